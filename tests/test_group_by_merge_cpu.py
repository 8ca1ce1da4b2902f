"""Merging partial group-by results (FJ_ALGO_GROUP_BY | FJ_ALGO_AGG_ALL | FJ_ALGO_AGG_MERGE, csrc/fj_groupby_merge.hip;
api.group_by_merge, api.GroupByAccumulator): what needs no GPU - the flag and its mirror, the unchanged ABI, every refusal the header
lists before any device work (fj_join_device on a NULL context with fake pointers that are never dereferenced, and fj_join_host before
its context exists), the valid combinations, the Python argument checks, and the NumPy reference the GPU tests compare with, on a
hand-written case."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

ROW_IDS, PO, BO = 0x80, 0x800, 0x1000
MIN, MAX, SIGNED, GB, INVERSE, ACC, FLOAT, ALL, ARG, MERGE = 0x4000, 0x8000, 0x10000, 0x40000, 0x100000, 0x1000000, 0x2000000, 0x4000000, 0x8000000, 0x10000000
V = GB | ALL | MERGE                                                      # the one valid setting of the bit
KINDS = ("unsigned", "signed", "float")
IDENTITY = {   # kind: (sum, min, max) of a partial row that no input row stands behind, as words
    "unsigned": (0, 2**64 - 1, 0),
    "signed": (0, 2**63 - 1, 2**63),
    "float": (0, 0x7FF0000000000000, 0xFFF0000000000000),                # +0.0, +inf, -inf
}


def ref_merge(keys, counts, sums, mins, maxs, kind):
    """the partial rows (uint64 keys, and four columns of 8-byte words) merged by key, nothing of the library: a dict of arrays aligned
    with the sorted distinct keys - "keys", "count" (uint64, wrapping), "sum", "min", "max" as uint64 words (kind "float": float64
    numbers; the sum with np.add.at in row order, exact for the multiples of 2^-10 the tests use)"""
    keys = np.asarray(keys, dtype=np.uint64)
    w = [np.ascontiguousarray(c).reshape(-1).view(np.uint64) for c in (counts, sums, mins, maxs)]
    uk, inv = np.unique(keys, return_inverse=True)
    inv = inv.reshape(-1)
    g = uk.size
    r = {"keys": uk, "count": np.zeros(g, np.uint64)}
    np.add.at(r["count"], inv, w[0])                                       # wraps modulo 2^64
    if kind == "float":
        f = [c.view(np.float64) for c in w[1:]]
        r["sum"] = np.zeros(g, np.float64); np.add.at(r["sum"], inv, f[0])
        r["min"] = np.full(g, np.inf); np.minimum.at(r["min"], inv, f[1])
        r["max"] = np.full(g, -np.inf); np.maximum.at(r["max"], inv, f[2])
        return r
    dt = np.int64 if kind == "signed" else np.uint64
    lo, hi = (np.iinfo(dt).min, np.iinfo(dt).max)
    r["sum"] = np.zeros(g, np.uint64); np.add.at(r["sum"], inv, w[1])
    mn = np.full(g, hi, dt); np.minimum.at(mn, inv, w[2].view(dt))
    mx = np.full(g, lo, dt); np.maximum.at(mx, inv, w[3].view(dt))
    r["min"], r["max"] = mn.view(np.uint64), mx.view(np.uint64)
    return r


def test_header_flag_and_python_mirror():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    assert int(re.search(r"#define FJ_ALGO_AGG_MERGE\s+(0x[0-9a-fA-F]+)", hdr).group(1), 16) == 0x10000000
    from flash_hash_join_amd import api
    assert api.ALGO_AGG_MERGE == 0x10000000


def test_no_other_define_has_the_bit_and_0x200000_is_still_unassigned():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    algos = {name: int(val, 16) for name, val in re.findall(r"#define (FJ_ALGO_[A-Z_]+)\s+(0x[0-9a-fA-F]+)", hdr)}
    assert [n for n, v in algos.items() if v & MERGE] == ["FJ_ALGO_AGG_MERGE"]
    assert not any(v & 0x200000 for v in algos.values())
    from flash_hash_join_amd import api
    mirrors = {n: v for n, v in vars(api).items() if n.startswith("ALGO_") and isinstance(v, int)}
    assert [n for n, v in mirrors.items() if v & MERGE] == ["ALGO_AGG_MERGE"] and not any(v & 0x200000 for v in mirrors.values())


def test_abi_version_and_function_count_are_unchanged():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    assert int(re.search(r"#define FJ_ABI_VERSION (\d+)", hdr).group(1)) == 8
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert len(set(re.findall(r"\b(fj_[a-z0-9_]+)\s*\(", code))) == 40
    assert "FJ_ALGO_AGG_MERGE" in hdr                                 # (what makes this test one of the new feature's)
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_abi_version() == 8 and len(_lib.SYMBOLS) == 40


def test_flash_join_exposes_the_function_and_the_class():
    import flash_join
    from flash_hash_join_amd import api
    for name in ("group_by_merge", "GroupByAccumulator", "group_by_accumulator"):
        assert callable(getattr(flash_join, name)) and name in api.EXTENSIONS and name in api.__all__
    assert isinstance(flash_join.group_by_accumulator(compact_at=7), flash_join.GroupByAccumulator)


def _device_call(algo, materialize=1, vals=0x20000, pk=None, n_p=0, ok=0x40000, ov=0x50000, cap=100, nb=100):
    from flash_hash_join_amd import _lib
    cnt = ctypes.c_uint64(0)
    rc = _lib.load().fj_join_device(None, algo, 0, materialize, 0x10000, vals, nb, pk, n_p, None, 64, ctypes.byref(cnt), ok, ov, cap, None)
    return rc, _lib.last_error()


UNKNOWN = [MERGE, MERGE | 1, MERGE | 2, GB | MERGE, GB | MERGE | SIGNED, ALL | MERGE, ALL | MERGE | FLOAT, MERGE | BO, MERGE | BO | MIN,
           MERGE | PO, MERGE | PO | ROW_IDS, GB | MERGE | MIN, GB | MERGE | ARG | MIN, GB | MERGE | INVERSE]


def test_the_bit_outside_its_one_combination_is_an_unknown_algo():
    for algo in UNKNOWN:
        rc, err = _device_call(algo=algo)
        assert rc != 0 and "unknown algo" in err and str(algo) in err and "null context" not in err, (hex(algo), err)


def test_the_neighbouring_bits_stay_what_they_were():
    """0x400, 0x2000, 0x20000, 0x80000 and 0x200000 are unknown algos beside the new combination too; GB | ACCUMULATE stays one"""
    for algo in (V | 0x400, V | 0x2000, V | 0x20000, V | 0x80000, V | 0x200000, GB | ACC, V | ACC, V | 3):
        rc, err = _device_call(algo=algo)
        assert rc != 0 and "unknown algo" in err and "null context" not in err, (hex(algo), err)


DEVICE_REFUSALS = [   # id, keyword arguments of _device_call, needles
    ("count_only", dict(algo=V, materialize=0), ("FJ_ALGO_AGG_MERGE", "materialize = 1")),
    ("no_values", dict(algo=V, vals=None), ("FJ_ALGO_AGG_MERGE", "d_build_vals")),
    ("no_values_float", dict(algo=V | FLOAT, vals=None), ("FJ_ALGO_AGG_MERGE", "d_build_vals")),
    ("no_keys_output", dict(algo=V | SIGNED, ok=None), ("FJ_ALGO_AGG_MERGE", "d_out_keys")),
    ("no_vals_output", dict(algo=V | 2, ov=None), ("FJ_ALGO_AGG_MERGE", "d_out_vals")),
    ("zero_capacity", dict(algo=V, cap=0), ("FJ_ALGO_AGG_MERGE", "capacity")),
    ("probe_keys", dict(algo=V, pk=0x30000), ("FJ_ALGO_AGG_MERGE", "no probe side")),
    ("probe_rows", dict(algo=V | 2, n_p=7), ("FJ_ALGO_AGG_MERGE", "no probe side")),
    ("min", dict(algo=V | MIN), ("FJ_ALGO_AGG_MERGE cannot be combined with FJ_ALGO_AGG_MIN",)),
    ("max", dict(algo=V | MAX | 2), ("FJ_ALGO_AGG_MERGE cannot be combined with FJ_ALGO_AGG_MAX",)),
    ("max_signed", dict(algo=V | MAX | SIGNED), ("FJ_ALGO_AGG_MERGE cannot be combined with FJ_ALGO_AGG_MAX",)),
    ("row_ids", dict(algo=V | ROW_IDS), ("FJ_ALGO_AGG_MERGE cannot be combined with FJ_ALGO_ROW_IDS",)),
    ("inverse", dict(algo=V | INVERSE | 1), ("FJ_ALGO_AGG_MERGE cannot be combined with FJ_ALGO_INVERSE",)),
    ("agg_arg", dict(algo=V | ARG), ("FJ_ALGO_AGG_MERGE cannot be combined with FJ_ALGO_AGG_ARG",)),
    ("agg_arg_min", dict(algo=V | ARG | MIN), ("FJ_ALGO_AGG_MERGE cannot be combined with",)),
    ("many", dict(algo=V | 0x10), ("FJ_ALGO_AGG_MERGE cannot be combined with FJ_ALGO_MANY_TO_MANY",)),
    ("left", dict(algo=V | 0x20), ("FJ_ALGO_AGG_MERGE cannot be combined with FJ_ALGO_LEFT_OUTER",)),
    ("build_order", dict(algo=V | BO), ("FJ_ALGO_AGG_MERGE cannot be combined with FJ_ALGO_BUILD_ORDER",)),
    ("signed_and_float", dict(algo=V | SIGNED | FLOAT), ("FJ_ALGO_AGG_MERGE", "FJ_ALGO_AGG_FLOAT cannot be combined with FJ_ALGO_AGG_SIGNED")),
    ("misaligned_keys", dict(algo=V, ok=0x40004), ("8-byte aligned",)),
    ("misaligned_vals", dict(algo=V | FLOAT, ov=0x50004), ("8-byte aligned",)),
    ("misaligned_input", dict(algo=V, vals=0x20008), ("16-byte aligned",)),
]


@pytest.mark.parametrize("cid,kw,needles", DEVICE_REFUSALS, ids=[r[0] for r in DEVICE_REFUSALS])
def test_invalid_combinations_are_refused_before_any_device_work(cid, kw, needles):
    """A NULL context: the checks come before the context is touched (the pointers are never dereferenced)."""
    rc, err = _device_call(**kw)
    assert rc != 0 and "null context" not in err, err
    for needle in needles:
        assert needle in err, err


VALID = [(f"{('adaptive', 'scalar', 'radix')[base]}-{fid}-cap{cap}", dict(algo=V | base | flags, cap=cap))
         for base in (0, 1, 2) for fid, flags in (("unsigned", 0), ("signed", SIGNED), ("float", FLOAT)) for cap in (1, 5000)]


@pytest.mark.parametrize("cid,kw", VALID, ids=[v[0] for v in VALID])
def test_valid_combinations_reach_the_context(cid, kw):
    """the nine combinations, with room for one group and with more room than rows: any capacity >= 1 passes the checks"""
    rc, err = _device_call(**kw)
    assert rc != 0 and "null context" in err, err


def test_no_rows_need_no_buffers():
    rc, err = _device_call(algo=V, nb=0, vals=None, ok=None, ov=None, cap=0)
    assert rc != 0 and "null context" in err, err


def test_the_four_aggregate_form_keeps_its_own_messages():
    rc, err = _device_call(algo=GB | ALL | MIN)
    assert rc != 0 and "FJ_ALGO_AGG_ALL cannot be combined with FJ_ALGO_AGG_MIN" in err and "MERGE" not in err, err
    rc, err = _device_call(algo=GB | ALL, vals=None)
    assert rc != 0 and "FJ_ALGO_AGG_ALL" in err and "MERGE" not in err, err


HOST_REFUSALS = [   # id, algo, materialize, values, out_keys, out_vals, probe rows, needles
    ("bare_bit", MERGE, 1, True, True, True, 0, ("unknown algo",)),
    ("group_by_alone", GB | MERGE, 1, True, True, True, 0, ("unknown algo",)),
    ("all_alone", ALL | MERGE, 1, True, True, True, 0, ("unknown algo",)),
    ("with_build_order", MERGE | BO, 1, True, True, True, 0, ("unknown algo",)),
    ("with_probe_order", MERGE | PO, 1, True, True, True, 0, ("unknown algo",)),
    ("unknown_base", V | 3, 1, True, True, True, 0, ("unknown algo",)),
    ("unknown_bit", V | 0x80000, 1, True, True, True, 0, ("unknown algo",)),
    ("count_only", V, 0, True, True, True, 0, ("FJ_ALGO_AGG_MERGE", "materialize = 1")),
    ("no_values", V | SIGNED, 1, False, True, True, 0, ("FJ_ALGO_AGG_MERGE", "build_vals")),
    ("no_keys_output", V, 1, True, False, True, 0, ("FJ_ALGO_AGG_MERGE", "out_keys")),
    ("no_vals_output", V | FLOAT, 1, True, True, False, 0, ("FJ_ALGO_AGG_MERGE", "out_vals")),
    ("probe_rows", V, 1, True, True, True, 8, ("FJ_ALGO_AGG_MERGE", "no probe side")),
    ("min", V | MIN, 1, True, True, True, 0, ("FJ_ALGO_AGG_MERGE cannot be combined with FJ_ALGO_AGG_MIN",)),
    ("max", V | MAX | 2, 1, True, True, True, 0, ("FJ_ALGO_AGG_MERGE cannot be combined with FJ_ALGO_AGG_MAX",)),
    ("row_ids", V | ROW_IDS, 1, True, True, True, 0, ("FJ_ALGO_AGG_MERGE cannot be combined with FJ_ALGO_ROW_IDS",)),
    ("inverse", V | INVERSE, 1, True, True, True, 0, ("FJ_ALGO_AGG_MERGE cannot be combined with FJ_ALGO_INVERSE",)),
    ("agg_arg", V | ARG, 1, True, True, True, 0, ("FJ_ALGO_AGG_MERGE cannot be combined with FJ_ALGO_AGG_ARG",)),
    ("many", V | 0x10, 1, True, True, True, 0, ("FJ_ALGO_AGG_MERGE cannot be combined with FJ_ALGO_MANY_TO_MANY",)),
    ("left", V | 0x20, 1, True, True, True, 0, ("FJ_ALGO_AGG_MERGE cannot be combined with FJ_ALGO_LEFT_OUTER",)),
    ("build_order", V | BO, 1, True, True, True, 0, ("FJ_ALGO_AGG_MERGE cannot be combined with FJ_ALGO_BUILD_ORDER",)),
    ("signed_and_float", V | SIGNED | FLOAT, 1, True, True, True, 0, ("FJ_ALGO_AGG_MERGE", "FJ_ALGO_AGG_FLOAT cannot be combined with FJ_ALGO_AGG_SIGNED")),
]


@pytest.mark.parametrize("cid,algo,materialize,vals,want_ok,want_ov,n_p,needles", HOST_REFUSALS, ids=[r[0] for r in HOST_REFUSALS])
def test_host_entry_refusals(cid, algo, materialize, vals, want_ok, want_ov, n_p, needles):
    """fj_join_host makes the same checks before its context is created"""
    from flash_hash_join_amd import _lib
    L = _lib.load()
    k = np.arange(8, dtype=np.uint64)
    v = np.zeros(32, dtype=np.uint64)
    cnt, sec = ctypes.c_uint64(0), ctypes.c_double(0)
    ok, ov = ctypes.c_void_p(), ctypes.c_void_p()
    rc = L.fj_join_host(algo, 0, materialize, k.ctypes.data, v.ctypes.data if vals else None, 8, k.ctypes.data if n_p else None, n_p,
                        ctypes.byref(cnt), ctypes.byref(sec), ctypes.byref(ok) if want_ok else None, ctypes.byref(ov) if want_ov else None)
    err = _lib.last_error()
    assert rc != 0 and "null context" not in err and "HIP device" not in err, err
    for needle in needles:
        assert needle in err, err
    assert not ok.value and not ov.value


def test_python_argument_errors():
    from flash_hash_join_amd import api
    k = np.arange(4, dtype=np.uint64)
    c = np.ones(4, dtype=np.int64)
    f = k.astype(np.float64)
    with pytest.raises(ValueError, match="maxs has 3 elements, keys has 4"):
        api.group_by_merge(k, c, k, k, k[:3])
    with pytest.raises(ValueError, match="counts has 5 elements, keys has 4"):
        api.group_by_merge(k, np.ones(5, np.int64), k, k, k)
    with pytest.raises(ValueError, match="sums has 2 elements, keys has 4"):
        api.group_by_merge([k, k], [c, c], [k, k[:2]], [k, k], [k, k])
    with pytest.raises(ValueError, match="mins has 1 arrays, keys has 2"):
        api.group_by_merge([k, k], [c, c], [k, k], [k], [k, k])
    with pytest.raises(TypeError, match="float64=True needs floating-point sums"):
        api.group_by_merge(k, c, k, f, f, float64=True)
    with pytest.raises(TypeError, match="float64=True needs floating-point maxs"):
        api.group_by_merge(k, c, f, f, k.astype(np.int64), float64=True)
    for signed in (True, False):
        with pytest.raises(TypeError, match="signed must be None with float64=True"):
            api.group_by_merge(k, c, f, f, f, signed=signed, float64=True)
        with pytest.raises(TypeError, match="signed must be None with float64=True"):
            api.GroupByAccumulator(signed=signed, float64=True)
    with pytest.raises(TypeError, match="signed must be None, True or False"):
        api.group_by_merge(k, c, k, k, k, signed="yes")
    with pytest.raises(TypeError, match="mins must be integers"):
        api.group_by_merge(k, c, k, f, k)                                 # a float column without float64=True has no integer order
    with pytest.raises(TypeError, match="counts must be int64 or uint64"):
        api.group_by_merge(k, c.astype(np.int32), k, k, k)
    with pytest.raises(TypeError, match="counts must be int64 or uint64"):
        api.group_by_merge(k, f, f, f, f, float64=True)
    for bad in (0, -1, 1.5, "3", True):
        with pytest.raises(ValueError, match="max_groups must be None or an integer >= 1"):
            api.group_by_merge(k, c, k, k, k, max_groups=bad)
        with pytest.raises(ValueError, match="max_groups must be None or an integer >= 1"):
            api.GroupByAccumulator(max_groups=bad)
        with pytest.raises(ValueError, match="compact_at must be an integer >= 1"):
            api.GroupByAccumulator(compact_at=bad)
    acc = api.GroupByAccumulator()
    with pytest.raises(ValueError, match="unknown aggregate 'median'"):
        acc.result(aggs=("sum", "median"))
    with pytest.raises(ValueError, match="'mean' needs float64=True"):
        acc.result(aggs=("count", "mean"))
    with pytest.raises(ValueError, match="aggs is empty"):
        acc.result(aggs=())
    with pytest.raises(TypeError, match="another GroupByAccumulator, or a"):
        acc.merge((k, c, k))
    with pytest.raises(TypeError, match="one accumulator is float64"):
        acc.merge(api.GroupByAccumulator(float64=True))


def test_an_accumulator_without_a_batch_and_a_merge_of_no_rows_are_empty():
    """neither touches the library: no row, no call"""
    from flash_hash_join_amd import api
    e = np.empty(0, np.uint64)
    for out in (api.group_by_merge(e, e, e, e, e), api.group_by_merge([], [], [], [], []), api.group_by_merge([e, e], [e, e], [e, e], [e, e], [e, e])):
        assert out[:2] == (0, 0.0) and len(out) == 7 and all(isinstance(a, np.ndarray) and a.shape == (0,) for a in out[2:])
        assert out[2].dtype == np.uint64 and out[3].dtype == np.int64
    out = api.group_by_merge(e, e, e.view(np.float64), e.view(np.float64), e.view(np.float64), float64=True)
    assert out[:2] == (0, 0.0) and [a.dtype for a in out[3:]] == [np.int64, np.float64, np.float64, np.float64]
    with api.GroupByAccumulator(float64=True) as acc:
        assert (acc.num_groups, acc.pending_rows, acc.rows_seen, acc.merges) == (0, 0, 0, 0)
        out = acc.result(aggs=("mean", "count"))
        assert out[:2] == (0, 0.0) and len(out) == 5 and out[3].dtype == np.float64 and out[4].dtype == np.int64 and out[3].shape == (0,)
        assert acc.merge(api.GroupByAccumulator(float64=True)) == 0.0 and acc.merges == 0
    with pytest.raises(ValueError, match="closed"):
        acc.result()


def test_numpy_reference_on_a_hand_written_case():
    u = lambda *a: np.array(a, dtype=np.uint64)
    keys = u(7, 5, 7, 2**64 - 1, 7, 5, 9)
    counts = u(2**33, 1, 2**33, 3, 2**33, 0, 0)
    sums = u(2**63, 4, 2**63, 10, 5, 0, 0)
    r = ref_merge(keys, counts, sums, u(3, 4, 2**64 - 5, 1, 9, 2**64 - 1, 2**64 - 1), u(3, 4, 2**64 - 5, 8, 9, 0, 0), "unsigned")
    assert r["keys"].tolist() == [5, 7, 9, 2**64 - 1] and r["count"].tolist() == [1, 3 * 2**33, 0, 3]
    assert r["sum"].tolist() == [4, 5, 0, 10]                             # 2^63 + 2^63 + 5 wraps to 5
    assert r["min"].tolist() == [4, 3, 2**64 - 1, 1] and r["max"].tolist() == [4, 2**64 - 5, 0, 8]      # key 9: the identities stay
    sid = IDENTITY["signed"]
    r = ref_merge(keys, counts, sums, u(3, 4, 2**64 - 5, 1, 9, sid[1], sid[1]), u(3, 4, 2**64 - 5, 8, 9, sid[2], sid[2]), "signed")
    assert r["min"].view(np.int64).tolist() == [4, -5, 2**63 - 1, 1] and r["max"].view(np.int64).tolist() == [4, 9, -2**63, 8]
    f = lambda *a: np.array(a, dtype=np.float64)
    r = ref_merge(u(1, 2, 1, 2), u(1, 0, 2, 0), f(0.5, 0.0, -2.25, 0.0), f(0.5, np.inf, -2.0, np.inf), f(0.5, -np.inf, -0.25, -np.inf), "float")
    assert r["count"].tolist() == [3, 0] and r["sum"].tolist() == [-1.75, 0.0]
    assert r["min"].tolist() == [-2.0, np.inf] and r["max"].tolist() == [0.5, -np.inf]
    assert f(0.0, np.inf, -np.inf).view(np.uint64).tolist() == list(IDENTITY["float"])
    r = ref_merge(np.empty(0, np.uint64), *([np.empty(0, np.uint64)] * 4), "unsigned")
    assert all(a.size == 0 for a in r.values())
