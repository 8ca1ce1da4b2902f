"""The row that holds each group's minimum / maximum (FJ_ALGO_GROUP_BY | FJ_ALGO_AGG_ARG, csrc/fj_groupby_arg.hip; api.group_by_argmin,
api.group_by_argmax): what needs no GPU - the flag and its mirror, the unchanged ABI, every refusal the header lists before any device
work (fj_join_device on a NULL context with fake pointers that are never dereferenced, and fj_join_host before its context exists),
the valid combinations, the Python argument checks, and the NumPy reference the GPU tests compare with on a hand-written case."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

ROW_IDS, PO, BO = 0x80, 0x800, 0x1000
MIN, MAX, SIGNED, GB, INVERSE, FLOAT, ALL, ARG = 0x4000, 0x8000, 0x10000, 0x40000, 0x100000, 0x2000000, 0x4000000, 0x8000000
KINDS = ("unsigned", "signed", "float")


def ref_group_by_arg(keys, vals, kind, is_max):
    """dict of arrays aligned with the sorted distinct keys 'keys': 'index' (int64), the smallest row whose value is the group's minimum
    (is_max: maximum), and 'value', vals[index].  vals: 8-byte words (uint64 / int64) read as `kind` says - "unsigned", "signed" - or,
    for "float", a float64 column.  A lexsort by (key, value in the kind's order, position): the first row of each group is the argmin;
    the argmax is the first position of the group's LAST run of equal values.  Floats compare as numbers (-0.0 == +0.0: one run).
    Nothing of the library"""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1)
    vals = np.asarray(vals).reshape(-1)
    assert kind in KINDS and vals.size == keys.size and vals.dtype.itemsize == 8
    if kind == "float":
        assert vals.dtype == np.float64
        v = vals
    else:
        assert vals.dtype.kind in "iu"
        v = vals.view(np.uint64 if kind == "unsigned" else np.int64)
    n = keys.size
    if n == 0:
        return {"keys": keys.copy(), "index": np.empty(0, np.int64), "value": vals.copy()}
    o = np.lexsort((np.arange(n), v, keys))                   # (last key first: by key, then value, then position)
    ks, vs = keys[o], v[o]
    first = np.concatenate([[True], ks[1:] != ks[:-1]])
    starts = np.flatnonzero(first)
    if not is_max:
        pick = starts
    else:
        run = first | np.concatenate([[True], vs[1:] != vs[:-1]])
        run_start = np.maximum.accumulate(np.where(run, np.arange(n), 0))
        ends = np.concatenate([starts[1:], [n]]) - 1
        pick = run_start[ends]
    idx = o[pick].astype(np.int64)
    return {"keys": ks[starts], "index": idx, "value": vals[idx]}


def test_header_flag_and_python_mirror():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    assert int(re.search(r"#define FJ_ALGO_AGG_ARG\s+(0x[0-9a-fA-F]+)", hdr).group(1), 16) == 0x8000000
    from flash_hash_join_amd import api
    assert api.ALGO_AGG_ARG == 0x8000000


def test_no_other_define_has_the_bit_and_0x200000_is_still_unassigned():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    algos = {name: int(val, 16) for name, val in re.findall(r"#define (FJ_ALGO_[A-Z_]+)\s+(0x[0-9a-fA-F]+)", hdr)}
    assert algos["FJ_ALGO_AGG_ARG"] == ARG
    assert [n for n, v in algos.items() if v & ARG] == ["FJ_ALGO_AGG_ARG"]
    assert not any(v & 0x200000 for v in algos.values())
    from flash_hash_join_amd import api
    mirrors = {n: v for n, v in vars(api).items() if n.startswith("ALGO_") and isinstance(v, int)}
    assert [n for n, v in mirrors.items() if v & ARG] == ["ALGO_AGG_ARG"] and not any(v & 0x200000 for v in mirrors.values())


def test_abi_version_and_function_count_are_unchanged():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    assert int(re.search(r"#define FJ_ABI_VERSION (\d+)", hdr).group(1)) == 8
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert len(set(re.findall(r"\b(fj_[a-z0-9_]+)\s*\(", code))) == 40
    assert "FJ_ALGO_AGG_ARG" in hdr                                   # (what makes this test one of the new feature's)
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_abi_version() == 8 and len(_lib.SYMBOLS) == 40


def test_flash_join_exposes_the_functions():
    import flash_join
    from flash_hash_join_amd import api
    for name in ("group_by_argmin", "group_by_argmax"):
        assert callable(getattr(flash_join, name)) and name in api.EXTENSIONS and name in api.__all__


def _device_call(algo, materialize=1, vals=0x20000, pk=None, n_p=0, ok=0x40000, ov=0x50000, cap=100, nb=100):
    from flash_hash_join_amd import _lib
    cnt = ctypes.c_uint64(0)
    rc = _lib.load().fj_join_device(None, algo, 0, materialize, 0x10000, vals, nb, pk, n_p, None, 64, ctypes.byref(cnt), ok, ov, cap, None)
    return rc, _lib.last_error()


DEVICE_REFUSALS = [   # id, keyword arguments of _device_call, needles
    ("without_group_by", dict(algo=ARG | MIN), ("unknown algo",)),
    ("without_group_by_radix_signed", dict(algo=ARG | MAX | SIGNED | 2), ("unknown algo",)),
    ("with_build_order", dict(algo=ARG | BO | MIN), ("unknown algo",)),
    ("with_probe_order", dict(algo=ARG | PO), ("unknown algo",)),
    ("neither_min_nor_max", dict(algo=GB | ARG), ("FJ_ALGO_AGG_ARG needs exactly one of FJ_ALGO_AGG_MIN and FJ_ALGO_AGG_MAX", "neither")),
    ("neither_signed", dict(algo=GB | ARG | SIGNED | 2), ("FJ_ALGO_AGG_ARG needs exactly one of FJ_ALGO_AGG_MIN and FJ_ALGO_AGG_MAX",)),
    ("both_min_and_max", dict(algo=GB | ARG | MIN | MAX), ("FJ_ALGO_AGG_ARG needs exactly one of FJ_ALGO_AGG_MIN and FJ_ALGO_AGG_MAX", "both")),
    ("row_ids", dict(algo=GB | ARG | MIN | ROW_IDS), ("FJ_ALGO_AGG_ARG cannot be combined with FJ_ALGO_ROW_IDS",)),
    ("inverse", dict(algo=GB | ARG | MAX | INVERSE | 1), ("FJ_ALGO_AGG_ARG cannot be combined with FJ_ALGO_INVERSE",)),
    ("agg_all", dict(algo=GB | ARG | ALL), ("FJ_ALGO_AGG_ARG cannot be combined with FJ_ALGO_AGG_ALL",)),
    ("agg_all_min", dict(algo=GB | ARG | ALL | MIN), ("FJ_ALGO_AGG_A",)),          # (either form's message names its flags)
    ("signed_and_float", dict(algo=GB | ARG | MIN | SIGNED | FLOAT), ("FJ_ALGO_AGG_FLOAT cannot be combined with FJ_ALGO_AGG_SIGNED",)),
    ("count_only", dict(algo=GB | ARG | MIN, materialize=0), ("FJ_ALGO_AGG_ARG", "materialize = 1")),
    ("no_values", dict(algo=GB | ARG | MAX, vals=None), ("FJ_ALGO_AGG_ARG", "d_build_vals")),
    ("no_values_float", dict(algo=GB | ARG | MIN | FLOAT, vals=None), ("FJ_ALGO_AGG_ARG", "d_build_vals")),
    ("no_keys_output", dict(algo=GB | ARG | MIN | SIGNED, ok=None), ("FJ_ALGO_AGG_ARG", "d_out_keys")),
    ("no_vals_output", dict(algo=GB | ARG | MAX | 2, ov=None), ("FJ_ALGO_AGG_ARG", "d_out_vals")),
    ("capacity_below_nb", dict(algo=GB | ARG | MIN, cap=99), ("output capacity 99 < 100 rows",)),
    ("zero_capacity", dict(algo=GB | ARG | MAX | FLOAT, cap=0), ("output capacity 0 < 100 rows",)),
    ("misaligned_keys", dict(algo=GB | ARG | MIN, ok=0x40004), ("8-byte aligned",)),
    ("misaligned_vals", dict(algo=GB | ARG | MAX | FLOAT, ov=0x50004), ("8-byte aligned",)),
    ("probe_keys", dict(algo=GB | ARG | MIN, pk=0x30000), ("FJ_ALGO_GROUP_BY", "no probe side")),
    ("probe_rows", dict(algo=GB | ARG | MAX | 2, n_p=7), ("FJ_ALGO_GROUP_BY", "no probe side")),
    ("many", dict(algo=GB | ARG | MIN | 0x10), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_MANY_TO_MANY",)),
    ("build_order", dict(algo=GB | ARG | MIN | BO), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_BUILD_ORDER",)),
    ("unknown_base", dict(algo=GB | ARG | MIN | 3), ("unknown algo",)),
    ("unknown_bit_0x80000", dict(algo=GB | ARG | MIN | 0x80000), ("unknown algo",)),
    ("unknown_bit_0x200000", dict(algo=GB | ARG | MAX | 0x200000), ("unknown algo",)),
    ("misaligned_input", dict(algo=GB | ARG | MIN, vals=0x20008), ("16-byte aligned",)),
]


@pytest.mark.parametrize("cid,kw,needles", DEVICE_REFUSALS, ids=[r[0] for r in DEVICE_REFUSALS])
def test_invalid_combinations_are_refused_before_any_device_work(cid, kw, needles):
    """A NULL context: the checks come before the context is touched (the pointers are never dereferenced)."""
    rc, err = _device_call(**kw)
    assert rc != 0 and "null context" not in err, err
    for needle in needles:
        assert needle in err, err


def test_row_ids_with_min_or_max_stays_refused_without_the_flag():
    for agg, name in ((MIN, "MIN"), (MAX, "MAX")):
        rc, err = _device_call(algo=GB | ROW_IDS | agg)
        assert rc != 0 and f"FJ_ALGO_ROW_IDS cannot be combined with FJ_ALGO_AGG_{name}" in err and "null context" not in err, err


VALID = [(f"{('adaptive', 'scalar', 'radix')[base]}-{aid}-{fid}-cap{cap}", dict(algo=GB | ARG | agg | base | flags, cap=cap))
         for base in (0, 1, 2) for aid, agg in (("min", MIN), ("max", MAX))
         for fid, flags in (("unsigned", 0), ("signed", SIGNED), ("float", FLOAT)) for cap in (100, 5000)]


@pytest.mark.parametrize("cid,kw", VALID, ids=[v[0] for v in VALID])
def test_valid_combinations_reach_the_context(cid, kw):
    """nb = 100 with room for exactly nb groups, and with more room than rows"""
    rc, err = _device_call(**kw)
    assert rc != 0 and "null context" in err, err


def test_an_empty_relation_needs_no_buffers():
    rc, err = _device_call(algo=GB | ARG | MIN, nb=0, vals=None, ok=None, ov=None, cap=0)
    assert rc != 0 and "null context" in err, err


def test_the_bare_bit_is_an_unknown_algo():
    for algo in (ARG, ARG | 1, ARG | MIN, ARG | MAX | 2, ARG | BO, ARG | BO | MIN, ARG | PO, ARG | PO | ROW_IDS, ARG | SIGNED, ARG | FLOAT, ARG | ALL):
        rc, err = _device_call(algo=algo)
        assert rc != 0 and "unknown algo" in err and "null context" not in err, (hex(algo), err)


HOST_REFUSALS = [   # id, algo, materialize, values, out_keys, out_vals, probe, needles
    ("bare_bit", ARG | MIN, 1, True, True, True, False, ("unknown algo",)),
    ("with_build_order", ARG | BO | MAX, 1, True, True, True, False, ("unknown algo",)),
    ("with_probe_order", ARG | PO, 1, True, True, True, False, ("unknown algo",)),
    ("neither_min_nor_max", GB | ARG, 1, True, True, True, False, ("FJ_ALGO_AGG_ARG needs exactly one of FJ_ALGO_AGG_MIN and FJ_ALGO_AGG_MAX", "neither")),
    ("both_min_and_max", GB | ARG | MIN | MAX | 2, 1, True, True, True, False, ("FJ_ALGO_AGG_ARG needs exactly one of FJ_ALGO_AGG_MIN and FJ_ALGO_AGG_MAX", "both")),
    ("row_ids", GB | ARG | MIN | ROW_IDS, 1, True, True, True, False, ("FJ_ALGO_AGG_ARG cannot be combined with FJ_ALGO_ROW_IDS",)),
    ("inverse", GB | ARG | MAX | INVERSE, 1, True, True, True, False, ("FJ_ALGO_AGG_ARG cannot be combined with FJ_ALGO_INVERSE",)),
    ("agg_all", GB | ARG | ALL, 1, True, True, True, False, ("FJ_ALGO_AGG_ARG cannot be combined with FJ_ALGO_AGG_ALL",)),
    ("signed_and_float", GB | ARG | MAX | SIGNED | FLOAT, 1, True, True, True, False, ("FJ_ALGO_AGG_FLOAT cannot be combined with FJ_ALGO_AGG_SIGNED",)),
    ("count_only", GB | ARG | MIN, 0, True, True, True, False, ("FJ_ALGO_AGG_ARG", "materialize = 1")),
    ("no_values", GB | ARG | MIN | SIGNED, 1, False, True, True, False, ("FJ_ALGO_AGG_ARG", "build_vals")),
    ("no_keys_output", GB | ARG | MAX, 1, True, False, True, False, ("FJ_ALGO_AGG_ARG", "out_keys")),
    ("no_vals_output", GB | ARG | MIN | FLOAT, 1, True, True, False, False, ("FJ_ALGO_AGG_ARG", "out_vals")),
    ("probe_side", GB | ARG | MIN, 1, True, True, True, True, ("FJ_ALGO_GROUP_BY", "no probe side")),
    ("many", GB | ARG | MIN | 0x10, 1, True, True, True, False, ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_MANY_TO_MANY",)),
    ("unknown_base", GB | ARG | MAX | 3, 1, True, True, True, False, ("unknown algo",)),
    ("unknown_bit_0x80000", GB | ARG | MIN | 0x80000, 1, True, True, True, False, ("unknown algo",)),
    ("unknown_bit_0x200000", GB | ARG | MIN | 0x200000, 1, True, True, True, False, ("unknown algo",)),
    ("row_ids_min_without_the_flag", GB | ROW_IDS | MIN, 1, True, True, True, False, ("FJ_ALGO_ROW_IDS cannot be combined with FJ_ALGO_AGG_MIN",)),
]


@pytest.mark.parametrize("cid,algo,materialize,vals,want_ok,want_ov,probe,needles", HOST_REFUSALS, ids=[r[0] for r in HOST_REFUSALS])
def test_host_entry_refusals(cid, algo, materialize, vals, want_ok, want_ov, probe, needles):
    """fj_join_host makes the same checks before its context is created"""
    from flash_hash_join_amd import _lib
    L = _lib.load()
    k = np.arange(8, dtype=np.uint64)
    cnt, sec = ctypes.c_uint64(0), ctypes.c_double(0)
    ok, ov = ctypes.c_void_p(), ctypes.c_void_p()
    rc = L.fj_join_host(algo, 0, materialize, k.ctypes.data, k.ctypes.data if vals else None, 8, k.ctypes.data if probe else None, 8 if probe else 0,
                        ctypes.byref(cnt), ctypes.byref(sec), ctypes.byref(ok) if want_ok else None, ctypes.byref(ov) if want_ov else None)
    err = _lib.last_error()
    assert rc != 0 and "null context" not in err and "HIP device" not in err, err
    for needle in needles:
        assert needle in err, err
    assert not ok.value and not ov.value


@pytest.mark.parametrize("name", ["group_by_argmin", "group_by_argmax"])
def test_python_argument_errors(name):
    from flash_hash_join_amd import api
    fn = getattr(api, name)
    k = np.arange(4, dtype=np.uint64)
    f = k.astype(np.float64)
    with pytest.raises(TypeError, match="float64=True needs floating-point values"):
        fn(k, k, float64=True)                                          # an integer column read as doubles
    with pytest.raises(TypeError, match="float64=True needs floating-point values"):
        fn(k, k.astype(np.int64), float64=True, return_values=True)
    for signed in (True, False):
        with pytest.raises(TypeError, match="signed must be None with float64=True"):
            fn(k, f, signed=signed, float64=True)
    with pytest.raises(ValueError, match="values has 3 elements, keys has 4"):
        fn(k, k[:3])
    with pytest.raises(ValueError, match="values has 5 elements, keys has 4"):
        fn(k, np.arange(5, dtype=np.float64), float64=True)
    with pytest.raises(ValueError, match=f"{name}: values is required"):
        fn(k, None)
    with pytest.raises(TypeError, match="signed must be None, True or False"):
        fn(k, k, signed="yes")
    with pytest.raises(TypeError, match="values must be integers"):
        fn(k, f)                                                        # a float column without float64=True has no integer order
    with pytest.raises(TypeError, match="keys"):
        fn(np.array(["a", "b", "c", "d"]), k)


def test_numpy_reference_on_a_hand_written_case():
    #                 row:  0  1  2       3  4  5           6       7  8  9
    keys = np.array([7, 5, 7, 2**64 - 1, 0, 7, 2**64 - 1, 9, 7, 5], dtype=np.uint64)
    vals = np.array([3, 4, 2**63, 2**63, 32, 1, 2**64 - 1, 0, 1, 4], dtype=np.uint64)
    # key 7 holds rows 0, 2, 5, 8 with 3, 2^63, 1, 1: the top bit makes row 2 the unsigned maximum and the signed minimum; 1 ties at 5 and 8
    r = ref_group_by_arg(keys, vals, "unsigned", False)
    assert r["keys"].tolist() == [0, 5, 7, 9, 2**64 - 1]
    assert r["index"].dtype == np.int64 and r["index"].tolist() == [4, 1, 5, 7, 3] and r["value"].tolist() == [32, 4, 1, 0, 2**63]
    r = ref_group_by_arg(keys, vals, "unsigned", True)
    assert r["index"].tolist() == [4, 1, 2, 7, 6] and r["value"].tolist() == [32, 4, 2**63, 0, 2**64 - 1]
    r = ref_group_by_arg(keys, vals.view(np.int64), "signed", False)
    assert r["index"].tolist() == [4, 1, 2, 7, 3] and r["value"].tolist() == [32, 4, -2**63, 0, -2**63]
    r = ref_group_by_arg(keys, vals.view(np.int64), "signed", True)
    assert r["index"].tolist() == [4, 1, 0, 7, 6] and r["value"].tolist() == [32, 4, 3, 0, -1]
    # floats: -0.0 before +0.0 tie (the first row wins for both extremes), a tie of the maximum, -inf as a minimum
    fk = np.array([3, 1, 3, 3, 1, 3, 1], dtype=np.uint64)
    fv = np.array([-0.0, 2.5, 0.0, -1.0, 2.5, 0.0, -np.inf])
    r = ref_group_by_arg(fk, fv, "float", True)
    assert r["keys"].tolist() == [1, 3] and r["index"].tolist() == [1, 0] and r["value"][0] == 2.5 and r["value"][1] == 0.0
    assert np.signbit(r["value"][1])                                                               # (row 0 is the -0.0)
    r = ref_group_by_arg(fk, fv, "float", False)
    assert r["index"].tolist() == [6, 3] and r["value"].tolist() == [-np.inf, -1.0]
    r = ref_group_by_arg(np.array([4, 4, 4], dtype=np.uint64), np.array([0.0, -0.0, 0.0]), "float", False)
    assert r["index"].tolist() == [0] and not np.signbit(r["value"][0])
    for kind, dt in (("unsigned", np.uint64), ("signed", np.int64), ("float", np.float64)):
        r = ref_group_by_arg(np.empty(0, np.uint64), np.empty(0, dt), kind, True)
        assert all(a.size == 0 for a in r.values())
