"""Group-by with count, sum, min and max of a column in one call (FJ_ALGO_GROUP_BY | FJ_ALGO_AGG_ALL, csrc/fj_groupby_multi.hip;
api.group_by_agg): what needs no GPU - the flag and its mirror, the unchanged ABI, every refusal the header lists before any device
work (fj_join_device on a NULL context with fake pointers that are never dereferenced, and fj_join_host before its context exists),
the valid combinations, the Python argument checks, and the NumPy reference the GPU tests compare with on a hand-written case."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT

ROW_IDS, PO, BO = 0x80, 0x800, 0x1000
MIN, MAX, SIGNED, GB, INVERSE, FLOAT, ALL = 0x4000, 0x8000, 0x10000, 0x40000, 0x100000, 0x2000000, 0x4000000
U64_MAX = np.uint64(2**64 - 1)


def ref_group_by_agg(keys, vals):
    """dict of arrays aligned with the sorted distinct keys 'keys': count, sum (wrapping uint64), min_u, max_u, min_s, max_s - np.unique
    and np.add.at / np.minimum.at / np.maximum.at over the uint64 and int64 words, nothing of the library"""
    keys, vals = np.asarray(keys, dtype=np.uint64), np.asarray(vals, dtype=np.uint64)
    uk, inv, cnt = np.unique(keys, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    g = uk.size
    r = {"keys": uk, "count": cnt.astype(np.int64)}
    r["sum"] = np.zeros(g, np.uint64); np.add.at(r["sum"], inv, vals)                       # wraps modulo 2^64
    r["min_u"] = np.full(g, U64_MAX, np.uint64); np.minimum.at(r["min_u"], inv, vals)
    r["max_u"] = np.zeros(g, np.uint64); np.maximum.at(r["max_u"], inv, vals)
    sv = vals.view(np.int64)
    r["min_s"] = np.full(g, np.iinfo(np.int64).max, np.int64); np.minimum.at(r["min_s"], inv, sv)
    r["max_s"] = np.full(g, np.iinfo(np.int64).min, np.int64); np.maximum.at(r["max_s"], inv, sv)
    return r


def ref_group_by_agg_float(keys, vals):
    """the float reference: count, min, max (np.minimum.at / np.maximum.at on float64), and per group the correctly rounded sum
    (math.fsum) and the sum of the absolute values, which scales the bound of an inexact sum"""
    keys, vals = np.asarray(keys, dtype=np.uint64), np.asarray(vals, dtype=np.float64)
    uk, inv, cnt = np.unique(keys, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    g = uk.size
    r = {"keys": uk, "count": cnt.astype(np.int64)}
    r["min"] = np.full(g, np.inf); np.minimum.at(r["min"], inv, vals)
    r["max"] = np.full(g, -np.inf); np.maximum.at(r["max"], inv, vals)
    order = np.argsort(inv, kind="stable")
    ends = np.cumsum(cnt)
    sv = vals[order]
    r["sum"] = np.array([math.fsum(sv[e - c:e]) for e, c in zip(ends, cnt)], dtype=np.float64)
    r["abs"] = np.array([math.fsum(np.abs(sv[e - c:e])) for e, c in zip(ends, cnt)], dtype=np.float64)
    return r


def test_header_flag_and_python_mirror():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    assert int(re.search(r"#define FJ_ALGO_AGG_ALL\s+(0x[0-9a-fA-F]+)", hdr).group(1), 16) == 0x4000000
    from flash_hash_join_amd import api
    assert api.ALGO_AGG_ALL == 0x4000000


def test_abi_version_and_function_count_are_unchanged():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    assert int(re.search(r"#define FJ_ABI_VERSION (\d+)", hdr).group(1)) == 8
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert len(set(re.findall(r"\b(fj_[a-z0-9_]+)\s*\(", code))) == 40
    assert "FJ_ALGO_AGG_ALL" in hdr                                   # (what makes this test one of the new feature's)
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_abi_version() == 8 and len(_lib.SYMBOLS) == 40


def test_flash_join_exposes_the_function():
    import flash_join
    from flash_hash_join_amd import api
    assert callable(flash_join.group_by_agg) and "group_by_agg" in api.EXTENSIONS and "group_by_agg" in api.__all__


def _device_call(algo, materialize=1, vals=0x20000, pk=None, n_p=0, ok=0x40000, ov=0x50000, cap=100, nb=100):
    from flash_hash_join_amd import _lib
    cnt = ctypes.c_uint64(0)
    rc = _lib.load().fj_join_device(None, algo, 0, materialize, 0x10000, vals, nb, pk, n_p, None, 64, ctypes.byref(cnt), ok, ov, cap, None)
    return rc, _lib.last_error()


DEVICE_REFUSALS = [   # id, keyword arguments of _device_call, needles
    ("without_group_by", dict(algo=ALL), ("unknown algo",)),
    ("without_group_by_radix_signed", dict(algo=ALL | SIGNED | 2), ("unknown algo",)),
    ("with_build_order", dict(algo=ALL | BO), ("unknown algo",)),
    ("with_probe_order", dict(algo=ALL | PO), ("unknown algo",)),
    ("min", dict(algo=GB | ALL | MIN), ("FJ_ALGO_AGG_ALL cannot be combined with FJ_ALGO_AGG_MIN",)),
    ("max", dict(algo=GB | ALL | MAX | 2), ("FJ_ALGO_AGG_ALL cannot be combined with FJ_ALGO_AGG_MAX",)),
    ("max_signed", dict(algo=GB | ALL | MAX | SIGNED), ("FJ_ALGO_AGG_ALL cannot be combined with FJ_ALGO_AGG_MAX",)),
    ("row_ids", dict(algo=GB | ALL | ROW_IDS), ("FJ_ALGO_AGG_ALL cannot be combined with FJ_ALGO_ROW_IDS",)),
    ("inverse", dict(algo=GB | ALL | INVERSE | 1), ("FJ_ALGO_AGG_ALL cannot be combined with FJ_ALGO_INVERSE",)),
    ("signed_and_float", dict(algo=GB | ALL | SIGNED | FLOAT), ("FJ_ALGO_AGG_FLOAT cannot be combined with FJ_ALGO_AGG_SIGNED",)),
    ("count_only", dict(algo=GB | ALL, materialize=0), ("FJ_ALGO_AGG_ALL", "materialize = 1")),
    ("no_values", dict(algo=GB | ALL, vals=None), ("FJ_ALGO_AGG_ALL", "d_build_vals")),
    ("no_values_float", dict(algo=GB | ALL | FLOAT, vals=None), ("FJ_ALGO_AGG_ALL", "d_build_vals")),
    ("no_keys_output", dict(algo=GB | ALL | SIGNED, ok=None), ("FJ_ALGO_AGG_ALL", "d_out_keys")),
    ("no_vals_output", dict(algo=GB | ALL | 2, ov=None), ("FJ_ALGO_AGG_ALL", "d_out_vals")),
    ("zero_capacity", dict(algo=GB | ALL, cap=0), ("FJ_ALGO_AGG_ALL", "capacity")),
    ("misaligned_keys", dict(algo=GB | ALL, ok=0x40004), ("8-byte aligned",)),
    ("misaligned_vals", dict(algo=GB | ALL | FLOAT, ov=0x50004), ("8-byte aligned",)),
    ("probe_keys", dict(algo=GB | ALL, pk=0x30000), ("FJ_ALGO_GROUP_BY", "no probe side")),
    ("probe_rows", dict(algo=GB | ALL | 2, n_p=7), ("FJ_ALGO_GROUP_BY", "no probe side")),
    ("many", dict(algo=GB | ALL | 0x10), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_MANY_TO_MANY",)),
    ("left", dict(algo=GB | ALL | 0x20), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_LEFT_OUTER",)),
    ("build_order", dict(algo=GB | ALL | BO), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_BUILD_ORDER",)),
    ("unknown_base", dict(algo=GB | ALL | 3), ("unknown algo",)),
    ("unknown_bit", dict(algo=GB | ALL | 0x80000), ("unknown algo",)),
    ("misaligned_input", dict(algo=GB | ALL, vals=0x20008), ("16-byte aligned",)),
]


@pytest.mark.parametrize("cid,kw,needles", DEVICE_REFUSALS, ids=[r[0] for r in DEVICE_REFUSALS])
def test_invalid_combinations_are_refused_before_any_device_work(cid, kw, needles):
    """A NULL context: the checks come before the context is touched (the pointers are never dereferenced)."""
    rc, err = _device_call(**kw)
    assert rc != 0 and "null context" not in err, err
    for needle in needles:
        assert needle in err, err


def test_signed_without_an_aggregate_it_modifies_keeps_its_message():
    rc, err = _device_call(algo=GB | SIGNED)
    assert rc != 0 and "FJ_ALGO_AGG_SIGNED modifies FJ_ALGO_AGG_MIN or FJ_ALGO_AGG_MAX" in err and "null context" not in err, err


VALID = [(f"{('adaptive', 'scalar', 'radix')[base]}-{fid}-cap{cap}", dict(algo=GB | ALL | base | flags, cap=cap))
         for base in (0, 1, 2) for fid, flags in (("unsigned", 0), ("signed", SIGNED), ("float", FLOAT)) for cap in (1, 5000)]


@pytest.mark.parametrize("cid,kw", VALID, ids=[v[0] for v in VALID])
def test_valid_combinations_reach_the_context(cid, kw):
    """nb = 100 with room for one group, and with more room than rows: any capacity >= 1 passes the checks"""
    rc, err = _device_call(**kw)
    assert rc != 0 and "null context" in err, err


def test_an_empty_relation_needs_no_buffers():
    rc, err = _device_call(algo=GB | ALL, nb=0, vals=None, ok=None, ov=None, cap=0)
    assert rc != 0 and "null context" in err, err


def test_the_bare_bit_is_an_unknown_algo():
    for algo in (ALL, ALL | 1, ALL | BO, ALL | BO | MIN, ALL | PO, ALL | PO | ROW_IDS, ALL | SIGNED, ALL | FLOAT):
        rc, err = _device_call(algo=algo)
        assert rc != 0 and "unknown algo" in err and "null context" not in err, (hex(algo), err)


HOST_REFUSALS = [   # id, algo, materialize, values, out_keys, out_vals, needles
    ("bare_bit", ALL, 1, True, True, True, ("unknown algo",)),
    ("with_build_order", ALL | BO, 1, True, True, True, ("unknown algo",)),
    ("with_probe_order", ALL | PO, 1, True, True, True, ("unknown algo",)),
    ("min", GB | ALL | MIN, 1, True, True, True, ("FJ_ALGO_AGG_ALL cannot be combined with FJ_ALGO_AGG_MIN",)),
    ("max", GB | ALL | MAX | 2, 1, True, True, True, ("FJ_ALGO_AGG_ALL cannot be combined with FJ_ALGO_AGG_MAX",)),
    ("row_ids", GB | ALL | ROW_IDS, 1, True, True, True, ("FJ_ALGO_AGG_ALL cannot be combined with FJ_ALGO_ROW_IDS",)),
    ("inverse", GB | ALL | INVERSE, 1, True, True, True, ("FJ_ALGO_AGG_ALL cannot be combined with FJ_ALGO_INVERSE",)),
    ("signed_and_float", GB | ALL | SIGNED | FLOAT, 1, True, True, True, ("FJ_ALGO_AGG_FLOAT cannot be combined with FJ_ALGO_AGG_SIGNED",)),
    ("count_only", GB | ALL, 0, True, True, True, ("FJ_ALGO_AGG_ALL", "materialize = 1")),
    ("no_values", GB | ALL | SIGNED, 1, False, True, True, ("FJ_ALGO_AGG_ALL", "build_vals")),
    ("no_keys_output", GB | ALL, 1, True, False, True, ("FJ_ALGO_AGG_ALL", "out_keys")),
    ("no_vals_output", GB | ALL | FLOAT, 1, True, True, False, ("FJ_ALGO_AGG_ALL", "out_vals")),
    ("many", GB | ALL | 0x10, 1, True, True, True, ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_MANY_TO_MANY",)),
    ("unknown_base", GB | ALL | 3, 1, True, True, True, ("unknown algo",)),
    ("unknown_bit", GB | ALL | 0x80000, 1, True, True, True, ("unknown algo",)),
    ("signed_alone", GB | SIGNED, 1, True, True, True, ("FJ_ALGO_AGG_SIGNED modifies",)),
]


@pytest.mark.parametrize("cid,algo,materialize,vals,want_ok,want_ov,needles", HOST_REFUSALS, ids=[r[0] for r in HOST_REFUSALS])
def test_host_entry_refusals(cid, algo, materialize, vals, want_ok, want_ov, needles):
    """fj_join_host makes the same checks before its context is created"""
    from flash_hash_join_amd import _lib
    L = _lib.load()
    k = np.arange(8, dtype=np.uint64)
    cnt, sec = ctypes.c_uint64(0), ctypes.c_double(0)
    ok, ov = ctypes.c_void_p(), ctypes.c_void_p()
    rc = L.fj_join_host(algo, 0, materialize, k.ctypes.data, k.ctypes.data if vals else None, 8, None, 0, ctypes.byref(cnt), ctypes.byref(sec),
                        ctypes.byref(ok) if want_ok else None, ctypes.byref(ov) if want_ov else None)
    err = _lib.last_error()
    assert rc != 0 and "null context" not in err and "HIP device" not in err, err
    for needle in needles:
        assert needle in err, err
    assert not ok.value and not ov.value


def test_python_argument_errors():
    from flash_hash_join_amd import api
    k = np.arange(4, dtype=np.uint64)
    f = k.astype(np.float64)
    with pytest.raises(ValueError, match="unknown aggregate 'median'"):
        api.group_by_agg(k, k, aggs=("sum", "median"))
    with pytest.raises(ValueError, match="unknown aggregate"):
        api.group_by_agg(k, k, aggs=("Sum",))
    with pytest.raises(ValueError, match="aggs"):
        api.group_by_agg(k, k, aggs="sum")                              # a string is no sequence of names
    with pytest.raises(ValueError, match="repeats"):
        api.group_by_agg(k, k, aggs=("min", "max", "min"))
    with pytest.raises(ValueError, match="aggs is empty"):
        api.group_by_agg(k, k, aggs=())
    with pytest.raises(ValueError, match="'mean' needs float64=True"):
        api.group_by_agg(k, k, aggs=("count", "mean"))
    with pytest.raises(ValueError, match="values has 3 elements, keys has 4"):
        api.group_by_agg(k, k[:3])
    with pytest.raises(ValueError, match="values has 5 elements, keys has 4"):
        api.group_by_agg(k, np.arange(5, dtype=np.float64), aggs=("mean",), float64=True)
    with pytest.raises(ValueError, match="values is required"):
        api.group_by_agg(k, None)
    with pytest.raises(TypeError, match="float64=True needs floating-point values"):
        api.group_by_agg(k, k, float64=True)
    with pytest.raises(TypeError, match="float64=True needs floating-point values"):
        api.group_by_agg(k, k.astype(np.int64), aggs=("mean",), float64=True)
    for signed in (True, False):
        with pytest.raises(TypeError, match="signed must be None with float64=True"):
            api.group_by_agg(k, f, signed=signed, float64=True)
    with pytest.raises(TypeError, match="signed must be None, True or False"):
        api.group_by_agg(k, k, signed="yes")
    with pytest.raises(TypeError, match="values must be integers"):
        api.group_by_agg(k, f)                                          # a float column without float64=True has no integer order
    with pytest.raises(TypeError, match="keys"):
        api.group_by_agg(np.array(["a", "b", "c", "d"]), k)
    for bad in (0, -1, 1.5, "3", True, np.float64(2.0)):
        with pytest.raises(ValueError, match="max_groups must be None or an integer >= 1"):
            api.group_by_agg(k, k, max_groups=bad)


def test_numpy_reference_on_a_hand_written_case():
    keys = np.array([7, 5, 7, 2**64 - 1, 0, 7, 2**64 - 1, 9], dtype=np.uint64)
    vals = np.array([1, 4, 2**63, 2**63, 32, 2**63 + 3, 2**64 - 1, 0], dtype=np.uint64)
    r = ref_group_by_agg(keys, vals)
    assert r["keys"].tolist() == [0, 5, 7, 9, 2**64 - 1] and r["count"].tolist() == [1, 1, 3, 1, 2]
    assert r["sum"].dtype == np.uint64 and r["sum"].tolist() == [32, 4, 4, 0, 2**63 - 1]          # 1 + 2^63 + 2^63 + 3 wraps to 4
    assert r["min_u"].tolist() == [32, 4, 1, 0, 2**63] and r["max_u"].tolist() == [32, 4, 2**63 + 3, 0, 2**64 - 1]
    assert r["min_s"].tolist() == [32, 4, -2**63, 0, -2**63] and r["max_s"].tolist() == [32, 4, 1, 0, -1]
    r = ref_group_by_agg(np.empty(0, np.uint64), np.empty(0, np.uint64))
    assert all(a.size == 0 for a in r.values())
    f = ref_group_by_agg_float(np.array([3, 1, 3, 3, 1], dtype=np.uint64), np.array([1e100, -2.5, 1.0, -1e100, 0.5]))
    assert f["keys"].tolist() == [1, 3] and f["count"].tolist() == [2, 3]
    assert f["sum"].tolist() == [-2.0, 1.0] and f["abs"].tolist() == [3.0, 2e100]                 # fsum: 1e100 + 1 - 1e100 == 1
    assert f["min"].tolist() == [-2.5, -1e100] and f["max"].tolist() == [0.5, 1e100]
