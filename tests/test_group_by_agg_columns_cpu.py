"""Four aggregates per two-column key in one call (FJ_ALGO_GROUP_BY | FJ_ALGO_KEY_PAIR | FJ_ALGO_AGG_ALL, csrc/fj_groupby_pair_agg.hip;
api.group_by_agg_columns): what needs no GPU - every refusal of the form in both entry points (a NULL context: the checks come before
any device work, the fake pointers are never dereferenced), the valid combinations, the unchanged ABI, the Python argument checks and
the NumPy reference the GPU half, tests/test_group_by_agg_columns.py, compares with."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

MANY, LEFT, ANTI, ROW_IDS, FULL, ALLC, PO, BO = 0x10, 0x20, 0x40, 0x80, 0x100, 0x200, 0x800, 0x1000
MIN, MAX, SIGNED, GB, INV, AFLOAT, AALL, AARG, AMERGE = 0x4000, 0x8000, 0x10000, 0x40000, 0x100000, 0x2000000, 0x4000000, 0x8000000, 0x10000000
PAIR, GROWS = 0x20000000, 0x40000000
GPA = GB | PAIR | AALL
FORM = "FJ_ALGO_KEY_PAIR | FJ_ALGO_AGG_ALL"
KINDS = ("unsigned", "signed", "float")


def ref_pair_agg(a, b, v, kind):
    """(A, B, count, sum, min, max) of GROUP BY a, b over the uint64 words a, b and the words v of `kind`, the groups in lexicographic
    order of (a, b): np.lexsort and ufunc.reduceat, nothing of the library.  unsigned / signed: the sum wraps in uint64 and comes back
    as uint64 words, min and max as uint64 / int64; float: v holds float64 numbers and all three are float64 (the GPU tests use
    multiples of 2^-10, whose sums are exact in any order)."""
    a, b = np.asarray(a, dtype=np.uint64).reshape(-1), np.asarray(b, dtype=np.uint64).reshape(-1)
    if kind == "float":
        v = np.asarray(v, dtype=np.float64).reshape(-1)
    else:
        v = np.asarray(v).reshape(-1)
        v = v.view(np.uint64) if v.dtype == np.int64 else v.astype(np.uint64)
    if a.size == 0:
        e = np.empty(0, np.uint64)
        return e, e, np.empty(0, np.int64), (np.empty(0, np.float64) if kind == "float" else e), v[:0], v[:0]
    order = np.lexsort((b, a))
    sa, sb, sv = a[order], b[order], v[order]
    starts = np.flatnonzero(np.r_[True, (sa[1:] != sa[:-1]) | (sb[1:] != sb[:-1])])
    count = np.diff(np.r_[starts, a.size]).astype(np.int64)
    total = np.add.reduceat(sv, starts)                                       # (uint64: wraps modulo 2^64)
    cmpv = sv.view(np.int64) if kind == "signed" else sv
    return sa[starts], sb[starts], count, total, np.minimum.reduceat(cmpv, starts), np.maximum.reduceat(cmpv, starts)


def test_numpy_reference_on_a_hand_written_case():
    a = np.array([7, 5, 7, 7, 5, 7], dtype=np.uint64)
    b = np.array([1, 1, 2, 1, 1, 2], dtype=np.uint64)
    v = np.array([1, 4, 2**63, 2**64 - 1, 32, 2**63 + 3], dtype=np.uint64)
    ga, gb, cnt, tot, lo, hi = ref_pair_agg(a, b, v, "unsigned")
    assert ga.tolist() == [5, 7, 7] and gb.tolist() == [1, 1, 2] and cnt.tolist() == [2, 2, 2]
    assert tot.dtype == np.uint64 and tot.tolist() == [36, 0, 3]                 # 1 + (2^64 - 1) and 2^63 + 2^63 + 3 wrap
    assert lo.tolist() == [4, 1, 2**63] and hi.tolist() == [32, 2**64 - 1, 2**63 + 3]
    ga, gb, cnt, tot, lo, hi = ref_pair_agg(a, b, v, "signed")
    assert tot.tolist() == [36, 0, 3] and lo.tolist() == [4, -1, -2**63] and hi.tolist() == [32, 1, -2**63 + 3]
    ga, gb, cnt, tot, lo, hi = ref_pair_agg(a, b, np.array([0.5, -2.0, 1.25, 3.0, 2.0, -1.25]), "float")
    assert tot.tolist() == [0.0, 3.5, 0.0] and lo.tolist() == [-2.0, 0.5, -1.25] and hi.tolist() == [2.0, 3.0, 1.25]
    assert all(x.size == 0 for x in ref_pair_agg([], [], [], "unsigned")) and all(x.size == 0 for x in ref_pair_agg([], [], [], "float"))


def test_abi_version_and_function_count_are_unchanged():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    assert int(re.search(r"#define FJ_ABI_VERSION (\d+)", hdr).group(1)) == 8
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert len(set(re.findall(r"\b(fj_[a-z0-9_]+)\s*\(", code))) == 40
    assert FORM in hdr                                                           # (what makes this test one of the new feature's)
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_abi_version() == 8 and len(_lib.SYMBOLS) == 40


def test_no_new_flag_mirror_and_the_function_is_exposed():
    import flash_join
    from flash_hash_join_amd import api
    mirrors = {n: v for n, v in vars(api).items() if n.startswith("ALGO_") and isinstance(v, int)}
    assert [n for n, v in mirrors.items() if v & PAIR] == ["ALGO_KEY_PAIR"] and [n for n, v in mirrors.items() if v & AALL] == ["ALGO_AGG_ALL"]
    assert flash_join.group_by_agg_columns is api.group_by_agg_columns and "group_by_agg_columns" in api.__all__


def _device_call(algo, materialize=1, a=0x10000, b=0x20000, v=0x30000, n_p=100, ok=0x40000, ov=0x50000, cap=100, nb=100):
    from flash_hash_join_amd import _lib
    cnt = ctypes.c_uint64(0)
    rc = _lib.load().fj_join_device(None, algo, 0, materialize, a, b, nb, v, n_p, None, 64, ctypes.byref(cnt), ok, ov, cap, None)
    return rc, _lib.last_error()


DEVICE_REFUSALS = [   # id, keyword arguments of _device_call, needles
    # with FJ_ALGO_INVERSE it is not this form: the messages of before, with and without a third column
    ("inverse", dict(algo=GPA | INV, v=None, n_p=0), ("FJ_ALGO_AGG_ALL cannot be combined with FJ_ALGO_INVERSE",)),
    ("inverse_radix", dict(algo=GPA | INV | 2, v=None, n_p=0), ("FJ_ALGO_AGG_ALL cannot be combined with FJ_ALGO_INVERSE",)),
    ("inverse_with_a_third_column", dict(algo=GPA | INV), ("FJ_ALGO_GROUP_BY", "no probe side")),
    ("min", dict(algo=GPA | MIN), (FORM, "FJ_ALGO_AGG_MIN")),
    ("max", dict(algo=GPA | MAX | 2), (FORM, "FJ_ALGO_AGG_MAX")),
    ("max_signed", dict(algo=GPA | MAX | SIGNED), (FORM, "FJ_ALGO_AGG_MAX")),
    ("row_ids", dict(algo=GPA | ROW_IDS | 1), (FORM, "FJ_ALGO_ROW_IDS")),
    ("agg_arg", dict(algo=GPA | AARG), (FORM, "FJ_ALGO_AGG_ARG")),
    ("agg_merge", dict(algo=GPA | AMERGE), (FORM, "FJ_ALGO_AGG_MERGE")),
    ("group_rows", dict(algo=GPA | GROWS), ("FJ_ALGO_GROUP_ROWS", "FJ_ALGO_AGG_ALL")),
    ("signed_and_float", dict(algo=GPA | SIGNED | AFLOAT), ("FJ_ALGO_AGG_FLOAT", "FJ_ALGO_AGG_SIGNED")),
    ("count_only", dict(algo=GPA, materialize=0), (FORM, "materialize = 1")),
    ("no_a", dict(algo=GPA, a=None), (FORM, "d_build_keys")),
    ("no_b", dict(algo=GPA | 1, b=None), (FORM, "d_build_vals")),
    ("no_v", dict(algo=GPA | 2, v=None), (FORM, "d_probe_keys")),
    ("no_keys_output", dict(algo=GPA | SIGNED, ok=None), (FORM, "d_out_keys")),
    ("no_vals_output", dict(algo=GPA | AFLOAT, ov=None), (FORM, "d_out_vals")),
    ("np_zero", dict(algo=GPA, n_p=0), (FORM, "np == nb")),
    ("np_smaller", dict(algo=GPA | 2, n_p=99), (FORM, "np == nb", "99")),
    ("np_larger", dict(algo=GPA | 1, n_p=101), (FORM, "np == nb", "101")),
    ("np_without_rows", dict(algo=GPA, nb=0, n_p=5, cap=0), (FORM, "np == nb")),
    ("zero_capacity", dict(algo=GPA, cap=0), (FORM, "capacity")),
    ("too_many_rows", dict(algo=GPA, nb=2**40 + 1, n_p=2**40 + 1), ("FJ_ALGO_KEY_PAIR", "2^40")),
    ("misaligned_a", dict(algo=GPA, a=0x10008), ("16-byte aligned",)),
    ("misaligned_b", dict(algo=GPA | SIGNED, b=0x20008), ("16-byte aligned",)),
    ("misaligned_v", dict(algo=GPA | 2, v=0x30008), ("16-byte aligned",)),
    ("misaligned_keys_output", dict(algo=GPA, ok=0x40004), ("8-byte aligned",)),
    ("misaligned_vals_output", dict(algo=GPA | AFLOAT, ov=0x50004), ("8-byte aligned",)),
    ("many", dict(algo=GPA | MANY), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_MANY_TO_MANY",)),
    ("left", dict(algo=GPA | LEFT), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_LEFT_OUTER",)),
    ("probe_order", dict(algo=GPA | PO), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_PROBE_ORDER",)),
    ("build_order", dict(algo=GPA | BO), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_BUILD_ORDER",)),
    ("base_3", dict(algo=GPA | 3), ("unknown algo",)),
    ("unassigned_bit", dict(algo=GPA | 0x80000), ("unknown algo",)),
    ("without_group_by", dict(algo=PAIR | AALL), ("unknown algo",)),
    # the neighbours keep their wording: the pair alone names both of its partners, every other group-by form takes no probe side
    ("pair_alone", dict(algo=GB | PAIR, v=None, n_p=0), ("FJ_ALGO_KEY_PAIR", "FJ_ALGO_INVERSE", "FJ_ALGO_AGG_ALL")),
    ("agg_all_with_a_third_column", dict(algo=GB | AALL), ("FJ_ALGO_GROUP_BY", "no probe side")),
    ("inverse_pair_with_a_third_column", dict(algo=GB | INV | PAIR), ("FJ_ALGO_GROUP_BY", "no probe side")),
]


@pytest.mark.parametrize("cid,kw,needles", DEVICE_REFUSALS, ids=[r[0] for r in DEVICE_REFUSALS])
def test_invalid_combinations_are_refused_before_any_device_work(cid, kw, needles):
    """A NULL context: the checks come before the context is touched (no GPU needed; the pointers are never dereferenced)."""
    rc, err = _device_call(**kw)
    assert rc != 0 and "null context" not in err, err
    for needle in needles:
        assert needle in err, err


VALID = [(f"{('adaptive', 'scalar', 'radix')[base]}-{kid}-{fid}", dict(algo=GPA | base | flags, **kw))
         for base in (0, 1, 2) for kid, flags in (("unsigned", 0), ("signed", SIGNED), ("float", AFLOAT))
         for fid, kw in (("cap1", dict(cap=1)), ("more_capacity_than_rows", dict(cap=5000)), ("rows_2_to_40", dict(nb=2**40, n_p=2**40, cap=7)),
                         ("no_rows", dict(nb=0, n_p=0, cap=0, a=None, b=None, v=None, ok=None, ov=None)))]


@pytest.mark.parametrize("cid,kw", VALID, ids=[v[0] for v in VALID])
def test_valid_combinations_reach_the_context(cid, kw):
    rc, err = _device_call(**kw)
    assert rc != 0 and "null context" in err, err


def _host_call(algo, materialize=1, a=True, b=True, v=True, n_p=8, nb=8, want_ok=True, want_ov=True):
    """(the refusals come before a byte of the columns is read: nb beyond the eight words is never dereferenced)"""
    from flash_hash_join_amd import _lib
    L = _lib.load()
    k = np.arange(8, dtype=np.uint64)
    cnt, sec = ctypes.c_uint64(0), ctypes.c_double(0)
    ok, ov = ctypes.c_void_p(), ctypes.c_void_p()
    p = k.ctypes.data
    rc = L.fj_join_host(algo, 0, materialize, p if a else None, p if b else None, nb, p if v else None, n_p, ctypes.byref(cnt), ctypes.byref(sec),
                        ctypes.byref(ok) if want_ok else None, ctypes.byref(ov) if want_ov else None)
    return rc, _lib.last_error(), ok, ov


HOST_REFUSALS = [   # id, keyword arguments of _host_call, needles
    ("inverse", dict(algo=GPA | INV, v=False, n_p=0), ("FJ_ALGO_AGG_ALL cannot be combined with FJ_ALGO_INVERSE",)),
    ("inverse_with_a_third_column", dict(algo=GPA | INV), ("no probe side",)),
    ("min", dict(algo=GPA | MIN), (FORM, "FJ_ALGO_AGG_MIN")),
    ("max", dict(algo=GPA | MAX | 2), (FORM, "FJ_ALGO_AGG_MAX")),
    ("row_ids", dict(algo=GPA | ROW_IDS), (FORM, "FJ_ALGO_ROW_IDS")),
    ("agg_arg", dict(algo=GPA | AARG | 1), (FORM, "FJ_ALGO_AGG_ARG")),
    ("agg_merge", dict(algo=GPA | AMERGE), (FORM, "FJ_ALGO_AGG_MERGE")),
    ("group_rows", dict(algo=GPA | GROWS), ("FJ_ALGO_GROUP_ROWS", "FJ_ALGO_AGG_ALL")),
    ("signed_and_float", dict(algo=GPA | SIGNED | AFLOAT), ("FJ_ALGO_AGG_FLOAT", "FJ_ALGO_AGG_SIGNED")),
    ("count_only", dict(algo=GPA, materialize=0), (FORM, "materialize = 1")),
    ("no_a", dict(algo=GPA, a=False), (FORM, "build_keys")),
    ("no_b", dict(algo=GPA | 2, b=False), (FORM, "build_vals")),
    ("no_v", dict(algo=GPA | 1, v=False), (FORM, "probe_keys")),
    ("no_keys_output", dict(algo=GPA, want_ok=False), (FORM, "out_keys")),
    ("no_vals_output", dict(algo=GPA | AFLOAT, want_ov=False), (FORM, "out_vals")),
    ("np_zero", dict(algo=GPA, n_p=0), (FORM, "np == nb")),
    ("np_smaller", dict(algo=GPA | SIGNED, n_p=7), (FORM, "np == nb")),
    ("too_many_rows", dict(algo=GPA | 1, nb=2**40 + 1, n_p=2**40 + 1), ("FJ_ALGO_KEY_PAIR", "2^40")),
    ("many", dict(algo=GPA | MANY), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_MANY_TO_MANY",)),
    ("build_order", dict(algo=GPA | BO), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_BUILD_ORDER",)),
    ("base_9", dict(algo=GPA | 9), ("unknown algo",)),
    ("unassigned_bit", dict(algo=GPA | 0x80000), ("unknown algo",)),
    ("pair_alone", dict(algo=GB | PAIR, v=False, n_p=0), ("FJ_ALGO_KEY_PAIR", "FJ_ALGO_INVERSE", "FJ_ALGO_AGG_ALL")),
    ("agg_all_with_a_third_column", dict(algo=GB | AALL), ("no probe side",)),
]


@pytest.mark.parametrize("cid,kw,needles", HOST_REFUSALS, ids=[r[0] for r in HOST_REFUSALS])
def test_host_entry_refusals(cid, kw, needles):
    """fj_join_host makes the same checks before its context is created (no GPU needed)."""
    rc, err, ok, ov = _host_call(**kw)
    assert rc != 0 and "null context" not in err and "HIP device" not in err, err
    for needle in needles:
        assert needle in err, err
    assert not ok.value and not ov.value


@pytest.mark.parametrize("base", [0, 1, 2])
@pytest.mark.parametrize("kind", [0, SIGNED, AFLOAT], ids=KINDS)
def test_host_entry_accepts_every_valid_combination(base, kind):
    """past the argument checks: the call runs where there is a device, and fails on the missing device - never on a flag - elsewhere"""
    from flash_hash_join_amd import _lib
    rc, err, ok, ov = _host_call(GPA | base | kind)
    try:
        assert rc == 0 or ("FJ_ALGO" not in err and "unknown algo" not in err and "np == nb" not in err), err
    finally:
        _lib.load().fj_free_host(ok)
        _lib.load().fj_free_host(ov)


def test_python_argument_errors():
    """every one is raised before any device work: this test runs without a GPU"""
    import torch
    from flash_hash_join_amd import api
    k = np.arange(4, dtype=np.uint64)
    f = k.astype(np.float64)
    G = api.group_by_agg_columns
    with pytest.raises(ValueError, match="rows"):
        G([k, k[:3]], k)                                                         # ragged columns
    with pytest.raises(ValueError, match="rows"):
        G([k, k, np.arange(5)], k)
    with pytest.raises(ValueError, match="columns is empty"):
        G([], k)
    with pytest.raises(ValueError, match="columns is empty"):
        G((), None, aggs=("count",))
    with pytest.raises(TypeError, match="one kind"):
        G([k, torch.arange(4)], k)
    with pytest.raises(TypeError, match=r"columns\[1\]"):
        G([k, np.array(["a", "b", "c", "d"])], k)
    with pytest.raises(ValueError, match="values is required unless"):
        G([k, k], None)                                                          # the default aggs
    with pytest.raises(ValueError, match="values is required unless"):
        G([k, k], None, aggs=("count", "sum"))
    with pytest.raises(ValueError, match="values is required unless"):
        G([k], None, aggs=("min",))
    with pytest.raises(ValueError, match="'mean' needs float64=True"):
        G([k, k], k, aggs=("count", "mean"))
    with pytest.raises(ValueError, match="'mean' needs float64=True"):
        G([k, k, k], f, aggs=("mean",))
    with pytest.raises(TypeError, match="float64=True needs floating-point values"):
        G([k, k], k, float64=True)                                               # an integer column read as doubles
    with pytest.raises(TypeError, match="float64=True needs floating-point values"):
        G([k, k, k], k.astype(np.int64), aggs=("mean",), float64=True)
    with pytest.raises(TypeError, match="float64=True needs floating-point values"):
        G([k], k, float64=True)
    for signed in (True, False):
        with pytest.raises(TypeError, match="signed must be None with float64=True"):
            G([k, k], f, signed=signed, float64=True)
    with pytest.raises(TypeError, match="signed must be None, True or False"):
        G([k, k], k, signed="yes")
    with pytest.raises(TypeError, match="values must be integers"):
        G([k, k], f)                                                             # a float column without float64=True has no integer order
    with pytest.raises(ValueError, match="values has 3 elements"):
        G([k, k], k[:3])
    with pytest.raises(ValueError, match="values has 5 elements"):
        G([k, k, k], np.arange(5, dtype=np.float64), float64=True)
    with pytest.raises(ValueError, match="unknown aggregate 'median'"):
        G([k, k], k, aggs=("sum", "median"))
    with pytest.raises(ValueError, match="repeats"):
        G([k, k], k, aggs=("min", "min"))
    with pytest.raises(ValueError, match="aggs is empty"):
        G([k, k], k, aggs=())
    for bad in (0, -1, 1.5, "3", True, np.float64(2.0)):
        with pytest.raises(ValueError, match="max_groups must be None or an integer >= 1"):
            G([k, k], k, max_groups=bad)
        with pytest.raises(ValueError, match="max_groups must be None or an integer >= 1"):
            G([k, k, k], None, aggs=("count",), max_groups=bad)
