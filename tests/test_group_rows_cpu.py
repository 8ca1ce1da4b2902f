"""The rows of every group (FJ_ALGO_GROUP_BY | FJ_ALGO_GROUP_ROWS, csrc/fj_groupby_rows.hip; api.group_rows / api.group_by_collect):
what needs no GPU - the flag's value and its refusals in both entry points (a NULL context: the checks come before any device work)
and the Python argument checks.  The GPU half is tests/test_group_rows.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

MANY, LEFT, ANTI, ROW_IDS, FULL, ALL, PO, BO = 0x10, 0x20, 0x40, 0x80, 0x100, 0x200, 0x800, 0x1000
MIN, MAX, SIGNED, GB, INV, AFLOAT, AALL, AARG, AMERGE = 0x4000, 0x8000, 0x10000, 0x40000, 0x100000, 0x2000000, 0x4000000, 0x8000000, 0x10000000
PAIR = 0x20000000
ROWS = 0x40000000
GR = GB | ROWS
PINNED_UNASSIGNED = (0x400, 0x2000, 0x20000, 0x80000, 0x200000)


def test_header_flag_and_python_mirror():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    flags = {name: int(v, 16) for name, v in re.findall(r"#define (FJ_ALGO_[A-Z_]+)\s+(0x[0-9a-fA-F]+)", hdr)}
    assert flags["FJ_ALGO_GROUP_ROWS"] == 0x40000000
    assert [n for n, v in flags.items() if v & 0x40000000] == ["FJ_ALGO_GROUP_ROWS"], "another flag shares the bit"
    assert not any(v & bit for v in flags.values() for bit in PINNED_UNASSIGNED), "a pinned bit was assigned"
    from flash_hash_join_amd import api
    assert api.ALGO_GROUP_ROWS == 0x40000000
    mirrors = {n: v for n, v in vars(api).items() if n.startswith("ALGO_") and isinstance(v, int)}
    assert [n for n, v in mirrors.items() if v & 0x40000000] == ["ALGO_GROUP_ROWS"]


def test_abi_version_and_function_count_are_unchanged():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    assert "FJ_ALGO_GROUP_ROWS" in hdr                                  # (what makes this test one of the new feature's)
    assert int(re.search(r"#define FJ_ABI_VERSION (\d+)", hdr).group(1)) == 8
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert len(set(re.findall(r"\b(fj_[a-z0-9_]+)\s*\(", code))) == 40
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_abi_version() == 8 and len(_lib.SYMBOLS) == 40
    exported = re.findall(r"\b(fj_[a-z0-9_]+);", open(os.path.join(ROOT, "flash_hash_join_amd", "csrc", "exports.map")).read())
    assert len(set(exported)) == 40 and set(exported) == set(_lib.SYMBOLS)


def _device_call(algo, materialize=1, vals=0x20000, pk=None, n_p=0, ok=0x40000, ov=0x50000, cap=100, nb=100):
    from flash_hash_join_amd import _lib
    cnt = ctypes.c_uint64(0)
    rc = _lib.load().fj_join_device(None, algo, 0, materialize, 0x10000, vals, nb, pk, n_p, None, 64, ctypes.byref(cnt), ok, ov, cap, None)
    return rc, _lib.last_error()


def _plain_form_is_accepted():
    """the refusals below are the flag's own: the same call without the offending part gets past every check"""
    rc, err = _device_call(algo=GR)
    assert rc != 0 and "null context" in err, err


_COMBOS = [("inverse", INV, "INVERSE"), ("row_ids", ROW_IDS, "ROW_IDS"), ("min", MIN, "AGG_MIN"), ("max", MAX, "AGG_MAX"),
           ("signed", SIGNED, "AGG_SIGNED"), ("float", AFLOAT, "AGG_FLOAT"), ("agg_all", AALL, "AGG_ALL"), ("agg_arg", AARG, "AGG_ARG"),
           ("agg_merge", AMERGE, "AGG_MERGE"), ("key_pair", PAIR, "KEY_PAIR")]

DEVICE_REFUSALS = [   # id, keyword arguments of _device_call, needles
    # the flag without FJ_ALGO_GROUP_BY: an unknown algo that carries the whole word
    ("bare", dict(algo=ROWS), (f"unknown algo {ROWS}",)),
    ("bare_with_base", dict(algo=ROWS | 2), (f"unknown algo {ROWS | 2}",)),
    ("with_inverse_but_no_group_by", dict(algo=ROWS | INV), (f"unknown algo {ROWS | INV}",)),
    ("with_probe_order", dict(algo=ROWS | PO), (f"unknown algo {ROWS | PO}",)),
    ("with_build_order", dict(algo=ROWS | BO | 1), (f"unknown algo {ROWS | BO | 1}",)),
    # its own
    ("count_only", dict(algo=GR, materialize=0), ("FJ_ALGO_GROUP_ROWS", "materialize = 1")),
    ("count_only_radix", dict(algo=GR | 2, materialize=0), ("FJ_ALGO_GROUP_ROWS", "materialize = 1")),
    ("no_keys_output", dict(algo=GR, ok=None), ("FJ_ALGO_GROUP_ROWS", "d_out_keys")),
    ("no_rows_output", dict(algo=GR | 1, ov=None), ("FJ_ALGO_GROUP_ROWS", "d_out_vals")),
    ("capacity", dict(algo=GR, cap=99), ("output capacity 99 < 100",)),
    ("capacity_zero", dict(algo=GR | 2, cap=0), ("output capacity 0 < 100",)),
    ("misaligned_keys", dict(algo=GR, ok=0x40004), ("8-byte aligned",)),
    ("misaligned_rows", dict(algo=GR | 2, ov=0x50004), ("8-byte aligned",)),
    ("too_many_rows", dict(algo=GR, nb=2**40 + 1, cap=2**40 + 1), ("FJ_ALGO_GROUP_ROWS", "2^40")),
    # everything FJ_ALGO_GROUP_BY refuses
    ("many", dict(algo=GR | MANY), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_MANY_TO_MANY",)),
    ("left", dict(algo=GR | LEFT), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_LEFT_OUTER",)),
    ("anti", dict(algo=GR | ANTI), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_ANTI",)),
    ("full", dict(algo=GR | FULL), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_FULL_OUTER",)),
    ("all_copies", dict(algo=GR | ALL), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_ALL_COPIES",)),
    ("probe_order", dict(algo=GR | PO), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_PROBE_ORDER",)),
    ("build_order", dict(algo=GR | BO), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_BUILD_ORDER",)),
    ("probe_keys", dict(algo=GR, pk=0x30000), ("FJ_ALGO_GROUP_BY", "no probe side")),
    ("probe_rows", dict(algo=GR, n_p=7), ("FJ_ALGO_GROUP_BY", "no probe side")),
    ("base_3", dict(algo=GR | 3), ("unknown algo",)),
]
for _cid, _flag, _name in _COMBOS:   # no other modifier beside it, with any base and whatever else the word holds
    DEVICE_REFUSALS.append((_cid, dict(algo=GR | _flag), (f"FJ_ALGO_GROUP_ROWS cannot be combined with FJ_ALGO_{_name}",)))
    DEVICE_REFUSALS.append((_cid + "_radix_no_values", dict(algo=GR | _flag | 2, vals=None), (f"FJ_ALGO_GROUP_ROWS cannot be combined with FJ_ALGO_{_name}",)))
DEVICE_REFUSALS += [
    ("agg_all_merge", dict(algo=GR | AALL | AMERGE), ("FJ_ALGO_GROUP_ROWS cannot be combined with FJ_ALGO_AGG_ALL",)),
    ("inverse_key_pair", dict(algo=GR | INV | PAIR), ("FJ_ALGO_GROUP_ROWS cannot be combined with FJ_ALGO_INVERSE",)),
    ("arg_min", dict(algo=GR | AARG | MIN), ("FJ_ALGO_GROUP_ROWS cannot be combined with FJ_ALGO_",)),
    ("inverse_count_only", dict(algo=GR | INV, materialize=0), ("FJ_ALGO_GROUP_ROWS cannot be combined with FJ_ALGO_INVERSE",)),
]
for _bit in PINNED_UNASSIGNED:   # the five pinned bits stay unassigned: alone, and beside the new flag
    DEVICE_REFUSALS.append((f"pinned_bit_{_bit:#x}_alone", dict(algo=_bit), (f"unknown algo {_bit}",)))
    DEVICE_REFUSALS.append((f"pinned_bit_{_bit:#x}_with_group_rows", dict(algo=GR | _bit), ("unknown algo",)))
    DEVICE_REFUSALS.append((f"pinned_bit_{_bit:#x}_with_group_rows_radix", dict(algo=GR | _bit | 2, vals=None), ("unknown algo",)))


@pytest.mark.parametrize("cid,kw,needles", DEVICE_REFUSALS, ids=[r[0] for r in DEVICE_REFUSALS])
def test_invalid_combinations_are_refused_before_any_device_work(cid, kw, needles):
    """A NULL context: the checks come before the context is touched (no GPU needed; the pointers are never dereferenced)."""
    _plain_form_is_accepted()
    rc, err = _device_call(**kw)
    assert rc != 0 and "null context" not in err, err
    for needle in needles:
        assert needle in err, err


VALID = [(f"{('adaptive', 'scalar', 'radix')[base]}-{fid}", dict(algo=GR | base, **kw)) for base in (0, 1, 2)
         for fid, kw in (("values_given", dict()), ("values_null", dict(vals=None)), ("values_misaligned", dict(vals=0x20008)),
                         ("more_capacity_than_rows", dict(cap=5000)), ("rows_2_to_40", dict(nb=2**40, cap=2**40, vals=None)),
                         ("no_rows", dict(nb=0, cap=0, ok=None, ov=None, vals=None)), ("no_rows_with_buffers", dict(nb=0, cap=16)))]


@pytest.mark.parametrize("cid,kw", VALID, ids=[v[0] for v in VALID])
def test_valid_combinations_reach_the_context(cid, kw):
    rc, err = _device_call(**kw)
    assert rc != 0 and "null context" in err, err


HOST_REFUSALS = [   # id, algo, materialize, values, probe keys, np, nb, needles
    ("bare", ROWS, 1, False, False, 0, 8, (f"unknown algo {ROWS}",)),
    ("bare_with_base", ROWS | 2, 1, True, False, 0, 8, (f"unknown algo {ROWS | 2}",)),
    ("with_inverse_but_no_group_by", ROWS | INV, 1, False, False, 0, 8, (f"unknown algo {ROWS | INV}",)),
    ("with_probe_order", ROWS | PO, 1, True, False, 0, 8, (f"unknown algo {ROWS | PO}",)),
    ("count_only", GR, 0, False, False, 0, 8, ("FJ_ALGO_GROUP_ROWS", "materialize = 1")),
    ("too_many_rows", GR | 1, 1, False, False, 0, 2**40 + 1, ("FJ_ALGO_GROUP_ROWS", "2^40")),
    ("agg_all_merge", GR | AALL | AMERGE, 1, True, False, 0, 8, ("FJ_ALGO_GROUP_ROWS cannot be combined with FJ_ALGO_AGG_ALL",)),
    ("many", GR | MANY, 1, False, False, 0, 8, ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_MANY_TO_MANY",)),
    ("left", GR | LEFT, 1, False, False, 0, 8, ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_LEFT_OUTER",)),
    ("anti", GR | ANTI, 1, False, False, 0, 8, ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_ANTI",)),
    ("full", GR | FULL, 1, False, False, 0, 8, ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_FULL_OUTER",)),
    ("all_copies", GR | ALL, 1, False, False, 0, 8, ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_ALL_COPIES",)),
    ("probe_order", GR | PO, 1, False, False, 0, 8, ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_PROBE_ORDER",)),
    ("build_order", GR | BO, 1, False, False, 0, 8, ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_BUILD_ORDER",)),
    ("probe_keys", GR, 1, False, True, 0, 8, ("no probe side",)),
    ("probe_rows", GR | 2, 1, False, True, 8, 8, ("no probe side",)),
    ("base_9", GR | 9, 1, False, False, 0, 8, ("unknown algo",)),
]
for _cid, _flag, _name in _COMBOS:
    HOST_REFUSALS.append((_cid, GR | _flag, 1, True, False, 0, 8, (f"FJ_ALGO_GROUP_ROWS cannot be combined with FJ_ALGO_{_name}",)))
    HOST_REFUSALS.append((_cid + "_scalar_no_values", GR | _flag | 1, 1, False, False, 0, 8, (f"FJ_ALGO_GROUP_ROWS cannot be combined with FJ_ALGO_{_name}",)))
for _bit in PINNED_UNASSIGNED:
    HOST_REFUSALS.append((f"pinned_bit_{_bit:#x}_alone", _bit, 1, False, False, 0, 8, (f"unknown algo {_bit}",)))
    HOST_REFUSALS.append((f"pinned_bit_{_bit:#x}_with_group_rows", GR | _bit, 1, False, False, 0, 8, ("unknown algo",)))


def _host_call(algo, materialize, vals, pk, n_p, nb=8, want_keys=True, want_rows=True):
    """(the refusals come before a byte of the column is read: nb beyond the eight words is never dereferenced)"""
    from flash_hash_join_amd import _lib
    L = _lib.load()
    k = np.arange(8, dtype=np.uint64)
    cnt, sec = ctypes.c_uint64(0), ctypes.c_double(0)
    ok, ov = ctypes.c_void_p(), ctypes.c_void_p()
    rc = L.fj_join_host(algo, 0, materialize, k.ctypes.data, k.ctypes.data if vals else None, nb, k.ctypes.data if pk else None, n_p,
                        ctypes.byref(cnt), ctypes.byref(sec), ctypes.byref(ok) if want_keys else None, ctypes.byref(ov) if want_rows else None)
    return rc, _lib.last_error(), ok, ov


@pytest.mark.parametrize("cid,algo,materialize,vals,pk,n_p,nb,needles", HOST_REFUSALS, ids=[r[0] for r in HOST_REFUSALS])
def test_host_entry_refusals(cid, algo, materialize, vals, pk, n_p, nb, needles):
    """fj_join_host makes the same checks before its context is created (no GPU needed)."""
    _plain_form_is_accepted()
    rc, err, ok, ov = _host_call(algo, materialize, vals, pk, n_p, nb)
    assert rc != 0 and "null context" not in err and "HIP device" not in err, err
    for needle in needles:
        assert needle in err, err
    assert not ok.value and not ov.value


@pytest.mark.parametrize("base", [0, 1, 2])
@pytest.mark.parametrize("vals", [False, True], ids=["values_null", "values_given"])
@pytest.mark.parametrize("want_keys,want_rows", [(True, True), (True, False), (False, True)], ids=["both", "keys_alone", "rows_alone"])
def test_host_entry_accepts_every_valid_combination(base, vals, want_keys, want_rows):
    """past the argument checks: the call runs where there is a device, and fails on the missing device - never on a flag - elsewhere"""
    from flash_hash_join_amd import _lib
    _plain_form_is_accepted()
    rc, err, ok, ov = _host_call(GR | base, 1, vals, False, 0, 8, want_keys, want_rows)
    try:
        assert rc == 0 or ("FJ_ALGO" not in err and "unknown algo" not in err), err
    finally:
        _lib.load().fj_free_host(ok)
        _lib.load().fj_free_host(ov)


def test_python_argument_errors():
    import torch
    from flash_hash_join_amd import api
    k = np.arange(4, dtype=np.uint64)
    with pytest.raises(TypeError, match="keys"):
        api.group_rows(np.array(["a", "b"]))                            # a string column
    with pytest.raises(TypeError):
        api.group_rows()
    with pytest.raises(TypeError):
        api.group_rows(k, k)                                            # no value column: group_by_collect takes one
    with pytest.raises(TypeError):
        api.group_by_collect(k)
    with pytest.raises(ValueError, match="rows"):
        api.group_by_collect(k, np.arange(3))                           # unequal lengths
    with pytest.raises(ValueError, match="rows"):
        api.group_by_collect(k, np.zeros((3, 4)))                       # the FIRST dimension counts
    with pytest.raises(ValueError, match="rows"):
        api.group_by_collect(k, np.float64(1.0))                        # no dimension at all
    with pytest.raises(ValueError, match="rows"):
        api.group_by_collect(torch.arange(4), torch.zeros(5))
    with pytest.raises(TypeError, match="keys"):
        api.group_by_collect(np.array(["a", "b"]), np.arange(2))


def test_flash_join_exposes_both_names():
    import flash_join
    from flash_hash_join_amd import api
    assert flash_join.group_rows is api.group_rows and flash_join.group_by_collect is api.group_by_collect
    assert callable(flash_join.group_rows) and callable(flash_join.group_by_collect)
    assert "group_rows" in api.__all__ and "group_by_collect" in api.__all__
    assert api.ROW_EXTENSIONS == ["group_rows", "group_by_collect"]
    assert "group_rows" not in api.EXTENSIONS and "group_by_collect" not in api.EXTENSIONS
    assert flash_join.factorize is api.factorize                        # the group of every row stays factorize's
