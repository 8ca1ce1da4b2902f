"""Group ids for two-column keys (FJ_ALGO_KEY_PAIR, csrc/fj_groupby_pair.hip; api.factorize_columns / api.encode_keys): what needs no
GPU - the flag's value and its refusals in both entry points (a NULL context: the checks come before any device work), the combined
word fj_key_pair64 against its NumPy restatement, and the Python argument checks.  The GPU half is tests/test_factorize_columns.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import keymix
from conftest import ROOT

MANY, LEFT, ANTI, ROW_IDS, FULL, ALL, PO, BO = 0x10, 0x20, 0x40, 0x80, 0x100, 0x200, 0x800, 0x1000
MIN, MAX, SIGNED, GB, INV, AFLOAT, AALL, AARG, AMERGE = 0x4000, 0x8000, 0x10000, 0x40000, 0x100000, 0x2000000, 0x4000000, 0x8000000, 0x10000000
PAIR = 0x20000000
GIP = GB | INV | PAIR
PINNED_UNASSIGNED = (0x400, 0x2000, 0x20000, 0x80000, 0x200000)
SALT = 0x9E3779B97F4A7C15


def pair64(a, b):
    """fj_key_pair64 in NumPy: a ^ mix(b ^ C)"""
    return np.asarray(a, dtype=np.uint64) ^ keymix.mix(np.asarray(b, dtype=np.uint64) ^ np.uint64(SALT))


def test_header_flag_and_python_mirror():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    flags = {name: int(v, 16) for name, v in re.findall(r"#define (FJ_ALGO_[A-Z_]+)\s+(0x[0-9a-fA-F]+)", hdr)}
    assert flags["FJ_ALGO_KEY_PAIR"] == 0x20000000
    assert [n for n, v in flags.items() if v & 0x20000000] == ["FJ_ALGO_KEY_PAIR"], "another flag shares the bit"
    from flash_hash_join_amd import api
    assert api.ALGO_KEY_PAIR == 0x20000000
    mirrors = {n: v for n, v in vars(api).items() if n.startswith("ALGO_") and isinstance(v, int)}
    assert [n for n, v in mirrors.items() if v & 0x20000000] == ["ALGO_KEY_PAIR"]


def test_abi_version_and_function_count_are_unchanged():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    assert int(re.search(r"#define FJ_ABI_VERSION (\d+)", hdr).group(1)) == 8
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert len(set(re.findall(r"\b(fj_[a-z0-9_]+)\s*\(", code))) == 40
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_abi_version() == 8 and len(_lib.SYMBOLS) == 40
    assert "fj_key_pair64" in _lib.LAB_SYMBOLS and "fj_key_pair64" not in _lib.SYMBOLS
    assert "fj_key_pair64" not in open(os.path.join(ROOT, "flash_hash_join_amd", "csrc", "exports.map")).read()


def _device_call(algo, materialize=1, vals=0x20000, pk=None, n_p=0, ok=0x40000, ov=0x50000, cap=100, nb=100):
    from flash_hash_join_amd import _lib
    cnt = ctypes.c_uint64(0)
    rc = _lib.load().fj_join_device(None, algo, 0, materialize, 0x10000, vals, nb, pk, n_p, None, 64, ctypes.byref(cnt), ok, ov, cap, None)
    return rc, _lib.last_error()


DEVICE_REFUSALS = [   # id, keyword arguments of _device_call, needles
    # the flag without FJ_ALGO_GROUP_BY: an unknown algo that carries the whole word
    ("bare", dict(algo=PAIR), (f"unknown algo {PAIR}",)),
    ("bare_with_base", dict(algo=PAIR | 2), (f"unknown algo {PAIR | 2}",)),
    ("with_inverse_but_no_group_by", dict(algo=PAIR | INV), (f"unknown algo {PAIR | INV}",)),
    ("with_probe_order", dict(algo=PAIR | PO), (f"unknown algo {PAIR | PO}",)),
    ("with_build_order", dict(algo=PAIR | BO | 1), (f"unknown algo {PAIR | BO | 1}",)),
    # with FJ_ALGO_GROUP_BY but without FJ_ALGO_INVERSE: both flags are named
    ("no_inverse", dict(algo=GB | PAIR), ("FJ_ALGO_KEY_PAIR", "FJ_ALGO_INVERSE")),
    ("no_inverse_radix", dict(algo=GB | PAIR | 2), ("FJ_ALGO_KEY_PAIR", "FJ_ALGO_INVERSE")),
    ("no_inverse_row_ids", dict(algo=GB | PAIR | ROW_IDS), ("FJ_ALGO_KEY_PAIR", "FJ_ALGO_INVERSE")),
    ("no_inverse_count_only", dict(algo=GB | PAIR, materialize=0), ("FJ_ALGO_KEY_PAIR", "FJ_ALGO_INVERSE")),
    # its own: the second key column, the 40-bit positions
    ("no_second_column", dict(algo=GIP, vals=None), ("FJ_ALGO_KEY_PAIR", "d_build_vals")),
    ("no_second_column_scalar", dict(algo=GIP | 1, vals=None), ("FJ_ALGO_KEY_PAIR", "d_build_vals")),
    ("too_many_rows", dict(algo=GIP, nb=2**40 + 1, cap=2**40 + 1), ("FJ_ALGO_KEY_PAIR", "2^40")),
    ("misaligned_second_column", dict(algo=GIP, vals=0x20008), ("16-byte aligned",)),
    # everything FJ_ALGO_INVERSE refuses
    ("min", dict(algo=GIP | MIN), ("FJ_ALGO_INVERSE cannot be combined with FJ_ALGO_AGG_MIN",)),
    ("max", dict(algo=GIP | MAX | 2), ("FJ_ALGO_INVERSE cannot be combined with FJ_ALGO_AGG_MAX",)),
    ("signed", dict(algo=GIP | SIGNED | 1), ("FJ_ALGO_INVERSE cannot be combined with FJ_ALGO_AGG_SIGNED",)),
    ("row_ids", dict(algo=GIP | ROW_IDS), ("FJ_ALGO_INVERSE cannot be combined with FJ_ALGO_ROW_IDS",)),
    ("count_only", dict(algo=GIP, materialize=0), ("FJ_ALGO_INVERSE", "materialize = 1")),
    ("no_ids_output", dict(algo=GIP, ov=None), ("FJ_ALGO_INVERSE", "d_out_vals")),
    ("no_first_rows_output", dict(algo=GIP | 1, ok=None), ("FJ_ALGO_INVERSE", "d_out_keys")),
    ("capacity", dict(algo=GIP, cap=99), ("output capacity 99 < 100",)),
    ("misaligned_first_rows", dict(algo=GIP, ok=0x40004), ("8-byte aligned",)),
    ("misaligned_ids", dict(algo=GIP | 2, ov=0x50004), ("8-byte aligned",)),
    ("float", dict(algo=GIP | AFLOAT), ("FJ_ALGO_AGG_FLOAT cannot be combined with FJ_ALGO_INVERSE",)),
    ("agg_all", dict(algo=GIP | AALL), ("FJ_ALGO_AGG_ALL cannot be combined with FJ_ALGO_INVERSE",)),
    ("agg_arg", dict(algo=GIP | AARG | MIN), ("FJ_ALGO_AGG_ARG cannot be combined with FJ_ALGO_INVERSE",)),
    ("agg_merge", dict(algo=GIP | AALL | AMERGE), ("FJ_ALGO_AGG_MERGE cannot be combined with FJ_ALGO_INVERSE",)),
    # everything FJ_ALGO_GROUP_BY refuses
    ("many", dict(algo=GIP | MANY), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_MANY_TO_MANY",)),
    ("left", dict(algo=GIP | LEFT), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_LEFT_OUTER",)),
    ("anti", dict(algo=GIP | ANTI), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_ANTI",)),
    ("full", dict(algo=GIP | FULL), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_FULL_OUTER",)),
    ("all_copies", dict(algo=GIP | ALL), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_ALL_COPIES",)),
    ("probe_order", dict(algo=GIP | PO), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_PROBE_ORDER",)),
    ("build_order", dict(algo=GIP | BO), ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_BUILD_ORDER",)),
    ("probe_keys", dict(algo=GIP, pk=0x30000), ("FJ_ALGO_GROUP_BY", "no probe side")),
    ("probe_rows", dict(algo=GIP, n_p=7), ("FJ_ALGO_GROUP_BY", "no probe side")),
    ("base_3", dict(algo=GIP | 3), ("unknown algo",)),
]
for _bit in PINNED_UNASSIGNED:   # the five pinned bits stay unassigned: alone, and beside the full flag set
    DEVICE_REFUSALS.append((f"pinned_bit_{_bit:#x}_alone", dict(algo=_bit), (f"unknown algo {_bit}",)))
    DEVICE_REFUSALS.append((f"pinned_bit_{_bit:#x}_with_pair", dict(algo=GIP | _bit), ("unknown algo",)))


@pytest.mark.parametrize("cid,kw,needles", DEVICE_REFUSALS, ids=[r[0] for r in DEVICE_REFUSALS])
def test_invalid_combinations_are_refused_before_any_device_work(cid, kw, needles):
    """A NULL context: the checks come before the context is touched (no GPU needed; the pointers are never dereferenced)."""
    rc, err = _device_call(**kw)
    assert rc != 0 and "null context" not in err, err
    for needle in needles:
        assert needle in err, err


VALID = [(f"{('adaptive', 'scalar', 'radix')[base]}-{fid}", dict(algo=GIP | base, **kw)) for base in (0, 1, 2)
         for fid, kw in (("two_columns", dict()), ("more_capacity_than_rows", dict(cap=5000)), ("rows_2_to_40", dict(nb=2**40, cap=2**40)),
                         ("no_rows", dict(nb=0, cap=0, ok=None, ov=None, vals=None)))]


@pytest.mark.parametrize("cid,kw", VALID, ids=[v[0] for v in VALID])
def test_valid_combinations_reach_the_context(cid, kw):
    rc, err = _device_call(**kw)
    assert rc != 0 and "null context" in err, err


HOST_REFUSALS = [   # id, algo, materialize, second column, probe keys, np, nb, needles
    ("bare", PAIR, 1, True, False, 0, 8, (f"unknown algo {PAIR}",)),
    ("bare_with_base", PAIR | 2, 1, True, False, 0, 8, (f"unknown algo {PAIR | 2}",)),
    ("with_inverse_but_no_group_by", PAIR | INV, 1, True, False, 0, 8, (f"unknown algo {PAIR | INV}",)),
    ("with_probe_order", PAIR | PO, 1, True, False, 0, 8, (f"unknown algo {PAIR | PO}",)),
    ("no_inverse", GB | PAIR, 1, True, False, 0, 8, ("FJ_ALGO_KEY_PAIR", "FJ_ALGO_INVERSE")),
    ("no_inverse_row_ids", GB | PAIR | ROW_IDS | 2, 1, True, False, 0, 8, ("FJ_ALGO_KEY_PAIR", "FJ_ALGO_INVERSE")),
    ("no_inverse_count_only", GB | PAIR, 0, True, False, 0, 8, ("FJ_ALGO_KEY_PAIR", "FJ_ALGO_INVERSE")),
    ("no_second_column", GIP, 1, False, False, 0, 8, ("FJ_ALGO_KEY_PAIR", "build_vals")),
    ("too_many_rows", GIP | 1, 1, True, False, 0, 2**40 + 1, ("FJ_ALGO_KEY_PAIR", "2^40")),
    ("min", GIP | MIN, 1, True, False, 0, 8, ("FJ_ALGO_INVERSE cannot be combined with FJ_ALGO_AGG_MIN",)),
    ("max_signed", GIP | MAX | SIGNED, 1, True, False, 0, 8, ("FJ_ALGO_INVERSE cannot be combined with FJ_ALGO_AGG_MAX",)),
    ("signed", GIP | SIGNED, 1, True, False, 0, 8, ("FJ_ALGO_INVERSE cannot be combined with FJ_ALGO_AGG_SIGNED",)),
    ("row_ids", GIP | ROW_IDS | 1, 1, True, False, 0, 8, ("FJ_ALGO_INVERSE cannot be combined with FJ_ALGO_ROW_IDS",)),
    ("count_only", GIP, 0, True, False, 0, 8, ("FJ_ALGO_INVERSE", "materialize = 1")),
    ("float", GIP | AFLOAT, 1, True, False, 0, 8, ("FJ_ALGO_AGG_FLOAT cannot be combined with FJ_ALGO_INVERSE",)),
    ("agg_all", GIP | AALL, 1, True, False, 0, 8, ("FJ_ALGO_AGG_ALL cannot be combined with FJ_ALGO_INVERSE",)),
    ("agg_arg", GIP | AARG | MAX, 1, True, False, 0, 8, ("FJ_ALGO_AGG_ARG cannot be combined with FJ_ALGO_INVERSE",)),
    ("agg_merge", GIP | AALL | AMERGE, 1, True, False, 0, 8, ("FJ_ALGO_AGG_MERGE cannot be combined with FJ_ALGO_INVERSE",)),
    ("many", GIP | MANY, 1, True, False, 0, 8, ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_MANY_TO_MANY",)),
    ("left", GIP | LEFT, 1, True, False, 0, 8, ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_LEFT_OUTER",)),
    ("anti", GIP | ANTI, 1, True, False, 0, 8, ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_ANTI",)),
    ("full", GIP | FULL, 1, True, False, 0, 8, ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_FULL_OUTER",)),
    ("all_copies", GIP | ALL, 1, True, False, 0, 8, ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_ALL_COPIES",)),
    ("probe_order", GIP | PO, 1, True, False, 0, 8, ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_PROBE_ORDER",)),
    ("build_order", GIP | BO, 1, True, False, 0, 8, ("FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_BUILD_ORDER",)),
    ("probe_keys", GIP, 1, True, True, 0, 8, ("no probe side",)),
    ("probe_rows", GIP | 2, 1, True, True, 8, 8, ("no probe side",)),
    ("base_9", GIP | 9, 1, True, False, 0, 8, ("unknown algo",)),
]
for _bit in PINNED_UNASSIGNED:
    HOST_REFUSALS.append((f"pinned_bit_{_bit:#x}_alone", _bit, 1, True, False, 0, 8, (f"unknown algo {_bit}",)))
    HOST_REFUSALS.append((f"pinned_bit_{_bit:#x}_with_pair", GIP | _bit, 1, True, False, 0, 8, ("unknown algo",)))


def _host_call(algo, materialize, vals, pk, n_p, nb=8, want_first=True, want_ids=True):
    """(the refusals come before a byte of the columns is read: nb beyond the eight words is never dereferenced)"""
    from flash_hash_join_amd import _lib
    L = _lib.load()
    k = np.arange(8, dtype=np.uint64)
    cnt, sec = ctypes.c_uint64(0), ctypes.c_double(0)
    ok, ov = ctypes.c_void_p(), ctypes.c_void_p()
    rc = L.fj_join_host(algo, 0, materialize, k.ctypes.data, k.ctypes.data if vals else None, nb, k.ctypes.data if pk else None, n_p,
                        ctypes.byref(cnt), ctypes.byref(sec), ctypes.byref(ok) if want_first else None, ctypes.byref(ov) if want_ids else None)
    return rc, _lib.last_error(), ok, ov


@pytest.mark.parametrize("cid,algo,materialize,vals,pk,n_p,nb,needles", HOST_REFUSALS, ids=[r[0] for r in HOST_REFUSALS])
def test_host_entry_refusals(cid, algo, materialize, vals, pk, n_p, nb, needles):
    """fj_join_host makes the same checks before its context is created (no GPU needed)."""
    rc, err, ok, ov = _host_call(algo, materialize, vals, pk, n_p, nb)
    assert rc != 0 and "null context" not in err and "HIP device" not in err, err
    for needle in needles:
        assert needle in err, err
    assert not ok.value and not ov.value


@pytest.mark.parametrize("base", [0, 1, 2])
@pytest.mark.parametrize("want_first,want_ids", [(True, True), (True, False), (False, True)], ids=["both", "first_rows_alone", "ids_alone"])
def test_host_entry_accepts_every_valid_combination(base, want_first, want_ids):
    """past the argument checks: the call runs where there is a device, and fails on the missing device - never on a flag - elsewhere"""
    from flash_hash_join_amd import _lib
    rc, err, ok, ov = _host_call(GIP | base, 1, True, False, 0, 8, want_first, want_ids)
    try:
        assert rc == 0 or ("FJ_ALGO" not in err and "unknown algo" not in err), err
    finally:
        _lib.load().fj_free_host(ok)
        _lib.load().fj_free_host(ov)


def test_key_pair64_is_the_numpy_formula():
    from flash_hash_join_amd import _lib
    L = _lib.load()
    assert L.has_lab, "the tests run on the lab library"
    rng = np.random.default_rng(2024)
    special = [0, 2**64 - 1, keymix.EMPTY_RAW, keymix.FILLER_RAW]
    a = np.concatenate([rng.integers(0, 2**64, size=1000, dtype=np.uint64), np.array(special * 4, dtype=np.uint64)])
    b = np.concatenate([rng.integers(0, 2**64, size=1000, dtype=np.uint64), np.repeat(np.array(special, dtype=np.uint64), 4)])
    want = pair64(a, b)
    got = np.array([L.fj_key_pair64(int(x), int(y)) for x, y in zip(a, b)], dtype=np.uint64)
    assert np.array_equal(got, want)
    # any word w is reached from any b: a = w ^ mix(b ^ C)
    for w in special:
        bb = rng.integers(0, 2**64, size=5, dtype=np.uint64)
        aa = np.uint64(w) ^ keymix.mix(bb ^ np.uint64(SALT))
        assert all(L.fj_key_pair64(int(x), int(y)) == w for x, y in zip(aa, bb))
        assert np.all(pair64(aa, bb) == np.uint64(w))


def test_python_argument_errors():
    import torch
    from flash_hash_join_amd import api
    k = np.arange(4, dtype=np.uint64)
    with pytest.raises(ValueError, match="factorize"):
        api.factorize_columns(k)                                        # a single array: one column
    with pytest.raises(ValueError, match="factorize"):
        api.factorize_columns([k])
    with pytest.raises(ValueError, match="factorize"):
        api.factorize_columns(())
    with pytest.raises(ValueError, match="rows"):
        api.factorize_columns([k, k[:3]])                               # unequal lengths
    with pytest.raises(ValueError, match="rows"):
        api.factorize_columns([k, k, np.arange(5)])
    with pytest.raises(TypeError, match="one kind"):
        api.factorize_columns([k, torch.arange(4)])                     # NumPy and torch side by side
    with pytest.raises(TypeError, match="one kind"):
        api.factorize_columns((torch.arange(4), k.view(np.int64)))
    with pytest.raises(TypeError, match=r"columns\[1\]"):
        api.factorize_columns([k, np.array(["a", "b", "c", "d"])])      # a string column
    with pytest.raises(TypeError):
        api.factorize_columns()
    with pytest.raises(ValueError, match="same number"):
        api.encode_keys([k, k], [k])                                    # mismatched column counts
    with pytest.raises(ValueError, match="same number"):
        api.encode_keys(k, [k, k])
    with pytest.raises(ValueError, match="rows"):
        api.encode_keys([k, k[:2]], [k, k])
    with pytest.raises(TypeError, match="one kind"):
        api.encode_keys([k, k], [torch.arange(4), torch.arange(4)])
    with pytest.raises(TypeError, match=r"probe_columns\[0\]"):
        api.encode_keys([k, k], [np.array(["a"]), np.array([1])])


def test_flash_join_exposes_both_names():
    import flash_join
    from flash_hash_join_amd import api
    assert flash_join.factorize_columns is api.factorize_columns and flash_join.encode_keys is api.encode_keys
    assert "factorize_columns" in api.__all__ and "encode_keys" in api.__all__
    assert flash_join.factorize is api.factorize                        # one column stays factorize's
