"""Probe-order joins (FJ_ALGO_PROBE_ORDER, csrc/fj_aligned.hip; api.lookup / isin / lookup_indices): one output row per probe row, at
the probe row's position.  The C-ABI contract and the argument checks need no GPU; on an MI355X every form is compared element for
element with a NumPy reference on every plan: empty sides, zero, one and two passes, a deep plan, the skewed partition, the
HBM-table fallback, scalar_hbm_table, the hash domain's special keys, a direct ctypes call on guarded buffers and one large case
checked on the device.

Reference: a stable argsort of the build keys, then searchsorted of the probe keys - the smallest build row per key (first
occurrence); no hashing anywhere, never the library."""
import ctypes
import functools
import os
import re
import zlib

import numpy as np
import pytest

import hbm_timings
import keymix
from conftest import ROOT

MANY, LEFT, ANTI, ROW_IDS, FULL, ALL, PO = 0x10, 0x20, 0x40, 0x80, 0x100, 0x200, 0x800
U64_MAX = np.uint64(2**64 - 1)
ODD = np.uint64(0x9E3779B97F4A7C15)
FILL = 2**64 - 3


def ref_probe_order(bk, pk):
    """(mask as bool, first-occurrence build row per probe row as int64, -1 where there is none)"""
    bk, pk = np.asarray(bk, dtype=np.uint64), np.asarray(pk, dtype=np.uint64)
    if bk.size == 0:
        return np.zeros(pk.size, dtype=bool), np.full(pk.size, -1, np.int64)
    order = np.argsort(bk, kind="stable")
    sb = bk[order]
    lo = np.searchsorted(sb, pk, "left")
    hit = (lo < sb.size) & (sb[np.minimum(lo, sb.size - 1)] == pk)
    idx = np.where(hit, order[np.minimum(lo, sb.size - 1)], -1).astype(np.int64)
    return hit, idx


def ref_lookup(bk, bv, pk, fill=0):
    hit, idx = ref_probe_order(bk, pk)
    bv = np.asarray(bv, dtype=np.uint64)
    vals = np.full(pk.size, np.uint64(fill), dtype=np.uint64)
    vals[hit] = bv[idx[hit]]
    return hit, idx, vals


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_header_flag_and_python_mirror():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    assert int(re.search(r"#define FJ_ALGO_PROBE_ORDER (0x[0-9a-fA-F]+)", hdr).group(1), 16) == 0x800
    from flash_hash_join_amd import api
    assert api.ALGO_PROBE_ORDER == 0x800


def test_abi_version_and_function_count_are_unchanged():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    assert int(re.search(r"#define FJ_ABI_VERSION (\d+)", hdr).group(1)) == 8
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert len(set(re.findall(r"\b(fj_[a-z0-9_]+)\s*\(", code))) == 40
    assert "FJ_ALGO_PROBE_ORDER" in hdr                               # (what makes this test one of the new feature's)
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_abi_version() == 8 and len(_lib.SYMBOLS) == 40


def test_flash_join_exposes_the_three_functions():
    import flash_join
    from flash_hash_join_amd import api
    for name in ("lookup", "isin", "lookup_indices"):
        assert callable(getattr(flash_join, name)) and name in api.EXTENSIONS


def _device_call(algo, materialize=1, bv=0x20000, mask=0x40000, vals=0x50000, cap=1000, nb=100, n_p=1000):
    from flash_hash_join_amd import _lib
    cnt = ctypes.c_uint64(0)
    rc = _lib.load().fj_join_device(None, algo, 0, materialize, 0x10000, bv, nb, 0x30000, n_p, None, 64, ctypes.byref(cnt), mask, vals, cap, None)
    return rc, _lib.last_error()


DEVICE_REFUSALS = [   # id, keyword arguments of _device_call, needles
    ("many", dict(algo=PO | MANY), ("FJ_ALGO_PROBE_ORDER cannot be combined with FJ_ALGO_MANY_TO_MANY",)),
    ("left", dict(algo=PO | LEFT), ("FJ_ALGO_PROBE_ORDER cannot be combined with FJ_ALGO_LEFT_OUTER",)),
    ("anti", dict(algo=PO | ANTI | 2), ("FJ_ALGO_PROBE_ORDER cannot be combined with FJ_ALGO_ANTI",)),
    ("full", dict(algo=PO | FULL), ("FJ_ALGO_PROBE_ORDER cannot be combined with FJ_ALGO_FULL_OUTER",)),
    ("all_copies", dict(algo=PO | ALL), ("FJ_ALGO_PROBE_ORDER cannot be combined with FJ_ALGO_ALL_COPIES",)),
    ("left_all_copies_row_ids", dict(algo=PO | LEFT | ALL | ROW_IDS), ("FJ_ALGO_PROBE_ORDER cannot be combined with FJ_ALGO_",)),
    ("count", dict(algo=PO, materialize=0), ("FJ_ALGO_PROBE_ORDER", "materialize = 1")),
    ("count_row_ids", dict(algo=PO | ROW_IDS, materialize=0), ("materialize = 1",)),
    ("no_output", dict(algo=PO, mask=None, vals=None), ("FJ_ALGO_PROBE_ORDER", "needs an output")),
    ("capacity", dict(algo=PO, cap=999), ("output capacity",)),
    ("capacity_mask_only", dict(algo=PO | 1, vals=None, bv=None, cap=0), ("output capacity",)),
    ("misaligned_values", dict(algo=PO, vals=0x50004), ("d_out_vals", "8-byte aligned")),
    ("values_without_build_values", dict(algo=PO | 2, bv=None), ("d_build_vals",)),
]


@pytest.mark.parametrize("cid,kw,needles", DEVICE_REFUSALS, ids=[r[0] for r in DEVICE_REFUSALS])
def test_invalid_combinations_are_refused_before_any_device_work(cid, kw, needles):
    """A NULL context: the checks come before the context is touched (no GPU needed; the pointers are never dereferenced)."""
    rc, err = _device_call(**kw)
    assert rc != 0 and "null context" not in err, err
    for needle in needles:
        assert needle in err, err


VALID = [   # id, keyword arguments of _device_call
    ("values_only", dict(algo=PO, mask=None)),
    ("mask_only", dict(algo=PO, vals=None, bv=None)),
    ("mask_only_with_build_values", dict(algo=PO, vals=None)),
    ("mask_at_an_odd_address", dict(algo=PO, mask=0x40003)),
    ("both", dict(algo=PO)),
    ("row_ids_null_build_values", dict(algo=PO | ROW_IDS, bv=None)),
    ("row_ids_mask_only", dict(algo=PO | ROW_IDS, bv=None, vals=None)),
    ("base_adaptive", dict(algo=PO | 0)),
    ("base_scalar", dict(algo=PO | 1)),
    ("base_radix", dict(algo=PO | 2)),
    ("more_capacity_than_rows", dict(algo=PO | 2, cap=5000)),
]


@pytest.mark.parametrize("cid,kw", VALID, ids=[v[0] for v in VALID])
def test_valid_combinations_reach_the_context(cid, kw):
    rc, err = _device_call(**kw)
    assert rc != 0 and "null context" in err, err


def test_the_next_free_bit_and_other_bases_are_still_unknown():
    for algo, needle in ((0x400, "unknown algo 1024"), (PO | 0x400, "unknown algo"), (PO | 9, "unknown algo"), (PO | 3, "unknown algo")):
        rc, err = _device_call(algo=algo)
        assert rc != 0 and needle in err and "null context" not in err, (hex(algo), err)


HOST_REFUSALS = [   # id, algo, materialize, build values, want mask, want values, needles
    ("many", PO | MANY, 1, True, True, True, ("FJ_ALGO_PROBE_ORDER cannot be combined with FJ_ALGO_MANY_TO_MANY",)),
    ("left", PO | LEFT, 1, True, True, True, ("FJ_ALGO_PROBE_ORDER cannot be combined with FJ_ALGO_LEFT_OUTER",)),
    ("anti", PO | ANTI, 1, True, True, True, ("FJ_ALGO_PROBE_ORDER cannot be combined with FJ_ALGO_ANTI",)),
    ("full", PO | FULL | 2, 1, True, True, True, ("FJ_ALGO_PROBE_ORDER cannot be combined with FJ_ALGO_FULL_OUTER",)),
    ("all_copies", PO | ALL, 1, True, True, True, ("FJ_ALGO_PROBE_ORDER cannot be combined with FJ_ALGO_ALL_COPIES",)),
    ("count", PO, 0, True, True, True, ("FJ_ALGO_PROBE_ORDER", "materialize = 1")),
    ("no_output", PO, 1, True, False, False, ("needs an output",)),
    ("values_without_build_values", PO, 1, False, True, True, ("build values",)),
    ("next_bit", 0x400, 1, True, True, True, ("unknown algo",)),
    ("base_9", PO | 9, 1, True, True, True, ("unknown algo",)),
]


@pytest.mark.parametrize("cid,algo,materialize,bv,want_mask,want_vals,needles", HOST_REFUSALS, ids=[r[0] for r in HOST_REFUSALS])
def test_host_entry_refusals(cid, algo, materialize, bv, want_mask, want_vals, needles):
    """fj_join_host makes the same checks before its context is created (no GPU needed)."""
    from flash_hash_join_amd import _lib
    L = _lib.load()
    k = np.arange(8, dtype=np.uint64)
    cnt, sec = ctypes.c_uint64(0), ctypes.c_double(0)
    om, ov = ctypes.c_void_p(), ctypes.c_void_p()
    rc = L.fj_join_host(algo, 0, materialize, k.ctypes.data, k.ctypes.data if bv else None, 8, k.ctypes.data, 8, ctypes.byref(cnt), ctypes.byref(sec),
                        ctypes.byref(om) if want_mask else None, ctypes.byref(ov) if want_vals else None)
    err = _lib.last_error()
    assert rc != 0 and "null context" not in err and "HIP device" not in err, err
    for needle in needles:
        assert needle in err, err
    assert not om.value and not ov.value


def test_python_argument_errors():
    from flash_hash_join_amd import api
    k = np.arange(4, dtype=np.uint64)
    with pytest.raises(ValueError, match="build_values has 3 elements"):
        api.lookup(k, k[:3], k)
    for bad in (1.5, "7", None, True):
        with pytest.raises(TypeError, match="fill_value"):
            api.lookup(k, k, k, fill_value=bad)
    with pytest.raises(ValueError, match="64 bits"):
        api.lookup(k, k, k, fill_value=2**64)
    with pytest.raises(ValueError, match="build_values"):
        api.lookup(k, None, k)


def test_numpy_reference_on_a_hand_written_case():
    bk = np.array([5, 7, 7, 9, 2**64 - 1, 0, 2**64 - 1], dtype=np.uint64)
    bv = np.array([50, 70, 71, 90, 11, 12, 13], dtype=np.uint64)
    pk = np.array([7, 3, 5, 7, 2**64 - 1, 4, 0, 3], dtype=np.uint64)
    hit, idx, vals = ref_lookup(bk, bv, pk, fill=99)
    assert hit.tolist() == [True, False, True, True, True, False, True, False]
    assert idx.tolist() == [1, -1, 0, 1, 4, -1, 5, -1]                 # key 7 -> row 1, 2^64 - 1 -> row 4: the first occurrences
    assert vals.tolist() == [70, 99, 50, 70, 11, 99, 12, 99]
    hit, idx = ref_probe_order(np.empty(0, np.uint64), pk)
    assert not hit.any() and np.all(idx == -1)
    hit, idx = ref_probe_order(bk, np.array([2**64 - 1, 2**64 - 2], dtype=np.uint64))     # a probe key beyond every build key but one
    assert hit.tolist() == [True, False] and idx.tolist() == [4, -1]


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fj():
    import flash_join
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_device_count() >= 1, "no HIP device: the product path must not silently fall back"
    assert flash_join.initialize() is None
    return flash_join


def _values_for(bk):
    """distinct per row (every copy of a key is recognisable), never 0, never the fill word, never a 0xA5A5.. word"""
    bv = (np.arange(bk.size, dtype=np.uint64) + np.uint64(1)) * ODD
    assert not np.isin(bv, np.array([0, FILL, 0xA5A5A5A5A5A5A5A5], dtype=np.uint64)).any()
    return bv


def _case(nb, n_p, hit, seed, dups=True):
    rng = np.random.default_rng(seed)
    bk = rng.integers(0, 2**64, size=nb, dtype=np.uint64)
    if not dups:
        bk = np.unique(bk)
        rng.shuffle(bk)
        nb = bk.size
    if nb >= 8:
        bk[0], bk[1] = 0, U64_MAX                                         # raw zero and raw 2^64 - 1: the HBM table's empty marker
        bk[2], bk[3] = keymix.EMPTY_RAW, keymix.FILLER_RAW                # the LDS tables' empty marker and the wide kernel's filler
        if dups:
            d = max(1, nb // 20)
            bk[nb - d:] = bk[4:4 + d]                                     # duplicated build keys, with other values
            bk[nb - d - 1] = keymix.EMPTY_RAW                             # ... the marker among them
    nhit = int(n_p * hit) if nb else 0
    parts = [rng.choice(bk, nhit)] if nhit else []                        # (probe keys repeat)
    parts.append(rng.integers(1, 2**63, size=n_p - nhit, dtype=np.uint64) * np.uint64(2) + np.uint64(2**63))   # ~never a build key
    pk = np.concatenate(parts)[:n_p] if n_p else np.empty(0, np.uint64)
    if n_p >= 16 and 0.0 < hit < 1.0:
        pk[:4] = np.array([0, 2**64 - 1, keymix.EMPTY_RAW, keymix.FILLER_RAW], dtype=np.uint64)   # ... on the probe side too
    rng.shuffle(pk)
    return bk, _values_for(bk), pk


class Ref:
    """a case and its reference, computed once"""
    def __init__(self, bk, bv, pk):
        self.bk, self.bv, self.pk = bk, bv, pk
        self.hit, self.idx, self.vals = ref_lookup(bk, bv, pk, fill=FILL)
        self.m = int(self.hit.sum())
        self._dev = None

    def args(self, device):
        if not device:
            return self.bk, self.bv, self.pk
        if self._dev is None:
            import torch
            self._dev = tuple(torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda() for a in (self.bk, self.bv, self.pk))
        return self._dev


def _host(a, dtype):
    if hasattr(a, "cpu"):
        assert a.is_cuda and str(a.dtype) == "torch." + dtype, a.dtype
        return a.cpu().numpy()
    assert a.dtype == np.dtype(dtype), a.dtype
    return a


def check_all_forms(fj, r, device, after=None, semi=True):
    """lookup (mask, non-zero fill), lookup without a mask and fill 0, isin, lookup_indices - element for element; after(name, timings)"""
    bk, bv, pk = r.args(device)
    n_p = r.pk.size
    note = (lambda fn: after(fn, fj.last_timings())) if after else (lambda fn: None)
    m, sec, vals, mask = fj.lookup(bk, bv, pk, fill_value=FILL, return_mask=True)
    note("lookup")
    assert isinstance(m, int) and isinstance(sec, float)
    vals, mask = _host(vals, "int64").view(np.uint64), _host(mask, "uint8")
    assert vals.shape == mask.shape == (n_p,)
    assert np.array_equal(mask, r.hit.astype(np.uint8)), "lookup: mask"
    assert np.array_equal(vals, r.vals), "lookup: values (first occurrence, fill_value where there is no partner)"
    assert m == r.m == int(mask.sum())
    m, _, vals = fj.lookup(bk, bv, pk)
    note("lookup(values only)")
    assert m == r.m and np.array_equal(_host(vals, "int64").view(np.uint64), np.where(r.hit, r.vals, np.uint64(0))), "lookup: fill 0, no mask"
    m, _, mask = fj.isin(pk, bk)
    note("isin")
    mask = _host(mask, "uint8")
    assert m == r.m == int(mask.sum()) and np.array_equal(mask, r.hit.astype(np.uint8)), "isin"
    m, _, idx = fj.lookup_indices(bk, pk)
    note("lookup_indices")
    assert m == r.m and np.array_equal(_host(idx, "int64"), r.idx), "lookup_indices: not the FIRST build row / -1"
    if semi:
        assert fj.semi_join_count(bk, pk)[0] == r.m


CASES = [   # id, nb, np, plan_target_keys, duplicates, passes
    ("nb0", 0, 1000, 4096, True, None),
    ("nb1", 1, 1000, 4096, True, None),
    ("np0", 1000, 0, 4096, True, None),
    ("zero_pass", 3000, 200_000, 4096, True, lambda p: p == 0),
    ("zero_pass_unique", 3000, 200_000, 4096, False, lambda p: p == 0),
    ("one_pass", 200_000, 1_000_000, 4096, True, lambda p: p == 1),
    ("one_pass_unique", 200_000, 1_000_000, 4096, False, lambda p: p == 1),
    ("two_pass", 3_000_000, 4_000_000, 4096, True, lambda p: p == 2),
    ("deep", 60_000, 400_000, 32, True, lambda p: p >= 2),
]


@functools.lru_cache(maxsize=None)
def _ref_case(cid):
    _, nb, n_p, _, dups, _ = next(c for c in CASES if c[0] == cid)
    return Ref(*_case(nb, n_p, 0.5, seed=zlib.crc32(cid.encode()) % 1000, dups=dups))


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("cid", [c[0] for c in CASES])
def test_parity_with_the_numpy_reference(fj, cid, device):
    _, nb, n_p, target, dups, passes = next(c for c in CASES if c[0] == cid)
    r = _ref_case(cid)
    if nb >= 8:
        assert (np.unique(r.bk).size < r.bk.size) == dups

    def after(fn, lt):
        if passes is not None:
            assert lt["path"] == 0 and lt["fell_back"] == 0 and passes(lt["passes"]) and lt["emit_ms"] == 0.0, (fn, lt)
    fj.set_option("plan_target_keys", target)
    try:
        check_all_forms(fj, r, device, after=after)
    finally:
        fj.set_option("plan_target_keys", 4096)


def _hash_w1(k):                                                   # fj_hash_w1 of csrc/fj_common.h
    return keymix.hash_w1(k)


@functools.lru_cache(maxsize=1)
def _oversized_case():
    cand = np.arange(1, 5_000_000, dtype=np.uint64)
    part = _hash_w1(cand) >> np.uint32(23)                             # top 9 hash bits: the final partition of a 9-bit plan
    sel = []
    for p in range(140):
        c = cand[part == p][:8500]
        assert c.size == 8500
        sel.append(c)
    one = np.concatenate(sel)
    np.random.default_rng(5).shuffle(one)
    bk = np.concatenate([one, one[:2000]])
    pk = np.concatenate([bk[::3], cand[-200000:]])
    return Ref(bk, _values_for(bk), pk)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_partitions_beyond_the_lds_table_fall_back_to_the_hbm_table(fj, device):
    """140 of the plan's 512 partitions hold 8500 distinct build keys each - beyond the 8192-slot table: the whole join runs again on
    the HBM table (fell_back == 1), still with first-occurrence values and build rows, in every form (the mask form has the same table)."""
    def after(fn, lt):
        assert lt["fell_back"] == 1 and lt["path"] == 1, (fn, lt)
        hbm_timings.check_hbm_form(lt, fn)
    check_all_forms(fj, _oversized_case(), device, after=after)


@functools.lru_cache(maxsize=1)
def _skew_case():
    cand = np.arange(1, 400000, dtype=np.uint64)
    skew = cand[(_hash_w1(cand) >> np.uint32(27)) == 0][:9000]
    assert skew.size == 9000
    bk = np.concatenate([skew, skew[:300]])
    pk = np.concatenate([bk, cand[:50000]])
    return Ref(bk, _values_for(bk), pk)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_a_skewed_partition(fj, device):
    """9000 build keys in one of the plan's 32 partitions: correct whichever rung serves it"""
    check_all_forms(fj, _skew_case(), device)


@pytest.mark.gpu
def test_scalar_hbm_table_path(fj):
    """hash_join's base value (FJ_ALGO_SCALAR) under scalar_hbm_table = 1: the global table from the start, every output form"""
    from flash_hash_join_amd import api
    r = Ref(*_case(50_000, 300_000, 0.6, seed=7))
    bk, bv, pk = r.args(True)
    S = api.ALGO_SCALAR | api.ALGO_PROBE_ORDER
    fj.set_option("scalar_hbm_table", 1)
    try:
        for want_mask in (False, True):
            m, _, vals, mask = api.join_device(S, 0, 1, bk, bv, pk, want_values=True, want_mask=want_mask)
            assert fj.last_timings()["path"] == 1 and fj.last_timings()["fell_back"] == 0
            hbm_timings.check_hbm_form(fj.last_timings())
            assert m == r.m and np.array_equal(vals.cpu().numpy().view(np.uint64), np.where(r.hit, r.vals, np.uint64(0)))
            assert (mask is None) if not want_mask else np.array_equal(mask.cpu().numpy(), r.hit.astype(np.uint8))
        m, _, vals, mask = api.join_device(S, 0, 1, bk, None, pk, want_values=False, want_mask=True)
        assert fj.last_timings()["path"] == 1
        hbm_timings.check_hbm_form(fj.last_timings())
        assert m == r.m and vals is None and np.array_equal(mask.cpu().numpy(), r.hit.astype(np.uint8))
        m, _, idx, mask = api.join_device(S | api.ALGO_ROW_IDS, 0, 1, bk, None, pk, want_values=True, want_mask=True)
        assert fj.last_timings()["path"] == 1
        hbm_timings.check_hbm_form(fj.last_timings())
        assert m == r.m and np.array_equal(idx.cpu().numpy(), r.idx) and np.array_equal(mask.cpu().numpy(), r.hit.astype(np.uint8))
        m, _, vals, mask = api._probe_order_host(S, r.bk, r.bv, r.pk, True, True)
        assert fj.last_timings()["path"] == 1
        hbm_timings.check_hbm_form(fj.last_timings())
        assert m == r.m and np.array_equal(vals, np.where(r.hit, r.vals, np.uint64(0))) and np.array_equal(mask, r.hit.astype(np.uint8))
    finally:
        fj.set_option("scalar_hbm_table", 0)


@pytest.mark.gpu
def test_hash_top_bits_48(fj):
    from flash_hash_join_amd import api
    r = _ref_case("one_pass")
    bk, bv, pk = r.args(True)
    m, _, idx, mask = api.join_device(api.ALGO_RADIX | api.ALGO_PROBE_ORDER | api.ALGO_ROW_IDS, 0, 1, bk, None, pk, hash_top_bits=48, want_mask=True)
    assert m == r.m and np.array_equal(idx.cpu().numpy(), r.idx) and np.array_equal(mask.cpu().numpy(), r.hit.astype(np.uint8))


# the hash domain's special keys, chosen as tests/test_special_keys.py chooses them: keymix.special_raw_keys for every radix_bits in
# 0..20 - the key whose mix is the tables' empty marker, the wide kernel's filler, their neighbours and the partition-edge keys
def _specials():
    keys = []
    for rb in range(21):
        for k in keymix.special_raw_keys(rb)[1].tolist():
            if k not in keys:
                keys.append(k)
    return np.array(keys, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _special_case(nb, n_p, arrangement):
    S = _specials()
    marker = np.uint64(keymix.EMPTY_RAW)
    rng = np.random.default_rng(nb % 1000 + 7 * len(arrangement))
    on_b, on_p = arrangement in ("both", "build_only"), arrangement in ("both", "probe_only")
    plain = np.unique(rng.integers(0, 2**64, size=nb, dtype=np.uint64))
    plain = plain[~np.isin(plain, S)]
    rng.shuffle(plain)
    bk = np.concatenate([plain] + ([S, np.full(2, marker), plain[:50]] if on_b else [plain[:50]]))      # the marker three times, 50 plain duplicates
    bk = bk[rng.permutation(bk.size)]
    miss = rng.integers(0, 2**64, size=n_p // 2, dtype=np.uint64)
    miss = miss[~np.isin(miss, S) & ~np.isin(miss, plain)]
    pk = np.concatenate([rng.choice(plain, n_p // 2), miss] + ([np.repeat(S, 3), np.full(3000, marker)] if on_p else []))
    pk = pk[rng.permutation(pk.size)]
    r = Ref(bk, _values_for(bk), pk)
    assert np.isin(S, bk).all() == on_b and np.isin(S, pk).all() == on_p
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("arrangement", ["both", "build_only", "probe_only"])
@pytest.mark.parametrize("depth,nb,n_p,passes", [("zero_pass", 3000, 50_000, 0), ("one_pass", 100_000, 200_000, 1)], ids=["zero_pass", "one_pass"])
def test_special_keys(fj, depth, nb, n_p, passes, arrangement, device):
    def after(fn, lt):
        assert lt["path"] == 0 and lt["fell_back"] == 0 and lt["passes"] == passes, (fn, lt)
    check_all_forms(fj, _special_case(nb, n_p, arrangement), device, after=after)


@pytest.mark.gpu
@pytest.mark.parametrize("base", [2, 1], ids=["partitioned", "hbm_table"])
@pytest.mark.parametrize("rid", [False, True], ids=["values", "row_ids"])
def test_direct_call_overwrites_every_row_and_nothing_else(fj, base, rid):
    """fj_join_device on buffers pre-filled with 0xA5 and 64 guard rows (bytes) behind row np: every row below np is overwritten (no
    reference value is a 0xA5A5.. word, the mask holds 0 / 1 only), the guards are intact, and no result is left pending."""
    import torch
    from flash_hash_join_amd import _lib, api
    L = _lib.load()
    r = _ref_case("one_pass")
    bk, bv, pk = r.args(True)
    n_p = r.pk.size
    exp = r.idx.view(np.uint64) if rid else np.where(r.hit, r.vals, np.uint64(0))
    assert not (exp == np.uint64(0xA5A5A5A5A5A5A5A5)).any()
    ctx = api.context(0)
    stream = torch.cuda.current_stream(0).cuda_stream
    A5 = int(np.array(0xA5A5A5A5A5A5A5A5, dtype=np.uint64).view(np.int64))
    ov = torch.full((n_p + 64,), A5, dtype=torch.int64, device="cuda")
    om = torch.full((n_p + 64 + 1,), 0xA5, dtype=torch.uint8, device="cuda")[1:]       # (an odd address: the mask needs no alignment)
    cnt = ctypes.c_uint64(0)
    t = _lib.FjTimings()
    algo = base | PO | (ROW_IDS if rid else 0)
    if base == 1:
        fj.set_option("scalar_hbm_table", 1)
    try:
        with api._ctx_locks.setdefault(0, __import__("threading").RLock()):
            # a pending result first: the probe-order call drops it
            _lib.check(L.fj_join_device(ctx, 2, 0, 1, bk.data_ptr(), bv.data_ptr(), r.bk.size, pk.data_ptr(), n_p, stream, 64, ctypes.byref(cnt), None, None, 0, None))
            _lib.check(L.fj_join_device(ctx, algo, 0, 1, bk.data_ptr(), None if rid else bv.data_ptr(), r.bk.size, pk.data_ptr(), n_p, stream, 64,
                                        ctypes.byref(cnt), om.data_ptr(), ov.data_ptr(), n_p, ctypes.byref(t)))
            assert L.fj_emit_pairs(ctx, ov.data_ptr(), ov.data_ptr(), n_p, stream, None) != 0, "a result was left pending"
    finally:
        fj.set_option("scalar_hbm_table", 0)
    assert t.path == (0 if base == 2 else 1) and t.emit_ms == 0.0
    hv, hm = ov.cpu().numpy().view(np.uint64), om.cpu().numpy()
    assert int(cnt.value) == r.m
    assert np.all(hv[n_p:] == np.uint64(0xA5A5A5A5A5A5A5A5)) and np.all(hm[n_p:] == 0xA5), "a row behind row np was written"
    assert not (hv[:n_p] == np.uint64(0xA5A5A5A5A5A5A5A5)).any() and np.isin(hm[:n_p], (0, 1)).all(), "a row below np was not written"
    assert np.array_equal(hv[:n_p], exp) and np.array_equal(hm[:n_p], r.hit.astype(np.uint8))


@pytest.mark.gpu
def test_large_case_checked_on_the_device(fj):
    """20M x 100M at 50 % hits: torch.isin for the mask, a sorted build side + searchsorted for values and build rows"""
    import torch
    from flash_hash_join_amd import datagen
    nb, n_p = 20_000_000, 100_000_000
    bk, bv = datagen.build_device(nb, "cuda:0")
    pk, expected = datagen.probe_device(n_p, nb, "cuda:0", seed=3, hit_bp=5000)
    m, _, vals, mask = fj.lookup(bk, bv, pk, return_mask=True)
    assert m == expected and 0.45 * n_p < m < 0.55 * n_p
    assert vals.dtype == torch.int64 and mask.dtype == torch.uint8 and vals.numel() == mask.numel() == n_p
    want = torch.isin(pk, bk)
    assert torch.equal(mask.bool(), want) and int(mask.sum()) == m
    sb, order = torch.sort(bk)                                         # (the generator's build keys are unique)
    pos = torch.searchsorted(sb, pk).clamp_(max=nb - 1)
    row = torch.where(want, order[pos], torch.full_like(pos, -1))
    del sb, pos, order
    assert torch.equal(vals, torch.where(want, bv[row.clamp(min=0)], torch.zeros_like(vals)))
    del vals, mask
    m, _, idx = fj.lookup_indices(bk, pk)
    assert m == expected and torch.equal(idx, row)
    del idx, row
    m, _, mask = fj.isin(pk, bk)
    assert m == expected and torch.equal(mask.bool(), want)
    del mask, want
    torch.cuda.empty_cache()
