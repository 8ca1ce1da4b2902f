"""A prepared build side (FJ_ALGO_RETAIN_BUILD / FJ_ALGO_REUSE_BUILD, csrc/fj_prepared.hip; api.build_index / api.Index): the build side
is partitioned and deduplicated to first occurrences once and probed many times by the probe-order forms.  The C-ABI contract and the
argument checks need no GPU; on an MI355X every form of every batch is compared element for element with a NumPy reference AND with
the one-shot lookup / isin / lookup_indices on the same inputs (outputs are positional: equality is exact, nothing is sorted), on every
plan, in the HBM-table form, with the hash domain's special keys, after the caller's arrays are gone, across other work on the context,
across a replacement, under a changed plan option, on guarded buffers and with two indexes alive.

Reference (that of tests/test_probe_order.py, restated): a stable argsort of the build keys, then searchsorted of the probe keys - the
smallest build row per key (first occurrence); no hashing anywhere, never the library."""
import ctypes
import functools
import gc
import os
import re
import zlib

import numpy as np
import pytest

import keymix
from conftest import ROOT

MANY, LEFT, ANTI, ROW_IDS, FULL, ALL, PO, BO, GB = 0x10, 0x20, 0x40, 0x80, 0x100, 0x200, 0x800, 0x1000, 0x40000
RETAIN, REUSE = 0x400000, 0x800000
U64_MAX = np.uint64(2**64 - 1)
ODD = np.uint64(0x9E3779B97F4A7C15)
FILL = 2**64 - 3
A5 = np.uint64(0xA5A5A5A5A5A5A5A5)


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
def test_header_flags_and_python_mirror():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    assert int(re.search(r"#define FJ_ALGO_RETAIN_BUILD\s+(0x[0-9a-fA-F]+)", hdr).group(1), 16) == RETAIN
    assert int(re.search(r"#define FJ_ALGO_REUSE_BUILD\s+(0x[0-9a-fA-F]+)", hdr).group(1), 16) == REUSE
    from flash_hash_join_amd import api
    assert api.ALGO_RETAIN_BUILD == RETAIN and api.ALGO_REUSE_BUILD == REUSE


def test_abi_version_and_function_count_are_unchanged():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    assert int(re.search(r"#define FJ_ABI_VERSION (\d+)", hdr).group(1)) == 8
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert len(set(re.findall(r"\b(fj_[a-z0-9_]+)\s*\(", code))) == 40
    assert "FJ_ALGO_RETAIN_BUILD" in hdr and "FJ_ALGO_REUSE_BUILD" in hdr      # (what makes this test one of the new feature's)
    assert not re.search(r"#define FJ_ALGO_\w+\s+0x200000\b", hdr), "bit 0x200000 stays unassigned"
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_abi_version() == 8 and len(_lib.SYMBOLS) == 40


def test_flash_join_exposes_build_index():
    import flash_join
    from flash_hash_join_amd import api
    assert callable(flash_join.build_index) and "build_index" in api.EXTENSIONS and "build_index" in api.__all__
    for name in ("lookup", "isin", "lookup_indices", "close", "__enter__", "__exit__"):
        assert callable(getattr(api.Index, name))


def _device_call(algo, materialize=1, bk=0x10000, bv=0x20000, nb=100, pk=0x30000, n_p=1000, mask=0x40000, vals=0x50000, cap=1000, top=64):
    from flash_hash_join_amd import _lib
    cnt = ctypes.c_uint64(0)
    rc = _lib.load().fj_join_device(None, algo, 0, materialize, bk, bv, nb, pk, n_p, None, top, ctypes.byref(cnt), mask, vals, cap, None)
    return rc, _lib.last_error()


NO_BUILD = dict(bk=None, bv=None, nb=0)
DEVICE_REFUSALS = [   # id, keyword arguments of _device_call, needles
    ("both_flags", dict(algo=PO | RETAIN | REUSE), ("FJ_ALGO_RETAIN_BUILD cannot be combined with FJ_ALGO_REUSE_BUILD",)),
    ("both_flags_no_build", dict(algo=PO | RETAIN | REUSE, **NO_BUILD), ("FJ_ALGO_RETAIN_BUILD cannot be combined with FJ_ALGO_REUSE_BUILD",)),
    ("retain_many", dict(algo=PO | RETAIN | MANY), ("FJ_ALGO_PROBE_ORDER cannot be combined with FJ_ALGO_MANY_TO_MANY",)),
    ("retain_left", dict(algo=PO | RETAIN | LEFT), ("FJ_ALGO_PROBE_ORDER cannot be combined with FJ_ALGO_LEFT_OUTER",)),
    ("reuse_anti", dict(algo=PO | REUSE | ANTI | 2, **NO_BUILD), ("FJ_ALGO_PROBE_ORDER cannot be combined with FJ_ALGO_ANTI",)),
    ("reuse_full", dict(algo=PO | REUSE | FULL, **NO_BUILD), ("FJ_ALGO_PROBE_ORDER cannot be combined with FJ_ALGO_FULL_OUTER",)),
    ("retain_all_copies", dict(algo=PO | RETAIN | ALL), ("FJ_ALGO_PROBE_ORDER cannot be combined with FJ_ALGO_ALL_COPIES",)),
    ("reuse_with_build_keys", dict(algo=PO | REUSE, bv=None, nb=0), ("FJ_ALGO_REUSE_BUILD takes no build side",)),
    ("reuse_with_build_values", dict(algo=PO | REUSE, bk=None, nb=0), ("FJ_ALGO_REUSE_BUILD takes no build side",)),
    ("reuse_with_build_rows", dict(algo=PO | REUSE, bk=None, bv=None, nb=100), ("FJ_ALGO_REUSE_BUILD takes no build side",)),
    ("reuse_with_a_build_side", dict(algo=PO | REUSE | ROW_IDS | 2), ("FJ_ALGO_REUSE_BUILD takes no build side",)),
    ("retain_no_output", dict(algo=PO | RETAIN, mask=None, vals=None), ("FJ_ALGO_PROBE_ORDER", "needs an output")),
    ("reuse_no_output", dict(algo=PO | REUSE, mask=None, vals=None, **NO_BUILD), ("FJ_ALGO_PROBE_ORDER", "needs an output")),
    ("retain_count", dict(algo=PO | RETAIN, materialize=0), ("materialize = 1",)),
    ("retain_only_count", dict(algo=PO | RETAIN, materialize=0, pk=None, n_p=0, mask=None, vals=None, cap=0), ("materialize = 1",)),
    ("reuse_count", dict(algo=PO | REUSE, materialize=0, **NO_BUILD), ("materialize = 1",)),
    ("retain_capacity", dict(algo=PO | RETAIN, cap=999), ("output capacity",)),
    ("reuse_capacity", dict(algo=PO | REUSE, cap=999, **NO_BUILD), ("output capacity",)),
    ("reuse_misaligned_values", dict(algo=PO | REUSE, vals=0x50004, **NO_BUILD), ("d_out_vals", "8-byte aligned")),
    ("retain_values_without_build_values", dict(algo=PO | RETAIN | 2, bv=None), ("d_build_vals",)),
    ("reuse_hash_top_bits", dict(algo=PO | REUSE, top=32, **NO_BUILD), ("hash_top_bits must be 64 or 48",)),
]


@pytest.mark.parametrize("cid,kw,needles", DEVICE_REFUSALS, ids=[r[0] for r in DEVICE_REFUSALS])
def test_invalid_combinations_are_refused_before_any_device_work(cid, kw, needles):
    """A NULL context: the checks come before the context is touched (no GPU needed; the pointers are never dereferenced)."""
    rc, err = _device_call(**kw)
    assert rc != 0 and "null context" not in err, err
    for needle in needles:
        assert needle in err, err


VALID = [   # id, keyword arguments of _device_call
    ("retain_values_and_mask", dict(algo=PO | RETAIN)),
    ("retain_values_only", dict(algo=PO | RETAIN | 2, mask=None)),
    ("retain_keys_only_mask", dict(algo=PO | RETAIN, bv=None, vals=None)),
    ("retain_row_ids_keys_only", dict(algo=PO | RETAIN | ROW_IDS | 1, bv=None)),
    ("retain_prepare_only", dict(algo=PO | RETAIN, pk=None, n_p=0, mask=None, vals=None, cap=0)),
    ("retain_prepare_only_keys_only", dict(algo=PO | RETAIN | 2, bv=None, pk=None, n_p=0, mask=None, vals=None, cap=0)),
    ("retain_empty_build_side", dict(algo=PO | RETAIN, **NO_BUILD)),
    ("retain_empty_prepare_only", dict(algo=PO | RETAIN, pk=None, n_p=0, mask=None, vals=None, cap=0, **NO_BUILD)),
    ("reuse_values_and_mask", dict(algo=PO | REUSE, **NO_BUILD)),
    ("reuse_values_only", dict(algo=PO | REUSE | 1, mask=None, **NO_BUILD)),
    ("reuse_mask_only_at_an_odd_address", dict(algo=PO | REUSE | 2, vals=None, mask=0x40003, **NO_BUILD)),
    ("reuse_row_ids", dict(algo=PO | REUSE | ROW_IDS, **NO_BUILD)),
    ("reuse_no_probe_rows", dict(algo=PO | REUSE, pk=None, n_p=0, mask=None, vals=None, cap=0, **NO_BUILD)),
    ("reuse_hash_top_bits_48", dict(algo=PO | REUSE, top=48, **NO_BUILD)),
]


@pytest.mark.parametrize("cid,kw", VALID, ids=[v[0] for v in VALID])
def test_valid_combinations_reach_the_context(cid, kw):
    rc, err = _device_call(**kw)
    assert rc != 0 and "null context" in err, err


def test_the_flags_modify_probe_order_only_and_the_free_bit_stays_unknown():
    cases = [(GB | 0x200000, dict(pk=None, n_p=0)), (RETAIN, {}), (REUSE, NO_BUILD), (BO | RETAIN, {}), (PO | 0x200000, {}),
             (GB | REUSE, dict(pk=None, n_p=0)), (RETAIN | REUSE, {}), (RETAIN | 2, {}), (ROW_IDS | REUSE, NO_BUILD),
             (PO | RETAIN | 3, {}), (PO | REUSE | 9, NO_BUILD)]
    for algo, kw in cases:
        rc, err = _device_call(algo=algo, **kw)
        assert rc != 0 and "unknown algo" in err and "null context" not in err, (hex(algo), err)
    rc, err = _device_call(algo=RETAIN)
    assert f"unknown algo {RETAIN}" in err, err                          # (the existing message, the whole algo word)


HOST = [   # id, algo, needles
    ("retain", PO | RETAIN, ("FJ_ALGO_RETAIN_BUILD", "fj_join_device")),
    ("reuse", PO | REUSE | 2, ("FJ_ALGO_REUSE_BUILD", "fj_join_device")),
    ("retain_row_ids", PO | RETAIN | ROW_IDS, ("FJ_ALGO_RETAIN_BUILD", "fj_join_device")),
    ("retain_without_probe_order", RETAIN, ("unknown algo",)),
    ("reuse_without_probe_order", REUSE | 2, ("unknown algo",)),
    ("free_bit", PO | 0x200000, ("unknown algo",)),
]


@pytest.mark.parametrize("cid,algo,needles", HOST, ids=[r[0] for r in HOST])
def test_host_entry_refuses_both_flags(cid, algo, needles):
    """fj_join_host's context is shared by every NumPy call of the process: no prepared side there (no GPU needed)."""
    from flash_hash_join_amd import _lib
    L = _lib.load()
    k = np.arange(8, dtype=np.uint64)
    cnt, sec = ctypes.c_uint64(0), ctypes.c_double(0)
    om, ov = ctypes.c_void_p(), ctypes.c_void_p()
    rc = L.fj_join_host(algo, 0, 1, k.ctypes.data, k.ctypes.data, 8, k.ctypes.data, 8, ctypes.byref(cnt), ctypes.byref(sec), ctypes.byref(om), ctypes.byref(ov))
    err = _lib.last_error()
    assert rc != 0 and "null context" not in err and "HIP device" not in err, err
    for needle in needles:
        assert needle in err, err
    assert not om.value and not ov.value


def test_python_argument_errors():
    from flash_hash_join_amd import api
    k = np.arange(4, dtype=np.uint64)
    with pytest.raises(ValueError, match="build_values has 3 elements"):
        api.build_index(k, k[:3])
    with pytest.raises(TypeError, match="cannot convert dtype"):
        api.build_index(np.array(["a"]))
    keys_only = api.Index(None, 0, 4, 4, False)                          # (no context behind it: what a closed index is)
    with pytest.raises(ValueError, match="without build_values"):
        keys_only.lookup(k)
    for bad in (1.5, "7", None, True):
        with pytest.raises(TypeError, match="fill_value"):
            keys_only.lookup(k, fill_value=bad)
    with pytest.raises(ValueError, match="64 bits"):
        keys_only.lookup(k, fill_value=2**64)
    closed = api.Index(None, 0, 4, 4, True)
    for call in (lambda: closed.lookup(k), lambda: closed.isin(k), lambda: closed.lookup_indices(k)):
        with pytest.raises(RuntimeError, match="closed"):
            call()
    closed.close()                                                       # (twice is fine)
    with closed as same:
        assert same is closed and (closed.num_rows, closed.num_keys, closed.has_values, closed.device) == (4, 4, True, 0)


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


def _build_side(nb, seed, dups):
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
    return bk, _values_for(bk)


def _batch(bk, n_p, seed):
    """about half the rows hit; probe keys repeat; the out-of-band keys are on the probe side too"""
    rng = np.random.default_rng(seed)
    nhit = n_p // 2 if bk.size else 0
    parts = [rng.choice(bk, nhit)] if nhit else []
    parts.append(rng.integers(1, 2**63, size=n_p - nhit, dtype=np.uint64) * np.uint64(2) + np.uint64(2**63))   # ~never a build key
    pk = np.concatenate(parts)[:n_p] if n_p else np.empty(0, np.uint64)
    if n_p >= 16:
        pk[:4] = np.array([0, 2**64 - 1, keymix.EMPTY_RAW, keymix.FILLER_RAW], dtype=np.uint64)
    rng.shuffle(pk)
    return pk


class Batch:
    """a probe batch and its reference, computed once"""
    def __init__(self, bk, bv, pk):
        self.pk = pk
        self.hit, self.idx, self.vals = ref_lookup(bk, bv, pk, fill=FILL)
        self.m = int(self.hit.sum())
        self._dev = None

    def keys(self, device):
        if not device:
            return self.pk
        if self._dev is None:
            self._dev = _cuda(self.pk)
        return self._dev


class Case:
    """a build side, its batches and their references, computed once"""
    def __init__(self, bk, bv, batches):
        self.bk, self.bv = bk, bv
        self.batches = [Batch(bk, bv, pk) for pk in batches]
        self._dev = None

    def build(self, device):
        if not device:
            return self.bk, self.bv
        if self._dev is None:
            self._dev = (_cuda(self.bk), _cuda(self.bv))
        return self._dev


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _host(a, dtype, device):
    if device:
        assert a.is_cuda and str(a.dtype) == "torch." + dtype, a.dtype
        return a.cpu().numpy()
    assert isinstance(a, np.ndarray) and a.dtype == np.dtype(dtype), a.dtype
    return a


def check_batch(fj, index, b, device, one_shot=None, after=None):
    """Index.lookup (mask, non-zero fill), lookup without a mask and fill 0, isin, lookup_indices against the reference, element for
    element; one_shot = (build keys, build values): also bit-identical to the module functions on the same inputs; after(name, timings)"""
    pk = b.keys(device)
    n_p = b.pk.size
    note = (lambda fn: after(fn, fj.last_timings())) if after else (lambda fn: None)
    m, sec, vals, mask = index.lookup(pk, fill_value=FILL, return_mask=True)
    note("lookup")
    assert isinstance(m, int) and isinstance(sec, float)
    vals, mask = _host(vals, "int64", device).view(np.uint64), _host(mask, "uint8", device)
    assert vals.shape == mask.shape == (n_p,)
    assert np.array_equal(mask, b.hit.astype(np.uint8)), "lookup: mask"
    assert np.array_equal(vals, b.vals), "lookup: values (first occurrence, fill_value where there is no partner)"
    assert m == b.m == int(mask.sum())
    m, _, vals0 = index.lookup(pk)
    note("lookup(values only)")
    vals0 = _host(vals0, "int64", device).view(np.uint64)
    assert m == b.m and np.array_equal(vals0, np.where(b.hit, b.vals, np.uint64(0))), "lookup: fill 0, no mask"
    m, _, mask2 = index.isin(pk)
    note("isin")
    mask2 = _host(mask2, "uint8", device)
    assert m == b.m == int(mask2.sum()) and np.array_equal(mask2, b.hit.astype(np.uint8)), "isin"
    m, _, idx = index.lookup_indices(pk)
    note("lookup_indices")
    idx = _host(idx, "int64", device)
    assert m == b.m and np.array_equal(idx, b.idx), "lookup_indices: not the FIRST build row / -1"
    if one_shot is not None:
        bk, bv = one_shot
        m1, _, v1, k1 = fj.lookup(bk, bv, pk, fill_value=FILL, return_mask=True)
        assert m1 == b.m and np.array_equal(_host(v1, "int64", device).view(np.uint64), vals) and np.array_equal(_host(k1, "uint8", device), mask)
        m1, _, v1 = fj.lookup(bk, bv, pk)
        assert m1 == b.m and np.array_equal(_host(v1, "int64", device).view(np.uint64), vals0)
        m1, _, k1 = fj.isin(pk, bk)
        assert m1 == b.m and np.array_equal(_host(k1, "uint8", device), mask2)
        m1, _, i1 = fj.lookup_indices(bk, pk)
        assert m1 == b.m and np.array_equal(_host(i1, "int64", device), idx)


CASES = [   # id, nb, plan_target_keys, passes of the prepared side, size of the batch larger than nb
    ("nb0", 0, 4096, None, 1000),
    ("nb1", 1, 4096, lambda p: p == 0, 1000),
    ("zero_pass", 3000, 4096, lambda p: p == 0, 200_000),
    ("one_pass", 200_000, 4096, lambda p: p == 1, 300_000),
    ("two_pass", 3_000_000, 4096, lambda p: p == 2, 3_500_000),
    ("deep", 60_000, 32, lambda p: p >= 2, 100_000),
]


@functools.lru_cache(maxsize=None)
def _plan_case(cid, dups):
    _, nb, _, _, big = next(c for c in CASES if c[0] == cid)
    seed = zlib.crc32(cid.encode()) % 1000
    bk, bv = _build_side(nb, seed, dups)
    if nb >= 8:
        assert (np.unique(bk).size < bk.size) == dups
    return Case(bk, bv, [_batch(bk, n, seed + 1 + i) for i, n in enumerate((0, 100, big))])


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("dups", [True, False], ids=["dups", "unique"])
@pytest.mark.parametrize("cid", [c[0] for c in CASES])
def test_every_plan_against_the_reference_and_the_one_shot_functions(fj, cid, dups, device):
    """np = 0, a batch smaller than a chunk and a batch larger than nb against one index, on the plan the build side's size chose"""
    _, nb, target, passes, _ = next(c for c in CASES if c[0] == cid)
    case = _plan_case(cid, dups)
    g = np.unique(case.bk).size

    def facts(fn, lt):
        if passes is not None:
            assert lt["path"] == 0 and lt["fell_back"] == 0 and passes(lt["passes"]), (fn, lt)

    def after(fn, lt):
        facts(fn, lt)
        assert lt["build_phase_ms"] == 0.0 and lt["emit_ms"] == 0.0, (fn, lt)
    fj.set_option("plan_target_keys", target)
    try:
        with fj.build_index(*case.build(device)) as index:
            facts("build_index", fj.last_timings())
            assert (index.num_rows, index.num_keys, index.has_values, index.device) == (case.bk.size, g, True, 0)
            for b in case.batches:
                check_batch(fj, index, b, device, one_shot=case.build(device), after=after)
    finally:
        fj.set_option("plan_target_keys", 4096)


def _hash_w1(k):                                                   # fj_hash_w1 of csrc/fj_common.h
    return keymix.hash_w1(k)


@functools.lru_cache(maxsize=1)
def _oversized_case():
    """the construction of tests/test_probe_order.py: 140 of a 9-bit plan's 512 partitions hold 8500 distinct build keys each"""
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
    return Case(bk, _values_for(bk), [np.concatenate([bk[::3], cand[-200000:]]), np.empty(0, np.uint64), cand[:100]])


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_partitions_beyond_the_lds_table_prepare_the_hbm_table_form(fj, device):
    case = _oversized_case()

    def after(fn, lt):
        assert lt["path"] == 1 and lt["fell_back"] == 0 and lt["passes"] == 0 and lt["build_phase_ms"] == 0.0, (fn, lt)
    with fj.build_index(*case.build(device)) as index:
        lt = fj.last_timings()
        assert lt["fell_back"] == 1 and lt["path"] == 1, lt
        assert index.num_keys == np.unique(case.bk).size
        for b in case.batches:
            check_batch(fj, index, b, device, after=after)


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
    assert np.isin(S, bk).all() == on_b and np.isin(S, pk).all() == on_p
    return Case(bk, _values_for(bk), [pk])


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("arrangement", ["both", "build_only", "probe_only"])
@pytest.mark.parametrize("depth,nb,n_p,passes", [("zero_pass", 3000, 50_000, 0), ("one_pass", 100_000, 200_000, 1)], ids=["zero_pass", "one_pass"])
def test_special_keys(fj, depth, nb, n_p, passes, arrangement, device):
    case = _special_case(nb, n_p, arrangement)

    def after(fn, lt):
        assert lt["path"] == 0 and lt["fell_back"] == 0 and lt["passes"] == passes and lt["build_phase_ms"] == 0.0, (fn, lt)
    with fj.build_index(*case.build(device)) as index:
        check_batch(fj, index, case.batches[0], device, one_shot=case.build(device), after=after)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_the_index_owns_its_copy_of_the_build_side(fj, device):
    """after build_index the caller's tensors are overwritten with garbage / the NumPy arrays freed: nothing changes"""
    case = _plan_case("one_pass", True)
    if device:
        bk, bv = (t.clone() for t in case.build(True))
    else:
        bk, bv = case.bk.copy(), case.bv.copy()
    index = fj.build_index(bk, bv)
    if device:
        import torch
        bk.fill_(0x5A5A5A5A5A5A5A5A)
        bv.fill_(0x5A5A5A5A5A5A5A5A)
        torch.cuda.synchronize()
    else:
        bk[:], bv[:] = 7, 7
    del bk, bv
    gc.collect()
    with index:
        for b in case.batches:
            check_batch(fj, index, b, device)


class Raw:
    """fj_join_device on a context of its own, device tensors in and out"""
    def __init__(self):
        from flash_hash_join_amd import _lib
        self.lib, self.L = _lib, _lib.load()
        self.ctx = self.L.fj_ctx_create(0)
        assert self.ctx, _lib.last_error()
        self.t = _lib.FjTimings()

    def close(self):
        self.L.fj_ctx_destroy(self.ctx)
        self.ctx = None

    def call(self, algo, bk=None, bv=None, pk=None, vals=None, mask=None, top=64, materialize=1):
        """rc, *out_count; outputs are written into the tensors given"""
        import torch
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        n_p = pk.numel() if pk is not None else 0
        cnt = ctypes.c_uint64(0)
        rc = self.L.fj_join_device(self.ctx, algo, 0, materialize, ptr(bk), ptr(bv), bk.numel() if bk is not None else 0, ptr(pk), n_p,
                                   torch.cuda.current_stream(0).cuda_stream, top, ctypes.byref(cnt), ptr(mask), ptr(vals), n_p, ctypes.byref(self.t))
        return rc, int(cnt.value)

    def probe(self, algo, pk, bk=None, bv=None, want_vals=True, want_mask=True, top=64):
        """rc, m, values as uint64, mask - of a probe-order call with fresh outputs"""
        import torch
        vals = torch.full((pk.numel(),), -1 - 0x5A, dtype=torch.int64, device="cuda") if want_vals else None
        mask = torch.full((pk.numel(),), 0xA5, dtype=torch.uint8, device="cuda") if want_mask else None
        rc, m = self.call(algo, bk, bv, pk, vals, mask, top)
        return rc, m, (vals.cpu().numpy().view(np.uint64) if want_vals else None), (mask.cpu().numpy() if want_mask else None)

    def check_reuse(self, b, values=True):
        """the three forms of FJ_ALGO_REUSE_BUILD against a batch's reference"""
        pk = b.keys(True)
        if values:
            rc, m, v, k = self.probe(PO | REUSE, pk)
            assert rc == 0, self.lib.last_error()
            assert m == b.m and np.array_equal(v, np.where(b.hit, b.vals, np.uint64(0))) and np.array_equal(k, b.hit.astype(np.uint8))
        rc, m, v, k = self.probe(PO | REUSE | ROW_IDS | 2, pk)
        assert rc == 0, self.lib.last_error()
        assert m == b.m and np.array_equal(v.view(np.int64), b.idx) and np.array_equal(k, b.hit.astype(np.uint8))
        rc, m, _, k = self.probe(PO | REUSE | 1, pk, want_vals=False)
        assert rc == 0, self.lib.last_error()
        assert m == b.m == int(k.sum()) and np.array_equal(k, b.hit.astype(np.uint8))
        assert self.t.build_phase_ms == 0.0


@pytest.fixture
def raw(fj):
    r = Raw()
    yield r
    r.close()


@pytest.mark.gpu
def test_other_work_on_the_context_leaves_the_prepared_side_alone(fj, raw):
    """RETAIN; then an inner join that grows the workspace, a group-by, a one-shot probe-order call and fj_ctx_trim on the SAME context;
    then REUSE: unchanged.  The prepared side is no workspace: after the trim the context reports what one that never held a
    prepared side reports."""
    import torch
    L = raw.L
    case = _plan_case("one_pass", True)
    bk, bv = case.build(True)
    b = case.batches[2]
    rc, g = raw.call(PO | RETAIN, bk, bv)
    assert rc == 0 and g == np.unique(case.bk).size, raw.lib.last_error()
    assert raw.t.passes == 1 and raw.t.path == 0 and raw.t.build_phase_ms > 0.0
    raw.check_reuse(b)
    ws_before = L.fj_ctx_workspace_bytes(raw.ctx)

    other = _plan_case("two_pass", False)
    obk, obv = other.build(True)
    opk = other.batches[2].keys(True)

    def unrelated(r):
        rc, n = r.call(2, obk, obv, opk)                                 # an inner join of 3M x 3.5M rows, counted and left pending
        assert rc == 0 and n == other.batches[2].m, r.lib.last_error()
        ok = torch.empty(obk.numel(), dtype=torch.int64, device="cuda")
        rc, n = r.call(GB | 2, obk, materialize=0)                       # COUNT(DISTINCT) ...
        assert rc == 0 and n == obk.numel(), r.lib.last_error()
        cnt = ctypes.c_uint64(0)
        rc = L.fj_join_device(r.ctx, GB | 2, 0, 1, obk.data_ptr(), None, obk.numel(), None, 0, torch.cuda.current_stream(0).cuda_stream, 64,
                              ctypes.byref(cnt), ok.data_ptr(), None, obk.numel(), None)             # ... and the group-by with its keys
        assert rc == 0 and cnt.value == obk.numel(), r.lib.last_error()
        rc, m, v, k = r.probe(PO | 2, opk, obk, obv)                     # a one-shot probe-order call, no flags
        assert rc == 0 and m == other.batches[2].m and np.array_equal(k, other.batches[2].hit.astype(np.uint8)), r.lib.last_error()
    unrelated(raw)
    assert L.fj_ctx_workspace_bytes(raw.ctx) > ws_before, "the unrelated join was meant to grow the workspace"
    raw.check_reuse(b)
    assert L.fj_ctx_trim(raw.ctx) == 0, raw.lib.last_error()
    fresh = Raw()
    try:
        unrelated(fresh)
        assert L.fj_ctx_trim(fresh.ctx) == 0
        assert L.fj_ctx_workspace_bytes(raw.ctx) == L.fj_ctx_workspace_bytes(fresh.ctx) == 0
    finally:
        fresh.close()
    for bb in case.batches:
        raw.check_reuse(bb)
    assert L.fj_emit_pairs(raw.ctx, bk.data_ptr(), bk.data_ptr(), 0, None, None) != 0, "the prepared side is not a pending result"


@pytest.mark.gpu
def test_replacement_and_refusals_on_a_live_context(fj, raw):
    first, second = _plan_case("one_pass", True), _plan_case("zero_pass", False)
    b1, b2 = first.batches[2], second.batches[2]
    lib = raw.lib
    # REUSE before any RETAIN: refused, the context stays usable
    rc, _, _, _ = raw.probe(PO | REUSE, b1.keys(True))
    assert rc != 0 and "without a prepared build side" in lib.last_error(), lib.last_error()
    # RETAIN with probe rows: the one-shot call's outputs, and the side stays
    bk, bv = first.build(True)
    rc, m, v, k = raw.probe(PO | RETAIN, b1.keys(True), bk, bv)
    assert rc == 0, lib.last_error()
    assert m == b1.m and np.array_equal(v, np.where(b1.hit, b1.vals, np.uint64(0))) and np.array_equal(k, b1.hit.astype(np.uint8))
    assert raw.t.build_phase_ms > 0.0 and raw.t.passes == 1 and raw.t.fell_back == 0
    raw.check_reuse(b1)
    # another hash_top_bits than the prepared side's
    rc, _, _, _ = raw.probe(PO | REUSE, b1.keys(True), top=48)
    assert rc != 0 and "hash_top_bits" in lib.last_error(), lib.last_error()
    raw.check_reuse(b1)
    # a second RETAIN replaces the first: a keys-only side (no d_build_vals) under another plan
    bk2, _ = second.build(True)
    rc, g = raw.call(PO | RETAIN | 2, bk2, None)
    assert rc == 0 and g == np.unique(second.bk).size and raw.t.passes == 0, lib.last_error()
    rc, _, _, _ = raw.probe(PO | REUSE, b2.keys(True))
    assert rc != 0 and "prepared with d_build_vals" in lib.last_error(), lib.last_error()
    rc, _, _, _ = raw.probe(PO | REUSE, b2.keys(True), want_mask=False)
    assert rc != 0 and "prepared with d_build_vals" in lib.last_error(), lib.last_error()
    raw.check_reuse(b2, values=False)                                    # (the mask and the row-id form always work)
    # RETAIN with nb == 0: every lookup misses
    rc, g = raw.call(PO | RETAIN, None, None)
    assert rc == 0 and g == 0, lib.last_error()
    rc, m, v, k = raw.probe(PO | REUSE, b1.keys(True))
    assert rc == 0 and m == 0 and not v.any() and not k.any(), lib.last_error()
    rc, m, v, k = raw.probe(PO | REUSE | ROW_IDS, b1.keys(True))
    assert rc == 0 and m == 0 and np.all(v == U64_MAX) and not k.any(), lib.last_error()
    # ... and a third RETAIN brings the first side back, at hash_top_bits = 48
    rc, g = raw.call(PO | RETAIN | 2, bk, bv, top=48)
    assert rc == 0 and g == np.unique(first.bk).size, lib.last_error()
    rc, m, v, k = raw.probe(PO | REUSE, b1.keys(True), top=48)
    assert rc == 0 and m == b1.m and np.array_equal(v, np.where(b1.hit, b1.vals, np.uint64(0))), lib.last_error()
    rc, _, _, _ = raw.probe(PO | REUSE, b1.keys(True))
    assert rc != 0 and "hash_top_bits" in lib.last_error(), lib.last_error()


@pytest.mark.gpu
def test_the_stored_plan_is_used_whatever_the_options_say_later(fj, raw):
    case = _plan_case("one_pass", True)
    bk, bv = case.build(True)
    try:
        rc, _ = raw.call(PO | RETAIN, bk, bv)
        assert rc == 0 and raw.t.passes == 1, raw.lib.last_error()
        bits = raw.t.radix_bits
        fj.set_option("plan_target_keys", 32)
        for b in case.batches:
            raw.check_reuse(b)
            assert raw.t.passes == 1 and raw.t.radix_bits == bits and raw.t.path == 0
        fj.set_option("scalar_hbm_table", 1)
        raw.check_reuse(case.batches[2])                                 # (the base value is ignored too: SCALAR in check_reuse's mask call)
        assert raw.t.path == 0 and raw.t.passes == 1
        rc, _ = raw.call(PO | RETAIN, bk, bv)                            # prepared under the deep plan now ...
        assert rc == 0 and raw.t.passes >= 2, raw.lib.last_error()
        deep = raw.t.passes
        fj.set_option("plan_target_keys", 4096)                          # ... and probed under the default options
        fj.set_option("scalar_hbm_table", 0)
        raw.check_reuse(case.batches[2])
        assert raw.t.passes == deep
    finally:
        fj.set_option("plan_target_keys", 4096)
        fj.set_option("scalar_hbm_table", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["partitioned", "hbm_table"])
@pytest.mark.parametrize("rid", [False, True], ids=["values", "row_ids"])
def test_direct_reuse_writes_every_row_and_nothing_else(fj, raw, form, rid):
    """FJ_ALGO_REUSE_BUILD into buffers with 64 guard rows (bytes) in front of row 0 and behind row np and a poisoned interior: every row
    below np is overwritten (no reference value is a 0xA5A5.. word, the mask holds 0 / 1 only), the guards are intact"""
    import torch
    case = _plan_case("one_pass", True)
    b = case.batches[2]
    bk, bv = case.build(True)
    pk, n_p = b.keys(True), b.pk.size
    exp = b.idx.view(np.uint64) if rid else np.where(b.hit, b.vals, np.uint64(0))
    assert not (exp == A5).any()
    if form == "hbm_table":
        fj.set_option("scalar_hbm_table", 1)
    try:
        rc, _ = raw.call(PO | RETAIN | 1, bk, None if rid else bv)
    finally:
        fj.set_option("scalar_hbm_table", 0)
    assert rc == 0 and raw.t.path == (1 if form == "hbm_table" else 0), raw.lib.last_error()
    word = int(np.array(A5, dtype=np.uint64).view(np.int64))
    ov = torch.full((64 + n_p + 64,), word, dtype=torch.int64, device="cuda")
    om = torch.full((1 + 64 + n_p + 64,), 0xA5, dtype=torch.uint8, device="cuda")[1:]      # (an odd address: the mask needs no alignment)
    rc, m = raw.call(PO | REUSE | (ROW_IDS if rid else 0), None, None, pk, ov[64:64 + n_p], om[64:64 + n_p])
    assert rc == 0, raw.lib.last_error()
    assert raw.t.path == (1 if form == "hbm_table" else 0) and raw.t.build_phase_ms == 0.0 and raw.t.emit_ms == 0.0
    hv, hm = ov.cpu().numpy().view(np.uint64), om.cpu().numpy()
    assert m == b.m
    assert np.all(hv[:64] == A5) and np.all(hv[64 + n_p:] == A5) and np.all(hm[:64] == 0xA5) and np.all(hm[64 + n_p:] == 0xA5), "a guard row was written"
    assert not (hv[64:64 + n_p] == A5).any() and np.isin(hm[64:64 + n_p], (0, 1)).all(), "a row below np was not written"
    assert np.array_equal(hv[64:64 + n_p], exp) and np.array_equal(hm[64:64 + n_p], b.hit.astype(np.uint8))


@pytest.mark.gpu
def test_two_indexes_at_once_and_mixed_inputs(fj):
    """two Index objects on one device, probed alternately; an index built from NumPy arrays probed with device tensors and the
    reverse; a keys-only index; close()"""
    import torch
    a, z = _plan_case("one_pass", True), _plan_case("zero_pass", False)
    ia, iz = fj.build_index(*a.build(False)), fj.build_index(*z.build(True))
    try:
        for _ in range(2):
            check_batch(fj, ia, a.batches[2], True)                      # (NumPy-built, device probes)
            check_batch(fj, iz, z.batches[2], False)                     # (device-built, NumPy probes)
            check_batch(fj, ia, a.batches[1], False)
            check_batch(fj, iz, z.batches[1], True)
        if torch.cuda.device_count() > 1:
            with pytest.raises(ValueError, match="on device 1"):
                ia.isin(a.batches[1].keys(True).to("cuda:1"))
        with pytest.raises(ValueError, match="device=1"):
            fj.build_index(a.build(True)[0], device=1)
    finally:
        ia.close()
        iz.close()
    with pytest.raises(RuntimeError, match="closed"):
        ia.isin(a.batches[1].pk)
    with fj.build_index(a.bk) as keys_only:
        assert not keys_only.has_values and keys_only.num_keys == np.unique(a.bk).size
        with pytest.raises(ValueError, match="without build_values"):
            keys_only.lookup(a.batches[1].pk)
        b = a.batches[2]
        m, _, mask = keys_only.isin(b.pk)
        assert m == b.m and np.array_equal(mask, b.hit.astype(np.uint8))
        m, _, idx = keys_only.lookup_indices(b.keys(True))
        assert m == b.m and np.array_equal(idx.cpu().numpy(), b.idx)
