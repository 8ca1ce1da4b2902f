"""Build-order aggregate joins (FJ_ALGO_BUILD_ORDER, csrc/fj_group.hip; api.group_join_count / group_join_sum): one output word per
build row, at the build row's position.  The C-ABI contract and the argument checks need no GPU; on an MI355X both forms are compared
element for element with a NumPy reference on every plan: empty sides, zero, one and two passes, a deep plan, a hot key, the HBM-table
fallback, scalar_hbm_table, radix_threshold, repeated calls, pre-filled and guarded buffers.

Reference: a stable sort of the probe keys, then searchsorted of the build keys on both sides - counts are the widths of the ranges,
sums the differences of a wrapping uint64 cumulative sum of the sorted probe values; no hashing anywhere, never the library."""
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

MANY, LEFT, ANTI, ROW_IDS, FULL, ALL, PO, BO = 0x10, 0x20, 0x40, 0x80, 0x100, 0x200, 0x800, 0x1000
U64_MAX = np.uint64(2**64 - 1)


def ref_group(bk, pk, pv=None):
    """(counts as int64, sums as uint64 or None), aligned with bk"""
    bk, pk = np.asarray(bk, dtype=np.uint64), np.asarray(pk, dtype=np.uint64)
    order = np.argsort(pk, kind="stable")
    sp = pk[order]
    lo, hi = np.searchsorted(sp, bk, "left"), np.searchsorted(sp, bk, "right")
    counts = (hi - lo).astype(np.int64)
    if pv is None:
        return counts, None
    cs = np.concatenate([np.zeros(1, np.uint64), np.cumsum(np.asarray(pv, dtype=np.uint64)[order], dtype=np.uint64)])   # wraps modulo 2^64
    return counts, cs[hi] - cs[lo]


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_header_flag_and_python_mirror():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    assert int(re.search(r"#define FJ_ALGO_BUILD_ORDER (0x[0-9a-fA-F]+)", hdr).group(1), 16) == 0x1000
    from flash_hash_join_amd import api
    assert api.ALGO_BUILD_ORDER == 0x1000


def test_abi_version_and_function_count_are_unchanged():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    assert int(re.search(r"#define FJ_ABI_VERSION (\d+)", hdr).group(1)) == 8
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert len(set(re.findall(r"\b(fj_[a-z0-9_]+)\s*\(", code))) == 40
    assert "FJ_ALGO_BUILD_ORDER" in hdr                               # (what makes this test one of the new feature's)
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_abi_version() == 8 and len(_lib.SYMBOLS) == 40


def test_flash_join_exposes_the_two_functions():
    import flash_join
    from flash_hash_join_amd import api
    for name in ("group_join_count", "group_join_sum"):
        assert callable(getattr(flash_join, name)) and name in api.EXTENSIONS and name in api.__all__


def _device_call(algo, materialize=1, pv=0x20000, counts=0x40000, sums=0x50000, cap=100, nb=100, n_p=1000):
    from flash_hash_join_amd import _lib
    cnt = ctypes.c_uint64(0)
    rc = _lib.load().fj_join_device(None, algo, 0, materialize, 0x10000, pv, nb, 0x30000, n_p, None, 64, ctypes.byref(cnt), counts, sums, cap, None)
    return rc, _lib.last_error()


DEVICE_REFUSALS = [   # id, keyword arguments of _device_call, needles
    ("many", dict(algo=BO | MANY), ("FJ_ALGO_BUILD_ORDER cannot be combined with FJ_ALGO_MANY_TO_MANY",)),
    ("left", dict(algo=BO | LEFT), ("FJ_ALGO_BUILD_ORDER cannot be combined with FJ_ALGO_LEFT_OUTER",)),
    ("anti", dict(algo=BO | ANTI | 2), ("FJ_ALGO_BUILD_ORDER cannot be combined with FJ_ALGO_ANTI",)),
    ("row_ids", dict(algo=BO | ROW_IDS), ("FJ_ALGO_BUILD_ORDER cannot be combined with FJ_ALGO_ROW_IDS",)),
    ("full", dict(algo=BO | FULL), ("FJ_ALGO_BUILD_ORDER cannot be combined with FJ_ALGO_FULL_OUTER",)),
    ("all_copies", dict(algo=BO | ALL), ("FJ_ALGO_BUILD_ORDER cannot be combined with FJ_ALGO_ALL_COPIES",)),
    ("probe_order", dict(algo=BO | PO | 1), ("FJ_ALGO_BUILD_ORDER cannot be combined with FJ_ALGO_PROBE_ORDER",)),
    ("left_all_copies", dict(algo=BO | LEFT | ALL), ("FJ_ALGO_BUILD_ORDER cannot be combined with FJ_ALGO_",)),
    ("count", dict(algo=BO, materialize=0), ("FJ_ALGO_BUILD_ORDER", "materialize = 1")),
    ("no_output", dict(algo=BO, counts=None, sums=None), ("FJ_ALGO_BUILD_ORDER", "needs an output")),
    ("capacity", dict(algo=BO, cap=99), ("output capacity",)),
    ("capacity_counts_only", dict(algo=BO | 1, sums=None, pv=None, cap=0), ("output capacity",)),
    ("misaligned_counts", dict(algo=BO, counts=0x40004), ("8-byte aligned",)),
    ("misaligned_sums", dict(algo=BO | 2, sums=0x50004), ("8-byte aligned",)),
    ("sums_without_probe_values", dict(algo=BO | 2, pv=None), ("d_build_vals",)),
    ("sums_only_without_probe_values", dict(algo=BO, pv=None, counts=None), ("d_build_vals",)),
]


@pytest.mark.parametrize("cid,kw,needles", DEVICE_REFUSALS, ids=[r[0] for r in DEVICE_REFUSALS])
def test_invalid_combinations_are_refused_before_any_device_work(cid, kw, needles):
    """A NULL context: the checks come before the context is touched (no GPU needed; the pointers are never dereferenced)."""
    rc, err = _device_call(**kw)
    assert rc != 0 and "null context" not in err, err
    for needle in needles:
        assert needle in err, err


VALID = [   # id, keyword arguments of _device_call
    ("counts_only", dict(algo=BO, sums=None)),
    ("counts_only_null_probe_values", dict(algo=BO, sums=None, pv=None)),
    ("sums_only", dict(algo=BO, counts=None)),
    ("both", dict(algo=BO)),
    ("base_adaptive", dict(algo=BO | 0)),
    ("base_scalar", dict(algo=BO | 1)),
    ("base_radix", dict(algo=BO | 2)),
    ("more_capacity_than_rows", dict(algo=BO | 2, cap=5000)),
    ("more_probe_rows_than_capacity", dict(algo=BO, cap=100, n_p=10**6)),
]


@pytest.mark.parametrize("cid,kw", VALID, ids=[v[0] for v in VALID])
def test_valid_combinations_reach_the_context(cid, kw):
    rc, err = _device_call(**kw)
    assert rc != 0 and "null context" in err, err


def test_the_next_free_bit_and_other_bases_are_still_unknown():
    for algo, needle in ((0x2000, "unknown algo 8192"), (0x400, "unknown algo 1024"), (BO | 0x2000, "unknown algo"), (BO | 0x400, "unknown algo"),
                         (BO | 9, "unknown algo"), (BO | 3, "unknown algo")):
        rc, err = _device_call(algo=algo)
        assert rc != 0 and needle in err and "null context" not in err, (hex(algo), err)


HOST_REFUSALS = [   # id, algo, materialize, probe values, want counts, want sums, needles
    ("many", BO | MANY, 1, True, True, True, ("FJ_ALGO_BUILD_ORDER cannot be combined with FJ_ALGO_MANY_TO_MANY",)),
    ("left", BO | LEFT, 1, True, True, True, ("FJ_ALGO_BUILD_ORDER cannot be combined with FJ_ALGO_LEFT_OUTER",)),
    ("anti", BO | ANTI, 1, True, True, True, ("FJ_ALGO_BUILD_ORDER cannot be combined with FJ_ALGO_ANTI",)),
    ("row_ids", BO | ROW_IDS, 1, True, True, True, ("FJ_ALGO_BUILD_ORDER cannot be combined with FJ_ALGO_ROW_IDS",)),
    ("full", BO | FULL | 2, 1, True, True, True, ("FJ_ALGO_BUILD_ORDER cannot be combined with FJ_ALGO_FULL_OUTER",)),
    ("all_copies", BO | ALL, 1, True, True, True, ("FJ_ALGO_BUILD_ORDER cannot be combined with FJ_ALGO_ALL_COPIES",)),
    ("probe_order", BO | PO, 1, True, True, True, ("FJ_ALGO_BUILD_ORDER cannot be combined with FJ_ALGO_PROBE_ORDER",)),
    ("count", BO, 0, True, True, True, ("FJ_ALGO_BUILD_ORDER", "materialize = 1")),
    ("no_output", BO, 1, True, False, False, ("needs an output",)),
    ("sums_without_probe_values", BO, 1, False, True, True, ("build_vals",)),
    ("next_bit", 0x2000, 1, True, True, True, ("unknown algo",)),
    ("base_9", BO | 9, 1, True, True, True, ("unknown algo",)),
]


@pytest.mark.parametrize("cid,algo,materialize,pv,want_counts,want_sums,needles", HOST_REFUSALS, ids=[r[0] for r in HOST_REFUSALS])
def test_host_entry_refusals(cid, algo, materialize, pv, want_counts, want_sums, needles):
    """fj_join_host makes the same checks before its context is created (no GPU needed)."""
    from flash_hash_join_amd import _lib
    L = _lib.load()
    k = np.arange(8, dtype=np.uint64)
    cnt, sec = ctypes.c_uint64(0), ctypes.c_double(0)
    oc, osum = ctypes.c_void_p(), ctypes.c_void_p()
    rc = L.fj_join_host(algo, 0, materialize, k.ctypes.data, k.ctypes.data if pv else None, 8, k.ctypes.data, 8, ctypes.byref(cnt), ctypes.byref(sec),
                        ctypes.byref(oc) if want_counts else None, ctypes.byref(osum) if want_sums else None)
    err = _lib.last_error()
    assert rc != 0 and "null context" not in err and "HIP device" not in err, err
    for needle in needles:
        assert needle in err, err
    assert not oc.value and not osum.value


def test_python_argument_errors():
    from flash_hash_join_amd import api
    k = np.arange(4, dtype=np.uint64)
    with pytest.raises(ValueError, match="probe_values has 3 elements"):
        api.group_join_sum(k, k, k[:3])
    with pytest.raises(ValueError, match="probe_values has 5 elements"):
        api.group_join_sum(k, k, np.arange(5, dtype=np.uint64), return_counts=True)
    with pytest.raises(ValueError, match="probe_values"):
        api.group_join_sum(k, k, None)
    with pytest.raises(TypeError):
        api.group_join_sum(k, k)                                       # probe_values is not optional
    with pytest.raises(TypeError, match="probe_values"):
        api.group_join_sum(k, k, np.array(["a", "b", "c", "d"]))


def test_numpy_reference_on_a_hand_written_case():
    bk = np.array([5, 7, 9, 7, 2**64 - 1, 0], dtype=np.uint64)         # 7 twice, 9 without a probe row
    pk = np.array([7, 3, 5, 7, 2**64 - 1, 7, 0, 2**64 - 1], dtype=np.uint64)
    pv = np.array([1, 2, 4, 8, 2**63, 16, 32, 2**63 + 3], dtype=np.uint64)
    counts, sums = ref_group(bk, pk, pv)
    assert counts.dtype == np.int64 and counts.tolist() == [1, 3, 0, 3, 2, 1]
    assert sums.dtype == np.uint64 and sums.tolist() == [4, 25, 0, 25, 3, 32]      # 2^63 + 2^63 + 3 wraps to 3
    assert int(counts.sum()) == 10                                     # P: pairs of the many-to-many inner join
    counts, sums = ref_group(bk, np.empty(0, np.uint64), np.empty(0, np.uint64))
    assert counts.tolist() == [0] * 6 and sums.tolist() == [0] * 6
    counts, sums = ref_group(np.empty(0, np.uint64), pk)
    assert counts.size == 0 and sums is None


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fj():
    import flash_join
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_device_count() >= 1, "no HIP device: the product path must not silently fall back"
    assert flash_join.initialize() is None
    return flash_join


def _values_for(rng, n):
    """random full-width words, never 0: the sums wrap"""
    pv = rng.integers(0, 2**64, size=n, dtype=np.uint64)
    pv[pv == 0] = np.uint64(1)
    return pv


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
            bk[nb - d:] = bk[4:4 + d]                                     # duplicated build keys
            bk[nb - d - 1] = keymix.EMPTY_RAW                             # ... the marker among them
    nhit = int(n_p * hit) if nb else 0
    parts = [rng.choice(bk, nhit)] if nhit else []                        # (probe keys repeat)
    parts.append(rng.integers(1, 2**63, size=n_p - nhit, dtype=np.uint64) * np.uint64(2) + np.uint64(2**63))   # ~never a build key
    pk = np.concatenate(parts)[:n_p] if n_p else np.empty(0, np.uint64)
    if n_p >= 16 and 0.0 < hit < 1.0:
        pk[:8] = np.array([0, 2**64 - 1, keymix.EMPTY_RAW, keymix.FILLER_RAW] * 2, dtype=np.uint64)   # ... on the probe side too
    rng.shuffle(pk)
    return bk, pk, _values_for(rng, pk.size)


class Ref:
    """a case and its reference, computed once"""
    def __init__(self, bk, pk, pv):
        self.bk, self.pk, self.pv = bk, pk, pv
        self.counts, self.sums = ref_group(bk, pk, pv)
        self.P = int(self.counts.sum())
        self._dev = None

    def args(self, device):
        if not device:
            return self.bk, self.pk, self.pv
        if self._dev is None:
            import torch
            self._dev = tuple(torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda() for a in (self.bk, self.pk, self.pv))
        return self._dev


def _host(a):
    if hasattr(a, "cpu"):
        assert a.is_cuda and str(a.dtype) == "torch.int64", a.dtype
        return a.cpu().numpy()
    assert isinstance(a, np.ndarray) and a.dtype == np.int64, a.dtype
    return a


def check_all_forms(fj, r, device, after=None, inner=False):
    """group_join_count, group_join_sum, group_join_sum(return_counts=True) - element for element; after(name, timings)"""
    bk, pk, pv = r.args(device)
    nb = r.bk.size
    note = (lambda fn: after(fn, fj.last_timings())) if after else (lambda fn: None)
    P, sec, counts = fj.group_join_count(bk, pk)
    note("group_join_count")
    assert isinstance(P, int) and isinstance(sec, float)
    counts = _host(counts)
    assert counts.shape == (nb,) and np.array_equal(counts, r.counts), "group_join_count: counts"
    assert P == r.P == int(counts.sum())
    P, _, sums = fj.group_join_sum(bk, pk, pv)
    note("group_join_sum")
    sums = _host(sums).view(np.uint64)
    assert sums.shape == (nb,) and np.array_equal(sums, r.sums), "group_join_sum: sums"
    assert P == r.P, "group_join_sum: P is the sum of all counts, duplicated build keys included"
    P, _, sums, counts = fj.group_join_sum(bk, pk, pv, return_counts=True)
    note("group_join_sum(return_counts)")
    assert P == r.P and np.array_equal(_host(sums).view(np.uint64), r.sums) and np.array_equal(_host(counts), r.counts), "both outputs"
    # every copy of a duplicated build key carries the same aggregate
    order = np.argsort(r.bk, kind="stable")
    same = r.bk[order][1:] == r.bk[order][:-1]
    c, s = _host(counts)[order], _host(sums)[order]
    assert np.all(c[1:][same] == c[:-1][same]) and np.all(s[1:][same] == s[:-1][same])
    if inner:
        assert fj.inner_join_count(bk, bk, pk)[0] == r.P


CASES = [   # id, nb, np, plan_target_keys, duplicates, passes, compare P with inner_join_count
    ("nb0", 0, 1000, 4096, True, None, True),
    ("nb1", 1, 1000, 4096, True, None, True),
    ("np0", 1000, 0, 4096, True, None, True),
    ("zero_pass", 3000, 200_000, 4096, True, lambda p: p == 0, True),
    ("zero_pass_unique", 3000, 200_000, 4096, False, lambda p: p == 0, True),
    ("one_pass", 200_000, 1_000_000, 4096, True, lambda p: p == 1, True),
    ("one_pass_unique", 200_000, 1_000_000, 4096, False, lambda p: p == 1, True),
    ("two_pass", 3_000_000, 4_000_000, 4096, True, lambda p: p == 2, False),
    ("deep", 60_000, 400_000, 32, True, lambda p: p >= 2, False),
]


@functools.lru_cache(maxsize=None)
def _ref_case(cid):
    _, nb, n_p, _, dups, _, _ = next(c for c in CASES if c[0] == cid)
    return Ref(*_case(nb, n_p, 0.5, seed=zlib.crc32(cid.encode()) % 1000, dups=dups))


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("cid", [c[0] for c in CASES])
def test_parity_with_the_numpy_reference(fj, cid, device):
    _, nb, n_p, target, dups, passes, inner = next(c for c in CASES if c[0] == cid)
    r = _ref_case(cid)
    if nb >= 8:
        assert (np.unique(r.bk).size < r.bk.size) == dups
    if n_p >= 16 and nb >= 8:
        assert 0.4 * n_p < np.isin(r.pk, r.bk).sum() < 0.6 * n_p and np.unique(r.pk).size < r.pk.size and not (r.pv == 0).any()

    def after(fn, lt):
        if passes is not None:
            assert lt["path"] == 0 and lt["fell_back"] == 0 and passes(lt["passes"]) and lt["emit_ms"] == 0.0, (fn, lt)
    fj.set_option("plan_target_keys", target)
    try:
        check_all_forms(fj, r, device, after=after, inner=inner)
    finally:
        fj.set_option("plan_target_keys", 4096)


@functools.lru_cache(maxsize=1)
def _hot_key_case():
    rng = np.random.default_rng(11)
    bk = np.unique(rng.integers(0, 2**64, size=200_000, dtype=np.uint64))[:199_951]
    hot = bk[1234]
    bk = np.concatenate([bk, np.full(49, hot)])                        # one key with 50 copies
    rng.shuffle(bk)
    assert bk.size == 200_000
    pk = np.concatenate([np.full(200_000, hot), rng.choice(bk, 200_000), rng.integers(0, 2**64, size=200_000, dtype=np.uint64)])
    rng.shuffle(pk)
    return Ref(bk, pk, _values_for(rng, pk.size))


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_a_hot_key(fj, device):
    """one key has 50 copies on the build side and a third of the probe rows: its LDS accumulator takes them all, every copy reads it"""
    r = _hot_key_case()
    assert r.counts.max() >= 200_000 and (r.counts == r.counts.max()).sum() == 50

    def after(fn, lt):
        assert lt["path"] == 0 and lt["fell_back"] == 0, (fn, lt)
    check_all_forms(fj, r, device, after=after, inner=True)


@pytest.mark.gpu
def test_the_same_call_twice_returns_the_same_arrays(fj):
    """accumulators and outputs are zeroed per call: a second call on the same context adds nothing to the first"""
    r = _ref_case("one_pass")
    for device in (False, True):
        for _ in range(2):
            check_all_forms(fj, r, device)


@pytest.mark.gpu
@pytest.mark.parametrize("base", [2, 1], ids=["partitioned", "hbm_table"])
def test_direct_call_defines_every_row_and_nothing_else(fj, base):
    """fj_join_device on buffers pre-filled with 0xA5 and 64 guard words behind word nb: every word below nb is defined by the call
    alone (the caller clears nothing), the guards are intact, and no result is left pending."""
    import threading
    import torch
    from flash_hash_join_amd import _lib, api
    L = _lib.load()
    r = _ref_case("one_pass")
    bk, pk, pv = r.args(True)
    nb, n_p = r.bk.size, r.pk.size
    ctx = api.context(0)
    stream = torch.cuda.current_stream(0).cuda_stream
    A5 = int(np.array(0xA5A5A5A5A5A5A5A5, dtype=np.uint64).view(np.int64))
    oc = torch.full((nb + 64,), A5, dtype=torch.int64, device="cuda")
    osum = torch.full((nb + 64,), A5, dtype=torch.int64, device="cuda")
    cnt = ctypes.c_uint64(0)
    t = _lib.FjTimings()
    if base == 1:
        fj.set_option("scalar_hbm_table", 1)
    try:
        with api._ctx_locks.setdefault(0, threading.RLock()):
            # a pending result first: the build-order call drops it
            _lib.check(L.fj_join_device(ctx, 2, 0, 1, bk.data_ptr(), bk.data_ptr(), nb, pk.data_ptr(), n_p, stream, 64, ctypes.byref(cnt), None, None, 0, None))
            _lib.check(L.fj_join_device(ctx, base | BO, 0, 1, bk.data_ptr(), pv.data_ptr(), nb, pk.data_ptr(), n_p, stream, 64,
                                        ctypes.byref(cnt), oc.data_ptr(), osum.data_ptr(), nb, ctypes.byref(t)))
            assert L.fj_emit_pairs(ctx, oc.data_ptr(), oc.data_ptr(), nb, stream, None) != 0, "a result was left pending"
    finally:
        fj.set_option("scalar_hbm_table", 0)
    assert t.path == (0 if base == 2 else 1) and t.emit_ms == 0.0
    hc, hs = oc.cpu().numpy(), osum.cpu().numpy().view(np.uint64)
    assert int(cnt.value) == r.P
    assert np.all(hc[nb:] == A5) and np.all(hs[nb:] == np.uint64(0xA5A5A5A5A5A5A5A5)), "a word behind word nb was written"
    assert np.array_equal(hc[:nb], r.counts) and np.array_equal(hs[:nb], r.sums)


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
    rng = np.random.default_rng(5)
    rng.shuffle(one)
    bk = np.concatenate([one, one[:2000], np.array([2**64 - 1, 2**64 - 1, 0], dtype=np.uint64)])
    pk = np.concatenate([bk[::3], bk[::7], cand[-200000:], np.full(5, 2**64 - 1, dtype=np.uint64)])
    return Ref(bk, pk, _values_for(rng, pk.size))


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_partitions_beyond_the_lds_table_fall_back_to_the_hbm_table(fj, device):
    """140 of the plan's 512 partitions hold 8500 distinct build keys each - beyond the 8192-slot table: the whole join runs again on
    the HBM table (fell_back == 1), whatever the partitioned attempt left in the outputs"""
    def after(fn, lt):
        assert lt["fell_back"] == 1 and lt["path"] == 1, (fn, lt)
        hbm_timings.check_hbm_form(lt, fn)
    check_all_forms(fj, _oversized_case(), device, after=after)


@pytest.mark.gpu
def test_scalar_hbm_table_path(fj):
    """hash_join's base value (FJ_ALGO_SCALAR) under scalar_hbm_table = 1: the global table from the start, every output form"""
    from flash_hash_join_amd import api
    r = Ref(*_case(50_000, 300_000, 0.6, seed=7))
    bk, pk, pv = r.args(True)
    S = api.ALGO_SCALAR | api.ALGO_BUILD_ORDER
    fj.set_option("scalar_hbm_table", 1)
    try:
        for want_counts, with_values in ((True, False), (False, True), (True, True)):
            P, _, counts, sums = api.join_device(S, 0, 1, bk, pv if with_values else None, pk, want_counts=want_counts)
            assert fj.last_timings()["path"] == 1 and fj.last_timings()["fell_back"] == 0
            hbm_timings.check_hbm_form(fj.last_timings())
            assert P == r.P
            assert (counts is None) if not want_counts else np.array_equal(counts.cpu().numpy(), r.counts)
            assert (sums is None) if not with_values else np.array_equal(sums.cpu().numpy().view(np.uint64), r.sums)
        P, _, counts, sums = api._group_host(S, r.bk, r.pk, r.pv, True)
        assert fj.last_timings()["path"] == 1
        hbm_timings.check_hbm_form(fj.last_timings())
        assert P == r.P and np.array_equal(counts, r.counts) and np.array_equal(sums.view(np.uint64), r.sums)
    finally:
        fj.set_option("scalar_hbm_table", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_radix_threshold_sends_the_adaptive_base_to_the_hbm_table(fj, device):
    r = Ref(*_case(50_000, 300_000, 0.5, seed=8))

    def after(fn, lt):
        assert lt["path"] == 1 and lt["fell_back"] == 0, (fn, lt)
        hbm_timings.check_hbm_form(lt, fn)
    fj.set_option("radix_threshold", r.bk.size + 1)
    try:
        check_all_forms(fj, r, device, after=after)
    finally:
        fj.set_option("radix_threshold", 0)


@pytest.mark.gpu
def test_device_form_writes_into_fresh_buffers_whatever_they_held(fj):
    """the device-tensor form allocates with torch.empty: fill the allocator's cache with a non-zero pattern of the same size first"""
    import torch
    r = _ref_case("zero_pass")
    bk, pk, pv = r.args(True)
    for _ in range(2):
        junk = [torch.full((r.bk.size,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda") for _ in range(4)]
        del junk
        P, _, sums, counts = fj.group_join_sum(bk, pk, pv, return_counts=True)
        assert P == r.P and np.array_equal(counts.cpu().numpy(), r.counts) and np.array_equal(sums.cpu().numpy().view(np.uint64), r.sums)
