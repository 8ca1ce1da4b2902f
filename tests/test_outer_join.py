"""Left outer and anti joins (FJ_ALGO_LEFT_OUTER / FJ_ALGO_ANTI, csrc/fj_outer.hip): the C-ABI contract, argument checks that need
no GPU, and - on an MI355X - parity with the NumPy reference on every plan (zero, one, two passes, deep plans), the global-table
path, the fallback of a partition beyond the LDS table, the pending-result rule and one large case checked on the device.

Reference: oracle.np_join (first occurrence of a duplicated build key wins) for the matched rows, pk[~np.isin(pk, bk)] for the
unmatched ones."""
import ctypes
import os
import re
import zlib

import numpy as np
import pytest

import hbm_timings
import keymix
from conftest import ROOT

U64_MAX = np.uint64(2**64 - 1)


def _np_outer(bk, bv, pk):
    """(m, matched keys, matched values, unmatched keys) of the NumPy reference."""
    from oracle.oracle import np_join
    bk, bv, pk = (np.asarray(x, dtype=np.uint64) for x in (bk, bv, pk))
    m, k, v = np_join(bk, bv, pk, return_arrays=True)
    return m, k, v, pk[~np.isin(pk, bk)]


def _sorted(a):
    return np.sort(np.asarray(a).reshape(-1).view(np.uint64))


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_header_flags_and_python_mirror():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    assert int(re.search(r"#define FJ_ALGO_LEFT_OUTER (0x[0-9a-fA-F]+)", hdr).group(1), 16) == 0x20
    assert int(re.search(r"#define FJ_ALGO_ANTI (0x[0-9a-fA-F]+)", hdr).group(1), 16) == 0x40
    from flash_hash_join_amd import api
    assert api.ALGO_LEFT_OUTER == 0x20 and api.ALGO_ANTI == 0x40


def test_flash_join_exposes_the_new_functions():
    import flash_join
    for name in ("left_join", "anti_join", "anti_join_count"):
        assert callable(getattr(flash_join, name)), name
    from flash_hash_join_amd import api
    assert {"left_join", "anti_join", "anti_join_count"} <= set(api.EXTENSIONS)


@pytest.mark.parametrize("algo,materialize,cap_less,misalign,needle", [
    (0x20 | 0x40, 1, 0, 0, "cannot be combined"),
    (0x20 | 0x10, 1, 0, 0, "MANY_TO_MANY"),
    (0x40 | 0x10, 0, 0, 0, "MANY_TO_MANY"),
    (0x20, 0, 0, 0, "needs materialize = 1"),
    (0x20 | 2, 1, 1, 0, "output capacity"),
    (0x40 | 1, 1, 1, 0, "output capacity"),
    (0x20, 1, 0, 4, "8-byte aligned"),
    (0x40, 1, 0, 4, "8-byte aligned"),
], ids=["both_flags", "left_many", "anti_many", "left_count", "left_capacity", "anti_capacity", "left_misaligned", "anti_misaligned"])
def test_invalid_combinations_are_refused_before_any_device_work(algo, materialize, cap_less, misalign, needle):
    """A NULL context: the checks come before the context is touched (no GPU needed; the pointers are never dereferenced)."""
    from flash_hash_join_amd import _lib
    L = _lib.load()
    nb, n_p = 100, 1000
    cnt = ctypes.c_uint64(0)
    rc = L.fj_join_device(None, algo, 0, materialize, 0x10000, 0x20000, nb, 0x30000, n_p, None, 64, ctypes.byref(cnt),
                          0x40000 + misalign, 0x50000, n_p - cap_less, None)
    assert rc != 0
    err = _lib.last_error()
    assert needle in err and "null context" not in err, err


def test_null_output_buffers_are_refused():
    from flash_hash_join_amd import _lib
    L = _lib.load()
    cnt = ctypes.c_uint64(0)
    assert L.fj_join_device(None, 0x20, 0, 1, 0x10000, 0x20000, 10, 0x30000, 10, None, 64, ctypes.byref(cnt), 0x40000, None, 10, None) != 0
    assert "output buffers" in _lib.last_error()
    # an anti join needs no value buffer: it gets as far as the (null) context
    assert L.fj_join_device(None, 0x40, 0, 1, 0x10000, None, 10, 0x30000, 10, None, 64, ctypes.byref(cnt), 0x40000, None, 10, None) != 0
    assert "null context" in _lib.last_error()


def test_numpy_reference_on_a_hand_written_case():
    bk = np.array([5, 7, 7, 9, 2**64 - 1, 0], dtype=np.uint64)
    bv = np.array([50, 70, 71, 90, 11, 1], dtype=np.uint64)
    pk = np.array([7, 3, 5, 7, 2**64 - 1, 4, 0, 3], dtype=np.uint64)
    m, k, v, anti = _np_outer(bk, bv, pk)
    assert m == 5
    pairs = sorted(zip(k.tolist(), v.tolist()))
    assert pairs == [(0, 1), (5, 50), (7, 70), (7, 70), (2**64 - 1, 11)]       # key 7: the first occurrence's value
    assert sorted(anti.tolist()) == [3, 3, 4]


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fj():
    import flash_join
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_device_count() >= 1, "no HIP device: the product path must not silently fall back"
    assert flash_join.initialize() is None
    return flash_join


def _case(nb, n_p, hit, seed):
    rng = np.random.default_rng(seed)
    bk = rng.integers(0, 2**64, size=nb, dtype=np.uint64)
    if nb >= 8:
        bk[0], bk[1] = 0, U64_MAX                                         # raw zero and raw 2^64 - 1: the HBM table's empty marker (an ordinary key in the hash domain)
        bk[2], bk[3] = keymix.EMPTY_RAW, keymix.FILLER_RAW                # the LDS tables' empty marker and the wide kernel's filler (mixed 2^64 - 1, 2^32 - 1)
        d = max(1, nb // 20)
        bk[nb - d:] = bk[4:4 + d]                                         # duplicated build keys, distinct values
    bv = rng.integers(0, 2**64, size=nb, dtype=np.uint64)
    nhit = int(n_p * hit) if nb else 0
    parts = [rng.choice(bk, nhit)] if nhit else []
    parts.append(rng.integers(1, 2**63, size=n_p - nhit, dtype=np.uint64) * np.uint64(2) + np.uint64(2**63))   # ~never a build key
    pk = np.concatenate(parts)[:n_p]
    if n_p >= 16 and 0.0 < hit < 1.0:
        pk[:4] = np.array([0, 2**64 - 1, keymix.EMPTY_RAW, keymix.FILLER_RAW], dtype=np.uint64)   # ... on the probe side too
    rng.shuffle(pk)
    return bk, bv, pk


def _check(fj, bk, bv, pk, device, fill=0):
    import torch
    m_exp, ek, ev, anti_exp = _np_outer(bk, bv, pk)
    if device:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
        args = (t(bk), t(bv), t(pk))
    else:
        args = (bk, bv, pk)
    host = lambda a: a.cpu().numpy().view(np.uint64) if hasattr(a, "cpu") else np.asarray(a).view(np.uint64)
    m, _, keys, vals = fj.left_join(*args, return_arrays=True, fill_value=fill)
    keys, vals = host(keys), host(vals)
    assert m == m_exp
    assert keys.size == pk.size and vals.size == pk.size
    assert np.array_equal(_sorted(keys), _sorted(pk))
    from oracle.oracle import canon_pairs
    a, b = canon_pairs(keys[:m], vals[:m]), canon_pairs(ek, ev)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "matched rows differ from np_join (first occurrence)"
    assert np.array_equal(_sorted(keys[m:]), _sorted(anti_exp))
    assert np.all(vals[m:] == np.uint64(fill))
    u, _, akeys = fj.anti_join(args[0], args[2], return_arrays=True)
    assert u == pk.size - m and np.array_equal(_sorted(host(akeys)), _sorted(anti_exp))
    uc, _ = fj.anti_join_count(args[0], args[2])
    assert uc == pk.size - m
    u2, _ = fj.anti_join(args[0], args[2])
    assert u2 == u


CASES = [   # id, nb, np, hit rate, plan_target_keys
    ("nb0", 0, 1000, 0.5, 4096),
    ("nb1", 1, 1000, 0.5, 4096),
    ("np0", 1000, 0, 0.5, 4096),
    ("zero_pass", 3000, 200_000, 0.5, 4096),
    ("zero_pass_all_hits", 3000, 100_000, 1.0, 4096),
    ("zero_pass_no_hits", 3000, 100_000, 0.0, 4096),
    ("one_pass", 200_000, 1_000_000, 0.5, 4096),
    ("one_pass_all_hits", 200_000, 500_000, 1.0, 4096),
    ("two_pass", 3_000_000, 4_000_000, 0.5, 4096),
    ("deep", 60_000, 400_000, 0.5, 32),
    ("deep_no_hits", 60_000, 200_000, 0.0, 32),
]


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("cid,nb,n_p,hit,target", CASES, ids=[c[0] for c in CASES])
def test_parity_with_the_numpy_reference(fj, cid, nb, n_p, hit, target, device):
    bk, bv, pk = _case(nb, n_p, hit, seed=zlib.crc32(cid.encode()) % 1000)
    fj.set_option("plan_target_keys", target)
    try:
        _check(fj, bk, bv, pk, device, fill=0 if cid != "one_pass" else 2**64 - 3)
        if cid == "zero_pass":
            _check(fj, bk, bv, pk, device, fill=12345)
        if target == 32 or cid == "two_pass":
            assert fj.last_timings()["path"] == 0 and fj.last_timings()["passes"] >= 2
    finally:
        fj.set_option("plan_target_keys", 4096)


@pytest.mark.gpu
def test_global_table_path_keeps_first_occurrence(fj):
    import torch
    from flash_hash_join_amd import api
    from oracle.oracle import canon_pairs
    bk, bv, pk = _case(50_000, 300_000, 0.6, seed=7)
    m_exp, ek, ev, anti_exp = _np_outer(bk, bv, pk)
    t = lambda a: torch.from_numpy(a.view(np.int64)).cuda()
    fj.set_option("scalar_hbm_table", 1)
    try:
        m, _, k, v = api.join_device(api.ALGO_SCALAR | api.ALGO_LEFT_OUTER, 0, 1, t(bk), t(bv), t(pk), return_arrays=True)
        assert fj.last_timings()["path"] == 1
        hbm_timings.check_hbm_form(fj.last_timings())
        k, v = k.cpu().numpy().view(np.uint64), v.cpu().numpy().view(np.uint64)
        assert m == m_exp
        a, b = canon_pairs(k[:m], v[:m]), canon_pairs(ek, ev)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(_sorted(k[m:]), _sorted(anti_exp)) and np.all(v[m:] == 0)
        u, _, ak, _ = api.join_device(api.ALGO_SCALAR | api.ALGO_ANTI, 0, 1, t(bk), None, t(pk), return_arrays=True)
        assert fj.last_timings()["path"] == 1
        hbm_timings.check_hbm_form(fj.last_timings())
        assert u == pk.size - m and np.array_equal(_sorted(ak.cpu().numpy()), _sorted(anti_exp))
        uc, _ = api.join_device(api.ALGO_SCALAR | api.ALGO_ANTI, 0, 0, t(bk), None, t(pk))
        assert uc == pk.size - m
    finally:
        fj.set_option("scalar_hbm_table", 0)
    fj.set_option("radix_threshold", 10**9)
    try:
        m, _, k, v = fj.left_join(bk, bv, pk, return_arrays=True, fill_value=5)
        assert fj.last_timings()["path"] == 1
        hbm_timings.check_hbm_form(fj.last_timings())
        a = canon_pairs(k[:m], v[:m])
        assert m == m_exp and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.all(v[m:] == 5)
    finally:
        fj.set_option("radix_threshold", 0)


@pytest.mark.gpu
def test_a_partition_beyond_the_lds_table_falls_back_to_the_global_table(fj):
    def hash_w1(k):                                                # fj_hash_w1 of csrc/fj_common.h
        lo = (k & np.uint64(0xFFFFFFFF)).astype(np.uint32); hi = (k >> np.uint64(32)).astype(np.uint32)
        with np.errstate(over="ignore"):
            x = (lo * np.uint32(0x9E3779B1)) ^ (hi * np.uint32(0x85EBCA77))
            x ^= x >> np.uint32(16); x *= np.uint32(0x85ebca6b)
            x ^= x >> np.uint32(13); x *= np.uint32(0xc2b2ae35)
            x ^= x >> np.uint32(16)
        return x
    cand = np.arange(1, 1_000_000, dtype=np.uint64)
    one = cand[(hash_w1(cand) >> np.uint32(27)) == 0][:20000]     # top 5 hash bits equal -> one of the plan's 32 partitions
    assert one.size == 20000
    rest = cand[(hash_w1(cand) >> np.uint32(27)) != 0][:3000]
    bk = np.concatenate([one, rest, one[:500]])
    bv = np.arange(bk.size, dtype=np.uint64) * np.uint64(3) + np.uint64(1)
    pk = np.concatenate([bk, cand[-60000:]])
    m_exp, ek, ev, anti_exp = _np_outer(bk, bv, pk)
    from oracle.oracle import canon_pairs
    m, _, k, v = fj.left_join(bk, bv, pk, return_arrays=True)
    assert fj.last_timings()["fell_back"] == 1
    hbm_timings.check_hbm_form(fj.last_timings())
    a, b = canon_pairs(k[:m], v[:m]), canon_pairs(ek, ev)
    assert m == m_exp and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(_sorted(k[m:]), _sorted(anti_exp))
    u, _, ak = fj.anti_join(bk, pk, return_arrays=True)
    assert fj.last_timings()["fell_back"] == 1
    hbm_timings.check_hbm_form(fj.last_timings())
    assert u == pk.size - m and np.array_equal(_sorted(ak), _sorted(anti_exp))


@pytest.mark.gpu
def test_a_left_join_drops_a_pending_result(fj):
    import torch
    from flash_hash_join_amd import _lib, api
    L = _lib.load()
    bk, bv, pk = _case(100_000, 400_000, 0.5, seed=11)
    t = lambda a: torch.from_numpy(a.view(np.int64)).cuda()
    dbk, dbv, dpk = t(bk), t(bv), t(pk)
    ctx = api.context(0)
    stream = torch.cuda.current_stream(0).cuda_stream
    cnt = ctypes.c_uint64(0)
    _lib.check(L.fj_join_device(ctx, api.ALGO_RADIX, 0, 1, dbk.data_ptr(), dbv.data_ptr(), bk.size, dpk.data_ptr(), pk.size, stream, 64,
                                ctypes.byref(cnt), None, None, 0, None))              # counted, pairs pending
    m, _ = fj.left_join(dbk, dbv, dpk)
    assert m == int(cnt.value)
    ok = torch.empty(max(1, m), dtype=torch.int64, device="cuda")
    ov = torch.empty(max(1, m), dtype=torch.int64, device="cuda")
    assert L.fj_emit_pairs(ctx, ok.data_ptr(), ov.data_ptr(), m, stream, None) != 0
    assert "no counted materialising join is pending" in _lib.last_error()
    n, _ = fj.hash_join_count_radix(dbk, dbv, dpk)
    assert n == _np_outer(bk, bv, pk)[0]


@pytest.mark.gpu
def test_large_case_checked_on_the_device(fj):
    import torch
    from flash_hash_join_amd import datagen
    nb, n_p = 50_000_000, 500_000_000
    bk, bv = datagen.build_device(nb, "cuda:0")
    pk, expected = datagen.probe_device(n_p, nb, "cuda:0", seed=3, hit_bp=5000)
    m, _, k, v = fj.left_join(bk, bv, pk, return_arrays=True)
    assert m == expected and 0.45 * n_p < m < 0.55 * n_p
    golden = -7046029254386353131                                      # 0x9E3779B97F4A7C15 as int64
    assert torch.equal(k[:m], (v[:m] + 1) * golden)                    # datagen: build_keys[i] = (i + 1) * M, build_vals[i] = i
    del v
    sb = torch.sort(bk).values
    misses = k[m:]
    pos = torch.searchsorted(sb, misses).clamp_(max=nb - 1)
    assert not bool((sb[pos] == misses).any()), "an unmatched row's key is in the build side"
    del k, misses, pos
    uc, _ = fj.anti_join_count(bk, pk)
    assert uc == n_p - m
    u, _ = fj.anti_join(bk, pk)
    assert u == n_p - m
    torch.cuda.empty_cache()
