"""Full outer join (FJ_ALGO_FULL_OUTER, csrc/fj_outer.hip) and the semi join: the C-ABI contract and argument checks that need no
GPU, and - on an MI355X - exact parity with the NumPy reference on every plan (zero, one, two passes, deep plans, partitions without
probe rows), the global-table path, the fallback of a partition beyond the LDS table, the fused join against the composition
left_join + anti_join with swapped roles, the pending-result rule and one large case checked on the device.

Reference (integers, compared exactly as sorted multisets per range): oracle.np_join (first occurrence of a duplicated build key wins)
for rows [0, m), pk[~np.isin(pk, bk)] for rows [m, np), (bk, bv)[~np.isin(bk, pk)] for rows [np, np + r)."""
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
FULL, ROW_IDS = 0x100, 0x80


def _np_full(bk, bv, pk):
    """(m, matched keys, matched values, unmatched probe keys, unmatched build keys, their values) of the NumPy reference."""
    from oracle.oracle import np_join
    bk, bv, pk = (np.asarray(x, dtype=np.uint64) for x in (bk, bv, pk))
    m, k, v = np_join(bk, bv, pk, return_arrays=True)
    rest = ~np.isin(bk, pk)
    return m, k, v, pk[~np.isin(pk, bk)], bk[rest], bv[rest]


def _sorted(a):
    return np.sort(np.asarray(a).reshape(-1).view(np.uint64))


def _same_pairs(k1, v1, k2, v2):
    from oracle.oracle import canon_pairs
    a, b = canon_pairs(np.asarray(k1).view(np.uint64), np.asarray(v1).view(np.uint64)), canon_pairs(k2, v2)
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_header_flag_and_python_mirror():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    assert int(re.search(r"#define FJ_ALGO_FULL_OUTER (0x[0-9a-fA-F]+)", hdr).group(1), 16) == 0x100
    from flash_hash_join_amd import api
    assert api.ALGO_FULL_OUTER == 0x100


def test_flash_join_exposes_the_new_functions():
    import flash_join
    for name in ("full_join", "semi_join", "semi_join_count"):
        assert callable(getattr(flash_join, name)), name
    from flash_hash_join_amd import api
    assert {"full_join", "semi_join", "semi_join_count"} <= set(api.EXTENSIONS)


REFUSALS = [   # id, algo, materialize, capacity short by, misalignment, build values, output values, needle
    ("full_left", FULL | 0x20, 1, 0, 0, 0x20000, 0x50000, "cannot be combined"),
    ("full_anti", FULL | 0x40 | 2, 1, 0, 0, 0x20000, 0x50000, "cannot be combined"),
    ("full_many", FULL | 0x10, 1, 0, 0, 0x20000, 0x50000, "MANY_TO_MANY"),
    ("full_count", FULL, 0, 0, 0, 0x20000, 0x50000, "needs materialize = 1"),
    ("full_rid_count", FULL | ROW_IDS, 0, 0, 0, 0x20000, 0x50000, "needs materialize = 1"),
    ("capacity", FULL | 2, 1, 1, 0, 0x20000, 0x50000, "output capacity"),
    ("capacity_np_only", FULL | 1, 1, 100, 0, 0x20000, 0x50000, "output capacity"),
    ("misaligned", FULL, 1, 0, 4, 0x20000, 0x50000, "8-byte aligned"),
    ("null_out_vals", FULL, 1, 0, 0, 0x20000, None, "output buffers"),
    ("null_build_vals", FULL, 1, 0, 0, None, 0x50000, "d_build_vals"),
]


@pytest.mark.parametrize("cid,algo,materialize,cap_less,misalign,bv,ov,needle", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_invalid_combinations_are_refused_before_any_device_work(cid, algo, materialize, cap_less, misalign, bv, ov, needle):
    """A NULL context: the checks come before the context is touched (no GPU needed; the pointers are never dereferenced)."""
    from flash_hash_join_amd import _lib
    L = _lib.load()
    nb, n_p = 100, 1000
    cnt = (ctypes.c_uint64 * 2)(0, 0)
    rc = L.fj_join_device(None, algo, 0, materialize, 0x10000, bv, nb, 0x30000, n_p, None, 64, cnt,
                          0x40000 + misalign, ov, n_p + nb - cap_less, None)
    assert rc != 0
    err = _lib.last_error()
    assert needle in err and "null context" not in err, err


def test_row_ids_need_no_build_values_and_valid_arguments_reach_the_context():
    from flash_hash_join_amd import _lib
    L = _lib.load()
    cnt = (ctypes.c_uint64 * 2)(0, 0)
    for algo, bv in ((FULL | ROW_IDS, None), (FULL, 0x20000), (FULL | 2, 0x20000)):
        assert L.fj_join_device(None, algo, 0, 1, 0x10000, bv, 10, 0x30000, 10, None, 64, cnt, 0x40000, 0x50000, 20, None) != 0
        assert "null context" in _lib.last_error()


@pytest.mark.parametrize("algo,materialize,bv,needle", [
    (FULL | 0x20, 1, True, "cannot be combined"),
    (FULL | 0x40, 1, True, "cannot be combined"),
    (FULL | 0x10, 1, True, "MANY_TO_MANY"),
    (FULL, 0, True, "needs materialize = 1"),
    (FULL, 1, False, "build values"),
    (9, 1, True, "unknown algo"),
    (FULL | 9, 1, True, "unknown algo"),
    (0x200, 1, True, "unknown algo"),
], ids=["full_left", "full_anti", "full_many", "full_count", "no_build_values", "algo9", "full_algo9", "next_bit"])
def test_host_entry_refusals(algo, materialize, bv, needle):
    from flash_hash_join_amd import _lib
    L = _lib.load()
    a = np.arange(16, dtype=np.uint64)
    cnt = (ctypes.c_uint64 * 2)(0, 0)
    sec = ctypes.c_double(0)
    rc = L.fj_join_host(algo, 0, materialize, a.ctypes.data, a.ctypes.data if bv else None, a.size, a.ctypes.data, a.size,
                        cnt, ctypes.byref(sec), None, None)
    assert rc != 0 and needle in _lib.last_error(), _lib.last_error()


def test_join_indices_argument_errors():
    import flash_join
    a = np.arange(4, dtype=np.uint64)
    for kw in (dict(how="full", many_to_many=True), dict(how="semi", many_to_many=True), dict(how="outer")):
        with pytest.raises(ValueError):
            flash_join.join_indices(a, a, **kw)


def test_numpy_reference_on_a_hand_written_case():
    # 7: duplicated and matched; 8: duplicated and unmatched; 0 and 2**64 - 1 on both sides; 9 and 6: build only
    bk = np.array([5, 7, 7, 9, 2**64 - 1, 0, 8, 8, 6], dtype=np.uint64)
    bv = np.array([50, 70, 71, 90, 11, 1, 80, 81, 60], dtype=np.uint64)
    pk = np.array([7, 3, 5, 7, 2**64 - 1, 4, 0, 3], dtype=np.uint64)
    m, k, v, anti, rk, rv = _np_full(bk, bv, pk)
    assert m == 5
    assert sorted(zip(k.tolist(), v.tolist())) == [(0, 1), (5, 50), (7, 70), (7, 70), (2**64 - 1, 11)]
    assert sorted(anti.tolist()) == [3, 3, 4]
    assert sorted(zip(rk.tolist(), rv.tolist())) == [(6, 60), (8, 80), (8, 81), (9, 90)]          # every copy of key 8
    # keys 0 and 2**64 - 1 on the build side only: they move to the third range
    m2, _, _, _, rk2, rv2 = _np_full(bk, bv, pk[(pk != 0) & (pk != U64_MAX)])
    assert m2 == 3 and sorted(zip(rk2.tolist(), rv2.tolist()))[:1] == [(0, 1)] and (2**64 - 1, 11) in set(zip(rk2.tolist(), rv2.tolist()))


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fj():
    import flash_join
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_device_count() >= 1, "no HIP device: the product path must not silently fall back"
    assert flash_join.initialize() is None
    return flash_join


def _case(nb, n_p, hit, seed, probed=0.7):
    """test_outer_join._case, extended: hits are drawn from the first `probed` share of the build rows only, so that some build
    keys are never probed; one duplicated key lies in the probed share (and is probed for certain), one outside it."""
    rng = np.random.default_rng(seed)
    bk = rng.integers(0, 2**64, size=nb, dtype=np.uint64)
    npr = max(1, int(nb * probed)) if nb else 0
    if nb >= 40:
        bk[0], bk[1] = 0, U64_MAX                                         # raw zero and raw 2^64 - 1 (the HBM table's empty marker), probed
        bk[2], bk[3] = keymix.EMPTY_RAW, keymix.FILLER_RAW                # the LDS tables' empty marker and the wide kernel's filler, probed
        bk[nb - 1], bk[nb - 2] = 1, U64_MAX - np.uint64(1)                # their neighbours, never probed
        d = max(1, nb // 20)
        bk[npr - d:npr] = bk[4:4 + d]                                     # duplicated build keys inside the probed share
        bk[nb - 2 - d:nb - 2] = bk[npr:npr + d]                           # ... and outside it: every copy is unmatched
    bv = rng.integers(0, 2**64, size=nb, dtype=np.uint64)
    nhit = int(n_p * hit) if nb else 0
    parts = [rng.choice(bk[:npr], nhit)] if nhit else []
    parts.append(rng.integers(1, 2**63, size=n_p - nhit, dtype=np.uint64) * np.uint64(2) + np.uint64(2**63))   # ~never a build key
    pk = np.concatenate(parts)[:n_p]
    if n_p >= 16 and 0.0 < hit < 1.0:
        pk[:2] = np.array([0, 2**64 - 1], dtype=np.uint64)                # ... on the probe side too
        pk[3:5] = np.array([keymix.EMPTY_RAW, keymix.FILLER_RAW], dtype=np.uint64)
        if nb >= 40:
            pk[2] = bk[4]                                                 # a duplicated key is matched for certain
    rng.shuffle(pk)
    return bk, bv, pk


def _host(a):
    return a.cpu().numpy().view(np.uint64) if hasattr(a, "cpu") else np.asarray(a).view(np.uint64)


def _check(fj, bk, bv, pk, device, fill=0):
    import torch
    m_exp, ek, ev, anti_exp, rk_exp, rv_exp = _np_full(bk, bv, pk)
    n_p = pk.size
    if device:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
        args = (t(bk), t(bv), t(pk))
    else:
        args = (bk, bv, pk)
    # ---- key / value form ----
    m, r, _, keys, vals = fj.full_join(*args, return_arrays=True, fill_value=fill)
    keys, vals = _host(keys), _host(vals)
    print(f"full_join: m={m} (expected {m_exp}) r={r} (expected {rk_exp.size}) rows={keys.size}")
    assert (m, r) == (m_exp, rk_exp.size)
    assert keys.size == n_p + r and vals.size == n_p + r
    assert _same_pairs(keys[:m], vals[:m], ek, ev), "matched rows differ from np_join (first occurrence)"
    assert np.array_equal(_sorted(keys[m:n_p]), _sorted(anti_exp)) and np.all(vals[m:n_p] == np.uint64(fill))
    assert _same_pairs(keys[n_p:], vals[n_p:], rk_exp, rv_exp), "unmatched build rows differ from (bk, bv)[~isin(bk, pk)]"
    assert fj.full_join(*args)[:2] == (m, r)
    # ---- row-id form ----
    m2, r2, _, pi, bi = fj.join_indices(args[0], args[2], how="full")
    pi, bi = _host(pi).view(np.int64), _host(bi).view(np.int64)
    assert (m2, r2) == (m_exp, rk_exp.size) and pi.size == n_p + r and bi.size == n_p + r
    assert np.array_equal(np.sort(pi[:n_p]), np.arange(n_p)), "probe_idx over ranges one and two is not a permutation"
    assert np.array_equal(pk[pi[:m]], bk[bi[:m]])
    if m:
        uniq, first = np.unique(bk, return_index=True)              # (the index of every key's first occurrence)
        assert np.array_equal(bi[:m], first[np.searchsorted(uniq, pk[pi[:m]])]), "not the smallest build index"
    assert np.all(bi[m:n_p] == -1) and np.all(~np.isin(pk[pi[m:n_p]], bk))
    assert np.all(pi[n_p:] == -1)
    assert np.array_equal(np.sort(bi[n_p:]), np.flatnonzero(~np.isin(bk, pk)))


CASES = [   # id, nb, np, hit rate, plan_target_keys
    ("nb0", 0, 1000, 0.5, 4096),
    ("nb1", 1, 1000, 0.5, 4096),
    ("np0", 1000, 0, 0.5, 4096),
    ("both0", 0, 0, 0.5, 4096),
    ("zero_pass", 3000, 200_000, 0.5, 4096),
    ("zero_pass_all_hits", 3000, 100_000, 1.0, 4096),
    ("zero_pass_no_hits", 3000, 100_000, 0.0, 4096),
    ("one_pass", 200_000, 1_000_000, 0.5, 4096),
    ("one_pass_all_hits", 200_000, 500_000, 1.0, 4096),
    ("two_pass", 3_000_000, 4_000_000, 0.5, 4096),
    ("deep", 60_000, 400_000, 0.5, 32),
    ("deep_no_hits", 60_000, 200_000, 0.0, 32),
    ("nb_gt_np", 1_000_000, 100_000, 0.5, 4096),
    ("empty_partitions", 3_000_000, 300, 0.5, 4096),        # a two-pass plan's ~1000 partitions, most without a probe row
]


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("cid,nb,n_p,hit,target", CASES, ids=[c[0] for c in CASES])
def test_parity_with_the_numpy_reference(fj, cid, nb, n_p, hit, target, device):
    bk, bv, pk = _case(nb, n_p, hit, seed=zlib.crc32(cid.encode()) % 1000)
    fj.set_option("plan_target_keys", target)
    try:
        _check(fj, bk, bv, pk, device, fill=0 if cid != "one_pass" else 2**64 - 3)
        if target == 32 or cid in ("two_pass", "empty_partitions"):
            assert fj.last_timings()["path"] == 0 and fj.last_timings()["passes"] >= 2
    finally:
        fj.set_option("plan_target_keys", 4096)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_unique_build_keys_take_the_single_launch(fj, device):
    """No duplicate on the build side: the values travel with the keys, no second launch with row indices."""
    rng = np.random.default_rng(5)
    bk = np.unique(rng.integers(0, 2**64, size=300_000, dtype=np.uint64))
    rng.shuffle(bk)
    bv = rng.integers(0, 2**64, size=bk.size, dtype=np.uint64)
    pk = np.concatenate([rng.choice(bk[:bk.size // 2], 600_000), rng.integers(0, 2**64, size=600_000, dtype=np.uint64)])
    _check(fj, bk, bv, pk, device)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["scalar_hbm_table", "radix_threshold"])
def test_global_table_path(fj, how):
    bk, bv, pk = _case(50_000, 300_000, 0.6, seed=7)
    from flash_hash_join_amd import api
    import torch
    if how == "scalar_hbm_table":
        m_exp, ek, ev, anti_exp, rk_exp, rv_exp = _np_full(bk, bv, pk)
        t = lambda a: torch.from_numpy(a.view(np.int64)).cuda()
        fj.set_option("scalar_hbm_table", 1)
        try:
            for dev in (True, False):
                a = (t(bk), t(bv), t(pk)) if dev else (bk, bv, pk)
                (m, r), _, k, v = api._join(api.ALGO_SCALAR | api.ALGO_FULL_OUTER, 0, 1, *a, True)
                assert fj.last_timings()["path"] == 1
                hbm_timings.check_hbm_form(fj.last_timings())
                k, v = _host(k), _host(v)
                assert (m, r) == (m_exp, rk_exp.size) and k.size == pk.size + r
                assert _same_pairs(k[:m], v[:m], ek, ev)
                assert np.array_equal(_sorted(k[m:pk.size]), _sorted(anti_exp)) and np.all(v[m:pk.size] == 0)
                assert _same_pairs(k[pk.size:], v[pk.size:], rk_exp, rv_exp)
                (m, r), _, pi, bi = api._join(api.ALGO_SCALAR | api.ALGO_FULL_OUTER | api.ALGO_ROW_IDS, 0, 1, a[0], None, a[2], True)
                assert fj.last_timings()["path"] == 1
                hbm_timings.check_hbm_form(fj.last_timings())
                pi, bi = _host(pi).view(np.int64), _host(bi).view(np.int64)
                assert (m, r) == (m_exp, rk_exp.size)
                assert np.array_equal(np.sort(pi[:pk.size]), np.arange(pk.size)) and np.array_equal(pk[pi[:m]], bk[bi[:m]])
                assert np.all(bi[m:pk.size] == -1) and np.all(pi[pk.size:] == -1)
                assert np.array_equal(np.sort(bi[pk.size:]), np.flatnonzero(~np.isin(bk, pk)))
        finally:
            fj.set_option("scalar_hbm_table", 0)
    else:
        fj.set_option("radix_threshold", 10**9)
        try:
            for dev in (False, True):
                _check(fj, bk, bv, pk, dev, fill=5)
                assert fj.last_timings()["path"] == 1
                hbm_timings.check_hbm_form(fj.last_timings())
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
    pk = np.concatenate([bk[::2], cand[-60000:]])                 # every second build row probed
    m_exp, ek, ev, anti_exp, rk_exp, rv_exp = _np_full(bk, bv, pk)
    assert rk_exp.size > 0
    m, r, _, k, v = fj.full_join(bk, bv, pk, return_arrays=True)
    assert fj.last_timings()["fell_back"] == 1
    hbm_timings.check_hbm_form(fj.last_timings())
    assert (m, r) == (m_exp, rk_exp.size)
    assert _same_pairs(k[:m], v[:m], ek, ev)
    assert np.array_equal(_sorted(k[m:pk.size]), _sorted(anti_exp))
    assert _same_pairs(k[pk.size:], v[pk.size:], rk_exp, rv_exp)
    m, r, _, pi, bi = fj.join_indices(bk, pk, how="full")
    assert fj.last_timings()["fell_back"] == 1
    hbm_timings.check_hbm_form(fj.last_timings())
    assert (m, r) == (m_exp, rk_exp.size) and np.array_equal(np.sort(bi[pk.size:]), np.flatnonzero(~np.isin(bk, pk)))
    assert np.array_equal(pk[pi[:m]], bk[bi[:m]]) and np.all(pi[pk.size:] == -1)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_the_fused_join_equals_the_composition(fj, device):
    """rows [0, np) = left_join of the same inputs, rows [np, np + r) = anti_join with the roles swapped."""
    import torch
    bk, bv, pk = _case(400_000, 2_000_000, 0.5, seed=21)
    if device:
        t = lambda a: torch.from_numpy(a.view(np.int64)).cuda()
        bk_, bv_, pk_ = t(bk), t(bv), t(pk)
    else:
        bk_, bv_, pk_ = bk, bv, pk
    m, r, _, k, v = fj.full_join(bk_, bv_, pk_, return_arrays=True)
    lm, _, lk, lv = fj.left_join(bk_, bv_, pk_, return_arrays=True)
    u, _, ak = fj.anti_join(pk_, bk_, return_arrays=True)
    k, v, lk, lv, ak = (_host(x) for x in (k, v, lk, lv, ak))
    assert m == lm and r == u and r > 0
    assert _same_pairs(k[:m], v[:m], lk[:m], lv[:m])
    assert _same_pairs(k[m:pk.size], v[m:pk.size], lk[m:], lv[m:])
    assert np.array_equal(_sorted(k[pk.size:]), _sorted(ak))


@pytest.mark.gpu
def test_a_full_join_drops_a_pending_result(fj):
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
    m, r, _ = fj.full_join(dbk, dbv, dpk)
    assert m == int(cnt.value) and r == int((~np.isin(bk, pk)).sum())
    ok = torch.empty(max(1, m), dtype=torch.int64, device="cuda")
    ov = torch.empty(max(1, m), dtype=torch.int64, device="cuda")
    assert L.fj_emit_pairs(ctx, ok.data_ptr(), ov.data_ptr(), m, stream, None) != 0
    assert "no counted materialising join is pending" in _lib.last_error()
    n, _ = fj.hash_join_count_radix(dbk, dbv, dpk)
    assert n == _np_full(bk, bv, pk)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("nb,n_p", [(0, 1000), (1000, 0), (3000, 100_000), (200_000, 1_000_000)], ids=["nb0", "np0", "zero_pass", "one_pass"])
def test_semi_join(fj, nb, n_p, device):
    import torch
    bk, bv, pk = _case(nb, n_p, 0.5, seed=nb % 97)
    exp = pk[np.isin(pk, bk)]
    if device:
        t = lambda a: torch.from_numpy(a.view(np.int64)).cuda()
        bk_, bv_, pk_ = t(bk), t(bv), t(pk)
    else:
        bk_, bv_, pk_ = bk, bv, pk
    s, _, keys = fj.semi_join(bk_, pk_, return_arrays=True)
    assert s == exp.size and np.array_equal(_sorted(_host(keys)), _sorted(exp))
    assert fj.semi_join(bk_, pk_)[0] == s and fj.semi_join_count(bk_, pk_)[0] == s
    assert fj.hash_join_count_radix(bk_, bv_, pk_)[0] == s
    s2, _, pi, none = fj.join_indices(bk_, pk_, how="semi")
    pi = _host(pi).view(np.int64)
    assert s2 == s and none is None and np.array_equal(np.sort(pi), np.flatnonzero(np.isin(pk, bk)))


@pytest.mark.gpu
def test_large_case_checked_on_the_device(fj):
    """50M x 500M, half the probe rows hitting.  Build ids 1..30M and 10^9+1..10^9+20M (datagen: key = id * M, value = id - 1); the probe
    side draws its hits from ids 1..30M and its misses from 30M+1..60M, so the 20M high build rows are unmatched for certain and of the
    low ones exactly those that no hit drew: r = nb - (distinct build rows among the matched values), counted with a mask."""
    import torch
    from flash_hash_join_amd import datagen
    lo, hi, n_p = 30_000_000, 20_000_000, 500_000_000
    nb = lo + hi
    k1, v1 = datagen.build_device(lo, "cuda:0")
    k2, v2 = datagen.build_device(hi, "cuda:0", first=10**9)
    bk, bv = torch.cat([k1, k2]), torch.cat([v1, v2])
    del k1, k2, v1, v2
    pk, expected = datagen.probe_device(n_p, lo, "cuda:0", seed=3, hit_bp=5000)
    m, r, _, k, v = fj.full_join(bk, bv, pk, return_arrays=True)
    print(f"large case: m={m} r={r} timings={fj.last_timings()}")
    assert m == expected and 0.45 * n_p < m < 0.55 * n_p
    assert k.numel() == n_p + r and hi <= r < nb
    golden = -7046029254386353131                                      # 0x9E3779B97F4A7C15 as int64
    assert torch.equal(k[:m], (v[:m] + 1) * golden)                    # matched: the build row of that key
    assert torch.equal(k[n_p:], (v[n_p:] + 1) * golden)                # third range: build rows as they are
    assert not bool(v[m:n_p].any())
    seen = torch.zeros(lo, dtype=torch.bool, device="cuda")
    seen[v[:m]] = True                                                 # matched values are build ids - 1 < lo
    distinct = int(seen.sum())
    assert r == nb - distinct
    v3 = v[n_p:]
    low = v3[v3 < lo]
    assert int((v3 >= 10**9).sum()) == hi and not bool(seen[low].any())   # every high row, and no low row that was matched
    assert torch.unique(v3).numel() == r                                # every build row at most once
    del seen, low, v3, v
    sb = torch.sort(bk).values
    misses = k[m:n_p]
    pos = torch.searchsorted(sb, misses).clamp_(max=nb - 1)
    assert not bool((sb[pos] == misses).any()), "an unmatched probe row's key is in the build side"
    del k, misses, pos, sb
    m2, r2, _ = fj.full_join(bk, bv, pk)
    assert (m2, r2) == (m, r)
    torch.cuda.empty_cache()
