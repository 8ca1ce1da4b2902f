"""Row-index gather maps (FJ_ALGO_ROW_IDS, api.join_indices): the C-ABI contract and argument checks that need no GPU, and - on an
MI355X - exact parity of the (probe row, build row) pair sets with a NumPy reference on every plan: empty sides, zero, one and two
passes, deep plans, the skew re-partition, the HBM-table fallback, scalar_hbm_table, the two-phase (count, then emit) path, and one
large case checked on the device.

Reference: a stable argsort of the build keys, then searchsorted of the probe keys - the smallest build row per key (first
occurrence); many-to-many expands every equal key."""
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


def ref_indices(bk, pk, how="inner", many=False):
    """(probe_idx, build_idx) of the NumPy reference as int64; left: unmatched rows carry build_idx -1; anti: build_idx None."""
    bk, pk = np.asarray(bk, dtype=np.uint64), np.asarray(pk, dtype=np.uint64)
    order = np.argsort(bk, kind="stable")
    sb = bk[order]
    lo, hi = np.searchsorted(sb, pk, "left"), np.searchsorted(sb, pk, "right")
    cnt = hi - lo
    hit = cnt > 0
    if how == "anti":
        return np.nonzero(~hit)[0].astype(np.int64), None
    if many:
        pi = np.repeat(np.arange(pk.size, dtype=np.int64), cnt)
        start = np.repeat(lo, cnt)
        within = np.arange(pi.size, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        return pi, order[start + within].astype(np.int64)
    pi = np.nonzero(hit)[0].astype(np.int64)
    bi = order[lo[hit]].astype(np.int64)
    if how == "left":
        miss = np.nonzero(~hit)[0].astype(np.int64)
        return np.concatenate([pi, miss]), np.concatenate([bi, np.full(miss.size, -1, np.int64)])
    return pi, bi


def _pairs(pi, bi):
    pi = np.asarray(pi, dtype=np.int64).reshape(-1)
    bi = np.full(pi.size, -1, np.int64) if bi is None else np.asarray(bi, dtype=np.int64).reshape(-1)
    o = np.lexsort((bi, pi))
    return pi[o], bi[o]


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_header_flag_and_python_mirror():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    assert int(re.search(r"#define FJ_ALGO_ROW_IDS (0x[0-9a-fA-F]+)", hdr).group(1), 16) == 0x80
    from flash_hash_join_amd import api
    assert api.ALGO_ROW_IDS == 0x80


def test_flash_join_exposes_join_indices():
    import flash_join
    from flash_hash_join_amd import api
    assert callable(flash_join.join_indices)
    assert "join_indices" in api.EXTENSIONS


@pytest.mark.parametrize("algo,materialize,cap_less,needle", [
    (0x80, 0, 0, "needs materialize = 1"),
    (0x80 | 0x40, 0, 0, "needs materialize = 1"),
    (0x80 | 0x20 | 0x10, 1, 0, "MANY_TO_MANY"),
    (0x80 | 0x40 | 0x10, 1, 0, "MANY_TO_MANY"),
    (0x80 | 0x20, 1, 1, "output capacity"),
    (0x80 | 0x40, 1, 1, "output capacity"),
], ids=["count", "anti_count", "left_many", "anti_many", "left_capacity", "anti_capacity"])
def test_invalid_combinations_are_refused_before_any_device_work(algo, materialize, cap_less, needle):
    """A NULL context: the checks come before the context is touched (no GPU needed; the pointers are never dereferenced)."""
    from flash_hash_join_amd import _lib
    L = _lib.load()
    nb, n_p = 100, 1000
    cnt = ctypes.c_uint64(0)
    rc = L.fj_join_device(None, algo, 0, materialize, 0x10000, 0x20000, nb, 0x30000, n_p, None, 64, ctypes.byref(cnt),
                          0x40000, 0x50000, n_p - cap_less, None)
    assert rc != 0
    err = _lib.last_error()
    assert needle in err and "null context" not in err, err


@pytest.mark.parametrize("algo", [0x80, 0x80 | 0x10, 0x80 | 0x20 | 2, 0x80 | 0x40 | 1], ids=["inner", "many", "left", "anti"])
def test_null_build_values_are_accepted(algo):
    from flash_hash_join_amd import _lib
    L = _lib.load()
    cnt = ctypes.c_uint64(0)
    assert L.fj_join_device(None, algo, 0, 1, 0x10000, None, 10, 0x30000, 10, None, 64, ctypes.byref(cnt), 0x40000, 0x50000, 10, None) != 0
    assert "null context" in _lib.last_error()


def test_host_entry_refuses_a_counting_row_id_join():
    from flash_hash_join_amd import _lib
    L = _lib.load()
    cnt, sec = ctypes.c_uint64(0), ctypes.c_double(0)
    bk = np.arange(4, dtype=np.uint64)
    assert L.fj_join_host(0x80, 0, 0, bk.ctypes.data, None, 4, bk.ctypes.data, 4, ctypes.byref(cnt), ctypes.byref(sec), None, None) != 0
    assert "needs materialize = 1" in _lib.last_error()


@pytest.mark.parametrize("kw", [dict(how="bogus"), dict(how="left", many_to_many=True), dict(how="anti", many_to_many=True)])
def test_join_indices_argument_errors(kw):
    from flash_hash_join_amd import api
    with pytest.raises(ValueError):
        api.join_indices(np.arange(3, dtype=np.uint64), np.arange(3, dtype=np.uint64), **kw)


def test_numpy_reference_on_a_hand_written_case():
    bk = np.array([5, 7, 7, 9, 2**64 - 1, 0, 2**64 - 1], dtype=np.uint64)
    pk = np.array([7, 3, 5, 7, 2**64 - 1, 4, 0, 3], dtype=np.uint64)
    pi, bi = ref_indices(bk, pk)
    assert list(zip(pi.tolist(), bi.tolist())) == [(0, 1), (2, 0), (3, 1), (4, 4), (6, 5)]     # key 7 -> row 1, 2^64-1 -> row 4
    pi, bi = ref_indices(bk, pk, many=True)
    assert sorted(zip(pi.tolist(), bi.tolist())) == [(0, 1), (0, 2), (2, 0), (3, 1), (3, 2), (4, 4), (4, 6), (6, 5)]
    pi, bi = ref_indices(bk, pk, "left")
    assert sorted(zip(pi.tolist(), bi.tolist())) == [(0, 1), (1, -1), (2, 0), (3, 1), (4, 4), (5, -1), (6, 5), (7, -1)]
    pi, bi = ref_indices(bk, pk, "anti")
    assert pi.tolist() == [1, 5, 7] and bi is None


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
        bk[nb - d:] = bk[4:4 + d]                                         # duplicated build keys
    nhit = int(n_p * hit) if nb else 0
    parts = [rng.choice(bk, nhit)] if nhit else []
    parts.append(rng.integers(1, 2**63, size=n_p - nhit, dtype=np.uint64) * np.uint64(2) + np.uint64(2**63))   # ~never a build key
    pk = np.concatenate(parts)[:n_p] if parts else np.empty(0, np.uint64)
    if n_p >= 16 and 0.0 < hit < 1.0:
        pk[:4] = np.array([0, 2**64 - 1, keymix.EMPTY_RAW, keymix.FILLER_RAW], dtype=np.uint64)   # ... on the probe side too
    rng.shuffle(pk)
    return bk, pk


def _host(a):
    if a is None:
        return None
    if hasattr(a, "cpu"):
        assert str(a.dtype) == "torch.int64"
        return a.cpu().numpy()
    assert a.dtype == np.int64
    return a


def _check_mode(fj, bk, pk, device, how, many=False):
    import torch
    args = (bk, pk)
    if device:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
        args = (t(bk), t(pk))
    n, sec, pi, bi = fj.join_indices(*args, how=how, many_to_many=many)
    lt = fj.last_timings()                                             # (of this call: the checks below run no join)
    assert isinstance(n, int) and isinstance(sec, float)
    if device:
        assert pi.is_cuda and (bi is None or bi.is_cuda)
    pi, bi = _host(pi), _host(bi)
    epi, ebi = ref_indices(bk, pk, how, many)
    if how == "anti":
        assert bi is None and n == epi.size == pi.size
        assert np.array_equal(np.sort(pi), epi)
        return lt
    if how == "left":
        m = int((ebi >= 0).sum())
        assert n == m and pi.size == bi.size == pk.size
        assert np.all(bi[:m] >= 0) and np.all(bi[m:] == -1)
    else:
        assert n == epi.size == pi.size == bi.size
    a, b = _pairs(pi, bi), _pairs(epi, ebi)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), f"{how} many={many}: pair sets differ from the reference"
    return lt


def _check_all(fj, bk, pk, device, many=True, passes=None):
    """every mode; passes(many) -> predicate on the plan's pass count, checked after each mode's own call"""
    modes = [("inner", False), ("left", False), ("anti", False)] + ([("inner", True)] if many else [])
    for how, mm in modes:
        lt = _check_mode(fj, bk, pk, device, how, many=mm)
        if passes is not None:
            assert lt["path"] == 0 and passes(mm)(lt["passes"]), (how, mm, lt)


CASES = [   # id, nb, np, hit rate, plan_target_keys
    ("nb0", 0, 1000, 0.5, 4096),
    ("nb1", 1, 1000, 0.5, 4096),
    ("np0", 1000, 0, 0.5, 4096),
    ("zero_pass", 3000, 200_000, 0.5, 4096),
    ("one_pass", 200_000, 1_000_000, 0.5, 4096),
    ("two_pass", 3_000_000, 4_000_000, 0.5, 4096),
    ("deep", 60_000, 400_000, 0.5, 32),
]


# the plan's pass count per case: (N:1 modes, many-to-many); the many-to-many plan aims at 2048 build rows per partition, so its
# 3000-row "zero-pass" case takes one pass
PASSES = {
    "zero_pass": (lambda p: p == 0, lambda p: p == 1),
    "one_pass": (lambda p: p == 1, lambda p: p == 1),
    "two_pass": (lambda p: p == 2, lambda p: p == 2),
    "deep": (lambda p: p >= 2, lambda p: p >= 2),
}


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("cid,nb,n_p,hit,target", CASES, ids=[c[0] for c in CASES])
def test_parity_with_the_numpy_reference(fj, cid, nb, n_p, hit, target, device):
    bk, pk = _case(nb, n_p, hit, seed=zlib.crc32(cid.encode()) % 1000)
    fj.set_option("plan_target_keys", target)
    try:
        want = PASSES.get(cid)
        _check_all(fj, bk, pk, device, passes=(lambda mm: want[1 if mm else 0]) if want else None)
    finally:
        fj.set_option("plan_target_keys", 4096)


@pytest.mark.gpu
@pytest.mark.parametrize("unique", [True, False], ids=["unique_build_keys", "duplicate_build_keys"])
@pytest.mark.parametrize("single", [1, 0], ids=["single_pass", "count_then_emit"])
@pytest.mark.parametrize("hooks", [0, 64], ids=["plain", "emit_retry_every_7th"])
def test_persistent_emit_kernel(fj, unique, single, hooks):
    """The resident-workgroup emit kernel's row-id forms (persistent_min_items = 1 puts every plan with chunk lists on them): the
    single-pass form with unique build keys - duplicates send it to count-then-emit with the first-occurrence form - and the
    two-pass form; lab hook 64 sends every 7th item down the tagged kernel's retry path."""
    bk, pk = _case(200_000, 1_000_000, 0.5, seed=31)
    if unique:
        bk = np.unique(bk)
        np.random.default_rng(2).shuffle(bk)
    prev = fj.get_option("persistent_min_items")
    fj.set_option("persistent_min_items", 1)
    fj.set_option("mat_single_pass", single)
    fj.set_option("lab_hooks", hooks)
    try:
        for device in (False, True):
            lt = _check_mode(fj, bk, pk, device, "inner")
            assert lt["passes"] == 1 and lt["fell_back"] == 0, lt
            if hooks:
                assert lt["lds_retries"] >= 1, lt
            elif single and unique and device:
                assert lt["emit_ms"] == 0.0, lt                       # one pass over the probe side: no separate emitting pass
            else:
                assert lt["emit_ms"] > 0.0, lt
    finally:
        fj.set_option("persistent_min_items", prev)
        fj.set_option("mat_single_pass", 1)
        fj.set_option("lab_hooks", 0)


def _hash_w1(k):                                                   # fj_hash_w1 of csrc/fj_common.h
    lo = (k & np.uint64(0xFFFFFFFF)).astype(np.uint32); hi = (k >> np.uint64(32)).astype(np.uint32)
    with np.errstate(over="ignore"):
        x = (lo * np.uint32(0x9E3779B1)) ^ (hi * np.uint32(0x85EBCA77))
        x ^= x >> np.uint32(16); x *= np.uint32(0x85ebca6b)
        x ^= x >> np.uint32(13); x *= np.uint32(0xc2b2ae35)
        x ^= x >> np.uint32(16)
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_a_skewed_partition_is_re_partitioned(fj, device):
    """9000 build keys in one of the plan's 32 partitions (beyond the tagged LDS table): the inner join re-partitions that
    partition alone (lds_retries >= 2), duplicates of its keys keep their first occurrence."""
    cand = np.arange(1, 400000, dtype=np.uint64)
    skew = cand[(_hash_w1(cand) >> np.uint32(27)) == 0][:9000]
    assert skew.size == 9000
    bk = np.concatenate([skew, skew[:300]])
    pk = np.concatenate([bk, cand[:50000]])
    _check_mode(fj, bk, pk, device, "inner")
    lt = fj.last_timings()
    assert lt["fell_back"] == 0 and lt["lds_retries"] >= 2, lt
    _check_mode(fj, bk, pk, device, "left")
    _check_mode(fj, bk, pk, device, "anti")


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_partitions_beyond_the_lds_tables_fall_back_to_the_hbm_table(fj, device):
    """140 of the plan's 512 partitions hold 8500 distinct build keys each - beyond the LDS tables and too many to re-partition
    one by one: the whole join runs again on the HBM table (fell_back == 1), still with first-occurrence build rows."""
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
    bk = np.concatenate([one, one[:2000]])
    pk = np.concatenate([bk[::3], cand[-200000:]])
    for how in ("inner", "left", "anti"):
        _check_mode(fj, bk, pk, device, how)
        if how != "anti":                                              # (the anti join's keys-only table takes 15360 keys)
            assert fj.last_timings()["fell_back"] == 1, (how, fj.last_timings())
            hbm_timings.check_hbm_form(fj.last_timings())


@pytest.mark.gpu
def test_scalar_hbm_table_path(fj):
    from flash_hash_join_amd import api
    import torch
    bk, pk = _case(50_000, 300_000, 0.6, seed=7)
    t = lambda a: torch.from_numpy(a.view(np.int64)).cuda()
    fj.set_option("scalar_hbm_table", 1)
    try:
        for how, flag in (("inner", 0), ("left", api.ALGO_LEFT_OUTER), ("anti", api.ALGO_ANTI)):
            n, _, pi, bi = api.join_device(api.ALGO_SCALAR | api.ALGO_ROW_IDS | flag, 0, 1, t(bk), None, t(pk), return_arrays=True)
            assert fj.last_timings()["path"] == 1
            hbm_timings.check_hbm_form(fj.last_timings())
            epi, ebi = ref_indices(bk, pk, how)
            pi = pi.cpu().numpy()
            if how == "anti":
                assert n == epi.size and np.array_equal(np.sort(pi), epi)
                continue
            a, b = _pairs(pi, bi.cpu().numpy()), _pairs(epi, ebi)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), how
    finally:
        fj.set_option("scalar_hbm_table", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("many", [False, True], ids=["n_to_1", "many_to_many"])
def test_two_phase_count_then_emit(fj, many):
    """mat_single_pass = 0: join_device counts (no output buffers), then fj_emit_pairs writes the pending row-id result."""
    import torch
    from flash_hash_join_amd import api
    bk, pk = _case(200_000, 1_000_000, 0.5, seed=21)
    t = lambda a: torch.from_numpy(a.view(np.int64)).cuda()
    algo = (api.ALGO_RADIX | api.ALGO_MANY_TO_MANY if many else api.ALGO_RADIX) | api.ALGO_ROW_IDS
    fj.set_option("mat_single_pass", 0)
    try:
        n, _, pi, bi = api.join_device(algo, 0, 1, t(bk), None, t(pk), return_arrays=True)
    finally:
        fj.set_option("mat_single_pass", 1)
    epi, ebi = ref_indices(bk, pk, many=many)
    assert n == epi.size
    a, b = _pairs(pi.cpu().numpy(), bi.cpu().numpy()), _pairs(epi, ebi)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # a key-value join on the same context afterwards is untouched: value = 3 * (first build row of the key)
    bv = np.arange(bk.size, dtype=np.uint64) * np.uint64(3)
    m, _, k, v = fj.hash_join_radix(bk, bv, pk, return_arrays=True)
    fpi, fbi = ref_indices(bk, pk)
    assert m == fpi.size and np.array_equal(np.sort(v), np.sort(bv[fbi]))


@pytest.mark.gpu
def test_large_case_checked_on_the_device(fj):
    import torch
    from flash_hash_join_amd import datagen
    nb, n_p = 50_000_000, 500_000_000
    bk, bv = datagen.build_device(nb, "cuda:0")
    del bv
    pk, expected = datagen.probe_device(n_p, nb, "cuda:0", seed=3, hit_bp=5000)
    n, _, pi, bi = fj.join_indices(bk, pk)
    assert n == expected and 0.45 * n_p < n < 0.55 * n_p
    assert pi.dtype == torch.int64 and bi.dtype == torch.int64 and pi.numel() == n
    assert torch.equal(pk[pi], bk[bi])
    s = torch.sort(pi).values
    assert int(s[0]) >= 0 and int(s[-1]) < n_p and not bool((s[1:] == s[:-1]).any()), "a probe row appears twice"
    del pi, bi, s
    m, _, pi, bi = fj.join_indices(bk, pk, how="left")
    assert m == expected and pi.numel() == n_p
    assert torch.equal(pk[pi[:m]], bk[bi[:m]]) and bool((bi[m:] == -1).all())
    sb = torch.sort(bk).values
    misses = pk[pi[m:]]
    pos = torch.searchsorted(sb, misses).clamp_(max=nb - 1)
    assert not bool((sb[pos] == misses).any()), "an unmatched row's key is in the build side"
    del misses, pos, sb
    assert torch.equal(torch.sort(pi).values, torch.arange(n_p, device=pi.device)), "the two ranges are not a permutation of the probe rows"
    del pi, bi
    torch.cuda.empty_cache()
