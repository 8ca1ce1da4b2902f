"""Many-to-many inner joins whose build side holds a key with thousands of copies (option "mm_heavy_keys", csrc/fj_many.hip
fj_mm_tile_kernel, csrc/fj_joins.hip mm_tile_join): the option's contract without a GPU, and - on an MI355X - exact parity with
the NumPy reference on inputs that the default setting refuses: one hot key, the tables' empty marker as the hot key, a dozen
moderately duplicated keys that overflow one partition together, a Zipf build side; the two-phase form of the C ABI, the timings
field that reports the tiled path, and the outer forms, which keep refusing.

Reference (integers, compared exactly as sorted pair multisets): oracle.np_inner_join / oracle.canon_pairs.  Build values are row
ids, so every build row is distinguishable.  Every heavy case asserts with NumPy alone that its input IS heavy (a key, or a group
of keys that share a final partition, with more than 4096 build rows), that the reference's pair count stays at or below 20M,
and that the same call at the default setting is refused."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import keymix
from conftest import ROOT, product_env

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
LIMIT = 4096                      # build rows per final partition the one-table kernel takes
MAX_PAIRS = 20_000_000
TILED = 4096                      # FJ_LDS_RETRIES_MM_TILED


# ---- inputs (NumPy only) ---------------------------------------------------------------------------------------------------
def refusal_input():
    """The input of test_many_to_many_refuses_a_key_with_too_many_duplicates (tests/test_gpu_parity.py), as it stands there."""
    bk = np.concatenate([np.full(6000, 12345, dtype=np.uint64), np.arange(100000, 100500, dtype=np.uint64)])
    bv = np.arange(bk.size, dtype=np.uint64)
    pk = np.array([12345, 100001, 7], dtype=np.uint64)
    return bk, bv, pk


def hot_key_input(hot):
    """One key 100 000 times among 200 000 rows of 50 000 background ids (about four copies each), shuffled; the probe side
    holds the hot key 40 times among 30 000 draws from twice the background domain (hits and misses)."""
    rng = np.random.default_rng(2024)
    ids = rng.integers(10, 50_010, size=200_000, dtype=np.uint64)
    bk = np.concatenate([np.full(100_000, hot, dtype=np.uint64), ids * GOLDEN])
    rng.shuffle(bk)
    bv = np.arange(bk.size, dtype=np.uint64)
    pk = np.concatenate([np.full(40, hot, dtype=np.uint64), rng.integers(10, 100_010, size=30_000, dtype=np.uint64) * GOLDEN])
    rng.shuffle(pk)
    return bk, bv, pk


def colliding_input():
    """Twelve keys whose hash word 1 agrees in its top 12 bits - the same final partition under every plan of at most 12 radix
    bits; this one has 6 - with 1000..3000 copies each, among 100 000 unique background keys."""
    rng = np.random.default_rng(7)
    cand = np.arange(1, 400_000, dtype=np.uint64)
    top = keymix.hash_w1(cand) >> np.uint32(20)
    group = cand[top == top[0]][:12]
    copies = rng.integers(1000, 3001, size=group.size)
    bk = np.concatenate([np.repeat(group, copies), np.arange(10**9, 10**9 + 100_000, dtype=np.uint64)])
    rng.shuffle(bk)
    bv = np.arange(bk.size, dtype=np.uint64)
    pk = np.concatenate([np.repeat(group, 50), rng.integers(10**9 - 50_000, 10**9 + 150_000, size=40_000, dtype=np.uint64)])
    rng.shuffle(pk)
    return bk, bv, pk, group, copies


def zipf_input():
    """Build side: 1M draws from ranks 1..1M with P(r) ~ 1 / r (the head key holds about 7 % of the rows); probe side: 1500
    draws from the same distribution over the same domain."""
    rng = np.random.default_rng(99)
    n_dom = 1_000_000
    cdf = np.cumsum(1.0 / np.arange(1, n_dom + 1))
    cdf /= cdf[-1]
    draw = lambda n: (np.searchsorted(cdf, rng.random(n)) + 1).astype(np.uint64)
    bk = draw(1_000_000) * GOLDEN
    bv = np.arange(bk.size, dtype=np.uint64)
    pk = draw(1500) * GOLDEN
    return bk, bv, pk


def max_multiplicity(bk):
    return int(np.unique(bk, return_counts=True)[1].max())


def expected(bk, bv, pk):
    from oracle.oracle import np_inner_join
    n = np_inner_join(bk, bv, pk)
    assert 0 < n <= MAX_PAIRS, n                                    # (bounded before anything runs on the GPU)
    return np_inner_join(bk, bv, pk, return_arrays=True)


def same_pairs(k1, v1, k2, v2):
    from oracle.oracle import canon_pairs
    a = canon_pairs(np.asarray(k1).view(np.uint64), np.asarray(v1).view(np.uint64))
    b = canon_pairs(np.asarray(k2).view(np.uint64), np.asarray(v2).view(np.uint64))
    return a[0].size == b[0].size and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def host(t):
    return (t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)).view(np.uint64)


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_the_option_defaults_to_zero_and_round_trips():
    from flash_hash_join_amd import api
    assert api.get_option("mm_heavy_keys") == 0
    try:
        for v in (1, 0, 1):
            api.set_option("mm_heavy_keys", v)
            assert api.get_option("mm_heavy_keys") == v
    finally:
        api.set_option("mm_heavy_keys", 0)
    assert api.get_option("mm_heavy_keys") == 0


@pytest.mark.parametrize("value", [-1, 2, 4096])
def test_a_value_outside_0_and_1_is_refused_with_a_message(value):
    from flash_hash_join_amd import api
    with pytest.raises(RuntimeError, match="mm_heavy_keys must be 0 or 1"):
        api.set_option("mm_heavy_keys", value)
    assert api.get_option("mm_heavy_keys") == 0


def test_fj_options_in_the_environment_sets_it():
    code = "from flash_hash_join_amd import api; print('opt', api.get_option('mm_heavy_keys'))"
    for env_value, want in (("mm_heavy_keys=1", 1), ("mm_heavy_keys=0", 0), ("mm_heavy_keys=2", 0)):
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT,
                             env=product_env(FJ_OPTIONS=env_value))
        assert out.returncode == 0, out.stderr
        assert f"opt {want}" in out.stdout, (env_value, out.stdout, out.stderr)
        assert ("ignoring" in out.stderr) == (env_value == "mm_heavy_keys=2"), out.stderr


def test_the_header_documents_the_option_and_the_abi_version_stays():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    assert int(re.search(r"#define FJ_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert '"mm_heavy_keys"' in hdr
    assert int(re.search(r"#define FJ_LDS_RETRIES_MM_TILED (\d+)", hdr).group(1)) == TILED
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_abi_version() == 8
    for doc in ("README.md", os.path.join("tools", "README.md"), os.path.join("flash_hash_join_amd", "csrc", "fj_host.h")):
        assert "mm_heavy_keys" in open(os.path.join(ROOT, doc)).read(), doc


def test_the_inputs_are_heavy_and_their_results_bounded():
    """What the GPU tests assume of their inputs, checked where no GPU is needed: each is beyond the one-table kernel's limit,
    and the reference's pair count is at most 20M."""
    from oracle.oracle import np_inner_join
    bk, bv, pk = refusal_input()
    assert max_multiplicity(bk) == 6000 > LIMIT and np_inner_join(bk, bv, pk) == 6001
    for hot in (77777, keymix.EMPTY_RAW):
        bk, bv, pk = hot_key_input(hot)
        assert max_multiplicity(bk) == 100_000 and int((bk == np.uint64(hot)).sum()) == 100_000
        n = np_inner_join(bk, bv, pk)
        assert 4_000_000 < n <= MAX_PAIRS, n
        assert 0 < int(np.isin(pk, bk).sum()) < pk.size                          # hits and misses
    assert int(keymix.mix(np.array([keymix.EMPTY_RAW], dtype=np.uint64))[0]) == 2**64 - 1
    bk, bv, pk, group, copies = colliding_input()
    assert group.size == 12 and np.unique(keymix.hash_w1(group) >> np.uint32(20)).size == 1
    assert max_multiplicity(bk) <= 3000 < LIMIT < int(copies.sum()) and int(np.isin(bk, group).sum()) == int(copies.sum())
    assert 0 < np_inner_join(bk, bv, pk) <= MAX_PAIRS
    bk, bv, pk = zipf_input()
    assert bk.size == 1_000_000 and max_multiplicity(bk) > 10 * LIMIT
    assert 1_000_000 < np_inner_join(bk, bv, pk) <= MAX_PAIRS


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fj():
    import flash_join
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_device_count() >= 1, "no HIP device: the product path must not silently fall back"
    assert flash_join.initialize() is None
    return flash_join


@pytest.fixture
def heavy(fj):
    """The option at 1 for the length of a test; the value found before is back afterwards."""
    old = fj.get_option("mm_heavy_keys")
    fj.set_option("mm_heavy_keys", 1)
    try:
        yield fj
    finally:
        fj.set_option("mm_heavy_keys", old)


def to_device(*arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda() for a in arrays)


def check_all_forms(fj, bk, bv, pk, device):
    """inner_join_count, inner_join and join_indices against the reference with the option at 1 (the caller set it); the same
    count call at 0 is refused, and the option is 1 again afterwards."""
    exp, ek, ev = expected(bk, bv, pk)
    args = to_device(bk, bv, pk) if device else (bk, bv, pk)
    fj.set_option("mm_heavy_keys", 0)
    try:
        with pytest.raises(RuntimeError, match="4096 build rows"):
            fj.inner_join_count(*args)
    finally:
        fj.set_option("mm_heavy_keys", 1)
    n, sec = fj.inner_join_count(*args)
    lt = fj.last_timings()
    print(f"count: {n} pairs, expected {exp}, lds_retries {lt['lds_retries']}, join_ms {lt['join_ms']:.3f}")
    assert isinstance(n, int) and isinstance(sec, float) and n == exp
    assert lt["lds_retries"] == TILED and lt["fell_back"] == 0 and lt["path"] == 0, lt
    n, sec, k, v = fj.inner_join(*args, return_arrays=True)
    lt = fj.last_timings()
    print(f"materialise: {n} pairs, join_ms {lt['join_ms']:.3f}, emit_ms {lt['emit_ms']:.3f}")
    assert n == exp and host(k).size == exp
    assert same_pairs(host(k), host(v), ek, ev)
    assert fj.inner_join(*args)[0] == exp                                       # (int, float) form
    n, sec, pi, bi = fj.join_indices(args[0], args[2], how="inner", many_to_many=True)
    pi, bi = host(pi), host(bi)
    assert n == exp and pi.size == exp and bi.size == exp
    assert int(pi.max()) < pk.size and int(bi.max()) < bk.size
    assert np.array_equal(pk[pi.astype(np.int64)], bk[bi.astype(np.int64)])     # every row joins equal keys ...
    assert same_pairs(pk[pi.astype(np.int64)], bv[bi.astype(np.int64)], ek, ev)  # ... and they are the reference's pairs (bv = row id)
    assert np.unique(pi * np.uint64(bk.size) + bi).size == exp                 # no (probe row, build row) twice


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_the_refused_input_is_joined_with_the_option_and_refused_again_without(fj, heavy, device):
    bk, bv, pk = refusal_input()
    assert max_multiplicity(bk) > LIMIT
    check_all_forms(fj, bk, bv, pk, device)
    args = to_device(bk, bv, pk) if device else (bk, bv, pk)
    fj.set_option("mm_heavy_keys", 0)
    try:
        for call in (lambda: fj.inner_join_count(*args), lambda: fj.inner_join(*args, return_arrays=True),
                     lambda: fj.join_indices(args[0], args[2], how="inner", many_to_many=True)):
            with pytest.raises(RuntimeError, match="4096 build rows"):
                call()
    finally:
        fj.set_option("mm_heavy_keys", 1)
    assert fj.hash_join_count_radix(*args)[0] == 2                              # an N:1 join on the same context
    n, _, k, v = fj.hash_join_radix(*args, return_arrays=True)
    assert n == 2 and sorted(host(k).tolist()) == [12345, 100001]


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("hot", [77777, keymix.EMPTY_RAW], ids=["ordinary_key", "empty_marker"])
def test_one_key_with_100k_copies(fj, heavy, hot, device):
    bk, bv, pk = hot_key_input(hot)
    assert max_multiplicity(bk) == 100_000 > LIMIT
    check_all_forms(fj, bk, bv, pk, device)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_moderately_duplicated_keys_that_overflow_one_partition_together(fj, heavy, device):
    bk, bv, pk, group, copies = colliding_input()
    assert max_multiplicity(bk) < LIMIT < int(copies.sum())                     # no heavy key, a heavy partition
    assert np.unique(keymix.hash_w1(group) >> np.uint32(20)).size == 1
    check_all_forms(fj, bk, bv, pk, device)
    assert fj.last_timings()["radix_bits"] <= 12                                # (what "share a final partition" rests on)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_zipf_build_side(fj, heavy, device):
    bk, bv, pk = zipf_input()
    assert max_multiplicity(bk) > LIMIT
    check_all_forms(fj, bk, bv, pk, device)


@pytest.mark.gpu
def test_two_phase_form_of_the_c_abi_and_a_trim_with_the_result_pending(fj, heavy):
    import torch
    from flash_hash_join_amd import _lib, api
    L = _lib.load()
    MANY, ROW_IDS, RADIX = 0x10, 0x80, 2
    bk, bv, pk = hot_key_input(77777)
    assert max_multiplicity(bk) > LIMIT
    exp, ek, ev = expected(bk, bv, pk)
    dbk, dbv, dpk = to_device(bk, bv, pk)
    ctx = api.context(0)
    stream = torch.cuda.current_stream(0).cuda_stream

    def count(algo, ok=None, ov=None, cap=0, t=None):
        cnt = ctypes.c_uint64(7)
        rc = L.fj_join_device(ctx, algo, 0, 1, dbk.data_ptr(), dbv.data_ptr(), bk.size, dpk.data_ptr(), pk.size, stream, 64,
                              ctypes.byref(cnt), ok.data_ptr() if ok is not None else None, ov.data_ptr() if ov is not None else None,
                              cap, ctypes.byref(t) if t is not None else None)
        return rc, int(cnt.value)

    for algo in (RADIX | MANY, RADIX | MANY | ROW_IDS):
        t = _lib.FjTimings()
        rc, n = count(algo, t=t)                                                # counted, pairs pending
        assert rc == 0 and n == exp and t.lds_retries == TILED, (_lib.last_error(), n, exp, t.lds_retries)
        ok = torch.full((exp + 1,), 12345, dtype=torch.int64, device="cuda")
        ov = torch.full((exp + 1,), 12345, dtype=torch.int64, device="cuda")
        assert L.fj_emit_pairs(ctx, ok.data_ptr(), ov.data_ptr(), exp - 1, stream, None) != 0        # one row too few: refused ...
        assert "output capacity" in _lib.last_error()
        _lib.check(L.fj_emit_pairs(ctx, ok.data_ptr(), ov.data_ptr(), exp, stream, ctypes.byref(t)))  # ... and still pending
        assert t.emit_ms > 0 and t.lds_retries == TILED
        assert int(ok[exp]) == 12345 and int(ov[exp]) == 12345, "a row behind the result was written"
        assert L.fj_emit_pairs(ctx, ok.data_ptr(), ov.data_ptr(), exp, stream, None) != 0
        assert "no counted materialising join is pending" in _lib.last_error()
        k, v = host(ok[:exp]), host(ov[:exp])
        if algo & ROW_IDS:
            k, v = pk[k.astype(np.int64)], bv[v.astype(np.int64)]
        assert same_pairs(k, v, ek, ev)
        # one call, enough capacity
        ok2 = torch.full((exp + 5,), 12345, dtype=torch.int64, device="cuda")
        ov2 = torch.full((exp + 5,), 12345, dtype=torch.int64, device="cuda")
        rc, n = count(algo, ok2, ov2, exp + 5)
        assert rc == 0 and n == exp, _lib.last_error()
        assert bool((ok2[exp:] == 12345).all()) and bool((ov2[exp:] == 12345).all())
        k2, v2 = host(ok2[:exp]), host(ov2[:exp])
        if algo & ROW_IDS:
            k2, v2 = pk[k2.astype(np.int64)], bv[v2.astype(np.int64)]
        assert same_pairs(k2, v2, ek, ev)
        assert L.fj_emit_pairs(ctx, ok.data_ptr(), ov.data_ptr(), exp, stream, None) != 0             # nothing pending after it
        # one call, too little capacity: the count is there, the pairs stay pending for fj_emit_pairs
        rc, n = count(algo, ok2, ov2, exp - 1)
        assert rc != 0 and "output capacity" in _lib.last_error() and n == exp
        _lib.check(L.fj_emit_pairs(ctx, ok2.data_ptr(), ov2.data_ptr(), exp, stream, None))
        del ok, ov, ok2, ov2
    # the workspace is given back with such a result pending: the result is dropped, a fresh join is exact
    rc, n = count(RADIX | MANY)
    assert rc == 0 and n == exp
    api.trim_workspace()
    ok = torch.empty(exp, dtype=torch.int64, device="cuda")
    ov = torch.empty(exp, dtype=torch.int64, device="cuda")
    assert L.fj_emit_pairs(ctx, ok.data_ptr(), ov.data_ptr(), exp, stream, None) != 0
    assert "no counted materialising join is pending" in _lib.last_error()
    n, _, k, v = fj.inner_join(dbk, dbv, dpk, return_arrays=True)
    assert n == exp and same_pairs(host(k), host(v), ek, ev)
    # ... and the next call that starts work drops a pending result too
    rc, n = count(RADIX | MANY)
    assert rc == 0 and n == exp
    assert fj.hash_join_count_radix(dbk, dbv, dpk)[0] == int(np.isin(pk, bk).sum())
    assert L.fj_emit_pairs(ctx, ok.data_ptr(), ov.data_ptr(), exp, stream, None) != 0


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_lds_retries_reports_the_tiled_path_and_nothing_else_does(fj, heavy, device):
    from oracle.oracle import np_inner_join
    bk, bv, pk = refusal_input()
    args = to_device(bk, bv, pk) if device else (bk, bv, pk)
    assert fj.inner_join_count(*args)[0] == 6001 and fj.last_timings()["lds_retries"] == TILED
    assert fj.inner_join(*args)[0] == 6001 and fj.last_timings()["lds_retries"] == TILED
    # a many-to-many input no partition of which is beyond the table (the 60 000-row case of tests/test_gpu_parity.py): 0 at either setting
    rng = np.random.default_rng(60007)
    bk = rng.integers(0, 9000, size=60000, dtype=np.uint64) * GOLDEN
    bv = np.arange(bk.size, dtype=np.uint64)
    pk = rng.integers(0, 18001, size=300000, dtype=np.uint64) * GOLDEN
    assert max_multiplicity(bk) < 100
    exp, ek, ev = expected(bk, bv, pk)
    args = to_device(bk, bv, pk) if device else (bk, bv, pk)
    for setting in (1, 0, 1):
        fj.set_option("mm_heavy_keys", setting)
        assert fj.inner_join_count(*args)[0] == exp and fj.last_timings()["lds_retries"] == 0
        n, _, k, v = fj.inner_join(*args, return_arrays=True)
        assert n == exp and fj.last_timings()["lds_retries"] == 0 and same_pairs(host(k), host(v), ek, ev)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_the_outer_forms_keep_refusing_whatever_the_option_says(fj, heavy, device):
    bk, bv, pk = refusal_input()
    args = to_device(bk, bv, pk) if device else (bk, bv, pk)
    assert fj.get_option("mm_heavy_keys") == 1
    with pytest.raises(RuntimeError, match="4096 build rows"):
        fj.left_join(*args, duplicates="all")
    with pytest.raises(RuntimeError, match="4096 build rows"):
        fj.full_join(*args, return_arrays=True, duplicates="all")
    with pytest.raises(RuntimeError, match="4096 build rows"):
        fj.join_indices(args[0], args[2], how="left", duplicates="all")
    with pytest.raises(RuntimeError, match="4096 build rows"):
        fj.join_indices(args[0], args[2], how="full", duplicates="all")
    assert fj.inner_join_count(*args)[0] == 6001                               # the inner form on the same context, right after
    assert fj.left_join(*args)[0] == 2
