"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C ABI via the
flash_join drop-in module, against the CPU oracle and the committed golden vectors.
Bit-exact bar: counts equal; materialised (key, value) pairs equal as multisets."""
import hashlib
import json
import os

import numpy as np
import pytest

from golden_inputs import CASES, make_case

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

COUNT_FUNCS = ["adaptive_join_count", "adaptive_join_count_bloom", "hash_join_count", "hash_join_count_bloom",
               "hash_join_count_radix", "hash_join_count_radix_bloom"]
MAT_FUNCS = ["adaptive_join", "adaptive_join_bloom", "hash_join", "hash_join_bloom", "hash_join_radix",
             "hash_join_radix_bloom"]


@pytest.fixture(scope="module")
def fj():
    import flash_join
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_device_count() >= 1, "no HIP device: the product path must not silently fall back"
    assert flash_join.initialize() is None
    return flash_join


@pytest.fixture(params=[0, 1, 2, 4, 5, 6], ids=["scalar=planned", "scalar=hbm_table", "persistent_join", "deep_plans", "wide_join", "wide_join_deep_plans"])
def scalar_mode(request, fj):
    """Run a test under the dispatch variants of the native library: the hash_join* functions served by the partitioned
    plan (default) or by the literal one-table-in-HBM algorithm (linear probing, bloom word per group); every
    partitioned counting join through the persistent join kernel (by default only plans with >= 8192 items use it); and
    "deep_plans": 32 build keys per final partition instead of 4096, so that the small inputs of these tests run the two-
    and three-pass plans -- and, in the *_bloom functions, the bloom precheck between the probe side's passes -- that
    production only takes for build sides above a million rows; "wide_join": every partitioned counting join on the 16384-slot
    table kernel (fj_join_wide.hip; by default only plans whose partitions average > 3300 build keys), also under deep plans."""
    fj.set_option("plan_target_keys", 32 if request.param in (4, 6) else 4096)
    fj.set_option("join_wide", 1 if request.param in (5, 6) else 2)
    fj.set_option("scalar_hbm_table", int(request.param == 1))
    fj.set_option("persistent_min_items", 0 if request.param == 2 else 8192)
    yield request.param
    fj.set_option("scalar_hbm_table", 0)
    fj.set_option("persistent_min_items", 8192)
    fj.set_option("plan_target_keys", 4096)
    fj.set_option("join_wide", 2)


def _digest(oracle, k, v):
    k, v = oracle.canon_pairs(k, v)
    return hashlib.sha256(k.tobytes() + v.tobytes()).hexdigest()


def _golden():
    with open(os.path.join(HERE, "golden", "golden_joins.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", CASES)
def test_all_twelve_functions_match_golden_vectors(fj, oracle, name, scalar_mode):
    g = _golden()[name]
    bk, bv, pk = make_case(name)
    for fn in COUNT_FUNCS + MAT_FUNCS:
        res = getattr(fj, fn)(bk, bv, pk)
        assert isinstance(res, tuple) and len(res) == 2, fn             # (int, float) like the reference
        assert isinstance(res[0], int) and isinstance(res[1], float), fn
        assert res[0] == g["count"], (fn, res[0], g["count"])
    for fn in MAT_FUNCS:
        n, sec, k, v = getattr(fj, fn)(bk, bv, pk, return_arrays=True)
        assert n == g["count"] and k.size == n and v.size == n, fn
        assert _digest(oracle, k, v) == g["pairs_sha256"], fn


def test_golden_vectors_through_the_product_library(fj):
    """This test process loads the lab build of the library (conftest.py: the same objects, linked without the export list).  The
    PRODUCT library - what a host binds - runs in a child process here: the twelve functions on every golden case, pair digests
    included, and the driver's own smoke()."""
    import subprocess
    import sys
    from conftest import ROOT, product_env
    code = """
import hashlib, json, os, sys
sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np
import flash_join
from flash_hash_join_amd import _lib
from golden_inputs import CASES, make_case
assert _lib.LIB_PATH.endswith("libflashjoin_hip.so") and not _lib.load().has_lab, _lib.LIB_PATH
g = json.load(open(os.path.join(%r, "tests", "golden", "golden_joins.json")))
def digest(k, v):
    o = np.lexsort((v, k)); k, v = k[o], v[o]
    return hashlib.sha256(k.tobytes() + v.tobytes()).hexdigest()
for name in CASES:
    bk, bv, pk = make_case(name)
    for fn in ("hash_join_count", "hash_join_count_bloom", "hash_join_count_radix", "hash_join_count_radix_bloom", "adaptive_join_count", "adaptive_join_count_bloom",
               "hash_join", "hash_join_bloom", "hash_join_radix", "hash_join_radix_bloom", "adaptive_join", "adaptive_join_bloom"):
        assert getattr(flash_join, fn)(bk, bv, pk)[0] == g[name]["count"], (name, fn)
    for fn in ("hash_join", "hash_join_radix", "adaptive_join"):
        n, sec, k, v = getattr(flash_join, fn)(bk, bv, pk, return_arrays=True)
        assert n == g[name]["count"] and digest(k.view(np.uint64), v.view(np.uint64)) == g[name]["pairs_sha256"], (name, fn)
import __graft_entry__
__graft_entry__.smoke()
print("PRODUCT OK", len(CASES))
""" % (ROOT, ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, cwd=ROOT, env=product_env())
    assert out.returncode == 0 and "PRODUCT OK" in out.stdout, out.stdout[-1500:] + out.stderr[-2500:]


def test_big_golden_case_two_pass_plan_and_the_wide_join_kernel(fj, oracle):
    """A committed fixture of 21M x 50M rows (tests/golden/golden_joins.json: count and pair digest by the C restatement AND the
    NumPy oracle, tests/golden/make_golden.py): a two-pass plan and the bucketed wide join kernel meet a golden vector, not only
    the generator's closed form.  Counting functions under the default dispatch, with the wide kernel forced on and off; pairs once."""
    from golden_inputs import BIG_CASES
    for name in BIG_CASES:
        g = _golden()[name]
        bk, bv, pk = make_case(name)
        assert bk.size == g["nb"] and pk.size == g["np"]
        for wide in (2, 1, 0):
            fj.set_option("join_wide", wide)
            try:
                for fn in ("hash_join_count_radix", "adaptive_join_count", "hash_join_count_radix_bloom"):
                    n, _ = getattr(fj, fn)(bk, bv, pk)
                    assert n == g["count"], (name, fn, wide, n, g["count"])
                    lt = fj.last_timings()
                    assert lt["passes"] == 2 and lt["fell_back"] == 0 and lt["lds_retries"] == 0, lt
            finally:
                fj.set_option("join_wide", 2)
        n, _, k, v = fj.hash_join_radix(bk, bv, pk, return_arrays=True)
        assert n == g["count"] and _digest(oracle, k, v) == g["pairs_sha256"]


def test_bench_line_at_one_gpu_is_self_consistent(fj):
    """`python bench.py --steps 3` (N = 1, the headline configuration) prints ONE JSON line whose per-kernel accounting adds up:
    every kernel's fraction of the HBM peak is <= 1, and the timed kernels' launch time x launches per step does not exceed the
    step (they run one after the other on one stream)."""
    import subprocess
    import sys
    from conftest import ROOT
    from conftest import product_env
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-host-entry"],
                         capture_output=True, text=True, timeout=900, cwd=ROOT, env=product_env())
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["config"]["bench_workload"] == "c3" and d["dtype"] == "int64" and d["vs_baseline"] is None
    assert d["config"]["build_rows_total"] == 100_000_000 and d["config"]["probe_rows_total"] == 1_000_000_000
    rows = d["roofline_kernels"]
    assert rows and all(0 < r["frac"] <= 1.0 for r in rows), rows
    kernel_ms = sum(r["avg_launch_ms"] * r["launches_per_step"] for r in rows)
    assert kernel_ms <= d["ms_per_step"] * 1.001, (kernel_ms, d["ms_per_step"])
    assert kernel_ms >= 0.8 * d["ms_per_step"], (kernel_ms, d["ms_per_step"])      # ... and they ARE the step: nothing big goes untimed
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["kernel"] == rows[0]["kernel"] and r["frac"] == rows[0]["frac"] and 0 < r["frac"] <= 1.0
    assert abs(d["value"] - 1e9 / (d["ms_per_step"] * 1e-3) / 1e9) < 0.01 * d["value"]


def test_bench_dumps_what_its_last_timed_step_returned(fj, tmp_path):
    """`python bench.py --dump-outputs DIR` on a materialising workload (c3_mat at 1/100: 1M x 10M rows, 5M pairs): the count and
    the fixed sample of the pairs equal what the generator's closed form says the join must return; a plain run leaves out what
    --full measures."""
    import subprocess
    import sys
    import bench
    from conftest import ROOT
    from conftest import product_env
    from flash_hash_join_amd import datagen
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "c3_mat", "--scale", "0.01", "--steps", "2",
                          "--warmup", "1", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=900, cwd=ROOT, env=product_env())
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["steps"] == 2 and d["ms_per_step"] > 0 and not {"cpu_baseline", "cpu_baseline_c1", "host_entry"} & set(d), sorted(d)
    nb, npk = 1_000_000, 10_000_000
    pk, exp = datagen.probe_numpy(npk, nb, seed=1, hit_bp=5000)
    with np.errstate(over="ignore"):
        r = pk * np.uint64(pow(0x9E3779B97F4A7C15, -1, 1 << 64))            # build row i has key (i + 1) * M, value i
    hit = (r >= 1) & (r <= nb)
    keys, vals = pk[hit], r[hit] - np.uint64(1)
    assert np.load(tmp_path / "match_count.npy").tolist() == [float(exp)] == [float(hit.sum())] == [float(d["config"]["matches"])]
    sel = (keys >> np.uint64(32)) < np.uint64((bench.DUMP_MAX_PAIRS << 32) // keys.size)
    o = np.lexsort((vals[sel], keys[sel]))
    ek, ev = keys[sel][o][:bench.DUMP_MAX_PAIRS], vals[sel][o][:bench.DUMP_MAX_PAIRS]
    for name, x in (("key", ek), ("value", ev)):
        hi, lo = np.load(tmp_path / f"pairs_{name}_hi.npy"), np.load(tmp_path / f"pairs_{name}_lo.npy")
        assert hi.dtype == lo.dtype == np.float64 and hi.size == x.size > 0
        assert np.array_equal((hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64), x), name


def test_against_c_oracle_on_fresh_random_inputs(fj, oracle, scalar_mode):
    rng = np.random.default_rng(2024)
    for nb, npk in [(1, 1), (2, 3), (255, 1000), (4096, 50000), (4097, 50000), (30000, 1), (123457, 654321)]:
        bk = np.unique(rng.integers(0, 2**64, size=nb, dtype=np.uint64))
        bv = rng.integers(0, 2**64, size=bk.size, dtype=np.uint64)
        pk = np.concatenate([rng.choice(bk, npk // 2 + 1), rng.integers(0, 2**64, size=npk // 2, dtype=np.uint64)])
        exp, _, ek, ev = oracle.c_join(bk, bv, pk, algo="radix", materialize=True, return_arrays=True)
        assert exp == oracle.np_join(bk, bv, pk)
        for fn in COUNT_FUNCS:
            assert getattr(fj, fn)(bk, bv, pk)[0] == exp, (fn, nb, npk)
        for fn in ("hash_join", "hash_join_radix"):
            n, _, k, v = getattr(fj, fn)(bk, bv, pk, return_arrays=True)
            assert n == exp
            a, b = oracle.canon_pairs(k, v), oracle.canon_pairs(ek, ev)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (fn, nb, npk)


def test_empty_inputs_return_zero(fj, scalar_mode):
    e = np.empty(0, dtype=np.uint64)
    one = np.array([7], dtype=np.uint64)
    for fn in COUNT_FUNCS + MAT_FUNCS:
        f = getattr(fj, fn)
        assert f(e, e, one)[0] == 0 and f(one, one, e)[0] == 0 and f(e, e, e)[0] == 0
    n, _, k, v = fj.hash_join_radix(e, e, one, return_arrays=True)
    assert n == 0 and k.size == 0 and v.size == 0


def test_int64_inputs_and_duplicates(fj, oracle, scalar_mode):
    bk = np.array([-1, -2, 5, 5, 5, 0], dtype=np.int64)
    bv = np.array([1, 2, 3, 3, 3, 9], dtype=np.int64)
    pk = np.array([-1, 5, 5, -3, 0, 2**63 - 1, -2], dtype=np.int64)
    exp = oracle.np_join(bk, bv, pk)
    assert exp == 5
    for fn in COUNT_FUNCS:
        assert getattr(fj, fn)(bk, bv, pk)[0] == exp
    n, _, k, v = fj.hash_join_radix(bk, bv, pk, return_arrays=True)
    pairs = sorted(zip(k.view(np.int64).tolist(), v.tolist()))
    assert pairs == sorted([(-1, 1), (5, 3), (5, 3), (0, 9), (-2, 2)])


def test_adaptive_threshold_both_sides(fj, oracle):
    """B = 999,999 and 1,000,000 (the reference's switch point, hash_join.cpp:576) both correct."""
    from flash_hash_join_amd import datagen
    for nb in (999_999, 1_000_000):
        bk, bv = datagen.build_numpy(nb)
        pk, exp = datagen.probe_numpy(300_000, nb, seed=3, hit_bp=5000)
        assert fj.adaptive_join_count(bk, bv, pk)[0] == exp
        assert fj.adaptive_join_count_bloom(bk, bv, pk)[0] == exp


@pytest.mark.gpu
@pytest.mark.parametrize("copies", [756, 3900])
def test_a_small_build_side_of_one_repeated_key_joins(fj, copies):
    """A build side below the partitioning threshold (no pass: one LDS table for the whole join) that is ONE key repeated: hundreds of
    copies inserted in the same instant miss each other's tags, and the tagged table of the materialising pass used to fill both
    candidate groups with copies and then walk until it counted as full - every materialising function raised "could not place every
    partition in LDS" (found by tools/r6_api_fuzz.py).  All twelve functions: counts exact, one pair per probe row, the FIRST
    occurrence's value (hash_join.cpp:125)."""
    import torch
    dev = "cuda:0"
    key = 123456789012345
    bk = torch.full((copies,), key, device=dev, dtype=torch.int64)
    bv = torch.arange(copies, device=dev, dtype=torch.int64) + 17
    pk = torch.cat([bk[:1].repeat(1793), torch.arange(5, device=dev, dtype=torch.int64)]).contiguous()
    for name in ("adaptive_join_count", "adaptive_join_count_bloom", "hash_join_count_radix", "hash_join_count", "hash_join_count_radix_bloom", "hash_join_count_bloom"):
        assert getattr(fj, name)(bk, bv, pk)[0] == 1793, name
    for name in ("adaptive_join", "adaptive_join_bloom", "hash_join_radix", "hash_join", "hash_join_radix_bloom", "hash_join_bloom"):
        for single in (1, 0):
            fj.set_option("mat_single_pass", single)
            try:
                n, _, k, v = getattr(fj, name)(bk, bv, pk, return_arrays=True)
            finally:
                fj.set_option("mat_single_pass", 1)
            assert n == 1793 == k.numel() and bool((k == key).all()) and bool((v == 17).all()), (name, single, n)


@pytest.mark.gpu
def test_millions_of_copies_of_a_few_build_keys_are_counted_once(fj):
    """Three distinct build keys, two million copies each, in a shape that takes the bucketed join (fewer than 3 probe rows per build
    row): their partitions are far beyond any LDS table, the probe side of each is cut into hundreds of items, and the retry ladder
    - tagged table per item, then the partition re-partitioned and joined whole (skew_join) - must not count an item twice.  Round 6's
    fuzz (tools/r6_wide_fuzz.py) found it doing so: the tagged kernel's verdict on a partition differs from item to item under
    racing duplicate inserts, and skew_join added the whole partition on top of what its other items had counted (15.9M instead of
    12M matches, differently on every run).  hash_join.cpp:125 (duplicates dropped at insert), :153-182 (one match per probe row)."""
    import torch
    dev = "cuda:0"
    g = torch.Generator(device=dev); g.manual_seed(77)
    nb, npk, d = 6_000_000, 12_000_000, 3
    bk = torch.randint(-2**62, 2**62, (nb,), device=dev, dtype=torch.int64, generator=g)[:d].repeat(nb // d).contiguous()
    bv = torch.arange(bk.numel(), device=dev, dtype=torch.int64)
    pk = bk[torch.randint(0, bk.numel(), (npk,), device=dev, generator=g)].contiguous()
    try:
        for mode in (2, 1, 0):                                  # the plan's choice (the bucketed kernel), the bucketed kernel forced, the cuckoo kernel
            fj.set_option("join_wide", mode)
            for rep in range(3):
                n = fj.join_device(1, 0, 0, bk, bv, pk, return_arrays=False)[0]
                assert n == npk, (mode, rep, n, fj.last_timings())
    finally:
        fj.set_option("join_wide", 2)


def test_lds_overflow_falls_back_to_global_table(fj, oracle):
    """Every build key lands in ONE radix partition (> LDS table capacity): the radix path must detect it; the join
    re-partitions that partition alone by more radix bits (counting and materialising joins) - exact either way."""
    def hash_w1(k):                                                # fj_hash_w1 of csrc/fj_common.h
        lo = (k & np.uint64(0xFFFFFFFF)).astype(np.uint32); hi = (k >> np.uint64(32)).astype(np.uint32)
        with np.errstate(over="ignore"):
            x = (lo * np.uint32(0x9E3779B1)) ^ (hi * np.uint32(0x85EBCA77))
            x ^= x >> np.uint32(16); x *= np.uint32(0x85ebca6b)
            x ^= x >> np.uint32(13); x *= np.uint32(0xc2b2ae35)
            x ^= x >> np.uint32(16)
        return x
    cand = np.arange(1, 400000, dtype=np.uint64)
    bk = cand[(hash_w1(cand) >> np.uint32(27)) == 0][:9000]      # top 5 hash bits equal -> one partition of the 32 the plan makes
    assert bk.size == 9000
    bv = bk + np.uint64(1)
    pk = np.concatenate([bk, cand[:50000]])
    exp = oracle.np_join(bk, bv, pk)
    n, sec = fj.hash_join_count_radix(bk, bv, pk)
    assert n == exp
    lt = fj.last_timings()
    assert lt["fell_back"] == 0 and lt["lds_retries"] == 2, lt      # counting joins re-partition the one oversized partition alone (round 3)
    n, _, k, v = fj.hash_join_radix(bk, bv, pk, return_arrays=True)
    assert n == exp and np.array_equal(np.sort(v), np.sort(k) + np.uint64(1))
    assert np.array_equal(np.sort(k), np.sort(pk[np.isin(pk, bk)]))
    lt = fj.last_timings()
    assert lt["fell_back"] == 0 and lt["lds_retries"] == 2, lt      # ... and so do materialising joins (a second item set behind the first)
    # duplicate build keys + an oversized partition: the first-occurrence emit path re-partitions the whole build side with row
    # indices and then the oversized partition again from that level - no fallback, and every duplicated key gets the value of its
    # FIRST occurrence, as the reference's radix path does (stable partition + key-only dedup, hash_join.cpp:125, :226-234)
    bk2, bv2 = np.concatenate([bk, bk[:100]]), np.concatenate([bv, bv[:100] + np.uint64(5)])
    n, _, k, v = fj.hash_join_radix(bk2, bv2, pk, return_arrays=True)
    lt = fj.last_timings()
    assert n == exp and lt["fell_back"] == 0, lt
    assert np.array_equal(np.sort(k), np.sort(pk[np.isin(pk, bk)]))
    assert np.all(v - k == 1)
    # ... also when the later occurrence comes FIRST in the other order (the smallest row index wins, whatever the value)
    bk3, bv3 = np.concatenate([bk[:100], bk]), np.concatenate([bv[:100] + np.uint64(5), bv])
    n, _, k, v = fj.hash_join_radix(bk3, bv3, pk, return_arrays=True)
    assert n == exp and fj.last_timings()["fell_back"] == 0
    d = v - k
    assert np.all(np.where(np.isin(k, bk[:100]), d == 6, d == 1))
    ek, ev = oracle.c_join(bk3, bv3, pk, algo="radix", materialize=True, return_arrays=True)[2:]
    a, b = oracle.canon_pairs(k, v), oracle.canon_pairs(ek, ev)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("nb", [3_800, 4_096, 1 << 20, 1 << 27])
def test_build_sizes_at_the_edge_of_the_lds_table_do_not_fall_back(fj, nb):
    """nb = 4096 * 2^k is the worst case for a plan that aims at 4096 keys per 8192-slot table: the counting join's cuckoo
    table is reliable only to a load of ~0.42.  The plan takes one more radix bit where that is free, and partitions that
    still overflow are redone one by one on the tagged table - never the whole join on the HBM table."""
    import torch
    from flash_hash_join_amd import datagen
    npk = min(4 * nb, 200_000_000)
    dbk, dbv = datagen.build_device(nb, "cuda:0")
    dpk, exp = datagen.probe_device(npk, nb, "cuda:0", seed=31, hit_bp=5000)
    n, _ = fj.hash_join_count_radix(dbk, dbv, dpk)
    t = fj.last_timings()
    assert n == exp and t["fell_back"] == 0 and t["path"] == 0, t
    n, _, k, v = fj.hash_join_radix(dbk, dbv, dpk, return_arrays=True)
    assert n == exp and fj.last_timings()["fell_back"] == 0
    M = torch.tensor(-7046029254386353131, dtype=torch.int64, device="cuda:0")
    assert bool(torch.all((v + 1) * M == k))
    del dbk, dbv, dpk, k, v
    torch.cuda.empty_cache()


def test_partition_over_the_cuckoo_limit_is_redone_on_the_tagged_table(fj, oracle):
    """6000 build keys in ONE partition: too many for the counting join's cuckoo table (4096 at best), fine for the tagged
    table (8128): only that partition's items are redone (lds_retries), no HBM-table fallback; duplicates among them keep
    first-occurrence semantics in the materialising join."""
    def hash_w1(k):                                                # fj_hash_w1 of csrc/fj_common.h
        lo = (k & np.uint64(0xFFFFFFFF)).astype(np.uint32); hi = (k >> np.uint64(32)).astype(np.uint32)
        with np.errstate(over="ignore"):
            x = (lo * np.uint32(0x9E3779B1)) ^ (hi * np.uint32(0x85EBCA77))
            x ^= x >> np.uint32(16); x *= np.uint32(0x85ebca6b)
            x ^= x >> np.uint32(13); x *= np.uint32(0xc2b2ae35)
            x ^= x >> np.uint32(16)
        return x
    cand = np.arange(1, 400000, dtype=np.uint64)
    one = cand[(hash_w1(cand) >> np.uint32(27)) == 0][:6000]     # top 5 hash bits equal -> one of the plan's 32 partitions
    rest = cand[(hash_w1(cand) >> np.uint32(27)) != 0][:3000]
    bk = np.concatenate([one, rest, one[:500]])                    # 500 duplicated keys with different values
    bv = np.arange(bk.size, dtype=np.uint64) + np.uint64(7)
    pk = np.concatenate([bk, cand[:50000]])
    exp, ek, ev = oracle.np_join(bk, bv, pk, return_arrays=True)
    n, _ = fj.hash_join_count_radix(bk, bv, pk)
    t = fj.last_timings()
    assert n == exp and t["fell_back"] == 0 and t["lds_retries"] == 1, t
    n, _, k, v = fj.hash_join_radix(bk, bv, pk, return_arrays=True)
    assert n == exp and fj.last_timings()["fell_back"] == 0
    a, b = oracle.canon_pairs(k, v), oracle.canon_pairs(ek, ev)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # The emitting pass of a unique-key build runs on the cuckoo table too (fj_emit_join_persistent); a table that
    # overflows there marks its item and the host redoes the marked items on the tagged table.  (A partition the COUNTING
    # pass already had to retry reports "duplicates possible" and takes the tagged kernel anyway, so the path is driven by
    # the kernel's test hook: lab_hooks & 64 (FJ_HOOK_EMIT_RETRY_7TH) sends every 7th item through it.)
    ubk = np.concatenate([one[:3000], rest])
    ubv = np.arange(ubk.size, dtype=np.uint64) * np.uint64(3) + np.uint64(1)
    upk = np.concatenate([ubk, ubk[::2], cand[:50000]])
    exp, ek, ev = oracle.np_join(ubk, ubv, upk, return_arrays=True)
    fj.set_option("lab_hooks", 64)
    try:
        n, _, k, v = fj.hash_join_radix(ubk, ubv, upk, return_arrays=True)
        t = fj.last_timings()
    finally:
        fj.set_option("lab_hooks", 0)
    assert n == exp and t["fell_back"] == 0 and t["lds_retries"] == 1, t      # the emitting pass's retry launch
    a, b = oracle.canon_pairs(k, v), oracle.canon_pairs(ek, ev)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    n, _, k, v = fj.hash_join_radix(ubk, ubv, upk, return_arrays=True)             # and without the hook: no retry
    assert n == exp and fj.last_timings()["lds_retries"] == 0
    a = oracle.canon_pairs(k, v)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_j1_harness_prints_parsable_result_lines(fj):
    """tools/benchmark_j1.py (the reference's benchmark.py cases, benchmark.py:83, :240-274): every RESULT line parses, the
    six implementations x two tasks are there for the three J1 cases, the CPU column (oracle port) rides along, and all
    columns of a case agree on the result."""
    import re
    import subprocess
    import sys
    from conftest import ROOT
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "benchmark_j1.py"), "--sizes", "1e6", "--reps", "1", "--cpu", "--duckdb"],
                         capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    # the reference's field set and order (benchmark.py:83), this harness's extras behind Result=
    pat = re.compile(r"^RESULT,Library=([\w]+),Task=(join_count|join_materialize),Threads=([\w+]+),Time=([\d.]+),Result=(\d+),Case=([\w\.\-+]+)(?:,Core=([\d.]+))?$")
    rows = [pat.match(l.strip()) for l in out.stdout.splitlines() if l.strip().startswith("RESULT,")]
    assert rows and all(rows), [l for l in out.stdout.splitlines() if l.startswith("RESULT,") and not pat.match(l.strip())]
    by_case = {}
    for m in rows:
        by_case.setdefault(m.group(6), []).append(m)
    assert sorted(by_case) == ["1e6-Q1", "1e6-Q2", "1e6-Q5"]
    for case, ms in by_case.items():
        libs = {(m.group(1), m.group(2)) for m in ms}
        for lib in ("adaptive_join", "adaptive_bloom", "flash_join", "flash_join_bloom", "flash_join_radix", "flash_join_radix_bloom", "cpu_reference_port"):
            assert (lib, "join_count") in libs and (lib, "join_materialize") in libs, (case, lib)
        assert len({m.group(5) for m in ms}) == 1, (case, "implementations disagree")
        assert all(float(m.group(4)) > 0 for m in ms)


def test_numpy_entry_streams_the_join_under_the_copy(fj, oracle):
    """fj_join_host: pageable NumPy arrays go through a pinned ring in pieces of >= 16 MiB; a counting join of the partitioned
    plan gets its first pass per piece while the next piece crosses PCIe (host_streamed), materialising joins copy first.
    Results equal the oracle's either way, including a probe side of several pieces with a ragged tail."""
    from flash_hash_join_amd import datagen
    nb, npk = 700_000, 9_000_001                                   # 72 MB of probe keys: five pieces, odd tail
    bk, bv = datagen.build_numpy(nb)
    pk, exp = datagen.probe_numpy(npk, nb, seed=13, hit_bp=4000)
    for fn in COUNT_FUNCS:
        n, sec = getattr(fj, fn)(bk, bv, pk)
        t = fj.last_timings()
        assert n == exp and t["host_streamed"] == 1 and t["h2d_ms"] > 0, (fn, t)
    n, sec, k, v = fj.hash_join_radix(bk, bv, pk, return_arrays=True)
    assert n == exp and fj.last_timings()["host_streamed"] == 0
    assert np.array_equal(k, (v + np.uint64(1)) * datagen.M)
    fj.set_option("scalar_hbm_table", 1)
    try:
        assert fj.hash_join_count(bk, bv, pk)[0] == exp and fj.last_timings()["host_streamed"] == 0 and fj.last_timings()["path"] == 1
    finally:
        fj.set_option("scalar_hbm_table", 0)


def test_device_tensor_inputs_and_device_generators(fj, oracle):
    import torch
    from flash_hash_join_amd import datagen
    nb, npk = 300_000, 2_000_000
    dbk, dbv = datagen.build_device(nb, "cuda:0")
    dpk, exp = datagen.probe_device(npk, nb, "cuda:0", seed=1, hit_bp=5000)
    hbk, hbv = datagen.build_numpy(nb)
    hpk, hexp = datagen.probe_numpy(npk, nb, seed=1, hit_bp=5000)
    assert exp == hexp                                                              # same generator on both sides
    assert np.array_equal(dbk.cpu().numpy().view(np.uint64), hbk)
    assert np.array_equal(dbv.cpu().numpy().view(np.uint64), hbv)
    assert np.array_equal(dpk.cpu().numpy().view(np.uint64), hpk)
    for fn in COUNT_FUNCS:
        assert getattr(fj, fn)(dbk, dbv, dpk)[0] == exp, fn
    n, sec, k, v = fj.hash_join_radix(dbk, dbv, dpk, return_arrays=True)
    assert n == exp and k.is_cuda and k.numel() == n
    kk, vv = k.cpu().numpy().view(np.uint64), v.cpu().numpy().view(np.uint64)
    assert np.array_equal(kk, (vv + np.uint64(1)) * datagen.M)                      # value i belongs to key (i+1)*M
    _, ek, ev = oracle.np_join(hbk, hbv, hpk, return_arrays=True)
    a, b = oracle.canon_pairs(kk, vv), oracle.canon_pairs(ek, ev)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])

    class Foreign:                       # a device array of "another library": only the DLPack protocol is visible
        def __init__(self, t): self._t = t
        def __dlpack__(self, stream=None): return self._t.__dlpack__() if stream is None else self._t.__dlpack__(stream=stream)
        def __dlpack_device__(self): return self._t.__dlpack_device__()
    assert fj.hash_join_count_radix(Foreign(dbk), Foreign(dbv), Foreign(dpk))[0] == exp
    # host containers that are not ndarrays: pandas, Arrow, lists
    import pandas as pd
    import pyarrow as pa
    small_k, small_v, small_p = hbk[:5000], hbv[:5000], hpk[:20000]
    e2 = oracle.np_join(small_k, small_v, small_p)
    assert fj.hash_join_count(pd.Series(small_k), pd.Series(small_v), pd.Series(small_p))[0] == e2
    assert fj.hash_join_count(pa.array(small_k), pa.array(small_v), pa.array(small_p))[0] == e2
    assert fj.adaptive_join_count(small_k.tolist(), small_v.tolist(), small_p.tolist())[0] == e2


@pytest.mark.parametrize("n,bits,with_vals", [(1000, 3, True), (100_000, 8, False), (300_000, 7, True),
                                                (2_000_000, 13, False), (1_500_000, 10, True), (700_001, 16, False),
                                                (2_000_000, 17, False), (1_200_000, 17, True), (3_000_000, 18, False),
                                                (2_500_000, 18, True), (1_000_000, 20, False), (1_500_000, 9, False), (800_000, 9, True)])
def test_partition_pass_in_isolation(fj, n, bits, with_vals):
    """fj_debug_partition: the chunk lists are a permutation of the input and every row sits in the
    bucket named by the top `bits` bits of its hash (1 pass for bits <= 9 -- a 512-bucket pass at exactly 9 --, 2 passes up to
    18 bits -- 512-bucket passes above 16 --, 3 passes above)."""
    import ctypes
    import torch
    from flash_hash_join_amd import _lib, api
    L = _lib.load()
    rng = np.random.default_rng(n + bits)
    keys = rng.integers(0, 2**64, size=n, dtype=np.uint64)
    keys[: n // 10] = keys[0]                                                    # a heavy duplicate: skewed bucket
    vals = np.arange(n, dtype=np.uint64)
    dk = torch.from_numpy(keys.view(np.int64)).cuda()
    dv = torch.from_numpy(vals.view(np.int64)).cuda() if with_vals else None
    ok = np.zeros(n, dtype=np.uint64); ov = np.zeros(n, dtype=np.uint64); ob = np.zeros(n, dtype=np.uint32)
    nvalid = ctypes.c_uint64(0)
    _lib.check(L.fj_debug_partition(api.context(0), dk.data_ptr(), dv.data_ptr() if with_vals else None, n, bits, 64,
                                    torch.cuda.current_stream(0).cuda_stream, ok.ctypes.data,
                                    ov.ctypes.data if with_vals else None, ob.ctypes.data, ctypes.byref(nvalid)))
    assert nvalid.value == n
    def hash_w1(k):                                                # fj_hash_w1 of csrc/fj_common.h
        lo = (k & np.uint64(0xFFFFFFFF)).astype(np.uint32); hi = (k >> np.uint64(32)).astype(np.uint32)
        with np.errstate(over="ignore"):
            x = (lo * np.uint32(0x9E3779B1)) ^ (hi * np.uint32(0x85EBCA77))
            x ^= x >> np.uint32(16); x *= np.uint32(0x85ebca6b)
            x ^= x >> np.uint32(13); x *= np.uint32(0xc2b2ae35)
            x ^= x >> np.uint32(16)
        return x
    if with_vals:
        assert np.array_equal(np.sort(ov), vals)                                 # permutation of the rows
        assert np.array_equal(keys[ov.astype(np.int64)], ok)                     # values travelled with their keys
    else:
        assert np.array_equal(np.sort(ok), np.sort(keys))
    assert np.array_equal(hash_w1(ok) >> np.uint32(32 - bits), ob)               # every row sits in its hash's bucket
    assert np.all(np.diff(ob.astype(np.int64)) >= 0)


def test_owner_split_then_local_joins_equals_global_join(fj):
    """Multi-GPU building blocks on one GPU: split into 8 owner segments, join each with
    hash_top_bits=48, sum == global count; segments are a permutation of the input."""
    import ctypes
    import torch
    from flash_hash_join_amd import datagen, api
    from flash_hash_join_amd.lab import LabEngine as HipEngine
    nb, npk, world = 1_000_000, 5_000_000, 8
    dbk, dbv = datagen.build_device(nb, "cuda:0")
    dpk, exp = datagen.probe_device(npk, nb, "cuda:0", seed=5, hit_bp=2500)
    eng = HipEngine("cuda:0")
    bk_s, bv_s, bc = eng.owner_split(dbk, dbv, world)
    pk_s, _, pc = eng.owner_split(dpk, None, world)
    assert sum(bc) == nb and sum(pc) == npk
    assert torch.equal(torch.sort(bk_s)[0], torch.sort(dbk)[0])
    assert torch.equal(torch.sort(pk_s)[0], torch.sort(dpk)[0])
    i = torch.argsort(bk_s)
    j = torch.argsort(dbk)
    assert torch.equal(bv_s[i], dbv[j])                                            # values moved with their keys
    total, bo, po = 0, 0, 0
    for r in range(world):
        assert abs(bc[r] - nb / world) < 0.05 * nb / world                           # balanced for uniform keys
        n, _ = api.join_device(api.ALGO_RADIX, 0, 0, bk_s[bo:bo + bc[r]].clone(), bv_s[bo:bo + bc[r]].clone(),
                               pk_s[po:po + pc[r]].clone(), hash_top_bits=48)
        total += n
        bo += bc[r]; po += pc[r]
    assert total == exp


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("nb_total,nb,npk,bpieces,ppieces", [(3_000_000, 1_000_000, 2_500_000, 1, 2), (40_000_000, 5_000_000, 30_000_000, 1, 3),
                                                              (300_000_000, 3_000_000, 20_000_000, 2, 1)])
def test_owner_shuffle_in_chunk_form_on_one_gpu(fj, world, nb_total, nb, npk, bpieces, ppieces):
    """The SURVEY 8(e) sender shape (the first radix pass of the GLOBAL plan is the owner split) with all ranks played by
    one GPU: fj_shuffle_pack_begin / _counts / _finish rewrite a relation for the wire - per owner rank a dense run of 256-key
    chunks (7 bytes per key when the first pass has >= 256 buckets) whose keys all hash to the bucket their directory word
    names, a bucket that rank owns; at most one partial chunk per bucket; nothing lost or invented - and every owner, fed what
    the `senders` packed for it (fj_stream_open_shuffled / append_*_chunks: the second pass unpacks the wire format), counts
    its share of the join: the shares add up to the closed-form count.  nb_total (the plan's build size) > nb emulates a rank
    of a larger job: plans of 256 and 512 first-pass buckets (and 32 for the small plan: whole 8-byte keys on the wire)."""
    import torch
    import keymix
    from flash_hash_join_amd import datagen
    from flash_hash_join_amd.lab import LabEngine as HipEngine
    eng = HipEngine("cuda:0")
    f0 = eng.shuffle_plan(nb_total, world)
    assert 5 <= f0 <= 9 and (1 << f0) >= world                    # 5 + 5, 7 + 7 and 9 + 8 bits for the three plan sizes
    cb = eng.shuffle_chunk_bytes(nb_total, world)
    assert cb == (1792 if f0 >= 8 else 2048)
    bk, _ = datagen.build_device(nb, "cuda:0")
    pk, exp = datagen.probe_device(npk, nb, "cuda:0", seed=21, hit_bp=4000)

    def pack_pieces(rel, pieces):
        """[piece][owner] -> (chunks, dir) exactly as they would travel, + a check of the packed form"""
        out, seen = [], []
        bounds = [(rel.numel() * c // pieces) & ~1 for c in range(pieces)] + [rel.numel()]
        for c in range(pieces):
            chunks, dirs, used = eng.shuffle_pack(rel[bounds[c]: bounds[c + 1]], None, nb_total, world)
            torch.cuda.synchronize()
            per_owner = []
            for r in range(world):
                assert chunks[r].numel() == used[r] * cb and dirs[r].numel() == used[r]
                per_owner.append((chunks[r], dirs[r]))
                if used[r] == 0:
                    continue
                keys, bucket, cnt = keymix.unpack_wire(chunks[r].cpu().numpy(), dirs[r].cpu().numpy(), f0)
                assert np.all((bucket * world) >> f0 == r) and np.all((cnt >= 1) & (cnt <= 256))
                assert np.array_equal((keymix.hash_w1(keys) >> np.uint32(32 - f0)).astype(np.int64), bucket)
                d = dirs[r].cpu().numpy().astype(np.int64)
                assert np.all(np.diff(d >> 9) >= 0)                                   # bucket after bucket
                assert np.unique((d >> 9)[(d & 0x1FF) < 256]).size == int(((d & 0x1FF) < 256).sum())   # dense: at most one partial chunk per bucket
                seen.append(keys)
            out.append(per_owner)
        assert np.array_equal(np.sort(np.concatenate(seen)), np.sort(rel.cpu().numpy().view(np.uint64)))      # a permutation of the rows
        return out

    bp, pp = pack_pieces(bk, bpieces), pack_pieces(pk, ppieces)
    total = 0
    for r in range(world):                                         # every owner in turn
        eng.stream_open_shuffled(nb_total, world, r, nb + 65536, bpieces, npk + 65536, ppieces)
        for c in range(bpieces):
            eng.stream_append_chunks(0, bp[c][r][0].clone(), bp[c][r][1].clone())
        for c in range(ppieces):
            eng.stream_append_chunks(1, pp[c][r][0].clone(), pp[c][r][1].clone())
        total += eng.stream_finish()
        lt = fj.last_timings()
        assert lt["fell_back"] == 0 and lt["passes"] >= 2
    assert total == exp


@pytest.mark.parametrize("world,nb_total,nb,npk", [(1, 40_000_000, 5_000_000, 30_000_000), (3, 300_000_000, 3_000_000, 20_000_000), (8, 300_000_000, 3_000_000, 20_000_000)])
def test_materialising_owner_shuffle_in_chunk_form_on_one_gpu(fj, world, nb_total, nb, npk):
    """_hash_join_radix_materialize (hash_join.cpp:315-381) across GPUs in the chunk form, all ranks played by one GPU: the build
    rows are packed WITH their values (256 per wire chunk), every owner opens its stream join with values, appends what the
    senders packed for it, counts (fj_stream_finish) and writes its pairs (fj_emit_pairs) - they stay with the owner.  Every pair
    is a probe key with its build value, the owners' pair sets add up to the closed-form count, and a pair sits with the owner of
    its key's first-pass bucket."""
    import torch
    import keymix
    from flash_hash_join_amd import datagen
    from flash_hash_join_amd.lab import LabEngine as HipEngine
    eng = HipEngine("cuda:0")
    f0 = eng.shuffle_plan(nb_total, world)
    bk, bv = datagen.build_device(nb, "cuda:0")
    pk, exp = datagen.probe_device(npk, nb, "cuda:0", seed=33, hit_bp=3000)
    bch, bdir, bused, bvals = eng.shuffle_pack(bk, bv, nb_total, world)
    pch, pdir, pused = eng.shuffle_pack(pk, None, nb_total, world)
    torch.cuda.synchronize()
    M = torch.tensor(-7046029254386353131, dtype=torch.int64, device="cuda:0")
    total = 0
    for r in range(world):
        assert bvals[r].numel() == bused[r] * 256
        eng.stream_open_shuffled(nb_total, world, r, bused[r] * 256 + 1024, 1, pused[r] * 256 + 1024, 1, with_vals=True)
        eng.stream_append_chunks(0, bch[r], bdir[r], bvals[r])
        eng.stream_append_chunks(1, pch[r], pdir[r])
        n = eng.stream_finish()
        k, v = eng.emit_pairs(n)
        assert k.numel() == n and bool(torch.all((v + 1) * M == k))              # (probe key, value of the build row with that key)
        if n:
            b = (keymix.hash_w1(k.cpu().numpy().view(np.uint64)) >> np.uint32(32 - f0)).astype(np.int64)
            assert np.all((b * world) >> f0 == r)                                 # pairs stay with the owner of their bucket
        total += n
    assert total == exp
    # duplicate build keys are refused in this form (first-occurrence semantics need the flat build arrays): an error, not a wrong pair
    dk = torch.cat([bk, bk[:1000]]); dv = torch.cat([bv, bv[:1000] + 7])
    dch, ddir, dused, dvals = eng.shuffle_pack(dk, dv, nb_total, 1)
    qch, qdir, qused = eng.shuffle_pack(pk, None, nb_total, 1)
    eng.stream_open_shuffled(nb_total, 1, 0, dused[0] * 256 + 1024, 1, qused[0] * 256 + 1024, 1, with_vals=True)
    eng.stream_append_chunks(0, dch[0], ddir[0], dvals[0])
    eng.stream_append_chunks(1, qch[0], qdir[0])
    with pytest.raises(RuntimeError, match="duplicate build keys"):
        eng.stream_finish()
    assert fj.hash_join_count_radix(bk, bv, pk)[0] == exp                         # the context serves other joins again


@pytest.mark.parametrize("nb_total,world", [(300_000_000, 8), (40_000_000, 3), (1_000_000_000, 64)])
def test_wire_format_edge_cases(fj, nb_total, world):
    """fj_shuffle_pack_* on ragged inputs: empty, one row, 255 / 256 / 257 rows, an odd count, every key equal (one bucket, one
    owner: exact region sizes mean skew cannot overflow anything), keys 0 and 2^64 - 1, and values riding along - what comes out,
    unpacked with the NumPy restatement of the wire format, is exactly the multiset that went in, every chunk with its owner."""
    import torch
    import keymix
    from flash_hash_join_amd.lab import LabEngine as HipEngine
    eng = HipEngine("cuda:0")
    f0 = eng.shuffle_plan(nb_total, world)
    rng = np.random.default_rng(11)
    cases = [np.empty(0, dtype=np.uint64), np.array([42], dtype=np.uint64), rng.integers(0, 2**63, 255, dtype=np.uint64),
             rng.integers(0, 2**63, 256, dtype=np.uint64), rng.integers(0, 2**63, 257, dtype=np.uint64),
             rng.integers(0, 2**63, 100_003, dtype=np.uint64) * np.uint64(2) + np.uint64(1),
             np.full(70_001, 0xDEADBEEFCAFEF00D, dtype=np.uint64),
             np.concatenate([np.array([0, 2**64 - 1, 1, 2**63], dtype=np.uint64), np.arange(5000, dtype=np.uint64) << np.uint64(32)])]
    for keys in cases:
        for with_vals in (False, True):
            tk = torch.from_numpy(keys.view(np.int64).copy()).cuda()
            tv = torch.from_numpy((keys * np.uint64(3) + np.uint64(1)).view(np.int64).copy()).cuda() if with_vals else None
            out = eng.shuffle_pack(tk, tv, nb_total, world)
            torch.cuda.synchronize()
            chunks, dirs, used = out[0], out[1], out[2]
            got_k, got_v = [], []
            for r in range(world):
                if used[r] == 0:
                    continue
                k, bucket, cnt = keymix.unpack_wire(chunks[r].cpu().numpy(), dirs[r].cpu().numpy(), f0)
                assert np.all((bucket * world) >> f0 == r)
                assert np.array_equal((keymix.hash_w1(k) >> np.uint32(32 - f0)).astype(np.int64), bucket)
                got_k.append(k)
                if with_vals:
                    v = out[3][r].cpu().numpy().view(np.uint64).reshape(-1, 256)
                    got_v.append(v[np.arange(256)[None, :] < cnt[:, None]])
            gk = np.concatenate(got_k) if got_k else np.empty(0, dtype=np.uint64)
            assert sum(used) == sum(-(-int(c) // 256) for c in np.bincount((keymix.hash_w1(keys) >> np.uint32(32 - f0)).astype(np.int64), minlength=1)) if keys.size else sum(used) == 0
            assert np.array_equal(np.sort(gk), np.sort(keys))
            if with_vals and keys.size:
                gv = np.concatenate(got_v)
                assert np.array_equal(gv, gk * np.uint64(3) + np.uint64(1))          # every value still sits next to its key


def test_c_host_example_runs(fj, tmp_path):
    """examples/host_join.c - a C99 program with nothing but include/flashjoin.h - joins 1M x 10M rows through fj_join_host."""
    import subprocess
    from conftest import ROOT
    from flash_hash_join_amd import _lib
    exe = str(tmp_path / "host_join")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "host_join.c"),
                           "-L" + os.path.dirname(_lib.LIB_PATH), "-lflashjoin_hip", "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "matches (expected" in out.stdout, out.stdout + out.stderr


def test_materialised_pairs_do_not_pin_the_probe_sized_buffers(fj):
    """The single-pass materialising join writes into buffers with room for ANY result (16 bytes per probe row); what it hands
    back must not keep them alive: at 30 % hits the returned tensors own exactly n rows."""
    import torch
    from flash_hash_join_amd import datagen
    bk, bv = datagen.build_device(2_000_000, "cuda:0")
    pk, exp = datagen.probe_device(20_000_000, 2_000_000, "cuda:0", seed=5, hit_bp=3000)
    n, _, k, v = fj.hash_join_radix(bk, bv, pk, return_arrays=True)
    assert n == exp and k.numel() == n and v.numel() == n
    assert k.untyped_storage().nbytes() == n * 8 and v.untyped_storage().nbytes() == n * 8
    M = torch.tensor(-7046029254386353131, dtype=torch.int64, device="cuda:0")
    assert bool(torch.all((v + 1) * M == k))


@pytest.mark.parametrize("top_bits", [64, 48])
@pytest.mark.parametrize("nb,npk,hit_bp", [(1, 1000, 5000), (3000, 200_000, 0), (1_000_000, 5_000_000, 500), (20_000_000, 30_000_000, 2500),
                                            (150_000_000, 40_000_000, 100)])
def test_sender_side_prefilter_keeps_every_hit(fj, nb, npk, hit_bp, top_bits):
    """fj_bloom_export + fj_bloom_prefilter (the owner shuffle's sender-side precheck): the survivors are a sub-multiset
    of the probe keys that contains every key of the build side, joining them gives the same count, and at low hit rates
    most misses are gone (filter load: nb / 512 keys in a 1.1 Mbit filter)."""
    import torch
    from flash_hash_join_amd import datagen, api
    from flash_hash_join_amd.lab import LabEngine as HipEngine
    bk, bv = datagen.build_device(nb, "cuda:0")
    pk, exp = datagen.probe_device(npk, nb, "cuda:0", seed=13, hit_bp=hit_bp)
    eng = HipEngine("cuda:0")
    filt = eng.bloom_export(bk, top_bits)
    assert filt.numel() == 512 * 35840 + 4                       # + header words (the variant the filters were built with)
    kept = eng.bloom_prefilter(pk, filt, top_bits)
    assert exp <= kept.numel() <= npk
    hit = torch.isin(pk, bk)
    assert int(hit.sum()) == exp
    ks, ps = torch.sort(kept)[0], torch.sort(pk)[0]
    assert torch.equal(torch.sort(pk[hit])[0], ks[torch.isin(ks, bk)])              # every hit survives, with its multiplicity
    uk, uc = torch.unique_consecutive(ks, return_counts=True)
    pu, pc = torch.unique_consecutive(ps, return_counts=True)
    at = torch.searchsorted(pu, uk)
    assert bool(torch.all(pu[at.clamp(max=pu.numel() - 1)] == uk)) and bool(torch.all(uc <= pc[at.clamp(max=pu.numel() - 1)]))   # nothing invented
    n, _ = api.join_device(api.ALGO_RADIX, 0, 0, bk, bv, kept.clone(), hash_top_bits=top_bits)
    assert n == exp
    misses_kept = kept.numel() - exp
    if nb <= 20_000_000:
        assert misses_kept <= 0.02 * (npk - exp) + 8                                 # <= 39k keys per 1.1 Mbit filter
    else:
        assert misses_kept <= 0.5 * (npk - exp)                                      # 293k keys per filter: past the good range, still useful
    # an empty build side exports all-zero filters: everything is rejected
    z = eng.bloom_export(bk[:0], top_bits)
    assert eng.bloom_prefilter(pk[:100_000], z, top_bits).numel() == 0


def test_sender_side_prefilter_refuses_filters_of_another_variant(fj):
    """Exporter and sender must set the same bits: filters carry the variant they were built with, and a sender configured
    for another one gets an error instead of silently dropping matching rows."""
    from flash_hash_join_amd import datagen
    from flash_hash_join_amd.lab import LabEngine as HipEngine
    bk, _ = datagen.build_device(2_000_000, "cuda:0")
    pk, _ = datagen.probe_device(1_000_000, 2_000_000, "cuda:0", seed=9, hit_bp=5000)
    eng = HipEngine("cuda:0")
    was = fj.get_option("bloom_variant")
    try:
        fj.set_option("bloom_variant", 0)
        filters = eng.bloom_export(bk, 64)
        assert eng.bloom_prefilter(pk, filters, 64).numel() >= 500_000 * 0.99
        fj.set_option("bloom_variant", 2)
        with pytest.raises(RuntimeError, match="bloom_variant"):
            eng.bloom_prefilter(pk, filters, 64)
        filters2 = eng.bloom_export(bk, 64)
        assert eng.bloom_prefilter(pk, filters2, 64).numel() >= 500_000 * 0.99
    finally:
        fj.set_option("bloom_variant", was)


@pytest.mark.parametrize("seed", range(8))
def test_sender_side_prefilter_on_random_key_distributions(fj, seed):
    """The precheck primitives on uniform, tiny-domain, sequential and sentinel-valued keys with duplicates on both sides:
    survivors = a sub-multiset of the probe rows that keeps every row whose key is in the build side."""
    import torch
    from flash_hash_join_amd.lab import LabEngine as HipEngine
    rng = np.random.default_rng(700 + seed)
    nb = int(rng.choice([1, 9, 4000, 70000, 900000]))
    npk = int(rng.choice([1, 2, 999, 65536, 1200001]))
    kind = seed % 4
    if kind == 0:
        dom = rng.integers(0, 1 << 64, max(2, nb + npk // 3), dtype=np.uint64)
    elif kind == 1:
        dom = rng.integers(0, 50, 40, dtype=np.uint64)
    elif kind == 2:
        dom = np.arange(1, max(3, 2 * nb), dtype=np.uint64)
    else:
        dom = np.concatenate([np.array([0, 1, (1 << 64) - 1, (1 << 63), (1 << 64) - 2], dtype=np.uint64), rng.integers(0, 1 << 64, nb + 5, dtype=np.uint64)])
    bk = dom[rng.integers(0, dom.size, nb)]
    other = rng.integers(0, 1 << 64, max(1, npk), dtype=np.uint64)
    pk = np.where(rng.random(npk) < 0.4, dom[rng.integers(0, dom.size, npk)], other[:npk])
    dbk, dpk = torch.from_numpy(bk.view(np.int64)).cuda(), torch.from_numpy(pk.view(np.int64)).cuda()
    eng = HipEngine("cuda:0")
    for top in (64, 48):
        kept = eng.bloom_prefilter(dpk, eng.bloom_export(dbk, top), top).cpu().numpy().view(np.uint64)
        hits = pk[np.isin(pk, bk)]
        assert np.array_equal(np.sort(kept[np.isin(kept, bk)]), np.sort(hits))            # every hit, with its multiplicity
        ku, kc = np.unique(kept, return_counts=True)
        pu, pc = np.unique(pk, return_counts=True)
        at = np.searchsorted(pu, ku)
        assert np.all(at < pu.size) and np.array_equal(pu[at], ku) and np.all(kc <= pc[at])    # nothing invented or multiplied


def test_distributed_protocol_on_one_rank_over_rccl(fj, monkeypatch):
    """The whole multi-GPU step on a 1-rank nccl group, both strategies: owner split -> RCCL all_to_all_single -> join
    with hash_top_bits=48 -> all_reduce, and all-gather of the build keys overlapped with the probe passes -> join ->
    all_reduce.  Exercises HipEngine and the collectives; the multi-rank logic itself is covered on CPU."""
    import socket
    import torch
    import torch.distributed as dist
    from flash_hash_join_amd import datagen
    from flash_hash_join_amd.distributed import distributed_join
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        import flash_hash_join_amd.distributed as D
        nb, npk = 3_000_000, 20_000_000
        bk, bv = datagen.build_device(nb, "cuda:0")
        pk, exp = datagen.probe_device(npk, nb, "cuda:0", seed=4, hit_bp=5000)
        M = torch.tensor(-7046029254386353131, dtype=torch.int64, device="cuda:0")
        dj = lambda *a, **kw: distributed_join(*a, force_exchange=True, **kw)        # the full protocol on this one rank
        for strategy, via in (("shuffle", "rccl"), ("shuffle", "python"), ("scatter", "rccl"), ("broadcast", "rccl"), ("broadcast", "python")):
            monkeypatch.setenv("FJ_DIST_STRATEGY", strategy)
            monkeypatch.setenv("FJ_DIST_NATIVE", "0" if via == "python" else "1")            # the same driver over callbacks into torch.distributed instead of RCCL directly
            t = {}
            n, sec = dj(bk, bv, pk, timings=t)
            assert n == exp and t["strategy"] == strategy, t
            if strategy == "broadcast":                    # the build-broadcast form on a 1-rank communicator: pack -> (no peer) -> probe passes -> 4 range joins
                assert t["shuffle_form"].startswith("build broadcast") and t["pieces"] == 4 and t["local_count"] == exp and t["wire_bytes_sent"] == 0, t
            if strategy == "shuffle":
                form = {"rccl": "chunks (fj_dist_join over RCCL)", "python": "chunks (fj_dist_join over a callback transport)"}[via]
                assert t["shuffle_form"] == form and t["pieces"] == 4 and t["local_count"] == exp and "chunk_form_error" not in t
                assert t["wire_chunk_bytes"] == 2048          # (a 3M-row build side: 5 + 5 bits, whole keys on the wire)
            if strategy == "scatter":
                assert t["shuffle_form"] == "owner-scatter" and t["local_count"] == exp
            if t.get("rows_are_chunk_capacity"):        # the native entry reports received chunks x 256 (partial chunks counted whole)
                assert npk <= t["local_probe_rows"] <= 1.3 * npk and nb <= t["local_build_rows"] <= 1.3 * nb
            else:
                assert t["local_probe_rows"] == npk and t["local_build_rows"] == nb
            tm = {}
            n, sec, k, v = dj(bk, bv, pk, materialize=True, return_arrays=True, timings=tm)
            assert n == exp and k.numel() == exp
            assert bool(torch.all((v + 1) * M == k))
            assert tm["strategy"] == strategy, tm       # materialising joins take every form too (broadcast: the values travel as a fourth part, the pairs stay with the probe rows)
        # duplicate build keys in the broadcast form (round 5's table failed the whole step from 52 copies of one key on):
        # a copy takes a slot of its own in the bucketed table, a lookup stops at the first match - 60 and 200 copies of two keys join
        # in the broadcast form itself, exactly
        monkeypatch.setenv("FJ_DIST_STRATEGY", "broadcast"); monkeypatch.setenv("FJ_DIST_NATIVE", "1")
        dk = torch.cat([bk, bk[777:778].repeat(60), bk[4242:4243].repeat(200)]); dv = torch.cat([bv, bv[777:778].repeat(60), bv[4242:4243].repeat(200)])
        t = {}
        n, sec = dj(dk, dv, pk, timings=t)
        assert n == exp and t["strategy"] == "broadcast" and "broadcast_form_error" not in t, t
        # ... materialising too: one pair per matching probe row, whatever the number of copies (round 6: the step is counted by the same kernel)
        tm = {}
        n, sec, k, v = dj(dk, dv, pk, materialize=True, return_arrays=True, timings=tm)
        assert n == exp == k.numel() and tm["strategy"] == "broadcast" and "broadcast_form_error" not in tm and bool(torch.all((v + 1) * M == k)), tm
        del k, v
        # ... and one key repeated 20000 times: its final partition does not fit the LDS table (that form has no per-partition
        # recovery) - the step fails on every rank alike and moves down the ladder to the shuffle, whose skew ladder takes it
        hot = bk[12345:12346].repeat(20000)
        sbk2, sbv2 = torch.cat([bk, hot]), torch.cat([bv, bv[12345:12346].repeat(20000)])
        t = {}
        n, sec = dj(sbk2, sbv2, pk, timings=t)
        assert n == exp and t["strategy"] == "shuffle" and "does not fit the LDS table" in t["broadcast_form_error"], t
        t = {}
        n, sec = dj(bk, bv, pk, timings=t)                                 # ... and the next plain join broadcasts again (a pinned strategy remembers nothing)
        assert n == exp and t["strategy"] == "broadcast" and "broadcast_form_error" not in t, t
        # under "auto" the failed rung is remembered for the shape: the second step of the skewed join goes straight to the shuffle
        monkeypatch.setenv("FJ_DIST_STRATEGY", "auto")
        D._FORM_MEMO.clear()
        monkeypatch.setattr(D, "form_model", lambda *a, **kw: {"pick": "broadcast"})      # (one rank: the model would never broadcast)
        for step in range(2):
            t = {}
            n, sec = dj(sbk2, sbv2, pk, timings=t, join_id="skewed")
            assert n == exp and t["strategy"] == "shuffle" and ("broadcast_form_error" in t) == (step == 0), (step, t)
        D._FORM_MEMO.clear()
        monkeypatch.undo(); monkeypatch.setenv("FJ_DIST_NATIVE", "1")
        # sender-side bloom precheck of the probe exchange in chunk form (per-partition filters: fj_stream_export_part_filters ->
        # all-gather -> fj_shuffle_pack_filter, inside the driver); the owner-scatter rung has none of its own
        monkeypatch.setenv("FJ_DIST_STRATEGY", "shuffle")
        lpk, lexp = datagen.probe_device(npk, nb, "cuda:0", seed=9, hit_bp=500)
        for pre in ("1", "0"):
            monkeypatch.setenv("FJ_DIST_PREFILTER", pre)
            t = {}
            n, sec = dj(bk, bv, lpk, timings=t)
            assert n == lexp and t["prefilter"] == (pre == "1") and t["shuffle_form"].startswith("chunks"), t
            assert t["probe_rows_sent"] == npk if pre == "0" else lexp <= t["probe_rows_sent"] < 0.08 * npk
            tm = {}
            n, sec, k, v = dj(bk, bv, lpk, materialize=True, return_arrays=True, timings=tm)      # materialising: the same precheck
            assert n == lexp and k.numel() == lexp and bool(torch.all((v + 1) * M == k))
            assert tm["prefilter"] == (pre == "1") and tm["probe_rows_sent"] == t["probe_rows_sent"] and tm["shuffle_form"].startswith("chunks"), tm
        n, sec = dj(bk, bv, lpk, bloom=True, timings=t)       # FJ_DIST_PREFILTER=0 overrides the bloom argument
        assert n == lexp and not t["prefilter"]
        n, sec = dj(bk, bv, lpk, bloom=True, timings=t, prefilter="on")       # ... and an explicit argument overrides the environment
        assert n == lexp and t["prefilter"]
        monkeypatch.delenv("FJ_DIST_PREFILTER")
        n, sec = dj(bk, bv, lpk, bloom=True, timings=t)       # the *_bloom meaning of the multi-GPU join: "auto"
        assert n == lexp and t["prefilter_mode"] == "auto"
        assert not t["prefilter"], t      # (a 20M-row probe side does not pay for the filters' fixed cost on one rank: nothing is exported or sampled)
        monkeypatch.setenv("FJ_DIST_STRATEGY", "scatter")
        n, sec = dj(bk, bv, lpk, bloom=True, timings=t)
        assert n == lexp and t["prefilter"] is False and t["shuffle_form"] == "owner-scatter"
        # a build side whose keys all land in ONE partition of the owner's plan: the shuffle's owner re-partitions that partition alone
        def hash_w1(kk):
            lo = (kk & np.uint64(0xFFFFFFFF)).astype(np.uint32); hi = (kk >> np.uint64(32)).astype(np.uint32)
            with np.errstate(over="ignore"):
                x = (lo * np.uint32(0x9E3779B1)) ^ (hi * np.uint32(0x85EBCA77))
                x ^= x >> np.uint32(16); x *= np.uint32(0x85ebca6b)
                x ^= x >> np.uint32(13); x *= np.uint32(0xc2b2ae35)
                x ^= x >> np.uint32(16)
            return x
        cand = np.arange(1, 400000, dtype=np.uint64)
        skew = cand[(hash_w1(cand) >> np.uint32(27)) == 0][:9000]
        sbk = torch.from_numpy(skew.view(np.int64)).cuda(); sbv = sbk + 1
        spk = torch.from_numpy(np.concatenate([skew, cand[:50000]]).view(np.int64)).cuda()
        sexp = int(np.isin(np.concatenate([skew, cand[:50000]]), skew).sum())
        for strategy in ("auto", "shuffle", "scatter"):
            monkeypatch.setenv("FJ_DIST_STRATEGY", strategy)
            n, sec = dj(sbk, sbv, spk)
            assert n == sexp
        # messages capped at 1M rows: the owner-scatter rung moves every segment in several rounds (list all_to_all on views: the
        # workaround for RCCL's > 4 GiB-per-peer defect)
        monkeypatch.setattr(D, "_MAX_ELEMS_PER_MESSAGE", 1 << 20)
        monkeypatch.setenv("FJ_DIST_STRATEGY", "scatter")
        t = {}
        n, sec = dj(bk, bv, pk, timings=t)
        assert n == exp and t["exchange_rounds"] > 1
        n, sec, k, v = dj(bk, bv, pk, materialize=True, return_arrays=True)
        assert n == exp and k.numel() == exp and bool(torch.all((v + 1) * M == k))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_multi_rank_join_with_ranks_sharing_this_gpu(fj, world):
    """The multi-GPU step under genuine multi-rank control flow with the real HipEngine: `world` processes share this
    GPU and talk over gloo (RCCL refuses two ranks on one device; the collectives are staged through the host, nothing
    else differs from the production path).  Both strategies, counting and materialising, uneven shards at world 3."""
    import subprocess
    import sys
    from conftest import ROOT
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "two_ranks_one_gpu.py"), str(world)],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert f"OK: {world} ranks on one GPU" in out.stdout


def test_bench_multi_rank_branch_with_ranks_sharing_this_gpu(fj):
    """bench.py's N>1 branch (per-rank generation, barrier, max over ranks, one JSON line from rank 0) launched the way
    the driver launches it, with two ranks on this one GPU (FJ_BENCH_SHARE_GPU: gloo, host-staged collectives)."""
    import socket
    import subprocess
    import sys
    from conftest import ROOT
    s_ = socket.socket(); s_.bind(("127.0.0.1", 0)); port = s_.getsockname()[1]; s_.close()
    from conftest import product_env
    env = product_env(FJ_BENCH_SHARE_GPU="1")               # (the bench runs on the PRODUCT library)
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--scale", "0.02", "--steps", "2",
                          "--warmup", "1", "--full"], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                                   # exactly one JSON line, from rank 0
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["config"]["probe_rows_total"] == 2 * 25_000_000     # default at N > 1: c5 (x 0.02)
    assert d["config"]["bench_workload"] == "c5" and d["config"]["build_rows_total"] == 2 * 2_500_000
    assert d["config"]["parallelism"].endswith("x2") and d["value"] > 0
    # the N > 1 line is complete: the CPU baseline (rank 0, the config-3-size run, labelled), the timed form's
    # roofline, the model's verdict, and the OTHER form as a labelled second measurement with a roofline block and wire bytes of its own
    cb = d["cpu_baseline"]
    assert cb["value"] > 0 and cb["kind"] == "port" and cb["cores"] >= 1 and cb["sample"].startswith("config-3-size run on rank 0's host cores"), cb
    # the pre-flight self-check ran (under the host-staged transport only the torch.distributed forms apply) and is in the line;
    # value is the form the driver's cost model picks for these sizes (10 probe rows per build row: the build broadcast), checked
    # before it is timed; the other form rides along as a labelled second measurement
    assert d["self_check"]["ok"] and d["self_check"]["forms_tried"][-1]["ok"]
    assert d["phases"]["form_model"]["pick"] == "broadcast" and d["phases"]["strategy_timed"] == "broadcast", d["phases"]
    assert d["config"]["parallelism"].startswith("build-broadcast") and d["phases"]["shuffle_form"].startswith("build broadcast")
    assert d["roofline"]["kernel"].startswith("fj_partition_kernel<keys> (a probe-side radix pass") and 0 < d["roofline"]["frac"] < 1
    alt = d["alt_strategy"]
    assert alt["strategy"] == "owner-shuffle" and alt["count_ok"] is True and alt["form"].startswith("chunks") and alt["fell_to"] is None and alt["errors"] is None, alt
    assert alt["roofline"]["kernel"].startswith("fj_partition_kernel<keys-only> (the owner's radix pass") and 0 < alt["roofline"]["frac"] < 1 and alt["roofline"]["bytes_per_unit"] in (15.0, 16.0), alt
    assert alt["wire_bytes_sent_rank0"] > 0 and alt["wire_chunk_bytes"] in (1792, 2048) and alt["value"] > 0, alt
    assert d["phases"]["wire_bytes_sent_rank0"] > 0 and d["phases"]["form_model"]["shuffle"] > 0 and d["phases"]["form_model"]["broadcast"] > 0
    # ... and a pinned strategy is what gets timed
    s_ = socket.socket(); s_.bind(("127.0.0.1", 0)); port = s_.getsockname()[1]; s_.close()
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--scale", "0.02", "--steps", "2",
                          "--warmup", "1", "--full"], capture_output=True, text=True, timeout=900, env=dict(env, FJ_DIST_STRATEGY="shuffle"), cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert d["config"]["parallelism"].startswith("owner-shuffle") and d["phases"]["shuffle_form"].startswith("chunks (fj_dist_join over a callback transport")
    assert d["alt_strategy"]["strategy"] == "build-broadcast" and d["alt_strategy"]["count_ok"] is True and 0 < d["alt_strategy"]["roofline"]["frac"] < 1 and "cpu_baseline" in d
    # a transport that moves wrong data (test hook): every shuffle form fails its check, ONE JSON line says so, exit code 3
    s_ = socket.socket(); s_.bind(("127.0.0.1", 0)); port = s_.getsockname()[1]; s_.close()
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--scale", "0.02", "--steps", "2",
                          "--warmup", "1", "--selfcheck-corrupt"], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert out.returncode != 0
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["value"] is None and "elements received from rank" in d["error"] and d["n_gpus"] == 2
    assert [f["ok"] for f in d["self_check"]["forms_tried"]] == [False] * len(d["self_check"]["forms_tried"]) and len(d["self_check"]["forms_tried"]) >= 2


def test_shuffled_stream_recovers_from_an_oversized_partition(fj):
    """The chunk form of the owner shuffle on one GPU (one owner, world 1) with a build side that puts 9000 keys into ONE final
    partition: fj_stream_finish re-partitions that partition alone (no fallback exists for chunk pieces) - exact count."""
    import torch
    from flash_hash_join_amd import datagen
    from flash_hash_join_amd.lab import LabEngine as HipEngine
    def hash_w1(k):                                                # fj_hash_w1 of csrc/fj_common.h
        lo = (k & np.uint64(0xFFFFFFFF)).astype(np.uint32); hi = (k >> np.uint64(32)).astype(np.uint32)
        with np.errstate(over="ignore"):
            x = (lo * np.uint32(0x9E3779B1)) ^ (hi * np.uint32(0x85EBCA77))
            x ^= x >> np.uint32(16); x *= np.uint32(0x85ebca6b)
            x ^= x >> np.uint32(13); x *= np.uint32(0xc2b2ae35)
            x ^= x >> np.uint32(16)
        return x
    nb_total = 3_000_000                                           # plan: 10 bits = 5 + 5
    cand = np.arange(1, 40_000_000, dtype=np.uint64)
    skew = cand[(hash_w1(cand) >> np.uint32(22)) == 77][:9000]     # top 10 hash bits equal: one final partition
    assert skew.size == 9000
    bk0, _ = datagen.build_device(nb_total - 9000, "cuda:0")
    bk = torch.cat([bk0, torch.from_numpy(skew.view(np.int64)).cuda()])
    pk0, exp0 = datagen.probe_device(8_000_000, nb_total - 9000, "cuda:0", seed=2, hit_bp=5000)
    pk = torch.cat([pk0, torch.from_numpy(np.tile(skew, 5).view(np.int64)).cuda()])
    assert not bool(torch.isin(bk[-9000:], bk0).any())
    eng = HipEngine("cuda:0")
    assert eng.shuffle_plan(nb_total, 1) == 5
    bch, bdir, _ = eng.shuffle_pack(bk, None, nb_total, 1)
    pch, pdir, _ = eng.shuffle_pack(pk, None, nb_total, 1)
    eng.stream_open_shuffled(nb_total, 1, 0, bk.numel() + 65536, 1, pk.numel() + 65536, 1)
    eng.stream_append_chunks(0, bch[0], bdir[0])
    eng.stream_append_chunks(1, pch[0], pdir[0])
    assert eng.stream_finish() == exp0 + 45_000
    lt = fj.last_timings()
    assert lt["fell_back"] == 0 and lt["lds_retries"] == 2, lt


@pytest.mark.parametrize("nb,npk,hit_bp,fn,hbm", [
    (1_000_000, 100_000_000, 5000, "hash_join_count", 0),            # BASELINE config 2
    (1_000_000, 100_000_000, 5000, "hash_join_count", 1),            # ... with the literal one-table algorithm
    (1_000_000, 100_000_000, 5000, "hash_join_count_radix", 0),
    (100_000_000, 1_000_000_000, 5000, "hash_join_count_radix", 0),  # BASELINE config 3
    (100_000_000, 1_000_000_000, 500, "hash_join_count_radix_bloom", 0),   # BASELINE config 4 (radix form)
    (100_000_000, 1_000_000_000, 500, "hash_join_count_bloom", 0),         # BASELINE config 4 as named
    (100_000_000, 1_000_000_000, 500, "hash_join_count_bloom", 1),         # ... non-partitioned HBM table + bloom precheck
    (1_000_000, 10_000_000, 5000, "adaptive_join_count", 0),               # BASELINE config 1 sizes on the device
    (1_000_000, 10_000_000, 5000, "hash_join_count", 0),                   # ... and through the function config 1 names ("flash_join scalar path")
    (1_000_000, 10_000_000, 5000, "hash_join_count", 1),                   # ... literally: one table, linear probing
    (300_000_000, 300_000_000, 5000, "hash_join_count_radix", 0),          # 17 radix bits: an 8-bit and a 9-bit pass
    (800_000_000, 200_000_000, 5000, "hash_join_count_radix", 0),          # 18 bits (9 + 9): the replicated build side of 8 GPUs
    (50_000_000, 3_900_000_000, 2500, "hash_join_count_radix", 0),         # probe side close to the 2^24-chunk directory limit (~4.0e9 rows)
    (3_000, 2_500_000_000, 7000, "hash_join_count", 0),                    # zero-pass plan over > 2^31 probe rows
])
def test_full_size_closed_form_counts(fj, nb, npk, hit_bp, fn, hbm):
    """BASELINE.json's full sizes, checked through the size-independent property of the generator:
    the match count equals the number of generated hits."""
    import torch
    from flash_hash_join_amd import datagen
    fj.set_option("scalar_hbm_table", hbm)
    dbk, dbv = datagen.build_device(nb, "cuda:0")
    dpk, exp = datagen.probe_device(npk, nb, "cuda:0", seed=1, hit_bp=hit_bp)
    assert abs(exp - npk * hit_bp / 10000) < 6 * (npk ** 0.5)
    n, sec = getattr(fj, fn)(dbk, dbv, dpk)
    assert n == exp
    n2, _ = getattr(fj, fn)(dbk, dbv, dpk)                                         # idempotent, workspace reuse
    assert n2 == exp
    assert fj.last_timings()["path"] == (1 if hbm else 0)
    if "bloom" in fn and not hbm and nb >= 100_000_000:                           # config 4: the precheck ran and pruned the misses
        t = fj.last_timings()
        assert t["bloom_level"] == 1 and exp <= t["filter_survivors"] <= exp + 0.2 * (npk - exp), t
    fj.set_option("scalar_hbm_table", 0)
    del dbk, dbv, dpk
    torch.cuda.empty_cache()


@pytest.mark.parametrize("nb,bits", [(100_000, 13), (6_000_000, 19), (12_000_000, 20)])
def test_level_bookkeeping_at_the_bucket_counts_where_its_scan_changes_form(fj, nb, bits):
    """After a pass the per-bucket chunk counts become chunk-list offsets: one workgroup up to 4096 buckets, one workgroup per 4096
    buckets from 8192 to 2^19 (fj_level_scan_wide, the counts then cleared by the chunk-list launch), one workgroup again beyond.
    16 build keys per final partition put small relations on 2^13, 2^19 and 2^20 final buckets; every join runs twice (the counts
    must be zero again for the second) and the match count is the generator's closed form."""
    import torch
    from flash_hash_join_amd import datagen
    fj.set_option("plan_target_keys", 16)
    try:
        dbk, dbv = datagen.build_device(nb, "cuda:0")
        dpk, exp = datagen.probe_device(3 * nb + 17, nb, "cuda:0", seed=bits, hit_bp=4000)
        for _ in range(2):
            n, _sec = fj.hash_join_count_radix(dbk, dbv, dpk)
            assert n == exp
            assert fj.last_timings()["radix_bits"] == bits
        n, _sec, k, v = fj.hash_join_radix(dbk, dbv, dpk, return_arrays=True)
        assert n == exp and k.numel() == exp and v.numel() == exp
    finally:
        fj.set_option("plan_target_keys", 4096)
    del dbk, dbv, dpk
    torch.cuda.empty_cache()


@pytest.mark.parametrize("hit_bp", [0, 500, 5000, 10000])
@pytest.mark.parametrize("nb,npk", [(5_000_000, 40_000_000), (30_000_000, 60_000_000)])
def test_bloom_precheck_prunes_misses_and_keeps_every_hit(fj, nb, npk, hit_bp):
    """The *_bloom functions run a bloom precheck between the probe side's two partition passes (an LDS-resident filter per
    level-1 bucket, built from the build side's same bucket): counts stay exact at 0 / 5 / 50 / 100 % hits (no false
    negatives), the keys that pass are the hits plus a bounded share of the misses, and the non-bloom functions do not
    run it (role of hash_join.cpp:165, :183-189)."""
    import torch
    from flash_hash_join_amd import datagen
    dbk, dbv = datagen.build_device(nb, "cuda:0")
    dpk, exp = datagen.probe_device(npk, nb, "cuda:0", seed=21, hit_bp=hit_bp)
    assert fj.hash_join_count_radix(dbk, dbv, dpk)[0] == exp
    assert fj.last_timings()["bloom_level"] == 0
    for fn in ("hash_join_count_radix_bloom", "hash_join_count_bloom"):
        n, _ = getattr(fj, fn)(dbk, dbv, dpk)
        t = fj.last_timings()
        assert n == exp, (fn, hit_bp)
        assert t["bloom_level"] == 1 and t["passes"] == 2 and t["fell_back"] == 0 and t["sampled_hit_bp"] == -1, (fn, t)
        assert exp <= t["filter_survivors"] <= exp + 0.25 * (npk - exp) + 1000, (fn, hit_bp, t["filter_survivors"], exp)
    # the adaptive functions (either name) decide from a sample of 4096 probe rows where a precheck could pay (a probe side of
    # >= 4x the build side): on up to 25 % sampled hits
    for fn in ("adaptive_join_count", "adaptive_join_count_bloom"):
        n, _ = getattr(fj, fn)(dbk, dbv, dpk)
        t = fj.last_timings()
        assert n == exp and t["fell_back"] == 0, (fn, hit_bp)
        if npk >= 4 * nb:
            assert abs(t["sampled_hit_bp"] - hit_bp) <= 350, (fn, t["sampled_hit_bp"], hit_bp)
            assert t["bloom_level"] == (1 if t["sampled_hit_bp"] <= fj.get_option("bloom_auto_max_hit_bp") else 0), (fn, t)
        else:
            assert t["sampled_hit_bp"] == -1 and t["bloom_level"] == 0, (fn, t)
    fj.set_option("bloom_auto", 0)                      # as named: adaptive_*_bloom filter, adaptive_* do not
    try:
        assert fj.adaptive_join_count_bloom(dbk, dbv, dpk)[0] == exp and fj.last_timings()["bloom_level"] == 1
        assert fj.adaptive_join_count(dbk, dbv, dpk)[0] == exp and fj.last_timings()["bloom_level"] == 0
    finally:
        fj.set_option("bloom_auto", 1)
    n, _, k, v = fj.hash_join_radix_bloom(dbk, dbv, dpk, return_arrays=True)
    assert n == exp and k.numel() == exp and fj.last_timings()["bloom_level"] == 1
    M = torch.tensor(-7046029254386353131, dtype=torch.int64, device="cuda:0")
    assert bool(torch.all((v + 1) * M == k))
    del dbk, dbv, dpk, k, v
    torch.cuda.empty_cache()


def test_config5_every_owner_shard_at_full_size_on_one_gpu(fj):
    """BASELINE configs[4] (flash_join_radix, 1B build x 10B probe rows over 8 GPUs) at FULL size on this one GPU: for each
    of the 8 owners in turn, the 8 ranks' blocks (125M x 1.25B rows each, generated like bench.py generates them) are split
    by owner (fj_owner_hist / fj_owner_scatter, nranks = 8), the owner's 8 build segments and 8 probe segments - what the
    all-to-all would deliver - are joined with fj_stream_begin / fj_stream_append_probe / fj_stream_finish at
    hash_top_bits = 48, and the 8 owners' counts add up to the closed-form count of the whole 1B x 10B join."""
    import torch
    from flash_hash_join_amd import datagen, api
    from flash_hash_join_amd.lab import LabEngine as HipEngine
    world, nb_rank, np_rank = 8, 125_000_000, 1_250_000_000
    nb_total = nb_rank * world
    eng = HipEngine("cuda:0")
    expected = None
    owner_counts, owner_build_rows, owner_probe_rows = [], [], []
    for o in range(world):
        bks, bvs, pks, exp_sum = [], [], [], 0
        for r in range(world):
            bk, bv = datagen.build_device(nb_rank, "cuda:0", first=r * nb_rank)
            ks, vs, bc = eng.owner_split(bk, bv, world)
            lo = sum(bc[:o])
            bks.append(ks[lo: lo + bc[o]].clone()); bvs.append(vs[lo: lo + bc[o]].clone())
            del bk, bv, ks, vs
            pk, e = datagen.probe_device(np_rank, nb_total, "cuda:0", seed=1, hit_bp=5000, first=r * np_rank)
            exp_sum += e
            pc = eng.owner_hist(pk, world)
            ps = eng.owner_scatter(pk, world, pc)
            lo = sum(pc[:o])
            pks.append(ps[lo: lo + pc[o]].clone())
            del pk, ps
        if expected is None:
            expected = exp_sum
            assert abs(expected - 0.5 * np_rank * world) < 6 * (np_rank * world) ** 0.5
        assert exp_sum == expected
        bk_o, bv_o = torch.cat(bks), torch.cat(bvs)
        del bks, bvs
        np_o = sum(p.numel() for p in pks)
        assert abs(bk_o.numel() - nb_rank) < 0.01 * nb_rank and abs(np_o - np_rank) < 0.01 * np_rank      # uniform keys: balanced owners
        eng.stream_begin(bk_o, bv_o, np_o, world, 48)
        for p in pks:
            eng.stream_append(p)
        n = eng.stream_finish()
        t = fj.last_timings()
        assert t["path"] == 0 and t["fell_back"] == 0 and t["passes"] == 2
        if o == 0:                                   # the one-shot join of the same shard agrees with the streamed one
            n1, _ = api.join_device(api.ALGO_RADIX, 0, 0, bk_o, bv_o, torch.cat(pks), hash_top_bits=48)
            assert n1 == n
        owner_counts.append(n); owner_build_rows.append(bk_o.numel()); owner_probe_rows.append(np_o)
        del bk_o, bv_o, pks
        torch.cuda.empty_cache()
    assert sum(owner_build_rows) == nb_total and sum(owner_probe_rows) == np_rank * world
    assert sum(owner_counts) == expected, (owner_counts, expected)


def test_config5_chunk_form_every_owner_at_full_size_on_one_gpu(fj):
    """BASELINE configs[4] (1B build x 10B probe rows over 8 GPUs) at FULL size in the form the multi-GPU bench runs (the chunk
    form of the owner shuffle, csrc/fj_dist.hip), all 8 ranks played by this one GPU: every sender's block (125M x 1.25B rows,
    generated like bench.py generates them) is packed once (fj_shuffle_pack_begin / _counts / _finish: first pass of the plan for
    1B build rows = 512 buckets, dense 7-byte chunks) and its 8 shares are kept in HBM exactly as they would travel (~77 GB in
    all); then every owner appends its 8 + 8 shares (fj_stream_open_shuffled / append_*_chunks: the 9-bit second pass reads the
    wire format) and joins.  The owners' counts add up to the closed-form count of the whole join; the wire carries 7.0x bytes
    per key."""
    import torch
    from flash_hash_join_amd import datagen
    from flash_hash_join_amd.lab import LabEngine as HipEngine
    world, nb_rank, np_rank = 8, 125_000_000, 1_250_000_000
    nb_total = nb_rank * world
    eng = HipEngine("cuda:0")
    assert eng.shuffle_plan(nb_total, world) == 9 and eng.shuffle_chunk_bytes(nb_total, world) == 1792
    bshare, pshare, expected = [], [], 0
    wire_bytes = 0
    for r in range(world):                                          # every sender packs its block once
        bk, _ = datagen.build_device(nb_rank, "cuda:0", first=r * nb_rank)
        ch, dw, used = eng.shuffle_pack(bk, None, nb_total, world)
        torch.cuda.synchronize()
        bshare.append([(c.clone(), d.clone()) for c, d in zip(ch, dw)])
        del bk, ch, dw
        pk, e = datagen.probe_device(np_rank, nb_total, "cuda:0", seed=1, hit_bp=5000, first=r * np_rank)
        expected += e
        ch, dw, used = eng.shuffle_pack(pk, None, nb_total, world)
        torch.cuda.synchronize()
        pshare.append([(c.clone(), d.clone()) for c, d in zip(ch, dw)])
        wire_bytes += sum(c.numel() + 4 * d.numel() for c, d in zip(ch, dw))
        assert abs(sum(used) * 256 - np_rank) < 512 * 256 + 1       # dense: one partial chunk per bucket at most
        assert max(used) < 1.01 * np_rank / world / 256 + 64        # uniform keys: balanced owners
        del pk, ch, dw
        torch.cuda.empty_cache()
    assert abs(expected - 0.5 * np_rank * world) < 6 * (np_rank * world) ** 0.5
    per_key = wire_bytes / (np_rank * world)
    assert 7.0 < per_key < 7.03, per_key                            # 7 bytes + a directory word per 256 keys + the partial chunks
    total = 0
    for o in range(world):                                          # every owner joins what it would have received
        nbc = sum(bshare[r][o][1].numel() for r in range(world)); npc = sum(pshare[r][o][1].numel() for r in range(world))
        eng.stream_open_shuffled(nb_total, world, o, nbc * 256, world, npc * 256, world)
        for r in range(world):
            eng.stream_append_chunks(0, bshare[r][o][0], bshare[r][o][1])
        for r in range(world):
            eng.stream_append_chunks(1, pshare[r][o][0], pshare[r][o][1])
        total += eng.stream_finish()
        t = fj.last_timings()
        assert t["path"] == 0 and t["fell_back"] == 0 and t["passes"] == 2
    assert total == expected, (total, expected)


def _bcast_emulated(eng, world, bks, pks, nb_total, pieces):
    """All ranks of a build-broadcast join on one GPU: every rank's build block packed into its region, then every rank's probe
    block joined against all regions, range by range.  Returns the sum of the ranks' counts."""
    import torch
    sizes = [int(b.numel()) for b in bks]
    rbs = [eng.bcast_region_bytes(nb_total, n) for n in sizes]
    offs = [sum(rbs[:r]) for r in range(world)]
    base = torch.empty(sum(rbs), dtype=torch.uint8, device="cuda:0")
    bits, nparts, _ = eng.bcast_plan(nb_total)
    empty = torch.empty(16, dtype=torch.int64, device="cuda:0")[:0]
    for r in range(world):
        eng.bcast_pack(bks[r], nb_total, base[offs[r]: offs[r] + rbs[r]], pieces)
        b = eng.bcast_pack_bounds(pieces)
        assert b[0] == 0 and b[-1] == sizes[r] and all(x <= y for x, y in zip(b, b[1:]))
        eng.bcast_probe(empty, nb_total)
        assert eng.bcast_finish() == 0
    total = 0
    for r in range(world):
        eng.bcast_pack(bks[r], nb_total, base[offs[r]: offs[r] + rbs[r]], pieces)      # (a step starts with the rank's own pack)
        eng.bcast_probe(pks[r], nb_total)
        for q in range(pieces):
            eng.bcast_join(base, offs, sizes, nparts * q // pieces, nparts * (q + 1) // pieces)
        total += eng.bcast_finish()
    return total


@pytest.mark.parametrize("world,nb_total,np_total,target", [(2, 70_000, 300_001, 32), (3, 250_000, 1_000_000, 32), (8, 9_000_000, 12_000_000, 4096),
                                                              (4, 40_000, 90_000, 256), (5, 3_000_000, 2_000_000, 32),
                                                              (2, 20_000, 9_000_000, 4096), (3, 400_000, 9_000_001, 4096), (4, 2_000_000, 30_000_000, 4096)])
def test_build_broadcast_form_matches_the_oracle(fj, oracle, world, nb_total, np_total, target):
    """The build-broadcast form of the multi-GPU join (csrc/fj_bcast.hip + fj_count_join_wide<DENSE>), all ranks played by this GPU,
    against the NumPy oracle: ragged blocks (one rank holds no build rows, one no probe rows), repeated probe keys, both widths of the
    high-word plane (bits < 16 / >= 16 under plan_target_keys), 1..5 pieces.  The last three: few, fat partitions whose probe side is
    cut into 18 / 3 / 2 items each - dealt to the workgroups in runs, a partition's table built once per run (FjWideArgs::group_log)."""
    import torch
    from flash_hash_join_amd.lab import LabEngine as HipEngine
    fj.set_option("plan_target_keys", target)
    try:
        eng = HipEngine("cuda:0")
        rng = np.random.default_rng(world * 1000 + nb_total % 97)
        bk = np.unique(rng.integers(0, 2**64, size=nb_total, dtype=np.uint64))
        pk = np.concatenate([rng.choice(bk, np_total // 2), rng.integers(0, 2**64, size=np_total - np_total // 2, dtype=np.uint64)])
        rng.shuffle(pk)
        exp = oracle.np_join(bk, bk, pk)
        assert eng.bcast_plan(bk.size) is not None
        cutb = sorted(rng.integers(0, bk.size, size=world - 1).tolist()); cutb[0] = 0            # rank 0: no build rows
        cutp = sorted(rng.integers(0, pk.size, size=world - 1).tolist()); cutp[-1] = pk.size      # last rank: no probe rows
        bks = [torch.from_numpy(x.view(np.int64).copy()).cuda() for x in np.split(bk, cutb)]
        pks = [torch.from_numpy(x.view(np.int64).copy()).cuda() for x in np.split(pk, cutp)]
        for pieces in (1, 1 + world % 5):
            assert _bcast_emulated(eng, world, bks, pks, int(bk.size), pieces) == exp
    finally:
        fj.set_option("plan_target_keys", 4096)


@pytest.mark.parametrize("world,nb_total,np_total,target", [(2, 70_000, 300_001, 32), (3, 250_000, 1_000_000, 32), (8, 9_000_000, 12_000_000, 4096),
                                                              (3, 400_000, 9_000_001, 4096), (4, 40_000, 90_000, 256)])
def test_build_broadcast_form_materialising_matches_the_oracle(fj, oracle, world, nb_total, np_total, target):
    """The MATERIALISING build-broadcast step (_hash_join_radix_materialize, hash_join.cpp:315-381, across GPUs; csrc/fj_bcast.hip:
    the values travel as a fourth part of every region, the step is counted by the counting step's kernel, fj_emit_pairs writes every
    rank's pairs - (probe key, build value) of its OWN probe rows - with fj_dense_mat_join), all ranks played by this GPU: the ranks'
    pair sets together are the NumPy oracle's pair list, digest for digest; ragged blocks, repeated probe keys, both plane widths, 1
    and several pieces.  A build key that two ranks hold yields one pair per matching probe row, with one of the copies' values."""
    import torch
    from flash_hash_join_amd.lab import LabEngine
    fj.set_option("plan_target_keys", target)
    try:
        eng = LabEngine("cuda:0")
        rng = np.random.default_rng(world * 77 + nb_total % 89)
        bk = np.unique(rng.integers(0, 2**64, size=nb_total, dtype=np.uint64))
        bv = bk * np.uint64(0x9E3779B97F4A7C15) + np.uint64(3)
        pk = np.concatenate([rng.choice(bk, np_total // 2), rng.integers(0, 2**64, size=np_total - np_total // 2, dtype=np.uint64)])
        rng.shuffle(pk)
        exp, ek, ev = oracle.np_join(bk, bv, pk, return_arrays=True)
        cutb = sorted(rng.integers(0, bk.size, size=world - 1).tolist()); cutb[0] = 0            # rank 0: no build rows
        cutp = sorted(rng.integers(0, pk.size, size=world - 1).tolist()); cutp[-1] = pk.size      # last rank: no probe rows
        bks = [torch.from_numpy(x.view(np.int64).copy()).cuda() for x in np.split(bk, cutb)]
        bvs = [torch.from_numpy(x.view(np.int64).copy()).cuda() for x in np.split(bv, cutb)]
        pks = [torch.from_numpy(x.view(np.int64).copy()).cuda() for x in np.split(pk, cutp)]
        sizes = [int(b.numel()) for b in bks]
        nbt = int(bk.size)
        bits, nparts, _ = eng.bcast_plan(nbt)
        for pieces in (1, 1 + world % 4):
            rbs = [eng.bcast_region_bytes(nbt, n, True) for n in sizes]
            offs = [sum(rbs[:r]) for r in range(world)]
            base = torch.empty(sum(rbs), dtype=torch.uint8, device="cuda:0")
            empty = torch.empty(16, dtype=torch.int64, device="cuda:0")[:0]
            for r in range(world):                      # what the peers would have sent
                eng.bcast_pack(bks[r], nbt, base[offs[r]: offs[r] + rbs[r]], pieces, vals=bvs[r])
                assert eng.bcast_pack_bounds(pieces)[-1] == sizes[r]
                eng.bcast_probe(empty, nbt)
                assert eng.bcast_finish() == 0
            ks, vs, total = [], [], 0
            for r in range(world):
                eng.bcast_pack(bks[r], nbt, base[offs[r]: offs[r] + rbs[r]], pieces, vals=bvs[r])
                eng.bcast_probe(pks[r], nbt)
                for q in range(pieces):
                    eng.bcast_join(base, offs, sizes, nparts * q // pieces, nparts * (q + 1) // pieces)
                n = eng.bcast_finish()
                k, v = eng.emit_pairs(n)
                assert k.numel() == n and bool(torch.isin(k, pks[r]).all())          # the pairs stay with the probe rows
                ks.append(k.cpu().numpy().view(np.uint64)); vs.append(v.cpu().numpy().view(np.uint64)); total += n
            assert total == exp
            assert _digest(oracle, np.concatenate(ks), np.concatenate(vs)) == _digest(oracle, ek, ev)
        # the same key on two ranks: served - ONE pair per matching probe row, carrying the value of one of the copies (across GPUs there
        # is no first occurrence to prefer; hash_join.cpp:125 drops duplicates at insert, so a probe row never yields two pairs)
        dup_b = [torch.cat([bks[-1], bks[1][:3] if world > 1 and sizes[1] >= 3 else bks[-1][:3]])] if sizes[-1] else None
        if dup_b is not None and world > 1 and sizes[1] >= 3:
            bks2, bvs2 = bks[:-1] + dup_b, bvs[:-1] + [torch.cat([bvs[-1], bvs[1][:3]])]
            sizes2 = [int(b.numel()) for b in bks2]
            nbt2 = sum(sizes2)
            if eng.bcast_plan(nbt2) is not None and eng.bcast_plan(nbt2)[0] == bits:
                rbs = [eng.bcast_region_bytes(nbt2, n, True) for n in sizes2]
                offs = [sum(rbs[:r]) for r in range(world)]
                base = torch.empty(sum(rbs), dtype=torch.uint8, device="cuda:0")
                for r in range(world):
                    eng.bcast_pack(bks2[r], nbt2, base[offs[r]: offs[r] + rbs[r]], 1, vals=bvs2[r])
                    eng.bcast_pack_bounds(1); eng.bcast_probe(empty, nbt2); eng.bcast_finish()
                probe_all = torch.cat(pks + [bks[1][:3]])
                eng.bcast_pack(bks2[0], nbt2, base[offs[0]: offs[0] + rbs[0]], 1, vals=bvs2[0])
                eng.bcast_probe(probe_all, nbt2)
                eng.bcast_join(base, offs, sizes2, 0, eng.bcast_plan(nbt2)[1])
                n = eng.bcast_finish()
                bk_all, bv_all = torch.cat(bks2), torch.cat(bvs2)
                assert n == int(torch.isin(probe_all, bk_all).sum())
                k, v = eng.emit_pairs(n)
                assert bool(torch.equal(torch.sort(k)[0], torch.sort(probe_all[torch.isin(probe_all, bk_all)])[0]))
                M = -7046029254386353131
                assert bool(torch.isin(k * M + v, bk_all * M + bv_all).all())            # every value belongs to a copy of its key
                d3 = torch.isin(k, bks[1][:3])                                           # the duplicated keys were probed (probe_all ends with them)
                assert int(d3.sum()) >= 3
    finally:
        fj.set_option("plan_target_keys", 4096)


def _bcast_mat_step(eng, rng, nb, np_):
    """One materialising build-broadcast step of a one-rank world, counted and NOT emitted: (count, what must stay alive, the
    oracle's pairs)."""
    import torch
    bk = np.unique(rng.integers(0, 2**64, size=nb, dtype=np.uint64))
    bv = bk * np.uint64(0x9E3779B97F4A7C15) + np.uint64(3)
    pk = np.concatenate([rng.choice(bk, np_ // 2), rng.integers(0, 2**64, size=np_ - np_ // 2, dtype=np.uint64)])
    bk_t, bv_t, pk_t = (torch.from_numpy(x.view(np.int64).copy()).cuda() for x in (bk, bv, pk))
    nbt = int(bk.size)
    nparts = eng.bcast_plan(nbt)[1]
    base = torch.empty(eng.bcast_region_bytes(nbt, nbt, True), dtype=torch.uint8, device="cuda:0")
    eng.bcast_pack(bk_t, nbt, base, 1, vals=bv_t)
    assert eng.bcast_pack_bounds(1)[-1] == nbt
    eng.bcast_probe(pk_t, nbt)
    eng.bcast_join(base, [0], [nbt], 0, nparts)
    n = eng.bcast_finish()
    assert n > 0
    return n, (bk_t, bv_t, pk_t, base), (bk, bv, pk)


def test_stale_build_broadcast_result_is_not_emitted(fj, oracle):
    """A materialising build-broadcast step whose pairs are never fetched (distributed_join(materialize=True) without return_arrays)
    must not stand in for the next two-phase materialising join on the same context: the one-shot join (count, then fj_emit_pairs)
    returns its OWN pairs.  The one-shot join is no bigger than the step on either side."""
    import torch
    from flash_hash_join_amd.lab import LabEngine
    eng = LabEngine("cuda:0")
    rng = np.random.default_rng(4242)
    _, keep, _ = _bcast_mat_step(eng, rng, 70_000, 300_000)
    bk = np.unique(rng.integers(0, 2**64, size=50_000, dtype=np.uint64))
    bv = rng.integers(0, 2**64, size=bk.size, dtype=np.uint64)
    pk = np.concatenate([rng.choice(bk, 100_000), rng.integers(0, 2**64, size=100_000, dtype=np.uint64)])
    exp, ek, ev = oracle.np_join(bk, bv, pk, return_arrays=True)
    fj.set_option("mat_single_pass", 0)
    try:
        n, _, k, v = fj.hash_join_radix(*(torch.from_numpy(x.view(np.int64).copy()).cuda() for x in (bk, bv, pk)), return_arrays=True)
    finally:
        fj.set_option("mat_single_pass", 1)
    assert n == exp
    assert _digest(oracle, k.cpu().numpy().view(np.uint64), v.cpu().numpy().view(np.uint64)) == _digest(oracle, ek, ev)
    del keep


def test_refused_build_broadcast_emit_leaves_the_result_pending(fj, oracle):
    """fj_emit_pairs of a materialising build-broadcast step: a call that is refused (output capacity below the count, a misaligned
    output buffer) writes nothing and leaves the result pending; the next correct call writes the oracle's pairs, and a further
    one finds nothing pending (as test_c_abi_rejects_bad_arguments asserts for a one-shot join)."""
    import ctypes
    import torch
    from flash_hash_join_amd import _lib
    from flash_hash_join_amd.lab import LabEngine
    eng = LabEngine("cuda:0")
    L = _lib.load()
    n, keep, (bk, bv, pk) = _bcast_mat_step(eng, np.random.default_rng(77), 40_000, 90_000)
    exp, ek, ev = oracle.np_join(bk, bv, pk, return_arrays=True)
    assert n == exp
    st = torch.cuda.current_stream(0).cuda_stream
    t = _lib.FjTimings()
    ok = torch.empty(n + 1, dtype=torch.int64, device="cuda:0"); ov = torch.empty_like(ok)
    assert L.fj_emit_pairs(eng.ctx, ok.data_ptr(), ov.data_ptr(), n - 1, st, ctypes.byref(t)) == 1 and "capacity" in _lib.last_error()
    assert L.fj_emit_pairs(eng.ctx, ok.data_ptr() + 4, ov.data_ptr(), n, st, ctypes.byref(t)) == 1 and "aligned" in _lib.last_error()
    assert L.fj_emit_pairs(eng.ctx, ok.data_ptr(), ov.data_ptr(), n, st, ctypes.byref(t)) == 0
    assert _digest(oracle, ok[:n].cpu().numpy().view(np.uint64), ov[:n].cpu().numpy().view(np.uint64)) == _digest(oracle, ek, ev)
    assert L.fj_emit_pairs(eng.ctx, ok.data_ptr(), ov.data_ptr(), n, st, ctypes.byref(t)) == 1 and "no counted" in _lib.last_error()
    del keep


@pytest.mark.parametrize("np_rank", [200_000, 4_000_000])
def test_build_broadcast_refuses_a_partition_that_cannot_fit_the_table(fj, np_rank):
    """One final partition of the global plan holds 20000 distinct build keys (built by inverting the key mixer: their mixed keys share
    the partition's top bits) - more than the 16384-slot table takes.  The step must fail loudly (the dispatcher then reruns the join as
    the owner shuffle), under the plain deal of items and - 4M probe rows per rank: 18 items per partition - under the deal in runs,
    where the items of the oversized partition inherit its verdict from the one that tried to build it."""
    import torch
    from flash_hash_join_amd import _lib
    from flash_hash_join_amd.lab import LabEngine as HipEngine
    L = _lib.load()
    eng = HipEngine("cuda:0")
    world, nb_total = 2, 400_000
    bits, nparts, _ = eng.bcast_plan(nb_total)
    assert 5 <= bits <= 8
    rng = np.random.default_rng(99)
    hot = np.unique(rng.integers(0, 2**(64 - bits), size=20_500, dtype=np.uint64))[:20_000] | (np.uint64(3) << np.uint64(64 - bits))   # mixed keys of partition 3
    hot = np.array([L.fj_key_unmix64(int(x)) for x in hot], dtype=np.uint64)
    rest = rng.integers(0, 2**64, size=nb_total - hot.size, dtype=np.uint64)
    bk = np.unique(np.concatenate([hot, rest]))
    rng.shuffle(bk)
    pk = np.concatenate([rng.choice(bk, np_rank), rng.integers(0, 2**64, size=np_rank, dtype=np.uint64)])
    bks = [torch.from_numpy(x.view(np.int64).copy()).cuda() for x in np.array_split(bk, world)]
    pks = [torch.from_numpy(x.view(np.int64).copy()).cuda() for x in np.array_split(pk, world)]
    with pytest.raises(RuntimeError, match="does not fit the LDS table"):
        _bcast_emulated(eng, world, bks, pks, int(bk.size), 2)
    # the context is usable afterwards: the same relations without the hot keys join exactly
    bk2 = np.setdiff1d(bk, hot)
    bks2 = [torch.from_numpy(x.view(np.int64).copy()).cuda() for x in np.array_split(bk2, world)]
    exp = int(np.isin(pk, bk2).sum())
    assert _bcast_emulated(eng, world, bks2, pks, int(bk2.size), 2) == exp


def test_config5_build_broadcast_every_rank_at_full_size_on_one_gpu(fj):
    """BASELINE configs[4] (1B build x 10B probe rows over 8 GPUs) at FULL size in the build-broadcast form, all 8 ranks played by
    this one GPU: every rank's 125M build rows are packed into its 0.75-GB region (18-bit plan: 262144 final partitions, 6 wire bytes
    per key), then every rank joins its own 1.25B probe rows against the 8 regions in 4 ranges.  The ranks' counts add up to the
    closed-form count of the whole join."""
    import torch
    from flash_hash_join_amd import datagen
    from flash_hash_join_amd.lab import LabEngine as HipEngine
    world, nb_rank, np_rank, pieces = 8, 125_000_000, 1_250_000_000, 4
    nb_total = nb_rank * world
    eng = HipEngine("cuda:0")
    assert eng.bcast_plan(nb_total) == (18, 262144, 2)
    rb = eng.bcast_region_bytes(nb_total, nb_rank)
    assert 6.0 < rb / nb_rank < 6.02
    base = torch.empty(rb * world, dtype=torch.uint8, device="cuda:0")
    offs = [r * rb for r in range(world)]
    empty = torch.empty(16, dtype=torch.int64, device="cuda:0")[:0]
    for r in range(world):
        bk, _ = datagen.build_device(nb_rank, "cuda:0", first=r * nb_rank)
        eng.bcast_pack(bk, nb_total, base[offs[r]: offs[r] + rb], pieces)
        b = eng.bcast_pack_bounds(pieces)
        assert b[-1] == nb_rank and all(abs(b[q] - nb_rank * q / pieces) < 6 * nb_rank ** 0.5 for q in range(pieces + 1))
        eng.bcast_probe(empty, nb_total); eng.bcast_finish()
        del bk
    total = expected = 0
    for r in range(world):
        bk, _ = datagen.build_device(nb_rank, "cuda:0", first=r * nb_rank)
        pk, e = datagen.probe_device(np_rank, nb_total, "cuda:0", seed=1, hit_bp=5000, first=r * np_rank)
        expected += e
        eng.bcast_pack(bk, nb_total, base[offs[r]: offs[r] + rb], pieces)
        eng.bcast_probe(pk, nb_total)
        for q in range(pieces):
            eng.bcast_join(base, offs, [nb_rank] * world, 262144 * q // pieces, 262144 * (q + 1) // pieces)
        total += eng.bcast_finish()
        del bk, pk
    assert abs(expected - 0.5 * np_rank * world) < 6 * (np_rank * world) ** 0.5
    assert total == expected, (total, expected)


def test_config5_materialising_build_broadcast_every_rank_at_full_size_on_one_gpu(fj):
    """The same full-size emulation for the MATERIALISING join (_hash_join_radix_materialize, hash_join.cpp:315-381, across 8 GPUs
    in the build-broadcast form): the regions carry the build values (14 bytes per row), every rank counts its 1.25B probe rows
    against the 8 regions (fj_dense_mat_join) and writes its ~625M pairs beside them (fj_emit_pairs).  Per rank: the count is the
    generator's closed form, every pair obeys the generator's key -> value rule with a value of the global build side, and the
    pairs' keys sum to the sum of the probe keys that are build keys (computed from the rule, independently of any join)."""
    import torch
    from flash_hash_join_amd import datagen
    from flash_hash_join_amd.lab import LabEngine as HipEngine
    world, nb_rank, np_rank, pieces = 8, 125_000_000, 1_250_000_000, 4
    nb_total = nb_rank * world
    eng = HipEngine("cuda:0")
    rb = eng.bcast_region_bytes(nb_total, nb_rank, True)
    assert 14.0 < rb / nb_rank < 14.02
    base = torch.empty(rb * world, dtype=torch.uint8, device="cuda:0")
    offs = [r * rb for r in range(world)]
    empty = torch.empty(16, dtype=torch.int64, device="cuda:0")[:0]
    for r in range(world):
        bk, bv = datagen.build_device(nb_rank, "cuda:0", first=r * nb_rank)
        eng.bcast_pack(bk, nb_total, base[offs[r]: offs[r] + rb], pieces, vals=bv)
        assert eng.bcast_pack_bounds(pieces)[-1] == nb_rank
        eng.bcast_probe(empty, nb_total); eng.bcast_finish()
        del bk, bv
    M = -7046029254386353131                               # build row i: key (i + 1) * M, value i (fj_generate_build)
    Minv = pow(M % 2**64, -1, 2**64)
    Minv = Minv - 2**64 if Minv >= 2**63 else Minv
    for r in range(world):
        bk, bv = datagen.build_device(nb_rank, "cuda:0", first=r * nb_rank)
        pk, e = datagen.probe_device(np_rank, nb_total, "cuda:0", seed=1, hit_bp=5000, first=r * np_rank)
        eng.bcast_pack(bk, nb_total, base[offs[r]: offs[r] + rb], pieces, vals=bv)
        eng.bcast_probe(pk, nb_total)
        for q in range(pieces):
            eng.bcast_join(base, offs, [nb_rank] * world, 262144 * q // pieces, 262144 * (q + 1) // pieces)
        n = eng.bcast_finish()
        assert n == e, (r, n, e)
        k, v = eng.emit_pairs(n)
        assert k.numel() == n and int(v.min()) >= 0 and int(v.max()) < nb_total
        assert bool(torch.all((v + 1) * M == k))
        w = pk * Minv - 1
        hit = (w >= 0) & (w < nb_total)
        assert int(hit.sum()) == n and int((pk * hit).sum()) == int(k.sum()) and int((w * hit).sum()) == int(v.sum())
        del bk, bv, pk, k, v, w, hit
        torch.cuda.empty_cache()


def test_config5_chunk_form_with_the_precheck_every_owner_at_full_size_on_one_gpu(fj):
    """The same full-size emulation (1B x 10B rows, the 8-rank plan: 9 + 9 bits, 262144 final partitions) with the sender-side
    precheck of the chunk form: every owner appends the 8 build shares and exports its 32768 partitions' Bloom filters
    (fj_stream_export_part_filters: 1 GiB in all, assembled as the driver's all-gather would), every sender compacts its probe
    pieces against them before the copy into the wire format (fj_shuffle_pack_filter), every owner joins what is left.  The owners'
    counts still add up to the closed-form count of the whole join - no build key's probe row is ever dropped - while ~48 % of the
    probe rows never reach the wire (the hits + ~3 % of the misses travel)."""
    import torch
    from flash_hash_join_amd import datagen
    from flash_hash_join_amd.lab import LabEngine as HipEngine
    world, nb_rank, np_rank = 8, 125_000_000, 1_250_000_000
    nb_total = nb_rank * world
    eng = HipEngine("cuda:0")
    bshare = []
    for r in range(world):
        bk, _ = datagen.build_device(nb_rank, "cuda:0", first=r * nb_rank)
        ch, dw, used = eng.shuffle_pack(bk, None, nb_total, world)
        torch.cuda.synchronize()
        bshare.append([(c.clone(), d.clone()) for c, d in zip(ch, dw)])
        del bk, ch, dw
    first, count, total_parts, fb = eng.part_filter_range(nb_total, world, 0)
    assert (total_parts, fb) == (1 << 18, 4096) and count == total_parts // world
    filters = torch.zeros(total_parts * fb, dtype=torch.uint8, device="cuda:0")
    for o in range(world):                                          # the owners' filters, where the all-gather would put them
        first, count, _, _ = eng.part_filter_range(nb_total, world, o)
        eng.stream_open_shuffled(nb_total, world, o, sum(bshare[r][o][1].numel() for r in range(world)) * 256, world, 1 << 20, 1)
        for r in range(world):
            eng.stream_append_chunks(0, bshare[r][o][0].clone(), bshare[r][o][1].clone())     # (directory words are rewritten in place: the shares are needed again)
        eng.stream_export_part_filters(filters[first * fb: (first + count) * fb])
        torch.cuda.synchronize()
        eng.L.fj_stream_abort(eng.ctx)
    pshare, expected, kept, wire_bytes = [], 0, 0, 0
    for r in range(world):
        pk, e = datagen.probe_device(np_rank, nb_total, "cuda:0", seed=1, hit_bp=5000, first=r * np_rank)
        expected += e
        ch, dw, used = eng.shuffle_pack(pk, None, nb_total, world, filters=filters)
        torch.cuda.synchronize()
        kept += eng.last_pack_kept
        assert e <= eng.last_pack_kept <= e + 0.04 * (np_rank - e)   # every hit + at most 4 % of the misses
        pshare.append([(c.clone(), d.clone()) for c, d in zip(ch, dw)])
        wire_bytes += sum(c.numel() + 4 * d.numel() for c, d in zip(ch, dw))
        del pk, ch, dw
        torch.cuda.empty_cache()
    assert 0.50 < kept / (np_rank * world) < 0.53 and wire_bytes / (np_rank * world) < 0.53 * 7.03
    total = 0
    for o in range(world):
        nbc = sum(bshare[r][o][1].numel() for r in range(world)); npc = sum(pshare[r][o][1].numel() for r in range(world))
        eng.stream_open_shuffled(nb_total, world, o, nbc * 256, world, npc * 256, world)
        for r in range(world):
            eng.stream_append_chunks(0, bshare[r][o][0], bshare[r][o][1])
        for r in range(world):
            eng.stream_append_chunks(1, pshare[r][o][0], pshare[r][o][1])
        total += eng.stream_finish()
    assert total == expected, (total, expected)
    print(f"precheck at the 8-rank plan, full size: {kept / (np_rank * world):.4f} of the probe rows travel, {wire_bytes / (np_rank * world):.3f} wire bytes per probe row")


def test_full_config5_shard_through_the_driver_on_a_one_rank_communicator(fj, monkeypatch):
    """fj_dist_join_count (csrc/fj_dist.hip) at the size the scaling run times it: one config-5 shard, 125M x 1.25B rows, on a
    1-rank RCCL communicator - plan for the shard, 8 + 7 bits, 7-byte wire chunks, four probe pieces on three streams - against
    the closed-form count; then the same step with the rank's own share routed through the grouped ncclSend / ncclRecv block
    (FJ_DIST_LOOPBACK=1: the code path every peer's share takes at N > 1), and once more over the callback transport."""
    import socket
    import torch
    import torch.distributed as dist
    from flash_hash_join_amd import datagen
    from flash_hash_join_amd.distributed import distributed_join
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        monkeypatch.setenv("FJ_DIST_STRATEGY", "shuffle"); monkeypatch.setenv("FJ_DIST_NO_FALLBACK", "1")
        _dj0 = distributed_join
        distributed_join = lambda *a, **kw: _dj0(*a, force_exchange=True, **kw)      # the full protocol on this one rank
        nb, npk = 125_000_000, 1_250_000_000
        bk, bv = datagen.build_device(nb, "cuda:0")
        pk, exp = datagen.probe_device(npk, nb, "cuda:0", seed=1, hit_bp=5000)
        for loop, native in (("0", "1"), ("1", "1"), ("0", "0")):
            fj.set_option("lab_hooks", int(loop)); monkeypatch.setenv("FJ_DIST_NATIVE", native)      # (lab_hooks & 1 = FJ_HOOK_LOOPBACK)
            t = {}
            n, sec = distributed_join(bk, bv, pk, timings=t)
            assert n == exp and t["local_count"] == exp and t["pieces"] == 4 and t["wire_chunk_bytes"] == 1792, t
            assert t["shuffle_form"] == ("chunks (fj_dist_join over RCCL)" if native == "1" else "chunks (fj_dist_join over a callback transport)")
            # dense chunks: at most one partial chunk per (bucket, piece); looped back, every chunk went through ncclSend / ncclRecv
            assert npk <= t["local_probe_rows"] <= npk + 256 * 256 * 4 and nb <= t["local_build_rows"] <= nb + 256 * 256
            sent = (t["local_probe_rows"] + t["local_build_rows"]) // 256 * (1792 + 4)
            assert t["wire_bytes_sent"] == (sent if loop == "1" else 0), (t["wire_bytes_sent"], sent)
            lt = fj.last_timings()
            assert lt["fell_back"] == 0 and lt["passes"] == 2
        # the control collectives on a communicator of their own (ncclCommSplit - what every N > 1 job does; a 1-rank communicator
        # only splits under this test hook): a fresh communicator, the same step, the same count
        from flash_hash_join_amd.lab import LabEngine as HipEngine
        HipEngine.close_native_comms()
        fj.set_option("lab_hooks", 4 | 1); monkeypatch.setenv("FJ_DIST_NATIVE", "1")                 # FJ_HOOK_SPLIT_ALWAYS | FJ_HOOK_LOOPBACK
        t = {}
        n, sec = distributed_join(bk[: nb // 10], bv[: nb // 10], pk[: npk // 10], timings=t)
        assert t["shuffle_form"] == "chunks (fj_dist_join over RCCL)" and n == int(torch.isin(pk[: npk // 10], bk[: nb // 10]).sum())
        HipEngine.close_native_comms()
    finally:
        fj.set_option("lab_hooks", 0)
        dist.destroy_process_group()


def test_sender_side_precheck_in_chunk_form_on_a_one_rank_communicator(fj, monkeypatch):
    """fj_dist_join(prefilter_below): the owner exports one 4-KiB Bloom filter per final partition of the global plan
    (fj_stream_export_part_filters), the sender compacts every probe piece's level-1 chunks in place to the keys some filter admits
    (fj_shuffle_pack_filter) before they are rewritten for the wire.  Counts stay exact (no build key is ever dropped), the rows
    that travel shrink to the hits plus 1-3 % of the misses; "auto" samples first (a strided 1M-row sample against the filters) and
    decides against the model's break-even - zero on one rank, where no link is saved; materialising joins and the callback
    transport take the same path."""
    import socket
    import torch
    import torch.distributed as dist
    from flash_hash_join_amd import datagen
    from flash_hash_join_amd.distributed import distributed_join
    import flash_hash_join_amd.distributed as D
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        monkeypatch.setenv("FJ_DIST_STRATEGY", "shuffle"); monkeypatch.setenv("FJ_DIST_NO_FALLBACK", "1")
        _dj0 = distributed_join
        distributed_join = lambda *a, **kw: _dj0(*a, force_exchange=True, **kw)      # the full protocol on this one rank
        for nb, npk in ((20_000_000, 200_000_000), (125_000_000, 1_250_000_000), (3_000_001, 10_000_003)):
            bk, bv = datagen.build_device(nb, "cuda:0")
            for hit_bp in (500, 5000):
                pk, exp = datagen.probe_device(npk, nb, "cuda:0", seed=3, hit_bp=hit_bp)
                monkeypatch.setenv("FJ_DIST_PREFILTER", "1")
                for loop, native in (("0", "1"), ("1", "1"), ("0", "0")):
                    if (loop, native) != ("0", "1") and npk > 200_000_000:
                        continue
                    fj.set_option("lab_hooks", int(loop)); monkeypatch.setenv("FJ_DIST_NATIVE", native)
                    t = {}
                    n, sec = distributed_join(bk, bv, pk, timings=t)
                    assert n == exp and t["shuffle_form"].startswith("chunks") and t["prefilter"] is True and t["prefilter_mode"] == "on", t
                    misses = npk - exp
                    assert exp <= t["probe_rows_sent"] <= exp + 0.15 * misses + 4 * 65536, (t["probe_rows_sent"], exp, misses)
                    assert t["local_probe_rows"] <= t["probe_rows_sent"] + 256 * 512 * 4, t
                    print(f"precheck {nb}x{npk} at {hit_bp / 100:.0f} % hits: {t['probe_rows_sent'] / npk:.3f} of the probe rows travel ({(t['probe_rows_sent'] - exp) / max(1, misses):.3f} of the misses), step {sec * 1e3:.2f} ms")
                monkeypatch.delenv("FJ_DIST_PREFILTER")
                fj.set_option("lab_hooks", 0); monkeypatch.setenv("FJ_DIST_NATIVE", "1")
                t = {}
                n, sec = distributed_join(bk, bv, pk, bloom=True, timings=t)              # "auto": on one rank the model always declines
                assert n == exp and t["prefilter_mode"] == "auto" and t["prefilter_below"] == 0 and t["prefilter"] is False and t["prefilter_sampled_survivors"] is None, t
                monkeypatch.setattr(D, "PREFILTER_BELOW_OVERRIDE", 0.3)                   # ... a threshold in its place: sample, then decide
                D._PRECHECK_MEMO.clear()
                n, sec = distributed_join(bk, bv, pk, bloom=True, timings=t)
                assert n == exp and t["prefilter_decision"] == "sampled" and abs(t["prefilter_sampled_survivors"] - (exp + 0.03 * (npk - exp)) / npk) < 0.03, t
                assert t["prefilter"] == (t["prefilter_sampled_survivors"] < 0.3) == (hit_bp == 500), t
                t2 = {}
                n, sec = distributed_join(bk, bv, pk, bloom=True, timings=t2)             # the same shape again: the verdict is remembered,
                assert n == exp and t2["prefilter"] == t["prefilter"] and t2["prefilter_sampled_survivors"] is None, t2      # nothing is sampled,
                assert t2["prefilter_decision"] == ("memo: runs" if hit_bp == 500 else "memo: declined"), t2
                assert t2["filter_bytes_received"] == 0 and (t2["prefilter"] or t2["prefilter_below"] == 0), t2              # and a declined precheck exports nothing
                monkeypatch.setattr(D, "PREFILTER_BELOW_OVERRIDE", None)
            if npk <= 200_000_000:
                monkeypatch.setenv("FJ_DIST_PREFILTER", "1")
                sub = pk[: min(npk, 50_000_000)]
                t = {}
                n, _, k, v = distributed_join(bk, bv, sub, materialize=True, return_arrays=True, timings=t)
                M = torch.tensor(-7046029254386353131, dtype=torch.int64, device="cuda:0")
                assert t["prefilter"] is True and n == k.numel() == int(torch.isin(sub, bk).sum()) and bool(torch.all((v + 1) * M == k)), t
                monkeypatch.delenv("FJ_DIST_PREFILTER")
            del bk, bv, pk
    finally:
        dist.destroy_process_group()


def test_driver_with_tiny_and_empty_probe_sides(fj, monkeypatch):
    """fj_dist_join_count on a 1-rank communicator when the probe side is too small to be cut into pieces (one piece then), one
    row, or empty; and a materialising step whose probe side is tiny."""
    import socket
    import torch
    import torch.distributed as dist
    from flash_hash_join_amd import datagen
    from flash_hash_join_amd.distributed import distributed_join
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        monkeypatch.setenv("FJ_DIST_STRATEGY", "shuffle"); monkeypatch.setenv("FJ_DIST_NO_FALLBACK", "1")
        _dj0 = distributed_join
        distributed_join = lambda *a, **kw: _dj0(*a, force_exchange=True, **kw)      # the full protocol on this one rank
        bk, bv = datagen.build_device(6_000_000, "cuda:0")
        pk, _ = datagen.probe_device(1000, 6_000_000, "cuda:0", seed=8, hit_bp=5000)
        for n in (0, 1, 5, 7, 1000):
            t = {}
            sub = pk[:n].clone() if n else pk[:0]
            got, _ = distributed_join(bk, bv, sub, timings=t)
            assert got == int(torch.isin(sub, bk).sum()) and t["shuffle_form"].startswith("chunks") and t["pieces"] == (4 if n >= 8 else 1), (n, t)
        n, _, k, v = distributed_join(bk, bv, pk[:7].clone(), materialize=True, return_arrays=True)
        M = torch.tensor(-7046029254386353131, dtype=torch.int64, device="cuda:0")
        assert n == int(torch.isin(pk[:7], bk).sum()) == k.numel() and bool(torch.all((v + 1) * M == k))
        for pre in ("0", "1"):                               # an EMPTY probe side, materialising (found by tools/precheck_fuzz.py): zero pairs, not an error
            monkeypatch.setenv("FJ_DIST_PREFILTER", pre)
            t = {}
            n, _, k, v = distributed_join(bk, bv, pk[:0], materialize=True, return_arrays=True, timings=t)
            assert n == 0 and k.numel() == 0 and v.numel() == 0 and t["shuffle_form"].startswith("chunks"), t
    finally:
        dist.destroy_process_group()


def test_one_oversized_partition_costs_little_at_full_size(fj):
    """Build-side skew at BASELINE configs[2] sizes: 100M x 1B rows plus 27K build keys that all land in ONE of the 32768 final
    partitions (ten times its share: keys picked so that the top 15 bits of their hash word 1 agree), probed 500K times.
    Only that partition is re-partitioned (fell_back == 0, lds_retries == 2); the count is exact and the join takes at most
    the uniform join's plan (rounds 1-2 re-ran the whole join on one table in HBM: 4.5x the time; the ratio here, 1.12-1.15x, is
    printed, not asserted)."""
    import torch
    from flash_hash_join_amd import datagen
    nb, npk = 100_000_000, 1_000_000_000
    dev = "cuda:0"

    def hash_w1(k):                                                # fj_hash_w1 of csrc/fj_common.h on int64 tensors
        m32 = 0xFFFFFFFF
        lo, hi = k & m32, (k >> 32) & m32
        x = ((lo * 0x9E3779B1) & m32) ^ ((hi * 0x85EBCA77) & m32)
        x = x ^ (x >> 16); x = (x * 0x85ebca6b) & m32
        x = x ^ (x >> 13); x = (x * 0xc2b2ae35) & m32
        return x ^ (x >> 16)
    found, target, base = [], 12345, 1 << 40
    for c0 in range(0, 1 << 30, 1 << 26):
        cand = torch.arange(base + c0, base + c0 + (1 << 26), dtype=torch.int64, device=dev)
        found.append(cand[(hash_w1(cand) >> 17) == target])
        del cand
    extra = torch.cat(found)[:27_000]
    assert extra.numel() == 27_000
    bk, bv = datagen.build_device(nb, dev)
    pk, exp = datagen.probe_device(npk, nb, dev, seed=1, hit_bp=5000)
    assert not bool(torch.isin(extra, bk).any())

    def timed(bk_, bv_, pk_):
        best = None
        for _ in range(4):
            n, sec = fj.hash_join_count_radix(bk_, bv_, pk_)
            best = sec if best is None else min(best, sec)
        return n, best, fj.last_timings()
    n_u, t_u, lt_u = timed(bk, bv, pk)
    assert n_u == exp and lt_u["fell_back"] == 0 and lt_u["lds_retries"] == 0
    lost = int(torch.isin(pk[:500_000], bk).sum())                 # hits of the probe rows that are overwritten below
    bk2, bv2 = torch.cat([bk, extra]), torch.cat([bv, extra + 1])
    del bk, bv
    pk[:500_000] = extra.repeat(19)[:500_000]
    n_s, t_s, lt_s = timed(bk2, bv2, pk)
    assert n_s == exp - lost + 500_000
    assert lt_s["fell_back"] == 0 and lt_s["lds_retries"] == 2, lt_s      # 1 (tagged-table retry) + 1 partition re-partitioned
    # structural, not a stopwatch: the plan is the uniform join's, only ONE partition was redone, nothing ran on the HBM table.
    # (What that costs - 1.12-1.15x the uniform join on one box - is measured by tools/skew_build_partition_probe.py; a wall-clock
    # bound in a parity suite fails for reasons that are not correctness.)
    assert lt_s["passes"] == lt_u["passes"] and lt_s["partitions"] == lt_u["partitions"] and lt_s["path"] == 0
    print(f"skewed / uniform join time on this box: {t_s / t_u:.3f}")


def test_hot_probe_key_is_sliced_across_workgroups(fj):
    """Skew: half of 400M probe rows carry ONE key.  Its partition's probe chunk list is cut into many work items (the
    item table), so the join stays within a small factor of the uniform case instead of serialising on one workgroup."""
    import torch
    from flash_hash_join_amd import datagen
    nb, npk = 20_000_000, 400_000_000
    dbk, dbv = datagen.build_device(nb, "cuda:0")
    dpk, exp = datagen.probe_device(npk, nb, "cuda:0", seed=5, hit_bp=5000)
    n, _ = fj.hash_join_count_radix(dbk, dbv, dpk)
    n, _ = fj.hash_join_count_radix(dbk, dbv, dpk)
    uniform_ms = fj.last_timings()["total_ms"]
    assert n == exp
    hot = dbk[12345].clone()
    uniform_hits_in_first_half = int(torch.isin(dpk[: npk // 2: 1000], dbk).sum())     # just to keep the generator honest
    assert uniform_hits_in_first_half > 0
    sel = torch.arange(0, npk, 2, device="cuda:0")
    replaced_hits = fj.hash_join_count_radix(dbk, dbv, dpk[sel].contiguous())[0]        # hits among the rows about to be replaced
    dpk[sel] = hot
    n, _ = fj.hash_join_count_radix(dbk, dbv, dpk)
    n2, _ = fj.hash_join_count_radix(dbk, dbv, dpk)
    skew_ms = fj.last_timings()["total_ms"]
    assert n == n2 == exp - replaced_hits + sel.numel()
    assert skew_ms < 8 * uniform_ms, (skew_ms, uniform_ms)      # (one workgroup streaming 200M rows alone would take ~100x)
    nm, _, k, v = fj.hash_join_radix(dbk, dbv, dpk, return_arrays=True)               # the materialising pass uses the same items
    assert nm == n and int((k == hot).sum()) >= sel.numel()
    del dpk, k, v
    torch.cuda.empty_cache()


def test_relation_beyond_the_chunk_directory_is_refused(fj):
    """A relation of more than ~4.2e9 rows does not fit one GPU's 24-bit chunk directory: the call must fail loudly
    (RuntimeError), not wrap around."""
    import torch
    from flash_hash_join_amd import datagen
    dbk, dbv = datagen.build_device(10_000_000, "cuda:0")
    dpk = torch.empty(4_400_000_000, dtype=torch.int64, device="cuda:0")         # contents irrelevant: refused before any kernel
    with pytest.raises(RuntimeError, match="too large"):
        fj.hash_join_count_radix(dbk, dbv, dpk)
    del dpk
    torch.cuda.empty_cache()
    assert fj.hash_join_count_radix(dbk, dbv, dbk)[0] == 10_000_000             # the context is still usable


@pytest.mark.parametrize("nb,npk", [(10_000_000, 100_000_000), (300_000_000, 50_000_000), (100_000_000, 1_000_000_000)])
def test_full_size_materialize_pairs_property(fj, nb, npk):
    """10M x 100M materialise, 300M x 50M (a 512-bucket pass that carries values) and BASELINE config 3's full 100M x 1B
    through hash_join_radix (500M pairs): every emitted pair satisfies key == (value+1)*M, count is closed-form."""
    import torch
    from flash_hash_join_amd import datagen
    dbk, dbv = datagen.build_device(nb, "cuda:0")
    dpk, exp = datagen.probe_device(npk, nb, "cuda:0", seed=9, hit_bp=5000)
    n, sec, k, v = fj.hash_join_radix(dbk, dbv, dpk, return_arrays=True)
    assert n == exp and k.numel() == exp
    del dpk
    M = torch.tensor(-7046029254386353131, dtype=torch.int64, device="cuda:0")      # 0x9E3779B97F4A7C15 as int64
    step = 100_000_000                                                              # (in slices: no 4 GB temporaries)
    for lo in range(0, exp, step):
        assert bool(torch.all((v[lo: lo + step] + 1) * M == k[lo: lo + step]))
    assert int(v.min()) >= 0 and int(v.max()) < nb
    del k, v, dbk, dbv
    torch.cuda.empty_cache()


def test_full_size_adaptive_materialize_with_the_precheck(fj):
    """BASELINE config 4's sizes (100M x 1B, 5 % hits) through adaptive_join: the sampled hit rate turns the bloom precheck on,
    the 50M emitted pairs satisfy key == (value+1)*M and the count is the closed form; adaptive_join_bloom agrees."""
    import torch
    from flash_hash_join_amd import datagen
    nb, npk = 100_000_000, 1_000_000_000
    dbk, dbv = datagen.build_device(nb, "cuda:0")
    dpk, exp = datagen.probe_device(npk, nb, "cuda:0", seed=1, hit_bp=500)
    n, sec, k, v = fj.adaptive_join(dbk, dbv, dpk, return_arrays=True)
    t = fj.last_timings()
    assert n == exp and k.numel() == exp and t["bloom_level"] == 1 and 300 <= t["sampled_hit_bp"] <= 700, t
    M = torch.tensor(-7046029254386353131, dtype=torch.int64, device="cuda:0")
    assert bool(torch.all((v + 1) * M == k))
    assert fj.adaptive_join_bloom(dbk, dbv, dpk)[0] == exp
    del dbk, dbv, dpk, k, v
    torch.cuda.empty_cache()


@pytest.mark.parametrize("nb,npk,pieces", [(2000, 300_000, 3), (50_000, 1_000_000, 4), (1_500_000, 6_000_000, 5),
                                           (3_000_000, 20_000_000, 4), (10, 1000, 2)])
def test_streamed_probe_equals_one_shot(fj, nb, npk, pieces):
    """fj_stream_begin / append_probe / finish (probe side in pieces) == the one-shot radix count, for zero-, one- and
    two-pass plans and both hash_top_bits settings."""
    import torch
    from flash_hash_join_amd import datagen, api
    from flash_hash_join_amd.lab import LabEngine as HipEngine
    bk, bv = datagen.build_device(nb, "cuda:0")
    pk, exp = datagen.probe_device(npk, nb, "cuda:0", seed=11, hit_bp=3000)
    eng = HipEngine("cuda:0")
    for top in (64, 48):
        assert api.join_device(api.ALGO_RADIX, 0, 0, bk, bv, pk, hash_top_bits=top)[0] == exp
        eng.stream_begin(bk, bv, npk, pieces, top)
        cuts = [npk * i // pieces for i in range(pieces + 1)]
        for i in range(pieces):
            eng.stream_append(pk[cuts[i]: cuts[i + 1]].clone())         # clones: 16-B aligned pieces
        assert eng.stream_finish() == exp


@pytest.mark.parametrize("nb,npk,bpieces,ppieces", [(2000, 300_000, 1, 3), (50_000, 1_000_000, 4, 2), (1_500_000, 6_000_000, 5, 1),
                                                    (3_000_000, 20_000_000, 3, 4), (10, 1000, 1, 2), (20_000_000, 30_000_000, 8, 1), (1_000_003, 5_000_011, 7, 3)])
def test_stream_join_with_both_sides_in_pieces(fj, nb, npk, bpieces, ppieces):
    """fj_stream_open / append_build / append_probe / advance_probe / finish == the one-shot radix count, with the
    probe side closed BEFORE the build side arrives (the replicate-build exchange order) and after it."""
    from flash_hash_join_amd import datagen
    from flash_hash_join_amd.lab import LabEngine as HipEngine
    bk, bv = datagen.build_device(nb, "cuda:0")
    pk, exp = datagen.probe_device(npk, nb, "cuda:0", seed=12, hit_bp=4000)
    eng = HipEngine("cuda:0")
    bcuts = [nb * i // bpieces for i in range(bpieces + 1)]
    pcuts = [npk * i // ppieces for i in range(ppieces + 1)]
    for probe_first in (True, False):
        eng.stream_open(nb, bpieces, npk, ppieces, 64)
        if probe_first:
            for i in range(ppieces):
                eng.stream_append(pk[pcuts[i]: pcuts[i + 1]])                 # views: the engine aligns them
            eng.stream_advance_probe()
        for i in range(bpieces):
            eng.stream_append_build(bk[bcuts[i]: bcuts[i + 1]])                 # views: the engine aligns them
        if not probe_first:
            for i in range(ppieces):
                eng.stream_append(pk[pcuts[i]: pcuts[i + 1]])                 # views: the engine aligns them
        assert eng.stream_finish() == exp


def test_streamed_join_recovers_from_an_oversized_partition_by_itself(fj):
    """A streamed (multi-GPU building block) join whose build side puts 9000 keys into one partition - beyond even the tagged
    LDS table - re-partitions that partition inside fj_stream_finish: exact count, no fallback, no exception."""
    import torch
    from flash_hash_join_amd.lab import LabEngine as HipEngine
    def hash_w1(k):                                                # fj_hash_w1 of csrc/fj_common.h
        lo = (k & np.uint64(0xFFFFFFFF)).astype(np.uint32); hi = (k >> np.uint64(32)).astype(np.uint32)
        with np.errstate(over="ignore"):
            x = (lo * np.uint32(0x9E3779B1)) ^ (hi * np.uint32(0x85EBCA77))
            x ^= x >> np.uint32(16); x *= np.uint32(0x85ebca6b)
            x ^= x >> np.uint32(13); x *= np.uint32(0xc2b2ae35)
            x ^= x >> np.uint32(16)
        return x
    cand = np.arange(1, 400000, dtype=np.uint64)
    skew = cand[(hash_w1(cand) >> np.uint32(27)) == 0][:9000]
    probe = np.concatenate([skew, cand[:50000]])
    exp = int(np.isin(probe, skew).sum())
    bk = torch.from_numpy(skew.view(np.int64)).cuda()
    pk = torch.from_numpy(probe.view(np.int64)).cuda()
    eng = HipEngine("cuda:0")
    eng.stream_open(bk.numel(), 2, pk.numel(), 3, 64)
    eng.stream_append(pk[:20000]); eng.stream_append(pk[20000:40000])
    eng.stream_append_build(bk[:5000]); eng.stream_append_build(bk[5000:])
    eng.stream_append(pk[40000:])
    assert eng.stream_finish() == exp
    t = fj.last_timings()
    assert t["fell_back"] == 0 and t["path"] == 0 and t["lds_retries"] == 2, t       # the oversized partition is re-partitioned alone (round 3)
    assert fj.hash_join_count_radix(bk, bk, pk)[0] == exp                      # the context is fine afterwards


@pytest.mark.parametrize("nb,dom,npk", [(1, 1, 1), (300, 40, 2000), (5000, 700, 60000), (60000, 9000, 300000), (1_000_000, 400_000, 3_000_000),
                                        (6_000_000, 3_000_000, 5_000_000)])
def test_many_to_many_extension_matches_the_numpy_oracle(fj, oracle, nb, dom, npk):
    """inner_join / inner_join_count (extension; the reference dedups build keys, hash_join.cpp:125): every duplicate build row
    yields a pair.  Counts and pair multisets vs the NumPy oracle, zero-, one- and two-pass plans, duplicates on both sides,
    keys 0 and 2^64-1 included; the reference-semantics functions on the same inputs still dedup."""
    rng = np.random.default_rng(nb + 7)
    ids = rng.integers(0, dom, size=nb, dtype=np.uint64)
    bk = ids * np.uint64(0x9E3779B97F4A7C15)
    bk[ids == 1] = np.uint64(2**64 - 1)                                       # the table's empty marker as a (duplicated) key
    bv = np.arange(nb, dtype=np.uint64) + np.uint64(5 * 10**12)               # value = row id: every row distinguishable
    pids = rng.integers(0, 2 * dom + 1, size=npk, dtype=np.uint64)
    pk = pids * np.uint64(0x9E3779B97F4A7C15)
    pk[pids == 1] = np.uint64(2**64 - 1)
    exp, ek, ev = oracle.np_inner_join(bk, bv, pk, return_arrays=True)
    n, sec = fj.inner_join_count(bk, bv, pk)
    assert isinstance(n, int) and isinstance(sec, float) and n == exp
    n, sec, k, v = fj.inner_join(bk, bv, pk, return_arrays=True)
    assert n == exp and k.size == exp
    a, b = oracle.canon_pairs(k, v), oracle.canon_pairs(ek, ev)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert fj.inner_join(bk, bv, pk)[0] == exp                                # (int, float) form
    assert fj.hash_join_count_radix(bk, bv, pk)[0] == oracle.np_join(bk, bv, pk)     # the reference's N:1 semantics are untouched
    import torch
    dk, dv, dp = (torch.from_numpy(x.view(np.int64)).cuda() for x in (bk, bv, pk))
    n2, _, k2, v2 = fj.inner_join(dk, dv, dp, return_arrays=True)             # device tensors
    assert n2 == exp and k2.numel() == exp
    a2 = oracle.canon_pairs(k2.cpu().numpy().view(np.uint64), v2.cpu().numpy().view(np.uint64))
    assert np.array_equal(a2[0], b[0]) and np.array_equal(a2[1], b[1])


def test_many_to_many_refuses_a_key_with_too_many_duplicates(fj):
    """More than 4096 build rows in one final partition (here: one key 6000 times) do not fit the kernel's LDS tables: a
    clear error, not a wrong result; the context stays usable."""
    bk = np.concatenate([np.full(6000, 12345, dtype=np.uint64), np.arange(100000, 100500, dtype=np.uint64)])
    bv = np.arange(bk.size, dtype=np.uint64)
    pk = np.array([12345, 100001, 7], dtype=np.uint64)
    with pytest.raises(RuntimeError, match="4096 build rows"):
        fj.inner_join_count(bk, bv, pk)
    assert fj.hash_join_count_radix(bk, bv, pk)[0] == 2


def test_concurrent_callers_on_one_device_are_serialised(fj):
    """Four Python threads issue counting, materialising and NumPy-entry joins on the same device at once (ctypes
    releases the GIL; the native contexts serialise their calls, SURVEY 8(b) threading row): every result exact."""
    import threading
    import torch
    from flash_hash_join_amd import datagen
    cases = []
    for i, (nb, npk) in enumerate([(5000, 300_000), (400_000, 3_000_000), (2_000_000, 9_000_000), (60_000, 1_000_000)]):
        bk, bv = datagen.build_device(nb, "cuda:0")
        pk, exp = datagen.probe_device(npk, nb, "cuda:0", seed=20 + i, hit_bp=3000 + 1500 * i)
        cases.append((bk, bv, pk, exp, tuple(x.cpu().numpy().view(np.uint64) for x in (bk, bv, pk))))
    M = torch.tensor(-7046029254386353131, dtype=torch.int64, device="cuda:0")
    errors = []

    def work(tid):
        try:
            for rep in range(6):
                bk, bv, pk, exp, host = cases[(tid + rep) % len(cases)]
                assert fj.hash_join_count_radix(bk, bv, pk)[0] == exp
                n, _, k, v = fj.adaptive_join(bk, bv, pk, return_arrays=True)
                assert n == exp and k.numel() == exp and bool(torch.all((v + 1) * M == k))
                assert fj.hash_join_count(*host)[0] == exp
        except Exception as ex:                                 # noqa: BLE001
            errors.append((tid, repr(ex)))
    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


@pytest.mark.parametrize("nb,dom,npk", [(50_000_000, 35_000_000, 200_000_000), (8_000_000, 1_000_000, 150_000_000)])
def test_two_pass_plans_with_duplicate_build_keys_against_a_device_side_oracle(fj, nb, dom, npk):
    """Sizes the CPU oracle does not reach in seconds: random 64-bit keys with duplicates on both sides, two-pass plans;
    expected count from sort + searchsorted on the device (torch), all count functions and the materialised pair count /
    membership; inner_join_count against the multiplicity sum."""
    import torch
    g = torch.Generator(device="cuda:0"); g.manual_seed(nb + npk)
    domain = torch.randint(-(1 << 62), 1 << 62, (dom,), dtype=torch.int64, device="cuda:0", generator=g) * 2 + 1   # odd keys
    bk = domain[torch.randint(0, dom, (nb,), device="cuda:0", generator=g)]
    bv = bk ^ 0x5555
    hit = torch.rand(npk, device="cuda:0", generator=g) < 0.35
    pk = torch.where(hit, domain[torch.randint(0, dom, (npk,), device="cuda:0", generator=g)],
                     torch.randint(-(1 << 62), 1 << 62, (npk,), dtype=torch.int64, device="cuda:0", generator=g) * 2)   # even keys never match
    del hit
    ub, mult = torch.unique(bk, return_counts=True)
    pos = torch.searchsorted(ub, pk).clamp(max=ub.numel() - 1)
    found = ub[pos] == pk
    exp = int(found.sum())
    exp_many = int(mult[pos][found].sum())
    del pos, found
    for fn in ("hash_join_count_radix", "hash_join_count", "adaptive_join_count", "hash_join_count_radix_bloom", "adaptive_join_count_bloom"):
        assert getattr(fj, fn)(bk, bv, pk)[0] == exp, fn
    assert fj.inner_join_count(bk, bv, pk)[0] == exp_many
    n, _, k, v = fj.hash_join_radix(bk, bv, pk, return_arrays=True)
    assert n == exp and k.numel() == exp and bool(torch.all((k ^ 0x5555) == v))          # every pair carries its key's value
    assert bool(torch.all(ub[torch.searchsorted(ub, k).clamp(max=ub.numel() - 1)] == k))
    assert torch.equal(torch.sort(k)[0], torch.sort(pk[ub[torch.searchsorted(ub, pk).clamp(max=ub.numel() - 1)] == pk])[0])


def test_workspace_can_be_trimmed_between_joins(fj, oracle):
    """fj_ctx_trim: the grow-only workspace goes back to the device, the next join re-grows it and gives the same result;
    refused while a stream join is open."""
    import torch
    from flash_hash_join_amd import api, datagen, _lib
    from flash_hash_join_amd.lab import LabEngine as HipEngine
    bk, bv = datagen.build_device(3_000_000, "cuda:0")
    pk, exp = datagen.probe_device(20_000_000, 3_000_000, "cuda:0", seed=2, hit_bp=5000)
    assert fj.hash_join_count_radix(bk, bv, pk)[0] == exp
    hbk, hbv, hpk = (x.cpu().numpy().view(np.uint64) for x in (bk[:200_000], bv[:200_000], pk[:1_000_000]))
    n_host = fj.hash_join_count(hbk, hbv, hpk)[0]                                   # the NumPy entry's own context
    before = api.workspace_bytes(0)
    assert before > 20_000_000 * 8
    free0 = torch.cuda.mem_get_info(0)[0]
    api.trim_workspace()
    assert api.workspace_bytes(0) == 0 and torch.cuda.mem_get_info(0)[0] >= free0 + before // 2
    assert fj.hash_join_count_radix(bk, bv, pk)[0] == exp and fj.hash_join_count(hbk, hbv, hpk)[0] == n_host
    n, _, k, v = fj.hash_join_radix(bk, bv, pk, return_arrays=True)
    assert n == exp and k.numel() == exp
    eng = HipEngine("cuda:0")
    eng.stream_begin(bk, bv, pk.numel(), 1, 64)
    with pytest.raises(RuntimeError, match="stream join is open"):
        api.trim_workspace(0)
    eng.stream_append(pk)
    assert eng.stream_finish() == exp
    api.trim_workspace(0)
    assert api.workspace_bytes(0) == 0


def test_c_abi_rejects_bad_arguments(fj):
    """Error behaviour at the C boundary: status 1 + fj_last_error text, translated to RuntimeError; the context stays usable."""
    import ctypes
    import torch
    from flash_hash_join_amd import _lib, api, datagen
    L = _lib.load()
    ctx = api.context(0)
    bk, bv = datagen.build_device(100_000, "cuda:0")
    pk, exp = datagen.probe_device(300_000, 100_000, "cuda:0", seed=2, hit_bp=5000)
    st = torch.cuda.current_stream(0).cuda_stream
    cnt = ctypes.c_uint64(0)
    t = _lib.FjTimings()

    def call(algo=2, bkp=None, pkp=None, top=64):
        return L.fj_join_device(ctx, algo, 0, 0, bk.data_ptr() if bkp is None else bkp, bv.data_ptr(), bk.numel(),
                                pk.data_ptr() if pkp is None else pkp, pk.numel(), st, top, ctypes.byref(cnt), None, None, 0, ctypes.byref(t))
    assert call(algo=9) == 1 and "unknown algo" in _lib.last_error()
    assert call(top=50) == 1 and "hash_top_bits" in _lib.last_error()
    assert call(bkp=bk.data_ptr() + 8) == 1 and "16-byte aligned" in _lib.last_error()
    assert call(pkp=0) == 1 and "null input pointer" in _lib.last_error()
    assert L.fj_join_device(None, 2, 0, 0, bk.data_ptr(), bv.data_ptr(), 1, pk.data_ptr(), 1, st, 64, ctypes.byref(cnt), None, None, 0, None) == 1
    assert call() == 0 and cnt.value == exp                                      # still works
    # materialise: emitting into too small a buffer is refused, the pending result survives for a second attempt
    assert L.fj_join_device(ctx, 2, 0, 1, bk.data_ptr(), bv.data_ptr(), bk.numel(), pk.data_ptr(), pk.numel(), st, 64,
                            ctypes.byref(cnt), None, None, 0, ctypes.byref(t)) == 0 and cnt.value == exp
    small_k = torch.empty(exp - 1, dtype=torch.int64, device="cuda:0"); small_v = torch.empty_like(small_k)
    assert L.fj_emit_pairs(ctx, small_k.data_ptr(), small_v.data_ptr(), exp - 1, st, ctypes.byref(t)) == 1 and "capacity" in _lib.last_error()
    ok_k = torch.empty(exp, dtype=torch.int64, device="cuda:0"); ok_v = torch.empty_like(ok_k)
    assert L.fj_emit_pairs(ctx, ok_k.data_ptr(), ok_v.data_ptr(), exp, st, ctypes.byref(t)) == 0
    M = torch.tensor(-7046029254386353131, dtype=torch.int64, device="cuda:0")
    assert bool(torch.all((ok_v + 1) * M == ok_k))
    assert L.fj_emit_pairs(ctx, ok_k.data_ptr(), ok_v.data_ptr(), exp, st, ctypes.byref(t)) == 1 and "no counted" in _lib.last_error()


def test_stream_join_rejects_misuse(fj):
    import torch
    from flash_hash_join_amd import datagen
    from flash_hash_join_amd.lab import LabEngine as HipEngine
    bk, bv = datagen.build_device(100_000, "cuda:0")
    pk, exp = datagen.probe_device(100_000, 100_000, "cuda:0", seed=1, hit_bp=5000)
    eng = HipEngine("cuda:0")
    eng.stream_open(100_000, 1, 100_000, 1, 64)
    eng.stream_append_build(bk)
    with pytest.raises(RuntimeError, match="more pieces"):
        eng.stream_append_build(bk)
    eng.stream_append(pk)
    eng.stream_advance_probe()
    with pytest.raises(RuntimeError, match="closed"):
        eng.stream_append(pk)
    assert eng.stream_finish() == exp
    with pytest.raises(RuntimeError, match="no stream join"):
        eng.stream_append(pk)
    # a stream join that is never finished occupies the context until it is aborted; the next plan starts from clean buffers
    big_bk, big_bv = datagen.build_device(3_000_000, "cuda:0")
    big_pk, big_exp = datagen.probe_device(8_000_000, 3_000_000, "cuda:0", seed=3, hit_bp=5000)
    eng.stream_begin(big_bk, big_bv, 2 * big_pk.numel(), 2, 64)
    eng.stream_append(big_pk)                                                     # first pass ran: chunk counts are left behind
    with pytest.raises(RuntimeError, match="stream join is open"):
        fj.hash_join_count_radix(bk, bv, pk)
    with pytest.raises(RuntimeError, match="stream join is open"):
        eng.bloom_export(bk, 64)
    eng.stream_abort()
    eng.stream_abort()                                                            # no-op when nothing is open
    assert fj.hash_join_count_radix(big_bk, big_bv, big_pk)[0] == big_exp
    assert fj.hash_join_count_radix(bk, bv, pk)[0] == exp
    # stale chunk counts of an abandoned plan must not reach a LATER plan that uses more of the self-cleaning buffers than the
    # plan right after the abort did: abort a two-pass stream, run a small one-pass join (32 buckets), then wide / deep ones
    eng.stream_begin(big_bk, big_bv, 2 * big_pk.numel(), 2, 64)
    eng.stream_append(big_pk)
    eng.stream_abort()
    small_bk, small_bv = datagen.build_device(60_000, "cuda:0")
    small_pk, small_exp = datagen.probe_device(500_000, 60_000, "cuda:0", seed=5, hit_bp=5000)
    assert fj.hash_join_count_radix(small_bk, small_bv, small_pk)[0] == small_exp
    mid_bk, mid_bv = datagen.build_device(1_000_000, "cuda:0")
    mid_pk, mid_exp = datagen.probe_device(4_000_000, 1_000_000, "cuda:0", seed=6, hit_bp=5000)
    assert fj.hash_join_count_radix(mid_bk, mid_bv, mid_pk)[0] == mid_exp                 # one 256-bucket pass
    assert fj.hash_join_count_radix(big_bk, big_bv, big_pk)[0] == big_exp                 # two passes, both ping-pong slots
    del small_bk, small_bv, small_pk, mid_bk, mid_bv, mid_pk
    # the multi-GPU driver aborts by itself when an engine call fails mid-stream
    import torch.distributed as dist
    import socket
    from flash_hash_join_amd.distributed import distributed_join

    class Failing(HipEngine):
        def local_join(self, *a, **kw):
            raise RuntimeError("injected failure in the owner's local join")

    s_ = socket.socket(); s_.bind(("127.0.0.1", 0)); port = s_.getsockname()[1]; s_.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    dj = lambda *a, **kw: distributed_join(*a, force_exchange=True, **kw)
    try:
        os.environ["FJ_DIST_STRATEGY"] = "scatter"                           # the owner-scatter rung runs the engine's hooks from Python
        with pytest.raises(RuntimeError, match="injected failure"):
            dj(big_bk, big_bv, big_pk, engine=Failing("cuda:0"))
        assert dj(big_bk, big_bv, big_pk)[0] == big_exp                      # the context is free again
        # ... and so does the C++ driver of the chunk form (csrc/fj_dist.hip): a local append that fails (test hook) is agreed on in the
        # final all-reduce, the stream join is dropped, every rank raises; without FJ_DIST_NO_FALLBACK the ranks move down to the owner-scatter rung
        os.environ["FJ_DIST_STRATEGY"] = "shuffle"; fj.set_option("lab_hooks", 2); os.environ["FJ_DIST_NO_FALLBACK"] = "1"      # FJ_HOOK_INJECT_FAIL
        with pytest.raises(RuntimeError, match="the local join failed on 1 rank.*injected failure of a local append"):
            dj(big_bk, big_bv, big_pk)
        os.environ.pop("FJ_DIST_NO_FALLBACK")
        t = {}
        assert dj(big_bk, big_bv, big_pk, timings=t)[0] == big_exp and t["shuffle_form"] == "owner-scatter" and "injected" in t["chunk_form_error"]
        fj.set_option("lab_hooks", 0)
        t = {}
        assert dj(big_bk, big_bv, big_pk, timings=t)[0] == big_exp and t["shuffle_form"].startswith("chunks") and "chunk_form_error" not in t
    finally:
        for k_ in ("FJ_DIST_STRATEGY", "FJ_DIST_NATIVE", "FJ_DIST_NO_FALLBACK"):
            os.environ.pop(k_, None)
        fj.set_option("lab_hooks", 0)
        dist.destroy_process_group()


# FJ_FUZZ_SEEDS="a-b" adds seeds for a longer campaign (the committed default stays at 24 seeds x 4 dispatch modes)
_FUZZ_EXTRA = os.environ.get("FJ_FUZZ_SEEDS", "")
_FUZZ_SEEDS = list(range(24)) + (list(range(int(_FUZZ_EXTRA.split("-")[0]), int(_FUZZ_EXTRA.split("-")[1]))) if "-" in _FUZZ_EXTRA else [])


@pytest.mark.parametrize("seed", _FUZZ_SEEDS)
def test_fuzz_against_oracle(fj, oracle, seed, scalar_mode):
    """Random sizes and key distributions (uniform, tiny domains with heavy duplication, sequential, skewed),
    duplicate build keys carrying equal values; every count function and the radix/scalar pair sets vs the oracle."""
    rng = np.random.default_rng(9000 + seed)
    nb = int(rng.choice([1, 7, 300, 4096, 4097, 9000, 70000, 200000, 1200000]))
    npk = int(rng.choice([1, 5, 1000, 33333, 250000, 1500000]))
    kind = seed % 4
    if kind == 0:                       # uniform 64-bit
        bk = rng.integers(0, 2**64, size=nb, dtype=np.uint64)
        pk = np.concatenate([rng.choice(bk, npk // 2 + 1), rng.integers(0, 2**64, size=npk // 2, dtype=np.uint64)])
    elif kind == 1:                     # tiny domain: massive duplication on both sides
        dom = int(rng.choice([3, 50, 5000]))
        bk = rng.integers(0, dom, size=nb, dtype=np.uint64)
        pk = rng.integers(0, 2 * dom, size=npk, dtype=np.uint64)
    elif kind == 2:                     # sequential ids, probe range twice as wide
        bk = rng.permutation(np.arange(nb, dtype=np.uint64))
        pk = rng.integers(0, 2 * nb + 1, size=npk, dtype=np.uint64)
    else:                               # skew: one hot key plus a uniform tail, 0 and 2^64-1 present
        bk = np.unique(np.concatenate([rng.integers(0, 2**64, size=nb, dtype=np.uint64), np.array([0, 2**64 - 1], dtype=np.uint64)]))
        hot = np.full(npk // 2, bk[rng.integers(0, bk.size)], dtype=np.uint64)
        pk = np.concatenate([hot, rng.integers(0, 2**64, size=npk - npk // 2, dtype=np.uint64), np.array([0, 2**64 - 1], dtype=np.uint64)])
    bv = bk * np.uint64(2654435761) + np.uint64(17)          # value is a function of the key: duplicates agree
    pk = rng.permutation(pk)
    exp, ek, ev = oracle.np_join(bk, bv, pk, return_arrays=True)
    for fn in COUNT_FUNCS:
        assert getattr(fj, fn)(bk, bv, pk)[0] == exp, (fn, seed, nb, npk, kind)
    for fn in ("hash_join_radix", "hash_join", "adaptive_join_bloom"):
        n, _, k, v = getattr(fj, fn)(bk, bv, pk, return_arrays=True)
        assert n == exp, (fn, seed)
        a, b = oracle.canon_pairs(k, v), oracle.canon_pairs(ek, ev)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (fn, seed, nb, npk, kind)


@pytest.mark.parametrize("nb,dom,npk", [(3000, 700, 20000), (60000, 9000, 200000), (500000, 120000, 900000), (3000000, 1000000, 4000000),
                                        (20_000_000, 6_000_000, 12_000_000)])      # 8192 partitions: the persistent counting kernel reports the duplicates
def test_duplicate_build_keys_first_occurrence_wins(fj, oracle, nb, dom, npk, scalar_mode):
    """Duplicate build keys with DIFFERENT values: the radix/adaptive joins must emit the value of the FIRST occurrence
    (the reference's radix path: stable partition + insert_local, hash_join.cpp:125 / SURVEY App. B); the scalar path is
    racy in the reference too, there any occurrence's value is acceptable."""
    rng = np.random.default_rng(nb)
    ids = rng.integers(0, dom, size=nb, dtype=np.uint64)
    bk = ids * np.uint64(0x9E3779B97F4A7C15) + np.uint64(3)
    bv = np.arange(nb, dtype=np.uint64) + np.uint64(10**12)                 # value = row id: every occurrence differs
    pk = rng.integers(0, 2 * dom, size=npk, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(3)
    exp, ek, ev = oracle.np_join(bk, bv, pk, return_arrays=True)            # first occurrence wins
    ref = oracle.canon_pairs(ek, ev)
    for fn in ("hash_join_radix", "adaptive_join", "hash_join_radix_bloom", "adaptive_join_bloom"):
        n, _, k, v = getattr(fj, fn)(bk, bv, pk, return_arrays=True)
        got = oracle.canon_pairs(k, v)
        assert n == exp and np.array_equal(got[0], ref[0]), fn
        assert np.array_equal(got[1], ref[1]), (fn, "value of a duplicated build key is not its first occurrence's")
    n, _, k, v = fj.hash_join(bk, bv, pk, return_arrays=True)               # scalar path: some occurrence of the right key
    assert n == exp and np.array_equal(np.sort(k), ref[0])
    assert np.array_equal(bk[(v - np.uint64(10**12)).astype(np.int64)], k)


@pytest.mark.parametrize("tool,args,expect", [
    ("r6_wide_fuzz.py", ["30", "101"], "OK: 30 cases"),                    # shapes of the bucketed join, duplicates up to millions of copies
    ("r6_api_fuzz.py", ["150", "102", "2", "6.8"], "OK: 150 cases"),       # the twelve functions + inner_join_count, random options, special keys, edge sizes
    ("r6_host_fuzz.py", ["60", "103"], "OK: 60 cases"),                    # the NumPy entry: int64 / uint64, strided, N-D, empty
    ("r6_bcast_fuzz.py", ["40", "104"], "OK: 40 joins"),                   # the multi-GPU ladder from the broadcast rung on one rank over RCCL
    ("r6_threads_fuzz.py", ["4", "20", "105"], "OK: 4 threads"),           # several Python threads on one context
    ("r6_ranks_fuzz.py", ["2", "6", "106"], "OK: 2 ranks on one GPU"),     # two ranks sharing this GPU over gloo: ragged / empty blocks, duplicates across ranks
])
def test_random_inputs(fj, tool, args, expect):
    """Round 6's random-input tools (EXPERIMENTS.md "Fuzzing": they found the double-counted re-partitioned partition and the
    one-repeated-key failure of the tagged table), a short fixed-seed run of each: every count against torch.isin / numpy.isin, every
    pair against the first-occurrence rule on one GPU (hash_join.cpp:125) and the some-copy rule across GPUs."""
    import subprocess
    import sys
    from conftest import ROOT
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool)] + args, capture_output=True, text=True, timeout=900, cwd=os.path.join(ROOT, "tools"))
    assert out.returncode == 0 and expect in out.stdout, out.stdout[-1500:] + out.stderr[-2500:]
