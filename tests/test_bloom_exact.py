"""The bloom precheck on an MI355X, bit for bit, in all three filter variants: every exported filter word, every surviving key and the
survivor count of the in-join stage against the NumPy model of tests/bloom_model.py - equalities only, no tolerance anywhere.  Public
API and LabEngine only.

The inputs, what each of them can tell apart (the seeded defects (a) - (d)) and the proof that the crafted shapes reach the corners of
the filter kernel's workgroup split are tests/test_bloom_exact_cpu.py; its docstring lists the build and probe sides.

  A  test_exported_filters       LabEngine.bloom_export, 512 x 35840 words and the header word, compared on the device
                                 (fj_bloom_export_kernel<VAR>, bf_build_filter, bf_insert, bf_bits)
  B  test_tiny_probe_sides,      LabEngine.bloom_prefilter: sorted survivors == the model's sorted survivors
     test_survivors, test_stale_tails, test_second_slab, test_filters_of_variant_1_are_refused_by_the_others
                                 (fj_bloom_filter_kernel<VAR> with prebuilt filters, bf_fetch, bf_pass, fj_bucket_base_kernel, fj_flatten_kernel)
  C  test_in_join_stage          hash_join_count_radix_bloom and hash_join_radix_bloom under plan_target_keys = 16: count and pairs
                                 against NumPy, filter_survivors == the model's count over the plan's level-1 buckets (the in-kernel
                                 bf_build_filter, prebuilt == NULL)
bloom_variant and plan_target_keys are set through the `opts` fixture, which puts both back after every test.

test_second_slab sizes its probe side from the chip's workgroup count: 1.5 x G x 16 waves x BF_SLAB x 256 keys (201M at 256 compute
units), so that every wave keeps more than one slab of output chunks; it checks sort(kept) == sort(probe) on the device and needs no
model.  It is skipped where less than 16 x its key bytes of device memory are free.

TIMES on an MI355X machine (pytest --durations=0, one run; 256 compute units): this file, 102 tests, 6.5 s in all.  1.7 s of that is
the setup of the first test (loading the library); the slowest calls are test_survivors[all_hits-0-64] 0.14 s (the first upload),
test_in_join_stage 0.06 - 0.14 s each, test_exported_filters 0.01 - 0.14 s, test_survivors[hits_1to7] 0.08 s, test_tiny_probe_sides
0.01 - 0.06 s, test_stale_tails 0.02 - 0.05 s and test_second_slab (201 326 592 keys) 0.05 s.  The NumPy model of a case costs more than
its kernels: tests/test_bloom_exact_cpu.py, which builds every input and model once more, takes 20 s on one CPU core.

WOULD THEY FAIL?  Once, while this file was written, it ran against five scratch builds of the library with one seeded defect each (all
of them stay inside LDS and the pools), and failed as it should:
  bf_pass without the mhi test          30 fail: test_survivors hits_1to1 / hits_1to7 / one_bucket / ends / partial, test_stale_tails and
                                        test_in_join_stage at 0 % and 5 % hits, each under VAR 0 and 2 only; everything of VAR 1, every
                                        export, all_hits, empty, the tiny probe sides and 100 % hits pass
  bf_bits<0>: (w >> 5) read as (w >> 6) 32 fail: every VAR 0 case of test_exported_filters and, through their filters, of the prefilter
                                        tests; test_in_join_stage[skewed] at 0 % and 5 % hits under VAR 0; VAR 1 and 2 pass
  bf_build_filter drops the inserts of  100 fail: every export, every prefilter test (test_second_slab included) and 16 of the 18 in-join
  its first step                        cases; test_in_join_stage[holes-0-0] and [holes-0-2] pass (no survivor with or without the step)
  flush stores `lane + 1 < n`           51 fail (parts A and B were run): every test that calls bloom_prefilter; every export passes
  seg_keys never accumulated            52 fail: every test that calls bloom_prefilter, by the library's own check ("internal error:
                                        prefilter flattened 0 of 40000 survivors"); the exports and the in-join stage, which does not
                                        count keys per bucket, pass
"""
import functools

import numpy as np
import pytest

import bloom_model as BM
import test_bloom_exact_cpu as C

pytestmark = pytest.mark.gpu
DEFAULTS = {"bloom_variant": 0, "plan_target_keys": 4096}
COMBOS = [(var, top) for var in BM.VARIANTS for top in C.TOPS]


@pytest.fixture(scope="module")
def fj():
    import flash_join
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_device_count() >= 1, "no HIP device: the product path must not silently fall back"
    assert flash_join.initialize() is None
    for name, value in DEFAULTS.items():
        assert flash_join.get_option(name) == value, f"option {name} is not at its default"
    return flash_join


@pytest.fixture
def opts(fj):
    """set(name, value); bloom_variant and plan_target_keys are back at their defaults after the test"""
    yield fj.set_option
    for name, value in DEFAULTS.items():
        fj.set_option(name, value)


@pytest.fixture(scope="module")
def eng(fj):
    from flash_hash_join_amd.lab import LabEngine
    return LabEngine("cuda:0")


@pytest.fixture(scope="module")
def G():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _assert_filters(got, want_np, what):
    import torch
    want = torch.from_numpy(want_np).cuda()
    assert got.dtype == torch.int32 and got.numel() == want.numel() == 512 * BM.WORDS + 4, what
    if torch.equal(got, want):
        return
    at = torch.nonzero(got != want).flatten()
    i = int(at[0])
    g, w = int(got[i]) & 0xFFFFFFFF, int(want[i]) & 0xFFFFFFFF
    where = f"bucket {i // BM.WORDS}, word {i % BM.WORDS}" if i < 512 * BM.WORDS else f"header word {i - 512 * BM.WORDS}"
    raise AssertionError(f"{what}: {at.numel()} words differ; the first: {where}: got {g:#010x}, the model {w:#010x}, xor {g ^ w:#010x}")


def _assert_survivors(kept, want, what, top_bits):
    """kept: the int64 tensor bloom_prefilter returned; want: the model's survivors (uint64, any order)"""
    import torch
    want_sorted = np.sort(np.ascontiguousarray(want).view(np.int64))
    got = torch.sort(kept)[0]
    if got.numel() == want_sorted.size and torch.equal(got, torch.from_numpy(want_sorted).cuda()):
        return
    g, w = got.cpu().numpy().view(np.uint64), want_sorted.view(np.uint64)
    gu, gc = np.unique(g, return_counts=True)
    wu, wc = np.unique(w, return_counts=True)
    missing = np.setdiff1d(wu, gu)
    extra = np.setdiff1d(gu, wu)
    both = np.intersect1d(gu, wu)
    miscounted = both[gc[np.searchsorted(gu, both)] != wc[np.searchsorted(wu, both)]]
    raise AssertionError(f"{what}: {g.size} survivors, the model {w.size}; {missing.size} keys missing (first {[hex(int(x)) for x in missing[:4]]}, buckets "
                         f"{BM.bucket_of(missing[:4], 9, top_bits).tolist()}), {extra.size} keys not expected (first {[hex(int(x)) for x in extra[:4]]}), "
                         f"{miscounted.size} with another multiplicity")


@pytest.fixture(scope="module")
def exported(fj, eng):
    """(build side, variant, top_bits) -> the filters bloom_export gave under that variant, checked against the model once"""
    cache = {}

    def get(name, var, top_bits):
        key = (name, var, top_bits)
        if key not in cache:
            assert fj.get_option("bloom_variant") == var
            build = C.build_side(name, top_bits)
            got = eng.bloom_export(_dev(build), top_bits)
            want = np.empty(512 * BM.WORDS + 4, dtype=np.uint32)
            want[:-4] = C.model_filters(name, var, top_bits).reshape(-1)
            want[-4:] = (BM.HDR_MAGIC | var, 0, 0, 0)
            _assert_filters(got, want.view(np.int32), f"bloom_export of `{name}`, variant {var}, top_bits {top_bits}")
            cache[key] = got
        return cache[key]
    yield get
    cache.clear()


# ---- A. exported filters, word for word ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_bits", C.TOPS)
@pytest.mark.parametrize("name,var", C.EXPORT_CASES, ids=[f"{n}-{v}" for n, v in C.EXPORT_CASES])
def test_exported_filters(fj, opts, eng, exported, name, var, top_bits):
    opts("bloom_variant", var)
    exported(name, var, top_bits)
    if name == "one":                                            # no build key at all: zero filters under the same header
        none = eng.bloom_export(_dev(np.zeros(0, dtype=np.uint64)), top_bits)
        _assert_filters(none, BM.exported(np.zeros(0, dtype=np.uint64), var, top_bits), f"bloom_export of no key, variant {var}")


# ---- B. survivors, key for key ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("var,top_bits", COMBOS)
def test_tiny_probe_sides(fj, opts, eng, exported, var, top_bits):
    """(i) one key that passes, one that does not, and 63 .. 257 keys of one bucket that all pass: pieces of 63, 64 and 65 keys in a
    wave's staging row, a chunk filled to exactly 256 keys, a second chunk of one"""
    opts("bloom_variant", var)
    filt = exported("three", var, top_bits)
    for name in C.TINY:
        bname, probe = C.probe_side(name, var, top_bits)
        assert bname == "three"
        kept = eng.bloom_prefilter(_dev(probe), filt, top_bits)
        _assert_survivors(kept, C.expected_survivors(name, var, top_bits), f"{name}, variant {var}, top_bits {top_bits}", top_bits)


SURVIVOR_CASES = [(n, v, t) for n in ("all_hits", "hits_1to1", "hits_1to7", "one_bucket", "ends", "partial", "empty") for v in C.probe_variants(n) for t in C.TOPS]


@pytest.mark.parametrize("name,var,top_bits", SURVIVOR_CASES)
def test_survivors(fj, opts, eng, exported, G, name, var, top_bits):
    """(ii) all_hits: every key survives - the slot-by-slot ring branch, chunks filled exactly; hits_1to1 / hits_1to7: both ring branches.
    (iii) one_bucket: many workgroups share a bucket, a segment each; ends: toff with runs of equal entries - the shape proofs run with
    this chip's workgroup count.  (iv) partial: misses that share the block and some bits of a build key, and a saturated block.
    (vi) empty: probe keys in buckets whose filter is empty, beside buckets that keep everything."""
    opts("bloom_variant", var)
    if name in ("one_bucket", "ends"):
        C.prove_shapes(G)
    bname, probe = C.probe_side(name, var, top_bits, G)
    kept = eng.bloom_prefilter(_dev(probe), exported(bname, var, top_bits), top_bits)
    _assert_survivors(kept, C.expected_survivors(name, var, top_bits, G), f"{name}, variant {var}, top_bits {top_bits}", top_bits)


@pytest.mark.parametrize("var,top_bits", COMBOS)
def test_stale_tails(fj, opts, eng, exported, var, top_bits):
    """(v) behind a 2M-key call whose keys all pass, 1 000 misses in short chunks of odd counts: exactly the model's survivors - nothing
    the first call left in the pools leaks out of a chunk's tail"""
    import torch
    opts("bloom_variant", var)
    filt = exported("big", var, top_bits)
    first = _dev(C.stale_first_call(top_bits))
    kept = eng.bloom_prefilter(first, filt, top_bits)
    assert kept.numel() == first.numel() and torch.equal(torch.sort(kept)[0], torch.sort(first)[0])
    _, probe = C.probe_side("stale", var, top_bits)
    kept = eng.bloom_prefilter(_dev(probe), filt, top_bits)
    _assert_survivors(kept, C.expected_survivors("stale", var, top_bits), f"stale, variant {var}, top_bits {top_bits}", top_bits)


def test_second_slab(fj, opts, eng, G):
    """(vii) every wave of every workgroup keeps more than BF_SLAB * 256 keys, so each takes a second slab of output chunks: probe ==
    build keys of the device generator, everything survives"""
    import torch
    from flash_hash_join_amd import datagen
    c = C.constants()
    waves = c["BF_NT"] // 64
    n = 3 * G * waves * c["BF_SLAB"] * C.CHUNK // 2
    if torch.cuda.mem_get_info(0)[0] < 16 * 8 * n:
        pytest.skip(f"{n} keys: less than {16 * 8 * n >> 30} GiB of device memory free")
    opts("bloom_variant", 0)
    keys, vals = datagen.build_device(n, "cuda:0")
    del vals
    filt = eng.bloom_export(keys, 64)
    kept = eng.bloom_prefilter(keys, filt, 64)
    assert kept.numel() == n
    assert torch.equal(torch.sort(kept)[0], torch.sort(keys)[0])
    del keys, kept, filt
    torch.cuda.empty_cache()


def test_filters_of_variant_1_are_refused_by_the_others(fj, opts, eng, exported):
    opts("bloom_variant", 1)
    filt = exported("three", 1, 64)
    probe = _dev(C.build_side("three", 64))
    assert eng.bloom_prefilter(probe, filt, 64).numel() == probe.numel()
    for other in (0, 2):
        opts("bloom_variant", other)
        with pytest.raises(RuntimeError, match="bloom_variant"):
            eng.bloom_prefilter(probe, filt, 64)
    opts("bloom_variant", 1)
    assert eng.bloom_prefilter(probe, filt, 64).numel() == probe.numel()


# ---- C. the in-join stage -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _join_inputs(build_name, hit_bp):
    return tuple(_dev(a) for a in C.join_case(build_name, hit_bp))


@pytest.mark.parametrize("var", BM.VARIANTS)
@pytest.mark.parametrize("hit_bp", C.JOIN_HITS)
@pytest.mark.parametrize("build_name", C.JOIN_BUILDS)
def test_in_join_stage(fj, opts, build_name, hit_bp, var):
    """the filter built inside the kernel from the build side's level-1 chunks: a bucket of three steps (skewed), buckets without a
    build chunk that probe keys reach (holes), at 0 %, 5 % and 100 % hits"""
    opts("bloom_variant", var)
    opts("plan_target_keys", 16)
    bk, bv, pk = C.join_case(build_name, hit_bp)
    dbk, dbv, dpk = _join_inputs(build_name, hit_bp)
    n_ref, k_ref, v_ref = C.join_reference(build_name, hit_bp)
    good_keys = C.constants()["FJ_BLOOM_GOOD_KEYS"]

    def check_stage(fn):
        t = fj.last_timings()
        assert t["passes"] == 2 and t["bloom_level"] == 1 and t["fell_back"] == 0, (fn, t)
        l1 = BM.level1_bits(t["radix_bits"])
        assert l1 == C.L1_BITS and (bk.size >> l1) <= good_keys, f"{fn}: radix_bits {t['radix_bits']}: the plan was rebalanced or split otherwise"
        want = BM.survivor_count(bk, pk, var, 64, l1)
        assert t["filter_survivors"] == want, f"{fn}: filter_survivors {t['filter_survivors']}, the model {want} ({n_ref} hits of {pk.size} probe rows)"

    n, _ = fj.hash_join_count_radix_bloom(dbk, dbv, dpk)
    assert n == n_ref
    check_stage("hash_join_count_radix_bloom")
    n, _, k, v = fj.hash_join_radix_bloom(dbk, dbv, dpk, return_arrays=True)
    assert n == n_ref and k.numel() == n_ref and v.numel() == n_ref
    check_stage("hash_join_radix_bloom")
    k, v = k.cpu().numpy().view(np.uint64), v.cpu().numpy().view(np.uint64)
    o = np.lexsort((v, k))
    assert np.array_equal(k[o], k_ref) and np.array_equal(v[o], v_ref)
