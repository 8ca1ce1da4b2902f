"""The bloom precheck, bit for bit - the part that needs no GPU: the NumPy model's self-checks (tests/bloom_model.py), the inputs of
every case of tests/test_bloom_exact.py (built HERE, so that both files see the same arrays), the proof that each input tells the
seeded defects below from the correct model, the proof that the crafted shapes reach the filter kernel's corners for the chip's
workgroup count, and the constants of the sources that all of this is derived from, pinned by name.

THE SEEDED DEFECTS (what a wrong kernel could do while today's count-and-bound tests stay green)
  (a) bf_pass ignores mhi                                     -> a miss that passes mlo and fails mhi must be among the probe keys
  (b) one bit position of bf_bits is read one bit higher      -> an exported filter word must differ
  (c) the exporter leaves out one 32-chunk step of a bucket   -> the bucket has that many steps, and fewer than 8192 of its keys lack a
      (first, second, third, last)                               bit of their own: whichever 8192 keys a step held, the filter differs
                                                                 (which key lands in which chunk is the partition pass's business)
  (d) a survivor is dropped per flush of a partial piece      -> the case has survivors whose number per wave is no multiple of 64;
                                                                 every case with at least one survivor has a flush that is counted
DETECTS lists, per case, the defects it is a test of; a case that cannot tell a defect from the correct model is not listed for it.

BUILD SIDES (build_side(name, top_bits); buckets are those of the 9-bit sender-side precheck at that hash_top_bits)
  one        1 key                                   sparse300  300 random keys: most buckets empty
  three      40 000 keys in buckets 0, 255, 511      dups       `three`, every key 3 times, shuffled
  big        bucket 77: 70 000 keys (>= 274 chunks, >= 9 steps: every stage of bf_build_filter's load pipeline and its clamped tail);
             buckets 10..13: 8191, 8192, 8193, 16 385 keys (around one and two steps); 5 000 keys spread over all buckets
  saturated  VAR 0: bucket 200: 5 000 keys on ONE 64-bit block (all 64 bits set); bucket 201: 64 keys, key i alone in block 280 * i with
             a known low word
PROBE SIDES (probe_side(name, var, top_bits, G) -> build side's name, probe keys)
  tiny_*     1 key that passes, 1 that does not, 63 / 64 / 65 / 255 / 256 / 257 keys of one bucket, all passing
  all_hits   the build keys of `big`; hits_1to1 / hits_1to7: interleaved with misses crafted into the same buckets
  one_bucket ~300 000 keys in bucket 77 of `big` (37 tiles at G = 256; tiles_for(G) otherwise), a third of them hits
  ends       ~300 000 keys in buckets 0, 255 and 511 of `three`: toff has runs of equal entries
  partial    VAR 0 on `saturated`: twins of the 64 known keys with the same low word (pass), with one of the mlo positions moved
             (fail), with the last mhi position moved (pass mlo, fail mhi); 2 000 misses on the saturated block (all pass) and 500
             elsewhere in its bucket (none passes)
  stale      1 000 misses with short, odd chunk counts, 40 of them false positives, behind a 2M-key call whose keys all pass
  empty      `three`'s keys and their twins in buckets 1, 254, 256, 510, whose filters are empty
"""
import functools
import os
import re
import shutil

import numpy as np
import pytest

import bloom_model as BM
import keymix
from conftest import ROOT

HERE = "tests/test_bloom_exact_cpu.py"
CSRC = os.path.join(ROOT, "flash_hash_join_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
TOPS = (64, 48)
STEP_KEYS, CHUNK, TILE_CHUNKS = 8192, 256, 32
SAT_BUCKET, SAT_BLOCK, KNOWN_BUCKET, KNOWN_STRIDE = 200, 4321, 201, 280
BIG_BUCKET, BIG_KEYS = 77, 70_000
STEP_BUCKETS = {10: 8191, 11: 8192, 12: 8193, 13: 16_385}
ENDS = (0, 255, 511)
EMPTY_NEIGHBOURS = (1, 254, 256, 510)
SHIFT_DEFECTS = ((1, 5, 9, 13), (0, 6, 9, 13), (0, 5, 10, 13), (0, 5, 9, 14))
_U = np.uint64


# ---- the constants, read from the sources ------------------------------------------------------------------------------------------------
def _source(csrc, name):
    with open(os.path.join(csrc, name)) as f:
        return f.read()


def _gone(what, pattern):
    return f"{what}: the sources no longer say /{pattern}/ - {HERE} and tests/bloom_model.py are written against it: read the new text, then update"


def _num(text, pattern, what):
    m = re.search(pattern, text)
    assert m, _gone(what, pattern)
    return int(m.group(1), 0)


def _says(text, fragment, what):
    assert fragment in text, _gone(what, fragment)


def constants(csrc=CSRC, include=INCLUDE):
    c = {}
    common, bloom, dev = _source(csrc, "fj_common.h"), _source(csrc, "fj_bloom.hip"), _source(csrc, "fj_bloom_dev.h")
    host, plan, internal = _source(csrc, "fj_host.h"), _source(csrc, "fj_plan.hip"), _source(csrc, "fj_internal.h")
    c["FJ_BLOOM_WORDS"] = _num(common, r"#define\s+FJ_BLOOM_WORDS\s+(\d+)u", "FJ_BLOOM_WORDS")
    c["FJ_PREFILTER_BITS"] = _num(common, r"#define\s+FJ_PREFILTER_BITS\s+(\d+)", "FJ_PREFILTER_BITS")
    c["FJ_MAX_FAN_LOG"] = _num(common, r"#define\s+FJ_MAX_FAN_LOG\s+(\d+)", "FJ_MAX_FAN_LOG")
    c["FJ_BLOOM_GOOD_KEYS"] = _num(common, r"#define\s+FJ_BLOOM_GOOD_KEYS\s+(\d+)u", "FJ_BLOOM_GOOD_KEYS")
    c["FJ_BLOOM_HDR_MAGIC"] = _num(internal, r"#define\s+FJ_BLOOM_HDR_MAGIC\s+(0x[0-9A-Fa-f]+)u", "FJ_BLOOM_HDR_MAGIC")
    c["BF_NT"] = _num(dev, r"constexpr u32 BF_NT = (\d+);", "BF_NT")
    c["BF_KPT"] = _num(bloom, r"constexpr u32 BF_KPT = (\d+);", "BF_KPT")
    c["BF_STG"] = _num(bloom, r"constexpr u32 BF_STG = (\d+);", "BF_STG")
    c["BF_SLAB"] = _num(bloom, r"constexpr u32 BF_SLAB = (\d+);", "BF_SLAB")
    c["FJ_BLOOM_SNAP16"] = _num(bloom, r"#define FJ_BLOOM_SNAP16 (\d+)\n", "FJ_BLOOM_SNAP16")
    # the text the model restates
    _says(dev, "byte_off = __umulhi(w, FJ_BLOOM_WORDS / 2u) * 8u;\n        mlo = (1u << (w & 31u)) | (1u << ((w >> 5) & 31u));\n"
               "        mhi = (1u << ((w >> 9) & 31u)) | (1u << ((w >> 13) & 31u));", "bf_bits<0>")
    _says(dev, "u32 x = (u32)key ^ __builtin_rotateleft32((u32)(key >> 32), 15);\n    x *= 0x9E3779B1u; x ^= x >> 15;\n"
               "    x *= 0x85EBCA77u; x ^= x >> 13;", "the mixer of bf_bits<1> and <2>")
    _says(dev, "byte_off = __umulhi(x, FJ_BLOOM_WORDS) * 4u;\n        mlo = (1u << (x & 31u)) | (1u << ((x >> 5) & 31u));\n        mhi = 0;", "bf_bits<1>")
    _says(dev, "return (wlo & mlo) == mlo && (VAR == 1 || (whi & mhi) == mhi);", "bf_pass")
    _says(bloom, "const u32 b0 = toff[lo], b1 = toff[lo + 1], slack = ((b1 - b0) * BF_SNAP16) >> 4;\n"
                 "            if (t - b0 <= slack) t = b0; else if (b1 - t <= slack) t = b1;", "boundary()")
    _says(bloom, "u32 t = (u32)(((u64)gg * ntiles) / G);", "boundary()")
    _says(bloom, "constexpr u32 BF_T = BF_NT * BF_KPT;", "the filter kernel's tile")
    # the split of a plan's bits: extra bits to the EARLIER passes, and when a bloom plan moves bits into its first pass
    _says(plan, "int plan_npass(int bits) { return bits <= FJ_MAX_FAN_LOG ? (bits > 0 ? 1 : 0) : (bits <= 2 * FJ_MAX_FAN_LOG ? 2 : "
                "(bits + FJ_MAX_FAN_LOG - 1) / FJ_MAX_FAN_LOG); }", "plan_npass")
    _says(plan, "p.fan_log[i] = p.bits / p.npass + ((extra_first ? i < rem : i >= p.npass - rem) ? 1 : 0);", "plan_passes")
    _says(plan, "plan_passes(p, true);\n    if (want_bloom && p.npass >= 2) {", "make_plan")
    _says(plan, "(nb >> p.fan_log[0]) > FJ_BLOOM_GOOD_KEYS) { ++p.fan_log[0]; --p.fan_log[1]; }", "make_plan's rebalancing")
    # partial chunks of the 9-bit pass in front of the filter: at most one per (workgroup, bucket), rows / (512 * 128) workgroups
    _says(plan, "const u64 g64 = std::min<u64>(chunks / tile_chunks, rows / ((u64)F * 128));", "pass_groups")
    # the default variant: the code, and what the header tells a caller
    c["variant_code"] = _num(host, r"int bloom_variant = (\d+),", "Options::bloom_variant")
    c["variant_doc"] = _num(_source(include, "flashjoin.h"), r"\"bloom_variant\"\s+- hash / bit layout of the filter, 0\.\.2 \(csrc/fj_bloom_dev\.h; default (\d+)\)",
                            "include/flashjoin.h on bloom_variant")
    c["variant_dev_h"] = _num(dev, r"//   VAR (\d+) \(default\):", "fj_bloom_dev.h on the default variant")
    return c


def test_the_constants_are_what_the_sources_say():
    c = constants()
    moved = f"a constant of the bloom precheck moved: tests/bloom_model.py, {HERE} and tests/test_bloom_exact.py are stated for these - read the new one, then update"
    assert (c["FJ_BLOOM_WORDS"], c["FJ_PREFILTER_BITS"], c["FJ_MAX_FAN_LOG"], c["FJ_BLOOM_HDR_MAGIC"]) == (BM.WORDS, BM.PREFILTER_BITS, BM.MAX_FAN_LOG, BM.HDR_MAGIC), moved
    assert (BM.WORDS, BM.PREFILTER_BITS, BM.MAX_FAN_LOG, BM.HDR_MAGIC) == (35840, 9, 9, 0xB100F000), moved
    assert (c["BF_NT"], c["BF_KPT"], c["BF_STG"], c["BF_SLAB"], c["FJ_BLOOM_SNAP16"]) == (1024, 8, 128, 128, 3), moved
    assert c["BF_NT"] * c["BF_KPT"] == STEP_KEYS == TILE_CHUNKS * CHUNK, moved
    assert c["FJ_BLOOM_GOOD_KEYS"] == 215_000, moved


def test_the_default_variant_is_stated_once():
    c = constants()
    assert c["variant_code"] == 0, "fj_host.h no longer starts bloom_variant at 0: the GPU tests restore that value"
    assert c["variant_doc"] == c["variant_code"], f"include/flashjoin.h says the default bloom_variant is {c['variant_doc']}, fj_host.h starts it at {c['variant_code']}"
    assert c["variant_dev_h"] == c["variant_code"], f"fj_bloom_dev.h calls VAR {c['variant_dev_h']} the default, fj_host.h starts it at {c['variant_code']}"


@pytest.mark.parametrize("where,name,old,new", [
    ("csrc", "fj_common.h", "#define FJ_BLOOM_WORDS 35840u", "#define FJ_BLOOM_WORDS 32768u"),
    ("csrc", "fj_common.h", "#define FJ_PREFILTER_BITS 9", "#define FJ_PREFILTER_BITS 8"),
    ("csrc", "fj_bloom.hip", "constexpr u32 BF_STG = 128;", "constexpr u32 BF_STG = 256;"),
    ("csrc", "fj_bloom.hip", "constexpr u32 BF_SLAB = 128;", "constexpr u32 BF_SLAB = 64;"),
    ("csrc", "fj_bloom.hip", "constexpr u32 BF_KPT = 8;", "constexpr u32 BF_KPT = 4;"),
    ("csrc", "fj_bloom.hip", "#define FJ_BLOOM_SNAP16 3\n", "#define FJ_BLOOM_SNAP16 2\n"),
    ("csrc", "fj_bloom_dev.h", "(1u << ((w >> 13) & 31u))", "(1u << ((w >> 14) & 31u))"),
    ("csrc", "fj_host.h", "int bloom_variant = 0,", "int bloom_variant = 2,"),
    ("include", "flashjoin.h", "csrc/fj_bloom_dev.h; default 0)", "csrc/fj_bloom_dev.h; default 2)"),
    ("csrc", "fj_plan.hip", "(extra_first ? i < rem : i >= p.npass - rem)", "(extra_first ? i >= p.npass - rem : i < rem)"),
])
def test_an_edited_constant_fails_by_name(tmp_path, where, name, old, new):
    csrc, include = str(tmp_path / "csrc"), str(tmp_path / "include")
    shutil.copytree(CSRC, csrc, ignore=shutil.ignore_patterns("*.o", "*.so", "*.a"))
    shutil.copytree(INCLUDE, include)
    path = os.path.join(csrc if where == "csrc" else include, name)
    with open(path) as f:
        text = f.read()
    assert text.count(old) == 1, (name, old)
    with open(path, "w") as f:
        f.write(text.replace(old, new))
    try:
        got = constants(csrc, include)
    except AssertionError as e:
        assert HERE in str(e), str(e)
        return
    assert got != constants(), f"{name}: `{old}` -> `{new}` went unnoticed"


def test_the_plan_split_rule():
    """extra bits go to the earlier pass: what tests/test_bloom_exact.py derives the in-join stage's level-1 bucket count from"""
    assert [BM.plan_fan_logs(b) for b in (0, 5, 9, 10, 13, 17, 18, 19, 20)] == [[], [5], [9], [5, 5], [7, 6], [9, 8], [9, 9], [7, 6, 6], [7, 7, 6]]
    assert BM.level1_bits(13) == 7
    # part C: 100 000 build rows under plan_target_keys = 16 -> 6250 parts -> 13 bits; no rebalancing: nb >> 7 is far below FJ_BLOOM_GOOD_KEYS
    nb, target, bits = join_sizes()[0], 16, 0
    while (1 << bits) < -(-nb // target):
        bits += 1
    assert bits == 13 and (nb >> BM.level1_bits(bits)) < constants()["FJ_BLOOM_GOOD_KEYS"] // 100


# ---- crafted keys ------------------------------------------------------------------------------------------------------------------------
def craft(bucket, w2, top_bits, seed, bucket_bits=BM.PREFILTER_BITS):
    """raw keys whose bucket - the bucket_bits bits of the mixed key below its 64 - top_bits owner bits - is `bucket` (a number or one
    per key) and whose low mixed word is w2[i]; the remaining bits of the high mixed word are drawn from `seed`"""
    w2 = np.asarray(w2, dtype=np.uint64)
    n, owner_bits = w2.size, 64 - top_bits
    low_bits = 32 - owner_bits - bucket_bits
    assert low_bits >= 1 and np.all(w2 < _U(0xFFFFFFFF)), "0xFFFFFFFF is the low word of the empty marker and the wide filler"
    rng = np.random.default_rng([seed, top_bits, bucket_bits])
    w1 = (np.broadcast_to(np.asarray(bucket, dtype=np.uint64), (n,)) << _U(low_bits)) | rng.integers(0, 1 << low_bits, n, dtype=np.uint64)
    if owner_bits:
        w1 = w1 | (rng.integers(0, 1 << owner_bits, n, dtype=np.uint64) << _U(32 - owner_bits))
    k = keymix.unmix((w1 << _U(32)) | w2)
    assert np.array_equal(BM.bucket_of(k, bucket_bits, top_bits), np.broadcast_to(np.asarray(bucket, dtype=np.int64), (n,)))
    return k


def in_bucket(bucket, n, top_bits, seed, bucket_bits=BM.PREFILTER_BITS):
    """n keys of a bucket with random low words"""
    w2 = np.random.default_rng([seed, 7]).integers(0, 0xFFFFFFFF, n, dtype=np.uint64)
    return craft(bucket, w2, top_bits, seed, bucket_bits)


def rebucket(keys, bucket, top_bits, bucket_bits=BM.PREFILTER_BITS):
    """the keys whose mixed form differs from that of `keys` in the bucket bits alone"""
    shift = _U(top_bits - bucket_bits)
    mask = _U(((1 << bucket_bits) - 1) << (top_bits - bucket_bits))
    return keymix.unmix((keymix.mix(keys) & ~mask) | (np.asarray(bucket, dtype=np.uint64) << shift))


def block_base(block):
    """the smallest low word w with umulhi(w, WORDS / 2) == block"""
    return -(-(block << 32) // (BM.WORDS // 2))


@functools.lru_cache(maxsize=None)
def known_lows():
    """The low 17 bits of the 64 known keys of `saturated`: bits 0-4, 5-9, 9-13 and 13-16 are the four bit positions (the last one's top
    bit is bit 17, the block's business).  Chosen so that the two positions of a half differ in more than one bit, whatever bit 17
    is: moving one position by one bit never lands it on the other, and the moved key must fail."""
    far = lambda a, b: bin(a ^ b).count("1") > 1
    out, i = [], 0
    while len(out) < 64:
        low = (i * 0x9E37 + 0x1234) & 0x1FFFF
        i += 1
        if far(low & 31, (low >> 5) & 31) and all(far((low >> 9) & 31, ((low >> 13) & 15) | top) for top in (0, 16)):
            out.append(low)
    return out


def known_words(flip=0):
    """Low words of the 64 keys of `saturated`'s bucket 201: key i alone in block 280 * i, its low 17 bits chosen - they hold the four
    bit positions but for the top bit of the last.  A block spans more than 2^17 words, so every choice of them exists in every
    block.  flip: the same words with these of the low 17 bits inverted, in the same blocks."""
    out = []
    for i, low in enumerate(known_lows()):
        base, low = block_base(KNOWN_STRIDE * i), low ^ flip
        w = base + ((low - base) % (1 << 17))
        assert (w * (BM.WORDS // 2)) >> 32 == KNOWN_STRIDE * i and w & 0x1FFFF == low
        out.append(w)
    return np.array(out, dtype=np.uint64)


def _distinct(k):
    assert np.unique(k).size == k.size, "the crafted keys collide: another seed"
    return k


@functools.lru_cache(maxsize=None)
def build_side(name, top_bits):
    rng = np.random.default_rng([20261021, top_bits])
    if name == "one":
        return craft(300, [0x12345678], top_bits, 1)
    if name == "sparse300":
        return _distinct(rng.integers(0, 2**64, 300, dtype=np.uint64))
    if name == "three":
        return _distinct(np.concatenate([in_bucket(b, n, top_bits, 10 + b) for b, n in zip(ENDS, (13_334, 13_333, 13_333))]))
    if name == "dups":
        return rng.permutation(np.tile(build_side("three", top_bits), 3))
    if name == "big":
        parts = [in_bucket(BIG_BUCKET, BIG_KEYS, top_bits, 20)] + [in_bucket(b, n, top_bits, 21 + b) for b, n in STEP_BUCKETS.items()]
        return rng.permutation(_distinct(np.concatenate(parts + [rng.integers(0, 2**64, 5000, dtype=np.uint64)])))
    if name == "saturated":
        lo, hi = block_base(SAT_BLOCK), block_base(SAT_BLOCK + 1)
        sat = craft(SAT_BUCKET, rng.integers(lo, hi, 5000, dtype=np.uint64), top_bits, 30)
        return _distinct(np.concatenate([sat, craft(KNOWN_BUCKET, known_words(), top_bits, 31)]))
    raise KeyError(name)


EXPORT_CASES = [(name, var) for name in ("one", "sparse300", "three", "big", "dups") for var in BM.VARIANTS] + [("saturated", 0)]


@functools.lru_cache(maxsize=4)
def model_filters(name, var, top_bits):
    f = BM.filters(build_side(name, top_bits), var, top_bits)
    f.setflags(write=False)
    return f


# ---- the shapes of the filter kernel's workgroup split ------------------------------------------------------------------------------------
def keys_for_tiles(tiles):
    """Keys of a bucket that the filter kernel reads as exactly `tiles` tiles: 256 * (32 * tiles - 16).  The 9-bit pass in front of it
    ends every (workgroup, bucket) pair in a partial chunk and runs at most rows / 65536 workgroups (pass_groups, pinned above), so a
    bucket of n keys arrives as ceil(n / 256) .. n / 256 + 16 chunks for every relation of up to 1M rows: 32 * tiles - 16 .. 32 * tiles
    chunks, which is `tiles` tiles all the same."""
    return CHUNK * (TILE_CHUNKS * tiles - 16)


def split_facts(tiles_per_bucket, G, extra_chunks=0):
    """What the filter kernel's workgroup split does with a probe side of these tiles per bucket ({bucket: tiles}, of 512) on G
    workgroups; extra_chunks: partial chunks added to every populated bucket (any number up to 16 leaves the facts unchanged)."""
    chunks = np.zeros(1 << BM.PREFILTER_BITS, dtype=np.int64)
    for b, t in tiles_per_bucket.items():
        chunks[b] = keys_for_tiles(t) // CHUNK + extra_chunks
    toff = BM.tile_offsets(chunks)
    assert [int(x) for x in np.diff(toff)[list(tiles_per_bucket)]] == list(tiles_per_bucket.values())
    bnd, moved = BM.boundaries(toff, G, constants()["FJ_BLOOM_SNAP16"])
    assert np.all(np.diff(bnd) >= 0) and bnd[0] == 0 and bnd[-1] == toff[-1]
    mine = np.diff(bnd)
    inner = bnd[1:G]
    t_raw = (np.arange(1, G, dtype=np.int64) * int(toff[-1])) // G
    on_bucket_edge = np.isin(inner, toff)
    sharing = {b: int(np.count_nonzero((bnd[:-1] < toff[b + 1]) & (bnd[1:] > toff[b]) & (mine > 0))) for b in tiles_per_bucket}
    # a boundary whose search sees equal consecutive entries of toff[0 .. nb) at or below t and above it
    inner_toff = toff[:-1]
    runs = inner_toff[:-1][np.diff(inner_toff) == 0]
    runs_both_sides = bool(runs.size and ((t_raw >= runs.min()) & (t_raw < runs.max())).any())
    return dict(tiles=set(int(x) for x in mine), idle=int(np.count_nonzero(mine == 0)), sharing=sharing, snaps=bool(moved.any()),
                stays=bool((~moved[1:G] & ~on_bucket_edge).any()), runs_both_sides=runs_both_sides, ntiles=int(toff[-1]))


def _wanted(one, ends):
    """the corners the two shapes must reach between them"""
    return ({1, 2, 5} <= (one["tiles"] | ends["tiles"]) and one["idle"] > 0 and max(one["sharing"].values()) >= 3
            and (one["snaps"] or ends["snaps"]) and (one["stays"] or ends["stays"]) and ends["runs_both_sides"])


@functools.lru_cache(maxsize=None)
def tiles_for(G):
    """(tiles of `one_bucket`, tiles of `ends` per bucket) for a chip of G compute units: 37 and (8, 24, 5) - about 300 000 keys each -
    where that reaches every corner (G = 256: the MI355X), else the first shape of a search that does"""
    cands = [(37, (8, 24, 5))] + [(a, (b, c, d)) for a in (3, 5, 11, 37, 2 * G + 5) for b in range(1, 27) for c in range(1, 27) for d in (1, 5, 9)]
    for one_t, ends_t in cands:
        if _wanted(split_facts({BIG_BUCKET: one_t}, G), split_facts(dict(zip(ENDS, ends_t)), G)):
            return one_t, ends_t
    raise AssertionError(f"no shape reaches every corner of the workgroup split on {G} workgroups: widen the search of tiles_for")


def prove_shapes(G):
    """Guards tests/test_bloom_exact.py test_survivors[one_bucket] and [ends] (probe sides (iii)): on G workgroups the two shapes put
    1, 2 and 5 tiles on some workgroup (the prologue clamps six descriptors when fewer than six tiles are owned), leave workgroups
    without a tile (t0 >= t1), share a bucket among at least 3 workgroups (a segment each), move one boundary onto a bucket boundary
    and leave one where it fell, and search toff with equal consecutive entries on both sides of a boundary.  Holds for any number of
    partial chunks up to 16 per bucket."""
    one_t, ends_t = tiles_for(G)
    for extra in (0, 1, 4, 16):
        one, ends = split_facts({BIG_BUCKET: one_t}, G, extra), split_facts(dict(zip(ENDS, ends_t)), G, extra)
        assert one == split_facts({BIG_BUCKET: one_t}, G) and ends == split_facts(dict(zip(ENDS, ends_t)), G), "partial chunks change the split"
        assert _wanted(one, ends), (G, one, ends)
    return one_t, ends_t


@pytest.mark.parametrize("G", [256, 8, 64, 304])
def test_the_crafted_shapes_reach_the_corners_of_the_workgroup_split(G):
    one_t, ends_t = prove_shapes(G)
    if G == 256:
        assert (one_t, ends_t) == (37, (8, 24, 5)) and keys_for_tiles(37) == 299_008 and sum(keys_for_tiles(t) for t in ends_t) == 290_816
        one, ends = split_facts({BIG_BUCKET: 37}, 256), split_facts(dict(zip(ENDS, ends_t)), 256)
        assert one["tiles"] == {0, 1, 7} and one["sharing"][BIG_BUCKET] == 25 and one["idle"] == 231, one
        assert ends["tiles"] == {0, 1, 2, 5} and ends["sharing"] == {0: 6, 255: 16, 511: 5}, ends


def test_boundaries_is_the_kernels_binary_search():
    """bloom_model.boundaries (a searchsorted) against the kernel's loop, word for word, on toff arrays with runs of equal entries"""
    def kernel_boundary(toff, nb, G, gg, snap16):
        ntiles = int(toff[nb])
        t = gg * ntiles // G
        if gg == 0 or gg >= G or ntiles == 0:
            return ntiles if gg >= G else t
        lo, hi = 0, nb
        while hi - lo > 1:
            mid = (lo + hi) >> 1
            if toff[mid] <= t:
                lo = mid
            else:
                hi = mid
        b0, b1 = int(toff[lo]), int(toff[lo + 1])
        slack = ((b1 - b0) * snap16) >> 4
        return b0 if t - b0 <= slack else (b1 if b1 - t <= slack else t)
    rng = np.random.default_rng(5)
    for trial in range(40):
        nb = int(rng.choice([32, 128, 512]))
        chunks = np.where(rng.random(nb) < 0.7, 0, rng.integers(1, 2000, nb))
        if trial == 0:
            chunks[:] = 0
        toff = BM.tile_offsets(chunks)
        for G in (8, 64, 256, 304):
            got, _ = BM.boundaries(toff, G)
            assert [int(x) for x in got] == [kernel_boundary(toff, nb, G, g, 3) for g in range(G + 1)], (trial, G)


# ---- probe sides ---------------------------------------------------------------------------------------------------------------------------
def _misses(bucket, n, top_bits, seed, build):
    m = in_bucket(bucket, n, top_bits, seed)
    assert not np.isin(m, build).any()
    return m


def _pick(pool, ok, n_pass, n_fail):
    """n_pass keys of the pool that the model lets through and n_fail that it does not, in pool order"""
    assert np.count_nonzero(ok) >= n_pass and np.count_nonzero(~ok) >= n_fail, (int(ok.sum()), n_pass)
    take = np.zeros(pool.size, dtype=bool)
    take[np.flatnonzero(ok)[:n_pass]] = True
    take[np.flatnonzero(~ok)[:n_fail]] = True
    return pool[take]


TINY = ("tiny_pass", "tiny_miss", "tiny_63", "tiny_64", "tiny_65", "tiny_255", "tiny_256", "tiny_257")
PROBE_CASES = list(TINY) + ["all_hits", "hits_1to1", "hits_1to7", "one_bucket", "ends", "partial", "stale", "empty"]


def probe_variants(name):
    return (0,) if name == "partial" else BM.VARIANTS


@functools.lru_cache(maxsize=None)
def probe_side(name, var, top_bits, G=256):
    """-> (the build side's name, the probe keys)"""
    rng = np.random.default_rng([20261022, top_bits, PROBE_CASES.index(name)])
    if name in TINY:
        build = build_side("three", top_bits)
        mine = build[BM.bucket_of(build, 9, top_bits) == 0]
        if name == "tiny_pass":
            return "three", mine[5:6]
        if name == "tiny_miss":
            pool = _misses(0, 16, top_bits, 40, build)
            return "three", _pick(pool, BM.passes(model_filters("three", var, top_bits), pool, var, top_bits), 0, 1)
        return "three", mine[:int(name[5:])]
    if name in ("all_hits", "hits_1to1", "hits_1to7"):
        build = build_side("big", top_bits)
        if name == "all_hits":
            return "big", build
        k = {"hits_1to1": 1, "hits_1to7": 7}[name]
        m = _misses(np.repeat(BM.bucket_of(build, 9, top_bits), k), build.size * k, top_bits, 41, build)
        return "big", np.concatenate([build[:, None], m.reshape(build.size, k)], axis=1).reshape(-1)
    if name == "one_bucket":
        build = build_side("big", top_bits)
        mine = build[BM.bucket_of(build, 9, top_bits) == BIG_BUCKET]
        n = keys_for_tiles(tiles_for(G)[0])
        hits = rng.choice(mine, n // 3)
        return "big", rng.permutation(np.concatenate([hits, _misses(BIG_BUCKET, n - hits.size, top_bits, 42, build)]))
    if name == "ends":
        build = build_side("three", top_bits)
        parts = []
        for b, t in zip(ENDS, tiles_for(G)[1]):
            n, mine = keys_for_tiles(t), build[BM.bucket_of(build, 9, top_bits) == b]
            hits = rng.choice(mine, n // 4)
            parts += [hits, _misses(b, n - hits.size, top_bits, 43 + b, build)]
        return "three", rng.permutation(np.concatenate(parts))
    if name == "partial":
        build = build_side("saturated", top_bits)
        w = known_words()
        same = craft(KNOWN_BUCKET, w, top_bits, 50)                                        # another high word, the same four bits: passes
        mlo_moved = [craft(KNOWN_BUCKET, known_words(1 << s), top_bits, 51 + s) for s in (0, 2, 4, 6, 8)]   # a position of mlo moved
        mhi_moved = [craft(KNOWN_BUCKET, known_words(1 << s), top_bits, 60 + s) for s in (14, 15, 16)]      # the last of mhi moved alone
        lo, hi = block_base(SAT_BLOCK), block_base(SAT_BLOCK + 1)
        on_block = craft(SAT_BUCKET, rng.integers(lo, hi, 2000, dtype=np.uint64), top_bits, 70)
        off_block = craft(SAT_BUCKET, rng.integers(0, lo, 500, dtype=np.uint64), top_bits, 71)
        p = np.concatenate([same] + mlo_moved + mhi_moved + [on_block, off_block])
        assert not np.isin(p, build).any()
        return "saturated", rng.permutation(p)
    if name == "stale":
        build = build_side("big", top_bits)
        f = model_filters("big", var, top_bits)
        pool = _misses(BIG_BUCKET, 60_000, top_bits, 80, build)
        a = _pick(pool, BM.passes(f, pool, var, top_bits), 40, 293)                        # 333 keys: one full chunk and one of 77
        pool = _misses(10, 2000, top_bits, 81, build)
        b = _pick(pool, BM.passes(f, pool, var, top_bits), 0, 1)                           # a chunk of one key
        c = rng.integers(0, 2**64, 1000 - a.size - b.size, dtype=np.uint64)                # 666 keys over 512 buckets: chunks of 1 - 5
        return "big", rng.permutation(np.concatenate([a, b, c]))
    if name == "empty":
        build = build_side("three", top_bits)
        buckets = BM.bucket_of(build, 9, top_bits)
        twins = [rebucket(build[buckets == b], nb_, top_bits) for b, nb_ in ((0, 1), (255, 254), (255, 256), (511, 510))]
        return "three", rng.permutation(np.concatenate([build] + twins))
    raise KeyError(name)


def stale_first_call(top_bits):
    """what runs in front of `stale` on the same engine: 2M keys, all of them build keys of `big`"""
    build = build_side("big", top_bits)
    return np.random.default_rng(9).choice(build, 2_000_000)


def expected_survivors(name, var, top_bits, G=256, **defect):
    bname, probe = probe_side(name, var, top_bits, G)
    if "shifts" in defect:                                        # a moved bit position moves it for insert and test alike
        f = BM.filters(build_side(bname, top_bits), var, top_bits, shifts=defect["shifts"])
    else:
        f = model_filters(bname, var, top_bits)
    return np.sort(probe[BM.passes(f, probe, var, top_bits, **defect)])


# ---- part C: the in-join stage -------------------------------------------------------------------------------------------------------------
def join_sizes():
    return 100_000, 400_000


JOIN_BUILDS = ("skewed", "holes")
JOIN_HITS = (0, 500, 10000)
L1_BITS = 7                                                     # level1_bits(13): test_the_plan_split_rule
SKEW_BUCKET, SKEW_KEYS = 5, 20_000


@functools.lru_cache(maxsize=None)
def join_case(build_name, hit_bp):
    """(bk, bv, pk): `skewed` - level-1 bucket 5 of 128 holds 20 000 of the 100 000 build keys (> 16 384: three steps of the in-kernel
    bf_build_filter); `holes` - no build key in level-1 buckets 64 .. 127, which the probe side does populate (nbc == 0).  Distinct build
    keys; the probe side repeats keys, hit_bp / 10000 of its rows hit."""
    nb, npk = join_sizes()
    rng = np.random.default_rng([20261023, JOIN_BUILDS.index(build_name)])
    if build_name == "skewed":
        bk = np.concatenate([in_bucket(SKEW_BUCKET, SKEW_KEYS, 64, 90, L1_BITS), rng.integers(0, 2**64, nb - SKEW_KEYS, dtype=np.uint64)])
    else:
        bk = in_bucket(rng.integers(0, 64, nb), nb, 64, 91, L1_BITS)
    bk = rng.permutation(_distinct(bk))
    bv = rng.integers(0, 2**64, nb, dtype=np.uint64)
    nhit = npk * hit_bp // 10000
    miss = np.concatenate([rng.integers(0, 2**64, (npk - nhit) // 2, dtype=np.uint64), in_bucket(SKEW_BUCKET, npk - nhit - (npk - nhit) // 2, 64, 92, L1_BITS)])
    pk = rng.permutation(np.concatenate([rng.choice(bk, nhit), miss]))
    assert not np.isin(miss, bk).any() and pk.size == npk
    return bk, bv, pk


def join_reference(build_name, hit_bp):
    """count and the (key, value) pairs in key order, by a sort and a searchsorted on raw keys"""
    bk, bv, pk = join_case(build_name, hit_bp)
    order = np.argsort(bk)
    sk = bk[order]
    at = np.minimum(np.searchsorted(sk, pk), sk.size - 1)
    hit = sk[at] == pk
    k, v = pk[hit], bv[order][at[hit]]
    o = np.lexsort((v, k))
    return int(hit.sum()), k[o], v[o]


# ---- 1. the model's self-checks ----------------------------------------------------------------------------------------------------------
def test_known_answers_worked_by_hand():
    """bf_bits<0> on mixed words whose fields can be read off the hex: 0x00012345 = 0b1_0010_0011_0100_0101 -> bits 0-4: 5, bits 5-9: 26,
    bits 9-13: 17, bits 13-17: 9; block 0.  0xFFFFFFFF: the last block, bit 31 four times."""
    word, mlo, mhi = BM.bits_of_mixed(np.array([0, 0x00012345, 0xFFFFFFFF, 0xABCDEF0000000000 | 0x00012345], dtype=np.uint64), 0)
    assert word.tolist() == [0, 0, BM.WORDS - 2, 0]
    assert mlo.tolist() == [1, (1 << 5) | (1 << 26), 1 << 31, (1 << 5) | (1 << 26)]
    assert mhi.tolist() == [1, (1 << 17) | (1 << 9), 1 << 31, (1 << 17) | (1 << 9)]
    # VAR 1 / 2 hash both words: x of mixed 0 is 0 -> word 0, bit 0
    for var in (1, 2):
        word, mlo, mhi = BM.bits_of_mixed(np.array([0], dtype=np.uint64), var)
        assert (int(word[0]), int(mlo[0]), int(mhi[0])) == (0, 1, 0 if var == 1 else 1)
    # x of mixed 1: 0x9E3779B1 ^ (0x9E3779B1 >> 15) = 0x9E3645DF; * 0x85EBCA77 mod 2^32, ^ >> 13
    x = 0x9E3779B1 ^ (0x9E3779B1 >> 15)
    x = (x * 0x85EBCA77) & 0xFFFFFFFF
    x ^= x >> 13
    word, mlo, mhi = BM.bits_of_mixed(np.array([1], dtype=np.uint64), 1)
    assert int(word[0]) == (x * BM.WORDS) >> 32 and int(mlo[0]) == (1 << (x & 31)) | (1 << ((x >> 5) & 31))
    # the high word enters rotated by 15
    a = BM.bits_of_mixed(np.array([1 << 32], dtype=np.uint64), 2)
    b = BM.bits_of_mixed(np.array([1 << 15], dtype=np.uint64), 2)
    assert [int(v[0]) for v in a] == [int(v[0]) for v in b]


@pytest.mark.parametrize("top_bits", TOPS)
@pytest.mark.parametrize("var", BM.VARIANTS)
def test_the_model_has_no_false_negatives_and_an_empty_filter_is_zero(var, top_bits):
    for name in ("sparse300", "three", "big") + (("saturated",) if var == 0 else ()):
        build = build_side(name, top_bits)
        f = model_filters(name, var, top_bits)
        assert BM.passes(f, build, var, top_bits).all(), name
        populated = np.unique(BM.bucket_of(build, 9, top_bits))
        assert not f[np.setdiff1d(np.arange(512), populated)].any() and f[populated].any(axis=1).all(), name
    assert not BM.filters(np.zeros(0, dtype=np.uint64), var, top_bits).any()
    assert np.array_equal(BM.exported(np.zeros(0, dtype=np.uint64), var, top_bits)[-4:].view(np.uint32), [BM.HDR_MAGIC | var, 0, 0, 0])


def test_var_1_sets_one_word_per_key_and_the_variants_differ():
    build = build_side("one", 64)
    f = [BM.filters(build, var) for var in BM.VARIANTS]
    assert [int(np.count_nonzero(x)) for x in f] == [2, 1, 2]
    for var in (0, 2):
        w = np.flatnonzero(f[var].reshape(-1))
        assert w[0] % 2 == 0 and w[1] == w[0] + 1, "a 64-bit block is two little-endian words, mlo the lower"
    big = [model_filters("big", var, 64) for var in BM.VARIANTS]
    assert not np.array_equal(big[0], big[1]) and not np.array_equal(big[0], big[2]) and not np.array_equal(big[1], big[2])
    # VAR 1 on many keys: a word holds the masks of its own keys and nothing of a neighbour's
    keys = build_side("three", 64)
    word, mlo, _ = BM.bits(keys, 1)
    g = BM.filters(keys, 1)
    at = BM.bucket_of(keys, 9) * BM.WORDS + word
    want = np.zeros(g.size, dtype=np.uint32)
    for a, m in zip(at.tolist(), mlo.tolist()):
        want[a] |= m
    assert np.array_equal(g.reshape(-1), want)


def test_the_crafted_blocks_of_saturated():
    for top_bits in TOPS:
        f = model_filters("saturated", 0, top_bits)
        assert f[SAT_BUCKET, 2 * SAT_BLOCK] == f[SAT_BUCKET, 2 * SAT_BLOCK + 1] == 0xFFFFFFFF and np.count_nonzero(f[SAT_BUCKET]) == 2
        w = known_words()
        for i in range(64):
            low = int(w[i])
            blk = f[KNOWN_BUCKET, 2 * KNOWN_STRIDE * i: 2 * KNOWN_STRIDE * i + 2]
            assert int(blk[0]) == (1 << (low & 31)) | (1 << ((low >> 5) & 31)) and int(blk[1]) == (1 << ((low >> 9) & 31)) | (1 << ((low >> 13) & 31))
        assert np.count_nonzero(f[KNOWN_BUCKET]) == 128 and np.count_nonzero(f) == 130


# ---- 2. what every input of the GPU file can tell apart --------------------------------------------------------------------------------------
def _own_bit_lacking(keys, var, top_bits):
    """per bucket: how many of its distinct keys set no filter bit that no other key of the bucket sets"""
    keys = np.unique(keys)
    word, mlo, mhi = BM.bits(keys, var)
    base = (BM.bucket_of(keys, 9, top_bits) * BM.WORDS + word) * 32
    ids = []
    for b in range(32):
        ids.append(np.where((mlo >> np.uint32(b)) & np.uint32(1), base + b, -1))
        ids.append(np.where((mhi >> np.uint32(b)) & np.uint32(1), base + 32 + b, -1))
    ids = np.stack(ids, axis=1)
    u, cnt = np.unique(ids[ids >= 0], return_counts=True)
    alone = np.zeros(ids.shape, dtype=bool)
    alone[ids >= 0] = cnt[np.searchsorted(u, ids[ids >= 0])] == 1
    lacking = ~alone.any(axis=1)
    return np.bincount(BM.bucket_of(keys, 9, top_bits)[lacking], minlength=512), np.bincount(BM.bucket_of(keys, 9, top_bits), minlength=512)


# which seeded defects each export case is a test of (guards tests/test_bloom_exact.py test_exported_filters[<name>-...])
EXPORT_DETECTS = {"one": "b", "sparse300": "b", "three": "bc", "big": "bc", "dups": "b", "saturated": "b"}


@pytest.mark.parametrize("top_bits", TOPS)
@pytest.mark.parametrize("name,var", EXPORT_CASES)
def test_every_export_case_tells_its_defects_from_the_model(name, var, top_bits):
    build, f = build_side(name, top_bits), model_filters(name, var, top_bits)
    # (b): the compared words differ when any one bit position is read one bit higher
    for shifts in SHIFT_DEFECTS[:2] if var == 1 else SHIFT_DEFECTS:
        assert not np.array_equal(BM.filters(build, var, top_bits, shifts=shifts), f), f"test_exported_filters[{name}]: defect (b) {shifts} goes unnoticed"
    if "c" not in EXPORT_DETECTS[name]:
        return
    # (c): a bucket of n keys has at least ceil(ceil(n / 256) / 32) steps; whichever keys a step held, leaving it out shows
    lacking, size = _own_bit_lacking(build, var, top_bits)
    steps = -(-(-(-size // CHUNK)) // TILE_CHUNKS)
    want = {"three": {b: 2 for b in ENDS}, "big": {BIG_BUCKET: 9, 10: 1, 11: 1, 12: 2, 13: 3}}[name]
    for b, s in want.items():
        assert steps[b] >= s, f"test_exported_filters[{name}]: bucket {b} has {steps[b]} steps, not {s}"
        # a full step holds 8192 keys, fewer than that lack a bit of their own: a left-out first, second or third step changes a word
        assert lacking[b] < STEP_KEYS, (name, b, int(lacking[b]))
        if b != BIG_BUCKET:
            # The sizes around one and two steps, where the last step may hold few keys.  A key lacks a bit of its own when each of its
            # bits is also set by another of the bucket's n keys.  With p = k * n / 1 146 880 the share of the filter's bits that are set,
            # that is n * p^4 keys on average for VAR 0 and 2 (0.2 at n = 16 385) and n * (p^2 + p / 32) for VAR 1, whose two positions
            # fall together for every 32nd key (28 at n = 16 385).  Four times that and no less than 8: a last step of 128 keys shows
            k = 2 if var == 1 else 4
            share = k * int(size[b]) / (BM.WORDS * 32)
            mean = size[b] * (share ** 2 + share / 32 if var == 1 else share ** 4)
            assert lacking[b] < max(8, 4 * mean) <= 128, f"test_exported_filters[{name}]: {lacking[b]} keys of bucket {b} could be left out unnoticed"
    if name == "big":
        # the last step of the 70 000-key bucket holds at least 70 000 - 8 * 8192 = 4464 keys when its chunks are full; partial chunks only
        # move keys towards later steps
        assert size[BIG_BUCKET] - 8 * STEP_KEYS > lacking[BIG_BUCKET], (int(lacking[BIG_BUCKET]), "keys of the big bucket lack a bit of their own")
        assert -(-size[BIG_BUCKET] // CHUNK) >= 273


# which seeded defects each probe case is a test of (guards tests/test_bloom_exact.py test_survivors[<name>-...] / test_tiny_probe_sides)
PROBE_DETECTS = {"tiny_pass": "d", "tiny_miss": "", "tiny_63": "d", "tiny_64": "d", "tiny_65": "d", "tiny_255": "d", "tiny_256": "d", "tiny_257": "d",
                 "all_hits": "d", "hits_1to1": "ad", "hits_1to7": "ad", "one_bucket": "ad", "ends": "d", "partial": "abd", "stale": "d", "empty": "d"}


@pytest.mark.parametrize("top_bits", TOPS)
@pytest.mark.parametrize("name", PROBE_CASES)
def test_every_probe_case_tells_its_defects_from_the_model(name, top_bits):
    for var in probe_variants(name):
        bname, probe = probe_side(name, var, top_bits)
        build = build_side(bname, top_bits)
        want = expected_survivors(name, var, top_bits)
        hits = np.sort(probe[np.isin(probe, build)])
        assert np.array_equal(want[np.isin(want, build)], hits), "no false negatives"
        tag = f"test_survivors[{name}] var {var} top_bits {top_bits}"
        detects = PROBE_DETECTS[name]
        if "a" in detects and var != 1:                          # misses that pass the mlo test and fail the mhi test
            loose = expected_survivors(name, var, top_bits, use_mhi=False)
            assert loose.size > want.size, f"{tag}: defect (a) goes unnoticed"
        if "b" in detects:                                       # a moved position, in insert and test alike, changes who passes
            for shifts in SHIFT_DEFECTS:
                assert not np.array_equal(expected_survivors(name, var, top_bits, shifts=shifts), want), f"{tag}: defect (b) {shifts} goes unnoticed"
        if "d" in detects:                                       # a survivor dropped per flush: any survivor at all means a flush
            assert want.size > 0, f"{tag}: defect (d) goes unnoticed"
        else:
            assert want.size == 0
        if name == "tiny_pass":
            assert want.size == 1
        if name.startswith("tiny_") and name[5:].isdigit():
            assert want.size == probe.size == int(name[5:]) and np.unique(BM.bucket_of(probe, 9, top_bits)).tolist() == [0]
        if name == "all_hits":
            assert want.size == probe.size
        if name in ("hits_1to1", "hits_1to7"):
            k = 1 if name == "hits_1to1" else 7
            assert probe.size == build.size * (k + 1) and hits.size == build.size and np.array_equal(probe[::k + 1], build)
            assert np.array_equal(BM.bucket_of(probe, 9, top_bits).reshape(-1, k + 1)[:, 1:], np.repeat(BM.bucket_of(build, 9, top_bits)[:, None], k, axis=1))
            assert want.size > hits.size, "some misses pass: the model decides which"
        if name == "one_bucket":
            assert probe.size == 299_008 and np.unique(BM.bucket_of(probe, 9, top_bits)).tolist() == [BIG_BUCKET] and want.size > hits.size > 90_000
        if name == "ends":
            assert probe.size == 290_816 and np.unique(BM.bucket_of(probe, 9, top_bits)).tolist() == list(ENDS)
        if name == "partial":
            assert want.size == 64 + 2000, "the 64 twins with the same low word and everything on the saturated block pass, nothing else"
            loose = expected_survivors(name, var, top_bits, use_mhi=False)
            assert loose.size == want.size + 3 * 64, "the keys whose last mhi position moved pass mlo and fail mhi"
        if name == "stale":
            sizes = np.bincount(BM.bucket_of(probe, 9, top_bits), minlength=512)
            assert probe.size == 1000 and not np.isin(probe, build).any() and want.size >= 40
            assert sizes[BIG_BUCKET] in (333, 334, 335, 336) and (sizes % 2 == 1).sum() > 100 and sizes.max() < 2 * CHUNK
            first = stale_first_call(top_bits)
            assert first.size == 2_000_000 and np.isin(first, build).all()
        if name == "empty":
            sizes = np.bincount(BM.bucket_of(probe, 9, top_bits), minlength=512)
            assert all(sizes[b] > 13_000 for b in EMPTY_NEIGHBOURS + ENDS) and want.size == build.size and np.array_equal(want, np.sort(build))
            if var == 0:                                         # under VAR 0 a twin would pass its neighbour's filter: same low word
                twins = probe[~np.isin(probe, build)]
                for b, home in ((1, 0), (254, 255), (256, 255), (510, 511)):
                    t = twins[BM.bucket_of(twins, 9, top_bits) == b]
                    assert BM.passes(model_filters("three", 0, top_bits), rebucket(t, home, top_bits), 0, top_bits).all()


@pytest.mark.parametrize("var", BM.VARIANTS)
def test_every_defect_has_a_case_for_every_variant_it_applies_to(var):
    exports = {n for n, v in EXPORT_CASES if v == var}
    probes = {n for n in PROBE_CASES if var in probe_variants(n)}
    assert any("b" in EXPORT_DETECTS[n] for n in exports) and any("c" in EXPORT_DETECTS[n] for n in exports)
    assert any("d" in PROBE_DETECTS[n] for n in probes)
    if var != 1:
        assert any("a" in PROBE_DETECTS[n] for n in probes)


@pytest.mark.parametrize("build_name", JOIN_BUILDS)
def test_the_join_cases_are_what_part_c_asks_for(build_name):
    """guards tests/test_bloom_exact.py test_in_join_stage[<build>-...]"""
    nb, npk = join_sizes()
    for hit_bp in JOIN_HITS:
        bk, bv, pk = join_case(build_name, hit_bp)
        n, k, v = join_reference(build_name, hit_bp)
        assert bk.size == bv.size == nb and pk.size == npk and np.unique(bk).size == nb and n == npk * hit_bp // 10000 == k.size
        sizes = np.bincount(BM.bucket_of(bk, L1_BITS), minlength=128)
        psizes = np.bincount(BM.bucket_of(pk, L1_BITS), minlength=128)
        if build_name == "skewed":
            assert sizes[SKEW_BUCKET] > 16_384 + 3000 and psizes[SKEW_BUCKET] > 80_000
        else:
            assert not sizes[64:].any() and sizes[:64].all() and (psizes[64:].all() if hit_bp < 10000 else True)
        for var in BM.VARIANTS:
            f = BM.filters(bk, var, 64, L1_BITS)
            ok = BM.passes(f, pk, var, 64)
            assert ok[np.isin(pk, bk)].all() and n <= int(ok.sum()) <= npk
            if hit_bp < 10000:
                assert not ok[BM.bucket_of(pk, L1_BITS) >= 64].any() if build_name == "holes" else int(ok.sum()) > n, "false positives for the model to name"
                if var != 1 and build_name == "skewed":
                    assert int(BM.passes(f, pk, var, 64, use_mhi=False).sum()) > int(ok.sum()), "defect (a) goes unnoticed"
