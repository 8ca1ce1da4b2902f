"""NumPy model of the bloom precheck (csrc/fj_bloom_dev.h read as a specification: bf_bits<VAR>, bf_insert, bf_fetch, bf_pass) - test
infrastructure: what tests/test_bloom_exact_cpu.py and tests/test_bloom_exact.py compare the filter kernels with, bit for bit.
Whole-array uint64 / uint32 arithmetic; imports nothing from the library.

A filter belongs to one radix bucket and is WORDS 32-bit words.  A key is hashed in its MIXED form (keymix.mix: chunk pools hold mixed
keys) to one place and one mask:
  VAR 0  w = the low mixed word; 64-bit block umulhi(w, WORDS / 2); mlo = bits (w & 31), (w >> 5 & 31) of the block's lower word,
         mhi = bits (w >> 9 & 31), (w >> 13 & 31) of its upper word
  VAR 1  x = the two-multiply mixer over lo ^ rotl(hi, 15); 32-bit word umulhi(x, WORDS); mlo = bits (x & 31), (x >> 5 & 31); mhi = 0
  VAR 2  the same x; 64-bit block umulhi(x, WORDS / 2); mlo and mhi as in VAR 0, from x
A 64-bit block is two little-endian words, mlo the lower.  A key passes when the filter holds all of its bits."""
import numpy as np

import keymix

WORDS = 35840                       # csrc/fj_common.h FJ_BLOOM_WORDS (pinned by tests/test_bloom_exact_cpu.py)
PREFILTER_BITS = 9                  # FJ_PREFILTER_BITS: the sender-side precheck keeps 512 filters per owner
HDR_MAGIC = 0xB100F000              # FJ_BLOOM_HDR_MAGIC: an exported set ends with 4 header words, [0] = magic | variant
MAX_FAN_LOG = 9                     # FJ_MAX_FAN_LOG
VARIANTS = (0, 1, 2)

_M32 = np.uint64(0xFFFFFFFF)
_U = np.uint64


def _two_bits(v, s0, s1):
    one = _U(1)
    return ((one << ((v >> _U(s0)) & _U(31))) | (one << ((v >> _U(s1)) & _U(31)))).astype(np.uint32)


def bits_of_mixed(h, var, shifts=(0, 5, 9, 13)):
    """bf_bits<var> of MIXED keys: (index of the key's first 32-bit word in the filter, mlo, mhi).  `shifts`: where the four bit
    positions are read from (the tests seed a defect by moving one)."""
    h = np.asarray(h, dtype=np.uint64)
    lo, hi = h & _M32, h >> _U(32)
    if var == 0:
        v = lo
    else:
        x = lo ^ (((hi << _U(15)) | (hi >> _U(17))) & _M32)
        x = (x * _U(0x9E3779B1)) & _M32; x ^= x >> _U(15)
        x = (x * _U(0x85EBCA77)) & _M32; x ^= x >> _U(13)
        v = x
    if var == 1:
        word = (v * _U(WORDS)) >> _U(32)
        return word.astype(np.int64), _two_bits(v, shifts[0], shifts[1]), np.zeros(h.shape, dtype=np.uint32)
    word = ((v * _U(WORDS // 2)) >> _U(32)) * _U(2)
    return word.astype(np.int64), _two_bits(v, shifts[0], shifts[1]), _two_bits(v, shifts[2], shifts[3])


def bits(keys, var, shifts=(0, 5, 9, 13)):
    """bf_bits<var> of RAW keys"""
    return bits_of_mixed(keymix.mix(keys), var, shifts)


def bucket_of(keys, bucket_bits, top_bits=64):
    return keymix.partition_of(keys, bucket_bits, top_bits)


def filters(build, var, top_bits=64, bucket_bits=PREFILTER_BITS, shifts=(0, 5, 9, 13)):
    """uint32[2^bucket_bits][WORDS]: per bucket the OR of the masks of its build keys (no keys: all zero)"""
    build = np.asarray(build, dtype=np.uint64)
    f = np.zeros((1 << bucket_bits, WORDS), dtype=np.uint32)
    if build.size == 0:
        return f
    word, mlo, mhi = bits(build, var, shifts)
    at = bucket_of(build, bucket_bits, top_bits) * WORDS + word
    flat = f.reshape(-1)
    np.bitwise_or.at(flat, at, mlo)
    if var != 1:
        np.bitwise_or.at(flat, at + 1, mhi)
    return f


def exported(build, var, top_bits=64):
    """what LabEngine.bloom_export returns: the 512 filters and the 4 header words, as int32"""
    out = np.zeros((1 << PREFILTER_BITS) * WORDS + 4, dtype=np.uint32)
    out[:-4] = filters(build, var, top_bits).reshape(-1)
    out[-4] = HDR_MAGIC | var
    return out.view(np.int32)


def passes(f, probe, var, top_bits=64, use_mhi=True, shifts=(0, 5, 9, 13)):
    """bf_pass of every probe key against the filter of its bucket (f: what filters() gave); use_mhi=False seeds the defect of a test
    that looks at mlo alone"""
    probe = np.asarray(probe, dtype=np.uint64)
    bucket_bits = int(f.shape[0]).bit_length() - 1
    word, mlo, mhi = bits(probe, var, shifts)
    at = bucket_of(probe, bucket_bits, top_bits) * WORDS + word
    flat = f.reshape(-1)
    ok = (flat[at] & mlo) == mlo
    if var != 1 and use_mhi:
        ok &= (flat[at + 1] & mhi) == mhi
    return ok


def survivors(build, probe, var, top_bits=64, bucket_bits=PREFILTER_BITS):
    """the sorted multiset of probe keys that pass"""
    probe = np.asarray(probe, dtype=np.uint64)
    return np.sort(probe[passes(filters(build, var, top_bits, bucket_bits), probe, var, top_bits)])


def survivor_count(build, probe, var, top_bits=64, bucket_bits=PREFILTER_BITS):
    return int(np.count_nonzero(passes(filters(build, var, top_bits, bucket_bits), probe, var, top_bits)))


# ---- the plan's split of its radix bits (csrc/fj_plan.hip plan_npass / plan_passes, extra bits to the EARLIER passes) -----------------
def plan_fan_logs(radix_bits):
    """fan_log[] of a plan of radix_bits bits: one pass up to 9 bits, two up to 18, ceil(bits / 9) beyond; bits / npass each and one
    more for the first bits % npass passes"""
    if radix_bits <= 0:
        return []
    npass = 1 if radix_bits <= MAX_FAN_LOG else (2 if radix_bits <= 2 * MAX_FAN_LOG else -(-radix_bits // MAX_FAN_LOG))
    rem = radix_bits % npass
    return [radix_bits // npass + (1 if i < rem else 0) for i in range(npass)]


def level1_bits(radix_bits):
    """bits of the level the in-join filter stage of a two-pass plan works on: the first pass's"""
    return plan_fan_logs(radix_bits)[0]


# ---- the filter kernel's split of its tiles among workgroups (csrc/fj_bloom.hip boundary()) -------------------------------------------
def tile_offsets(chunks_per_bucket, tile_chunks=32):
    """toff[0 .. nb]: ceil(chunks / 32) tiles per bucket, scanned"""
    c = np.asarray(chunks_per_bucket, dtype=np.int64)
    return np.concatenate(([0], np.cumsum(-(-c // tile_chunks))))


def boundaries(toff, G, snap16=3):
    """boundary(0 .. G) and, per inner boundary, whether it moved onto a bucket boundary: t = g * ntiles / G; lo = the last bucket with
    toff[lo] <= t; within (tiles of lo * snap16) >> 4 of toff[lo] (tested first) or of toff[lo + 1] the boundary moves there"""
    toff = np.asarray(toff, dtype=np.int64)
    nb, ntiles = toff.size - 1, int(toff[-1])
    g = np.arange(G + 1, dtype=np.int64)
    t = g * ntiles // G
    if ntiles == 0:
        return t, np.zeros(G + 1, dtype=bool)
    lo = np.searchsorted(toff[:nb], t, side="right") - 1
    b0, b1 = toff[lo], toff[lo + 1]
    slack = ((b1 - b0) * snap16) >> 4
    out = np.where(t - b0 <= slack, b0, np.where(b1 - t <= slack, b1, t))
    out[0], out[G] = 0, ntiles
    moved = out != t
    moved[0] = moved[G] = False
    return out, moved
