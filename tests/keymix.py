"""NumPy restatement of the device's key mixer (csrc/fj_common.h fj_key_mix / fj_key_unmix; C ABI fj_key_mix64 / fj_key_unmix64)
and of the owner shuffle's 7-byte wire format (csrc/fj_pack.hip) - test infrastructure: what the tests check placements and
packed chunks against.  tests/test_abi.py pins these functions to the library's own."""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


def _fmix32(x):
    x = x.astype(np.uint64)
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x85EBCA6B)) & _M32
    x ^= x >> np.uint64(13); x = (x * np.uint64(0xC2B2AE35)) & _M32
    x ^= x >> np.uint64(16)
    return x


def _fmix32_inv(x):
    x = x.astype(np.uint64)
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x7ED1B41D)) & _M32
    x ^= (x >> np.uint64(13)) ^ (x >> np.uint64(26)); x = (x * np.uint64(0xA5CB9243)) & _M32
    x ^= x >> np.uint64(16)
    return x


def mix(k):
    """fj_key_mix64 of a uint64 array: high word = radix digits / owner (hash word 1), low word = table slots (hash word 2)."""
    k = np.asarray(k).astype(np.uint64)
    a = ((k & _M32) * np.uint64(0x9E3779B1)) & _M32
    b = ((k >> np.uint64(32)) * np.uint64(0x85EBCA77)) & _M32
    w1 = _fmix32(a ^ b)
    w2 = _fmix32((a + w1) & _M32)
    return (w1 << np.uint64(32)) | w2


def unmix(h):
    h = np.asarray(h).astype(np.uint64)
    w1, w2 = h >> np.uint64(32), h & _M32
    a = (_fmix32_inv(w2) - w1) & _M32
    b = _fmix32_inv(w1) ^ a
    lo = (a * np.uint64(0x0E8B2F51)) & _M32
    hi = (b * np.uint64(0xB6C92F47)) & _M32
    return (hi << np.uint64(32)) | lo


# ---- the keys the kernels treat out of band -----------------------------------------------------------------------------------
# Chunk pools and LDS tables hold MIXED keys, so the partitioned kernels' empty marker (FJ_EMPTY_KEY, csrc/fj_common.h) and the
# wide kernel's filler (W_POISON2, csrc/fj_join_wide.hip) are the raw keys whose mixed forms are these words; the HBM table
# stores raw keys, so there the marker is raw 2^64 - 1.  tests/test_special_keys.py pins the two constants to the sources.
EMPTY_MIXED = 0xFFFFFFFFFFFFFFFF
FILLER_MIXED = 0x00000000FFFFFFFF
EMPTY_RAW = int(unmix(np.array([EMPTY_MIXED], dtype=np.uint64))[0])
FILLER_RAW = int(unmix(np.array([FILLER_MIXED], dtype=np.uint64))[0])


def special_mixed_words(radix_bits):
    """[(name, mixed word)] of the keys special_raw_keys(radix_bits) plants in the hash domain.  The two partition keys share
    the low word (home slot) of the marker and the filler and differ from them in the first bit below the plan's radix_bits
    partition bits (the top bits of the high word): the last / first partition of every plan of at most radix_bits bits."""
    if not 0 <= radix_bits <= 31:
        raise ValueError("radix_bits must be 0..31")
    below = 1 << (31 - radix_bits)
    return [("marker", EMPTY_MIXED), ("marker_minus_1", EMPTY_MIXED - 1), ("mixed_zero", 0), ("mixed_one", 1),
            ("wide_filler", FILLER_MIXED), ("high_word_ones", 0xFFFFFFFF00000000),
            (f"last_partition_low_ones_{radix_bits}", ((0xFFFFFFFF ^ below) << 32) | 0xFFFFFFFF),
            (f"first_partition_low_ones_{radix_bits}", (below << 32) | 0xFFFFFFFF)]


def special_raw_keys(radix_bits):
    """(names, raw keys as a uint64 array): the raw keys whose mixed forms are special_mixed_words(radix_bits), then raw 2^64 - 1
    and raw 0 - the marker and the zero of the HBM-table path, ordinary keys everywhere else.  The names serve as test ids."""
    words = special_mixed_words(radix_bits)
    names = [n for n, _ in words] + ["raw_all_ones", "raw_zero"]
    raw = np.concatenate([unmix(np.array([w for _, w in words], dtype=np.uint64)), np.array([2**64 - 1, 0], dtype=np.uint64)])
    return names, raw


# ---- keys crafted to collide in a partition's table -----------------------------------------------------------------------------
# The mixer is a bijection, so any (hash word 1, hash word 2) pair names exactly one raw key.  A partition of a plan of radix_bits
# bits is the top radix_bits bits of hash word 1; every table takes its slots, groups, buckets and tags from hash word 2 alone
# (csrc/fj_common.h FJ_HW2).  craft() fixes both and lets the keys differ in the rest of hash word 1 only - bits no table looks at.
def _w2_array(w2, n):
    w = np.asarray(w2, dtype=np.uint64)
    if w.ndim == 0:
        w = np.full(n, w, dtype=np.uint64)
    if w.shape != (n,) or np.any(w > _M32):
        raise ValueError("w2: a 32-bit scalar or an array of n of them")
    return w


def craft_mixed(radix_bits, partition, w2, n, seed=0, low_bits=None, allow_special=False, skip=0):
    """The mixed words of craft(): n distinct words (partition << (32 - radix_bits) | low) << 32 | w2.  low runs through
    (start + i * odd) mod 2^low_bits for i = skip .. (start and odd drawn from seed): distinct as long as skip + n <= 2^low_bits, and
    for one seed the ranges [0, n) and [n, ...) never meet - which is how ghosts() stays clear of craft().  low_bits defaults to all
    32 - radix_bits remaining bits; a smaller value keeps the bits right below the partition bits at zero (keys that further radix
    bits cannot tell apart).  The empty marker and the wide filler are left out unless allow_special (the sequence's next word stands in)."""
    if not 0 <= radix_bits <= 31 or not 0 <= partition < (1 << radix_bits):
        raise ValueError("partition must be one of the plan's 2^radix_bits")
    rest = 32 - radix_bits
    low_bits = rest if low_bits is None else low_bits
    if not 1 <= low_bits <= rest:
        raise ValueError("low_bits must be 1 .. 32 - radix_bits")
    w = _w2_array(w2, n)
    rng = np.random.default_rng([seed, radix_bits, partition, low_bits])
    start, odd = int(rng.integers(0, 1 << low_bits)), int(rng.integers(0, 1 << low_bits)) | 1
    if skip + n > (1 << low_bits):
        raise ValueError("not that many distinct keys in 2^low_bits")
    top, mask = np.uint64(partition) << np.uint64(rest), np.uint64((1 << low_bits) - 1)
    word = lambda idx: (((top | ((np.uint64(start) + idx * np.uint64(odd)) & mask)) << np.uint64(32)) | w)
    idx = np.arange(skip, skip + n, dtype=np.uint64)
    h, spare = word(idx), skip + n
    while not allow_special:                                              # a special word gives its place to the sequence's next one
        bad = np.flatnonzero((h == np.uint64(EMPTY_MIXED)) | (h == np.uint64(FILLER_MIXED)))
        if bad.size == 0:
            break
        if spare + bad.size > (1 << low_bits):
            raise ValueError("not that many distinct keys in 2^low_bits")
        idx[bad] = np.arange(spare, spare + bad.size, dtype=np.uint64)
        spare += bad.size
        h = word(idx)
    return h


def craft(radix_bits, partition, w2, n, seed=0, low_bits=None, allow_special=False):
    """n distinct raw uint64 keys whose mixed form has the top radix_bits bits of hash word 1 equal to partition and hash word 2
    exactly w2 (a scalar, or an array of n words: key i gets w2[i]).  They differ from each other in the remaining bits of hash
    word 1 only (the lowest low_bits of them)."""
    return unmix(craft_mixed(radix_bits, partition, w2, n, seed, low_bits, allow_special))


def ghosts(radix_bits, partition, w2, n, not_in, seed=0, low_bits=None):
    """n more keys of the same partition and w2 as craft(..., seed, low_bits) that are not among not_in (raw keys): what a table
    must report as a miss after walking everything the crafted keys put in its way."""
    not_in = np.asarray(not_in, dtype=np.uint64)
    g = unmix(craft_mixed(radix_bits, partition, w2, n, seed, low_bits, skip=not_in.size + n))
    if np.isin(g, not_in).any() or np.unique(g).size != n:
        raise ValueError("ghosts: the sequence met not_in (another seed, or more low_bits)")
    return g


def twins(keys, radix_bits, partition):
    """The keys whose mixed form equals that of `keys` except for the top radix_bits bits of hash word 1, which become `partition`:
    same slot, same tag, same remaining bits - in another partition's table."""
    if not 1 <= radix_bits <= 31 or not 0 <= partition < (1 << radix_bits):
        raise ValueError("partition must be one of the plan's 2^radix_bits")
    h = mix(keys)
    keep = np.uint64((1 << (64 - radix_bits)) - 1)
    return unmix((h & keep) | (np.uint64(partition) << np.uint64(64 - radix_bits)))


def partition_of(k, radix_bits, top_bits=64):
    """the partition of raw keys under a plan of radix_bits bits (0 bits: partition 0): the radix_bits bits of the mixed key below
    its 64 - top_bits owner bits (hash_top_bits of the C ABI; 64: no owner bits, the partition is the top of hash word 1)"""
    if not radix_bits:
        return np.zeros(np.asarray(k).shape, dtype=np.int64)
    return ((mix(k) >> np.uint64(top_bits - radix_bits)) & np.uint64((1 << radix_bits) - 1)).astype(np.int64)


# ---- one crafted key per row ---------------------------------------------------------------------------------------------------
def craft_rows(bits, bucket_of_row, top_bits=64, distinct=True, seed=0, keys_per_bucket=1):
    """One raw key per row whose radix bucket under a plan of `bits` bits is bucket_of_row[i]: the `bits` bits of hash word 1 below
    the 64 - top_bits owner bits (partition_of(keys, bits, top_bits) gives bucket_of_row back).  The owner bits (top_bits = 48: 16 of
    them) and the bits of hash word 1 below the bucket are pseudo-random per key; hash word 2 runs through an odd multiple of the
    key's number and never is 0xFFFFFFFF, so that neither the empty marker nor the wide filler (both end in that word) is made.
    distinct=True: the keys are pairwise distinct (key number = row).  distinct=False: the j-th row of a bucket (in row order) gets
    that bucket's key number j % keys_per_bucket - keys_per_bucket distinct keys per bucket, distinct across buckets."""
    b = np.asarray(bucket_of_row, dtype=np.int64)
    n, owner_bits = b.size, 64 - top_bits
    low_bits = 32 - owner_bits - bits
    if b.ndim != 1 or not 1 <= bits <= 31 or not 0 <= owner_bits <= 31 or low_bits < 0:
        raise ValueError("craft_rows: bits and 64 - top_bits must fit into hash word 1")
    if n and (b.min() < 0 or b.max() >= (1 << bits)):
        raise ValueError("craft_rows: a bucket outside the plan's 2^bits")
    if distinct:
        kid = np.arange(n, dtype=np.uint64)
    else:
        if keys_per_bucket < 1:
            raise ValueError("craft_rows: keys_per_bucket must be >= 1")
        order = np.argsort(b, kind="stable")
        sb = b[order]
        first = np.flatnonzero(np.r_[True, sb[1:] != sb[:-1]]) if n else np.zeros(0, dtype=np.int64)
        occ = np.empty(n, dtype=np.int64)
        occ[order] = np.arange(n) - np.repeat(first, np.diff(np.r_[first, n]))
        kid = (b * keys_per_bucket + occ % keys_per_bucket).astype(np.uint64)
    if kid.size and int(kid.max()) >= 2**32 - 1:
        raise ValueError("craft_rows: not that many distinct words in hash word 2")
    odd = np.uint64((0x9E3779B1 + 2 * seed) | 1)
    w2 = (_M32 + odd * (kid + np.uint64(1))) & _M32                       # a bijection of the key number; 0xFFFFFFFF only at number 2^32 - 1
    r = _fmix32((kid * np.uint64(0x85EBCA77) + np.uint64(seed * 0x9E3779B1 + 0x1234567)) & _M32)
    r2 = _fmix32(r ^ np.uint64(0x5BD1E995))
    low = r & np.uint64((1 << low_bits) - 1)
    owner = r2 & np.uint64((1 << owner_bits) - 1)
    w1 = (owner << np.uint64(32 - owner_bits)) | (b.astype(np.uint64) << np.uint64(low_bits)) | low if owner_bits \
        else (b.astype(np.uint64) << np.uint64(low_bits)) | low
    return unmix((w1 << np.uint64(32)) | w2)


def hash_w1(k):
    """hash word 1 of raw keys (csrc/fj_common.h fj_hash_w1) as uint32"""
    return (mix(k) >> np.uint64(32)).astype(np.uint32)


def unpack_wire(chunks_u8, dirw, fan_log0):
    """Wire chunks (uint8 array) + directory words -> (raw keys, bucket of every key, keys per chunk).  chunk_bytes = 1792 when
    fan_log0 >= 8 (three planes + the bucket's top bits), else 2048 (whole mixed keys)."""
    d = np.asarray(dirw).astype(np.int64) & 0xFFFFFFFF
    n = d.size
    bucket, cnt = d >> 9, d & 0x1FF
    if fan_log0 >= 8:
        c = np.asarray(chunks_u8, dtype=np.uint8).reshape(n, 1792)
        lo = c[:, :1024].copy().view(np.uint32).astype(np.uint64)
        mid = c[:, 1024:1536].copy().view(np.uint16).astype(np.uint64)
        hi = c[:, 1536:].astype(np.uint64)
        top = (bucket >> (fan_log0 - 8)).astype(np.uint64)[:, None]
        h = (top << np.uint64(56)) | (hi << np.uint64(48)) | (mid << np.uint64(32)) | lo
    else:
        h = np.asarray(chunks_u8, dtype=np.uint8).reshape(n, 2048).copy().view(np.uint64)
    mask = np.arange(256)[None, :] < cnt[:, None]
    return unmix(h[mask]), np.repeat(bucket, cnt), cnt
