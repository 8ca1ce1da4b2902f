"""NumPy restatement of the two wire formats a rank sends its peers besides the owner shuffle's chunks (keymix.unpack_wire): the
build-broadcast REGION and the per-partition sender FILTERS - test infrastructure, written from DESIGN.md sections 3 and 6 and
include/flashjoin_lab.h, not from the kernels.  It never imports the library; tests/test_wire_exact_cpu.py pins the constants it
restates to the sources and tests/test_wire_exact.py compares the library with it, byte for byte.

REGION ("Broadcast regions"): a rank's build keys after both passes of the global plan of `bits` bits, final partition
after final partition, without the radix bits the partition implies:
    u32 offs[nparts + 1] (keys before partition p) | low words u32[n] | the low 32 - bits bits of the high words as u16[n] (where
    they fit: 32 - bits <= 16) or u32[n] [| the build values u64[n]: regions of materialising joins]
every plane 16-byte aligned and followed by 16 bytes of padding.  Key i of partition p is unmix(((p << (32 - bits)) | mid[i]) << 32
| lo[i]).  A PIECE of consecutive partitions is a byte range of each plane (piece_span: part 0 = the offset table, 1 = low words,
2 = high-word plane, 3 = values, of the keys [k_lo, k_hi)).

FILTERS ("Sender-side precheck in chunk form"): one blocked Bloom filter of PFILT_BYTES = 4 KiB = 512 64-bit blocks per
FINAL partition; a key sets four bits of ONE block, all taken from hash word 2 (w2, the low mixed word): block = its top 9 bits
(umulhi(w2, 512)), bit positions w2 >> {0, 6, 12, 18} & 63.  An owner exports the filters of the partitions it owns: first-pass
bucket b of F0 = 2^fan_log0 belongs to rank (b * world) >> fan_log0, a bucket holds 2^(bits - fan_log0) consecutive partitions."""
import numpy as np

import keymix

_U = np.uint64
PFILT_BYTES = 4096
PF_BLOCKS = PFILT_BYTES // 8
PF_SHIFTS = (0, 6, 12, 18)
WIDE_MAXSRC = 16                        # ranks a build-broadcast join accepts
MAX_PIECES = 16


# ---- regions -------------------------------------------------------------------------------------------------------------------
def _pad16(nbytes):
    return (nbytes + 15) & ~15


def region_layout(bits, nkeys, with_vals=False):
    """-> nparts, mid_bytes, lo_off, mid_off, val_off, bytes"""
    nparts = 1 << bits
    mid_bytes = 2 if 32 - bits <= 16 else 4
    lo_off = _pad16((nparts + 1) * 4)
    mid_off = lo_off + _pad16(nkeys * 4) + 16
    val_off = mid_off + _pad16(nkeys * mid_bytes) + 16
    total = val_off + _pad16(nkeys * 8) + 16 if with_vals else val_off
    return nparts, mid_bytes, lo_off, mid_off, val_off, total


def live_mask(bits, nkeys, with_vals=False):
    """bool per byte of a region: True where offs, lo[0:n], mid[0:n] (and vals[0:n]) lie - everything else is padding"""
    nparts, mb, lo_off, mid_off, val_off, total = region_layout(bits, nkeys, with_vals)
    m = np.zeros(total, dtype=bool)
    m[: (nparts + 1) * 4] = True
    m[lo_off: lo_off + 4 * nkeys] = True
    m[mid_off: mid_off + mb * nkeys] = True
    if with_vals:
        m[val_off: val_off + 8 * nkeys] = True
    return m


def _plane(region, off, n, dtype):
    return np.frombuffer(np.ascontiguousarray(region[off: off + n * np.dtype(dtype).itemsize]).tobytes(), dtype=dtype)


def unpack_region(region_u8, bits, nkeys, with_vals=False):
    """-> offs (int64[nparts + 1]), raw keys (uint64[n]), partition of every key (int64[n]) [, values (uint64[n])].  Raises
    ValueError when the offset table is no exclusive scan that ends at nkeys (nothing can be decoded then)."""
    region = np.asarray(region_u8, dtype=np.uint8)
    nparts, mb, lo_off, mid_off, val_off, total = region_layout(bits, nkeys, with_vals)
    if region.size != total:
        raise ValueError(f"a region of {nkeys} keys under {bits} bits has {total} bytes, not {region.size}")
    offs = _plane(region, 0, nparts + 1, np.uint32).astype(np.int64)
    if offs[0] != 0 or offs[-1] != nkeys or np.any(np.diff(offs) < 0):
        raise ValueError(f"the offset table is no exclusive scan ending at {nkeys}: starts {offs[:4].tolist()}, ends {offs[-3:].tolist()}")
    lo = _plane(region, lo_off, nkeys, np.uint32).astype(_U)
    mid = _plane(region, mid_off, nkeys, np.uint16 if mb == 2 else np.uint32).astype(_U)
    part = np.repeat(np.arange(nparts, dtype=np.int64), np.diff(offs))
    h = ((((part.astype(_U) << _U(32 - bits)) | mid) << _U(32)) | lo)
    out = (offs, keymix.unmix(h), part)
    return out + (_plane(region, val_off, nkeys, np.uint64),) if with_vals else out


def pack_region(keys, bits, vals=None, fill=0xA5):
    """The region of `keys` (one of the many legal ones: inside a partition the keys stand in input order), padding = `fill`."""
    keys = np.asarray(keys, dtype=_U)
    n = keys.size
    nparts, mb, lo_off, mid_off, val_off, total = region_layout(bits, n, vals is not None)
    part = keymix.partition_of(keys, bits)
    order = np.argsort(part, kind="stable")
    h = keymix.mix(keys[order])
    r = np.full(total, fill, dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum(np.bincount(part, minlength=nparts))]).astype(np.uint32)
    r[: (nparts + 1) * 4] = offs.view(np.uint8)
    r[lo_off: lo_off + 4 * n] = (h & _U(0xFFFFFFFF)).astype(np.uint32).view(np.uint8)
    midw = (h >> _U(32)) & _U((1 << (32 - bits)) - 1)
    r[mid_off: mid_off + mb * n] = midw.astype(np.uint16 if mb == 2 else np.uint32).view(np.uint8)
    if vals is not None:
        r[val_off: val_off + 8 * n] = np.asarray(vals, dtype=_U)[order].view(np.uint8)
    return r


def piece_span(bits, nkeys, k_lo, k_hi, part):
    """-> (offset, bytes) of part `part` of the keys [k_lo, k_hi) inside a region of nkeys keys (values included in the layout)"""
    if not (0 <= k_lo <= k_hi <= nkeys and 0 <= part <= 3):
        raise ValueError("piece_span: bad range")
    nparts, mb, lo_off, mid_off, val_off, _ = region_layout(bits, nkeys, True)
    if part == 0:
        return 0, (nparts + 1) * 4
    off, width = {1: (lo_off, 4), 2: (mid_off, mb), 3: (val_off, 8)}[part]
    return off + k_lo * width, (k_hi - k_lo) * width


def piece_bounds(offs, pieces):
    """key index at which piece q of `pieces` pieces of consecutive partitions starts; [pieces] = all keys"""
    nparts = len(offs) - 1
    return [int(offs[nparts * q // pieces]) for q in range(pieces)] + [int(offs[nparts])]


# ---- per-partition filters -------------------------------------------------------------------------------------------------------
def pf_bits(h, shifts=PF_SHIFTS):
    """mixed keys -> (block, mask): the 64-bit block of the partition's filter and the four bits a key sets / needs there"""
    w2 = np.asarray(h, dtype=_U) & _U(0xFFFFFFFF)
    block = ((w2 * _U(PF_BLOCKS)) >> _U(32)).astype(np.int64)
    mask = np.zeros(w2.shape, dtype=_U)
    for s in shifts:
        mask |= _U(1) << ((w2 >> _U(s)) & _U(63))
    return block, mask


def part_filters(raw_keys, bits, shifts=PF_SHIFTS):
    """-> uint64[nparts][512]: the filters of all final partitions of a plan of `bits` bits over these build keys"""
    h = keymix.mix(np.asarray(raw_keys, dtype=_U))
    f = np.zeros((1 << bits, PF_BLOCKS), dtype=_U)
    if h.size == 0:
        return f
    w2 = h & _U(0xFFFFFFFF)
    block = (w2 * _U(PF_BLOCKS)) >> _U(32)
    word = (h >> _U(64 - bits)) * _U(PF_BLOCKS) + block
    ids = np.unique(np.concatenate([(word << _U(6)) | ((w2 >> _U(s)) & _U(63)) for s in shifts]))
    w, bit = (ids >> _U(6)).astype(np.int64), _U(1) << (ids & _U(63))
    starts = np.flatnonzero(np.r_[True, w[1:] != w[:-1]])
    f.reshape(-1)[w[starts]] = np.bitwise_or.reduceat(bit, starts)
    return f


def admits(filters, raw_keys, bits, shifts=PF_SHIFTS, part_xor=0):
    """bool per key: the filter of the key's partition has all four of its bits.  (shifts, part_xor: seeded defects of
    tests/test_wire_exact_cpu.py.)"""
    h = keymix.mix(np.asarray(raw_keys, dtype=_U))
    block, mask = pf_bits(h, shifts)
    part = (h >> _U(64 - bits)).astype(np.int64) ^ part_xor
    return (np.asarray(filters).reshape(-1, PF_BLOCKS)[part, block] & mask) == mask


def filter_range(bits, fan_log0, world, rank):
    """-> (first partition, partitions) whose filters owner `rank` exports: its first-pass buckets' partitions"""
    f0, rest = 1 << fan_log0, 1 << (bits - fan_log0)
    lo, hi = -(-rank * f0 // world), -(-(rank + 1) * f0 // world)
    return lo * rest, (hi - lo) * rest


def owner_of_bucket(bucket, fan_log0, world):
    return (np.asarray(bucket, dtype=np.int64) * world) >> fan_log0


# ---- the plan, as far as the tests steer it ----------------------------------------------------------------------------------------
def fan_logs(bits, max_fan_log=9):
    """radix bits per pass (Plan: one pass up to 9 bits, two up to 18, extra bits to the earlier passes)"""
    npass = 0 if bits == 0 else 1 if bits <= max_fan_log else 2 if bits <= 2 * max_fan_log else -(-bits // max_fan_log)
    return [bits // npass + (1 if i < bits % npass else 0) for i in range(npass)]


def nominal_rows(bits, target=16):
    """a total build side whose plan has exactly `bits` bits under plan_target_keys = target (< 4096: no free extra bit)"""
    return target << bits
