"""What a rank sends its peers besides the owner shuffle's chunks - broadcast regions and per-partition filters - the part that needs
no GPU: the NumPy model's self-checks (tests/wire_model.py), the inputs of every case of tests/test_wire_exact.py (built HERE, so that
both files see the same arrays), the checks both files apply to a region and to a prechecked piece, the proof that each input tells the
seeded defects below from the correct model, and the constants of the sources all of this is derived from, pinned by name.

THE SEEDED DEFECTS (what a wrong kernel could do while the count-and-bound tests of tests/test_gpu_parity.py stay green)
  regions (region_defect)
  R-a  the first / the last key of a partition whose offset is no multiple of 4 (low plane) or of 8 / 4 (u16 / u32 plane) is not written
  R-b  ... is written one element early, into the neighbour partition
  R-c  the second stage() of a chunk that straddles a 512-key tile is skipped: the partition's first key beyond its first tile is missing
  R-d  offs is inclusive instead of exclusive
  R-e  a piece bound is taken from partition nparts * q / pieces + 1
  R-f  values are placed in another order than the keys
  R-g  the u16 plane is masked with one bit too few
  R-h  piece_span uses 4 bytes per element for a u16 plane
  filters
  F-a  one of the four bit positions is ignored by the test (one sub-case per position)
  F-b  a key is tested against the filter of partition p ^ 1
  F-c  the export leaves out keys of a partition (its last chunk, the keys beyond lane 63 of a chunk)
  F-d  a wave drops the survivor of its last lane
  F-e  an XCD whose bucket list has empty buckets in it skips the chunks behind them (or visits chunks twice: only the exact `kept` and
       the exact multiset on the wire tell that)
  F-f  a workgroup never takes a second batch
  F-g  a chunk without survivors is reported with its old count
  F-h  the sample ignores `stride`
REGION_DETECTS / PROBE_DETECTS / EXPORT_DETECTS list, per case, the defects it is a test of; a case is listed only for what it detects.

PLANS  every plan is reached with plan_target_keys = 16 and a NOMINAL total build side of 16 << bits rows (WM.nominal_rows): bits 12
(single-workgroup scan, u32 plane), 13 (wide scan, two workgroups), 16 and 17 (wide scan, u16 plane) for the regions; bits 10, 12, 16, 17
= first passes of 32, 64, 256, 512 buckets for the filters.  The GPU file reads the bits back from the engine.

REGION KEY SETS (region_keys(kind, bits))
  crafted   EDGE_SIZES = 0 .. 9 keys (every offset residue mod 8 at both ends), 255 .. 513 and 1023, 1025 keys (a chunk boundary, a tile
            boundary, a tile crossed inside a chunk) in neighbouring partitions - behind 5 empty partitions at the start of the table,
            in front of and behind an empty run across partition 4096 (the wide scan's workgroup seam; seam_of() at 12 bits), in front
            of 7 empty partitions at the table's end; 3 keys in each partition a piece of 16 starts at; 300 partitions of 1 - 5 keys
  random    200 000 random keys             one   5 000 keys, all in partition nparts - 3             none  no key
FILTER BUILD SIDES (filter_build(name, bits))   random: 50 000 random keys; crafted: partitions of 0, 1, 255, 256, 257, 700 and 3000 keys,
  three times over the table (so that every owner of 3 and most of 8 hold some); dups: crafted, every key three times, shuffled
PROBE SIDES (probe_side(name, bits) -> build side's name, keys): see PROBE_CASES
"""
import functools
import os
import re
import shutil

import numpy as np
import pytest

import keymix
import wire_model as WM
from conftest import ROOT

HERE = "tests/test_wire_exact_cpu.py"
CSRC = os.path.join(ROOT, "flash_hash_join_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
_U = np.uint64
CHUNK, TILE = 256, 512
TARGET = 16                                                     # plan_target_keys of every case
REGION_BITS = (12, 13, 16, 17)
FILTER_BITS = {32: 10, 64: 12, 256: 16, 512: 17}                # first-pass buckets -> bits
PIECES = (1, 2, 3, 5, 7, 16)
EDGE_SIZES = tuple(range(10)) + (255, 256, 257, 511, 512, 513, 1023, 1025)
FILTER_SIZES = (0, 1, 255, 256, 257, 700, 3000)
FA_PART_SIZE, FA_MISSES = 3000, 20_000
VAL_MUL, VAL_ADD = 0x9E3779B97F4A7C15, 3


# ---- the constants, read from the sources ------------------------------------------------------------------------------------------------
def _source(d, name):
    with open(os.path.join(d, name)) as f:
        return f.read()


def _gone(what, pattern):
    return f"{what}: the sources no longer say /{pattern}/ - {HERE} and tests/wire_model.py are written against it: read the new text, then update"


def _num(text, pattern, what):
    m = re.search(pattern, text)
    assert m, _gone(what, pattern)
    return int(m.group(1), 0)


def _says(text, fragment, what):
    assert fragment in text, _gone(what, fragment)


def constants(csrc=CSRC, include=INCLUDE):
    c = {}
    internal, pack, bcast, stream = (_source(csrc, n) for n in ("fj_internal.h", "fj_pack.hip", "fj_bcast.hip", "fj_stream.hip"))
    # workgroups of a partition pass: at most rows / (F * 128), and 512 - one partial chunk per workgroup and bucket (check_precheck)
    _says(_source(csrc, "fj_plan.hip"), "const u64 g64 = std::min<u64>(chunks / tile_chunks, rows / ((u64)F * 128));\n    return (u32)std::min<u64>(512, std::max<u64>(1, g64));",
          "pass_groups")
    c["FJ_PFILT_BYTES"] = _num(internal, r"#define\s+FJ_PFILT_BYTES\s+(\d+)u", "FJ_PFILT_BYTES")
    c["FJ_PF_COUNTERS"] = _num(internal, r"#define\s+FJ_PF_COUNTERS\s+(\d+)u", "FJ_PF_COUNTERS")
    c["FJ_WIDE_MAXSRC"] = _num(internal, r"#define\s+FJ_WIDE_MAXSRC\s+(\d+)u", "FJ_WIDE_MAXSRC")
    c["batch"] = _num(pack, r"hipLaunchKernelGGL\(fj_part_filter_inplace<(\d+)>,", "the batch size of fj_part_filter_inplace")
    c["grid_per_cu"] = _num(stream, r"fj_launch_part_filter_inplace\(it\.cs, filters, pk\.part_shift, &c->d_sc->pack_kept, c->d_sc->pack_xcd, (\d+)u \* c->num_cus, s\)",
                            "the grid of fj_part_filter_inplace")
    _says(pack, "grid = (grid + 7u) & ~7u;", "the grid of fj_part_filter_inplace, rounded to 8")
    _says(pack, "block = __umulhi(w, FJ_PFILT_BYTES / 8u);", "pf_bits: the block")
    m = re.search(r"mask = \(1ull << \(w & 63u\)\) \| \(1ull << \(\(w >> (\d+)\) & 63u\)\) \| \(1ull << \(\(w >> (\d+)\) & 63u\)\) \| \(1ull << \(\(w >> (\d+)\) & 63u\)\);", pack)
    assert m, _gone("pf_bits: the four shifts", "mask = (1ull << (w & 63u)) | ...")
    c["pf_shifts"] = (0,) + tuple(int(x) for x in m.groups())
    _says(pack, "const u32 xcd = blockIdx.x & 7u;", "fj_part_filter_inplace: XCD x takes buckets x, x + 8, ...")
    c["DC_T"] = _num(bcast, r"constexpr u32 DC_T = (\d+);", "DC_T")
    c["DP_NT"] = _num(bcast, r"constexpr u32 DP_NT = (\d+);", "DP_NT")
    c["scan_sweep"] = _num(bcast, r"for \(u32 base = 0; base < nparts; base \+= (\d+)\) \{", "the sweep of fj_dense_scan")
    m = re.search(r"if \(L\.nparts >= (\d+)u && L\.nparts <= \(1u << (\d+)\)\) \{", bcast)
    assert m, _gone("the window of fj_dense_scan_wide", "if (L.nparts >= 8192u && L.nparts <= (1u << 19)) {")
    c["wide_scan"] = (int(m.group(1)), 1 << int(m.group(2)))
    c["wide_scan_group"] = _num(bcast, r"fj_dense_scan_wide, dim3\(L\.nparts / (\d+)u\)", "fj_dense_scan_wide: counts per workgroup")
    _says(bcast, "L->bits = (u32)p.bits; L->nparts = 1u << p.bits; L->mid_bytes = 32 - p.bits <= 16 ? 2u : 4u;", "layout_of: the plane width")
    _says(bcast, "L->lo_off = (((size_t)L->nparts + 1) * 4 + 15) & ~(size_t)15;\n    L->mid_off = L->lo_off + ((nkeys * 4 + 15) & ~(size_t)15) + 16;\n"
                 "    L->val_off = L->mid_off + ((nkeys * L->mid_bytes + 15) & ~(size_t)15) + 16;", "the three lines of layout_of")
    _says(bcast, "L->bytes = with_vals ? L->val_off + ((nkeys * 8 + 15) & ~(size_t)15) + 16 : L->val_off;", "layout_of: the values")
    c["max_pieces"] = _num(bcast, r"if \(pieces < 1 \|\| pieces > (\d+)\) return set_err\(\"fj_bcast_pack: pieces must be 1\.\.16\"\);", "the pieces limit")
    _says(_source(include, "flashjoin_lab.h"), "int fj_bcast_piece_span(size_t nb_total, size_t nkeys, size_t k_lo, size_t k_hi, int part, size_t* offset, size_t* bytes);",
          "fj_bcast_piece_span")
    return c


def test_the_constants_are_what_the_sources_say():
    c = constants()
    moved = f"a constant of the wire formats moved: tests/wire_model.py, {HERE} and tests/test_wire_exact.py are stated for these - read the new one, then update"
    assert (c["FJ_PFILT_BYTES"], c["pf_shifts"], c["FJ_WIDE_MAXSRC"], c["max_pieces"]) == (WM.PFILT_BYTES, WM.PF_SHIFTS, WM.WIDE_MAXSRC, WM.MAX_PIECES), moved
    assert (WM.PFILT_BYTES, WM.PF_SHIFTS, WM.WIDE_MAXSRC, WM.MAX_PIECES) == (4096, (0, 6, 12, 18), 16, 16), moved
    assert (c["FJ_PF_COUNTERS"], c["batch"], c["grid_per_cu"]) == (4, 4, 4), moved
    assert (c["DC_T"], c["DP_NT"], c["scan_sweep"], c["wide_scan"], c["wide_scan_group"]) == (TILE, 256, 16384, (8192, 1 << 19), 4096), moved
    assert max(PIECES) == c["max_pieces"]


@pytest.mark.parametrize("where,name,old,new", [
    ("csrc", "fj_internal.h", "#define FJ_PFILT_BYTES 4096u", "#define FJ_PFILT_BYTES 8192u"),
    ("csrc", "fj_internal.h", "#define FJ_PF_COUNTERS 4u", "#define FJ_PF_COUNTERS 2u"),
    ("csrc", "fj_internal.h", "#define FJ_WIDE_MAXSRC 16u", "#define FJ_WIDE_MAXSRC 8u"),
    ("csrc", "fj_pack.hip", "hipLaunchKernelGGL(fj_part_filter_inplace<4>,", "hipLaunchKernelGGL(fj_part_filter_inplace<8>,"),
    ("csrc", "fj_stream.hip", "c->d_sc->pack_xcd, 4u * c->num_cus, s)", "c->d_sc->pack_xcd, 2u * c->num_cus, s)"),
    ("csrc", "fj_pack.hip", "grid = (grid + 7u) & ~7u;", "grid = (grid + 3u) & ~3u;"),
    ("csrc", "fj_pack.hip", "(1ull << ((w >> 18) & 63u));", "(1ull << ((w >> 19) & 63u));"),
    ("csrc", "fj_pack.hip", "(1ull << ((w >> 6) & 63u))", "(1ull << ((w >> 5) & 63u))"),
    ("csrc", "fj_bcast.hip", "constexpr u32 DC_T = 512;", "constexpr u32 DC_T = 1024;"),
    ("csrc", "fj_bcast.hip", "constexpr u32 DP_NT = 256;", "constexpr u32 DP_NT = 512;"),
    ("csrc", "fj_bcast.hip", "base < nparts; base += 16384) {", "base < nparts; base += 4096) {"),
    ("csrc", "fj_bcast.hip", "L.nparts <= (1u << 19)) {", "L.nparts <= (1u << 20)) {"),
    ("csrc", "fj_bcast.hip", "L->mid_bytes = 32 - p.bits <= 16 ? 2u : 4u;", "L->mid_bytes = 32 - p.bits < 16 ? 2u : 4u;"),
    ("csrc", "fj_bcast.hip", "L->mid_off = L->lo_off + ((nkeys * 4 + 15) & ~(size_t)15) + 16;", "L->mid_off = L->lo_off + ((nkeys * 4 + 15) & ~(size_t)15);"),
    ("csrc", "fj_bcast.hip", "if (pieces < 1 || pieces > 16)", "if (pieces < 1 || pieces > 32)"),
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


# ---- the model's self-checks ---------------------------------------------------------------------------------------------------------------
def test_layout_worked_by_hand():
    # 5 bits, 3 keys: offs 33 words = 132 -> 144; lo 12 -> 16 + 16; u32 plane 12 -> 16 + 16; vals 24 -> 32 + 16
    assert WM.region_layout(5, 3, True) == (32, 4, 144, 176, 208, 256) and WM.region_layout(5, 3)[5] == 208
    # 16 bits: the first u16 plane; 8 keys: lo 32 + 16, mid 16 + 16
    assert WM.region_layout(16, 8) == (65536, 2, 262160, 262208, 262240, 262240) and WM.region_layout(15, 8)[1] == 4
    assert WM.region_layout(12, 0, True) == (4096, 4, 16400, 16416, 16432, 16448)
    assert WM.piece_span(16, 8, 2, 5, 0) == (0, 65537 * 4) and WM.piece_span(16, 8, 2, 5, 1) == (262160 + 8, 12)
    assert WM.piece_span(16, 8, 2, 5, 2) == (262208 + 4, 6) and WM.piece_span(16, 8, 2, 5, 3) == (262240 + 16, 24)
    assert WM.piece_span(12, 8, 2, 5, 2)[1] == 12
    assert WM.filter_range(10, 5, 3, 0) == (0, 11 * 32) and WM.filter_range(10, 5, 3, 1) == (11 * 32, 11 * 32) and WM.filter_range(10, 5, 3, 2) == (22 * 32, 10 * 32)
    assert [WM.fan_logs(b) for b in (10, 12, 13, 16, 17, 20)] == [[5, 5], [6, 6], [7, 6], [8, 8], [9, 8], [7, 7, 6]]


def test_pf_bits_worked_by_hand():
    # w2 = 0x00FFF041: bits 0-5 = 1, 6-11 = 1, 12-17 = 0x3F, 18-23 = 0x3F; the top 9 bits (block) = 1
    block, mask = WM.pf_bits(np.array([0xABCD000000FFF041, 0xFFFFFFFF, 0], dtype=_U))
    assert block.tolist() == [1, 511, 0] and mask.tolist() == [(1 << 1) | (1 << 63), 1 << 63, 1]
    k = keymix.unmix(np.array([(5 << 54) | 0x00FFF041], dtype=_U))           # partition 5 of a 10-bit plan
    f = WM.part_filters(k, 10)
    assert f[5, 1] == (1 << 1) | (1 << 63) and np.count_nonzero(f) == 1 and WM.admits(f, k, 10).all()
    assert not WM.admits(f, keymix.unmix(np.array([(4 << 54) | 0x00FFF041, (5 << 54) | 0x00FFF042], dtype=_U)), 10).any()


# ---- regions: inputs, the check, the defects -----------------------------------------------------------------------------------------------
def vals_of(keys):
    return np.asarray(keys, dtype=_U) * _U(VAL_MUL) + _U(VAL_ADD)


def seam_of(bits):
    """where the crafted set's inner run of empty partitions lies: across partition 4096, the wide scan's workgroup seam; a 12-bit plan
    (one workgroup, one sweep) has no seam: anywhere that no piece starts at"""
    return 4096 if bits >= 13 else (1 << bits) // 2 + 37


@functools.lru_cache(maxsize=None)
def crafted_counts(bits):
    """keys per partition of the `crafted` region key set, and the partitions that must stay empty"""
    nparts, seam, E = 1 << bits, seam_of(bits), len(EDGE_SIZES)
    cnt = np.zeros(nparts, dtype=np.int64)
    empty = np.zeros(nparts, dtype=bool)
    empty[:5] = True; empty[seam - 6: seam + 6] = True; empty[nparts - 7:] = True
    for at in (5, seam - 6 - E, seam + 6, nparts - 7 - E):
        cnt[at: at + E] = EDGE_SIZES
        empty[at] = True                                         # (the 0 of EDGE_SIZES)
    taken = empty | (cnt > 0)
    for pieces in PIECES:                                        # 3 keys where a piece starts (R-e), unless the partition has its role already
        for q in range(1, pieces):
            p = nparts * q // pieces
            if not taken[p]:
                cnt[p] = 3; taken[p] = True
    rng = np.random.default_rng([20261101, bits])
    free = np.flatnonzero(~taken)
    at = rng.choice(free, 300, replace=False)
    cnt[at] = rng.integers(1, 6, 300)
    assert not cnt[empty].any()
    return cnt


@functools.lru_cache(maxsize=None)
def region_keys(kind, bits):
    nparts = 1 << bits
    rng = np.random.default_rng([20261102, bits])
    if kind == "crafted":
        k = keymix.craft_rows(bits, rng.permutation(np.repeat(np.arange(nparts), crafted_counts(bits))))
    elif kind == "random":
        k = rng.integers(0, 2**64, 200_000, dtype=_U)
    elif kind == "one":
        k = keymix.craft_rows(bits, np.full(5000, nparts - 3))
    elif kind == "none":
        k = np.zeros(0, dtype=_U)
    else:
        raise KeyError(kind)
    assert np.unique(k).size == k.size
    k.setflags(write=False)
    return k


REGION_KINDS = ("crafted", "random", "one", "none")


def check_region(region_u8, keys, bits, with_vals, what=""):
    """A region - as a byte array, padding included - against the keys it was packed from: the offset table is the exclusive scan of the
    partition sizes, every partition holds exactly its keys (in any order), value i belongs to key i.  What tests/test_wire_exact.py
    asserts of the library's regions and what the defect proofs below apply to the model's."""
    keys = np.asarray(keys, dtype=_U)
    n, nparts = keys.size, 1 << bits
    want_offs = np.concatenate([[0], np.cumsum(np.bincount(keymix.partition_of(keys, bits), minlength=nparts))])
    offs = np.frombuffer(np.ascontiguousarray(region_u8[: 4 * (nparts + 1)]).tobytes(), dtype=np.uint32).astype(np.int64)
    bad = np.flatnonzero(offs != want_offs)
    assert bad.size == 0, f"{what}: offs differs from the exclusive scan at {bad.size} partitions, the first: offs[{bad[0]}] = {offs[bad[0]]}, expected {want_offs[bad[0]]}"
    out = WM.unpack_region(region_u8, bits, n, with_vals)
    got, part = out[1], out[2]
    o_got, o_want = np.lexsort((got, part)), np.lexsort((keys, keymix.partition_of(keys, bits)))
    diff = np.flatnonzero(got[o_got] != keys[o_want])
    if diff.size:
        i = int(diff[0]); p = int(part[o_got][i])
        raise AssertionError(f"{what}: {diff.size} keys differ; the first in partition {p} (offs {offs[p]} .. {offs[p + 1]}): decoded {int(got[o_got][i]):#018x} "
                             f"(region index {int(o_got[i])}), expected {int(keys[o_want][i]):#018x}")
    if with_vals:
        wrong = np.flatnonzero(out[3] != vals_of(got))
        assert wrong.size == 0, f"{what}: {wrong.size} values do not belong to the key at their index, the first at index {wrong[0]} (partition {part[wrong[0]]})"
    return offs


def check_padding(buf_u8, guard, bits, n, with_vals, fill=0xA5, what=""):
    """buf = guard | region | guard, pre-filled with `fill`: every byte outside offs, lo[0:n], mid[0:n], vals[0:n] still holds it"""
    live = WM.live_mask(bits, n, with_vals)
    assert buf_u8.size == live.size + 2 * guard
    g = np.flatnonzero(np.concatenate([buf_u8[:guard], buf_u8[guard + live.size:]]) != fill)
    assert g.size == 0, f"{what}: {g.size} GUARD bytes were written (a neighbour rank's region in the real buffer), the first at {g[0] - guard if g[0] < guard else g[0] - guard + live.size} relative to the region"
    pad = np.flatnonzero((buf_u8[guard: guard + live.size] != fill) & ~live)
    assert pad.size == 0, f"{what}: {pad.size} padding bytes inside the region were written, the first at byte {pad[0]} (planes at {WM.region_layout(bits, n, with_vals)[2:5]})"


def _elems(region, off, n, dtype):
    return region[off: off + n * np.dtype(dtype).itemsize].view(dtype)


def region_defect(keys, bits, with_vals, defect):
    """the model's region of `keys` with one seeded defect; None where the input gives the defect nothing to act on"""
    keys = np.asarray(keys, dtype=_U)
    n = keys.size
    r = WM.pack_region(keys, bits, vals_of(keys) if with_vals else None)
    nparts, mb, lo_off, mid_off, val_off, _ = WM.region_layout(bits, n, with_vals)
    offs = _elems(r, 0, nparts + 1, np.uint32).astype(np.int64)
    size = np.diff(offs)
    lo, mid = _elems(r, lo_off, n, np.uint32), _elems(r, mid_off, n, np.uint16 if mb == 2 else np.uint32)
    mg = 16 // mb
    name, _, arg = defect.partition(":")
    if name in ("R-a", "R-b"):
        plane, end = arg.split("-")
        arr, per = (lo, 4) if plane == "lo" else (mid, mg)
        if end == "first":
            p = np.flatnonzero((size > 0) & (offs[:-1] % per != 0))
            at = offs[p]
        else:
            p = np.flatnonzero((size > 0) & (offs[1:] % per != 0))
            at = offs[p + 1] - 1
        if p.size == 0:
            return None
        if name == "R-b":
            to = at - 1 if end == "first" else at + 1
            ok = (to >= 0) & (to < n)
            if not ok.any():
                return None
            moved = arr[at[ok]].copy()
            arr[at[ok]] = 0xA5A5A5A5 if arr.dtype == np.uint32 else 0xA5A5
            arr[to[ok]] = moved
        else:
            arr[at] = 0xA5A5A5A5 if arr.dtype == np.uint32 else 0xA5A5
    elif name == "R-c":
        first_tile_end = (offs[:-1] & ~7) + TILE
        p = np.flatnonzero(offs[1:] > first_tile_end)
        if p.size == 0:
            return None
        lo[first_tile_end[p]] = 0xA5A5A5A5
    elif name == "R-d":
        if n == 0:
            return None
        _elems(r, 0, nparts + 1, np.uint32)[:-1] = offs[1:]
    elif name == "R-f":
        if not with_vals:
            return None
        p = np.flatnonzero(size >= 2)
        if p.size == 0:
            return None
        v = _elems(r, val_off, n, np.uint64)
        a, b = v[offs[p]].copy(), v[offs[p] + 1].copy()
        v[offs[p]], v[offs[p] + 1] = b, a
    elif name == "R-g":
        if mb != 2:
            return None
        mid &= np.uint16((1 << (32 - bits - 1)) - 1)
    else:
        raise KeyError(defect)
    return r


REGION_DEFECTS = ("R-a:lo-first", "R-a:lo-last", "R-a:mid-first", "R-a:mid-last", "R-b:lo-first", "R-b:lo-last", "R-b:mid-first", "R-b:mid-last",
                  "R-c", "R-d", "R-f", "R-g")
# which defects each region key set is a test of (guards tests/test_wire_exact.py test_regions_decoded[<kind>-...]); R-e and R-h are host
# arithmetic: test_piece_bounds_and_spans_tell_their_defects
REGION_DETECTS = {"crafted": set(REGION_DEFECTS), "random": set(REGION_DEFECTS) - {"R-c"}, "one": {"R-c", "R-d", "R-f", "R-g"}, "none": set()}


@pytest.mark.parametrize("bits", REGION_BITS)
@pytest.mark.parametrize("kind", REGION_KINDS)
def test_every_region_case_tells_its_defects_from_the_model(kind, bits):
    keys = region_keys(kind, bits)
    for with_vals in (False, True):
        good = WM.pack_region(keys, bits, vals_of(keys) if with_vals else None)
        offs = check_region(good, keys, bits, with_vals, "the model's own region")
        assert offs[-1] == keys.size
        check_padding(np.concatenate([np.full(64, 0xA5, np.uint8), good, np.full(64, 0xA5, np.uint8)]), 64, bits, keys.size, with_vals)
        for d in REGION_DEFECTS:
            applies = d in REGION_DETECTS[kind] and not (d == "R-g" and bits < 16) and not (d == "R-f" and not with_vals)
            bad = region_defect(keys, bits, with_vals, d)
            if not applies:
                continue
            assert bad is not None, f"test_regions_decoded[{kind}-{bits}]: nothing for defect {d} to act on"
            with pytest.raises((AssertionError, ValueError)):
                check_region(bad, keys, bits, with_vals)


@pytest.mark.parametrize("bits", REGION_BITS)
def test_the_crafted_region_keys_are_what_part_a_asks_for(bits):
    cnt, nparts, seam = crafted_counts(bits), 1 << bits, seam_of(bits)
    keys = region_keys("crafted", bits)
    assert np.array_equal(np.bincount(keymix.partition_of(keys, bits), minlength=nparts), cnt)
    offs = np.concatenate([[0], np.cumsum(cnt)])
    full = cnt > 0
    assert set((offs[:-1][full] % 8).tolist()) == set(range(8)) == set((offs[1:][full] % 8).tolist()), "every offset residue mod 8 at both ends"
    assert not cnt[:5].any() and not cnt[nparts - 7:].any() and not cnt[seam - 6: seam + 6].any() and cnt[seam - 7] == 1025 and cnt[seam + 7] == 1
    assert cnt[nparts - 8] == 1025 and cnt[6] == 1
    assert ((offs[:-1] & ~7) + TILE < offs[1:]).any(), "a partition that leaves its first tile"
    assert ((offs[:-1][full] // TILE) != ((offs[1:][full] - 1) // TILE)).any()
    one = region_keys("one", bits)
    assert np.unique(keymix.partition_of(one, bits)).tolist() == [nparts - 3] and region_keys("random", bits).size == 200_000
    if bits >= 16:                                               # R-g: keys whose plane entry has its top bit set
        assert ((keymix.mix(keys) >> _U(32 + 31 - bits)) & _U(1)).any()


@pytest.mark.parametrize("bits", REGION_BITS)
@pytest.mark.parametrize("kind", ("crafted", "random"))
def test_piece_bounds_and_spans_tell_their_defects(kind, bits):
    """R-e: for every piece count some bound sits on a partition that holds keys, so the next partition's offset differs.  R-h: a u16
    plane's span under 4 bytes per element differs in offset or length for every piece that holds keys."""
    keys = region_keys(kind, bits)
    nparts = 1 << bits
    offs = np.concatenate([[0], np.cumsum(np.bincount(keymix.partition_of(keys, bits), minlength=nparts))])
    for pieces in PIECES[1:]:
        b = WM.piece_bounds(offs, pieces)
        assert b[0] == 0 and b[-1] == keys.size and len(b) == pieces + 1
        if (kind, bits, pieces) == ("crafted", 13, 2):          # its one inner bound is the seam, which stays empty: `random` is the test of it
            continue
        assert any(offs[nparts * q // pieces + 1] != b[q] for q in range(pieces)), f"test_regions_decoded[{kind}-{bits}]: defect R-e goes unnoticed at {pieces} pieces"
        if bits >= 16:
            _, _, _, mid_off, _, _ = WM.region_layout(bits, keys.size, True)
            for q in range(pieces):
                if b[q + 1] > b[q]:
                    assert WM.piece_span(bits, keys.size, b[q], b[q + 1], 2) != (mid_off + 4 * b[q], 4 * (b[q + 1] - b[q])), "defect R-h goes unnoticed"
    # the spans of all pieces tile the live bytes of the region exactly
    for with_vals in (False, True):
        live = np.zeros(WM.region_layout(bits, keys.size, True)[5], dtype=np.int64)
        b = WM.piece_bounds(offs, 5)
        for q in range(5):
            for part in ([0] if q == 0 else []) + [1, 2] + ([3] if with_vals else []):
                o, nbytes = WM.piece_span(bits, keys.size, b[q], b[q + 1], part)
                live[o: o + nbytes] += 1
        want = np.zeros(live.size, dtype=bool)
        _, mb, lo_off, mid_off, val_off, _ = WM.region_layout(bits, keys.size, True)
        want[: 4 * (nparts + 1)] = True; want[lo_off: lo_off + 4 * keys.size] = True; want[mid_off: mid_off + mb * keys.size] = True
        if with_vals:
            want[val_off: val_off + 8 * keys.size] = True
        assert np.array_equal(live, want.astype(np.int64))


# ---- part B: range joins ---------------------------------------------------------------------------------------------------------------------
JOIN_WORLDS, JOIN_PIECES = (2, 3, 8), (2, 5, 16)
JOIN_SHAPES = {"u32": (70_000, 300_001, 32), "u16": (600_000, 1_000_000, 16)}        # total build rows, total probe rows, plan_target_keys


def join_bits(width):
    nb, _, target = JOIN_SHAPES[width]
    bits = 0
    while (1 << bits) < -(-nb // target):
        bits += 1
    return bits


@functools.lru_cache(maxsize=None)
def join_blocks(world, width):
    """(build keys, build values, probe keys per rank, build cuts): the ragged blocks of test_build_broadcast_form_matches_the_oracle -
    rank 0 holds no build rows, the last rank no probe rows; half of the probe rows hit, with repeats"""
    nb, npk, _ = JOIN_SHAPES[width]
    rng = np.random.default_rng([20261103, world, nb])
    bk = np.unique(rng.integers(0, 2**64, nb, dtype=_U))
    pk = np.concatenate([rng.choice(bk, npk // 2), rng.integers(0, 2**64, npk - npk // 2, dtype=_U)])
    rng.shuffle(pk)
    cutb = sorted(rng.integers(0, bk.size, world - 1).tolist()); cutb[0] = 0
    cutp = sorted(rng.integers(0, pk.size, world - 1).tolist()); cutp[-1] = pk.size
    return np.split(bk, cutb), np.split(vals_of(bk), cutb), np.split(pk, cutp)


@functools.lru_cache(maxsize=None)
def join_reference(world, width):
    """per rank: (count, the pairs (probe key, build value) of its probe rows, sorted) - oracle.np_join of ALL ranks' build rows with the
    rank's probe rows (in this form the pairs stay with the probe rows' rank); the counts add up to np_join of the whole relations"""
    from oracle import oracle as O
    bks, bvs, pks = join_blocks(world, width)
    bk, bv = np.concatenate(bks), np.concatenate(bvs)
    out = []
    for pk in pks:
        n, k, v = O.np_join(bk, bv, pk, return_arrays=True)
        out.append((n,) + O.canon_pairs(k, v))
    assert sum(r[0] for r in out) == O.np_join(bk, bv, np.concatenate(pks))
    return out


@pytest.mark.parametrize("width", JOIN_SHAPES)
def test_the_join_blocks_are_what_part_b_asks_for(width):
    bits = join_bits(width)
    assert (bits, WM.region_layout(bits, 0)[1]) == {"u32": (12, 4), "u16": (16, 2)}[width]
    for world in JOIN_WORLDS:
        bks, bvs, pks = join_blocks(world, width)
        assert bks[0].size == 0 and pks[-1].size == 0 and len(bks) == len(pks) == world
        allb = np.concatenate(bks)
        # no rung of the fallback ladder: every final partition far below the wide table (and the pair writer's 6000 keys)
        assert np.bincount(keymix.partition_of(allb, bits)).max() < 200
        ref = join_reference(world, width)
        assert sum(r[0] for r in ref) >= JOIN_SHAPES[width][1] // 2
        assert any(np.unique(r[1]).size < r[1].size for r in ref), "repeated probe keys"


# ---- filters: build sides, probe sides, the check -------------------------------------------------------------------------------------------
FILTER_BUILDS = ("random", "crafted", "dups")


def fa_partition(bits):
    """the 3000-key partition of `crafted` that the F-a twins probe"""
    return (1 << bits) // 3 + 1 + FILTER_SIZES.index(FA_PART_SIZE)


@functools.lru_cache(maxsize=None)
def filter_build(name, bits):
    nparts = 1 << bits
    rng = np.random.default_rng([20261104, bits])
    if name == "random":
        k = np.unique(rng.integers(0, 2**64, 50_000, dtype=_U))
        k = rng.permutation(k)
    elif name == "crafted":
        part = np.concatenate([np.repeat(at + np.arange(len(FILTER_SIZES)), FILTER_SIZES) for at in (0, nparts // 3 + 1, nparts - len(FILTER_SIZES))])
        k = keymix.craft_rows(bits, rng.permutation(part))
        assert np.unique(k).size == k.size
    elif name == "dups":
        k = rng.permutation(np.tile(filter_build("crafted", bits), 3))
    else:
        raise KeyError(name)
    k.setflags(write=False)
    return k


@functools.lru_cache(maxsize=8)
def model_filters(name, bits):
    f = WM.part_filters(filter_build(name, bits), bits)
    f.setflags(write=False)
    return f


def misses_like(keys, bits, seed, not_in):
    """one key per key of `keys`, in the same final partition, none of them in `not_in`"""
    m = keymix.craft_rows(bits, keymix.partition_of(keys, bits), seed=seed)
    assert not np.isin(m, not_in).any() and np.unique(m).size == m.size
    return m


def l1_bucket(keys, bits):
    return keymix.partition_of(keys, WM.fan_logs(bits)[0])


HOLES = {10: {"all": (3, 11, 19, 27), "some": (5, 21, 14, 30)},                                    # XCD 3 empty; XCD 5: e n e n; XCD 6: n e n e
         12: {"all": tuple(range(3, 64, 8)), "some": (5, 21, 29, 61)}}                             # XCD 5: e n e e n n n e
PROBE_CASES = ("all_hits", "no_hits", "hits_1to1", "hits_1to7", "fa_twins", "b255", "b256", "b257", "holes", "random")


def probe_bits(name):
    return {"holes": (10, 12), "fa_twins": (10, 17), "random": (12, 16, 17)}.get(name, (10,))


@functools.lru_cache(maxsize=None)
def probe_side(name, bits):
    """-> (build side's name, probe keys)
    all_hits / no_hits / hits_1to1 / hits_1to7: `crafted`'s keys, misses crafted into the same partitions, interleaved 1:1 and 1:7
    fa_twins: 20 000 misses of the 3000-key partition (false positives, and misses that fail exactly one bit position) + its keys
    b255 / b256 / b257: that many keys of ONE first-pass bucket, all admitted         random: 300 000 keys, a third of them hits of `random`
    holes: `random`'s keys and as many misses, without the first-pass buckets of HOLES: one XCD's list empty, empties at the start, in
    the middle and at the end of others"""
    rng = np.random.default_rng([20261105, bits, PROBE_CASES.index(name)])
    if name in ("all_hits", "no_hits", "hits_1to1", "hits_1to7"):
        build = filter_build("crafted", bits)
        if name == "all_hits":
            return "crafted", build
        k = 7 if name == "hits_1to7" else 1
        m = misses_like(np.repeat(build, k), bits, 7, build)
        if name == "no_hits":
            return "crafted", m
        return "crafted", np.concatenate([build[:, None], m.reshape(build.size, k)], axis=1).reshape(-1)
    if name == "fa_twins":
        build = filter_build("crafted", bits)
        m = keymix.craft_rows(bits, np.full(FA_MISSES, fa_partition(bits)), seed=11)
        assert not np.isin(m, build).any()
        mine = build[keymix.partition_of(build, bits) == fa_partition(bits)]
        return "crafted", rng.permutation(np.concatenate([m, mine]))
    if name in ("b255", "b256", "b257"):
        build = filter_build("crafted", bits)
        mine = build[keymix.partition_of(build, bits) == fa_partition(bits)]
        return "crafted", mine[: int(name[1:])]
    if name == "random":
        build = filter_build("random", bits)
        return "random", rng.permutation(np.concatenate([rng.choice(build, 100_000), rng.integers(0, 2**64, 200_000, dtype=_U)]))
    if name == "holes":
        build = filter_build("random", bits)
        p = np.concatenate([build, rng.integers(0, 2**64, build.size, dtype=_U)])
        gone = np.isin(l1_bucket(p, bits), HOLES[bits]["all"] + HOLES[bits]["some"])
        return "random", rng.permutation(p[~gone])
    raise KeyError(name)


def big_piece(cus, bits=10):
    """(build side's name, keys): more than twice the chunks one round of batches covers - 8 XCDs x (4 x CUs / 8) workgroups x 4 chunks
    - so that every workgroup takes a second batch: 12 x CUs x 1024 keys (3.1M at 256 compute units), hits in the first half of the
    rows, misses in the second (a bucket's later chunks hold its later rows)"""
    n = 12 * cus * 1024
    build = filter_build("random", bits)
    rng = np.random.default_rng([20261106, cus])
    return "random", np.concatenate([rng.choice(build, n // 2), rng.integers(0, 2**64, n - n // 2, dtype=_U)])


def check_precheck(keys, admitted, wire_keys, wire_bucket, wire_cnt, kept, used, bits, what=""):
    """A prechecked piece on the wire (keymix.unpack_wire of every owner's share, concatenated) against the model's verdict per input key:
    kept exact; per first-pass bucket the wire holds the admitted keys as an exact multiset, and extras only where a chunk kept no key -
    input keys of that bucket that the model rejects; a bucket with rows has a key on the wire; sum(used) * 256 >= kept."""
    fl0 = WM.fan_logs(bits)[0]
    F = 1 << fl0
    keys, admitted = np.asarray(keys, dtype=_U), np.asarray(admitted, dtype=bool)
    want_kept = int(admitted.sum())
    assert kept == want_kept, f"{what}: kept {kept}, the model admits {want_kept} of {keys.size}"
    assert sum(used) * CHUNK >= kept and sum(used) == wire_cnt.size and wire_keys.size == int(wire_cnt.sum())
    assert np.array_equal(l1_bucket(wire_keys, bits), wire_bucket), f"{what}: a key travels in a chunk of another bucket"
    kb = l1_bucket(keys, bits)
    n_b, adm_b, wire_b = (np.bincount(x, minlength=F) for x in (kb, kb[admitted], wire_bucket))
    a, w = np.sort(keys[admitted]), np.sort(wire_keys)
    au, ac = np.unique(a, return_counts=True)
    wu, wc = np.unique(w, return_counts=True)
    missing = np.setdiff1d(au, wu)
    assert missing.size == 0, f"{what}: {missing.size} admitted keys are not on the wire, the first {int(missing[0]):#018x} of bucket {int(l1_bucket(missing[:1], bits)[0])}"
    have = wc[np.searchsorted(wu, au)]
    assert np.all(have >= ac), f"{what}: {int((have < ac).sum())} admitted keys travel fewer times than they were sent"
    extra_u = np.setdiff1d(wu, au)
    rejected, rc = np.unique(keys[~admitted], return_counts=True)
    assert np.isin(extra_u, rejected).all(), f"{what}: keys on the wire that are no input keys"
    # an extra is a row of the input: it travels at most as often as it was sent
    assert np.all(wc[np.searchsorted(wu, extra_u)] <= rc[np.searchsorted(rejected, extra_u)]), f"{what}: a rejected key travels more often than it was sent"
    assert np.all(have == ac), f"{what}: {int((have > ac).sum())} admitted keys travel more often than they were sent (a chunk visited twice?)"
    extras_b = wire_b - adm_b
    assert np.all(extras_b >= 0)
    assert np.all(wire_b[n_b > 0] >= 1), f"{what}: a bucket with rows has no key on the wire"
    none = (n_b > 0) & (adm_b == 0)
    assert np.all((extras_b[none] >= 1) & (extras_b[none] <= n_b[none])), f"{what}: a bucket without admitted keys must travel with 1 .. n_b keys"
    # an extra is the first key of a level-1 chunk that kept nothing: at most one per chunk of the bucket, and a first pass of G workgroups
    # leaves a bucket of n_b keys in at most n_b / 256 + G + 1 chunks (one partial chunk per segment and bucket, G + 1 segments:
    # pass_groups, pinned above, and the pool size pass_prepare derives from it)
    G = min(512, max(1, keys.size // (F * 128)))
    over = np.flatnonzero(extras_b > np.minimum(n_b - adm_b, n_b // CHUNK + G + 1))
    assert over.size == 0, f"{what}: bucket {over[:1]} travels with {extras_b[over[:1]]} keys nobody admitted, more than it has chunks ({n_b[over[:1]]} rows, {G} workgroups)"
    return extras_b


def model_wire(keys, admitted, bits, defect=None, filters=None):
    """What a correct precheck (defect None) or a seeded one puts on the wire, as check_precheck's arguments - for the proofs only: the
    level-1 chunks are taken to be the bucket's keys in row order, 256 at a time."""
    fl0 = WM.fan_logs(bits)[0]
    keys, admitted = np.asarray(keys, dtype=_U), np.asarray(admitted, dtype=bool).copy()
    kb = l1_bucket(keys, bits)
    order = np.argsort(kb, kind="stable")
    k, a, b = keys[order], admitted[order], kb[order]
    first = np.flatnonzero(np.r_[True, b[1:] != b[:-1]])
    pos = np.arange(k.size) - np.repeat(first, np.diff(np.r_[first, k.size]))
    chunk_id = np.cumsum(np.r_[True, (b[1:] != b[:-1]) | (pos[1:] % CHUNK == 0)]) - 1
    chunk_bucket = b[np.flatnonzero(np.r_[True, chunk_id[1:] != chunk_id[:-1]])]
    keep_chunk = np.ones(chunk_bucket.size, dtype=bool)
    if defect == "F-d":
        a &= ~(pos % CHUNK >= 252)                               # lane 63 holds keys 252 .. 255 of a chunk
    elif defect == "F-e":
        # XCD x takes buckets x, x + 8, ...: everything behind the list's first empty bucket is skipped (kept as it was)
        n_b = np.bincount(kb, minlength=1 << fl0)
        for x in range(8):
            lst = np.arange(x, 1 << fl0, 8)
            e = np.flatnonzero(n_b[lst] == 0)
            if e.size:
                keep_chunk &= ~np.isin(chunk_bucket, lst[e[0]:])
    elif defect == "F-f":
        rounds = filters                                          # (here: chunks covered by the first round of batches, per XCD)
        for x in range(8):
            mine = np.flatnonzero(chunk_bucket % 8 == x)
            keep_chunk[mine[rounds:]] = False
    untouched = ~keep_chunk[chunk_id]
    nsurv = np.bincount(chunk_id[a & ~untouched], minlength=chunk_bucket.size)
    kept = int((a & ~untouched).sum())
    if defect == "F-g":
        travels = a | (nsurv[chunk_id] == 0)                     # the old count: the whole chunk travels
    else:
        firsts = np.r_[True, chunk_id[1:] != chunk_id[:-1]]
        travels = (a & ~untouched) | untouched | ((nsurv[chunk_id] == 0) & firsts)
    wk, wb = k[travels], b[travels]
    cnt = np.bincount(wb, minlength=1 << fl0)
    wire_cnt = np.concatenate([np.r_[np.full(c // CHUNK, CHUNK), [c % CHUNK] if c % CHUNK else []] for c in cnt if c]).astype(np.int64) if wk.size else np.zeros(0, np.int64)
    return wk, wb, wire_cnt, kept, [wire_cnt.size]


# which seeded defects each probe case is a test of (guards tests/test_wire_exact.py test_precheck_key_for_key[<name>-...]).  F-f and F-g
# belong to the big piece and its run against zero filters (test_the_second_batch_and_the_zero_filters guards
# test_every_workgroup_takes_a_second_batch), F-c to the exports (EXPORT_DETECTS), F-h to the sample.  The 17-bit cases are too large to
# prove here; the GPU file runs prove_fa on fa_twins-17 itself.
PROBE_DETECTS = {"all_hits": {"F-b", "F-d"}, "no_hits": {"F-b"}, "hits_1to1": {"F-b", "F-d"}, "hits_1to7": {"F-b", "F-d"},
                 "fa_twins": {"F-a", "F-b", "F-d"}, "b255": set(), "b256": {"F-d"}, "b257": {"F-d"}, "holes": {"F-e"}, "random": {"F-b"}}


@pytest.mark.parametrize("name,bits", [(n, b) for n in PROBE_CASES for b in probe_bits(n) if b < 17])
def test_every_probe_case_tells_its_defects_from_the_model(name, bits):
    bname, probe = probe_side(name, bits)
    build, f = filter_build(bname, bits), model_filters(bname, bits)
    ok = WM.admits(f, probe, bits)
    assert ok[np.isin(probe, build)].all(), "no false negatives"
    tag = f"test_precheck_key_for_key[{name}-{bits}]"
    good = model_wire(probe, ok, bits)
    check_precheck(probe, ok, *good, bits, "the model's own wire")
    detects = PROBE_DETECTS[name]
    if "F-a" in detects:
        prove_fa(probe, build, f, bits, tag)
    if "F-b" in detects:
        assert not np.array_equal(WM.admits(f, probe, bits, part_xor=1), ok), f"{tag}: defect F-b goes unnoticed"
    for d in ("F-d", "F-e", "F-g"):
        if d in detects:
            with pytest.raises(AssertionError):
                check_precheck(probe, ok, *model_wire(probe, ok, bits, d), bits)
    if name == "all_hits":
        assert ok.all() and np.bincount(l1_bucket(probe, bits)).max() >= 3000
    if name == "no_hits":
        assert not np.isin(probe, build).any() and (~ok).sum() > probe.size // 2
    if name in ("hits_1to1", "hits_1to7"):
        k = 1 if name == "hits_1to1" else 7
        assert probe.size == build.size * (k + 1) and np.array_equal(probe[::k + 1], build)
        assert np.array_equal(keymix.partition_of(probe, bits).reshape(-1, k + 1)[:, 1:], np.repeat(keymix.partition_of(build, bits)[:, None], k, axis=1))
    if name in ("b255", "b256", "b257"):
        assert probe.size == int(name[1:]) and ok.all() and np.unique(l1_bucket(probe, bits)).size == 1
    if name == "holes":
        n_b = np.bincount(l1_bucket(probe, bits), minlength=1 << WM.fan_logs(bits)[0])
        H = HOLES[bits]
        assert not n_b[list(H["all"] + H["some"])].any() and np.count_nonzero(n_b == 0) == len(H["all"] + H["some"])
        assert sorted(H["all"]) == list(range(3, n_b.size, 8)), "one XCD's list is empty altogether"
        for x in sorted({b % 8 for b in H["some"]}):
            lst = n_b[x::8]
            assert lst.any() and not lst.all()
        shape = ["".join("e" if c == 0 else "n" for c in n_b[x::8]) for x in sorted({b % 8 for b in H["some"]})]
        assert shape == {10: ["enen", "nene"], 12: ["eneennne"]}[bits], shape
        # behind every empty bucket of those lists there are chunks with admitted keys: skipping them changes kept
        assert model_wire(probe, ok, bits, "F-e")[3] < good[3]


def prove_fa(probe, build, f, bits, tag):
    """F-a: at least 32 false positives, and per bit position at least 32 misses that fail exactly that position"""
    ok = WM.admits(f, probe, bits)
    miss = ~np.isin(probe, build)
    assert int((ok & miss).sum()) >= 32, f"{tag}: only {int((ok & miss).sum())} false positives"
    for i, s in enumerate(WM.PF_SHIFTS):
        others = tuple(x for x in WM.PF_SHIFTS if x != s)
        loose = WM.admits(f, probe, bits, shifts=others)
        only = loose & ~ok & miss
        assert int(only.sum()) >= 32, f"{tag}: defect F-a, position {i}: only {int(only.sum())} misses fail exactly that position"


def test_the_twins_partition_has_false_positives_and_small_partitions_have_none():
    """a 3000-key partition probed with 20 000 misses of its own: a few hundred false positives, and over a thousand misses that fail
    exactly one bit position - what F-a needs; partitions of about 50 keys have next to none: nothing to rely on there"""
    bits = 10
    bname, probe = probe_side("fa_twins", bits)
    build, f = filter_build(bname, bits), model_filters(bname, bits)
    ok, miss = WM.admits(f, probe, bits), ~np.isin(probe, build)
    assert miss.sum() == FA_MISSES and np.unique(keymix.partition_of(probe, bits)).tolist() == [fa_partition(bits)]
    one = sum(int((WM.admits(f, probe, bits, shifts=tuple(x for x in WM.PF_SHIFTS if x != s)) & ~ok & miss).sum()) for s in WM.PF_SHIFTS)
    assert 100 <= int((ok & miss).sum()) <= 400 and 1000 <= one <= 2500, (int((ok & miss).sum()), one)
    assert WM.admits(model_filters("random", bits), np.random.default_rng(3).integers(0, 2**64, 20_000, dtype=_U), bits).sum() < 8


# which seeded defects each export case is a test of (guards tests/test_wire_exact.py test_exported_filters[...-<name>])
EXPORT_DETECTS = {"random": {"F-a", "F-b"}, "crafted": {"F-a", "F-b", "F-c"}, "dups": {"F-a", "F-b", "F-c"}}


@pytest.mark.parametrize("bits", [10, 12, 16])
@pytest.mark.parametrize("name", FILTER_BUILDS)
def test_every_export_case_tells_its_defects_from_the_model(name, bits):
    build, f = filter_build(name, bits), model_filters(name, bits)
    assert WM.admits(f, build, bits).all()
    sizes = np.bincount(keymix.partition_of(build, bits), minlength=1 << bits)
    assert not f[sizes == 0].any() and f[sizes > 0].any(axis=1).all()
    for s in range(4):                                           # a bit position read one bit higher changes a word
        shifts = tuple(x + (i == s) for i, x in enumerate(WM.PF_SHIFTS))
        assert not np.array_equal(WM.part_filters(build, bits, shifts), f), f"test_exported_filters[{name}]: a moved position {s} goes unnoticed"
    # F-b for an export: the filters of partitions p and p ^ 1 differ wherever one of them holds a key
    assert not np.array_equal(f.reshape(-1, 2, WM.PF_BLOCKS)[:, ::-1].reshape(f.shape), f)
    if "F-c" in EXPORT_DETECTS[name]:
        # nearly every key sets a bit no other key of its partition sets: leaving out keys of it - a last chunk, what lies beyond lane 63
        # of a chunk - changes a word, whichever keys a chunk happened to hold
        u = np.unique(build)
        part = keymix.partition_of(u, bits)
        block, _ = WM.pf_bits(keymix.mix(u))
        w2 = keymix.mix(u) & _U(0xFFFFFFFF)
        ids = np.stack([(part * WM.PF_BLOCKS + block) * 64 + ((w2 >> _U(s)) & _U(63)).astype(np.int64) for s in WM.PF_SHIFTS], axis=1)
        v, c = np.unique(ids, return_counts=True)
        own = (c[np.searchsorted(v, ids)] == 1).any(axis=1)
        usizes = np.bincount(part, minlength=1 << bits)
        lacking = np.bincount(part[~own], minlength=1 << bits)
        # at most 4 keys of a partition of up to 700 keys (and fewer than 70 of the 3000) lack a bit of their own: what lies beyond lane
        # 63 of any chunk of 69 keys or more, and any last chunk of 5 keys or more, shows
        assert lacking[usizes <= 700].max() <= 4 and lacking.max() < 70, lacking[lacking > 0]
        assert (usizes == 257).sum() == 3 and (usizes == 700).sum() == 3 and (usizes == 3000).sum() == 3, "one chunk, a chunk boundary, several chunks"
    for world in (1, 3, 8):                                      # the owners' ranges tile the table; uneven at 3
        fl0 = WM.fan_logs(bits)[0]
        r = [WM.filter_range(bits, fl0, world, o) for o in range(world)]
        assert r[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(r, r[1:])) and r[-1][0] + r[-1][1] == 1 << bits
        owner = WM.owner_of_bucket(np.arange(1 << fl0), fl0, world)
        assert [int((owner == o).sum()) << (bits - fl0) for o in range(world)] == [x[1] for x in r]
        if world == 3:
            assert len({x[1] for x in r}) == 2


def test_the_second_batch_and_the_zero_filters():
    """F-f and F-g on a small stand-in for big_piece (16 compute units): one round of batches covers 4 x CUs x 4 chunks; the piece has
    more than twice that in every XCD's list, and a precheck that stops after the first round is told apart by kept"""
    cus, bits = 16, 10
    bname, probe = big_piece(cus, bits)
    ok = WM.admits(model_filters(bname, bits), probe, bits)
    assert probe.size == 12 * cus * 1024 and ok[: probe.size // 2].all() and ok[probe.size // 2:].sum() < 100
    per_xcd_round = (4 * cus // 8) * 4
    chunks_x = [int(-(-np.bincount(l1_bucket(probe, bits), minlength=32)[x::8] // CHUNK).sum()) for x in range(8)]
    assert min(chunks_x) > 2 * per_xcd_round, (chunks_x, per_xcd_round)
    good = model_wire(probe, ok, bits)
    check_precheck(probe, ok, *good, bits)
    assert model_wire(probe, ok, bits, "F-f", per_xcd_round)[3] < good[3]
    zero = np.zeros(probe.size, dtype=bool)
    z = model_wire(probe, zero, bits)
    extras = check_precheck(probe, zero, *z, bits)
    assert z[3] == 0 and np.array_equal(extras, -(-np.bincount(l1_bucket(probe, bits), minlength=32) // CHUNK)), "every chunk travels with one key"
    with pytest.raises(AssertionError):
        check_precheck(probe, zero, *model_wire(probe, zero, bits, "F-g"), bits)


# ---- part E: the sample ----------------------------------------------------------------------------------------------------------------------
SAMPLE_STRIDES, SAMPLE_N = (1, 7, 4099), (0, 1, 255, 256, 257, 100_003)


@functools.lru_cache(maxsize=None)
def sample_keys(bits=10):
    """(build side's name, the 100 003 keys a sample must test - every other one a hit).  What lies between them at a stride > 1 is the GPU
    file's business: random keys, misses all but a handful"""
    build = filter_build("random", bits)
    rng = np.random.default_rng(20261107)
    k = rng.integers(0, 2**64, max(SAMPLE_N), dtype=_U)
    k[::2] = rng.choice(build, k[::2].size)
    return "random", k


def test_the_sample_tells_a_kernel_that_ignores_stride():
    bname, k = sample_keys()
    ok = WM.admits(model_filters(bname, 10), k, 10)
    for n in SAMPLE_N[1:]:
        want = int(ok[:n].sum())
        assert want >= (n + 1) // 2
        # F-h: at a stride > 1 the keys between the sampled ones are random misses - reading raw[0:n] counts about 1 / stride of `want`
        for stride in SAMPLE_STRIDES[1:]:
            assert -(-n // stride) // 2 + 8 < want or n < 16
