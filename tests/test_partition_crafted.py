"""The radix partition pass (csrc/fj_partition.hip fj_partition_kernel) on keys crafted per tile and bucket.

The mixer is a bijection (tests/keymix.py inverts it), so keymix.craft_rows() gives every ROW any radix bucket.  Where one workgroup
walks all tiles in order - always below 256 * F rows, see pass_groups - the test therefore decides what every bucket receives in every
tile, and by lane (row (i * 1024 + tid) * 2 + j of a tile is register slot 2 i + j of thread tid) which lanes of a wave share a digit.

TWO LAYERS, kept apart:

  THE REFERENCE is independent of the kernel's structure: per bucket (keymix.partition_of on the input: the mixer restated in NumPy,
  pinned to the library by tests/test_abi.py) the sorted multiset of (raw key, row index).  With values (vals = arange(n)) every
  bucket's sorted (key, val) arrays must equal it exactly and keys[val] == key; keys-only every bucket's sorted keys must.  Every row
  is compared, integers only, no tolerance.  The pass runs through fj_debug_partition of the lab library, which already fails on a
  device error word (pool overflow: FJ_ERR_POOL), a chunk listed under the wrong bucket and a chunk whose count differs between
  directory and list - so the worst-case shapes also test pass_prepare's pool bound.

  THE COVERAGE MODEL (simulate(), class Model) restates the kernel's per-(workgroup, bucket) bookkeeping - st_left, st_fill, chunks opened per tile,
  ids left in the run, units asked for at a flush, the slab's remainder, the hot bucket of every wave - and is used for COVERAGE
  ASSERTIONS ONLY, never as the expected output.  Every case is named after one condition and asserts on the model that its input
  reaches it (the event carries pass, workgroup, tile and bucket or wave); a script that no longer reaches its condition because a
  constant changed fails instead of passing vacuously.  test_geometry_* pins the constants and formulas the scripts are cut to.

What the model may assume.  The keys of one bucket keep no defined order inside a tile (LDS atomics give the ranks), so WHICH keys sit
in which chunk of a parent bucket is not defined; the model uses row order.  Every condition asserted on a second or third pass is
independent of that order by construction of its script: the per-tile counts are (a parent of at most one tile; parents all of whose
keys share the child; chunks of one key), or only the chunk sizes matter.  Where the first pass runs several workgroups the order of
their spans in a bucket's list is not defined either (one global atomic per span): such a condition is asserted for both orders.

At 5 bits a flat pass has one workgroup only below 8192 rows, so the multi-tile scripts there run as G = 3 (one_bucket) or are left
to 8 and 9 bits; flush_needs_slab and multi_slab need runs of ids and 512 buckets to use up a slab below the single-workgroup bound
(a slab is 1024 single ids: more chunks than 65 535 rows fill), so they exist at 9 bits only."""
import ctypes
import functools
import os

import numpy as np
import pytest

import keymix
from conftest import ROOT

CHUNK, NT, RUN_LOG, SLAB, MAX_FAN_LOG, NWAVES = 256, 1024, 2, 1024, 9, 16


# ---- the constants and formulas the scripts are cut to, read from the sources ---------------------------------------------------
def _source(name):
    with open(os.path.join(ROOT, "flash_hash_join_amd", "csrc", name)) as f:
        return f.read()


def _says(text, fragment, what):
    assert fragment in text, f"{what}: the sources no longer say `{fragment}` - tests/test_partition_crafted.py scripts its tiles for another kernel"


def test_geometry_constants_pinned_to_the_sources():
    c, k, p, h = _source("fj_common.h"), _source("fj_partition.hip"), _source("fj_plan.hip"), _source("fj_host.h")
    _says(c, "#define FJ_CHUNK_LOG 8", "keys per chunk")
    _says(c, "#define FJ_RUN_LOG 2", "ids per run")
    _says(c, "#define FJ_MAX_FAN_LOG 9", "widest pass")
    _says(c, "#define FJ_DIR_CNT_BITS 9", "directory word")
    _says(c, "static inline unsigned fj_slab_for(unsigned appends) { return appends > 1u ? 256u : 1024u; }", "slab of a single append")
    assert (CHUNK, RUN_LOG, MAX_FAN_LOG, SLAB) == (1 << 8, 2, 9, 1024)
    # tile sizes: keys-only 1024 threads x 8 keys, with values 1024 x 4 - for every fan-out
    _says(k, "u32 fj_partition_tile_chunks(u32 fan_log, bool vals) { (void)fan_log; return vals ? 16u : 32u; }", "tile size")
    _says(k, "if (vals) return line_log == 3 ? launch_part2<1024, 4, true>(a, 3, grid, s) : hipErrorInvalidValue;", "512 buckets with values")
    _says(k, "return launch_part2<1024, 8, false>(a, line_log, grid, s);", "512 buckets, keys only")
    _says(k, "return launch_part2<1024, 4, true>(a, line_log, grid, s);", "<= 256 buckets with values")
    _says(k, "return launch_part2<1024, 8, false>(a, line_log, grid < 256 ? grid : 256, s);", "<= 256 buckets, keys only")
    _says(k, "constexpr u32 T = NT * KPT, LINE = 1u << LINE_LOG, TC = T / FJ_CHUNK, NW = NT / 64", "tile geometry")
    # lines: 16 keys, 8 where values go through a 512-bucket pass
    _says(p, "const int line_log = (it.has_vals && it.F > 256) ? 3 : 4;", "line size")
    # single ids for flat passes of <= 256 buckets, runs everywhere else
    _says(p, "cs.run_log = (!it.have_prev && it.i == 0 && F <= 256) ? 0u : (u32)FJ_RUN_LOG;", "runs")
    _says(k, "if constexpr (FLAT) { if (a.run_log == 0) return launch_part0<NT, KPT, LINE_LOG, HAS_VALS, FLAT, PROBE_SIDE, 0>(a, grid, s); }", "runs")
    # workgroups and their share of the tiles
    _says(p, "const u64 g64 = std::min<u64>(chunks / tile_chunks, rows / ((u64)F * 128));", "workgroups per launch")
    _says(p, "return (u32)std::min<u64>(512, std::max<u64>(1, g64));", "workgroups per launch")
    _says(p, "it.Gmax = pass_groups(it.lbound, it.n, it.tile_chunks, it.F);", "workgroups per launch")
    _says(p, "G = std::min(G, pass_groups((n + FJ_CHUNK - 1) / FJ_CHUNK, n, it.tile_chunks, it.F));", "workgroups of a flat launch")
    _says(p, "it.lbound = (n + FJ_CHUNK - 1) / FJ_CHUNK;", "chunk bound of the flat input")
    _says(p, "it.lbound = it.n / FJ_CHUNK + 1 + (u64)(it.Gmax + it.parents) * it.F * it.appends;", "chunk bound of a level")
    _says(h, "u32 parents = 1;", "parents of the first pass")
    _says(k, "const u32 t0 = (u32)(((u64)g * ntiles) / G);", "tile share")
    _says(k, "const u32 nmine = (u32)(((u64)(g + 1) * ntiles) / G) - t0;", "tile share")
    _says(k, "const u32 ntiles = FLAT ? (Lc + TC - 1) / TC : *a.in_ntiles;", "tiles of a flat input")
    # plans
    _says(p, "int plan_npass(int bits) { return bits <= FJ_MAX_FAN_LOG ? (bits > 0 ? 1 : 0) : (bits <= 2 * FJ_MAX_FAN_LOG ? 2 : (bits + FJ_MAX_FAN_LOG - 1) / FJ_MAX_FAN_LOG); }", "passes of a plan")
    _says(p, "p.fan_log[i] = p.bits / p.npass + ((extra_first ? i < rem : i >= p.npass - rem) ? 1 : 0);", "bits of a pass")
    _says(p, "plan_passes(plan, true);", "the diagnostic's plan")
    # row -> lane, chunk-list tiles
    _says(k, "base = (u64)(t0 + tt) * T + ((u32)i * NT + tid) * 2;", "row to lane")
    _says(k, "const u32 kidx = ((u32)i * NT + tid) * 2;", "chunk-list key to lane")
    _says(k, "nv = off + 1 < cnt ? 2u : (off < cnt ? 1u : 0u);", "pair loads of a chunk")
    _says(k, "tiles[t] = make_uint4(pos, rem < step ? rem : step, lo, 0);", "tile table")
    # bookkeeping the model restates
    _says(k, "const u32 avg2 = (2u * T / LINE) >> a.fan_log;", "descriptor threshold")
    _says(k, "const u32 own_lines = avg2 > 4u ? avg2 : 4u;", "descriptor threshold")
    _says(k, "u64 big = __ballot(nl > own_lines);", "descriptor threshold")
    _says(k, "nf = tot & ~(LINE - 1);", "whole lines")
    _says(k, "km = nf ? ((st_fill + nf - 1) >> FJ_CHUNK_LOG) : 0;", "chunks opened per tile")
    _says(k, "kr = RUNS ? (km > rl ? (km - rl + RU - 1u) >> RL : 0u) : km;", "units per tile")
    _says(k, "(RUNS && c0 != FJ_DIR_INVALID) ? (RU - 1u) - ((c0 - rot(b)) & (RU - 1u)) : 0u;", "ids left in a run")
    _says(k, "const u32 su = a.slab >> RL, k = (need - misc[M_SLAB_REM] + su - 1) / su;", "slabs")
    _says(k, "if (need > misc[M_SLAB_REM]) take_slabs(need);", "slabs taken by a tile")
    _says(k, "if (tid == 0 && misc[M_FLUSH] > misc[M_SLAB_REM]) take_slabs(misc[M_FLUSH]);", "slabs taken by a flush")
    _says(k, "if (tid < F && st_left > 0 && st_fill == FJ_CHUNK && !run_left(st_cur, tid)) fresh = atomicAdd(&misc[M_FLUSH], 1u);", "fresh unit at a flush")
    _says(k, "if (pend_nf == 0) {                                   // nothing was written: append the new keys", "carry")
    # the hot test
    _says(k, "const u32 bl = br[KPT - 1] >> 16;", "hot test: the last slot")
    _says(k, "const u32 cand = (u32)__builtin_amdgcn_readfirstlane((int)bl);", "hot test: lane 0")
    _says(k, "if (__popcll(__ballot(bl == cand)) >= 8) hotb = cand;", "hot test: 8 lanes")
    _says(k, "if (seen < 8) hotb = 0xFFFFFFFFu;                // cooled down", "cool-down")
    _says(k, "if (n >= 2) {", "hot ranking: one hot lane takes the plain atomic")
    _says(k, "const u32 b = (valid & (1u << i)) ? ((FJ_HW1(k[i]) >> sh32) & FM) : F;", "dummy bucket of invalid lanes")


# ---- the plan and launch geometry, restated ---------------------------------------------------------------------------------
def plan_fans(bits):
    npass = 1 if bits <= MAX_FAN_LOG else (2 if bits <= 2 * MAX_FAN_LOG else -(-bits // MAX_FAN_LOG))
    rem = bits % npass
    return [bits // npass + (1 if i < rem else 0) for i in range(npass)]


def pass_groups(chunks, rows, tile_chunks, F):
    return min(512, max(1, min(chunks // tile_chunks, rows // (F * 128))))


class Geom:
    """one pass: fan-out, tile, line, run length, slab units, descriptor threshold"""
    def __init__(self, fan_log, vals, first):
        self.fan_log, self.vals, self.first, self.F = fan_log, vals, first, 1 << fan_log
        self.KPT = 4 if vals else 8
        self.T = NT * self.KPT
        self.TC = self.T // CHUNK
        self.LINE = 8 if (vals and self.F > 256) else 16
        self.RL = 0 if (first and self.F <= 256) else RUN_LOG
        self.RU = 1 << self.RL
        self.su = SLAB >> self.RL
        self.own_lines = max(4, (2 * self.T // self.LINE) >> fan_log)
        self.grid_cap = 256 if (not vals and self.F <= 256) else 512

    def flat_groups(self, n):
        return min(self.grid_cap, pass_groups(-(-n // CHUNK), n, self.TC, self.F))


def test_geometry_formulas():
    assert [plan_fans(b) for b in (5, 8, 9, 10, 17, 18, 19, 20)] == [[5], [8], [9], [5, 5], [9, 8], [9, 9], [7, 6, 6], [7, 7, 6]]
    for vals in (False, True):
        g8, g9 = Geom(8, vals, True), Geom(9, vals, True)
        assert g8.flat_groups(65535) == 1 and g8.flat_groups(65536) == 2          # one workgroup whenever n < 256 F
        assert g9.flat_groups(131071) == 1 and g9.flat_groups(131072) == 2
        assert all(g.flat_groups(n) == 1 for g in (g8, g9) for n in (1, 255, 4096, 12289, 24577, 57344))
        assert (g8.RL, g9.RL, Geom(8, vals, False).RL, Geom(5, vals, False).RL) == (0, 2, 2, 2)
        assert (g8.T, g8.TC) == ((4096, 16) if vals else (8192, 32))
        assert (g8.LINE, g9.LINE) == (16, 8 if vals else 16)
    assert Geom(9, True, True).own_lines == 4 and Geom(9, False, True).own_lines == 4 and Geom(5, True, True).own_lines == 16
    assert Geom(8, False, True).own_lines == 4 and Geom(5, False, True).own_lines == 32
    # 18 bits, 131 071 rows: both passes run one workgroup (the second: min(1536 / tile_chunks, 131071 / 65536))
    n = 131071
    lbound = n // CHUNK + 1 + (1 + 1) * 512
    assert lbound == 1536 and pass_groups(lbound, n, 16, 512) == 1 and pass_groups(lbound, n, 32, 512) == 1


# ---- the coverage model ---------------------------------------------------------------------------------------------------------
class Events:
    def __init__(self):
        self.n, self.first, self.max, self.all = {}, {}, {}, {}

    def hit(self, name, where):
        self.n[name] = self.n.get(name, 0) + 1
        self.first.setdefault(name, where)
        if self.n[name] <= 4096:
            self.all.setdefault(name, []).append(where)

    def top(self, name, value, where):
        if value > self.max.get(name, (-1, None))[0]:
            self.max[name] = (value, where)

    def count(self, name):
        return self.n.get(name, 0)

    def need(self, name, at_least=1):
        assert self.count(name) >= at_least, f"the script does not reach `{name}` ({self.count(name)} < {at_least}); reached: {sorted(self.n)}"
        return self.first[name]


def to_lanes(tile, KPT):
    """tile offsets -> [thread, register slot]: offset (i * 1024 + tid) * 2 + j is slot 2 i + j of thread tid"""
    return tile.reshape(KPT // 2, NT, 2).transpose(1, 0, 2).reshape(NT, KPT)


def from_lanes(lanes, KPT):
    return lanes.reshape(NT, KPT // 2, 2).transpose(1, 0, 2).reshape(NT * KPT)


def flat_tiles(n, P):
    ntiles = -(-(-(-n // CHUNK)) // P.TC)
    out = []
    for t in range(ntiles):
        rows = np.arange(t * P.T, (t + 1) * P.T, dtype=np.int64)
        rows[rows >= n] = -1
        out.append((0, rows, P.TC))
    return out


def list_tiles(level, P, pass_no, ev, descending=False):
    """tiles of a chunk-list pass: per parent bucket (ascending) its chunk list - the spans of the producing segments, each cut into
    chunks of 256 with a partial last one - cut into tiles of tile_chunks chunks"""
    out = []
    for parent in sorted(level):
        segs = level[parent][::-1] if descending else level[parent]
        chunks = [s[c:c + CHUNK] for s in segs for c in range(0, s.size, CHUNK)]
        for i in range(0, len(chunks), P.TC):
            mine = chunks[i:i + P.TC]
            rows = np.full(P.T, -1, dtype=np.int64)
            for j, ch in enumerate(mine):
                rows[j * CHUNK:j * CHUNK + ch.size] = ch
                if (ch.size & 1) and j + 1 < len(mine):
                    ev.hit("odd_chunk_mid_tile", (pass_no, len(out), j, ch.size))     # a pair load with one valid key, chunks behind it
                if ch.size == 1:
                    ev.hit("one_key_chunk", (pass_no, len(out), j))
            out.append((parent, rows, len(mine)))
    return out


def simulate(P, tiles, G, dig_of_row, pass_no, ev):
    """one pass: the bookkeeping of every workgroup over its share of the tiles.  Returns (output level: out bucket -> spans of row
    ids in segment order, chunks listed)."""
    F, LINE, RUNS, RU, RL = P.F, P.LINE, P.RL > 0, P.RU, P.RL
    ntiles, out, listed = len(tiles), {}, 0
    ev.top("groups_with_tiles", sum(1 for g in range(G) if (g + 1) * ntiles // G > g * ntiles // G), (pass_no,))
    for g in range(G):
        t0 = g * ntiles // G
        nmine = (g + 1) * ntiles // G - t0
        if nmine == 0:
            continue
        z = lambda: np.zeros(F, dtype=np.int64)
        st = dict(left=z(), fill=np.full(F, CHUNK, dtype=np.int64), nch=z(), rl=z(), pend_nf=z(), pend_cnt=z(), streak=z())
        slab = dict(rem=0)
        hot = np.full(NWAVES, -1, dtype=np.int64)
        parts, cur_parent, flushes_in_loop, prev_full = [], None, 0, False

        def take(need, name, where):
            k = -(-(need - slab["rem"]) // P.su)
            ev.hit(name, where + (need, slab["rem"], k))
            if k >= 2:
                ev.hit(name + "_several_slabs", where + (need, k))
            return k * P.su

        def commit(need, new_units):
            slab["rem"] = slab["rem"] - need if need <= slab["rem"] else new_units - (need - slab["rem"])

        def carry(t):
            app = (st["pend_nf"] == 0) & (st["pend_cnt"] > 0)
            st["streak"] = np.where(st["pend_nf"] > 0, 0, st["streak"] + app)
            if app.any():
                b = int(np.argmax(st["streak"]))
                ev.top("append_streak", int(st["streak"][b]), (pass_no, g, t, b))
            st["left"] = st["left"] + st["pend_cnt"] - st["pend_nf"]
            st["pend_nf"], st["pend_cnt"] = z(), z()

        def flush(parent, t):
            nonlocal listed
            left, fill, nch, rl = st["left"], st["fill"], st["nch"], st["rl"]
            where = (pass_no, g, t)
            fresh = (left > 0) & (fill == CHUNK) & (rl == 0)
            need = int(fresh.sum())
            new_units = take(need, "take_flush", where) if need > slab["rem"] else 0
            for name, m in (("flush_full_no_partial", (left == 0) & (fill == CHUNK) & (nch > 0)),
                            ("flush_next_id_of_run", (left > 0) & (fill == CHUNK) & (rl > 0)),
                            ("flush_fresh_run_exhausted" if RUNS else "flush_fresh_single_id", fresh & (nch > 0)),
                            ("flush_fresh_first_chunk", fresh & (nch == 0)),
                            ("flush_into_open_chunk", (left > 0) & (fill < CHUNK))):
                for b in np.flatnonzero(m)[:8]:
                    ev.hit(name, where + (int(b), int(nch[b])))
            nseg = nch + ((left > 0) & (fill == CHUNK))
            commit(need, new_units)
            d = np.concatenate([p[0] for p in parts]) if parts else np.zeros(0, dtype=np.int64)
            r = np.concatenate([p[1] for p in parts]) if parts else np.zeros(0, dtype=np.int64)
            o = np.argsort(d, kind="stable")
            d, r = d[o], r[o]
            tot = np.bincount(d, minlength=F)
            assert np.array_equal(nseg, -(-tot // CHUNK)), "model: the chunks of a segment are not ceil(keys / 256)"
            assert np.array_equal((fill % CHUNK + left)[tot > 0] % CHUNK, (tot % CHUNK)[tot > 0]), "model: the last chunk's count"
            listed += int(nseg.sum())
            edges = np.r_[0, np.cumsum(tot)]
            for b in np.flatnonzero(tot):
                out.setdefault(parent * F + int(b), []).append(r[edges[b]:edges[b + 1]])
            for b in np.flatnonzero(tot == 1)[:4]:
                ev.hit("segment_bucket_of_one_key", where + (int(b),))
            ev.n["segment_buckets_of_one_key"] = ev.n.get("segment_buckets_of_one_key", 0) + int((tot == 1).sum())
            parts.clear()
            st.update(left=z(), fill=np.full(F, CHUNK, dtype=np.int64), nch=z(), rl=z(), streak=z())

        for t in range(nmine):
            parent, rows, nchunks = tiles[t0 + t]
            where = (pass_no, g, t)
            carry(t)
            if parent != cur_parent:
                if cur_parent is not None:
                    flush(cur_parent, t)
                    flushes_in_loop += 1
                    if prev_full:
                        ev.hit("parent_change_on_tile_boundary", where + (cur_parent, parent))
                cur_parent = parent
            prev_full = nchunks == P.TC and bool((rows[(P.TC - 1) * CHUNK:] >= 0).all())
            valid = rows >= 0
            d = np.where(valid, dig_of_row[np.where(valid, rows, 0)], F)
            cnt = np.bincount(d, minlength=F + 1)[:F]
            parts.append((d[valid], rows[valid]))
            # ---- ranking: the hot bucket of every wave
            lanes = to_lanes(d, P.KPT).reshape(NWAVES, 64, P.KPT)
            for w in range(NWAVES):
                if hot[w] < 0:
                    last = lanes[w, :, P.KPT - 1]
                    c = int((last == last[0]).sum())
                    if c in (7, 8):
                        ev.hit(f"detect_{c}_lanes", where + (w, int(last[0])))
                    if c >= 8:
                        hot[w] = last[0]
                        ev.hit("hot_on", where + (w, int(last[0]), c))
                        if last[0] == F:
                            ev.hit("hot_on_dummy_bucket", where + (w,))
                else:
                    per = (lanes[w] == hot[w]).sum(axis=0)
                    ev.hit("hot_active", where + (w, int(hot[w])))
                    if (per == 1).any():
                        ev.hit("hot_single_lane", where + (w, int(hot[w])))
                    if ((per >= 2) & (per < 64)).any():
                        ev.hit("hot_mixed_lanes", where + (w, int(hot[w])))
                    if (per == 64).any():
                        ev.hit("hot_all_lanes", where + (w, int(hot[w])))
                    if per.sum() < 8:
                        ev.hit("hot_cooled", where + (w, int(hot[w])))
                        hot[w] = -1
            # ---- the scan's per-bucket quantities
            left, fill, rl = st["left"], st["fill"], st["rl"]
            tot = left + cnt
            nf = tot & ~(LINE - 1)
            km = np.where(nf > 0, (fill + nf - 1) >> 8, 0)
            kr = np.where(km > rl, (km - rl + RU - 1) >> RL, 0) if RUNS else km
            need = int(kr.sum())
            new_units = take(need, "take_tile", where) if need > slab["rem"] else 0
            commit(need, new_units)
            nl = nf // LINE
            big = nl > P.own_lines
            for b in np.flatnonzero(big)[:8]:
                ev.hit("descriptors_by_wave", where + (int(b), int(b) // 64))
                ev.hit(f"descriptors_by_wave_{'0' if b < 64 else 'later'}", where + (int(b), int(b) // 64))
            if big.any() and np.bincount(np.flatnonzero(big) // 64).max() >= 2:
                ev.hit("two_big_in_one_wave", where + tuple(int(b) for b in np.flatnonzero(big)[:2]))
            if km.max() == P.TC:
                ev.hit("opened_tile_chunks", where + (int(np.argmax(km)),))
            strad = (nf > 0) & (left > 0)
            for b in np.flatnonzero(strad)[:4]:
                ev.hit("line_straddles_carry", where + (int(b), int(left[b])))
            ev.n["straddles"] = ev.n.get("straddles", 0) + int(strad.sum())
            for b in np.flatnonzero(strad & (st["streak"] >= 2))[:4]:
                ev.hit("straddle_after_appends", where + (int(b), int(st["streak"][b]), int(left[b])))
            if strad.any():
                ev.top("straddle_from_carry", int(left[strad].max()), where + (int(np.argmax(np.where(strad, left, -1))),))
                if (left[strad] == LINE - 1).all() and strad.all():
                    ev.hit("every_bucket_takes_line_minus_1_from_carry", where)
            if ((tot - nf) == 0).all():
                ev.hit("tile_carries_nothing", where)
            elif ((tot - nf) == LINE - 1).all():
                ev.hit("tile_carries_line_minus_1_everywhere", where)
            else:
                ev.hit("tile_carries_something", where)
            if RUNS:
                q = km - rl - 1
                st["rl"] = np.where(km == 0, rl, np.where(km <= rl, rl - km, RU - 1 - (q & (RU - 1))))
            st["fill"] = fill + nf - (km << 8)
            st["nch"] = st["nch"] + km
            st["pend_cnt"], st["pend_nf"] = cnt, nf
        carry(nmine)
        flush(cur_parent, nmine)
        if nmine >= 3 and flushes_in_loop == nmine - 1:
            ev.hit("flush_in_every_iteration", (pass_no, g, nmine))
    return out, listed


class Model:
    """the plan's passes over n rows whose final bucket is bucket_of_row"""
    def __init__(self, bits, vals, bucket_of_row, descending=False):
        b = np.asarray(bucket_of_row, dtype=np.int64)
        self.bits, self.vals, self.n, self.ev, self.passes, self.rows = bits, vals, b.size, Events(), [], b
        fans, used = plan_fans(bits), bits
        n, level, lbound, parents = b.size, None, -(-b.size // CHUNK), 1
        for i, f in enumerate(fans):
            used -= f
            P = Geom(f, vals, i == 0)
            dig = (b >> used) & (P.F - 1)
            if i == 0:
                G, tiles = P.flat_groups(n), flat_tiles(n, P)
            else:
                G, tiles = min(P.grid_cap, pass_groups(lbound, n, P.TC, P.F)), list_tiles(level, P, i, self.ev, descending)
            level, listed = simulate(P, tiles, G, dig, i, self.ev)
            self.passes.append(dict(P=P, G=G, ntiles=len(tiles), listed=listed))
            lbound = n // CHUNK + 1 + (G + parents) * P.F
            parents *= P.F
        self.level, self.listed = level, self.passes[-1]["listed"]
        got = np.sort(np.concatenate([s for segs in level.values() for s in segs])) if level else np.zeros(0, dtype=np.int64)
        assert np.array_equal(got, np.arange(n)), "model: rows lost"
        assert all((b[s] == ob).all() for ob, segs in level.items() for s in segs), "model: a row in the wrong bucket"

    def level_spans(self, d):
        """sizes of the spans the first pass's workgroups give its bucket d (what the second pass reads), from the tile share alone"""
        P, G, ntiles = self.passes[0]["P"], self.passes[0]["G"], self.passes[0]["ntiles"]
        d1 = self.rows >> (self.bits - P.fan_log)
        spans = [int((d1[(g * ntiles // G) * P.T:((g + 1) * ntiles // G) * P.T] == d).sum()) for g in range(G)]
        return [k for k in spans if k]


# ---- scripts ------------------------------------------------------------------------------------------------------------------
def _cyc(m, allowed, start=0):
    allowed = np.asarray(allowed, dtype=np.int64)
    return allowed[(start + np.arange(m)) % allowed.size]


class Case:
    def __init__(self, cid, bits, vals, rows, check, top_bits=64, both_orders=False):
        self.id, self.bits, self.vals, self.rows, self.check, self.top_bits, self.both_orders = cid, bits, vals, np.asarray(rows, dtype=np.int64), check, top_bits, both_orders

    def model(self):
        ms = [Model(self.bits, self.vals, self.rows, d) for d in ((False, True) if self.both_orders else (False,))]
        where = [self.check(m) for m in ms]
        for m in ms:
            assert m.listed <= WORST_POOL_CHUNKS, "more listed chunks (one copy each in the diagnostic) than worst_pool"
        return ms[0], where[0]

    def keys(self):
        return keymix.craft_rows(self.bits, self.rows, top_bits=self.top_bits, seed=len(self.id))


WORST_POOL_CHUNKS = 131071
CASES = {}


def case(name, bits_list, vals_list=(True, False), **kw):
    def deco(fn):
        for bits in bits_list:
            for vals in vals_list:
                cid = f"{name}-{bits}bits-{'vals' if vals else 'keys'}"
                CASES[cid] = functools.partial(fn, cid, bits, vals, **kw)
        return fn
    return deco


def _one_bucket(cid, bits, vals, which, top_bits=64):
    P = Geom(bits, vals, True)
    bucket = {"0": 0, "63": 63, "64": 64, "last": P.F - 1}[which]
    n = 3 * P.T + 1
    G, ntiles = (3 if bits == 5 else 1), 4                              # 5 bits: 12 289 or 24 577 rows are three workgroups' worth

    def check(m):
        e = m.ev
        assert m.passes[0]["G"] == G and m.passes[0]["ntiles"] == ntiles
        w = e.need("descriptors_by_wave_0" if bucket < 64 else "descriptors_by_wave_later")
        assert w[3] == bucket
        e.need("opened_tile_chunks")
        after_first = sum((g + 1) * ntiles // G - g * ntiles // G - 1 for g in range(G))
        assert after_first >= 1 and e.count("hot_active") == NWAVES * after_first, "hot ranking in every wave of every tile after a workgroup's first"
        assert all(x[4] == bucket for x in e.all["hot_active"])
        return w
    return Case(cid, bits, vals, np.full(n, bucket), check, top_bits)


for _which in ("0", "63", "64", "last"):
    case(f"one_bucket_{_which}", (5, 8, 9) if _which in ("0", "last") else (8, 9), which=_which)(_one_bucket)
case("top48_one_bucket_last", (5, 8, 9), which="last", top_bits=48)(_one_bucket)


@case("two_big_in_one_wave", (5, 8, 9))
def _two_big(cid, bits, vals):
    P = Geom(bits, vals, True)
    n = P.T + 100
    rows = np.where(np.arange(n) % 2 == 0, 1, 2)

    def check(m):
        assert m.passes[0]["G"] == 1
        w = m.ev.need("two_big_in_one_wave")
        assert w[:3] == (0, 0, 0) and w[3:] == (1, 2)
        return w
    return Case(cid, bits, vals, rows, check)


@case("exact_line", (8, 9))
def _exact_line(cid, bits, vals):
    P = Geom(bits, vals, True)
    rows = np.tile(np.repeat(np.arange(P.F), P.T // P.F), 3)           # T / F keys per bucket and tile: a whole number of lines
    assert (P.T // P.F) % P.LINE == 0

    def check(m):
        assert m.passes[0]["G"] == 1 and m.passes[0]["ntiles"] == 3
        assert m.ev.count("tile_carries_nothing") == 3 and m.ev.count("straddles") == 0 and m.ev.count("tile_carries_something") == 0
        assert m.ev.count("append_streak") == 0 and "append_streak" not in m.ev.max
        return m.ev.first["tile_carries_nothing"]
    return Case(cid, bits, vals, rows, check)


@case("exact_line_minus_one", (8, 9))
def _exact_line_minus_one(cid, bits, vals):
    """tile 0: every bucket one key short of its whole lines (it carries LINE - 1), the F rows this frees go to F / LINE buckets as one
    more whole line each; tiles 1 and 2: whole lines again - every bucket's first line takes LINE - 1 keys from the carry rows"""
    P = Geom(bits, vals, True)
    per = P.T // P.F
    t0 = np.concatenate([np.repeat(np.arange(P.F), per - 1), np.repeat(np.arange(P.F // P.LINE) * 3 % P.F, P.LINE)])
    assert t0.size == P.T
    rng = np.random.default_rng(bits)
    full = np.repeat(np.arange(P.F), per)
    rows = np.concatenate([rng.permutation(t0), rng.permutation(full), rng.permutation(full)])

    def check(m):
        assert m.passes[0]["G"] == 1 and m.passes[0]["ntiles"] == 3
        assert m.ev.count("tile_carries_line_minus_1_everywhere") == 3
        assert m.ev.count("every_bucket_takes_line_minus_1_from_carry") == 2 and m.ev.count("straddles") == 2 * P.F
        assert m.ev.max["straddle_from_carry"][0] == P.LINE - 1
        return m.ev.first["every_bucket_takes_line_minus_1_from_carry"]
    return Case(cid, bits, vals, rows, check)


@case("trickle", (8, 9))
def _trickle(cid, bits, vals):
    P = Geom(bits, vals, True)
    X, pattern = 77, [1, 2, 3, 3, 3, 3, 3]
    others = [b for b in range(P.F) if b != X]
    tiles = []
    for t, k in enumerate(pattern):
        tile = _cyc(P.T, others, start=t * 31)
        tile[np.arange(k) * 997 + 5] = X
        tiles.append(tile)
    rows = np.concatenate(tiles)
    appends = int((np.cumsum(pattern) < P.LINE).sum())                 # 1 + 2 + 3 (+ 3 + 3 + 3) stay below a line; the next 3 complete it
    assert appends == (3 if P.LINE == 8 else 6)

    def check(m):
        assert m.passes[0]["G"] == 1 and m.passes[0]["ntiles"] == len(pattern)
        v, w = m.ev.max["append_streak"]
        assert v >= appends and w[3] == X, (v, w)
        s = [x for x in m.ev.all["straddle_after_appends"] if x[3] == X]               # the line that takes the appended keys from the carry rows
        assert s and s[0][4] >= appends and s[0][5] == sum(pattern[:appends]), s
        return s[0]
    return Case(cid, bits, vals, rows, check)


@case("chunk_totals", (5, 8, 9))
def _chunk_totals(cid, bits, vals, top_bits=64):
    P = Geom(bits, vals, True)
    totals = [CHUNK * k + d for k in (1, 4, 5) for d in (-1, 0, 1)]
    rows = np.random.default_rng(7).permutation(np.repeat(np.arange(1, 10), totals))

    def check(m):
        e = m.ev
        assert m.passes[0]["G"] == 1 and m.n == 7680
        assert {x[3] for x in e.all["flush_full_no_partial"]} == {2, 5, 8}            # 256, 1024, 1280: nothing left, no partial chunk
        assert {x[3] for x in e.all["flush_into_open_chunk"]} == {1, 4, 7}             # 255, 1023, 1279
        if P.RL:
            assert {x[3] for x in e.all["flush_next_id_of_run"]} == {3, 9}             # 257 and 1281: the next id of the open run
            assert [(x[3], x[4]) for x in e.all["flush_fresh_run_exhausted"]] == [(6, 4)]   # 1025: four full chunks used the run up
        else:
            assert {x[3] for x in e.all["flush_fresh_single_id"]} == {3, 6, 9} and e.count("flush_next_id_of_run") == 0
        return e.first["flush_full_no_partial"]
    return Case(cid, bits, vals, rows, check, top_bits)


case("top48_chunk_totals", (5, 8, 9), top_bits=48)(_chunk_totals)


@case("flush_needs_slab", (9,))
def _flush_needs_slab(cid, bits, vals):
    """every one of the 512 buckets opens exactly one run (512 units = two slabs, nothing left of them); eight buckets end on 1025
    keys - four full chunks and one key whose run is used up - so the flush asks for eight units from an empty slab"""
    P = Geom(bits, vals, True)
    totals = np.full(P.F, 2 * P.LINE)
    totals[np.arange(8) * 61 + 3] = 4 * CHUNK + 1
    rows = np.random.default_rng(11).permutation(np.repeat(np.arange(P.F), totals))

    def check(m):
        assert m.passes[0]["G"] == 1
        w = m.ev.need("take_flush")
        assert w[3] == 8 and w[4] == 0 and m.ev.count("flush_fresh_run_exhausted") == 8, w
        return w
    return Case(cid, bits, vals, rows, check)


@case("multi_slab", (9,))
def _multi_slab(cid, bits, vals):
    P = Geom(bits, vals, True)
    rng = np.random.default_rng(13)
    rows = np.concatenate([rng.permutation(np.repeat(np.arange(P.F), P.LINE)), np.full(P.T, 7)])
    assert rows.size == 2 * P.T

    def check(m):
        assert m.passes[0]["G"] == 1
        w = m.ev.need("take_tile_several_slabs")
        assert w[:3] == (0, 0, 0) and w[3] == 512 and w[4] == 2                        # 512 runs = 2048 ids in the first tile
        later = [x for x in m.ev.all["take_tile"] if x[2] == 1]
        assert later and later[0][4] == 0, later                                       # ... and tile 1 finds the slab empty
        return w
    return Case(cid, bits, vals, rows, check)


@case("hot_switch", (8, 9))
def _hot_switch(cid, bits, vals):
    P = Geom(bits, vals, True)
    X, Y, K = 5, 200, P.KPT
    tid, lane = np.arange(NT), np.arange(NT) % 64

    def uniform(shift):
        d = (tid[:, None] * K + np.arange(K)[None, :] + shift) % P.F
        d[(d == X) | (d == Y)] = 9
        return d
    t0 = uniform(0); t0[lane < 8, K - 1] = X                                            # exactly 8 lanes of every wave: x becomes hot
    t1 = uniform(3); t1[lane == 3, 0] = X; t1[lane < 20, 1] = X; t1[:, 2] = X            # hot: 1 hot lane, hot and other lanes, all lanes
    t2 = uniform(5)                                                                     # no x at all: cool-down
    t3 = uniform(7); t3[lane < 7, K - 1] = Y                                            # exactly 7 lanes: below the threshold
    t4 = uniform(11); t4[lane < 9, K - 1] = Y; t4[lane == 0, K - 1] = Y                  # y becomes hot
    t5 = uniform(13); t5[lane == 40, 1] = Y; t5[lane >= 32, 3] = Y
    rows = np.concatenate([from_lanes(t, K) for t in (t0, t1, t2, t3, t4, t5)])

    def check(m):
        e = m.ev
        assert m.passes[0]["G"] == 1 and m.passes[0]["ntiles"] == 6
        on = e.all["hot_on"]
        assert [x for x in on if x[2] == 0] == [(0, 0, 0, w, X, 8) for w in range(NWAVES)]
        assert [x for x in on if x[2] == 4] == [(0, 0, 4, w, Y, 9) for w in range(NWAVES)] and len(on) == 2 * NWAVES
        assert e.count("detect_8_lanes") == NWAVES and [x[2] for x in e.all["detect_7_lanes"]] == [3] * NWAVES
        assert sorted({(x[2], x[4]) for x in e.all["hot_active"]}) == [(1, X), (2, X), (5, Y)]
        for name in ("hot_single_lane", "hot_mixed_lanes", "hot_all_lanes"):
            assert (0, 0, 1, 0, X) in e.all[name], name
        assert [x[2] for x in e.all["hot_cooled"]] == [2] * NWAVES
        assert (0, 0, 5, 0, Y) in e.all["hot_single_lane"] and (0, 0, 5, 0, Y) in e.all["hot_mixed_lanes"]
        return on[0]
    return Case(cid, bits, vals, rows, check)


def _tails(cid, bits, vals, which):
    P = Geom(bits, vals, True)
    n = {"1": 1, "2": 2, "3": 3, "255": 255, "256": 256, "257": 257, "T-1": P.T - 1, "T": P.T, "T+1": P.T + 1, "2T-1": 2 * P.T - 1,
         "2T+1": 2 * P.T + 1}[which]
    own = P.F - 2
    rows = _cyc(n, [b for b in range(P.F) if b != own], start=n)
    rows[-1] = own                                                                     # the last row: a bucket (and a key) of its own

    def check(m):
        assert (m.passes[0]["G"] == 1 or bits == 5) and m.passes[0]["ntiles"] == -(-n // P.T)     # (5 bits: two workgroups from 8192 rows on)
        assert [s.tolist() for s in m.level[own]] == [[n - 1]]
        return (0, 0, m.passes[0]["ntiles"] - 1, own)
    return Case(cid, bits, vals, rows, check)


for _which in ("1", "2", "3", "255", "256", "257", "T-1", "T", "T+1", "2T-1", "2T+1"):
    case(f"tails_{_which}", (5, 8, 9), which=_which)(_tails)


# ---- several workgroups, flat pass (5 bits: G = n / 4096 while the chunks reach) -----------------------------------------------
def _multi(cid, bits, vals, G, shared):
    P = Geom(bits, vals, True)
    n = G * P.T + 300
    ntiles = G + 1
    share = [((g + 1) * ntiles // G) * P.T for g in range(G)]
    if shared:
        rows = np.where(np.arange(n) % 3 == 0, 3, 17)
    else:
        rows = np.searchsorted(np.asarray(share), np.arange(n), side="right") * 4 + 1       # workgroup g: bucket 4 g + 1

    def check(m):
        assert m.passes[0]["G"] == G and m.passes[0]["ntiles"] == ntiles and ntiles % G != 0
        assert m.ev.max["groups_with_tiles"][0] == G
        if shared:
            assert len(m.level[3]) == G and len(m.level[17]) == G                       # a span of every workgroup in both lists
        else:
            assert sorted(m.level) == [4 * g + 1 for g in range(G)] and all(len(s) == 1 for s in m.level.values())
        return (0, G - 1, 0)
    return Case(cid, bits, vals, rows, check)


for _G in (2, 3, 7):
    case(f"disjoint_G{_G}", (5,), G=_G, shared=False)(_multi)
    case(f"shared_G{_G}", (5,), G=_G, shared=True)(_multi)


# ---- chunk-list passes -----------------------------------------------------------------------------------------------------------
def _final(bits, d_first, rest):
    f0 = plan_fans(bits)[0]
    return (np.asarray(d_first, dtype=np.int64) << (bits - f0)) | (np.asarray(rest, dtype=np.int64) & ((1 << (bits - f0)) - 1))


def _tiny_chunks(cid, bits, vals, top_bits=64):
    F0 = 1 << plan_fans(bits)[0]
    rows = _final(bits, np.arange(F0), np.arange(F0) * 2654435761 >> 7)

    def check(m):
        assert all(p["G"] == 1 for p in m.passes)
        assert m.passes[1]["ntiles"] == F0 and m.ev.count("one_key_chunk") >= F0
        m.ev.need("hot_on_dummy_bucket")
        w = [x for x in m.ev.all["hot_on_dummy_bucket"] if x[0] >= 1][0]                  # (pass, workgroup, tile, wave) in a chunk-list pass
        on = [x for x in m.ev.all["hot_on"] if x[0] == 1]
        assert len(on) == NWAVES and all(x[4] == m.passes[1]["P"].F for x in on)         # every wave of the second pass, at its first tile
        return w
    return Case(cid, bits, vals, rows, check, top_bits)


case("tiny_chunks", (10, 17, 18, 19))(_tiny_chunks)
case("top48_tiny_chunks", (10,), top_bits=48)(_tiny_chunks)


@case("odd_chunks", (10,))
def _odd_chunks(cid, bits, vals):
    """first pass with two workgroups: parent 9 gets 511 keys from the first and 257 from the second (chunks of 256, 255, 256 and 1
    keys: the 255 is followed by more chunks in one order of the two spans, so parent 25 gets the same spans the other way round),
    parent 20 gets 1 and 513"""
    P = Geom(5, vals, True)
    n, ntiles = 2 * P.T + 300, 3
    cut = (ntiles // 2) * P.T                                                          # workgroup 0: tile 0
    d1 = _cyc(n, [b for b in range(32) if b not in (9, 20, 25)])
    d1[np.arange(511) * 2] = 9; d1[cut + np.arange(257) * 2] = 9
    d1[2001] = 20; d1[cut + np.arange(513) * 2 + 1] = 20
    d1[np.arange(257) * 2 + 1] = 25; d1[cut + 1100 + np.arange(511)] = 25               # (parent 9 with the spans exchanged)
    rows = _final(bits, d1, np.arange(n) * 2654435761 >> 9)

    def check(m):
        assert m.passes[0]["G"] == 2
        assert m.level_spans(9) == [511, 257] and m.level_spans(25) == [257, 511] and m.level_spans(20) == [1, 513]
        sizes = {x[3] for x in m.ev.all["odd_chunk_mid_tile"]}
        assert {1, 255} <= sizes, sizes
        return m.ev.first["odd_chunk_mid_tile"]
    return Case(cid, bits, vals, rows, check, both_orders=True)


@case("one_parent_one_child", (10, 17, 18, 19))
def _one_parent_one_child(cid, bits, vals):
    n = 2 * 8192 + 1
    B = (1 << bits) - 3

    def check(m):
        assert sorted(m.level) == [B] and m.passes[-1]["ntiles"] >= 2
        return (len(m.passes) - 1, 0, 0, B)
    return Case(cid, bits, vals, np.full(n, B), check)


@case("one_parent_all_children", (10, 17, 18, 19))
def _one_parent_all_children(cid, bits, vals):
    n = 2 * 8192 + 1
    f0 = plan_fans(bits)[0]
    rest = 1 << (bits - f0)
    rows = _final(bits, np.full(n, 6), np.arange(n) % rest)

    def check(m):
        assert len(m.level) == min(rest, n) and min(m.level) == 6 * rest and max(m.level) == 6 * rest + min(rest, n) - 1
        return (1, 0, 0)
    return Case(cid, bits, vals, rows, check)


def _parent_edges(cid, bits, vals, small_only):
    """one parent of exactly tile_chunks chunks, one of tile_chunks + 1, a run of 40 parents of 100 keys; small_only: the run alone,
    so that the one workgroup of the second pass changes parent - and flushes - in every iteration"""
    P = Geom(9, vals, False)
    parts = [] if small_only else [np.full(P.TC * CHUNK, 100), np.full(P.TC * CHUNK + 1, 101)]
    parts += [np.full(100, 200 + i) for i in range(40)]
    d1 = np.random.default_rng(17).permutation(np.concatenate(parts))
    rows = _final(bits, d1, np.arange(d1.size) * 2654435761 >> 5)

    def check(m):
        assert [p["G"] for p in m.passes] == [1, 1]
        if small_only:
            w = m.ev.need("flush_in_every_iteration")
            assert w == (1, 0, 40)
        else:
            assert m.passes[1]["ntiles"] == 1 + 2 + 40
            w = m.ev.need("parent_change_on_tile_boundary")
            # parent 100 ends with a full tile; parent 101 (tile_chunks + 1 chunks) ends with a tile of one chunk: no boundary case
            assert w[3:] == (100, 101) and (1, 0, 3, 101, 200) not in m.ev.all["parent_change_on_tile_boundary"]
        return w
    return Case(cid, bits, vals, rows, check)


case("parent_edges", (18,), small_only=False)(_parent_edges)
case("parent_edges_small_parents", (18,), small_only=True)(_parent_edges)


@case("worst_pool", (18,))
def _worst_pool(cid, bits, vals):
    """131 071 rows in 131 071 different final buckets, 255 or 256 per parent: every (segment, bucket) pair of the second pass holds
    exactly one key, opens a run of four ids for it and lists one chunk"""
    n = WORST_POOL_CHUNKS
    i = np.arange(n)
    rows = _final(bits, i % 512, (i // 512) * 2 + ((i % 512) & 1))

    def check(m):
        assert [p["G"] for p in m.passes] == [1, 1] and np.unique(rows).size == n
        assert m.listed == n and m.ev.count("segment_buckets_of_one_key") == n           # (none in the first pass: 255 or 256 keys per parent)
        return m.ev.first["segment_bucket_of_one_key"]
    return Case(cid, bits, vals, rows, check)


@functools.lru_cache(maxsize=None)
def built(cid):
    c = CASES[cid]()
    m, where = c.model()
    return c, m, where


ALL = sorted(CASES)


# ---- CPU: the helper, and every script against its condition ---------------------------------------------------------------------
@pytest.mark.parametrize("bits,top_bits", [(5, 64), (9, 64), (9, 48), (10, 48), (16, 48), (18, 64), (19, 64), (24, 64)])
def test_craft_rows_puts_every_row_into_its_bucket(bits, top_bits):
    rng = np.random.default_rng(bits)
    n = 70_000
    want = rng.integers(0, 1 << bits, size=n)
    k = keymix.craft_rows(bits, want, top_bits=top_bits, seed=3)
    assert k.dtype == np.uint64 and np.array_equal(keymix.partition_of(k, bits, top_bits), want)
    assert np.unique(k).size == n
    h = keymix.mix(k)
    assert not np.any((h == np.uint64(keymix.EMPTY_MIXED)) | (h == np.uint64(keymix.FILLER_MIXED)))
    assert not np.any((h & np.uint64(0xFFFFFFFF)) == np.uint64(0xFFFFFFFF))            # the word both special keys end in is never made
    if top_bits == 48:
        owners = (h >> np.uint64(48)).astype(np.int64)
        assert np.unique(owners).size > 30_000                                        # the 16 owner bits vary
        # ... and do not move any row: the same buckets come out under every owner
        assert np.array_equal((h >> np.uint64(48 - bits)).astype(np.int64) & ((1 << bits) - 1), want)
    if top_bits == 64:
        assert np.array_equal(keymix.partition_of(k, bits), want)                       # the default is the top of hash word 1


def test_craft_rows_with_duplicates():
    want = np.array([3, 3, 3, 3, 3, 1, 1, 3, 1, 0], dtype=np.int64)
    k = keymix.craft_rows(5, want, distinct=False, keys_per_bucket=2)
    assert np.array_equal(keymix.partition_of(k, 5), want)
    assert k[0] == k[2] == k[4] and k[1] == k[3] == k[7] and k[0] != k[1] and k[5] == k[8] and k[5] != k[6]
    assert np.unique(k).size == 2 + 2 + 1
    rng = np.random.default_rng(1)
    want = rng.integers(0, 512, size=50_000)
    k = keymix.craft_rows(9, want, distinct=False, keys_per_bucket=7, top_bits=48)
    assert np.array_equal(keymix.partition_of(k, 9, 48), want) and np.unique(k).size == 512 * 7
    with pytest.raises(ValueError):
        keymix.craft_rows(9, [512])
    with pytest.raises(ValueError):
        keymix.craft_rows(18, [0], top_bits=48)                                         # 16 + 18 bits do not fit into hash word 1
    assert keymix.craft_rows(9, np.zeros(0, dtype=np.int64)).size == 0


def test_lane_mapping_round_trip():
    for K in (4, 8):
        t = np.arange(NT * K)
        lanes = to_lanes(t, K)
        assert lanes[5, 0] == 10 and lanes[5, 1] == 11 and lanes[5, 2] == (1024 + 5) * 2 and lanes[1023, K - 1] == NT * K - 1
        assert np.array_equal(from_lanes(lanes, K), t)


@pytest.mark.parametrize("cid", ALL)
def test_script_reaches_its_condition(cid):
    c, m, where = built(cid)
    assert np.array_equal(keymix.partition_of(c.keys(), c.bits, c.top_bits), c.rows)
    print(f"{cid}: n = {c.rows.size}, workgroups per pass {[p['G'] for p in m.passes]}, tiles {[p['ntiles'] for p in m.passes]}, "
          f"listed chunks {m.listed}; condition at (pass, workgroup, tile, ...) = {where}")


# ---- GPU: the pass against the reference ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fj():
    import flash_join
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_device_count() >= 1, "no HIP device: the product path must not silently fall back"
    assert flash_join.initialize() is None
    return flash_join


def run_partition(keys, bits, with_vals, top_bits):
    import torch
    from flash_hash_join_amd import _lib, api
    L = _lib.load()
    n = keys.size
    dk = torch.from_numpy(keys.view(np.int64)).cuda()
    dv = torch.arange(n, dtype=torch.int64, device="cuda") if with_vals else None
    ok = np.zeros(n, dtype=np.uint64); ov = np.zeros(n, dtype=np.uint64); ob = np.zeros(n, dtype=np.uint32)
    nvalid = ctypes.c_uint64(0)
    _lib.check(L.fj_debug_partition(api.context(0), dk.data_ptr(), dv.data_ptr() if with_vals else None, n, bits, top_bits,
                                    torch.cuda.current_stream(0).cuda_stream, ok.ctypes.data,
                                    ov.ctypes.data if with_vals else None, ob.ctypes.data, ctypes.byref(nvalid)))
    return nvalid.value, ok, ov, ob


def check_against_reference(keys, bits, with_vals, top_bits):
    """every row: per bucket the sorted (key, row) multiset of the output equals that of the input"""
    n = keys.size
    nvalid, ok, ov, ob = run_partition(keys, bits, with_vals, top_bits)
    assert nvalid == n
    want_b = keymix.partition_of(keys, bits, top_bits)
    rows = np.arange(n, dtype=np.int64)
    ref = np.lexsort((rows, keys, want_b))
    got_b = ob.astype(np.int64)
    if with_vals:
        got = np.lexsort((ov, ok, got_b))
        assert np.array_equal(got_b[got], want_b[ref])
        assert np.array_equal(ok[got], keys[ref])
        assert np.array_equal(ov[got].astype(np.int64), rows[ref])
        assert np.array_equal(keys[ov.astype(np.int64)], ok)
    else:
        got = np.lexsort((ok, got_b))
        assert np.array_equal(got_b[got], want_b[ref])
        assert np.array_equal(ok[got], keys[ref])
    assert np.all(np.diff(got_b) >= 0)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ALL)
def test_crafted_partition(fj, cid):
    c, m, where = built(cid)                                        # (asserts that the script reaches its condition)
    check_against_reference(c.keys(), c.bits, c.vals, c.top_bits)


# ---- GPU: what the diagnostic cannot reach - positions made by the first pass, value columns through real consumers ---------------
def _api_one_bucket():
    n = 3 * 4096 + 1
    return 9, 32, keymix.craft_rows(9, np.full(n, 300), distinct=False, keys_per_bucket=64, seed=21)


def _api_exact_line_minus_one():
    c = CASES["exact_line_minus_one-9bits-vals"]()
    return 9, 32, c.keys()


def _api_tails(n):
    c_rows = _cyc(n, [b for b in range(32) if b != 30], start=n)
    c_rows[-1] = 30
    return 5, -(-n // 32), keymix.craft_rows(5, c_rows, seed=n)


def _api_tiny_chunks():
    """Through the public API the plan's bits follow from the row count (at least 16 rows per partition), so a 10-bit plan has more
    than 8192 rows: 257 per first-pass bucket - every parent's chunk list ends in a chunk of a single key (with one workgroup; with
    two, in chunks of a few)."""
    d1 = np.repeat(np.arange(32), 257)
    rng = np.random.default_rng(23)
    rows = rng.permutation((d1 << 5) | (np.arange(d1.size) % 32))
    return 10, 16, keymix.craft_rows(10, rows, seed=23)


API_CASES = {"one_bucket_few_keys": _api_one_bucket, "exact_line_minus_one": _api_exact_line_minus_one, "tiny_chunks": _api_tiny_chunks}
for _n in (4095, 4096, 4097, 8191, 8193):
    API_CASES[f"tails_{_n}"] = functools.partial(_api_tails, _n)


def test_api_scripts_have_their_buckets():
    for name, fn in API_CASES.items():
        bits, target, keys = fn()
        parts = -(-keys.size // target)
        assert 16 <= target <= 4096 and max(5, int(parts - 1).bit_length()) == bits, name     # make_plan: ceil(log2(ceil(n / target))), at least 5
        b = keymix.partition_of(keys, bits)
        if name == "one_bucket_few_keys":
            assert np.all(b == 300) and np.unique(keys).size == 64
        if name.startswith("tails"):
            assert (b == 30).sum() == 1 and b[-1] == 30 and (keys == keys[-1]).sum() == 1
        if name == "tiny_chunks":
            assert np.all(np.bincount(b >> 5, minlength=32) == 257)


def _u64(x):
    import torch
    if isinstance(x, torch.Tensor):
        x = x.cpu().numpy()
    x = np.asarray(x)
    return x.view(np.uint64) if x.dtype == np.int64 else x.astype(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(API_CASES))
def test_crafted_scripts_through_the_public_api(fj, name):
    bits, target, keys = API_CASES[name]()
    n = keys.size
    passes = len(plan_fans(bits))
    rng = np.random.default_rng(n)
    values = rng.integers(0, 2**64, size=n, dtype=np.uint64)
    uk, inv = np.unique(keys, return_inverse=True)

    def after(fn):
        lt = fj.last_timings()
        assert lt["fell_back"] == 0 and lt["path"] == 0 and lt["radix_bits"] == bits and lt["passes"] == passes, (fn, lt)
    fj.set_option("plan_target_keys", target)
    try:
        # factorize: positions are made by the first pass and carried through every pass
        g, _, codes, uniques = fj.factorize(keys)
        after("factorize")
        codes, uniques = np.asarray(codes).astype(np.int64), _u64(uniques)
        assert g == uk.size and uniques.size == g and codes.size == n
        assert codes.min() >= 0 and codes.max() < g and np.array_equal(uniques[codes], keys)
        # lookup_indices: probe-side positions, against sort and search
        build = keys
        probe = np.concatenate([rng.permutation(keys)[: n // 2 + 1], keymix.craft_rows(bits, keymix.partition_of(keys[: n // 4 + 1], bits), seed=977)])
        order = np.argsort(build, kind="stable")
        sb = build[order]
        pos = np.minimum(np.searchsorted(sb, probe, side="left"), n - 1)
        want = np.where(sb[pos] == probe, order[pos], -1)
        m, _, idx = fj.lookup_indices(build, probe)
        after("lookup_indices")
        assert (want >= 0).sum() >= n // 2 + 1 and (want < 0).sum() > 0
        assert m == (want >= 0).sum() and np.array_equal(np.asarray(idx).astype(np.int64), want)
        # group_by_sum: a value column through every pass
        g2, _, gk, sums = fj.group_by_sum(keys, values)
        after("group_by_sum")
        want_s = np.zeros(uk.size, dtype=np.uint64)
        np.add.at(want_s, inv, values)
        gk, sums = _u64(gk), _u64(sums)
        o = np.argsort(gk)
        assert g2 == uk.size and np.array_equal(gk[o], uk) and np.array_equal(sums[o], want_s)
    finally:
        fj.set_option("plan_target_keys", 4096)
