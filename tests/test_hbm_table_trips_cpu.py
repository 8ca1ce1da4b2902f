"""The HBM-table form beyond one trip of its grid-stride loops: the launch caps pinned from the sources, the
shapes derived from them, the NumPy references, and the proof that every shape tells a one-trip kernel from a correct one.  Needs
no GPU; tests/test_hbm_table_trips.py runs these shapes on an MI355X against these references.

THE CAPS, AS READ FROM THE SOURCES (geometry(); a source that no longer says so fails here, by name)
  fj_host.h    gt_grid(n): workgroups of 1024 threads over n rows or slots, 4096 at most     -> a thread's 2nd trip at n > 4 194 304
               the sweeps run gt_grid(cap + 2) or gt_grid(cap) over the table's slots        -> cap >= 2^22, i.e. nb > 2^20; from there the
                                                                                                out-of-band slot `cap` is a trip of its own
  fj_join.hip  fj_launch_gt_build / _build_first: 256 threads, `blocks > 4096`               -> nb > 1 048 576
               fj_launch_gt_probe_order: `(a.np + 1023) / 1024`, `rounds < 4096`             -> np > 4 194 304
               fj_launch_gt_outer_probe: `(a.np + 4095) / 4096`, `rounds < 2048`             -> np > 8 388 608 (4096 rows per workgroup trip)
               fj_launch_gt_full_sweep: `(a.nb + 1023) / 1024`, `rounds < 2048`              -> nb > 2 097 152
  fj_group.hip fj_launch_group_fill -> fj_fill64_kernel: 256 threads, `blocks < 4096`        -> cap + 1 > 1 048 576 words (about 8 words per
                                                                                                thread below the cap, which binds from 2^23 words)
  fj_groupby_rows.hip  tiles of GJ_TS = 8192 slots over cap + 1 slots, scanned by ONE workgroup
               in rounds of GJ_NT == 1024 tiles with a carry                                 -> 2 rounds at nb > 2^21, 3 at nb > 2^22
  fj_plan.hip  gt_capacity: `cap = 64; while (cap < 2 * (u64)nb) cap <<= 1;`

THE SHAPES, DERIVED FROM THEM (shapes(); with today's sources)
  R1   one relation, n = 4 194 304 + 1 061 = 4 195 365 rows (two row trips, the second partial and ending inside a wave), cap = 2^24
       (four full sweep trips and the trip for slot `cap`), 2 049 scan tiles (three rounds).  1 500 000 distinct keys: a seeded pool,
       keys crafted (keymix.unmix) to sit in the middle of each sweep trip's slots, 500 keys whose only rows lie behind row 4 194 304,
       raw 0 three times and raw 2^64 - 1 - the form's out-of-band key - three times, once as the last row.  Two keys, KA and KB, hold
       their minimum / maximum (unsigned, signed and float64 alike) in a row behind the cut.
  R1d  the same n, all rows distinct: g == nb == out_capacity; g > 4 194 304 slots, so one sweep trip cannot hold every key.
  R1e  R1's first 4 194 304 rows, and those plus one row whose key is found nowhere else.
  J    nb = 2 097 152 + 1 061, np = 8 388 608 + 4 096 + 37; 10 % of the build rows are later copies of earlier keys; about half the
       probe rows hit; the probe side repeats keys; raw 2^64 - 1 on both sides (build: only behind row 2 097 152).  Build rows behind
       each build cut are hit, unmatched, copies; probe rows behind each probe cut hit, miss, and are the only partners of some keys;
       keys GA / GB hold their minimum / maximum in a probe row behind row 4 194 304.
  G    build side = R1's keys (nb > 4 194 304: fj_gt_group_flush_kernel's second trip), 100 003 probe rows.
Value columns: uint64 words over the full 64 bits, the same words as int64, and float64 in the "exact" domain of
tests/test_float_aggregates.py (multiples of 2^-10 up to 2^10 in magnitude, groups of at most 2^16 rows): no tolerance anywhere.

References: class GroupRef (a stable argsort, then reduceat over the runs) and class JoinRef (np.searchsorted into the sorted distinct
build keys) on RAW keys - no hashing, no keymix, never the library.  keymix only PLACES keys when a shape is built.

TIMES.  Measured without a GPU (NumPy, one CPU core): GroupRef of R1 0.7 s and 0.35 s per aggregated column, JoinRef of J 4.1 s
(the searchsorted of 8.4 M probe rows), building R1 0.25 s and J 0.6 s; this file 24 s in all, its slowest test 4.2 s.  The times on
an MI355X are in the docstring of tests/test_hbm_table_trips.py."""
import functools
import os
import re
import shutil
from types import SimpleNamespace

import numpy as np
import pytest

import keymix
from conftest import ROOT

HERE = "tests/test_hbm_table_trips_cpu.py"
CSRC = os.path.join(ROOT, "flash_hash_join_amd", "csrc")
MAXKEY = np.uint64(2**64 - 1)                              # raw: the HBM table's empty marker, kept out of band
TAIL = 1061                                                # rows behind a threshold: 16 waves and 37 lanes
EXACT = 2.0**-10


# ---- the caps, read from the sources ---------------------------------------------------------------------------------------------------
def _source(csrc, name):
    with open(os.path.join(csrc, name)) as f:
        return f.read()


def _gone(what, pattern):
    return f"{what}: the sources no longer say /{pattern}/ - {HERE} derives its shapes from that launch cap: read the new one, then update"


def _nums(text, pattern, what):
    m = re.search(pattern, text)
    assert m, _gone(what, pattern)
    return tuple(int(x, 0) for x in m.groups())


def _says(text, fragment, what):
    assert fragment in text, _gone(what, fragment)


def _body(text, signature, what):
    """a host function's text, from its signature to the closing brace in column 0"""
    at = text.find(signature)
    assert at >= 0, _gone(what, signature)
    return text[at:text.index("\n}\n", at)]


GT_GRID_USES = {                                           # every launch sized by gt_grid: file -> its arguments, in order
    "fj_groupby.hip": ["a.nb", "a.cap_mask + 2", "a.nb"],
    "fj_groupby_multi.hip": ["a.nb", "a.cap_mask + 2"],
    "fj_groupby_arg.hip": ["a.nb", "a.cap_mask + 2"],
    "fj_groupby_merge.hip": ["a.nb"],
    "fj_groupby_pair.hip": ["nb", "cap", "nb", "nb"],
    "fj_groupby_rows.hip": ["nb"],
    "fj_group.hip": ["a.np", "a.nb"],
    "fj_prepared.hip": ["a.np"],
}


@functools.lru_cache(maxsize=None)
def geometry(csrc=CSRC):
    g = {}
    h, j, p = _source(csrc, "fj_host.h"), _source(csrc, "fj_join.hip"), _source(csrc, "fj_plan.hip")
    gr, rows, dev = _source(csrc, "fj_group.hip"), _source(csrc, "fj_groupby_rows.hip"), _source(csrc, "fj_group_dev.h")

    # gt_grid: the row kernels and the sweeps over the slots
    up, nt, cap_a, cap_b = _nums(h, r"inline u32 gt_grid\(u64 n\) \{ const u64 rounds = \(n \+ (\d+)\) / (\d+); "
                                    r"return \(u32\)\(rounds < (\d+) \? \(rounds \? rounds : 1\) : (\d+)\); \}", "gt_grid")
    assert up + 1 == nt and cap_a == cap_b, _gone("gt_grid", "rounds < 4096")
    for name, want in GT_GRID_USES.items():
        uses = re.findall(r"dim3\((?:fjh::)?gt_grid\(([^()]+)\)\),\s*dim3\((\d+)\)", _source(csrc, name))
        assert [u for u, _ in uses] == want and all(int(b) == nt for _, b in uses), \
            f"{name}: gt_grid sizes {uses}, {HERE} was written against {want} with {nt} threads: read the new launch, then update"
    g["ROWS"] = nt * cap_a                                   # rows (or slots) one trip of a gt_grid launch serves

    # fj_join.hip: the table's build, the probe-order probe, the outer probe, the full join's sweep
    for fn, kern in (("fj_launch_gt_build", "fj_gt_build_kernel"), ("fj_launch_gt_build_first", "fj_gt_build_first_kernel<true>")):
        b = _body(j, f"hipError_t {fn}(const FjGtArgs& a", fn)
        up, nt, cap_a, cap_b = _nums(b, r"u64 blocks = \(a\.nb \+ (\d+)\) / (\d+);\s*if \(blocks > (\d+)\) blocks = (\d+);", fn)
        assert up + 1 == nt and cap_a == cap_b, _gone(fn, "blocks > 4096")
        _says(b, f"{kern}, dim3((u32)blocks), dim3({nt})", fn)
        assert g.setdefault("BUILD", nt * cap_a) == nt * cap_a, _gone(fn, "blocks > 4096")
    b = _body(j, "hipError_t fj_launch_gt_probe_order(", "fj_launch_gt_probe_order")
    up, nt, cap_a, cap_b = _nums(b, r"const u64 rounds = \(a\.np \+ (\d+)\) / (\d+);\s*const u32 grid = \(u32\)\(rounds < (\d+) \? rounds : (\d+)\);",
                                 "fj_launch_gt_probe_order")
    assert up + 1 == nt and cap_a == cap_b, _gone("fj_launch_gt_probe_order", "rounds < 4096")
    _says(b, f"hipLaunchKernelGGL(kern, dim3(grid), dim3({nt})", "fj_launch_gt_probe_order")
    _says(j, f"for (u64 base = (u64)blockIdx.x * {nt}; base < np; base += (u64)gridDim.x * {nt})", "fj_gt_probe_order_kernel")
    g["PROBE_ORDER"] = nt * cap_a
    b = _body(j, "hipError_t fj_launch_gt_outer_probe(", "fj_launch_gt_outer_probe")
    up, per, cap_a, cap_b = _nums(b, r"const u64 rounds = \(a\.np \+ (\d+)\) / (\d+);\s*const u32 grid = \(u32\)\(rounds < (\d+) \? rounds : (\d+)\);",
                                  "fj_launch_gt_outer_probe")
    assert up + 1 == per and cap_a == cap_b, _gone("fj_launch_gt_outer_probe", "(a.np + 4095) / 4096")
    nt, kpt = _nums(j, r"constexpr u32 NT = (\d+), KPT = (\d+);\s*__shared__ FjOjCursor cur;", "fj_gt_outer_probe_kernel")
    assert nt * kpt == per, _gone("fj_gt_outer_probe_kernel", "NT * KPT rows per trip")
    _says(j, "base < np; base += (u64)gridDim.x * NT * KPT)", "fj_gt_outer_probe_kernel")
    assert b.count(f"dim3(grid), dim3({nt})") == 6, _gone("fj_launch_gt_outer_probe", "six launches of 1024 threads")
    g["OUTER"], g["OUTER_WG_ROWS"] = per * cap_a, per
    b = _body(j, "hipError_t fj_launch_gt_full_sweep(", "fj_launch_gt_full_sweep")
    up, nt, cap_a, cap_b = _nums(b, r"const u64 rounds = \(a\.nb \+ (\d+)\) / (\d+);\s*const u32 grid = \(u32\)\(rounds < (\d+) \? rounds : (\d+)\);",
                                 "fj_launch_gt_full_sweep")
    assert up + 1 == nt and cap_a == cap_b, _gone("fj_launch_gt_full_sweep", "rounds < 2048")
    _says(b, f"fj_gt_full_sweep_kernel, dim3(grid), dim3({nt})", "fj_launch_gt_full_sweep")
    _says(j, f"for (u64 i0 = (u64)blockIdx.x * {nt}; i0 < a.nb; i0 += (u64)gridDim.x * {nt})", "fj_gt_full_sweep_kernel")
    g["FULL_SWEEP"] = nt * cap_a

    # fj_group.hip: the identities that are no byte pattern
    b = _body(gr, "hipError_t fj_launch_group_fill(", "fj_launch_group_fill")
    cap_a, cap_b, nt = _nums(b, r"fj_fill64_kernel, dim3\(\(u32\)\(blocks < (\d+) \? blocks : (\d+)\)\), dim3\((\d+)\)", "fj_launch_group_fill")
    assert cap_a == cap_b, _gone("fj_launch_group_fill", "blocks < 4096")
    _says(b, "if (v == 0 || v == ~0ull) return hipMemsetAsync(", "fj_launch_group_fill")
    g["FILL"] = nt * cap_a

    # fj_groupby_rows.hip: the tile scan
    g["GJ_TS"], = _nums(dev, r"constexpr\s+u32\s+GJ_TS\s*=\s*(\d+),", "GJ_TS")
    g["GJ_NT"], = _nums(dev, r"constexpr\s+u32\s+GJ_NT\s*=\s*(\d+),", "GJ_NT")
    _says(rows, f"GR_SPT * GJ_NT == GJ_TS && GJ_NT == {g['GJ_NT']}", "the scan's workgroup")
    _says(rows, "const u64 ntiles64 = (cap + 1 + GJ_TS - 1) / GJ_TS;", "the scan's tiles")
    _says(rows, "for (u32 base = 0; base < n; base += GJ_NT) {", "fj_gt_group_rows_scan_kernel")
    _says(rows, "hipLaunchKernelGGL(fj_gt_group_rows_scan_kernel, dim3(1), dim3(GJ_NT)", "fj_gt_group_rows_scan_kernel")
    g["SCAN_ROUND"] = g["GJ_NT"] * g["GJ_TS"]               # slots one round of the scan covers

    # fj_plan.hip: the table's capacity
    g["MIN_CAP"], g["SLOTS_PER_ROW"] = _nums(p, r"u64 cap = (\d+);\s*while \(cap < (\d+) \* \(u64\)nb\) cap <<= 1;", "gt_capacity")
    return g


def gt_capacity(nb, g=None):
    g = g or geometry()
    cap = g["MIN_CAP"]
    while cap < g["SLOTS_PER_ROW"] * nb:
        cap <<= 1
    return cap


def trips(n, per_trip):
    return -(-n // per_trip)


@functools.lru_cache(maxsize=None)
def shapes():
    """the sizes of R1 / R1d / R1e, J and G, from the caps"""
    g = geometry()
    s = SimpleNamespace()
    s.T = g["ROWS"]
    s.n1 = s.T + TAIL
    s.cap1 = gt_capacity(s.n1)
    s.sweep_trips = trips(s.cap1 + 1, g["ROWS"])            # the slots 0 .. cap, wave-uniform: gt_grid(cap + 2) is capped all the same
    s.ntiles1 = trips(s.cap1 + 1, g["GJ_TS"])
    s.scan_rounds = trips(s.ntiles1, g["GJ_NT"])
    s.B1, s.B2 = g["BUILD"], g["FULL_SWEEP"]
    s.P1, s.P2 = g["PROBE_ORDER"], g["OUTER"]
    s.nb = s.B2 + TAIL
    s.np = s.P2 + g["OUTER_WG_ROWS"] + 37
    s.capj = gt_capacity(s.nb)
    return s


# ---- references ----------------------------------------------------------------------------------------------------------------------
def identity(agg, dtype):
    """what a row without a partner holds"""
    if agg == "sum":
        return dtype.type(0)
    if dtype.kind == "f":
        return dtype.type(np.inf if agg == "min" else -np.inf)
    info = np.iinfo(dtype)
    return dtype.type(info.max if agg == "min" else info.min)


class GroupRef:
    """GROUP BY on raw keys: a stable argsort, the runs of equal keys, reduceat over them.  uniq is sorted; everything per group is
    aligned with it"""

    def __init__(self, keys):
        self.keys = np.ascontiguousarray(keys, dtype=np.uint64)
        self.n = n = self.keys.size
        self.order = np.argsort(self.keys, kind="stable")
        sk = self.keys[self.order]
        self.starts = np.flatnonzero(np.concatenate(([True], sk[1:] != sk[:-1])))
        self.uniq = sk[self.starts]
        self.g = int(self.starts.size)
        self.counts = np.diff(np.concatenate((self.starts, [n]))).astype(np.int64)
        self.first = self.order[self.starts].astype(np.int64)             # (stable: the smallest row of every run comes first)

    @functools.cached_property
    def inverse(self):
        inv = np.empty(self.n, np.int64)
        inv[self.order] = np.repeat(np.arange(self.g, dtype=np.int64), self.counts)
        return inv

    def agg(self, col):
        """sum (wrapping for integers), min, max and the smallest rows that hold min and max, per group"""
        sv = np.asarray(col)[self.order]
        r = SimpleNamespace(sum=np.add.reduceat(sv, self.starts), min=np.minimum.reduceat(sv, self.starts), max=np.maximum.reduceat(sv, self.starts))
        rows = self.order.astype(np.int64)
        r.argmin = np.minimum.reduceat(np.where(sv == np.repeat(r.min, self.counts), rows, self.n), self.starts)
        r.argmax = np.minimum.reduceat(np.where(sv == np.repeat(r.max, self.counts), rows, self.n), self.starts)
        return r

    def index_of(self, key):
        i = int(np.searchsorted(self.uniq, np.uint64(key)))
        assert i < self.g and self.uniq[i] == np.uint64(key), key
        return i


class JoinRef:
    """N:1 joins of raw keys: the probe rows looked up in the sorted distinct build keys.  `build` may be a GroupRef made before"""

    def __init__(self, build, pk):
        self.b = build if isinstance(build, GroupRef) else GroupRef(build)
        self.pk = np.ascontiguousarray(pk, dtype=np.uint64)
        idx = np.minimum(np.searchsorted(self.b.uniq, self.pk), self.b.g - 1)
        self.hit = self.b.uniq[idx] == self.pk
        self.kidx = idx                                                   # the key's place in b.uniq (valid where hit)
        self.m = int(np.count_nonzero(self.hit))
        self.build_idx = np.where(self.hit, self.b.first[idx], -1)        # the key's FIRST build row, -1 for a miss

    @functools.cached_property
    def hits_by_key(self):
        rows = np.flatnonzero(self.hit)
        k = self.kidx[rows]
        o = np.argsort(k, kind="stable")
        sk = k[o]
        starts = np.flatnonzero(np.concatenate(([True], sk[1:] != sk[:-1]))) if sk.size else np.empty(0, np.int64)
        return rows[o], starts, sk[starts]

    @functools.cached_property
    def key_counts(self):
        return np.bincount(self.kidx[self.hit], minlength=self.b.g).astype(np.int64)

    def key_agg(self, agg, col):
        """the aggregate of a probe column per build key; the identity where no probe row has the key"""
        col = np.asarray(col)
        rows, starts, present = self.hits_by_key
        out = np.full(self.b.g, identity(agg, col.dtype), dtype=col.dtype)
        op = {"sum": np.add, "min": np.minimum, "max": np.maximum}[agg]
        if present.size:
            out[present] = op.reduceat(col[rows], starts)
        return out

    def per_build_row(self, per_key):
        """group_join_*: every copy of a build key carries the key's aggregate"""
        return per_key[self.b.inverse]

    def at_first_rows(self, per_key, ident):
        """Index.group_*: the aggregate at the key's first build row, the identity in every other row"""
        out = np.full(self.b.n, ident, dtype=per_key.dtype)
        out[self.b.first] = per_key
        return out

    @functools.cached_property
    def unmatched_build_rows(self):
        return np.flatnonzero(self.key_counts[self.b.inverse] == 0)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def _distinct(rng, k, exclude=None):
    """k distinct raw keys in random order, none 0, none 2^64 - 1, none of `exclude`"""
    a = np.unique(rng.integers(1, 2**64 - 1, size=k + k // 32 + 4096, dtype=np.uint64))
    if exclude is not None:
        a = a[~np.isin(a, exclude)]
    assert a.size >= k
    return rng.permutation(a)[:k]


def _words(rng, n):
    return rng.integers(0, 2**64, size=n, dtype=np.uint64)


def _exact(rng, n):
    return rng.integers(-2**20, 2**20 + 1, size=n).astype(np.float64) * EXACT


def _pin_extremes(cols, rows_min, rows_max):
    """rows_min / rows_max: (earlier rows, the late row) of a key - the late row becomes the key's minimum / maximum in all three kinds"""
    w, f = cols
    for (early, late), low in ((rows_min, True), (rows_max, False)):
        w[early] = np.uint64(2**62) + np.arange(1, early.size + 1, dtype=np.uint64)      # (positive as uint64 and as int64)
        f[early] = np.arange(1, early.size + 1, dtype=np.float64)
        w[late] = np.uint64(5) if low else np.uint64(2**63 - 1)
        f[late] = -1024.0 if low else 1024.0


def slot_homes(keys, cap):
    """where the table of `cap` slots starts looking for a key (csrc/fj_group_dev.h gj_gt_find: hash & cap_mask, its group of 8)"""
    return (keymix.mix(keys) & np.uint64(cap - 1)) & ~np.uint64(7)


@functools.lru_cache(maxsize=None)
def r1():
    """R1: keys, the word column w (uint64; .view(int64) is the signed column) and the float column f, with what was placed where"""
    s, g = shapes(), geometry()
    rng = np.random.default_rng(20260117)
    T, n, cap = s.T, s.n1, s.cap1
    NDIST, NLATE = 1_500_000, 500
    # keys crafted into the middle of every sweep trip's slots, and into the table's last group (the walk wraps)
    per = g["ROWS"]
    placed = []
    for t in range(cap // per):
        mids = np.uint64(t * per + per // 2) + np.arange(8, dtype=np.uint64) * np.uint64(64)
        placed.append(keymix.unmix(mids | (_words(rng, 8) & ~np.uint64(cap - 1))))
    placed.append(keymix.unmix(np.uint64(cap - 8) | (_words(rng, 4) & ~np.uint64(cap - 1))))
    placed = np.concatenate(placed).astype(np.uint64)
    assert np.unique(placed).size == placed.size and not np.isin(placed, [0, 2**64 - 1]).any()
    pool = _distinct(rng, NDIST - 2 - placed.size, exclude=placed)
    late, early = pool[:NLATE], np.concatenate((pool[NLATE:], placed))
    ka, kb = early[0], early[1]
    keys = np.empty(n, np.uint64)
    keys[:early.size] = early                                              # every early key once, rows [0, early.size)
    others = early[2:]                                                     # (KA and KB get their copies by hand)
    keys[early.size:T] = rng.choice(others, T - early.size)
    keys[T:T + NLATE] = late                                               # first occurrences behind the cut
    keys[T + NLATE:] = rng.choice(others, n - T - NLATE)                   # copies behind the cut of keys before it
    keys[T + NLATE:T + NLATE + 20] = late[:20]                             # ... and of keys behind it
    rows0 = np.array([early.size + 2000, T - 1, T + NLATE + 64])
    rowsm = np.array([early.size + 1000, T + NLATE + 25, n - 1])
    rows_a = np.array([0, early.size + 10, early.size + 11, T + NLATE + 100])
    rows_b = np.array([1, early.size + 12, early.size + 13, T + NLATE + 101])
    keys[rows0], keys[rowsm], keys[rows_a], keys[rows_b] = 0, MAXKEY, ka, kb
    w, f = _words(rng, n), _exact(rng, n)
    _pin_extremes((w, f), (rows_a[:-1], rows_a[-1]), (rows_b[:-1], rows_b[-1]))
    return SimpleNamespace(keys=keys, w=w, f=f, n=n, late=late, placed=placed, ka=ka, kb=kb, rows0=rows0, rowsm=rowsm, ndist=NDIST)


@functools.lru_cache(maxsize=None)
def r1d():
    s = shapes()
    rng = np.random.default_rng(20260118)
    keys = _distinct(rng, s.n1)
    keys[12345], keys[-1] = 0, MAXKEY
    return SimpleNamespace(keys=keys, w=_words(rng, s.n1), f=_exact(rng, s.n1), n=s.n1)


@functools.lru_cache(maxsize=None)
def r1e(extra):
    """R1's rows before the cut and, extra = 1, one more row: a key found nowhere else"""
    s, r = shapes(), r1()
    n = s.T + extra
    keys = r.keys[:n].copy()
    if extra:
        assert keys[-1] == r.late[0]
    return SimpleNamespace(keys=keys, w=r.w[:n].copy(), f=r.f[:n].copy(), n=n)


@functools.lru_cache(maxsize=None)
def j():
    """J: bk / bv, pk and the probe columns pw (uint64; .view(int64)) and pf"""
    s = shapes()
    rng = np.random.default_rng(20260119)
    B1, B2, P1, P2, nb, npr = s.B1, s.B2, s.P1, s.P2, s.nb, s.np
    ncopies = nb // 10
    nnew_b = (B2 - B1) - (ncopies - 360)                                    # new keys of region B; the tail holds 359 copies and the marker's
    pool = _distinct(rng, B1 + nnew_b + 700 + 1_000_000)
    a_keys, b_new, c_new, misses = np.split(pool, [B1, B1 + nnew_b, B1 + nnew_b + 700])
    # region A: rows [0, B1), all distinct.  Its first keys are set aside: GA, GB (aggregates pinned by hand), X1 / X2 (hit only by
    # probe rows in [P1, P2) / behind P2), then 100 000 keys that no probe row has
    ga, gb, x1, x2 = a_keys[0], a_keys[1], a_keys[2:7], a_keys[7:12]
    a_unprobed, a_probed = a_keys[12:100_012], a_keys[100_012:]
    bk = np.empty(nb, np.uint64)
    bk[:B1] = a_keys
    # region B: rows [B1, B2): new keys and copies of region A's keys (probed and unprobed alike), shuffled
    bk[B1:B2] = rng.permutation(np.concatenate((b_new, rng.choice(a_keys[12:], ncopies - 360))))
    # region C: rows [B2, nb): 400 new keys that probe rows hit, 300 that none hits, 200 copies of unprobed and 159 of probed keys,
    # and raw 2^64 - 1 twice: its first row behind both build cuts, a copy as the last row
    c_hit, c_unm = c_new[:400], c_new[400:]
    tail = rng.permutation(np.concatenate((c_hit[1:], c_unm, rng.choice(a_unprobed, 200), rng.choice(a_probed, 159))))
    bk[B2:] = np.concatenate((c_hit[:1], tail[:6], [MAXKEY], tail[6:], [MAXKEY]))
    max_rows = np.array([B2 + 7, nb - 1])
    bv = _words(rng, nb)
    # probe side: half hits over the probed keys (repeats), half misses over a pool of a million (repeats)
    hit_pool = np.concatenate((a_probed, b_new))
    pk = np.where(rng.random(npr) < 0.5, rng.choice(hit_pool, npr), rng.choice(misses, npr))
    once = _distinct(rng, 3, exclude=pool)                                  # misses found nowhere else
    place = {
        "c_all": (1000 + np.arange(c_hit.size), c_hit),                    # keys whose only build row lies behind B2: every one is hit
        "c_hit": (np.array([3, P1 + 3, P2 + 10]), c_hit[:3]),              # ... in every probe trip
        "b_new": (np.array([4, P1 + 4, P2 + 12]), b_new[:3]),              # ... behind B1
        "x1": (P1 + 200 + np.arange(5), x1), "x2": (P2 + 200 + np.arange(5), x2),
        "once": (np.array([P1 - 1, P1 + 5, P2 + 11]), once),
        "max": (np.array([9, P1 + 9, npr - 1]), np.full(3, MAXKEY)),
    }
    for rows, k in place.values():
        pk[rows] = k
    rows_a, rows_b = np.array([5, 6, P1 + 100]), np.array([7, 8, P1 + 101])
    pk[rows_a], pk[rows_b] = ga, gb
    pw, pf = _words(rng, npr), _exact(rng, npr)
    _pin_extremes((pw, pf), (rows_a[:-1], rows_a[-1]), (rows_b[:-1], rows_b[-1]))
    return SimpleNamespace(bk=bk, bv=bv, pk=pk, pw=pw, pf=pf, nb=nb, np=npr, ga=ga, gb=gb, x1=x1, x2=x2, c_hit=c_hit, c_unm=c_unm,
                           a_unprobed=a_unprobed, b_new=b_new, max_rows=max_rows, place=place, ncopies=ncopies)


@functools.lru_cache(maxsize=None)
def gshape():
    """G: R1's keys as a build side, 100 003 probe rows - half of them R1's keys (those behind the cut among them), half misses"""
    r = r1()
    rng = np.random.default_rng(20260120)
    npr = 100_003
    pk = np.where(rng.random(npr) < 0.5, rng.choice(r.keys, npr), _words(rng, npr))
    pk[:r.late.size] = r.late
    pk[r.late.size:r.late.size + 3] = (r.ka, MAXKEY, 0)
    return SimpleNamespace(bk=r.keys, pk=pk, pw=_words(rng, npr), nb=r.n, np=npr)


@functools.lru_cache(maxsize=None)
def group_ref(name):
    d = {"r1": r1, "r1d": r1d, "r1e0": lambda: r1e(0), "r1e1": lambda: r1e(1)}[name]()
    return GroupRef(d.keys)


@functools.lru_cache(maxsize=None)
def join_ref(name):
    if name == "g":
        return JoinRef(group_ref("r1"), gshape().pk)
    d = j()
    return JoinRef(d.bk, d.pk)


# ---- 1. the caps -------------------------------------------------------------------------------------------------------------------------
def test_the_caps_are_what_the_sources_say_and_the_shapes_follow():
    g, s = geometry(), shapes()
    moved = f"a launch cap of the HBM-table form moved: {HERE} and tests/test_hbm_table_trips.py state the shapes for these - read the new cap, then update"
    assert (g["ROWS"], g["BUILD"], g["PROBE_ORDER"], g["OUTER"], g["FULL_SWEEP"], g["FILL"]) == (4_194_304, 1_048_576, 4_194_304, 8_388_608, 2_097_152, 1_048_576), moved
    assert (g["GJ_TS"], g["GJ_NT"], g["SCAN_ROUND"], g["MIN_CAP"], g["SLOTS_PER_ROW"], g["OUTER_WG_ROWS"]) == (8192, 1024, 2**23, 64, 2, 4096), moved
    assert [gt_capacity(nb) for nb in (0, 1, 32, 33, 2**20, 2**20 + 1, 2**21 + 1, 2**22 + 1)] == [64, 64, 64, 128, 2**21, 2**22, 2**23, 2**24]
    assert (s.n1, s.cap1, s.sweep_trips, s.ntiles1, s.scan_rounds) == (4_195_365, 2**24, 5, 2049, 3)
    assert (s.nb, s.np, s.capj) == (2_098_213, 8_392_741, 2**23)
    # R1: two row trips, the second partial and ending inside a wave; the last sweep trip serves the out-of-band slot alone; the
    # fill and the scan take more than one trip / round
    assert trips(s.n1, g["ROWS"]) == 2 and (s.n1 - g["ROWS"]) % 64 not in (0, 63) and s.n1 - g["ROWS"] > 64
    assert s.cap1 == (s.sweep_trips - 1) * g["ROWS"] and trips(s.cap1 + 1, g["FILL"]) > 1
    assert (s.ntiles1 - 1) * g["GJ_TS"] == s.cap1, "the last tile holds slot `cap` alone"
    # J: every join launch takes a second trip; the outer probe's covers more than one workgroup, the last one partial
    assert trips(s.nb, g["BUILD"]) == 3 and trips(s.nb, g["FULL_SWEEP"]) == 2 and trips(s.np, g["PROBE_ORDER"]) == 3 and trips(s.np, g["OUTER"]) == 2
    assert g["OUTER_WG_ROWS"] < s.np - g["OUTER"] < 2 * g["OUTER_WG_ROWS"]
    assert trips(gshape().nb, g["ROWS"]) == 2 and trips(gshape().np, g["ROWS"]) == 1


@pytest.mark.parametrize("name,old,new", [
    ("fj_host.h", "rounds < 4096 ? (rounds ? rounds : 1) : 4096", "rounds < 8192 ? (rounds ? rounds : 1) : 8192"),
    ("fj_join.hip", "if (blocks > 4096) blocks = 4096;", "if (blocks > 2048) blocks = 2048;"),
    ("fj_join.hip", "const u64 rounds = (a.np + 4095) / 4096;", "const u64 rounds = (a.np + 2047) / 2048;"),
    ("fj_join.hip", "(u32)(rounds < 2048 ? rounds : 2048);\n    hipLaunchKernelGGL(fj_gt_full_sweep_kernel", "(u32)(rounds < 1024 ? rounds : 1024);\n    hipLaunchKernelGGL(fj_gt_full_sweep_kernel"),
    ("fj_group.hip", "(u32)(blocks < 4096 ? blocks : 4096)", "(u32)(blocks < 4096 ? blocks : 2048)"),
    ("fj_groupby_rows.hip", "dim3(gt_grid(nb)), dim3(1024)", "dim3(gt_grid(nb)), dim3(512)"),
    ("fj_groupby_rows.hip", "base += GJ_NT) {", "base += 2 * GJ_NT) {"),
    ("fj_plan.hip", "while (cap < 2 * (u64)nb) cap <<= 1;", "while (cap < 4 * (u64)nb) cap <<= 1;"),
])
def test_an_edited_cap_fails_by_name(tmp_path, name, old, new):
    csrc = str(tmp_path / "csrc")
    shutil.copytree(CSRC, csrc, ignore=shutil.ignore_patterns("*.o", "*.so", "*.a"))
    text = _source(csrc, name)
    assert text.count(old) >= 1
    with open(os.path.join(csrc, name), "w") as f:
        f.write(text.replace(old, new))
    try:
        got = geometry(csrc)
    except AssertionError as e:
        assert HERE in str(e), str(e)
        return
    # a cap may change consistently (gt_grid's two numbers, the capacity's factor): then the derived thresholds move
    assert got != geometry(), f"{name}: `{old}` -> `{new}` went unnoticed"


# ---- 2. what the shapes hold, and what a one-trip kernel would lose ----------------------------------------------------------------------
def _differs(full, cut, what):
    assert not np.array_equal(full, cut), what


def test_r1_tells_one_row_trip_from_two():
    """rows [0, 4 194 304) against all rows: the second trip of every gt_grid(n) row kernel - fj_gt_group_by_combine_kernel,
    fj_gt_group_by_inverse_kernel, fj_gt_group_by_all_combine_kernel, fj_gt_group_by_arg_resolve_kernel and the arg combine,
    fj_gt_group_by_merge_combine_kernel, fj_pair_combine_kernel, fj_gt_pair_build_kernel, fj_gt_pair_inverse_kernel,
    fj_gt_group_rows_place_kernel - and of fj_gt_build_first_kernel behind them (4 trips at this n)"""
    s, r, full, cut = shapes(), r1(), group_ref("r1"), group_ref("r1e0")
    assert full.g == r.ndist and r.n == s.n1 and full.n == s.n1 and cut.n == s.T
    assert full.g - cut.g == r.late.size, "g differs by the keys whose first occurrence lies behind the cut"
    assert not np.isin(r.late, r.keys[:s.T]).any() and np.isin(r.late, full.uniq).all()
    assert np.all(full.first[np.searchsorted(full.uniq, r.late)] >= s.T)
    assert r.keys[-1] == MAXKEY and np.array_equal(np.flatnonzero(r.keys == MAXKEY), np.sort(r.rowsm)) and np.array_equal(np.flatnonzero(r.keys == 0), np.sort(r.rows0))
    assert (r.rowsm < s.T).sum() == 1 and (r.rows0 < s.T).sum() == 2
    # keys before the cut with copies behind it: same first occurrence, another count - and the inverse has rows the cut never wrote
    both = np.isin(cut.uniq, r.keys[s.T:])
    assert both.sum() > 400
    at = np.searchsorted(full.uniq, cut.uniq)
    assert np.array_equal(full.first[at], cut.first) and np.all(full.counts[at][both] > cut.counts[both])
    assert np.isin(r.late[:20], r.keys[s.T + r.late.size:]).all(), "copies behind the cut of keys whose first row lies behind it"
    # KA / KB: count, sum, min, max, argmin and argmax all differ, in every kind
    for col in (r.w, r.w.view(np.int64), r.f):
        fa, ca = full.agg(col), cut.agg(col[:s.T])
        for key, ext in ((r.ka, "min"), (r.kb, "max")):
            i, c = full.index_of(key), cut.index_of(key)
            assert full.counts[i] == cut.counts[c] + 1 == 4
            assert fa.sum[i] != ca.sum[c] and getattr(fa, ext)[i] != getattr(ca, ext)[c]
            assert getattr(fa, "arg" + ext)[i] >= s.T > getattr(ca, "arg" + ext)[c]
    assert full.counts.max() <= 2**16
    # R1e: the row behind the cut is a key found nowhere else
    one = group_ref("r1e1")
    assert one.n == s.T + 1 and one.g == cut.g + 1 and one.first[one.index_of(r.late[0])] == s.T


def test_r1_tells_one_sweep_trip_fill_trip_and_scan_round_from_all_of_them():
    """the slots: fj_gt_group_by_sweep_kernel, fj_gt_group_by_all_sweep_kernel, fj_gt_group_by_arg_sweep_kernel, fj_gt_pair_sweep_kernel
    (trips of 4 194 304 slots, the last one for slot `cap`), fj_fill64_kernel (trips of 1 048 576 words) and
    fj_gt_group_rows_scan_kernel (rounds of 1024 tiles of 8192 slots)"""
    g, s, r, rd = geometry(), shapes(), r1(), r1d()
    full = group_ref("r1")
    homes = slot_homes(r.placed, s.cap1)
    # a key moves forward from its home by fewer slots than the table has keys: a key homed half a trip from the trip's end stays in it
    assert full.g < g["ROWS"] // 2 - 1024 and np.isin(r.placed, full.uniq).all()
    for t in range(s.sweep_trips - 1):
        mine = (homes >= t * g["ROWS"] + g["ROWS"] // 2) & (homes < t * g["ROWS"] + g["ROWS"] // 2 + 1024)
        assert mine.sum() == 8, f"sweep trip {t}: no key placed in its slots"
    assert (homes == s.cap1 - 8).sum() == 4, "the table's last group: a walk that wraps"
    assert s.scan_rounds == 3 and g["SCAN_ROUND"] == 2 * g["ROWS"], "sweep trips 0-1 are scan round 0, trips 2-3 round 1, slot `cap` round 2"
    assert trips(s.cap1, g["FILL"]) == 16 and g["ROWS"] % g["FILL"] == 0, "every sweep trip but the first lies behind the fill's first trip"
    # the last trip / the third round serve slot `cap`: the out-of-band key's group
    assert MAXKEY in full.uniq and rd.keys[-1] == MAXKEY
    # R1d: more distinct keys than one sweep trip has slots, and than two fill trips have words: one trip must lose keys
    gd = group_ref("r1d")
    assert gd.g == gd.n == s.n1 > g["ROWS"] and gt_capacity(gd.n) == s.cap1
    assert np.all(gd.counts == 1)


def _cut_join(d, full, nb=None, np_=None):
    if nb is not None:
        return JoinRef(d.bk[:nb], d.pk)
    return JoinRef(full.b, d.pk[:np_])


def test_j_is_what_the_issue_asks_for():
    s, d, full = shapes(), j(), join_ref("j")
    assert d.bk.size == s.nb and d.pk.size == d.pw.size == d.pf.size == s.np
    assert full.b.n - full.b.g == d.ncopies and 0.09 < (full.b.n - full.b.g) / full.b.n < 0.11
    assert 0.45 < full.m / s.np < 0.55
    assert np.unique(d.pk).size < s.np // 2, "the probe side repeats keys"
    assert full.key_counts.max() <= 2**16
    assert np.array_equal(np.flatnonzero(d.bk == MAXKEY), d.max_rows) and d.max_rows.min() >= s.B2
    assert (d.pk == MAXKEY).sum() == 3 and d.pk[-1] == MAXKEY and full.hit[-1]
    for name, (rows, keys) in d.place.items():
        assert np.array_equal(d.pk[rows], keys), name
    assert not full.hit[d.place["once"][0]].any() and all((d.pk == k).sum() == 1 for k in d.place["once"][1])


@pytest.mark.parametrize("cut,kernels", [("B1", "fj_gt_build_kernel, fj_gt_build_first_kernel"), ("B2", "fj_gt_full_sweep_kernel")])
def test_j_tells_a_build_side_cut_at_a_trip_from_the_whole(cut, kernels):
    """the first 1 048 576 build rows (fj_launch_gt_build / _build_first: what one trip places in the table) and the first 2 097 152
    (fj_launch_gt_full_sweep: what one trip sweeps) against all of them"""
    s, d, full = shapes(), j(), join_ref("j")
    c = getattr(s, cut)
    part = _cut_join(d, full, nb=c)
    assert part.b.n == c < full.b.n
    assert part.m < full.m, f"{kernels}: the hit count"
    _differs(full.hit, part.hit, f"{kernels}: the miss set of left / anti / full join, join_indices, lookup, isin")
    lost = full.hit & ~part.hit
    assert lost[:s.P1].any() and lost[s.P1:s.P2].any() and lost[s.P2:].any(), "hits lost in every probe trip"
    assert np.all(full.build_idx[lost] >= c)
    assert np.isin(d.c_hit[:3], d.pk[lost]).all() and d.pk[-1] == MAXKEY and lost[-1]
    # build keys before the cut with a copy behind it: the copy is a build row the cut never saw
    copies = np.flatnonzero(np.isin(d.bk[c:], d.bk[:c])) + c
    assert copies.size >= 100 and np.all(full.b.first[full.b.inverse[copies]] < c)
    assert (full.per_build_row(full.key_counts)[copies] > 0).any(), "group_join_*: a copy behind the cut carries its key's aggregate"
    # the full join's unmatched build rows lie on both sides of the cut
    un = full.unmatched_build_rows
    assert (un < c).sum() > 1000 and (un >= c).sum() >= 300
    assert np.array_equal(un[un < c], part.unmatched_build_rows)
    if cut == "B2":
        assert np.isin(d.c_unm, d.bk[un[un >= c]]).all() and np.isin(d.bk[un[un >= c]], d.a_unprobed).sum() >= 150, "new keys and copies, unmatched, behind the cut"
        assert (full.key_counts[full.b.inverse[c:]] > 0).sum() >= 400, "... and matched rows behind it, which the sweep must skip"


@pytest.mark.parametrize("cut,kernels", [("P1", "fj_gt_probe_order_kernel, fj_gt_group_probe_kernel, fj_prep_gt_group_kernel"),
                                         ("P2", "fj_gt_outer_probe_kernel")])
def test_j_tells_a_probe_side_cut_at_a_trip_from_the_whole(cut, kernels):
    """the first 4 194 304 probe rows (fj_launch_gt_probe_order and the gt_grid(np) launches of fj_group.hip and fj_prepared.hip) and
    the first 8 388 608 (fj_launch_gt_outer_probe, whose workgroups reuse one LDS cursor pair per trip) against all of them"""
    s, d, full = shapes(), j(), join_ref("j")
    c = getattr(s, cut)
    part = _cut_join(d, full, np_=c)
    assert part.pk.size == c and np.array_equal(part.hit, full.hit[:c])
    assert part.m < full.m and full.hit[c:].any() and (~full.hit[c:]).any(), f"{kernels}: hits and misses behind the cut"
    assert (~full.hit).sum() > (~part.hit).sum(), f"{kernels}: the miss set"
    once_rows, once = d.place["once"]
    assert (once_rows >= c).any() and not np.isin(once[once_rows >= c], d.pk[:c]).any(), "a miss behind the cut found nowhere else"
    # keys whose only partners lie behind the cut: matched in the whole, unmatched build rows in the cut
    only = d.x2 if cut == "P2" else np.concatenate((d.x1, d.x2))
    rows = full.b.first[np.searchsorted(full.b.uniq, only)]
    assert np.isin(rows, part.unmatched_build_rows).all() and not np.isin(rows, full.unmatched_build_rows).any()
    _differs(full.key_counts, part.key_counts, f"{kernels}: the counts")
    if cut == "P1":                                                        # GA / GB: count, sum, min and max differ in every kind
        ia, ib = full.b.index_of(d.ga), full.b.index_of(d.gb)
        assert full.key_counts[ia] == part.key_counts[ia] + 1 == 3 and full.key_counts[ib] == part.key_counts[ib] + 1 == 3
        for col in (d.pw, d.pw.view(np.int64), d.pf):
            for agg, at in (("sum", (ia, ib)), ("min", (ia,)), ("max", (ib,))):
                whole, some = full.key_agg(agg, col), part.key_agg(agg, col[:c])
                assert all(whole[i] != some[i] for i in at), (kernels, agg, col.dtype)


def test_g_tells_one_trip_over_the_build_rows_from_two():
    """R1's keys as the build side of group_join_*: fj_gt_group_flush_kernel runs gt_grid(nb) over 4 195 365 build rows"""
    s, r, d, ref = shapes(), r1(), gshape(), join_ref("g")
    counts = ref.per_build_row(ref.key_counts)
    assert counts.size == s.n1 and (counts[s.T:] > 0).sum() >= r.late.size and (counts[s.T:] == 0).any()
    assert counts[-1] == ref.key_counts[ref.b.index_of(MAXKEY)] >= 1 and 0.4 < ref.m / d.np < 0.6
