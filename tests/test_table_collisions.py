"""Every LDS hash table (and the HBM table) against keys crafted to collide in it.

All tables here take slot, group, bucket and tag from hash word 2 (w2) of the mixed key and the partition from the top bits of hash
word 1.  The mixer is a bijection (tests/keymix.py inverts it), so keymix.craft() makes raw keys that land in one chosen partition
with any chosen w2: clusters, wrap-arounds, equal tags, cuckoo cycles - patterns random keys never form at the plan's load factors.
Every case splices one crafted partition (emptied of random keys) into an ordinary relation and compares every entry point with a
sort-and-search NumPy model on RAW keys (class Ref: np.unique / np.searchsorted / np.add.at / np.minimum.at - no hashing, no keymix,
never the library): equality of integers everywhere, no tolerance.  Each check also asserts that the crafted keys, the ghosts (same
partition, same w2, not on the build side) and the twins (same mixed key in another partition) are inside what was compared.

THE BOUND THAT ENDS EVERY TABLE LOOP ON THESE PATTERNS (read from the sources before the first GPU run; test_geometry_* pins them):

  linear probing + 64-bit CAS - fj_many.hip (MM_S), fj_outer.hip (TS 8192 / 16384), fj_group.hip and fj_groupby.hip (GJ_TS),
    fj_aligned.hip (PO_TS), fj_prepared.hip (PP_TS):
      insert  `for (step = 0; step < TS; ++step)`: at most TS steps whatever the cluster; a key that finds no slot sets hdr->full.
              fj_many's insert is `for (;;)`: at most MM_ROWS = 4096 rows are offered to MM_S = 8192 slots (a row beyond that sets
              hdr->full before it touches the table), so an empty slot always exists.
      lookup  `for (;;)` until the key or an empty slot: reached only behind `if (hdr->full) return`, and full is raised once
              LIMIT = TS - TS / 16 keys are in - at least TS / 16 slots stay empty, so a walk over any cluster, wrapped or not, stops.
              The flush / sweep loops (`while (tkeys[pos] != key)`) look for keys the build phase placed in that same table.
    A cluster therefore never climbs a ladder here: every crafted partition below (<= 3000 distinct keys < LIMIT) is joined in place.
  cuckoo (fj_join.hip cuckoo_claim / cuckoo_insert): no loop in the claim; the evicting insert is `for (it = 0; it < CK_MAXIT; ++it)`
    (48 exchanges, also when a key's two slots are the same slot and it keeps exchanging with itself), then the stash (CK_STASH = 32;
    one more sets hdr->full -> FJ_STAT_RETRY); the overflow list holds CK_OVF = 1024 keys, one more sets hdr->full.  Lookups read two
    slots and, when it is not empty, the stash: no loop over the table.
  tagged 2x4 (lds_insert / lds_probe): insert `for (step = 0; step < LDS_MAX_WALK + 2; ++step)`: the two candidate groups, then
    LDS_MAX_WALK groups from g1 + 1 on (wrapping: `(g + 1) & (NGRP - 1)`), then hdr->full; the tag loops run over the <= 4 set bits of
    a group's match mask.  The overflow lookup is `for (step = 0; step < NGRP; ++step)` and stops at the first group with a free slot.
  wide buckets (fj_join_wide.hip): claim_issue / claim_mid are straight-line; claim_resolve and the lookup walk
    `do { ++step; ... } while (__ballot(c) && step < W_MAXWALK)` - 64 buckets, wrapping `(b + 1) & (NBK - 1)` - per pending key, and a
    lane has at most 8 pending keys; a key without a slot sets hdr->full[parity] -> FJ_ITEM_RETRY.
  HBM table (fj_gt_*): insert `for (step = 0; step <= cap_mask; ++step)`, lookup `for (step = 0; step < ngroups; ++step)`; the table
    has >= 2 slots per build row, so both end at an empty slot long before.
No loop is unbounded on any pattern; no kernel was changed for that.

WHAT ONE w2 CAN HOLD (n distinct keys with the same w2 in a partition that holds nothing else; sizes derived from the pinned constants):
  cuckoo   2 slots + CK_STASH                      = 34    one more: the item is redone on the tagged table (lds_retries == 1)
  wide     BS * (1 + W_MAXWALK)                    = 260   one more: the same
  tagged   FJ_LDS_GROUP * (2 + LDS_MAX_WALK)       = 520   one more: FJ_ITEM_TOOBIG -> skew_join re-partitions that partition by 5 more
           bits of hash word 1 (lds_retries == 2: 1 + one partition) - unless the keys share those bits (craft(low_bits=...)): then the
           sub-partition is as large, skew_join gives up ("keys colliding in all of hash word 1") and the whole join runs again on the
           HBM table (fell_back == 1).  A zero-pass plan has no chunk lists to re-partition: fell_back == 1 right away.

WHICH TABLE RAN.  last_timings() tells the partitioned path from the HBM table (path), the plan (passes, radix_bits) and the rungs
(lds_retries, fell_back).  It does NOT name the counting kernel: cuckoo and wide are told apart by the plan's own rule
(wide_join_planned: a counting join over chunk lists with at most 3 probe rows per build row; pinned below), which the shapes are cut
to, and by their different capacities - 100 keys on one w2 are in place on the wide table and a retry on the cuckoo table, and both
are asserted.  The tagged table is reached through the retry rung (lds_retries >= 1) only."""
import functools
import os
import re

import numpy as np
import pytest

import keymix
from conftest import ROOT

ODD = np.uint64(0x9E3779B97F4A7C15)
ODD2 = np.uint64(0xD6E8FEB86659FD93)
FILL = 2**64 - 3
R1 = 5                 # radix bits of the one-pass plans below (pinned: make_plan lifts 1 .. 4 bits to 5)
NB_RANDOM = 30_000     # random build keys of a one-pass case
NB_ZERO = 1_500        # ... of a zero-pass case: with the crafted keys below 2048, where the many-to-many plan too stays at zero bits


# ---- the tables' geometry, read from the sources ---------------------------------------------------------------------------------
def _source(name):
    with open(os.path.join(ROOT, "flash_hash_join_amd", "csrc", name)) as f:
        return f.read()


def _num(text, pattern, what):
    m = re.search(pattern, text)
    assert m, f"{what}: the sources no longer say /{pattern}/ - tests/test_table_collisions.py crafts its inputs for another table"
    return int(m.group(1), 0)


def _says(text, fragment, what):
    assert fragment in text, f"{what}: the sources no longer say `{fragment}` - tests/test_table_collisions.py crafts its inputs for another table"


@functools.lru_cache(maxsize=1)
def geometry():
    g = {}
    c, j, w = _source("fj_common.h"), _source("fj_join.hip"), _source("fj_join_wide.hip")
    g["S"] = 1 << _num(c, r"#define\s+FJ_LDS_SLOTS_LOG\s+(\d+)", "cuckoo / tagged table size")
    g["GROUP"] = _num(c, r"#define\s+FJ_LDS_GROUP\s+(\d+)u", "tagged group size")
    g["GT_GROUP"] = _num(c, r"#define\s+FJ_GT_GROUP\s+(\d+)u", "HBM table group")
    g["BUMP"] = _num(c, r"#define\s+FJ_PLAN_BUMP_KEYS\s+(\d+)u", "plan")
    g["TARGET"] = _num(c, r"#define\s+FJ_PART_TARGET_KEYS\s+(\d+)u", "plan")
    _says(c, "#define FJ_HW2(h) ((u32)(h))", "hash word 2")
    _says(j, "constexpr u32 S = FJ_LDS_SLOTS;", "cuckoo / tagged table size")
    _says(j, "constexpr u32 NGRP = S / FJ_LDS_GROUP;", "tagged groups")
    g["NGRP"] = g["S"] // g["GROUP"]
    _says(j, "const u32 g1 = w & (NGRP - 1), g2 = (w >> 11) & (NGRP - 1);", "tagged groups of a key")
    _says(j, "{ const u32 t = w2 >> 24; return t ? t : 1u; }", "tag of a key")
    g["MAX_WALK"] = _num(j, r"constexpr\s+u32\s+LDS_MAX_WALK\s*=\s*(\d+);", "tagged walk limit")
    _says(j, "for (u32 step = 0; step < LDS_MAX_WALK + 2; ++step)", "tagged walk limit")
    _says(j, "for (u32 step = 0; step < NGRP; ++step)", "tagged overflow lookup")
    g["CK_STASH"] = _num(j, r"constexpr\s+u32\s+CK_STASH\s*=\s*(\d+)", "cuckoo stash")
    g["CK_MAXIT"] = _num(j, r"CK_MAXIT\s*=\s*(\d+);", "cuckoo eviction cap")
    g["CK_OVF"] = _num(j, r"constexpr\s+u32\s+CK_OVF\s*=\s*(\d+);", "cuckoo overflow list")
    _says(j, "for (u32 it = 0; it < CK_MAXIT; ++it)", "cuckoo eviction cap")
    _says(j, "l1 = w & (S - 1), l2 = (w >> 13) & (S - 1)", "cuckoo slots of a key")
    _says(j, "const u64 home = (h & a.cap_mask) & ~(u64)(FJ_GT_GROUP - 1);", "HBM table home")
    _says(j, "for (u64 step = 0; step <= a.cap_mask; ++step)", "HBM table insert bound")
    g["WS"] = 1 << _num(w, r"#define\s+FJ_WIDE_WSLOG\s+(\d+)", "wide table size")
    g["BS"] = _num(w, r"#define\s+FJ_WIDE_BS\s+(\d+)", "wide bucket size")
    g["W_MAXWALK"] = _num(w, r"constexpr\s+u32\s+W_MAXWALK\s*=\s*(\d+);", "wide walk limit")
    _says(w, "return (FJ_HW2(h) >> NPCLOG) & (NBK - 1u);", "wide bucket of a key")
    _says(w, "constexpr u32 NPCLOG = BSLOG - 1;", "wide bucket of a key")
    assert w.count("while (__ballot(c) && step < W_MAXWALK)") == 2, "wide walk limit: insert and lookup"
    m = _source("fj_many.hip")
    g["MM_S"] = _num(m, r"constexpr\s+u32\s+MM_S\s*=\s*(\d+),", "many-to-many table")
    g["MM_ROWS"] = _num(m, r"MM_ROWS\s*=\s*(\d+),", "many-to-many rows")
    _says(m, "if (r >= MM_ROWS) hdr->full = 1;", "many-to-many rows")
    gd = _source("fj_group_dev.h")
    g["GJ_TS"] = _num(gd, r"constexpr\s+u32\s+GJ_TS\s*=\s*(\d+),", "group table")
    _says(gd, "GJ_LIMIT = GJ_TS - GJ_TS / 16;", "group table limit")
    al = _source("fj_aligned.hip")
    g["PO_TS"] = _num(al, r"constexpr\s+u32\s+PO_TS\s*=\s*(\d+),", "probe-order table")
    _says(al, "PO_LIMIT = PO_TS - PO_TS / 16;", "probe-order table limit")
    pr = _source("fj_prepared.hip")
    _says(pr, "PP_TS = GJ_TS, PP_LIMIT = GJ_LIMIT;", "prepared table")
    o = _source("fj_outer.hip")
    _says(o, "constexpr u32 TS = VALS ? 8192u : 16384u, LIMIT = TS - TS / 16;", "outer tables")
    g["OUTER_TS"], g["ANTI_TS"] = 8192, 16384
    for name, text, ts, n in (("fj_many.hip", m, "MM_S", 7), ("fj_outer.hip", o, "TS", 3), ("fj_group.hip", _source("fj_group.hip"), "GJ_TS", 3),
                              ("fj_groupby.hip", _source("fj_groupby.hip"), "GJ_TS", 3), ("fj_aligned.hip", al, "PO_TS", 2), ("fj_prepared.hip", pr, "PP_TS", 6)):
        homes = len(re.findall(r"u32 pos = FJ_HW2\(\w+(?:\[u\])?\) & \(%s - 1\);" % ts, text))
        assert homes == n, f"{name}: {homes} probing loops start at w2 & ({ts} - 1), this file was written against {n}: read the new one, then update"
        # every loop without a step bound sits behind the full-table exit or walks to a key the build phase placed
        assert text.count("for (;;)") + text.count("while (tkeys[pos] != key)") <= n
    for name, text in (("fj_outer.hip", o), ("fj_group.hip", _source("fj_group.hip")), ("fj_aligned.hip", al)):
        _says(text, "if (hdr->full) { if (tid == 0) atomicOr(a.err, FJ_ERR_LDS_FULL); return; }", f"{name}: a full table ends the item before any lookup")
    p = _source("fj_plan.hip")
    _says(p, "if (p.bits > 0 && p.bits < 5) p.bits = 5;", "plan: one-pass plans have at least 5 bits")
    _says(p, "return np_eff <= 3 * nb;", "plan: the wide kernel's rule")
    _says(p, "if (materialize || bits <= 0 || options().join_wide == 0) return false;", "plan: the wide kernel's rule")
    js = _source("fj_joins.hip")
    _says(js, "make_plan(nb, top_bits, false, 2048)", "many-to-many plan")
    _says(js, "if (S < 5) S = std::min(5, top_bits - plan.bits - 32);", "skew_join's extra bits")
    _says(js, "keys colliding in all of hash word 1", "skew_join gives up")
    _says(js, "if (ok) t->lds_retries = 1 + (int)redone;", "skew_join's report")
    g["SKEW_BITS"] = 5
    g["CUCKOO_SAME"] = 2 + g["CK_STASH"]
    g["WIDE_SAME"] = g["BS"] * (1 + g["W_MAXWALK"])
    g["TAGGED_SAME"] = g["GROUP"] * (2 + g["MAX_WALK"])
    return g


def test_geometry_is_what_the_crafted_inputs_assume():
    g = geometry()
    assert (g["S"], g["GROUP"], g["NGRP"], g["MAX_WALK"], g["CK_STASH"], g["CK_MAXIT"], g["CK_OVF"]) == (8192, 4, 2048, 128, 32, 48, 1024)
    assert (g["WS"], g["BS"], g["W_MAXWALK"]) == (16384, 4, 64)
    assert (g["MM_S"], g["MM_ROWS"], g["GJ_TS"], g["PO_TS"], g["GT_GROUP"]) == (8192, 4096, 8192, 8192, 8)
    assert (g["CUCKOO_SAME"], g["WIDE_SAME"], g["TAGGED_SAME"]) == (34, 260, 520)
    assert (g["BUMP"], g["TARGET"]) == (3950, 4096)
    # the bit fields the patterns below are written in: cuckoo slots = w2 bits 0..12 and 13..25, tagged groups = bits 0..10 and
    # 11..21, tag = bits 24..31, wide bucket = bits 1..12, linear home = bits 0..12 (0..13 in the 16384-slot table)
    assert g["S"] == 1 << 13 and g["NGRP"] == 1 << 11 and g["WS"] // g["BS"] == 1 << 12 and g["ANTI_TS"] == 1 << 14
    # the plans the shapes are cut to: NB_RANDOM + at most 6000 crafted rows -> 5 bits for the N:1 plan and for the 2048-row plan
    for nb in (NB_RANDOM, NB_RANDOM + 6000):
        for target, bump in ((g["TARGET"], g["BUMP"]), (2048, None)):
            parts = -(-nb // target)
            bits = max(parts - 1, 0).bit_length()
            assert 1 <= bits <= 5 and (bump is None or (nb >> bits) <= bump), (nb, target, bits)
    assert NB_ZERO + 521 < 2048 < g["BUMP"]


# ---- the crafter ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radix_bits,partition", [(0, 0), (5, 0), (5, 13), (5, 31), (9, 511), (17, 70001)])
def test_crafted_keys_are_distinct_land_in_one_partition_and_collide_as_asked(radix_bits, partition):
    from flash_hash_join_amd import _lib
    L = _lib.load()
    n = 700
    for w2 in (0x5A3C1234, 0, 0xFFFFFFFF, np.arange(n, dtype=np.uint64) * np.uint64(8192) + np.uint64(8191)):
        k = keymix.craft(radix_bits, partition, w2, n, seed=3)
        assert k.dtype == np.uint64 and k.shape == (n,) and np.unique(k).size == n
        h = keymix.mix(k)
        assert np.array_equal(h & np.uint64(0xFFFFFFFF), np.broadcast_to(np.asarray(w2, dtype=np.uint64), (n,)))
        assert np.all(keymix.partition_of(k, radix_bits) == partition)
        if radix_bits:
            assert np.all(h >> np.uint64(64 - radix_bits) == np.uint64(partition))
        for i in (0, 1, n // 2, n - 1):                                  # ... and the library's own mixer says the same
            assert L.fj_key_mix64(int(k[i])) == int(h[i]) and L.fj_key_unmix64(int(h[i])) == int(k[i])
        assert not np.isin(k, np.array([keymix.EMPTY_RAW, keymix.FILLER_RAW], dtype=np.uint64)).any()
        g = keymix.ghosts(radix_bits, partition, w2, n, k, seed=3)
        assert np.unique(g).size == n and not np.isin(g, k).any() and np.all(keymix.partition_of(g, radix_bits) == partition)
        assert np.array_equal(keymix.mix(g) & np.uint64(0xFFFFFFFF), h & np.uint64(0xFFFFFFFF))
        assert not np.isin(g, np.array([keymix.EMPTY_RAW, keymix.FILLER_RAW], dtype=np.uint64)).any()
    a, b = keymix.craft(radix_bits, partition, 7, n, seed=1), keymix.craft(radix_bits, partition, 7, n, seed=2)
    assert not np.array_equal(a, b)                                      # the seed matters


def test_crafted_keys_with_few_low_bits_share_every_further_radix_bit():
    k = keymix.craft(5, 13, 0x00C0FFEE, 521, seed=1, low_bits=12)
    w1 = (keymix.mix(k) >> np.uint64(32)).astype(np.uint64)
    assert np.unique(k).size == 521 and np.all(w1 >> np.uint64(27) == 13)
    assert np.unique(w1 >> np.uint64(12)).size == 1 and np.unique(w1 & np.uint64(0xFFF)).size == 521
    wide = keymix.craft(5, 13, 0x00C0FFEE, 521, seed=1)
    assert np.unique((keymix.mix(wide) >> np.uint64(32 + 22)) & np.uint64(31)).size == 32      # all 32 values of the next 5 bits
    with pytest.raises(ValueError):
        keymix.craft(5, 13, 1, 5000, low_bits=12)
    with pytest.raises(ValueError):
        keymix.craft(5, 32, 1, 5)


def test_the_marker_and_the_filler_are_crafted_only_when_asked():
    # the marker is the last partition's word with w2 = all ones and every remaining bit set; the filler the first partition's, none set
    for part, word, raw in ((31, keymix.EMPTY_MIXED, keymix.EMPTY_RAW), (0, keymix.FILLER_MIXED, keymix.FILLER_RAW)):
        with_it = keymix.craft(5, part, 0xFFFFFFFF, 4096, seed=5, low_bits=12, allow_special=True)
        low = (keymix.mix(with_it) >> np.uint64(32)) & np.uint64(0xFFF)
        assert np.unique(low).size == 4096                               # all of the 2^12 words: the special one is among them ...
        special_there = np.uint64(raw) in with_it
        without = keymix.craft(5, part, 0xFFFFFFFF, 4095, seed=5, low_bits=12)
        assert np.uint64(raw) not in without and np.unique(without).size == 4095
        assert np.all(keymix.partition_of(without, 5) == part)
        # (low_bits = 12 leaves bits 12..26 of hash word 1 at zero: the marker's word has them set, the filler's does not)
        assert special_there == (word == keymix.FILLER_MIXED)
    full = keymix.craft_mixed(27, (1 << 27) - 1, 0xFFFFFFFF, 32, seed=9, allow_special=True)
    assert np.uint64(keymix.EMPTY_MIXED) in full
    with pytest.raises(ValueError):                                      # 32 words, one of them the marker: 32 others do not exist
        keymix.craft_mixed(27, (1 << 27) - 1, 0xFFFFFFFF, 32, seed=9)
    ok = keymix.craft_mixed(27, (1 << 27) - 1, 0xFFFFFFFF, 31, seed=9)
    assert np.uint64(keymix.EMPTY_MIXED) not in ok and np.unique(ok).size == 31


def test_twins_differ_in_the_partition_bits_only():
    k = keymix.craft(5, 13, 0x5A3C1234, 300, seed=4)
    for part in (0, 12, 14, 31):
        t = keymix.twins(k, 5, part)
        assert np.unique(t).size == 300 and not np.isin(t, k).any() and np.all(keymix.partition_of(t, 5) == part)
        assert np.array_equal(keymix.mix(t) << np.uint64(5), keymix.mix(k) << np.uint64(5))
    assert np.array_equal(keymix.twins(k, 5, 13), k)


# ---- the model: raw keys, sorting and searching ------------------------------------------------------------------------------------
def _lex(k, v):
    k, v = np.asarray(k).reshape(-1).view(np.uint64), np.asarray(v).reshape(-1).view(np.uint64)
    o = np.lexsort((v, k))
    return k[o], v[o]


class Ref:
    """Every expected result of one (build keys, build values, probe keys, probe values) case - computed once, never modified."""

    def __init__(self, bk, bv, pk, pv):
        self.bk, self.bv, self.pk, self.pv = bk, bv, pk, pv
        self.uk, self.first, self.copies = np.unique(bk, return_index=True, return_counts=True)
        pos = np.minimum(np.searchsorted(self.uk, pk), self.uk.size - 1)
        self.hit = self.uk[pos] == pk
        self.pos = pos
        self.m = int(self.hit.sum())
        hp = np.flatnonzero(self.hit)
        # N:1 (first occurrence)
        self.first_idx = _lex(hp.astype(np.int64), self.first[pos[hp]].astype(np.int64))
        self.first_pairs = _lex(pk[hp], bv[self.first[pos[hp]]])
        # every copy
        order = np.argsort(bk, kind="stable")
        start = np.searchsorted(bk[order], self.uk)
        rep = self.copies[pos[hp]]
        self.P = int(rep.sum())
        within = np.arange(self.P) - np.repeat(np.cumsum(rep) - rep, rep)
        all_pi, all_bi = np.repeat(hp, rep), order[np.repeat(start[pos[hp]], rep) + within]
        self.all_idx = _lex(all_pi.astype(np.int64), all_bi.astype(np.int64))
        self.all_pairs = _lex(pk[all_pi], bv[all_bi])
        self.miss_rows = np.flatnonzero(~self.hit)
        self.miss_keys = np.sort(pk[~self.hit])
        self.hit_keys = np.sort(pk[self.hit])
        self.rest_rows = np.flatnonzero(~np.isin(bk, pk))                # build rows whose key no probe row has, every copy
        self.rest_pairs = _lex(bk[self.rest_rows], bv[self.rest_rows])
        # probe order
        self.lookup_vals = np.where(self.hit, bv[self.first[pos]], np.uint64(FILL))
        self.lookup_rows = np.where(self.hit, self.first[pos].astype(np.int64), np.int64(-1))
        # build order: one word per distinct key, then per build row (every copy) / at the first row only (the prepared side's rule)
        self.key_cnt = np.bincount(pos[hp], minlength=self.uk.size).astype(np.int64)
        self.key_sum = np.zeros(self.uk.size, dtype=np.uint64)
        np.add.at(self.key_sum, pos[hp], pv[hp])
        self.key_min = np.full(self.uk.size, 2**64 - 1, dtype=np.uint64)
        np.minimum.at(self.key_min, pos[hp], pv[hp])
        self.row_key = np.searchsorted(self.uk, bk)

    def per_row(self, per_key):
        return per_key[self.row_key]

    def at_first(self, per_key, rest):
        out = np.full(self.bk.size, rest, dtype=per_key.dtype)
        out[self.first] = per_key
        return out


class Case:
    """bk / bv / pk / pv and what was planted: crafted (distinct, on the build side), ghosts and twins (probe side only)."""

    def __init__(self, name, bk, bv, pk, pv, crafted, ghosts, twins, radix_bits, part):
        self.name, self.bk, self.bv, self.pk, self.pv = name, bk, bv, pk, pv
        self.crafted, self.ghosts, self.twins, self.radix_bits, self.part = crafted, ghosts, twins, radix_bits, part
        self._dev = None
        # the case itself: the planted keys are where they should be, and only there
        assert np.isin(crafted, bk).all() and np.isin(crafted, pk).all()
        absent = np.concatenate([ghosts, twins])
        assert absent.size and np.isin(absent, pk).all() and not np.isin(absent, bk).any()
        special = np.array([keymix.EMPTY_RAW, keymix.FILLER_RAW], dtype=np.uint64)
        assert not np.isin(special, bk).any() and not np.isin(special, pk).any()
        assert np.unique(bv).size == bv.size

    @functools.cached_property
    def ref(self):
        return Ref(self.bk, self.bv, self.pk, self.pv)

    def args(self, device):
        """(bk, bv, pk, pv): NumPy uint64 arrays, or int64 device tensors of the same words"""
        if not device:
            return self.bk, self.bv, self.pk, self.pv
        if self._dev is None:
            import torch
            self._dev = tuple(torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda() for a in (self.bk, self.bv, self.pk, self.pv))
        return self._dev

    # what a comparison must have covered
    def covered_hits(self, keys):
        """`keys`, a compared output that holds matched probe keys, names every crafted key"""
        assert np.isin(self.crafted, _u64(keys)).all(), f"{self.name}: a crafted key is missing from the compared rows"

    def covered_misses(self, keys):
        assert np.isin(self.ghosts, _u64(keys)).all() and np.isin(self.twins, _u64(keys)).all(), f"{self.name}: a ghost or twin is missing from the compared rows"

    def covered_rows(self, probe_rows_hit, probe_rows_miss):
        pk = self.pk
        assert np.isin(self.crafted, pk[probe_rows_hit]).all(), f"{self.name}: a crafted key is missing from the compared rows"
        if probe_rows_miss is not None:
            self.covered_misses(pk[probe_rows_miss])


def _u64(a):
    return a.cpu().numpy().view(np.uint64) if hasattr(a, "cpu") else np.asarray(a).view(np.uint64)


def _i64(a):
    return _u64(a).view(np.int64)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b)


def _same_pairs(k, v, exp):
    a = _lex(_u64(k), _u64(v))
    return _same(a[0], exp[0]) and _same(a[1], exp[1])


# ---- the crafted partitions ------------------------------------------------------------------------------------------------------
# w2 of the one-slot patterns: cuckoo slots 0x1234 & 8191 = 0x1234 and (w2 >> 13) & 8191 = 0x11E1 (two different slots), tagged groups
# 0x234 and 0x786 (apart by more than LDS_MAX_WALK groups either way round: the walk from g1 never meets g2), tag 0x5A
W2_ONE = 0x5A3C3234
assert (W2_ONE & 8191, (W2_ONE >> 13) & 8191, W2_ONE & 2047, (W2_ONE >> 11) & 2047, W2_ONE >> 24) == (0x1234, 0x11E1, 0x234, 0x786, 0x5A)


def _w2_pattern(pattern, n):
    """w2 of the n crafted keys and of the ghosts (as many) of a pattern; None in place of an array: the scalar for all"""
    i = np.arange(n, dtype=np.uint64)
    if pattern == "same_w2":
        return np.full(n, W2_ONE, dtype=np.uint64), np.full(n, W2_ONE, dtype=np.uint64)
    if pattern == "same_slot":
        # both cuckoo slots are slot 0x0ABC (bits 0..12 == bits 13..25); the keys differ in bits 26..31: one slot for all of them
        w = np.uint64(0x0ABC | (0x0ABC << 13)) | ((i % np.uint64(64)) << np.uint64(26))
        return w, w
    if pattern == "cycle":
        # n = k + 1 keys over k cuckoo slots: (s0,s1) (s1,s2) .. (s_{k-1},s0) and one more pair (s0,s2) - every slot pair overlaps the next
        k = n - 1
        assert k >= 3
        s = np.uint64(0x0100) + np.arange(k, dtype=np.uint64) * np.uint64(0x0111)
        l1, l2 = np.concatenate([s, s[:1]]), np.concatenate([np.roll(s, -1), s[2:3]])
        w = l1 | (l2 << np.uint64(13)) | (np.uint64(0x15) << np.uint64(26))
        return w, w
    if pattern == "wrap":
        # home = the LAST slot of every table: bits 0..21 set - linear home 8191 (16383 in the 16384-slot table), wide bucket 4095,
        # both tagged groups 2047, cuckoo slot 8191 and one of 16 second slots; the keys differ in bits 22..31 (the tag among them)
        w = np.uint64(0x003FFFFF) | ((i % np.uint64(1024)) << np.uint64(22))
        return w, w
    if pattern == "wrap_few":
        # homes spread over the last four slots (wide buckets 4094 / 4095, tagged groups 2044 .. 2047, four pairs of cuckoo slots)
        w = (np.uint64(0x003FFFFF) - (i % np.uint64(4))) | ((i % np.uint64(256)) << np.uint64(24))
        return w, w
    if pattern == "run":
        # consecutive homes 0x0800 .. 0x0800 + n - 1 under one second cuckoo slot: ONE cluster of n slots for linear probing; ghosts: home
        # = the cluster's first slot (a miss walks all of it)
        w = np.uint64(0x4C000800) + i
        return w, np.full(n, 0x4C000800, dtype=np.uint64)
    if pattern == "tag_alias":
        # the same two tagged groups (and cuckoo slot 1), w2 >> 24 alternately 0 and 1 - both tag 1: a lookup must compare whole keys
        w = np.uint64(0x003C3234) | ((i % np.uint64(2)) << np.uint64(24))
        return w, w
    raise ValueError(pattern)


def _values(n, salt):
    return (np.arange(n, dtype=np.uint64) + np.uint64(salt)) * ODD


@functools.lru_cache(maxsize=3)
def make_case(pattern, n, shape="cuckoo", part=13, low_bits=None, dupes=False):
    """An ordinary relation with one crafted partition spliced in.
    shape "cuckoo": one-pass plan, 3.5 probe rows per build row; "wide": 2.5 (wide_join_planned); "zero": a zero-pass plan."""
    rng = np.random.default_rng([n, part, len(pattern), {"cuckoo": 0, "wide": 1, "zero": 2}[shape]])
    rb, part = (0, 0) if shape == "zero" else (R1, part)
    w2c, w2g = _w2_pattern(pattern, n)
    crafted = keymix.craft(rb, part, w2c, n, seed=n, low_bits=low_bits)
    ng = min(n, 2000)
    ghosts = keymix.ghosts(rb, part, w2g[:ng], ng, crafted, seed=n, low_bits=low_bits)
    tw = crafted[:2000]
    # the neighbouring partitions, the first and the last one (a zero-pass plan has one partition: no twins, a ghost stands in)
    others = sorted({(part + 1) % 32, (part - 1) % 32, 0, 31} - {part})
    twins = np.concatenate([keymix.twins(tw, R1, q) for q in others]) if rb else ghosts[:1]
    plain = np.unique(rng.integers(0, 2**64, size=NB_ZERO if shape == "zero" else NB_RANDOM, dtype=np.uint64))
    if rb:
        plain = plain[keymix.partition_of(plain, rb) != part]            # the crafted partition holds crafted keys only
    plain = plain[~np.isin(plain, np.concatenate([crafted, ghosts, twins]))]
    rng.shuffle(plain)
    extra = [crafted[::3], crafted[::6], plain[:40]] if dupes else []    # copies, with values of their own
    bk = np.concatenate([plain, crafted] + extra)
    bk = bk[rng.permutation(bk.size)]
    bv = _values(bk.size, 1)
    ratio = 2.5 if shape == "wide" else 3.5
    planted = [np.repeat(crafted, 1 + np.arange(n) % 3), ghosts] + ([twins] if rb else [])
    nplanted = sum(a.size for a in planted)
    room = int(bk.size * ratio) - nplanted
    assert room > bk.size // 2
    miss = rng.integers(0, 2**64, size=room // 2, dtype=np.uint64)
    miss = miss[~np.isin(miss, bk)]
    pk = np.concatenate(planted + [rng.choice(plain[: plain.size * 7 // 10], room - miss.size), miss])
    pk = pk[rng.permutation(pk.size)]
    pv = (np.arange(pk.size, dtype=np.uint64) + np.uint64(7)) * ODD2
    if shape == "wide":
        assert pk.size <= 3 * bk.size
    else:
        assert pk.size > 3 * bk.size
    return Case(f"{pattern}-{n}-{shape}", bk, bv, pk, pv, crafted, ghosts, twins, rb, part)


def test_the_cases_hold_what_they_claim():
    g = geometry()
    for pattern, n, shape in (("same_w2", g["TAGGED_SAME"] + 1, "cuckoo"), ("wrap", 3000, "wide"), ("run", 600, "cuckoo"), ("cycle", 5, "zero")):
        c = make_case(pattern, n, shape, dupes=pattern == "run")
        rb = c.radix_bits
        assert np.unique(c.crafted).size == n and np.all(keymix.partition_of(c.crafted, rb) == c.part)
        assert np.all(keymix.partition_of(c.ghosts, rb) == c.part)
        if rb:
            # the crafted partition of the build side holds the crafted keys and nothing else; the twins sit in four other partitions
            inpart = c.bk[keymix.partition_of(c.bk, rb) == c.part]
            assert np.isin(inpart, c.crafted).all()
            assert set(keymix.partition_of(c.twins, rb).tolist()) == {0, 12, 14, 31}
            nt = min(n, 2000)                                             # (the first partition's twins: of the first 2000 crafted keys)
            assert np.array_equal(keymix.mix(c.twins[:nt]) << np.uint64(rb), keymix.mix(c.crafted[:nt]) << np.uint64(rb))
        w2 = (keymix.mix(c.crafted) & np.uint64(0xFFFFFFFF)).astype(np.int64)
        if pattern == "same_w2":
            assert np.all(w2 == W2_ONE)
        if pattern == "wrap":
            assert np.all(w2 & 8191 == 8191) and np.all(w2 & 16383 == 16383) and np.all((w2 >> 1) & 4095 == 4095)
            assert np.all(w2 & 2047 == 2047) and np.all((w2 >> 11) & 2047 == 2047)
        if pattern == "run":
            assert np.array_equal(np.sort(w2 & 8191), 0x0800 + np.arange(n)) and np.unique(w2 >> 13).size == 1
            gw = (keymix.mix(c.ghosts) & np.uint64(8191)).astype(np.int64)
            assert np.all(gw == 0x0800)
            assert np.unique(c.bk).size < c.bk.size                       # duplicates, with distinct values
        if pattern == "cycle":
            l1, l2 = w2 & 8191, (w2 >> 13) & 8191
            slots = set(l1.tolist()) | set(l2.tolist())
            assert len(slots) == n - 1 and np.all(l1 != l2)               # k + 1 keys over k slots
        r = c.ref
        assert r.m == int(np.isin(c.pk, c.bk).sum()) and r.P >= r.m and r.miss_keys.size == c.pk.size - r.m
        assert np.isin(c.crafted, r.hit_keys).all() and np.isin(c.ghosts, r.miss_keys).all() and np.isin(c.twins, r.miss_keys).all()
    tag = (keymix.mix(make_case("tag_alias", 40, "cuckoo").crafted) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert set((tag >> 24).tolist()) == {0, 1} and np.unique(tag & 2047).size == 1 and np.unique((tag >> 11) & 2047).size == 1
    same = (keymix.mix(make_case("same_slot", 3, "cuckoo").crafted) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert np.all(same & 8191 == (same >> 13) & 8191) and np.unique(same).size == 3


# ---- the checks --------------------------------------------------------------------------------------------------------------------
def _plan(c, lt, many=False):
    """the plan a case was cut for (the same 5 bits for the 4096-row and the 2048-row plan; zero bits below 2048 rows)"""
    assert lt["path"] == 0, lt
    assert (lt["passes"], lt["radix_bits"]) == ((1, R1) if c.radix_bits else (0, 0)), (c.name, lt)


def _in_place(c, lt):
    _plan(c, lt)
    assert lt["fell_back"] == 0 and lt["lds_retries"] == 0, (c.name, lt)


def check_counting(fj, c, device, rung):
    """hash_join_count_radix on the shape's counting kernel; rung: "in_place" / "tagged" / "skew" / "fallback" """
    a = c.args(device)
    n = fj.hash_join_count_radix(a[0], a[1], a[2])[0]
    lt = fj.last_timings()
    print(f"{c.name}: hash_join_count_radix {n} (expected {c.ref.m}) {lt['lds_retries']=} {lt['fell_back']=} {lt['path']=}")
    assert n == c.ref.m, (c.name, n, c.ref.m)
    # the count is one integer: it covers the hard rows because the model's m counts every crafted row in and every ghost and twin out
    assert np.isin(c.crafted, c.ref.hit_keys).all() and np.isin(c.ghosts, c.ref.miss_keys).all() and np.isin(c.twins, c.ref.miss_keys).all()
    if not device:
        return                                                            # (host arrays: the streamed form reports its own path; exactness only)
    if rung == "fallback":
        assert lt["fell_back"] == 1, (c.name, lt)
        return
    _plan(c, lt)
    assert lt["fell_back"] == 0 and lt["lds_retries"] == {"in_place": 0, "tagged": 1, "skew": 2}[rung], (c.name, rung, lt)


def check_materialising(fj, c, device, rung):
    """hash_join_radix(return_arrays=True), join_indices (inner) and semi_join: the emitting kernels of the N:1 family"""
    a = c.args(device)
    r = c.ref
    for fn in ("hash_join_radix", "semi_join", "join_indices"):
        if fn == "hash_join_radix":
            n, _, k, v = fj.hash_join_radix(a[0], a[1], a[2], return_arrays=True)
            ok = _same_pairs(k, v, r.first_pairs)
            c.covered_hits(k)
        elif fn == "semi_join":
            n, _, k = fj.semi_join(a[0], a[2], return_arrays=True)
            ok = _same(np.sort(_u64(k)), r.hit_keys)
            c.covered_hits(k)
        else:
            n, _, pi, bi = fj.join_indices(a[0], a[2])
            ok = _same_pairs(pi, bi, r.first_idx)
            c.covered_rows(_i64(pi), None)
        lt = fj.last_timings()
        print(f"{c.name}: {fn} {n} (expected {r.m}) {lt['lds_retries']=} {lt['fell_back']=} {lt['path']=}")
        assert n == r.m and ok, (c.name, fn)
        if rung == "fallback":
            assert lt["fell_back"] == 1, (c.name, fn, lt)
        elif rung is not None:
            _plan(c, lt)
            assert lt["fell_back"] == 0, (c.name, fn, lt)
            # (an emitting pass may add a retry of its own to the counting pass's: fj_emit_pairs)
            assert (lt["lds_retries"] == 0) if rung == "in_place" else (lt["lds_retries"] >= {"tagged": 1, "skew": 2}[rung]), (c.name, fn, rung, lt)


def check_outer_forms(fj, c, device):
    """left / anti / full (fj_outer.hip: 8192 slots with values, 16384 for the anti form), both duplicates settings, the many-to-many
    inner join (fj_many.hip) and the gather maps - linear probing: in place whatever the cluster"""
    a = c.args(device)
    r = c.ref
    n_p, m, P, u, rest = c.pk.size, r.m, r.P, r.miss_keys.size, r.rest_rows.size
    n, _, k, v = fj.left_join(a[0], a[1], a[2], return_arrays=True, fill_value=FILL)
    _in_place(c, fj.last_timings())
    k, v = _u64(k), _u64(v)
    assert n == m and k.size == n_p and _same_pairs(k[:m], v[:m], r.first_pairs), (c.name, "left_join: matched rows")
    assert _same(np.sort(k[m:]), r.miss_keys) and np.all(v[m:] == np.uint64(FILL)), (c.name, "left_join: unmatched rows")
    c.covered_hits(k[:m]); c.covered_misses(k[m:])
    n, _, k = fj.anti_join(a[0], a[2], return_arrays=True)
    _in_place(c, fj.last_timings())
    assert n == u and _same(np.sort(_u64(k)), r.miss_keys), (c.name, "anti_join")
    c.covered_misses(k)
    n, rr, _, k, v = fj.full_join(a[0], a[1], a[2], return_arrays=True, fill_value=FILL)
    _in_place(c, fj.last_timings())
    k, v = _u64(k), _u64(v)
    assert (n, rr) == (m, rest) and k.size == n_p + rest and _same_pairs(k[:m], v[:m], r.first_pairs), (c.name, "full_join: matched rows")
    assert _same(np.sort(k[m:n_p]), r.miss_keys) and np.all(v[m:n_p] == np.uint64(FILL)), (c.name, "full_join: unmatched probe rows")
    assert _same_pairs(k[n_p:], v[n_p:], r.rest_pairs), (c.name, "full_join: unmatched build rows")
    c.covered_hits(k[:m]); c.covered_misses(k[m:n_p])
    # every copy (fj_many.hip)
    n = fj.inner_join_count(a[0], a[1], a[2])[0]
    _in_place(c, fj.last_timings())
    assert n == P, (c.name, "inner_join_count", n, P)
    n, _, k, v = fj.inner_join(a[0], a[1], a[2], return_arrays=True)
    _in_place(c, fj.last_timings())
    assert n == P and _same_pairs(k, v, r.all_pairs), (c.name, "inner_join")
    c.covered_hits(k)
    n, uu, _, k, v = fj.left_join(a[0], a[1], a[2], return_arrays=True, fill_value=FILL, duplicates="all")
    _in_place(c, fj.last_timings())
    k, v = _u64(k), _u64(v)
    assert (n, uu) == (P, u) and k.size == P + u and _same_pairs(k[:P], v[:P], r.all_pairs), (c.name, "left_join(all): pairs")
    assert _same(np.sort(k[P:]), r.miss_keys) and np.all(v[P:] == np.uint64(FILL)), (c.name, "left_join(all): unmatched rows")
    c.covered_hits(k[:P]); c.covered_misses(k[P:])
    # gather maps: the left form (first occurrence) and the full form over every copy
    n, _, pi, bi = fj.join_indices(a[0], a[2], how="left")
    _in_place(c, fj.last_timings())
    pi, bi = _i64(pi), _i64(bi)
    assert n == m and pi.size == n_p and _same_pairs(pi[:m], bi[:m], r.first_idx), (c.name, "join_indices(left): matched")
    assert _same(np.sort(pi[m:]), r.miss_rows) and np.all(bi[m:] == -1), (c.name, "join_indices(left): unmatched")
    c.covered_rows(pi[:m], pi[m:])
    n, uu, rr, _, pi, bi = fj.join_indices(a[0], a[2], how="full", duplicates="all")
    _in_place(c, fj.last_timings())
    pi, bi = _i64(pi), _i64(bi)
    assert (n, uu, rr) == (P, u, rest) and _same_pairs(pi[:P], bi[:P], r.all_idx), (c.name, "join_indices(full, all): pairs")
    assert _same(np.sort(pi[P:P + u]), r.miss_rows) and np.all(bi[P:P + u] == -1), (c.name, "join_indices(full, all): unmatched probe rows")
    assert np.all(pi[P + u:] == -1) and _same(np.sort(bi[P + u:]), r.rest_rows), (c.name, "join_indices(full, all): unmatched build rows")
    c.covered_rows(pi[:P], pi[P:P + u])


def _covers_every_probe_row(c, out):
    """a probe-order output has one word per probe row: all of them are compared, and the planted keys are among the probe rows"""
    assert out.shape[0] == c.pk.size
    assert np.isin(c.crafted, c.pk).all() and np.isin(c.ghosts, c.pk).all() and np.isin(c.twins, c.pk).all()


def check_probe_order(fj, c, device):
    """lookup / isin / lookup_indices (fj_aligned.hip)"""
    a = c.args(device)
    r = c.ref
    m, _, vals, mask = fj.lookup(a[0], a[1], a[2], fill_value=FILL, return_mask=True)
    _in_place(c, fj.last_timings())
    mask = mask.cpu().numpy() if device else mask
    assert m == r.m and _same(_u64(vals), r.lookup_vals) and _same(mask != 0, r.hit), (c.name, "lookup")
    _covers_every_probe_row(c, _u64(vals))
    m, _, mask = fj.isin(a[2], a[0])
    _in_place(c, fj.last_timings())
    mask = mask.cpu().numpy() if device else mask
    assert m == r.m and _same(mask != 0, r.hit), (c.name, "isin")
    _covers_every_probe_row(c, mask)
    m, _, idx = fj.lookup_indices(a[0], a[2])
    _in_place(c, fj.last_timings())
    assert m == r.m and _same(_i64(idx), r.lookup_rows), (c.name, "lookup_indices")
    _covers_every_probe_row(c, _i64(idx))


def _covers_every_build_row(c, out):
    assert out.shape[0] == c.bk.size and np.isin(c.crafted, c.bk).all()
    # ghosts and twins have no build row: they take part as probe rows that must add to NO row - the totals below say so
    assert not np.isin(c.ghosts, c.bk).any() and not np.isin(c.twins, c.bk).any()


def check_build_order(fj, c, device):
    """group_join_count / sum / min (fj_group.hip): one word per build row, every copy of a duplicated key carries the key's"""
    a = c.args(device)
    r = c.ref
    P, _, cnt = fj.group_join_count(a[0], a[2])
    _in_place(c, fj.last_timings())
    assert P == r.P and _same(_i64(cnt), r.per_row(r.key_cnt)), (c.name, "group_join_count")
    _covers_every_build_row(c, _i64(cnt))
    P, _, sums, cnt = fj.group_join_sum(a[0], a[2], a[3], return_counts=True)
    _in_place(c, fj.last_timings())
    assert P == r.P and _same(_u64(sums), r.per_row(r.key_sum)) and _same(_i64(cnt), r.per_row(r.key_cnt)), (c.name, "group_join_sum")
    P, _, mins = fj.group_join_min(a[0], a[2], a[3], signed=False)
    _in_place(c, fj.last_timings())
    assert P == r.P and _same(_u64(mins), r.per_row(r.key_min)), (c.name, "group_join_min")
    _covers_every_build_row(c, _u64(mins))


def check_prepared(fj, c, device):
    """build_index(...).lookup / lookup_indices / group_sum with out= over two batches (fj_prepared.hip: build, probe and aggregate
    kernels); a duplicated key's aggregate lands at its FIRST build row"""
    a = c.args(device)
    r = c.ref
    with fj.build_index(a[0], a[1]) as idx:
        lt = fj.last_timings()
        _plan(c, lt)
        assert lt["fell_back"] == 0, (c.name, lt)
        assert idx.num_keys == r.uk.size and idx.num_rows == c.bk.size
        m, _, vals, mask = idx.lookup(a[2], fill_value=FILL, return_mask=True)
        _in_place(c, fj.last_timings())
        mask = mask.cpu().numpy() if device else mask
        assert m == r.m and _same(_u64(vals), r.lookup_vals) and _same(mask != 0, r.hit), (c.name, "Index.lookup")
        _covers_every_probe_row(c, _u64(vals))
        m, _, rows = idx.lookup_indices(a[2])
        _in_place(c, fj.last_timings())
        assert m == r.m and _same(_i64(rows), r.lookup_rows), (c.name, "Index.lookup_indices")
        _covers_every_probe_row(c, _i64(rows))
        cut = (c.pk.size * 2 // 5) & ~1
        m0, _, acc = idx.group_sum(a[2][:cut], a[3][:cut])
        _in_place(c, fj.last_timings())
        m1, _, acc2 = idx.group_sum(a[2][cut:], a[3][cut:], out=acc)
        _in_place(c, fj.last_timings())
        assert m0 + m1 == r.m and m0 == int(r.hit[:cut].sum()), (c.name, "Index.group_sum: hits per batch")
        assert _same(_u64(acc2), r.at_first(r.key_sum, 0)), (c.name, "Index.group_sum over two batches")
        _covers_every_build_row(c, _u64(acc2))


def check_single_relation(fj, keys_np, vals_np, device, name, crafted, radix_bits_passes):
    """group_by_sum / unique(return_index=True) / factorize (fj_groupby.hip) on one relation"""
    if device:
        import torch
        keys, vals = (torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda() for x in (keys_np, vals_np))
    else:
        keys, vals = keys_np, vals_np
    uk, first, inv = np.unique(keys_np, return_index=True, return_inverse=True)
    sums = np.zeros(uk.size, dtype=np.uint64)
    np.add.at(sums, inv, vals_np)
    assert np.isin(crafted, uk).all()

    def planned():
        lt = fj.last_timings()
        assert lt["path"] == 0 and lt["fell_back"] == 0 and lt["lds_retries"] == 0 and (lt["radix_bits"], lt["passes"]) == radix_bits_passes, (name, lt)
    g, _, gk, gs = fj.group_by_sum(keys, vals)
    planned()
    gk, gs = _u64(gk), _u64(gs)
    o = np.argsort(gk)
    assert g == uk.size and _same(gk[o], uk) and _same(gs[o], sums), (name, "group_by_sum")     # (gk == uk: every crafted key has its row)
    g, _, gk, gi = fj.unique(keys, return_index=True)
    planned()
    gk, gi = _u64(gk), _i64(gi)
    o = np.argsort(gk)
    assert g == uk.size and _same(gk[o], uk) and _same(gi[o], first.astype(np.int64)), (name, "unique(return_index=True)")
    g, _, codes, uniques = fj.factorize(keys)
    planned()
    codes, uniques = _i64(codes), _u64(uniques)
    assert g == uk.size and _same(np.sort(uniques), uk) and codes.shape == keys_np.shape and codes.min() >= 0 and codes.max() < g, (name, "factorize")
    rank = np.empty(g, dtype=np.int64)
    rank[np.argsort(uniques)] = np.arange(g)                              # codes in the order of the sorted keys == NumPy's inverse
    assert _same(rank[codes], inv.reshape(-1).astype(np.int64)), (name, "factorize: inverse codes")


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
OPTION_DEFAULTS = {"plan_target_keys": 4096, "join_wide": 2, "persistent_min_items": 8192, "mat_single_pass": 1, "lab_hooks": 0,
                   "scalar_hbm_table": 0, "radix_threshold": 0}


@pytest.fixture(scope="module")
def fj():
    import flash_join
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_device_count() >= 1, "no HIP device: the product path must not silently fall back"
    assert flash_join.initialize() is None
    for name, value in OPTION_DEFAULTS.items():
        assert flash_join.get_option(name) == value, f"option {name} is not at its default: the shapes below would not pick their kernels"
    return flash_join


def _same_w2_sizes():
    g = geometry()
    ck, wd, tg = g["CUCKOO_SAME"], g["WIDE_SAME"], g["TAGGED_SAME"]
    assert 2 * g["GROUP"] == 8 and g["BS"] == 4
    # (n, rung on the cuckoo kernel, rung on the wide kernel): just below, at and just above every capacity
    sizes = [(2, "in_place", "in_place"), (3, "in_place", "in_place"),                      # the cuckoo pair (the third key: the stash)
             (g["BS"], "in_place", "in_place"), (g["BS"] + 1, "in_place", "in_place"),      # a wide bucket
             (2 * g["GROUP"], "in_place", "in_place"), (2 * g["GROUP"] + 1, "in_place", "in_place"),   # the two tagged groups
             (ck, "in_place", "in_place"), (ck + 1, "tagged", "in_place"),                  # pair + stash
             (g["BS"] * g["W_MAXWALK"], "tagged", "in_place"), (wd, "tagged", "in_place"), (wd + 1, "tagged", "tagged"),
             (tg, "tagged", "tagged"), (tg + 1, "skew", "skew"), (tg + 9, "skew", "skew")]
    assert [s[0] for s in sizes] == [2, 3, 4, 5, 8, 9, 34, 35, 256, 260, 261, 520, 521, 529]
    return sizes


@pytest.mark.gpu
@pytest.mark.parametrize("n,on_cuckoo,on_wide", _same_w2_sizes(), ids=[f"n{s[0]}" for s in _same_w2_sizes()])
def test_same_w2_below_at_and_above_every_capacity(fj, n, on_cuckoo, on_wide):
    """n distinct keys on ONE w2 in a partition that holds nothing else: the counting join on the cuckoo kernel (3.5 probe rows per
    build row) and on the wide kernel (2.5), the emitting kernels and the gather map - in place where the table holds them, redone on
    the tagged table above that, re-partitioned alone beyond the tagged walk (the keys differ in the next bits of hash word 1)."""
    c = make_case("same_w2", n, "cuckoo")
    check_counting(fj, c, True, on_cuckoo)
    check_materialising(fj, c, True, on_cuckoo)
    w = make_case("same_w2", n, "wide")
    check_counting(fj, w, True, on_wide)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["cuckoo", "wide"])
def test_keys_colliding_in_all_of_hash_word_1_fall_back_to_the_whole_join(fj, shape):
    """One key more than the tagged walk takes, and the keys share every bit of hash word 1 that five more radix bits could look at:
    skew_join cannot split them and hands over to the whole-join fallback - exact there too."""
    c = make_case("same_w2", geometry()["TAGGED_SAME"] + 1, shape, low_bits=12)
    w1 = (keymix.mix(c.crafted) >> np.uint64(32)).astype(np.int64)
    assert np.unique(w1 >> 12).size == 1
    check_counting(fj, c, True, "fallback")
    if shape == "cuckoo":
        check_materialising(fj, c, True, "fallback")


@pytest.mark.gpu
@pytest.mark.parametrize("pattern,n,on_cuckoo,on_wide", [
    # one slot for three keys (the slot + two stash entries) / 5 keys over 4 pairwise-overlapping slots (one ends in the stash)
    ("same_slot", 3, "in_place", "in_place"), ("cycle", 5, "in_place", "in_place"), ("cycle", 9, "in_place", "in_place"),
    # the last slot / bucket / group of every table.  cuckoo: slot 8191 + 16 second slots + the stash hold 17 + 32 = 49 keys;
    # wide: bucket 4095, then buckets 0, 1, .. (10 / 15 of the 64 it may walk); tagged (both groups 2047): the walk wraps to group 0
    ("wrap", 40, "in_place", "in_place"), ("wrap", 60, "tagged", "in_place"),
    ("wrap_few", 36, "in_place", "in_place"),
    # 512 consecutive slots: every key has a first cuckoo slot of its own, two keys per wide bucket
    ("run", 512, "in_place", "in_place"),
    # tag bytes 0 and 1 are both tag 1: 40 keys over 3 cuckoo slots + stash = 35 -> tagged table, groups 0x234 / 0x787 and the walk
    ("tag_alias", 40, "tagged", "in_place"),
], ids=lambda v: str(v))
def test_cuckoo_edges_wraps_runs_and_equal_tags_on_the_counting_and_emitting_kernels(fj, pattern, n, on_cuckoo, on_wide):
    part = 31 if pattern.startswith("wrap") else 13                      # (the wide kernel refills its table before the LAST partition)
    c = make_case(pattern, n, "cuckoo", part=part)
    check_counting(fj, c, True, on_cuckoo)
    check_materialising(fj, c, True, on_cuckoo)
    w = make_case(pattern, n, "wide", part=part)
    check_counting(fj, w, True, on_wide)


LINEAR_CASES = [("same_w2", 600, 13, False), ("wrap", 60, 31, False), ("wrap", 3000, 31, False), ("wrap_few", 1500, 0, False),
                ("run", 2000, 13, False), ("tag_alias", 64, 13, False), ("run", 600, 13, True), ("same_w2", 300, 31, True)]
LINEAR_IDS = [f"{p}-{n}-part{q}{'-dupes' if d else ''}" for p, n, q, d in LINEAR_CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("pattern,n,part,dupes", LINEAR_CASES, ids=LINEAR_IDS)
def test_linear_probing_tables_join_any_cluster_in_place(fj, pattern, n, part, dupes):
    """One cluster of n slots - on one home, wrapping over the table's end (8192 slots, and 16384 in the anti form), a run of
    consecutive homes whose ghosts start at its first slot - through every user of the linear-probing tables: in place, exact."""
    c = make_case(pattern, n, "cuckoo", part=part, dupes=dupes)
    check_outer_forms(fj, c, True)
    check_probe_order(fj, c, True)
    check_build_order(fj, c, True)
    check_prepared(fj, c, True)
    check_materialising(fj, c, True, None)                                # (the N:1 emitting kernels on the same rows: exactness; their rungs are asserted above)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern,n", [("same_w2", 500), ("wrap", 3000), ("run", 2000)])
def test_single_relation_forms_on_a_relation_that_is_one_cluster(fj, pattern, n):
    """group_by_sum / unique / factorize: the crafted keys ARE the relation (a zero-pass plan: the kernels mix them from the flat
    array), every fourth one twice; then the same cluster inside a one-pass relation."""
    rng = np.random.default_rng(n)
    w2c, _ = _w2_pattern(pattern, n)
    crafted = keymix.craft(0, 0, w2c, n, seed=n)
    keys = np.repeat(crafted, 1 + (np.arange(n) % 4 == 0))
    keys = keys[rng.permutation(keys.size)]
    assert keys.size <= geometry()["BUMP"] and n < geometry()["GJ_TS"] - geometry()["GJ_TS"] // 16      # a zero-pass plan, a table that holds them
    check_single_relation(fj, keys, _values(keys.size, 3), True, f"{pattern}-{n}-alone", crafted, (0, 0))
    c = make_case(pattern, n, "cuckoo", part=31 if pattern == "wrap" else 13, dupes=True)
    rel = np.concatenate([c.bk, np.repeat(c.crafted, 2)])
    rel = rel[rng.permutation(rel.size)]
    check_single_relation(fj, rel, _values(rel.size, 5), True, f"{pattern}-{n}-spliced", c.crafted, (R1, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("pattern,n,rung", [("same_w2", 3, "in_place"), ("cycle", 5, "in_place"), ("same_w2", 100, "tagged"), ("wrap", 300, "tagged"),
                                            ("same_w2", 521, "fallback")], ids=lambda v: str(v))
def test_zero_pass_plans_mix_the_crafted_keys_from_the_flat_arrays(fj, pattern, n, rung):
    """Below 2048 build rows every plan has zero bits: one table, built from the caller's flat arrays (the kernels mix the raw keys
    themselves).  No chunk lists, so nothing can be re-partitioned: beyond the tagged walk the join falls back at once."""
    c = make_case(pattern, n, "zero")
    assert c.bk.size < 2048 and c.radix_bits == 0
    check_counting(fj, c, True, rung)
    check_materialising(fj, c, True, rung)
    if rung != "fallback":
        check_outer_forms(fj, c, True)
        check_probe_order(fj, c, True)
        check_build_order(fj, c, True)
        check_prepared(fj, c, True)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern,n", [("same_w2", 600), ("wrap", 1000), ("run", 2000)])
def test_hbm_table_on_keys_that_share_its_home_group(fj, pattern, n):
    """scalar_hbm_table = 1: one table of raw keys in HBM, home = the mixed key's low bits & cap_mask, aligned to a group of 8 - the
    crafted keys share it (cap >= 2^16 here: the low bits of w2), one cluster of n slots; wrap: the cluster runs over the table's end."""
    c = make_case(pattern, n, "cuckoo", part=31 if pattern == "wrap" else 13)
    a = c.args(True)
    r = c.ref
    cap = 64
    while cap < 2 * c.bk.size:
        cap <<= 1
    home = (keymix.mix(c.crafted) & np.uint64(cap - 1)).astype(np.int64) & ~7
    assert cap >= 1 << 16 and (np.unique(home).size == 1 if pattern != "run" else np.ptp(home) < n)
    if pattern == "wrap":
        assert home[0] == cap - 8
    fj.set_option("scalar_hbm_table", 1)
    try:
        n_hit = fj.hash_join_count(a[0], a[1], a[2])[0]
        assert fj.last_timings()["path"] == 1, fj.last_timings()
        assert n_hit == r.m
        n_hit, _, k, v = fj.hash_join(a[0], a[1], a[2], return_arrays=True)
        assert fj.last_timings()["path"] == 1, fj.last_timings()
        assert n_hit == r.m and _same_pairs(k, v, r.first_pairs)           # (distinct build keys: no race between copies)
        c.covered_hits(k)
        assert np.isin(c.ghosts, r.miss_keys).all() and np.isin(c.twins, r.miss_keys).all()
    finally:
        fj.set_option("scalar_hbm_table", 0)


@pytest.mark.gpu
def test_numpy_inputs_one_case_per_family(fj):
    """Host arrays: the host entries copy and call the same device code (the counting join streams the probe side under its copy and
    reports that form's path: exactness only there)."""
    c = make_case("wrap", 60, "cuckoo", part=31)
    check_counting(fj, c, False, "tagged")
    check_materialising(fj, c, False, "tagged")
    d = make_case("run", 600, "cuckoo", part=13, dupes=True)
    check_outer_forms(fj, d, False)
    check_probe_order(fj, d, False)
    check_build_order(fj, d, False)
    check_prepared(fj, d, False)
    rel = np.concatenate([d.bk, np.repeat(d.crafted, 2)])
    check_single_relation(fj, rel, _values(rel.size, 5), False, "run-600-numpy", d.crafted, (R1, 1))
    fj.set_option("scalar_hbm_table", 1)
    try:
        assert fj.hash_join_count(c.bk, c.bv, c.pk)[0] == c.ref.m and fj.last_timings()["path"] == 1
    finally:
        fj.set_option("scalar_hbm_table", 0)


@pytest.mark.gpu
def test_wide_table_is_not_fooled_by_what_an_earlier_partition_left_behind(fj):
    """The wide table is never cleared: a workgroup builds its next partition over the last one's keys and tells "ours" from "stale"
    by the partition bits of hash word 1 alone.  Twins are the hardest stale entries there are: the same w2 (bucket 0x0ABC >> 1), the
    same remaining bits of hash word 1 - in EVERY one of the plan's 512 partitions, partition 0 and the last one included.  Each
    partition builds its own subset of 12 twin words (2 .. 8 of them: a bucket that is not full, full, or spilling into the next) and
    is probed for all 12: its own must hit, the words only other partitions built must miss.  The subsets differ from partition to
    partition, so whichever partition a workgroup built before, some stale twin is not among the next partition's own keys.
    How the test knows that tables were built over leftovers: the launch has at most one workgroup per CU (fj_joins.hip: grid =
    min(items, CUs)) and items are dealt round-robin, and last_timings() reports 512 partitions, every one with probe rows, on a
    device of fewer than 512 CUs - so every workgroup built at least two partitions in the one table."""
    import torch
    bits, nparts, nwords = 9, 512, 12
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus < nparts
    rng = np.random.default_rng(512)
    base = keymix.craft(bits, 0, 0x0ABC, nwords, seed=12)                 # 12 words of partition 0; their twins everywhere else
    own = np.zeros((nparts, nwords), dtype=bool)
    for q in range(nparts):
        own[q, rng.permutation(nwords)[: 2 + q % 7]] = True
    allw = np.stack([keymix.twins(base, bits, q) if q else base for q in range(nparts)])      # [partition, word]
    assert np.unique(allw).size == allw.size and np.all(keymix.partition_of(allw.reshape(-1), bits).reshape(nparts, nwords) == np.arange(nparts)[:, None])
    crafted, ghosts = allw[own], allw[~own]
    plain = np.unique(rng.integers(0, 2**64, size=NB_RANDOM, dtype=np.uint64))
    plain = plain[~np.isin(plain, allw.reshape(-1))]
    bk = np.concatenate([plain, crafted])
    bk = bk[rng.permutation(bk.size)]
    miss = rng.integers(0, 2**64, size=20_000, dtype=np.uint64)
    miss = miss[~np.isin(miss, bk)]
    pk = np.concatenate([np.repeat(allw.reshape(-1), 2), rng.choice(plain, 25_000), miss])
    pk = pk[rng.permutation(pk.size)]
    assert pk.size <= 3 * bk.size and np.bincount(keymix.partition_of(pk, bits), minlength=nparts).min() >= 2 * nwords
    c = Case("stale_twins", bk, _values(bk.size, 1), pk, _values(pk.size, 9), crafted, ghosts, ghosts, bits, -1)
    a = c.args(True)
    fj.set_option("plan_target_keys", 64)                                 # 30 000 rows / 64 -> 469 -> 512 partitions, one pass
    try:
        n = fj.hash_join_count_radix(a[0], a[1], a[2])[0]
        lt = fj.last_timings()
    finally:
        fj.set_option("plan_target_keys", 4096)
    print(f"stale twins: {n} (expected {c.ref.m}) {lt}")
    assert (lt["path"], lt["passes"], lt["radix_bits"], lt["partitions"]) == (0, 1, bits, nparts), lt
    assert lt["fell_back"] == 0 and lt["lds_retries"] == 0, lt
    assert n == c.ref.m == int(np.isin(pk, bk).sum())
    assert np.isin(crafted, c.ref.hit_keys).all() and np.isin(ghosts, c.ref.miss_keys).all()
    # ... and the same rows through the cuckoo kernel (a table that IS cleared): the same count
    fj.set_option("plan_target_keys", 64)
    fj.set_option("join_wide", 0)
    try:
        assert fj.hash_join_count_radix(a[0], a[1], a[2])[0] == c.ref.m
    finally:
        fj.set_option("join_wide", 2)
        fj.set_option("plan_target_keys", 4096)
