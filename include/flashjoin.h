/*
 * flashjoin.h -- C ABI of libflashjoin_hip.so, the MI355X (gfx950) drop-in for the hot path of
 * conanhujinming/flash_hash_join.
 *
 * The reference exposes this path only through a pybind11 module (hash_join.cpp:598-640):
 * twelve join functions that all take (build_keys, build_values, probe_keys) as uint64 arrays
 * and all return (total_results, core_duration_sec), plus initialize().  A C ABI for it does not
 * exist in the reference; this header is what a binding for the path (ctypes / cgo / JNI / a
 * pybind11 shim) binds instead of the reference's C++ templates.  Each entry point names the
 * reference interface it replaces.
 *
 * Conventions: every function returns 0 on success, non-zero on failure; fj_last_error() then
 * returns a thread-local, NUL-terminated description.  No torch / pybind types cross this ABI:
 * plain pointers and sizes only.  Keys and values are 64-bit words; int64 inputs are
 * reinterpreted bit-for-bit (the reference does the same through array_t<uint64_t>'s cast).
 */
#ifndef FLASHJOIN_H
#define FLASHJOIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)       /* the library is built with -fvisibility=hidden and linked with csrc/exports.map: these 40 entry points are all it exports */
#endif

/* algo: which of the reference's drivers the call stands for */
#define FJ_ALGO_ADAPTIVE 0 /* adaptive_hash_join_{count,materialize}   hash_join.cpp:576-594 */
#define FJ_ALGO_SCALAR 1   /* _hash_join_scalar_{count,materialize}     hash_join.cpp:383-496, :536-567 */
#define FJ_ALGO_RADIX 2    /* _hash_join_radix_{count,materialize}      hash_join.cpp:315-381, :498-534 */

/* EXTENSION (no reference counterpart: the reference deduplicates build keys, hash_join.cpp:125): OR this into `algo` for a
 * many-to-many inner join - every build row is kept, a probe row yields one pair per build row with its key, the count is the
 * number of pairs.  Partitioned plan only; fails when a final partition would hold more than 4096 build rows (a key with
 * thousands of duplicates) - unless the option "mm_heavy_keys" is 1 (below): then such a partition is joined in tiles of at most
 * 4096 build rows, in every form of the call (counting, one call with buffers, count + fj_emit_pairs, FJ_ALGO_ROW_IDS,
 * fj_join_host).  `bloom` is ignored. */
#define FJ_ALGO_MANY_TO_MANY 0x10
/* EXTENSIONS (no reference counterpart; csrc/fj_outer.hip): OR one of these into `algo` together with a base value (ADAPTIVE, SCALAR
 * or RADIX: it picks the partitioned plan or the global HBM table exactly as for the inner join).  N:1 semantics as everywhere: a
 * duplicated build key matches with the value of its FIRST occurrence in build order, on both paths.
 *   FJ_ALGO_LEFT_OUTER - left outer join; materialize = 1 only.  d_out_keys and d_out_vals (8-byte aligned) hold >= np rows.
 *                        *out_count = m, the matched probe rows (what the counting join returns); rows [0, m) are the matched
 *                        (probe_key, build_value) pairs, rows [m, np) the unmatched probe keys with value 0: every probe row once,
 *                        order within either range unspecified.
 *   FJ_ALGO_ANTI       - the probe rows without a partner.  materialize = 0: *out_count = np - the N:1 count of the same algo and
 *                        bloom.  materialize = 1: d_out_keys (8-byte aligned, >= np rows) receives the u = *out_count unmatched probe
 *                        keys in rows [0, u); d_out_vals may be NULL and is never written.  d_build_vals may be NULL.
 * Both: bloom is ignored when materialising; never a pending result for fj_emit_pairs (a result that was pending is dropped);
 * fj_join_host returns np rows (LEFT) or u keys and *out_vals = NULL (ANTI).  Refused up front, before any device work: both flags,
 * either with FJ_ALGO_MANY_TO_MANY, LEFT with materialize = 0, an output capacity below np, NULL or misaligned output buffers. */
#define FJ_ALGO_LEFT_OUTER 0x20
#define FJ_ALGO_ANTI 0x40
/* EXTENSION (no reference counterpart; the reference returns (probe_key, build_value) pairs, hash_join.cpp:365-380): OR this into
 * `algo` (also together with one of the flags above) and the output rows hold ROW POSITIONS - gather maps - instead of keys and
 * values: d_out_keys[i] = 0-based position of the probe row in d_probe_keys, d_out_vals[i] = 0-based position of the build row in
 * d_build_keys.  Order within each range unspecified, as everywhere.
 *   base (ADAPTIVE / SCALAR / RADIX) - one row per matched probe row; the build position is the key's FIRST occurrence (smallest
 *                                      index) on every path (partitioned plan, skew re-partition, HBM-table fallback, scalar_hbm_table)
 *   | FJ_ALGO_MANY_TO_MANY           - one row per (probe row, build row) with equal keys; the same 4096-rows limit
 *   | FJ_ALGO_LEFT_OUTER             - np rows: [0, m) matched, [m, np) unmatched with build position UINT64_MAX; *out_count = m
 *   | FJ_ALGO_ANTI                   - the u = *out_count unmatched probe positions; d_out_vals may be NULL and is never written
 * materialize = 1 only; d_build_vals may be NULL and is never read; bloom is ignored.  The two-phase form (count with d_out_keys ==
 * NULL, then fj_emit_pairs) works for the base and many-to-many forms: the pending result remembers that it holds row ids.
 * fj_join_host: *out_keys / *out_vals are the position arrays (*out_vals = NULL with ANTI).  Refused up front, before any device
 * work: materialize = 0, and with LEFT_OUTER or ANTI everything those flags refuse (FJ_ALGO_MANY_TO_MANY among it).  The multi-GPU
 * and stream joins take no algo word: they have no row-id form. */
#define FJ_ALGO_ROW_IDS 0x80
/* EXTENSION (no reference counterpart; csrc/fj_outer.hip): OR this into `algo` together with a base value (ADAPTIVE, SCALAR or RADIX:
 * the partitioned plan or the global HBM table exactly as for FJ_ALGO_LEFT_OUTER) and optionally FJ_ALGO_ROW_IDS for the full outer
 * join, fused into ONE call and one set of partition passes.  N:1 semantics as everywhere.  materialize = 1 only; d_out_keys and
 * d_out_vals (8-byte aligned) hold >= np + nb rows (room for any result: the caller trims).
 * With this flag out_count points to TWO words: out_count[0] = m, out_count[1] = r, and np + r rows are written in three ranges:
 *   [0, m)        matched (probe_key, build_value), a duplicated build key with its FIRST occurrence's value
 *                 (FJ_ALGO_ROW_IDS: probe position, build position of the first occurrence)
 *   [m, np)       unmatched probe keys, value 0                       (FJ_ALGO_ROW_IDS: probe position, UINT64_MAX)
 *   [np, np + r)  (build_key, build_value) of EVERY build row whose key is not among the probe keys, all copies of a duplicated
 *                 key included                                       (FJ_ALGO_ROW_IDS: UINT64_MAX, build position)
 * Rows [0, np) are what FJ_ALGO_LEFT_OUTER writes for the same inputs; order within each range unspecified.  bloom is ignored; never
 * a pending result for fj_emit_pairs (a result that was pending is dropped).  fj_join_host: out_count likewise points to two words,
 * *out_keys / *out_vals are malloc'ed arrays of np + r rows.  fj_timings: emit_ms is the sweep that appends the third range.
 * Refused up front, before any device work: combined with FJ_ALGO_LEFT_OUTER, FJ_ALGO_ANTI or FJ_ALGO_MANY_TO_MANY; materialize = 0;
 * an output capacity below np + nb; NULL or misaligned output buffers; d_build_vals == NULL without FJ_ALGO_ROW_IDS. */
#define FJ_ALGO_FULL_OUTER 0x100
/* EXTENSION (no reference counterpart; csrc/fj_many.hip): a MODIFIER - OR it into `algo` together with FJ_ALGO_LEFT_OUTER or
 * FJ_ALGO_FULL_OUTER (and optionally FJ_ALGO_ROW_IDS) and the outer join keeps EVERY copy of a duplicated build key (SQL semantics,
 * what FJ_ALGO_MANY_TO_MANY is to the inner join): a probe row yields one output row per build row with its key, and one row with
 * the filler when there is none.  materialize = 1 only.  Partitioned plan only, like FJ_ALGO_MANY_TO_MANY: the base value (ADAPTIVE,
 * SCALAR or RADIX) is accepted and never selects the HBM table, bloom is ignored, and a final partition of more than 4096 build rows
 * is refused with the same error (the context stays usable) - whatever the option "mm_heavy_keys" says: it serves the inner form
 * only - unless the option "mm_heavy_outer" is 1 (below): then such a partition is joined in tiles of at most 4096 build rows, in
 * every form of the call, with the contract stated here.  (Across the build tiles a probe row's "no partner" verdict is combined in a
 * bitmap per probe row, which a sweep over the oversized partitions' probe rows reads: csrc/fj_many.hip.)
 * With this flag out_count points to THREE words, for both forms: out_count[0] = P, the matched pairs (what the many-to-many inner
 * join counts), out_count[1] = r, the build rows whose key no probe row has (0 with FJ_ALGO_LEFT_OUTER), out_count[2] = u, the probe
 * rows without a partner (what the counting anti join returns).  P + u + r rows are written, in three ranges:
 *   [0, P)             (probe_key, build_value) of every pair                (FJ_ALGO_ROW_IDS: probe position, build position)
 *   [P, P + u)         unmatched probe keys, value 0                         (FJ_ALGO_ROW_IDS: probe position, UINT64_MAX)
 *   [P + u, P + u + r) (FULL only) (build_key, build_value), every copy      (FJ_ALGO_ROW_IDS: UINT64_MAX, build position)
 * Order within each range unspecified.  The result's size is not known up front, so the two-phase rule of the materialising joins
 * (fj_join_device below) applies unchanged: with d_out_keys == NULL the call counts, fills the three words and leaves ONE pending
 * result on the context; fj_emit_pairs writes all P + u + r rows into buffers of at least that capacity.  With buffers and
 * out_capacity >= P + u + r both steps happen in the one call.  fj_timings: emit_ms covers the emitting pass and the sweep that
 * appends the third range.  fj_join_host: out_count likewise three words, *out_keys / *out_vals malloc'ed arrays of P + u + r rows.
 * An empty side needs no join: nb == 0 gives P = r = 0, u = np; np == 0 gives P = u = 0 and, for FULL, r = nb.
 * Refused up front, before any device work: the flag without FJ_ALGO_LEFT_OUTER or FJ_ALGO_FULL_OUTER (an unknown algo: the inner
 * form is FJ_ALGO_MANY_TO_MANY), or with FJ_ALGO_ANTI (an anti join has no copies to keep) or FJ_ALGO_MANY_TO_MANY; materialize = 0;
 * out_count == NULL; misaligned output buffers; d_build_vals == NULL without FJ_ALGO_ROW_IDS. */
#define FJ_ALGO_ALL_COPIES 0x200
/* EXTENSION (no reference counterpart; csrc/fj_aligned.hip): OR this into `algo` together with a base value (ADAPTIVE, SCALAR or RADIX:
 * the partitioned plan or the global HBM table exactly as for FJ_ALGO_LEFT_OUTER) and optionally FJ_ALGO_ROW_IDS for a PROBE-ORDER
 * join: one output row per probe row, AT the probe row's position - a dictionary lookup, a foreign-key column, an isin mask, a mark
 * join.  N:1 semantics as everywhere: a duplicated build key answers with its FIRST occurrence, on every path.  materialize = 1 only;
 * bloom is ignored.  With np probe rows:
 *   d_out_vals   optional; 8-byte aligned, np words: d_out_vals[i] = the build value of the first occurrence of d_probe_keys[i], 0 when
 *                the key has no partner.  With FJ_ALGO_ROW_IDS: that build row's position, UINT64_MAX when there is none; d_build_vals
 *                may then be NULL and is never read.
 *   d_out_keys   optional; no alignment asked, np BYTES (the parameter is reused as a byte pointer - there is no key to return, row i
 *                IS probe row i): ((uint8_t*)d_out_keys)[i] = 1 if probe row i has a partner, else 0.
 * At least one of the two is non-NULL; with the mask alone d_build_vals may be NULL (the semi / mark form).  *out_count = m, the probe
 * rows with a partner (what the counting join returns).  out_capacity >= np.  Every one of the np positions is written exactly once
 * per launch, nothing at or beyond row np (byte np of the mask) is touched, and the caller need not clear anything.  nb == 0: zeros
 * (FJ_ALGO_ROW_IDS: all ones), a zero mask, m = 0; np == 0: nothing happens.  Never a pending result for fj_emit_pairs (a result that
 * was pending is dropped).  fj_join_host: *out_vals is a malloc'ed array of np words, *out_keys one of np bytes; either pointer may be
 * NULL to drop that output.  fj_timings as for FJ_ALGO_LEFT_OUTER; emit_ms = 0.
 * Refused up front, before any device work: combined with FJ_ALGO_MANY_TO_MANY, FJ_ALGO_LEFT_OUTER, FJ_ALGO_ANTI, FJ_ALGO_FULL_OUTER or
 * FJ_ALGO_ALL_COPIES; materialize = 0; both outputs NULL; an output capacity below np; a misaligned d_out_vals; d_out_vals with
 * d_build_vals == NULL and no FJ_ALGO_ROW_IDS. */
#define FJ_ALGO_PROBE_ORDER 0x800
/* EXTENSION (no reference counterpart; csrc/fj_group.hip): OR this into `algo` together with a base value (ADAPTIVE, SCALAR or RADIX:
 * the partitioned plan or the global HBM table exactly as for FJ_ALGO_PROBE_ORDER) and nothing else for a BUILD-ORDER aggregate join
 * (a "group join"): one output word per BUILD row, AT the build row's position - orders per customer, the degree of every vertex, a
 * histogram over a dictionary - without the pairs in between.  materialize = 1 only; bloom is ignored.  With nb build rows and np
 * probe rows:
 *   d_build_vals optional; REUSED AS THE PROBE SIDE'S VALUE COLUMN: np words (not nb), one per probe row, 16-byte aligned like every
 *                input.  The build side has no value column in this join (its payload is the row's position).  NULL: counts only.
 *   d_out_keys   optional; 8-byte aligned, nb words: d_out_keys[i] = the number of probe rows whose key equals d_build_keys[i].
 *   d_out_vals   optional; 8-byte aligned, nb words: d_out_vals[i] = the sum, modulo 2^64, of d_build_vals[j] over those probe rows j,
 *                0 when there are none.  Needs a non-NULL d_build_vals.
 * At least one of the two is non-NULL.  Every copy of a duplicated build key receives the aggregate of that key.  *out_count = P, the
 * sum of all counts: the number of pairs the FJ_ALGO_MANY_TO_MANY inner join counts for the same inputs.  out_capacity >= nb.  Every
 * one of the nb positions of a requested output is defined after the call (the library zeroes what it accumulates into; the caller
 * need not clear anything), nothing at or beyond word nb is touched.  np == 0: zeros, P = 0; nb == 0: nothing is written, P = 0.
 * Never a pending result for fj_emit_pairs (a result that was pending is dropped).  fj_join_host: build_vals is the probe value column
 * of np words; *out_keys / *out_vals are malloc'ed arrays of nb words, either pointer may be NULL to drop that output.  fj_timings as
 * for FJ_ALGO_PROBE_ORDER; emit_ms = 0.
 * Refused up front, before any device work: combined with any other flag (FJ_ALGO_ROW_IDS and FJ_ALGO_PROBE_ORDER included);
 * materialize = 0; both outputs NULL; an output capacity below nb; a misaligned output; d_out_vals with d_build_vals == NULL. */
#define FJ_ALGO_BUILD_ORDER 0x1000
/* EXTENSION: modifiers of FJ_ALGO_BUILD_ORDER (and of FJ_ALGO_GROUP_BY below; without either each of them is an unknown algo).  FJ_ALGO_AGG_MIN /
 * FJ_ALGO_AGG_MAX: d_out_vals[i] = the MINIMUM / MAXIMUM, instead of the sum, of d_build_vals[j] over the probe rows j whose key equals
 * d_build_keys[i] ("latest order per customer", "cheapest offer per product").  The words are compared as uint64, or as
 * two's-complement int64 with FJ_ALGO_AGG_SIGNED.  A build row without a partner receives the aggregate's identity:
 *   unsigned min UINT64_MAX | signed min INT64_MAX | unsigned max 0 | signed max INT64_MIN
 * A key whose true aggregate EQUALS the identity cannot be told from "no partner" in d_out_vals alone: ask for the counts (d_out_keys)
 * in the same call - a row has a partner exactly when its count is non-zero.  Everything else is as for the sum: d_out_keys optional
 * and unchanged (nb counts), every copy of a duplicated build key receives the key's aggregate, *out_count = P, every requested word
 * below nb is defined by the call alone whatever the buffer held (the library fills what it combines into; no pass over the outputs
 * afterwards), nothing at or beyond word nb is touched, never a pending result.  np == 0: the identity in every row of d_out_vals,
 * zero counts, P = 0; nb == 0: nothing is written.  fj_join_host: *out_vals is the malloc'ed array of nb aggregates.
 * Refused up front, before any device work, in addition to what FJ_ALGO_BUILD_ORDER refuses: FJ_ALGO_AGG_MIN together with
 * FJ_ALGO_AGG_MAX (one aggregate per call: call twice); FJ_ALGO_AGG_SIGNED without either (the sum is taken modulo 2^64 and has no
 * sign); FJ_ALGO_AGG_MIN / FJ_ALGO_AGG_MAX with d_out_vals == NULL (the counts alone are the plain count form). */
#define FJ_ALGO_AGG_MIN    0x4000
#define FJ_ALGO_AGG_MAX    0x8000
#define FJ_ALGO_AGG_SIGNED 0x10000
/* EXTENSION: one more modifier of FJ_ALGO_BUILD_ORDER and FJ_ALGO_GROUP_BY (without either an unknown algo), the FJ_ALGO_REUSE_BUILD and
 * FJ_ALGO_ACCUMULATE combinations of the former included.  FJ_ALGO_AGG_FLOAT: the value column and the values output hold IEEE-754
 * binary64 ("double") numbers in their uint64_t slots - d_build_vals (the relation's value column under FJ_ALGO_GROUP_BY, the PROBE
 * side's under FJ_ALGO_BUILD_ORDER) and d_out_vals; the counts in d_out_keys stay integers.  Alone it is the float SUM, with
 * FJ_ALGO_AGG_MIN / FJ_ALGO_AGG_MAX the float minimum / maximum.  A build row without a partner receives the aggregate's identity:
 *   sum +0.0 | min +infinity | max -infinity
 * and FJ_ALGO_ACCUMULATE combines into what a float64 output holds.  Everything else - the outputs' layout, *out_count, the
 * first-occurrence rule of the prepared side, the fallback - is that of the integer forms.
 *   The sum is accumulated with atomic adds in an UNSPECIFIED ORDER: it can differ in its last bits from run to run and from a
 *   sequential sum (it is exact, and then reproducible, whenever every partial sum is representable).
 *   Min / max compare as numbers; which zero comes back for a group that holds both -0.0 and +0.0 is unspecified.
 *   A NaN makes the sum of ITS group NaN and the minimum / maximum of its group unspecified; no other group is affected.
 * d_out_vals (and a running aggregate under FJ_ALGO_ACCUMULATE) must be ordinary device memory: the float sum is a hardware f64 atomic.
 * fj_join_host stages through device buffers of its own and returns malloc'ed arrays as for the integer forms.
 * Refused up front, before any device work, in addition to what the base flag refuses: combined with FJ_ALGO_AGG_SIGNED (a double has
 * its own sign), with FJ_ALGO_ROW_IDS or FJ_ALGO_INVERSE (positions and ids are integers); without a value column (d_build_vals ==
 * NULL: the count forms have no float form); under FJ_ALGO_BUILD_ORDER with d_out_vals == NULL. */
#define FJ_ALGO_AGG_FLOAT  0x2000000
/* EXTENSION (no reference counterpart; csrc/fj_groupby.hip): OR this into `algo` together with a base value (ADAPTIVE, SCALAR or RADIX:
 * the partitioned plan or the global HBM table exactly as for FJ_ALGO_BUILD_ORDER) for a GROUP BY / DISTINCT on ONE relation: the
 * list of groups that FJ_ALGO_BUILD_ORDER asks its caller for, and one aggregate per group.  The relation is passed as the build side:
 *   d_build_keys  nb keys.
 *   d_build_vals  optional; nb words, the value column.
 *   d_probe_keys  must be NULL and np 0: there is no second relation.
 * *out_count = g, the number of distinct keys.  The result has one row per group, g rows, in an unspecified order that both arrays of
 * one call share:
 *   d_out_keys[i] the raw key of group i.
 *   d_out_vals[i] optional (NULL: the keys alone); the group's aggregate -
 *                   no modifier, d_build_vals == NULL:   the group's row count
 *                   no modifier, d_build_vals != NULL:   the sum of the values modulo 2^64
 *                   FJ_ALGO_AGG_MIN / FJ_ALGO_AGG_MAX:   the minimum / maximum, compared as uint64, or as int64 with FJ_ALGO_AGG_SIGNED
 *                                                        (needs d_build_vals; every group has a row, so the identity never appears)
 *                   FJ_ALGO_ROW_IDS:                     the 0-based position of the key's FIRST occurrence in d_build_keys
 *                                                        (d_build_vals is never read)
 * materialize = 1 needs 8-byte aligned outputs and out_capacity >= nb, room for any result; the caller trims to g.  Rows [g, nb) may
 * hold anything afterwards, nothing at or beyond word out_capacity is touched.  materialize = 0 is COUNT(DISTINCT): g alone from a
 * keys-only pass; no output pointer is read and no capacity needed.  nb == 0: g = 0, nothing is written.  bloom is ignored.  Never a
 * pending result for fj_emit_pairs (a result that was pending is dropped).  fj_timings: the relation's passes in build_phase_ms, the
 * kernel in join_ms = probe_phase_ms, emit_ms = 0, fell_back = 1 when a final partition held more distinct keys than the LDS table
 * takes and the call ran again on the HBM table.  fj_join_host: probe_keys NULL, np 0; *out_keys / *out_vals are malloc'ed arrays of
 * exactly g rows, either pointer may be NULL to drop that output.
 * A key that owns a large share of the rows is aggregated by ONE workgroup (a final partition is one work item); the result is exact
 * at any distribution, the time is not flat.
 * Refused up front, before any device work: combined with FJ_ALGO_MANY_TO_MANY, FJ_ALGO_LEFT_OUTER, FJ_ALGO_ANTI, FJ_ALGO_FULL_OUTER,
 * FJ_ALGO_ALL_COPIES, FJ_ALGO_PROBE_ORDER or FJ_ALGO_BUILD_ORDER; a probe side; FJ_ALGO_AGG_MIN with FJ_ALGO_AGG_MAX; FJ_ALGO_AGG_SIGNED
 * without either; FJ_ALGO_AGG_MIN / FJ_ALGO_AGG_MAX with d_build_vals == NULL (and nb > 0); FJ_ALGO_ROW_IDS with either of them or with
 * materialize = 0; materialize = 1 with d_out_keys == NULL (and nb > 0), an output capacity below nb or a misaligned output. */
#define FJ_ALGO_GROUP_BY   0x40000
/* EXTENSION: a modifier of FJ_ALGO_GROUP_BY (without it an unknown algo; csrc/fj_groupby.hip): the INVERSE of the group-by, what
 * np.unique(return_inverse=True), torch.unique(return_inverse=True) and pandas.factorize return - the group of EVERY row.  OR it into
 * `algo` together with FJ_ALGO_GROUP_BY and a base value (ADAPTIVE, SCALAR or RADIX), materialize = 1:
 *   d_out_keys[0 .. g) the distinct raw keys in an unspecified order, exactly as without the flag; rows [g, nb) may hold anything.
 *   d_out_vals[i]      for every i < nb: the group id of build row i, AT row i's position - a uint64 in [0, g) with
 *                      d_out_keys[d_out_vals[i]] == d_build_keys[i].
 * *out_count = g.  out_capacity >= nb covers both arrays; both are required (nb > 0) and 8-byte aligned.  All nb words of d_out_vals are
 * defined by the call alone, whatever the buffer held before; nothing at or beyond word out_capacity of either array is touched.
 * d_build_vals is never read and may be NULL.  nb == 0: g = 0, nothing is written.  bloom is ignored.  Never a pending result for
 * fj_emit_pairs.  The ids are the dictionary encoding of the key column: with them the relation is grouped ONCE, and every further
 * aggregate (an average, a variance, several value columns) is a scatter of the caller's over ids in [0, g).  The order of the groups
 * is the cursor's: neither sorted nor by first occurrence.  fj_timings as for FJ_ALGO_GROUP_BY: the pass over the rows that writes the
 * ids counts into join_ms = probe_phase_ms, emit_ms = 0, fell_back as there (the re-run on the HBM table writes all nb ids again).
 * fj_join_host: *out_keys is a malloc'ed array of exactly g rows, *out_vals one of exactly nb rows; either pointer may be NULL to drop
 * that output (out_vals == NULL runs the plain distinct form).
 * Refused up front, before any device work, in addition to what FJ_ALGO_GROUP_BY refuses: combined with FJ_ALGO_AGG_MIN,
 * FJ_ALGO_AGG_MAX or FJ_ALGO_AGG_SIGNED (no aggregate in the same call) or with FJ_ALGO_ROW_IDS (d_out_vals is taken: one per-call
 * output); materialize = 0; fj_join_device with d_out_keys == NULL or d_out_vals == NULL (and nb > 0). */
#define FJ_ALGO_INVERSE    0x100000
/* EXTENSION: modifiers of FJ_ALGO_PROBE_ORDER (without it each of them is an unknown algo; csrc/fj_prepared.hip) for a PREPARED build
 * side: one dictionary or dimension table probed by many batches - a foreign-key column arriving in morsels, id remapping per training
 * step, an IN list applied to every partition of a fact table - pays its partition passes and its first-occurrence logic once.
 *
 * FJ_ALGO_RETAIN_BUILD: the call does what the same call does without the flag - same outputs, *out_count = m - and in addition leaves
 * the build side prepared on the context: deduplicated to the first occurrence of every key, grouped by the final partitions of the
 * plan, in device memory the context owns OUTSIDE its workspace.  The build keys are copied, the values when d_build_vals is non-NULL,
 * the first-occurrence positions always: the caller may overwrite or free its build arrays as soon as the call returns.  np == 0: the
 * call only prepares - both outputs may be NULL, *out_count = g, the number of distinct build keys.  The base value (ADAPTIVE, SCALAR
 * or RADIX) and the options "plan_target_keys", "radix_threshold" and "scalar_hbm_table" are read NOW and choose between the partitioned
 * form and the HBM-table form exactly as for the one-shot call; the plan and hash_top_bits are stored with the side.  A partition of
 * more distinct keys than the LDS table takes prepares the HBM-table form instead (fj_timings: fell_back = 1 in this call).  nb == 0
 * prepares an empty side, on which every lookup misses, and frees what was held.  fj_timings: the preparation in build_phase_ms.
 * A context holds ONE prepared side: the next FJ_ALGO_RETAIN_BUILD call replaces it (one that fails after its argument checks leaves
 * none) and fj_ctx_destroy frees it.  Nothing else touches it - not another join of any kind on the context, not fj_emit_pairs, not
 * fj_ctx_trim - fj_ctx_workspace_bytes does not count it, and it is not the context's pending result.  Memory: 16 bytes per build row,
 * 24 with values, and 16 bytes per final partition; the HBM-table form 16 bytes per table slot (2 to 4 slots per row) and 8 bytes per
 * row with values.
 *
 * FJ_ALGO_REUSE_BUILD: d_build_keys and d_build_vals must be NULL and nb 0; the probe side runs against the context's prepared side.
 * The outputs are exactly those of FJ_ALGO_PROBE_ORDER on the build side that was prepared: d_out_vals[i] the first occurrence's build
 * value, 0 on a miss (FJ_ALGO_ROW_IDS: its position, UINT64_MAX on a miss), the byte mask in d_out_keys, either or both, *out_count = m;
 * every one of the np positions is written exactly once, nothing at or beyond np is touched, np == 0 does nothing.  The base value
 * must be 0..2 and is otherwise ignored: the stored plan decides.  The context's workspace serves the probe side's passes only.
 * fj_timings: build_phase_ms = 0; passes, radix_bits, partitions and path are those of the prepared side.
 *
 * Refused up front, before any device work: either flag without FJ_ALGO_PROBE_ORDER (unknown algo) or with anything it refuses; both
 * flags together; FJ_ALGO_REUSE_BUILD with a build side (a non-NULL d_build_keys or d_build_vals, nb != 0).  Refused on the context,
 * which stays usable: FJ_ALGO_REUSE_BUILD with no prepared side, with another hash_top_bits than the prepared side's, or asking for
 * values (d_out_vals without FJ_ALGO_ROW_IDS) from a side prepared without d_build_vals - the mask and the row-id form always work.
 * fj_join_host refuses both flags (its internal context is shared by every host-buffer call of the process): use fj_join_device on a
 * context of your own. */
#define FJ_ALGO_RETAIN_BUILD 0x400000
#define FJ_ALGO_REUSE_BUILD  0x800000
/* EXTENSION (csrc/fj_prepared.hip): FJ_ALGO_BUILD_ORDER | FJ_ALGO_REUSE_BUILD, plus a base value 0..2 and optionally FJ_ALGO_AGG_MIN /
 * FJ_ALGO_AGG_MAX / FJ_ALGO_AGG_SIGNED, through fj_join_device: the build-order aggregate join of the probe side onto the context's
 * PREPARED build side - orders per customer, revenue per product, latest event per user over a fact column that arrives in morsels,
 * without the build side's passes in every call.  With NB = the number of rows the side was prepared from:
 *   d_build_keys must be NULL and nb 0 (the context's prepared side is aggregated onto).
 *   d_build_vals the PROBE side's value column, np words, exactly as in the one-shot FJ_ALGO_BUILD_ORDER call.  NULL: counts only.
 *   d_out_keys   optional; 8-byte aligned, NB words: the counts.          d_out_vals  optional; NB words: the sums / minima / maxima.
 *   out_capacity >= NB.
 * FIRST-OCCURRENCE RULE: the prepared side is deduplicated to first occurrences, so the aggregate of a key lands AT THE POSITION OF
 * THE KEY'S FIRST BUILD ROW; every further copy of a duplicated build key holds 0 (count, sum) or the aggregate's identity (min /
 * max).  This is the rule of the prepared side's other forms (FJ_ALGO_ROW_IDS names the first row) and DELIBERATELY DIFFERS from the
 * one-shot FJ_ALGO_BUILD_ORDER call, where every copy carries the aggregate.  On distinct build keys the two calls agree bit for bit.
 * *out_count = the probe rows of THIS call that have a partner.  Every requested word below NB is defined by the call, nothing at or
 * beyond NB is touched; never a pending result.  fj_timings: build_phase_ms = 0; passes, radix_bits, partitions and path are the
 * prepared side's.  A side prepared without d_build_vals serves every form (no build value is read); a side prepared from nb == 0
 * writes nothing and returns 0.  On the HBM-table form every hit is a global atomic at the output word: a hot key serialises there.
 *
 * FJ_ALGO_ACCUMULATE: a modifier of that combination ONLY (anywhere else an unknown algo).  Without it the library fills the outputs
 * first, as the one-shot call does (zeros; the identity for min / max).  With it the call does NOT fill: it combines into whatever the
 * outputs hold - add for counts and sums, the typed min / max otherwise - so N morsels make ONE running aggregate in N calls on the
 * same buffers.  The flag applies to every output of the call; np == 0 touches nothing.
 *
 * Refused up front, before any device work: FJ_ALGO_BUILD_ORDER | FJ_ALGO_RETAIN_BUILD (an unknown algo); FJ_ALGO_ACCUMULATE without
 * both FJ_ALGO_BUILD_ORDER and FJ_ALGO_REUSE_BUILD (an unknown algo); a build side (non-NULL d_build_keys or nb != 0 - d_build_vals is
 * the probe value column here and is no build side); everything FJ_ALGO_BUILD_ORDER refuses.  Refused on the context, which stays
 * usable: no prepared side, another hash_top_bits than the prepared side's, out_capacity < NB.  fj_join_host refuses the combination
 * with and without FJ_ALGO_ACCUMULATE: use fj_join_device on a context of your own. */
#define FJ_ALGO_ACCUMULATE 0x1000000
/* EXTENSION: a modifier of FJ_ALGO_GROUP_BY (without it an unknown algo; csrc/fj_groupby_multi.hip): the row count, the sum, the
 * minimum AND the maximum of the value column in ONE call - SELECT k, COUNT(*), SUM(v), MIN(v), MAX(v) ... GROUP BY k - where the
 * single forms take four calls, four trips of the relation through the partition passes and an alignment by key.  OR it into `algo`
 * together with FJ_ALGO_GROUP_BY and a base value (ADAPTIVE, SCALAR or RADIX), optionally with FJ_ALGO_AGG_SIGNED or with
 * FJ_ALGO_AGG_FLOAT, materialize = 1:
 *   d_build_keys / d_build_vals   the relation and its value column, nb words each; both required (nb > 0).
 *   d_out_keys[0 .. g)            the distinct raw keys in an unspecified order, exactly as without the flag.
 *   d_out_vals                    FOUR planes of out_capacity words each: plane j starts at d_out_vals + j * out_capacity, and row i of
 *                                 every plane belongs to d_out_keys[i] -
 *                                   plane 0  the group's row count (uint64)
 *                                   plane 1  the sum modulo 2^64, or the IEEE-754 binary64 sum with FJ_ALGO_AGG_FLOAT
 *                                   plane 2  the minimum
 *                                   plane 3  the maximum
 *                                 compared as uint64, as int64 with FJ_ALGO_AGG_SIGNED, as numbers with FJ_ALGO_AGG_FLOAT (NaN and
 *                                 -0.0 / +0.0 as in the float forms of FJ_ALGO_AGG_MIN / FJ_ALGO_AGG_MAX).
 * *out_count = g.  Every group has a row, so no identity appears.  out_capacity may be ANY value >= 1: a caller who knows a bound on
 * the number of groups need not hold five arrays of nb words.  When g > out_capacity the call fails AFTER the device work with an error
 * that states g and the capacity, and *out_count = g; the buffers' contents are then unspecified and the context stays usable.  Nothing at or beyond word
 * out_capacity of d_out_keys or word 4 * out_capacity of d_out_vals is ever touched.  nb == 0: g = 0, nothing is written.  bloom is
 * ignored.  Never a pending result for fj_emit_pairs.  fj_timings as for FJ_ALGO_GROUP_BY; fell_back = 1 when a final partition held
 * more distinct keys than this form's LDS table takes (3840) and the call ran again on the HBM table.  fj_join_host: *out_keys is a
 * malloc'ed array of g words, *out_vals one of 4 * g words, plane-major with stride g; both pointers are required.
 * Refused up front, before any device work, in addition to what FJ_ALGO_GROUP_BY refuses: combined with FJ_ALGO_AGG_MIN or
 * FJ_ALGO_AGG_MAX (it holds both), with FJ_ALGO_ROW_IDS or FJ_ALGO_INVERSE, with FJ_ALGO_AGG_SIGNED and FJ_ALGO_AGG_FLOAT together;
 * materialize = 0; d_build_vals, d_out_keys or d_out_vals == NULL (and nb > 0); out_capacity == 0 (and nb > 0); a misaligned output.
 * With FJ_ALGO_KEY_PAIR beside it (and without FJ_ALGO_INVERSE) the key is a PAIR of columns and d_out_vals holds FIVE planes: the
 * form FJ_ALGO_KEY_PAIR | FJ_ALGO_AGG_ALL, described under FJ_ALGO_KEY_PAIR. */
#define FJ_ALGO_AGG_ALL    0x4000000
/* EXTENSION: a modifier of FJ_ALGO_GROUP_BY (without it an unknown algo; csrc/fj_groupby_arg.hip): the ROW that holds each group's
 * minimum or maximum - pandas idxmin / idxmax, SQL arg_min / arg_max - so that the caller can gather the row's other columns.  OR it
 * into `algo` together with FJ_ALGO_GROUP_BY, a base value (ADAPTIVE, SCALAR or RADIX) and exactly one of FJ_ALGO_AGG_MIN and
 * FJ_ALGO_AGG_MAX, optionally with FJ_ALGO_AGG_SIGNED or with FJ_ALGO_AGG_FLOAT, materialize = 1:
 *   d_build_keys / d_build_vals   the relation and its value column, nb words each; both required (nb > 0).
 *   d_out_keys[0 .. g)            the distinct raw keys in an unspecified order, exactly as without the flag.
 *   d_out_vals                    TWO planes of out_capacity words each, row i of both belonging to d_out_keys[i] -
 *                                   plane 0  (d_out_vals)                 the row index: the SMALLEST i with d_build_vals[i] equal to
 *                                            the extreme of the key's rows, for the minimum and the maximum alike (first occurrence)
 *                                   plane 1  (d_out_vals + out_capacity)  that extreme, what FJ_ALGO_AGG_MIN / FJ_ALGO_AGG_MAX return
 *                                 compared as uint64, as int64 with FJ_ALGO_AGG_SIGNED, as numbers with FJ_ALGO_AGG_FLOAT: -0.0 and
 *                                 +0.0 tie (the smaller index wins; which zero plane 1 holds is unspecified); a group that holds a
 *                                 NaN has an unspecified extreme and an index that is a row of the relation or all ones, and no other
 *                                 group is affected.
 * *out_count = g.  Every group has a row, so every index is a row of the relation - also where the extreme equals the aggregate's
 * identity: no counts are needed to tell such a group apart.  out_capacity >= nb, as for the single forms.  nb == 0: g = 0, nothing is
 * written.  bloom is ignored.  Never a pending result for fj_emit_pairs.  fj_timings as for FJ_ALGO_GROUP_BY; fell_back = 1 when a
 * final partition held more distinct keys than this form's LDS table takes (3840) and the call ran again on the HBM table.
 * fj_join_host: *out_keys is a malloc'ed array of g words, *out_vals one of 2 * g words, plane-major with stride g; both required.
 * Refused up front, before any device work, in addition to what FJ_ALGO_GROUP_BY refuses: without FJ_ALGO_AGG_MIN and FJ_ALGO_AGG_MAX
 * or with both; combined with FJ_ALGO_ROW_IDS, FJ_ALGO_INVERSE or FJ_ALGO_AGG_ALL, with FJ_ALGO_AGG_SIGNED and FJ_ALGO_AGG_FLOAT
 * together; materialize = 0; d_build_vals, d_out_keys or d_out_vals == NULL (and nb > 0); out_capacity < nb; a misaligned output. */
#define FJ_ALGO_AGG_ARG    0x8000000
/* EXTENSION: a modifier of FJ_ALGO_GROUP_BY | FJ_ALGO_AGG_ALL (in every other combination an unknown algo; csrc/fj_groupby_merge.hip):
 * MERGE partial group-by results.  The build side is not a relation but nb PARTIAL rows - a key and beside it a row count, a sum, a
 * minimum and a maximum, what FJ_ALGO_AGG_ALL returned for one batch, one shard or one slice of a relation - and the rows that share a
 * key are combined into one.  OR it into `algo` together with FJ_ALGO_GROUP_BY, FJ_ALGO_AGG_ALL and a base value (ADAPTIVE, SCALAR or
 * RADIX), optionally with FJ_ALGO_AGG_SIGNED or with FJ_ALGO_AGG_FLOAT, materialize = 1:
 *   d_build_keys                  nb keys, one per partial row.
 *   d_build_vals                  FOUR planes of nb words at stride nb - count, sum, min, max: the layout FJ_ALGO_AGG_ALL writes, with
 *                                 stride nb in place of out_capacity.  Required (nb > 0).
 *   d_out_keys, d_out_vals        exactly as for FJ_ALGO_AGG_ALL: the g distinct keys and four planes of out_capacity words -
 *                                   plane 0  the sum of the rows' counts modulo 2^64
 *                                   plane 1  the sum of the rows' sums: modulo 2^64, or binary64 atomic adds in an unspecified order
 *                                            with FJ_ALGO_AGG_FLOAT
 *                                   plane 2  the minimum of the rows' minima
 *                                   plane 3  the maximum of the rows' maxima
 *                                 in the kind's order (uint64, int64 with FJ_ALGO_AGG_SIGNED, numbers with FJ_ALGO_AGG_FLOAT; NaN and
 *                                 -0.0 / +0.0 as for FJ_ALGO_AGG_ALL).
 * A partial row with count 0 whose other planes hold the aggregates' identities (sum 0 / +0.0; min all ones, INT64_MAX or +inf; max 0,
 * INT64_MIN or -inf) is legal: it is what FJ_ALGO_BUILD_ORDER leaves for a build row without a partner.  Its key becomes a group of the
 * result, with count 0 unless another row of that key says otherwise.
 * *out_count = g.  out_capacity may be ANY value >= 1; g > out_capacity fails AFTER the device work with an error that states g, with
 * *out_count = g, and the context stays usable.  nb == 0: g = 0, no buffer is needed.  bloom is ignored.  Never a pending result.
 * fj_timings as for FJ_ALGO_AGG_ALL; fell_back = 1 when a final partition held more distinct keys than this form's LDS table takes
 * (1920) and the call ran again on the HBM table.  fj_join_host: build_vals is 4 * nb words; the outputs as for FJ_ALGO_AGG_ALL.
 * Refused up front, before any device work: everything FJ_ALGO_AGG_ALL refuses (FJ_ALGO_AGG_MIN, FJ_ALGO_AGG_MAX, FJ_ALGO_ROW_IDS,
 * FJ_ALGO_INVERSE, FJ_ALGO_AGG_SIGNED with FJ_ALGO_AGG_FLOAT, materialize = 0, a NULL d_build_vals, d_out_keys or d_out_vals with
 * nb > 0, out_capacity == 0 with nb > 0, a misaligned buffer), FJ_ALGO_AGG_ARG beside it, and whatever FJ_ALGO_GROUP_BY refuses. */
#define FJ_ALGO_AGG_MERGE  0x10000000
/* EXTENSION: a modifier of FJ_ALGO_GROUP_BY | FJ_ALGO_INVERSE, or of FJ_ALGO_GROUP_BY | FJ_ALGO_AGG_ALL (the second form, below; in every
 * other combination refused; csrc/fj_groupby_pair.hip): the key of
 * the group-by is a PAIR of columns - (customer, day), (src, dst), (tenant, user).  OR it into `algo` together with FJ_ALGO_GROUP_BY,
 * FJ_ALGO_INVERSE and a base value (ADAPTIVE, SCALAR or RADIX), materialize = 1:
 *   d_build_keys       column A, nb words.
 *   d_build_vals       column B, nb words: a KEY column here.  Required (nb > 0), 16-byte aligned.
 * Rows i and j belong to one group iff A[i] == A[j] && B[i] == B[j], compared as 64-bit words.
 *   d_out_vals[i]      for every i < nb: the group id of row i, AT row i's position - a uint64 in [0, g), as for FJ_ALGO_INVERSE.
 *   d_out_keys[r]      for r < g: NOT a key but the ROW INDEX of group r's first occurrence - the smallest i whose pair is the group's.
 *                      The caller gathers A[idx], B[idx] and any other column with it; rows [g, nb) may hold anything.
 * *out_count = g.  out_capacity >= nb covers both arrays; both are required (nb > 0) and 8-byte aligned; nothing at or beyond word
 * out_capacity of either is touched.  nb == 0: g = 0, nothing is written.  nb <= 2^40.  bloom is ignored.  Never a pending result.
 * The ids are ordinary dense keys: every function of this header takes them as its one key column, and a third column folds onto them
 * with another call (ids, C).  The result is deterministic up to the order of the groups, which is the cursor's.
 * The partition passes run over ONE combined word per row, a ^ fj_key_mix64(b ^ 0x9E3779B97F4A7C15).  That map is not injective: every
 * row's pair is compared with its group's first row, and where two distinct pairs share a word the call runs again on an HBM table
 * that compares pairs.  The result is exact for every input.
 * fj_timings as for FJ_ALGO_INVERSE; fell_back = 1 when the call ran again on the HBM table (a final partition of more than 7680
 * distinct combined words, or two pairs on one word).
 * fj_join_host: build_vals is column B; *out_keys is a malloc'ed array of exactly g row indices, *out_vals one of exactly nb ids; a
 * NULL pointer drops that output.
 * Refused up front, before any device work: the flag without FJ_ALGO_GROUP_BY (an unknown algo); with it but without FJ_ALGO_INVERSE
 * or FJ_ALGO_AGG_ALL (the form below); everything FJ_ALGO_INVERSE and FJ_ALGO_GROUP_BY refuse; a NULL d_build_vals with nb > 0; nb > 2^40.
 *
 * FJ_ALGO_KEY_PAIR | FJ_ALGO_AGG_ALL (csrc/fj_groupby_pair_agg.hip): the pairs themselves with FOUR aggregates of a third column -
 * SELECT a, b, COUNT(*), SUM(v), MIN(v), MAX(v) ... GROUP BY a, b - in ONE call, without the group ids.  OR both into `algo` together
 * with FJ_ALGO_GROUP_BY and a base value (ADAPTIVE, SCALAR or RADIX), optionally with FJ_ALGO_AGG_SIGNED or with FJ_ALGO_AGG_FLOAT,
 * WITHOUT FJ_ALGO_INVERSE, materialize = 1:
 *   d_build_keys       column A, nb words.
 *   d_build_vals       column B, nb words: a KEY column.
 *   d_probe_keys       the VALUE column V, nb words, and np == nb: the one form of FJ_ALGO_GROUP_BY that takes a third column.
 *                      All three are required (nb > 0) and 16-byte aligned.  nb <= 2^40.
 *   d_out_keys[r]      for r < g: A of group r.
 *   d_out_vals         FIVE planes of out_capacity words each, row r of every plane belonging to group r -
 *                        plane 0  B of group r
 *                        planes 1 .. 4  the row count, the sum, the minimum and the maximum of V over the group's rows: planes 0 .. 3 of
 *                                 FJ_ALGO_AGG_ALL, with its semantics, kinds, NaN and signed-zero rules
 * *out_count = g; the order of the groups is unspecified.  out_capacity may be ANY value >= 1; g > out_capacity fails AFTER the device
 * work with an error that states g, with *out_count = g, and the context stays usable.  nb == 0: g = 0, nothing is written, no buffer
 * is needed.  bloom is ignored.  Never a pending result.  Exact for every input: a table slot keeps the smallest and the largest b it
 * met, two pairs on one combined word differ in b, and where that shows the call runs again on an HBM table that compares pairs.
 * fj_timings as for FJ_ALGO_AGG_ALL: the combined words and the passes in build_phase_ms, the aggregation in join_ms ==
 * probe_phase_ms, emit_ms = 0; fell_back = 1 when the call ran again on the HBM table (a final partition of more than 1920 distinct
 * combined words, or two pairs on one word).
 * fj_join_host: the same roles - probe_keys is V, np == nb; *out_keys is a malloc'ed array of g words, *out_vals one of 5 * g words,
 * plane-major with stride g; both pointers are required.
 * Refused up front, before any device work: combined with FJ_ALGO_AGG_MIN, FJ_ALGO_AGG_MAX, FJ_ALGO_ROW_IDS, FJ_ALGO_AGG_ARG,
 * FJ_ALGO_AGG_MERGE or FJ_ALGO_GROUP_ROWS (with FJ_ALGO_INVERSE: FJ_ALGO_AGG_ALL's refusal of it); FJ_ALGO_AGG_SIGNED and
 * FJ_ALGO_AGG_FLOAT together; materialize = 0; a NULL A, B, V, d_out_keys or d_out_vals with nb > 0; np != nb; out_capacity == 0 with
 * nb > 0; nb > 2^40; a misaligned buffer; and whatever FJ_ALGO_GROUP_BY refuses but the probe side. */
#define FJ_ALGO_KEY_PAIR   0x20000000
/* EXTENSION: a modifier of FJ_ALGO_GROUP_BY alone (without it an unknown algo; csrc/fj_groupby_rows.hip): the ROWS of every group - the
 * relation's row indices in group-contiguous order and the offset at which every group starts, a CSR of row indices.  What pandas
 * groupby().indices, SQL array_agg and the CSR of an edge list by source are, and what a median, a top-k or any segment reduction per
 * group starts from - without the stable sort of the group ids that FJ_ALGO_INVERSE would need for it.  OR it into `algo` together
 * with FJ_ALGO_GROUP_BY and a base value (ADAPTIVE, SCALAR or RADIX), materialize = 1:
 *   d_build_keys       the relation, nb words.  d_build_vals is never read and may be NULL.
 *   d_out_keys[r]      for r < g: the distinct raw keys; rows [g, nb) may hold anything.
 *   d_out_vals         TWO planes of out_capacity words each, plane-major:
 *     plane 0, words [0, nb): the row indices in group order; every i < nb appears exactly once.
 *     plane 1, words [0, g):  start[r], the first word of plane 0 that belongs to group r.  The starts are strictly increasing,
 *                        start[0] = 0, and group r owns the words [start[r], start[r + 1]) with start[g] = nb implied:
 *                        d_build_keys[plane0[j]] == d_out_keys[r] for every j in that range.
 * *out_count = g.  out_capacity >= nb; d_out_keys and d_out_vals are required (nb > 0) and 8-byte aligned.  The words [nb, out_capacity)
 * of plane 0 are not written, the words [g, out_capacity) of plane 1 may hold anything, nothing at or beyond word out_capacity of
 * d_out_keys or word 2 * out_capacity of d_out_vals is touched.  nb == 0: g = 0, nothing is written.  nb <= 2^40.  bloom is ignored.
 * Never a pending result for fj_emit_pairs.
 * The order of the groups is unspecified, but keys and starts share it.  The order of the rows INSIDE a group is unspecified too and
 * may differ from run to run: an atomic counter per group hands out the places.  A caller that needs the rows of a group ascending
 * sorts inside the groups.
 * fj_timings as for FJ_ALGO_INVERSE: the relation's passes in build_phase_ms, everything behind them - three launches: count, scan,
 * place - in join_ms = probe_phase_ms, emit_ms = 0, fell_back = 1 when a final partition held more than 7680 distinct keys and the
 * call ran again on the HBM table (which defines all nb + g words itself).  A key that owns a large share of the rows is streamed by
 * ONE workgroup, three times; exact at any distribution, the time is not flat.
 * fj_join_host: *out_keys is a malloc'ed array of exactly g keys, *out_vals one of exactly nb + g words - the nb row indices, then the
 * g starts; a NULL pointer drops that output.
 * Refused up front, before any device work: the flag without FJ_ALGO_GROUP_BY (an unknown algo); combined with FJ_ALGO_INVERSE,
 * FJ_ALGO_ROW_IDS, FJ_ALGO_AGG_MIN, FJ_ALGO_AGG_MAX, FJ_ALGO_AGG_SIGNED, FJ_ALGO_AGG_FLOAT, FJ_ALGO_AGG_ALL, FJ_ALGO_AGG_ARG,
 * FJ_ALGO_AGG_MERGE or FJ_ALGO_KEY_PAIR; materialize = 0; fj_join_device with d_out_keys == NULL or d_out_vals == NULL (and nb > 0),
 * out_capacity < nb or a misaligned output; nb > 2^40; and whatever FJ_ALGO_GROUP_BY refuses (a probe side, the join flags). */
#define FJ_ALGO_GROUP_ROWS 0x40000000

typedef struct fj_ctx fj_ctx;

/* Per-call device timings (milliseconds, HIP events on the caller's stream) and plan facts. */
typedef struct fj_timings {
    double total_ms;             /* whole device-resident join: what core_duration_sec reports */
    double build_phase_ms;       /* everything that touches only the build relation            */
    double probe_phase_ms;       /* probe-side partition passes + per-partition build/probe    */
    double join_ms;              /* the join kernel(s) alone (part of probe_phase_ms)          */
    double emit_ms;              /* second (writing) pass of a materialising join              */
    double probe_part_kernel_ms[4]; /* each probe-side partition kernel launch                 */
    double h2d_ms, d2h_ms;       /* host-buffer entry only                                     */
    int path;                    /* 0 = radix + LDS tables, 1 = global table                   */
    int passes;                  /* radix passes run on each relation (k)                      */
    int radix_bits;              /* total partition bits                                       */
    int fell_back;               /* 1 if the radix path overflowed an LDS table and the global path re-ran */
    uint64_t partitions;
    int overlapped;              /* always 0: build_phase_ms and probe_phase_ms are disjoint intervals (the two-stream schedules of
                                    rounds 1-2 are gone; the field keeps the struct layout)                              */
    int lds_retries;             /* 1 if some partitions overflowed the counting join's cuckoo table and were redone on the tagged table;
                                    1 + n if n oversized partitions were re-partitioned alone; FJ_LDS_RETRIES_MM_TILED (no other path
                                    reports it) if a many-to-many join ran partitions of more than 4096 build rows tile by tile
                                    (options "mm_heavy_keys", "mm_heavy_outer") */
#define FJ_LDS_RETRIES_MM_TILED 4096
    /* bloom precheck of the partitioned plan (the *_bloom functions): */
    double filter_ms;            /* the filter kernel between the probe side's passes (part of probe_phase_ms)              */
    uint64_t filter_survivors;   /* probe keys that passed it (hits + false positives); 0 when bloom_level == 0             */
    int bloom_level;             /* 0: no precheck ran; L: the probe side was filtered after its L-th partition pass         */
    int sampled_hit_bp;          /* adaptive_* joins: hit rate (basis points) of the probe-side sample that decided on the precheck; -1: no sample taken */
    int host_streamed;           /* fj_join_host: 1 if the join ran piece by piece under the PCIe copy (h2d_ms then contains it) */
    int reserved3;
} fj_timings;

/* replaces: flash_join.initialize() / initialize_memory_system (hash_join.cpp:596, :639).
 * Selects nothing, allocates nothing; verifies a HIP device is usable. */
int fj_initialize(void);
const char* fj_last_error(void);
int fj_device_count(void);
const char* fj_version(void);
/* The binary interface's version.  It changes whenever a struct of this header changes layout or an entry point its signature; a
 * binding checks it once after loading the library (flash_hash_join_amd/_lib.py does).  Structs the library fills or reads on a
 * caller's behalf (fj_dist_timings, fj_dist_engine_ops) start with a struct_size word the caller sets to sizeof(its struct): the
 * library touches no byte beyond it. */
#define FJ_ABI_VERSION 8
int fj_abi_version(void);

/* Process-wide dispatch options (no reference counterpart; the reference hard-codes 1'000'000 at hash_join.cpp:576).  Initial values:
 * the ONE environment variable FJ_OPTIONS="name=value,name=value" (read once):
 *   "radix_threshold"  - adaptive_* joins use the non-partitioned HBM table below this many build rows (default 0:
 *                        the partitioned driver wins at every size on MI355X);
 *   "scalar_hbm_table" - (the HBM-table path is NOT a fast path: probe 0.05-0.07 of the HBM peak, build by global CAS 20 ms per
 *                        100M rows, profiles/README.md; it exists as the literal form of the reference's scalar algorithm
 *                        and as the fallback for a partition of more than 8128 distinct keys)
 *                        1: the "scalar" functions (FJ_ALGO_SCALAR: hash_join*, hash_join.cpp:383-496, :536-567) keep
 *                        ONE table for the whole build side in HBM, as the reference does in DRAM; 0 (default): they
 *                        run the same partitioned plan as the radix functions (identical results, 2-4x faster here)
 *                        and the HBM table is only the overflow fallback.
 *   "persistent_min_items" - counting joins whose plan has at least this many (partition, probe slice) work items use
 *                        the persistent join kernel (default 8192; a tuning/testing knob).
 *   "bloom_auto"       - 1 (default): the adaptive_* functions decide on the bloom precheck of the partitioned plan from a
 *                        sample of the probe side (4096 rows looked up in the partitioned build side): on when at most
 *                        "bloom_auto_max_hit_bp" (default 2300 = 23 %; measured break-even 24 %) of them hit; 0: adaptive_*_bloom filter, adaptive_* do
 *                        not, as named.  The explicit hash_join*_bloom
 *                        functions always run the precheck when the plan has two or more passes; hash_join* never do.
 *   "bloom_variant"    - hash / bit layout of the filter, 0..2 (csrc/fj_bloom_dev.h; default 0).  Must be
 *                        the same on every rank of a multi-GPU job (fj_bloom_prefilter checks it against the exporter's).
 *   "mat_single_pass"  - 1 (default): a materialising join whose output buffers hold >= np pairs runs single-pass (above);
 *                        0: always count, scan, emit.
 *   "plan_target_keys" - average build keys per final partition the plan aims for (default and maximum 4096 = half an LDS
 *                        table).  A testing knob: small values make small inputs take the deep
 *                        (two- and three-pass, bloom-filtered) plans that production only uses for >1M-row build sides.
 *   "join_wide"        - counting joins on the bucketed 16384-slot LDS table kernel (csrc/fj_join_wide.hip): 0 never, 1 whenever
 *                        eligible, 2 (default) when at most ~3 probe rows per build row reach the join (behind a filter: an estimate).
 *   "join_items_target" - work items the join of a plan with few partitions is cut into (default 2048; a tuning knob).
 *   "mm_heavy_keys"    - many-to-many inner join (FJ_ALGO_MANY_TO_MANY): 0 (default) a final partition of more than 4096 build rows
 *                        is refused; 1 it is joined in tiles of at most 4096 build rows, so that a build key may have any number of
 *                        copies (a join without such a partition launches nothing more than with 0).  Other values are refused.
 *                        The outer forms (FJ_ALGO_ALL_COPIES) refuse such a partition at either setting of THIS option.
 *   "mm_heavy_outer"   - the same for the all-copies outer joins (FJ_ALGO_ALL_COPIES with FJ_ALGO_LEFT_OUTER or FJ_ALGO_FULL_OUTER):
 *                        0 (default) a final partition of more than 4096 build rows is refused, message as ever; 1 it is joined in
 *                        tiles of at most 4096 build rows (a join without such a partition launches nothing more than with 0).  Other
 *                        values are refused.  Independent of "mm_heavy_keys", which keeps serving the inner form only: the two options
 *                        exist side by side only because existing behaviour is pinned - the outer forms' refusal at "mm_heavy_keys" = 1
 *                        and that option's refusal of any value but 0 and 1 are what callers and tests rely on today.
 *   "lab_hooks"        - test / measurement hooks, one bit each (csrc/fj_host.h FJ_HOOK_*; default 0): 1 a rank's own share of a
 *                        multi-GPU exchange travels through ncclSend / ncclRecv too, 2 injected failure of a local append, 4 split a
 *                        1-rank communicator, 8 one communicator, 16 the CU reserve on one rank too, 32 emitting pass on the tagged
 *                        kernel, 64 every 7th emit item takes its retry path.
 * fj_get_option returns -1 for an unknown name. */
int fj_set_option(const char* name, long long value);
long long fj_get_option(const char* name);

/* The device's key mixer (no reference counterpart; the reference hashes with CRC32C * const, hash_join.cpp:40-44, and
 * join results are hash-independent): a BIJECTION of 64-bit words.  Chunk pools, LDS tables and the owner shuffle's wire
 * format hold fj_key_mix64(key) instead of key - equality is preserved, radix digits are its top bits, table slots its low
 * bits, and a chunk of one radix bucket need not store the digits the bucket implies (7 bytes per key on the wire).
 * Host functions, no GPU needed: for tests and for hosts that want to predict the owner GPU of a key
 * (owner = ((mix >> 48) * nranks) >> 16 in the owner-scatter form; first-pass bucket * nranks >> fan_log0 in the chunk form). */
uint64_t fj_key_mix64(uint64_t key);
uint64_t fj_key_unmix64(uint64_t mixed);

/* One context per (process, device): owns the grow-only workspace, events and scratch words. */
fj_ctx* fj_ctx_create(int device);
void fj_ctx_destroy(fj_ctx* ctx);
size_t fj_ctx_workspace_bytes(const fj_ctx* ctx);
int fj_ctx_trim(fj_ctx* ctx);                 /* free the cached workspace; the context stays usable (grows again on demand).
                                                 NULL = the internal context of fj_join_host */

/*
 * replaces: all twelve pybind entry points hash_join.cpp:603-637 for HOST (NumPy) buffers.
 *   algo x bloom x materialize selects the function, e.g.
 *     hash_join_count_radix_bloom == (FJ_ALGO_RADIX, 1, 0); adaptive_join == (FJ_ALGO_ADAPTIVE, 0, 1).
 * build_vals must hold nb words (the reference never checks this; here it is the caller's
 * contract).  out_seconds receives the device-resident time (fj_timings.total_ms / 1e3); copies
 * over PCIe are reported separately through fj_last_timings().  When materialize != 0 and
 * out_keys/out_vals are non-NULL they receive malloc'ed host arrays of *out_count
 * (probe_key, build_value) pairs, to be released with fj_free_host(); pass NULL to drop them as
 * the reference does (hash_join.cpp:365-380).
 */
int fj_join_host(int algo, int bloom, int materialize,
                 const uint64_t* build_keys, const uint64_t* build_vals, size_t nb,
                 const uint64_t* probe_keys, size_t np,
                 uint64_t* out_count, double* out_seconds,
                 uint64_t** out_keys, uint64_t** out_vals);
void fj_free_host(void* p);
int fj_last_timings(fj_timings* out);

/*
 * Device-resident form of the same twelve functions (inputs already in HBM, 16-byte aligned).
 * stream is a hipStream_t (NULL = default stream).  hash_top_bits is 64 for a single-GPU join and
 * 48 after fj_owner_split (the top 16 hash bits chose the owner GPU).
 * Materialising joins: with d_out_keys == NULL the call counts only and keeps its partitions
 * resident; fj_emit_pairs() then writes exactly *out_count pairs into caller-allocated buffers.  A context holds ONE such
 * pending result (of this call, a materialising stream join or build-broadcast step): the next call that starts new work on the
 * context drops it; an fj_emit_pairs that is refused (capacity below the count, misaligned buffers) leaves it pending.
 * With d_out_keys != NULL and out_capacity >= count both steps happen in this call.  With out_capacity >= np - room for
 * ANY result, what the reference allocates too (hash_join.cpp:330-334) - a partitioned join with unique build keys runs in
 * ONE pass over the probe side (no counting pass; option "mat_single_pass", default 1): the first *out_count rows of the
 * buffers are the pairs.
 */
int fj_join_device(fj_ctx* ctx, int algo, int bloom, int materialize,
                   const uint64_t* d_build_keys, const uint64_t* d_build_vals, size_t nb,
                   const uint64_t* d_probe_keys, size_t np,
                   void* stream, int hash_top_bits,
                   uint64_t* out_count,
                   uint64_t* d_out_keys, uint64_t* d_out_vals, size_t out_capacity,
                   fj_timings* timings);
int fj_emit_pairs(fj_ctx* ctx, uint64_t* d_out_keys, uint64_t* d_out_vals, size_t out_capacity,
                  void* stream, fj_timings* timings);

/*
 * Multi-GPU building block (no reference counterpart: the reference is single-process).
 * Splits n local rows by owner GPU = (top 16 hash bits * nranks) >> 16 into nranks contiguous
 * segments of d_out_keys (and d_out_vals when d_vals != NULL); h_counts[r] = rows for rank r.
 * The caller exchanges the segments (RCCL all-to-all) and joins what it receives with
 * hash_top_bits = 48.
 */
int fj_owner_split(fj_ctx* ctx, const uint64_t* d_keys, const uint64_t* d_vals, size_t n, int nranks,
                   uint64_t* d_out_keys, uint64_t* d_out_vals, uint64_t* h_counts, void* stream);

/* error recovery: drops a stream join that a failed multi-GPU step may have left open on the context (no-op when none is open) */
int fj_stream_abort(fj_ctx* ctx);

/* Plan queries of the two multi-GPU forms: what fj_dist_join can do for a total build side of nb_total rows (no GPU work).
 *   fj_shuffle_plan - 0 if the owner shuffle's chunk form applies (a plan of two or more passes and at least nranks first-pass
 *                     buckets: build sides above ~2M rows in all); *fan_log0 = log2 of the first pass's buckets, *npass = passes
 *   fj_bcast_plan   - 0 if the build-broadcast form applies (the plan has a pass): radix bits, final partitions, bytes per key of
 *                     the high-word plane (2 from 134M build rows in all: 6 bytes per key on the wire) */
int fj_shuffle_plan(size_t nb_total, int nranks, int* fan_log0, int* npass);
int fj_bcast_plan(size_t nb_total, int* bits, uint32_t* nparts, int* mid_bytes);

/*
 * Native multi-GPU entry (no reference counterpart: the reference is one process, hash_join.cpp:318; SURVEY.md 5 row
 * "Distributed communication backend", 7.1 dist/alltoall): the counting radix join of relations whose rows are block-distributed
 * over the ranks of a communicator - BASELINE configs[4].  One process per GPU; every rank calls fj_dist_join_count with its
 * LOCAL rows and gets the GLOBAL match count.  ONE driver (csrc/fj_dist.hip) runs the owner shuffle in chunk form (above) over
 * whatever moves the bytes: per piece the first radix pass, the per-owner chunk counts all-gathered on a control channel, the
 * copy into the 7-byte wire format (a rank's own share straight into its receive buffer), the exchange, the owner's second
 * pass - on three streams, the host blocking once per piece; a failure on any rank is reported by every rank.
 *   fj_dist_unique_id           - rank 0: 128 bytes for the other ranks (any out-of-band channel), as ncclGetUniqueId
 *   fj_dist_comm_create         - every rank, after selecting its device and creating its fj_ctx (which outlives the
 *                                 communicator: fj_dist_comm_destroy drops a result the context holds in its buffers): ncclCommInitRank inside.
 *                                 RCCL is bound at run time (dlopen of librccl.so.1): a host that never calls this needs neither
 *                                 the library nor its headers.  Payload: grouped ncclSend / ncclRecv on an exchange stream;
 *                                 control collectives on a second communicator (ncclCommSplit) so that they do not queue behind
 *                                 the previous piece's sends.
 *   fj_dist_comm_from_nccl      - or wrap an ncclComm_t the host already has (not destroyed by fj_dist_comm_destroy)
 *   fj_dist_comm_from_transport - or bring your own transport: three blocking callbacks (gloo, MPI, a test harness).  With
 *                                 engine == NULL the rank's work runs on ctx's GPU; a stand-in engine (tests) replaces it,
 *                                 then ctx may be NULL and "device" pointers are whatever the stand-in's alloc returns.
 *   (a communicator serves ONE join at a time - it owns the exchange buffers and streams of the step; use one per thread)
 *   The CU reserve: over RCCL with more than one rank, the transport's send / receive kernels are resident on the GPU for the
 *   length of an exchange, and the partition passes and the wide join (one persistent workgroup per CU, static tile shares) must not
 *   find CUs taken.  Whether leaving 32 CUs free beats sharing all 256 is MEASURED per communicator: its second step runs with the
 *   reserve, its third without, both times the probe-side passes are timed (HIP events, an exchange in flight), the ranks add their
 *   times up in the next step's first all-gather, and every later step uses the faster setting (fj_dist_timings.reserve_*).
 *   FJ_DIST_RESERVE_CUS=n pins the number instead.
 *   fj_dist_join_count          - collective.  pieces: rounds of the probe exchange / partition ranges of a broadcast step; 0 = the
 *                                 driver decides (4, the measured default; 8 for a broadcast step that its model finds wire-bound:
 *                                 the tail behind the last piece is an eighth of the join), rank 0's value counts.  A build side
 *                                 of less than ~2M rows in all is refused (one-pass plan: join it on one GPU).
 *   fj_dist_join                - the same step, optionally materialising (materialize != 0: the build rows travel with their
 *                                 values, 16 bytes per build row on the wire): *out_local_count = pairs this rank owns; the
 *                                 caller then allocates them and calls fj_emit_pairs(ctx, ...) - before the next join on ctx.
 *                                 prefilter_below: the sender-side precheck (above) runs when a sample of the probe rows says that
 *                                 less than this share of them would travel - 0 = never (nothing is exported or sampled), >= 2 =
 *                                 always (no sample); rank 0's value is used on every rank; the HIP engine, or a stand-in with the
 *                                 optional precheck callbacks.  Costs one more kernel over a sender's probe rows and 1 byte
 *                                 per build key to every rank, saves (1 - survivors) of the probe exchange and of the owner's work.
 */
typedef struct fj_dist_comm fj_dist_comm;
typedef struct fj_dist_timings {
    size_t struct_size;                                /* IN: sizeof(fj_dist_timings) as the caller compiled it (the library writes no byte beyond it; 0 is refused) */
    double total_ms, split_ms, exchange_ms, join_ms;   /* host wall clock of this rank: whole step; waiting for the packing passes'
                                                          counts; the rest up to the local join's finish; finish + all-reduce */
    uint64_t local_count;                              /* matches this rank found in what it owns                 */
    uint64_t local_build_chunks, local_probe_chunks;   /* 256-key wire chunks this rank received (own share included); broadcast form: ROWS it joined (all ranks' build rows, its own probe rows) */
    uint64_t sent_chunks;                              /* ... and put on the links (own share excluded)            */
    int pieces, nranks, fan_log0, wire_chunk_bytes;    /* wire_chunk_bytes: 1792 (7 bytes per key) or 2048         */
    int prefilter;                                     /* 1: the sender-side precheck ran                          */
    double prefilter_sampled;                          /* share of the sampled probe rows that passed (-1: no sample) */
    uint64_t probe_rows_kept;                          /* probe rows of this rank that went into wire chunks       */
    uint64_t filter_bytes;                             /* bytes of partition filters this rank received            */
    int form;                                          /* FJ_DIST_FORM_SHUFFLE or FJ_DIST_FORM_BROADCAST: what the step ran as */
    int form_reserved;
    uint64_t wire_bytes_sent;                          /* bytes this rank put on the links (all peers)             */
    fj_timings local;                                  /* device timings of this rank's local join (fj_stream_finish) */
    /* the CU reserve (below): CUs this step's passes and joins left to the transport's own kernels; how that number came about
     * (0 = no reserve applies: one rank / a transport without kernels of its own, 1 = pinned by FJ_DIST_RESERVE_CUS, 2 = a measuring
     * step, 3 = chosen from the measurements); the measurements: this communicator's probe-side pass time per step, summed over the
     * ranks, with 32 CUs reserved and with none (ms; 0 until measured) */
    int reserve_cus, reserve_how;
    double reserve_with_ms, reserve_without_ms;
} fj_dist_timings;
typedef struct fj_dist_transport {
    void* user;
    int nranks, rank;
    int (*all_gather_u64)(void* user, const uint64_t* v, int n, uint64_t* out /* [nranks][n], rank-major */);
    int (*all_reduce_sum_u64)(void* user, uint64_t* v, int n);
    /* all-to-all of byte ranges that live in device memory (the driver has finished writing them): for part p < nparts and
     * peer r, send_bytes[p * nranks + r] bytes at send_ptr[...] go to r, recv_bytes[...] bytes from r land at recv_ptr[...];
     * returns once everything has landed.  Zero-byte entries (null pointers) are skipped on both sides. */
    int (*all_to_all_bytes)(void* user, int nparts, const void* const* send_ptr, const uint64_t* send_bytes,
                            void* const* recv_ptr, const uint64_t* recv_bytes);
} fj_dist_transport;
typedef struct fj_dist_engine_ops {   /* a stand-in for the rank's own work (the CPU test-suite); 0 = success everywhere */
    size_t struct_size;                                /* sizeof(fj_dist_engine_ops) as the caller compiled it: callbacks beyond it read as NULL (0 is refused) */
    void* user;
    size_t chunk_bytes;                                /* bytes per wire chunk the stand-in produces and consumes */
    const char* (*error)(void* user);
    int (*plan)(void* user, uint64_t nb_total, int nranks);
    void* (*alloc)(void* user, size_t bytes);
    void (*release)(void* user, void* p);
    int (*pack_begin)(void* user, const void* rows, uint64_t n, uint64_t nb_total, int nranks);
    int (*pack_counts)(void* user, uint64_t* used);
    int (*pack_finish)(void* user, void* const* dst_chunks, uint32_t* const* dst_dir);
    int (*open)(void* user, uint64_t nb_total, int nranks, int rank, uint64_t nb_bound, uint64_t np_bound, int pieces);
    int (*append)(void* user, int side, const void* chunks, uint32_t* dir, uint64_t nchunks);
    int (*finish)(void* user, uint64_t* count);
    void (*abort)(void* user);
    /* optional, all four or none (NULL: the stand-in has no sender-side precheck and fj_dist_join refuses prefilter_below > 0):
     * what fj_shuffle_part_filter_range / fj_stream_export_part_filters / fj_shuffle_pack_filter (called right after pack_begin
     * for a prechecked piece; *kept = rows it kept) / fj_part_filter_sample do */
    int (*filter_range)(void* user, uint64_t nb_total, int nranks, int rank, uint64_t* first, uint64_t* count, uint64_t* total, uint64_t* bytes_each);
    int (*export_filters)(void* user, void* dst);
    int (*pack_filter)(void* user, const void* filters, uint64_t* kept);
    int (*sample)(void* user, const void* rows, uint64_t n, uint64_t stride, const void* filters, uint64_t nb_total, int nranks, uint64_t* kept);
    /* optional, all seven or none (NULL: the stand-in has no build-broadcast form): what fj_bcast_region_bytes / fj_bcast_piece_span /
     * fj_bcast_plan (final partitions) / fj_bcast_pack + fj_bcast_pack_bounds (synchronous: bounds[pieces + 1]) / fj_bcast_probe /
     * fj_bcast_join / fj_bcast_finish do */
    uint64_t (*bc_region_bytes)(void* user, uint64_t nb_total, uint64_t nkeys);
    int (*bc_span)(void* user, uint64_t nb_total, uint64_t nkeys, uint64_t k_lo, uint64_t k_hi, int part, uint64_t* offset, uint64_t* bytes);
    int (*bc_nparts)(void* user, uint64_t nb_total, uint32_t* nparts);
    int (*bc_pack)(void* user, const void* rows, uint64_t n, uint64_t nb_total, void* region, int pieces, uint64_t* bounds);
    int (*bc_probe)(void* user, const void* rows, uint64_t n, uint64_t nb_total);
    int (*bc_join)(void* user, const void* base, int nsrc, const uint64_t* region_off, const uint64_t* nkeys, uint32_t part_lo, uint32_t part_hi);
    int (*bc_finish)(void* user, uint64_t* count);
} fj_dist_engine_ops;
/* The form a counting step takes (rank 0's setting is used on every rank):
 *   FJ_DIST_FORM_SHUFFLE   - the owner shuffle in chunk form: every row of both relations travels to the owner of its first radix
 *                            digit, 7 bytes per key;
 *   FJ_DIST_FORM_BROADCAST - the build broadcast (csrc/fj_bcast.hip): the probe rows stay, every rank's build rows travel to every
 *                            peer, 6 bytes per key; up to 16 ranks.  Materialising joins too (round 6): the values travel as a
 *                            fourth part (14 bytes per build row) and the pairs stay with the rank that holds the PROBE row
 *                            (fj_emit_pairs after the step).  In every form a build key that occurs more than once yields ONE pair
 *                            per matching probe row, with the value of one of its copies;
 *   FJ_DIST_FORM_AUTO      - (default) whichever a per-link / per-rank cost model puts ahead for the step's sizes: bytes per link
 *                            over link_bytes_per_s (<= 0: 55e9) against the kernel time per rank measured on one MI355X
 *                            (profiles/r05_scale_model.txt).  Probe-heavy joins (BASELINE configs[4]: 10 probe rows per build row)
 *                            broadcast at every N <= 16; build-heavy ones shuffle. */
#define FJ_DIST_FORM_AUTO 0
#define FJ_DIST_FORM_SHUFFLE 1
#define FJ_DIST_FORM_BROADCAST 2
int fj_dist_comm_set_form(fj_dist_comm* comm, int form, double link_bytes_per_s);
/* the model behind FJ_DIST_FORM_AUTO: modelled seconds of one counting step in either form (NULL: not wanted); returns the form it picks */
int fj_dist_model(int nranks, uint64_t nb_max, uint64_t np_max, uint64_t nb_total, uint64_t np_global, uint64_t region_max, double link_bytes_per_s,
                  double* t_shuffle, double* t_broadcast);
int fj_dist_unique_id(char* out128);
fj_dist_comm* fj_dist_comm_create(fj_ctx* ctx, const char* unique_id128, int nranks, int rank);
fj_dist_comm* fj_dist_comm_from_nccl(fj_ctx* ctx, void* nccl_comm);
fj_dist_comm* fj_dist_comm_from_transport(fj_ctx* ctx, const fj_dist_transport* transport, const fj_dist_engine_ops* engine);
void fj_dist_comm_destroy(fj_dist_comm* comm);
int fj_dist_comm_rank(const fj_dist_comm* comm);
int fj_dist_comm_size(const fj_dist_comm* comm);
int fj_dist_join_count(fj_dist_comm* comm, const uint64_t* d_build_keys, size_t nb, const uint64_t* d_probe_keys, size_t np, int pieces,
                       void* stream, uint64_t* out_global_count, fj_dist_timings* timings);
int fj_dist_join(fj_dist_comm* comm, const uint64_t* d_build_keys, const uint64_t* d_build_vals, size_t nb, const uint64_t* d_probe_keys, size_t np,
                 int pieces, int materialize, double prefilter_below, void* stream, uint64_t* out_global_count, uint64_t* out_local_count,
                 fj_dist_timings* timings);

/*
 * Deterministic synthetic relations, generated in HBM:
 *   build_keys[i] = (first+i+1)*M, build_vals[i] = first+i, M = 0x9E3779B97F4A7C15;
 *   probe j = first+i: r = 1 + mix(seed,j) % B, hit = mix(seed^1,j) % 10000 < hit_bp,
 *   key = (r + (hit ? 0 : B)) * M.   *h_expected_hits = number of hits generated (closed-form count).
 */
int fj_generate_build(fj_ctx* ctx, uint64_t* d_keys, uint64_t* d_vals, uint64_t first, size_t n, void* stream);
int fj_generate_probe(fj_ctx* ctx, uint64_t* d_keys, uint64_t first, size_t n, uint64_t build_total,
                      uint64_t seed, uint32_t hit_bp, uint64_t* h_expected_hits, void* stream);

/* plain device memory helpers for hosts without another allocator */
int fj_device_malloc(void** p, size_t bytes);
int fj_device_free(void* p);
int fj_memcpy_h2d(void* d, const void* h, size_t bytes);
int fj_memcpy_d2h(void* h, const void* d, size_t bytes);
int fj_memcpy_d2d(void* d_dst, const void* d_src, size_t bytes);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* FLASHJOIN_H */