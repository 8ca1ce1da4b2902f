// fj_entry.hip -- the algo word's decoder and the refusal list of fj_join_device and fj_join_host (fj_entry.h).  Host code only.
#include "fj_entry.h"
#include "fj_host.h"

namespace fjh {

const EntryWords DEVICE_ENTRY = {"fj_join_device", "d_build_keys", "d_build_vals", "d_probe_keys", "d_out_keys", "d_out_vals", "out_capacity", "d_build_vals", "no build value", false};
const EntryWords HOST_ENTRY = {"fj_join_host", "build_keys", "build_vals", "probe_keys", "out_keys", "out_vals", "g", "build values", "none", true};

AlgoForm decode_algo(int algo) {
    AlgoForm f{};
    f.word = f.base = algo;
    f.agg = FJ_GJ_SUM;
    if (algo < 0) return f;                                 // (no flag is read out of a negative word: an unknown algo)
    auto has = [algo](int bit) { return (algo & bit) != 0; };
    f.many = has(FJ_ALGO_MANY_TO_MANY); f.left = has(FJ_ALGO_LEFT_OUTER); f.anti = has(FJ_ALGO_ANTI); f.rid = has(FJ_ALGO_ROW_IDS);
    f.full = has(FJ_ALGO_FULL_OUTER); f.allc = has(FJ_ALGO_ALL_COPIES); f.po = has(FJ_ALGO_PROBE_ORDER); f.bo = has(FJ_ALGO_BUILD_ORDER);
    f.gb = has(FJ_ALGO_GROUP_BY);
    f.inv = f.gb && has(FJ_ALGO_INVERSE); f.kpair = f.gb && has(FJ_ALGO_KEY_PAIR); f.grows = f.gb && has(FJ_ALGO_GROUP_ROWS);
    f.aall = f.gb && has(FJ_ALGO_AGG_ALL); f.aarg = f.gb && has(FJ_ALGO_AGG_ARG);
    f.amerge = f.aall && has(FJ_ALGO_AGG_MERGE);
    f.pagg = f.kpair && f.aall && !f.inv;
    f.retain = f.po && has(FJ_ALGO_RETAIN_BUILD); f.reuse = f.po && has(FJ_ALGO_REUSE_BUILD);
    f.bo_reuse = f.bo && has(FJ_ALGO_REUSE_BUILD);          // (FJ_ALGO_BUILD_ORDER | FJ_ALGO_RETAIN_BUILD stays unknown)
    f.accum = f.bo_reuse && has(FJ_ALGO_ACCUMULATE);
    const bool agg_form = f.bo || f.gb;
    f.amin = agg_form && has(FJ_ALGO_AGG_MIN); f.amax = agg_form && has(FJ_ALGO_AGG_MAX);
    f.asigned = agg_form && has(FJ_ALGO_AGG_SIGNED); f.afloat = agg_form && has(FJ_ALGO_AGG_FLOAT);
    if (f.amin) f.agg = f.asigned ? FJ_GJ_MIN_S : FJ_GJ_MIN_U;
    if (f.amax) f.agg = f.asigned ? FJ_GJ_MAX_S : FJ_GJ_MAX_U;
    if (f.afloat) f.agg = f.amin ? FJ_GJ_MIN_F : f.amax ? FJ_GJ_MAX_F : FJ_GJ_SUM_F;
    f.kind = f.afloat ? KIND_FLOAT : f.asigned ? KIND_SIGNED : KIND_UNSIGNED;
    // a modifier counts as recognised only beside the flag it modifies: anywhere else it stays in the base, an unknown algo
    int known = FJ_ALGO_MANY_TO_MANY | FJ_ALGO_LEFT_OUTER | FJ_ALGO_ANTI | FJ_ALGO_ROW_IDS | FJ_ALGO_FULL_OUTER | FJ_ALGO_ALL_COPIES |
                FJ_ALGO_PROBE_ORDER | FJ_ALGO_BUILD_ORDER | FJ_ALGO_GROUP_BY;
    if (agg_form) known |= FJ_ALGO_AGG_MIN | FJ_ALGO_AGG_MAX | FJ_ALGO_AGG_SIGNED | FJ_ALGO_AGG_FLOAT;
    if (f.gb) known |= FJ_ALGO_INVERSE | FJ_ALGO_AGG_ALL | FJ_ALGO_AGG_ARG | FJ_ALGO_KEY_PAIR | FJ_ALGO_GROUP_ROWS;
    if (f.amerge) known |= FJ_ALGO_AGG_MERGE;
    if (f.po) known |= FJ_ALGO_RETAIN_BUILD | FJ_ALGO_REUSE_BUILD;
    if (f.bo_reuse) known |= FJ_ALGO_REUSE_BUILD | FJ_ALGO_ACCUMULATE;
    f.base = algo & ~known;
    return f;
}

// Every refusal that needs no context, in ONE order for both entries (so both hold for a null context and on a machine without a
// device).  `e` words the message; a rule that one entry lacks is one line conditioned on e.host:
//   device entry only: output capacities and alignments, hash_top_bits, null and misaligned inputs, the outputs a form cannot do without
//                      when it has rows (the host entry allocates them itself), the prepared side's FJ_ALGO_REUSE_BUILD rules;
//   host entry only:   FJ_ALGO_RETAIN_BUILD / _REUSE_BUILD are not served; an output it hands out unconditionally is needed without rows too.
int check_entry(const AlgoForm& f, const EntryWords& e, const EntryArgs& a) {
    const bool dev = !e.host, materialize = a.materialize != 0;
    const size_t nb = a.nb, np = a.np;
    const bool have_bk = a.bk || e.host, have_pk = a.pk || e.host;       // (the host entry has never looked at its key columns' pointers)
    const bool unread = build_vals_unread(f, a.bv != nullptr);
    const void* bv = unread ? a.bk : a.bv;                               // the pointer the paths read as build values
    const bool have_bv = unread ? have_bk : a.bv != nullptr;
    const bool outs_misaligned = dev && (((uintptr_t)a.ok | (uintptr_t)a.ov) & 7);
    const char* joins = f.many ? "MANY_TO_MANY" : f.left ? "LEFT_OUTER" : f.anti ? "ANTI" : f.full ? "FULL_OUTER" : f.allc ? "ALL_COPIES" : nullptr;
    const char* gb_joins = joins ? joins : f.po ? "PROBE_ORDER" : f.bo ? "BUILD_ORDER" : nullptr;      // what a group-by of one relation cannot carry
    const char* minmax = f.amin ? "MIN" : "MAX";

    if (f.word >= 0 && (f.word & FJ_ALGO_GROUP_ROWS) && !f.gb)
        return set_err("%s: unknown algo %d (FJ_ALGO_GROUP_ROWS modifies FJ_ALGO_GROUP_BY)", e.fn, f.word);
    if (f.grows && (f.word & (FJ_ALGO_INVERSE | FJ_ALGO_ROW_IDS | FJ_ALGO_AGG_MIN | FJ_ALGO_AGG_MAX | FJ_ALGO_AGG_SIGNED | FJ_ALGO_AGG_FLOAT | FJ_ALGO_AGG_ALL | FJ_ALGO_AGG_ARG | FJ_ALGO_AGG_MERGE | FJ_ALGO_KEY_PAIR)))
        return set_err("%s: FJ_ALGO_GROUP_ROWS cannot be combined with FJ_ALGO_%s (%s is taken by the row indices and the groups' starts, and no value column is read)", e.fn,
                       f.inv ? "INVERSE" : f.rid ? "ROW_IDS" : f.amin ? "AGG_MIN" : f.amax ? "AGG_MAX" : f.asigned ? "AGG_SIGNED" : f.afloat ? "AGG_FLOAT" :
                       f.aall ? "AGG_ALL" : f.aarg ? "AGG_ARG" : (f.word & FJ_ALGO_AGG_MERGE) ? "AGG_MERGE" : "KEY_PAIR", e.ov);
    if (f.word >= 0 && (f.word & FJ_ALGO_AGG_MERGE) && !f.amerge)
        return set_err("%s: unknown algo %d (FJ_ALGO_AGG_MERGE modifies FJ_ALGO_GROUP_BY | FJ_ALGO_AGG_ALL)", e.fn, f.word);
    if (f.word >= 0 && (f.word & FJ_ALGO_KEY_PAIR) && !f.gb)
        return set_err("%s: unknown algo %d (FJ_ALGO_KEY_PAIR modifies FJ_ALGO_GROUP_BY | FJ_ALGO_INVERSE)", e.fn, f.word);
    if (f.gb) {
        // group-by on one relation (csrc/fj_groupby*.hip): the relation is the build side; out_keys = the g distinct keys, out_vals = one
        // aggregate per key - or what the modifier below says
        const bool need_outs = nb || e.host;                 // the plane forms: both outputs (the host entry hands both out without rows too)
        if (f.pagg) {                                       // a two-column key with four aggregates: build_keys = A, build_vals = B, probe_keys = the value column V, np == nb
            if (gb_joins) return set_err("%s: FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_%s (it groups one relation: there is no join in it)", e.fn, gb_joins);
            if (f.amin || f.amax || f.rid || f.aarg || f.amerge)
                return set_err("%s: FJ_ALGO_KEY_PAIR | FJ_ALGO_AGG_ALL cannot be combined with FJ_ALGO_%s (%s is taken by column B and the four aggregates of the value column)", e.fn,
                               f.amin ? "AGG_MIN" : f.amax ? "AGG_MAX" : f.rid ? "ROW_IDS" : f.aarg ? "AGG_ARG" : "AGG_MERGE", e.ov);
            if (f.asigned && f.afloat) return set_err("%s: FJ_ALGO_KEY_PAIR | FJ_ALGO_AGG_ALL: FJ_ALGO_AGG_FLOAT cannot be combined with FJ_ALGO_AGG_SIGNED (a double carries its own sign)", e.fn);
            if (!materialize) return set_err("%s: FJ_ALGO_KEY_PAIR | FJ_ALGO_AGG_ALL needs materialize = 1 (the pairs and their aggregates are the result)", e.fn);
            if ((need_outs && (!a.ok || !a.ov)) || (nb && (!a.bk || !a.bv || !a.pk)))
                return set_err("%s: FJ_ALGO_KEY_PAIR | FJ_ALGO_AGG_ALL needs %s, %s, %s, %s and %s (the key columns A and B, the value column V, column A of the g groups and five planes of %s words)",
                               e.fn, e.bk, e.bv, e.pk, e.ok, e.ov, e.plane);
            if (np != nb) return set_err("%s: FJ_ALGO_KEY_PAIR | FJ_ALGO_AGG_ALL needs np == nb, got np = %zu and nb = %zu (%s is the value column of the one relation)", e.fn, np, nb, e.pk);
            if (dev && nb && !a.cap) return set_err("%s: FJ_ALGO_KEY_PAIR | FJ_ALGO_AGG_ALL needs an output capacity of at least 1 row (any bound on the number of groups will do)", e.fn);
            if ((uint64_t)nb > (1ull << 40)) return set_err("%s: FJ_ALGO_KEY_PAIR takes at most 2^40 rows, got %zu (a row position is kept in 40 bits)", e.fn, nb);
        }
        if (f.amerge) {                                     // partial rows in, FJ_ALGO_AGG_ALL's outputs out: its refusals under this flag's name, ahead of them
            if (gb_joins) return set_err("%s: FJ_ALGO_AGG_MERGE cannot be combined with FJ_ALGO_%s (it merges partial group-by rows: there is no join in it)", e.fn, gb_joins);
            if (a.pk || np) return set_err("%s: FJ_ALGO_AGG_MERGE takes no probe side (%s must be NULL and np 0: the partial rows are the build side)", e.fn, e.pk);
            if (f.amin || f.amax) return set_err("%s: FJ_ALGO_AGG_MERGE cannot be combined with FJ_ALGO_AGG_%s (it merges both the minima and the maxima)", e.fn, minmax);
            if (f.rid || f.inv || f.aarg) return set_err("%s: FJ_ALGO_AGG_MERGE cannot be combined with FJ_ALGO_%s (a partial row is no row of a relation)", e.fn, f.rid ? "ROW_IDS" : f.inv ? "INVERSE" : "AGG_ARG");
            if (f.asigned && f.afloat) return set_err("%s: FJ_ALGO_AGG_MERGE: FJ_ALGO_AGG_FLOAT cannot be combined with FJ_ALGO_AGG_SIGNED (a double carries its own sign)", e.fn);
            if (!materialize) return set_err("%s: FJ_ALGO_AGG_MERGE needs materialize = 1 (the merged rows are the result)", e.fn);
            if ((need_outs && (!a.ok || !a.ov)) || (nb && !a.bv))
                return set_err("%s: FJ_ALGO_AGG_MERGE needs %s, %s and %s (four planes of nb words - count, sum, min, max -, the g distinct keys and four planes of %s words)", e.fn, e.bv, e.ok, e.ov, e.plane);
            if (dev && nb && !a.cap) return set_err("%s: FJ_ALGO_AGG_MERGE needs an output capacity of at least 1 row (any bound on the number of groups will do)", e.fn);
        }
        if (gb_joins) return set_err("%s: FJ_ALGO_GROUP_BY cannot be combined with FJ_ALGO_%s (it groups one relation: there is no join in it)", e.fn, gb_joins);
        if (!f.pagg && (a.pk || np)) return set_err("%s: FJ_ALGO_GROUP_BY takes no probe side (%s must be NULL and np 0: the relation to group is the build side)", e.fn, e.pk);
        if (f.aall) {                                       // four aggregates in four planes of out_vals; the device entry takes any capacity >= 1 (g is checked after the device work)
            if (f.amin || f.amax) return set_err("%s: FJ_ALGO_AGG_ALL cannot be combined with FJ_ALGO_AGG_%s (it holds both the minimum and the maximum)", e.fn, minmax);
            if (f.rid || f.inv) return set_err("%s: FJ_ALGO_AGG_ALL cannot be combined with FJ_ALGO_%s (%s is taken by the four aggregates)", e.fn, f.rid ? "ROW_IDS" : "INVERSE", e.ov);
            if (f.asigned && f.afloat) return set_err("%s: FJ_ALGO_AGG_FLOAT cannot be combined with FJ_ALGO_AGG_SIGNED (a double carries its own sign)", e.fn);
            if (!materialize) return set_err("%s: FJ_ALGO_AGG_ALL needs materialize = 1 (materialize = 0 returns the number of distinct keys alone)", e.fn);
            if ((need_outs && (!a.ok || !a.ov)) || (nb && !a.bv))
                return set_err("%s: FJ_ALGO_AGG_ALL needs %s, %s and %s (the value column, the g distinct keys and four planes of %s words)", e.fn, e.bv, e.ok, e.ov, e.plane);
            if (dev && nb && !a.cap) return set_err("%s: FJ_ALGO_AGG_ALL needs an output capacity of at least 1 row (any bound on the number of groups will do)", e.fn);
        }
        if (f.aarg) {                                       // the row of each group's extreme: out_vals is two planes, the row index and the extreme
            if (f.aall) return set_err("%s: FJ_ALGO_AGG_ARG cannot be combined with FJ_ALGO_AGG_ALL (%s is taken by the four aggregates)", e.fn, e.ov);
            if (f.rid || f.inv) return set_err("%s: FJ_ALGO_AGG_ARG cannot be combined with FJ_ALGO_%s (%s is taken by the row indices and the extremes)", e.fn, f.rid ? "ROW_IDS" : "INVERSE", e.ov);
            if (f.amin == f.amax) return set_err("%s: FJ_ALGO_AGG_ARG needs exactly one of FJ_ALGO_AGG_MIN and FJ_ALGO_AGG_MAX (%s)", e.fn, f.amin ? "both are set: call twice" : "neither is set");
            if (f.asigned && f.afloat) return set_err("%s: FJ_ALGO_AGG_FLOAT cannot be combined with FJ_ALGO_AGG_SIGNED (a double carries its own sign)", e.fn);
            if (!materialize) return set_err("%s: FJ_ALGO_AGG_ARG needs materialize = 1 (materialize = 0 returns the number of distinct keys alone)", e.fn);
            if ((need_outs && (!a.ok || !a.ov)) || (nb && !a.bv))
                return set_err("%s: FJ_ALGO_AGG_ARG needs %s, %s and %s (the value column, the g distinct keys and two planes of %s words)", e.fn, e.bv, e.ok, e.ov, e.plane);
        }
        if (f.afloat) {                                     // the value column and out_vals hold IEEE-754 doubles
            if (f.asigned) return set_err("%s: FJ_ALGO_AGG_FLOAT cannot be combined with FJ_ALGO_AGG_SIGNED (a double carries its own sign)", e.fn);
            if (f.rid || f.inv) return set_err("%s: FJ_ALGO_AGG_FLOAT cannot be combined with FJ_ALGO_%s (positions and group ids are integers)", e.fn, f.rid ? "ROW_IDS" : "INVERSE");
            if (nb && !a.bv) return set_err("%s: FJ_ALGO_AGG_FLOAT with FJ_ALGO_GROUP_BY needs %s (the float64 value column, nb words: the count form has no float form)", e.fn, e.bv);
        }
        if (f.inv) {                                        // the group id of every row (out_vals: nb words), no aggregate beside it
            if (f.amin || f.amax || f.asigned)
                return set_err("%s: FJ_ALGO_INVERSE cannot be combined with FJ_ALGO_AGG_%s (the ids group the rows once: every aggregate is a pass of the caller's over them)", e.fn,
                               f.amin ? "MIN" : f.amax ? "MAX" : "SIGNED");
            if (f.rid) return set_err("%s: FJ_ALGO_INVERSE cannot be combined with FJ_ALGO_ROW_IDS (%s is taken: one per-call output)", e.fn, e.ov);
            if (!materialize) return set_err("%s: FJ_ALGO_INVERSE needs materialize = 1 (materialize = 0 returns the number of distinct keys alone)", e.fn);
            if (dev && nb && (!a.ok || !a.ov)) return set_err("%s: FJ_ALGO_INVERSE needs d_out_keys and d_out_vals (the g distinct keys and the nb group ids that index them)", e.fn);
        }
        if (f.kpair) {                                      // a two-column key: the group ids as above, out_keys the row index of every group's first occurrence
            if (!f.inv && !f.pagg) return set_err("%s: FJ_ALGO_KEY_PAIR modifies FJ_ALGO_GROUP_BY | FJ_ALGO_INVERSE (the group ids of a two-column key are its result: FJ_ALGO_INVERSE is missing) or FJ_ALGO_GROUP_BY | FJ_ALGO_AGG_ALL (the pairs with four aggregates of a third column)", e.fn);
            if (nb && !a.bv) return set_err("%s: FJ_ALGO_KEY_PAIR needs %s (the second key column, nb words)", e.fn, e.bv);
            if ((uint64_t)nb > (1ull << 40)) return set_err("%s: FJ_ALGO_KEY_PAIR takes at most 2^40 rows, got %zu (a row position is kept in 40 bits)", e.fn, nb);
            if (dev && ((uintptr_t)a.bv & 15)) return set_err("%s: input pointers must be 16-byte aligned", e.fn);
        }
        if (f.grows) {                                      // the rows of every group: out_vals is two planes, the nb row indices and the g starts (no other modifier: refused above)
            if (!materialize) return set_err("%s: FJ_ALGO_GROUP_ROWS needs materialize = 1 (materialize = 0 returns the number of distinct keys alone)", e.fn);
            if (dev && nb && (!a.ok || !a.ov)) return set_err("%s: FJ_ALGO_GROUP_ROWS needs d_out_keys and d_out_vals (the g distinct keys and two planes of out_capacity words: the nb row indices and the g starts)", e.fn);
            if ((uint64_t)nb > (1ull << 40)) return set_err("%s: FJ_ALGO_GROUP_ROWS takes at most 2^40 rows, got %zu (a row position is kept in 40 bits)", e.fn, nb);
        }
        if (f.amin && f.amax) return set_err("%s: FJ_ALGO_AGG_MIN cannot be combined with FJ_ALGO_AGG_MAX (one aggregate per call: call twice)", e.fn);
        if (f.asigned && !f.amin && !f.amax && !f.aall) return set_err("%s: FJ_ALGO_AGG_SIGNED modifies FJ_ALGO_AGG_MIN or FJ_ALGO_AGG_MAX (the sum is taken modulo 2^64 and has no sign)", e.fn);
        if ((f.amin || f.amax) && nb && !a.bv) return set_err("%s: FJ_ALGO_AGG_%s with FJ_ALGO_GROUP_BY needs %s (the value column, nb words)", e.fn, minmax, e.bv);
        if (f.rid && (f.amin || f.amax)) return set_err("%s: FJ_ALGO_ROW_IDS cannot be combined with FJ_ALGO_AGG_%s under FJ_ALGO_GROUP_BY (the first occurrence's position IS the aggregate)", e.fn, minmax);
        if (f.rid && !materialize) return set_err("%s: FJ_ALGO_ROW_IDS with FJ_ALGO_GROUP_BY needs materialize = 1 (materialize = 0 returns the number of distinct keys alone)", e.fn);
        if (dev && materialize) {
            if (nb && !a.ok) return set_err("%s: FJ_ALGO_GROUP_BY with materialize = 1 needs d_out_keys (d_out_vals is optional; materialize = 0 returns the number of distinct keys alone)", e.fn);
            if (!f.aall && a.cap < nb) return set_err("%s: output capacity %zu < %zu rows (FJ_ALGO_GROUP_BY: every row may be a group of its own)", e.fn, a.cap, nb);
            if (outs_misaligned) return set_err("%s: output buffers must be 8-byte aligned", e.fn);
        }
    }
    if (f.bo) {
        // build-order aggregate join (csrc/fj_group.hip): out_keys = the counts, out_vals = the sums (FJ_ALGO_AGG_MIN / _MAX: the minima /
        // maxima), nb words each; build_vals is the PROBE side's value column.  Onto the prepared build side (csrc/fj_prepared.hip) there
        // is no build side in the call and the outputs hold the rows the side was prepared from (checked on the context)
        const bool rows = nb || f.bo_reuse || e.host;        // (the host entry hands out what was asked for without rows too)
        if (e.host && f.bo_reuse)
            return set_err("%s: FJ_ALGO_BUILD_ORDER | FJ_ALGO_REUSE_BUILD%s is not served here (the internal context is shared by every host-buffer call of the process): call fj_join_device on a context of your own",
                           e.fn, f.accum ? " | FJ_ALGO_ACCUMULATE" : "");
        if (joins || f.rid || f.po)
            return set_err("%s: FJ_ALGO_BUILD_ORDER cannot be combined with FJ_ALGO_%s (it has one row per build row, at the build row's position)", e.fn,
                           f.many ? "MANY_TO_MANY" : f.left ? "LEFT_OUTER" : f.anti ? "ANTI" : f.rid ? "ROW_IDS" : f.full ? "FULL_OUTER" : f.allc ? "ALL_COPIES" : "PROBE_ORDER");
        if (f.afloat) {                                     // the probe side's value column and out_vals hold IEEE-754 doubles
            if (f.asigned) return set_err("%s: FJ_ALGO_AGG_FLOAT cannot be combined with FJ_ALGO_AGG_SIGNED (a double carries its own sign)", e.fn);
            if (np && !a.bv) return set_err("%s: FJ_ALGO_AGG_FLOAT with FJ_ALGO_BUILD_ORDER needs %s (here the probe side's float64 value column, np words: the count form has no float form)", e.fn, e.bv);
            if (rows && !a.ov) return set_err("%s: FJ_ALGO_AGG_FLOAT with FJ_ALGO_BUILD_ORDER needs %s (the float64 aggregates; the counts alone are the plain count form)", e.fn, e.ov);
        }
        if (f.bo_reuse && (a.bk || nb)) return set_err("%s: FJ_ALGO_REUSE_BUILD takes no build side (d_build_keys must be NULL and nb 0: the context's prepared side is aggregated onto; d_build_vals is the probe side's value column)", e.fn);
        if (f.amin && f.amax) return set_err("%s: FJ_ALGO_AGG_MIN cannot be combined with FJ_ALGO_AGG_MAX (one aggregate per call: call twice)", e.fn);
        if (f.asigned && !f.amin && !f.amax) return set_err("%s: FJ_ALGO_AGG_SIGNED modifies FJ_ALGO_AGG_MIN or FJ_ALGO_AGG_MAX (the sum is taken modulo 2^64 and has no sign)", e.fn);
        if (!materialize) return set_err("%s: FJ_ALGO_BUILD_ORDER needs materialize = 1 (its outputs are the result; P alone is the many-to-many counting join's)", e.fn);
        if (rows && !a.ok && !a.ov) return set_err("%s: FJ_ALGO_BUILD_ORDER needs an output (the counts %s, the sums %s, or both)", e.fn, e.ok, e.ov);
        if (rows && (f.amin || f.amax) && !a.ov) return set_err("%s: FJ_ALGO_AGG_%s needs %s (the counts alone are the plain count form of FJ_ALGO_BUILD_ORDER)", e.fn, minmax, e.ov);
        if (dev && a.cap < nb) return set_err("%s: output capacity %zu < %zu build rows (FJ_ALGO_BUILD_ORDER writes every build row)", e.fn, a.cap, nb);
        if (outs_misaligned) return set_err("%s: output buffers must be 8-byte aligned", e.fn);
        if (np && a.ov && !a.bv) return set_err("%s: FJ_ALGO_BUILD_ORDER with %s needs %s (here the probe side's value column, np words)", e.fn, e.ov, e.bv);
    }
    if (f.po) {
        // probe-order join (csrc/fj_aligned.hip); out_keys is the byte mask here: no alignment asked of it.  The prepared build side
        // (csrc/fj_prepared.hip): one call prepares OR reuses, and a reuse brings no build side of its own
        if (e.host && (f.retain || f.reuse))
            return set_err("%s: FJ_ALGO_%s_BUILD is not served here (the internal context is shared by every host-buffer call of the process): call fj_join_device on a context of your own",
                           e.fn, f.retain ? "RETAIN" : "REUSE");
        if (joins) return set_err("%s: FJ_ALGO_PROBE_ORDER cannot be combined with FJ_ALGO_%s (it has one row per probe row, at the probe row's position)", e.fn, joins);
        if (!materialize) return set_err("%s: FJ_ALGO_PROBE_ORDER needs materialize = 1 (its match count is the counting join's)", e.fn);
        if ((np || e.host) && !a.ok && !a.ov) return set_err("%s: FJ_ALGO_PROBE_ORDER needs an output (%s, the byte mask %s, or both)", e.fn, e.ov, e.ok);
        if (dev && a.cap < np) return set_err("%s: output capacity %zu < %zu probe rows (FJ_ALGO_PROBE_ORDER writes every probe row)", e.fn, a.cap, np);
        if (dev && ((uintptr_t)a.ov & 7)) return set_err("%s: d_out_vals must be 8-byte aligned", e.fn);
        if (f.retain && f.reuse) return set_err("%s: FJ_ALGO_RETAIN_BUILD cannot be combined with FJ_ALGO_REUSE_BUILD (a call prepares a build side or probes the prepared one)", e.fn);
        if (f.reuse && (a.bk || a.bv || nb)) return set_err("%s: FJ_ALGO_REUSE_BUILD takes no build side (d_build_keys and d_build_vals must be NULL and nb 0: the context's prepared side is probed)", e.fn);
        if (nb && a.ov && !f.rid && !a.bv) return set_err("%s: FJ_ALGO_PROBE_ORDER with %s needs %s (only FJ_ALGO_ROW_IDS and the mask alone read %s)", e.fn, e.ov, e.values, e.none);
    }
    if (f.rid && !f.gb && !materialize) return set_err("%s: FJ_ALGO_ROW_IDS needs materialize = 1 (it changes what the output rows hold)", e.fn);
    if (f.allc) {
        // left / full outer join that keeps every copy of a duplicated build key (csrc/fj_many.hip).  The result's size is not known up
        // front: no capacity check here, the two-phase rule of the materialising joins applies (count, then emit)
        if (f.anti) return set_err("%s: FJ_ALGO_ALL_COPIES cannot be combined with FJ_ALGO_ANTI (an anti join has no copies to keep)", e.fn);
        if (f.many) return set_err("%s: FJ_ALGO_ALL_COPIES cannot be combined with FJ_ALGO_MANY_TO_MANY (that flag alone is the inner join that keeps every copy)", e.fn);
        if (!f.left && !f.full) return set_err("%s: unknown algo %d (FJ_ALGO_ALL_COPIES modifies FJ_ALGO_LEFT_OUTER or FJ_ALGO_FULL_OUTER; FJ_ALGO_MANY_TO_MANY is the inner form)", e.fn, f.word);
        if (f.left && f.full) return set_err("%s: FJ_ALGO_FULL_OUTER cannot be combined with FJ_ALGO_LEFT_OUTER", e.fn);
        if (!materialize) return set_err("%s: FJ_ALGO_ALL_COPIES needs materialize = 1 (there is no counting-only form)", e.fn);
        if (!a.out_count) return set_err("%s: FJ_ALGO_ALL_COPIES needs out_count (three words: pairs, unmatched build rows, unmatched probe rows)", e.fn);
        if (outs_misaligned) return set_err("%s: output buffers must be 8-byte aligned", e.fn);
        if (nb && !have_bv) return set_err("%s: FJ_ALGO_ALL_COPIES needs %s (only FJ_ALGO_ROW_IDS reads %s)", e.fn, e.values, e.none);
    } else if (f.full) {
        // full outer join (csrc/fj_outer.hip)
        if (f.left || f.anti) return set_err("%s: FJ_ALGO_FULL_OUTER cannot be combined with FJ_ALGO_%s", e.fn, f.left ? "LEFT_OUTER" : "ANTI");
        if (f.many) return set_err("%s: FJ_ALGO_FULL_OUTER cannot be combined with FJ_ALGO_MANY_TO_MANY", e.fn);
        if (!materialize) return set_err("%s: FJ_ALGO_FULL_OUTER needs materialize = 1 (its match count is the counting join's)", e.fn);
        if (dev && (np || nb) && (!a.ok || !a.ov)) return set_err("%s: FJ_ALGO_FULL_OUTER needs output buffers (d_out_keys and d_out_vals)", e.fn);
        if (dev && (a.cap < np || a.cap - np < nb)) return set_err("%s: output capacity %zu < %zu probe rows + %zu build rows (FJ_ALGO_FULL_OUTER may write every row of both sides)", e.fn, a.cap, np, nb);
        if (outs_misaligned) return set_err("%s: output buffers must be 8-byte aligned", e.fn);
        if (nb && !have_bv) return set_err("%s: FJ_ALGO_FULL_OUTER needs %s (only FJ_ALGO_ROW_IDS reads %s)", e.fn, e.values, e.none);
        if (!a.out_count) return set_err("%s: FJ_ALGO_FULL_OUTER needs out_count (two words: matched probe rows, unmatched build rows)", e.fn);
    }
    if ((f.left || f.anti) && !f.allc) {
        // left outer / anti join (csrc/fj_outer.hip)
        if (f.left && f.anti) return set_err("%s: FJ_ALGO_LEFT_OUTER and FJ_ALGO_ANTI cannot be combined", e.fn);
        if (f.many) return set_err("%s: FJ_ALGO_%s cannot be combined with FJ_ALGO_MANY_TO_MANY", e.fn, f.left ? "LEFT_OUTER" : "ANTI");
        if (f.left && !materialize) return set_err("%s: FJ_ALGO_LEFT_OUTER needs materialize = 1 (its match count is the counting join's)", e.fn);
        if (dev && materialize) {
            if (np && (!a.ok || (f.left && !a.ov))) return set_err("%s: FJ_ALGO_%s needs output buffers (d_out_keys%s)", e.fn, f.left ? "LEFT_OUTER" : "ANTI", f.left ? " and d_out_vals" : "");
            if (a.cap < np) return set_err("%s: output capacity %zu < %zu probe rows (FJ_ALGO_%s writes every probe row)", e.fn, a.cap, np, f.left ? "LEFT_OUTER" : "ANTI");
            if (((uintptr_t)a.ok | (uintptr_t)(f.left ? a.ov : nullptr)) & 7) return set_err("%s: output buffers must be 8-byte aligned", e.fn);
        }
    }
    if (f.base < 0 || f.base > 2) return set_err("%s: unknown algo %d", e.fn, e.host ? f.word : f.base);      // (the host entry has always named the whole word)
    if (dev) {
        if (a.top_bits != 64 && a.top_bits != 48) return set_err("%s: hash_top_bits must be 64 or 48", e.fn);
        if ((nb && (!have_bk || !have_bv)) || (np && !have_pk)) return set_err("%s: null input pointer", e.fn);
        if (((uintptr_t)a.bk | (uintptr_t)bv | (uintptr_t)a.pk) & 15) return set_err("%s: input pointers must be 16-byte aligned", e.fn);
    }
    return 0;
}

}  // namespace fjh
