// fj_entry.h -- what the two join entry points, fj_join_device (fj_joins.hip) and fj_join_host (fj_hostentry.hip), share before any
// device work: the `algo` word decoded ONCE, and the ONE list of refusals that need no context (fj_entry.hip).  Host code only.
// A new FJ_ALGO_* flag is decoded in decode_algo, refused in check_entry and, where the host entry returns a new shape for it,
// described in host_result (fj_hostentry.hip): nowhere else.
#pragma once
#include <cstddef>

namespace fjh {

struct AlgoForm {
    int word;                                   // the algo word as the caller gave it
    int base;                                   // ... without every flag it was recognised to carry: FJ_ALGO_ADAPTIVE / _SCALAR / _RADIX, anything else is an unknown algo
    bool many, left, anti, rid, full, allc, po, bo, gb;
    bool inv, kpair, grows, aall, aarg;         // modifiers of FJ_ALGO_GROUP_BY (false without it: the bit then stays in `base`)
    bool amerge;                                // ... of FJ_ALGO_GROUP_BY | FJ_ALGO_AGG_ALL: the build side is partial rows with four planes
    bool pagg;                                  // FJ_ALGO_KEY_PAIR | FJ_ALGO_AGG_ALL without FJ_ALGO_INVERSE: the pairs and four aggregates of a THIRD column, the probe keys
    bool retain, reuse;                         // modifiers of FJ_ALGO_PROBE_ORDER
    bool bo_reuse, accum;                       // FJ_ALGO_BUILD_ORDER | FJ_ALGO_REUSE_BUILD, and FJ_ALGO_ACCUMULATE beside that pair
    bool amin, amax, asigned, afloat;           // modifiers of FJ_ALGO_BUILD_ORDER / FJ_ALGO_GROUP_BY
    int agg;                                    // FJ_GJ_*: what the value output of those two receives (the count form of a group-by without a value column is the caller's: it depends on a pointer)
    int kind;                                   // the value column holds uint64 (0), int64 (1) or binary64 (2) words
};
AlgoForm decode_algo(int algo);

// The forms that read no build value - always, or when none is given: fj_join_device passes d_build_keys on in its place, and the checks
// of the input pointers look at that pointer.
inline bool build_vals_unread(const AlgoForm& f, bool given) {
    return f.gb ? (!given || f.rid || f.inv || f.grows) : (!given && (f.bo || f.po || f.rid || (f.anti && !f.left && !f.allc)));
}

// The calling entry's words: its name, its names for the five pointers and for the rows of a plane of the value output, and how it has
// always said "the build values" and "none of them" (tests pin both entries' words).
struct EntryWords { const char *fn, *bk, *bv, *pk, *ok, *ov, *plane, *values, *none; bool host; };
extern const EntryWords DEVICE_ENTRY, HOST_ENTRY;

// What a call brings besides the algo word.  The pointers are compared with null and, for the device entry, looked at for their
// alignment; none is dereferenced.  The host entry leaves cap and top_bits at their defaults.
struct EntryArgs {
    int materialize;
    const void *bk, *bv; size_t nb;
    const void* pk; size_t np;
    const void *out_count, *ok, *ov;
    size_t cap = 0; int top_bits = 64;
};
int check_entry(const AlgoForm& f, const EntryWords& e, const EntryArgs& a);      // 0, or set_err's 1 with the refusal in fj_last_error()

}  // namespace fjh
