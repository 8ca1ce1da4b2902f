// fj_group_dev.h -- device-side pieces shared by the two users of the 8192-slot LDS table with one 8-byte accumulator per slot:
// the build-order aggregate joins (csrc/fj_group.hip) and the group-by on one relation (csrc/fj_groupby.hip).  The table itself -
// home slot, probing, what an insert and a find may assume - is STATED in csrc/fj_lds_table_dev.h; the insert and find loops
// are written out in each kernel (that header says why).  Here are the aggregates.
#pragma once
#include "fj_lds_table_dev.h"

constexpr u32 GJ_NT = 1024, GJ_KPT = 8, GJ_ROUND_CHUNKS = GJ_NT * GJ_KPT / FJ_CHUNK;
constexpr u32 GJ_TS = 8192, GJ_LIMIT = GJ_TS - GJ_TS / 16;

__device__ __forceinline__ u64 gj_wave_sum64(u64 v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (u64)__shfl_xor((unsigned long long)v, d, 64);
    return v;
}

// the aggregate's identity: what an accumulator holds before its first hit and a build row without a partner receives
template <int AGG> __host__ __device__ __forceinline__ constexpr u64 gj_identity() {
    return AGG == FJ_GJ_MIN_U ? ~0ull : AGG == FJ_GJ_MIN_S ? 0x7FFFFFFFFFFFFFFFull : AGG == FJ_GJ_MAX_S ? 0x8000000000000000ull :
           AGG == FJ_GJ_MIN_F ? 0x7FF0000000000000ull : AGG == FJ_GJ_MAX_F ? 0xFFF0000000000000ull : 0ull;      // (+inf, -inf; the float sum: +0.0)
}

// one atomic of the aggregate's own type on an accumulator, in LDS or in HBM (count and sum: the add; min / max: the native 64-bit
// atomic of the value's signedness - no transform of the words, so nothing to undo afterwards).
// The float forms (the word holds an IEEE-754 binary64): the sum is the native f64 atomic add - p must be LDS or ordinary device
// memory.  Min / max work on the raw bits, split by the value's sign BIT (not v >= 0: -0.0 has it set): doubles of a clear sign
// order like int64, doubles of a set sign order backwards as uint64 and lie below every one of a clear sign.  So a minimum is the
// signed integer minimum for a value of a clear sign (an accumulator of a set sign is negative as int64 and stays) and the unsigned
// integer MAXIMUM for one of a set sign (an accumulator of a clear sign is smaller as uint64 and gives way); the maximum is the
// mirror image.  One integer atomic either way, no transform of the words: it works in place on a caller's running aggregate.
template <int AGG> __device__ __forceinline__ void gj_combine(u64* p, u64 v) {
    if constexpr (AGG == FJ_GJ_MIN_U) atomicMin((unsigned long long*)p, (unsigned long long)v);
    else if constexpr (AGG == FJ_GJ_MIN_S) atomicMin((long long*)p, (long long)v);
    else if constexpr (AGG == FJ_GJ_MAX_U) atomicMax((unsigned long long*)p, (unsigned long long)v);
    else if constexpr (AGG == FJ_GJ_MAX_S) atomicMax((long long*)p, (long long)v);
    else if constexpr (AGG == FJ_GJ_SUM_F) atomicAdd(reinterpret_cast<double*>(p), __longlong_as_double((long long)v));
    else if constexpr (AGG == FJ_GJ_MIN_F) {
        if (v >> 63) atomicMax((unsigned long long*)p, (unsigned long long)v);
        else atomicMin((long long*)p, (long long)v);
    } else if constexpr (AGG == FJ_GJ_MAX_F) {
        if (v >> 63) atomicMin((unsigned long long*)p, (unsigned long long)v);
        else atomicMax((long long*)p, (long long)v);
    }
    else atomicAdd((unsigned long long*)p, (unsigned long long)v);
}

// one round of a partition's stream for the group-by kernels (csrc/fj_groupby.hip, csrc/fj_groupby_multi.hip): GJ_KPT rows per thread
// from the chunks [c0, c0 + GJ_ROUND_CHUNKS) of the partition's nbc chunks behind chunk-list entry b0 - the keys, and with POS the word
// that travels beside each (rel.vals: the value column or the positions the first pass made; flat arrays without one: the row's index).
// ok: one bit per row that exists.  Loads only: the callers request the next round before they work on this one
template <bool POS>
__device__ __forceinline__ void gb_load_round(const FjChunkSet& rel, u32 b0, u32 nbc, u32 c0, u32 tid, u64 (&kk)[GJ_KPT],
                                              u64 (&vv)[POS ? GJ_KPT : 1], u32& ok) {
    ok = 0;
#pragma unroll
    for (u32 u = 0; u < GJ_KPT; ++u) {
        const u32 c = c0 + u * (GJ_NT / FJ_CHUNK) + tid / FJ_CHUNK, off = tid % FJ_CHUNK;
        kk[u] = 0; if (POS) vv[POS ? u : 0] = 0;
        if (c >= nbc) continue;
        const u32 e = fj_chunk_entry(rel, b0 + c);
        if (off >= FJ_LIST_CNT(e)) continue;
        const u64 src = (u64)FJ_LIST_ID(e) * FJ_CHUNK + off;
        kk[u] = rel.keys[src];
        if (POS) vv[POS ? u : 0] = rel.vals ? rel.vals[src] : src;                // (zero-pass plan: the flat index IS the position)
        ok |= 1u << u;
    }
}

// ---- the global-table form.  The table is fj_gt_build_first_kernel's, keys only (csrc/fj_join.hip: group-aligned home slot, linear
// probing, the raw empty key out of band); the accumulators are arrays of capacity + 1 words, the last one the empty key's ----
__device__ __forceinline__ bool gj_gt_find(const u64* __restrict__ tkeys, u64 cap_mask, u64 key, u64& where) {
    u64 pos = (fj_hash64(key) & cap_mask) & ~(u64)(FJ_GT_GROUP - 1);
    for (u64 step = 0; step <= cap_mask; ++step) {
        const u64 t = tkeys[pos];
        if (t == key) { where = pos; return true; }
        if (t == FJ_EMPTY_KEY) return false;
        pos = (pos + 1) & cap_mask;
    }
    return false;
}
