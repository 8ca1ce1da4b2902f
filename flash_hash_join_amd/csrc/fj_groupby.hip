// fj_groupby.hip -- group-by on ONE relation (an EXTENSION: FJ_ALGO_GROUP_BY, include/flashjoin.h): the distinct keys of a relation,
// densely packed, and optionally one aggregate per key - its row count, the sum / minimum / maximum of a value column, or the position
// of its first occurrence (FJ_ALGO_ROW_IDS: an unsigned minimum over the positions the first pass makes).  DISTINCT, COUNT(DISTINCT)
// and GROUP BY with one aggregate; the reference's first step, "deduplicate the build keys" (hash_join.cpp:125), handed out.
//
// The relation goes through the build side's partition passes (keys only for the distinct and count forms, with the value column or
// the rows' positions otherwise).  One work item is one WHOLE final partition - two slices of a partition would each emit the same
// key - and the kernel builds its table from the stream it aggregates: every row inserts or finds its key in the 8192-slot LDS table
// (CAS, linear probing: the table csrc/fj_lds_table_dev.h states, its insert-or-find loop written out in the kernel) and combines
// into the slot's 8-byte accumulator with one LDS atomic (gj_combine, csrc/fj_group_dev.h).  Then
// the workgroup reserves its g_p output rows on the call's cursor with ONE global atomic and sweeps the table: occupied slots take
// ranks inside the range by wave ballot + popcount on an LDS cursor.  The emit is the only phase that writes to HBM; the order of
// the groups is whatever the cursor and the slots make it.
//
// FJ_ALGO_INVERSE is the inverse of that: beside the distinct keys, the result row of its key - a dense group id - for EVERY row of the
// relation, at the row's own position (fj_group_by_inverse_kernel: the table from the keys, the ranks, then a second sweep over the
// partition's rows).  np.unique(return_inverse=True) / pandas.factorize without the sort.
//
// Float aggregates (FJ_ALGO_AGG_FLOAT: FJ_GJ_SUM_F / FJ_GJ_MIN_F / FJ_GJ_MAX_F): the value column and the accumulators hold IEEE-754
// binary64 in the same words - one native f64 LDS atomic add per row, or one integer atomic on the raw bits for min / max (gj_combine).
//
// Count, sum, minimum and maximum of the value column in ONE call (FJ_ALGO_AGG_ALL) are csrc/fj_groupby_multi.hip's: a 4096-slot table
// with four accumulators per slot; the stream's loads (gb_load_round, csrc/fj_group_dev.h) are shared with it.
//
// Weak spot: a key that owns a large share of the rows is streamed by the one workgroup of its partition, and its LDS atomics hit
// one address; fewer than ~256 distinct keys leave CUs idle.  Correct at any distribution (DESIGN.md "Group-by on one relation").
//
// Fallback: FJ_ERR_LDS_FULL, a partition of more than GJ_LIMIT distinct keys; the HBM-table kernels end this file.
#include "fj_host.h"
#include "fj_group_dev.h"

namespace {

struct GbHdr { u32 full, has_empty, nkeys, cursor; u64 empty_acc, base; };      // 32 B: the key slots behind it stay 16-byte aligned

// AGG (FJ_GJ_*): FJ_GJ_COUNT adds 1 per row; every other form combines the row's value - a.rel.vals, or the row's flat index where the
// zero-pass plan carries positions (FJ_ALGO_ROW_IDS: FJ_GJ_MIN_U over them).  EMIT = false: only g is added to a.cursor (COUNT(DISTINCT):
// no accumulator is touched, no output pointer read).  a.out_vals == nullptr: the keys alone.
template <int AGG, bool EMIT>
__global__ __launch_bounds__(GJ_NT, 1) void fj_group_by_kernel(FjGroupByArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    GbHdr* hdr = reinterpret_cast<GbHdr*>(smem);
    u64* tkeys = reinterpret_cast<u64*>(smem + sizeof(GbHdr));
    u64* acc = tkeys + GJ_TS;
    constexpr bool VALS = AGG != FJ_GJ_COUNT;
    constexpr u64 IDENT = gj_identity<AGG>();
    const u32 tid = threadIdx.x, lane = tid & 63;
    const u32 p = blockIdx.x;
    u32 b0, nbc;
    fj_part_chunks(a.rel, p, b0, nbc);
    if (nbc == 0) return;

    for (u32 i = tid; i < GJ_TS; i += GJ_NT) { tkeys[i] = FJ_EMPTY_KEY; if (EMIT) acc[i] = IDENT; }
    if (tid == 0) { hdr->full = 0; hdr->has_empty = 0; hdr->nkeys = 0; hdr->cursor = 0; hdr->empty_acc = IDENT; hdr->base = 0; }
    __syncthreads();

    // ---- stream: rounds of GJ_NT * GJ_KPT rows; the next round's loads are requested before this round's inserts.  No global
    // store, no barrier inside the loop ----
    u64 k[GJ_KPT], pv[VALS ? GJ_KPT : 1];
    u32 okm = 0;
    auto load_round = [&](u32 c0, u64 (&kk)[GJ_KPT], u64 (&vv)[VALS ? GJ_KPT : 1], u32& ok) {
        ok = 0;
#pragma unroll
        for (u32 u = 0; u < GJ_KPT; ++u) {
            const u32 c = c0 + u * (GJ_NT / FJ_CHUNK) + tid / FJ_CHUNK, off = tid % FJ_CHUNK;
            kk[u] = 0; if (VALS) vv[VALS ? u : 0] = 0;
            if (c >= nbc) continue;
            const u32 e = fj_chunk_entry(a.rel, b0 + c);
            if (off >= FJ_LIST_CNT(e)) continue;
            const u64 src = (u64)FJ_LIST_ID(e) * FJ_CHUNK + off;
            kk[u] = a.rel.keys[src];
            if (VALS) vv[VALS ? u : 0] = a.rel.vals ? a.rel.vals[src] : src;      // (zero-pass plan, positions: the flat index IS the position)
            ok |= 1u << u;
        }
    };
    load_round(0, k, pv, okm);
    for (u32 c0 = 0; c0 < nbc; c0 += GJ_ROUND_CHUNKS) {
        u64 kn[GJ_KPT], pvn[VALS ? GJ_KPT : 1];
        u32 okn = 0;
        if (c0 + GJ_ROUND_CHUNKS < nbc) load_round(c0 + GJ_ROUND_CHUNKS, kn, pvn, okn);
#pragma unroll
        for (u32 u = 0; u < GJ_KPT; ++u) {
            if (!((okm >> u) & 1u)) continue;
            const u64 key = a.rel.list ? k[u] : fj_key_mix(k[u]);                 // chunk pools hold mixed keys, flat arrays raw ones
            const u64 v = VALS ? pv[VALS ? u : 0] : 1ull;
            if (key == FJ_EMPTY_KEY) {                       // the empty marker is never stored in the table
                hdr->has_empty = 1;
                if (EMIT) gj_combine<AGG>(&hdr->empty_acc, v);
                continue;
            }
            if (*(volatile u32*)&hdr->full) continue;        // the item is lost already: the rest of its rows do no table work
            u32 pos = FJ_HW2(key) & (GJ_TS - 1);
            bool placed = false;
            for (u32 step = 0; step < GJ_TS; ++step) {
                u64 t = tkeys[pos];                          // (a slot never changes once it holds a key: a stale read costs a CAS at most)
                if (t == FJ_EMPTY_KEY) {
                    t = atomicCAS((unsigned long long*)&tkeys[pos], (unsigned long long)FJ_EMPTY_KEY, (unsigned long long)key);
                    if (t == FJ_EMPTY_KEY) {
                        if (atomicAdd(&hdr->nkeys, 1u) >= GJ_LIMIT) hdr->full = 1;
                        t = key;
                    }
                }
                if (t == key) { placed = true; break; }
                pos = (pos + 1) & (GJ_TS - 1);
            }
            if (!placed) hdr->full = 1;
            else if (EMIT) gj_combine<AGG>(&acc[pos], v);
        }
#pragma unroll
        for (u32 u = 0; u < GJ_KPT; ++u) { k[u] = kn[u]; if (VALS) pv[VALS ? u : 0] = pvn[VALS ? u : 0]; }
        okm = okn;
    }
    __syncthreads();
    if (hdr->full) { if (tid == 0) atomicOr(a.err, FJ_ERR_LDS_FULL); return; }     // nothing written: the host re-runs the call on the HBM table

    // ---- emit: one global atomic reserves [o, o + g_p); the table's occupied slots take ranks inside it, the marker key the last ----
    const u32 nk = hdr->nkeys;
    const bool has_empty = hdr->has_empty != 0;
    if (tid == 0) hdr->base = (u64)atomicAdd(a.cursor, (unsigned long long)(nk + (has_empty ? 1u : 0u)));
    if (!EMIT) return;
    __syncthreads();
    const u64 o = hdr->base;
    for (u32 i = tid; i < GJ_TS; i += GJ_NT) {               // (GJ_TS is a multiple of GJ_NT: whole waves every round)
        const u64 key = tkeys[i];
        const bool occ = key != FJ_EMPTY_KEY;
        const unsigned long long m = __ballot(occ);
        u32 wbase = 0;
        if (lane == 0 && m) wbase = atomicAdd(&hdr->cursor, (u32)__popcll(m));
        wbase = __shfl(wbase, 0, 64);
        if (!occ) continue;
        const u64 row = o + wbase + (u32)__popcll(m & ((1ull << lane) - 1ull));
        if (row < a.out_capacity) {
            a.out_keys[row] = fj_key_unmix(key);
            if (a.out_vals) a.out_vals[row] = acc[i];
        } else atomicOr(a.err, FJ_ERR_OUTCAP);
    }
    if (tid == 0 && has_empty) {
        const u64 row = o + nk;
        if (row < a.out_capacity) {
            a.out_keys[row] = fj_key_unmix(FJ_EMPTY_KEY);
            if (a.out_vals) a.out_vals[row] = hdr->empty_acc;
        } else atomicOr(a.err, FJ_ERR_OUTCAP);
    }
}

// ---- the inverse form (FJ_ALGO_INVERSE): the distinct keys as above and, for EVERY row, the result row of its key - the group id - at
// the row's own position (a.rel.vals: the positions the first pass made; flat arrays: the index).  Three phases over one partition:
//   stream 1  the rows' keys build the table (no accumulator work; the plane behind the key slots stays free),
//   rank      the emit above: one global atomic reserves [o, o + g_p), an occupied slot takes rank r by wave ballot, out_keys[o + r] is
//             written and the id o + r is stored in the word behind the slot (the marker key's id, o + nkeys, in the header),
//   stream 2  the same chunks again, keys and positions (L2 / MALL hits: a partition is ~64 KiB): a read-only probe of the finished
//             table - no CAS, no atomic - and out_vals[position] = id, one 8-byte scattered store per row.
// A partition beyond the table skips the last two phases (all threads alike: hdr->full is read behind a barrier) and the host runs the
// call again on the HBM table, which overwrites every id the other partitions wrote from the abandoned cursor.
__global__ __launch_bounds__(GJ_NT, 1) void fj_group_by_inverse_kernel(FjGroupByArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    GbHdr* hdr = reinterpret_cast<GbHdr*>(smem);
    u64* tkeys = reinterpret_cast<u64*>(smem + sizeof(GbHdr));
    u64* ids = tkeys + GJ_TS;                                // written for every occupied slot before stream 2 reads it: no fill
    const u32 tid = threadIdx.x, lane = tid & 63;
    const u32 p = blockIdx.x;
    u32 b0, nbc;
    fj_part_chunks(a.rel, p, b0, nbc);
    if (nbc == 0) return;

    for (u32 i = tid; i < GJ_TS; i += GJ_NT) tkeys[i] = FJ_EMPTY_KEY;
    if (tid == 0) { hdr->full = 0; hdr->has_empty = 0; hdr->nkeys = 0; hdr->cursor = 0; hdr->empty_acc = 0; hdr->base = 0; }
    __syncthreads();

    // ---- stream 1: the keys alone, the shape of fj_group_by_kernel's stream ----
    {
        u64 k[GJ_KPT], none[1];
        u32 okm = 0;
        gb_load_round<false>(a.rel, b0, nbc, 0, tid, k, none, okm);
        for (u32 c0 = 0; c0 < nbc; c0 += GJ_ROUND_CHUNKS) {
            u64 kn[GJ_KPT];
            u32 okn = 0;
            if (c0 + GJ_ROUND_CHUNKS < nbc) gb_load_round<false>(a.rel, b0, nbc, c0 + GJ_ROUND_CHUNKS, tid, kn, none, okn);
#pragma unroll
            for (u32 u = 0; u < GJ_KPT; ++u) {
                if (!((okm >> u) & 1u)) continue;
                const u64 key = a.rel.list ? k[u] : fj_key_mix(k[u]);
                if (key == FJ_EMPTY_KEY) { hdr->has_empty = 1; continue; }        // the empty marker is never stored in the table
                if (*(volatile u32*)&hdr->full) continue;
                u32 pos = FJ_HW2(key) & (GJ_TS - 1);
                bool placed = false;
                for (u32 step = 0; step < GJ_TS; ++step) {
                    u64 t = tkeys[pos];
                    if (t == FJ_EMPTY_KEY) {
                        t = atomicCAS((unsigned long long*)&tkeys[pos], (unsigned long long)FJ_EMPTY_KEY, (unsigned long long)key);
                        if (t == FJ_EMPTY_KEY) {
                            if (atomicAdd(&hdr->nkeys, 1u) >= GJ_LIMIT) hdr->full = 1;
                            t = key;
                        }
                    }
                    if (t == key) { placed = true; break; }
                    pos = (pos + 1) & (GJ_TS - 1);
                }
                if (!placed) hdr->full = 1;
            }
#pragma unroll
            for (u32 u = 0; u < GJ_KPT; ++u) k[u] = kn[u];
            okm = okn;
        }
    }
    __syncthreads();
    if (hdr->full) { if (tid == 0) atomicOr(a.err, FJ_ERR_LDS_FULL); return; }     // (uniform: every thread reads the word behind the barrier)

    // ---- reserve and rank: the emit of fj_group_by_kernel; the slot's result row stays behind it in LDS ----
    const u32 nk = hdr->nkeys;
    const bool has_empty = hdr->has_empty != 0;
    if (tid == 0) {
        const u64 o0 = (u64)atomicAdd(a.cursor, (unsigned long long)(nk + (has_empty ? 1u : 0u)));
        hdr->base = o0; hdr->empty_acc = o0 + nk;
    }
    __syncthreads();
    const u64 o = hdr->base;
    for (u32 i = tid; i < GJ_TS; i += GJ_NT) {               // (GJ_TS is a multiple of GJ_NT: whole waves every round)
        const u64 key = tkeys[i];
        const bool occ = key != FJ_EMPTY_KEY;
        const unsigned long long m = __ballot(occ);
        u32 wbase = 0;
        if (lane == 0 && m) wbase = atomicAdd(&hdr->cursor, (u32)__popcll(m));
        wbase = __shfl(wbase, 0, 64);
        if (!occ) continue;
        const u64 row = o + wbase + (u32)__popcll(m & ((1ull << lane) - 1ull));
        ids[i] = row;
        if (row < a.out_capacity) a.out_keys[row] = fj_key_unmix(key);
        else atomicOr(a.err, FJ_ERR_OUTCAP);
    }
    if (tid == 0 && has_empty) {
        const u64 row = o + nk;
        if (row < a.out_capacity) a.out_keys[row] = fj_key_unmix(FJ_EMPTY_KEY);
        else atomicOr(a.err, FJ_ERR_OUTCAP);
    }
    __syncthreads();

    // ---- stream 2: every row finds its key's slot in the finished table and stores the slot's id at the row's position ----
    const u64 empty_id = hdr->empty_acc;
    u64 k[GJ_KPT], pv[GJ_KPT];
    u32 okm = 0;
    gb_load_round<true>(a.rel, b0, nbc, 0, tid, k, pv, okm);
    for (u32 c0 = 0; c0 < nbc; c0 += GJ_ROUND_CHUNKS) {
        u64 kn[GJ_KPT], pvn[GJ_KPT];
        u32 okn = 0;
        if (c0 + GJ_ROUND_CHUNKS < nbc) gb_load_round<true>(a.rel, b0, nbc, c0 + GJ_ROUND_CHUNKS, tid, kn, pvn, okn);
#pragma unroll
        for (u32 u = 0; u < GJ_KPT; ++u) {
            if (!((okm >> u) & 1u)) continue;
            const u64 key = a.rel.list ? k[u] : fj_key_mix(k[u]);
            u64 id = empty_id;
            if (key != FJ_EMPTY_KEY) {
                u32 pos = FJ_HW2(key) & (GJ_TS - 1);
                for (u32 step = 0; step < GJ_TS && tkeys[pos] != key; ++step) pos = (pos + 1) & (GJ_TS - 1);      // (stream 1 placed every key)
                id = ids[pos];
            }
            if (pv[u] < a.out_capacity) a.out_vals[pv[u]] = id;
            else atomicOr(a.err, FJ_ERR_OUTCAP);
        }
#pragma unroll
        for (u32 u = 0; u < GJ_KPT; ++u) { k[u] = kn[u]; pv[u] = pvn[u]; }
        okm = okn;
    }
}

// ---- the global-table form.  The table is fj_gt_build_first_kernel's (csrc/fj_join.hip: raw keys, the raw empty key out of band);
// the accumulators are capacity + 1 words holding the aggregate's identity, the last one the empty key's ----
// thread per row of the relation: one typed global atomic on the slot of the row's key (the build placed every key)
template <int AGG>
__global__ __launch_bounds__(1024) void fj_gt_group_by_combine_kernel(FjGtArgs a, const u64* __restrict__ vals, u64* acc) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < a.nb; i += stride) {
        const u64 key = a.bk[i];
        u64 where = a.cap_mask + 1;
        if (key != FJ_EMPTY_KEY && !gj_gt_find(a.tkeys, a.cap_mask, key, where)) continue;
        gj_combine<AGG>(&acc[where], AGG == FJ_GJ_COUNT ? 1ull : vals[i]);
    }
}

// the capacity + 1 slots, compacted: an occupied slot's (key, accumulator) goes to the row a wave-aggregated cursor hands out (one
// global atomic per wave that holds a key).  out_keys == nullptr: the cursor alone (COUNT(DISTINCT)); acc == nullptr: the keys alone.
// IDS (the inverse form; out_vals is not written here): the row a slot receives is also stored in ids[slot], capacity + 1 words
template <bool IDS>
__global__ __launch_bounds__(1024) void fj_gt_group_by_sweep_kernel(FjGtArgs a, const u64* __restrict__ acc, u64* __restrict__ out_keys,
                                                                    u64* __restrict__ out_vals, u64 out_capacity, unsigned long long* cursor, u32* err,
                                                                    u64* __restrict__ ids) {
    const u64 cap = a.cap_mask + 1;
    const bool has_empty = a.flags[0] != 0;
    const u32 lane = threadIdx.x & 63;
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 w0 = (u64)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); w0 <= cap; w0 += stride) {     // (uniform per wave)
        const u64 i = w0 + lane;
        const u64 key = i < cap ? a.tkeys[i] : FJ_EMPTY_KEY;
        const bool occ = i < cap ? key != FJ_EMPTY_KEY : (i == cap && has_empty);
        const unsigned long long m = __ballot(occ);
        if (!m) continue;
        unsigned long long wbase = 0;
        if (lane == 0) wbase = atomicAdd(cursor, (unsigned long long)__popcll(m));
        wbase = __shfl(wbase, 0, 64);
        if (!occ || !out_keys) continue;
        const u64 row = wbase + (u32)__popcll(m & ((1ull << lane) - 1ull));
        if (IDS) ids[i] = row;
        if (row < out_capacity) {
            out_keys[row] = key;
            if (!IDS && out_vals) out_vals[row] = acc[i];
        } else atomicOr(err, FJ_ERR_OUTCAP);
    }
}

// the inverse form's last step, behind the sweep on the same stream: thread per row of the relation, out_vals[i] = the row the sweep
// handed to the slot of row i's key (the build placed every key; the empty key's id is the plane's last word)
__global__ __launch_bounds__(1024) void fj_gt_group_by_inverse_kernel(FjGtArgs a, const u64* __restrict__ ids, u64* __restrict__ out_vals,
                                                                      u64 out_capacity) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    const u64 n = a.nb < out_capacity ? a.nb : out_capacity;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const u64 key = a.bk[i];
        u64 where = a.cap_mask + 1;
        if (key != FJ_EMPTY_KEY && !gj_gt_find(a.tkeys, a.cap_mask, key, where)) continue;
        out_vals[i] = ids[where];
    }
}

template <bool EMIT> hipError_t launch_lds(const FjGroupByArgs& a, int agg, hipStream_t s) {
    const u32 lds = (u32)sizeof(GbHdr) + GJ_TS * 16u;
    void (*kern)(FjGroupByArgs);
    if constexpr (EMIT) kern = fjh::for_agg(agg, [](auto A) { return fj_group_by_kernel<FJ_V(A), true>; });
    else kern = fj_group_by_kernel<FJ_GJ_COUNT, false>;
    hipError_t e = fj_set_max_lds_once(reinterpret_cast<const void*>(kern), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(a.nparts), dim3(GJ_NT), lds, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t fj_launch_group_by(const FjGroupByArgs& a, int agg, bool emit, hipStream_t s) {
    if (agg < FJ_GJ_COUNT || agg > FJ_GJ_LAST || !a.cursor || !a.err || !a.nparts) return hipErrorInvalidValue;
    if (emit && !a.out_keys) return hipErrorInvalidValue;
    if (!emit && agg != FJ_GJ_COUNT) return hipErrorInvalidValue;                 // (the total needs no aggregate)
    return emit ? launch_lds<true>(a, agg, s) : launch_lds<false>(a, agg, s);
}

hipError_t fj_launch_group_by_inverse(const FjGroupByArgs& a, hipStream_t s) {
    if (!a.cursor || !a.err || !a.nparts || !a.out_keys || !a.out_vals) return hipErrorInvalidValue;
    const u32 lds = (u32)sizeof(GbHdr) + GJ_TS * 16u;
    hipError_t e = fj_set_max_lds_once(reinterpret_cast<const void*>(fj_group_by_inverse_kernel), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fj_group_by_inverse_kernel, dim3(a.nparts), dim3(GJ_NT), lds, s, a);
    return hipGetLastError();
}

hipError_t fj_launch_gt_group_by_combine(const FjGtArgs& a, int agg, const u64* vals, u64* acc, hipStream_t s) {
    if (agg < FJ_GJ_COUNT || agg > FJ_GJ_LAST || !acc || (agg != FJ_GJ_COUNT && !vals)) return hipErrorInvalidValue;
    if (!a.nb) return hipSuccess;
    void (*kern)(FjGtArgs, const u64*, u64*) = fjh::for_agg(agg, [](auto A) { return fj_gt_group_by_combine_kernel<FJ_V(A)>; });
    hipLaunchKernelGGL(kern, dim3(fjh::gt_grid(a.nb)), dim3(1024), 0, s, a, vals, acc);
    return hipGetLastError();
}

hipError_t fj_launch_gt_group_by_sweep(const FjGtArgs& a, const u64* acc, u64* out_keys, u64* out_vals, u64 out_capacity,
                                       unsigned long long* cursor, u32* err, hipStream_t s, u64* ids) {
    if (!cursor || !err || (out_vals && (!acc || !out_keys)) || (ids && (!out_keys || out_vals))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ids ? fj_gt_group_by_sweep_kernel<true> : fj_gt_group_by_sweep_kernel<false>, dim3(fjh::gt_grid(a.cap_mask + 2)),
                       dim3(1024), 0, s, a, acc, out_keys, out_vals, out_capacity, cursor, err, ids);
    return hipGetLastError();
}

hipError_t fj_launch_gt_group_by_inverse(const FjGtArgs& a, const u64* ids, u64* out_vals, u64 out_capacity, hipStream_t s) {
    if (!ids || !out_vals) return hipErrorInvalidValue;
    if (!a.nb) return hipSuccess;
    hipLaunchKernelGGL(fj_gt_group_by_inverse_kernel, dim3(fjh::gt_grid(a.nb)), dim3(1024), 0, s, a, ids, out_vals, out_capacity);
    return hipGetLastError();
}

namespace fjh {

// the global-table form (fj_host.h).  rid: the table build itself keeps every key's first row index (fj_gt_build_first_kernel with
// values), so the accumulators are its value plane and no combine pass runs.  inv: the value plane receives the row the sweep hands to
// every slot instead, and one more kernel, behind the sweep on the same stream, stores every row's id at the row's position: all nb
// words of d_ov, whatever an abandoned partitioned attempt left there.
static int group_by_global(fj_ctx* c, const u64* bk, const u64* bv, size_t nb, hipStream_t s, fj_timings* t, u64* out_count,
                           u64* d_ok, u64* d_ov, size_t cap_out, int agg, bool rid, bool inv) {
    const u64 cap = gt_capacity(nb);
    FjGtArgs a{};
    u64* acc = nullptr;
    if (gt_open(c, nb, d_ov ? cap + 1 : 0, s, &a, &acc)) return 1;
    a.bk = bk;
    if (inv) HIPCHK(fj_launch_gt_build_first(a, false, s));  // (the id plane needs no fill: the sweep writes every word that is read)
    else if (acc && rid) {                                   // (row index minimum: all ones at rest; the empty key's word is the table's last)
        a.tvals = acc; a.empty_val = acc + cap;
        HIPCHK(hipMemsetAsync(acc, 0xFF, (cap + 1) * 8, s));
        HIPCHK(fj_launch_gt_build_first(a, true, s));
    } else {
        HIPCHK(fj_launch_gt_build_first(a, false, s));
        if (acc) {
            HIPCHK(fj_launch_group_fill(acc, cap + 1, agg, s));
            HIPCHK(fj_launch_gt_group_by_combine(a, agg, bv, acc, s));
        }
    }
    HIPCHK(hipEventRecord(c->ev[E_BUILD], s));
    HIPCHK(hipEventRecord(c->ev[E_PPART], s));
    if (inv) {
        HIPCHK(fj_launch_gt_group_by_sweep(a, nullptr, d_ok, nullptr, cap_out, &c->d_sc->total, &c->d_sc->err, s, acc));
        HIPCHK(fj_launch_gt_group_by_inverse(a, acc, d_ov, cap_out, s));
    } else HIPCHK(fj_launch_gt_group_by_sweep(a, acc, d_ok, d_ov, cap_out, &c->d_sc->total, &c->d_sc->err, s));
    if (gt_close(c, s, t)) return 1;
    if (c->h_sc->err & FJ_ERR_OUTCAP) return distinct_error();
    *out_count = c->h_sc->total;
    return 0;
}

// FJ_ALGO_GROUP_BY (fj_join_device has checked the arguments): the g distinct keys of bk[0 .. nb) in d_ok and their aggregates in d_ov
// (null: the keys alone), g <= nb <= cap_out rows; d_ok == nullptr: *out_count = g alone (COUNT(DISTINCT), a keys-only pass).  agg:
// FJ_GJ_COUNT (bv is not read), FJ_GJ_SUM or a min / max form over bv; rid: the first occurrence's position instead (bv is not read).
// use_radix: the partitioned plan, else the global table.  inv (FJ_ALGO_INVERSE; d_ok and d_ov given, no aggregate): d_ov receives
// nb words instead, the group id of every row at the row's position (bv is not read).
int group_by(fj_ctx* c, bool use_radix, const u64* bk, const u64* bv, size_t nb, int top_bits, hipStream_t s, fj_timings* t,
             u64* out_count, u64* d_ok, u64* d_ov, size_t cap_out, int agg, bool rid, bool inv) {
    *out_count = 0;
    if (nb == 0) return 0;
    if (!d_ok) d_ov = nullptr;
    if (!d_ov) { agg = FJ_GJ_COUNT; rid = false; inv = false; }      // no aggregate leaves the call: nothing travels beside the keys
    if (inv) rid = false;
    if (rid) agg = FJ_GJ_MIN_U;
    if (!use_radix) return group_by_global(c, bk, bv, nb, s, t, out_count, d_ok, d_ov, cap_out, agg, rid, inv);

    RelAttempt r;
    const RelBeside beside = (rid || inv) ? REL_POSITIONS : agg != FJ_GJ_COUNT ? REL_VALUES : REL_KEYS_ONLY;
    if (rel_open(c, bk, beside, bv, nb, top_bits, 0, s, &r)) return 1;
    FjGroupByArgs ga{};
    ga.rel = r.rel; ga.nparts = r.nparts;
    ga.out_keys = d_ok; ga.out_vals = d_ov; ga.out_capacity = cap_out;
    ga.cursor = &c->d_sc->total; ga.err = &c->d_sc->err;
    if (inv) HIPCHK(fj_launch_group_by_inverse(ga, s));
    else HIPCHK(fj_launch_group_by(ga, agg, d_ok != nullptr, s));
    if (rel_close(c, r.plan, r.nparts, s, t)) return 1;
    if (c->h_sc->err & FJ_ERR_LDS_FULL)                      // a partition beyond the LDS table: the whole call on the HBM table
        return gt_fallback(t, [&](fj_timings* g) { return group_by_global(c, bk, bv, nb, s, g, out_count, d_ok, d_ov, cap_out, agg, rid, inv); });
    if (c->h_sc->err & FJ_ERR_OUTCAP) return distinct_error();
    *out_count = c->h_sc->total;
    return 0;
}

}  // namespace fjh
