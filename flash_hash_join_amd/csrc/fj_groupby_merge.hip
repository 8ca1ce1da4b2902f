// fj_groupby_merge.hip -- MERGE of partial group-by results (an EXTENSION: FJ_ALGO_GROUP_BY | FJ_ALGO_AGG_ALL | FJ_ALGO_AGG_MERGE,
// include/flashjoin.h).  The input is not a relation but rows that are already aggregates: a key and beside it a row count, a sum, a
// minimum and a maximum - what FJ_ALGO_AGG_ALL wrote for one batch, one shard or one slice of a hot partition.  Rows that share a key
// are combined: the counts and the sums add, the minima and maxima take the extreme.  The output is FJ_ALGO_AGG_ALL's.  This is what a
// running GROUP BY over morsels, a group-by over shards and a pre-aggregated hot key all need (DESIGN.md "Merging partial group-bys").
//
// A pass carries ONE payload plane beside the keys and a partial row has four.  The passes carry the rows' POSITIONS
// (PassIter::vals_pos, as FJ_ALGO_AGG_ARG does) and the kernel reads vals[q * nb + position] for the four planes q itself: four 8-byte
// random gathers per row on a partitioned plan; on a zero-pass plan the position is the flat index and the reads are coalesced.
//
// The kernel is fj_group_by_all_kernel's with a 64-bit count: one workgroup per WHOLE final partition, the LDS table of
// csrc/fj_lds_table_dev.h (home slot FJ_HW2(key) & (TS - 1), linear probing, one 64-bit CAS per claim, inserts bounded by TS steps,
// `full` behind LIMIT = TS - TS / 16, the marker key out of band in the header with four accumulators of its own).
//
// LDS budget, TS = 2048 slots (LIMIT 1920):  key 8 B + count 8 B + sum 8 B + min 8 B + max 8 B = 40 B per slot,
//   40 B * 2048 = 81 920 B, + the 64-byte header = 81 984 B of the 163 840 B one workgroup may take.
// The u32 count of fj_group_by_all_kernel is safe because a partition holds fewer than 2^32 ROWS; a partial row carries any count, so
// the plane is 8 bytes here, and five 8-byte planes over 4096 slots are 163 840 B before the header.  So 2048 slots, and the plan aims
// at 1024 rows per partition - one radix bit more than the four-aggregate form takes.
//
// The stream loop has no barrier and no global store.  The next round's keys and positions are requested before this round's inserts,
// its gathers behind them.  The emit is fj_group_by_all_kernel's: one global atomic reserves the partition's rows on the call's cursor,
// ballot + popcount ranks the occupied slots, a slot writes its key and its four aggregates at stride out_capacity.
//
// Fallback: FJ_ERR_LDS_FULL, a partition of more than 1920 distinct keys, which writes nothing; the HBM-table
// kernels end this file.
//
// Weak spot: a hot key's partial rows are still one workgroup's and its four LDS atomics per row hit four addresses - but a hot key now
// has one row per batch (shard, slice), not one per input row.  Correct at any distribution.
#include "fj_host.h"
#include "fj_group_dev.h"

namespace {

constexpr u32 GM_TS = 2048, GM_LIMIT = GM_TS - GM_TS / 16;
using fjh::KIND_UNSIGNED; using fjh::KIND_SIGNED; using fjh::KIND_FLOAT;        // the `kind` of the value column (fj_host.h)

// 64 B: the key slots behind it stay 16-byte aligned.  empty_*: the marker key's accumulators
struct GmHdr { u32 full, has_empty, nkeys, cursor; u64 empty_cnt, empty_sum, empty_min, empty_max, base, pad; };
static_assert(sizeof(GmHdr) == 64, "GmHdr");
constexpr u32 GM_LDS = (u32)sizeof(GmHdr) + GM_TS * 40u;
static_assert(GM_LDS == 81984u && GM_LDS <= 163840u, "the table must fit one workgroup's LDS");
static_assert(GM_TS % GJ_NT == 0, "the emit sweeps whole waves");

template <int KIND> struct GmAgg {
    static constexpr int SUM = KIND == KIND_FLOAT ? FJ_GJ_SUM_F : FJ_GJ_SUM;
    static constexpr int MIN = KIND == KIND_FLOAT ? FJ_GJ_MIN_F : KIND == KIND_SIGNED ? FJ_GJ_MIN_S : FJ_GJ_MIN_U;
    static constexpr int MAX = KIND == KIND_FLOAT ? FJ_GJ_MAX_F : KIND == KIND_SIGNED ? FJ_GJ_MAX_S : FJ_GJ_MAX_U;
};

// Rounds of FOUR rows per thread, as in fj_group_by_arg_kernel: a row in flight is its key, its position and FOUR gathered words, and
// this round's 24 words with the next round's 8 fit the 128 VGPRs of a 1024-thread workgroup without scratch (77 VGPRs; 56 at two
// rows: profiles/group_by_merge_kernel_resources.txt).  A round covers 16 chunks, so the plan's 1024-row partition is one round also
// where the passes left it in partial chunks
constexpr u32 GM_KPT = 4, GM_ROUND_CHUNKS = GJ_NT * GM_KPT / FJ_CHUNK;
__device__ __forceinline__ void gm_load_round(const FjChunkSet& rel, u32 b0, u32 nbc, u32 c0, u32 tid, u64 (&kk)[GM_KPT], u64 (&pp)[GM_KPT], u32& ok) {
    ok = 0;
#pragma unroll
    for (u32 u = 0; u < GM_KPT; ++u) {
        const u32 c = c0 + u * (GJ_NT / FJ_CHUNK) + tid / FJ_CHUNK, off = tid % FJ_CHUNK;
        kk[u] = 0; pp[u] = 0;
        if (c >= nbc) continue;
        const u32 e = fj_chunk_entry(rel, b0 + c);
        if (off >= FJ_LIST_CNT(e)) continue;
        const u64 src = (u64)FJ_LIST_ID(e) * FJ_CHUNK + off;
        kk[u] = rel.keys[src];
        pp[u] = rel.vals ? rel.vals[src] : src;              // (zero-pass plan: the flat index IS the position)
        ok |= 1u << u;
    }
}

// the four words of one round's rows: planes[q * nrows + position].  A position at or beyond nrows (the passes make none) is not read
__device__ __forceinline__ void gm_gather(const u64* __restrict__ planes, u64 nrows, const u64 (&ps)[GM_KPT], u32& ok, u64 (&v)[GM_KPT][4], u32* err) {
#pragma unroll
    for (u32 u = 0; u < GM_KPT; ++u) {
#pragma unroll
        for (u32 q = 0; q < 4; ++q) v[u][q] = 0;
        if (!((ok >> u) & 1u)) continue;
        if (ps[u] < nrows) {
#pragma unroll
            for (u32 q = 0; q < 4; ++q) v[u][q] = planes[q * nrows + ps[u]];
        } else { ok &= ~(1u << u); atomicOr(err, FJ_ERR_OUTCAP); }
    }
}

// a.rel.vals: the rows' positions (the first pass made them; flat arrays: the index); planes: four planes of nrows words - count, sum,
// min, max of every partial row.  a.out_vals: four planes of a.out_capacity words, the same order
template <int KIND>
__global__ __launch_bounds__(GJ_NT, 1) void fj_group_by_merge_kernel(FjGroupByArgs a, const u64* __restrict__ planes, u64 nrows) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    GmHdr* hdr = reinterpret_cast<GmHdr*>(smem);
    u64* tkeys = reinterpret_cast<u64*>(smem + sizeof(GmHdr));
    u64* acnt = tkeys + GM_TS;
    u64* asum = acnt + GM_TS;
    u64* amin = asum + GM_TS;
    u64* amax = amin + GM_TS;
    using A = GmAgg<KIND>;
    constexpr u64 ID_SUM = gj_identity<A::SUM>(), ID_MIN = gj_identity<A::MIN>(), ID_MAX = gj_identity<A::MAX>();
    const u32 tid = threadIdx.x, lane = tid & 63;
    const u32 p = blockIdx.x;
    u32 b0, nbc;
    fj_part_chunks(a.rel, p, b0, nbc);
    if (nbc == 0) return;

    for (u32 i = tid; i < GM_TS; i += GJ_NT) { tkeys[i] = FJ_EMPTY_KEY; acnt[i] = 0; asum[i] = ID_SUM; amin[i] = ID_MIN; amax[i] = ID_MAX; }
    if (tid == 0) {
        hdr->full = 0; hdr->has_empty = 0; hdr->nkeys = 0; hdr->cursor = 0; hdr->empty_cnt = 0;
        hdr->empty_sum = ID_SUM; hdr->empty_min = ID_MIN; hdr->empty_max = ID_MAX; hdr->base = 0;
    }
    __syncthreads();

    // ---- stream: rounds of GJ_NT * GM_KPT rows; the next round's keys and positions are requested before this round's inserts, its
    // four words behind them.  No global store, no barrier inside the loop ----
    u64 k[GM_KPT], ps[GM_KPT], v[GM_KPT][4];
    u32 okm = 0;
    gm_load_round(a.rel, b0, nbc, 0, tid, k, ps, okm);
    gm_gather(planes, nrows, ps, okm, v, a.err);
    for (u32 c0 = 0; c0 < nbc; c0 += GM_ROUND_CHUNKS) {
        const bool more = c0 + GM_ROUND_CHUNKS < nbc;
        u64 kn[GM_KPT], pn[GM_KPT];
        u32 okn = 0;
        if (more) gm_load_round(a.rel, b0, nbc, c0 + GM_ROUND_CHUNKS, tid, kn, pn, okn);
#pragma unroll
        for (u32 u = 0; u < GM_KPT; ++u) {
            if (!((okm >> u) & 1u)) continue;
            const u64 key = a.rel.list ? k[u] : fj_key_mix(k[u]);                 // chunk pools hold mixed keys, flat arrays raw ones
            if (key == FJ_EMPTY_KEY) {                       // the empty marker is never stored in the table
                hdr->has_empty = 1;
                atomicAdd((unsigned long long*)&hdr->empty_cnt, (unsigned long long)v[u][0]);
                gj_combine<A::SUM>(&hdr->empty_sum, v[u][1]); gj_combine<A::MIN>(&hdr->empty_min, v[u][2]); gj_combine<A::MAX>(&hdr->empty_max, v[u][3]);
                continue;
            }
            if (*(volatile u32*)&hdr->full) continue;        // the item is lost already: the rest of its rows do no table work
            u32 pos = FJ_HW2(key) & (GM_TS - 1);
            bool placed = false;
            for (u32 step = 0; step < GM_TS; ++step) {
                u64 t = tkeys[pos];                          // (a slot never changes once it holds a key: a stale read costs a CAS at most)
                if (t == FJ_EMPTY_KEY) {
                    t = atomicCAS((unsigned long long*)&tkeys[pos], (unsigned long long)FJ_EMPTY_KEY, (unsigned long long)key);
                    if (t == FJ_EMPTY_KEY) {
                        if (atomicAdd(&hdr->nkeys, 1u) >= GM_LIMIT) hdr->full = 1;
                        t = key;
                    }
                }
                if (t == key) { placed = true; break; }
                pos = (pos + 1) & (GM_TS - 1);
            }
            if (!placed) { hdr->full = 1; continue; }
            atomicAdd((unsigned long long*)&acnt[pos], (unsigned long long)v[u][0]);      // (64 bits: a partial row carries any count)
            gj_combine<A::SUM>(&asum[pos], v[u][1]); gj_combine<A::MIN>(&amin[pos], v[u][2]); gj_combine<A::MAX>(&amax[pos], v[u][3]);
        }
        if (more) {
#pragma unroll
            for (u32 u = 0; u < GM_KPT; ++u) { k[u] = kn[u]; ps[u] = pn[u]; }
            okm = okn;
            gm_gather(planes, nrows, ps, okm, v, a.err);
        }
    }
    __syncthreads();
    if (hdr->full) { if (tid == 0) atomicOr(a.err, FJ_ERR_LDS_FULL); return; }     // nothing written: the host re-runs the call on the HBM table

    // ---- emit: one global atomic reserves [o, o + g_p); the table's occupied slots take ranks inside it, the marker key the last ----
    const u32 nk = hdr->nkeys;
    const bool has_empty = hdr->has_empty != 0;
    if (tid == 0) hdr->base = (u64)atomicAdd(a.cursor, (unsigned long long)(nk + (has_empty ? 1u : 0u)));
    __syncthreads();
    const u64 o = hdr->base, cap = a.out_capacity;
    u64* const ov = a.out_vals;
    for (u32 i = tid; i < GM_TS; i += GJ_NT) {               // (GM_TS is a multiple of GJ_NT: whole waves every round)
        const u64 key = tkeys[i];
        const bool occ = key != FJ_EMPTY_KEY;
        const unsigned long long m = __ballot(occ);
        u32 wbase = 0;
        if (lane == 0 && m) wbase = atomicAdd(&hdr->cursor, (u32)__popcll(m));
        wbase = __shfl(wbase, 0, 64);
        if (!occ) continue;
        const u64 row = o + wbase + (u32)__popcll(m & ((1ull << lane) - 1ull));
        if (row < cap) {
            a.out_keys[row] = fj_key_unmix(key);
            ov[row] = acnt[i]; ov[cap + row] = asum[i]; ov[2 * cap + row] = amin[i]; ov[3 * cap + row] = amax[i];
        } else atomicOr(a.err, FJ_ERR_OUTCAP);
    }
    if (tid == 0 && has_empty) {
        const u64 row = o + nk;
        if (row < cap) {
            a.out_keys[row] = fj_key_unmix(FJ_EMPTY_KEY);
            ov[row] = hdr->empty_cnt; ov[cap + row] = hdr->empty_sum; ov[2 * cap + row] = hdr->empty_min; ov[3 * cap + row] = hdr->empty_max;
        } else atomicOr(a.err, FJ_ERR_OUTCAP);
    }
}

// ---- the global-table form.  The table is fj_gt_build_first_kernel's, keys only (csrc/fj_join.hip: raw keys, the raw empty key out
// of band); acc: four planes of capacity + 1 words - count, sum, min, max - each holding its identity, the last word the empty key's.
// fj_gt_group_by_all_sweep_kernel (csrc/fj_groupby_multi.hip) compacts them ----
// thread per partial row: coalesced reads of the four planes at i, four typed global atomics on the slot of the row's key (the build
// placed every key); u64 counts
template <int KIND>
__global__ __launch_bounds__(1024) void fj_gt_group_by_merge_combine_kernel(FjGtArgs a, const u64* __restrict__ planes, u64* acc) {
    using A = GmAgg<KIND>;
    const u64 plane = a.cap_mask + 2;
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < a.nb; i += stride) {
        const u64 key = a.bk[i];
        u64 where = a.cap_mask + 1;
        if (key != FJ_EMPTY_KEY && !gj_gt_find(a.tkeys, a.cap_mask, key, where)) continue;
        gj_combine<FJ_GJ_COUNT>(&acc[where], planes[i]);
        gj_combine<A::SUM>(&acc[plane + where], planes[a.nb + i]);
        gj_combine<A::MIN>(&acc[2 * plane + where], planes[2 * a.nb + i]);
        gj_combine<A::MAX>(&acc[3 * plane + where], planes[3 * a.nb + i]);
    }
}

}  // namespace

hipError_t fj_launch_group_by_merge(const FjGroupByArgs& a, const u64* planes, u64 nrows, int kind, hipStream_t s) {
    if (kind < KIND_UNSIGNED || kind > KIND_FLOAT || !a.cursor || !a.err || !a.nparts || !a.out_keys || !a.out_vals || !a.out_capacity || !planes)
        return hipErrorInvalidValue;
    if (!a.rel.list ? a.rel.n_flat > nrows : !a.rel.vals) return hipErrorInvalidValue;      // (a chunk pool without positions has nothing to gather by)
    void (*kern)(FjGroupByArgs, const u64*, u64) = fjh::for_kind(kind, [](auto K) { return fj_group_by_merge_kernel<FJ_V(K)>; });
    hipError_t e = fj_set_max_lds_once(reinterpret_cast<const void*>(kern), GM_LDS);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(a.nparts), dim3(GJ_NT), GM_LDS, s, a, planes, nrows);
    return hipGetLastError();
}

hipError_t fj_launch_gt_group_by_merge_combine(const FjGtArgs& a, int kind, const u64* planes, u64* acc, hipStream_t s) {
    if (kind < KIND_UNSIGNED || kind > KIND_FLOAT || !acc || !planes) return hipErrorInvalidValue;
    if (!a.nb) return hipSuccess;
    void (*kern)(FjGtArgs, const u64*, u64*) = fjh::for_kind(kind, [](auto K) { return fj_gt_group_by_merge_combine_kernel<FJ_V(K)>; });
    hipLaunchKernelGGL(kern, dim3(fjh::gt_grid(a.nb)), dim3(1024), 0, s, a, planes, acc);
    return hipGetLastError();
}

namespace fjh {

static int merge_outcap_error(u64 g, size_t cap_out) {
    return set_err("fj_join_device: FJ_ALGO_AGG_MERGE found g = %llu distinct keys, output capacity %zu rows (the outputs hold no complete result; call again with room for g)",
                   (unsigned long long)g, cap_out);
}

// the global-table form (fj_host.h): group_by_all's accumulator planes and sweep behind this file's combine kernel
static int group_by_merge_global(fj_ctx* c, const u64* bk, const u64* bv, size_t nb, hipStream_t s, fj_timings* t, u64* out_count,
                                 u64* d_ok, u64* d_ov, size_t cap_out, int kind) {
    const u64 plane = gt_capacity(nb) + 1;
    FjGtArgs a{};
    u64* acc = nullptr;
    if (gt_open(c, nb, 4 * plane, s, &a, &acc)) return 1;
    a.bk = bk;
    HIPCHK(fj_launch_gt_build_first(a, false, s));
    for (int j = PLANE_COUNT; j <= PLANE_MAX; ++j) HIPCHK(fj_launch_group_fill(acc + j * plane, plane, kind_agg(kind, j), s));
    HIPCHK(fj_launch_gt_group_by_merge_combine(a, kind, bv, acc, s));
    HIPCHK(hipEventRecord(c->ev[E_BUILD], s));
    HIPCHK(hipEventRecord(c->ev[E_PPART], s));
    HIPCHK(fj_launch_gt_group_by_all_sweep(a, acc, d_ok, d_ov, cap_out, &c->d_sc->total, &c->d_sc->err, s));
    if (gt_close(c, s, t)) return 1;
    *out_count = c->h_sc->total;
    if (c->h_sc->err & FJ_ERR_OUTCAP) return merge_outcap_error(c->h_sc->total, cap_out);      // (g goes back with the error)
    return 0;
}

// FJ_ALGO_GROUP_BY | FJ_ALGO_AGG_ALL | FJ_ALGO_AGG_MERGE (fj_join_device has checked the arguments): the g distinct keys of the nb
// partial rows bk in d_ok and, in the four planes of cap_out words of d_ov, the merged counts, sums, minima and maxima of the four
// planes of nb words of bv; kind 0 / 1 / 2: the words of the sum, min and max planes as uint64 / int64 / binary64.  cap_out >= 1 is all
// that is asked: g > cap_out fails here, after the device work.  use_radix: the partitioned plan, else the global table
int group_by_merge(fj_ctx* c, bool use_radix, const u64* bk, const u64* bv, size_t nb, int top_bits, hipStream_t s, fj_timings* t,
                   u64* out_count, u64* d_ok, u64* d_ov, size_t cap_out, int kind) {
    *out_count = 0;
    if (nb == 0) return 0;
    if (!use_radix) return group_by_merge_global(c, bk, bv, nb, s, t, out_count, d_ok, d_ov, cap_out, kind);

    RelAttempt r;      // aim at half of the table's 2048 slots per partition; the rows' positions travel, the kernel gathers the planes
    if (rel_open(c, bk, REL_POSITIONS, nullptr, nb, top_bits, GM_TS / 2, s, &r)) return 1;
    FjGroupByArgs ga{};
    ga.rel = r.rel; ga.nparts = r.nparts;
    ga.out_keys = d_ok; ga.out_vals = d_ov; ga.out_capacity = cap_out;
    ga.cursor = &c->d_sc->total; ga.err = &c->d_sc->err;
    HIPCHK(fj_launch_group_by_merge(ga, bv, nb, kind, s));
    if (rel_close(c, r.plan, r.nparts, s, t)) return 1;
    if (c->h_sc->err & FJ_ERR_LDS_FULL)                      // a partition beyond the LDS table: the whole call on the HBM table
        return gt_fallback(t, [&](fj_timings* g) { return group_by_merge_global(c, bk, bv, nb, s, g, out_count, d_ok, d_ov, cap_out, kind); });
    *out_count = c->h_sc->total;
    if (c->h_sc->err & FJ_ERR_OUTCAP) return merge_outcap_error(c->h_sc->total, cap_out);      // (g goes back with the error)
    return 0;
}

}  // namespace fjh
