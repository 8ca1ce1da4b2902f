// fj_groupby_multi.hip -- group-by on ONE relation with FOUR aggregates of its value column in one call (an EXTENSION: FJ_ALGO_GROUP_BY |
// FJ_ALGO_AGG_ALL, include/flashjoin.h): the distinct keys, densely packed, and beside each its row count, the sum, the minimum and the
// maximum of the values - SELECT k, COUNT(*), SUM(v), MIN(v), MAX(v) ... GROUP BY k.  The single forms (csrc/fj_groupby.hip) have one
// accumulator per slot and one d_out_vals: four calls, four trips through the partition passes (most of a group-by's time), and an
// alignment of the four results by key.  Here the relation goes through the passes ONCE, with its value column.
//
// The kernel is fj_group_by_kernel's with a narrower table and more planes behind it: one workgroup per final partition, every row
// inserts or finds its key in the LDS table of csrc/fj_lds_table_dev.h (home slot FJ_HW2(key) & (TS - 1), linear probing, one 64-bit
// CAS per claim, inserts bounded by TS steps, `full` behind LIMIT = TS - TS / 16, the marker key out of band in the header with four
// accumulators of its own) and then combines into the slot's four accumulators: one u32 atomic add for the count and three
// gj_combine (csrc/fj_group_dev.h) of the value's kind - unsigned, signed (FJ_ALGO_AGG_SIGNED) or float (FJ_ALGO_AGG_FLOAT).
//
// LDS budget, TS = 4096 slots (LIMIT 3840):  key 8 B + sum 8 B + min 8 B + max 8 B + count 4 B = 36 B per slot,
//   36 B * 4096 = 147 456 B, + the 64-byte header = 147 520 B of the 163 840 B one workgroup may take.
// An 8-byte count plane would come to 163 840 B before the header; 8192 slots to twice that.  So the count is a u32 in LDS, widened
// at the emit, and the plan aims at 2048 rows per partition (make_plan's target_override, as the many-to-many join does) - one radix
// bit more than the single forms take.
// The u32 cannot wrap: a partition is a chunk list of FJ_CHUNK = 256-row chunks, pass_prepare (csrc/fj_plan.hip) refuses a relation
// that would need 2^24 chunk ids, so a partition holds fewer than 2^24 * 256 = 2^32 rows; a flat (zero-pass) relation has at most
// 2048.  group_by_all below sends nb >= 2^32 to the HBM form, whose counts are u64, whatever the passes would say.
//
// The stream loop has no barrier and no global store, and requests the next round's loads before this round's inserts
// (gb_load_round, shared with fj_groupby.hip through fj_group_dev.h).  The emit is fj_group_by_kernel's: one global atomic reserves
// the partition's rows on the call's cursor, ballot + popcount ranks the occupied slots, and a slot writes its key and its four
// aggregates at stride out_capacity.  out_capacity may be smaller than nb here: a row at or past it is not written and raises
// FJ_ERR_OUTCAP, the cursor still counts it, and the host reports g against the capacity.
//
// Fallback: FJ_ERR_LDS_FULL, a partition of more than 3840 distinct keys; the HBM-table kernels end this file.
//
// Weak spot, as in fj_groupby.hip and four times over: a key that owns a large share of the rows is streamed by one workgroup and
// its four LDS atomics per row hit four addresses.  Correct at any distribution (DESIGN.md "Group-by with four aggregates").
#include "fj_host.h"
#include "fj_group_dev.h"

namespace {

constexpr u32 GA_TS = 4096, GA_LIMIT = GA_TS - GA_TS / 16;
using fjh::KIND_UNSIGNED; using fjh::KIND_SIGNED; using fjh::KIND_FLOAT;        // the `kind` of the value column (fj_host.h)

// 64 B: the key slots behind it stay 16-byte aligned.  empty_*: the marker key's accumulators
struct GaHdr { u32 full, has_empty, nkeys, cursor; u32 empty_cnt, pad; u64 empty_sum, empty_min, empty_max, base, pad2; };
static_assert(sizeof(GaHdr) == 64, "GaHdr");
constexpr u32 GA_LDS = (u32)sizeof(GaHdr) + GA_TS * 36u;
static_assert(GA_LDS <= 163840u, "the table must fit one workgroup's LDS");
static_assert(GA_TS % GJ_NT == 0, "the emit sweeps whole waves");

template <int KIND> struct GaAgg {
    static constexpr int SUM = KIND == KIND_FLOAT ? FJ_GJ_SUM_F : FJ_GJ_SUM;
    static constexpr int MIN = KIND == KIND_FLOAT ? FJ_GJ_MIN_F : KIND == KIND_SIGNED ? FJ_GJ_MIN_S : FJ_GJ_MIN_U;
    static constexpr int MAX = KIND == KIND_FLOAT ? FJ_GJ_MAX_F : KIND == KIND_SIGNED ? FJ_GJ_MAX_S : FJ_GJ_MAX_U;
};

// a.out_vals: four planes of a.out_capacity words - count, sum, min, max
template <int KIND>
__global__ __launch_bounds__(GJ_NT, 1) void fj_group_by_all_kernel(FjGroupByArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    GaHdr* hdr = reinterpret_cast<GaHdr*>(smem);
    u64* tkeys = reinterpret_cast<u64*>(smem + sizeof(GaHdr));
    u64* asum = tkeys + GA_TS;
    u64* amin = asum + GA_TS;
    u64* amax = amin + GA_TS;
    u32* acnt = reinterpret_cast<u32*>(amax + GA_TS);
    using A = GaAgg<KIND>;
    constexpr u64 ID_SUM = gj_identity<A::SUM>(), ID_MIN = gj_identity<A::MIN>(), ID_MAX = gj_identity<A::MAX>();
    const u32 tid = threadIdx.x, lane = tid & 63;
    const u32 p = blockIdx.x;
    u32 b0, nbc;
    fj_part_chunks(a.rel, p, b0, nbc);
    if (nbc == 0) return;

    for (u32 i = tid; i < GA_TS; i += GJ_NT) { tkeys[i] = FJ_EMPTY_KEY; asum[i] = ID_SUM; amin[i] = ID_MIN; amax[i] = ID_MAX; acnt[i] = 0; }
    if (tid == 0) {
        hdr->full = 0; hdr->has_empty = 0; hdr->nkeys = 0; hdr->cursor = 0; hdr->empty_cnt = 0;
        hdr->empty_sum = ID_SUM; hdr->empty_min = ID_MIN; hdr->empty_max = ID_MAX; hdr->base = 0;
    }
    __syncthreads();

    // ---- stream: rounds of GJ_NT * GJ_KPT rows; the next round's loads are requested before this round's inserts.  No global
    // store, no barrier inside the loop ----
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
            const u64 key = a.rel.list ? k[u] : fj_key_mix(k[u]);                 // chunk pools hold mixed keys, flat arrays raw ones
            const u64 v = pv[u];
            if (key == FJ_EMPTY_KEY) {                       // the empty marker is never stored in the table
                hdr->has_empty = 1;
                atomicAdd(&hdr->empty_cnt, 1u);
                gj_combine<A::SUM>(&hdr->empty_sum, v); gj_combine<A::MIN>(&hdr->empty_min, v); gj_combine<A::MAX>(&hdr->empty_max, v);
                continue;
            }
            if (*(volatile u32*)&hdr->full) continue;        // the item is lost already: the rest of its rows do no table work
            u32 pos = FJ_HW2(key) & (GA_TS - 1);
            bool placed = false;
            for (u32 step = 0; step < GA_TS; ++step) {
                u64 t = tkeys[pos];                          // (a slot never changes once it holds a key: a stale read costs a CAS at most)
                if (t == FJ_EMPTY_KEY) {
                    t = atomicCAS((unsigned long long*)&tkeys[pos], (unsigned long long)FJ_EMPTY_KEY, (unsigned long long)key);
                    if (t == FJ_EMPTY_KEY) {
                        if (atomicAdd(&hdr->nkeys, 1u) >= GA_LIMIT) hdr->full = 1;
                        t = key;
                    }
                }
                if (t == key) { placed = true; break; }
                pos = (pos + 1) & (GA_TS - 1);
            }
            if (!placed) { hdr->full = 1; continue; }
            atomicAdd(&acnt[pos], 1u);                       // (a partition holds fewer than 2^32 rows: the header comment)
            gj_combine<A::SUM>(&asum[pos], v); gj_combine<A::MIN>(&amin[pos], v); gj_combine<A::MAX>(&amax[pos], v);
        }
#pragma unroll
        for (u32 u = 0; u < GJ_KPT; ++u) { k[u] = kn[u]; pv[u] = pvn[u]; }
        okm = okn;
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
    for (u32 i = tid; i < GA_TS; i += GJ_NT) {               // (GA_TS is a multiple of GJ_NT: whole waves every round)
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
            ov[row] = (u64)acnt[i]; ov[cap + row] = asum[i]; ov[2 * cap + row] = amin[i]; ov[3 * cap + row] = amax[i];
        } else atomicOr(a.err, FJ_ERR_OUTCAP);
    }
    if (tid == 0 && has_empty) {
        const u64 row = o + nk;
        if (row < cap) {
            a.out_keys[row] = fj_key_unmix(FJ_EMPTY_KEY);
            ov[row] = (u64)hdr->empty_cnt; ov[cap + row] = hdr->empty_sum; ov[2 * cap + row] = hdr->empty_min; ov[3 * cap + row] = hdr->empty_max;
        } else atomicOr(a.err, FJ_ERR_OUTCAP);
    }
}

// ---- the global-table form.  The table is fj_gt_build_first_kernel's, keys only (csrc/fj_join.hip: raw keys, the raw empty key out
// of band); acc: four planes of capacity + 1 words - count, sum, min, max - each holding its identity, the last word the empty key's ----
// thread per row of the relation: four typed global atomics on the slot of the row's key (the build placed every key); u64 counts
template <int KIND>
__global__ __launch_bounds__(1024) void fj_gt_group_by_all_combine_kernel(FjGtArgs a, const u64* __restrict__ vals, u64* acc) {
    using A = GaAgg<KIND>;
    const u64 plane = a.cap_mask + 2;
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < a.nb; i += stride) {
        const u64 key = a.bk[i];
        u64 where = a.cap_mask + 1;
        if (key != FJ_EMPTY_KEY && !gj_gt_find(a.tkeys, a.cap_mask, key, where)) continue;
        const u64 v = vals[i];
        gj_combine<FJ_GJ_COUNT>(&acc[where], 1ull);
        gj_combine<A::SUM>(&acc[plane + where], v); gj_combine<A::MIN>(&acc[2 * plane + where], v); gj_combine<A::MAX>(&acc[3 * plane + where], v);
    }
}

// the capacity + 1 slots, compacted: an occupied slot's key and four accumulators go to the row a wave-aggregated cursor hands out
// (one global atomic per wave that holds a key), the planes at stride out_capacity.  The cursor counts past out_capacity
__global__ __launch_bounds__(1024) void fj_gt_group_by_all_sweep_kernel(FjGtArgs a, const u64* __restrict__ acc, u64* __restrict__ out_keys,
                                                                        u64* __restrict__ out_vals, u64 out_capacity, unsigned long long* cursor, u32* err) {
    const u64 cap = a.cap_mask + 1, plane = cap + 1;
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
        if (!occ) continue;
        const u64 row = wbase + (u32)__popcll(m & ((1ull << lane) - 1ull));
        if (row < out_capacity) {
            out_keys[row] = key;
#pragma unroll
            for (u32 j = 0; j < 4; ++j) out_vals[j * out_capacity + row] = acc[j * plane + i];
        } else atomicOr(err, FJ_ERR_OUTCAP);
    }
}

}  // namespace

hipError_t fj_launch_group_by_all(const FjGroupByArgs& a, int kind, hipStream_t s) {
    if (kind < KIND_UNSIGNED || kind > KIND_FLOAT || !a.cursor || !a.err || !a.nparts || !a.out_keys || !a.out_vals || !a.out_capacity)
        return hipErrorInvalidValue;
    if (!a.rel.list && (!a.rel.vals || a.rel.n_flat > 0xFFFFFFFFull)) return hipErrorInvalidValue;      // (the value column; the u32 counts)
    void (*kern)(FjGroupByArgs) = fjh::for_kind(kind, [](auto K) { return fj_group_by_all_kernel<FJ_V(K)>; });
    hipError_t e = fj_set_max_lds_once(reinterpret_cast<const void*>(kern), GA_LDS);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(a.nparts), dim3(GJ_NT), GA_LDS, s, a);
    return hipGetLastError();
}

hipError_t fj_launch_gt_group_by_all_combine(const FjGtArgs& a, int kind, const u64* vals, u64* acc, hipStream_t s) {
    if (kind < KIND_UNSIGNED || kind > KIND_FLOAT || !acc || !vals) return hipErrorInvalidValue;
    if (!a.nb) return hipSuccess;
    void (*kern)(FjGtArgs, const u64*, u64*) = fjh::for_kind(kind, [](auto K) { return fj_gt_group_by_all_combine_kernel<FJ_V(K)>; });
    hipLaunchKernelGGL(kern, dim3(fjh::gt_grid(a.nb)), dim3(1024), 0, s, a, vals, acc);
    return hipGetLastError();
}

hipError_t fj_launch_gt_group_by_all_sweep(const FjGtArgs& a, const u64* acc, u64* out_keys, u64* out_vals, u64 out_capacity,
                                           unsigned long long* cursor, u32* err, hipStream_t s) {
    if (!cursor || !err || !acc || !out_keys || !out_vals || !out_capacity) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fj_gt_group_by_all_sweep_kernel, dim3(fjh::gt_grid(a.cap_mask + 2)), dim3(1024), 0, s, a, acc, out_keys, out_vals,
                       out_capacity, cursor, err);
    return hipGetLastError();
}

namespace fjh {

static int outcap_error(u64 g, size_t cap_out) {
    return set_err("fj_join_device: FJ_ALGO_AGG_ALL found g = %llu distinct keys, output capacity %zu rows (the outputs hold no complete result; call again with room for g)",
                   (unsigned long long)g, cap_out);
}

// the global-table form (fj_host.h); also what a relation of 2^32 rows or more takes.  Four accumulator planes of capacity + 1 words
static int group_by_all_global(fj_ctx* c, const u64* bk, const u64* bv, size_t nb, hipStream_t s, fj_timings* t, u64* out_count,
                               u64* d_ok, u64* d_ov, size_t cap_out, int kind) {
    const u64 plane = gt_capacity(nb) + 1;
    FjGtArgs a{};
    u64* acc = nullptr;
    if (gt_open(c, nb, 4 * plane, s, &a, &acc)) return 1;
    a.bk = bk;
    HIPCHK(fj_launch_gt_build_first(a, false, s));
    for (int j = PLANE_COUNT; j <= PLANE_MAX; ++j) HIPCHK(fj_launch_group_fill(acc + j * plane, plane, kind_agg(kind, j), s));
    HIPCHK(fj_launch_gt_group_by_all_combine(a, kind, bv, acc, s));
    HIPCHK(hipEventRecord(c->ev[E_BUILD], s));
    HIPCHK(hipEventRecord(c->ev[E_PPART], s));
    HIPCHK(fj_launch_gt_group_by_all_sweep(a, acc, d_ok, d_ov, cap_out, &c->d_sc->total, &c->d_sc->err, s));
    if (gt_close(c, s, t)) return 1;
    *out_count = c->h_sc->total;
    if (c->h_sc->err & FJ_ERR_OUTCAP) return outcap_error(c->h_sc->total, cap_out);      // (g goes back with the error)
    return 0;
}

// FJ_ALGO_GROUP_BY | FJ_ALGO_AGG_ALL (fj_join_device has checked the arguments): the g distinct keys of bk[0 .. nb) in d_ok and, in the
// four planes of cap_out words of d_ov, their row counts and the sums, minima and maxima of bv; kind 0 / 1 / 2: the words of bv as
// uint64 / int64 / binary64.  cap_out >= 1 is all that is asked: g > cap_out fails here, after the device work.
// use_radix: the partitioned plan, else the global table
int group_by_all(fj_ctx* c, bool use_radix, const u64* bk, const u64* bv, size_t nb, int top_bits, hipStream_t s, fj_timings* t,
                 u64* out_count, u64* d_ok, u64* d_ov, size_t cap_out, int kind) {
    *out_count = 0;
    if (nb == 0) return 0;
    if ((u64)nb >> 32) use_radix = false;                    // (the LDS table counts in u32)
    if (!use_radix) return group_by_all_global(c, bk, bv, nb, s, t, out_count, d_ok, d_ov, cap_out, kind);

    RelAttempt r;
    if (rel_open(c, bk, REL_VALUES, bv, nb, top_bits, GA_TS / 2, s, &r)) return 1;      // aim at half of the table's 4096 slots per partition
    FjGroupByArgs ga{};
    ga.rel = r.rel; ga.nparts = r.nparts;
    ga.out_keys = d_ok; ga.out_vals = d_ov; ga.out_capacity = cap_out;
    ga.cursor = &c->d_sc->total; ga.err = &c->d_sc->err;
    HIPCHK(fj_launch_group_by_all(ga, kind, s));
    if (rel_close(c, r.plan, r.nparts, s, t)) return 1;
    if (c->h_sc->err & FJ_ERR_LDS_FULL)                      // a partition beyond the LDS table: the whole call on the HBM table
        return gt_fallback(t, [&](fj_timings* g) { return group_by_all_global(c, bk, bv, nb, s, g, out_count, d_ok, d_ov, cap_out, kind); });
    *out_count = c->h_sc->total;
    if (c->h_sc->err & FJ_ERR_OUTCAP) return outcap_error(c->h_sc->total, cap_out);      // (g goes back with the error)
    return 0;
}

}  // namespace fjh
