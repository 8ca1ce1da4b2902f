// fj_groupby_pair_agg.hip -- group-by under a TWO-COLUMN key with FOUR aggregates of a value column in one call (an EXTENSION:
// FJ_ALGO_GROUP_BY | FJ_ALGO_KEY_PAIR | FJ_ALGO_AGG_ALL, include/flashjoin.h): the distinct pairs (A, B), densely packed, and beside
// each its row count, the sum, the minimum and the maximum of V - SELECT a, b, COUNT(*), SUM(v), MIN(v), MAX(v) ... GROUP BY a, b.
// Composed it is FJ_ALGO_KEY_PAIR's group ids (csrc/fj_groupby_pair.hip: two trips of every partition, a gather of every row's own
// pair, nb ids written), FJ_ALGO_AGG_ALL over the ids (the relation through the passes a second time) and two gathers through the
// first rows.  Here the relation goes through the passes ONCE and every partition is streamed ONCE.
//
// A pair becomes one word, w = fj_key_pair(a, b) = a ^ fj_key_mix(b ^ C) (csrc/fj_common.h); fj_pair_combine_kernel writes the nb
// words and the passes run over them, carrying the rows' positions (PassIter::vals_pos).  w and b together determine a, so a table slot
// that knows its word and its group's b knows the whole pair: nothing looks up a representative row, and the slot emits both key
// columns itself.
//
// fj_group_by_pair_agg_kernel is fj_group_by_merge_kernel's shape (csrc/fj_groupby_merge.hip): one workgroup of 1024 threads per WHOLE
// final partition, the LDS table that csrc/fj_lds_table_dev.h STATES over the mixed words (the insert loop is written out in the kernel,
// as that header says every kernel's is), the marker word out of band in the header.  Per row:
// gather B[position] and V[position], find or insert the word, and six LDS atomics behind the slot - a 64-bit minimum of b into bmin
// (all ones at rest), a 64-bit maximum of b into bmax (0 at rest), a u32 add for the count and three gj_combine of V's kind.
//
// THE bmin / bmax ARGUMENT.  For a fixed b the word is a bijection of a, so two DISTINCT pairs on one word differ in b.  After the
// barrier behind the stream, bmin and bmax of a slot are the exact minimum and maximum of b over the rows that met that slot (the
// atomics are unconditional and the identities, all ones and 0, are the extremes of u64: no value of b is special, b == 0 and
// b == 2^64 - 1 included).  So the slot holds ONE pair iff bmin == bmax, and then that value is the group's b.  A slot - or the marker -
// with bmin != bmax raises FJ_ERR_PAIR_COLLISION, its partition writes nothing, and the host re-runs the whole call on the HBM form,
// which compares pairs.  Exact at any input; no lane waits on another lane's store, there is no spin loop.
//
// LDS budget, TS = 2048 slots (LIMIT 1920):  word 8 B + bmin 8 B + bmax 8 B + sum 8 B + min 8 B + max 8 B + count 4 B = 52 B per slot,
//   52 B * 2048 = 106 496 B, + the 128-byte header = 106 624 B of the 163 840 B one workgroup may take; 4096 slots would be 213 120 B.
// So the plan aims at 1024 rows per partition, as the merge does.  The count is a u32 in LDS as in fj_group_by_all_kernel (a partition
// holds fewer than 2^32 rows: that file's header); nb >= 2^32 goes to the HBM form, whose counts are u64.
//
// ONE stream, rounds of FOUR rows per thread: the next round's words and positions are requested before this round's inserts, its
// gathers of B and V behind them.  No global store and no barrier inside the loop.  The emit is fj_group_by_all_kernel's: one global
// atomic per workgroup reserves the rows, ballot + popcount ranks the occupied slots, the marker's group is last; a slot writes
// a = fj_key_unmix(slot) ^ fj_key_mix(b ^ C), plane 0 = b and the four aggregates in planes 1..4 at stride out_capacity.
//
// Fallback: FJ_ERR_LDS_FULL (a partition of more than 1920 distinct words) or FJ_ERR_PAIR_COLLISION.  The HBM
// form keeps fj_gt_pair_build_kernel's table of ROW INDICES (csrc/fj_groupby_pair.hip): pairs are compared, words are only a hash.
//
// Weak spot: a hot pair is one workgroup's, and its six LDS atomics per row land on the six words behind ONE slot - two of them,
// bmin and bmax, for a b that never changes.  Correct at any distribution (DESIGN.md "Two-column keys with aggregates").
#include "fj_host.h"
#include "fj_group_dev.h"

namespace {

constexpr u32 GQ_TS = 2048, GQ_LIMIT = GQ_TS - GQ_TS / 16;
using fjh::KIND_UNSIGNED; using fjh::KIND_SIGNED; using fjh::KIND_FLOAT;        // the `kind` of the value column (fj_host.h)

// 128 B: the key slots behind it stay 16-byte aligned.  empty_*: the marker word's b evidence and accumulators
struct GqHdr { u32 full, has_empty, nkeys, cursor; u32 empty_cnt, collided; u64 empty_bmin, empty_bmax, empty_sum, empty_min, empty_max, base; u64 pad[7]; };
static_assert(sizeof(GqHdr) == 128, "GqHdr");
constexpr u32 GQ_LDS = (u32)sizeof(GqHdr) + GQ_TS * 52u;
static_assert(GQ_LDS == 106624u && GQ_LDS <= 163840u, "the table must fit one workgroup's LDS");
static_assert(GQ_TS % GJ_NT == 0, "the verification and the emit sweep whole waves");

template <int KIND> struct GqAgg {
    static constexpr int SUM = KIND == KIND_FLOAT ? FJ_GJ_SUM_F : FJ_GJ_SUM;
    static constexpr int MIN = KIND == KIND_FLOAT ? FJ_GJ_MIN_F : KIND == KIND_SIGNED ? FJ_GJ_MIN_S : FJ_GJ_MIN_U;
    static constexpr int MAX = KIND == KIND_FLOAT ? FJ_GJ_MAX_F : KIND == KIND_SIGNED ? FJ_GJ_MAX_S : FJ_GJ_MAX_U;
};

// Rounds of FOUR rows per thread, as in fj_group_by_merge_kernel: a row in flight is its word, its position and the two gathered
// words (profiles/group_by_pair_agg_kernel_resources.txt).  A round covers 16 chunks: the plan's 1024-row partition is one round also
// where the passes left it in partial chunks
constexpr u32 GQ_KPT = 4, GQ_ROUND_CHUNKS = GJ_NT * GQ_KPT / FJ_CHUNK;
__device__ __forceinline__ void gq_load_round(const FjChunkSet& rel, u32 b0, u32 nbc, u32 c0, u32 tid, u64 (&kk)[GQ_KPT], u64 (&pp)[GQ_KPT], u32& ok) {
    ok = 0;
#pragma unroll
    for (u32 u = 0; u < GQ_KPT; ++u) {
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

// B[position] and V[position] of one round's rows.  A position at or beyond nrows (the passes make none) is not read
__device__ __forceinline__ void gq_gather(const u64* __restrict__ B, const u64* __restrict__ V, u64 nrows, const u64 (&ps)[GQ_KPT], u32& ok,
                                          u64 (&b)[GQ_KPT], u64 (&v)[GQ_KPT], u32* err) {
#pragma unroll
    for (u32 u = 0; u < GQ_KPT; ++u) {
        b[u] = 0; v[u] = 0;
        if (!((ok >> u) & 1u)) continue;
        if (ps[u] < nrows) { b[u] = B[ps[u]]; v[u] = V[ps[u]]; }
        else { ok &= ~(1u << u); atomicOr(err, FJ_ERR_OUTCAP); }
    }
}

// a.rel: the combined words (chunk pools: mixed, with the positions in the vals plane; a flat array: raw, the index is the position).
// B, V: the second key column and the value column, nrows words each.  a.out_keys: column A of every group; a.out_vals: FIVE planes of
// a.out_capacity words - column B, count, sum, min, max
template <int KIND>
__global__ __launch_bounds__(GJ_NT, 1) void fj_group_by_pair_agg_kernel(FjGroupByArgs a, const u64* __restrict__ B, const u64* __restrict__ V, u64 nrows) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    GqHdr* hdr = reinterpret_cast<GqHdr*>(smem);
    u64* tkeys = reinterpret_cast<u64*>(smem + sizeof(GqHdr));
    u64* bmin = tkeys + GQ_TS;
    u64* bmax = bmin + GQ_TS;
    u64* asum = bmax + GQ_TS;
    u64* amin = asum + GQ_TS;
    u64* amax = amin + GQ_TS;
    u32* acnt = reinterpret_cast<u32*>(amax + GQ_TS);
    using A = GqAgg<KIND>;
    constexpr u64 ID_SUM = gj_identity<A::SUM>(), ID_MIN = gj_identity<A::MIN>(), ID_MAX = gj_identity<A::MAX>();
    const u32 tid = threadIdx.x, lane = tid & 63;
    const u32 p = blockIdx.x;
    u32 b0, nbc;
    fj_part_chunks(a.rel, p, b0, nbc);
    if (nbc == 0) return;

    for (u32 i = tid; i < GQ_TS; i += GJ_NT) {
        tkeys[i] = FJ_EMPTY_KEY; bmin[i] = ~0ull; bmax[i] = 0; asum[i] = ID_SUM; amin[i] = ID_MIN; amax[i] = ID_MAX; acnt[i] = 0;
    }
    if (tid == 0) {
        hdr->full = 0; hdr->has_empty = 0; hdr->nkeys = 0; hdr->cursor = 0; hdr->empty_cnt = 0; hdr->collided = 0;
        hdr->empty_bmin = ~0ull; hdr->empty_bmax = 0; hdr->empty_sum = ID_SUM; hdr->empty_min = ID_MIN; hdr->empty_max = ID_MAX; hdr->base = 0;
    }
    __syncthreads();

    // ---- the ONE stream: rounds of GJ_NT * GQ_KPT rows; the next round's words and positions are requested before this round's
    // inserts, its two gathered words behind them.  No global store, no barrier inside the loop ----
    u64 k[GQ_KPT], ps[GQ_KPT], kb[GQ_KPT], v[GQ_KPT];
    u32 okm = 0;
    gq_load_round(a.rel, b0, nbc, 0, tid, k, ps, okm);
    gq_gather(B, V, nrows, ps, okm, kb, v, a.err);
    for (u32 c0 = 0; c0 < nbc; c0 += GQ_ROUND_CHUNKS) {
        const bool more = c0 + GQ_ROUND_CHUNKS < nbc;
        u64 kn[GQ_KPT], pn[GQ_KPT];
        u32 okn = 0;
        if (more) gq_load_round(a.rel, b0, nbc, c0 + GQ_ROUND_CHUNKS, tid, kn, pn, okn);
#pragma unroll
        for (u32 u = 0; u < GQ_KPT; ++u) {
            if (!((okm >> u) & 1u)) continue;
            const u64 key = a.rel.list ? k[u] : fj_key_mix(k[u]);                 // chunk pools hold mixed words, the flat buffer raw ones
            if (key == FJ_EMPTY_KEY) {                       // the empty marker is never stored in the table
                hdr->has_empty = 1;
                atomicMin((unsigned long long*)&hdr->empty_bmin, (unsigned long long)kb[u]);
                atomicMax((unsigned long long*)&hdr->empty_bmax, (unsigned long long)kb[u]);
                atomicAdd(&hdr->empty_cnt, 1u);
                gj_combine<A::SUM>(&hdr->empty_sum, v[u]); gj_combine<A::MIN>(&hdr->empty_min, v[u]); gj_combine<A::MAX>(&hdr->empty_max, v[u]);
                continue;
            }
            if (*(volatile u32*)&hdr->full) continue;        // the item is lost already: the rest of its rows do no table work
            u32 pos = FJ_HW2(key) & (GQ_TS - 1);
            bool placed = false;
            for (u32 step = 0; step < GQ_TS; ++step) {
                u64 t = tkeys[pos];                          // (a slot never changes once it holds a key: a stale read costs a CAS at most)
                if (t == FJ_EMPTY_KEY) {
                    t = atomicCAS((unsigned long long*)&tkeys[pos], (unsigned long long)FJ_EMPTY_KEY, (unsigned long long)key);
                    if (t == FJ_EMPTY_KEY) {
                        if (atomicAdd(&hdr->nkeys, 1u) >= GQ_LIMIT) hdr->full = 1;
                        t = key;
                    }
                }
                if (t == key) { placed = true; break; }
                pos = (pos + 1) & (GQ_TS - 1);
            }
            if (!placed) { hdr->full = 1; continue; }
            atomicMin((unsigned long long*)&bmin[pos], (unsigned long long)kb[u]);        // the slot's b evidence: one pair iff the two agree
            atomicMax((unsigned long long*)&bmax[pos], (unsigned long long)kb[u]);
            atomicAdd(&acnt[pos], 1u);                       // (a partition holds fewer than 2^32 rows: the header comment)
            gj_combine<A::SUM>(&asum[pos], v[u]); gj_combine<A::MIN>(&amin[pos], v[u]); gj_combine<A::MAX>(&amax[pos], v[u]);
        }
        if (more) {
#pragma unroll
            for (u32 u = 0; u < GQ_KPT; ++u) { k[u] = kn[u]; ps[u] = pn[u]; }
            okm = okn;
            gq_gather(B, V, nrows, ps, okm, kb, v, a.err);
        }
    }
    __syncthreads();
    if (hdr->full) { if (tid == 0) atomicOr(a.err, FJ_ERR_LDS_FULL); return; }     // nothing written: the host re-runs the call on the HBM table

    // ---- verification: every occupied slot, and the marker, holds ONE pair iff its bmin == bmax (the header comment) ----
    {
        bool differs = false;
        for (u32 i = tid; i < GQ_TS; i += GJ_NT) differs |= tkeys[i] != FJ_EMPTY_KEY && bmin[i] != bmax[i];
        if (tid == 0 && hdr->has_empty && hdr->empty_bmin != hdr->empty_bmax) differs = true;
        if (differs) hdr->collided = 1;
    }
    __syncthreads();
    if (hdr->collided) { if (tid == 0) atomicOr(a.err, FJ_ERR_PAIR_COLLISION); return; }      // (uniform) nothing written either

    // ---- emit: one global atomic reserves [o, o + g_p); the table's occupied slots take ranks inside it, the marker word the last ----
    const u32 nk = hdr->nkeys;
    const bool has_empty = hdr->has_empty != 0;
    if (tid == 0) hdr->base = (u64)atomicAdd(a.cursor, (unsigned long long)(nk + (has_empty ? 1u : 0u)));
    __syncthreads();
    const u64 o = hdr->base, cap = a.out_capacity;
    u64* const ov = a.out_vals;
    for (u32 i = tid; i < GQ_TS; i += GJ_NT) {               // (GQ_TS is a multiple of GJ_NT: whole waves every round)
        const u64 key = tkeys[i];
        const bool occ = key != FJ_EMPTY_KEY;
        const unsigned long long m = __ballot(occ);
        u32 wbase = 0;
        if (lane == 0 && m) wbase = atomicAdd(&hdr->cursor, (u32)__popcll(m));
        wbase = __shfl(wbase, 0, 64);
        if (!occ) continue;
        const u64 row = o + wbase + (u32)__popcll(m & ((1ull << lane) - 1ull));
        if (row < cap) {
            const u64 b = bmin[i];
            a.out_keys[row] = fj_key_unmix(key) ^ fj_key_mix(b ^ FJ_PAIR_SALT);
            ov[row] = b;
            ov[cap + row] = (u64)acnt[i]; ov[2 * cap + row] = asum[i]; ov[3 * cap + row] = amin[i]; ov[4 * cap + row] = amax[i];
        } else atomicOr(a.err, FJ_ERR_OUTCAP);
    }
    if (tid == 0 && has_empty) {
        const u64 row = o + nk;
        if (row < cap) {
            const u64 b = hdr->empty_bmin;
            a.out_keys[row] = fj_key_unmix(FJ_EMPTY_KEY) ^ fj_key_mix(b ^ FJ_PAIR_SALT);
            ov[row] = b;
            ov[cap + row] = (u64)hdr->empty_cnt; ov[2 * cap + row] = hdr->empty_sum; ov[3 * cap + row] = hdr->empty_min; ov[4 * cap + row] = hdr->empty_max;
        } else atomicOr(a.err, FJ_ERR_OUTCAP);
    }
}

// ---- the global-table form.  The table is fj_gt_pair_build_kernel's (csrc/fj_groupby_pair.hip): capacity ROW INDICES, all ones at
// rest, a slot names a pair by its smallest row; acc: four planes of capacity + 1 words - count, sum, min, max - each holding its
// identity (the siblings' plane size: nothing is out of band here, the last word of each plane stays at rest) ----
// thread per row: the slot whose row holds the row's pair (the build placed every pair), then four typed global atomics; u64 counts
template <int KIND>
__global__ __launch_bounds__(1024) void fj_gt_pair_agg_combine_kernel(const u64* __restrict__ A, const u64* __restrict__ B, const u64* __restrict__ V, u64 nb,
                                                                      const u64* __restrict__ tab, u64 cap_mask, u64* acc) {
    using G = GqAgg<KIND>;
    const u64 plane = cap_mask + 2;
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < nb; i += stride) {
        const u64 ka = A[i], kb = B[i];
        u64 pos = fj_hash64(fj_key_pair(ka, kb)) & cap_mask;
        for (u64 step = 0; step <= cap_mask; ++step) {
            const u64 t = tab[pos];
            if (t >= nb) break;                              // (an empty slot: the build placed every pair, so this is not met)
            if (A[t] == ka && B[t] == kb) {
                const u64 v = V[i];
                gj_combine<FJ_GJ_COUNT>(&acc[pos], 1ull);
                gj_combine<G::SUM>(&acc[plane + pos], v); gj_combine<G::MIN>(&acc[2 * plane + pos], v); gj_combine<G::MAX>(&acc[3 * plane + pos], v);
                break;
            }
            pos = (pos + 1) & cap_mask;
        }
    }
}

// the capacity slots, compacted: an occupied slot's pair A[t], B[t] - t the slot's row - and its four accumulators go to the row a
// wave-aggregated cursor hands out (one global atomic per wave that holds a row), the five planes at stride out_capacity.  The cursor
// counts past out_capacity
__global__ __launch_bounds__(1024) void fj_gt_pair_agg_sweep_kernel(const u64* __restrict__ A, const u64* __restrict__ B, u64 nb, const u64* __restrict__ tab,
                                                                    u64 cap_mask, const u64* __restrict__ acc, u64* __restrict__ out_keys,
                                                                    u64* __restrict__ out_vals, u64 out_capacity, unsigned long long* cursor, u32* err) {
    const u64 cap = cap_mask + 1, plane = cap + 1;
    const u32 lane = threadIdx.x & 63;
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 w0 = (u64)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); w0 < cap; w0 += stride) {      // (uniform per wave; capacity is a multiple of 64)
        const u64 i = w0 + lane;
        const u64 t = tab[i];
        const bool occ = t < nb;                             // (the build stores row indices below nb and nothing else)
        const unsigned long long m = __ballot(occ);
        if (!m) continue;
        unsigned long long wbase = 0;
        if (lane == 0) wbase = atomicAdd(cursor, (unsigned long long)__popcll(m));
        wbase = __shfl(wbase, 0, 64);
        if (!occ) continue;
        const u64 row = wbase + (u32)__popcll(m & ((1ull << lane) - 1ull));
        if (row < out_capacity) {
            out_keys[row] = A[t];
            out_vals[row] = B[t];
#pragma unroll
            for (u32 j = 0; j < 4; ++j) out_vals[(j + 1) * out_capacity + row] = acc[j * plane + i];
        } else atomicOr(err, FJ_ERR_OUTCAP);
    }
}

hipError_t launch_pair_agg_lds(const FjGroupByArgs& a, const u64* B, const u64* V, u64 nrows, int kind, hipStream_t s) {
    if (kind < KIND_UNSIGNED || kind > KIND_FLOAT || !a.cursor || !a.err || !a.nparts || !a.out_keys || !a.out_vals || !a.out_capacity || !B || !V)
        return hipErrorInvalidValue;
    if (!a.rel.list ? a.rel.n_flat > nrows : !a.rel.vals) return hipErrorInvalidValue;      // (a chunk pool without positions has nothing to gather by)
    if (nrows > 0xFFFFFFFFull) return hipErrorInvalidValue;                                 // (the u32 counts)
    void (*kern)(FjGroupByArgs, const u64*, const u64*, u64) = fjh::for_kind(kind, [](auto K) { return fj_group_by_pair_agg_kernel<FJ_V(K)>; });
    hipError_t e = fj_set_max_lds_once(reinterpret_cast<const void*>(kern), GQ_LDS);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(a.nparts), dim3(GJ_NT), GQ_LDS, s, a, B, V, nrows);
    return hipGetLastError();
}

hipError_t launch_gt_pair_agg_combine(const u64* A, const u64* B, const u64* V, u64 nb, const u64* tab, u64 cap_mask, u64* acc, int kind, hipStream_t s) {
    if (kind < KIND_UNSIGNED || kind > KIND_FLOAT || !A || !B || !V || !tab || !acc) return hipErrorInvalidValue;
    if (!nb) return hipSuccess;
    void (*kern)(const u64*, const u64*, const u64*, u64, const u64*, u64, u64*) =
        fjh::for_kind(kind, [](auto K) { return fj_gt_pair_agg_combine_kernel<FJ_V(K)>; });
    hipLaunchKernelGGL(kern, dim3(fjh::gt_grid(nb)), dim3(1024), 0, s, A, B, V, nb, tab, cap_mask, acc);
    return hipGetLastError();
}

}  // namespace

namespace fjh {

static int pair_outcap_error(u64 g, size_t cap_out) {
    return set_err("fj_join_device: FJ_ALGO_KEY_PAIR | FJ_ALGO_AGG_ALL found g = %llu distinct pairs, output capacity %zu rows (the outputs hold no complete result; call again with room for g)",
                   (unsigned long long)g, cap_out);
}

// the global-table form (fj_host.h); also what a relation of 2^32 rows or more takes, and the fallback of two pairs on one word
static int group_by_pair_agg_global(fj_ctx* c, const u64* ka, const u64* kb, const u64* kv, size_t nb, hipStream_t s, fj_timings* t,
                                    u64* out_count, u64* d_ok, u64* d_ov, size_t cap_out, int kind) {
    const u64 cap = gt_capacity(nb), plane = cap + 1;
    FjGtArgs a{};
    u64* acc = nullptr;
    if (gt_open(c, nb, 4 * plane, s, &a, &acc)) return 1;
    u64* tab = a.tkeys;
    HIPCHK(fj_launch_gt_pair_build(ka, kb, (u64)nb, tab, cap - 1, s));
    for (int j = PLANE_COUNT; j <= PLANE_MAX; ++j) HIPCHK(fj_launch_group_fill(acc + j * plane, plane, kind_agg(kind, j), s));
    HIPCHK(launch_gt_pair_agg_combine(ka, kb, kv, (u64)nb, tab, cap - 1, acc, kind, s));
    HIPCHK(hipEventRecord(c->ev[E_BUILD], s));
    HIPCHK(hipEventRecord(c->ev[E_PPART], s));
    hipLaunchKernelGGL(fj_gt_pair_agg_sweep_kernel, dim3(gt_grid(cap)), dim3(1024), 0, s, ka, kb, (u64)nb, tab, cap - 1, acc, d_ok, d_ov, (u64)cap_out,
                       &c->d_sc->total, &c->d_sc->err);
    HIPCHK(hipGetLastError());
    if (gt_close(c, s, t)) return 1;
    *out_count = c->h_sc->total;
    if (c->h_sc->err & FJ_ERR_OUTCAP) return pair_outcap_error(c->h_sc->total, cap_out);      // (g goes back with the error)
    return 0;
}

// FJ_ALGO_GROUP_BY | FJ_ALGO_KEY_PAIR | FJ_ALGO_AGG_ALL (fj_join_device has checked the arguments): the g distinct pairs of
// (ka[i], kb[i]), i < nb <= 2^40 - column A in d_ok, column B in plane 0 of d_ov - and in planes 1..4 of cap_out words their row
// counts and the sums, minima and maxima of kv; kind 0 / 1 / 2: the words of kv as uint64 / int64 / binary64.  cap_out >= 1 is all that
// is asked: g > cap_out fails here, after the device work.  use_radix: the partitioned plan over the combined words, else the global
// table of row indices
int group_by_pair_agg(fj_ctx* c, bool use_radix, const u64* ka, const u64* kb, const u64* kv, size_t nb, int top_bits, hipStream_t s,
                      fj_timings* t, u64* out_count, u64* d_ok, u64* d_ov, size_t cap_out, int kind) {
    *out_count = 0;
    if (nb == 0) return 0;
    if ((u64)nb >> 32) use_radix = false;                    // (the LDS table counts in u32)
    if (!use_radix) return group_by_pair_agg_global(c, ka, kb, kv, nb, s, t, out_count, d_ok, d_ov, cap_out, kind);

    void* p;
    if (get_buf(c, W_PAIR_WORDS, nb * 8, &p)) return 1;
    u64* words = (u64*)p;
    RelAttempt r;
    if (rel_begin(c, nb, top_bits, GQ_TS / 2, s, &r)) return 1;          // aim at half of the table's 2048 slots per partition
    HIPCHK(fj_launch_pair_combine(ka, kb, words, (u64)nb, s));           // (inside build_phase_ms)
    if (rel_passes(c, words, REL_POSITIONS, nullptr, nb, top_bits, s, &r)) return 1;   // the rows' positions travel through the passes; the kernel gathers B and V
    FjGroupByArgs ga{};
    ga.rel = r.rel; ga.nparts = r.nparts;
    ga.out_keys = d_ok; ga.out_vals = d_ov; ga.out_capacity = cap_out;
    ga.cursor = &c->d_sc->total; ga.err = &c->d_sc->err;
    HIPCHK(launch_pair_agg_lds(ga, kb, kv, nb, kind, s));
    if (rel_close(c, r.plan, r.nparts, s, t)) return 1;
    if (c->h_sc->err & (FJ_ERR_LDS_FULL | FJ_ERR_PAIR_COLLISION))        // a partition beyond the LDS table, or two pairs on one word: the whole call on the HBM table
        return gt_fallback(t, [&](fj_timings* g) { return group_by_pair_agg_global(c, ka, kb, kv, nb, s, g, out_count, d_ok, d_ov, cap_out, kind); });
    *out_count = c->h_sc->total;
    if (c->h_sc->err & FJ_ERR_OUTCAP) {
        if (c->h_sc->total > cap_out) return pair_outcap_error(c->h_sc->total, cap_out);     // (g goes back with the error)
        return set_err("internal error: group-by met a row position beyond the relation");
    }
    return 0;
}

}  // namespace fjh
