// fj_groupby_arg.hip -- group-by on ONE relation that returns, per distinct key, the ROW that holds the minimum or the maximum of the
// value column (an EXTENSION: FJ_ALGO_GROUP_BY | FJ_ALGO_AGG_ARG | FJ_ALGO_AGG_MIN or FJ_ALGO_AGG_MAX, include/flashjoin.h): the distinct
// keys, densely packed, and beside each the smallest row index whose value is the group's extreme, and that extreme - pandas' idxmin /
// idxmax, SQL's arg_min / DISTINCT ON ... ORDER BY.  "Cheapest offer per product" wants the offer, not only its price: the caller
// gathers the row's other columns with the index.  Composed from the single forms it is group_by_min, a lookup of that minimum back
// onto every row with a compare, and a second group_by_min over the surviving rows' positions: three trips through the partition passes.
//
// A pass carries ONE payload plane beside the keys and this form needs two things per row, its value and its position.  The passes
// carry the POSITIONS (PassIter::vals_pos, as FJ_ALGO_ROW_IDS and FJ_ALGO_INVERSE do) and the kernel reads values[position] itself: one
// 8-byte random gather per row on a partitioned plan; on a zero-pass plan the position is the flat index and the read is coalesced.
//
// The kernel is fj_group_by_all_kernel's table with two planes behind the keys: one workgroup per WHOLE final partition, the LDS table
// of csrc/fj_lds_table_dev.h (home slot FJ_HW2(key) & (TS - 1), linear probing, one 64-bit CAS per claim, inserts bounded by TS steps,
// `full` behind LIMIT = TS - TS / 16, the marker key out of band in the header with a value and a position word of its own).
//
// LDS budget, TS = 4096 slots (LIMIT 3840):  key 8 B + value 8 B + position 8 B = 24 B per slot,
//   24 B * 4096 = 98 304 B, + the 64-byte header = 98 368 B of the 163 840 B one workgroup may take.
// 8192 slots would be 196 608 B.  So the plan aims at 2048 rows per partition, as the four-aggregate form does.
//
// Three phases over one partition:
//   stream   every row inserts or finds its key, gathers its value and does ONE gj_combine (csrc/fj_group_dev.h) of the MIN or MAX
//            kind on the value plane, which starts at gj_identity.  No barrier, no global store; the next round's keys and positions
//            are requested before this round's work.
//   resolve  behind a barrier the value plane holds every group's extreme.  A row whose value EQUALS its slot's extreme (integers by
//            bits, floats as numbers: -0.0 == +0.0, a NaN equals nothing) does one 64-bit LDS atomicMin of its position on the
//            position plane, which starts at all ones: the smallest index wins, for argmin and argmax alike.  The table probe is
//            read-only.  A partition of one round (the plan's 2048 rows fit it) resolves from the registers the stream left; a longer
//            one (duplicates, a hot key) streams its chunks again, as fj_group_by_inverse_kernel's stream 2 does, values included.
//   emit     fj_group_by_kernel's: one global atomic reserves the partition's rows on the call's cursor, ballot + popcount ranks the
//            occupied slots, a slot stores its key, its position (plane 0 of out_vals) and its value (plane 1), the marker key last.
// Every group has a row, so every position is a row index - also where the extreme equals the aggregate's identity: the rows that
// hold it compare equal to the untouched plane.  Only a group whose extreme is a NaN keeps all ones (-1 as int64).
//
// Fallback: FJ_ERR_LDS_FULL, a partition of more than 3840 distinct keys, which writes nothing; the HBM-table
// kernels end this file.
//
// Weak spot: a key that owns a large share of the rows is streamed by the one workgroup of its partition - here TWICE, since such a
// partition is longer than one round - and where its values tie, the position atomics hit one address too.  Correct at any
// distribution (DESIGN.md "The row of each group's extreme").
#include "fj_host.h"
#include "fj_group_dev.h"

namespace {

constexpr u32 GR_TS = 4096, GR_LIMIT = GR_TS - GR_TS / 16;
using fjh::KIND_UNSIGNED; using fjh::KIND_SIGNED; using fjh::KIND_FLOAT;        // the `kind` of the value column (fj_host.h)

// 64 B: the key slots behind it stay 16-byte aligned.  empty_*: the marker key's value and position words
struct GrHdr { u32 full, has_empty, nkeys, cursor; u64 empty_val, empty_pos, base; u64 pad[3]; };
static_assert(sizeof(GrHdr) == 64, "GrHdr");
constexpr u32 GR_LDS = (u32)sizeof(GrHdr) + GR_TS * 24u;
static_assert(GR_LDS == 98368u && GR_LDS <= 163840u, "the table must fit one workgroup's LDS");
static_assert(GR_TS % GJ_NT == 0, "the emit sweeps whole waves");

template <int KIND, bool IS_MAX> struct GrAgg {
    static constexpr int AGG = KIND == KIND_FLOAT ? (IS_MAX ? FJ_GJ_MAX_F : FJ_GJ_MIN_F) :
                               KIND == KIND_SIGNED ? (IS_MAX ? FJ_GJ_MAX_S : FJ_GJ_MIN_S) : (IS_MAX ? FJ_GJ_MAX_U : FJ_GJ_MIN_U);
};

// does the row's value equal the group's extreme?  Integers by bits; floats as numbers (both zeros tie, a NaN equals nothing)
template <int KIND> __device__ __forceinline__ bool gr_same(u64 v, u64 ext) {
    if constexpr (KIND == KIND_FLOAT) return __longlong_as_double((long long)v) == __longlong_as_double((long long)ext);
    else return v == ext;
}

// Rounds of FOUR rows per thread here, not the eight of the other group-by kernels: two rounds of key, position and value in flight do
// not fit the 128 VGPRs of a 1024-thread workgroup at eight (39 spilled registers, profiles/group_by_arg_kernel_resources.txt).  One
// round is 4096 rows, so the plan's 2048-row partition is still a single round.  gb_load_round (csrc/fj_group_dev.h) at that width
constexpr u32 GR_KPT = 4, GR_ROUND_CHUNKS = GJ_NT * GR_KPT / FJ_CHUNK;
__device__ __forceinline__ void gr_load_round(const FjChunkSet& rel, u32 b0, u32 nbc, u32 c0, u32 tid, u64 (&kk)[GR_KPT], u64 (&pp)[GR_KPT], u32& ok) {
    ok = 0;
#pragma unroll
    for (u32 u = 0; u < GR_KPT; ++u) {
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

// the values of one round's rows: vcol[position].  A position at or beyond nrows (the passes make none) is not read
__device__ __forceinline__ void gr_gather(const u64* __restrict__ vcol, u64 nrows, const u64 (&ps)[GR_KPT], u32& ok, u64 (&v)[GR_KPT], u32* err) {
#pragma unroll
    for (u32 u = 0; u < GR_KPT; ++u) {
        v[u] = 0;
        if (!((ok >> u) & 1u)) continue;
        if (ps[u] < nrows) v[u] = vcol[ps[u]];
        else { ok &= ~(1u << u); atomicOr(err, FJ_ERR_OUTCAP); }
    }
}

// a.rel.vals: the rows' positions (the first pass made them; flat arrays: the index); vcol: the value column, nrows words.
// a.out_vals: two planes of a.out_capacity words - the row index, the extreme value
template <int KIND, bool IS_MAX>
__global__ __launch_bounds__(GJ_NT, 1) void fj_group_by_arg_kernel(FjGroupByArgs a, const u64* __restrict__ vcol, u64 nrows) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    GrHdr* hdr = reinterpret_cast<GrHdr*>(smem);
    u64* tkeys = reinterpret_cast<u64*>(smem + sizeof(GrHdr));
    u64* aval = tkeys + GR_TS;
    u64* apos = aval + GR_TS;
    constexpr int AGG = GrAgg<KIND, IS_MAX>::AGG;
    constexpr u64 IDENT = gj_identity<AGG>();
    const u32 tid = threadIdx.x, lane = tid & 63;
    const u32 p = blockIdx.x;
    u32 b0, nbc;
    fj_part_chunks(a.rel, p, b0, nbc);
    if (nbc == 0) return;

    for (u32 i = tid; i < GR_TS; i += GJ_NT) { tkeys[i] = FJ_EMPTY_KEY; aval[i] = IDENT; apos[i] = ~0ull; }
    if (tid == 0) { hdr->full = 0; hdr->has_empty = 0; hdr->nkeys = 0; hdr->cursor = 0; hdr->empty_val = IDENT; hdr->empty_pos = ~0ull; hdr->base = 0; }
    __syncthreads();

    // ---- stream: rounds of GJ_NT * GR_KPT rows; the next round's keys and positions are requested before this round's inserts, its
    // values behind them.  No global store, no barrier inside the loop ----
    u64 k[GR_KPT], ps[GR_KPT], v[GR_KPT];
    u32 okm = 0;
    gr_load_round(a.rel, b0, nbc, 0, tid, k, ps, okm);
    gr_gather(vcol, nrows, ps, okm, v, a.err);
    for (u32 c0 = 0; c0 < nbc; c0 += GR_ROUND_CHUNKS) {
        const bool more = c0 + GR_ROUND_CHUNKS < nbc;
        u64 kn[GR_KPT], pn[GR_KPT];
        u32 okn = 0;
        if (more) gr_load_round(a.rel, b0, nbc, c0 + GR_ROUND_CHUNKS, tid, kn, pn, okn);
#pragma unroll
        for (u32 u = 0; u < GR_KPT; ++u) {
            if (!((okm >> u) & 1u)) continue;
            const u64 key = a.rel.list ? k[u] : fj_key_mix(k[u]);                 // chunk pools hold mixed keys, flat arrays raw ones
            if (key == FJ_EMPTY_KEY) {                       // the empty marker is never stored in the table
                hdr->has_empty = 1;
                gj_combine<AGG>(&hdr->empty_val, v[u]);
                continue;
            }
            if (*(volatile u32*)&hdr->full) continue;        // the item is lost already: the rest of its rows do no table work
            u32 pos = FJ_HW2(key) & (GR_TS - 1);
            bool placed = false;
            for (u32 step = 0; step < GR_TS; ++step) {
                u64 t = tkeys[pos];                          // (a slot never changes once it holds a key: a stale read costs a CAS at most)
                if (t == FJ_EMPTY_KEY) {
                    t = atomicCAS((unsigned long long*)&tkeys[pos], (unsigned long long)FJ_EMPTY_KEY, (unsigned long long)key);
                    if (t == FJ_EMPTY_KEY) {
                        if (atomicAdd(&hdr->nkeys, 1u) >= GR_LIMIT) hdr->full = 1;
                        t = key;
                    }
                }
                if (t == key) { placed = true; break; }
                pos = (pos + 1) & (GR_TS - 1);
            }
            if (!placed) { hdr->full = 1; continue; }
            gj_combine<AGG>(&aval[pos], v[u]);
        }
        if (more) {                                          // (a partition of one round keeps its rows in registers for the resolve)
#pragma unroll
            for (u32 u = 0; u < GR_KPT; ++u) { k[u] = kn[u]; ps[u] = pn[u]; }
            okm = okn;
            gr_gather(vcol, nrows, ps, okm, v, a.err);
        }
    }
    __syncthreads();
    if (hdr->full) { if (tid == 0) atomicOr(a.err, FJ_ERR_LDS_FULL); return; }     // nothing written: the host re-runs the call on the HBM table

    // ---- resolve: the value plane is final.  A row that holds its group's extreme offers its position; the smallest one stays ----
    auto resolve_round = [&](const u64 (&kk)[GR_KPT], const u64 (&pp)[GR_KPT], const u64 (&vv)[GR_KPT], u32 ok) {
#pragma unroll
        for (u32 u = 0; u < GR_KPT; ++u) {
            if (!((ok >> u) & 1u)) continue;
            const u64 key = a.rel.list ? kk[u] : fj_key_mix(kk[u]);
            if (key == FJ_EMPTY_KEY) {
                if (gr_same<KIND>(vv[u], hdr->empty_val)) atomicMin((unsigned long long*)&hdr->empty_pos, (unsigned long long)pp[u]);
                continue;
            }
            u32 pos = FJ_HW2(key) & (GR_TS - 1);
            for (u32 step = 0; step < GR_TS && tkeys[pos] != key; ++step) pos = (pos + 1) & (GR_TS - 1);      // (the stream placed every key)
            if (gr_same<KIND>(vv[u], aval[pos])) atomicMin((unsigned long long*)&apos[pos], (unsigned long long)pp[u]);
        }
    };
    if (nbc <= GR_ROUND_CHUNKS) resolve_round(k, ps, v, okm);                      // (uniform: the whole partition is in registers)
    else {
        gr_load_round(a.rel, b0, nbc, 0, tid, k, ps, okm);
        gr_gather(vcol, nrows, ps, okm, v, a.err);
        for (u32 c0 = 0; c0 < nbc; c0 += GR_ROUND_CHUNKS) {
            const bool more = c0 + GR_ROUND_CHUNKS < nbc;
            u64 kn[GR_KPT], pn[GR_KPT];
            u32 okn = 0;
            if (more) gr_load_round(a.rel, b0, nbc, c0 + GR_ROUND_CHUNKS, tid, kn, pn, okn);
            resolve_round(k, ps, v, okm);
            if (more) {
#pragma unroll
                for (u32 u = 0; u < GR_KPT; ++u) { k[u] = kn[u]; ps[u] = pn[u]; }
                okm = okn;
                gr_gather(vcol, nrows, ps, okm, v, a.err);
            }
        }
    }
    __syncthreads();

    // ---- emit: one global atomic reserves [o, o + g_p); the table's occupied slots take ranks inside it, the marker key the last ----
    const u32 nk = hdr->nkeys;
    const bool has_empty = hdr->has_empty != 0;
    if (tid == 0) hdr->base = (u64)atomicAdd(a.cursor, (unsigned long long)(nk + (has_empty ? 1u : 0u)));
    __syncthreads();
    const u64 o = hdr->base, cap = a.out_capacity;
    u64* const ov = a.out_vals;
    for (u32 i = tid; i < GR_TS; i += GJ_NT) {               // (GR_TS is a multiple of GJ_NT: whole waves every round)
        const u64 key = tkeys[i];
        const bool occ = key != FJ_EMPTY_KEY;
        const unsigned long long m = __ballot(occ);
        u32 wbase = 0;
        if (lane == 0 && m) wbase = atomicAdd(&hdr->cursor, (u32)__popcll(m));
        wbase = __shfl(wbase, 0, 64);
        if (!occ) continue;
        const u64 row = o + wbase + (u32)__popcll(m & ((1ull << lane) - 1ull));
        if (row < cap) { a.out_keys[row] = fj_key_unmix(key); ov[row] = apos[i]; ov[cap + row] = aval[i]; }
        else atomicOr(a.err, FJ_ERR_OUTCAP);
    }
    if (tid == 0 && has_empty) {
        const u64 row = o + nk;
        if (row < cap) { a.out_keys[row] = fj_key_unmix(FJ_EMPTY_KEY); ov[row] = hdr->empty_pos; ov[cap + row] = hdr->empty_val; }
        else atomicOr(a.err, FJ_ERR_OUTCAP);
    }
}

// ---- the global-table form.  The table is fj_gt_build_first_kernel's, keys only (csrc/fj_join.hip: raw keys, the raw empty key out
// of band); ext and pos: planes of capacity + 1 words, the last word of each the empty key's.  fj_gt_group_by_combine_kernel
// (csrc/fj_groupby.hip) has taken the extreme per slot into ext; pos holds all ones ----
// thread per row of the relation: a row whose value equals its slot's extreme offers its index.  Coalesced reads of the flat arrays
template <int KIND>
__global__ __launch_bounds__(1024) void fj_gt_group_by_arg_resolve_kernel(FjGtArgs a, const u64* __restrict__ vals, const u64* __restrict__ ext, u64* pos) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < a.nb; i += stride) {
        const u64 key = a.bk[i];
        u64 where = a.cap_mask + 1;
        if (key != FJ_EMPTY_KEY && !gj_gt_find(a.tkeys, a.cap_mask, key, where)) continue;
        if (gr_same<KIND>(vals[i], ext[where])) atomicMin((unsigned long long*)&pos[where], (unsigned long long)i);
    }
}

// the capacity + 1 slots, compacted: an occupied slot's key, position and extreme go to the row a wave-aggregated cursor hands out
// (one global atomic per wave that holds a key), the two planes of out_vals at stride out_capacity
__global__ __launch_bounds__(1024) void fj_gt_group_by_arg_sweep_kernel(FjGtArgs a, const u64* __restrict__ ext, const u64* __restrict__ pos,
                                                                        u64* __restrict__ out_keys, u64* __restrict__ out_vals, u64 out_capacity,
                                                                        unsigned long long* cursor, u32* err) {
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
        if (!occ) continue;
        const u64 row = wbase + (u32)__popcll(m & ((1ull << lane) - 1ull));
        if (row < out_capacity) { out_keys[row] = key; out_vals[row] = pos[i]; out_vals[out_capacity + row] = ext[i]; }
        else atomicOr(err, FJ_ERR_OUTCAP);
    }
}

template <int KIND> void (*gr_kernel(bool is_max))(FjGroupByArgs, const u64*, u64) {
    return is_max ? fj_group_by_arg_kernel<KIND, true> : fj_group_by_arg_kernel<KIND, false>;
}

}  // namespace

hipError_t fj_launch_group_by_arg(const FjGroupByArgs& a, const u64* vals, u64 nrows, int kind, bool is_max, hipStream_t s) {
    if (kind < KIND_UNSIGNED || kind > KIND_FLOAT || !a.cursor || !a.err || !a.nparts || !a.out_keys || !a.out_vals || !vals) return hipErrorInvalidValue;
    if (a.out_capacity < nrows) return hipErrorInvalidValue;                       // (every row may be a group of its own)
    if (!a.rel.list ? a.rel.n_flat > nrows : !a.rel.vals) return hipErrorInvalidValue;      // (a chunk pool without positions has nothing to gather by)
    void (*kern)(FjGroupByArgs, const u64*, u64) = kind == KIND_UNSIGNED ? gr_kernel<KIND_UNSIGNED>(is_max) :
                                                   kind == KIND_SIGNED ? gr_kernel<KIND_SIGNED>(is_max) : gr_kernel<KIND_FLOAT>(is_max);
    hipError_t e = fj_set_max_lds_once(reinterpret_cast<const void*>(kern), GR_LDS);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(a.nparts), dim3(GJ_NT), GR_LDS, s, a, vals, nrows);
    return hipGetLastError();
}

hipError_t fj_launch_gt_group_by_arg_resolve(const FjGtArgs& a, int kind, const u64* vals, const u64* ext, u64* pos, hipStream_t s) {
    if (kind < KIND_UNSIGNED || kind > KIND_FLOAT || !vals || !ext || !pos) return hipErrorInvalidValue;
    if (!a.nb) return hipSuccess;
    hipLaunchKernelGGL(kind == KIND_FLOAT ? fj_gt_group_by_arg_resolve_kernel<KIND_FLOAT> : fj_gt_group_by_arg_resolve_kernel<KIND_UNSIGNED>,
                       dim3(fjh::gt_grid(a.nb)), dim3(1024), 0, s, a, vals, ext, pos);      // (signed words compare equal by bits too)
    return hipGetLastError();
}

hipError_t fj_launch_gt_group_by_arg_sweep(const FjGtArgs& a, const u64* ext, const u64* pos, u64* out_keys, u64* out_vals, u64 out_capacity,
                                           unsigned long long* cursor, u32* err, hipStream_t s) {
    if (!cursor || !err || !ext || !pos || !out_keys || !out_vals || !out_capacity) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fj_gt_group_by_arg_sweep_kernel, dim3(fjh::gt_grid(a.cap_mask + 2)), dim3(1024), 0, s, a, ext, pos, out_keys, out_vals,
                       out_capacity, cursor, err);
    return hipGetLastError();
}

namespace fjh {

// the global-table form (fj_host.h): a plane of extremes and a plane of positions, capacity + 1 words each.  Every kernel on the one
// stream
static int group_by_arg_global(fj_ctx* c, const u64* bk, const u64* bv, size_t nb, hipStream_t s, fj_timings* t, u64* out_count,
                               u64* d_ok, u64* d_ov, size_t cap_out, int kind, bool is_max) {
    const u64 plane = gt_capacity(nb) + 1;
    FjGtArgs a{};
    u64* ext = nullptr;
    if (gt_open(c, nb, 2 * plane, s, &a, &ext)) return 1;
    u64* pos = ext + plane;
    a.bk = bk;
    const int agg = kind_agg(kind, is_max ? PLANE_MAX : PLANE_MIN);
    HIPCHK(fj_launch_gt_build_first(a, false, s));
    HIPCHK(fj_launch_group_fill(ext, plane, agg, s));
    HIPCHK(hipMemsetAsync(pos, 0xFF, plane * 8, s));
    HIPCHK(fj_launch_gt_group_by_combine(a, agg, bv, ext, s));
    HIPCHK(hipEventRecord(c->ev[E_BUILD], s));
    HIPCHK(hipEventRecord(c->ev[E_PPART], s));
    HIPCHK(fj_launch_gt_group_by_arg_resolve(a, kind, bv, ext, pos, s));
    HIPCHK(fj_launch_gt_group_by_arg_sweep(a, ext, pos, d_ok, d_ov, cap_out, &c->d_sc->total, &c->d_sc->err, s));
    if (gt_close(c, s, t)) return 1;
    if (c->h_sc->err & FJ_ERR_OUTCAP) return distinct_error();
    *out_count = c->h_sc->total;
    return 0;
}

// FJ_ALGO_GROUP_BY | FJ_ALGO_AGG_ARG (fj_join_device has checked the arguments): the g distinct keys of bk[0 .. nb) in d_ok and, in the
// two planes of cap_out words of d_ov, the smallest row index that holds the minimum (is_max: the maximum) of bv over the key's rows,
// and that extreme; kind 0 / 1 / 2: the words of bv as uint64 / int64 / binary64.  g <= nb <= cap_out.
// use_radix: the partitioned plan, else the global table
int group_by_arg(fj_ctx* c, bool use_radix, const u64* bk, const u64* bv, size_t nb, int top_bits, hipStream_t s, fj_timings* t,
                 u64* out_count, u64* d_ok, u64* d_ov, size_t cap_out, int kind, bool is_max) {
    *out_count = 0;
    if (nb == 0) return 0;
    if (!use_radix) return group_by_arg_global(c, bk, bv, nb, s, t, out_count, d_ok, d_ov, cap_out, kind, is_max);

    RelAttempt r;      // aim at half of the table's 4096 slots per partition; the rows' positions travel, the kernel gathers the values
    if (rel_open(c, bk, REL_POSITIONS, nullptr, nb, top_bits, GR_TS / 2, s, &r)) return 1;
    FjGroupByArgs ga{};
    ga.rel = r.rel; ga.nparts = r.nparts;
    ga.out_keys = d_ok; ga.out_vals = d_ov; ga.out_capacity = cap_out;
    ga.cursor = &c->d_sc->total; ga.err = &c->d_sc->err;
    HIPCHK(fj_launch_group_by_arg(ga, bv, nb, kind, is_max, s));
    if (rel_close(c, r.plan, r.nparts, s, t)) return 1;
    if (c->h_sc->err & FJ_ERR_LDS_FULL)                      // a partition beyond the LDS table: the whole call on the HBM table
        return gt_fallback(t, [&](fj_timings* g) { return group_by_arg_global(c, bk, bv, nb, s, g, out_count, d_ok, d_ov, cap_out, kind, is_max); });
    if (c->h_sc->err & FJ_ERR_OUTCAP) return set_err("internal error: group-by met a row position beyond the relation, or more distinct keys than rows");
    *out_count = c->h_sc->total;
    return 0;
}

}  // namespace fjh
