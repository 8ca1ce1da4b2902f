// fj_groupby_pair.hip -- the dense group id of every row under a TWO-COLUMN key (an EXTENSION: FJ_ALGO_GROUP_BY | FJ_ALGO_INVERSE |
// FJ_ALGO_KEY_PAIR, include/flashjoin.h): rows i and j share an id iff A[i] == A[j] && B[i] == B[j].  Beside the nb ids the call returns,
// per group, the ROW INDEX of the group's first occurrence - the caller gathers A[idx], B[idx] and any other column with it, as with
// join_indices and group_by_argmin.  Composed from the single-key forms it is factorize(A), factorize(B), a multiply-add of the two
// code columns and a third factorize: three trips through the partition passes.
//
// A pair becomes ONE word, w = fj_key_pair(a, b) = a ^ fj_key_mix(b ^ C) (csrc/fj_common.h): a streaming kernel writes the nb words
// into a workspace buffer and the relation's partition passes run over that buffer, carrying the rows' positions beside the words
// (PassIter::vals_pos).  On a zero-pass plan the kernel below reads that same buffer as a flat array; the position is the flat index.
// The map is not injective - two distinct pairs share a word with probability ~n^2 / 2^65 per call on natural data, and such pairs are
// trivial to craft - so every row's pair is COMPARED with its group's before the call's result counts, and a mismatch sends the whole
// call to the exact global-table form below.  The result is exact at any input.
//
// fj_group_by_pair_kernel is a sibling of fj_group_by_inverse_kernel (csrc/fj_groupby.hip): one workgroup of 1024 threads per WHOLE
// final partition, the 8192-slot LDS table of csrc/fj_lds_table_dev.h over the mixed words, the marker word out of band in the header.
//   stream 1  every row finds or inserts its word (a plain read, CAS on an empty slot, linear probing) and does one 64-bit LDS atomic
//             minimum of its position on the word behind the slot, which starts at all ones: the smallest position is the group's
//             representative, and the first occurrence the call returns.
//   rank      one global atomic reserves [o, o + g_p); an occupied slot takes rank r by wave ballot + popcount, out_keys[o + r] = the
//             slot's smallest position, and r moves into the top 24 bits of the word behind the slot, above the position's 40 (nb <= 2^40
//             is checked by the entry points).  The marker's group is last.
//   stream 2  the same chunks again, words and positions: a read-only probe, out_vals[position] = o + r, and the VERIFICATION - the
//             row gathers its own pair A[position], B[position] and its slot's representative pair A[rep], B[rep] (at most a few
//             thousand representatives per partition) and raises FJ_ERR_PAIR_COLLISION where they differ.  A row that IS the
//             representative reads and compares nothing.
// Position and rank share the one word behind each of the 8192 slots (16 B per slot, 131 136 B with the header) rather than taking a
// third plane at 4096 slots: the partitions are then factorize's own - the plan, the table's load and the `full` limit of 7680
// distinct words are unchanged, and half as many workgroups stream twice as much each.
// Rounds of EIGHT rows per thread, fj_group_by_inverse_kernel's (gb_load_round, csrc/fj_group_dev.h): stream 2 holds two rounds of
// word and position plus the round's slot words and own pairs in 118 of the 128 VGPRs, no scratch; at four rows it is 66
// (profiles/group_by_pair_kernel_resources.txt).  Eight keep twice as many gathers in flight per thread.
//
// Fallback: FJ_ERR_LDS_FULL (a partition of more than 7680 distinct words) or FJ_ERR_PAIR_COLLISION; the HBM
// table holds ROW INDICES (the kernels at the end of this file) and compares pairs, never words.
//
// Weak spot: a pair that owns a large share of the rows is streamed TWICE by the one workgroup of its partition, its position atomics
// hit one address, and its rows' representative reads hit one line.  Correct at any distribution (DESIGN.md "Two-column keys").
#include "fj_host.h"
#include "fj_group_dev.h"

namespace {

constexpr u32 GP_POS_BITS = 40;
constexpr u64 GP_POS_MASK = (1ull << GP_POS_BITS) - 1ull;

// 64 B: the key slots behind it stay 16-byte aligned.  empty_word: the marker word's slot word (its smallest position, then rank | position)
struct GpHdr { u32 full, has_empty, nkeys, cursor; u64 empty_word, base; u64 pad[4]; };
static_assert(sizeof(GpHdr) == 64, "GpHdr");
constexpr u32 GP_LDS = (u32)sizeof(GpHdr) + GJ_TS * 16u;
static_assert(GP_LDS == 131136u && GP_LDS <= 163840u, "the table must fit one workgroup's LDS");
static_assert(GJ_TS % GJ_NT == 0, "the rank sweep runs whole waves");
static_assert(GJ_TS < (1u << (64 - GP_POS_BITS)), "a slot's rank lies above the position's 40 bits");

// thread per row: the combined word of (A[i], B[i])
__global__ __launch_bounds__(1024) void fj_pair_combine_kernel(const u64* __restrict__ A, const u64* __restrict__ B, u64* __restrict__ out, u64 n) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = fj_key_pair(A[i], B[i]);
}

// a.rel: the combined words (chunk pools: mixed, with the positions in the vals plane; a flat array: raw, the index is the position).
// A, B: the two key columns, nrows words each.  a.out_keys: first-occurrence row indices; a.out_vals: nrows group ids
__global__ __launch_bounds__(GJ_NT, 1) void fj_group_by_pair_kernel(FjGroupByArgs a, const u64* __restrict__ A, const u64* __restrict__ B, u64 nrows) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    GpHdr* hdr = reinterpret_cast<GpHdr*>(smem);
    u64* tkeys = reinterpret_cast<u64*>(smem + sizeof(GpHdr));
    u64* rep = tkeys + GJ_TS;                                // stream 1: the slot's smallest position; from the rank on: rank << 40 | position
    const u32 tid = threadIdx.x, lane = tid & 63;
    const u32 p = blockIdx.x;
    u32 b0, nbc;
    fj_part_chunks(a.rel, p, b0, nbc);
    if (nbc == 0) return;

    for (u32 i = tid; i < GJ_TS; i += GJ_NT) { tkeys[i] = FJ_EMPTY_KEY; rep[i] = ~0ull; }
    if (tid == 0) { hdr->full = 0; hdr->has_empty = 0; hdr->nkeys = 0; hdr->cursor = 0; hdr->empty_word = ~0ull; hdr->base = 0; }
    __syncthreads();

    // ---- stream 1: the words build the table, the positions offer themselves as the slot's representative.  No global store, no
    // barrier inside the loop; the next round's loads are requested before this round's inserts ----
    {
        u64 k[GJ_KPT], ps[GJ_KPT];
        u32 okm = 0;
        gb_load_round<true>(a.rel, b0, nbc, 0, tid, k, ps, okm);
        for (u32 c0 = 0; c0 < nbc; c0 += GJ_ROUND_CHUNKS) {
            u64 kn[GJ_KPT], pn[GJ_KPT];
            u32 okn = 0;
            if (c0 + GJ_ROUND_CHUNKS < nbc) gb_load_round<true>(a.rel, b0, nbc, c0 + GJ_ROUND_CHUNKS, tid, kn, pn, okn);
#pragma unroll
            for (u32 u = 0; u < GJ_KPT; ++u) {
                if (!((okm >> u) & 1u)) continue;
                if (ps[u] >= nrows) { atomicOr(a.err, FJ_ERR_OUTCAP); continue; }         // (the passes make no such position)
                const u64 key = a.rel.list ? k[u] : fj_key_mix(k[u]);                     // chunk pools hold mixed words, the flat buffer raw ones
                if (key == FJ_EMPTY_KEY) {                   // the empty marker is never stored in the table
                    hdr->has_empty = 1;
                    atomicMin((unsigned long long*)&hdr->empty_word, (unsigned long long)ps[u]);
                    continue;
                }
                if (*(volatile u32*)&hdr->full) continue;    // the item is lost already: the rest of its rows do no table work
                u32 pos = FJ_HW2(key) & (GJ_TS - 1);
                bool placed = false;
                for (u32 step = 0; step < GJ_TS; ++step) {
                    u64 t = tkeys[pos];                      // (a slot never changes once it holds a key: a stale read costs a CAS at most)
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
                if (!placed) { hdr->full = 1; continue; }
                atomicMin((unsigned long long*)&rep[pos], (unsigned long long)ps[u]);
            }
#pragma unroll
            for (u32 u = 0; u < GJ_KPT; ++u) { k[u] = kn[u]; ps[u] = pn[u]; }
            okm = okn;
        }
    }
    __syncthreads();
    if (hdr->full) { if (tid == 0) atomicOr(a.err, FJ_ERR_LDS_FULL); return; }     // (uniform: every thread reads the word behind the barrier)

    // ---- reserve and rank: the emit of fj_group_by_inverse_kernel; out_keys receives the representative's position, and the slot's
    // rank joins that position in the word behind the slot ----
    const u32 nk = hdr->nkeys;
    const bool has_empty = hdr->has_empty != 0;
    if (tid == 0) hdr->base = (u64)atomicAdd(a.cursor, (unsigned long long)(nk + (has_empty ? 1u : 0u)));
    __syncthreads();
    const u64 o = hdr->base;
    for (u32 i = tid; i < GJ_TS; i += GJ_NT) {               // (GJ_TS is a multiple of GJ_NT: whole waves every round)
        const bool occ = tkeys[i] != FJ_EMPTY_KEY;
        const unsigned long long m = __ballot(occ);
        u32 wbase = 0;
        if (lane == 0 && m) wbase = atomicAdd(&hdr->cursor, (u32)__popcll(m));
        wbase = __shfl(wbase, 0, 64);
        if (!occ) continue;
        const u32 r = wbase + (u32)__popcll(m & ((1ull << lane) - 1ull));
        const u64 first = rep[i] & GP_POS_MASK;
        rep[i] = ((u64)r << GP_POS_BITS) | first;
        if (o + r < a.out_capacity) a.out_keys[o + r] = first;
        else atomicOr(a.err, FJ_ERR_OUTCAP);
    }
    if (tid == 0 && has_empty) {
        const u64 first = hdr->empty_word & GP_POS_MASK;
        hdr->empty_word = ((u64)nk << GP_POS_BITS) | first;
        if (o + nk < a.out_capacity) a.out_keys[o + nk] = first;
        else atomicOr(a.err, FJ_ERR_OUTCAP);
    }
    __syncthreads();

    // ---- stream 2: every row finds its word's slot in the finished table, stores the slot's id at its position and compares its
    // pair with the representative's ----
    const u64 empty_word = hdr->empty_word;
    bool differs = false;
    u64 k[GJ_KPT], ps[GJ_KPT];
    u32 okm = 0;
    gb_load_round<true>(a.rel, b0, nbc, 0, tid, k, ps, okm);
    for (u32 c0 = 0; c0 < nbc; c0 += GJ_ROUND_CHUNKS) {
        u64 kn[GJ_KPT], pn[GJ_KPT];
        u32 okn = 0;
        if (c0 + GJ_ROUND_CHUNKS < nbc) gb_load_round<true>(a.rel, b0, nbc, c0 + GJ_ROUND_CHUNKS, tid, kn, pn, okn);
        u64 oa[GJ_KPT], ob[GJ_KPT], w[GJ_KPT];
#pragma unroll
        for (u32 u = 0; u < GJ_KPT; ++u) {                   // the slot words first: they say which rows have a pair to fetch at all
            w[u] = 0;
            if (!((okm >> u) & 1u)) continue;
            if (ps[u] >= nrows) { okm &= ~(1u << u); continue; }                          // (stream 1 reported it)
            const u64 key = a.rel.list ? k[u] : fj_key_mix(k[u]);
            w[u] = empty_word;
            if (key != FJ_EMPTY_KEY) {
                u32 pos = FJ_HW2(key) & (GJ_TS - 1);
                for (u32 step = 0; step < GJ_TS && tkeys[pos] != key; ++step) pos = (pos + 1) & (GJ_TS - 1);      // (stream 1 placed every word)
                w[u] = rep[pos];
            }
            if ((w[u] & GP_POS_MASK) == ps[u]) okm |= 0x100u << u;                        // the row IS the representative: nothing to compare
        }
#pragma unroll
        for (u32 u = 0; u < GJ_KPT; ++u) {                   // the rows' own pairs: two 8-byte random reads each
            oa[u] = 0; ob[u] = 0;
            if (((okm >> u) & 0x101u) != 1u) continue;
            oa[u] = A[ps[u]]; ob[u] = B[ps[u]];
        }
#pragma unroll
        for (u32 u = 0; u < GJ_KPT; ++u) {
            if (!((okm >> u) & 1u)) continue;
            a.out_vals[ps[u]] = o + (w[u] >> GP_POS_BITS);   // (ps < nrows <= out_capacity: the launch checks it)
            if ((okm >> u) & 0x100u) continue;
            const u64 r = w[u] & GP_POS_MASK;                // (a minimum over positions stream 1 checked: the bound is never met)
            if (r >= nrows) { atomicOr(a.err, FJ_ERR_OUTCAP); continue; }
            if (A[r] != oa[u] || B[r] != ob[u]) differs = true;
        }
#pragma unroll
        for (u32 u = 0; u < GJ_KPT; ++u) { k[u] = kn[u]; ps[u] = pn[u]; }
        okm = okn;
    }
    if (differs) atomicOr(a.err, FJ_ERR_PAIR_COLLISION);
}

// ---- the exact global-table form: ONE table of ROW INDICES, capacity words, all ones at rest (no row index is all ones: nothing is
// kept out of band).  A slot names a pair by one of its rows; rows are compared by their pairs, never by their combined words ----
// thread per row i: empty home or next slot -> CAS i in; a slot whose row holds the same pair -> atomicMin (the slot keeps naming that
// pair, now by a smaller row); another pair -> the next slot.  capacity >= 2 nb: an empty slot is always met
__global__ __launch_bounds__(1024) void fj_gt_pair_build_kernel(const u64* __restrict__ A, const u64* __restrict__ B, u64 nb, u64* tab, u64 cap_mask) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < nb; i += stride) {
        const u64 ka = A[i], kb = B[i];
        u64 pos = fj_hash64(fj_key_pair(ka, kb)) & cap_mask;
        for (u64 step = 0; step <= cap_mask; ++step) {
            u64 t = *(volatile u64*)&tab[pos];
            if (t == ~0ull) {
                t = atomicCAS((unsigned long long*)&tab[pos], ~0ull, (unsigned long long)i);
                if (t == ~0ull) break;
            }
            if (t < nb && A[t] == ka && B[t] == kb) { atomicMin((unsigned long long*)&tab[pos], (unsigned long long)i); break; }
            pos = (pos + 1) & cap_mask;
        }
    }
}

// the capacity slots, compacted: an occupied slot takes the id a wave-aggregated cursor hands out (one global atomic per wave that
// holds a row), out_keys[id] = the slot's row - its pair's smallest - and ids[slot] = id
__global__ __launch_bounds__(1024) void fj_gt_pair_sweep_kernel(const u64* __restrict__ tab, u64 cap_mask, u64* __restrict__ ids, u64* __restrict__ out_keys,
                                                                u64 out_capacity, unsigned long long* cursor, u32* err) {
    const u64 cap = cap_mask + 1;
    const u32 lane = threadIdx.x & 63;
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 w0 = (u64)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); w0 < cap; w0 += stride) {      // (uniform per wave; capacity is a multiple of 64)
        const u64 i = w0 + lane;
        const u64 row = tab[i];
        const bool occ = row != ~0ull;
        const unsigned long long m = __ballot(occ);
        if (!m) continue;
        unsigned long long wbase = 0;
        if (lane == 0) wbase = atomicAdd(cursor, (unsigned long long)__popcll(m));
        wbase = __shfl(wbase, 0, 64);
        if (!occ) continue;
        const u64 id = wbase + (u32)__popcll(m & ((1ull << lane) - 1ull));
        ids[i] = id;
        if (id < out_capacity) out_keys[id] = row;
        else atomicOr(err, FJ_ERR_OUTCAP);
    }
}

// behind the sweep on the same stream, thread per row i: the slot whose row holds i's pair (the build placed every pair), out_vals[i] = its id
__global__ __launch_bounds__(1024) void fj_gt_pair_inverse_kernel(const u64* __restrict__ A, const u64* __restrict__ B, u64 nb, const u64* __restrict__ tab,
                                                                  u64 cap_mask, const u64* __restrict__ ids, u64* __restrict__ out_vals, u64 out_capacity) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    const u64 n = nb < out_capacity ? nb : out_capacity;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const u64 ka = A[i], kb = B[i];
        u64 pos = fj_hash64(fj_key_pair(ka, kb)) & cap_mask;
        for (u64 step = 0; step <= cap_mask; ++step) {
            const u64 t = tab[pos];
            if (t >= nb) break;                              // (an empty slot: the build placed every pair, so this is not met)
            if (A[t] == ka && B[t] == kb) { out_vals[i] = ids[pos]; break; }
            pos = (pos + 1) & cap_mask;
        }
    }
}

hipError_t launch_pair_lds(const FjGroupByArgs& a, const u64* A, const u64* B, u64 nrows, hipStream_t s) {
    if (!a.cursor || !a.err || !a.nparts || !a.out_keys || !a.out_vals || !A || !B) return hipErrorInvalidValue;
    if (a.out_capacity < nrows || nrows > (1ull << GP_POS_BITS)) return hipErrorInvalidValue;      // (every row may be a group of its own; a position takes 40 bits)
    if (!a.rel.list ? a.rel.n_flat > nrows : !a.rel.vals) return hipErrorInvalidValue;              // (a chunk pool without positions has nothing to gather by)
    hipError_t e = fj_set_max_lds_once(reinterpret_cast<const void*>(fj_group_by_pair_kernel), GP_LDS);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fj_group_by_pair_kernel, dim3(a.nparts), dim3(GJ_NT), GP_LDS, s, a, A, B, nrows);
    return hipGetLastError();
}

}  // namespace

// the two kernels FJ_ALGO_KEY_PAIR | FJ_ALGO_AGG_ALL shares (csrc/fj_groupby_pair_agg.hip) have launchers, this one and
// fj_launch_pair_combine at the end of the file: host code only - the kernels above are unchanged and compile to the same resources
// as before (profiles/group_by_pair_agg_kernel_resources.txt).  They sit apart on purpose: tests/test_hbm_table_trips_cpu.py reads
// this file's gt_grid launches IN ORDER - build (nb), sweep (cap), inverse (nb), combine (nb) - to derive its shapes, and each launch
// stays at its old place in that order
hipError_t fj_launch_gt_pair_build(const u64* A, const u64* B, u64 nb, u64* tab, u64 cap_mask, hipStream_t s) {
    if (!A || !B || !tab || cap_mask + 1 < 2 * nb) return hipErrorInvalidValue;          // (capacity >= 2 nb: an empty slot is always met)
    if (!nb) return hipSuccess;
    hipLaunchKernelGGL(fj_gt_pair_build_kernel, dim3(fjh::gt_grid(nb)), dim3(1024), 0, s, A, B, nb, tab, cap_mask);
    return hipGetLastError();
}

extern "C" uint64_t fj_key_pair64(uint64_t a, uint64_t b) { return fj_key_pair(a, b); }

namespace fjh {

// the global-table form (fj_host.h), also the fallback of two pairs on one combined word.  The key plane holds row indices, the value
// plane the slots' ids; the three kernels run in order on the one stream and define every one of the nb ids and all g first rows
static int group_by_pair_global(fj_ctx* c, const u64* ka, const u64* kb, size_t nb, hipStream_t s, fj_timings* t, u64* out_count,
                                u64* d_ok, u64* d_ov, size_t cap_out) {
    const u64 cap = gt_capacity(nb);
    FjGtArgs a{};
    u64* ids = nullptr;                                      // (no fill: the sweep writes every word the inverse kernel reads)
    if (gt_open(c, nb, cap, s, &a, &ids)) return 1;
    u64* tab = a.tkeys;
    HIPCHK(fj_launch_gt_pair_build(ka, kb, (u64)nb, tab, cap - 1, s));
    HIPCHK(hipEventRecord(c->ev[E_BUILD], s));
    HIPCHK(hipEventRecord(c->ev[E_PPART], s));
    hipLaunchKernelGGL(fj_gt_pair_sweep_kernel, dim3(gt_grid(cap)), dim3(1024), 0, s, tab, cap - 1, ids, d_ok, (u64)cap_out, &c->d_sc->total, &c->d_sc->err);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(fj_gt_pair_inverse_kernel, dim3(gt_grid(nb)), dim3(1024), 0, s, ka, kb, (u64)nb, tab, cap - 1, ids, d_ov, (u64)cap_out);
    HIPCHK(hipGetLastError());
    if (gt_close(c, s, t)) return 1;
    if (c->h_sc->err & FJ_ERR_OUTCAP) return set_err("internal error: group-by found more distinct pairs than the relation has rows");
    *out_count = c->h_sc->total;
    return 0;
}

// FJ_ALGO_GROUP_BY | FJ_ALGO_INVERSE | FJ_ALGO_KEY_PAIR (fj_join_device has checked the arguments): the group id of every row of the
// relation (ka[i], kb[i]), i < nb <= 2^40, in d_ov (nb words) and the row index of every group's first occurrence in d_ok (g words);
// g <= nb <= cap_out.  use_radix: the partitioned plan over the combined words, else the global table of row indices
int group_by_pair(fj_ctx* c, bool use_radix, const u64* ka, const u64* kb, size_t nb, int top_bits, hipStream_t s, fj_timings* t,
                  u64* out_count, u64* d_ok, u64* d_ov, size_t cap_out) {
    *out_count = 0;
    if (nb == 0) return 0;
    if (!use_radix) return group_by_pair_global(c, ka, kb, nb, s, t, out_count, d_ok, d_ov, cap_out);

    void* p;
    if (get_buf(c, W_PAIR_WORDS, nb * 8, &p)) return 1;
    u64* words = (u64*)p;
    RelAttempt r;                                            // factorize's plan: the table is its 8192 slots
    if (rel_begin(c, nb, top_bits, 0, s, &r)) return 1;
    HIPCHK(fj_launch_pair_combine(ka, kb, words, (u64)nb, s));           // (inside build_phase_ms)
    if (rel_passes(c, words, REL_POSITIONS, nullptr, nb, top_bits, s, &r)) return 1;   // the rows' positions travel through the passes; the kernel gathers the pairs
    FjGroupByArgs ga{};
    ga.rel = r.rel; ga.nparts = r.nparts;
    ga.out_keys = d_ok; ga.out_vals = d_ov; ga.out_capacity = cap_out;
    ga.cursor = &c->d_sc->total; ga.err = &c->d_sc->err;
    HIPCHK(launch_pair_lds(ga, ka, kb, nb, s));
    if (rel_close(c, r.plan, r.nparts, s, t)) return 1;
    if (c->h_sc->err & (FJ_ERR_LDS_FULL | FJ_ERR_PAIR_COLLISION))        // a partition beyond the LDS table, or two pairs on one word: the whole call on the HBM table
        return gt_fallback(t, [&](fj_timings* g) { return group_by_pair_global(c, ka, kb, nb, s, g, out_count, d_ok, d_ov, cap_out); });
    if (c->h_sc->err & FJ_ERR_OUTCAP) return set_err("internal error: group-by met a row position beyond the relation, or more distinct pairs than rows");
    *out_count = c->h_sc->total;
    return 0;
}

}  // namespace fjh

hipError_t fj_launch_pair_combine(const u64* A, const u64* B, u64* out, u64 nb, hipStream_t s) {
    if (!A || !B || !out) return hipErrorInvalidValue;
    if (!nb) return hipSuccess;
    hipLaunchKernelGGL(fj_pair_combine_kernel, dim3(fjh::gt_grid(nb)), dim3(1024), 0, s, A, B, out, nb);
    return hipGetLastError();
}
