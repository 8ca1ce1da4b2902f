// fj_groupby_rows.hip -- the ROWS of every group of one relation (an EXTENSION: FJ_ALGO_GROUP_BY | FJ_ALGO_GROUP_ROWS, include/flashjoin.h):
// the distinct keys, densely packed, and the relation's row indices in group-contiguous order with the offset at which every group
// starts - a CSR of row indices.  pandas groupby().indices, SQL array_agg, the CSR of an edge list by source; what a median, a top-k
// or any segment_reduce per group is computed from.  Without it: factorize plus a stable sort of the codes.
//
// The passes are the inverse form's (csrc/fj_groupby.hip): keys plus the rows' positions.  A final partition is a chunk list, so its
// place in the row plane has to be reserved, and the groups' order and the row ranges' order have to agree: count -> scan -> place at
// exact offsets, three launches on one stream and no host sync between them.
//   count  one workgroup per final partition: stream 1 builds the 8192-slot table of fj_group_by_inverse_kernel and writes
//          part_groups[p] (the distinct keys, the marker key included) and part_rows[p]; beyond GJ_LIMIT keys: FJ_ERR_LDS_FULL.
//   scan   two single-workgroup exclusive scans over the partitions (fj_launch_scan_u32_to_u64): group_base, row_base; the first
//          one's total is g.
//   place  returns at once behind FJ_ERR_LDS_FULL.  Stream 1 again, with an LDS add of 1 on the word behind the key's slot; ONE
//          workgroup-wide exclusive scan over the slots in slot order (8 per thread) gives every occupied slot its rank r and its
//          local start; the word becomes row_base[p] + local start, out_keys[group_base[p] + r] and out_starts[group_base[p] + r]
//          are written.  Stream 2 re-reads keys and positions, finds the slot read-only and stores the position at the place an LDS
//          atomicAdd(word, 1) hands out.  Afterwards every word equals the next group's start.
// The marker key (FJ_EMPTY_KEY after mixing) never enters the table: it is the partition's LAST group, its rows come last, its cursor
// lives in the header.  The order of the rows inside a group is the atomics': unspecified, and it may differ from run to run.
//
// HBM per row behind the passes: 8 B (count) + 8 B + 16 B (the two streams of place; L2 / MALL hits where a partition is small)
// read, 8 B written, scattered inside the group's range.
//
// Weak spot, as in fj_groupby.hip: a key that owns a large share of the rows is streamed by the one workgroup of its partition -
// three times here - and in stream 2 all its rows bump one LDS word.  Correct at any distribution (DESIGN.md "The rows of every group").
//
// Fallback: FJ_ERR_LDS_FULL; the HBM-table kernels end this file.  The count kernel sees the overflow, so the
// abandoned attempt wrote no output.
// No kernel here waits on another workgroup.
#include "fj_host.h"
#include "fj_group_dev.h"

namespace {

struct FjGroupRowsArgs {
    FjChunkSet rel;
    u32 nparts;
    u64* out_keys;               // [out_capacity] the distinct keys
    u64* out_rows;               // [nrows] row indices in group order
    u64* out_starts;             // [out_capacity] first word of out_rows of every group
    u64 out_capacity, nrows;
    u32* part_groups; u32* part_rows;            // [nparts] written by the count kernel
    const u64* group_base; const u64* row_base;  // [nparts + 1] their exclusive scans
    unsigned long long* total;   // device scalar: receives g
    u32* err;
};

// 160 B: the key slots behind it stay 16-byte aligned.  wsum: the wave totals of the workgroup-wide scan
struct GrHdr { u32 full, has_empty, nkeys, rows; u64 empty_cur, pad; u64 wsum[16]; };
static_assert(sizeof(GrHdr) == 160, "GrHdr");
constexpr u32 GR_LDS = (u32)sizeof(GrHdr) + GJ_TS * 16u;
constexpr u32 GR_SPT = GJ_TS / GJ_NT;                        // slots per thread of the scan
static_assert(GR_SPT * GJ_NT == GJ_TS && GJ_NT == 1024, "the scan takes whole threads");

__device__ __forceinline__ u64 gr_wave_incl(u64 v, u32 lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const u64 y = (u64)__shfl_up((unsigned long long)v, d, 64); if ((int)lane >= d) v += y; }
    return v;
}

// exclusive prefix of v over the 1024 threads of the workgroup, in thread order; total: the sum.  wsum: 16 LDS words, free again
// behind the call (a barrier at both ends)
__device__ __forceinline__ u64 gr_block_excl(u64 v, u64* wsum, u32 tid, u64& total) {
    const u32 lane = tid & 63, wave = tid >> 6;
    const u64 inc = gr_wave_incl(v, lane);
    __syncthreads();
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    u64 before = 0, all = 0;
#pragma unroll
    for (u32 w = 0; w < 16; ++w) { const u64 c = wsum[w]; all += c; if (w < wave) before += c; }
    total = all;
    return before + inc - v;
}

// ---- count: the table from the keys, no accumulator work.  part_groups[p], part_rows[p] ----
__global__ __launch_bounds__(GJ_NT, 1) void fj_group_rows_count_kernel(FjGroupRowsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    GrHdr* hdr = reinterpret_cast<GrHdr*>(smem);
    u64* tkeys = reinterpret_cast<u64*>(smem + sizeof(GrHdr));
    const u32 tid = threadIdx.x;
    const u32 p = blockIdx.x;
    u32 b0, nbc;
    fj_part_chunks(a.rel, p, b0, nbc);
    if (nbc == 0) { if (tid == 0) { a.part_groups[p] = 0; a.part_rows[p] = 0; } return; }

    for (u32 i = tid; i < GJ_TS; i += GJ_NT) tkeys[i] = FJ_EMPTY_KEY;
    if (tid == 0) { hdr->full = 0; hdr->has_empty = 0; hdr->nkeys = 0; hdr->rows = 0; }
    __syncthreads();

    u32 nrows = 0;
    {
        u64 k[GJ_KPT], none[1];
        u32 okm = 0;
        gb_load_round<false>(a.rel, b0, nbc, 0, tid, k, none, okm);
        for (u32 c0 = 0; c0 < nbc; c0 += GJ_ROUND_CHUNKS) {
            u64 kn[GJ_KPT];
            u32 okn = 0;
            if (c0 + GJ_ROUND_CHUNKS < nbc) gb_load_round<false>(a.rel, b0, nbc, c0 + GJ_ROUND_CHUNKS, tid, kn, none, okn);
            nrows += (u32)__popc(okm);
#pragma unroll
            for (u32 u = 0; u < GJ_KPT; ++u) {
                if (!((okm >> u) & 1u)) continue;
                const u64 key = a.rel.list ? k[u] : fj_key_mix(k[u]);                 // chunk pools hold mixed keys, flat arrays raw ones
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
    nrows = (u32)gj_wave_sum64(nrows);                       // (a partition holds fewer than 2^32 rows: csrc/fj_groupby_multi.hip)
    if ((tid & 63) == 0 && nrows) atomicAdd(&hdr->rows, nrows);
    __syncthreads();
    if (tid != 0) return;
    if (hdr->full) { atomicOr(a.err, FJ_ERR_LDS_FULL); return; }      // nothing else written: the host re-runs the call on the HBM table
    a.part_groups[p] = hdr->nkeys + (hdr->has_empty ? 1u : 0u);
    a.part_rows[p] = hdr->rows;
}

// ---- place: counts per slot, the scan in slot order, the rows at their places ----
__global__ __launch_bounds__(GJ_NT, 1) void fj_group_rows_place_kernel(FjGroupRowsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    GrHdr* hdr = reinterpret_cast<GrHdr*>(smem);
    u64* tkeys = reinterpret_cast<u64*>(smem + sizeof(GrHdr));
    u64* cur = tkeys + GJ_TS;                                // rows of the slot's key, then the next free place of its group
    const u32 tid = threadIdx.x;
    const u32 p = blockIdx.x;
    if (*a.err & FJ_ERR_LDS_FULL) return;                    // (uniform over the grid: the count launch has finished)
    if (p == 0 && tid == 0) *a.total = a.group_base[a.nparts];
    u32 b0, nbc;
    fj_part_chunks(a.rel, p, b0, nbc);
    if (nbc == 0) return;

    for (u32 i = tid; i < GJ_TS; i += GJ_NT) { tkeys[i] = FJ_EMPTY_KEY; cur[i] = 0; }
    if (tid == 0) { hdr->full = 0; hdr->has_empty = 0; hdr->nkeys = 0; hdr->rows = 0; hdr->empty_cur = 0; }
    __syncthreads();

    // ---- stream 1: the keys alone; one LDS add per row on the word behind the key's slot ----
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
                u32 pos = FJ_HW2(key) & (GJ_TS - 1);
                bool placed = false;
                for (u32 step = 0; step < GJ_TS; ++step) {
                    u64 t = tkeys[pos];
                    if (t == FJ_EMPTY_KEY) {
                        t = atomicCAS((unsigned long long*)&tkeys[pos], (unsigned long long)FJ_EMPTY_KEY, (unsigned long long)key);
                        if (t == FJ_EMPTY_KEY) t = key;
                    }
                    if (t == key) { placed = true; break; }
                    pos = (pos + 1) & (GJ_TS - 1);
                }
                if (placed) atomicAdd((unsigned long long*)&cur[pos], 1ull);
                else hdr->full = 1;                          // (the count kernel took this partition: not met)
            }
#pragma unroll
            for (u32 u = 0; u < GJ_KPT; ++u) k[u] = kn[u];
            okm = okn;
        }
    }
    __syncthreads();
    if (hdr->full) { if (tid == 0) atomicOr(a.err, FJ_ERR_OUTCAP); return; }      // (uniform: every thread reads the word behind the barrier)

    // ---- scan in slot order: occupied slots -> the group's rank, row counts -> the group's local start; both in one word (a
    // partition holds fewer than 2^32 rows and 8192 slots) ----
    const u64 gb = a.group_base[p], rb = a.row_base[p];
    const u32 s0 = tid * GR_SPT;
    u64 mine = 0;
#pragma unroll
    for (u32 j = 0; j < GR_SPT; ++j) if (tkeys[s0 + j] != FJ_EMPTY_KEY) mine += (1ull << 32) | (u64)(u32)cur[s0 + j];
    u64 all;
    u64 ex = gr_block_excl(mine, hdr->wsum, tid, all);
#pragma unroll
    for (u32 j = 0; j < GR_SPT; ++j) {
        const u64 key = tkeys[s0 + j];
        if (key == FJ_EMPTY_KEY) continue;
        const u64 cnt = (u64)(u32)cur[s0 + j];
        const u64 row = gb + (ex >> 32), start = rb + (u64)(u32)ex;
        cur[s0 + j] = start;
        if (row < a.out_capacity) { a.out_keys[row] = fj_key_unmix(key); a.out_starts[row] = start; }
        else atomicOr(a.err, FJ_ERR_OUTCAP);
        ex += (1ull << 32) | cnt;
    }
    if (tid == 0 && hdr->has_empty) {                        // the marker key: the partition's last group, its rows behind the table's
        const u64 row = gb + (all >> 32), start = rb + (u64)(u32)all;
        hdr->empty_cur = start;
        if (row < a.out_capacity) { a.out_keys[row] = fj_key_unmix(FJ_EMPTY_KEY); a.out_starts[row] = start; }
        else atomicOr(a.err, FJ_ERR_OUTCAP);
    }
    __syncthreads();

    // ---- stream 2: every row finds its key's slot in the finished table and takes the next place of its group ----
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
            u64* word = &hdr->empty_cur;
            if (key != FJ_EMPTY_KEY) {
                u32 pos = FJ_HW2(key) & (GJ_TS - 1);
                for (u32 step = 0; step < GJ_TS && tkeys[pos] != key; ++step) pos = (pos + 1) & (GJ_TS - 1);      // (stream 1 placed every key)
                word = &cur[pos];
            }
            const u64 place = (u64)atomicAdd((unsigned long long*)word, 1ull);
            if (place < a.nrows) a.out_rows[place] = pv[u];
            else atomicOr(a.err, FJ_ERR_OUTCAP);
        }
#pragma unroll
        for (u32 u = 0; u < GJ_KPT; ++u) { k[u] = kn[u]; pv[u] = pvn[u]; }
        okm = okn;
    }
}

// ---- the global-table form.  The table is fj_gt_build_first_kernel's, keys only (csrc/fj_join.hip: raw keys, the raw empty key out
// of band); cnt: capacity + 1 words, the last one the empty key's, holding every slot's row count (fj_launch_gt_group_by_combine,
// FJ_GJ_COUNT).  The capacity + 1 slots are cut into tiles of GJ_TS slots, one workgroup each, a thread taking GR_SPT neighbours:
//   sums    tile_occ[b] / tile_rows[b] = occupied slots / rows of tile b,
//   scan    one workgroup: both arrays to exclusive prefixes in place, [ntiles] = the totals (g and nb),
//   starts  the tile's own scan again on top of its bases: an occupied slot's rank r and start; out_keys[r], out_starts[r], and
//           cnt[slot] = start - the fill plane,
//   rows    thread per row: the slot of the row's key, place = atomicAdd(cnt[slot], 1), out_rows[place] = i.
// Nothing waits on another workgroup: four launches in stream order ----
__device__ __forceinline__ bool gr_gt_slot(const FjGtArgs& a, u64 i, bool has_empty, u64& key) {
    const u64 cap = a.cap_mask + 1;
    key = FJ_EMPTY_KEY;
    if (i < cap) { key = a.tkeys[i]; return key != FJ_EMPTY_KEY; }
    return i == cap && has_empty;
}

template <bool PLACE>
__global__ __launch_bounds__(GJ_NT) void fj_gt_group_rows_tile_kernel(FjGtArgs a, u64* cnt, u64* tile_occ, u64* tile_rows, u32 ntiles,
                                                                      u64* __restrict__ out_keys, u64* __restrict__ out_starts, u64 out_capacity,
                                                                      unsigned long long* total, u32* err) {
    __shared__ u64 wsum[16];
    const u32 tid = threadIdx.x;
    const bool has_empty = a.flags[0] != 0;
    const u64 s0 = (u64)blockIdx.x * GJ_TS + (u64)tid * GR_SPT;
    u64 occ = 0, rows = 0;
#pragma unroll
    for (u32 j = 0; j < GR_SPT; ++j) {
        u64 key;
        if (gr_gt_slot(a, s0 + j, has_empty, key)) { occ += 1; rows += cnt[s0 + j]; }
    }
    u64 occ_all, rows_all;
    u64 r = gr_block_excl(occ, wsum, tid, occ_all);
    u64 st = gr_block_excl(rows, wsum, tid, rows_all);
    if (!PLACE) {
        if (tid == 0) { tile_occ[blockIdx.x] = occ_all; tile_rows[blockIdx.x] = rows_all; }
        return;
    }
    if (blockIdx.x == 0 && tid == 0) *total = tile_occ[ntiles];
    r += tile_occ[blockIdx.x]; st += tile_rows[blockIdx.x];
#pragma unroll
    for (u32 j = 0; j < GR_SPT; ++j) {
        u64 key;
        if (!gr_gt_slot(a, s0 + j, has_empty, key)) continue;
        const u64 c = cnt[s0 + j];
        cnt[s0 + j] = st;
        if (r < out_capacity) { out_keys[r] = key; out_starts[r] = st; }
        else atomicOr(err, FJ_ERR_OUTCAP);
        r += 1; st += c;
    }
}

// one workgroup: occ[0 .. n) and rows[0 .. n) to their exclusive prefixes in place, occ[n] and rows[n] the totals
__global__ __launch_bounds__(GJ_NT) void fj_gt_group_rows_scan_kernel(u64* occ, u64* rows, u32 n) {
    __shared__ u64 wsum[16];
    const u32 tid = threadIdx.x;
    u64 carry_o = 0, carry_r = 0;
    for (u32 base = 0; base < n; base += GJ_NT) {            // (uniform trip count: the barriers inside are met by every thread)
        const u32 i = base + tid;
        const u64 vo = i < n ? occ[i] : 0, vr = i < n ? rows[i] : 0;
        u64 all_o, all_r;
        const u64 eo = gr_block_excl(vo, wsum, tid, all_o);
        const u64 er = gr_block_excl(vr, wsum, tid, all_r);
        if (i < n) { occ[i] = carry_o + eo; rows[i] = carry_r + er; }
        carry_o += all_o; carry_r += all_r;
    }
    if (tid == 0) { occ[n] = carry_o; rows[n] = carry_r; }
}

__global__ __launch_bounds__(1024) void fj_gt_group_rows_place_kernel(FjGtArgs a, u64* cnt, u64* __restrict__ out_rows, u64 nrows, u32* err) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < a.nb; i += stride) {
        const u64 key = a.bk[i];
        u64 where = a.cap_mask + 1;
        if (key != FJ_EMPTY_KEY && !gj_gt_find(a.tkeys, a.cap_mask, key, where)) continue;      // (the build placed every key)
        const u64 place = (u64)atomicAdd((unsigned long long*)&cnt[where], 1ull);
        if (place < nrows) out_rows[place] = i;
        else atomicOr(err, FJ_ERR_OUTCAP);
    }
}

hipError_t launch_rows_lds(const FjGroupRowsArgs& a, hipStream_t s, u64* group_base, u64* row_base) {
    if (!a.total || !a.err || !a.nparts || !a.out_keys || !a.out_rows || !a.out_starts || !a.part_groups || !a.part_rows) return hipErrorInvalidValue;
    if (a.out_capacity < a.nrows) return hipErrorInvalidValue;                                       // (every row may be a group of its own)
    if (!a.rel.list ? a.rel.n_flat > a.nrows : !a.rel.vals) return hipErrorInvalidValue;              // (a chunk pool without positions has no row indices)
    hipError_t e = fj_set_max_lds_once(reinterpret_cast<const void*>(fj_group_rows_count_kernel), GR_LDS);
    if (e != hipSuccess) return e;
    e = fj_set_max_lds_once(reinterpret_cast<const void*>(fj_group_rows_place_kernel), GR_LDS);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fj_group_rows_count_kernel, dim3(a.nparts), dim3(GJ_NT), GR_LDS, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = fj_launch_scan_u32_to_u64(a.part_groups, group_base, a.nparts, s)) != hipSuccess) return e;
    if ((e = fj_launch_scan_u32_to_u64(a.part_rows, row_base, a.nparts, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(fj_group_rows_place_kernel, dim3(a.nparts), dim3(GJ_NT), GR_LDS, s, a);
    return hipGetLastError();
}

}  // namespace

namespace fjh {

static int rows_outcap_error() {
    return set_err("internal error: FJ_ALGO_GROUP_ROWS met a place beyond the relation's rows, or more distinct keys than rows");
}

// the global-table form (fj_host.h): a count per slot, scanned per tile of GJ_TS slots.  It defines all nb row words, all g keys and
// all g starts itself
static int group_rows_global(fj_ctx* c, const u64* bk, size_t nb, hipStream_t s, fj_timings* t, u64* out_count,
                             u64* d_ok, u64* d_rows, u64* d_starts, size_t cap_out) {
    const u64 cap = gt_capacity(nb);
    const u64 ntiles64 = (cap + 1 + GJ_TS - 1) / GJ_TS;
    if (ntiles64 > 0x7FFFFFFFull) return set_err("fj_join_device: FJ_ALGO_GROUP_ROWS on the HBM table takes fewer than 2^43 rows, got %zu", nb);
    const u32 ntiles = (u32)ntiles64;
    void* p;
    if (get_buf(c, W_GR_BASE, 2 * ((size_t)ntiles + 1) * 8, &p)) return 1;
    u64* tile_occ = (u64*)p; u64* tile_rows = tile_occ + ntiles + 1;
    FjGtArgs a{};
    u64* cnt = nullptr;
    if (gt_open(c, nb, ntiles64 * GJ_TS, s, &a, &cnt)) return 1;                 // (whole tiles: the slots behind capacity + 1 are never read)
    a.bk = bk;
    HIPCHK(fj_launch_gt_build_first(a, false, s));
    HIPCHK(fj_launch_group_fill(cnt, cap + 1, FJ_GJ_COUNT, s));
    HIPCHK(fj_launch_gt_group_by_combine(a, FJ_GJ_COUNT, nullptr, cnt, s));
    HIPCHK(hipEventRecord(c->ev[E_BUILD], s));
    HIPCHK(hipEventRecord(c->ev[E_PPART], s));
    hipLaunchKernelGGL(fj_gt_group_rows_tile_kernel<false>, dim3(ntiles), dim3(GJ_NT), 0, s, a, cnt, tile_occ, tile_rows, ntiles,
                       (u64*)nullptr, (u64*)nullptr, (u64)0, (unsigned long long*)nullptr, (u32*)nullptr);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(fj_gt_group_rows_scan_kernel, dim3(1), dim3(GJ_NT), 0, s, tile_occ, tile_rows, ntiles);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(fj_gt_group_rows_tile_kernel<true>, dim3(ntiles), dim3(GJ_NT), 0, s, a, cnt, tile_occ, tile_rows, ntiles,
                       d_ok, d_starts, (u64)cap_out, &c->d_sc->total, &c->d_sc->err);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(fj_gt_group_rows_place_kernel, dim3(gt_grid(nb)), dim3(1024), 0, s, a, cnt, d_rows, (u64)nb, &c->d_sc->err);
    HIPCHK(hipGetLastError());
    if (gt_close(c, s, t)) return 1;
    if (c->h_sc->err & FJ_ERR_OUTCAP) return rows_outcap_error();
    *out_count = c->h_sc->total;
    return 0;
}

// FJ_ALGO_GROUP_BY | FJ_ALGO_GROUP_ROWS (fj_join_device has checked the arguments): the g distinct keys of bk[0 .. nb) in d_ok, the nb
// row indices in group order in d_ov[0 .. nb) and every group's first word of them in d_ov[cap_out .. cap_out + g); g <= nb <= cap_out.
// use_radix: the partitioned plan, else the global table
int group_rows(fj_ctx* c, bool use_radix, const u64* bk, size_t nb, int top_bits, hipStream_t s, fj_timings* t,
               u64* out_count, u64* d_ok, u64* d_ov, size_t cap_out) {
    *out_count = 0;
    if (nb == 0) return 0;
    u64* d_rows = d_ov; u64* d_starts = d_ov + cap_out;
    if (!use_radix) return group_rows_global(c, bk, nb, s, t, out_count, d_ok, d_rows, d_starts, cap_out);

    RelAttempt r;                                            // factorize's plan: the table is its 8192 slots; the rows' positions travel
    if (rel_open(c, bk, REL_POSITIONS, nullptr, nb, top_bits, 0, s, &r)) return 1;
    FjGroupRowsArgs ga{};
    ga.rel = r.rel; ga.nparts = r.nparts;
    void* p;
    if (get_buf(c, W_GR_PART, 2 * (size_t)ga.nparts * 4, &p)) return 1;
    ga.part_groups = (u32*)p; ga.part_rows = ga.part_groups + ga.nparts;
    if (get_buf(c, W_GR_BASE, 2 * ((size_t)ga.nparts + 1) * 8, &p)) return 1;
    u64* group_base = (u64*)p; u64* row_base = group_base + ga.nparts + 1;
    ga.group_base = group_base; ga.row_base = row_base;
    ga.out_keys = d_ok; ga.out_rows = d_rows; ga.out_starts = d_starts; ga.out_capacity = cap_out; ga.nrows = nb;
    ga.total = &c->d_sc->total; ga.err = &c->d_sc->err;
    HIPCHK(launch_rows_lds(ga, s, group_base, row_base));
    if (rel_close(c, r.plan, r.nparts, s, t)) return 1;
    if (c->h_sc->err & FJ_ERR_LDS_FULL)                      // a partition beyond the LDS table: the whole call on the HBM table
        return gt_fallback(t, [&](fj_timings* g) { return group_rows_global(c, bk, nb, s, g, out_count, d_ok, d_rows, d_starts, cap_out); });
    if (c->h_sc->err & FJ_ERR_OUTCAP) return rows_outcap_error();
    *out_count = c->h_sc->total;
    return 0;
}

}  // namespace fjh
