// fj_many.hip -- many-to-many equi-join on the partitioned plan (an EXTENSION: SURVEY 8(f) rank 4).
//
// The reference deduplicates build keys at insert (hash_join.cpp:125, :147) and stops a probe at the first match
// (:172-176): an N:1 join.  inner_join / inner_join_count keep every build row: a probe row yields one output pair per
// build row with its key (SQL inner join semantics), count = sum over probe rows of the key's multiplicity.
//
// Same partitioning and work items as the other joins; per final partition (<= 4096 build ROWS, the plan aims at 2048)
// one 1024-thread workgroup keeps in LDS
//   tkeys[8192]  distinct keys, linear probing, slot claimed by a 64-bit compare-and-swap (find-or-insert is exact:
//                no racing copies of one key),
//   head[8192]   first build row of the key's chain,   rnext[4096]  next row of the chain,   rvals[4096]  the rows' values;
// a probe walks its key's chain: counting adds the chain's length, materialising writes (probe key, value) per link at a
// position from a wave-wide exclusive scan + one LDS cursor bump per wave.  Two passes like the other materialising
// joins (count per item -> scan -> emit at exact offsets).  Written for correctness and reasonable speed, not tuned like
// the N:1 kernels (64-bit LDS CAS inserts, one key per lane and step).
//
// Outer forms (FJ_ALGO_ALL_COPIES with FJ_ALGO_LEFT_OUTER / FJ_ALGO_FULL_OUTER; template parameter OUTER): the same table and chains;
// a probe row without a chain is a MISS.  The counting pass keeps a second count per item (misses), the emitting pass writes a miss
// as (probe key, 0) at P + miss_off[item] + its rank in the item (ballot + popcount, one LDS cursor bump per wave).  FULL, counting
// pass only: the item remembers which table slots its probe rows hit (one bit per slot in LDS behind rnext, one more word for the
// empty-marker key's head), then walks its partition's build chunks once more and ORs the rows of hit slots into the per-build-row
// bitmap in HBM - one 64-bit atomic per non-zero ballot of 64 rows, the scheme of fj_outer_join_kernel<.., FULL>; the bits an atomic
// newly set are counted, so the launch also yields r = nb - marked rows.  fj_full_sweep_kernel appends the unmarked rows.
//
// Partitions of more than 4096 build rows (option "mm_heavy_keys" = 1 for the inner form, "mm_heavy_outer" = 1 for the outer forms;
// more radix bits cannot split the copies of one key): the counting launch marks such an item FJ_ITEM_TOOBIG instead of raising FJ_ERR_LDS_FULL, the host cuts it into
// (probe item, build tile) work items - a tile = MT_CHUNKS consecutive chunks of the partition's build chunk list, at most 4096
// rows - and fj_mm_tile_kernel joins each of them.  Every pair is found exactly once, in the tile that holds its build row: counts
// add, outputs concatenate, no state crosses tiles.  A heavy key means few probe rows with thousands of partners each, so the tile
// kernel does not walk chains: a counting sort by table slot (count, scan, place) turns a key's rows into one contiguous run of
// values, a hit is (start, length), and the WORKGROUP writes a round's concatenated runs - thread j of a stride-1024 loop finds
// its hit by binary search over the scanned lengths - so that consecutive lanes write consecutive output rows of both planes.
// Outer forms over tiles (fj_mm_tile_kernel<false, false, FJ_MM_LEFT / FJ_MM_FULL>, counting pass only - the pairs are the inner form's,
// counted and emitted as above): a probe row's "no partner" is a verdict over ALL tiles of its partition, so a tile records the
// opposite - per round one ballot of "found a partner here" and one 64-bit atomicOr by lane 0 into a bitmap over the probe side's
// final chunk pool (a wave covers 64 consecutive rows of one probe chunk).  fj_mm_miss_sweep_kernel, one workgroup per oversized
// probe item, then counts (and, emitting, writes) the item's rows whose bit stayed zero.  FULL: the tile remembers the table slots
// its probe rows hit (one bit per slot, one word for the empty marker's slot MM_S, behind soff) and walks its chunks once more to
// OR the rows of hit slots into the per-build-row bitmap, counting the newly set bits - fj_mm_join_kernel<.., FULL>'s scheme on
// the tile; the tiles of a partition hold disjoint rows, so r = nb - marked holds as before.
#include "fj_lds_table_dev.h"

namespace {

constexpr u32 MM_S = 8192, MM_ROWS = 4096, MM_NT = 1024, MM_NONE = 0xFFFFFFFFu;
constexpr u32 MM_SBITS_WORDS = MM_S / 32 + 4;               // FULL: hit bits of the slots + the empty marker's word (16-byte multiple)
struct MmHdr { u32 nrows, full, empty_head, cursor; unsigned long long cnt; u32 miss, marked; };   // miss: the item's misses (counting) / its miss cursor (emitting)

// RID (MAT only): the row-id form (FjLdsJoinArgs::row_ids) - build values are row positions, and the probe row's position
// (its vals plane; flat arrays: the index) takes the key's place
// OUTER: FJ_MM_INNER, FJ_MM_LEFT or FJ_MM_FULL (fj_internal.h).  The emitting pass of FULL is LEFT's: the marking belongs to the counting pass
template <bool MAT, bool RID = false, int OUTER = FJ_MM_INNER>
__global__ __launch_bounds__(MM_NT, 1) void fj_mm_join_kernel(FjLdsJoinArgs a, FjMmOuterArgs oa) {
    static_assert(!(MAT && OUTER == FJ_MM_FULL), "the build rows are marked by the counting pass");
    constexpr bool FULL = OUTER == FJ_MM_FULL;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    MmHdr* hdr = reinterpret_cast<MmHdr*>(smem);
    u64* tkeys = reinterpret_cast<u64*>(smem + sizeof(MmHdr));
    u64* rvals = tkeys + MM_S;
    u32* head = reinterpret_cast<u32*>(rvals + MM_ROWS);
    u32* rnext = head + MM_S;
    u32* sbits = rnext + MM_ROWS;                              // (FULL only) [MM_S / 32] hit slots, [MM_S / 32] != 0: the empty marker key was hit
    const u32 tid = threadIdx.x, lane = tid & 63;
    const u32 item = blockIdx.x;
    u32 p, b0, nbc, s_lo, s_hi;
    if (!fj_item_slice(a.items, a.nitems_dev, a.nsplit, a.probe.n_flat, item, p, s_lo, s_hi)) return;
    fj_part_chunks(a.build, p, b0, nbc);
    // (OUTER: a partition without build rows still has its probe rows to report - the build loop below runs zero times)
    if ((!OUTER && nbc == 0) || s_lo >= s_hi) { if (!MAT && tid == 0) { a.part_count[item] = 0; if (OUTER) oa.miss_count[item] = 0; } return; }
    if (MAT && a.part_count[item] == 0 && (!OUTER || oa.miss_count[item] == 0)) return;

    for (u32 i = tid; i < MM_S; i += MM_NT) { tkeys[i] = FJ_EMPTY_KEY; head[i] = MM_NONE; }
    if (FULL) for (u32 i = tid; i < MM_SBITS_WORDS; i += MM_NT) sbits[i] = 0;
    if (tid == 0) { hdr->nrows = 0; hdr->full = 0; hdr->empty_head = MM_NONE; hdr->cursor = 0; hdr->cnt = 0; hdr->miss = 0; hdr->marked = 0; }
    __syncthreads();

    // ---- build: every row is kept; a key's rows form a chain ----
    for (u32 c0 = 0; c0 < nbc; c0 += MM_NT / FJ_CHUNK) {
        const u32 c = c0 + tid / FJ_CHUNK, off = tid % FJ_CHUNK;
        if (c < nbc) {
            const u32 e = fj_chunk_entry(a.build, b0 + c);
            if (off < FJ_LIST_CNT(e)) {
                const u64 src = (u64)FJ_LIST_ID(e) * FJ_CHUNK + off;
                const u64 key = a.build.list ? a.build.keys[src] : fj_key_mix(a.build.keys[src]);     // chunk pools hold mixed keys, flat arrays raw ones (fj_common.h)
                const u32 r = atomicAdd(&hdr->nrows, 1u);
                if (r >= MM_ROWS) hdr->full = 1;
                else {
                    if (MAT) rvals[r] = (RID && !a.build.vals) ? src : a.build.vals[src];
                    u32* h;
                    if (key == FJ_EMPTY_KEY) h = &hdr->empty_head;        // the empty marker is never stored in the table
                    else {
                        u32 pos = FJ_HW2(key) & (MM_S - 1);
                        for (;;) {                                          // <= 4096 distinct keys in 8192 slots: always terminates
                            const u64 old = atomicCAS((unsigned long long*)&tkeys[pos], (unsigned long long)FJ_EMPTY_KEY, (unsigned long long)key);
                            if (old == FJ_EMPTY_KEY || old == key) break;
                            pos = (pos + 1) & (MM_S - 1);
                        }
                        h = &head[pos];
                    }
                    rnext[r] = atomicExch(h, r);
                }
            }
        }
    }
    __syncthreads();
    if (hdr->full) {                                   // more rows than the LDS tables hold: the host reports it (no fallback for this extension) ...
        if (!MAT && a.mark_toobig) {                   // ... or - options "mm_heavy_keys" / "mm_heavy_outer" - joins the item tile by tile (fj_mm_tile_kernel)
            if (tid == 0) { a.part_count[item] = FJ_ITEM_TOOBIG; if (OUTER) oa.miss_count[item] = 0; atomicOr(a.err, FJ_STAT_TOOBIG); }
            return;
        }
        if (tid == 0) { atomicOr(a.err, FJ_ERR_LDS_FULL); if (!MAT) { a.part_count[item] = 0; if (OUTER) oa.miss_count[item] = 0; } }
        return;
    }

    // ---- probe: one key per lane and step ----
    const u64 obase = MAT ? a.out_off[item] : 0;
    const u64 mbase = (MAT && OUTER) ? oa.miss_base + oa.miss_off[item] : 0;
    unsigned long long local = 0;
    u32 lmiss = 0;
    for (u32 pc = s_lo; pc < s_hi; pc += MM_NT / FJ_CHUNK) {
        const u32 c = pc + tid / FJ_CHUNK, off = tid % FJ_CHUNK;
        u64 key = 0, psrc = 0; bool ok = false;
        if (c < s_hi) {
            const u32 e = fj_chunk_entry(a.probe, c);
            psrc = (u64)FJ_LIST_ID(e) * FJ_CHUNK + off;
            if (off < FJ_LIST_CNT(e)) { key = a.probe.keys[psrc]; if (!a.probe.list) key = fj_key_mix(key); ok = true; }
        }
        u32 h = MM_NONE;
        if (ok) {
            if (key == FJ_EMPTY_KEY) h = hdr->empty_head;
            else {
                u32 pos = FJ_HW2(key) & (MM_S - 1);
                for (;;) {
                    const u64 t = tkeys[pos];
                    if (t == key) {
                        h = head[pos];
                        // (read first: most hits find their slot's bit set already and skip the LDS atomic)
                        if (FULL && !((sbits[pos >> 5] >> (pos & 31)) & 1u)) atomicOr(&sbits[pos >> 5], 1u << (pos & 31));
                        break;
                    }
                    if (t == FJ_EMPTY_KEY) break;
                    pos = (pos + 1) & (MM_S - 1);
                }
            }
        }
        if (FULL && ok && key == FJ_EMPTY_KEY && h != MM_NONE) sbits[MM_S / 32] = 1;
        const bool miss = OUTER && ok && h == MM_NONE;
        u32 cnt = 0;
        for (u32 r = h; r != MM_NONE; r = rnext[r]) ++cnt;
        if (!MAT) { local += cnt; lmiss += miss ? 1u : 0u; continue; }
        if (OUTER) {                                       // misses: (probe key, 0) behind the pairs; row ids: (probe position, ~0)
            const u64 mbal = __ballot(miss);
            if (mbal) {
                u32 wm = 0;
                if (lane == 0) wm = atomicAdd(&hdr->miss, (u32)__popcll(mbal));
                wm = __shfl(wm, 0, 64);
                if (miss) {
                    const u64 o = mbase + wm + (u32)__popcll(mbal & ((1ull << lane) - 1ull));
                    a.out_keys[o] = RID ? (a.probe.vals ? a.probe.vals[psrc] : psrc) : fj_key_unmix(key);
                    a.out_vals[o] = RID ? ~0ull : 0ull;
                }
            }
        }
        // exclusive scan of cnt over the wave, one LDS cursor bump per wave
        u32 inc = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const u32 y = __shfl_up(inc, d, 64); if ((int)lane >= d) inc += y; }
        const u32 wave_total = __shfl(inc, 63, 64);
        u32 wb = 0;
        if (wave_total) {
            if (lane == 63) wb = atomicAdd(&hdr->cursor, wave_total);
            wb = __shfl(wb, 63, 64);
            u64 o = obase + wb + (inc - cnt);
            const u64 raw = RID ? ((h != MM_NONE && a.probe.vals) ? a.probe.vals[psrc] : psrc) : fj_key_unmix(key);     // (read by the lanes that write)
            for (u32 r = h; r != MM_NONE; r = rnext[r]) { a.out_keys[o] = raw; a.out_vals[o] = rvals[r]; ++o; }
        }
    }
    if (!MAT) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) local += __shfl_xor(local, d, 64);
        if (lane == 0 && local) atomicAdd(&hdr->cnt, local);
        if (OUTER) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) lmiss += __shfl_xor(lmiss, d, 64);
            if (lane == 0 && lmiss) atomicAdd(&hdr->miss, lmiss);
        }
        __syncthreads();
        if (tid == 0) {
            const unsigned long long n = hdr->cnt;
            if (n > 0xFFFFFFFFull) atomicOr(a.err, FJ_ERR_POOL);       // (cannot happen: <= 131072 probe rows x 4096 build rows per item)
            a.part_count[item] = (u32)n;
            if (n) atomicAdd(a.total, n);
            if (OUTER) {
                const u32 m = hdr->miss;
                oa.miss_count[item] = m;
                if (m) atomicAdd(oa.miss_total, (unsigned long long)m);
            }
        }
        if (FULL) {
            // ---- the build rows this item's probe rows found (the slot bits are complete: the barrier above); uniform control
            // flow up to the ballot (c is wave-uniform: a wave covers 64 consecutive rows of one chunk) ----
            static_assert(FJ_CHUNK % 64 == 0, "a wave covers 64 consecutive rows of one chunk");
            const bool empty_hit = sbits[MM_S / 32] != 0;
            u32 newly = 0;                                 // (lane 0) bits this wave's atomics turned on
            for (u32 c0 = 0; c0 < nbc; c0 += MM_NT / FJ_CHUNK) {
                const u32 c = c0 + tid / FJ_CHUNK, off = tid % FJ_CHUNK;
                bool mt = false;
                u64 src = 0;
                if (c < nbc) {
                    const u32 e = fj_chunk_entry(a.build, b0 + c);
                    src = (u64)FJ_LIST_ID(e) * FJ_CHUNK + off;
                    if (off < FJ_LIST_CNT(e)) {
                        const u64 key = a.build.list ? a.build.keys[src] : fj_key_mix(a.build.keys[src]);
                        if (key == FJ_EMPTY_KEY) mt = empty_hit;
                        else {
                            u32 pos = FJ_HW2(key) & (MM_S - 1);
                            for (;;) {                       // (the key is in the table: the build put it there)
                                const u64 t = tkeys[pos];
                                if (t == key) { mt = (sbits[pos >> 5] >> (pos & 31)) & 1u; break; }
                                if (t == FJ_EMPTY_KEY) break;
                                pos = (pos + 1) & (MM_S - 1);
                            }
                        }
                    }
                }
                const u64 bal = __ballot(mt);
                if (lane == 0 && bal) {                      // another item of the partition may have set some of them already
                    const u64 old = atomicOr((unsigned long long*)&oa.bits[src >> 6], (unsigned long long)bal);
                    newly += (u32)__popcll(bal & ~old);
                }
            }
            if (lane == 0 && newly) atomicAdd(&hdr->marked, newly);
            __syncthreads();
            if (tid == 0 && hdr->marked) atomicAdd(oa.marked, (unsigned long long)hdr->marked);
        }
    }
}

// ---- one (probe item, build tile) work item of an oversized partition: items[] = {first probe list index, probe chunks, partition,
// first build chunk of the tile (relative to the partition's list)}; the grid is exactly items_cap workgroups ----
constexpr u32 MT_CHUNKS = FJ_MM_TILE_CHUNKS;                  // build chunks per tile: whatever their fill, never more than MM_ROWS rows
constexpr u32 MT_NOSLOT = 0xFFFFFFFFu;
struct MtHdr { u32 wsum[MM_NT / 64]; unsigned long long cnt; u32 marked, pad_; };     // marked: (FULL) build rows whose bit this work item turned on
// LDS: header, tkeys[MM_S], soff[MM_S + 4] (per slot: row count, then start, then - after the placing - end of the slot's run; entry
// MM_S is the empty marker key's, which never enters the table), and for the emitting form rvals[MM_ROWS] (the values, run by run)
// and a round's hits: hraw[MM_NT] (probe key / position), hsc[MM_NT] (inclusive scan of the lengths), hpk[MM_NT] (start | length << 16);
// the counting form of FULL keeps sbits[MM_SBITS_WORDS] behind soff instead: bit `slot` = a probe row of this work item hit the slot
// (slot MM_S, the empty marker's, is bit 0 of word MM_S / 32)
constexpr u32 MT_LDS_COUNT = sizeof(MtHdr) + MM_S * 8 + (MM_S + 4) * 4;
constexpr u32 MT_LDS_MAT = MT_LDS_COUNT + MM_ROWS * 8 + MM_NT * 8 + MM_NT * 4 + MM_NT * 4;
static_assert(sizeof(MtHdr) % 16 == 0 && MT_LDS_COUNT % 16 == 0, "every carve offset is a multiple of 16 bytes");
static_assert(MT_LDS_MAT <= 160 * 1024, "one workgroup's LDS on a CU");
static_assert(MT_CHUNKS * FJ_CHUNK <= MM_ROWS && MM_S == 8 * MM_NT && MM_ROWS <= 0xFFFF, "the slot scan takes 8 slots per thread; start and length share a word");

// inclusive scan of v over the workgroup, *total = the sum; one barrier inside, and the caller keeps another one between two calls
__device__ __forceinline__ u32 mt_block_scan(u32 v, u32* wsum, u32 tid, u32 lane, u32* total) {
    u32 inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const u32 y = __shfl_up(inc, d, 64); if ((int)lane >= d) inc += y; }
    if (lane == 63) wsum[tid >> 6] = inc;
    __syncthreads();
    u32 before = 0, tot = 0;
#pragma unroll
    for (u32 w = 0; w < MM_NT / 64; ++w) { const u32 x = wsum[w]; tot += x; if (w < (tid >> 6)) before += x; }
    *total = tot;
    return inc + before;
}

// OUTER: FJ_MM_INNER, or - counting pass only - FJ_MM_LEFT / FJ_MM_FULL (oa.pbits; FULL: oa.bits, oa.marked)
template <bool MAT, bool RID = false, int OUTER = FJ_MM_INNER>
__global__ __launch_bounds__(MM_NT, 1) void fj_mm_tile_kernel(FjLdsJoinArgs a, FjMmOuterArgs oa) {
    static_assert(!(MAT && OUTER != FJ_MM_INNER), "the verdicts and the marks belong to the counting pass; the inner form emits the pairs");
    constexpr bool FULL = OUTER == FJ_MM_FULL;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    MtHdr* hdr = reinterpret_cast<MtHdr*>(smem);
    u64* tkeys = reinterpret_cast<u64*>(smem + sizeof(MtHdr));
    u32* soff = reinterpret_cast<u32*>(tkeys + MM_S);
    u64* rvals = reinterpret_cast<u64*>(soff + MM_S + 4);      // (MAT only, and what follows)
    u32* sbits = soff + MM_S + 4;                              // (FULL only, in rvals' place)
    u64* hraw = rvals + MM_ROWS;
    u32* hsc = reinterpret_cast<u32*>(hraw + MM_NT);
    u32* hpk = hsc + MM_NT;
    const u32 tid = threadIdx.x, lane = tid & 63;
    const u32 item = blockIdx.x;
    const uint4 it = a.items[item];
    const u32 p = it.z, s_lo = it.x, s_hi = it.x + it.y;
    const u32 b0 = a.build.boff[p], nbc = a.build.boff[p + 1] - b0;
    const u32 c_lo = it.w, c_hi = nbc - c_lo < MT_CHUNKS ? nbc : c_lo + MT_CHUNKS;
    if (c_lo >= nbc || s_lo >= s_hi) { if (!MAT && tid == 0) a.part_count[item] = 0; return; }
    if (MAT && a.part_count[item] == 0) return;

    for (u32 i = tid; i < MM_S; i += MM_NT) { tkeys[i] = FJ_EMPTY_KEY; soff[i] = 0; }
    if (tid < 4) soff[MM_S + tid] = 0;
    if (FULL) for (u32 i = tid; i < MM_SBITS_WORDS; i += MM_NT) sbits[i] = 0;
    if (tid == 0) { hdr->cnt = 0; if (FULL) hdr->marked = 0; }
    __syncthreads();

    // ---- build, first sweep over the tile: find-or-insert the key, count the slot's rows ----
    for (u32 cl0 = 0; cl0 < MT_CHUNKS; cl0 += MM_NT / FJ_CHUNK) {
        const u32 c = c_lo + cl0 + tid / FJ_CHUNK, off = tid % FJ_CHUNK;
        if (c < c_hi) {
            const u32 e = a.build.list[b0 + c];
            if (off < FJ_LIST_CNT(e)) {
                const u64 key = a.build.keys[(u64)FJ_LIST_ID(e) * FJ_CHUNK + off];      // (chunk pools hold mixed keys)
                u32 slot = MM_S;
                if (key != FJ_EMPTY_KEY) {
                    u32 pos = FJ_HW2(key) & (MM_S - 1);
                    for (;;) {                                      // <= 4096 distinct keys in 8192 slots: always terminates
                        const u64 old = atomicCAS((unsigned long long*)&tkeys[pos], (unsigned long long)FJ_EMPTY_KEY, (unsigned long long)key);
                        if (old == FJ_EMPTY_KEY || old == key) break;
                        pos = (pos + 1) & (MM_S - 1);
                    }
                    slot = pos;
                }
                atomicAdd(&soff[slot], 1u);
            }
        }
    }
    __syncthreads();

    if (MAT) {
        // ---- counts -> starts (8 slots per thread; the empty marker's run comes last) ----
        uint4* so4 = reinterpret_cast<uint4*>(soff);
        uint4 x0 = so4[2 * tid], x1 = so4[2 * tid + 1];
        const u32 sum = x0.x + x0.y + x0.z + x0.w + x1.x + x1.y + x1.z + x1.w;
        u32 total;
        u32 run = mt_block_scan(sum, hdr->wsum, tid, lane, &total) - sum;
        u32 t;
        t = x0.x; x0.x = run; run += t;  t = x0.y; x0.y = run; run += t;  t = x0.z; x0.z = run; run += t;  t = x0.w; x0.w = run; run += t;
        t = x1.x; x1.x = run; run += t;  t = x1.y; x1.y = run; run += t;  t = x1.z; x1.z = run; run += t;  t = x1.w; x1.w = run; run += t;
        so4[2 * tid] = x0; so4[2 * tid + 1] = x1;
        if (tid == MM_NT - 1) soff[MM_S] = total;
        __syncthreads();
        // ---- second sweep: every row's value goes to the next free place of its slot's run; afterwards soff[slot] is the END of the
        // run and the end of the slot before it (0 for slot 0) its start ----
        for (u32 cl0 = 0; cl0 < MT_CHUNKS; cl0 += MM_NT / FJ_CHUNK) {
            const u32 c = c_lo + cl0 + tid / FJ_CHUNK, off = tid % FJ_CHUNK;
            if (c < c_hi) {
                const u32 e = a.build.list[b0 + c];
                if (off < FJ_LIST_CNT(e)) {
                    const u64 src = (u64)FJ_LIST_ID(e) * FJ_CHUNK + off;
                    const u64 key = a.build.keys[src];
                    u32 slot = MM_S;
                    if (key != FJ_EMPTY_KEY) {
                        u32 pos = FJ_HW2(key) & (MM_S - 1);
                        while (tkeys[pos] != key) pos = (pos + 1) & (MM_S - 1);       // (the first sweep put it there)
                        slot = pos;
                    }
                    const u32 dst = atomicAdd(&soff[slot], 1u);
                    if (dst < MM_ROWS) rvals[dst] = a.build.vals[src];                // (always: a tile holds <= MM_ROWS rows)
                }
            }
        }
        __syncthreads();
    }

    // ---- probe: one key per thread and round ----
    const u64 obase = MAT ? a.out_off[item] : 0;
    unsigned long long local = 0;
    u32 written = 0;                                           // (MAT) pairs of the earlier rounds
    for (u32 pc = s_lo; pc < s_hi; pc += MM_NT / FJ_CHUNK) {
        const u32 c = pc + tid / FJ_CHUNK, off = tid % FJ_CHUNK;
        u64 key = 0, psrc = 0; bool ok = false;
        if (c < s_hi) {
            const u32 e = a.probe.list[c];
            psrc = (u64)FJ_LIST_ID(e) * FJ_CHUNK + off;
            if (off < FJ_LIST_CNT(e)) { key = a.probe.keys[psrc]; ok = true; }
        }
        u32 slot = MT_NOSLOT;
        if (ok) {
            if (key == FJ_EMPTY_KEY) slot = MM_S;
            else {
                u32 pos = FJ_HW2(key) & (MM_S - 1);
                for (;;) {
                    const u64 t = tkeys[pos];
                    if (t == key) { slot = pos; break; }
                    if (t == FJ_EMPTY_KEY) break;
                    pos = (pos + 1) & (MM_S - 1);
                }
            }
        }
        if (!MAT && OUTER) {
            // ---- the row's partners in this tile, and the verdict "found some" for the wave's 64 consecutive rows of probe chunk c
            // (c is wave-uniform, lane 0's psrc is the first of them; a wave beyond the item's chunks has no ok lane) ----
            static_assert(FJ_CHUNK % 64 == 0, "a wave covers 64 consecutive rows of one chunk");
            const u32 n = slot != MT_NOSLOT ? soff[slot] : 0u;     // (the empty marker's slot MM_S is in every tile's table: 0 rows = no partner here)
            local += n;
            // (read first: most hits find their slot's bit set already and skip the LDS atomic)
            if (FULL && n && !((sbits[slot >> 5] >> (slot & 31)) & 1u)) atomicOr(&sbits[slot >> 5], 1u << (slot & 31));
            const u64 bal = __ballot(n != 0);
            if (lane == 0 && bal) atomicOr((unsigned long long*)&oa.pbits[psrc >> 6], (unsigned long long)bal);
            continue;
        }
        if (!MAT) { if (slot != MT_NOSLOT) local += soff[slot]; continue; }
        u32 start = 0, len = 0;
        if (slot != MT_NOSLOT) { start = slot ? soff[slot - 1] : 0u; len = soff[slot] - start; }
        // ---- the round's hits as (start, length) beside the scanned lengths; then the workgroup writes the concatenated runs:
        // output row j of the round belongs to the first hit whose inclusive scan exceeds j ----
        u32 round_total;
        const u32 incl = mt_block_scan(len, hdr->wsum, tid, lane, &round_total);
        hsc[tid] = incl; hpk[tid] = start | (len << 16);
        if (len) hraw[tid] = RID ? (a.probe.vals ? a.probe.vals[psrc] : psrc) : fj_key_unmix(key);
        __syncthreads();
        for (u32 j = tid; j < round_total; j += MM_NT) {
            u32 lo = 0;
#pragma unroll
            for (u32 w = MM_NT / 2; w; w >>= 1) if (hsc[lo + w - 1] <= j) lo += w;      // lo = hits whose scan is <= j (< MM_NT: the last scan is round_total > j)
            const u32 pk2 = hpk[lo];
            const u32 k = j - (hsc[lo] - (pk2 >> 16));
            const u64 o = obase + written + j;
            a.out_keys[o] = hraw[lo];
            a.out_vals[o] = rvals[(pk2 & 0xFFFFu) + k];
        }
        written += round_total;
        __syncthreads();
    }
    if (!MAT) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) local += __shfl_xor(local, d, 64);
        if (lane == 0 && local) atomicAdd(&hdr->cnt, local);
        __syncthreads();
        if (tid == 0) {
            const unsigned long long n = hdr->cnt;
            if (n > 0xFFFFFFFFull) atomicOr(a.err, FJ_ERR_POOL);       // (cannot happen: <= 131072 probe rows x 4096 build rows per (item, tile))
            a.part_count[item] = (u32)n;
            if (n) atomicAdd(a.total, n);
        }
        if (FULL) {
            // ---- the tile's build rows that this work item's probe rows found (the slot bits are complete: the barrier above);
            // uniform control flow up to the ballot, one 64-bit atomic per non-zero ballot of 64 rows of one chunk ----
            u32 newly = 0;                                 // (lane 0) bits this wave's atomics turned on
            for (u32 cl0 = 0; cl0 < MT_CHUNKS; cl0 += MM_NT / FJ_CHUNK) {
                const u32 c = c_lo + cl0 + tid / FJ_CHUNK, off = tid % FJ_CHUNK;
                bool mt = false;
                u64 src = 0;
                if (c < c_hi) {
                    const u32 e = a.build.list[b0 + c];
                    src = (u64)FJ_LIST_ID(e) * FJ_CHUNK + off;
                    if (off < FJ_LIST_CNT(e)) {
                        const u64 key = a.build.keys[src];
                        u32 slot = MM_S;
                        if (key != FJ_EMPTY_KEY) {
                            u32 pos = FJ_HW2(key) & (MM_S - 1);
                            while (tkeys[pos] != key) pos = (pos + 1) & (MM_S - 1);       // (the first sweep put it there)
                            slot = pos;
                        }
                        mt = (sbits[slot >> 5] >> (slot & 31)) & 1u;
                    }
                }
                const u64 bal = __ballot(mt);
                if (lane == 0 && bal) {                      // another probe item of the partition may have set some of them already
                    const u64 old = atomicOr((unsigned long long*)&oa.bits[src >> 6], (unsigned long long)bal);
                    newly += (u32)__popcll(bal & ~old);
                }
            }
            if (lane == 0 && newly) atomicAdd(&hdr->marked, newly);
            __syncthreads();
            if (tid == 0 && hdr->marked) atomicAdd(oa.marked, (unsigned long long)hdr->marked);
        }
    }
}

// ---- the "no partner" verdicts of the oversized probe items, read off the bitmap the tiles' counting pass filled: one workgroup per
// item (w.items holds only the items marked FJ_ITEM_TOOBIG).  Counting: the item's rows whose bit is zero -> miss_count[item], their
// sum -> *miss_total.  Emitting: the same rows as (probe key, 0) / (probe position, ~0) at miss_base + miss_off[item] + rank, rank from
// ballot + popcount and one LDS cursor bump per wave (fj_mm_join_kernel's miss writer): consecutive lanes write consecutive rows ----
template <bool MAT, bool RID = false>
__global__ __launch_bounds__(MM_NT) void fj_mm_miss_sweep_kernel(FjMmSweepArgs w) {
    static_assert(FJ_CHUNK % 64 == 0, "a wave covers 64 consecutive rows of one chunk");
    __shared__ u32 cur;                                        // the item's misses (counting) / its miss cursor (emitting)
    const u32 tid = threadIdx.x, lane = tid & 63;
    const u32 item = blockIdx.x;
    const uint4 it = w.items[item];
    const u32 s_lo = it.x, s_hi = it.x + it.y;
    if (MAT && w.miss_count[item] == 0) return;
    if (tid == 0) cur = 0;
    __syncthreads();
    const u64 mbase = MAT ? w.miss_base + w.miss_off[item] : 0;
    u32 lmiss = 0;
    for (u32 pc = s_lo; pc < s_hi; pc += MM_NT / FJ_CHUNK) {
        const u32 c = pc + tid / FJ_CHUNK, off = tid % FJ_CHUNK;
        bool miss = false;
        u64 psrc = 0;
        if (c < s_hi) {
            const u32 e = w.probe.list[c];
            psrc = (u64)FJ_LIST_ID(e) * FJ_CHUNK + off;
            if (off < FJ_LIST_CNT(e)) miss = !((w.pbits[psrc >> 6] >> (psrc & 63)) & 1ull);
        }
        const u64 mbal = __ballot(miss);
        if (!MAT) { lmiss += (u32)__popcll(mbal); continue; }
        if (mbal) {
            u32 wm = 0;
            if (lane == 0) wm = atomicAdd(&cur, (u32)__popcll(mbal));
            wm = __shfl(wm, 0, 64);
            if (miss) {
                const u64 o = mbase + wm + (u32)__popcll(mbal & ((1ull << lane) - 1ull));
                w.out_keys[o] = RID ? (w.probe.vals ? w.probe.vals[psrc] : psrc) : fj_key_unmix(w.probe.keys[psrc]);      // (chunk pools hold mixed keys)
                w.out_vals[o] = RID ? ~0ull : 0ull;
            }
        }
    }
    if (!MAT) {
        if (lane == 0 && lmiss) atomicAdd(&cur, lmiss);
        __syncthreads();
        if (tid == 0) {
            const u32 m = cur;
            w.miss_count[item] = m;
            if (m) atomicAdd(w.miss_total, (unsigned long long)m);
        }
    }
}

}  // namespace

hipError_t fj_launch_mm_join(const FjLdsJoinArgs& a, bool materialize, hipStream_t s, int outer, const FjMmOuterArgs* oa) {
    const u32 nb = a.items ? a.items_cap : a.nparts * a.nsplit;
    u32 lds = sizeof(MmHdr) + MM_S * 8 + MM_ROWS * 8 + MM_S * 4 + MM_ROWS * 4;
    static_assert(sizeof(MmHdr) == 32, "the inner form's LDS footprint stays 147488 bytes");
    auto kern = materialize ? (a.row_ids ? fj_mm_join_kernel<true, true> : fj_mm_join_kernel<true>) : fj_mm_join_kernel<false>;
    FjMmOuterArgs o{};
    if (outer != FJ_MM_INNER) {
        if ((outer != FJ_MM_LEFT && outer != FJ_MM_FULL) || !oa || !oa->miss_count) return hipErrorInvalidValue;
        o = *oa;
        if (materialize) {                                   // (FULL emits as LEFT does: the sweep behind it is the caller's)
            if (!o.miss_off || !a.out_keys || !a.out_vals) return hipErrorInvalidValue;
            kern = a.row_ids ? fj_mm_join_kernel<true, true, FJ_MM_LEFT> : fj_mm_join_kernel<true, false, FJ_MM_LEFT>;
        } else {
            if (!o.miss_total || (outer == FJ_MM_FULL && (!o.bits || !o.marked))) return hipErrorInvalidValue;
            kern = outer == FJ_MM_FULL ? fj_mm_join_kernel<false, false, FJ_MM_FULL> : fj_mm_join_kernel<false, false, FJ_MM_LEFT>;
            if (outer == FJ_MM_FULL) lds += MM_SBITS_WORDS * 4;
        }
    }
    hipError_t e = fj_set_max_lds_once(reinterpret_cast<const void*>(kern), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(nb), dim3(MM_NT), lds, s, a, o);
    return hipGetLastError();
}

hipError_t fj_launch_mm_tile_join(const FjLdsJoinArgs& a, bool materialize, hipStream_t s, int outer, const FjMmOuterArgs* oa) {
    if (!a.items || !a.items_cap || !a.build.list || !a.probe.list || !a.part_count) return hipErrorInvalidValue;
    if (materialize && (!a.out_off || !a.out_keys || !a.out_vals || !a.build.vals)) return hipErrorInvalidValue;
    u32 lds = materialize ? MT_LDS_MAT : MT_LDS_COUNT;
    auto kern = materialize ? (a.row_ids ? fj_mm_tile_kernel<true, true> : fj_mm_tile_kernel<true>) : fj_mm_tile_kernel<false>;
    FjMmOuterArgs o{};
    if (outer != FJ_MM_INNER) {                              // (counting pass only: the pairs of an outer form are emitted by the inner form)
        if ((outer != FJ_MM_LEFT && outer != FJ_MM_FULL) || materialize || !oa || !oa->pbits) return hipErrorInvalidValue;
        if (outer == FJ_MM_FULL && (!oa->bits || !oa->marked)) return hipErrorInvalidValue;
        o = *oa;
        kern = outer == FJ_MM_FULL ? fj_mm_tile_kernel<false, false, FJ_MM_FULL> : fj_mm_tile_kernel<false, false, FJ_MM_LEFT>;
        if (outer == FJ_MM_FULL) lds += MM_SBITS_WORDS * 4;
    }
    static_assert(MT_LDS_COUNT + MM_SBITS_WORDS * 4 <= MT_LDS_MAT, "the outer counting forms stay below the emitting form's footprint");
    hipError_t e = fj_set_max_lds_once(reinterpret_cast<const void*>(kern), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(a.items_cap), dim3(MM_NT), lds, s, a, o);
    return hipGetLastError();
}

hipError_t fj_launch_mm_miss_sweep(const FjMmSweepArgs& w, bool materialize, hipStream_t s) {
    if (!w.items || !w.nitems || !w.probe.list || !w.probe.keys || !w.pbits || !w.miss_count) return hipErrorInvalidValue;
    if (materialize ? (!w.miss_off || !w.out_keys || !w.out_vals) : !w.miss_total) return hipErrorInvalidValue;
    auto kern = materialize ? (w.row_ids ? fj_mm_miss_sweep_kernel<true, true> : fj_mm_miss_sweep_kernel<true>) : fj_mm_miss_sweep_kernel<false>;
    hipLaunchKernelGGL(kern, dim3(w.nitems), dim3(MM_NT), 0, s, w);
    return hipGetLastError();
}
