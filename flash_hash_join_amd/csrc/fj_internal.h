// fj_internal.h -- host-side declarations shared by the .hip translation units.
#pragma once
#include "fj_common.h"

// device error word bits
#define FJ_ERR_POOL 1u       // chunk pool exhausted (sizing bug) -> call fails
#define FJ_ERR_LDS_FULL 2u   // a final partition does not fit its LDS table -> global-table fallback
#define FJ_STAT_DUPS 4u      // (status, not an error) the build side holds duplicate keys
#define FJ_STAT_RETRY 8u     // (status) some counting-join items overflowed the cuckoo table: part_count[item] == FJ_ITEM_RETRY marks them
#define FJ_STAT_EMIT_RETRY 16u // (status) some items of the emitting pass overflowed the cuckoo table: marked the same way, redone on the tagged table
#define FJ_ERR_VARIANT 32u   // filters handed to the filter kernel were built with another bloom_variant (sender-side precheck across ranks)
#define FJ_BLOOM_HDR_MAGIC 0xB100F000u   // exported filter sets end with 4 header words: [0] = magic | variant
#define FJ_STAT_TOOBIG 64u   // (status) some items' partitions hold more distinct build keys than even the tagged LDS table takes: part_count[item] == FJ_ITEM_TOOBIG marks them; the host re-partitions just those
#define FJ_ERR_OUTCAP 128u   // single-pass materialising join: more pairs than the caller's output buffers hold
#define FJ_ERR_PAIR_COLLISION 256u // FJ_ALGO_KEY_PAIR: two distinct pairs share a combined word (fj_key_pair) -> global-table fallback, which compares pairs
#define FJ_ITEM_RETRY 0xFFFFFFFFu
#define FJ_ITEM_TOOBIG 0xFFFFFFFEu

// ---- partition pass ---------------------------------------------------------------------------
struct FjPartArgs {
    // input: flat arrays (in_list == nullptr) or a bucket-grouped chunk list over a chunk pool
    const u64* in_keys;
    const u64* in_vals;
    const u32* in_list;
    const u32* in_dir;
    const uint4* in_tiles;   // list input: tile table {first list index, chunks, bucket, -}
    const u32* in_ntiles;    // device scalar: number of tiles
    u64 n_flat;
    u32 parent0;             // bucket id of every key of a flat input
    // output chunk pool
    u64* out_keys;
    u64* out_vals;
    u32* out_dir;            // pre-set to FJ_DIR_INVALID
    u64* out_rel;            // per chunk: (producing segment << 32) | rank inside (segment, bucket)
    u32* seg_off;            // [max_segs][F] span offset of a segment inside a bucket's chunk list
    u32* bchunks;            // [nb_out] chunks per bucket (zeroed before the pass)
    u32* alloc;              // device scalar: next unallocated chunk id (zeroed before the pass)
    u32* seg_counter;        // device scalar: next segment id (zeroed before the pass)
    u32 cap_chunks;
    u32 max_segs;
    u32* err;
    // radix digit: bucket = (hash >> shift) & (2^fan_log - 1)
    u32 shift;
    u32 fan_log;
    u32 side;                // 0 = build relation, 1 = probe relation (selects the kernel's name only)
    u32 slab;                // chunk ids a workgroup takes per allocator hit (fj_slab_for; a multiple of the run length)
    u32 run_log;             // chunk ids per (segment, bucket) in aligned runs of 2^run_log (0 or FJ_RUN_LOG; FjChunkSet::run_log of the output)
    // chunk-list input in the owner shuffle's 7-byte wire format (chunks received from other GPUs, csrc/fj_pack.hip): chunk id i
    // lives at byte i * FJ_WIRE7_BYTES of in_keys; bits 56..63 of its keys = (in_b0 + the tile's parent bucket) >> in_top_shift
    u32 in_pk7, in_b0, in_top_shift;
    // flat input with values: 1 = the values are the rows' 0-based positions, made by the pass (in_vals is not read; row-id joins)
    u32 vals_pos;
};

// a chunk pool plus its per-bucket chunk lists (output of one pass, input of the next)
struct FjChunkSet {
    u64* keys;               // chunk pool, or (list == nullptr) a flat array of n_flat keys
    u64* vals;               // nullptr for the probe side
    u64 n_flat;
    u32* dir;                // [cap]
    u64* rel;                // [cap]
    u32* seg_off;            // [max_segs][fan]
    u32* alloc;              // device scalar
    u32 cap;
    u32 nb;                  // number of buckets at this level
    u32 fan_mask;            // fan-out of the producing pass - 1
    u32 max_segs;
    u32* bchunks;            // [nb]   chunks per bucket
    u32* boff;               // [nb+1] chunk-list offsets; boff[nb] = list length
    u32* list;               // [cap]  chunk ids grouped by bucket
    u32 run_log;             // chunk ids were handed out in aligned runs of 2^run_log ids per (segment, bucket), used in order, the unused rest
                             // marked FJ_DIR_INVALID (the partition pass: FJ_RUN_LOG); 0: every id stands alone (bloom stage, owner shuffle)
};

u32 fj_partition_lds_bytes(u32 fan_log, bool vals, int line_log);
// chunks (of 256 rows) per input tile of the pass kernel chosen for this fan-out and payload
u32 fj_partition_tile_chunks(u32 fan_log, bool vals);
hipError_t fj_launch_partition(const FjPartArgs& a, bool vals, int line_log, u32 grid, hipStream_t s);
// level bookkeeping after a pass: chunk-list offsets (clears cs.bchunks for the next join), chunk lists, and the tile table
// of the level's consumer (tc chunks per tile; 0 = none); zero_tail: optional [max_tiles] array whose entries past the
// number of tiles are cleared
hipError_t fj_launch_group(const FjChunkSet& cs, u32 tc, u32* toff, uint4* tiles, u32 max_tiles, u32* zero_tail, hipStream_t s);
hipError_t fj_launch_scan_u32_to_u64(const u32* in, u64* out, u32 n, hipStream_t s);
// received chunks (directory words only) -> (segment, rank, span offset) for fj_launch_group; fan = power of two >= nbk
hipError_t fj_launch_dir_rank(u32* dir, u32 n, u32 b_lo, u32 nbk, u32 fan, u64* rel, u32* seg_off, u32* bchunks, u32* nalloc, hipStream_t s);

// ---- bloom precheck between two probe-side passes (csrc/fj_bloom.hip) ----------------------------
struct FjBloomArgs {
    // hot: read for every tile - these stay in scalar registers across the kernel's loop
    const u64* pkeys;            // probe relation at the filtered level: chunk pool,
    const u32* plist;            // chunk lists,
    const uint4* tiles;          // and the tile table over them (tiles of fj_bloom_tile_chunks() chunks)
    u64* out_keys; u32* out_dir; u64* out_rel;   // output chunk pool: same bucket structure, survivors only (a level with fan-out 1)
    u32 cap_chunks;
    u32 pnb;                     // buckets of the level
    // cold: read at kernel start, at a bucket change, or once per slab of output chunks.  The kernel reads them through
    // bf_late_args() at the point of use, so that they do not occupy scalar registers across the loop (round 2's form of this
    // kernel spilled ~95 scalar registers into vector lanes: a v_readlane per use)
    const u32* toff;             // [pnb+1] first tile of every bucket; toff[pnb] = number of tiles
    const u64* bkeys; const u32* blist; const u32* bboff;   // build relation at the filtered level (filter source)
    u32* seg_off; u32* bchunks; u32* alloc; u32* seg_counter;
    u32 max_segs;
    u32* err;
    unsigned long long* survivors;   // device scalar: probe keys that passed
    const u32* prebuilt;             // non-null: filters come from HBM (FJ_BLOOM_WORDS words per bucket) instead of being built from the build keys
    unsigned long long* bucket_keys; // non-null: [pnb] survivors per bucket are accumulated here (zeroed by the caller)
};
u32 fj_bloom_tile_chunks();
u32 fj_bloom_waves_per_group();
u32 fj_bloom_slab_chunks();
hipError_t fj_launch_bloom_filter(const FjBloomArgs& a, u32 grid, int variant, hipStream_t s);
// all bucket filters of a build-side level -> HBM; chunk set -> dense array (base[nb+1] receives the buckets' offsets, base[nb] the total)
hipError_t fj_launch_bloom_export(const FjChunkSet& build, u32* out, u32 grid, int variant, hipStream_t s);
hipError_t fj_launch_flatten(const FjChunkSet& cs, const unsigned long long* bucket_keys, unsigned long long* base, u64* out, hipStream_t s);

// ---- owner shuffle, sender side (csrc/fj_pack.hip): level-1 chunk set -> dense wire-format chunks grouped by owner GPU ----------
struct FjPackArgs {
    const u64* keys; const u64* vals;            // the packing pass's chunk pool (vals: nullptr for keys-only relations)
    const u32* list; const u32* boff;            // its chunk lists
    u32 nb, fan_log, nranks, wire7;              // nb = 2^fan_log first-pass buckets; wire7: 7-byte chunks (fan_log >= 8), else 8-byte
    uint4* fi;                                   // [output chunks] descriptor: {list entry of the input chunk holding the chunk's key 0, the next entry,
                                                 //  position of key 0 inside that input chunk, index of that entry in the chunk list}
    u32* fb;                                     // [output chunks] the chunk's directory word (bucket << 9 | keys)
    u32* bkeys;                                  // [nb] keys per bucket
    u32* obase;                                  // [nb + 1] output chunks before bucket b; [nb + 1 + r]: first output chunk of owner r
    unsigned long long* used;                    // [nranks] output chunks per owner
    unsigned char* dst_k[64]; u64* dst_v[64]; u32* dst_d[64];   // per owner: where its chunks, values and directory words go
};
hipError_t fj_launch_pack_plan(const FjPackArgs& a, hipStream_t s);       // fills fi, bkeys, obase, used
// sender-side precheck in chunk form (csrc/fj_pack.hip): FJ_PFILT_BYTES of Bloom filter per final partition of the global plan
#define FJ_PF_COUNTERS 4u              // work counters per XCD of fj_part_filter_inplace
#ifndef FJ_PFILT_BYTES
#define FJ_PFILT_BYTES 4096u
#endif
hipError_t fj_launch_part_filter_export(const FjChunkSet& build, u64* out, u32 grid, hipStream_t s);            // owner: [build.nb][FJ_PFILT_BYTES / 8]
hipError_t fj_launch_part_filter_inplace(const FjChunkSet& cs, const u64* filters, u32 part_shift, unsigned long long* kept, u32* next_of_xcd /* [8 * FJ_PF_COUNTERS], zeroed */, u32 grid, hipStream_t s);
hipError_t fj_launch_part_filter_sample(const u64* raw, u64 n, u64 stride, const u64* filters, u32 part_shift, unsigned long long* kept, hipStream_t s);
hipError_t fj_launch_pack_squeeze(const FjPackArgs& a, u32 grid, hipStream_t s);

// A partition pass is ONE persistent workgroup per CU with a static share of the tiles: a workgroup that finds no free CU (RCCL's
// send / receive kernels hold some for the length of an exchange) starts when another one has finished, and the pass takes twice as
// long.  While a multi-GPU step runs, the passes therefore launch num_cus - n workgroups (csrc/fj_dist.hip; internal, not part of the
// public header).  n = 0 restores the full grid.
// (fj_ctx_reserve_cus: include/flashjoin.h)

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel, device) instead of on every launch
hipError_t fj_set_max_lds_once(const void* fn, u32 bytes);

// ---- joins ------------------------------------------------------------------------------------
struct FjLdsJoinArgs {
    FjChunkSet build, probe;     // final-level chunk sets (same nb), or flat arrays (list == nullptr)
    u32 nparts;                  // number of final partitions
    u32 nsplit;                  // flat probe side only: work items per partition (equal slices of the probe side)
    // chunk-list probe side: work items = tiles of the probe chunk lists, {first list index, chunks, partition, -}; a
    // partition with many probe chunks (skew) becomes many items, each rebuilding the partition's small table
    const uint4* items;          // nullptr for a flat probe side
    const u32* nitems_dev;       // device scalar: number of valid entries of items[]
    u32 items_cap;               // allocated entries (grid of the one-workgroup-per-item kernels)
    u32* part_count;             // [items] matches per work item
    unsigned long long* total;   // device scalar
    u32* err;
    // materialise
    const u64* out_off;          // [items+1] exclusive scan of part_count
    u64* out_keys;
    u64* out_vals;
    // single-pass materialising join (fj_emit_join_persistent<SINGLE>): no counting pass, no per-item offsets - every probe round
    // reserves its pairs' output range on this device cursor (one atomic per workgroup and round); out_capacity = pairs the
    // output buffers hold.  The cursor ends as the join's match count.
    unsigned long long* out_cursor;
    u64 out_capacity;
    u32 retry_only;              // tagged-table counting kernel: process only the items the cuckoo kernel marked FJ_ITEM_RETRY
    u32 mark_toobig;             // tagged-table counting kernel, many-to-many counting kernel (every form): a partition beyond the table marks its item FJ_ITEM_TOOBIG (FJ_STAT_TOOBIG) instead of raising FJ_ERR_LDS_FULL
    u32 want_dups;               // counting pass of a materialising join: report duplicate build keys (FJ_STAT_DUPS)
    u32 dedup;                   // materialising pass: build 'values' are row indices, the smallest wins, then orig_vals[idx]
    const u64* orig_vals;        // the caller's build_values (dedup only)
    u32 avg_build_keys;          // build rows per final partition on average (host hint: selects the 16384-slot counting kernel, fj_join_wide.hip)
    unsigned long long* dbg;     // diagnostic: per-item phase stamps (s_memrealtime), nullptr in production
    u32 dbg_flags;               // diagnostic ablations: 1 = skip lookups, 2 = skip inserts, 4 = no output stores (results wrong on purpose); 8 = test hook: the cuckoo emit kernel sends every 7th item down its retry path (results exact)
    // row-id join (FJ_ALGO_ROW_IDS): both sides' values are row positions (chunk pools: the vals plane; flat arrays: the index
    // itself, vals == nullptr); the writers put the probe row's position in out_keys and the build row's in out_vals
    u32 row_ids;
};
// next_item: device word for the persistent counting kernel's work counter (nullptr: one workgroup per item)
hipError_t fj_launch_lds_join(const FjLdsJoinArgs& a, bool materialize, hipStream_t s, u32* next_item = nullptr,
                              u32 persistent_min_items = 8192);
// the single-pass materialising join over chunk lists (a.out_cursor != nullptr; unique build keys: duplicates are reported, FJ_STAT_DUPS)
hipError_t fj_launch_emit_single(const FjLdsJoinArgs& a, hipStream_t s, u32* next_item);
// ---- counting join with a 16384-slot table, one 1024-thread workgroup per CU (csrc/fj_join_wide.hip) ----
// for joins whose build side is not small against the probe side (wide_join_planned, fj_plan.hip), and for the multi-GPU
// build-broadcast form, whose build side arrives as dense per-partition runs from every rank (DENSE)
#define FJ_WIDE_MAXSRC 16u
struct FjWideArgs {
    const u32* toff; u32 part_lo, part_hi;       // toff != nullptr: only the items of partitions [part_lo, part_hi) (toff = first item of every partition)
    // DENSE build side: source s keeps, at byte offsets into base, an offset table u32[nparts + 1] (keys before partition p), the keys'
    // low words u32[n_s] and the low (32 - bits) bits of their high words as u16[n_s] (mid_bytes == 2) or u32[n_s]; partition p supplies the top `bits` bits
    const unsigned char* base; u32 nsrc, bits, mid_bytes;
    u32 group_log;                               // items are dealt to the workgroups in runs of 2^group_log consecutive ones (0: one by one); > 0 where partitions are cut into several items: a run's items of one partition share one table build
    u32 max_units;                               // DENSE: a partition of more 256-slot load units than this is marked for the retry ladder (0: the kernel's own limit, 32 = 8192 key slots)
    u32 pmask;                                   // the bits of a mixed key's HIGH word that name its final partition (all radix digits come from hash word 1): what tells a
                                                 // table entry of the partition in place from one that an earlier partition left behind (fj_wide_pmask)
    u64 offs_off[FJ_WIDE_MAXSRC], lo_off[FJ_WIDE_MAXSRC], mid_off[FJ_WIDE_MAXSRC];
};
hipError_t fj_launch_count_join_wide(const FjLdsJoinArgs& a, const FjWideArgs& w, bool dense, u32 grid, hipStream_t s);
// FjWideArgs::pmask of a plan of `bits` radix bits taken from bit `top_bits` of the mixed key downwards (top_bits = 64 or 48)
static inline u32 fj_wide_pmask(int bits, int top_bits) { return bits <= 0 ? 0u : (bits >= 32 ? 0xFFFFFFFFu : ((1u << bits) - 1u) << (top_bits - 32 - bits)); }

// second chance for the items whose partition overflowed the cuckoo table (load > ~0.45): the tagged 2x4-slot table
// with linear-probing overflow holds up to 8128 keys; only a partition beyond that raises FJ_ERR_LDS_FULL
hipError_t fj_launch_lds_join_retry(const FjLdsJoinArgs& a, hipStream_t s);
hipError_t fj_launch_lds_emit_retry(const FjLdsJoinArgs& a, hipStream_t s, bool only_marked = true);   // same for the emitting pass (FJ_STAT_EMIT_RETRY); only_marked = false: every item

// how many of `nsamples` evenly spaced probe rows have their key in the build side (final chunk set `build`, partition id =
// (hash word 1 >> shift32) & pmask): one wave per sample scans the sample's build partition
hipError_t fj_launch_sample_hits(const FjChunkSet& build, const u64* pk, u64 np, u32 nsamples, u32 shift32, u32 pmask,
                                 unsigned long long* hits, hipStream_t s);

// many-to-many join of one work item's partition (csrc/fj_many.hip): counting (part_count / total) or emitting at out_off
// outer forms (FJ_ALGO_ALL_COPIES): FJ_MM_LEFT also reports the probe rows without a partner; FJ_MM_FULL (counting pass) also marks
// the build rows that have one in `bits`, the bitmap fj_launch_full_sweep reads (one bit per row of the build side's final chunk
// pool, zeroed before the launch).  The emitting pass is the same for both: pairs at out_off[item], misses at miss_base + miss_off[item]
#define FJ_MM_INNER 0
#define FJ_MM_LEFT 1
#define FJ_MM_FULL 2
struct FjMmOuterArgs {
    u32* miss_count;                 // [items] probe rows without a partner per work item (zeroed before the counting launch)
    unsigned long long* miss_total;  // device scalar: their sum, u
    const u64* miss_off;             // emitting pass: [items+1] exclusive scan of miss_count
    u64 miss_base;                   // emitting pass: first row of the misses' range (P, the number of pairs)
    u64* bits;                       // FULL, counting pass
    unsigned long long* marked;      // FULL, counting pass: device scalar, build rows whose bit this launch turned on (r = nb - marked)
    u64* pbits;                      // tile kernel, counting pass of LEFT and FULL: one bit per row of the PROBE side's final chunk pool (indexed as `bits`
                                     // indexes the build pool), zeroed before the launch; a probe row that finds a partner in a tile sets its bit
};
hipError_t fj_launch_mm_join(const FjLdsJoinArgs& a, bool materialize, hipStream_t s, int outer = FJ_MM_INNER, const FjMmOuterArgs* oa = nullptr);
// the same over (probe item, build tile) work items of partitions beyond 4096 build rows (a.mark_toobig made the counting launch
// above mark their items FJ_ITEM_TOOBIG): a.items[i] = {first probe list index, probe chunks, partition, first build chunk of the tile
// within the partition's chunk list}, a tile = FJ_MM_TILE_CHUNKS chunks; exactly a.items_cap items (a.nitems_dev is not read).
// outer = FJ_MM_LEFT / FJ_MM_FULL, counting pass only (the pairs of an outer form are emitted by the inner form: a pair lives in one
// tile): a probe row that finds a partner in the tile sets its bit in oa->pbits - "no partner" is a verdict over ALL tiles of the
// partition, fj_launch_mm_miss_sweep reads it off the bitmap afterwards - and FULL marks the tile's matched build rows in oa->bits and
// adds the newly set bits to oa->marked, as fj_launch_mm_join's FULL form does (miss_count, miss_total, miss_off are not read)
#define FJ_MM_TILE_CHUNKS 16u
hipError_t fj_launch_mm_tile_join(const FjLdsJoinArgs& a, bool materialize, hipStream_t s, int outer = FJ_MM_INNER, const FjMmOuterArgs* oa = nullptr);
// the probe rows of the oversized items that no tile gave a partner: one workgroup per item of items[] = {first probe list index, probe
// chunks, -, -} (the items the counting launch marked FJ_ITEM_TOOBIG, nothing else: the cost follows them, not the probe side).
// Counting: miss_count[i] = rows of item i whose bit in pbits is zero, their sum added to *miss_total.  Emitting: the same rows as
// (probe key, 0) - row ids: (probe position, ~0) - at miss_base + miss_off[i] + rank within the item
struct FjMmSweepArgs {
    FjChunkSet probe;
    const uint4* items; u32 nitems;
    const u64* pbits;
    u32* miss_count;                 // [nitems]
    unsigned long long* miss_total;  // counting
    const u64* miss_off;             // emitting: [nitems + 1] exclusive scan of miss_count
    u64 miss_base;
    u64* out_keys; u64* out_vals;
    u32 row_ids;
};
hipError_t fj_launch_mm_miss_sweep(const FjMmSweepArgs& w, bool materialize, hipStream_t s);

struct FjGtArgs {                // global (non-partitioned) table
    u64* tkeys; u64* tvals; u32* bloom;    // bloom == nullptr: no precheck
    u64 cap_mask;                           // capacity - 1 (capacity = power of two, multiple of 8)
    u32* flags;                             // [0] = build saw FJ_EMPTY_KEY, value in empty_val
    u64* empty_val;
    const u64* bk; const u64* bv; u64 nb;
    const u64* pk; u64 np;
    u32* wg_count;                          // [grid] matches per workgroup
    unsigned long long* total;
    const u64* out_off;                     // [grid+1]
    u64* out_keys; u64* out_vals;
    u32 row_ids;                            // row-id join: tvals hold first-occurrence row indices (fj_gt_build_first_kernel); the writer
                                            // puts the probe row's index in out_keys and the table's in out_vals
    u32* matched;                           // full outer join: one bit per table slot, set by the outer probe on a hit (zeroed before it;
                                            // capacity / 32 words + one more: a probe row hit the empty marker key); nullptr otherwise
};
hipError_t fj_launch_gt_build(const FjGtArgs& a, hipStream_t s);
hipError_t fj_launch_gt_probe(const FjGtArgs& a, bool materialize, u32 grid, hipStream_t s);

// ---- multi-GPU owner split --------------------------------------------------------------------
hipError_t fj_launch_owner_hist(const u64* keys, u64 n, u32 nranks, unsigned long long* counts, hipStream_t s);
hipError_t fj_launch_owner_scatter(const u64* keys, const u64* vals, u64 n, u32 nranks,
                                   const unsigned long long* offsets, unsigned long long* cursors,
                                   u64* out_keys, u64* out_vals, hipStream_t s);

// ---- synthetic data ---------------------------------------------------------------------------
hipError_t fj_launch_iota(u64* out, u64 n, hipStream_t s);
hipError_t fj_launch_gen_build(u64* keys, u64* vals, u64 first, u64 n, hipStream_t s);
hipError_t fj_launch_gen_probe(u64* keys, u64 first, u64 n, u64 build_total, u64 seed, u32 hit_bp,
                               unsigned long long* expected_hits, hipStream_t s);

// owner GPU of a key: range reduction of the top 16 bits of hash word 1
__host__ __device__ inline u32 fj_owner_of_w1(u32 w1, u32 nranks) { return ((w1 >> 16) * nranks) >> 16; }

// ---- left outer / anti joins (csrc/fj_outer.hip; FJ_ALGO_LEFT_OUTER / FJ_ALGO_ANTI of include/flashjoin.h) ----------------------
// Output rows: hits (probe key, build value) from a front cursor counting up from 0, misses (probe key[, 0]) from a back cursor
// counting down from np.  One LDS cursor pair per workgroup collects a round's reservations wave by wave (ballot + popcount); thread 0
// turns the round's totals into global ranges with ONE atomic per cursor, behind a barrier.
#define FJ_OJ_LEFT 0          // left outer join, unique build keys (duplicates: FJ_STAT_DUPS)
#define FJ_OJ_ANTI 1          // anti join: misses only, keys only
#define FJ_OJ_LEFT_FIRST 2    // left outer join whose build 'values' are row indices: the smallest wins, then orig_vals[idx]
struct FjOjCursor { u32 hit, miss; u64 hit_base, miss_base; };
// called by every thread of the workgroup with its wave's totals nh / nm (wave-uniform): returns the first hit row and the first
// miss rank (counted from the back) of the calling wave in this round
__device__ __forceinline__ void fj_oj_reserve(FjOjCursor* cur, u32 nh, u32 nm, u32 lane, u32 tid, unsigned long long* ghit,
                                              unsigned long long* gmiss, u64& hpos, u64& mpos) {
    u32 wh = 0, wm = 0;
    if (lane == 0) { if (nh) wh = atomicAdd(&cur->hit, nh); if (nm) wm = atomicAdd(&cur->miss, nm); }
    wh = __shfl(wh, 0, 64); wm = __shfl(wm, 0, 64);
    __syncthreads();
    if (tid == 0) {
        const u32 H = cur->hit, M = cur->miss;
        cur->hit_base = H ? (u64)atomicAdd(ghit, (unsigned long long)H) : 0ull;
        cur->miss_base = M ? (u64)atomicAdd(gmiss, (unsigned long long)M) : 0ull;
        cur->hit = 0; cur->miss = 0;
    }
    __syncthreads();
    hpos = cur->hit_base + wh; mpos = cur->miss_base + wm;
}
// a.out_cursor counts the hits, miss_cursor the misses; a.out_capacity >= np (rows beyond it are never written: FJ_ERR_OUTCAP)
hipError_t fj_launch_outer_join(const FjLdsJoinArgs& a, int mode, u64 np, unsigned long long* miss_cursor, hipStream_t s);
// global table: build with row indices (first occurrence; vals = false: keys only), then the outer probe (a.total = hit cursor)
hipError_t fj_launch_gt_build_first(const FjGtArgs& a, bool vals, hipStream_t s);
hipError_t fj_launch_gt_outer_probe(const FjGtArgs& a, int mode, unsigned long long* miss_cursor, u64 out_capacity, hipStream_t s);

// ---- probe-order joins (csrc/fj_aligned.hip; FJ_ALGO_PROBE_ORDER of include/flashjoin.h) -----------------------------------------
// One output row per probe row at the row's own position (the probe chunk pool's vals plane; flat arrays: the index): a.out_vals[pos]
// (nullptr: the mask form, the build side carries no values) and / or mask[pos] = 1 / 0.  first: the build 'values' are row indices,
// the smallest wins, then a.orig_vals[idx] - or, a.row_ids, the index itself (a miss: ~0 instead of 0); !first: unique build keys
// expected (duplicates: FJ_STAT_DUPS).  a.total counts the hits, miss_total the misses; positions >= np are not written (FJ_ERR_OUTCAP).
hipError_t fj_launch_probe_order_join(const FjLdsJoinArgs& a, bool first, u64 np, unsigned long long* miss_total, unsigned char* mask, hipStream_t s);
// global table built by fj_launch_gt_build_first (vals = a.out_vals != nullptr): thread i serves probe row i
hipError_t fj_launch_gt_probe_order(const FjGtArgs& a, unsigned long long* miss_total, unsigned char* mask, hipStream_t s);

// ---- prepared build side (csrc/fj_prepared.hip; FJ_ALGO_RETAIN_BUILD / FJ_ALGO_REUSE_BUILD of include/flashjoin.h) -------------------
// Three dense planes of one row per DISTINCT build key - the mixed key, the position of its first occurrence, that row's value - in
// which final partition p owns the run [runs[p].off, runs[p].off + runs[p].n); the mixed empty marker is an ordinary row of its run.
struct FjPrepRun { u64 off, n; };
// One workgroup per final partition of `rel` (chunk lists whose vals plane holds the rows' positions; flat arrays: one partition, the
// index is the position): the partition's distinct keys, first positions and - orig_vals != nullptr - orig_vals[first position] go to
// the run that ONE atomic on `cursor` reserves; the cursor ends as g.  runs[] is zeroed before the launch (an empty partition writes
// no record).  A partition of more distinct keys than the probe kernel's table takes writes nothing and raises FJ_ERR_LDS_FULL; a row
// at or beyond out_capacity or a position at or beyond nrows is not stored (FJ_ERR_OUTCAP).
struct FjPrepBuildArgs {
    FjChunkSet rel;
    u32 nparts;
    const u64* orig_vals; u64 nrows;                         // the caller's build_values (nullptr: a keys-only side) / build rows
    u64* out_keys; u64* out_rows; u64* out_vals;
    u64 out_capacity;
    FjPrepRun* runs;
    unsigned long long* cursor;                              // device scalar, zeroed before the launch
    u32* err;
};
hipError_t fj_launch_prep_build(const FjPrepBuildArgs& a, hipStream_t s);
// The probe-order join's probe phase against those runs; the work items are the one-shot join's (items: tiles of the probe chunk lists;
// nullptr: nsplit equal slices of a flat probe side).  out_vals[pos] = plane[row of the key] (plane: the values or the positions), or
// miss_word; out_vals == nullptr: the mask form, a keys-only table.  total counts the hits, miss_total the misses; positions >= np are
// not written (FJ_ERR_OUTCAP); a run that is not one of fj_launch_prep_build's (beyond the table, beyond nkeys rows): FJ_ERR_LDS_FULL.
struct FjPrepProbeArgs {
    FjChunkSet probe;
    u32 nparts, nsplit;
    const uint4* items; const u32* nitems_dev; u32 items_cap;
    const u64* keys; const u64* plane; const FjPrepRun* runs; u64 nkeys;
    u64 miss_word;
    u64* out_vals; unsigned char* mask; u64 np;
    unsigned long long* total; unsigned long long* miss_total;
    u32* err;
};
hipError_t fj_launch_prep_probe(const FjPrepProbeArgs& a, hipStream_t s);
// The build-order aggregate join's probe phase against those runs (FJ_ALGO_BUILD_ORDER | FJ_ALGO_REUSE_BUILD); work items as above.  The
// table is loaded from the run with one accumulator per slot at the aggregate's identity; a hit is one LDS atomic; the flush reads the
// run once more and combines every accumulator that left the identity into out[rows[row of the key]] with ONE global atomic - several
// items may serve one partition, and out may hold a running aggregate (it holds the identity, or whatever the caller accumulates into,
// before the launch).  agg: FJ_GJ_* below; every form but FJ_GJ_COUNT reads probe.vals.  total / miss_total (both or neither) count the
// hits and the misses; a first position >= nb is not written (FJ_ERR_OUTCAP); a foreign run: FJ_ERR_LDS_FULL.
struct FjPrepGroupArgs {
    FjChunkSet probe;
    u32 nparts, nsplit;
    const uint4* items; const u32* nitems_dev; u32 items_cap;
    const u64* keys; const u64* rows; const FjPrepRun* runs; u64 nkeys;
    u64* out; u64 nb;
    unsigned long long* total; unsigned long long* miss_total;
    u32* err;
};
hipError_t fj_launch_prep_group(const FjPrepGroupArgs& a, int agg, hipStream_t s);
// ... and against the HBM-table form (the table of fj_launch_gt_build_first, vals = true: a.tkeys / a.tvals / a.flags / a.empty_val):
// thread i serves probe row a.pk[i]; a hit adds 1 at out_cnt[first position] and / or combines pv[i] into out_val[first position] with
// the typed global atomic - no accumulator arrays, no flush; a hot key serialises at its output word.  a.total counts the hits
hipError_t fj_launch_prep_gt_group(const FjGtArgs& a, int agg, const u64* pv, u64* out_cnt, u64* out_val, u64 nb,
                                   unsigned long long* miss_total, u32* err, hipStream_t s);

// ---- build-order aggregate joins (csrc/fj_group.hip; FJ_ALGO_BUILD_ORDER of include/flashjoin.h) ------------------------------------
// One output word per build row at the row's own position (the build chunk pool's vals plane; flat arrays: the index).  sum = false:
// out[pos] += the probe rows of the item's slice that carry the row's key; sum = true: += the sum of their values (a.probe.vals).  out
// holds nb words and is zeroed before the launch (several items may serve one partition: global atomic adds); out == nullptr (count
// form only): nothing is flushed.  a.total (may be null) receives P, the sum of all counts - the sum form adds its HITS instead and
// raises FJ_STAT_DUPS where a partition's build keys repeat (then the hits are not P).  A partition beyond the table: FJ_ERR_LDS_FULL.
// agg: FJ_GJ_COUNT / FJ_GJ_SUM as above; the four min / max forms combine the values with the native 64-bit atomic min / max of their
// signedness instead of adding them - out then holds the aggregate's identity (fj_group_identity) before the launch, not zeros - and
// report P like the sum form.  The three float forms (FJ_ALGO_AGG_FLOAT) read the words as IEEE-754 binary64: FJ_GJ_SUM_F is the sum
// form with the native f64 atomic add, FJ_GJ_MIN_F / FJ_GJ_MAX_F are min / max forms whose identities are the bits of +inf / -inf.
enum { FJ_GJ_COUNT = 0, FJ_GJ_SUM = 1, FJ_GJ_MIN_U = 2, FJ_GJ_MIN_S = 3, FJ_GJ_MAX_U = 4, FJ_GJ_MAX_S = 5,
       FJ_GJ_SUM_F = 6, FJ_GJ_MIN_F = 7, FJ_GJ_MAX_F = 8, FJ_GJ_LAST = FJ_GJ_MAX_F };
u64 fj_group_identity(int agg);                                         // 0, 0, UINT64_MAX, INT64_MAX, 0, INT64_MIN, +0.0, +inf, -inf
hipError_t fj_launch_group_fill(u64* out, u64 n, int agg, hipStream_t s);      // out[0 .. n) = the identity: a memset where it is a byte pattern, else a fill kernel
hipError_t fj_launch_group_join(const FjLdsJoinArgs& a, int agg, u64* out, u64 nb, hipStream_t s);
// global table built by fj_launch_gt_build_first (vals = false): one thread per probe row adds to cnt[slot] (and sum[slot] += pv[i] when
// out_sum is asked for), then thread i stores build row i's out_cnt[i] / out_sum[i]; cnt / sum: capacity + 1 zeroed words each (the last
// one is the empty key's); a.total += the counts of all build rows.  agg (used with out_sum): FJ_GJ_SUM, or a min / max form - sum[]
// then holds the aggregate's identity in all capacity + 1 words before the launch
hipError_t fj_launch_gt_group(const FjGtArgs& a, int agg, const u64* pv, unsigned long long* cnt, unsigned long long* sum, u64* out_cnt, u64* out_sum, hipStream_t s);

// ---- group-by on one relation (csrc/fj_groupby.hip; FJ_ALGO_GROUP_BY of include/flashjoin.h) ------------------------------------------
// One workgroup per final partition of `rel` (chunk lists with boff per partition; flat arrays: one partition): the partition's distinct
// keys go to out_keys, un-mixed, and - out_vals != nullptr - their aggregates beside them, in the rows [o, o + g_p) that ONE atomic on
// `cursor` reserves; the cursor ends as g.  agg: FJ_GJ_COUNT (1 per row), or FJ_GJ_SUM / a min / max form over rel.vals (flat arrays
// with rel.vals == nullptr: over the rows' indices - the first occurrence's position is FJ_GJ_MIN_U of them).  emit = false
// (FJ_GJ_COUNT only): the cursor alone.  A partition of more distinct keys than the table takes writes nothing and raises
// FJ_ERR_LDS_FULL; a row at or beyond out_capacity is not written (FJ_ERR_OUTCAP).
struct FjGroupByArgs {
    FjChunkSet rel;
    u32 nparts;
    u64* out_keys; u64* out_vals;
    u64 out_capacity;
    unsigned long long* cursor;  // device scalar, zeroed before the launch
    u32* err;
};
hipError_t fj_launch_group_by(const FjGroupByArgs& a, int agg, bool emit, hipStream_t s);
// the inverse form (FJ_ALGO_INVERSE): the distinct keys as above (out_keys) and, in out_vals, the result row of its key - the group id -
// for EVERY row of `rel` at the row's own position (rel.vals: the positions the first pass made; flat arrays: the index).  A position at
// or beyond out_capacity is not written (FJ_ERR_OUTCAP); a partition beyond the table writes nothing and raises FJ_ERR_LDS_FULL, while
// other partitions have written ids of the cursor the caller then abandons: the re-run must define every id again.
hipError_t fj_launch_group_by_inverse(const FjGroupByArgs& a, hipStream_t s);
// global table built by fj_launch_gt_build_first (vals = false) over a.bk: one thread per row combines into acc[slot] (capacity + 1 words
// holding the aggregate's identity, the last one the empty key's) - 1 per row (FJ_GJ_COUNT) or vals[i]
hipError_t fj_launch_gt_group_by_combine(const FjGtArgs& a, int agg, const u64* vals, u64* acc, hipStream_t s);
// ... and its capacity + 1 slots compacted into out rows [0, *cursor): (key, acc[slot]); out_vals == nullptr: the keys alone; out_keys
// == nullptr: the cursor alone.  Rows at or beyond out_capacity are not written (FJ_ERR_OUTCAP).  ids != nullptr (capacity + 1 words,
// the last one the empty key's; out_vals must be null): every occupied slot's row is stored there too
hipError_t fj_launch_gt_group_by_sweep(const FjGtArgs& a, const u64* acc, u64* out_keys, u64* out_vals, u64 out_capacity,
                                       unsigned long long* cursor, u32* err, hipStream_t s, u64* ids = nullptr);
// ... and, behind that sweep on the same stream, out_vals[i] = ids[slot of a.bk[i]] for the rows i < min(a.nb, out_capacity)
hipError_t fj_launch_gt_group_by_inverse(const FjGtArgs& a, const u64* ids, u64* out_vals, u64 out_capacity, hipStream_t s);
// the four-aggregate form (csrc/fj_groupby_multi.hip; FJ_ALGO_AGG_ALL): as fj_launch_group_by, but out_vals is FOUR planes of
// out_capacity words - row count, sum, minimum, maximum of rel.vals (required) - and the table takes 3840 distinct keys per partition.
// kind: the words of the value column as 0 uint64, 1 int64, 2 binary64.  out_capacity >= 1 may be below the number of groups: a row at
// or beyond it is not written (FJ_ERR_OUTCAP) while the cursor goes on counting
hipError_t fj_launch_group_by_all(const FjGroupByArgs& a, int kind, hipStream_t s);
// ... on the global table of fj_launch_gt_build_first (vals = false) over a.bk: acc is four planes of capacity + 1 words holding the
// identities of count, sum, min and max (the last word of each the empty key's); one thread per row combines into all four, and the
// sweep compacts the occupied slots into out rows [0, *cursor) of out_keys and of the four planes of out_vals at stride out_capacity
hipError_t fj_launch_gt_group_by_all_combine(const FjGtArgs& a, int kind, const u64* vals, u64* acc, hipStream_t s);
hipError_t fj_launch_gt_group_by_all_sweep(const FjGtArgs& a, const u64* acc, u64* out_keys, u64* out_vals, u64 out_capacity,
                                           unsigned long long* cursor, u32* err, hipStream_t s);
// the row of each group's extreme (csrc/fj_groupby_arg.hip; FJ_ALGO_AGG_ARG): as fj_launch_group_by, but a.rel.vals holds the rows'
// POSITIONS (the first pass made them; flat arrays: the index), the kernel gathers vals[position] (nrows words) itself, and out_vals is
// TWO planes of out_capacity >= nrows words - the smallest row index that holds the minimum (is_max: the maximum) of the key's rows, and
// that extreme.  kind: the words of vals as 0 uint64, 1 int64, 2 binary64 (compared as numbers)
hipError_t fj_launch_group_by_arg(const FjGroupByArgs& a, const u64* vals, u64 nrows, int kind, bool is_max, hipStream_t s);
// ... on the global table of fj_launch_gt_build_first (vals = false) over a.bk: ext and pos are planes of capacity + 1 words, ext
// holding every slot's extreme (fj_launch_gt_group_by_combine), pos all ones.  One thread per row offers its index to pos[slot] where
// vals[i] equals ext[slot]; the sweep compacts the occupied slots into out rows [0, *cursor) of out_keys and of the two planes of out_vals
hipError_t fj_launch_gt_group_by_arg_resolve(const FjGtArgs& a, int kind, const u64* vals, const u64* ext, u64* pos, hipStream_t s);
hipError_t fj_launch_gt_group_by_arg_sweep(const FjGtArgs& a, const u64* ext, const u64* pos, u64* out_keys, u64* out_vals, u64 out_capacity,
                                           unsigned long long* cursor, u32* err, hipStream_t s);
// the merge of partial group-bys (csrc/fj_groupby_merge.hip; FJ_ALGO_AGG_MERGE): as fj_launch_group_by_all, but a.rel.vals holds the
// partial rows' POSITIONS (the first pass made them; flat arrays: the index), the kernel gathers planes[q * nrows + position] for the four
// planes q - count, sum, min, max of every partial row - itself, the counts ADD in 64 bits, and the table takes 1920 distinct keys per
// partition.  kind: the words of the sum, min and max planes as 0 uint64, 1 int64, 2 binary64
hipError_t fj_launch_group_by_merge(const FjGroupByArgs& a, const u64* planes, u64 nrows, int kind, hipStream_t s);
// ... on the global table of fj_launch_gt_build_first (vals = false) over a.bk: acc as for fj_launch_gt_group_by_all_combine; one thread
// per partial row combines planes[q * a.nb + i] into all four.  fj_launch_gt_group_by_all_sweep compacts
hipError_t fj_launch_gt_group_by_merge_combine(const FjGtArgs& a, int kind, const u64* planes, u64* acc, hipStream_t s);
// two-column keys (csrc/fj_groupby_pair.hip; FJ_ALGO_KEY_PAIR), the pieces its forms share: out[i] = fj_key_pair(A[i], B[i]) for i < n;
// and the global table of ROW INDICES over the pairs - tab: cap_mask + 1 >= 2 nb words, all ones before the launch; behind it every
// pair's slot holds the pair's smallest row, and rows are found by comparing pairs from the home slot fj_hash64(fj_key_pair(a, b)) & cap_mask
hipError_t fj_launch_pair_combine(const u64* A, const u64* B, u64* out, u64 n, hipStream_t s);
hipError_t fj_launch_gt_pair_build(const u64* A, const u64* B, u64 nb, u64* tab, u64 cap_mask, hipStream_t s);

// ---- full outer join (FJ_ALGO_FULL_OUTER): the left outer join above plus the build rows nobody asked for ------------------------
// bits: one bit per build row, indexed by the row's place in the build side's final chunk pool (chunk id * FJ_CHUNK + offset; flat
// arrays: the row index), zeroed before the launch.  Every work item ORs in the rows whose key one of its probe rows hit (mode
// FJ_OJ_LEFT or FJ_OJ_LEFT_FIRST; otherwise fj_launch_outer_join).
hipError_t fj_launch_outer_join_full(const FjLdsJoinArgs& a, int mode, u64 np, unsigned long long* miss_cursor, u64* bits, hipStream_t s);
// the rows with a zero bit, compacted into out rows [base, base + *cursor): (key, value), or (~0, build position) in the row-id
// form; orig_vals != nullptr: the vals plane holds row indices into it.  Rows at or beyond out_capacity are not written (FJ_ERR_OUTCAP).
hipError_t fj_launch_full_sweep(const FjChunkSet& build, const u64* bits, const u64* orig_vals, u32 row_ids, u64* out_keys, u64* out_vals,
                                u64 base, u64 out_capacity, unsigned long long* cursor, u32* err, hipStream_t s);
// global table: the build rows whose slot's bit in a.matched is zero (a.bk / a.bv / a.row_ids as for the probe)
hipError_t fj_launch_gt_full_sweep(const FjGtArgs& a, u64 base, u64 out_capacity, unsigned long long* cursor, u32* err, hipStream_t s);
