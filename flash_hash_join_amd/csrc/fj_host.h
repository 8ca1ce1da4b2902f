// fj_host.h -- host-side state shared by the translation units behind the C ABI (include/flashjoin.h):
//   fj_plan.hip   workspace, plans, the partition-pass state machine, the HBM-table form's scaffold, contexts, options, diagnostics
//   fj_joins.hip  one-shot joins (the reference's drivers, hash_join.cpp:315-594), emit, owner split, bloom export / prefilter
//   fj_prepared.hip  a build side prepared once and probed many times (FJ_ALGO_RETAIN_BUILD / FJ_ALGO_REUSE_BUILD)
//   fj_stream.hip joins whose relations arrive in pieces, the owner shuffle's pack / append side
//   fj_entry.hip  the algo word decoded once and the one refusal list of fj_join_device and fj_join_host (fj_entry.h: not included here)
//   fj_hostentry.hip  the NumPy (host-buffer) entry
// (one file, fj_api.hip, until round 4).
#pragma once
#include "fj_internal.h"
#include "../../include/flashjoin.h"
#include "../../include/flashjoin_lab.h"

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

struct StreamState;

namespace fjh {

int set_err(const char* fmt, ...);
fj_timings& last_timings();               // thread-local: what fj_last_timings() returns
#define HIPCHK(x)                                                                                          \
    do {                                                                                                   \
        hipError_t e_ = (x);                                                                               \
        if (e_ != hipSuccess) return fjh::set_err("%s:%d: %s failed: %s", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
    } while (0)

struct DeviceGuard {
    int prev = -1; bool changed = false; hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) { err = hipSetDevice(dev); changed = err == hipSuccess; }
    }
    ~DeviceGuard() { if (changed) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define FJ_ON_DEVICE(dev)                                                                                   \
    fjh::DeviceGuard dev_guard_(dev);                                                                            \
    if (dev_guard_.err != hipSuccess) return fjh::set_err("selecting HIP device %d failed: %s", (int)(dev), hipGetErrorString(dev_guard_.err))
// Entry of a C-ABI call on context c: a null context is refused; calls on one context are serialised (the workspace, the scratch
// words and the events are per context; fj_join_host re-enters through fj_join_device / fj_stream_*: a recursive lock), then the
// device guard.  What the call reads or writes of the context's state comes after it.
#define FJ_ENTER(c)                                                                                         \
    if (!(c)) return fjh::set_err("%s: null context", __func__);                                             \
    std::lock_guard<std::recursive_mutex> ctx_lock_((c)->mu);                                                \
    FJ_ON_DEVICE((c)->device)

struct Scalars {                       // device scratch words, mirrored in pinned host memory
    unsigned long long total;
    unsigned long long expected;
    u64 empty_val;
    u32 err;
    u32 flags;
    u32 alloc[8];                      // [side*4 + pass] chunk allocators ([side*4 + 3]: the bloom stage's output pool)
    u32 seg_counter[8];                // [side*4 + pass] segment ids
    unsigned long long bloom_survivors;   // probe keys that passed the bloom precheck
    unsigned long long sample_hits;       // sampled probe rows found in the build side (adaptive bloom decision)
    u32 next_item;                     // work counter of the persistent join kernel
    u32 next_emit_item;                // ... and of the persistent emitting kernel (zeroed right before its launch)
    unsigned long long owner_counts[64], owner_cursors[64], owner_offsets[64];
    // owner shuffle, sender side (fj_shuffle_pack_*: runs while a stream join is open and on another stream, so it has words of
    // its own, outside what clear_plan_scalars and the plan's error handling touch)
    u32 pack_alloc, pack_seg, pack_err, rx_alloc;   // chunk allocator / segment counter / error word of the packing pass; chunk count of a received piece
    unsigned long long pack_used[64];  // wire-format chunks per owner GPU (fj_pack_offsets)
    unsigned long long pack_kept;      // probe keys a piece kept after the sender-side precheck (fj_part_filter_inplace) / passing keys of a sample
    u32 pack_xcd[8 * FJ_PF_COUNTERS];  // ... and its per-XCD work counters (directly behind pack_kept: one memset clears both)
    u32 bc_bounds[20];                 // build broadcast (fj_bcast_pack): key index at which piece q of the rank's region starts
};

enum Slot {
    // [side][pingpong][kind]
    W_POOL_K = 0, W_POOL_V, W_DIR, W_LIST, W_BCHUNKS, W_REL, W_BOFF, W_SEGOFF, W_TOFF, W_TILES, W_KINDS,
    W_SIDE_STRIDE = 2 * W_KINDS,                 // sides: 0 = build relation, 1 = probe relation, 2 = the owner shuffle's packing pass
    W_PART_COUNT = 3 * W_SIDE_STRIDE, W_OUT_OFF, W_GT_KEYS, W_GT_VALS, W_GT_BLOOM, W_WG_COUNT,
    W_H_BK, W_H_BV, W_H_PK, W_H_OK, W_H_OV, W_ROWIDX, W_BKEYS, W_BBASE,
    W_PK_FI, W_PK_BKEYS, W_PK_OBASE,                                   // fj_shuffle_pack_*: output-chunk index, keys per bucket, output chunks before a bucket
    W_RX_REL, W_RX_LIST, W_RX_SEGOFF, W_RX_BCH, W_RX_BOFF, W_RX_TOFF, W_RX_TILES,   // a received piece as a chunk set
    W_SK_TILES_B, W_SK_TILES_P, W_SK_NT, W_PART_COUNT2, W_OUT_OFF2,                 // re-partitioning of oversized final partitions (skew_join)
    W_MM_TILES,                                                                     // many-to-many join, option "mm_heavy_keys": the (probe item, build tile) items of oversized partitions (their counts and offsets: W_PART_COUNT2, W_OUT_OFF2)
                                                                                    // ... option "mm_heavy_outer": W_PART_COUNT2 and W_OUT_OFF2 hold the first set's misses, so one buffer here carries the tiles, the oversized
                                                                                    // probe items, both sets' counts and both sets' offsets (mm_tile_join)
    W_MM_PBITS,                                                                     // ... option "mm_heavy_outer": "found a partner in some tile" bits of the probe rows (one per row of the probe side's final chunk pool)
    W_FULL_BITS,                                                                    // full outer join: matched bits of the build rows / of the global table's slots
    W_PAIR_WORDS,                                                                   // FJ_ALGO_KEY_PAIR: the nb combined words of the two key columns, the input of the relation's passes (fj_groupby_pair.hip)
    W_GR_PART, W_GR_BASE,                                                           // FJ_ALGO_GROUP_ROWS: groups and rows per final partition; their exclusive scans (the HBM form: per tile of table slots) (fj_groupby_rows.hip)
    W_NSLOTS
};

struct Buf { void* p = nullptr; size_t bytes = 0; };

enum Ev { E_START = 0, E_BUILD, E_PPART, E_JOIN, E_EMIT0, E_EMIT1, E_SB0, E_SB1, E_BF0, E_BF1, E_H0, E_H1, E_H2, E_PK0, E_NEV = E_PK0 + 8 };

// the regions of a build-broadcast step (csrc/fj_bcast.hip): source i's region of nkeys[i] keys starts off[i] bytes into base
struct BcastSources { const void* base = nullptr; int n = 0; uint64_t off[FJ_WIDE_MAXSRC] = {}, nkeys[FJ_WIDE_MAXSRC] = {}; };

// The one record of a materialising join that was counted and whose pairs fj_emit_pairs has not written yet (emit_pending consumes
// it; begin_step drops it: what it points at is about to be overwritten)
struct Pending {
    enum Kind { LDS, HBM_TABLE, MANY, BCAST };
    bool valid = false;
    Kind kind = LDS;
    FjLdsJoinArgs lds{};                 // LDS, MANY; BCAST: the probe partitions, items and per-item counts of the step
    FjGtArgs gt{};
    u32 nitems = 0, gt_grid = 0;
    u64 count = 0;
    // oversized partitions that skew_join re-partitioned: their sub-partitions are a second item set, emitted behind the first
    // (MANY, inner form under the option "mm_heavy_keys": the (probe item, build tile) items of partitions beyond 4096 build rows are
    //  the second set - has_second, lds2, nitems2, count_main; the flagged items' counts are zeroed when the set is made)
    bool has_second = false; FjLdsJoinArgs lds2{}; u32 nitems2 = 0; u64 count_main = 0; std::vector<u32> flagged;
    bool dups_main = false; std::vector<u32> sk_parts; int sk_bits = 0, sk_plan_bits = 0, sk_npass = 0;     // ... which partitions, by how many more bits (the first-occurrence emit path repeats it with row indices)
    // MANY, outer forms (FJ_ALGO_ALL_COPIES; mm_outer != FJ_MM_INNER): `count` is P + u + r; the emit scans the misses per item too, writes
    // them behind the P pairs and - mm_r > 0 - sweeps the build rows the counting pass left unmarked in mm.bits behind those
    int mm_outer = 0; FjMmOuterArgs mm{}; u64 mm_P = 0, mm_u = 0, mm_r = 0;
    // ... under the option "mm_heavy_outer" with a partition beyond 4096 build rows (has_second, lds2, nitems2, count_main as for the inner
    // form: the tiles' pairs follow the first set's, written by the inner tile kernel): the oversized probe items are a third item set, mm_sweep,
    // whose rows without a partner in ANY tile fj_launch_mm_miss_sweep counted and writes.  The two sets share the range [P, P + u) in
    // this order: the first set's mm_u_main misses at P + miss_off[item] (its emitting launch skips the oversized items: both their
    // counts are 0), the sweep's behind them at P + mm_u_main + mm_sweep_off[item].  mm_tile_off / mm_sweep_off: where the emit scans
    // the second and third sets' counts to (W_OUT_OFF2 holds the first set's miss offsets)
    FjMmSweepArgs mm_sweep{}; u64 mm_u_main = 0; u64* mm_tile_off = nullptr; u64* mm_sweep_off = nullptr;
    bool mm_trivial = false; const u64* mm_pk = nullptr;        // ... one side was empty: no partitions, the emit copies the other side's rows (bk / bv below, mm_pk)
    // duplicate build keys seen by the counting pass: the emitting pass must pick the FIRST occurrence's value
    bool has_dups = false;
    const u64* bk = nullptr; const u64* bv = nullptr; size_t nb = 0; int top_bits = 64;
    // BCAST: the regions the step was counted against (they stay where they are), the first item of every partition, the plan's total build side
    BcastSources src; const u32* toff = nullptr; size_t nb_total = 0;
};

// caller-provided output buffers large enough for ANY result (>= probe rows): the materialising join may run in one pass
struct SingleOut { u64* keys = nullptr; u64* vals = nullptr; size_t cap = 0; bool done = false; };

// bloom_level: 0 = no bloom precheck; L >= 1 = the probe side's level-L chunk set (output of its L-th pass) is filtered
// against per-bucket Bloom filters of the build side's level L before pass L+1 (csrc/fj_bloom.hip)
struct Plan { int bits = 0, npass = 0; int fan_log[4] = {0, 0, 0, 0}; int bloom_level = 0; };

// The build side that FJ_ALGO_RETAIN_BUILD left on the context for FJ_ALGO_REUSE_BUILD (csrc/fj_prepared.hip): at most one, in device
// memory of its own (hipMalloc, not a workspace slot: fj_ctx_trim and fj_ctx_workspace_bytes do not see it), freed when it is replaced
// and by fj_ctx_destroy.  Not the pending result: begin_step leaves it alone
struct Prepared {
    enum Form { EMPTY, LDS, HBM };       // no build rows / runs per final partition for the LDS table / the global table
    bool valid = false;
    Form form = EMPTY;
    bool has_vals = false;               // prepared with d_build_vals (or empty): the value form may be asked for
    int top_bits = 64, path = 0;         // hash_top_bits of the plan; fj_timings::path of a probe against it
    Plan plan; u32 nparts = 0;           // LDS: the stored plan and its final partitions
    size_t nb = 0; u64 g = 0;            // build rows, distinct keys
    // LDS: g mixed keys, first positions and values (nb rows allocated each), aux = nparts FjPrepRun records
    // HBM: the table's key and first-position planes (cap_mask + 1 slots each), vals = a copy of the nb values, aux = the table's
    //      flag word and, 8 bytes in, the empty key's first position
    u64* keys = nullptr; u64* rows = nullptr; u64* vals = nullptr; void* aux = nullptr;
    u64 cap_mask = 0;
    size_t bytes = 0;                    // device memory held
};

// iteration state over the plan's passes for one relation (see pass_prepare / pass_launch / pass_complete)
struct PassIter {
    int side = 0; bool has_vals = false; size_t n = 0; Plan plan; int used = 64; u32 parents = 1; u64 lbound = 0;
    u32 tile_chunks = 16; int i = 0;
    FjChunkSet prev{}; bool have_prev = false; const uint4* tiles = nullptr; const u32* ntiles = nullptr; const u32* toff = nullptr;
    FjChunkSet cs{}; u32 Gmax = 1, F = 1, appends = 1;
    size_t piece_rows = 0;               // > 0: no single append of the first pass brings more rows than this (sizes the per-append slack)
    int slot = 0, cs_base = 0;           // ping-pong workspace slot of the next output level / base index of cs's buffers
    // probe side of a join: the final level's consumer is the join kernel; its item table (tiles of the final probe chunk
    // lists) and per-item count array are produced by the final level's bookkeeping launches
    u32 item_tc_max = 0;                 // > 0: the join's items hold at most this many probe chunks (32: the 16384-slot counting kernel will run, fj_join_wide.hip)
    bool want_items = false; u32 items_cap = 0; u32* part_count = nullptr; int part_count_slot = W_PART_COUNT;
    // bloom precheck (probe side): run the filter stage once `bloom_level` passes are complete, against bloom_build
    bool bloom_done = false; const FjChunkSet* bloom_build = nullptr;
    const u32* bloom_prebuilt = nullptr;            // filters shipped by another GPU (sender-side precheck) instead of bloom_build's keys
    unsigned long long* bloom_bucket_keys = nullptr; // [buckets] survivors per bucket (for flattening the survivors)
    // build side: keep a copy of the level the probe side's filter will read
    int save_level = 0; FjChunkSet saved{};
    // scalars of the pass when they are not the plan's (the owner shuffle's packing pass runs beside an open stream join)
    u32* alloc_word = nullptr; u32* seg_word = nullptr; u32* err_word = nullptr;
    // the previous level arrived from other GPUs in the 7-byte wire format (FjPartArgs::in_pk7)
    bool in_pk7 = false; u32 in_b0 = 0, in_top_shift = 0;
    // has_vals with a flat first input and no value array: the first pass makes the rows' positions (FjPartArgs::vals_pos)
    bool vals_pos = false;
};

}  // namespace fjh

struct PackState {              // fj_shuffle_pack_begin .. _finish: one piece on its way into the wire format
    bool begun = false, deferred = false;      // deferred: the first pass is queued, fj_shuffle_pack_filter queues the rest
    u32 part_shift = 0;                        // mixed key >> part_shift = final partition of the global plan
    fjh::PassIter it;
    FjPackArgs args{};
    int nranks = 0;
};

struct StreamState {            // fj_stream_*: a counting join whose relations arrive in pieces
    bool active = false;
    fjh::Plan plan; fjh::PassIter pit, bit; FjLdsJoinArgs ja{};
    int top_bits = 64, evc = 0;
    size_t np_bound = 0, np_seen = 0, nb_bound = 0, nb_seen = 0;
    u32 p_appends_left = 0, b_appends_left = 0;
    bool probe_done = false, build_done = false;
    // zero-pass plans (build side <= one LDS table): the pieces are joined as flat arrays
    const u64* flat_build = nullptr;
    const u64* flat_probe[64]; size_t flat_np[64]; u32 nflat = 0;
    // every piece appended so far (they stay allocated until fj_stream_finish returns): what the HBM-table fallback reads
    std::vector<std::pair<const u64*, size_t>> bpieces, ppieces;
    // owner shuffle, receiver side (fj_stream_open_shuffled): the pieces are chunk pools that peers filled with the FIRST pass of
    // the global plan; this rank owns level-1 buckets [b_lo, b_lo + nbk) and runs the plan from its second pass on
    bool shuffled = false; u32 b_lo = 0, nbk = 0, nbk_pad = 0;
    bool probe_prepared = true; u32 probe_appends = 0;      // shuffled: the probe side's pools are sized when its first piece is seen (an owner of hot probe keys receives far more than the mean)
    bool with_vals = false;         // ... and the build side carries values: a materialising join (pairs stay with the owner: fj_emit_pairs after the finish)
};

struct BcastState {             // fj_bcast_*: one step of the multi-GPU build-broadcast join on this rank (csrc/fj_bcast.hip)
    bool packed = false, probed = false;
    size_t nb_total = 0, nb = 0, np = 0;
    int pieces = 1, evc = 0;
    fjh::Plan plan; fjh::PassIter pit; FjLdsJoinArgs ja{};
    // a materialising step (the regions carry the build values): counted by fj_bcast_join against `src`; fj_bcast_finish hands
    // what the pairs need to the context's pending slot, and fj_emit_pairs writes them
    bool with_vals = false;
    fjh::BcastSources src;
};

struct fj_ctx {
    int device = 0;
    fjh::Buf bufs[fjh::W_NSLOTS];
    hipEvent_t ev[fjh::E_NEV];
    hipStream_t side = nullptr;        // copy stream of the host-buffer entry (fj_join_host)
    fjh::Scalars* d_sc = nullptr;
    fjh::Scalars* h_sc = nullptr;
    fjh::Pending pend;
    fjh::Prepared prep;                // the prepared build side (FJ_ALGO_RETAIN_BUILD), if any
    StreamState st;
    PackState pk;
    BcastState bc;
    hipEvent_t pk_ev = nullptr;        // the packing pass's counts have landed in pk_h
    unsigned long long* pk_h = nullptr;   // pinned: [64] chunks per owner, [64] = the pass's error word, [65] = keys kept by the precheck, [66] = sample result
    size_t ws_bytes = 0;
    u32 num_cus = 256;
    u32 reserve_cus = 0;               // CUs the partition passes leave free (set by the multi-GPU driver while RCCL's kernels share the GPU: fj_ctx_reserve_cus)
    void* stage[3] = {nullptr, nullptr, nullptr};     // pinned staging ring of the host-buffer entry (fj_join_host)
    size_t stage_bytes = 0;
    bool plan_in_flight = false;       // a plan was begun and has not completed (an error in between leaves chunk counts behind)
    bool slot_dirty[fjh::W_NSLOTS] = {};    // ... in which case every self-cleaning buffer is re-zeroed IN FULL before its next use (get_zeroed_buf)
    std::recursive_mutex mu;           // one C-ABI call at a time per context (FJ_ENTER)
};

namespace fjh {

// Process-wide dispatch options (fj_set_option; initial values from the environment).
//   radix_threshold  : adaptive joins take the non-partitioned HBM table below this many build rows.  MI355X: the
//                      partitioned driver wins at every build size (<= 4096 rows it runs zero passes: one LDS table per
//                      workgroup over the flat inputs), so the switch point is 0 (tools/sweep_adaptive.py).
//   (schedule: build relation first, then the probe relation, on the caller's stream.  The two-stream and interleaved
//    schedules of rounds 1-2 were measured slower once the level bookkeeping was fused - EXPERIMENTS.md - and are gone.)
//   mm_heavy_keys / mm_heavy_outer : a final partition of more than 4096 build rows in a many-to-many join - inner form / all-copies
//                      outer forms: 0 (default) refused, 1 joined in tiles (join_many, mm_tile_join).  Independent of each other; two
//                      options only because the outer forms' refusal at mm_heavy_keys = 1 is pinned behaviour.
//   persistent_min_items : counting joins with at least this many (partition, slice) items run the persistent join
//                      kernel (resident workgroups that prefetch the next item); below it one workgroup per item.
//   scalar_hbm_table : 1 = the reference's "scalar" functions (hash_join*, one table for the whole build side) use the
//                      non-partitioned HBM table at every size; 0 (default) = they use it only as the fallback and
//                      otherwise run the partitioned plan.  One table for B rows means one cache-missing 64-B access
//                      per probe in HBM -- more traffic than the 40 B per probe the two streaming passes + LDS join
//                      move -- so on this machine "scalar" is the slower way to the same result at every size.
// test / measurement hooks, one bit each in the option "lab_hooks" (fj_set_option; nothing reads the environment for them):
#define FJ_HOOK_LOOPBACK 1        // multi-GPU driver: a rank's own share travels through ncclSend / ncclRecv too (the code path every peer's share takes at N > 1)
#define FJ_HOOK_INJECT_FAIL 2     // multi-GPU driver: this rank's probe-side appends fail (agreed failures, reruns)
#define FJ_HOOK_SPLIT_ALWAYS 4    // a 1-rank communicator gets its own control communicator too
#define FJ_HOOK_ONE_COMM 8        // control collectives on the data communicator
#define FJ_HOOK_RESERVE_ALWAYS 16 // the CU reserve of an N > 1 step on one rank too (measurement)
#define FJ_HOOK_EMIT_TAGGED 32    // emitting pass on the tagged-table kernel (A/B)
#define FJ_HOOK_EMIT_RETRY_7TH 64 // every 7th item of the cuckoo emit kernel takes its retry path (results exact)
struct Options {
    size_t radix_threshold = 0; int scalar_hbm_table = 0; u32 persistent_min_items = 8192; u32 plan_target_keys = FJ_PART_TARGET_KEYS;
    int bloom_variant = 0, bloom_auto = 1, bloom_auto_max_hit_bp = 2300, mat_single_pass = 1;     // (2300: measured break-even at c4 sizes is 24 % hits, profiles/r03_bloom_threshold.csv)
    int join_wide = 2;                 // counting joins on the bucketed 16384-slot table (fj_join_wide.hip): 0 never, 1 whenever eligible, 2 (default) when at most ~3 probe rows per build row reach the join (wide_join_planned)
    u32 lab_hooks = 0;                 // FJ_HOOK_* bits
    u32 join_items_target = 2048;      // work items the join of a plan with few partitions is cut into (tuning knob)
    int mm_heavy_keys = 0;             // many-to-many inner join: 0 (default) a final partition of more than 4096 build rows is refused; 1 it is joined in tiles of <= 4096 build rows (join_many, fj_mm_tile_kernel).  The outer forms (FJ_ALGO_ALL_COPIES) refuse either way
    int mm_heavy_outer = 0;            // the same for the all-copies outer forms (FJ_ALGO_ALL_COPIES with LEFT_OUTER / FULL_OUTER): 0 (default) refused, 1 joined in tiles, the probe rows' "no partner" verdicts combined across the tiles (mm_tile_join, fj_mm_miss_sweep_kernel).  Independent of mm_heavy_keys; two options only because tests pin the outer forms' refusal at mm_heavy_keys = 1
    Options();                         // initial values: FJ_OPTIONS="name=value,name=value" (the names of fj_set_option), the ONE environment variable behind all of them
};
Options& options();

// ---- workspace and plans (fj_plan.hip) ----
int get_buf(fj_ctx* c, int slot, size_t bytes, void** out);
int get_zeroed_buf(fj_ctx* c, int slot, size_t bytes, void** out, hipStream_t s);
int plan_npass(int bits);
void plan_passes(Plan& p, bool extra_first);
Plan make_plan(size_t nb, int top_bits, bool want_bloom = false, u64 target_override = 0);
void pass_init(PassIter& it, int side, bool has_vals, size_t n, const Plan& plan, int top_bits);
u32 pass_groups(u64 chunks, u64 rows, u32 tile_chunks, u32 F);
int pass_prepare(fj_ctx* c, PassIter& it, u32 appends, hipStream_t s);
int pass_launch(fj_ctx* c, PassIter& it, const u64* keys, const u64* vals, size_t n, hipStream_t s, int* ev_cursor);
bool bloom_stage_follows(const PassIter& it, int level);
void join_item_geometry(u64 nparts, size_t np, u64 chunk_bound, u32* tc, u64* max_items);
bool wide_join_planned(bool materialize, size_t nb, size_t np_eff, int bits);
int level_finish(fj_ctx* c, PassIter& it, bool final_level, hipStream_t s);
int pass_complete(fj_ctx* c, PassIter& it, hipStream_t s);
int bloom_stage(fj_ctx* c, PassIter& it, hipStream_t s);
int run_passes(fj_ctx* c, PassIter& it, const u64* keys, const u64* vals, hipStream_t s, FjChunkSet* out, int* ev_cursor);
int clear_plan_scalars(fj_ctx* c, hipStream_t s);
void begin_plan(fj_ctx* c);
void end_plan(fj_ctx* c);
void drop_pending(fj_ctx* c);
int begin_step(fj_ctx* c, const char* who);
int read_scalars(fj_ctx* c, hipStream_t s);
float ev_ms(fj_ctx* c, int a, int b);
void plan_timings(fj_ctx* c, const Plan& plan, u64 partitions, int evc, fj_timings* t);
int pool_error();                         // the one set_err of FJ_ERR_POOL behind a partition pass
int distinct_error();                     // ... and of a group-by that found more distinct keys than the relation has rows

// ---- the global-table form (one table in HBM for the whole build side, no partition passes) and the fallback onto it (fj_plan.hip;
// DESIGN.md section 5).  gt_capacity: the smallest power of two >= max(64, 2 * nb).  gt_grid: workgroups of 1024 threads over n rows or
// slots, 4096 at most, never 0.  gt_open takes W_GT_KEYS (and W_GT_VALS, val_words != 0), wires `a` to the context's scalars and nb,
// records E_START, clears the scalars up to `alloc` (the cursor starts at 0) and fills the key plane with 0xFF.  gt_close records E_JOIN,
// then gt_read: the scalars read back, gt_facts (path 1, no passes, one partition) and the intervals between E_START, E_BUILD, E_PPART
// and E_JOIN, which the form records.  gt_fallback runs `global_form` into fresh timings, adds the abandoned attempt's total_ms, sets
// fell_back, stores them in *t - also when the form fails; a failed call publishes no timings - and returns the form's code.
// kind_agg: the FJ_GJ_* form of an accumulator plane over a value column of that kind; -1 outside either range ----
enum ValueKind { KIND_UNSIGNED = 0, KIND_SIGNED = 1, KIND_FLOAT = 2 };          // uint64 / int64 / binary64 words: the `kind` of group_by_all, _arg, _merge
enum AggPlane { PLANE_COUNT = 0, PLANE_SUM = 1, PLANE_MIN = 2, PLANE_MAX = 3 };  // the order of the four output planes of FJ_ALGO_AGG_ALL
u64 gt_capacity(size_t nb);
inline u32 gt_grid(u64 n) { const u64 rounds = (n + 1023) / 1024; return (u32)(rounds < 4096 ? (rounds ? rounds : 1) : 4096); }
int gt_open(fj_ctx* c, size_t nb, size_t val_words, hipStream_t s, FjGtArgs* a, u64** vals);
void gt_facts(fj_timings* t);
int gt_read(fj_ctx* c, hipStream_t s, fj_timings* t);
int gt_close(fj_ctx* c, hipStream_t s, fj_timings* t);
template <class F> int gt_fallback(fj_timings* t, F&& global_form) {
    fj_timings t2; memset(&t2, 0, sizeof t2); t2.sampled_hit_bp = -1;
    const int rc = global_form(&t2);
    t2.total_ms += t->total_ms; t2.fell_back = 1; *t = t2;
    return rc;
}
int kind_agg(int kind, int plane);

// ---- the partitioned attempt on ONE relation (fj_groupby*.hip).  rel_open: make_plan (target: make_plan's override, 0 = none) ..
// E_PPART - the relation's passes, with `beside` travelling beside the keys (vals is read for REL_VALUES only).  It is rel_begin
// (make_plan .. clear_plan_scalars) + rel_passes (the passes .. E_PPART): a form whose input is made on the stream takes the two
// halves and launches in between, inside build_phase_ms (fj_groupby_pair*.hip).  rel_close: E_JOIN .. plan_timings behind the
// form's kernel, the pool check included; probe_phase_ms = join_ms (there is no second relation) ----
enum RelBeside { REL_KEYS_ONLY, REL_VALUES, REL_POSITIONS };      // nothing / the value column / the rows' positions, made by the first pass
struct RelAttempt { Plan plan; FjChunkSet rel{}; u32 nparts = 0; };
int rel_begin(fj_ctx* c, size_t n, int top_bits, u64 target, hipStream_t s, RelAttempt* r);
int rel_passes(fj_ctx* c, const u64* keys, RelBeside beside, const u64* vals, size_t n, int top_bits, hipStream_t s, RelAttempt* r);
int rel_open(fj_ctx* c, const u64* keys, RelBeside beside, const u64* vals, size_t n, int top_bits, u64 target, hipStream_t s,
             RelAttempt* r);
int rel_close(fj_ctx* c, const Plan& plan, u32 nparts, hipStream_t s, fj_timings* t);

// ---- the partitioned attempt on TWO relations (fj_aligned, fj_group, fj_outer, fj_prepared, join_many) ----
// pair_open: the caller's plan (make_plan; join_many's has a target of its own), then begin_plan .. E_PPART - the build relation's
//   passes with spec.build beside its keys, E_BUILD, the probe relation's with spec.probe and the join's item table, E_PPART.
// pair_open_probe_only: the probe half against a stored plan (fj_prepared.hip); E_BUILD stands right behind clear_plan_scalars and
//   a.build stays empty.
// pair_items: the join's work items - the probe side's item table, or slices of a flat probe side (a zero-pass plan) - into the four
//   fields of that name of the kernel's arguments.
// pair_close: E_JOIN, then pair_read: the scalars read back, the pool error returned BEFORE end_plan (plan_in_flight then stays set
//   and get_zeroed_buf re-zeroes), end_plan, plan_timings.  The caller tests FJ_ERR_LDS_FULL behind it - plan_timings first, so that
//   gt_fallback adds the abandoned attempt's total_ms.
// pair_rerun_build_with_row_ids: duplicate build keys - the build side once more with row indices as payload (W_ROWIDX); the
//   counters, `also` (a further scalar of the form, or null), the error word and the allocators are cleared, and the passes stand
//   between a begin_plan / end_plan of their own.  The caller sets orig_vals, launches again and closes AGAIN.
// Closing again (behind a rerun's relaunch; join_group: behind the count launch for P): the second pair_close / pair_read records
//   the second E_JOIN and reads back again; its end_plan finds the plan ended already, its pool check reads a bit the first close has
//   ruled out unless a rerun's passes raised it, and its plan_timings assigns every field anew - the first close's timings are
//   discarded, and the call reports the intervals up to the second E_JOIN.
// trivial_done: an empty side - E_START, fill(), E_JOIN, synchronise; *ms = the interval, which the caller assigns as its form
//   reports it.
struct PairSpec { RelBeside build, probe; };
struct PairAttempt { Plan plan; PassIter bit, pit; FjChunkSet build{}, probe{}; u32 nparts = 0; int evc = 0; };
int pair_open(fj_ctx* c, const Plan& plan, const PairSpec& spec, const u64* bk, const u64* bv, size_t nb, const u64* pk, const u64* pv,
              size_t np, int top_bits, hipStream_t s, PairAttempt* a);
int pair_open_probe_only(fj_ctx* c, const Plan& plan, int top_bits, RelBeside probe, const u64* pk, const u64* pv, size_t np,
                         hipStream_t s, PairAttempt* a);
void pair_items(const PairAttempt& a, size_t np, const uint4** items, const u32** nitems_dev, u32* items_cap, u32* nsplit);
int pair_read(fj_ctx* c, const PairAttempt& a, hipStream_t s, fj_timings* t);
int pair_close(fj_ctx* c, const PairAttempt& a, hipStream_t s, fj_timings* t);
int pair_rerun_build_with_row_ids(fj_ctx* c, PairAttempt* a, const u64* bk, size_t nb, int top_bits, unsigned long long* also,
                                  hipStream_t s);
template <class F> int trivial_done(fj_ctx* c, hipStream_t s, float* ms, F&& fill) {
    HIPCHK(hipEventRecord(c->ev[E_START], s));
    if (fill()) return 1;
    HIPCHK(hipEventRecord(c->ev[E_JOIN], s));
    HIPCHK(hipStreamSynchronize(s));
    *ms = ev_ms(c, E_START, E_JOIN);
    return 0;
}

// ---- one dispatch per enum: a runtime `agg` (FJ_GJ_COUNT .. FJ_GJ_LAST) or `kind` (ValueKind) handed to f as a compile-time constant,
// so that `for_agg(agg, [](auto A) { return kernel<FJ_V(A)>; })` names the instantiation to launch.  for_value_agg: the eight forms
// that read a value - FJ_GJ_COUNT takes FJ_GJ_SUM's, and no FJ_GJ_COUNT instantiation is made.  Out of range (the launchers refuse
// it first) falls where the chains `agg == FJ_GJ_COUNT ? kernel<FJ_GJ_COUNT> : ...` these replace let it fall: their last
// alternative ----
template <int V> using IntC = std::integral_constant<int, V>;
#define FJ_V(A) decltype(A)::value
template <class F> auto for_agg(int agg, F&& f) -> decltype(f(IntC<FJ_GJ_MIN_F>{})) {
    // KEEP THIS ORDER OF THE CASES (and the form in the return type: the first of them).  The compiler emits a kernel's instantiations
    // in the order in which they are named here, and this is the order the replaced chains gave (last alternative first); another
    // order computes the same and reorders the kernels in the device objects, which profiles/host_scaffold_device_objects.txt
    // compares byte for byte
    switch (agg) {
    case FJ_GJ_MIN_F: return f(IntC<FJ_GJ_MIN_F>{});
    default: return f(IntC<FJ_GJ_MAX_F>{});
    case FJ_GJ_SUM_F: return f(IntC<FJ_GJ_SUM_F>{});
    case FJ_GJ_MAX_S: return f(IntC<FJ_GJ_MAX_S>{});
    case FJ_GJ_MAX_U: return f(IntC<FJ_GJ_MAX_U>{});
    case FJ_GJ_MIN_S: return f(IntC<FJ_GJ_MIN_S>{});
    case FJ_GJ_MIN_U: return f(IntC<FJ_GJ_MIN_U>{});
    case FJ_GJ_SUM: return f(IntC<FJ_GJ_SUM>{});
    case FJ_GJ_COUNT: return f(IntC<FJ_GJ_COUNT>{});
    }
}
template <class F> auto for_value_agg(int agg, F&& f) -> decltype(f(IntC<FJ_GJ_MAX_F>{})) {
    // KEEP THIS ORDER OF THE CASES (for_agg says why)
    switch (agg) {
    case FJ_GJ_MAX_F: return f(IntC<FJ_GJ_MAX_F>{});
    default: return f(IntC<FJ_GJ_SUM>{});                   // (FJ_GJ_SUM itself, and FJ_GJ_COUNT)
    case FJ_GJ_MIN_F: return f(IntC<FJ_GJ_MIN_F>{});
    case FJ_GJ_SUM_F: return f(IntC<FJ_GJ_SUM_F>{});
    case FJ_GJ_MAX_S: return f(IntC<FJ_GJ_MAX_S>{});
    case FJ_GJ_MAX_U: return f(IntC<FJ_GJ_MAX_U>{});
    case FJ_GJ_MIN_S: return f(IntC<FJ_GJ_MIN_S>{});
    case FJ_GJ_MIN_U: return f(IntC<FJ_GJ_MIN_U>{});
    }
}
template <class F> auto for_kind(int kind, F&& f) -> decltype(f(IntC<KIND_SIGNED>{})) {      // (KEEP THIS ORDER too)
    return kind == KIND_SIGNED ? f(IntC<KIND_SIGNED>{}) : kind == KIND_FLOAT ? f(IntC<KIND_FLOAT>{}) : f(IntC<KIND_UNSIGNED>{});
}

int stamps_begin(unsigned long long** dbg, hipStream_t s);
int stamps_report(const char* label, const unsigned long long* dbg, u32 nitems, hipStream_t s);

// ---- one-shot joins (fj_joins.hip) ----
int emit_pending(fj_ctx* c, u64* d_ok, u64* d_ov, size_t cap, hipStream_t s, fj_timings* t);
int radix_join_tail(fj_ctx* c, int materialize, FjLdsJoinArgs& ja, const Plan& plan, size_t np, const PassIter& pit, hipStream_t s,
                    fj_timings* t, int evc, u64* out_count, bool* lds_full, int top_bits, SingleOut* so = nullptr);

// ---- left outer / anti joins (fj_outer.hip): mode FJ_OJ_LEFT or FJ_OJ_ANTI, materialising; outputs hold >= np rows ----
// rid: the row-id form (FJ_ALGO_ROW_IDS): probe positions in d_ok, first-occurrence build positions (~0: none) in d_ov
int join_outer(fj_ctx* c, int mode, bool use_radix, const u64* bk, const u64* bv, size_t nb, const u64* pk, size_t np, int top_bits,
               hipStream_t s, fj_timings* t, u64* out_count, u64* d_ok, u64* d_ov, bool rid = false);
// FJ_ALGO_FULL_OUTER: rows [0, np) as FJ_OJ_LEFT writes them, then the build rows without a probe partner; outputs hold >= np + nb
// rows; out_counts[0] = matched probe rows, out_counts[1] = unmatched build rows
int join_full(fj_ctx* c, bool use_radix, const u64* bk, const u64* bv, size_t nb, const u64* pk, size_t np, int top_bits,
              hipStream_t s, fj_timings* t, u64* out_counts, u64* d_ok, u64* d_ov, bool rid);

// ---- probe-order joins (fj_aligned.hip): FJ_ALGO_PROBE_ORDER; d_ov[i] (np words) and / or d_mask[i] (np bytes) for every probe row i,
// either may be null; *out_count = probe rows with a partner; rid: d_ov holds first-occurrence build positions (~0: none) ----
int join_probe_order(fj_ctx* c, bool use_radix, const u64* bk, const u64* bv, size_t nb, const u64* pk, size_t np, int top_bits,
                     hipStream_t s, fj_timings* t, u64* out_count, unsigned char* d_mask, u64* d_ov, bool rid);

// ---- prepared build side (fj_prepared.hip): FJ_ALGO_RETAIN_BUILD prepares bk / bv (null: keys only) under the plan the one-shot call
// would take now and leaves it on the context - on failure the caller calls prepared_free; prepared_probe is FJ_ALGO_REUSE_BUILD's
// probe side against it, outputs and count as join_probe_order's ----
void prepared_free(fj_ctx* c);
int prepared_retain(fj_ctx* c, bool use_radix, const u64* bk, const u64* bv, size_t nb, int top_bits, hipStream_t s, fj_timings* t);
int prepared_probe(fj_ctx* c, const u64* pk, size_t np, hipStream_t s, fj_timings* t, u64* out_count, unsigned char* d_mask, u64* d_ov, bool rid);
// FJ_ALGO_BUILD_ORDER | FJ_ALGO_REUSE_BUILD: the probe side aggregated onto the prepared side - d_cnt / d_val (prep.nb words each, either
// may be null) receive the counts / the aggregate `agg` (FJ_GJ_SUM or a min / max form) of pv at every key's FIRST build row; filled
// first unless `accumulate`; *out_count = probe rows with a partner
int prepared_group(fj_ctx* c, const u64* pk, const u64* pv, size_t np, hipStream_t s, fj_timings* t, u64* out_count, u64* d_cnt, u64* d_val,
                   int agg, bool accumulate);

// ---- build-order aggregate joins (fj_group.hip): FJ_ALGO_BUILD_ORDER; d_cnt[i] and / or d_sum[i] (nb words each) for every build row i,
// either may be null; pv: the probe side's value column (np words, read for d_sum only); agg: the aggregate d_sum receives, FJ_GJ_SUM or
// one of the four min / max forms (csrc/fj_internal.h); *out_count = P, the sum of all counts ----
int join_group(fj_ctx* c, bool use_radix, const u64* bk, size_t nb, const u64* pk, const u64* pv, size_t np, int top_bits,
               hipStream_t s, fj_timings* t, u64* out_count, u64* d_cnt, u64* d_sum, int agg);

// ---- group-by on one relation (fj_groupby.hip): FJ_ALGO_GROUP_BY; the g distinct keys of bk in d_ok and one aggregate per key in d_ov
// (null: the keys alone), cap_out >= nb rows each; d_ok == nullptr: g alone; agg: FJ_GJ_COUNT, FJ_GJ_SUM or a min / max form over bv;
// rid: the position of the key's first occurrence instead; inv (FJ_ALGO_INVERSE): d_ov receives nb words instead, every row's group id
// (its key's row in d_ok) at the row's position; *out_count = g ----
int group_by(fj_ctx* c, bool use_radix, const u64* bk, const u64* bv, size_t nb, int top_bits, hipStream_t s, fj_timings* t,
             u64* out_count, u64* d_ok, u64* d_ov, size_t cap_out, int agg, bool rid, bool inv = false);
// ... with FJ_ALGO_AGG_ALL (fj_groupby_multi.hip): d_ov is four planes of cap_out words - count, sum, min, max of bv; kind 0 / 1 / 2: bv
// holds uint64 / int64 / binary64; cap_out >= 1; g > cap_out fails after the device work with *out_count = g
int group_by_all(fj_ctx* c, bool use_radix, const u64* bk, const u64* bv, size_t nb, int top_bits, hipStream_t s, fj_timings* t,
                 u64* out_count, u64* d_ok, u64* d_ov, size_t cap_out, int kind);
// ... with FJ_ALGO_AGG_ARG (fj_groupby_arg.hip): d_ov is two planes of cap_out >= nb words - the smallest row index that holds the
// minimum (is_max: the maximum) of bv over the key's rows, and that extreme; kind as above
int group_by_arg(fj_ctx* c, bool use_radix, const u64* bk, const u64* bv, size_t nb, int top_bits, hipStream_t s, fj_timings* t,
                 u64* out_count, u64* d_ok, u64* d_ov, size_t cap_out, int kind, bool is_max);
// ... with FJ_ALGO_AGG_ALL | FJ_ALGO_AGG_MERGE (fj_groupby_merge.hip): bk holds nb PARTIAL rows and bv their four planes of nb words -
// count, sum, min, max; d_ov is four planes of cap_out words, the rows of one key combined; kind and cap_out as for group_by_all
int group_by_merge(fj_ctx* c, bool use_radix, const u64* bk, const u64* bv, size_t nb, int top_bits, hipStream_t s, fj_timings* t,
                   u64* out_count, u64* d_ok, u64* d_ov, size_t cap_out, int kind);

// ... with FJ_ALGO_INVERSE | FJ_ALGO_KEY_PAIR (fj_groupby_pair.hip): the key is the PAIR (ka[i], kb[i]); d_ov receives nb words, every row's
// group id at the row's position, and d_ok the g row indices of the groups' first occurrences; nb <= 2^40, cap_out >= nb
int group_by_pair(fj_ctx* c, bool use_radix, const u64* ka, const u64* kb, size_t nb, int top_bits, hipStream_t s, fj_timings* t,
                  u64* out_count, u64* d_ok, u64* d_ov, size_t cap_out);
// ... with FJ_ALGO_KEY_PAIR | FJ_ALGO_AGG_ALL (fj_groupby_pair_agg.hip): the key is the PAIR (ka[i], kb[i]) and kv the value column, nb
// words each (fj_join_device takes kv as d_probe_keys: the one group-by form with a third column); d_ok receives column A of the g
// groups and d_ov FIVE planes of cap_out words - column B, then count, sum, min, max of kv as group_by_all writes them; kind as above;
// nb <= 2^40, cap_out >= 1; g > cap_out fails after the device work with *out_count = g
int group_by_pair_agg(fj_ctx* c, bool use_radix, const u64* ka, const u64* kb, const u64* kv, size_t nb, int top_bits, hipStream_t s,
                      fj_timings* t, u64* out_count, u64* d_ok, u64* d_ov, size_t cap_out, int kind);

// ... with FJ_ALGO_GROUP_ROWS (fj_groupby_rows.hip): d_ov is two planes of cap_out >= nb words - the nb row indices in group order, and
// the first word of them that belongs to each of the g groups; nb <= 2^40
int group_rows(fj_ctx* c, bool use_radix, const u64* bk, size_t nb, int top_bits, hipStream_t s, fj_timings* t,
               u64* out_count, u64* d_ok, u64* d_ov, size_t cap_out);

// ---- streamed joins (fj_stream.hip) ----
int stream_open(fj_ctx* c, size_t nb_bound, int build_appends, size_t np_bound, int probe_appends, hipStream_t s, int top_bits,
                size_t probe_piece_rows = 0);
int stream_append_build(fj_ctx* c, const u64* d_bk, size_t n, hipStream_t s);
int stream_flush_build(fj_ctx* c, StreamState& st, hipStream_t s);
int stream_abort(fj_ctx* c);

// ---- build broadcast (fj_bcast.hip) ----
int bcast_emit_launch(fj_ctx* c, const Pending& pd, u64* d_ok, u64* d_ov, hipStream_t s);
void drop_bcast_result_in(fj_ctx* c, const void* p, size_t bytes);

// ---- host-buffer entry (fj_hostentry.hip) ----
fj_ctx*& host_ctx();                      // the internal context of fj_join_host (null before its first call)

}  // namespace fjh
