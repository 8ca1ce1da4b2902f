// fj_prepared.hip -- a PREPARED build side (an EXTENSION: FJ_ALGO_RETAIN_BUILD / FJ_ALGO_REUSE_BUILD, modifiers of FJ_ALGO_PROBE_ORDER,
// include/flashjoin.h): the build relation is partitioned and deduplicated to first occurrences ONCE, kept in device memory the context
// owns outside its slot workspace, and probed any number of times by the probe-order forms - one dictionary or dimension table under
// many batches: a foreign-key column arriving in morsels, id remapping per training step, an IN list applied to every partition.
//
// Layout of the partitioned form: three dense planes of one row per DISTINCT build key - the MIXED key, the position of its first
// occurrence and (when values were given) that row's value - in which every final partition of the plan owns one run [o, o + g_p), and
// one (o, g_p) record per partition.  fj_prep_build_kernel makes it: one workgroup per final partition streams the partition's rows
// (the build side went through its passes carrying row positions, PassIter::vals_pos) into the 8192-slot LDS table, the smallest
// position per key winning by the native 64-bit LDS atomic minimum, then reserves the run with ONE global atomic and sweeps the table
// into it by wave ballot - the one gather from the caller's values per distinct key happens here, once.  The mixed empty marker is an
// ordinary row of the run.
//
// fj_prep_probe_kernel is the one-shot kernel's probe phase (csrc/fj_aligned.hip: rounds of 8 rows per thread, the next round's loads
// requested before this round's stores, plain stores at the row's own position, hits and misses counted per wave) behind a table build
// that has nothing left to decide: the run's keys are distinct, so a coalesced load and one CAS per key place them - no first-occurrence
// logic, no duplicate status, no overflow fallback.  The payload plane (values or positions) and the miss word (0 or ~0) are run-time
// arguments: three instantiations - payload, payload + mask, mask alone (a keys-only table).
//
// The HBM-table form (a partition beyond the LDS table when the side is prepared, scalar_hbm_table = 1, a build side below
// radix_threshold) needs no kernel of its own: the global table of fj_launch_gt_build_first in owned memory, beside an owned copy of
// the values and the table's two out-of-band words, probed by fj_launch_gt_probe_order.
//
// The aggregate join onto the prepared side (fj_prep_group_kernel, fj_prep_gt_group_kernel) takes the float aggregates too
// (FJ_ALGO_AGG_FLOAT: FJ_GJ_SUM_F / FJ_GJ_MIN_F / FJ_GJ_MAX_F, gj_combine in csrc/fj_group_dev.h): binary64 values and accumulators in the
// same words, combined in place into the call's - or the caller's running - float64 output, which must be device memory.
#include "fj_host.h"
#include "fj_group_dev.h"

namespace {

// the table of both kernels: the probe kernel loads what the build kernel accepted, so ONE limit serves both (the numbers are those of
// the one-shot probe-order kernel: 8192 slots, at most 7680 keys)
constexpr u32 PP_NT = GJ_NT, PP_KPT = GJ_KPT, PP_ROUND_CHUNKS = GJ_ROUND_CHUNKS, PP_TS = GJ_TS, PP_LIMIT = GJ_LIMIT;

struct PbHdr { u32 full, has_empty, nkeys, cursor; u64 empty_row, base; };      // 32 B: the key slots behind it stay 16-byte aligned

__global__ __launch_bounds__(PP_NT, 1) void fj_prep_build_kernel(FjPrepBuildArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    PbHdr* hdr = reinterpret_cast<PbHdr*>(smem);
    u64* tkeys = reinterpret_cast<u64*>(smem + sizeof(PbHdr));
    u64* trows = tkeys + PP_TS;
    const u32 tid = threadIdx.x, lane = tid & 63;
    const u32 p = blockIdx.x;
    u32 b0, nbc;
    fj_part_chunks(a.rel, p, b0, nbc);
    if (nbc == 0) return;                                    // (its record stays {0, 0}: the host cleared them)

    for (u32 i = tid; i < PP_TS; i += PP_NT) { tkeys[i] = FJ_EMPTY_KEY; trows[i] = ~0ull; }
    if (tid == 0) { hdr->full = 0; hdr->has_empty = 0; hdr->nkeys = 0; hdr->cursor = 0; hdr->empty_row = ~0ull; hdr->base = 0; }
    __syncthreads();

    // ---- stream: rounds of PP_NT * PP_KPT rows; the next round's loads are requested before this round's inserts.  No global store,
    // no barrier inside the loop ----
    u64 k[PP_KPT], rp[PP_KPT];
    u32 okm = 0;
    auto load_round = [&](u32 c0, u64 (&kk)[PP_KPT], u64 (&pp)[PP_KPT], u32& ok) {
        ok = 0;
#pragma unroll
        for (u32 u = 0; u < PP_KPT; ++u) {
            const u32 c = c0 + u * (PP_NT / FJ_CHUNK) + tid / FJ_CHUNK, off = tid % FJ_CHUNK;
            kk[u] = 0; pp[u] = 0;
            if (c >= nbc) continue;
            const u32 e = fj_chunk_entry(a.rel, b0 + c);
            if (off >= FJ_LIST_CNT(e)) continue;
            const u64 src = (u64)FJ_LIST_ID(e) * FJ_CHUNK + off;
            kk[u] = a.rel.keys[src];
            pp[u] = a.rel.vals ? a.rel.vals[src] : src;      // (zero-pass plan: the flat index IS the position)
            ok |= 1u << u;
        }
    };
    load_round(0, k, rp, okm);
    for (u32 c0 = 0; c0 < nbc; c0 += PP_ROUND_CHUNKS) {
        u64 kn[PP_KPT], rpn[PP_KPT];
        u32 okn = 0;
        if (c0 + PP_ROUND_CHUNKS < nbc) load_round(c0 + PP_ROUND_CHUNKS, kn, rpn, okn);
#pragma unroll
        for (u32 u = 0; u < PP_KPT; ++u) {
            if (!((okm >> u) & 1u)) continue;
            const u64 key = a.rel.list ? k[u] : fj_key_mix(k[u]);                 // chunk pools hold mixed keys, flat arrays raw ones
            if (key == FJ_EMPTY_KEY) {                       // the empty marker is never stored in the table
                hdr->has_empty = 1;
                atomicMin((unsigned long long*)&hdr->empty_row, (unsigned long long)rp[u]);
                continue;
            }
            if (*(volatile u32*)&hdr->full) continue;        // the partition is lost already: the rest of its rows do no table work
            u32 pos = FJ_HW2(key) & (PP_TS - 1);
            bool placed = false;
            for (u32 step = 0; step < PP_TS; ++step) {
                u64 t = tkeys[pos];                          // (a slot never changes once it holds a key: a stale read costs a CAS at most)
                if (t == FJ_EMPTY_KEY) {
                    t = atomicCAS((unsigned long long*)&tkeys[pos], (unsigned long long)FJ_EMPTY_KEY, (unsigned long long)key);
                    if (t == FJ_EMPTY_KEY) {
                        if (atomicAdd(&hdr->nkeys, 1u) >= PP_LIMIT) hdr->full = 1;
                        t = key;
                    }
                }
                if (t == key) { placed = true; break; }
                pos = (pos + 1) & (PP_TS - 1);
            }
            if (!placed) hdr->full = 1;
            else atomicMin((unsigned long long*)&trows[pos], (unsigned long long)rp[u]);
        }
#pragma unroll
        for (u32 u = 0; u < PP_KPT; ++u) { k[u] = kn[u]; rp[u] = rpn[u]; }
        okm = okn;
    }
    __syncthreads();
    if (hdr->full) { if (tid == 0) atomicOr(a.err, FJ_ERR_LDS_FULL); return; }     // nothing written: the host prepares the HBM-table form

    // ---- emit: one global atomic reserves the run [o, o + g_p); the table's occupied slots take ranks inside it, the marker key the last ----
    const u32 nk = hdr->nkeys;
    const bool has_empty = hdr->has_empty != 0;
    if (tid == 0) {
        const u32 gp = nk + (has_empty ? 1u : 0u);
        const u64 o0 = (u64)atomicAdd(a.cursor, (unsigned long long)gp);
        hdr->base = o0;
        FjPrepRun r; r.off = o0; r.n = gp;
        a.runs[p] = r;
    }
    __syncthreads();
    const u64 o = hdr->base;
    for (u32 i = tid; i < PP_TS; i += PP_NT) {               // (PP_TS is a multiple of PP_NT: whole waves every round)
        const u64 key = tkeys[i];
        const bool occ = key != FJ_EMPTY_KEY;
        const unsigned long long m = __ballot(occ);
        u32 wbase = 0;
        if (lane == 0 && m) wbase = atomicAdd(&hdr->cursor, (u32)__popcll(m));
        wbase = __shfl(wbase, 0, 64);
        if (!occ) continue;
        const u64 row = o + wbase + (u32)__popcll(m & ((1ull << lane) - 1ull));
        const u64 first = trows[i];
        if (row < a.out_capacity && first < a.nrows) {       // (always: g <= nb rows, positions are 0 .. nb - 1)
            a.out_keys[row] = key;
            a.out_rows[row] = first;
            if (a.orig_vals) a.out_vals[row] = a.orig_vals[first];
        } else atomicOr(a.err, FJ_ERR_OUTCAP);
    }
    if (tid == 0 && has_empty) {
        const u64 row = o + nk, first = hdr->empty_row;
        if (row < a.out_capacity && first < a.nrows) {
            a.out_keys[row] = FJ_EMPTY_KEY;
            a.out_rows[row] = first;
            if (a.orig_vals) a.out_vals[row] = a.orig_vals[first];
        } else atomicOr(a.err, FJ_ERR_OUTCAP);
    }
}

struct PqHdr { u32 bad, has_empty, hits, misses; u64 empty_val, pad; };

// PAYLOAD: a.plane (the values or the first-row positions) travels into the table and a.out_vals is written, a.miss_word for a row
//          without a partner (else the table holds keys only: the mask form)          MASK: a.mask is written
template <bool PAYLOAD, bool MASK>
__global__ __launch_bounds__(PP_NT, 1) void fj_prep_probe_kernel(FjPrepProbeArgs a) {
    static_assert(PAYLOAD || MASK, "an output");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    PqHdr* hdr = reinterpret_cast<PqHdr*>(smem);
    u64* tkeys = reinterpret_cast<u64*>(smem + sizeof(PqHdr));
    u64* tvals = tkeys + PP_TS;                               // (PAYLOAD only)
    const u32 tid = threadIdx.x, lane = tid & 63;
    const u32 item = blockIdx.x;
    // (fj_item_slice of csrc/fj_lds_table_dev.h, kept in place: the helper changes this kernel's code, and it is a hot one)
    u32 p, s_lo, s_hi;
    if (a.items) {
        if (item >= *a.nitems_dev) return;
        const uint4 it = a.items[item];
        p = it.z; s_lo = it.x; s_hi = it.x + it.y;
    } else {
        const u32 slice = item % a.nsplit;
        p = item / a.nsplit;
        const u32 npc = (u32)((a.probe.n_flat + FJ_CHUNK - 1) >> FJ_CHUNK_LOG);
        s_lo = (u32)(((u64)slice * npc) / a.nsplit); s_hi = (u32)(((u64)(slice + 1) * npc) / a.nsplit);
    }
    if (s_lo >= s_hi || p >= a.nparts) return;
    const FjPrepRun run = a.runs[p];
    if (run.n > PP_LIMIT + 1 || run.off + run.n > a.nkeys) {  // (uniform) not a run fj_prep_build_kernel wrote: nothing is loaded
        if (tid == 0) atomicOr(a.err, FJ_ERR_LDS_FULL);
        return;
    }

    for (u32 i = tid; i < PP_TS; i += PP_NT) tkeys[i] = FJ_EMPTY_KEY;
    if (tid == 0) { hdr->bad = 0; hdr->has_empty = 0; hdr->hits = 0; hdr->misses = 0; hdr->empty_val = a.miss_word; }
    __syncthreads();

    // ---- build: the partition's dense run, distinct keys: one coalesced load and one CAS each ----
    for (u32 i = tid; i < (u32)run.n; i += PP_NT) {
        const u64 key = a.keys[run.off + i];
        const u64 pay = PAYLOAD ? a.plane[run.off + i] : 0ull;
        if (key == FJ_EMPTY_KEY) {                           // the empty marker is never stored in the table
            hdr->has_empty = 1;
            if (PAYLOAD) hdr->empty_val = pay;
            continue;
        }
        u32 pos = FJ_HW2(key) & (PP_TS - 1);
        bool placed = false;
        for (u32 step = 0; step < PP_TS; ++step) {
            const u64 old = atomicCAS((unsigned long long*)&tkeys[pos], (unsigned long long)FJ_EMPTY_KEY, (unsigned long long)key);
            if (old == FJ_EMPTY_KEY) {
                if (PAYLOAD) tvals[pos] = pay;
                placed = true;
                break;
            }
            if (old == key) break;                           // (a key twice in a run: not a prepared side)
            pos = (pos + 1) & (PP_TS - 1);
        }
        if (!placed) hdr->bad = 1;
    }
    __syncthreads();
    if (hdr->bad) { if (tid == 0) atomicOr(a.err, FJ_ERR_LDS_FULL); return; }      // (an internal error on this path: there is no fallback)
    const bool has_empty = hdr->has_empty != 0;
    const u64 empty_val = hdr->empty_val;
    const u64 miss_word = a.miss_word;

    // ---- probe: rounds of PP_NT * PP_KPT rows; the next round's keys and positions are requested before this round's stores.
    // A row's result goes to the row's own position: no reservation of any kind ----
    u64 k[PP_KPT], rp[PP_KPT];
    u32 okm = 0, nh = 0, nm = 0;                             // nh / nm: wave-uniform counts of this wave's hits and misses
    auto load_round = [&](u32 pc, u64 (&kk)[PP_KPT], u64 (&pp)[PP_KPT], u32& ok) {
        ok = 0;
#pragma unroll
        for (u32 u = 0; u < PP_KPT; ++u) {
            const u32 c = pc + u * (PP_NT / FJ_CHUNK) + tid / FJ_CHUNK, off = tid % FJ_CHUNK;
            kk[u] = 0; pp[u] = 0;
            if (c >= s_hi) continue;
            const u32 e = fj_chunk_entry(a.probe, c);
            if (off >= FJ_LIST_CNT(e)) continue;
            const u64 src = (u64)FJ_LIST_ID(e) * FJ_CHUNK + off;
            kk[u] = a.probe.keys[src];
            pp[u] = a.probe.vals ? a.probe.vals[src] : src;  // (zero-pass plan: the flat index IS the position)
            ok |= 1u << u;
        }
    };
    load_round(s_lo, k, rp, okm);
    for (u32 pc = s_lo; pc < s_hi; pc += PP_ROUND_CHUNKS) {
        u64 v[PAYLOAD ? PP_KPT : 1];
        u32 hit = 0;
#pragma unroll
        for (u32 u = 0; u < PP_KPT; ++u) {
            if (PAYLOAD) v[PAYLOAD ? u : 0] = miss_word;
            const bool ok = (okm >> u) & 1u;
            bool h = false;
            if (ok) {
                const u64 key = a.probe.list ? k[u] : fj_key_mix(k[u]);
                if (key == FJ_EMPTY_KEY) { h = has_empty; if (PAYLOAD && h) v[PAYLOAD ? u : 0] = empty_val; }
                else {
                    u32 pos = FJ_HW2(key) & (PP_TS - 1);
                    for (;;) {                               // the run left >= 1/16 of the slots empty: always terminates
                        const u64 t = tkeys[pos];
                        if (t == key) { h = true; if (PAYLOAD) v[PAYLOAD ? u : 0] = tvals[pos]; break; }
                        if (t == FJ_EMPTY_KEY) break;
                        pos = (pos + 1) & (PP_TS - 1);
                    }
                }
            }
            if (h) hit |= 1u << u;
            nh += (u32)__popcll(__ballot(h)); nm += (u32)__popcll(__ballot(ok && !h));
        }
        u64 kn[PP_KPT], rpn[PP_KPT];
        u32 okn = 0;
        if (pc + PP_ROUND_CHUNKS < s_hi) load_round(pc + PP_ROUND_CHUNKS, kn, rpn, okn);
#pragma unroll
        for (u32 u = 0; u < PP_KPT; ++u) {
            if (!((okm >> u) & 1u)) continue;
            const u64 o = rp[u];
            if (o < a.np) {                                  // (always: positions are 0 .. np - 1; a row outside would be a pass's bug)
                if (PAYLOAD) a.out_vals[o] = v[PAYLOAD ? u : 0];
                if (MASK) a.mask[o] = (unsigned char)((hit >> u) & 1u);
            } else atomicOr(a.err, FJ_ERR_OUTCAP);
        }
#pragma unroll
        for (u32 u = 0; u < PP_KPT; ++u) { k[u] = kn[u]; rp[u] = rpn[u]; }
        okm = okn;
    }
    if (lane == 0) { if (nh) atomicAdd(&hdr->hits, nh); if (nm) atomicAdd(&hdr->misses, nm); }
    __syncthreads();
    if (tid == 0) {
        if (hdr->hits) atomicAdd(a.total, (unsigned long long)hdr->hits);
        if (hdr->misses) atomicAdd(a.miss_total, (unsigned long long)hdr->misses);
    }
}

struct PgHdr { u32 bad, has_empty, hits, rows; u64 empty_acc, flushed; };       // 32 B: the key slots behind it stay 16-byte aligned

// The build-order aggregate join (csrc/fj_group.hip) onto the prepared side: its probe phase behind the table build of the kernel above,
// one 8-byte accumulator per slot.  AGG (FJ_GJ_*): FJ_GJ_COUNT adds 1 per hit; every other form takes the probe rows' values
// (a.probe.vals) - FJ_GJ_SUM adds them, the four min / max forms combine them with gj_combine.  The flush reads the run once more -
// keys and first positions, coalesced - and combines every accumulator that left the identity into a.out[first position]: a partition
// may be cut into several items and a.out may hold a running aggregate, so it is always the global atomic (its result is unused).  The
// run's keys are distinct: the hits ARE the count, nothing like FJ_STAT_DUPS exists here.  They are counted as the one-shot kernel
// counts P - the count form adds up what it flushes (its accumulators are this call's counts), the forms with values one ballot per
// row - and the misses are the item's rows minus its hits, the rows one popcount of the round's mask per thread.
template <int AGG>
__global__ __launch_bounds__(PP_NT, 1) void fj_prep_group_kernel(FjPrepGroupArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    PgHdr* hdr = reinterpret_cast<PgHdr*>(smem);
    u64* tkeys = reinterpret_cast<u64*>(smem + sizeof(PgHdr));
    u64* acc = tkeys + PP_TS;
    constexpr bool VALS = AGG != FJ_GJ_COUNT;                 // the probe side carries values
    constexpr u64 IDENT = gj_identity<AGG>();
    const u32 tid = threadIdx.x, lane = tid & 63;
    const u32 item = blockIdx.x;
    // (fj_item_slice of csrc/fj_lds_table_dev.h, kept in place: the helper changes this kernel's code, and it is a hot one)
    u32 p, s_lo, s_hi;
    if (a.items) {
        if (item >= *a.nitems_dev) return;
        const uint4 it = a.items[item];
        p = it.z; s_lo = it.x; s_hi = it.x + it.y;
    } else {
        const u32 slice = item % a.nsplit;
        p = item / a.nsplit;
        const u32 npc = (u32)((a.probe.n_flat + FJ_CHUNK - 1) >> FJ_CHUNK_LOG);
        s_lo = (u32)(((u64)slice * npc) / a.nsplit); s_hi = (u32)(((u64)(slice + 1) * npc) / a.nsplit);
    }
    if (s_lo >= s_hi || p >= a.nparts) return;
    const FjPrepRun run = a.runs[p];
    if (run.n > PP_LIMIT + 1 || run.off + run.n > a.nkeys) {  // (uniform) not a run fj_prep_build_kernel wrote: nothing is loaded
        if (tid == 0) atomicOr(a.err, FJ_ERR_LDS_FULL);
        return;
    }

    for (u32 i = tid; i < PP_TS; i += PP_NT) { tkeys[i] = FJ_EMPTY_KEY; acc[i] = IDENT; }
    if (tid == 0) { hdr->bad = 0; hdr->has_empty = 0; hdr->hits = 0; hdr->rows = 0; hdr->empty_acc = IDENT; hdr->flushed = 0; }
    __syncthreads();

    // ---- build: the partition's dense run, distinct keys: one coalesced load and one CAS each; the empty marker stays out of band ----
    for (u32 i = tid; i < (u32)run.n; i += PP_NT) {
        const u64 key = a.keys[run.off + i];
        if (key == FJ_EMPTY_KEY) { hdr->has_empty = 1; continue; }
        u32 pos = FJ_HW2(key) & (PP_TS - 1);
        bool placed = false;
        for (u32 step = 0; step < PP_TS; ++step) {
            const u64 old = atomicCAS((unsigned long long*)&tkeys[pos], (unsigned long long)FJ_EMPTY_KEY, (unsigned long long)key);
            if (old == FJ_EMPTY_KEY) { placed = true; break; }
            if (old == key) break;                           // (a key twice in a run: not a prepared side)
            pos = (pos + 1) & (PP_TS - 1);
        }
        if (!placed) hdr->bad = 1;
    }
    __syncthreads();
    if (hdr->bad) { if (tid == 0) atomicOr(a.err, FJ_ERR_LDS_FULL); return; }      // (an internal error on this path: there is no fallback)
    const bool has_empty = hdr->has_empty != 0;

    // ---- probe: rounds of PP_NT * PP_KPT rows; the next round's loads are requested before this round's lookups.  A hit is one LDS
    // atomic on its slot's accumulator and nothing else: no global traffic ----
    u64 k[PP_KPT], pv[VALS ? PP_KPT : 1];
    u32 okm = 0, nh = 0, nrows = 0;                          // nh: wave-uniform count of this wave's hits (VALS); nrows: this thread's rows
    auto load_round = [&](u32 pc, u64 (&kk)[PP_KPT], u64 (&vv)[VALS ? PP_KPT : 1], u32& ok) {
        ok = 0;
#pragma unroll
        for (u32 u = 0; u < PP_KPT; ++u) {
            const u32 c = pc + u * (PP_NT / FJ_CHUNK) + tid / FJ_CHUNK, off = tid % FJ_CHUNK;
            kk[u] = 0; if (VALS) vv[VALS ? u : 0] = 0;
            if (c >= s_hi) continue;
            const u32 e = fj_chunk_entry(a.probe, c);
            if (off >= FJ_LIST_CNT(e)) continue;
            const u64 src = (u64)FJ_LIST_ID(e) * FJ_CHUNK + off;
            kk[u] = a.probe.keys[src];
            if (VALS) vv[VALS ? u : 0] = a.probe.vals[src];
            ok |= 1u << u;
        }
    };
    load_round(s_lo, k, pv, okm);
    for (u32 pc = s_lo; pc < s_hi; pc += PP_ROUND_CHUNKS) {
        u64 kn[PP_KPT], pvn[VALS ? PP_KPT : 1];
        u32 okn = 0;
        if (pc + PP_ROUND_CHUNKS < s_hi) load_round(pc + PP_ROUND_CHUNKS, kn, pvn, okn);
        nrows += (u32)__popc(okm);
#pragma unroll
        for (u32 u = 0; u < PP_KPT; ++u) {
            bool h = false;
            if ((okm >> u) & 1u) {
                const u64 key = a.probe.list ? k[u] : fj_key_mix(k[u]);           // chunk pools hold mixed keys, flat arrays raw ones
                const unsigned long long add = VALS ? (unsigned long long)pv[VALS ? u : 0] : 1ull;
                if (key == FJ_EMPTY_KEY) {
                    h = has_empty;
                    if (h) gj_combine<AGG>(&hdr->empty_acc, add);
                } else {
                    u32 pos = FJ_HW2(key) & (PP_TS - 1);
                    for (;;) {                               // the run left >= 1/16 of the slots empty: always terminates
                        const u64 t = tkeys[pos];
                        if (t == key) { h = true; gj_combine<AGG>(&acc[pos], add); break; }
                        if (t == FJ_EMPTY_KEY) break;
                        pos = (pos + 1) & (PP_TS - 1);
                    }
                }
            }
            if (VALS) nh += (u32)__popcll(__ballot(h));
        }
#pragma unroll
        for (u32 u = 0; u < PP_KPT; ++u) { k[u] = kn[u]; if (VALS) pv[VALS ? u : 0] = pvn[VALS ? u : 0]; }
        okm = okn;
    }
    const u32 wrows = (u32)gj_wave_sum64(nrows);
    if (lane == 0) { if (VALS && nh) atomicAdd(&hdr->hits, nh); if (wrows) atomicAdd(&hdr->rows, wrows); }
    __syncthreads();

    // ---- flush: the run once more, keys and first positions; a slot that still holds the identity has nothing to say (count, sum: 0
    // adds nothing; min / max: the identity changes no word) ----
    const u64 empty_acc = hdr->empty_acc;
    u64 flushed = 0;
    for (u32 i = tid; i < (u32)run.n; i += PP_NT) {
        const u64 key = a.keys[run.off + i];
        const u64 o = a.rows[run.off + i];
        u64 v = empty_acc;
        if (key != FJ_EMPTY_KEY) {
            u32 pos = FJ_HW2(key) & (PP_TS - 1);
            while (tkeys[pos] != key) pos = (pos + 1) & (PP_TS - 1);              // (the build phase placed it)
            v = acc[pos];
        }
        if (v == IDENT) continue;
        if (!VALS) flushed += v;
        if (o < a.nb) gj_combine<AGG>(&a.out[o], v);                              // (always: first positions are 0 .. nb - 1)
        else atomicOr(a.err, FJ_ERR_OUTCAP);
    }
    if (!a.total) return;                                    // (uniform: the other launch of a two-output call has them)
    if (!VALS) {
        flushed = gj_wave_sum64(flushed);
        if (lane == 0 && flushed) atomicAdd((unsigned long long*)&hdr->flushed, (unsigned long long)flushed);
        __syncthreads();
    }
    if (tid == 0) {
        const u64 hits = VALS ? (u64)hdr->hits : hdr->flushed, rows = hdr->rows;
        if (hits) atomicAdd(a.total, (unsigned long long)hits);
        if (rows > hits) atomicAdd(a.miss_total, (unsigned long long)(rows - hits));
    }
}

// the HBM-table form: thread i serves probe row i against the owned table (raw keys, the raw empty key out of band: its flag and first
// position in a.flags / a.empty_val); a hit goes straight to the output words of the key's first build row with the typed global
// atomic - no accumulators, no flush.  AGG is out_val's aggregate (FJ_GJ_SUM for the counts alone).  Global atomics serialise on a hot key
template <int AGG>
__global__ __launch_bounds__(1024) void fj_prep_gt_group_kernel(FjGtArgs a, const u64* __restrict__ pv, u64* out_cnt, u64* out_val, u64 nb,
                                                                unsigned long long* miss_total, u32* err) {
    __shared__ u32 s_hits, s_misses;
    const u32 tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) { s_hits = 0; s_misses = 0; }
    __syncthreads();
    const bool has_empty = a.flags[0] != 0;
    const u64 np = a.np;
    u32 nh = 0, nm = 0;                                                           // (wave-uniform)
    for (u64 base = (u64)blockIdx.x * 1024; base < np; base += (u64)gridDim.x * 1024) {     // (uniform per workgroup)
        const u64 i = base + tid;
        const bool ok = i < np;
        bool h = false;
        if (ok) {
            const u64 key = a.pk[i];
            u64 where = 0;
            if (key == FJ_EMPTY_KEY) h = has_empty;
            else h = gj_gt_find(a.tkeys, a.cap_mask, key, where);
            if (h) {
                const u64 o = key == FJ_EMPTY_KEY ? *a.empty_val : a.tvals[where];
                if (o < nb) {                                                     // (always: first positions are 0 .. nb - 1)
                    if (out_cnt) atomicAdd((unsigned long long*)&out_cnt[o], 1ull);
                    if (out_val) gj_combine<AGG>(&out_val[o], pv[i]);
                } else atomicOr(err, FJ_ERR_OUTCAP);
            }
        }
        nh += (u32)__popcll(__ballot(h)); nm += (u32)__popcll(__ballot(ok && !h));
    }
    if (lane == 0) { if (nh) atomicAdd(&s_hits, nh); if (nm) atomicAdd(&s_misses, nm); }
    __syncthreads();
    if (tid == 0) {
        if (s_hits) atomicAdd(a.total, (unsigned long long)s_hits);
        if (s_misses) atomicAdd(miss_total, (unsigned long long)s_misses);
    }
}

}  // namespace

hipError_t fj_launch_prep_build(const FjPrepBuildArgs& a, hipStream_t s) {
    if (!a.nparts || !a.cursor || !a.err || !a.runs || !a.out_keys || !a.out_rows || (a.orig_vals && !a.out_vals)) return hipErrorInvalidValue;
    const u32 lds = (u32)sizeof(PbHdr) + PP_TS * 16u;
    hipError_t e = fj_set_max_lds_once(reinterpret_cast<const void*>(fj_prep_build_kernel), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fj_prep_build_kernel, dim3(a.nparts), dim3(PP_NT), lds, s, a);
    return hipGetLastError();
}

hipError_t fj_launch_prep_probe(const FjPrepProbeArgs& a, hipStream_t s) {
    const u32 grid = a.items ? a.items_cap : a.nparts * a.nsplit;
    const bool payload = a.out_vals != nullptr;
    if (!a.total || !a.miss_total || !a.err || !a.runs || !a.keys || (!payload && !a.mask) || (payload && !a.plane)) return hipErrorInvalidValue;
    const u32 lds = (u32)sizeof(PqHdr) + PP_TS * (payload ? 16u : 8u);
    void (*kern)(FjPrepProbeArgs);
    if (!payload) kern = fj_prep_probe_kernel<false, true>;
    else kern = a.mask ? fj_prep_probe_kernel<true, true> : fj_prep_probe_kernel<true, false>;
    hipError_t e = fj_set_max_lds_once(reinterpret_cast<const void*>(kern), lds);
    if (e != hipSuccess) return e;
    if (grid) hipLaunchKernelGGL(kern, dim3(grid), dim3(PP_NT), lds, s, a);
    return hipGetLastError();
}

hipError_t fj_launch_prep_group(const FjPrepGroupArgs& a, int agg, hipStream_t s) {
    const u32 grid = a.items ? a.items_cap : a.nparts * a.nsplit;
    if (agg < FJ_GJ_COUNT || agg > FJ_GJ_LAST) return hipErrorInvalidValue;
    if (!a.err || !a.runs || !a.keys || !a.rows || !a.out || (a.total && !a.miss_total)) return hipErrorInvalidValue;
    if (agg != FJ_GJ_COUNT && !a.probe.vals) return hipErrorInvalidValue;         // the probe side carries the values
    const u32 lds = (u32)sizeof(PgHdr) + PP_TS * 16u;
    void (*kern)(FjPrepGroupArgs) = fjh::for_agg(agg, [](auto A) { return fj_prep_group_kernel<FJ_V(A)>; });
    hipError_t e = fj_set_max_lds_once(reinterpret_cast<const void*>(kern), lds);
    if (e != hipSuccess) return e;
    if (grid) hipLaunchKernelGGL(kern, dim3(grid), dim3(PP_NT), lds, s, a);
    return hipGetLastError();
}

hipError_t fj_launch_prep_gt_group(const FjGtArgs& a, int agg, const u64* pv, u64* out_cnt, u64* out_val, u64 nb,
                                   unsigned long long* miss_total, u32* err, hipStream_t s) {
    if (a.np == 0) return hipSuccess;
    if (!a.total || !miss_total || !err || !a.tkeys || !a.tvals || !a.flags || !a.empty_val || !a.pk) return hipErrorInvalidValue;
    if ((!out_cnt && !out_val) || (out_val && !pv)) return hipErrorInvalidValue;
    if (agg < FJ_GJ_COUNT || agg > FJ_GJ_LAST || (out_val && agg == FJ_GJ_COUNT)) return hipErrorInvalidValue;
    void (*kern)(FjGtArgs, const u64*, u64*, u64*, u64, unsigned long long*, u32*) =
        fjh::for_value_agg(agg, [](auto A) { return fj_prep_gt_group_kernel<FJ_V(A)>; });      // (the counts alone: out_val == nullptr)
    hipLaunchKernelGGL(kern, dim3(fjh::gt_grid(a.np)), dim3(1024), 0, s, a, pv, out_cnt, out_val, nb, miss_total, err);
    return hipGetLastError();
}

namespace fjh {

// what the context holds is given back (a replacement, a failed FJ_ALGO_RETAIN_BUILD, fj_ctx_destroy); hipFree waits for the device
void prepared_free(fj_ctx* c) {
    Prepared& P = c->prep;
    for (void* p : {(void*)P.keys, (void*)P.rows, (void*)P.vals, P.aux}) if (p) (void)hipFree(p);
    P = Prepared();
}

static int prep_alloc(Prepared& P, void** out, size_t bytes) {
    void* p = nullptr;
    const size_t want = bytes ? bytes : 16;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) return set_err("hipMalloc(%zu bytes) for the prepared build side failed: %s", want, hipGetErrorString(e));
    *out = p; P.bytes += want;
    return 0;
}

// the HBM-table form: the global table of first-occurrence positions (raw keys; the table's flag and the empty key's position in
// P.aux), an owned copy of the values beside it, g counted by the group-by's sweep of the table (cursor alone)
static int prepared_retain_global(fj_ctx* c, const u64* bk, const u64* bv, size_t nb, hipStream_t s) {
    Prepared& P = c->prep;
    const u64 cap = gt_capacity(nb);
    P.form = Prepared::HBM; P.cap_mask = cap - 1;
    if (prep_alloc(P, (void**)&P.keys, cap * 8) || prep_alloc(P, (void**)&P.rows, cap * 8) || prep_alloc(P, &P.aux, 16)) return 1;
    if (bv && prep_alloc(P, (void**)&P.vals, nb * 8)) return 1;
    FjGtArgs a{};
    a.tkeys = P.keys; a.tvals = P.rows; a.cap_mask = P.cap_mask; a.flags = (u32*)P.aux; a.empty_val = (u64*)P.aux + 1;
    a.bk = bk; a.nb = nb; a.total = &c->d_sc->total;
    HIPCHK(hipEventRecord(c->ev[E_START], s));
    HIPCHK(hipMemsetAsync(c->d_sc, 0, offsetof(Scalars, alloc), s));
    HIPCHK(hipMemsetAsync(P.aux, 0, 8, s));
    HIPCHK(hipMemsetAsync((u64*)P.aux + 1, 0xFF, 8, s));                          // (row index minimum)
    HIPCHK(hipMemsetAsync(P.keys, 0xFF, cap * 8, s));
    HIPCHK(hipMemsetAsync(P.rows, 0xFF, cap * 8, s));
    if (bv) HIPCHK(hipMemcpyAsync(P.vals, bv, nb * 8, hipMemcpyDeviceToDevice, s));
    HIPCHK(fj_launch_gt_build_first(a, true, s));
    HIPCHK(fj_launch_gt_group_by_sweep(a, nullptr, nullptr, nullptr, 0, &c->d_sc->total, &c->d_sc->err, s));
    HIPCHK(hipEventRecord(c->ev[E_BUILD], s));
    if (read_scalars(c, s)) return 1;
    P.g = c->h_sc->total;
    if (P.g == 0 || P.g > nb) return set_err("internal error: the prepared build side holds %llu distinct keys of %zu rows", (unsigned long long)P.g, nb);
    return 0;
}

// FJ_ALGO_RETAIN_BUILD (fj_join_device has checked the arguments): whatever the context held is freed, then bk[0 .. nb) - and bv, when
// given - is prepared under the plan that the one-shot call would run now.  t receives the plan's facts, the time in build_phase_ms
// = total_ms and fell_back = 1 when a partition was beyond the LDS table.  On failure the caller frees what is half made
int prepared_retain(fj_ctx* c, bool use_radix, const u64* bk, const u64* bv, size_t nb, int top_bits, hipStream_t s, fj_timings* t) {
    prepared_free(c);
    Prepared& P = c->prep;
    P.top_bits = top_bits; P.nb = nb; P.has_vals = bv != nullptr || nb == 0;      // (an empty side answers every form: no row has a partner)
    t->path = use_radix ? 0 : 1;
    if (nb == 0) { P.form = Prepared::EMPTY; P.path = t->path; P.valid = true; return 0; }
    if (use_radix) {
        const Plan plan = make_plan(nb, top_bits, false);
        begin_plan(c);
        HIPCHK(hipEventRecord(c->ev[E_START], s));
        if (clear_plan_scalars(c, s)) return 1;              // (total = the cursor of the runs)
        FjPrepBuildArgs ba{};
        PassIter bit;
        pass_init(bit, 0, true, nb, plan, top_bits);
        bit.vals_pos = true;                                 // the rows' positions travel through the passes
        if (run_passes(c, bit, bk, nullptr, s, &ba.rel, nullptr)) return 1;
        ba.nparts = ba.rel.list ? ba.rel.nb : 1u;
        P.form = Prepared::LDS; P.plan = plan; P.nparts = ba.nparts;
        if (prep_alloc(P, (void**)&P.keys, nb * 8) || prep_alloc(P, (void**)&P.rows, nb * 8) || prep_alloc(P, &P.aux, (size_t)ba.nparts * sizeof(FjPrepRun))) return 1;
        if (bv && prep_alloc(P, (void**)&P.vals, nb * 8)) return 1;
        HIPCHK(hipMemsetAsync(P.aux, 0, (size_t)ba.nparts * sizeof(FjPrepRun), s));
        ba.orig_vals = bv; ba.nrows = nb;
        ba.out_keys = P.keys; ba.out_rows = P.rows; ba.out_vals = P.vals; ba.out_capacity = nb;
        ba.runs = (FjPrepRun*)P.aux; ba.cursor = &c->d_sc->total; ba.err = &c->d_sc->err;
        HIPCHK(fj_launch_prep_build(ba, s));
        HIPCHK(hipEventRecord(c->ev[E_BUILD], s));
        if (read_scalars(c, s)) return 1;
        if (c->h_sc->err & FJ_ERR_POOL) return pool_error();
        end_plan(c);
        t->build_phase_ms = ev_ms(c, E_START, E_BUILD);
        if (!(c->h_sc->err & FJ_ERR_LDS_FULL)) {
            if (c->h_sc->err & FJ_ERR_OUTCAP) return set_err("internal error: the prepared build side found more distinct keys than the relation has rows");
            P.g = c->h_sc->total;
            if (P.g == 0 || P.g > nb) return set_err("internal error: the prepared build side holds %llu distinct keys of %zu rows", (unsigned long long)P.g, nb);
            t->passes = plan.npass; t->radix_bits = plan.bits; t->partitions = ba.nparts;
            t->total_ms = t->build_phase_ms;
            P.path = 0; P.valid = true;
            return 0;
        }
        // a partition beyond the LDS table: the side is prepared as the HBM table instead
        const int tb = P.top_bits; const bool hv = P.has_vals;
        prepared_free(c);
        P.top_bits = tb; P.nb = nb; P.has_vals = hv;
        t->fell_back = 1;
    }
    if (prepared_retain_global(c, bk, bv, nb, s)) return 1;
    gt_facts(t);
    t->build_phase_ms += ev_ms(c, E_START, E_BUILD);
    t->total_ms = t->build_phase_ms;
    P.path = 1; P.valid = true;
    return 0;
}

// the probe side of FJ_ALGO_REUSE_BUILD - and of FJ_ALGO_RETAIN_BUILD with np > 0, behind prepared_retain - against the context's
// prepared side: d_ov[i] (np words, may be null) and d_mask[i] (np bytes, may be null) for every probe row i, *out_count = probe rows
// with a partner.  rid: d_ov holds first-occurrence build positions (~0: none).  The stored plan decides; the context's workspace
// serves the probe side's passes only.  t: build_phase_ms = 0, the plan's facts those of the prepared side
int prepared_probe(fj_ctx* c, const u64* pk, size_t np, hipStream_t s, fj_timings* t, u64* out_count, unsigned char* d_mask, u64* d_ov, bool rid) {
    const Prepared& P = c->prep;
    const bool vals = d_ov != nullptr;
    if (!vals) rid = false;                                  // (the mask form reads no payload of either kind)
    *out_count = 0;
    t->path = P.path; t->passes = P.form == Prepared::LDS ? P.plan.npass : 0; t->radix_bits = P.form == Prepared::LDS ? P.plan.bits : 0;
    t->partitions = P.form == Prepared::LDS ? P.nparts : 1;
    t->build_phase_ms = 0;
    if (np == 0) return 0;
    if (P.form == Prepared::EMPTY) {                         // no probe row has a partner
        float ms;
        if (trivial_done(c, s, &ms, [&]() -> int {
                if (vals) HIPCHK(hipMemsetAsync(d_ov, rid ? 0xFF : 0, np * 8, s));
                if (d_mask) HIPCHK(hipMemsetAsync(d_mask, 0, np, s));
                return 0;
            })) return 1;
        t->total_ms = t->join_ms = t->probe_phase_ms = ms;
        return 0;
    }
    if (P.form == Prepared::HBM) {
        FjGtArgs a{};
        a.tkeys = P.keys; a.tvals = P.rows; a.cap_mask = P.cap_mask; a.flags = (u32*)P.aux; a.empty_val = (u64*)P.aux + 1;
        a.bv = (vals && !rid) ? P.vals : nullptr; a.nb = P.nb; a.pk = pk; a.np = np; a.total = &c->d_sc->total;
        a.out_vals = d_ov; a.row_ids = rid ? 1u : 0u;
        HIPCHK(hipEventRecord(c->ev[E_START], s));
        HIPCHK(hipMemsetAsync(c->d_sc, 0, offsetof(Scalars, alloc), s));
        HIPCHK(fj_launch_gt_probe_order(a, &c->d_sc->expected, d_mask, s));
        HIPCHK(hipEventRecord(c->ev[E_JOIN], s));
        if (read_scalars(c, s)) return 1;
        t->join_ms = t->probe_phase_ms = t->total_ms = ev_ms(c, E_START, E_JOIN);
    } else {
        // (total = the hits, expected = the misses; the probe rows' positions travel through the passes)
        PairAttempt a;
        if (pair_open_probe_only(c, P.plan, P.top_bits, REL_POSITIONS, pk, nullptr, np, s, &a)) return 1;
        FjPrepProbeArgs pa{};
        pa.probe = a.probe; pa.nparts = P.nparts;
        if (pa.probe.list && pa.probe.nb != P.nparts) return set_err("internal error: the probe side has %u partitions, the prepared build side %u", pa.probe.nb, P.nparts);
        if (!pa.probe.list && P.nparts != 1) return set_err("internal error: a flat probe side against %u prepared partitions", P.nparts);
        pair_items(a, np, &pa.items, &pa.nitems_dev, &pa.items_cap, &pa.nsplit);
        pa.keys = P.keys; pa.plane = vals ? (rid ? P.rows : P.vals) : nullptr; pa.runs = (const FjPrepRun*)P.aux; pa.nkeys = P.g;
        pa.miss_word = rid ? ~0ull : 0ull;
        pa.out_vals = d_ov; pa.mask = d_mask; pa.np = np;
        pa.total = &c->d_sc->total; pa.miss_total = &c->d_sc->expected; pa.err = &c->d_sc->err;
        HIPCHK(fj_launch_prep_probe(pa, s));
        if (pair_close(c, a, s, t)) return 1;
        t->build_phase_ms = 0;                               // (nothing touched the build relation: its passes ran when it was prepared)
        if (c->h_sc->err & FJ_ERR_LDS_FULL) return set_err("internal error: a run of the prepared build side does not fit the LDS table");
        if (c->h_sc->err & FJ_ERR_OUTCAP) return set_err("internal error: a probe row's position lies beyond the probe side");
    }
    const u64 hits = c->h_sc->total, misses = c->h_sc->expected;
    if (hits + misses != np) return set_err("internal error: probe-order join placed %llu + %llu of %zu probe rows", (unsigned long long)hits, (unsigned long long)misses, np);
    *out_count = hits;
    return 0;
}

// FJ_ALGO_BUILD_ORDER | FJ_ALGO_REUSE_BUILD (fj_join_device has checked the arguments, the prepared side and the capacity): the probe
// side aggregated onto the prepared side.  d_cnt / d_val: P.nb words each, either may be null; agg: what d_val receives (FJ_GJ_SUM or a
// min / max form); pv: the probe side's value column, read for d_val only.  A key's aggregate lands at its FIRST build row: the runs (the
// HBM table) hold first positions only, so every further copy of a duplicated key keeps what the fill - or, accumulating, the caller -
// left there.  Unless `accumulate`, the outputs are filled with the aggregate's identity on the stream first; with it they are combined
// into as they are.  Same shape as prepared_probe; the prepared planes are read and never written.  *out_count = probe rows with a partner
int prepared_group(fj_ctx* c, const u64* pk, const u64* pv, size_t np, hipStream_t s, fj_timings* t, u64* out_count, u64* d_cnt, u64* d_val,
                   int agg, bool accumulate) {
    const Prepared& P = c->prep;
    const size_t nb = P.nb;
    *out_count = 0;
    t->path = P.path; t->passes = P.form == Prepared::LDS ? P.plan.npass : 0; t->radix_bits = P.form == Prepared::LDS ? P.plan.bits : 0;
    t->partitions = P.form == Prepared::LDS ? P.nparts : 1;
    t->build_phase_ms = 0;
    if (P.form == Prepared::EMPTY || nb == 0) return 0;      // the outputs have zero words
    if (np == 0 && accumulate) return 0;                     // nothing to combine: nothing is touched
    auto fill = [&]() -> int {
        if (accumulate) return 0;
        if (d_cnt) HIPCHK(hipMemsetAsync(d_cnt, 0, nb * 8, s));
        if (d_val) HIPCHK(fj_launch_group_fill(d_val, nb, agg, s));
        return 0;
    };
    if (np == 0) {                                           // no build row has a partner
        float ms;
        if (trivial_done(c, s, &ms, fill)) return 1;
        t->total_ms = t->join_ms = t->probe_phase_ms = ms;
        return 0;
    }
    if (P.form == Prepared::HBM) {
        FjGtArgs a{};
        a.tkeys = P.keys; a.tvals = P.rows; a.cap_mask = P.cap_mask; a.flags = (u32*)P.aux; a.empty_val = (u64*)P.aux + 1;
        a.nb = nb; a.pk = pk; a.np = np; a.total = &c->d_sc->total;
        HIPCHK(hipEventRecord(c->ev[E_START], s));
        HIPCHK(hipMemsetAsync(c->d_sc, 0, offsetof(Scalars, alloc), s));
        if (fill()) return 1;
        HIPCHK(fj_launch_prep_gt_group(a, d_val ? agg : FJ_GJ_SUM, pv, d_cnt, d_val, nb, &c->d_sc->expected, &c->d_sc->err, s));
        HIPCHK(hipEventRecord(c->ev[E_JOIN], s));
        if (read_scalars(c, s)) return 1;
        t->join_ms = t->probe_phase_ms = t->total_ms = ev_ms(c, E_START, E_JOIN);
    } else {
        // (total = the hits, expected = the misses; the counts alone: the keys-only pass)
        PairAttempt a;
        if (pair_open_probe_only(c, P.plan, P.top_bits, d_val ? REL_VALUES : REL_KEYS_ONLY, pk, pv, np, s, &a)) return 1;
        FjPrepGroupArgs ga{};
        ga.probe = a.probe; ga.nparts = P.nparts;
        if (ga.probe.list && ga.probe.nb != P.nparts) return set_err("internal error: the probe side has %u partitions, the prepared build side %u", ga.probe.nb, P.nparts);
        if (!ga.probe.list && P.nparts != 1) return set_err("internal error: a flat probe side against %u prepared partitions", P.nparts);
        pair_items(a, np, &ga.items, &ga.nitems_dev, &ga.items_cap, &ga.nsplit);
        ga.keys = P.keys; ga.rows = P.rows; ga.runs = (const FjPrepRun*)P.aux; ga.nkeys = P.g; ga.nb = nb;
        ga.err = &c->d_sc->err;
        if (fill()) return 1;
        if (d_cnt) {                                         // both outputs: the passes ran once, the kernel runs once per accumulator
            ga.out = d_cnt; ga.total = &c->d_sc->total; ga.miss_total = &c->d_sc->expected;
            HIPCHK(fj_launch_prep_group(ga, FJ_GJ_COUNT, s));
        }
        if (d_val) {
            ga.out = d_val; ga.total = d_cnt ? nullptr : &c->d_sc->total; ga.miss_total = d_cnt ? nullptr : &c->d_sc->expected;   // (the count launch has them)
            HIPCHK(fj_launch_prep_group(ga, agg, s));
        }
        if (pair_close(c, a, s, t)) return 1;
        t->build_phase_ms = 0;                               // (nothing touched the build relation: its passes ran when it was prepared)
        if (c->h_sc->err & FJ_ERR_LDS_FULL) return set_err("internal error: a run of the prepared build side does not fit the LDS table");
    }
    if (c->h_sc->err & FJ_ERR_OUTCAP) return set_err("internal error: a first-occurrence position lies beyond the prepared build side");
    const u64 hits = c->h_sc->total, misses = c->h_sc->expected;
    if (hits + misses != np) return set_err("internal error: aggregate join onto the prepared side placed %llu + %llu of %zu probe rows", (unsigned long long)hits, (unsigned long long)misses, np);
    *out_count = hits;
    return 0;
}

}  // namespace fjh
