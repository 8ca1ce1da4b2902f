// fj_aligned.hip -- probe-order joins (an EXTENSION: FJ_ALGO_PROBE_ORDER, include/flashjoin.h): one output row per probe row, AT the
// probe row's position.  out_vals[i] = the build value (FJ_ALGO_ROW_IDS: the build position) of the first occurrence of probe key i,
// mask[i] = 1 / 0 whether it has a partner: a dictionary lookup, a foreign-key column, an isin mask, a mark join.
//
// It is the one join whose size and layout are known before it starts, so nothing is reserved: the partition passes and work items
// are the left join's (csrc/fj_outer.hip; the probe side carries its rows' positions through the passes, PassIter::vals_pos), the LDS
// table is the left join's 8192 key slots (+ 8192 values), and the probe phase ends in one 8-byte and / or one 1-byte store per row
// at the row's own position - no ballots for placement, no LDS cursors, no global cursor.  Hits and misses are counted per wave and
// added to the two device words once per workgroup; the host checks hits + misses == np.
//
// Fallbacks as for the left join, decided by the host from the device error word: FJ_STAT_DUPS (value form, unique-key launch) -> the
// build side once more with row indices, the FIRST form overwrites every row (a scatter by position is idempotent);
// FJ_ERR_LDS_FULL -> the whole join on the global HBM table (fj_gt_probe_order_kernel, csrc/fj_join.hip), timings.fell_back = 1.
#include "fj_host.h"
#include "fj_lds_table_dev.h"

namespace {

constexpr u32 PO_NT = 1024, PO_KPT = 8, PO_ROUND_CHUNKS = PO_NT * PO_KPT / FJ_CHUNK;
constexpr u32 PO_TS = 8192, PO_LIMIT = PO_TS - PO_TS / 16;
struct PoHdr { u32 full, dups, empty_cnt, nkeys, hits, misses, pad0, pad1; u64 empty_val, pad2; };

// FIRST: build 'values' are row indices, the smallest wins (LDS atomic minimum), then - unless RID - one gather from a.orig_vals;
//        !FIRST: unique build keys expected, a duplicate raises FJ_STAT_DUPS and the item writes nothing
// RID:   the row-id form - the winning row index is the output; a miss gets ~0 instead of 0
// VALS:  a.out_vals is written (else the table holds keys only: the mask form)      MASK: mask[] is written
template <bool FIRST, bool RID, bool VALS, bool MASK>
__global__ __launch_bounds__(PO_NT, 1) void fj_probe_order_join_kernel(FjLdsJoinArgs a, u64 np, unsigned long long* miss_total, unsigned char* __restrict__ mask) {
    static_assert(VALS || MASK, "an output");
    static_assert(!RID || (FIRST && VALS), "row ids: the first occurrence wins");
    static_assert(VALS || !FIRST, "the mask form keeps no values");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    PoHdr* hdr = reinterpret_cast<PoHdr*>(smem);
    u64* tkeys = reinterpret_cast<u64*>(smem + sizeof(PoHdr));
    u64* tvals = tkeys + PO_TS;                               // (VALS only)
    const u32 tid = threadIdx.x, lane = tid & 63;
    const u32 item = blockIdx.x;
    u32 p, b0, nbc, s_lo, s_hi;
    if (!fj_item_slice(a.items, a.nitems_dev, a.nsplit, a.probe.n_flat, item, p, s_lo, s_hi) || s_lo >= s_hi) return;
    fj_part_chunks(a.build, p, b0, nbc);

    for (u32 i = tid; i < PO_TS; i += PO_NT) { tkeys[i] = FJ_EMPTY_KEY; if (FIRST) tvals[i] = ~0ull; }
    if (tid == 0) { hdr->full = 0; hdr->dups = 0; hdr->empty_cnt = 0; hdr->nkeys = 0; hdr->hits = 0; hdr->misses = 0; hdr->empty_val = FIRST ? ~0ull : 0ull; }
    __syncthreads();

    // ---- build: distinct keys (and the value of one copy; FIRST: the smallest row index) ----
    for (u32 c0 = 0; c0 < nbc; c0 += PO_NT / FJ_CHUNK) {
        const u32 c = c0 + tid / FJ_CHUNK, off = tid % FJ_CHUNK;
        if (c >= nbc) continue;
        const u32 e = fj_chunk_entry(a.build, b0 + c);
        if (off >= FJ_LIST_CNT(e)) continue;
        const u64 src = (u64)FJ_LIST_ID(e) * FJ_CHUNK + off;
        const u64 key = a.build.list ? a.build.keys[src] : fj_key_mix(a.build.keys[src]);   // chunk pools hold mixed keys, flat arrays raw ones
        const u64 val = VALS ? ((RID && !a.build.vals) ? src : a.build.vals[src]) : 0;
        if (key == FJ_EMPTY_KEY) {                           // the empty marker is never stored in the table
            const u32 before = atomicAdd(&hdr->empty_cnt, 1u);
            if (FIRST) atomicMin((unsigned long long*)&hdr->empty_val, (unsigned long long)val);
            else if (VALS) { if (before == 0) hdr->empty_val = val; else hdr->dups = 1; }
            continue;
        }
        u32 pos = FJ_HW2(key) & (PO_TS - 1);
        bool placed = false;
        for (u32 step = 0; step < PO_TS; ++step) {
            const u64 old = atomicCAS((unsigned long long*)&tkeys[pos], (unsigned long long)FJ_EMPTY_KEY, (unsigned long long)key);
            if (old == FJ_EMPTY_KEY) {
                if (atomicAdd(&hdr->nkeys, 1u) >= PO_LIMIT) hdr->full = 1;
                if (FIRST) atomicMin((unsigned long long*)&tvals[pos], (unsigned long long)val);
                else if (VALS) tvals[pos] = val;
                placed = true;
                break;
            }
            if (old == key) {
                if (FIRST) atomicMin((unsigned long long*)&tvals[pos], (unsigned long long)val);
                else if (VALS) hdr->dups = 1;
                placed = true;
                break;
            }
            pos = (pos + 1) & (PO_TS - 1);
        }
        if (!placed) hdr->full = 1;
    }
    __syncthreads();
    if (hdr->full) { if (tid == 0) atomicOr(a.err, FJ_ERR_LDS_FULL); return; }     // the host re-runs the join on the HBM table
    if (VALS && !FIRST && hdr->dups) { if (tid == 0) atomicOr(a.err, FJ_STAT_DUPS); return; }   // ... or this one with row indices
    const bool has_empty = hdr->empty_cnt != 0;
    if (FIRST && !RID) {                                     // winning row indices -> the caller's values
        for (u32 i = tid; i < PO_TS; i += PO_NT) if (tkeys[i] != FJ_EMPTY_KEY) tvals[i] = a.orig_vals[tvals[i]];
        if (tid == 0 && has_empty) hdr->empty_val = a.orig_vals[hdr->empty_val];
        __syncthreads();
    }
    const u64 empty_val = hdr->empty_val;

    // ---- probe: rounds of PO_NT * PO_KPT rows; the next round's keys and positions are requested before this round's stores.
    // A row's result goes to the row's own position: no reservation of any kind ----
    u64 k[PO_KPT], rp[PO_KPT];
    u32 okm = 0, nh = 0, nm = 0;                             // nh / nm: wave-uniform counts of this wave's hits and misses
    auto load_round = [&](u32 pc, u64 (&kk)[PO_KPT], u64 (&pp)[PO_KPT], u32& ok) {
        ok = 0;
#pragma unroll
        for (u32 u = 0; u < PO_KPT; ++u) {
            const u32 c = pc + u * (PO_NT / FJ_CHUNK) + tid / FJ_CHUNK, off = tid % FJ_CHUNK;
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
    for (u32 pc = s_lo; pc < s_hi; pc += PO_ROUND_CHUNKS) {
        u64 v[VALS ? PO_KPT : 1];
        u32 hit = 0;
#pragma unroll
        for (u32 u = 0; u < PO_KPT; ++u) {
            if (VALS) v[VALS ? u : 0] = RID ? ~0ull : 0ull;
            const bool ok = (okm >> u) & 1u;
            bool h = false;
            if (ok) {
                const u64 key = a.probe.list ? k[u] : fj_key_mix(k[u]);
                if (key == FJ_EMPTY_KEY) { h = has_empty; if (VALS && h) v[VALS ? u : 0] = empty_val; }
                else {
                    u32 pos = FJ_HW2(key) & (PO_TS - 1);
                    for (;;) {                               // the build left >= 1/16 of the slots empty: always terminates
                        const u64 t = tkeys[pos];
                        if (t == key) { h = true; if (VALS) v[VALS ? u : 0] = tvals[pos]; break; }
                        if (t == FJ_EMPTY_KEY) break;
                        pos = (pos + 1) & (PO_TS - 1);
                    }
                }
            }
            if (h) hit |= 1u << u;
            nh += (u32)__popcll(__ballot(h)); nm += (u32)__popcll(__ballot(ok && !h));
        }
        u64 kn[PO_KPT], rpn[PO_KPT];
        u32 okn = 0;
        if (pc + PO_ROUND_CHUNKS < s_hi) load_round(pc + PO_ROUND_CHUNKS, kn, rpn, okn);
#pragma unroll
        for (u32 u = 0; u < PO_KPT; ++u) {
            if (!((okm >> u) & 1u)) continue;
            const u64 o = rp[u];
            if (o < np) {                                    // (always: positions are 0 .. np - 1; a row outside would be a pass's bug)
                if (VALS) a.out_vals[o] = v[VALS ? u : 0];
                if (MASK) mask[o] = (unsigned char)((hit >> u) & 1u);
            } else atomicOr(a.err, FJ_ERR_OUTCAP);
        }
#pragma unroll
        for (u32 u = 0; u < PO_KPT; ++u) { k[u] = kn[u]; rp[u] = rpn[u]; }
        okm = okn;
    }
    if (lane == 0) { if (nh) atomicAdd(&hdr->hits, nh); if (nm) atomicAdd(&hdr->misses, nm); }
    __syncthreads();
    if (tid == 0) {
        if (hdr->hits) atomicAdd(a.total, (unsigned long long)hdr->hits);
        if (hdr->misses) atomicAdd(miss_total, (unsigned long long)hdr->misses);
    }
}

}  // namespace

hipError_t fj_launch_probe_order_join(const FjLdsJoinArgs& a, bool first, u64 np, unsigned long long* miss_total, unsigned char* mask, hipStream_t s) {
    const u32 nb = a.items ? a.items_cap : a.nparts * a.nsplit;
    const bool vals = a.out_vals != nullptr, rid = a.row_ids != 0;
    if (!a.total || !miss_total || !a.err || (!vals && !mask)) return hipErrorInvalidValue;
    if (rid && (!vals || !first)) return hipErrorInvalidValue;                    // row ids: the first occurrence from the start
    if (first && (!vals || (!rid && !a.orig_vals))) return hipErrorInvalidValue;
    const u32 lds = (u32)sizeof(PoHdr) + PO_TS * (vals ? 16u : 8u);
    void (*kern)(FjLdsJoinArgs, u64, unsigned long long*, unsigned char*);
    if (!vals) kern = fj_probe_order_join_kernel<false, false, false, true>;
    else if (rid) kern = mask ? fj_probe_order_join_kernel<true, true, true, true> : fj_probe_order_join_kernel<true, true, true, false>;
    else if (first) kern = mask ? fj_probe_order_join_kernel<true, false, true, true> : fj_probe_order_join_kernel<true, false, true, false>;
    else kern = mask ? fj_probe_order_join_kernel<false, false, true, true> : fj_probe_order_join_kernel<false, false, true, false>;
    hipError_t e = fj_set_max_lds_once(reinterpret_cast<const void*>(kern), lds);
    if (e != hipSuccess) return e;
    if (nb) hipLaunchKernelGGL(kern, dim3(nb), dim3(PO_NT), lds, s, a, np, miss_total, mask);
    return hipGetLastError();
}

namespace fjh {

// the global-table form (fj_host.h).  The table holds first-occurrence row indices (d_ov != nullptr) or keys only (the mask form)
static int join_probe_order_global(fj_ctx* c, const u64* bk, const u64* bv, size_t nb, const u64* pk, size_t np, hipStream_t s,
                                   fj_timings* t, u64* out_count, unsigned char* d_mask, u64* d_ov, bool rid) {
    const bool vals = d_ov != nullptr;
    const u64 cap = gt_capacity(nb);
    FjGtArgs a{};
    if (gt_open(c, nb, vals ? cap : 0, s, &a, &a.tvals)) return 1;
    a.bk = bk; a.bv = (vals && !rid) ? bv : nullptr; a.pk = pk; a.np = np;
    a.out_vals = d_ov; a.row_ids = rid ? 1u : 0u;
    HIPCHK(hipMemsetAsync(&c->d_sc->empty_val, 0xFF, sizeof(u64), s));           // (row index minimum)
    if (vals) HIPCHK(hipMemsetAsync(a.tvals, 0xFF, cap * 8, s));
    HIPCHK(fj_launch_gt_build_first(a, vals, s));
    HIPCHK(hipEventRecord(c->ev[E_BUILD], s));
    HIPCHK(hipEventRecord(c->ev[E_PPART], s));
    HIPCHK(fj_launch_gt_probe_order(a, &c->d_sc->expected, d_mask, s));
    if (gt_close(c, s, t)) return 1;
    const u64 hits = c->h_sc->total, misses = c->h_sc->expected;
    if (hits + misses != np) return set_err("internal error: probe-order join placed %llu + %llu of %zu probe rows", (unsigned long long)hits, (unsigned long long)misses, np);
    *out_count = hits;
    return 0;
}

// FJ_ALGO_PROBE_ORDER (fj_join_device has checked the arguments): d_ov[i] (np words, may be null) and d_mask[i] (np bytes, may be
// null) for every probe row i; *out_count = probe rows with a partner.  use_radix: the partitioned plan, else the global table.
// rid: d_ov holds first-occurrence build positions (~0: none) and bv is not read
int join_probe_order(fj_ctx* c, bool use_radix, const u64* bk, const u64* bv, size_t nb, const u64* pk, size_t np, int top_bits,
                     hipStream_t s, fj_timings* t, u64* out_count, unsigned char* d_mask, u64* d_ov, bool rid) {
    const bool vals = d_ov != nullptr;
    if (!vals) rid = false;                                  // (the mask form reads no value of either kind)
    *out_count = 0;
    if (np == 0) return 0;
    if (nb == 0) {                                           // no probe row has a partner
        float ms;
        if (trivial_done(c, s, &ms, [&]() -> int {
                if (vals) HIPCHK(hipMemsetAsync(d_ov, rid ? 0xFF : 0, np * 8, s));
                if (d_mask) HIPCHK(hipMemsetAsync(d_mask, 0, np, s));
                return 0;
            })) return 1;
        t->path = use_radix ? 0 : 1; t->total_ms = t->join_ms = t->probe_phase_ms = ms;
        return 0;
    }
    if (!use_radix) return join_probe_order_global(c, bk, bv, nb, pk, np, s, t, out_count, d_mask, d_ov, rid);

    // (total = the hits, expected = the misses; the probe rows' positions travel through the passes)
    PairAttempt a;
    if (pair_open(c, make_plan(nb, top_bits, false), {!vals ? REL_KEYS_ONLY : rid ? REL_POSITIONS : REL_VALUES, REL_POSITIONS}, bk, bv, nb, pk, nullptr, np, top_bits, s, &a)) return 1;
    FjLdsJoinArgs ja{};
    ja.build = a.build; ja.probe = a.probe; ja.nparts = a.nparts;
    pair_items(a, np, &ja.items, &ja.nitems_dev, &ja.items_cap, &ja.nsplit);
    ja.err = &c->d_sc->err; ja.total = &c->d_sc->total;
    ja.out_capacity = np; ja.out_vals = d_ov;
    ja.row_ids = rid ? 1u : 0u;
    HIPCHK(fj_launch_probe_order_join(ja, rid, np, &c->d_sc->expected, d_mask, s));
    if (pair_close(c, a, s, t)) return 1;
    if (vals && !rid && !(c->h_sc->err & FJ_ERR_LDS_FULL) && (c->h_sc->err & FJ_STAT_DUPS)) {
        // duplicate build keys: the build side once more with row indices as payload, and every row stored again
        if (pair_rerun_build_with_row_ids(c, &a, bk, nb, top_bits, nullptr, s)) return 1;
        ja.build = a.build; ja.orig_vals = bv;
        HIPCHK(fj_launch_probe_order_join(ja, true, np, &c->d_sc->expected, d_mask, s));
        if (pair_close(c, a, s, t)) return 1;
    }
    if (c->h_sc->err & FJ_ERR_LDS_FULL)                      // a partition beyond the LDS table: the whole join on the HBM table
        return gt_fallback(t, [&](fj_timings* g) { return join_probe_order_global(c, bk, bv, nb, pk, np, s, g, out_count, d_mask, d_ov, rid); });
    if (c->h_sc->err & FJ_ERR_OUTCAP) return set_err("internal error: a probe row's position lies beyond the probe side");
    const u64 hits = c->h_sc->total, misses = c->h_sc->expected;
    if (hits + misses != np) return set_err("internal error: probe-order join placed %llu + %llu of %zu probe rows", (unsigned long long)hits, (unsigned long long)misses, np);
    *out_count = hits;
    return 0;
}

}  // namespace fjh
