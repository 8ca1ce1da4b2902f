// fj_outer.hip -- left outer, anti and full outer joins on the partitioned plan (an EXTENSION: FJ_ALGO_LEFT_OUTER / FJ_ALGO_ANTI /
// FJ_ALGO_FULL_OUTER, include/flashjoin.h).
//
// The N:1 join of the reference (first occurrence of a duplicate build key wins, hash_join.cpp:125) answers "which probe rows have
// a partner, and with which value".  A left outer join also returns the rows WITHOUT one, an anti join only those.  With N:1
// semantics a left join has exactly np output rows, so it runs in ONE pass over the probe side: no counting pass, no scan.
//
// Same partitioning and work items as the other joins (zero-pass plans: flat arrays, items are nsplit slices; one or more passes:
// chunk lists, items are the probe side's final tiles); one 1024-thread workgroup per item keeps in LDS
//   LEFT  8192 key slots + 8192 values (128 KiB),     ANTI  16384 key slots (128 KiB),
// linear probing from the low hash word, a slot claimed by a 64-bit compare-and-swap, duplicate keys merged at insert.  Then the
// item's probe rows stream through in rounds of 8192 (8 per thread; the next round's loads in flight during this one's reservation): hits are written from a FRONT cursor counting up from 0,
// misses from a BACK cursor counting down from np (ANTI: misses only, from row 0 up).  Positions are reserved wave-wide (ballot + popcount into
// an LDS cursor per workgroup), and thread 0 turns the round's totals into global ranges with one atomic per cursor and round
// (fj_oj_reserve; the scheme of the single-pass emit kernel, csrc/fj_join.hip): ~125K atomics per cursor at 1B probe rows.
//
// Fallbacks, both decided by the host from the device error word:
//   FJ_STAT_DUPS (LEFT)    a build key occurs more than once: the output is rewritten by a second launch whose build side carries
//                          row indices (fj_iota_kernel); every copy lowers its slot's index with an LDS atomic minimum and the
//                          winners are turned into values with one gather from the caller's build_values (the first-occurrence rule
//                          of the radix path and of the NumPy reference in the tests);
//   FJ_ERR_LDS_FULL        a partition holds more distinct keys than the table takes (15/16 of its slots): the whole join runs
//                          again on the global HBM table (fj_gt_outer_probe_kernel, csrc/fj_join.hip), timings.fell_back = 1.
//
// Full outer join (FJ_ALGO_FULL_OUTER): the left join's launch in its FULL form also marks, in a bitmap in HBM, the build rows its
// probe rows matched; fj_full_sweep_kernel then appends the unmarked build rows behind row np (join_full below).
#include "fj_host.h"
#include "fj_lds_table_dev.h"

namespace {

constexpr u32 OJ_NT = 1024, OJ_KPT = 8, OJ_ROUND_CHUNKS = OJ_NT * OJ_KPT / FJ_CHUNK;
constexpr u32 OJ_MBITS_WORDS = 8192 / 32 + 4;                 // full outer join: hit bits of the 8192 slots + the empty marker's word (16-byte multiple)
struct OjHdr { u32 full, dups, empty_cnt, nkeys; FjOjCursor cur; u64 empty_val; };

// RID: the row-id form (FjLdsJoinArgs::row_ids; MODE LEFT_FIRST or ANTI) - build values are row positions and the smallest is
// written as it is; every output row gets the probe row's position (its vals plane; flat arrays: the index), a miss the value ~0
// FULL: the full outer join (FJ_ALGO_FULL_OUTER; MODE LEFT or LEFT_FIRST) - rows [0, np) as above, and the item remembers which of its
// table's slots were hit: one bit per slot in LDS (mbits, behind the values; one more word for the empty marker key), set by the probe
// rounds.  After its last round the item walks its partition's build chunks once more, looks every row's key up and ORs the rows of hit
// slots into `bits` (one bit per build row at chunk id * FJ_CHUNK + offset - the same place for every item of the partition, whatever
// slot the key took in this item's table; a wave covers 64 consecutive rows of one chunk: one 64-bit atomic per non-zero ballot).
// Marking per ROW is what makes every copy of a matched duplicate key count as matched.  fj_full_sweep_kernel reads the zero bits.
template <int MODE, bool RID = false, bool FULL = false>
__global__ __launch_bounds__(OJ_NT, 1) void fj_outer_join_kernel(FjLdsJoinArgs a, u64 np, unsigned long long* miss_cursor, u64* bits) {
    constexpr bool VALS = MODE != FJ_OJ_ANTI, FIRST = MODE == FJ_OJ_LEFT_FIRST;
    static_assert(!RID || MODE != FJ_OJ_LEFT, "row ids: the first occurrence wins");
    static_assert(!FULL || VALS, "full outer join: a left join's table");
    constexpr u32 TS = VALS ? 8192u : 16384u, LIMIT = TS - TS / 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    OjHdr* hdr = reinterpret_cast<OjHdr*>(smem);
    u64* tkeys = reinterpret_cast<u64*>(smem + sizeof(OjHdr));
    u64* tvals = tkeys + TS;                                  // (VALS only)
    u32* mbits = reinterpret_cast<u32*>(tvals + TS);          // (FULL only) [TS / 32] hit slots, [TS / 32] != 0: the empty marker key was hit
    const u32 tid = threadIdx.x, lane = tid & 63;
    const u32 item = blockIdx.x;
    u32 p, b0 = 0, nbc, s_lo, s_hi;
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
    if (s_lo >= s_hi) return;
    if (a.build.list) { b0 = a.build.boff[p]; nbc = a.build.boff[p + 1] - b0; }
    else nbc = (u32)((a.build.n_flat + FJ_CHUNK - 1) >> FJ_CHUNK_LOG);

    for (u32 i = tid; i < TS; i += OJ_NT) { tkeys[i] = FJ_EMPTY_KEY; if (FIRST) tvals[i] = ~0ull; }
    if (FULL) for (u32 i = tid; i < OJ_MBITS_WORDS; i += OJ_NT) mbits[i] = 0;
    if (tid == 0) { hdr->full = 0; hdr->dups = 0; hdr->empty_cnt = 0; hdr->nkeys = 0; hdr->cur.hit = 0; hdr->cur.miss = 0; hdr->empty_val = FIRST ? ~0ull : 0ull; }
    __syncthreads();

    // ---- build: distinct keys (and the value of one copy; FIRST: the smallest row index) ----
    for (u32 c0 = 0; c0 < nbc; c0 += OJ_NT / FJ_CHUNK) {
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
        u32 pos = FJ_HW2(key) & (TS - 1);
        bool placed = false;
        for (u32 step = 0; step < TS; ++step) {
            const u64 old = atomicCAS((unsigned long long*)&tkeys[pos], (unsigned long long)FJ_EMPTY_KEY, (unsigned long long)key);
            if (old == FJ_EMPTY_KEY) {
                if (atomicAdd(&hdr->nkeys, 1u) >= LIMIT) hdr->full = 1;
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
            pos = (pos + 1) & (TS - 1);
        }
        if (!placed) hdr->full = 1;
    }
    __syncthreads();
    if (hdr->full) { if (tid == 0) atomicOr(a.err, FJ_ERR_LDS_FULL); return; }     // the host re-runs the join on the HBM table
    if (VALS && !FIRST && hdr->dups) { if (tid == 0) atomicOr(a.err, FJ_STAT_DUPS); return; }   // ... or this one with row indices
    const bool has_empty = hdr->empty_cnt != 0;
    if (FIRST && !RID) {                                     // winning row indices -> the caller's values
        for (u32 i = tid; i < TS; i += OJ_NT) if (tkeys[i] != FJ_EMPTY_KEY) tvals[i] = a.orig_vals[tvals[i]];
        if (tid == 0 && has_empty) hdr->empty_val = a.orig_vals[hdr->empty_val];
        __syncthreads();
    }
    const u64 empty_val = hdr->empty_val;

    // ---- probe: rounds of OJ_NT * OJ_KPT rows, hits to the front, misses to the back; the next round's keys are requested
    // before this round's reservation (its barriers and the global atomic's round trip hide the loads' latency) ----
    u64 k[OJ_KPT], rp[RID ? OJ_KPT : 1];                      // rp: the probe rows' positions (RID)
    u32 okm = 0;
    auto load_round = [&](u32 pc, u64 (&kk)[OJ_KPT], u64 (&pp)[RID ? OJ_KPT : 1], u32& ok) {
        ok = 0;
#pragma unroll
        for (u32 u = 0; u < OJ_KPT; ++u) {
            const u32 c = pc + u * (OJ_NT / FJ_CHUNK) + tid / FJ_CHUNK, off = tid % FJ_CHUNK;
            kk[u] = 0;
            if (RID) pp[RID ? u : 0] = 0;
            if (c >= s_hi) continue;
            const u32 e = fj_chunk_entry(a.probe, c);
            if (off >= FJ_LIST_CNT(e)) continue;
            const u64 src = (u64)FJ_LIST_ID(e) * FJ_CHUNK + off;
            kk[u] = a.probe.keys[src];
            if (RID) pp[RID ? u : 0] = a.probe.vals ? a.probe.vals[src] : src;
            ok |= 1u << u;
        }
    };
    load_round(s_lo, k, rp, okm);
    for (u32 pc = s_lo; pc < s_hi; pc += OJ_ROUND_CHUNKS) {
        u64 v[OJ_KPT];
        u32 hit = 0, miss = 0;
#pragma unroll
        for (u32 u = 0; u < OJ_KPT; ++u) {
            v[u] = 0;
            if (!((okm >> u) & 1u)) continue;
            if (!a.probe.list) k[u] = fj_key_mix(k[u]);
            bool h = false;
            if (k[u] == FJ_EMPTY_KEY) { h = has_empty; v[u] = empty_val; if (FULL && h) mbits[TS / 32] = 1; }
            else {
                u32 pos = FJ_HW2(k[u]) & (TS - 1);
                for (;;) {                                   // the build left >= 1/16 of the slots empty: always terminates
                    const u64 t = tkeys[pos];
                    if (t == k[u]) {
                        h = true;
                        if (VALS) v[u] = tvals[pos];
                        // (read first: most hits find their slot's bit set already and skip the LDS atomic)
                        if (FULL && !((mbits[pos >> 5] >> (pos & 31)) & 1u)) atomicOr(&mbits[pos >> 5], 1u << (pos & 31));
                        break;
                    }
                    if (t == FJ_EMPTY_KEY) break;
                    pos = (pos + 1) & (TS - 1);
                }
            }
            if (h) hit |= 1u << u; else miss |= 1u << u;
        }
        if (!VALS) hit = 0;                                  // ANTI writes misses only
        u64 hb[OJ_KPT], mb[OJ_KPT];
        u32 nh = 0, nm = 0;
#pragma unroll
        for (u32 u = 0; u < OJ_KPT; ++u) {
            hb[u] = __ballot((hit >> u) & 1u); mb[u] = __ballot((miss >> u) & 1u);
            nh += (u32)__popcll(hb[u]); nm += (u32)__popcll(mb[u]);
        }
        u64 kn[OJ_KPT], rpn[RID ? OJ_KPT : 1];
        u32 okn = 0;
        if (pc + OJ_ROUND_CHUNKS < s_hi) load_round(pc + OJ_ROUND_CHUNKS, kn, rpn, okn);
        u64 hpos, mpos;
        fj_oj_reserve(&hdr->cur, nh, nm, lane, tid, a.out_cursor, miss_cursor, hpos, mpos);
        const u64 below = (1ull << lane) - 1ull;
#pragma unroll
        for (u32 u = 0; u < OJ_KPT; ++u) {
            if ((hit >> u) & 1u) {
                const u64 o = hpos + (u32)__popcll(hb[u] & below);
                if (o < a.out_capacity) { a.out_keys[o] = RID ? rp[RID ? u : 0] : fj_key_unmix(k[u]); a.out_vals[o] = v[u]; }
                else atomicOr(a.err, FJ_ERR_OUTCAP);
            }
            if ((miss >> u) & 1u) {
                const u64 m = mpos + (u32)__popcll(mb[u] & below);
                const u64 o = VALS ? np - 1 - m : m;          // LEFT: from the back; ANTI: the misses are the whole output
                if (m < np && o < a.out_capacity) {
                    a.out_keys[o] = RID ? rp[RID ? u : 0] : fj_key_unmix(k[u]);
                    if (VALS) a.out_vals[o] = RID ? ~0ull : 0ull;
                } else atomicOr(a.err, FJ_ERR_OUTCAP);
            }
            hpos += (u32)__popcll(hb[u]); mpos += (u32)__popcll(mb[u]);
        }
#pragma unroll
        for (u32 u = 0; u < OJ_KPT; ++u) { k[u] = kn[u]; if (RID) rp[RID ? u : 0] = rpn[RID ? u : 0]; }
        okm = okn;
    }
    if (FULL) {
        // ---- the build rows this item's probe rows found: uniform control flow up to the ballot (c is wave-uniform) ----
        static_assert(FJ_CHUNK % 64 == 0, "a wave covers 64 consecutive rows of one chunk");
        __syncthreads();
        const bool empty_hit = mbits[TS / 32] != 0;
        for (u32 c0 = 0; c0 < nbc; c0 += OJ_NT / FJ_CHUNK) {
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
                        u32 pos = FJ_HW2(key) & (TS - 1);
                        for (;;) {                           // (the key is in the table: the build put it there)
                            const u64 t = tkeys[pos];
                            if (t == key) { mt = (mbits[pos >> 5] >> (pos & 31)) & 1u; break; }
                            if (t == FJ_EMPTY_KEY) break;
                            pos = (pos + 1) & (TS - 1);
                        }
                    }
                }
            }
            const u64 bal = __ballot(mt);
            if (lane == 0 && bal) atomicOr((unsigned long long*)&bits[src >> 6], (unsigned long long)bal);
        }
    }
}

// full outer join, last step: the build rows whose bit is still zero -> out rows [base, base + *cursor).  Rounds of four chunks per
// workgroup; a round's rows are reserved wave by wave in LDS (ballot + popcount) and with one global atomic per workgroup.
__global__ __launch_bounds__(OJ_NT) void fj_full_sweep_kernel(FjChunkSet b, const u64* __restrict__ bits, const u64* __restrict__ orig_vals, u32 row_ids,
                                                              u64* __restrict__ out_keys, u64* __restrict__ out_vals, u64 base, u64 out_capacity,
                                                              unsigned long long* cursor, u32* err) {
    __shared__ u32 s_cnt;
    __shared__ u64 s_base;
    const u32 tid = threadIdx.x, lane = tid & 63;
    const u32 nch = b.list ? b.boff[b.nb] : (u32)((b.n_flat + FJ_CHUNK - 1) >> FJ_CHUNK_LOG);
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    for (u32 c0 = blockIdx.x * (OJ_NT / FJ_CHUNK); c0 < nch; c0 += gridDim.x * (OJ_NT / FJ_CHUNK)) {     // (uniform per workgroup)
        const u32 c = c0 + tid / FJ_CHUNK, off = tid % FJ_CHUNK;
        bool un = false;
        u64 src = 0;
        if (c < nch) {
            const u32 e = fj_chunk_entry(b, c);
            src = (u64)FJ_LIST_ID(e) * FJ_CHUNK + off;
            if (off < FJ_LIST_CNT(e)) un = !((bits[src >> 6] >> (src & 63)) & 1ull);
        }
        const u64 bal = __ballot(un);
        const u32 n = (u32)__popcll(bal);
        u32 w = 0;
        if (lane == 0 && n) w = atomicAdd(&s_cnt, n);
        w = __shfl(w, 0, 64);
        __syncthreads();
        if (tid == 0) { s_base = s_cnt ? (u64)atomicAdd(cursor, (unsigned long long)s_cnt) : 0ull; s_cnt = 0; }
        __syncthreads();
        if (un) {
            const u64 o = base + s_base + w + (u32)__popcll(bal & ((1ull << lane) - 1ull));
            if (o < out_capacity) {
                u64 v = b.vals ? b.vals[src] : src;              // (no vals plane: flat arrays of a row-id join, the index is the position)
                if (orig_vals) v = orig_vals[v];
                out_keys[o] = row_ids ? ~0ull : (b.list ? fj_key_unmix(b.keys[src]) : b.keys[src]);   // chunk pools hold mixed keys
                out_vals[o] = v;
            } else atomicOr(err, FJ_ERR_OUTCAP);
        }
    }
}

}  // namespace

hipError_t fj_launch_outer_join(const FjLdsJoinArgs& a, int mode, u64 np, unsigned long long* miss_cursor, hipStream_t s) {
    const u32 nb = a.items ? a.items_cap : a.nparts * a.nsplit;
    if (!a.out_cursor || !miss_cursor || !a.out_keys || (mode != FJ_OJ_ANTI && !a.out_vals) || (mode == FJ_OJ_LEFT_FIRST && !a.orig_vals && !a.row_ids))
        return hipErrorInvalidValue;
    if (a.row_ids && mode == FJ_OJ_LEFT) return hipErrorInvalidValue;            // row ids: LEFT_FIRST (first occurrence) or ANTI
    const u32 lds = (u32)sizeof(OjHdr) + (mode == FJ_OJ_ANTI ? 16384u * 8 : 8192u * 16);
    auto kern = a.row_ids ? (mode == FJ_OJ_ANTI ? fj_outer_join_kernel<FJ_OJ_ANTI, true> : fj_outer_join_kernel<FJ_OJ_LEFT_FIRST, true>)
              : mode == FJ_OJ_ANTI ? fj_outer_join_kernel<FJ_OJ_ANTI>
              : mode == FJ_OJ_LEFT_FIRST ? fj_outer_join_kernel<FJ_OJ_LEFT_FIRST> : fj_outer_join_kernel<FJ_OJ_LEFT>;
    hipError_t e = fj_set_max_lds_once(reinterpret_cast<const void*>(kern), lds);
    if (e != hipSuccess) return e;
    if (nb) hipLaunchKernelGGL(kern, dim3(nb), dim3(OJ_NT), lds, s, a, np, miss_cursor, (u64*)nullptr);
    return hipGetLastError();
}

hipError_t fj_launch_outer_join_full(const FjLdsJoinArgs& a, int mode, u64 np, unsigned long long* miss_cursor, u64* bits, hipStream_t s) {
    const u32 nb = a.items ? a.items_cap : a.nparts * a.nsplit;
    if (!a.out_cursor || !miss_cursor || !a.out_keys || !a.out_vals || !bits || (mode != FJ_OJ_LEFT && mode != FJ_OJ_LEFT_FIRST)) return hipErrorInvalidValue;
    if (mode == FJ_OJ_LEFT ? a.row_ids != 0 : (!a.orig_vals && !a.row_ids)) return hipErrorInvalidValue;
    const u32 lds = (u32)sizeof(OjHdr) + 8192u * 16 + OJ_MBITS_WORDS * 4;
    auto kern = a.row_ids ? fj_outer_join_kernel<FJ_OJ_LEFT_FIRST, true, true>
              : mode == FJ_OJ_LEFT_FIRST ? fj_outer_join_kernel<FJ_OJ_LEFT_FIRST, false, true> : fj_outer_join_kernel<FJ_OJ_LEFT, false, true>;
    hipError_t e = fj_set_max_lds_once(reinterpret_cast<const void*>(kern), lds);
    if (e != hipSuccess) return e;
    if (nb) hipLaunchKernelGGL(kern, dim3(nb), dim3(OJ_NT), lds, s, a, np, miss_cursor, bits);
    return hipGetLastError();
}

hipError_t fj_launch_full_sweep(const FjChunkSet& build, const u64* bits, const u64* orig_vals, u32 row_ids, u64* out_keys, u64* out_vals,
                                u64 base, u64 out_capacity, unsigned long long* cursor, u32* err, hipStream_t s) {
    if (!bits || !out_keys || !out_vals || !cursor || !err) return hipErrorInvalidValue;
    const u64 bound = build.list ? build.cap : (build.n_flat + FJ_CHUNK - 1) >> FJ_CHUNK_LOG;      // chunks at most
    if (bound == 0) return hipSuccess;
    const u32 grid = (u32)std::min<u64>(4096, (bound + OJ_NT / FJ_CHUNK - 1) / (OJ_NT / FJ_CHUNK));
    hipLaunchKernelGGL(fj_full_sweep_kernel, dim3(grid), dim3(OJ_NT), 0, s, build, bits, orig_vals, row_ids, out_keys, out_vals, base, out_capacity, cursor, err);
    return hipGetLastError();
}

namespace fjh {

// the global-table form (fj_host.h).  LEFT builds with row indices (the smallest wins, first occurrence)
// full_r != nullptr (LEFT only): the full outer join - the probe marks the slots it hits, a sweep over the flat build rows looks every
// key up again and appends the rows of unmarked slots behind row np; *full_r = their number
static int join_outer_global(fj_ctx* c, int mode, const u64* bk, const u64* bv, size_t nb, const u64* pk, size_t np, hipStream_t s,
                             fj_timings* t, u64* out_count, u64* d_ok, u64* d_ov, bool rid, u64* full_r = nullptr) {
    const bool left = mode != FJ_OJ_ANTI;
    const u64 cap = gt_capacity(nb);
    FjGtArgs a{};
    if (full_r) {
        void* p;
        if (get_buf(c, W_FULL_BITS, (cap / 32 + 1) * 4, &p)) return 1;
        a.matched = (u32*)p;
    }
    if (gt_open(c, nb, left ? cap : 0, s, &a, &a.tvals)) return 1;
    a.bk = bk; a.bv = (left && !rid) ? bv : nullptr; a.pk = pk; a.np = np;
    a.out_keys = d_ok; a.out_vals = left ? d_ov : nullptr; a.row_ids = rid ? 1u : 0u;
    if (full_r) {
        HIPCHK(hipMemsetAsync(a.matched, 0, (cap / 32 + 1) * 4, s));
        HIPCHK(hipMemsetAsync(&c->d_sc->sample_hits, 0, sizeof(unsigned long long), s));      // (the sweep's row cursor)
    }
    HIPCHK(hipMemsetAsync(&c->d_sc->empty_val, 0xFF, sizeof(u64), s));           // (row index minimum)
    if (left) HIPCHK(hipMemsetAsync(a.tvals, 0xFF, cap * 8, s));
    HIPCHK(fj_launch_gt_build_first(a, left, s));
    HIPCHK(hipEventRecord(c->ev[E_BUILD], s));
    HIPCHK(hipEventRecord(c->ev[E_PPART], s));
    HIPCHK(fj_launch_gt_outer_probe(a, mode, &c->d_sc->expected, np, s));
    HIPCHK(hipEventRecord(c->ev[E_JOIN], s));
    if (full_r) {
        HIPCHK(hipEventRecord(c->ev[E_EMIT0], s));
        HIPCHK(fj_launch_gt_full_sweep(a, np, (u64)np + nb, &c->d_sc->sample_hits, &c->d_sc->err, s));
        HIPCHK(hipEventRecord(c->ev[E_EMIT1], s));
    }
    if (gt_read(c, s, t)) return 1;                          // (E_JOIN stands before the sweep: gt_close's second half)
    if (c->h_sc->err & FJ_ERR_OUTCAP) return set_err("internal error: the outer join's global-table probe wrote out of its rows");
    const u64 hits = c->h_sc->total, misses = c->h_sc->expected;
    if (left ? hits + misses != np : misses > np) return set_err("internal error: outer join placed %llu + %llu of %zu probe rows", (unsigned long long)hits, (unsigned long long)misses, np);
    *out_count = left ? hits : misses;
    if (full_r) {
        *full_r = c->h_sc->sample_hits;
        if (*full_r > nb) return set_err("internal error: full outer join kept %llu of %zu build rows", (unsigned long long)*full_r, nb);
        t->emit_ms = ev_ms(c, E_EMIT0, E_EMIT1); t->total_ms += t->emit_ms;
    }
    return 0;
}

// FJ_ALGO_LEFT_OUTER / FJ_ALGO_ANTI with materialize = 1 (fj_join_device has checked the arguments): *out_count = matched probe
// rows (LEFT) or unmatched ones (ANTI).  use_radix: the partitioned plan, else the global table.
// rid (row-id join): positions instead of keys and values; LEFT keeps the first occurrence from the start (its build side carries
// the positions its first pass makes), a miss gets the value ~0
int join_outer(fj_ctx* c, int mode, bool use_radix, const u64* bk, const u64* bv, size_t nb, const u64* pk, size_t np, int top_bits,
               hipStream_t s, fj_timings* t, u64* out_count, u64* d_ok, u64* d_ov, bool rid) {
    const bool left = mode != FJ_OJ_ANTI;
    *out_count = 0;
    if (np == 0) return 0;
    if (nb == 0) {                                           // every probe row is unmatched
        float ms;
        if (trivial_done(c, s, &ms, [&]() -> int {
                if (rid) HIPCHK(fj_launch_iota(d_ok, np, s));
                else HIPCHK(hipMemcpyAsync(d_ok, pk, np * 8, hipMemcpyDeviceToDevice, s));
                if (left) HIPCHK(hipMemsetAsync(d_ov, rid ? 0xFF : 0, np * 8, s));
                return 0;
            })) return 1;
        t->path = use_radix ? 0 : 1; t->total_ms = t->join_ms = t->probe_phase_ms = ms;
        *out_count = left ? 0 : np;
        return 0;
    }
    if (!use_radix) return join_outer_global(c, mode, bk, bv, nb, pk, np, s, t, out_count, d_ok, d_ov, rid);

    // (total = the hit cursor, expected = the miss cursor)
    PairAttempt a;
    if (pair_open(c, make_plan(nb, top_bits, false), {!left ? REL_KEYS_ONLY : rid ? REL_POSITIONS : REL_VALUES, rid ? REL_POSITIONS : REL_KEYS_ONLY}, bk, bv, nb, pk, nullptr, np, top_bits, s, &a)) return 1;
    FjLdsJoinArgs ja{};
    ja.build = a.build; ja.probe = a.probe; ja.nparts = a.nparts;
    pair_items(a, np, &ja.items, &ja.nitems_dev, &ja.items_cap, &ja.nsplit);
    ja.err = &c->d_sc->err; ja.total = &c->d_sc->total;
    ja.out_cursor = &c->d_sc->total; ja.out_capacity = np; ja.out_keys = d_ok; ja.out_vals = left ? d_ov : nullptr;
    ja.row_ids = rid ? 1u : 0u;
    HIPCHK(fj_launch_outer_join(ja, (rid && left) ? FJ_OJ_LEFT_FIRST : mode, np, &c->d_sc->expected, s));
    if (pair_close(c, a, s, t)) return 1;
    if (left && !rid && !(c->h_sc->err & FJ_ERR_LDS_FULL) && (c->h_sc->err & FJ_STAT_DUPS)) {
        // duplicate build keys: the build side once more with row indices as payload, and the whole output rewritten
        if (pair_rerun_build_with_row_ids(c, &a, bk, nb, top_bits, nullptr, s)) return 1;
        ja.build = a.build; ja.orig_vals = bv;
        HIPCHK(fj_launch_outer_join(ja, FJ_OJ_LEFT_FIRST, np, &c->d_sc->expected, s));
        if (pair_close(c, a, s, t)) return 1;
    }
    if (c->h_sc->err & FJ_ERR_LDS_FULL)                      // a partition beyond the LDS table: the whole join on the HBM table
        return gt_fallback(t, [&](fj_timings* g) { return join_outer_global(c, mode, bk, bv, nb, pk, np, s, g, out_count, d_ok, d_ov, rid); });
    if (c->h_sc->err & FJ_ERR_OUTCAP) return set_err("internal error: the outer join kernel wrote out of its rows");
    const u64 hits = c->h_sc->total, misses = c->h_sc->expected;
    if (left ? hits + misses != np : misses > np) return set_err("internal error: outer join placed %llu + %llu of %zu probe rows", (unsigned long long)hits, (unsigned long long)misses, np);
    *out_count = left ? hits : misses;
    return 0;
}

// FJ_ALGO_FULL_OUTER (fj_join_device has checked the arguments; d_ok / d_ov hold np + nb rows).  The partitioned plan of the left join,
// run once: its kernel also marks the build rows it matched in a bitmap (one bit per row of the build side's final chunk pool, zeroed
// per launch), and a sweep over the build side's final chunk lists appends the rows left unmarked.  A partition without probe rows has
// no work item: its bits stay zero, all its rows are unmatched.  Duplicate build keys: as the left join, the whole output is rewritten
// with row indices on the build side - new chunk pools, so the bitmap is cleared and filled again.
int join_full(fj_ctx* c, bool use_radix, const u64* bk, const u64* bv, size_t nb, const u64* pk, size_t np, int top_bits,
              hipStream_t s, fj_timings* t, u64* out_counts, u64* d_ok, u64* d_ov, bool rid) {
    out_counts[0] = out_counts[1] = 0;
    if (nb == 0) return join_outer(c, FJ_OJ_LEFT, use_radix, bk, bv, nb, pk, np, top_bits, s, t, &out_counts[0], d_ok, d_ov, rid);
    if (np == 0) {                                           // every build row is unmatched
        float ms;
        if (trivial_done(c, s, &ms, [&]() -> int {
                if (rid) { HIPCHK(hipMemsetAsync(d_ok, 0xFF, nb * 8, s)); HIPCHK(fj_launch_iota(d_ov, nb, s)); }
                else {
                    HIPCHK(hipMemcpyAsync(d_ok, bk, nb * 8, hipMemcpyDeviceToDevice, s));
                    HIPCHK(hipMemcpyAsync(d_ov, bv, nb * 8, hipMemcpyDeviceToDevice, s));
                }
                return 0;
            })) return 1;
        t->path = use_radix ? 0 : 1; t->total_ms = t->emit_ms = ms;
        out_counts[1] = nb;
        return 0;
    }
    if (!use_radix) return join_outer_global(c, FJ_OJ_LEFT, bk, bv, nb, pk, np, s, t, &out_counts[0], d_ok, d_ov, rid, &out_counts[1]);

    // (total = the hit cursor, expected = the miss cursor, sample_hits = the sweep's)
    PairAttempt a;
    if (pair_open(c, make_plan(nb, top_bits, false), {rid ? REL_POSITIONS : REL_VALUES, rid ? REL_POSITIONS : REL_KEYS_ONLY}, bk, bv, nb, pk, nullptr, np, top_bits, s, &a)) return 1;
    FjLdsJoinArgs ja{};
    ja.build = a.build; ja.probe = a.probe; ja.nparts = a.nparts;
    pair_items(a, np, &ja.items, &ja.nitems_dev, &ja.items_cap, &ja.nsplit);
    ja.err = &c->d_sc->err; ja.total = &c->d_sc->total;
    ja.out_cursor = &c->d_sc->total; ja.out_capacity = np; ja.out_keys = d_ok; ja.out_vals = d_ov;
    ja.row_ids = rid ? 1u : 0u;
    const u64 out_cap = (u64)np + nb;
    // the join, then the sweep behind it on the same stream: one read-back serves both (a join that reports duplicates or a partition
    // beyond its table leaves rows behind row np that the rerun overwrites).  E_JOIN stands before the sweep: pair_close's second half
    auto join_and_sweep = [&](int mode) -> int {
        const size_t bit_bytes = (ja.build.list ? (size_t)ja.build.cap : (nb + FJ_CHUNK - 1) / FJ_CHUNK) * (FJ_CHUNK / 8);
        void* p;
        if (get_buf(c, W_FULL_BITS, bit_bytes, &p)) return 1;
        u64* bits = (u64*)p;
        HIPCHK(hipMemsetAsync(bits, 0, bit_bytes, s));
        HIPCHK(fj_launch_outer_join_full(ja, mode, np, &c->d_sc->expected, bits, s));
        HIPCHK(hipEventRecord(c->ev[E_JOIN], s));
        HIPCHK(hipEventRecord(c->ev[E_EMIT0], s));
        HIPCHK(fj_launch_full_sweep(ja.build, bits, ja.orig_vals, ja.row_ids, d_ok, d_ov, np, out_cap, &c->d_sc->sample_hits, &c->d_sc->err, s));
        HIPCHK(hipEventRecord(c->ev[E_EMIT1], s));
        return pair_read(c, a, s, t);
    };
    if (join_and_sweep(rid ? FJ_OJ_LEFT_FIRST : FJ_OJ_LEFT)) return 1;
    if (!rid && !(c->h_sc->err & FJ_ERR_LDS_FULL) && (c->h_sc->err & FJ_STAT_DUPS)) {
        // duplicate build keys: the build side once more with row indices as payload, and the whole output rewritten
        if (pair_rerun_build_with_row_ids(c, &a, bk, nb, top_bits, &c->d_sc->sample_hits, s)) return 1;
        ja.build = a.build; ja.orig_vals = bv;
        if (join_and_sweep(FJ_OJ_LEFT_FIRST)) return 1;
    }
    if (c->h_sc->err & FJ_ERR_LDS_FULL)                      // a partition beyond the LDS table: the whole join on the HBM table
        return gt_fallback(t, [&](fj_timings* g) { return join_outer_global(c, FJ_OJ_LEFT, bk, bv, nb, pk, np, s, g, &out_counts[0], d_ok, d_ov, rid, &out_counts[1]); });
    if (c->h_sc->err & FJ_ERR_OUTCAP) return set_err("internal error: the full outer join wrote out of its rows");
    const u64 hits = c->h_sc->total, misses = c->h_sc->expected, rest = c->h_sc->sample_hits;
    if (hits + misses != np || rest > nb) return set_err("internal error: full outer join placed %llu + %llu of %zu probe rows and %llu of %zu build rows",
                                                         (unsigned long long)hits, (unsigned long long)misses, np, (unsigned long long)rest, nb);
    t->emit_ms = ev_ms(c, E_EMIT0, E_EMIT1); t->total_ms += t->emit_ms;
    out_counts[0] = hits; out_counts[1] = rest;
    return 0;
}

}  // namespace fjh
