// fj_group.hip -- build-order aggregate joins (an EXTENSION: FJ_ALGO_BUILD_ORDER, include/flashjoin.h): one output word per BUILD row,
// at the build row's position.  counts[i] = the probe rows whose key equals build key i, sums[i] = the sum (mod 2^64) of a probe-side
// value column over those rows: the join that feeds a GROUP BY on the build side, without the pairs in between.
//
// Like the probe-order joins (csrc/fj_aligned.hip) its size and layout are known before it starts, so nothing is reserved and nothing
// stays pending.  The build side carries its rows' positions through the passes (PassIter::vals_pos); the probe side carries its
// values when sums are asked for and NOTHING when only counts are (the keys-only pass).  Per work item the join kernel builds the
// partition's distinct keys into the 8192-slot LDS table with one 8-byte accumulator per slot (128 KiB), streams the slice's probe
// rows adding 1 or the row's value to the slot with an LDS atomic, and then walks the partition's build rows again: every row looks
// its slot up and adds a non-zero accumulator to out[position] with a global atomic (a partition may be cut into several items; the
// outputs are zeroed once per call).  Every copy of a duplicated build key reads the same slot, so it receives the same aggregate.
//
// Both outputs in one call: the passes run once and the kernel is launched twice over the same partitions, once per accumulator (keys
// plus two accumulators would be 192 KiB of LDS).
//
// P, the sum of all counts: the count form adds up what it flushes.  The sum form keeps no counts; it counts its hits, which is P when
// the partition's build keys are distinct, and reports duplicates (FJ_STAT_DUPS) otherwise - the host then runs the count form once
// without an output, for P alone.
//
// Min / max (FJ_ALGO_AGG_MIN / FJ_ALGO_AGG_MAX, unsigned or FJ_ALGO_AGG_SIGNED): the same kernel with another aggregate parameter.  The
// accumulators and the output start at the aggregate's identity (UINT64_MAX, INT64_MAX, 0, INT64_MIN) instead of zero - a memset where
// that is a byte pattern, a fill kernel where it is not - a hit is one native 64-bit LDS atomic min / max of the value's own signedness,
// the flush skips a slot that still holds the identity and combines the others into out[position] with the matching global atomic.  No
// pass over the outputs afterwards.  P and the duplicates are handled as in the sum form.
//
// Float aggregates (FJ_ALGO_AGG_FLOAT: FJ_GJ_SUM_F / FJ_GJ_MIN_F / FJ_GJ_MAX_F): three more aggregate parameters of the same kernels.  The
// values and accumulators are IEEE-754 binary64 in the same 8-byte words; the sum is one native f64 atomic add per hit (LDS) and per
// flushed row (HBM), min / max one integer atomic on the raw bits chosen by the value's sign bit (gj_combine, csrc/fj_group_dev.h);
// identities +0.0, +inf, -inf.  Every word they touch is LDS or device memory of the call (DESIGN.md "Float aggregates").
//
// Fallback: FJ_ERR_LDS_FULL; the HBM-table kernels end this file.
#include "fj_host.h"
#include "fj_group_dev.h"

namespace {

struct GjHdr { u32 full, dups, empty_cnt, nkeys, hits, pad0; u64 empty_acc, total; };

// AGG (FJ_GJ_*): FJ_GJ_COUNT adds 1 per row; every other form takes the probe rows' values (a.probe.vals) - FJ_GJ_SUM adds them, the
// four min / max forms combine them with gj_combine.  out: nb words holding the aggregate's identity before the launch (zeroed for
// count and sum; nullptr, count form only: nothing is flushed, the launch is for P alone).  a.total (may be null) receives P - count
// form: what the flush read; the forms with values: the hits, and FJ_STAT_DUPS tells the host that this is not P.
template <int AGG>
__global__ __launch_bounds__(GJ_NT, 1) void fj_group_join_kernel(FjLdsJoinArgs a, u64* __restrict__ out, u64 nb) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    GjHdr* hdr = reinterpret_cast<GjHdr*>(smem);
    u64* tkeys = reinterpret_cast<u64*>(smem + sizeof(GjHdr));
    u64* acc = tkeys + GJ_TS;
    constexpr bool SUM = AGG != FJ_GJ_COUNT;                 // the probe side carries values; hits are counted instead of counts flushed
    constexpr bool MINMAX = AGG >= FJ_GJ_MIN_U && AGG != FJ_GJ_SUM_F;
    constexpr u64 IDENT = gj_identity<AGG>();
    const u32 tid = threadIdx.x, lane = tid & 63;
    const u32 item = blockIdx.x;
    u32 p, b0, nbc, s_lo, s_hi;
    if (!fj_item_slice(a.items, a.nitems_dev, a.nsplit, a.probe.n_flat, item, p, s_lo, s_hi) || s_lo >= s_hi) return;
    fj_part_chunks(a.build, p, b0, nbc);

    for (u32 i = tid; i < GJ_TS; i += GJ_NT) { tkeys[i] = FJ_EMPTY_KEY; acc[i] = IDENT; }
    if (tid == 0) { hdr->full = 0; hdr->dups = 0; hdr->empty_cnt = 0; hdr->nkeys = 0; hdr->hits = 0; hdr->empty_acc = IDENT; hdr->total = 0; }
    __syncthreads();

    // ---- build: distinct keys; a copy finds its key in place ----
    for (u32 c0 = 0; c0 < nbc; c0 += GJ_NT / FJ_CHUNK) {
        const u32 c = c0 + tid / FJ_CHUNK, off = tid % FJ_CHUNK;
        if (c >= nbc) continue;
        const u32 e = fj_chunk_entry(a.build, b0 + c);
        if (off >= FJ_LIST_CNT(e)) continue;
        const u64 src = (u64)FJ_LIST_ID(e) * FJ_CHUNK + off;
        const u64 key = a.build.list ? a.build.keys[src] : fj_key_mix(a.build.keys[src]);   // chunk pools hold mixed keys, flat arrays raw ones
        if (key == FJ_EMPTY_KEY) {                           // the empty marker is never stored in the table
            if (atomicAdd(&hdr->empty_cnt, 1u) != 0 && SUM) hdr->dups = 1;
            continue;
        }
        u32 pos = FJ_HW2(key) & (GJ_TS - 1);
        bool placed = false;
        for (u32 step = 0; step < GJ_TS; ++step) {
            const u64 old = atomicCAS((unsigned long long*)&tkeys[pos], (unsigned long long)FJ_EMPTY_KEY, (unsigned long long)key);
            if (old == FJ_EMPTY_KEY) {
                if (atomicAdd(&hdr->nkeys, 1u) >= GJ_LIMIT) hdr->full = 1;
                placed = true;
                break;
            }
            if (old == key) { if (SUM) hdr->dups = 1; placed = true; break; }
            pos = (pos + 1) & (GJ_TS - 1);
        }
        if (!placed) hdr->full = 1;
    }
    __syncthreads();
    if (hdr->full) { if (tid == 0) atomicOr(a.err, FJ_ERR_LDS_FULL); return; }     // the host re-runs the join on the HBM table
    const bool has_empty = hdr->empty_cnt != 0;

    // ---- probe: rounds of GJ_NT * GJ_KPT rows; the next round's loads are requested before this round's lookups.  A hit adds to
    // its slot's accumulator in LDS (min / max: combines with it): no global traffic ----
    u64 k[GJ_KPT], pv[SUM ? GJ_KPT : 1];
    u32 okm = 0, nh = 0;                                     // nh: wave-uniform count of this wave's hits (SUM)
    auto load_round = [&](u32 pc, u64 (&kk)[GJ_KPT], u64 (&vv)[SUM ? GJ_KPT : 1], u32& ok) {
        ok = 0;
#pragma unroll
        for (u32 u = 0; u < GJ_KPT; ++u) {
            const u32 c = pc + u * (GJ_NT / FJ_CHUNK) + tid / FJ_CHUNK, off = tid % FJ_CHUNK;
            kk[u] = 0; if (SUM) vv[SUM ? u : 0] = 0;
            if (c >= s_hi) continue;
            const u32 e = fj_chunk_entry(a.probe, c);
            if (off >= FJ_LIST_CNT(e)) continue;
            const u64 src = (u64)FJ_LIST_ID(e) * FJ_CHUNK + off;
            kk[u] = a.probe.keys[src];
            if (SUM) vv[SUM ? u : 0] = a.probe.vals[src];
            ok |= 1u << u;
        }
    };
    load_round(s_lo, k, pv, okm);
    for (u32 pc = s_lo; pc < s_hi; pc += GJ_ROUND_CHUNKS) {
        u64 kn[GJ_KPT], pvn[SUM ? GJ_KPT : 1];
        u32 okn = 0;
        if (pc + GJ_ROUND_CHUNKS < s_hi) load_round(pc + GJ_ROUND_CHUNKS, kn, pvn, okn);
#pragma unroll
        for (u32 u = 0; u < GJ_KPT; ++u) {
            bool h = false;
            if ((okm >> u) & 1u) {
                const u64 key = a.probe.list ? k[u] : fj_key_mix(k[u]);
                const unsigned long long add = SUM ? (unsigned long long)pv[SUM ? u : 0] : 1ull;
                if (key == FJ_EMPTY_KEY) {
                    h = has_empty;
                    if (h) gj_combine<AGG>(&hdr->empty_acc, add);
                } else {
                    u32 pos = FJ_HW2(key) & (GJ_TS - 1);
                    for (;;) {                               // the build left >= 1/16 of the slots empty: always terminates
                        const u64 t = tkeys[pos];
                        if (t == key) { h = true; gj_combine<AGG>(&acc[pos], add); break; }
                        if (t == FJ_EMPTY_KEY) break;
                        pos = (pos + 1) & (GJ_TS - 1);
                    }
                }
            }
            if (SUM) nh += (u32)__popcll(__ballot(h));
        }
#pragma unroll
        for (u32 u = 0; u < GJ_KPT; ++u) { k[u] = kn[u]; if (SUM) pv[SUM ? u : 0] = pvn[SUM ? u : 0]; }
        okm = okn;
    }
    if (SUM && lane == 0 && nh) atomicAdd(&hdr->hits, nh);
    __syncthreads();

    // ---- flush: the partition's build rows once more; every copy of a key reads the same slot ----
    u64 flushed = 0;
    if (out || !SUM) {
        const u64 empty_acc = hdr->empty_acc;
        for (u32 c0 = 0; c0 < nbc; c0 += GJ_NT / FJ_CHUNK) {
            const u32 c = c0 + tid / FJ_CHUNK, off = tid % FJ_CHUNK;
            if (c >= nbc) continue;
            const u32 e = fj_chunk_entry(a.build, b0 + c);
            if (off >= FJ_LIST_CNT(e)) continue;
            const u64 src = (u64)FJ_LIST_ID(e) * FJ_CHUNK + off;
            const u64 key = a.build.list ? a.build.keys[src] : fj_key_mix(a.build.keys[src]);
            u64 v = empty_acc;
            if (key != FJ_EMPTY_KEY) {
                u32 pos = FJ_HW2(key) & (GJ_TS - 1);
                while (tkeys[pos] != key) pos = (pos + 1) & (GJ_TS - 1);      // (the build phase placed it)
                v = acc[pos];
            }
            if (v == IDENT) continue;                        // (count, sum: 0 adds nothing; min / max: out[] holds the identity already)
            if (!SUM && !MINMAX) flushed += v;               // (the count form's total: never a value's bits)
            if (!out) continue;
            const u64 o = a.build.vals ? a.build.vals[src] : src;             // (zero-pass plan: the flat index IS the position)
            if (o < nb) gj_combine<AGG>(&out[o], v);                          // (always: positions are 0 .. nb - 1)
            else atomicOr(a.err, FJ_ERR_OUTCAP);
        }
    }
    if (!a.total) return;
    if (SUM) {
        if (tid == 0) {
            if (hdr->hits) atomicAdd(a.total, (unsigned long long)hdr->hits);
            if (hdr->dups) atomicOr(a.err, FJ_STAT_DUPS);
        }
    } else {
        flushed = gj_wave_sum64(flushed);
        if (lane == 0 && flushed) atomicAdd((unsigned long long*)&hdr->total, (unsigned long long)flushed);
        __syncthreads();
        if (tid == 0 && hdr->total) atomicAdd(a.total, (unsigned long long)hdr->total);
    }
}

// ---- the global-table form (gj_gt_find: csrc/fj_group_dev.h) ----
// thread per probe row: a hit adds 1 to cnt[slot] and (sum != nullptr) combines the row's value into sum[slot]: AGG = FJ_GJ_SUM adds
// it, the min / max forms take the typed global atomic (sum[] then starts at the aggregate's identity, not at zero)
template <int AGG>
__global__ __launch_bounds__(1024) void fj_gt_group_probe_kernel(FjGtArgs a, const u64* __restrict__ pv, unsigned long long* cnt, unsigned long long* sum) {
    const bool has_empty = a.flags[0] != 0;
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < a.np; i += stride) {
        const u64 key = a.pk[i];
        u64 where = a.cap_mask + 1;
        if (key == FJ_EMPTY_KEY ? !has_empty : !gj_gt_find(a.tkeys, a.cap_mask, key, where)) continue;
        atomicAdd(&cnt[where], 1ull);
        if (sum) gj_combine<AGG>((u64*)&sum[where], pv[i]);
    }
}

// thread i per build row i: out_cnt[i] / out_sum[i] = the slot's accumulators (coalesced stores, every row: a row without a partner
// reads what sum[] was filled with, the aggregate's identity); a.total += the counts
__global__ __launch_bounds__(1024) void fj_gt_group_flush_kernel(FjGtArgs a, const unsigned long long* cnt, const unsigned long long* sum,
                                                                 u64* __restrict__ out_cnt, u64* __restrict__ out_sum) {
    __shared__ unsigned long long s_total;
    const u32 tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) s_total = 0;
    __syncthreads();
    u64 mine = 0;
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + tid; i < a.nb; i += stride) {
        const u64 key = a.bk[i];
        u64 where = a.cap_mask + 1;
        if (key != FJ_EMPTY_KEY) gj_gt_find(a.tkeys, a.cap_mask, key, where);     // (the build placed it)
        const u64 n = cnt[where];
        mine += n;
        if (out_cnt) out_cnt[i] = n;
        if (out_sum) out_sum[i] = sum[where];
    }
    mine = gj_wave_sum64(mine);
    if (lane == 0 && mine) atomicAdd(&s_total, (unsigned long long)mine);
    __syncthreads();
    if (tid == 0 && s_total) atomicAdd(a.total, s_total);
}

// out[i] = v for i < n: the identities that are no byte pattern (INT64_MAX, INT64_MIN, the bits of +inf and -inf)
__global__ __launch_bounds__(256) void fj_fill64_kernel(u64* __restrict__ out, u64 v, u64 n) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = v;
}

}  // namespace

u64 fj_group_identity(int agg) {
    if (agg < FJ_GJ_COUNT || agg > FJ_GJ_LAST) return 0;
    return fjh::for_agg(agg, [](auto A) { return gj_identity<FJ_V(A)>(); });
}

hipError_t fj_launch_group_fill(u64* out, u64 n, int agg, hipStream_t s) {
    if (!n) return hipSuccess;
    const u64 v = fj_group_identity(agg);
    if (v == 0 || v == ~0ull) return hipMemsetAsync(out, v ? 0xFF : 0, n * 8, s);
    const u64 blocks = (n + 256 * 8 - 1) / (256 * 8);                             // ~8 words per thread, at most 4096 workgroups
    hipLaunchKernelGGL(fj_fill64_kernel, dim3((u32)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, out, v, n);
    return hipGetLastError();
}

hipError_t fj_launch_group_join(const FjLdsJoinArgs& a, int agg, u64* out, u64 nb, hipStream_t s) {
    const u32 grid = a.items ? a.items_cap : a.nparts * a.nsplit;
    const bool vals = agg != FJ_GJ_COUNT;
    if (agg < FJ_GJ_COUNT || agg > FJ_GJ_LAST) return hipErrorInvalidValue;
    if (!a.err || (!out && (vals || !a.total))) return hipErrorInvalidValue;
    if (vals && !a.probe.vals) return hipErrorInvalidValue;                       // the probe side carries the values
    const u32 lds = (u32)sizeof(GjHdr) + GJ_TS * 16u;
    void (*kern)(FjLdsJoinArgs, u64*, u64) = fjh::for_agg(agg, [](auto A) { return fj_group_join_kernel<FJ_V(A)>; });
    hipError_t e = fj_set_max_lds_once(reinterpret_cast<const void*>(kern), lds);
    if (e != hipSuccess) return e;
    if (grid) hipLaunchKernelGGL(kern, dim3(grid), dim3(GJ_NT), lds, s, a, out, nb);
    return hipGetLastError();
}

hipError_t fj_launch_gt_group(const FjGtArgs& a, int agg, const u64* pv, unsigned long long* cnt, unsigned long long* sum, u64* out_cnt, u64* out_sum, hipStream_t s) {
    if (!a.total || !cnt || (!out_cnt && !out_sum) || (out_sum && (!sum || !pv))) return hipErrorInvalidValue;
    if (agg < FJ_GJ_COUNT || agg > FJ_GJ_LAST || (out_sum && agg == FJ_GJ_COUNT)) return hipErrorInvalidValue;
    if (a.np) {
        void (*probe)(FjGtArgs, const u64*, unsigned long long*, unsigned long long*) =
            fjh::for_value_agg(agg, [](auto A) { return fj_gt_group_probe_kernel<FJ_V(A)>; });     // (the count form: sum == nullptr)
        hipLaunchKernelGGL(probe, dim3(fjh::gt_grid(a.np)), dim3(1024), 0, s, a, pv, cnt, out_sum ? sum : nullptr);
    }
    if (a.nb) hipLaunchKernelGGL(fj_gt_group_flush_kernel, dim3(fjh::gt_grid(a.nb)), dim3(1024), 0, s, a, cnt, sum, out_cnt, out_sum);
    return hipGetLastError();
}

namespace fjh {

// the global-table form (fj_host.h).  Counts are always kept (P is their sum over the build rows)
// agg: what d_sum receives (FJ_GJ_SUM or a min / max form); its accumulators start at the aggregate's identity, the empty key's too
static int join_group_global(fj_ctx* c, const u64* bk, size_t nb, const u64* pk, const u64* pv, size_t np, hipStream_t s,
                             fj_timings* t, u64* out_count, u64* d_cnt, u64* d_sum, int agg) {
    const u64 cap = gt_capacity(nb);
    const size_t acc_words = (d_sum ? 2 : 1) * (cap + 1);
    FjGtArgs a{};
    u64* acc = nullptr;
    if (gt_open(c, nb, acc_words, s, &a, &acc)) return 1;
    unsigned long long* cnt = (unsigned long long*)acc;
    unsigned long long* sum = d_sum ? cnt + cap + 1 : nullptr;
    a.bk = bk; a.pk = pk; a.np = np;
    const bool own_fill = sum && fj_group_identity(agg) != 0;                    // (sum, unsigned max: one memset serves both arrays)
    HIPCHK(hipMemsetAsync(cnt, 0, (own_fill ? cap + 1 : acc_words) * 8, s));
    if (own_fill) HIPCHK(fj_launch_group_fill((u64*)sum, cap + 1, agg, s));
    HIPCHK(fj_launch_gt_build_first(a, false, s));
    HIPCHK(hipEventRecord(c->ev[E_BUILD], s));
    HIPCHK(hipEventRecord(c->ev[E_PPART], s));
    HIPCHK(fj_launch_gt_group(a, d_sum ? agg : FJ_GJ_COUNT, pv, cnt, sum, d_cnt, d_sum, s));
    if (gt_close(c, s, t)) return 1;
    *out_count = c->h_sc->total;
    return 0;
}

// FJ_ALGO_BUILD_ORDER (fj_join_device has checked the arguments): d_cnt[i] and / or d_sum[i] (nb words each, either may be null) for
// every build row i; pv: the probe side's value column (np words; read only when d_sum is asked for); agg: the aggregate d_sum holds
// (FJ_GJ_SUM, or a min / max form: FJ_ALGO_AGG_MIN / FJ_ALGO_AGG_MAX); *out_count = P, the sum of all counts.  use_radix: the
// partitioned plan, else the global table.  d_sum is filled with the aggregate's identity on the stream before the kernel combines into
// it, so every word below nb is defined by the call and a row without a partner reads the identity.
int join_group(fj_ctx* c, bool use_radix, const u64* bk, size_t nb, const u64* pk, const u64* pv, size_t np, int top_bits,
               hipStream_t s, fj_timings* t, u64* out_count, u64* d_cnt, u64* d_sum, int agg) {
    *out_count = 0;
    if (nb == 0) return 0;
    if (np == 0) {                                           // no build row has a partner
        float ms;
        if (trivial_done(c, s, &ms, [&]() -> int {
                if (d_cnt) HIPCHK(hipMemsetAsync(d_cnt, 0, nb * 8, s));
                if (d_sum) HIPCHK(fj_launch_group_fill(d_sum, nb, agg, s));
                return 0;
            })) return 1;
        t->path = use_radix ? 0 : 1; t->total_ms = t->join_ms = t->probe_phase_ms = ms;
        return 0;
    }
    if (!use_radix) return join_group_global(c, bk, nb, pk, pv, np, s, t, out_count, d_cnt, d_sum, agg);

    // the build rows' positions travel through the passes; the count form alone: the probe side's keys-only pass
    PairAttempt a;
    if (pair_open(c, make_plan(nb, top_bits, false), {REL_POSITIONS, d_sum ? REL_VALUES : REL_KEYS_ONLY}, bk, nullptr, nb, pk, pv, np, top_bits, s, &a)) return 1;
    FjLdsJoinArgs ja{};
    ja.build = a.build; ja.probe = a.probe; ja.nparts = a.nparts;
    pair_items(a, np, &ja.items, &ja.nitems_dev, &ja.items_cap, &ja.nsplit);
    ja.err = &c->d_sc->err;
    if (d_cnt) {
        ja.total = &c->d_sc->total;
        HIPCHK(hipMemsetAsync(d_cnt, 0, nb * 8, s));
        HIPCHK(fj_launch_group_join(ja, FJ_GJ_COUNT, d_cnt, nb, s));
    }
    if (d_sum) {
        ja.total = d_cnt ? nullptr : &c->d_sc->total;        // (the count launch has P)
        HIPCHK(fj_launch_group_fill(d_sum, nb, agg, s));
        HIPCHK(fj_launch_group_join(ja, agg, d_sum, nb, s));
    }
    if (pair_close(c, a, s, t)) return 1;
    if (!d_cnt && !(c->h_sc->err & FJ_ERR_LDS_FULL) && (c->h_sc->err & FJ_STAT_DUPS)) {
        // sums (minima, maxima) alone over duplicated build keys: the hits are not P.  The count form once, without an output, for P
        HIPCHK(hipMemsetAsync(&c->d_sc->total, 0, sizeof(unsigned long long), s));
        ja.total = &c->d_sc->total;
        HIPCHK(fj_launch_group_join(ja, FJ_GJ_COUNT, nullptr, nb, s));
        if (pair_close(c, a, s, t)) return 1;
    }
    if (c->h_sc->err & FJ_ERR_LDS_FULL)                      // a partition beyond the LDS table: the whole join on the HBM table
        return gt_fallback(t, [&](fj_timings* g) { return join_group_global(c, bk, nb, pk, pv, np, s, g, out_count, d_cnt, d_sum, agg); });
    if (c->h_sc->err & FJ_ERR_OUTCAP) return set_err("internal error: a build row's position lies beyond the build side");
    *out_count = c->h_sc->total;
    return 0;
}

}  // namespace fjh
