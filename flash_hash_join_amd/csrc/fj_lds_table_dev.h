// fj_lds_table_dev.h -- what the extension kernels that keep a linear-probing LDS table share (csrc/fj_group.hip, fj_groupby.hip,
// fj_groupby_multi.hip, fj_groupby_arg.hip, fj_groupby_merge.hip, fj_groupby_pair.hip, fj_groupby_rows.hip, fj_aligned.hip, fj_prepared.hip, fj_outer.hip, fj_many.hip; csrc/fj_join.hip takes fj_chunk_entry): the decoding of chunk lists and
// work items every one of them starts with, and, stated once, the table they all build.
//
// THE TABLE: TS slots (a power of two) of 64-bit MIXED keys in LDS, all FJ_EMPTY_KEY at rest.  A key's home slot is
// FJ_HW2(key) & (TS - 1), the next slot (pos + 1) & (TS - 1); a slot is claimed by one 64-bit compare-and-swap and never changes
// afterwards.  The empty marker itself is never stored: every kernel keeps it out of band.
//   - An insert walks at most TS steps (`for (step = 0; step < TS; ++step)`; a key without a slot raises hdr->full) - except in
//     csrc/fj_many.hip, which offers at most MM_ROWS < MM_S rows to its table and walks until it finds a slot.
//   - Inserts never run concurrently with lookups on one table: a barrier separates them.
//   - A lookup walks until the key or an empty slot.  It runs only while at least one slot is empty: behind `if (hdr->full) return`,
//     with full raised at LIMIT = TS - TS / 16 keys (fj_many.hip: MM_ROWS < MM_S).
//   - The flush / sweep walks (`while (tkeys[pos] != key)`) are for keys the build phase put into that same table.
// The loops themselves stay in the kernels.  As shared __forceinline__ helpers (insert, read-then-CAS insert, find, find-placed)
// they changed register counts, spills or occupancy of most kernels, and where they did not, the probe and stream loops ran
// measurably slower (DESIGN.md "Shared decoding of the extension kernels"); tests/test_table_collisions.py pins every copy.
#pragma once
#include "fj_internal.h"

// encoded chunk-list entry ((count-1) << 24 | id) of chunk `idx`; a flat array is read as a virtual chunk list
__device__ __forceinline__ u32 fj_chunk_entry(const FjChunkSet& cs, u32 idx) {
    if (cs.list) return cs.list[idx];
    const u64 rem = cs.n_flat - (u64)idx * FJ_CHUNK;
    const u32 cnt = rem >= FJ_CHUNK ? FJ_CHUNK : (u32)rem;
    return ((cnt - 1u) << 24) | idx;
}

// work item -> partition p and the probe chunk-list range [s_lo, s_hi): an entry of the item table (chunk-list probe side), or one of
// nsplit equal slices of the flat probe side.  false: the item lies beyond *nitems_dev.  An empty slice is the caller's to skip
__device__ __forceinline__ bool fj_item_slice(const uint4* items, const u32* nitems_dev, u32 nsplit, u64 probe_n_flat, u32 item,
                                              u32& p, u32& s_lo, u32& s_hi) {
    if (items) {
        if (item >= *nitems_dev) return false;
        const uint4 it = items[item];
        p = it.z; s_lo = it.x; s_hi = it.x + it.y;
    } else {
        const u32 slice = item % nsplit;
        p = item / nsplit;
        const u32 npc = (u32)((probe_n_flat + FJ_CHUNK - 1) >> FJ_CHUNK_LOG);
        s_lo = (u32)(((u64)slice * npc) / nsplit); s_hi = (u32)(((u64)(slice + 1) * npc) / nsplit);
    }
    return true;
}

// partition p's chunks: entries [b0, b0 + nbc) of the chunk list, or all virtual chunks of a flat array
__device__ __forceinline__ void fj_part_chunks(const FjChunkSet& cs, u32 p, u32& b0, u32& nbc) {
    b0 = 0;
    if (cs.list) { b0 = cs.boff[p]; nbc = cs.boff[p + 1] - b0; }
    else nbc = (u32)((cs.n_flat + FJ_CHUNK - 1) >> FJ_CHUNK_LOG);
}
