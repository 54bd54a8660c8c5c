// The un-permute map of the tiled pullback, kept per record RUN (Plan::run_map): what k_scatter_wc_runs writes into
// the `indices` and `slot_of` regions of the workspace and how k_unpermute_runs reads it back.  Plain functions that
// compile for the device AND for the host: tests/run_map_host_check.cpp runs the encoder and the decoder under the
// address and undefined-behaviour sanitizers on the CPU, against a counting sort of its own.
//
// The scatter orders the n_valid accepted points of a sub-chunk of S points (4096 fp32, 2048 fp64) by tile (the SORTED
// positions 0 .. n_valid - 1, ascending tile order) and gives the records of one tile consecutive slots, cur[tile] +
// rank.  The positions are cut into SEGMENTS of 64 (a wave of either kernel).  A RUN is the set of records of one tile
// inside one segment: its slots are consecutive, so a slot is stored once per run --
//
//   owner words   indices region, uint16 [g * S + i], for every position i < nloc of sub-chunk g:
//                   bits 0-11   the index inside the sub-chunk of the point that owns sorted position i
//                   bits 12-14  zero
//                   bit 15      set on the first position of a run: the first record of a tile, or i % 64 == 0
//                 positions n_valid .. nloc - 1 (rejected points own none) hold kRunNone: bit 15 clear, bits 12-14 set
//   run table     slot_of region, uint32 [g * S + seg * 64 + j]: the record slot of the first record of the j-th run
//                 of segment seg, j < (start bits of the segment).  The other entries are never written and never
//                 trusted.
//   decoding      inside the segment: j(i) = (number of start bits at positions <= i) - 1, start(i) = the last start
//                 position <= i, slot(i) = run_table[seg * 64 + j(i)] + (i - start(i))
//
// The scatter writes 2 + 4 (tiles' runs + S / 64) / S bytes per point instead of 2 + 4: 3.2 at C3, where a sub-chunk
// holds 1147 tiles' runs.  Cutting the runs at the segments is what lets a wave decode its 64 positions from its own
// loads: a table indexed by the run number inside the whole sub-chunk (2 + 4 * 1147 / 4096 = 3.1 bytes per point)
// needs the start bits of every earlier segment first -- a workgroup barrier and a scan in front of the gradient
// loads, which cost the un-permute more than the bytes saved (profiles/run_map_per_run.md).
//
// WHO USES WHAT.  scatter_wc_body<RUNS>: run_starts, run_owner_word, kRunNone and run_table_index on the ballot of
// its write-out.  k_unpermute_runs: run_owner_valid, run_owner_index and run_segment_decode on its ballots.
// run_map_encode / run_map_decode are the same steps written for one host thread: the form the CPU check runs.
#pragma once
#include <stdint.h>

#ifndef DPR_HD
#if defined(__HIPCC__)
#define DPR_HD __host__ __device__ __forceinline__
#else
#define DPR_HD inline
#endif
#endif

namespace dpr {

constexpr uint32_t kRunMapVersion = 2;  // mixed into plan_layout_id: 1 was a slot per sorted position
constexpr int kRunMaxSub = 4096;        // points per sub-chunk an owner word can index
constexpr int kRunSegment = 64;         // positions decoded together: one wave ballot
constexpr uint32_t kRunStart = 0x8000u, kRunOwnerBits = 0x0fffu, kRunSpare = 0x7000u;
constexpr uint16_t kRunNone = 0x7fffu;  // no record at this position

// sorted position sidx, held by the record of rank `rank` inside its (sub-chunk, tile): does a run start here?
DPR_HD bool run_starts(uint32_t sidx, uint32_t rank) { return rank == 0u || sidx % (uint32_t)kRunSegment == 0u; }
DPR_HD uint16_t run_owner_word(uint32_t lp, bool first) { return (uint16_t)((lp & kRunOwnerBits) | (first ? kRunStart : 0u)); }
DPR_HD bool run_owner_valid(uint32_t w) { return (w & kRunSpare) == 0u; }
template <int S> DPR_HD uint32_t run_owner_index(uint32_t w) {
    static_assert(S <= kRunMaxSub && (S & (S - 1)) == 0 && S % kRunSegment == 0, "an owner word holds 12 index bits");
    return w & (uint32_t)(S - 1);
}

// One segment, `starts` = the ballot of its start bits (bit l = position seg0 + l).
// Where the start at position i = seg0 + l puts its slot: entry (index inside the sub-chunk's table) ...
DPR_HD uint32_t run_table_index(uint32_t i, uint64_t starts, uint32_t l) {
    return i - l + (uint32_t)__builtin_popcountll(starts & ((1ull << l) - 1ull));
}
// ... and the decoding of position seg0 + l: j = the entry of the segment that holds the first slot of its run (always
// < 64), dist = the distance to the run's start.  False where no run has started at or before the position.
DPR_HD bool run_segment_decode(uint64_t starts, uint32_t l, uint32_t& j, uint32_t& dist) {
    const uint64_t upto = starts & (~0ull >> (63u - l));
    j = ((uint32_t)__builtin_popcountll(upto) - 1u) & 63u;
    dist = upto ? l - (63u - (uint32_t)__builtin_clzll(upto)) : 0u;
    return upto != 0ull;
}

// ---------------------------------------------------------------------------------------------- host form
// The map of one sub-chunk, by the phases of scatter_wc_body: tile[lp] in [0, NT) or -1 for a rejected point, lp <
// nloc <= S; cursor[NT] = the next free record slot of every tile, advanced as the scatter advances it.  Writes
// owner[0 .. nloc) and the table entries of the runs, dest[lp] = the record slot of point lp (untouched for a rejected
// one); returns the number of runs.
template <int S>
uint32_t run_map_encode(const int* tile, uint32_t nloc, int NT, uint32_t* cursor, uint16_t* owner, uint32_t* table,
                        uint32_t* dest, uint32_t* lhist /* [NT] scratch */, uint32_t* lrank /* [S] scratch */) {
    static_assert(S <= kRunMaxSub, "an owner word holds 12 index bits");
    uint32_t sorted_dest[S];
    for (int t = 0; t < NT; ++t) lhist[t] = 0;
    for (uint32_t lp = 0; lp < nloc; ++lp)  // a. rank inside (sub-chunk, tile)
        if (tile[lp] >= 0) lrank[lp] = lhist[tile[lp]]++;
    uint32_t n_valid = 0;  // b. exclusive scan
    for (int t = 0; t < NT; ++t) {
        const uint32_t cnt = lhist[t];
        lhist[t] = n_valid;
        n_valid += cnt;
    }
    for (uint32_t lp = 0; lp < nloc; ++lp) {  // c. owners in tile order
        if (tile[lp] < 0) continue;
        const uint32_t sidx = lhist[tile[lp]] + lrank[lp];
        owner[sidx] = run_owner_word(lp, run_starts(sidx, lrank[lp]));
        sorted_dest[sidx] = dest[lp] = cursor[tile[lp]] + lrank[lp];
    }
    uint32_t runs = 0;
    for (uint32_t seg0 = 0; seg0 < nloc; seg0 += kRunSegment) {  // d. a wave per segment
        uint64_t starts = 0;
        for (uint32_t l = 0; l < (uint32_t)kRunSegment && seg0 + l < nloc; ++l) {
            if (seg0 + l >= n_valid) owner[seg0 + l] = kRunNone;
            else if (owner[seg0 + l] & kRunStart) starts |= 1ull << l;
        }
        for (uint32_t l = 0; l < (uint32_t)kRunSegment; ++l)
            if (starts >> l & 1u) table[run_table_index(seg0 + l, starts, l)] = sorted_dest[seg0 + l];
        runs += (uint32_t)__builtin_popcountll(starts);
    }
    for (int t = 0; t < NT; ++t) {  // e.
        const uint32_t next = t + 1 < NT ? lhist[t + 1] : n_valid;
        cursor[t] += next - lhist[t];
    }
    return runs;
}

// Every sorted position i < nloc of a sub-chunk -> its record slot and owner, by the steps of k_unpermute_runs, segment
// by segment.  has[i] is false for a position without a record: a none word, a position before any start, a slot >= P.
// A table index never passes the position it serves, so it stays inside the sub-chunk's part of the region whatever
// the map holds.
template <int S>
void run_map_decode(const uint16_t* owner, const uint32_t* table, uint32_t nloc, uint64_t P, uint32_t* slot, uint32_t* lp,
                    bool* has) {
    for (uint32_t seg0 = 0; seg0 < nloc; seg0 += kRunSegment) {
        uint64_t starts = 0;
        for (uint32_t l = 0; l < (uint32_t)kRunSegment && seg0 + l < nloc; ++l)
            if (owner[seg0 + l] & kRunStart) starts |= 1ull << l;
        for (uint32_t l = 0; l < (uint32_t)kRunSegment && seg0 + l < nloc; ++l) {
            const uint32_t i = seg0 + l;
            uint32_t j, dist;
            has[i] = run_segment_decode(starts, l, j, dist) && run_owner_valid(owner[i]);
            if (!has[i]) continue;
            slot[i] = table[seg0 + j] + dist;
            lp[i] = run_owner_index<S>(owner[i]);
            has[i] = slot[i] < P;
        }
    }
}

}  // namespace dpr
