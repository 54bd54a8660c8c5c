// Index arithmetic of DPR_ALGO_ORDERED: sort keys on the extended grid, cell ranges on the sorted keys and the
// merge walk of one output cell.  Plain functions that compile for the device (dpr_ordered.hip) AND for the
// host: every loop bound of k_ord_gather comes from here, so tests/ordered_host_check.cpp runs the same code
// under the address and undefined-behaviour sanitizers on the CPU before any kernel reads through it.
//
// The EXTENDED grid has one more cell on the low side of every axis: a point's reference cell (the lower
// neighbour, ref0[d] in -1 .. n_d - 1) is extended cell ref0[d] + 1 in 0 .. n_d.  Its key is the column-major
// index of that cell, axis 0 fastest.  A rejected point carries the all-ones key.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DPR_HD __host__ __device__ __forceinline__
#else
#define DPR_HD inline
#endif

namespace dpr {

constexpr uint32_t kOrdNoKey = 0xffffffffu;    // a rejected point; sorts behind every cell
constexpr uint32_t kOrdNoPoint = 0xffffffffu;  // an exhausted list head; P <= 2^32 - 2, so no point has it

// cells of the extended grid, GE <= 2^32 - 1, or 0 when they do not fit the 32-bit key space (keys 0 .. GE - 1 must
// stay below kOrdNoKey)
template <int NO> DPR_HD uint64_t ord_ext_cells(const int (&n)[NO]) {
    uint64_t ge = 1;
    for (int d = 0; d < NO; ++d) {
        ge *= (uint64_t)(n[d] + 1);
        if (ge > (uint64_t)0xffffffffu) return 0;
    }
    return ge;
}

// key bits the radix sort has to look at: the smallest `bits` with 2^bits - 1 >= GE, so that the all-ones key
// of a rejected point, cut to `bits` bits, still sorts behind key GE - 1
DPR_HD int ord_key_bits(uint64_t ge) {
    int bits = 1;
    while (bits < 32 && (((uint64_t)1 << bits) - 1) < ge) ++bits;
    return bits;
}

template <int NO> DPR_HD uint32_t ord_key_encode(const int (&ref0)[NO], const int (&n)[NO]) {
    uint32_t key = 0, stride = 1;
    for (int d = 0; d < NO; ++d) {
        key += (uint32_t)(ref0[d] + 1) * stride;
        stride *= (uint32_t)(n[d] + 1);
    }
    return key;
}

template <int NO> DPR_HD void ord_key_decode(uint32_t key, const int (&n)[NO], int (&ref0)[NO]) {
    for (int d = 0; d < NO; ++d) {
        const uint32_t e = (uint32_t)(n[d] + 1);
        ref0[d] = (int)(key % e) - 1;
        key /= e;
    }
}

// coordinates of output cell `cell` (column-major, axis 0 fastest)
template <int NO> DPR_HD void ord_cell_coords(uint32_t cell, const int (&n)[NO], int (&c)[NO]) {
    for (int d = 0; d < NO; ++d) {
        c[d] = (int)(cell % (uint32_t)n[d]);
        cell /= (uint32_t)n[d];
    }
}

// The neighbour test: a point whose reference cell is ref0 reaches output cell c through neighbour s exactly
// when ref0[d] + bit_d(s) == c[d] on every axis, i.e. ref0 = c - shift(s).  For 0 <= c[d] < n[d] that source
// cell always lies on the extended grid (c[d] - 1 >= -1), so all 2^NO keys are valid.  Returns its key.
template <int NO> DPR_HD uint32_t ord_source_key(const int (&c)[NO], int s, const int (&n)[NO]) {
    int ref0[NO];
    for (int d = 0; d < NO; ++d) ref0[d] = c[d] - ((s >> d) & 1);
    return ord_key_encode<NO>(ref0, n);
}

// first position in the ascending keys[0 .. count) whose key is >= key (count if there is none).  Keys are
// compared on their low `bits` bits, as the sort orders them.
DPR_HD uint32_t ord_lower_bound(const uint32_t* keys, uint32_t count, uint32_t key, int bits) {
    const uint32_t mask = bits >= 32 ? 0xffffffffu : ((1u << bits) - 1u);
    uint32_t lo = 0, hi = count;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if ((keys[mid] & mask) < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// [begin, end) of extended cell `key` in the sorted order, from the start table (GE + 1 entries, start[k] =
// lower bound of key k, start[GE] = number of accepted points).  Clamped to `count` and to begin <= end: a
// damaged table can shorten a walk, never send it outside idx[0 .. count).
DPR_HD void ord_cell_range(const uint32_t* start, uint32_t key, uint32_t count, uint32_t& begin, uint32_t& end) {
    uint32_t b = start[key], e = start[key + 1];
    if (e > count) e = count;
    if (b > e) b = e;
    begin = b;
    end = e;
}

// The merge walk of output cell c: its candidates are the points of the 2^NO source cells c - shift(s); each
// list is ascending in point index (the sort is stable), the lists are disjoint, so taking the smallest head
// 2^NO ways visits the cell's contributions in ascending point index.  visit(point, s) is called once per
// contribution.  The loops are written over registers only (no indexing by a run-time value): the kernel must
// not spill them to scratch.
template <int NO, typename Visit>
DPR_HD void ord_merge_walk(const int (&c)[NO], const int (&n)[NO], const uint32_t* start, const uint32_t* idx,
                           uint32_t count, Visit visit) {
    constexpr int NS = 1 << NO;
    uint32_t pos[NS], end[NS], head[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        ord_cell_range(start, ord_source_key<NO>(c, s, n), count, pos[s], end[s]);
        head[s] = pos[s] < end[s] ? idx[pos[s]] : kOrdNoPoint;
    }
    for (;;) {
        uint32_t best = kOrdNoPoint;
        int bs = 0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const bool take = head[s] < best;
            best = take ? head[s] : best;
            bs = take ? s : bs;
        }
        if (best == kOrdNoPoint) break;
        visit(best, bs);
        // advance list bs: one load, placed with selects
        uint32_t np = 0, ne = 0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            np = s == bs ? pos[s] + 1u : np;
            ne = s == bs ? end[s] : ne;
        }
        const uint32_t nh = np < ne ? idx[np] : kOrdNoPoint;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            pos[s] = s == bs ? np : pos[s];
            head[s] = s == bs ? nh : head[s];
        }
    }
}

}  // namespace dpr
