// Index arithmetic of DPR_ALGO_TILED for the smooth splat: the tile shapes, the tile of a point, the LDS cell of a
// deposit and the grid cell an LDS cell is flushed to.  Plain functions that compile for the device AND for the host:
// tests/smooth_tile_host_check.cpp runs them under the address and undefined-behaviour sanitizers on the CPU.
//
// WHO USES WHAT.  The tile shapes, SmoothTiles and smooth_tiles are the ones of the host plan and of every key and tile
// kernel.  smooth_tile_key, smooth_tile_origin, smooth_lds_axes and smooth_lds_decode are the written-down form of the
// arithmetic that the three key kernels and the seven tile kernels (dpr_smooth.hip, dpr_smooth_channels.hip,
// dpr_smooth_bodies.hip, dpr_sample_smooth_bodies.hip) each still carry as their own text, line for line the same
// rule.  The kernels were rewritten on these functions and put back: every family had rows of its probe's tiled column
// slower than with the kernels' own text, beyond the run-to-run noise (up to 5 % on densely filled 2-D tiles; figures
// and what the compiler did differently: profiles/smooth_tile_refactor.md).  A change to the rule is made here first, checked on
// the CPU, and then in the kernels' text.
//
// A workgroup owns a tile and keeps it, plus one halo cell on both sides of every axis, as f64 cells in LDS:
// 3-D 16 x 8 x 8 (18 x 10 x 10 cells, 14 400 bytes), 2-D 64 x 16 (66 x 18 cells, 9 504 bytes) -- ten workgroups and
// more per CU's 160 KB.  LDS cell l_d = (cell_d - org_d) + 1 per axis, column-major over the e_d + 2 cells of an axis.
//
// THE RULE the path rests on: a point is binned by its centre cell j0 (-1 .. n_d per axis, smooth_cell) CLAMPED into
// the grid.  The clamped cell lies on the tile, so every cell j0 - 1 .. j0 + 1 that is in the grid lies on the tile +
// halo: each of the point's 3^N deposits is either dropped because it is outside the grid, or lands in an LDS cell
// that smooth_lds_decode sends back to exactly that grid cell.
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

template <int NO> struct SmoothTileShape;
template <> struct SmoothTileShape<2> {
    static constexpr int e[2] = {64, 16};
};
template <> struct SmoothTileShape<3> {
    static constexpr int e[3] = {16, 8, 8};
};
template <int NO> constexpr int smooth_lds_cells() {
    int c = 1;
    for (int d = 0; d < NO; ++d) c *= SmoothTileShape<NO>::e[d] + 2;
    return c;
}

template <int NO> struct SmoothTiles {
    int nt[NO];     // tiles per axis
    int64_t tiles;  // their product
};
// (host only, the one function here without DPR_HD: the plan of the launchers and the host check call it, no kernel)
template <int NO> SmoothTiles<NO> smooth_tiles(const int64_t* grid) {
    SmoothTiles<NO> t;
    t.tiles = 1;
    for (int d = 0; d < NO; ++d) {
        const int e = SmoothTileShape<NO>::e[d];
        t.nt[d] = (int)((grid[d] + e - 1) / e);
        t.tiles *= t.nt[d];
    }
    return t;
}

// id of the tile (column-major over the tiles, axis 0 fastest) that holds centre cell j0 clamped into the grid
template <int NO> DPR_HD uint32_t smooth_tile_key(const int (&j0)[NO], const int (&n)[NO], const int (&nt)[NO]) {
    uint32_t key = 0, stride = 1;
#pragma unroll
    for (int d = 0; d < NO; ++d) {
        const int c = j0[d] < 0 ? 0 : (j0[d] >= n[d] ? n[d] - 1 : j0[d]);
        key += (uint32_t)(c / SmoothTileShape<NO>::e[d]) * stride;
        stride *= (uint32_t)nt[d];
    }
    return key;
}

// first cell of tile t
template <int NO> DPR_HD void smooth_tile_origin(uint32_t t, const int (&nt)[NO], int (&org)[NO]) {
#pragma unroll
    for (int d = 0; d < NO; ++d) {
        org[d] = (int)(t % (uint32_t)nt[d]) * SmoothTileShape<NO>::e[d];
        t /= (uint32_t)nt[d];
    }
}

// Per axis, for the three cells j0 - 1 .. j0 + 1: whether the cell is in the grid AND on the tile + halo of origin
// org, and its term of the LDS index (0 for a dropped cell).  A deposit is made where `in` holds on every axis, into
// the LDS cell that is the sum of the terms.
template <int NO> struct SmoothLdsAxes {
    int loff[NO][3];
    bool in[NO][3];
};
template <int NO>
DPR_HD SmoothLdsAxes<NO> smooth_lds_axes(const int (&j0)[NO], const int (&org)[NO], const int (&n)[NO]) {
    SmoothLdsAxes<NO> la;
    int lstride = 1;
#pragma unroll
    for (int d = 0; d < NO; ++d) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int c = j0[d] + k - 1, l = c - org[d] + 1;
            la.in[d][k] = c >= 0 && c < n[d] && l >= 0 && l < SmoothTileShape<NO>::e[d] + 2;
            la.loff[d][k] = la.in[d][k] ? l * lstride : 0;
        }
        lstride *= SmoothTileShape<NO>::e[d] + 2;
    }
    return la;
}

// The grid cell of LDS cell i in [0, smooth_lds_cells) of the tile at org: false where it is outside the grid (halo
// beyond an edge, or the part of a ragged last tile past it), else its column-major offset in the plane.  The offset
// accumulates only while the cell is in the grid: the product would overflow an int next to 2^31 cells.
template <int NO> DPR_HD bool smooth_lds_decode(int i, const int (&org)[NO], const int (&n)[NO], int& off) {
    int rest = i, stride = 1;
    bool in_grid = true;
    off = 0;
#pragma unroll
    for (int d = 0; d < NO; ++d) {
        const int ext = SmoothTileShape<NO>::e[d] + 2;
        const int c = org[d] + (rest % ext) - 1;
        rest /= ext;
        in_grid = in_grid && c >= 0 && c < n[d];
        off += in_grid ? c * stride : 0;
        stride *= n[d];
    }
    return in_grid;
}

}  // namespace dpr
