// Host run of the index arithmetic of the smooth DPR_ALGO_TILED path (csrc/dpr_smooth_tile.h: tile key, tile origin,
// LDS axes of a point's 3^N cells, decode of an LDS cell at the flush) -- the written-down form of the rule every key
// and tile kernel of the smooth families follows.  tests/test_smooth_tile_host.py builds this file with
// -fsanitize=address,undefined and runs it as a child process.  No input: every tile, every centre cell and every LDS
// cell of a fixed list of grids is visited.  Per grid it checks
//   1. key(origin(t)) == t for every tile t,
//   2. key(j0) < tiles for every centre cell j0 in [-1, n_d] per axis (the range of smooth_cell),
//   3. for every centre j0, against the origin of ITS tile, and each of its 3^N cells c: c in the grid => `in` holds
//      on every axis, the LDS cell l is in [0, NC) and decodes to "in the grid" at exactly the column-major offset of
//      c; c outside the grid => the combined `in` is false; a dropped cell has offset term 0,
//   4. for every tile and every LDS cell i < NC: the decode says "outside the grid" or gives an offset in [0, G), and
//      no two i of a tile give the same offset.
// Exit status: 0 all grids pass, 1 a statement failed (named on stderr), 2 bad arguments.  `--shifted-origins` (for
// the test of the checker itself) moves every origin one cell up on every axis, on the host only.  Deposit and flush
// still agree with each other (both use the shifted origin); what disagrees is the key and the origin: a point binned
// by the key meets a tile + halo that misses its lowest cells.  Grids of one tile per axis still pass; from (65, 17)
// on a cell of the grid falls off its tile + halo and the program must exit 1 on statement 3.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../diffpointrasterisation.jl_amd/csrc/dpr_smooth_tile.h"

using namespace dpr;

static bool g_shifted_origins = false;

template <int NO> static void origin(uint32_t t, const int (&nt)[NO], int (&org)[NO]) {
    smooth_tile_origin<NO>(t, nt, org);
    if (g_shifted_origins)
        for (int d = 0; d < NO; ++d) org[d] += 1;
}

template <int NO> static int fail(int statement, const int64_t (&grid)[NO], const char* what, long long a, long long b) {
    fprintf(stderr, "grid (");
    for (int d = 0; d < NO; ++d) fprintf(stderr, "%s%lld", d ? ", " : "", (long long)grid[d]);
    fprintf(stderr, "): statement %d: %s (%lld, %lld)\n", statement, what, a, b);
    return 1;
}

// f(c) for every c with lo[d] <= c[d] <= hi[d], axis 0 fastest; stops at the first non-zero result and returns it
template <int NO, typename F> static int for_each_cell(const int (&lo)[NO], const int (&hi)[NO], F f) {
    int c[NO];
    for (int d = 0; d < NO; ++d) c[d] = lo[d];
    for (;;) {
        if (int rc = f(c)) return rc;
        int d = 0;
        while (d < NO && ++c[d] > hi[d]) { c[d] = lo[d]; ++d; }
        if (d == NO) return 0;
    }
}

template <int NO> static int run(const int64_t (&grid)[NO]) {
    constexpr int NC = smooth_lds_cells<NO>();
    int n[NO];
    int64_t G = 1;
    for (int d = 0; d < NO; ++d) { n[d] = (int)grid[d]; G *= grid[d]; }
    const SmoothTiles<NO> tl = smooth_tiles<NO>(grid);

    // 1. the key of a tile's first cell is the tile
    for (uint32_t t = 0; t < (uint32_t)tl.tiles; ++t) {
        int org[NO];
        origin<NO>(t, tl.nt, org);
        const uint32_t key = smooth_tile_key<NO>(org, n, tl.nt);
        if (key != t) return fail<NO>(1, grid, "key(origin(t)) != t", key, t);
    }

    int lo[NO], hi[NO], klo[NO], khi[NO];
    for (int d = 0; d < NO; ++d) { lo[d] = -1; hi[d] = n[d]; klo[d] = 0; khi[d] = 2; }
    long long deposits = 0;
    int rc = for_each_cell<NO>(lo, hi, [&](const int (&j0)[NO]) {
        // 2. every centre smooth_cell can return has a tile
        const uint32_t t = smooth_tile_key<NO>(j0, n, tl.nt);
        if (t >= (uint32_t)tl.tiles) return fail<NO>(2, grid, "key(j0) >= tiles", t, tl.tiles);
        // 3. every cell deposited is flushed to the cell it was meant for
        int org[NO];
        origin<NO>(t, tl.nt, org);
        const SmoothLdsAxes<NO> la = smooth_lds_axes<NO>(j0, org, n);
        return for_each_cell<NO>(klo, khi, [&](const int (&k)[NO]) {
            bool in_grid = true, in = true;
            int64_t want = 0, stride = 1;
            int l = 0;
            for (int d = 0; d < NO; ++d) {
                const int c = j0[d] + k[d] - 1;
                in_grid = in_grid && c >= 0 && c < n[d];
                want += (int64_t)c * stride;
                stride *= n[d];
                in = in && la.in[d][k[d]];
                l += la.loff[d][k[d]];
                if (!la.in[d][k[d]] && la.loff[d][k[d]] != 0)
                    return fail<NO>(3, grid, "a dropped cell has a non-zero offset term", d, la.loff[d][k[d]]);
            }
            if (!in_grid) return in ? fail<NO>(3, grid, "a cell outside the grid is deposited", t, l) : 0;
            if (!in) return fail<NO>(3, grid, "a cell of the grid is not on its tile + halo", t, want);
            if (l < 0 || l >= NC) return fail<NO>(3, grid, "LDS cell outside [0, NC)", t, l);
            int off = -1;
            if (!smooth_lds_decode<NO>(l, org, n, off))
                return fail<NO>(3, grid, "the flush drops a cell that was deposited", t, l);
            if (off != want) return fail<NO>(3, grid, "the flush sends a deposit to another cell", off, want);
            ++deposits;
            return 0;
        });
    });
    if (rc) return rc;

    // 4. the flush of a tile stays in the plane and writes no cell twice
    for (uint32_t t = 0; t < (uint32_t)tl.tiles; ++t) {
        int org[NO];
        origin<NO>(t, tl.nt, org);
        std::vector<char> seen((size_t)G, 0);
        for (int i = 0; i < NC; ++i) {
            int off = -1;
            if (!smooth_lds_decode<NO>(i, org, n, off)) continue;
            if (off < 0 || off >= G) return fail<NO>(4, grid, "flush offset outside [0, G)", t, off);
            if (seen[off]) return fail<NO>(4, grid, "two LDS cells of a tile flush to one cell", t, off);
            seen[off] = 1;
        }
    }
    printf("grid (");
    for (int d = 0; d < NO; ++d) printf("%s%lld", d ? ", " : "", (long long)grid[d]);
    printf("): ok (%lld tiles, %lld deposits)\n", (long long)tl.tiles, deposits);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && std::strcmp(argv[1], "--shifted-origins") == 0) g_shifted_origins = true;
    else if (argc != 1) { fprintf(stderr, "usage: %s [--shifted-origins]\n", argv[0]); return 2; }
    // one tile, an exact tile, one cell over it, one cell under it, several tiles with a ragged last one
    const int64_t g2[][2] = {{1, 1}, {64, 16}, {65, 17}, {63, 15}, {130, 33}};
    const int64_t g3[][3] = {{1, 1, 1}, {16, 8, 8}, {17, 9, 9}, {15, 7, 7}, {33, 17, 3}};
    for (const auto& g : g2)
        if (int rc = run<2>(g)) return rc;
    for (const auto& g : g3)
        if (int rc = run<3>(g)) return rc;
    return 0;
}
