// Host run of the index arithmetic of DPR_ALGO_ORDERED (csrc/dpr_ordered_index.h: key encode / decode, cell
// ranges, the merge walk, the neighbour test) -- the code every loop bound of k_ord_gather comes from.
// tests/test_ordered_host.py builds this file with -fsanitize=address,undefined and runs it as a child process on
// generated clouds.  Per input file it
//   1. builds the keys of every point,  2. stable-sorts (key, index),  3. fills the start table and walks every
//   output cell with ord_merge_walk,    4. compares the planes bit for bit with a plain serial splat.
// Exit status: 0 every file walked and equal, 1 a walk out of order / a wrong point / a plane that differs, 2 an
// unreadable file.  `--reversed-lists` (first argument; for the test of the checker itself) reverses every cell's
// list after the host sort, so that the walk meets descending point indices: the program must then exit 1.
// File layout (little endian): int32 n_in, n_out, P, has_pw, grid[4]; float32 rot[n_out * n_in] (column-major),
// trans[n_out], background, out_weight, points[P * n_in], pw[P if has_pw].
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>

#include "../diffpointrasterisation.jl_amd/csrc/dpr_ordered_index.h"

using namespace dpr;

struct Case {
    int n_in, n_out, P, has_pw, grid[4];
    std::vector<float> rot, trans, points, pw;
    float bg, ow;
};

static bool g_reversed_lists = false;

static bool read_case(const char* path, Case& c) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    int32_t h[8];
    bool ok = fread(h, 4, 8, f) == 8;
    if (ok) {
        c.n_in = h[0]; c.n_out = h[1]; c.P = h[2]; c.has_pw = h[3];
        for (int d = 0; d < 4; ++d) c.grid[d] = h[4 + d];
        ok = c.n_in >= 1 && c.n_in <= 4 && c.n_out >= 1 && c.n_out <= 4 && c.P >= 0;
    }
    auto rd = [&](std::vector<float>& v, size_t n) {
        v.resize(n);
        if (ok && n) ok = fread(v.data(), 4, n, f) == n;
    };
    if (ok) {
        rd(c.rot, (size_t)c.n_out * c.n_in);
        rd(c.trans, (size_t)c.n_out);
        std::vector<float> two;
        rd(two, 2);
        if (ok) { c.bg = two[0]; c.ow = two[1]; }
        rd(c.points, (size_t)c.P * c.n_in);
        rd(c.pw, c.has_pw ? (size_t)c.P : 0);
    }
    fclose(f);
    return ok;
}

// the reference's cell choice and deltas (csrc/dpr_device.h ref_and_deltas, same operation order)
template <int NO> static bool ref_and_deltas(const Case& c, const float* p, int (&ref0)[NO], float (&dlo)[NO]) {
    bool ok = true;
    for (int d = 0; d < NO; ++d) {
        float proj = c.rot[d] * p[0];
        for (int j = 1; j < c.n_in; ++j) proj = proj + c.rot[d + j * NO] * p[j];
        const float origin = -1.0f - c.trans[d];
        const float scale = (float)c.grid[d] / 2.0f;
        const float coord = (proj - origin) * scale;
        const float cc = coord - 0.5f;
        ok = ok && (cc > -1.0f) && (cc <= (float)c.grid[d]);
        const float r = std::ceil(cc);
        ref0[d] = ok ? (int)r - 1 : 0;
        dlo[d] = coord - (r - 0.5f);
    }
    return ok;
}
template <int NO> static float voxel_weight(const float (&dlo)[NO], int s, float w) {
    float v = (s & 1) ? dlo[0] : (1.0f - dlo[0]);
    for (int d = 1; d < NO; ++d) v = v * (((s >> d) & 1) ? dlo[d] : (1.0f - dlo[d]));
    return v * w;
}

template <int NO> static int run(const Case& c, const char* path) {
    int n[NO];
    uint64_t G = 1;
    for (int d = 0; d < NO; ++d) { n[d] = c.grid[d]; G *= (uint64_t)n[d]; }
    const uint64_t ge = ord_ext_cells<NO>(n);
    if (ge == 0) { fprintf(stderr, "%s: extended grid does not fit\n", path); return 1; }
    const int bits = ord_key_bits(ge);
    const uint32_t mask = bits >= 32 ? 0xffffffffu : ((1u << bits) - 1u);
    const uint32_t P = (uint32_t)c.P;
    auto weight = [&](uint32_t p) { return c.ow * (c.has_pw ? c.pw[p] : 1.0f); };

    // serial splat: (point, neighbour) order from the background
    std::vector<float> want(G, c.bg);
    for (uint32_t p = 0; p < P; ++p) {
        int ref0[NO];
        float dlo[NO];
        if (!ref_and_deltas<NO>(c, &c.points[(size_t)p * c.n_in], ref0, dlo)) continue;
        for (int s = 0; s < (1 << NO); ++s) {
            uint64_t off = 0, stride = 1;
            bool in = true;
            for (int d = 0; d < NO; ++d) {
                const int i = ref0[d] + ((s >> d) & 1);
                in = in && i >= 0 && i < n[d];
                off += (uint64_t)(in ? i : 0) * stride;
                stride *= (uint64_t)n[d];
            }
            if (in) want[off] += voxel_weight<NO>(dlo, s, weight(p));
        }
    }

    // 1. keys (and the round trip of the encoding)
    std::vector<uint32_t> keys(P), idx(P);
    for (uint32_t p = 0; p < P; ++p) {
        int ref0[NO], back[NO];
        float dlo[NO];
        const bool ok = ref_and_deltas<NO>(c, &c.points[(size_t)p * c.n_in], ref0, dlo);
        keys[p] = ok ? ord_key_encode<NO>(ref0, n) : kOrdNoKey;
        if (ok) {
            if (keys[p] >= ge) { fprintf(stderr, "%s: key %u of point %u outside the extended grid\n", path, keys[p], p); return 1; }
            ord_key_decode<NO>(keys[p], n, back);
            for (int d = 0; d < NO; ++d)
                if (back[d] != ref0[d]) { fprintf(stderr, "%s: key round trip of point %u\n", path, p); return 1; }
        }
    }
    // 2. stable sort on the key bits the device sorts on
    std::iota(idx.begin(), idx.end(), 0u);
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return (keys[a] & mask) < (keys[b] & mask); });
    if (g_reversed_lists)
        for (uint32_t i = 0; i < P;) {
            uint32_t j = i;
            while (j < P && (keys[idx[j]] & mask) == (keys[idx[i]] & mask)) ++j;
            std::reverse(idx.begin() + i, idx.begin() + j);
            i = j;
        }
    std::vector<uint32_t> skeys(P);
    for (uint32_t i = 0; i < P; ++i) skeys[i] = keys[idx[i]];
    // 3. the start table (exactly ge + 1 entries: the sanitizer sees any read past it) and the walk of every cell
    std::vector<uint32_t> start(ge + 1);
    for (uint64_t k = 0; k <= ge; ++k) start[k] = ord_lower_bound(skeys.data(), P, (uint32_t)k, bits);
    uint64_t visited = 0;
    for (uint64_t cell = 0; cell < G; ++cell) {
        int cc[NO];
        ord_cell_coords<NO>((uint32_t)cell, n, cc);
        float acc = c.bg;
        uint32_t last = 0;
        bool first = true, ordered = true;
        ord_merge_walk<NO>(cc, n, start.data(), idx.data(), P, [&](uint32_t p, int s) {
            ordered = ordered && (first || p > last) && p < P;
            first = false;
            last = p;
            ++visited;
            int ref0[NO];
            float dlo[NO];
            if (p < P && ref_and_deltas<NO>(c, &c.points[(size_t)p * c.n_in], ref0, dlo)) {
                for (int d = 0; d < NO; ++d) ordered = ordered && ref0[d] + ((s >> d) & 1) == cc[d];  // the neighbour test
                acc += voxel_weight<NO>(dlo, s, weight(p));
            } else {
                ordered = false;
            }
        });
        if (!ordered) { fprintf(stderr, "%s: cell %llu walked out of order / a wrong point\n", path, (unsigned long long)cell); return 1; }
        // 4. bit for bit
        if (std::memcmp(&acc, &want[cell], 4) != 0) {
            fprintf(stderr, "%s: cell %llu: %.9g != %.9g\n", path, (unsigned long long)cell, acc, want[cell]);
            return 1;
        }
    }
    printf("%s: ok (%u points, %llu cells, %llu contributions)\n", path, P, (unsigned long long)G, (unsigned long long)visited);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s case.bin ...\n", argv[0]); return 2; }
    int first = 1;
    if (std::strcmp(argv[1], "--reversed-lists") == 0) { g_reversed_lists = true; first = 2; }
    for (int a = first; a < argc; ++a) {
        Case c;
        if (!read_case(argv[a], c)) { fprintf(stderr, "%s: unreadable\n", argv[a]); return 2; }
        int rc = 2;
        switch (c.n_out) {
            case 1: rc = run<1>(c, argv[a]); break;
            case 2: rc = run<2>(c, argv[a]); break;
            case 3: rc = run<3>(c, argv[a]); break;
            case 4: rc = run<4>(c, argv[a]); break;
        }
        if (rc) return rc;
    }
    return 0;
}
