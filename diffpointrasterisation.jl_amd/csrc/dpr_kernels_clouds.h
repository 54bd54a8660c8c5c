// Per-pose clouds (dpr_raster_clouds_ex_* / dpr_raster_pullback_clouds_ex_*, include/dpr.h "PER-POSE CLOUDS"):
// pose b reads its own cloud, points + b * P * NI and point_weight + b * P, and its point gradients are its own
// (ds_dpoints + b * P * NI, ds_dpoint_weight + b * P) -- disjoint across poses, so no point accumulator is carried
// from one pose to the next and every point gradient is written once with a plain store.
//   DPR_ALGO_ATOMIC   one thread per (point, pose): global float atomics forward, gathers + wave -> block -> one
//                     atomic per scalar per block backward (k_fwd_atomic / k_bwd_gather with the cloud indexed
//                     by pose)
//   DPR_ALGO_CHUNKED  pose-owned LDS tiles, (2,2) / (3,3) / (3,2): a workgroup owns (pose b, a tile of b's grid,
//                     a slice of consecutive points of cloud b).  Forward: LDS accumulation (fp32: 64-bit fixed
//                     point, per-pose scale), plain-store flush with the background when the (pose, tile) has one
//                     slice, row-shaped global atomics onto the filled background when it has several.  Pullback:
//                     the tile of ds_dout (+ one halo cell on the high side) staged in LDS; the tile holding a
//                     point's reference cell owns it, gathers from LDS and stores its gradients; per-pose sums go
//                     wave -> block -> one f64 partial per workgroup, summed in a fixed order by k_clouds_reduce.
#pragma once
#include <type_traits>

#include "dpr_device.h"
#include "dpr_kernels_atomic.h"

namespace dpr {

// ---------------------------------------------------------------- DPR_ALGO_ATOMIC
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kBlock) void k_clouds_fwd_atomic(GridDesc<NO> gd, int64_t P, int64_t B,
                                                              T* __restrict__ out, const T* __restrict__ points,
                                                              const T* __restrict__ rot,
                                                              const T* __restrict__ trans,
                                                              const T* __restrict__ ow,
                                                              const T* __restrict__ pw) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= P) return;
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        T pt[NI];
        load_point<T, NI>(points + b * P * NI, p, pt);
        const T pwi = pw ? pw[b * P + p] : T(1);
        const Pose<T, NI, NO> ps = load_pose<T, NI, NO>(rot, trans, ow, b);
        int ref0[NO];
        T dlo[NO];
        if (!ref_and_deltas<T, NI, NO>(pt, ps, gd, ref0, dlo)) continue;
        const T w = ps.ow * pwi;  // as k_fwd_atomic
        T* o = out + b * gd.G;
#pragma unroll
        for (int s = 0; s < (1 << NO); ++s) {
            const int off = nbr_offset<NO>(ref0, s, gd);
            if (off >= 0) atomic_add<T>(o + off, voxel_weight<T, NO>(dlo, s, w));
        }
    }
}

// The per-pose sums of one (point, pose): vals = dR (NO x NI, column-major) | dt | d out_weight, and the point
// gradients, exactly as k_bwd_gather forms them (the point accumulators start at 0 and add once, so a B = 1 call
// stores the same bits as k_bwd_gather's single-slice launch).
template <typename T, int NI, int NO>
__device__ __forceinline__ void clouds_point_terms(const T (&pt)[NI], const Pose<T, NI, NO>& ps,
                                                   const T (&scaled)[NO], T dow_part, T dpw_part,
                                                   T (&vals)[NO * NI + NO + 1], T (&gpt)[NI], T& gpw) {
#pragma unroll
    for (int n = 0; n < NO; ++n) {
#pragma unroll
        for (int j = 0; j < NI; ++j) vals[n + j * NO] = scaled[n] * pt[j];
        vals[NO * NI + n] = scaled[n];
    }
    vals[NO * NI + NO] = dow_part;
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        T v = ps.R[0 + j * NO] * scaled[0];
#pragma unroll
        for (int n = 1; n < NO; ++n) v = v + ps.R[n + j * NO] * scaled[n];
        gpt[j] = T(0);
        gpt[j] += v;
    }
    gpw = T(0);
    gpw += dpw_part;
}

// Pullback, one thread per (point, pose).  Pre-zeroed: ds_drotation, ds_dtranslation, ds_dout_weight.
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kBlock) void k_clouds_bwd_atomic(
    GridDesc<NO> gd, int64_t P, int64_t B, const T* __restrict__ g, const T* __restrict__ points,
    const T* __restrict__ rot, const T* __restrict__ trans, const T* __restrict__ ow, const T* __restrict__ pw,
    T* __restrict__ ds_dpoints, T* __restrict__ ds_drotation, T* __restrict__ ds_dtranslation,
    T* __restrict__ ds_dout_weight, T* __restrict__ ds_dpoint_weight) {
    constexpr int NV = NO * NI + NO + 1;
    constexpr int NW = kBlock / kWave;
    __shared__ T red[NW][NV];
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = p < P;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        const Pose<T, NI, NO> ps = load_pose<T, NI, NO>(rot, trans, ow, b);
        const int64_t q = b * P + p;  // (point, pose) index of the point gradients
        T pt[NI];
#pragma unroll
        for (int j = 0; j < NI; ++j) pt[j] = T(0);
        if (live) load_point<T, NI>(points + b * P * NI, p, pt);
        const T pwi = (live && pw) ? pw[q] : T(1);
        T vals[NV], gpt[NI], gpw = T(0);
#pragma unroll
        for (int k = 0; k < NV; ++k) vals[k] = T(0);
#pragma unroll
        for (int j = 0; j < NI; ++j) gpt[j] = T(0);
        int ref0[NO];
        T dlo[NO];
        if (live && ref_and_deltas<T, NI, NO>(pt, ps, gd, ref0, dlo)) {
            const int64_t gb = b * gd.G;
            T scaled[NO], dow_part, dpw_part;
            point_backward<T, NI, NO>(ref0, dlo, gd, ps.ow, pwi, [&](int off) { return g[gb + off]; }, scaled,
                                      dow_part, dpw_part);
            clouds_point_terms<T, NI, NO>(pt, ps, scaled, dow_part, dpw_part, vals, gpt, gpw);
        }
        if (live) {
#pragma unroll
            for (int j = 0; j < NI; ++j) ds_dpoints[q * NI + j] = gpt[j];
            if (ds_dpoint_weight) ds_dpoint_weight[q] = gpw;
        }
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const T s = wave_sum<T>(vals[k]);
            if (lane == 0) red[wave][k] = s;
        }
        __syncthreads();
        if (threadIdx.x < NV) {
            T s = red[0][threadIdx.x];
#pragma unroll
            for (int w = 1; w < NW; ++w) s += red[w][threadIdx.x];
            const int k = threadIdx.x;
            if (s != T(0)) {
                if (k < NO * NI)
                    atomic_add<T>(ds_drotation + b * (NO * NI) + k, s);
                else if (k < NO * NI + NO)
                    atomic_add<T>(ds_dtranslation + b * NO + (k - NO * NI), s);
                else
                    atomic_add<T>(ds_dout_weight + b, s);
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- DPR_ALGO_CHUNKED: pose-owned LDS tiles
constexpr int kCLThreads = 512;
// tile extents: 2-D 128 x 78 = 9984 cells of 8 bytes (the chunk-owner tile of dpr_chunkown.hip, two workgroups
// per CU); 3-D 32 x 16 x 16 = 8192 (its pullback tile with the halo, 33 x 17 x 17 cells of f64, stays below
// 80 KiB)
template <int NO> struct CloudTileShape;
template <> struct CloudTileShape<2> {
    static constexpr int e[2] = {128, 78};
};
template <> struct CloudTileShape<3> {
    static constexpr int e[3] = {32, 16, 16};
};
template <int NO> __host__ __device__ constexpr int cl_tile_cells(int halo) {
    int n = 1;
    for (int d = 0; d < NO; ++d) n *= CloudTileShape<NO>::e[d] + halo;
    return n;
}

template <int NO> struct CloudTiles {
    int nt[NO];  // tiles per axis
    int tiles;   // product
};

// first cell of tile `tile` per axis
template <int NO>
__device__ __forceinline__ void cl_tile_origin(const CloudTiles<NO>& ct, int tile, int (&lo)[NO]) {
#pragma unroll
    for (int d = 0; d < NO; ++d) {
        lo[d] = (tile % ct.nt[d]) * CloudTileShape<NO>::e[d];
        tile /= ct.nt[d];
    }
}

// Per-pose (max, min non-zero) |point_weight| key (dpr_device.h wrange_*) for the fp32 fixed-point scale: one
// block per pose.
template <typename T>
__global__ __launch_bounds__(256) void k_clouds_wrange(const T* __restrict__ pw, int64_t P, int64_t b0,
                                                       uint32_t* __restrict__ keys) {
    __shared__ uint32_t part[256 / kWave];
    const int64_t b = b0 + blockIdx.x;
    const T* w = pw + b * P;
    uint32_t key = 0;
    for (int64_t i = threadIdx.x; i < P; i += 256) key = wrange_merge(key, wrange_key((float)w[i]));
    key = wrange_wave(key);
    if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x / kWave] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t k = part[0];
#pragma unroll
        for (int i = 1; i < 256 / kWave; ++i) k = wrange_merge(k, part[i]);
        keys[b] = k;
    }
}

// Forward.  grid.x = tile * slices + slice, grid.y = pose - b0.  `atomic_flush` 0: one slice per (pose, tile),
// the flush stores background + sum; 1: `out` holds the background and the sum is added with float atomics.
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kCLThreads) void k_clouds_fwd_tile(
    GridDesc<NO> gd, CloudTiles<NO> ct, int slices, int64_t slice_len, int64_t P, int64_t b0,
    T* __restrict__ out, const T* __restrict__ points, const T* __restrict__ rot, const T* __restrict__ trans,
    const T* __restrict__ bg, const T* __restrict__ ow, const T* __restrict__ pw,
    const uint32_t* __restrict__ wkeys, int atomic_flush) {
    constexpr int CAP = cl_tile_cells<NO>(0);
    __shared__ double cell[CAP];
    const int64_t b = b0 + blockIdx.y;
    const int tile = blockIdx.x / slices, slice = blockIdx.x % slices;
    int lo[NO], ext[NO];
    cl_tile_origin<NO>(ct, tile, lo);
#pragma unroll
    for (int d = 0; d < NO; ++d) {
        const int rest = gd.n[d] - lo[d];
        ext[d] = rest < CloudTileShape<NO>::e[d] ? rest : CloudTileShape<NO>::e[d];
    }
    const int64_t p_lo = (int64_t)slice * slice_len;
    const int64_t p_hi = (p_lo + slice_len < P) ? p_lo + slice_len : P;
    for (int c = threadIdx.x; c < CAP; c += kCLThreads) cell[c] = 0.0;
    const Pose<T, NI, NO> ps = load_pose<T, NI, NO>(rot, trans, ow, b);
    // fp32: exact 64-bit fixed point, scale from |out_weight[b]| * max |point_weight[b, :]| and the slice's
    // point count (a point adds to a cell at most once), f64 atomics where the 2^10 range guard trips
    FixScale fs{0.0, 0.0};
    if constexpr (sizeof(T) == 4) {
        float maxw = fabsf((float)ps.ow);
        if (wkeys) {
            const uint32_t k = wkeys[b];
            maxw = maxw * wrange_guarded_max(k >> 16, k & 0xffffu);
        }
        fs = fix_scale(maxw, (uint32_t)(p_hi - p_lo), 1);
    }
    __syncthreads();
    auto splat = [&](auto fix_tag) {
        constexpr bool FIX = decltype(fix_tag)::value;
        const T* cloud = points + b * P * NI;
        for (int64_t p = p_lo + threadIdx.x; p < p_hi; p += kCLThreads) {
            T pt[NI];
            load_point<T, NI>(cloud, p, pt);
            const T pwi = pw ? pw[b * P + p] : T(1);
            int ref0[NO];
            T dlo[NO];
            if (!ref_and_deltas<T, NI, NO>(pt, ps, gd, ref0, dlo)) continue;
            bool touches = true;
#pragma unroll
            for (int d = 0; d < NO; ++d) touches = touches && ref0[d] + 1 >= lo[d] && ref0[d] < lo[d] + ext[d];
            if (!touches) continue;
            const T w = ps.ow * pwi;
#pragma unroll
            for (int s = 0; s < (1 << NO); ++s) {
                bool in = true;
                int li = 0, stride = 1;
#pragma unroll
                for (int d = 0; d < NO; ++d) {
                    const int l = ref0[d] + ((s >> d) & 1) - lo[d];
                    in = in && l >= 0 && l < ext[d];
                    li += l * stride;
                    stride *= CloudTileShape<NO>::e[d];
                }
                if (in) cell_add<FIX, T>(&cell[li], voxel_weight<T, NO>(dlo, s, w), fs);
            }
        }
    };
    if constexpr (sizeof(T) == 4) {
        if (fs.mul != 0.0) splat(std::true_type{});
        else splat(std::false_type{});
    } else {
        splat(std::false_type{});
    }
    __syncthreads();
    const T bgv = bg ? bg[b] : T(0);
    T* o = out + b * gd.G;
    for (int c = threadIdx.x; c < CAP; c += kCLThreads) {
        int rest = c, off = 0, stride = 1;
        bool in = true;
#pragma unroll
        for (int d = 0; d < NO; ++d) {
            const int l = rest % CloudTileShape<NO>::e[d];
            rest /= CloudTileShape<NO>::e[d];
            in = in && l < ext[d];
            off += (lo[d] + l) * stride;
            stride *= gd.n[d];
        }
        if (!in) continue;
        const T v = (T)fix_value(cell[c], fs);
        if (!atomic_flush) o[off] = bgv + v;
        else if (v != T(0)) atomic_add<T>(o + off, v);
    }
}

// Pullback.  grid.x = tile * slices + slice, grid.y = pose - b0.  Writes ds_dpoints / ds_dpoint_weight of the
// (point, pose) pairs this tile owns and one f64 partial per per-pose scalar:
// partials[(k * B + b) * (tiles * slices) + blockIdx.x].
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kCLThreads) void k_clouds_bwd_tile(
    GridDesc<NO> gd, CloudTiles<NO> ct, int slices, int64_t slice_len, int64_t P, int64_t B, int64_t b0,
    const T* __restrict__ g, const T* __restrict__ points, const T* __restrict__ rot, const T* __restrict__ trans,
    const T* __restrict__ ow, const T* __restrict__ pw, T* __restrict__ ds_dpoints,
    T* __restrict__ ds_dpoint_weight, double* __restrict__ partials) {
    constexpr int NV = NO * NI + NO + 1;
    constexpr int NW = kCLThreads / kWave;
    constexpr int HCAP = cl_tile_cells<NO>(1);
    __shared__ T gt[HCAP];
    __shared__ double red[NW][NV];
    const int64_t b = b0 + blockIdx.y;
    const int tile = blockIdx.x / slices, slice = blockIdx.x % slices;
    int lo[NO];
    cl_tile_origin<NO>(ct, tile, lo);
    const int64_t gb = b * gd.G;
    // stage the tile and its high-side halo (cells outside the grid: 0, never used -- their neighbours are dropped)
    for (int c = threadIdx.x; c < HCAP; c += kCLThreads) {
        int rest = c, off = 0, stride = 1;
        bool in = true;
#pragma unroll
        for (int d = 0; d < NO; ++d) {
            const int x = lo[d] + rest % (CloudTileShape<NO>::e[d] + 1);
            rest /= CloudTileShape<NO>::e[d] + 1;
            in = in && x < gd.n[d];
            off += x * stride;
            stride *= gd.n[d];
        }
        gt[c] = in ? g[gb + off] : T(0);
    }
    const Pose<T, NI, NO> ps = load_pose<T, NI, NO>(rot, trans, ow, b);
    __syncthreads();
    const int64_t p_lo = (int64_t)slice * slice_len;
    const int64_t p_hi = (p_lo + slice_len < P) ? p_lo + slice_len : P;
    const T* cloud = points + b * P * NI;
    T acc[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = T(0);
    for (int64_t p = p_lo + threadIdx.x; p < p_hi; p += kCLThreads) {
        T pt[NI];
        load_point<T, NI>(cloud, p, pt);
        int ref0[NO];
        T dlo[NO];
        const bool ok = ref_and_deltas<T, NI, NO>(pt, ps, gd, ref0, dlo);
        // the owner: the tile of the reference cell (-1 clamped to 0); a dropped point belongs to tile 0
        int owner = 0;
        if (ok) {
            int stride = 1;
#pragma unroll
            for (int d = 0; d < NO; ++d) {
                owner += ((ref0[d] < 0 ? 0 : ref0[d]) / CloudTileShape<NO>::e[d]) * stride;
                stride *= ct.nt[d];
            }
        }
        if (owner != tile) continue;
        const int64_t q = b * P + p;
        T gpt[NI], gpw = T(0);
#pragma unroll
        for (int j = 0; j < NI; ++j) gpt[j] = T(0);
        if (ok) {
            const T pwi = pw ? pw[q] : T(1);
            T vals[NV], scaled[NO], dow_part, dpw_part;
            // point_backward fetches neighbour s = 0, 1, .., 2^N - 1 in that order, once each: `s` follows the
            // calls, and the neighbour's cell is read from the staged tile (each axis clamped to the tile: a
            // dropped neighbour's value is never used)
            int s = 0;
            auto fetch = [&](int) {
                int li = 0, stride = 1;
#pragma unroll
                for (int d = 0; d < NO; ++d) {
                    const int l = ref0[d] + ((s >> d) & 1) - lo[d];
                    li += (l < 0 ? 0 : l) * stride;
                    stride *= CloudTileShape<NO>::e[d] + 1;
                }
                ++s;
                return gt[li];
            };
            point_backward<T, NI, NO>(ref0, dlo, gd, ps.ow, pwi, fetch, scaled, dow_part, dpw_part);
            clouds_point_terms<T, NI, NO>(pt, ps, scaled, dow_part, dpw_part, vals, gpt, gpw);
#pragma unroll
            for (int k = 0; k < NV; ++k) acc[k] += vals[k];
        }
#pragma unroll
        for (int j = 0; j < NI; ++j) ds_dpoints[q * NI + j] = gpt[j];
        if (ds_dpoint_weight) ds_dpoint_weight[q] = gpw;
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const double s = wave_sum<double>((double)acc[k]);
        if (lane == 0) red[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        double s = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < NW; ++w) s += red[w][threadIdx.x];
        partials[((int64_t)threadIdx.x * B + b) * gridDim.x + blockIdx.x] = s;
    }
}

// partials[NV][B][nparts] -> ds_drotation | ds_dtranslation | ds_dout_weight (overwritten), a fixed order per
// (scalar, pose): block per (scalar, pose - b0)
template <typename T, int NI, int NO>
__global__ __launch_bounds__(256) void k_clouds_reduce(const double* __restrict__ partials, int64_t B, int64_t b0,
                                                       int64_t nparts, T* __restrict__ d_rot,
                                                       T* __restrict__ d_trans, T* __restrict__ d_ow) {
    __shared__ double wsum[256 / kWave];
    const int k = blockIdx.x;
    const int64_t b = b0 + blockIdx.y;
    const double* src = partials + ((int64_t)k * B + b) * nparts;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < nparts; i += 256) s += src[i];
    s = wave_sum<double>(s);
    if ((threadIdx.x & (kWave - 1)) == 0) wsum[threadIdx.x / kWave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double tot = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        if (k < NO * NI)
            d_rot[b * (NO * NI) + k] = (T)tot;
        else if (k < NO * NI + NO)
            d_trans[b * NO + (k - NO * NI)] = (T)tot;
        else
            d_ow[b] = (T)tot;
    }
}

}  // namespace dpr
