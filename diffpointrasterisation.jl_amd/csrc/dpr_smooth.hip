// The smooth splat: quadratic B-spline (TSC) weights on 3^N cells per point (include/dpr.h, "SMOOTH SPLAT").
//
//   coord_d = ((R p + t)_d + 1) * n_d / 2,  j0_d = floor(coord_d),  u_d = coord_d - (j0_d + 1/2)  in [-1/2, 1/2)
//   w_d(-1) = (1/2 - u)^2 / 2    w_d(0) = 3/4 - u^2    w_d(+1) = (1/2 + u)^2 / 2         (sum: 1)
//   out[j0 + s] += out_weight * point_weight * prod_d w_d(s_d),  s in {-1, 0, +1}^N, cells outside the grid dropped
//
//   DPR_ALGO_ATOMIC forward   k_smooth_fwd_atomic: one thread per point, pose loop inside, 3^N global atomics
//   DPR_ALGO_ATOMIC pullback  k_smooth_bwd: k_bwd_gather's shape (point gradients in registers across the poses of a
//                             slice, per-pose sums wave -> block -> one atomic per block); the 3^N gathers are issued
//                             one 3^(N-1) slab at a time and contracted axis by axis (the weights are separable)
//   DPR_ALGO_TILED forward    per pose: k_smooth_keys (tile of the clamped centre cell, all ones for a rejected
//                             point) -> stable radix sort of (key, index) -> k_smooth_ranges (start table over the
//                             tiles) -> k_smooth_tile: one workgroup per tile adds its run of points into an LDS tile
//                             + halo of f64 cells (ds_add_f64) and adds every non-zero cell inside the grid onto
//                             `out` with one global atomic in T, rows of axis 0 on consecutive lanes.  No global
//                             atomic per point; a cell receives at most 3^N tile partials.
//   smooth sampling           k_sample_smooth_fwd / k_sample_smooth_bwd (include/dpr.h, "SMOOTH SAMPLING"): the same
//                             cell, weights and gathers read the other way round -- an image at the points
//   forward-mode derivative   k_smooth_jvp_atomic / k_smooth_tile_jvp (include/dpr.h, "SMOOTH SPLAT, FORWARD MODE"):
//                             the two forward shapes with the deposit of a tangent in the place of the weight
//                             product; the tiled path bins a pose once for all K tangents
//   per-pose clouds           k_smooth_clouds_fwd_atomic / k_smooth_clouds_bwd / k_smooth_clouds_keys /
//                             k_smooth_clouds_tile (include/dpr.h, "SMOOTH SPLAT, PER-POSE CLOUDS"): pose b reads
//                             cloud b; a thread per (point, pose); the tiled forward bins a GROUP of poses with one
//                             key pass, one sort, one start table and one launch of (poses x tiles) workgroups
//   host side of the binning  smooth_plan (the workspace), smooth_binning, smooth_sort_group, smooth_bin_pose: one copy
//                             for every tiled launcher here, in dpr_smooth_channels.hip, in dpr_smooth_bodies.hip and
//                             in dpr_sample_smooth_bodies.hip
#include <hip/hip_runtime.h>

#include "../../include/dpr.h"
#include "dpr_ordered.h"
#include "dpr_ordered_index.h"
#include "dpr_smooth.h"
#include "dpr_smooth_device.h"

namespace dpr {

// ---------------------------------------------------------------- DPR_ALGO_ATOMIC forward
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kSmBlock) void k_smooth_fwd_atomic(GridDesc<NO> gd, int64_t P, int64_t B,
                                                                T* __restrict__ out, const T* __restrict__ points,
                                                                const T* __restrict__ rot,
                                                                const T* __restrict__ trans,
                                                                const T* __restrict__ ow, const T* __restrict__ pw) {
    static_assert(NO == 2 || NO == 3, "the smooth splat is written for 2-D and 3-D grids");
    const int64_t p = (int64_t)blockIdx.x * kSmBlock + threadIdx.x;
    if (p >= P) return;
    T pt[NI];
    load_point<T, NI>(points, p, pt);
    const T pwi = pw ? pw[p] : T(1);
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        const Pose<T, NI, NO> ps = load_pose<T, NI, NO>(rot, trans, ow, b);
        int j0[NO];
        T u[NO];
        if (!smooth_cell<T, NI, NO>(pt, ps, gd, j0, u)) continue;
        const T w = ps.ow * pwi;
        const SmoothAxes<T, NO> ax = smooth_axes<T, NO>(j0, u, gd);
        T* o = out + b * gd.G;
#pragma unroll
        for (int k2 = 0; k2 < (NO == 3 ? 3 : 1); ++k2) {
            const bool in2 = NO == 3 ? ax.in[NO - 1][k2] : true;
            const int off2 = NO == 3 ? ax.off[NO - 1][k2] : 0;
            const T w2 = NO == 3 ? ax.w[NO - 1][k2] * w : w;
#pragma unroll
            for (int k1 = 0; k1 < 3; ++k1) {
                const T w12 = ax.w[1][k1] * w2;
#pragma unroll
                for (int k0 = 0; k0 < 3; ++k0)
                    if (in2 && ax.in[1][k1] && ax.in[0][k0])
                        atomic_add<T>(o + (off2 + ax.off[1][k1] + ax.off[0][k0]), ax.w[0][k0] * w12);
            }
        }
    }
}

// ---------------------------------------------------------------- DPR_ALGO_ATOMIC pullback
// (the point term, smooth_point_backward: dpr_smooth_device.h)
// Pre-zeroed: ds_drotation, ds_dtranslation, ds_dout_weight; with accumulate_points also ds_dpoints and
// ds_dpoint_weight (the poses are cut into slices on grid.y, every slice adds its share with atomics).
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kSmBlock) void k_smooth_bwd(
    GridDesc<NO> gd, int64_t P, int64_t B, const T* __restrict__ g, const T* __restrict__ points,
    const T* __restrict__ rot, const T* __restrict__ trans, const T* __restrict__ ow, const T* __restrict__ pw,
    T* __restrict__ ds_dpoints, T* __restrict__ ds_drotation, T* __restrict__ ds_dtranslation,
    T* __restrict__ ds_dout_weight, T* __restrict__ ds_dpoint_weight, int poses_per_slice, int accumulate_points) {
    static_assert(NO == 2 || NO == 3, "the smooth splat is written for 2-D and 3-D grids");
    constexpr int NV = NO * NI + NO + 1;  // dR | dt | d out_weight
    constexpr int NW = kSmBlock / kWave;
    __shared__ T red[NW][NV];

    const int64_t p = (int64_t)blockIdx.x * kSmBlock + threadIdx.x;
    const bool live = p < P;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    T pt[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) pt[j] = T(0);
    if (live) load_point<T, NI>(points, p, pt);
    const T pwi = (live && pw) ? pw[p] : T(1);

    T acc_pt[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) acc_pt[j] = T(0);
    T acc_pw = T(0);

    const int64_t b_lo = (int64_t)blockIdx.y * poses_per_slice;
    const int64_t b_hi = (b_lo + poses_per_slice < B) ? b_lo + poses_per_slice : B;
    for (int64_t b = b_lo; b < b_hi; ++b) {
        const Pose<T, NI, NO> ps = load_pose<T, NI, NO>(rot, trans, ow, b);
        T vals[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) vals[k] = T(0);
        int j0[NO];
        T u[NO];
        if (live && smooth_cell<T, NI, NO>(pt, ps, gd, j0, u)) {
            const T* gb = g + b * gd.G;
            T dcoord[NO], W;
            smooth_point_backward<T, NO>(j0, u, gd, [&](int off) { return gb[off]; }, dcoord, W);
            const T opw = ps.ow * pwi;
            T scaled[NO];
#pragma unroll
            for (int n = 0; n < NO; ++n) scaled[n] = (dcoord[n] * opw) * (T(gd.n[n]) / T(2));
#pragma unroll
            for (int n = 0; n < NO; ++n) {
#pragma unroll
                for (int j = 0; j < NI; ++j) vals[n + j * NO] = scaled[n] * pt[j];
                vals[NO * NI + n] = scaled[n];
            }
            vals[NO * NI + NO] = W * pwi;
#pragma unroll
            for (int j = 0; j < NI; ++j) {  // rotation' * scaled
                T v = ps.R[0 + j * NO] * scaled[0];
#pragma unroll
                for (int n = 1; n < NO; ++n) v = v + ps.R[n + j * NO] * scaled[n];
                acc_pt[j] += v;
            }
            acc_pw += W * ps.ow;
        }
        // per-pose sums: wave -> block -> one atomic per scalar per block
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
    if (live) {
        if (accumulate_points) {
#pragma unroll
            for (int j = 0; j < NI; ++j) atomic_add<T>(ds_dpoints + p * NI + j, acc_pt[j]);
            if (ds_dpoint_weight) atomic_add<T>(ds_dpoint_weight + p, acc_pw);
        } else {
#pragma unroll
            for (int j = 0; j < NI; ++j) ds_dpoints[p * NI + j] = acc_pt[j];
            if (ds_dpoint_weight) ds_dpoint_weight[p] = acc_pw;
        }
    }
}

// ---------------------------------------------------------------- smooth sampling (include/dpr.h, "SMOOTH SAMPLING")
//   values[p, b] = W of smooth_point_backward for g = image_b: the transpose of the splat in the point weights.
//   values, ds_dvalues   P x B, point index fastest: pose b is the contiguous column at b * P
//   image, ds_dimage     (n_1, .., n_N, B) column-major, as `out`
// Both kernels hold a point in registers and loop over a slice of the poses (k_smooth_bwd's shape).

// Forward: one thread per point, the gathers issued plane by plane (smooth_point_backward), the value stored with a
// plain coalesced store into column b.  A rejected point gives 0.
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kSmBlock) void k_sample_smooth_fwd(GridDesc<NO> gd, int64_t P, int64_t B,
                                                                T* __restrict__ values, const T* __restrict__ image,
                                                                const T* __restrict__ points,
                                                                const T* __restrict__ rot,
                                                                const T* __restrict__ trans, int poses_per_slice) {
    static_assert(NO == 2 || NO == 3, "the smooth splat is written for 2-D and 3-D grids");
    const int64_t p = (int64_t)blockIdx.x * kSmBlock + threadIdx.x;
    if (p >= P) return;
    T pt[NI];
    load_point<T, NI>(points, p, pt);
    const int64_t b_lo = (int64_t)blockIdx.y * poses_per_slice;
    const int64_t b_hi = (b_lo + poses_per_slice < B) ? b_lo + poses_per_slice : B;
    for (int64_t b = b_lo; b < b_hi; ++b) {
        const Pose<T, NI, NO> ps = load_pose<T, NI, NO>(rot, trans, nullptr, b);
        int j0[NO];
        T u[NO];
        T v = T(0);
        if (smooth_cell<T, NI, NO>(pt, ps, gd, j0, u)) {
            const T* img = image + b * gd.G;
            T dcoord[NO];  // (only W is kept; the compiler drops the derivative sums)
            smooth_point_backward<T, NO>(j0, u, gd, [&](int off) { return img[off]; }, dcoord, v);
        }
        values[b * P + p] = v;
    }
}

// Pullback over the pose range of the slice for dv = ds_dvalues[p, b]:
//   ds_dpoints, ds_drotation, ds_dtranslation: k_smooth_bwd's terms with ds_dout = image_b, out_weight = 1 and
//                                              point_weight = dv
//   ds_dimage[.., b] += dv * prod_d w_d(s_d)   (k_smooth_fwd_atomic's contribution for point weight dv), when non-NULL
// Any output may be NULL (uniform branches; the image is read only for the three geometric gradients).  Pre-zeroed:
// ds_drotation, ds_dtranslation, ds_dimage; ds_dpoints is stored (accumulate_points == 0) or added atomically onto
// a zeroed buffer.
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kSmBlock) void k_sample_smooth_bwd(
    GridDesc<NO> gd, int64_t P, int64_t B, const T* __restrict__ ds_dvalues, const T* __restrict__ image,
    const T* __restrict__ points, const T* __restrict__ rot, const T* __restrict__ trans,
    T* __restrict__ ds_dimage, T* __restrict__ ds_dpoints, T* __restrict__ ds_drotation,
    T* __restrict__ ds_dtranslation, int poses_per_slice, int accumulate_points) {
    static_assert(NO == 2 || NO == 3, "the smooth splat is written for 2-D and 3-D grids");
    constexpr int NV = NO * NI + NO;  // dR | dt
    constexpr int NW = kSmBlock / kWave;
    __shared__ T red[NW][NV];

    const int64_t p = (int64_t)blockIdx.x * kSmBlock + threadIdx.x;
    const bool live = p < P;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    const bool geom = ds_dpoints || ds_drotation || ds_dtranslation;
    const bool pose_sums = ds_drotation || ds_dtranslation;
    T pt[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) pt[j] = T(0);
    if (live) load_point<T, NI>(points, p, pt);

    T acc_pt[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) acc_pt[j] = T(0);

    const int64_t b_lo = (int64_t)blockIdx.y * poses_per_slice;
    const int64_t b_hi = (b_lo + poses_per_slice < B) ? b_lo + poses_per_slice : B;
    for (int64_t b = b_lo; b < b_hi; ++b) {
        const Pose<T, NI, NO> ps = load_pose<T, NI, NO>(rot, trans, nullptr, b);
        T vals[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) vals[k] = T(0);
        int j0[NO];
        T u[NO];
        if (live && smooth_cell<T, NI, NO>(pt, ps, gd, j0, u)) {
            const T dv = ds_dvalues[b * P + p];
            if (ds_dimage) {
                const SmoothAxes<T, NO> ax = smooth_axes<T, NO>(j0, u, gd);
                T* o = ds_dimage + b * gd.G;
#pragma unroll
                for (int k2 = 0; k2 < (NO == 3 ? 3 : 1); ++k2) {
                    const bool in2 = NO == 3 ? ax.in[NO - 1][k2] : true;
                    const int off2 = NO == 3 ? ax.off[NO - 1][k2] : 0;
                    const T w2 = NO == 3 ? ax.w[NO - 1][k2] * dv : dv;
#pragma unroll
                    for (int k1 = 0; k1 < 3; ++k1) {
                        const T w12 = ax.w[1][k1] * w2;
#pragma unroll
                        for (int k0 = 0; k0 < 3; ++k0)
                            if (in2 && ax.in[1][k1] && ax.in[0][k0])
                                atomic_add<T>(o + (off2 + ax.off[1][k1] + ax.off[0][k0]), ax.w[0][k0] * w12);
                    }
                }
            }
            if (geom) {
                const T* img = image + b * gd.G;
                T dcoord[NO], W;
                smooth_point_backward<T, NO>(j0, u, gd, [&](int off) { return img[off]; }, dcoord, W);
                T scaled[NO];
#pragma unroll
                for (int n = 0; n < NO; ++n) scaled[n] = (dcoord[n] * dv) * (T(gd.n[n]) / T(2));
#pragma unroll
                for (int n = 0; n < NO; ++n) {
#pragma unroll
                    for (int j = 0; j < NI; ++j) vals[n + j * NO] = scaled[n] * pt[j];
                    vals[NO * NI + n] = scaled[n];
                }
#pragma unroll
                for (int j = 0; j < NI; ++j) {  // rotation' * scaled
                    T v = ps.R[0 + j * NO] * scaled[0];
#pragma unroll
                    for (int n = 1; n < NO; ++n) v = v + ps.R[n + j * NO] * scaled[n];
                    acc_pt[j] += v;
                }
            }
        }
        if (!pose_sums) continue;
        // per-pose sums: wave -> block -> one atomic per scalar per block
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
                if (k < NO * NI) {
                    if (ds_drotation) atomic_add<T>(ds_drotation + b * (NO * NI) + k, s);
                } else if (ds_dtranslation) {
                    atomic_add<T>(ds_dtranslation + b * NO + (k - NO * NI), s);
                }
            }
        }
        __syncthreads();
    }
    if (live && ds_dpoints) {
        if (accumulate_points) {
#pragma unroll
            for (int j = 0; j < NI; ++j) atomic_add<T>(ds_dpoints + p * NI + j, acc_pt[j]);
        } else {
#pragma unroll
            for (int j = 0; j < NI; ++j) ds_dpoints[p * NI + j] = acc_pt[j];
        }
    }
}

// ---------------------------------------------------------------- DPR_ALGO_TILED forward
// key = id of the tile (column-major over the tiles, axis 0 fastest) that holds cell j0 clamped into the grid
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kSmBlock) void k_smooth_keys(GridDesc<NO> gd, SmoothTiles<NO> tl, int64_t P, int64_t b,
                                                          const T* __restrict__ points, const T* __restrict__ rot,
                                                          const T* __restrict__ trans, uint32_t* __restrict__ keys,
                                                          uint32_t* __restrict__ idx) {
    const int64_t p = (int64_t)blockIdx.x * kSmBlock + threadIdx.x;
    if (p >= P) return;
    T pt[NI];
    load_point<T, NI>(points, p, pt);
    const Pose<T, NI, NO> ps = load_pose<T, NI, NO>(rot, trans, nullptr, b);
    int j0[NO];
    T u[NO];
    uint32_t key = kSmoothNoKey;
    if (smooth_cell<T, NI, NO>(pt, ps, gd, j0, u)) {
        uint32_t stride = 1;
        key = 0;
#pragma unroll
        for (int d = 0; d < NO; ++d) {
            const int c = j0[d] < 0 ? 0 : (j0[d] >= gd.n[d] ? gd.n[d] - 1 : j0[d]);
            key += (uint32_t)(c / SmoothTileShape<NO>::e[d]) * stride;
            stride *= (uint32_t)tl.nt[d];
        }
    }
    keys[p] = key;
    idx[p] = (uint32_t)p;
}

// start[k] = first position of the sorted keys with key >= k, for k = 0 .. tiles (start[tiles]: accepted points)
__global__ __launch_bounds__(kSmBlock) void k_smooth_ranges(const uint32_t* __restrict__ keys, uint32_t count,
                                                            uint64_t entries, int bits,
                                                            uint32_t* __restrict__ start) {
    const uint64_t k = (uint64_t)blockIdx.x * kSmBlock + threadIdx.x;
    if (k >= entries) return;
    start[k] = ord_lower_bound(keys, count, (uint32_t)k, bits);
}

template <typename T, int NI, int NO>
__global__ __launch_bounds__(kSmBlock) void k_smooth_tile(GridDesc<NO> gd, SmoothTiles<NO> tl, int64_t P, int64_t b,
                                                          T* __restrict__ out, const T* __restrict__ points,
                                                          const T* __restrict__ rot, const T* __restrict__ trans,
                                                          const T* __restrict__ ow, const T* __restrict__ pw,
                                                          const uint32_t* __restrict__ start,
                                                          const uint32_t* __restrict__ idx) {
    static_assert(NO == 2 || NO == 3, "the smooth splat is written for 2-D and 3-D grids");
    constexpr int NC = smooth_lds_cells<NO>();
    __shared__ double cells[NC];
    // the tile's run of the sorted points, clamped: a damaged table can shorten a walk, never leave idx[0 .. P)
    uint32_t begin, end;
    ord_cell_range(start, blockIdx.x, (uint32_t)P, begin, end);
    if (begin >= end) return;  // (uniform: an empty tile adds nothing)
    int org[NO];               // first cell of the tile
    {
        uint32_t t = blockIdx.x;
#pragma unroll
        for (int d = 0; d < NO; ++d) {
            org[d] = (int)(t % (uint32_t)tl.nt[d]) * SmoothTileShape<NO>::e[d];
            t /= (uint32_t)tl.nt[d];
        }
    }
    for (int i = threadIdx.x; i < NC; i += kSmBlock) cells[i] = 0.0;
    __syncthreads();

    const Pose<T, NI, NO> ps = load_pose<T, NI, NO>(rot, trans, ow, b);
    for (uint32_t i = begin + threadIdx.x; i < end; i += kSmBlock) {
        const uint32_t p = idx[i];
        if ((int64_t)p >= P) continue;  // (never for an index k_smooth_keys wrote)
        T pt[NI];
        load_point<T, NI>(points, (int64_t)p, pt);
        int j0[NO];
        T u[NO];
        if (!smooth_cell<T, NI, NO>(pt, ps, gd, j0, u)) continue;
        const T w = ps.ow * (pw ? pw[p] : T(1));
        // LDS cell l = (cell - org) + 1 per axis; only cells of the grid that lie on the tile + halo are added
        T wt[NO][3];
        int loff[NO][3];
        bool in[NO][3];
        int lstride = 1;
#pragma unroll
        for (int d = 0; d < NO; ++d) {
            spline_weights<T>(u[d], wt[d]);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int c = j0[d] + k - 1, l = c - org[d] + 1;
                in[d][k] = c >= 0 && c < gd.n[d] && l >= 0 && l < SmoothTileShape<NO>::e[d] + 2;
                loff[d][k] = in[d][k] ? l * lstride : 0;
            }
            lstride *= SmoothTileShape<NO>::e[d] + 2;
        }
#pragma unroll
        for (int k2 = 0; k2 < (NO == 3 ? 3 : 1); ++k2) {
            const bool in2 = NO == 3 ? in[NO - 1][k2] : true;
            const int off2 = NO == 3 ? loff[NO - 1][k2] : 0;
            const T w2 = NO == 3 ? wt[NO - 1][k2] * w : w;
#pragma unroll
            for (int k1 = 0; k1 < 3; ++k1) {
                const T w12 = wt[1][k1] * w2;
#pragma unroll
                for (int k0 = 0; k0 < 3; ++k0)
                    if (in2 && in[1][k1] && in[0][k0])
                        atomicAdd(&cells[off2 + loff[1][k1] + loff[0][k0]], (double)(wt[0][k0] * w12));
            }
        }
    }
    __syncthreads();

    // flush: consecutive threads walk axis 0 of the tile + halo, so a wave's atomics cover rows of `out`
    T* o = out + b * gd.G;
    for (int i = threadIdx.x; i < NC; i += kSmBlock) {
        const double v = cells[i];
        int rest = i, off = 0, stride = 1;
        bool in_grid = true;
#pragma unroll
        for (int d = 0; d < NO; ++d) {
            const int ext = SmoothTileShape<NO>::e[d] + 2;
            const int c = org[d] + (rest % ext) - 1;
            rest /= ext;
            in_grid = in_grid && c >= 0 && c < gd.n[d];
            off += in_grid ? c * stride : 0;
            stride *= gd.n[d];
        }
        if (in_grid && v != 0.0) atomic_add<T>(o + off, (T)v);
    }
}

// ---------------------------------------------------------------- forward-mode derivative of the smooth splat
// include/dpr.h, "SMOOTH SPLAT, FORWARD MODE".  For tangent k of an accepted (point, pose), with a and
// bc_n = ow * pw * cdot_n of jvp_coeffs (dpr_jvp.h), e_d = w_d and f_d = bc_d * w'_d:
//   deposit(s) = a * prod_d e_d + sum_n f_n * prod_{d != n} e_d = e_0 * X + f_0 * Y
//   2-D: X = a * e_1 + f_1,                  Y = e_1
//   3-D: X = e_1 * (a * e_2 + f_2) + f_1 * e_2,  Y = e_1 * e_2
// X and Y are formed once per (k1, k2): smooth_jvp_rows (dpr_smooth_device.h, shared with dpr_smooth_bodies.hip).
// out_dot holds the background tangent already (k_jvp_fill); plane (b, k) is at (b * K + k) * G.  These kernels are
// copies of k_smooth_fwd_atomic / k_smooth_tile, not shared bodies: the forward kernels keep their registers
// (DESIGN.md 4.15).

// One thread per point, the poses strided over gridDim.y (k_smooth_fwd_atomic's shape).  The cell, the weights and
// their derivatives once per accepted (point, pose); the K tangents are a run-time loop of 3^N atomics each.  A
// rejected point reads none of its tangents.
//
// Lanes of a wave that share a centre cell share all 3^N addresses.  A cloud with many points in a cell would send
// every one of them to the same few cells as fp32 atomics in arrival order: slow (they serialise) and, with deposits
// of both signs, noisy run to run.  So where a wave holds at least kSmJvpMinRun lanes whose neighbour lane has the
// same cell, up to kSmJvpGroups groups of lanes with equal cells are found (ballots, wave-uniform), each group's
// deposits are added across the wave in a fixed order (wave_sum) and its first lane issues one atomic per cell.
// Lanes outside the groups, and every lane of a wave without such runs, issue their own atomics.  A wave of
// a scattered cloud pays one shuffle per axis and one ballot per (point, pose) for the test.
constexpr int kSmJvpGroups = 4;   // groups of equal cells combined per wave
constexpr int kSmJvpTries = 8;    // cells looked at while searching for them
constexpr int kSmJvpMinRun = 8;   // lanes equal to their neighbour before a wave searches at all
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kSmBlock) void k_smooth_jvp_atomic(GridDesc<NO> gd, int64_t P, int64_t B, int K,
                                                                T* __restrict__ out_dot,
                                                                const T* __restrict__ points,
                                                                const T* __restrict__ rot,
                                                                const T* __restrict__ trans,
                                                                const T* __restrict__ ow, const T* __restrict__ pw,
                                                                JvpTangents<T> tan) {
    static_assert(NO == 2 || NO == 3, "the smooth splat is written for 2-D and 3-D grids");
    const int64_t p = (int64_t)blockIdx.x * kSmBlock + threadIdx.x;
    const bool live = p < P;  // (no early return: the wave sums below need every lane of the wave)
    const int lane = threadIdx.x & (kWave - 1);
    T pt[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) pt[j] = T(0);
    if (live) load_point<T, NI>(points, p, pt);
    const T pwi = (live && pw) ? pw[p] : T(1);
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        const Pose<T, NI, NO> ps = load_pose<T, NI, NO>(rot, trans, ow, b);
        int j0[NO];
        T u[NO];
        const bool ok = smooth_cell<T, NI, NO>(pt, ps, gd, j0, u) && live;
        const uint64_t okm = __ballot(ok);
        if (okm == 0) continue;  // (uniform)
        // groups of accepted lanes with equal cells: masks gm*, first lanes gl*; `solo`: lanes on their own
        uint64_t solo = okm, gm0 = 0, gm1 = 0, gm2 = 0, gm3 = 0;
        int gl0 = 0, gl1 = 0, gl2 = 0, gl3 = 0, ng = 0;
        {
            bool run = ok && lane > 0 && __shfl_up((int)ok, 1, kWave) != 0;
#pragma unroll
            for (int d = 0; d < NO; ++d) run = run && j0[d] == __shfl_up(j0[d], 1, kWave);
            if (__popcll(__ballot(run)) >= kSmJvpMinRun) {
                uint64_t todo = okm;
                for (int t = 0; t < kSmJvpTries && todo != 0 && ng < kSmJvpGroups; ++t) {
                    const int lead = __ffsll((unsigned long long)todo) - 1;
                    bool same = ok;
#pragma unroll
                    for (int d = 0; d < NO; ++d) same = same && j0[d] == __shfl(j0[d], lead, kWave);
                    const uint64_t m = __ballot(same);
                    todo &= ~m;
                    if (__popcll(m) > 1) {
                        solo &= ~m;
                        if (ng == 0) { gm0 = m; gl0 = lead; }
                        else if (ng == 1) { gm1 = m; gl1 = lead; }
                        else if (ng == 2) { gm2 = m; gl2 = lead; }
                        else { gm3 = m; gl3 = lead; }
                        ++ng;
                    }
                }
            }
        }
        const bool own = (solo >> lane) & 1;
        const SmoothAxes<T, NO> ax = smooth_axes<T, NO>(j0, u, gd);
        T dw[NO][3];
#pragma unroll
        for (int d = 0; d < NO; ++d) spline_derivatives<T>(u[d], dw[d]);
        T* o = out_dot + b * K * gd.G;
        for (int k = 0; k < K; ++k) {
            const JvpPose<T, NI, NO> tp = load_jvp_pose<T, NI, NO>(tan.rot, tan.trans, tan.ow, (int64_t)k * B + b);
            T pd[NI], pwd;
            load_jvp_point<T, NI>(ok ? tan.points : nullptr, ok ? tan.pw : nullptr, (int64_t)k * P + p, pd, pwd);
            T a, bc[NO];
            jvp_coeffs<T, NI, NO>(pt, pwi, pd, pwd, ps, tp, gd, a, bc);
            const SmoothJvpRows<T, NO> r = smooth_jvp_rows<T, NO>(a, bc, ax.w, dw);
            T f0[3];
#pragma unroll
            for (int k0 = 0; k0 < 3; ++k0) f0[k0] = bc[0] * dw[0][k0];
            T* ok_plane = o + (int64_t)k * gd.G;
#pragma unroll
            for (int k2 = 0; k2 < (NO == 3 ? 3 : 1); ++k2) {
                const bool in2 = NO == 3 ? ax.in[NO - 1][k2] : true;
                const int off2 = NO == 3 ? ax.off[NO - 1][k2] : 0;
#pragma unroll
                for (int k1 = 0; k1 < 3; ++k1) {
#pragma unroll
                    for (int k0 = 0; k0 < 3; ++k0) {
                        const bool in = ok && in2 && ax.in[1][k1] && ax.in[0][k0];
                        T* addr = ok_plane + (off2 + ax.off[1][k1] + ax.off[0][k0]);
                        const T dep = ax.w[0][k0] * r.X[k2][k1] + f0[k0] * r.Y[k2][k1];
                        for (int g = 0; g < ng; ++g) {  // (uniform; none in a wave without runs)
                            const uint64_t m = g == 0 ? gm0 : g == 1 ? gm1 : g == 2 ? gm2 : gm3;
                            const int lead = g == 0 ? gl0 : g == 1 ? gl1 : g == 2 ? gl2 : gl3;
                            const T s = wave_sum<T>(((m >> lane) & 1) ? dep : T(0));
                            if (lane == lead && in) atomic_add<T>(addr, s);
                        }
                        if (own && in) atomic_add<T>(addr, dep);
                    }
                }
            }
        }
    }
}

// Workgroup (tile, k) = (blockIdx.x, blockIdx.y): k_smooth_tile's walk over the tile's run of the sorted points,
// its LDS array, clamped-centre rule and flush, with the deposit of tangent k in the place of the weight product.
// Deposits have both signs; a cell whose sum is exactly 0 is skipped by the flush, which is right because the
// plane holds the background tangent already.
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kSmBlock) void k_smooth_tile_jvp(GridDesc<NO> gd, SmoothTiles<NO> tl, int64_t P,
                                                              int64_t B, int64_t b, int K, T* __restrict__ out_dot,
                                                              const T* __restrict__ points,
                                                              const T* __restrict__ rot, const T* __restrict__ trans,
                                                              const T* __restrict__ ow, const T* __restrict__ pw,
                                                              JvpTangents<T> tan, const uint32_t* __restrict__ start,
                                                              const uint32_t* __restrict__ idx) {
    static_assert(NO == 2 || NO == 3, "the smooth splat is written for 2-D and 3-D grids");
    constexpr int NC = smooth_lds_cells<NO>();
    __shared__ double cells[NC];
    uint32_t begin, end;
    ord_cell_range(start, blockIdx.x, (uint32_t)P, begin, end);
    if (begin >= end) return;  // (uniform: an empty tile adds nothing)
    const int64_t k = blockIdx.y;
    int org[NO];  // first cell of the tile
    {
        uint32_t t = blockIdx.x;
#pragma unroll
        for (int d = 0; d < NO; ++d) {
            org[d] = (int)(t % (uint32_t)tl.nt[d]) * SmoothTileShape<NO>::e[d];
            t /= (uint32_t)tl.nt[d];
        }
    }
    for (int i = threadIdx.x; i < NC; i += kSmBlock) cells[i] = 0.0;
    __syncthreads();

    const Pose<T, NI, NO> ps = load_pose<T, NI, NO>(rot, trans, ow, b);
    const JvpPose<T, NI, NO> tp = load_jvp_pose<T, NI, NO>(tan.rot, tan.trans, tan.ow, k * B + b);
    for (uint32_t i = begin + threadIdx.x; i < end; i += kSmBlock) {
        const uint32_t p = idx[i];
        if ((int64_t)p >= P) continue;  // (never for an index k_smooth_keys wrote)
        T pt[NI];
        load_point<T, NI>(points, (int64_t)p, pt);
        int j0[NO];
        T u[NO];
        if (!smooth_cell<T, NI, NO>(pt, ps, gd, j0, u)) continue;
        T pd[NI], pwd;
        load_jvp_point<T, NI>(tan.points, tan.pw, k * P + (int64_t)p, pd, pwd);
        T a, bc[NO];
        jvp_coeffs<T, NI, NO>(pt, pw ? pw[p] : T(1), pd, pwd, ps, tp, gd, a, bc);
        // LDS cell l = (cell - org) + 1 per axis; only cells of the grid that lie on the tile + halo are added
        T wt[NO][3], dw[NO][3];
        int loff[NO][3];
        bool in[NO][3];
        int lstride = 1;
#pragma unroll
        for (int d = 0; d < NO; ++d) {
            spline_weights<T>(u[d], wt[d]);
            spline_derivatives<T>(u[d], dw[d]);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int c = j0[d] + q - 1, l = c - org[d] + 1;
                in[d][q] = c >= 0 && c < gd.n[d] && l >= 0 && l < SmoothTileShape<NO>::e[d] + 2;
                loff[d][q] = in[d][q] ? l * lstride : 0;
            }
            lstride *= SmoothTileShape<NO>::e[d] + 2;
        }
        const SmoothJvpRows<T, NO> r = smooth_jvp_rows<T, NO>(a, bc, wt, dw);
        T f0[3];
#pragma unroll
        for (int k0 = 0; k0 < 3; ++k0) f0[k0] = bc[0] * dw[0][k0];
#pragma unroll
        for (int k2 = 0; k2 < (NO == 3 ? 3 : 1); ++k2) {
            const bool in2 = NO == 3 ? in[NO - 1][k2] : true;
            const int off2 = NO == 3 ? loff[NO - 1][k2] : 0;
#pragma unroll
            for (int k1 = 0; k1 < 3; ++k1) {
#pragma unroll
                for (int k0 = 0; k0 < 3; ++k0)
                    if (in2 && in[1][k1] && in[0][k0])
                        atomicAdd(&cells[off2 + loff[1][k1] + loff[0][k0]],
                                  (double)(wt[0][k0] * r.X[k2][k1] + f0[k0] * r.Y[k2][k1]));
            }
        }
    }
    __syncthreads();

    // flush: consecutive threads walk axis 0 of the tile + halo, so a wave's atomics cover rows of the plane
    T* o = out_dot + (b * K + k) * gd.G;
    for (int i = threadIdx.x; i < NC; i += kSmBlock) {
        const double v = cells[i];
        int rest = i, off = 0, stride = 1;
        bool in_grid = true;
#pragma unroll
        for (int d = 0; d < NO; ++d) {
            const int ext = SmoothTileShape<NO>::e[d] + 2;
            const int c = org[d] + (rest % ext) - 1;
            rest /= ext;
            in_grid = in_grid && c >= 0 && c < gd.n[d];
            off += in_grid ? c * stride : 0;
            stride *= gd.n[d];
        }
        if (in_grid && v != 0.0) atomic_add<T>(o + off, (T)v);
    }
}

// ---------------------------------------------------------------- per-pose clouds
// include/dpr.h, "SMOOTH SPLAT, PER-POSE CLOUDS": pose b reads cloud b (points at b * P * NI, weights at b * P).
// Plane b and the gradients of pose b are those of the single-pose kernels above for (cloud b, pose b).  These are
// copies of k_smooth_fwd_atomic / k_smooth_bwd / k_smooth_keys / k_smooth_tile, not shared bodies: the single-pose
// kernels keep their registers.

// One thread per (point, pose): a block lies inside one pose, the poses strided over gridDim.y.
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kSmBlock) void k_smooth_clouds_fwd_atomic(GridDesc<NO> gd, int64_t P, int64_t B,
                                                                       T* __restrict__ out,
                                                                       const T* __restrict__ points,
                                                                       const T* __restrict__ rot,
                                                                       const T* __restrict__ trans,
                                                                       const T* __restrict__ ow,
                                                                       const T* __restrict__ pw) {
    static_assert(NO == 2 || NO == 3, "the smooth splat is written for 2-D and 3-D grids");
    const int64_t p = (int64_t)blockIdx.x * kSmBlock + threadIdx.x;
    if (p >= P) return;
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        T pt[NI];
        load_point<T, NI>(points + b * P * NI, p, pt);
        const T pwi = pw ? pw[b * P + p] : T(1);
        const Pose<T, NI, NO> ps = load_pose<T, NI, NO>(rot, trans, ow, b);
        int j0[NO];
        T u[NO];
        if (!smooth_cell<T, NI, NO>(pt, ps, gd, j0, u)) continue;
        const T w = ps.ow * pwi;
        const SmoothAxes<T, NO> ax = smooth_axes<T, NO>(j0, u, gd);
        T* o = out + b * gd.G;
#pragma unroll
        for (int k2 = 0; k2 < (NO == 3 ? 3 : 1); ++k2) {
            const bool in2 = NO == 3 ? ax.in[NO - 1][k2] : true;
            const int off2 = NO == 3 ? ax.off[NO - 1][k2] : 0;
            const T w2 = NO == 3 ? ax.w[NO - 1][k2] * w : w;
#pragma unroll
            for (int k1 = 0; k1 < 3; ++k1) {
                const T w12 = ax.w[1][k1] * w2;
#pragma unroll
                for (int k0 = 0; k0 < 3; ++k0)
                    if (in2 && ax.in[1][k1] && ax.in[0][k0])
                        atomic_add<T>(o + (off2 + ax.off[1][k1] + ax.off[0][k0]), ax.w[0][k0] * w12);
            }
        }
    }
}

// Pullback, one thread per (point, pose), a block inside one pose: the point gradients are one plain store each
// (a rejected point stores 0), the per-pose sums go wave -> block -> one atomic per scalar per block.  Pre-zeroed:
// ds_drotation, ds_dtranslation, ds_dout_weight.
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kSmBlock) void k_smooth_clouds_bwd(
    GridDesc<NO> gd, int64_t P, int64_t B, const T* __restrict__ g, const T* __restrict__ points,
    const T* __restrict__ rot, const T* __restrict__ trans, const T* __restrict__ ow, const T* __restrict__ pw,
    T* __restrict__ ds_dpoints, T* __restrict__ ds_drotation, T* __restrict__ ds_dtranslation,
    T* __restrict__ ds_dout_weight, T* __restrict__ ds_dpoint_weight) {
    static_assert(NO == 2 || NO == 3, "the smooth splat is written for 2-D and 3-D grids");
    constexpr int NV = NO * NI + NO + 1;  // dR | dt | d out_weight
    constexpr int NW = kSmBlock / kWave;
    __shared__ T red[NW][NV];

    const int64_t p = (int64_t)blockIdx.x * kSmBlock + threadIdx.x;
    const bool live = p < P;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {  // (uniform over the block)
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
        int j0[NO];
        T u[NO];
        if (live && smooth_cell<T, NI, NO>(pt, ps, gd, j0, u)) {
            const T* gb = g + b * gd.G;
            T dcoord[NO], W;
            smooth_point_backward<T, NO>(j0, u, gd, [&](int off) { return gb[off]; }, dcoord, W);
            const T opw = ps.ow * pwi;
            T scaled[NO];
#pragma unroll
            for (int n = 0; n < NO; ++n) scaled[n] = (dcoord[n] * opw) * (T(gd.n[n]) / T(2));
#pragma unroll
            for (int n = 0; n < NO; ++n) {
#pragma unroll
                for (int j = 0; j < NI; ++j) vals[n + j * NO] = scaled[n] * pt[j];
                vals[NO * NI + n] = scaled[n];
            }
            vals[NO * NI + NO] = W * pwi;
#pragma unroll
            for (int j = 0; j < NI; ++j) {  // rotation' * scaled
                T v = ps.R[0 + j * NO] * scaled[0];
#pragma unroll
                for (int n = 1; n < NO; ++n) v = v + ps.R[n + j * NO] * scaled[n];
                gpt[j] += v;
            }
            gpw += W * ps.ow;
        }
        if (live) {
#pragma unroll
            for (int j = 0; j < NI; ++j) ds_dpoints[q * NI + j] = gpt[j];
            if (ds_dpoint_weight) ds_dpoint_weight[q] = gpw;
        }
        // per-pose sums: wave -> block -> one atomic per scalar per block
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

// DPR_ALGO_TILED, the binning of a GROUP of nb poses b0 .. b0 + nb - 1 at once.  `points` / `pw` are those of the
// group's first cloud; the flat index q = b_local * P + p addresses them directly (consecutive clouds are
// contiguous).  key = b_local * tiles + (tile of the clamped centre cell, as k_smooth_keys), all ones for a rejected
// point; value = q.  Block blockIdx.x covers points (blockIdx.x % blocks_per_pose) * 256 .. of pose
// blockIdx.x / blocks_per_pose: a block lies inside one pose.
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kSmBlock) void k_smooth_clouds_keys(GridDesc<NO> gd, SmoothTiles<NO> tl, uint32_t tiles,
                                                                 int64_t P, uint32_t blocks_per_pose, int64_t b0,
                                                                 const T* __restrict__ points,
                                                                 const T* __restrict__ rot,
                                                                 const T* __restrict__ trans,
                                                                 uint32_t* __restrict__ keys,
                                                                 uint32_t* __restrict__ idx) {
    const uint32_t bl = blockIdx.x / blocks_per_pose;
    const int64_t p = (int64_t)(blockIdx.x % blocks_per_pose) * kSmBlock + threadIdx.x;
    if (p >= P) return;
    const int64_t q = (int64_t)bl * P + p;
    T pt[NI];
    load_point<T, NI>(points, q, pt);
    const Pose<T, NI, NO> ps = load_pose<T, NI, NO>(rot, trans, nullptr, b0 + bl);
    int j0[NO];
    T u[NO];
    uint32_t key = kSmoothNoKey;
    if (smooth_cell<T, NI, NO>(pt, ps, gd, j0, u)) {
        uint32_t stride = 1;
        key = bl * tiles;
#pragma unroll
        for (int d = 0; d < NO; ++d) {
            const int c = j0[d] < 0 ? 0 : (j0[d] >= gd.n[d] ? gd.n[d] - 1 : j0[d]);
            key += (uint32_t)(c / SmoothTileShape<NO>::e[d]) * stride;
            stride *= (uint32_t)tl.nt[d];
        }
    }
    keys[q] = key;
    idx[q] = (uint32_t)q;
}

// Workgroup blockIdx.x = b_local * tiles + tile: k_smooth_tile's body for the (pose, tile)'s run of the group's
// sorted flat indices (`count` of them: nb * P), flushed onto plane b0 + b_local.
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kSmBlock) void k_smooth_clouds_tile(GridDesc<NO> gd, SmoothTiles<NO> tl, uint32_t tiles,
                                                                 uint32_t count, int64_t b0, T* __restrict__ out,
                                                                 const T* __restrict__ points,
                                                                 const T* __restrict__ rot,
                                                                 const T* __restrict__ trans,
                                                                 const T* __restrict__ ow, const T* __restrict__ pw,
                                                                 const uint32_t* __restrict__ start,
                                                                 const uint32_t* __restrict__ idx) {
    static_assert(NO == 2 || NO == 3, "the smooth splat is written for 2-D and 3-D grids");
    constexpr int NC = smooth_lds_cells<NO>();
    __shared__ double cells[NC];
    // the run of the sorted indices, clamped: a damaged table can shorten a walk, never leave idx[0 .. count)
    uint32_t begin, end;
    ord_cell_range(start, blockIdx.x, count, begin, end);
    if (begin >= end) return;  // (uniform: an empty (pose, tile) adds nothing)
    const int64_t b = b0 + (int64_t)(blockIdx.x / tiles);
    int org[NO];  // first cell of the tile
    {
        uint32_t t = blockIdx.x % tiles;
#pragma unroll
        for (int d = 0; d < NO; ++d) {
            org[d] = (int)(t % (uint32_t)tl.nt[d]) * SmoothTileShape<NO>::e[d];
            t /= (uint32_t)tl.nt[d];
        }
    }
    for (int i = threadIdx.x; i < NC; i += kSmBlock) cells[i] = 0.0;
    __syncthreads();

    const Pose<T, NI, NO> ps = load_pose<T, NI, NO>(rot, trans, ow, b);
    for (uint32_t i = begin + threadIdx.x; i < end; i += kSmBlock) {
        const uint32_t q = idx[i];
        if (q >= count) continue;  // (never for an index k_smooth_clouds_keys wrote)
        T pt[NI];
        load_point<T, NI>(points, (int64_t)q, pt);
        int j0[NO];
        T u[NO];
        if (!smooth_cell<T, NI, NO>(pt, ps, gd, j0, u)) continue;
        const T w = ps.ow * (pw ? pw[q] : T(1));
        // LDS cell l = (cell - org) + 1 per axis; only cells of the grid that lie on the tile + halo are added
        T wt[NO][3];
        int loff[NO][3];
        bool in[NO][3];
        int lstride = 1;
#pragma unroll
        for (int d = 0; d < NO; ++d) {
            spline_weights<T>(u[d], wt[d]);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int c = j0[d] + k - 1, l = c - org[d] + 1;
                in[d][k] = c >= 0 && c < gd.n[d] && l >= 0 && l < SmoothTileShape<NO>::e[d] + 2;
                loff[d][k] = in[d][k] ? l * lstride : 0;
            }
            lstride *= SmoothTileShape<NO>::e[d] + 2;
        }
#pragma unroll
        for (int k2 = 0; k2 < (NO == 3 ? 3 : 1); ++k2) {
            const bool in2 = NO == 3 ? in[NO - 1][k2] : true;
            const int off2 = NO == 3 ? loff[NO - 1][k2] : 0;
            const T w2 = NO == 3 ? wt[NO - 1][k2] * w : w;
#pragma unroll
            for (int k1 = 0; k1 < 3; ++k1) {
                const T w12 = wt[1][k1] * w2;
#pragma unroll
                for (int k0 = 0; k0 < 3; ++k0)
                    if (in2 && in[1][k1] && in[0][k0])
                        atomicAdd(&cells[off2 + loff[1][k1] + loff[0][k0]], (double)(wt[0][k0] * w12));
            }
        }
    }
    __syncthreads();

    // flush: consecutive threads walk axis 0 of the tile + halo, so a wave's atomics cover rows of the plane
    T* o = out + b * gd.G;
    for (int i = threadIdx.x; i < NC; i += kSmBlock) {
        const double v = cells[i];
        int rest = i, off = 0, stride = 1;
        bool in_grid = true;
#pragma unroll
        for (int d = 0; d < NO; ++d) {
            const int ext = SmoothTileShape<NO>::e[d] + 2;
            const int c = org[d] + (rest % ext) - 1;
            rest /= ext;
            in_grid = in_grid && c >= 0 && c < gd.n[d];
            off += in_grid ? c * stride : 0;
            stride *= gd.n[d];
        }
        if (in_grid && v != 0.0) atomic_add<T>(o + off, (T)v);
    }
}

// ---------------------------------------------------------------- host
int64_t smooth_tile_count(int n_out, const int64_t* grid, int64_t P) {
    if (P > (int64_t)0xfffffffeLL) return 0;
    const int64_t tiles = n_out == 2 ? smooth_tiles<2>(grid).tiles : n_out == 3 ? smooth_tiles<3>(grid).tiles : 0;
    return tiles < (int64_t)0x7fffffffLL ? tiles : 0;  // (also the largest launch: one workgroup per tile)
}

// The workspace of a call of B images that bins `group` of them at a time, `tiles` tiles and P points each: offsets of
// its pieces and `total` bytes (all 0 for P <= 0).  The storage sorts group * P pairs, and (B % group) * P in a
// shorter last group, whose sort may ask for more temporary bytes.  The one plan of every tiled smooth launcher
// (smooth_binning) and of both workspace queries below.
struct SmoothPlan {
    size_t off_keys_in, off_keys_out, off_idx_in, off_idx_out, off_temp, temp_bytes, off_start, total;
};
static SmoothPlan smooth_plan(int64_t tiles, int64_t P, int64_t B, int64_t group) {
    SmoothPlan pl{};
    if (P <= 0) return pl;
    const int64_t count = group * P, last = (B % group) * P;
    size_t o = 0;
    pl.off_keys_in = o;  o += align_up((size_t)count * 4);
    pl.off_keys_out = o; o += align_up((size_t)count * 4);
    pl.off_idx_in = o;   o += align_up((size_t)count * 4);
    pl.off_idx_out = o;  o += align_up((size_t)count * 4);
    pl.off_temp = o;
    pl.temp_bytes = radix_pairs_temp_bytes(count);
    if (last > 0 && radix_pairs_temp_bytes(last) > pl.temp_bytes) pl.temp_bytes = radix_pairs_temp_bytes(last);
    o += align_up(pl.temp_bytes);
    pl.off_start = o;    o += align_up((size_t)(group * tiles + 1) * 4);
    pl.total = o;
    return pl;
}

size_t smooth_tiled_workspace_bytes(int n_out, const int64_t* grid, int64_t P) {
    return smooth_clouds_tiled_workspace_bytes(n_out, grid, P, 1, 1);
}

template <typename T, int NI, int NO>
int smooth_fwd_atomic(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, T* out, const T* points,
                      const T* rot, const T* trans, const T* ow, const T* pw) {
    if (P <= 0 || B <= 0) return DPR_OK;
    const GridDesc<NO> gd = make_grid_desc<NO>(grid, G);
    dim3 g((unsigned)((P + kSmBlock - 1) / kSmBlock), (unsigned)(B < 65535 ? B : 65535));
    hipLaunchKernelGGL((k_smooth_fwd_atomic<T, NI, NO>), g, dim3(kSmBlock), 0, st, gd, P, B, out, points, rot, trans,
                       ow, pw);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

// What the tiled launchers share (declared in dpr_smooth.h): the tiles and workspace pieces of a call
// (smooth_binning), what follows a key kernel (smooth_sort_group), and the binning of one pose (smooth_bin_pose).
// (No entry point reaches the workspace message: each has compared ws_bytes with the query's answer, the same plan.)
template <int NO>
int smooth_binning(const int64_t* grid, int64_t G, int64_t P, int64_t B, int64_t group, void* ws_, size_t ws_bytes,
                   SmoothBinning<NO>* sb) {
    const int64_t tiles = smooth_tile_count(NO, grid, P);
    if (tiles == 0 || group == 0) return fail(DPR_ERR_UNSUPPORTED_ALGO, kSmoothTiledRefused);
    const SmoothPlan pl = smooth_plan(tiles, P, B, group);
    if (!ws_ || ws_bytes < pl.total)
        return fail(DPR_ERR_WORKSPACE, "smooth DPR_ALGO_TILED needs %zu workspace bytes, got %zu", pl.total,
                    ws_ ? ws_bytes : (size_t)0);
    char* ws = (char*)ws_;
    sb->gd = make_grid_desc<NO>(grid, G);
    sb->tl = smooth_tiles<NO>(grid);
    sb->tiles = tiles;
    sb->group = group;
    sb->temp = ws + pl.off_temp;
    sb->temp_bytes = pl.temp_bytes;
    sb->keys_in = (uint32_t*)(ws + pl.off_keys_in);
    sb->keys_out = (uint32_t*)(ws + pl.off_keys_out);
    sb->idx_in = (uint32_t*)(ws + pl.off_idx_in);
    sb->idx_out = (uint32_t*)(ws + pl.off_idx_out);
    sb->start = (uint32_t*)(ws + pl.off_start);
    return DPR_OK;
}
template <int NO> int smooth_sort_group(hipStream_t st, const SmoothBinning<NO>& sb, int64_t nb, int64_t P) {
    const int64_t count = nb * P, entries = nb * sb.tiles + 1;
    const int bits = ord_key_bits((uint64_t)(nb * sb.tiles));
    stage_mark(st);
    DPR_HIP(radix_sort_pairs_u32(sb.temp, sb.temp_bytes, sb.keys_in, sb.keys_out, sb.idx_in, sb.idx_out,
                                 (size_t)count, 0u, (unsigned)bits, st));
    stage_mark(st);
    hipLaunchKernelGGL(k_smooth_ranges, dim3((unsigned)((entries + kSmBlock - 1) / kSmBlock)), dim3(kSmBlock), 0, st,
                       (const uint32_t*)sb.keys_out, (uint32_t)count, (uint64_t)entries, bits, sb.start);
    DPR_HIP(hipGetLastError());
    stage_mark(st);
    return DPR_OK;
}
template <typename T, int NI, int NO>
int smooth_bin_pose(hipStream_t st, const SmoothBinning<NO>& sb, int64_t P, int64_t b, const T* points,
                    const T* rot, const T* trans) {
    hipLaunchKernelGGL((k_smooth_keys<T, NI, NO>), dim3((unsigned)((P + kSmBlock - 1) / kSmBlock)), dim3(kSmBlock), 0,
                       st, sb.gd, sb.tl, P, b, points, rot, trans, sb.keys_in, sb.idx_in);
    return smooth_sort_group<NO>(st, sb, 1, P);
}

template <typename T, int NI, int NO>
int smooth_fwd_tiled(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, T* out, const T* points,
                     const T* rot, const T* trans, const T* ow, const T* pw, void* ws, size_t ws_bytes) {
    if (P <= 0 || B <= 0) return DPR_OK;
    SmoothBinning<NO> sb;
    if (int rc = smooth_binning<NO>(grid, G, P, B, 1, ws, ws_bytes, &sb)) return rc;
    for (int64_t b = 0; b < B; ++b) {
        if (int rc = smooth_bin_pose<T, NI, NO>(st, sb, P, b, points, rot, trans)) return rc;
        hipLaunchKernelGGL((k_smooth_tile<T, NI, NO>), dim3((unsigned)sb.tiles), dim3(kSmBlock), 0, st, sb.gd, sb.tl,
                           P, b, out, points, rot, trans, ow, pw, (const uint32_t*)sb.start,
                           (const uint32_t*)sb.idx_out);
        stage_mark(st);
    }
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

// ---- per-pose clouds
int64_t smooth_clouds_group(int n_out, const int64_t* grid, int64_t P, int64_t B, int max_group) {
    const int64_t tiles = smooth_tile_count(n_out, grid, P);
    if (tiles == 0) return 0;
    const int64_t per_pose = P > tiles ? P : tiles;
    int64_t bg = kSmoothCloudsGroupWork / per_pose;
    if (bg > B) bg = B;
    if (max_group > 0 && bg > max_group) bg = max_group;
    return bg < 1 ? 1 : bg;
}

size_t smooth_clouds_tiled_workspace_bytes(int n_out, const int64_t* grid, int64_t P, int64_t B, int max_group) {
    const int64_t bg = smooth_clouds_group(n_out, grid, P, B, max_group);
    if (bg == 0) return (size_t)-1;
    return smooth_plan(smooth_tile_count(n_out, grid, P), P, B, bg).total;
}

template <typename T, int NI, int NO>
int smooth_clouds_fwd_atomic(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, T* out,
                             const T* points, const T* rot, const T* trans, const T* ow, const T* pw) {
    if (P <= 0 || B <= 0) return DPR_OK;
    const GridDesc<NO> gd = make_grid_desc<NO>(grid, G);
    dim3 g((unsigned)((P + kSmBlock - 1) / kSmBlock), (unsigned)(B < 65535 ? B : 65535));
    hipLaunchKernelGGL((k_smooth_clouds_fwd_atomic<T, NI, NO>), g, dim3(kSmBlock), 0, st, gd, P, B, out, points, rot,
                       trans, ow, pw);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

template <typename T, int NI, int NO>
int smooth_clouds_bwd_atomic(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, const T* g,
                             const T* points, const T* rot, const T* trans, const T* ow, const T* pw, T* d_pts,
                             T* d_rot, T* d_trans, T* d_ow, T* d_pw) {
    if (P <= 0 || B <= 0) return DPR_OK;
    const GridDesc<NO> gd = make_grid_desc<NO>(grid, G);
    dim3 gg((unsigned)((P + kSmBlock - 1) / kSmBlock), (unsigned)(B < 65535 ? B : 65535));
    hipLaunchKernelGGL((k_smooth_clouds_bwd<T, NI, NO>), gg, dim3(kSmBlock), 0, st, gd, P, B, g, points, rot, trans,
                       ow, pw, d_pts, d_rot, d_trans, d_ow, d_pw);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

// group after group of sb.group poses: keys -> sort -> start table -> tiles, four launches per GROUP (the last group
// may hold fewer poses)
template <typename T, int NI, int NO>
int smooth_clouds_fwd_tiled(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int max_group,
                            T* out, const T* points, const T* rot, const T* trans, const T* ow, const T* pw,
                            void* ws, size_t ws_bytes) {
    if (P <= 0 || B <= 0) return DPR_OK;
    SmoothBinning<NO> sb;
    if (int rc = smooth_binning<NO>(grid, G, P, B, smooth_clouds_group(NO, grid, P, B, max_group), ws, ws_bytes, &sb))
        return rc;
    const int64_t blocks_per_pose = (P + kSmBlock - 1) / kSmBlock;
    const dim3 blk(kSmBlock);
    for (int64_t b0 = 0; b0 < B; b0 += sb.group) {
        const int64_t nb = B - b0 < sb.group ? B - b0 : sb.group;
        const T* gpts = points + b0 * P * NI;
        const T* gpw = pw ? pw + b0 * P : nullptr;
        hipLaunchKernelGGL((k_smooth_clouds_keys<T, NI, NO>), dim3((unsigned)(nb * blocks_per_pose)), blk, 0, st,
                           sb.gd, sb.tl, (uint32_t)sb.tiles, P, (uint32_t)blocks_per_pose, b0, gpts, rot, trans,
                           sb.keys_in, sb.idx_in);
        if (int rc = smooth_sort_group<NO>(st, sb, nb, P)) return rc;
        hipLaunchKernelGGL((k_smooth_clouds_tile<T, NI, NO>), dim3((unsigned)(nb * sb.tiles)), blk, 0, st, sb.gd,
                           sb.tl, (uint32_t)sb.tiles, (uint32_t)(nb * P), b0, out, gpts, rot, trans, ow, gpw,
                           (const uint32_t*)sb.start, (const uint32_t*)sb.idx_out);
        stage_mark(st);
    }
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

template <typename T, int NI, int NO>
int smooth_jvp_atomic(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int K, T* out_dot,
                      const T* points, const T* rot, const T* trans, const T* ow, const T* pw, JvpTangents<T> tan) {
    if (P <= 0 || B <= 0) return DPR_OK;
    const GridDesc<NO> gd = make_grid_desc<NO>(grid, G);
    dim3 g((unsigned)((P + kSmBlock - 1) / kSmBlock), (unsigned)(B < 65535 ? B : 65535));
    hipLaunchKernelGGL((k_smooth_jvp_atomic<T, NI, NO>), g, dim3(kSmBlock), 0, st, gd, P, B, K, out_dot, points, rot,
                       trans, ow, pw, tan);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

// per pose: the binning of smooth_fwd_tiled, then ONE launch over (tiles, K): a binning serves all K tangents
template <typename T, int NI, int NO>
int smooth_jvp_tiled(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int K, T* out_dot,
                     const T* points, const T* rot, const T* trans, const T* ow, const T* pw, JvpTangents<T> tan,
                     void* ws, size_t ws_bytes) {
    if (P <= 0 || B <= 0) return DPR_OK;
    SmoothBinning<NO> sb;
    if (int rc = smooth_binning<NO>(grid, G, P, B, 1, ws, ws_bytes, &sb)) return rc;
    for (int64_t b = 0; b < B; ++b) {
        if (int rc = smooth_bin_pose<T, NI, NO>(st, sb, P, b, points, rot, trans)) return rc;
        hipLaunchKernelGGL((k_smooth_tile_jvp<T, NI, NO>), dim3((unsigned)sb.tiles, (unsigned)K), dim3(kSmBlock), 0,
                           st, sb.gd, sb.tl, P, B, b, K, out_dot, points, rot, trans, ow, pw, tan,
                           (const uint32_t*)sb.start, (const uint32_t*)sb.idx_out);
        stage_mark(st);
    }
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

template <typename T, int NI, int NO>
int smooth_bwd_atomic(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, const T* g,
                      const T* points, const T* rot, const T* trans, const T* ow, const T* pw, T* d_pts, T* d_rot,
                      T* d_trans, T* d_ow, T* d_pw, int poses_per_slice, int64_t slices) {
    if (P <= 0 || B <= 0) return DPR_OK;
    const GridDesc<NO> gd = make_grid_desc<NO>(grid, G);
    const int accumulate = slices > 1;
    if (accumulate) {
        DPR_HIP(zero_async(st, d_pts, sizeof(T) * (size_t)(P * NI)));
        if (d_pw) DPR_HIP(zero_async(st, d_pw, sizeof(T) * (size_t)P));
    }
    dim3 gg((unsigned)((P + kSmBlock - 1) / kSmBlock), (unsigned)slices);
    hipLaunchKernelGGL((k_smooth_bwd<T, NI, NO>), gg, dim3(kSmBlock), 0, st, gd, P, B, g, points, rot, trans, ow, pw,
                       d_pts, d_rot, d_trans, d_ow, d_pw, poses_per_slice, accumulate);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

template <typename T, int NI, int NO>
int sample_smooth_fwd(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, T* values, const T* image,
                      const T* points, const T* rot, const T* trans, int poses_per_slice, int64_t slices) {
    if (P <= 0 || B <= 0) return DPR_OK;
    const GridDesc<NO> gd = make_grid_desc<NO>(grid, G);
    dim3 gg((unsigned)((P + kSmBlock - 1) / kSmBlock), (unsigned)slices);
    hipLaunchKernelGGL((k_sample_smooth_fwd<T, NI, NO>), gg, dim3(kSmBlock), 0, st, gd, P, B, values, image, points,
                       rot, trans, poses_per_slice);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

template <typename T, int NI, int NO>
int sample_smooth_bwd(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, const T* dv,
                      const T* image, const T* points, const T* rot, const T* trans, T* d_img, T* d_pts, T* d_rot,
                      T* d_trans, int poses_per_slice, int64_t slices) {
    if (P <= 0 || B <= 0 || !(d_img || d_pts || d_rot || d_trans)) return DPR_OK;
    const GridDesc<NO> gd = make_grid_desc<NO>(grid, G);
    const int accumulate = slices > 1;
    if (accumulate && d_pts) DPR_HIP(zero_async(st, d_pts, sizeof(T) * (size_t)(P * NI)));
    dim3 gg((unsigned)((P + kSmBlock - 1) / kSmBlock), (unsigned)slices);
    hipLaunchKernelGGL((k_sample_smooth_bwd<T, NI, NO>), gg, dim3(kSmBlock), 0, st, gd, P, B, dv, image, points, rot,
                       trans, d_img, d_pts, d_rot, d_trans, poses_per_slice, accumulate);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

template int smooth_binning<2>(const int64_t*, int64_t, int64_t, int64_t, int64_t, void*, size_t, SmoothBinning<2>*);
template int smooth_binning<3>(const int64_t*, int64_t, int64_t, int64_t, int64_t, void*, size_t, SmoothBinning<3>*);
template int smooth_sort_group<2>(hipStream_t, const SmoothBinning<2>&, int64_t, int64_t);
template int smooth_sort_group<3>(hipStream_t, const SmoothBinning<3>&, int64_t, int64_t);

#define DPR_SMOOTH_INSTANTIATE(T, NI, NO)                                                                           \
    template int smooth_bin_pose<T, NI, NO>(hipStream_t, const SmoothBinning<NO>&, int64_t, int64_t, const T*,      \
                                            const T*, const T*);                                                   \
    template int sample_smooth_fwd<T, NI, NO>(hipStream_t, const int64_t*, int64_t, int64_t, int64_t, T*, const T*, \
                                              const T*, const T*, const T*, int, int64_t);                         \
    template int sample_smooth_bwd<T, NI, NO>(hipStream_t, const int64_t*, int64_t, int64_t, int64_t, const T*,     \
                                              const T*, const T*, const T*, const T*, T*, T*, T*, T*, int,         \
                                              int64_t);                                                            \
    template int smooth_fwd_atomic<T, NI, NO>(hipStream_t, const int64_t*, int64_t, int64_t, int64_t, T*, const T*, \
                                              const T*, const T*, const T*, const T*);                             \
    template int smooth_fwd_tiled<T, NI, NO>(hipStream_t, const int64_t*, int64_t, int64_t, int64_t, T*, const T*,  \
                                             const T*, const T*, const T*, const T*, void*, size_t);               \
    template int smooth_jvp_atomic<T, NI, NO>(hipStream_t, const int64_t*, int64_t, int64_t, int64_t, int, T*,      \
                                              const T*, const T*, const T*, const T*, const T*, JvpTangents<T>);   \
    template int smooth_jvp_tiled<T, NI, NO>(hipStream_t, const int64_t*, int64_t, int64_t, int64_t, int, T*,       \
                                             const T*, const T*, const T*, const T*, const T*, JvpTangents<T>,     \
                                             void*, size_t);                                                       \
    template int smooth_bwd_atomic<T, NI, NO>(hipStream_t, const int64_t*, int64_t, int64_t, int64_t, const T*,     \
                                              const T*, const T*, const T*, const T*, const T*, T*, T*, T*, T*,    \
                                              T*, int, int64_t);                                                   \
    template int smooth_clouds_fwd_atomic<T, NI, NO>(hipStream_t, const int64_t*, int64_t, int64_t, int64_t, T*,    \
                                                     const T*, const T*, const T*, const T*, const T*);            \
    template int smooth_clouds_fwd_tiled<T, NI, NO>(hipStream_t, const int64_t*, int64_t, int64_t, int64_t, int,    \
                                                    T*, const T*, const T*, const T*, const T*, const T*, void*,   \
                                                    size_t);                                                       \
    template int smooth_clouds_bwd_atomic<T, NI, NO>(hipStream_t, const int64_t*, int64_t, int64_t, int64_t,        \
                                                     const T*, const T*, const T*, const T*, const T*, const T*,   \
                                                     T*, T*, T*, T*, T*);
#define DPR_SMOOTH_INSTANTIATE_T(T) \
    DPR_SMOOTH_INSTANTIATE(T, 2, 2) DPR_SMOOTH_INSTANTIATE(T, 3, 3) DPR_SMOOTH_INSTANTIATE(T, 3, 2)
DPR_SMOOTH_INSTANTIATE_T(float)
DPR_SMOOTH_INSTANTIATE_T(double)

}  // namespace dpr
