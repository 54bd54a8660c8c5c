// The smooth splat with C weights per point (include/dpr.h, "SMOOTH SPLAT, MULTI-CHANNEL"): the cell, the B-spline
// weights and the offsets of a (point, pose) are computed once and serve all C channels.
//
//   out / ds_dout   (n_1, .., n_N, C, B): plane (c, b) at (b * C + c) * G
//   point_weight    P x C, a point's C weights contiguous; ds_dpoint_weight likewise
//
//   DPR_ALGO_ATOMIC forward   k_smooth_ch_fwd_atomic: k_smooth_fwd_atomic's shape (a thread per point, the pose loop
//                             inside), C global atomics per accepted cell
//   DPR_ALGO_TILED forward    per pose the binning of the smooth forward (smooth_bin_pose: keys -> sort -> start
//                             table), then ONE launch of k_smooth_ch_tile over (tiles, chunks of kSmChTile channels):
//                             a workgroup keeps the f64 tile + halo of its channels in LDS, walks its run of the
//                             sorted points once and flushes channel after channel
//   DPR_ALGO_ATOMIC pullback  k_smooth_ch_bwd: k_smooth_bwd's shape and tail; weights, derivatives and offsets once
//                             per (point, pose), the separable contraction once per channel; one launch for all C
//                             channels behind a compile-time bound of 4 or kMaxChannels (no scratch at either)
#include <hip/hip_runtime.h>

#include "../../include/dpr.h"
#include "dpr_ordered.h"
#include "dpr_ordered_index.h"
#include "dpr_smooth.h"
#include "dpr_smooth_device.h"

namespace dpr {

// channels a workgroup of the tiled forward holds in LDS: 3-D 2 x 14 400 = 28 800 bytes, 2-D 2 x 9 504 = 19 008
// (profiles/smooth_channels_probe.txt has the measurements of 1, 2 and 4)
constexpr int kSmChTile = 2;

// the weights of channels c0 .. c0 + CB - 1 of point p (0 for a channel >= C: it deposits and gathers nothing)
template <typename T, int CB>
__device__ __forceinline__ void load_smooth_channel_weights(const T* __restrict__ pw, int64_t p, int C, int c0,
                                                            T (&w)[CB]) {
#pragma unroll
    for (int c = 0; c < CB; ++c) w[c] = (c0 + c < C) ? pw[p * C + (c0 + c)] : T(0);
}

// ---------------------------------------------------------------- DPR_ALGO_ATOMIC forward
// CB: compile-time bound of C (4 or kMaxChannels), the weights in registers, `c < C` guards (uniform).
template <typename T, int NI, int NO, int CB>
__global__ __launch_bounds__(kSmBlock) void k_smooth_ch_fwd_atomic(GridDesc<NO> gd, int64_t P, int64_t B, int C,
                                                                   T* __restrict__ out,
                                                                   const T* __restrict__ points,
                                                                   const T* __restrict__ rot,
                                                                   const T* __restrict__ trans,
                                                                   const T* __restrict__ ow,
                                                                   const T* __restrict__ pw) {
    static_assert(NO == 2 || NO == 3, "the smooth splat is written for 2-D and 3-D grids");
    const int64_t p = (int64_t)blockIdx.x * kSmBlock + threadIdx.x;
    if (p >= P) return;
    T pt[NI];
    load_point<T, NI>(points, p, pt);
    T pwc[CB];
    load_smooth_channel_weights<T, CB>(pw, p, C, 0, pwc);
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        const Pose<T, NI, NO> ps = load_pose<T, NI, NO>(rot, trans, ow, b);
        int j0[NO];
        T u[NO];
        if (!smooth_cell<T, NI, NO>(pt, ps, gd, j0, u)) continue;
        const SmoothAxes<T, NO> ax = smooth_axes<T, NO>(j0, u, gd);
        T w[CB];
#pragma unroll
        for (int c = 0; c < CB; ++c) w[c] = ps.ow * pwc[c];
        T* o = out + b * C * gd.G;
#pragma unroll
        for (int k2 = 0; k2 < (NO == 3 ? 3 : 1); ++k2) {
            const bool in2 = NO == 3 ? ax.in[NO - 1][k2] : true;
            const int off2 = NO == 3 ? ax.off[NO - 1][k2] : 0;
#pragma unroll
            for (int k1 = 0; k1 < 3; ++k1) {
                const T w12 = NO == 3 ? ax.w[1][k1] * ax.w[NO - 1][k2] : ax.w[1][k1];
#pragma unroll
                for (int k0 = 0; k0 < 3; ++k0) {
                    if (!(in2 && ax.in[1][k1] && ax.in[0][k0])) continue;
                    const T v = ax.w[0][k0] * w12;
                    T* cell = o + (off2 + ax.off[1][k1] + ax.off[0][k0]);
#pragma unroll
                    for (int c = 0; c < CB; ++c)
                        if (c < C) atomic_add<T>(cell + (int64_t)c * gd.G, v * w[c]);
                }
            }
        }
    }
}

// ---------------------------------------------------------------- DPR_ALGO_TILED forward
// Workgroup (tile, chunk) = (blockIdx.x, blockIdx.y): k_smooth_tile's walk over the tile's run of the sorted points,
// its clamped-centre rule and its flush, for channels c0 = chunk * CB .. min(C, c0 + CB) - 1, each with an LDS array
// of its own.  The point, its cell and the 3^N weight products are formed once per point; a channel costs one
// multiplication and one ds_add_f64 per cell.
template <typename T, int NI, int NO, int CB>
__global__ __launch_bounds__(kSmBlock) void k_smooth_ch_tile(GridDesc<NO> gd, SmoothTiles<NO> tl, int64_t P,
                                                             int64_t b, int C, T* __restrict__ out,
                                                             const T* __restrict__ points,
                                                             const T* __restrict__ rot, const T* __restrict__ trans,
                                                             const T* __restrict__ ow, const T* __restrict__ pw,
                                                             const uint32_t* __restrict__ start,
                                                             const uint32_t* __restrict__ idx) {
    static_assert(NO == 2 || NO == 3, "the smooth splat is written for 2-D and 3-D grids");
    constexpr int NC = smooth_lds_cells<NO>();
    static_assert(sizeof(double) * CB * NC <= 64 * 1024, "static LDS of a workgroup");
    __shared__ double cells[CB][NC];
    // the tile's run of the sorted points, clamped: a damaged table can shorten a walk, never leave idx[0 .. P)
    uint32_t begin, end;
    ord_cell_range(start, blockIdx.x, (uint32_t)P, begin, end);
    if (begin >= end) return;  // (uniform: an empty tile adds nothing)
    const int c0 = (int)blockIdx.y * CB;
    const int nc = C - c0 < CB ? C - c0 : CB;  // (>= 1: the launch has ceil(C / CB) chunks)
    int org[NO];                               // first cell of the tile
    {
        uint32_t t = blockIdx.x;
#pragma unroll
        for (int d = 0; d < NO; ++d) {
            org[d] = (int)(t % (uint32_t)tl.nt[d]) * SmoothTileShape<NO>::e[d];
            t /= (uint32_t)tl.nt[d];
        }
    }
#pragma unroll
    for (int c = 0; c < CB; ++c)
        if (c < nc)
            for (int i = threadIdx.x; i < NC; i += kSmBlock) cells[c][i] = 0.0;
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
        T w[CB];
        load_smooth_channel_weights<T, CB>(pw, (int64_t)p, C, c0, w);
#pragma unroll
        for (int c = 0; c < CB; ++c) w[c] = ps.ow * w[c];
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
                const int cc = j0[d] + k - 1, l = cc - org[d] + 1;
                in[d][k] = cc >= 0 && cc < gd.n[d] && l >= 0 && l < SmoothTileShape<NO>::e[d] + 2;
                loff[d][k] = in[d][k] ? l * lstride : 0;
            }
            lstride *= SmoothTileShape<NO>::e[d] + 2;
        }
#pragma unroll
        for (int k2 = 0; k2 < (NO == 3 ? 3 : 1); ++k2) {
            const bool in2 = NO == 3 ? in[NO - 1][k2] : true;
            const int off2 = NO == 3 ? loff[NO - 1][k2] : 0;
#pragma unroll
            for (int k1 = 0; k1 < 3; ++k1) {
                const T w12 = NO == 3 ? wt[1][k1] * wt[NO - 1][k2] : wt[1][k1];
#pragma unroll
                for (int k0 = 0; k0 < 3; ++k0) {
                    if (!(in2 && in[1][k1] && in[0][k0])) continue;
                    const T v = wt[0][k0] * w12;
                    const int l = off2 + loff[1][k1] + loff[0][k0];
#pragma unroll
                    for (int c = 0; c < CB; ++c)
                        if (c < nc) atomicAdd(&cells[c][l], (double)(v * w[c]));
                }
            }
        }
    }
    __syncthreads();

    // flush: consecutive threads walk axis 0 of the tile + halo, so a wave's atomics cover rows of a plane
    T* o = out + (b * C + c0) * gd.G;
    for (int i = threadIdx.x; i < NC; i += kSmBlock) {
        int rest = i, off = 0, stride = 1;
        bool in_grid = true;
#pragma unroll
        for (int d = 0; d < NO; ++d) {
            const int ext = SmoothTileShape<NO>::e[d] + 2;
            const int cc = org[d] + (rest % ext) - 1;
            rest /= ext;
            in_grid = in_grid && cc >= 0 && cc < gd.n[d];
            off += in_grid ? cc * stride : 0;
            stride *= gd.n[d];
        }
        if (!in_grid) continue;
#pragma unroll
        for (int c = 0; c < CB; ++c) {
            if (c < nc) {
                const double v = cells[c][i];
                if (v != 0.0) atomic_add<T>(o + (int64_t)c * gd.G + off, (T)v);
            }
        }
    }
}

// ---------------------------------------------------------------- DPR_ALGO_ATOMIC pullback
// (the point term of a channel, smooth_point_backward_axes: dpr_smooth_device.h)
// CB: compile-time bound of C (4 or kMaxChannels): the channel weights and the ds_dpoint_weight accumulators live in
// registers.  Pre-zeroed: ds_drotation, ds_dtranslation, ds_dout_weight; with accumulate_points also ds_dpoints and
// ds_dpoint_weight (the poses are cut into slices on grid.y, every slice adds its share with atomics).
template <typename T, int NI, int NO, int CB>
__global__ __launch_bounds__(kSmBlock) void k_smooth_ch_bwd(
    GridDesc<NO> gd, int64_t P, int64_t B, int C, const T* __restrict__ g, const T* __restrict__ points,
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
    T pwc[CB];
#pragma unroll
    for (int c = 0; c < CB; ++c) pwc[c] = T(0);
    if (live) {
        load_point<T, NI>(points, p, pt);
        load_smooth_channel_weights<T, CB>(pw, p, C, 0, pwc);
    }

    T acc_pt[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) acc_pt[j] = T(0);
    T acc_pw[CB];
#pragma unroll
    for (int c = 0; c < CB; ++c) acc_pw[c] = T(0);

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
            const SmoothAxes<T, NO> ax = smooth_axes<T, NO>(j0, u, gd);
            T dw[NO][3];
#pragma unroll
            for (int d = 0; d < NO; ++d) spline_derivatives<T>(u[d], dw[d]);
            const T* gb = g + b * C * gd.G;
            T dsum[NO], wsum = T(0);  // sum_c pw[p, c] * dcoord_c, sum_c W_c * pw[p, c]
#pragma unroll
            for (int n = 0; n < NO; ++n) dsum[n] = T(0);
#pragma unroll
            for (int c = 0; c < CB; ++c) {
                if (c < C) {  // (uniform)
                    const T* gc = gb + (int64_t)c * gd.G;
                    T dcoord[NO], W;
                    smooth_point_backward_axes<T, NO>(ax, dw, [&](int off) { return gc[off]; }, dcoord, W);
#pragma unroll
                    for (int n = 0; n < NO; ++n) dsum[n] += dcoord[n] * pwc[c];
                    wsum += W * pwc[c];
                    acc_pw[c] += W * ps.ow;
                }
            }
            T scaled[NO];
#pragma unroll
            for (int n = 0; n < NO; ++n) scaled[n] = (dsum[n] * ps.ow) * (T(gd.n[n]) / T(2));
#pragma unroll
            for (int n = 0; n < NO; ++n) {
#pragma unroll
                for (int j = 0; j < NI; ++j) vals[n + j * NO] = scaled[n] * pt[j];
                vals[NO * NI + n] = scaled[n];
            }
            vals[NO * NI + NO] = wsum;
#pragma unroll
            for (int j = 0; j < NI; ++j) {  // rotation' * scaled
                T v = ps.R[0 + j * NO] * scaled[0];
#pragma unroll
                for (int n = 1; n < NO; ++n) v = v + ps.R[n + j * NO] * scaled[n];
                acc_pt[j] += v;
            }
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
        T* dp = ds_dpoints + p * NI;
        T* dq = ds_dpoint_weight ? ds_dpoint_weight + p * C : nullptr;
        if (accumulate_points) {
#pragma unroll
            for (int j = 0; j < NI; ++j) atomic_add<T>(dp + j, acc_pt[j]);
            if (dq) {
#pragma unroll
                for (int c = 0; c < CB; ++c)
                    if (c < C) atomic_add<T>(dq + c, acc_pw[c]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < NI; ++j) dp[j] = acc_pt[j];
            if (dq) {
#pragma unroll
                for (int c = 0; c < CB; ++c)
                    if (c < C) dq[c] = acc_pw[c];
            }
        }
    }
}

// ---------------------------------------------------------------- host
template <typename T, int NI, int NO>
int smooth_channels_fwd_atomic(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int C, T* out,
                               const T* points, const T* rot, const T* trans, const T* ow, const T* pw) {
    if (P <= 0 || B <= 0) return DPR_OK;
    const GridDesc<NO> gd = make_grid_desc<NO>(grid, G);
    dim3 g((unsigned)((P + kSmBlock - 1) / kSmBlock), (unsigned)(B < 65535 ? B : 65535));
    if (C <= 4)
        hipLaunchKernelGGL((k_smooth_ch_fwd_atomic<T, NI, NO, 4>), g, dim3(kSmBlock), 0, st, gd, P, B, C, out, points,
                           rot, trans, ow, pw);
    else
        hipLaunchKernelGGL((k_smooth_ch_fwd_atomic<T, NI, NO, kMaxChannels>), g, dim3(kSmBlock), 0, st, gd, P, B, C,
                           out, points, rot, trans, ow, pw);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

// per pose: the binning of smooth_fwd_tiled, then ONE launch over (tiles, chunks): a binning serves all C channels
template <typename T, int NI, int NO>
int smooth_channels_fwd_tiled(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int C, T* out,
                              const T* points, const T* rot, const T* trans, const T* ow, const T* pw, void* ws,
                              size_t ws_bytes) {
    if (P <= 0 || B <= 0) return DPR_OK;
    SmoothBinning<NO> sb;
    if (int rc = smooth_binning<NO>(grid, G, P, B, 1, ws, ws_bytes, &sb)) return rc;
    const dim3 tgrid((unsigned)sb.tiles, (unsigned)((C + kSmChTile - 1) / kSmChTile));  // (y <= kMaxChannels)
    for (int64_t b = 0; b < B; ++b) {
        if (int rc = smooth_bin_pose<T, NI, NO>(st, sb, P, b, points, rot, trans)) return rc;
        hipLaunchKernelGGL((k_smooth_ch_tile<T, NI, NO, kSmChTile>), tgrid, dim3(kSmBlock), 0, st, sb.gd, sb.tl, P, b,
                           C, out, points, rot, trans, ow, pw, (const uint32_t*)sb.start,
                           (const uint32_t*)sb.idx_out);
        stage_mark(st);
    }
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

template <typename T, int NI, int NO>
int smooth_channels_bwd_atomic(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int C, const T* g,
                               const T* points, const T* rot, const T* trans, const T* ow, const T* pw, T* d_pts,
                               T* d_rot, T* d_trans, T* d_ow, T* d_pw, int poses_per_slice, int64_t slices) {
    if (P <= 0 || B <= 0) return DPR_OK;
    const GridDesc<NO> gd = make_grid_desc<NO>(grid, G);
    const int accumulate = slices > 1;
    if (accumulate) {
        DPR_HIP(zero_async(st, d_pts, sizeof(T) * (size_t)(P * NI)));
        if (d_pw) DPR_HIP(zero_async(st, d_pw, sizeof(T) * (size_t)(P * C)));
    }
    dim3 gg((unsigned)((P + kSmBlock - 1) / kSmBlock), (unsigned)slices);
    if (C <= 4)
        hipLaunchKernelGGL((k_smooth_ch_bwd<T, NI, NO, 4>), gg, dim3(kSmBlock), 0, st, gd, P, B, C, g, points, rot,
                           trans, ow, pw, d_pts, d_rot, d_trans, d_ow, d_pw, poses_per_slice, accumulate);
    else
        hipLaunchKernelGGL((k_smooth_ch_bwd<T, NI, NO, kMaxChannels>), gg, dim3(kSmBlock), 0, st, gd, P, B, C, g,
                           points, rot, trans, ow, pw, d_pts, d_rot, d_trans, d_ow, d_pw, poses_per_slice,
                           accumulate);
    stage_mark(st);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

#define DPR_SMOOTH_CHANNELS_INSTANTIATE(T, NI, NO)                                                                  \
    template int smooth_channels_fwd_atomic<T, NI, NO>(hipStream_t, const int64_t*, int64_t, int64_t, int64_t, int, \
                                                       T*, const T*, const T*, const T*, const T*, const T*);      \
    template int smooth_channels_fwd_tiled<T, NI, NO>(hipStream_t, const int64_t*, int64_t, int64_t, int64_t, int,  \
                                                      T*, const T*, const T*, const T*, const T*, const T*, void*, \
                                                      size_t);                                                     \
    template int smooth_channels_bwd_atomic<T, NI, NO>(hipStream_t, const int64_t*, int64_t, int64_t, int64_t, int, \
                                                       const T*, const T*, const T*, const T*, const T*, const T*, \
                                                       T*, T*, T*, T*, T*, int, int64_t);
#define DPR_SMOOTH_CHANNELS_INSTANTIATE_T(T)                                           \
    DPR_SMOOTH_CHANNELS_INSTANTIATE(T, 2, 2) DPR_SMOOTH_CHANNELS_INSTANTIATE(T, 3, 3) \
    DPR_SMOOTH_CHANNELS_INSTANTIATE(T, 3, 2)
DPR_SMOOTH_CHANNELS_INSTANTIATE_T(float)
DPR_SMOOTH_CHANNELS_INSTANTIATE_T(double)

}  // namespace dpr
