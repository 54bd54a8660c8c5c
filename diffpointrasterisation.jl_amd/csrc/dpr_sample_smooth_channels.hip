// Smooth sampling of C-channel images (include/dpr.h, "SMOOTH SAMPLING, MULTI-CHANNEL"): the image
// dpr_raster_smooth_channels_ex_* writes, read back at the points.  The cell, the B-spline weights and the offsets of
// a (point, pose) are formed once and serve all C planes.
//
//   image / ds_dimage     (n_1, .., n_N, C, B): plane (c, b) at (b * C + c) * G
//   values / ds_dvalues   a point's C values contiguous, pose slowest: (b * P + p) * C + c -- column b is a
//                         point_weight of the smooth channel splat
//
//   forward    k_sample_smooth_ch_fwd: k_sample_smooth_fwd's shape (a thread per point, the pose slice loop inside);
//              a run-time loop over the channels in groups of four planes, whose gathers are independent, then one
//              plane at a time; no atomics.  values[:, c, b] has the bits of k_sample_smooth_fwd on plane (c, b):
//              smooth_point_backward_axes forms smooth_point_backward's sums operation for operation
//   pullback   k_sample_smooth_ch_bwd: k_sample_smooth_bwd's shape and tail; a channel loop with C atomics per accepted
//              cell (ds_dimage, DPR_ALGO_ATOMIC), then a channel loop that adds dv_c * dcoord_c into N_out running
//              sums -- two loops, so that the weight products of the first and the gathers of the second are not live
//              together; no per-channel accumulator lives across either, so there is no compile-time bound on C
//   DPR_ALGO_TILED pullback: this kernel without ds_dimage; dpr_api_smooth.hip then runs smooth_channels_fwd_tiled
//              (dpr_smooth_channels.hip) pose by pose with column b of ds_dvalues as the point weights
#include <hip/hip_runtime.h>

#include "../../include/dpr.h"
#include "dpr_smooth.h"
#include "dpr_smooth_device.h"

namespace dpr {

// The base of a plane, which is the same in every lane, as a scalar pair the optimiser cannot see through.  Without
// it the channel loops keep one 64-bit address per (cell, plane in flight) as an induction variable: 3-D, 27 x 4 x 2
// VGPRs in the forward.  With it a loop keeps the 3^N 32-bit offsets and adds the base at the gather.
template <typename T> __device__ __forceinline__ T* uniform_ptr(T* q) {
    const uint64_t a = (uint64_t)q;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    return (T*)(((uint64_t)hi << 32) | lo);
}

// ---------------------------------------------------------------- forward
// vec4: C % 4 == 0, T = float and `values` 16-byte aligned -- a group of four values leaves as one 16-byte store
// (element (b * P + p) * C + c0 with c0 % 4 == 0 is then 16-byte aligned).  A rejected point stores C zeros.
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kSmBlock) void k_sample_smooth_ch_fwd(GridDesc<NO> gd, int64_t P, int64_t B, int C,
                                                                   T* __restrict__ values,
                                                                   const T* __restrict__ image,
                                                                   const T* __restrict__ points,
                                                                   const T* __restrict__ rot,
                                                                   const T* __restrict__ trans, int poses_per_slice,
                                                                   int vec4) {
    static_assert(NO == 2 || NO == 3, "the smooth splat is written for 2-D and 3-D grids");
    const int64_t p = (int64_t)blockIdx.x * kSmBlock + threadIdx.x;
    if (p >= P) return;
    T pt[NI];
    load_point<T, NI>(points, p, pt);
    const int64_t b_lo = (int64_t)blockIdx.y * poses_per_slice;
    const int64_t b_hi = (b_lo + poses_per_slice < B) ? b_lo + poses_per_slice : B;
    for (int64_t b = b_lo; b < b_hi; ++b) {
        const Pose<T, NI, NO> ps = load_pose<T, NI, NO>(rot, trans, nullptr, b);
        T* v = values + (b * P + p) * C;
        int j0[NO];
        T u[NO];
        if (!smooth_cell<T, NI, NO>(pt, ps, gd, j0, u)) {
            for (int c = 0; c < C; ++c) v[c] = T(0);
            continue;
        }
        const SmoothAxes<T, NO> ax = smooth_axes<T, NO>(j0, u, gd);
        T dw[NO][3];  // (only W is kept; the compiler drops the derivative sums)
#pragma unroll
        for (int d = 0; d < NO; ++d) spline_derivatives<T>(u[d], dw[d]);
        const T* img = image + b * C * gd.G;
        int c = 0;
        for (; c + 4 <= C; c += 4) {
            T w4[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const T* plane = uniform_ptr(img + (int64_t)(c + i) * gd.G);
                T dcoord[NO];
                smooth_point_backward_axes<T, NO>(ax, dw, [&](int off) { return plane[off]; }, dcoord, w4[i]);
            }
            if constexpr (std::is_same<T, float>::value) {
                if (vec4) {  // (uniform)
                    *reinterpret_cast<float4*>(v + c) = make_float4(w4[0], w4[1], w4[2], w4[3]);
                    continue;
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) v[c + i] = w4[i];
        }
        for (; c < C; ++c) {
            const T* plane = uniform_ptr(img + (int64_t)c * gd.G);
            T dcoord[NO], W;
            smooth_point_backward_axes<T, NO>(ax, dw, [&](int off) { return plane[off]; }, dcoord, W);
            v[c] = W;
        }
    }
}

// ---------------------------------------------------------------- pullback
// Over the pose range of the slice, with dv_c = ds_dvalues[p, c, b]:
//   ds_dimage[.., c, b] += dv_c * prod_d w_d(s_d)   (k_smooth_ch_fwd_atomic's contribution for point weight dv_c and
//                                                    out_weight 1), when non-NULL
//   ds_dpoints, ds_drotation, ds_dtranslation: k_sample_smooth_bwd's terms of the C planes, summed over c before the
//                                              scale: dsum_n = sum_c dv_c * dcoord_c[n]
// Any output may be NULL (uniform branches; the image is read only for the three geometric gradients).  Pre-zeroed:
// ds_drotation, ds_dtranslation, ds_dimage; ds_dpoints is stored (accumulate_points == 0) or added atomically onto
// a zeroed buffer.
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kSmBlock) void k_sample_smooth_ch_bwd(
    GridDesc<NO> gd, int64_t P, int64_t B, int C, const T* __restrict__ ds_dvalues, const T* __restrict__ image,
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
            const SmoothAxes<T, NO> ax = smooth_axes<T, NO>(j0, u, gd);
            T dw[NO][3];
#pragma unroll
            for (int d = 0; d < NO; ++d) spline_derivatives<T>(u[d], dw[d]);
            const T* dv = ds_dvalues + (b * P + p) * C;
            T dsum[NO];  // sum_c dv_c * dcoord_c
#pragma unroll
            for (int n = 0; n < NO; ++n) dsum[n] = T(0);
            if (ds_dimage) {
#pragma nounroll
                for (int c = 0; c < C; ++c) {
                    const T dvc = dv[c];
                    T* o = uniform_ptr(ds_dimage + (b * C + c) * gd.G);
#pragma unroll
                    for (int k2 = 0; k2 < (NO == 3 ? 3 : 1); ++k2) {
                        const bool in2 = NO == 3 ? ax.in[NO - 1][k2] : true;
                        const int off2 = NO == 3 ? ax.off[NO - 1][k2] : 0;
#pragma unroll
                        for (int k1 = 0; k1 < 3; ++k1) {
                            const T w12 = NO == 3 ? ax.w[1][k1] * ax.w[NO - 1][k2] : ax.w[1][k1];
#pragma unroll
                            for (int k0 = 0; k0 < 3; ++k0)
                                if (in2 && ax.in[1][k1] && ax.in[0][k0])
                                    atomic_add<T>(o + (off2 + ax.off[1][k1] + ax.off[0][k0]),
                                                  (ax.w[0][k0] * w12) * dvc);
                        }
                    }
                }
            }
            if (geom) {
#pragma nounroll
                for (int c = 0; c < C; ++c) {
                    const T dvc = dv[c];
                    const T* img = uniform_ptr(image + (b * C + c) * gd.G);
                    T dcoord[NO], W;
                    smooth_point_backward_axes<T, NO>(ax, dw, [&](int off) { return img[off]; }, dcoord, W);
#pragma unroll
                    for (int n = 0; n < NO; ++n) dsum[n] += dcoord[n] * dvc;
                }
            }
            if (geom) {
                T scaled[NO];
#pragma unroll
                for (int n = 0; n < NO; ++n) scaled[n] = dsum[n] * (T(gd.n[n]) / T(2));
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

// ---------------------------------------------------------------- host
template <typename T, int NI, int NO>
int sample_smooth_channels_fwd(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int C, T* values,
                               const T* image, const T* points, const T* rot, const T* trans, int poses_per_slice,
                               int64_t slices) {
    if (P <= 0 || B <= 0) return DPR_OK;
    const GridDesc<NO> gd = make_grid_desc<NO>(grid, G);
    const int vec4 = std::is_same<T, float>::value && C % 4 == 0 && ((uintptr_t)values & 15) == 0;
    dim3 gg((unsigned)((P + kSmBlock - 1) / kSmBlock), (unsigned)slices);
    hipLaunchKernelGGL((k_sample_smooth_ch_fwd<T, NI, NO>), gg, dim3(kSmBlock), 0, st, gd, P, B, C, values, image,
                       points, rot, trans, poses_per_slice, vec4);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

template <typename T, int NI, int NO>
int sample_smooth_channels_bwd(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int C,
                               const T* dv, const T* image, const T* points, const T* rot, const T* trans, T* d_img,
                               T* d_pts, T* d_rot, T* d_trans, int poses_per_slice, int64_t slices) {
    if (P <= 0 || B <= 0 || !(d_img || d_pts || d_rot || d_trans)) return DPR_OK;
    const GridDesc<NO> gd = make_grid_desc<NO>(grid, G);
    const int accumulate = slices > 1;
    if (accumulate && d_pts) DPR_HIP(zero_async(st, d_pts, sizeof(T) * (size_t)(P * NI)));
    dim3 gg((unsigned)((P + kSmBlock - 1) / kSmBlock), (unsigned)slices);
    hipLaunchKernelGGL((k_sample_smooth_ch_bwd<T, NI, NO>), gg, dim3(kSmBlock), 0, st, gd, P, B, C, dv, image, points,
                       rot, trans, d_img, d_pts, d_rot, d_trans, poses_per_slice, accumulate);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

#define DPR_SAMPLE_SMOOTH_CHANNELS_INSTANTIATE(T, NI, NO)                                                           \
    template int sample_smooth_channels_fwd<T, NI, NO>(hipStream_t, const int64_t*, int64_t, int64_t, int64_t, int, \
                                                       T*, const T*, const T*, const T*, const T*, int, int64_t);  \
    template int sample_smooth_channels_bwd<T, NI, NO>(hipStream_t, const int64_t*, int64_t, int64_t, int64_t, int, \
                                                       const T*, const T*, const T*, const T*, const T*, T*, T*,   \
                                                       T*, T*, int, int64_t);
#define DPR_SAMPLE_SMOOTH_CHANNELS_INSTANTIATE_T(T)                                                  \
    DPR_SAMPLE_SMOOTH_CHANNELS_INSTANTIATE(T, 2, 2) DPR_SAMPLE_SMOOTH_CHANNELS_INSTANTIATE(T, 3, 3) \
    DPR_SAMPLE_SMOOTH_CHANNELS_INSTANTIATE(T, 3, 2)
DPR_SAMPLE_SMOOTH_CHANNELS_INSTANTIATE_T(float)
DPR_SAMPLE_SMOOTH_CHANNELS_INSTANTIATE_T(double)

}  // namespace dpr
