// Point sampling (dpr_sample_ex_*, dpr_sample_pullback_ex_*): N-linear interpolation of an image at the
// transformed points, the transpose of `raster` with respect to the point weights.
//   values[p, b] = sum_s in-grid voxel_weight(deltas(R_b p + t_b), s) * image[ref(p, b) + shift_s, b]
// which is point_backward's ds_dpoint_weight term with ds_dout = image, out_weight = 1 and point_weight = 1.
//   values, ds_dvalues   P x B, point index fastest: pose b is the contiguous column at b * P
//   image, ds_dimage     (n_1, .., n_N, B) column-major, as `out` of dpr_raster_ex_*
// Both kernels hold a point in registers and loop over a slice of the poses (k_bwd_gather's shape); every term
// comes from the shared helpers of dpr_device.h in their order, so the forward is bit-identical to the
// ds_dpoint_weight of k_bwd_gather for those arguments.
#pragma once
#include "dpr_kernels_atomic.h"

namespace dpr {

// Forward: one thread per point, all 2^N_out gathers issued before their first use (point_backward), the
// value stored with a plain coalesced store into column b.  A rejected point gives 0.
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kBlock) void k_sample_fwd(GridDesc<NO> gd, int64_t P, int64_t B,
                                                       T* __restrict__ values, const T* __restrict__ image,
                                                       const T* __restrict__ points, const T* __restrict__ rot,
                                                       const T* __restrict__ trans, int poses_per_slice) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= P) return;
    T pt[NI];
    load_point<T, NI>(points, p, pt);
    const int64_t b_lo = (int64_t)blockIdx.y * poses_per_slice;
    const int64_t b_hi = (b_lo + poses_per_slice < B) ? b_lo + poses_per_slice : B;
    for (int64_t b = b_lo; b < b_hi; ++b) {
        const Pose<T, NI, NO> ps = load_pose<T, NI, NO>(rot, trans, nullptr, b);
        int ref0[NO];
        T dlo[NO];
        T v = T(0);
        if (ref_and_deltas<T, NI, NO>(pt, ps, gd, ref0, dlo)) {
            const T* img = image + b * gd.G;
            T scaled[NO], dow_part;
            // (only the ds_dpoint_weight term is kept; the compiler drops the others)
            point_backward<T, NI, NO>(ref0, dlo, gd, T(1), T(1), [&](int off) { return img[off]; }, scaled,
                                      dow_part, v);
        }
        values[b * P + p] = v;
    }
}

// Pullback over the pose range [b_lo, b_hi) for g = ds_dvalues[p, b]:
//   ds_dpoints, ds_drotation, ds_dtranslation: k_bwd_gather's terms with ds_dout = image_b, out_weight = 1 and
//                                              point_weight = g (point_backward)
//   ds_dimage[.., b] += voxel_weight(s, g)    (k_fwd_atomic's contribution for point weight g), when non-NULL
// Any output may be NULL.  Pre-zeroed: ds_drotation, ds_dtranslation, ds_dimage; ds_dpoints is stored
// (accumulate_points == 0) or added atomically onto a zeroed buffer.
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kBlock) void k_sample_bwd(
    GridDesc<NO> gd, int64_t P, int64_t B, const T* __restrict__ ds_dvalues, const T* __restrict__ image,
    const T* __restrict__ points, const T* __restrict__ rot, const T* __restrict__ trans,
    T* __restrict__ ds_dimage, T* __restrict__ ds_dpoints, T* __restrict__ ds_drotation,
    T* __restrict__ ds_dtranslation, int poses_per_slice, int accumulate_points) {
    constexpr int NV = NO * NI + NO;  // dR | dt
    constexpr int NW = kBlock / kWave;
    __shared__ T red[NW][NV];

    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = p < P;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    // (uniform: which gradients read the image, and whether the per-pose sums are wanted)
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
        int ref0[NO];
        T dlo[NO];
        if (live && ref_and_deltas<T, NI, NO>(pt, ps, gd, ref0, dlo)) {
            const T g = ds_dvalues[b * P + p];
            if (ds_dimage) {
                T* o = ds_dimage + b * gd.G;
#pragma unroll
                for (int s = 0; s < (1 << NO); ++s) {
                    const int off = nbr_offset<NO>(ref0, s, gd);
                    if (off >= 0) atomic_add<T>(o + off, voxel_weight<T, NO>(dlo, s, g));
                }
            }
            if (geom) {
                const T* img = image + b * gd.G;
                T scaled[NO], dow_part, dpw_part;
                point_backward<T, NI, NO>(ref0, dlo, gd, T(1), g, [&](int off) { return img[off]; }, scaled,
                                          dow_part, dpw_part);
#pragma unroll
                for (int n = 0; n < NO; ++n) {
#pragma unroll
                    for (int j = 0; j < NI; ++j) vals[n + j * NO] = scaled[n] * pt[j];  // raster_pullback.jl:69
                    vals[NO * NI + n] = scaled[n];                                      // :68
                }
#pragma unroll
                for (int j = 0; j < NI; ++j) {  // rotation' * scaled  (:70)
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

}  // namespace dpr
