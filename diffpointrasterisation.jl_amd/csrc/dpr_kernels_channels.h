// DPR_ALGO_ATOMIC for C weight channels per point (dpr_raster_channels_ex_*,
// dpr_raster_pullback_channels_ex_*): the geometry of a (point, pose) -- cell choice, deltas,
// the 2^N_out voxel weights -- is computed ONCE and serves all C channels.
//   out / ds_dout       (n_1, .., n_N, C, B): plane (b, c) at offset (b * C + c) * G
//   point_weight        C x P (channel fastest), ds_dpoint_weight likewise
//   background          C x B, ds_dbackground likewise -- so plane k = b * C + c pairs with
//                       background[k], and k_fill_background / k_grid_sum serve B * C planes as is
// Channel c of every output is the single-channel result for point_weight[c, :] (the per-pose
// sums and ds_dpoints: summed over c).  CB = compile-time channel bound (C <= CB): the per-channel
// weights and accumulators live in registers, unrolled over CB with `c < C` guards.
#pragma once
#include "dpr_kernels_atomic.h"

namespace dpr {

// the point's C weights (1 for the default) as one vector in registers
template <typename T, int CB>
__device__ __forceinline__ void load_channel_weights(const T* __restrict__ pw, int64_t p, int C,
                                                     T (&w)[CB]) {
#pragma unroll
    for (int c = 0; c < CB; ++c) w[c] = (pw && c < C) ? pw[p * C + c] : T(1);
}

// prod_d deltas of neighbour s: voxel_weight() without its final `* w`, so that
// voxel_prod(dlo, s) * w == voxel_weight(dlo, s, w) bit for bit
template <typename T, int NO>
__device__ __forceinline__ T voxel_prod(const T (&dlo)[NO], int s) {
    T v = (s & 1) ? dlo[0] : (T(1) - dlo[0]);
#pragma unroll
    for (int d = 1; d < NO; ++d) v = v * (((s >> d) & 1) ? dlo[d] : (T(1) - dlo[d]));
    return v;
}

// Forward: one thread per (point, pose), 2^N_out x C global float atomics.  Every contribution
// is the single-channel kernel's value for that channel's weight (same operation order).
template <typename T, int NI, int NO, int CB>
__global__ __launch_bounds__(kBlock) void k_fwd_atomic_ch(GridDesc<NO> gd, int64_t P, int64_t B, int C,
                                                          T* __restrict__ out,
                                                          const T* __restrict__ points,
                                                          const T* __restrict__ rot,
                                                          const T* __restrict__ trans,
                                                          const T* __restrict__ ow,
                                                          const T* __restrict__ pw) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= P) return;
    T pt[NI];
    load_point<T, NI>(points, p, pt);
    T pwc[CB];
    load_channel_weights<T, CB>(pw, p, C, pwc);
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        const Pose<T, NI, NO> ps = load_pose<T, NI, NO>(rot, trans, ow, b);
        int ref0[NO];
        T dlo[NO];
        if (!ref_and_deltas<T, NI, NO>(pt, ps, gd, ref0, dlo)) continue;
        T w[CB];
#pragma unroll
        for (int c = 0; c < CB; ++c) w[c] = ps.ow * pwc[c];  // src/raster.jl:52, per channel
        T* o = out + b * C * gd.G;
#pragma unroll
        for (int s = 0; s < (1 << NO); ++s) {
            const int off = nbr_offset<NO>(ref0, s, gd);
            if (off < 0) continue;
            const T v = voxel_prod<T, NO>(dlo, s);
#pragma unroll
            for (int c = 0; c < CB; ++c)
                if (c < C) atomic_add<T>(o + (int64_t)c * gd.G + off, v * w[c]);
        }
    }
}

// Pullback over the pose range [b_lo, b_hi), the shape of k_bwd_gather.  For every neighbour s the C
// planes of ds_dout are read once and folded into
//   sum_c g_c(s) * out_weight * point_weight[c]   -> ds_dpoints and the per-pose sums: one channel's
//                                                    work from here on (point_backward's arithmetic)
//   out_weight * voxel_weight(s) * g_c(s)          -> ds_dpoint_weight[c], per channel
// Every term keeps point_backward's operation order, so C = 1 computes exactly what k_bwd_gather does.
// Pre-zeroed: ds_drotation, ds_dtranslation, ds_dout_weight; ds_dpoints / ds_dpoint_weight are
// stored (accumulate_points == 0) or added atomically onto zeroed buffers.
template <typename T, int NI, int NO, int CB>
__global__ __launch_bounds__(kBlock) void k_bwd_gather_ch(
    GridDesc<NO> gd, int64_t P, int64_t B, int C, const T* __restrict__ g,
    const T* __restrict__ points, const T* __restrict__ rot, const T* __restrict__ trans,
    const T* __restrict__ ow, const T* __restrict__ pw, T* __restrict__ ds_dpoints,
    T* __restrict__ ds_drotation, T* __restrict__ ds_dtranslation, T* __restrict__ ds_dout_weight,
    T* __restrict__ ds_dpoint_weight, int poses_per_slice, int accumulate_points) {
    constexpr int NV = NO * NI + NO + 1;  // dR | dt | d out_weight
    constexpr int NW = kBlock / kWave;
    __shared__ T red[NW][NV];

    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = p < P;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    T pt[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) pt[j] = T(0);
    if (live) load_point<T, NI>(points, p, pt);
    T pwc[CB];
    load_channel_weights<T, CB>(live ? pw : nullptr, p, C, pwc);

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
        int ref0[NO];
        T dlo[NO];
        if (live && ref_and_deltas<T, NI, NO>(pt, ps, gd, ref0, dlo)) {
            const T* gb = g + b * C * gd.G;
            T dcoord[NO];
#pragma unroll
            for (int n = 0; n < NO; ++n) dcoord[n] = T(0);
            T dow_part = T(0);
            T dpw_pose[CB];
#pragma unroll
            for (int c = 0; c < CB; ++c) dpw_pose[c] = T(0);
#pragma unroll
            for (int s = 0; s < (1 << NO); ++s) {
                const int o = nbr_offset<NO>(ref0, s, gd);
                const bool in = o >= 0;
                const int64_t off = in ? o : 0;  // a dropped neighbour reads cell 0 and adds nothing
                T gc[CB];
#pragma unroll
                for (int c = 0; c < CB; ++c) gc[c] = (c < C) ? gb[(int64_t)c * gd.G + off] : T(0);
                const T vp = voxel_prod<T, NO>(dlo, s);
                // (each term in point_backward's operation order: C = 1 is the single-channel arithmetic)
                T dow_s = T(0), factor = T(0);
#pragma unroll
                for (int c = 0; c < CB; ++c) {
                    if (c < C) {
                        const T dweight = vp * gc[c];
                        dow_s += dweight * pwc[c];                 // :57
                        dpw_pose[c] += in ? dweight * ps.ow : T(0);  // :58
                        factor += gc[c] * ps.ow * pwc[c];
                    }
                }
                dow_part += in ? dow_s : T(0);
#pragma unroll
                for (int n = 0; n < NO; ++n)
                    dcoord[n] += in ? factor * interp_weight<T, NO>(n, dlo, s) : T(0);
            }
            T scaled[NO];
#pragma unroll
            for (int n = 0; n < NO; ++n) scaled[n] = dcoord[n] * (T(gd.n[n]) / T(2));
#pragma unroll
            for (int n = 0; n < NO; ++n) {
#pragma unroll
                for (int j = 0; j < NI; ++j) vals[n + j * NO] = scaled[n] * pt[j];  // :69
                vals[NO * NI + n] = scaled[n];                                      // :68
            }
            vals[NO * NI + NO] = dow_part;
#pragma unroll
            for (int c = 0; c < CB; ++c) acc_pw[c] += dpw_pose[c];
#pragma unroll
            for (int j = 0; j < NI; ++j) {  // rotation' * scaled  (:70)
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
        if (accumulate_points) {
#pragma unroll
            for (int j = 0; j < NI; ++j) atomic_add<T>(ds_dpoints + p * NI + j, acc_pt[j]);
            if (ds_dpoint_weight) {
#pragma unroll
                for (int c = 0; c < CB; ++c)
                    if (c < C) atomic_add<T>(ds_dpoint_weight + p * C + c, acc_pw[c]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < NI; ++j) ds_dpoints[p * NI + j] = acc_pt[j];
            if (ds_dpoint_weight) {
#pragma unroll
                for (int c = 0; c < CB; ++c)
                    if (c < C) ds_dpoint_weight[p * C + c] = acc_pw[c];
            }
        }
    }
}

}  // namespace dpr
