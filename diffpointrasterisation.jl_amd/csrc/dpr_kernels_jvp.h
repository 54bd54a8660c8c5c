// DPR_ALGO_ATOMIC forward-mode derivative of raster (dpr_raster_jvp_ex_*), every (n_in, n_out):
//   out_dot  (n_1, .., n_N, K, B): plane (b, k) at offset (b * K + k) * G -- the channel layout with C = K
// k_jvp_fill writes the background tangent (or 0) into every plane first; k_jvp_atomic then adds the deposits of
// dpr_jvp.h with global float atomics.
#pragma once
#include "dpr_jvp.h"
#include "dpr_kernels_atomic.h"

namespace dpr {

// plane q = b * K + k of out_dot := bg_dot[k * B + b] (0 without bg_dot); planes [q0, q0 + gridDim.y)
template <typename T>
__global__ __launch_bounds__(kBlock) void k_jvp_fill(T* __restrict__ out, int64_t G, int K, int64_t B, int64_t q0,
                                                     const T* __restrict__ bg_dot) {
    const int64_t q = q0 + blockIdx.y;
    const int64_t b = q / K, k = q % K;
    const T v = bg_dot ? bg_dot[k * B + b] : T(0);
    T* o = out + q * G;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < G; i += (int64_t)gridDim.x * kBlock)
        o[i] = v;
}

// One thread per point over the pose range [b_lo, b_hi) (k_bwd_gather's slicing).  The cell, the deltas, the
// 2^N voxel weights and the N * 2^N interpolation weights of a (point, pose) are computed once; the K tangents
// are a run-time loop of 2^N atomics each.  A rejected point reads none of its tangents and adds nothing.
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kBlock) void k_jvp_atomic(GridDesc<NO> gd, int64_t P, int64_t B, int K,
                                                       T* __restrict__ out_dot, const T* __restrict__ points,
                                                       const T* __restrict__ rot, const T* __restrict__ trans,
                                                       const T* __restrict__ ow, const T* __restrict__ pw,
                                                       JvpTangents<T> tan, int poses_per_slice) {
    constexpr int S = 1 << NO;
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= P) return;
    T pt[NI];
    load_point<T, NI>(points, p, pt);
    const T pwv = pw ? pw[p] : T(1);
    const int64_t b_lo = (int64_t)blockIdx.y * poses_per_slice;
    const int64_t b_hi = (b_lo + poses_per_slice < B) ? b_lo + poses_per_slice : B;
    for (int64_t b = b_lo; b < b_hi; ++b) {
        const Pose<T, NI, NO> ps = load_pose<T, NI, NO>(rot, trans, ow, b);
        int ref0[NO];
        T dlo[NO];
        if (!ref_and_deltas<T, NI, NO>(pt, ps, gd, ref0, dlo)) continue;
        int off[S];
        T vw[S], iw[S][NO];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            off[s] = nbr_offset<NO>(ref0, s, gd);
            vw[s] = voxel_weight<T, NO>(dlo, s, T(1));
#pragma unroll
            for (int n = 0; n < NO; ++n) iw[s][n] = interp_weight<T, NO>(n, dlo, s);
        }
        T* o = out_dot + b * K * gd.G;
        for (int k = 0; k < K; ++k) {
            const JvpPose<T, NI, NO> tp = load_jvp_pose<T, NI, NO>(tan.rot, tan.trans, tan.ow, (int64_t)k * B + b);
            T pd[NI], pwd;
            load_jvp_point<T, NI>(tan.points, tan.pw, (int64_t)k * P + p, pd, pwd);
            T a, bc[NO];
            jvp_coeffs<T, NI, NO>(pt, pwv, pd, pwd, ps, tp, gd, a, bc);
            T* ok = o + (int64_t)k * gd.G;
#pragma unroll
            for (int s = 0; s < S; ++s)
                if (off[s] >= 0) atomic_add<T>(ok + off[s], jvp_deposit_pre<T, NO>(a, bc, vw[s], iw[s]));
        }
    }
}

}  // namespace dpr
