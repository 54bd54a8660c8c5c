// Forward-mode derivative of raster (dpr_raster_jvp_ex_*): the per-(point, pose, tangent) arithmetic shared by
// the direct kernel (dpr_kernels_jvp.h) and the tiled path (dpr_tiled.hip).  For tangent k of pose b and point p
//   cdot_n    = n_n/2 * (sum_j Rdot[n, j] p_j + sum_j R[n, j] pdot_j + tdot[n])
//   a         = owdot * pw + ow * pwdot
//   b_n       = (ow * pw) * cdot_n
//   deposit_s = voxel_weight(dlo, s, a) + sum_n b_n * interp_weight(n, dlo, s)
// with ref0 held fixed: the one-sided derivative point_backward (dpr_device.h) differentiates, so the JVP is the
// exact transpose of the pullback.  |voxel_weight(dlo, s, 1)| <= 1 and |interp_weight| <= 1, hence
// |deposit_s| <= m = |a| + sum_n |b_n|: the bound the tiled path takes its fixed-point scale and range guard from.
#pragma once
#include "dpr_device.h"

namespace dpr {

constexpr int kMaxTangents = 16;  // tangents of one dpr_raster_jvp_ex_* call

// The tangents of one call; NULL = zero.  Each array holds K copies of its primal's layout (tangent k at
// k * primal size); ow / bg: K x B.
template <typename T> struct JvpTangents {
    const T* points;  // K x P x N_in
    const T* rot;     // K x B x (N_out x N_in, column-major)
    const T* trans;   // K x B x N_out
    const T* ow;      // K x B
    const T* pw;      // K x P
};

// tangent of one pose (wave-uniform addresses: scalar loads); zeros where the tangent is NULL, so that a NULL
// tangent and a zero one give the same bits
template <typename T, int NI, int NO> struct JvpPose {
    T Rd[NO * NI];
    T td[NO];
    T owd;
};
template <typename T, int NI, int NO>
__device__ __forceinline__ JvpPose<T, NI, NO> load_jvp_pose(const T* __restrict__ rot_dot,
                                                           const T* __restrict__ trans_dot,
                                                           const T* __restrict__ ow_dot, int64_t i) {
    JvpPose<T, NI, NO> tp;
#pragma unroll
    for (int k = 0; k < NO * NI; ++k) tp.Rd[k] = rot_dot ? rot_dot[i * (NO * NI) + k] : T(0);
#pragma unroll
    for (int d = 0; d < NO; ++d) tp.td[d] = trans_dot ? trans_dot[i * NO + d] : T(0);
    tp.owd = ow_dot ? ow_dot[i] : T(0);
    return tp;
}

// the point's tangent (zeros where NULL)
template <typename T, int NI>
__device__ __forceinline__ void load_jvp_point(const T* __restrict__ pts_dot, const T* __restrict__ pw_dot,
                                               int64_t i, T (&pd)[NI], T& pwd) {
#pragma unroll
    for (int j = 0; j < NI; ++j) pd[j] = pts_dot ? pts_dot[i * NI + j] : T(0);
    pwd = pw_dot ? pw_dot[i] : T(0);
}

// a and b_n of one (point, pose, tangent); pwv = the primal point weight (1 for the default)
template <typename T, int NI, int NO>
__device__ __forceinline__ void jvp_coeffs(const T (&pt)[NI], T pwv, const T (&pd)[NI], T pwd,
                                           const Pose<T, NI, NO>& ps, const JvpPose<T, NI, NO>& tp,
                                           const GridDesc<NO>& gd, T& a, T (&bc)[NO]) {
    const T w = ps.ow * pwv;  // src/raster.jl:52
    a = tp.owd * pwv + ps.ow * pwd;
#pragma unroll
    for (int n = 0; n < NO; ++n) {
        T u = tp.Rd[n] * pt[0];
#pragma unroll
        for (int j = 1; j < NI; ++j) u = u + tp.Rd[n + j * NO] * pt[j];
#pragma unroll
        for (int j = 0; j < NI; ++j) u = u + ps.R[n + j * NO] * pd[j];
        u = u + tp.td[n];
        bc[n] = w * (u * (T(gd.n[n]) / T(2)));
    }
}

// deposit_s from precomputed weights: vw = voxel_weight(dlo, s, 1), iw[n] = interp_weight(n, dlo, s)
template <typename T, int NO>
__device__ __forceinline__ T jvp_deposit_pre(T a, const T (&bc)[NO], T vw, const T* iw) {
    T v = vw * a;  // (== voxel_weight(dlo, s, a): the same product)
#pragma unroll
    for (int n = 0; n < NO; ++n) v = v + bc[n] * iw[n];
    return v;
}

template <typename T, int NO>
__device__ __forceinline__ T jvp_deposit(T a, const T (&bc)[NO], const T (&dlo)[NO], int s) {
    T iw[NO];
#pragma unroll
    for (int n = 0; n < NO; ++n) iw[n] = interp_weight<T, NO>(n, dlo, s);
    return jvp_deposit_pre<T, NO>(a, bc, voxel_weight<T, NO>(dlo, s, T(1)), iw);
}

// |deposit_s| bound of one (point, pose, tangent)
template <typename T, int NO>
__device__ __forceinline__ T jvp_bound(T a, const T (&bc)[NO]) {
    T m = a < T(0) ? -a : a;
#pragma unroll
    for (int n = 0; n < NO; ++n) m = m + (bc[n] < T(0) ? -bc[n] : bc[n]);
    return m;
}

}  // namespace dpr
