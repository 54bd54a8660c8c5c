// Device helpers of the smooth splat (include/dpr.h, "SMOOTH SPLAT") that the kernels of dpr_smooth.hip,
// dpr_smooth_channels.hip, dpr_smooth_bodies.hip, dpr_sample_smooth_channels.hip and dpr_sample_smooth_clouds.hip
// share: the cell of a point, the B-spline weights of an axis and their derivatives, the per-axis offsets of the 3^N
// cells, the pullback's sums of one (point, pose), and the rows of one tangent's deposits in forward mode.
#pragma once
#include <hip/hip_runtime.h>

#include "dpr_smooth.h"

namespace dpr {

constexpr int kSmBlock = 256;

template <typename T> __device__ __forceinline__ T floor_t(T x);
template <> __device__ __forceinline__ float floor_t<float>(float x) { return floorf(x); }
template <> __device__ __forceinline__ double floor_t<double>(double x) { return floor(x); }

// Centre cell j0 (0-based, -1 .. n_d) and offset u from its centre.  false: the point is rejected for the pose
// (some coord outside [-1, n_d + 1); the test runs in floating point before the conversion to int and rejects
// NaN / Inf).  The projection has ref_and_deltas' operation order.
template <typename T, int NI, int NO>
__device__ __forceinline__ bool smooth_cell(const T (&p)[NI], const Pose<T, NI, NO>& ps, const GridDesc<NO>& gd,
                                            int (&j0)[NO], T (&u)[NO]) {
    bool ok = true;
#pragma unroll
    for (int d = 0; d < NO; ++d) {
        T proj = ps.R[d] * p[0];
#pragma unroll
        for (int j = 1; j < NI; ++j) proj = proj + ps.R[d + j * NO] * p[j];
        const T origin = T(-1) - ps.t[d];
        const T scale = T(gd.n[d]) / T(2);
        const T coord = (proj - origin) * scale;
        ok = ok && (coord >= T(-1)) && (coord < T(gd.n[d] + 1));
        const T f = floor_t<T>(coord);
        j0[d] = ok ? (int)f : 0;
        u[d] = coord - (f + T(0.5));
    }
    return ok;
}

// the three weights of an axis and their derivatives in coord
template <typename T> __device__ __forceinline__ void spline_weights(T u, T (&w)[3]) {
    const T a = T(0.5) - u, b = T(0.5) + u;
    w[0] = a * a * T(0.5);
    w[1] = T(0.75) - u * u;
    w[2] = b * b * T(0.5);
}
template <typename T> __device__ __forceinline__ void spline_derivatives(T u, T (&dw)[3]) {
    dw[0] = -(T(0.5) - u);
    dw[1] = T(-2) * u;
    dw[2] = T(0.5) + u;
}

// Per axis: the weights and, for the three cells j0 - 1 .. j0 + 1, whether the cell is in the grid and its
// column-major offset term (0 for a dropped cell: the product would overflow an int next to 2^31 cells).
template <typename T, int NO> struct SmoothAxes {
    T w[NO][3];
    int off[NO][3];
    bool in[NO][3];
};
template <typename T, int NO>
__device__ __forceinline__ SmoothAxes<T, NO> smooth_axes(const int (&j0)[NO], const T (&u)[NO],
                                                         const GridDesc<NO>& gd) {
    SmoothAxes<T, NO> ax;
    int stride = 1;
#pragma unroll
    for (int d = 0; d < NO; ++d) {
        spline_weights<T>(u[d], ax.w[d]);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int c = j0[d] + k - 1;
            ax.in[d][k] = c >= 0 && c < gd.n[d];
            ax.off[d][k] = ax.in[d][k] ? c * stride : 0;
        }
        stride *= gd.n[d];
    }
    return ax;
}

// The sums of one (point, pose) without out_weight * point_weight:
//   W = sum_s g[j0 + s] prod_d w_d(s_d),   dcoord[k] = sum_s g[j0 + s] w'_k(s_k) prod_{d != k} w_d(s_d).
// The nine gathers of a plane (axes 0 and 1) are requested before the first is used; a dropped cell fetches cell 0
// of the pose and is replaced by 0 (a select, not a multiplication).  3-D: plane after plane, so that nine values
// are live at a time, not 27.
// smooth_point_backward_axes: the same sums, operation for operation, for axes and derivatives the caller has formed
// already -- the kernels with C planes per (point, pose) (dpr_smooth_channels.hip, dpr_sample_smooth_channels.hip) form
// them once and call this per plane.  (Two bodies, not one calling the other: the kernels compiled before the second
// user of the _axes form keep their code objects byte for byte.)
template <typename T, int NO, typename Fetch>
__device__ __forceinline__ void smooth_point_backward_axes(const SmoothAxes<T, NO>& ax, const T (&dw)[NO][3],
                                                           Fetch fetch, T (&dcoord)[NO], T& W) {
    auto plane = [&](int base, bool vb, T& S, T& S0, T& S1) {
        T gq[3][3];
#pragma unroll
        for (int k1 = 0; k1 < 3; ++k1)
#pragma unroll
            for (int k0 = 0; k0 < 3; ++k0) {
                const bool v = vb && ax.in[1][k1] && ax.in[0][k0];
                const T x = fetch(v ? base + ax.off[1][k1] + ax.off[0][k0] : 0);
                gq[k1][k0] = v ? x : T(0);
            }
        S = T(0);
        S0 = T(0);
        S1 = T(0);
#pragma unroll
        for (int k1 = 0; k1 < 3; ++k1) {
            const T a = (gq[k1][0] * ax.w[0][0] + gq[k1][1] * ax.w[0][1]) + gq[k1][2] * ax.w[0][2];
            const T da = (gq[k1][0] * dw[0][0] + gq[k1][1] * dw[0][1]) + gq[k1][2] * dw[0][2];
            S += a * ax.w[1][k1];
            S0 += da * ax.w[1][k1];
            S1 += a * dw[1][k1];
        }
    };
    if constexpr (NO == 2) {
        plane(0, true, W, dcoord[0], dcoord[1]);
    } else {
        W = T(0);
#pragma unroll
        for (int d = 0; d < NO; ++d) dcoord[d] = T(0);
#pragma unroll
        for (int k2 = 0; k2 < 3; ++k2) {
            T S, S0, S1;
            plane(ax.off[2][k2], ax.in[2][k2], S, S0, S1);
            W += S * ax.w[2][k2];
            dcoord[0] += S0 * ax.w[2][k2];
            dcoord[1] += S1 * ax.w[2][k2];
            dcoord[2] += S * dw[2][k2];
        }
    }
}
template <typename T, int NO, typename Fetch>
__device__ __forceinline__ void smooth_point_backward(const int (&j0)[NO], const T (&u)[NO], const GridDesc<NO>& gd,
                                                      Fetch fetch, T (&dcoord)[NO], T& W) {
    const SmoothAxes<T, NO> ax = smooth_axes<T, NO>(j0, u, gd);
    T dw[NO][3];
#pragma unroll
    for (int d = 0; d < NO; ++d) spline_derivatives<T>(u[d], dw[d]);
    auto plane = [&](int base, bool vb, T& S, T& S0, T& S1) {
        T gq[3][3];
#pragma unroll
        for (int k1 = 0; k1 < 3; ++k1)
#pragma unroll
            for (int k0 = 0; k0 < 3; ++k0) {
                const bool v = vb && ax.in[1][k1] && ax.in[0][k0];
                const T x = fetch(v ? base + ax.off[1][k1] + ax.off[0][k0] : 0);
                gq[k1][k0] = v ? x : T(0);
            }
        S = T(0);
        S0 = T(0);
        S1 = T(0);
#pragma unroll
        for (int k1 = 0; k1 < 3; ++k1) {
            const T a = (gq[k1][0] * ax.w[0][0] + gq[k1][1] * ax.w[0][1]) + gq[k1][2] * ax.w[0][2];
            const T da = (gq[k1][0] * dw[0][0] + gq[k1][1] * dw[0][1]) + gq[k1][2] * dw[0][2];
            S += a * ax.w[1][k1];
            S0 += da * ax.w[1][k1];
            S1 += a * dw[1][k1];
        }
    };
    if constexpr (NO == 2) {
        plane(0, true, W, dcoord[0], dcoord[1]);
    } else {
        W = T(0);
#pragma unroll
        for (int d = 0; d < NO; ++d) dcoord[d] = T(0);
#pragma unroll
        for (int k2 = 0; k2 < 3; ++k2) {
            T S, S0, S1;
            plane(ax.off[2][k2], ax.in[2][k2], S, S0, S1);
            W += S * ax.w[2][k2];
            dcoord[0] += S0 * ax.w[2][k2];
            dcoord[1] += S1 * ax.w[2][k2];
            dcoord[2] += S * dw[2][k2];
        }
    }
}

// Forward mode (include/dpr.h, "SMOOTH SPLAT, FORWARD MODE"): the rows of one tangent's deposits.  With a and
// bc_n = ow * pw * cdot_n of jvp_coeffs (dpr_jvp.h), e_d = w_d and f_d = bc_d * w'_d,
//   deposit(s) = a * prod_d e_d + sum_n f_n * prod_{d != n} e_d = e_0 * X + f_0 * Y
//   2-D: X = a * e_1 + f_1,                  Y = e_1
//   3-D: X = e_1 * (a * e_2 + f_2) + f_1 * e_2,  Y = e_1 * e_2
// X and Y once per (k1, k2); the kernels of dpr_smooth.hip and dpr_smooth_bodies.hip finish with axis 0.
template <typename T, int NO> struct SmoothJvpRows {
    T X[NO == 3 ? 3 : 1][3], Y[NO == 3 ? 3 : 1][3];
};
template <typename T, int NO>
__device__ __forceinline__ SmoothJvpRows<T, NO> smooth_jvp_rows(T a, const T (&bc)[NO], const T (&w)[NO][3],
                                                                const T (&dw)[NO][3]) {
    SmoothJvpRows<T, NO> r;
#pragma unroll
    for (int k2 = 0; k2 < (NO == 3 ? 3 : 1); ++k2) {
        const T e2 = NO == 3 ? w[NO - 1][k2] : T(1);
        const T a2 = NO == 3 ? a * e2 + bc[NO - 1] * dw[NO - 1][k2] : a;  // a * e_2 + f_2
#pragma unroll
        for (int k1 = 0; k1 < 3; ++k1) {
            r.X[k2][k1] = w[1][k1] * a2 + (bc[1] * dw[1][k1]) * e2;
            r.Y[k2][k1] = w[1][k1] * e2;
        }
    }
    return r;
}

}  // namespace dpr
