// Smooth sampling at per-pose clouds (include/dpr.h, "SMOOTH SAMPLING, PER-POSE CLOUDS"): the image
// dpr_raster_smooth_clouds_ex_* writes, read back at the clouds -- pose b reads cloud b.
//
//   points / ds_dpoints   cloud b at b * P * NI
//   values / ds_dvalues   (B, P), point index fastest: row b at b * P -- a point_weight of the smooth cloud splat
//   image / ds_dimage     (n_1, .., n_N, B) column-major, as `out`
//
//   forward    k_sample_smooth_clouds_fwd: k_smooth_clouds_fwd_atomic's launch shape (a thread per (point, pose), a
//              block inside one pose, the poses strided over gridDim.y), k_sample_smooth_fwd's gathers and sums; no
//              atomics, every value stored.  Row b has the bits of k_sample_smooth_fwd on (image b, cloud b, pose b)
//   pullback   k_sample_smooth_clouds_bwd: k_sample_smooth_bwd's terms of one (point, pose) in its order; ds_dpoints is
//              one plain store per (point, pose), the per-pose sums leave the block as k_smooth_clouds_bwd's do;
//              ds_dimage by 3^N global atomics (DPR_ALGO_ATOMIC)
//   DPR_ALGO_TILED pullback: this kernel without ds_dimage; dpr_api_smooth.hip then runs smooth_clouds_fwd_tiled
//              (dpr_smooth.hip) with ds_dvalues as the point weights
// These are copies of the sampling kernels with the clouds' indexing, not shared bodies: the kernels of dpr_smooth.hip
// keep their code objects byte for byte.
#include <hip/hip_runtime.h>

#include "../../include/dpr.h"
#include "dpr_smooth.h"
#include "dpr_smooth_device.h"

namespace dpr {

// Forward: the value of (point p, pose b) into values[b * P + p], coalesced; 0 for a rejected point.
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kSmBlock) void k_sample_smooth_clouds_fwd(GridDesc<NO> gd, int64_t P, int64_t B,
                                                                       T* __restrict__ values,
                                                                       const T* __restrict__ image,
                                                                       const T* __restrict__ points,
                                                                       const T* __restrict__ rot,
                                                                       const T* __restrict__ trans) {
    static_assert(NO == 2 || NO == 3, "the smooth splat is written for 2-D and 3-D grids");
    const int64_t p = (int64_t)blockIdx.x * kSmBlock + threadIdx.x;
    if (p >= P) return;
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        T pt[NI];
        load_point<T, NI>(points + b * P * NI, p, pt);
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

// Pullback of one (point, pose) per thread for dv = ds_dvalues[b, p].  Any output may be NULL (uniform branches; the
// image is read only for the three geometric gradients).  Pre-zeroed: ds_drotation, ds_dtranslation, ds_dimage;
// ds_dpoints is stored for every live (point, pose), 0 for a rejected point.
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kSmBlock) void k_sample_smooth_clouds_bwd(
    GridDesc<NO> gd, int64_t P, int64_t B, const T* __restrict__ ds_dvalues, const T* __restrict__ image,
    const T* __restrict__ points, const T* __restrict__ rot, const T* __restrict__ trans,
    T* __restrict__ ds_dimage, T* __restrict__ ds_dpoints, T* __restrict__ ds_drotation,
    T* __restrict__ ds_dtranslation) {
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
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {  // (uniform over the block)
        const Pose<T, NI, NO> ps = load_pose<T, NI, NO>(rot, trans, nullptr, b);
        const int64_t q = b * P + p;  // (point, pose) index of values and point gradients
        T pt[NI];
#pragma unroll
        for (int j = 0; j < NI; ++j) pt[j] = T(0);
        if (live) load_point<T, NI>(points + b * P * NI, p, pt);
        T vals[NV], gpt[NI];
#pragma unroll
        for (int k = 0; k < NV; ++k) vals[k] = T(0);
#pragma unroll
        for (int j = 0; j < NI; ++j) gpt[j] = T(0);
        int j0[NO];
        T u[NO];
        if (live && smooth_cell<T, NI, NO>(pt, ps, gd, j0, u)) {
            const T dv = ds_dvalues[q];
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
                    gpt[j] += v;
                }
            }
        }
        if (live && ds_dpoints) {
#pragma unroll
            for (int j = 0; j < NI; ++j) ds_dpoints[q * NI + j] = gpt[j];
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
}

// ---------------------------------------------------------------- host
template <typename T, int NI, int NO>
int sample_smooth_clouds_fwd(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, T* values,
                             const T* image, const T* points, const T* rot, const T* trans) {
    if (P <= 0 || B <= 0) return DPR_OK;
    const GridDesc<NO> gd = make_grid_desc<NO>(grid, G);
    dim3 gg((unsigned)((P + kSmBlock - 1) / kSmBlock), (unsigned)(B < 65535 ? B : 65535));
    hipLaunchKernelGGL((k_sample_smooth_clouds_fwd<T, NI, NO>), gg, dim3(kSmBlock), 0, st, gd, P, B, values, image,
                       points, rot, trans);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

template <typename T, int NI, int NO>
int sample_smooth_clouds_bwd(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, const T* dv,
                             const T* image, const T* points, const T* rot, const T* trans, T* d_img, T* d_pts,
                             T* d_rot, T* d_trans) {
    if (P <= 0 || B <= 0 || !(d_img || d_pts || d_rot || d_trans)) return DPR_OK;
    const GridDesc<NO> gd = make_grid_desc<NO>(grid, G);
    dim3 gg((unsigned)((P + kSmBlock - 1) / kSmBlock), (unsigned)(B < 65535 ? B : 65535));
    hipLaunchKernelGGL((k_sample_smooth_clouds_bwd<T, NI, NO>), gg, dim3(kSmBlock), 0, st, gd, P, B, dv, image, points,
                       rot, trans, d_img, d_pts, d_rot, d_trans);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

#define DPR_SAMPLE_SMOOTH_CLOUDS_INSTANTIATE(T, NI, NO)                                                            \
    template int sample_smooth_clouds_fwd<T, NI, NO>(hipStream_t, const int64_t*, int64_t, int64_t, int64_t, T*,   \
                                                     const T*, const T*, const T*, const T*);                     \
    template int sample_smooth_clouds_bwd<T, NI, NO>(hipStream_t, const int64_t*, int64_t, int64_t, int64_t,       \
                                                     const T*, const T*, const T*, const T*, const T*, T*, T*, T*, \
                                                     T*);
#define DPR_SAMPLE_SMOOTH_CLOUDS_INSTANTIATE_T(T)                                                \
    DPR_SAMPLE_SMOOTH_CLOUDS_INSTANTIATE(T, 2, 2) DPR_SAMPLE_SMOOTH_CLOUDS_INSTANTIATE(T, 3, 3) \
    DPR_SAMPLE_SMOOTH_CLOUDS_INSTANTIATE(T, 3, 2)
DPR_SAMPLE_SMOOTH_CLOUDS_INSTANTIATE_T(float)
DPR_SAMPLE_SMOOTH_CLOUDS_INSTANTIATE_T(double)

}  // namespace dpr
