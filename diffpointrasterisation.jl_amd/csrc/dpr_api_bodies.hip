// The rigid-body entry points of libdpr: host checks, launches and C ABI (core: dpr_api.hip).
#include <hip/hip_runtime.h>

#include "dpr_host.h"
#include "dpr_kernels_bodies.h"

namespace dpr {

// ---------------------------------------------------------------- rigid bodies
// dpr_raster_bodies_ex_* / dpr_raster_pullback_bodies_ex_* (include/dpr.h, "RIGID BODIES"): the direct kernels of
// dpr_kernels_bodies.h, no workspace.  Every refusal comes from check_bodies, which the entry points, the workspace
// query and dpr_resolve_algo_bodies share.
static int check_bodies(int op, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid, int64_t P,
                        int64_t B, int64_t K, int64_t* G_out) {
    // (a pair of supported dimensions outside the three is refused before the grid is looked at; dimensions outside
    // 1..4 by check_common)
    if (n_in >= 1 && n_in <= 4 && n_out >= 1 && n_out <= 4 && !dims_have_all_algos(n_in, n_out))
        return fail(DPR_ERR_UNSUPPORTED_DIMS, "rigid bodies: (n_in, n_out) = (%d, %d); supports (2,2), (3,3), (3,2)",
                    n_in, n_out);
    if (int rc = check_common(n_in, n_out, grid, P, B, G_out)) return rc;
    if (op == DPR_OP_RESIDUAL_PULLBACK)
        return fail(DPR_ERR_UNSUPPORTED_ALGO, "rigid bodies have no residual pullback");
    if (op != DPR_OP_RASTER && op != DPR_OP_PULLBACK)
        return fail(DPR_ERR_INVALID_ARG, "bodies: op %d is not DPR_OP_RASTER / DPR_OP_PULLBACK", op);
    if (K < 1) return fail(DPR_ERR_INVALID_ARG, "K = %lld: a call needs at least one body", (long long)K);
    // the kernels compare a body index with K as 32-bit values and count poses b * K + k in 64 bits; the zeroing of
    // the B * K pose gradients and their offsets stay far inside both with this bound
    if (K > 0x7fffffffLL || (B > 0 && K > 0x7fffffffLL / B))
        return fail(DPR_ERR_INVALID_ARG, "B * K = %lld * %lld poses exceed 2^31 - 1", (long long)B, (long long)K);
    if (int rc = check_point_blocks(P)) return rc;
    if (flags & 3u)
        return fail(DPR_ERR_UNSUPPORTED_ALGO,
                    "rigid bodies keep / reuse no binning (DPR_FLAG_KEEP_BINNING / REUSE_BINNING)");
    if (flags & 0xff00u)
        return fail(DPR_ERR_UNSUPPORTED_ALGO, "rigid bodies form no pose groups (DPR_FLAG_MAX_POSE_GROUP)");
    if (algo != DPR_ALGO_AUTO && algo != DPR_ALGO_ATOMIC)
        return fail(DPR_ERR_UNSUPPORTED_ALGO, "algorithm %d: rigid bodies run on DPR_ALGO_ATOMIC only", algo);
    return DPR_OK;
}

template <typename T>
static int raster_bodies_impl(void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                              int64_t P, int64_t B, int64_t K, T* out, const T* points, const int32_t* body,
                              const T* rot, const T* trans, const T* bg, const T* ow, const T* pw, void* ws) {
    int64_t G = 0;
    if (int rc = check_bodies(DPR_OP_RASTER, algo, flags, n_in, n_out, grid, P, B, K, &G)) return rc;
    if (B == 0) return DPR_OK;
    if (!out) return fail(DPR_ERR_INVALID_ARG, "out is NULL");
    if (P > 0 && !points) return fail(DPR_ERR_INVALID_ARG, "points is NULL with P > 0");
    if (P > 0 && !body) return fail(DPR_ERR_INVALID_ARG, "body is NULL with P > 0");
    if (P > 0 && (!rot || !trans)) return fail(DPR_ERR_INVALID_ARG, "rotation/translation is NULL with P > 0");
    if (int rc = check_alignment<T>(ws, {out, points, rot, trans, bg, ow, pw})) return rc;
    if (int rc = check_body_alignment(body)) return rc;
    hipStream_t st = (hipStream_t)stream;
    stage_mark(st);
    fill_background(st, out, G, B, bg);
    stage_mark(st);
    if (P > 0) {
        const int rc = with_dims(n_in, n_out, [&](auto ni, auto no) -> int {
            constexpr int NI = decltype(ni)::value, NO = decltype(no)::value;
            if constexpr (dims_have_all_algos(NI, NO)) {
                const GridDesc<NO> gd = make_grid_desc<NO>(grid, G);
                dim3 gg((unsigned)((P + kBlock - 1) / kBlock), (unsigned)(B < 65535 ? B : 65535));
                hipLaunchKernelGGL((k_bodies_fwd<T, NI, NO>), gg, dim3(kBlock), 0, st, gd, P, B, (int)K, out, points,
                                   body, rot, trans, ow, pw);
            }
            return DPR_OK;
        });
        if (rc) return rc;
    }
    stage_mark(st);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

template <typename T>
static int pullback_bodies_impl(void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                                int64_t P, int64_t B, int64_t K, const T* g, const T* points, const int32_t* body,
                                const T* rot, const T* trans, const T* ow, const T* pw, T* d_pts, T* d_rot,
                                T* d_trans, T* d_bg, T* d_ow, T* d_pw, void* ws) {
    int64_t G = 0;
    if (int rc = check_bodies(DPR_OP_PULLBACK, algo, flags, n_in, n_out, grid, P, B, K, &G)) return rc;
    if (flags & DPR_FLAG_NO_POINT_WEIGHT_GRAD) d_pw = nullptr;
    if (P > 0 && (!d_pts || (!d_pw && !(flags & DPR_FLAG_NO_POINT_WEIGHT_GRAD))))
        return fail(DPR_ERR_INVALID_ARG, "ds_dpoints/ds_dpoint_weight is NULL with P > 0");
    if (B > 0) {
        if (!g) return fail(DPR_ERR_INVALID_ARG, "ds_dout is NULL");
        if (!d_rot || !d_trans || !d_bg || !d_ow)
            return fail(DPR_ERR_INVALID_ARG, "a per-pose output pointer is NULL");
        if (P > 0 && !points) return fail(DPR_ERR_INVALID_ARG, "points is NULL with P > 0");
        if (P > 0 && !body) return fail(DPR_ERR_INVALID_ARG, "body is NULL with P > 0");
        if (P > 0 && (!rot || !trans)) return fail(DPR_ERR_INVALID_ARG, "rotation/translation is NULL with P > 0");
    }
    if (int rc = check_alignment<T>(ws, {g, points, rot, trans, ow, pw, d_pts, d_rot, d_trans, d_bg, d_ow, d_pw}))
        return rc;
    if (int rc = check_body_alignment(body)) return rc;
    hipStream_t st = (hipStream_t)stream;
    stage_mark(st);
    if (B == 0) {  // no image: the sums over the poses are empty
        if (P > 0) {
            DPR_HIP(zero_async(st, d_pts, sizeof(T) * (size_t)(P * n_in)));
            if (d_pw) DPR_HIP(zero_async(st, d_pw, sizeof(T) * (size_t)P));
        }
        return DPR_OK;
    }
    DPR_HIP(zero_async(st, d_rot, sizeof(T) * (size_t)(B * K * n_out * n_in)));
    DPR_HIP(zero_async(st, d_trans, sizeof(T) * (size_t)(B * K * n_out)));
    DPR_HIP(zero_async(st, d_ow, sizeof(T) * (size_t)B));
    DPR_HIP(zero_async(st, d_bg, sizeof(T) * (size_t)B));
    grid_sum(st, g, G, B, d_bg, Residual<T>{nullptr, T(0), nullptr});
    stage_mark(st);
    if (P > 0) {
        int64_t slices = 1;
        const int poses_per_slice = pose_slices(P, B, &slices);
        const int accumulate = slices > 1;
        if (accumulate) {
            DPR_HIP(zero_async(st, d_pts, sizeof(T) * (size_t)(P * n_in)));
            if (d_pw) DPR_HIP(zero_async(st, d_pw, sizeof(T) * (size_t)P));
        }
        const int rc = with_dims(n_in, n_out, [&](auto ni, auto no) -> int {
            constexpr int NI = decltype(ni)::value, NO = decltype(no)::value;
            if constexpr (dims_have_all_algos(NI, NO)) {
                const GridDesc<NO> gd = make_grid_desc<NO>(grid, G);
                dim3 gg((unsigned)((P + kBlock - 1) / kBlock), (unsigned)slices);
                hipLaunchKernelGGL((k_bodies_bwd<T, NI, NO>), gg, dim3(kBlock), 0, st, gd, P, B, (int)K, g, points,
                                   body, rot, trans, ow, pw, d_pts, d_rot, d_trans, d_ow, d_pw, poses_per_slice,
                                   accumulate);
            }
            return DPR_OK;
        });
        if (rc) return rc;
    }
    stage_mark(st);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

}  // namespace dpr

extern "C" {

int dpr_resolve_algo_bodies(int op, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B, int64_t K) {
    int64_t G = 0;
    if (int rc = dpr::check_bodies(op, DPR_ALGO_AUTO, 0u, n_in, n_out, grid, P, B, K, &G)) return rc;
    return DPR_ALGO_ATOMIC;
}

#define DPR_DEFINE_BODIES(SUF, T)                                                                               \
    size_t dpr_workspace_bytes_bodies_ex_##SUF(int op, int algo, unsigned flags, int n_in, int n_out,           \
                                               const int64_t* grid, int64_t P, int64_t B, int64_t K) {          \
        int64_t G = 0;                                                                                          \
        return dpr::check_bodies(op, algo, flags, n_in, n_out, grid, P, B, K, &G) ? (size_t)-1 : (size_t)0;     \
    }                                                                                                           \
    int dpr_raster_bodies_ex_##SUF(void* stream, int algo, unsigned flags, int n_in, int n_out,                 \
                                   const int64_t* grid, int64_t P, int64_t B, int64_t K, T* out,                \
                                   const T* points, const void* body, const T* rotation, const T* translation,  \
                                   const T* background, const T* out_weight, const T* point_weight,             \
                                   void* workspace, size_t workspace_bytes) {                                   \
        (void)workspace_bytes;                                                                                  \
        return dpr::raster_bodies_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B, K, out, points,         \
                                          (const int32_t*)body, rotation, translation, background, out_weight,  \
                                          point_weight, workspace);                                             \
    }                                                                                                           \
    int dpr_raster_pullback_bodies_ex_##SUF(                                                                    \
        void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B, \
        int64_t K, const T* ds_dout, const T* points, const void* body, const T* rotation, const T* translation, \
        const T* out_weight, const T* point_weight, T* ds_dpoints, T* ds_drotation, T* ds_dtranslation,         \
        T* ds_dbackground, T* ds_dout_weight, T* ds_dpoint_weight, void* workspace, size_t workspace_bytes) {   \
        (void)workspace_bytes;                                                                                  \
        return dpr::pullback_bodies_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B, K, ds_dout, points,   \
                                            (const int32_t*)body, rotation, translation, out_weight,            \
                                            point_weight, ds_dpoints, ds_drotation, ds_dtranslation,            \
                                            ds_dbackground, ds_dout_weight, ds_dpoint_weight, workspace);       \
    }
DPR_DEFINE_BODIES(f32, float)
DPR_DEFINE_BODIES(f64, double)
#undef DPR_DEFINE_BODIES

}  // extern "C"
