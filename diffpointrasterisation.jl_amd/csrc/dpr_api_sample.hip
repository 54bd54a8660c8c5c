// The point-sampling entry points of libdpr: host checks, AUTO rule, launches and C ABI (core: dpr_api.hip).
#include <hip/hip_runtime.h>

#include "dpr_host.h"
#include "dpr_kernels_sample.h"

namespace dpr {

// ---------------------------------------------------------------- point sampling
// dpr_sample_ex_* / dpr_sample_pullback_ex_* (include/dpr.h, "SAMPLING").  Forward: k_sample_fwd
// (DPR_ALGO_ATOMIC) for every (n_in, n_out).  Pullback: DPR_ALGO_ATOMIC, the fused k_sample_bwd with image
// atomics; DPR_ALGO_TILED for (2,2), (3,3), (3,2): k_sample_bwd without the image atomics, then ds_dimage pose
// by pose from the tiled forward (raster_tiled with B = 1, point weights ds_dvalues[:, b]).
static int check_sample_op(int op, unsigned flags) {
    if (op != DPR_OP_RASTER && op != DPR_OP_PULLBACK)
        return fail(DPR_ERR_INVALID_ARG, "sampling: op %d is not DPR_OP_RASTER / DPR_OP_PULLBACK", op);
    if (flags & 3u)
        return fail(DPR_ERR_UNSUPPORTED_ALGO,
                    "sampling keeps / reuses no binning (DPR_FLAG_KEEP_BINNING / REUSE_BINNING)");
    return DPR_OK;
}

// AUTO: the pullback takes DPR_ALGO_TILED where the single-pose forward of the same shape would
// (dpr_resolve_algo(DPR_OP_RASTER, .., P, 1)), DPR_ALGO_ATOMIC otherwise; the forward is always ATOMIC
static int resolve_algo_sample(int algo, int op, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t G) {
    if (algo != DPR_ALGO_AUTO) return algo;
    if (op == DPR_OP_PULLBACK && dims_have_all_algos(n_in, n_out)) {
        unsigned f = 0;
        if (resolve_algo(DPR_ALGO_AUTO, DPR_OP_RASTER, n_in, n_out, grid, P, 1, G, &f) == DPR_ALGO_TILED)
            return DPR_ALGO_TILED;
    }
    return DPR_ALGO_ATOMIC;
}

// the pullback's ds_dimage on DPR_ALGO_TILED: one single-pose tiled forward per pose
static size_t sample_tiled_workspace_bytes(size_t elem, unsigned flags, int n_in, int n_out, const int64_t* grid,
                                           int64_t P) {
    return tiled_workspace_bytes(elem, DPR_OP_RASTER, flags & DPR_FLAG_COHERENT_POINTS, n_in, n_out, grid, P, 1);
}

int check_sample_sizes(int64_t P, int64_t B, int64_t G) {
    if (int rc = check_point_blocks(P)) return rc;
    if (B > 0 && (P > ((int64_t)1 << 62) / B || G > ((int64_t)1 << 62) / B))
        return fail(DPR_ERR_INVALID_ARG, "P * B or the image (G * B) too large");
    if (B > (int64_t)65535 * 0x7fffffff) return fail(DPR_ERR_INVALID_ARG, "B too large");
    return DPR_OK;
}

template <typename T, int NI, int NO>
static int sample_direct(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, T* values,
                         const T* image, const T* points, const T* rot, const T* trans) {
    const GridDesc<NO> gd = make_grid_desc<NO>(grid, G);
    int64_t slices = 1;
    const int pps = pose_slices(P, B, &slices);
    dim3 gg((unsigned)((P + kBlock - 1) / kBlock), (unsigned)slices);
    hipLaunchKernelGGL((k_sample_fwd<T, NI, NO>), gg, dim3(kBlock), 0, st, gd, P, B, values, image, points, rot,
                       trans, pps);
    stage_mark(st);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

template <typename T>
static int sample_impl(void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid, int64_t P,
                       int64_t B, T* values, const T* image, const T* points, const T* rot, const T* trans,
                       void* ws, size_t ws_bytes) {
    (void)ws_bytes;
    int64_t G = 0;
    if (int rc = check_common(n_in, n_out, grid, P, B, &G)) return rc;
    if (int rc = check_sample_op(DPR_OP_RASTER, flags)) return rc;
    algo = resolve_algo_sample(algo, DPR_OP_RASTER, n_in, n_out, grid, P, G);
    if (algo != DPR_ALGO_ATOMIC)
        return fail(DPR_ERR_UNSUPPORTED_ALGO, "the sampling forward runs on DPR_ALGO_ATOMIC only (algorithm %d)",
                    algo);
    if (int rc = check_sample_sizes(P, B, G)) return rc;
    if (P == 0 || B == 0) return DPR_OK;
    if (!values) return fail(DPR_ERR_INVALID_ARG, "values is NULL");
    if (!image) return fail(DPR_ERR_INVALID_ARG, "image is NULL");
    if (!points) return fail(DPR_ERR_INVALID_ARG, "points is NULL with P > 0");
    if (!rot || !trans) return fail(DPR_ERR_INVALID_ARG, "rotation/translation is NULL");
    if (int rc = check_alignment<T>(ws, {values, image, points, rot, trans})) return rc;
    hipStream_t st = (hipStream_t)stream;
    stage_mark(st);
    return with_dims(n_in, n_out, [&](auto ni, auto no) -> int {
        return sample_direct<T, decltype(ni)::value, decltype(no)::value>(st, grid, G, P, B, values, image, points,
                                                                          rot, trans);
    });
}

template <typename T, int NI, int NO>
static int sample_pullback_run(hipStream_t st, int algo, unsigned flags, const int64_t* grid, int64_t G, int64_t P,
                               int64_t B, const T* dv, const T* image, const T* points, const T* rot,
                               const T* trans, T* d_img, T* d_pts, T* d_rot, T* d_trans, void* ws,
                               size_t ws_bytes) {
    const GridDesc<NO> gd = make_grid_desc<NO>(grid, G);
    const bool tiled = algo == DPR_ALGO_TILED;
    if (d_rot) DPR_HIP(zero_async(st, d_rot, sizeof(T) * (size_t)(B * NO * NI)));
    if (d_trans) DPR_HIP(zero_async(st, d_trans, sizeof(T) * (size_t)(B * NO)));
    if (d_img && (!tiled || P == 0)) DPR_HIP(zero_async(st, d_img, sizeof(T) * (size_t)(B * G)));
    if (d_pts && B == 0) DPR_HIP(zero_async(st, d_pts, sizeof(T) * (size_t)(P * NI)));
    if (P == 0 || B == 0) return DPR_OK;
    T* const kernel_img = tiled ? nullptr : d_img;
    if (kernel_img || d_pts || d_rot || d_trans) {
        int64_t slices = 1;
        const int pps = pose_slices(P, B, &slices);
        const int accumulate = slices > 1;
        if (accumulate && d_pts) DPR_HIP(zero_async(st, d_pts, sizeof(T) * (size_t)(P * NI)));
        dim3 gg((unsigned)((P + kBlock - 1) / kBlock), (unsigned)slices);
        hipLaunchKernelGGL((k_sample_bwd<T, NI, NO>), gg, dim3(kBlock), 0, st, gd, P, B, dv, image, points, rot,
                           trans, kernel_img, d_pts, d_rot, d_trans, pps, accumulate);
        DPR_HIP(hipGetLastError());
    }
    stage_mark(st);
    if (tiled && d_img) {
        if constexpr (dims_have_all_algos(NI, NO)) {
            // pose b: the single-pose tiled forward of weights ds_dvalues[:, b] (a contiguous column),
            // background 0, out_weight 1 -- plane b is what dpr_raster_ex_*(DPR_ALGO_TILED) returns for them
            for (int64_t b = 0; b < B; ++b)
                if (int rc = raster_tiled<T, NI, NO>(st, flags & DPR_FLAG_COHERENT_POINTS, grid, G, P, 1,
                                                     d_img + b * G, points, rot + b * (NO * NI), trans + b * NO,
                                                     nullptr, nullptr, dv + b * P, ws, ws_bytes))
                    return rc;
        } else {
            return fail(DPR_ERR_UNSUPPORTED_ALGO, "(n_in, n_out) = (%d, %d) runs on DPR_ALGO_ATOMIC only", NI, NO);
        }
    }
    return DPR_OK;
}

template <typename T>
static int sample_pullback_impl(void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                                int64_t P, int64_t B, const T* dv, const T* image, const T* points,
                                const T* rot, const T* trans, T* d_img, T* d_pts, T* d_rot, T* d_trans,
                                void* ws, size_t ws_bytes) {
    int64_t G = 0;
    if (int rc = check_common(n_in, n_out, grid, P, B, &G)) return rc;
    if (int rc = check_sample_op(DPR_OP_PULLBACK, flags)) return rc;
    if (!d_img && !d_pts && !d_rot && !d_trans)
        return fail(DPR_ERR_INVALID_ARG, "sampling pullback: every output is NULL");
    algo = resolve_algo_sample(algo, DPR_OP_PULLBACK, n_in, n_out, grid, P, G);
    if (algo != DPR_ALGO_ATOMIC && algo != DPR_ALGO_TILED)
        return fail(DPR_ERR_UNSUPPORTED_ALGO,
                    "the sampling pullback runs on DPR_ALGO_ATOMIC or DPR_ALGO_TILED (algorithm %d)", algo);
    if (algo == DPR_ALGO_TILED) {
        if (!dims_have_all_algos(n_in, n_out))
            return fail(DPR_ERR_UNSUPPORTED_ALGO, "(n_in, n_out) = (%d, %d) runs on DPR_ALGO_ATOMIC only", n_in,
                        n_out);
        const size_t need = sample_tiled_workspace_bytes(sizeof(T), flags, n_in, n_out, grid, P);
        if (need == (size_t)-1)
            return fail(DPR_ERR_UNSUPPORTED_ALGO, "DPR_ALGO_TILED: grid needs too many tiles or P >= 2^32");
        if (d_img && P > 0 && B > 0 && (!ws || ws_bytes < need))
            return fail(DPR_ERR_WORKSPACE, "DPR_ALGO_TILED sampling pullback needs %zu workspace bytes, got %zu",
                        need, ws ? ws_bytes : (size_t)0);
    }
    if (int rc = check_sample_sizes(P, B, G)) return rc;
    if (P > 0 && !points) return fail(DPR_ERR_INVALID_ARG, "points is NULL with P > 0");
    if (P > 0 && B > 0) {
        if (!dv) return fail(DPR_ERR_INVALID_ARG, "ds_dvalues is NULL");
        if (!rot || !trans) return fail(DPR_ERR_INVALID_ARG, "rotation/translation is NULL");
        if ((d_pts || d_rot || d_trans) && !image)
            return fail(DPR_ERR_INVALID_ARG, "image is NULL (needed for ds_dpoints / ds_drotation / ds_dtranslation)");
    }
    if (int rc = check_alignment<T>(ws, {dv, image, points, rot, trans, d_img, d_pts, d_rot, d_trans})) return rc;
    hipStream_t st = (hipStream_t)stream;
    stage_mark(st);
    return with_dims(n_in, n_out, [&](auto ni, auto no) -> int {
        return sample_pullback_run<T, decltype(ni)::value, decltype(no)::value>(
            st, algo, flags, grid, G, P, B, dv, image, points, rot, trans, d_img, d_pts, d_rot, d_trans, ws, ws_bytes);
    });
}

template <typename T>
static size_t workspace_sample_impl(int op, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                                    int64_t P, int64_t B) {
    int64_t G = 0;
    if (check_common(n_in, n_out, grid, P, B, &G)) return (size_t)-1;
    if (check_sample_op(op, flags)) return (size_t)-1;
    algo = resolve_algo_sample(algo, op, n_in, n_out, grid, P, G);
    if (algo == DPR_ALGO_ATOMIC) return 0;
    if (op == DPR_OP_PULLBACK && algo == DPR_ALGO_TILED && dims_have_all_algos(n_in, n_out)) {
        const size_t n = sample_tiled_workspace_bytes(sizeof(T), flags, n_in, n_out, grid, P);
        if (n == (size_t)-1)
            fail(DPR_ERR_UNSUPPORTED_ALGO, "DPR_ALGO_TILED: grid needs too many tiles or P >= 2^32");
        return n;
    }
    fail(DPR_ERR_UNSUPPORTED_ALGO, "algorithm %d has no sampling %s", algo, op == DPR_OP_RASTER ? "forward" : "pullback");
    return (size_t)-1;
}

}  // namespace dpr

extern "C" {

int dpr_resolve_algo_sample(int op, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B) {
    int64_t G = 0;
    if (int rc = dpr::check_common(n_in, n_out, grid, P, B, &G)) return rc;
    if (int rc = dpr::check_sample_op(op, 0u)) return rc;
    return dpr::resolve_algo_sample(DPR_ALGO_AUTO, op, n_in, n_out, grid, P, G);
}

#define DPR_DEFINE_SAMPLE(SUF, T)                                                                          \
    size_t dpr_workspace_bytes_sample_ex_##SUF(int op, int algo, unsigned flags, int n_in, int n_out,      \
                                               const int64_t* grid, int64_t P, int64_t B) {                \
        return dpr::workspace_sample_impl<T>(op, algo, flags, n_in, n_out, grid, P, B);                    \
    }                                                                                                      \
    int dpr_sample_ex_##SUF(void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid, \
                            int64_t P, int64_t B, T* values, const T* image, const T* points,              \
                            const T* rotation, const T* translation, void* workspace,                      \
                            size_t workspace_bytes) {                                                      \
        return dpr::sample_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B, values, image, points,    \
                                   rotation, translation, workspace, workspace_bytes);                     \
    }                                                                                                      \
    int dpr_sample_pullback_ex_##SUF(void* stream, int algo, unsigned flags, int n_in, int n_out,          \
                                     const int64_t* grid, int64_t P, int64_t B, const T* ds_dvalues,       \
                                     const T* image, const T* points, const T* rotation,                   \
                                     const T* translation, T* ds_dimage, T* ds_dpoints, T* ds_drotation,   \
                                     T* ds_dtranslation, void* workspace, size_t workspace_bytes) {        \
        return dpr::sample_pullback_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B, ds_dvalues,      \
                                            image, points, rotation, translation, ds_dimage, ds_dpoints,   \
                                            ds_drotation, ds_dtranslation, workspace, workspace_bytes);    \
    }
DPR_DEFINE_SAMPLE(f32, float)
DPR_DEFINE_SAMPLE(f64, double)
#undef DPR_DEFINE_SAMPLE

}  // extern "C"
