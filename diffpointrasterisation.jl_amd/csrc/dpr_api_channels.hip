// The multi-channel entry points of libdpr: host checks, AUTO rule, launches and C ABI (core: dpr_api.hip).
#include <hip/hip_runtime.h>

#include "dpr_host.h"
#include "dpr_kernels_channels.h"

namespace dpr {

// ---------------------------------------------------------------- C weight channels
// dpr_raster_channels_ex_* / dpr_raster_pullback_channels_ex_* (include/dpr.h, "MULTI-CHANNEL").
// Forward: DPR_ALGO_ATOMIC for every (n_in, n_out); DPR_ALGO_TILED for (2,2), (3,3), (3,2) on the
// per-pose binning path of single-slab grids.  Pullback: DPR_ALGO_ATOMIC.
static int check_channels(int64_t C, unsigned flags, bool residual = false) {
    if (C < 1 || C > kMaxChannels)
        return fail(DPR_ERR_INVALID_ARG, "channels C = %lld out of range [1, %d]", (long long)C, kMaxChannels);
    if (flags & 3u)
        return fail(DPR_ERR_UNSUPPORTED_ALGO,
                    "the channel entry points keep / reuse no binning (DPR_FLAG_KEEP_BINNING / REUSE_BINNING)");
    if (residual)
        return fail(DPR_ERR_UNSUPPORTED_ALGO, "the channel entry points have no residual pullback");
    return DPR_OK;
}

// AUTO: the forward takes DPR_ALGO_TILED where the single-channel rule prefers it for the shape and the
// channel path supports it; everything else (and every pullback) runs on DPR_ALGO_ATOMIC
static int resolve_algo_channels(int algo, int op, int n_in, int n_out, const int64_t* grid, int64_t P,
                                 int64_t B, int64_t G) {
    if (algo != DPR_ALGO_AUTO) return algo;
    if (op == DPR_OP_RASTER && dims_have_all_algos(n_in, n_out) && tiled_channels_supported(n_out, grid, P) &&
        tiled_preferred(DPR_OP_RASTER, n_out, grid, P, B, G))
        return DPR_ALGO_TILED;
    return DPR_ALGO_ATOMIC;
}

template <typename T, int NI, int NO>
static int raster_atomic_channels(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int C,
                                  T* out, const T* points, const T* rot, const T* trans, const T* bg,
                                  const T* ow, const T* pw) {
    const GridDesc<NO> gd = make_grid_desc<NO>(grid, G);
    // B * C planes, plane k = b * C + c, background[k] (C x B, channel fastest)
    fill_background(st, out, G, B * C, bg);
    stage_mark(st);
    if (P > 0) {
        dim3 g((unsigned)((P + kBlock - 1) / kBlock), (unsigned)(B < 65535 ? B : 65535));
        if (C <= 4)
            hipLaunchKernelGGL((k_fwd_atomic_ch<T, NI, NO, 4>), g, dim3(kBlock), 0, st, gd, P, B, C, out, points,
                               rot, trans, ow, pw);
        else
            hipLaunchKernelGGL((k_fwd_atomic_ch<T, NI, NO, kMaxChannels>), g, dim3(kBlock), 0, st, gd, P, B, C,
                               out, points, rot, trans, ow, pw);
    }
    stage_mark(st);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

template <typename T>
static int raster_channels_impl(void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                                int64_t P, int64_t B, int64_t C, T* out, const T* points, const T* rot,
                                const T* trans, const T* bg, const T* ow, const T* pw, void* ws,
                                size_t ws_bytes) {
    int64_t G = 0;
    if (int rc = check_common(n_in, n_out, grid, P, B, &G)) return rc;
    if (int rc = check_channels(C, flags)) return rc;
    if (B == 0) return DPR_OK;
    if (!out) return fail(DPR_ERR_INVALID_ARG, "out is NULL");
    if (!rot || !trans) return fail(DPR_ERR_INVALID_ARG, "rotation/translation is NULL");
    if (P > 0 && !points) return fail(DPR_ERR_INVALID_ARG, "points is NULL with P > 0");
    if (int rc = check_point_blocks(P)) return rc;
    if (G * C * B / B != G * C || G * C > ((int64_t)1 << 62) / (B > 0 ? B : 1))
        return fail(DPR_ERR_INVALID_ARG, "output too large");
    if (int rc = check_alignment<T>(ws, {out, points, rot, trans, bg, ow, pw})) return rc;
    hipStream_t st = (hipStream_t)stream;
    algo = resolve_algo_channels(algo, DPR_OP_RASTER, n_in, n_out, grid, P, B, G);
    if (algo == DPR_ALGO_TILED && !dims_have_all_algos(n_in, n_out))
        return fail(DPR_ERR_UNSUPPORTED_ALGO,
                    "(n_in, n_out) = (%d, %d) runs on DPR_ALGO_ATOMIC only", n_in, n_out);
    if (algo == DPR_ALGO_TILED && !tiled_channels_supported(n_out, grid, P))
        return fail(DPR_ERR_UNSUPPORTED_ALGO,
                    "DPR_ALGO_TILED with channels: per-pose binning of single-slab grids and P < 2^32 only");
    if (algo != DPR_ALGO_ATOMIC && algo != DPR_ALGO_TILED)
        return fail(DPR_ERR_UNSUPPORTED_ALGO, "the channel forward runs on DPR_ALGO_ATOMIC or DPR_ALGO_TILED "
                                              "(algorithm %d)", algo);
    stage_mark(st);
    const int c = (int)C;
    return with_dims(n_in, n_out, [&](auto ni, auto no) -> int {
        constexpr int NI = decltype(ni)::value, NO = decltype(no)::value;
        // (algo is ATOMIC, or TILED on a pair that has it)
        if constexpr (dims_have_all_algos(NI, NO)) {
            if (algo == DPR_ALGO_TILED)
                return raster_tiled_channels<T, NI, NO>(st, grid, G, P, B, c, out, points, rot, trans, bg, ow, pw,
                                                        ws, ws_bytes);
        }
        return raster_atomic_channels<T, NI, NO>(st, grid, G, P, B, c, out, points, rot, trans, bg, ow, pw);
    });
}

// The DPR_ALGO_ATOMIC pullback launch: defined in dpr_api_channels_pullback.h and instantiated in the
// dpr_api_channels_pullback_*.hip units, which share out the compile time of k_bwd_gather_ch
template <typename T, int NI, int NO>
int pullback_atomic_channels(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int C,
                             const T* g, const T* points, const T* rot, const T* trans, const T* ow,
                             const T* pw, T* d_pts, T* d_rot, T* d_trans, T* d_bg, T* d_ow, T* d_pw);

template <typename T>
static int pullback_channels_impl(void* stream, int algo, unsigned flags, int n_in, int n_out,
                                  const int64_t* grid, int64_t P, int64_t B, int64_t C, const T* g,
                                  const T* points, const T* rot, const T* trans, const T* ow, const T* pw,
                                  T* d_pts, T* d_rot, T* d_trans, T* d_bg, T* d_ow, T* d_pw, void* ws,
                                  size_t ws_bytes) {
    (void)ws_bytes;
    int64_t G = 0;
    if (int rc = check_common(n_in, n_out, grid, P, B, &G)) return rc;
    if (int rc = check_channels(C, flags)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (flags & DPR_FLAG_NO_POINT_WEIGHT_GRAD) d_pw = nullptr;
    if (P > 0 && (!d_pts || (!d_pw && !(flags & DPR_FLAG_NO_POINT_WEIGHT_GRAD))))
        return fail(DPR_ERR_INVALID_ARG, "ds_dpoints/ds_dpoint_weight is NULL with P > 0");
    if (P > 0 && !points) return fail(DPR_ERR_INVALID_ARG, "points is NULL with P > 0");
    algo = resolve_algo_channels(algo, DPR_OP_PULLBACK, n_in, n_out, grid, P, B, G);
    if (algo != DPR_ALGO_ATOMIC)
        return fail(DPR_ERR_UNSUPPORTED_ALGO, "the channel pullback runs on DPR_ALGO_ATOMIC only (algorithm %d)",
                    algo);
    if (B == 0) {
        if (P > 0) {
            DPR_HIP(zero_async(st, d_pts, sizeof(T) * (size_t)(P * n_in)));
            if (d_pw) DPR_HIP(zero_async(st, d_pw, sizeof(T) * (size_t)(P * C)));
        }
        return DPR_OK;
    }
    if (!g) return fail(DPR_ERR_INVALID_ARG, "ds_dout is NULL");
    if (!rot || !trans) return fail(DPR_ERR_INVALID_ARG, "rotation/translation is NULL");
    if (!d_rot || !d_trans || !d_bg || !d_ow)
        return fail(DPR_ERR_INVALID_ARG, "a per-pose output pointer is NULL");
    if (int rc = check_point_blocks(P)) return rc;
    if (int rc = check_alignment<T>(ws, {g, points, rot, trans, ow, pw, d_pts, d_rot, d_trans, d_bg, d_ow, d_pw}))
        return rc;
    stage_mark(st);
    const int c = (int)C;
    return with_dims(n_in, n_out, [&](auto ni, auto no) -> int {
        return pullback_atomic_channels<T, decltype(ni)::value, decltype(no)::value>(
            st, grid, G, P, B, c, g, points, rot, trans, ow, pw, d_pts, d_rot, d_trans, d_bg, d_ow, d_pw);
    });
}

template <typename T>
static size_t workspace_channels_impl(int op, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                                      int64_t P, int64_t B, int64_t C) {
    int64_t G = 0;
    if (check_common(n_in, n_out, grid, P, B, &G)) return (size_t)-1;
    if (op != DPR_OP_RASTER && op != DPR_OP_PULLBACK) {
        fail(op == DPR_OP_RESIDUAL_PULLBACK ? DPR_ERR_UNSUPPORTED_ALGO : DPR_ERR_INVALID_ARG,
             op == DPR_OP_RESIDUAL_PULLBACK ? "the channel entry points have no residual pullback" : "unknown op %d",
             op);
        return (size_t)-1;
    }
    if (check_channels(C, flags)) return (size_t)-1;
    algo = resolve_algo_channels(algo, op, n_in, n_out, grid, P, B, G);
    if (algo == DPR_ALGO_ATOMIC) return 0;
    if (op == DPR_OP_RASTER && algo == DPR_ALGO_TILED && dims_have_all_algos(n_in, n_out)) {
        const size_t n = tiled_channels_workspace_bytes(sizeof(T), n_in, n_out, grid, P, B, (int)C);
        if (n == (size_t)-1)
            fail(DPR_ERR_UNSUPPORTED_ALGO,
                 "DPR_ALGO_TILED with channels: per-pose binning of single-slab grids and P < 2^32 only");
        return n;
    }
    fail(DPR_ERR_UNSUPPORTED_ALGO, "algorithm %d has no channel %s", algo, op == DPR_OP_RASTER ? "forward" : "pullback");
    return (size_t)-1;
}

}  // namespace dpr

extern "C" {

int dpr_resolve_algo_channels(int op, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B,
                              int64_t C) {
    int64_t G = 0;
    if (int rc = dpr::check_common(n_in, n_out, grid, P, B, &G)) return rc;
    if (op != DPR_OP_RASTER && op != DPR_OP_PULLBACK)
        return dpr::fail(op == DPR_OP_RESIDUAL_PULLBACK ? DPR_ERR_UNSUPPORTED_ALGO : DPR_ERR_INVALID_ARG,
                         "channels: op %d is not DPR_OP_RASTER / DPR_OP_PULLBACK", op);
    if (int rc = dpr::check_channels(C, 0u)) return rc;
    return dpr::resolve_algo_channels(DPR_ALGO_AUTO, op, n_in, n_out, grid, P, B, G);
}

#define DPR_DEFINE_CHANNELS(SUF, T)                                                                   \
    size_t dpr_workspace_bytes_channels_ex_##SUF(int op, int algo, unsigned flags, int n_in, int n_out, \
                                                 const int64_t* grid, int64_t P, int64_t B, int64_t C) { \
        return dpr::workspace_channels_impl<T>(op, algo, flags, n_in, n_out, grid, P, B, C);          \
    }                                                                                                 \
    int dpr_raster_channels_ex_##SUF(void* stream, int algo, unsigned flags, int n_in, int n_out,     \
                                     const int64_t* grid, int64_t P, int64_t B, int64_t C, T* out,    \
                                     const T* points, const T* rotation, const T* translation,        \
                                     const T* background, const T* out_weight, const T* point_weight, \
                                     void* workspace, size_t workspace_bytes) {                       \
        return dpr::raster_channels_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B, C, out,     \
                                            points, rotation, translation, background, out_weight,    \
                                            point_weight, workspace, workspace_bytes);                \
    }                                                                                                 \
    int dpr_raster_pullback_channels_ex_##SUF(                                                        \
        void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid, int64_t P,  \
        int64_t B, int64_t C, const T* ds_dout, const T* points, const T* rotation,                   \
        const T* translation, const T* out_weight, const T* point_weight, T* ds_dpoints,              \
        T* ds_drotation, T* ds_dtranslation, T* ds_dbackground, T* ds_dout_weight,                    \
        T* ds_dpoint_weight, void* workspace, size_t workspace_bytes) {                               \
        return dpr::pullback_channels_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B, C,        \
                                              ds_dout, points, rotation, translation, out_weight,     \
                                              point_weight, ds_dpoints, ds_drotation,                 \
                                              ds_dtranslation, ds_dbackground, ds_dout_weight,        \
                                              ds_dpoint_weight, workspace, workspace_bytes);          \
    }
DPR_DEFINE_CHANNELS(f32, float)
DPR_DEFINE_CHANNELS(f64, double)
#undef DPR_DEFINE_CHANNELS

}  // extern "C"
