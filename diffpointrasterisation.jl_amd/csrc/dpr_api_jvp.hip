// The forward-mode entry points of libdpr: host checks, AUTO rule, launches and C ABI (core: dpr_api.hip).
#include <hip/hip_runtime.h>

#include "dpr_host.h"
#include "dpr_kernels_jvp.h"

namespace dpr {

// ---------------------------------------------------------------- forward-mode derivative
// dpr_raster_jvp_ex_* (include/dpr.h, "FORWARD-MODE DERIVATIVE").  DPR_ALGO_ATOMIC: k_jvp_fill, then k_jvp_atomic,
// every (n_in, n_out).  DPR_ALGO_TILED for (2,2), (3,3), (3,2) on single-slab grids: raster_tiled_jvp.
int check_jvp(int64_t K, unsigned flags) {
    if (K < 1 || K > kMaxTangents)
        return fail(DPR_ERR_INVALID_ARG, "tangents K = %lld out of range [1, %d]", (long long)K, kMaxTangents);
    if (flags & 3u)
        return fail(DPR_ERR_UNSUPPORTED_ALGO,
                    "the JVP keeps / reuses no binning (DPR_FLAG_KEEP_BINNING / REUSE_BINNING)");
    return DPR_OK;
}

// AUTO: DPR_ALGO_TILED where the pair and the grid support it and the single-pose forward of the shape would take
// it (dpr_resolve_algo(DPR_OP_RASTER, .., P, 1)), DPR_ALGO_ATOMIC otherwise
static int resolve_algo_jvp(int algo, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t G) {
    if (algo != DPR_ALGO_AUTO) return algo;
    if (dims_have_all_algos(n_in, n_out) && tiled_channels_supported(n_out, grid, P)) {
        unsigned f = 0;
        if (resolve_algo(DPR_ALGO_AUTO, DPR_OP_RASTER, n_in, n_out, grid, P, 1, G, &f) == DPR_ALGO_TILED)
            return DPR_ALGO_TILED;
    }
    return DPR_ALGO_ATOMIC;
}

// workspace of an algorithm that is not AUTO, or (size_t)-1 with the error recorded
static size_t jvp_workspace_bytes(size_t elem, int algo, int n_in, int n_out, const int64_t* grid, int64_t P) {
    if (algo == DPR_ALGO_ATOMIC) return 0;
    if (algo == DPR_ALGO_TILED) {
        if (!dims_have_all_algos(n_in, n_out)) {
            fail(DPR_ERR_UNSUPPORTED_ALGO, "(n_in, n_out) = (%d, %d): the JVP runs on DPR_ALGO_ATOMIC only", n_in,
                 n_out);
            return (size_t)-1;
        }
        const size_t n = tiled_jvp_workspace_bytes(elem, n_in, n_out, grid, P);
        if (n == (size_t)-1)
            fail(DPR_ERR_UNSUPPORTED_ALGO, "DPR_ALGO_TILED JVP: per-pose binning of single-slab grids and P < 2^32 only");
        return n;
    }
    fail(DPR_ERR_UNSUPPORTED_ALGO, "the JVP runs on DPR_ALGO_ATOMIC or DPR_ALGO_TILED (algorithm %d)", algo);
    return (size_t)-1;
}

template <typename T>
void jvp_fill(hipStream_t st, T* out_dot, int64_t G, int K, int64_t B, const T* bg_dot) {
    const int64_t planes = B * K;
    const int64_t want = (G + kBlock - 1) / kBlock;
    dim3 g((unsigned)(want < 4096 ? want : 4096), 1);
    for (int64_t q0 = 0; q0 < planes; q0 += 65535) {
        const int64_t nq = (planes - q0 < 65535) ? planes - q0 : 65535;
        g.y = (unsigned)nq;
        hipLaunchKernelGGL(k_jvp_fill<T>, g, dim3(kBlock), 0, st, out_dot, G, K, B, q0, bg_dot);
    }
}
template void jvp_fill<float>(hipStream_t, float*, int64_t, int, int64_t, const float*);
template void jvp_fill<double>(hipStream_t, double*, int64_t, int, int64_t, const double*);

template <typename T, int NI, int NO>
static int raster_jvp_run(hipStream_t st, int algo, const int64_t* grid, int64_t G, int64_t P, int64_t B, int K,
                          T* out_dot, const T* points, const T* rot, const T* trans, const T* ow, const T* pw,
                          JvpTangents<T> tan, const T* bg_dot, void* ws, size_t ws_bytes) {
    const bool any = tan.points || tan.rot || tan.trans || tan.ow || tan.pw;
    if (algo == DPR_ALGO_TILED && P > 0 && any) {
        if constexpr (dims_have_all_algos(NI, NO))
            return raster_tiled_jvp<T, NI, NO>(st, grid, G, P, B, K, out_dot, points, rot, trans, ow, pw, tan,
                                               bg_dot, ws, ws_bytes);
        return fail(DPR_ERR_UNSUPPORTED_ALGO, "(n_in, n_out) = (%d, %d) runs on DPR_ALGO_ATOMIC only", NI, NO);
    }
    // the background tangent (or 0) into every plane; then the deposits, where any other tangent is given
    jvp_fill(st, out_dot, G, K, B, bg_dot);
    stage_mark(st);
    if (P > 0 && any) {
        const GridDesc<NO> gd = make_grid_desc<NO>(grid, G);
        int64_t slices = 1;
        const int pps = pose_slices(P, B, &slices);
        dim3 gg((unsigned)((P + kBlock - 1) / kBlock), (unsigned)slices);
        hipLaunchKernelGGL((k_jvp_atomic<T, NI, NO>), gg, dim3(kBlock), 0, st, gd, P, B, K, out_dot, points, rot,
                           trans, ow, pw, tan, pps);
        stage_mark(st);
    }
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

template <typename T>
static int raster_jvp_impl(void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                           int64_t P, int64_t B, int64_t K, T* out_dot, const T* points, const T* rot,
                           const T* trans, const T* ow, const T* pw, JvpTangents<T> tan, const T* bg_dot, void* ws,
                           size_t ws_bytes) {
    int64_t G = 0;
    if (int rc = check_common(n_in, n_out, grid, P, B, &G)) return rc;
    if (int rc = check_jvp(K, flags)) return rc;
    algo = resolve_algo_jvp(algo, n_in, n_out, grid, P, G);
    const size_t need = jvp_workspace_bytes(sizeof(T), algo, n_in, n_out, grid, P);
    if (need == (size_t)-1) return DPR_ERR_UNSUPPORTED_ALGO;  // (the message is recorded)
    if (B == 0) return DPR_OK;
    if (!out_dot) return fail(DPR_ERR_INVALID_ARG, "out_dot is NULL");
    if (!rot || !trans) return fail(DPR_ERR_INVALID_ARG, "rotation/translation is NULL");
    if (P > 0 && !points) return fail(DPR_ERR_INVALID_ARG, "points is NULL with P > 0");
    if (int rc = check_sample_sizes(P, B, G)) return rc;
    if (G * K > ((int64_t)1 << 62) / B) return fail(DPR_ERR_INVALID_ARG, "output too large");
    if (need > 0 && P > 0 && (!ws || ws_bytes < need))
        return fail(DPR_ERR_WORKSPACE, "DPR_ALGO_TILED JVP needs %zu workspace bytes, got %zu", need,
                    ws ? ws_bytes : (size_t)0);
    if (int rc = check_alignment<T>(ws, {out_dot, points, rot, trans, ow, pw, tan.points, tan.rot, tan.trans, tan.ow,
                                         tan.pw, bg_dot}))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    stage_mark(st);
    const int k = (int)K;
    return with_dims(n_in, n_out, [&](auto ni, auto no) -> int {
        return raster_jvp_run<T, decltype(ni)::value, decltype(no)::value>(st, algo, grid, G, P, B, k, out_dot, points,
                                                                           rot, trans, ow, pw, tan, bg_dot, ws,
                                                                           ws_bytes);
    });
}

template <typename T>
static size_t workspace_jvp_impl(int algo, unsigned flags, int n_in, int n_out, const int64_t* grid, int64_t P,
                                 int64_t B, int64_t K) {
    int64_t G = 0;
    if (check_common(n_in, n_out, grid, P, B, &G)) return (size_t)-1;
    if (check_jvp(K, flags)) return (size_t)-1;
    algo = resolve_algo_jvp(algo, n_in, n_out, grid, P, G);
    return jvp_workspace_bytes(sizeof(T), algo, n_in, n_out, grid, P);
}

}  // namespace dpr

extern "C" {

int dpr_resolve_algo_jvp(int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B, int64_t K) {
    int64_t G = 0;
    if (int rc = dpr::check_common(n_in, n_out, grid, P, B, &G)) return rc;
    if (int rc = dpr::check_jvp(K, 0u)) return rc;
    return dpr::resolve_algo_jvp(DPR_ALGO_AUTO, n_in, n_out, grid, P, G);
}

#define DPR_DEFINE_JVP(SUF, T)                                                                                 \
    size_t dpr_workspace_bytes_jvp_ex_##SUF(int algo, unsigned flags, int n_in, int n_out, const int64_t* grid, \
                                            int64_t P, int64_t B, int64_t K) {                                 \
        return dpr::workspace_jvp_impl<T>(algo, flags, n_in, n_out, grid, P, B, K);                            \
    }                                                                                                          \
    int dpr_raster_jvp_ex_##SUF(void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid, \
                                int64_t P, int64_t B, int64_t K, T* out_dot, const T* points, const T* rotation, \
                                const T* translation, const T* out_weight, const T* point_weight,              \
                                const T* points_dot, const T* rotation_dot, const T* translation_dot,          \
                                const T* background_dot, const T* out_weight_dot, const T* point_weight_dot,   \
                                void* workspace, size_t workspace_bytes) {                                     \
        return dpr::raster_jvp_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B, K, out_dot, points,       \
                                       rotation, translation, out_weight, point_weight,                        \
                                       dpr::JvpTangents<T>{points_dot, rotation_dot, translation_dot,          \
                                                           out_weight_dot, point_weight_dot},                  \
                                       background_dot, workspace, workspace_bytes);                            \
    }
DPR_DEFINE_JVP(f32, float)
DPR_DEFINE_JVP(f64, double)
#undef DPR_DEFINE_JVP

}  // extern "C"
