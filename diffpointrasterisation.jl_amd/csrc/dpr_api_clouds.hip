// The per-pose-cloud entry points of libdpr: host checks, AUTO rule, launches and C ABI (core: dpr_api.hip).
#include <hip/hip_runtime.h>

#include "dpr_host.h"
#include "dpr_kernels_clouds.h"

namespace dpr {

// ---------------------------------------------------------------- per-pose clouds
// dpr_raster_clouds_ex_* / dpr_raster_pullback_clouds_ex_* (include/dpr.h, "PER-POSE CLOUDS").  DPR_ALGO_ATOMIC:
// k_clouds_fwd_atomic / k_clouds_bwd_atomic, every (n_in, n_out).  For (2,2), (3,3), (3,2): DPR_ALGO_TILED runs the
// single-pose tiled path pose by pose on the offset pointers (workspace reused), DPR_ALGO_CHUNKED the pose-owned LDS
// tiles of dpr_kernels_clouds.h.
static int check_clouds_op(int op, unsigned flags) {
    if (op == DPR_OP_RESIDUAL_PULLBACK)
        return fail(DPR_ERR_UNSUPPORTED_ALGO, "per-pose clouds have no residual pullback");
    if (op != DPR_OP_RASTER && op != DPR_OP_PULLBACK)
        return fail(DPR_ERR_INVALID_ARG, "clouds: op %d is not DPR_OP_RASTER / DPR_OP_PULLBACK", op);
    if (flags & 3u)
        return fail(DPR_ERR_UNSUPPORTED_ALGO,
                    "per-pose clouds keep / reuse no binning (DPR_FLAG_KEEP_BINNING / REUSE_BINNING)");
    return DPR_OK;
}

// 64-bit offsets: cloud b starts at b * P * n_in, plane b at b * G
static int check_clouds_sizes(int n_in, int64_t P, int64_t B, int64_t G) {
    if (int rc = check_point_blocks(P)) return rc;
    if (B > 0 && (P > ((int64_t)1 << 60) / B / n_in || G > ((int64_t)1 << 62) / B))
        return fail(DPR_ERR_INVALID_ARG, "B * P * n_in or the image (G * B) too large");
    return DPR_OK;
}

template <int NO> static CloudTiles<NO> clouds_tiles(const int64_t* grid) {
    CloudTiles<NO> ct;
    ct.tiles = 1;
    for (int d = 0; d < NO; ++d) {
        const int e = CloudTileShape<NO>::e[d];
        ct.nt[d] = (int)((grid[d] + e - 1) / e);
        ct.tiles *= ct.nt[d];
    }
    return ct;
}
static int64_t clouds_tile_count(int n_out, const int64_t* grid) {
    return n_out == 2 ? clouds_tiles<2>(grid).tiles : clouds_tiles<3>(grid).tiles;
}

// Slices of each cloud on DPR_ALGO_CHUNKED: enough workgroups (pose x tile x slice) to fill 256 CUs with two
// resident workgroups four times over, and no slice under 2048 points.
struct CloudsPlan {
    int64_t tiles, slices, slice_len;
};
static CloudsPlan clouds_plan(int n_out, const int64_t* grid, int64_t P, int64_t B) {
    CloudsPlan pl;
    pl.tiles = clouds_tile_count(n_out, grid);
    const int64_t items = pl.tiles * (B > 0 ? B : 1);
    int64_t s = (2048 + items - 1) / items;
    const int64_t by_points = (P + 2047) / 2048;
    if (s > by_points) s = by_points;
    if (s > 64) s = 64;
    if (s < 1) s = 1;
    pl.slice_len = (P + s - 1) / s;
    if (pl.slice_len < 1) pl.slice_len = 1;
    pl.slices = (P + pl.slice_len - 1) / pl.slice_len;
    if (pl.slices < 1) pl.slices = 1;
    return pl;
}

// AUTO (dpr_resolve_algo_clouds), host arithmetic on the shape and the element size (profiles/clouds_probe.txt):
//  - the forward: DPR_ALGO_CHUNKED while a pose's grid is at most kCloudsChunkedMaxTiles tiles (every tile re-reads
//    its slices of the cloud; 128^2 x 256 poses of 2e4 points: 0.14 ms against 1.0 ms ATOMIC, 64^3 x 32 of 1e5:
//    0.51 against 1.5 ms TILED);
//  - the pullback: DPR_ALGO_CHUNKED on 2-D grids of fp32 data within the same bound (128^2 x 256: 0.14 against
//    0.16 ms ATOMIC); on 3-D grids (64^3 x 32: 0.77 against 0.25 ms) and for fp64 data (128^2 x 256: 0.27 against
//    0.20 ms) the direct gathers of DPR_ALGO_ATOMIC are faster;
//  - then DPR_ALGO_TILED where the single-pose rule prefers it (256^3 x 4 of 2e6: 0.44 / 0.46 ms against 3.1 / 0.63
//    ATOMIC), DPR_ALGO_ATOMIC otherwise and for the other pairs.
constexpr int64_t kCloudsChunkedMaxTiles = 32;
static int resolve_algo_clouds(int algo, int op, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t G,
                               size_t elem) {
    if (algo != DPR_ALGO_AUTO) return algo;
    if (!dims_have_all_algos(n_in, n_out)) return DPR_ALGO_ATOMIC;
    if (clouds_tile_count(n_out, grid) <= kCloudsChunkedMaxTiles &&
        (op == DPR_OP_RASTER || (n_out == 2 && elem == 4)))
        return DPR_ALGO_CHUNKED;
    if (tiled_preferred(op, n_out, grid, P, 1, G) &&
        tiled_workspace_bytes(elem, op, 0u, n_in, n_out, grid, P, 1) != (size_t)-1)
        return DPR_ALGO_TILED;
    return DPR_ALGO_ATOMIC;
}

// bytes of workspace, or (size_t)-1 (message recorded) when the algorithm cannot run the shape
static size_t clouds_workspace_bytes(size_t elem, int op, int algo, int n_in, int n_out, const int64_t* grid,
                                     int64_t P, int64_t B) {
    if (algo == DPR_ALGO_ATOMIC) return 0;
    if (algo != DPR_ALGO_TILED && algo != DPR_ALGO_CHUNKED) {
        fail(DPR_ERR_UNSUPPORTED_ALGO, "unknown algorithm %d", algo);
        return (size_t)-1;
    }
    if (!dims_have_all_algos(n_in, n_out)) {
        fail(DPR_ERR_UNSUPPORTED_ALGO, "(n_in, n_out) = (%d, %d): per-pose clouds run on DPR_ALGO_ATOMIC only",
             n_in, n_out);
        return (size_t)-1;
    }
    if (algo == DPR_ALGO_TILED) {
        // the single-pose tiled workspace, reused from pose to pose
        const size_t n = tiled_workspace_bytes(elem, op, 0u, n_in, n_out, grid, P, 1);
        if (n == (size_t)-1)
            fail(DPR_ERR_UNSUPPORTED_ALGO, "DPR_ALGO_TILED: grid needs too many tiles or P >= 2^32");
        return n;
    }
    if (op == DPR_OP_RASTER) return elem == 4 ? align_up(sizeof(uint32_t) * (size_t)B) : 0;  // per-pose weight keys
    const CloudsPlan pl = clouds_plan(n_out, grid, P, B);
    return align_up(sizeof(double) * (size_t)(n_out * n_in + n_out + 1) * (size_t)B * (size_t)(pl.tiles * pl.slices));
}

template <typename T, int NI, int NO>
static int raster_clouds_run(hipStream_t st, int algo, const int64_t* grid, int64_t G, int64_t P, int64_t B, T* out,
                             const T* points, const T* rot, const T* trans, const T* bg, const T* ow, const T* pw,
                             void* ws, size_t ws_bytes) {
    const GridDesc<NO> gd = make_grid_desc<NO>(grid, G);
    if (algo == DPR_ALGO_ATOMIC || P == 0) {
        fill_background(st, out, G, B, bg);
        stage_mark(st);
        if (P > 0) {
            dim3 g((unsigned)((P + kBlock - 1) / kBlock), (unsigned)(B < 65535 ? B : 65535));
            hipLaunchKernelGGL((k_clouds_fwd_atomic<T, NI, NO>), g, dim3(kBlock), 0, st, gd, P, B, out, points, rot,
                               trans, ow, pw);
        }
        stage_mark(st);
        DPR_HIP(hipGetLastError());
        return DPR_OK;
    }
    if constexpr (!dims_have_all_algos(NI, NO)) {
        return fail(DPR_ERR_UNSUPPORTED_ALGO, "(n_in, n_out) = (%d, %d) runs on DPR_ALGO_ATOMIC only", NI, NO);
    } else {
        if (algo == DPR_ALGO_TILED) {
            // plane b: exactly dpr_raster_ex_*(DPR_ALGO_TILED) of (cloud b, pose b)
            for (int64_t b = 0; b < B; ++b)
                if (int rc = raster_tiled<T, NI, NO>(st, 0u, grid, G, P, 1, out + b * G, points + b * P * NI,
                                                     rot + b * (NO * NI), trans + b * NO, bg ? bg + b : nullptr,
                                                     ow ? ow + b : nullptr, pw ? pw + b * P : nullptr, ws, ws_bytes))
                    return rc;
            return DPR_OK;
        }
        const CloudTiles<NO> ct = clouds_tiles<NO>(grid);
        const CloudsPlan pl = clouds_plan(NO, grid, P, B);
        const uint32_t* keys = nullptr;
        if constexpr (sizeof(T) == 4) {  // the per-pose weight ranges of the fixed-point scale
            if (pw) {
                hipLaunchKernelGGL(k_clouds_wrange<T>, dim3((unsigned)B), dim3(256), 0, st, pw, P, (int64_t)0,
                                   (uint32_t*)ws);
                keys = (const uint32_t*)ws;
            }
        }
        const int atomic_flush = pl.slices > 1;
        if (atomic_flush) fill_background(st, out, G, B, bg);
        stage_mark(st);
        for (int64_t b0 = 0; b0 < B; b0 += 65535) {
            const int64_t nb = B - b0 < 65535 ? B - b0 : 65535;
            hipLaunchKernelGGL((k_clouds_fwd_tile<T, NI, NO>), dim3((unsigned)(pl.tiles * pl.slices), (unsigned)nb),
                               dim3(kCLThreads), 0, st, gd, ct, (int)pl.slices, pl.slice_len, P, b0, out, points, rot,
                               trans, bg, ow, pw, keys, atomic_flush);
        }
        stage_mark(st);
        DPR_HIP(hipGetLastError());
        return DPR_OK;
    }
}

template <typename T>
static int raster_clouds_impl(void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                              int64_t P, int64_t B, T* out, const T* points, const T* rot, const T* trans,
                              const T* bg, const T* ow, const T* pw, void* ws, size_t ws_bytes) {
    int64_t G = 0;
    if (int rc = check_common(n_in, n_out, grid, P, B, &G)) return rc;
    if (int rc = check_clouds_op(DPR_OP_RASTER, flags)) return rc;
    if (int rc = check_clouds_sizes(n_in, P, B, G)) return rc;
    algo = resolve_algo_clouds(algo, DPR_OP_RASTER, n_in, n_out, grid, P, G, sizeof(T));
    const size_t need = clouds_workspace_bytes(sizeof(T), DPR_OP_RASTER, algo, n_in, n_out, grid, P, B);
    if (need == (size_t)-1) return DPR_ERR_UNSUPPORTED_ALGO;
    if (B == 0) return DPR_OK;
    if (!out) return fail(DPR_ERR_INVALID_ARG, "out is NULL");
    if (!rot || !trans) return fail(DPR_ERR_INVALID_ARG, "rotation/translation is NULL");
    if (P > 0 && !points) return fail(DPR_ERR_INVALID_ARG, "points is NULL with P > 0");
    if (P > 0 && need > 0 && (!ws || ws_bytes < need))
        return fail(DPR_ERR_WORKSPACE, "per-pose clouds (algorithm %d) need %zu workspace bytes, got %zu", algo, need,
                    ws ? ws_bytes : (size_t)0);
    if (int rc = check_alignment<T>(ws, {out, points, rot, trans, bg, ow, pw})) return rc;
    hipStream_t st = (hipStream_t)stream;
    stage_mark(st);
    return with_dims(n_in, n_out, [&](auto ni, auto no) -> int {
        return raster_clouds_run<T, decltype(ni)::value, decltype(no)::value>(st, algo, grid, G, P, B, out, points,
                                                                              rot, trans, bg, ow, pw, ws, ws_bytes);
    });
}

template <typename T, int NI, int NO>
static int pullback_clouds_run(hipStream_t st, int algo, unsigned flags, const int64_t* grid, int64_t G, int64_t P,
                               int64_t B, const T* g, const T* points, const T* rot, const T* trans, const T* ow,
                               const T* pw, T* d_pts, T* d_rot, T* d_trans, T* d_bg, T* d_ow, T* d_pw, void* ws,
                               size_t ws_bytes) {
    const GridDesc<NO> gd = make_grid_desc<NO>(grid, G);
    if constexpr (dims_have_all_algos(NI, NO)) {
        if (algo == DPR_ALGO_TILED && P > 0) {
            // pose b: exactly dpr_raster_pullback_ex_*(DPR_ALGO_TILED) of (cloud b, pose b)
            const Residual<T> none{nullptr, T(0), nullptr};
            for (int64_t b = 0; b < B; ++b)
                if (int rc = pullback_tiled<T, NI, NO>(
                        st, flags & DPR_FLAG_NO_POINT_WEIGHT_GRAD, grid, G, P, 1, g + b * G, points + b * P * NI,
                        rot + b * (NO * NI), trans + b * NO, ow ? ow + b : nullptr, pw ? pw + b * P : nullptr,
                        d_pts + b * P * NI, d_rot + b * (NO * NI), d_trans + b * NO, d_bg + b, d_ow + b,
                        d_pw ? d_pw + b * P : nullptr, ws, ws_bytes, none))
                    return rc;
            return DPR_OK;
        }
    }
    DPR_HIP(zero_async(st, d_bg, sizeof(T) * (size_t)B));
    grid_sum(st, g, G, B, d_bg, Residual<T>{nullptr, T(0), nullptr});
    stage_mark(st);
    if (algo == DPR_ALGO_ATOMIC || P == 0) {
        DPR_HIP(zero_async(st, d_rot, sizeof(T) * (size_t)(B * NO * NI)));
        DPR_HIP(zero_async(st, d_trans, sizeof(T) * (size_t)(B * NO)));
        DPR_HIP(zero_async(st, d_ow, sizeof(T) * (size_t)B));
        if (P > 0) {
            dim3 gg((unsigned)((P + kBlock - 1) / kBlock), (unsigned)(B < 65535 ? B : 65535));
            hipLaunchKernelGGL((k_clouds_bwd_atomic<T, NI, NO>), gg, dim3(kBlock), 0, st, gd, P, B, g, points, rot,
                               trans, ow, pw, d_pts, d_rot, d_trans, d_ow, d_pw);
        }
        stage_mark(st);
        DPR_HIP(hipGetLastError());
        return DPR_OK;
    }
    if constexpr (!dims_have_all_algos(NI, NO)) {
        return fail(DPR_ERR_UNSUPPORTED_ALGO, "(n_in, n_out) = (%d, %d) runs on DPR_ALGO_ATOMIC only", NI, NO);
    } else {
        (void)ws_bytes;
        const CloudTiles<NO> ct = clouds_tiles<NO>(grid);
        const CloudsPlan pl = clouds_plan(NO, grid, P, B);
        const int64_t parts = pl.tiles * pl.slices;
        double* partials = (double*)ws;
        for (int64_t b0 = 0; b0 < B; b0 += 65535) {
            const int64_t nb = B - b0 < 65535 ? B - b0 : 65535;
            hipLaunchKernelGGL((k_clouds_bwd_tile<T, NI, NO>), dim3((unsigned)parts, (unsigned)nb), dim3(kCLThreads),
                               0, st, gd, ct, (int)pl.slices, pl.slice_len, P, B, b0, g, points, rot, trans, ow, pw,
                               d_pts, d_pw, partials);
        }
        for (int64_t b0 = 0; b0 < B; b0 += 65535) {
            const int64_t nb = B - b0 < 65535 ? B - b0 : 65535;
            hipLaunchKernelGGL((k_clouds_reduce<T, NI, NO>), dim3(NO * NI + NO + 1, (unsigned)nb), dim3(256), 0, st,
                               partials, B, b0, parts, d_rot, d_trans, d_ow);
        }
        stage_mark(st);
        DPR_HIP(hipGetLastError());
        return DPR_OK;
    }
}

template <typename T>
static int pullback_clouds_impl(void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                                int64_t P, int64_t B, const T* g, const T* points, const T* rot, const T* trans,
                                const T* ow, const T* pw, T* d_pts, T* d_rot, T* d_trans, T* d_bg, T* d_ow, T* d_pw,
                                void* ws, size_t ws_bytes) {
    int64_t G = 0;
    if (int rc = check_common(n_in, n_out, grid, P, B, &G)) return rc;
    if (int rc = check_clouds_op(DPR_OP_PULLBACK, flags)) return rc;
    if (int rc = check_clouds_sizes(n_in, P, B, G)) return rc;
    if (flags & DPR_FLAG_NO_POINT_WEIGHT_GRAD) d_pw = nullptr;
    algo = resolve_algo_clouds(algo, DPR_OP_PULLBACK, n_in, n_out, grid, P, G, sizeof(T));
    const size_t need = clouds_workspace_bytes(sizeof(T), DPR_OP_PULLBACK, algo, n_in, n_out, grid, P, B);
    if (need == (size_t)-1) return DPR_ERR_UNSUPPORTED_ALGO;
    if (B == 0) return DPR_OK;  // (every output is empty)
    if (!g) return fail(DPR_ERR_INVALID_ARG, "ds_dout is NULL");
    if (!rot || !trans) return fail(DPR_ERR_INVALID_ARG, "rotation/translation is NULL");
    if (!d_rot || !d_trans || !d_bg || !d_ow) return fail(DPR_ERR_INVALID_ARG, "a per-pose output pointer is NULL");
    if (P > 0 && (!d_pts || (!d_pw && !(flags & DPR_FLAG_NO_POINT_WEIGHT_GRAD))))
        return fail(DPR_ERR_INVALID_ARG, "ds_dpoints/ds_dpoint_weight is NULL with P > 0");
    if (P > 0 && !points) return fail(DPR_ERR_INVALID_ARG, "points is NULL with P > 0");
    if (P > 0 && need > 0 && (!ws || ws_bytes < need))
        return fail(DPR_ERR_WORKSPACE, "per-pose clouds (algorithm %d) need %zu workspace bytes, got %zu", algo, need,
                    ws ? ws_bytes : (size_t)0);
    if (int rc = check_alignment<T>(ws, {g, points, rot, trans, ow, pw, d_pts, d_rot, d_trans, d_bg, d_ow, d_pw}))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    stage_mark(st);
    return with_dims(n_in, n_out, [&](auto ni, auto no) -> int {
        return pullback_clouds_run<T, decltype(ni)::value, decltype(no)::value>(
            st, algo, flags, grid, G, P, B, g, points, rot, trans, ow, pw, d_pts, d_rot, d_trans, d_bg, d_ow, d_pw, ws,
            ws_bytes);
    });
}

template <typename T>
static size_t workspace_clouds_impl(int op, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                                    int64_t P, int64_t B) {
    int64_t G = 0;
    if (check_common(n_in, n_out, grid, P, B, &G)) return (size_t)-1;
    if (check_clouds_op(op, flags)) return (size_t)-1;
    if (check_clouds_sizes(n_in, P, B, G)) return (size_t)-1;
    algo = resolve_algo_clouds(algo, op, n_in, n_out, grid, P, G, sizeof(T));
    return clouds_workspace_bytes(sizeof(T), op, algo, n_in, n_out, grid, P, B);
}

}  // namespace dpr

extern "C" {

int dpr_resolve_algo_clouds(int op, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B) {
    int64_t G = 0;
    if (int rc = dpr::check_common(n_in, n_out, grid, P, B, &G)) return rc;
    if (int rc = dpr::check_clouds_op(op, 0u)) return rc;
    return dpr::resolve_algo_clouds(DPR_ALGO_AUTO, op, n_in, n_out, grid, P, G, sizeof(float));
}

#define DPR_DEFINE_CLOUDS(SUF, T)                                                                              \
    size_t dpr_workspace_bytes_clouds_ex_##SUF(int op, int algo, unsigned flags, int n_in, int n_out,          \
                                               const int64_t* grid, int64_t P, int64_t B) {                    \
        return dpr::workspace_clouds_impl<T>(op, algo, flags, n_in, n_out, grid, P, B);                        \
    }                                                                                                          \
    int dpr_raster_clouds_ex_##SUF(void* stream, int algo, unsigned flags, int n_in, int n_out,                \
                                   const int64_t* grid, int64_t P, int64_t B, T* out, const T* points,         \
                                   const T* rotation, const T* translation, const T* background,               \
                                   const T* out_weight, const T* point_weight, void* workspace,                \
                                   size_t workspace_bytes) {                                                   \
        return dpr::raster_clouds_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B, out, points, rotation, \
                                          translation, background, out_weight, point_weight, workspace,        \
                                          workspace_bytes);                                                    \
    }                                                                                                          \
    int dpr_raster_pullback_clouds_ex_##SUF(                                                                   \
        void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B, \
        const T* ds_dout, const T* points, const T* rotation, const T* translation, const T* out_weight,       \
        const T* point_weight, T* ds_dpoints, T* ds_drotation, T* ds_dtranslation, T* ds_dbackground,          \
        T* ds_dout_weight, T* ds_dpoint_weight, void* workspace, size_t workspace_bytes) {                     \
        return dpr::pullback_clouds_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B, ds_dout, points,     \
                                            rotation, translation, out_weight, point_weight, ds_dpoints,       \
                                            ds_drotation, ds_dtranslation, ds_dbackground, ds_dout_weight,     \
                                            ds_dpoint_weight, workspace, workspace_bytes);                     \
    }
DPR_DEFINE_CLOUDS(f32, float)
DPR_DEFINE_CLOUDS(f64, double)
#undef DPR_DEFINE_CLOUDS

}  // extern "C"
