// The smooth rigid-body entry points of libdpr -- splat, pullback, forward mode and sampling: host checks, AUTO rules
// and C ABI (include/dpr.h, "SMOOTH SPLAT, RIGID BODIES", "SMOOTH SPLAT, RIGID BODIES, FORWARD MODE" and "SMOOTH
// SAMPLING, RIGID BODIES"; core: dpr_api.hip; kernels and their launches: dpr_smooth_bodies.hip,
// dpr_sample_smooth_bodies.hip).
#include <hip/hip_runtime.h>

#include "dpr_host.h"
#include "dpr_smooth.h"

namespace dpr {

// ---------------------------------------------------------------- host checks
// AUTO (dpr_resolve_algo_smooth_bodies), from the shape alone.  The pullback is DPR_ALGO_ATOMIC.  The forward is
// DPR_ALGO_TILED where the default GROUP of images holds bg * P >= the constant below and the cloud holds at least
// kSmoothBodiesTiledMinPointsPerTile points per tile of the grid, DPR_ALGO_ATOMIC otherwise: the shape of
// dpr_resolve_algo_smooth_clouds' rule, because the tiled path pays its four launches per group here too.  K does not
// enter: TILED / ATOMIC move by less than 10 % from K = 1 to 64 and between a sorted and a shuffled cloud.  From this
// op's own rows (profiles/smooth_bodies_probe.txt, tests/golden/smooth_bodies_auto.json; fp32, ms TILED / ATOMIC):
//  - 3-D, 1e5 (the smooth clouds' constant, confirmed): 128^3, 1e4 x 4 images (bg * P = 4e4) 0.130 / 0.130 and
//    0.128 / 0.114, 3e4 x 4 (1.2e5) 0.155 / 0.214, 1e4 x 16 0.235 / 0.271, 1e6 x 4 0.35 / 4.4.
//  - 2-D, 1.6e5 (the smooth clouds' 4e5 lost this op's two lowest rows): 128^2, 1e4 x 16 (1.6e5) 0.121 / 0.144 --
//    1.19x, beyond the 1.15 margin -- 1e4 x 32 0.176 / 0.200, 3e4 x 16 0.192 / 0.266; 512^2, 3e4 x 16 0.203 / 0.269,
//    1e6 x 16 0.91 / 6.2.  TILED is ahead on every 2-D row measured; nothing was measured below 1.6e5.
//  - 4 points per tile (confirmed): 256^3 (16 384 tiles), 1e4 x 16 (0.6 per tile) 0.685 / 0.426, 3e4 x 4 (1.8)
//    0.309 / 0.244, 1e5 x 4 (6.1) 0.424 / 0.534; 128^3, 1e4 x 16 (4.9) 0.235 / 0.271.
constexpr int64_t kSmoothBodiesTiledMinWork3D = 100000;
constexpr int64_t kSmoothBodiesTiledMinWork2D = 160000;
constexpr int64_t kSmoothBodiesTiledMinPointsPerTile = 4;
static int resolve_algo_smooth_bodies(int algo, int op, int n_out, const int64_t* grid, int64_t P, int64_t B) {
    if (algo != DPR_ALGO_AUTO) return algo;
    if (op != DPR_OP_RASTER) return DPR_ALGO_ATOMIC;
    const int64_t bg = smooth_clouds_group(n_out, grid, P, B, 0);
    if (bg == 0) return DPR_ALGO_ATOMIC;
    const int64_t min_work = n_out == 3 ? kSmoothBodiesTiledMinWork3D : kSmoothBodiesTiledMinWork2D;
    const int64_t tiles = smooth_tile_count(n_out, grid, P);
    return bg * P >= min_work && P / kSmoothBodiesTiledMinPointsPerTile >= tiles ? DPR_ALGO_TILED : DPR_ALGO_ATOMIC;
}

// Every refusal of the family, shared by the entry points, the workspace query and dpr_resolve_algo_smooth_bodies;
// *G, the resolved *algo and the workspace bytes *need come back.
static int check_smooth_bodies(int op, int* algo, unsigned flags, int n_in, int n_out, const int64_t* grid, int64_t P,
                               int64_t B, int64_t K, int64_t* G, size_t* need) {
    // (a pair outside the three is refused before the grid is looked at)
    if (!smooth_dims_supported(n_in, n_out))
        return fail(DPR_ERR_UNSUPPORTED_DIMS,
                    "smooth rigid bodies: (n_in, n_out) = (%d, %d); supports (2,2), (3,3), (3,2)", n_in, n_out);
    if (int rc = check_common(n_in, n_out, grid, P, B, G)) return rc;
    if (op == DPR_OP_RESIDUAL_PULLBACK)
        return fail(DPR_ERR_UNSUPPORTED_ALGO, "smooth rigid bodies have no residual pullback");
    if (op != DPR_OP_RASTER && op != DPR_OP_PULLBACK)
        return fail(DPR_ERR_INVALID_ARG, "smooth bodies: op %d is not DPR_OP_RASTER / DPR_OP_PULLBACK", op);
    if (K < 1) return fail(DPR_ERR_INVALID_ARG, "K = %lld: a call needs at least one body", (long long)K);
    // the kernels compare a body index with K as 32-bit values and count poses b * K + k in 64 bits; the zeroing of
    // the B * K pose gradients and their offsets stay far inside both with this bound
    if (K > 0x7fffffffLL || (B > 0 && K > 0x7fffffffLL / B))
        return fail(DPR_ERR_INVALID_ARG, "B * K = %lld * %lld poses exceed 2^31 - 1", (long long)B, (long long)K);
    if (int rc = check_point_blocks(P)) return rc;
    if (flags & 3u)
        return fail(DPR_ERR_UNSUPPORTED_ALGO,
                    "smooth rigid bodies keep / reuse no binning (DPR_FLAG_KEEP_BINNING / REUSE_BINNING)");
    if (op == DPR_OP_PULLBACK && (flags & 0xff00u))
        return fail(DPR_ERR_UNSUPPORTED_ALGO,
                    "the smooth rigid-body pullback forms no groups of images (DPR_FLAG_MAX_POSE_GROUP)");
    if (*algo != DPR_ALGO_AUTO && *algo != DPR_ALGO_ATOMIC && *algo != DPR_ALGO_TILED)
        return fail(DPR_ERR_UNSUPPORTED_ALGO,
                    "smooth rigid bodies run on DPR_ALGO_ATOMIC and DPR_ALGO_TILED, not algorithm %d", *algo);
    if (*algo == DPR_ALGO_TILED && op != DPR_OP_RASTER)
        return fail(DPR_ERR_UNSUPPORTED_ALGO, "the smooth rigid-body pullback runs on DPR_ALGO_ATOMIC only");
    *algo = resolve_algo_smooth_bodies(*algo, op, n_out, grid, P, B);
    *need = 0;
    if (*algo == DPR_ALGO_TILED) {
        *need = smooth_clouds_tiled_workspace_bytes(n_out, grid, P, B, max_pose_group(flags));
        if (*need == (size_t)-1) return fail(DPR_ERR_UNSUPPORTED_ALGO, kSmoothTiledRefused);
    }
    return DPR_OK;
}

template <typename T>
static int raster_smooth_bodies_impl(void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                                     int64_t P, int64_t B, int64_t K, T* out, const T* points, const int32_t* body,
                                     const T* rot, const T* trans, const T* bg, const T* ow, const T* pw, void* ws,
                                     size_t ws_bytes) {
    int64_t G = 0;
    size_t need = 0;
    if (int rc = check_smooth_bodies(DPR_OP_RASTER, &algo, flags, n_in, n_out, grid, P, B, K, &G, &need)) return rc;
    if (B == 0) return DPR_OK;
    if (!out) return fail(DPR_ERR_INVALID_ARG, "out is NULL");
    if (P > 0 && !points) return fail(DPR_ERR_INVALID_ARG, "points is NULL with P > 0");
    if (P > 0 && !body) return fail(DPR_ERR_INVALID_ARG, "body is NULL with P > 0");
    if (P > 0 && (!rot || !trans)) return fail(DPR_ERR_INVALID_ARG, "rotation/translation is NULL with P > 0");
    if (P > 0 && need > 0 && (!ws || ws_bytes < need))
        return fail(DPR_ERR_WORKSPACE, "smooth rigid bodies (algorithm %d) need %zu workspace bytes, got %zu", algo,
                    need, ws ? ws_bytes : (size_t)0);
    if (int rc = check_alignment<T>(ws, {out, points, rot, trans, bg, ow, pw})) return rc;
    if ((uintptr_t)body & 3) return fail(DPR_ERR_INVALID_ARG, "body is not aligned to its element type (int32_t)");
    hipStream_t st = (hipStream_t)stream;
    stage_mark(st);
    fill_background(st, out, G, B, bg);
    stage_mark(st);
    return with_smooth_dims(n_in, n_out, [&](auto ni, auto no) -> int {
        constexpr int NI = decltype(ni)::value, NO = decltype(no)::value;
        const int rc = algo == DPR_ALGO_TILED
                           ? smooth_bodies_fwd_tiled<T, NI, NO>(st, grid, G, P, B, (int)K,
                                                                max_pose_group(flags), out, points, body, rot,
                                                                trans, ow, pw, ws, ws_bytes)
                           : smooth_bodies_fwd_atomic<T, NI, NO>(st, grid, G, P, B, (int)K, out, points, body, rot,
                                                                 trans, ow, pw);
        stage_mark(st);
        return rc;
    });
}

template <typename T>
static int pullback_smooth_bodies_impl(void* stream, int algo, unsigned flags, int n_in, int n_out,
                                       const int64_t* grid, int64_t P, int64_t B, int64_t K, const T* g,
                                       const T* points, const int32_t* body, const T* rot, const T* trans,
                                       const T* ow, const T* pw, T* d_pts, T* d_rot, T* d_trans, T* d_bg, T* d_ow,
                                       T* d_pw, void* ws) {
    int64_t G = 0;
    size_t need = 0;
    if (int rc = check_smooth_bodies(DPR_OP_PULLBACK, &algo, flags, n_in, n_out, grid, P, B, K, &G, &need)) return rc;
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
    if ((uintptr_t)body & 3) return fail(DPR_ERR_INVALID_ARG, "body is not aligned to its element type (int32_t)");
    hipStream_t st = (hipStream_t)stream;
    stage_mark(st);
    if (B == 0) {  // no image: the sums over the images are empty
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
    if (P == 0) return DPR_OK;  // (the pose sums are 0, ds_dbackground is done)
    int64_t slices = 1;
    const int poses_per_slice = pose_slices(P, B, &slices);  // (the smooth pullback's: SUMMATION ORDER, note 1)
    return with_smooth_dims(n_in, n_out, [&](auto ni, auto no) -> int {
        const int rc = smooth_bodies_bwd_atomic<T, decltype(ni)::value, decltype(no)::value>(
            st, grid, G, P, B, (int)K, g, points, body, rot, trans, ow, pw, d_pts, d_rot, d_trans, d_ow, d_pw,
            poses_per_slice, slices);
        stage_mark(st);
        return rc;
    });
}

// ---------------------------------------------------------------- forward mode: host checks and entry point
// AUTO (dpr_resolve_algo_smooth_bodies_jvp), from the shape and V alone: the forward's rule -- DPR_ALGO_TILED where the
// default GROUP holds enough work and the cloud at least 4 points per tile -- with the group's work counted as
// bg * P * V^2.  The rule started as the forward's with bg * P * V (what dpr_resolve_algo_smooth_jvp does with P * K);
// this op's own rows (profiles/smooth_bodies_jvp_probe.txt, tests/golden/smooth_bodies_jvp_auto.json; fp32, K = 4,
// ms ATOMIC / TILED) leave no constant for that product: on 128^2 1000 x 4 images at V = 12 (bg * P * V = 4.8e4) is
// 0.111 / 0.087 -- TILED 1.28x ahead -- and 1e4 x 8 at V = 1 (8e4) 0.095 / 0.122 -- ATOMIC 1.28x ahead; on 64^3 1100 x 2 at
// V = 12 (2.6e4) 0.205 / 0.122 against 1e4 x 4 at V = 1 (4e4, 128^3) 0.117 / 0.147.  The binning is paid once per group
// whatever V and costs about what one tangent's atomics cost, so the bg * P from which TILED pays falls faster than
// 1 / V: at V = 12 TILED is ahead on every row measured with 4 points per tile (down to bg * P = 2200), at V = 1 from about the forward's
// constants on.  V^2 puts both on one side of one constant each:
//  - 2-D, 1.6e5 (the forward's, confirmed): V = 1, 128^2, 1e4 x 12 (1.2e5) 0.111 / 0.126, 1e4 x 16 (1.6e5) 0.126 / 0.132 --
//    1.04x behind --, 3e4 x 16 0.255 / 0.204.
//  - 3-D, 9.6e4 (the forward's 1e5 lost this op's row 64^3, 24 000 x 4 at V = 1: 0.178 / 0.133, 1.34x): below it 1e4 x 4
//    (4e4) 0.108 / 0.113 on 64^3 and 0.117 / 0.147 on 128^3.
//  - 4 points per tile (confirmed): 256^3, 1e4 x 16 (0.6 per tile) 0.44 / 0.80 and 4.39 / 7.65 at V = 12, 3e4 x 4 (1.8)
//    0.25 / 0.36 and 2.17 / 3.15, 1e5 x 4 (6.1) 0.53 / 0.49 and 5.64 / 4.06.
// Only V = 1 and V = 12 were measured: between them the square is an interpolation.
constexpr int64_t kSmoothBodiesJvpTiledMinWork3D = 96000;
constexpr int64_t kSmoothBodiesJvpTiledMinWork2D = 160000;
constexpr int64_t kSmoothBodiesJvpTiledMinPointsPerTile = 4;
static int resolve_algo_smooth_bodies_jvp(int algo, int n_out, const int64_t* grid, int64_t P, int64_t B, int64_t V) {
    if (algo != DPR_ALGO_AUTO) return algo;
    const int64_t bg = smooth_clouds_group(n_out, grid, P, B, 0);
    if (bg == 0) return DPR_ALGO_ATOMIC;
    const int64_t min_work = n_out == 3 ? kSmoothBodiesJvpTiledMinWork3D : kSmoothBodiesJvpTiledMinWork2D;
    const int64_t tiles = smooth_tile_count(n_out, grid, P);
    // (bg * P <= 2^24 for bg > 1, P < 2^32 for bg = 1, V <= 16: the product stays inside 64 bits)
    return bg * P * V * V >= min_work && P / kSmoothBodiesJvpTiledMinPointsPerTile >= tiles ? DPR_ALGO_TILED
                                                                                          : DPR_ALGO_ATOMIC;
}

// Every refusal of the forward-mode entry points, shared by them, the workspace query and
// dpr_resolve_algo_smooth_bodies_jvp; *G, the resolved *algo and the workspace bytes *need come back.
static int check_smooth_bodies_jvp(int* algo, unsigned flags, int n_in, int n_out, const int64_t* grid, int64_t P,
                                   int64_t B, int64_t K, int64_t V, int64_t* G, size_t* need) {
    if (!smooth_dims_supported(n_in, n_out))
        return fail(DPR_ERR_UNSUPPORTED_DIMS,
                    "smooth rigid bodies, forward mode: (n_in, n_out) = (%d, %d); supports (2,2), (3,3), (3,2)", n_in,
                    n_out);
    if (int rc = check_common(n_in, n_out, grid, P, B, G)) return rc;
    if (K < 1) return fail(DPR_ERR_INVALID_ARG, "K = %lld: a call needs at least one body", (long long)K);
    if (K > 0x7fffffffLL || (B > 0 && K > 0x7fffffffLL / B))
        return fail(DPR_ERR_INVALID_ARG, "B * K = %lld * %lld poses exceed 2^31 - 1", (long long)B, (long long)K);
    if (int rc = check_jvp(V, flags)) return rc;  // (V in 1 .. kMaxTangents; KEEP / REUSE refused)
    if (int rc = check_sample_sizes(P, B, *G)) return rc;
    if (B > 0 && *G * V > ((int64_t)1 << 62) / B) return fail(DPR_ERR_INVALID_ARG, "output too large");
    if (*algo != DPR_ALGO_AUTO && *algo != DPR_ALGO_ATOMIC && *algo != DPR_ALGO_TILED)
        return fail(DPR_ERR_UNSUPPORTED_ALGO,
                    "the smooth rigid-body JVP runs on DPR_ALGO_ATOMIC and DPR_ALGO_TILED, not algorithm %d", *algo);
    *algo = resolve_algo_smooth_bodies_jvp(*algo, n_out, grid, P, B, V);
    *need = 0;
    if (*algo == DPR_ALGO_TILED) {
        *need = smooth_clouds_tiled_workspace_bytes(n_out, grid, P, B, max_pose_group(flags));
        if (*need == (size_t)-1) return fail(DPR_ERR_UNSUPPORTED_ALGO, kSmoothTiledRefused);
    }
    return DPR_OK;
}

template <typename T>
static int raster_smooth_bodies_jvp_impl(void* stream, int algo, unsigned flags, int n_in, int n_out,
                                         const int64_t* grid, int64_t P, int64_t B, int64_t K, int64_t V, T* out_dot,
                                         const T* points, const int32_t* body, const T* rot, const T* trans,
                                         const T* ow, const T* pw, JvpTangents<T> tan, const T* bg_dot, void* ws,
                                         size_t ws_bytes) {
    int64_t G = 0;
    size_t need = 0;
    if (int rc = check_smooth_bodies_jvp(&algo, flags, n_in, n_out, grid, P, B, K, V, &G, &need)) return rc;
    if (B == 0) return DPR_OK;
    if (!out_dot) return fail(DPR_ERR_INVALID_ARG, "out_dot is NULL");
    if (P > 0 && !points) return fail(DPR_ERR_INVALID_ARG, "points is NULL with P > 0");
    if (P > 0 && !body) return fail(DPR_ERR_INVALID_ARG, "body is NULL with P > 0");
    if (P > 0 && (!rot || !trans)) return fail(DPR_ERR_INVALID_ARG, "rotation/translation is NULL with P > 0");
    if (P > 0 && need > 0 && (!ws || ws_bytes < need))
        return fail(DPR_ERR_WORKSPACE, "smooth rigid bodies JVP (algorithm %d) needs %zu workspace bytes, got %zu",
                    algo, need, ws ? ws_bytes : (size_t)0);
    if (int rc = check_alignment<T>(ws, {out_dot, points, rot, trans, ow, pw, tan.points, tan.rot, tan.trans, tan.ow,
                                         tan.pw, bg_dot}))
        return rc;
    if ((uintptr_t)body & 3) return fail(DPR_ERR_INVALID_ARG, "body is not aligned to its element type (int32_t)");
    hipStream_t st = (hipStream_t)stream;
    stage_mark(st);
    // the background tangent (or 0) into every plane; then the deposits, where any other tangent is given
    jvp_fill(st, out_dot, G, (int)V, B, bg_dot);
    stage_mark(st);
    DPR_HIP(hipGetLastError());
    if (P == 0 || !(tan.points || tan.rot || tan.trans || tan.ow || tan.pw)) return DPR_OK;
    return with_smooth_dims(n_in, n_out, [&](auto ni, auto no) -> int {
        constexpr int NI = decltype(ni)::value, NO = decltype(no)::value;
        const int rc = algo == DPR_ALGO_TILED
                           ? smooth_bodies_jvp_tiled<T, NI, NO>(st, grid, G, P, B, (int)K, (int)V,
                                                                max_pose_group(flags), out_dot, points, body,
                                                                rot, trans, ow, pw, tan, ws, ws_bytes)
                           : smooth_bodies_jvp_atomic<T, NI, NO>(st, grid, G, P, B, (int)K, (int)V, out_dot, points,
                                                                 body, rot, trans, ow, pw, tan);
        stage_mark(st);
        return rc;
    });
}

// ---------------------------------------------------------------- smooth sampling at the points of rigid bodies
// dpr_sample_smooth_bodies_ex_* / dpr_sample_smooth_bodies_pullback_ex_* (include/dpr.h, "SMOOTH SAMPLING, RIGID
// BODIES"; kernels: dpr_sample_smooth_bodies.hip).  Forward: DPR_ALGO_ATOMIC.  Pullback: DPR_ALGO_ATOMIC, the fused
// point kernel with image atomics; DPR_ALGO_TILED, the same kernel without them, then ds_dimage group by group of
// images through the binning of the tiled smooth rigid-body forward.
// AUTO: the forward is ATOMIC; the pullback is TILED exactly where the smooth rigid-body forward of the shape would
// be (resolve_algo_smooth_bodies above; dpr_resolve_algo_sample_smooth's precedent).
static int resolve_algo_sample_smooth_bodies(int algo, int op, int n_out, const int64_t* grid, int64_t P, int64_t B) {
    if (algo != DPR_ALGO_AUTO) return algo;
    if (op != DPR_OP_PULLBACK) return DPR_ALGO_ATOMIC;
    return resolve_algo_smooth_bodies(DPR_ALGO_AUTO, DPR_OP_RASTER, n_out, grid, P, B);
}

// Every refusal of the family, shared by the entry points, the workspace query and
// dpr_resolve_algo_sample_smooth_bodies; *G, the resolved *algo and the workspace bytes *need come back.
static int check_sample_smooth_bodies(int op, int* algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                                      int64_t P, int64_t B, int64_t K, int64_t* G, size_t* need) {
    if (!smooth_dims_supported(n_in, n_out))
        return fail(DPR_ERR_UNSUPPORTED_DIMS,
                    "smooth rigid-body sampling: (n_in, n_out) = (%d, %d); supports (2,2), (3,3), (3,2)", n_in, n_out);
    if (int rc = check_common(n_in, n_out, grid, P, B, G)) return rc;
    if (op != DPR_OP_RASTER && op != DPR_OP_PULLBACK)
        return fail(DPR_ERR_INVALID_ARG, "smooth rigid-body sampling: op %d is not DPR_OP_RASTER / DPR_OP_PULLBACK",
                    op);
    if (K < 1) return fail(DPR_ERR_INVALID_ARG, "K = %lld: a call needs at least one body", (long long)K);
    if (K > 0x7fffffffLL || (B > 0 && K > 0x7fffffffLL / B))  // (check_smooth_bodies' bound, for its reasons)
        return fail(DPR_ERR_INVALID_ARG, "B * K = %lld * %lld poses exceed 2^31 - 1", (long long)B, (long long)K);
    if (int rc = check_point_blocks(P)) return rc;
    if (flags & 3u)
        return fail(DPR_ERR_UNSUPPORTED_ALGO,
                    "smooth rigid-body sampling keeps / reuses no binning (DPR_FLAG_KEEP_BINNING / REUSE_BINNING)");
    if (*algo != DPR_ALGO_AUTO && *algo != DPR_ALGO_ATOMIC && *algo != DPR_ALGO_TILED)
        return fail(DPR_ERR_UNSUPPORTED_ALGO,
                    "smooth rigid-body sampling runs on DPR_ALGO_ATOMIC and, the pullback, DPR_ALGO_TILED, not "
                    "algorithm %d", *algo);
    if (*algo == DPR_ALGO_TILED && op != DPR_OP_PULLBACK)
        return fail(DPR_ERR_UNSUPPORTED_ALGO, "the smooth rigid-body sampling forward runs on DPR_ALGO_ATOMIC only");
    *algo = resolve_algo_sample_smooth_bodies(*algo, op, n_out, grid, P, B);
    if ((flags & 0xff00u) && *algo != DPR_ALGO_TILED)
        return fail(DPR_ERR_UNSUPPORTED_ALGO,
                    "smooth rigid-body sampling forms groups of images on the DPR_ALGO_TILED pullback only "
                    "(DPR_FLAG_MAX_POSE_GROUP)");
    *need = 0;
    if (*algo == DPR_ALGO_TILED) {
        *need = smooth_clouds_tiled_workspace_bytes(n_out, grid, P, B, max_pose_group(flags));
        if (*need == (size_t)-1) return fail(DPR_ERR_UNSUPPORTED_ALGO, kSmoothTiledRefused);
    }
    return check_sample_sizes(P, B, *G);
}

template <typename T>
static int sample_smooth_bodies_impl(void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid,
                                     int64_t P, int64_t B, int64_t K, T* values, const T* image, const T* points,
                                     const int32_t* body, const T* rot, const T* trans, void* ws) {
    int64_t G = 0;
    size_t need = 0;
    if (int rc = check_sample_smooth_bodies(DPR_OP_RASTER, &algo, flags, n_in, n_out, grid, P, B, K, &G, &need))
        return rc;
    if (P == 0 || B == 0) return DPR_OK;
    if (!values) return fail(DPR_ERR_INVALID_ARG, "values is NULL");
    if (!image) return fail(DPR_ERR_INVALID_ARG, "image is NULL");
    if (!points) return fail(DPR_ERR_INVALID_ARG, "points is NULL with P > 0");
    if (!body) return fail(DPR_ERR_INVALID_ARG, "body is NULL with P > 0");
    if (!rot || !trans) return fail(DPR_ERR_INVALID_ARG, "rotation/translation is NULL");
    if (int rc = check_alignment<T>(ws, {values, image, points, rot, trans})) return rc;
    if ((uintptr_t)body & 3) return fail(DPR_ERR_INVALID_ARG, "body is not aligned to its element type (int32_t)");
    hipStream_t st = (hipStream_t)stream;
    stage_mark(st);
    int64_t slices = 1;
    const int pps = pose_slices(P, B, &slices);
    return with_smooth_dims(n_in, n_out, [&](auto ni, auto no) -> int {
        const int rc = sample_smooth_bodies_fwd<T, decltype(ni)::value, decltype(no)::value>(
            st, grid, G, P, B, (int)K, values, image, points, body, rot, trans, pps, slices);
        stage_mark(st);
        return rc;
    });
}

template <typename T>
static int sample_smooth_bodies_pullback_impl(void* stream, int algo, unsigned flags, int n_in, int n_out,
                                              const int64_t* grid, int64_t P, int64_t B, int64_t K, const T* dv,
                                              const T* image, const T* points, const int32_t* body, const T* rot,
                                              const T* trans, T* d_img, T* d_pts, T* d_rot, T* d_trans, void* ws,
                                              size_t ws_bytes) {
    int64_t G = 0;
    size_t need = 0;
    if (int rc = check_sample_smooth_bodies(DPR_OP_PULLBACK, &algo, flags, n_in, n_out, grid, P, B, K, &G, &need))
        return rc;
    if (!d_img && !d_pts && !d_rot && !d_trans)
        return fail(DPR_ERR_INVALID_ARG, "smooth rigid-body sampling pullback: every output is NULL");
    const bool tiled = algo == DPR_ALGO_TILED;
    if (tiled && d_img && P > 0 && B > 0 && need > 0 && (!ws || ws_bytes < need))
        return fail(DPR_ERR_WORKSPACE,
                    "DPR_ALGO_TILED smooth rigid-body sampling pullback needs %zu workspace bytes, got %zu", need,
                    ws ? ws_bytes : (size_t)0);
    if (P > 0 && !points) return fail(DPR_ERR_INVALID_ARG, "points is NULL with P > 0");
    if (P > 0 && !body) return fail(DPR_ERR_INVALID_ARG, "body is NULL with P > 0");
    if (P > 0 && B > 0) {
        if (!dv) return fail(DPR_ERR_INVALID_ARG, "ds_dvalues is NULL");
        if (!rot || !trans) return fail(DPR_ERR_INVALID_ARG, "rotation/translation is NULL");
        if ((d_pts || d_rot || d_trans) && !image)
            return fail(DPR_ERR_INVALID_ARG, "image is NULL (needed for ds_dpoints / ds_drotation / ds_dtranslation)");
    }
    if (int rc = check_alignment<T>(ws, {dv, image, points, rot, trans, d_img, d_pts, d_rot, d_trans})) return rc;
    if ((uintptr_t)body & 3) return fail(DPR_ERR_INVALID_ARG, "body is not aligned to its element type (int32_t)");
    hipStream_t st = (hipStream_t)stream;
    stage_mark(st);
    if (d_rot) DPR_HIP(zero_async(st, d_rot, sizeof(T) * (size_t)(B * K * n_out * n_in)));
    if (d_trans) DPR_HIP(zero_async(st, d_trans, sizeof(T) * (size_t)(B * K * n_out)));
    if (d_img) DPR_HIP(zero_async(st, d_img, sizeof(T) * (size_t)(B * G)));
    if (d_pts && B == 0) DPR_HIP(zero_async(st, d_pts, sizeof(T) * (size_t)(P * n_in)));
    if (P == 0 || B == 0) return DPR_OK;
    int64_t slices = 1;
    const int pps = pose_slices(P, B, &slices);
    return with_smooth_dims(n_in, n_out, [&](auto ni, auto no) -> int {
        constexpr int NI = decltype(ni)::value, NO = decltype(no)::value;
        if (int rc = sample_smooth_bodies_bwd<T, NI, NO>(st, grid, G, P, B, (int)K, dv, image, points, body, rot,
                                                         trans, tiled ? nullptr : d_img, d_pts, d_rot, d_trans, pps,
                                                         slices))
            return rc;
        stage_mark(st);
        if (tiled && d_img)  // (the planes are zeroed above)
            return sample_smooth_bodies_image_tiled<T, NI, NO>(st, grid, G, P, B, (int)K, max_pose_group(flags),
                                                               d_img, dv, points, body, rot, trans, ws, ws_bytes);
        return DPR_OK;
    });
}

}  // namespace dpr

extern "C" {

int dpr_resolve_algo_sample_smooth_bodies(int op, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B,
                                          int64_t K) {
    int64_t G = 0;
    size_t need = 0;
    int algo = DPR_ALGO_AUTO;
    if (int rc = dpr::check_sample_smooth_bodies(op, &algo, 0u, n_in, n_out, grid, P, B, K, &G, &need)) return rc;
    return algo;
}

#define DPR_DEFINE_SAMPLE_SMOOTH_BODIES(SUF, T)                                                                     \
    size_t dpr_workspace_bytes_sample_smooth_bodies_ex_##SUF(int op, int algo, unsigned flags, int n_in, int n_out, \
                                                             const int64_t* grid, int64_t P, int64_t B,             \
                                                             int64_t K) {                                           \
        int64_t G = 0;                                                                                              \
        size_t need = 0;                                                                                            \
        return dpr::check_sample_smooth_bodies(op, &algo, flags, n_in, n_out, grid, P, B, K, &G, &need)             \
                   ? (size_t)-1                                                                                     \
                   : need;                                                                                          \
    }                                                                                                               \
    int dpr_sample_smooth_bodies_ex_##SUF(void* stream, int algo, unsigned flags, int n_in, int n_out,              \
                                          const int64_t* grid, int64_t P, int64_t B, int64_t K, T* values,          \
                                          const T* image, const T* points, const void* body, const T* rotation,     \
                                          const T* translation, void* workspace, size_t workspace_bytes) {          \
        (void)workspace_bytes;                                                                                      \
        return dpr::sample_smooth_bodies_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B, K, values, image,    \
                                                 points, (const int32_t*)body, rotation, translation, workspace);   \
    }                                                                                                               \
    int dpr_sample_smooth_bodies_pullback_ex_##SUF(                                                                 \
        void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B,     \
        int64_t K, const T* ds_dvalues, const T* image, const T* points, const void* body, const T* rotation,       \
        const T* translation, T* ds_dimage, T* ds_dpoints, T* ds_drotation, T* ds_dtranslation, void* workspace,    \
        size_t workspace_bytes) {                                                                                   \
        return dpr::sample_smooth_bodies_pullback_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B, K,          \
                                                          ds_dvalues, image, points, (const int32_t*)body,          \
                                                          rotation, translation, ds_dimage, ds_dpoints,             \
                                                          ds_drotation, ds_dtranslation, workspace,                 \
                                                          workspace_bytes);                                         \
    }
DPR_DEFINE_SAMPLE_SMOOTH_BODIES(f32, float)
DPR_DEFINE_SAMPLE_SMOOTH_BODIES(f64, double)
#undef DPR_DEFINE_SAMPLE_SMOOTH_BODIES

int dpr_resolve_algo_smooth_bodies(int op, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B,
                                   int64_t K) {
    int64_t G = 0;
    size_t need = 0;
    int algo = DPR_ALGO_AUTO;
    if (int rc = dpr::check_smooth_bodies(op, &algo, 0u, n_in, n_out, grid, P, B, K, &G, &need)) return rc;
    return algo;
}

#define DPR_DEFINE_SMOOTH_BODIES(SUF, T)                                                                          \
    size_t dpr_workspace_bytes_smooth_bodies_ex_##SUF(int op, int algo, unsigned flags, int n_in, int n_out,      \
                                                      const int64_t* grid, int64_t P, int64_t B, int64_t K) {     \
        int64_t G = 0;                                                                                            \
        size_t need = 0;                                                                                          \
        return dpr::check_smooth_bodies(op, &algo, flags, n_in, n_out, grid, P, B, K, &G, &need) ? (size_t)-1     \
                                                                                                  : need;         \
    }                                                                                                             \
    int dpr_raster_smooth_bodies_ex_##SUF(void* stream, int algo, unsigned flags, int n_in, int n_out,            \
                                          const int64_t* grid, int64_t P, int64_t B, int64_t K, T* out,           \
                                          const T* points, const void* body, const T* rotation,                   \
                                          const T* translation, const T* background, const T* out_weight,         \
                                          const T* point_weight, void* workspace, size_t workspace_bytes) {       \
        return dpr::raster_smooth_bodies_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B, K, out, points,    \
                                                 (const int32_t*)body, rotation, translation, background,         \
                                                 out_weight, point_weight, workspace, workspace_bytes);           \
    }                                                                                                             \
    int dpr_raster_pullback_smooth_bodies_ex_##SUF(                                                               \
        void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B,   \
        int64_t K, const T* ds_dout, const T* points, const void* body, const T* rotation, const T* translation,  \
        const T* out_weight, const T* point_weight, T* ds_dpoints, T* ds_drotation, T* ds_dtranslation,           \
        T* ds_dbackground, T* ds_dout_weight, T* ds_dpoint_weight, void* workspace, size_t workspace_bytes) {     \
        (void)workspace_bytes;                                                                                    \
        return dpr::pullback_smooth_bodies_impl<T>(stream, algo, flags, n_in, n_out, grid, P, B, K, ds_dout,      \
                                                   points, (const int32_t*)body, rotation, translation,           \
                                                   out_weight, point_weight, ds_dpoints, ds_drotation,            \
                                                   ds_dtranslation, ds_dbackground, ds_dout_weight,               \
                                                   ds_dpoint_weight, workspace);                                  \
    }
DPR_DEFINE_SMOOTH_BODIES(f32, float)
DPR_DEFINE_SMOOTH_BODIES(f64, double)
#undef DPR_DEFINE_SMOOTH_BODIES

int dpr_resolve_algo_smooth_bodies_jvp(int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B, int64_t K,
                                       int64_t V) {
    int64_t G = 0;
    size_t need = 0;
    int algo = DPR_ALGO_AUTO;
    if (int rc = dpr::check_smooth_bodies_jvp(&algo, 0u, n_in, n_out, grid, P, B, K, V, &G, &need)) return rc;
    return algo;
}

#define DPR_DEFINE_SMOOTH_BODIES_JVP(SUF, T)                                                                      \
    size_t dpr_workspace_bytes_smooth_bodies_jvp_ex_##SUF(int algo, unsigned flags, int n_in, int n_out,          \
                                                          const int64_t* grid, int64_t P, int64_t B, int64_t K,   \
                                                          int64_t V) {                                            \
        int64_t G = 0;                                                                                            \
        size_t need = 0;                                                                                          \
        return dpr::check_smooth_bodies_jvp(&algo, flags, n_in, n_out, grid, P, B, K, V, &G, &need) ? (size_t)-1  \
                                                                                                     : need;      \
    }                                                                                                             \
    int dpr_raster_smooth_bodies_jvp_ex_##SUF(                                                                    \
        void* stream, int algo, unsigned flags, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B,   \
        int64_t K, int64_t V, T* out_dot, const T* points, const void* body, const T* rotation,                   \
        const T* translation, const T* out_weight, const T* point_weight, const T* points_dot,                    \
        const T* rotation_dot, const T* translation_dot, const T* background_dot, const T* out_weight_dot,        \
        const T* point_weight_dot, void* workspace, size_t workspace_bytes) {                                     \
        return dpr::raster_smooth_bodies_jvp_impl<T>(                                                             \
            stream, algo, flags, n_in, n_out, grid, P, B, K, V, out_dot, points, (const int32_t*)body, rotation,  \
            translation, out_weight, point_weight,                                                                \
            dpr::JvpTangents<T>{points_dot, rotation_dot, translation_dot, out_weight_dot, point_weight_dot},     \
            background_dot, workspace, workspace_bytes);                                                          \
    }
DPR_DEFINE_SMOOTH_BODIES_JVP(f32, float)
DPR_DEFINE_SMOOTH_BODIES_JVP(f64, double)
#undef DPR_DEFINE_SMOOTH_BODIES_JVP

}  // extern "C"
