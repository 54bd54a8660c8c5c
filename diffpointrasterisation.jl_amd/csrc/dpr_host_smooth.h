// The host side of a call that the smooth op families share (dpr_api_smooth.hip, dpr_api_smooth_bodies.hip): what a
// family is (SmoothFamily), the one funnel of refusals behind every entry point, workspace query and AUTO resolver
// (smooth_checks), the pointer checks, the stream prologues and the skeletons of the entry points.  No kernel and no
// launch: the launchers of dpr_smooth.h are handed in as generic lambdas.
//
// THE ORDER OF REFUSALS, for every family and for entry point, query and resolver alike:
//   1. the pair (n_in, n_out) -- before the grid is looked at
//   2. check_common: grid, P, B
//   3. op
//   4. the family's extent: C; K and B * K; the tangent count
//   5. the family's 64-bit size bounds
//   6. flags: KEEP / REUSE, then DPR_FLAG_MAX_POSE_GROUP where the op refuses it
//   7. the algorithm: one of AUTO, ATOMIC, TILED, and TILED on the op that has it
//   8. AUTO becomes the family's choice; DPR_FLAG_MAX_POSE_GROUP where only a TILED call takes it
//   9. the workspace need of DPR_ALGO_TILED
// then, in the entry points alone, the pointers: outputs, points, body, poses, the rest, workspace, alignment.
#pragma once
#include "dpr_host.h"
#include "dpr_smooth.h"

namespace dpr {

enum SmoothTiledOp { kTiledForward, kTiledPullback, kTiledOnlyOp };  // (kTiledOnlyOp: the family has no `op`)
// DPR_FLAG_MAX_POSE_GROUP: no meaning and ignored / sizes the groups of the TILED op, ignored on ATOMIC and refused
// on the other op / sizes the groups of a TILED call and is refused on every other
enum SmoothGroupFlag { kGroupIgnored, kGroupRefusedOffTiledOp, kGroupRefusedOffTiled };

struct SmoothFamily {
    const char* name;      // the noun phrase every message starts with
    SmoothTiledOp tiled_op;
    bool residual_refusal;  // DPR_OP_RESIDUAL_PULLBACK is DPR_ERR_UNSUPPORTED_ALGO (a splat), not an unknown op
    bool group_plan;        // workspace: smooth_clouds_tiled_workspace_bytes with max_pose_group(flags), not the
                            // single-pose smooth_tiled_workspace_bytes
    SmoothGroupFlag group_flag;
    bool has_body;              // rigid bodies: a `body` pointer, and pose pointers that P == 0 leaves unread
    bool needs_point_weight;    // point_weight may not be NULL (C weights per point)
    bool pullback_slices_poses; // the splat pullback takes pose_slices and has nothing to launch for P == 0
    bool per_pose_clouds = false;  // sampling: ds_dpoints holds B clouds, each entry stored by its own (point, pose)
};

// what the funnel hands back: the status, voxels per pose, the resolved algorithm, the workspace bytes
struct SmoothCall {
    int rc;
    int64_t G;
    int algo;
    size_t need;
};
inline size_t query_value(const SmoothCall& c) { return c.rc ? (size_t)-1 : c.need; }
inline int resolver_value(const SmoothCall& c) { return c.rc ? c.rc : c.algo; }

// ---------------------------------------------------------------- the funnel
// extent() and sizes(G) return a status; auto_rule() returns DPR_ALGO_ATOMIC or DPR_ALGO_TILED, the latter only for
// the family's tiled op.  A family without `op` passes DPR_OP_RASTER.
template <class Extent, class Sizes, class Auto>
SmoothCall smooth_checks(const SmoothFamily& fam, int op, int algo, unsigned flags, int n_in, int n_out,
                         const int64_t* grid, int64_t P, int64_t B, Extent&& extent, Sizes&& sizes, Auto&& auto_rule) {
    SmoothCall c{DPR_OK, 0, algo, 0};
    const auto refuse = [&](int rc) {
        c.rc = rc;
        return c;
    };
    if (!smooth_dims_supported(n_in, n_out))
        return refuse(fail(DPR_ERR_UNSUPPORTED_DIMS,
                           "%s: unsupported (n_in, n_out) = (%d, %d); supports (2,2), (3,3), (3,2)", fam.name, n_in,
                           n_out));
    if (int rc = check_common(n_in, n_out, grid, P, B, &c.G)) return refuse(rc);
    const bool has_op = fam.tiled_op != kTiledOnlyOp;
    if (has_op && op == DPR_OP_RESIDUAL_PULLBACK && fam.residual_refusal)
        return refuse(fail(DPR_ERR_UNSUPPORTED_ALGO, "%s: no residual pullback", fam.name));
    if (has_op && op != DPR_OP_RASTER && op != DPR_OP_PULLBACK)
        return refuse(fail(DPR_ERR_INVALID_ARG, "%s: op %d is not DPR_OP_RASTER / DPR_OP_PULLBACK", fam.name, op));
    if (int rc = extent()) return refuse(rc);
    if (int rc = sizes(c.G)) return refuse(rc);
    if (flags & 3u)
        return refuse(fail(DPR_ERR_UNSUPPORTED_ALGO,
                           "%s: no binning is kept or reused (DPR_FLAG_KEEP_BINNING / REUSE_BINNING)", fam.name));
    const bool tiled_op = !has_op || op == (fam.tiled_op == kTiledForward ? DPR_OP_RASTER : DPR_OP_PULLBACK);
    const char* const other_op = fam.tiled_op == kTiledForward ? "pullback" : "forward";
    if ((flags & 0xff00u) && fam.group_flag == kGroupRefusedOffTiledOp && !tiled_op)
        return refuse(fail(DPR_ERR_UNSUPPORTED_ALGO, "%s: the %s forms no groups of images (DPR_FLAG_MAX_POSE_GROUP)",
                           fam.name, other_op));
    if (algo != DPR_ALGO_AUTO && algo != DPR_ALGO_ATOMIC && algo != DPR_ALGO_TILED)
        return refuse(fail(DPR_ERR_UNSUPPORTED_ALGO, "%s: DPR_ALGO_ATOMIC and DPR_ALGO_TILED only, not algorithm %d",
                           fam.name, algo));
    if (algo == DPR_ALGO_TILED && !tiled_op)
        return refuse(fail(DPR_ERR_UNSUPPORTED_ALGO, "%s: the %s runs on DPR_ALGO_ATOMIC only", fam.name, other_op));
    if (algo == DPR_ALGO_AUTO) c.algo = auto_rule();
    if ((flags & 0xff00u) && fam.group_flag == kGroupRefusedOffTiled && c.algo != DPR_ALGO_TILED)
        return refuse(fail(DPR_ERR_UNSUPPORTED_ALGO,
                           "%s: groups of images are formed on the DPR_ALGO_TILED %s only (DPR_FLAG_MAX_POSE_GROUP)",
                           fam.name, fam.tiled_op == kTiledForward ? "forward" : "pullback"));
    if (c.algo == DPR_ALGO_TILED) {  // (ATOMIC: none -- the pullbacks' per-pose partials leave their block as atomics)
        c.need = fam.group_plan ? smooth_clouds_tiled_workspace_bytes(n_out, grid, P, B, max_pose_group(flags))
                                : smooth_tiled_workspace_bytes(n_out, grid, P);
        if (c.need == (size_t)-1) return refuse(fail(DPR_ERR_UNSUPPORTED_ALGO, kSmoothTiledRefused));
    }
    return c;
}

// the extents and size bounds that more than one family has
inline int check_channel_count(int64_t C) {
    if (C < 1 || C > kMaxChannels)
        return fail(DPR_ERR_INVALID_ARG, "channels C = %lld out of range [1, %d]", (long long)C, kMaxChannels);
    return DPR_OK;
}
inline int check_body_count(int64_t B, int64_t K) {
    if (K < 1) return fail(DPR_ERR_INVALID_ARG, "K = %lld: a call needs at least one body", (long long)K);
    // the kernels compare a body index with K as 32-bit values and count poses b * K + k in 64 bits; the zeroing of
    // the B * K pose gradients and their offsets stay far inside both with this bound
    if (K > 0x7fffffffLL || (B > 0 && K > 0x7fffffffLL / B))
        return fail(DPR_ERR_INVALID_ARG, "B * K = %lld * %lld poses exceed 2^31 - 1", (long long)B, (long long)K);
    return DPR_OK;
}
// (planes per pose: C channels or the tangents of a JVP)
inline int check_plane_offsets(int64_t G, int64_t planes_per_pose, int64_t B) {
    if (B > 0 && G * planes_per_pose > ((int64_t)1 << 62) / B) return fail(DPR_ERR_INVALID_ARG, "output too large");
    return DPR_OK;
}

// ---------------------------------------------------------------- pointer checks
inline int check_smooth_workspace(const SmoothFamily& fam, const SmoothCall& c, bool used, const void* ws,
                                  size_t ws_bytes) {
    if (used && c.need > 0 && (!ws || ws_bytes < c.need))
        return fail(DPR_ERR_WORKSPACE, "%s (algorithm %d) needs %zu workspace bytes, got %zu", fam.name, c.algo,
                    c.need, ws ? ws_bytes : (size_t)0);
    return DPR_OK;
}
// the primal inputs of a splat or a JVP: read where there are points; the splat of one cloud asks for the poses anyway
template <typename T>
int check_primal_ptrs(const SmoothFamily& fam, int64_t P, const T* points, const int32_t* body, const T* rot,
                      const T* trans, const T* pw) {
    if (P > 0 && !points) return fail(DPR_ERR_INVALID_ARG, "%s: points is NULL with P > 0", fam.name);
    if (P > 0 && fam.has_body && !body) return fail(DPR_ERR_INVALID_ARG, "%s: body is NULL with P > 0", fam.name);
    if ((P > 0 || !fam.has_body) && (!rot || !trans))
        return fail(DPR_ERR_INVALID_ARG, "%s: rotation/translation is NULL", fam.name);
    if (P > 0 && fam.needs_point_weight && !pw)
        return fail(DPR_ERR_INVALID_ARG, "%s: point_weight is NULL with P > 0 (the channel form needs it)", fam.name);
    return DPR_OK;
}

template <typename T>
int check_splat_forward_ptrs(const SmoothFamily& fam, const SmoothCall& c, int64_t P, const T* out, const T* points,
                             const int32_t* body, const T* rot, const T* trans, const T* bg, const T* ow, const T* pw,
                             const void* ws, size_t ws_bytes) {
    if (!out) return fail(DPR_ERR_INVALID_ARG, "%s: out is NULL", fam.name);
    if (int rc = check_primal_ptrs(fam, P, points, body, rot, trans, pw)) return rc;
    if (int rc = check_smooth_workspace(fam, c, P > 0, ws, ws_bytes)) return rc;
    if (int rc = check_alignment<T>(ws, {out, points, rot, trans, bg, ow, pw})) return rc;
    return check_body_alignment(body);
}

// (d_pw: already NULL under DPR_FLAG_NO_POINT_WEIGHT_GRAD.  B == 0 comes here from the rigid bodies alone, whose
// per-point gradients are written then too)
template <typename T>
int check_splat_pullback_ptrs(const SmoothFamily& fam, unsigned flags, int64_t P, int64_t B, const T* g,
                              const T* points, const int32_t* body, const T* rot, const T* trans, const T* ow,
                              const T* pw, const T* d_pts, const T* d_rot, const T* d_trans, const T* d_bg,
                              const T* d_ow, const T* d_pw, const void* ws) {
    if (P > 0 && (!d_pts || (!d_pw && !(flags & DPR_FLAG_NO_POINT_WEIGHT_GRAD))))
        return fail(DPR_ERR_INVALID_ARG, "%s: ds_dpoints/ds_dpoint_weight is NULL with P > 0", fam.name);
    if (B > 0) {
        if (!g) return fail(DPR_ERR_INVALID_ARG, "%s: ds_dout is NULL", fam.name);
        if (!d_rot || !d_trans || !d_bg || !d_ow)
            return fail(DPR_ERR_INVALID_ARG, "%s: a per-pose output pointer is NULL", fam.name);
        if (int rc = check_primal_ptrs(fam, P, points, body, rot, trans, pw)) return rc;
    }
    if (int rc = check_alignment<T>(ws, {g, points, rot, trans, ow, pw, d_pts, d_rot, d_trans, d_bg, d_ow, d_pw}))
        return rc;
    return check_body_alignment(body);
}

// (called with P > 0 and B > 0)
template <typename T>
int check_sample_forward_ptrs(const SmoothFamily& fam, const T* values, const T* image, const T* points,
                              const int32_t* body, const T* rot, const T* trans, const void* ws) {
    if (!values) return fail(DPR_ERR_INVALID_ARG, "%s: values is NULL", fam.name);
    if (!image) return fail(DPR_ERR_INVALID_ARG, "%s: image is NULL", fam.name);
    if (int rc = check_primal_ptrs<T>(fam, 1, points, body, rot, trans, nullptr)) return rc;
    if (int rc = check_alignment<T>(ws, {values, image, points, rot, trans})) return rc;
    return check_body_alignment(body);
}

// any of the four outputs may be NULL, not all; the workspace serves ds_dimage alone; `image` is read for the
// point and pose gradients alone
template <typename T>
int check_sample_pullback_ptrs(const SmoothFamily& fam, const SmoothCall& c, int64_t P, int64_t B, const T* dv,
                               const T* image, const T* points, const int32_t* body, const T* rot, const T* trans,
                               const T* d_img, const T* d_pts, const T* d_rot, const T* d_trans, const void* ws,
                               size_t ws_bytes) {
    if (!d_img && !d_pts && !d_rot && !d_trans)
        return fail(DPR_ERR_INVALID_ARG, "%s pullback: every output is NULL", fam.name);
    if (int rc = check_smooth_workspace(fam, c, d_img && P > 0 && B > 0, ws, ws_bytes)) return rc;
    if (P > 0 && !points) return fail(DPR_ERR_INVALID_ARG, "%s: points is NULL with P > 0", fam.name);
    if (P > 0 && fam.has_body && !body) return fail(DPR_ERR_INVALID_ARG, "%s: body is NULL with P > 0", fam.name);
    if (P > 0 && B > 0) {
        if (!dv) return fail(DPR_ERR_INVALID_ARG, "%s: ds_dvalues is NULL", fam.name);
        if (!rot || !trans) return fail(DPR_ERR_INVALID_ARG, "%s: rotation/translation is NULL", fam.name);
        if ((d_pts || d_rot || d_trans) && !image)
            return fail(DPR_ERR_INVALID_ARG,
                        "%s: image is NULL (needed for ds_dpoints / ds_drotation / ds_dtranslation)", fam.name);
    }
    if (int rc = check_alignment<T>(ws, {dv, image, points, rot, trans, d_img, d_pts, d_rot, d_trans})) return rc;
    return check_body_alignment(body);
}

template <typename T>
int check_jvp_ptrs(const SmoothFamily& fam, const SmoothCall& c, int64_t P, const T* out_dot, const T* points,
                   const int32_t* body, const T* rot, const T* trans, const T* ow, const T* pw,
                   const JvpTangents<T>& tan, const T* bg_dot, const void* ws, size_t ws_bytes) {
    if (!out_dot) return fail(DPR_ERR_INVALID_ARG, "%s: out_dot is NULL", fam.name);
    if (int rc = check_primal_ptrs(fam, P, points, body, rot, trans, pw)) return rc;
    if (int rc = check_smooth_workspace(fam, c, P > 0, ws, ws_bytes)) return rc;
    if (int rc = check_alignment<T>(ws, {out_dot, points, rot, trans, ow, pw, tan.points, tan.rot, tan.trans, tan.ow,
                                         tan.pw, bg_dot}))
        return rc;
    return check_body_alignment(body);
}

// ---------------------------------------------------------------- stream prologues
// `planes` images of G cells (B, or B * C with channels), `poses` poses (B, or B * K with rigid bodies)
template <typename T>
void smooth_forward_prologue(hipStream_t st, T* out, int64_t G, int64_t planes, const T* bg) {
    stage_mark(st);
    fill_background(st, out, G, planes, bg);
    stage_mark(st);
}

// the per-pose sums start at zero; ds_dbackground[k] = sum of plane k is done here
template <typename T>
int smooth_pullback_prologue(hipStream_t st, int n_in, int n_out, int64_t G, int64_t B, int64_t planes, int64_t poses,
                             const T* g, T* d_rot, T* d_trans, T* d_bg, T* d_ow) {
    stage_mark(st);
    DPR_HIP(zero_async(st, d_rot, sizeof(T) * (size_t)(poses * n_out * n_in)));
    DPR_HIP(zero_async(st, d_trans, sizeof(T) * (size_t)(poses * n_out)));
    DPR_HIP(zero_async(st, d_ow, sizeof(T) * (size_t)B));
    DPR_HIP(zero_async(st, d_bg, sizeof(T) * (size_t)planes));
    grid_sum(st, g, G, planes, d_bg, Residual<T>{nullptr, T(0), nullptr});
    stage_mark(st);
    return DPR_OK;
}

// the outputs that are wanted start at zero; ds_dpoints here only where no pose adds to it
template <typename T>
int sample_pullback_prologue(hipStream_t st, int n_in, int n_out, int64_t G, int64_t P, int64_t B, int64_t planes,
                             int64_t poses, T* d_img, T* d_pts, T* d_rot, T* d_trans) {
    stage_mark(st);
    if (d_rot) DPR_HIP(zero_async(st, d_rot, sizeof(T) * (size_t)(poses * n_out * n_in)));
    if (d_trans) DPR_HIP(zero_async(st, d_trans, sizeof(T) * (size_t)(poses * n_out)));
    if (d_img) DPR_HIP(zero_async(st, d_img, sizeof(T) * (size_t)(planes * G)));
    if (d_pts && B == 0) DPR_HIP(zero_async(st, d_pts, sizeof(T) * (size_t)(P * n_in)));
    return DPR_OK;
}

// the background tangent (or 0) into every plane
template <typename T>
int smooth_jvp_prologue(hipStream_t st, T* out_dot, int64_t G, int V, int64_t B, const T* bg_dot) {
    stage_mark(st);
    jvp_fill(st, out_dot, G, V, B, bg_dot);
    stage_mark(st);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

// ---------------------------------------------------------------- entry points
// What an entry point does after the funnel (c).  The family's launch is a generic lambda that gets the stream and
// the pair as std::integral_constant values; body is NULL in the families without one.
// launch(st, ni, no): the ATOMIC or TILED forward, onto `out` that holds the backgrounds.
template <typename T, class Launch>
int smooth_splat_forward(const SmoothFamily& fam, const SmoothCall& c, void* stream, int n_in, int n_out, int64_t P,
                         int64_t B, int64_t planes, T* out, const T* points, const int32_t* body, const T* rot,
                         const T* trans, const T* bg, const T* ow, const T* pw, void* ws, size_t ws_bytes,
                         Launch&& launch) {
    if (c.rc) return c.rc;
    if (B == 0) return DPR_OK;
    if (int rc = check_splat_forward_ptrs(fam, c, P, out, points, body, rot, trans, bg, ow, pw, ws, ws_bytes))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    smooth_forward_prologue(st, out, c.G, planes, bg);
    return with_smooth_dims(n_in, n_out, [&](auto ni, auto no) -> int {
        const int rc = launch(st, ni, no);
        stage_mark(st);
        return rc;
    });
}

// launch(st, ni, no, poses_per_slice, slices): the ATOMIC pullback; the slicing is pose_slices' (the linear atomic
// pullback's: SUMMATION ORDER, note 1) where the family slices, (0, 1) where it does not.  d_pw: NULL under
// DPR_FLAG_NO_POINT_WEIGHT_GRAD.
template <typename T, class Launch>
int smooth_splat_pullback(const SmoothFamily& fam, const SmoothCall& c, void* stream, unsigned flags, int n_in,
                          int n_out, int64_t P, int64_t B, int64_t planes, int64_t poses, const T* g, const T* points,
                          const int32_t* body, const T* rot, const T* trans, const T* ow, const T* pw, T* d_pts,
                          T* d_rot, T* d_trans, T* d_bg, T* d_ow, T* d_pw, void* ws, Launch&& launch) {
    if (c.rc) return c.rc;
    if (B == 0 && !fam.has_body) return DPR_OK;  // (every output is empty, or left as it is)
    if (int rc = check_splat_pullback_ptrs(fam, flags, P, B, g, points, body, rot, trans, ow, pw, d_pts, d_rot,
                                           d_trans, d_bg, d_ow, d_pw, ws))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) {  // rigid bodies without an image: the sums over the images are empty
        stage_mark(st);
        if (P > 0) {
            DPR_HIP(zero_async(st, d_pts, sizeof(T) * (size_t)(P * n_in)));
            if (d_pw) DPR_HIP(zero_async(st, d_pw, sizeof(T) * (size_t)P));
        }
        return DPR_OK;
    }
    if (int rc = smooth_pullback_prologue(st, n_in, n_out, c.G, B, planes, poses, g, d_rot, d_trans, d_bg, d_ow))
        return rc;
    int64_t slices = 1;
    int poses_per_slice = 0;
    if (fam.pullback_slices_poses) {
        // (without points the per-pose sums are 0 and ds_dbackground is done; pose_slices divides by the blocks)
        if (P == 0) return DPR_OK;
        poses_per_slice = pose_slices(P, B, &slices);
    }
    return with_smooth_dims(n_in, n_out, [&](auto ni, auto no) -> int {
        const int rc = launch(st, ni, no, poses_per_slice, slices);
        stage_mark(st);
        return rc;
    });
}

// launch(st, ni, no, poses_per_slice, slices): the one kernel of the forward
template <typename T, class Launch>
int smooth_sample_forward(const SmoothFamily& fam, const SmoothCall& c, void* stream, int n_in, int n_out, int64_t P,
                          int64_t B, const T* values, const T* image, const T* points, const int32_t* body,
                          const T* rot, const T* trans, void* ws, Launch&& launch) {
    if (c.rc) return c.rc;
    if (P == 0 || B == 0) return DPR_OK;
    if (int rc = check_sample_forward_ptrs(fam, values, image, points, body, rot, trans, ws)) return rc;
    hipStream_t st = (hipStream_t)stream;
    stage_mark(st);
    int64_t slices = 1;
    const int poses_per_slice = pose_slices(P, B, &slices);
    return with_smooth_dims(n_in, n_out, [&](auto ni, auto no) -> int {
        const int rc = launch(st, ni, no, poses_per_slice, slices);
        stage_mark(st);
        return rc;
    });
}

// points_launch(st, ni, no, d_img, poses_per_slice, slices): the fused point kernel, with image atomics (ATOMIC) or
// with d_img = NULL (TILED); image_launch(st, ni, no): ds_dimage of a TILED call, onto the planes zeroed here, from
// the family's tiled forward
template <typename T, class PointsLaunch, class ImageLaunch>
int smooth_sample_pullback(const SmoothFamily& fam, const SmoothCall& c, void* stream, int n_in, int n_out, int64_t P,
                           int64_t B, int64_t planes, int64_t poses, const T* dv, const T* image, const T* points,
                           const int32_t* body, const T* rot, const T* trans, T* d_img, T* d_pts, T* d_rot,
                           T* d_trans, void* ws, size_t ws_bytes, PointsLaunch&& points_launch,
                           ImageLaunch&& image_launch) {
    if (c.rc) return c.rc;
    if (int rc = check_sample_pullback_ptrs(fam, c, P, B, dv, image, points, body, rot, trans, d_img, d_pts, d_rot,
                                            d_trans, ws, ws_bytes))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    // (per-pose clouds: ds_dpoints is empty with B == 0, so nothing of it is zeroed)
    if (int rc = sample_pullback_prologue(st, n_in, n_out, c.G, fam.per_pose_clouds ? 0 : P, B, planes, poses, d_img,
                                          d_pts, d_rot, d_trans))
        return rc;
    if (P == 0 || B == 0) return DPR_OK;
    const bool tiled = c.algo == DPR_ALGO_TILED;
    int64_t slices = 1;
    const int poses_per_slice = pose_slices(P, B, &slices);
    return with_smooth_dims(n_in, n_out, [&](auto ni, auto no) -> int {
        if (int rc = points_launch(st, ni, no, tiled ? nullptr : d_img, poses_per_slice, slices)) return rc;
        stage_mark(st);
        return tiled && d_img ? image_launch(st, ni, no) : DPR_OK;
    });
}

// launch(st, ni, no): the deposits of the tangents, ATOMIC or TILED, onto the planes the prologue filled; skipped
// where only the background has a tangent
template <typename T, class Launch>
int smooth_jvp_forward(const SmoothFamily& fam, const SmoothCall& c, void* stream, int n_in, int n_out, int64_t P,
                       int64_t B, int64_t V, T* out_dot, const T* points, const int32_t* body, const T* rot,
                       const T* trans, const T* ow, const T* pw, const JvpTangents<T>& tan, const T* bg_dot, void* ws,
                       size_t ws_bytes, Launch&& launch) {
    if (c.rc) return c.rc;
    if (B == 0) return DPR_OK;
    if (int rc = check_jvp_ptrs(fam, c, P, out_dot, points, body, rot, trans, ow, pw, tan, bg_dot, ws, ws_bytes))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = smooth_jvp_prologue(st, out_dot, c.G, (int)V, B, bg_dot)) return rc;
    if (P == 0 || !(tan.points || tan.rot || tan.trans || tan.ow || tan.pw)) return DPR_OK;
    return with_smooth_dims(n_in, n_out, [&](auto ni, auto no) -> int {
        const int rc = launch(st, ni, no);
        stage_mark(st);
        return rc;
    });
}

}  // namespace dpr
