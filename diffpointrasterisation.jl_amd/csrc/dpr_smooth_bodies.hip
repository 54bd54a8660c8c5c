// The smooth splat of rigid bodies (include/dpr.h, "SMOOTH SPLAT, RIGID BODIES"): RIGID BODIES with the quadratic
// B-spline weights of SMOOTH SPLAT.  Point p belongs to body[p] in [0, K) and is seen in image b through pose
// b * K + body[p]; the kernels of the family and their launches (declared in dpr_smooth.h; host checks, AUTO rules and
// the C ABI: dpr_api_smooth_bodies.hip).
//
//   DPR_ALGO_ATOMIC forward   k_smooth_bodies_fwd_atomic: k_smooth_fwd_atomic with the pose of wave_bodies /
//                             load_body_pose (dpr_kernels_bodies.h): scalar loads where a wave's accepted lanes share
//                             a body, a per-lane gather otherwise
//   DPR_ALGO_ATOMIC pullback  k_smooth_bodies_bwd: k_bodies_bwd's per-(image, body) reduction around the point term of
//                             k_smooth_bwd (smooth_point_backward, the same operation order)
//   DPR_ALGO_TILED forward    the images binned in GROUPS as smooth_clouds_fwd_tiled bins poses: k_smooth_bodies_keys
//                             (key = b_local * tiles + tile, value = b_local * P + p) -> smooth_sort_group (one stable
//                             radix sort, k_smooth_ranges) -> k_smooth_bodies_tile, one workgroup per (image, tile),
//                             which takes p = q - b_local * P, checks body[p] and gathers its pose per lane
//   forward mode              (include/dpr.h, "SMOOTH SPLAT, RIGID BODIES, FORWARD MODE") jvp_fill, then
//                             k_smooth_bodies_jvp_atomic, or the binning above once per group of images and
//                             k_smooth_bodies_tile_jvp, one workgroup per (image, tile, tangent)
// These are copies of the smooth and the rigid-body kernels, not shared bodies: those kernels keep their registers.
// A body index outside [0, K) is checked per lane before it addresses a pose, in every kernel.
#include <hip/hip_runtime.h>

#include "../../include/dpr.h"
#include "dpr_jvp.h"
#include "dpr_kernels_bodies.h"
#include "dpr_ordered.h"
#include "dpr_ordered_index.h"
#include "dpr_smooth.h"
#include "dpr_smooth_device.h"

namespace dpr {

static_assert(kSmBlock == kBlock, "pose_slices and the P bound of the host checks count blocks of kBlock points");

// ---------------------------------------------------------------- DPR_ALGO_ATOMIC forward
// One thread per point, the images striding over blockIdx.y.  `out` holds the background.
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kSmBlock) void k_smooth_bodies_fwd_atomic(
    GridDesc<NO> gd, int64_t P, int64_t B, int K, T* __restrict__ out, const T* __restrict__ points,
    const int32_t* __restrict__ body, const T* __restrict__ rot, const T* __restrict__ trans,
    const T* __restrict__ ow, const T* __restrict__ pw) {
    static_assert(NO == 2 || NO == 3, "the smooth splat is written for 2-D and 3-D grids");
    const int64_t p = (int64_t)blockIdx.x * kSmBlock + threadIdx.x;
    const WaveBodies wb = wave_bodies(body, p, P, K);
    if (wb.distinct == 0) return;  // (the whole wave: no lane has a point to deposit)
    T pt[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) pt[j] = T(0);
    if (wb.ok) load_point<T, NI>(points, p, pt);
    const T pwi = (wb.ok && pw) ? pw[p] : T(1);
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        const Pose<T, NI, NO> ps = load_body_pose<T, NI, NO>(rot, trans, ow, b, K, wb);
        int j0[NO];
        T u[NO];
        if (!(wb.ok && smooth_cell<T, NI, NO>(pt, ps, gd, j0, u))) continue;
        const T w = ps.ow * pwi;  // as k_smooth_fwd_atomic
        const SmoothAxes<T, NO> ax = smooth_axes<T, NO>(j0, u, gd);
        T* o = out + b * gd.G;
#pragma unroll
        for (int k2 = 0; k2 < (NO == 3 ? 3 : 1); ++k2) {
            const bool in2 = NO == 3 ? ax.in[NO - 1][k2] : true;
            const int off2 = NO == 3 ? ax.off[NO - 1][k2] : 0;
            const T w2 = NO == 3 ? ax.w[NO - 1][k2] * w : w;
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
}

// ---------------------------------------------------------------- DPR_ALGO_ATOMIC pullback
// Over the image range [b_lo, b_hi) of blockIdx.y.  Pre-zeroed: ds_drotation, ds_dtranslation (B * K poses),
// ds_dout_weight.  ds_dpoints / ds_dpoint_weight: plain stores when `accumulate_points` is 0 (one launch covers all
// images), atomics onto pre-zeroed buffers otherwise.  The per-(image, body) sums are k_bodies_bwd's: a block whose
// accepted lanes share one body goes wave -> block -> one atomic per value, otherwise every wave walks its bodies.
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kSmBlock) void k_smooth_bodies_bwd(
    GridDesc<NO> gd, int64_t P, int64_t B, int K, const T* __restrict__ g, const T* __restrict__ points,
    const int32_t* __restrict__ body, const T* __restrict__ rot, const T* __restrict__ trans,
    const T* __restrict__ ow, const T* __restrict__ pw, T* __restrict__ ds_dpoints, T* __restrict__ ds_drotation,
    T* __restrict__ ds_dtranslation, T* __restrict__ ds_dout_weight, T* __restrict__ ds_dpoint_weight,
    int poses_per_slice, int accumulate_points) {
    static_assert(NO == 2 || NO == 3, "the smooth splat is written for 2-D and 3-D grids");
    constexpr int NR = NO * NI + NO;  // dR | dt: per (image, body)
    constexpr int NV = NR + 1;        // | d out_weight: per image
    constexpr int NW = kSmBlock / kWave;
    __shared__ T red[NW][NV];
    __shared__ int wave_body[NW];

    const int64_t p = (int64_t)blockIdx.x * kSmBlock + threadIdx.x;
    const bool live = p < P;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    const WaveBodies wb = wave_bodies(body, p, P, K);
    // the block's body: -1 no accepted lane in the block, -2 more than one body, else the body all of them share
    if (lane == 0) wave_body[wave] = wb.distinct == 0 ? -1 : (wb.distinct == 1 ? wb.first : -2);
    __syncthreads();
    int block_body = -1;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const int v = wave_body[i];
        if (v == -1) continue;
        block_body = (block_body == -1 || block_body == v) ? v : -2;
    }
    block_body = __builtin_amdgcn_readfirstlane(block_body);

    T pt[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) pt[j] = T(0);
    if (wb.ok) load_point<T, NI>(points, p, pt);
    const T pwi = (wb.ok && pw) ? pw[p] : T(1);
    T acc_pt[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) acc_pt[j] = T(0);
    T acc_pw = T(0);

    const int64_t b_lo = (int64_t)blockIdx.y * poses_per_slice;
    const int64_t b_hi = (b_lo + poses_per_slice < B) ? b_lo + poses_per_slice : B;
    for (int64_t b = b_lo; b < b_hi; ++b) {
        const Pose<T, NI, NO> ps = load_body_pose<T, NI, NO>(rot, trans, ow, b, K, wb);
        T vals[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) vals[i] = T(0);
        int j0[NO];
        T u[NO];
        if (wb.ok && smooth_cell<T, NI, NO>(pt, ps, gd, j0, u)) {
            const T* gb = g + b * gd.G;
            T dcoord[NO], W;
            smooth_point_backward<T, NO>(j0, u, gd, [&](int off) { return gb[off]; }, dcoord, W);
            const T opw = ps.ow * pwi;  // from here to acc_pw: k_smooth_bwd's operation order
            T scaled[NO];
#pragma unroll
            for (int n = 0; n < NO; ++n) scaled[n] = (dcoord[n] * opw) * (T(gd.n[n]) / T(2));
#pragma unroll
            for (int n = 0; n < NO; ++n) {
#pragma unroll
                for (int j = 0; j < NI; ++j) vals[n + j * NO] = scaled[n] * pt[j];
                vals[NO * NI + n] = scaled[n];
            }
            vals[NR] = W * pwi;
#pragma unroll
            for (int j = 0; j < NI; ++j) {  // rotation' * scaled
                T v = ps.R[0 + j * NO] * scaled[0];
#pragma unroll
                for (int n = 1; n < NO; ++n) v = v + ps.R[n + j * NO] * scaled[n];
                acc_pt[j] += v;
            }
            acc_pw += W * ps.ow;
        }
        // value i of pose q = b * K + body: ds_drotation[q][i], then ds_dtranslation[q][i - NO * NI]
        auto add_to_pose = [&](int64_t q, int i, T s) {
            if (i < NO * NI)
                atomic_add<T>(ds_drotation + q * (NO * NI) + i, s);
            else
                atomic_add<T>(ds_dtranslation + q * NO + (i - NO * NI), s);
        };
        if (block_body != -2) {
            // one body in the block: wave -> block -> one atomic per value, d out_weight with them
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const T s = wave_sum<T>(vals[i]);
                if (lane == 0) red[wave][i] = s;
            }
        } else {
            const T sw = wave_sum<T>(vals[NR]);
            if (lane == 0) red[wave][NR] = sw;
            // walk the wave's bodies: lane i ends up with the sum of value i over the lanes of the body
            uint64_t rest = __builtin_amdgcn_ballot_w64(wb.ok);
            while (rest) {
                const int kc = lane_value(wb.k, __ffsll((unsigned long long)rest) - 1);
                const bool mine = wb.ok && wb.k == kc;
                T s_lane = T(0);
#pragma unroll
                for (int i = 0; i < NR; ++i) {
                    const T s = wave_sum<T>(mine ? vals[i] : T(0));
                    if (lane == i) s_lane = s;
                }
                if (lane < NR && s_lane != T(0)) add_to_pose(b * K + kc, lane, s_lane);
                rest &= ~__builtin_amdgcn_ballot_w64(mine);
            }
        }
        __syncthreads();
        if (threadIdx.x < NV && (threadIdx.x == NR || block_body >= 0)) {
            T s = red[0][threadIdx.x];
#pragma unroll
            for (int i = 1; i < NW; ++i) s += red[i][threadIdx.x];
            if (s != T(0)) {
                if (threadIdx.x == NR)
                    atomic_add<T>(ds_dout_weight + b, s);
                else
                    add_to_pose(b * K + block_body, threadIdx.x, s);
            }
        }
        __syncthreads();
    }
    if (live) {
        if (accumulate_points) {
#pragma unroll
            for (int j = 0; j < NI; ++j) atomic_add<T>(ds_dpoints + p * NI + j, acc_pt[j]);
            if (ds_dpoint_weight) atomic_add<T>(ds_dpoint_weight + p, acc_pw);
        } else {
#pragma unroll
            for (int j = 0; j < NI; ++j) ds_dpoints[p * NI + j] = acc_pt[j];
            if (ds_dpoint_weight) ds_dpoint_weight[p] = acc_pw;
        }
    }
}

// ---------------------------------------------------------------- DPR_ALGO_TILED forward
// The binning of a GROUP of nb images b0 .. b0 + nb - 1 at once (k_smooth_clouds_keys' shape): block blockIdx.x covers
// points (blockIdx.x % blocks_per_image) * 256 .. of image blockIdx.x / blocks_per_image.  key = b_local * tiles +
// (tile of the clamped centre cell under pose (b0 + b_local) * K + body[p]); all ones for a rejected point and for a
// body outside [0, K); value = the flat index b_local * P + p.  Every entry of keys / idx [0, nb * P) is written.
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kSmBlock) void k_smooth_bodies_keys(
    GridDesc<NO> gd, SmoothTiles<NO> tl, uint32_t tiles, int64_t P, uint32_t blocks_per_image, int64_t b0, int K,
    const T* __restrict__ points, const int32_t* __restrict__ body, const T* __restrict__ rot,
    const T* __restrict__ trans, uint32_t* __restrict__ keys, uint32_t* __restrict__ idx) {
    const uint32_t bl = blockIdx.x / blocks_per_image;
    const int64_t p = (int64_t)(blockIdx.x % blocks_per_image) * kSmBlock + threadIdx.x;
    const WaveBodies wb = wave_bodies(body, p, P, K);  // (all 64 lanes; before the return of the lanes past P)
    if (p >= P) return;
    uint32_t key = kSmoothNoKey;
    if (wb.ok) {
        T pt[NI];
        load_point<T, NI>(points, p, pt);
        const Pose<T, NI, NO> ps = load_body_pose<T, NI, NO>(rot, trans, nullptr, b0 + bl, K, wb);
        int j0[NO];
        T u[NO];
        if (smooth_cell<T, NI, NO>(pt, ps, gd, j0, u)) {
            uint32_t stride = 1;
            key = bl * tiles;
#pragma unroll
            for (int d = 0; d < NO; ++d) {
                const int c = j0[d] < 0 ? 0 : (j0[d] >= gd.n[d] ? gd.n[d] - 1 : j0[d]);
                key += (uint32_t)(c / SmoothTileShape<NO>::e[d]) * stride;
                stride *= (uint32_t)tl.nt[d];
            }
        }
    }
    const int64_t q = (int64_t)bl * P + p;
    keys[q] = key;
    idx[q] = (uint32_t)q;
}

// Workgroup blockIdx.x = b_local * tiles + tile: k_smooth_tile's body for the (image, tile)'s run of the group's sorted
// flat indices (`count` of them: nb * P), flushed onto plane b0 + b_local.  idx comes from a workspace whose contents
// the kernel does not trust: the run is clamped to [0, count) (ord_cell_range), the point index to [0, P) and the
// body to [0, K) before either addresses anything.  The pose is gathered per lane; out_weight is per image.
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kSmBlock) void k_smooth_bodies_tile(
    GridDesc<NO> gd, SmoothTiles<NO> tl, uint32_t tiles, uint32_t count, int64_t P, int64_t b0, int K,
    T* __restrict__ out, const T* __restrict__ points, const int32_t* __restrict__ body, const T* __restrict__ rot,
    const T* __restrict__ trans, const T* __restrict__ ow, const T* __restrict__ pw,
    const uint32_t* __restrict__ start, const uint32_t* __restrict__ idx) {
    static_assert(NO == 2 || NO == 3, "the smooth splat is written for 2-D and 3-D grids");
    constexpr int NC = smooth_lds_cells<NO>();
    __shared__ double cells[NC];
    uint32_t begin, end;
    ord_cell_range(start, blockIdx.x, count, begin, end);
    if (begin >= end) return;  // (uniform: an empty (image, tile) adds nothing)
    const int64_t bl = (int64_t)(blockIdx.x / tiles);
    const int64_t b = b0 + bl;
    int org[NO];  // first cell of the tile
    {
        uint32_t t = blockIdx.x % tiles;
#pragma unroll
        for (int d = 0; d < NO; ++d) {
            org[d] = (int)(t % (uint32_t)tl.nt[d]) * SmoothTileShape<NO>::e[d];
            t /= (uint32_t)tl.nt[d];
        }
    }
    for (int i = threadIdx.x; i < NC; i += kSmBlock) cells[i] = 0.0;
    __syncthreads();

    const T owb = ow ? ow[b] : T(1);
    for (uint32_t i = begin + threadIdx.x; i < end; i += kSmBlock) {
        const int64_t p = (int64_t)idx[i] - bl * P;
        if (p < 0 || p >= P) continue;  // (never for an index k_smooth_bodies_keys wrote into this run)
        const int kb = body[p];
        if ((unsigned)kb >= (unsigned)K) continue;  // (its key was all ones: never in a run of the sorted keys)
        T pt[NI];
        load_point<T, NI>(points, p, pt);
        const Pose<T, NI, NO> ps = load_pose<T, NI, NO>(rot, trans, nullptr, b * K + kb);
        int j0[NO];
        T u[NO];
        if (!smooth_cell<T, NI, NO>(pt, ps, gd, j0, u)) continue;
        const T w = owb * (pw ? pw[p] : T(1));
        // LDS cell l = (cell - org) + 1 per axis; only cells of the grid that lie on the tile + halo are added
        T wt[NO][3];
        int loff[NO][3];
        bool in[NO][3];
        int lstride = 1;
#pragma unroll
        for (int d = 0; d < NO; ++d) {
            spline_weights<T>(u[d], wt[d]);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int c = j0[d] + k - 1, l = c - org[d] + 1;
                in[d][k] = c >= 0 && c < gd.n[d] && l >= 0 && l < SmoothTileShape<NO>::e[d] + 2;
                loff[d][k] = in[d][k] ? l * lstride : 0;
            }
            lstride *= SmoothTileShape<NO>::e[d] + 2;
        }
#pragma unroll
        for (int k2 = 0; k2 < (NO == 3 ? 3 : 1); ++k2) {
            const bool in2 = NO == 3 ? in[NO - 1][k2] : true;
            const int off2 = NO == 3 ? loff[NO - 1][k2] : 0;
            const T w2 = NO == 3 ? wt[NO - 1][k2] * w : w;
#pragma unroll
            for (int k1 = 0; k1 < 3; ++k1) {
                const T w12 = wt[1][k1] * w2;
#pragma unroll
                for (int k0 = 0; k0 < 3; ++k0)
                    if (in2 && in[1][k1] && in[0][k0])
                        atomicAdd(&cells[off2 + loff[1][k1] + loff[0][k0]], (double)(wt[0][k0] * w12));
            }
        }
    }
    __syncthreads();

    // flush: consecutive threads walk axis 0 of the tile + halo, so a wave's atomics cover rows of the plane
    T* o = out + b * gd.G;
    for (int i = threadIdx.x; i < NC; i += kSmBlock) {
        const double v = cells[i];
        int rest = i, off = 0, stride = 1;
        bool in_grid = true;
#pragma unroll
        for (int d = 0; d < NO; ++d) {
            const int ext = SmoothTileShape<NO>::e[d] + 2;
            const int c = org[d] + (rest % ext) - 1;
            rest /= ext;
            in_grid = in_grid && c >= 0 && c < gd.n[d];
            off += in_grid ? c * stride : 0;
            stride *= gd.n[d];
        }
        if (in_grid && v != 0.0) atomic_add<T>(o + off, (T)v);
    }
}

// ---------------------------------------------------------------- forward mode
// include/dpr.h, "SMOOTH SPLAT, RIGID BODIES, FORWARD MODE": out_dot = J . v for V tangents.  Pose tangent (v, b, k)
// sits at (v * B + b) * K + k, out_weight_dot and background_dot at v * B + b, plane (b, v) of out_dot at
// (b * V + v) * G; out_dot holds the background tangent already (jvp_fill).  The per-tangent arithmetic is that of
// k_smooth_jvp_atomic / k_smooth_tile_jvp: jvp_coeffs (dpr_jvp.h), smooth_jvp_rows (dpr_smooth_device.h).

// The tangent of pose (b, k) of a lane, vb = v * B + b: loaded as load_body_pose loads the primal -- scalar loads
// where the wave's ok lanes share a body, a per-lane gather otherwise; out_weight_dot is per (tangent, image).
template <typename T, int NI, int NO>
__device__ __forceinline__ JvpPose<T, NI, NO> load_body_jvp_pose(const T* __restrict__ rot_dot,
                                                                const T* __restrict__ trans_dot,
                                                                const T* __restrict__ ow_dot, int64_t vb, int K,
                                                                const WaveBodies& w) {
    JvpPose<T, NI, NO> tp;
    if (w.distinct <= 1)
        tp = load_jvp_pose<T, NI, NO>(rot_dot, trans_dot, nullptr, vb * K + __builtin_amdgcn_readfirstlane(w.first));
    else
        tp = load_jvp_pose<T, NI, NO>(rot_dot, trans_dot, nullptr, vb * K + w.k);
    tp.owd = ow_dot ? ow_dot[vb] : T(0);
    return tp;
}

// DPR_ALGO_ATOMIC: k_smooth_bodies_fwd_atomic's shape (one thread per point, the images striding over blockIdx.y)
// around k_smooth_jvp_atomic's run-time loop over the tangents.  The cell, the weights and their derivatives once per
// accepted (point, image); 3^N atomics per tangent.  A dropped point reads none of its tangents.  There is no
// equal-cell wave combine here: every lane issues its own atomics.
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kSmBlock) void k_smooth_bodies_jvp_atomic(
    GridDesc<NO> gd, int64_t P, int64_t B, int K, int V, T* __restrict__ out_dot, const T* __restrict__ points,
    const int32_t* __restrict__ body, const T* __restrict__ rot, const T* __restrict__ trans,
    const T* __restrict__ ow, const T* __restrict__ pw, JvpTangents<T> tan) {
    static_assert(NO == 2 || NO == 3, "the smooth splat is written for 2-D and 3-D grids");
    const int64_t p = (int64_t)blockIdx.x * kSmBlock + threadIdx.x;
    const WaveBodies wb = wave_bodies(body, p, P, K);
    if (wb.distinct == 0) return;  // (the whole wave: no lane has a point to deposit)
    T pt[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) pt[j] = T(0);
    if (wb.ok) load_point<T, NI>(points, p, pt);
    const T pwi = (wb.ok && pw) ? pw[p] : T(1);
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        const Pose<T, NI, NO> ps = load_body_pose<T, NI, NO>(rot, trans, ow, b, K, wb);
        int j0[NO];
        T u[NO];
        if (!(wb.ok && smooth_cell<T, NI, NO>(pt, ps, gd, j0, u))) continue;
        const SmoothAxes<T, NO> ax = smooth_axes<T, NO>(j0, u, gd);
        T dw[NO][3];
#pragma unroll
        for (int d = 0; d < NO; ++d) spline_derivatives<T>(u[d], dw[d]);
        T* o = out_dot + b * V * gd.G;
        for (int v = 0; v < V; ++v) {
            const JvpPose<T, NI, NO> tp =
                load_body_jvp_pose<T, NI, NO>(tan.rot, tan.trans, tan.ow, (int64_t)v * B + b, K, wb);
            T pd[NI], pwd;
            load_jvp_point<T, NI>(tan.points, tan.pw, (int64_t)v * P + p, pd, pwd);
            T a, bc[NO];
            jvp_coeffs<T, NI, NO>(pt, pwi, pd, pwd, ps, tp, gd, a, bc);
            const SmoothJvpRows<T, NO> r = smooth_jvp_rows<T, NO>(a, bc, ax.w, dw);
            T f0[3];
#pragma unroll
            for (int k0 = 0; k0 < 3; ++k0) f0[k0] = bc[0] * dw[0][k0];
            T* plane = o + (int64_t)v * gd.G;
#pragma unroll
            for (int k2 = 0; k2 < (NO == 3 ? 3 : 1); ++k2) {
                const bool in2 = NO == 3 ? ax.in[NO - 1][k2] : true;
                const int off2 = NO == 3 ? ax.off[NO - 1][k2] : 0;
#pragma unroll
                for (int k1 = 0; k1 < 3; ++k1) {
#pragma unroll
                    for (int k0 = 0; k0 < 3; ++k0)
                        if (in2 && ax.in[1][k1] && ax.in[0][k0])
                            atomic_add<T>(plane + (off2 + ax.off[1][k1] + ax.off[0][k0]),
                                          ax.w[0][k0] * r.X[k2][k1] + f0[k0] * r.Y[k2][k1]);
                }
            }
        }
    }
}

// DPR_ALGO_TILED: workgroup (blockIdx.x, blockIdx.y) = (b_local * tiles + tile, v).  k_smooth_bodies_tile's walk over
// the (image, tile)'s run of the group's sorted flat indices, with its distrust of the workspace (the run clamped to
// [0, count), the point index to [0, P), the body to [0, K)), its f64 LDS tile + halo and its flush, and the deposit
// of tangent v in the place of the weight product.  The pose and its tangent are gathered per lane; a and bc are
// formed before the spline terms, so neither outlives jvp_coeffs.  Deposits have both signs; a cell whose sum is
// exactly 0 is skipped by the flush, which is right because the plane holds the background tangent already.
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kSmBlock) void k_smooth_bodies_tile_jvp(
    GridDesc<NO> gd, SmoothTiles<NO> tl, uint32_t tiles, uint32_t count, int64_t P, int64_t B, int64_t b0, int K,
    int V, T* __restrict__ out_dot, const T* __restrict__ points, const int32_t* __restrict__ body,
    const T* __restrict__ rot, const T* __restrict__ trans, const T* __restrict__ ow, const T* __restrict__ pw,
    JvpTangents<T> tan, const uint32_t* __restrict__ start, const uint32_t* __restrict__ idx) {
    static_assert(NO == 2 || NO == 3, "the smooth splat is written for 2-D and 3-D grids");
    constexpr int NC = smooth_lds_cells<NO>();
    __shared__ double cells[NC];
    uint32_t begin, end;
    ord_cell_range(start, blockIdx.x, count, begin, end);
    if (begin >= end) return;  // (uniform: an empty (image, tile) adds nothing)
    const int64_t bl = (int64_t)(blockIdx.x / tiles);
    const int64_t b = b0 + bl;
    const int64_t v = blockIdx.y;
    const int64_t vb = v * B + b;
    int org[NO];  // first cell of the tile
    {
        uint32_t t = blockIdx.x % tiles;
#pragma unroll
        for (int d = 0; d < NO; ++d) {
            org[d] = (int)(t % (uint32_t)tl.nt[d]) * SmoothTileShape<NO>::e[d];
            t /= (uint32_t)tl.nt[d];
        }
    }
    for (int i = threadIdx.x; i < NC; i += kSmBlock) cells[i] = 0.0;
    __syncthreads();

    const T owb = ow ? ow[b] : T(1);
    const T owd = tan.ow ? tan.ow[vb] : T(0);
    for (uint32_t i = begin + threadIdx.x; i < end; i += kSmBlock) {
        const int64_t p = (int64_t)idx[i] - bl * P;
        if (p < 0 || p >= P) continue;  // (never for an index k_smooth_bodies_keys wrote into this run)
        const int kb = body[p];
        if ((unsigned)kb >= (unsigned)K) continue;  // (its key was all ones: never in a run of the sorted keys)
        T pt[NI];
        load_point<T, NI>(points, p, pt);
        int j0[NO];
        T u[NO], a, bc[NO];
        {
            Pose<T, NI, NO> ps = load_pose<T, NI, NO>(rot, trans, nullptr, b * K + kb);
            ps.ow = owb;
            if (!smooth_cell<T, NI, NO>(pt, ps, gd, j0, u)) continue;
            JvpPose<T, NI, NO> tp = load_jvp_pose<T, NI, NO>(tan.rot, tan.trans, nullptr, vb * K + kb);
            tp.owd = owd;
            T pd[NI], pwd;
            load_jvp_point<T, NI>(tan.points, tan.pw, v * P + p, pd, pwd);
            jvp_coeffs<T, NI, NO>(pt, pw ? pw[p] : T(1), pd, pwd, ps, tp, gd, a, bc);
        }
        // LDS cell l = (cell - org) + 1 per axis; only cells of the grid that lie on the tile + halo are added
        T wt[NO][3], dw[NO][3];
        int loff[NO][3];
        bool in[NO][3];
        int lstride = 1;
#pragma unroll
        for (int d = 0; d < NO; ++d) {
            spline_weights<T>(u[d], wt[d]);
            spline_derivatives<T>(u[d], dw[d]);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int c = j0[d] + q - 1, l = c - org[d] + 1;
                in[d][q] = c >= 0 && c < gd.n[d] && l >= 0 && l < SmoothTileShape<NO>::e[d] + 2;
                loff[d][q] = in[d][q] ? l * lstride : 0;
            }
            lstride *= SmoothTileShape<NO>::e[d] + 2;
        }
        const SmoothJvpRows<T, NO> r = smooth_jvp_rows<T, NO>(a, bc, wt, dw);
        T f0[3];
#pragma unroll
        for (int k0 = 0; k0 < 3; ++k0) f0[k0] = bc[0] * dw[0][k0];
#pragma unroll
        for (int k2 = 0; k2 < (NO == 3 ? 3 : 1); ++k2) {
            const bool in2 = NO == 3 ? in[NO - 1][k2] : true;
            const int off2 = NO == 3 ? loff[NO - 1][k2] : 0;
#pragma unroll
            for (int k1 = 0; k1 < 3; ++k1) {
#pragma unroll
                for (int k0 = 0; k0 < 3; ++k0)
                    if (in2 && in[1][k1] && in[0][k0])
                        atomicAdd(&cells[off2 + loff[1][k1] + loff[0][k0]],
                                  (double)(wt[0][k0] * r.X[k2][k1] + f0[k0] * r.Y[k2][k1]));
            }
        }
    }
    __syncthreads();

    // flush: consecutive threads walk axis 0 of the tile + halo, so a wave's atomics cover rows of the plane
    T* o = out_dot + (b * V + v) * gd.G;
    for (int i = threadIdx.x; i < NC; i += kSmBlock) {
        const double val = cells[i];
        int rest = i, off = 0, stride = 1;
        bool in_grid = true;
#pragma unroll
        for (int d = 0; d < NO; ++d) {
            const int ext = SmoothTileShape<NO>::e[d] + 2;
            const int c = org[d] + (rest % ext) - 1;
            rest /= ext;
            in_grid = in_grid && c >= 0 && c < gd.n[d];
            off += in_grid ? c * stride : 0;
            stride *= gd.n[d];
        }
        if (in_grid && val != 0.0) atomic_add<T>(o + off, (T)val);
    }
}

// ---------------------------------------------------------------- launches
template <typename T, int NI, int NO>
int smooth_bodies_fwd_atomic(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int K, T* out,
                             const T* points, const int32_t* body, const T* rot, const T* trans, const T* ow,
                             const T* pw) {
    if (P <= 0 || B <= 0) return DPR_OK;
    const GridDesc<NO> gd = make_grid_desc<NO>(grid, G);
    dim3 gg((unsigned)((P + kSmBlock - 1) / kSmBlock), (unsigned)(B < 65535 ? B : 65535));
    hipLaunchKernelGGL((k_smooth_bodies_fwd_atomic<T, NI, NO>), gg, dim3(kSmBlock), 0, st, gd, P, B, K, out, points,
                       body, rot, trans, ow, pw);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

// The binning of the group of nb images b0 .. b0 + nb - 1: k_smooth_bodies_keys, then smooth_sort_group.  Depends on
// the primal only; afterwards sb.start / sb.idx_out hold the runs of the group's (image, tile) pairs.
template <typename T, int NI, int NO>
int smooth_bodies_bin_group(hipStream_t st, const SmoothBinning<NO>& sb, int64_t P, int64_t b0, int64_t nb, int K,
                            const T* points, const int32_t* body, const T* rot, const T* trans) {
    const int64_t blocks_per_image = (P + kSmBlock - 1) / kSmBlock;
    hipLaunchKernelGGL((k_smooth_bodies_keys<T, NI, NO>), dim3((unsigned)(nb * blocks_per_image)), dim3(kSmBlock), 0,
                       st, sb.gd, sb.tl, (uint32_t)sb.tiles, P, (uint32_t)blocks_per_image, b0, K, points, body, rot,
                       trans, sb.keys_in, sb.idx_in);
    return smooth_sort_group<NO>(st, sb, nb, P);
}

// group after group of sb.group images: keys -> sort -> start table -> tiles, four launches per GROUP (the last group
// may hold fewer images): the group rule, the workspace and the byte count of smooth_clouds_fwd_tiled
template <typename T, int NI, int NO>
int smooth_bodies_fwd_tiled(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int K, int max_group,
                            T* out, const T* points, const int32_t* body, const T* rot, const T* trans, const T* ow,
                            const T* pw, void* ws, size_t ws_bytes) {
    if (P <= 0 || B <= 0) return DPR_OK;
    SmoothBinning<NO> sb;
    if (int rc = smooth_binning<NO>(grid, G, P, B, smooth_clouds_group(NO, grid, P, B, max_group), ws, ws_bytes, &sb))
        return rc;
    const dim3 blk(kSmBlock);
    for (int64_t b0 = 0; b0 < B; b0 += sb.group) {
        const int64_t nb = B - b0 < sb.group ? B - b0 : sb.group;
        if (int rc = smooth_bodies_bin_group<T, NI, NO>(st, sb, P, b0, nb, K, points, body, rot, trans)) return rc;
        hipLaunchKernelGGL((k_smooth_bodies_tile<T, NI, NO>), dim3((unsigned)(nb * sb.tiles)), blk, 0, st, sb.gd,
                           sb.tl, (uint32_t)sb.tiles, (uint32_t)(nb * P), P, b0, K, out, points, body, rot, trans, ow,
                           pw, (const uint32_t*)sb.start, (const uint32_t*)sb.idx_out);
        stage_mark(st);
    }
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

// Pre-zeroed by the caller: d_rot, d_trans, d_ow; with more than one slice of images d_pts and d_pw are zeroed here
// and added with atomics (smooth_bwd_atomic's shape)
template <typename T, int NI, int NO>
int smooth_bodies_bwd_atomic(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int K, const T* g,
                             const T* points, const int32_t* body, const T* rot, const T* trans, const T* ow,
                             const T* pw, T* d_pts, T* d_rot, T* d_trans, T* d_ow, T* d_pw, int poses_per_slice,
                             int64_t slices) {
    if (P <= 0 || B <= 0) return DPR_OK;
    const GridDesc<NO> gd = make_grid_desc<NO>(grid, G);
    const int accumulate = slices > 1;
    if (accumulate) {
        DPR_HIP(zero_async(st, d_pts, sizeof(T) * (size_t)(P * NI)));
        if (d_pw) DPR_HIP(zero_async(st, d_pw, sizeof(T) * (size_t)P));
    }
    dim3 gg((unsigned)((P + kSmBlock - 1) / kSmBlock), (unsigned)slices);
    hipLaunchKernelGGL((k_smooth_bodies_bwd<T, NI, NO>), gg, dim3(kSmBlock), 0, st, gd, P, B, K, g, points, body, rot,
                       trans, ow, pw, d_pts, d_rot, d_trans, d_ow, d_pw, poses_per_slice, accumulate);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

template <typename T, int NI, int NO>
int smooth_bodies_jvp_atomic(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int K, int V,
                             T* out_dot, const T* points, const int32_t* body, const T* rot, const T* trans,
                             const T* ow, const T* pw, JvpTangents<T> tan) {
    if (P <= 0 || B <= 0) return DPR_OK;
    const GridDesc<NO> gd = make_grid_desc<NO>(grid, G);
    dim3 gg((unsigned)((P + kSmBlock - 1) / kSmBlock), (unsigned)(B < 65535 ? B : 65535));
    hipLaunchKernelGGL((k_smooth_bodies_jvp_atomic<T, NI, NO>), gg, dim3(kSmBlock), 0, st, gd, P, B, K, V, out_dot,
                       points, body, rot, trans, ow, pw, tan);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

// smooth_bodies_fwd_tiled's groups, workspace and first three stages -- the keys and the sort depend on the primal
// only -- then ONE launch of (nb * tiles) x V workgroups: four launches per group, whatever V
template <typename T, int NI, int NO>
int smooth_bodies_jvp_tiled(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int K, int V,
                            int max_group, T* out_dot, const T* points, const int32_t* body, const T* rot,
                            const T* trans, const T* ow, const T* pw, JvpTangents<T> tan, void* ws, size_t ws_bytes) {
    if (P <= 0 || B <= 0) return DPR_OK;
    SmoothBinning<NO> sb;
    if (int rc = smooth_binning<NO>(grid, G, P, B, smooth_clouds_group(NO, grid, P, B, max_group), ws, ws_bytes, &sb))
        return rc;
    const dim3 blk(kSmBlock);
    for (int64_t b0 = 0; b0 < B; b0 += sb.group) {
        const int64_t nb = B - b0 < sb.group ? B - b0 : sb.group;
        if (int rc = smooth_bodies_bin_group<T, NI, NO>(st, sb, P, b0, nb, K, points, body, rot, trans)) return rc;
        hipLaunchKernelGGL((k_smooth_bodies_tile_jvp<T, NI, NO>), dim3((unsigned)(nb * sb.tiles), (unsigned)V), blk,
                           0, st, sb.gd, sb.tl, (uint32_t)sb.tiles, (uint32_t)(nb * P), P, B, b0, K, V, out_dot,
                           points, body, rot, trans, ow, pw, tan, (const uint32_t*)sb.start,
                           (const uint32_t*)sb.idx_out);
        stage_mark(st);
    }
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

#define DPR_SMOOTH_BODIES_INSTANTIATE(T, NI, NO)                                                                     \
    template int smooth_bodies_bin_group<T, NI, NO>(hipStream_t, const SmoothBinning<NO>&, int64_t, int64_t,         \
                                                    int64_t, int, const T*, const int32_t*, const T*, const T*);    \
    template int smooth_bodies_fwd_atomic<T, NI, NO>(hipStream_t, const int64_t*, int64_t, int64_t, int64_t, int,    \
                                                     T*, const T*, const int32_t*, const T*, const T*, const T*,    \
                                                     const T*);                                                     \
    template int smooth_bodies_fwd_tiled<T, NI, NO>(hipStream_t, const int64_t*, int64_t, int64_t, int64_t, int,     \
                                                    int, T*, const T*, const int32_t*, const T*, const T*,          \
                                                    const T*, const T*, void*, size_t);                             \
    template int smooth_bodies_bwd_atomic<T, NI, NO>(hipStream_t, const int64_t*, int64_t, int64_t, int64_t, int,    \
                                                     const T*, const T*, const int32_t*, const T*, const T*,        \
                                                     const T*, const T*, T*, T*, T*, T*, T*, int, int64_t);         \
    template int smooth_bodies_jvp_atomic<T, NI, NO>(hipStream_t, const int64_t*, int64_t, int64_t, int64_t, int,    \
                                                     int, T*, const T*, const int32_t*, const T*, const T*,         \
                                                     const T*, const T*, JvpTangents<T>);                           \
    template int smooth_bodies_jvp_tiled<T, NI, NO>(hipStream_t, const int64_t*, int64_t, int64_t, int64_t, int,     \
                                                    int, int, T*, const T*, const int32_t*, const T*, const T*,     \
                                                    const T*, const T*, JvpTangents<T>, void*, size_t);
#define DPR_SMOOTH_BODIES_INSTANTIATE_T(T)                                           \
    DPR_SMOOTH_BODIES_INSTANTIATE(T, 2, 2) DPR_SMOOTH_BODIES_INSTANTIATE(T, 3, 3) \
    DPR_SMOOTH_BODIES_INSTANTIATE(T, 3, 2)
DPR_SMOOTH_BODIES_INSTANTIATE_T(float)
DPR_SMOOTH_BODIES_INSTANTIATE_T(double)

}  // namespace dpr

