// Smooth sampling at the points of rigid bodies (include/dpr.h, "SMOOTH SAMPLING, RIGID BODIES"): SMOOTH SAMPLING
// through the poses of RIGID BODIES.  Point p belongs to body[p] in [0, K) and reads image b through pose
// b * K + body[p]; the kernels of the family and their launches (declared in dpr_smooth.h; host checks, AUTO rule and
// the C ABI: dpr_api_smooth_bodies.hip).
//
//   forward                   k_sample_smooth_bodies_fwd: k_sample_smooth_fwd with the pose of wave_bodies /
//                             load_body_pose (dpr_kernels_bodies.h); every values[p, b] is stored, 0 for a dropped point
//   pullback, point kernel    k_sample_smooth_bodies_bwd: the point terms of k_sample_smooth_bwd (the same operation
//                             order) inside the per-(image, body) reduction of k_smooth_bodies_bwd; a block of several
//                             bodies adds its masked wave sums into an LDS table indexed by body while K <= kBodyTable
//                             and sends one global atomic per non-zero (body, value) of the BLOCK, not of the wave
//   ds_dimage, DPR_ALGO_TILED the images binned in groups by smooth_bodies_bin_group (dpr_smooth_bodies.hip), then
//                             k_sample_smooth_bodies_tile: k_smooth_bodies_tile with the weight of the flat index
//                             b_local * P + p read from ds_dvalues[(b0 + b_local) * P + p]
// These are copies of the sampling and the rigid-body kernels, not shared bodies: those kernels keep their registers.
// A body index outside [0, K) is checked per lane before it addresses a pose, in every kernel.
#include <hip/hip_runtime.h>

#include "../../include/dpr.h"
#include "dpr_kernels_bodies.h"
#include "dpr_ordered.h"
#include "dpr_ordered_index.h"
#include "dpr_smooth.h"
#include "dpr_smooth_device.h"

namespace dpr {

static_assert(kSmBlock == kBlock, "pose_slices and the P bound of the host checks count blocks of kBlock points");

// Bodies a block's LDS table of pose sums holds: 64 x (N_out * N_in + N_out) values, 6 KB for fp64 (3,3).
constexpr int kBodyTable = 64;

// ---------------------------------------------------------------- forward
// One thread per point over the image range of blockIdx.y.  No atomics and no sum across threads: the value of a
// (point, image) does not depend on where the point stands in the cloud.  A wave without an accepted lane still
// stores its zeros.
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kSmBlock) void k_sample_smooth_bodies_fwd(
    GridDesc<NO> gd, int64_t P, int64_t B, int K, T* __restrict__ values, const T* __restrict__ image,
    const T* __restrict__ points, const int32_t* __restrict__ body, const T* __restrict__ rot,
    const T* __restrict__ trans, int poses_per_slice) {
    static_assert(NO == 2 || NO == 3, "the smooth splat is written for 2-D and 3-D grids");
    const int64_t p = (int64_t)blockIdx.x * kSmBlock + threadIdx.x;
    const WaveBodies wb = wave_bodies(body, p, P, K);
    T pt[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) pt[j] = T(0);
    if (wb.ok) load_point<T, NI>(points, p, pt);
    const int64_t b_lo = (int64_t)blockIdx.y * poses_per_slice;
    const int64_t b_hi = (b_lo + poses_per_slice < B) ? b_lo + poses_per_slice : B;
    for (int64_t b = b_lo; b < b_hi; ++b) {
        const Pose<T, NI, NO> ps = load_body_pose<T, NI, NO>(rot, trans, nullptr, b, K, wb);
        int j0[NO];
        T u[NO];
        T v = T(0);
        if (wb.ok && smooth_cell<T, NI, NO>(pt, ps, gd, j0, u)) {
            const T* img = image + b * gd.G;
            T dcoord[NO];  // (only W is kept; the compiler drops the derivative sums)
            smooth_point_backward<T, NO>(j0, u, gd, [&](int off) { return img[off]; }, dcoord, v);
        }
        if (p < P) values[b * P + p] = v;
    }
}

// ---------------------------------------------------------------- pullback, point kernel
// Over the image range [b_lo, b_hi) of blockIdx.y, for dv = ds_dvalues[p, b].  Any output may be NULL (uniform
// branches; the image is read only for the three geometric gradients).  Pre-zeroed: ds_drotation, ds_dtranslation
// (B * K poses), ds_dimage; ds_dpoints is stored (accumulate_points == 0) or added atomically onto a zeroed buffer.
// The per-(image, body) sums:
//   one body in the block          wave -> block -> one atomic per value (k_smooth_bodies_bwd's path)
//   several, K <= kBodyTable       every wave walks its bodies as there and adds the masked wave sums into
//                                  tab[body][value] with LDS atomics; after the barrier the block sends one global
//                                  atomic per non-zero entry and clears it for the next image
//   several, K > kBodyTable        the walk with one global atomic per value, wave and body
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kSmBlock) void k_sample_smooth_bodies_bwd(
    GridDesc<NO> gd, int64_t P, int64_t B, int K, const T* __restrict__ ds_dvalues, const T* __restrict__ image,
    const T* __restrict__ points, const int32_t* __restrict__ body, const T* __restrict__ rot,
    const T* __restrict__ trans, T* __restrict__ ds_dimage, T* __restrict__ ds_dpoints, T* __restrict__ ds_drotation,
    T* __restrict__ ds_dtranslation, int poses_per_slice, int accumulate_points) {
    static_assert(NO == 2 || NO == 3, "the smooth splat is written for 2-D and 3-D grids");
    constexpr int NR = NO * NI + NO;  // dR | dt: per (image, body)
    constexpr int NW = kSmBlock / kWave;
    __shared__ T red[NW][NR];
    __shared__ T tab[kBodyTable * NR];
    __shared__ int wave_body[NW];

    const int64_t p = (int64_t)blockIdx.x * kSmBlock + threadIdx.x;
    const bool live = p < P;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    const bool geom = ds_dpoints || ds_drotation || ds_dtranslation;
    const bool pose_sums = ds_drotation || ds_dtranslation;
    const bool table = K <= kBodyTable;
    const WaveBodies wb = wave_bodies(body, p, P, K);
    // the block's body: -1 no accepted lane in the block, -2 more than one body, else the body all of them share
    if (lane == 0) wave_body[wave] = wb.distinct == 0 ? -1 : (wb.distinct == 1 ? wb.first : -2);
    for (int i = threadIdx.x; i < kBodyTable * NR; i += kSmBlock) tab[i] = T(0);
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
    T acc_pt[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) acc_pt[j] = T(0);

    const int64_t b_lo = (int64_t)blockIdx.y * poses_per_slice;
    const int64_t b_hi = (b_lo + poses_per_slice < B) ? b_lo + poses_per_slice : B;
    for (int64_t b = b_lo; b < b_hi; ++b) {
        const Pose<T, NI, NO> ps = load_body_pose<T, NI, NO>(rot, trans, nullptr, b, K, wb);
        T vals[NR];
#pragma unroll
        for (int i = 0; i < NR; ++i) vals[i] = T(0);
        int j0[NO];
        T u[NO];
        if (wb.ok && smooth_cell<T, NI, NO>(pt, ps, gd, j0, u)) {
            const T dv = ds_dvalues[b * P + p];
            if (ds_dimage) {  // k_sample_smooth_bwd's deposit
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
            if (geom) {  // from here to acc_pt: k_sample_smooth_bwd's operation order
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
                    acc_pt[j] += v;
                }
            }
        }
        if (!pose_sums) continue;  // (uniform: no barrier is skipped by a part of the block)
        // value i of pose q = b * K + body: ds_drotation[q][i], then ds_dtranslation[q][i - NO * NI]
        auto add_to_pose = [&](int64_t q, int i, T s) {
            if (i < NO * NI) {
                if (ds_drotation) atomic_add<T>(ds_drotation + q * (NO * NI) + i, s);
            } else if (ds_dtranslation) {
                atomic_add<T>(ds_dtranslation + q * NO + (i - NO * NI), s);
            }
        };
        if (block_body != -2) {
            // one body in the block: wave -> block -> one atomic per value
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const T s = wave_sum<T>(vals[i]);
                if (lane == 0) red[wave][i] = s;
            }
        } else {
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
                if (lane < NR && s_lane != T(0)) {
                    if (table)
                        atomicAdd(&tab[kc * NR + lane], s_lane);  // (kc < K <= kBodyTable)
                    else
                        add_to_pose(b * K + kc, lane, s_lane);
                }
                rest &= ~__builtin_amdgcn_ballot_w64(mine);
            }
        }
        __syncthreads();
        if (block_body >= 0) {
            if (threadIdx.x < NR) {
                T s = red[0][threadIdx.x];
#pragma unroll
                for (int i = 1; i < NW; ++i) s += red[i][threadIdx.x];
                if (s != T(0)) add_to_pose(b * K + block_body, threadIdx.x, s);
            }
        } else if (block_body == -2 && table) {
            for (int i = threadIdx.x; i < K * NR; i += kSmBlock) {
                const T s = tab[i];
                if (s != T(0)) {
                    add_to_pose(b * K + i / NR, i % NR, s);
                    tab[i] = T(0);
                }
            }
        }
        __syncthreads();
    }
    if (live && ds_dpoints) {
        if (accumulate_points) {
#pragma unroll
            for (int j = 0; j < NI; ++j) atomic_add<T>(ds_dpoints + p * NI + j, acc_pt[j]);
        } else {
#pragma unroll
            for (int j = 0; j < NI; ++j) ds_dpoints[p * NI + j] = acc_pt[j];
        }
    }
}

// ---------------------------------------------------------------- ds_dimage on DPR_ALGO_TILED
// Workgroup blockIdx.x = b_local * tiles + tile: k_smooth_bodies_tile's walk over the (image, tile)'s run of the
// group's sorted flat indices (`count` of them: nb * P), its f64 LDS tile + halo and its flush onto plane
// b0 + b_local, with the weight of (point, image) from ds_dvalues.  idx comes from a workspace whose contents the
// kernel does not trust: the run is clamped to [0, count) (ord_cell_range), the point index to [0, P) and the body to
// [0, K) before either addresses anything.  The pose is gathered per lane.
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kSmBlock) void k_sample_smooth_bodies_tile(
    GridDesc<NO> gd, SmoothTiles<NO> tl, uint32_t tiles, uint32_t count, int64_t P, int64_t b0, int K,
    T* __restrict__ ds_dimage, const T* __restrict__ ds_dvalues, const T* __restrict__ points,
    const int32_t* __restrict__ body, const T* __restrict__ rot, const T* __restrict__ trans,
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

    const T* dvb = ds_dvalues + b * P;
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
        const T w = dvb[p];
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
    T* o = ds_dimage + b * gd.G;
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

// ---------------------------------------------------------------- launches
template <typename T, int NI, int NO>
int sample_smooth_bodies_fwd(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int K, T* values,
                             const T* image, const T* points, const int32_t* body, const T* rot, const T* trans,
                             int poses_per_slice, int64_t slices) {
    if (P <= 0 || B <= 0) return DPR_OK;
    const GridDesc<NO> gd = make_grid_desc<NO>(grid, G);
    dim3 gg((unsigned)((P + kSmBlock - 1) / kSmBlock), (unsigned)slices);
    hipLaunchKernelGGL((k_sample_smooth_bodies_fwd<T, NI, NO>), gg, dim3(kSmBlock), 0, st, gd, P, B, K, values, image,
                       points, body, rot, trans, poses_per_slice);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

// Pre-zeroed by the caller: d_img, d_rot, d_trans; with more than one slice of images d_pts is zeroed here and added
// with atomics.  Nothing is launched without an output.
template <typename T, int NI, int NO>
int sample_smooth_bodies_bwd(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int K, const T* dv,
                             const T* image, const T* points, const int32_t* body, const T* rot, const T* trans,
                             T* d_img, T* d_pts, T* d_rot, T* d_trans, int poses_per_slice, int64_t slices) {
    if (P <= 0 || B <= 0 || !(d_img || d_pts || d_rot || d_trans)) return DPR_OK;
    const GridDesc<NO> gd = make_grid_desc<NO>(grid, G);
    const int accumulate = slices > 1;
    if (accumulate && d_pts) DPR_HIP(zero_async(st, d_pts, sizeof(T) * (size_t)(P * NI)));
    dim3 gg((unsigned)((P + kSmBlock - 1) / kSmBlock), (unsigned)slices);
    hipLaunchKernelGGL((k_sample_smooth_bodies_bwd<T, NI, NO>), gg, dim3(kSmBlock), 0, st, gd, P, B, K, dv, image,
                       points, body, rot, trans, d_img, d_pts, d_rot, d_trans, poses_per_slice, accumulate);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

// group after group of sb.group images: keys -> sort -> start table -> tiles, four launches per GROUP (the last group
// may hold fewer images): the group rule and the workspace of smooth_bodies_fwd_tiled
template <typename T, int NI, int NO>
int sample_smooth_bodies_image_tiled(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int K,
                                     int max_group, T* d_img, const T* dv, const T* points, const int32_t* body,
                                     const T* rot, const T* trans, void* ws, size_t ws_bytes) {
    if (P <= 0 || B <= 0) return DPR_OK;
    SmoothBinning<NO> sb;
    if (int rc = smooth_binning<NO>(grid, G, P, B, smooth_clouds_group(NO, grid, P, B, max_group), ws, ws_bytes, &sb))
        return rc;
    for (int64_t b0 = 0; b0 < B; b0 += sb.group) {
        const int64_t nb = B - b0 < sb.group ? B - b0 : sb.group;
        if (int rc = smooth_bodies_bin_group<T, NI, NO>(st, sb, P, b0, nb, K, points, body, rot, trans)) return rc;
        hipLaunchKernelGGL((k_sample_smooth_bodies_tile<T, NI, NO>), dim3((unsigned)(nb * sb.tiles)), dim3(kSmBlock),
                           0, st, sb.gd, sb.tl, (uint32_t)sb.tiles, (uint32_t)(nb * P), P, b0, K, d_img, dv, points,
                           body, rot, trans, (const uint32_t*)sb.start, (const uint32_t*)sb.idx_out);
        stage_mark(st);
    }
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

#define DPR_SAMPLE_SMOOTH_BODIES_INSTANTIATE(T, NI, NO)                                                              \
    template int sample_smooth_bodies_fwd<T, NI, NO>(hipStream_t, const int64_t*, int64_t, int64_t, int64_t, int,    \
                                                     T*, const T*, const T*, const int32_t*, const T*, const T*,    \
                                                     int, int64_t);                                                 \
    template int sample_smooth_bodies_bwd<T, NI, NO>(hipStream_t, const int64_t*, int64_t, int64_t, int64_t, int,    \
                                                     const T*, const T*, const T*, const int32_t*, const T*,        \
                                                     const T*, T*, T*, T*, T*, int, int64_t);                       \
    template int sample_smooth_bodies_image_tiled<T, NI, NO>(hipStream_t, const int64_t*, int64_t, int64_t, int64_t, \
                                                             int, int, T*, const T*, const T*, const int32_t*,      \
                                                             const T*, const T*, void*, size_t);
#define DPR_SAMPLE_SMOOTH_BODIES_INSTANTIATE_T(T)                                                  \
    DPR_SAMPLE_SMOOTH_BODIES_INSTANTIATE(T, 2, 2) DPR_SAMPLE_SMOOTH_BODIES_INSTANTIATE(T, 3, 3) \
    DPR_SAMPLE_SMOOTH_BODIES_INSTANTIATE(T, 3, 2)
DPR_SAMPLE_SMOOTH_BODIES_INSTANTIATE_T(float)
DPR_SAMPLE_SMOOTH_BODIES_INSTANTIATE_T(double)

}  // namespace dpr
