// Rigid bodies (dpr_raster_bodies_ex_* / dpr_raster_pullback_bodies_ex_*, include/dpr.h "RIGID BODIES"): one cloud
// whose point p belongs to body[p] in [0, K) and is seen in image b through pose (b, body[p]), stored at index
// b * K + body[p].  The kernels are k_fwd_atomic / k_bwd_gather (dpr_kernels_atomic.h) with that pose index; what
// the index changes:
//   the pose load       a wave whose accepted lanes share one body (the caller sorts the cloud by body) passes the
//                       index through readfirstlane and keeps the scalar pose loads of the core kernels; a mixed
//                       wave gathers its poses with vector loads.  One ballot per wave, taken once: the body of a
//                       point does not depend on the image.
//   the per-body sums   ds_drotation / ds_dtranslation are per (image, body).  A block whose accepted lanes all
//                       share one body reduces wave -> block -> one atomic per value, as k_bwd_gather does.
//                       Otherwise every wave works alone and walks its bodies: mask the lanes of the first live
//                       lane's body, masked wave_sum, one atomic per value, clear the lanes, repeat.
//                       ds_dout_weight is per image and always goes wave -> block -> one atomic.
//                       There is no switch to one atomic per value and LANE for waves of many bodies: measured, it
//                       loses to the walk at every number of distinct bodies per wave (profiles/bodies_probe.txt,
//                       "crossover": at 40.7 of 64 lanes distinct 7.9 against 6.0 ms, at 4.0 -- every lane of the
//                       device on the same 4 x 9 addresses -- 74 against 4.0 ms; 1e6 points x 16 poses -> 512^2).
// A point whose body index lies outside [0, K) is dropped like a point outside the grid: the index is checked per
// lane before it addresses anything.
#pragma once
#include "dpr_device.h"

namespace dpr {

// What a wave knows about the bodies of its lanes (the same for every pose).
struct WaveBodies {
    bool ok;        // this lane holds a point of the cloud with a body in [0, K)
    int k;          // its body (0 for a lane that is not ok: a valid index, never deposited)
    int first;      // the body of the first ok lane, wave-uniform (0 without one)
    int distinct;   // bodies among the ok lanes, wave-uniform: 0, 1, or 2 for several
};

__device__ __forceinline__ int lane_value(int v, int lane) {
    return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(lane));
}

// All 64 lanes must call.
__device__ __forceinline__ WaveBodies wave_bodies(const int32_t* __restrict__ body, int64_t p, int64_t P, int K) {
    WaveBodies w;
    const int kb = p < P ? body[p] : -1;
    w.ok = (unsigned)kb < (unsigned)K;  // (K <= 2^31 - 1: negative indices fail the unsigned comparison)
    w.k = w.ok ? kb : 0;
    const uint64_t live = __builtin_amdgcn_ballot_w64(w.ok);
    w.first = live ? lane_value(w.k, __ffsll((unsigned long long)live) - 1) : 0;
    w.distinct = live ? (__builtin_amdgcn_ballot_w64(w.ok && w.k != w.first) ? 2 : 1) : 0;
    return w;
}

// Pose (b, k) of a lane; out_weight is per image.  Where the wave's ok lanes share body `first` the index is
// wave-uniform and the loads are scalar.
template <typename T, int NI, int NO>
__device__ __forceinline__ Pose<T, NI, NO> load_body_pose(const T* __restrict__ rot, const T* __restrict__ trans,
                                                         const T* __restrict__ ow, int64_t b, int K,
                                                         const WaveBodies& w) {
    Pose<T, NI, NO> ps;
    if (w.distinct <= 1)
        ps = load_pose<T, NI, NO>(rot, trans, nullptr, b * K + __builtin_amdgcn_readfirstlane(w.first));
    else
        ps = load_pose<T, NI, NO>(rot, trans, nullptr, b * K + w.k);
    ps.ow = ow ? ow[b] : T(1);
    return ps;
}

// Forward: one thread per point, the pose loop striding over blockIdx.y.  `out` holds the background.
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kBlock) void k_bodies_fwd(GridDesc<NO> gd, int64_t P, int64_t B, int K,
                                                       T* __restrict__ out, const T* __restrict__ points,
                                                       const int32_t* __restrict__ body,
                                                       const T* __restrict__ rot, const T* __restrict__ trans,
                                                       const T* __restrict__ ow, const T* __restrict__ pw) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const WaveBodies w = wave_bodies(body, p, P, K);
    if (w.distinct == 0) return;  // (the whole wave: no lane has a point to deposit)
    T pt[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) pt[j] = T(0);
    if (w.ok) load_point<T, NI>(points, p, pt);
    const T pwi = (w.ok && pw) ? pw[p] : T(1);
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        const Pose<T, NI, NO> ps = load_body_pose<T, NI, NO>(rot, trans, ow, b, K, w);
        int ref0[NO];
        T dlo[NO];
        if (!(w.ok && ref_and_deltas<T, NI, NO>(pt, ps, gd, ref0, dlo))) continue;
        const T wt = ps.ow * pwi;  // as k_fwd_atomic
        T* o = out + b * gd.G;
#pragma unroll
        for (int s = 0; s < (1 << NO); ++s) {
            const int off = nbr_offset<NO>(ref0, s, gd);
            if (off >= 0) atomic_add<T>(o + off, voxel_weight<T, NO>(dlo, s, wt));
        }
    }
}

// Pullback over the pose range [b_lo, b_hi) of blockIdx.y.  Pre-zeroed: ds_drotation, ds_dtranslation (B * K poses),
// ds_dout_weight.  ds_dpoints / ds_dpoint_weight: plain stores when `accumulate_points` is 0 (one launch covers all
// poses), atomics onto pre-zeroed buffers otherwise -- as k_bwd_gather, whose operation order per (point, pose)
// this kernel keeps.
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kBlock) void k_bodies_bwd(
    GridDesc<NO> gd, int64_t P, int64_t B, int K, const T* __restrict__ g, const T* __restrict__ points,
    const int32_t* __restrict__ body, const T* __restrict__ rot, const T* __restrict__ trans,
    const T* __restrict__ ow, const T* __restrict__ pw, T* __restrict__ ds_dpoints, T* __restrict__ ds_drotation,
    T* __restrict__ ds_dtranslation, T* __restrict__ ds_dout_weight, T* __restrict__ ds_dpoint_weight,
    int poses_per_slice, int accumulate_points) {
    constexpr int NR = NO * NI + NO;  // dR | dt: per (pose, body)
    constexpr int NV = NR + 1;        // | d out_weight: per pose
    constexpr int NW = kBlock / kWave;
    __shared__ T red[NW][NV];
    __shared__ int wave_body[NW];

    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = p < P;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    const WaveBodies w = wave_bodies(body, p, P, K);
    // the block's body: -1 no accepted lane in the block, -2 more than one body, else the body all of them share
    if (lane == 0) wave_body[wave] = w.distinct == 0 ? -1 : (w.distinct == 1 ? w.first : -2);
    __syncthreads();
    int block_body = -1;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const int wb = wave_body[i];
        if (wb == -1) continue;
        block_body = (block_body == -1 || block_body == wb) ? wb : -2;
    }
    block_body = __builtin_amdgcn_readfirstlane(block_body);

    T pt[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) pt[j] = T(0);
    if (w.ok) load_point<T, NI>(points, p, pt);
    const T pwi = (w.ok && pw) ? pw[p] : T(1);
    T acc_pt[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) acc_pt[j] = T(0);
    T acc_pw = T(0);

    const int64_t b_lo = (int64_t)blockIdx.y * poses_per_slice;
    const int64_t b_hi = (b_lo + poses_per_slice < B) ? b_lo + poses_per_slice : B;
    for (int64_t b = b_lo; b < b_hi; ++b) {
        const Pose<T, NI, NO> ps = load_body_pose<T, NI, NO>(rot, trans, ow, b, K, w);
        T vals[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) vals[i] = T(0);
        int ref0[NO];
        T dlo[NO];
        if (w.ok && ref_and_deltas<T, NI, NO>(pt, ps, gd, ref0, dlo)) {
            const int64_t gb = b * gd.G;
            T scaled[NO], dow_part, dpw_part;
            point_backward<T, NI, NO>(ref0, dlo, gd, ps.ow, pwi, [&](int off) { return g[gb + off]; }, scaled,
                                      dow_part, dpw_part);
#pragma unroll
            for (int n = 0; n < NO; ++n) {
#pragma unroll
                for (int j = 0; j < NI; ++j) vals[n + j * NO] = scaled[n] * pt[j];
                vals[NO * NI + n] = scaled[n];
            }
            vals[NR] = dow_part;
#pragma unroll
            for (int j = 0; j < NI; ++j) {  // rotation' * scaled
                T v = ps.R[0 + j * NO] * scaled[0];
#pragma unroll
                for (int n = 1; n < NO; ++n) v = v + ps.R[n + j * NO] * scaled[n];
                acc_pt[j] += v;
            }
            acc_pw += dpw_part;
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
            uint64_t rest = __builtin_amdgcn_ballot_w64(w.ok);
            while (rest) {
                const int kc = lane_value(w.k, __ffsll((unsigned long long)rest) - 1);
                const bool mine = w.ok && w.k == kc;
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

}  // namespace dpr
