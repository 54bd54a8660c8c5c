// The DPR_ALGO_ATOMIC launch of the channel pullback, which dpr_api_channels.hip declares and calls.  k_bwd_gather_ch
// is the slowest kernel family of the library to compile (its 64 instantiations: a minute, most of it the 16-channel
// fp64 ones), so they are spread over the dpr_api_channels_pullback_*.hip units: each includes this header and
// instantiates its share of the (T, n_in, n_out) with DPR_CHANNELS_PULLBACK.  No build then waits on one object.
#pragma once
#include "dpr_host.h"
#include "dpr_kernels_channels.h"

namespace dpr {

template <typename T, int NI, int NO>
int pullback_atomic_channels(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, int C,
                             const T* g, const T* points, const T* rot, const T* trans, const T* ow,
                             const T* pw, T* d_pts, T* d_rot, T* d_trans, T* d_bg, T* d_ow, T* d_pw) {
    const GridDesc<NO> gd = make_grid_desc<NO>(grid, G);
    const int64_t planes = B * C;
    DPR_HIP(zero_async(st, d_rot, sizeof(T) * (size_t)(B * NO * NI)));
    DPR_HIP(zero_async(st, d_trans, sizeof(T) * (size_t)(B * NO)));
    DPR_HIP(zero_async(st, d_ow, sizeof(T) * (size_t)B));
    DPR_HIP(zero_async(st, d_bg, sizeof(T) * (size_t)planes));
    // ds_dbackground[c, b] = sum of plane b * C + c: the single-channel grid sum over B * C planes
    grid_sum(st, g, G, planes, d_bg, Residual<T>{nullptr, T(0), nullptr});
    stage_mark(st);
    if (P > 0) {
        const int64_t pblocks = (P + kBlock - 1) / kBlock;
        int64_t slices = 1;
        const int poses_per_slice = pose_slices(P, B, &slices);
        const int accumulate = slices > 1;
        if (accumulate) {
            DPR_HIP(zero_async(st, d_pts, sizeof(T) * (size_t)(P * NI)));
            if (d_pw) DPR_HIP(zero_async(st, d_pw, sizeof(T) * (size_t)(P * C)));
        }
        dim3 gg((unsigned)pblocks, (unsigned)slices);
        if (C <= 4)
            hipLaunchKernelGGL((k_bwd_gather_ch<T, NI, NO, 4>), gg, dim3(kBlock), 0, st, gd, P, B, C, g, points,
                               rot, trans, ow, pw, d_pts, d_rot, d_trans, d_ow, d_pw, poses_per_slice, accumulate);
        else
            hipLaunchKernelGGL((k_bwd_gather_ch<T, NI, NO, kMaxChannels>), gg, dim3(kBlock), 0, st, gd, P, B, C,
                               g, points, rot, trans, ow, pw, d_pts, d_rot, d_trans, d_ow, d_pw, poses_per_slice,
                               accumulate);
    }
    stage_mark(st);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

#define DPR_CHANNELS_PULLBACK(T, NI, NO)                                                                            \
    template int pullback_atomic_channels<T, NI, NO>(hipStream_t, const int64_t*, int64_t, int64_t, int64_t, int,   \
                                                     const T*, const T*, const T*, const T*, const T*, const T*,    \
                                                     T*, T*, T*, T*, T*, T*);
// every n_in of one n_out
#define DPR_CHANNELS_PULLBACK_OUT(T, NO)                            \
    DPR_CHANNELS_PULLBACK(T, 1, NO) DPR_CHANNELS_PULLBACK(T, 2, NO) \
    DPR_CHANNELS_PULLBACK(T, 3, NO) DPR_CHANNELS_PULLBACK(T, 4, NO)

}  // namespace dpr
