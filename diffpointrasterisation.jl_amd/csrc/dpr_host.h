// Host-side helpers that cross a boundary between the API translation units (dpr_api.hip and dpr_api_*.hip, one per
// op family): declared here, defined once in the unit named above each group.  Everything else in those units is
// static.  fail, stage_mark and DPR_HIP, which the algorithm units use too, come with dpr_tiled.h.
#pragma once
#include <initializer_list>
#include <type_traits>

#include "../../include/dpr.h"
#include "dpr_tiled.h"

namespace dpr {

// ---------------------------------------------------------------- dpr_api.hip
// (constexpr: `if constexpr` keeps the other algorithms' templates to these three pairs)
constexpr bool dims_have_all_algos(int n_in, int n_out) {
    return (n_in == 2 && n_out == 2) || (n_in == 3 && n_out == 3) || (n_in == 3 && n_out == 2);
}

// f(std::integral_constant<int, NI>{}, std::integral_constant<int, NO>{}) for the runtime pair: the one place
// that maps (n_in, n_out) to template arguments.  Callers have passed check_common, so the pair is supported.
template <int NI, class F> int with_out_dim(int n_out, F& f) {
    using NIc = std::integral_constant<int, NI>;
    switch (n_out) {
        case 1: return f(NIc{}, std::integral_constant<int, 1>{});
        case 2: return f(NIc{}, std::integral_constant<int, 2>{});
        case 3: return f(NIc{}, std::integral_constant<int, 3>{});
        case 4: return f(NIc{}, std::integral_constant<int, 4>{});
    }
    return fail(DPR_ERR_UNSUPPORTED_DIMS, "unsupported (n_in, n_out) = (%d, %d)", NI, n_out);
}
template <class F> int with_dims(int n_in, int n_out, F&& f) {
    switch (n_in) {
        case 1: return with_out_dim<1>(n_out, f);
        case 2: return with_out_dim<2>(n_out, f);
        case 3: return with_out_dim<3>(n_out, f);
        case 4: return with_out_dim<4>(n_out, f);
    }
    return fail(DPR_ERR_UNSUPPORTED_DIMS, "unsupported (n_in, n_out) = (%d, %d)", n_in, n_out);
}

// The kernels move records as 16/32-byte vectors and scalars as T: a misaligned pointer
// would fault on the device, so it is refused here.
template <typename T>
int check_alignment(const void* ws, std::initializer_list<const void*> data) {
    if (ws && ((uintptr_t)ws & 255))
        return fail(DPR_ERR_WORKSPACE, "workspace must be 256-byte aligned");
    uintptr_t bits = 0;
    for (const void* p : data) bits |= (uintptr_t)p;  // NULL (optional argument) adds nothing
    if (bits & (sizeof(T) - 1))
        return fail(DPR_ERR_INVALID_ARG, "a data pointer is not aligned to its element type");
    return DPR_OK;
}
// (the body index of a point, the rigid-body families' int32_t array; NULL where the family has none)
inline int check_body_alignment(const void* body) {
    return ((uintptr_t)body & 3) ? fail(DPR_ERR_INVALID_ARG, "body is not aligned to its element type (int32_t)")
                                 : DPR_OK;
}

int check_common(int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B, int64_t* G_out);
// (a launch of one thread per point counts its blocks of kBlock points in 31 bits)
inline int check_point_blocks(int64_t P) {
    return P / kBlock + (P % kBlock != 0) > 0x7fffffffLL ? fail(DPR_ERR_INVALID_ARG, "P too large") : DPR_OK;
}
int resolve_algo(int algo, int op, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B, int64_t G,
                 unsigned* flags);
int pose_slices(int64_t P, int64_t B, int64_t* slices_out);
// (instantiated for float and double: their kernels are compiled in dpr_api.hip only)
template <typename T> void fill_background(hipStream_t st, T* out, int64_t G, int64_t planes, const T* bg);
template <typename T> void grid_sum(hipStream_t st, const T* g, int64_t G, int64_t planes, T* d_bg, Residual<T> rs);

// ---------------------------------------------------------------- dpr_api_sample.hip
int check_sample_sizes(int64_t P, int64_t B, int64_t G);

// ---------------------------------------------------------------- dpr_api_jvp.hip
int check_jvp(int64_t K, unsigned flags);
// k_jvp_fill: plane b * K + k of out_dot = bg_dot[k * B + b] (0 without bg_dot), in launches of at most 65535 planes
// (instantiated for float and double)
template <typename T> void jvp_fill(hipStream_t st, T* out_dot, int64_t G, int K, int64_t B, const T* bg_dot);

}  // namespace dpr
