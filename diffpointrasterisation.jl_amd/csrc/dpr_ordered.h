// DPR_ALGO_ORDERED entry points (dpr_ordered.hip) as dpr_api.hip, the core of the API layer, calls them
#pragma once
#include "dpr_tiled.h"

namespace dpr {

// dpr_sort.hip: the library's one rocPRIM instantiation, radix_sort_pairs<uint32, uint32> (stable), on key
// bits [begin_bit, end_bit)
size_t radix_pairs_temp_bytes(int64_t P);
hipError_t radix_sort_pairs_u32(void* temp, size_t temp_bytes, uint32_t* keys_in, uint32_t* keys_out,
                                uint32_t* vals_in, uint32_t* vals_out, size_t n, unsigned begin_bit,
                                unsigned end_bit, hipStream_t st);

// the extended grid fits the 32-bit key space and P <= 2^32 - 2
bool ordered_supported(int n_out, const int64_t* grid, int64_t P);
// bytes of workspace of `op` (DPR_OP_RASTER / DPR_OP_PULLBACK), or (size_t)-1 where !ordered_supported
size_t ordered_workspace_bytes(int op, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B);

template <typename T, int NI, int NO>
int raster_ordered(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, T* out, const T* points,
                   const T* rot, const T* trans, const T* bg, const T* ow, const T* pw, void* ws, size_t ws_bytes);

template <typename T, int NI, int NO>
int pullback_ordered(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, const T* g,
                     const T* points, const T* rot, const T* trans, const T* ow, const T* pw, T* d_pts, T* d_rot,
                     T* d_trans, T* d_bg, T* d_ow, T* d_pw, void* ws, size_t ws_bytes, Residual<T> rs);

}  // namespace dpr
