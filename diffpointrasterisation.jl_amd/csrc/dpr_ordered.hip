// DPR_ALGO_ORDERED: every sum in a fixed order, so that every output is bit-reproducible (include/dpr.h,
// SUMMATION ORDER).  No floating-point atomic in this file; every output and every partial has one writer and
// one store.
//
//   forward, pose by pose on the stream (the per-pose workspace is reused):
//     k_ord_keys    one thread per point: the key of its reference cell on the extended grid (all ones for a
//                   rejected point), value = point index
//     radix sort    stable, on the key bits the extended grid needs: ascending point index inside a cell
//     k_ord_ranges  one thread per entry of the start table (GE + 1 entries): a lower-bound search on the sorted
//                   keys -- one writer per entry
//     k_ord_gather  one thread per output cell: merges the <= 2^N index-sorted lists of its source cells by point
//                   index and adds the one neighbour of each point that lands on the cell, starting from the
//                   background: the order of the serial reference (oracle_raster).  One plain store.
//   pullback:
//     k_ord_grid_sum  ds_dbackground / loss partials: fixed chunks of kOrdCellChunk consecutive cells
//     k_ord_bwd       k_bwd_gather's body with the pose loop always inside the thread over ALL poses (point
//                     gradients: registers, poses in index order, one store) and the per-pose sums reduced per fixed
//                     chunk of kOrdPointChunk consecutive points into one f64 slot per (chunk, pose, scalar)
//     k_ord_reduce    one block per (pose, scalar): the chunk partials staged through LDS and added by one thread
//                     in ascending chunk order in f64, one store
#include <hip/hip_runtime.h>

#include "../../include/dpr.h"
#include "dpr_ordered.h"
#include "dpr_ordered_index.h"

namespace dpr {

constexpr int kOrdBlock = 256;
constexpr int kOrdPointChunk = DPR_ORDERED_POINT_CHUNK;
constexpr int kOrdCellChunk = DPR_ORDERED_CELL_CHUNK;
static_assert(kOrdPointChunk % kOrdBlock == 0 && kOrdCellChunk % kOrdBlock == 0, "chunks are whole sub-steps");

// ---------------------------------------------------------------- forward
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kOrdBlock) void k_ord_keys(GridDesc<NO> gd, int64_t P, int64_t b,
                                                        const T* __restrict__ points, const T* __restrict__ rot,
                                                        const T* __restrict__ trans, uint32_t* __restrict__ keys,
                                                        uint32_t* __restrict__ idx) {
    const int64_t p = (int64_t)blockIdx.x * kOrdBlock + threadIdx.x;
    if (p >= P) return;
    T pt[NI];
    load_point<T, NI>(points, p, pt);
    const Pose<T, NI, NO> ps = load_pose<T, NI, NO>(rot, trans, nullptr, b);
    int ref0[NO];
    T dlo[NO];
    const bool ok = ref_and_deltas<T, NI, NO>(pt, ps, gd, ref0, dlo);
    keys[p] = ok ? ord_key_encode<NO>(ref0, gd.n) : kOrdNoKey;
    idx[p] = (uint32_t)p;
}

// start[k] = first position of the sorted keys with key >= k, for k = 0 .. GE (start[GE]: the accepted points)
__global__ __launch_bounds__(kOrdBlock) void k_ord_ranges(const uint32_t* __restrict__ keys, uint32_t count,
                                                          uint64_t entries, int bits, uint32_t* __restrict__ start) {
    const uint64_t k = (uint64_t)blockIdx.x * kOrdBlock + threadIdx.x;
    if (k >= entries) return;
    start[k] = ord_lower_bound(keys, count, (uint32_t)k, bits);
}

// `start` == nullptr: no points (P = 0), the plane is its background
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kOrdBlock) void k_ord_gather(GridDesc<NO> gd, int64_t P, int64_t b, T* __restrict__ out,
                                                          const T* __restrict__ points, const T* __restrict__ rot,
                                                          const T* __restrict__ trans, const T* __restrict__ bg,
                                                          const T* __restrict__ ow, const T* __restrict__ pw,
                                                          const uint32_t* __restrict__ start,
                                                          const uint32_t* __restrict__ idx) {
    const int64_t cell = (int64_t)blockIdx.x * kOrdBlock + threadIdx.x;
    if (cell >= gd.G) return;
    T acc = bg ? bg[b] : T(0);
    if (start) {
        const Pose<T, NI, NO> ps = load_pose<T, NI, NO>(rot, trans, ow, b);
        int c[NO];
        ord_cell_coords<NO>((uint32_t)cell, gd.n, c);
        ord_merge_walk<NO>(c, gd.n, start, idx, (uint32_t)P, [&](uint32_t p, int s) {
            if ((int64_t)p >= P) return;  // (never for an index k_ord_keys wrote)
            T pt[NI];
            load_point<T, NI>(points, (int64_t)p, pt);
            const T w = ps.ow * (pw ? pw[p] : T(1));  // src/raster.jl:52
            int ref0[NO];
            T dlo[NO];
            if (ref_and_deltas<T, NI, NO>(pt, ps, gd, ref0, dlo)) acc += voxel_weight<T, NO>(dlo, s, w);
        });
    }
    out[b * gd.G + cell] = acc;
}

// ---------------------------------------------------------------- pullback
// part[(b * chunks + chunk) * 2 + {0, 1}] = sum of ds_dout (of the residual's sensitivity) | of (out - target)^2
// over the chunk's cells: per-thread sums in T over the sub-steps in order, wave_sum, waves in index order
template <typename T>
__global__ __launch_bounds__(kOrdBlock) void k_ord_grid_sum(const T* __restrict__ g, int64_t G, int64_t chunks,
                                                            double* __restrict__ part, Residual<T> rs) {
    constexpr int NW = kOrdBlock / kWave;
    __shared__ T red[2][NW];
    const int64_t b = blockIdx.y, chunk = blockIdx.x;
    const int64_t o = b * G;
    T acc = T(0), sq = T(0);
    for (int j = 0; j < kOrdCellChunk / kOrdBlock; ++j) {
        const int64_t i = chunk * kOrdCellChunk + (int64_t)j * kOrdBlock + threadIdx.x;
        if (i >= G) break;
        const T x = g[o + i];
        if (rs.target) {
            const T d = x - rs.target[o + i];
            acc += rs.scale * d;
            sq += d * d;
        } else {
            acc += x;
        }
    }
    acc = wave_sum<T>(acc);
    sq = wave_sum<T>(sq);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        red[0][threadIdx.x / kWave] = acc;
        red[1][threadIdx.x / kWave] = sq;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        T s = red[threadIdx.x][0];
#pragma unroll
        for (int w = 1; w < NW; ++w) s += red[threadIdx.x][w];
        part[(b * chunks + chunk) * 2 + threadIdx.x] = (double)s;
    }
}

// One block per chunk of kOrdPointChunk consecutive points, walked in sub-steps of kOrdBlock points.  Per
// sub-step a thread holds one point in registers across ALL poses.  The per-pose terms of a sub-step are reduced
// in T (wave_sum, then the waves in index order) and added, in T and in sub-step order, into the chunk's slot
// part[(chunk * B + b) * NV + k] by the one thread that owns scalar k -- a fixed tree that depends on nothing but
// kOrdPointChunk and kOrdBlock.
template <typename T, int NI, int NO>
__global__ __launch_bounds__(kOrdBlock) void k_ord_bwd(GridDesc<NO> gd, int64_t P, int64_t B, const T* __restrict__ g,
                                                       const T* __restrict__ points, const T* __restrict__ rot,
                                                       const T* __restrict__ trans, const T* __restrict__ ow,
                                                       const T* __restrict__ pw, T* __restrict__ ds_dpoints,
                                                       T* __restrict__ ds_dpoint_weight, double* part,
                                                       Residual<T> rs) {
    constexpr int NV = NO * NI + NO + 1;  // dR | dt | d out_weight
    constexpr int NW = kOrdBlock / kWave;
    __shared__ T red[NW][NV];
    const int64_t chunk = blockIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    for (int j = 0; j < kOrdPointChunk / kOrdBlock; ++j) {
        const int64_t p0 = chunk * kOrdPointChunk + (int64_t)j * kOrdBlock;
        if (p0 >= P) break;  // (uniform; sub-step 0 of a chunk always holds a point)
        const int64_t p = p0 + threadIdx.x;
        const bool live = p < P;
        T pt[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) pt[i] = T(0);
        if (live) load_point<T, NI>(points, p, pt);
        const T pwi = (live && pw) ? pw[p] : T(1);
        T acc_pt[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) acc_pt[i] = T(0);
        T acc_pw = T(0);
        for (int64_t b = 0; b < B; ++b) {
            const Pose<T, NI, NO> ps = load_pose<T, NI, NO>(rot, trans, ow, b);
            T vals[NV];
#pragma unroll
            for (int k = 0; k < NV; ++k) vals[k] = T(0);
            int ref0[NO];
            T dlo[NO];
            if (live && ref_and_deltas<T, NI, NO>(pt, ps, gd, ref0, dlo)) {
                const int64_t gb = b * gd.G;
                T scaled[NO], dow_part, dpw_part;
                if (rs.target)  // (uniform)
                    point_backward<T, NI, NO>(
                        ref0, dlo, gd, ps.ow, pwi,
                        [&](int off) { return rs.scale * (g[gb + off] - rs.target[gb + off]); }, scaled, dow_part,
                        dpw_part);
                else
                    point_backward<T, NI, NO>(ref0, dlo, gd, ps.ow, pwi, [&](int off) { return g[gb + off]; },
                                              scaled, dow_part, dpw_part);
#pragma unroll
                for (int n = 0; n < NO; ++n) {
#pragma unroll
                    for (int i = 0; i < NI; ++i) vals[n + i * NO] = scaled[n] * pt[i];  // :69
                    vals[NO * NI + n] = scaled[n];                                      // :68
                }
                vals[NO * NI + NO] = dow_part;  // :57
#pragma unroll
                for (int i = 0; i < NI; ++i) {  // rotation' * scaled  (:70)
                    T v = ps.R[0 + i * NO] * scaled[0];
#pragma unroll
                    for (int n = 1; n < NO; ++n) v = v + ps.R[n + i * NO] * scaled[n];
                    acc_pt[i] += v;
                }
                acc_pw += dpw_part;  // :58
            }
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const T s = wave_sum<T>(vals[k]);
                if (lane == 0) red[wave][k] = s;
            }
            __syncthreads();
            if (threadIdx.x < NV) {
                T s = red[0][threadIdx.x];
#pragma unroll
                for (int w = 1; w < NW; ++w) s += red[w][threadIdx.x];
                double* slot = part + ((chunk * B + b) * NV + threadIdx.x);
                T run = j == 0 ? T(0) : (T)*slot;  // (this thread's own store of the sub-step before)
                run += s;
                *slot = (double)run;
            }
            __syncthreads();
        }
        if (live) {
#pragma unroll
            for (int i = 0; i < NI; ++i) ds_dpoints[p * NI + i] = acc_pt[i];
            if (ds_dpoint_weight) ds_dpoint_weight[p] = acc_pw;
        }
    }
}

// One block per (pose b, scalar k): k < NV -- the point-chunk partials of scalar k; k = NV: ds_dbackground; k = NV + 1:
// loss.  The block's threads fetch kOrdBlock partials at a time into LDS (the loads of one thread walking the chunks
// alone each waited for the one before: 1.1 ms at 4883 chunks); thread 0 adds them in ascending chunk order in f64.
template <typename T>
__global__ __launch_bounds__(kOrdBlock) void k_ord_reduce(int64_t B, int n_rot, int n_tr, int64_t pchunks,
                                                          int64_t gchunks, const double* __restrict__ part_pts,
                                                          const double* __restrict__ part_grid,
                                                          T* __restrict__ d_rot, T* __restrict__ d_trans,
                                                          T* __restrict__ d_ow, T* __restrict__ d_bg,
                                                          T* __restrict__ loss) {
    __shared__ double stage[kOrdBlock];
    const int NV = n_rot + n_tr + 1;
    for (int64_t t = blockIdx.x; t < B * (NV + 2); t += gridDim.x) {  // (uniform per block)
        const int64_t b = t / (NV + 2);
        const int k = (int)(t % (NV + 2));
        const bool pts = k < NV;
        const int64_t n = pts ? pchunks : gchunks;
        double s = 0.0;
        for (int64_t c0 = 0; c0 < n; c0 += kOrdBlock) {
            const int64_t c = c0 + threadIdx.x;
            double v = 0.0;
            if (c < n) v = pts ? part_pts[(c * B + b) * NV + k] : part_grid[(b * gchunks + c) * 2 + (k - NV)];
            stage[threadIdx.x] = v;
            __syncthreads();
            if (threadIdx.x == 0) {
                const int m = (int)(n - c0 < kOrdBlock ? n - c0 : kOrdBlock);
                for (int i = 0; i < m; ++i) s += stage[i];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            if (k < n_rot) d_rot[b * n_rot + k] = (T)s;
            else if (k < n_rot + n_tr) d_trans[b * n_tr + (k - n_rot)] = (T)s;
            else if (k < NV) d_ow[b] = (T)s;
            else if (k == NV) d_bg[b] = (T)s;
            else if (loss) loss[b] = (T)s;
        }
    }
}

// ---------------------------------------------------------------- host
template <int NO> static uint64_t ext_cells(const int64_t* grid) {
    int n[NO];
    for (int d = 0; d < NO; ++d) n[d] = (int)grid[d];
    return ord_ext_cells<NO>(n);
}
static uint64_t ext_cells_rt(int n_out, const int64_t* grid) {
    switch (n_out) {
        case 1: return ext_cells<1>(grid);
        case 2: return ext_cells<2>(grid);
        case 3: return ext_cells<3>(grid);
        case 4: return ext_cells<4>(grid);
    }
    return 0;
}

bool ordered_supported(int n_out, const int64_t* grid, int64_t P) {
    return ext_cells_rt(n_out, grid) != 0 && P < (int64_t)0xffffffffLL;
}

struct OrdFwdPlan {
    size_t off_keys_in, off_keys_out, off_idx_in, off_idx_out, off_temp, temp_bytes, off_start, total;
};
static OrdFwdPlan ord_fwd_plan(uint64_t ge, int64_t P) {
    OrdFwdPlan pl{};
    if (P <= 0) return pl;
    size_t o = 0;
    pl.off_keys_in = o;  o += align_up((size_t)P * 4);
    pl.off_keys_out = o; o += align_up((size_t)P * 4);
    pl.off_idx_in = o;   o += align_up((size_t)P * 4);
    pl.off_idx_out = o;  o += align_up((size_t)P * 4);
    pl.off_temp = o;
    pl.temp_bytes = radix_pairs_temp_bytes(P);
    o += align_up(pl.temp_bytes);
    pl.off_start = o;    o += align_up((size_t)(ge + 1) * 4);
    pl.total = o;
    return pl;
}
struct OrdBwdPlan {
    int64_t pchunks, gchunks;
    size_t off_pts, off_grid, total;
};
static OrdBwdPlan ord_bwd_plan(int n_in, int n_out, int64_t G, int64_t P, int64_t B) {
    OrdBwdPlan pl{};
    pl.pchunks = (P + kOrdPointChunk - 1) / kOrdPointChunk;
    pl.gchunks = (G + kOrdCellChunk - 1) / kOrdCellChunk;
    const size_t nv = (size_t)(n_out * n_in + n_out + 1);
    size_t o = 0;
    pl.off_pts = o;  o += align_up(sizeof(double) * nv * (size_t)B * (size_t)pl.pchunks);
    pl.off_grid = o; o += align_up(sizeof(double) * 2 * (size_t)B * (size_t)pl.gchunks);
    pl.total = B > 0 ? o : 0;
    return pl;
}

size_t ordered_workspace_bytes(int op, int n_in, int n_out, const int64_t* grid, int64_t P, int64_t B) {
    const uint64_t ge = ext_cells_rt(n_out, grid);
    if (ge == 0 || P >= (int64_t)0xffffffffLL) return (size_t)-1;
    if (op == DPR_OP_RASTER) return ord_fwd_plan(ge, P).total;
    int64_t G = 1;
    for (int d = 0; d < n_out; ++d) G *= grid[d];
    return ord_bwd_plan(n_in, n_out, G, P, B).total;
}

static int refuse_shape() {
    return fail(DPR_ERR_UNSUPPORTED_ALGO,
                "DPR_ALGO_ORDERED: the grid extended by one cell per axis must have at most 2^32 - 1 cells "
                "and P <= 2^32 - 2");
}

template <typename T, int NI, int NO>
int raster_ordered(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, T* out, const T* points,
                   const T* rot, const T* trans, const T* bg, const T* ow, const T* pw, void* ws_, size_t ws_bytes) {
    if (!ordered_supported(NO, grid, P)) return refuse_shape();
    const uint64_t ge = ext_cells<NO>(grid);
    const OrdFwdPlan pl = ord_fwd_plan(ge, P);
    if (pl.total > 0 && (!ws_ || ws_bytes < pl.total))
        return fail(DPR_ERR_WORKSPACE, "DPR_ALGO_ORDERED forward needs %zu workspace bytes, got %zu", pl.total,
                    ws_ ? ws_bytes : (size_t)0);
    const GridDesc<NO> gd = make_grid_desc<NO>(grid, G);
    char* ws = (char*)ws_;
    uint32_t* keys_in = (uint32_t*)(ws + pl.off_keys_in);
    uint32_t* keys_out = (uint32_t*)(ws + pl.off_keys_out);
    uint32_t* idx_in = (uint32_t*)(ws + pl.off_idx_in);
    uint32_t* idx_out = (uint32_t*)(ws + pl.off_idx_out);
    uint32_t* start = (uint32_t*)(ws + pl.off_start);
    const int bits = ord_key_bits(ge);
    const dim3 blk(kOrdBlock);
    const dim3 pgrid((unsigned)((P + kOrdBlock - 1) / kOrdBlock));
    const dim3 ggrid((unsigned)((G + kOrdBlock - 1) / kOrdBlock));
    const dim3 rgrid((unsigned)((ge + 1 + kOrdBlock - 1) / kOrdBlock));
    for (int64_t b = 0; b < B; ++b) {
        if (P > 0) {
            hipLaunchKernelGGL((k_ord_keys<T, NI, NO>), pgrid, blk, 0, st, gd, P, b, points, rot, trans, keys_in,
                               idx_in);
            stage_mark(st);
            DPR_HIP(radix_sort_pairs_u32(ws + pl.off_temp, pl.temp_bytes, keys_in, keys_out, idx_in, idx_out,
                                         (size_t)P, 0u, (unsigned)bits, st));
            stage_mark(st);
            hipLaunchKernelGGL(k_ord_ranges, rgrid, blk, 0, st, (const uint32_t*)keys_out, (uint32_t)P, ge + 1, bits,
                               start);
            stage_mark(st);
        } else {
            stage_mark(st);
            stage_mark(st);
            stage_mark(st);
        }
        hipLaunchKernelGGL((k_ord_gather<T, NI, NO>), ggrid, blk, 0, st, gd, P, b, out, points, rot, trans, bg, ow, pw,
                           P > 0 ? (const uint32_t*)start : (const uint32_t*)nullptr, (const uint32_t*)idx_out);
        stage_mark(st);
    }
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

template <typename T, int NI, int NO>
int pullback_ordered(hipStream_t st, const int64_t* grid, int64_t G, int64_t P, int64_t B, const T* g,
                     const T* points, const T* rot, const T* trans, const T* ow, const T* pw, T* d_pts, T* d_rot,
                     T* d_trans, T* d_bg, T* d_ow, T* d_pw, void* ws_, size_t ws_bytes, Residual<T> rs) {
    if (!ordered_supported(NO, grid, P)) return refuse_shape();
    const OrdBwdPlan pl = ord_bwd_plan(NI, NO, G, P, B);
    if (pl.total > 0 && (!ws_ || ws_bytes < pl.total))
        return fail(DPR_ERR_WORKSPACE, "DPR_ALGO_ORDERED pullback needs %zu workspace bytes, got %zu", pl.total,
                    ws_ ? ws_bytes : (size_t)0);
    const GridDesc<NO> gd = make_grid_desc<NO>(grid, G);
    char* ws = (char*)ws_;
    double* part_pts = (double*)(ws + pl.off_pts);
    double* part_grid = (double*)(ws + pl.off_grid);
    const dim3 blk(kOrdBlock);
    for (int64_t b0 = 0; b0 < B; b0 += 65535) {
        const int64_t nb = B - b0 < 65535 ? B - b0 : 65535;
        Residual<T> rk = rs;
        if (rk.target) rk.target += b0 * G;
        hipLaunchKernelGGL(k_ord_grid_sum<T>, dim3((unsigned)pl.gchunks, (unsigned)nb), blk, 0, st, g + b0 * G, G,
                           pl.gchunks, part_grid + b0 * pl.gchunks * 2, rk);
    }
    stage_mark(st);
    if (pl.pchunks > 0)
        hipLaunchKernelGGL((k_ord_bwd<T, NI, NO>), dim3((unsigned)pl.pchunks), blk, 0, st, gd, P, B, g, points, rot,
                           trans, ow, pw, d_pts, d_pw, part_pts, rs);
    stage_mark(st);
    constexpr int NV = NO * NI + NO + 1;
    const int64_t sums = B * (NV + 2);
    hipLaunchKernelGGL(k_ord_reduce<T>, dim3((unsigned)(sums < (1 << 20) ? sums : (1 << 20))), blk, 0, st, B,
                       NO * NI, NO, pl.pchunks, pl.gchunks, (const double*)part_pts, (const double*)part_grid, d_rot,
                       d_trans, d_ow, d_bg, rs.target ? rs.loss : (T*)nullptr);
    stage_mark(st);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

#define DPR_ORD_INSTANTIATE(T, NI, NO)                                                                            \
    template int raster_ordered<T, NI, NO>(hipStream_t, const int64_t*, int64_t, int64_t, int64_t, T*, const T*,  \
                                           const T*, const T*, const T*, const T*, const T*, void*, size_t);     \
    template int pullback_ordered<T, NI, NO>(hipStream_t, const int64_t*, int64_t, int64_t, int64_t, const T*,   \
                                             const T*, const T*, const T*, const T*, const T*, T*, T*, T*, T*,   \
                                             T*, T*, void*, size_t, Residual<T>);
#define DPR_ORD_INSTANTIATE_NI(T, NI) \
    DPR_ORD_INSTANTIATE(T, NI, 1) DPR_ORD_INSTANTIATE(T, NI, 2) DPR_ORD_INSTANTIATE(T, NI, 3) DPR_ORD_INSTANTIATE(T, NI, 4)
#define DPR_ORD_INSTANTIATE_T(T) \
    DPR_ORD_INSTANTIATE_NI(T, 1) DPR_ORD_INSTANTIATE_NI(T, 2) DPR_ORD_INSTANTIATE_NI(T, 3) DPR_ORD_INSTANTIATE_NI(T, 4)
DPR_ORD_INSTANTIATE_T(float)
DPR_ORD_INSTANTIATE_T(double)

}  // namespace dpr
