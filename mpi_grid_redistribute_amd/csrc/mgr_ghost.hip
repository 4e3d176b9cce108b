// Ghost-cell lists over owned + halo rows: the two kernels
// between the halo exchange and the ranked fine sort.
//
//  * shift_regions_kernel (mgr_shift_regions): rows [end[r-1], end[r]) of a
//    position array get pos[row][d] += (T)shift[r][d], one add in the
//    positions' own type.  The halo exchange calls it on the rows a periodic
//    wrap brought in, so a halo row's position is the image next to this
//    rank's cell (x + L or x - L), not the owner's.
//  * ghost_cells_kernel (mgr_ghost_cells): the cell of every row in the
//    extended grid of fine + 2 * ghost cells per dimension, as the uint16 ids
//    mgr_rank_ids / mgr_count_ids sort by; as uint32 ids for grids beyond 1024
//    cells (mgr_ghost_cells_wide, §3.12), the same kernel on the id type.
#include "mgr_device.h"

namespace mgr {

// ------------------------------------------------------- shift regions
// Element-centric: a workgroup walks slabs of slab_rows rows; thread t takes
// the slab's elements t, t + 256, ... (consecutive lanes, consecutive
// addresses: the loads and stores of a round are contiguous whatever the
// stride), finds the element's row and column with one 32-bit float multiply
// (exact after the +-1 fix-up: slab_rows * stride <= 2^22), the row's region
// by bisection of the staged ends, and stores x + shift only where the shift
// is not zero.  Columns >= dim and zero-shift coordinates are neither stored
// nor, for whole zero regions at either end of the call, read (the launcher
// trims them).  slab_rows == 1 (a stride beyond 2^22): the slab is the row's
// first dim elements.
template <typename T>
__global__ __launch_bounds__(kBlock) void shift_regions_kernel(T* __restrict__ pos,
                                                               int64_t row_begin, int64_t row_end,
                                                               int64_t stride, int dim, int nreg,
                                                               int slab_rows, ShiftTable tab) {
    __shared__ int64_t s_end[kMaxRegions];
    __shared__ T s_shift[kShiftVals];
    if ((int)threadIdx.x < nreg) s_end[threadIdx.x] = tab.end[threadIdx.x];
    for (int i = threadIdx.x; i < nreg * dim; i += kBlock) s_shift[i] = (T)tab.shift[i];
    __syncthreads();
    const unsigned su = (unsigned)stride;            // read only when slab_rows > 1
    const float inv = 1.0f / (float)su;
    const int64_t step = (int64_t)gridDim.x * slab_rows;
    for (int64_t s0 = row_begin + (int64_t)blockIdx.x * slab_rows; s0 < row_end; s0 += step) {
        const unsigned rows = (unsigned)min((int64_t)slab_rows, row_end - s0);
        const unsigned ne = slab_rows == 1 ? (unsigned)dim : rows * su;
        T* base = pos + s0 * stride;
        for (unsigned e = threadIdx.x; e < ne; e += kBlock) {
            unsigned row = 0, col = e;
            if (slab_rows > 1) {
                row = (unsigned)((float)e * inv);
                if (row * su > e) --row;
                else if ((row + 1u) * su <= e) ++row;
                col = e - row * su;
            }
            if (col >= (unsigned)dim) continue;
            const int64_t r = s0 + row;
            int lo = 0, hi = nreg - 1;               // first region with r < end (end[nreg-1] > r)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (r < s_end[mid]) hi = mid;
                else lo = mid + 1;
            }
            const T sh = s_shift[lo * dim + (int)col];
            if (sh != T(0)) base[e] = base[e] + sh;
        }
    }
}

template <typename T>
static void shift_t(void* pos, int64_t r0, int64_t r1, int64_t stride, int dim, int nreg,
                    const ShiftTable& tab, hipStream_t s) {
    const int64_t cap = (int64_t)1 << 22;
    const int slab = stride <= cap ? (int)max((int64_t)1, min((int64_t)1024, cap / stride)) : 1;
    hipLaunchKernelGGL(shift_regions_kernel<T>, dim3(grid_for(r1 - r0, slab)), dim3(kBlock), 0, s,
                       (T*)pos, r0, r1, stride, dim, nreg, slab, tab);
}

// Regions go to the kernel by value, kShiftVals shift values at a time (64
// regions of up to 3 dimensions in one launch); regions whose shifts are all
// zero, or that are empty, at either end of a launch are trimmed away, and a
// launch left with nothing is not made.
hipError_t launch_shift_regions(void* pos, int pos_dtype, int64_t n, int64_t stride, int dim,
                                int nregions, const int64_t* region_end, const double* shift,
                                hipStream_t s) {
    if (n <= 0) return hipSuccess;
    auto live = [&](int k) {
        const int64_t b = k ? region_end[k - 1] : 0;
        if (region_end[k] <= b) return false;
        for (int d = 0; d < dim; ++d)
            if (pos_dtype == MGR_F32 ? (float)shift[k * dim + d] != 0.0f : shift[k * dim + d] != 0.0)
                return true;
        return false;
    };
    const int per = max(1, min(kMaxRegions, kShiftVals / dim));
    for (int k0 = 0; k0 < nregions; k0 += per) {
        int a = k0, b = min(nregions, k0 + per);
        while (a < b && !live(a)) ++a;
        while (b > a && !live(b - 1)) --b;
        if (a == b) continue;
        ShiftTable tab{};
        for (int k = a; k < b; ++k) {
            tab.end[k - a] = region_end[k];
            for (int d = 0; d < dim; ++d) tab.shift[(k - a) * dim + d] = shift[k * dim + d];
        }
        const int64_t r0 = a ? region_end[a - 1] : 0, r1 = region_end[b - 1];
        if (pos_dtype == MGR_F32) shift_t<float>(pos, r0, r1, stride, dim, b - a, tab, s);
        else shift_t<double>(pos, r0, r1, stride, dim, b - a, tab, s);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// --------------------------------------------------------- ghost cells
// Row-centric, lane = row in 64-row rounds (halo_flags_kernel's and the
// unstaged bin_count_kernel's position loads: lane l reads its row's dim
// coordinates at row * stride, neighbouring lanes neighbouring rows, every
// cache line of a round read whole).  Per coordinate, in float64:
//   k = floor((x - origin) / width) + ghost
// clamped in the double domain (no integer conversion of an unbounded value)
// to the interior [ghost, ghost + fine - 1] for owned rows, to the extended
// grid [0, ext - 1] for the others; a NaN takes the lower bound.  A clamp
// that changed a halo row's k (NaN included) counts the row once into
// *outside: one ballot per round, one vector atomic add by the round's first
// lane when the round has any.  A full round's ids go out as 16 8-byte stores
// (uint16 ids: lane 4k gathers lanes 4k..4k+3, as the binning's side field) or
// 16 16-byte stores (uint32 ids, mgr_ghost_cells_wide: the same gather).

// The one per-row arithmetic of mgr_ghost_cells and mgr_ghost_cells_wide: the
// row's cell id; *out: a halo row whose k a clamp changed.
template <typename T, int DIM>
__device__ __forceinline__ unsigned ghost_cell_of(const T* __restrict__ p, bool owned, int dim_rt,
                                                  const GhostGeom& g, bool* out) {
    const int dim = DIM > 0 ? DIM : dim_rt;
    unsigned id = 0;
    bool o = false;
#pragma unroll
    for (int d = 0; d < dim; ++d) {
        const double x = (double)p[d];
        const double kd = floor((x - g.origin[d]) / g.width[d]) + (double)g.ghost[d];
        const int lo = owned ? g.ghost[d] : 0;
        const int hi = owned ? g.ghost[d] + g.fine[d] - 1 : g.ext[d] - 1;
        int k;
        if (!(kd >= (double)lo)) k = lo;           // below, or NaN
        else if (kd > (double)hi) k = hi;
        else k = (int)kd;
        o = o || (!owned && !(kd >= (double)lo && kd <= (double)hi));
        id += (unsigned)k * (unsigned)g.off[d];
    }
    *out = o;
    return id;
}

template <typename T, int DIM, typename IdT>
__global__ __launch_bounds__(kBlock) void ghost_cells_kernel(const T* __restrict__ pos, int64_t n,
                                                             int64_t n_owned, int64_t stride,
                                                             int dim_rt, GhostGeom g,
                                                             IdT* __restrict__ ids,
                                                             uint32_t* __restrict__ outside) {
    constexpr bool kWide = sizeof(IdT) == 4;
    const int lane = lane_id();
    const bool idsv = ((uintptr_t)ids & (kWide ? 15 : 7)) == 0;   // 4 ids per vector store
    const int64_t step = (int64_t)gridDim.x * kBlock;
    for (int64_t r0 = (int64_t)blockIdx.x * kBlock + (threadIdx.x & ~63); r0 < n; r0 += step) {
        const int64_t r = r0 + lane;
        const bool valid = r < n;
        unsigned id = 0;
        bool out = false;
        if (valid) id = ghost_cell_of<T, DIM>(pos + r * stride, r < n_owned, dim_rt, g, &out);
        if (idsv && n - r0 >= 64) {
            const unsigned v1 = __shfl_down(id, 1, 64), v2 = __shfl_down(id, 2, 64),
                           v3 = __shfl_down(id, 3, 64);
            if ((lane & 3) == 0) {
                if constexpr (kWide)
                    *(uint4*)(ids + r) = make_uint4(id, v1, v2, v3);
                else
                    *(uint2*)(ids + r) = make_uint2((id & 0xffffu) | (v1 << 16),
                                                    (v2 & 0xffffu) | (v3 << 16));
            }
        } else if (valid) {
            ids[r] = (IdT)id;
        }
        if (outside) {
            const unsigned long long b = __ballot(out);
            if (b && lane == __builtin_ctzll(b)) atomicAdd(outside, (uint32_t)__popcll(b));
        }
    }
}

template <typename T, typename IdT>
static void ghost_t(const void* pos, int64_t n, int64_t n_owned, int64_t stride, int dim,
                    const GhostGeom& g, IdT* ids, uint32_t* outside, hipStream_t s) {
    auto k = dim == 1 ? ghost_cells_kernel<T, 1, IdT> : dim == 2 ? ghost_cells_kernel<T, 2, IdT>
           : dim == 3 ? ghost_cells_kernel<T, 3, IdT> : ghost_cells_kernel<T, 0, IdT>;
    hipLaunchKernelGGL(k, dim3(grid_for(n)), dim3(kBlock), 0, s, (const T*)pos, n, n_owned, stride,
                       dim, g, ids, outside);
}

hipError_t launch_ghost_cells(const void* pos, int pos_dtype, int64_t n, int64_t n_owned,
                              int64_t stride, int dim, const GhostGeom& g, uint16_t* ids,
                              uint32_t* outside, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (pos_dtype == MGR_F32) ghost_t<float>(pos, n, n_owned, stride, dim, g, ids, outside, s);
    else ghost_t<double>(pos, n, n_owned, stride, dim, g, ids, outside, s);
    return hipGetLastError();
}

hipError_t launch_ghost_cells_wide(const void* pos, int pos_dtype, int64_t n, int64_t n_owned,
                                   int64_t stride, int dim, const GhostGeom& g, uint32_t* ids,
                                   uint32_t* outside, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    prof_begin(s, K_GHOST_WIDE);
    if (pos_dtype == MGR_F32) ghost_t<float>(pos, n, n_owned, stride, dim, g, ids, outside, s);
    else ghost_t<double>(pos, n, n_owned, stride, dim, g, ids, outside, s);
    prof_end(s, K_GHOST_WIDE);
    return hipGetLastError();
}

}  // namespace mgr
