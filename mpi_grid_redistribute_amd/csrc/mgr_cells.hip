// Cell lists beyond 1024 cells: the two small kernels around
// the two-pass sort of 32-bit cell ids.
//
//  * id_digit_kernel (mgr_id_digit): one digit of the 32-bit ids as the
//    uint16 ids mgr_rank_ids / mgr_count_ids sort by.
//  * cell_offsets_kernel (mgr_cell_offsets): the first row of every cell in
//    the sorted ids, and the check of their order and range.
#include "mgr_device.h"

namespace mgr {

// ------------------------------------------------------------- id digit
// Streaming: a thread takes 8 consecutive ids as two 16-byte loads and stores
// their digits as one 16-byte store (a wave: 2 KiB read, 1 KiB written, both
// contiguous).  Groups of 8 are counted from the first 16-byte-aligned id, so
// the vector loads are aligned whatever the pointer; the ids in front of it,
// the tail behind the last whole group, and every group when `out` is not
// aligned with it, go element by element -- nothing at or beyond ids + n is
// read.
__global__ __launch_bounds__(kBlock) void id_digit_kernel(const uint32_t* __restrict__ ids,
                                                          int64_t n, int shift, unsigned mask,
                                                          uint16_t* __restrict__ out) {
    // ids before the first aligned one (0..3; ids are 4-byte aligned)
    const int64_t head = min(n, (int64_t)((16 - ((uintptr_t)ids & 15)) & 15) >> 2);
    const bool vec = ((uintptr_t)(out + head) & 15) == 0;
    const int64_t groups = (n - head + 7) >> 3;
    const int64_t step = (int64_t)gridDim.x * kBlock;
    for (int64_t gi = (int64_t)blockIdx.x * kBlock + threadIdx.x; gi < groups; gi += step) {
        const int64_t i = head + 8 * gi;
        if (vec && i + 8 <= n) {
            const uint4 a = *(const uint4*)(ids + i), b = *(const uint4*)(ids + i + 4);
            auto dg = [&](unsigned lo, unsigned hi) {
                return ((lo >> shift) & mask) | (((hi >> shift) & mask) << 16);
            };
            *(uint4*)(out + i) = make_uint4(dg(a.x, a.y), dg(a.z, a.w), dg(b.x, b.y), dg(b.z, b.w));
        } else {
            const int64_t e = min(n, i + 8);
            for (int64_t r = i; r < e; ++r) out[r] = (uint16_t)((ids[r] >> shift) & mask);
        }
    }
    if (blockIdx.x == 0 && (int64_t)threadIdx.x < head)
        out[threadIdx.x] = (uint16_t)((ids[threadIdx.x] >> shift) & mask);
}

hipError_t launch_id_digit(const uint32_t* ids, int64_t n, int shift, int bits, uint16_t* out,
                           hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const unsigned mask = bits >= 32 ? 0xffffffffu : (1u << bits) - 1u;
    prof_begin(s, K_ID_DIGIT);
    hipLaunchKernelGGL(id_digit_kernel, dim3(grid_for((n + 7) / 8 + 1)), dim3(kBlock), 0, s, ids, n,
                       shift, mask, out);
    prof_end(s, K_ID_DIGIT);
    return hipGetLastError();
}

// --------------------------------------------------------- cell offsets
// Cell-centric lower bounds, not a row-centric boundary pass: thread c finds
// the first row whose id is >= c by bisection of the sorted ids (<= 25 probes;
// the upper levels are the same few lines for every cell and stay in L2, the
// lower ones are as local as the cells are).  Every cell costs the same
// whether it is empty, holds all rows, or ends a gap of a million empty cells:
// no thread fills a gap, so there is nothing to balance.  The same grid-stride
// loop reads every id once, coalesced, with its predecessor, and counts the
// rows out of range (id >= ncells) or out of order (id < predecessor) into
// *bad: one ballot per wave and round, one vector atomic add by the first lane
// of a round that has any.  n == 0: every offset 0, nothing read.
__global__ __launch_bounds__(kBlock) void cell_offsets_kernel(const uint32_t* __restrict__ ids,
                                                              int64_t n, int64_t ncells,
                                                              int64_t* __restrict__ offsets,
                                                              uint32_t* __restrict__ bad) {
    const int lane = lane_id();
    const int64_t total = max(n, ncells + 1);
    const int64_t step = (int64_t)gridDim.x * kBlock;
    // whole waves walk the loop together (the ballot below): the bound is the
    // wave's first index
    for (int64_t i0 = (int64_t)blockIdx.x * kBlock + (threadIdx.x & ~63); i0 < total; i0 += step) {
        const int64_t i = i0 + lane;
        if (i <= ncells) {
            int64_t lo = 0, hi = n;              // first row in [0, n] with id >= i
            while (lo < hi) {
                const int64_t mid = lo + ((hi - lo) >> 1);   // < hi <= n
                if ((int64_t)ids[mid] < i) lo = mid + 1;
                else hi = mid;
            }
            offsets[i] = lo;
        }
        if (bad && i0 < n) {
            bool b = false;
            if (i < n) {
                const uint32_t v = ids[i];
                b = (int64_t)v >= ncells || (i > 0 && v < ids[i - 1]);
            }
            const unsigned long long m = __ballot(b);
            if (m && lane == __builtin_ctzll(m)) atomicAdd(bad, (uint32_t)__popcll(m));
        }
    }
}

hipError_t launch_cell_offsets(const uint32_t* sorted_ids, int64_t n, int64_t ncells,
                               int64_t* offsets, uint32_t* bad, hipStream_t s) {
    prof_begin(s, K_CELL_OFFSETS);
    hipLaunchKernelGGL(cell_offsets_kernel, dim3(grid_for(max(n, ncells + 1))), dim3(kBlock), 0, s,
                       sorted_ids, n, ncells, offsets, bad);
    prof_end(s, K_CELL_OFFSETS);
    return hipGetLastError();
}

}  // namespace mgr
