// The halo's return path (mgr_msel_unpack_add): the inverse of the
// multi-selection pack with an add.  Where mgr_msel_pack copies set k's rows,
// in row order, to dsts[k], this kernel adds srcs[k]'s rows back onto the rows
// they were selected from:
//   acc[r] += srcs[k][rank_k(r)]   for every live set k holding row r, k ascending,
// rank_k(r) = the scanned (set, tile) segment start minus the set's start, plus
// the earlier rows of the tile in the set -- the place msel_pack_kernel gave
// the row.  Nothing is counted or scanned again: flags, masks, tile_rows and
// the workspace are the forward mgr_msel_count + mgr_scan's.
//
// Row-centric, so no atomics and a fixed add order: one wave per tile_rows
// tile, four waves per workgroup (msel_count_kernel's shape), the tile walked
// in 64-row rounds with lane = row (round, lane order IS row order, so a
// ballot rank inside a round plus a running per-set count across rounds is
// the row's rank).  Lane k keeps set k's mask, source and running rank, read
// by readlane (msel_pack_kernel: no run-time index into kernel arguments in
// the loop).  Per round: the flags load coalesced (the next round's a round
// ahead); every lane's membership of the live sets as one 32-bit word; rows
// in a live set load their ncomp accumulator elements; per live set one
// ballot -- a set no lane holds costs that and a branch --, the members load
// their source row and add in the element type; one store per touched row.
// Rows in no live set are neither read nor written.
#include "mgr_device.h"

namespace mgr {

struct AddSrcs {
    const void* p[kMaxSets];
};

// NC > 0: ncomp == NC, the accumulator in NC registers; NC == 0: any ncomp,
// four components at a time (the sets are balloted once per group of four,
// the running ranks advance with the last group).
template <typename E, int NC>
__global__ __launch_bounds__(kBlock) void msel_unpack_add_kernel(
    E* __restrict__ acc, int ncomp, int64_t n, const uint16_t* __restrict__ flags, int nsets,
    SetMasks masks, AddSrcs srcs, const int64_t* __restrict__ offsets,
    const int64_t* __restrict__ set_starts, int64_t T, int tile_rows,
    const uint32_t* __restrict__ scan_err) {
    constexpr int CH = NC > 0 ? NC : 4;
    const int w = threadIdx.x >> 6, lane = lane_id();
    const int64_t tile = xcd_tile(blockIdx.x, gridDim.x) * kWaves + w;
    if (tile >= T || scan_failed(scan_err)) return;
    const int64_t row0 = tile * (int64_t)tile_rows;
    const int rows = (int)min((int64_t)tile_rows, n - row0);
    // lane k: set k's mask (0: no source, the set is not live), source and the
    // rank of the set's next row
    unsigned lmask = 0;
    unsigned long long lsrc = 0;
    long long at = 0;
    if (lane < nsets && srcs.p[lane]) {
        lmask = masks.m[lane];
        lsrc = (unsigned long long)srcs.p[lane];
        at = offsets[(int64_t)lane * T + tile] - set_starts[lane];
    }
    const uint32_t live = (uint32_t)__ballot(lmask != 0u);
    if (!live) return;
    const int nr = (rows + 63) >> 6;
    unsigned fnext = lane < rows ? flags[row0 + lane] : 0u;
    for (int q = 0; q < nr; ++q) {
        const int i = 64 * q + lane;
        const unsigned f = fnext;
        if (q + 1 < nr) fnext = i + 64 < rows ? flags[row0 + i + 64] : 0u;
        // bit k: the lane's row is in live set k (a lane past the tile's end
        // holds no flag, and no mask is empty)
        uint32_t memb = 0;
        for (uint32_t l = live; l; l &= l - 1u) {
            const int k = __builtin_ctz(l);
            const unsigned m = (unsigned)__builtin_amdgcn_readlane((int)lmask, k);
            memb |= ((f & m) == m ? 1u : 0u) << k;
        }
        const bool touched = memb != 0u;
        if (!__ballot(touched)) continue;
        E* ap = acc + (row0 + i) * (int64_t)ncomp;
        for (int c0 = 0; c0 < ncomp; c0 += CH) {
            const bool last = NC > 0 || c0 + CH >= ncomp;
            E a[CH];
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                a[c] = E(0);
                if (touched && (NC > 0 || c0 + c < ncomp)) a[c] = ap[c0 + c];
            }
            for (uint32_t l = live; l; l &= l - 1u) {
                const int k = __builtin_ctz(l);
                const bool mem = (memb >> k) & 1u;
                const unsigned long long b = __ballot(mem);
                if (!b) continue;
                const long long base = readlane64(at, k);
                const E* sp = (const E*)readlane64(lsrc, k);
                if (mem) {
                    sp += (base + rank_in(b)) * (int64_t)ncomp + c0;
#pragma unroll
                    for (int c = 0; c < CH; ++c)
                        if (NC > 0 || c0 + c < ncomp) a[c] += sp[c];
                }
                if (last && lane == k) at += __popcll(b);
            }
            if (touched) {
#pragma unroll
                for (int c = 0; c < CH; ++c)
                    if (NC > 0 || c0 + c < ncomp) ap[c0 + c] = a[c];
            }
        }
    }
}

template <typename E>
static hipError_t launch_add(E* acc, int ncomp, int64_t n, const uint16_t* flags, int nsets,
                             const SetMasks& sm, const AddSrcs& as, int tile_rows,
                             const Workspace& ws, hipStream_t s) {
    auto k = ncomp == 1 ? msel_unpack_add_kernel<E, 1> : ncomp == 2 ? msel_unpack_add_kernel<E, 2>
           : ncomp == 3 ? msel_unpack_add_kernel<E, 3> : ncomp == 4 ? msel_unpack_add_kernel<E, 4>
                        : msel_unpack_add_kernel<E, 0>;
    const int64_t grid = (ws.T + kWaves - 1) / kWaves;
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(kBlock), 0, s, acc, ncomp, n, flags, nsets,
                       sm, as, ws.offsets, ws.bin_starts, ws.T, tile_rows, ws.scan_err);
    return hipGetLastError();
}

// Integer elements add as unsigned: the sum wraps, as numpy's does.
hipError_t launch_msel_unpack_add(void* acc, int elem, int ncomp, int64_t n,
                                  const uint16_t* flags, int nsets, const int* masks,
                                  int tile_rows, const Workspace& ws, const void* const* srcs,
                                  hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (nsets < 1 || nsets > kMaxSets || ncomp < 1) return hipErrorInvalidValue;
    SetMasks sm{};
    AddSrcs as{};
    bool any = false;
    for (int k = 0; k < nsets; ++k) {
        sm.m[k] = (uint16_t)masks[k];
        as.p[k] = srcs[k];
        any = any || srcs[k];
    }
    if (!any) return hipSuccess;
    switch (elem) {
        case MGR_ELEM_F32:
            return launch_add((float*)acc, ncomp, n, flags, nsets, sm, as, tile_rows, ws, s);
        case MGR_ELEM_F64:
            return launch_add((double*)acc, ncomp, n, flags, nsets, sm, as, tile_rows, ws, s);
        case MGR_ELEM_I32:
            return launch_add((uint32_t*)acc, ncomp, n, flags, nsets, sm, as, tile_rows, ws, s);
        case MGR_ELEM_I64:
            return launch_add((uint64_t*)acc, ncomp, n, flags, nsets, sm, as, tile_rows, ws, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace mgr
