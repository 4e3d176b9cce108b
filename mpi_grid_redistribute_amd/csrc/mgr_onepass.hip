// One-pass source partition (gfx950): bin + rank + scatter of records whose
// positions sit inside the rows (config 5's 36-byte records with their f32
// position view, S9), reading every record ONCE.  The classic path reads the
// record lines twice -- the bin pass fetches the whole lines its positions
// sit in, the pack reads them again (116 B/row for 36-byte rows with fine
// ids) -- this kernel moves 36 + 36 + 2 = 74 B/row.
//
// Output: the reference's send_buff list itself (redist.py:195-198,
// send_buff[i] = data[rank_to_send == i], original order kept): bin b's rows
// go to their own region out + b * cap * row_bytes (and their fine ids to
// fine_out + b * cap), in order.  No global bin starts are needed before a
// row is placed: a tile's place inside every bin's region is the sum of the
// earlier tiles' counts of that bin, found by a decoupled look-back per bin
// over the tiles (the tile stages, mgr_onepass_device.h, shared with the SoA
// kernel).  bin_counts[b] = bin b's rows; rows at or past cap are not written
// -- the caller compares the counts with cap (overflow: redo with the classic
// path, whose bin pass re-reads the stored, already wrapped positions with
// periodic = 0 and bins them identically, S2).  A look-back that gives up
// (bounded polls) poisons its prefix: every later tile that meets it writes
// nothing and the counts, written by the last tile, read -1 (the completion
// without the done counter, onepass_complete<false>).
//
// What is this kernel's own: one source, one output, the bins' addresses
// filled once and the row size switched at compile time (32, 36, else the
// gathered store).
#include "mgr_onepass_device.h"

namespace mgr {

// [T][nbins] look-back words, then the control words; zeroed before a launch.
static_assert(sizeof(OnePassCtl) == 16, "the workspace's control words");
int64_t onepass_workspace_bytes(int64_t n, int nbins) {
    return (onepass_tiles(n) * (int64_t)nbins) * 8 + (int64_t)sizeof(OnePassCtl);
}

template <typename PosT, bool kP, int SIDE, int GEO, int NW>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(8))) void onepass_partition_kernel(
    uint8_t* __restrict__ data, int rb, int pos_off, uint8_t* __restrict__ out, int64_t n, Geom g,
    FineGeom fg, uint16_t* __restrict__ fine_out, int64_t cap, int64_t* __restrict__ bin_counts,
    uint64_t* __restrict__ words, int64_t T, int spins, int write_all, int poison_tile) {
    constexpr int RPW = kOneWR / 64;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ int s_tile, s_poison;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = lane_id();
    const int nb = g.nbins;
    OnePassCtl* ctl = (OnePassCtl*)(words + T * nb);
    const int64_t tile = onepass_take_ticket(ctl, &s_tile, &s_poison);
    const OneLds L = onepass_carve<NW>(smem, w, kOneWR * rb, nb);
    int64_t row0;
    const int nrows = onepass_wave_rows<NW>(tile, w, n, &row0);
    const int nbytes = nrows * rb;
    uint8_t* gp = data + row0 * rb;
    onepass_stage(gp, L.wl, nbytes, lane);
    onepass_staged();
    unsigned b[RPW], side[RPW];
    bool valid[RPW];
    const bool dirty =
        onepass_bin<RPW, PosT, kP, SIDE, GEO>(L.wl, rb, pos_off, nrows, lane, g, fg, b, side, valid);
    onepass_write_back<kP>(gp, L.wl, nbytes, dirty, write_all, lane);
    unsigned long long pe[RPW];
    int cq[RPW], slot[RPW];
    const int cnt = onepass_rank<RPW>(L, w, nb, g.nbits, lane, b, valid, pe, cq);
    if (!onepass_scan<NW, false>(L, words, ctl, tile, T, w, nb, lane, spins, poison_tile, &s_poison,
                                 bin_counts) ||
        nrows == 0)
        return;
    const OnePlace pl =
        onepass_place<RPW, SIDE>(L, w, nb, lane, cnt, b, valid, pe, cq, side, cap, fine_out, slot);
    if (lane < nb) L.gaddr[lane] = pl.fits ? (unsigned long long)(out + pl.ro * rb) : 0ull;
    wave_sync();
    // the destination-ordered image streamed out in 16-byte units
    switch (rb) {
        case 32: image_pass<32, RPW>(L.wl, L.ibin, L.gaddr, slot, valid, nrows, lane); break;
        case 36: image_pass<36, RPW>(L.wl, L.ibin, L.gaddr, slot, valid, nrows, lane); break;
        default: gather_pass(L.wl, rb, L.inv, L.ibin, L.gaddr, nbytes, lane);
    }
}

struct OneRecordKernels {
    template <typename PosT, bool kP, int SIDE, int GEO>
    static auto kernel() {
        return onepass_partition_kernel<PosT, kP, SIDE, GEO, kOneNW>;
    }
};

hipError_t launch_onepass(const Geom& g, const FineGeom* fg, void* data, int64_t row_bytes,
                          int64_t pos_off, int pos_dtype, int64_t n, int periodic, void* out,
                          uint16_t* fine_out, int64_t cap, int64_t* bin_counts, void* workspace,
                          hipStream_t s) {
    const int psz = pos_dtype == MGR_F32 ? 4 : pos_dtype == MGR_F64 ? 8 : 0;
    // shapes this kernel takes; the caller runs the classic path otherwise
    if (!psz || g.dim != 3 || g.nbins > 64 || row_bytes % 4 || row_bytes < 4 ||
        row_bytes > 128 || pos_off < 0 || pos_off % psz || pos_off + 3 * psz > row_bytes ||
        ((uintptr_t)data & 15) || ((uintptr_t)out & 3) || ((uintptr_t)fine_out & 1) || cap < 0)
        return hipErrorNotSupported;
    if (n <= 0) return hipMemsetAsync(bin_counts, 0, (size_t)g.nbins * 8, s);
    const OneLaunch L{g, fg, pos_dtype, periodic, (int)row_bytes, n, fine_out, cap, bin_counts,
                      (uint64_t*)workspace, K_ONEPASS, s};
    return onepass_dispatch<OneRecordKernels>(L, (uint8_t*)data, (int)row_bytes, (int)pos_off,
                                              (uint8_t*)out);
}

}  // namespace mgr
