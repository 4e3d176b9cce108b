// One-pass source partition of a SoA payload (gfx950): the multi-field form of
// mgr_onepass.hip.  The payload's fields are separate arrays sharing their
// rows (config 5 as positions, velocities, masses, ids); every field is read
// ONCE, staged in LDS, the rows binned from the staged copy of the position
// field, ranked by ballots, placed by one decoupled look-back per bin and tile
// (the shared tile stages, mgr_onepass_device.h) and every field
// scattered from its staged copy into the reference's send_buff list
// (redist.py:195-198): bin b's rows of field f, in source order, from
// outs[f] + b * cap * rb[f], their fine ids from fine_out + b * cap.  The
// look-back is per bin and tile, whatever the number of fields.  Config 5's
// four arrays move 36 + 36 + 2 = 74 B/row, as its records do, plus the
// position write-back: the 12-byte position rows of every wave in which a
// row wrapped (all of them with write-back "all": 86 B/row); the classic SoA
// source side (bin + scan + pack) re-reads the positions and moves a
// destination byte and a fine id per row through HBM twice.
//
// The position field may have no output (outs[pos_field] == NULL): positions
// that are not part of the payload are staged, wrapped and written back, not
// scattered.
//
// The tile stages and the LDS layout are the record kernel's
// (mgr_onepass_device.h); failure reporting is the completion WITH the done
// counter (onepass_complete<true>).  What is this kernel's own: the field
// table, a position field that may have no output, and the loop over the
// fields with the bins' addresses refilled per field (4, 8, 12, 16-byte rows
// at compile time, else the gathered store).
#include "mgr_onepass_device.h"

namespace mgr {

constexpr int kOneFMaxFields = 8;
constexpr int kOneFMaxRowBytes = 64;    // one field's rows
constexpr int kOneFMaxSumBytes = 128;   // all staged fields' rows: the record kernel's LDS envelope

// The staged fields, by value (kernarg segment).
struct OneFields {
    uint8_t* src[kOneFMaxFields];
    uint8_t* out[kOneFMaxFields];   // NULL: staged (the position field), not scattered
    int rb[kOneFMaxFields];
    int off[kOneFMaxFields];        // the field's block inside a wave's staged rows
    int nf, pf, pos_off;
    int rows_bytes;                 // kOneWR * sum(rb): a wave's staged rows
};

template <typename PosT, bool kP, int SIDE, int GEO, int NW>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(8))) void onepass_fields_kernel(
    OneFields fl, int64_t n, Geom g, FineGeom fg, uint16_t* __restrict__ fine_out, int64_t cap,
    int64_t* __restrict__ bin_counts, uint64_t* __restrict__ words, int64_t T, int spins,
    int write_all, int poison_tile) {
    constexpr int RPW = kOneWR / 64;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ int s_tile, s_poison;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = lane_id();
    const int nb = g.nbins;
    OnePassCtl* ctl = (OnePassCtl*)(words + T * nb);
    const int64_t tile = onepass_take_ticket(ctl, &s_tile, &s_poison);
    // the wave's staged rows: one block of kOneWR rows per field, each a
    // multiple of 512 bytes; config 5's four arrays (36 B/row together) take
    // what its records take
    const OneLds L = onepass_carve<NW>(smem, w, fl.rows_bytes, nb);
    int64_t row0;
    const int nrows = onepass_wave_rows<NW>(tile, w, n, &row0);
    // all fields in flight before the wait
#pragma nounroll
    for (int f = 0; f < fl.nf; ++f)
        onepass_stage(fl.src[f] + row0 * fl.rb[f], L.wl + fl.off[f], nrows * fl.rb[f], lane);
    onepass_staged();
    const int prb = fl.rb[fl.pf];
    uint8_t* pl = L.wl + fl.off[fl.pf];   // the staged position field
    unsigned b[RPW], side[RPW];
    bool valid[RPW];
    const bool dirty = onepass_bin<RPW, PosT, kP, SIDE, GEO>(pl, prb, fl.pos_off, nrows, lane, g, fg,
                                                             b, side, valid);
    onepass_write_back<kP>(fl.src[fl.pf] + row0 * prb, pl, nrows * prb, dirty, write_all, lane);
    unsigned long long pe[RPW];
    int cq[RPW], slot[RPW];
    const int cnt = onepass_rank<RPW>(L, w, nb, g.nbits, lane, b, valid, pe, cq);
    if (!onepass_scan<NW, true>(L, words, ctl, tile, T, w, nb, lane, spins, poison_tile, &s_poison,
                                 bin_counts) ||
        nrows == 0)
        return;
    const OnePlace at =
        onepass_place<RPW, SIDE>(L, w, nb, lane, cnt, b, valid, pe, cq, side, cap, fine_out, slot);
    // every field's destination-ordered image streamed out in 16-byte units
#pragma nounroll
    for (int f = 0; f < fl.nf; ++f) {
        uint8_t* out = fl.out[f];
        if (!out) continue;   // the position field outside the payload
        const int rb = fl.rb[f];
        uint8_t* rows = L.wl + fl.off[f];
        wave_sync();   // the previous field's units read their addresses
        if (lane < nb) L.gaddr[lane] = at.fits ? (unsigned long long)(out + at.ro * rb) : 0ull;
        wave_sync();
        switch (rb) {
            case 4: image_pass<4, RPW>(rows, L.ibin, L.gaddr, slot, valid, nrows, lane); break;
            case 8: image_pass<8, RPW>(rows, L.ibin, L.gaddr, slot, valid, nrows, lane); break;
            case 12: image_pass<12, RPW>(rows, L.ibin, L.gaddr, slot, valid, nrows, lane); break;
            case 16: image_pass<16, RPW>(rows, L.ibin, L.gaddr, slot, valid, nrows, lane); break;
            default: gather_pass(rows, rb, L.inv, L.ibin, L.gaddr, nrows * rb, lane);
        }
    }
}

struct OneFieldsKernels {
    template <typename PosT, bool kP, int SIDE, int GEO>
    static auto kernel() {
        return onepass_fields_kernel<PosT, kP, SIDE, GEO, kOneNW>;
    }
};

// The shapes the kernel takes (the caller runs the two-pass path otherwise):
// NULL when it takes them, else the argument that rules the shape out.
const char* onepass_fields_refusal(const Geom& g, int nf, void* const* srcs,
                                   const int64_t* row_bytes, int pos_field, int64_t pos_off,
                                   int pos_dtype, int64_t n, void* const* outs,
                                   const uint16_t* fine_out) {
    const int psz = pos_dtype == MGR_F32 ? 4 : pos_dtype == MGR_F64 ? 8 : 0;
    if (!psz) return "pos_dtype: float32 / float64 positions only";
    if (g.dim != 3) return "plan: 3-D grids only";
    if (g.nbins > 64) return "plan: at most 64 bins";
    if (nf > kOneFMaxFields) return "nfields: at most 8 staged fields";
    int64_t sum = 0;
    for (int f = 0; f < nf; ++f) {
        if (row_bytes[f] % 4 || row_bytes[f] < 4 || row_bytes[f] > kOneFMaxRowBytes)
            return "row_bytes: every field's rows a multiple of 4 in 4..64 bytes";
        sum += row_bytes[f];
    }
    if (sum > kOneFMaxSumBytes) return "row_bytes: at most 128 staged bytes per row";
    if (pos_off < 0 || pos_off % psz || pos_off + 3 * psz > row_bytes[pos_field])
        return "pos_offset: three aligned coordinates inside the position field's rows";
    if (n > 0) {
        for (int f = 0; f < nf; ++f) {
            if ((uintptr_t)srcs[f] & 15) return "srcs: 16-byte aligned sources";
            if (outs && ((uintptr_t)outs[f] & 3)) return "outs: 4-byte aligned outputs";
        }
        if ((uintptr_t)fine_out & 1) return "fine_out: 2-byte aligned";
    }
    return nullptr;
}

hipError_t launch_onepass_fields(const Geom& g, const FineGeom* fg, int nf, void* const* srcs,
                                 const int64_t* row_bytes, int pos_field, int64_t pos_off,
                                 int pos_dtype, int64_t n, int periodic, void* const* outs,
                                 uint16_t* fine_out, int64_t cap, int64_t* bin_counts,
                                 void* workspace, hipStream_t s) {
    if (nf < 1 || pos_field < 0 || pos_field >= nf || cap < 0 ||
        onepass_fields_refusal(g, nf, srcs, row_bytes, pos_field, pos_off, pos_dtype, n, outs,
                               fine_out))
        return hipErrorNotSupported;
    if (n <= 0) return hipMemsetAsync(bin_counts, 0, (size_t)g.nbins * 8, s);
    OneFields fl{};
    int sum = 0;
    for (int f = 0; f < nf; ++f) {
        fl.src[f] = (uint8_t*)srcs[f];
        fl.out[f] = (uint8_t*)outs[f];
        fl.rb[f] = (int)row_bytes[f];
        fl.off[f] = kOneWR * sum;
        sum += (int)row_bytes[f];
    }
    fl.nf = nf;
    fl.pf = pos_field;
    fl.pos_off = (int)pos_off;
    fl.rows_bytes = kOneWR * sum;
    const OneLaunch L{g, fg, pos_dtype, periodic, sum, n, fine_out, cap, bin_counts,
                      (uint64_t*)workspace, K_ONEPASS_FIELDS, s};
    return onepass_dispatch<OneFieldsKernels>(L, fl);
}

}  // namespace mgr
