// One-pass source partition of a SoA payload (gfx950): the multi-field form of
// mgr_onepass.hip.  The payload's fields are separate arrays sharing their
// rows (config 5 as positions, velocities, masses, ids); every field is read
// ONCE, staged in LDS, the rows binned from the staged copy of the position
// field, ranked by ballots, placed by one decoupled look-back per bin and tile
// (the record kernel's words and helpers, mgr_device.h) and every field
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
// Failure reporting: every tile counts itself done ONCE, after it published
// its inclusive words, in one 64-bit word (finished tiles in bits 0-31, tiles
// whose look-back gave up in bits 32-63: one location, so the failures arrive
// with the count).  The tile that counts last is the only writer of
// bin_counts: every bin's total from the last tile's inclusive words, or -1
// for every bin when any tile gave up -- also a middle tile that later tiles
// looked past (they use its aggregate, which is valid, and place their rows
// behind rows that were never written).
#include "mgr_device.h"

namespace mgr {

constexpr int kOneFWR = 128;   // rows per wave (two 64-row rounds)
constexpr int kOneFNW = 8;     // waves per workgroup: 1024-row tiles, as the record kernel
constexpr int kOneFTile = kOneFWR * kOneFNW;
constexpr int kOneFMaxFields = 8;
constexpr int kOneFMaxRowBytes = 64;    // one field's rows
constexpr int kOneFMaxSumBytes = 128;   // all staged fields' rows: the record kernel's LDS envelope

// Behind the [T][nbins] look-back words (mgr_onepass_workspace_bytes: the
// record kernel's two control words and its 8 spare bytes).
struct OneFieldsCtl {
    uint32_t ticket;   // tiles in dispatch order
    uint32_t err;      // a look-back gave up
    uint64_t done;     // tiles that published their words (bits 0-31), failed ones (32-63)
};

// The staged fields, by value (kernarg segment).
struct OneFields {
    uint8_t* src[kOneFMaxFields];
    uint8_t* out[kOneFMaxFields];   // NULL: staged (the position field), not scattered
    int rb[kOneFMaxFields];
    int off[kOneFMaxFields];        // the field's block inside a wave's staged rows
    int nf, pf, pos_off;
    int rows_bytes;                 // kOneFWR * sum(rb): a wave's staged rows
};

static int onepass_fields_lds_bytes(int nw, int sum_rb, int nb) {
    const int nbe = (nb + 1) & ~1;
    return nw * (kOneFWR * sum_rb + 8 * nbe + 2 * kOneFWR) + 16 * nbe + 4 * nw * nb;
}

// One field's rows of a wave, gathered through the inverse permutation: any
// 4-byte-multiple row (the record kernel's generic path).
__device__ __forceinline__ void gather_pass(const uint8_t* rows, int rb, const uint8_t* inv,
                                            const uint8_t* ibin, const unsigned long long* gaddr,
                                            int nbytes, int lane) {
    const uint32_t rinv = (uint32_t)(0x100000000ull / (unsigned)rb + 1);
    for (int x = 16 * lane; x < nbytes; x += 1024) {
        int s[4];
        u32x4_t v;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int xd = min(x + 4 * d, nbytes - 4);
            s[d] = (int)__umulhi((unsigned)xd, rinv);
            v[d] = *(const uint32_t*)(rows + (int)inv[s[d]] * rb + (xd - s[d] * rb));
        }
        const int bf = ibin[s[0]], bl = ibin[s[3]];
        const unsigned long long af = gaddr[bf];
        if (x + 16 <= nbytes && bf == bl) {
            if (af) gstore<u32x4_a4>(af + x, v);
        } else {
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const int xd = x + 4 * d;
                const unsigned long long ad = gaddr[ibin[s[d]]];
                if (xd < nbytes && ad) gstore<uint32_t>(ad + xd, v[d]);
            }
        }
    }
}

template <typename PosT, bool kP, int SIDE, int GEO, int NW>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(8))) void onepass_fields_kernel(
    OneFields fl, int64_t n, Geom g, FineGeom fg, uint16_t* __restrict__ fine_out, int64_t cap,
    int64_t* __restrict__ bin_counts, uint64_t* __restrict__ words, int64_t T, int spins,
    int write_all, int poison_tile) {
    constexpr int WR = kOneFWR, RPW = WR / 64;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ int s_tile, s_poison;
    OneFieldsCtl* ctl = (OneFieldsCtl*)(words + T * g.nbins);
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = lane_id();
    const int nb = g.nbins;
    if (threadIdx.x == 0) {
        s_tile = (int)__hip_atomic_fetch_add(&ctl->ticket, 1u, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
        s_poison = 0;
    }
    __syncthreads();
    const int64_t tile = s_tile;
    // LDS (onepass_fields_lds_bytes), as the record kernel's: per wave its rows
    // -- one block of WR rows per field, each a multiple of 512 bytes -- the
    // bins' output addresses of the field being scattered, the inverse
    // permutation and the slots' bins; then the waves' bin counts and the
    // tile's bases and counts.  Sized by the bins and the fields' bytes:
    // config 5's four arrays (36 B/row together) take what its records take.
    const int nbe = (nb + 1) & ~1;
    const int wave_lds = fl.rows_bytes + 8 * nbe + 2 * WR;
    uint8_t* wl = smem + w * wave_lds;
    unsigned long long* gaddr = (unsigned long long*)(wl + fl.rows_bytes);
    uint8_t* inv = (uint8_t*)(gaddr + nbe);
    uint8_t* ibin = inv + WR;
    long long* s_base = (long long*)(smem + NW * wave_lds);
    long long* s_agg = s_base + nbe;
    int* s_cnt = (int*)(s_agg + nbe);   // [NW][nb]
    const int64_t row0 = tile * (int64_t)(WR * NW) + (int64_t)WR * w;
    const int nrows = __builtin_amdgcn_readfirstlane(
        (int)max((int64_t)0, min((int64_t)WR, n - row0)));
    // the wave's rows of every field into LDS (LDS-DMA: wave-uniform base +
    // lane * 16; lanes past the rows masked off; a field's last unit reads up
    // to 12 bytes past the array's end, inside its 16-byte-aligned unit, and
    // lands inside the field's own block), all fields in flight before the wait
#pragma nounroll
    for (int f = 0; f < fl.nf; ++f) {
        const int nbytes = nrows * fl.rb[f];
        const uint8_t* gp = fl.src[f] + row0 * fl.rb[f];
        uint8_t* lp = wl + fl.off[f];
        for (int i = 0; 1024 * i < nbytes; ++i) {
            const int x = 16 * (64 * i + lane);
            if (x < nbytes)
                __builtin_amdgcn_global_load_lds(
                    (const void*)(gp + x), (__attribute__((address_space(3))) void*)(lp + 1024 * i),
                    16, 0, 0);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    wave_sync();
    // bin every row from the staged position field (the wrap is written into
    // the copy, S1)
    const int prb = fl.rb[fl.pf];
    uint8_t* pl = wl + fl.off[fl.pf];
    unsigned b[RPW], side[RPW];
    bool valid[RPW];
    bool dirty = false;
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        const int r = 64 * q + lane;
        valid[q] = r < nrows;
        b[q] = 0;
        side[q] = 0;
        if (valid[q]) {
            long long sc = 0;
            b[q] = (unsigned)bin_row<PosT, kP, 3, SIDE, GEO>((PosT*)(pl + r * prb + fl.pos_off), g,
                                                             nullptr, &dirty, &fg, nullptr, &sc);
            side[q] = (unsigned)sc;
        }
    }
    wave_sync();
    // the caller's position array holds the wrapped values (redist.py:68 in
    // place): the wave's block of that one field goes back when a row changed
    // (or always, write_all)
    if (kP && (write_all || __ballot(dirty) != 0ull)) {
        uint8_t* gp = fl.src[fl.pf] + row0 * prb;
        const int nbytes = nrows * prb, full = nbytes & ~15;
        for (int x = 16 * lane; x < full; x += 1024)
            *(u32x4_t*)(gp + x) = *(const u32x4_t*)(pl + x);
        for (int x = full + 4 * lane; x < nbytes; x += 256)
            *(uint32_t*)(gp + x) = *(const uint32_t*)(pl + x);
    }
    // rank inside each round; lane l counts bin l over the wave's rounds
    unsigned long long pe[RPW];
    int cq[RPW], cnt = 0;
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        cq[q] = round_rank(b[q], valid[q], lane, g.nbits, &pe[q]);
        cnt += cq[q];
    }
    if (lane < nb) s_cnt[w * nb + lane] = cnt;
    __syncthreads();
    // the tile's count of every bin, published at once (wave 0, lane b) so
    // later tiles can look past this one before its prefix is known
    if (w == 0 && lane < nb) {
        long long agg = 0;
#pragma unroll
        for (int j = 0; j < NW; ++j) agg += s_cnt[j * nb + lane];
        s_agg[lane] = agg;
        flag_store(words + tile * nb + lane, (tile == 0 ? kScanInc : kScanAgg) | (uint64_t)agg);
    }
    __syncthreads();
    // the earlier tiles' counts of every bin, by wave 0 (the record kernel's
    // look-back: lane k * nbp + b reads bin b's word of tile base - k)
    if (w == 0) {
        const int nbp = nb <= 1 ? 1 : 1 << (32 - __clz(nb - 1));
        const int win = 64 / nbp;
        const int bb = lane & (nbp - 1), k = lane / nbp;
        unsigned long long grp = 0;   // the lanes of one bin: bits bb, bb + nbp, ...
        for (int j = 0; j < win; ++j) grp |= 1ull << (j * nbp);
        grp <<= bb;
        // test hook (onepass_poison_tile): this tile treats its look-back as
        // given up -- the bounded-poll error path, taken deterministically
        const bool hooked = tile == (int64_t)poison_tile;
        bool done = bb >= nb || tile == 0 || hooked;
        long long excl = 0;
        uint64_t poison = hooked ? kScanPoison : 0;
        for (int64_t base = tile - 1;; base -= win) {
            const int64_t idx = base - k;
            uint64_t v = kScanInc;
            if (!done && idx >= 0) v = flag_poll(words + idx * nb + bb, 1, poison ? 0 : spins);
            const unsigned long long im = __ballot(!done && (v >> 62) >= 2) & grp;
            const int first = im ? __ffsll((long long)im) - 1 : 64;   // nearest inclusive of my bin
            const bool used = !done && lane <= first;
            long long x = used ? (long long)(v & kScanVal) : 0;
            if (__ballot(used && (v & kScanPoison)) & grp) poison = kScanPoison;
            for (int o = nbp; o < 64; o <<= 1) x += __shfl_xor(x, o, 64);
            excl += x;
            if (im) done = true;
            if (__ballot(!done) == 0ull) break;
        }
        const bool mine = k == 0 && bb < nb;
        const bool failed_here = __ballot(mine && poison) != 0ull;
        if (mine) {
            if (tile > 0 || poison)
                flag_store(words + tile * nb + bb, kScanInc | poison | (uint64_t)(excl + s_agg[bb]));
            s_base[bb] = excl;
            if (poison) {
                s_poison = 1;
                __hip_atomic_store(&ctl->err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        // this tile is done with the words: counted once, with its failure
        // (relaxed atomics on ONE location are seen in order, so the failures
        // of every tile counted before arrive with the count)
        unsigned long long seen = 0;
        if (lane == 0)
            seen = __hip_atomic_fetch_add(&ctl->done, 1ull + (failed_here ? (1ull << 32) : 0ull),
                                          __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        seen = readlane64(seen, 0);
        if ((int64_t)(seen & 0xFFFFFFFFull) == T - 1) {
            // the last tile to be counted: the only writer of bin_counts.  The
            // last tile's inclusive words were stored before it counted itself,
            // but relaxed atomics on two locations are not ordered for another
            // reader, so they are polled (bounded; one look in practice)
            bool bad = failed_here || (seen >> 32) != 0 ||
                       __hip_atomic_load(&ctl->err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
            long long total = 0;
            if (mine) {
                if (tile == T - 1) {
                    total = excl + s_agg[bb];
                } else {
                    const uint64_t v = flag_poll(words + (T - 1) * nb + bb, 2, spins < 0 ? 0 : spins);
                    total = (long long)(v & kScanVal);
                    bad = bad || (v & kScanPoison) != 0;
                }
            }
            bad = __ballot(bad) != 0ull;
            if (mine) bin_counts[bb] = bad ? -1 : total;
        }
    }
    __syncthreads();
    if (s_poison || nrows == 0) return;
    // this wave's rows of bin b start at the tile's base + the earlier waves' counts
    long long tbase = 0;
    if (lane < nb) {
        tbase = s_base[lane];
        for (int j = 0; j < w; ++j) tbase += s_cnt[j * nb + lane];
    }
    const int excl = wave_incl_dpp(cnt) - cnt;   // the bins' image starts (bin-major)
    int run = excl;
    int slot[RPW];
    // lane b: a bin whose rows of this wave would reach cap writes none of
    // them, for any field nor their fine ids (the caller sees count > cap and
    // redoes the partition)
    const bool fits = tbase + cnt <= cap;
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        // (shuffles in uniform control flow)
        slot[q] = __shfl(run, (int)b[q], 64) + (valid[q] ? rank_in(pe[q]) : 0);
        const long long orow = __shfl(tbase - excl, (int)b[q], 64) + slot[q];   // row in the region
        const int fitb = __shfl((int)fits, (int)b[q], 64);
        run += cq[q];
        if (valid[q]) {
            inv[slot[q]] = (uint8_t)(64 * q + lane);
            ibin[slot[q]] = (uint8_t)b[q];
            if (SIDE == kSideFine && fitb)
                fine_out[(int64_t)b[q] * cap + orow] = (uint16_t)side[q];
        }
    }
    // lane b: region row of bin b's image slot 0
    const long long ro = (int64_t)lane * cap + tbase - excl;
    // every field's destination-ordered image streamed out in 16-byte units
#pragma nounroll
    for (int f = 0; f < fl.nf; ++f) {
        uint8_t* out = fl.out[f];
        if (!out) continue;   // the position field outside the payload
        const int rb = fl.rb[f];
        uint8_t* rows = wl + fl.off[f];
        wave_sync();   // the previous field's units read their addresses
        if (lane < nb) gaddr[lane] = fits ? (unsigned long long)(out + ro * rb) : 0ull;
        wave_sync();
        switch (rb) {
            case 4: image_pass<4, RPW>(rows, ibin, gaddr, slot, valid, nrows, lane); break;
            case 8: image_pass<8, RPW>(rows, ibin, gaddr, slot, valid, nrows, lane); break;
            case 12: image_pass<12, RPW>(rows, ibin, gaddr, slot, valid, nrows, lane); break;
            case 16: image_pass<16, RPW>(rows, ibin, gaddr, slot, valid, nrows, lane); break;
            default: gather_pass(rows, rb, inv, ibin, gaddr, nrows * rb, lane);
        }
    }
}

template <typename PosT, bool kP, int SIDE>
static hipError_t onepass_fields_t(const Geom& g, const FineGeom& fg, const OneFields& fl,
                                   int sum_rb, int64_t n, uint16_t* fine_out, int64_t cap,
                                   int64_t* bin_counts, uint64_t* words, hipStream_t s) {
    const Hooks& h = hooks();   // one snapshot for the launch
    constexpr int NW = kOneFNW;
    auto k = onepass_fields_kernel<PosT, kP, SIDE, kGeoAny, NW>;
    if constexpr (kP) {
        const int geo = h.bin_generic ? kGeoAny : geo_kind(g, sizeof(PosT) == 4);
        if (geo == kGeoF32) k = onepass_fields_kernel<PosT, kP, SIDE, kGeoF32, NW>;
        else if (geo == kGeoF64) k = onepass_fields_kernel<PosT, kP, SIDE, kGeoF64, NW>;
    }
    const int64_t T = (n + kOneFTile - 1) / kOneFTile;
    const int lds = onepass_fields_lds_bytes(NW, sum_rb, g.nbins);
    ensure_lds(k, lds);
    hipLaunchKernelGGL(k, dim3((unsigned)T), dim3(64 * NW), (size_t)lds, s, fl, n, g, fg, fine_out,
                       cap, bin_counts, words, T, h.scan_spins, g.write_back_all,
                       h.onepass_poison_tile);
    return hipGetLastError();
}

template <typename PosT>
static hipError_t onepass_fields_d(const Geom& g, const FineGeom* fg, const OneFields& fl,
                                   int sum_rb, int64_t n, int periodic, uint16_t* fine_out,
                                   int64_t cap, int64_t* bin_counts, uint64_t* words,
                                   hipStream_t s) {
    FineGeom f{};
    if (fg) f = *fg;
    if (periodic)
        return fg ? onepass_fields_t<PosT, true, kSideFine>(g, f, fl, sum_rb, n, fine_out, cap, bin_counts, words, s)
                  : onepass_fields_t<PosT, true, kSideNone>(g, f, fl, sum_rb, n, fine_out, cap, bin_counts, words, s);
    return fg ? onepass_fields_t<PosT, false, kSideFine>(g, f, fl, sum_rb, n, fine_out, cap, bin_counts, words, s)
              : onepass_fields_t<PosT, false, kSideNone>(g, f, fl, sum_rb, n, fine_out, cap, bin_counts, words, s);
}

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
        fl.off[f] = kOneFWR * sum;
        sum += (int)row_bytes[f];
    }
    fl.nf = nf;
    fl.pf = pos_field;
    fl.pos_off = (int)pos_off;
    fl.rows_bytes = kOneFWR * sum;
    uint64_t* words = (uint64_t*)workspace;
    hipError_t e = hipMemsetAsync(words, 0, (size_t)onepass_workspace_bytes(n, g.nbins), s);
    if (e != hipSuccess) return e;
    prof_begin(s, K_ONEPASS_FIELDS);
    e = pos_dtype == MGR_F32
            ? onepass_fields_d<float>(g, fg, fl, sum, n, periodic, fine_out, cap, bin_counts, words, s)
            : onepass_fields_d<double>(g, fg, fl, sum, n, periodic, fine_out, cap, bin_counts, words, s);
    prof_end(s, K_ONEPASS_FIELDS);
    return e;
}

}  // namespace mgr
