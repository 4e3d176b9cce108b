// Multi-field (SoA) pack kernels (gfx950): several fields of the same rows
// packed from ONE ranking of the rows (mgr_pack_fields), with their launcher;
// a field they do not take goes through the single-array packs of
// mgr_pack.hip.  Helpers: mgr_device.h.
#include <vector>

#include "mgr_device.h"

namespace mgr {

// Multi-field (SoA) pack in the cooperative shape of pack_coop_kernel, for
// the common field signatures (compile time): one wave per 64-row round,
// the round ranked ONCE for every field (ballot match, per-bin bases through
// LDS behind one barrier), then every field's rows moved straight from
// registers -- unit-transposed: lane l loads the W-byte units 64 k + l of
// the field's round (each load instruction reads 64 W contiguous bytes), the
// unit's row gets its slot by shfl, same-bin rows of a round land in
// consecutive slots (contiguous runs that L2 merges with the neighbouring
// rounds').  No LDS image: a few instructions per field and round, where the
// image kernel (pack_fields_kernel) spends a permutation and a 16-byte unit
// walk per field.  CF<U>: one field, U = W * 32 + UPR (UPR = row_bytes / W
// units of W bytes), 0 = no field.
template <int U>
struct CoopField {
    static constexpr int W = U >> 5, UPR = U & 31;
    using T = typename Unit<(W ? W : 4)>::T;
    T v[UPR ? UPR : 1];
    __device__ __forceinline__ void load(const uint8_t* __restrict__ src, int64_t row0, int nr,
                                         int lane) {
        if constexpr (U != 0) {
            const T* __restrict__ sp = (const T*)src + row0 * UPR;
#pragma unroll
            for (int k = 0; k < UPR; ++k)
                if (64 * k + lane < nr * UPR) v[k] = sp[64 * k + lane];
        }
    }
    // tgt: this lane's row's tagged slot
    __device__ __forceinline__ void store(uint8_t* __restrict__ dst, uint8_t* __restrict__ red,
                                          long long tgt, int nr, int lane) const {
        if constexpr (U != 0) {
            T* __restrict__ d_u = (T*)dst;
            T* __restrict__ r_u = (T*)red;
#pragma unroll
            for (int k = 0; k < UPR; ++k) {
                const int u = 64 * k + lane;
                const int r = u / UPR, part = u - r * UPR;
                const long long t = __shfl(tgt, r, 64);
                if (u < nr * UPR && t >= 0) {
                    T* o = slot_redirected(t) ? r_u : d_u;
                    o[slot_row(t) * UPR + part] = v[k];
                }
            }
        }
    }
};

struct CoopFieldPtrs {
    const uint8_t* src[4];
    uint8_t* dst[4];
    uint8_t* red[4];
};

template <int U0, int U1, int U2, int U3>
__global__ __launch_bounds__(1024) void pack_coop_fields_kernel(
    TileCtx c, CoopFieldPtrs fp, SideIds ids) {
    __shared__ int s_cnt[kCoopMaxRounds][64];
    const int w = threadIdx.x >> 6, lane = lane_id();
    const int64_t tile = tile_index(c);
    const int64_t row0 = tile * (int64_t)c.tile_rows + 64 * w;
    const int nr = (int)max((int64_t)0, min((int64_t)64, c.n - row0));
    const uint8_t* __restrict__ dest = (const uint8_t*)c.dest;
    // the destination bytes first, waited for, then every field's loads
    // (pack_coop_kernel: 0.77 vs 0.86 ms against issuing everything at once)
    const unsigned b = lane < nr ? (unsigned)dest[row0 + lane] : 0u;
    const unsigned idv = ids.src && lane < nr ? (unsigned)ids.src[row0 + lane] : 0u;
    long long tbase = 0;
    if (lane < c.nb) tbase = seg_start(c, tile, lane);
    CoopField<U0> f0;
    CoopField<U1> f1;
    CoopField<U2> f2;
    CoopField<U3> f3;
    f0.load(fp.src[0], row0, nr, lane);
    f1.load(fp.src[1], row0, nr, lane);
    f2.load(fp.src[2], row0, nr, lane);
    f3.load(fp.src[3], row0, nr, lane);
    // rank inside the round; lane l counts bin l
    const bool valid = lane < nr;
    unsigned long long pe;
    s_cnt[w][lane] = round_rank(b, valid, lane, c.nbits, &pe);
    __syncthreads();
    if (scan_failed(c)) return;
    for (int j = 0; j < w; ++j) tbase += s_cnt[j][lane];
    const long long base = __shfl(tbase, (int)b, 64);
    long long tgt = -1;
    if (valid && (int)b != c.drop_bin) tgt = tag_slot(base + rank_in(pe), (int)b, c.redirect_bin);
    if (ids.src) store_side(ids.dst, ids.red, tgt, idv);
    f0.store(fp.dst[0], fp.red[0], tgt, nr, lane);
    f1.store(fp.dst[1], fp.red[1], tgt, nr, lane);
    f2.store(fp.dst[2], fp.red[2], tgt, nr, lane);
    f3.store(fp.dst[3], fp.red[3], tgt, nr, lane);
}

// Multi-field (SoA) pack, <= 64 bins: the fields of the same rows -- e.g.
// positions, velocities, masses and ids held as separate arrays -- moved by
// ONE launch that reads every row's destination byte once and ranks it once
// (redist.py:195-198 applied to every field with the same rank_to_send, the
// :160-164 pattern).  The cooperative shape of pack_img_kernel: one wave per
// 128 rows (two 64-row rounds), per-bin bases exchanged through LDS behind
// one barrier.  Every field's 128 rows (128 * rb bytes, 16-byte aligned) are
// copied into wave-private LDS by LDS-DMA (global_load_lds_dwordx4: no
// registers, every field's loads in flight at once), and each field in turn
// is permuted in place into its destination-ordered image (a row's slot is
// shared by all fields) and streamed out in 16-byte units (store_img_unit: a
// unit inside one bin's run is one 16-byte store to the run's 4-byte-aligned
// place, a unit straddling two runs goes dword by dword).  Field row sizes
// of 4..64 bytes (4-byte multiples) run a pass with the size at compile time
// (LDS accesses at immediate offsets, division by a constant); wider ones a
// generic pass that gathers the image's dwords through the inverse
// permutation.  The optional 2-byte side field (fine cells) is stored per
// row as in pack_img_kernel.
constexpr int kFieldsMax = 8;          // fields per launch
constexpr int kFieldsWR = 128;         // rows per wave
struct PackFieldsArgs {
    const uint8_t* src[kFieldsMax];
    uint8_t* dst[kFieldsMax];
    uint8_t* red[kFieldsMax];
    int rb[kFieldsMax];          // row bytes, 4-byte multiples
    int loff[kFieldsMax];        // byte offset of field f's rows in a wave's LDS area
    int nf;
    int wave_lds;                // LDS bytes per wave
    // field nf: its rows of a wave at LDS offset loff; returns the next offset
    int add(const void* s, void* d, void* r, int row_bytes, int off) {
        src[nf] = (const uint8_t*)s;
        dst[nf] = (uint8_t*)d;
        red[nf] = (uint8_t*)r;
        rb[nf] = row_bytes;
        loff[nf++] = off;
        return off + kFieldsWR * row_bytes;
    }
};
// a wave's LDS after the fields' rows: per-bin output address (one field at
// a time), per-bin image row offset, slot -> wave row, slot -> bin
constexpr int kFieldsTail = 64 * 8 + 64 * 8 + 2 * kFieldsWR;
// a launch's kernel arguments hold at most 4 KB
static_assert(std::is_trivially_copyable<PackFieldsArgs>::value && std::is_trivially_copyable<CoopFieldPtrs>::value,
              "kernel arguments are copied bytewise");
static_assert(sizeof(TileCtx) + sizeof(PackFieldsArgs) + 7 * 8 + 8 <= 4096 &&
              sizeof(TileCtx) + sizeof(CoopFieldPtrs) + sizeof(SideIds) <= 4096,
              "the multi-field packs' arguments exceed 4 KB");

// Any 4-byte-multiple row size (the generic pass): every 16-byte unit of the
// image gathered dword by dword from the rows in row order through the
// inverse permutation (slot -> row); rowoff[bin] = the output row of the
// bin's image slot 0.
__device__ __forceinline__ void fields_pass_any(const uint8_t* rows, int rb, const uint8_t* inv,
                                                const uint8_t* ibin, const long long* rowoff,
                                                unsigned long long dbase, unsigned long long rbase,
                                                int redirect_bin, int drop_bin, int nrows,
                                                int lane) {
    const uint32_t rinv = (uint32_t)(0x100000000ull / (unsigned)rb + 1);   // x / rb, x < 2^18
    const int nbytes = nrows * rb;
    auto addr = [&](int bb) -> unsigned long long {
        return (bb == redirect_bin ? rbase : dbase) + (unsigned long long)(rowoff[bb] * rb);
    };
    for (int x = 16 * lane; x < nbytes; x += 1024) {
        int s[4];
        u32x4_t q;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int xd = min(x + 4 * d, nbytes - 4);
            s[d] = (int)__umulhi((unsigned)xd, rinv);
            q[d] = *(const uint32_t*)(rows + (int)inv[s[d]] * rb + (xd - s[d] * rb));
        }
        const int bf = ibin[s[0]], bl = ibin[s[3]];
        if (x + 16 <= nbytes && bf == bl) {
            if (bf != drop_bin) gstore<u32x4_a4>(addr(bf) + x, q);
        } else {
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const int xd = x + 4 * d;
                const int bd = ibin[s[d]];
                if (xd < nbytes && bd != drop_bin) gstore<uint32_t>(addr(bd) + xd, q[d]);
            }
        }
    }
}

__global__ __launch_bounds__(1024) void pack_fields_kernel(
    TileCtx c, PackFieldsArgs fa, SideIds ids) {
    constexpr int WR = kFieldsWR, RPW = WR / 64;
    const int64_t n = c.n;
    const int nb = c.nb, drop_bin = c.drop_bin, redirect_bin = c.redirect_bin;
    const uint8_t* __restrict__ dest = (const uint8_t*)c.dest;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = lane_id();
    const int nw = blockDim.x >> 6;
    int* s_cnt = (int*)smem;                                    // [nw][64]
    uint8_t* wl = smem + nw * 64 * 4 + w * fa.wave_lds;         // the fields' rows
    uint8_t* tail = wl + fa.wave_lds - kFieldsTail;
    unsigned long long* gaddr = (unsigned long long*)tail;      // [64]
    long long* rowoff = (long long*)(tail + 64 * 8);            // [64]
    uint8_t* inv = tail + 64 * 16;                              // slot -> wave row
    uint8_t* ibin = inv + WR;                                   // slot -> bin
    const int64_t tile = tile_index(c);
    const int64_t row0 = tile * (int64_t)c.tile_rows + (int64_t)WR * w;
    const int nrows = __builtin_amdgcn_readfirstlane((int)max((int64_t)0, min((int64_t)WR, n - row0)));
    unsigned braw[RPW], b[RPW], idv[RPW];
    bool valid[RPW];
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        valid[q] = 64 * q + lane < nrows;
        const int64_t r = min(row0 + 64 * q + lane, n - 1);
        braw[q] = (unsigned)dest[r];
        idv[q] = ids.src ? (unsigned)ids.src[r] : 0u;
    }
    const SegLoad seg = seg_load(c, tile, lane);
    // every field's rows into LDS: unit x = 16 * (64 i + lane) of the field's
    // 128 rows lands at loff + x (LDS-DMA: wave-uniform base + lane * 16;
    // lanes past the rows are masked off, so nothing lands beyond them); the
    // last unit of the array reads up to 12 bytes past its end, inside the
    // 16-byte-aligned unit's page
#pragma unroll
    for (int f = 0; f < kFieldsMax; ++f) {
        if (f >= fa.nf) break;
        const int rb = fa.rb[f];
        const int nbytes = nrows * rb;
        const uint8_t* sp = fa.src[f] + row0 * rb;
        for (int i = 0; 1024 * i < nbytes; ++i) {
            const int x = 16 * (64 * i + lane);
            if (x < nbytes)
                __builtin_amdgcn_global_load_lds(
                    (const void*)(sp + x),
                    (__attribute__((address_space(3))) void*)(wl + fa.loff[f] + 1024 * i), 16, 0, 0);
        }
    }
#pragma unroll
    for (int q = 0; q < RPW; ++q) b[q] = valid[q] ? braw[q] : 0u;
    long long tbase = lane < nb ? seg_value(seg, lane, redirect_bin) : 0;
    // rank inside each round; lane l counts bin l per round, cnt over the wave
    unsigned long long pe[RPW];
    int cq[RPW], cnt = 0;
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        cq[q] = round_rank(b[q], valid[q], lane, c.nbits, &pe[q]);
        cnt += cq[q];
    }
    s_cnt[w * 64 + lane] = cnt;
    __syncthreads();   // (also retires the LDS-DMA loads: vmcnt(0) before the barrier)
    if (scan_failed(c)) return;
    for (int j = 0; j < w; ++j) tbase += s_cnt[j * 64 + lane];
    // wave image order: exclusive prefix of the wave's bin counts
    const int excl = wave_incl_dpp(cnt) - cnt;
    int run = excl;   // lane b: bin b's next image slot, round by round
    int slot[RPW];
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        // (shuffles in uniform control flow: a bpermute from a lane outside
        // the exec mask does not read that lane's value)
        slot[q] = __shfl(run, (int)b[q], 64) + (valid[q] ? rank_in(pe[q]) : 0);
        const long long gr = ids.src ? __shfl(tbase - excl, (int)b[q], 64) + slot[q] : 0;
        run += cq[q];
        if (valid[q]) {
            inv[slot[q]] = (uint8_t)(64 * q + lane);
            ibin[slot[q]] = (uint8_t)b[q];
            if (ids.src && (int)b[q] != drop_bin)
                ((int)b[q] == redirect_bin ? ids.red : ids.dst)[gr] = (uint16_t)idv[q];
        }
    }
    const long long ro = tbase - excl;   // lane b: output row of bin b's image slot 0
    if (lane < nb) rowoff[lane] = ro;
    // per-lane copies of the fields' run-time values (lane f: field f), read
    // with readlane: a kernel-argument array indexed at run time would be a
    // memory load (msel_pack_kernel)
    const int lrb = lane < fa.nf ? fa.rb[lane] : 0;
    const int lloff = lane < fa.nf ? fa.loff[lane] : 0;
    const unsigned long long ldst = lane < fa.nf ? (unsigned long long)fa.dst[lane] : 0ull;
    const unsigned long long lred = lane < fa.nf ? (unsigned long long)fa.red[lane] : 0ull;
#pragma unroll 1
    for (int f = 0; f < fa.nf; ++f) {
        const int rb = __builtin_amdgcn_readlane(lrb, f);
        uint8_t* rows = wl + __builtin_amdgcn_readlane(lloff, f);
        const unsigned long long dbase = readlane64(ldst, f), rbase = readlane64(lred, f);
        wave_sync();   // the previous field's stores have read gaddr
        if (lane < nb)
            gaddr[lane] = lane == drop_bin ? 0ull
                          : (lane == redirect_bin ? rbase : dbase) + (unsigned long long)(ro * rb);
        wave_sync();
        switch (rb) {
#define MGR_FP(RB_) case RB_: image_pass<RB_, kFieldsWR / 64>(rows, ibin, gaddr, slot, valid, nrows, lane); break;
            MGR_FP(4) MGR_FP(8) MGR_FP(12) MGR_FP(16) MGR_FP(20) MGR_FP(24) MGR_FP(28) MGR_FP(32)
            MGR_FP(36) MGR_FP(40) MGR_FP(44) MGR_FP(48) MGR_FP(52) MGR_FP(56) MGR_FP(60) MGR_FP(64)
#undef MGR_FP
            default:
                fields_pass_any(rows, rb, inv, ibin, rowoff, dbase, rbase, redirect_bin, drop_bin,
                                nrows, lane);
        }
    }
}

// Multi-field pack with one destination-ordered image per WORKGROUP and
// field (the tile's rows of a field, bin-major): every bin's rows of the tile
// leave as ONE contiguous run per field (tile_rows / nbins rows: 256 B of the
// 4-byte masses at 512-row tiles and 8 bins) instead of one run per wave --
// SoA fields are narrow, and per-wave runs of a few rows leave most store
// instructions writing partial lines.  Loads as pack_fields_kernel (every
// field's rows of a wave by LDS-DMA into wave-private staging, ranked once);
// then per field: the wave's rows into a tile image at their tile slots
// (row -> slot, a compile-time row size), a barrier, the tile image streamed
// out in 16-byte units by the whole workgroup (store_img_unit), a barrier.
// (A/B on the config-5 SoA rows, 512-row tiles: this 1.16-1.23 ms; two
// alternating images, one barrier per field, 1.33; every field's image at
// once with ONE barrier per tile 1.60 -- a tile's stores all at its end.)
template <int RB>
__device__ __forceinline__ void tile_field_permute(const uint8_t* rows, uint8_t* img,
                                                   const int* tslot, const bool* valid, int lane) {
    constexpr int DW = RB / 4;
    constexpr int RPW = kFieldsWR / 64;
    const uint32_t* r32 = (const uint32_t*)rows;
    uint32_t* i32 = (uint32_t*)img;
#pragma unroll
    for (int q = 0; q < RPW; ++q)
        if (valid[q]) {
            uint32_t v[DW];
#pragma unroll
            for (int p = 0; p < DW; ++p) v[p] = r32[(64 * q + lane) * DW + p];
#pragma unroll
            for (int p = 0; p < DW; ++p) i32[tslot[q] * DW + p] = v[p];
        }
}

template <int RB>
__device__ __forceinline__ void tile_field_store(const uint8_t* img, const uint8_t* ibin,
                                                 const unsigned long long* gaddr, int tile_bytes) {
    for (int x = 16 * (int)threadIdx.x; x < tile_bytes; x += 16 * (int)blockDim.x)
        store_img_unit<RB, true>(img, ibin, gaddr, x, tile_bytes);
}

__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(6))) void pack_fields_tile_kernel(
    TileCtx c, PackFieldsArgs fa, const uint8_t* __restrict__ dest,
    const int64_t* __restrict__ offsets, const int64_t* __restrict__ bin_starts,
    const uint32_t* __restrict__ scan_err, const uint16_t* __restrict__ id_src,
    uint16_t* __restrict__ id_dst, uint16_t* __restrict__ id_red, int img_bytes) {
    // (the pointers stay direct __restrict__ parameters here: read through
    // the context this kernel measured 1 % slower, profiles/tile_ctx/notes.md;
    // the context gives the rest)
    constexpr int WR = kFieldsWR, RPW = WR / 64;
    const int64_t n = c.n;
    const int nb = c.nb, drop_bin = c.drop_bin, redirect_bin = c.redirect_bin;
    const int tile_rows = c.tile_rows;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ unsigned long long s_gaddr[64];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = lane_id();
    const int nw = blockDim.x >> 6;
    uint8_t* img = smem;                                        // [img_bytes]
    uint8_t* ibin = smem + img_bytes;                           // [tile_rows]
    uint8_t* wl = ibin + align16(tile_rows) + w * fa.wave_lds;  // the wave's staged rows
    // the waves' bin counts [nw][64], after the staging (sized by the waves,
    // so six 512-row workgroups of config 5's SoA fields fit a CU's LDS)
    int (*s_cnt)[64] = (int (*)[64])(ibin + align16(tile_rows) + nw * fa.wave_lds);
    const int64_t tile = tile_index(c);
    const int64_t tile0 = tile * (int64_t)tile_rows;
    const int64_t row0 = tile0 + (int64_t)WR * w;
    const int nrows = __builtin_amdgcn_readfirstlane((int)max((int64_t)0, min((int64_t)WR, n - row0)));
    const int trows = (int)min((int64_t)tile_rows, n - tile0);
    unsigned braw[RPW], b[RPW], idv[RPW];
    bool valid[RPW];
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        valid[q] = 64 * q + lane < nrows;
        const int64_t r = min(row0 + 64 * q + lane, n - 1);
        braw[q] = (unsigned)dest[r];
        idv[q] = id_src ? (unsigned)id_src[r] : 0u;
    }
    const SegLoad seg = seg_load(offsets, bin_starts, c.T, tile, lane, nb, redirect_bin);
#pragma unroll
    for (int f = 0; f < kFieldsMax; ++f) {
        if (f >= fa.nf) break;
        const int rb = fa.rb[f];
        const int nbytes = nrows * rb;
        const uint8_t* sp = fa.src[f] + row0 * rb;
        for (int i = 0; 1024 * i < nbytes; ++i) {
            const int x = 16 * (64 * i + lane);
            if (x < nbytes)
                __builtin_amdgcn_global_load_lds(
                    (const void*)(sp + x),
                    (__attribute__((address_space(3))) void*)(wl + fa.loff[f] + 1024 * i), 16, 0, 0);
        }
    }
#pragma unroll
    for (int q = 0; q < RPW; ++q) b[q] = valid[q] ? braw[q] : 0u;
    // rank inside each round; lane l counts bin l over the wave's rounds
    unsigned long long pe[RPW];
    int cq[RPW], cnt = 0;
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        cq[q] = round_rank(b[q], valid[q], lane, c.nbits, &pe[q]);
        cnt += cq[q];
    }
    s_cnt[w][lane] = cnt;
    __syncthreads();   // (also retires the LDS-DMA loads)
    if (scan_failed(scan_err)) return;
    // lane b: the tile's count of bin b, the earlier waves' count, the bin's
    // start in the tile image (exclusive over the bins)
    int tot = 0, wpre = 0;
    for (int j = 0; j < nw; ++j) {
        const int cj = s_cnt[j][lane];
        tot += cj;
        wpre += j < w ? cj : 0;
    }
    if (lane >= nb) tot = 0;
    const int tstart = wave_incl_dpp(tot) - tot;
    const int wexcl = wave_incl_dpp(cnt) - cnt;   // the wave's own bin-major order
    const int toff = tstart + wpre - wexcl;        // lane b: wave slot -> tile slot
    int run = wexcl;
    int tslot[RPW];
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        // (shuffles in uniform control flow)
        const int ws = __shfl(run, (int)b[q], 64) + (valid[q] ? rank_in(pe[q]) : 0);
        tslot[q] = ws + __shfl(toff, (int)b[q], 64);
        run += cq[q];
        if (valid[q]) ibin[tslot[q]] = (uint8_t)b[q];
    }
    // lane b (wave 0): the bin's output row of tile image slot 0
    const long long obase = (lane < nb ? seg_value(seg, lane, redirect_bin) : 0) - tstart;
    if (id_src) {
        const long long ob = obase;
#pragma unroll
        for (int q = 0; q < RPW; ++q) {
            const long long gr = __shfl(ob, (int)b[q], 64) + tslot[q];
            if (valid[q] && (int)b[q] != drop_bin)
                ((int)b[q] == redirect_bin ? id_red : id_dst)[gr] = (uint16_t)idv[q];
        }
    }
    const int lrb = lane < fa.nf ? fa.rb[lane] : 0;
    const int lloff = lane < fa.nf ? fa.loff[lane] : 0;
    const unsigned long long ldst = lane < fa.nf ? (unsigned long long)fa.dst[lane] : 0ull;
    const unsigned long long lred = lane < fa.nf ? (unsigned long long)fa.red[lane] : 0ull;
    // per field: the wave's rows into the tile image at their slots, a
    // barrier, the image streamed out, a barrier before the next field's
#pragma unroll 1
    for (int f = 0; f < fa.nf; ++f) {
        const int rb = __builtin_amdgcn_readlane(lrb, f);
        const uint8_t* rows = wl + __builtin_amdgcn_readlane(lloff, f);
        uint8_t* fimg = img;
        unsigned long long* ga = s_gaddr;
        if (w == 0 && lane < nb) {
            const unsigned long long dbase = readlane64(ldst, f), rbase = readlane64(lred, f);
            ga[lane] = lane == drop_bin ? 0ull
                       : (lane == redirect_bin ? rbase : dbase) + (unsigned long long)(obase * rb);
        }
        switch (rb) {
#define MGR_TFP(RB_) case RB_: tile_field_permute<RB_>(rows, fimg, tslot, valid, lane); break;
            MGR_TFP(4) MGR_TFP(8) MGR_TFP(12) MGR_TFP(16) MGR_TFP(20) MGR_TFP(24) MGR_TFP(28)
            MGR_TFP(32) MGR_TFP(36) MGR_TFP(40) MGR_TFP(44) MGR_TFP(48) MGR_TFP(52) MGR_TFP(56)
            MGR_TFP(60) MGR_TFP(64)
#undef MGR_TFP
            default: break;   // (the launcher sends only 4..64-byte rows)
        }
        __syncthreads();   // the image, ibin and the field's addresses complete
        switch (rb) {
#define MGR_TFS(RB_) case RB_: tile_field_store<RB_>(fimg, ibin, ga, trows * RB_); break;
            MGR_TFS(4) MGR_TFS(8) MGR_TFS(12) MGR_TFS(16) MGR_TFS(20) MGR_TFS(24) MGR_TFS(28)
            MGR_TFS(32) MGR_TFS(36) MGR_TFS(40) MGR_TFS(44) MGR_TFS(48) MGR_TFS(52) MGR_TFS(56)
            MGR_TFS(60) MGR_TFS(64)
#undef MGR_TFS
            default: break;
        }
        __syncthreads();   // the image is reused by the next field
    }
}

template <int A, int B, int C, int D>
static hipError_t launch_coop_fields(const CoopFieldPtrs& fp, const PackJob& j) {
    prof_begin(j.s, K_PACK);
    // one wave per 64-row round
    hipLaunchKernelGGL((pack_coop_fields_kernel<A, B, C, D>), dim3((unsigned)j.c.tn),
                       dim3(j.c.tile_rows), 0, j.s, j.c, fp, j.side->ids);
    prof_end(j.s, K_PACK);
    return hipGetLastError();
}

// The cooperative multi-field kernel for a field signature it is built for
// (hipErrorNotSupported otherwise; coop_unit: each field's unit width and
// units per row).  j: the tile context and the side field of the pack.
static hipError_t pack_coop_fields(int nf, const void* const* srcs, const int64_t* row_bytes,
                                   void* const* dsts, void* const* reds, const PackJob& j) {
    int u[4] = {0, 0, 0, 0};
    CoopFieldPtrs fp{};
    for (int f = 0; f < nf; ++f) {
        u[f] = coop_unit(srcs[f], row_bytes[f], dsts[f], reds ? reds[f] : nullptr);
        if (u[f] < 0) return hipErrorNotSupported;
        fp.src[f] = (const uint8_t*)srcs[f];
        fp.dst[f] = (uint8_t*)dsts[f];
        fp.red[f] = reds ? (uint8_t*)reds[f] : nullptr;
    }
    auto sig = [&](int a, int b, int c, int d) { return u[0] == a && u[1] == b && u[2] == c && u[3] == d; };
    constexpr int F4x1 = 4 * 32 + 1, F4x3 = 4 * 32 + 3, F8x1 = 8 * 32 + 1, F8x3 = 8 * 32 + 3,
                  F16x2 = 16 * 32 + 2, F4x9 = 4 * 32 + 9, F16x1 = 16 * 32 + 1, F8x2 = 8 * 32 + 2;
    // config 5's fields as arrays: pos f32 x3, vel f32 x3, mass f32, id i64
    if (sig(F4x3, F4x3, F4x1, F8x1)) return launch_coop_fields<F4x3, F4x3, F4x1, F8x1>(fp, j);
    // f64 positions + i64 ids; 32-byte records + their f64 positions (return_positions)
    if (sig(F8x3, F8x1, 0, 0)) return launch_coop_fields<F8x3, F8x1, 0, 0>(fp, j);
    if (sig(F16x2, F8x3, 0, 0)) return launch_coop_fields<F16x2, F8x3, 0, 0>(fp, j);
    // 36-byte records + their f32 positions (config 5 with return_positions)
    if (sig(F4x9, F4x3, 0, 0)) return launch_coop_fields<F4x9, F4x3, 0, 0>(fp, j);
    // positions f32 x3 + ids i64 / f64 x2 + i64
    if (sig(F4x3, F8x1, 0, 0)) return launch_coop_fields<F4x3, F8x1, 0, 0>(fp, j);
    if (sig(F16x1, F8x1, 0, 0)) return launch_coop_fields<F16x1, F8x1, 0, 0>(fp, j);
    if (sig(F8x3, F8x3, F8x1, 0)) return launch_coop_fields<F8x3, F8x3, F8x1, 0>(fp, j);
    if (sig(F4x3, F4x3, F8x1, 0)) return launch_coop_fields<F4x3, F4x3, F8x1, 0>(fp, j);
    if (sig(F8x2, F8x1, 0, 0)) return launch_coop_fields<F8x2, F8x1, 0, 0>(fp, j);
    return hipErrorNotSupported;
}

// mgr_pack_fields: several fields of the same rows, one ranking.  With one
// field this is launch_pack (the coop / image kernels A/B'd for it).  With
// more, the fields pack_fields_kernel takes (4-byte-multiple rows, 16-byte
// aligned sources, 4-byte aligned outputs, <= 64 bins on 1-byte
// destinations, tiles of 128-row waves) move in as few launches as their LDS
// rows allow -- one for every realistic SoA set -- carrying the side field;
// any other field is packed by launch_pack on the same destinations.
hipError_t launch_pack_fields(int nf, const void* const* srcs, const int64_t* row_bytes, int64_t n,
                              const void* dest, int nbins, int drop_bin, int tile_rows,
                              const Workspace& ws, void* const* dsts, int redirect_bin,
                              void* const* reds, hipStream_t s, const uint16_t* ids_src,
                              uint16_t* ids_dst, uint16_t* ids_red) {
    if (n <= 0) return hipSuccess;
    // one tile context and side field for whichever kernels take the fields
    const TileCtx c = tile_ctx(n, dest, nbins, drop_bin, tile_rows, ws, redirect_bin);
    const SideIds ids{ids_src, ids_dst, ids_red};
    if (nf == 1)
        return launch_pack_array(srcs[0], row_bytes[0], c, dsts[0], reds ? reds[0] : nullptr, s, ids);
    const Hooks& h = hooks();
    const int nw = tile_rows / kFieldsWR;
    const bool shape = !h.pack_generic && nbins <= 64 && dest_bytes(nbins) == 1 &&
                       tile_rows % kFieldsWR == 0 && nw >= 1 && nw <= 16;
    // rows of one wave's fields, within the LDS a workgroup may take
    const int budget = (160 * 1024 - nw * 256) / max(nw, 1) - kFieldsTail;
    std::vector<int> fast, slow;
    for (int f = 0; f < nf; ++f) {
        uintptr_t a = (uintptr_t)dsts[f] | (uintptr_t)row_bytes[f];
        if (redirect_bin >= 0 && reds) a |= (uintptr_t)reds[f];
        const bool ok = shape && row_bytes[f] >= 4 && row_bytes[f] % 4 == 0 &&
                        (int64_t)kFieldsWR * row_bytes[f] <= budget &&
                        ((uintptr_t)srcs[f] & 15) == 0 && (a & 3) == 0;
        (ok ? fast : slow).push_back(f);
    }
    if (fast.size() < 2) {   // nothing to share: each field by its own kernel
        slow.insert(slow.end(), fast.begin(), fast.end());
        fast.clear();
    }
    bool side_done = ids_src == nullptr;
    int max_rb = 0;
    for (const int f : fast) max_rb = max(max_rb, (int)row_bytes[f]);
    const int want = h.fields_kernel;   // test hook: 0 = the product's choice
    if ((want == 0 || want == 2) && fast.size() == (size_t)nf && nf <= kFieldsMax &&
        max_rb <= 64 && nw <= 16) {
        // every field in the tile-image kernel when they fit one launch
        int rows = 0;
        PackFieldsArgs fa{};
        for (const int f : fast)
            rows = fa.add(srcs[f], dsts[f], reds ? reds[f] : nullptr, (int)row_bytes[f], rows);
        fa.wave_lds = rows;
        const int img = align16(tile_rows * max_rb);
        const int lds = img + align16(tile_rows) + nw * fa.wave_lds + nw * 64 * 4;
        if (lds <= 150 * 1024) {
            ensure_lds(pack_fields_tile_kernel, lds);
            prof_begin(s, K_PACK);
            hipLaunchKernelGGL(pack_fields_tile_kernel, dim3((unsigned)c.tn), dim3(64 * nw),
                               (size_t)lds, s, c, fa, (const uint8_t*)c.dest, c.offsets,
                               c.bin_starts, c.scan_err, ids.src, ids.dst, ids.red, img);
            prof_end(s, K_PACK);
            return hipGetLastError();
        }
    }
    if ((want == 0 || want == 3) && fast.size() == (size_t)nf && nf <= 4 &&
        tile_rows <= 64 * kCoopMaxRounds && tile_rows / 64 <= 16) {
        // every field in the cooperative multi-field kernel when the fields'
        // signature is one it is built for
        SideField side{ids, false};
        const PackJob j{nullptr, 0, nullptr, nullptr, s, &side, h, c};
        const hipError_t e = pack_coop_fields(nf, srcs, row_bytes, dsts, reds, j);
        if (e != hipErrorNotSupported) return e;
    }
    size_t i = 0;
    while (i < fast.size()) {
        PackFieldsArgs fa{};
        int rows = 0;
        for (; i < fast.size() && fa.nf < kFieldsMax; ++i) {
            const int f = fast[i];
            const int rb = (int)row_bytes[f];
            if (rows + kFieldsWR * rb > budget) break;
            rows = fa.add(srcs[f], dsts[f], reds ? reds[f] : nullptr, rb, rows);   // + n * 512 bytes
        }
        fa.wave_lds = rows + kFieldsTail;
        const int lds = nw * 64 * 4 + nw * fa.wave_lds;
        ensure_lds(pack_fields_kernel, lds);
        prof_begin(s, K_PACK);
        hipLaunchKernelGGL(pack_fields_kernel, dim3((unsigned)c.tn), dim3(64 * nw), (size_t)lds, s,
                           c, fa, side_done ? SideIds{} : ids);
        prof_end(s, K_PACK);
        side_done = true;
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    for (const int f : slow) {
        const hipError_t e = launch_pack_array(srcs[f], row_bytes[f], c, dsts[f],
                                               reds ? reds[f] : nullptr, s,
                                               side_done ? SideIds{} : ids);
        side_done = true;
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace mgr
