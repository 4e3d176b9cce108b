// Pack kernels of the hot path (gfx950): the stable partition of every
// payload field into the bin-major send buffer / output (redist.py:195-198,
// send_buff[i] = data[rank_to_send == i], order kept), with their launchers
// and tile-size policy: the single-array kernels and the ranked pack (the
// multi-field packs: mgr_pack_fields.hip; the multi-selection packs:
// mgr_msel_pack.hip).  Every tile-walking kernel takes its tiles as one
// TileCtx (mgr_internal.h).  Helpers: mgr_device.h.
#include "mgr_device.h"

namespace mgr {

// a launch's kernel arguments hold at most 4 KB
static_assert(std::is_trivially_copyable<TileCtx>::value && std::is_trivially_copyable<SideIds>::value,
              "kernel arguments are copied bytewise");
static_assert(sizeof(TileCtx) + sizeof(SideIds) + 64 <= 4096, "the single-array packs' arguments exceed 4 KB");

// ------------------------------------------------------------------ pack
// Kernel 3 of the hot path.  Per round: ballot match -> rank inside the
// wave; slot = tile segment start of the bin + running count + rank; the
// row is copied straight to its slot.  Same-bin lanes hold consecutive
// slots, so each store instruction writes a few contiguous runs, and the
// runs of consecutive rounds continue each other (merged in L2).
// kWide (rows > 256 B): the wave copies one row at a time, 64 lanes wide.
template <int W, typename DestT, bool kWide>
__global__ __launch_bounds__(kBlock) void pack_kernel(
    TileCtx c, const uint8_t* __restrict__ src, int64_t upr /* W-units per row */,
    int per_wave_lds, uint8_t* __restrict__ dst, uint8_t* __restrict__ redirect_dst) {
    using U = typename Unit<W>::T;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int w = threadIdx.x >> 6, lane = lane_id();
    const int64_t tl = (int64_t)blockIdx.x * (blockDim.x >> 6) + w;
    if (tl >= c.tn || scan_failed(c)) return;
    const int64_t tile = c.t0 + tl;
    const int nb = c.nb, drop_bin = c.drop_bin, redirect_bin = c.redirect_bin;
    const DestT* __restrict__ dest = (const DestT*)c.dest;
    int64_t* goff = (int64_t*)(smem + w * per_wave_lds);
    int32_t* run = (int32_t*)(smem + w * per_wave_lds + align16(nb * 8));
    for (int b = lane; b < nb; b += 64) {
        goff[b] = seg_start(c, tile, b);
        run[b] = 0;
    }
    wave_sync();
    const int64_t row0 = tile * (int64_t)c.tile_rows;
    const int rows = (int)min((int64_t)c.tile_rows, c.n - row0);
    const U* __restrict__ s_u = (const U*)src;
    U* __restrict__ d_u = (U*)dst;
    U* __restrict__ r_u = (U*)redirect_dst;
    for (int r0 = 0; r0 < rows; r0 += 64) {
        const bool valid = r0 + lane < rows;
        const int64_t row = row0 + r0 + lane;
        const unsigned b = valid ? (unsigned)dest[row] : 0u;
        const unsigned long long peers = match_bin(b, valid, c.nbits);
        const int rk = rank_in(peers);
        int64_t slot = 0;
        if (valid) slot = goff[b] + run[b] + rk;
        wave_sync();
        if (valid && rk == 0) run[b] += __popcll(peers);
        const bool live = valid && (int)b != drop_bin;
        if (!kWide) {
            if (live) {
                const U* sp = s_u + row * upr;
                U* dp = ((int)b == redirect_bin ? r_u : d_u) + slot * upr;
                int64_t k = 0;
                for (; k + 4 <= upr; k += 4) {
                    const U a0 = sp[k], a1 = sp[k + 1], a2 = sp[k + 2], a3 = sp[k + 3];
                    dp[k] = a0; dp[k + 1] = a1; dp[k + 2] = a2; dp[k + 3] = a3;
                }
                for (; k < upr; ++k) dp[k] = sp[k];
            }
        } else {
            const unsigned long long todo = __ballot(live);
            for (int j = 0; j < 64; ++j) {
                if (!((todo >> j) & 1ull)) continue;
                const int bj = __shfl((int)b, j, 64);
                const int64_t sj = __shfl((long long)slot, j, 64);
                const U* sp = s_u + (row0 + r0 + j) * upr;
                U* dp = (bj == redirect_bin ? r_u : d_u) + sj * upr;
                for (int64_t k = lane; k < upr; k += 64) dp[k] = sp[k];
            }
        }
        wave_sync();
    }
}

// Block-cooperative pack for <= 64 bins and rows of <= 64 bytes: one
// workgroup per tile of R rounds, wave w ranks and moves round w (64 rows)
// in one shot -- the short-lived, fully parallel shape that streams best.
// The waves exchange their per-bin counts through a [R][64] LDS table (one
// barrier) to get each bin's base inside the tile.  Unit-transposed moves:
// lane l moves W-byte units 64k + l of the round, so each load instruction
// reads 64*W contiguous bytes; the unit's row gets its slot by shfl.
// (A/B, same box: issuing every load branch-free before the first wait, as
// the image pack does, made this kernel slower -- 0.86 vs 0.77 ms at config 2
// -- so the destination bytes are waited for before the payload loads go out.)
template <int W, int UPR, int RPW>
__global__ __launch_bounds__(1024) void pack_coop_kernel(
    TileCtx c, const uint8_t* __restrict__ src, const uint8_t* __restrict__ dest,
    const int64_t* __restrict__ offsets, const int64_t* __restrict__ bin_starts,
    const uint32_t* __restrict__ scan_err, uint8_t* __restrict__ dst,
    uint8_t* __restrict__ redirect_dst, int sel, SideIds ids) {
    // (dest, offsets, bin_starts, scan_err and sel stay direct parameters
    // here: read through the context, this kernel's register counts moved and
    // four instantiations changed occupancy, profiles/tile_ctx/resource_usage.md;
    // the context gives the rest)
    using U = typename Unit<W>::T;
    __shared__ int s_cnt[kCoopMaxRounds][64];
    const int w = threadIdx.x >> 6, lane = lane_id();
    const int64_t tile = tile_index(c);
    // wave w moves rounds w*RPW .. w*RPW+RPW-1 of the tile
    const int64_t row0 = tile * (int64_t)c.tile_rows + 64 * RPW * w;
    // issue every load of the wave's rounds first
    int nr[RPW];
    unsigned b[RPW];
    U v[RPW][UPR];
    unsigned idv[RPW];   // side field: every row's 2-byte id (fine cell), moved alike
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        nr[q] = (int)max((int64_t)0, min((int64_t)64, c.n - row0 - 64 * q));
        b[q] = lane < nr[q] ? (unsigned)dest[row0 + 64 * q + lane] : 0u;
        idv[q] = ids.src && lane < nr[q] ? (unsigned)ids.src[row0 + 64 * q + lane] : 0u;
    }
    long long tbase = 0;
    if (lane < c.nb) tbase = seg_start(offsets, bin_starts, c.T, tile, lane, c.redirect_bin);
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        const U* __restrict__ sp = (const U*)src + (row0 + 64 * q) * UPR;
        if (sel) {
            // selection (most rows dropped): load only the units of kept rows
#pragma unroll
            for (int k = 0; k < UPR; ++k) {
                const int u = 64 * k + lane;
                const int rb = __shfl((int)b[q], u / UPR, 64);
                if (u < nr[q] * UPR && rb != c.drop_bin) v[q][k] = sp[u];
            }
        } else {
#pragma unroll
            for (int k = 0; k < UPR; ++k)
                if (64 * k + lane < nr[q] * UPR) v[q][k] = sp[64 * k + lane];
        }
    }
    // rank inside each round; lane l counts bin l
    unsigned long long peers[RPW];
    int cnt[RPW];
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        cnt[q] = round_rank(b[q], lane < nr[q], lane, c.nbits, &peers[q]);
        s_cnt[w * RPW + q][lane] = cnt[q];
    }
    __syncthreads();
    if (scan_failed(scan_err)) return;
    for (int j = 0; j < w * RPW; ++j) tbase += s_cnt[j][lane];
    U* __restrict__ d_u = (U*)dst;
    U* __restrict__ r_u = (U*)redirect_dst;
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        const long long base = __shfl(tbase, (int)b[q], 64);
        long long tgt = -1;
        if (lane < nr[q] && (int)b[q] != c.drop_bin)
            tgt = tag_slot(base + rank_in(peers[q]), (int)b[q], c.redirect_bin);
        tbase += cnt[q];
        if (ids.src) store_side(ids.dst, ids.red, tgt, idv[q]);
#pragma unroll
        for (int k = 0; k < UPR; ++k) {
            const int u = 64 * k + lane;
            const int r = u / UPR, part = u - r * UPR;
            const long long t = __shfl(tgt, r, 64);
            if (u < nr[q] * UPR && t >= 0) {
                U* o = slot_redirected(t) ? r_u : d_u;
                o[slot_row(t) * UPR + part] = v[q][k];
            }
        }
    }
}

// Image pack for rows of RB bytes, RB a multiple of 4 but not of 16 (e.g.
// the 36-byte records of config 5), <= 64 bins: the cooperative shape of
// pack_coop_kernel (one wave per 64-row round, per-bin bases exchanged
// through LDS behind one barrier) but every global access is 16 bytes wide.
// The round (64 * RB bytes, 16-byte aligned) is loaded in 16-byte units,
// parked in wave-private LDS, each row moved to its slot of a round image
// ordered by destination (bin-major, stable), and the image stored back in
// 16-byte units: a unit inside one bin's run is one 16-byte store to the
// run's (4-byte aligned) place in the output, a unit straddling two runs is
// stored dword by dword.  Plain 4-byte units would need RB/4 load and RB/4
// store instructions per round instead of ~RB/16.
template <int RB, int RPW, bool SEL>
__global__ __launch_bounds__(1024) void pack_img_kernel(
    TileCtx c, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
    uint8_t* __restrict__ redirect_dst, SideIds ids) {
    static_assert(RB % 4 == 0 && RB % 16 != 0 && RB <= 64, "image pack row size");
    const int64_t n = c.n;
    const int nb = c.nb, drop_bin = c.drop_bin, redirect_bin = c.redirect_bin;
    const uint8_t* __restrict__ dest = (const uint8_t*)c.dest;
    constexpr int WR = 64 * RPW;                    // rows per wave (RPW consecutive rounds)
    constexpr int RBYTES = WR * RB;                 // the wave's rows, a multiple of 16
    constexpr int NU = (RBYTES / 16 + 63) / 64;     // 16-byte units per lane
    constexpr int DW = RB / 4;
    constexpr int WAVE_LDS = RBYTES + 64 * 8 + WR;  // image, per-bin output address, row bins
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int w = threadIdx.x >> 6, lane = lane_id();
    const int nw = blockDim.x >> 6;
    int* s_cnt = (int*)smem;                                    // [nw][64]
    uint8_t* img = smem + nw * 64 * 4 + w * WAVE_LDS;
    unsigned long long* gaddr = (unsigned long long*)(img + RBYTES);
    uint8_t* ibin = img + RBYTES + 64 * 8;
    uint32_t* imgw = (uint32_t*)img;
    const int64_t tile = tile_index(c);
    const int64_t row0 = tile * (int64_t)c.tile_rows + (int64_t)WR * w;
    const int nrows = (int)max((int64_t)0, min((int64_t)WR, n - row0));
    const int nbytes = nrows * RB;
    // every load issued first, branch-free (clamped indices; rows past n are
    // masked by valid / nbytes afterwards): the first wait -- for the
    // destination bytes -- leaves the payload and side loads in flight
    unsigned braw[RPW], b[RPW], idv[RPW];
    bool valid[RPW];
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        valid[q] = 64 * q + lane < nrows;
        const int64_t r = min(row0 + 64 * q + lane, n - 1);
        braw[q] = (unsigned)dest[r];
        idv[q] = ids.src ? (unsigned)ids.src[r] : 0u;  // side field
    }
    const SegLoad seg = seg_load(c, tile, lane);
    const uint8_t* __restrict__ sp = src + row0 * RB;
    u32x4_t v[NU];
    if constexpr (!SEL) {
        // a 16-byte unit that starts inside the array stays inside its page;
        // units past the wave's rows re-read the array's last one (never stored)
        const int64_t xmax = ((n * RB - 1) & ~(int64_t)15) - row0 * RB;
#pragma unroll
        for (int k = 0; k < NU; ++k)
            v[k] = *(const u32x4_t*)(sp + min((int64_t)(16 * (64 * k + lane)), xmax));
    }
#pragma unroll
    for (int q = 0; q < RPW; ++q) b[q] = valid[q] ? braw[q] : 0u;
    long long tbase = lane < nb ? seg_value(seg, lane, redirect_bin) : 0;
#pragma unroll
    for (int k = 0; k < NU && SEL; ++k) {
        const int x = 16 * (64 * k + lane);
        bool need = true;
        {   // selection: skip units whose rows (at most two, RB > 16) are all dropped
            const int r0 = min(x / RB, WR - 1), r1 = min((x + 15) / RB, WR - 1);
            int b0 = 0, b1 = 0;
#pragma unroll
            for (int q = 0; q < RPW; ++q) {
                const int t0 = __shfl((int)b[q], r0 & 63, 64), t1 = __shfl((int)b[q], r1 & 63, 64);
                if ((r0 >> 6) == q) b0 = t0;
                if ((r1 >> 6) == q) b1 = t1;
            }
            need = b0 != drop_bin || b1 != drop_bin;
        }
        if (!need) {
        } else if (x + 16 <= nbytes) {
            v[k] = *(const u32x4_t*)(sp + x);
        } else if (x < nbytes) {            // last partial unit of the array
            const uint32_t* q = (const uint32_t*)(sp + x);
            v[k] = u32x4_t{q[0], x + 4 < nbytes ? q[1] : 0u, x + 8 < nbytes ? q[2] : 0u,
                           x + 12 < nbytes ? q[3] : 0u};
        }
    }
    // rank inside each round; lane l counts bin l per round, cnt over the wave
    unsigned long long pe[RPW];
    int cq[RPW], cnt = 0;
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        cq[q] = round_rank(b[q], valid[q], lane, c.nbits, &pe[q]);
        cnt += cq[q];
    }
    s_cnt[w * 64 + lane] = cnt;
#pragma unroll
    for (int k = 0; k < NU; ++k) {
        const int x = 16 * (64 * k + lane);
        if (x < nbytes) *(u32x4_t*)(img + x) = v[k];
    }
    __syncthreads();
    if (scan_failed(c)) return;
    for (int j = 0; j < w; ++j) tbase += s_cnt[j * 64 + lane];
    // wave image order: exclusive prefix of the wave's bin counts
    const int excl = wave_incl_dpp(cnt) - cnt;
    int slot[RPW];
    int run = excl;   // lane b: bin b's next image slot, round by round
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        slot[q] = __shfl(run, (int)b[q], 64) + (valid[q] ? rank_in(pe[q]) : 0);
        run += cq[q];
    }
    if (lane < nb) {
        uint8_t* base = lane == redirect_bin ? redirect_dst : dst;
        gaddr[lane] = lane == drop_bin ? 0ull
                                       : (unsigned long long)(base + (tbase - excl) * (long long)RB);
    }
    if (ids.src) {   // the row's output row: its bin's (tile base - wave image start) + image slot
#pragma unroll
        for (int q = 0; q < RPW; ++q) {
            const long long gr = __shfl(tbase - excl, (int)b[q], 64) + slot[q];
            if (valid[q] && (int)b[q] != drop_bin)
                ((int)b[q] == redirect_bin ? ids.red : ids.dst)[gr] = (uint16_t)idv[q];
        }
    }
    uint32_t row[RPW][DW];
#pragma unroll
    for (int q = 0; q < RPW; ++q)
        if (valid[q]) {
#pragma unroll
            for (int p = 0; p < DW; ++p) row[q][p] = imgw[(64 * q + lane) * DW + p];
        }
    wave_sync();
#pragma unroll
    for (int q = 0; q < RPW; ++q)
        if (valid[q]) {
#pragma unroll
            for (int p = 0; p < DW; ++p) imgw[slot[q] * DW + p] = row[q][p];
            ibin[slot[q]] = (uint8_t)b[q];
        }
    wave_sync();
#pragma unroll
    for (int k = 0; k < NU; ++k) {
        const int x = 16 * (64 * k + lane);
        if (x < nbytes) store_img_unit<RB, true>(img, ibin, gaddr, x, nbytes);
    }
}

// Many-destination pack (65..1024 bins, e.g. the 512 fine cells of config
// 5) in the cooperative shape: one workgroup of 16 waves per tile of R = 16*RPW
// rounds, wave w ranking and moving rounds w*RPW.. with unit-transposed
// coalesced loads and stores.  The per-(round, bin) counts go to an LDS table
// (uint16 [R][nbins], written by each peer group's leader lane), one pass
// turns every bin column into an exclusive prefix over the rounds, and a
// row's slot = the tile's segment start of its bin (staged once per tile in
// LDS) + its round's prefix + its ballot rank.
template <int W, int UPR, typename DestT, int RPW>
__global__ __launch_bounds__(1024) void pack_many_kernel(
    TileCtx c, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
    uint8_t* __restrict__ redirect_dst) {
    using U = typename Unit<W>::T;
    constexpr int R = 16 * RPW;                                // rounds per super-round
    const int64_t n = c.n;
    const int nb = c.nb, tile_rows = c.tile_rows;
    const DestT* __restrict__ dest = (const DestT*)c.dest;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    long long* s_off = (long long*)smem;                       // [nb] running bin bases
    uint16_t* tab = (uint16_t*)(smem + align16(nb * 8));       // [R][nb]
    const int w = threadIdx.x >> 6, lane = lane_id();
    const int64_t tile = tile_index(c);
    if (scan_failed(c)) return;
    for (int bb = threadIdx.x; bb < nb; bb += blockDim.x) s_off[bb] = seg_start(c, tile, bb);
    U* __restrict__ d_u = (U*)dst;
    U* __restrict__ r_u = (U*)redirect_dst;
    // the tile's super-rounds of 64 * R rows, in order: a bin's rows of
    // consecutive super-rounds continue each other's output run, so the
    // tile writes one run of ~tile_rows / nb rows per bin
    for (int64_t sr0 = tile * (int64_t)tile_rows; sr0 < min(n, (tile + 1) * (int64_t)tile_rows);
         sr0 += 64 * R) {
        const int64_t row0 = sr0 + 64 * RPW * w;
        for (int i = threadIdx.x; i < R * nb; i += blockDim.x) tab[i] = 0;
        int nr[RPW];
        unsigned b[RPW];
        U v[RPW][UPR];
#pragma unroll
        for (int q = 0; q < RPW; ++q) {
            nr[q] = (int)max((int64_t)0, min((int64_t)64, n - row0 - 64 * q));
            b[q] = lane < nr[q] ? (unsigned)dest[row0 + 64 * q + lane] : 0u;
        }
#pragma unroll
        for (int q = 0; q < RPW; ++q) {
            const U* __restrict__ sp = (const U*)src + (row0 + 64 * q) * UPR;
#pragma unroll
            for (int k = 0; k < UPR; ++k)
                if (64 * k + lane < nr[q] * UPR) v[q][k] = sp[64 * k + lane];
        }
        __syncthreads();   // table zeroed (and, first time, tile offsets staged)
        unsigned long long peers[RPW];
#pragma unroll
        for (int q = 0; q < RPW; ++q) {
            const bool valid = lane < nr[q];
            peers[q] = match_bin(b[q], valid, c.nbits);
            if (valid && rank_in(peers[q]) == 0)
                tab[(w * RPW + q) * nb + b[q]] = (uint16_t)__popcll(peers[q]);
        }
        __syncthreads();
        // per bin (one per thread, nb <= 1024): exclusive prefix over the
        // super-round's rounds; the total moves the bin's running base later
        int total = 0;
        if (threadIdx.x < nb) {
            const int bb = threadIdx.x;
            for (int r = 0; r < R; ++r) {
                const int c = tab[r * nb + bb];
                tab[r * nb + bb] = (uint16_t)total;
                total += c;
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < RPW; ++q) {
            long long tgt = -1;
            if (lane < nr[q] && (int)b[q] != c.drop_bin)
                tgt = tag_slot(s_off[b[q]] + tab[(w * RPW + q) * nb + b[q]] + rank_in(peers[q]),
                               (int)b[q], c.redirect_bin);
#pragma unroll
            for (int k = 0; k < UPR; ++k) {
                const int u = 64 * k + lane;
                const int r = u / UPR, part = u - r * UPR;
                const long long t = __shfl(tgt, r, 64);
                if (u < nr[q] * UPR && t >= 0) {
                    U* o = slot_redirected(t) ? r_u : d_u;
                    o[slot_row(t) * UPR + part] = v[q][k];
                }
            }
        }
        __syncthreads();   // every base and prefix read before they move on
        if (threadIdx.x < nb) s_off[threadIdx.x] += total;
    }
}

typedef unsigned int u32x3_a4 __attribute__((ext_vector_type(3), aligned(4)));
typedef unsigned int u32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));

// One row of NDW dwords (4-byte aligned) into registers: 16-byte loads and a tail.
template <int NDW>
__device__ __forceinline__ void load_row_dw(const uint8_t* __restrict__ p, uint32_t (&v)[NDW]) {
    int i = 0;
#pragma unroll
    for (; i + 4 <= NDW; i += 4) {
        const u32x4_a4 x = *(const u32x4_a4*)(p + 4 * i);
        v[i] = x[0]; v[i + 1] = x[1]; v[i + 2] = x[2]; v[i + 3] = x[3];
    }
    if constexpr (NDW % 4 == 3) {
        const u32x3_a4 x = *(const u32x3_a4*)(p + 4 * i);
        v[i] = x[0]; v[i + 1] = x[1]; v[i + 2] = x[2];
    } else if constexpr (NDW % 4 == 2) {
        const u32x2_a4 x = *(const u32x2_a4*)(p + 4 * i);
        v[i] = x[0]; v[i + 1] = x[1];
    } else if constexpr (NDW % 4 == 1) {
        v[i] = *(const uint32_t*)(p + 4 * i);
    }
}

constexpr int kFineTR = 2048;      // ranked tiles when a 4096-row image does not fit
constexpr int kFineWaves = 16;     // ranked pack: 1024 threads

// fn(std::integral_constant<int, UPR>) for upr = the row's units of W bytes,
// UPR at compile time: rows of <= 64 bytes in 16/8/4-byte units (1..4, 1..8,
// 1..16 units: registers, no scratch); hipErrorNotSupported for other shapes.
template <int W, typename Fn>
static hipError_t dispatch_upr(int64_t upr, Fn fn) {
#define MGR_UPR(U_) case U_: return fn(std::integral_constant<int, U_>{});
    switch ((int)upr) {
        MGR_UPR(1) MGR_UPR(2) MGR_UPR(3) MGR_UPR(4)
        default: break;
    }
    if constexpr (W <= 8) {
        switch ((int)upr) {
            MGR_UPR(5) MGR_UPR(6) MGR_UPR(7) MGR_UPR(8)
            default: break;
        }
    }
    if constexpr (W == 4) {
        switch ((int)upr) {
            MGR_UPR(9) MGR_UPR(10) MGR_UPR(11) MGR_UPR(12) MGR_UPR(13) MGR_UPR(14) MGR_UPR(15) MGR_UPR(16)
            default: break;
        }
    }
#undef MGR_UPR
    return hipErrorNotSupported;
}

// pack_many_kernel: one super-round of 64 * R rows per tile (the uint16
// [R][nbins] LDS table stays <= 128 KiB at 4096 rows and 1024 bins; A/B: 2-16
// super-rounds per tile, i.e. longer per-bin runs, measured slower).
// Up to 512 bins 2048-row super-rounds (8x8x8 cells, 64M 36-byte rows: pack
// 1.43-1.49 vs 1.55-1.70 ms at 4096 rows and 1.70 at 1024; the bin kernel and
// the scan pay ~+0.05 ms each for the twice larger histogram; whole sort 2.17-2.24
// vs 2.19-2.34 ms; 120 cells 1.85 vs 2.03 ms); above 512 bins 4096 rows (1024
// cells: 2.53 vs 2.84 ms -- there the [bins][tiles] histogram dominates).
// profiles/round1/fine_many_ab.log, fine_shapes_ab.log.
static int many_round_rows(int nbins) { return nbins <= 512 ? 2048 : 4096; }

int pack_tile_rows(int64_t row_bytes, int nbins) {
    const int tr = hooks().tile_rounds;   // one snapshot
    if (tr > 0) return 64 * tr;
    // <= 16 bins: 512-row tiles (bin: 4 waves x 2 rounds; pack: 8 waves x
    // 1 round; A/B against 1024 at 8 bins: bin -3 %, pack within noise);
    // <= 64 bins: 1024 rows (64 bins: pack 0.92 vs 1.07 ms at 512: longer
    // same-bin runs); more bins: longer tiles keep the [nbins][tiles]
    // histogram small next to the payload.
    // rows the image pack takes (4-byte, not 16-byte multiples, 24..60 B, e.g.
    // config 5's 36-B records): 1024-row tiles (2 rounds x 8 waves per image
    // workgroup; A/B at 36 B: bin 0.382 vs 0.418, scan 0.014 vs 0.023, pack
    // 0.850 vs 0.856 ms per 64M)
    const bool img = row_bytes % 4 == 0 && row_bytes % 16 != 0 && row_bytes >= 24 && row_bytes <= 60;
    if (nbins <= 16) return img ? 1024 : 512;
    if (nbins <= 64) return 1024;
    if (nbins <= 1024 && row_bytes <= 64) return many_round_rows(nbins);
    int r = 16;
    while (r < 4096 / 64 && (int64_t)nbins * 4 > (int64_t)r * 8) r *= 2;
    return 64 * r;
}

template <int W, typename DestT, bool kWide>
static hipError_t pack_t(const PackJob& j) {
    auto k = pack_kernel<W, DestT, kWide>;
    const int per_wave = align16(j.c.nb * 8) + align16(j.c.nb * 4);
    const int wpb = waves_per_block(per_wave);
    const int lds = per_wave * wpb;
    ensure_lds(k, lds);
    const int64_t grid = (j.c.tn + wpb - 1) / wpb;
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(64 * wpb), (size_t)lds, j.s, j.c,
                       (const uint8_t*)j.src, j.row_bytes / W, per_wave, (uint8_t*)j.dst,
                       (uint8_t*)j.redirect);
    return hipGetLastError();
}

// The job's side field as the kernels take it (none: all null).
static SideIds side_ids(const PackJob& j) { return j.side ? j.side->ids : SideIds{}; }

// (selection packs -- TileCtx::selection -- skip the loads of dropped rows;
// elsewhere loads go out before the bins are known)
template <int W, int UPR, int RPW>
static void launch_pack_coop(const PackJob& j, int threads) {
    hipLaunchKernelGGL((pack_coop_kernel<W, UPR, RPW>), dim3((unsigned)j.c.tn), dim3(threads), 0,
                       j.s, j.c, (const uint8_t*)j.src, (const uint8_t*)j.c.dest, j.c.offsets,
                       j.c.bin_starts, j.c.scan_err, (uint8_t*)j.dst, (uint8_t*)j.redirect,
                       (int)j.c.selection(), side_ids(j));
}

template <int W, int UPR>
static hipError_t pack_coop_u(const PackJob& j) {
    const int tile_rows = j.c.tile_rows;
    if (j.h.pack_generic || tile_rows > 2048) return hipErrorNotSupported;
    // one wave per RPW 64-row rounds of the tile (<= 16 waves)
    const int rpw = tile_rows > 1024 ? 2 : 1;
    if (j.side) j.side->used = j.side->ids.src != nullptr;
    if (rpw == 2) launch_pack_coop<W, UPR, 2>(j, tile_rows / 2);
    else launch_pack_coop<W, UPR, 1>(j, tile_rows);
    return hipGetLastError();
}

template <int W, int UPR, typename DestT, int RPW>
static void launch_pack_many(const PackJob& j, int lds) {
    auto k = pack_many_kernel<W, UPR, DestT, RPW>;
    ensure_lds(k, lds);
    hipLaunchKernelGGL(k, dim3((unsigned)j.c.tn), dim3(1024), (size_t)lds, j.s, j.c,
                       (const uint8_t*)j.src, (uint8_t*)j.dst, (uint8_t*)j.redirect);
}

template <int W, int UPR, typename DestT>
static hipError_t pack_many_u(const PackJob& j) {
    const int round_rows = many_round_rows(j.c.nb);
    if (j.c.tile_rows % round_rows) return hipErrorNotSupported;
    const int lds = align16(j.c.nb * 8) + (round_rows / 64) * j.c.nb * 2;
    if (round_rows == 4096) launch_pack_many<W, UPR, DestT, 4>(j, lds);
    else if (round_rows == 2048) launch_pack_many<W, UPR, DestT, 2>(j, lds);
    else return hipErrorNotSupported;
    return hipGetLastError();
}

template <int RB>
static hipError_t pack_img_t(const PackJob& j) {
    // two 64-row rounds per wave (A/B, 36-B records: 0.90-0.92 vs 1.02-1.05
    // ms per 64M with one, 4: 1.17 -- a wave's fixed per-round chain of load,
    // count exchange, LDS permutation and store then moves twice the rows);
    // tiles that are not a multiple of two rounds go to the coop pack
    constexpr int rpw = kImgRoundsPerWave;
    if (j.c.tile_rows % (64 * rpw)) return hipErrorNotSupported;
    const int nw = j.c.tile_rows / (64 * rpw);
    const int lds = nw * 64 * 4 + nw * (64 * rpw * RB + 64 * 8 + 64 * rpw);
    auto k = j.c.selection() ? pack_img_kernel<RB, rpw, true> : pack_img_kernel<RB, rpw, false>;
    ensure_lds(k, lds);
    hipLaunchKernelGGL(k, dim3((unsigned)j.c.tn), dim3(64 * nw), (size_t)lds, j.s, j.c,
                       (const uint8_t*)j.src, (uint8_t*)j.dst, (uint8_t*)j.redirect,
                       side_ids(j));
    if (j.side) j.side->used = j.side->ids.src != nullptr;
    return hipGetLastError();
}

static int g_cus = 0;   // compute units of the current device (persistent grids)
static int device_cus() {
    if (g_cus <= 0) {
        int dev = 0, c = 0;
        if (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess)
            g_cus = c;
        if (g_cus <= 0) g_cus = 256;
    }
    return g_cus;
}

// Ranked sorted-image pack (mgr_pack_ranked), the stable sort of 65..1024
// bins (config 5's fine cells): every row's rank inside (tile, bin) and every
// tile's bin starts come from mgr_rank_ids, so a tile is: load (a tile
// ahead), rows into the LDS image at tile_start[bin] + rank, stream the image
// out in 16-byte units (a unit inside one bin's run is one 16-byte store to
// the run's place, a unit straddling two runs goes dword by dword).
// Persistent: one 1024-thread workgroup per CU (the image fills most of the
// LDS) walks its XCD's tiles, the workgroups of an XCD on adjacent tiles at a
// time (the lines their runs share meet in one L2).  No ballots, no per-tile
// count table, three barriers per tile.
template <int RB, int TR>
__global__ __launch_bounds__(1024) void pack_ranked_kernel(
    const uint8_t* __restrict__ src, int64_t n, const uint16_t* __restrict__ ids,
    const uint16_t* __restrict__ ranks, const uint16_t* __restrict__ tile_starts, int nb,
    const int64_t* __restrict__ offsets, int64_t T, uint8_t* __restrict__ dst,
    const uint32_t* __restrict__ scan_err) {
    static_assert(RB % 4 == 0 && RB <= 64, "ranked pack row size");
    constexpr int NW = kFineWaves, RPW = TR / 64 / NW;
    constexpr int NDW = RB / 4;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t* img = (uint32_t*)smem;
    uint8_t* p = smem + align16(TR * RB);
    uint16_t* ibin = (uint16_t*)p;                 p += align16(TR * 2);
    unsigned long long* gaddr = (unsigned long long*)p;
    if (scan_failed(scan_err)) return;
    const int tid = threadIdx.x, w = tid >> 6, lane = lane_id();
    // tile walk: XCD x owns tiles [x*per, (x+1)*per), its gx workgroups on
    // gx adjacent tiles at a time, so the lines that adjacent tiles' runs
    // share meet in one L2 (A/B: all 8 XCDs on one region of the input at a
    // time measured no better)
    const int64_t per = (T + 7) >> 3;
    const int gx = (int)(gridDim.x >> 3), kx = (int)(blockIdx.x >> 3), xx = (int)(blockIdx.x & 7);
    const int64_t first = (int64_t)xx * per + kx;
    const int64_t stride = gx;
    const int64_t last = min(T, (int64_t)xx * per + per);
    const int mb = min(tid, nb - 1);
    struct Set {
        uint32_t v[RPW][NDW];
        unsigned b[RPW];
        unsigned rk[RPW];
        long long seg;
        unsigned ls;
    };
    auto load = [&](Set& S, int64_t t) __attribute__((always_inline)) {
        t = min(t, last - 1);
        S.seg = offsets[(int64_t)mb * T + t];
        S.ls = tile_starts[t * nb + mb];
#pragma unroll
        for (int q = 0; q < RPW; ++q) {
            const int64_t row = min(t * TR + (int64_t)(w * RPW + q) * 64 + lane, n - 1);
            S.b[q] = min((unsigned)ids[row], (unsigned)(nb - 1));   // ids >= nb: clamped (mgr_rank_ids reports them)
            S.rk[q] = ranks[row];
            load_row_dw<NDW>(src + row * RB, S.v[q]);
        }
    };
    // (A/Bs, round 4, profiles/round4/ab_notes.md: a branch-free scatter,
    // which let the compiler keep the next tile's loads in flight through the
    // store phase, measured SLOWER (1.14 vs 1.10 ms, with or without a fully
    // unrolled store loop); so did the rows stored straight from registers
    // to their slots by small workgroups, no LDS image (1.50-1.96 ms).  With
    // every store sent sequentially to the tile's own region this kernel
    // takes 0.95 ms: the one 1024-thread workgroup per CU that the image
    // needs is the ceiling, the run scatter adds 0.15 ms.)
    auto process = [&](Set& S, int64_t t) __attribute__((always_inline)) {
        const int tr = (int)min((int64_t)TR, n - t * TR);
        if (tid < nb) gaddr[tid] = (unsigned long long)(dst + (S.seg - (long long)S.ls) * (long long)RB);
        __syncthreads();
#pragma unroll
        for (int q = 0; q < RPW; ++q) {
            if ((w * RPW + q) * 64 + lane < tr) {
                const int lpos = S.rk[q];   // the row's slot in the tile (mgr_rank_ids)
#pragma unroll
                for (int i = 0; i < NDW; ++i) img[lpos * NDW + i] = S.v[q][i];
                ibin[lpos] = (uint16_t)S.b[q];
            }
        }
        __syncthreads();
        const int nbytes = tr * RB;
        // (the image pack's two-address unit store, store_img_unit, measured
        // 12 % slower here)
        for (int x = 16 * tid; x < nbytes; x += 16 * 1024) {
            const u32x4_t q = *(const u32x4_t*)((const uint8_t*)img + x);
            const int bf = ibin[x / RB];
            if (x + 16 <= nbytes && ibin[(x + 15) / RB] == bf) {
                gstore<u32x4_a4>(gaddr[bf] + x, q);
            } else {
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const int xd = x + 4 * d;
                    if (xd < nbytes) gstore<uint32_t>(gaddr[ibin[xd / RB]] + xd, q[d]);
                }
            }
        }
        __syncthreads();   // the image, ibin and gaddr are reused by the next tile
    };
    Set A, B;
    int64_t t = first;
    if (t >= last) return;
    load(A, t);
    for (;;) {
        load(B, t + stride);
        process(A, t);
        t += stride;
        if (t >= last) break;
        load(A, t + stride);
        process(B, t);
        t += stride;
        if (t >= last) break;
    }
}

// LDS of the ranked pack: the tile image, its row bins and per-bin output
// addresses.
static int ranked_lds_bytes(int tile_rows, int64_t row_bytes, int nbins) {
    return align16(tile_rows * (int)row_bytes) + align16(tile_rows * 2) + nbins * 8;
}
// Ranked tiles: 4096 rows when their image fits the LDS (36-byte rows: 157 KiB),
// else 2048.  Longer tiles halve the [bins][tiles] histogram the scan walks and
// the per-tile fixed work (A/B: profiles/round2/ab_notes.md).
int ranked_tile_rows(int64_t row_bytes, int nbins) {
    if (row_bytes < 1 || row_bytes % 4 || row_bytes > 64 || nbins < 1 || nbins > 1024) return 0;
    const int want = hooks().rank_rows;
    if (want != 2048 && ranked_lds_bytes(4096, row_bytes, nbins) <= 160 * 1024) return 4096;
    return ranked_lds_bytes(kFineTR, row_bytes, nbins) <= 160 * 1024 ? kFineTR : 0;
}

hipError_t launch_pack_ranked(const void* src, int64_t row_bytes, int64_t n, const uint16_t* ids,
                              const uint16_t* ranks, const uint16_t* tile_starts, int nbins,
                              int tile_rows, const Workspace& ws, void* dst, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if ((tile_rows != kFineTR && tile_rows != 4096) || row_bytes % 4 || row_bytes > 64 ||
        ((uintptr_t)src & 3) || ((uintptr_t)dst & 3))
        return hipErrorNotSupported;
    const int lds = ranked_lds_bytes(tile_rows, row_bytes, nbins);
    if (lds > 160 * 1024) return hipErrorNotSupported;
    prof_begin(s, K_PACK_FINE);
    hipError_t e = hipErrorNotSupported;
    // one persistent workgroup per CU (A/B, round 6: as many per CU as the LDS
    // holds -- two to four for the 4..12-byte fields of a SoA payload --
    // measured slower, 0.41 vs 0.36 ms per field launch at 64M rows)
    int64_t grid = ((int64_t)device_cus() + 7) / 8 * 8;
    const int64_t need = (ws.T + 7) / 8 * 8;
    if (grid > need) grid = need;
#define MGR_PRT(RB_, TR_)                                                                     \
    {                                                                                         \
        auto k = pack_ranked_kernel<RB_, TR_>;                                                \
        ensure_lds(k, lds);                                                                   \
        hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(1024), (size_t)lds, s,               \
                           (const uint8_t*)src, n, ids, ranks, tile_starts, nbins,            \
                           ws.offsets, ws.T, (uint8_t*)dst, ws.scan_err);                     \
        e = hipGetLastError();                                                                \
    }
#define MGR_PR(RB_)                                                                           \
    case RB_:                                                                                 \
        if (tile_rows == 4096) MGR_PRT(RB_, 4096) else MGR_PRT(RB_, kFineTR)                  \
        break;
    switch ((int)row_bytes) {
        MGR_PR(4) MGR_PR(8) MGR_PR(12) MGR_PR(16) MGR_PR(20) MGR_PR(24) MGR_PR(28) MGR_PR(32)
        MGR_PR(36)
        default: break;
    }
    if (e == hipErrorNotSupported && tile_rows == kFineTR) {
        switch ((int)row_bytes) {
#undef MGR_PR
#define MGR_PR(RB_) case RB_: MGR_PRT(RB_, kFineTR) break;
            MGR_PR(40) MGR_PR(44) MGR_PR(48) MGR_PR(52) MGR_PR(56) MGR_PR(60) MGR_PR(64)
            default: break;
        }
    }
#undef MGR_PR
#undef MGR_PRT
    prof_end(s, K_PACK_FINE);
    return e;
}

// Rows of 24..60 (pack_img 2: 12..60) bytes, 4-byte multiples but not 16-byte ones: the
// image pack (16-byte global accesses) when the source is 16-byte aligned,
// the outputs 4-byte aligned, <= 64 bins and <= 16 waves per tile.
static hipError_t pack_img(const PackJob& j) {
    uintptr_t a = (uintptr_t)j.dst | (uintptr_t)j.row_bytes | (uintptr_t)j.redirect;
    // pack_img 1: rows of >= 24 bytes (A/B: 36 B 0.90 vs 1.05 ms, 40 B 0.97 vs
    // 1.00, 24 B 0.70 vs 0.71; 12 B 0.56 vs 0.48 -- the LDS passes cost more
    // than narrow units for small rows); 2: every size it takes (tests)
    const int64_t min_rb = j.h.pack_img_all ? 12 : 24;
    if (((uintptr_t)j.src & 15) || (a & 3) || j.row_bytes % 16 == 0 ||
        j.row_bytes < min_rb || j.row_bytes > 60 || j.c.nb > 64 || j.c.tile_rows > 1024 ||
        dest_bytes(j.c.nb) != 1)
        return hipErrorNotSupported;
#define MGR_PI(RB_) case RB_: return pack_img_t<RB_>(j);
    switch ((int)j.row_bytes) {
        MGR_PI(12) MGR_PI(20) MGR_PI(24) MGR_PI(28) MGR_PI(36) MGR_PI(40) MGR_PI(44)
        MGR_PI(52) MGR_PI(56) MGR_PI(60)
        default: break;
    }
#undef MGR_PI
    return hipErrorNotSupported;
}

// The pack of one array in W-byte units: the many-bin, cooperative or
// wave-per-tile kernel its shape takes.
template <int W>
static hipError_t pack_w(const PackJob& j) {
    const int nb = j.c.nb;
    const bool dest8 = dest_bytes(nb) == 1;
    if constexpr (W >= 4) {
        const int64_t upr = j.row_bytes / W;
        if (nb > 64 && nb <= 1024 && j.row_bytes <= 64 && j.c.tile_rows == many_round_rows(nb)) {
            const hipError_t e = dispatch_upr<W>(upr, [&](auto u) {
                return dest8 ? pack_many_u<W, u(), uint8_t>(j) : pack_many_u<W, u(), uint16_t>(j);
            });
            if (e != hipErrorNotSupported) return e;
        }
        if (nb <= 64 && j.row_bytes <= 64) {
            const hipError_t e = dispatch_upr<W>(upr, [&](auto u) { return pack_coop_u<W, u()>(j); });
            if (e != hipErrorNotSupported) return e;
        }
    }
    if constexpr (W == 2) {   // 2-byte rows (the fine cells travelling with config-5 rows)
        if (nb <= 64 && j.row_bytes == 2) {
            PackJob plain = j;   // the side field is left to its own pack
            plain.side = nullptr;
            const hipError_t e = pack_coop_u<2, 1>(plain);
            if (e != hipErrorNotSupported) return e;
        }
    }
    const bool wide = j.row_bytes > 256;
    if (dest8) return wide ? pack_t<W, uint8_t, true>(j) : pack_t<W, uint8_t, false>(j);
    return wide ? pack_t<W, uint16_t, true>(j) : pack_t<W, uint16_t, false>(j);
}

static hipError_t launch_pack_rows(const void* src, int64_t row_bytes, const TileCtx& c, void* dst,
                                   void* redirect_dst, hipStream_t s, SideField* side) {
    // one snapshot of the hooks for the whole launch
    const PackJob j{src, row_bytes, dst, redirect_dst, s, side, hooks(), c};
    // profiler: narrow (< 4-byte) rows apart
    const int kid = row_bytes < 4 ? K_PACK_NARROW : K_PACK;
    prof_begin(s, kid);
    hipError_t e = pack_img(j);
    if (e == hipErrorNotSupported) {
        // the widest unit dividing the row and every base address
        switch (unit_log((uintptr_t)src | (uintptr_t)dst | (uintptr_t)row_bytes |
                         (uintptr_t)redirect_dst)) {
            case 4: e = pack_w<16>(j); break;
            case 3: e = pack_w<8>(j); break;
            case 2: e = pack_w<4>(j); break;
            case 1: e = pack_w<2>(j); break;
            default: e = pack_w<1>(j); break;
        }
    }
    prof_end(s, kid);
    return e;
}

hipError_t launch_pack_array(const void* src, int64_t row_bytes, const TileCtx& c, void* dst,
                             void* redirect_dst, hipStream_t s, const SideIds& ids) {
    SideField side{ids, false};
    hipError_t e = launch_pack_rows(src, row_bytes, c, dst, redirect_dst, s, ids.src ? &side : nullptr);
    const bool rest = ids.src && !side.used;
    if (e != hipSuccess || !rest) return e;
    // the kernel that moved the rows cannot carry the ids: a 2-byte-row pack
    return launch_pack_rows(ids.src, 2, c, ids.dst, ids.red, s, nullptr);
}

hipError_t launch_pack(const void* src, int64_t row_bytes, int64_t n, const void* dest,
                       int nbins, int drop_bin, int tile_rows, const Workspace& ws, void* dst,
                       int redirect_bin, void* redirect_dst, hipStream_t s, const uint16_t* ids_src,
                       uint16_t* ids_dst, uint16_t* ids_red) {
    if (n <= 0) return hipSuccess;
    return launch_pack_array(src, row_bytes, tile_ctx(n, dest, nbins, drop_bin, tile_rows, ws, redirect_bin),
                             dst, redirect_dst, s, SideIds{ids_src, ids_dst, ids_red});
}

}  // namespace mgr
