// Unpack kernels (gfx950): the return path, the inverse of the packs of
// mgr_pack.hip and mgr_pack_fields.hip.  For the (dest, nbins, drop_bin,
// tile_rows, workspace, redirect_bin) of a pack, slot(r) is the row at which
// that pack writes source row r (redist.py:195-199, send_buff[i] = data[rank_to_send == i],
// order kept -- the permutation being inverted); the unpack writes
// out[r] = packed[slot(r)] (redirect_src[slot(r)] for a row of redirect_bin,
// zero bytes for a row of drop_bin).  The slot arithmetic is the pack's own
// (seg_start, the ballot match and rank of mgr_device.h); nothing is binned
// or scanned again.  Helpers: mgr_device.h.
#include "mgr_device.h"

namespace mgr {

constexpr int kUnpackCoopRounds = 16;   // cooperative unpack tiles: <= 1024 rows (one wave a round)

// ---------------------------------------------------------------- generic
// Mirror of pack_kernel: one wave per tile, per-wave LDS goff/run tables, any
// row size in W-byte units, 1- or 2-byte destinations.  Per round: ballot
// match -> rank inside the wave; slot = tile segment start of the bin +
// running count + rank; the row is copied from its slot to its own place.
// kWide (rows > 256 B): the wave copies one row at a time, 64 lanes wide.
template <int W, typename DestT, bool kWide>
__global__ __launch_bounds__(kBlock) void unpack_kernel(
    TileCtx c, const uint8_t* __restrict__ packed, int64_t upr /* W-units per row */,
    int per_wave_lds, uint8_t* __restrict__ out, const uint8_t* __restrict__ redirect_src) {
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
    const U* __restrict__ p_u = (const U*)packed;
    const U* __restrict__ r_u = (const U*)redirect_src;
    U* __restrict__ o_u = (U*)out;
    const U zero{};
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
                const U* sp = ((int)b == redirect_bin ? r_u : p_u) + slot * upr;
                U* dp = o_u + row * upr;
                int64_t k = 0;
                for (; k + 4 <= upr; k += 4) {
                    const U a0 = sp[k], a1 = sp[k + 1], a2 = sp[k + 2], a3 = sp[k + 3];
                    dp[k] = a0; dp[k + 1] = a1; dp[k + 2] = a2; dp[k + 3] = a3;
                }
                for (; k < upr; ++k) dp[k] = sp[k];
            } else if (valid) {   // a dropped row: zero bytes
                U* dp = o_u + row * upr;
                for (int64_t k = 0; k < upr; ++k) dp[k] = zero;
            }
        } else {
            const unsigned long long todo = __ballot(valid);
            for (int j = 0; j < 64; ++j) {
                if (!((todo >> j) & 1ull)) continue;
                const int bj = __shfl((int)b, j, 64);
                const int64_t sj = __shfl((long long)slot, j, 64);
                U* dp = o_u + (row0 + r0 + j) * upr;
                if (bj == drop_bin) {
                    for (int64_t k = lane; k < upr; k += 64) dp[k] = zero;
                } else {
                    const U* sp = (bj == redirect_bin ? r_u : p_u) + sj * upr;
                    for (int64_t k = lane; k < upr; k += 64) dp[k] = sp[k];
                }
            }
        }
        wave_sync();
    }
}

// ------------------------------------------------------------ cooperative
// Mirror of pack_coop_kernel / pack_coop_fields_kernel, <= 64 bins and rows
// of <= 16 units of 4/8/16 bytes: one workgroup per tile, wave w ranks round
// w (64 rows) -- lane b fetches bin b's tile base, the waves exchange their
// per-bin counts through a [rounds][64] LDS table behind one barrier -- and
// moves up to four fields of the round from that ONE ranking.  The moves are
// unit-transposed: lane l owns units 64 k + l of the round, takes its row's
// slot by shfl, gathers packed[slot * UPR + part] and stores out[row0 * UPR +
// 64 k + l], so every store instruction writes 64 * W contiguous bytes; the
// gathers read a few contiguous runs (same-bin rows of a round hold
// consecutive slots).  The destination bytes are loaded and waited for
// first: every gather address depends on them.  A field is U = W * 32 + UPR
// (0: no field), as the pack's CoopField.
template <int U>
struct CoopGather {
    static constexpr int W = U >> 5, UPR = U & 31;
    using T = typename Unit<(W ? W : 4)>::T;
    T v[UPR ? UPR : 1];
    // tgt: this lane's row's tagged slot (redirect bit: in redirect_src), < 0: a dropped row
    __device__ __forceinline__ void load(const uint8_t* __restrict__ packed,
                                         const uint8_t* __restrict__ red, long long tgt, int nr,
                                         int lane) {
        if constexpr (U != 0) {
            const T* __restrict__ p_u = (const T*)packed;
            const T* __restrict__ r_u = (const T*)red;
#pragma unroll
            for (int k = 0; k < UPR; ++k) {
                const int u = 64 * k + lane;
                const int r = u / UPR, part = u - r * UPR;
                const long long t = __shfl(tgt, r, 64);
                v[k] = T{};
                if (u < nr * UPR && t >= 0) {
                    const T* s = slot_redirected(t) ? r_u : p_u;
                    v[k] = s[slot_row(t) * UPR + part];
                }
            }
        }
    }
    __device__ __forceinline__ void store(uint8_t* __restrict__ out, int64_t row0, int nr,
                                          int lane) const {
        if constexpr (U != 0) {
            T* __restrict__ o_u = (T*)out + row0 * UPR;
#pragma unroll
            for (int k = 0; k < UPR; ++k)
                if (64 * k + lane < nr * UPR) o_u[64 * k + lane] = v[k];
        }
    }
};

struct UnpackFieldPtrs {
    const uint8_t* packed[4];
    const uint8_t* red[4];
    uint8_t* out[4];
};

template <int U0, int U1, int U2, int U3>
__global__ __launch_bounds__(1024) void unpack_coop_kernel(
    TileCtx c, UnpackFieldPtrs fp) {
    __shared__ int s_cnt[kUnpackCoopRounds][64];
    const int w = threadIdx.x >> 6, lane = lane_id();
    const int64_t tile = tile_index(c);
    const int64_t row0 = tile * (int64_t)c.tile_rows + 64 * w;
    const int nr = (int)max((int64_t)0, min((int64_t)64, c.n - row0));
    const uint8_t* __restrict__ dest = (const uint8_t*)c.dest;
    const unsigned b = lane < nr ? (unsigned)dest[row0 + lane] : 0u;
    long long tbase = 0;
    if (lane < c.nb) tbase = seg_start(c, tile, lane);
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
    CoopGather<U0> f0;
    CoopGather<U1> f1;
    CoopGather<U2> f2;
    CoopGather<U3> f3;
    f0.load(fp.packed[0], fp.red[0], tgt, nr, lane);
    f1.load(fp.packed[1], fp.red[1], tgt, nr, lane);
    f2.load(fp.packed[2], fp.red[2], tgt, nr, lane);
    f3.load(fp.packed[3], fp.red[3], tgt, nr, lane);
    f0.store(fp.out[0], row0, nr, lane);
    f1.store(fp.out[1], row0, nr, lane);
    f2.store(fp.out[2], row0, nr, lane);
    f3.store(fp.out[3], row0, nr, lane);
}

// --------------------------------------------------------------- launchers
// (unit widths and field signatures: unit_log, coop_unit of mgr_internal.h)
static bool coop_shape(int nbins, int tile_rows) {
    return nbins <= 64 && dest_bytes(nbins) == 1 && tile_rows <= 64 * kUnpackCoopRounds;
}

static_assert(std::is_trivially_copyable<UnpackFieldPtrs>::value &&
              sizeof(TileCtx) + sizeof(UnpackFieldPtrs) <= 4096,
              "unpack_coop_kernel's arguments: copied bytewise, at most 4 KB");

// The unpacks take a PackJob (mgr_internal.h) read backwards: src = the
// packed rows, redirect = the redirect bin's source (read only), dst = the output.
template <int A, int B, int C, int D>
static hipError_t launch_unpack_coop(const UnpackFieldPtrs& fp, const PackJob& j) {
    hipLaunchKernelGGL((unpack_coop_kernel<A, B, C, D>), dim3((unsigned)j.c.tn),
                       dim3(j.c.tile_rows), 0, j.s, j.c, fp);
    return hipGetLastError();
}

// One field through the cooperative kernel (hipErrorNotSupported: not its shape).
static hipError_t unpack_coop(const PackJob& j) {
    if (!coop_shape(j.c.nb, j.c.tile_rows)) return hipErrorNotSupported;
    const int u = coop_unit(j.src, j.row_bytes, j.dst, j.redirect);
    if (u < 0) return hipErrorNotSupported;
    UnpackFieldPtrs fp{};
    fp.packed[0] = (const uint8_t*)j.src;
    fp.red[0] = (const uint8_t*)j.redirect;
    fp.out[0] = (uint8_t*)j.dst;
#define MGR_UC1(W_, N_) case W_ * 32 + N_: return launch_unpack_coop<W_ * 32 + N_, 0, 0, 0>(fp, j);
    switch (u) {
        MGR_UC1(16, 1) MGR_UC1(16, 2) MGR_UC1(16, 3) MGR_UC1(16, 4)
        MGR_UC1(8, 1) MGR_UC1(8, 2) MGR_UC1(8, 3) MGR_UC1(8, 4)
        MGR_UC1(8, 5) MGR_UC1(8, 6) MGR_UC1(8, 7) MGR_UC1(8, 8)
        MGR_UC1(4, 1) MGR_UC1(4, 2) MGR_UC1(4, 3) MGR_UC1(4, 4)
        MGR_UC1(4, 5) MGR_UC1(4, 6) MGR_UC1(4, 7) MGR_UC1(4, 8)
        MGR_UC1(4, 9) MGR_UC1(4, 10) MGR_UC1(4, 11) MGR_UC1(4, 12)
        MGR_UC1(4, 13) MGR_UC1(4, 14) MGR_UC1(4, 15) MGR_UC1(4, 16)
        default: break;
    }
#undef MGR_UC1
    return hipErrorNotSupported;
}

// 2..4 fields of a signature pack_coop_fields takes, from one ranking
// (hipErrorNotSupported otherwise).  t: the tile context and stream (no array).
static hipError_t unpack_coop_fields(int nf, const void* const* packed, const int64_t* row_bytes,
                                     void* const* outs, const void* const* reds,
                                     const PackJob& t) {
    if (!coop_shape(t.c.nb, t.c.tile_rows)) return hipErrorNotSupported;
    int u[4] = {0, 0, 0, 0};
    UnpackFieldPtrs fp{};
    for (int f = 0; f < nf; ++f) {
        u[f] = coop_unit(packed[f], row_bytes[f], outs[f], reds ? reds[f] : nullptr);
        if (u[f] < 0) return hipErrorNotSupported;
        fp.packed[f] = (const uint8_t*)packed[f];
        fp.red[f] = reds ? (const uint8_t*)reds[f] : nullptr;
        fp.out[f] = (uint8_t*)outs[f];
    }
    auto sig = [&](int a, int b, int c, int d) { return u[0] == a && u[1] == b && u[2] == c && u[3] == d; };
    constexpr int F4x1 = 4 * 32 + 1, F4x3 = 4 * 32 + 3, F8x1 = 8 * 32 + 1, F8x3 = 8 * 32 + 3,
                  F16x2 = 16 * 32 + 2, F4x9 = 4 * 32 + 9, F16x1 = 16 * 32 + 1, F8x2 = 8 * 32 + 2;
    // the field sets of pack_coop_fields (mgr_pack_fields.hip)
    if (sig(F4x3, F4x3, F4x1, F8x1)) return launch_unpack_coop<F4x3, F4x3, F4x1, F8x1>(fp, t);
    if (sig(F8x3, F8x1, 0, 0)) return launch_unpack_coop<F8x3, F8x1, 0, 0>(fp, t);
    if (sig(F16x2, F8x3, 0, 0)) return launch_unpack_coop<F16x2, F8x3, 0, 0>(fp, t);
    if (sig(F4x9, F4x3, 0, 0)) return launch_unpack_coop<F4x9, F4x3, 0, 0>(fp, t);
    if (sig(F4x3, F8x1, 0, 0)) return launch_unpack_coop<F4x3, F8x1, 0, 0>(fp, t);
    if (sig(F16x1, F8x1, 0, 0)) return launch_unpack_coop<F16x1, F8x1, 0, 0>(fp, t);
    if (sig(F8x3, F8x3, F8x1, 0)) return launch_unpack_coop<F8x3, F8x3, F8x1, 0>(fp, t);
    if (sig(F4x3, F4x3, F8x1, 0)) return launch_unpack_coop<F4x3, F4x3, F8x1, 0>(fp, t);
    if (sig(F8x2, F8x1, 0, 0)) return launch_unpack_coop<F8x2, F8x1, 0, 0>(fp, t);
    return hipErrorNotSupported;
}

template <int W, typename DestT, bool kWide>
static hipError_t unpack_t(const PackJob& j) {
    auto k = unpack_kernel<W, DestT, kWide>;
    const int per_wave = align16(j.c.nb * 8) + align16(j.c.nb * 4);
    const int wpb = waves_per_block(per_wave);
    const int lds = per_wave * wpb;
    ensure_lds(k, lds);
    const int64_t grid = (j.c.tn + wpb - 1) / wpb;
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(64 * wpb), (size_t)lds, j.s, j.c,
                       (const uint8_t*)j.src, j.row_bytes / W, per_wave, (uint8_t*)j.dst,
                       (const uint8_t*)j.redirect);
    return hipGetLastError();
}

template <int W>
static hipError_t unpack_w(const PackJob& j) {
    const bool wide = j.row_bytes > 256;
    if (dest_bytes(j.c.nb) == 1)
        return wide ? unpack_t<W, uint8_t, true>(j) : unpack_t<W, uint8_t, false>(j);
    return wide ? unpack_t<W, uint16_t, true>(j) : unpack_t<W, uint16_t, false>(j);
}

// One field (j.redirect null without a redirect bin): the cooperative
// kernel where it takes the shape (hook unpack_kernel 1: never), else the
// generic one in the widest unit dividing the row and every base address.
static hipError_t unpack_rows(const PackJob& j) {
    if (j.h.unpack_kernel != 1) {
        const hipError_t e = unpack_coop(j);
        if (e != hipErrorNotSupported) return e;
    }
    switch (unit_log((uintptr_t)j.src | (uintptr_t)j.dst | (uintptr_t)j.row_bytes |
                     (uintptr_t)j.redirect)) {
        case 4: return unpack_w<16>(j);
        case 3: return unpack_w<8>(j);
        case 2: return unpack_w<4>(j);
        case 1: return unpack_w<2>(j);
        default: return unpack_w<1>(j);
    }
}

// mgr_unpack_fields: 2..4 fields of a cooperative signature move from one
// ranking in one launch (hook unpack_kernel 0 only); any other set goes
// field by field through the single-field kernels with the same dest.
hipError_t launch_unpack_fields(int nf, const void* const* packed, const int64_t* row_bytes,
                                int64_t n, const void* dest, int nbins, int drop_bin,
                                int tile_rows, const Workspace& ws, void* const* outs,
                                int redirect_bin, const void* const* reds, hipStream_t s) {
    if (n <= 0 || ws.tn <= 0) return hipSuccess;
    const Hooks& h = hooks();   // one snapshot for the whole launch
    if (redirect_bin < 0) reds = nullptr;
    const TileCtx c = tile_ctx(n, dest, nbins, drop_bin, tile_rows, ws, redirect_bin);
    prof_begin(s, K_UNPACK);
    hipError_t e = hipErrorNotSupported;
    if (nf >= 2 && nf <= 4 && h.unpack_kernel == 0)
        e = unpack_coop_fields(nf, packed, row_bytes, outs, reds,
                               PackJob{nullptr, 0, nullptr, nullptr, s, nullptr, h, c});
    if (e == hipErrorNotSupported) {
        e = hipSuccess;
        for (int f = 0; f < nf && e == hipSuccess; ++f)
            e = unpack_rows(PackJob{packed[f], row_bytes[f], outs[f],
                                    reds ? (void*)reds[f] : nullptr /* read only */, s,
                                    nullptr, h, c});
    }
    prof_end(s, K_UNPACK);
    return e;
}

// ------------------------------------------------------------------ ranked
// Inverse of pack_ranked_kernel (mgr_unpack_ranked_fields): the fine-cell sort
// places row r of tile t, bin b at
//     slot(r) = offsets[b * T + t] - tile_starts[t * nb + b] + ranks[r]
// (the pack's gaddr[b] + lpos * RB), so the way back needs no ranking, no
// ballots and no scan: one 256-thread workgroup per forward tile puts base[b]
// = offsets[b * T + t] - tile_starts[t * nb + b] into LDS as int64 (<= 8 KiB,
// one barrier), then wave w walks the 64-row rounds w, w + 4, ...: ids and
// ranks are loaded coalesced, once for every field, lane l's slot is base[id]
// + rank, and every field is moved unit-transposed as CoopGather does (lane l
// owns units 64 k + l of the round and takes its row's slot by shfl), so a
// store instruction writes 64 * W contiguous bytes of outs[f].  8 KiB of LDS
// and four waves: up to eight workgroups per CU.
//
// Fields: a set of <= 4 fields whose signatures (CoopGather's W * 32 + UPR)
// are template arguments moves with compile-time unit counts; any other set
// -- up to MGR_MAX_FIELDS fields, any row size -- moves in the same single
// launch from the run-time table RankedFields: per field the unit width
// (16/8/4/2/1 bytes), the units per row and, for rows of <= 64 units, the
// multiplier that replaces the division unit -> row; rows of more units go a
// row at a time, 64 lanes wide (unpack_kernel's kWide).
struct RankedFields {
    const uint8_t* src[MGR_MAX_FIELDS];
    uint8_t* out[MGR_MAX_FIELDS];
    int64_t upr[MGR_MAX_FIELDS];      // units per row
    uint32_t magic[MGR_MAX_FIELDS];   // ceil(2^20 / upr): u / upr == (u * magic) >> 20, u < 4096, upr <= 64
    uint8_t wlog[MGR_MAX_FIELDS];     // log2 of the unit's bytes
    int nf;
};

template <int W>
__device__ __forceinline__ void ranked_move(const uint8_t* __restrict__ src,
                                            uint8_t* __restrict__ out, int64_t upr64,
                                            uint32_t magic, long long slot, int64_t row0, int nr,
                                            int lane) {
    using U = typename Unit<W>::T;
    const U* __restrict__ s_u = (const U*)src;
    if (upr64 <= 64) {
        const int upr = (int)upr64, total = nr * upr;
        U* __restrict__ o_u = (U*)out + row0 * upr;
        for (int k0 = 0; 64 * k0 < total; k0 += 4) {
            U v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int u = 64 * (k0 + j) + lane;
                const int r = (int)(((uint32_t)u * magic) >> 20);
                const int part = u - r * upr;
                const long long t = __shfl(slot, r & 63, 64);
                v[j] = U{};
                if (u < total) v[j] = s_u[t * upr + part];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int u = 64 * (k0 + j) + lane;
                if (u < total) o_u[u] = v[j];
            }
        }
    } else {
        for (int j = 0; j < nr; ++j) {
            const long long t = __shfl(slot, j, 64);
            const U* sp = s_u + t * upr64;
            U* dp = (U*)out + (row0 + j) * upr64;
            for (int64_t k = lane; k < upr64; k += 64) dp[k] = sp[k];
        }
    }
}

// U0 < 0: the run-time field table; else CoopGather signatures (0: no field).
template <int U0, int U1, int U2, int U3>
__global__ __launch_bounds__(kBlock) void unpack_ranked_kernel(
    RankedFields fp, int64_t n, const uint16_t* __restrict__ ids,
    const uint16_t* __restrict__ ranks, const uint16_t* __restrict__ tile_starts, int nb,
    const int64_t* __restrict__ offsets, int64_t T, int tile_rows,
    const uint32_t* __restrict__ scan_err) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    long long* base = (long long*)smem;
    if (scan_failed(scan_err)) return;
    const int tid = threadIdx.x, w = tid >> 6, lane = lane_id();
    const int64_t tile = xcd_tile(blockIdx.x, T);
    for (int b = tid; b < nb; b += kBlock)
        base[b] = offsets[(int64_t)b * T + tile] - (long long)tile_starts[tile * nb + b];
    __syncthreads();
    const int64_t trow0 = tile * (int64_t)tile_rows;
    const int rows = (int)min((int64_t)tile_rows, n - trow0);
    for (int r0 = 64 * w; r0 < rows; r0 += 64 * kWaves) {
        const int nr = min(64, rows - r0);
        const int64_t row0 = trow0 + r0;
        long long slot = 0;
        if (lane < nr) {
            // ids >= nb: clamped as pack_ranked_kernel clamps them
            const unsigned b = min((unsigned)ids[row0 + lane], (unsigned)(nb - 1));
            const unsigned rk = ranks[row0 + lane];
            // inside [0, n) for the arrays mgr_rank_ids + mgr_scan left; held
            // there for any others, so that no read leaves the buffers
            slot = min(max(base[b] + (long long)rk, 0ll), (long long)n - 1);
        }
        if constexpr (U0 >= 0) {
            CoopGather<U0> f0;
            CoopGather<U1> f1;
            CoopGather<U2> f2;
            CoopGather<U3> f3;
            f0.load(fp.src[0], nullptr, slot, nr, lane);
            f1.load(fp.src[1], nullptr, slot, nr, lane);
            f2.load(fp.src[2], nullptr, slot, nr, lane);
            f3.load(fp.src[3], nullptr, slot, nr, lane);
            f0.store(fp.out[0], row0, nr, lane);
            f1.store(fp.out[1], row0, nr, lane);
            f2.store(fp.out[2], row0, nr, lane);
            f3.store(fp.out[3], row0, nr, lane);
        } else {
            for (int f = 0; f < fp.nf; ++f) {
                const uint8_t* __restrict__ src = fp.src[f];
                uint8_t* __restrict__ out = fp.out[f];
                const int64_t upr = fp.upr[f];
                const uint32_t mg = fp.magic[f];
                switch (fp.wlog[f]) {
                    case 4: ranked_move<16>(src, out, upr, mg, slot, row0, nr, lane); break;
                    case 3: ranked_move<8>(src, out, upr, mg, slot, row0, nr, lane); break;
                    case 2: ranked_move<4>(src, out, upr, mg, slot, row0, nr, lane); break;
                    case 1: ranked_move<2>(src, out, upr, mg, slot, row0, nr, lane); break;
                    default: ranked_move<1>(src, out, upr, mg, slot, row0, nr, lane); break;
                }
            }
        }
    }
}

// mgr_unpack_ranked_fields: ONE launch for every field set.  Templated
// signatures: one field of <= 16 units of 16/8/4 bytes, and the 2..4-field
// sets of pack_coop_fields (config 5's four arrays first); every other set
// takes the run-time table in the same launch -- nothing goes field by field.
hipError_t launch_unpack_ranked_fields(int nf, const void* const* sorted, const int64_t* row_bytes,
                                       int64_t n, const uint16_t* ids, const uint16_t* ranks,
                                       const uint16_t* tile_starts, int nbins, int tile_rows,
                                       const Workspace& ws, void* const* outs, hipStream_t s) {
    if (n <= 0 || ws.T <= 0) return hipSuccess;
    if (nf < 1 || nf > MGR_MAX_FIELDS || nbins < 1 || nbins > 1024 ||
        (tile_rows != 2048 && tile_rows != 4096))
        return hipErrorNotSupported;
    RankedFields fp{};
    fp.nf = nf;
    int u[4] = {0, 0, 0, 0};
    bool coop = nf <= 4;
    for (int f = 0; f < nf; ++f) {
        const int64_t rb = row_bytes[f];
        const int wl = unit_log((uintptr_t)sorted[f] | (uintptr_t)outs[f] | (uintptr_t)rb);
        fp.src[f] = (const uint8_t*)sorted[f];
        fp.out[f] = (uint8_t*)outs[f];
        fp.wlog[f] = (uint8_t)wl;
        fp.upr[f] = rb >> wl;
        fp.magic[f] = fp.upr[f] <= 64 ? (uint32_t)(((1u << 20) + fp.upr[f] - 1) / fp.upr[f]) : 0u;
        if (coop) {
            u[f] = coop_unit(sorted[f], rb, outs[f], nullptr);
            coop = u[f] >= 0;
        }
    }
    const int lds = align16(nbins * 8);
    prof_begin(s, K_UNPACK_RANKED);
    hipError_t e = hipErrorNotSupported;
#define MGR_URK(A, B, C, D)                                                                     \
    {                                                                                           \
        hipLaunchKernelGGL((unpack_ranked_kernel<A, B, C, D>), dim3((unsigned)ws.T),            \
                           dim3(kBlock), (size_t)lds, s, fp, n, ids, ranks, tile_starts, nbins, \
                           ws.offsets, ws.T, tile_rows, ws.scan_err);                           \
        e = hipGetLastError();                                                                  \
    }
    if (coop && hooks().unpack_kernel != 1) {
        auto sig = [&](int a, int b, int c, int d) { return u[0] == a && u[1] == b && u[2] == c && u[3] == d; };
        constexpr int F4x1 = 4 * 32 + 1, F4x3 = 4 * 32 + 3, F8x1 = 8 * 32 + 1, F8x3 = 8 * 32 + 3,
                      F16x2 = 16 * 32 + 2, F4x9 = 4 * 32 + 9, F16x1 = 16 * 32 + 1, F8x2 = 8 * 32 + 2;
        if (nf == 1) {
#define MGR_UR1(W_, N_) case W_ * 32 + N_: MGR_URK(W_ * 32 + N_, 0, 0, 0) break;
            switch (u[0]) {
                MGR_UR1(16, 1) MGR_UR1(16, 2) MGR_UR1(16, 3) MGR_UR1(16, 4)
                MGR_UR1(8, 1) MGR_UR1(8, 2) MGR_UR1(8, 3) MGR_UR1(8, 4)
                MGR_UR1(8, 5) MGR_UR1(8, 6) MGR_UR1(8, 7) MGR_UR1(8, 8)
                MGR_UR1(4, 1) MGR_UR1(4, 2) MGR_UR1(4, 3) MGR_UR1(4, 4)
                MGR_UR1(4, 5) MGR_UR1(4, 6) MGR_UR1(4, 7) MGR_UR1(4, 8)
                MGR_UR1(4, 9) MGR_UR1(4, 10) MGR_UR1(4, 11) MGR_UR1(4, 12)
                MGR_UR1(4, 13) MGR_UR1(4, 14) MGR_UR1(4, 15) MGR_UR1(4, 16)
                default: break;
            }
#undef MGR_UR1
        }
        else if (sig(F4x3, F4x3, F4x1, F8x1)) MGR_URK(F4x3, F4x3, F4x1, F8x1)
        else if (sig(F8x3, F8x1, 0, 0)) MGR_URK(F8x3, F8x1, 0, 0)
        else if (sig(F16x2, F8x3, 0, 0)) MGR_URK(F16x2, F8x3, 0, 0)
        else if (sig(F4x9, F4x3, 0, 0)) MGR_URK(F4x9, F4x3, 0, 0)
        else if (sig(F4x3, F8x1, 0, 0)) MGR_URK(F4x3, F8x1, 0, 0)
        else if (sig(F16x1, F8x1, 0, 0)) MGR_URK(F16x1, F8x1, 0, 0)
        else if (sig(F8x3, F8x3, F8x1, 0)) MGR_URK(F8x3, F8x3, F8x1, 0)
        else if (sig(F4x3, F4x3, F8x1, 0)) MGR_URK(F4x3, F4x3, F8x1, 0)
        else if (sig(F8x2, F8x1, 0, 0)) MGR_URK(F8x2, F8x1, 0, 0)
    }
    if (e == hipErrorNotSupported) MGR_URK(-1, 0, 0, 0)
#undef MGR_URK
    prof_end(s, K_UNPACK_RANKED);
    return e;
}

}  // namespace mgr
