// One-pass source partition (gfx950): what the record kernel (mgr_onepass.hip)
// and the SoA kernel (mgr_onepass_fields.hip) share -- the tile shape, the
// control words, the LDS layout (one function for the host's size and the
// kernels' pointers), every per-tile stage and the host dispatcher.
//
// A tile takes a ticket, stages its rows in LDS by LDS-DMA, bins them from the
// staged positions, writes the wrap back, ranks the rounds, publishes its count
// of every bin, finds the earlier tiles' counts by a decoupled look-back per
// bin (the one-pass scan's word format, mgr_device.h: status + poison + value
// in one 64-bit word, bounded polls), counts itself done and scatters a
// destination-ordered image.  Tiles take tickets in dispatch order, so a tile
// only ever waits on tiles that already run.
//
// Failure reporting (onepass_complete<true>, the SoA kernel; the record kernel
// runs without the counter, see there): every tile counts itself done ONCE, after it published
// its inclusive words, in one 64-bit word (finished tiles in bits 0-31, tiles
// whose look-back gave up in bits 32-63: one location, so the failures arrive
// with the count).  The tile that counts last is the only writer of
// bin_counts: every bin's total from the last tile's inclusive words, or -1
// for every bin when any tile gave up -- also a middle tile that later tiles
// looked past (they use its aggregate, which is valid, and place their rows
// behind rows that were never written).
#pragma once
#include "mgr_device.h"

namespace mgr {

constexpr int kOneWR = 128;   // rows per wave (two 64-row rounds)
constexpr int kOneNW = 8;     // waves per workgroup: 1024-row tiles
constexpr int kOneTile = kOneWR * kOneNW;

// Behind the [T][nbins] look-back words (onepass_workspace_bytes), zeroed with
// them before a launch.
struct OnePassCtl {
    uint32_t ticket;   // tiles in dispatch order
    uint32_t err;      // a look-back gave up
    uint64_t done;     // tiles that published their words (bits 0-31), failed ones (32-63)
};

static inline int64_t onepass_tiles(int64_t n) { return (n + kOneTile - 1) / kOneTile; }

// LDS of a tile, as byte offsets: per wave (`wave` bytes each) its staged rows
// -- `staged` bytes, a multiple of 512 -- the bins' output addresses, the
// inverse permutation and the slots' bins; then the tile's bases and counts of
// every bin and the waves' bin counts.  Sized by the bins, so 8-bin 36-byte
// rows take < 40 KiB and, with <= 64 VGPRs (amdgpu_waves_per_eu(8)), four
// workgroups fit a CU: a tile waiting on its look-back leaves three to keep
// memory busy (A/B, 64M config-5 rows: 1.19-1.20 ms against 1.39 with the
// 64-entry tables and three per CU; 512-row tiles, eight per CU: 1.60; a
// persistent grid taking tiles by ticket: 1.40, and 2.64 with the next
// ticket taken during the look-back -- the held tile delays its successors)
struct OneLayout {
    int gaddr, inv, ibin, wave;   // inside a wave's part
    int base, agg, cnt, total;    // from the start of the tile's LDS
};
__host__ __device__ inline OneLayout onepass_layout(int nw, int staged, int nb) {
    const int nbe = (nb + 1) & ~1;
    OneLayout l;
    l.gaddr = staged;
    l.inv = l.gaddr + 8 * nbe;
    l.ibin = l.inv + kOneWR;
    l.wave = l.ibin + kOneWR;
    l.base = nw * l.wave;
    l.agg = l.base + 8 * nbe;
    l.cnt = l.agg + 8 * nbe;
    l.total = l.cnt + 4 * nw * nb;
    return l;
}

static inline int onepass_lds_bytes(int nw, int staged_bytes_per_row, int nbins) {
    return onepass_layout(nw, kOneWR * staged_bytes_per_row, nbins).total;
}

struct OneLds {
    uint8_t* wl;                 // this wave's staged rows
    unsigned long long* gaddr;   // [nb] output address of every bin's image slot 0 (0: not written)
    uint8_t* inv;                // [WR] image slot -> row of the wave
    uint8_t* ibin;               // [WR] image slot -> bin
    long long* s_base;           // [nb] the earlier tiles' rows of every bin
    long long* s_agg;            // [nb] this tile's rows of every bin
    int* s_cnt;                  // [NW][nb] the waves' rows of every bin
};
template <int NW>
__device__ __forceinline__ OneLds onepass_carve(uint8_t* smem, int w, int staged, int nb) {
    const OneLayout l = onepass_layout(NW, staged, nb);
    uint8_t* wl = smem + w * l.wave;
    OneLds L;
    L.wl = wl;
    L.gaddr = (unsigned long long*)(wl + l.gaddr);
    L.inv = (uint8_t*)L.gaddr + (l.inv - l.gaddr);
    L.ibin = L.inv + (l.ibin - l.inv);
    L.s_base = (long long*)(smem + l.base);
    L.s_agg = (long long*)((uint8_t*)L.s_base + (l.agg - l.base));
    L.s_cnt = (int*)((uint8_t*)L.s_agg + (l.cnt - l.agg));
    return L;
}

// ---------------------------------------------------------- per-tile stages
// The tile's ticket (thread 0 takes it; the whole workgroup returns it).
__device__ __forceinline__ int64_t onepass_take_ticket(OnePassCtl* ctl, int* s_tile,
                                                       int* s_poison) {
    if (threadIdx.x == 0) {
        *s_tile = (int)__hip_atomic_fetch_add(&ctl->ticket, 1u, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
        *s_poison = 0;
    }
    __syncthreads();
    return *s_tile;
}

// Wave w's rows of the tile: its first row and how many of them exist.
template <int NW>
__device__ __forceinline__ int onepass_wave_rows(int64_t tile, int w, int64_t n, int64_t* row0) {
    *row0 = tile * (int64_t)(kOneWR * NW) + (int64_t)kOneWR * w;
    return __builtin_amdgcn_readfirstlane((int)max((int64_t)0, min((int64_t)kOneWR, n - *row0)));
}

// nbytes of one array from gp into the wave's LDS block lp (LDS-DMA:
// wave-uniform base + lane * 16; lanes past the rows masked off; the array's
// last unit reads up to 12 bytes past its end, inside the 16-byte-aligned
// unit's page, and lands inside the block).  Not waited for: a kernel puts
// all its arrays in flight, then onepass_staged().
__device__ __forceinline__ void onepass_stage(const uint8_t* gp, uint8_t* lp, int nbytes,
                                              int lane) {
    for (int i = 0; 1024 * i < nbytes; ++i) {
        const int x = 16 * (64 * i + lane);
        if (x < nbytes)
            __builtin_amdgcn_global_load_lds(
                (const void*)(gp + x), (__attribute__((address_space(3))) void*)(lp + 1024 * i), 16,
                0, 0);
    }
}
__device__ __forceinline__ void onepass_staged() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    wave_sync();
}

// Bin the wave's rows from the staged block pl that holds their positions
// (rows of prb bytes, positions at pos_off; the wrap is written into the
// copy, S1).  Returns whether this lane changed a position.
template <int RPW, typename PosT, bool kP, int SIDE, int GEO>
__device__ __forceinline__ bool onepass_bin(uint8_t* pl, int prb, int pos_off, int nrows, int lane,
                                            const Geom& g, const FineGeom& fg, unsigned (&b)[RPW],
                                            unsigned (&side)[RPW], bool (&valid)[RPW]) {
    bool dirty = false;
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        const int r = 64 * q + lane;
        valid[q] = r < nrows;
        b[q] = 0;
        side[q] = 0;
        if (valid[q]) {
            long long sc = 0;
            b[q] = (unsigned)bin_row<PosT, kP, 3, SIDE, GEO>((PosT*)(pl + r * prb + pos_off), g,
                                                             nullptr, &dirty, &fg, nullptr, &sc);
            side[q] = (unsigned)sc;
        }
    }
    wave_sync();
    return dirty;
}

// The caller's array holds the wrapped positions (redist.py:68 in place): the
// wave's staged block lp goes back to gp when one of its rows changed (or
// always, write_all).
template <bool kP>
__device__ __forceinline__ void onepass_write_back(uint8_t* gp, const uint8_t* lp, int nbytes,
                                                   bool dirty, int write_all, int lane) {
    if (kP && (write_all || __ballot(dirty) != 0ull)) {
        const int full = nbytes & ~15;
        for (int x = 16 * lane; x < full; x += 1024)
            *(u32x4_t*)(gp + x) = *(const u32x4_t*)(lp + x);
        for (int x = full + 4 * lane; x < nbytes; x += 256)
            *(uint32_t*)(gp + x) = *(const uint32_t*)(lp + x);
    }
}

// Rank inside each round; lane l counts bin l over the wave's rounds (the
// return value) and stores the count for the tile.
template <int RPW>
__device__ __forceinline__ int onepass_rank(const OneLds& L, int w, int nb, int nbits, int lane,
                                            const unsigned (&b)[RPW], const bool (&valid)[RPW],
                                            unsigned long long (&pe)[RPW], int (&cq)[RPW]) {
    int cnt = 0;
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        cq[q] = round_rank(b[q], valid[q], lane, nbits, &pe[q]);
        cnt += cq[q];
    }
    if (lane < nb) L.s_cnt[w * nb + lane] = cnt;
    return cnt;
}

// The tile's count of every bin, published at once (wave 0, lane b) so later
// tiles can look past this one before its prefix is known.  Workgroup-wide:
// waits for the waves' counts, and for the aggregate before it returns.
template <int NW>
__device__ __forceinline__ void onepass_publish(const OneLds& L, uint64_t* words, int64_t tile,
                                                int w, int nb, int lane) {
    __syncthreads();
    if (w == 0 && lane < nb) {
        long long agg = 0;
#pragma unroll
        for (int j = 0; j < NW; ++j) agg += L.s_cnt[j * nb + lane];
        L.s_agg[lane] = agg;
        flag_store(words + tile * nb + lane, (tile == 0 ? kScanInc : kScanAgg) | (uint64_t)agg);
    }
    __syncthreads();
}

// What a lane of wave 0 holds after the look-back: lanes with `mine` own bin bb.
struct OneLook {
    long long excl;    // the earlier tiles' rows of bin bb
    uint64_t poison;   // kScanPoison: the look-back gave up (or met a tile that had)
    int bb;
    bool mine;
};

// The earlier tiles' counts of every bin, by wave 0: lane k * nbp + b reads
// bin b's word of tile base - k (nbp = bins rounded up to a power of two, a
// window of 64 / nbp tiles per bin and round trip: 8 for 8 bins), summing up
// to the nearest inclusive prefix.  (A/B, round 6: one wave per bin reading 64
// tiles per round trip measured slower -- every look-back word is an
// agent-scope load past the XCD's L2 -- and one lane per bin polling one tile
// at a time too.)  Stores the tile's inclusive words, its bases (s_base) and,
// when it gave up, s_poison and the control word.
// Test hook (onepass_poison_tile): that tile treats its look-back as given up
// -- the bounded-poll error path, taken deterministically.
__device__ __forceinline__ OneLook onepass_look_back(const OneLds& L, uint64_t* words,
                                                     OnePassCtl* ctl, int64_t tile, int nb,
                                                     int lane, int spins, int poison_tile,
                                                     int* s_poison) {
    const int nbp = nb <= 1 ? 1 : 1 << (32 - __clz(nb - 1));
    const int win = 64 / nbp;
    const int bb = lane & (nbp - 1), k = lane / nbp;
    unsigned long long grp = 0;   // the lanes of one bin: bits bb, bb + nbp, ...
    for (int j = 0; j < win; ++j) grp |= 1ull << (j * nbp);
    grp <<= bb;
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
    if (mine) {
        if (tile > 0 || poison)
            flag_store(words + tile * nb + bb, kScanInc | poison | (uint64_t)(excl + L.s_agg[bb]));
        L.s_base[bb] = excl;
        if (poison) {
            *s_poison = 1;
            __hip_atomic_store(&ctl->err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    return OneLook{excl, poison, bb, mine};
}

// This tile is done with the words (wave 0).  DONE: counted once, with its
// failure (relaxed atomics on ONE location are seen in order, so the failures
// of every tile counted before arrive with the count); the last tile to be
// counted is the only writer of bin_counts.  !DONE: tile T - 1 writes
// bin_counts from its own prefix, -1 where that prefix is poisoned -- a middle
// tile that gave up after later tiles summed past its aggregate goes
// unreported.  The record kernel runs without the counter: with it the
// config-5 kernel measured 1.63 ms against 1.20 (profiles/round10/ab_notes.md;
// the counter shares its cache line with the ticket).
template <bool DONE>
__device__ __forceinline__ void onepass_complete(const OneLds& L, uint64_t* words, OnePassCtl* ctl,
                                                 const OneLook& lk, int64_t tile, int64_t T,
                                                 int nb, int lane, int spins,
                                                 int64_t* __restrict__ bin_counts) {
    if constexpr (!DONE) {
        if (lk.mine && tile == T - 1)
            bin_counts[lk.bb] = lk.poison ? -1 : lk.excl + L.s_agg[lk.bb];
        return;
    }
    const bool failed_here = __ballot(lk.mine && lk.poison) != 0ull;
    unsigned long long seen = 0;
    if (lane == 0)
        seen = __hip_atomic_fetch_add(&ctl->done, 1ull + (failed_here ? (1ull << 32) : 0ull),
                                      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    seen = readlane64(seen, 0);
    if ((int64_t)(seen & 0xFFFFFFFFull) == T - 1) {
        // The last tile's inclusive words were stored before it counted itself,
        // but relaxed atomics on two locations are not ordered for another
        // reader, so they are polled (bounded; one look in practice)
        bool bad = failed_here || (seen >> 32) != 0 ||
                   __hip_atomic_load(&ctl->err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
        long long total = 0;
        if (lk.mine) {
            if (tile == T - 1) {
                total = lk.excl + L.s_agg[lk.bb];
            } else {
                const uint64_t v =
                    flag_poll(words + (T - 1) * nb + lk.bb, 2, spins < 0 ? 0 : spins);
                total = (long long)(v & kScanVal);
                bad = bad || (v & kScanPoison) != 0;
            }
        }
        bad = __ballot(bad) != 0ull;
        if (lk.mine) bin_counts[lk.bb] = bad ? -1 : total;
    }
}

// Publish, look back, complete: false when this tile must write no rows (its
// look-back gave up or met a tile that had).
template <int NW, bool DONE>
__device__ __forceinline__ bool onepass_scan(const OneLds& L, uint64_t* words, OnePassCtl* ctl,
                                             int64_t tile, int64_t T, int w, int nb, int lane,
                                             int spins, int poison_tile, int* s_poison,
                                             int64_t* __restrict__ bin_counts) {
    onepass_publish<NW>(L, words, tile, w, nb, lane);
    if (w == 0) {
        const OneLook lk =
            onepass_look_back(L, words, ctl, tile, nb, lane, spins, poison_tile, s_poison);
        onepass_complete<DONE>(L, words, ctl, lk, tile, T, nb, lane, spins, bin_counts);
    }
    __syncthreads();
    return *s_poison == 0;
}

// Where the wave's rows go.  Every valid row gets its image slot (slot[q]; inv
// and ibin filled), its fine id stored beside its region row.  Lane b returns
// for bin b: ro, the region row (from row 0 of the output, b * cap included)
// of the bin's image slot 0, and fits -- a bin whose rows of this wave would
// reach cap writes none of them, for any field nor their fine ids (the caller
// sees count > cap and redoes the partition).
struct OnePlace {
    long long ro;
    bool fits;
};
template <int RPW, int SIDE>
__device__ __forceinline__ OnePlace onepass_place(const OneLds& L, int w, int nb, int lane, int cnt,
                                                  const unsigned (&b)[RPW],
                                                  const bool (&valid)[RPW],
                                                  const unsigned long long (&pe)[RPW],
                                                  const int (&cq)[RPW], const unsigned (&side)[RPW],
                                                  int64_t cap, uint16_t* __restrict__ fine_out,
                                                  int (&slot)[RPW]) {
    // this wave's rows of bin b start at the tile's base + the earlier waves' counts
    long long tbase = 0;
    if (lane < nb) {
        tbase = L.s_base[lane];
        for (int j = 0; j < w; ++j) tbase += L.s_cnt[j * nb + lane];
    }
    const int excl = wave_incl_dpp(cnt) - cnt;   // the bins' image starts (bin-major)
    int run = excl;
    const bool fits = tbase + cnt <= cap;
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        // (shuffles in uniform control flow)
        slot[q] = __shfl(run, (int)b[q], 64) + (valid[q] ? rank_in(pe[q]) : 0);
        const long long orow = __shfl(tbase - excl, (int)b[q], 64) + slot[q];   // row in the region
        const int fitb = __shfl((int)fits, (int)b[q], 64);
        run += cq[q];
        if (valid[q]) {
            L.inv[slot[q]] = (uint8_t)(64 * q + lane);
            L.ibin[slot[q]] = (uint8_t)b[q];
            if (SIDE == kSideFine && fitb)
                fine_out[(int64_t)b[q] * cap + orow] = (uint16_t)side[q];
        }
    }
    return OnePlace{(int64_t)lane * cap + tbase - excl, fits};
}

// One staged block's rows of a wave, gathered through the inverse permutation
// and streamed out in 16-byte units: any 4-byte-multiple row.
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

// ------------------------------------------------------------- host dispatch
// What both launchers hand over; the kernels take `head...` (their sources and
// outputs), then these, then the tile count and the hooks.
struct OneLaunch {
    const Geom& g;
    const FineGeom* fg;   // NULL: no fine ids
    int pos_dtype, periodic;
    int staged_row_bytes;   // LDS per row: the record, or all staged fields
    int64_t n;
    uint16_t* fine_out;
    int64_t cap;
    int64_t* bin_counts;
    uint64_t* words;   // the workspace
    int prof_id;
    hipStream_t s;
};

// One launch of Fam::kernel<PosT, kP, SIDE, GEO>() -- selected over the
// position dtype, periodic, fine ids or none, and the plan's geometry class --
// between the workspace's zeroing and the profiler marks.  One hook snapshot.
template <typename Fam, typename PosT, bool kP, int SIDE, typename... Head>
static hipError_t onepass_launch(const OneLaunch& L, Head... head) {
    const Hooks& h = hooks();   // one snapshot for the launch
    const Geom& g = L.g;
    auto k = Fam::template kernel<PosT, kP, SIDE, kGeoAny>();
    if constexpr (kP) {
        const int geo = h.bin_generic ? kGeoAny : geo_kind(g, sizeof(PosT) == 4);
        if (geo == kGeoF32) k = Fam::template kernel<PosT, kP, SIDE, kGeoF32>();
        else if (geo == kGeoF64) k = Fam::template kernel<PosT, kP, SIDE, kGeoF64>();
    }
    FineGeom f{};
    if (L.fg) f = *L.fg;
    const int64_t T = onepass_tiles(L.n);
    const int lds = onepass_lds_bytes(kOneNW, L.staged_row_bytes, g.nbins);
    ensure_lds(k, lds);
    hipLaunchKernelGGL(k, dim3((unsigned)T), dim3(64 * kOneNW), (size_t)lds, L.s, head..., L.n, g, f,
                       L.fine_out, L.cap, L.bin_counts, L.words, T, h.scan_spins,
                       g.write_back_all, h.onepass_poison_tile);
    return hipGetLastError();
}

template <typename Fam, typename PosT, typename... Head>
static hipError_t onepass_select(const OneLaunch& L, Head... head) {
    if (L.periodic)
        return L.fg ? onepass_launch<Fam, PosT, true, kSideFine>(L, head...)
                    : onepass_launch<Fam, PosT, true, kSideNone>(L, head...);
    return L.fg ? onepass_launch<Fam, PosT, false, kSideFine>(L, head...)
                : onepass_launch<Fam, PosT, false, kSideNone>(L, head...);
}

template <typename Fam, typename... Head>
static hipError_t onepass_dispatch(const OneLaunch& L, Head... head) {
    hipError_t e = hipMemsetAsync(L.words, 0, (size_t)onepass_workspace_bytes(L.n, L.g.nbins), L.s);
    if (e != hipSuccess) return e;
    prof_begin(L.s, L.prof_id);
    e = L.pos_dtype == MGR_F32 ? onepass_select<Fam, float>(L, head...)
                               : onepass_select<Fam, double>(L, head...);
    prof_end(L.s, L.prof_id);
    return e;
}

}  // namespace mgr
