// Multi-selection pack kernels (gfx950): the halo's sends, up to
// MGR_MSEL_MAX_FIELDS fields of the same rows to every selection set in one
// launch, with their launcher.  The way back: mgr_msel_unpack.hip.  Helpers:
// mgr_device.h.
#include "mgr_device.h"

namespace mgr {

// Multi-selection pack (the halo's sends, msel counts + mgr_scan with nbins
// = nsets), up to kSelFields fields of the same rows in one launch.  Set k's
// rows of field f go, in row order, to dsts[f][k] (null: set k is not
// written), so one launch places a set straight where it is consumed (a
// staging buffer for a neighbour, or the halo store itself when the
// neighbour is this rank).  One wave per tile, kSelChunk rows at a time: the
// chunk's flags are read once (chunk_flags); per set, the lanes' membership
// masks and a wave prefix list the set's rows in row order in LDS (u16 entry:
// chunk row | set << 10), the sets one after the other; then one copy loop
// per field moves every listed row -- 64 / upr rows per instruction, W-byte
// units (the widest the field's alignment allows), groups of kSelDepth
// instructions, two groups in flight -- to its set's next output row.  Rows
// wider than 64 units are copied one after the other, lanes across the row.
// The gathers read whole lines for sparse rows (PMC: 3.3 GB read for 1.3 GB
// of rows at the halo's density), so the kernel runs near the HBM rate of
// the lines it must touch (profiles/round4/ab_notes.md).
constexpr int kSelCap = 2048;   // LDS entries per wave (>= kSelChunk)
static_assert(kSelCap >= kSelChunk, "a set of one chunk must fit an empty list");
constexpr int kSelDepth = 4;    // copy instructions per group (round 3: 8 in flight, 1.17 vs 1.10 ms)
constexpr int kSelFields = 3;
struct SelFields {
    const uint8_t* src[kSelFields];
    int64_t row_bytes[kSelFields];
    int wlog[kSelFields];                 // log2 of the copy unit
    uint8_t* dst[kSelFields][kMaxSets];
};

// Lanes without a row (past the list's end, or past cap) store to a per-wave
// slot of this buffer, so every copy group issues exactly kSelDepth loads and
// kSelDepth stores: the counts s_waitcnt works with stay static.
__device__ uint4 g_sel_trash[256][64];

template <int W>
__device__ __forceinline__ void sel_copy(const uint8_t* __restrict__ src, int64_t row_bytes,
                                         uint8_t* const* dst, const long long* at,
                                         const int* start, const uint16_t* list, int fill,
                                         int lane, long long cap, uint8_t* trash) {
    // global address space throughout: pointers read from LDS or by readlane
    // are generic to the compiler, and a flat access counts on lgkmcnt too, so
    // every LDS read of the list waited for all copies in flight
    using U = __attribute__((address_space(1))) typename Unit<W>::T;
    const int64_t upr = row_bytes / W;
    const U* sp = (const U*)src;
    if (upr <= 64) {
        const int per = 64 / (int)upr;   // rows per copy instruction
        const int lr = lane / (int)upr;
        const int u = lane - lr * (int)upr;
        const int step = kSelDepth * per;
        const int ng = (fill + step - 1) / step;
        // group g: kSelDepth loads into v, targets into o (entry 0 of the
        // list, a row of this chunk, stands in for a lane without a row)
        auto load = [&](int g, typename Unit<W>::T (&v)[kSelDepth], U* (&o)[kSelDepth]) {
#pragma unroll
            for (int q = 0; q < kSelDepth; ++q) {
                const int i = g * step + q * per + lr;
                const bool ok = lr < per && i < fill;
                const unsigned e = list[ok ? i : 0];
                const int k = (int)(e >> 10);
                const long long row = at[k] + (i - start[k]);
                o[q] = ok && row < cap ? (U*)dst[k] + row * upr + u : (U*)trash;
                v[q] = sp[(int64_t)(e & 1023u) * upr + u];
            }
        };
        auto store = [&](const typename Unit<W>::T (&v)[kSelDepth], U* const (&o)[kSelDepth]) {
#pragma unroll
            for (int q = 0; q < kSelDepth; ++q) *o[q] = v[q];
        };
        // two groups in flight: group g+1's loads are issued before group g's
        // stores, so waiting for a group's loads never waits for the stores
        // before it (one vmcnt counts loads and stores, retired in order)
        typename Unit<W>::T va[kSelDepth], vb[kSelDepth];
        U* oa[kSelDepth];
        U* ob[kSelDepth];
        load(0, va, oa);
        for (int g = 0;; g += 2) {
            load(g + 1, vb, ob);
            store(va, oa);
            if (g + 1 >= ng) break;
            load(g + 2, va, oa);
            store(vb, ob);
            if (g + 2 >= ng) break;
        }
    } else {
        for (int i = 0; i < fill; ++i) {
            const unsigned e = list[i];
            const int k = (int)(e >> 10);
            const long long row = at[k] + (i - start[k]);
            if (row >= cap) continue;
            const U* rs = sp + (int64_t)(e & 1023u) * upr;
            U* rd = (U*)dst[k] + row * upr;
            for (int64_t q = lane; q < upr; q += 64) rd[q] = rs[q];
        }
    }
}

template <int NB>
__global__ __launch_bounds__(256) void msel_pack_kernel(
    SelFields fs, int nf, int64_t n, const uint16_t* __restrict__ flags, int nsets, SetMasks masks,
    const int64_t* __restrict__ offsets, const int64_t* __restrict__ set_starts, int64_t T,
    int tile_rows, long long cap, const uint32_t* __restrict__ scan_err) {
    __shared__ uint16_t list_s[4][kSelCap];
    __shared__ uint8_t* dst_s[4][kSelFields][kMaxSets];
    __shared__ long long at_s[4][kMaxSets];    // next output row of every set
    __shared__ int start_s[4][kMaxSets], cnt_s[4][kMaxSets];
    const int w = threadIdx.x >> 6, lane = lane_id();
    const int64_t tile = (int64_t)blockIdx.x * 4 + w;
    if (tile >= T || scan_failed(scan_err)) return;
    const int64_t row0 = tile * (int64_t)tile_rows;
    const int rows = (int)min((int64_t)tile_rows, n - row0);
    uint8_t* trash = (uint8_t*)&g_sel_trash[tile & 255][lane];
    uint16_t* list = list_s[w];
    long long* at = at_s[w];
    int* start = start_s[w];
    int* cnt = cnt_s[w];
    uint32_t live = 0;   // sets with a destination (in field 0: all fields alike)
#pragma unroll
    for (int k = 0; k < kMaxSets; ++k) {
        if (k >= nsets) break;
        if (fs.dst[0][k]) live |= 1u << k;
        if (lane == k) {
#pragma unroll
            for (int f = 0; f < kSelFields; ++f) dst_s[w][f][k] = fs.dst[f][k];
            // set_starts == nullptr: the sets back to back from dst (placed on the device)
            at[k] = offsets[(int64_t)k * T + tile] - (set_starts ? set_starts[k] : 0);
            cnt[k] = 0;
        }
    }
    wave_sync();
    const int nbits = mask_bits(masks, nsets);
    // Per-lane copies of what the loops index at run time (lane k: set k's
    // mask; lane f: field f's source, row bytes, unit width), read by
    // readlane: a kernel-argument array indexed at run time is a memory load
    // whose s_waitcnt vmcnt(0) drained every copy and prefetch in flight --
    // once per set and per field of every chunk.
    const unsigned lmask = lane < nsets ? (unsigned)masks.m[lane] : 0u;
    const unsigned long long lsrc = lane < nf ? (unsigned long long)fs.src[lane] : 0ull;
    const long long lrb = lane < nf ? fs.row_bytes[lane] : 0;
    const int lwl = lane < nf ? fs.wlog[lane] : 0;
    uint32_t fn[kSelWords];   // the next chunk's flags, loaded a chunk ahead
    chunk_flags(flags, row0, min(kSelChunk, rows), lane, fn);
    for (int c0 = 0; c0 < rows; c0 += kSelChunk) {
        uint32_t fw[kSelWords];
#pragma unroll
        for (int i = 0; i < kSelWords; ++i) fw[i] = fn[i];
        if (c0 + kSelChunk < rows)
            chunk_flags(flags, row0 + c0 + kSelChunk, min(kSelChunk, rows - c0 - kSelChunk), lane, fn);
        FlagPlanes fp;
        flag_planes_t<NB>(fw, nbits, fp);
        auto flush = [&](int fill) {
            wave_sync();
            for (int f = 0; f < nf; ++f) {
                const long long rb = readlane64(lrb, f);
                const uint8_t* sp = (const uint8_t*)readlane64(lsrc, f) + (row0 + c0) * rb;
                uint8_t* const* d = dst_s[w][f];
                switch (__builtin_amdgcn_readlane(lwl, f)) {
                    case 4: sel_copy<16>(sp, rb, d, at, start, list, fill, lane, cap, trash); break;
                    case 3: sel_copy<8>(sp, rb, d, at, start, list, fill, lane, cap, trash); break;
                    case 2: sel_copy<4>(sp, rb, d, at, start, list, fill, lane, cap, trash); break;
                    case 1: sel_copy<2>(sp, rb, d, at, start, list, fill, lane, cap, trash); break;
                    default: sel_copy<1>(sp, rb, d, at, start, list, fill, lane, cap, trash); break;
                }
            }
            wave_sync();
            if (lane < nsets) {
                at[lane] += cnt[lane];
                cnt[lane] = 0;
            }
            wave_sync();
        };
        // the sets' lists, flushed when the next set does not fit: ONE call
        // site of flush (its copy loops are most of the kernel's code; inlined
        // at two or three sites the kernel ran 2x slower)
        int k = 0;
        for (;;) {
            int fill = 0;
            bool full = false;
            for (; k < nsets; ++k) {
                if (!((live >> k) & 1u)) continue;
                uint32_t m = set_mask_t<NB>(fp, (unsigned)__builtin_amdgcn_readlane((int)lmask, k), nbits);
                if (!__ballot(m != 0u)) continue;   // an empty set costs no prefix
                int total;
                // bit-sliced ballot prefix (A/B: 1.122 vs 1.162 ms with the
                // __shfl_up scan)
                int pos = wave_excl_small<5>(__popc(m), &total);   // popc(m) <= 16
                if (!total) continue;
                if (fill + total > kSelCap) {   // (fill > 0: a set is <= kSelChunk rows)
                    full = true;
                    break;                       // set k again after the flush
                }
                if (lane == 0) {
                    start[k] = fill;
                    cnt[k] = total;
                }
                pos += fill;
                while (m) {
                    const int j = __builtin_ctz(m);
                    m &= m - 1u;
                    list[pos++] = (uint16_t)((16 * lane + j) | (k << 10));
                }
                fill += total;
            }
            if (fill) flush(fill);
            if (!full) break;
        }
    }
}

// The multi-selection pack for 4..kWideFields fields (a SoA payload's halo:
// up to MGR_MAX_FIELDS arrays, the positions, the face flags): the shape of
// msel_pack_kernel -- one wave per tile, kSelChunk-row chunks, the chunk's
// flags read and its per-set row lists built ONCE, then one sel_copy per
// field from those lists, the unit width chosen per field -- with the one
// thing that does not scale changed: the destination table.  dst[18][32] is
// 4.6 KB, more than a launch's kernel arguments hold, and per-wave LDS copies
// of it would be 18 KB.  So the arguments carry a flat table of kWideDsts
// pointers (entry f * nsets + k; placed mode: entry f, every set of field f
// from the same base), the workgroup stages it ONCE into one LDS table shared
// by its four waves (entry f * nsets + k in both modes, so sel_copy indexes
// it by set as it does in msel_pack_kernel), and the launcher packs the
// fields in groups when nfields * nsets exceeds kWideDsts.  Which sets are
// written (field 0's null destinations) is resolved on the host into `live`,
// so every group of a split pack lists the same sets.  The workgroup barrier
// behind the staging comes before any wave returns.  (The chunk loop repeats
// msel_pack_kernel's instead of sharing it: that kernel's code is tuned and
// measured as it stands, profiles/round4/ab_notes.md.)
constexpr int kWideFields = MGR_MSEL_MAX_FIELDS;
constexpr int kWideDsts = 384;   // destination pointers per launch (3 KB of arguments)
static_assert(kWideFields <= 64, "per-field values live in lanes");
static_assert(kWideDsts >= kMaxSets && kWideDsts >= kWideFields, "one field / placed mode must fit");
struct WideSel {
    const uint8_t* src[kWideFields];
    int64_t row_bytes[kWideFields];
    int wlog[kWideFields];                // log2 of the copy unit
    int nf, nsets, placed;
    uint32_t live;                        // sets that are written
    SetMasks masks;
    uint8_t* dst[kWideDsts];
};
// HIP passes at most 4 KB of kernel arguments; the kernel's scalars take < 128 B
static_assert(sizeof(WideSel) <= 4096 - 128, "msel_pack_wide_kernel's arguments exceed 4 KB");

template <int NB>
__global__ __launch_bounds__(256) void msel_pack_wide_kernel(
    WideSel fs, int64_t n, const uint16_t* __restrict__ flags,
    const int64_t* __restrict__ offsets, const int64_t* __restrict__ set_starts, int64_t T,
    int tile_rows, long long cap, const uint32_t* __restrict__ scan_err) {
    __shared__ uint16_t list_s[4][kSelCap];
    __shared__ uint8_t* dst_s[kWideFields * kMaxSets];   // [field][set], nsets per field
    __shared__ long long at_s[4][kMaxSets];    // next output row of every set
    __shared__ int start_s[4][kMaxSets], cnt_s[4][kMaxSets];
    const int nf = fs.nf, nsets = fs.nsets;
    // (host: nf <= kWideFields, nsets <= kMaxSets, nf * nsets <= kWideDsts unless placed)
    for (int i = threadIdx.x; i < nf * nsets; i += 256) dst_s[i] = fs.dst[fs.placed ? i / nsets : i];
    __syncthreads();
    const int w = threadIdx.x >> 6, lane = lane_id();
    const int64_t tile = (int64_t)blockIdx.x * 4 + w;
    if (tile >= T || scan_failed(scan_err)) return;
    const int64_t row0 = tile * (int64_t)tile_rows;
    const int rows = (int)min((int64_t)tile_rows, n - row0);
    uint8_t* trash = (uint8_t*)&g_sel_trash[tile & 255][lane];
    uint16_t* list = list_s[w];
    long long* at = at_s[w];
    int* start = start_s[w];
    int* cnt = cnt_s[w];
    const uint32_t live = fs.live;
    if (lane < nsets) {
        // set_starts == nullptr: the sets back to back from dst (placed on the device)
        at[lane] = offsets[(int64_t)lane * T + tile] - (set_starts ? set_starts[lane] : 0);
        cnt[lane] = 0;
    }
    wave_sync();
    const int nbits = mask_bits(fs.masks, nsets);
    // per-lane copies of what the loops index at run time, read by readlane
    // (msel_pack_kernel: an indexed kernel argument is a load whose wait
    // drains every copy in flight)
    const unsigned lmask = lane < nsets ? (unsigned)fs.masks.m[lane] : 0u;
    const unsigned long long lsrc = lane < nf ? (unsigned long long)fs.src[lane] : 0ull;
    const long long lrb = lane < nf ? fs.row_bytes[lane] : 0;
    const int lwl = lane < nf ? fs.wlog[lane] : 0;
    uint32_t fn[kSelWords];   // the next chunk's flags, loaded a chunk ahead
    chunk_flags(flags, row0, min(kSelChunk, rows), lane, fn);
    for (int c0 = 0; c0 < rows; c0 += kSelChunk) {
        uint32_t fw[kSelWords];
#pragma unroll
        for (int i = 0; i < kSelWords; ++i) fw[i] = fn[i];
        if (c0 + kSelChunk < rows)
            chunk_flags(flags, row0 + c0 + kSelChunk, min(kSelChunk, rows - c0 - kSelChunk), lane, fn);
        FlagPlanes fp;
        flag_planes_t<NB>(fw, nbits, fp);
        auto flush = [&](int fill) {
            wave_sync();
            for (int f = 0; f < nf; ++f) {
                const long long rb = readlane64(lrb, f);
                const uint8_t* sp = (const uint8_t*)readlane64(lsrc, f) + (row0 + c0) * rb;
                uint8_t* const* d = dst_s + f * nsets;
                switch (__builtin_amdgcn_readlane(lwl, f)) {
                    case 4: sel_copy<16>(sp, rb, d, at, start, list, fill, lane, cap, trash); break;
                    case 3: sel_copy<8>(sp, rb, d, at, start, list, fill, lane, cap, trash); break;
                    case 2: sel_copy<4>(sp, rb, d, at, start, list, fill, lane, cap, trash); break;
                    case 1: sel_copy<2>(sp, rb, d, at, start, list, fill, lane, cap, trash); break;
                    default: sel_copy<1>(sp, rb, d, at, start, list, fill, lane, cap, trash); break;
                }
            }
            wave_sync();
            if (lane < nsets) {
                at[lane] += cnt[lane];
                cnt[lane] = 0;
            }
            wave_sync();
        };
        // the sets' lists, flushed when the next set does not fit (one call
        // site of flush, as in msel_pack_kernel)
        int k = 0;
        for (;;) {
            int fill = 0;
            bool full = false;
            for (; k < nsets; ++k) {
                if (!((live >> k) & 1u)) continue;
                uint32_t m = set_mask_t<NB>(fp, (unsigned)__builtin_amdgcn_readlane((int)lmask, k), nbits);
                if (!__ballot(m != 0u)) continue;   // an empty set costs no prefix
                int total;
                int pos = wave_excl_small<5>(__popc(m), &total);   // popc(m) <= 16
                if (!total) continue;
                if (fill + total > kSelCap) {   // (fill > 0: a set is <= kSelChunk rows)
                    full = true;
                    break;                       // set k again after the flush
                }
                if (lane == 0) {
                    start[k] = fill;
                    cnt[k] = total;
                }
                pos += fill;
                while (m) {
                    const int j = __builtin_ctz(m);
                    m &= m - 1u;
                    list[pos++] = (uint16_t)((16 * lane + j) | (k << 10));
                }
                fill += total;
            }
            if (fill) flush(fill);
            if (!full) break;
        }
    }
}

static hipError_t launch_msel_pack_wide(int nfields, const void* const* srcs,
                                        const int64_t* row_bytes, int64_t n,
                                        const uint16_t* flags, int nsets, const int* masks,
                                        int tile_rows, const Workspace& ws, void* const* dsts,
                                        hipStream_t s, int64_t cap_rows) {
    const bool placed = cap_rows >= 0;
    WideSel fs{};
    unsigned u = 0;
    for (int k = 0; k < nsets; ++k) {
        fs.masks.m[k] = (uint16_t)masks[k];
        u |= (unsigned)fs.masks.m[k];
        // a set is written in every field or in none (field 0 decides)
        if (placed || dsts[0 * nsets + k]) fs.live |= 1u << k;
    }
    if (!fs.live) return hipSuccess;
    fs.nsets = nsets;
    fs.placed = placed;
    const int nb = flag_bits_class(u ? 32 - __builtin_clz(u) : 0);
    auto kern = nb == 2 ? msel_pack_wide_kernel<2> : nb == 4 ? msel_pack_wide_kernel<4>
              : nb == 6 ? msel_pack_wide_kernel<6> : nb == 8 ? msel_pack_wide_kernel<8>
                        : msel_pack_wide_kernel<0>;
    // the fields in equal groups whose destination tables fit a launch
    const int fit = placed ? kWideFields : kWideDsts / nsets;
    const int groups = (nfields + fit - 1) / fit, per = (nfields + groups - 1) / groups;
    const dim3 grid((unsigned)((ws.T + 3) / 4));
    for (int f0 = 0; f0 < nfields; f0 += per) {
        fs.nf = min(per, nfields - f0);
        for (int i = 0; i < fs.nf; ++i) {
            const int f = f0 + i;
            fs.src[i] = (const uint8_t*)srcs[f];
            fs.row_bytes[i] = row_bytes[f];
            uintptr_t a = (uintptr_t)srcs[f] | (uintptr_t)row_bytes[f];
            if (placed) {
                fs.dst[i] = (uint8_t*)dsts[f];
                a |= (uintptr_t)dsts[f];
            } else {
                for (int k = 0; k < nsets; ++k) {
                    uint8_t* d = (fs.live >> k) & 1u ? (uint8_t*)dsts[f * nsets + k] : nullptr;
                    fs.dst[i * nsets + k] = d;
                    a |= (uintptr_t)d;
                }
            }
            fs.wlog[i] = unit_log(a);
        }
        prof_begin(s, K_HALO_PACK);
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, fs, n, flags, ws.offsets,
                           placed ? nullptr : ws.bin_starts, ws.T, tile_rows,
                           placed ? (long long)cap_rows : (long long)INT64_MAX, ws.scan_err);
        prof_end(s, K_HALO_PACK);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_msel_pack(int nfields, const void* const* srcs, const int64_t* row_bytes,
                            int64_t n, const uint16_t* flags, int nsets, const int* masks,
                            int tile_rows, const Workspace& ws, void* const* dsts, hipStream_t s,
                            int64_t cap_rows) {
    if (n <= 0) return hipSuccess;
    if (nfields < 1 || nfields > kWideFields || nsets < 1 || nsets > kMaxSets)
        return hipErrorInvalidValue;
    // up to kSelFields fields: msel_pack_kernel, as ever (hook msel_wide: the
    // wide kernel on those too, for parity tests and A/B timing)
    if (nfields > kSelFields || hooks().msel_wide)
        return launch_msel_pack_wide(nfields, srcs, row_bytes, n, flags, nsets, masks, tile_rows,
                                     ws, dsts, s, cap_rows);
    SetMasks sb{};
    for (int k = 0; k < nsets; ++k) sb.m[k] = (uint16_t)masks[k];
    SelFields fs{};
    for (int f = 0; f < nfields; ++f) {
        fs.src[f] = (const uint8_t*)srcs[f];
        fs.row_bytes[f] = row_bytes[f];
        uintptr_t a = (uintptr_t)srcs[f] | (uintptr_t)row_bytes[f];
        for (int k = 0; k < nsets; ++k) {
            // a set is written in every field or in none (field 0 decides);
            // placed mode (cap_rows >= 0): every set of field f from dsts[f]
            fs.dst[f][k] = cap_rows >= 0 ? (uint8_t*)dsts[f]
                           : dsts[0 * nsets + k] ? (uint8_t*)dsts[f * nsets + k] : nullptr;
            a |= (uintptr_t)fs.dst[f][k];
        }
        fs.wlog[f] = unit_log(a);
    }
    unsigned u = 0;
    for (int k = 0; k < nsets; ++k) u |= (unsigned)sb.m[k];
    const int nb = flag_bits_class(u ? 32 - __builtin_clz(u) : 0);
    auto kern = nb == 2 ? msel_pack_kernel<2> : nb == 4 ? msel_pack_kernel<4>
              : nb == 6 ? msel_pack_kernel<6> : nb == 8 ? msel_pack_kernel<8>
                        : msel_pack_kernel<0>;
    const dim3 grid((unsigned)((ws.T + 3) / 4));
    prof_begin(s, K_HALO_PACK);
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, fs, nfields, n, flags, nsets, sb,
                       ws.offsets, cap_rows >= 0 ? nullptr : ws.bin_starts, ws.T, tile_rows,
                       cap_rows >= 0 ? (long long)cap_rows : (long long)INT64_MAX, ws.scan_err);
    prof_end(s, K_HALO_PACK);
    return hipGetLastError();
}

}  // namespace mgr
