// rj_partition.hip — gfx950 (wave64) kernels of the radix partition: K3 the bin scans, the tuple loaders, K2 the pass
// histograms, K4 the pass scatters, and the heavy task list.  Every node kind that partitions its input uses them:
// the five join node kinds (INNER, SEMI, ANTI, OUTER, FULL) and RJ_NODE_AGG.
#include <hip/hip_ext.h>

#include "rj_kernels.hpp"
#include "rj_kernel_util.hpp"
#include "rj_tuple_util.hpp"

#include <algorithm>
#include <type_traits>

namespace rj {

// ==================================================================== K3 scan
// Single workgroup of 1024 threads; thread t owns a contiguous chunk.
// MODE 0: v[i] = in[i].  MODE 1: v[i] = ceil((in[i+1]-in[i]) / div)  (group table)
// (in_end, MODE 1 only: segment i ends at in_end[i] instead of in[i + 1])
template <int MODE>
__global__ __launch_bounds__(1024) void k_scan_bins(const uint32_t* in, const uint32_t* in_end, uint32_t n,
                                                    uint32_t div, uint32_t* off, uint32_t* cursor) {
    __shared__ uint32_t s_wsum[16];
    const uint32_t      chunk = (n + 1023u) / 1024u;
    const uint32_t      b = threadIdx.x * chunk;
    const uint32_t      e = min(n, b + chunk);
    uint32_t            sum = 0;
    for (uint32_t i = b; i < e; ++i) {
        uint32_t v = MODE == 0 ? in[i] : ((in_end ? in_end[i] : in[i + 1]) - in[i] + div - 1u) / div;
        sum += v;
    }
    uint32_t total;
    uint32_t run = block_excl_scan(sum, s_wsum, total);
    for (uint32_t i = b; i < e; ++i) {
        uint32_t v = MODE == 0 ? in[i] : ((in_end ? in_end[i] : in[i + 1]) - in[i] + div - 1u) / div;
        off[i] = run;
        if (cursor) cursor[i] = run;
        run += v;
    }
    if (threadIdx.x == 0) off[n] = total;
}

// Exclusive scan of the bins of ONE input segment per workgroup.  A segment's tuples are
// exactly the sum of its bins (NULL keys were dropped in the first pass), so the global
// offset of bin (seg, d) is seg_off[seg] + prefix inside the segment: every segment scans
// independently instead of one workgroup walking all nseg*F bins.
__global__ __launch_bounds__(PT_MAXF) void k_scan_segments(const uint32_t* hist,
                                                           const uint32_t* seg_off, uint32_t nseg,
                                                           uint32_t F, uint32_t xcd_log2, uint32_t* off,
                                                           uint32_t* cursor) {
    __shared__ uint32_t s_wsum[PT_MAXF / 64];
    const uint32_t      seg = blockIdx.x, d = threadIdx.x, X = 1u << xcd_log2;
    // a partition's sub-ranges (one per XCD, see PassParams::xcd_log2) lie one behind the other
    const size_t        b0 = ((size_t)seg * F + d) << xcd_log2;
    uint32_t            v = 0;
    if (d < F)
        for (uint32_t x = 0; x < X; ++x) v += hist[b0 + x];
    uint32_t            total;
    const uint32_t      ex = block_excl_scan(v, s_wsum, total);
    const uint32_t      base = seg_off ? seg_off[seg] : 0u;
    if (d < F) {
        off[(size_t)seg * F + d] = base + ex;
        uint32_t at = base + ex;
        for (uint32_t x = 0; x < X; ++x) {
            cursor[b0 + x] = at;
            at += hist[b0 + x];
        }
    }
    if (seg + 1 == nseg && d == 0) off[(size_t)nseg * F] = base + total;
}

// ========================================================== tuple loaders (K2/K4)
// Loader concept:  key(i, hk) -> valid      load<NW>(i, w) -> valid
// A loader fills one tile: item j of thread t is element base + j*PT_THREADS + t.  Every
// load is UNCONDITIONAL (the index is clamped to the last valid element) and all uniform
// decisions (column kind, validity array present, carry mode) are taken once per tile, so
// the compiler can issue the whole tile's loads back to back behind a single wait.  The
// returned bit mask says which items hold a tuple.
// PAIR >= 0: in.w[PAIR] is an array of 8-byte {word PAIR, word PAIR+1} pairs (a two-word carry)
// (issue_tile / finish_tile: the two halves of load_tile for the scatter's software pipeline —
// issue only ISSUES the tile's loads, finish does what needs the data.  Loaders of tuples that are
// already in the partition layout have nothing to finish.)
#define RJ_TRIVIAL_ISSUE_FINISH                                                                              \
    template <int NW>                                                                                        \
    __device__ __forceinline__ uint32_t issue_tile(uint32_t base, uint32_t end, uint32_t (&w)[PT_ITEMS][NW]) const { \
        return this->template load_tile<NW>(base, end, w);                                                   \
    }                                                                                                        \
    template <int NW>                                                                                        \
    __device__ __forceinline__ uint32_t finish_tile(uint32_t, uint32_t, uint32_t ok, uint32_t (&)[PT_ITEMS][NW]) const { \
        return ok;                                                                                           \
    }

template <int PAIR>
struct DenseLoaderT {
    static constexpr int pair = PAIR;
    Words in;
    RJ_TRIVIAL_ISSUE_FINISH
    // two-halves interface of the fine histogram (see SrcLoader): the words are hashed already
    __device__ __forceinline__ uint32_t issue_keys(uint32_t base, uint32_t end, uint32_t (&lo)[PT_ITEMS],
                                                   uint32_t (&)[PT_ITEMS]) const {
        return key_tile(base, end, lo);
    }
    __device__ __forceinline__ uint32_t finish_keys(uint32_t, uint32_t, uint32_t ok, uint32_t (&)[PT_ITEMS],
                                                    uint32_t (&)[PT_ITEMS]) const {
        return ok;
    }
    __device__ __forceinline__ uint32_t key_tile(uint32_t base, uint32_t end,
                                                 uint32_t (&hk)[PT_ITEMS]) const {
        if (base + PT_TILE <= end) {  // full tile: four consecutive tuples per 16-byte load
#pragma unroll
            for (int v = 0; v < PT_ITEMS / 4; ++v) {
                u32x4a x = *reinterpret_cast<const u32x4a*>(in.w[0] + base +
                                                            (v * PT_THREADS + threadIdx.x) * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) hk[4 * v + e] = x[e];
            }
            return PT_ALL_ITEMS;
        }
        uint32_t ok = 0;
#pragma unroll
        for (int j = 0; j < PT_ITEMS; ++j) {
            uint32_t i = base + j * PT_THREADS + threadIdx.x;
            hk[j] = in.w[0][min(i, end - 1u)];
            ok |= (uint32_t)(i < end) << j;
        }
        return ok;
    }
    template <int NW>
    __device__ __forceinline__ uint32_t load_tile(uint32_t base, uint32_t end,
                                                  uint32_t (&w)[PT_ITEMS][NW]) const {
        if (base + PT_TILE <= end) {
#pragma unroll
            for (int v = 0; v < PT_ITEMS / 4; ++v) {
                const uint32_t i0 = base + (v * PT_THREADS + threadIdx.x) * 4;
#pragma unroll
                for (int a = 0; a < NW; ++a) {
                    if (a == pair) {  // four consecutive pairs = two 16-byte loads
                        const uint32_t* pp2 = in.w[a] + (size_t)i0 * 2;
                        u32x4a x = *reinterpret_cast<const u32x4a*>(pp2);
                        u32x4a y = *reinterpret_cast<const u32x4a*>(pp2 + 4);
                        if constexpr (NW >= 2) {
                            w[4 * v + 0][a] = x[0];
                            w[4 * v + 0][a + 1 < NW ? a + 1 : a] = x[1];
                            w[4 * v + 1][a] = x[2];
                            w[4 * v + 1][a + 1 < NW ? a + 1 : a] = x[3];
                            w[4 * v + 2][a] = y[0];
                            w[4 * v + 2][a + 1 < NW ? a + 1 : a] = y[1];
                            w[4 * v + 3][a] = y[2];
                            w[4 * v + 3][a + 1 < NW ? a + 1 : a] = y[3];
                        }
                    } else if (a != pair + 1 || pair < 0) {
                        u32x4a x = *reinterpret_cast<const u32x4a*>(in.w[a] + i0);
#pragma unroll
                        for (int e = 0; e < 4; ++e) w[4 * v + e][a] = x[e];
                    }
                }
            }
            return PT_ALL_ITEMS;
        }
        uint32_t ok = 0;
#pragma unroll
        for (int j = 0; j < PT_ITEMS; ++j) {
            uint32_t i = base + j * PT_THREADS + threadIdx.x;
            uint32_t ic = min(i, end - 1u);
#pragma unroll
            for (int a = 0; a < NW; ++a) {
                if (a == pair) {
                    const uint2 t = reinterpret_cast<const uint2*>(in.w[a])[ic];
                    w[j][a] = t.x;
                    w[j][a + 1 < NW ? a + 1 : a] = t.y;
                } else if (a != pair + 1 || pair < 0) {
                    w[j][a] = in.w[a][ic];
                }
            }
            ok |= (uint32_t)(i < end) << j;
        }
        return ok;
    }
};

using DenseLoader = DenseLoaderT<-1>;


// One array of 12-byte {hashed key, carry lo, carry hi} tuples (what every pass of a key +
// two-word-carry plan writes): four consecutive tuples = three 16-byte loads.
struct Aos3Loader {
    const uint32_t* in;
    RJ_TRIVIAL_ISSUE_FINISH
    template <int NW>
    __device__ __forceinline__ uint32_t load_tile(uint32_t base, uint32_t end, uint32_t (&w)[PT_ITEMS][NW]) const {
        static_assert(NW == 3, "12-byte tuples");
        if (base + PT_TILE <= end) {
#pragma unroll
            for (int v = 0; v < PT_ITEMS / 4; ++v) {
                const uint32_t* p = in + (size_t)(base + (v * PT_THREADS + threadIdx.x) * 4) * 3;
                const u32x4a    x = *reinterpret_cast<const u32x4a*>(p), y = *reinterpret_cast<const u32x4a*>(p + 4),
                             z = *reinterpret_cast<const u32x4a*>(p + 8);
                w[4 * v + 0][0] = x[0];
                w[4 * v + 0][1] = x[1];
                w[4 * v + 0][2] = x[2];
                w[4 * v + 1][0] = x[3];
                w[4 * v + 1][1] = y[0];
                w[4 * v + 1][2] = y[1];
                w[4 * v + 2][0] = y[2];
                w[4 * v + 2][1] = y[3];
                w[4 * v + 2][2] = z[0];
                w[4 * v + 3][0] = z[1];
                w[4 * v + 3][1] = z[2];
                w[4 * v + 3][2] = z[3];
            }
            return PT_ALL_ITEMS;
        }
        uint32_t ok = 0;
#pragma unroll
        for (int j = 0; j < PT_ITEMS; ++j) {
            const uint32_t  i = base + j * PT_THREADS + threadIdx.x;
            const uint32_t* p = in + (size_t)min(i, end - 1u) * 3;
            w[j][0] = p[0];
            w[j][1] = p[1];
            w[j][2] = p[2];
            ok |= (uint32_t)(i < end) << j;
        }
        return ok;
    }
};

// Keys only out of 12-byte tuples (the histogram of a later pass when no digit side array was
// written): every third word.  The lines are fetched whole either way — 12 bytes of HBM traffic
// per tuple for 4 bytes of key — which pays only where the scatter behind it finds them cached.
struct Aos3KeyLoader {
    const uint32_t* in;
    __device__ __forceinline__ uint32_t key_tile(uint32_t base, uint32_t end, uint32_t (&hk)[PT_ITEMS]) const {
        if (base + PT_TILE <= end) {
#pragma unroll
            for (int v = 0; v < PT_ITEMS / 4; ++v) {
                const uint32_t* p = in + (size_t)(base + (v * PT_THREADS + threadIdx.x) * 4) * 3;
                const u32x4a    x = *reinterpret_cast<const u32x4a*>(p), y = *reinterpret_cast<const u32x4a*>(p + 4),
                             z = *reinterpret_cast<const u32x4a*>(p + 8);
                hk[4 * v + 0] = x[0];
                hk[4 * v + 1] = x[3];
                hk[4 * v + 2] = y[2];
                hk[4 * v + 3] = z[1];
            }
            return PT_ALL_ITEMS;
        }
        uint32_t ok = 0;
#pragma unroll
        for (int j = 0; j < PT_ITEMS; ++j) {
            const uint32_t i = base + j * PT_THREADS + threadIdx.x;
            hk[j] = in[(size_t)min(i, end - 1u) * 3];
            ok |= (uint32_t)(i < end) << j;
        }
        return ok;
    }
};

// The side array of 16-bit digits a 12-byte-tuple pass wrote for its successor: the histogram
// of that successor reads 2 bytes per tuple.  key_tile hands the digit back in the bit position
// the histogram kernel takes it from.
struct DigitLoader {
    static constexpr bool kNeedsBegin = true;
    const uint16_t* digits;
    uint32_t        shift;
    // Full tiles read sixteen consecutive digits per thread with two 16-byte loads.  Loads are
    // 4-byte aligned, digits 2-byte: a full tile that starts at an ODD index covers the window
    // one element earlier, [base - 1, base - 1 + PT_TILE).  The windows of consecutive tiles
    // still tile the group's range [begin, end) exactly once (the histogram does not care which
    // tile counts a tuple):
    //   * the element in front of the group's first tile (begin - 1) is masked out;
    //   * the element a full odd tile leaves behind (base + PT_TILE - 1) is the first one of the
    //     next tile's window — a partial last tile starts one element early for it, and when
    //     there is no next tile extra() hands it to thread 0.
    __device__ __forceinline__ uint32_t key_tile(uint32_t base, uint32_t begin, uint32_t end,
                                                 uint32_t (&hk)[PT_ITEMS]) const {
        static_assert(PT_ITEMS % 8 == 0, "16-byte loads of eight digits each");
        if (base + PT_TILE <= end) {
            const uint32_t* w = reinterpret_cast<const uint32_t*>(digits) + (base >> 1);
#pragma unroll
            for (int v = 0; v < PT_ITEMS / 8; ++v) {
                const uint32_t wi = (v * PT_THREADS + threadIdx.x) * 4;
                const u32x4a   x = __builtin_nontemporal_load(reinterpret_cast<const u32x4a*>(w + wi));
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    hk[8 * v + 2 * e] = (x[e] & 0xffffu) << shift;
                    hk[8 * v + 2 * e + 1] = (x[e] >> 16) << shift;
                }
            }
            uint32_t ok = PT_ALL_ITEMS;
            if ((base & 1u) && base == begin && threadIdx.x == 0) ok &= ~1u;  // element begin - 1
            return ok;
        }
        const uint32_t b0 = ((base & 1u) && base != begin) ? base - 1u : base;
        uint32_t       ok = 0;
#pragma unroll
        for (int j = 0; j < PT_ITEMS; ++j) {
            const uint32_t i = b0 + j * PT_THREADS + threadIdx.x;
            hk[j] = (uint32_t)digits[min(i, end - 1u)] << shift;
            ok |= (uint32_t)(i < end) << j;
        }
        return ok;
    }
    // the group's last element when its last tile is a full odd one (see above)
    __device__ __forceinline__ bool extra(uint32_t begin, uint32_t end, uint32_t& hk) const {
        if (threadIdx.x != 0 || !(begin & 1u) || end == begin || (end - begin) % (uint32_t)PT_TILE) return false;
        hk = (uint32_t)digits[end - 1u] << shift;
        return true;
    }
};

// Partitioned tuples of ONE key word + ONE carry word can also be kept packed: an array of
// 8-byte {hashed key, carry} pairs instead of two word arrays (see k_pass_scatter_packed).
struct PackedLoader {
    const uint2* in;
    RJ_TRIVIAL_ISSUE_FINISH
    __device__ __forceinline__ uint32_t issue_keys(uint32_t base, uint32_t end, uint32_t (&lo)[PT_ITEMS],
                                                   uint32_t (&)[PT_ITEMS]) const {
        return key_tile(base, end, lo);
    }
    __device__ __forceinline__ uint32_t finish_keys(uint32_t, uint32_t, uint32_t ok, uint32_t (&)[PT_ITEMS],
                                                    uint32_t (&)[PT_ITEMS]) const {
        return ok;
    }
    // keys only (histogram of a later pass): every second word of the pairs
    __device__ __forceinline__ uint32_t key_tile(uint32_t base, uint32_t end,
                                                 uint32_t (&hk)[PT_ITEMS]) const {
        if (base + PT_TILE <= end) {
#pragma unroll
            for (int v = 0; v < PT_ITEMS / 2; ++v) {
                u32x4a x = *reinterpret_cast<const u32x4a*>(in + base + (v * PT_THREADS + threadIdx.x) * 2);
                hk[2 * v] = x[0];
                hk[2 * v + 1] = x[2];
            }
            return PT_ALL_ITEMS;
        }
        uint32_t ok = 0;
#pragma unroll
        for (int j = 0; j < PT_ITEMS; ++j) {
            uint32_t i = base + j * PT_THREADS + threadIdx.x;
            hk[j] = in[min(i, end - 1u)].x;
            ok |= (uint32_t)(i < end) << j;
        }
        return ok;
    }
    template <int NW>
    __device__ __forceinline__ uint32_t load_tile(uint32_t base, uint32_t end,
                                                  uint32_t (&w)[PT_ITEMS][NW]) const {
        static_assert(NW == 2, "packed tuples are key + one carry word");
        if (base + PT_TILE <= end) {  // two consecutive tuples per 16-byte load
#pragma unroll
            for (int v = 0; v < PT_ITEMS / 2; ++v) {
                u32x4a x = *reinterpret_cast<const u32x4a*>(in + base + (v * PT_THREADS + threadIdx.x) * 2);
                w[2 * v][0] = x[0];
                w[2 * v][1] = x[1];
                w[2 * v + 1][0] = x[2];
                w[2 * v + 1][1] = x[3];
            }
            return PT_ALL_ITEMS;
        }
        uint32_t ok = 0;
#pragma unroll
        for (int j = 0; j < PT_ITEMS; ++j) {
            uint32_t i = base + j * PT_THREADS + threadIdx.x;
            uint2    t = in[min(i, end - 1u)];
            w[j][0] = t.x;
            w[j][1] = t.y;
            ok |= (uint32_t)(i < end) << j;
        }
        return ok;
    }
};

// {hashed key, carry} pairs BETWEEN the passes of a packed plan, blocked: tuple g lives in block g / 256 —
// 512 words: the 256 keys, then the 256 carries — so that the next pass' histogram reads the key halves
// only (4 instead of 8 bytes per tuple; with 16-tuple blocks it still pulled every line) while a
// scatter writes a run of consecutive tuples into ONE array.
struct BlockedLoader {
    const uint32_t* in;
    RJ_TRIVIAL_ISSUE_FINISH
    __device__ __forceinline__ uint32_t issue_keys(uint32_t base, uint32_t end, uint32_t (&lo)[PT_ITEMS],
                                                   uint32_t (&)[PT_ITEMS]) const {
        return key_tile(base, end, lo);
    }
    __device__ __forceinline__ uint32_t finish_keys(uint32_t, uint32_t, uint32_t ok, uint32_t (&)[PT_ITEMS],
                                                    uint32_t (&)[PT_ITEMS]) const {
        return ok;
    }
    static constexpr uint32_t BLK = 256;  // tuples per block: 1 KiB of keys, then 1 KiB of carries (64 / 256 / 1024 measured: profiles/r03_ao_*)
    static __device__ __forceinline__ size_t key_at(uint32_t g) { return (size_t)(g / BLK) * (2u * BLK) + (g % BLK); }
    __device__ __forceinline__ uint32_t key_tile(uint32_t base, uint32_t end, uint32_t (&hk)[PT_ITEMS]) const {
        uint32_t ok = 0;
#pragma unroll
        for (int j = 0; j < PT_ITEMS; ++j) {
            const uint32_t i = base + j * PT_THREADS + threadIdx.x;
            hk[j] = in[key_at(min(i, end - 1u))];
            ok |= (uint32_t)(i < end) << j;
        }
        return ok;
    }
    template <int NW>
    __device__ __forceinline__ uint32_t load_tile(uint32_t base, uint32_t end, uint32_t (&w)[PT_ITEMS][NW]) const {
        static_assert(NW == 2, "packed tuples are key + one carry word");
        uint32_t ok = 0;
#pragma unroll
        for (int j = 0; j < PT_ITEMS; ++j) {
            const uint32_t i = base + j * PT_THREADS + threadIdx.x;
            const size_t   a = key_at(min(i, end - 1u));
            w[j][0] = in[a];
            w[j][1] = in[a + BLK];
            ok |= (uint32_t)(i < end) << j;
        }
        return ok;
    }
};

// byte offset of row `row` in a 4-byte / 8-byte column (regular page images or dense)
__device__ __forceinline__ uint64_t col_off32(bool paged, uint32_t row) {
    uint32_t p = row / ROWS32, i = row - p * ROWS32;
    uint64_t po = (uint64_t)p * PAGE_BYTES + HDR32 + i * 4u;
    return paged ? po : (uint64_t)row * 4u;
}
__device__ __forceinline__ uint64_t col_off64(bool paged, uint32_t row) {
    uint32_t p = row / ROWS64, i = row - p * ROWS64;
    uint64_t po = (uint64_t)p * PAGE_BYTES + HDR64 + i * 8u;
    return paged ? po : (uint64_t)row * 8u;
}

// Forms tuples straight from columns: page decode (regular pages), NULL-key
// drop (reference src/execute.cpp:62-83: only rows whose variant holds KeyType
// are valid) and hashing fused into the first radix pass.
// WIDE (WideLayout): the carry is made of several columns — two or three 32-bit ones, or a
// 64-bit one followed by a 32-bit one (CARRY_WIDE; a validity word, where some carried column
// has NULLs, is one of the 32-bit columns by then: k_pack_validity).
template <int KW, int CW, int WIDE = WIDE_NONE>
struct SrcLoader {
    static_assert(WIDE == WIDE_NONE || (WIDE == WIDE_32S && CW >= 2) || (WIDE == WIDE_64_32 && CW == 3), "wide carry layouts");
    TupleSrc s;

    // Row of item j.  Full tiles use the vector mapping (four consecutive rows per thread
    // and 16-byte load; ROWS32 % 4 == 0 and tiles start at multiples of 4, so the four rows
    // share a page), partial tiles the strided one with clamped indices.
    // (tid: threadIdx.x, or the scatter kernels' tile_tid())
    __device__ __forceinline__ static uint32_t item_row(bool vec, uint32_t base, int j, uint32_t tid = threadIdx.x) {
        return vec ? base + ((j / 4) * PT_THREADS + tid) * 4 + (j % 4)
                   : base + j * PT_THREADS + tid;
    }

    // 32-bit column -> one word per item
    // NT: non-temporal loads — the histogram kernels stream the key column once and gain from
    // not parking it in the L2 (pass-1 histogram 1.47 -> 1.38 ms at 1 B rows, the fine histogram
    // 0.115 -> 0.085 ms at 100 M); the scatter kernels lose with the same hint (their loads
    // compete with half-written output lines for the L2: profiles/r02_ax_*), so they do not use it
    // Addresses are formed as a UNIFORM 64-bit tile base (the page that holds the tile's first row,
    // or the first row itself for dense columns) plus a 32-bit per-lane byte offset — one VGPR per
    // outstanding load instead of a 64-bit pair, and no 64-bit vector arithmetic: with all loads of
    // a tile in flight at once the 64-bit form spilled to scratch.
    template <bool NT = false>
    __device__ __forceinline__ static void load_col32(const ColRef& c, bool vec, uint32_t base,
                                                      uint32_t end, uint32_t (&out)[PT_ITEMS], uint32_t tid = threadIdx.x) {
        const bool     paged = c.kind == COL_PAGED;
        const uint32_t ub = __builtin_amdgcn_readfirstlane(base);
        const uint32_t p0 = ub / ROWS32, s0 = ub - p0 * ROWS32;  // page / slot of the tile's first row
        const uint8_t* tp = paged ? c.ptr + (size_t)p0 * PAGE_BYTES : c.ptr + (size_t)ub * 4u;
        // byte offset of row base + rel from tp, branch-free for both kinds:
        //   dense  rel * 4
        //   paged  q * PAGE + HDR + (t - q * ROWS) * 4  =  rel * 4 + (s0 * 4 + HDR) + q * (PAGE - ROWS * 4),
        //          t = s0 + rel, q = t / ROWS  (pages crossed since the tile's first page)
        const uint32_t bias = paged ? s0 * 4u + HDR32 : 0u, per_page = paged ? PAGE_BYTES - ROWS32 * 4u : 0u;
        auto           off = [&](uint32_t rel) -> uint32_t { return rel * 4u + bias + ((s0 + rel) / ROWS32) * per_page; };
        if (vec) {
#pragma unroll
            for (int v = 0; v < PT_ITEMS / 4; ++v) {
                const u32x4a* q = reinterpret_cast<const u32x4a*>(tp + off((v * PT_THREADS + tid) * 4u));
                u32x4a        x;
                if constexpr (NT)
                    x = __builtin_nontemporal_load(q);
                else
                    x = *q;
#pragma unroll
                for (int e = 0; e < 4; ++e) out[4 * v + e] = x[e];
            }
        } else {
            const uint32_t last = end - 1u - ub;
#pragma unroll
            for (int j = 0; j < PT_ITEMS; ++j)
                out[j] = *reinterpret_cast<const uint32_t*>(tp + off(min((uint32_t)(j * PT_THREADS + tid), last)));
        }
    }
    template <bool NT = false>
    __device__ __forceinline__ static void load_col64(const ColRef& c, bool vec, uint32_t base,
                                                      uint32_t end, uint32_t (&lo)[PT_ITEMS],
                                                      uint32_t (&hi)[PT_ITEMS], uint32_t tid = threadIdx.x) {
        const bool     paged = c.kind == COL_PAGED;
        const uint32_t ub = __builtin_amdgcn_readfirstlane(base);
        const uint32_t p0 = ub / ROWS64, s0 = ub - p0 * ROWS64;
        const uint8_t* tp = paged ? c.ptr + (size_t)p0 * PAGE_BYTES : c.ptr + (size_t)ub * 8u;
        const uint32_t last = end - 1u - ub;
        const uint32_t bias = paged ? s0 * 8u + HDR64 : 0u, per_page = paged ? PAGE_BYTES - ROWS64 * 8u : 0u;
#pragma unroll
        for (int j = 0; j < PT_ITEMS; ++j) {
            const uint32_t rel = min(item_row(vec, 0u, j, tid), last);
            const uint32_t o = rel * 8u + bias + ((s0 + rel) / ROWS64) * per_page;  // (see load_col32)
            const uint64_t* a = reinterpret_cast<const uint64_t*>(tp + o);
            uint64_t        v;
            if constexpr (NT)
                v = __builtin_nontemporal_load(a);
            else
                v = *a;
            lo[j] = (uint32_t)v;
            hi[j] = (uint32_t)(v >> 32);
        }
    }
    // a 32-bit column of any kind (a base table's row-id column included)
    __device__ __forceinline__ static void load_col32_any(const ColRef& c, bool vec, uint32_t base, uint32_t end,
                                                          uint32_t (&out)[PT_ITEMS], uint32_t tid = threadIdx.x) {
        if (c.kind == COL_IOTA) {
#pragma unroll
            for (int j = 0; j < PT_ITEMS; ++j) out[j] = item_row(vec, base, j, tid);
        } else {
            load_col32(c, vec, base, end, out, tid);
        }
    }

    // raw key words of the tile + in-range mask
    template <bool NT = false>
    __device__ __forceinline__ uint32_t raw_keys(bool vec, uint32_t base, uint32_t end,
                                                 uint32_t (&lo)[PT_ITEMS],
                                                 uint32_t (&hi)[PT_ITEMS], uint32_t tid = threadIdx.x) const {
        if constexpr (KW == 1) {
            load_col32<NT>(s.key, vec, base, end, lo, tid);
#pragma unroll
            for (int j = 0; j < PT_ITEMS; ++j) hi[j] = 0;
        } else {
            load_col64<NT>(s.key, vec, base, end, lo, hi, tid);
        }
        if (vec) return PT_ALL_ITEMS;
        uint32_t ok = 0;
#pragma unroll
        for (int j = 0; j < PT_ITEMS; ++j)
            ok |= (uint32_t)(base + j * PT_THREADS + tid < end) << j;
        return ok;
    }
    __device__ __forceinline__ uint32_t drop_invalid(bool vec, uint32_t base, uint32_t end,
                                                     uint32_t ok, uint32_t tid = threadIdx.x) const {
        const uint8_t* vp = s.key.valid;
        if (vp) {  // uniform: the column was decoded by K1 and carries validity bytes
#pragma unroll
            for (int j = 0; j < PT_ITEMS; ++j)
                if (!vp[min(item_row(vec, base, j, tid), end - 1u)]) ok &= ~(1u << j);
        }
        return ok;
    }
    // hash in place; FP64: NaN never matches (see key semantics below)
    __device__ __forceinline__ uint32_t hash_keys(uint32_t ok, uint32_t (&lo)[PT_ITEMS],
                                                  uint32_t (&hi)[PT_ITEMS]) const {
#pragma unroll
        for (int j = 0; j < PT_ITEMS; ++j) {
            if constexpr (KW == 1) {
                lo[j] = s.prehashed ? lo[j] : fmix32(lo[j]);
            } else {
                uint64_t k = (uint64_t)lo[j] | ((uint64_t)hi[j] << 32);
                // The reference hashes the BIT PATTERN of a double (src/execute.cpp:28-31) and
                // compares with == (:215,231): NaN equals nothing, and -0.0 / +0.0 hash to
                // different slots so they only meet by accident of probing.  Bit-pattern
                // equality with NaN excluded reproduces that (SURVEY.md §8a note on FP64).
                if (s.key_f64 && (k & 0x7ff0000000000000ull) == 0x7ff0000000000000ull &&
                    (k & 0x000fffffffffffffull))
                    ok &= ~(1u << j);
                uint64_t h = fmix64(k);
                lo[j] = (uint32_t)h;
                hi[j] = (uint32_t)(h >> 32);
            }
        }
        return ok;
    }
    __device__ __forceinline__ uint32_t key_tile(uint32_t base, uint32_t end,
                                                 uint32_t (&hk)[PT_ITEMS]) const {
        const bool vec = base + PT_TILE <= end;
        uint32_t   hi[PT_ITEMS];
        uint32_t   ok = raw_keys<true>(vec, base, end, hk, hi);
        ok = drop_invalid(vec, base, end, ok);
        return hash_keys(ok, hk, hi);
    }
    // The same in two halves, for a software pipeline: issue_keys only ISSUES the loads of the
    // raw key words, finish_keys (which needs the data) drops invalid rows and hashes.
    __device__ __forceinline__ uint32_t issue_keys(uint32_t base, uint32_t end,
                                                   uint32_t (&lo)[PT_ITEMS],
                                                   uint32_t (&hi)[PT_ITEMS]) const {
        return raw_keys<true>(base + PT_TILE <= end, base, end, lo, hi);
    }
    __device__ __forceinline__ uint32_t finish_keys(uint32_t base, uint32_t end, uint32_t ok,
                                                    uint32_t (&lo)[PT_ITEMS],
                                                    uint32_t (&hi)[PT_ITEMS]) const {
        ok = drop_invalid(base + PT_TILE <= end, base, end, ok);
        return hash_keys(ok, lo, hi);
    }
    // The tile in two halves (see issue_keys / finish_keys): issue_tile ISSUES every load of the
    // tile — raw key words into w[.][0..KW), carry words behind them — and finish_tile, which
    // needs the key data, drops invalid rows and hashes the keys in place.
    template <int NW>
    __device__ __forceinline__ uint32_t issue_tile(uint32_t base, uint32_t end,
                                                   uint32_t (&w)[PT_ITEMS][NW]) const {
        static_assert(NW == KW + CW, "word count");
        const bool vec = base + PT_TILE <= end;
        uint32_t   lo[PT_ITEMS], hi[PT_ITEMS];
        // (an opaque thread index: the per-lane rows and offsets are formed anew for every tile instead of
        // being kept in registers, or spilled, from tile to tile)
        const uint32_t tid = tile_tid();
        uint32_t       ok = raw_keys(vec, base, end, lo, hi, tid);
        if constexpr (WIDE == WIDE_32S) {
            uint32_t c0[PT_ITEMS];
            load_col32_any(s.carry, vec, base, end, c0, tid);
#pragma unroll
            for (int j = 0; j < PT_ITEMS; ++j) w[j][KW] = c0[j];
            load_col32_any(s.carry2, vec, base, end, c0, tid);
#pragma unroll
            for (int j = 0; j < PT_ITEMS; ++j) w[j][KW + 1] = c0[j];
            if constexpr (CW == 3) {
                load_col32_any(s.carry3, vec, base, end, c0, tid);
#pragma unroll
                for (int j = 0; j < PT_ITEMS; ++j) w[j][KW + 2] = c0[j];
            }
        } else if constexpr (WIDE == WIDE_64_32) {
            uint32_t c0[PT_ITEMS], c1[PT_ITEMS];
            load_col64(s.carry, vec, base, end, c0, c1, tid);
#pragma unroll
            for (int j = 0; j < PT_ITEMS; ++j) {
                w[j][KW] = c0[j];
                w[j][KW + 1] = c1[j];
            }
            load_col32_any(s.carry2, vec, base, end, c0, tid);
#pragma unroll
            for (int j = 0; j < PT_ITEMS; ++j) w[j][KW + 2] = c0[j];
        } else if constexpr (CW == 1) {
            // (a row-index carry is one word by construction.  Asked for at every CW, the branch left the
            // second carry word of a two-word tuple undefined on one path, and the compiler kept the last
            // item's pair in scratch memory for it: 16 bytes per lane, stored behind a wait for the payload)
            if (s.carry_mode == CARRY_ROWIDX) {
#pragma unroll
                for (int j = 0; j < PT_ITEMS; ++j) w[j][KW] = item_row(vec, base, j, tid);
            } else {
                uint32_t c0[PT_ITEMS];
                load_col32(s.carry, vec, base, end, c0, tid);
#pragma unroll
                for (int j = 0; j < PT_ITEMS; ++j) w[j][KW] = c0[j];
            }
        } else if constexpr (CW >= 2) {
            uint32_t c0[PT_ITEMS], c1[PT_ITEMS];
            load_col64(s.carry, vec, base, end, c0, c1, tid);
#pragma unroll
            for (int j = 0; j < PT_ITEMS; ++j) {
                w[j][KW] = c0[j];
                w[j][KW + 1] = c1[j];
            }
        }
#pragma unroll
        for (int j = 0; j < PT_ITEMS; ++j) {
            w[j][0] = lo[j];
            if constexpr (KW == 2) w[j][1] = hi[j];
        }
        return ok;
    }
    template <int NW>
    __device__ __forceinline__ uint32_t finish_tile(uint32_t base, uint32_t end, uint32_t ok,
                                                    uint32_t (&w)[PT_ITEMS][NW]) const {
        const bool vec = base + PT_TILE <= end;
        uint32_t   lo[PT_ITEMS], hi[PT_ITEMS];
#pragma unroll
        for (int j = 0; j < PT_ITEMS; ++j) {
            lo[j] = w[j][0];
            hi[j] = KW == 2 ? w[j][KW - 1] : 0u;
        }
        ok = drop_invalid(vec, base, end, ok, tile_tid());
        ok = hash_keys(ok, lo, hi);
#pragma unroll
        for (int j = 0; j < PT_ITEMS; ++j) {
            w[j][0] = lo[j];
            if constexpr (KW == 2) w[j][1] = hi[j];
        }
        return ok;
    }
    template <int NW>
    __device__ __forceinline__ uint32_t load_tile(uint32_t base, uint32_t end,
                                                  uint32_t (&w)[PT_ITEMS][NW]) const {
        return finish_tile<NW>(base, end, issue_tile<NW>(base, end, w), w);
    }
};

// Which tuples does workgroup `g` own?  A group is up to tiles_per_group
// consecutive tiles inside ONE input segment.
__device__ __forceinline__ bool group_range(const PassParams& pp, uint32_t g, uint32_t& seg,
                                            uint32_t& begin, uint32_t& end) {
    const uint32_t gt = pp.tiles_per_group * (uint32_t)PT_TILE;
    if (pp.seg_off == nullptr) {
        seg = 0;
        uint64_t b = (uint64_t)g * gt;
        if (b >= pp.n) return false;
        begin = (uint32_t)b;
        end = (uint32_t)min((uint64_t)pp.n, b + gt);
        return true;
    }
    const uint32_t G = pp.grp_start[pp.nseg] - pp.grp_base;
    if (pp.xcd_remap) {
        const uint32_t per = (G + 7u) >> 3;
        if ((g >> 3) >= per) return false;
        g = (g & 7u) * per + (g >> 3);
    }
    if (g >= G) return false;
    uint32_t lo = 0, hi = pp.nseg;  // largest s with grp_start[s] <= g
    while (hi - lo > 1) {
        uint32_t mid = (lo + hi) >> 1;
        if (pp.grp_start[mid] - pp.grp_base <= g)
            lo = mid;
        else
            hi = mid;
    }
    seg = lo >> pp.oseg_shift;  // the OUTPUT segment (bins, cursors) input segment `lo` feeds
    uint32_t gi = g - (pp.grp_start[lo] - pp.grp_base);
    uint64_t b = (uint64_t)pp.seg_off[lo] + (uint64_t)gi * gt;
    begin = (uint32_t)b;
    end = (uint32_t)min((uint64_t)(pp.seg_end ? pp.seg_end[lo] : pp.seg_off[lo + 1]), b + gt);
    return begin < end;
}

template <class L, class = void>
struct loader_needs_begin : std::false_type {};
template <class L>
struct loader_needs_begin<L, std::enable_if_t<L::kNeedsBegin>> : std::true_type {};

// ============================================================== K2 histogram
// Counting half of the radix partition (reference counterpart: the serial
// histogram src/execute.cpp:124-132).  LDS atomics per tuple, F global adds per group for
// the bin totals.
// (A hot-key test per tuple — one probe of a 4096-entry LDS set, the price of a skew bypass — cost
// +0.17 ms here and nothing measurable in the scatters.  Taken out again;
// profiles/r03_am_hot_probe_ab.log is the record.)
template <class Loader>
__global__ __launch_bounds__(PT_THREADS) void k_pass_hist(Loader ld, PassParams pp) {
    __shared__ uint32_t s_h[PT_MAXF];
    uint32_t            seg, begin, end;
    if (!group_range(pp, blockIdx.x, seg, begin, end)) return;
    const uint32_t F = 1u << pp.fanout_log2, mask = F - 1u;
    for (uint32_t d = threadIdx.x; d < F; d += PT_THREADS) s_h[d] = 0;
    lds_barrier();
    for (uint32_t base = begin; base < end; base += PT_TILE) {
        uint32_t hk[PT_ITEMS];
        uint32_t ok;
        if constexpr (loader_needs_begin<Loader>::value)
            ok = ld.key_tile(base, begin, end, hk);
        else
            ok = ld.key_tile(base, end, hk);
#pragma unroll
        for (int j = 0; j < PT_ITEMS; ++j) {
            if ((ok >> j) & 1u) atomicAdd(&s_h[pass_digit(pp, hk[j], mask)], 1u);
        }
    }
    if constexpr (loader_needs_begin<Loader>::value) {
        uint32_t hx;
        if (ld.extra(begin, end, hx)) atomicAdd(&s_h[pass_digit(pp, hx, mask)], 1u);
    }
    lds_barrier();
    for (uint32_t d = threadIdx.x; d < F; d += PT_THREADS) {
        uint32_t c = s_h[d];
        if (c) atomicAdd(&pp.hist[(((size_t)seg * F + d) << pp.xcd_log2) | (blockIdx.x & ((1u << pp.xcd_log2) - 1u))], c);
    }
}

// ============================================== speculative first pass: sample, capacities, closing
// k_pass_hist over the source with a 2^-sample_log2 sample: grid, workgroup -> tile-group mapping and bins
// (hist[(d << 3) | (blockIdx.x & 7)]) are k_pass_hist's, but of every tile only one slice of
// PT_TILE >> sample_log2 consecutive rows is read.  Sub-range x of digit d is therefore sampled from exactly the
// rows that the workgroups with g & 7 == x will scatter.  The slice's place inside its tile moves with the tile
// index by 7 slices (an odd number: every place comes up before one repeats), so that data with a fixed period
// does not meet the sample at the same phase in every tile.  NULL keys, rows behind the relation's end and
// hashing are the scatter's (SrcLoader::drop_invalid / hash_keys).  In a partial last tile the slice ends with the
// tile at the latest (its place is min(that place, rows - slice)); a tile of no more rows than a slice is read whole.
static_assert((PT_TILE & (PT_TILE - 1)) == 0, "a tile's sample slice is a power-of-two fraction of it");
template <int KW>
__global__ __launch_bounds__(PT_THREADS) void k_pass_sample(TupleSrc s, PassParams pp, SpecParams sp) {
    __shared__ uint32_t s_h[PT_MAXF];
    uint32_t            seg, begin, end;
    if (!group_range(pp, blockIdx.x, seg, begin, end)) return;
    const uint32_t F = 1u << pp.fanout_log2, mask = F - 1u;
    for (uint32_t d = threadIdx.x; d < F; d += PT_THREADS) s_h[d] = 0;
    lds_barrier();
    const uint32_t slog = (uint32_t)__builtin_ctz((unsigned)PT_TILE) - sp.sample_log2, slice = 1u << slog;
    const uint32_t ntiles = (end - begin + (uint32_t)PT_TILE - 1u) / (uint32_t)PT_TILE;
    const uint32_t total = ntiles << slog;  // sample positions of this group
    constexpr int  U = 4;                   // positions a thread has in flight
    for (uint32_t i0 = threadIdx.x; i0 < total; i0 += U * PT_THREADS) {
        uint32_t lo[U], hi[U];
        bool     ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t i = i0 + u * PT_THREADS, ic = min(i, total - 1u);
            const uint32_t t = ic >> slog, r = ic & (slice - 1u);
            const uint32_t tb = begin + t * (uint32_t)PT_TILE, rows = min((uint32_t)PT_TILE, end - tb);
            const uint32_t rot = ((tb / (uint32_t)PT_TILE) * 7u << slog) & ((uint32_t)PT_TILE - 1u);
            const uint32_t at = rows > slice ? min(rot, rows - slice) : 0u;
            const uint32_t row = tb + min(at + r, rows - 1u);
            ok[u] = i < total && r < rows;
            if constexpr (KW == 1) {
                lo[u] = col_load32(s.key, row);
                hi[u] = 0;
            } else {
                const uint64_t k = col_load64(s.key, row);
                lo[u] = (uint32_t)k;
                hi[u] = (uint32_t)(k >> 32);
            }
            if (s.key.valid && !s.key.valid[row]) ok[u] = false;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            uint32_t h;
            if constexpr (KW == 1) {
                h = s.prehashed ? lo[u] : fmix32(lo[u]);
            } else {
                const uint64_t k = (uint64_t)lo[u] | ((uint64_t)hi[u] << 32);
                if (s.key_f64 && (k & 0x7ff0000000000000ull) == 0x7ff0000000000000ull && (k & 0x000fffffffffffffull))
                    ok[u] = false;  // NaN never matches (see SrcLoader::hash_keys)
                h = (uint32_t)fmix64(k);
            }
            if (ok[u]) atomicAdd(&s_h[pass_digit(pp, h, mask)], 1u);
        }
    }
    lds_barrier();
    for (uint32_t d = threadIdx.x; d < F; d += PT_THREADS) {
        uint32_t c = s_h[d];
        if (c) atomicAdd(&pp.hist[(((size_t)seg * F + d) << pp.xcd_log2) | (blockIdx.x & ((1u << pp.xcd_log2) - 1u))], c);
    }
}

// Capacities from the sample counts, one workgroup.  A sub-range whose sample holds c tuples gets room for
//   cap = 2^s (c + z sqrt(c + 1) + z^2 / 2)   tuples, rounded up to a multiple of 32
// — a one-sided normal bound on a binomial count: for rows in random order a sub-range overflows with
// probability Phi(-z).  start[] is the exclusive scan of cap in bin order (x minor under d: a digit's eight
// sub-ranges stay adjacent), limit[] = start + cap, cursor[] = {start, cap}.  Nothing reaches beyond cap_max,
// the tuples the host made room for from its bound on the sum (radix_cap_bound, rj_radix_plan.cpp): a sub-range that would is cut
// there, and overflows like any other that is too small.
__global__ __launch_bounds__(1024) void k_spec_caps(const uint32_t* sample, uint32_t nbins, uint32_t sample_log2, float z,
                                                    uint32_t cap_max, uint32_t* start, uint32_t* limit,
                                                    unsigned long long* cursor) {
    __shared__ unsigned long long s_sum[1024];
    const uint32_t                chunk = (nbins + 1023u) / 1024u;
    const uint32_t                b = min(nbins, threadIdx.x * chunk), e = min(nbins, b + chunk);
    auto                          cap_of = [&](uint32_t c) -> unsigned long long {
        const double zz = (double)z, x = (double)c + zz * sqrt((double)c + 1.0) + 0.5 * zz * zz;
        const unsigned long long t = (unsigned long long)ceil(ldexp(x, (int)sample_log2));
        return (t + 31ull) & ~31ull;
    };
    unsigned long long sum = 0;
    for (uint32_t i = b; i < e; ++i) sum += cap_of(sample[i]);
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    unsigned long long run = 0;
    for (uint32_t k = 0; k < threadIdx.x; ++k) run += s_sum[k];
    for (uint32_t i = b; i < e; ++i) {
        const unsigned long long nx = run + cap_of(sample[i]);
        const uint32_t           st = (uint32_t)min(run, (unsigned long long)cap_max);
        const uint32_t           lim = (uint32_t)min(nx, (unsigned long long)cap_max);
        start[i] = st;
        limit[i] = lim;
        cursor[i] = (unsigned long long)st | ((unsigned long long)(lim - st) << 32);
        run = nx;
    }
}

// Closing the speculative pass, one workgroup, thread d = digit d: sub-range i of the output holds
// [start[i], seg_end[i]), seg_end = min(where its cursor stands, its limit) — the input segments of the second
// pass — and digit d, the OUTPUT segment of its eight sub-ranges, has the sum of their sizes; oseg_off is the
// exclusive scan of those: where the partitions of digit d begin in the dense output of the second pass.
__global__ __launch_bounds__(PT_MAXF) void k_spec_close(const unsigned long long* cursor, const uint32_t* start,
                                                        const uint32_t* limit, uint32_t F, uint32_t* seg_end,
                                                        uint32_t* oseg_off) {
    __shared__ uint32_t s_wsum[PT_MAXF / 64];
    const uint32_t      d = threadIdx.x;
    uint32_t            v = 0;
    if (d < F)
        for (uint32_t x = 0; x < 8; ++x) {
            const uint32_t i = (d << 3) | x, en = min((uint32_t)cursor[i], limit[i]);
            seg_end[i] = en;
            v += en - start[i];
        }
    uint32_t       total;
    const uint32_t ex = block_excl_scan(v, s_wsum, total);
    if (d < F) oseg_off[d] = ex;
    if (d == 0) oseg_off[F] = total;
}

// Two-pass plans whose final partition count fits an LDS histogram (<= 2^PT_FINEBITS bins)
// count BOTH digits in the one read of the source: bin q = d1 * F2 + d2 is the final
// partition, its exclusive scan is at once the pass-2 offsets and (every F2-th entry) the
// pass-1 offsets, and no second histogram pass over the partitioned tuples is needed.
// Persistent workgroups (one per CU: the histogram takes most of the LDS) stride over the
// tiles and flush their bins with one global add each.
// xcd_tpg > 0 (XCD-aware placement, see PassParams::xcd_log2): the first pass' scatter works in
// groups of xcd_tpg tiles and writes group g's runs into sub-range g & 7 of every partition, so
// it needs the pass-1 digit counts per sub-range.  Workgroup w therefore counts exactly the tile
// groups g with g & 7 == w & 7 (gridDim.x is a multiple of 8) — its whole LDS histogram belongs
// to ONE sub-range, and the per-sub-range counts fall out of the flush (row sums of its bins)
// with no extra work per tuple.
template <class Loader>
__global__ __launch_bounds__(PT_THREADS) void k_fine_hist(Loader ld, uint32_t n, uint32_t shift,
                                                          uint32_t b1, uint32_t b2,
                                                          uint32_t* fine, uint32_t xcd_tpg,
                                                          uint32_t* coarse_x) {
    __shared__ uint32_t s_f[1u << PT_FINEBITS];
    const uint32_t      NB = 1u << (b1 + b2), m1 = (1u << b1) - 1u, m2 = (1u << b2) - 1u;
    for (uint32_t d = threadIdx.x; d < NB; d += PT_THREADS) s_f[d] = 0;
    lds_barrier();
    const uint32_t tiles = (uint32_t)(((uint64_t)n + PT_TILE - 1) / PT_TILE);
    // tile walk: plain striding, or the tile groups of this workgroup's sub-range
    const uint32_t x = blockIdx.x & 7u, gstride = gridDim.x >> 3;
    uint32_t       gk = blockIdx.x >> 3, gj = 0;  // group x + 8 * gk, tile gj inside it
    auto           tile_of = [&](uint32_t k, uint32_t j) { return (x + 8u * k) * xcd_tpg + j; };
    auto           advance = [&](uint32_t t) -> uint32_t {  // the tile after t, >= tiles: none
        if (!xcd_tpg) return t + gridDim.x;
        if (++gj < xcd_tpg && tile_of(gk, gj) < tiles) return tile_of(gk, gj);
        gk += gstride;
        gj = 0;
        const uint64_t nt = (uint64_t)(x + 8ull * gk) * xcd_tpg;
        return nt < tiles ? (uint32_t)nt : 0xffffffffu;
    };
    uint32_t t = xcd_tpg ? tile_of(gk, 0) : blockIdx.x;
    // Software pipeline: the LDS atomics of a tile (a third of its time) run while the NEXT
    // tile's loads are in flight — the raw loads are issued before the atomics, hashing (which
    // needs the data) comes after them.
    uint32_t lo[PT_ITEMS], hi[PT_ITEMS], raw = 0;
    if (t < tiles) raw = ld.issue_keys(t * (uint32_t)PT_TILE, n, lo, hi);
    while (t < tiles) {
        const uint32_t ok = ld.finish_keys(t * (uint32_t)PT_TILE, n, raw, lo, hi);
        uint32_t       q[PT_ITEMS];
#pragma unroll
        for (int j = 0; j < PT_ITEMS; ++j) {
            const uint32_t h = lo[j] >> shift;
            q[j] = ((h & m1) << b2) | ((h >> b1) & m2);
        }
        const uint32_t t2 = advance(t);
        if (t2 < tiles) raw = ld.issue_keys(t2 * (uint32_t)PT_TILE, n, lo, hi);
#pragma unroll
        for (int j = 0; j < PT_ITEMS; ++j)
            if ((ok >> j) & 1u) atomicAdd(&s_f[q[j]], 1u);
        t = t2;
    }
    lds_barrier();
    for (uint32_t d = threadIdx.x; d < NB; d += PT_THREADS) {
        uint32_t c = s_f[d];
        if (c) atomicAdd(&fine[d], c);
    }
    if (xcd_tpg) {
        const uint32_t F2 = 1u << b2;
        for (uint32_t d1 = threadIdx.x; d1 <= m1; d1 += PT_THREADS) {
            uint32_t sum = 0;
            // (rotated start: the threads of a wave do not all hit the same LDS bank)
            for (uint32_t i = 0; i < F2; ++i) sum += s_f[d1 * F2 + ((i + d1) & m2)];
            if (sum) atomicAdd(&coarse_x[(d1 << 3) | x], sum);
        }
    }
}

// Exclusive scan of the fine histogram, one workgroup per pass-1 digit: the workgroup sums
// everything below its F2 bins (coalesced, the whole histogram is 128 KiB of L2), scans its
// own bins on top, and with that writes the pass-2 offsets/cursors of its segment and the
// pass-1 offset/cursor of its digit — one launch instead of a serial walk over 2^15 bins.
__global__ __launch_bounds__(PT_MAXF) void k_scan_fine(const uint32_t* fine, uint32_t F1,
                                                       uint32_t F2, uint32_t* off2,
                                                       uint32_t* cursor2, uint32_t* off1,
                                                       uint32_t* cursor1, const uint32_t* coarse_x) {
    __shared__ uint32_t s_wsum[PT_MAXF / 64];
    const uint32_t      d1 = blockIdx.x, below = d1 * F2;
    uint32_t            sum = 0;
    if ((F2 & 3u) == 0) {  // 16 bytes per load (hipMalloc'd, so `fine` is 16-byte aligned)
        const uint4* f4 = reinterpret_cast<const uint4*>(fine);
        for (uint32_t i = threadIdx.x; i < below / 4; i += PT_MAXF) {
            const uint4 v = f4[i];
            sum += v.x + v.y + v.z + v.w;
        }
    } else {
        for (uint32_t i = threadIdx.x; i < below; i += PT_MAXF) sum += fine[i];
    }
    uint32_t base, tot;
    (void)block_excl_scan(sum, s_wsum, base);
    lds_barrier();
    const uint32_t v = threadIdx.x < F2 ? fine[below + threadIdx.x] : 0u;
    const uint32_t ex = block_excl_scan(v, s_wsum, tot);
    if (threadIdx.x < F2) {
        off2[below + threadIdx.x] = base + ex;
        cursor2[below + threadIdx.x] = base + ex;
    }
    if (threadIdx.x == 0) {
        off1[d1] = base;
        if (coarse_x) {  // eight sub-ranges (one per XCD) one behind the other: cursor1[d1 * 8 + x]
            uint32_t at = base;
            for (uint32_t x = 0; x < 8; ++x) {
                cursor1[(d1 << 3) | x] = at;
                at += coarse_x[(d1 << 3) | x];
            }
        } else {
            cursor1[d1] = base;
        }
        if (d1 + 1 == F1) {
            off1[F1] = base + tot;
            off2[(size_t)F1 * F2] = base + tot;
        }
    }
}

// Ranking and positions of a tile where k_pass_scatter takes them branch-free (BATCHED there), so a thread's
// PT_ITEMS LDS operations are issued together and waited for once (an exec-masked block per item made
// them PT_ITEMS serial round trips), and both need the key words only: with a loader that issues the
// key loads first, the carry loads are still in flight behind them.
// rank_tile: every tuple takes its rank inside its digit from an LDS atomic add.  An item that holds
// no tuple (ok bit clear: past the end of a partial tile, NULL key) adds to a dummy counter behind the
// real ones instead of taking a branch; PT_DUMMY of them, by lane, so that a run of such items does
// not serialise a wave on one LDS address.  Ranks are kept two per register.
template <int NW>
__device__ __forceinline__ void rank_tile(const PassParams& pp, uint32_t mask, uint32_t ok,
                                          const uint32_t (&w)[PT_ITEMS][NW], uint32_t* s_cnt,
                                          uint32_t (&rk)[PT_ITEMS / 2]) {
    const uint32_t dummy = PT_MAXF + (threadIdx.x & (PT_DUMMY - 1));
    uint32_t       r[PT_ITEMS];
#pragma unroll
    for (int j = 0; j < PT_ITEMS; ++j) {
        const uint32_t m = 0u - ((ok >> j) & 1u);  // a bit select, not ?: (which compiles to a branch around the digit)
        r[j] = atomicAdd(&s_cnt[(pass_digit(pp, w[j][0], mask) & m) | (dummy & ~m)], 1u);
    }
#pragma unroll
    for (int j = 0; j < PT_ITEMS; j += 2)
        rk[j / 2] = (r[j] & PT_RANK_MASK) | ((r[j + 1] & PT_RANK_MASK) << 16);
}
// place_tile: ranks -> LDS positions (start of the digit in the sorted tile + rank), in place and two per
// register; PT_NO_POS, which no position reaches, for an item without a tuple.  The digit is recomputed
// from the key word.
constexpr uint32_t PT_NO_POS = 0xffffu;
template <int NW>
__device__ __forceinline__ void place_tile(const PassParams& pp, uint32_t mask, uint32_t ok,
                                           const uint32_t (&w)[PT_ITEMS][NW], const uint32_t* s_base,
                                           uint32_t (&rk)[PT_ITEMS / 2]) {
    uint32_t b[PT_ITEMS];
#pragma unroll
    for (int j = 0; j < PT_ITEMS; ++j) b[j] = s_base[pass_digit(pp, w[j][0], mask)];
#pragma unroll
    for (int j = 0; j < PT_ITEMS; j += 2) {
        const uint32_t p0 = ((ok >> j) & 1u) ? b[j] + (rk[j / 2] & 0xffffu) : PT_NO_POS;
        const uint32_t p1 = ((ok >> (j + 1)) & 1u) ? b[j + 1] + (rk[j / 2] >> 16) : PT_NO_POS;
        rk[j / 2] = p0 | (p1 << 16);
    }
}
__device__ __forceinline__ uint32_t tile_pos(const uint32_t (&ps)[PT_ITEMS / 2], int j) {
    return (j & 1) ? ps[j / 2] >> 16 : ps[j / 2] & 0xffffu;
}

// (the shared scatter bodies name the last pass' cursor and limit arrays through these, so that their SPEC_LAST
// branch, which the other kernels discard, is well-formed with either parameter struct.  The SpecParams overloads
// are never called: a kernel whose `sp` is a SpecParams has SPEC_LAST = false.  The other direction is
// LastParams::cursor, rj_device.hpp)
__device__ __forceinline__ uint32_t*       last_cursor(const LastParams& p) { return p.cursor32; }
__device__ __forceinline__ uint32_t*       last_cursor(const SpecParams&) { return nullptr; }
__device__ __forceinline__ const uint32_t* last_limit(const LastParams& p) { return p.limit; }
__device__ __forceinline__ const uint32_t* last_limit(const SpecParams&) { return nullptr; }

template <class L>
struct is_src_loader : std::false_type {};
template <int KW, int CW, int WIDE>
struct is_src_loader<SrcLoader<KW, CW, WIDE>> : std::true_type {};

// ================================================================ K4 scatter
// Scatter half of the radix partition (reference counterpart: the serial
// scatter src/execute.cpp:175-184).  Per tile of PT_TILE (16384) tuples:
//   1. every tuple takes its rank inside its digit from an LDS atomic add (rank_tile);
//   2. the digit counters are scanned (wave shuffles) into LDS positions;
//   3. per word array the tile is written to LDS in digit order, then copied out
//      so that consecutive lanes write consecutive addresses of one digit's run
//      (software write-combining: HBM sees contiguous runs, not 4-byte scatters).
// Every tile reserves its output ranges with one atomic per digit (cursor = start of the
// digit's partition, from the scanned histogram).
// Steps 1 and 2 and the reservation need the key words only.  In the first pass of a key + two-word-carry
// plan (SrcLoader issues the key loads first) they run while the tile's carry loads, two thirds of its
// bytes, are in flight; the carries are waited for where they are staged.
// PAIR >= 0: words PAIR and PAIR+1 (a two-word carry) are written as 8-byte pairs into ONE array,
// out.w[PAIR] — one output stream and one staging round less than two word arrays.
// AOS (NW == 3, PAIR == 1: key + two-word carry, the LAST pass of a plan): the output is ONE array
// of 12-byte {hashed key, carry lo, carry hi} tuples instead of a key array plus a pair array —
// one output stream whose runs are 12 bytes per tuple long (a 32-tuple run is 384 contiguous
// bytes instead of 128 + 256 in two places), and the join reads one stream.  The tile is staged
// in two halves by sorted position (8192 tuples = 96 KiB of LDS each), so the runs are still
// those of the whole 16384-tuple tile.
// (Prefetching the next tile's loads behind the second half's staging lost at 1 B rows, pass 1
// 10.4-11.3 -> 12.0 ms: a burst of loads next to the copy-out's stores only gets in their way.
// Taken out again; profiles/r03_h_scatter_tile_prefetch_ab.log is the record.)
// SPEC (k_spec_scatter, the speculative first pass: SpecParams): a digit's run is reserved from the 64-bit
// {position, room} cursor of its sub-range; a run that does not fit raises sp.flag and goes, with the unchanged
// copy-out, to the spare tile at sp.sink — inside the allocation and in nobody's sub-range.  Kernels of their
// own names (the exact ones keep theirs, their arguments and their machine code); both include the one body,
// rj_pass_scatter.inc, with SPEC as a constant.
template <int NW, class Loader, int PAIR, bool AOS>
__global__ __launch_bounds__(PT_THREADS) void k_pass_scatter(Loader ld, PassParams pp, Words out) {
    constexpr bool       SPEC = false, SPEC_LAST = false;
    constexpr SpecParams sp{};
#include "rj_pass_scatter.inc"
}
template <int NW, class Loader, int PAIR>
__global__ __launch_bounds__(PT_THREADS) void k_spec_scatter(Loader ld, PassParams pp, Words out, SpecParams sp) {
    constexpr bool SPEC = true, SPEC_LAST = false, AOS = false;
#include "rj_pass_scatter.inc"
}

// Packed variant for {hashed key, one carry word} tuples (the BASELINE shape): the tile is
// staged as 8-byte pairs (128 KiB of LDS — the workgroup owns the CU anyway) and copied out
// with one 8-byte store per tuple into ONE output array.  Against two word arrays this
// halves the number of output streams and doubles the bytes per contiguous run (a run of 64
// tuples is 512 contiguous bytes instead of two runs of 256), which is what the scatter's
// rate follows; it also needs one staging round and two barriers less per tile.
template <class Loader, bool BLK_OUT = false>
__global__ __launch_bounds__(PT_THREADS) void k_pass_scatter_packed(Loader ld, PassParams pp, uint2* out) {
    constexpr bool       SPEC = false, SPEC_LAST = false;
    constexpr SpecParams sp{};
#include "rj_pass_scatter_packed.inc"
}
// (the speculative first pass: see k_spec_scatter)
template <class Loader, bool BLK_OUT>
__global__ __launch_bounds__(PT_THREADS) void k_spec_scatter_packed(Loader ld, PassParams pp, uint2* out, SpecParams sp) {
    constexpr bool SPEC = true, SPEC_LAST = false;
#include "rj_pass_scatter_packed.inc"
}

// ================================================== speculative last pass: sample, capacities, scatter, closing
// (rj_device.hpp: LastParams.  Kernels of their own family names, k_last_*: every exact kernel and every kernel of
// the speculative first pass keeps its name, its arguments and its machine code.)
// k_last_sample: k_pass_hist of a later pass — its grid, a group table (of its own, see sample_last in rj_radix.hip), xcd_remap
// and LDS bins — over the input segments a speculative first pass left behind, but of every tile only one slice of PT_TILE >> sample_log2
// consecutive keys is read, four keys per 16-byte load.  The slice's place moves from tile to tile as in
// k_pass_sample; in a partial last tile of a segment it ends with the tile at the latest (its place is the
// largest multiple of four that allows it, so that the loads stay aligned), and a tile of no more rows than a
// slice is read whole.  Bin (oseg, d2) is sampled from exactly the rows that will be scattered into it: all
// tuples of an output segment come from its own eight input segments.  A load may reach up to three keys
// behind the segment's end (never behind the array's: the spare tile follows the sub-ranges); they are masked out.
__device__ __forceinline__ u32x4a sample_keys4(const DenseLoader& ld, uint32_t g) {
    return *reinterpret_cast<const u32x4a*>(ld.in.w[0] + g);
}
__device__ __forceinline__ u32x4a sample_keys4(const BlockedLoader& ld, uint32_t g) {  // (g % 4 == 0: one block)
    return *reinterpret_cast<const u32x4a*>(ld.in + BlockedLoader::key_at(g));
}
static_assert(BlockedLoader::BLK % 4 == 0, "four consecutive keys of a blocked array share a block");
template <class Loader>
__global__ __launch_bounds__(PT_THREADS) void k_last_sample(Loader ld, PassParams pp, LastParams sp) {
    __shared__ uint32_t s_h[PT_MAXF];
    uint32_t            seg, begin, end;
    if (!group_range(pp, blockIdx.x, seg, begin, end)) return;
    const uint32_t F = 1u << pp.fanout_log2, mask = F - 1u;
    for (uint32_t d = threadIdx.x; d < F; d += PT_THREADS) s_h[d] = 0;
    lds_barrier();
    const uint32_t slog = (uint32_t)__builtin_ctz((unsigned)PT_TILE) - sp.sample_log2, slice = 1u << slog;
    const uint32_t ntiles = (end - begin + (uint32_t)PT_TILE - 1u) / (uint32_t)PT_TILE;
    const uint32_t total = ntiles << (slog - 2u);  // units of four consecutive keys
    constexpr int  U = 4;                          // units a thread has in flight
    for (uint32_t i0 = threadIdx.x; i0 < total; i0 += U * PT_THREADS) {
        u32x4a   k[U];
        uint32_t nv[U];  // keys of the unit that count
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t i = i0 + u * PT_THREADS, ic = min(i, total - 1u);
            const uint32_t t = ic >> (slog - 2u), r = (ic & ((slice >> 2) - 1u)) << 2;
            const uint32_t tb = begin + t * (uint32_t)PT_TILE, rows = min((uint32_t)PT_TILE, end - tb);
            const uint32_t rot = ((tb / (uint32_t)PT_TILE) * 7u << slog) & ((uint32_t)PT_TILE - 1u);
            const uint32_t at = rows > slice ? min(rot, (rows - slice) & ~3u) : 0u;
            const uint32_t first = at + r;  // the unit's first row inside the tile
            k[u] = sample_keys4(ld, tb + min(first, (rows - 1u) & ~3u));
            nv[u] = (i < total && first < rows) ? min(4u, rows - first) : 0u;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if ((uint32_t)e < nv[u]) atomicAdd(&s_h[pass_digit(pp, k[u][e], mask)], 1u);
    }
    lds_barrier();
    for (uint32_t d = threadIdx.x; d < F; d += PT_THREADS) {
        uint32_t c = s_h[d];
        if (c) atomicAdd(&pp.hist[(size_t)seg * F + d], c);
    }
}

// Capacities of the final partitions from their sample counts — k_spec_caps' formula over up to 2^18 bins, so as
// a grid and a two-level scan: one workgroup per output segment (the F final partitions of a first-pass
// partition, which stay adjacent), thread d = digit d.  LEVEL 0 leaves the segment's sum of capacities in
// seg_sum[seg]; LEVEL 1 starts from the sum of the segments below and writes the exclusive scan — the partition's
// begin, into pairs[2 i] of the {begin, end} pairs — limit[] = begin + capacity and cursor[] = begin.  Nothing reaches beyond cap_max, the tuples the
// host made room for (radix_cap_bound, rj_radix_plan.cpp): a partition that would is cut there and overflows like any other.
template <int LEVEL>
__global__ __launch_bounds__(PT_MAXF) void k_last_caps(const uint32_t* sample, uint32_t nseg, uint32_t F, uint32_t sample_log2,
                                                       float z, uint32_t cap_max, unsigned long long* seg_sum,
                                                       uint32_t* pairs, uint32_t* limit, uint32_t* cursor) {
    __shared__ unsigned long long s_sum[PT_MAXF];
    const uint32_t                seg = blockIdx.x, d = threadIdx.x;
    const size_t                  i = (size_t)seg * F + d;
    unsigned long long            cap = 0;
    if (d < F) {
        const double zz = (double)z, x = (double)sample[i] + zz * sqrt((double)sample[i] + 1.0) + 0.5 * zz * zz;
        cap = ((unsigned long long)ceil(ldexp(x, (int)sample_log2)) + 31ull) & ~31ull;
    }
    s_sum[d] = cap;
    __syncthreads();
    if constexpr (LEVEL == 0) {
        if (d == 0) {
            unsigned long long sum = 0;
            for (uint32_t k = 0; k < F; ++k) sum += s_sum[k];
            seg_sum[seg] = sum;
        }
    } else {
        unsigned long long run = 0;
        for (uint32_t k = 0; k < d && k < F; ++k) run += s_sum[k];
        __syncthreads();
        unsigned long long below = 0;  // the segments below this one
        for (uint32_t k = d; k < seg; k += PT_MAXF) below += seg_sum[k];
        s_sum[d] = below;
        __syncthreads();
        for (uint32_t k = 0; k < (uint32_t)PT_MAXF; ++k) run += s_sum[k];
        if (d < F) {
            const uint32_t st = (uint32_t)min(run, (unsigned long long)cap_max);
            const uint32_t lim = (uint32_t)min(run + cap, (unsigned long long)cap_max);
            pairs[2 * i] = st;
            limit[i] = lim;
            cursor[i] = st;
        }
    }
}

// (k_pass_scatter's and k_pass_scatter_packed's bodies with the speculative switch, for the LAST pass: 12-byte
// tuples out of the dense key array + pair array, pairs out of blocked pairs)
template <int NW, class Loader, int PAIR>
__global__ __launch_bounds__(PT_THREADS) void k_last_scatter(Loader ld, PassParams pp, Words out, LastParams sp) {
    constexpr bool SPEC = true, SPEC_LAST = true, AOS = true;
#include "rj_pass_scatter.inc"
}
template <class Loader>
__global__ __launch_bounds__(PT_THREADS) void k_last_scatter_packed(Loader ld, PassParams pp, uint2* out, LastParams sp) {
    constexpr bool SPEC = true, SPEC_LAST = true, BLK_OUT = false;
#include "rj_pass_scatter_packed.inc"
}

// Closing the pass: final partition q holds [begin[q], end[q]), end = min(where its cursor stands, its limit), next
// to begin in the pairs.  Nothing is compacted: the join skips the unused room behind a partition.
__global__ __launch_bounds__(256) void k_last_close(const uint32_t* cursor, const uint32_t* limit, uint32_t nbins,
                                                    uint32_t* pairs) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < nbins) pairs[2 * (size_t)i + 1] = min(cursor[i], limit[i]);
}

// ============================================================= heavy task list
// Probe partitions above JN_HEAVY tuples are cut into tasks so that a skewed
// (Zipf) probe side does not serialise on one workgroup; each task rebuilds the
// (small) build table of its partition.
// (off_pairs: JoinParams' — neighbouring offsets, or {begin, end} pairs behind a speculative last pass)
__global__ void k_heavy_tasks(const uint32_t* offR, const uint32_t* offS, uint32_t NP,
                              uint32_t* tasks, uint32_t* n_heavy, uint32_t max_tasks, uint32_t off_pairs) {
    uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= NP) return;
    const uint32_t ir = q << (off_pairs & 1u), is = q << (off_pairs >> 1);
    uint32_t sb = offS[is], se = offS[is + 1];
    uint32_t len = se - sb;
    if (len <= JN_HEAVY || offR[ir + 1] == offR[ir]) return;
    uint32_t nt = (len + JN_HEAVY - 1) / JN_HEAVY;
    uint32_t b = atomicAdd(n_heavy, nt);
    for (uint32_t t = 0; t < nt; ++t) {
        uint32_t k = b + t;
        if (k >= max_tasks) break;  // cannot happen: max_tasks >= 2*|S|/JN_HEAVY + 1
        tasks[3 * k + 0] = q;
        // bounds in 64 bits: a partition ending within JN_HEAVY of 2^32 must not wrap
        tasks[3 * k + 1] = (uint32_t)((uint64_t)sb + (uint64_t)t * JN_HEAVY);
        tasks[3 * k + 2] = (uint32_t)min((uint64_t)se, (uint64_t)sb + (uint64_t)(t + 1) * JN_HEAVY);
    }
}

// ================================================================== launchers
void launch_scan_bins(const Launch& L, const uint32_t* in, uint32_t n, uint32_t* off,
                      uint32_t* cursor) {
    RJ_KLAUNCH(L, "scan_bins", (k_scan_bins<0>), 1, 1024, in, (const uint32_t*)nullptr, n, 1u, off, cursor);
}

void launch_scan_segments(const Launch& L, const uint32_t* hist, const uint32_t* seg_off,
                          uint32_t nseg, uint32_t F, uint32_t xcd_log2, uint32_t* off, uint32_t* cursor) {
    RJ_KLAUNCH(L, "scan_segments", k_scan_segments, nseg, PT_MAXF, hist, seg_off, nseg, F, xcd_log2, off,
               cursor);
}

void launch_group_table(const Launch& L, const uint32_t* seg_off, uint32_t nseg,
                        uint32_t group_tuples, uint32_t* grp_start, const uint32_t* seg_end) {
    RJ_KLAUNCH(L, "group_table", (k_scan_bins<1>), 1, 1024, seg_off, seg_end, nseg, group_tuples, grp_start,
               (uint32_t*)nullptr);
}

void launch_pass_hist_src(const Launch& L, const TupleSrc& src, int key_words, const PassParams& pp,
                          uint32_t n_groups) {
    if (!n_groups) return;
    if (key_words == 1) {
        SrcLoader<1, 0> ld{src};
        RJ_KLAUNCH(L, "pass1_hist", (k_pass_hist<SrcLoader<1, 0>>), n_groups, PT_THREADS, ld, pp);
    } else {
        SrcLoader<2, 0> ld{src};
        RJ_KLAUNCH(L, "pass1_hist", (k_pass_hist<SrcLoader<2, 0>>), n_groups, PT_THREADS, ld, pp);
    }
}

void launch_pass_sample_src(const Launch& L, const TupleSrc& src, int key_words, const PassParams& pp,
                            const SpecParams& sp, uint32_t n_groups) {
    if (!n_groups) return;
    if (key_words == 1)
        RJ_KLAUNCH(L, "pass1_sample", (k_pass_sample<1>), n_groups, PT_THREADS, src, pp, sp);
    else
        RJ_KLAUNCH(L, "pass1_sample", (k_pass_sample<2>), n_groups, PT_THREADS, src, pp, sp);
}

void launch_spec_caps(const Launch& L, const uint32_t* sample, uint32_t nbins, uint32_t sample_log2, float z,
                      uint32_t cap_max, uint32_t* start, uint32_t* limit, unsigned long long* cursor) {
    RJ_KLAUNCH(L, "spec_caps", k_spec_caps, 1, 1024, sample, nbins, sample_log2, z, cap_max, start, limit, cursor);
}

void launch_spec_close(const Launch& L, const unsigned long long* cursor, const uint32_t* start, const uint32_t* limit,
                       uint32_t F, uint32_t* seg_end, uint32_t* oseg_off) {
    RJ_KLAUNCH(L, "spec_close", k_spec_close, 1, PT_MAXF, cursor, start, limit, F, seg_end, oseg_off);
}

void launch_fine_hist_src(const Launch& L, const TupleSrc& src, int key_words, uint32_t shift,
                          uint32_t b1, uint32_t b2, uint32_t grid, uint32_t* fine, uint32_t xcd_tpg,
                          uint32_t* coarse_x) {
    if (!grid || !src.n_rows) return;
    if (key_words == 1) {
        SrcLoader<1, 0> ld{src};
        RJ_KLAUNCH(L, "pass1_hist", (k_fine_hist<SrcLoader<1, 0>>), grid, PT_THREADS, ld, src.n_rows,
                   shift, b1, b2, fine, xcd_tpg, coarse_x);
    } else {
        SrcLoader<2, 0> ld{src};
        RJ_KLAUNCH(L, "pass1_hist", (k_fine_hist<SrcLoader<2, 0>>), grid, PT_THREADS, ld, src.n_rows,
                   shift, b1, b2, fine, xcd_tpg, coarse_x);
    }
}

void launch_fine_hist_words(const Launch& L, const Words& in, bool packed, uint32_t n, uint32_t shift,
                            uint32_t b1, uint32_t b2, uint32_t grid, uint32_t* fine, uint32_t xcd_tpg,
                            uint32_t* coarse_x) {
    if (!grid || !n) return;
    if (packed) {
        PackedLoader ld{reinterpret_cast<const uint2*>(in.w[0])};
        RJ_KLAUNCH(L, "pass1_hist", (k_fine_hist<PackedLoader>), grid, PT_THREADS, ld, n, shift, b1, b2, fine,
                   xcd_tpg, coarse_x);
    } else {
        DenseLoader ld{in};
        RJ_KLAUNCH(L, "pass1_hist", (k_fine_hist<DenseLoader>), grid, PT_THREADS, ld, n, shift, b1, b2, fine,
                   xcd_tpg, coarse_x);
    }
}

void launch_scan_fine(const Launch& L, const uint32_t* fine, uint32_t F1, uint32_t F2,
                      uint32_t* off2, uint32_t* cursor2, uint32_t* off1, uint32_t* cursor1,
                      const uint32_t* coarse_x) {
    RJ_KLAUNCH(L, "scan_fine", k_scan_fine, F1, PT_MAXF, fine, F1, F2, off2, cursor2, off1, cursor1,
               coarse_x);
}

// (carries of two or more words: the last two travel as one array of 8-byte pairs)
template <int KW, int CW, int WIDE = WIDE_NONE>
static void scatter_src_t(const Launch& L, const TupleSrc& src, const PassParams& pp,
                          uint32_t n_groups, const Words& out, const SpecParams* spec) {
    SrcLoader<KW, CW, WIDE> ld{src};
    if (spec) {
        RJ_KLAUNCH(L, "pass1_scatter", (k_spec_scatter<KW + CW, SrcLoader<KW, CW, WIDE>, (CW >= 2 ? KW + CW - 2 : -1)>),
                   n_groups, PT_THREADS, ld, pp, out, *spec);
        return;
    }
    RJ_KLAUNCH(L, "pass1_scatter", (k_pass_scatter<KW + CW, SrcLoader<KW, CW, WIDE>, (CW >= 2 ? KW + CW - 2 : -1), false>),
               n_groups, PT_THREADS, ld, pp, out);
}

void launch_pass_scatter_src(const Launch& L, const TupleSrc& src, int key_words, int carry_words,
                             const PassParams& pp, uint32_t n_groups, const Words& out, bool aos3, const SpecParams* spec) {
    if (!n_groups) return;
    const int wide = src.carry_mode == CARRY_WIDE ? src.wide : WIDE_NONE;
    if (aos3) {
        if (spec) launch_failed("pass1_scatter", "no speculative kernel writes 12-byte tuples", true);
        if (key_words != 1 || carry_words != 2) launch_failed("pass1_scatter", "12-byte tuples need KW=1, CW=2", true);
        if (wide == WIDE_32S) {
            SrcLoader<1, 2, WIDE_32S> ld{src};
            RJ_KLAUNCH(L, "pass1_scatter", (k_pass_scatter<3, SrcLoader<1, 2, WIDE_32S>, 1, true>), n_groups, PT_THREADS, ld, pp, out);
            return;
        }
        SrcLoader<1, 2> ld{src};
        RJ_KLAUNCH(L, "pass1_scatter", (k_pass_scatter<3, SrcLoader<1, 2>, 1, true>), n_groups, PT_THREADS, ld, pp, out);
        return;
    }
    if (wide != WIDE_NONE) {
        switch (key_words * 100 + carry_words * 10 + wide) {
        case 121: scatter_src_t<1, 2, WIDE_32S>(L, src, pp, n_groups, out, spec); break;
        case 131: scatter_src_t<1, 3, WIDE_32S>(L, src, pp, n_groups, out, spec); break;
        case 132: scatter_src_t<1, 3, WIDE_64_32>(L, src, pp, n_groups, out, spec); break;
        case 221: scatter_src_t<2, 2, WIDE_32S>(L, src, pp, n_groups, out, spec); break;
        default: launch_failed("pass1_scatter", "no kernel for this wide carry layout", true);
        }
        return;
    }
    for_shape("pass1_scatter", key_words, carry_words, [&](auto KW, auto CW) {
        if constexpr (CW <= 2)  // (three carry words travel only as a wide carry, above)
            scatter_src_t<KW, CW>(L, src, pp, n_groups, out, spec);
        else
            launch_failed("pass1_scatter", "no kernel for this key/carry word count", true);
    });
}

void launch_pass_hist_dense(const Launch& L, const Words& in, const PassParams& pp,
                            uint32_t n_groups) {
    if (!n_groups) return;
    DenseLoader ld{in};
    RJ_KLAUNCH(L, "pass2_hist", (k_pass_hist<DenseLoader>), n_groups, PT_THREADS, ld, pp);
}

void launch_pass_scatter_dense(const Launch& L, const Words& in, int n_words, int pair_word,
                               const PassParams& pp, uint32_t n_groups, const Words& out, bool aos3) {
    if (!n_groups) return;
    if (aos3) {
        if (n_words != 3 || pair_word != 1) launch_failed("pass2_scatter", "12-byte tuples need KW=1, CW=2", true);
        RJ_KLAUNCH(L, "pass2_scatter", (k_pass_scatter<3, DenseLoaderT<1>, 1, true>), n_groups, PT_THREADS,
                   DenseLoaderT<1>{in}, pp, out);
        return;
    }
    switch (n_words * 10 + (pair_word < 0 ? 9 : pair_word)) {
    case 19:
        RJ_KLAUNCH(L, "pass2_scatter", (k_pass_scatter<1, DenseLoader, -1, false>), n_groups, PT_THREADS,
                   DenseLoader{in}, pp, out);
        break;
    case 29:
        RJ_KLAUNCH(L, "pass2_scatter", (k_pass_scatter<2, DenseLoader, -1, false>), n_groups, PT_THREADS,
                   DenseLoader{in}, pp, out);
        break;
    case 39:
        RJ_KLAUNCH(L, "pass2_scatter", (k_pass_scatter<3, DenseLoader, -1, false>), n_groups, PT_THREADS,
                   DenseLoader{in}, pp, out);
        break;
    case 31:  // key + carry pair
        RJ_KLAUNCH(L, "pass2_scatter", (k_pass_scatter<3, DenseLoaderT<1>, 1, false>), n_groups, PT_THREADS,
                   DenseLoaderT<1>{in}, pp, out);
        break;
    case 42:  // two key words + carry pair
        RJ_KLAUNCH(L, "pass2_scatter", (k_pass_scatter<4, DenseLoaderT<2>, 2, false>), n_groups, PT_THREADS,
                   DenseLoaderT<2>{in}, pp, out);
        break;
    default: launch_failed("pass2_scatter", "no kernel for this word layout", true);
    }
}

void launch_pass_hist_digits(const Launch& L, const uint16_t* digits, const PassParams& pp, uint32_t n_groups) {
    if (!n_groups) return;
    DigitLoader ld{digits, pp.shift};
    RJ_KLAUNCH(L, "pass2_hist", (k_pass_hist<DigitLoader>), n_groups, PT_THREADS, ld, pp);
}

void launch_pass_hist_aos3(const Launch& L, const uint32_t* in_tuples, const PassParams& pp, uint32_t n_groups) {
    if (!n_groups) return;
    RJ_KLAUNCH(L, "pass2_hist", (k_pass_hist<Aos3KeyLoader>), n_groups, PT_THREADS, Aos3KeyLoader{in_tuples}, pp);
}

void launch_pass_scatter_aos3(const Launch& L, const uint32_t* in_tuples, const PassParams& pp, uint32_t n_groups,
                              uint32_t* out_tuples) {
    if (!n_groups) return;
    Words out{};
    out.w[0] = out_tuples;
    RJ_KLAUNCH(L, "pass2_scatter", (k_pass_scatter<3, Aos3Loader, 1, true>), n_groups, PT_THREADS,
               Aos3Loader{in_tuples}, pp, out);
}

void launch_pass_hist_packed(const Launch& L, const uint32_t* in_pairs, const PassParams& pp,
                             uint32_t n_groups) {
    if (!n_groups) return;
    PackedLoader ld{reinterpret_cast<const uint2*>(in_pairs)};
    RJ_KLAUNCH(L, "pass2_hist", (k_pass_hist<PackedLoader>), n_groups, PT_THREADS, ld, pp);
}

void launch_pass_scatter_src_packed(const Launch& L, const TupleSrc& src, const PassParams& pp,
                                    uint32_t n_groups, uint32_t* out_pairs, bool blocked_out, const SpecParams* spec) {
    if (!n_groups) return;
    SrcLoader<1, 1> ld{src};
    if (spec) {
        if (blocked_out)
            RJ_KLAUNCH(L, "pass1_scatter", (k_spec_scatter_packed<SrcLoader<1, 1>, true>), n_groups, PT_THREADS, ld,
                       pp, reinterpret_cast<uint2*>(out_pairs), *spec);
        else
            RJ_KLAUNCH(L, "pass1_scatter", (k_spec_scatter_packed<SrcLoader<1, 1>, false>), n_groups, PT_THREADS, ld,
                       pp, reinterpret_cast<uint2*>(out_pairs), *spec);
        return;
    }
    if (blocked_out)
        RJ_KLAUNCH(L, "pass1_scatter", (k_pass_scatter_packed<SrcLoader<1, 1>, true>), n_groups, PT_THREADS, ld,
                   pp, reinterpret_cast<uint2*>(out_pairs));
    else
        RJ_KLAUNCH(L, "pass1_scatter", (k_pass_scatter_packed<SrcLoader<1, 1>>), n_groups, PT_THREADS, ld,
                   pp, reinterpret_cast<uint2*>(out_pairs));
}

// a later pass over BLOCKED pairs (see BlockedLoader); its output is blocked again, or — the last pass — packed
void launch_pass_hist_blocked(const Launch& L, const uint32_t* in_blocked, const PassParams& pp, uint32_t n_groups) {
    if (!n_groups) return;
    RJ_KLAUNCH(L, "pass2_hist", (k_pass_hist<BlockedLoader>), n_groups, PT_THREADS, BlockedLoader{in_blocked}, pp);
}
void launch_pass_scatter_blocked(const Launch& L, const uint32_t* in_blocked, const PassParams& pp, uint32_t n_groups,
                                 uint32_t* out_pairs, bool blocked_out) {
    if (!n_groups) return;
    BlockedLoader ld{in_blocked};
    if (blocked_out)
        RJ_KLAUNCH(L, "pass2_scatter", (k_pass_scatter_packed<BlockedLoader, true>), n_groups, PT_THREADS, ld, pp,
                   reinterpret_cast<uint2*>(out_pairs));
    else
        RJ_KLAUNCH(L, "pass2_scatter", (k_pass_scatter_packed<BlockedLoader>), n_groups, PT_THREADS, ld, pp,
                   reinterpret_cast<uint2*>(out_pairs));
}

void launch_pass_scatter_packed(const Launch& L, const uint32_t* in_pairs, const PassParams& pp,
                                uint32_t n_groups, uint32_t* out_pairs) {
    if (!n_groups) return;
    PackedLoader ld{reinterpret_cast<const uint2*>(in_pairs)};
    RJ_KLAUNCH(L, "pass2_scatter", (k_pass_scatter_packed<PackedLoader>), n_groups, PT_THREADS, ld, pp,
               reinterpret_cast<uint2*>(out_pairs));
}

void launch_last_sample(const Launch& L, const uint32_t* in_keys, bool blocked, const PassParams& pp, const LastParams& sp,
                        uint32_t n_groups) {
    if (!n_groups) return;
    if (blocked) {
        RJ_KLAUNCH(L, "pass2_sample", (k_last_sample<BlockedLoader>), n_groups, PT_THREADS, BlockedLoader{in_keys}, pp, sp);
    } else {
        Words in{};
        in.w[0] = const_cast<uint32_t*>(in_keys);
        RJ_KLAUNCH(L, "pass2_sample", (k_last_sample<DenseLoader>), n_groups, PT_THREADS, DenseLoader{in}, pp, sp);
    }
}

void launch_last_caps(const Launch& L, const uint32_t* sample, uint32_t nseg, uint32_t F, uint32_t sample_log2, float z,
                      uint32_t cap_max, unsigned long long* seg_sum, uint32_t* pairs, uint32_t* limit,
                      uint32_t* cursor) {
    RJ_KLAUNCH(L, "last_caps", (k_last_caps<0>), nseg, PT_MAXF, sample, nseg, F, sample_log2, z, cap_max, seg_sum, pairs,
               limit, cursor);
    RJ_KLAUNCH(L, "last_caps", (k_last_caps<1>), nseg, PT_MAXF, sample, nseg, F, sample_log2, z, cap_max, seg_sum, pairs,
               limit, cursor);
}

void launch_last_scatter_dense(const Launch& L, const Words& in, const PassParams& pp, uint32_t n_groups, const Words& out,
                               const LastParams& sp) {
    if (!n_groups) return;
    RJ_KLAUNCH(L, "pass2_scatter", (k_last_scatter<3, DenseLoaderT<1>, 1>), n_groups, PT_THREADS, DenseLoaderT<1>{in}, pp, out,
               sp);
}

void launch_last_scatter_blocked(const Launch& L, const uint32_t* in_blocked, const PassParams& pp, uint32_t n_groups,
                                 uint32_t* out_pairs, const LastParams& sp) {
    if (!n_groups) return;
    RJ_KLAUNCH(L, "pass2_scatter", (k_last_scatter_packed<BlockedLoader>), n_groups, PT_THREADS, BlockedLoader{in_blocked}, pp,
               reinterpret_cast<uint2*>(out_pairs), sp);
}

void launch_last_close(const Launch& L, const uint32_t* cursor, const uint32_t* limit, uint32_t nbins,
                       uint32_t* pairs) {
    RJ_KLAUNCH(L, "last_close", k_last_close, (nbins + 255u) / 256u, 256, cursor, limit, nbins, pairs);
}

void launch_heavy_tasks(const Launch& L, const uint32_t* offR, const uint32_t* offS, uint32_t NP,
                        uint32_t* tasks, uint32_t* n_heavy, uint32_t max_tasks, uint32_t off_pairs) {
    RJ_KLAUNCH(L, "heavy_tasks", k_heavy_tasks, (NP + 255) / 256, 256, offR, offS, NP, tasks,
               n_heavy, max_tasks, off_pairs);
}

// RJ_CTX_PREWARM: one harmless launch, so that HIP loads this translation unit's code object when the context is
// built (as prewarm_varchar_dev does).  NP = 0: every thread of k_heavy_tasks leaves at `q >= NP`, its first check,
// before any pointer is read.
void prewarm_partition(const Launch& L, uint32_t* zeroed) {
    RJ_KLAUNCH(L, "prewarm", k_heavy_tasks, 1, 256, zeroed, zeroed, 0u, zeroed, zeroed, 0u, 0u);
}

}  // namespace rj
