// rj_kernels.hip — hand-written gfx950 (CDNA4, wave64) kernels of the radix join.
//
// Everything here is integer / indexing work bound by HBM bandwidth (no MFMA):
//   K0  page headers        4 B read per 8 KiB page
//   K1  page decode         irregular (NULL-bearing) pages -> dense values + validity
//   K2  pass histogram      per-workgroup LDS histogram, flushed once per tile group
//   K3  bin scan            one workgroup per input segment, wave-shuffle scan
//   K4  pass scatter        tile of 16384 tuples sorted by digit in LDS (LDS atomics give the
//                           rank), runs written out contiguously = software write-combining
//   K5/6 build + probe      per-partition bucketised hash table in LDS (one 16-byte read per
//                           probe), ballot/mbcnt output offsets, one global reservation per
//                           4096 probe tuples, streams written straight into Page images
//                           (partitioned: rj_join.hip; the broadcast form is here)
//   K7  gather              row-id -> column value (generic late materialisation)
//   K8  page finish/encode  Page headers + validity bitmaps of the result
//
// Reference counterparts are cited at each kernel (paths relative to the reference).
#include <hip/hip_ext.h>

#include "rj_kernels.hpp"
#include "rj_kernel_util.hpp"
#include "rj_tuple_util.hpp"

#include <algorithm>
#include <type_traits>

namespace rj {

// ================================================================= K0 headers
// One wave per page: reads `u16 n_rows @0` and the validity bitmap in the last
// (n_rows+7)/8 bytes (layout: reference src/build_table.cpp:326-331).  A column is
// "regular" when every page but the last holds exactly rows_full rows and every bitmap bit
// of every page is set; regular columns are addressed in place by every later kernel, the
// others go through K1 once.  The reference decodes fixed-width pages from the bitmap alone
// and never reads the header's non-null count (:332-343), so neither does this.
__global__ __launch_bounds__(256) void k_page_headers(const uint8_t* pages, uint32_t n_pages,
                                                      uint32_t rows_full, uint32_t* page_rows,
                                                      unsigned long long* flags) {
    // every workgroup walks a strip of pages (one wave per page at a time) and adds its two
    // sums with ONE pair of global atomics: a million pages must not queue on two words
    __shared__ unsigned long long s_irr[4], s_rows[4];
    const uint32_t     lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    unsigned long long irr = 0, rows = 0;
    for (uint32_t p = blockIdx.x * 4u + wid; p < n_pages; p += gridDim.x * 4u) {
        const uint8_t* page = pages + (size_t)p * PAGE_BYTES;
        const uint32_t nr = *reinterpret_cast<const uint16_t*>(page);
        const uint32_t nb = (nr + 7) / 8;
        const uint8_t* bm = page + PAGE_BYTES - nb;
        bool           ones = true;
        // full pages: 248 bitmap bytes at a dword boundary (INT32) or 126 at a halfword boundary
        // (INT64/FP64) — one load per lane; anything else byte by byte
        const uint32_t boff = PAGE_BYTES - nb;
        if ((nr & 31u) == 0 && (boff & 3u) == 0) {
            for (uint32_t k = lane; k < nb / 4; k += 64)
                ones = ones && reinterpret_cast<const uint32_t*>(bm)[k] == 0xffffffffu;
        } else if ((boff & 1u) == 0 && (nb & 1u) == 0) {
            for (uint32_t k = lane; k < nb / 2; k += 64) {
                const uint32_t rem = nr - k * 16u;
                const uint32_t want = rem >= 16 ? 0xffffu : ((1u << rem) - 1u);
                ones = ones && ((uint32_t)reinterpret_cast<const uint16_t*>(bm)[k] & want) == want;
            }
        } else {
            for (uint32_t k = lane; k < nb; k += 64) {
                const uint32_t rem = nr - k * 8u;
                const uint32_t want = rem >= 8 ? 0xffu : ((1u << rem) - 1u);
                ones = ones && ((bm[k] & want) == want);
            }
        }
        const bool all_ones = __ballot(!ones) == 0;
        if (lane == 0) {
            page_rows[p] = nr;
            irr += !all_ones || (p + 1 < n_pages ? nr != rows_full : (nr > rows_full || nr == 0));
            rows += nr;
        }
    }
    if (lane == 0) {
        s_irr[wid] = irr;
        s_rows[wid] = rows;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long i = s_irr[0] + s_irr[1] + s_irr[2] + s_irr[3];
        const unsigned long long r = s_rows[0] + s_rows[1] + s_rows[2] + s_rows[3];
        if (i) atomicAdd(&flags[0], i);
        if (r) atomicAdd(&flags[1], r);
    }
}

// "row_idx" rule of Table::from_columnar (reference src/build_table.cpp:334-336): the
// reference throws only when a NON-NULL value lands at a row index >= num_rows; NULL rows
// past the end are tolerated.  One wave per page; flag[0] counts offending pages.
__global__ __launch_bounds__(256) void k_rows_beyond(const uint8_t* pages, uint32_t n_pages,
                                                     const uint32_t* row_base, uint64_t num_rows,
                                                     unsigned long long* flag) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t p = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (p >= n_pages) return;
    const uint8_t* page = pages + (size_t)p * PAGE_BYTES;
    const uint32_t nr = *reinterpret_cast<const uint16_t*>(page);
    const uint64_t rb = row_base[p];
    if (rb + nr <= num_rows) return;
    const uint8_t* bm = page + PAGE_BYTES - (nr + 7) / 8;
    bool           bad = false;
    for (uint32_t i = lane; i < nr; i += 64)
        if (rb + i >= num_rows && ((bm[i >> 3] >> (i & 7u)) & 1u)) bad = true;
    if (__ballot(bad) != 0 && lane == 0) atomicAdd(flag, 1ull);
}

// ================================================================== K1 decode
// One workgroup per page: rows -> dense values + validity bytes.  The value
// index of row i is the number of set validity bits below i (values are stored
// densely, the bitmap sits in the last (n_rows+7)/8 bytes: reference
// src/build_table.cpp:325-381).  Per 64 rows one ballot + mbcnt.
template <int WIDTH>
__global__ __launch_bounds__(256) void k_decode_pages(const uint8_t* pages, const uint32_t* row_base,
                                                      uint64_t num_rows, uint8_t* values,
                                                      uint8_t* valid) {
    __shared__ uint32_t s_w[4];
    const uint8_t*      page = pages + (size_t)blockIdx.x * PAGE_BYTES;
    const uint32_t      nr = *reinterpret_cast<const uint16_t*>(page);
    const uint32_t      rb = row_base[blockIdx.x];
    const uint8_t*      bitmap = page + PAGE_BYTES - (nr + 7) / 8;
    const uint8_t*      vals = page + (WIDTH == 4 ? HDR32 : HDR64);
    const uint32_t      lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    uint32_t            running = 0;
    for (uint32_t base = 0; base < nr; base += 256) {
        uint32_t i = base + threadIdx.x;
        bool     bit = i < nr ? ((bitmap[i >> 3] >> (i & 7u)) & 1u) : false;
        uint64_t mask = __ballot(bit);
        uint32_t pre = lane_prefix(mask);
        if (lane == 0) s_w[wid] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t wpre = 0, tot = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            uint32_t c = s_w[k];
            if (k < wid) wpre += c;
            tot += c;
        }
        uint64_t row = (uint64_t)rb + i;
        if (i < nr && row < num_rows) {
            valid[row] = bit ? 1 : 0;
            uint32_t vi = running + wpre + pre;
            if (WIDTH == 4) {
                reinterpret_cast<uint32_t*>(values)[row] =
                    bit ? reinterpret_cast<const uint32_t*>(vals)[vi] : 0u;
            } else {
                reinterpret_cast<uint64_t*>(values)[row] =
                    bit ? reinterpret_cast<const uint64_t*>(vals)[vi] : 0ull;
            }
        }
        running += tot;
        __syncthreads();
    }
}

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
template <int NW, class Loader, int PAIR, bool AOS>
__global__ __launch_bounds__(PT_THREADS) void k_pass_scatter(Loader ld, PassParams pp, Words out) {
    static_assert(PAIR < 0 || (PAIR >= 1 && PAIR + 1 < NW), "pair = two carry words behind the key");
    static_assert(!AOS || (NW == 3 && PAIR == 1), "12-byte tuples: one key word + a two-word carry");
    __shared__ uint2    s_stage2[PT_TILE];  // 128 KiB: a word array uses the first half
    uint32_t* const     s_stage = reinterpret_cast<uint32_t*>(s_stage2);
    __shared__ uint32_t s_cnt[PT_MAXF + PT_DUMMY];  // (see rank_tile)
    __shared__ uint32_t s_base[PT_MAXF];
    __shared__ uint32_t s_delta[PT_MAXF];
    __shared__ uint32_t s_wsum[PT_THREADS / 64];
    uint32_t            seg, begin, end;
    if (!group_range(pp, blockIdx.x, seg, begin, end)) return;
    const uint32_t F = 1u << pp.fanout_log2, mask = F - 1u;

    // Thread d owns digit d's write cursor in a REGISTER: the reservation's round trip is
    // not waited for until the first tile has been loaded and ranked.
    uint32_t run = 0;  // thread d: where digit d's run of the current tile starts in the output
    uint32_t w[PT_ITEMS][NW];

    for (uint32_t base = begin; base < end; base += PT_TILE) {
        for (uint32_t d = threadIdx.x; d < F; d += PT_THREADS) s_cnt[d] = 0;
        lds_barrier();

        // every load of the tile is issued before the first rank is taken; the ranks wait for the keys only
        const uint32_t ok = ld.template load_tile<NW>(base, end, w);
        // first pass of key + two-word carry: ranks and positions two per register, branch-free (rank_tile).
        // Everything else keeps a rank per register and a branch per item.  The later passes of that shape
        // and the packed kernel gained nothing measurable from the branch-free form
        // (profiles/scatter_rank_ab.log), and with up to four words per tuple in registers there is no room
        // for PT_ITEMS ranks in flight (compiled that way, the four-word kernels spilled more than they do)
        constexpr bool BATCHED = NW == 3 && PAIR == 1 && is_src_loader<Loader>::value;
        uint32_t       ps[PT_ITEMS / 2];  // BATCHED: ranks, then LDS positions, two per register
        uint32_t       dr[PT_ITEMS];      // otherwise: digit << 16 | rank, then LDS position; 0xffffffff = no tuple
        if constexpr (BATCHED) {
            rank_tile<NW>(pp, mask, ok, w, s_cnt, ps);
        } else {
#pragma unroll
            for (int j = 0; j < PT_ITEMS; ++j) {
                dr[j] = 0xffffffffu;
                if ((ok >> j) & 1u) {
                    uint32_t d = pass_digit(pp, w[j][0], mask);
                    uint32_t r = atomicAdd(&s_cnt[d], 1u);
                    dr[j] = (d << 16) | r;
                }
            }
        }
        lds_barrier();

        // PT_THREADS >= PT_MAXF: thread d scans digit d
        // Thread d reserves digit d's range of this tile with one global atomic; its round
        // trip is not waited for until word 0 has been staged.
        uint32_t c = threadIdx.x < F ? s_cnt[threadIdx.x] : 0u;
        if (c) {
            run = atomicAdd(&pp.cursor[(((size_t)seg * F + threadIdx.x) << pp.xcd_log2) |
                                       (blockIdx.x & ((1u << pp.xcd_log2) - 1u))], c);
        }
        uint32_t total;
        uint32_t ex = block_excl_scan(c, s_wsum, total);
        if (threadIdx.x < F) s_base[threadIdx.x] = ex;
        lds_barrier();

        // LDS position of every tuple, computed once for all word arrays
        if constexpr (BATCHED) {
            place_tile<NW>(pp, mask, ok, w, s_base, ps);
        } else {
#pragma unroll
            for (int j = 0; j < PT_ITEMS; ++j)
                if (dr[j] != 0xffffffffu) dr[j] = s_base[dr[j] >> 16] + (dr[j] & 0xffffu);
        }

        // key + two-word carry (NW == 3): keys and carry pairs of half the sorted tile are staged
        // TOGETHER and copied out together — as 12-byte tuples (AOS) or into the key array and the
        // pair array — so no per-element destination has to be kept in registers between the two
        // arrays (the 16 extra VGPRs spilled to scratch)
        // (the copy-out's thread index is opaque to the compiler: its element indices and LDS addresses,
        // 3 * PT_ITEMS values that do not change from tile to tile, were otherwise hoisted out of the tile
        // loop and held in registers — or spilled — through the phases that have every load in flight)
        const uint32_t tid = BATCHED ? tile_tid() : threadIdx.x;  // (the other shapes compile to more scratch with it)
        if constexpr (NW == 3 && PAIR == 1) {
            constexpr uint32_t HALF = PT_TILE / 2;
            uint2* const       s_p = s_stage2;                                      // [HALF] carries
            uint32_t* const    s_k = reinterpret_cast<uint32_t*>(s_stage2 + HALF);  // [HALF] keys
            if (!BATCHED && threadIdx.x < F) s_delta[threadIdx.x] = run - ex;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int j = 0; j < PT_ITEMS; ++j) {
                    const uint32_t lp = (BATCHED ? tile_pos(ps, j) : dr[j]) - h * HALF;  // (no tuple: PT_NO_POS stays out of range)
                    if (lp < HALF) {
                        s_k[lp] = w[j][0];
                        s_p[lp] = make_uint2(w[j][1], w[j][2]);
                    }
                }
                // global index = delta + sorted position.  BATCHED: behind the first half's staging, since the
                // reservation was issued after the carry loads and waiting for it waits for all of them
                if (BATCHED && h == 0 && threadIdx.x < F) s_delta[threadIdx.x] = run - ex;
                lds_barrier();
#pragma unroll
                for (int k = 0; k < PT_ITEMS / 2; ++k) {
                    const uint32_t i = k * PT_THREADS + tid, gi = h * HALF + i;
                    if (gi < total) {
                        const uint32_t v = s_k[i];
                        const uint2    c = s_p[i];
                        const uint32_t g = s_delta[pass_digit(pp, v, mask)] + gi;
                        if constexpr (AOS) {
                            uint32_t* o = out.w[0] + (size_t)g * 3u;
                            o[0] = v;
                            o[1] = c.x;
                            o[2] = c.y;
                            if (pp.side_out) pp.side_out[g] = (uint16_t)((v >> pp.next_shift) & pp.next_mask);
                        } else {
                            out.w[0][g] = v;
                            reinterpret_cast<uint2*>(out.w[1])[g] = c;
                        }
                    }
                }
                lds_barrier();
            }
            continue;
        }
        // word 0 (the hashed key): stage in digit order, copy out.  The digit of a staged
        // key is recomputed from the key itself, and the global destination of each LDS
        // position is kept in a register for the remaining word arrays.
#pragma unroll
        for (int j = 0; j < PT_ITEMS; ++j)
            if (dr[j] != 0xffffffffu) s_stage[dr[j]] = w[j][0];
        if (threadIdx.x < F) s_delta[threadIdx.x] = run - ex;  // global index = delta + LDS position
        lds_barrier();
        uint32_t dest[PT_ITEMS];
#pragma unroll
        for (int k = 0; k < PT_ITEMS; ++k) {
            const uint32_t i = k * PT_THREADS + tid;
            dest[k] = 0;
            if (i < total) {
                const uint32_t v = s_stage[i];
                dest[k] = s_delta[pass_digit(pp, v, mask)] + i;
                out.w[0][dest[k]] = v;
            }
        }
        lds_barrier();
#pragma unroll
        for (int a = 1; a < NW; ++a) {
            if constexpr (PAIR >= 0) {
                if (a == PAIR + 1) continue;  // went out with word PAIR
                if (a == PAIR) {
#pragma unroll
                    for (int j = 0; j < PT_ITEMS; ++j)
                        if (dr[j] != 0xffffffffu)
                            s_stage2[dr[j]] = make_uint2(w[j][a], w[j][a + 1 < NW ? a + 1 : a]);
                    lds_barrier();
                    uint2* dst2 = reinterpret_cast<uint2*>(out.w[a]);
#pragma unroll
                    for (int k = 0; k < PT_ITEMS; ++k) {
                        const uint32_t i = k * PT_THREADS + tid;
                        if (i < total) dst2[dest[k]] = s_stage2[i];
                    }
                    lds_barrier();
                    continue;
                }
            }
#pragma unroll
            for (int j = 0; j < PT_ITEMS; ++j)
                if (dr[j] != 0xffffffffu) s_stage[dr[j]] = w[j][a];
            lds_barrier();
            uint32_t* dst = out.w[a];
#pragma unroll
            for (int k = 0; k < PT_ITEMS; ++k) {
                const uint32_t i = k * PT_THREADS + tid;
                if (i < total) dst[dest[k]] = s_stage[i];
            }
            lds_barrier();
        }
    }
}

// Packed variant for {hashed key, one carry word} tuples (the BASELINE shape): the tile is
// staged as 8-byte pairs (128 KiB of LDS — the workgroup owns the CU anyway) and copied out
// with one 8-byte store per tuple into ONE output array.  Against two word arrays this
// halves the number of output streams and doubles the bytes per contiguous run (a run of 64
// tuples is 512 contiguous bytes instead of two runs of 256), which is what the scatter's
// rate follows; it also needs one staging round and two barriers less per tile.
template <class Loader, bool BLK_OUT = false>
__global__ __launch_bounds__(PT_THREADS) void k_pass_scatter_packed(Loader ld, PassParams pp, uint2* out) {
    __shared__ uint2    s_stage[PT_TILE];
    __shared__ uint32_t s_cnt[PT_MAXF];
    __shared__ uint32_t s_base[PT_MAXF];
    __shared__ uint32_t s_delta[PT_MAXF];
    __shared__ uint32_t s_wsum[PT_THREADS / 64];
    uint32_t            seg, begin, end;
    if (!group_range(pp, blockIdx.x, seg, begin, end)) return;
    const uint32_t F = 1u << pp.fanout_log2, mask = F - 1u;

    uint32_t run = 0;  // thread d: where digit d's run of the current tile starts in the output
    // the next tile's loads are issued as soon as this tile has been staged (its registers are
    // dead then) and fly during the copy-out
    uint32_t w[PT_ITEMS][2];
    uint32_t ok_raw = ld.template issue_tile<2>(begin, end, w);
    for (uint32_t base = begin; base < end; base += PT_TILE) {
        for (uint32_t d = threadIdx.x; d < F; d += PT_THREADS) s_cnt[d] = 0;
        lds_barrier();

        uint32_t       dr[PT_ITEMS];  // digit << 16 | rank, 0xffffffff = no tuple
        const uint32_t ok = ld.template finish_tile<2>(base, end, ok_raw, w);  // (source tuples: NULL drop + hashing)
#pragma unroll
        for (int j = 0; j < PT_ITEMS; ++j) {
            dr[j] = 0xffffffffu;
            if ((ok >> j) & 1u) {
                uint32_t d = pass_digit(pp, w[j][0], mask);
                uint32_t r = atomicAdd(&s_cnt[d], 1u);
                dr[j] = (d << 16) | r;
            }
        }
        lds_barrier();

        uint32_t c = threadIdx.x < F ? s_cnt[threadIdx.x] : 0u;
        if (c)
            run = atomicAdd(&pp.cursor[(((size_t)seg * F + threadIdx.x) << pp.xcd_log2) |
                                       (blockIdx.x & ((1u << pp.xcd_log2) - 1u))], c);
        uint32_t total;
        uint32_t ex = block_excl_scan(c, s_wsum, total);
        if (threadIdx.x < F) s_base[threadIdx.x] = ex;
        lds_barrier();

#pragma unroll
        for (int j = 0; j < PT_ITEMS; ++j)
            if (dr[j] != 0xffffffffu)
                s_stage[s_base[dr[j] >> 16] + (dr[j] & 0xffffu)] = make_uint2(w[j][0], w[j][1]);
        if (base + PT_TILE < end) ok_raw = ld.template issue_tile<2>(base + PT_TILE, end, w);
        if (threadIdx.x < F) s_delta[threadIdx.x] = run - ex;  // global index = delta + LDS position
        lds_barrier();

#pragma unroll
        for (int k = 0; k < PT_ITEMS; ++k) {
            const uint32_t i = k * PT_THREADS + threadIdx.x;
            if (i < total) {
                const uint2    v = s_stage[i];
                const uint32_t g = s_delta[pass_digit(pp, v.x, mask)] + i;
                if constexpr (BLK_OUT) {  // (see BlockedLoader)
                    uint32_t* o = reinterpret_cast<uint32_t*>(out) + BlockedLoader::key_at(g);
                    o[0] = v.x;
                    o[BlockedLoader::BLK] = v.y;
                } else {
                    out[g] = v;
                }
                if (pp.side_out) pp.side_out[g] = (uint16_t)((v.x >> pp.next_shift) & pp.next_mask);
            }
        }
        // no barrier: the next tile passes two barriers before it overwrites s_stage / s_delta
    }
}

// ============================================================= heavy task list
// Probe partitions above JN_HEAVY tuples are cut into tasks so that a skewed
// (Zipf) probe side does not serialise on one workgroup; each task rebuilds the
// (small) build table of its partition.
__global__ void k_heavy_tasks(const uint32_t* offR, const uint32_t* offS, uint32_t NP,
                              uint32_t* tasks, uint32_t* n_heavy, uint32_t max_tasks) {
    uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= NP) return;
    uint32_t sb = offS[q], se = offS[q + 1];
    uint32_t len = se - sb;
    if (len <= JN_HEAVY || offR[q + 1] == offR[q]) return;
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

// ============================================================ broadcast join
// A build side of at most JN_RMAX rows (the filtered dimension tables of the JOB plans: a
// handful of rows against millions) needs no partitioning: every workgroup builds the SAME
// LDS table straight from the build child's columns and streams a slice of the probe
// child's columns past it — page decode, NULL-key drop and hashing happen on the way, the
// probe side is read exactly once and nothing is scattered.  (The reference counterpart is
// still hash_join_omp, src/execute.cpp:44-262, with num_buckets = 1.)
// The table keeps key words + the build ROW; build carries are fetched from the build
// columns on emit (a few KB: cache resident).  With no radix digit to derive an EMPTY
// sentinel from, a slot is valid when its index is below its bucket's insert counter.
template <int KW, int CWR, int CWS>
__global__ __launch_bounds__(JN_THREADS) void k_join_bcast(BcastParams bp) {
    constexpr int RW = KW + 1;  // key words + build row
    __shared__ __attribute__((aligned(16))) uint32_t t_w[RW][JN_CAP];
    __shared__ __attribute__((aligned(16))) uint32_t t_cnt[JN_CAP / 4];
    __shared__ uint32_t s_wtot[JN_THREADS / 64];
    __shared__ unsigned long long s_obase;
    const uint32_t     lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    constexpr uint32_t BMASK = JN_CAP / 4 - 1;

    // ---- build (identical in every workgroup)
    for (uint32_t i = threadIdx.x; i < JN_CAP / 4; i += JN_THREADS) t_cnt[i] = 0;
    lds_barrier();
    for (uint32_t r = threadIdx.x; r < bp.R.n_rows; r += JN_THREADS) {
        uint32_t lo, hi;
        if (!src_key<KW>(bp.R, r, lo, hi)) continue;
        uint32_t b = lo & BMASK;
        while (true) {
            uint32_t pos = atomicAdd(&t_cnt[b], 1u);
            if (pos < 4) {
                const uint32_t slot = b * 4 + pos;
                t_w[0][slot] = lo;
                if constexpr (KW == 2) t_w[1][slot] = hi;
                t_w[KW][slot] = r;
                break;
            }
            b = (b + 1) & BMASK;
        }
    }
    lds_barrier();

    // matches of one probe key in bucket b: bit mask over its (valid) slots; `more` = the
    // bucket overflowed, the walk goes on in the next one
    auto match = [&](uint32_t b, uint32_t lo, uint32_t hi, bool& more) -> uint32_t {
        const uint32_t cnt = t_cnt[b];
        const uint4    kv = *reinterpret_cast<const uint4*>(&t_w[0][b * 4]);
        uint32_t       eq = (uint32_t)(kv.x == lo) | ((uint32_t)(kv.y == lo) << 1) |
                      ((uint32_t)(kv.z == lo) << 2) | ((uint32_t)(kv.w == lo) << 3);
        if constexpr (KW == 2) {
            const uint4 hv = *reinterpret_cast<const uint4*>(&t_w[1][b * 4]);
            eq &= (uint32_t)(hv.x == hi) | ((uint32_t)(hv.y == hi) << 1) |
                  ((uint32_t)(hv.z == hi) << 2) | ((uint32_t)(hv.w == hi) << 3);
        }
        more = cnt > 4;
        return eq & ((1u << min(cnt, 4u)) - 1u);
    };

    // ---- probe: chunks of JN_SUB rows, strided over the grid
    const uint32_t n = bp.S.n_rows;
    for (uint64_t base = (uint64_t)blockIdx.x * JN_SUB; base < n; base += (uint64_t)gridDim.x * JN_SUB) {
        uint32_t klo[JN_SPT], khi[JN_SPT], m[JN_SPT];
#pragma unroll
        for (int j = 0; j < JN_SPT; ++j) {
            const uint64_t row = base + (uint64_t)j * JN_THREADS + threadIdx.x;
            m[j] = 0;
            klo[j] = khi[j] = 0;
            if (row < n && src_key<KW>(bp.S, (uint32_t)row, klo[j], khi[j])) {
                uint32_t b = klo[j] & BMASK;
                bool     more;
                do {
                    m[j] += (uint32_t)__popc(match(b, klo[j], khi[j], more));
                    b = (b + 1) & BMASK;
                } while (more);
            }
        }
        // output offsets: wave prefix (ballot when every lane has <= 1 match), one global
        // reservation per chunk
        uint32_t pre[JN_SPT], wave_total = 0;
#pragma unroll
        for (int j = 0; j < JN_SPT; ++j) {
            uint32_t tot;
            if (__ballot(m[j] > 1) == 0) {
                uint64_t mk = __ballot(m[j] == 1);
                pre[j] = lane_prefix(mk);
                tot = (uint32_t)__popcll(mk);
            } else {
                uint32_t incl = m[j];
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    uint32_t t = __shfl_up(incl, off);
                    if (lane >= (uint32_t)off) incl += t;
                }
                pre[j] = incl - m[j];
                tot = __shfl(incl, 63);
            }
            pre[j] += wave_total;
            wave_total += tot;
        }
        if (lane == 0) s_wtot[wid] = wave_total;
        lds_barrier();
        if (threadIdx.x == 0) {
            uint32_t tot = 0;
            for (int w = 0; w < JN_THREADS / 64; ++w) tot += s_wtot[w];
            s_obase = tot ? atomicAdd(bp.out_cursor, (unsigned long long)tot) : 0ull;
        }
        lds_barrier();
        const uint64_t gbase = s_obase;
        uint64_t       obase = gbase;
        uint32_t       block_total = 0;
        for (uint32_t w = 0; w < JN_THREADS / 64; ++w) {
            uint32_t t = s_wtot[w];
            if (w < wid) obase += t;
            block_total += t;
        }
        // rows beyond the stream capacity are counted but not written (the host re-runs the
        // join with exact-size buffers)
        if (gbase + block_total <= bp.out_cap) {
#pragma unroll
            for (int j = 0; j < JN_SPT; ++j) {
                if (m[j] == 0) continue;
                const uint32_t srow = (uint32_t)(base + (uint64_t)j * JN_THREADS + threadIdx.x);
                uint64_t       row = obase + pre[j];
                uint32_t       k0, k1 = 0;
                unhash_key<KW>(klo[j], khi[j], k0, k1);
                uint32_t p0, p1, p2;
                src_carry<CWS>(bp.S, srow, p0, p1, p2);
                uint32_t b = klo[j] & BMASK;
                bool     more;
                do {
                    uint32_t eq = match(b, klo[j], khi[j], more);
                    while (eq) {
                        const uint32_t slot = b * 4 + (uint32_t)__builtin_ctz(eq);
                        eq &= eq - 1;
                        uint32_t b0, b1, b2;
                        src_carry<CWR>(bp.R, t_w[KW][slot], b0, b1, b2);
                        stream_store(bp.key, row, k0, k1);
                        if constexpr (CWR >= 1) stream_store(bp.bc, row, b0, b1, b2);
                        if constexpr (CWS >= 1) stream_store(bp.pc, row, p0, p1, p2);
                        ++row;
                    }
                    b = (b + 1) & BMASK;
                } while (more);
            }
        }
        lds_barrier();  // s_wtot / s_obase are reused by the next chunk
    }
}

// ====================================================== semi / anti joins
// RJ_NODE_SEMI / RJ_NODE_ANTI ask "has this preserved row a partner on the filter side?".  The
// filter side's DISTINCT hashed keys go into an LDS set; the preserved tuples are looked up and
// each one that hits (SEMI) or misses (ANTI) is emitted ONCE — the un-hashed key and its carry,
// ballot/mbcnt offsets inside the wave, one global reservation per JN_SUB tuples (as k_join_bcast).
// Nothing travels with a filter key, so a slot is the hashed key alone: 32 KiB (KW = 1) or 64 KiB
// (KW = 2) for JN_CAP slots, of which at most JN_RMAX are used (load <= 50 %).
//   insert  open addressing, linear probing, one LDS compare-and-swap per step: a key that is
//           already there is not stored again (duplicates collapse on insert);
//   lookup  walk from the home slot until the key or an EMPTY slot.
// EMPTY is the all-ones word; a filter key whose hash is all ones sets a flag instead of a slot.
// The home slot is the multiplicative hash of the key words: their low radix bits are the same for
// a whole partition, the product's high bits are not.
static_assert((JN_CAP & (JN_CAP - 1)) == 0, "set slots: a power of two");

template <int KW>
struct FilterSet {
    using Slot = std::conditional_t<KW == 1, uint32_t, unsigned long long>;
    static constexpr Slot     EMPTY = ~Slot(0);
    static constexpr uint32_t LOG2 = ilog2_u32(JN_CAP), MASK = JN_CAP - 1;
    Slot*     t;         // [JN_CAP]
    uint32_t* count;     // distinct keys in the slots
    uint32_t* sentinel;  // 1: the EMPTY key itself is in the set

    __device__ __forceinline__ static Slot make(uint32_t lo, uint32_t hi) {
        if constexpr (KW == 1)
            return lo;
        else
            return (Slot)lo | ((Slot)hi << 32);
    }
    __device__ __forceinline__ static uint32_t home(uint32_t lo, uint32_t hi) {
        return ((lo ^ hi) * 0x9e3779b1u) >> (32 - LOG2);
    }
    // every thread of the workgroup; the caller puts a barrier behind it
    __device__ __forceinline__ void clear() const {
        uint4* t4 = reinterpret_cast<uint4*>(t);
        for (uint32_t i = threadIdx.x; i < JN_CAP * sizeof(Slot) / 16; i += blockDim.x)
            t4[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
        if (threadIdx.x == 0) {
            *count = 0;
            *sentinel = 0;
        }
    }
    // true: the key was not in the set before
    __device__ __forceinline__ bool insert(uint32_t lo, uint32_t hi) const {
        const Slot k = make(lo, hi);
        if (k == EMPTY) {
            *sentinel = 1u;
            return false;
        }
        uint32_t s = home(lo, hi);
        while (true) {
            const Slot prev = atomicCAS(&t[s], EMPTY, k);
            if (prev == EMPTY) return true;
            if (prev == k) return false;
            s = (s + 1) & MASK;
        }
    }
    __device__ __forceinline__ bool has(uint32_t lo, uint32_t hi) const {
        const Slot k = make(lo, hi);
        if (k == EMPTY) return *sentinel != 0;
        uint32_t s = home(lo, hi);
        while (true) {
            const Slot v = t[s];
            if (v == k) return true;
            if (v == EMPTY) return false;
            s = (s + 1) & MASK;
        }
    }
};

// Emit the items with e[j] set: offsets from the wave ballots, ONE global reservation for the
// workgroup, then the un-hashed key (key stream) and carry(j, p0, p1, p2) (preserved carry stream).
// Contains barriers: every thread of the workgroup calls it.
template <int KW, int SPT, class Carry>
__device__ __forceinline__ void filter_emit(const FilterParams& fp, const bool (&e)[SPT], const uint32_t (&klo)[SPT],
                                            const uint32_t (&khi)[SPT], uint32_t* s_wtot,
                                            unsigned long long* s_obase, Carry carry) {
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint32_t       pre[SPT], wave_total = 0;
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
        const uint64_t mk = __ballot(e[j]);
        pre[j] = wave_total + lane_prefix(mk);
        wave_total += (uint32_t)__popcll(mk);
    }
    if (lane == 0) s_wtot[wid] = wave_total;
    lds_barrier();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (uint32_t w = 0; w < nw; ++w) tot += s_wtot[w];
        *s_obase = tot ? atomicAdd(fp.out_cursor, (unsigned long long)tot) : 0ull;
    }
    lds_barrier();
    uint64_t obase = *s_obase;
    for (uint32_t w = 0; w < wid; ++w) obase += s_wtot[w];
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
        const uint64_t row = obase + pre[j];
        // (the output never holds more rows than the preserved side: the bound is a guard only)
        if (!e[j] || row >= fp.out_cap) continue;
        if (fp.key.mode != ST_NONE) {
            uint32_t k0, k1 = 0;
            unhash_key<KW>(klo[j], khi[j], k0, k1);
            stream_store(fp.key, row, k0, k1);
        }
        if (fp.pc.mode != ST_NONE) {
            uint32_t p0, p1, p2;
            carry(j, p0, p1, p2);
            stream_store(fp.pc, row, p0, p1, p2);
        }
    }
    lds_barrier();  // s_wtot / s_obase are reused by the next chunk
}

// Broadcast form: a filter side of at most JN_RMAX rows.  Every workgroup builds the SAME set
// straight from the filter child's key column (page decode, NULL / NaN drop, hashing on the way)
// and streams a grid-strided slice of the preserved child past it.  A preserved row whose key is
// NULL or NaN has no partner: ANTI emits it.  keyless (the key types differ): no key is read,
// every row misses.
template <int KW, int CWS>
__global__ __launch_bounds__(JN_THREADS) void k_filter_bcast(FilterParams fp) {
    using Set = FilterSet<KW>;
    __shared__ __attribute__((aligned(16))) typename Set::Slot t_set[JN_CAP];
    __shared__ uint32_t s_cnt[2];
    __shared__ uint32_t s_wtot[JN_THREADS / 64];
    __shared__ unsigned long long s_obase;
    const Set set{t_set, &s_cnt[0], &s_cnt[1]};
    set.clear();
    lds_barrier();
    if (!fp.keyless) {
        for (uint32_t r = threadIdx.x; r < fp.F.n_rows; r += JN_THREADS) {
            uint32_t lo, hi;
            if (src_key<KW>(fp.F, r, lo, hi)) (void)set.insert(lo, hi);
        }
    }
    lds_barrier();
    const uint32_t n = fp.P.n_rows;
    for (uint64_t base = (uint64_t)blockIdx.x * JN_SUB; base < n; base += (uint64_t)gridDim.x * JN_SUB) {
        uint32_t klo[JN_SPT], khi[JN_SPT];
        bool     e[JN_SPT];
#pragma unroll
        for (int j = 0; j < JN_SPT; ++j) {
            const uint64_t row = base + (uint64_t)j * JN_THREADS + threadIdx.x;
            klo[j] = khi[j] = 0;
            e[j] = false;
            if (row < n) {
                bool hit = false;
                if (!fp.keyless && src_key<KW>(fp.P, (uint32_t)row, klo[j], khi[j])) hit = set.has(klo[j], khi[j]);
                e[j] = fp.anti ? !hit : hit;
            }
        }
        filter_emit<KW, JN_SPT>(fp, e, klo, khi, s_wtot, &s_obase, [&](int j, uint32_t& p0, uint32_t& p1, uint32_t& p2) {
            src_carry<CWS>(fp.P, (uint32_t)(base + (uint64_t)j * JN_THREADS + threadIdx.x), p0, p1, p2);
        });
    }
}

// ANTI on the partitioned path: the preserved rows the first radix pass drops (NULL key; FP64 NaN
// key) have no partner, so they belong to the result.  Grid-strided over the preserved child, the
// same tuple formation (src_key / src_carry over the TupleSrc) and output cursor as the filter.
template <int KW, int CWS>
__global__ __launch_bounds__(JN_THREADS) void k_filter_nullkeys(FilterParams fp) {
    __shared__ uint32_t s_wtot[JN_THREADS / 64];
    __shared__ unsigned long long s_obase;
    const uint32_t n = fp.P.n_rows;
    for (uint64_t base = (uint64_t)blockIdx.x * JN_SUB; base < n; base += (uint64_t)gridDim.x * JN_SUB) {
        uint32_t klo[JN_SPT], khi[JN_SPT];
        bool     e[JN_SPT];
#pragma unroll
        for (int j = 0; j < JN_SPT; ++j) {
            const uint64_t row = base + (uint64_t)j * JN_THREADS + threadIdx.x;
            klo[j] = khi[j] = 0;
            e[j] = row < n && !src_key<KW>(fp.P, (uint32_t)row, klo[j], khi[j]);
        }
        filter_emit<KW, JN_SPT>(fp, e, klo, khi, s_wtot, &s_obase, [&](int j, uint32_t& p0, uint32_t& p1, uint32_t& p2) {
            src_carry<CWS>(fp.P, (uint32_t)(base + (uint64_t)j * JN_THREADS + threadIdx.x), p0, p1, p2);
        });
    }
}

// Partitioned form: one workgroup per co-partition, or per heavy task of a preserved partition
// above JN_HEAVY tuples (k_heavy_tasks; it leaves partitions WITHOUT filter tuples to the main
// workgroups, which is where ANTI emits them whole).  The set is built from the partition's filter
// keys in blocks of JN_RMAX / 2 tuples for as long as it holds at most JN_RMAX / 2 distinct keys,
// so a round ends with at most JN_RMAX of them.  A partition that needs more than one round (more
// distinct filter keys than one set holds: a forced radix_bits, or adversarial hashes) is exact
// all the same: every JN_SUB-tuple chunk of preserved tuples stays in registers while the rounds
// are rebuilt one after the other, its per-tuple hit flags OR-ed over them, and is emitted after
// the last one.  No memory outside the LDS holds a flag.
template <int KW, int CWS>
__global__ __launch_bounds__(JN_THREADS) void k_filter_join(FilterParams fp) {
    using Set = FilterSet<KW>;
    constexpr int      TH = JN_THREADS, SPT = JN_SPT, SUB = JN_SUB, SW = KW + CWS;
    constexpr uint32_t RB = JN_RMAX / 2;  // filter tuples per insert block
    static_assert(SPT * TH == SUB, "sub-chunk geometry");
    __shared__ __attribute__((aligned(16))) typename Set::Slot t_set[JN_CAP];
    __shared__ uint32_t s_cnt[2];
    __shared__ uint32_t s_wtot[TH / 64];
    __shared__ unsigned long long s_obase;
    const Set set{t_set, &s_cnt[0], &s_cnt[1]};

    uint32_t q, sbeg, send;
    if (blockIdx.x < fp.heavy_grid) {
        if (blockIdx.x >= *fp.n_heavy) return;
        q = fp.heavy_tasks[3 * blockIdx.x + 0];
        sbeg = fp.heavy_tasks[3 * blockIdx.x + 1];
        send = fp.heavy_tasks[3 * blockIdx.x + 2];
    } else {
        q = blockIdx.x - fp.heavy_grid;
        if (q >= fp.NP) return;
        sbeg = fp.offP[q];
        send = fp.offP[q + 1];
        if (send - sbeg > JN_HEAVY && fp.offF[q + 1] != fp.offF[q]) return;  // split into heavy tasks
    }
    const uint32_t rbeg = fp.offF[q], rend = fp.offF[q + 1];
    if (sbeg >= send || (!fp.anti && rbeg == rend)) return;

    // one round of the set: filter tuples from `from` on; returns where the round ended
    auto build_round = [&](uint32_t from) -> uint32_t {
        lds_barrier();  // nobody still looks up the previous round
        set.clear();
        lds_barrier();
        uint32_t cur = from;
        while (cur < rend) {
            const uint32_t nb = min(RB, rend - cur);
            uint32_t       added = 0;
            for (uint32_t i = threadIdx.x; i < nb; i += TH) {
                const uint32_t lo = fp.Fw.w[0][cur + i], hi = KW == 2 ? fp.Fw.w[KW - 1][cur + i] : 0u;
                added += set.insert(lo, hi) ? 1u : 0u;
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) added += __shfl_xor(added, off);
            if ((threadIdx.x & 63u) == 0 && added) atomicAdd(set.count, added);
            lds_barrier();
            cur += nb;
            const uint32_t distinct = *set.count;
            lds_barrier();  // every thread has read the count before the next block adds to it
            if (distinct > (uint32_t)JN_RMAX - RB) break;
        }
        return cur;
    };

    uint32_t sw[SPT][SW];
    auto load_chunk = [&](uint32_t sc, uint32_t sn) {
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            // (items past the chunk re-read its last tuple; they are masked off)
            const uint32_t idx = sc + min((uint32_t)(j * TH + threadIdx.x), sn - 1u);
            part_tuple<KW, CWS>(fp.Pw, fp.packP, fp.aosP, idx, sw[j]);
        }
    };

    const uint32_t first_end = build_round(rbeg);
    const bool     one_round = first_end == rend;
    for (uint32_t sc = sbeg; sc < send; sc += SUB) {
        const uint32_t sn = min((uint32_t)SUB, send - sc);
        load_chunk(sc, sn);
        bool hit[SPT];
#pragma unroll
        for (int j = 0; j < SPT; ++j) hit[j] = false;
        uint32_t end = (one_round || sc == sbeg) ? first_end : build_round(rbeg);
        while (true) {
#pragma unroll
            for (int j = 0; j < SPT; ++j)
                if ((uint32_t)(j * TH + threadIdx.x) < sn && !hit[j]) hit[j] = set.has(sw[j][0], KW == 2 ? sw[j][KW - 1] : 0u);
            if (end == rend) break;
            end = build_round(end);
        }
        uint32_t klo[SPT], khi[SPT];
        bool     e[SPT];
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            klo[j] = sw[j][0];
            khi[j] = KW == 2 ? sw[j][KW - 1] : 0u;
            e[j] = (uint32_t)(j * TH + threadIdx.x) < sn && (fp.anti ? !hit[j] : hit[j]);
        }
        filter_emit<KW, SPT>(fp, e, klo, khi, s_wtot, &s_obase, [&](int j, uint32_t& p0, uint32_t& p1, uint32_t& p2) {
            tuple_carry<KW, CWS>(sw[j], p0, p1, p2);
        });
    }
}

// k_gather for the row-index stream of an outer join's optional side: OUTER_NO_ROW (a padded row)
// is never dereferenced and gives a NULL; every row gets a validity byte.
template <int WIDTH>
__global__ __launch_bounds__(256) void k_outer_gather(ColRef src, const uint32_t* idx, uint64_t n, uint8_t* dst,
                                                      uint8_t* dst_valid) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = idx[i];
    const bool     there = r != OUTER_NO_ROW;
    if (WIDTH == 4)
        reinterpret_cast<uint32_t*>(dst)[i] = there ? col_load32(src, r) : 0u;
    else
        reinterpret_cast<uint64_t*>(dst)[i] = there ? col_load64(src, r) : 0ull;
    dst_valid[i] = there ? (src.valid ? src.valid[r] : (uint8_t)1) : (uint8_t)0;
}

// ================================================================== K7 gather
// Late materialisation: out[i] = column[idx[i]] (reference counterpart: the
// per-row `out.push_back(lrow[ci])`, src/execute.cpp:236-242).
template <int WIDTH>
__global__ __launch_bounds__(256) void k_gather(ColRef src, const uint32_t* idx, uint64_t n,
                                                OutStream dst, uint8_t* dst_valid) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t r = idx ? idx[i] : (uint32_t)i;
    if (WIDTH == 4) {
        stream_store(dst, i, col_load32(src, r), 0u);
    } else {
        uint64_t v = col_load64(src, r);
        stream_store(dst, i, (uint32_t)v, (uint32_t)(v >> 32));
    }
    if (dst_valid) dst_valid[i] = src.valid ? src.valid[r] : (uint8_t)1;
}

// =========================================================== K8 page finishing
// Headers + all-ones validity bitmaps of result pages whose values were written
// in place by the probe / gather kernels (page layout: reference
// src/build_table.cpp:472-481).
__global__ __launch_bounds__(256) void k_finish_pages(uint8_t* pages, uint64_t n_rows,
                                                      uint32_t rows_full) {
    uint8_t*       page = pages + (size_t)blockIdx.x * PAGE_BYTES;
    const uint64_t first = (uint64_t)blockIdx.x * rows_full;
    const uint32_t nr = (uint32_t)min((uint64_t)rows_full, n_rows - first);
    const uint32_t nb = (nr + 7) / 8;
    if (threadIdx.x == 0) {
        reinterpret_cast<uint16_t*>(page)[0] = (uint16_t)nr;
        reinterpret_cast<uint16_t*>(page)[1] = (uint16_t)nr;
    }
    uint8_t* bm = page + PAGE_BYTES - nb;
    for (uint32_t k = threadIdx.x; k < nb; k += blockDim.x) {
        uint32_t bits = nr - k * 8u;
        bm[k] = bits >= 8 ? 0xff : (uint8_t)((1u << bits) - 1u);
    }
}

// Same, for the (up to three) streams the probe kernel wrote, with the row count still on
// the device: launched right behind the probe, before the host reads the count back.
struct FinishStreams {
    uint8_t* pages[3];
    uint32_t rows_full[3];
    uint32_t n;
};
__global__ __launch_bounds__(256) void k_finish_streams(FinishStreams fs,
                                                        const unsigned long long* n_rows_dev,
                                                        uint64_t cap_rows) {
    const uint64_t n_rows = *n_rows_dev;
    if (n_rows > cap_rows) return;  // overflow: the host re-runs the probe with larger buffers
    // one wave per page: the header and a bitmap of at most 248 bytes
    const uint32_t b = blockIdx.y, lane = threadIdx.x & 63u;
    const uint32_t rf = fs.rows_full[b];
    const uint64_t pg = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t first = pg * rf;
    if (first >= n_rows) return;
    uint8_t*       page = fs.pages[b] + (size_t)pg * PAGE_BYTES;
    const uint32_t nr = (uint32_t)min((uint64_t)rf, n_rows - first);
    const uint32_t nb = (nr + 7) / 8;
    if (lane == 0) *reinterpret_cast<uint32_t*>(page) = nr | (nr << 16);  // n_rows, n_nonnull
    uint8_t* bm = page + PAGE_BYTES - nb;
    if (nr == rf && (nr & 31u) == 0 && ((PAGE_BYTES - nb) & 3u) == 0) {
        // full INT32 page: 248 bytes of ones, dword aligned
        for (uint32_t k = lane; k < nb / 4; k += 64) reinterpret_cast<uint32_t*>(bm)[k] = 0xffffffffu;
        return;
    }
    if (nr == rf && rf == ROWS64) {
        // full INT64 / FP64 page: 1007 bits = 126 bytes from offset 8066 — one halfword, then 31
        // dwords (the last byte holds 7 bits)
        static_assert(ROWS64 == 1007 && ((PAGE_BYTES - 126 + 2) & 3u) == 0, "bitmap layout of a full 8-byte page");
        if (lane == 0) *reinterpret_cast<uint16_t*>(bm) = 0xffffu;
        if (lane < 31) reinterpret_cast<uint32_t*>(bm + 2)[lane] = lane == 30 ? 0x7fffffffu : 0xffffffffu;
        return;
    }
    for (uint32_t k = lane; k < nb; k += 64) {
        uint32_t bits = nr - k * 8u;
        bm[k] = bits >= 8 ? 0xff : (uint8_t)((1u << bits) - 1u);
    }
}

// Result pages of a column that carries NULLs: a fixed rows_full rows per page
// (any fill that satisfies the layout decodes to the same rows), values packed
// densely in row order, bitmap at the tail.
template <int WIDTH>
__global__ __launch_bounds__(256) void k_encode_nullable(const uint8_t* values, const uint8_t* valid,
                                                         uint64_t n_rows, uint8_t* pages) {
    __shared__ uint32_t s_w[4];
    constexpr uint32_t  RF = WIDTH == 4 ? ROWS32 : ROWS64;
    uint8_t*            page = pages + (size_t)blockIdx.x * PAGE_BYTES;
    const uint64_t      first = (uint64_t)blockIdx.x * RF;
    const uint32_t      nr = (uint32_t)min((uint64_t)RF, n_rows - first);
    const uint32_t      nb = (nr + 7) / 8;
    uint8_t*            out_vals = page + (WIDTH == 4 ? HDR32 : HDR64);
    uint8_t*            bm = page + PAGE_BYTES - nb;
    const uint32_t      lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    uint32_t            running = 0;
    for (uint32_t base = 0; base < nr; base += 256) {
        uint32_t i = base + threadIdx.x;
        bool     bit = i < nr ? valid[first + i] != 0 : false;
        uint64_t mask = __ballot(bit);
        uint32_t pre = lane_prefix(mask);
        if (lane == 0) s_w[wid] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t wpre = 0, tot = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            uint32_t c = s_w[k];
            if (k < wid) wpre += c;
            tot += c;
        }
        if (bit) {
            uint32_t vi = running + wpre + pre;
            if (WIDTH == 4)
                reinterpret_cast<uint32_t*>(out_vals)[vi] =
                    reinterpret_cast<const uint32_t*>(values)[first + i];
            else
                reinterpret_cast<uint64_t*>(out_vals)[vi] =
                    reinterpret_cast<const uint64_t*>(values)[first + i];
        }
        // bitmap bytes of this 256-row slab: the wave's ballot holds 8 of them
        if (lane < 8) {
            uint32_t byte_idx = (base >> 3) + wid * 8u + lane;
            if (byte_idx < nb) bm[byte_idx] = (uint8_t)(mask >> (lane * 8u));
        }
        running += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        reinterpret_cast<uint16_t*>(page)[0] = (uint16_t)nr;
        reinterpret_cast<uint16_t*>(page)[1] = (uint16_t)running;
    }
}

// ============================================================ wide carries
// Validity of up to three carried columns as ONE 32-bit word per row (bit c = column c is
// non-NULL): the word then travels like a 32-bit column of the wide carry.
__global__ __launch_bounds__(256) void k_pack_validity(const uint8_t* v0, const uint8_t* v1, const uint8_t* v2,
                                                       uint32_t n, uint32_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = (uint32_t)(!v0 || v0[i]) | ((uint32_t)(!v1 || v1[i]) << 1) | ((uint32_t)(!v2 || v2[i]) << 2);
}

// The records a join emitted for a wide carry (cw words per output row) -> one dense array per
// carried column, plus validity bytes for the columns that have them.  Sequential reads and
// writes: this replaces k_gather's random reads through a row-index stream.
__global__ __launch_bounds__(256) void k_split_records(SplitParams sp, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* r = sp.rec + i * sp.cw;
    const uint32_t  vw = sp.valid_word >= 0 ? r[sp.valid_word] : 0xffffffffu;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (c >= sp.n_cols) break;
        const uint32_t lo = r[sp.col[c].word];
        if (sp.col[c].paged)
            stream_store(OutStream{sp.col[c].out, sp.col[c].width == 8 ? ST_PAGED64 : ST_PAGED32, 0}, i, lo,
                         sp.col[c].width == 8 ? r[sp.col[c].word + 1] : 0u);
        else if (sp.col[c].width == 8)
            reinterpret_cast<uint64_t*>(sp.col[c].out)[i] = (uint64_t)lo | ((uint64_t)r[sp.col[c].word + 1] << 32);
        else
            reinterpret_cast<uint32_t*>(sp.col[c].out)[i] = lo;
        if (sp.col[c].valid) sp.col[c].valid[i] = (uint8_t)((vw >> sp.col[c].valid_bit) & 1u);
    }
}

// Test hook (RJ_DEBUG_SHARD_FAIL=4): holds a stream for `ticks` of the constant-rate wall clock
// (hipDeviceAttributeWallClockRate) — a rank whose stage A "never finishes", so that its peers'
// bounded waits can be seen to expire.  Every wave leaves on its own when the time is up.
__global__ void k_debug_stall(unsigned long long ticks) {
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(127);
}

// ============================================================ aggregation
// RJ_NODE_AGG: GROUP BY the key of ONE partitioned relation (rj_device.hpp, AggParams).
// part_tuple's inverse: a tuple goes back into the partition layout (the tuples k_agg_parts defers).
template <int KW, int CW>
__device__ __forceinline__ void part_tuple_store(const Words& W, int pack, int aos, uint32_t idx, const uint32_t (&t)[KW + CW]) {
    constexpr int NW = KW + CW;
    if constexpr (KW == 1 && CW == 2) {
        if (aos) {
            uint32_t* p = W.w[0] + (size_t)idx * 3u;
            p[0] = t[0];
            p[1] = t[1];
            p[2] = t[2];
            return;
        }
    }
    if constexpr (KW == 1 && CW == 1) {
        if (pack) {
            reinterpret_cast<uint2*>(W.w[0])[idx] = make_uint2(t[0], t[1]);
            return;
        }
    }
    constexpr int NA = CW >= 2 ? NW - 2 : NW;
#pragma unroll
    for (int a = 0; a < NA; ++a) W.w[a][idx] = t[a];
    if constexpr (CW >= 2) reinterpret_cast<uint2*>(W.w[NA])[idx] = make_uint2(t[NA], t[NA + 1]);
}

constexpr long long AGG_MIN_INIT = 0x7fffffffffffffffll, AGG_MAX_INIT = -0x7fffffffffffffffll - 1;

// value of carried column `a` in the carry words c0..c2 (selects, no indexed registers); false = NULL
__device__ __forceinline__ bool agg_value(const AggCol& a, int valid_word, uint32_t c0, uint32_t c1, uint32_t c2, long long& v) {
    const uint32_t vw = valid_word == 0 ? c0 : (valid_word == 1 ? c1 : c2);
    if (a.valid_bit >= 0 && !((vw >> a.valid_bit) & 1u)) return false;
    const uint32_t lo = a.word == 0 ? c0 : (a.word == 1 ? c1 : c2), hi = a.word == 0 ? c1 : c2;
    v = a.width == 4 ? (long long)(int32_t)lo : (long long)((uint64_t)lo | ((uint64_t)hi << 32));
    return true;
}

// The merge table's entry of a hashed key (open addressing over m_slots entries; the key that
// equals the "nobody's" pattern owns entry m_slots); 0xffffffff and *m_overflow set when the walk
// finds neither the key nor a free entry within AGG_MERGE_WALK steps.
constexpr uint32_t AGG_MERGE_WALK = 4096, AGG_NO_ENTRY = 0xffffffffu;
__device__ __forceinline__ uint32_t agg_merge_entry(const AggParams& ap, unsigned long long k64) {
    if (k64 == AGG_NO_KEY) return ap.m_slots;
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(ap.m.key);
    const uint32_t      mask = ap.m_slots - 1u;
    uint32_t            slot = (uint32_t)((k64 * 0x9e3779b97f4a7c15ull) >> 32) & mask;
    if (ap.m_slots)
        for (uint32_t pr = 0; pr < AGG_MERGE_WALK && pr < ap.m_slots; ++pr) {
            unsigned long long cur = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == AGG_NO_KEY) {
                cur = atomicCAS(&keys[slot], AGG_NO_KEY, k64);
                if (cur == AGG_NO_KEY) cur = k64;
            }
            if (cur == k64) return slot;
            slot = (slot + 1u) & mask;
        }
    atomicOr(ap.m_overflow, 1u);
    return AGG_NO_ENTRY;
}
// one partial group -> the merge table (ordinary vector atomics in HBM)
template <int NC>
__device__ __forceinline__ void agg_merge(const AggParams& ap, uint32_t entry, unsigned long long rows,
                                          const unsigned long long (&nn)[NC], const unsigned long long (&sum)[NC],
                                          const long long (&mn)[NC], const long long (&mx)[NC]) {
    if (entry == AGG_NO_ENTRY) return;
    atomicAdd(&ap.m.rows[entry], rows);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        if (c >= ap.n_cols || nn[c] == 0) continue;
        atomicAdd(&ap.m.nn[c][entry], nn[c]);
        if (ap.col[c].need & AGG_NEED_SUM) atomicAdd(&ap.m.sum[c][entry], sum[c]);
        if (ap.col[c].need & AGG_NEED_MIN) atomicMin(&ap.m.mn[c][entry], mn[c]);
        if (ap.col[c].need & AGG_NEED_MAX) atomicMax(&ap.m.mx[c][entry], mx[c]);
    }
}
// one finished group -> row `row` of the node's output arrays; the key is un-hashed, as the join does
template <int KW, int NC>
__device__ __forceinline__ void agg_write(const AggParams& ap, uint64_t row, unsigned long long k64, bool null_key,
                                          unsigned long long rows, const unsigned long long (&nn)[NC],
                                          const unsigned long long (&sum)[NC], const long long (&mn)[NC],
                                          const long long (&mx)[NC]) {
    if (row >= ap.out_cap) return;
    if (ap.out.key) {
        if constexpr (KW == 1)
            reinterpret_cast<uint32_t*>(ap.out.key)[row] = null_key ? 0u : unfmix32((uint32_t)k64);
        else
            reinterpret_cast<unsigned long long*>(ap.out.key)[row] = null_key ? 0ull : unfmix64(k64);
    }
    if (null_key && ap.out_keyvalid) ap.out_keyvalid[row] = 0;
    if (ap.out.rows) ap.out.rows[row] = rows;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        if (c >= ap.n_cols) continue;
        if (ap.out.nn[c]) ap.out.nn[c][row] = nn[c];
        if (ap.out.sum[c]) ap.out.sum[c][row] = sum[c];
        if (ap.out.mn[c]) ap.out.mn[c][row] = mn[c];
        if (ap.out.mx[c]) ap.out.mx[c][row] = mx[c];
    }
}

template <int NC>
struct AggTable {
    unsigned long long key[AGG_CAP];
    uint32_t           rows[AGG_CAP];
    uint32_t           nn[NC][AGG_CAP];
    unsigned long long sum[NC][AGG_CAP];
    long long          mn[NC][AGG_CAP], mx[NC][AGG_CAP];
};

// One workgroup per partition, or per heavy task of a partition above JN_HEAVY tuples.  The LDS
// table is open addressing over AGG_CAP entries, keyed by the hashed key words (64-bit compare and
// swap; the "free" pattern is a key word 0 whose lowest radix bit differs from the partition's, so
// no key of the partition equals it); the accumulators are LDS atomics: 32-bit counts, 64-bit add
// and signed min / max.  The tuples go by in steps of AGG_STEP; between two steps every thread
// reads the table's fill, and from AGG_FREEZE keys on the round is FROZEN: a tuple whose key is
// not in the table (or — before that — that found the AGG_WALK entries from its home taken) is put back into the
// partition's own memory from its start, always behind the read position, and is aggregated in the
// next round with a fresh table.  A key that is in the table catches every later tuple of its
// own, and a key that was turned away once never enters the same round (free entries only
// vanish, and the frozen state only begins at a barrier), so every key is emitted in exactly one
// round.  A partition's main workgroup reserves the rows of all groups of a round at once and
// writes them; a heavy task adds its groups to the merge table in HBM instead (k_agg_emit).
template <int KW, int CW>
__global__ __launch_bounds__(AGG_THREADS) void k_agg_parts(AggParams ap) {
    constexpr int NW = KW + CW, NC = CW ? CW : 1;
    __shared__ AggTable<NC>       T;
    __shared__ uint32_t           s_used, s_ndefer, s_wsum[AGG_THREADS / 64];
    __shared__ unsigned long long s_obase;
    const bool heavy = blockIdx.x < ap.heavy_grid;
    uint32_t   b, e;
    if (heavy) {
        if (blockIdx.x >= *ap.n_heavy) return;
        b = ap.heavy_tasks[3 * blockIdx.x + 1];
        e = ap.heavy_tasks[3 * blockIdx.x + 2];
    } else {
        const uint32_t q = blockIdx.x - ap.heavy_grid;
        if (q >= ap.NP) return;
        b = ap.off[q];
        e = ap.off[q + 1];
        if (e - b > JN_HEAVY) return;  // (its tasks do it)
    }
    if (b >= e) return;
    unsigned long long EMPTY;
    {
        uint32_t t0[NW];
        part_tuple<KW, CW>(ap.W, ap.pack, ap.aos, b, t0);
        EMPTY = (unsigned long long)(t0[0] ^ 1u);
    }
    uint32_t rd_e = e;
    while (true) {
        for (uint32_t i = threadIdx.x; i < AGG_CAP; i += AGG_THREADS) {
            T.key[i] = EMPTY;
            T.rows[i] = 0;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                T.nn[c][i] = 0;
                T.sum[c][i] = 0;
                T.mn[c][i] = AGG_MIN_INIT;
                T.mx[c][i] = AGG_MAX_INIT;
            }
        }
        if (threadIdx.x == 0) {
            s_used = 0;
            s_ndefer = 0;
        }
        __syncthreads();
        for (uint64_t base = b; base < rd_e; base += AGG_STEP) {
            // (nobody changes s_used between the barrier that ended the last step and the next one)
            const bool frozen = *(volatile uint32_t*)&s_used >= (uint32_t)AGG_FREEZE;
            uint32_t   t[AGG_SPT][NW];
            bool       live[AGG_SPT];
#pragma unroll
            for (int j = 0; j < AGG_SPT; ++j) {
                const uint64_t idx = base + (uint64_t)j * AGG_THREADS + threadIdx.x;
                live[j] = idx < rd_e;
                if (live[j]) part_tuple<KW, CW>(ap.W, ap.pack, ap.aos, (uint32_t)idx, t[j]);
            }
            __syncthreads();  // every tuple of the step is in registers before a deferred one lands on it
#pragma unroll
            for (int j = 0; j < AGG_SPT; ++j) {
                if (!live[j]) continue;
                const uint32_t           lo = t[j][0], hi = KW == 2 ? t[j][KW - 1] : 0u;
                const unsigned long long k64 = (unsigned long long)lo | ((unsigned long long)hi << 32);
                uint32_t                 slot = ((lo ^ hi) * 0x9e3779b1u) >> (32 - ilog2_u32(AGG_CAP));
                bool                     found = false;
                for (uint32_t pr = 0; pr < (uint32_t)AGG_WALK; ++pr) {
                    unsigned long long cur = __hip_atomic_load(&T.key[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (cur == EMPTY && !frozen) {
                        cur = atomicCAS(&T.key[slot], EMPTY, k64);
                        if (cur == EMPTY) {
                            atomicAdd(&s_used, 1u);
                            cur = k64;
                        }
                    }
                    if (cur == k64) {
                        found = true;
                        break;
                    }
                    if (cur == EMPTY) break;  // frozen, and the key is not in the table
                    slot = (slot + 1u) & (uint32_t)(AGG_CAP - 1);
                }
                if (!found) {
                    const uint32_t pos = atomicAdd(&s_ndefer, 1u);
                    part_tuple_store<KW, CW>(ap.W, ap.pack, ap.aos, b + pos, t[j]);
                    continue;
                }
                atomicAdd(&T.rows[slot], 1u);
                if constexpr (CW >= 1) {
                    const uint32_t c0 = t[j][KW], c1 = CW >= 2 ? t[j][KW + (CW >= 2 ? 1 : 0)] : 0u,
                                   c2 = CW >= 3 ? t[j][KW + (CW >= 3 ? 2 : 0)] : 0u;
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        long long v;
                        if (c >= ap.n_cols || !agg_value(ap.col[c], ap.valid_word, c0, c1, c2, v)) continue;
                        atomicAdd(&T.nn[c][slot], 1u);
                        if (ap.col[c].need & AGG_NEED_SUM) atomicAdd(&T.sum[c][slot], (unsigned long long)v);
                        if (ap.col[c].need & AGG_NEED_MIN) atomicMin(&T.mn[c][slot], v);
                        if (ap.col[c].need & AGG_NEED_MAX) atomicMax(&T.mx[c][slot], v);
                    }
                }
            }
            __syncthreads();
        }
        // ---- the round's groups
        constexpr int      EPT = AGG_CAP / AGG_THREADS;
        uint32_t           cnt = 0;
#pragma unroll
        for (int k = 0; k < EPT; ++k) cnt += T.key[threadIdx.x + k * AGG_THREADS] != EMPTY;
        uint64_t row = 0;
        if (!heavy) {
            uint32_t       total;
            const uint32_t pre = block_excl_scan(cnt, s_wsum, total);
            if (threadIdx.x == 0) s_obase = total ? atomicAdd(ap.out_cursor, (unsigned long long)total) : 0ull;
            __syncthreads();
            row = s_obase + pre;
        }
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
            const uint32_t           i = threadIdx.x + k * AGG_THREADS;
            const unsigned long long k64 = T.key[i];
            if (k64 == EMPTY) continue;
            unsigned long long nn[NC], sum[NC];
            long long          mn[NC], mx[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                nn[c] = T.nn[c][i];
                sum[c] = T.sum[c][i];
                mn[c] = T.mn[c][i];
                mx[c] = T.mx[c][i];
            }
            if (heavy)
                agg_merge<NC>(ap, agg_merge_entry(ap, k64), T.rows[i], nn, sum, mn, mx);
            else
                agg_write<KW, NC>(ap, row++, k64, false, T.rows[i], nn, sum, mn, mx);
        }
        const uint32_t nd = *(volatile uint32_t*)&s_ndefer;
        if (nd == 0) break;
        // the deferred tuples, written by any thread of the workgroup, are read by any other next round
        __threadfence();
        __syncthreads();
        __threadfence();
        rd_e = b + nd;
    }
}

// The rows whose key is NULL: the first radix pass drops them; they form one group (SQL's GROUP BY),
// entry m_slots + 1 of the merge table.  Grid-strided over the child's columns, per-thread
// accumulators, a wave reduction, one set of atomics per wave that saw such a row.
template <int CW>
__global__ __launch_bounds__(JN_THREADS) void k_agg_nullkey(AggParams ap) {
    constexpr int      NC = CW ? CW : 1;
    unsigned long long rows = 0, nn[NC], sum[NC];
    long long          mn[NC], mx[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        nn[c] = sum[c] = 0;
        mn[c] = AGG_MIN_INIT;
        mx[c] = AGG_MAX_INIT;
    }
    const uint32_t n = ap.src.n_rows;
    for (uint64_t r = (uint64_t)blockIdx.x * JN_THREADS + threadIdx.x; r < n; r += (uint64_t)gridDim.x * JN_THREADS) {
        if (ap.src.key.valid[r]) continue;
        ++rows;
        if constexpr (CW >= 1) {
            uint32_t c0, c1, c2;
            src_carry<CW>(ap.src, (uint32_t)r, c0, c1, c2);
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                long long v;
                if (c >= ap.n_cols || !agg_value(ap.col[c], ap.valid_word, c0, c1, c2, v)) continue;
                ++nn[c];
                sum[c] += (unsigned long long)v;
                mn[c] = min(mn[c], v);
                mx[c] = max(mx[c], v);
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        rows += __shfl_xor(rows, off);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            nn[c] += __shfl_xor(nn[c], off);
            sum[c] += __shfl_xor(sum[c], off);
            mn[c] = min(mn[c], __shfl_xor(mn[c], off));
            mx[c] = max(mx[c], __shfl_xor(mx[c], off));
        }
    }
    if ((threadIdx.x & 63u) == 0 && rows) agg_merge<NC>(ap, ap.m_slots + 1u, rows, nn, sum, mn, mx);
}

// the merge table before anybody adds to it
__global__ __launch_bounds__(256) void k_agg_merge_init(AggParams ap) {
    const uint64_t n = (uint64_t)ap.m_slots + 2;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        reinterpret_cast<unsigned long long*>(ap.m.key)[i] = AGG_NO_KEY;
        ap.m.rows[i] = 0;
        for (int c = 0; c < ap.n_cols; ++c) {
            ap.m.nn[c][i] = 0;
            ap.m.sum[c][i] = 0;
            ap.m.mn[c][i] = AGG_MIN_INIT;
            ap.m.mx[c][i] = AGG_MAX_INIT;
        }
    }
}

// The live entries of the merge table -> rows of the output, through the same cursor as
// k_agg_parts: one reservation per 256 entries.  The NULL-key group's key comes out NULL.
template <int KW>
__global__ __launch_bounds__(256) void k_agg_emit(AggParams ap) {
    __shared__ uint32_t           s_wsum[256 / 64];
    __shared__ unsigned long long s_obase;
    const uint64_t n = (uint64_t)ap.m_slots + 2;
    for (uint64_t base = (uint64_t)blockIdx.x * 256; base < n; base += (uint64_t)gridDim.x * 256) {
        const uint64_t i = base + threadIdx.x;
        const bool     live = i < n && ap.m.rows[i] != 0;
        uint32_t       total;
        const uint32_t pre = block_excl_scan(live ? 1u : 0u, s_wsum, total);
        if (threadIdx.x == 0) s_obase = total ? atomicAdd(ap.out_cursor, (unsigned long long)total) : 0ull;
        __syncthreads();
        if (live) {
            unsigned long long nn[AGG_MAX_COLS], sum[AGG_MAX_COLS];
            long long          mn[AGG_MAX_COLS], mx[AGG_MAX_COLS];
#pragma unroll
            for (int c = 0; c < AGG_MAX_COLS; ++c) {
                const bool has = c < ap.n_cols;
                nn[c] = has ? ap.m.nn[c][i] : 0;
                sum[c] = has ? ap.m.sum[c][i] : 0;
                mn[c] = has ? ap.m.mn[c][i] : 0;
                mx[c] = has ? ap.m.mx[c][i] : 0;
            }
            const unsigned long long k64 = i < ap.m_slots ? reinterpret_cast<const unsigned long long*>(ap.m.key)[i] : AGG_NO_KEY;
            agg_write<KW, AGG_MAX_COLS>(ap, s_obase + pre, k64, i == (uint64_t)ap.m_slots + 1, ap.m.rows[i], nn, sum, mn, mx);
        }
        __syncthreads();
    }
}

// An accumulator array as a result column: narrowed to 32 bits for an INT32 MIN / MAX (dst,
// optional), and NULL where the group had no value (dst_valid, optional; nn = nullptr: never).
template <int WIDTH>
__global__ __launch_bounds__(256) void k_agg_column(const unsigned long long* src, const unsigned long long* nn, uint64_t n,
                                                    uint8_t* dst, uint8_t* dst_valid) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (dst) {
        if (WIDTH == 4)
            reinterpret_cast<uint32_t*>(dst)[i] = (uint32_t)src[i];
        else
            reinterpret_cast<unsigned long long*>(dst)[i] = src[i];
    }
    if (dst_valid) dst_valid[i] = nn ? (nn[i] != 0) : 1;
}

// ================================================================== selection
// RJ_NODE_SELECT: the predicate program of rj_device.hpp (SelectProg) over a relation's columns, the
// row ids of the rows it keeps compacted into out_ids.  The program is the same for every row, so the
// op loop, the stack pointer and every branch on an op are uniform and ops[k] is read with scalar
// loads; a row's stack is one 64-bit register of bits, as in k_ing_filter (the host checked the
// depth: at most 60).  A thread evaluates SEL_BATCH rows op by op, so that the loads of one leaf are
// in flight together, and keeps one bit per row it owns in the tile (SEL_ITEMS of them).  Wave w owns
// the w-th quarter of the tile, 64 consecutive rows per item: ranks come from a ballot per item and a
// prefix over the four wave totals in LDS, the tile reserves its range of out_ids with ONE atomic on
// the cursor and writes its ids in ascending order.  The tile is large because that atomic is the
// scarce resource: every workgroup of the grid adds to the same address.
template <class T>
__device__ __forceinline__ bool sel_cmp(int cmp, T x, T y) {
    switch (cmp) {
    case 0: return x == y;
    case 1: return x != y;
    case 2: return x < y;
    case 3: return x > y;
    case 4: return x <= y;
    default: return x >= y;
    }
}
// a leaf on one row: a comparison is false when an operand is NULL; doubles compare IEEE-wise
__device__ __forceinline__ bool sel_leaf(const SelectOp& o, uint32_t row) {
    bool nn = o.a.valid ? o.a.valid[row] != 0 : true;
    if (o.kind == SEL_IS_NULL) return !nn;
    if (o.kind == SEL_NOT_NULL) return nn;
    const bool col = o.kind == SEL_COL;
    if (col && o.b.valid) nn = nn && o.b.valid[row] != 0;
    if (o.a.width == 4) {
        const int64_t x = (int32_t)col_load32(o.a, row);
        const int64_t y = col ? (int64_t)(int32_t)col_load32(o.b, row) : o.literal;
        return nn && sel_cmp(o.cmp, x, y);
    }
    const uint64_t xb = col_load64(o.a, row);
    const uint64_t yb = col ? col_load64(o.b, row) : (uint64_t)o.literal;
    if (o.f64) return nn && sel_cmp(o.cmp, __longlong_as_double((long long)xb), __longlong_as_double((long long)yb));
    return nn && sel_cmp(o.cmp, (int64_t)xb, (int64_t)yb);
}

__global__ __launch_bounds__(SEL_THREADS) void k_select(const SelectProg* __restrict__ prog, uint32_t n_ops, uint32_t n_rows,
                                                        uint32_t* __restrict__ out_ids, unsigned long long* cursor) {
    constexpr uint32_t NWAVES = SEL_THREADS / 64, WAVE_ROWS = SEL_TILE / NWAVES;
    __shared__ uint32_t s_wtot[NWAVES];
    __shared__ uint32_t s_base;
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    const uint32_t n_tiles = n_rows / SEL_TILE + (n_rows % SEL_TILE != 0);  // (n_rows + SEL_TILE - 1 may not fit 32 bits)
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t tile_base = tile * SEL_TILE;  // (< n_rows)
        const uint32_t in_tile = min((uint32_t)SEL_TILE, n_rows - tile_base);
        const uint32_t local0 = wid * WAVE_ROWS + lane;  // item i: row tile_base + local0 + 64 i
        uint32_t       keep = 0, wtot = 0;               // bit i: item i passed; the wave's rows that passed
#pragma unroll 1
        for (uint32_t b = 0; b < SEL_ITEMS; b += SEL_BATCH) {
            if (wid * WAVE_ROWS + 64u * b >= in_tile) break;  // (the same for the whole wave)
            uint64_t st[SEL_BATCH];
#pragma unroll
            for (int j = 0; j < SEL_BATCH; ++j) st[j] = 0;
            uint32_t sp = 0;
            for (uint32_t k = 0; k < n_ops; ++k) {
                const SelectOp& o = prog->ops[k];
                if (o.kind == SEL_AND || o.kind == SEL_OR) {
                    sp -= 2;
#pragma unroll
                    for (int j = 0; j < SEL_BATCH; ++j) {
                        const uint64_t x = (st[j] >> sp) & 1u, y = (st[j] >> (sp + 1)) & 1u;
                        st[j] = (st[j] & ((1ull << sp) - 1ull)) | ((o.kind == SEL_AND ? (x & y) : (x | y)) << sp);
                    }
                    ++sp;
                } else if (o.kind == SEL_NOT) {
#pragma unroll
                    for (int j = 0; j < SEL_BATCH; ++j) st[j] ^= 1ull << (sp - 1);
                } else {
#pragma unroll
                    for (int j = 0; j < SEL_BATCH; ++j) {
                        const uint32_t local = local0 + 64u * (b + j);
                        const uint64_t v = local < in_tile && sel_leaf(o, tile_base + local);
                        st[j] |= v << sp;
                    }
                    ++sp;
                }
            }
#pragma unroll
            for (int j = 0; j < SEL_BATCH; ++j) {
                const bool pass = local0 + 64u * (b + j) < in_tile && (st[j] & 1u);
                keep |= (uint32_t)pass << (b + j);
                wtot += (uint32_t)__popcll(__ballot(pass));
            }
        }
        // ranks: item by item inside the wave (below), over the waves here; ONE reservation per tile
        if (lane == 0) s_wtot[wid] = wtot;
        __syncthreads();
        uint32_t wbase = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < NWAVES; ++w) {
            const uint32_t t = s_wtot[w];
            if (w < wid) wbase += t;
            total += t;
        }
        if (threadIdx.x == 0 && total) s_base = (uint32_t)atomicAdd(cursor, (unsigned long long)total);
        __syncthreads();
        if (wtot) {  // (the same for the whole wave)
            uint32_t pos = s_base + wbase;
#pragma unroll 4
            for (uint32_t i = 0; i < SEL_ITEMS; ++i) {
                const bool     pass = (keep >> i) & 1u;
                const uint64_t mask = __ballot(pass);
                if (pass) out_ids[pos + lane_prefix(mask)] = tile_base + local0 + 64u * i;
                pos += (uint32_t)__popcll(mask);
            }
        }
    }
}

// ================================================================== launchers
void launch_page_headers(const Launch& L, const uint8_t* pages, uint32_t n_pages, uint32_t rows_full,
                         uint32_t* page_rows, unsigned long long* flags) {
    if (!n_pages) return;
    RJ_KLAUNCH(L, "page_headers", k_page_headers, std::min<uint32_t>((n_pages + 3) / 4, 8192u), 256, pages, n_pages,
               rows_full, page_rows, flags);
}

void launch_rows_beyond(const Launch& L, const uint8_t* pages, uint32_t n_pages,
                        const uint32_t* row_base, uint64_t num_rows, unsigned long long* flag) {
    if (!n_pages) return;
    RJ_KLAUNCH(L, "rows_beyond", k_rows_beyond, (n_pages + 3) / 4, 256, pages, n_pages, row_base,
               num_rows, flag);
}

void launch_decode_pages(const Launch& L, const uint8_t* pages, uint32_t n_pages, int width,
                         const uint32_t* row_base, uint64_t num_rows, uint8_t* values,
                         uint8_t* valid) {
    if (!n_pages) return;
    if (width == 4)
        RJ_KLAUNCH(L, "decode_pages", (k_decode_pages<4>), n_pages, 256, pages, row_base, num_rows,
                   values, valid);
    else
        RJ_KLAUNCH(L, "decode_pages", (k_decode_pages<8>), n_pages, 256, pages, row_base, num_rows,
                   values, valid);
}

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
                          uint32_t n_groups, const Words& out) {
    SrcLoader<KW, CW, WIDE> ld{src};
    RJ_KLAUNCH(L, "pass1_scatter", (k_pass_scatter<KW + CW, SrcLoader<KW, CW, WIDE>, (CW >= 2 ? KW + CW - 2 : -1), false>),
               n_groups, PT_THREADS, ld, pp, out);
}

void launch_pass_scatter_src(const Launch& L, const TupleSrc& src, int key_words, int carry_words,
                             const PassParams& pp, uint32_t n_groups, const Words& out, bool aos3) {
    if (!n_groups) return;
    const int wide = src.carry_mode == CARRY_WIDE ? src.wide : WIDE_NONE;
    if (aos3) {
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
        case 121: scatter_src_t<1, 2, WIDE_32S>(L, src, pp, n_groups, out); break;
        case 131: scatter_src_t<1, 3, WIDE_32S>(L, src, pp, n_groups, out); break;
        case 132: scatter_src_t<1, 3, WIDE_64_32>(L, src, pp, n_groups, out); break;
        case 221: scatter_src_t<2, 2, WIDE_32S>(L, src, pp, n_groups, out); break;
        default: launch_failed("pass1_scatter", "no kernel for this wide carry layout", true);
        }
        return;
    }
    for_shape("pass1_scatter", key_words, carry_words, [&](auto KW, auto CW) {
        if constexpr (CW <= 2)  // (three carry words travel only as a wide carry, above)
            scatter_src_t<KW, CW>(L, src, pp, n_groups, out);
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
                                    uint32_t n_groups, uint32_t* out_pairs, bool blocked_out) {
    if (!n_groups) return;
    SrcLoader<1, 1> ld{src};
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

void launch_heavy_tasks(const Launch& L, const uint32_t* offR, const uint32_t* offS, uint32_t NP,
                        uint32_t* tasks, uint32_t* n_heavy, uint32_t max_tasks) {
    RJ_KLAUNCH(L, "heavy_tasks", k_heavy_tasks, (NP + 255) / 256, 256, offR, offS, NP, tasks,
               n_heavy, max_tasks);
}

void launch_join_bcast(const Launch& L, int key_words, int cw_build, int cw_probe,
                       const BcastParams& bp, uint32_t grid) {
    if (!grid) return;
    for_shape2("join_broadcast", key_words, cw_build, cw_probe, [&](auto KW, auto CWR, auto CWS) {
        RJ_KLAUNCH(L, "join_broadcast", (k_join_bcast<KW, CWR, CWS>), grid, JN_THREADS, bp);
    });
}

// semi / anti joins: the preserved side's carry
void launch_filter_bcast(const Launch& L, int key_words, int cw_preserved, const FilterParams& fp, uint32_t grid) {
    if (!grid) return;
    for_shape("filter_broadcast", key_words, cw_preserved, [&](auto KW, auto CW) {
        RJ_KLAUNCH(L, "filter_broadcast", (k_filter_bcast<KW, CW>), grid, JN_THREADS, fp);
    });
}

void launch_filter_join(const Launch& L, int key_words, int cw_preserved, const FilterParams& fp, uint32_t grid) {
    if (!grid) return;
    for_shape("filter_probe", key_words, cw_preserved, [&](auto KW, auto CW) {
        RJ_KLAUNCH(L, "filter_probe", (k_filter_join<KW, CW>), grid, JN_THREADS, fp);
    });
}

void launch_filter_nullkeys(const Launch& L, int key_words, int cw_preserved, const FilterParams& fp, uint32_t grid) {
    if (!grid) return;
    for_shape("filter_nullkeys", key_words, cw_preserved, [&](auto KW, auto CW) {
        RJ_KLAUNCH(L, "filter_nullkeys", (k_filter_nullkeys<KW, CW>), grid, JN_THREADS, fp);
    });
}

void launch_outer_gather(const Launch& L, const ColRef& src, const uint32_t* idx, uint64_t n, uint8_t* dst,
                         uint8_t* dst_valid) {
    if (!n) return;
    const uint32_t grid = (uint32_t)((n + 255) / 256);
    if (src.width == 4)
        RJ_KLAUNCH(L, "outer_gather", (k_outer_gather<4>), grid, 256, src, idx, n, dst, dst_valid);
    else
        RJ_KLAUNCH(L, "outer_gather", (k_outer_gather<8>), grid, 256, src, idx, n, dst, dst_valid);
}

void launch_debug_stall(const Launch& L, uint32_t ms) {
    int dev = 0, khz = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) khz = 100000;
    RJ_KLAUNCH(L, "debug_stall", k_debug_stall, 1, 64, (unsigned long long)ms * (unsigned long long)khz);
}

void launch_pack_validity(const Launch& L, const uint8_t* v0, const uint8_t* v1, const uint8_t* v2, uint32_t n,
                          uint32_t* out) {
    if (!n) return;
    RJ_KLAUNCH(L, "pack_validity", k_pack_validity, (n + 255) / 256, 256, v0, v1, v2, n, out);
}

void launch_split_records(const Launch& L, const SplitParams& sp, uint64_t n) {
    if (!n) return;
    RJ_KLAUNCH(L, "split_records", k_split_records, (uint32_t)((n + 255) / 256), 256, sp, n);
}

void launch_gather(const Launch& L, const ColRef& src, const uint32_t* idx, uint64_t n,
                   const OutStream& dst, uint8_t* dst_valid) {
    if (!n) return;
    uint32_t grid = (uint32_t)((n + 255) / 256);
    if (src.width == 4)
        RJ_KLAUNCH(L, "gather", (k_gather<4>), grid, 256, src, idx, n, dst, dst_valid);
    else
        RJ_KLAUNCH(L, "gather", (k_gather<8>), grid, 256, src, idx, n, dst, dst_valid);
}

void launch_finish_pages(const Launch& L, uint8_t* pages, uint64_t n_rows, int width) {
    if (!n_rows) return;
    uint32_t rf = width == 4 ? ROWS32 : ROWS64;
    uint32_t np = (uint32_t)((n_rows + rf - 1) / rf);
    RJ_KLAUNCH(L, "finish_pages", k_finish_pages, np, 256, pages, n_rows, rf);
}

void launch_finish_streams(const Launch& L, uint8_t* const* pages, const int* widths, uint32_t n,
                           const unsigned long long* n_rows_dev, uint64_t cap_rows) {
    if (!n || !cap_rows) return;
    FinishStreams fs{};
    fs.n = n;
    uint64_t max_pages = 0;
    for (uint32_t i = 0; i < n && i < 3; ++i) {
        fs.pages[i] = pages[i];
        fs.rows_full[i] = widths[i] == 4 ? ROWS32 : ROWS64;
        max_pages = std::max<uint64_t>(max_pages, (cap_rows + fs.rows_full[i] - 1) / fs.rows_full[i]);
    }
    RJ_KLAUNCH(L, "finish_pages", k_finish_streams, dim3((uint32_t)((max_pages + 3) / 4), n), 256, fs,
               n_rows_dev, cap_rows);
}

void launch_encode_nullable(const Launch& L, const uint8_t* values, const uint8_t* valid,
                            uint64_t n_rows, int width, uint8_t* pages) {
    if (!n_rows) return;
    uint32_t rf = width == 4 ? ROWS32 : ROWS64;
    uint32_t np = (uint32_t)((n_rows + rf - 1) / rf);
    if (width == 4)
        RJ_KLAUNCH(L, "encode_nullable", (k_encode_nullable<4>), np, 256, values, valid, n_rows,
                   pages);
    else
        RJ_KLAUNCH(L, "encode_nullable", (k_encode_nullable<8>), np, 256, values, valid, n_rows,
                   pages);
}

// ---- aggregation
void launch_agg_merge_init(const Launch& L, const AggParams& ap, uint32_t grid) {
    RJ_KLAUNCH(L, "agg_merge_init", k_agg_merge_init, grid, 256, ap);
}
void launch_agg_parts(const Launch& L, int key_words, int carry_words, const AggParams& ap, uint32_t grid) {
    if (!grid) return;
    for_shape("agg_parts", key_words, carry_words, [&](auto KW, auto CW) {
        RJ_KLAUNCH(L, "agg_parts", (k_agg_parts<KW, CW>), grid, AGG_THREADS, ap);
    });
}
void launch_agg_nullkey(const Launch& L, int carry_words, const AggParams& ap, uint32_t grid) {
    if (!grid) return;
    for_shape("agg_nullkey", 1, carry_words, [&](auto, auto CW) {  // (no key: the carries of a one-word key)
        RJ_KLAUNCH(L, "agg_nullkey", (k_agg_nullkey<CW>), grid, JN_THREADS, ap);
    });
}
void launch_agg_emit(const Launch& L, int key_words, const AggParams& ap, uint32_t grid) {
    if (key_words == 1)
        RJ_KLAUNCH(L, "agg_emit", (k_agg_emit<1>), grid, 256, ap);
    else
        RJ_KLAUNCH(L, "agg_emit", (k_agg_emit<2>), grid, 256, ap);
}
void launch_agg_column(const Launch& L, const unsigned long long* src, const unsigned long long* nn, uint64_t n, int width,
                       uint8_t* dst, uint8_t* dst_valid) {
    if (!n) return;
    const uint32_t grid = (uint32_t)((n + 255) / 256);
    if (width == 4)
        RJ_KLAUNCH(L, "agg_column", (k_agg_column<4>), grid, 256, src, nn, n, dst, dst_valid);
    else
        RJ_KLAUNCH(L, "agg_column", (k_agg_column<8>), grid, 256, src, nn, n, dst, dst_valid);
}

// ---- selection
void launch_select(const Launch& L, const SelectProg* prog, uint32_t n_ops, uint32_t n_rows, uint32_t* out_ids,
                   unsigned long long* cursor, uint32_t grid) {
    if (!n_rows || !grid) return;
    RJ_KLAUNCH(L, "select", k_select, grid, SEL_THREADS, prog, n_ops, n_rows, out_ids, cursor);
}

// RJ_CTX_PREWARM: one harmless launch, so that HIP loads this translation unit's code object when the context is
// built (as prewarm_varchar_dev does).  NP = 0: every thread of k_heavy_tasks leaves at `q >= NP`, its first check,
// before any pointer is read.
void prewarm_kernels(const Launch& L, uint32_t* zeroed) {
    RJ_KLAUNCH(L, "prewarm", k_heavy_tasks, 1, 256, zeroed, zeroed, 0u, zeroed, zeroed, 0u);
}

}  // namespace rj
