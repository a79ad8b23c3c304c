// rj_pages.hip — gfx950 (wave64) kernels that read and write Page images, on either end of every plan:
// K0 page headers and K1 page decode (the upload of a table), K7 gather, K8 page finishing and encoding (the result
// columns of every node kind), the validity word and the record split of the wide carries (the join node kinds),
// and the stall test hook.
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

void launch_gather(const Launch& L, const ColRef& src, const uint32_t* idx, uint64_t n,
                   const OutStream& dst, uint8_t* dst_valid) {
    if (!n) return;
    uint32_t grid = (uint32_t)((n + 255) / 256);
    if (src.width == 4)
        RJ_KLAUNCH(L, "gather", (k_gather<4>), grid, 256, src, idx, n, dst, dst_valid);
    else
        RJ_KLAUNCH(L, "gather", (k_gather<8>), grid, 256, src, idx, n, dst, dst_valid);
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

void launch_pack_validity(const Launch& L, const uint8_t* v0, const uint8_t* v1, const uint8_t* v2, uint32_t n,
                          uint32_t* out) {
    if (!n) return;
    RJ_KLAUNCH(L, "pack_validity", k_pack_validity, (n + 255) / 256, 256, v0, v1, v2, n, out);
}

void launch_split_records(const Launch& L, const SplitParams& sp, uint64_t n) {
    if (!n) return;
    RJ_KLAUNCH(L, "split_records", k_split_records, (uint32_t)((n + 255) / 256), 256, sp, n);
}

void launch_debug_stall(const Launch& L, uint32_t ms) {
    int dev = 0, khz = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) khz = 100000;
    RJ_KLAUNCH(L, "debug_stall", k_debug_stall, 1, 64, (unsigned long long)ms * (unsigned long long)khz);
}

// RJ_CTX_PREWARM: one harmless launch, so that HIP loads this translation unit's code object when the context is
// built.  n = 0: every thread of k_pack_validity leaves at `i >= n`, its first check, before any pointer is read.
void prewarm_pages(const Launch& L, uint32_t* zeroed) {
    const uint8_t* const v = reinterpret_cast<const uint8_t*>(zeroed);
    RJ_KLAUNCH(L, "prewarm", k_pack_validity, 1, 256, v, v, v, 0u, zeroed);
}

}  // namespace rj
