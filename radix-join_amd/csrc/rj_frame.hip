// rj_frame.hip — the gfx950 (wave64) kernels of RJ_NODE_WINDOW's frame layer and their launchers: ROWS
// frames, LAG / LEAD / FIRST_VALUE / LAST_VALUE and NTILE on top of the order, the head masks and the
// scans of rj_window.hip.
#include <algorithm>
#include <vector>

#include "rj_frame.hpp"
#include "rj_group_util.hpp"
#include "rj_kernel_util.hpp"
#include "rj_sortkey.hpp"

namespace rj {

// Every kernel here has one thread per position of the order (geometry and structs: rj_device.hpp); the
// position's partition [ps, pe] comes from FrameRows, its frame from frame_bounds (rj_frame.hpp).
//   k_frame_pick<W>   LAG / LEAD / FIRST_VALUE / LAST_VALUE: the value at one end of the frame, gathered
//                     through the permutation with its validity
//   k_frame_ntile     NTILE from ps and pe
//   k_frame_sum       ROWS COUNT(*) / COUNT / SUM: the difference of two entries of k_win_scan's arrays
//   k_frame_leaves<W> the range-extreme tree of one value column under MIN or MAX: levels 0, 1 and 2
//   k_frame_levels    ... two more levels from the last one built
//   k_frame_extreme   ROWS MIN / MAX: the tree over [a, b], the ragged ends at each level and whole
//                     blocks above; the non-NULL count (the scan's) decides NULL
// No workgroup waits for another: a level is read by the launch after the one that wrote it.  Every word
// these kernels read was written by an earlier launch of the same node.

__device__ __forceinline__ void frame_partition(const FrameRows& rows, uint64_t i, uint64_t& ps, uint64_t& pe) {
    ps = i + 1u - rows.row_number[i];
    pe = rows.part_end[i];
}

// end = FramePick; lo, hi: the frame (LAG k: -k, -k; LEAD k: k, k).  The value's own bits, 0 for a NULL.
template <int W>
__global__ __launch_bounds__(256) void k_frame_pick(ColRef col, const uint32_t* __restrict__ perm, uint32_t n_rows, FrameRows rows,
                                                    int64_t lo, int64_t hi, int32_t end, uint8_t* __restrict__ dst,
                                                    uint8_t* __restrict__ dst_valid) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_rows) return;
    uint64_t ps, pe, a, b;
    frame_partition(rows, i, ps, pe);
    uint64_t bits = 0;
    bool     valid = false;
    if (frame_bounds(i, ps, pe, lo, hi, a, b)) {
        const uint64_t s = end == FRAME_FIRST ? a : b;
        const uint32_t r = perm ? perm[s] : (uint32_t)s;
        valid = !(col.valid && !col.valid[r]);
        if (valid) bits = group_load<W>(col, r);
    }
    if constexpr (W == 4)
        reinterpret_cast<uint32_t*>(dst)[i] = (uint32_t)bits;
    else
        reinterpret_cast<uint64_t*>(dst)[i] = bits;
    dst_valid[i] = valid ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_frame_ntile(uint32_t n_rows, FrameRows rows, int64_t buckets, unsigned long long* __restrict__ dst) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_rows) return;
    uint64_t ps, pe;
    frame_partition(rows, i, ps, pe);
    dst[i] = (unsigned long long)frame_ntile(i - ps, pe - ps + 1u, buckets);
}

// what = FrameSum.  nn / sum: the partition-segmented inclusive running count and sum (k_win_scan); an
// empty frame reads neither.  dst_valid (optional): the frame has a non-NULL value.
__global__ __launch_bounds__(256) void k_frame_sum(const uint32_t* __restrict__ nn, const unsigned long long* __restrict__ sum, uint32_t n_rows,
                                                   FrameRows rows, int64_t lo, int64_t hi, int32_t what, unsigned long long* __restrict__ dst,
                                                   uint8_t* __restrict__ dst_valid) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_rows) return;
    uint64_t ps, pe, a, b;
    frame_partition(rows, i, ps, pe);
    uint64_t v = 0;
    bool     valid = false;
    if (frame_bounds(i, ps, pe, lo, hi, a, b)) {
        if (what == FRAME_COUNT_STAR) {
            v = b - a + 1u;
            valid = true;
        } else {
            const uint32_t cnt = nn[b] - (a > ps ? nn[a - 1u] : 0u);
            valid = cnt != 0;
            if (what == FRAME_COUNT)
                v = cnt;
            else if (valid)
                v = sum[b] - (a > ps ? sum[a - 1u] : 0ull);
        }
    }
    dst[i] = v;
    if (dst_valid) dst_valid[i] = valid ? 1 : 0;
}

__device__ __forceinline__ uint64_t frame_op(uint64_t x, uint64_t y, bool is_max) { return is_max ? max(x, y) : min(x, y); }
__device__ __forceinline__ uint64_t frame_identity(bool is_max) { return is_max ? 0ull : ~0ull; }

// Words v of one level, one per thread of the workgroup (the identity behind the level's end; first =
// the workgroup's first word, n_in = the level's length) -> the level above (up1, n_in / FRAME_FANOUT
// rounded up words) and the one above that (up2, optional: one word per workgroup).  Every thread of
// the workgroup calls it.
__device__ __forceinline__ void frame_two_levels(uint64_t v, uint64_t first, uint64_t n_in, bool is_max, unsigned long long* __restrict__ up1,
                                                 unsigned long long* __restrict__ up2) {
    __shared__ unsigned long long s[FRAME_FANOUT];
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
#pragma unroll
    for (int m = 1; m < FRAME_FANOUT; m <<= 1) v = frame_op(v, __shfl_xor(v, m), is_max);
    const uint64_t mine = first + threadIdx.x;
    if ((lane & (FRAME_FANOUT - 1u)) == 0) {
        if (mine < n_in) up1[mine / FRAME_FANOUT] = v;
        s[threadIdx.x / FRAME_FANOUT] = v;
    }
    if (!up2) return;  // (uniform over the launch)
    __syncthreads();
    if (wid == 0) {
        uint64_t x = lane < (uint32_t)FRAME_FANOUT ? s[lane] : frame_identity(is_max);
#pragma unroll
        for (int m = 1; m < FRAME_FANOUT; m <<= 1) x = frame_op(x, __shfl_xor(x, m), is_max);
        if (lane == 0) up2[blockIdx.x] = x;
    }
}

// Level 0: the encoded value (sort_key_bits, ascending) at every position, the identity for a NULL; and
// the two levels above it (up1 optional too: a relation of at most FRAME_FANOUT rows has level 0 only).
template <int W>
__global__ __launch_bounds__(FRAME_THREADS) void k_frame_leaves(ColRef col, const uint32_t* __restrict__ perm, uint32_t n_rows, int32_t f64,
                                                                int32_t is_max, unsigned long long* __restrict__ level0,
                                                                unsigned long long* __restrict__ up1, unsigned long long* __restrict__ up2) {
    const uint64_t first = (uint64_t)blockIdx.x * FRAME_THREADS, i = first + threadIdx.x;
    uint64_t       v = frame_identity(is_max != 0);
    if (i < n_rows) {
        const uint32_t r = perm ? perm[i] : (uint32_t)i;
        if (!(col.valid && !col.valid[r])) v = sort_key_bits(group_load<W>(col, r), W, f64 != 0, false);
        level0[i] = v;
    }
    if (!up1) return;  // (uniform over the launch)
    frame_two_levels(v, first, n_rows, is_max != 0, up1, up2);
}

__global__ __launch_bounds__(FRAME_THREADS) void k_frame_levels(const unsigned long long* __restrict__ in, uint64_t n_in, int32_t is_max,
                                                                unsigned long long* __restrict__ up1, unsigned long long* __restrict__ up2) {
    const uint64_t first = (uint64_t)blockIdx.x * FRAME_THREADS, i = first + threadIdx.x;
    frame_two_levels(i < n_in ? in[i] : frame_identity(is_max != 0), first, n_in, is_max != 0, up1, up2);
}

// tree: the levels one behind the other, level 0 = n_rows words.  The walk: at a level of more than
// FRAME_FANOUT words the words of [l, h) in front of the first and behind the last block border are
// taken one by one, what is left is whole blocks = a range of the level above; the top level is walked
// word by word.  The result: decoded (GroupDecode), narrowed to `width` bytes, 0 for a NULL.
__global__ __launch_bounds__(256) void k_frame_extreme(const unsigned long long* __restrict__ tree, const uint32_t* __restrict__ nn,
                                                       uint32_t n_rows, FrameRows rows, int64_t lo, int64_t hi, int32_t is_max, int32_t decode,
                                                       int32_t width, uint8_t* __restrict__ dst, uint8_t* __restrict__ dst_valid) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_rows) return;
    constexpr uint64_t F = FRAME_FANOUT;
    uint64_t           ps, pe, a, b;
    frame_partition(rows, i, ps, pe);
    uint64_t v = 0;
    bool     valid = false;
    if (frame_bounds(i, ps, pe, lo, hi, a, b)) valid = nn[b] - (a > ps ? nn[a - 1u] : 0u) != 0;
    if (valid) {
        const bool mx = is_max != 0;
        uint64_t   l = a, h = b + 1u, len = n_rows, x = frame_identity(mx);
        const unsigned long long* level = tree;
        while (len > F) {
            while ((l & (F - 1u)) != 0 && l < h) x = frame_op(x, level[l++], mx);
            while ((h & (F - 1u)) != 0 && l < h) x = frame_op(x, level[--h], mx);
            if (l >= h) break;
            l /= F, h /= F;
            level += len;
            len = (len + F - 1u) / F;
        }
        for (; l < h; ++l) x = frame_op(x, level[l], mx);  // (the top level, or nothing)
        v = sort_key_value(x, decode == GROUP_KEY32 ? 4 : 8, decode == GROUP_KEYF64, false);
    }
    if (width == 4)
        reinterpret_cast<uint32_t*>(dst)[i] = (uint32_t)v;
    else
        reinterpret_cast<uint64_t*>(dst)[i] = v;
    if (dst_valid) dst_valid[i] = valid ? 1 : 0;
}

// ================================================================== launchers
static uint32_t frame_grid(uint64_t n) { return (uint32_t)((n + 255u) / 256u); }

uint64_t frame_tree_words(uint64_t n_rows) {
    uint64_t words = n_rows;
    for (uint64_t len = n_rows; len > (uint64_t)FRAME_FANOUT;) {
        len = (len + FRAME_FANOUT - 1u) / FRAME_FANOUT;
        words += len;
    }
    return words;
}

void launch_frame_pick(const Launch& L, const ColRef& col, const uint32_t* perm, uint32_t n_rows, const FrameRows& rows, int64_t lo, int64_t hi,
                       int end, uint8_t* dst, uint8_t* dst_valid) {
    if (!n_rows) return;
    if (col.width == 4)
        RJ_KLAUNCH(L, "frame_pick", (k_frame_pick<4>), frame_grid(n_rows), 256, col, perm, n_rows, rows, lo, hi, (int32_t)end, dst, dst_valid);
    else
        RJ_KLAUNCH(L, "frame_pick", (k_frame_pick<8>), frame_grid(n_rows), 256, col, perm, n_rows, rows, lo, hi, (int32_t)end, dst, dst_valid);
}

void launch_frame_ntile(const Launch& L, uint32_t n_rows, const FrameRows& rows, int64_t buckets, unsigned long long* dst) {
    if (!n_rows) return;
    RJ_KLAUNCH(L, "frame_ntile", k_frame_ntile, frame_grid(n_rows), 256, n_rows, rows, buckets, dst);
}

void launch_frame_sum(const Launch& L, const uint32_t* nn, const unsigned long long* sum, uint32_t n_rows, const FrameRows& rows, int64_t lo,
                      int64_t hi, int what, unsigned long long* dst, uint8_t* dst_valid) {
    if (!n_rows) return;
    RJ_KLAUNCH(L, "frame_sum", k_frame_sum, frame_grid(n_rows), 256, nn, sum, n_rows, rows, lo, hi, (int32_t)what, dst, dst_valid);
}

void launch_frame_tree(const Launch& L, const ColRef& col, const uint32_t* perm, uint32_t n_rows, bool f64, bool is_max,
                       unsigned long long* tree) {
    if (!n_rows) return;
    std::vector<uint64_t> len{n_rows}, at{0};  // the levels' lengths and offsets
    while (len.back() > (uint64_t)FRAME_FANOUT) {
        at.push_back(at.back() + len.back());
        len.push_back((len.back() + FRAME_FANOUT - 1u) / FRAME_FANOUT);
    }
    auto level = [&](size_t k) { return k < len.size() ? tree + at[k] : nullptr; };
    const uint32_t grid = (uint32_t)(((uint64_t)n_rows + FRAME_THREADS - 1u) / FRAME_THREADS);
    if (col.width == 4)
        RJ_KLAUNCH(L, "frame_leaves", (k_frame_leaves<4>), grid, FRAME_THREADS, col, perm, n_rows, (int32_t)f64, (int32_t)is_max, tree, level(1),
                   level(2));
    else
        RJ_KLAUNCH(L, "frame_leaves", (k_frame_leaves<8>), grid, FRAME_THREADS, col, perm, n_rows, (int32_t)f64, (int32_t)is_max, tree, level(1),
                   level(2));
    for (size_t k = 2; k + 1 < len.size(); k += 2)
        RJ_KLAUNCH(L, "frame_levels", k_frame_levels, (uint32_t)((len[k] + FRAME_THREADS - 1u) / FRAME_THREADS), FRAME_THREADS,
                   (const unsigned long long*)level(k), len[k], (int32_t)is_max, level(k + 1), level(k + 2));
}

void launch_frame_extreme(const Launch& L, const unsigned long long* tree, const uint32_t* nn, uint32_t n_rows, const FrameRows& rows, int64_t lo,
                          int64_t hi, bool is_max, int decode, int width, uint8_t* dst, uint8_t* dst_valid) {
    if (!n_rows) return;
    RJ_KLAUNCH(L, "frame_extreme", k_frame_extreme, frame_grid(n_rows), 256, tree, nn, n_rows, rows, lo, hi, (int32_t)is_max, (int32_t)decode,
               (int32_t)width, dst, dst_valid);
}

}  // namespace rj
