// rj_frame.hpp — the frame arithmetic of RJ_NODE_WINDOW's ROWS frames and NTILE, one function each for
// the kernels (k_frame_*, rj_frame.hip) and the host (rj_debug_win_frame / rj_debug_win_ntile, which the
// CPU tests pin them through).
#pragma once
#include <stdint.h>

namespace rj {

constexpr int64_t FRAME_CLAMP = 1ll << 32;  // a relation has fewer than 2^32 - 16 rows: an offset beyond it is "unbounded"

// a frame offset as the kernels take it: the sentinels and everything beyond +-2^32 become +-2^32
__host__ __device__ inline int64_t frame_clamp(int64_t off) {
    return off < -FRAME_CLAMP ? -FRAME_CLAMP : (off > FRAME_CLAMP ? FRAME_CLAMP : off);
}

// ROWS BETWEEN lo AND hi (signed offsets from the current row) of the row at position i, whose
// partition is the positions [ps, pe] (all three below 2^32): the frame is [a, b] with
// a = max(ps, i + lo) and b = min(pe, i + hi).  -> false, and a and b untouched, when it is empty.
__host__ __device__ inline bool frame_bounds(uint64_t i, uint64_t ps, uint64_t pe, int64_t lo, int64_t hi, uint64_t& a, uint64_t& b) {
    const int64_t first = (int64_t)i + frame_clamp(lo), last = (int64_t)i + frame_clamp(hi);  // |.| < 2^33
    const int64_t fa = first > (int64_t)ps ? first : (int64_t)ps, fb = last < (int64_t)pe ? last : (int64_t)pe;
    if (fa > fb) return false;
    a = (uint64_t)fa;
    b = (uint64_t)fb;
    return true;
}

// NTILE(n) of the row with r rows of its partition in front of it, the partition having N rows
// (r < N, n >= 1): PostgreSQL's rule.  With q = N / n and m = N % n the first m buckets hold q + 1
// rows, the rest q.  n > N gives q = 0 and m = N: every row is in front of m (q + 1) = N, so the
// division by q is never reached.
__host__ __device__ inline int64_t frame_ntile(uint64_t r, uint64_t N, int64_t n) {
    const uint64_t q = N / (uint64_t)n, m = N % (uint64_t)n, big = m * (q + 1);  // big <= N
    if (r < big || q == 0) return (int64_t)(r / (q + 1)) + 1;
    return (int64_t)(m + (r - big) / q) + 1;
}

}  // namespace rj
