// rj_group_util.hpp — the device helpers that the kernels of RJ_NODE_GROUP (rj_group.hip) and of
// RJ_NODE_WINDOW (rj_window.hip) share: the accumulators a wave moves between lanes, their segmented
// scan under a head mask, and a wave's share of a tile's head masks.  Device code: include from a .hip
// file only.
#pragma once
#include "rj_kernel_util.hpp"

namespace rj {

// what a wave moves between lanes: the counts of at most 16 * 64 positions fit 32 bits
template <int W>
struct GroupPart {
    uint32_t rows, nn;
    uint64_t sum, mn, mx;
};
template <int W>
__device__ __forceinline__ GroupPart<W> group_identity() {
    return GroupPart<W>{0u, 0u, 0ull, ~0ull, 0ull};
}
template <int W>
__device__ __forceinline__ void group_add(GroupPart<W>& a, const GroupPart<W>& b) {
    a.rows += b.rows;
    if constexpr (W != 0) {
        a.nn += b.nn;
        a.sum += b.sum;
        a.mn = min(a.mn, b.mn);
        a.mx = max(a.mx, b.mx);
    }
}
template <int W>
__device__ __forceinline__ GroupPart<W> group_shfl_up(const GroupPart<W>& a, int off) {
    GroupPart<W> t = a;
    t.rows = __shfl_up(a.rows, off);
    if constexpr (W != 0) {
        t.nn = __shfl_up(a.nn, off);
        t.sum = __shfl_up(a.sum, off);
        t.mn = __shfl_up(a.mn, off);
        t.mx = __shfl_up(a.mx, off);
    }
    return t;
}
template <int W>
__device__ __forceinline__ GroupPart<W> group_shfl_xor(const GroupPart<W>& a, int mask) {
    GroupPart<W> t = a;
    t.rows = __shfl_xor(a.rows, mask);
    if constexpr (W != 0) {
        t.nn = __shfl_xor(a.nn, mask);
        t.sum = __shfl_xor(a.sum, mask);
        t.mn = __shfl_xor(a.mn, mask);
        t.mx = __shfl_xor(a.mx, mask);
    }
    return t;
}
template <int W>
__device__ __forceinline__ GroupPart<W> group_shfl(const GroupPart<W>& a, int src) {
    GroupPart<W> t = a;
    t.rows = __shfl(a.rows, src);
    if constexpr (W != 0) {
        t.nn = __shfl(a.nn, src);
        t.sum = __shfl(a.sum, src);
        t.mn = __shfl(a.mn, src);
        t.mx = __shfl(a.mx, src);
    }
    return t;
}
// every lane: the wave's total
template <int W>
__device__ __forceinline__ GroupPart<W> group_wave_total(GroupPart<W> a) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) group_add(a, group_shfl_xor(a, m));
    return a;
}
// lane l: the total of lanes [s, l], s = the last head at or below l (lane 0 if there is none)
template <int W>
__device__ __forceinline__ GroupPart<W> group_segmented_scan(GroupPart<W> a, uint64_t heads, uint32_t lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const GroupPart<W> t = group_shfl_up(a, off);
        // no head in (lane - off, lane]: lane - off is in my segment
        const bool joins = lane >= (uint32_t)off && ((heads >> ((lane - (uint32_t)off + 1u) & 63u)) & ((1ull << off) - 1ull)) == 0;
        if (joins) group_add(a, t);
    }
    return a;
}

__device__ __forceinline__ uint64_t group_uniform(uint64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v);  // (the builtin returns int: no sign extension)
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return (uint64_t)lo | (uint64_t)hi << 32;
}

template <int W>
__device__ __forceinline__ uint64_t group_load(const ColRef& col, uint32_t r) {
    if constexpr (W == 4) return (uint64_t)col_load32(col, r);
    return col_load64(col, r);
}

// Lane j < GROUP_ITEMS of wave `wid`: `mask` = the head mask of the wave's item j in `tile`, `before` =
// the tile's heads in front of that item.
// One barrier; s_w (GROUP_WAVES words) is free again after the caller's next one.
__device__ __forceinline__ void group_wave_heads(const unsigned long long* __restrict__ masks, uint64_t n_masks, uint32_t tile,
                                                 uint32_t wid, uint32_t lane, uint32_t* s_w, uint64_t& mask, uint32_t& before) {
    const uint64_t idx = (uint64_t)tile * (GROUP_TILE / 64) + wid * GROUP_ITEMS + lane;
    mask = 0;
    if (lane < (uint32_t)GROUP_ITEMS && idx < n_masks) mask = masks[idx];
    const uint32_t c = (uint32_t)__popcll(mask);
    uint32_t       incl = c;
#pragma unroll
    for (int off = 1; off < GROUP_ITEMS; off <<= 1) {
        const uint32_t t = __shfl_up(incl, off);
        if (lane >= (uint32_t)off) incl += t;
    }
    if (lane == (uint32_t)GROUP_ITEMS - 1) s_w[wid] = incl;
    __syncthreads();
    uint32_t wbase = 0;
    for (uint32_t k = 0; k < wid; ++k) wbase += s_w[k];
    before = wbase + incl - c;
}

}  // namespace rj
