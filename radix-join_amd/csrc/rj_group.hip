// rj_group.hip — the gfx950 (wave64) kernels of RJ_NODE_GROUP and their launchers.
#include <algorithm>

#include "rj_group_util.hpp"
#include "rj_kernel_util.hpp"
#include "rj_sortkey.hpp"

namespace rj {

// RJ_NODE_GROUP: the rows are ordered by the group keys (the sort's kernels, rj_sort.hip); what is
// left is to cut that order into runs of equal keys and to reduce every run (geometry: rj_device.hpp).
//   k_group_heads   one key column, read through the permutation: position i starts a group when its
//                   encoded value or NULL flag differs from position i - 1's -> one 64-bit head mask
//                   per item, OR-ed over the key columns; the last column's launch counts a tile's heads
//   k_group_scan    tile head counts -> every tile's first group index, and the group count
//   k_group_keys    every head stores its group's canonical key value (one writer per group)
//   k_group_init    the identities of the accumulators that atomics may touch (below)
//   k_group_reduce  one aggregated column (or none: COUNT(*)) gathered through the permutation and
//                   reduced run by run; its scalar variant reduces a whole relation into one group
//   k_group_column  an accumulator array -> a result column (decode, narrow, validity from the count)
// No rank or group index comes from an atomic: group(i) = heads in [0, i] - 1.
//
// k_group_reduce.  A lane adds the values of its positions into accumulators of its own while the
// items carry no head: those all belong to the wave's open group, so nothing crosses lanes (every
// group longer than a few items runs almost entirely here).  An item with heads
// first folds the lanes' accumulators (one butterfly), then scans the item segment by segment: the
// lane in front of a head holds a finished group.  A group that starts and ends inside one wave's
// quarter of the tile is stored by that lane.  What is left of a wave is its first segment (it
// continues a group from before) and its last (it is still open): the workgroup's four pairs meet in
// LDS, where thread 0 strings them together with the group it carries from tile to tile over its
// contiguous run of tiles.  A group that thread 0 closes inside the run is stored; only the FIRST
// group it closes and the one still open at the end of the run may be shared with a neighbour
// workgroup, and only those two are added to memory with atomics — whatever the group sizes, 2 per
// workgroup and accumulator.  k_group_init gave exactly those entries their identities in an earlier
// launch; every other entry is written exactly once, so nothing relies on what the memory held.

// One key column (W = bytes of a value).  first: this launch writes the masks, else it ORs into them;
// last: it also writes tile_heads[tile] = heads of the tile.  The neighbour of a position is the lane
// below, or the previous item's lane 63 (kept in a register); only a wave's first position reads it
// from memory.  A NULL's value bits count as 0.
template <int W>
__global__ __launch_bounds__(GROUP_THREADS) void k_group_heads(ColRef col, const uint32_t* __restrict__ perm, uint32_t n_rows, int32_t f64,
                                                               int32_t first, int32_t last, unsigned long long* __restrict__ masks,
                                                               uint32_t* __restrict__ tile_heads) {
    __shared__ uint32_t s_cnt[GROUP_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6, tile = blockIdx.x;
    const uint64_t wave_base = (uint64_t)tile * GROUP_TILE + (uint64_t)wid * (GROUP_TILE / GROUP_WAVES);
    auto           encoded = [&](uint64_t i, uint32_t& is_null) {
        const uint32_t r = perm ? perm[i] : (uint32_t)i;
        is_null = col.valid && !col.valid[r];
        return is_null ? 0ull : sort_key_bits(group_load<W>(col, r), W, f64 != 0, false);
    };
    uint64_t last_e = 0;
    uint32_t last_null = 0, cnt = 0;
    for (uint32_t j = 0; j < (uint32_t)GROUP_ITEMS; ++j) {
        const uint64_t i0 = wave_base + 64u * j, i = i0 + lane;
        if (i0 >= n_rows) break;  // (the whole wave, and every later item of it)
        const bool active = i < n_rows;
        uint64_t   e = 0;
        uint32_t   is_null = 0;
        if (active) e = encoded(i, is_null);
        uint64_t pe = __shfl_up(e, 1);
        uint32_t pn = __shfl_up(is_null, 1);
        if (lane == 0) {
            pe = last_e;
            pn = last_null;
            if (j == 0 && i > 0) pe = encoded(i - 1, pn);
        }
        const bool     head = active && (i == 0 || pe != e || pn != is_null);
        uint64_t       m = __ballot(head);
        const uint64_t idx = i0 / 64u;  // (< ceil(n_rows / 64): i0 < n_rows)
        if (!first) m |= masks[idx];
        if (lane == 0) masks[idx] = m;
        cnt += (uint32_t)__popcll(m);
        last_e = __shfl(e, 63);
        last_null = __shfl(is_null, 63);
    }
    if (last) {
        if (lane == 0) s_cnt[wid] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t t = 0;
            for (int w = 0; w < GROUP_WAVES; ++w) t += s_cnt[w];
            tile_heads[tile] = t;
        }
    }
}

// tile_base[t] = heads of the tiles before t, tile_base[n_tiles] = *total = all heads.  One workgroup.
__global__ __launch_bounds__(1024) void k_group_scan(const uint32_t* __restrict__ tile_heads, uint32_t n_tiles,
                                                     uint32_t* __restrict__ tile_base, uint32_t* __restrict__ total) {
    __shared__ uint32_t s_wsum[16];
    uint32_t            running = 0;
    for (uint32_t t0 = 0; t0 < n_tiles; t0 += 1024u) {  // (n_tiles <= 2^20)
        const uint32_t t = t0 + threadIdx.x;
        const uint32_t c = t < n_tiles ? tile_heads[t] : 0u;
        uint32_t       tot;
        lds_barrier();  // s_wsum is free again
        const uint32_t pre = block_excl_scan(c, s_wsum, tot);
        if (t < n_tiles) tile_base[t] = running + pre;
        running += tot;
    }
    if (threadIdx.x == 0) {
        tile_base[n_tiles] = running;
        *total = running;
    }
}

// Every head stores the canonical value of its group's key (the decoding of the encoded key: +0.0 for
// a zero, one NaN for every NaN; 0 and validity 0 for the NULL group) at its group index.
template <int W>
__global__ __launch_bounds__(GROUP_THREADS) void k_group_keys(ColRef col, const uint32_t* __restrict__ perm, uint32_t n_rows, int32_t f64,
                                                              const unsigned long long* __restrict__ masks,
                                                              const uint32_t* __restrict__ tile_base, uint32_t n_groups,
                                                              uint8_t* __restrict__ out, uint8_t* __restrict__ out_valid) {
    __shared__ uint32_t s_w[GROUP_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6, tile = blockIdx.x;
    const uint64_t n_masks = ((uint64_t)n_rows + 63u) / 64u;
    const uint64_t wave_base = (uint64_t)tile * GROUP_TILE + (uint64_t)wid * (GROUP_TILE / GROUP_WAVES);
    uint64_t       mask;
    uint32_t       before;
    group_wave_heads(masks, n_masks, tile, wid, lane, s_w, mask, before);
    before += tile_base[tile];
    for (uint32_t j = 0; j < (uint32_t)GROUP_ITEMS; ++j) {
        const uint64_t m = group_uniform(__shfl(mask, (int)j));
        const uint32_t b = __builtin_amdgcn_readfirstlane(__shfl(before, (int)j));
        if (!m) continue;
        const uint64_t i = wave_base + 64u * j + lane;
        const uint32_t gid = b + lane_prefix(m);
        if (((m >> lane) & 1ull) && i < n_rows && gid < n_groups) {
            const uint32_t r = perm ? perm[i] : (uint32_t)i;
            const bool     is_null = col.valid && !col.valid[r];
            uint64_t       v = 0;
            if (!is_null) v = sort_key_value(sort_key_bits(group_load<W>(col, r), W, f64 != 0, false), W, f64 != 0, false);
            if constexpr (W == 4)
                reinterpret_cast<uint32_t*>(out)[gid] = (uint32_t)v;
            else
                reinterpret_cast<uint64_t*>(out)[gid] = v;
            if (out_valid) out_valid[gid] = is_null ? 0 : 1;
        }
    }
}

// The run of tiles of workgroup b of k_group_reduce is [b * tiles_per_wg, (b + 1) * tiles_per_wg).
// Thread b: the identities of the two groups that run may share with its neighbours — the one its
// first position belongs to and the one that is open at its end.
__global__ __launch_bounds__(256) void k_group_init(GroupAcc acc, const unsigned long long* __restrict__ masks,
                                                    const uint32_t* __restrict__ tile_base, uint32_t n_tiles, uint32_t tiles_per_wg,
                                                    uint32_t n_runs, uint32_t n_groups) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= n_runs) return;
    const uint64_t t0 = (uint64_t)b * tiles_per_wg, t1 = t0 + tiles_per_wg;
    uint32_t       g[2] = {0u, n_groups - 1u};
    if (masks && t0 < n_tiles) g[0] = tile_base[t0] + (uint32_t)(masks[t0 * (GROUP_TILE / 64)] & 1ull) - 1u;
    if (masks && t1 < n_tiles) g[1] = tile_base[t1] - 1u;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (g[k] >= n_groups) continue;
        if (acc.rows) acc.rows[g[k]] = 0ull;
        if (acc.nn) acc.nn[g[k]] = 0ull;
        if (acc.sum) acc.sum[g[k]] = 0ull;
        if (acc.mn) acc.mn[g[k]] = ~0ull;
        if (acc.mx) acc.mx[g[k]] = 0ull;
    }
}

template <int W>
__device__ __forceinline__ void group_store(const GroupAcc& acc, uint32_t gid, uint32_t n_groups, uint64_t rows, uint64_t nn, uint64_t sum,
                                            uint64_t mn, uint64_t mx) {
    if (gid >= n_groups) return;
    if (acc.rows) acc.rows[gid] = rows;
    if constexpr (W != 0) {
        if (acc.nn) acc.nn[gid] = nn;
        if (acc.sum) acc.sum[gid] = sum;
        if (acc.mn) acc.mn[gid] = mn;
        if (acc.mx) acc.mx[gid] = mx;
    }
}
template <int W>
__device__ __forceinline__ void group_merge(const GroupAcc& acc, uint32_t gid, uint32_t n_groups, uint64_t rows, uint64_t nn, uint64_t sum,
                                            uint64_t mn, uint64_t mx) {
    if (gid >= n_groups) return;
    if (acc.rows) atomicAdd(&acc.rows[gid], (unsigned long long)rows);
    if constexpr (W != 0) {
        if (acc.nn) atomicAdd(&acc.nn[gid], (unsigned long long)nn);
        if (acc.sum) atomicAdd(&acc.sum[gid], (unsigned long long)sum);
        if (acc.mn) atomicMin(&acc.mn[gid], (unsigned long long)mn);
        if (acc.mx) atomicMax(&acc.mx[gid], (unsigned long long)mx);
    }
}

// W = bytes of a value of `col`, 0 = no column (COUNT(*) only).  Workgroup b walks its run of tiles
// (k_group_init).  KEYED = false is the scalar aggregate, ONE group of all rows: no masks, no tile_base,
// no permutation — nothing but the lanes' own accumulators until the run is over, then one fold per
// wave, one per workgroup and its atomics on group 0.  It is a variant of its own so that it keeps few
// registers and many loads in flight: it is a plain streaming read.
constexpr int GROUP_BATCH = 4;         // items whose loads are in flight together
constexpr int GROUP_SCALAR_BATCH = 8;  // ... in the scalar variant
static_assert(GROUP_ITEMS % GROUP_BATCH == 0 && GROUP_ITEMS % GROUP_SCALAR_BATCH == 0, "whole batches");

template <int W, bool KEYED>
__global__ __launch_bounds__(GROUP_THREADS) void k_group_reduce(ColRef col, const uint32_t* __restrict__ perm, uint32_t n_rows, int32_t f64,
                                                                const unsigned long long* __restrict__ masks,
                                                                const uint32_t* __restrict__ tile_base, uint32_t n_tiles,
                                                                uint32_t tiles_per_wg, uint32_t n_groups, GroupAcc acc) {
    __shared__ uint32_t s_w[GROUP_WAVES];
    __shared__ uint64_t s_first[GROUP_WAVES][5], s_open[GROUP_WAVES][5];  // rows, nn, sum, mn, mx
    __shared__ uint32_t s_has_head[GROUP_WAVES], s_gid_first[GROUP_WAVES], s_gid_open[GROUP_WAVES];
    using Part = GroupPart<W>;
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    const uint64_t n_masks = ((uint64_t)n_rows + 63u) / 64u;
    const uint64_t t_begin = (uint64_t)blockIdx.x * tiles_per_wg, t_end = min(t_begin + (uint64_t)tiles_per_wg, (uint64_t)n_tiles);
    // thread 0: the group that is open across waves and tiles
    uint64_t c_rows = 0, c_nn = 0, c_sum = 0, c_mn = ~0ull, c_mx = 0;
    uint32_t c_gid = 0;
    bool     c_shared = true;  // the next group to close may have begun in the previous workgroup's run
    if constexpr (!KEYED) {
        uint64_t rows = 0, nn = 0, sum = 0, mn = ~0ull, mx = 0;  // (a lane's share of a run of any length)
        for (uint64_t tile = t_begin; tile < t_end; ++tile) {
            const uint64_t wave_base = tile * GROUP_TILE + (uint64_t)wid * (GROUP_TILE / GROUP_WAVES);
            for (uint32_t j0 = 0; j0 < (uint32_t)GROUP_ITEMS; j0 += GROUP_SCALAR_BATCH) {
                if (wave_base + 64u * j0 >= n_rows) break;  // (the whole wave, and every later item of it)
                uint64_t bits[GROUP_SCALAR_BATCH];
                uint32_t state[GROUP_SCALAR_BATCH];  // bit 0: a row, bit 1: a value
#pragma unroll
                for (int k = 0; k < GROUP_SCALAR_BATCH; ++k) {
                    const uint64_t i = wave_base + 64u * (j0 + k) + lane;
                    bits[k] = 0;
                    state[k] = i < n_rows ? 1u : 0u;
                    if constexpr (W != 0) {
                        if (i < n_rows && !(col.valid && !col.valid[i])) {
                            bits[k] = group_load<W>(col, (uint32_t)i);
                            state[k] = 3u;
                        }
                    }
                }
#pragma unroll
                for (int k = 0; k < GROUP_SCALAR_BATCH; ++k) {
                    rows += state[k] & 1u;
                    if constexpr (W != 0) {
                        if (state[k] & 2u) {
                            const uint64_t e = sort_key_bits(bits[k], W, f64 != 0, false);
                            nn += 1;
                            sum += W == 4 ? (uint64_t)(int64_t)(int32_t)(uint32_t)bits[k] : bits[k];
                            mn = min(mn, e);
                            mx = max(mx, e);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            rows += __shfl_xor(rows, m);
            if constexpr (W != 0) {
                nn += __shfl_xor(nn, m);
                sum += __shfl_xor(sum, m);
                mn = min(mn, __shfl_xor(mn, m));
                mx = max(mx, __shfl_xor(mx, m));
            }
        }
        if (lane == 0) s_open[wid][0] = rows, s_open[wid][1] = nn, s_open[wid][2] = sum, s_open[wid][3] = mn, s_open[wid][4] = mx;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 0; w < GROUP_WAVES; ++w) {
                c_rows += s_open[w][0], c_nn += s_open[w][1], c_sum += s_open[w][2];
                c_mn = min(c_mn, s_open[w][3]), c_mx = max(c_mx, s_open[w][4]);
            }
            if (c_rows) group_merge<W>(acc, 0u, n_groups, c_rows, c_nn, c_sum, c_mn, c_mx);
        }
        return;
    }
    for (uint64_t tile = t_begin; tile < t_end; ++tile) {
        const uint64_t wave_base = tile * GROUP_TILE + (uint64_t)wid * (GROUP_TILE / GROUP_WAVES);
        uint64_t       mask;
        uint32_t       before;
        group_wave_heads(masks, n_masks, (uint32_t)tile, wid, lane, s_w, mask, before);
        before += tile_base[tile];
        uint32_t g_before = __builtin_amdgcn_readfirstlane(before);  // heads in front of the wave's next item (lane 0's: item 0)
        const uint32_t gid_first = g_before - 1u;                    // the group the wave's first segment belongs to
        Part     mine = group_identity<W>(), first_seg = group_identity<W>();
        bool     seen_head = false;
        for (uint32_t j0 = 0; j0 < (uint32_t)GROUP_ITEMS; j0 += GROUP_BATCH) {
            if (wave_base + 64u * j0 >= n_rows) break;  // (the whole wave, and every later item of it)
            Part x[GROUP_BATCH];
#pragma unroll
            for (int k = 0; k < GROUP_BATCH; ++k) {
                const uint64_t i = wave_base + 64u * (j0 + k) + lane;
                x[k] = group_identity<W>();
                if (i < n_rows) {
                    x[k].rows = 1;
                    if constexpr (W != 0) {
                        const uint32_t r = perm ? perm[i] : (uint32_t)i;
                        if (!(col.valid && !col.valid[r])) {
                            const uint64_t bits = group_load<W>(col, r);
                            x[k].nn = 1;
                            x[k].sum = W == 4 ? (uint64_t)(int64_t)(int32_t)(uint32_t)bits : bits;
                            x[k].mn = x[k].mx = sort_key_bits(bits, W, f64 != 0, false);
                        }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < GROUP_BATCH; ++k) {
                const uint64_t m = group_uniform(__shfl(mask, (int)(j0 + k)));
                if (!m) {  // the open group goes on: every lane for itself
                    group_add(mine, x[k]);
                    continue;
                }
                const Part     open = group_wave_total(mine);
                Part           s = group_segmented_scan(x[k], m, lane);
                const uint32_t heads_le = (uint32_t)__popcll(m & ((2ull << lane) - 1ull));  // heads in [0, lane]
                if (heads_le == 0) group_add(s, open);
                // the open group ends in front of the item's first head
                const uint32_t fh = (uint32_t)__builtin_ctzll(m);
                Part           closed = group_shfl(s, (int)((fh - 1u) & 63u));
                if (fh == 0) closed = open;
                if (!seen_head) {
                    first_seg = closed;
                    seen_head = true;
                } else if (lane == 0) {  // it began at a head of this wave: nobody else knows it
                    group_store<W>(acc, g_before - 1u, n_groups, closed.rows, closed.nn, closed.sum, closed.mn, closed.mx);
                }
                // groups that begin and end inside the item: the lane in front of the next head has the total
                if (heads_le != 0 && lane < 63u && ((m >> (lane + 1u)) & 1ull))
                    group_store<W>(acc, g_before + heads_le - 1u, n_groups, s.rows, s.nn, s.sum, s.mn, s.mx);
                const uint32_t lh = 63u - (uint32_t)__builtin_clzll(m);
                mine = lane >= lh ? x[k] : group_identity<W>();
                g_before += (uint32_t)__popcll(m);
            }
        }
        const Part rest = group_wave_total(mine);
        if (lane == 0) {
            const Part& f = seen_head ? first_seg : rest;
            s_first[wid][0] = f.rows, s_first[wid][1] = f.nn, s_first[wid][2] = f.sum, s_first[wid][3] = f.mn, s_first[wid][4] = f.mx;
            s_open[wid][0] = rest.rows, s_open[wid][1] = rest.nn, s_open[wid][2] = rest.sum, s_open[wid][3] = rest.mn, s_open[wid][4] = rest.mx;
            s_has_head[wid] = seen_head ? 1u : 0u;
            s_gid_first[wid] = gid_first;
            s_gid_open[wid] = g_before - 1u;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 0; w < GROUP_WAVES; ++w) {
                c_rows += s_first[w][0], c_nn += s_first[w][1], c_sum += s_first[w][2];
                c_mn = min(c_mn, s_first[w][3]), c_mx = max(c_mx, s_first[w][4]);
                c_gid = s_gid_first[w];
                if (!s_has_head[w]) continue;
                if (c_rows) {  // (nothing in front of a run's first head: nothing to close)
                    if (c_shared)
                        group_merge<W>(acc, c_gid, n_groups, c_rows, c_nn, c_sum, c_mn, c_mx);
                    else
                        group_store<W>(acc, c_gid, n_groups, c_rows, c_nn, c_sum, c_mn, c_mx);
                }
                c_shared = false;
                c_rows = s_open[w][0], c_nn = s_open[w][1], c_sum = s_open[w][2], c_mn = s_open[w][3], c_mx = s_open[w][4];
                c_gid = s_gid_open[w];
            }
        }
        // (the next tile writes s_w before its first barrier and the arrays above behind it: thread 0 is
        // through with them by then)
    }
    if (threadIdx.x == 0 && c_rows) group_merge<W>(acc, c_gid, n_groups, c_rows, c_nn, c_sum, c_mn, c_mx);
}

// An accumulator array as a result column: decoded (GroupDecode), narrowed to `width` bytes, 0 where
// the group has no non-NULL value; validity bytes nn[i] != 0 (dst_valid optional; nn == nullptr: all valid).
__global__ __launch_bounds__(256) void k_group_column(const unsigned long long* __restrict__ src, const unsigned long long* __restrict__ nn,
                                                      uint64_t n, int32_t decode, int32_t width, uint8_t* __restrict__ dst,
                                                      uint8_t* __restrict__ dst_valid) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const bool valid = nn ? nn[i] != 0 : true;
    uint64_t   v = src[i];
    if (decode != GROUP_RAW) v = sort_key_value(v, decode == GROUP_KEY32 ? 4 : 8, decode == GROUP_KEYF64, false);
    if (!valid) v = 0;
    if (width == 4)
        reinterpret_cast<uint32_t*>(dst)[i] = (uint32_t)v;
    else
        reinterpret_cast<uint64_t*>(dst)[i] = v;
    if (dst_valid) dst_valid[i] = valid ? 1 : 0;
}

// ================================================================== launchers
static uint32_t group_tiles(uint32_t n_rows) { return n_rows / GROUP_TILE + (n_rows % GROUP_TILE != 0); }

void launch_group_heads(const Launch& L, const ColRef& col, const uint32_t* perm, uint32_t n_rows, bool f64, bool first, bool last,
                        unsigned long long* masks, uint32_t* tile_heads) {
    if (!n_rows) return;
    if (col.width == 4)
        RJ_KLAUNCH(L, "group_heads", (k_group_heads<4>), group_tiles(n_rows), GROUP_THREADS, col, perm, n_rows, (int32_t)f64,
                   (int32_t)first, (int32_t)last, masks, tile_heads);
    else
        RJ_KLAUNCH(L, "group_heads", (k_group_heads<8>), group_tiles(n_rows), GROUP_THREADS, col, perm, n_rows, (int32_t)f64,
                   (int32_t)first, (int32_t)last, masks, tile_heads);
}

void launch_group_scan(const Launch& L, const uint32_t* tile_heads, uint32_t n_rows, uint32_t* tile_base, uint32_t* total) {
    if (!n_rows) return;
    RJ_KLAUNCH(L, "group_scan", k_group_scan, 1, 1024, tile_heads, group_tiles(n_rows), tile_base, total);
}

void launch_group_keys(const Launch& L, const ColRef& col, const uint32_t* perm, uint32_t n_rows, bool f64,
                       const unsigned long long* masks, const uint32_t* tile_base, uint32_t n_groups, uint8_t* out, uint8_t* out_valid) {
    if (!n_rows || !n_groups) return;
    if (col.width == 4)
        RJ_KLAUNCH(L, "group_keys", (k_group_keys<4>), group_tiles(n_rows), GROUP_THREADS, col, perm, n_rows, (int32_t)f64, masks,
                   tile_base, n_groups, out, out_valid);
    else
        RJ_KLAUNCH(L, "group_keys", (k_group_keys<8>), group_tiles(n_rows), GROUP_THREADS, col, perm, n_rows, (int32_t)f64, masks,
                   tile_base, n_groups, out, out_valid);
}

void launch_group_reduce(const Launch& L, const ColRef* col, const uint32_t* perm, uint32_t n_rows, bool f64,
                         const unsigned long long* masks, const uint32_t* tile_base, uint32_t n_groups, const GroupAcc& acc,
                         uint32_t max_grid) {
    if (!n_groups) return;
    const uint32_t n_tiles = group_tiles(n_rows);
    const uint32_t grid0 = std::max(1u, std::min(n_tiles, std::max(1u, max_grid)));
    const uint32_t tiles_per_wg = std::max(1u, n_tiles / grid0 + (n_tiles % grid0 != 0));
    const uint32_t n_runs = std::max(1u, n_tiles / tiles_per_wg + (n_tiles % tiles_per_wg != 0));
    // an empty scalar aggregate has one group and no tile: the identities are its result
    RJ_KLAUNCH(L, "group_init", k_group_init, n_runs / 256u + (n_runs % 256u != 0), 256, acc, masks, tile_base, n_tiles, tiles_per_wg,
               n_runs, n_groups);
    if (!n_tiles) return;
    const ColRef none{nullptr, nullptr, COL_NONE, 0};
    const ColRef ref = col ? *col : none;
    const int    width = col ? col->width : 0;
    const bool   keyed = masks != nullptr;
    if (keyed != (tile_base != nullptr) || (!keyed && (perm || n_groups != 1)))
        launch_failed("group_reduce", "a scalar aggregate has neither masks nor a permutation and one group", false);
    auto go = [&](auto kernel) {
        RJ_KLAUNCH(L, "group_reduce", kernel, n_runs, GROUP_THREADS, ref, perm, n_rows, (int32_t)f64, masks, tile_base, n_tiles, tiles_per_wg,
                   n_groups, acc);
    };
    if (width == 0)
        keyed ? go(k_group_reduce<0, true>) : go(k_group_reduce<0, false>);
    else if (width == 4)
        keyed ? go(k_group_reduce<4, true>) : go(k_group_reduce<4, false>);
    else
        keyed ? go(k_group_reduce<8, true>) : go(k_group_reduce<8, false>);
}

void launch_group_column(const Launch& L, const unsigned long long* src, const unsigned long long* nn, uint64_t n, int decode, int width,
                         uint8_t* dst, uint8_t* dst_valid) {
    if (!n) return;
    const uint32_t grid = (uint32_t)((n + 255) / 256);
    RJ_KLAUNCH(L, "group_column", k_group_column, grid, 256, src, nn, n, (int32_t)decode, (int32_t)width, dst, dst_valid);
}

}  // namespace rj
