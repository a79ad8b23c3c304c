// rj_setop.hip — the gfx950 (wave64) kernels of RJ_NODE_SETOP and their launchers.
#include <algorithm>

#include "rj_group_util.hpp"
#include "rj_kernel_util.hpp"
#include "rj_tuple_util.hpp"

namespace rj {

// RJ_NODE_SETOP: the two children's rows sit in one relation (k_setop_concat; row id < n_left: a left
// row), ordered by every column (the sort's kernels, rj_sort.hip) and cut into runs of equal rows (the
// grouping's k_group_heads / k_group_scan, rj_group.hip).  What is left (geometry: rj_device.hpp):
//   k_setop_concat   one column of both children, one behind the other, into a dense array or — a root
//                    column without NULLs — straight into Page images
//   k_setop_left     a tile's left rows, found through the permutation
//   k_setop_scan     tile counts -> every tile's prefix, and the total (one workgroup)
//   k_setop_runs     every head stores where its run starts and how many left rows lie in front of it
//                    (one writer per run); a run's rows and left rows are differences of neighbours
//   k_setop_mult     a tile of runs -> the sum of their multiplicities
//   k_setop_offsets  the exclusive scan of the multiplicities: where a run's copies start in the output
//   k_setop_emit     output row j -> the run it is a copy of (the last run whose offset is <= j)
// Reduce, scan, apply, each a launch of its own: no workgroup waits for another, nothing comes from an
// atomic, and every entry of every array is written exactly once, whatever the memory held.
//
// A run may span any number of tiles and workgroups: nothing is reduced run by run.  The left rows
// in front of a position are a plain prefix count over the positions (k_setop_left, k_setop_scan, then
// inside the tile by ballots), so a run of any length costs what its head costs.

__device__ __forceinline__ uint32_t setop_mult(int32_t op, uint32_t rows, uint32_t l) {
    const uint32_t r = rows - l;
    switch (op) {
    case SETOP_UNION: return 1u;
    case SETOP_INTERSECT: return (l && r) ? 1u : 0u;
    case SETOP_INTERSECT_ALL: return min(l, r);
    case SETOP_EXCEPT: return (l && !r) ? 1u : 0u;
    case SETOP_EXCEPT_ALL: return l > r ? l - r : 0u;
    default: return rows;  // SETOP_UNION_ALL
    }
}

// Row i of the output = row i of `l` for i < n_left, else row i - n_left of `r`; validity bytes where
// dst_valid is given (1 for a side without any).  A side without rows is never read.  A thread takes
// SETOP_RUN = 16 / W consecutive output rows: where they come from one side and lie in one page on both
// ends (always, for dense arrays), they move as one 16-byte vector; else row by row.
template <int W>
__device__ __forceinline__ void setop_copy(const ColRef& c, uint32_t row, uint64_t i, const OutStream& dst, uint8_t* __restrict__ dst_valid) {
    if constexpr (W == 4) {
        stream_store(dst, i, col_load32(c, row), 0u);
    } else {
        const uint64_t v = col_load64(c, row);
        stream_store(dst, i, (uint32_t)v, (uint32_t)(v >> 32));
    }
    if (dst_valid) dst_valid[i] = c.valid ? c.valid[row] : (uint8_t)1;
}
// where 16 / W values from `row` on lie one behind the other, or nullptr
template <int W>
__device__ __forceinline__ const uint8_t* setop_src_run(const ColRef& c, uint32_t row) {
    constexpr uint32_t V = 16 / W, ROWS = W == 4 ? ROWS32 : ROWS64, HDR = W == 4 ? HDR32 : HDR64;
    if (c.kind == COL_DENSE) return c.ptr + (size_t)row * W;
    if (c.kind != COL_PAGED) return nullptr;  // (COL_IOTA: nothing to load)
    const uint32_t p = row / ROWS, i = row - p * ROWS;
    return i + V <= ROWS ? c.ptr + (size_t)p * PAGE_BYTES + HDR + i * W : nullptr;
}
template <int W>
__device__ __forceinline__ uint8_t* setop_dst_run(const OutStream& o, uint64_t row) {
    constexpr uint32_t V = 16 / W, ROWS = W == 4 ? ROWS32 : ROWS64, HDR = W == 4 ? HDR32 : HDR64;
    if (o.mode == (W == 4 ? ST_DENSE32 : ST_DENSE64)) return o.base + row * W;
    if (o.mode != (W == 4 ? ST_PAGED32 : ST_PAGED64)) return nullptr;
    const uint32_t r = (uint32_t)row, p = r / ROWS, i = r - p * ROWS;
    return i + V <= ROWS ? o.base + (size_t)p * PAGE_BYTES + HDR + i * W : nullptr;
}
// 16 / W rows of one side as a vector; false: not one run on both ends (nothing was written)
template <int W>
__device__ __forceinline__ bool setop_copy_run(const ColRef& c, uint32_t row, uint64_t i, const OutStream& dst, uint8_t* __restrict__ dst_valid) {
    constexpr int  V = 16 / W;
    const uint8_t* src = setop_src_run<W>(c, row);
    uint8_t*       out = setop_dst_run<W>(dst, i);
    if (!src || !out) return false;
    *reinterpret_cast<u32x4a*>(out) = *reinterpret_cast<const u32x4a*>(src);  // (values are 4-byte aligned at least)
    if (dst_valid) {
#pragma unroll
        for (int k = 0; k < V; ++k) dst_valid[i + k] = c.valid ? c.valid[row + k] : (uint8_t)1;
    }
    return true;
}
template <int W>
__global__ __launch_bounds__(256) void k_setop_concat(ColRef l, ColRef r, uint32_t n_left, uint64_t n, OutStream dst,
                                                      uint8_t* __restrict__ dst_valid) {
    constexpr uint32_t V = 16 / W;
    const uint64_t     i0 = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * V;
    if (i0 >= n) return;
    if (i0 + V <= n) {
        if (i0 + V <= n_left) {
            if (setop_copy_run<W>(l, (uint32_t)i0, i0, dst, dst_valid)) return;
        } else if (i0 >= n_left) {
            if (setop_copy_run<W>(r, (uint32_t)(i0 - n_left), i0, dst, dst_valid)) return;
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < V; ++k) {
        const uint64_t i = i0 + k;
        if (i >= n) break;
        if (i < n_left)
            setop_copy<W>(l, (uint32_t)i, i, dst, dst_valid);
        else
            setop_copy<W>(r, (uint32_t)(i - n_left), i, dst, dst_valid);
    }
}

// tile_left[t] = positions of tile t whose row is a left row.  Workgroup b walks the tiles
// [b * tiles_per_wg, (b + 1) * tiles_per_wg).
__global__ __launch_bounds__(SETOP_THREADS) void k_setop_left(const uint32_t* __restrict__ perm, uint32_t n_rows, uint32_t n_left,
                                                              uint32_t n_tiles, uint32_t tiles_per_wg, uint32_t* __restrict__ tile_left) {
    __shared__ uint32_t s_w[GROUP_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    const uint64_t t_begin = (uint64_t)blockIdx.x * tiles_per_wg, t_end = min(t_begin + (uint64_t)tiles_per_wg, (uint64_t)n_tiles);
    for (uint64_t tile = t_begin; tile < t_end; ++tile) {
        uint32_t c = 0;
#pragma unroll
        for (int k = 0; k < GROUP_ITEMS; ++k) {
            const uint64_t i = tile * GROUP_TILE + (uint64_t)k * SETOP_THREADS + threadIdx.x;
            if (i < n_rows) c += (perm ? perm[i] : (uint32_t)i) < n_left ? 1u : 0u;
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) c += __shfl_xor(c, m);
        if (lane == 0) s_w[wid] = c;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t t = 0;
            for (int w = 0; w < GROUP_WAVES; ++w) t += s_w[w];
            tile_left[tile] = t;
        }
        __syncthreads();  // s_w is free again
    }
}

// base[t] = sum of in[0 .. t), base[n] = *total = the sum of all.  One workgroup.
__global__ __launch_bounds__(1024) void k_setop_scan(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ base,
                                                     uint32_t* __restrict__ total) {
    __shared__ uint32_t s_wsum[16];
    uint32_t            running = 0;
    for (uint32_t t0 = 0; t0 < n; t0 += 1024u) {  // (n <= 2^20)
        const uint32_t t = t0 + threadIdx.x;
        const uint32_t c = t < n ? in[t] : 0u;
        uint32_t       tot;
        lds_barrier();  // s_wsum is free again
        const uint32_t pre = block_excl_scan(c, s_wsum, tot);
        if (t < n) base[t] = running + pre;
        running += tot;
    }
    if (threadIdx.x == 0) {
        base[n] = running;
        if (total) *total = running;
    }
}

// The head of run g stores runs.start[g] = its position and runs.left[g] = the left rows in front of it;
// entry n_runs is (n_rows, n_left).  masks / tile_base: the grouping's; tile_lbase: the scan of
// k_setop_left's counts.  Positions in the grouping's (wave, item, lane) order.
__global__ __launch_bounds__(SETOP_THREADS) void k_setop_runs(const uint32_t* __restrict__ perm, uint32_t n_rows, uint32_t n_left,
                                                              const unsigned long long* __restrict__ masks,
                                                              const uint32_t* __restrict__ tile_base,
                                                              const uint32_t* __restrict__ tile_lbase, uint32_t n_tiles,
                                                              uint32_t tiles_per_wg, uint32_t n_runs, SetopRuns runs) {
    __shared__ uint32_t s_w[GROUP_WAVES], s_l[GROUP_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    const uint64_t n_masks = ((uint64_t)n_rows + 63u) / 64u;
    const uint64_t t_begin = (uint64_t)blockIdx.x * tiles_per_wg, t_end = min(t_begin + (uint64_t)tiles_per_wg, (uint64_t)n_tiles);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        runs.start[n_runs] = n_rows;
        runs.left[n_runs] = n_left;
    }
    for (uint64_t tile = t_begin; tile < t_end; ++tile) {
        const uint64_t wave_base = tile * GROUP_TILE + (uint64_t)wid * (GROUP_TILE / GROUP_WAVES);
        uint64_t       mask;
        uint32_t       before;
        group_wave_heads(masks, n_masks, (uint32_t)tile, wid, lane, s_w, mask, before);
        before += tile_base[tile];
        // lane j: the left rows of the wave's item j as a mask
        uint64_t lmask = 0;
#pragma unroll
        for (int j = 0; j < GROUP_ITEMS; ++j) {
            const uint64_t i = wave_base + 64u * (uint32_t)j + lane;
            const bool     is_left = i < n_rows && (perm ? perm[i] : (uint32_t)i) < n_left;
            const uint64_t b = __ballot(is_left);
            if (lane == (uint32_t)j) lmask = b;
        }
        // ... and the wave's left rows in front of it
        const uint32_t lc = (uint32_t)__popcll(lmask);
        uint32_t       lincl = lc;
#pragma unroll
        for (int off = 1; off < GROUP_ITEMS; off <<= 1) {
            const uint32_t t = __shfl_up(lincl, off);
            if (lane >= (uint32_t)off) lincl += t;
        }
        if (lane == (uint32_t)GROUP_ITEMS - 1) s_l[wid] = lincl;
        __syncthreads();
        uint32_t lbase = tile_lbase[tile];
        for (uint32_t k = 0; k < wid; ++k) lbase += s_l[k];
        const uint32_t lbefore = lbase + lincl - lc;
        for (uint32_t j = 0; j < (uint32_t)GROUP_ITEMS; ++j) {
            const uint64_t m = group_uniform(__shfl(mask, (int)j));
            const uint64_t lm = group_uniform(__shfl(lmask, (int)j));
            const uint32_t b = __builtin_amdgcn_readfirstlane(__shfl(before, (int)j));
            const uint32_t lb = __builtin_amdgcn_readfirstlane(__shfl(lbefore, (int)j));
            if (!m) continue;
            const uint64_t i = wave_base + 64u * j + lane;
            const uint32_t gid = b + lane_prefix(m);
            if (((m >> lane) & 1ull) && i < n_rows && gid < n_runs) {
                runs.start[gid] = (uint32_t)i;
                runs.left[gid] = lb + lane_prefix(lm);
            }
        }
        // (the next tile writes s_w before its first barrier: every wave has read it in front of the
        // barrier above; it writes s_l behind that barrier: every wave has read s_l by then)
    }
}

// tile_m[t] = the multiplicities of the runs [t * SETOP_TILE, (t + 1) * SETOP_TILE), summed.
__global__ __launch_bounds__(SETOP_THREADS) void k_setop_mult(SetopRuns runs, uint32_t n_runs, int32_t op, uint32_t n_tiles,
                                                              uint32_t tiles_per_wg, uint32_t* __restrict__ tile_m) {
    __shared__ uint32_t s_w[GROUP_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    const uint64_t t_begin = (uint64_t)blockIdx.x * tiles_per_wg, t_end = min(t_begin + (uint64_t)tiles_per_wg, (uint64_t)n_tiles);
    for (uint64_t tile = t_begin; tile < t_end; ++tile) {
        uint32_t c = 0;
#pragma unroll
        for (int k = 0; k < SETOP_ITEMS; ++k) {
            const uint64_t g = tile * SETOP_TILE + (uint64_t)k * SETOP_THREADS + threadIdx.x;
            if (g < n_runs) c += setop_mult(op, runs.start[g + 1] - runs.start[g], runs.left[g + 1] - runs.left[g]);
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) c += __shfl_xor(c, m);
        if (lane == 0) s_w[wid] = c;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t t = 0;
            for (int w = 0; w < GROUP_WAVES; ++w) t += s_w[w];
            tile_m[tile] = t;
        }
        __syncthreads();  // s_w is free again
    }
}

// off[g] = the multiplicities of the runs in front of g, off[n_runs] = all of them (tile_mbase: the scan
// of k_setop_mult's sums).
__global__ __launch_bounds__(SETOP_THREADS) void k_setop_offsets(SetopRuns runs, uint32_t n_runs, int32_t op,
                                                                 const uint32_t* __restrict__ tile_mbase, uint32_t n_tiles,
                                                                 uint32_t tiles_per_wg, uint32_t* __restrict__ off) {
    __shared__ uint32_t s_wsum[GROUP_WAVES];
    const uint64_t t_begin = (uint64_t)blockIdx.x * tiles_per_wg, t_end = min(t_begin + (uint64_t)tiles_per_wg, (uint64_t)n_tiles);
    for (uint64_t tile = t_begin; tile < t_end; ++tile) {
        uint32_t running = tile_mbase[tile];
        for (int k = 0; k < SETOP_ITEMS; ++k) {
            const uint64_t g = tile * SETOP_TILE + (uint64_t)k * SETOP_THREADS + threadIdx.x;
            uint32_t       m = 0;
            if (g < n_runs) m = setop_mult(op, runs.start[g + 1] - runs.start[g], runs.left[g + 1] - runs.left[g]);
            uint32_t       tot;
            const uint32_t pre = block_excl_scan(m, s_wsum, tot);
            if (g < n_runs) off[g] = running + pre;
            if (g + 1 == n_runs) off[n_runs] = running + pre + m;
            running += tot;
            lds_barrier();  // s_wsum is free again
        }
    }
}

// the last g of [lo, hi] with off[g] <= j (off[lo] <= j)
__device__ __forceinline__ uint32_t setop_find(const uint32_t* __restrict__ off, uint32_t lo, uint32_t hi, uint32_t j) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1u) / 2u;
        if (off[mid] <= j)
            lo = mid;
        else
            hi = mid - 1u;
    }
    return lo;
}

// run_of[j] = the run that output row j is a copy of: the last run whose offset is <= j (the runs behind
// it that share its offset have no copies).  A tile first brackets the runs of its first and its last
// row; every row is then searched for between those two.
__global__ __launch_bounds__(SETOP_THREADS) void k_setop_emit(const uint32_t* __restrict__ off, uint32_t n_runs, uint32_t n_out,
                                                              uint32_t n_tiles, uint32_t tiles_per_wg, uint32_t* __restrict__ run_of) {
    __shared__ uint32_t s_bracket[2];
    const uint64_t t_begin = (uint64_t)blockIdx.x * tiles_per_wg, t_end = min(t_begin + (uint64_t)tiles_per_wg, (uint64_t)n_tiles);
    for (uint64_t tile = t_begin; tile < t_end; ++tile) {
        const uint64_t j0 = tile * SETOP_EMIT_TILE, j1 = min(j0 + (uint64_t)SETOP_EMIT_TILE, (uint64_t)n_out);
        if (threadIdx.x == 0) s_bracket[0] = setop_find(off, 0u, n_runs - 1u, (uint32_t)j0);
        if (threadIdx.x == 64) s_bracket[1] = setop_find(off, 0u, n_runs - 1u, (uint32_t)(j1 - 1u));
        __syncthreads();
        const uint32_t lo = s_bracket[0], hi = s_bracket[1];
#pragma unroll
        for (int k = 0; k < SETOP_EMIT_ITEMS; ++k) {
            const uint64_t j = j0 + (uint64_t)k * SETOP_THREADS + threadIdx.x;
            if (j < j1) run_of[j] = setop_find(off, lo, hi, (uint32_t)j);
        }
        __syncthreads();  // s_bracket is free again
    }
}

// ================================================================== launchers
namespace {
struct SetopGrid {
    uint32_t n_tiles, tiles_per_wg, grid;
};
// `n` entries in tiles of `tile`, on at most max_grid workgroups, each of which walks a run of tiles
SetopGrid setop_grid(uint64_t n, uint32_t tile, uint32_t max_grid) {
    SetopGrid g;
    g.n_tiles = (uint32_t)((n + tile - 1) / tile);
    const uint32_t grid0 = std::max(1u, std::min(g.n_tiles, std::max(1u, max_grid)));
    g.tiles_per_wg = std::max(1u, g.n_tiles / grid0 + (g.n_tiles % grid0 != 0));
    g.grid = std::max(1u, g.n_tiles / g.tiles_per_wg + (g.n_tiles % g.tiles_per_wg != 0));
    return g;
}
}  // namespace

void launch_setop_concat(const Launch& L, const ColRef& l, const ColRef& r, uint32_t n_left, uint64_t n, const OutStream& dst,
                         uint8_t* dst_valid) {
    if (!n) return;
    const ColRef&  any = n_left ? l : r;
    const uint64_t per_wg = 256u * (16u / (uint32_t)any.width);  // (a thread takes 16 bytes of values)
    const uint32_t grid = (uint32_t)((n + per_wg - 1) / per_wg);
    if (any.width == 4)
        RJ_KLAUNCH(L, "setop_concat", (k_setop_concat<4>), grid, 256, l, r, n_left, n, dst, dst_valid);
    else
        RJ_KLAUNCH(L, "setop_concat", (k_setop_concat<8>), grid, 256, l, r, n_left, n, dst, dst_valid);
}

void launch_setop_runs(const Launch& L, const uint32_t* perm, uint32_t n_rows, uint32_t n_left, const unsigned long long* masks,
                       const uint32_t* tile_base, uint32_t n_runs, uint32_t* tile_left, uint32_t* tile_lbase, const SetopRuns& runs,
                       uint32_t max_grid) {
    if (!n_rows || !n_runs) return;
    const SetopGrid g = setop_grid(n_rows, GROUP_TILE, max_grid);
    RJ_KLAUNCH(L, "setop_left", k_setop_left, g.grid, SETOP_THREADS, perm, n_rows, n_left, g.n_tiles, g.tiles_per_wg, tile_left);
    RJ_KLAUNCH(L, "setop_scan", k_setop_scan, 1, 1024, tile_left, g.n_tiles, tile_lbase, (uint32_t*)nullptr);
    RJ_KLAUNCH(L, "setop_runs", k_setop_runs, g.grid, SETOP_THREADS, perm, n_rows, n_left, masks, tile_base, tile_lbase, g.n_tiles,
               g.tiles_per_wg, n_runs, runs);
}

void launch_setop_offsets(const Launch& L, const SetopRuns& runs, uint32_t n_runs, int op, uint32_t* tile_m, uint32_t* tile_mbase,
                          uint32_t* off, uint32_t* total, uint32_t max_grid) {
    if (!n_runs) return;
    const SetopGrid g = setop_grid(n_runs, SETOP_TILE, max_grid);
    RJ_KLAUNCH(L, "setop_mult", k_setop_mult, g.grid, SETOP_THREADS, runs, n_runs, (int32_t)op, g.n_tiles, g.tiles_per_wg, tile_m);
    RJ_KLAUNCH(L, "setop_scan", k_setop_scan, 1, 1024, tile_m, g.n_tiles, tile_mbase, total);
    RJ_KLAUNCH(L, "setop_offsets", k_setop_offsets, g.grid, SETOP_THREADS, runs, n_runs, (int32_t)op, tile_mbase, g.n_tiles,
               g.tiles_per_wg, off);
}

void launch_setop_emit(const Launch& L, const uint32_t* off, uint32_t n_runs, uint32_t n_out, uint32_t* run_of, uint32_t max_grid) {
    if (!n_runs || !n_out) return;
    const SetopGrid g = setop_grid(n_out, SETOP_EMIT_TILE, max_grid);
    RJ_KLAUNCH(L, "setop_emit", k_setop_emit, g.grid, SETOP_THREADS, off, n_runs, n_out, g.n_tiles, g.tiles_per_wg, run_of);
}

}  // namespace rj
