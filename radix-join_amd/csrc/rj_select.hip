// rj_select.hip — the gfx950 (wave64) kernel of the selection (RJ_NODE_SELECT).
#include <hip/hip_ext.h>

#include "rj_kernels.hpp"
#include "rj_kernel_util.hpp"

namespace rj {

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
void launch_select(const Launch& L, const SelectProg* prog, uint32_t n_ops, uint32_t n_rows, uint32_t* out_ids,
                   unsigned long long* cursor, uint32_t grid) {
    if (!n_rows || !grid) return;
    RJ_KLAUNCH(L, "select", k_select, grid, SEL_THREADS, prog, n_ops, n_rows, out_ids, cursor);
}

// RJ_CTX_PREWARM: one harmless launch, so that HIP loads this translation unit's code object when the context is
// built.  n_rows = 0 gives n_tiles = 0: the tile loop of k_select (`tile < n_tiles`) does not run, and nothing before
// it reads or writes memory (no op is read: prog is not dereferenced).
void prewarm_select(const Launch& L, uint32_t* zeroed) {
    RJ_KLAUNCH(L, "prewarm", k_select, 1, SEL_THREADS, reinterpret_cast<const SelectProg*>(zeroed), 0u, 0u, zeroed,
               reinterpret_cast<unsigned long long*>(zeroed));
}

}  // namespace rj
