// rj_map.hip — the gfx950 (wave64) kernel of RJ_NODE_MAP and its launcher.
#include "rj_expr.hpp"
#include "rj_kernel_util.hpp"

#pragma clang fp contract(off)

namespace rj {

// RJ_NODE_MAP: the postfix program of rj_expr.hpp (MapProg) over a relation's columns; every X_OUT writes
// one dense result column (+ validity bytes where the host could not prove the expression non-NULL).
// ALL expressions of a node are evaluated in this one launch.
//
// The program is the same for every row, so the op loop, the stack pointer and every branch on an op are
// uniform and ops[k] is read with scalar loads.  A thread evaluates MAP_BATCH rows op by op, so that the
// loads of one leaf are in flight together.  Geometry: the selection's (rj_expr.hpp) — wave w owns the
// w-th quarter of a tile, 64 consecutive rows per item, so every load and store of an item is one run
// of 64 values.
//
// The value stack is MAP_MAX_DEPTH x MAP_BATCH 64-bit NAMED registers: eight variables of their own,
// which RJ_MAP_SLOT reaches through a switch on the (uniform) stack pointer.  They must not be the
// rows of ONE array: the compiler then merges the arms of the switch into one access at a computed
// address, and a runtime-indexed private array lives in scratch (profiles/map_codeobj.log).  LDS laid out
// [slot][thread] would cost 32 KiB per workgroup and an LDS round trip per operand.  The NULL flags are one bit per slot in
// one register per row, as the selection's truth bits are.
using MapSlot = uint64_t[MAP_BATCH];
#define RJ_MAP_SLOTS s0, s1, s2, s3, s4, s5, s6, s7
#define RJ_MAP_ARM(I, S, STMT) \
    case I:                    \
        _Pragma("unroll") for (int j = 0; j < MAP_BATCH; ++j) { MapSlot& S_ = S; STMT; } \
        break;
// STMT for every row j of the batch with S_ = slot `i` (a uniform value below MAP_MAX_DEPTH).  A macro and
// not a function over eight references: inside a function the slots are pointer arguments, and the
// compiler merges the arms into one access through a selected pointer before it inlines.
#define RJ_MAP_SLOT(i, STMT)       \
    switch (i) {                   \
        RJ_MAP_ARM(0, s0, STMT)    \
        RJ_MAP_ARM(1, s1, STMT)    \
        RJ_MAP_ARM(2, s2, STMT)    \
        RJ_MAP_ARM(3, s3, STMT)    \
        RJ_MAP_ARM(4, s4, STMT)    \
        RJ_MAP_ARM(5, s5, STMT)    \
        RJ_MAP_ARM(6, s6, STMT)    \
        default: RJ_MAP_ARM(7, s7, STMT) \
    }
static_assert(MAP_MAX_DEPTH == 8, "RJ_MAP_SLOT names eight slots");

__global__ __launch_bounds__(MAP_THREADS) void k_map(const MapProg* __restrict__ prog, uint32_t n_ops, uint32_t n_rows) {
    constexpr uint32_t NWAVES = MAP_THREADS / 64, WAVE_ROWS = MAP_TILE / NWAVES;
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    const uint32_t n_tiles = n_rows / MAP_TILE + (n_rows % MAP_TILE != 0);  // (n_rows + MAP_TILE - 1 may not fit 32 bits)
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t tile_base = tile * MAP_TILE;  // (< n_rows)
        const uint32_t in_tile = min((uint32_t)MAP_TILE, n_rows - tile_base);
        const uint32_t local0 = wid * WAVE_ROWS + lane;  // item i: row tile_base + local0 + 64 i
#pragma unroll 1
        for (uint32_t b = 0; b < MAP_ITEMS; b += MAP_BATCH) {
            if (wid * WAVE_ROWS + 64u * b >= in_tile) break;  // (the same for the whole wave)
            uint32_t row[MAP_BATCH];
            bool     live[MAP_BATCH];
#pragma unroll
            for (int j = 0; j < MAP_BATCH; ++j) {
                const uint32_t local = local0 + 64u * (b + j);
                live[j] = local < in_tile;
                row[j] = tile_base + (live[j] ? local : 0u);  // (a row that exists: rows past the end compute and write nothing)
            }
            MapSlot  RJ_MAP_SLOTS;  // the value stack: eight variables of their own, never one array
            uint32_t nul[MAP_BATCH];  // bit s: slot s holds a NULL
#pragma unroll
            for (int j = 0; j < MAP_BATCH; ++j) nul[j] = 0;
            uint32_t sp = 0;
#pragma unroll 1
            for (uint32_t k = 0; k < n_ops; ++k) {
                const MapOp&   o = prog->ops[k];
                const int      op = o.op;
                const bool     f64 = o.f64 != 0;
                const uint32_t arity = (uint32_t)o.arity;
                uint64_t       r[MAP_BATCH];
                uint32_t       rn = 0;  // bit j: row j's result is NULL
                if (op == X_COL) {
                    const ColRef c = o.a;
#pragma unroll
                    for (int j = 0; j < MAP_BATCH; ++j) {
                        r[j] = c.width == 4 ? (uint64_t)(int64_t)(int32_t)col_load32(c, row[j]) : col_load64(c, row[j]);
                        if (c.valid) rn |= (uint32_t)(c.valid[row[j]] == 0) << j;
                    }
                } else if (op <= X_NULL) {
#pragma unroll
                    for (int j = 0; j < MAP_BATCH; ++j) r[j] = (uint64_t)o.lit;
                    rn = op == X_NULL ? ~0u : 0u;
                } else {
                    uint64_t x[MAP_BATCH], y[MAP_BATCH], z[MAP_BATCH];  // in the order they were pushed
#pragma unroll
                    for (int j = 0; j < MAP_BATCH; ++j) x[j] = y[j] = z[j] = 0;
                    const uint32_t base = sp - arity;  // (the host checked: arity <= sp)
                    RJ_MAP_SLOT(base, x[j] = S_[j])
                    if (arity >= 2) RJ_MAP_SLOT(base + 1, y[j] = S_[j])
                    if (arity >= 3) RJ_MAP_SLOT(base + 2, z[j] = S_[j])
                    if (op == X_OUT) {
#pragma unroll
                        for (int j = 0; j < MAP_BATCH; ++j) {
                            if (!live[j]) continue;
                            const bool     is_null = (nul[j] >> base) & 1u;
                            const uint64_t v = x_out(f64, x[j]);
                            if (o.out8) reinterpret_cast<uint64_t*>(o.out8)[row[j]] = v;
                            if (o.out4) reinterpret_cast<uint32_t*>(o.out4)[row[j]] = (uint32_t)v;
                            if (o.valid) o.valid[row[j]] = is_null ? 0 : 1;
                        }
                        sp = base;
                        continue;
                    }
                    // ONE branch on the op per batch: inside an arm the op is a constant, and x_apply folds to its case
#define RJ_MAP_OP(OP)                                                                                                      \
    case OP:                                                                                                               \
        _Pragma("unroll") for (int j = 0; j < MAP_BATCH; ++j) {                                                            \
            bool n1 = false;                                                                                               \
            r[j] = x_apply(OP, f64, x[j], (nul[j] >> base) & 1u, y[j], (nul[j] >> (base + 1)) & 1u, z[j],                  \
                           (nul[j] >> (base + 2)) & 1u, n1);                                                               \
            rn |= (uint32_t)n1 << j;                                                                                       \
        }                                                                                                                  \
        break;
                    switch (op) {
                        RJ_MAP_OP(X_ADD) RJ_MAP_OP(X_SUB) RJ_MAP_OP(X_MUL) RJ_MAP_OP(X_DIV) RJ_MAP_OP(X_MOD) RJ_MAP_OP(X_NEG) RJ_MAP_OP(X_ABS)
                        RJ_MAP_OP(X_EQ) RJ_MAP_OP(X_NEQ) RJ_MAP_OP(X_LT) RJ_MAP_OP(X_GT) RJ_MAP_OP(X_LEQ) RJ_MAP_OP(X_GEQ)
                        RJ_MAP_OP(X_AND) RJ_MAP_OP(X_OR) RJ_MAP_OP(X_NOT) RJ_MAP_OP(X_IS_NULL) RJ_MAP_OP(X_IS_NOT_NULL)
                        RJ_MAP_OP(X_COALESCE) RJ_MAP_OP(X_CASE) RJ_MAP_OP(X_TO_I64) RJ_MAP_OP(X_TO_F64)
                    default:  // (the host checked the opcodes)
#pragma unroll
                        for (int j = 0; j < MAP_BATCH; ++j) r[j] = 0;
                        rn = ~0u;
                        break;
                    }
#undef RJ_MAP_OP
                    sp = base;
                }
                RJ_MAP_SLOT(sp, S_[j] = r[j])
#pragma unroll
                for (int j = 0; j < MAP_BATCH; ++j) nul[j] = (nul[j] & ((1u << sp) - 1u)) | (((rn >> j) & 1u) << sp);
                ++sp;
            }
        }
    }
}
#undef RJ_MAP_SLOT
#undef RJ_MAP_ARM
#undef RJ_MAP_SLOTS

void launch_map(const Launch& L, const MapProg* prog, uint32_t n_ops, uint32_t n_rows, uint32_t grid) {
    if (!n_rows || !n_ops || !grid) return;
    RJ_KLAUNCH(L, "map", k_map, grid, MAP_THREADS, prog, n_ops, n_rows);
}

}  // namespace rj
