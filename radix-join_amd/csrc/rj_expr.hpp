// rj_expr.hpp — the scalar expressions of RJ_NODE_MAP: the device program and the op functions, one
// set for the kernel (k_map, rj_map.hip) and the host (rj_debug_map_eval, which the CPU tests pin
// them through).  Semantics in include/rj.h.
//
// Every F64 op is rounded once: x_apply, the one function here that does floating-point arithmetic, is
// compiled under `#pragma clang fp contract(off)` (inside its body, so that the pragma does not reach
// the code of whoever includes this header).
#pragma once
#include <stdint.h>

#include "rj_device.hpp"

namespace rj {

constexpr int MAP_MAX_OPS = 128;  // RJ_MAP_MAX_OPS
constexpr int MAP_MAX_DEPTH = 8;  // RJ_MAP_MAX_DEPTH

// ---- geometry of k_map: the selection's.  A workgroup owns tiles of MAP_TILE consecutive rows: wave w
// of it evaluates rows [w * MAP_TILE / 4, (w + 1) * MAP_TILE / 4) of the tile, 64 consecutive ones per item.
constexpr int MAP_THREADS = 256;
constexpr int MAP_TILE = 4096;
constexpr int MAP_ITEMS = MAP_TILE / MAP_THREADS;  // rows per thread per tile
constexpr int MAP_BATCH = 2;                       // ... of which a thread evaluates this many together
static_assert(MAP_TILE % 256 == 0 && MAP_TILE % MAP_THREADS == 0 && MAP_ITEMS % MAP_BATCH == 0, "whole rows of threads; whole batches");

// opcodes: the values of rj_expr_opcode (rj_exec.hip asserts that they agree)
enum MapOpcode : int32_t {
    X_COL = 0, X_INT = 1, X_F64 = 2, X_NULL = 3,
    X_ADD = 4, X_SUB = 5, X_MUL = 6, X_DIV = 7, X_MOD = 8, X_NEG = 9, X_ABS = 10,
    X_EQ = 11, X_NEQ = 12, X_LT = 13, X_GT = 14, X_LEQ = 15, X_GEQ = 16,
    X_AND = 17, X_OR = 18, X_NOT = 19, X_IS_NULL = 20, X_IS_NOT_NULL = 21,
    X_COALESCE = 22, X_CASE = 23, X_TO_I64 = 24, X_TO_F64 = 25, X_OUT = 26
};

// One op as the kernel reads it.  `f64`: the type of the op's OPERANDS (of a and b for X_CASE, of the
// popped value for X_OUT, of the pushed value for a leaf), decided by the host.  `arity`: values popped.
struct MapOp {
    int32_t  op;     // MapOpcode
    int32_t  f64;
    int32_t  arity;
    int32_t  pad;
    int64_t  lit;    // X_INT / X_F64: the value's bits
    ColRef   a;      // X_COL
    uint8_t* out8;   // X_OUT: dense 8-byte results (INT64 / FP64), or nullptr
    uint8_t* out4;   // ... dense 4-byte results (an I64 expression declared INT32), or nullptr
    uint8_t* valid;  // ... validity bytes, nullptr = the expression cannot be NULL
};
// One small device buffer per node; every thread reads ops[k] at the same k, so the loads are scalar.
struct MapProg {
    MapOp ops[MAP_MAX_OPS];
};

constexpr uint64_t X_SIGN = 0x8000000000000000ull;
constexpr uint64_t X_CANONICAL_NAN = 0x7ff8000000000000ull;

__host__ __device__ inline double x_f64(uint64_t bits) {
    union {
        uint64_t u;
        double   d;
    } c;
    c.u = bits;
    return c.d;
}
__host__ __device__ inline uint64_t x_bits(double d) {
    union {
        uint64_t u;
        double   d;
    } c;
    c.d = d;
    return c.u;
}
__host__ __device__ inline bool x_is_nan(uint64_t bits) { return (bits & ~X_SIGN) > 0x7ff0000000000000ull; }

template <class T>
__host__ __device__ inline bool x_cmp(int op, T x, T y) {
    switch (op) {
    case X_EQ: return x == y;
    case X_NEQ: return x != y;
    case X_LT: return x < y;
    case X_GT: return x > y;
    case X_LEQ: return x <= y;
    default: return x >= y;
    }
}

// What a non-leaf op other than X_OUT leaves.  Operands in the order they were pushed: a, b, c (a unary
// op reads a, a binary one a and b); *n, *_null: their NULL flags.  Returns the bits, NULL flag in `rn`.
// The bits of a NULL result are unspecified except where rj.h says what the value is.
__host__ __device__ inline uint64_t x_apply(int op, bool f64, uint64_t a, bool an, uint64_t b, bool bn, uint64_t c, bool cn, bool& rn) {
#pragma clang fp contract(off)
    switch (op) {
    case X_ADD:
    case X_SUB:
    case X_MUL:
    case X_DIV:
    case X_MOD: {
        rn = an || bn;
        if (f64) {
            const double x = x_f64(a), y = x_f64(b);
            return x_bits(op == X_ADD ? x + y : (op == X_SUB ? x - y : (op == X_MUL ? x * y : x / y)));
        }
        if (op == X_ADD) return a + b;
        if (op == X_SUB) return a - b;
        if (op == X_MUL) return a * b;
        // a zero divisor gives NULL; INT64_MIN / -1 wraps (x86 would raise SIGFPE there): x / -1 = 0 - x, x % -1 = 0
        if (b == 0) {
            rn = true;
            return 0;
        }
        if (b == ~0ull) return op == X_DIV ? 0ull - a : 0ull;
        return op == X_DIV ? (uint64_t)((int64_t)a / (int64_t)b) : (uint64_t)((int64_t)a % (int64_t)b);
    }
    case X_NEG:
        rn = an;
        return f64 ? a ^ X_SIGN : 0ull - a;
    case X_ABS:
        rn = an;
        return f64 ? a & ~X_SIGN : ((int64_t)a < 0 ? 0ull - a : a);
    case X_EQ:
    case X_NEQ:
    case X_LT:
    case X_GT:
    case X_LEQ:
    case X_GEQ:
        rn = an || bn;
        return f64 ? x_cmp(op, x_f64(a), x_f64(b)) : x_cmp(op, (int64_t)a, (int64_t)b);
    case X_AND: {
        const bool a_false = !an && a == 0, b_false = !bn && b == 0;
        rn = !(a_false || b_false) && (an || bn);
        return !(a_false || b_false) && !rn;
    }
    case X_OR: {
        const bool a_true = !an && a != 0, b_true = !bn && b != 0;
        rn = !(a_true || b_true) && (an || bn);
        return a_true || b_true;
    }
    case X_NOT:
        rn = an;
        return a == 0;
    case X_IS_NULL:
        rn = false;
        return an;
    case X_IS_NOT_NULL:
        rn = false;
        return !an;
    case X_COALESCE:
        rn = an && bn;
        return an ? b : a;
    case X_CASE: {
        const bool take_b = an || a == 0;  // a: the condition; b, c: the two values
        rn = take_b ? cn : bn;
        return take_b ? c : b;
    }
    case X_TO_I64: {
        if (!f64) {
            rn = an;
            return a;
        }
        const double x = x_f64(a);
        const bool   in = x >= -9223372036854775808.0 && x < 9223372036854775808.0;  // (false for a NaN)
        rn = an || !in;
        return (uint64_t)(int64_t)(in ? x : 0.0);
    }
    case X_TO_F64:
        rn = an;
        return f64 ? a : x_bits((double)(int64_t)a);
    default:
        rn = true;
        return 0;
    }
}

// what X_OUT writes for a non-NULL value: a NaN comes out as the one canonical NaN
__host__ __device__ inline uint64_t x_out(bool f64, uint64_t v) { return f64 && x_is_nan(v) ? X_CANONICAL_NAN : v; }

}  // namespace rj
