// rj_fsum.hpp — the arithmetic of RJ_AGG_FSUM, the exactly rounded sum of FP64 values: one text for
// the kernels (k_fsum_*, rj_fsum.hip) and the host (rj_debug_fsum, which the CPU tests pin it through).
// Semantics in include/rj.h.
//
// The accumulator is a fixed-point number that holds every finite double exactly: FSUM_CHUNKS signed
// 64-bit chunks, chunk k of weight 2^(32 k) in units of 2^-1074 (the smallest subnormal, of which every
// double is a multiple).  Nominally a chunk holds 32 bits; the upper 32 are headroom, so that values are
// added and partial sums merged chunk by chunk with plain (or atomic) 64-bit adds and no carry between
// them.  The VALUE of an accumulator is sum(c[k] * 2^(32 k)) whatever the chunks hold, so propagating
// carries, merging and negating never change it, and the order of the adds cannot matter.
//
// Headroom.  One value changes a chunk by less than 2^32 in magnitude (fsum_split: three pieces of 32
// bits), so a chunk that starts below 2^33 absorbs 2^30 values before it could reach 2^63:
// FSUM_MAX_ADDS.  A propagated accumulator (fsum_propagate) has every chunk of its range but the top one
// in [0, 2^32); merging M of them, or the same number of single values, moves a chunk by less than
// M * 2^32.  Who adds and merges says next to the code why it stays below FSUM_MAX_ADDS.  The top chunk
// of a range is signed and takes what is left: a relation has fewer than 2^32 rows of less than 2^2046
// units each, so a sum is below 2^2078 < 2^(32 * 67 - 66) in magnitude and chunk 67 stays tiny.
#pragma once
#include <stdint.h>

#include "rj_device.hpp"

namespace rj {

typedef long long fsum_t;  // (the signed counterpart of the type the 64-bit atomics take)

constexpr int      FSUM_CHUNKS = 68;    // 68 * 32 = 2176 bits >= 2046 + 53 (the largest double's top bit) + 32 (2^32 rows)
constexpr int      FSUM_FLAGS = 68;     // word 68 of an accumulator in memory: FSUM_PINF | FSUM_NINF | FSUM_NAN
constexpr int      FSUM_WORDS = 72;     // ... padded to 576 bytes
constexpr uint64_t FSUM_M32 = 0xffffffffull;
constexpr uint64_t FSUM_MAX_ADDS = 1ull << 30;  // values or propagated partials per chunk between two propagations
constexpr uint32_t FSUM_PINF = 1, FSUM_NINF = 2, FSUM_NAN = 4;
constexpr int      FSUM_BLOCK = 4096;   // values per partial sum of the host twin: a tile of the kernels

// One value: a non-finite one sets `flag` and stays out of the chunks; a finite one that is not zero
// adds d[i] to chunk k + i (k >= 0, k + 2 <= 65).
struct FsumPieces {
    int32_t  k;  // -1: nothing to add
    uint32_t flag;
    fsum_t   d[3];
};

__host__ __device__ inline FsumPieces fsum_split(uint64_t bits) {
    FsumPieces     x{-1, 0u, {0, 0, 0}};
    const uint32_t e = (uint32_t)(bits >> 52) & 0x7ffu;
    uint64_t       m = bits & ((1ull << 52) - 1ull);
    const bool     neg = (bits >> 63) != 0;
    if (e == 0x7ffu) {
        x.flag = m ? FSUM_NAN : (neg ? FSUM_NINF : FSUM_PINF);
        return x;
    }
    if (e) m |= 1ull << 52;
    if (!m) return x;
    // the value is m * 2^p units: m << (p & 31), at most 84 bits, from chunk p >> 5 on
    const uint32_t p = (e ? e : 1u) - 1u, s = p & 31u;
    const uint64_t lo = m << s, hi = s ? m >> (64u - s) : 0ull;
    x.k = (int32_t)(p >> 5);
    x.d[0] = (fsum_t)(lo & FSUM_M32), x.d[1] = (fsum_t)(lo >> 32), x.d[2] = (fsum_t)hi;
    if (neg) x.d[0] = -x.d[0], x.d[1] = -x.d[1], x.d[2] = -x.d[2];
    return x;
}

// add(k, d): chunk k += d — a plain add on the host, an LDS atomic in the kernels
template <class Add>
__host__ __device__ inline void fsum_add(const FsumPieces& x, Add&& add) {
    if (x.k < 0) return;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (x.d[i]) add(x.k + i, x.d[i]);
}

// word k of `src` into word k of `dst`: a chunk is added, the flags are OR-ed
__host__ __device__ inline void fsum_merge_word(fsum_t* dst, const fsum_t* src, int k) {
    if (k < FSUM_CHUNKS)
        dst[k] += src[k];
    else if (k == FSUM_FLAGS)
        dst[k] |= src[k];
}

// Chunks [lo, hi] hold the whole value (every other chunk is 0).  Afterwards chunks [lo, hi) are in
// [0, 2^32) and chunk hi, signed, holds the rest: the value is negative exactly when c[hi] < 0.
__host__ __device__ inline void fsum_propagate(fsum_t* c, int lo, int hi) {
    fsum_t carry = 0;
    for (int k = lo; k < hi; ++k) {
        const fsum_t v = c[k] + carry;
        c[k] = v & (fsum_t)FSUM_M32;
        carry = v >> 32;  // (arithmetic: floor)
    }
    c[hi] += carry;
}

// After fsum_propagate: the accumulator becomes its magnitude, still propagated; true = it was negative.
__host__ __device__ inline bool fsum_magnitude(fsum_t* c, int lo, int hi) {
    if (c[hi] >= 0) return false;
    for (int k = lo; k <= hi; ++k) c[k] = -c[k];
    fsum_propagate(c, lo, hi);  // (chunks in (-2^32, 0] below a top >= 1: the top stays >= 0)
    return true;
}

// The magnitude in chunks [lo, hi] (fsum_magnitude), as 32-bit digits: the top chunk may hold two.
__host__ __device__ inline uint64_t fsum_digit(const fsum_t* c, int lo, int hi, int k) {
    if (k < lo || k > hi + 1) return 0ull;
    if (k < hi) return (uint64_t)c[k];
    return k == hi ? (uint64_t)c[hi] & FSUM_M32 : (uint64_t)c[hi] >> 32;
}

// The accumulator's value as a double, rounded to nearest, ties to even, once.  flags: the non-finite
// values that were seen; neg and chunks [lo, hi]: the finite ones' sum (fsum_magnitude).
__host__ __device__ inline uint64_t fsum_round(const fsum_t* c, int lo, int hi, bool neg, uint32_t flags) {
    if ((flags & FSUM_NAN) || ((flags & FSUM_PINF) && (flags & FSUM_NINF))) return 0x7ff8000000000000ull;
    if (flags & FSUM_PINF) return 0x7ff0000000000000ull;
    if (flags & FSUM_NINF) return 0xfff0000000000000ull;
    int t = hi + 1;
    while (t >= lo && fsum_digit(c, lo, hi, t) == 0) --t;
    if (t < lo) return 0ull;  // +0.0, whatever the signs of the zeros were
    const uint64_t sign = neg ? 1ull << 63 : 0ull;
    const int      top = 32 * t + 31 - __builtin_clz((uint32_t)fsum_digit(c, lo, hi, t));  // the magnitude's top bit
    const uint64_t low64 = fsum_digit(c, lo, hi, 0) | fsum_digit(c, lo, hi, 1) << 32;
    if (top <= 52) return sign | low64;  // a subnormal, or the first binade of the normals: the bit pattern itself
    // w = bits [top - 63, top] of the magnitude, its top bit at 63; below = is any bit under them set
    uint64_t w;
    bool     below = false;
    if (top <= 63) {
        w = low64 << (63 - top);
    } else {
        const int      l = top - 63, q = l >> 5, r = l & 31;
        const uint64_t a = fsum_digit(c, lo, hi, q) | fsum_digit(c, lo, hi, q + 1) << 32, b = fsum_digit(c, lo, hi, q + 2);
        w = r ? a >> r | b << (64 - r) : a;
        below = r && (fsum_digit(c, lo, hi, q) & ((1ull << r) - 1ull)) != 0;
        for (int k = lo; k < q && !below; ++k) below = c[k] != 0;
    }
    uint64_t   mant = w >> 11;  // 53 bits
    const bool guard = (w >> 10) & 1ull, sticky = (w & 0x3ffull) != 0 || below;
    int        shift = top - 52;  // the value is mant * 2^shift units
    if (guard && (sticky || (mant & 1ull))) {
        mant += 1;
        if (mant >> 53) mant >>= 1, shift += 1;
    }
    const int e = shift + 1;  // biased: 1.f * 2^(e - 1023) = mant * 2^(e - 1) units
    if (e >= 2047) return sign | 0x7ff0000000000000ull;
    return sign | (uint64_t)e << 52 | (mant & ((1ull << 52) - 1ull));
}

// The chunks that are not 0: [lo, hi], or lo = hi = 0 if there is none.  (The kernels find them with
// a ballot.)
inline void fsum_range_host(const fsum_t* c, int& lo, int& hi) {
    lo = hi = 0;
    bool any = false;
    for (int k = 0; k < FSUM_CHUNKS; ++k)
        if (c[k]) {
            if (!any) lo = k;
            any = true;
            hi = k;
        }
}

// rj_debug_fsum: the values in blocks of FSUM_BLOCK as the kernels take them in tiles — a partial sum
// per block, propagated and merged into the total, which is propagated after every merge.  Headroom:
// FSUM_BLOCK values per partial, and the total is propagated between any two merges.
inline void fsum_host(const uint64_t* bits, const uint8_t* is_null, uint64_t n, uint64_t* out_bits, int32_t* out_is_null) {
    fsum_t   total[FSUM_WORDS] = {0};
    uint64_t count = 0;
    int      lo, hi;
    for (uint64_t i0 = 0; i0 < n; i0 += FSUM_BLOCK) {
        fsum_t part[FSUM_WORDS] = {0};
        for (uint64_t i = i0; i < n && i < i0 + FSUM_BLOCK; ++i) {
            if (is_null && is_null[i]) continue;
            const FsumPieces x = fsum_split(bits[i]);
            part[FSUM_FLAGS] |= (fsum_t)x.flag;
            fsum_add(x, [&](int k, fsum_t d) { part[k] += d; });
            ++count;
        }
        fsum_range_host(part, lo, hi);
        fsum_propagate(part, lo, hi);
        for (int k = 0; k < FSUM_WORDS; ++k) fsum_merge_word(total, part, k);
        fsum_range_host(total, lo, hi);
        fsum_propagate(total, lo, hi);
    }
    fsum_range_host(total, lo, hi);
    fsum_propagate(total, lo, hi);
    const bool neg = fsum_magnitude(total, lo, hi);
    *out_is_null = count == 0;
    *out_bits = count ? fsum_round(total, lo, hi, neg, (uint32_t)total[FSUM_FLAGS]) : 0ull;
}

}  // namespace rj
