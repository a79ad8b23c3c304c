// rj_sortkey.hpp — the order-preserving key encoding of RJ_NODE_SORT and RJ_NODE_GROUP and its
// inverse, one function each for the kernels (k_sort_encode, k_group_*) and the host
// (rj_debug_sort_key / rj_debug_sort_key_value, which the CPU tests pin them through).
#pragma once
#include <stdint.h>

namespace rj {

constexpr int32_t SORTKEY_DESC = 1;         // RJ_SORT_DESC
constexpr int32_t SORTKEY_NULLS_FIRST = 2;  // RJ_SORT_NULLS_FIRST

// The value bits of a non-NULL value as an unsigned key: a < b as values <=> key(a) < key(b) as
// unsigned numbers, equal as values <=> equal keys.  `width` 4: an INT32 (low word of `bits`, the key
// has 32 bits); 8: an INT64, or with `f64` a double under PostgreSQL's rules (-0.0 = +0.0, every NaN
// equal to every other and above +inf).  `desc`: the bitwise NOT, within the key's width.
__host__ __device__ inline uint64_t sort_key_bits(uint64_t bits, int width, bool f64, bool desc) {
    uint64_t k;
    if (width == 4) {
        k = (uint32_t)bits ^ 0x80000000u;
        return desc ? (uint32_t)~k : k;
    }
    if (f64) {
        const uint64_t mag = bits & 0x7fffffffffffffffull;
        if (mag > 0x7ff0000000000000ull) bits = 0x7ff8000000000000ull;  // any NaN -> one NaN, above +inf
        else if (mag == 0) bits = 0;                                    // -0.0 -> +0.0
        k = bits ^ ((bits >> 63) ? ~0ull : 0x8000000000000000ull);
    } else {
        k = bits ^ 0x8000000000000000ull;
    }
    return desc ? ~k : k;
}

// The inverse of sort_key_bits for a non-NULL key: the canonical value bits of every value that has
// this key (an INT32's in the low word).  For INT32 / INT64 that is the value itself; for a double
// +0.0 for either zero and 0x7ff8000000000000 for any NaN, every other value its own bits.  A grouping
// (RJ_NODE_GROUP) outputs its keys, and decodes the unsigned minima / maxima it keeps, through it.
__host__ __device__ inline uint64_t sort_key_value(uint64_t key, int width, bool f64, bool desc) {
    if (width == 4) {
        const uint32_t k = desc ? ~(uint32_t)key : (uint32_t)key;
        return k ^ 0x80000000u;
    }
    const uint64_t k = desc ? ~key : key;
    if (f64) return k ^ ((k >> 63) ? 0x8000000000000000ull : ~0ull);
    return k ^ 0x8000000000000000ull;
}

// The digit above the value bits of a nullable column: NULLs last unless nulls_first.
__host__ __device__ inline uint32_t sort_null_digit(bool is_null, bool nulls_first) {
    return (uint32_t)(is_null != nulls_first);
}

}  // namespace rj
