// rj_tuple_util.hpp — what the kernel files of the join path (rj_pages, rj_partition, rj_join, rj_bcast, rj_filter,
// rj_outer, rj_full, rj_agg .hip; rj_setop.hip) share: the hash mixers, stream stores, one tuple of a partitioned relation
// or of a child's columns, and the host side of the one shape rule.  Device code: include from a .hip file only.
#pragma once
#include "rj_kernel_util.hpp"

#include <type_traits>

namespace rj {

// ============================================================== small helpers
// Bijective finalisers (murmur3 fmix32 / fmix64).  The reference hashes with
// fmix64 (src/execute.cpp:21-27); the hash is not observable in results
// (SURVEY.md §2 #11), so INT32 keys use the cheaper 32-bit mix.  Because both
// are bijections the partitions store HASHED keys and the probe un-hashes on
// emit; equal hashed keys <=> equal keys.
__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}
__device__ __forceinline__ uint32_t unfmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x7ed1b41du;  // inverse of 0xc2b2ae35 mod 2^32
    h ^= (h >> 13) ^ (h >> 26);
    h *= 0xa5cb9243u;  // inverse of 0x85ebca6b mod 2^32
    h ^= h >> 16;
    return h;
}
__device__ __forceinline__ uint64_t fmix64(uint64_t k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdULL;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ULL;
    k ^= k >> 33;
    return k;
}
__device__ __forceinline__ uint64_t unfmix64(uint64_t k) {
    k ^= k >> 33;
    k *= 0x9cb4b2f8129337dbULL;  // inverse of 0xc4ceb9fe1a85ec53 mod 2^64
    k ^= k >> 33;
    k *= 0x4f74430c22a54005ULL;  // inverse of 0xff51afd7ed558ccd mod 2^64
    k ^= k >> 33;
    return k;
}

// 16-byte vector of four tuples' words.  Tuple runs start at arbitrary (4-byte aligned)
// offsets; gfx950 global loads only need dword alignment, so one dwordx4 replaces four
// dword loads and their address arithmetic.
typedef uint32_t u32x4a __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ void stream_store(const OutStream& o, uint64_t row, uint32_t lo,
                                             uint32_t hi, uint32_t x2 = 0u) {
    switch (o.mode) {
    case ST_DENSE96: {
        uint32_t* r = reinterpret_cast<uint32_t*>(o.base) + row * 3u;
        r[0] = lo;
        r[1] = hi;
        r[2] = x2;
        break;
    }
    case ST_DENSE32: reinterpret_cast<uint32_t*>(o.base)[row] = lo; break;
    case ST_DENSE64:
        reinterpret_cast<uint64_t*>(o.base)[row] = (uint64_t)lo | ((uint64_t)hi << 32);
        break;
    case ST_PAGED32: {
        uint32_t r = (uint32_t)row, p = r / ROWS32, i = r - p * ROWS32;
        *reinterpret_cast<uint32_t*>(o.base + (size_t)p * PAGE_BYTES + HDR32 + i * 4u) = lo;
        break;
    }
    case ST_PAGED64: {
        uint32_t r = (uint32_t)row, p = r / ROWS64, i = r - p * ROWS64;
        *reinterpret_cast<uint64_t*>(o.base + (size_t)p * PAGE_BYTES + HDR64 + i * 8u) =
            (uint64_t)lo | ((uint64_t)hi << 32);
        break;
    }
    default: break;
    }
}

// ============================================= tuples of a partitioned relation
// One tuple of a partitioned relation (the layouts radix_partition() writes: 12-byte tuples, 8-byte
// pairs, or word arrays whose last two carry words are one pair array).
template <int KW, int CW>
__device__ __forceinline__ void part_tuple(const Words& W, int pack, int aos, uint32_t idx, uint32_t (&t)[KW + CW]) {
    constexpr int NW = KW + CW;
    if constexpr (KW == 1 && CW == 2) {
        if (aos) {
            const uint32_t* p = W.w[0] + (size_t)idx * 3u;
            t[0] = p[0];
            t[1] = p[1];
            t[2] = p[2];
            return;
        }
    }
    if constexpr (KW == 1 && CW == 1) {
        if (pack) {
            const uint2 v = reinterpret_cast<const uint2*>(W.w[0])[idx];
            t[0] = v.x;
            t[1] = v.y;
            return;
        }
    }
    constexpr int NA = CW >= 2 ? NW - 2 : NW;
#pragma unroll
    for (int a = 0; a < NA; ++a) t[a] = W.w[a][idx];
    if constexpr (CW >= 2) {
        const uint2 v = reinterpret_cast<const uint2*>(W.w[NA])[idx];
        t[NA] = v.x;
        t[NA + 1] = v.y;
    }
}

// The carry words behind the key of such a tuple (words the shape does not have: zero).
template <int KW, int CW>
__device__ __forceinline__ void tuple_carry(const uint32_t (&t)[KW + CW], uint32_t& c0, uint32_t& c1, uint32_t& c2) {
    constexpr int W = KW + CW;
    c0 = CW >= 1 ? t[KW < W ? KW : 0] : 0u;
    c1 = CW >= 2 ? t[KW + 1 < W ? KW + 1 : 0] : 0u;
    c2 = CW == 3 ? t[W - 1] : 0u;
}

// A hashed key (lo, hi: KW words) back to the key the source column held.
template <int KW>
__device__ __forceinline__ void unhash_key(uint32_t lo, uint32_t hi, uint32_t& k0, uint32_t& k1) {
    if constexpr (KW == 1) {
        k0 = unfmix32(lo);
    } else {
        const uint64_t k64 = unfmix64((uint64_t)lo | ((uint64_t)hi << 32));
        k0 = (uint32_t)k64;
        k1 = (uint32_t)(k64 >> 32);
    }
}

// ================================================== tuples of a child's columns
// One tuple straight from a child's columns (TupleSrc), as the kernels without a partition pass form
// it: the hashed key (false: NULL or NaN, the row has no partner) and the carry words behind it.
template <int KW>
__device__ __forceinline__ bool src_key(const TupleSrc& s, uint32_t row, uint32_t& lo, uint32_t& hi) {
    bool ok = s.key.valid ? s.key.valid[row] != 0 : true;
    if constexpr (KW == 1) {
        uint32_t v = col_load32(s.key, row);
        lo = s.prehashed ? v : fmix32(v);
        hi = 0;
    } else {
        uint64_t k = col_load64(s.key, row);
        if (s.key_f64 && (k & 0x7ff0000000000000ull) == 0x7ff0000000000000ull &&
            (k & 0x000fffffffffffffull))
            ok = false;  // NaN never matches (see SrcLoader::hash_keys)
        uint64_t h = fmix64(k);
        lo = (uint32_t)h;
        hi = (uint32_t)(h >> 32);
    }
    return ok;
}
template <int CW>
__device__ __forceinline__ void src_carry(const TupleSrc& s, uint32_t row, uint32_t& c0, uint32_t& c1, uint32_t& c2) {
    c0 = c1 = c2 = 0;
    if constexpr (CW >= 1) {
        if (s.carry_mode == CARRY_WIDE) {
            if constexpr (CW >= 2) {
                if (s.wide == WIDE_64_32) {
                    const uint64_t v = col_load64(s.carry, row);
                    c0 = (uint32_t)v;
                    c1 = (uint32_t)(v >> 32);
                    c2 = col_load32(s.carry2, row);
                } else {
                    c0 = col_load32(s.carry, row);
                    c1 = col_load32(s.carry2, row);
                    if constexpr (CW == 3) c2 = col_load32(s.carry3, row);
                }
            }
        } else if (s.carry_mode == CARRY_ROWIDX) {
            c0 = row;
        } else if constexpr (CW == 1) {
            c0 = col_load32(s.carry, row);
        } else {
            uint64_t v = col_load64(s.carry, row);
            c0 = (uint32_t)v;
            c1 = (uint32_t)(v >> 32);
        }
    }
}

// floor(log2(v)): the index bits of the LDS tables, whose sizes are powers of two
constexpr uint32_t ilog2_u32(uint32_t v) { return v > 1 ? 1 + ilog2_u32(v / 2) : 0; }

// ============================================================= shape dispatch
// The one shape rule of the tuple kernels: one or two key words, zero to three carry words,
// KW + CW <= MAX_WORDS.  for_shape turns run-time word counts into compile-time ones: it walks the
// shapes in the order (KW, CW) and calls f(int_c<KW>, int_c<CW>) for the match, so a launcher
// instantiates exactly the kernels of the rule; any other count is an unsupported launch.
template <int N>
using int_c = std::integral_constant<int, N>;

template <int KW = 1, int CW = 0, class F>
static void for_shape(const char* name, int kw, int cw, F&& f) {
    if constexpr (KW > 2) {
        launch_failed(name, "no kernel for this key/carry word count", true);
    } else {
        if constexpr (KW + CW <= MAX_WORDS)
            if (kw == KW && cw == CW) return f(int_c<KW>{}, int_c<CW>{});
        for_shape<(CW < 3 ? KW : KW + 1), (CW < 3 ? CW + 1 : 0)>(name, kw, cw, f);
    }
}

// two carries behind the same key: f(int_c<KW>, int_c<CWA>, int_c<CWB>)
template <class F>
static void for_shape2(const char* name, int kw, int cwa, int cwb, F&& f) {
    for_shape(name, kw, cwa, [&](auto KW, auto CWA) {
        for_shape(name, kw, cwb, [&](auto KW2, auto CWB) {
            if constexpr (decltype(KW2)::value == decltype(KW)::value) f(KW, CWA, CWB);
        });
    });
}

}  // namespace rj
