// rj_agg.hip — gfx950 (wave64) kernels of the hash aggregation (RJ_NODE_AGG).
#include <hip/hip_ext.h>

#include "rj_kernels.hpp"
#include "rj_kernel_util.hpp"
#include "rj_tuple_util.hpp"

#include <algorithm>
#include <type_traits>

namespace rj {

// ============================================================ aggregation
// RJ_NODE_AGG: GROUP BY the key of ONE partitioned relation (rj_device.hpp, AggParams).
// part_tuple's inverse: a tuple goes back into the partition layout (the tuples k_agg_parts defers).
template <int KW, int CW>
__device__ __forceinline__ void part_tuple_store(const Words& W, int pack, int aos, uint32_t idx, const uint32_t (&t)[KW + CW]) {
    constexpr int NW = KW + CW;
    if constexpr (KW == 1 && CW == 2) {
        if (aos) {
            uint32_t* p = W.w[0] + (size_t)idx * 3u;
            p[0] = t[0];
            p[1] = t[1];
            p[2] = t[2];
            return;
        }
    }
    if constexpr (KW == 1 && CW == 1) {
        if (pack) {
            reinterpret_cast<uint2*>(W.w[0])[idx] = make_uint2(t[0], t[1]);
            return;
        }
    }
    constexpr int NA = CW >= 2 ? NW - 2 : NW;
#pragma unroll
    for (int a = 0; a < NA; ++a) W.w[a][idx] = t[a];
    if constexpr (CW >= 2) reinterpret_cast<uint2*>(W.w[NA])[idx] = make_uint2(t[NA], t[NA + 1]);
}

constexpr long long AGG_MIN_INIT = 0x7fffffffffffffffll, AGG_MAX_INIT = -0x7fffffffffffffffll - 1;

// value of carried column `a` in the carry words c0..c2 (selects, no indexed registers); false = NULL
__device__ __forceinline__ bool agg_value(const AggCol& a, int valid_word, uint32_t c0, uint32_t c1, uint32_t c2, long long& v) {
    const uint32_t vw = valid_word == 0 ? c0 : (valid_word == 1 ? c1 : c2);
    if (a.valid_bit >= 0 && !((vw >> a.valid_bit) & 1u)) return false;
    const uint32_t lo = a.word == 0 ? c0 : (a.word == 1 ? c1 : c2), hi = a.word == 0 ? c1 : c2;
    v = a.width == 4 ? (long long)(int32_t)lo : (long long)((uint64_t)lo | ((uint64_t)hi << 32));
    return true;
}

// The merge table's entry of a hashed key (open addressing over m_slots entries; the key that
// equals the "nobody's" pattern owns entry m_slots); 0xffffffff and *m_overflow set when the walk
// finds neither the key nor a free entry within AGG_MERGE_WALK steps.
constexpr uint32_t AGG_MERGE_WALK = 4096, AGG_NO_ENTRY = 0xffffffffu;
__device__ __forceinline__ uint32_t agg_merge_entry(const AggParams& ap, unsigned long long k64) {
    if (k64 == AGG_NO_KEY) return ap.m_slots;
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(ap.m.key);
    const uint32_t      mask = ap.m_slots - 1u;
    uint32_t            slot = (uint32_t)((k64 * 0x9e3779b97f4a7c15ull) >> 32) & mask;
    if (ap.m_slots)
        for (uint32_t pr = 0; pr < AGG_MERGE_WALK && pr < ap.m_slots; ++pr) {
            unsigned long long cur = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == AGG_NO_KEY) {
                cur = atomicCAS(&keys[slot], AGG_NO_KEY, k64);
                if (cur == AGG_NO_KEY) cur = k64;
            }
            if (cur == k64) return slot;
            slot = (slot + 1u) & mask;
        }
    atomicOr(ap.m_overflow, 1u);
    return AGG_NO_ENTRY;
}
// one partial group -> the merge table (ordinary vector atomics in HBM)
template <int NC>
__device__ __forceinline__ void agg_merge(const AggParams& ap, uint32_t entry, unsigned long long rows,
                                          const unsigned long long (&nn)[NC], const unsigned long long (&sum)[NC],
                                          const long long (&mn)[NC], const long long (&mx)[NC]) {
    if (entry == AGG_NO_ENTRY) return;
    atomicAdd(&ap.m.rows[entry], rows);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        if (c >= ap.n_cols || nn[c] == 0) continue;
        atomicAdd(&ap.m.nn[c][entry], nn[c]);
        if (ap.col[c].need & AGG_NEED_SUM) atomicAdd(&ap.m.sum[c][entry], sum[c]);
        if (ap.col[c].need & AGG_NEED_MIN) atomicMin(&ap.m.mn[c][entry], mn[c]);
        if (ap.col[c].need & AGG_NEED_MAX) atomicMax(&ap.m.mx[c][entry], mx[c]);
    }
}
// one finished group -> row `row` of the node's output arrays; the key is un-hashed, as the join does
template <int KW, int NC>
__device__ __forceinline__ void agg_write(const AggParams& ap, uint64_t row, unsigned long long k64, bool null_key,
                                          unsigned long long rows, const unsigned long long (&nn)[NC],
                                          const unsigned long long (&sum)[NC], const long long (&mn)[NC],
                                          const long long (&mx)[NC]) {
    if (row >= ap.out_cap) return;
    if (ap.out.key) {
        if constexpr (KW == 1)
            reinterpret_cast<uint32_t*>(ap.out.key)[row] = null_key ? 0u : unfmix32((uint32_t)k64);
        else
            reinterpret_cast<unsigned long long*>(ap.out.key)[row] = null_key ? 0ull : unfmix64(k64);
    }
    if (null_key && ap.out_keyvalid) ap.out_keyvalid[row] = 0;
    if (ap.out.rows) ap.out.rows[row] = rows;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        if (c >= ap.n_cols) continue;
        if (ap.out.nn[c]) ap.out.nn[c][row] = nn[c];
        if (ap.out.sum[c]) ap.out.sum[c][row] = sum[c];
        if (ap.out.mn[c]) ap.out.mn[c][row] = mn[c];
        if (ap.out.mx[c]) ap.out.mx[c][row] = mx[c];
    }
}

template <int NC>
struct AggTable {
    unsigned long long key[AGG_CAP];
    uint32_t           rows[AGG_CAP];
    uint32_t           nn[NC][AGG_CAP];
    unsigned long long sum[NC][AGG_CAP];
    long long          mn[NC][AGG_CAP], mx[NC][AGG_CAP];
};

// One workgroup per partition, or per heavy task of a partition above JN_HEAVY tuples.  The LDS
// table is open addressing over AGG_CAP entries, keyed by the hashed key words (64-bit compare and
// swap; the "free" pattern is a key word 0 whose lowest radix bit differs from the partition's, so
// no key of the partition equals it); the accumulators are LDS atomics: 32-bit counts, 64-bit add
// and signed min / max.  The tuples go by in steps of AGG_STEP; between two steps every thread
// reads the table's fill, and from AGG_FREEZE keys on the round is FROZEN: a tuple whose key is
// not in the table (or — before that — that found the AGG_WALK entries from its home taken) is put back into the
// partition's own memory from its start, always behind the read position, and is aggregated in the
// next round with a fresh table.  A key that is in the table catches every later tuple of its
// own, and a key that was turned away once never enters the same round (free entries only
// vanish, and the frozen state only begins at a barrier), so every key is emitted in exactly one
// round.  A partition's main workgroup reserves the rows of all groups of a round at once and
// writes them; a heavy task adds its groups to the merge table in HBM instead (k_agg_emit).
template <int KW, int CW>
__global__ __launch_bounds__(AGG_THREADS) void k_agg_parts(AggParams ap) {
    constexpr int NW = KW + CW, NC = CW ? CW : 1;
    __shared__ AggTable<NC>       T;
    __shared__ uint32_t           s_used, s_ndefer, s_wsum[AGG_THREADS / 64];
    __shared__ unsigned long long s_obase;
    const bool heavy = blockIdx.x < ap.heavy_grid;
    uint32_t   b, e;
    if (heavy) {
        if (blockIdx.x >= *ap.n_heavy) return;
        b = ap.heavy_tasks[3 * blockIdx.x + 1];
        e = ap.heavy_tasks[3 * blockIdx.x + 2];
    } else {
        const uint32_t q = blockIdx.x - ap.heavy_grid;
        if (q >= ap.NP) return;
        b = ap.off[q];
        e = ap.off[q + 1];
        if (e - b > JN_HEAVY) return;  // (its tasks do it)
    }
    if (b >= e) return;
    unsigned long long EMPTY;
    {
        uint32_t t0[NW];
        part_tuple<KW, CW>(ap.W, ap.pack, ap.aos, b, t0);
        EMPTY = (unsigned long long)(t0[0] ^ 1u);
    }
    uint32_t rd_e = e;
    while (true) {
        for (uint32_t i = threadIdx.x; i < AGG_CAP; i += AGG_THREADS) {
            T.key[i] = EMPTY;
            T.rows[i] = 0;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                T.nn[c][i] = 0;
                T.sum[c][i] = 0;
                T.mn[c][i] = AGG_MIN_INIT;
                T.mx[c][i] = AGG_MAX_INIT;
            }
        }
        if (threadIdx.x == 0) {
            s_used = 0;
            s_ndefer = 0;
        }
        __syncthreads();
        for (uint64_t base = b; base < rd_e; base += AGG_STEP) {
            // (nobody changes s_used between the barrier that ended the last step and the next one)
            const bool frozen = *(volatile uint32_t*)&s_used >= (uint32_t)AGG_FREEZE;
            uint32_t   t[AGG_SPT][NW];
            bool       live[AGG_SPT];
#pragma unroll
            for (int j = 0; j < AGG_SPT; ++j) {
                const uint64_t idx = base + (uint64_t)j * AGG_THREADS + threadIdx.x;
                live[j] = idx < rd_e;
                if (live[j]) part_tuple<KW, CW>(ap.W, ap.pack, ap.aos, (uint32_t)idx, t[j]);
            }
            __syncthreads();  // every tuple of the step is in registers before a deferred one lands on it
#pragma unroll
            for (int j = 0; j < AGG_SPT; ++j) {
                if (!live[j]) continue;
                const uint32_t           lo = t[j][0], hi = KW == 2 ? t[j][KW - 1] : 0u;
                const unsigned long long k64 = (unsigned long long)lo | ((unsigned long long)hi << 32);
                uint32_t                 slot = ((lo ^ hi) * 0x9e3779b1u) >> (32 - ilog2_u32(AGG_CAP));
                bool                     found = false;
                for (uint32_t pr = 0; pr < (uint32_t)AGG_WALK; ++pr) {
                    unsigned long long cur = __hip_atomic_load(&T.key[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (cur == EMPTY && !frozen) {
                        cur = atomicCAS(&T.key[slot], EMPTY, k64);
                        if (cur == EMPTY) {
                            atomicAdd(&s_used, 1u);
                            cur = k64;
                        }
                    }
                    if (cur == k64) {
                        found = true;
                        break;
                    }
                    if (cur == EMPTY) break;  // frozen, and the key is not in the table
                    slot = (slot + 1u) & (uint32_t)(AGG_CAP - 1);
                }
                if (!found) {
                    const uint32_t pos = atomicAdd(&s_ndefer, 1u);
                    part_tuple_store<KW, CW>(ap.W, ap.pack, ap.aos, b + pos, t[j]);
                    continue;
                }
                atomicAdd(&T.rows[slot], 1u);
                if constexpr (CW >= 1) {
                    const uint32_t c0 = t[j][KW], c1 = CW >= 2 ? t[j][KW + (CW >= 2 ? 1 : 0)] : 0u,
                                   c2 = CW >= 3 ? t[j][KW + (CW >= 3 ? 2 : 0)] : 0u;
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        long long v;
                        if (c >= ap.n_cols || !agg_value(ap.col[c], ap.valid_word, c0, c1, c2, v)) continue;
                        atomicAdd(&T.nn[c][slot], 1u);
                        if (ap.col[c].need & AGG_NEED_SUM) atomicAdd(&T.sum[c][slot], (unsigned long long)v);
                        if (ap.col[c].need & AGG_NEED_MIN) atomicMin(&T.mn[c][slot], v);
                        if (ap.col[c].need & AGG_NEED_MAX) atomicMax(&T.mx[c][slot], v);
                    }
                }
            }
            __syncthreads();
        }
        // ---- the round's groups
        constexpr int      EPT = AGG_CAP / AGG_THREADS;
        uint32_t           cnt = 0;
#pragma unroll
        for (int k = 0; k < EPT; ++k) cnt += T.key[threadIdx.x + k * AGG_THREADS] != EMPTY;
        uint64_t row = 0;
        if (!heavy) {
            uint32_t       total;
            const uint32_t pre = block_excl_scan(cnt, s_wsum, total);
            if (threadIdx.x == 0) s_obase = total ? atomicAdd(ap.out_cursor, (unsigned long long)total) : 0ull;
            __syncthreads();
            row = s_obase + pre;
        }
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
            const uint32_t           i = threadIdx.x + k * AGG_THREADS;
            const unsigned long long k64 = T.key[i];
            if (k64 == EMPTY) continue;
            unsigned long long nn[NC], sum[NC];
            long long          mn[NC], mx[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                nn[c] = T.nn[c][i];
                sum[c] = T.sum[c][i];
                mn[c] = T.mn[c][i];
                mx[c] = T.mx[c][i];
            }
            if (heavy)
                agg_merge<NC>(ap, agg_merge_entry(ap, k64), T.rows[i], nn, sum, mn, mx);
            else
                agg_write<KW, NC>(ap, row++, k64, false, T.rows[i], nn, sum, mn, mx);
        }
        const uint32_t nd = *(volatile uint32_t*)&s_ndefer;
        if (nd == 0) break;
        // the deferred tuples, written by any thread of the workgroup, are read by any other next round
        __threadfence();
        __syncthreads();
        __threadfence();
        rd_e = b + nd;
    }
}

// The rows whose key is NULL: the first radix pass drops them; they form one group (SQL's GROUP BY),
// entry m_slots + 1 of the merge table.  Grid-strided over the child's columns, per-thread
// accumulators, a wave reduction, one set of atomics per wave that saw such a row.
template <int CW>
__global__ __launch_bounds__(JN_THREADS) void k_agg_nullkey(AggParams ap) {
    constexpr int      NC = CW ? CW : 1;
    unsigned long long rows = 0, nn[NC], sum[NC];
    long long          mn[NC], mx[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        nn[c] = sum[c] = 0;
        mn[c] = AGG_MIN_INIT;
        mx[c] = AGG_MAX_INIT;
    }
    const uint32_t n = ap.src.n_rows;
    for (uint64_t r = (uint64_t)blockIdx.x * JN_THREADS + threadIdx.x; r < n; r += (uint64_t)gridDim.x * JN_THREADS) {
        if (ap.src.key.valid[r]) continue;
        ++rows;
        if constexpr (CW >= 1) {
            uint32_t c0, c1, c2;
            src_carry<CW>(ap.src, (uint32_t)r, c0, c1, c2);
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                long long v;
                if (c >= ap.n_cols || !agg_value(ap.col[c], ap.valid_word, c0, c1, c2, v)) continue;
                ++nn[c];
                sum[c] += (unsigned long long)v;
                mn[c] = min(mn[c], v);
                mx[c] = max(mx[c], v);
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        rows += __shfl_xor(rows, off);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            nn[c] += __shfl_xor(nn[c], off);
            sum[c] += __shfl_xor(sum[c], off);
            mn[c] = min(mn[c], __shfl_xor(mn[c], off));
            mx[c] = max(mx[c], __shfl_xor(mx[c], off));
        }
    }
    if ((threadIdx.x & 63u) == 0 && rows) agg_merge<NC>(ap, ap.m_slots + 1u, rows, nn, sum, mn, mx);
}

// the merge table before anybody adds to it
__global__ __launch_bounds__(256) void k_agg_merge_init(AggParams ap) {
    const uint64_t n = (uint64_t)ap.m_slots + 2;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        reinterpret_cast<unsigned long long*>(ap.m.key)[i] = AGG_NO_KEY;
        ap.m.rows[i] = 0;
        for (int c = 0; c < ap.n_cols; ++c) {
            ap.m.nn[c][i] = 0;
            ap.m.sum[c][i] = 0;
            ap.m.mn[c][i] = AGG_MIN_INIT;
            ap.m.mx[c][i] = AGG_MAX_INIT;
        }
    }
}

// The live entries of the merge table -> rows of the output, through the same cursor as
// k_agg_parts: one reservation per 256 entries.  The NULL-key group's key comes out NULL.
template <int KW>
__global__ __launch_bounds__(256) void k_agg_emit(AggParams ap) {
    __shared__ uint32_t           s_wsum[256 / 64];
    __shared__ unsigned long long s_obase;
    const uint64_t n = (uint64_t)ap.m_slots + 2;
    for (uint64_t base = (uint64_t)blockIdx.x * 256; base < n; base += (uint64_t)gridDim.x * 256) {
        const uint64_t i = base + threadIdx.x;
        const bool     live = i < n && ap.m.rows[i] != 0;
        uint32_t       total;
        const uint32_t pre = block_excl_scan(live ? 1u : 0u, s_wsum, total);
        if (threadIdx.x == 0) s_obase = total ? atomicAdd(ap.out_cursor, (unsigned long long)total) : 0ull;
        __syncthreads();
        if (live) {
            unsigned long long nn[AGG_MAX_COLS], sum[AGG_MAX_COLS];
            long long          mn[AGG_MAX_COLS], mx[AGG_MAX_COLS];
#pragma unroll
            for (int c = 0; c < AGG_MAX_COLS; ++c) {
                const bool has = c < ap.n_cols;
                nn[c] = has ? ap.m.nn[c][i] : 0;
                sum[c] = has ? ap.m.sum[c][i] : 0;
                mn[c] = has ? ap.m.mn[c][i] : 0;
                mx[c] = has ? ap.m.mx[c][i] : 0;
            }
            const unsigned long long k64 = i < ap.m_slots ? reinterpret_cast<const unsigned long long*>(ap.m.key)[i] : AGG_NO_KEY;
            agg_write<KW, AGG_MAX_COLS>(ap, s_obase + pre, k64, i == (uint64_t)ap.m_slots + 1, ap.m.rows[i], nn, sum, mn, mx);
        }
        __syncthreads();
    }
}

// An accumulator array as a result column: narrowed to 32 bits for an INT32 MIN / MAX (dst,
// optional), and NULL where the group had no value (dst_valid, optional; nn = nullptr: never).
template <int WIDTH>
__global__ __launch_bounds__(256) void k_agg_column(const unsigned long long* src, const unsigned long long* nn, uint64_t n,
                                                    uint8_t* dst, uint8_t* dst_valid) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (dst) {
        if (WIDTH == 4)
            reinterpret_cast<uint32_t*>(dst)[i] = (uint32_t)src[i];
        else
            reinterpret_cast<unsigned long long*>(dst)[i] = src[i];
    }
    if (dst_valid) dst_valid[i] = nn ? (nn[i] != 0) : 1;
}

// ================================================================== launchers
void launch_agg_merge_init(const Launch& L, const AggParams& ap, uint32_t grid) {
    RJ_KLAUNCH(L, "agg_merge_init", k_agg_merge_init, grid, 256, ap);
}
void launch_agg_parts(const Launch& L, int key_words, int carry_words, const AggParams& ap, uint32_t grid) {
    if (!grid) return;
    for_shape("agg_parts", key_words, carry_words, [&](auto KW, auto CW) {
        RJ_KLAUNCH(L, "agg_parts", (k_agg_parts<KW, CW>), grid, AGG_THREADS, ap);
    });
}
void launch_agg_nullkey(const Launch& L, int carry_words, const AggParams& ap, uint32_t grid) {
    if (!grid) return;
    for_shape("agg_nullkey", 1, carry_words, [&](auto, auto CW) {  // (no key: the carries of a one-word key)
        RJ_KLAUNCH(L, "agg_nullkey", (k_agg_nullkey<CW>), grid, JN_THREADS, ap);
    });
}
void launch_agg_emit(const Launch& L, int key_words, const AggParams& ap, uint32_t grid) {
    if (key_words == 1)
        RJ_KLAUNCH(L, "agg_emit", (k_agg_emit<1>), grid, 256, ap);
    else
        RJ_KLAUNCH(L, "agg_emit", (k_agg_emit<2>), grid, 256, ap);
}
void launch_agg_column(const Launch& L, const unsigned long long* src, const unsigned long long* nn, uint64_t n, int width,
                       uint8_t* dst, uint8_t* dst_valid) {
    if (!n) return;
    const uint32_t grid = (uint32_t)((n + 255) / 256);
    if (width == 4)
        RJ_KLAUNCH(L, "agg_column", (k_agg_column<4>), grid, 256, src, nn, n, dst, dst_valid);
    else
        RJ_KLAUNCH(L, "agg_column", (k_agg_column<8>), grid, 256, src, nn, n, dst, dst_valid);
}

// RJ_CTX_PREWARM: one harmless launch, so that HIP loads this translation unit's code object when the context is
// built.  n = 0: every thread of k_agg_column leaves at `i >= n`, its first check, before any pointer is read.
void prewarm_agg(const Launch& L, uint32_t* zeroed) {
    const unsigned long long* const z = reinterpret_cast<const unsigned long long*>(zeroed);
    RJ_KLAUNCH(L, "prewarm", (k_agg_column<4>), 1, 256, z, z, (uint64_t)0, reinterpret_cast<uint8_t*>(zeroed),
               reinterpret_cast<uint8_t*>(zeroed));
}

}  // namespace rj
