// rj_filter.hip — gfx950 (wave64) kernels of the semi / anti joins (RJ_NODE_SEMI, RJ_NODE_ANTI).
#include <hip/hip_ext.h>

#include "rj_kernels.hpp"
#include "rj_kernel_util.hpp"
#include "rj_tuple_util.hpp"

#include <algorithm>
#include <type_traits>

namespace rj {

// ====================================================== semi / anti joins
// RJ_NODE_SEMI / RJ_NODE_ANTI ask "has this preserved row a partner on the filter side?".  The
// filter side's DISTINCT hashed keys go into an LDS set; the preserved tuples are looked up and
// each one that hits (SEMI) or misses (ANTI) is emitted ONCE — the un-hashed key and its carry,
// ballot/mbcnt offsets inside the wave, one global reservation per JN_SUB tuples (as k_join_bcast).
// Nothing travels with a filter key, so a slot is the hashed key alone: 32 KiB (KW = 1) or 64 KiB
// (KW = 2) for JN_CAP slots, of which at most JN_RMAX are used (load <= 50 %).
//   insert  open addressing, linear probing, one LDS compare-and-swap per step: a key that is
//           already there is not stored again (duplicates collapse on insert);
//   lookup  walk from the home slot until the key or an EMPTY slot.
// EMPTY is the all-ones word; a filter key whose hash is all ones sets a flag instead of a slot.
// The home slot is the multiplicative hash of the key words: their low radix bits are the same for
// a whole partition, the product's high bits are not.
static_assert((JN_CAP & (JN_CAP - 1)) == 0, "set slots: a power of two");

template <int KW>
struct FilterSet {
    using Slot = std::conditional_t<KW == 1, uint32_t, unsigned long long>;
    static constexpr Slot     EMPTY = ~Slot(0);
    static constexpr uint32_t LOG2 = ilog2_u32(JN_CAP), MASK = JN_CAP - 1;
    Slot*     t;         // [JN_CAP]
    uint32_t* count;     // distinct keys in the slots
    uint32_t* sentinel;  // 1: the EMPTY key itself is in the set

    __device__ __forceinline__ static Slot make(uint32_t lo, uint32_t hi) {
        if constexpr (KW == 1)
            return lo;
        else
            return (Slot)lo | ((Slot)hi << 32);
    }
    __device__ __forceinline__ static uint32_t home(uint32_t lo, uint32_t hi) {
        return ((lo ^ hi) * 0x9e3779b1u) >> (32 - LOG2);
    }
    // every thread of the workgroup; the caller puts a barrier behind it
    __device__ __forceinline__ void clear() const {
        uint4* t4 = reinterpret_cast<uint4*>(t);
        for (uint32_t i = threadIdx.x; i < JN_CAP * sizeof(Slot) / 16; i += blockDim.x)
            t4[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
        if (threadIdx.x == 0) {
            *count = 0;
            *sentinel = 0;
        }
    }
    // true: the key was not in the set before
    __device__ __forceinline__ bool insert(uint32_t lo, uint32_t hi) const {
        const Slot k = make(lo, hi);
        if (k == EMPTY) {
            *sentinel = 1u;
            return false;
        }
        uint32_t s = home(lo, hi);
        while (true) {
            const Slot prev = atomicCAS(&t[s], EMPTY, k);
            if (prev == EMPTY) return true;
            if (prev == k) return false;
            s = (s + 1) & MASK;
        }
    }
    __device__ __forceinline__ bool has(uint32_t lo, uint32_t hi) const {
        const Slot k = make(lo, hi);
        if (k == EMPTY) return *sentinel != 0;
        uint32_t s = home(lo, hi);
        while (true) {
            const Slot v = t[s];
            if (v == k) return true;
            if (v == EMPTY) return false;
            s = (s + 1) & MASK;
        }
    }
};

// Emit the items with e[j] set: offsets from the wave ballots, ONE global reservation for the
// workgroup, then the un-hashed key (key stream) and carry(j, p0, p1, p2) (preserved carry stream).
// Contains barriers: every thread of the workgroup calls it.
template <int KW, int SPT, class Carry>
__device__ __forceinline__ void filter_emit(const FilterParams& fp, const bool (&e)[SPT], const uint32_t (&klo)[SPT],
                                            const uint32_t (&khi)[SPT], uint32_t* s_wtot,
                                            unsigned long long* s_obase, Carry carry) {
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint32_t       pre[SPT], wave_total = 0;
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
        const uint64_t mk = __ballot(e[j]);
        pre[j] = wave_total + lane_prefix(mk);
        wave_total += (uint32_t)__popcll(mk);
    }
    if (lane == 0) s_wtot[wid] = wave_total;
    lds_barrier();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (uint32_t w = 0; w < nw; ++w) tot += s_wtot[w];
        *s_obase = tot ? atomicAdd(fp.out_cursor, (unsigned long long)tot) : 0ull;
    }
    lds_barrier();
    uint64_t obase = *s_obase;
    for (uint32_t w = 0; w < wid; ++w) obase += s_wtot[w];
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
        const uint64_t row = obase + pre[j];
        // (the output never holds more rows than the preserved side: the bound is a guard only)
        if (!e[j] || row >= fp.out_cap) continue;
        if (fp.key.mode != ST_NONE) {
            uint32_t k0, k1 = 0;
            unhash_key<KW>(klo[j], khi[j], k0, k1);
            stream_store(fp.key, row, k0, k1);
        }
        if (fp.pc.mode != ST_NONE) {
            uint32_t p0, p1, p2;
            carry(j, p0, p1, p2);
            stream_store(fp.pc, row, p0, p1, p2);
        }
    }
    lds_barrier();  // s_wtot / s_obase are reused by the next chunk
}

// Broadcast form: a filter side of at most JN_RMAX rows.  Every workgroup builds the SAME set
// straight from the filter child's key column (page decode, NULL / NaN drop, hashing on the way)
// and streams a grid-strided slice of the preserved child past it.  A preserved row whose key is
// NULL or NaN has no partner: ANTI emits it.  keyless (the key types differ): no key is read,
// every row misses.
template <int KW, int CWS>
__global__ __launch_bounds__(JN_THREADS) void k_filter_bcast(FilterParams fp) {
    using Set = FilterSet<KW>;
    __shared__ __attribute__((aligned(16))) typename Set::Slot t_set[JN_CAP];
    __shared__ uint32_t s_cnt[2];
    __shared__ uint32_t s_wtot[JN_THREADS / 64];
    __shared__ unsigned long long s_obase;
    const Set set{t_set, &s_cnt[0], &s_cnt[1]};
    set.clear();
    lds_barrier();
    if (!fp.keyless) {
        for (uint32_t r = threadIdx.x; r < fp.F.n_rows; r += JN_THREADS) {
            uint32_t lo, hi;
            if (src_key<KW>(fp.F, r, lo, hi)) (void)set.insert(lo, hi);
        }
    }
    lds_barrier();
    const uint32_t n = fp.P.n_rows;
    for (uint64_t base = (uint64_t)blockIdx.x * JN_SUB; base < n; base += (uint64_t)gridDim.x * JN_SUB) {
        uint32_t klo[JN_SPT], khi[JN_SPT];
        bool     e[JN_SPT];
#pragma unroll
        for (int j = 0; j < JN_SPT; ++j) {
            const uint64_t row = base + (uint64_t)j * JN_THREADS + threadIdx.x;
            klo[j] = khi[j] = 0;
            e[j] = false;
            if (row < n) {
                bool hit = false;
                if (!fp.keyless && src_key<KW>(fp.P, (uint32_t)row, klo[j], khi[j])) hit = set.has(klo[j], khi[j]);
                e[j] = fp.anti ? !hit : hit;
            }
        }
        filter_emit<KW, JN_SPT>(fp, e, klo, khi, s_wtot, &s_obase, [&](int j, uint32_t& p0, uint32_t& p1, uint32_t& p2) {
            src_carry<CWS>(fp.P, (uint32_t)(base + (uint64_t)j * JN_THREADS + threadIdx.x), p0, p1, p2);
        });
    }
}

// ANTI on the partitioned path: the preserved rows the first radix pass drops (NULL key; FP64 NaN
// key) have no partner, so they belong to the result.  Grid-strided over the preserved child, the
// same tuple formation (src_key / src_carry over the TupleSrc) and output cursor as the filter.
template <int KW, int CWS>
__global__ __launch_bounds__(JN_THREADS) void k_filter_nullkeys(FilterParams fp) {
    __shared__ uint32_t s_wtot[JN_THREADS / 64];
    __shared__ unsigned long long s_obase;
    const uint32_t n = fp.P.n_rows;
    for (uint64_t base = (uint64_t)blockIdx.x * JN_SUB; base < n; base += (uint64_t)gridDim.x * JN_SUB) {
        uint32_t klo[JN_SPT], khi[JN_SPT];
        bool     e[JN_SPT];
#pragma unroll
        for (int j = 0; j < JN_SPT; ++j) {
            const uint64_t row = base + (uint64_t)j * JN_THREADS + threadIdx.x;
            klo[j] = khi[j] = 0;
            e[j] = row < n && !src_key<KW>(fp.P, (uint32_t)row, klo[j], khi[j]);
        }
        filter_emit<KW, JN_SPT>(fp, e, klo, khi, s_wtot, &s_obase, [&](int j, uint32_t& p0, uint32_t& p1, uint32_t& p2) {
            src_carry<CWS>(fp.P, (uint32_t)(base + (uint64_t)j * JN_THREADS + threadIdx.x), p0, p1, p2);
        });
    }
}

// Partitioned form: one workgroup per co-partition, or per heavy task of a preserved partition
// above JN_HEAVY tuples (k_heavy_tasks; it leaves partitions WITHOUT filter tuples to the main
// workgroups, which is where ANTI emits them whole).  The set is built from the partition's filter
// keys in blocks of JN_RMAX / 2 tuples for as long as it holds at most JN_RMAX / 2 distinct keys,
// so a round ends with at most JN_RMAX of them.  A partition that needs more than one round (more
// distinct filter keys than one set holds: a forced radix_bits, or adversarial hashes) is exact
// all the same: every JN_SUB-tuple chunk of preserved tuples stays in registers while the rounds
// are rebuilt one after the other, its per-tuple hit flags OR-ed over them, and is emitted after
// the last one.  No memory outside the LDS holds a flag.
template <int KW, int CWS>
__global__ __launch_bounds__(JN_THREADS) void k_filter_join(FilterParams fp) {
    using Set = FilterSet<KW>;
    constexpr int      TH = JN_THREADS, SPT = JN_SPT, SUB = JN_SUB, SW = KW + CWS;
    constexpr uint32_t RB = JN_RMAX / 2;  // filter tuples per insert block
    static_assert(SPT * TH == SUB, "sub-chunk geometry");
    __shared__ __attribute__((aligned(16))) typename Set::Slot t_set[JN_CAP];
    __shared__ uint32_t s_cnt[2];
    __shared__ uint32_t s_wtot[TH / 64];
    __shared__ unsigned long long s_obase;
    const Set set{t_set, &s_cnt[0], &s_cnt[1]};

    uint32_t q, sbeg, send;
    if (blockIdx.x < fp.heavy_grid) {
        if (blockIdx.x >= *fp.n_heavy) return;
        q = fp.heavy_tasks[3 * blockIdx.x + 0];
        sbeg = fp.heavy_tasks[3 * blockIdx.x + 1];
        send = fp.heavy_tasks[3 * blockIdx.x + 2];
    } else {
        q = blockIdx.x - fp.heavy_grid;
        if (q >= fp.NP) return;
        sbeg = fp.offP[q];
        send = fp.offP[q + 1];
        if (send - sbeg > JN_HEAVY && fp.offF[q + 1] != fp.offF[q]) return;  // split into heavy tasks
    }
    const uint32_t rbeg = fp.offF[q], rend = fp.offF[q + 1];
    if (sbeg >= send || (!fp.anti && rbeg == rend)) return;

    // one round of the set: filter tuples from `from` on; returns where the round ended
    auto build_round = [&](uint32_t from) -> uint32_t {
        lds_barrier();  // nobody still looks up the previous round
        set.clear();
        lds_barrier();
        uint32_t cur = from;
        while (cur < rend) {
            const uint32_t nb = min(RB, rend - cur);
            uint32_t       added = 0;
            for (uint32_t i = threadIdx.x; i < nb; i += TH) {
                const uint32_t lo = fp.Fw.w[0][cur + i], hi = KW == 2 ? fp.Fw.w[KW - 1][cur + i] : 0u;
                added += set.insert(lo, hi) ? 1u : 0u;
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) added += __shfl_xor(added, off);
            if ((threadIdx.x & 63u) == 0 && added) atomicAdd(set.count, added);
            lds_barrier();
            cur += nb;
            const uint32_t distinct = *set.count;
            lds_barrier();  // every thread has read the count before the next block adds to it
            if (distinct > (uint32_t)JN_RMAX - RB) break;
        }
        return cur;
    };

    uint32_t sw[SPT][SW];
    auto load_chunk = [&](uint32_t sc, uint32_t sn) {
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            // (items past the chunk re-read its last tuple; they are masked off)
            const uint32_t idx = sc + min((uint32_t)(j * TH + threadIdx.x), sn - 1u);
            part_tuple<KW, CWS>(fp.Pw, fp.packP, fp.aosP, idx, sw[j]);
        }
    };

    const uint32_t first_end = build_round(rbeg);
    const bool     one_round = first_end == rend;
    for (uint32_t sc = sbeg; sc < send; sc += SUB) {
        const uint32_t sn = min((uint32_t)SUB, send - sc);
        load_chunk(sc, sn);
        bool hit[SPT];
#pragma unroll
        for (int j = 0; j < SPT; ++j) hit[j] = false;
        uint32_t end = (one_round || sc == sbeg) ? first_end : build_round(rbeg);
        while (true) {
#pragma unroll
            for (int j = 0; j < SPT; ++j)
                if ((uint32_t)(j * TH + threadIdx.x) < sn && !hit[j]) hit[j] = set.has(sw[j][0], KW == 2 ? sw[j][KW - 1] : 0u);
            if (end == rend) break;
            end = build_round(end);
        }
        uint32_t klo[SPT], khi[SPT];
        bool     e[SPT];
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            klo[j] = sw[j][0];
            khi[j] = KW == 2 ? sw[j][KW - 1] : 0u;
            e[j] = (uint32_t)(j * TH + threadIdx.x) < sn && (fp.anti ? !hit[j] : hit[j]);
        }
        filter_emit<KW, SPT>(fp, e, klo, khi, s_wtot, &s_obase, [&](int j, uint32_t& p0, uint32_t& p1, uint32_t& p2) {
            tuple_carry<KW, CWS>(sw[j], p0, p1, p2);
        });
    }
}

// ================================================================== launchers
// semi / anti joins: the preserved side's carry
void launch_filter_bcast(const Launch& L, int key_words, int cw_preserved, const FilterParams& fp, uint32_t grid) {
    if (!grid) return;
    for_shape("filter_broadcast", key_words, cw_preserved, [&](auto KW, auto CW) {
        RJ_KLAUNCH(L, "filter_broadcast", (k_filter_bcast<KW, CW>), grid, JN_THREADS, fp);
    });
}

void launch_filter_join(const Launch& L, int key_words, int cw_preserved, const FilterParams& fp, uint32_t grid) {
    if (!grid) return;
    for_shape("filter_probe", key_words, cw_preserved, [&](auto KW, auto CW) {
        RJ_KLAUNCH(L, "filter_probe", (k_filter_join<KW, CW>), grid, JN_THREADS, fp);
    });
}

void launch_filter_nullkeys(const Launch& L, int key_words, int cw_preserved, const FilterParams& fp, uint32_t grid) {
    if (!grid) return;
    for_shape("filter_nullkeys", key_words, cw_preserved, [&](auto KW, auto CW) {
        RJ_KLAUNCH(L, "filter_nullkeys", (k_filter_nullkeys<KW, CW>), grid, JN_THREADS, fp);
    });
}

// RJ_CTX_PREWARM: one harmless launch, so that HIP loads this translation unit's code object when the context is
// built.  A zeroed FilterParams: fp.P.n_rows = 0, so the row loop of k_filter_nullkeys (`base < n`) does not run;
// nothing before it reads or writes memory.
void prewarm_filter(const Launch& L, uint32_t*) {
    RJ_KLAUNCH(L, "prewarm", (k_filter_nullkeys<1, 0>), 1, JN_THREADS, FilterParams{});
}

}  // namespace rj
