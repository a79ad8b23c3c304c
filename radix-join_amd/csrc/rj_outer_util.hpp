// rj_outer_util.hpp — the LDS table and the emit step that the outer and the full outer join kernels share
// (rj_outer.hip, rj_full.hip; the section comment of rj_outer.hip describes the table).  Device code: include
// from a .hip file only, behind rj_tuple_util.hpp.
#pragma once

namespace rj {

template <int KW>
struct OuterTable {
    static constexpr uint32_t NB = JN_CAP / 4, BMASK = NB - 1, LOG2 = ilog2_u32(NB);
    uint32_t (*w)[JN_CAP];  // [KW + 1]
    uint32_t* cnt;          // [NB]

    __device__ __forceinline__ static uint32_t home(uint32_t lo, uint32_t hi) {
        return ((lo ^ hi) * 0x9e3779b1u) >> (32 - LOG2);
    }
    // every thread of the workgroup; the caller puts a barrier behind it
    __device__ __forceinline__ void clear() const {
        for (uint32_t i = threadIdx.x; i < NB; i += blockDim.x) cnt[i] = 0;
    }
    // at most JN_RMAX inserts per table (load <= 50 %), so the walk ends
    __device__ __forceinline__ void insert(uint32_t lo, uint32_t hi, uint32_t ref) const {
        uint32_t b = home(lo, hi);
        while (true) {
            const uint32_t pos = atomicAdd(&cnt[b], 1u);
            if (pos < 4) {
                const uint32_t slot = b * 4 + pos;
                w[0][slot] = lo;
                if constexpr (KW == 2) w[1][slot] = hi;
                w[KW][slot] = ref;
                return;
            }
            b = (b + 1) & BMASK;
        }
    }
    // matches of one key in bucket b: bit mask over its valid slots; `more`: the bucket overflowed
    __device__ __forceinline__ uint32_t match(uint32_t b, uint32_t lo, uint32_t hi, bool& more) const {
        const uint32_t c = cnt[b];
        const uint4    kv = *reinterpret_cast<const uint4*>(&w[0][b * 4]);
        uint32_t       eq = (uint32_t)(kv.x == lo) | ((uint32_t)(kv.y == lo) << 1) | ((uint32_t)(kv.z == lo) << 2) |
                      ((uint32_t)(kv.w == lo) << 3);
        if constexpr (KW == 2) {
            const uint4 hv = *reinterpret_cast<const uint4*>(&w[1][b * 4]);
            eq &= (uint32_t)(hv.x == hi) | ((uint32_t)(hv.y == hi) << 1) | ((uint32_t)(hv.z == hi) << 2) |
                  ((uint32_t)(hv.w == hi) << 3);
        }
        more = c > 4;
        return eq & ((1u << min(c, 4u)) - 1u);
    }
};

// Probe SPT items per thread against the table and emit: every match of an item with probe[j]
// set, and one padded row for an item with padrow[j] set that has no match now and had none
// before (hit[j], which is updated).  Offsets from the wave ballots (a shuffle scan where some lane
// has several matches), ONE global reservation for the workgroup; rows beyond the stream capacity
// are counted, not written (the host runs the probe again with exact-size streams).
// bcarry(ref, b0, b1, b2) / pcarry(j, p0, p1, p2) deliver the carries.  Contains barriers: every
// thread of the workgroup calls it.
// FULL (RJ_NODE_FULL, compile time): every matched build tuple is also recorded — bit
// (ref - flag_base) of the workgroup's LDS words s_flag, which the caller merges into the node's
// flags in HBM — and no key stream is written (a full outer join has none).  The counting loop
// records, not the emitting one: a run that only counts (streams too small) flags all the same.
template <bool FULL, int KW, int CWB, int CWP, int SPT, class BCarry, class PCarry>
__device__ __forceinline__ void outer_emit(const OuterParams& op, const OuterTable<KW>& T, const bool (&probe)[SPT],
                                           const bool (&padrow)[SPT], bool (&hit)[SPT], const uint32_t (&klo)[SPT],
                                           const uint32_t (&khi)[SPT], uint32_t* s_wtot, unsigned long long* s_obase,
                                           BCarry bcarry, PCarry pcarry, uint32_t* s_flag = nullptr,
                                           uint32_t flag_base = 0) {
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint32_t       m[SPT], cnt[SPT], pre[SPT], wave_total = 0;
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
        m[j] = 0;
        if (probe[j]) {
            uint32_t b = OuterTable<KW>::home(klo[j], khi[j]);
            bool     more;
            do {
                uint32_t eq = T.match(b, klo[j], khi[j], more);
                m[j] += (uint32_t)__popc(eq);
                if constexpr (FULL) {
                    while (eq) {
                        const uint32_t bit = T.w[KW][b * 4 + (uint32_t)__builtin_ctz(eq)] - flag_base;
                        eq &= eq - 1;
                        // (a hot build tuple is flagged by many probes: look before the atomic)
                        if (!((s_flag[bit >> 5] >> (bit & 31u)) & 1u)) atomicOr(&s_flag[bit >> 5], 1u << (bit & 31u));
                    }
                }
                b = (b + 1) & OuterTable<KW>::BMASK;
            } while (more);
        }
        hit[j] = hit[j] || m[j] != 0;
        cnt[j] = m[j] ? m[j] : ((padrow[j] && !hit[j]) ? 1u : 0u);
    }
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
        uint32_t tot;
        if (__ballot(cnt[j] > 1) == 0) {
            const uint64_t mk = __ballot(cnt[j] == 1);
            pre[j] = lane_prefix(mk);
            tot = (uint32_t)__popcll(mk);
        } else {
            uint32_t incl = cnt[j];
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t t = __shfl_up(incl, off);
                if (lane >= (uint32_t)off) incl += t;
            }
            pre[j] = incl - cnt[j];
            tot = __shfl(incl, 63);
        }
        pre[j] += wave_total;
        wave_total += tot;
    }
    if (lane == 0) s_wtot[wid] = wave_total;
    lds_barrier();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (uint32_t w = 0; w < nw; ++w) tot += s_wtot[w];
        *s_obase = tot ? atomicAdd(op.out_cursor, (unsigned long long)tot) : 0ull;
    }
    lds_barrier();
    const uint64_t gbase = *s_obase;
    uint64_t       obase = gbase;
    uint32_t       block_total = 0;
    for (uint32_t w = 0; w < nw; ++w) {
        const uint32_t t = s_wtot[w];
        if (w < wid) obase += t;
        block_total += t;
    }
    if (gbase + block_total <= op.out_cap) {
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            if (cnt[j] == 0) continue;
            uint64_t row = obase + pre[j];
            uint32_t k0 = 0, k1 = 0;
            if (!FULL && op.key.mode != ST_NONE) unhash_key<KW>(klo[j], khi[j], k0, k1);
            uint32_t p0 = 0, p1 = 0, p2 = 0;
            if constexpr (CWP >= 1) pcarry(j, p0, p1, p2);
            if (m[j] == 0) {  // no partner in any round: the padded row
                if constexpr (!FULL) stream_store(op.key, row, k0, k1);
                if constexpr (CWB >= 1) stream_store(op.bc, row, op.pad_bc, 0u, 0u);
                if constexpr (CWP >= 1) stream_store(op.pc, row, p0, p1, p2);
                continue;
            }
            uint32_t b = OuterTable<KW>::home(klo[j], khi[j]);
            bool     more;
            do {
                uint32_t eq = T.match(b, klo[j], khi[j], more);
                while (eq) {
                    const uint32_t slot = b * 4 + (uint32_t)__builtin_ctz(eq);
                    eq &= eq - 1;
                    if constexpr (!FULL) stream_store(op.key, row, k0, k1);
                    if constexpr (CWB >= 1) {
                        uint32_t b0, b1, b2;
                        bcarry(T.w[KW][slot], b0, b1, b2);
                        stream_store(op.bc, row, b0, b1, b2);
                    }
                    if constexpr (CWP >= 1) stream_store(op.pc, row, p0, p1, p2);
                    ++row;
                }
                b = (b + 1) & OuterTable<KW>::BMASK;
            } while (more);
        }
    }
    lds_barrier();  // s_wtot / s_obase are reused by the next call
}

}  // namespace rj
