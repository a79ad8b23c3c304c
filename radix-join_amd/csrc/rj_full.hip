// rj_full.hip — gfx950 (wave64) kernels of the full outer joins (RJ_NODE_FULL).
#include <hip/hip_ext.h>

#include "rj_kernels.hpp"
#include "rj_kernel_util.hpp"
#include "rj_tuple_util.hpp"
#include "rj_outer_util.hpp"

#include <algorithm>
#include <type_traits>

namespace rj {

// ======================================================= full outer joins
// RJ_NODE_FULL: an outer join's rows plus, ONCE, every build row without a partner, with NULL in
// the probed side's columns.  The probe kernels are the outer join's bodies with FULL set: they
// write no key stream and leave one matched bit per build tuple in fp.flags.  The kernels below
// run AFTER them in the same stream — the launch boundary makes every flag visible — and emit
// the build rows through the same cursor and streams.
template <int KW, int CWB, int CWP>
__global__ __launch_bounds__(JN_THREADS) void k_full_bcast(FullParams fp) {
    constexpr bool     FULL = true;
    const OuterParams& op = fp.o;
    uint32_t* const    gflags = fp.flags;
#include "rj_outer_bcast_body.inc"
}
template <int KW, int CWB, int CWP>
__global__ __launch_bounds__(JN_THREADS) void k_full_join(FullParams fp) {
    constexpr bool     FULL = true;
    const OuterParams& op = fp.o;
    uint32_t* const    gflags = fp.flags;
#include "rj_outer_join_body.inc"
}

// Rows for the items of one chunk a workgroup wants to emit: bit j of `emit` is the thread's item
// j (lane-strided: item j of thread t is element j * JN_THREADS + t of the chunk).  Positions come
// from the wave ballots, so the lanes of a wave write consecutive rows for each j; ONE reservation
// on the output cursor per chunk.  Item j goes to row `first + pre[j]`; returns false when the
// chunk's rows would pass the stream capacity (they are counted only).  Contains barriers: every
// thread of the workgroup calls it.
template <int SPT>
__device__ __forceinline__ bool full_reserve(const OuterParams& op, uint32_t emit, uint32_t* s_wtot,
                                             unsigned long long* s_obase, uint32_t (&pre)[SPT], uint64_t& first) {
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint32_t       wave_total = 0;
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
        const uint64_t mk = __ballot((emit >> j) & 1u);
        pre[j] = wave_total + lane_prefix(mk);
        wave_total += (uint32_t)__popcll(mk);
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
    uint32_t       before = 0, total = 0;
    for (uint32_t w = 0; w < nw; ++w) {
        const uint32_t t = s_wtot[w];
        if (w < wid) before += t;
        total += t;
    }
    first = gbase + before;
    lds_barrier();  // s_wtot / s_obase are reused by the next call
    return gbase + total <= op.out_cap;
}

// The build tuples nobody matched (partitioned path): a grid-strided walk over the partitioned
// build arrays and the flags, lane-strided so that a wave reads 64 consecutive tuples and two flag
// words per item and writes consecutive rows.  A tuple whose bit is clear comes out with its
// carry as it is and the pad value (fp.pad_pc, then zeros) as the probed carry; which words the
// probed carry stream takes is a run-time property of o.pc.
template <int KW, int CWB>
__global__ __launch_bounds__(JN_THREADS) void k_full_unmatched(FullParams fp) {
    constexpr int BW = KW + CWB;
    __shared__ uint32_t s_wtot[JN_THREADS / 64];
    __shared__ unsigned long long s_obase;
    const OuterParams& op = fp.o;
    const uint32_t     n = op.offB[op.NP];
    for (uint64_t base = (uint64_t)blockIdx.x * JN_SUB; base < n; base += (uint64_t)gridDim.x * JN_SUB) {
        uint32_t emit = 0, pre[JN_SPT];
#pragma unroll
        for (int j = 0; j < JN_SPT; ++j) {
            const uint64_t i = base + (uint64_t)j * JN_THREADS + threadIdx.x;
            if (i < n) emit |= (uint32_t)!((fp.flags[i >> 5] >> (i & 31u)) & 1u) << j;
        }
        uint64_t first;
        if (!full_reserve<JN_SPT>(op, emit, s_wtot, &s_obase, pre, first)) continue;
#pragma unroll
        for (int j = 0; j < JN_SPT; ++j) {
            if (!((emit >> j) & 1u)) continue;
            const uint64_t row = first + pre[j];
            if constexpr (CWB >= 1) {
                uint32_t t[BW];
                part_tuple<KW, CWB>(op.Bw, op.packB, op.aosB, (uint32_t)(base + (uint64_t)j * JN_THREADS + threadIdx.x), t);
                uint32_t b0, b1, b2;
                tuple_carry<KW, CWB>(t, b0, b1, b2);
                stream_store(op.bc, row, b0, b1, b2);
            }
            stream_store(op.pc, row, fp.pad_pc, 0u, 0u);
        }
    }
}

// Build rows straight from the built child's column: those whose key is missing (NULL; FP64 NaN;
// any key when the key types differ) have no partner — the first radix pass dropped them, or the
// broadcast table never held them — and, with fp.use_flags (broadcast path, flags by child row),
// the rows whose flag stayed clear go out in the same sweep.
template <int KW, int CWB>
__global__ __launch_bounds__(JN_THREADS) void k_full_buildrows(FullParams fp) {
    __shared__ uint32_t s_wtot[JN_THREADS / 64];
    __shared__ unsigned long long s_obase;
    const OuterParams& op = fp.o;
    const uint32_t     n = op.B.n_rows;
    for (uint64_t base = (uint64_t)blockIdx.x * JN_SUB; base < n; base += (uint64_t)gridDim.x * JN_SUB) {
        uint32_t emit = 0, pre[JN_SPT];
#pragma unroll
        for (int j = 0; j < JN_SPT; ++j) {
            const uint64_t r = base + (uint64_t)j * JN_THREADS + threadIdx.x;
            if (r >= n) continue;
            uint32_t lo, hi;
            bool     unmatched = op.keyless || !src_key<KW>(op.B, (uint32_t)r, lo, hi);
            if (!unmatched && fp.use_flags) unmatched = !((fp.flags[r >> 5] >> (r & 31u)) & 1u);
            emit |= (uint32_t)unmatched << j;
        }
        uint64_t first;
        if (!full_reserve<JN_SPT>(op, emit, s_wtot, &s_obase, pre, first)) continue;
#pragma unroll
        for (int j = 0; j < JN_SPT; ++j) {
            if (!((emit >> j) & 1u)) continue;
            const uint64_t row = first + pre[j];
            if constexpr (CWB >= 1) {
                uint32_t b0, b1, b2;
                src_carry<CWB>(op.B, (uint32_t)(base + (uint64_t)j * JN_THREADS + threadIdx.x), b0, b1, b2);
                stream_store(op.bc, row, b0, b1, b2);
            }
            stream_store(op.pc, row, fp.pad_pc, 0u, 0u);
        }
    }
}

// ================================================================== launchers
// full outer joins: the outer join's shapes, both carries optional
void launch_full_bcast(const Launch& L, int key_words, int cw_optional, int cw_preserved, const FullParams& op,
                       uint32_t grid) {
    if (!grid) return;
    for_shape2("full_broadcast", key_words, cw_optional, cw_preserved, [&](auto KW, auto CWB, auto CWP) {
        RJ_KLAUNCH(L, "full_broadcast", (k_full_bcast<KW, CWB, CWP>), grid, JN_THREADS, op);
    });
}

void launch_full_join(const Launch& L, int key_words, int cw_optional, int cw_preserved, const FullParams& op,
                      uint32_t grid) {
    if (!grid) return;
    for_shape2("full_probe", key_words, cw_optional, cw_preserved, [&](auto KW, auto CWB, auto CWP) {
        RJ_KLAUNCH(L, "full_probe", (k_full_join<KW, CWB, CWP>), grid, JN_THREADS, op);
    });
}

void launch_full_unmatched(const Launch& L, int key_words, int cw_built, const FullParams& fp, uint32_t grid) {
    if (!grid) return;
    for_shape("full_unmatched", key_words, cw_built, [&](auto KW, auto CW) {
        RJ_KLAUNCH(L, "full_unmatched", (k_full_unmatched<KW, CW>), grid, JN_THREADS, fp);
    });
}

void launch_full_buildrows(const Launch& L, int key_words, int cw_built, const FullParams& fp, uint32_t grid) {
    if (!grid) return;
    for_shape("full_buildrows", key_words, cw_built, [&](auto KW, auto CW) {
        RJ_KLAUNCH(L, "full_buildrows", (k_full_buildrows<KW, CW>), grid, JN_THREADS, fp);
    });
}

// RJ_CTX_PREWARM: one harmless launch, so that HIP loads this translation unit's code object when the context is
// built.  A zeroed FullParams: o.B.n_rows = 0, so the row loop of k_full_buildrows (`base < n`) does not run; nothing
// before it reads or writes memory.
void prewarm_full(const Launch& L, uint32_t*) {
    RJ_KLAUNCH(L, "prewarm", (k_full_buildrows<1, 0>), 1, JN_THREADS, FullParams{});
}

}  // namespace rj
