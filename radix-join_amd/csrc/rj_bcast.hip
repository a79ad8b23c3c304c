// rj_bcast.hip — the gfx950 (wave64) kernel of the broadcast inner join: a build side of at most JN_RMAX rows,
// nothing partitioned (the inner join node; the partitioned form, k_join, is rj_join.hip).
#include <hip/hip_ext.h>

#include "rj_kernels.hpp"
#include "rj_kernel_util.hpp"
#include "rj_tuple_util.hpp"

#include <algorithm>
#include <type_traits>

namespace rj {

// ============================================================ broadcast join
// A build side of at most JN_RMAX rows (the filtered dimension tables of the JOB plans: a
// handful of rows against millions) needs no partitioning: every workgroup builds the SAME
// LDS table straight from the build child's columns and streams a slice of the probe
// child's columns past it — page decode, NULL-key drop and hashing happen on the way, the
// probe side is read exactly once and nothing is scattered.  (The reference counterpart is
// still hash_join_omp, src/execute.cpp:44-262, with num_buckets = 1.)
// The table keeps key words + the build ROW; build carries are fetched from the build
// columns on emit (a few KB: cache resident).  With no radix digit to derive an EMPTY
// sentinel from, a slot is valid when its index is below its bucket's insert counter.
template <int KW, int CWR, int CWS>
__global__ __launch_bounds__(JN_THREADS) void k_join_bcast(BcastParams bp) {
    constexpr int RW = KW + 1;  // key words + build row
    __shared__ __attribute__((aligned(16))) uint32_t t_w[RW][JN_CAP];
    __shared__ __attribute__((aligned(16))) uint32_t t_cnt[JN_CAP / 4];
    __shared__ uint32_t s_wtot[JN_THREADS / 64];
    __shared__ unsigned long long s_obase;
    const uint32_t     lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    constexpr uint32_t BMASK = JN_CAP / 4 - 1;

    // ---- build (identical in every workgroup)
    for (uint32_t i = threadIdx.x; i < JN_CAP / 4; i += JN_THREADS) t_cnt[i] = 0;
    lds_barrier();
    for (uint32_t r = threadIdx.x; r < bp.R.n_rows; r += JN_THREADS) {
        uint32_t lo, hi;
        if (!src_key<KW>(bp.R, r, lo, hi)) continue;
        uint32_t b = lo & BMASK;
        while (true) {
            uint32_t pos = atomicAdd(&t_cnt[b], 1u);
            if (pos < 4) {
                const uint32_t slot = b * 4 + pos;
                t_w[0][slot] = lo;
                if constexpr (KW == 2) t_w[1][slot] = hi;
                t_w[KW][slot] = r;
                break;
            }
            b = (b + 1) & BMASK;
        }
    }
    lds_barrier();

    // matches of one probe key in bucket b: bit mask over its (valid) slots; `more` = the
    // bucket overflowed, the walk goes on in the next one
    auto match = [&](uint32_t b, uint32_t lo, uint32_t hi, bool& more) -> uint32_t {
        const uint32_t cnt = t_cnt[b];
        const uint4    kv = *reinterpret_cast<const uint4*>(&t_w[0][b * 4]);
        uint32_t       eq = (uint32_t)(kv.x == lo) | ((uint32_t)(kv.y == lo) << 1) |
                      ((uint32_t)(kv.z == lo) << 2) | ((uint32_t)(kv.w == lo) << 3);
        if constexpr (KW == 2) {
            const uint4 hv = *reinterpret_cast<const uint4*>(&t_w[1][b * 4]);
            eq &= (uint32_t)(hv.x == hi) | ((uint32_t)(hv.y == hi) << 1) |
                  ((uint32_t)(hv.z == hi) << 2) | ((uint32_t)(hv.w == hi) << 3);
        }
        more = cnt > 4;
        return eq & ((1u << min(cnt, 4u)) - 1u);
    };

    // ---- probe: chunks of JN_SUB rows, strided over the grid
    const uint32_t n = bp.S.n_rows;
    for (uint64_t base = (uint64_t)blockIdx.x * JN_SUB; base < n; base += (uint64_t)gridDim.x * JN_SUB) {
        uint32_t klo[JN_SPT], khi[JN_SPT], m[JN_SPT];
#pragma unroll
        for (int j = 0; j < JN_SPT; ++j) {
            const uint64_t row = base + (uint64_t)j * JN_THREADS + threadIdx.x;
            m[j] = 0;
            klo[j] = khi[j] = 0;
            if (row < n && src_key<KW>(bp.S, (uint32_t)row, klo[j], khi[j])) {
                uint32_t b = klo[j] & BMASK;
                bool     more;
                do {
                    m[j] += (uint32_t)__popc(match(b, klo[j], khi[j], more));
                    b = (b + 1) & BMASK;
                } while (more);
            }
        }
        // output offsets: wave prefix (ballot when every lane has <= 1 match), one global
        // reservation per chunk
        uint32_t pre[JN_SPT], wave_total = 0;
#pragma unroll
        for (int j = 0; j < JN_SPT; ++j) {
            uint32_t tot;
            if (__ballot(m[j] > 1) == 0) {
                uint64_t mk = __ballot(m[j] == 1);
                pre[j] = lane_prefix(mk);
                tot = (uint32_t)__popcll(mk);
            } else {
                uint32_t incl = m[j];
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    uint32_t t = __shfl_up(incl, off);
                    if (lane >= (uint32_t)off) incl += t;
                }
                pre[j] = incl - m[j];
                tot = __shfl(incl, 63);
            }
            pre[j] += wave_total;
            wave_total += tot;
        }
        if (lane == 0) s_wtot[wid] = wave_total;
        lds_barrier();
        if (threadIdx.x == 0) {
            uint32_t tot = 0;
            for (int w = 0; w < JN_THREADS / 64; ++w) tot += s_wtot[w];
            s_obase = tot ? atomicAdd(bp.out_cursor, (unsigned long long)tot) : 0ull;
        }
        lds_barrier();
        const uint64_t gbase = s_obase;
        uint64_t       obase = gbase;
        uint32_t       block_total = 0;
        for (uint32_t w = 0; w < JN_THREADS / 64; ++w) {
            uint32_t t = s_wtot[w];
            if (w < wid) obase += t;
            block_total += t;
        }
        // rows beyond the stream capacity are counted but not written (the host re-runs the
        // join with exact-size buffers)
        if (gbase + block_total <= bp.out_cap) {
#pragma unroll
            for (int j = 0; j < JN_SPT; ++j) {
                if (m[j] == 0) continue;
                const uint32_t srow = (uint32_t)(base + (uint64_t)j * JN_THREADS + threadIdx.x);
                uint64_t       row = obase + pre[j];
                uint32_t       k0, k1 = 0;
                unhash_key<KW>(klo[j], khi[j], k0, k1);
                uint32_t p0, p1, p2;
                src_carry<CWS>(bp.S, srow, p0, p1, p2);
                uint32_t b = klo[j] & BMASK;
                bool     more;
                do {
                    uint32_t eq = match(b, klo[j], khi[j], more);
                    while (eq) {
                        const uint32_t slot = b * 4 + (uint32_t)__builtin_ctz(eq);
                        eq &= eq - 1;
                        uint32_t b0, b1, b2;
                        src_carry<CWR>(bp.R, t_w[KW][slot], b0, b1, b2);
                        stream_store(bp.key, row, k0, k1);
                        if constexpr (CWR >= 1) stream_store(bp.bc, row, b0, b1, b2);
                        if constexpr (CWS >= 1) stream_store(bp.pc, row, p0, p1, p2);
                        ++row;
                    }
                    b = (b + 1) & BMASK;
                } while (more);
            }
        }
        lds_barrier();  // s_wtot / s_obase are reused by the next chunk
    }
}

// ================================================================== launchers
void launch_join_bcast(const Launch& L, int key_words, int cw_build, int cw_probe,
                       const BcastParams& bp, uint32_t grid) {
    if (!grid) return;
    for_shape2("join_broadcast", key_words, cw_build, cw_probe, [&](auto KW, auto CWR, auto CWS) {
        RJ_KLAUNCH(L, "join_broadcast", (k_join_bcast<KW, CWR, CWS>), grid, JN_THREADS, bp);
    });
}

// RJ_CTX_PREWARM: one harmless launch, so that HIP loads this translation unit's code object when the context is
// built.  A zeroed BcastParams: bp.R.n_rows = 0, so the build loop (`r < bp.R.n_rows`) inserts nothing, and
// bp.S.n_rows = 0, so the probe loop (`base < n`) does not run; what comes before them clears the bucket counters
// in LDS and reads or writes no memory.
void prewarm_bcast(const Launch& L, uint32_t*) {
    RJ_KLAUNCH(L, "prewarm", (k_join_bcast<1, 0, 0>), 1, JN_THREADS, BcastParams{});
}

}  // namespace rj
