// rj_window.hip — the gfx950 (wave64) kernels of RJ_NODE_WINDOW and their launchers.
#include <algorithm>

#include "rj_group_util.hpp"
#include "rj_kernel_util.hpp"
#include "rj_sortkey.hpp"

namespace rj {

// RJ_NODE_WINDOW: the rows are ordered by (partition keys, order keys) (the sort's kernels), and two
// head masks in k_group_heads' layout say where the partitions (P) and the peer groups (Q, a superset)
// begin.  The unit of work is a QUARTER: the WIN_QUARTER positions one wave of a tile holds, 16 mask
// words.  A wave never talks to another one inside a launch; what crosses quarters goes through memory
// from one launch to the next (geometry and structs: rj_device.hpp).
//   k_win_one_head  the P mask of a node without partition keys: position 0 and nothing else
// Ranks, from the two masks alone:
//   k_win_marks     a quarter's summary: its last P head, its last and first Q head, the Q heads at or
//                   behind its last P head
//   k_win_carry     ONE launch of two workgroups turns the summaries into what a quarter needs from
//                   outside: workgroup 0 scans forward (the last P head and the last Q head in front of the
//                   quarter, the Q heads since that P head), workgroup 1 backward (the first Q head behind it)
//   k_win_ranks     ROW_NUMBER / RANK / DENSE_RANK / COUNT(*) and every position's PEER END, by popcounts
//                   and leading / trailing zero counts on the mask words of the quarter
// Aggregates, one set of launches per distinct value column (a segmented inclusive scan over the
// P segments of the column, gathered through the permutation; reduce, then scan):
//   k_win_tails     a quarter's tail: the accumulators of its positions from its last P head on
//   k_win_tail_carry  ONE workgroup: the tails -> every quarter's carry-in (it resets at a quarter with a head)
//   k_win_scan      the scan of a quarter with its carry-in, stored per position
//   k_win_column    a result column: the scan at every row's peer end (decode, narrow, validity from the count)
// The accumulators are k_group_reduce's: non-NULL count, wrapping sum, unsigned min / max of the
// ENCODED value.  Every word these kernels read was written by an earlier launch of the same node.

__global__ __launch_bounds__(256) void k_win_one_head(unsigned long long* __restrict__ masks, uint64_t n_masks) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n_masks) masks[i] = i == 0 ? 1ull : 0ull;
}

// Thread q: the summary of quarter q.  Positions travel as 1 + position, 0 = none; next_q as the
// position itself, n_rows = none.
__global__ __launch_bounds__(256) void k_win_marks(const unsigned long long* __restrict__ P, const unsigned long long* __restrict__ Q,
                                                   uint32_t n_rows, uint32_t n_quarters, WinMarks m) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= n_quarters) return;
    const uint64_t n_masks = ((uint64_t)n_rows + 63u) / 64u;
    uint32_t       lp = 0, lq = 0, d = 0, fq = n_rows;
    for (uint32_t j = 0; j < (uint32_t)WIN_ITEMS; ++j) {
        const uint64_t idx = (uint64_t)q * WIN_ITEMS + j;
        if (idx >= n_masks) break;
        const uint64_t pw = P[idx], qw = Q[idx];
        const uint32_t base = (uint32_t)(idx * 64u);
        if (qw) {
            if (fq == n_rows) fq = base + (uint32_t)__builtin_ctzll(qw);
            lq = base + (63u - (uint32_t)__builtin_clzll(qw)) + 1u;
        }
        if (pw) {
            const uint32_t hp = 63u - (uint32_t)__builtin_clzll(pw);
            lp = base + hp + 1u;
            d = (uint32_t)__popcll(qw >> hp);
        } else {
            d += (uint32_t)__popcll(qw);
        }
    }
    m.last_p[q] = lp;
    m.last_q[q] = lq;
    m.dense[q] = d;
    m.next_q[q] = fq;
}

struct WinMark {
    uint32_t lp, lq, d;
};
struct WinTail {
    uint32_t head, nn;
    uint64_t sum, mn, mx;
};
__device__ __forceinline__ uint32_t win_shfl_up(uint32_t a, int off) { return __shfl_up(a, off); }
__device__ __forceinline__ WinMark  win_shfl_up(const WinMark& a, int off) {
    return WinMark{__shfl_up(a.lp, off), __shfl_up(a.lq, off), __shfl_up(a.d, off)};
}
__device__ __forceinline__ WinTail win_shfl_up(const WinTail& a, int off) {
    return WinTail{__shfl_up(a.head, off), __shfl_up(a.nn, off), __shfl_up(a.sum, off), __shfl_up(a.mn, off), __shfl_up(a.mx, off)};
}

// Exclusive scan of one value per thread over the WIN_CARRY_THREADS threads of a workgroup: a wave scan by
// shuffles, the waves' totals through LDS (`s`: one entry per wave).  op(a, b): a in front of b.
// -> what is in front of the thread; total: all threads.  Two barriers.
template <typename T, typename Op>
__device__ __forceinline__ T win_block_exclusive(T v, T ident, Op op, T* s, T& total) {
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T t = win_shfl_up(v, off);
        if (lane >= (uint32_t)off) v = op(t, v);
    }
    __syncthreads();  // s is free again
    if (lane == 63u) s[wid] = v;
    __syncthreads();
    T before = ident;
    total = ident;
    for (uint32_t k = 0; k < (uint32_t)WIN_CARRY_THREADS / 64u; ++k) {
        const T w = s[k];
        if (k < wid) before = op(before, w);
        total = op(total, w);
    }
    T ex = win_shfl_up(v, 1);
    if (lane == 0) ex = ident;
    return op(before, ex);
}

// In place: entry k -> the combination of the entries in front of it.  The workgroup takes `chunk`
// consecutive entries per step, one per thread (coalesced), scans them and carries the total of the
// steps so far in every thread.  (A backward scan mirrors the index in `load` and `store`.)
template <typename T, typename Op, typename Load, typename Store>
__device__ __forceinline__ void win_chunk_scan(uint32_t n, uint32_t chunk, T ident, Op op, Load load, Store store, T* s) {
    T running = ident;
    for (uint64_t k0 = 0; k0 < n; k0 += chunk) {  // (uniform: every thread meets every barrier)
        const uint64_t k = k0 + threadIdx.x;
        const bool     mine = threadIdx.x < chunk && k < n;
        T              total;
        const T        before = win_block_exclusive(mine ? load((uint32_t)k) : ident, ident, op, s, total);
        if (mine) store((uint32_t)k, op(running, before));
        running = op(running, total);
    }
}

// chunk = entries per step (at most WIN_CARRY_THREADS)
__global__ __launch_bounds__(WIN_CARRY_THREADS) void k_win_carry(WinMarks m, uint32_t n_quarters, uint32_t chunk, uint32_t n_rows) {
    __shared__ WinMark  s_f[WIN_CARRY_THREADS / 64];
    __shared__ uint32_t s_b[WIN_CARRY_THREADS / 64];
    if (blockIdx.x == 0) {
        auto op = [](const WinMark& a, const WinMark& b) {
            return WinMark{b.lp ? b.lp : a.lp, b.lq ? b.lq : a.lq, b.lp ? b.d : a.d + b.d};
        };
        win_chunk_scan(
            n_quarters, chunk, WinMark{0u, 0u, 0u}, op, [&](uint32_t k) { return WinMark{m.last_p[k], m.last_q[k], m.dense[k]}; },
            [&](uint32_t k, const WinMark& c) {
                m.last_p[k] = c.lp;
                m.last_q[k] = c.lq;
                m.dense[k] = c.d;
            },
            s_f);
    } else {
        auto op = [](uint32_t a, uint32_t b) { return b < a ? b : a; };
        win_chunk_scan(
            n_quarters, chunk, n_rows, op, [&](uint32_t k) { return m.next_q[n_quarters - 1u - k]; },
            [&](uint32_t k, uint32_t c) { m.next_q[n_quarters - 1u - k] = c; }, s_b);
    }
}

// Wave w of workgroup b: quarter 4 b + w.  Lane j < WIN_ITEMS keeps the masks of item j; the items are
// walked twice, backward for the first Q head behind every item, forward for everything else, with
// wave-uniform running values.  Each output is optional.
__global__ __launch_bounds__(GROUP_THREADS) void k_win_ranks(const unsigned long long* __restrict__ P,
                                                             const unsigned long long* __restrict__ Q, uint32_t n_rows,
                                                             uint32_t n_quarters, WinMarks m, WinRanks out) {
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    const uint32_t q = blockIdx.x * GROUP_WAVES + wid;
    if (q >= n_quarters) return;
    const uint64_t n_masks = ((uint64_t)n_rows + 63u) / 64u;
    const uint64_t midx = (uint64_t)q * WIN_ITEMS + lane;
    uint64_t       pm = 0, qm = 0;
    if (lane < (uint32_t)WIN_ITEMS && midx < n_masks) pm = P[midx], qm = Q[midx];
    const uint64_t qbase = (uint64_t)q * WIN_QUARTER;
    uint32_t       prev_p = m.last_p[q], prev_q = m.last_q[q], dense_run = m.dense[q], run = m.next_q[q];
    uint32_t       my_next = run;  // lane j: the first Q head behind item j
    for (int j = WIN_ITEMS - 1; j >= 0; --j) {
        const uint64_t qw = group_uniform(__shfl(qm, j));
        if (lane == (uint32_t)j) my_next = run;
        if (qw) run = (uint32_t)(qbase + 64u * (uint32_t)j) + (uint32_t)__builtin_ctzll(qw);
    }
    for (uint32_t j = 0; j < (uint32_t)WIN_ITEMS; ++j) {
        const uint64_t base = qbase + 64u * j;
        if (base >= n_rows) break;  // (the whole wave, and every later item of it)
        const uint64_t pw = group_uniform(__shfl(pm, (int)j)), qw = group_uniform(__shfl(qm, (int)j));
        const uint32_t nx = __builtin_amdgcn_readfirstlane(__shfl(my_next, (int)j));
        const uint64_t le = (2ull << lane) - 1ull;  // positions [0, lane] of the item (lane 63: all)
        const uint64_t mp = pw & le, mq = qw & le, gt = qw & ~le;
        const uint32_t b32 = (uint32_t)base;
        uint32_t       pstart1 = prev_p, qstart1 = prev_q, dense = dense_run + (uint32_t)__popcll(mq);
        if (mp) {
            const uint32_t hp = 63u - (uint32_t)__builtin_clzll(mp);
            pstart1 = b32 + hp + 1u;
            dense = (uint32_t)__popcll(mq >> hp);
        }
        if (mq) qstart1 = b32 + (63u - (uint32_t)__builtin_clzll(mq)) + 1u;
        const uint32_t qend = gt ? b32 + (uint32_t)__builtin_ctzll(gt) : nx;  // the position behind my last peer
        const uint64_t i = base + lane;
        if (i < n_rows) {
            const uint32_t pstart = pstart1 - 1u;
            if (out.row_number) out.row_number[i] = (unsigned long long)((uint32_t)i - pstart) + 1ull;
            if (out.rank) out.rank[i] = (unsigned long long)(qstart1 - pstart1) + 1ull;
            if (out.dense_rank) out.dense_rank[i] = (unsigned long long)dense;
            if (out.count_star) out.count_star[i] = (unsigned long long)(qend - pstart);
            if (out.peer_end) out.peer_end[i] = qend - 1u;
        }
        if (pw) {
            const uint32_t hp = 63u - (uint32_t)__builtin_clzll(pw);
            prev_p = b32 + hp + 1u;
            dense_run = (uint32_t)__popcll(qw >> hp);
        } else {
            dense_run += (uint32_t)__popcll(qw);
        }
        if (qw) prev_q = b32 + (63u - (uint32_t)__builtin_clzll(qw)) + 1u;
    }
}

// position i of the order as a one-row accumulator (the identity for a NULL and behind the last row)
template <int W>
__device__ __forceinline__ GroupPart<W> win_value(const ColRef& col, const uint32_t* __restrict__ perm, uint64_t i, uint32_t n_rows,
                                                  int32_t f64) {
    GroupPart<W> x = group_identity<W>();
    if (i < n_rows) {
        const uint32_t r = perm ? perm[i] : (uint32_t)i;
        if (!(col.valid && !col.valid[r])) {
            const uint64_t bits = group_load<W>(col, r);
            x.nn = 1;
            x.sum = W == 4 ? (uint64_t)(int64_t)(int32_t)(uint32_t)bits : bits;
            x.mn = x.mx = sort_key_bits(bits, W, f64 != 0, false);
        }
    }
    return x;
}

constexpr int WIN_BATCH = 4;  // items whose loads are in flight together
static_assert(WIN_ITEMS % WIN_BATCH == 0, "whole batches");

// Wave w of workgroup b: the tail of quarter 4 b + w.  Only the items from the one with the quarter's last
// P head on are read: a quarter of short partitions costs one item.
template <int W>
__global__ __launch_bounds__(GROUP_THREADS) void k_win_tails(ColRef col, const uint32_t* __restrict__ perm, uint32_t n_rows, int32_t f64,
                                                             const unsigned long long* __restrict__ P, uint32_t n_quarters, WinTails t) {
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    const uint32_t q = blockIdx.x * GROUP_WAVES + wid;
    if (q >= n_quarters) return;
    const uint64_t n_masks = ((uint64_t)n_rows + 63u) / 64u;
    const uint64_t midx = (uint64_t)q * WIN_ITEMS + lane;
    uint64_t       pm = 0;
    if (lane < (uint32_t)WIN_ITEMS && midx < n_masks) pm = P[midx];
    const uint64_t with_head = __ballot(pm != 0);
    uint32_t       j_first = 0, l_first = 0;  // the tail begins at lane l_first of item j_first
    if (with_head) {
        j_first = 63u - (uint32_t)__builtin_clzll(with_head);
        l_first = 63u - (uint32_t)__builtin_clzll(group_uniform(__shfl(pm, (int)j_first)));
    }
    const uint64_t qbase = (uint64_t)q * WIN_QUARTER;
    GroupPart<W>   mine = group_identity<W>();
    for (uint32_t j0 = j_first & ~(uint32_t)(WIN_BATCH - 1); j0 < (uint32_t)WIN_ITEMS; j0 += WIN_BATCH) {
        if (qbase + 64u * j0 >= n_rows) break;
        GroupPart<W> x[WIN_BATCH];
#pragma unroll
        for (int k = 0; k < WIN_BATCH; ++k) {
            const uint32_t j = j0 + (uint32_t)k;
            const bool     in_tail = j > j_first || (j == j_first && lane >= l_first);
            x[k] = group_identity<W>();
            if (in_tail) x[k] = win_value<W>(col, perm, qbase + 64u * j + lane, n_rows, f64);
        }
#pragma unroll
        for (int k = 0; k < WIN_BATCH; ++k) group_add(mine, x[k]);
    }
    const GroupPart<W> tot = group_wave_total(mine);
    if (lane == 0) {
        t.head[q] = with_head ? 1u : 0u;
        t.nn[q] = tot.nn;
        t.sum[q] = tot.sum;
        t.mn[q] = tot.mn;
        t.mx[q] = tot.mx;
    }
}

__global__ __launch_bounds__(WIN_CARRY_THREADS) void k_win_tail_carry(WinTails t, uint32_t n_quarters, uint32_t chunk) {
    __shared__ WinTail s[WIN_CARRY_THREADS / 64];
    auto op = [](const WinTail& a, const WinTail& b) {
        if (b.head) return b;
        return WinTail{a.head, a.nn + b.nn, a.sum + b.sum, b.mn < a.mn ? b.mn : a.mn, b.mx > a.mx ? b.mx : a.mx};
    };
    win_chunk_scan(
        n_quarters, chunk, WinTail{0u, 0u, 0ull, ~0ull, 0ull}, op,
        [&](uint32_t k) { return WinTail{t.head[k], t.nn[k], t.sum[k], t.mn[k], t.mx[k]}; },
        [&](uint32_t k, const WinTail& c) {
            t.head[k] = c.head;
            t.nn[k] = c.nn;
            t.sum[k] = c.sum;
            t.mn[k] = c.mn;
            t.mx[k] = c.mx;
        },
        s);
}

// Wave w of workgroup b: the segmented inclusive scan of quarter 4 b + w, item by item: a segmented wave
// scan under the item's P mask, the wave's running value added in front of the item's first head.
// Each output array is optional.
template <int W>
__global__ __launch_bounds__(GROUP_THREADS) void k_win_scan(ColRef col, const uint32_t* __restrict__ perm, uint32_t n_rows, int32_t f64,
                                                            const unsigned long long* __restrict__ P, uint32_t n_quarters, WinTails carry,
                                                            WinScan out) {
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    const uint32_t q = blockIdx.x * GROUP_WAVES + wid;
    if (q >= n_quarters) return;
    const uint64_t n_masks = ((uint64_t)n_rows + 63u) / 64u;
    const uint64_t midx = (uint64_t)q * WIN_ITEMS + lane;
    uint64_t       pm = 0;
    if (lane < (uint32_t)WIN_ITEMS && midx < n_masks) pm = P[midx];
    const uint64_t qbase = (uint64_t)q * WIN_QUARTER;
    GroupPart<W>   open = group_identity<W>();  // every lane: the scan at the position in front of the item
    open.nn = carry.nn[q], open.sum = carry.sum[q], open.mn = carry.mn[q], open.mx = carry.mx[q];
    for (uint32_t j0 = 0; j0 < (uint32_t)WIN_ITEMS; j0 += WIN_BATCH) {
        if (qbase + 64u * j0 >= n_rows) break;  // (the whole wave, and every later item of it)
        GroupPart<W> x[WIN_BATCH];
#pragma unroll
        for (int k = 0; k < WIN_BATCH; ++k) x[k] = win_value<W>(col, perm, qbase + 64u * (j0 + (uint32_t)k) + lane, n_rows, f64);
#pragma unroll
        for (int k = 0; k < WIN_BATCH; ++k) {
            const uint64_t pw = group_uniform(__shfl(pm, (int)(j0 + (uint32_t)k)));
            GroupPart<W> s = group_segmented_scan(x[k], pw, lane);
            if ((pw & ((2ull << lane) - 1ull)) == 0) group_add(s, open);  // no head in [0, lane]
            const uint64_t i = qbase + 64u * (j0 + (uint32_t)k) + lane;
            if (i < n_rows) {
                if (out.nn) out.nn[i] = s.nn;
                if (out.sum) out.sum[i] = s.sum;
                if (out.mn) out.mn[i] = s.mn;
                if (out.mx) out.mx[i] = s.mx;
            }
            open = group_shfl(s, 63);
        }
    }
}

// src[e] (or the count nn[e] where src == nullptr) at e = peer_end[i] as row i of a result column:
// decoded (GroupDecode), narrowed to `width` bytes, 0 where the frame has no non-NULL value; validity
// bytes nn[e] != 0 (dst_valid optional).
__global__ __launch_bounds__(256) void k_win_column(const unsigned long long* __restrict__ src, const uint32_t* __restrict__ nn,
                                                    const uint32_t* __restrict__ peer_end, uint64_t n, int32_t decode, int32_t width,
                                                    uint8_t* __restrict__ dst, uint8_t* __restrict__ dst_valid) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint64_t       e = peer_end[i];
    if (e >= n) e = n - 1u;
    const bool     valid = dst_valid ? nn[e] != 0 : true;
    uint64_t       v = src ? src[e] : (uint64_t)nn[e];
    if (decode != GROUP_RAW) v = sort_key_value(v, decode == GROUP_KEY32 ? 4 : 8, decode == GROUP_KEYF64, false);
    if (!valid) v = 0;
    if (width == 4)
        reinterpret_cast<uint32_t*>(dst)[i] = (uint32_t)v;
    else
        reinterpret_cast<uint64_t*>(dst)[i] = v;
    if (dst_valid) dst_valid[i] = valid ? 1 : 0;
}

// ================================================================== launchers
static uint32_t win_quarters(uint32_t n_rows) { return n_rows / WIN_QUARTER + (n_rows % WIN_QUARTER != 0); }
// entries per step of a carry kernel: max_chunk (0: all its threads) caps them
static uint32_t win_chunk(uint32_t max_chunk) {
    return max_chunk ? std::min<uint32_t>(max_chunk, WIN_CARRY_THREADS) : (uint32_t)WIN_CARRY_THREADS;
}

void launch_win_one_head(const Launch& L, unsigned long long* masks, uint32_t n_rows) {
    if (!n_rows) return;
    const uint64_t n_masks = ((uint64_t)n_rows + 63u) / 64u;
    RJ_KLAUNCH(L, "win_one_head", k_win_one_head, (uint32_t)((n_masks + 255u) / 256u), 256, masks, n_masks);
}

void launch_win_ranks(const Launch& L, const unsigned long long* P, const unsigned long long* Q, uint32_t n_rows, const WinMarks& m,
                      const WinRanks& out, uint32_t max_chunk) {
    if (!n_rows) return;
    const uint32_t nq = win_quarters(n_rows);
    RJ_KLAUNCH(L, "win_marks", k_win_marks, (nq + 255u) / 256u, 256, P, Q, n_rows, nq, m);
    RJ_KLAUNCH(L, "win_carry", k_win_carry, 2, WIN_CARRY_THREADS, m, nq, win_chunk(max_chunk), n_rows);
    RJ_KLAUNCH(L, "win_ranks", k_win_ranks, (nq + GROUP_WAVES - 1u) / GROUP_WAVES, GROUP_THREADS, P, Q, n_rows, nq, m, out);
}

void launch_win_scan(const Launch& L, const ColRef& col, const uint32_t* perm, uint32_t n_rows, bool f64, const unsigned long long* P,
                     const WinTails& tails, const WinScan& out, uint32_t max_chunk) {
    if (!n_rows) return;
    const uint32_t nq = win_quarters(n_rows), grid = (nq + GROUP_WAVES - 1u) / GROUP_WAVES;
    if (col.width == 4)
        RJ_KLAUNCH(L, "win_tails", (k_win_tails<4>), grid, GROUP_THREADS, col, perm, n_rows, (int32_t)f64, P, nq, tails);
    else
        RJ_KLAUNCH(L, "win_tails", (k_win_tails<8>), grid, GROUP_THREADS, col, perm, n_rows, (int32_t)f64, P, nq, tails);
    RJ_KLAUNCH(L, "win_tail_carry", k_win_tail_carry, 1, WIN_CARRY_THREADS, tails, nq, win_chunk(max_chunk));
    if (col.width == 4)
        RJ_KLAUNCH(L, "win_scan", (k_win_scan<4>), grid, GROUP_THREADS, col, perm, n_rows, (int32_t)f64, P, nq, tails, out);
    else
        RJ_KLAUNCH(L, "win_scan", (k_win_scan<8>), grid, GROUP_THREADS, col, perm, n_rows, (int32_t)f64, P, nq, tails, out);
}

void launch_win_column(const Launch& L, const unsigned long long* src, const uint32_t* nn, const uint32_t* peer_end, uint64_t n, int decode,
                       int width, uint8_t* dst, uint8_t* dst_valid) {
    if (!n) return;
    RJ_KLAUNCH(L, "win_column", k_win_column, (uint32_t)((n + 255) / 256), 256, src, nn, peer_end, n, (int32_t)decode, (int32_t)width, dst,
               dst_valid);
}

}  // namespace rj
