// rj_outer.hip — gfx950 (wave64) kernels of the outer joins (RJ_NODE_OUTER).
#include <hip/hip_ext.h>

#include "rj_kernels.hpp"
#include "rj_kernel_util.hpp"
#include "rj_tuple_util.hpp"
#include "rj_outer_util.hpp"

#include <algorithm>
#include <type_traits>

namespace rj {

// ============================================================ outer joins
// RJ_NODE_OUTER: the inner join's rows (duplicates multiply) plus, ONCE, every preserved row that
// has no partner, with NULL in the optional (build) side's columns.  Both halves come out of one
// pass over the preserved tuples and through one output cursor.
// The LDS table is k_join_bcast's: buckets of four slots with an insert counter each (a slot is
// valid when its index is below the counter; a counter above 4 sends the walk on to the next
// bucket), key words + a REFERENCE to the build tuple (its row in the child for k_outer_bcast, its
// index in the partitioned arrays for k_outer_join).  The optional side's carry is fetched through
// the reference on emit: a few KB per table, cache resident.  (KW + 1) * 32 KiB + 8 KiB of LDS:
// 72 KiB (two workgroups per CU) for 32-bit keys, 104 KiB (one) for 64-bit keys.
// The home bucket is the multiplicative hash of the key words: their low radix bits are the same
// for a whole partition, the product's high bits are not.
// A padded row carries "NULL" in-band (rj_device.hpp, OuterParams): the build carry's first word is
// op.pad_bc, the others zero.

// Broadcast form: an optional side of at most JN_RMAX rows.  Every workgroup builds the SAME table
// straight from the optional child's key column (page decode, NULL / NaN drop, hashing on the way)
// and streams a grid-strided slice of the preserved child past it.  A preserved row whose key is
// NULL or NaN has no partner and comes out padded here.  keyless (the key types differ) or an
// empty optional side: no key is read or no tuple inserted, every row comes out padded.
// The body (rj_outer_bcast_body.inc) is shared with k_full_bcast (FULL, compile time): there the workgroup also keeps one
// matched bit per build row in LDS (JN_RMAX bits) and ORs its non-zero words into gflags at the end.
template <int KW, int CWB, int CWP>
__global__ __launch_bounds__(JN_THREADS) void k_outer_bcast(OuterParams op) {
    constexpr bool FULL = false;
    uint32_t* const gflags = nullptr;
#include "rj_outer_bcast_body.inc"
}

// The partitioned path's leftovers: the preserved rows the first radix pass drops (NULL key; FP64
// NaN key) have no partner, so they come out padded.  Grid-strided over the preserved child, the
// same tuple formation (src_key / src_carry over the TupleSrc) and output cursor as the probe.
template <int KW, int CWP>
__global__ __launch_bounds__(JN_THREADS) void k_outer_nullkeys(OuterParams op) {
    __shared__ uint32_t s_wtot[JN_THREADS / 64];
    __shared__ unsigned long long s_obase;
    const OuterTable<KW> T{nullptr, nullptr};  // (nothing is probed)
    const uint32_t       n = op.P.n_rows;
    for (uint64_t base = (uint64_t)blockIdx.x * JN_SUB; base < n; base += (uint64_t)gridDim.x * JN_SUB) {
        uint32_t klo[JN_SPT], khi[JN_SPT];
        bool     probe[JN_SPT], padrow[JN_SPT], hit[JN_SPT];
#pragma unroll
        for (int j = 0; j < JN_SPT; ++j) {
            const uint64_t row = base + (uint64_t)j * JN_THREADS + threadIdx.x;
            klo[j] = khi[j] = 0;
            probe[j] = hit[j] = false;
            padrow[j] = row < n && !src_key<KW>(op.P, (uint32_t)row, klo[j], khi[j]);
        }
        // (the build carry's width is a run-time property of op.bc here: 1 stands for "some")
        outer_emit<false, KW, 1, CWP, JN_SPT>(
            op, T, probe, padrow, hit, klo, khi, s_wtot, &s_obase,
            [&](uint32_t, uint32_t& b0, uint32_t& b1, uint32_t& b2) { b0 = b1 = b2 = 0; },
            [&](int j, uint32_t& p0, uint32_t& p1, uint32_t& p2) {
                src_carry<CWP>(op.P, (uint32_t)(base + (uint64_t)j * JN_THREADS + threadIdx.x), p0, p1, p2);
            });
    }
}

// Partitioned form: one workgroup per co-partition, or per heavy task of a preserved partition
// above JN_HEAVY tuples (k_heavy_tasks; every task sees its partition's whole build side, and a
// partition WITHOUT build tuples stays with its main workgroup, which pads it whole).  The loop
// order is k_filter_join's: a JN_SUB-tuple chunk of preserved tuples stays in registers while the
// partition's build tuples pass by in table rounds of JN_RMAX tuples; every round emits its
// matches, a per-tuple "matched in some round" flag is OR-ed over the rounds, and the LAST round
// also emits the padded rows of the tuples that never matched.  The usual partition needs one
// round, i.e. one reservation per chunk.  No memory outside the registers holds a flag.
// The body (rj_outer_join_body.inc) is shared with k_full_join (FULL, compile time).  There the build tuples that matched
// must be known AFTER the launch, across the heavy tasks of a partition and across table rounds:
// the workgroup collects one bit per build tuple of the current round in LDS (FW words: JN_RMAX
// bits from the 32-aligned index below the round's first tuple) and ORs the non-zero words into
// gflags (one bit per tuple of the partitioned build arrays) before the table is rebuilt and when
// the task ends — a few hundred vector atomics per task, not one per match.
template <int KW, int CWB, int CWP>
__global__ __launch_bounds__(JN_THREADS) void k_outer_join(OuterParams op) {
    constexpr bool FULL = false;
    uint32_t* const gflags = nullptr;
#include "rj_outer_join_body.inc"
}

// ================================================================== launchers
// outer joins: the optional and the preserved side's carries
void launch_outer_bcast(const Launch& L, int key_words, int cw_optional, int cw_preserved, const OuterParams& op,
                        uint32_t grid) {
    if (!grid) return;
    for_shape2("outer_broadcast", key_words, cw_optional, cw_preserved, [&](auto KW, auto CWB, auto CWP) {
        RJ_KLAUNCH(L, "outer_broadcast", (k_outer_bcast<KW, CWB, CWP>), grid, JN_THREADS, op);
    });
}

void launch_outer_join(const Launch& L, int key_words, int cw_optional, int cw_preserved, const OuterParams& op,
                       uint32_t grid) {
    if (!grid) return;
    for_shape2("outer_probe", key_words, cw_optional, cw_preserved, [&](auto KW, auto CWB, auto CWP) {
        RJ_KLAUNCH(L, "outer_probe", (k_outer_join<KW, CWB, CWP>), grid, JN_THREADS, op);
    });
}

void launch_outer_nullkeys(const Launch& L, int key_words, int cw_preserved, const OuterParams& op, uint32_t grid) {
    if (!grid) return;
    for_shape("outer_nullkeys", key_words, cw_preserved, [&](auto KW, auto CW) {
        RJ_KLAUNCH(L, "outer_nullkeys", (k_outer_nullkeys<KW, CW>), grid, JN_THREADS, op);
    });
}

// RJ_CTX_PREWARM: one harmless launch, so that HIP loads this translation unit's code object when the context is
// built.  A zeroed OuterParams: op.P.n_rows = 0, so the row loop of k_outer_nullkeys (`base < n`) does not run; nothing
// before it reads or writes memory.
void prewarm_outer(const Launch& L, uint32_t*) {
    RJ_KLAUNCH(L, "prewarm", (k_outer_nullkeys<1, 0>), 1, JN_THREADS, OuterParams{});
}

}  // namespace rj
