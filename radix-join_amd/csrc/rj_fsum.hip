// rj_fsum.hip — the gfx950 (wave64) kernels of RJ_AGG_FSUM, the exactly rounded FP64 sum of
// RJ_NODE_GROUP, and their launcher.  The arithmetic is rj_fsum.hpp's, shared with the host.
#include <algorithm>

#include "rj_fsum.hpp"
#include "rj_group_util.hpp"
#include "rj_kernel_util.hpp"

namespace rj {

// The grid, the tiles, the runs of tiles and the head masks are k_group_reduce's (rj_group.hip); what
// differs is the state.  An accumulator is FSUM_WORDS 64-bit words (rj_fsum.hpp), too long for
// registers and shuffles, so it lives in LDS:
//   k_fsum_slots   the group that is open at the end of a run of tiles is the one a run may share with
//                  its neighbours (the group that comes into a run is the one open at the end of the
//                  run before it) -> one arena slot per distinct such group: a scan over n_runs
//                  entries in one workgroup
//   k_fsum_zero    the arena's words = 0: nothing relies on what the memory held
//   k_fsum_reduce  every wave keeps the accumulator of its open group in LDS.  A lane adds the three
//                  pieces of its value with non-returning 64-bit LDS atomics; an item with heads is
//                  walked segment by segment (a wave-uniform loop).  A group that begins and ends
//                  inside the wave's quarter of the tile is rounded and stored when its segment ends.
//                  The wave's first segment and its open one meet the other waves' in LDS, where wave
//                  0 strings them together with the accumulator the workgroup carries from tile to
//                  tile.  A group the workgroup closes and owns alone is rounded and stored; the first
//                  group it closes and the one open at the end of its run are added to their arena
//                  slots, propagated, with 64-bit global atomics on the chunks that are not 0.
//   k_fsum_finish  every slot rounded into out[its group]
// Every group has one writer, no workgroup waits for another, and every sum is exact until it is
// rounded once, so the result does not depend on the grid, the order or the timing.
// The count that decides NULL is k_group_reduce's `nn` over the same column (rj_exec.hip).
//
// A wave works on an accumulator with lane l on chunk l, lanes 0 .. 7 also on word 64 + l.

using ull = unsigned long long;

// the wave's LDS writes are visible to its own later reads (LDS serves a wave's requests in order;
// this keeps the compiler from moving them)
__device__ __forceinline__ void fsum_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ void fsum_wave_zero(fsum_t* a, uint32_t lane) {
    a[lane] = 0;
    if (lane < (uint32_t)(FSUM_WORDS - 64)) a[64u + lane] = 0;
}
__device__ __forceinline__ void fsum_wave_copy(fsum_t* dst, const fsum_t* src, uint32_t lane) {
    dst[lane] = src[lane];
    if (lane < (uint32_t)(FSUM_WORDS - 64)) dst[64u + lane] = src[64u + lane];
}
__device__ __forceinline__ void fsum_wave_merge(fsum_t* dst, const fsum_t* src, uint32_t lane) {
    fsum_merge_word(dst, src, (int)lane);
    if (lane < (uint32_t)(FSUM_WORDS - 64)) fsum_merge_word(dst, src, (int)(64u + lane));
}
// the chunks that are not 0: [lo, hi], lo = hi = 0 if there is none
__device__ __forceinline__ void fsum_wave_range(const fsum_t* a, uint32_t lane, int& lo, int& hi) {
    const uint64_t m0 = __ballot(a[lane] != 0);
    const uint64_t m1 = __ballot(lane < (uint32_t)(FSUM_CHUNKS - 64) && a[64u + lane] != 0);
    lo = m0 ? __builtin_ctzll(m0) : (m1 ? 64 + __builtin_ctzll(m1) : 0);
    hi = m1 ? 64 + 63 - __builtin_clzll(m1) : (m0 ? 63 - __builtin_clzll(m0) : 0);
}
// One step of carry propagation, every chunk at once: each keeps its low 32 bits and hands the rest to
// the next one; chunk 67 keeps everything.  Afterwards every chunk below 67 is within (-2^31, 2^32 + 2^31).
__device__ __forceinline__ void fsum_wave_carry_step(fsum_t* a, uint32_t lane) {
    const fsum_t   va = a[lane], vb = lane < 4u ? a[64u + lane] : 0;
    const fsum_t   ha = va >> 32, hb = lane < 3u ? vb >> 32 : 0;
    const fsum_t   la = va & (fsum_t)FSUM_M32, lb = lane < 3u ? vb & (fsum_t)FSUM_M32 : vb;
    const fsum_t   up_a = __shfl_up(ha, 1), up_b = __shfl_up(hb, 1), top_a = __shfl(ha, 63);
    a[lane] = la + (lane ? up_a : 0);
    if (lane < 4u) a[64u + lane] = lb + (lane ? up_b : top_a);
}
// The accumulator's value as a double (lane 0 has it; `flags` is wave-uniform), and the accumulator 0 again.
__device__ __forceinline__ uint64_t fsum_wave_result(fsum_t* a, uint32_t flags, uint32_t lane) {
    int lo, hi;
    fsum_wave_sync();
    fsum_wave_range(a, lane, lo, hi);
    uint64_t bits = 0;
    if (lane == 0) {
        fsum_propagate(a, lo, hi);
        const bool neg = fsum_magnitude(a, lo, hi);
        bits = fsum_round(a, lo, hi, neg, flags);
    }
    fsum_wave_sync();
    if ((int)lane >= lo && (int)lane <= hi) a[lane] = 0;
    if (lane < 4u && (int)(64u + lane) >= lo && (int)(64u + lane) <= hi) a[64u + lane] = 0;
    fsum_wave_sync();
    return bits;
}
// The accumulator, propagated, added to an arena slot: the chunks that are not 0, and the flags.
__device__ __forceinline__ void fsum_wave_to_slot(fsum_t* a, uint32_t flags, ull* slot, uint32_t lane) {
    int lo, hi;
    fsum_wave_sync();
    fsum_wave_range(a, lane, lo, hi);
    if (lane == 0) fsum_propagate(a, lo, hi);
    fsum_wave_sync();
    const fsum_t va = a[lane], vb = lane < 4u ? a[64u + lane] : 0;
    if (va) atomicAdd(&slot[lane], (ull)va);
    if (vb) atomicAdd(&slot[64u + lane], (ull)vb);
    if (lane == 0 && flags) atomicOr(&slot[FSUM_FLAGS], (ull)flags);
}

// the lanes [s, e) of an item add their values to the wave's accumulator; the non-finite ones' flags
__device__ __forceinline__ uint32_t fsum_wave_add(fsum_t* a, uint64_t bits, bool has, uint32_t lane, uint32_t s, uint32_t e) {
    FsumPieces x{-1, 0u, {0, 0, 0}};
    if (has && lane >= s && lane < e) x = fsum_split(bits);
    fsum_add(x, [&](int k, fsum_t d) { atomicAdd(reinterpret_cast<ull*>(a) + k, (ull)d); });
    uint32_t flags = 0;
    if (__ballot(x.flag != 0u)) {
        if (__ballot((x.flag & FSUM_PINF) != 0u)) flags |= FSUM_PINF;
        if (__ballot((x.flag & FSUM_NINF) != 0u)) flags |= FSUM_NINF;
        if (__ballot((x.flag & FSUM_NAN) != 0u)) flags |= FSUM_NAN;
    }
    return flags;
}

// The run of tiles of workgroup b is [b * tiles_per_wg, (b + 1) * tiles_per_wg).  Entry b: the group that
// is open at its end; the entries do not decrease.  slot_of[b] = distinct groups in front of entry b,
// slot_gid[slot] = its group, *n_slots = the slots.  A group is in a slot exactly when it is open at
// the end of a run: run b adds what it holds of it at its end, and the runs behind it add the rows in
// front of their first head.  Every other group begins at a head of the run that closes it.
// masks == nullptr: the scalar aggregate, group 0 everywhere.  One workgroup.
__global__ __launch_bounds__(1024) void k_fsum_slots(const ull* __restrict__ masks, const uint32_t* __restrict__ tile_base, uint32_t n_tiles,
                                                     uint32_t tiles_per_wg, uint32_t n_runs, uint32_t n_groups,
                                                     uint32_t* __restrict__ slot_of, uint32_t* __restrict__ slot_gid,
                                                     uint32_t* __restrict__ n_slots) {
    __shared__ uint32_t s_wsum[16];
    auto                entry = [&](uint32_t i) -> uint32_t {
        if (!masks) return 0u;
        const uint64_t t1 = ((uint64_t)i + 1u) * tiles_per_wg;
        return t1 < n_tiles ? tile_base[t1] - 1u : n_groups - 1u;
    };
    uint32_t running = 0;
    for (uint32_t i0 = 0; i0 < n_runs; i0 += 1024u) {  // (n_runs <= n_tiles <= 2^20)
        const uint32_t i = i0 + threadIdx.x;
        uint32_t       g = 0, fresh = 0;
        if (i < n_runs) {
            g = entry(i);
            fresh = i == 0 || entry(i - 1u) != g ? 1u : 0u;
        }
        uint32_t tot;
        lds_barrier();  // s_wsum is free again
        const uint32_t pre = block_excl_scan(fresh, s_wsum, tot);
        if (i < n_runs) {
            const uint32_t slot = running + pre + fresh - 1u;
            slot_of[i] = slot;
            if (fresh) slot_gid[slot] = g;
        }
        running += tot;
    }
    if (threadIdx.x == 0) *n_slots = running;
}

__global__ __launch_bounds__(256) void k_fsum_zero(ull* __restrict__ arena, uint64_t n_words) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n_words) arena[i] = 0ull;
}

constexpr int FSUM_BATCH = 4;  // items whose loads are in flight together
static_assert(GROUP_ITEMS % FSUM_BATCH == 0, "whole batches");
// Headroom (rj_fsum.hpp): a wave's accumulator takes the values of its quarter of ONE tile in the keyed
// variant; in the scalar one it takes a carry step after every tile.  The workgroup's accumulator takes
// four wave accumulators per tile (each below 2^10 * 2^32 per chunk) and a carry step after every tile.
// An arena slot takes at most two propagated accumulators per run, of which there are at most 2^20.
static_assert((uint64_t)GROUP_TILE * 4u < FSUM_MAX_ADDS && (2ull << 20) < FSUM_MAX_ADDS, "headroom");

template <bool KEYED>
__global__ __launch_bounds__(GROUP_THREADS) void k_fsum_reduce(ColRef col, const uint32_t* __restrict__ perm, uint32_t n_rows,
                                                               const ull* __restrict__ masks, const uint32_t* __restrict__ tile_base,
                                                               uint32_t n_tiles, uint32_t tiles_per_wg, uint32_t n_groups,
                                                               const uint32_t* __restrict__ slot_of, ull* __restrict__ arena,
                                                               ull* __restrict__ out) {
    __shared__ fsum_t   s_acc[GROUP_WAVES][FSUM_WORDS], s_first[GROUP_WAVES][FSUM_WORDS], s_carry[FSUM_WORDS];
    __shared__ uint32_t s_w[GROUP_WAVES], s_has_head[GROUP_WAVES], s_gid_first[GROUP_WAVES], s_gid_open[GROUP_WAVES];
    __shared__ uint32_t s_rows_first[GROUP_WAVES], s_rows_open[GROUP_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    const uint64_t n_masks = ((uint64_t)n_rows + 63u) / 64u;
    const uint64_t t_begin = (uint64_t)blockIdx.x * tiles_per_wg, t_end = min(t_begin + (uint64_t)tiles_per_wg, (uint64_t)n_tiles);
    fsum_t* const  acc = s_acc[wid];
    // the group that comes into the run is the one open at the end of the run before it (run 0 begins with a head)
    ull* const     slot_first = arena + (uint64_t)slot_of[blockIdx.x ? blockIdx.x - 1u : 0u] * FSUM_WORDS;
    ull* const     slot_last = arena + (uint64_t)slot_of[blockIdx.x] * FSUM_WORDS;
    fsum_wave_zero(acc, lane);
    if (wid == 0) fsum_wave_zero(s_carry, lane);
    fsum_wave_sync();

    if constexpr (!KEYED) {
        uint32_t flags = 0;
        for (uint64_t tile = t_begin; tile < t_end; ++tile) {
            const uint64_t wave_base = tile * GROUP_TILE + (uint64_t)wid * (GROUP_TILE / GROUP_WAVES);
            for (uint32_t j0 = 0; j0 < (uint32_t)GROUP_ITEMS; j0 += FSUM_BATCH) {
                if (wave_base + 64u * j0 >= n_rows) break;  // (the whole wave, and every later item of it)
                uint64_t bits[FSUM_BATCH];
                bool     has[FSUM_BATCH];
#pragma unroll
                for (int k = 0; k < FSUM_BATCH; ++k) {
                    const uint64_t i = wave_base + 64u * (j0 + k) + lane;
                    bits[k] = 0;
                    has[k] = i < n_rows && !(col.valid && !col.valid[i]);
                    if (has[k]) bits[k] = col_load64(col, (uint32_t)i);
                }
#pragma unroll
                for (int k = 0; k < FSUM_BATCH; ++k) flags |= fsum_wave_add(acc, bits[k], has[k], lane, 0u, 64u);
            }
            fsum_wave_sync();
            fsum_wave_carry_step(acc, lane);
            fsum_wave_sync();
        }
        if (lane == 0) acc[FSUM_FLAGS] = (fsum_t)flags;
        __syncthreads();
        if (wid == 0) {
            for (int w = 1; w < GROUP_WAVES; ++w) fsum_wave_merge(acc, s_acc[w], lane);
            fsum_wave_sync();
            const uint32_t all = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)acc[FSUM_FLAGS]);
            fsum_wave_to_slot(acc, all, slot_last, lane);
        }
        return;
    }

    // wave 0: the group that is open across waves and tiles, its chunks in s_carry
    uint64_t c_rows = 0;
    uint32_t c_flags = 0, c_gid = 0;
    bool     c_shared = true;  // the next group to close came into the run: it goes to its slot
    for (uint64_t tile = t_begin; tile < t_end; ++tile) {
        const uint64_t wave_base = tile * GROUP_TILE + (uint64_t)wid * (GROUP_TILE / GROUP_WAVES);
        uint64_t       mask;
        uint32_t       before;
        group_wave_heads(masks, n_masks, (uint32_t)tile, wid, lane, s_w, mask, before);
        before += tile_base[tile];
        uint32_t       g_before = __builtin_amdgcn_readfirstlane(before);  // heads in front of the wave's next segment
        const uint32_t gid_first = g_before - 1u;                          // the group the wave's first segment belongs to
        bool           seen_head = false;
        uint32_t       o_flags = 0, o_rows = 0, first_rows = 0;            // of the open group
        for (uint32_t j0 = 0; j0 < (uint32_t)GROUP_ITEMS; j0 += FSUM_BATCH) {
            if (wave_base + 64u * j0 >= n_rows) break;  // (the whole wave, and every later item of it)
            uint64_t bits[FSUM_BATCH];
            bool     row[FSUM_BATCH], has[FSUM_BATCH];
#pragma unroll
            for (int k = 0; k < FSUM_BATCH; ++k) {
                const uint64_t i = wave_base + 64u * (j0 + k) + lane;
                bits[k] = 0;
                row[k] = i < n_rows;
                has[k] = false;
                if (row[k]) {
                    const uint32_t r = perm ? perm[i] : (uint32_t)i;
                    has[k] = !(col.valid && !col.valid[r]);
                    if (has[k]) bits[k] = col_load64(col, r);
                }
            }
#pragma unroll
            for (int k = 0; k < FSUM_BATCH; ++k) {
                uint64_t       m = group_uniform(__shfl(mask, (int)(j0 + k)));
                const uint64_t rows_m = __ballot(row[k]);
                uint32_t       s = 0;
                for (;;) {  // the segments [s, e) of the item: e = the next head, or the item's end
                    const uint32_t e = m ? (uint32_t)__builtin_ctzll(m) : 64u;
                    if (e > s) {
                        o_flags |= fsum_wave_add(acc, bits[k], has[k], lane, s, e);
                        const uint64_t seg = (e == 64u ? ~0ull : (1ull << e) - 1ull) & ~((1ull << s) - 1ull);
                        o_rows += (uint32_t)__popcll(rows_m & seg);
                    }
                    if (e == 64u) break;
                    // a head at lane e: the open group is complete
                    if (!seen_head) {  // it came from before the wave: wave 0 strings it together
                        fsum_wave_sync();
                        fsum_wave_copy(s_first[wid], acc, lane);
                        fsum_wave_sync();
                        if (lane == 0) s_first[wid][FSUM_FLAGS] = (fsum_t)o_flags;
                        fsum_wave_zero(acc, lane);
                        fsum_wave_sync();
                        first_rows = o_rows;
                        seen_head = true;
                    } else {  // it began at a head of this wave: nobody else knows it
                        const uint64_t v = fsum_wave_result(acc, o_flags, lane);
                        if (lane == 0 && g_before - 1u < n_groups) out[g_before - 1u] = v;
                    }
                    g_before += 1u;
                    o_flags = 0, o_rows = 0;
                    m &= m - 1ull;
                    s = e;
                }
            }
        }
        fsum_wave_sync();
        if (lane == 0) {
            acc[FSUM_FLAGS] = (fsum_t)o_flags;
            s_has_head[wid] = seen_head ? 1u : 0u;
            s_gid_first[wid] = gid_first;
            s_gid_open[wid] = g_before - 1u;
            s_rows_first[wid] = first_rows;
            s_rows_open[wid] = o_rows;
        }
        __syncthreads();
        if (wid == 0) {
            for (int w = 0; w < GROUP_WAVES; ++w) {
                const bool    has_head = __builtin_amdgcn_readfirstlane(s_has_head[w]) != 0u;
                const fsum_t* src = has_head ? s_first[w] : s_acc[w];
                fsum_wave_merge(s_carry, src, lane);
                fsum_wave_sync();
                c_flags |= (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)src[FSUM_FLAGS]);
                c_rows += __builtin_amdgcn_readfirstlane(has_head ? s_rows_first[w] : s_rows_open[w]);
                c_gid = __builtin_amdgcn_readfirstlane(s_gid_first[w]);
                if (!has_head) continue;
                if (c_rows) {  // (nothing in front of a run's first head: nothing to close)
                    if (c_shared) {
                        fsum_wave_to_slot(s_carry, c_flags, slot_first, lane);
                    } else {
                        const uint64_t v = fsum_wave_result(s_carry, c_flags, lane);
                        if (lane == 0 && c_gid < n_groups) out[c_gid] = v;
                    }
                }
                c_shared = false;
                fsum_wave_sync();
                fsum_wave_copy(s_carry, s_acc[w], lane);
                fsum_wave_sync();
                c_flags = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)s_acc[w][FSUM_FLAGS]);
                c_rows = __builtin_amdgcn_readfirstlane(s_rows_open[w]);
                c_gid = __builtin_amdgcn_readfirstlane(s_gid_open[w]);
            }
            fsum_wave_carry_step(s_carry, lane);
            fsum_wave_sync();
        }
        __syncthreads();  // wave 0 is through with the waves' accumulators
        fsum_wave_zero(acc, lane);
        fsum_wave_sync();
    }
    if (wid == 0 && c_rows) fsum_wave_to_slot(s_carry, c_flags, slot_last, lane);
}

// One wave per slot: the slot's value, rounded, is its group's result.
__global__ __launch_bounds__(64) void k_fsum_finish(const ull* __restrict__ arena, const uint32_t* __restrict__ slot_gid,
                                                    const uint32_t* __restrict__ n_slots, uint32_t n_groups, ull* __restrict__ out) {
    __shared__ fsum_t s_a[FSUM_WORDS];
    const uint32_t    lane = threadIdx.x, slot = blockIdx.x;
    if (slot >= *n_slots) return;
    fsum_wave_copy(s_a, reinterpret_cast<const fsum_t*>(arena + (uint64_t)slot * FSUM_WORDS), lane);
    fsum_wave_sync();
    const uint32_t flags = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)s_a[FSUM_FLAGS]);
    const uint64_t v = fsum_wave_result(s_a, flags, lane);
    const uint32_t gid = slot_gid[slot];
    if (lane == 0 && gid < n_groups) out[gid] = v;
}

// ================================================================== launcher
static uint32_t fsum_tiles(uint32_t n_rows) { return n_rows / GROUP_TILE + (n_rows % GROUP_TILE != 0); }
// the runs of tiles: launch_group_reduce's arithmetic
static void fsum_runs(uint32_t n_rows, uint32_t max_grid, uint32_t& tiles_per_wg, uint32_t& n_runs) {
    const uint32_t n_tiles = fsum_tiles(n_rows);
    const uint32_t grid0 = std::max(1u, std::min(n_tiles, std::max(1u, max_grid)));
    tiles_per_wg = std::max(1u, n_tiles / grid0 + (n_tiles % grid0 != 0));
    n_runs = std::max(1u, n_tiles / tiles_per_wg + (n_tiles % tiles_per_wg != 0));
}

uint64_t fsum_scratch_bytes(uint32_t n_rows, uint32_t max_grid) {
    uint32_t tiles_per_wg, n_runs;
    fsum_runs(n_rows, max_grid, tiles_per_wg, n_runs);
    // the arena, slot_of, slot_gid, n_slots
    return (uint64_t)n_runs * FSUM_WORDS * 8 + (uint64_t)n_runs * 4 * 2 + 8;
}

void launch_fsum(const Launch& L, const ColRef& col, const uint32_t* perm, uint32_t n_rows, const unsigned long long* masks,
                 const uint32_t* tile_base, uint32_t n_groups, unsigned long long* out, uint32_t max_grid, uint8_t* scratch) {
    const uint32_t n_tiles = fsum_tiles(n_rows);
    if (!n_groups || !n_tiles) return;  // (no row: no group has a value, and k_group_reduce's count says so)
    const bool keyed = masks != nullptr;
    if (keyed != (tile_base != nullptr) || (!keyed && (perm || n_groups != 1)))
        launch_failed("fsum_reduce", "a scalar aggregate has neither masks nor a permutation and one group", false);
    if (col.width != 8) launch_failed("fsum_reduce", "an FP64 column has 8-byte values", false);
    uint32_t tiles_per_wg, n_runs;
    fsum_runs(n_rows, max_grid, tiles_per_wg, n_runs);
    ull* const      arena = reinterpret_cast<ull*>(scratch);
    const uint64_t  n_words = (uint64_t)n_runs * FSUM_WORDS;
    uint32_t* const slot_of = reinterpret_cast<uint32_t*>(arena + n_words);
    uint32_t* const slot_gid = slot_of + n_runs;
    uint32_t* const n_slots = slot_gid + n_runs;
    RJ_KLAUNCH(L, "fsum_slots", k_fsum_slots, 1, 1024, masks, tile_base, n_tiles, tiles_per_wg, n_runs, n_groups, slot_of, slot_gid, n_slots);
    RJ_KLAUNCH(L, "fsum_zero", k_fsum_zero, (uint32_t)((n_words + 255) / 256), 256, arena, n_words);
    if (keyed)
        RJ_KLAUNCH(L, "fsum_reduce", (k_fsum_reduce<true>), n_runs, GROUP_THREADS, col, perm, n_rows, masks, tile_base, n_tiles, tiles_per_wg,
                   n_groups, slot_of, arena, out);
    else
        RJ_KLAUNCH(L, "fsum_reduce", (k_fsum_reduce<false>), n_runs, GROUP_THREADS, col, perm, n_rows, masks, tile_base, n_tiles, tiles_per_wg,
                   n_groups, slot_of, arena, out);
    RJ_KLAUNCH(L, "fsum_finish", k_fsum_finish, n_runs, 64, arena, slot_gid, n_slots, n_groups, out);
}

}  // namespace rj
