// rj_sort.hip — the gfx950 (wave64) kernels of RJ_NODE_SORT and their launchers.
#include <type_traits>

#include "rj_kernel_util.hpp"
#include "rj_sortkey.hpp"

namespace rj {

// RJ_NODE_SORT: a stable LSD radix sort of {encoded key, row id}, 8 bits per pass (rj_device.hpp).
//   k_sort_encode   one key column, read through the current permutation -> order-preserving unsigned
//                   keys (rj_sortkey.hpp) + the histogram of EVERY digit position, which does not
//                   depend on the row order: the host reads it once and launches only the passes whose
//                   digit has more than one non-empty bin
//   k_sort_count    per pass: tile x digit counts, digit-major
//   k_sort_scan     ... -> where tile t's rows of digit d start in the output (one workgroup per digit)
//   k_sort_scatter  ... rows to their places, earlier rows of a digit first
// The partition passes above rank with LDS atomics (whoever arrives first), which is why they cannot
// be used here.  The rank of a row among the rows of its digit is: rows of earlier tiles (the scanned
// table) + rows of earlier waves of the tile (LDS, one counter row per wave) + rows of earlier items
// of the wave (the wave's own counter row, advanced item by item in program order) + lower lanes of the
// item with the same digit (match mask from eight ballots, mbcnt).  No atomic takes part in a rank.
//
// lanes of the wave whose 8-bit digit equals mine, among the active ones (garbage in inactive lanes)
__device__ __forceinline__ uint64_t sort_match(uint32_t d, bool active) {
    uint64_t m = __ballot(active);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool     bit = (d >> b) & 1u;
        const uint64_t v = __ballot(bit);
        m &= bit ? v : ~v;
    }
    return m;
}

template <int MODE>
__device__ __forceinline__ uint32_t sort_digit(uint64_t key, uint32_t id, uint32_t shift, const uint8_t* valid, uint32_t null_digit) {
    if constexpr (MODE == SORT_FLAG) return valid[id] ? 1u - null_digit : null_digit;
    return (uint32_t)(key >> shift) & (SORT_RADIX - 1);
}

// W = bytes of a value and of its key (4 or 8).  perm: the order the later key columns left (row i of
// the current order is row perm[i] of the relation), nullptr = the relation's own order.  hist
// (SORT_HIST_WORDS, zeroed): [p][b] += rows whose key has byte p equal to b, [SORT_NULL_DIGIT][0 / 1]
// += rows by NULL digit (nullable columns only).  Counting is order-free, so LDS atomics do here; a
// wave whose 64 rows agree on a byte (the high bytes of small numbers) adds once.
template <int W>
__global__ __launch_bounds__(SORT_THREADS) void k_sort_encode(ColRef col, const uint32_t* __restrict__ perm, uint32_t n_rows,
                                                              int32_t f64, int32_t flags, uint8_t* __restrict__ keys_out,
                                                              uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_hist[SORT_NULL_DIGIT + 1][SORT_RADIX];
    for (uint32_t k = threadIdx.x; k < (uint32_t)SORT_HIST_WORDS; k += SORT_THREADS) (&s_hist[0][0])[k] = 0;
    __syncthreads();
    const bool     desc = flags & SORTKEY_DESC, nulls_first = flags & SORTKEY_NULLS_FIRST;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_chunks = n_rows / SORT_THREADS + (n_rows % SORT_THREADS != 0);  // (n_rows + 255 may not fit 32 bits)
    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const uint32_t i = chunk * SORT_THREADS + threadIdx.x;  // (chunk * 256 < n_rows)
        const bool     active = i < n_rows;                     // lane 0 of a wave is active if any lane is
        uint64_t       key = 0;
        bool           is_null = false;
        if (active) {
            const uint32_t r = perm ? perm[i] : i;
            is_null = col.valid && !col.valid[r];
            const uint64_t bits = W == 4 ? (uint64_t)col_load32(col, r) : col_load64(col, r);
            key = is_null ? 0ull : sort_key_bits(bits, W, f64 != 0, desc);
            if constexpr (W == 4)
                reinterpret_cast<uint32_t*>(keys_out)[i] = (uint32_t)key;
            else
                reinterpret_cast<uint64_t*>(keys_out)[i] = key;
        }
        const uint64_t act = __ballot(active);
        if (!act) continue;  // (the whole wave)
#pragma unroll
        for (int p = 0; p <= W; ++p) {
            if (p == W && !col.valid) break;
            const uint32_t row = p == W ? SORT_NULL_DIGIT : p;
            const uint32_t d = p == W ? sort_null_digit(is_null, nulls_first) : (uint32_t)(key >> (8 * p)) & 255u;
            const uint32_t d0 = __builtin_amdgcn_readfirstlane(d);
            if (__ballot(active && d != d0) == 0) {
                if (lane == 0) atomicAdd(&s_hist[row][d0], (uint32_t)__popcll(act));
            } else if (active) {
                atomicAdd(&s_hist[row][d], 1u);
            }
        }
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < (uint32_t)SORT_HIST_WORDS; k += SORT_THREADS) {
        const uint32_t c = (&s_hist[0][0])[k];
        if (c) atomicAdd(&hist[k], c);
    }
}

// table[d * n_tiles + tile] = rows of the tile whose digit is d (every entry is written).  One workgroup
// per tile; a wave adds once per distinct digit of an item (match mask), so equal digits do not queue.
template <int MODE>
__global__ __launch_bounds__(SORT_THREADS) void k_sort_count(const uint8_t* __restrict__ keys, const uint32_t* __restrict__ ids,
                                                             const uint8_t* __restrict__ valid, uint32_t null_digit, uint32_t n_rows,
                                                             uint32_t shift, uint32_t n_tiles, uint32_t* __restrict__ table) {
    __shared__ uint32_t s_cnt[SORT_RADIX];
    s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t tile = blockIdx.x, tile_base = tile * SORT_TILE;  // (< n_rows)
    const uint32_t in_tile = min((uint32_t)SORT_TILE, n_rows - tile_base);
#pragma unroll 4
    for (uint32_t j = 0; j < SORT_ITEMS; ++j) {
        const uint32_t local = j * SORT_THREADS + threadIdx.x;
        const bool     active = local < in_tile;
        if (!__ballot(active)) break;  // (the whole wave, and every later item of it)
        const uint32_t i = tile_base + local;
        uint64_t       key = 0;
        uint32_t       id = 0;
        if (active) {
            if constexpr (MODE == SORT_KEY32) key = reinterpret_cast<const uint32_t*>(keys)[i];
            if constexpr (MODE == SORT_KEY64) key = reinterpret_cast<const uint64_t*>(keys)[i];
            if constexpr (MODE == SORT_FLAG) id = ids ? ids[i] : i;
        }
        const uint32_t d = active ? sort_digit<MODE>(key, id, shift, valid, null_digit) : 0u;
        const uint64_t m = sort_match(d, active);
        if (active && lane_prefix(m) == 0) atomicAdd(&s_cnt[d], (uint32_t)__popcll(m));
    }
    __syncthreads();
    table[(size_t)threadIdx.x * n_tiles + tile] = s_cnt[threadIdx.x];
}

// Workgroup d: table[d][t] -> (rows of digits below d, from the column's histogram row `hist`) + rows
// of digit d in the tiles before t, in place.
__global__ __launch_bounds__(1024) void k_sort_scan(const uint32_t* __restrict__ hist, uint32_t n_tiles, uint32_t* __restrict__ table) {
    __shared__ uint32_t s_wsum[16];
    const uint32_t d = blockIdx.x;
    uint32_t       running = 0;
    (void)block_excl_scan(threadIdx.x < d ? hist[threadIdx.x] : 0u, s_wsum, running);  // (d <= 255 < blockDim.x)
    uint32_t* row = table + (size_t)d * n_tiles;
    for (uint32_t t0 = 0; t0 < n_tiles; t0 += 1024u) {  // (n_tiles <= 2^20)
        const uint32_t t = t0 + threadIdx.x;
        const uint32_t c = t < n_tiles ? row[t] : 0u;
        uint32_t       total;
        lds_barrier();  // s_wsum is free again
        const uint32_t pre = block_excl_scan(c, s_wsum, total);
        if (t < n_tiles) row[t] = running + pre;
        running += total;
    }
}

// One workgroup per tile.  keys_out == nullptr: only the ids move (the last pass of a column: nobody
// reads its keys again).  ids_in == nullptr: the rows are still in the relation's order, id = position.
template <int MODE>
__global__ __launch_bounds__(SORT_THREADS) void k_sort_scatter(const uint8_t* __restrict__ keys_in, const uint32_t* __restrict__ ids_in,
                                                               const uint8_t* __restrict__ valid, uint32_t null_digit, uint32_t n_rows,
                                                               uint32_t shift, uint32_t n_tiles, const uint32_t* __restrict__ table,
                                                               uint8_t* __restrict__ keys_out, uint32_t* __restrict__ ids_out) {
    constexpr uint32_t NWAVES = SORT_THREADS / 64, WAVE_ROWS = SORT_TILE / NWAVES;
    using KeyT = std::conditional_t<MODE == SORT_KEY64, uint64_t, uint32_t>;
    __shared__ uint32_t s_cnt[NWAVES][SORT_RADIX];  // phase 1: a wave's rows per digit so far; phase 2: where they start
#pragma unroll
    for (uint32_t w = 0; w < NWAVES; ++w) s_cnt[w][threadIdx.x] = 0;
    __syncthreads();
    const uint32_t tile = blockIdx.x, tile_base = tile * SORT_TILE;  // (< n_rows)
    const uint32_t in_tile = min((uint32_t)SORT_TILE, n_rows - tile_base);
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    const uint32_t local0 = wid * WAVE_ROWS + lane;  // item j: row tile_base + local0 + 64 j
    KeyT           key[SORT_ITEMS];
    uint32_t       id[SORT_ITEMS];
    uint32_t       dr[SORT_ITEMS];  // digit << 16 | rank among the wave's rows of the digit
#pragma unroll
    for (int j = 0; j < SORT_ITEMS; ++j) {
        const uint32_t i = tile_base + local0 + 64u * j;
        const bool     active = local0 + 64u * j < in_tile;
        key[j] = 0;
        id[j] = 0;
        if (active) {
            if constexpr (MODE != SORT_FLAG) key[j] = reinterpret_cast<const KeyT*>(keys_in)[i];
            id[j] = ids_in ? ids_in[i] : i;
        }
    }
    uint32_t* mine = s_cnt[wid];
#pragma unroll
    for (int j = 0; j < SORT_ITEMS; ++j) {
        const bool     active = local0 + 64u * j < in_tile;
        const uint32_t d = active ? sort_digit<MODE>(key[j], id[j], shift, valid, null_digit) : 0u;
        const uint64_t m = sort_match(d, active);
        const uint32_t below = lane_prefix(m);
        const uint32_t before = active ? mine[d] : 0u;  // every lane reads, then one lane per digit adds
        __builtin_amdgcn_wave_barrier();
        if (active && below == 0) mine[d] = before + (uint32_t)__popcll(m);
        __builtin_amdgcn_wave_barrier();
        dr[j] = d << 16 | (before + below);
    }
    __syncthreads();
    {
        uint32_t at = table[(size_t)threadIdx.x * n_tiles + tile];  // thread d: where the tile's rows of digit d start
#pragma unroll
        for (uint32_t w = 0; w < NWAVES; ++w) {
            const uint32_t c = s_cnt[w][threadIdx.x];
            s_cnt[w][threadIdx.x] = at;
            at += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SORT_ITEMS; ++j) {
        const bool     active = local0 + 64u * j < in_tile;
        const uint32_t pos = active ? mine[dr[j] >> 16] + (dr[j] & 0xffffu) : 0u;
        if (active && pos < n_rows) {  // (a table that did not fit the keys must not write outside)
            ids_out[pos] = id[j];
            if constexpr (MODE != SORT_FLAG)
                if (keys_out) reinterpret_cast<KeyT*>(keys_out)[pos] = key[j];
        }
    }
}

// out[i] = base + i: the slice of a relation that no pass reordered
__global__ __launch_bounds__(256) void k_sort_iota(uint32_t* __restrict__ out, uint32_t base, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) out[i] = base + i;
}

// ================================================================== launchers
template <int N>
using int_c = std::integral_constant<int, N>;

void launch_sort_encode(const Launch& L, const ColRef& col, const uint32_t* perm, uint32_t n_rows, bool f64, int32_t flags,
                        uint8_t* keys_out, uint32_t* hist, uint32_t grid) {
    if (!n_rows || !grid) return;
    if (col.width == 4)
        RJ_KLAUNCH(L, "sort_encode", (k_sort_encode<4>), grid, SORT_THREADS, col, perm, n_rows, (int32_t)f64, flags, keys_out, hist);
    else
        RJ_KLAUNCH(L, "sort_encode", (k_sort_encode<8>), grid, SORT_THREADS, col, perm, n_rows, (int32_t)f64, flags, keys_out, hist);
}

static uint32_t sort_tiles(uint32_t n_rows) { return n_rows / SORT_TILE + (n_rows % SORT_TILE != 0); }

template <class F>
static void for_sort_mode(const char* name, int mode, F&& f) {
    switch (mode) {
    case SORT_KEY32: return f(int_c<SORT_KEY32>{});
    case SORT_KEY64: return f(int_c<SORT_KEY64>{});
    case SORT_FLAG: return f(int_c<SORT_FLAG>{});
    default: launch_failed(name, "no kernel for this digit source", true);
    }
}

void launch_sort_count(const Launch& L, int mode, const uint8_t* keys, const uint32_t* ids, const uint8_t* valid, uint32_t null_digit,
                       uint32_t n_rows, uint32_t shift, uint32_t* table) {
    if (!n_rows) return;
    const uint32_t n_tiles = sort_tiles(n_rows);
    for_sort_mode("sort_count", mode, [&](auto M) {
        RJ_KLAUNCH(L, "sort_count", (k_sort_count<decltype(M)::value>), n_tiles, SORT_THREADS, keys, ids, valid, null_digit, n_rows,
                   shift, n_tiles, table);
    });
}

void launch_sort_scan(const Launch& L, const uint32_t* hist, uint32_t n_rows, uint32_t* table) {
    if (!n_rows) return;
    RJ_KLAUNCH(L, "sort_scan", k_sort_scan, SORT_RADIX, 1024, hist, sort_tiles(n_rows), table);
}

void launch_sort_scatter(const Launch& L, int mode, const uint8_t* keys_in, const uint32_t* ids_in, const uint8_t* valid,
                         uint32_t null_digit, uint32_t n_rows, uint32_t shift, const uint32_t* table, uint8_t* keys_out,
                         uint32_t* ids_out) {
    if (!n_rows) return;
    const uint32_t n_tiles = sort_tiles(n_rows);
    for_sort_mode("sort_scatter", mode, [&](auto M) {
        RJ_KLAUNCH(L, "sort_scatter", (k_sort_scatter<decltype(M)::value>), n_tiles, SORT_THREADS, keys_in, ids_in, valid,
                   null_digit, n_rows, shift, n_tiles, table, keys_out, ids_out);
    });
}

void launch_sort_iota(const Launch& L, uint32_t* out, uint32_t base, uint32_t n) {
    if (!n) return;
    RJ_KLAUNCH(L, "sort_iota", k_sort_iota, n / 256u + (n % 256u != 0), 256, out, base, n);
}

}  // namespace rj
