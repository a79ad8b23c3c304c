// rj_kernels.hpp — host-callable launchers of every gfx950 (CDNA4, wave64) kernel, one block per kernel file.
//
// The radix join is integer / indexing work bound by HBM bandwidth (no MFMA):
//   K0  page headers        rj_pages.hip      4 B read per 8 KiB page
//   K1  page decode         rj_pages.hip      irregular (NULL-bearing) pages -> dense values + validity
//   K2  pass histogram      rj_partition.hip  per-workgroup LDS histogram, flushed once per tile group
//   K3  bin scan            rj_partition.hip  one workgroup per input segment, wave-shuffle scan
//   K4  pass scatter        rj_partition.hip  tile of 16384 tuples sorted by digit in LDS (LDS atomics give the
//                                             rank), runs written out contiguously = software write-combining
//   K5/6 build + probe      rj_join.hip       per-partition bucketised hash table in LDS (one 16-byte read per
//                                             probe), ballot/mbcnt output offsets, one global reservation per
//                                             4096 probe tuples, streams written straight into Page images
//                           rj_bcast.hip      (the broadcast form: a small build side, nothing partitioned)
//   K7  gather              rj_pages.hip      row-id -> column value (generic late materialisation)
//   K8  page finish/encode  rj_pages.hip      Page headers + validity bitmaps of the result
// The other node kinds build on these: rj_filter.hip (semi / anti joins), rj_outer.hip, rj_full.hip (outer and full
// outer joins), rj_agg.hip (hash aggregation), rj_select.hip, rj_map.hip, rj_sort.hip, rj_group.hip, rj_fsum.hip,
// rj_window.hip, rj_frame.hip, rj_setop.hip; rj_varchar_dev.hip holds the VARCHAR kernels.
// Reference counterparts are cited at each kernel (paths relative to the reference).
#pragma once
#include <hip/hip_runtime.h>

#include "rj_device.hpp"

namespace rj {

// Stream + optional per-kernel HIP-event timing.  Implemented in rj_context.hip.
// timed(): should this launch be timed?  If so it hands out the start/stop events the launch
// itself records (hipExtLaunchKernelGGL: the timestamps of the dispatch packet — no extra
// event packets, so no idle gaps at the kernel boundaries).
// logged(): set only while the context's launch log is on (rj_debug_launch_log); receives the
// kernel handle of every launch, so that tests can see which template instantiation ran.
struct Launch {
    hipStream_t stream;
    bool (*timed)(void* self, const char* name, hipEvent_t* start, hipEvent_t* stop);
    void* self;
    void (*logged)(void* self, const void* kernel);
};

// A launch the runtime rejected, or a template combination no kernel exists for: throws
// rj::Error (RJ_ERR_DEVICE / RJ_ERR_UNSUPPORTED).  Implemented in rj_context.hip.
[[noreturn]] void launch_failed(const char* kernel, const char* what, bool unsupported);

// ======================================================================================================== rj_pages.hip
// ---- page metadata / decode (replaces Table::from_columnar, reference
//      src/build_table.cpp:312-436, for fixed-width columns)
// flags[0] = #pages breaking the "regular" shape, flags[1..2] = total rows (u64)
void launch_page_headers(const Launch& L, const uint8_t* pages, uint32_t n_pages, uint32_t rows_full,
                         uint32_t* page_rows, unsigned long long* flags);
// flag[0] += pages that hold a NON-NULL value at a row index >= num_rows (the reference's
// "row_idx" error, src/build_table.cpp:334-336); row_base = exclusive scan of the page rows
void launch_rows_beyond(const Launch& L, const uint8_t* pages, uint32_t n_pages,
                        const uint32_t* row_base, uint64_t num_rows, unsigned long long* flag);
void launch_decode_pages(const Launch& L, const uint8_t* pages, uint32_t n_pages, int width,
                         const uint32_t* row_base, uint64_t num_rows, uint8_t* values,
                         uint8_t* valid);

// ---- materialise (replaces the per-row output copy, reference src/execute.cpp:236-242,
//      and Table::to_columnar, src/build_table.cpp:456-594)
void launch_gather(const Launch& L, const ColRef& src, const uint32_t* idx, uint64_t n,
                   const OutStream& dst, uint8_t* dst_valid);
// k_gather for an optional side's row-index stream: OUTER_NO_ROW gives a NULL (valid byte 0, value
// 0) and is never dereferenced; dense values and validity bytes for every row
void launch_outer_gather(const Launch& L, const ColRef& src, const uint32_t* idx, uint64_t n, uint8_t* dst,
                         uint8_t* dst_valid);
void launch_finish_pages(const Launch& L, uint8_t* pages, uint64_t n_rows, int width);
// headers + bitmaps of up to three probe-written streams, row count read on the device
void launch_finish_streams(const Launch& L, uint8_t* const* pages, const int* widths, uint32_t n,
                           const unsigned long long* n_rows_dev, uint64_t cap_rows);
void launch_encode_nullable(const Launch& L, const uint8_t* values, const uint8_t* valid,
                            uint64_t n_rows, int width, uint8_t* pages);
// wide carries (several payload columns travelling with the key): validity bits of up to three
// columns as one word per row; the emitted records -> one dense array (+ validity bytes) per column
void launch_pack_validity(const Launch& L, const uint8_t* v0, const uint8_t* v1, const uint8_t* v2, uint32_t n,
                          uint32_t* out);
void launch_split_records(const Launch& L, const SplitParams& sp, uint64_t n);
// test hook: keeps the stream busy for `ms` milliseconds (bounded; see RJ_DEBUG_SHARD_FAIL)
void launch_debug_stall(const Launch& L, uint32_t ms);

// ==================================================================================================== rj_partition.hip
// ---- small single-workgroup scans
// off[i] = sum_{j<i} in[j], off[n] = total; cursor (optional) = copy of off[0..n)
void launch_scan_bins(const Launch& L, const uint32_t* in, uint32_t n, uint32_t* off,
                      uint32_t* cursor);
// per-segment scan: off[seg*F+d] = seg_off[seg] + prefix of hist[seg][0..d); off[nseg*F] = total
void launch_scan_segments(const Launch& L, const uint32_t* hist, const uint32_t* seg_off,
                          uint32_t nseg, uint32_t F, uint32_t xcd_log2, uint32_t* off, uint32_t* cursor);
// grp_start[s] = sum_{t<s} ceil(len_t / group_tuples) over segments (seg_off[nseg+1]; with seg_end,
// segment t is [seg_off[t], seg_end[t]) and seg_off needs only nseg entries)
void launch_group_table(const Launch& L, const uint32_t* seg_off, uint32_t nseg,
                        uint32_t group_tuples, uint32_t* grp_start, const uint32_t* seg_end = nullptr);

// ---- radix partition pass (replaces the ≤128-way hash partition of row indices,
//      reference src/execute.cpp:124-184)
// Source pass: tuples are formed from columns (page decode fused in).
void launch_pass_hist_src(const Launch& L, const TupleSrc& src, int key_words, const PassParams& pp,
                          uint32_t n_groups);
// Fine histogram of a two-pass plan (both digits in one read of the source): fine[d1 * F2 + d2],
// pre-zeroed; `grid` persistent workgroups (one per CU).  launch_scan_fine turns it into the
// pass-2 offsets/cursors (off2[F1*F2 + 1], cursor2) and the pass-1 ones (off1[F1 + 1], cursor1).
// xcd_tpg > 0 (grid a multiple of 8): XCD-aware placement of the first pass — workgroup w counts
// the tile groups (of xcd_tpg tiles) g with g & 7 == w & 7 and also adds its pass-1 digit counts
// to coarse_x[d1 * 8 + (w & 7)] (pre-zeroed); launch_scan_fine then writes cursor1[d1 * 8 + x]
void launch_fine_hist_src(const Launch& L, const TupleSrc& src, int key_words, uint32_t shift,
                          uint32_t b1, uint32_t b2, uint32_t grid, uint32_t* fine, uint32_t xcd_tpg = 0,
                          uint32_t* coarse_x = nullptr);
// the same over tuples that already sit in the partition layout (hashed words / packed pairs):
// the passes behind a sharded join's exchange
void launch_fine_hist_words(const Launch& L, const Words& in, bool packed, uint32_t n, uint32_t shift,
                            uint32_t b1, uint32_t b2, uint32_t grid, uint32_t* fine, uint32_t xcd_tpg = 0,
                            uint32_t* coarse_x = nullptr);
void launch_scan_fine(const Launch& L, const uint32_t* fine, uint32_t F1, uint32_t F2,
                      uint32_t* off2, uint32_t* cursor2, uint32_t* off1, uint32_t* cursor1,
                      const uint32_t* coarse_x = nullptr);
// aos3 (key_words == 1, carry_words == 2, last pass of a plan): out.w[0] receives 12-byte
// {hashed key, carry lo, carry hi} tuples instead of a key array + a pair array
void launch_pass_scatter_src(const Launch& L, const TupleSrc& src, int key_words, int carry_words,
                             const PassParams& pp, uint32_t n_groups, const Words& out, bool aos3 = false,
                             const SpecParams* spec = nullptr);
// Speculative first pass (SpecParams; `spec` above and in launch_pass_scatter_src_packed selects the scatter
// that checks its reservations): the sampled histogram — launch_pass_hist_src's grid and bins —, the
// capacities out of it (start[nbins], limit[nbins], cursor[nbins]; nothing beyond cap_max; z = the normal
// quantile of the margin) and, behind the scatter, the second pass' input segments [start[i], seg_end[i]) and
// output segment bases oseg_off[F + 1] (F <= PT_MAXF digits of 8 sub-ranges each)
void launch_pass_sample_src(const Launch& L, const TupleSrc& src, int key_words, const PassParams& pp,
                            const SpecParams& sp, uint32_t n_groups);
void launch_spec_caps(const Launch& L, const uint32_t* sample, uint32_t nbins, uint32_t sample_log2, float z,
                      uint32_t cap_max, uint32_t* start, uint32_t* limit, unsigned long long* cursor);
void launch_spec_close(const Launch& L, const unsigned long long* cursor, const uint32_t* start, const uint32_t* limit,
                       uint32_t F, uint32_t* seg_end, uint32_t* oseg_off);
// Dense pass: re-partition every segment of already partitioned word arrays.
void launch_pass_hist_dense(const Launch& L, const Words& in, const PassParams& pp,
                            uint32_t n_groups);
// pair_word >= 0: words pair_word / pair_word+1 (a two-word carry) live as 8-byte pairs in
// in.w[pair_word] / out.w[pair_word] (what every pass writes for two-word carries); else -1
void launch_pass_scatter_dense(const Launch& L, const Words& in, int n_words, int pair_word,
                               const PassParams& pp, uint32_t n_groups, const Words& out, bool aos3 = false);

// 12-byte tuples between the passes of a key + two-word-carry plan: the histogram of a later
// pass reads the 16-bit digit side array its predecessor wrote (PassParams::side_out), the
// scatter reads and writes 12-byte tuples
void launch_pass_hist_digits(const Launch& L, const uint16_t* digits, const PassParams& pp, uint32_t n_groups);
// ... or, without a side array, fishes the keys out of the 12-byte tuples themselves
void launch_pass_hist_aos3(const Launch& L, const uint32_t* in_tuples, const PassParams& pp, uint32_t n_groups);
void launch_pass_scatter_aos3(const Launch& L, const uint32_t* in_tuples, const PassParams& pp, uint32_t n_groups,
                              uint32_t* out_tuples);

// Packed layout ({hashed key, carry} pairs in one array) for one key word + one carry word.
void launch_pass_hist_packed(const Launch& L, const uint32_t* in_pairs, const PassParams& pp,
                             uint32_t n_groups);
void launch_pass_scatter_src_packed(const Launch& L, const TupleSrc& src, const PassParams& pp,
                                    uint32_t n_groups, uint32_t* out_pairs, bool blocked_out = false,
                                    const SpecParams* spec = nullptr);
// (pairs between the passes of a packed plan in blocks of 256 keys + 256 carries: the next histogram reads the keys only)
void launch_pass_hist_blocked(const Launch& L, const uint32_t* in_blocked, const PassParams& pp, uint32_t n_groups);
void launch_pass_scatter_blocked(const Launch& L, const uint32_t* in_blocked, const PassParams& pp, uint32_t n_groups,
                                 uint32_t* out_pairs, bool blocked_out);
void launch_pass_scatter_packed(const Launch& L, const uint32_t* in_pairs, const PassParams& pp,
                                uint32_t n_groups, uint32_t* out_pairs);

// ---- the probe partitions above JN_HEAVY tuples, cut into tasks for the build + probe kernels
// (off_pairs: JoinParams')
void launch_heavy_tasks(const Launch& L, const uint32_t* offR, const uint32_t* offS, uint32_t NP,
                        uint32_t* tasks, uint32_t* n_heavy, uint32_t max_tasks, uint32_t off_pairs = 0);

// ---- Speculative LAST pass of a two-pass inner join (rj_device.hpp: SpecParams).  `pp` is the exact second
// pass' (grid, group table over the input segments, xcd_remap; xcd_log2 = 0), pp.hist the zeroed sample bins,
// one per final partition.  in_keys: the first pass' key array, or (blocked) its blocked pairs.
//   sample  -> pp.hist[oseg * F + d2]
//   caps    -> pairs[2 q] = begin of final partition q (exclusive scan of the capacities), limit[q] = begin + capacity,
//              cursor[q] = begin; nothing beyond cap_max.  seg_sum: nseg words of scratch
//   scatter -> 12-byte tuples (dense key array + pair array in) or pairs (blocked pairs in)
//   close   -> pairs[2 q + 1] = end = min(position, limit[q])
void launch_last_sample(const Launch& L, const uint32_t* in_keys, bool blocked, const PassParams& pp, const LastParams& sp,
                        uint32_t n_groups);
void launch_last_caps(const Launch& L, const uint32_t* sample, uint32_t nseg, uint32_t F, uint32_t sample_log2, float z,
                      uint32_t cap_max, unsigned long long* seg_sum, uint32_t* pairs, uint32_t* limit,
                      uint32_t* cursor);
void launch_last_scatter_dense(const Launch& L, const Words& in, const PassParams& pp, uint32_t n_groups, const Words& out,
                               const LastParams& sp);
void launch_last_scatter_blocked(const Launch& L, const uint32_t* in_blocked, const PassParams& pp, uint32_t n_groups,
                                 uint32_t* out_pairs, const LastParams& sp);
void launch_last_close(const Launch& L, const uint32_t* cursor, const uint32_t* limit, uint32_t nbins,
                       uint32_t* pairs);

// ========================================================================================================= rj_join.hip
// ---- build + probe (replaces reference src/execute.cpp:196-249)
// grid = jp.heavy_grid + ceil(jp.NP / join_partitions_per_workgroup(...))
uint32_t join_partitions_per_workgroup(int key_words, int cw_build, const JoinParams& jp);
void launch_join(const Launch& L, int key_words, int cw_build, int cw_probe, const JoinParams& jp,
                 uint32_t grid);

// ======================================================================================================== rj_bcast.hip
// Broadcast join: build side of at most JN_RMAX rows, no partitioning; `grid` workgroups stride
// over the probe rows in chunks of JN_SUB.
void launch_join_bcast(const Launch& L, int key_words, int cw_build, int cw_probe,
                       const BcastParams& bp, uint32_t grid);

// ======================================================================================================= rj_filter.hip
// ---- semi / anti joins (FilterParams): key_words 1 or 2, cw_preserved 0..MAX_WORDS - key_words
// broadcast: filter side of at most JN_RMAX rows, `grid` workgroups stride over the preserved rows
void launch_filter_bcast(const Launch& L, int key_words, int cw_preserved, const FilterParams& fp, uint32_t grid);
// partitioned: grid = fp.heavy_grid + fp.NP (one workgroup per heavy task, then per partition)
void launch_filter_join(const Launch& L, int key_words, int cw_preserved, const FilterParams& fp, uint32_t grid);
// ANTI after the partitioned filter: the preserved rows the first radix pass drops (NULL key,
// FP64 NaN key) go out through the same cursor
void launch_filter_nullkeys(const Launch& L, int key_words, int cw_preserved, const FilterParams& fp, uint32_t grid);

// ======================================================================================================== rj_outer.hip
// ---- outer joins (OuterParams): key_words 1 or 2; cw_optional 0 (nothing), 1 (row index) or the
// words of a wide carry; cw_preserved 0..MAX_WORDS - key_words
// broadcast: optional side of at most JN_RMAX rows (or none / keys of another type)
void launch_outer_bcast(const Launch& L, int key_words, int cw_optional, int cw_preserved, const OuterParams& op,
                        uint32_t grid);
// partitioned: grid = op.heavy_grid + op.NP (one workgroup per heavy task, then per partition)
void launch_outer_join(const Launch& L, int key_words, int cw_optional, int cw_preserved, const OuterParams& op,
                       uint32_t grid);
// after the partitioned probe: the preserved rows the first radix pass drops (NULL key, FP64 NaN
// key) go out padded through the same cursor
void launch_outer_nullkeys(const Launch& L, int key_words, int cw_preserved, const OuterParams& op, uint32_t grid);

// ========================================================================================================= rj_full.hip
// ---- full outer joins (FullParams): the outer join's shapes, both carries under the optional rules
// (0 = nothing, 1 = row index, 2 / 3 = a wide record that ends in a validity word)
// broadcast probe: built side of at most JN_RMAX rows (or none / keys of another type); ORs the
// matched build rows into fp.flags (bit = row of the built child)
void launch_full_bcast(const Launch& L, int key_words, int cw_optional, int cw_preserved, const FullParams& fp,
                       uint32_t grid);
// partitioned probe: grid = fp.o.heavy_grid + fp.o.NP; ORs the matched build tuples into fp.flags
// (bit = index in the partitioned build arrays)
void launch_full_join(const Launch& L, int key_words, int cw_optional, int cw_preserved, const FullParams& fp,
                      uint32_t grid);
// after the partitioned probe: the build tuples whose flag stayed clear, probed side padded
void launch_full_unmatched(const Launch& L, int key_words, int cw_built, const FullParams& fp, uint32_t grid);
// after a probe: the rows of the built child without a usable key (NULL, FP64 NaN, keyless) and —
// fp.use_flags, broadcast — the rows whose flag stayed clear, probed side padded
void launch_full_buildrows(const Launch& L, int key_words, int cw_built, const FullParams& fp, uint32_t grid);

// ========================================================================================================== rj_agg.hip
// ---- aggregation (AggParams): key_words 1 or 2, carry_words 0..MAX_WORDS - key_words
// the merge table's entries (ap.m_slots + 2) before anybody adds to them
void launch_agg_merge_init(const Launch& L, const AggParams& ap, uint32_t grid);
// grid = ap.heavy_grid + ap.NP (one workgroup per heavy task, then per partition)
void launch_agg_parts(const Launch& L, int key_words, int carry_words, const AggParams& ap, uint32_t grid);
// the rows the first radix pass drops (NULL key): one group, into the merge table
void launch_agg_nullkey(const Launch& L, int carry_words, const AggParams& ap, uint32_t grid);
// the merge table's live entries -> output rows
void launch_agg_emit(const Launch& L, int key_words, const AggParams& ap, uint32_t grid);
// an accumulator array as a result column: values narrowed to `width` bytes (dst, optional) and
// validity bytes nn[i] != 0 (dst_valid, optional; nn == nullptr: all valid)
void launch_agg_column(const Launch& L, const unsigned long long* src, const unsigned long long* nn, uint64_t n, int width,
                       uint8_t* dst, uint8_t* dst_valid);

// ======================================================================================================= rj_select.hip
// ---- selection (RJ_NODE_SELECT): the rows of [0, n_rows) for which the program (a device copy of
// SelectProg, n_ops of its ops) leaves 1 -> their row ids in out_ids (room for n_rows), ascending
// within every tile of SEL_TILE rows; *cursor (zeroed) += their number.  `grid` workgroups stride
// over the tiles.
void launch_select(const Launch& L, const SelectProg* prog, uint32_t n_ops, uint32_t n_rows, uint32_t* out_ids,
                   unsigned long long* cursor, uint32_t grid);

// ========================================================================================================== rj_map.hip
// ---- computed columns (RJ_NODE_MAP, rj_map.hip): the n_ops ops of the program (a device copy of MapProg,
// rj_expr.hpp) over every row of [0, n_rows); every X_OUT op names the dense arrays it writes.  `grid`
// workgroups stride over the tiles of MAP_TILE rows.
struct MapProg;
void launch_map(const Launch& L, const MapProg* prog, uint32_t n_ops, uint32_t n_rows, uint32_t grid);

// ========================================================================================================= rj_sort.hip
// ---- sort (RJ_NODE_SORT): a stable LSD radix sort of {key, row id}, SORT_RADIX bins per pass, tiles of
// SORT_TILE rows (rj_device.hpp).  n_tiles = ceil(n_rows / SORT_TILE) everywhere.
// One key column read through `perm` (row i of the current order = row perm[i]; nullptr = i) -> keys_out
// (n_rows keys of col.width bytes) and hist (SORT_HIST_WORDS, zeroed) += the counts of every digit
// position; flags = RJ_SORT_DESC | RJ_SORT_NULLS_FIRST.  `grid` workgroups stride over the rows.
void launch_sort_encode(const Launch& L, const ColRef& col, const uint32_t* perm, uint32_t n_rows, bool f64, int32_t flags,
                        uint8_t* keys_out, uint32_t* hist, uint32_t grid);
// One pass (mode: SortMode; SORT_FLAG reads valid[id] and gives a NULL row the digit null_digit):
// table[SORT_RADIX][n_tiles] = rows per digit and tile ...
void launch_sort_count(const Launch& L, int mode, const uint8_t* keys, const uint32_t* ids, const uint8_t* valid, uint32_t null_digit,
                       uint32_t n_rows, uint32_t shift, uint32_t* table);
// ... -> where they start in the output (hist: the SORT_RADIX totals of this digit position) ...
void launch_sort_scan(const Launch& L, const uint32_t* hist, uint32_t n_rows, uint32_t* table);
// ... and the rows moved there, stably.  ids_in == nullptr: id = position; keys_out == nullptr: ids only.
void launch_sort_scatter(const Launch& L, int mode, const uint8_t* keys_in, const uint32_t* ids_in, const uint8_t* valid,
                         uint32_t null_digit, uint32_t n_rows, uint32_t shift, const uint32_t* table, uint8_t* keys_out,
                         uint32_t* ids_out);
// out[i] = base + i, i < n
void launch_sort_iota(const Launch& L, uint32_t* out, uint32_t base, uint32_t n);

// ======================================================================================================== rj_group.hip
// ---- grouping (RJ_NODE_GROUP): runs of equal keys in the order the sort left, tiles of GROUP_TILE
// positions (rj_device.hpp).  perm: row i of that order = row perm[i] (nullptr = i); masks: one 64-bit
// head mask per 64 positions (ceil(n_rows / 64)); n_tiles = ceil(n_rows / GROUP_TILE) everywhere.
// One key column: heads where it changes.  first: the masks are written, else OR-ed into; last:
// tile_heads[n_tiles] = heads per tile.
void launch_group_heads(const Launch& L, const ColRef& col, const uint32_t* perm, uint32_t n_rows, bool f64, bool first, bool last,
                        unsigned long long* masks, uint32_t* tile_heads);
// tile_base[n_tiles + 1] = exclusive scan of tile_heads, *total = the group count
void launch_group_scan(const Launch& L, const uint32_t* tile_heads, uint32_t n_rows, uint32_t* tile_base, uint32_t* total);
// out[g] (col.width bytes) = the canonical key value of group g, out_valid[g] (optional) = 0 for the NULL group
void launch_group_keys(const Launch& L, const ColRef& col, const uint32_t* perm, uint32_t n_rows, bool f64,
                       const unsigned long long* masks, const uint32_t* tile_base, uint32_t n_groups, uint8_t* out, uint8_t* out_valid);
// One aggregated column (col == nullptr: none, COUNT(*) only) -> the arrays of `acc`, one entry per
// group, every entry written whatever the memory held (k_group_init, then k_group_reduce on at most
// max_grid workgroups).  masks == tile_base == perm == nullptr: the scalar aggregate, one group of all
// rows (n_groups = 1; the kernel's variant without heads) — also over n_rows = 0, where the identities
// are the result.
void launch_group_reduce(const Launch& L, const ColRef* col, const uint32_t* perm, uint32_t n_rows, bool f64,
                         const unsigned long long* masks, const uint32_t* tile_base, uint32_t n_groups, const GroupAcc& acc,
                         uint32_t max_grid);
// an accumulator array as a result column of `width` bytes: decode = GroupDecode; validity bytes
// nn[i] != 0 (dst_valid optional; nn == nullptr: all valid), the value of a NULL is 0
void launch_group_column(const Launch& L, const unsigned long long* src, const unsigned long long* nn, uint64_t n, int decode, int width,
                         uint8_t* dst, uint8_t* dst_valid);

// ========================================================================================================= rj_fsum.hip
// ---- RJ_AGG_FSUM (rj_fsum.hip): out[g] = the bits of the exactly rounded sum of the non-NULL values of
// the FP64 column `col` in group g (+0.0 where there is none: k_group_reduce's count says which are
// NULL), every entry written whatever the memory held.  perm, masks, tile_base, max_grid and the scalar
// aggregate as for launch_group_reduce; n_rows = 0 launches nothing.  scratch: fsum_scratch_bytes()
// bytes, 8-byte aligned (the arena of the groups that runs of tiles share, and their slots).
uint64_t fsum_scratch_bytes(uint32_t n_rows, uint32_t max_grid);
void     launch_fsum(const Launch& L, const ColRef& col, const uint32_t* perm, uint32_t n_rows, const unsigned long long* masks,
                     const uint32_t* tile_base, uint32_t n_groups, unsigned long long* out, uint32_t max_grid, uint8_t* scratch);

// ======================================================================================================= rj_window.hip
// ---- window functions (RJ_NODE_WINDOW): P / Q = the head masks of the partitions / the peer groups in
// the grouping's layout, over the order the sort left; one entry per quarter of a tile in WinMarks / WinTails
// (ceil(n_rows / WIN_QUARTER)); max_chunk: cap on the entries a carry kernel's workgroup takes per step
// (0 = one per thread).
// masks[0] = 1, every other word 0: one partition of all rows
void launch_win_one_head(const Launch& L, unsigned long long* masks, uint32_t n_rows);
// k_win_marks, k_win_carry, k_win_ranks: the arrays of `out` that are wanted
void launch_win_ranks(const Launch& L, const unsigned long long* P, const unsigned long long* Q, uint32_t n_rows, const WinMarks& m,
                      const WinRanks& out, uint32_t max_chunk);
// k_win_tails, k_win_tail_carry, k_win_scan: the segmented inclusive scan of one value column over the
// P segments -> the arrays of `out` that are wanted
void launch_win_scan(const Launch& L, const ColRef& col, const uint32_t* perm, uint32_t n_rows, bool f64, const unsigned long long* P,
                     const WinTails& tails, const WinScan& out, uint32_t max_chunk);
// row i of a result column of `width` bytes = src[peer_end[i]] (src == nullptr: the count nn[...]),
// decode = GroupDecode; validity bytes nn[peer_end[i]] != 0 where dst_valid is given, the value of a NULL is 0
void launch_win_column(const Launch& L, const unsigned long long* src, const uint32_t* nn, const uint32_t* peer_end, uint64_t n, int decode,
                       int width, uint8_t* dst, uint8_t* dst_valid);

// ======================================================================================================== rj_frame.hip
// ---- the frame layer of RJ_NODE_WINDOW (rj_frame.hip): `rows` = every position's partition (k_win_ranks
// with Q := P), lo / hi = ROWS BETWEEN lo AND hi as signed offsets (any int64_t: rj_frame.hpp clamps them)
// k_frame_pick: row i = the value of `col` (through perm) at the frame's first or last position (end =
// FramePick), its own bits; validity bytes 0 where the frame is empty or the value NULL
void launch_frame_pick(const Launch& L, const ColRef& col, const uint32_t* perm, uint32_t n_rows, const FrameRows& rows, int64_t lo, int64_t hi,
                       int end, uint8_t* dst, uint8_t* dst_valid);
// k_frame_ntile: NTILE(buckets), buckets >= 1
void launch_frame_ntile(const Launch& L, uint32_t n_rows, const FrameRows& rows, int64_t buckets, unsigned long long* dst);
// k_frame_sum: what = FrameSum over the frame, from the scan's running count nn and running sum (the
// latter for FRAME_SUM only, neither for FRAME_COUNT_STAR); dst_valid optional
void launch_frame_sum(const Launch& L, const uint32_t* nn, const unsigned long long* sum, uint32_t n_rows, const FrameRows& rows, int64_t lo,
                      int64_t hi, int what, unsigned long long* dst, uint8_t* dst_valid);
// the words of a range-extreme tree over n_rows positions, level 0 included
uint64_t frame_tree_words(uint64_t n_rows);
// k_frame_leaves, k_frame_levels: the tree of `col` under MIN or MAX
void launch_frame_tree(const Launch& L, const ColRef& col, const uint32_t* perm, uint32_t n_rows, bool f64, bool is_max,
                       unsigned long long* tree);
// k_frame_extreme: MIN / MAX over the frame from the tree, NULL where the count nn says so; decode = GroupDecode
void launch_frame_extreme(const Launch& L, const unsigned long long* tree, const uint32_t* nn, uint32_t n_rows, const FrameRows& rows, int64_t lo,
                          int64_t hi, bool is_max, int decode, int width, uint8_t* dst, uint8_t* dst_valid);

// ======================================================================================================== rj_setop.hip
// ---- set operations (RJ_NODE_SETOP, rj_setop.hip): both children's rows in one relation of n_rows rows
// (row id < n_left: a left row), ordered and cut into runs by the sort's and the grouping's kernels
// (perm, masks, tile_base as above).  max_grid: cap on the workgroups of the kernels that walk tiles.
// One column of both children, `r` behind `l` (n = rows of both): dst dense or Page images (the caller
// finishes those), validity bytes where dst_valid is given (1 for a side without any)
void launch_setop_concat(const Launch& L, const ColRef& l, const ColRef& r, uint32_t n_left, uint64_t n, const OutStream& dst,
                         uint8_t* dst_valid);
// k_setop_left, k_setop_scan, k_setop_runs: runs.start / runs.left [n_runs + 1]: where run g begins and the
// left rows in front of it; entry n_runs = (n_rows, n_left).  tile_left [n_tiles], tile_lbase [n_tiles + 1]: scratch.
void launch_setop_runs(const Launch& L, const uint32_t* perm, uint32_t n_rows, uint32_t n_left, const unsigned long long* masks,
                       const uint32_t* tile_base, uint32_t n_runs, uint32_t* tile_left, uint32_t* tile_lbase, const SetopRuns& runs,
                       uint32_t max_grid);
// k_setop_mult, k_setop_scan, k_setop_offsets: off[n_runs + 1] = the exclusive scan of the runs' multiplicities
// under `op` (SetOp), *total = off[n_runs] = the output rows.  tile_m [t], tile_mbase [t + 1], t = ceil(n_runs / SETOP_TILE): scratch.
void launch_setop_offsets(const Launch& L, const SetopRuns& runs, uint32_t n_runs, int op, uint32_t* tile_m, uint32_t* tile_mbase,
                          uint32_t* off, uint32_t* total, uint32_t max_grid);
// run_of[j] = the run output row j is a copy of, j < n_out = off[n_runs]
void launch_setop_emit(const Launch& L, const uint32_t* off, uint32_t n_runs, uint32_t n_out, uint32_t* run_of, uint32_t max_grid);

// ================================================================================================== rj_varchar_dev.hip
// ---- VARCHAR gather + page encode on the device (replaces, for large results, the string half
//      of Table::to_columnar, reference src/build_table.cpp:595-677)
void launch_vc_resolve(const Launch& L, const uint8_t* pages, uint32_t n_pages, const uint32_t* row_base,
                       const uint32_t* rowids, uint32_t n, VcRow* out);
// VARCHAR join keys: 64-bit FNV-1a of every row's string (+ where it sits, + validity), the
// byte-for-byte check of the joined pairs, and the compaction that only a hash collision triggers
void launch_vc_hash(const Launch& L, const uint8_t* pages, uint32_t n_pages, const uint32_t* row_base,
                    const uint32_t* rowids, uint32_t n, VcRow* rows, uint64_t* hash, uint8_t* valid,
                    uint64_t hash_mask = ~0ull);
void launch_vc_verify(const Launch& L, const uint8_t* pages_b, uint32_t np_b, const VcRow* rows_b,
                      const uint8_t* pages_p, uint32_t np_p, const VcRow* rows_p, const uint32_t* bidx,
                      const uint32_t* pidx, uint32_t n, uint8_t* keep, unsigned long long* n_bad);
void launch_vc_compact(const Launch& L, const uint8_t* keep, const uint32_t* bidx, const uint32_t* pidx, uint32_t n,
                       uint32_t* out_b, uint32_t* out_p, unsigned long long* cursor);
// page_out == nullptr: pages_in_chunk[c] = pages of chunk c; else the pages are written to
// page_out[page_base[c] ...]
void launch_vc_walk(const Launch& L, const VcRow* rows, uint32_t n, uint32_t* pages_in_chunk,
                    const uint32_t* page_base, VcPage* page_out);
void launch_vc_encode(const Launch& L, const uint8_t* pages, uint32_t n_pages, const VcRow* rows,
                      const VcPage* plist, uint32_t n_out_pages, uint8_t* out);

// ---- RJ_CTX_PREWARM: one launch per kernel file of the join path and of rj_varchar_dev.hip, whose threads leave at
// the kernel's first bounds check: HIP loads a file's code object on the first use of one of its kernels.  One
// signature for all (Context::prewarm walks an array of them); zeroed: 256 zero bytes on the device.
void prewarm_pages(const Launch& L, uint32_t* zeroed);
void prewarm_partition(const Launch& L, uint32_t* zeroed);
void prewarm_join(const Launch& L, uint32_t* zeroed);
void prewarm_bcast(const Launch& L, uint32_t* zeroed);
void prewarm_filter(const Launch& L, uint32_t* zeroed);
void prewarm_outer(const Launch& L, uint32_t* zeroed);
void prewarm_full(const Launch& L, uint32_t* zeroed);
void prewarm_agg(const Launch& L, uint32_t* zeroed);
void prewarm_select(const Launch& L, uint32_t* zeroed);
void prewarm_varchar_dev(const Launch& L, uint32_t* zeroed);

}  // namespace rj
