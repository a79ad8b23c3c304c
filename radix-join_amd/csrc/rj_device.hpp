// rj_device.hpp — POD structs and tuning constants shared by the host executor
// and the gfx950 kernels.  Everything here is written for MI355X only: wave64,
// 160 KiB LDS per CU, 256 CUs in 8 XCDs.
#pragma once
#include <stdint.h>

namespace rj {

// ---- Page geometry (reference include/plan.h:54, src/build_table.cpp:488,531)
constexpr uint32_t PAGE_BYTES = 8192;
constexpr uint32_t ROWS32 = 1984;  // rows of a full non-NULL INT32 page
constexpr uint32_t ROWS64 = 1007;  // rows of a full non-NULL INT64/FP64 page
constexpr uint32_t HDR32 = 4;      // first value offset, INT32
constexpr uint32_t HDR64 = 8;      // first value offset, INT64/FP64

// ---- Columns as the kernels see them
enum ColKind : int32_t {
    COL_NONE  = 0,
    COL_PAGED = 1,  // "regular" page images: every page but the last holds ROWS32/ROWS64
                    // non-NULL values, so row r lives at page r / ROWS, slot r % ROWS
    COL_DENSE = 2,  // flat array of 4- or 8-byte values (+ optional validity bytes)
    COL_IOTA  = 3   // value(row) = row: the row-id column of a base table (late
                    // materialisation of VARCHAR)
};

struct ColRef {
    const uint8_t* ptr;
    const uint8_t* valid;  // COL_DENSE only; nullptr = all rows valid
    int32_t        kind;
    int32_t        width;  // 4 or 8
};

// What travels with the key through the radix passes.
enum CarryMode : int32_t {
    CARRY_NONE   = 0,
    CARRY_ROWIDX = 1,  // row index into the child relation (generic path: gather later)
    CARRY_COLUMN = 2,  // the single payload column itself (direct path: no gather)
    CARRY_WIDE   = 3   // several payload columns (and/or a validity word) packed into 2 or 3 carry
                       // words, see TupleSrc::wide: the values themselves travel, nothing is
                       // gathered afterwards and nothing refers to a row of this rank
};

// Layout of a wide carry.  The executor orders the carried columns so that two loaders suffice:
enum WideLayout : int32_t {
    WIDE_NONE = 0,  // one column (carry), 32 or 64 bits
    WIDE_32S  = 1,  // two or three 32-bit columns: carry, carry2 [, carry3]
    WIDE_64_32 = 2  // a 64-bit column (carry) followed by a 32-bit one (carry2)
};

struct TupleSrc {
    ColRef   key;
    ColRef   carry;
    uint32_t n_rows;
    int32_t  carry_mode;
    int32_t  key_f64;    // FP64 key: compared by bit pattern, NaN never matches
    int32_t  prehashed;  // key column already holds hashed keys (sharded stage B)
    int32_t  wide;       // WideLayout (CARRY_WIDE)
    int32_t  pad;
    ColRef   carry2, carry3;  // further columns of a wide carry
};

// Partitioned tuples are SoA arrays of 32-bit words (or, for one key word + one carry word in
// fine-histogram plans, ONE array of 8-byte {word 0, carry} pairs — "packed"):
//   word 0            = hashed key (low 32 bits); radix digits and slot bits come from it
//   word 1 (KW == 2)  = high 32 bits of the 64-bit hashed key
//   following words   = carry (0, 1 or 2 words)
constexpr int MAX_WORDS = 4;
struct Words {
    uint32_t* w[MAX_WORDS];
};

// ---- Radix partition pass --------------------------------------------------
// One workgroup sorts a tile of PT_TILE tuples by digit in LDS and writes each
// digit's run contiguously (software write-combining), see rj_partition.hip.
// Geometry is overridable at build time (-DRJ_PT_THREADS=...) for tuning runs.
#ifndef RJ_PT_THREADS
#define RJ_PT_THREADS 1024
#endif
#ifndef RJ_PT_ITEMS
#define RJ_PT_ITEMS 16
#endif
constexpr int PT_THREADS = RJ_PT_THREADS;         // waves = PT_THREADS / 64
constexpr int PT_ITEMS   = RJ_PT_ITEMS;           // tuples per thread per tile
constexpr int PT_TILE    = PT_THREADS * PT_ITEMS; // 16384 tuples = 64 KiB of LDS staging; longer
                                                  // digit runs per tile = fewer partial HBM lines
constexpr uint32_t PT_ALL_ITEMS = PT_ITEMS >= 32 ? 0xffffffffu : ((1u << (PT_ITEMS & 31)) - 1u);  // one bit per item
// what the kernels can fan out per pass; -DRJ_PT_CAPBITS=10 builds the 1024-digit variant that
// RJ_TUNE_P1_BITS=8 / 10 needs to cut 18 bits 8+10 / 10+8 (profiles/r03_r_bits_8_10_ab.log: no gain)
#ifndef RJ_PT_CAPBITS
#define RJ_PT_CAPBITS 9
#endif
constexpr int PT_CAPBITS = RJ_PT_CAPBITS;
constexpr int PT_MAXF    = 1 << PT_CAPBITS;
constexpr int PT_MAXBITS = 9;                     // what the bit plans use per pass (512 digits: runs of 32 tuples per tile)
static_assert(PT_CAPBITS >= PT_MAXBITS && PT_CAPBITS <= 10, "fan-out capacity");
constexpr int PT_FINEBITS = 15;                   // fine (two-digit) histogram: 2^15 bins = 128 KiB of LDS
constexpr int LDS_BYTES  = 160 * 1024;            // per CU (and the most one workgroup may declare)
static_assert(PT_THREADS >= PT_MAXF, "thread d scans digit d");
// Dummy rank counters behind the real ones (s_cnt[PT_MAXF + lane % PT_DUMMY]): where the scatter's
// branch-free ranking sends the items that hold no tuple.  Never cleared, scanned or read.
constexpr int PT_DUMMY   = 32;
// static LDS of the partition kernels: staging tile of 8-byte pairs + three digit arrays + dummy counters + wave sums
static_assert(PT_TILE * 8 + (3 * PT_MAXF + PT_DUMMY) * 4 + (PT_THREADS / 64) * 4 <= LDS_BYTES,
              "scatter tile does not fit the 160 KiB of LDS");
static_assert((4 << PT_FINEBITS) <= LDS_BYTES, "fine histogram does not fit the LDS");
// a rank (< PT_TILE) is kept in PT_RANK_MASK's bits, two ranks or two LDS positions (< PT_TILE; 0xffff
// for an item without a tuple) per register
constexpr uint32_t PT_RANK_MASK = PT_TILE <= 16384 ? 0x3fffu : 0x7fffu;
static_assert(PT_TILE <= 32768 && PT_ITEMS % 2 == 0, "ranks and LDS positions are packed two per register");
static_assert(PT_ITEMS % 4 == 0 && PT_ITEMS <= 32, "full tiles are loaded as 16-byte vectors; one mask bit per item");

struct PassParams {
    const uint32_t* seg_off;    // [nseg+1] input segments (previous pass' partitions);
                                // nullptr = one segment [0, n)
    const uint32_t* grp_start;  // [nseg+1] exclusive scan of groups per segment (nseg > 1)
    uint32_t        nseg;
    uint32_t        n;          // tuples (single-segment case)
    uint32_t        shift;      // digit = (word0 >> shift) & (F-1)
    uint32_t        fanout_log2;
    uint32_t        tiles_per_group;
    uint32_t*       hist;       // [nseg*F << xcd_log2]  global bin totals
    uint32_t*       cursor;     // [nseg*F << xcd_log2]  write cursors (start = exclusive scan of hist)
    // 3: every partition's range is cut into 8 sub-ranges, one per XCD (workgroup g counts and
    // writes into sub-range g & 7 — workgroups go round-robin over the XCDs), so that the runs
    // next to each other in memory were written through the SAME L2, which can then complete
    // the lines they share before writing them back; 0: one range per partition
    uint32_t        xcd_log2;
    // passes over several segments: workgroup b takes group (b & 7) * ceil(G / 8) + (b >> 3), i.e.
    // every XCD walks its own contiguous eighth of the groups — the workgroups that write into
    // one segment's partitions at the same time then share an L2
    uint32_t        xcd_remap;
    // 12-byte-tuple passes that are not the last one also write the NEXT pass' digit of every
    // tuple as a 16-bit side array (same index as the tuple), so that the next histogram reads
    // 2 bytes per tuple instead of fishing 4-byte keys out of 12-byte tuples; nullptr = none
    uint16_t*       side_out;
    uint32_t        next_shift, next_mask;
    // Input segments that do not lie one behind the other (what a rank holds after the exchange
    // of a sharded join: one run per (source rank, local digit), listed digit-major): segment s
    // is [seg_off[s], seg_end[s]); nullptr = [seg_off[s], seg_off[s + 1])
    const uint32_t* seg_end;
    // ... and several input segments may feed ONE output segment (all runs of a local digit):
    // input segment s belongs to output segment s >> oseg_shift, whose bins / cursors it uses
    uint32_t        oseg_shift;
    // a launch over a sub-range of the segments (a later pass run chunk by chunk): grp_start points at the
    // sub-range's first entry of the table of ALL segments, whose group numbers start at grp_base
    uint32_t        grp_base;
    // Composite digit (stage A of a sharded join: owner rank from the TOP hash bits, first local
    // digit from the LOW ones, one pass for both): hi_shift != 0 =>
    //   digit = ((w >> shift) & ((1 << lo_bits) - 1)) | ((w >> hi_shift) << lo_bits)
    uint32_t        hi_shift, lo_bits;
};

// digit of hashed key word `w` in this pass (mask = fan-out - 1)
__host__ __device__ inline uint32_t pass_digit(const PassParams& pp, uint32_t w, uint32_t mask) {
    if (pp.hi_shift) return (((w >> pp.shift) & ((1u << pp.lo_bits) - 1u)) | ((w >> pp.hi_shift) << pp.lo_bits)) & mask;
    return (w >> pp.shift) & mask;
}

// ---- Speculative first pass (no histogram: DESIGN.md §4) ---------------------------------------
// The first pass of a big two-pass plan sizes the 2^fanout_log2 * 8 output sub-ranges from a SAMPLE
// of the keys instead of counting them all: sub-range i gets cap[i] tuples of room (k_spec_caps), the
// scatter checks the room in the reservation itself, and a sub-range that turns out too small sends
// the whole radix_partition() call back to the exact histogram path.  The speculative kernels take these
// parameters as an argument of their own: PassParams, and with it every kernel of the exact path,
// stays as it is.
constexpr uint32_t SPEC_BINS = (1u << PT_MAXBITS) * 8u;  // sub-ranges of a 9-bit first pass: 4096
struct SpecParams {
    // one 64-bit word per sub-range: {next free position : low 32, tuples of room left : high 32}.
    // A tile reserves c tuples with ONE atomic add of c | (0 - c) << 32; what comes back holds where
    // the run starts and whether it fits (room >= c, compared as signed numbers: the room of a
    // sub-range that overflowed goes negative and stays so)
    unsigned long long* cursor;
    uint32_t*           flag;        // OR 1: some reservation did not fit, the output is to be thrown away
    uint32_t            sink;        // first tuple of the PT_TILE spare tuples behind the sub-ranges: where
                                     // a run that did not fit is written (sink + its offset inside the tile)
    uint32_t            sample_log2; // k_pass_sample: PT_TILE >> sample_log2 rows of every tile are counted
};
// ---- Speculative LAST pass of a two-pass inner join (no second histogram: DESIGN.md §4) ---------
// The same estimate / check / repeat, one level down: the final partitions (up to 2^18 of them) get their room
// from a sample of the first pass' output (k_last_sample, k_last_caps), the scatter (k_last_scatter*) reserves
// from one cursor per final partition (xcd_log2 = 0) and checks the run's end against the partition's limit, and
// k_last_close leaves end[q] = min(position, limit[q]) next to begin[q] ({begin, end} pairs: JoinParams::off_pairs):
// the join reads [begin[q], end[q]) and never the room behind it.  (A 32-bit cursor and a limit array instead of SpecParams' {position, room} words: the scatter keeps
// a group's limits in the LDS and, per digit thread, the registers of the exact kernel.  The fields the shared
// scatter bodies name in their first-pass branch are here too, unused.)
struct LastParams {
    unsigned long long* cursor;      // NEVER READ OR SET.  It is here only because the shared bodies' first-pass branch,
                                     // `res = atomicAdd(&sp.cursor[at], ...)` (rj_pass_scatter.inc and
                                     // rj_pass_scatter_packed.inc, the `else if constexpr (SPEC)` arm of the reservation),
                                     // is discarded in the k_last_* kernels but must still be well-formed with this struct
    uint32_t*           flag;        // OR 1: some run did not fit, the output is to be thrown away
    uint32_t            sink;        // first tuple of the PT_TILE spare tuples behind the partitions
    uint32_t            sample_log2; // k_last_sample: PT_TILE >> sample_log2 keys of every tile are counted
    uint32_t*           cursor32;    // [bins] next free position of final partition (oseg, d2)
    const uint32_t*     limit;       // [bins] begin + capacity
};

// ---- Build/probe -------------------------------------------------------------
#ifndef RJ_JN_THREADS
#define RJ_JN_THREADS 512
#endif
#ifndef RJ_JN_SPT
#define RJ_JN_SPT 8
#endif
#ifndef RJ_JN_CAP
#define RJ_JN_CAP 8192
#endif
constexpr int      JN_THREADS = RJ_JN_THREADS;
constexpr int      JN_SPT     = RJ_JN_SPT;             // probe tuples per thread per sub-chunk
constexpr int      JN_SUB     = JN_THREADS * JN_SPT;   // probe tuples per output reservation
constexpr int      JN_CAP     = RJ_JN_CAP;             // LDS table slots (power of two)
constexpr int      JN_RMAX    = JN_CAP / 2;            // build tuples per table (load <= 50 %)
constexpr int      JN_RPT     = (JN_RMAX + JN_THREADS - 1) / JN_THREADS;  // build tuples per thread
// Threads of a join workgroup: tables of 3+ word arrays only fit once per CU, that one workgroup
// then brings all 16 waves itself.
constexpr int jn_threads(int table_words) { return table_words >= 3 ? 2 * JN_THREADS : JN_THREADS; }
// __launch_bounds__ "waves per SIMD" for the join: as many workgroups per CU as the LDS
// table (table_words arrays of JN_CAP words) allows, times threads / 256, capped at 8
constexpr int jn_min_waves(int table_words) {
    int blocks = (160 * 1024) / (JN_CAP * 4 * table_words + JN_CAP + 1024);
    int w = blocks * jn_threads(table_words) / 256;
    return w > 8 ? 8 : (w < 1 ? 1 : w);
}
static_assert(JN_RPT % 4 == 0 && JN_SPT % 4 == 0, "tuples are loaded as 16-byte vectors");
static_assert(JN_CAP * 4 * 4 + JN_CAP + 1024 <= 160 * 1024, "a four-array join table does not fit the LDS");
#ifndef RJ_JN_PPW
#define RJ_JN_PPW 1
#endif
#ifndef RJ_JN_PPW3
#define RJ_JN_PPW3 4
#endif
// Partitions per workgroup: the next partition's loads are issued behind the current one's
// probe (software pipeline).  Tables of two word arrays run two workgroups per CU, whose phases
// overlap by themselves (pipelining them only spilled); tables of 3+ arrays run ONE 1024-thread
// workgroup per CU, which would otherwise serialise load latency, build, probe and emit.
constexpr int jn_ppw(int table_words) { return table_words >= 3 ? RJ_JN_PPW3 : RJ_JN_PPW; }
#ifndef RJ_JN_HEAVY
#define RJ_JN_HEAVY 65536  // (16 K / 32 K / 64 K / 128 K at 1 B rows, Zipf 0.9: join 9.30 / 9.16 / 9.03 / 9.11 ms — profiles/r03_v_*)
#endif
constexpr uint32_t JN_HEAVY   = RJ_JN_HEAVY;           // probe tuples per task before splitting
constexpr uint32_t JN_TARGET_BUILD = JN_RMAX * 3 / 4;  // mean build tuples per final partition

enum StreamMode : int32_t {
    ST_NONE    = 0,
    ST_DENSE32 = 1,
    ST_DENSE64 = 2,
    ST_PAGED32 = 3,  // page images, ROWS32 per page, values from +4
    ST_PAGED64 = 4,  // page images, ROWS64 per page, values from +8
    ST_DENSE96 = 5   // 12-byte records (a three-word wide carry; two-word ones use ST_DENSE64)
};

struct OutStream {
    uint8_t* base;
    int32_t  mode;
    int32_t  pad;
};

struct JoinParams {
    Words           R, S;
    const uint32_t* offR;   // [NP+1] neighbouring offsets, or [2 NP] {begin, end} pairs: see off_pairs
    const uint32_t* offS;   // (the same)
    uint32_t        NP;
    uint32_t        radix_bits;  // low bits of word 0 shared by a partition's tuples
    uint32_t        n_pass;      // radix passes and their bit widths: partition index
    uint32_t        pass_bits[4]; //   q = ((d1 * F2) + d2) * F3 + d3, hash low bits = d1 | d2 << b1 | ...
    OutStream       key, bc, pc; // emitted streams: key, build carry, probe carry
    unsigned long long* out_cursor;
    uint64_t        out_cap;     // rows that fit the stream buffers
    const uint32_t* heavy_tasks; // [n][3] = {partition, s_begin, s_end}
    const uint32_t* n_heavy;
    uint32_t        heavy_grid;  // the first heavy_grid workgroups of the launch take heavy tasks
    int32_t         packR, packS; // R.w[0] / S.w[0] is an array of {hashed key, carry} pairs
    int32_t         aosR, aosS;   // R.w[0] / S.w[0] is an array of 12-byte {hashed key, carry lo, carry hi}
    // Partition q holds tuples [off[q << sh], off[(q << sh) + 1]).  sh = 0: exact partitions, one behind the other
    // (off[NP + 1]).  sh = 1: a speculative last pass (LastParams) left unused room behind each partition and
    // off[2 NP] holds {begin, end} pairs.  Bit 0: offR's sh, bit 1: offS's (a side that fell back is exact again)
    uint32_t        off_pairs;
    unsigned long long* diag;    // phase cycle counters (RJ_DIAG=1 only), else nullptr
};

// ---- wide carries: the records a join emits for one side -> its columns (k_split_records)
struct SplitParams {
    const uint32_t* rec;         // cw words per output row
    uint32_t        cw;
    int32_t         n_cols;
    int32_t         valid_word;  // word of the record that holds the validity bits, -1 = none
    int32_t         pad;
    struct Col {
        uint8_t* out;            // dense values
        uint8_t* valid;          // validity bytes, nullptr = the column has no NULLs
        int32_t  word;           // first word of the column inside the record
        int32_t  width;          // 4 or 8
        int32_t  valid_bit;
        int32_t  paged;          // 1: `out` is a run of Page images (values at their slot), 0: a dense array
    } col[3];
};

// ---- VARCHAR materialisation on the device (rj_varchar_dev.hip) ----------------------------
struct VcRow {
    uint32_t page;  // source page index (first page of a long string's chain)
    uint32_t beg;   // byte offset of the first character inside the page; 0xffffffff = long string
    uint32_t len;   // characters; 0xffffffff = NULL
};
struct VcPage {
    uint32_t first;  // first result row of the page (the row itself for long-string pieces)
    uint32_t nr;     // rows of a normal page
    uint32_t kind;   // 0 = normal page, 1 + k = piece k of a long string
};
constexpr uint32_t VC_CHUNK = 512;  // result rows per fill-rule chunk (one lane walks one chunk)

// ---- Broadcast join (build side fits ONE LDS table): no partitioning at all --------------
struct BcastParams {
    TupleSrc        R, S;        // build / probe tuples straight from the child columns
    OutStream       key, bc, pc; // emitted streams: key, build carry, probe carry
    unsigned long long* out_cursor;
    uint64_t        out_cap;
};

// ---- Semi / anti joins (RJ_NODE_SEMI / RJ_NODE_ANTI): "has this preserved row a partner?" ------
// The filter side builds an LDS set of its DISTINCT hashed keys; the preserved side is probed and
// the rows that hit (SEMI) or miss (ANTI) are emitted once each: the un-hashed key (if requested)
// and the preserved carry.  The set holds JN_RMAX keys at most (load <= 50 %); a partition with
// more distinct filter keys is filtered round by round (k_filter_join).
struct FilterParams {
    TupleSrc        F, P;         // broadcast: filter / preserved tuples straight from the columns;
                                  // k_filter_nullkeys: P
    Words           Fw, Pw;       // partitioned: filter key words / preserved tuples
    const uint32_t* offF;         // [NP+1]
    const uint32_t* offP;         // [NP+1]
    uint32_t        NP;
    uint32_t        radix_bits;
    int32_t         packP, aosP;  // Pw.w[0] holds {hashed key, carry} pairs / 12-byte tuples
    const uint32_t* heavy_tasks;  // [n][3] = {partition, p_begin, p_end} (k_heavy_tasks)
    const uint32_t* n_heavy;
    uint32_t        heavy_grid;   // the first heavy_grid workgroups of the launch take heavy tasks
    int32_t         anti;         // 0: SEMI (emit hits), 1: ANTI (emit misses)
    int32_t         keyless;      // 1: the key types differ, no row can match (keys are not read)
    int32_t         pad;
    OutStream       key, pc;      // emitted streams: key, preserved carry
    unsigned long long* out_cursor;
    uint64_t        out_cap;      // rows that fit the streams (= preserved rows)
};

// ---- Outer joins (RJ_NODE_OUTER): the inner join's rows plus every preserved row without a
// partner, once, with NULL in the optional (build) side's columns.  "NULL" travels in-band in the
// build carry stream: the reserved row id OUTER_NO_ROW for a CARRY_ROWIDX optional side, an
// all-zero record (validity word included, which such a carry always has) for a CARRY_WIDE one;
// CARRY_COLUMN is not used for an optional side.  `pad_bc` is the first word of a padded row's
// build carry, the other words are zero.
constexpr uint32_t OUTER_NO_ROW = 0xffffffffu;
struct OuterParams {
    TupleSrc        B, P;         // broadcast: optional / preserved tuples straight from the columns;
                                  // k_outer_nullkeys: P
    Words           Bw, Pw;       // partitioned: optional / preserved tuples
    const uint32_t* offB;         // [NP+1]
    const uint32_t* offP;         // [NP+1]
    uint32_t        NP;
    uint32_t        radix_bits;
    int32_t         packB, aosB;  // Bw.w[0] holds {hashed key, carry} pairs / 12-byte tuples
    int32_t         packP, aosP;  // ... and Pw.w[0]
    const uint32_t* heavy_tasks;  // [n][3] = {partition, p_begin, p_end} (k_heavy_tasks)
    const uint32_t* n_heavy;
    uint32_t        heavy_grid;   // the first heavy_grid workgroups of the launch take heavy tasks
    int32_t         keyless;      // 1: the key types differ, no row can match (keys are not read)
    uint32_t        pad_bc;       // OUTER_NO_ROW (row-index carry) or 0 (wide carry)
    int32_t         pad;
    OutStream       key, bc, pc;  // emitted streams: preserved key, optional carry, preserved carry
    unsigned long long* out_cursor;
    uint64_t        out_cap;      // rows that fit the streams; rows beyond are counted, not written
};

// ---- Full outer joins (RJ_NODE_FULL): an outer join's rows plus every BUILD row without a partner,
// once, with NULL in the probed side's columns.  Both carries follow the optional rules above
// (`pad_pc` is to the probed carry what OuterParams::pad_bc is to the build carry) and no key
// stream is written.  `flags` holds one "matched" bit per build tuple (bit i = tuple i of the
// partitioned build arrays, or row i of the built child on the broadcast path), zeroed once per
// node; the probe kernels OR their matches in, the kernels launched after them emit the tuples
// whose bit stayed clear.
struct FullParams {
    OuterParams     o;
    uint32_t*       flags;
    uint32_t        pad_pc;       // OUTER_NO_ROW (row-index carry) or 0 (wide carry)
    int32_t         use_flags;    // k_full_buildrows: 1 = also emit the rows whose flag is clear (broadcast)
};

// ---- Aggregation (RJ_NODE_AGG): GROUP BY the key, COUNT / SUM / MIN / MAX over the carried columns.
// ONE relation is partitioned; a workgroup aggregates a partition (or a heavy task of one) in an
// LDS table of AGG_CAP entries {hashed key, rows, per carried column: non-NULL count, sum, min,
// max}.  New keys enter the table until it holds AGG_FREEZE of them at the end of a step; from then
// on tuples of keys that are not in it are put back into the partition's own memory, behind the
// read position, for the next round (k_agg_parts).
constexpr int AGG_THREADS = 512;
constexpr int AGG_SPT     = 2;                      // tuples per thread per step
constexpr int AGG_STEP    = AGG_THREADS * AGG_SPT;  // tuples between two looks at the table's fill
constexpr int AGG_CAP     = 1024;                   // LDS table entries (power of two)
constexpr int AGG_FREEZE  = AGG_CAP * 5 / 8;        // no new keys once this many are in
constexpr int AGG_WALK    = 32;                     // entries a key may sit away from its home: a walk that
                                                    // finds them all taken by other keys turns the tuple away
constexpr uint32_t AGG_TARGET = AGG_CAP * 3 / 8;    // mean tuples (an upper bound of the groups) per partition
constexpr int AGG_MAX_COLS = 3;
static_assert((AGG_CAP & (AGG_CAP - 1)) == 0 && AGG_CAP % AGG_THREADS == 0, "table entries: a power of two, whole rows of threads");
static_assert(AGG_CAP * (12 + 28 * AGG_MAX_COLS) + 1024 <= LDS_BYTES, "the widest aggregation table does not fit the LDS");

enum AggNeed : uint32_t { AGG_NEED_COUNT = 1, AGG_NEED_SUM = 2, AGG_NEED_MIN = 4, AGG_NEED_MAX = 8 };
struct AggCol {
    int32_t  word;       // first word of the column inside the carry
    int32_t  width;      // 4 or 8 bytes; 32-bit values are sign-extended
    int32_t  valid_bit;  // bit of the validity word, -1 = the column has no NULLs
    uint32_t need;       // AggNeed bits: the accumulators some output reads
};
// One group's accumulators as arrays: the merge table in HBM (entry index) and the node's output
// (row index) share the layout.  key: KW * 4 bytes per entry in the output (un-hashed), always 8
// in the merge table (hashed).  Arrays nobody reads are nullptr (output only).
struct AggArrays {
    uint8_t*            key;
    unsigned long long* rows;
    unsigned long long* nn[AGG_MAX_COLS];
    unsigned long long* sum[AGG_MAX_COLS];
    long long*          mn[AGG_MAX_COLS];
    long long*          mx[AGG_MAX_COLS];
};
constexpr unsigned long long AGG_NO_KEY = ~0ull;  // merge table: an entry nobody owns yet
struct AggParams {
    TupleSrc        src;          // k_agg_nullkey: the child's columns
    Words           W;            // the partitioned tuples
    const uint32_t* off;          // [NP+1]
    uint32_t        NP;
    int32_t         pack, aos;    // W.w[0] holds {hashed key, carry} pairs / 12-byte tuples
    const uint32_t* heavy_tasks;  // [n][3] = {partition, begin, end} (k_heavy_tasks)
    const uint32_t* n_heavy;
    uint32_t        heavy_grid;   // the first heavy_grid workgroups of k_agg_parts take heavy tasks
    int32_t         n_cols;
    int32_t         valid_word;   // word of the carry that holds the validity bits, -1 = none
    AggCol          col[AGG_MAX_COLS];
    AggArrays       out;          // one row per group, out_cap rows
    uint8_t*        out_keyvalid; // validity bytes of the key column, preset to 1; nullptr = the key has no NULLs
    unsigned long long* out_cursor;
    uint64_t        out_cap;
    // merge table (heavy tasks, NULL-key rows): m_slots entries of open addressing (a power of two,
    // or 0), then entry m_slots for the hashed key AGG_NO_KEY itself and entry m_slots + 1 for the
    // NULL-key group; an entry is live when its `rows` is not 0
    AggArrays       m;
    uint32_t        m_slots;
    uint32_t*       m_overflow;   // set when a key found no entry: the host repeats the node with a larger table
};

// ---- Selection (RJ_NODE_SELECT): a postfix predicate program over a relation's columns; the row ids
// of the rows it keeps are compacted into one array (k_select), which the output columns are then
// gathered through.  A workgroup owns tiles of SEL_TILE consecutive rows: wave w of it evaluates rows
// [w * SEL_TILE / 4, (w + 1) * SEL_TILE / 4) of the tile, 64 consecutive ones per item.
constexpr int SEL_THREADS = 256;
constexpr int SEL_TILE = 8192;                        // rows per output reservation (one global atomic)
constexpr int SEL_ITEMS = SEL_TILE / SEL_THREADS;     // rows per thread per tile
constexpr int SEL_BATCH = 4;                          // ... of which a thread evaluates this many together
constexpr int SEL_MAX_OPS = 64;
static_assert(SEL_TILE % 256 == 0 && SEL_TILE % SEL_THREADS == 0 && SEL_ITEMS <= 32 && SEL_ITEMS % SEL_BATCH == 0,
              "whole rows of threads; one keep bit per item; whole batches");

enum SelKind : int32_t {
    SEL_LIT = 0,      // column a <cmp> literal
    SEL_COL = 1,      // column a <cmp> column b
    SEL_IS_NULL = 2,
    SEL_NOT_NULL = 3,
    SEL_AND = 4,
    SEL_OR = 5,
    SEL_NOT = 6
};
struct SelectOp {
    int32_t kind;    // SelKind
    int32_t cmp;     // 0..5 = EQ, NEQ, LT, GT, LEQ, GEQ (the order of rj_filter_opcode)
    int32_t f64;     // the operands are doubles (compared IEEE-wise), else integers of a.width bytes
    int32_t pad;
    int64_t literal; // SEL_LIT: the literal (an INT32 column's already cut to 32 bits and sign-extended; FP64: the bits)
    ColRef  a, b;
};
// One small device buffer per node; every thread reads ops[k] at the same k, so the loads are scalar.
struct SelectProg {
    SelectOp ops[SEL_MAX_OPS];
};

// ---- Sort (RJ_NODE_SORT): a stable LSD radix sort of {encoded key, row id} pairs, one key column at
// a time from the last to the first, 8 bits per pass.  A workgroup owns one tile of SORT_TILE
// consecutive rows: wave w of it holds rows [w * SORT_TILE / 4, (w + 1) * SORT_TILE / 4) of the tile,
// 64 consecutive ones per item, so that "earlier row" is (wave, item, lane) order.
constexpr int SORT_THREADS = 256;
constexpr int SORT_TILE = 4096;                          // rows per workgroup and per column of the tile x digit table
constexpr int SORT_ITEMS = SORT_TILE / SORT_THREADS;     // rows per thread
constexpr int SORT_RADIX = 256;                          // bins per pass
constexpr int SORT_NULL_DIGIT = 8;                       // row of the histogram that counts the NULL flag (bins 0 and 1)
constexpr int SORT_HIST_WORDS = (SORT_NULL_DIGIT + 1) * SORT_RADIX;  // per key column: [digit position][bin]
constexpr int SORT_MAX_KEYS = 8;                         // RJ_SORT_MAX_KEYS
static_assert(SORT_THREADS == SORT_RADIX && SORT_TILE % SORT_THREADS == 0 && SORT_TILE <= 65536,
              "thread d owns bin d; whole rows of threads; ranks inside a tile are 16 bits");
// what a pass takes its digit from
enum SortMode : int32_t {
    SORT_KEY32 = 0,  // (key >> shift) & 255 of 32-bit keys
    SORT_KEY64 = 1,  // ... of 64-bit keys
    SORT_FLAG = 2    // the NULL flag of the row the id names (no keys travel: the column's last pass)
};

// ---- Grouping (RJ_NODE_GROUP): the rows ordered by the sort above, then cut into runs of equal keys.
// The geometry is the sort's: a tile is GROUP_TILE consecutive positions of the sorted order, wave w
// of a workgroup holds positions [w * GROUP_TILE / 4, (w + 1) * GROUP_TILE / 4) of it, 64 consecutive
// ones per item, so that "previous row" is (wave, item, lane) order.  One 64-bit head mask per item
// (bit l: position 64 * item + l starts a group); a position's group is the number of heads up to it.
constexpr int GROUP_THREADS = 256;
constexpr int GROUP_TILE = 4096;                            // positions per tile
constexpr int GROUP_WAVES = GROUP_THREADS / 64;
constexpr int GROUP_ITEMS = GROUP_TILE / GROUP_THREADS;     // items of 64 positions per wave
static_assert(GROUP_TILE % GROUP_THREADS == 0 && GROUP_ITEMS <= 64, "whole items; a wave's masks sit in one lane each");

// The accumulator arrays of one k_group_reduce launch, one entry per group; nullptr = not wanted.
// mn / mx hold the ENCODED value (sort_key_bits, ascending), so that they compare as unsigned numbers.
struct GroupAcc {
    unsigned long long* rows;  // COUNT(*)
    unsigned long long* nn;    // non-NULL values of the column
    unsigned long long* sum;   // their sum, wrapping
    unsigned long long* mn;
    unsigned long long* mx;
};
// how k_group_column turns an accumulator into a result column
enum GroupDecode : int32_t { GROUP_RAW = 0, GROUP_KEY32 = 1, GROUP_KEY64 = 2, GROUP_KEYF64 = 3 };

// ---- Window functions (RJ_NODE_WINDOW): the rows ordered by (partition keys, order keys) as above, and
// TWO head masks in the grouping's layout: P marks where the partitions begin, Q (a superset) where
// the peer groups begin.  The kernels work QUARTER by quarter — the positions of one wave of a tile,
// WIN_ITEMS mask words — and no wave waits for another: what a quarter needs from outside is one entry
// per quarter, computed by a launch of its own (rj_window.hip).
constexpr int WIN_QUARTER = GROUP_TILE / GROUP_WAVES;  // positions per wave
constexpr int WIN_ITEMS = GROUP_ITEMS;                 // items of 64 positions per quarter
constexpr int WIN_CARRY_THREADS = 1024;                // threads of the one workgroup that scans the quarters' entries
static_assert(WIN_QUARTER == 64 * WIN_ITEMS && WIN_ITEMS <= 64, "a quarter's masks sit in one lane each");

// One entry per quarter.  k_win_marks writes the quarter's own summary, k_win_carry turns it in place
// into what the quarter needs from outside (positions as 1 + position, 0 = none):
struct WinMarks {
    uint32_t* last_p;  // the quarter's last P head          -> the last P head in front of the quarter
    uint32_t* last_q;  // ... last Q head                     -> the last Q head in front of the quarter
    uint32_t* dense;   // Q heads at or behind its last P head (all, if it has none) -> ... in front of the quarter
    uint32_t* next_q;  // position of its first Q head, n_rows = none -> of the first Q head behind the quarter
};
// What k_win_ranks writes, one entry per position of the order; nullptr = not wanted.
struct WinRanks {
    unsigned long long* row_number;
    unsigned long long* rank;
    unsigned long long* dense_rank;
    unsigned long long* count_star;  // rows of the frame
    uint32_t*           peer_end;    // position of the row's last peer: where its frame ends
};
// One entry per quarter: k_win_tails writes the accumulators of the quarter's positions from its last
// P head on (head = 1 if it has one), k_win_tail_carry turns them in place into the quarter's carry-in.
struct WinTails {
    uint32_t*           head;
    uint32_t*           nn;
    unsigned long long* sum;
    unsigned long long* mn;
    unsigned long long* mx;
};
// The segmented inclusive scan of one value column, one entry per position; nullptr = not wanted.
struct WinScan {
    uint32_t*           nn;
    unsigned long long* sum;
    unsigned long long* mn;
    unsigned long long* mx;
};

// ---- ROWS frames, LAG / LEAD / FIRST_VALUE / LAST_VALUE and NTILE of RJ_NODE_WINDOW (rj_frame.hip): every
// position knows its partition [ps, pe] from a k_win_ranks launch with Q := P (ROW_NUMBER gives ps,
// the peer end gives pe); a frame is two positions (rj_frame.hpp).  COUNT / SUM are differences of two
// entries of WinScan.  MIN / MAX read a RANGE-EXTREME TREE over the encoded values in the order: level
// 0 has one word per position (a NULL is the identity), level k + 1 one word per FRAME_FANOUT words of
// level k (the extreme of that aligned block), up to the first level of at most FRAME_FANOUT words; the
// levels lie one behind the other in ONE array, so that a level's offset and length follow from the one
// below it by arithmetic and no kernel indexes an array of pointers.  Above level 0 that is fewer than
// n / (FRAME_FANOUT - 1) + 8 words.
constexpr int FRAME_FANOUT = 16;
constexpr int FRAME_THREADS = 256;  // a workgroup of the tree's build: FRAME_FANOUT^2 words of a level -> two levels
static_assert(FRAME_THREADS == FRAME_FANOUT * FRAME_FANOUT && 64 % FRAME_FANOUT == 0, "a block of a level sits in one wave");
// which end of the frame k_frame_pick reads
enum FramePick : int32_t { FRAME_FIRST = 0, FRAME_LAST = 1 };
// what k_frame_sum writes
enum FrameSum : int32_t { FRAME_COUNT_STAR = 0, FRAME_COUNT = 1, FRAME_SUM = 2 };
// every position's partition, as k_win_ranks leaves it
struct FrameRows {
    const unsigned long long* row_number;  // ps = i + 1 - row_number[i]
    const uint32_t*           part_end;    // pe
};

// ---- Set operations (RJ_NODE_SETOP): the rows of both children in one relation (row id < n_left: a
// left row), ordered and cut into runs by the sort's and the grouping's kernels; a run's rows and left
// rows are differences of two prefix counts taken at its head and at the next run's, its multiplicity
// follows from them (rj.h has the table), and an exclusive scan of the multiplicities says where its
// copies go (rj_setop.hip).  Positions are walked in the grouping's geometry, runs in tiles of SETOP_TILE
// and output rows in tiles of SETOP_EMIT_TILE.
enum SetOp : int32_t {  // rj_setop
    SETOP_UNION_ALL = 0,
    SETOP_UNION = 1,
    SETOP_INTERSECT = 2,
    SETOP_INTERSECT_ALL = 3,
    SETOP_EXCEPT = 4,
    SETOP_EXCEPT_ALL = 5
};
constexpr int SETOP_THREADS = GROUP_THREADS;
constexpr int SETOP_TILE = GROUP_TILE;                      // runs per tile of the multiplicity kernels
constexpr int SETOP_ITEMS = SETOP_TILE / SETOP_THREADS;     // runs per thread
constexpr int SETOP_EMIT_ITEMS = 4;                         // output rows per thread
constexpr int SETOP_EMIT_TILE = SETOP_THREADS * SETOP_EMIT_ITEMS;
// One entry per run and one behind the last (start[G] = rows, left[G] = left rows), so that run g has
// start[g + 1] - start[g] rows, left[g + 1] - left[g] of them from the left child.
struct SetopRuns {
    uint32_t* start;  // position of the run's head
    uint32_t* left;   // left rows in front of that position
};

}  // namespace rj
