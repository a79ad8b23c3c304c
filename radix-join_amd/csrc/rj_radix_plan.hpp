// rj_radix_plan.hpp — every decision of a radix partition call that is taken before its first launch: how many
// passes over which bits, which layout the tuples travel in, where each pass gets its partition offsets from
// and which launchers read and write it.  Host-only arithmetic over the facts of the request, the tuning
// knobs and the device's compute-unit count: no HIP (unit-tested on the CPU through rj_debug_partition_plan,
// include/rj.h).  The driver that allocates and launches by this plan is rj_radix.hip.
// There is no reference counterpart (the reference joins with one hash table).
#pragma once
#include <cstdint>
#include <vector>

namespace rj {

struct Tuning;

// What the plan needs to know of a request (PartitionRequest, rj_radix.hpp) — no pointers, no device.
struct RadixFacts {
    uint64_t n = 0;          // rows of the source (NULL keys are dropped on the way: an upper bound on the tuples)
    int      KW = 1, CW = 0;  // key words, carry words
    uint32_t bits = 0, shift0 = 0;
    bool     single_pass = false;
    bool     word_src = false, word_src_packed = false;  // tuples already in the partition layout; ... as 8-byte pairs
    bool     external = false;                            // caller-owned output arrays
    bool     composite = false;                           // PassShape: composite digit (sharded stage A)
    uint32_t preseg_nseg = 0, preseg_n_oseg = 0;          // PassShape: pre-segmented input (sharded stage B), 0 = not
    bool     after_offsets = false;                       // the caller wants the first pass' offsets ahead of its scatter
    bool     spec_flag = false, spec2_ok = false;         // a flag word was given; the caller reads through Parted::off_shift
};

// How tuples lie in the arrays the passes hand to one another (and in a word source).
enum class RadixMid : int32_t {
    Dense = 0,       // one array per word; the last two words of a 2- or 3-word carry as one array of 8-byte pairs
    Packed = 1,      // key + one carry word: one array of 8-byte pairs
    PackedSide = 2,  // ... and the next pass' digit of every tuple in a 16-bit side array
    Blocked = 3,     // ... the pairs in blocks of 256 keys + 256 carries (BlockedLoader)
    Aos3 = 4,        // key + two carry words: one array of 12-byte tuples
    Aos3Side = 5,    // ... and the 16-bit digit side array
};
// How the last pass writes (what Parted::packed / Parted::aos3 say).
enum class RadixLast : int32_t { Dense = 0, Packed = 1, Aos3 = 2 };
// Where a pass gets its partition offsets from.
enum class RadixOffsets : int32_t {
    Fine = 0,     // both digits counted in one read of the source, ahead of the first pass
    Hist = 1,     // its own exact histogram
    Sample = 2,   // capacities from a sample: the speculative first pass (k_spec_*) or last pass (k_last_*)
    Chunked = 3,  // second pass only: exact histogram, scan and scatter chunk by chunk on two streams
};
// The launcher that counts for a pass (rj_kernels.hpp: launch_pass_hist_*, launch_fine_hist_*, launch_*_sample*).
enum class RadixHist : int32_t { None = 0, FineSrc, FineWords, Src, Digits, Aos3, Blocked, Packed, Dense, SampleSrc, LastSample };
// The launcher that writes a pass (launch_pass_scatter_*, launch_last_scatter_*).
enum class RadixScatter : int32_t { Src = 0, SrcPacked, Dense, Packed, Blocked, Aos3, LastBlocked, LastDense };

struct RadixPass {
    uint32_t     bits = 0;
    uint32_t     tiles_per_group = 1, xcd_log2 = 0, xcd_remap = 0;
    uint32_t     nseg_in = 1, n_oseg = 1;  // segments the pass reads / output segments it fills
    uint64_t     bins = 0;                 // n_oseg << bits
    uint32_t     n_groups = 0;             // workgroups: exact for a one-segment first pass, else an upper bound
    uint32_t     sample_groups = 0;        // RadixHist::LastSample: the bound for the sample's own groups (LAST_SAMPLE_TPG tiles)
    bool         spec_in = false;          // reads the sub-ranges a speculative first pass left behind, eight per output segment
    bool         aos_out = false, blocked_out = false, side_out = false;  // what the scatter writes
    RadixOffsets offsets = RadixOffsets::Hist;
    RadixHist    hist = RadixHist::None;
    RadixScatter scatter = RadixScatter::Dense;
};

struct RadixPlan {
    std::vector<uint32_t>  pbits;  // radix bits of each pass
    std::vector<RadixPass> pass;
    uint32_t  passes() const { return (uint32_t)pbits.size(); }
    bool      fine = false, fine_xcd = false;
    uint32_t  fine_grid = 0;  // workgroups of the fine histogram
    RadixMid  mid = RadixMid::Dense;
    RadixLast last = RadixLast::Dense;
    int       pair_word = -1;  // Dense: the word at which the carry's 8-byte pair array starts, -1 = none
    bool      spec = false, spec2 = false;
    uint64_t  spec_cap_max = 0, spec2_cap_max = 0;  // the bounds, whether or not the pass is speculative
    uint64_t  n_first_out = 0, n_last_out = 0;      // tuples the first / last pass' output arrays hold
    uint32_t  tpg_first = 1;                        // tiles per group of the first pass
    bool packed() const { return last == RadixLast::Packed; }
    bool aos3() const { return last == RadixLast::Aos3; }
    bool aos_mid() const { return mid == RadixMid::Aos3 || mid == RadixMid::Aos3Side; }
    bool side() const { return mid == RadixMid::Aos3Side || mid == RadixMid::PackedSide; }
    bool chunk_second() const { return pass.size() == 2 && pass[1].offsets == RadixOffsets::Chunked; }
};

// tiles per group of a speculative last pass' sample, whatever the scatter's are (see radix_plan)
constexpr uint32_t LAST_SAMPLE_TPG = 8;

uint32_t radix_tiles_per_group(uint64_t tuples_per_segment, uint64_t target_groups);

// Room for the sub-ranges of a speculative pass, made before any count exists.  With C sampled positions, B
// sub-ranges and sample counts c_i, sum c_i <= C, the capacities k_spec_caps / k_last_caps hand out sum to
//   sum 2^s (c_i + z sqrt(c_i + 1) + z^2 / 2) + 32 B  <=  2^s C + 2^s z sqrt(B (C + B)) + 2^s z^2 / 2 B + 32 B
// (Cauchy–Schwarz on the square roots; 32 B: each is rounded up to a multiple of 32), rounded up to a multiple
// of 256; 2^63 - 1 when that is 4e9 or more.
uint64_t radix_cap_bound(double B, double C, uint32_t s, double z);

RadixPlan radix_plan(const RadixFacts& f, const Tuning& tune, int compute_units);

}  // namespace rj
