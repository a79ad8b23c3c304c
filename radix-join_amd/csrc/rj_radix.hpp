// rj_radix.hpp — the radix partition driver every join, aggregation and sharded stage goes through: what a
// call asks for (PartitionRequest), what it leaves behind (Parted), and radix_partition() itself.  Host code
// only (rj_radix.hip): the decisions come from rj_radix_plan.hpp, the kernels are launched through rj_kernels.hpp.
#pragma once
#include <functional>

#include "rj_internal.hpp"

namespace rj {

struct Parted {
    int      NW = 0;
    BufP     wbuf[MAX_WORDS];
    Words    w{};
    BufP     off;  // u32[NP+1]
    uint32_t NP = 0;
    std::vector<uint32_t> pbits;  // radix bits of each pass
    bool     packed = false;      // w[0] = {hashed key, carry} pairs, no w[1]
    bool     aos3 = false;        // w[0] = 12-byte {hashed key, carry lo, carry hi} tuples, no w[1..2]
    uint64_t n_tuples = 0;        // tuples that went in (NULL keys are dropped on the way: an upper bound)
    bool     spec = false;        // the first pass ran without its histogram (PartitionRequest::spec_flag); the caller's flag word tells
                                  // whether everything found room — if not, what is in here is in bounds but not the partition
    // Partition q holds tuples [off[q << off_shift], off[(q << off_shift) + 1]).  Exact partitions lie one behind the
    // other (off_shift = 0, off = u32[NP + 1]); a speculative LAST pass (spec2, only behind a speculative first one
    // and under the same flag word) leaves unused room behind each: off = u32[2 NP], {begin, end} pairs
    uint32_t off_shift = 0;
    bool     spec2 = false;
};

// Tuples that already sit in the partition layout (hashed word arrays, a pair array for a
// two-word carry, or one array of packed {key, carry} pairs): what a rank holds after the
// exchange step of a sharded join.
struct WordSrc {
    Words    w{};
    uint64_t n = 0;
    bool     packed = false;
};

// How the FIRST pass of a radix_partition() call differs from the plain "one segment, one bit field"
// case — both forms belong to the sharded join:
//   * composite digit (stage A): owner rank from the top hash bits, first local digit from the
//     low ones, in one pass (PassParams::hi_shift / lo_bits);
//   * pre-segmented input (stage B): what arrived in the exchange is a set of runs, one per
//     (source rank, local digit), listed digit-major; `world` of them feed one output segment
//     (ExchangePlan::seg_begin / seg_end / part_off, rj_xplan.hpp).
struct PassShape {
    uint32_t        hi_shift = 0, lo_bits = 0;
    const uint32_t* seg_begin = nullptr;  // device, [nseg]
    const uint32_t* seg_end = nullptr;    // device, [nseg]
    uint32_t        nseg = 0;
    uint32_t        oseg_shift = 0;       // input segment i feeds output segment i >> oseg_shift
    const uint32_t* oseg_off = nullptr;   // device, [n_oseg + 1]
    uint32_t        n_oseg = 0;
    std::vector<uint32_t> prior_bits;     // digits consumed before this call (for the partition index)
};

// One call of the driver.  Source = columns (`src`: page decode, NULL drop and hashing ride on the first pass)
// or tuples already in the partition layout (`ws`, sharded stage B): columns() / words() set the four fields
// every call has, a caller then names what else it needs.
struct PartitionRequest {
    const TupleSrc* src = nullptr;
    const WordSrc*  ws = nullptr;
    int             KW = 1, CW = 0;
    uint32_t        bits = 0;
    uint32_t        shift0 = 0;
    bool            single_pass = false;
    const Words*    external = nullptr;  // caller-owned arrays that receive the output of a single-pass partition
    // called once the FIRST pass' partition offsets are enqueued to be computed, before its scatter is
    // enqueued — a caller that needs the counts on the host (the sharded join's stage A) copies them out
    // ahead of the scatter
    const std::function<void(const uint32_t*)>* after_offsets = nullptr;
    const PassShape* shape = nullptr;
    // device, zeroed by the caller: the call may run its first pass speculatively (RadixPlan::spec); the word is
    // then set on the device if the result has to be thrown away, Parted::spec says it was tried
    uint32_t* spec_flag = nullptr;
    // ... and, behind a speculative first pass, its last pass too (only a caller whose kernels read a partition
    // through Parted::off_shift: the inner join)
    bool spec2_ok = false;

    static PartitionRequest columns(const TupleSrc& s, int KW, int CW, uint32_t bits) {
        PartitionRequest rq;
        rq.src = &s, rq.KW = KW, rq.CW = CW, rq.bits = bits;
        return rq;
    }
    static PartitionRequest words(const WordSrc& s, int KW, int CW, uint32_t bits) {
        PartitionRequest rq;
        rq.ws = &s, rq.KW = KW, rq.CW = CW, rq.bits = bits;
        return rq;
    }
};

Parted radix_partition(Context* ctx, const Launch& L, const PartitionRequest& rq);

// RAII event (timing disabled) on the current device
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    void make() { RJ_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming)); }
    ~Event() {
        if (e) (void)hipEventDestroy(e);
    }
};

// `bytes` from the device into `dst`, waited for.  `dst` is the end of a copy that may still be
// queued when something throws: the stream drains before the exception travels on, so that the
// caller's variable outlives the copy.
void read_back(Context* ctx, void* dst, const void* src, size_t bytes);

}  // namespace rj
