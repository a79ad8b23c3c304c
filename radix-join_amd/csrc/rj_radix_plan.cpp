// rj_radix_plan.cpp — the pass plan of a radix partition call (see rj_radix_plan.hpp).  Host only.
#include "rj_radix_plan.hpp"

#include <algorithm>
#include <cmath>

#include "rj_internal.hpp"

namespace rj {

uint32_t radix_tiles_per_group(uint64_t tuples_per_segment, uint64_t target_groups) {
    uint64_t k = (tuples_per_segment + (uint64_t)PT_TILE * target_groups - 1) / ((uint64_t)PT_TILE * target_groups);
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(k, 1), 8);
}

uint64_t radix_cap_bound(double B, double C, uint32_t s, double z) {
    const double bound = std::ldexp(C + z * std::sqrt(B * (C + B)) + 0.5 * z * z * B, (int)s) + 32.0 * B;
    return bound < 4.0e9 ? (((uint64_t)std::ceil(bound) + 255u) & ~(uint64_t)255u) : ~(uint64_t)0 >> 1;
}

namespace {

// the layout questions: fills pl.fine .. pl.n_last_out (pl.pbits is set)
void choose_layout(const RadixFacts& f, const Tuning& t, int compute_units, RadixPlan& pl) {
    const uint64_t n = f.n;
    const uint32_t passes = pl.passes(), bits = f.bits;
    const bool     shaped = f.composite || f.preseg_nseg > 0;
    const bool     big = t.xcd_split && n >= (uint64_t)t.xcd_min_rows;  // XCD-aware placement is on for this call
    // Two passes whose final partitions fit one LDS histogram: both digits are counted in a
    // single read of the source, the scatters reserve their ranges tile by tile, and the
    // second histogram pass (4 B/tuple) disappears.
    pl.fine = passes == 2 && bits <= (uint32_t)PT_FINEBITS && !f.external && !shaped && t.fine != 0;
    // tiles per group of the first pass (the fine histogram must know it: see fine_xcd)
    pl.tpg_first = t.tpg1 > 0 ? (uint32_t)t.tpg1 : radix_tiles_per_group(n, 4096);
    if (pl.fine) {
        const uint64_t tiles = (n + PT_TILE - 1) / PT_TILE;
        pl.fine_grid = (uint32_t)std::min<uint64_t>(tiles, (uint64_t)compute_units);
        // XCD-aware placement of the first pass: per-sub-range counts out of the histogram
        // (its grid then is a multiple of 8: workgroup w counts for sub-range w & 7)
        pl.fine_xcd = big && pl.fine_grid >= 8;
        if (pl.fine_xcd) pl.fine_grid &= ~7u;
    }
    // key + one carry word travel as 8-byte pairs in one array (half the streams, twice the
    // bytes per run); RJ_TUNE_PACK: 0 = never, 1 = every plan, 2 = fine-histogram plans only
    // (a later pass' plain histogram reads 8 instead of 4 bytes per tuple from pairs)
    const bool packed = f.word_src ? f.word_src_packed
                                   : (!f.external && f.KW == 1 && f.CW == 1 && (t.pack == 1 || (t.pack == 2 && pl.fine)));
    // one key word + a two-word carry: the LAST pass writes 12-byte tuples into one array
    // (RJ_TUNE_AOS3=0: key array + pair array, as the earlier passes do)
    const bool aos3 = f.KW == 1 && f.CW == 2 && !f.external && !f.single_pass && t.aos3 != 0;
    pl.last = packed ? RadixLast::Packed : (aos3 ? RadixLast::Aos3 : RadixLast::Dense);
    // the last two words of a carry of two or three words are ONE array of 8-byte pairs (at word
    // pair_word); key + one carry word one array of pairs altogether (packed)
    pl.pair_word = f.CW >= 2 ? f.KW + f.CW - 2 : -1;

    // ---- between the passes.  `packed` and `aos3` need different carry widths, so at most one branch applies.
    pl.mid = packed ? RadixMid::Packed : RadixMid::Dense;
    // ... and so do the passes before it (one output stream of 384-byte runs instead of a
    // 128-byte-run key stream + a 256-byte-run pair stream; a later pass' histogram then
    // reads a 16-bit digit side array instead of the keys)
    // RJ_TUNE_AOS_MID: 0 never, 1 always, 2 (default) only for fine-histogram plans, which
    // need no digit side array — with it the first pass loses more (+0.8 ms at 1 B rows) than
    // the histogram gains (−0.4 ms): profiles/r02_y_aos_between_passes_ab.log
    // RJ_TUNE_AOS_MID=3: always, and WITHOUT the side array (the next histogram reads the keys
    // out of the 12-byte tuples)
    if (aos3 && passes >= 2 && (t.aos_mid == 1 || t.aos_mid == 3 || (t.aos_mid == 2 && pl.fine)))
        pl.mid = (!pl.fine && t.aos_mid != 3) ? RadixMid::Aos3Side : RadixMid::Aos3;
    // packed pairs above the fine histogram's limit: a later pass' histogram would read the
    // 8-byte pairs for their 4-byte keys — the pass before it writes the NEXT digit of every
    // tuple as a 16-bit side array instead (2 bytes written + 2 read per tuple instead of 8 read)
    if (packed && !pl.fine && passes >= 2 && t.packed_side != 0 && n >= (uint64_t)t.xcd_min_rows) pl.mid = RadixMid::PackedSide;
    // only a plan that reads columns into arrays of its own, with an exact histogram per pass, takes one of the next two
    const bool plain_packed = pl.mid == RadixMid::Packed && !pl.fine && !shaped && !f.word_src && !f.external;
    // RJ_TUNE_MALL_CHUNK: the second pass of a big packed two-pass plan runs chunk by chunk (RadixOffsets::Chunked)
    const bool chunk_second = t.mall_chunk > 0 && passes == 2 && plain_packed && big;
    // RJ_TUNE_BLOCKED_MID: between the passes of a packed plan the pairs lie in blocks of 256 keys + 256 carries
    // (BlockedLoader), so that the next pass' histogram reads 4 instead of 8 bytes per tuple
    // (the chunked pass has no kernel that reads blocks)
    if (t.blocked_mid != 0 && passes >= 2 && plain_packed && !chunk_second) pl.mid = RadixMid::Blocked;

    // ---- The speculative first pass (SpecParams; only for a caller that handed in a flag word and
    // repeats the call without it when the flag comes back set): no histogram over the source, the 8 << pbits[0]
    // sub-ranges of its output are sized from a 2^-s sample of the keys plus a margin of z standard deviations,
    // and the second pass reads them as input segments with gaps between them.
    // The arrays of that output are made before any count exists: radix_cap_bound with C sampled row positions (at
    // most a slice per tile) and B sub-ranges — 1.071 n at 1 B rows, s = 5, z = 6.  One more tile behind them takes
    // the runs that found no room.  Positions stay 32-bit even if every tuple were reserved behind a full sub-range:
    // cap_max and n are both below 2^31.
    const uint32_t s1 = (uint32_t)t.spec_sample, s2 = (uint32_t)t.spec2_sample;
    const double   B1 = (double)((uint64_t)8 << pl.pbits[0]);
    pl.spec_cap_max = radix_cap_bound(B1, (double)((n + PT_TILE - 1) / PT_TILE) * (double)(PT_TILE >> s1), s1, t.spec_z / 10.0);
    // It has kernels for a source of columns and one input segment (no word source, no shape), arrays of its own
    // whose sizes nobody waits for (not external, no after_offsets), key arrays, pairs or blocked pairs out (no
    // 12-byte tuples between the passes, no side array), and a second pass in one launch (no chunks at all:
    // RJ_TUNE_MALL_CHUNK switches it off for every layout)
    pl.spec = f.spec_flag && t.spec_p1 != 0 && passes == 2 && !pl.fine && !f.word_src && !f.external && !shaped &&
              !f.after_offsets && !pl.aos_mid() && pl.mid != RadixMid::PackedSide && t.mall_chunk <= 0 && big &&
              n >= (uint64_t)t.spec_min_rows && pl.spec_cap_max < (uint64_t(1) << 31) &&
              n < (uint64_t(1) << 31);  // (... and the room left, which goes down by at most n, stays a signed 32-bit number)
    pl.n_first_out = pl.spec ? pl.spec_cap_max + PT_TILE : n;
    // The speculative last pass (k_last_*): the same once more for the B = 2^bits final partitions,
    // sampled from the first pass' output — at most a slice per tile of the second pass (a partial one at the end
    // of each of its 8 << pbits[0] input segments) and never more than n positions — with knobs of its own.
    // 12-byte-tuple plans and packed plans with blocked pairs between the passes have kernels for it.
    const double C2 = std::min((double)n, ((double)(n / PT_TILE) + B1) * (double)(PT_TILE >> s2));
    pl.spec2_cap_max = radix_cap_bound(std::ldexp(1.0, (int)bits), C2, s2, t.spec2_z / 10.0);
    pl.spec2 = pl.spec && f.spec2_ok && t.spec_p2 != 0 && n >= (uint64_t)t.spec2_min_rows &&
               (aos3 || pl.mid == RadixMid::Blocked) && pl.spec2_cap_max < (uint64_t(1) << 31);
    pl.n_last_out = pl.spec2 ? pl.spec2_cap_max + PT_TILE : n;
    if (chunk_second) pl.pass[1].offsets = RadixOffsets::Chunked;
}

// geometry and launchers of pass p; nseg = partitions the pass before it made (1 in front of the first)
void plan_pass(const RadixFacts& f, const Tuning& t, const RadixPlan& pl, uint32_t p, uint32_t nseg, RadixPass& ps) {
    const uint64_t n = f.n;
    const bool     first = p == 0, last = p + 1 == pl.passes(), preseg = first && f.preseg_nseg > 0;
    const bool     big = t.xcd_split && n >= (uint64_t)t.xcd_min_rows;
    ps.bits = pl.pbits[p];
    // segments this pass reads / output segments it fills (the same unless the input is a
    // set of exchanged runs, several of which feed one output segment)
    // (... or the sub-ranges a speculative first pass left behind, eight per output segment)
    ps.spec_in = p == 1 && pl.spec;
    ps.nseg_in = preseg ? f.preseg_nseg : (ps.spec_in ? nseg << 3 : nseg);
    ps.n_oseg = preseg ? f.preseg_n_oseg : nseg;
    ps.bins = (uint64_t)ps.n_oseg << ps.bits;
    if (first && !preseg) {
        ps.tiles_per_group = pl.tpg_first;
        const uint64_t gt = (uint64_t)ps.tiles_per_group * PT_TILE;
        ps.n_groups = (uint32_t)((n + gt - 1) / gt);
    } else {
        ps.tiles_per_group = radix_tiles_per_group(n / (ps.spec_in ? ps.n_oseg : ps.nseg_in) + 1, 16);  // (spec_in: as for whole segments)
        // the last pass of 12-byte-tuple plans (one 384-byte-run output stream) does
        // better with short groups — 2 tiles per workgroup: 9.3-10.3 -> 8.9-9.1 ms per step
        // at 1 B rows; packed 8-byte tuples lose with them
        // (profiles/r03_l_later_pass_group_size_ab.log)
        if (pl.aos3() && last) ps.tiles_per_group = std::min<uint32_t>(ps.tiles_per_group, 2u);
        if (t.tpg2 > 0) ps.tiles_per_group = (uint32_t)t.tpg2;
        const uint64_t gt = (uint64_t)ps.tiles_per_group * PT_TILE;
        ps.n_groups = (uint32_t)(n / gt + ps.nseg_in);  // upper bound; exact count lives on device
        if (big) {
            ps.xcd_remap = 1;
            ps.n_groups += 8;  // 8 * ceil(G / 8) workgroups
        }
    }
    // ---- offsets, and who counts for them
    if (pl.fine) {  // offsets and cursors of both passes came out of the fine histogram
        ps.offsets = RadixOffsets::Fine;
        ps.hist = !first ? RadixHist::None : (f.word_src ? RadixHist::FineWords : RadixHist::FineSrc);
        ps.xcd_log2 = (first && pl.fine_xcd) ? 3u : 0u;
    } else if (first && pl.spec) {
        ps.offsets = RadixOffsets::Sample;
        ps.hist = RadixHist::SampleSrc;
        ps.xcd_log2 = 3u;
    } else if (p == 1 && pl.spec2) {
        ps.offsets = RadixOffsets::Sample;
        ps.hist = RadixHist::LastSample;
        // (the sample's own groups, eight tiles each whatever the scatter's are: a group of the scatter's two
        // tiles would flush its 512 bins for 4096 sampled keys, as many global adds as the exact histogram's)
        ps.sample_groups = (uint32_t)(n / ((uint64_t)LAST_SAMPLE_TPG * PT_TILE) + ps.nseg_in) + (ps.xcd_remap ? 8u : 0u);
    } else {  // RadixOffsets::Hist, or Chunked as choose_layout left it
        // sub-ranges per XCD only where a partition gets many runs (big inputs)
        ps.xcd_log2 = (big && first && !preseg) ? 3u : 0u;
        if (first && !f.word_src)
            ps.hist = RadixHist::Src;
        else if (pl.side() && !first)
            ps.hist = RadixHist::Digits;
        else if (pl.aos_mid() && !first)
            ps.hist = RadixHist::Aos3;
        else if (pl.mid == RadixMid::Blocked && !first)
            ps.hist = RadixHist::Blocked;
        else
            ps.hist = pl.packed() ? RadixHist::Packed : RadixHist::Dense;
    }
    // ---- what the scatter writes, and which one it is
    ps.aos_out = pl.aos_mid() || (pl.aos3() && last);
    ps.blocked_out = pl.mid == RadixMid::Blocked && !last;
    ps.side_out = pl.side() && !last;
    const bool from_columns = first && !f.word_src;
    if (p == 1 && pl.spec2)
        ps.scatter = pl.packed() ? RadixScatter::LastBlocked : RadixScatter::LastDense;
    else if (pl.aos_mid())
        ps.scatter = from_columns ? RadixScatter::Src : (first ? RadixScatter::Dense : RadixScatter::Aos3);
    else if (pl.packed())
        ps.scatter = from_columns ? RadixScatter::SrcPacked : (pl.mid == RadixMid::Blocked ? RadixScatter::Blocked : RadixScatter::Packed);
    else
        ps.scatter = from_columns ? RadixScatter::Src : RadixScatter::Dense;
}

}  // namespace

RadixPlan radix_plan(const RadixFacts& f, const Tuning& t, int compute_units) {
    RadixPlan pl;
    uint32_t  passes = f.single_pass ? 1 : (f.bits + PT_MAXBITS - 1) / PT_MAXBITS;
    if (passes == 0) passes = 1;
    pl.pbits.assign(passes, f.bits / passes);
    for (uint32_t i = 0; i < f.bits % passes; ++i) pl.pbits[i]++;
    // tuning knobs (experiments): RJ_TUNE_P1_BITS moves bits between pass 1 and pass 2
    if (passes == 2 && t.p1_bits > 0) {
        const uint32_t b1 = (uint32_t)t.p1_bits;
        if (b1 < f.bits && b1 <= PT_CAPBITS && f.bits - b1 <= PT_CAPBITS) {
            pl.pbits[0] = b1;
            pl.pbits[1] = f.bits - b1;
        }
    }
    pl.pass.resize(passes);
    choose_layout(f, t, compute_units, pl);
    uint32_t nseg = 1;
    for (uint32_t p = 0; p < passes; ++p) {
        plan_pass(f, t, pl, p, nseg, pl.pass[p]);
        nseg = (uint32_t)pl.pass[p].bins;
    }
    return pl;
}

}  // namespace rj
