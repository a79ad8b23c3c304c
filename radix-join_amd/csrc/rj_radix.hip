// rj_radix.hip — the radix partition driver (see rj_radix.hpp): it asks rj_radix_plan.cpp for the plan,
// allocates, and runs one offsets step and one scatter step per pass.  Host code only.
#include "rj_radix.hpp"

#include <algorithm>

#include "rj_radix_plan.hpp"

namespace rj {

void read_back(Context* ctx, void* dst, const void* src, size_t bytes) {
    try {
        RJ_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
    } catch (...) {
        (void)hipStreamSynchronize(ctx->stream);
        throw;
    }
}

namespace {

RadixFacts facts_of(const PartitionRequest& rq) {
    RadixFacts f;
    f.n = rq.ws ? rq.ws->n : (rq.src ? rq.src->n_rows : 0);
    f.KW = rq.KW, f.CW = rq.CW, f.bits = rq.bits, f.shift0 = rq.shift0, f.single_pass = rq.single_pass;
    f.word_src = rq.ws != nullptr, f.word_src_packed = rq.ws && rq.ws->packed;
    f.external = rq.external != nullptr;
    f.composite = rq.shape && rq.shape->hi_shift;
    if (rq.shape && rq.shape->nseg > 0) f.preseg_nseg = rq.shape->nseg, f.preseg_n_oseg = rq.shape->n_oseg;
    f.after_offsets = rq.after_offsets != nullptr;
    f.spec_flag = rq.spec_flag != nullptr, f.spec2_ok = rq.spec2_ok;
    return f;
}

// RJ_DIAG >= 1: how full the sub-ranges of a speculative first pass came out (waits for the stream)
void spec_report(Context* ctx, const BufP& cursor, const BufP& limit, const BufP& start, uint32_t nb, uint64_t n, uint64_t n_alloc,
                 int pass) {
    std::vector<unsigned long long> c(nb);  // (pass 1: {position, room} words; pass 2: 32-bit positions)
    std::vector<uint32_t>           lim(nb), st(nb);
    if (pass == 1) {
        read_back(ctx, c.data(), cursor->p, (size_t)nb * 8);
        read_back(ctx, st.data(), start->p, (size_t)nb * 4);
    } else {  // (`start`: {begin, end} pairs)
        std::vector<uint32_t> c32(nb), be(2 * (size_t)nb);
        read_back(ctx, c32.data(), cursor->p, (size_t)nb * 4);
        read_back(ctx, be.data(), start->p, (size_t)nb * 8);
        for (uint32_t i = 0; i < nb; ++i) c[i] = c32[i], st[i] = be[2 * (size_t)i];
    }
    read_back(ctx, lim.data(), limit->p, (size_t)nb * 4);
    double   worst = 0;
    uint32_t over = 0;
    for (uint32_t i = 0; i < nb; ++i) {
        const double used = (double)((uint32_t)c[i] - st[i]), room = (double)(lim[i] - st[i]);
        if (used > room) ++over;
        if (room > 0) worst = std::max(worst, used / room);
    }
    fprintf(stderr, "[rj diag] speculative pass %d: rows=%llu sub-ranges=%u fullest=%.4f of its capacity, over=%u, room for %llu tuples (+%.3f)\n",
            pass, (unsigned long long)n, nb, worst, over, (unsigned long long)n_alloc, (double)n_alloc / (double)std::max<uint64_t>(n, 1) - 1.0);
}

// What one pass owns while it runs.  Its histogram, cursors and group table go back to the block cache when the
// pass is through; its offsets live on as the next pass' input segments.
struct PassRun {
    const RadixPass& ps;
    uint32_t         p, F;
    PassParams       pp{};
    SpecParams       sp{};
    LastParams       lp{};
    BufP             grp_start, off, hist, cursor;  // group table, partition offsets, bin totals, write cursors
    const uint32_t*  in_end = nullptr;              // ends of input segments that do not lie one behind the other
    const uint32_t*  oseg_base = nullptr;           // where every OUTPUT segment starts (nullptr: one segment from 0)
    PassRun(const RadixPass& s, uint32_t pass) : ps(s), p(pass), F(1u << s.bits) {}
};

class Driver {
   public:
    Driver(Context* c, const Launch& l, const PartitionRequest& r)
        : ctx(c), L(l), rq(r), src(r.src ? *r.src : none), n(r.ws ? r.ws->n : src.n_rows),
          pl(radix_plan(facts_of(r), c->tune, c->compute_units())), passes(pl.passes()) {}

    Parted run() {
        P.NW = rq.KW + rq.CW;
        P.packed = pl.packed(), P.aos3 = pl.aos3(), P.spec = pl.spec, P.spec2 = pl.spec2;
        allocate();
        shift = rq.shift0;
        cur = rq.ws ? rq.ws->w : Words{};
        nxt = (pl.aos3() && passes == 1) ? waos : wa;
        for (uint32_t p = 0; p < passes; ++p) {
            PassRun r(pl.pass[p], p);
            begin_pass(r);
            offsets_for_pass(r);
            if (p == 0 && rq.after_offsets) (*rq.after_offsets)(r.off->as<uint32_t>());
            if (p == 0 && pl.chunk_second()) send_sizes_to_host(r);
            if (r.ps.offsets != RadixOffsets::Chunked) scatter_pass(r);  // (the chunked pass scattered chunk by chunk, behind each histogram)
            advance(r);
        }
        P.w = cur;
        for (int a = 0; a < P.NW; ++a) P.wbuf[a] = cur_is_a ? A[a] : B[a];
        if (pl.aos3()) P.wbuf[0] = AOS;
        P.off = seg_off;
        P.NP = nseg;
        P.pbits = pl.pbits;
        const PassShape* shape = rq.shape;
        if (shape && !shape->prior_bits.empty()) P.pbits.insert(P.pbits.begin(), shape->prior_bits.begin(), shape->prior_bits.end());
        P.n_tuples = n;
        return std::move(P);
    }

   private:
    Context*                ctx;
    const Launch&           L;
    const PartitionRequest& rq;
    const TupleSrc          none{};
    const TupleSrc&         src;
    const uint64_t          n;
    const RadixPlan         pl;
    const uint32_t          passes;
    Parted                  P;
    // the word arrays two passes swap (A, B), the last pass' 12-byte tuples, 12-byte tuples and digit side arrays between passes
    BufP  A[MAX_WORDS], B[MAX_WORDS], AOS, MID[2], SIDE[2];
    Words wa{}, wb{}, waos{};
    BufP  fine_off, fine_cursor, coarse_off, coarse_cursor;
    BufP  last_limit, last_seg_sum, last_grp;  // per final partition of a speculative last pass: limit = begin + capacity, [begin, end) holds tuples
    BufP  spec_start, spec_limit, spec_end;    // per sub-range of a speculative first pass' output: [start, end) holds tuples, limit = start + capacity
    Event chunk_ev;                            // the first pass' partition sizes have reached the host (chunked second pass)
    // what moves from pass to pass
    BufP     seg_off;  // offsets produced by the previous pass
    uint32_t nseg = 1, shift = 0;
    Words    cur{}, nxt{};
    bool     cur_is_a = false;

    // (MID / SIDE buffers of a pass are read by the next one only; they go back to the block cache
    // with everything else here when the call returns — all on one stream)
    void allocate() {
        const uint32_t mids = std::min<uint32_t>(passes - 1, 2);
        if (pl.aos_mid())
            for (uint32_t k = 0; k < mids; ++k) {
                MID[k] = ctx->buf(std::max<uint64_t>(n, 1) * 12);
                if (pl.mid == RadixMid::Aos3Side) SIDE[k] = ctx->buf(std::max<uint64_t>(n, 1) * 2 + 16);
            }
        if (pl.mid == RadixMid::PackedSide)
            for (uint32_t k = 0; k < mids; ++k) SIDE[k] = ctx->buf(std::max<uint64_t>(n, 1) * 2 + 16);
        if (pl.aos3()) {
            AOS = ctx->buf(std::max<uint64_t>(pl.n_last_out, 1) * 12);
            waos.w[0] = AOS->as<uint32_t>();
        }
        for (int a = 0; a < (pl.packed() ? 1 : P.NW); ++a) {
            if (pl.pair_word >= 0 && a == pl.pair_word + 1) continue;
            const uint64_t wbytes = (pl.packed() || a == pl.pair_word) ? 8 : 4;
            if (rq.external) {
                wa.w[a] = rq.external->w[a];
                continue;
            }
            if ((pl.aos3() && passes == 1) || pl.aos_mid()) continue;  // every pass writes 12-byte tuples
            // (+2048: a blocked array ends with a whole block, see BlockedLoader)
            A[a] = ctx->buf(pl.n_first_out * wbytes + 2048);
            wa.w[a] = A[a]->as<uint32_t>();
            if (passes > (pl.aos3() ? 2u : 1u)) {
                B[a] = ctx->buf(pl.n_last_out * wbytes + 2048);
                wb.w[a] = B[a]->as<uint32_t>();
            }
        }
    }

    // PassParams of the pass, and the group table of a pass over several segments
    void begin_pass(PassRun& r) {
        const RadixPass& ps = r.ps;
        const PassShape* shape = r.p == 0 ? rq.shape : nullptr;
        const bool       preseg = shape && shape->nseg > 0;
        PassParams&      pp = r.pp;
        pp.nseg = nseg;
        pp.n = (uint32_t)n;
        pp.shift = shift;
        pp.fanout_log2 = ps.bits;
        pp.tiles_per_group = ps.tiles_per_group;
        pp.xcd_log2 = ps.xcd_log2;
        pp.xcd_remap = ps.xcd_remap;
        if (shape && shape->hi_shift) {
            pp.hi_shift = shape->hi_shift;
            pp.lo_bits = shape->lo_bits;
        }
        r.in_end = preseg ? shape->seg_end : (ps.spec_in ? spec_end->as<uint32_t>() : nullptr);
        // (one workgroup per OUTPUT segment scans; its base = where that segment starts)
        r.oseg_base = preseg ? shape->oseg_off : (seg_off ? seg_off->as<uint32_t>() : nullptr);
        if (r.p == 0 && !preseg) return;  // one segment [0, n)
        const uint32_t* in_off = preseg ? shape->seg_begin : (ps.spec_in ? spec_start->as<uint32_t>() : seg_off->as<uint32_t>());
        r.grp_start = ctx->buf(((uint64_t)ps.nseg_in + 1) * 4);
        launch_group_table(L, in_off, ps.nseg_in, ps.tiles_per_group * (uint32_t)PT_TILE, r.grp_start->as<uint32_t>(), r.in_end);
        pp.nseg = ps.nseg_in;
        pp.seg_off = in_off;
        pp.seg_end = r.in_end;
        pp.oseg_shift = preseg ? shape->oseg_shift : (ps.spec_in ? 3u : 0u);
        pp.grp_start = r.grp_start->as<uint32_t>();
    }

    // the pass' partition offsets and write cursors, enqueued
    void offsets_for_pass(PassRun& r) {
        switch (r.ps.offsets) {
        case RadixOffsets::Fine:  // offsets and cursors of both passes come out of the fine histogram
            if (r.ps.hist != RadixHist::None) fine_histogram();
            r.off = r.p == 0 ? coarse_off : fine_off;
            r.cursor = r.p == 0 ? coarse_cursor : fine_cursor;
            r.pp.cursor = r.cursor->as<uint32_t>();
            break;
        case RadixOffsets::Hist:
            exact_bins(r);
            exact_histogram(r);
            launch_scan_segments(L, r.pp.hist, r.oseg_base, r.ps.n_oseg, r.F, r.pp.xcd_log2, r.off->as<uint32_t>(), r.pp.cursor);
            break;
        case RadixOffsets::Sample:
            if (r.ps.hist == RadixHist::SampleSrc)
                sample_first(r);
            else
                sample_last(r);
            break;
        case RadixOffsets::Chunked:
            exact_bins(r);
            chunked_pass(r);
            break;
        }
    }

    void fine_histogram() {
        const uint32_t NB = 1u << rq.bits, F1 = 1u << pl.pbits[0], F2 = 1u << pl.pbits[1];
        const bool     fine_xcd = pl.fine_xcd;
        BufP           fh = ctx->buf((uint64_t)NB * 4);
        fine_off = ctx->buf(((uint64_t)NB + 1) * 4);
        fine_cursor = ctx->buf((uint64_t)NB * 4);
        coarse_off = ctx->buf(((uint64_t)F1 + 1) * 4);
        coarse_cursor = ctx->buf((uint64_t)F1 * 4 * (fine_xcd ? 8 : 1));
        BufP coarse_x;
        RJ_HIP(hipMemsetAsync(fh->p, 0, (uint64_t)NB * 4, ctx->stream));
        if (fine_xcd) {
            coarse_x = ctx->buf((uint64_t)F1 * 8 * 4);
            RJ_HIP(hipMemsetAsync(coarse_x->p, 0, (uint64_t)F1 * 8 * 4, ctx->stream));
        }
        uint32_t* cx = fine_xcd ? coarse_x->as<uint32_t>() : nullptr;
        if (rq.ws)
            launch_fine_hist_words(L, rq.ws->w, rq.ws->packed, (uint32_t)n, rq.shift0, pl.pbits[0], pl.pbits[1], pl.fine_grid,
                                   fh->as<uint32_t>(), fine_xcd ? pl.tpg_first : 0u, cx);
        else
            launch_fine_hist_src(L, src, rq.KW, rq.shift0, pl.pbits[0], pl.pbits[1], pl.fine_grid, fh->as<uint32_t>(),
                                 fine_xcd ? pl.tpg_first : 0u, cx);
        launch_scan_fine(L, fh->as<uint32_t>(), F1, F2, fine_off->as<uint32_t>(), fine_cursor->as<uint32_t>(),
                         coarse_off->as<uint32_t>(), coarse_cursor->as<uint32_t>(), cx);
    }

    // zeroed bin totals, offsets and cursors of a pass that counts every tuple
    void exact_bins(PassRun& r) {
        const uint64_t bins = r.ps.bins;
        r.hist = ctx->buf((bins << r.pp.xcd_log2) * 4);
        r.off = ctx->buf((bins + 1) * 4);
        r.cursor = ctx->buf((bins << r.pp.xcd_log2) * 4);
        RJ_HIP(hipMemsetAsync(r.hist->p, 0, (bins << r.pp.xcd_log2) * 4, ctx->stream));
        r.pp.hist = r.hist->as<uint32_t>();
        r.pp.cursor = r.cursor->as<uint32_t>();
    }

    void exact_histogram(PassRun& r) {
        const uint32_t G = r.ps.n_groups, prev = (r.p + 1) % 2;  // (the MID / SIDE array the pass before this one wrote)
        switch (r.ps.hist) {
        case RadixHist::Src: launch_pass_hist_src(L, src, rq.KW, r.pp, G); break;
        case RadixHist::Digits: launch_pass_hist_digits(L, SIDE[prev]->as<uint16_t>(), r.pp, G); break;
        case RadixHist::Aos3: launch_pass_hist_aos3(L, MID[prev]->as<uint32_t>(), r.pp, G); break;
        case RadixHist::Blocked: launch_pass_hist_blocked(L, cur.w[0], r.pp, G); break;
        case RadixHist::Packed: launch_pass_hist_packed(L, cur.w[0], r.pp, G); break;
        case RadixHist::Dense: launch_pass_hist_dense(L, cur, r.pp, G); break;
        default: throw_fmt(RJ_ERR_DEVICE, "radix plan: pass %u has no exact histogram", r.p);
        }
    }

    // speculative first pass: sample -> capacities, {position, room} cursors; the partition offsets come from
    // where the cursors stand once the scatter is through (launch_spec_close in scatter_pass)
    void sample_first(PassRun& r) {
        const uint32_t spec_s = (uint32_t)ctx->tune.spec_sample;
        const uint32_t nb = (uint32_t)r.ps.bins << 3;
        r.hist = ctx->buf((uint64_t)nb * 4);
        r.off = ctx->buf((r.ps.bins + 1) * 4);
        r.cursor = ctx->buf((uint64_t)nb * 8);
        spec_start = ctx->buf((uint64_t)nb * 4);
        spec_limit = ctx->buf((uint64_t)nb * 4);
        spec_end = ctx->buf((uint64_t)nb * 4);
        RJ_HIP(hipMemsetAsync(r.hist->p, 0, (uint64_t)nb * 4, ctx->stream));
        r.pp.hist = r.hist->as<uint32_t>();
        r.sp.cursor = r.cursor->as<unsigned long long>();
        r.sp.flag = rq.spec_flag;
        r.sp.sink = (uint32_t)pl.spec_cap_max;
        r.sp.sample_log2 = spec_s;
        launch_pass_sample_src(L, src, rq.KW, r.pp, r.sp, r.ps.n_groups);
        launch_spec_caps(L, r.pp.hist, nb, spec_s, (float)(ctx->tune.spec_z / 10.0), (uint32_t)pl.spec_cap_max,
                         spec_start->as<uint32_t>(), spec_limit->as<uint32_t>(), r.sp.cursor);
    }

    // speculative last pass: sample of the first pass' output -> capacities; `off` = where the final partitions begin
    void sample_last(PassRun& r) {
        const uint32_t spec2_s = (uint32_t)ctx->tune.spec2_sample;
        const uint32_t nb = (uint32_t)r.ps.bins, nseg_in = r.ps.nseg_in;
        r.hist = ctx->buf((uint64_t)nb * 4);
        r.off = ctx->buf((uint64_t)nb * 8);  // {begin, end} pairs
        r.cursor = ctx->buf((uint64_t)nb * 4);
        last_limit = ctx->buf((uint64_t)nb * 4);
        last_seg_sum = ctx->buf((uint64_t)r.ps.n_oseg * 8);
        RJ_HIP(hipMemsetAsync(r.hist->p, 0, (uint64_t)nb * 4, ctx->stream));
        r.pp.hist = r.hist->as<uint32_t>();
        r.lp.cursor32 = r.cursor->as<uint32_t>();
        r.lp.limit = last_limit->as<uint32_t>();
        r.lp.flag = rq.spec_flag;
        r.lp.sink = (uint32_t)pl.spec2_cap_max;
        r.lp.sample_log2 = spec2_s;
        // (the sample's own groups, LAST_SAMPLE_TPG tiles each whatever the scatter's are: see rj_radix_plan.cpp)
        PassParams ps = r.pp;
        ps.tiles_per_group = LAST_SAMPLE_TPG;
        last_grp = ctx->buf(((uint64_t)nseg_in + 1) * 4);
        launch_group_table(L, r.pp.seg_off, nseg_in, LAST_SAMPLE_TPG * (uint32_t)PT_TILE, last_grp->as<uint32_t>(), r.in_end);
        ps.grp_start = last_grp->as<uint32_t>();
        launch_last_sample(L, cur.w[0], P.packed, ps, r.lp, r.ps.sample_groups);
        launch_last_caps(L, r.pp.hist, r.ps.n_oseg, r.F, spec2_s, (float)(ctx->tune.spec2_z / 10.0), (uint32_t)pl.spec2_cap_max,
                         last_seg_sum->as<unsigned long long>(), r.off->as<uint32_t>(), last_limit->as<uint32_t>(), r.lp.cursor32);
    }

    // the second pass in chunks needs the first pass' partition sizes on the HOST (exact grids per
    // chunk): they leave before the first scatter is enqueued, and are read while it runs
    void send_sizes_to_host(PassRun& r) {
        const uint64_t bytes = (r.ps.bins + 1) * 4;
        if (bytes > Context::SMALL_PINNED / 4) throw_fmt(RJ_ERR_DEVICE, "chunked pass: too many segments");
        RJ_HIP(hipMemcpyAsync(ctx->small_pinned(), r.off->p, bytes, hipMemcpyDeviceToHost, ctx->stream));
        chunk_ev.make();
        RJ_HIP(hipEventRecord(chunk_ev.e, ctx->stream));
    }

    // ---- histogram / scan / scatter of the pass, `mall_chunk` input segments at a time,
    // chunks alternating between the context's two compute streams: the scatter of a
    // chunk re-reads what its histogram launch has just pulled through the Infinity
    // Cache.  Segments never share bins, cursors or output ranges, so the chunks are
    // independent; grids are exact (the segment sizes are on the host by now).
    void chunked_pass(PassRun& r) {
        const PassParams& pp = r.pp;
        const uint32_t    nseg_in = r.ps.nseg_in, F = r.F;
        RJ_HIP(hipEventSynchronize(chunk_ev.e));
        const uint32_t* hoff = static_cast<const uint32_t*>(ctx->small_pinned());
        const uint64_t  gt = (uint64_t)pp.tiles_per_group * PT_TILE;
        std::vector<uint32_t> gstart(nseg_in + 1, 0);
        for (uint32_t sgi = 0; sgi < nseg_in; ++sgi)
            gstart[sgi + 1] = gstart[sgi] + (uint32_t)(((uint64_t)(hoff[sgi + 1] - hoff[sgi]) + gt - 1) / gt);
        Event e_in, e_aux;
        e_in.make();
        e_aux.make();
        hipStream_t aux = ctx->aux_stream();
        RJ_HIP(hipEventRecord(e_in.e, ctx->stream));  // (behind the previous scatter and the bin memset)
        RJ_HIP(hipStreamWaitEvent(aux, e_in.e, 0));
        Launch L2 = L;
        L2.stream = aux;
        const uint32_t CH = (uint32_t)ctx->tune.mall_chunk;
        uint32_t       c = 0;
        for (uint32_t s0 = 0; s0 < nseg_in; s0 += CH, ++c) {
            const uint32_t s1 = std::min(nseg_in, s0 + CH), G = gstart[s1] - gstart[s0];
            const Launch& Lc = (c & 1u) ? L2 : L;
            PassParams    pc = pp;
            pc.nseg = s1 - s0;
            pc.seg_off = pp.seg_off + s0;
            pc.grp_start = pp.grp_start + s0;
            pc.grp_base = gstart[s0];
            pc.hist = pp.hist + (size_t)s0 * F;
            pc.cursor = pp.cursor + (size_t)s0 * F;
            const uint32_t grid = pp.xcd_remap ? ((G + 7u) & ~7u) : G;
            if (G) launch_pass_hist_packed(Lc, cur.w[0], pc, grid);
            // (empty segments still need their partition offsets)
            launch_scan_segments(Lc, pc.hist, pc.seg_off, pc.nseg, F, 0, r.off->as<uint32_t>() + (size_t)s0 * F, pc.cursor);
            if (G) launch_pass_scatter_packed(Lc, cur.w[0], pc, grid, nxt.w[0]);
        }
        RJ_HIP(hipEventRecord(e_aux.e, aux));
        RJ_HIP(hipStreamWaitEvent(ctx->stream, e_aux.e, 0));  // (before any buffer of this pass is reused)
    }

    void scatter_pass(PassRun& r) {
        const RadixPass& ps = r.ps;
        const uint32_t   p = r.p, G = ps.n_groups;
        PassParams&      pp = r.pp;
        if (pl.aos_mid()) {  // 12-byte tuples out of every pass
            nxt = Words{};
            nxt.w[0] = p + 1 == passes ? waos.w[0] : MID[p % 2]->as<uint32_t>();
        }
        if (ps.side_out) {
            pp.side_out = SIDE[p % 2]->as<uint16_t>();
            pp.next_shift = shift + ps.bits;
            pp.next_mask = (1u << pl.pbits[p + 1]) - 1u;
        }
        const SpecParams* sp = (p == 0 && pl.spec) ? &r.sp : nullptr;
        switch (ps.scatter) {
        case RadixScatter::Src: launch_pass_scatter_src(L, src, rq.KW, rq.CW, pp, G, nxt, ps.aos_out, sp); break;
        case RadixScatter::SrcPacked: launch_pass_scatter_src_packed(L, src, pp, G, nxt.w[0], ps.blocked_out, sp); break;
        case RadixScatter::Dense: launch_pass_scatter_dense(L, cur, P.NW, pl.pair_word, pp, G, nxt, ps.aos_out); break;
        case RadixScatter::Packed: launch_pass_scatter_packed(L, cur.w[0], pp, G, nxt.w[0]); break;
        case RadixScatter::Blocked: launch_pass_scatter_blocked(L, cur.w[0], pp, G, nxt.w[0], ps.blocked_out); break;
        case RadixScatter::Aos3: launch_pass_scatter_aos3(L, MID[(p + 1) % 2]->as<uint32_t>(), pp, G, nxt.w[0]); break;
        case RadixScatter::LastBlocked: launch_last_scatter_blocked(L, cur.w[0], pp, G, nxt.w[0], r.lp); break;
        case RadixScatter::LastDense: launch_last_scatter_dense(L, cur, pp, G, nxt, r.lp); break;
        }
        const uint32_t bins = (uint32_t)ps.bins;
        if (ps.hist == RadixHist::LastSample) {
            launch_last_close(L, r.lp.cursor32, last_limit->as<uint32_t>(), bins, r.off->as<uint32_t>());
            if (ctx->tune.diag >= 1) spec_report(ctx, r.cursor, last_limit, r.off, bins, n, pl.n_last_out, 2);
            P.off_shift = 1;
        }
        if (ps.hist == RadixHist::SampleSrc) {
            launch_spec_close(L, r.sp.cursor, spec_start->as<uint32_t>(), spec_limit->as<uint32_t>(), r.F, spec_end->as<uint32_t>(),
                              r.off->as<uint32_t>());
            if (ctx->tune.diag >= 1) spec_report(ctx, r.cursor, spec_limit, spec_start, bins << 3, n, pl.n_first_out, 1);
        }
    }

    // the pass' output becomes the next pass' input
    void advance(PassRun& r) {
        seg_off = r.off;
        nseg = (uint32_t)r.ps.bins;
        shift += r.ps.bits;
        cur = nxt;
        cur_is_a = (r.p % 2 == 0);
        nxt = cur_is_a ? wb : wa;
        if (pl.aos3() && r.p + 2 == passes) nxt = waos;  // the next pass is the last one
    }
};

}  // namespace

Parted radix_partition(Context* ctx, const Launch& L, const PartitionRequest& rq) { return Driver(ctx, L, rq).run(); }

}  // namespace rj
