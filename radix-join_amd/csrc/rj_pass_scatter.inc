// rj_pass_scatter.inc — the body of k_pass_scatter and of k_spec_scatter (rj_partition.hip), which include it with
// NW, Loader, PAIR, AOS, SPEC, SPEC_LAST and ld, pp, out, sp in scope.  Text shared by inclusion, not through a function: the
// exact kernels are then compiled from what they were compiled from before the speculative ones existed, and come
// out instruction for instruction the same (profiles/spec_pass1_codeobj.log).
    static_assert(PAIR < 0 || (PAIR >= 1 && PAIR + 1 < NW), "pair = two carry words behind the key");
    static_assert(!AOS || (NW == 3 && PAIR == 1), "12-byte tuples: one key word + a two-word carry");
    __shared__ uint2    s_stage2[PT_TILE];  // 128 KiB: a word array uses the first half
    uint32_t* const     s_stage = reinterpret_cast<uint32_t*>(s_stage2);
    __shared__ uint32_t s_cnt[PT_MAXF + PT_DUMMY];  // (see rank_tile)
    __shared__ uint32_t s_base[PT_MAXF];
    __shared__ uint32_t s_delta[PT_MAXF];
    __shared__ uint32_t s_wsum[PT_THREADS / 64];
    uint32_t            seg, begin, end;
    if (!group_range(pp, blockIdx.x, seg, begin, end)) return;
    const uint32_t F = 1u << pp.fanout_log2, mask = F - 1u;
    // SPEC_LAST (k_last_scatter*, the speculative last pass: LastParams): the reservation is the exact kernel's 32-bit add,
    // and the run fits if it ends at or before the partition's limit.  The limits of the group's output segment are
    // loaded once, into the LDS: thread d keeps nothing more in registers than the exact kernel does (with the first
    // pass' 64-bit {position, room} word the 12-byte kernel spilled two VGPRs in every tile).
    __shared__ uint32_t s_limit[SPEC && SPEC_LAST ? PT_MAXF : 1];
    if constexpr (SPEC && SPEC_LAST) {
        if (threadIdx.x < F) s_limit[threadIdx.x] = last_limit(sp)[(size_t)seg * F + threadIdx.x];  // (the tile loop's first barrier is behind it)
    }

    // Thread d owns digit d's write cursor in a REGISTER: the reservation's round trip is
    // not waited for until the first tile has been loaded and ranked.
    uint32_t run = 0;  // thread d: where digit d's run of the current tile starts in the output
    [[maybe_unused]] unsigned long long res = 0;  // SPEC: what the reservation returned, {position, room}
    uint32_t w[PT_ITEMS][NW];

    for (uint32_t base = begin; base < end; base += PT_TILE) {
        for (uint32_t d = threadIdx.x; d < F; d += PT_THREADS) s_cnt[d] = 0;
        lds_barrier();

        // every load of the tile is issued before the first rank is taken; the ranks wait for the keys only
        const uint32_t ok = ld.template load_tile<NW>(base, end, w);
        // first pass of key + two-word carry: ranks and positions two per register, branch-free (rank_tile).
        // Everything else keeps a rank per register and a branch per item.  The later passes of that shape
        // and the packed kernel gained nothing measurable from the branch-free form
        // (profiles/scatter_rank_ab.log), and with up to four words per tuple in registers there is no room
        // for PT_ITEMS ranks in flight (compiled that way, the four-word kernels spilled more than they do)
        constexpr bool BATCHED = NW == 3 && PAIR == 1 && is_src_loader<Loader>::value;
        uint32_t       ps[PT_ITEMS / 2];  // BATCHED: ranks, then LDS positions, two per register
        uint32_t       dr[PT_ITEMS];      // otherwise: digit << 16 | rank, then LDS position; 0xffffffff = no tuple
        if constexpr (BATCHED) {
            rank_tile<NW>(pp, mask, ok, w, s_cnt, ps);
        } else {
#pragma unroll
            for (int j = 0; j < PT_ITEMS; ++j) {
                dr[j] = 0xffffffffu;
                if ((ok >> j) & 1u) {
                    uint32_t d = pass_digit(pp, w[j][0], mask);
                    uint32_t r = atomicAdd(&s_cnt[d], 1u);
                    dr[j] = (d << 16) | r;
                }
            }
        }
        lds_barrier();

        // PT_THREADS >= PT_MAXF: thread d scans digit d
        // Thread d reserves digit d's range of this tile with one global atomic; its round
        // trip is not waited for until word 0 has been staged.
        uint32_t c = threadIdx.x < F ? s_cnt[threadIdx.x] : 0u;
        if (c) {
            const size_t at = (((size_t)seg * F + threadIdx.x) << pp.xcd_log2) | (blockIdx.x & ((1u << pp.xcd_log2) - 1u));
            if constexpr (SPEC && SPEC_LAST)
                run = atomicAdd(&last_cursor(sp)[at], c);
            else if constexpr (SPEC)
                res = atomicAdd(&sp.cursor[at], (unsigned long long)c | ((unsigned long long)(0u - c) << 32));
            else
                run = atomicAdd(&pp.cursor[at], c);
        }
        uint32_t total;
        uint32_t ex = block_excl_scan(c, s_wsum, total);
        if (threadIdx.x < F) s_base[threadIdx.x] = ex;
        lds_barrier();
        // thread d: global index of digit d's tuples = delta + position in the sorted tile.  (SPEC: looked at
        // here, where the exact kernel first uses `run`, so the reservation's round trip stays hidden as it is)
        auto delta_of = [&]() -> uint32_t {
            if constexpr (SPEC && SPEC_LAST) {
                if (c && run + c > s_limit[threadIdx.x]) {
                    atomicOr(sp.flag, 1u);
                    return sp.sink;
                }
                return run - ex;
            } else if constexpr (SPEC) {
                if (c && (int32_t)(uint32_t)(res >> 32) < (int32_t)c) {
                    atomicOr(sp.flag, 1u);
                    return sp.sink;
                }
                return (uint32_t)res - ex;
            } else {
                return run - ex;
            }
        };

        // LDS position of every tuple, computed once for all word arrays
        if constexpr (BATCHED) {
            place_tile<NW>(pp, mask, ok, w, s_base, ps);
        } else {
#pragma unroll
            for (int j = 0; j < PT_ITEMS; ++j)
                if (dr[j] != 0xffffffffu) dr[j] = s_base[dr[j] >> 16] + (dr[j] & 0xffffu);
        }

        // key + two-word carry (NW == 3): keys and carry pairs of half the sorted tile are staged
        // TOGETHER and copied out together — as 12-byte tuples (AOS) or into the key array and the
        // pair array — so no per-element destination has to be kept in registers between the two
        // arrays (the 16 extra VGPRs spilled to scratch)
        // (the copy-out's thread index is opaque to the compiler: its element indices and LDS addresses,
        // 3 * PT_ITEMS values that do not change from tile to tile, were otherwise hoisted out of the tile
        // loop and held in registers — or spilled — through the phases that have every load in flight)
        const uint32_t tid = BATCHED ? tile_tid() : threadIdx.x;  // (the other shapes compile to more scratch with it)
        if constexpr (NW == 3 && PAIR == 1) {
            constexpr uint32_t HALF = PT_TILE / 2;
            uint2* const       s_p = s_stage2;                                      // [HALF] carries
            uint32_t* const    s_k = reinterpret_cast<uint32_t*>(s_stage2 + HALF);  // [HALF] keys
            if (!BATCHED && threadIdx.x < F) s_delta[threadIdx.x] = delta_of();
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int j = 0; j < PT_ITEMS; ++j) {
                    const uint32_t lp = (BATCHED ? tile_pos(ps, j) : dr[j]) - h * HALF;  // (no tuple: PT_NO_POS stays out of range)
                    if (lp < HALF) {
                        s_k[lp] = w[j][0];
                        s_p[lp] = make_uint2(w[j][1], w[j][2]);
                    }
                }
                // global index = delta + sorted position.  BATCHED: behind the first half's staging, since the
                // reservation was issued after the carry loads and waiting for it waits for all of them
                if (BATCHED && h == 0 && threadIdx.x < F) s_delta[threadIdx.x] = delta_of();
                lds_barrier();
#pragma unroll
                for (int k = 0; k < PT_ITEMS / 2; ++k) {
                    const uint32_t i = k * PT_THREADS + tid, gi = h * HALF + i;
                    if (gi < total) {
                        const uint32_t v = s_k[i];
                        const uint2    c = s_p[i];
                        const uint32_t g = s_delta[pass_digit(pp, v, mask)] + gi;
                        if constexpr (AOS) {
                            uint32_t* o = out.w[0] + (size_t)g * 3u;
                            o[0] = v;
                            o[1] = c.x;
                            o[2] = c.y;
                            if (pp.side_out) pp.side_out[g] = (uint16_t)((v >> pp.next_shift) & pp.next_mask);
                        } else {
                            out.w[0][g] = v;
                            reinterpret_cast<uint2*>(out.w[1])[g] = c;
                        }
                    }
                }
                lds_barrier();
            }
            continue;
        }
        // word 0 (the hashed key): stage in digit order, copy out.  The digit of a staged
        // key is recomputed from the key itself, and the global destination of each LDS
        // position is kept in a register for the remaining word arrays.
#pragma unroll
        for (int j = 0; j < PT_ITEMS; ++j)
            if (dr[j] != 0xffffffffu) s_stage[dr[j]] = w[j][0];
        if (threadIdx.x < F) s_delta[threadIdx.x] = delta_of();  // global index = delta + LDS position
        lds_barrier();
        uint32_t dest[PT_ITEMS];
#pragma unroll
        for (int k = 0; k < PT_ITEMS; ++k) {
            const uint32_t i = k * PT_THREADS + tid;
            dest[k] = 0;
            if (i < total) {
                const uint32_t v = s_stage[i];
                dest[k] = s_delta[pass_digit(pp, v, mask)] + i;
                out.w[0][dest[k]] = v;
            }
        }
        lds_barrier();
#pragma unroll
        for (int a = 1; a < NW; ++a) {
            if constexpr (PAIR >= 0) {
                if (a == PAIR + 1) continue;  // went out with word PAIR
                if (a == PAIR) {
#pragma unroll
                    for (int j = 0; j < PT_ITEMS; ++j)
                        if (dr[j] != 0xffffffffu)
                            s_stage2[dr[j]] = make_uint2(w[j][a], w[j][a + 1 < NW ? a + 1 : a]);
                    lds_barrier();
                    uint2* dst2 = reinterpret_cast<uint2*>(out.w[a]);
#pragma unroll
                    for (int k = 0; k < PT_ITEMS; ++k) {
                        const uint32_t i = k * PT_THREADS + tid;
                        if (i < total) dst2[dest[k]] = s_stage2[i];
                    }
                    lds_barrier();
                    continue;
                }
            }
#pragma unroll
            for (int j = 0; j < PT_ITEMS; ++j)
                if (dr[j] != 0xffffffffu) s_stage[dr[j]] = w[j][a];
            lds_barrier();
            uint32_t* dst = out.w[a];
#pragma unroll
            for (int k = 0; k < PT_ITEMS; ++k) {
                const uint32_t i = k * PT_THREADS + tid;
                if (i < total) dst[dest[k]] = s_stage[i];
            }
            lds_barrier();
        }
    }
