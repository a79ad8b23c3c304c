// rj_pass_scatter_packed.inc — the body of k_pass_scatter_packed and of k_spec_scatter_packed (rj_partition.hip),
// which include it with Loader, BLK_OUT, SPEC, SPEC_LAST and ld, pp, out, sp in scope (see rj_pass_scatter.inc).
    __shared__ uint2    s_stage[PT_TILE];
    __shared__ uint32_t s_cnt[PT_MAXF];
    __shared__ uint32_t s_base[PT_MAXF];
    __shared__ uint32_t s_delta[PT_MAXF];
    __shared__ uint32_t s_wsum[PT_THREADS / 64];
    uint32_t            seg, begin, end;
    if (!group_range(pp, blockIdx.x, seg, begin, end)) return;
    const uint32_t F = 1u << pp.fanout_log2, mask = F - 1u;
    // (SPEC_LAST: see rj_pass_scatter.inc)
    __shared__ uint32_t s_limit[SPEC && SPEC_LAST ? PT_MAXF : 1];
    if constexpr (SPEC && SPEC_LAST) {
        if (threadIdx.x < F) s_limit[threadIdx.x] = last_limit(sp)[(size_t)seg * F + threadIdx.x];
    }

    uint32_t run = 0;  // thread d: where digit d's run of the current tile starts in the output
    [[maybe_unused]] unsigned long long res = 0;  // SPEC: what the reservation returned, {position, room}
    // the next tile's loads are issued as soon as this tile has been staged (its registers are
    // dead then) and fly during the copy-out
    uint32_t w[PT_ITEMS][2];
    uint32_t ok_raw = ld.template issue_tile<2>(begin, end, w);
    for (uint32_t base = begin; base < end; base += PT_TILE) {
        for (uint32_t d = threadIdx.x; d < F; d += PT_THREADS) s_cnt[d] = 0;
        lds_barrier();

        uint32_t       dr[PT_ITEMS];  // digit << 16 | rank, 0xffffffff = no tuple
        const uint32_t ok = ld.template finish_tile<2>(base, end, ok_raw, w);  // (source tuples: NULL drop + hashing)
#pragma unroll
        for (int j = 0; j < PT_ITEMS; ++j) {
            dr[j] = 0xffffffffu;
            if ((ok >> j) & 1u) {
                uint32_t d = pass_digit(pp, w[j][0], mask);
                uint32_t r = atomicAdd(&s_cnt[d], 1u);
                dr[j] = (d << 16) | r;
            }
        }
        lds_barrier();

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

#pragma unroll
        for (int j = 0; j < PT_ITEMS; ++j)
            if (dr[j] != 0xffffffffu)
                s_stage[s_base[dr[j] >> 16] + (dr[j] & 0xffffu)] = make_uint2(w[j][0], w[j][1]);
        if (base + PT_TILE < end) ok_raw = ld.template issue_tile<2>(base + PT_TILE, end, w);
        if (threadIdx.x < F) {  // global index = delta + LDS position
            if constexpr (SPEC && SPEC_LAST) {
                if (c && run + c > s_limit[threadIdx.x]) {
                    atomicOr(sp.flag, 1u);
                    s_delta[threadIdx.x] = sp.sink;
                } else {
                    s_delta[threadIdx.x] = run - ex;
                }
            } else if constexpr (SPEC) {
                if (c && (int32_t)(uint32_t)(res >> 32) < (int32_t)c) {  // the run does not fit: to the spare tile
                    atomicOr(sp.flag, 1u);
                    s_delta[threadIdx.x] = sp.sink;
                } else {
                    s_delta[threadIdx.x] = (uint32_t)res - ex;
                }
            } else {
                s_delta[threadIdx.x] = run - ex;
            }
        }
        lds_barrier();

#pragma unroll
        for (int k = 0; k < PT_ITEMS; ++k) {
            const uint32_t i = k * PT_THREADS + threadIdx.x;
            if (i < total) {
                const uint2    v = s_stage[i];
                const uint32_t g = s_delta[pass_digit(pp, v.x, mask)] + i;
                if constexpr (BLK_OUT) {  // (see BlockedLoader)
                    uint32_t* o = reinterpret_cast<uint32_t*>(out) + BlockedLoader::key_at(g);
                    o[0] = v.x;
                    o[BlockedLoader::BLK] = v.y;
                } else {
                    out[g] = v;
                }
                if (pp.side_out) pp.side_out[g] = (uint16_t)((v.x >> pp.next_shift) & pp.next_mask);
            }
        }
        // no barrier: the next tile passes two barriers before it overwrites s_stage / s_delta
    }
