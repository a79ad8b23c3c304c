// The partitioned probe's body: k_outer_join (FULL false) and k_full_join (FULL true) include this
// text into their own bodies, with `constexpr bool FULL`, `const OuterParams& op`, `uint32_t* gflags`
// and KW / CWB / CWP in scope.  (A shared __device__ __forceinline__ function would say the same, but a
// k_outer_join that only calls one compiles, ROCm 7.2 hipcc for gfx950, to 16 VGPRs more in every 32-bit-key
// shape: <1,1,1> 164 -> 180 and 3 -> 2 waves per SIMD, <1,1,0> 120 -> 136 and 4 -> 3; k_outer_bcast
// <1,1,1> 94 -> 100.  The table is in DESIGN.md section 4, "Full outer joins".  The compile-time
// switch itself lives in outer_emit.)
    constexpr int TH = JN_THREADS, SPT = JN_SPT, SUB = JN_SUB, SW = KW + CWP, BW = KW + CWB;
    constexpr uint32_t FW = JN_RMAX / 32 + 1;
    static_assert(SPT * TH == SUB, "sub-chunk geometry");
    __shared__ __attribute__((aligned(16))) uint32_t t_w[KW + 1][JN_CAP];
    __shared__ __attribute__((aligned(16))) uint32_t t_cnt[JN_CAP / 4];
    __shared__ uint32_t s_wtot[TH / 64];
    __shared__ unsigned long long s_obase;
    __shared__ uint32_t s_flag[FULL ? FW : 1];
    const OuterTable<KW> T{t_w, t_cnt};

    uint32_t q, sbeg, send;
    if (blockIdx.x < op.heavy_grid) {
        if (blockIdx.x >= *op.n_heavy) return;
        q = op.heavy_tasks[3 * blockIdx.x + 0];
        sbeg = op.heavy_tasks[3 * blockIdx.x + 1];
        send = op.heavy_tasks[3 * blockIdx.x + 2];
    } else {
        q = blockIdx.x - op.heavy_grid;
        if (q >= op.NP) return;
        sbeg = op.offP[q];
        send = op.offP[q + 1];
        if (send - sbeg > JN_HEAVY && op.offB[q + 1] != op.offB[q]) return;  // split into heavy tasks
    }
    const uint32_t rbeg = op.offB[q], rend = op.offB[q + 1];
    if (sbeg >= send) return;

    uint32_t flag_base = 0;  // FULL: the build tuple bit 0 of s_flag stands for
    // FULL: this round's flags -> HBM (word-aligned with gflags), LDS words zeroed for the next round
    auto flush_flags = [&]() {
        for (uint32_t i = threadIdx.x; i < FW; i += TH) {
            const uint32_t v = s_flag[i];
            if (v) {
                atomicOr(&gflags[(flag_base >> 5) + i], v);
                s_flag[i] = 0;
            }
        }
    };
    if constexpr (FULL)
        for (uint32_t i = threadIdx.x; i < FW; i += TH) s_flag[i] = 0;

    // one round of the table: build tuples [from, from + JN_RMAX); returns where the round ended
    auto build_round = [&](uint32_t from) -> uint32_t {
        lds_barrier();  // nobody still probes the previous round
        if constexpr (FULL) {
            flush_flags();
            flag_base = from & ~31u;
        }
        T.clear();
        lds_barrier();
        const uint32_t to = from + min((uint32_t)JN_RMAX, rend - from);
        for (uint32_t i = from + threadIdx.x; i < to; i += TH) {
            uint32_t t[BW];
            part_tuple<KW, CWB>(op.Bw, op.packB, op.aosB, i, t);
            T.insert(t[0], KW == 2 ? t[KW - 1] : 0u, i);
        }
        lds_barrier();
        return to;
    };

    uint32_t       sw[SPT][SW];
    const uint32_t first_end = build_round(rbeg);
    const bool     one_round = first_end == rend;
    for (uint32_t sc = sbeg; sc < send; sc += SUB) {
        const uint32_t sn = min((uint32_t)SUB, send - sc);
        uint32_t       klo[SPT], khi[SPT];
        bool           in[SPT], padrow[SPT], hit[SPT];
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            // (items past the chunk re-read its last tuple; they are masked off)
            part_tuple<KW, CWP>(op.Pw, op.packP, op.aosP, sc + min((uint32_t)(j * TH + threadIdx.x), sn - 1u), sw[j]);
            klo[j] = sw[j][0];
            khi[j] = KW == 2 ? sw[j][KW - 1] : 0u;
            in[j] = (uint32_t)(j * TH + threadIdx.x) < sn;
            hit[j] = false;
        }
        uint32_t end = (one_round || sc == sbeg) ? first_end : build_round(rbeg);
        while (true) {
            const bool last = end == rend;
#pragma unroll
            for (int j = 0; j < SPT; ++j) padrow[j] = last && in[j];
            outer_emit<FULL, KW, CWB, CWP, SPT>(
                op, T, in, padrow, hit, klo, khi, s_wtot, &s_obase,
                [&](uint32_t ref, uint32_t& b0, uint32_t& b1, uint32_t& b2) {
                    uint32_t t[BW];
                    part_tuple<KW, CWB>(op.Bw, op.packB, op.aosB, ref, t);
                    tuple_carry<KW, CWB>(t, b0, b1, b2);
                },
                [&](int j, uint32_t& p0, uint32_t& p1, uint32_t& p2) { tuple_carry<KW, CWP>(sw[j], p0, p1, p2); },
                s_flag, flag_base);
            if (last) break;
            end = build_round(end);
        }
    }
    if constexpr (FULL) flush_flags();  // (outer_emit ends with a barrier)
