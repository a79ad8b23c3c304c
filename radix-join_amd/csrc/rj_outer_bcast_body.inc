// The broadcast probe's body: k_outer_bcast (FULL false) and k_full_bcast (FULL true) include this
// text into their own bodies, with `constexpr bool FULL`, `const OuterParams& op`, `uint32_t* gflags`
// and KW / CWB / CWP in scope.  (Why an include and not a __device__ function: rj_outer_join_body.inc.)
    __shared__ __attribute__((aligned(16))) uint32_t t_w[KW + 1][JN_CAP];
    __shared__ __attribute__((aligned(16))) uint32_t t_cnt[JN_CAP / 4];
    __shared__ uint32_t s_wtot[JN_THREADS / 64];
    __shared__ unsigned long long s_obase;
    __shared__ uint32_t s_flag[FULL ? JN_RMAX / 32 : 1];
    const OuterTable<KW> T{t_w, t_cnt};
    T.clear();
    if constexpr (FULL)
        for (uint32_t i = threadIdx.x; i < JN_RMAX / 32; i += JN_THREADS) s_flag[i] = 0;
    lds_barrier();
    if (!op.keyless) {
        for (uint32_t r = threadIdx.x; r < op.B.n_rows; r += JN_THREADS) {
            uint32_t lo, hi;
            if (src_key<KW>(op.B, r, lo, hi)) T.insert(lo, hi, r);
        }
    }
    lds_barrier();
    const uint32_t n = op.P.n_rows;
    for (uint64_t base = (uint64_t)blockIdx.x * JN_SUB; base < n; base += (uint64_t)gridDim.x * JN_SUB) {
        uint32_t klo[JN_SPT], khi[JN_SPT];
        bool     probe[JN_SPT], padrow[JN_SPT], hit[JN_SPT];
#pragma unroll
        for (int j = 0; j < JN_SPT; ++j) {
            const uint64_t row = base + (uint64_t)j * JN_THREADS + threadIdx.x;
            klo[j] = khi[j] = 0;
            hit[j] = false;
            padrow[j] = row < n;
            probe[j] = row < n && !op.keyless && src_key<KW>(op.P, (uint32_t)row, klo[j], khi[j]);
        }
        outer_emit<FULL, KW, CWB, CWP, JN_SPT>(
            op, T, probe, padrow, hit, klo, khi, s_wtot, &s_obase,
            [&](uint32_t ref, uint32_t& b0, uint32_t& b1, uint32_t& b2) { src_carry<CWB>(op.B, ref, b0, b1, b2); },
            [&](int j, uint32_t& p0, uint32_t& p1, uint32_t& p2) {
                src_carry<CWP>(op.P, (uint32_t)(base + (uint64_t)j * JN_THREADS + threadIdx.x), p0, p1, p2);
            },
            s_flag, 0u);
    }
    if constexpr (FULL) {  // (outer_emit ends with a barrier: every flag of this workgroup is in LDS)
        for (uint32_t i = threadIdx.x; i < JN_RMAX / 32; i += JN_THREADS)
            if (s_flag[i]) atomicOr(&gflags[i], s_flag[i]);
    }
