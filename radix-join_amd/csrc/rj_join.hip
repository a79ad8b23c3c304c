// rj_join.hip — the gfx950 (wave64) build + probe kernel of the partitioned inner join: K5/K6.
#include <hip/hip_ext.h>

#include "rj_kernels.hpp"
#include "rj_kernel_util.hpp"
#include "rj_tuple_util.hpp"

#include <algorithm>
#include <type_traits>

namespace rj {

// ========================================================== K5/K6 build + probe
// Replaces the per-bucket table of the reference (src/execute.cpp:203-248):
//   build  — bucketised table in LDS: a tuple takes the next free slot of its 4-slot home
//            bucket (one LDS counter atomic), a full bucket overflows into the next one;
//            duplicate build keys simply occupy further slots;
//   probe  — one 16-byte read per bucket, four register compares; a bucket whose last slot
//            is EMPTY ends the walk; every equal key is a match (so duplicates multiply,
//            reference :232-243);
//   emit   — ballot/mbcnt offsets inside the wave, one global atomic per 4096
//            probe tuples reserves the output rows; lanes of a wave then write
//            consecutive rows of each output stream (coalesced).
// Bucket index uses hash bits ABOVE the radix bits (the reference reuses the low
// bits for both, SURVEY.md §3.2 — not copied).  EMPTY is a word whose radix bits
// differ from the partition's, so it cannot collide with a stored hashed key.
// A build partition larger than JN_RMAX is processed in table-sized chunks
// (block nested loop), which keeps any duplicate-heavy input correct.
// OM (output mode) fixes the stream layout at compile time for the two hot shapes, so the
// emit code is straight-line stores instead of a per-store mode switch:
//   OM_PAGED32  key/bc/pc are all INT32 Page images (root of a plan, BASELINE config)
//   OM_DENSE32  all present streams are dense 32-bit arrays (inner joins, row-index carries)
//   OM_GENERIC  anything else (64-bit streams, mixed layouts, no key stream)
//   OM_P32_64_64 INT32 key pages + INT64/FP64 pages for both carries (root of BASELINE config 3)
enum { OM_GENERIC = 0, OM_PAGED32 = 1, OM_DENSE32 = 2, OM_P32_64_64 = 3 };

// Diagnostic phase stamps (RJ_DIAG=1): thread 0 of every workgroup adds the cycles between
// consecutive stamps to jp.diag[phase].  Shares only — the stamps perturb the timing.
#define RJ_STAMP(PHASE)                                                         \
    do {                                                                        \
        if (jp.diag) {                                                          \
            unsigned long long _t = __builtin_amdgcn_s_memtime();               \
            if (threadIdx.x == 0) atomicAdd(&jp.diag[PHASE], _t - diag_t);      \
            diag_t = _t;                                                        \
        }                                                                       \
    } while (0)

// PK: bit 0 = the build side, bit 1 = the probe side is a packed {hashed key, carry} array
// TG: "tagged" table for one key word + a two-word build carry when the plan has >= 14 radix
//     bits.  All hashed keys of a partition share their low radix bits, so the remaining
//     (<= 18) high bits identify a key inside its partition: a slot is ONE word
//     {tag (19 bits) | build tuple index << 19} and the carries sit densely, indexed by build tuple.
//     Table = 32 KiB of slots + 32 KiB of carries (instead of three 32 KiB word arrays), so
//     two 512-thread workgroups share a CU and overlap their phases like the two-word join.
template <int KW, int CWR, int CWS, int OM, int PK, int TG>
__global__ __launch_bounds__(jn_threads(TG ? 2 : KW + CWR), jn_min_waves(TG ? 2 : KW + CWR)) void k_join(JoinParams jp) {
    // Tables of three or four word arrays (64-bit keys, two-word build carries) leave room for
    // ONE workgroup per CU; it then runs 1024 threads, so the CU holds the same 16 waves as with
    // two 512-thread workgroups.  (Fetching wide build carries from the partitioned arrays on
    // emit instead — a two-array table — cost 7 of 17 ms at 1 B rows: 2 random 4-byte reads per
    // match are bound by the request rate of the vector memory path.)
    static_assert(!TG || (KW == 1 && CWR == 2), "tagged table: one key word + two-word build carry");
    constexpr int      TH = jn_threads(TG ? 2 : KW + CWR);
    constexpr int      RPT = (JN_RMAX + TH - 1) / TH;  // build tuples per thread
    constexpr int      SPT = JN_SUB / TH;          // probe tuples per thread per sub-chunk
    constexpr int      SUB = JN_SUB;
    static_assert(RPT % 4 == 0 && SPT % 4 == 0, "tuples are loaded as 16-byte vectors");
    constexpr int      RW = KW + CWR;  // LDS table arrays (one per word)
    constexpr int      SW = KW + CWS;
    // Bucketised table: JN_CAP slots = JN_CAP/4 buckets of 4 consecutive slots.  A probe
    // reads a whole bucket with ONE 16-byte LDS read and compares in registers, an insert
    // takes its slot from ONE LDS counter atomic — so nearly every lane finishes in a single
    // iteration and the wave does not pay the longest linear-probing chain of its 64 lanes.
    // A full bucket (4th slot used) sends probe and insert on to the next bucket.
    __shared__ __attribute__((aligned(16))) uint32_t t_w[TG ? 1 : RW][JN_CAP];
    __shared__ __attribute__((aligned(16))) uint2    t_c2[TG ? JN_RMAX : 1];  // TG: carries by build tuple
    __shared__ __attribute__((aligned(16))) uint32_t t_cnt[JN_CAP / 4];
    __shared__ uint32_t s_wtot[TH / 64];
    __shared__ unsigned long long s_obase;

    const uint32_t     lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    constexpr uint32_t SMASK = JN_CAP - 1;
    constexpr uint32_t BMASK = JN_CAP / 4 - 1;

    // A workgroup joins PPW consecutive partitions (main pass) or one heavy task.
    constexpr int PPW = jn_ppw(TG ? 2 : KW + CWR);
    struct Task {
        uint32_t q, rbeg, rend, sbeg, send;
        bool     active;
    };
    // The first jp.heavy_grid workgroups of the launch take the heavy tasks (they start first:
    // with a skewed probe side they are the long pole), the others one partition each.
    const bool     heavy_wg = blockIdx.x < jp.heavy_grid;
    const uint32_t wg = heavy_wg ? blockIdx.x : blockIdx.x - jp.heavy_grid;
    // {begin, end} pairs (JoinParams::off_pairs) reach only the shapes whose sides a speculative last pass can
    // write: one key word and a carry of one or two words on BOTH sides (Exec::join_core).  Every other
    // instantiation reads neighbouring offsets as it always did — the pipelined kernels of 3- and 4-word tables,
    // which share one load between a partition's end and its successor's begin, ran 2–7 % slower with the
    // shift (profiles/spec_pass2_ab.log) — and is compiled to the code it had.
    constexpr bool PAIRS = KW == 1 && CWR >= 1 && CWR <= 2 && CWS >= 1 && CWS <= 2;
    auto get_task = [&](uint32_t k) {
        Task t{0, 0, 0, 0, 0, false};
        if (heavy_wg) {
            if (k == 0 && wg < *jp.n_heavy) {
                t.q = jp.heavy_tasks[3 * wg + 0];
                t.sbeg = jp.heavy_tasks[3 * wg + 1];
                t.send = jp.heavy_tasks[3 * wg + 2];
                const uint32_t ir = PAIRS ? t.q << (jp.off_pairs & 1u) : t.q;
                t.rbeg = jp.offR[ir];
                t.rend = jp.offR[ir + 1];
                t.active = t.rbeg < t.rend && t.sbeg < t.send;
            }
            return t;
        }
        t.q = wg * PPW + k;
        if (k < (uint32_t)PPW && t.q < jp.NP) {
            // (neighbouring offsets, or {begin, end} pairs behind a speculative last pass: JoinParams::off_pairs)
            const uint32_t ir = PAIRS ? t.q << (jp.off_pairs & 1u) : t.q, is = PAIRS ? t.q << (jp.off_pairs >> 1) : t.q;
            t.rbeg = jp.offR[ir];
            t.rend = jp.offR[ir + 1];
            t.sbeg = jp.offS[is];
            t.send = jp.offS[is + 1];
            // partitions above JN_HEAVY probe tuples are split into tasks (k_heavy_tasks)
            t.active = t.rbeg < t.rend && t.sbeg < t.send && t.send - t.sbeg <= JN_HEAVY;
        }
        return t;
    };

    // item j of a thread is element ((j/4)*TH + tid)*4 + j%4: four consecutive
    // tuples per 16-byte load
    uint32_t rw[RPT][RW];
    uint32_t sw[SPT][SW];
    // item j of a thread holds element item_index(j): four consecutive tuples per 16-byte load
    // of a word array, two consecutive {key, carry} pairs per load of a packed array
    auto item_index = [&](int j, bool packed) -> uint32_t {
        return packed ? ((j / 2) * TH + threadIdx.x) * 2 + (j % 2)
                      : ((j / 4) * TH + threadIdx.x) * 4 + (j % 4);
    };
    constexpr bool packR = (PK & 1) != 0, packS = (PK & 2) != 0;
    constexpr bool aosR = (PK & 4) != 0, aosS = (PK & 8) != 0;
    static_assert(!aosR || (KW == 1 && CWR == 2), "12-byte build tuples: key + two-word carry");
    static_assert(!aosS || (KW == 1 && CWS == 2), "12-byte probe tuples: key + two-word carry");
    // four consecutive 12-byte tuples = three 16-byte loads (dword aligned)
    auto load_aos3 = [&](const uint32_t* base, uint32_t n, auto& regs, auto n_items) {
        constexpr int NI = decltype(n_items)::value;
#pragma unroll
        for (int v = 0; v < NI / 4; ++v) {
            const uint32_t  i0 = (v * TH + threadIdx.x) * 4;
            const uint32_t* p = base + (size_t)i0 * 3;
            if (i0 + 3 < n) {
                const u32x4a x = *reinterpret_cast<const u32x4a*>(p), y = *reinterpret_cast<const u32x4a*>(p + 4),
                             z = *reinterpret_cast<const u32x4a*>(p + 8);
                regs[4 * v + 0][0] = x[0];
                regs[4 * v + 0][1] = x[1];
                regs[4 * v + 0][2] = x[2];
                regs[4 * v + 1][0] = x[3];
                regs[4 * v + 1][1] = y[0];
                regs[4 * v + 1][2] = y[1];
                regs[4 * v + 2][0] = y[2];
                regs[4 * v + 2][1] = y[3];
                regs[4 * v + 2][2] = z[0];
                regs[4 * v + 3][0] = z[1];
                regs[4 * v + 3][1] = z[2];
                regs[4 * v + 3][2] = z[3];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int a = 0; a < 3; ++a) regs[4 * v + e][a] = i0 + e < n ? p[e * 3 + a] : 0u;
            }
        }
    };
    static_assert(!packR || (KW == 1 && CWR == 1), "packed build side: key + one carry word");
    static_assert(!packS || (KW == 1 && CWS == 1), "packed probe side: key + one carry word");
    auto load_build = [&](uint32_t rc, uint32_t rn) {
        constexpr int LW = RW;
        if constexpr (aosR) {
            load_aos3(jp.R.w[0] + (size_t)rc * 3, rn, rw, std::integral_constant<int, RPT>{});
            return;
        }
        if constexpr (packR) {
            {
                const uint2* rp = reinterpret_cast<const uint2*>(jp.R.w[0]) + rc;
#pragma unroll
                for (int v = 0; v < RPT / 2; ++v) {
                    const uint32_t i0 = (v * TH + threadIdx.x) * 2;
                    if (i0 + 1 < rn) {
                        u32x4a x = *reinterpret_cast<const u32x4a*>(rp + i0);
                        rw[2 * v][0] = x[0];
                        rw[2 * v][1] = x[1];
                        rw[2 * v + 1][0] = x[2];
                        rw[2 * v + 1][1] = x[3];
                    } else {
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            uint2 t = i0 + e < rn ? rp[i0 + e] : make_uint2(0u, 0u);
                            rw[2 * v + e][0] = t.x;
                            rw[2 * v + e][1] = t.y;
                        }
                    }
                }
                return;
            }
        }
        constexpr int NA = CWR >= 2 ? KW + CWR - 2 : LW;  // plain word arrays; the last two carry words are a pair array
#pragma unroll
        for (int v = 0; v < RPT / 4; ++v) {
            const uint32_t i0 = (v * TH + threadIdx.x) * 4;
            if (i0 + 3 < rn) {
#pragma unroll
                for (int a = 0; a < NA; ++a) {
                    u32x4a x = *reinterpret_cast<const u32x4a*>(jp.R.w[a] + rc + i0);
#pragma unroll
                    for (int e = 0; e < 4; ++e) rw[4 * v + e][a] = x[e];
                }
                if constexpr (CWR >= 2) {
                    const uint32_t* p2 = jp.R.w[NA] + ((size_t)rc + i0) * 2;
                    u32x4a x = *reinterpret_cast<const u32x4a*>(p2), y = *reinterpret_cast<const u32x4a*>(p2 + 4);
                    rw[4 * v + 0][NA] = x[0];
                    rw[4 * v + 0][NA + 1] = x[1];
                    rw[4 * v + 1][NA] = x[2];
                    rw[4 * v + 1][NA + 1] = x[3];
                    rw[4 * v + 2][NA] = y[0];
                    rw[4 * v + 2][NA + 1] = y[1];
                    rw[4 * v + 3][NA] = y[2];
                    rw[4 * v + 3][NA + 1] = y[3];
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
#pragma unroll
                    for (int a = 0; a < NA; ++a)
                        rw[4 * v + e][a] = i0 + e < rn ? jp.R.w[a][rc + i0 + e] : 0u;
                    if constexpr (CWR >= 2) {
                        uint2 t = i0 + e < rn ? reinterpret_cast<const uint2*>(jp.R.w[NA])[rc + i0 + e]
                                              : make_uint2(0u, 0u);
                        rw[4 * v + e][NA] = t.x;
                        rw[4 * v + e][NA + 1] = t.y;
                    }
                }
            }
        }
    };
    auto load_probe = [&](uint32_t sc, uint32_t sn) {
        if constexpr (aosS) {
            load_aos3(jp.S.w[0] + (size_t)sc * 3, sn, sw, std::integral_constant<int, SPT>{});
            return;
        }
        if constexpr (packS) {
            {
                const uint2* sp = reinterpret_cast<const uint2*>(jp.S.w[0]) + sc;
#pragma unroll
                for (int v = 0; v < SPT / 2; ++v) {
                    const uint32_t i0 = (v * TH + threadIdx.x) * 2;
                    if (i0 + 1 < sn) {
                        u32x4a x = *reinterpret_cast<const u32x4a*>(sp + i0);
                        sw[2 * v][0] = x[0];
                        sw[2 * v][1] = x[1];
                        sw[2 * v + 1][0] = x[2];
                        sw[2 * v + 1][1] = x[3];
                    } else {
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            uint2 t = i0 + e < sn ? sp[i0 + e] : make_uint2(0u, 0u);
                            sw[2 * v + e][0] = t.x;
                            sw[2 * v + e][1] = t.y;
                        }
                    }
                }
                return;
            }
        }
        constexpr int NA = CWS >= 2 ? KW + CWS - 2 : SW;  // plain word arrays; the last two carry words are a pair array
#pragma unroll
        for (int v = 0; v < SPT / 4; ++v) {
            const uint32_t i0 = (v * TH + threadIdx.x) * 4;
            if (i0 + 3 < sn) {
#pragma unroll
                for (int a = 0; a < NA; ++a) {
                    u32x4a x = *reinterpret_cast<const u32x4a*>(jp.S.w[a] + sc + i0);
#pragma unroll
                    for (int e = 0; e < 4; ++e) sw[4 * v + e][a] = x[e];
                }
                if constexpr (CWS >= 2) {
                    const uint32_t* p2 = jp.S.w[NA] + ((size_t)sc + i0) * 2;
                    u32x4a x = *reinterpret_cast<const u32x4a*>(p2), y = *reinterpret_cast<const u32x4a*>(p2 + 4);
                    sw[4 * v + 0][NA] = x[0];
                    sw[4 * v + 0][NA + 1] = x[1];
                    sw[4 * v + 1][NA] = x[2];
                    sw[4 * v + 1][NA + 1] = x[3];
                    sw[4 * v + 2][NA] = y[0];
                    sw[4 * v + 2][NA + 1] = y[1];
                    sw[4 * v + 3][NA] = y[2];
                    sw[4 * v + 3][NA + 1] = y[3];
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
#pragma unroll
                    for (int a = 0; a < NA; ++a)
                        sw[4 * v + e][a] = i0 + e < sn ? jp.S.w[a][sc + i0 + e] : 0u;
                    if constexpr (CWS >= 2) {
                        uint2 t = i0 + e < sn ? reinterpret_cast<const uint2*>(jp.S.w[NA])[sc + i0 + e]
                                              : make_uint2(0u, 0u);
                        sw[4 * v + e][NA] = t.x;
                        sw[4 * v + e][NA + 1] = t.y;
                    }
                }
            }
        }
    };
    // one output row: key + build carry + probe carry
    auto emit_row = [&](uint64_t row, uint32_t klo, uint32_t khi, uint32_t b0, uint32_t b1,
                        uint32_t p0, uint32_t p1, uint32_t b2 = 0u, uint32_t p2 = 0u) {
        if constexpr (OM == OM_PAGED32) {
            // one page/slot computation serves all three streams
            uint32_t r = (uint32_t)row, p = r / ROWS32;
            size_t   off = (size_t)p * PAGE_BYTES + HDR32 + (r - p * ROWS32) * 4u;
            *reinterpret_cast<uint32_t*>(jp.key.base + off) = klo;
            if constexpr (CWR >= 1) *reinterpret_cast<uint32_t*>(jp.bc.base + off) = b0;
            if constexpr (CWS >= 1) *reinterpret_cast<uint32_t*>(jp.pc.base + off) = p0;
        } else if constexpr (OM == OM_P32_64_64) {
            // one page/slot computation serves both 64-bit streams
            const uint32_t r = (uint32_t)row, p4 = r / ROWS32, p8 = r / ROWS64;
            *reinterpret_cast<uint32_t*>(jp.key.base + (size_t)p4 * PAGE_BYTES + HDR32 + (r - p4 * ROWS32) * 4u) = klo;
            const size_t off8 = (size_t)p8 * PAGE_BYTES + HDR64 + (r - p8 * ROWS64) * 8u;
            *reinterpret_cast<uint2*>(jp.bc.base + off8) = make_uint2(b0, b1);
            *reinterpret_cast<uint2*>(jp.pc.base + off8) = make_uint2(p0, p1);
        } else if constexpr (OM == OM_DENSE32) {
            reinterpret_cast<uint32_t*>(jp.key.base)[row] = klo;
            if constexpr (CWR >= 1) reinterpret_cast<uint32_t*>(jp.bc.base)[row] = b0;
            if constexpr (CWS >= 1) reinterpret_cast<uint32_t*>(jp.pc.base)[row] = p0;
        } else {
            stream_store(jp.key, row, klo, khi);
            if constexpr (CWR >= 1) stream_store(jp.bc, row, b0, b1, b2);
            if constexpr (CWS >= 1) stream_store(jp.pc, row, p0, p1, p2);
        }
    };

    unsigned long long diag_t = jp.diag ? __builtin_amdgcn_s_memtime() : 0ull;
    const uint32_t     n_tasks = heavy_wg ? 1u : (uint32_t)PPW;
    Task               cur = get_task(0);
    // haveR / haveS: the first build chunk / first probe sub-chunk of `cur` already sit in
    // rw / sw (prefetched while the previous partition was being probed / before its build)
    bool haveR = false, haveS = false;
    for (uint32_t k = 0; k < n_tasks; ++k) {
        const Task nxt = get_task(k + 1);
        if (!cur.active) {
            cur = nxt;
            haveR = haveS = false;
            continue;
        }
        if (!haveR) load_build(cur.rbeg, min((uint32_t)JN_RMAX, cur.rend - cur.rbeg));
        if (!haveS) load_probe(cur.sbeg, min((uint32_t)SUB, cur.send - cur.sbeg));
        uint32_t sw_pos = cur.sbeg;  // which probe sub-chunk sw holds
        RJ_STAMP(0);  // loads issued

        // The low radix bits every hashed key of partition q shares, rebuilt from q
        // (q = ((d1*F2)+d2)*F3+d3, hash low bits = d1 | d2<<b1 | d3<<(b1+b2)); EMPTY differs
        // from them in bit 0, so no stored key can equal it.
        uint32_t qbits = 0;
        {
            uint32_t rem = cur.q, sh = jp.radix_bits;
            for (int p = (int)jp.n_pass - 1; p >= 0; --p) {
                uint32_t b = jp.pass_bits[p];
                sh -= b;
                qbits |= (rem & ((1u << b) - 1u)) << sh;
                rem >>= b;
            }
        }
        // TG: no build index reaches 0x1fff (a table holds JN_RMAX = 4096 tuples), so no slot equals
        // the all-ones word, and with >= 14 radix bits no tag (<= 18 bits) equals its 19 tag bits
        constexpr uint32_t TGB = 19, TGM = (1u << TGB) - 1u;
        static_assert(JN_RMAX <= (1u << (32 - TGB)) - 1u, "build index field of a tagged slot");
        const uint32_t EMPTY = TG ? 0xffffffffu : (qbits ^ 1u);

        for (uint32_t rc = cur.rbeg; rc < cur.rend; rc += JN_RMAX) {
            const uint32_t rn = min((uint32_t)JN_RMAX, cur.rend - rc);
            if (rc != cur.rbeg) load_build(rc, rn);
            {  // clear the key array, 16 bytes per store
                const uint4 e4 = make_uint4(EMPTY, EMPTY, EMPTY, EMPTY);
                uint4*      t4 = reinterpret_cast<uint4*>(&t_w[0][0]);
                for (uint32_t i = threadIdx.x; i < JN_CAP / 4; i += TH) t4[i] = e4;
                uint4* c4 = reinterpret_cast<uint4*>(&t_cnt[0]);
                for (uint32_t i = threadIdx.x; i < JN_CAP / 16; i += TH)
                    c4[i] = make_uint4(0, 0, 0, 0);
            }
            lds_barrier();
            RJ_STAMP(1);  // table cleared
            // ---- build
#pragma unroll
            for (int j = 0; j < RPT; ++j) {
                uint32_t i = item_index(j, packR);
                if (i < rn) {
                    uint32_t b = (rw[j][0] >> jp.radix_bits) & BMASK;
                    if constexpr (TG) t_c2[i] = make_uint2(rw[j][1], rw[j][2]);
                    while (true) {
                        uint32_t pos = atomicAdd(&t_cnt[b], 1u);
                        if (pos < 4) {
                            const uint32_t slot = b * 4 + pos;
                            if constexpr (TG) {
                                t_w[0][slot] = (rw[j][0] >> jp.radix_bits) | (i << TGB);
                            } else {
#pragma unroll
                                for (int a = 0; a < RW; ++a) t_w[a][slot] = rw[j][a];
                            }
                            break;
                        }
                        b = (b + 1) & BMASK;  // bucket full: overflow to the next one
                    }
                }
            }
            lds_barrier();
            RJ_STAMP(2);  // built
            // rw is dead now: start the NEXT partition's build loads behind this probe
            const bool last_chunk = rc + JN_RMAX >= cur.rend;
            if (last_chunk && nxt.active)
                load_build(nxt.rbeg, min((uint32_t)JN_RMAX, nxt.rend - nxt.rbeg));

            // ---- probe, SUB tuples at a time
            for (uint32_t sc = cur.sbeg; sc < cur.send; sc += SUB) {
                const uint32_t sn = min((uint32_t)SUB, cur.send - sc);
                if (sw_pos != sc) {
                    load_probe(sc, sn);
                    sw_pos = sc;
                }
                uint32_t m[SPT], f[SPT];
                // count matches, remember the first matching slot
#pragma unroll
                for (int j = 0; j < SPT; ++j) {
                    uint32_t i = item_index(j, packS);
                    m[j] = 0;
                    f[j] = 0;
                    if (i < sn) {
                        uint32_t b = (sw[j][0] >> jp.radix_bits) & BMASK;
                        while (true) {
                            const uint4 kv = *reinterpret_cast<const uint4*>(&t_w[0][b * 4]);
                            if constexpr (TG) {
                                const uint32_t tag = sw[j][0] >> jp.radix_bits;
                                const uint32_t eq = (uint32_t)((kv.x & TGM) == tag) | ((uint32_t)((kv.y & TGM) == tag) << 1) |
                                                    ((uint32_t)((kv.z & TGM) == tag) << 2) | ((uint32_t)((kv.w & TGM) == tag) << 3);
                                if (eq) {
                                    // f = build tuple index of the FIRST match (its carries: t_c2[f])
                                    if (m[j] == 0) f[j] = ((eq & 1u) ? kv.x : (eq & 2u) ? kv.y : (eq & 4u) ? kv.z : kv.w) >> TGB;
                                    m[j] += (uint32_t)__popc(eq);
                                }
                                if (kv.w == EMPTY) break;
                                b = (b + 1) & BMASK;
                                continue;
                            }
                            uint32_t    eq = (uint32_t)(kv.x == sw[j][0]) | ((uint32_t)(kv.y == sw[j][0]) << 1) |
                                          ((uint32_t)(kv.z == sw[j][0]) << 2) | ((uint32_t)(kv.w == sw[j][0]) << 3);
                            if (KW == 2 && eq) {
                                const uint4 hv = *reinterpret_cast<const uint4*>(&t_w[KW - 1][b * 4]);
                                eq &= (uint32_t)(hv.x == sw[j][KW - 1]) | ((uint32_t)(hv.y == sw[j][KW - 1]) << 1) |
                                      ((uint32_t)(hv.z == sw[j][KW - 1]) << 2) | ((uint32_t)(hv.w == sw[j][KW - 1]) << 3);
                            }
                            if (eq) {
                                if (m[j] == 0) f[j] = b * 4 + (uint32_t)__builtin_ctz(eq);
                                m[j] += (uint32_t)__popc(eq);
                            }
                            if (kv.w == EMPTY) break;  // bucket not full: nothing overflowed
                            b = (b + 1) & BMASK;
                        }
                    }
                }
                RJ_STAMP(3);  // counted
                // offsets inside the wave: ballot + mbcnt when every lane has <= 1 match
                // (the PK-FK case), shuffle scan otherwise
                uint32_t pre[SPT];
                uint32_t wave_total = 0;
#pragma unroll
                for (int j = 0; j < SPT; ++j) {
                    uint32_t tot;
                    if (__ballot(m[j] > 1) == 0) {
                        uint64_t mk = __ballot(m[j] == 1);
                        pre[j] = lane_prefix(mk);
                        tot = (uint32_t)__popcll(mk);
                    } else {
                        uint32_t incl = m[j];
#pragma unroll
                        for (int off = 1; off < 64; off <<= 1) {
                            uint32_t t = __shfl_up(incl, off);
                            if (lane >= (uint32_t)off) incl += t;
                        }
                        pre[j] = incl - m[j];
                        tot = __shfl(incl, 63);
                    }
                    pre[j] += wave_total;
                    wave_total += tot;
                }
                if (lane == 0) s_wtot[wid] = wave_total;
                lds_barrier();
                RJ_STAMP(4);  // wave prefixes + barrier
                if (threadIdx.x == 0) {
                    uint32_t tot = 0;
                    for (int w = 0; w < TH / 64; ++w) tot += s_wtot[w];
                    s_obase = tot ? atomicAdd(jp.out_cursor, (unsigned long long)tot) : 0ull;
                }
                lds_barrier();
                RJ_STAMP(5);  // output reservation
                const uint64_t gbase = s_obase;
                uint64_t       obase = gbase;
                uint32_t       block_total = 0;
                for (uint32_t w = 0; w < TH / 64; ++w) {
                    uint32_t t = s_wtot[w];
                    if (w < wid) obase += t;
                    block_total += t;
                }
                // rows beyond the stream capacity are counted but not written; the host
                // re-runs the join with exact-size buffers (out_cursor = rows needed)
                const bool fits = gbase + block_total <= jp.out_cap;
                if (fits) {
                    // the build carry of a tuple's FIRST match sits at the remembered slot
                    // f[j]: issue those reads for all tuples before the first store
                    // (TG reads them row by row instead: its registers are spoken for)
                    uint32_t c0[TG ? 1 : SPT], c1[TG ? 1 : SPT], c2[CWR == 3 ? SPT : 1];
                    if constexpr (!TG) {
#pragma unroll
                        for (int j = 0; j < SPT; ++j) {
                            c0[j] = 0;
                            c1[j] = 0;
                            if constexpr (CWR >= 1) c0[j] = m[j] ? t_w[KW][f[j]] : 0u;
                            if constexpr (CWR >= 2) c1[j] = m[j] ? t_w[KW + 1][f[j]] : 0u;
                            if constexpr (CWR == 3) c2[j] = m[j] ? t_w[KW + 2][f[j]] : 0u;
                        }
                    }
#pragma unroll
                    for (int j = 0; j < SPT; ++j) {
                        if (m[j] == 0) continue;
                        uint64_t row = obase + pre[j];
                        uint32_t klo, khi = 0;
                        unhash_key<KW>(sw[j][0], sw[j][KW - 1], klo, khi);
                        const uint32_t p0 = CWS >= 1 ? sw[j][KW < SW ? KW : 0] : 0u;
                        const uint32_t p1 = CWS >= 2 ? sw[j][KW + 1 < SW ? KW + 1 : 0] : 0u;
                        const uint32_t p2 = CWS == 3 ? sw[j][SW - 1] : 0u;
                        if constexpr (TG) {
                            const uint2 c = t_c2[f[j]];
                            emit_row(row, klo, khi, c.x, c.y, p0, p1, 0u, p2);
                        } else {
                            emit_row(row, klo, khi, c0[j], c1[j], p0, p1, CWR == 3 ? c2[CWR == 3 ? j : 0] : 0u, p2);
                        }
                        if constexpr (TG) {
                            // duplicates of the build key (rare): walk the buckets again from the
                            // home bucket and emit every match but the first
                            if (m[j] > 1) {
                                const uint32_t tag = sw[j][0] >> jp.radix_bits;
                                uint32_t       left = m[j], b = tag & BMASK;
                                while (left) {
                                    const uint4 kv = *reinterpret_cast<const uint4*>(&t_w[0][b * 4]);
                                    const uint32_t sv[4] = {kv.x, kv.y, kv.z, kv.w};
#pragma unroll
                                    for (int e = 0; e < 4; ++e) {
                                        if ((sv[e] & TGM) == tag && left) {
                                            if (left != m[j]) {  // the first match went out above
                                                ++row;
                                                const uint2 c = t_c2[sv[e] >> TGB];
                                                emit_row(row, klo, khi, c.x, c.y, p0, p1, 0u, p2);
                                            }
                                            --left;
                                        }
                                    }
                                    b = (b + 1) & BMASK;
                                }
                            }
                            continue;
                        }
                        // duplicates of the build key occupy further slots of the same run
                        uint32_t left = m[j] - 1;
                        uint32_t slot = (f[j] + 1) & SMASK;
                        while (left) {
                            bool eq = t_w[0][slot] == sw[j][0];
                            if (KW == 2) eq = eq && t_w[KW - 1][slot] == sw[j][KW - 1];
                            if (eq) {
                                ++row;
                                uint32_t b0 = 0, b1 = 0, b2 = 0;
                                if constexpr (CWR >= 1) b0 = t_w[KW][slot];
                                if constexpr (CWR >= 2) b1 = t_w[KW + 1][slot];
                                if constexpr (CWR == 3) b2 = t_w[KW + 2][slot];
                                emit_row(row, klo, khi, b0, b1, p0, p1, b2, p2);
                                --left;
                            }
                            slot = (slot + 1) & SMASK;
                        }
                    }
                }
                RJ_STAMP(6);  // emitted
                lds_barrier();  // s_wtot / s_obase are reused by the next sub-chunk
            }
            lds_barrier();  // table is cleared for the next build chunk
        }
        // sw is dead now: start the next partition's probe loads behind its table build
        if (nxt.active) load_probe(nxt.sbeg, min((uint32_t)SUB, nxt.send - nxt.sbeg));
        haveR = haveS = nxt.active;
        cur = nxt;
    }
}

// ================================================================== launchers
// tagged table (see k_join): one key word + two-word build carry, >= 14 radix bits
static bool join_tagged(int key_words, int cw_build, const JoinParams& jp) {
    return key_words == 1 && cw_build == 2 && jp.radix_bits >= 14 && jp.radix_bits <= 31;
}

template <int KW, int CWR, int CWS, int PK>
static void join_pk(const Launch& L, const JoinParams& jp, uint32_t grid) {
    const char* name = "join_build_probe";
    // (the tagged table also serves a PACKED probe side — key + one carry word, PK bit 1: the shape of
    // every join whose build side carries two words and whose probe side one; 1.45 -> 0.9 ms at 100 M rows)
    if constexpr (KW == 1 && CWR == 2 && (PK & 1) == 0) {
        const bool p366 = CWS == 2 && jp.key.mode == ST_PAGED32 && jp.bc.mode == ST_PAGED64 &&
                          jp.pc.mode == ST_PAGED64;
        if (join_tagged(KW, CWR, jp)) {
            if constexpr (CWS == 2) {
                if (p366) {
                    RJ_KLAUNCH(L, name, (k_join<KW, CWR, CWS, OM_P32_64_64, PK, 1>), grid, jn_threads(2), jp);
                    return;
                }
            }
            RJ_KLAUNCH(L, name, (k_join<KW, CWR, CWS, OM_GENERIC, PK, 1>), grid, jn_threads(2), jp);
            return;
        }
        if constexpr (CWS == 2) {
            if (p366) {
                RJ_KLAUNCH(L, name, (k_join<KW, CWR, CWS, OM_P32_64_64, PK, 0>), grid, jn_threads(KW + CWR), jp);
                return;
            }
        }
    }
    // pick the straight-line emit variant when the stream layout allows it
    int om = OM_GENERIC;
    if (KW == 1 && CWR <= 1 && CWS <= 1) {
        auto all = [&](int mode) {
            return jp.key.mode == mode && (CWR == 0 || jp.bc.mode == mode) &&
                   (CWS == 0 || jp.pc.mode == mode);
        };
        if (all(ST_PAGED32)) om = OM_PAGED32;
        if (all(ST_DENSE32)) om = OM_DENSE32;
    }
    if constexpr (KW == 1 && CWR <= 1 && CWS <= 1) {
        if (om == OM_PAGED32) {
            RJ_KLAUNCH(L, name, (k_join<KW, CWR, CWS, OM_PAGED32, PK, 0>), grid, jn_threads(KW + CWR), jp);
            return;
        }
        if (om == OM_DENSE32) {
            RJ_KLAUNCH(L, name, (k_join<KW, CWR, CWS, OM_DENSE32, PK, 0>), grid, jn_threads(KW + CWR), jp);
            return;
        }
    }
    RJ_KLAUNCH(L, name, (k_join<KW, CWR, CWS, OM_GENERIC, PK, 0>), grid, jn_threads(KW + CWR), jp);
}

// the packed / 12-byte variants exist only for the shapes that can have them
template <int KW, int CWR, int CWS>
static void join_t(const Launch& L, const JoinParams& jp, uint32_t grid) {
    constexpr int CAN = (KW == 1 && CWR == 1 ? 1 : 0) | (KW == 1 && CWS == 1 ? 2 : 0) |
                        (KW == 1 && CWR == 2 ? 4 : 0) | (KW == 1 && CWS == 2 ? 8 : 0);
    const int     pk = (jp.packR ? 1 : 0) | (jp.packS ? 2 : 0) | (jp.aosR ? 4 : 0) | (jp.aosS ? 8 : 0);
    if (pk & ~CAN) launch_failed("join_build_probe", "tuple layout flags do not fit the key/carry widths", true);
    auto packed = [&](auto... V) {  // the first layout V that is this join's: its kernel
        auto one = [&](auto v) {
            if constexpr ((CAN & v) == v)
                if (pk == v) return join_pk<KW, CWR, CWS, v>(L, jp, grid), true;
            return false;
        };
        return (... || one(V));
    };
    if (packed(int_c<1>{}, int_c<2>{}, int_c<3>{}, int_c<4>{}, int_c<8>{}, int_c<12>{}, int_c<6>{}, int_c<9>{})) return;
    if (pk != 0) launch_failed("join_build_probe", "no kernel for this tuple layout", true);
    join_pk<KW, CWR, CWS, 0>(L, jp, grid);
}

uint32_t join_partitions_per_workgroup(int key_words, int cw_build, const JoinParams& jp) {
    return (uint32_t)jn_ppw(join_tagged(key_words, cw_build, jp) ? 2 : key_words + cw_build);
}

void launch_join(const Launch& L, int key_words, int cw_build, int cw_probe, const JoinParams& jp,
                 uint32_t grid) {
    if (!grid) return;
    for_shape2("join_build_probe", key_words, cw_build, cw_probe,
               [&](auto KW, auto CWR, auto CWS) { join_t<KW, CWR, CWS>(L, jp, grid); });
}

// RJ_CTX_PREWARM: one harmless launch, so that HIP loads this translation unit's code object when the context is
// built.  A zeroed JoinParams (heavy_grid = 0, NP = 0, no diag): the workgroup is no heavy one and get_task finds no
// partition at `t.q < jp.NP`, so the task loop skips every task and the kernel ends without a load or a store.
void prewarm_join(const Launch& L, uint32_t*) {
    RJ_KLAUNCH(L, "prewarm", (k_join<1, 0, 0, OM_GENERIC, 0, 0>), 1, jn_threads(1), JoinParams{});
}

}  // namespace rj
