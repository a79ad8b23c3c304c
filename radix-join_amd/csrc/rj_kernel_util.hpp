// rj_kernel_util.hpp — what every kernel file but rj_ingest.hip and rj_varchar_dev.hip shares: wave / workgroup
// helpers, column loads and the launch macro.  Device code: include from a .hip file only.
#pragma once
#include <hip/hip_ext.h>

#include "rj_kernels.hpp"

namespace rj {

// lanes below me whose bit is set in `mask` (wave64)
__device__ __forceinline__ uint32_t lane_prefix(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                     __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for
// vmcnt(0), i.e. for every outstanding global load AND store of the wave; the kernels
// below never hand global data from wave to wave inside a launch, so their barriers only
// need the LDS counter drained — global stores then retire asynchronously behind the
// next phase instead of stalling every barrier.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// threadIdx.x as a value the compiler cannot see through.  What is derived from it inside a loop is
// computed there: derived from threadIdx.x itself, a tile loop's per-lane indices and offsets (a few
// dozen of them in the scatter kernels) are hoisted out of the loop and occupy registers, or spill,
// through the phases that need every register for loads in flight.
__device__ __forceinline__ uint32_t tile_tid() {
    uint32_t t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}

// Exclusive scan of one value per thread across the workgroup (blockDim.x a
// multiple of 64, at most 1024).  s_wsum needs blockDim.x/64 words.  Contains
// one barrier; the caller must sync again before reusing s_wsum.
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* s_wsum, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint32_t       incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        uint32_t t = __shfl_up(incl, off);
        if (lane >= (uint32_t)off) incl += t;
    }
    if (lane == 63) s_wsum[wid] = incl;
    lds_barrier();
    uint32_t wbase = 0, tot = 0;
    for (uint32_t k = 0; k < nw; ++k) {
        uint32_t s = s_wsum[k];
        if (k < wid) wbase += s;
        tot += s;
    }
    total = tot;
    return wbase + incl - v;
}

__device__ __forceinline__ uint32_t col_load32(const ColRef& c, uint32_t row) {
    if (c.kind == COL_PAGED) {
        uint32_t p = row / ROWS32, i = row - p * ROWS32;
        return *reinterpret_cast<const uint32_t*>(c.ptr + (size_t)p * PAGE_BYTES + HDR32 + i * 4u);
    } else if (c.kind == COL_DENSE) {
        return reinterpret_cast<const uint32_t*>(c.ptr)[row];
    }
    return row;  // COL_IOTA
}
__device__ __forceinline__ uint64_t col_load64(const ColRef& c, uint32_t row) {
    if (c.kind == COL_PAGED) {
        uint32_t p = row / ROWS64, i = row - p * ROWS64;
        return *reinterpret_cast<const uint64_t*>(c.ptr + (size_t)p * PAGE_BYTES + HDR64 + i * 8u);
    } else if (c.kind == COL_DENSE) {
        return reinterpret_cast<const uint64_t*>(c.ptr)[row];
    }
    return row;
}

}  // namespace rj

// A rejected launch (LDS or launch-bounds mismatch of a tuning variant, wrong device) must not
// pass silently: the stream would "succeed" and the join return stale buffers with RJ_OK.
#define RJ_KLAUNCH(L, NAME, KERNEL, GRID, BLOCK, ...)                                          \
    do {                                                                                       \
        hipEvent_t _ev0 = nullptr, _ev1 = nullptr;                                             \
        if ((L).logged) (L).logged((L).self, reinterpret_cast<const void*>(KERNEL));           \
        if ((L).timed && (L).timed((L).self, NAME, &_ev0, &_ev1))                              \
            hipExtLaunchKernelGGL(KERNEL, dim3(GRID), dim3(BLOCK), 0, (L).stream, _ev0, _ev1,  \
                                  0, __VA_ARGS__);                                             \
        else                                                                                   \
            hipLaunchKernelGGL(KERNEL, dim3(GRID), dim3(BLOCK), 0, (L).stream, __VA_ARGS__);   \
        hipError_t _le = hipGetLastError();                                                    \
        if (_le != hipSuccess) launch_failed(NAME, hipGetErrorString(_le), false);             \
    } while (0)
