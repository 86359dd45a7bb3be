// orbx_device.h — wave64 / workgroup helpers for the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace orbx {
#define ORBX_XCD_REMAP 1
// Logical (x, y) block of a 2-D grid.  Consecutive linear blocks are dealt round-robin over
// the 8 XCDs (MI355X_MICROARCH.md §Workgroup dispatch: blocks b and b + 8 share an XCD), so
// linear block L runs logical block (L mod 8) * n/8 + L / 8: every XCD walks a contiguous
// eighth of the logical order, and blocks that share halo rows, patches or an image share
// that XCD's L2.  Results never depend on the mapping.
__device__ __forceinline__ void xcd_block(int& bx, int& by) {
    const uint32_t gx = gridDim.x, n = gx * gridDim.y;
    uint32_t L = blockIdx.y * gx + blockIdx.x;
    if (ORBX_XCD_REMAP && (n & 7u) == 0) L = (L & 7u) * (n >> 3) + (L >> 3);
    by = (int)(L / gx);
    bx = (int)(L - (uint32_t)by * gx);
}


__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// Number of set bits of `mask` below this lane (v_mbcnt_lo/hi).
__device__ __forceinline__ int lanes_below(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                     __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
}

__device__ __forceinline__ int wave_incl_scan(int v) {
    const int lane = lane_id();
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        int t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// Exclusive scan across a workgroup of NW waves (default 4 = 256 threads).  `tmp` = NW ints
// of LDS.  Every thread must call it (contains barriers).
template <int NW = 4>
__device__ __forceinline__ int block_excl_scan(int v, int* tmp, int& total) {
    const int lane = lane_id(), wid = threadIdx.x >> 6;
    int incl = wave_incl_scan(v);
    if (lane == 63) tmp[wid] = incl;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        int s = tmp[w];
        base += (w < wid) ? s : 0;
        tot += s;
    }
    __syncthreads();
    total = tot;
    return base + incl - v;
}

template <int NW = 4>
__device__ __forceinline__ int block_sum(int v, int* tmp) {
    int total;
    block_excl_scan<NW>(v, tmp, total);
    return total;
}

}  // namespace orbx

namespace orbx {

// An explicit s_waitcnt vmcnt(0) (expcnt / lgkmcnt left at their maxima).  A staging loop
// (k_fast's stage_roi) waits for its loads only inside the guarded LDS stores, so on the path
// that skips a store the compiler's wait analysis still counts that load as pending, and it then inserts
// a vmcnt(0) at the next use of the register anywhere downstream -- for k_fast that was the
// head of the compass loop, which drained the next cell's prefetch on every iteration.
// Waiting once here (every load has landed by now anyway) clears that state.
__device__ __forceinline__ void vmem_drained() { __builtin_amdgcn_s_waitcnt(0x0F70); }

}  // namespace orbx
