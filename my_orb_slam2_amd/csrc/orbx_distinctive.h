// orbx_distinctive.h — the 256-bit descriptor, its Hamming distance, the wave-wide minimum, and the
// median selection of MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:282-312), once, for
// k_distinctive (orbx_match.hip) and k_refresh_map_points (orbx_localmap.hip).  Device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace orbx {

struct Desc {
    uint32_t w[8];
};

// ORBmatcher::DescriptorDistance (:1715-1731): popcount of the XOR, 8 words, as a chain
// of accumulating v_bcnt_u32_b32 (the compiler otherwise sums 8 counts with 3 v_add3).
__device__ __forceinline__ uint32_t bcnt_acc(uint32_t x, uint32_t acc) {
    uint32_t r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
}

__device__ __forceinline__ int hamming(const Desc& a, const Desc& b) {
    uint32_t d = __popc(a.w[0] ^ b.w[0]);
#pragma unroll
    for (int k = 1; k < 8; ++k) d = bcnt_acc(a.w[k] ^ b.w[k], d);
    return (int)d;
}

// Wave-wide unsigned min, uniform result: DPP within rows of 16, then 4 readlanes.
// Must be called with all 64 lanes active.
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xF, 0xF, true));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xF, 0xF, true));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x124, 0xF, 0xF, true));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x128, 0xF, 0xF, true));
    const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)v, 0);
    const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
    const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)v, 32);
    const uint32_t d = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
    return min(min(a, b), min(c, d));
}

// The row of the least median (:297-312) over the N >= 1 descriptors staged at dl (8 words each,
// LDS, visible to the wave), by one wave with all 64 lanes active.  Lane i computes row i of the
// distance matrix into its own u16 row of `rows` (64 rows of row_stride >= N entries), finds the
// row's median vDists[(N-1)/2] by a binary search over distance values (9 counting passes), and a
// wave-min over (median << 16 | i) keeps the first row with the least median; more than 64
// descriptors take one such pass per 64 rows.
__device__ __forceinline__ int distinctive_best(const uint32_t* dl, uint16_t* rows, int row_stride,
                                                int N) {
    const int lane = threadIdx.x & 63;
    const int k = (N - 1) >> 1;   // vDists[0.5*(N-1)]
    uint32_t bestkey = 0xFFFFFFFFu;
    uint16_t* row = rows + lane * row_stride;
    for (int i0 = 0; i0 < N; i0 += 64) {
        const int i = i0 + lane;
        const bool has = i < N;
        const int ic = has ? i : N - 1;
        Desc di;
#pragma unroll
        for (int w = 0; w < 8; ++w) di.w[w] = dl[ic * 8 + w];
        for (int j = 0; j < N; ++j) {
            Desc dj;
#pragma unroll
            for (int w = 0; w < 8; ++w) dj.w[w] = dl[j * 8 + w];
            row[j] = (uint16_t)hamming(di, dj);
        }
        int lo = 0, hi = 256;   // smallest v with #(row <= v) >= k + 1
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            int cnt = 0;
            for (int j = 0; j < N; ++j) cnt += row[j] <= mid;
            if (cnt >= k + 1) hi = mid; else lo = mid + 1;
        }
        const uint32_t key = has ? ((uint32_t)lo << 16 | (uint32_t)i) : 0xFFFFFFFFu;
        bestkey = min(bestkey, wave_min_u32(key));
    }
    return (int)(bestkey & 0xFFFFu);
}

}  // namespace orbx
