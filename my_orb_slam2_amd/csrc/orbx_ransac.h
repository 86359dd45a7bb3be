// orbx_ransac.h — what the RANSAC solvers (orbx_sim3.hip, orbx_pnp.hip) share: everything that is
// the reference's RANSAC loop and not Horn or EPnP.  On the host the minimal-set sampling and the
// iteration count of SetRansacParameters; on both sides the window of one iterate() call and the
// cursor the scratch layouts are written with; on the device the 4x4 of a pose.  The inlier counts
// (lanes stride over N, ballot, popcount) stay written out in the kernels: through a helper that
// takes the test as a callable k_sim3_hypotheses and k_pnp_select compiled to other code.  The
// exactly rounded one-line wrappers (dv, sq, fdiv, fsqrt) are orbx_cv.h's.
// Built with -ffp-contract=off like the rest of the library: every operation is rounded on its own.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>

#include "orbx_host.h"
#include "orbx_math.h"

namespace orbx {

// The minimal sets of n_its iterations from K raw rand() values each (Sim3Solver.cc:163-177,
// PnPsolver.cc:188-201): DUtils::Random::RandomInt(0, size - 1) on vAvailableIndices, which is
// 0 .. N-1 at the start of every iteration, so the K swap-with-last steps touch at most K
// positions: pos[] / val[] hold the positions overwritten so far.
template <int K>
orbx_status sample_minimal_sets(int32_t N, int32_t n_its, const int32_t* rand_values,
                                int32_t* out) {
    if (N < K || n_its < 0 || (n_its > 0 && (!rand_values || !out))) return ORBX_ERR_INVALID;
    for (int64_t k = 0; k < K * (int64_t)n_its; ++k)
        if (rand_values[k] < 0) return ORBX_ERR_INVALID;   // RAND_MAX is INT_MAX
    for (int32_t it = 0; it < n_its; ++it) {
        int32_t pos[K], val[K];
        int nmod = 0;
        int32_t size = N;
        for (int i = 0; i < K; ++i) {
            const int randi =
                (int)(((double)rand_values[K * (size_t)it + i] / ((double)RAND_MAX + 1.0)) * size);
            auto at = [&](int32_t p) {
                int32_t v = p;
                for (int m = 0; m < nmod; ++m)
                    if (pos[m] == p) v = val[m];
                return v;
            };
            out[K * (size_t)it + i] = at(randi);
            pos[nmod] = randi;
            val[nmod] = at(size - 1);
            ++nmod;
            --size;
        }
    }
    return ORBX_OK;
}

// mRansacMaxIts at the end of SetRansacParameters (Sim3Solver.cc:128-135, PnPsolver.cc:145-152);
// epsilon is the caller's, all_inliers its mRansacMinInliers == N
inline int ransac_iterations(double prob, float epsilon, bool all_inliers, int max_its) {
    const int nIterations =
        all_inliers ? 1 : x86_trunc(::ceil(::log(1 - prob) / ::log(1 - ::pow((double)epsilon, 3.0))));
    const int lo = nIterations < max_its ? nIterations : max_its;
    return lo > 1 ? lo : 1;
}

// The iterations one iterate(n_iterations) call runs from mnIterations = iterations unless it
// returns early.  Sim3Solver.cc:158 loops while it is below mRansacMaxIts `&&` below the call's
// count, PnPsolver.cc:182 while it is below mRansacMaxIts `||` below the call's count.
__host__ __device__ __forceinline__ int ransac_window_and(int max_its, int iterations,
                                                          int n_iterations) {
    const long long left = (long long)max_its - iterations;
    const long long n = left < n_iterations ? left : (long long)n_iterations;
    return n < 0 ? 0 : (int)n;
}
__host__ __device__ __forceinline__ long long ransac_window_or(int max_its, int iterations,
                                                               int n_iterations) {
    long long w = (long long)max_its - iterations;
    if (w < n_iterations) w = n_iterations;
    return w < 0 ? 0 : w;
}

// A scratch layout is written once, as the take() calls of its scratch_of(base, ...): part after
// part from base, each a T[n0][n1][n2] rounded up to 256 bytes.  Over a null base only the size is
// of use: end.
struct ScratchCursor {
    uint8_t* p;
    size_t end = 0;
    template <class T> __host__ __device__ T* take(size_t n0, size_t n1 = 1, size_t n2 = 1) {
        T* part = (T*)p;
        const size_t bytes = al256(sizeof(T) * n0 * n1 * n2);
        p += bytes;
        end += bytes;
        return part;
    }
};

// [R | t; 0 0 0 1] as 16 floats, row-major (Mat::convertTo(CV_32F) where R and t are doubles)
template <class T> __device__ __forceinline__ void rt_to_4x4(const T* R, const T* t, float* out) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[4 * i + c] = (float)R[3 * i + c];
        out[4 * i + 3] = (float)t[i];
        out[12 + i] = 0.0f;
    }
    out[15] = 1.0f;
}

}  // namespace orbx
