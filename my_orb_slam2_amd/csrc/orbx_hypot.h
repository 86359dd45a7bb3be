// orbx_hypot.h — glibc's double hypot on the device, shared by the Jacobi SVD restatements
// (orbx_triangulate.hip, orbx_pnp.hip): lapack.cpp's JacobiSVDImpl_ calls the C library's hypot.
#pragma once
#include <hip/hip_runtime.h>

#include "orbx_cv.h"

namespace orbx {
// glibc 2.35 __hypot for finite and non-finite doubles (e_hypot.c: kernel() without
// __FP_FAST_FMA, SCALE 0x1p-600, LARGE_VAL 0x1p+511, TINY_VAL 0x1p-459, EPS 0x1p-54)
__device__ __forceinline__ double hypot_kernel(double ax, double ay) {
    double t1, t2;
    double h = sq(da(dm(ax, ax), dm(ay, ay)));
    if (h <= dm(2.0, ay)) {
        const double delta = ds(h, ay);
        t1 = dm(ax, ds(dm(2.0, delta), ax));
        t2 = dm(ds(delta, dm(2.0, ds(ax, ay))), delta);
    } else {
        const double delta = ds(h, ax);
        t1 = dm(dm(2.0, delta), ds(ax, dm(2.0, ay)));
        t2 = da(dm(ds(dm(4.0, delta), ay), ay), dm(delta, delta));
    }
    return ds(h, dv(da(t1, t2), dm(2.0, h)));
}
__device__ __forceinline__ double glibc_hypot(double x, double y) {
    if (!isfinite(x) || !isfinite(y)) {
        if (isinf(x) || isinf(y)) return INFINITY;
        return da(x, y);
    }
    x = fabs(x);
    y = fabs(y);
    const double ax = x < y ? y : x, ay = x < y ? x : y;
    if (ax > 0x1p+511) {
        if (ay <= dm(ax, 0x1p-54)) return da(ax, ay);
        return dv(hypot_kernel(dm(ax, 0x1p-600), dm(ay, 0x1p-600)), 0x1p-600);
    }
    if (ay < 0x1p-459) {
        if (ax >= dv(ay, 0x1p-54)) return da(ax, ay);
        return dm(hypot_kernel(dv(ax, 0x1p-600), dv(ay, 0x1p-600)), 0x1p-600);
    }
    if (ax >= dv(ay, 0x1p-54)) return da(ax, ay);
    return hypot_kernel(ax, ay);
}
}  // namespace orbx
