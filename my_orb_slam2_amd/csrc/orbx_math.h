// orbx_math.h — bit-exact scalar primitives shared by host and gfx950 device code.
//
// The reference ORB path (src/ORBextractor.cc) calls three pieces of float arithmetic that
// live outside its own sources:
//   * glibc cosf/sinf           — src/ORBextractor.cc:113  (`(float)cos(angle)` on a float)
//   * OpenCV 3.2 cv::fastAtan2  — src/ORBextractor.cc:103
//   * OpenCV cvRound / cvFloor  — src/ORBextractor.cc:81,115,119-120
// A GPU has none of these, and the device libm is not glibc, so this header restates them.
//
// sinf/cosf: glibc 2.35 sysdeps/ieee754/flt-32 (s_sinf.c / s_cosf.c / sincosf.h /
// sincosf_data.c), the double-precision polynomial algorithm.  On x86-64 glibc dispatches
// by ifunc to a copy built with -mfma (`__sinf_fma`) on FMA-capable CPUs; that copy
// contracts every `a + b*c` of the polynomial and the range reduction into an fma.  The
// port below writes those fmas explicitly (glibc_madd) so the result does
// not depend on the compiler's contraction mode.  tests/test_libm_port.py checks the
// host build of this port against the real glibc over every float in [0, 2*pi).
//
// Everything here is compiled with -ffp-contract=off (host and device).
#pragma once
#include <limits.h>
#include <stdint.h>
#include <string.h>
#include <math.h>

#if defined(__HIPCC__)
#define ORBX_HD __host__ __device__ __forceinline__
#else
#define ORBX_HD static inline
#endif

namespace orbx {

ORBX_HD uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
ORBX_HD float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

// a*b+c with the rounding the glibc FMA ifunc variant uses (one rounding), or the SSE2
// variant (two roundings).
ORBX_HD double glibc_madd(double a, double b, double c) {
    return fma(a, b, c);
}

// Polynomial coefficients, __sincosf_table[0] of glibc sincosf_data.c (!TOINT_INTRINSICS).
struct SinCosTab {
    double sign0, sign1, sign2, sign3;
    double hpi_inv, hpi;
    double c0, c1, c2, c3, c4;
    double s1, s2, s3;
};

ORBX_HD SinCosTab sincos_tab(int which) {
    SinCosTab t;
    t.sign0 = 1.0; t.sign1 = -1.0; t.sign2 = -1.0; t.sign3 = 1.0;
    t.hpi_inv = 0x1.45F306DC9C883p+23;
    t.hpi = 0x1.921FB54442D18p0;
    const double s = which ? -1.0 : 1.0;
    t.c0 = s * 0x1p0;
    t.c1 = s * -0x1.ffffffd0c621cp-2;
    t.c2 = s * 0x1.55553e1068f19p-5;
    t.c3 = s * -0x1.6c087e89a359dp-10;
    t.c4 = s * 0x1.99343027bf8c3p-16;
    t.s1 = -0x1.555545995a603p-3;
    t.s2 = 0x1.1107605230bc4p-7;
    t.s3 = -0x1.994eb3774cf24p-13;
    return t;
}

ORBX_HD uint32_t abstop12(float x) { return (f2u(x) >> 20) & 0x7ff; }

// sinf_poly of glibc sincosf.h
ORBX_HD float glibc_sinf_poly(double x, double x2, const SinCosTab& p, int n) {
    if ((n & 1) == 0) {
        double x3 = x * x2;
        double s1 = glibc_madd(x2, p.s3, p.s2);
        double x7 = x3 * x2;
        double s = glibc_madd(x3, p.s1, x);
        return (float)glibc_madd(x7, s1, s);
    } else {
        double x4 = x2 * x2;
        double c2 = glibc_madd(x2, p.c4, p.c3);
        double c1 = glibc_madd(x2, p.c1, p.c0);
        double x6 = x4 * x2;
        double c = glibc_madd(x4, p.c2, c1);
        return (float)glibc_madd(x6, c2, c);
    }
}

// reduce_fast of glibc sincosf.h (scaled float->int conversion variant).
ORBX_HD double glibc_reduce_fast(double x, const SinCosTab& p, int* np) {
    double r = x * p.hpi_inv;
    int n = ((int32_t)r + 0x800000) >> 24;
    *np = n;
    return fma(-(double)n, p.hpi, x);
}

ORBX_HD double sign_of(const SinCosTab& p, int q) {
    q &= 3;
    return q == 0 ? p.sign0 : q == 1 ? p.sign1 : q == 2 ? p.sign2 : p.sign3;
}

// glibc sinf for |y| < 120 (the ORB path feeds angles in [0, 2*pi)).  Larger inputs use
// glibc's Payne-Hanek path, which the ORB path cannot reach; they return NaN here so a
// misuse is loud.
ORBX_HD float glibc_sinf(float y) {
    double x = y;
    SinCosTab p = sincos_tab(0);
    if (abstop12(y) < abstop12(0x1.921FB54442D18p-1f)) {
        double s = x * x;
        if (abstop12(y) < abstop12(0x1p-12f)) return y;
        return glibc_sinf_poly(x, s, p, 0);
    } else if (abstop12(y) < abstop12(120.0f)) {
        int n;
        x = glibc_reduce_fast(x, p, &n);
        double s = sign_of(p, n);
        if (n & 2) p = sincos_tab(1);
        return glibc_sinf_poly(x * s, x * x, p, n);
    }
    return __builtin_nanf("");
}

ORBX_HD float glibc_cosf(float y) {
    double x = y;
    SinCosTab p = sincos_tab(0);
    if (abstop12(y) < abstop12(0x1.921FB54442D18p-1f)) {
        double x2 = x * x;
        if (abstop12(y) < abstop12(0x1p-12f)) return 1.0f;
        return glibc_sinf_poly(x, x2, p, 1);
    } else if (abstop12(y) < abstop12(120.0f)) {
        int n;
        x = glibc_reduce_fast(x, p, &n);
        double s = sign_of(p, n);
        if (n & 2) p = sincos_tab(1);
        return glibc_sinf_poly(x * s, x * x, p, n ^ 1);
    }
    return __builtin_nanf("");
}

// (int) of a float as x86-64 converts it (cvttss2si): toward zero; NaN and everything outside
// int's range give INT_MIN (the GPU's v_cvt_i32_f32 saturates instead and turns NaN into 0).
ORBX_HD int x86_trunc(float f) { return (f >= -2147483648.0f && f < 2147483648.0f) ? (int)f : INT_MIN; }
// (int) of a double likewise (cvttsd2si; cvttss2si for a widened float)
ORBX_HD int x86_trunc(double v) { return (v > -2147483649.0 && v < 2147483648.0) ? (int)v : INT_MIN; }

// OpenCV cvRound(float) on x86-64 SSE2: cvtss2si with the default MXCSR, i.e.
// round-half-to-even; NaN and values outside int's range give INT_MIN.
// tests/native/x86_cvt_check.cpp checks the three against the instructions.
ORBX_HD int cv_round(float v) {
    if (!(v >= -2147483648.0f && v < 2147483648.0f)) return INT_MIN;
    return (int)rintf(v);
}

// OpenCV 3.2 cv::fastAtan2 (core/src/mathfuncs.cpp): octant reduction + 7th-order odd
// polynomial in degrees, every operation a separate float rounding.
ORBX_HD float cv_fast_atan2(float y, float x) {
    const float k180pi = (float)(180.0 / 3.14159265358979323846);
    const float p1 = 0.9997878412794807f * k180pi;
    const float p3 = -0.3258083974640975f * k180pi;
    const float p5 = 0.1555786518463281f * k180pi;
    const float p7 = -0.04432655554792128f * k180pi;
    const float eps = (float)2.2204460492503131e-16;  // (float)DBL_EPSILON
    float ax = fabsf(x), ay = fabsf(y);
    float a, c, c2;
    if (ax >= ay) {
        c = ay / (ax + eps);
        c2 = c * c;
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    } else {
        c = ax / (ay + eps);
        c2 = c * c;
        a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    }
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}

// logf: glibc 2.35 sysdeps/ieee754/flt-32 (e_logf.c, e_logf_data.c; LOGF_TABLE_BITS 4,
// LOGF_POLY_ORDER 4): log(x) = log1p(z/c - 1) + log(c) + k ln2 in double, one rounding to
// float.  MapPoint::PredictScale (src/MapPoint.cc:430-444) and Frame's mfLogScaleFactor
// (src/Frame.cc:82) call std::log on floats (TemplatedVocabulary.h:36 puts `using namespace
// std` in scope), i.e. logf.  This port equals the host glibc logf for every positive normal
// float, both with the polynomial's a*b+c contracted into fma (the __logf_fma ifunc variant)
// and without (tests/native/libm_port_check.cpp checks every one).
struct LogfEntry { double invc, logc; };
ORBX_HD LogfEntry logf_tab(int i) {
    switch (i) {
        case 0: return {0x1.661ec79f8f3bep+0, -0x1.57bf7808caadep-2};
        case 1: return {0x1.571ed4aaf883dp+0, -0x1.2bef0a7c06ddbp-2};
        case 2: return {0x1.49539f0f010bp+0, -0x1.01eae7f513a67p-2};
        case 3: return {0x1.3c995b0b80385p+0, -0x1.b31d8a68224e9p-3};
        case 4: return {0x1.30d190c8864a5p+0, -0x1.6574f0ac07758p-3};
        case 5: return {0x1.25e227b0b8eap+0, -0x1.1aa2bc79c81p-3};
        case 6: return {0x1.1bb4a4a1a343fp+0, -0x1.a4e76ce8c0e5ep-4};
        case 7: return {0x1.12358f08ae5bap+0, -0x1.1973c5a611cccp-4};
        case 8: return {0x1.0953f419900a7p+0, -0x1.252f438e10c1ep-5};
        case 9: return {0x1p+0, 0x0p+0};
        case 10: return {0x1.e608cfd9a47acp-1, 0x1.aa5aa5df25984p-5};
        case 11: return {0x1.ca4b31f026aap-1, 0x1.c5e53aa362eb4p-4};
        case 12: return {0x1.b2036576afce6p-1, 0x1.526e57720db08p-3};
        case 13: return {0x1.9c2d163a1aa2dp-1, 0x1.bc2860d22477p-3};
        case 14: return {0x1.886e6037841edp-1, 0x1.1058bc8a07ee1p-2};
        default: return {0x1.767dcf5534862p-1, 0x1.4043057b6ee09p-2};
    }
}

ORBX_HD float glibc_logf(float x) {
    uint32_t ix = f2u(x);
    if (ix == 0x3f800000u) return 0.0f;
    if (ix - 0x00800000u >= 0x7f800000u - 0x00800000u) {
        // x < 0x1p-126, inf or nan
        if (ix * 2 == 0) return -INFINITY;                 // log(+-0)
        if (ix == 0x7f800000u) return x;                   // log(inf)
        if ((ix & 0x80000000u) || ix * 2 >= 0xff000000u) return NAN;   // x < 0 or nan
        ix = f2u(x * 0x1p23f);                             // subnormal: normalize
        ix -= 23u << 23;
    }
    const uint32_t tmp = ix - 0x3f330000u;
    const int i = (int)((tmp >> (23 - 4)) % 16);
    const int k = (int32_t)tmp >> 23;
    const uint32_t iz = ix - (tmp & 0xff800000u);
    const LogfEntry e = logf_tab(i);
    const double z = (double)u2f(iz);
    const double A0 = -0x1.00ea348b88334p-2, A1 = 0x1.5575b0be00b6ap-2, A2 = -0x1.ffffef20a4123p-2;
    const double Ln2 = 0x1.62e42fefa39efp-1;
    const double r = z * e.invc - 1;
    const double y0 = e.logc + (double)k * Ln2;
    const double r2 = r * r;
    double y = A1 * r + A2;
    y = A0 * r2 + y;
    y = y * r2 + (y0 + r);
    return (float)y;
}

// sin and cos of a double for the pose optimisation (SE3Quat::exp, se3quat.h:249-254).  The
// device's double sin / cos are not glibc's, so the kernel, the C++ reference and the numpy
// restatement share this one routine instead: the fdlibm algorithm (e_rem_pio2.c
// medium path: Cody-Waite reduction by pi/2 in up to three steps; k_sin.c, k_cos.c polynomials on
// |r| <= pi/4), every operation rounded on its own.  Valid for finite |x| <= ORBX_SINCOS_F64_LIMIT
// (2^20); outside it returns false and leaves *s, *c untouched.  Below 1 ulp from the true value.
// A NaN x is outside the limit too: a caller that wants libm's sin(NaN) = cos(NaN) = NaN sets them
// itself on false, as the Sim3 solver's Rodrigues step does (theta = 2 * ang <= 2 * pi otherwise).
#define ORBX_SINCOS_F64_LIMIT 1048576.0

ORBX_HD int f64_exponent(double v) {
    uint64_t u;
    memcpy(&u, &v, 8);
    return (int)((u >> 52) & 0x7ff);
}

ORBX_HD bool orbx_sincos_f64(double x, double* s, double* c) {
    if (!(fabs(x) <= ORBX_SINCOS_F64_LIMIT)) return false;
    const double invpio2 = 6.36619772367581382433e-01;
    const double pio2_1 = 1.57079632673412561417e+00, pio2_1t = 6.07710050650619224932e-11;
    const double pio2_2 = 6.07710050630396597660e-11, pio2_2t = 2.02226624879595063154e-21;
    const double pio2_3 = 2.02226624871116645580e-21, pio2_3t = 8.47842766036889956997e-32;
    const double fn = rint(x * invpio2);
    const int n = (int)fn;
    double r = x - fn * pio2_1;
    double w = fn * pio2_1t;
    double y0 = r - w;
    const int ex = f64_exponent(x);
    if (ex - f64_exponent(y0) > 16) {
        double t = r;
        w = fn * pio2_2;
        r = t - w;
        w = fn * pio2_2t - ((t - r) - w);
        y0 = r - w;
        if (ex - f64_exponent(y0) > 49) {
            t = r;
            w = fn * pio2_3;
            r = t - w;
            w = fn * pio2_3t - ((t - r) - w);
            y0 = r - w;
        }
    }
    const double y1 = (r - y0) - w;
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03,
                 S3 = -1.98412698298579493134e-04, S4 = 2.75573137070700676789e-06,
                 S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03,
                 C3 = 2.48015872894767294178e-05, C4 = -2.75573143513906633035e-07,
                 C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double z = y0 * y0;
    const double v = z * y0;
    const double rs = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
    const double ks = y0 - ((z * (0.5 * y1 - v * rs) - y1) - v * S1);
    const double z2 = z * z;
    const double rc = z * (C1 + z * (C2 + z * C3)) + (z2 * z2) * (C4 + z * (C5 + z * C6));
    const double hz = 0.5 * z;
    const double wc = 1.0 - hz;
    const double kc = wc + (((1.0 - wc) - hz) + (z * rc - y0 * y1));
    switch (n & 3) {
        case 0: *s = ks; *c = kc; break;
        case 1: *s = kc; *c = -ks; break;
        case 2: *s = -ks; *c = -kc; break;
        default: *s = -kc; *c = ks; break;
    }
    return true;
}

// exp of a double for the Sim3 refinement (Sim3(update), sim3.h:84: s = std::exp(sigma)).  As with
// orbx_sincos_f64 the kernel, the C++ reference and the numpy restatement share this routine: the
// fdlibm algorithm (e_exp.c: x = k ln2 + r with ln2 in two parts, the rational form of
// exp(r) on |r| <= 0.5 ln2, the scaling by 2^k on the exponent field), every operation rounded on
// its own.  exp(0) = 1 exactly (|x| < 2^-28 returns 1 + x).  Valid for |x| <= ORBX_EXP_F64_LIMIT
// (700: the result is a normal double); outside it, and for a NaN, returns false and leaves *e
// untouched.  Below 1 ulp from the true value.
#define ORBX_EXP_F64_LIMIT 700.0

ORBX_HD double orbx_div_f64(double a, double b);   // below: an IEEE division on host and device

ORBX_HD bool orbx_exp_f64(double x, double* e) {
    if (!(fabs(x) <= ORBX_EXP_F64_LIMIT)) return false;
    const double ln2HI = 6.93147180369123816490e-01, ln2LO = 1.90821492927058770002e-10,
                 invln2 = 1.44269504088896338700e+00;
    const double P1 = 1.66666666666666019037e-01, P2 = -2.77777777770155933842e-03,
                 P3 = 6.61375632143793436117e-05, P4 = -1.65339022054652515390e-06,
                 P5 = 4.13813679705723846039e-08;
    uint64_t u;
    memcpy(&u, &x, 8);
    const uint32_t hx = (uint32_t)(u >> 32) & 0x7fffffffu;
    const bool neg = (u >> 63) != 0;
    double hi = 0.0, lo = 0.0;
    int k = 0;
    if (hx > 0x3fd62e42u) {                      // |x| > 0.5 ln2
        if (hx < 0x3ff0a2b2u) {                  // and |x| < 1.5 ln2
            hi = neg ? x + ln2HI : x - ln2HI;
            lo = neg ? -ln2LO : ln2LO;
            k = neg ? -1 : 1;
        } else {
            k = (int)(invln2 * x + (neg ? -0.5 : 0.5));
            const double t = (double)k;
            hi = x - t * ln2HI;
            lo = t * ln2LO;
        }
        x = hi - lo;
    } else if (hx < 0x3e300000u) {               // |x| < 2^-28
        *e = 1.0 + x;
        return true;
    }
    const double t = x * x;
    const double c = x - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))));
    if (k == 0) {
        *e = 1.0 - (orbx_div_f64(x * c, c - 2.0) - x);
        return true;
    }
    const double y = 1.0 - ((lo - orbx_div_f64(x * c, 2.0 - c)) - hi);
    uint64_t v;
    memcpy(&v, &y, 8);
    v += (uint64_t)(int64_t)k << 52;             // |k| <= 1010 and y in [0.5, 2]: a normal double
    memcpy(e, &v, 8);
    return true;
}

// atan2 of two doubles for the Sim3 solver's rotation angle (Sim3Solver.cc:278).  As with
// orbx_sincos_f64 the kernel, the C++ reference and the numpy restatement share this routine: the
// fdlibm algorithm (e_atan2.c over s_atan.c: argument reduction to one of four intervals, an odd
// polynomial of degree 23), every operation rounded on its own, with fdlibm's NaN, infinity and
// signed-zero cases.  Below 1 ulp from the true value.
// The quotients of the reduction in one place: an IEEE division on the host and on the device
// (the double `/` of device code is the correctly rounded expansion, as __ddiv_rn is).
ORBX_HD double orbx_div_f64(double a, double b) { return a / b; }

ORBX_HD double orbx_atan_f64(double x) {
    const double hi0 = 4.63647609000806093515e-01, hi1 = 7.85398163397448278999e-01,
                 hi2 = 9.82793723247329054082e-01, hi3 = 1.57079632679489655800e+00;
    const double lo0 = 2.26987774529616870924e-17, lo1 = 3.06161699786838301793e-17,
                 lo2 = 1.39033110312309984516e-17, lo3 = 6.12323399573676603587e-17;
    const double aT0 = 3.33333333333329318027e-01, aT1 = -1.99999999998764832476e-01,
                 aT2 = 1.42857142725034663711e-01, aT3 = -1.11111104054623557880e-01,
                 aT4 = 9.09088713343650656196e-02, aT5 = -7.69187620504482999495e-02,
                 aT6 = 6.66107313738753120669e-02, aT7 = -5.83357013379057348645e-02,
                 aT8 = 4.97687799461593236017e-02, aT9 = -3.65315727442169155270e-02,
                 aT10 = 1.62858201153657823623e-02;
    uint64_t u;
    memcpy(&u, &x, 8);
    const int32_t hx = (int32_t)(u >> 32);
    const uint32_t lx = (uint32_t)u;
    const int32_t ix = hx & 0x7fffffff;
    if (ix >= 0x44100000) {                      // |x| >= 2^66
        if (ix > 0x7ff00000 || (ix == 0x7ff00000 && lx != 0)) return x + x;   // NaN
        return hx > 0 ? hi3 + lo3 : -hi3 - lo3;
    }
    int id;
    double hi = 0.0, lo = 0.0;
    if (ix < 0x3fdc0000) {                       // |x| < 0.4375
        if (ix < 0x3e200000) return x;           // |x| < 2^-29
        id = -1;
    } else {
        x = fabs(x);
        if (ix < 0x3ff30000) {
            if (ix < 0x3fe60000) { id = 0; hi = hi0; lo = lo0; x = orbx_div_f64(2.0 * x - 1.0, 2.0 + x); }
            else { id = 1; hi = hi1; lo = lo1; x = orbx_div_f64(x - 1.0, x + 1.0); }
        } else {
            if (ix < 0x40038000) { id = 2; hi = hi2; lo = lo2; x = orbx_div_f64(x - 1.5, 1.0 + 1.5 * x); }
            else { id = 3; hi = hi3; lo = lo3; x = orbx_div_f64(-1.0, x); }
        }
    }
    const double z = x * x;
    const double w = z * z;
    const double s1 = z * (aT0 + w * (aT2 + w * (aT4 + w * (aT6 + w * (aT8 + w * aT10)))));
    const double s2 = w * (aT1 + w * (aT3 + w * (aT5 + w * (aT7 + w * aT9))));
    if (id < 0) return x - x * (s1 + s2);
    const double r = hi - ((x * (s1 + s2) - lo) - x);
    return hx < 0 ? -r : r;
}

ORBX_HD double orbx_atan2_f64(double y, double x) {
    const double tiny = 1.0e-300, pi_o_4 = 7.8539816339744827900E-01,
                 pi_o_2 = 1.5707963267948965580E+00, pi = 3.1415926535897931160E+00,
                 pi_lo = 1.2246467991473531772E-16;
    uint64_t ux, uy;
    memcpy(&ux, &x, 8);
    memcpy(&uy, &y, 8);
    const int32_t hx = (int32_t)(ux >> 32), hy = (int32_t)(uy >> 32);
    const uint32_t lx = (uint32_t)ux, ly = (uint32_t)uy;
    const int32_t ix = hx & 0x7fffffff, iy = hy & 0x7fffffff;
    if ((uint32_t)ix + (lx != 0) > 0x7ff00000u || (uint32_t)iy + (ly != 0) > 0x7ff00000u)
        return x + y;                            // NaN
    if (hx == 0x3ff00000 && lx == 0) return orbx_atan_f64(y);   // x = 1.0
    const int m = ((hy >> 31) & 1) | ((hx >> 30) & 2);          // 2 * sign(x) + sign(y)
    if ((iy | ly) == 0) {                        // y = 0
        if (m < 2) return y;
        return m == 2 ? pi + tiny : -pi - tiny;
    }
    if ((ix | lx) == 0) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;   // x = 0
    if (ix == 0x7ff00000) {                      // x infinite
        if (iy == 0x7ff00000)
            return m == 0 ? pi_o_4 + tiny : m == 1 ? -pi_o_4 - tiny
                 : m == 2 ? 3.0 * pi_o_4 + tiny : -3.0 * pi_o_4 - tiny;
        return m == 0 ? 0.0 : m == 1 ? -0.0 : m == 2 ? pi + tiny : -pi - tiny;
    }
    if (iy == 0x7ff00000) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
    const int32_t k = (iy - ix) >> 20;
    double z;
    if (k > 60) z = pi_o_2 + 0.5 * pi_lo;        // |y / x| > 2^60
    else if (hx < 0 && k < -60) z = 0.0;         // |y| / x < -2^60
    else z = orbx_atan_f64(fabs(orbx_div_f64(y, x)));
    switch (m) {
        case 0: return z;
        case 1: return -z;
        case 2: return pi - (z - pi_lo);
        default: return (z - pi_lo) - pi;
    }
}

}  // namespace orbx
