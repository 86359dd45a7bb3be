// Check of orbx::x86_trunc(float), orbx::x86_trunc(double) and orbx::cv_round(float)
// (my_orb_slam2_amd/csrc/orbx_math.h) against the x86-64 instructions they stand for:
// cvttss2si, cvttsd2si and cvtss2si (default MXCSR: round to nearest even).
// Test infrastructure only.  Usage: x86_cvt_check
#include "../../my_orb_slam2_amd/csrc/orbx_math.h"
#include <emmintrin.h>
#include <cstdio>
#include <cstring>

static unsigned long long checked = 0, bad_t = 0, bad_r = 0, bad_d = 0;

static void check_f(uint32_t bits) {
    volatile float x = orbx::u2f(bits);
    const int t = _mm_cvttss_si32(_mm_set_ss(x)), r = _mm_cvtss_si32(_mm_set_ss(x));
    if (orbx::x86_trunc((float)x) != t && bad_t++ < 3) printf("x86_trunc(float) mismatch %a\n", (float)x);
    if (orbx::cv_round((float)x) != r && bad_r++ < 3) printf("cv_round mismatch %a\n", (float)x);
    ++checked;
}

static void check_d(uint64_t bits) {
    double v;
    memcpy(&v, &bits, 8);
    volatile double x = v;
    if (orbx::x86_trunc((double)x) != _mm_cvttsd_si32(_mm_set_sd(x)) && bad_d++ < 3)
        printf("x86_trunc(double) mismatch %a\n", (double)x);
    ++checked;
}

static uint64_t d2u(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }

int main() {
    // every float bit pattern at a fixed odd stride over all 2^32
    for (uint64_t u = 0; u < (1ull << 32); u += 257) check_f((uint32_t)u);
    // every pattern within 64 ulps of 0, +-0.5, +-2^23, +-2^31, inf and NaN (the patterns next to
    // +-inf on the far side are NaNs; the quiet NaN 0x7fc00000 has its own neighbourhood)
    const uint32_t centres[] = {0x00000000u, 0x3f000000u, 0x4b000000u, 0x4f000000u, 0x7f800000u,
                                0x7fc00000u};
    for (uint32_t c : centres)
        for (int sign = 0; sign < 2; ++sign)
            for (int d = -64; d <= 64; ++d) {
                const int64_t m = (int64_t)c + d;
                if (m < 0 || m > 0x7fffffff) continue;
                check_f((uint32_t)m | (sign ? 0x80000000u : 0u));
            }
    // all half-integers below 2^20 in magnitude
    for (int k = 0; k < (1 << 20); ++k) {
        const float h = (float)k + 0.5f;
        check_f(orbx::f2u(h));
        check_f(orbx::f2u(-h));
    }
    // the double form: every float widened at a coarser stride, then the same neighbourhoods in
    // double ulps, and those of +-2^31 and -2^31 - 1
    for (uint64_t u = 0; u < (1ull << 32); u += 4099) check_d(d2u((double)orbx::u2f((uint32_t)u)));
    const double dcentres[] = {0.0, 0.5, 8388608.0, 2147483648.0, 2147483649.0,
                               __builtin_inf(), __builtin_nan("")};
    for (double c : dcentres)
        for (int sign = 0; sign < 2; ++sign)
            for (int d = -64; d <= 64; ++d) {
                const uint64_t base = d2u(c);
                if (d < 0 && base < (uint64_t)-d) continue;
                check_d((base + (int64_t)d) | (sign ? 1ull << 63 : 0));
            }
    printf("checked=%llu trunc_mismatch=%llu round_mismatch=%llu trunc_f64_mismatch=%llu\n",
           checked, bad_t, bad_r, bad_d);
    return (bad_t || bad_r || bad_d) ? 1 : 0;
}
