// orbx_fast_pretest.h — k_fast's compass pre-test, four pixels per 32-bit operation.
//
// A pixel is scored (fast_arc_score_pk, exact) only if the pre-test flags it, so the pre-test
// may flag too much but must never miss a pixel the exact compass test passes:
//   bright: (n0 > v + t || n8 > v + t) && (n4 > v + t || n12 > v + t)
//   dark:   (n0 < v - t || n8 < v - t) && (n4 < v - t || n12 < v - t)
// With x7 = x >> 1 and tb = (t + 1) >> 1 (t >= 1), n > v + t implies n7 >= v7 + tb and
// n < v - t implies n7 <= v7 - tb (floor((a + b) / 2) >= floor(a / 2) + floor(b / 2)), so the
// test runs on 7-bit pixels with bit 7 of every byte as the guard: H(x) = 0x80 | x7 per byte.
//
//   bright:  P = v7 + tb (<= 255, no carry), Pm = P & 0x7F.  H(n) - Pm = 0x80 + n7 - Pm lies
//            in [1, 255] (no borrow) and has bit 7 iff n7 >= Pm; P >= 0x80 means no n7 can
//            reach it, so the flag is and-ed with ~P.
//   dark:    D1 = H(v) - (tb - 1) lies in [1, 255] (no borrow) and has bit 7 iff v7 >= tb - 1;
//            e = D1 & 0x7F = v7 - tb + 1 then.  (e - 1) - H(n): every byte has e <= 0x7F <
//            0x80 <= H(n), so every byte borrows exactly one from the next and the one
//            subtracted from the whole dword is the borrow into byte 0.  The byte is
//            0x80 + (v7 - tb - n7) mod 256: bit 7 iff n7 <= v7 - tb.  And-ed with D1.
//
// Plain inline functions for host and device (tests/native/fast_pretest_test.cpp).
#pragma once
#include <stdint.h>

#include "orbx_math.h"   // ORBX_HD

namespace orbx {

constexpr uint32_t PT_LO7 = 0x7F7F7F7Fu, PT_ONES = 0x01010101u;

// The 7-bit form of four pixels.
ORBX_HD uint32_t pt_h(uint32_t x) { return (x >> 1) | 0x80808080u; }

// The thresholds of one pass in every byte: T = tb, T1 = tb - 1 (t in 1..255).
ORBX_HD uint32_t pt_T(int t) { return (uint32_t)((t + 1) >> 1) * PT_ONES; }
ORBX_HD uint32_t pt_T1(int t) { return (uint32_t)(((t + 1) >> 1) - 1) * PT_ONES; }

// Bytes s .. s + 3 of the byte run lo, hi (s in 0..3): one v_alignbyte / v_alignbit.
ORBX_HD uint32_t pt_align(uint32_t hi, uint32_t lo, int s) {
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * s));
}

// The flags of the four pixels of Hv at bits 7, 15, 23, 31 (the other bits are not zero).
// H0 / H8 are the same bytes three rows below / above, H4 / H12 three bytes to the right /
// left, all in 7-bit form.
ORBX_HD uint32_t pt_flags(uint32_t Hv, uint32_t H0, uint32_t H4, uint32_t H8, uint32_t H12,
                          uint32_t T, uint32_t T1) {
    const uint32_t P = (Hv & PT_LO7) + T;
    const uint32_t Pm = P & PT_LO7;
    const uint32_t br = ((H0 - Pm) | (H8 - Pm)) & ((H4 - Pm) | (H12 - Pm)) & ~P;
    const uint32_t D1 = Hv - T1;
    const uint32_t E1 = (D1 & PT_LO7) - 1u;
    const uint32_t dk = ((E1 - H0) | (E1 - H8)) & ((E1 - H4) | (E1 - H12)) & D1;
    return br | dk;
}

// Bits 7, 15, 23, 31 of f0 to bits 0..3 and of f1 to bits 4..7 (pixel order), on right
// shifts, ands and ors only.  a holds pixel j of f0 at bit 8j and of f1 at bit 8j + 4;
// a | a >> 7 brings pixels 1 and 3 next to pixels 0 and 2 (bits 8j - 7), and >> 14 then
// brings the pair of pixels 2, 3 (bits 16, 17 / 20, 21) down to bits 2, 3 / 6, 7.
ORBX_HD uint32_t pt_gather2(uint32_t f0, uint32_t f1) {
    const uint32_t a = ((f0 >> 7) & 0x01010101u) | ((f1 >> 3) & 0x10101010u);
    const uint32_t b = a | (a >> 7);
    return (b | (b >> 14)) & 0xFFu;
}

// The pre-test of 4 * DW adjacent pixels (DW = 4, 2 or 1 dwords).  C[0 .. DW + 1] are the
// centre row's dwords from one before the first pixel to one after the last, D / U[0 .. DW - 1]
// the pixels' own dwords three rows below / above.  Returns bit i = pixel i is flagged.
template <int DW>
ORBX_HD uint32_t pt_unit(const uint32_t* C, const uint32_t* D, const uint32_t* U, uint32_t T,
                         uint32_t T1) {
    uint32_t Hc[DW + 2], f[DW + (DW & 1)];
#pragma unroll
    for (int i = 0; i < DW + 2; ++i) Hc[i] = pt_h(C[i]);
    if (DW & 1) f[DW] = 0u;
#pragma unroll
    for (int i = 0; i < DW; ++i)
        f[i] = pt_flags(Hc[i + 1], pt_h(D[i]), pt_align(Hc[i + 2], Hc[i + 1], 3), pt_h(U[i]),
                        pt_align(Hc[i + 1], Hc[i], 1), T, T1);
    uint32_t mask = 0;
#pragma unroll
    for (int i = 0; i < DW; i += 2) mask |= pt_gather2(f[i], f[i + 1]) << (4 * i);
    return mask;
}

}  // namespace orbx
