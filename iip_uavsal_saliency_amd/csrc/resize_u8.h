// cv2.resize's 8-bit INTER_LINEAR rule, the one statement of it that letterbox.hip and overlay.hip share (letterbox.hip's
// header spells it out; tests/letterbox_ref.py is its numpy restatement).
#pragma once
#include "common.h"

// source index and the two 11-bit weights of output index d
__device__ __forceinline__ void lb_tap(int d, double scale, int n_in, int& s, int& c0, int& c1) {
    float f = (float)__dsub_rn(__dmul_rn((double)d + 0.5, scale), 0.5);
    s = (int)floorf(f);
    f = __fsub_rn(f, (float)s);
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= n_in - 1) { s = n_in - 1; f = 0.f; }
    c1 = (int)rintf(__fmul_rn(f, 2048.f));
    c0 = (int)rintf(__fmul_rn(__fsub_rn(1.f, f), 2048.f));
}

// one output byte from the four source bytes its taps name: (p00, p01) on the first source row, (p10, p11) on the second
__device__ __forceinline__ int lb_mix(int p00, int p01, int p10, int p11, int a0, int a1, int b0, int b1) {
    const int t0 = p00 * a0 + p01 * a1;
    const int t1 = p10 * a0 + p11 * a1;
    const int v = ((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16);
    return min((v + 2) >> 2, 255);
}
