// What the channel sums of the training kernels share (csrc/train_block.hip, train_nets.hip, train_decoder.hip, train_st.hip,
// train_bn.hip).  Bit-reproducible gradients and the workspace layouts depend on every user taking the SAME slab rule, the
// same per-pixel arithmetic and the same order in which the four waves of a workgroup meet: they live here, once.
#pragma once
#include "common.h"

namespace sums {

constexpr int kMaxSlabs = 256;
constexpr int kGroup = 256;                  // channels of one workgroup of the wave-order sums: 64 lanes x 4

// The slab rule: a slab is `slab_rows` whole rows (counted through all images) of about `target` pixels, but there are at
// most kMaxSlabs slabs; a function of the shape alone, so two calls add in the same order.  `row_pixels`: the pixels a row
// stands for (W; 2 W input pixels for an output row of a stride-2 conv).  false: more than `max_rows` rows per slab.
inline bool slab_rule(long long rows, long long row_pixels, int target, int& slab_rows, int& slabs, long long max_rows = 0x7fffffffll) {
    long long sr = (target + row_pixels - 1) / row_pixels;     // rows of about `target` pixels ...
    const long long cap = (rows + kMaxSlabs - 1) / kMaxSlabs;  // ... but at most kMaxSlabs slabs
    if (sr < cap) sr = cap;
    if (sr > max_rows) return false;
    slab_rows = (int)sr;
    slabs = (int)((rows + sr - 1) / sr);
    return true;
}

// a finish kernel's store: the double sum rounded once, or added to what is there and rounded once
__device__ __forceinline__ void put(float* o, double v, int accumulate) {
    if (accumulate) v += (double)*o;
    *o = (float)v;
}

// The four waves of a 256-thread workgroup meet in wave order: lane l of every wave holds `a` for channels 4 l .. 4 l + 3 of
// the workgroup's kGroup; thread t writes ((wave 0 + wave 1) + wave 2) + wave 3 of channel t to o[t] where t < n.  `red`: 4 *
// kGroup doubles of LDS.  Every thread of the workgroup calls it (it synchronises, before and after the store).
__device__ __forceinline__ void wave_meet(double* red, const double (&a)[4], double* o, int n) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int u = 0; u < 4; ++u) red[wave * kGroup + lane * 4 + u] = a[u];
    __syncthreads();
    if (t < n) o[t] = ((red[t] + red[kGroup + t]) + red[2 * kGroup + t]) + red[3 * kGroup + t];
    __syncthreads();
}

// Where the nine taps of e of one output pixel live.  A policy answers for tap (ky, kx): row(ky) && col(kx), whether it is
// inside the picture, and at(ky, kx), the address of the lane's channel quad there.  It is built from a kernel's argument
// struct `p` (e, H, W, Ch, ...), the global output pixel `q` (counted through all images: the row inside ITS image is taken,
// so no image sees its neighbour) and the lane's first channel `c`.
//
// Stride 1: the tap is e at pixel q + dil ((ky - 1) W + (kx - 1)).  kDilated = false: dil is a compile-time 1 and `p` needs
// no such member; true: p.dil at run time.
template <bool kDilated>
struct Stride1Taps {
    static constexpr int kStride = 1;
    const float* e;
    long long q;
    int x, y, H, W, Ch, dil;
    template <class K>
    __device__ __forceinline__ Stride1Taps(const K& p, long long q_, int c) : e(p.e + c), q(q_), H(p.H), W(p.W), Ch(p.Ch), dil(1) {
        const long long row = q / W;
        x = (int)(q - row * W);
        y = (int)(row % H);
        if constexpr (kDilated) dil = p.dil;
    }
    __device__ __forceinline__ int step() const { return kDilated ? dil : 1; }
    __device__ __forceinline__ bool row(int ky) const { const int iy = y + (ky - 1) * step(); return iy >= 0 && iy < H; }
    __device__ __forceinline__ bool col(int kx) const { const int ix = x + (kx - 1) * step(); return ix >= 0 && ix < W; }
    __device__ __forceinline__ const float* at(int ky, int kx) const {
        return e + (q + (long long)(ky - 1) * step() * W + (kx - 1) * step()) * Ch;
    }
};

// Stride 2 (padding 1, dilation 1): q counts the OUTPUT pixels [n][Ho][Wo]; the tap is e at (2 oy - 1 + ky, 2 ox - 1 + kx)
// of the output row's own INPUT image [H][W]: -1 at the top and the left, H (W) below (behind) an odd size's last output.
struct Stride2Taps {
    static constexpr int kStride = 2;
    const float* e;
    int ox, oy, H, W, Ch;
    template <class K>
    __device__ __forceinline__ Stride2Taps(const K& p, long long q, int c) : H(p.H), W(p.W), Ch(p.Ch) {
        const long long row = q / p.Wo;
        ox = (int)(q - row * p.Wo);
        const long long n = row / p.Ho;
        oy = (int)(row - n * p.Ho);
        e = p.e + n * p.H * p.W * p.Ch + c;
    }
    __device__ __forceinline__ bool row(int ky) const { const int iy = 2 * oy - 1 + ky; return iy >= 0 && iy < H; }
    __device__ __forceinline__ bool col(int kx) const { const int ix = 2 * ox - 1 + kx; return ix >= 0 && ix < W; }
    __device__ __forceinline__ const float* at(int ky, int kx) const {
        return e + ((long long)(2 * oy - 1 + ky) * W + (2 * ox - 1 + kx)) * Ch;
    }
};

// One output pixel of an inverted-residual block's channel sums, for the lane's four channels: delta2 = gd where 0 < d < 6
// (fp32, as uavsal_ir_bwd forms it), S2 += delta2 into acc[0] and Gd[ky][kx] += delta2 e(tap) into acc[1 + 3 ky + kx], every
// product in double.  acc[10] (S1) is the caller's.
template <class Taps>
__device__ __forceinline__ void pixel_sums(const Taps& taps, const f32x4 dv, const f32x4 gv, double (&acc)[UAVSAL_IR_NSUM][4]) {
    f32x4 d2;
#pragma unroll
    for (int u = 0; u < 4; ++u) d2[u] = (dv[u] > 0.f && dv[u] < 6.f) ? gv[u] : 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[0][u] += (double)d2[u];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        if (!taps.row(ky)) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            if (!taps.col(kx)) continue;
            const f32x4 ev = ld4(taps.at(ky, kx));
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[1 + ky * 3 + kx][u] += (double)d2[u] * (double)ev[u];
        }
    }
}

}  // namespace sums
