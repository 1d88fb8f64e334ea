// Repacking refreshed weights on the device: what packing.py / weights.py do on the host after an optimiser step, from the
// module's fp32 parameters and buffers where they lie to the packed device tensors the launch plans hold the addresses of.
// include/uavsal_hip.h states the table and every formula.
//
// ONE launch for a whole refresh.  The table lists one entry per packed tensor; behind it lies a prefix array of block
// counts, and a workgroup finds its entry by a binary search in it (uniform over the workgroup: scalar loads, no
// divergence).  A thread owns one UNIT of its entry's destination and writes it once:
//   conv   16 bytes: four consecutive k of one row (fp32) or eight consecutive halves of one 32-run (16-bit layouts);
//          every value is one gather from the parameter plus, for the 16-bit layouts, the split
//   wino   one (o, c): the nine taps are read once, all P * P values of U = G g G^T leave for their matrices
//   fold   one channel of a folded BatchNorm vector (scale, bias, 1 / sqrt(var + eps), mean), identity padding included
//   dw     one element of the tap-major [9][C] depthwise weights
//   copy   one float
// Padding is written every time (zeros, or the identity of a fold).  No atomics, no LDS, no cross-thread traffic: the bytes
// are a function of the parameters alone.
//
// Arithmetic: the host packer never fuses a multiply with an add, so nothing here may be contracted -- the pragma below
// covers the file, and the products and sums that matter are spelled with the __*_rn intrinsics as well.  Divides and
// square roots are the correctly rounded ones (no fast-math flag in the build).
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxSrc = UAVSAL_REPACK_MAX_SRC;

// the source (of up to kMaxSrc lying side by side) that holds row `m`; m becomes the row inside it
__device__ __forceinline__ int find_src(const uavsal_repack_entry& e, int& m) {
    int s = 0;
    while (s + 1 < e.n_src && m >= e.rows[s]) ++s;
    if (s) m -= e.rows[s - 1];
    return s;
}

// one element of the logical [Npad][Kpad] weight matrix of a conv entry (packing.pack_conv_weight's `m`)
__device__ __forceinline__ float conv_value(const uavsal_repack_entry& e, int n, int k) {
    if (n >= e.N || k >= e.C * e.taps) return 0.f;
    int c = k, tap = 0;
    if (e.taps == 9) {                                  // channel-block-major, tap-minor: k = ((c / kt) * 9 + tap) * kt + c % kt
        const int blk = k / (9 * e.kt), rem = k - blk * 9 * e.kt;
        tap = rem / e.kt;
        c = blk * e.kt + (rem - tap * e.kt);
    }
    int m = e.gi ? (n & 3) * e.gi + (n >> 2) : n;       // ConvLSTM gate rows: packed row 4 c + g <- row g * hid + c
    const int s = find_src(e, m);
    const int st = e.flip ? e.taps - 1 - tap : tap;
    float v = e.src[s][e.off + (long long)m * e.sN + (long long)c * e.sC + st];
    if (e.sg) {                                         // the folded scale of the BatchNorm behind the conv, fp64 fold rounded once
        const double sc = __ddiv_rn((double)e.sg[c], __dsqrt_rn(__dadd_rn((double)e.sv[c], e.seps)));
        v = __fmul_rn(v, (float)sc);
    }
    return v;
}

__device__ __forceinline__ unsigned short bf16_rne(float x) {      // round to nearest even, NaN -> the quiet NaN torch writes
    const unsigned u = __builtin_bit_cast(unsigned, x);
    if (x != x) return 0x7fc0;
    return (unsigned short)((u + (0x7fffu + ((u >> 16) & 1u))) >> 16);
}

__device__ __forceinline__ unsigned short half_of(const uavsal_repack_entry& e, int n, int k, int panel) {
    float m = conv_value(e, n, k);
    if (e.layout == UAVSAL_REPACK_BF16 || e.layout == UAVSAL_REPACK_BF16X3) {
        const unsigned short hi = bf16_rne(m);
        if (!panel) return hi;
        return bf16_rne(__fsub_rn(m, __builtin_bit_cast(float, (unsigned)hi << 16)));
    }
    m = __fmul_rn(m, 64.0f);
    const _Float16 hi = (_Float16)m;                    // v_cvt_f16_f32: round to nearest even, overflow to inf as the host does
    if (!panel) return __builtin_bit_cast(unsigned short, hi);
    const _Float16 lo = (_Float16)__fsub_rn(m, (float)hi);
    return __builtin_bit_cast(unsigned short, lo);
}

__device__ __forceinline__ void conv_unit(const uavsal_repack_entry& e, long long u) {
    const int npad = e.Npad;
    if (e.layout == UAVSAL_REPACK_F32) {                // [Npad][Kpad] floats, Kpad % 16 == 0
        const long long e0 = u * 4;
        const int n = (int)(e0 / e.Kpad), k0 = (int)(e0 - (long long)n * e.Kpad);
        f32x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = conv_value(e, n, k0 + i);
        reinterpret_cast<f32x4*>(e.dst)[u] = v;
        return;
    }
    const long long e0 = u * 8;                         // eight halves of one run
    int n, panel, j0, kbase;
    bool perm = true;
    if (e.layout == UAVSAL_REPACK_F16X3J) {             // [Kpad / 16][Npad][hi 16 | lo 16]
        j0 = (int)(e0 & 15);
        panel = (int)((e0 >> 4) & 1);
        n = (int)((e0 >> 5) % npad);
        kbase = (int)((e0 >> 5) / npad) * 16;
        perm = false;
    } else if (e.layout == UAVSAL_REPACK_F16X3I) {      // [Kpad / 32][Npad][hi 32 | lo 32]
        j0 = (int)(e0 & 31);
        panel = (int)((e0 >> 5) & 1);
        n = (int)((e0 >> 6) % npad);
        kbase = (int)((e0 >> 6) / npad) * 32;
        perm = false;
    } else if (e.layout == UAVSAL_REPACK_BF16) {        // [Kpad / 32][Npad][32]
        j0 = (int)(e0 & 31);
        panel = 0;
        n = (int)((e0 >> 5) % npad);
        kbase = (int)((e0 >> 5) / npad) * 32;
    } else {                                            // f16x3, bf16x3: [Kpad / 32][hi | lo][Npad][32]
        j0 = (int)(e0 & 31);
        const long long run = e0 >> 5;
        n = (int)(run % npad);
        panel = (int)((run / npad) & 1);
        kbase = (int)(run / (2ll * npad)) * 32;
    }
    unsigned short h[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int j = j0 + i;                           // the permuted runs hold chunk c = {4c..4c+3, 16+4c..16+4c+3}
        const int k = perm ? ((j & 4) ? 16 : 0) + 4 * (j >> 3) + (j & 3) : j;
        h[i] = half_of(e, n, kbase + k, panel);
    }
    u32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (unsigned)h[2 * i] | ((unsigned)h[2 * i + 1] << 16);
    reinterpret_cast<u32x4*>(e.dst)[u] = o;
}

// U = G g G^T in double, in ONE fixed order: t[i][k] = (G[i][0] g[0][k] + G[i][1] g[1][k]) + G[i][2] g[2][k], then
// U[i][l] = (t[i][0] G[l][0] + t[i][1] G[l][1]) + t[i][2] G[l][2]; each U rounded once to fp32
__device__ __forceinline__ void wino_unit(const uavsal_repack_entry& e, long long u) {
    const int o = (int)(u / e.Kpad), c = (int)(u - (long long)o * e.Kpad);
    const int P = e.P;
    const long long plane = (long long)e.Npad * e.Kpad;
    float* dst = reinterpret_cast<float*>(e.dst) + (long long)o * e.Kpad + c;
    if (o >= e.N || c >= e.C) {
        for (int q = 0; q < P * P; ++q) dst[q * plane] = 0.f;
        return;
    }
    const float* g = e.src[0] + e.off + (long long)o * e.sN + (long long)c * e.sC;
    double w[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) w[q] = (double)g[q];
    for (int i = 0; i < P; ++i) {
        const double g0 = e.G[3 * i], g1 = e.G[3 * i + 1], g2 = e.G[3 * i + 2];
        double t[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            t[k] = __dadd_rn(__dadd_rn(__dmul_rn(g0, w[k]), __dmul_rn(g1, w[3 + k])), __dmul_rn(g2, w[6 + k]));
        for (int l = 0; l < P; ++l) {
            const double v = __dadd_rn(__dadd_rn(__dmul_rn(t[0], e.G[3 * l]), __dmul_rn(t[1], e.G[3 * l + 1])),
                                       __dmul_rn(t[2], e.G[3 * l + 2]));
            dst[(long long)(i * P + l) * plane] = (float)v;
        }
    }
}

// one channel of a folded BatchNorm vector: scale = g / sqrt(v + eps), bias = b - m scale, rstd = 1 / sqrt(v + eps), all in
// double and rounded once; mean is copied.  Channels at and behind N hold the identity `pad`.
__device__ __forceinline__ void fold_unit(const uavsal_repack_entry& e, long long u) {
    float* dst = reinterpret_cast<float*>(e.dst);
    int c = (int)u;
    if (c >= e.N) {
        dst[u] = e.pad;
        return;
    }
    const int s = find_src(e, c);
    if (e.layout == UAVSAL_REPACK_MEAN) {
        dst[u] = e.mean[s][c];
        return;
    }
    const double root = __dsqrt_rn(__dadd_rn((double)e.var[s][c], e.eps[s]));
    if (e.layout == UAVSAL_REPACK_RSTD) {
        dst[u] = (float)__ddiv_rn(1.0, root);
        return;
    }
    const double scale = __ddiv_rn((double)e.src[s][c], root);
    if (e.layout == UAVSAL_REPACK_SCALE) {
        dst[u] = (float)scale;
        return;
    }
    dst[u] = (float)__dsub_rn((double)e.beta[s][c], __dmul_rn((double)e.mean[s][c], scale));
}

__global__ __launch_bounds__(kThreads) void repack_kernel(const uavsal_repack_entry* __restrict__ table,
                                                          const int* __restrict__ first_block, int n_entries) {
    const int b = (int)blockIdx.x;
    int lo = 0, hi = n_entries;                         // the entry with first_block[lo] <= b < first_block[lo + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first_block[mid] <= b) lo = mid; else hi = mid;
    }
    const uavsal_repack_entry& e = table[lo];
    const long long u = (long long)(b - first_block[lo]) * kThreads + threadIdx.x;
    if (u >= e.units) return;
    switch (e.kind) {
    case UAVSAL_REPACK_CONV: conv_unit(e, u); break;
    case UAVSAL_REPACK_WINO: wino_unit(e, u); break;
    case UAVSAL_REPACK_FOLD: fold_unit(e, u); break;
    case UAVSAL_REPACK_DW: {                            // tap-major [9][N] from [C_s][3][3] weights side by side
        const int tap = (int)(u / e.N);
        int c = (int)(u - (long long)tap * e.N);
        const int s = find_src(e, c);
        reinterpret_cast<float*>(e.dst)[u] = e.src[s][(long long)c * 9 + tap];
        break;
    }
    case UAVSAL_REPACK_COPY: reinterpret_cast<float*>(e.dst)[u] = e.src[0][u]; break;
    case UAVSAL_REPACK_COPY_T: {                        // [C][N] from src[0] = [N][C]: u = c * N + n
        const int c = (int)(u / e.N), n = (int)(u - (long long)c * e.N);
        reinterpret_cast<float*>(e.dst)[u] = e.src[0][(long long)n * e.C + c];
        break;
    }
    default: break;
    }
}

}  // namespace

extern "C" int uavsal_repack_sizeof_desc(void) { return (int)sizeof(uavsal_repack_entry); }

extern "C" int uavsal_repack(const void* table, int n_entries, int n_blocks, uavsal_stream_t stream) {
    if (!table || n_entries <= 0 || n_blocks <= 0) return UAVSAL_EINVAL;
    if (n_blocks >= UAVSAL_REPACK_MAX_BLOCKS) return UAVSAL_ESHAPE;          // 256 threads each: under 2^32 threads a launch
    if (!uavsal_aligned16(table)) return UAVSAL_EALIGN;
    static_assert(sizeof(uavsal_repack_entry) % 8 == 0, "the prefix array lies behind the entries");
    const uavsal_repack_entry* entries = static_cast<const uavsal_repack_entry*>(table);
    const int* first_block = reinterpret_cast<const int*>(entries + n_entries);
    hipLaunchKernelGGL(repack_kernel, dim3((unsigned)n_blocks), dim3(kThreads), 0, (hipStream_t)stream, entries, first_block, n_entries);
    return uavsal_launch_status();
}
