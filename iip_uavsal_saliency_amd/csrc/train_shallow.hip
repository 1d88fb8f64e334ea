// The skinny weight-gradient GEMM of the shallow MobileNetV2 blocks features[2:8] (include/uavsal_hip.h states the contract
// and the partition): out[m][n] = row_scale[m] sum over pixels p of A[p][m] B[p][n] with one side at most 32 wide and the
// other at most 192 -- 96 x 16, 144 x 24, 24 x 96, 24 x 144, 32 x 144 -- over up to 1,152,000 pixels.
//
// 1. skinny_wgrad_kernel: the products are memory bound ((M + N) * 4 bytes against 2 M N flop per pixel: 7 to 21 flop per
//    byte), so the kernel is built around ONE pass over both operands, not around the MFMA.  A WAVE owns a share of the
//    pixels and the WHOLE M x N result: kWide accumulators of v_mfma_f32_32x32x2_f32 (the narrow side is one tile, the wide
//    side ceil(wide / 32)), so no operand byte is fetched twice and no workgroup re-reads the narrow operand per tile of the
//    wide one, as pix_gemm32_kernel (csrc/train_decoder.hip) does.  The operands are read from global memory in the MFMA's
//    own layout (lane l: pixel p + (l >> 5), column (l & 31) of a tile: two 128-byte rows per tile and instruction), kLoads
//    pixel pairs in flight; columns behind a side's width are zeros in registers and are never read.  No LDS, no barrier.
//    1024 shares at most: one wave per SIMD of the 256 CUs, 6 to 8 KB of loads in flight per wave at the five shapes.  Four
//    shares to a workgroup.  Chains of at most UAVSAL_WGRAD_CHAIN products, as in every other weight gradient.
// 2. skinny_reduce_kernel: a workgroup of 1024 threads per row m: floor(1024 / N) groups of consecutive shares are summed in
//    share order in double side by side (1024 shares on 24 to 144 rows would otherwise be one long dependent walk per
//    thread), then the groups in group order; uavsal_pix_gemm's scale, store and rowdot.
#include "common.h"

namespace {

constexpr int kUnit = UAVSAL_SKINNY_UNIT, kMaxShares = UAVSAL_SKINNY_SHARES;
constexpr int kMaxNarrow = UAVSAL_SKINNY_MAX_NARROW, kMaxWide = UAVSAL_SKINNY_MAX_WIDE;
constexpr int kRedThreads = 1024;

struct SkK {
    const float *a, *b, *row_scale, *w;
    double* rowdot;
    float *ws, *out;
    long long K;
    long long spp;                               // pixels of one share: ups * kUnit
    int lda, ldb, ldw, ldo, M, N;
    int shares, accumulate;
};

// kWide: 32-wide tiles of the wide side; kWideM: the wide side is M (the operand a), else N (b)
template <int kWide, bool kWideM>
__global__ __launch_bounds__(256) void skinny_wgrad_kernel(const SkK k) {
    constexpr int kLoads = kWide <= 3 ? 8 : 4;                 // pixel pairs in flight: (kWide + 1) * kLoads loads of 256 bytes
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int share = (int)blockIdx.x * 4 + wave;
    if (share >= k.shares) return;                             // uniform over the wave; the kernel has no barrier
    const int half = lane >> 5, col = lane & 31;

    const long long p0 = (long long)share * k.spp;
    long long p1 = p0 + k.spp;
    if (p1 > k.K) p1 = k.K;
    const int wide = kWideM ? k.M : k.N, narrow = kWideM ? k.N : k.M;
    const int ldw = kWideM ? k.lda : k.ldb, ldn = kWideM ? k.ldb : k.lda;
    const float* wp = (kWideM ? k.a : k.b) + col;
    const float* np = (kWideM ? k.b : k.a) + col;
    const bool nok = col < narrow;                             // the narrow side's padding columns: zeros, never read
    bool wok[kWide];
#pragma unroll
    for (int t = 0; t < kWide; ++t) wok[t] = t * 32 + col < wide;

    f32x16 tot[kWide], acc[kWide];
#pragma unroll
    for (int t = 0; t < kWide; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) { tot[t][r] = 0.f; acc[t][r] = 0.f; }
    for (long long c0 = p0; c0 < p1; c0 += UAVSAL_WGRAD_CHAIN) {      // a chain: at most UAVSAL_WGRAD_CHAIN products
        long long c1 = c0 + UAVSAL_WGRAD_CHAIN;
        if (c1 > p1) c1 = p1;
        for (long long q = c0; q < c1; q += 2 * kLoads) {
            float nv[kLoads], wv[kWide][kLoads];
#pragma unroll
            for (int u = 0; u < kLoads; ++u) {
                const long long g = q + 2 * u + half;
                const bool ok = g < c1;                                 // rows at and behind p1 are zeros and never read
                nv[u] = ok && nok ? np[g * ldn] : 0.f;
#pragma unroll
                for (int t = 0; t < kWide; ++t) wv[t][u] = ok && wok[t] ? wp[g * ldw + t * 32] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < kLoads; ++u)
#pragma unroll
                for (int t = 0; t < kWide; ++t)
                    acc[t] = kWideM ? __builtin_amdgcn_mfma_f32_32x32x2f32(wv[t][u], nv[u], acc[t], 0, 0, 0)
                                    : __builtin_amdgcn_mfma_f32_32x32x2f32(nv[u], wv[t][u], acc[t], 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < kWide; ++t) {
            tot[t] += acc[t];
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
        }
    }
    float* w = k.ws + (long long)share * k.M * k.N;           // ws [share][m][n]
#pragma unroll
    for (int t = 0; t < kWide; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
            const int m = kWideM ? t * 32 + row : row;
            const int n = kWideM ? col : t * 32 + col;
            if (m < k.M && n < k.N) w[m * k.N + n] = tot[t][r];
        }
}

__global__ __launch_bounds__(kRedThreads) void skinny_reduce_kernel(const SkK k) {
    __shared__ double part[kRedThreads];
    __shared__ double red[256];
    const int m = blockIdx.x, tid = threadIdx.x;
    const int groups = kRedThreads / k.N;                      // N <= 192: at least 5
    const int spg = (k.shares + groups - 1) / groups;
    const int n = tid % k.N, j = tid / k.N;
    if (j < groups) {
        int s0 = j * spg, s1 = s0 + spg;
        if (s1 > k.shares) s1 = k.shares;
        const float* p = k.ws + (long long)m * k.N + n;
        double s = 0.0;
        for (int sh = s0; sh < s1; ++sh) s += (double)p[(long long)sh * k.M * k.N];
        part[tid] = s;                                         // tid == j * N + n
    }
    __syncthreads();
    double dot = 0.0;
    if (tid < k.N) {
        double s = 0.0;
        for (int g = 0; g < groups; ++g) s += part[g * k.N + tid];
        if (k.rowdot) dot = (double)k.w[(long long)m * k.ldw + tid] * s;
        float* o = k.out + (long long)m * k.ldo + tid;
        double v = (k.row_scale ? (double)k.row_scale[m] : 1.0) * s;
        if (k.accumulate) v += (double)*o;
        *o = (float)v;
    }
    if (!k.rowdot) return;                                     // uniform over the workgroup
    if (tid < 256) red[tid] = dot;                             // N <= 192 < 256: threads N .. 255 hold 0
    for (int s = 128; s > 0; s >>= 1) {
        __syncthreads();
        if (tid < s) red[tid] += red[tid + s];
    }
    if (tid == 0) k.rowdot[m] = red[0];
}

bool sk_shape_ok(int M, int N) {
    if (M <= 0 || N <= 0 || (M % 8) || (N % 8)) return false;
    const int lo = M < N ? M : N, hi = M < N ? N : M;
    return lo <= kMaxNarrow && hi <= kMaxWide;
}

bool sk_plan(const uavsal_skinny_wgrad_desc* d, SkK& k) {
    if (!d || d->K <= 0 || !sk_shape_ok(d->M, d->N)) return false;
    const long long units = (d->K + kUnit - 1) / kUnit;
    const long long want = units < kMaxShares ? units : kMaxShares;
    const long long ups = (units + want - 1) / want;
    if (ups > 0x7fffffffll / kUnit) return false;
    k.K = d->K; k.M = d->M; k.N = d->N;
    k.spp = ups * kUnit;
    k.shares = (int)((units + ups - 1) / ups);
    return true;
}

template <bool kWideM>
void sk_launch(int tiles, dim3 grid, hipStream_t stream, const SkK& k) {
    switch (tiles) {
    case 1: hipLaunchKernelGGL((skinny_wgrad_kernel<1, kWideM>), grid, dim3(256), 0, stream, k); break;
    case 2: hipLaunchKernelGGL((skinny_wgrad_kernel<2, kWideM>), grid, dim3(256), 0, stream, k); break;
    case 3: hipLaunchKernelGGL((skinny_wgrad_kernel<3, kWideM>), grid, dim3(256), 0, stream, k); break;
    case 4: hipLaunchKernelGGL((skinny_wgrad_kernel<4, kWideM>), grid, dim3(256), 0, stream, k); break;
    case 5: hipLaunchKernelGGL((skinny_wgrad_kernel<5, kWideM>), grid, dim3(256), 0, stream, k); break;
    default: hipLaunchKernelGGL((skinny_wgrad_kernel<6, kWideM>), grid, dim3(256), 0, stream, k); break;
    }
}

}  // namespace

extern "C" int uavsal_shallow_sizeof_desc(int which) { return which == 0 ? (int)sizeof(uavsal_skinny_wgrad_desc) : -1; }

extern "C" int uavsal_skinny_wgrad_shares(const uavsal_skinny_wgrad_desc* d) {
    SkK k;
    return sk_plan(d, k) ? k.shares : 0;
}

extern "C" int64_t uavsal_skinny_wgrad_workspace_bytes(const uavsal_skinny_wgrad_desc* d) {
    SkK k;
    if (!sk_plan(d, k)) return 0;
    return (int64_t)k.shares * k.M * k.N * (int64_t)sizeof(float);
}

extern "C" int uavsal_skinny_wgrad(const uavsal_skinny_wgrad_desc* d, uavsal_stream_t stream) {
    if (!d || !d->a || !d->b || !d->ws || !d->out) return UAVSAL_EINVAL;
    if (d->K <= 0 || d->M <= 0 || d->N <= 0) return UAVSAL_EINVAL;
    if (d->rowdot && !d->w) return UAVSAL_EINVAL;
    if (!sk_shape_ok(d->M, d->N)) return UAVSAL_ESHAPE;
    SkK k;
    if (!sk_plan(d, k)) return UAVSAL_ESHAPE;
    if (d->ws_bytes < uavsal_skinny_wgrad_workspace_bytes(d)) return UAVSAL_EINVAL;
    if (d->lda < d->M || d->ldb < d->N || d->ldo < d->N || (d->rowdot && d->ldw < d->N)) return UAVSAL_EINVAL;
    if ((d->lda | d->ldb) & 3) return UAVSAL_EALIGN;
    if (!al16(d->a) || !al16(d->b) || !al16(d->ws) || !al4(d->out) || (d->row_scale && !al4(d->row_scale)) ||
        (d->rowdot && (!al8(d->rowdot) || !al4(d->w)))) return UAVSAL_EALIGN;
    k.a = d->a; k.b = d->b; k.row_scale = d->row_scale; k.w = d->w; k.rowdot = d->rowdot; k.ws = d->ws; k.out = d->out;
    k.lda = d->lda; k.ldb = d->ldb; k.ldw = d->ldw; k.ldo = d->ldo;
    k.accumulate = d->accumulate != 0;
    const dim3 grid((unsigned)((k.shares + 3) / 4));
    const bool wide_m = k.M >= k.N;
    const int tiles = ((wide_m ? k.M : k.N) + 31) / 32;
    if (wide_m) sk_launch<true>(tiles, grid, (hipStream_t)stream, k);
    else sk_launch<false>(tiles, grid, (hipStream_t)stream, k);
    hipLaunchKernelGGL(skinny_reduce_kernel, dim3((unsigned)k.M), dim3(kRedThreads), 0, (hipStream_t)stream, k);
    return uavsal_launch_status();
}
