// Fine-tuning the gauss / ob prior nets: the parameter gradients of a NARROW inverted-residual block (8 -> 48 -> 64 and
// 20 -> 120 -> 64: hidden and input widths that fit no tile of uavsal_pix_gemm / uavsal_ir_sums) and the sum over frames that
// carries the output gradient of a net that ran on ONE frame.  include/uavsal_hip.h states the formulas.
//
// 1. uavsal_ir_narrow_grads: everything the nine gradients need, in ONE launch.  A workgroup owns a slab of whole picture
//    rows counted through all images (sums::slab_rule of csrc/train_sums.h with about 256 pixels: at most 256 slabs, a
//    function of the shape alone) and writes one partial per output into `ws` [slab][...] doubles.  The outputs of one block
//    are at most 64 x 120 + 120 x 20 + 11 x 120 + 64 numbers and the maps are the 45 x 80 prior maps: the stage is bound by
//    its launches, so the products run as VALU FMAs out of LDS, not on the matrix cores -- a 16-row MFMA tile would be a
//    third padding at Ch = 48 and the operands would need a transposing stage for five pixels' worth of arithmetic.
//    a. the eleven sums per hidden channel (S2, Gd[9], S1) and S3: a lane owns four channels and every 256 / (Ch / 4)-th
//       (S3: 16th) pixel of the slab, forms delta2 in fp32 as uavsal_ir_bwd does and adds every product to a double accumulator, exactly the
//       per-pixel arithmetic of ir_sums_kernel (sums::pixel_sums); the pixel lanes meet in LDS in lane order.
//    b. G1 = ga x x and G3 = go x d: the slab goes through LDS in chunks of UAVSAL_NARROW_CHUNK pixels; a lane owns a 4 x 4
//       tile of G1 and two 4 x 4 tiles of G3, accumulates a chunk in fp32 (fmaf, pixel order) and carries it to double
//       accumulators between chunks (the convention of pix_gemm_tile.h).  144 accumulator registers, no scratch.
//    The two phases reuse the same registers and the same LDS; the second reads the slab from L2.
// 2. uavsal_ir_narrow_finish: a workgroup per hidden channel and per output channel sums the slabs in slab order in double
//    and writes the nine gradients, each rounded once (or added to: `accumulate`).
// 3. uavsal_frame_sum: out[p][c] = sum_n a[n][p][c], frames in frame order in double, rounded once.
// No atomics anywhere: two calls return the same bits.
#include "common.h"
#include "train_sums.h"

namespace {

using sums::put;
constexpr int kNS = UAVSAL_IR_NSUM;                    // 11 sums per hidden channel: S2, Gd[9], S1
constexpr int kP = UAVSAL_NARROW_CHUNK;                // pixels of one fp32 chunk
constexpr int kCo = 64, kMaxCh = 128, kMaxCin = 32;
constexpr int kSlabPixels = 256;                       // pixels of a slab (1. above)

struct NarK {
    const float *x, *e, *d, *gd, *ga, *go;
    double* ws;
    long long rows;             // n_img * H
    int H, W, Cin, Ch, ldgo, slab_rows, slabs;
};

__host__ __device__ inline long long slab_doubles(int Cin, int Ch) {
    return (long long)kNS * Ch + kCo + (long long)Ch * Cin + (long long)kCo * Ch;
}

__global__ __launch_bounds__(256) void ir_narrow_kernel(const NarK p) {
    __shared__ __attribute__((aligned(16))) float lds[kP * (kMaxCin + kMaxCh + kCo + kMaxCh)];
    const int t = threadIdx.x, slab = blockIdx.x;
    const int Ch = p.Ch, Cin = p.Cin;
    const long long r0 = (long long)slab * p.slab_rows;
    long long r1 = r0 + p.slab_rows;
    if (r1 > p.rows) r1 = p.rows;
    const long long q0 = r0 * p.W, q1 = r1 * p.W;              // global pixels of the slab
    double* o = p.ws + (long long)slab * slab_doubles(Cin, Ch);
    double* red = reinterpret_cast<double*>(lds);

    {   // ---- S2, Gd[9], S1: a lane owns four channels and every `lanes`-th pixel, lanes = 256 / (Ch / 4) (8 at Ch = 120, 21 at 48)
        const int c4 = Ch >> 2, lanes = 256 / c4;
        const int pl = t / c4, c = (t - pl * c4) * 4;
        double acc[kNS][4];
#pragma unroll
        for (int j = 0; j < kNS; ++j)
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[j][u] = 0.0;
        if (pl < lanes)
            for (long long q = q0 + pl; q < q1; q += lanes) {
                const sums::Stride1Taps<false> taps(p, q, c);
                const f32x4 dv = ld4(p.d + q * Ch + c);
                const f32x4 gv = ld4(p.gd + q * Ch + c);
                const f32x4 av = ld4(p.ga + q * Ch + c);
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[10][u] += (double)av[u];
                sums::pixel_sums(taps, dv, gv, acc);
            }
#pragma unroll
        for (int j = 0; j < kNS; ++j) {                        // the pixel lanes meet in lane order (lanes * Ch <= 1024 doubles)
            if (pl < lanes)
#pragma unroll
                for (int u = 0; u < 4; ++u) red[pl * Ch + c + u] = acc[j][u];
            __syncthreads();
            if (t < Ch) {
                double s = red[t];
                for (int l = 1; l < lanes; ++l) s += red[l * Ch + t];
                o[(long long)j * Ch + t] = s;
            }
            __syncthreads();
        }
    }
    {   // ---- S3: a lane owns four output channels and every 16th pixel
        const int m = (t & 15) * 4, pl = t >> 4;
        double a3[4] = {0.0, 0.0, 0.0, 0.0};
        for (long long q = q0 + pl; q < q1; q += 16) {
            const f32x4 gv = ld4(p.go + q * p.ldgo + m);
#pragma unroll
            for (int u = 0; u < 4; ++u) a3[u] += (double)gv[u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) red[pl * kCo + m + u] = a3[u];
        __syncthreads();
        if (t < kCo) {
            double s = red[t];
#pragma unroll
            for (int l = 1; l < 16; ++l) s += red[l * kCo + t];
            o[(long long)kNS * Ch + t] = s;
        }
        __syncthreads();
    }

    // ---- G1 [Ch][Cin] = ga x x and G3 [64][Ch] = go x d
    float* sx = lds;
    float* sga = sx + kP * Cin;
    float* sgo = sga + kP * Ch;
    float* sd = sgo + kP * kCo;
    const int c4 = Ch >> 2, j4 = Cin >> 2;
    const int tc = t & 15, m3 = (t >> 4) * 4;                  // G3: rows m3..m3+3, channel quads tc and tc + 16
    const bool l30 = tc < c4, l31 = tc + 16 < c4;
    const int c1 = (t & 31) * 4, jj = (t >> 5) * 4;            // G1: rows c1..c1+3, columns jj..jj+3
    const bool l1 = c1 < Ch && jj < Cin;
    double D3[2][4][4], D1[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) D3[0][u][v] = D3[1][u][v] = D1[u][v] = 0.0;

    for (long long qc = q0; qc < q1; qc += kP) {
        const int np = (int)((q1 - qc < kP) ? (q1 - qc) : kP);
        for (int i = t; i < np * j4; i += 256) {
            const int px = i / j4, k = (i - px * j4) * 4;
            *reinterpret_cast<f32x4*>(sx + px * Cin + k) = ld4(p.x + (qc + px) * Cin + k);
        }
        for (int i = t; i < np * c4; i += 256) {
            const int px = i / c4, k = (i - px * c4) * 4;
            *reinterpret_cast<f32x4*>(sga + px * Ch + k) = ld4(p.ga + (qc + px) * Ch + k);
            *reinterpret_cast<f32x4*>(sd + px * Ch + k) = ld4(p.d + (qc + px) * Ch + k);
        }
        for (int i = t; i < np * (kCo / 4); i += 256) {
            const int px = i >> 4, k = (i & 15) * 4;
            *reinterpret_cast<f32x4*>(sgo + px * kCo + k) = ld4(p.go + (qc + px) * p.ldgo + k);
        }
        __syncthreads();
        float a3[2][4][4], a1[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) a3[0][u][v] = a3[1][u][v] = a1[u][v] = 0.f;
        for (int px = 0; px < np; ++px) {
            if (l30) {
                const f32x4 g = *reinterpret_cast<const f32x4*>(sgo + px * kCo + m3);
                const f32x4 d0 = *reinterpret_cast<const f32x4*>(sd + px * Ch + tc * 4);
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int v = 0; v < 4; ++v) a3[0][u][v] = __builtin_fmaf(g[u], d0[v], a3[0][u][v]);
                if (l31) {
                    const f32x4 d1 = *reinterpret_cast<const f32x4*>(sd + px * Ch + (tc + 16) * 4);
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int v = 0; v < 4; ++v) a3[1][u][v] = __builtin_fmaf(g[u], d1[v], a3[1][u][v]);
                }
            }
            if (l1) {
                const f32x4 av = *reinterpret_cast<const f32x4*>(sga + px * Ch + c1);
                const f32x4 xv = *reinterpret_cast<const f32x4*>(sx + px * Cin + jj);
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int v = 0; v < 4; ++v) a1[u][v] = __builtin_fmaf(av[u], xv[v], a1[u][v]);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                D3[0][u][v] += (double)a3[0][u][v];
                D3[1][u][v] += (double)a3[1][u][v];
                D1[u][v] += (double)a1[u][v];
            }
        __syncthreads();
    }
    double* o1 = o + (long long)kNS * Ch + kCo;
    double* o3 = o1 + (long long)Ch * Cin;
    if (l1)
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) o1[(long long)(c1 + u) * Cin + jj + v] = D1[u][v];
#pragma unroll
    for (int h = 0; h < 2; ++h)
        if (h ? l31 : l30)
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) o3[(long long)(m3 + u) * Ch + (tc + 16 * h) * 4 + v] = D3[h][u][v];
}

bool narrow_plan(const uavsal_ir_narrow_desc* d, NarK& k) {
    if (!d || d->n_img <= 0 || d->H <= 0 || d->W <= 0) return false;
    if (d->Cin <= 0 || d->Cin > kMaxCin || (d->Cin & 3) || d->Ch <= 0 || d->Ch > kMaxCh || (d->Ch & 3) || d->Co != kCo) return false;
    if ((long long)d->H * d->W > 0x7fffffffll) return false;
    k.H = d->H; k.W = d->W; k.Cin = d->Cin; k.Ch = d->Ch;
    k.rows = (long long)d->n_img * d->H;
    return sums::slab_rule(k.rows, d->W, kSlabPixels, k.slab_rows, k.slabs);
}

// ------------------------------------------------------------------------------------------------ finalise
struct NarFinK {
    const double* ws;
    const float *w1, *wd, *w3, *s1, *s2, *s3, *r1, *mu1, *r2, *mu2, *r3, *mu3;
    float *g_w1, *g_gamma1, *g_beta1, *g_wd, *g_gamma2, *g_beta2, *g_w3, *g_gamma3, *g_beta3;
    int Cin, Ch, slabs, accumulate;
};

__global__ __launch_bounds__(128) void ir_narrow_finish_kernel(const NarFinK k) {
    __shared__ double prod[kMaxCh];
    __shared__ double sums[kNS];
    const int b = blockIdx.x, t = threadIdx.x;
    const int Ch = k.Ch, Cin = k.Cin;
    const long long stride = slab_doubles(Cin, Ch);
    const long long off1 = (long long)kNS * Ch + kCo, off3 = off1 + (long long)Ch * Cin;
    if (b < Ch) {                                              // hidden channel c: W1's row, gamma1, beta1, Wd, gamma2, beta2
        const int c = b;
        if (t < Cin) {
            double G = 0.0;
            for (int sl = 0; sl < k.slabs; ++sl) G += k.ws[sl * stride + off1 + (long long)c * Cin + t];
            put(k.g_w1 + (long long)c * Cin + t, (double)k.s1[c] * G, k.accumulate);
            prod[t] = (double)k.w1[(long long)c * Cin + t] * G;
        }
        if (t >= kMaxCin && t < kMaxCin + kNS) {
            const int j = t - kMaxCin;
            double s = 0.0;
            for (int sl = 0; sl < k.slabs; ++sl) s += k.ws[sl * stride + (long long)j * Ch + c];
            sums[j] = s;
        }
        __syncthreads();
        if (t == 0) {
            double dot1 = 0.0, dotd = 0.0;
            for (int j = 0; j < Cin; ++j) dot1 += prod[j];
            const double s2 = (double)k.s2[c];
            for (int q = 0; q < 9; ++q) {
                put(k.g_wd + (long long)c * 9 + q, s2 * sums[1 + q], k.accumulate);
                dotd += (double)k.wd[(long long)c * 9 + q] * sums[1 + q];
            }
            put(k.g_beta2 + c, sums[0], k.accumulate);
            put(k.g_gamma2 + c, (double)k.r2[c] * (dotd - (double)k.mu2[c] * sums[0]), k.accumulate);
            put(k.g_beta1 + c, sums[10], k.accumulate);
            put(k.g_gamma1 + c, (double)k.r1[c] * (dot1 - (double)k.mu1[c] * sums[10]), k.accumulate);
        }
        return;
    }
    const int m = b - Ch;                                      // output channel m: W3's row, gamma3, beta3
    if (t < Ch) {
        double G = 0.0;
        for (int sl = 0; sl < k.slabs; ++sl) G += k.ws[sl * stride + off3 + (long long)m * Ch + t];
        put(k.g_w3 + (long long)m * Ch + t, (double)k.s3[m] * G, k.accumulate);
        prod[t] = (double)k.w3[(long long)m * Ch + t] * G;
    }
    if (t == 127) {
        double s = 0.0;
        for (int sl = 0; sl < k.slabs; ++sl) s += k.ws[sl * stride + (long long)kNS * Ch + m];
        sums[0] = s;
    }
    __syncthreads();
    if (t == 0) {
        double dot3 = 0.0;
        for (int c = 0; c < Ch; ++c) dot3 += prod[c];
        put(k.g_beta3 + m, sums[0], k.accumulate);
        put(k.g_gamma3 + m, (double)k.r3[m] * (dot3 - (double)k.mu3[m] * sums[0]), k.accumulate);
    }
}

// ------------------------------------------------------------------------------------------------ sum over frames
struct FsK {
    const float* a;
    float* out;
    long long total, HW;
    int lda, ldo, N, C4;
};

__global__ __launch_bounds__(256) void frame_sum_kernel(const FsK k) {
    const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
    if (item >= k.total) return;
    const long long pix = item / k.C4;
    const int c = (int)(item - pix * k.C4) * 4;
    const float* src = k.a + pix * k.lda + c;
    const f32x4 v0 = ld4(src);
    double s[4] = {(double)v0[0], (double)v0[1], (double)v0[2], (double)v0[3]};   // (N = 1: the input's bits, -0 included)
    for (int n = 1; n < k.N; ++n) {
        const f32x4 v = ld4(src + (long long)n * k.HW * k.lda);
#pragma unroll
        for (int u = 0; u < 4; ++u) s[u] += (double)v[u];
    }
    *reinterpret_cast<f32x4*>(k.out + pix * k.ldo + c) = (f32x4){(float)s[0], (float)s[1], (float)s[2], (float)s[3]};
}

}  // namespace

extern "C" int uavsal_nets_sizeof_desc(int which) {
    return which == 0 ? (int)sizeof(uavsal_ir_narrow_desc) : which == 1 ? (int)sizeof(uavsal_ir_narrow_finish_desc)
         : which == 2 ? (int)sizeof(uavsal_frame_sum_desc) : -1;
}

extern "C" int uavsal_ir_narrow_slabs(const uavsal_ir_narrow_desc* d) {
    NarK k;
    return narrow_plan(d, k) ? k.slabs : 0;
}

extern "C" int uavsal_ir_narrow_slab_rows(const uavsal_ir_narrow_desc* d) {
    NarK k;
    return narrow_plan(d, k) ? k.slab_rows : 0;
}

extern "C" int64_t uavsal_ir_narrow_workspace_bytes(const uavsal_ir_narrow_desc* d) {
    NarK k;
    if (!narrow_plan(d, k)) return 0;
    return (int64_t)k.slabs * slab_doubles(k.Cin, k.Ch) * (int64_t)sizeof(double);
}

extern "C" int uavsal_ir_narrow_grads(const uavsal_ir_narrow_desc* d, uavsal_stream_t stream) {
    if (!d || !d->x || !d->e || !d->d || !d->gd || !d->ga || !d->go || !d->ws) return UAVSAL_EINVAL;
    if (d->n_img <= 0 || d->H <= 0 || d->W <= 0 || d->Cin <= 0 || d->Ch <= 0 || d->Co <= 0) return UAVSAL_EINVAL;
    if ((d->Cin & 3) || (d->Ch & 3) || d->Cin > kMaxCin || d->Ch > kMaxCh || d->Co != kCo) return UAVSAL_ESHAPE;
    if (d->ldgo & 3) return UAVSAL_EALIGN;
    if (d->ldgo < d->Co) return UAVSAL_EINVAL;
    NarK k;
    if (!narrow_plan(d, k)) return UAVSAL_ESHAPE;
    if (d->ws_bytes < uavsal_ir_narrow_workspace_bytes(d)) return UAVSAL_EINVAL;
    if (!al16(d->x) || !al16(d->e) || !al16(d->d) || !al16(d->gd) || !al16(d->ga) || !al16(d->go) || !al8(d->ws)) return UAVSAL_EALIGN;
    k.x = d->x; k.e = d->e; k.d = d->d; k.gd = d->gd; k.ga = d->ga; k.go = d->go; k.ldgo = d->ldgo; k.ws = d->ws;
    hipLaunchKernelGGL(ir_narrow_kernel, dim3((unsigned)k.slabs), dim3(256), 0, (hipStream_t)stream, k);
    return uavsal_launch_status();
}

extern "C" int uavsal_ir_narrow_finish(const uavsal_ir_narrow_finish_desc* d, uavsal_stream_t stream) {
    if (!d || !d->ws || !d->w1 || !d->wd || !d->w3 || !d->s1 || !d->s2 || !d->s3 || !d->r1 || !d->mu1 || !d->r2 || !d->mu2 ||
        !d->r3 || !d->mu3 || !d->g_w1 || !d->g_gamma1 || !d->g_beta1 || !d->g_wd || !d->g_gamma2 || !d->g_beta2 || !d->g_w3 ||
        !d->g_gamma3 || !d->g_beta3)
        return UAVSAL_EINVAL;
    if (d->Cin <= 0 || d->Ch <= 0 || d->Co <= 0 || d->slabs <= 0) return UAVSAL_EINVAL;
    if ((d->Cin & 3) || (d->Ch & 3) || d->Cin > kMaxCin || d->Ch > kMaxCh || d->Co != kCo) return UAVSAL_ESHAPE;
    if (d->ws_bytes < (int64_t)d->slabs * slab_doubles(d->Cin, d->Ch) * (int64_t)sizeof(double)) return UAVSAL_EINVAL;
    const void* f4[] = {d->w1, d->wd, d->w3, d->s1, d->s2, d->s3, d->r1, d->mu1, d->r2, d->mu2, d->r3, d->mu3, d->g_w1, d->g_gamma1,
                        d->g_beta1, d->g_wd, d->g_gamma2, d->g_beta2, d->g_w3, d->g_gamma3, d->g_beta3};
    for (const void* p : f4)
        if (!al4(p)) return UAVSAL_EALIGN;
    if (!al8(d->ws)) return UAVSAL_EALIGN;
    NarFinK k;
    k.ws = d->ws; k.w1 = d->w1; k.wd = d->wd; k.w3 = d->w3; k.s1 = d->s1; k.s2 = d->s2; k.s3 = d->s3;
    k.r1 = d->r1; k.mu1 = d->mu1; k.r2 = d->r2; k.mu2 = d->mu2; k.r3 = d->r3; k.mu3 = d->mu3;
    k.g_w1 = d->g_w1; k.g_gamma1 = d->g_gamma1; k.g_beta1 = d->g_beta1; k.g_wd = d->g_wd; k.g_gamma2 = d->g_gamma2;
    k.g_beta2 = d->g_beta2; k.g_w3 = d->g_w3; k.g_gamma3 = d->g_gamma3; k.g_beta3 = d->g_beta3;
    k.Cin = d->Cin; k.Ch = d->Ch; k.slabs = d->slabs; k.accumulate = d->accumulate != 0;
    hipLaunchKernelGGL(ir_narrow_finish_kernel, dim3((unsigned)(d->Ch + kCo)), dim3(128), 0, (hipStream_t)stream, k);
    return uavsal_launch_status();
}

extern "C" int uavsal_frame_sum(const uavsal_frame_sum_desc* d, uavsal_stream_t stream) {
    if (!d || !d->a || !d->out) return UAVSAL_EINVAL;
    if (d->N <= 0 || d->HW <= 0 || d->C <= 0) return UAVSAL_EINVAL;
    if ((d->C & 3) || (d->lda & 3) || (d->ldo & 3)) return UAVSAL_EALIGN;
    if (d->lda < d->C || d->ldo < d->C) return UAVSAL_EINVAL;
    if (!al16(d->a) || !al16(d->out)) return UAVSAL_EALIGN;
    FsK k;
    k.a = d->a; k.out = d->out; k.lda = d->lda; k.ldo = d->ldo; k.N = d->N; k.HW = d->HW; k.C4 = d->C / 4;
    k.total = (long long)d->HW * k.C4;
    const long long blocks = (k.total + 255) / 256;
    if (blocks > 0x7fffffffll) return UAVSAL_ESHAPE;
    hipLaunchKernelGGL(frame_sum_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, k);
    return uavsal_launch_status();
}
