// Input gradients of the FROZEN context-prior path (reference model.py:357-361): the three launches behind
// train.block_input_grad / train.fust_output_grad that the trained-block kernels (csrc/train_block.hip) do not cover.
// include/uavsal_hip.h states the formulas.
//
// 1. uavsal_ir_bwd_s2: uavsal_ir_bwd for a depthwise 3x3 with stride 2 (padding 1, dilation 1).  A lane owns four channels
//    (16-byte loads) of a 2 x 2 INPUT patch (2 ty + a, 2 tx + b) and reads the 2 x 2 outputs (ty + r, tx + q) that touch it:
//    an input pixel receives 1 (both coordinates even), 2 or 4 (both odd) taps.  gd is masked by d in registers, the sum is
//    scaled by s2 and masked by e, in the order of ir_bwd_kernel.  Every pixel is guarded: with an odd H or W the last input
//    row / column has no partner, and the outputs ty + 1 = Ho, tx + 1 = Wo do not exist.
//
// 2. uavsal_bilinear_ac_bwd: the adjoint of uavsal_bilinear_ac (csrc/glue.hip) with its frame map, as a GATHER: a lane owns
//    four channels of one source pixel, walks the output images that read its source image in increasing order, then the
//    candidate rows and columns, recomputes the forward's own fp32 coordinates and weights for each and adds the weight
//    where the forward read THIS source pixel.  Double accumulation, one rounding, no atomics: a function of the shape.
//
// 3. uavsal_tsum_bwd: out[b T + t] = a[b T + t] + g[b], the adjoint of uavsal_tsum added to a given gradient.
//
// And, for the path when it is TRAINED (train.prior_path_backward):
//
// 4. uavsal_ir_sums_s2 lives in csrc/train_block.hip: ir_sums_kernel with the stride-2 tap policy of csrc/train_sums.h,
//    into the same workspace [slab][11 * Ch + Co], so that uavsal_ir_finish serves both; only its descriptor's size is
//    answered here (uavsal_mp_sizeof_desc).
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------ ga from gd, stride 2
struct S2K {
    const float *gd, *d, *e, *wd9, *s2;
    float* ga;
    long long total;
    int n, H, W, Ho, Wo, C, C4;
};

__global__ __launch_bounds__(256) void ir_bwd_s2_kernel(const S2K p) {
    const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
    if (item >= p.total) return;
    const int c = (int)(item % p.C4) * 4;
    long long t = item / p.C4;
    const int tx = (int)(t % p.Wo); t /= p.Wo;                 // tiles_x == Wo, tiles_y == Ho: ceil(W / 2) = (W - 1) / 2 + 1
    const int ty = (int)(t % p.Ho);
    const int n = (int)(t / p.Ho);

    f32x4 wt[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) wt[r] = ld4(p.wd9 + (size_t)r * p.C + c);
    const size_t oimg = (size_t)n * p.Ho * p.Wo * p.C + c;
    f32x4 D[2][2];                                             // delta2 of the outputs (ty + r, tx + q), zero outside
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            D[r][q] = (f32x4){0.f, 0.f, 0.f, 0.f};
            const int oy = ty + r, ox = tx + q;
            if (oy < p.Ho && ox < p.Wo) {
                const size_t pix = oimg + ((size_t)oy * p.Wo + ox) * p.C;
                const f32x4 dv = ld4(p.d + pix), gv = ld4(p.gd + pix);
#pragma unroll
                for (int u = 0; u < 4; ++u) D[r][q][u] = (dv[u] > 0.f && dv[u] < 6.f) ? gv[u] : 0.f;
            }
        }
    const f32x4 s2 = ld4(p.s2 + c);
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int y = 2 * ty + a;
        if (y >= p.H) continue;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int x = 2 * tx + b;
            if (x >= p.W) continue;
            // input (y, x) is read by output (oy, ox) through tap (ky, kx) when y = 2 oy - 1 + ky, x = 2 ox - 1 + kx
            f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                if ((a + 1 - ky) & 1) continue;
                const int r = (a + 1 - ky) / 2;                // oy - ty: 0 or 1
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    if ((b + 1 - kx) & 1) continue;
                    const int q = (b + 1 - kx) / 2;
                    acc += wt[ky * 3 + kx] * D[r][q];
                }
            }
            const size_t o = (((size_t)n * p.H + y) * p.W + x) * p.C + c;
            const f32x4 ev = ld4(p.e + o);
            f32x4 v = acc * s2;
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = (ev[u] > 0.f && ev[u] < 6.f) ? v[u] : 0.f;
            *reinterpret_cast<f32x4*>(p.ga + o) = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------ bilinear adjoint
struct BbK {
    const float* gout; float* gin;
    int ldo, Hi, Wi, Ho, Wo, C, C4, n_out, n_src, src_mod, src_div;
    float sy, sx; long long total;
};

// the output rows (columns) that may read source row `s`: fy = scale * o lies in (s - 1, s + 1); two rows of margin cover
// the rounding of the division, membership is decided by the forward's own expressions
__device__ __forceinline__ void cand(int s, float scale, int n_o, int& lo, int& hi) {
    lo = 0; hi = n_o - 1;
    if (scale > 0.f) {
        const float a = floorf((float)(s - 1) / scale) - 2.f, b = ceilf((float)(s + 1) / scale) + 2.f;
        if (a > 0.f) lo = a < (float)(n_o - 1) ? (int)a : n_o - 1;
        if (b < (float)(n_o - 1)) hi = b > 0.f ? (int)b : 0;
    }
}

// the weight with which the forward's output row (column) `o` reads source row `s`: hy where y0 == s plus ly where y1 == s
// (both at the border, where y0 == y1); false when it does not read it
__device__ __forceinline__ bool weight(int o, int s, float scale, int n_i, double& w) {
    const float f = scale * o;
    const int i0 = (int)f;
    const int i1 = i0 + (i0 < n_i - 1 ? 1 : 0);
    const float l = f - i0, h = 1.f - l;
    w = 0.0;
    if (i0 == s) w += (double)h;
    if (i1 == s) w += (double)l;
    return i0 == s || i1 == s;
}

__global__ __launch_bounds__(256) void bilinear_bwd_kernel(const BbK p) {
    const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
    if (item >= p.total) return;
    const int c = (int)(item % p.C4) * 4;
    long long t = item / p.C4;
    const int sx = (int)(t % p.Wi); t /= p.Wi;
    const int sy = (int)(t % p.Hi);
    const int ns = (int)(t / p.Hi);
    int oy_lo, oy_hi, ox_lo, ox_hi;
    cand(sy, p.sy, p.Ho, oy_lo, oy_hi);
    cand(sx, p.sx, p.Wo, ox_lo, ox_hi);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int n = 0; n < p.n_out; ++n) {
        if ((n % p.src_mod) / p.src_div != ns) continue;
        const float* img = p.gout + (size_t)n * p.Ho * p.Wo * p.ldo + c;
        for (int oy = oy_lo; oy <= oy_hi; ++oy) {
            double wy;
            if (!weight(oy, sy, p.sy, p.Hi, wy)) continue;
            for (int ox = ox_lo; ox <= ox_hi; ++ox) {
                double wx;
                if (!weight(ox, sx, p.sx, p.Wi, wx)) continue;
                const f32x4 g = ld4(img + ((size_t)oy * p.Wo + ox) * p.ldo);
                const double w = wy * wx;
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[u] += w * (double)g[u];
            }
        }
    }
    const f32x4 r = {(float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]};
    *reinterpret_cast<f32x4*>(p.gin + (((size_t)ns * p.Hi + sy) * p.Wi + sx) * p.C + c) = r;
}

// ------------------------------------------------------------------------------------------------ time-sum adjoint
struct TbK { const float *a, *g; float* out; int lda, ldg, ldo, HW, C4, T; long long total; };

__global__ __launch_bounds__(256) void tsum_bwd_kernel(const TbK p) {
    const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
    if (item >= p.total) return;
    const int c = (int)(item % p.C4) * 4;
    long long t = item / p.C4;
    const int pix = (int)(t % p.HW);
    const long long n = t / p.HW;
    const long long b = n / p.T;
    const f32x4 av = ld4(p.a + ((size_t)n * p.HW + pix) * p.lda + c);
    const f32x4 gv = ld4(p.g + ((size_t)b * p.HW + pix) * p.ldg + c);
    *reinterpret_cast<f32x4*>(p.out + ((size_t)n * p.HW + pix) * p.ldo + c) = av + gv;
}

inline int grid_for(long long total, unsigned* nblk) {
    const long long b = (total + 255) / 256;
    if (b <= 0 || b > 0x7fffffffLL) return UAVSAL_ESHAPE;
    *nblk = (unsigned)b;
    return 0;
}

}  // namespace

extern "C" int uavsal_ctx_sizeof_desc(int which) {
    return which == 0 ? (int)sizeof(uavsal_ir_bwd_s2_desc) : which == 1 ? (int)sizeof(uavsal_bilinear_bwd_desc)
         : which == 2 ? (int)sizeof(uavsal_tsum_bwd_desc) : -1;
}

extern "C" int uavsal_ir_bwd_s2(const uavsal_ir_bwd_s2_desc* d, uavsal_stream_t stream) {
    if (!d || !d->gd || !d->d || !d->e || !d->wd9 || !d->s2 || !d->ga) return UAVSAL_EINVAL;
    if (d->n_img <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0) return UAVSAL_EINVAL;
    if (d->C & 3) return UAVSAL_ESHAPE;
    if (!uavsal_aligned16(d->gd) || !uavsal_aligned16(d->d) || !uavsal_aligned16(d->e) || !uavsal_aligned16(d->ga) ||
        !uavsal_aligned16(d->wd9) || !uavsal_aligned16(d->s2))
        return UAVSAL_EALIGN;
    if ((long long)d->H * d->W > 0x7fffffffll) return UAVSAL_ESHAPE;
    S2K k;
    k.gd = d->gd; k.d = d->d; k.e = d->e; k.wd9 = d->wd9; k.s2 = d->s2; k.ga = d->ga;
    k.n = d->n_img; k.H = d->H; k.W = d->W; k.C = d->C; k.C4 = d->C / 4;
    k.Ho = (d->H - 1) / 2 + 1; k.Wo = (d->W - 1) / 2 + 1;
    k.total = (long long)d->n_img * k.Ho * k.Wo * k.C4;
    unsigned nblk; int e = grid_for(k.total, &nblk); if (e) return e;
    hipLaunchKernelGGL(ir_bwd_s2_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, k);
    return uavsal_launch_status();
}

extern "C" int uavsal_mp_sizeof_desc(int which) { return which == 0 ? (int)sizeof(uavsal_ir_sums_s2_desc) : -1; }

extern "C" int uavsal_bilinear_ac_bwd(const uavsal_bilinear_bwd_desc* d, uavsal_stream_t stream) {
    if (!d || !d->gout || !d->gin) return UAVSAL_EINVAL;
    if (d->n_out <= 0 || d->n_src <= 0 || d->C <= 0 || d->Hi <= 0 || d->Wi <= 0 || d->Ho <= 0 || d->Wo <= 0) return UAVSAL_EINVAL;
    if (d->src_mod <= 0 || d->src_div <= 0) return UAVSAL_EINVAL;
    const int last = ((d->n_out < d->src_mod ? d->n_out : d->src_mod) - 1) / d->src_div;     // the largest source image read
    if (d->n_src <= last) return UAVSAL_EINVAL;
    if ((d->C & 3) || (d->ldo & 3) || d->ldo < d->C) return UAVSAL_EALIGN;
    if (!uavsal_aligned16(d->gout) || !uavsal_aligned16(d->gin)) return UAVSAL_EALIGN;
    if (d->Ho > (1 << 22) || d->Wo > (1 << 22) || d->Hi > (1 << 22) || d->Wi > (1 << 22)) return UAVSAL_ESHAPE;
    BbK k;
    k.gout = d->gout; k.gin = d->gin; k.ldo = d->ldo;
    k.Hi = d->Hi; k.Wi = d->Wi; k.Ho = d->Ho; k.Wo = d->Wo; k.C = d->C; k.C4 = d->C / 4;
    k.n_out = d->n_out; k.n_src = d->n_src; k.src_mod = d->src_mod; k.src_div = d->src_div;
    k.sy = d->Ho > 1 ? (float)(d->Hi - 1) / (float)(d->Ho - 1) : 0.f;         // uavsal_bilinear_ac's own expressions
    k.sx = d->Wo > 1 ? (float)(d->Wi - 1) / (float)(d->Wo - 1) : 0.f;
    k.total = (long long)d->n_src * d->Hi * d->Wi * k.C4;
    unsigned nblk; int e = grid_for(k.total, &nblk); if (e) return e;
    hipLaunchKernelGGL(bilinear_bwd_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, k);
    return uavsal_launch_status();
}

extern "C" int uavsal_tsum_bwd(const uavsal_tsum_bwd_desc* d, uavsal_stream_t stream) {
    if (!d || !d->a || !d->g || !d->out) return UAVSAL_EINVAL;
    if (d->n_groups <= 0 || d->T <= 0 || d->HW <= 0 || d->C <= 0) return UAVSAL_EINVAL;
    if ((d->C & 3) || (d->lda & 3) || (d->ldg & 3) || (d->ldo & 3) || d->lda < d->C || d->ldg < d->C || d->ldo < d->C)
        return UAVSAL_EALIGN;
    if (!uavsal_aligned16(d->a) || !uavsal_aligned16(d->g) || !uavsal_aligned16(d->out)) return UAVSAL_EALIGN;
    TbK k; k.a = d->a; k.g = d->g; k.out = d->out; k.lda = d->lda; k.ldg = d->ldg; k.ldo = d->ldo;
    k.HW = d->HW; k.C4 = d->C / 4; k.T = d->T;
    k.total = (long long)d->n_groups * d->T * d->HW * k.C4;
    unsigned nblk; int e = grid_for(k.total, &nblk); if (e) return e;
    hipLaunchKernelGGL(tsum_bwd_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, k);
    return uavsal_launch_status();
}
