// Backward of a general inverted-residual block (a dwBlock with an expand conv, stride 1, dilation 1, in eval mode): the
// three launches behind train.block_backward / train.block_param_grads that the decoder's kernels (csrc/train.hip,
// csrc/train_decoder.hip: a projection to ONE channel) do not cover.  include/uavsal_hip.h states the formulas.
//
// 1. uavsal_ir_bwd: ga = d loss / d a1 from gd = d loss / d d.  The access pattern of dec_bwd_kernel (csrc/train.hip): a
//    lane owns four channels (16-byte loads) of a 2 x 2 pixel patch, reads the 4 x 4 halo of gd and d once, masks gd by d
//    (delta2 lives in registers only), correlates with the flipped depthwise taps, scales by s2 and masks by e.  Reads gd,
//    d, e and writes ga: 4 x Ch x 4 bytes per pixel.
//
// 2. uavsal_ir_sums: the channel sums S2, Gd[9], S1 (11 per hidden channel) and S3 (per output channel).  The layout of
//    dec_sums_kernel: a workgroup owns a channel group of 256 (64 lanes x 4; the lanes behind Ch are idle: 1920 = 7 groups
//    + 128) and a slab of whole picture rows counted through all frames; its four waves take the slab's pixels in turn;
//    per pixel a lane forms delta2 in fp32 as uavsal_ir_bwd does and adds every product to a double accumulator (4 x 11
//    doubles per lane).  The waves meet in LDS in wave order and the workgroup writes one partial per sum.  Behind the
//    hidden channel groups the grid holds ceil(Co / 256) more workgroups per slab that sum go the same way.  Workspace
//    [slab][11 * Ch + Co] doubles.  No atomics; the slab size depends on the shape alone.
//    uavsal_ir_sums_dil (a dilated depthwise conv: the SRF-Net head) and uavsal_ir_sums_s2 (stride 2: the multi-prior path and
//    the backbone) are the SAME kernel, ir_sums_kernel, with another tap policy (csrc/train_sums.h: where the nine taps of e
//    of an output pixel live): the same slabs, channel groups, double accumulators, wave order and workspace, so
//    uavsal_ir_finish takes any of the three.  With stride 2 a slab is whole OUTPUT rows; the waves take its output pixels
//    in turn for S2 and Gd, then the input pixels of the rows 2 oy and 2 oy + 1 for S1.  The stride-1, dilation-1
//    instantiation carries no dilation: no multiply, no kernel argument.
//
// 3. uavsal_ir_finish: a thread per channel sums the slabs in slab order in double and writes the seven small gradients,
//    each rounded once.
#include "common.h"
#include "train_sums.h"

namespace {

using sums::kGroup; using sums::put;
constexpr int kNS = UAVSAL_IR_NSUM;          // 11 sums per hidden channel: S2, Gd[9], S1
constexpr int kSlabPixels = 512;             // pixels of a slab of output rows (stride 1) ...
constexpr int kSlabInputPixels = 256;        // ... and of the input rows behind a slab of output rows (stride 2)

// ------------------------------------------------------------------------------------------------ ga from gd
struct BwdK {
    const float *gd, *d, *e, *wd9, *s2;
    float* ga;
    long long total;
    int n, H, W, C, C4, tiles_x, tiles_y;
};

__global__ __launch_bounds__(256) void ir_bwd_kernel(const BwdK p) {
    const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
    if (item >= p.total) return;
    const int c = (int)(item % p.C4) * 4;
    long long t = item / p.C4;
    const int tx = (int)(t % p.tiles_x); t /= p.tiles_x;
    const int ty = (int)(t % p.tiles_y);
    const int n = (int)(t / p.tiles_y);

    f32x4 wt[9];                                               // flipped: ga[p] = sum_r wd[8 - r] delta2[p + r - (1,1)]
#pragma unroll
    for (int r = 0; r < 9; ++r) wt[r] = ld4(p.wd9 + (size_t)(8 - r) * p.C + c);
    const int oy0 = ty * 2, ox0 = tx * 2;
    const size_t img = (size_t)n * p.H * p.W * p.C + c;
    const float* db = p.d + img;
    const float* gb = p.gd + img;

    f32x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int iy = oy0 - 1 + r;
        const bool rok = iy >= 0 && iy < p.H;
        f32x4 row[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ix = ox0 - 1 + q;
            row[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (rok && ix >= 0 && ix < p.W) {
                const size_t pix = ((size_t)iy * p.W + ix) * p.C;
                const f32x4 dv = ld4(db + pix), gv = ld4(gb + pix);
#pragma unroll
                for (int u = 0; u < 4; ++u) row[q][u] = (dv[u] > 0.f && dv[u] < 6.f) ? gv[u] : 0.f;
            }
        }
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int ky = r - a;
            if (ky < 0 || ky > 2) continue;
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) acc[a][b] += row[b + kx] * wt[ky * 3 + kx];
        }
    }
    const f32x4 s2 = ld4(p.s2 + c);
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int oy = oy0 + a;
        if (oy >= p.H) continue;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int ox = ox0 + b;
            if (ox >= p.W) continue;
            const size_t o = (((size_t)n * p.H + oy) * p.W + ox) * p.C + c;
            const f32x4 ev = ld4(p.e + o);
            f32x4 v = acc[a][b] * s2;
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = (ev[u] > 0.f && ev[u] < 6.f) ? v[u] : 0.f;
            *reinterpret_cast<f32x4*>(p.ga + o) = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------ channel sums
// The kernel arguments.  SumK is all the stride-1, dilation-1 instantiation gets; the other two append what their taps need.
struct SumK {
    const float *gd, *d, *e, *ga, *go;
    double* ws;
    long long rows;             // n_img * (output rows of an image)
    int H, W, Ch, Co, ldgo, slab_rows, slabs, cgroups;          // H, W: of e and ga
};
struct SumDilK : SumK { int dil; };
struct SumS2K : SumK { int Ho, Wo; };                           // of gd, d and go

template <class Taps, class K>
__global__ __launch_bounds__(256) void ir_sums_kernel(const K p) {
    __shared__ double red[4 * kGroup];
    constexpr bool kS2 = Taps::kStride == 2;
    const int slab = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r0 = (long long)slab * p.slab_rows;
    long long r1 = r0 + p.slab_rows;
    if (r1 > p.rows) r1 = p.rows;
    int Wo = p.W;
    if constexpr (kS2) Wo = p.Wo;
    const long long q0 = r0 * Wo, q1 = r1 * Wo;                // global OUTPUT pixels of the slab
    double* o = p.ws + (long long)slab * ((long long)kNS * p.Ch + p.Co);      // ws [slab][kNS][Ch], then S3 [Co]

    if ((int)blockIdx.y >= p.cgroups) {                        // uniform over the workgroup: S3 of one group of output channels
        const int m0 = ((int)blockIdx.y - p.cgroups) * kGroup;
        const int m = m0 + lane * 4;
        double a3[4] = {0.0, 0.0, 0.0, 0.0};
        if (m < p.Co)
            for (long long q = q0 + wave; q < q1; q += 4) {
                const f32x4 gv = ld4(p.go + q * p.ldgo + m);
#pragma unroll
                for (int u = 0; u < 4; ++u) a3[u] += (double)gv[u];
            }
        sums::wave_meet(red, a3, o + (long long)kNS * p.Ch + m0, p.Co - m0);
        return;
    }

    const int cg = blockIdx.y;
    const int c = cg * kGroup + lane * 4;
    const bool live = c < p.Ch;                                // Ch % 4 == 0: a lane's four channels are all inside or all outside
    double acc[kNS][4];
#pragma unroll
    for (int j = 0; j < kNS; ++j)
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[j][u] = 0.0;

    if (live) {
        for (long long q = q0 + wave; q < q1; q += 4) {        // S2 and Gd (stride 1: and S1): the slab's output pixels
            const Taps taps(p, q, c);
            const f32x4 dv = ld4(p.d + q * p.Ch + c);
            const f32x4 gv = ld4(p.gd + q * p.Ch + c);
            if constexpr (!kS2) {
                const f32x4 av = ld4(p.ga + q * p.Ch + c);
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[10][u] += (double)av[u];
            }
            sums::pixel_sums(taps, dv, gv, acc);
        }
        if constexpr (kS2) {
            // S1: the input rows 2 oy and 2 oy + 1 of every output row of the slab (each input row belongs to one output row)
            const long long j0 = r0 * 2 * p.W, j1 = r1 * 2 * p.W;
            for (long long j = j0 + wave; j < j1; j += 4) {
                const long long vr = j / p.W;                  // 2 * (output row) + (0 | 1)
                const int x = (int)(j - vr * p.W);
                const long long row = vr >> 1;
                const long long n = row / p.Ho;
                const int y = 2 * (int)(row - n * p.Ho) + (int)(vr & 1);
                if (y >= p.H) continue;                        // an odd H: the last output row has one input row
                const f32x4 av = ld4(p.ga + ((n * p.H + y) * p.W + x) * p.Ch + c);
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[10][u] += (double)av[u];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kNS; ++j) sums::wave_meet(red, acc[j], o + (long long)j * p.Ch + cg * kGroup, p.Ch - cg * kGroup);
}

// the hidden widths taken: multiples of 64, or with the descriptor's ch16 of 16 (the kernel itself needs Ch % 4 == 0 only)
inline int ch_step(int ch16) { return ch16 ? 16 : 64; }

// What the three entry points (uavsal_ir_sums, _s2, _dil) hand the one launcher: their descriptor's common fields, and
// which taps.  ok: the descriptor was not null.
enum SumsKind { kUnit, kStride2, kDilated };
struct SumsCall {
    bool ok;
    SumsKind kind;
    const float *gd, *d, *e, *ga, *go;
    double* ws;
    int64_t ws_bytes;
    int n_img, H, W, Ch, Co, ldgo, ch_mod, dil;
};

template <class Desc>
SumsCall sums_call(const Desc* d, SumsKind kind) {
    SumsCall c = {};
    if (!d) return c;
    c.ok = true; c.kind = kind;
    c.gd = d->gd; c.d = d->d; c.e = d->e; c.ga = d->ga; c.go = d->go; c.ldgo = d->ldgo; c.ws = d->ws; c.ws_bytes = d->ws_bytes;
    c.n_img = d->n_img; c.H = d->H; c.W = d->W; c.Ch = d->Ch; c.Co = d->Co; c.ch_mod = 64; c.dil = 1;
    return c;
}
SumsCall sums_call(const uavsal_ir_sums_desc* d) {
    SumsCall c = sums_call(d, kUnit);
    if (d) c.ch_mod = ch_step(d->ch16);
    return c;
}
SumsCall sums_call(const uavsal_ir_sums_s2_desc* d) {
    SumsCall c = sums_call(d, kStride2);
    if (d) c.ch_mod = ch_step(d->ch16);     // the opt-in of uavsal_ir_sums_desc
    return c;
}
SumsCall sums_call(const uavsal_ir_sums_dil_desc* d) {          // no ch16: Ch % 64
    SumsCall c = sums_call(d, kDilated);
    if (d) c.dil = d->dil;
    return c;
}

// The slab plan, a function of the shape alone (the dilation is not part of it).  Stride 1: rows of about kSlabPixels pixels.
// Stride 2: OUTPUT rows whose two input rows hold about kSlabInputPixels, and at most 0x3fffffff of them.
bool sums_plan(const SumsCall& c, SumS2K& k) {
    if (!c.ok || c.n_img <= 0 || c.H <= 0 || c.W <= 0 || c.Ch <= 0 || c.Co <= 0 || (c.Ch % c.ch_mod) || (c.Co % 4)) return false;
    k.cgroups = (c.Ch + kGroup - 1) / kGroup;
    if ((long long)c.H * c.W > 0x7fffffffll || k.cgroups + (c.Co + kGroup - 1) / kGroup > 65535) return false;
    const bool s2 = c.kind == kStride2;
    k.H = c.H; k.W = c.W; k.Ch = c.Ch; k.Co = c.Co;
    k.Ho = s2 ? (c.H - 1) / 2 + 1 : c.H; k.Wo = s2 ? (c.W - 1) / 2 + 1 : c.W;
    k.rows = (long long)c.n_img * k.Ho;
    return s2 ? sums::slab_rule(k.rows, 2ll * c.W, kSlabInputPixels, k.slab_rows, k.slabs, 0x3fffffffll)
              : sums::slab_rule(k.rows, c.W, kSlabPixels, k.slab_rows, k.slabs);
}

int sums_slabs(const SumsCall& c) {
    SumS2K k;
    return sums_plan(c, k) ? k.slabs : 0;
}

int sums_slab_rows(const SumsCall& c) {
    SumS2K k;
    return sums_plan(c, k) ? k.slab_rows : 0;
}

int64_t sums_workspace_bytes(const SumsCall& c) {
    SumS2K k;
    if (!sums_plan(c, k)) return 0;
    return (int64_t)k.slabs * ((int64_t)kNS * k.Ch + k.Co) * (int64_t)sizeof(double);
}

int sums_launch(const SumsCall& c, uavsal_stream_t stream) {
    if (!c.ok || !c.gd || !c.d || !c.e || !c.ga || !c.go || !c.ws) return UAVSAL_EINVAL;
    if (c.n_img <= 0 || c.H <= 0 || c.W <= 0 || c.Ch <= 0 || c.Co <= 0 || c.dil < 1) return UAVSAL_EINVAL;
    if (c.Ch % c.ch_mod) return UAVSAL_ESHAPE;
    if ((c.Co & 3) || (c.ldgo & 3)) return UAVSAL_EALIGN;
    if (c.ldgo < c.Co) return UAVSAL_EINVAL;
    SumS2K k;
    if (!sums_plan(c, k)) return UAVSAL_ESHAPE;
    if (c.kind == kDilated && (long long)c.dil * 2 > 0x7fffffffll / ((long long)c.W + 1)) return UAVSAL_ESHAPE;
    if (c.ws_bytes < sums_workspace_bytes(c)) return UAVSAL_EINVAL;
    if (!al16(c.gd) || !al16(c.d) || !al16(c.e) || !al16(c.ga) || !al16(c.go) || !al8(c.ws)) return UAVSAL_EALIGN;
    k.gd = c.gd; k.d = c.d; k.e = c.e; k.ga = c.ga; k.go = c.go; k.ldgo = c.ldgo; k.ws = c.ws;
    const dim3 grid((unsigned)k.slabs, (unsigned)(k.cgroups + (k.Co + kGroup - 1) / kGroup));
    const hipStream_t s = (hipStream_t)stream;
    if (c.kind == kStride2) {
        hipLaunchKernelGGL((ir_sums_kernel<sums::Stride2Taps, SumS2K>), grid, dim3(256), 0, s, k);
    } else if (c.kind == kDilated) {
        SumDilK kd;
        static_cast<SumK&>(kd) = k;
        kd.dil = c.dil;
        hipLaunchKernelGGL((ir_sums_kernel<sums::Stride1Taps<true>, SumDilK>), grid, dim3(256), 0, s, kd);
    } else {
        hipLaunchKernelGGL((ir_sums_kernel<sums::Stride1Taps<false>, SumK>), grid, dim3(256), 0, s, static_cast<const SumK&>(k));
    }
    return uavsal_launch_status();
}

// ------------------------------------------------------------------------------------------------ finalise
struct FinK {
    const double *ws, *rowdot1, *rowdot3;
    const float *wd, *s2, *r1, *mu1, *r2, *mu2, *r3, *mu3;
    float *g_gamma1, *g_beta1, *g_wd, *g_gamma2, *g_beta2, *g_gamma3, *g_beta3;
    int Ch, Co, slabs, accumulate;
};

__global__ __launch_bounds__(256) void ir_finish_kernel(const FinK k) {
    const long long stride = (long long)kNS * k.Ch + k.Co;
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < k.Ch) {
        double s[kNS];
#pragma unroll
        for (int j = 0; j < kNS; ++j) s[j] = 0.0;
        for (int sl = 0; sl < k.slabs; ++sl) {
            const double* q = k.ws + sl * stride + c;
#pragma unroll
            for (int j = 0; j < kNS; ++j) s[j] += q[(long long)j * k.Ch];
        }
        const double s2 = (double)k.s2[c];
        double dotd = 0.0;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            put(k.g_wd + (long long)c * 9 + t, s2 * s[1 + t], k.accumulate);
            dotd += (double)k.wd[(long long)c * 9 + t] * s[1 + t];
        }
        put(k.g_beta2 + c, s[0], k.accumulate);
        put(k.g_gamma2 + c, (double)k.r2[c] * (dotd - (double)k.mu2[c] * s[0]), k.accumulate);
        put(k.g_beta1 + c, s[10], k.accumulate);
        put(k.g_gamma1 + c, (double)k.r1[c] * (k.rowdot1[c] - (double)k.mu1[c] * s[10]), k.accumulate);
    }
    if (c < k.Co) {
        double S3 = 0.0;
        for (int sl = 0; sl < k.slabs; ++sl) S3 += k.ws[sl * stride + (long long)kNS * k.Ch + c];
        put(k.g_beta3 + c, S3, k.accumulate);
        put(k.g_gamma3 + c, (double)k.r3[c] * (k.rowdot3[c] - (double)k.mu3[c] * S3), k.accumulate);
    }
}

}  // namespace

extern "C" int uavsal_block_sizeof_desc(int which) {
    return which == 0 ? (int)sizeof(uavsal_ir_bwd_desc) : which == 1 ? (int)sizeof(uavsal_ir_sums_desc)
         : which == 2 ? (int)sizeof(uavsal_ir_finish_desc) : -1;
}

extern "C" int uavsal_ir_bwd(const uavsal_ir_bwd_desc* d, uavsal_stream_t stream) {
    if (!d || !d->gd || !d->d || !d->e || !d->wd9 || !d->s2 || !d->ga) return UAVSAL_EINVAL;
    if (d->n_img <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0) return UAVSAL_EINVAL;
    if (d->C & 3) return UAVSAL_EALIGN;
    if (!al16(d->gd) || !al16(d->d) || !al16(d->e) || !al16(d->ga) || !al16(d->wd9) || !al16(d->s2)) return UAVSAL_EALIGN;
    if ((long long)d->H * d->W > 0x7fffffffll) return UAVSAL_ESHAPE;
    BwdK k;
    k.gd = d->gd; k.d = d->d; k.e = d->e; k.wd9 = d->wd9; k.s2 = d->s2; k.ga = d->ga;
    k.n = d->n_img; k.H = d->H; k.W = d->W; k.C = d->C; k.C4 = d->C / 4;
    k.tiles_y = (d->H + 1) / 2; k.tiles_x = (d->W + 1) / 2;
    k.total = (long long)d->n_img * k.tiles_y * k.tiles_x * k.C4;
    const long long blocks = (k.total + 255) / 256;
    if (blocks > 0x7fffffffll) return UAVSAL_ESHAPE;
    hipLaunchKernelGGL(ir_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, k);
    return uavsal_launch_status();
}

// The three channel-sums launches and their queries: one kernel, one launcher (sums_launch above), three tap policies.
extern "C" int uavsal_ir_sums_slabs(const uavsal_ir_sums_desc* d) { return sums_slabs(sums_call(d)); }
extern "C" int uavsal_ir_sums_slab_rows(const uavsal_ir_sums_desc* d) { return sums_slab_rows(sums_call(d)); }
extern "C" int64_t uavsal_ir_sums_workspace_bytes(const uavsal_ir_sums_desc* d) { return sums_workspace_bytes(sums_call(d)); }
extern "C" int uavsal_ir_sums(const uavsal_ir_sums_desc* d, uavsal_stream_t stream) { return sums_launch(sums_call(d), stream); }

extern "C" int uavsal_ir_sums_s2_slabs(const uavsal_ir_sums_s2_desc* d) { return sums_slabs(sums_call(d)); }
extern "C" int uavsal_ir_sums_s2_slab_rows(const uavsal_ir_sums_s2_desc* d) { return sums_slab_rows(sums_call(d)); }
extern "C" int64_t uavsal_ir_sums_s2_workspace_bytes(const uavsal_ir_sums_s2_desc* d) { return sums_workspace_bytes(sums_call(d)); }
extern "C" int uavsal_ir_sums_s2(const uavsal_ir_sums_s2_desc* d, uavsal_stream_t stream) { return sums_launch(sums_call(d), stream); }

extern "C" int uavsal_ir_sums_dil_slabs(const uavsal_ir_sums_dil_desc* d) { return sums_slabs(sums_call(d)); }
extern "C" int uavsal_ir_sums_dil_slab_rows(const uavsal_ir_sums_dil_desc* d) { return sums_slab_rows(sums_call(d)); }
extern "C" int64_t uavsal_ir_sums_dil_workspace_bytes(const uavsal_ir_sums_dil_desc* d) { return sums_workspace_bytes(sums_call(d)); }
extern "C" int uavsal_ir_sums_dil(const uavsal_ir_sums_dil_desc* d, uavsal_stream_t stream) { return sums_launch(sums_call(d), stream); }

static int ir_finish(const uavsal_ir_finish_desc* d, uavsal_stream_t stream, int ch16) {
    if (!d || !d->ws || !d->rowdot1 || !d->rowdot3 || !d->wd || !d->s2 || !d->r1 || !d->mu1 || !d->r2 || !d->mu2 || !d->r3 ||
        !d->mu3 || !d->g_gamma1 || !d->g_beta1 || !d->g_wd || !d->g_gamma2 || !d->g_beta2 || !d->g_gamma3 || !d->g_beta3)
        return UAVSAL_EINVAL;
    if (d->Ch <= 0 || d->Co <= 0 || d->slabs <= 0) return UAVSAL_EINVAL;
    if ((d->Ch % ch_step(ch16)) || (d->Co & 3)) return UAVSAL_ESHAPE;
    if (d->ws_bytes < (int64_t)d->slabs * ((int64_t)kNS * d->Ch + d->Co) * (int64_t)sizeof(double)) return UAVSAL_EINVAL;
    const void* f4[] = {d->wd, d->s2, d->r1, d->mu1, d->r2, d->mu2, d->r3, d->mu3, d->g_gamma1, d->g_beta1, d->g_wd,
                        d->g_gamma2, d->g_beta2, d->g_gamma3, d->g_beta3};
    for (const void* p : f4)
        if (!al4(p)) return UAVSAL_EALIGN;
    if (!al8(d->ws) || !al8(d->rowdot1) || !al8(d->rowdot3)) return UAVSAL_EALIGN;
    FinK k;
    k.ws = d->ws; k.rowdot1 = d->rowdot1; k.rowdot3 = d->rowdot3; k.wd = d->wd; k.s2 = d->s2;
    k.r1 = d->r1; k.mu1 = d->mu1; k.r2 = d->r2; k.mu2 = d->mu2; k.r3 = d->r3; k.mu3 = d->mu3;
    k.g_gamma1 = d->g_gamma1; k.g_beta1 = d->g_beta1; k.g_wd = d->g_wd; k.g_gamma2 = d->g_gamma2; k.g_beta2 = d->g_beta2;
    k.g_gamma3 = d->g_gamma3; k.g_beta3 = d->g_beta3;
    k.Ch = d->Ch; k.Co = d->Co; k.slabs = d->slabs; k.accumulate = d->accumulate != 0;
    const int most = d->Ch > d->Co ? d->Ch : d->Co;
    hipLaunchKernelGGL(ir_finish_kernel, dim3((unsigned)((most + 255) / 256)), dim3(256), 0, (hipStream_t)stream, k);
    return uavsal_launch_status();
}

extern "C" int uavsal_ir_finish(const uavsal_ir_finish_desc* d, uavsal_stream_t stream) { return ir_finish(d, stream, 0); }

extern "C" int uavsal_ir_finish_c16(const uavsal_ir_finish_desc* d, uavsal_stream_t stream) { return ir_finish(d, stream, 1); }
