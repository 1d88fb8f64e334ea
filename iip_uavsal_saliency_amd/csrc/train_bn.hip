// BatchNorm in TRAINING mode for a general NHWC tensor u [P][C] (P = n_img * H * W pixels of ALL frames of the call), and the
// pieces the decoder conv_out_st needs around it (train/bn.py, train.decoder_forward_batch / decoder_backward_batch;
// include/uavsal_hip.h states the formulas).  Every kernel is memory bound.
//
// Geometry of the reductions (bn_stats, bn_bwd_sums, dw_wgrad): a lane owns `vec` = 4 consecutive channels of a pixel (16-byte
// loads; C == 1: one channel, vec = 1), `lc` lanes -- the smallest power of two >= C / vec, at most 64 -- stand side by side on
// one pixel (a wave reads 1 KB of a 256-channel row), and the 256 / lc pixel lanes of a workgroup take the pixels of the
// workgroup's slab in turn.  A workgroup owns one group of lc * vec channels and one slab of whole picture rows, counted
// through all frames (sums::slab_rule of csrc/train_sums.h: about 512 pixels, at most 256 slabs: a function of the shape alone).  A
// thread adds its products in double; the pixel lanes of a channel meet in LDS and are added in pixel-lane order; one partial
// per sum, slab and channel goes to the workspace [slab][sum][C].  A finish launch, a thread per channel, adds the slabs in
// slab order and rounds once.  No atomics: two calls return the same bits.
//
// 1. uavsal_bn_stats: sum u, sum u^2 -> mu, var, r, s = gamma r, b = beta - mu s, and the running statistics blended in double
//    in place (two launches).
// 2. uavsal_bn_apply: out = act(fma(u, s, b)) element-wise; with dot_w: out[p] = sum_c dot_w[c] act(...)[p][c], a wave per
//    pixel (the decoder's projection to one channel: d is never stored).  uavsal_bn_apply_res: out = act(fma(u, s, b)) + res,
//    the last BatchNorm of an inverted-residual block with its residual (train.block_forward_batch).
// 3. uavsal_bn_bwd_sums: sum g_a, sum g_a xh (and, for a rank-one gradient g[p][c] = g_pix[p] g_chan[c], sum g_pix act(a): the
//    weight gradient of the projection that made it) -> d beta, d gamma (two launches).
// 4. uavsal_bn_bwd_apply: g_u = s (g_a - d beta / P - xh d gamma / P), element-wise.
// 5. uavsal_dw_wgrad: the nine sums per channel of a depthwise 3x3's weight gradient (two launches).
#include "common.h"
#include "train_sums.h"

namespace {

using sums::put;
constexpr int kSlabPixels = 512;             // pixels of a slab
constexpr int kThreads = 256;

template <int V> struct Vec { float v[V]; };

template <int V> __device__ __forceinline__ Vec<V> ldv(const float* p) {
    Vec<V> r;
    if constexpr (V == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
        for (int u = 0; u < 4; ++u) r.v[u] = t[u];
    } else {
        r.v[0] = *p;
    }
    return r;
}

template <int V> __device__ __forceinline__ void stv(float* p, const Vec<V>& r) {
    if constexpr (V == 4) {
        f32x4 t;
#pragma unroll
        for (int u = 0; u < 4; ++u) t[u] = r.v[u];
        *reinterpret_cast<f32x4*>(p) = t;
    } else {
        *p = r.v[0];
    }
}

// the pre-activation as EVERY kernel of this file forms it: one fused multiply-add
__device__ __forceinline__ float bn_pre(float u, float s, float b) { return fmaf(u, s, b); }

// g_a = g * act'(a): torch's strict ReLU6 mask; y (1 - y) of the sigmoid apply_act forms
__device__ __forceinline__ float bn_ga(float g, float a, int act) {
    if (act == UAVSAL_ACT_RELU6) return (a > 0.f && a < 6.f) ? g : 0.f;
    if (act == UAVSAL_ACT_SIGMOID) {
        const float y = apply_act(a, UAVSAL_ACT_SIGMOID);
        return g * (y * (1.f - y));
    }
    return g;
}

struct Geo {
    long long rows, P;          // n_img * H picture rows, pixels
    int H, W, C, vec, lc, pl, cgc, cgs, slab_rows, slabs;
};

bool geo_plan(int n_img, int H, int W, int C, Geo& g) {
    if (n_img <= 0 || H <= 0 || W <= 0 || C <= 0) return false;
    if (C != 1 && (C & 3)) return false;
    if ((long long)H * W > 0x7fffffffll) return false;
    g.H = H; g.W = W; g.C = C;
    g.rows = (long long)n_img * H;
    g.P = g.rows * W;
    g.vec = C == 1 ? 1 : 4;
    const int lanes = C / g.vec;
    int lc = 1;
    while (lc < lanes && lc < 64) lc <<= 1;
    g.lc = lc; g.pl = kThreads / lc; g.cgc = lc * g.vec;
    g.cgs = (C + g.cgc - 1) / g.cgc;
    if (g.cgs > 65535) return false;
    return sums::slab_rule(g.rows, W, kSlabPixels, g.slab_rows, g.slabs);
}

// The pixel lanes of a channel meet in pixel-lane order: red holds kThreads * 4 doubles; `o` points at this slab's and this
// sum's [C] doubles.  Every thread of the workgroup calls it (it synchronises).
template <int V>
__device__ __forceinline__ void slab_reduce(double* red, const double* acc, bool active, const Geo& g, int cg, double* o) {
    const int cl = threadIdx.x % g.lc, pi = threadIdx.x / g.lc;
#pragma unroll
    for (int u = 0; u < V; ++u) red[pi * g.cgc + cl * V + u] = active ? acc[u] : 0.0;
    __syncthreads();
    const int t = threadIdx.x;
    if (t < g.cgc && cg * g.cgc + t < g.C) {
        double s = 0.0;
        for (int i = 0; i < g.pl; ++i) s += red[i * g.cgc + t];
        o[cg * g.cgc + t] = s;
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------ 1. statistics
struct StatK {
    Geo g;
    const float *u, *gamma, *beta;
    float *rm, *rv, *mu, *var, *r, *s, *b;
    double* ws;
    double eps, mom;
    int ld;
};

template <int V>
__global__ __launch_bounds__(kThreads) void bn_stats_kernel(const StatK k) {
    __shared__ double red[kThreads * 4];
    const Geo& g = k.g;
    const int slab = blockIdx.x, cg = blockIdx.y;
    const int cl = threadIdx.x % g.lc, pi = threadIdx.x / g.lc;
    const int c = cg * g.cgc + cl * V;
    const bool active = c < g.C;
    const long long r0 = (long long)slab * g.slab_rows;
    long long r1 = r0 + g.slab_rows;
    if (r1 > g.rows) r1 = g.rows;
    const long long q0 = r0 * g.W, q1 = r1 * g.W;
    double a1[V], a2[V];
#pragma unroll
    for (int u = 0; u < V; ++u) { a1[u] = 0.0; a2[u] = 0.0; }
    if (active)
        for (long long q = q0 + pi; q < q1; q += g.pl) {
            const Vec<V> x = ldv<V>(k.u + q * k.ld + c);
#pragma unroll
            for (int u = 0; u < V; ++u) {
                const double d = (double)x.v[u];
                a1[u] += d;
                a2[u] += d * d;
            }
        }
    double* o = k.ws + (long long)slab * 2 * g.C;
    slab_reduce<V>(red, a1, active, g, cg, o);
    slab_reduce<V>(red, a2, active, g, cg, o + g.C);
}

__global__ __launch_bounds__(kThreads) void bn_stats_finish_kernel(const StatK k) {
    const int C = k.g.C;
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int sl = 0; sl < k.g.slabs; ++sl) {
        const double* q = k.ws + (long long)sl * 2 * C + c;
        s1 += q[0];
        s2 += q[C];
    }
    const double P = (double)k.g.P;
    const double mean = s1 / P;
    double var = s2 / P - mean * mean;
    if (var < 0.0) var = 0.0;
    const double r = 1.0 / sqrt(var + k.eps);
    const double s = (double)k.gamma[c] * r;
    k.mu[c] = (float)mean;
    k.var[c] = (float)var;
    k.r[c] = (float)r;
    k.s[c] = (float)s;
    k.b[c] = (float)((double)k.beta[c] - mean * s);
    if (k.rm) k.rm[c] = (float)((1.0 - k.mom) * (double)k.rm[c] + k.mom * mean);
    if (k.rv) k.rv[c] = (float)((1.0 - k.mom) * (double)k.rv[c] + k.mom * (var * (P / (P - 1.0))));
}

// ------------------------------------------------------------------------------------------------ 2. apply
struct ApplyK {
    const float *u, *s, *b, *w;
    float* out;
    long long P, total;
    int C, CV, ld, act;
};

template <int V>
__global__ __launch_bounds__(kThreads) void bn_apply_kernel(const ApplyK k) {
    const long long item = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (item >= k.total) return;
    const int c = (int)(item % k.CV) * V;
    const long long p = item / k.CV;
    const Vec<V> x = ldv<V>(k.u + p * k.ld + c), s = ldv<V>(k.s + c), b = ldv<V>(k.b + c);
    Vec<V> o;
#pragma unroll
    for (int u = 0; u < V; ++u) o.v[u] = apply_act(bn_pre(x.v[u], s.v[u], b.v[u]), k.act);
    stv<V>(k.out + p * k.C + c, o);
}

// out = act(fma(u, s, b)) + res: bn_apply_kernel's items (a lane owns four channels of a pixel), `res` rows ldr apart
struct ApplyResK {
    const float *u, *s, *b, *res;
    float* out;
    long long total;
    int C, CV, ld, ldr, act;
};

__global__ __launch_bounds__(kThreads) void bn_apply_res_kernel(const ApplyResK k) {
    const long long item = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (item >= k.total) return;
    const int c = (int)(item % k.CV) * 4;
    const long long p = item / k.CV;
    const Vec<4> x = ldv<4>(k.u + p * k.ld + c), s = ldv<4>(k.s + c), b = ldv<4>(k.b + c), r = ldv<4>(k.res + p * k.ldr + c);
    Vec<4> o;
#pragma unroll
    for (int u = 0; u < 4; ++u) o.v[u] = apply_act(bn_pre(x.v[u], s.v[u], b.v[u]), k.act) + r.v[u];
    stv<4>(k.out + p * k.C + c, o);
}

// a wave per pixel: lane l adds its channels 4 l + 256 j (j = 0, 1, ...; the four of a load in channel order) to ONE fp32
// accumulator by fused multiply-adds, and the 64 lanes meet in a butterfly (xor 32, 16, ..., 1)
__global__ __launch_bounds__(kThreads) void bn_apply_dot_kernel(const ApplyK k) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long p = (long long)blockIdx.x * 4 + wave;
    if (p >= k.P) return;                                      // uniform over the wave; the kernel has no barrier
    float acc = 0.f;
    for (int c = lane * 4; c < k.C; c += 256) {
        const Vec<4> x = ldv<4>(k.u + p * k.ld + c), s = ldv<4>(k.s + c), b = ldv<4>(k.b + c), w = ldv<4>(k.w + c);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = fmaf(w.v[u], apply_act(bn_pre(x.v[u], s.v[u], b.v[u]), k.act), acc);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) k.out[p] = acc;
}

// ------------------------------------------------------------------------------------------------ 3. / 4. backward
struct BwdK {
    Geo g;
    const float *gr, *gpix, *gchan, *u, *s, *b, *mu, *r;
    double *ws, *sums;
    float *g_gamma, *g_beta, *g_w, *gu;
    long long total;
    int ldg, ld, act, accumulate, ns;
};

template <int V>
__global__ __launch_bounds__(kThreads) void bn_bwd_sums_kernel(const BwdK k) {
    __shared__ double red[kThreads * 4];
    const Geo& g = k.g;
    const int slab = blockIdx.x, cg = blockIdx.y;
    const int cl = threadIdx.x % g.lc, pi = threadIdx.x / g.lc;
    const int c = cg * g.cgc + cl * V;
    const bool active = c < g.C;
    const long long r0 = (long long)slab * g.slab_rows;
    long long r1 = r0 + g.slab_rows;
    if (r1 > g.rows) r1 = g.rows;
    const long long q0 = r0 * g.W, q1 = r1 * g.W;
    double a0[V], a1[V], a2[V];
#pragma unroll
    for (int u = 0; u < V; ++u) { a0[u] = 0.0; a1[u] = 0.0; a2[u] = 0.0; }
    if (active) {
        const Vec<V> s = ldv<V>(k.s + c), b = ldv<V>(k.b + c), mu = ldv<V>(k.mu + c), r = ldv<V>(k.r + c);
        Vec<V> gc;
        if (!k.gr) gc = ldv<V>(k.gchan + c);
        for (long long q = q0 + pi; q < q1; q += g.pl) {
            const Vec<V> x = ldv<V>(k.u + q * k.ld + c);
            Vec<V> gv;
            float gp = 0.f;
            if (k.gr) {
                gv = ldv<V>(k.gr + q * k.ldg + c);
            } else {
                gp = k.gpix[q];
#pragma unroll
                for (int u = 0; u < V; ++u) gv.v[u] = gp * gc.v[u];
            }
#pragma unroll
            for (int u = 0; u < V; ++u) {
                const float a = bn_pre(x.v[u], s.v[u], b.v[u]);
                const float ga = bn_ga(gv.v[u], a, k.act);
                const float xh = (x.v[u] - mu.v[u]) * r.v[u];
                a0[u] += (double)ga;
                a1[u] += (double)ga * (double)xh;
                if (!k.gr) a2[u] += (double)gp * (double)apply_act(a, k.act);
            }
        }
    }
    double* o = k.ws + (long long)slab * k.ns * g.C;
    slab_reduce<V>(red, a0, active, g, cg, o);
    slab_reduce<V>(red, a1, active, g, cg, o + g.C);
    if (k.ns == 3) slab_reduce<V>(red, a2, active, g, cg, o + 2 * g.C);      // uniform over the launch
}

__global__ __launch_bounds__(kThreads) void bn_bwd_finish_kernel(const BwdK k) {
    const int C = k.g.C;
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= C) return;
    double s[3] = {0.0, 0.0, 0.0};
    for (int sl = 0; sl < k.g.slabs; ++sl) {
        const double* q = k.ws + (long long)sl * k.ns * C + c;
        for (int j = 0; j < k.ns; ++j) s[j] += q[(long long)j * C];
    }
    k.sums[c] = s[0];
    k.sums[C + c] = s[1];
    if (k.g_beta) put(k.g_beta + c, s[0], k.accumulate);
    if (k.g_gamma) put(k.g_gamma + c, s[1], k.accumulate);
    if (k.g_w && k.ns == 3) put(k.g_w + c, s[2], k.accumulate);
}

template <int V>
__global__ __launch_bounds__(kThreads) void bn_bwd_apply_kernel(const BwdK k) {
    const long long item = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (item >= k.total) return;
    const int C = k.g.C, CV = C / V;
    const int c = (int)(item % CV) * V;
    const long long p = item / CV;
    const Vec<V> x = ldv<V>(k.u + p * k.ld + c), s = ldv<V>(k.s + c), b = ldv<V>(k.b + c), mu = ldv<V>(k.mu + c),
                 r = ldv<V>(k.r + c);
    Vec<V> gv;
    if (k.gr) {
        gv = ldv<V>(k.gr + p * k.ldg + c);
    } else {
        const float gp = k.gpix[p];
        const Vec<V> gc = ldv<V>(k.gchan + c);
#pragma unroll
        for (int u = 0; u < V; ++u) gv.v[u] = gp * gc.v[u];
    }
    const double P = (double)k.g.P;
    Vec<V> o;
#pragma unroll
    for (int u = 0; u < V; ++u) {
        const float c1 = (float)(k.sums[c + u] / P), c2 = (float)(k.sums[C + c + u] / P);
        const float a = bn_pre(x.v[u], s.v[u], b.v[u]);
        const float ga = bn_ga(gv.v[u], a, k.act);
        const float xh = (x.v[u] - mu.v[u]) * r.v[u];
        o.v[u] = s.v[u] * fmaf(-xh, c2, ga - c1);
    }
    stv<V>(k.gu + p * C + c, o);
}

// ------------------------------------------------------------------------------------------------ 5. depthwise weight gradient
struct DwK {
    Geo g;
    const float *gr, *e;
    double* ws;
    float* out;
    int ldg, lde, accumulate;
};

__global__ __launch_bounds__(kThreads) void dw_wgrad_kernel(const DwK k) {
    __shared__ double red[kThreads * 4];
    const Geo& g = k.g;
    const int slab = blockIdx.x, cg = blockIdx.y;
    const int cl = threadIdx.x % g.lc, pi = threadIdx.x / g.lc;
    const int c = cg * g.cgc + cl * 4;
    const bool active = c < g.C;
    const long long r0 = (long long)slab * g.slab_rows;
    long long r1 = r0 + g.slab_rows;
    if (r1 > g.rows) r1 = g.rows;
    const long long q0 = r0 * g.W, q1 = r1 * g.W;
    double acc[9][4];
#pragma unroll
    for (int j = 0; j < 9; ++j)
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[j][u] = 0.0;
    if (active)
        for (long long q = q0 + pi; q < q1; q += g.pl) {
            const long long row = q / g.W;
            const int x = (int)(q - row * g.W);
            const int yy = (int)(row % g.H);                   // the row inside ITS frame: no frame sees its neighbour
            const Vec<4> gv = ldv<4>(k.gr + q * k.ldg + c);
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int iy = yy + ky - 1;
                if (iy < 0 || iy >= g.H) continue;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int ix = x + kx - 1;
                    if (ix < 0 || ix >= g.W) continue;
                    const Vec<4> ev = ldv<4>(k.e + (q + (long long)(ky - 1) * g.W + (kx - 1)) * k.lde + c);
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc[ky * 3 + kx][u] += (double)gv.v[u] * (double)ev.v[u];
                }
            }
        }
    double* o = k.ws + (long long)slab * 9 * g.C;
#pragma unroll
    for (int j = 0; j < 9; ++j) slab_reduce<4>(red, acc[j], active, g, cg, o + (long long)j * g.C);
}

__global__ __launch_bounds__(kThreads) void dw_wgrad_finish_kernel(const DwK k) {
    const int C = k.g.C;
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= C) return;
    double s[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) s[j] = 0.0;
    for (int sl = 0; sl < k.g.slabs; ++sl) {
        const double* q = k.ws + (long long)sl * 9 * C + c;
#pragma unroll
        for (int j = 0; j < 9; ++j) s[j] += q[(long long)j * C];
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) put(k.out + (long long)c * 9 + j, s[j], k.accumulate);
}

// a tensor read `vec` floats at a time: the pointer and the pitch
bool alv(const void* p, int ld, int vec) { return vec == 1 ? al4(p) : (al16(p) && !(ld & 3)); }
bool blocks_ok(long long total, unsigned& blocks) {
    const long long b = (total + kThreads - 1) / kThreads;
    if (b <= 0 || b > 0x7fffffffll) return false;
    blocks = (unsigned)b;
    return true;
}

}  // namespace

extern "C" int uavsal_bn_sizeof_desc(int which) {
    return which == 0 ? (int)sizeof(uavsal_bn_stats_desc) : which == 1 ? (int)sizeof(uavsal_bn_apply_desc)
         : which == 2 ? (int)sizeof(uavsal_bn_bwd_desc) : which == 3 ? (int)sizeof(uavsal_dw_wgrad_desc) : -1;
}

extern "C" int uavsal_bn_slabs(int n_img, int H, int W) {
    Geo g;
    return geo_plan(n_img, H, W, 4, g) ? g.slabs : 0;
}

extern "C" int uavsal_bn_slab_rows(int n_img, int H, int W) {
    Geo g;
    return geo_plan(n_img, H, W, 4, g) ? g.slab_rows : 0;
}

extern "C" int64_t uavsal_bn_stats_workspace_bytes(const uavsal_bn_stats_desc* d) {
    Geo g;
    if (!d || !geo_plan(d->n_img, d->H, d->W, d->C, g)) return 0;
    return (int64_t)g.slabs * 2 * g.C * (int64_t)sizeof(double);
}

extern "C" int uavsal_bn_stats(const uavsal_bn_stats_desc* d, uavsal_stream_t stream) {
    if (!d || !d->u || !d->gamma || !d->beta || !d->ws || !d->mu || !d->var || !d->r || !d->s || !d->b) return UAVSAL_EINVAL;
    if (d->n_img <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0 || d->ld < d->C) return UAVSAL_EINVAL;
    if (!(d->eps >= 0.0) || !(d->momentum >= 0.0 && d->momentum <= 1.0)) return UAVSAL_EINVAL;
    StatK k;
    if (!geo_plan(d->n_img, d->H, d->W, d->C, k.g)) return UAVSAL_ESHAPE;
    if ((d->running_mean || d->running_var) && k.g.P < 2) return UAVSAL_ESHAPE;      // the unbiased variance needs two values
    if (d->ws_bytes < uavsal_bn_stats_workspace_bytes(d)) return UAVSAL_EINVAL;
    if (!alv(d->u, d->ld, k.g.vec) || !al8(d->ws)) return UAVSAL_EALIGN;
    const void* f4[] = {d->gamma, d->beta, d->running_mean, d->running_var, d->mu, d->var, d->r, d->s, d->b};
    for (const void* p : f4)
        if (!al4(p)) return UAVSAL_EALIGN;
    k.u = d->u; k.ld = d->ld; k.gamma = d->gamma; k.beta = d->beta; k.rm = d->running_mean; k.rv = d->running_var;
    k.mu = d->mu; k.var = d->var; k.r = d->r; k.s = d->s; k.b = d->b; k.ws = d->ws; k.eps = d->eps; k.mom = d->momentum;
    const dim3 grid((unsigned)k.g.slabs, (unsigned)k.g.cgs);
    if (k.g.vec == 4) hipLaunchKernelGGL(bn_stats_kernel<4>, grid, dim3(kThreads), 0, (hipStream_t)stream, k);
    else hipLaunchKernelGGL(bn_stats_kernel<1>, grid, dim3(kThreads), 0, (hipStream_t)stream, k);
    hipLaunchKernelGGL(bn_stats_finish_kernel, dim3((unsigned)((k.g.C + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, k);
    return uavsal_launch_status();
}

extern "C" int uavsal_bn_apply(const uavsal_bn_apply_desc* d, uavsal_stream_t stream) {
    if (!d || !d->u || !d->s || !d->b || !d->out) return UAVSAL_EINVAL;
    if (d->n_pix <= 0 || d->C <= 0 || d->ld < d->C) return UAVSAL_EINVAL;
    if (d->act != UAVSAL_ACT_NONE && d->act != UAVSAL_ACT_RELU6 && d->act != UAVSAL_ACT_SIGMOID) return UAVSAL_EINVAL;
    if (d->C != 1 && (d->C & 3)) return UAVSAL_ESHAPE;
    const int vec = d->C == 1 ? 1 : 4;
    if (d->dot_w && vec != 4) return UAVSAL_ESHAPE;
    if (!alv(d->u, d->ld, vec) || !alv(d->s, 0, vec) || !alv(d->b, 0, vec)) return UAVSAL_EALIGN;
    if (d->dot_w ? (!al16(d->dot_w) || !al4(d->out)) : !alv(d->out, 0, vec)) return UAVSAL_EALIGN;
    ApplyK k;
    k.u = d->u; k.s = d->s; k.b = d->b; k.w = d->dot_w; k.out = d->out; k.P = d->n_pix; k.C = d->C; k.CV = d->C / vec;
    k.ld = d->ld; k.act = d->act;
    k.total = k.P * k.CV;
    unsigned blocks;
    if (d->dot_w) {
        const long long b = (k.P + 3) / 4;
        if (b > 0x7fffffffll) return UAVSAL_ESHAPE;
        hipLaunchKernelGGL(bn_apply_dot_kernel, dim3((unsigned)b), dim3(kThreads), 0, (hipStream_t)stream, k);
        return uavsal_launch_status();
    }
    if (!blocks_ok(k.total, blocks)) return UAVSAL_ESHAPE;
    if (vec == 4) hipLaunchKernelGGL(bn_apply_kernel<4>, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, k);
    else hipLaunchKernelGGL(bn_apply_kernel<1>, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, k);
    return uavsal_launch_status();
}

extern "C" int uavsal_block_bn_sizeof_desc(int which) { return which == 0 ? (int)sizeof(uavsal_bn_apply_res_desc) : -1; }

extern "C" int uavsal_bn_apply_res(const uavsal_bn_apply_res_desc* d, uavsal_stream_t stream) {
    if (!d || !d->u || !d->s || !d->b || !d->res || !d->out) return UAVSAL_EINVAL;
    if (d->n_pix <= 0 || d->C <= 0 || d->ld < d->C || d->ldr < d->C) return UAVSAL_EINVAL;
    if (d->act != UAVSAL_ACT_NONE && d->act != UAVSAL_ACT_RELU6 && d->act != UAVSAL_ACT_SIGMOID) return UAVSAL_EINVAL;
    if (d->C & 3) return UAVSAL_ESHAPE;
    if (!alv(d->u, d->ld, 4) || !alv(d->res, d->ldr, 4) || !al16(d->s) || !al16(d->b) || !al16(d->out)) return UAVSAL_EALIGN;
    ApplyResK k;
    k.u = d->u; k.s = d->s; k.b = d->b; k.res = d->res; k.out = d->out; k.C = d->C; k.CV = d->C / 4;
    k.ld = d->ld; k.ldr = d->ldr; k.act = d->act;
    if (d->n_pix > 0x7fffffffffffffffll / k.CV) return UAVSAL_ESHAPE;
    k.total = d->n_pix * k.CV;
    unsigned blocks;
    if (!blocks_ok(k.total, blocks)) return UAVSAL_ESHAPE;
    hipLaunchKernelGGL(bn_apply_res_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, k);
    return uavsal_launch_status();
}

namespace {
// what uavsal_bn_bwd_sums and uavsal_bn_bwd_apply check alike
int bwd_plan(const uavsal_bn_bwd_desc* d, BwdK& k) {
    if (!d || !d->u || !d->s || !d->b || !d->mu || !d->r || !d->sums) return UAVSAL_EINVAL;
    if (!d->g && (!d->g_pix || !d->g_chan)) return UAVSAL_EINVAL;
    if (d->n_img <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0 || d->ld < d->C || (d->g && d->ldg < d->C)) return UAVSAL_EINVAL;
    if (d->act != UAVSAL_ACT_NONE && d->act != UAVSAL_ACT_RELU6 && d->act != UAVSAL_ACT_SIGMOID) return UAVSAL_EINVAL;
    if (!geo_plan(d->n_img, d->H, d->W, d->C, k.g)) return UAVSAL_ESHAPE;
    const int vec = k.g.vec;
    if (!alv(d->u, d->ld, vec) || (d->g && !alv(d->g, d->ldg, vec)) || (!d->g && (!al4(d->g_pix) || !alv(d->g_chan, 0, vec))))
        return UAVSAL_EALIGN;
    if (!alv(d->s, 0, vec) || !alv(d->b, 0, vec) || !alv(d->mu, 0, vec) || !alv(d->r, 0, vec) || !al8(d->sums)) return UAVSAL_EALIGN;
    k.gr = d->g; k.ldg = d->ldg; k.gpix = d->g_pix; k.gchan = d->g_chan; k.u = d->u; k.ld = d->ld;
    k.s = d->s; k.b = d->b; k.mu = d->mu; k.r = d->r; k.ws = d->ws; k.sums = d->sums;
    k.g_gamma = d->g_gamma; k.g_beta = d->g_beta; k.g_w = d->g_w; k.gu = d->gu;
    k.act = d->act; k.accumulate = d->accumulate != 0; k.ns = d->g ? 2 : 3;
    k.total = k.g.P * (k.g.C / vec);
    return 0;
}
}  // namespace

extern "C" int64_t uavsal_bn_bwd_workspace_bytes(const uavsal_bn_bwd_desc* d) {
    Geo g;
    if (!d || !geo_plan(d->n_img, d->H, d->W, d->C, g)) return 0;
    return (int64_t)g.slabs * 3 * g.C * (int64_t)sizeof(double);
}

extern "C" int uavsal_bn_bwd_sums(const uavsal_bn_bwd_desc* d, uavsal_stream_t stream) {
    BwdK k;
    const int rc = bwd_plan(d, k);
    if (rc) return rc;
    if (!d->ws || d->ws_bytes < uavsal_bn_bwd_workspace_bytes(d)) return UAVSAL_EINVAL;
    if (!al8(d->ws) || !al4(d->g_gamma) || !al4(d->g_beta) || !al4(d->g_w)) return UAVSAL_EALIGN;
    const dim3 grid((unsigned)k.g.slabs, (unsigned)k.g.cgs);
    if (k.g.vec == 4) hipLaunchKernelGGL(bn_bwd_sums_kernel<4>, grid, dim3(kThreads), 0, (hipStream_t)stream, k);
    else hipLaunchKernelGGL(bn_bwd_sums_kernel<1>, grid, dim3(kThreads), 0, (hipStream_t)stream, k);
    hipLaunchKernelGGL(bn_bwd_finish_kernel, dim3((unsigned)((k.g.C + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, k);
    return uavsal_launch_status();
}

extern "C" int uavsal_bn_bwd_apply(const uavsal_bn_bwd_desc* d, uavsal_stream_t stream) {
    BwdK k;
    const int rc = bwd_plan(d, k);
    if (rc) return rc;
    if (!d->gu) return UAVSAL_EINVAL;
    if (!alv(d->gu, 0, k.g.vec)) return UAVSAL_EALIGN;
    unsigned blocks;
    if (!blocks_ok(k.total, blocks)) return UAVSAL_ESHAPE;
    if (k.g.vec == 4) hipLaunchKernelGGL(bn_bwd_apply_kernel<4>, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, k);
    else hipLaunchKernelGGL(bn_bwd_apply_kernel<1>, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, k);
    return uavsal_launch_status();
}

extern "C" int64_t uavsal_dw_wgrad_workspace_bytes(const uavsal_dw_wgrad_desc* d) {
    Geo g;
    if (!d || (d->C & 3) || !geo_plan(d->n_img, d->H, d->W, d->C, g)) return 0;
    return (int64_t)g.slabs * 9 * g.C * (int64_t)sizeof(double);
}

extern "C" int uavsal_dw_wgrad(const uavsal_dw_wgrad_desc* d, uavsal_stream_t stream) {
    if (!d || !d->g || !d->e || !d->ws || !d->out) return UAVSAL_EINVAL;
    if (d->n_img <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0 || d->ldg < d->C || d->lde < d->C) return UAVSAL_EINVAL;
    if (d->C & 3) return UAVSAL_ESHAPE;
    DwK k;
    if (!geo_plan(d->n_img, d->H, d->W, d->C, k.g)) return UAVSAL_ESHAPE;
    if (d->ws_bytes < uavsal_dw_wgrad_workspace_bytes(d)) return UAVSAL_EINVAL;
    if (!alv(d->g, d->ldg, 4) || !alv(d->e, d->lde, 4) || !al8(d->ws) || !al4(d->out)) return UAVSAL_EALIGN;
    k.gr = d->g; k.ldg = d->ldg; k.e = d->e; k.lde = d->lde; k.ws = d->ws; k.out = d->out; k.accumulate = d->accumulate != 0;
    hipLaunchKernelGGL(dw_wgrad_kernel, dim3((unsigned)k.g.slabs, (unsigned)k.g.cgs), dim3(kThreads), 0, (hipStream_t)stream, k);
    hipLaunchKernelGGL(dw_wgrad_finish_kernel, dim3((unsigned)((k.g.C + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, k);
    return uavsal_launch_status();
}
