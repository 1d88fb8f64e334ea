// Fine-tuning the ST blocks (train.st_block_backward): what the block backward's kernels (csrc/train_block.hip) and the
// pixel GEMM (csrc/train_decoder.hip, which also takes the 32-wide sides) leave open.  include/uavsal_hip.h states the formulas.
//
// 1. uavsal_cbr_sums: gp = g m6(y) and the channel sums S of a 1x1 conv + BatchNorm + ReLU6.  A workgroup owns a group of
//    32 channels (8 lanes x 4 channels, 16-byte loads: one 128-byte line per pixel) and a slab of whole picture rows counted
//    through all frames; its 256 threads take 32 pixels of the slab per pass.  A thread adds its four channels in double;
//    the 32 pixel lanes of a channel meet in LDS and are added in lane order.  Workspace [slab][C] doubles.  No atomics; the
//    slab size depends on the shape alone.
//
// 2. uavsal_cbr_finish: a thread per channel sums the slabs in slab order in double and writes beta and gamma.
//
// 3. uavsal_tdiff_bwd: the adjoint of uavsal_tdiff (csrc/glue.hip) masked by its input: the access pattern of tdiff_kernel, a
//    thread per four channels of a pixel; it gathers the at most six terms of frames j - 1, j, j + 1 of ITS sequence in a
//    fixed order in double.
#include "common.h"
#include "train_sums.h"

namespace {

using sums::put;
constexpr int kCG = 32;                      // channels of one workgroup of the sums: 8 lanes x 4
constexpr int kPixLanes = 32;                // pixels of one pass: 256 threads / 8
constexpr int kSlabPixels = 512;             // pixels of a slab

// ------------------------------------------------------------------------------------------------ gp and S
struct SumK {
    const float *g, *y;
    float* gp;
    double* ws;
    long long rows;             // n_img * H
    int W, C, ldg, ldy, slab_rows, slabs;
};

__global__ __launch_bounds__(256) void cbr_sums_kernel(const SumK p) {
    __shared__ double red[kPixLanes * kCG];
    const int slab = blockIdx.x, cg = blockIdx.y;
    const int cl = (threadIdx.x & 7) * 4, pl = threadIdx.x >> 3;
    const int c = cg * kCG + cl;
    const long long r0 = (long long)slab * p.slab_rows;
    long long r1 = r0 + p.slab_rows;
    if (r1 > p.rows) r1 = p.rows;
    const long long q0 = r0 * p.W, q1 = r1 * p.W;              // global pixels of the slab

    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long q = q0 + pl; q < q1; q += kPixLanes) {
        const f32x4 gv = ld4(p.g + q * p.ldg + c);
        const f32x4 yv = ld4(p.y + q * p.ldy + c);
        f32x4 v;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            v[u] = (yv[u] > 0.f && yv[u] < 6.f) ? gv[u] : 0.f;
            acc[u] += (double)v[u];
        }
        *reinterpret_cast<f32x4*>(p.gp + q * p.C + c) = v;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) red[pl * kCG + cl + u] = acc[u];
    __syncthreads();
    if (threadIdx.x < kCG) {                                   // the 32 pixel lanes of a channel in lane order
        double s = 0.0;
        for (int i = 0; i < kPixLanes; ++i) s += red[i * kCG + threadIdx.x];
        p.ws[(long long)slab * p.C + cg * kCG + threadIdx.x] = s;
    }
}

bool sums_plan(const uavsal_cbr_sums_desc* d, SumK& k) {
    if (!d || d->n_img <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0 || (d->C % kCG)) return false;
    if ((long long)d->H * d->W > 0x7fffffffll || d->C / kCG > 65535) return false;
    k.W = d->W; k.C = d->C;
    k.rows = (long long)d->n_img * d->H;
    return sums::slab_rule(k.rows, d->W, kSlabPixels, k.slab_rows, k.slabs);
}

// ------------------------------------------------------------------------------------------------ finalise
struct FinK {
    const double *ws, *rowdot;
    const float *r, *mu;
    float *g_gamma, *g_beta;
    int C, slabs, accumulate;
};

__global__ __launch_bounds__(256) void cbr_finish_kernel(const FinK k) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= k.C) return;
    double S = 0.0;
    for (int sl = 0; sl < k.slabs; ++sl) S += k.ws[(long long)sl * k.C + c];
    put(k.g_beta + c, S, k.accumulate);
    put(k.g_gamma + c, (double)k.r[c] * (k.rowdot[c] - (double)k.mu[c] * S), k.accumulate);
}

// ------------------------------------------------------------------------------------------------ adjoint of tdiff
struct TbK { const float *g, *r; float* out; int ldg, ldr, ldo, HW, C4, L; long long total; };

__global__ __launch_bounds__(256) void tdiff_bwd_kernel(const TbK p) {
    const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
    if (item >= p.total) return;
    const int c = (int)(item % p.C4) * 4;
    long long t = item / p.C4;
    const int pix = (int)(t % p.HW);
    const int n = (int)(t / p.HW);
    const int j = n % p.L;
    const size_t img = (size_t)p.HW * p.ldg;
    const float* cur = p.g + (size_t)n * img + (size_t)pix * p.ldg + c;       // P_j; Q_j at + C
    const int C = p.C4 * 4;
    double s[4];
    const auto add = [&](const float* q, double sp, double sq) {              // + sp P + sq Q of one frame (0: not read)
        if (sp != 0.0) {
            const f32x4 v = ld4(q);
#pragma unroll
            for (int u = 0; u < 4; ++u) s[u] += sp * (double)v[u];
        }
        if (sq != 0.0) {
            const f32x4 v = ld4(q + C);
#pragma unroll
            for (int u = 0; u < 4; ++u) s[u] += sq * (double)v[u];
        }
    };
#pragma unroll
    for (int u = 0; u < 4; ++u) s[u] = 0.0;
    if (j == 0) add(cur, -1.0, 1.0);                           // dif[0] = [r1 - r0, r0 - r1]
    else if (j == p.L - 1) add(cur, 1.0, -1.0);                // dif[L-1] = [r[L-1] - r[L-2], r[L-2] - r[L-1]]
    else add(cur, 1.0, 1.0);                                   // dif[j] = [r[j] - r[j-1], r[j] - r[j+1]]
    if (j >= 1) {                                              // frame j - 1 reads r[j] as its next frame
        if (j - 1 == 0) add(cur - img, 1.0, -1.0);
        else add(cur - img, 0.0, -1.0);
    }
    if (j <= p.L - 2) {                                        // frame j + 1 reads r[j] as its previous frame
        if (j + 1 == p.L - 1) add(cur + img, -1.0, 1.0);
        else add(cur + img, -1.0, 0.0);
    }
    const size_t row = (size_t)n * p.HW + pix;
    const f32x4 rv = ld4(p.r + row * p.ldr + c);
    f32x4 v;
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = (rv[u] > 0.f && rv[u] < 6.f) ? (float)s[u] : 0.f;
    *reinterpret_cast<f32x4*>(p.out + row * p.ldo + c) = v;
}

}  // namespace

extern "C" int uavsal_st_sizeof_desc(int which) {
    return which == 0 ? (int)sizeof(uavsal_cbr_sums_desc) : which == 1 ? (int)sizeof(uavsal_cbr_finish_desc)
         : which == 2 ? (int)sizeof(uavsal_tdiff_bwd_desc) : -1;
}

extern "C" int uavsal_cbr_sums_slabs(const uavsal_cbr_sums_desc* d) {
    SumK k;
    return sums_plan(d, k) ? k.slabs : 0;
}

extern "C" int uavsal_cbr_sums_slab_rows(const uavsal_cbr_sums_desc* d) {
    SumK k;
    return sums_plan(d, k) ? k.slab_rows : 0;
}

extern "C" int64_t uavsal_cbr_sums_workspace_bytes(const uavsal_cbr_sums_desc* d) {
    SumK k;
    if (!sums_plan(d, k)) return 0;
    return (int64_t)k.slabs * k.C * (int64_t)sizeof(double);
}

extern "C" int uavsal_cbr_sums(const uavsal_cbr_sums_desc* d, uavsal_stream_t stream) {
    if (!d || !d->g || !d->y || !d->gp || !d->ws) return UAVSAL_EINVAL;
    if (d->n_img <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0) return UAVSAL_EINVAL;
    if (d->C % kCG) return UAVSAL_ESHAPE;
    if ((d->ldg & 3) || (d->ldy & 3)) return UAVSAL_EALIGN;
    if (d->ldg < d->C || d->ldy < d->C) return UAVSAL_EINVAL;
    SumK k;
    if (!sums_plan(d, k)) return UAVSAL_ESHAPE;
    if (d->ws_bytes < uavsal_cbr_sums_workspace_bytes(d)) return UAVSAL_EINVAL;
    if (!al16(d->g) || !al16(d->y) || !al16(d->gp) || !al8(d->ws)) return UAVSAL_EALIGN;
    k.g = d->g; k.y = d->y; k.gp = d->gp; k.ws = d->ws; k.ldg = d->ldg; k.ldy = d->ldy;
    hipLaunchKernelGGL(cbr_sums_kernel, dim3((unsigned)k.slabs, (unsigned)(k.C / kCG)), dim3(256), 0, (hipStream_t)stream, k);
    return uavsal_launch_status();
}

extern "C" int uavsal_cbr_finish(const uavsal_cbr_finish_desc* d, uavsal_stream_t stream) {
    if (!d || !d->ws || !d->rowdot || !d->r || !d->mu || !d->g_gamma || !d->g_beta) return UAVSAL_EINVAL;
    if (d->C <= 0 || d->slabs <= 0) return UAVSAL_EINVAL;
    if (d->C % kCG) return UAVSAL_ESHAPE;
    if (d->ws_bytes < (int64_t)d->slabs * d->C * (int64_t)sizeof(double)) return UAVSAL_EINVAL;
    if (!al4(d->r) || !al4(d->mu) || !al4(d->g_gamma) || !al4(d->g_beta) || !al8(d->ws) || !al8(d->rowdot)) return UAVSAL_EALIGN;
    FinK k;
    k.ws = d->ws; k.rowdot = d->rowdot; k.r = d->r; k.mu = d->mu; k.g_gamma = d->g_gamma; k.g_beta = d->g_beta;
    k.C = d->C; k.slabs = d->slabs; k.accumulate = d->accumulate != 0;
    hipLaunchKernelGGL(cbr_finish_kernel, dim3((unsigned)((d->C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, k);
    return uavsal_launch_status();
}

extern "C" int uavsal_tdiff_bwd(const uavsal_tdiff_bwd_desc* d, uavsal_stream_t stream) {
    if (!d || !d->g || !d->r || !d->out) return UAVSAL_EINVAL;
    if (d->n_img <= 0 || d->HW <= 0 || d->C <= 0) return UAVSAL_EINVAL;
    if (d->seq_len < 2 || (d->n_img % d->seq_len)) return UAVSAL_ESHAPE;
    if ((d->C & 3) || (d->ldg & 3) || (d->ldr & 3) || (d->ldo & 3) || d->ldg < 2 * d->C || d->ldr < d->C || d->ldo < d->C)
        return UAVSAL_EALIGN;
    if (!al16(d->g) || !al16(d->r) || !al16(d->out)) return UAVSAL_EALIGN;
    TbK k;
    k.g = d->g; k.r = d->r; k.out = d->out; k.ldg = d->ldg; k.ldr = d->ldr; k.ldo = d->ldo;
    k.HW = d->HW; k.C4 = d->C / 4; k.L = d->seq_len;
    k.total = (long long)d->n_img * d->HW * k.C4;
    const long long blocks = (k.total + 255) / 256;
    if (blocks <= 0 || blocks > 0x7fffffffll) return UAVSAL_ESHAPE;
    hipLaunchKernelGGL(tdiff_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, k);
    return uavsal_launch_status();
}
