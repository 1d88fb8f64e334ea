// The two pieces of the reference's `val` phase that surround the forward (Demo_Train_Test.py:87-156), on device:
// the gaze ground truth of a video and the criterion `loss_fu = 10 * KL - 2 * CC - NSS` with its gradient.
//
// 1. uavsal_gaze_prepare: y_gaze [F][2][h][w] fp32 from source-size uint8 fixMap / fixLoc (utils_data.py:229-253).
//    Channel 0 is `padding(fixMap, h, w, 1)` (:321-343): the geometry of letterbox.hip, cv2.resize's 8-bit INTER_LINEAR
//    rule from resize_u8.h (one thread per output pixel, its two taps per axis computed in place), zero bars, values
//    0..255 (preprocess_vidmaps does not divide by 255).  Channel 1 is `padding_fixation(fixLoc, h, w)` (:345-385): one
//    thread per four source pixels of a row; a non-zero pixel (r, c) stores 1.0 at
//        (y0 + rint(r * (rows / h0)), x0 + rint(c * (cols / w0)))        rows x cols = the picture area
//    with the quotient, the product and the round-half-to-even in double (np.round on float64) and an index equal to rows /
//    cols pulled in by one.  At h0 == h and w0 == w the reference returns its input (:366-367): the source VALUE is stored.
//    The output and the flags were zeroed by the caller; writers of one cell store the same value: plain stores.
//    flags [F][2]: 1 where a channel holds a non-zero (np.any(y_gaze, axis=(2, 3)), Demo_Train_Test.py:125).
//
// 2. uavsal_loss_fu (loss_functions.py:43-50, 64-86), per frame with p = pred, t = truth channel 0, f = channel 1, N pixels:
//      kl  = sum t' log(t' / (p' + EPS) + EPS),     t' = t / (sum t + EPS),  p' = p / (sum p + EPS)
//      cc  = r1 / (r2 + EPS),  r1 = sum t~ p~,  r2 = sqrt(sum p~^2 * sum t~^2),  x~ = (x - mean x) / (std x + EPS)
//      nss = sum(f p~) / (sum f + EPS)
//    (`torch.std` is the unbiased one; the second `- get_mean` of metric_cc subtracts the mean of an already centred map,
//    0 up to rounding, and is dropped).  One workgroup per frame, two passes over the frame (sums, then everything that needs
//    the means); per-pixel arithmetic and every sum in double, wave shuffles then a fixed-order sum over the waves in LDS.
//    With q = p - mean p, tc = t - mean t:  sum t~ p~ = sum(tc q) / (dt dp),  sum p~^2 = sum q^2 / dp^2, ... so pass two
//    accumulates sum tc^2, sum q^2, sum tc q, sum f q, kl and sum A p' (for the backward).
//    The means over the frames are taken by a second launch of one wave, lanes striding the frames and a shuffle tree:
//    a fixed order, no float atomics.  (A ticket in the first launch would need its counter cleared on the stream before
//    every call -- a memset node, the cost of the launch it saves.)
//
// 3. uavsal_loss_fu_grad: with g = *grad_out / B, D = sum p + EPS, Y = std p + EPS, c = std t + EPS, gam = 1 / ((N - 1) std p)
//    (= d std p / d p_k per q_k), X = sum tc q, Z = sqrt(sum q^2 sum tc^2), r1 = X / (c Y), r2 = Z / (c Y), e = r2 + EPS:
//      d kl  / d p_k = (A_k - sum_j A_j p'_j) / D,         A_j = -t'_j^2 / ((t'_j / (p'_j + EPS) + EPS) (p'_j + EPS)^2)
//      d cc  / d p_k = tc_k / (c Y e) + q_k * (-X gam / (c Y^2 e) - r1 / e^2 * (Z / (sum q^2 c Y) - Z gam / (c Y^2)))
//      d nss / d p_k = ((f_k - sum f / N) / Y - sum(f q) gam q_k / Y^2) / (sum f + EPS)
//    A frame of constant predictions has std p = 0, gam = inf and X = 0: the cc and nss terms are NaN for every pixel,
//    which is what autograd returns for the reference (torch.std at zero).  A term whose weight is 0 is not evaluated
//    (loss_kl's gradient of such a frame is finite, as the reference's is).
#include "common.h"
#include "resize_u8.h"

namespace {

constexpr double kEps = 2.2204e-16;                        // loss_functions.py:6
constexpr int kLossThreads = 1024;
constexpr int kLossWaves = kLossThreads / 64;
constexpr int kGradThreads = 256;
constexpr int kGazeThreads = 256;

enum { S_KL = 0, S_CC, S_NSS, S_SP, S_MP, S_MT, S_SSP, S_SST, S_CTP, S_FP, S_SF, S_SAP, S_ST };

// ------------------------------------------------------------------------------------------------ gaze ground truth

struct GazeK {
    const unsigned char* map; long long map_row, map_col, map_img;
    const unsigned char* loc; long long loc_row, loc_col, loc_img;
    float* out; unsigned char* flags;
    int h0, w0, h, w;
    int new_r, new_c, y0, x0;          // picture area inside h x w (the geometry of letterbox.hip)
    int identity;                      // h0 == h && w0 == w: channel 1 is the source itself
    int resize_blocks, quads;          // blocks of channel 0 in front of the scatter blocks; quads = ceil(w0 / 4)
    double sy, sx;                     // n_in / n_out per axis (resize);
    double fr, fc;                     // rows / h0, cols / w0 (scatter)
};

__global__ __launch_bounds__(kGazeThreads) void gaze_prepare_kernel(const GazeK p) {
    const int img = blockIdx.y;
    float* o = p.out + (long long)img * 2 * p.h * p.w;
    if ((int)blockIdx.x < p.resize_blocks) {               // channel 0: one output pixel of the picture area per thread
        const int i = blockIdx.x * kGazeThreads + threadIdx.x;
        if (i >= p.new_r * p.new_c) return;
        const int dy = i / p.new_c, dx = i - dy * p.new_c;
        int s0, b0, b1, c0, a0, a1;
        lb_tap(dy, p.sy, p.h0, s0, b0, b1);
        lb_tap(dx, p.sx, p.w0, c0, a0, a1);
        const int s1 = min(s0 + 1, p.h0 - 1), c1 = min(c0 + 1, p.w0 - 1);
        const unsigned char* m = p.map + (long long)img * p.map_img;
        const int v = lb_mix(m[s0 * p.map_row + c0 * p.map_col], m[s0 * p.map_row + c1 * p.map_col],
                             m[s1 * p.map_row + c0 * p.map_col], m[s1 * p.map_row + c1 * p.map_col], a0, a1, b0, b1);
        if (v != 0) {                                      // (the bars and the zeros were written by the caller's fill)
            o[(p.y0 + dy) * p.w + p.x0 + dx] = (float)v;
            p.flags[2 * img] = 1;
        }
        return;
    }
    // channel 1: four adjacent source pixels of one row per thread
    const long long i = (long long)(blockIdx.x - p.resize_blocks) * kGazeThreads + threadIdx.x;
    if (i >= (long long)p.h0 * p.quads) return;
    const int r = (int)(i / p.quads), cq = (int)(i - (long long)r * p.quads) * 4;
    const unsigned char* l = p.loc + (long long)img * p.loc_img + (long long)r * p.loc_row + (long long)cq * p.loc_col;
    const int n = min(4, p.w0 - cq);
    unsigned v4 = 0;
    if (n == 4 && p.loc_col == 1 && (reinterpret_cast<uintptr_t>(l) & 3u) == 0) {
        v4 = *reinterpret_cast<const unsigned*>(l);
    } else {
        for (int j = 0; j < n; ++j) v4 |= (unsigned)l[j * p.loc_col] << (8 * j);
    }
    if (v4 == 0) return;
    float* o1 = o + p.h * p.w;
    int rr = r;
    if (!p.identity) {
        rr = (int)rint(__dmul_rn((double)r, p.fr));        // int(np.round(coord[0] * factor_scale_r))
        if (rr >= p.new_r) rr = p.new_r - 1;               // `if r == rows: r -= 1`; nothing larger can come out
        rr += p.y0;
    }
    for (int j = 0; j < n; ++j) {
        const unsigned v = (v4 >> (8 * j)) & 255u;
        if (v == 0) continue;
        int cc = cq + j;
        if (!p.identity) {
            cc = (int)rint(__dmul_rn((double)cc, p.fc));
            if (cc >= p.new_c) cc = p.new_c - 1;
            cc += p.x0;
        }
        o1[rr * p.w + cc] = p.identity ? (float)v : 1.f;
    }
    p.flags[2 * img + 1] = 1;
}

// ------------------------------------------------------------------------------------------------ criterion

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// sums of K values over the workgroup, the same bits in every thread: shuffles inside a wave, then the waves in order
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
    __syncthreads();                                       // the readers of an earlier call are done
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[k * kLossWaves + wave] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double s = 0.0;
        for (int w = 0; w < kLossWaves; ++w) s += red[k * kLossWaves + w];
        v[k] = s;
    }
}

// pixels 4 i .. 4 i + 3 of a frame (n of them exist): one 16-byte load per map when `vec`
__device__ __forceinline__ int load_px4(const float* p, const float* t, const float* f, int i, int N, int vec,
                                        float (&pp)[4], float (&tt)[4], float (&ff)[4]) {
    if (vec) {
        const f32x4 a = reinterpret_cast<const f32x4*>(p)[i], b = reinterpret_cast<const f32x4*>(t)[i],
                    c = reinterpret_cast<const f32x4*>(f)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) { pp[j] = a[j]; tt[j] = b[j]; ff[j] = c[j]; }
        return 4;
    }
    const int n = min(4, N - 4 * i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool in = j < n;
        pp[j] = in ? p[4 * i + j] : 0.f; tt[j] = in ? t[4 * i + j] : 0.f; ff[j] = in ? f[4 * i + j] : 0.f;
    }
    return n;
}

struct LossK {
    const float* pred; const float* truth; double* stats; float* out;
    const float* grad_out; float* grad;
    int B, N, vec;
    double w_kl, w_cc, w_nss;
};

// d kl / d p' of one pixel (A above) and the pixel's kl term
__device__ __forceinline__ double kl_terms(double t, double p, double Dt, double Dp, double& A_out, double& pn_out) {
    const double tn = t / Dt, pn = p / Dp;
    const double den = pn + kEps;
    const double u = tn / den + kEps;
    A_out = -(tn * tn) / (u * den * den);
    pn_out = pn;
    return tn * log(u);
}

__global__ __launch_bounds__(kLossThreads) void loss_stats_kernel(const LossK k) {
    __shared__ double red[6 * kLossWaves];
    const int img = blockIdx.x, N = k.N;
    const float* p = k.pred + (long long)img * N;
    const float* t = k.truth + (long long)img * 2 * N;
    const float* f = t + N;
    const int n4 = (N + 3) >> 2;
    float pp[4], tt[4], ff[4];

    double a[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n4; i += kLossThreads) {
        const int n = load_px4(p, t, f, i, N, k.vec, pp, tt, ff);
        for (int j = 0; j < n; ++j) { a[0] += (double)tt[j]; a[1] += (double)pp[j]; a[2] += (double)ff[j]; }
    }
    block_sum<3>(a, red);
    const double St = a[0], Sp = a[1], Sf = a[2];
    const double mt = St / N, mp = Sp / N, Dt = St + kEps, Dp = Sp + kEps;

    double b[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n4; i += kLossThreads) {     // (the frame comes back from L2)
        const int n = load_px4(p, t, f, i, N, k.vec, pp, tt, ff);
        for (int j = 0; j < n; ++j) {
            const double tc = (double)tt[j] - mt, q = (double)pp[j] - mp;
            b[0] += tc * tc; b[1] += q * q; b[2] += tc * q; b[3] += (double)ff[j] * q;
            double A, pn;
            b[4] += kl_terms((double)tt[j], (double)pp[j], Dt, Dp, A, pn);
            b[5] += A * pn;
        }
    }
    block_sum<6>(b, red);
    if (threadIdx.x == 0) {
        const double SSt = b[0], SSp = b[1], Ctp = b[2], Fp = b[3];
        const double dt = sqrt(SSt / (N - 1)) + kEps, dp = sqrt(SSp / (N - 1)) + kEps;
        const double r1 = Ctp / (dt * dp);
        const double r2 = sqrt((SSp / (dp * dp)) * (SSt / (dt * dt)));
        double* s = k.stats + (long long)img * UAVSAL_LOSS_NSTAT;
        s[S_KL] = b[4]; s[S_CC] = r1 / (r2 + kEps); s[S_NSS] = (Fp / dp) / (Sf + kEps);
        s[S_SP] = Sp; s[S_MP] = mp; s[S_MT] = mt; s[S_SSP] = SSp; s[S_SST] = SSt; s[S_CTP] = Ctp; s[S_FP] = Fp;
        s[S_SF] = Sf; s[S_SAP] = b[5]; s[S_ST] = St; s[13] = 0.0; s[14] = 0.0; s[15] = 0.0;
    }
}

// one wave: the means over the frames, lanes striding the frames, then the shuffle tree -- the same order every run
__global__ __launch_bounds__(64) void loss_mean_kernel(const LossK k) {
    double s[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < k.B; i += 64) {
        const double* st = k.stats + (long long)i * UAVSAL_LOSS_NSTAT;
        s[0] += st[S_KL]; s[1] += st[S_CC]; s[2] += st[S_NSS];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) s[j] = wave_sum(s[j]) / k.B;
    if (threadIdx.x < 4) {
        const double loss = k.w_kl * s[0] + k.w_cc * s[1] + k.w_nss * s[2];
        k.out[threadIdx.x] = (float)(threadIdx.x == 0 ? s[0] : threadIdx.x == 1 ? s[1] : threadIdx.x == 2 ? s[2] : loss);
    }
}

__global__ __launch_bounds__(kGradThreads) void loss_grad_kernel(const LossK k) {
    const int img = blockIdx.y, N = k.N;
    const int i = blockIdx.x * kGradThreads + threadIdx.x;
    if (i >= ((N + 3) >> 2)) return;
    const double* s = k.stats + (long long)img * UAVSAL_LOSS_NSTAT;
    const double g = (double)k.grad_out[0] / k.B;
    const double mp = s[S_MP], mt = s[S_MT], Sf = s[S_SF];
    const double Dp = s[S_SP] + kEps, Dt = s[S_ST] + kEps;
    // the per-frame coefficients: every thread of the frame computes the same ones
    double alpha = 0.0, beta = 0.0, nf = 0.0, nq = 0.0;
    const bool shape_terms = k.w_cc != 0.0 || k.w_nss != 0.0;
    if (shape_terms) {
        const double SSp = s[S_SSP], SSt = s[S_SST], X = s[S_CTP];
        const double sp = sqrt(SSp / (N - 1));
        const double Y = sp + kEps, c = sqrt(SSt / (N - 1)) + kEps;
        const double gam = 1.0 / ((N - 1) * sp);
        if (k.w_cc != 0.0) {
            const double Z = sqrt(SSp * SSt), cY = c * Y;
            const double r1 = X / cY, e = Z / cY + kEps;
            alpha = k.w_cc / (cY * e);
            beta = k.w_cc * (-X * gam / (cY * Y * e) - r1 / (e * e) * (Z / (SSp * cY) - Z * gam / (cY * Y)));
        }
        if (k.w_nss != 0.0) {
            nf = k.w_nss / (Y * (Sf + kEps));
            nq = -k.w_nss * s[S_FP] * gam / (Y * Y * (Sf + kEps));
        }
    }
    const float* p = k.pred + (long long)img * N;
    const float* t = k.truth + (long long)img * 2 * N;
    float pp[4], tt[4], ff[4];
    const int n = load_px4(p, t, t + N, i, N, k.vec, pp, tt, ff);
    f32x4 out;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double d = 0.0;
        if (k.w_kl != 0.0) {
            double A, pn;
            kl_terms((double)tt[j], (double)pp[j], Dt, Dp, A, pn);
            d += k.w_kl * (A - s[S_SAP]) / Dp;
        }
        if (shape_terms) {
            const double tc = (double)tt[j] - mt, q = (double)pp[j] - mp;
            d += alpha * tc + (beta + nq) * q + nf * ((double)ff[j] - Sf / N);
        }
        out[j] = (float)(g * d);
    }
    float* o = k.grad + (long long)img * N;
    if (k.vec) {
        reinterpret_cast<f32x4*>(o)[i] = out;
    } else {
        for (int j = 0; j < n; ++j) o[4 * i + j] = out[j];
    }
}

int loss_args(const uavsal_loss_desc* d, LossK& k) {
    if (!d || !d->pred || !d->truth || !d->stats) return UAVSAL_EINVAL;
    if (d->n_img <= 0 || d->n_pix <= 0) return UAVSAL_EINVAL;
    if (d->n_pix < 2 || d->n_img > 65535) return UAVSAL_ESHAPE;          // the unbiased std divides by n_pix - 1
    if ((reinterpret_cast<uintptr_t>(d->pred) | reinterpret_cast<uintptr_t>(d->truth)) & 3u) return UAVSAL_EALIGN;
    if (reinterpret_cast<uintptr_t>(d->stats) & 7u) return UAVSAL_EALIGN;
    k.pred = d->pred; k.truth = d->truth; k.stats = d->stats; k.out = d->out; k.grad_out = d->grad_out; k.grad = d->grad;
    k.B = d->n_img; k.N = d->n_pix;
    k.vec = d->n_pix % 4 == 0 && uavsal_aligned16(d->pred) && uavsal_aligned16(d->truth) && (!d->grad || uavsal_aligned16(d->grad));
    k.w_kl = d->w_kl; k.w_cc = d->w_cc; k.w_nss = d->w_nss;
    return 0;
}

}  // namespace

extern "C" int uavsal_gaze_prepare(const uavsal_gaze_desc* d, uavsal_stream_t stream) {
    if (!d || !d->fix_map || !d->fix_loc || !d->out || !d->flags) return UAVSAL_EINVAL;
    if (d->n_img <= 0 || d->h0 <= 0 || d->w0 <= 0 || d->h <= 0 || d->w <= 0) return UAVSAL_EINVAL;
    if (d->map_row_pitch < 0 || d->map_col_pitch < 0 || d->map_img_pitch < 0 || d->loc_row_pitch < 0 ||
        d->loc_col_pitch < 0 || d->loc_img_pitch < 0) return UAVSAL_EINVAL;
    if (d->n_img > 65535) return UAVSAL_ESHAPE;
    GazeK k;
    k.map = d->fix_map; k.map_row = d->map_row_pitch; k.map_col = d->map_col_pitch; k.map_img = d->map_img_pitch;
    k.loc = d->fix_loc; k.loc_row = d->loc_row_pitch; k.loc_col = d->loc_col_pitch; k.loc_img = d->loc_img_pitch;
    k.out = d->out; k.flags = d->flags;
    k.h0 = d->h0; k.w0 = d->w0; k.h = d->h; k.w = d->w;
    if ((double)d->h0 / d->h > (double)d->w0 / d->w) {      // utils_data.py:330-335 / 372-377
        k.new_r = d->h; k.new_c = (int)(((long long)d->w0 * d->h) / d->h0);
        k.y0 = 0; k.x0 = (d->w - k.new_c) / 2;
    } else {                                                // utils_data.py:336-341 / 378-383
        k.new_c = d->w; k.new_r = (int)(((long long)d->h0 * d->w) / d->w0);
        k.x0 = 0; k.y0 = (d->h - k.new_r) / 2;
    }
    if (k.new_r <= 0 || k.new_c <= 0 || k.new_r > d->h || k.new_c > d->w) return UAVSAL_ESHAPE;
    k.identity = d->h0 == d->h && d->w0 == d->w;
    k.sy = (double)d->h0 / k.new_r; k.sx = (double)d->w0 / k.new_c;
    k.fr = (double)k.new_r / (double)d->h0; k.fc = (double)k.new_c / (double)d->w0;
    k.quads = (d->w0 + 3) / 4;
    k.resize_blocks = (k.new_r * k.new_c + kGazeThreads - 1) / kGazeThreads;
    const long long scatter_blocks = ((long long)d->h0 * k.quads + kGazeThreads - 1) / kGazeThreads;
    if (k.resize_blocks + scatter_blocks > 0x7fffffffll) return UAVSAL_ESHAPE;
    dim3 grid((unsigned)(k.resize_blocks + scatter_blocks), (unsigned)d->n_img);
    hipLaunchKernelGGL(gaze_prepare_kernel, grid, dim3(kGazeThreads), 0, (hipStream_t)stream, k);
    return uavsal_launch_status();
}

extern "C" int uavsal_loss_fu(const uavsal_loss_desc* d, uavsal_stream_t stream) {
    LossK k;
    const int e = loss_args(d, k);
    if (e) return e;
    if (!d->out) return UAVSAL_EINVAL;
    hipLaunchKernelGGL(loss_stats_kernel, dim3((unsigned)k.B), dim3(kLossThreads), 0, (hipStream_t)stream, k);
    hipLaunchKernelGGL(loss_mean_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, k);
    return uavsal_launch_status();
}

extern "C" int uavsal_loss_fu_grad(const uavsal_loss_desc* d, uavsal_stream_t stream) {
    LossK k;
    const int e = loss_args(d, k);
    if (e) return e;
    if (!d->grad || !d->grad_out) return UAVSAL_EINVAL;
    if (reinterpret_cast<uintptr_t>(d->grad) & 3u) return UAVSAL_EALIGN;
    dim3 grid((unsigned)(((k.N + 3) / 4 + kGradThreads - 1) / kGradThreads), (unsigned)k.B);
    hipLaunchKernelGGL(loss_grad_kernel, grid, dim3(kGradThreads), 0, (hipStream_t)stream, k);
    return uavsal_launch_status();
}
