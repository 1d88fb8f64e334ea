// Back-propagation through the ConvTWA recurrence (model.rnn, model_convlstm.py:238-295) and the input gradient of the
// frozen decoder conv_out_st: the three launches the existing kernels cannot do (include/uavsal_hip.h states the formulas).
//
// 1. uavsal_twa_gate_bwd: element-wise, 16 bytes per lane.  The gate i = sigmoid(z) and its complement are both formed from
//    e = exp(-|z|): for z >= 0  i = 1 / (1 + e), 1 - i = e / (1 + e), mirrored below zero.  1 - fl(i) would lose all relative
//    accuracy in a saturated gate, and dz carries the factor i (1 - i).
//
// 2. uavsal_twa_wgrad: dW = dz^T . im2col(cat[x, h_prev]) with the reduction over pixels.  Both operands are pixel-major with
//    the M (output channel) / N (input channel) index contiguous, which is what v_mfma_f32_32x32x2_f32 reads from LDS without
//    a transpose: lane l takes A[m = l & 31][k = l >> 5] = dz[pixel k][co m] and B[k][n = l & 31] = cat[pixel k + tap][ci n].
//    (The tile loop itself -- K steps, MFMA tiles, chains -- is csrc/pix_gemm_tile.h, shared with uavsal_pix_gemm of
//    csrc/train_decoder.hip; this file supplies the operand loaders: the rows of dz, and b_row below.)
//      tiles   128 (co) x 128 (ci of ONE tap; 256 % 128 == 0, so a tile reads x or the history, never both): 2 x 36 = 72.
//      K step  32 pixels: 2 x 20 KB of LDS (32 rows of 128 floats padded to 160: the two half-waves of a ds_read_b32 hit disjoint banks),
//              loaded as float4 by 256 threads, the next step's global loads in flight while the current one multiplies.
//              The tap shift and the border mask are in the B loader: a row whose shifted pixel leaves the picture, or whose
//              pixel lies behind the last frame, is zeros -- nothing is read out of bounds and no frame sees its neighbour.
//      wave    2 x 2 MFMA tiles of 32 x 32 (four independent accumulators: the issue rate of the fp32 MFMA, 64 cycles each).
//      K split 72 tiles do not fill 256 CUs.  The pixels are cut into chunks of UAVSAL_WGRAD_CHAIN = 1024 (32 K steps): one
//              accumulation chain never exceeds 1024 products, the range where the fp32 MFMA chain was measured at
//              0.75-1.5e-7 sum|ab|.  A workgroup owns `cps` whole chunks of one tile (a share); after every chunk it adds the
//              chain's tile to a second fp32 register tile and starts a new chain.  Shares are sized for about 1024 workgroups in
//              the grid (kTargetWGs, four per CU queued); the reference's T = 20 at 45 x 80 (71 chunks) runs 12 shares of 6
//              chunks, 864 workgroups.  How many are RESIDENT per CU was not measured: 40 KB of LDS allows four, the two
//              64-register accumulator tiles plus 32 prefetch registers per lane more likely two.
//      reduce  partial tiles [share][co][tap][ci] -> a second launch sums the shares in share order in double, adds the old
//              value when accumulating, rounds once and writes [co][ci][tap].  No atomics anywhere.
//      error   per element: each chain <= 1.5e-7 S_chain, each of the <= cps fp32 adds u |partial|, the double sum ~1e-16:
//              well inside LAMBDA u sqrt(T H W) sum|dz||cat| (tests/train_ref64.py).
//
// 3. uavsal_dec_bwd: the access pattern of dw3x3_kernel (csrc/dw_conv.hip): a lane owns four channels of a 2 x 2 pixel
//    patch, reads the 4 x 4 halo of d once, masks it, scales it by the per-pixel factor gy y (1 - y) s3 and correlates with the
//    flipped depthwise taps.  Reads e and d, writes ge: 3 x 1536 channels x 4 bytes per pixel.
#include "common.h"
#include "pix_gemm_tile.h"

namespace {

using pixgemm::kTile; using pixgemm::kStep; using pixgemm::kRow; using pixgemm::kTargetWGs; using pixgemm::ld4;
constexpr int kC = 256;                      // hidden channels: the only size the model builds
constexpr int kNT = 9 * (2 * kC / kTile);    // 36 N tiles
constexpr int kTiles = (kC / kTile) * kNT;   // 72

// ------------------------------------------------------------------------------------------------ gate
struct GateK {
    const float *g, *carry, *z, *x, *h;
    float *dz, *co, *dx;
    long long n4; int C4, ldg, ldx, ldh, C;
};

__global__ __launch_bounds__(256) void twa_gate_bwd_kernel(const GateK k) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= k.n4) return;
    const long long p = i / k.C4;
    const int c = (int)(i - p * k.C4) * 4;
    const long long o = p * k.C + c;
    f32x4 g = ld4(k.g + p * k.ldg + c);
    if (k.carry) g += ld4(k.carry + o);
    const f32x4 z = ld4(k.z + o), x = ld4(k.x + p * k.ldx + c), h = ld4(k.h + p * k.ldh + c);
    f32x4 dz, co, dx;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float e = expf(-fabsf(z[q]));
        const float big = 1.f / (1.f + e), small = e / (1.f + e);
        const float gi = z[q] >= 0.f ? big : small, gc = z[q] >= 0.f ? small : big;
        dz[q] = g[q] * (x[q] - h[q]) * (gi * gc);
        co[q] = g[q] * gc;
        dx[q] = g[q] * gi;
    }
    *reinterpret_cast<f32x4*>(k.dz + o) = dz;
    *reinterpret_cast<f32x4*>(k.co + o) = co;
    if (k.dx) *reinterpret_cast<f32x4*>(k.dx + o) = dx;
}

// ------------------------------------------------------------------------------------------------ weight gradient
struct WgK {
    const float *dz, *x, *h, *h0;
    float* ws; float* out;
    int ldx, ldh, ldh0;
    int T, H, W, HW;
    long long K;            // T * H * W
    int cps, shares, accumulate;
};

// the B row of global pixel `g` for tap (ky, kx): pointer to 128 channels, or nullptr for a row of zeros
__device__ __forceinline__ const float* b_row(const WgK& k, long long g, int dy, int dx, int ci0) {
    if (g >= k.K) return nullptr;
    const int t = (int)(g / k.HW);
    const int r = (int)(g - (long long)t * k.HW);
    const int y = r / k.W, x = r - y * k.W;
    const int yy = y + dy, xx = x + dx;
    if (yy < 0 || yy >= k.H || xx < 0 || xx >= k.W) return nullptr;
    const long long q = (long long)yy * k.W + xx;
    if (ci0 < kC) return k.x + ((long long)t * k.HW + q) * k.ldx + ci0;
    if (t == 0) return k.h0 + q * k.ldh0 + (ci0 - kC);
    return k.h + ((long long)(t - 1) * k.HW + q) * k.ldh + (ci0 - kC);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void twa_wgrad_kernel(const WgK k) {
    const int tile = blockIdx.x, share = blockIdx.y;
    const int mt = tile % (kC / kTile), nt = tile / (kC / kTile);
    const int tap = nt / (2 * kC / kTile), ci0 = (nt % (2 * kC / kTile)) * kTile;
    const int dy = tap / 3 - 1, dx = tap % 3 - 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = (wave & 1) * 64, wn = (wave >> 1) * 64;
    const int lc = (threadIdx.x & 31) * 4;

    const long long p0 = (long long)share * k.cps * UAVSAL_WGRAD_CHAIN;
    long long p1 = p0 + (long long)k.cps * UAVSAL_WGRAD_CHAIN;
    if (p1 > k.K) p1 = k.K;

    f32x16 tot[2][2];
    pixgemm::tile_loop(p0, p1,
        [&](long long g) { return k.dz + g * kC + mt * kTile + lc; },
        [&](long long g) {
            const float* bp = b_row(k, g, dy, dx, ci0);
            return bp ? bp + lc : nullptr;
        }, tot);
    // D: column n = lane & 31, row m = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).  ws [share][co][tap][ci]
    float* w = k.ws + (long long)share * (kC * 9 * 2 * kC);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = mt * kTile + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                const int ci = ci0 + wn + j * 32 + (lane & 31);
                w[((long long)co * 9 + tap) * (2 * kC) + ci] = tot[i][j][r];
            }
}

__global__ __launch_bounds__(256) void twa_wgrad_reduce_kernel(const WgK k) {
    const int idx = blockIdx.x * 256 + threadIdx.x;           // (co, ci)
    if (idx >= kC * 2 * kC) return;
    const int co = idx / (2 * kC), ci = idx - co * (2 * kC);
    float* o = k.out + (long long)idx * 9;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const float* p = k.ws + ((long long)co * 9 + tap) * (2 * kC) + ci;
        double s = 0.0;
        for (int sh = 0; sh < k.shares; ++sh) s += (double)p[(long long)sh * (kC * 9 * 2 * kC)];
        if (k.accumulate) s += (double)o[tap];
        o[tap] = (float)s;
    }
}

bool wgrad_plan(const uavsal_twa_wgrad_desc* d, WgK& k) {
    if (!d || d->T <= 0 || d->H <= 0 || d->W <= 0) return false;
    k.T = d->T; k.H = d->H; k.W = d->W;
    const long long hw = (long long)d->H * d->W;
    if (hw > 0x7fffffffll) return false;
    k.HW = (int)hw;
    k.K = hw * d->T;
    if (!pixgemm::split(k.K, kTiles, k.cps, k.shares)) return false;      // at most 14 shares
    return true;
}

// ------------------------------------------------------------------------------------------------ decoder
struct DecK {
    const float *gy, *y, *e, *d, *s1, *wd9, *s2, *w3, *s3;
    float* ge;
    long long gi, gr, gc, total;
    int n, H, W, C, C4, tiles_x, tiles_y;
};

__global__ __launch_bounds__(256) void dec_bwd_kernel(const DecK p) {
    const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
    if (item >= p.total) return;
    const int c = (int)(item % p.C4) * 4;
    long long t = item / p.C4;
    const int tx = (int)(t % p.tiles_x); t /= p.tiles_x;
    const int ty = (int)(t % p.tiles_y);
    const int n = (int)(t / p.tiles_y);

    f32x4 wt[9];                                               // flipped: ge[p] = sum_r wd[8 - r] t[p + r - (1,1)]
#pragma unroll
    for (int r = 0; r < 9; ++r) wt[r] = ld4(p.wd9 + (size_t)(8 - r) * p.C + c);
    const f32x4 w3 = ld4(p.w3 + c);
    const float s3 = p.s3[0];
    const int oy0 = ty * 2, ox0 = tx * 2;
    const float* db = p.d + (size_t)n * p.H * p.W * p.C + c;
    const float* yb = p.y + (size_t)n * p.H * p.W;
    const float* gb = p.gy + (long long)n * p.gi;

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
                const size_t pix = (size_t)iy * p.W + ix;
                const float yv = yb[pix];
                const float a = gb[iy * p.gr + ix * p.gc] * yv * (1.f - yv) * s3;
                const f32x4 dv = ld4(db + pix * p.C);
#pragma unroll
                for (int u = 0; u < 4; ++u) row[q][u] = (dv[u] > 0.f && dv[u] < 6.f) ? a * w3[u] : 0.f;
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
    const f32x4 s12 = ld4(p.s1 + c) * ld4(p.s2 + c);
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
            f32x4 v = acc[a][b] * s12;
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = (ev[u] > 0.f && ev[u] < 6.f) ? v[u] : 0.f;
            *reinterpret_cast<f32x4*>(p.ge + o) = v;
        }
    }
}


}  // namespace

extern "C" int uavsal_train_sizeof_desc(int which) {
    return which == 0 ? (int)sizeof(uavsal_twa_gate_desc) : which == 1 ? (int)sizeof(uavsal_twa_wgrad_desc)
         : which == 2 ? (int)sizeof(uavsal_dec_bwd_desc) : -1;
}

extern "C" int uavsal_twa_gate_bwd(const uavsal_twa_gate_desc* d, uavsal_stream_t stream) {
    if (!d || !d->g || !d->z || !d->x || !d->hprev || !d->dz || !d->carry_out) return UAVSAL_EINVAL;
    if (d->n_pix <= 0 || d->C <= 0) return UAVSAL_EINVAL;
    if (d->C != kC) return UAVSAL_ESHAPE;
    if (d->ldg < d->C || d->ldx < d->C || d->ldh < d->C) return UAVSAL_EINVAL;
    if ((d->ldg | d->ldx | d->ldh) & 3) return UAVSAL_EALIGN;
    if (!al16(d->g) || !al16(d->z) || !al16(d->x) || !al16(d->hprev) || !al16(d->dz) || !al16(d->carry_out) ||
        (d->carry && !al16(d->carry)) || (d->dx && !al16(d->dx))) return UAVSAL_EALIGN;
    GateK k;
    k.g = d->g; k.carry = d->carry; k.z = d->z; k.x = d->x; k.h = d->hprev;
    k.dz = d->dz; k.co = d->carry_out; k.dx = d->dx;
    k.C = d->C; k.C4 = d->C / 4; k.n4 = d->n_pix * k.C4;
    k.ldg = d->ldg; k.ldx = d->ldx; k.ldh = d->ldh;
    const long long blocks = (k.n4 + 255) / 256;
    if (blocks > 0x7fffffffll) return UAVSAL_ESHAPE;
    hipLaunchKernelGGL(twa_gate_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, k);
    return uavsal_launch_status();
}

extern "C" int uavsal_twa_wgrad_shares(const uavsal_twa_wgrad_desc* d) {
    WgK k;
    return wgrad_plan(d, k) ? k.shares : 0;
}

extern "C" int64_t uavsal_twa_wgrad_workspace_bytes(const uavsal_twa_wgrad_desc* d) {
    WgK k;
    if (!wgrad_plan(d, k)) return 0;
    return (int64_t)k.shares * kC * 9 * 2 * kC * (int64_t)sizeof(float);
}

extern "C" int uavsal_twa_wgrad(const uavsal_twa_wgrad_desc* d, uavsal_stream_t stream) {
    if (!d || !d->dz || !d->x || !d->h0 || !d->ws || !d->out) return UAVSAL_EINVAL;
    if (d->T <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0) return UAVSAL_EINVAL;
    if (d->T > 1 && !d->h) return UAVSAL_EINVAL;
    if (d->C != kC) return UAVSAL_ESHAPE;
    WgK k;
    if (!wgrad_plan(d, k)) return UAVSAL_ESHAPE;
    if (d->ws_bytes < uavsal_twa_wgrad_workspace_bytes(d)) return UAVSAL_EINVAL;
    if (d->ldx < kC || d->ldh0 < kC || (d->T > 1 && d->ldh < kC)) return UAVSAL_EINVAL;
    if ((d->ldx | d->ldh0 | (d->T > 1 ? d->ldh : 0)) & 3) return UAVSAL_EALIGN;
    if (!al16(d->dz) || !al16(d->x) || !al16(d->h0) || !al16(d->ws) || (d->h && !al16(d->h)) ||
        (reinterpret_cast<uintptr_t>(d->out) & 3u)) return UAVSAL_EALIGN;
    k.dz = d->dz; k.x = d->x; k.h = d->h; k.h0 = d->h0; k.ws = d->ws; k.out = d->out;
    k.ldx = d->ldx; k.ldh = d->ldh; k.ldh0 = d->ldh0;
    k.accumulate = d->accumulate != 0;
    hipLaunchKernelGGL(twa_wgrad_kernel, dim3(kTiles, (unsigned)k.shares), dim3(256), 0, (hipStream_t)stream, k);
    hipLaunchKernelGGL(twa_wgrad_reduce_kernel, dim3(kC * 2 * kC / 256), dim3(256), 0, (hipStream_t)stream, k);
    return uavsal_launch_status();
}

extern "C" int uavsal_dec_bwd(const uavsal_dec_bwd_desc* d, uavsal_stream_t stream) {
    if (!d || !d->gy || !d->y || !d->e || !d->d || !d->s1 || !d->wd9 || !d->s2 || !d->w3 || !d->s3 || !d->ge) return UAVSAL_EINVAL;
    if (d->n_img <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0) return UAVSAL_EINVAL;
    if (d->gy_img_pitch < 0 || d->gy_row_pitch < 0 || d->gy_col_pitch < 0) return UAVSAL_EINVAL;
    if (d->C & 3) return UAVSAL_EALIGN;
    if (!al16(d->e) || !al16(d->d) || !al16(d->ge) || !al16(d->s1) || !al16(d->wd9) || !al16(d->s2) || !al16(d->w3)) return UAVSAL_EALIGN;
    if ((long long)d->H * d->W > 0x7fffffffll) return UAVSAL_ESHAPE;
    DecK k;
    k.gy = d->gy; k.y = d->y; k.e = d->e; k.d = d->d; k.s1 = d->s1; k.wd9 = d->wd9; k.s2 = d->s2; k.w3 = d->w3; k.s3 = d->s3;
    k.ge = d->ge; k.gi = d->gy_img_pitch; k.gr = d->gy_row_pitch; k.gc = d->gy_col_pitch;
    k.n = d->n_img; k.H = d->H; k.W = d->W; k.C = d->C; k.C4 = d->C / 4;
    k.tiles_y = (d->H + 1) / 2; k.tiles_x = (d->W + 1) / 2;
    k.total = (long long)d->n_img * k.tiles_y * k.tiles_x * k.C4;
    const long long blocks = (k.total + 255) / 256;
    if (blocks > 0x7fffffffll) return UAVSAL_ESHAPE;
    hipLaunchKernelGGL(dec_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, k);
    return uavsal_launch_status();
}
