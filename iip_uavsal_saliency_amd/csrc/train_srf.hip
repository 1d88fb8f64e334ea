// Fine-tuning the SRF-Net head (model.sfnet behind the frozen MobileNetV2 features): the three launches the other training
// kernels do not cover (include/uavsal_hip.h states the formulas).
//
// 1. uavsal_conv3_wgrad: the weight gradient of a dense 3x3 conv (conv_last, 448 -> 256), G = g^T . im2col(x) with the
//    reduction over pixels.  twa_wgrad_kernel (csrc/train.hip) with the channel counts as arguments: the same tile loop
//    (csrc/pix_gemm_tile.h), 128 (co) x 128 (ci of ONE tap) tiles, the tap shift and the border mask in the B loader -- a row
//    whose shifted pixel leaves the picture is zeros, so nothing is read out of bounds and no frame sees its neighbour --,
//    chunks of UAVSAL_WGRAD_CHAIN pixels, shares from pixgemm::split, partial tiles [share][co][tap][ci].  Ci % 64 == 0: the last
//    tile of a tap may be half empty (448 = 3.5 tiles); its loader hands the tile loop zeros for the columns at and behind Ci
//    and they are not written.  Co = 256, Ci = 448 is 2 x 9 x 4 = 72 tiles, the count of uavsal_twa_wgrad, of which 18 do
//    half the useful work.  The reduce launch, a workgroup per co: a thread sums its elements' shares in share order in
//    double, writes fl(row_scale G) (+ the old value) into [co][ci][tap] and adds w G to its row dot; the 256 partial dots
//    meet in a fixed tree (uavsal_pix_gemm's reduce with the tap transpose of twa_wgrad_reduce_kernel).
//
// 2. uavsal_ir_bwd_dil: uavsal_ir_bwd for a dilated depthwise conv.  A lane owns four channels (16-byte loads) of ONE pixel
//    and gathers its nine taps of gd and d, each bounds-checked; delta2 lives in registers only.  At dilation 6 to 18 on a
//    12 x 20 map neighbouring pixels share no tap, so there is no halo to reuse; the launch reads at most 18 + 1 and writes
//    1 x C x 4 bytes per pixel on a 1/32-scale map.
//
// 3. uavsal_ir_sums_dil lives in csrc/train_block.hip: ir_sums_kernel with the taps of e at dil (ky-1, kx-1) (the dilated
//    tap policy of csrc/train_sums.h); only its descriptor's size is answered here.
#include "common.h"
#include "pix_gemm_tile.h"

namespace {

using pixgemm::kTile;

// ------------------------------------------------------------------------------------------------ weight gradient
struct C3K {
    const float *g, *x, *row_scale, *w;
    double* rowdot;
    float *ws, *out;
    long long K;            // n_img * H * W
    int ldx, H, W, HW, Co, Ci, mt_n, ntap_n;     // ntap_n: N tiles of one tap
    int cps, shares, accumulate;
};

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void conv3_wgrad_kernel(const C3K k) {
    const int tile = blockIdx.x, share = blockIdx.y;
    const int mt = tile % k.mt_n, nt = tile / k.mt_n;
    const int tap = nt / k.ntap_n, ci0 = (nt % k.ntap_n) * kTile;
    const int dy = tap / 3 - 1, dx = tap % 3 - 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = (wave & 1) * 64, wn = (wave >> 1) * 64;
    const int lc = (threadIdx.x & 31) * 4;

    const long long p0 = (long long)share * k.cps * UAVSAL_WGRAD_CHAIN;
    long long p1 = p0 + (long long)k.cps * UAVSAL_WGRAD_CHAIN;
    if (p1 > k.K) p1 = k.K;

    f32x16 tot[2][2];
    const float* arow = k.g + mt * kTile + lc;
    const bool bok = ci0 + lc < k.Ci;                         // Ci % 64 == 0: the last tile of a tap may be half empty
    pixgemm::tile_loop(p0, p1,
        [&](long long g) { return arow + g * k.Co; },
        [&](long long g) -> const float* {
            if (!bok) return nullptr;
            const long long t = g / k.HW;
            const int r = (int)(g - t * k.HW);
            const int y = r / k.W, x = r - y * k.W;
            const int yy = y + dy, xx = x + dx;
            if (yy < 0 || yy >= k.H || xx < 0 || xx >= k.W) return nullptr;
            return k.x + (t * k.HW + (long long)yy * k.W + xx) * k.ldx + ci0 + lc;
        }, tot);
    // D: column n = lane & 31, row m = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).  ws [share][co][tap][ci]
    float* w = k.ws + (long long)share * k.Co * 9 * k.Ci;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = mt * kTile + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                const int ci = ci0 + wn + j * 32 + (lane & 31);
                if (ci < k.Ci) w[((long long)co * 9 + tap) * k.Ci + ci] = tot[i][j][r];
            }
}

__global__ __launch_bounds__(256) void conv3_wgrad_reduce_kernel(const C3K k) {
    __shared__ double red[256];
    const int co = blockIdx.x;
    const long long per = (long long)k.Co * 9 * k.Ci;
    const double rs = k.row_scale ? (double)k.row_scale[co] : 1.0;
    double dot = 0.0;
    for (int j = threadIdx.x; j < 9 * k.Ci; j += 256) {       // j = tap * Ci + ci: the workspace's order
        const int tap = j / k.Ci, ci = j - tap * k.Ci;
        const float* p = k.ws + (long long)co * 9 * k.Ci + j;
        double s = 0.0;
        for (int sh = 0; sh < k.shares; ++sh) s += (double)p[sh * per];
        const long long o = ((long long)co * k.Ci + ci) * 9 + tap;
        if (k.rowdot) dot += (double)k.w[o] * s;
        double v = rs * s;
        if (k.accumulate) v += (double)k.out[o];
        k.out[o] = (float)v;
    }
    if (!k.rowdot) return;                                     // uniform over the workgroup
    red[threadIdx.x] = dot;
    for (int s = 128; s > 0; s >>= 1) {                        // a fixed tree
        __syncthreads();
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    }
    if (threadIdx.x == 0) k.rowdot[co] = red[0];
}

bool c3_shape_ok(const uavsal_conv3_wgrad_desc* d) { return !(d->Co % kTile) && !(d->Ci % (kTile / 2)); }

bool c3_plan(const uavsal_conv3_wgrad_desc* d, C3K& k) {
    if (!d || d->n_img <= 0 || d->H <= 0 || d->W <= 0 || d->Co <= 0 || d->Ci <= 0 || !c3_shape_ok(d)) return false;
    const long long hw = (long long)d->H * d->W;
    if (hw > 0x7fffffffll || (long long)d->Co * 9 * d->Ci > 0x7fffffffll) return false;
    k.H = d->H; k.W = d->W; k.HW = (int)hw; k.Co = d->Co; k.Ci = d->Ci;
    k.K = hw * d->n_img;
    k.mt_n = d->Co / kTile; k.ntap_n = (d->Ci + kTile - 1) / kTile;
    const long long tiles = (long long)k.mt_n * 9 * k.ntap_n;
    if (tiles > 65535) return false;
    return pixgemm::split(k.K, (int)tiles, k.cps, k.shares);
}

// ------------------------------------------------------------------------------------------------ ga from gd, dilated
struct BwdK {
    const float *gd, *d, *e, *wd9, *s2;
    float* ga;
    long long total;
    int H, W, C, C4, dil;
};

__global__ __launch_bounds__(256) void ir_bwd_dil_kernel(const BwdK p) {
    const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
    if (item >= p.total) return;
    const int c = (int)(item % p.C4) * 4;
    const long long q = item / p.C4;                           // global pixel
    const long long row = q / p.W;
    const int x = (int)(q - row * p.W);
    const int y = (int)(row % p.H);                            // the row inside ITS frame: no frame sees its neighbour

    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 9; ++r) {                              // ga[p] = sum_r wd[8 - r] delta2[p + dil (r - (1,1))]
        const int iy = y + (r / 3 - 1) * p.dil, ix = x + (r % 3 - 1) * p.dil;
        if (iy < 0 || iy >= p.H || ix < 0 || ix >= p.W) continue;
        const long long o = (q + (long long)(r / 3 - 1) * p.dil * p.W + (r % 3 - 1) * p.dil) * p.C + c;
        const f32x4 dv = ld4(p.d + o), gv = ld4(p.gd + o);
        const f32x4 wt = ld4(p.wd9 + (size_t)(8 - r) * p.C + c);
        f32x4 d2;
#pragma unroll
        for (int u = 0; u < 4; ++u) d2[u] = (dv[u] > 0.f && dv[u] < 6.f) ? gv[u] : 0.f;
        acc += d2 * wt;
    }
    const f32x4 ev = ld4(p.e + q * p.C + c);
    f32x4 v = acc * ld4(p.s2 + c);
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = (ev[u] > 0.f && ev[u] < 6.f) ? v[u] : 0.f;
    *reinterpret_cast<f32x4*>(p.ga + q * p.C + c) = v;
}

}  // namespace

extern "C" int uavsal_srf_sizeof_desc(int which) {
    return which == 0 ? (int)sizeof(uavsal_conv3_wgrad_desc) : which == 1 ? (int)sizeof(uavsal_ir_bwd_dil_desc)
         : which == 2 ? (int)sizeof(uavsal_ir_sums_dil_desc) : -1;
}

extern "C" int uavsal_conv3_wgrad_shares(const uavsal_conv3_wgrad_desc* d) {
    C3K k;
    return c3_plan(d, k) ? k.shares : 0;
}

extern "C" int64_t uavsal_conv3_wgrad_workspace_bytes(const uavsal_conv3_wgrad_desc* d) {
    C3K k;
    if (!c3_plan(d, k)) return 0;
    return (int64_t)k.shares * k.Co * 9 * k.Ci * (int64_t)sizeof(float);
}

extern "C" int uavsal_conv3_wgrad(const uavsal_conv3_wgrad_desc* d, uavsal_stream_t stream) {
    if (!d || !d->g || !d->x || !d->ws || !d->out) return UAVSAL_EINVAL;
    if (d->n_img <= 0 || d->H <= 0 || d->W <= 0 || d->Co <= 0 || d->Ci <= 0) return UAVSAL_EINVAL;
    if (d->rowdot && !d->w) return UAVSAL_EINVAL;
    if (!c3_shape_ok(d)) return UAVSAL_ESHAPE;
    C3K k;
    if (!c3_plan(d, k)) return UAVSAL_ESHAPE;
    if (d->ws_bytes < uavsal_conv3_wgrad_workspace_bytes(d)) return UAVSAL_EINVAL;
    if (d->ldx < d->Ci) return UAVSAL_EINVAL;
    if (d->ldx & 3) return UAVSAL_EALIGN;
    if (!al16(d->g) || !al16(d->x) || !al16(d->ws) || !al4(d->out) || (d->row_scale && !al4(d->row_scale)) ||
        (d->rowdot && (!al8(d->rowdot) || !al4(d->w)))) return UAVSAL_EALIGN;
    k.g = d->g; k.x = d->x; k.row_scale = d->row_scale; k.w = d->w; k.rowdot = d->rowdot; k.ws = d->ws; k.out = d->out;
    k.ldx = d->ldx;
    k.accumulate = d->accumulate != 0;
    hipLaunchKernelGGL(conv3_wgrad_kernel, dim3((unsigned)(k.mt_n * 9 * k.ntap_n), (unsigned)k.shares), dim3(256), 0,
                       (hipStream_t)stream, k);
    hipLaunchKernelGGL(conv3_wgrad_reduce_kernel, dim3((unsigned)k.Co), dim3(256), 0, (hipStream_t)stream, k);
    return uavsal_launch_status();
}

extern "C" int uavsal_ir_bwd_dil(const uavsal_ir_bwd_dil_desc* d, uavsal_stream_t stream) {
    if (!d || !d->gd || !d->d || !d->e || !d->wd9 || !d->s2 || !d->ga) return UAVSAL_EINVAL;
    if (d->n_img <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0 || d->dil < 1) return UAVSAL_EINVAL;
    if (d->C & 3) return UAVSAL_EALIGN;
    if (!al16(d->gd) || !al16(d->d) || !al16(d->e) || !al16(d->ga) || !al16(d->wd9) || !al16(d->s2)) return UAVSAL_EALIGN;
    if ((long long)d->H * d->W > 0x7fffffffll || (long long)d->dil * 2 > 0x7fffffffll / ((long long)d->W + 1)) return UAVSAL_ESHAPE;
    BwdK k;
    k.gd = d->gd; k.d = d->d; k.e = d->e; k.wd9 = d->wd9; k.s2 = d->s2; k.ga = d->ga;
    k.H = d->H; k.W = d->W; k.C = d->C; k.C4 = d->C / 4; k.dil = d->dil;
    k.total = (long long)d->n_img * d->H * d->W * k.C4;
    const long long blocks = (k.total + 255) / 256;
    if (blocks > 0x7fffffffll) return UAVSAL_ESHAPE;
    hipLaunchKernelGGL(ir_bwd_dil_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, k);
    return uavsal_launch_status();
}
