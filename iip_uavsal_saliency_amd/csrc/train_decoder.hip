// Parameter gradients of the decoder conv_out_st (a dwBlock(256, 1) in eval mode + sigmoid): the three launches behind
// train.decoder_param_grads (include/uavsal_hip.h states the formulas).
//
// 1. uavsal_pix_gemm: out[m][n] = row_scale[m] sum over pixels p of A[p][m] B[p][n].  The tile loop of uavsal_twa_wgrad
//    (csrc/pix_gemm_tile.h: 128 x 128 tiles, 32-pixel K steps, chains of at most UAVSAL_WGRAD_CHAIN products, a second fp32
//    register tile per share) with plain pitched rows as both operands.  M and N are multiples of 64 (a 32-wide side goes to the
//    sibling pix_gemm32_kernel below; with the descriptor's tails32 every other multiple of 32 is taken too, by THIS kernel with
//    quarter-tile tails and shares of 128-pixel units: pg_short_ok below): the last tile of either
//    may be half empty (its loader hands the tile loop zeros, nothing at or behind row M / column N is read or written).  K
//    split by the same rule: ceil(M / 128) ceil(N / 128) tiles, about 1024 workgroups.  M = 1536, N = 256 is 24 tiles, at
//    most 42 shares: T = 20 at 45 x 80 (71 chunks) runs 36 shares of 2 chunks.  Partial tiles [share][M][N] -> a second
//    launch, one workgroup per row m, sums the shares in share order in double, writes fl(row_scale G) (+ the old value) and, when asked, rowdot[m] = sum_n w[m][n] G[m][n] in double: each
//    thread adds its columns n = tid, tid + 256, ... in that order and the 256 partial sums meet in a fixed tree in LDS.
//
// 2. uavsal_dec_sums: the channel sums S3, G3, S2, Gd, S1.  The access pattern of dec_bwd_kernel: a lane owns four channels
//    (16-byte loads), a wave 256 channels.  A workgroup owns one channel group of 256 and a slab of whole picture rows (rows
//    of all frames counted through: a slab may end one frame and begin the next; the halo of e is masked per pixel by the
//    row inside ITS frame, so no frame sees its neighbour); its four waves take the slab's pixels in turn.  Per pixel a lane
//    reads d and ga once and the 3 x 3 neighbourhood of e (neighbouring pixels re-read it from the cache), forms delta3 and
//    delta2 in fp32 as dec_bwd_kernel does, and adds every product to a double accumulator: 4 channels x 12 sums per lane =
//    96 VGPRs of accumulators.  At the end the four waves' sums meet in LDS in wave order and the workgroup writes ONE partial
//    per sum to the workspace [slab][12][C] (+ S3 behind them, by channel group 0).  No atomics; the slab size depends on
//    the shape alone, so two calls return the same bits.
//
// 3. uavsal_dec_finish: one launch, a thread per channel: sums the slabs in slab order in double and writes the eight small
//    gradients, each rounded once.  Workgroup 0 also forms the two one-element gradients of the last BatchNorm, for which it
//    sums G3 of ALL channels itself (sum_c w3[c] G3[c]: per thread its channels in order, then the fixed tree).
#include "common.h"
#include "pix_gemm_tile.h"
#include "train_sums.h"

namespace {

using pixgemm::kTile; using pixgemm::kStep; using pixgemm::kRow;
using sums::kGroup; using sums::put;
constexpr int kNS = UAVSAL_DEC_NSUM;         // 12 sums per channel: G3, S2, Gd[9], S1
constexpr int kSlabPixels = 512;             // pixels of a slab

// ------------------------------------------------------------------------------------------------ pixel GEMM
struct PgK {
    const float *a, *b, *row_scale, *w;
    double* rowdot;
    float *ws, *out;
    long long K;
    long long spp;                               // pixels of one share: cps * UAVSAL_WGRAD_CHAIN, or (tails32) whole kShortUnit's
    int lda, ldb, ldw, ldo, M, N, mt_n, nt_n;
    int cps, shares, accumulate;
};

// kMTail: M % 128 != 0, the last M tile is half empty (or, with tails32, a quarter or three quarters: the loader's test is per
// thread, four columns at lc, and M and N are multiples of 4, so it holds for any tail; so does the row guard of the store).  Without it the kernel is the instruction stream it was before M
// tails existed (the A loader's test and the row guard fold away): the calls with whole M tiles keep their bits and their time.
template <bool kMTail>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void pix_gemm_kernel(const PgK k) {
    const int tile = blockIdx.x, share = blockIdx.y;
    const int mt = tile % k.mt_n, nt = tile / k.mt_n;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = (wave & 1) * 64, wn = (wave >> 1) * 64;
    const int lc = (threadIdx.x & 31) * 4;

    const long long p0 = (long long)share * k.spp;
    long long p1 = p0 + k.spp;
    if (p1 > k.K) p1 = k.K;

    f32x16 tot[2][2];
    const float* arow = k.a + mt * kTile + lc;
    const float* brow = k.b + nt * kTile + lc;
    const bool bok = nt * kTile + lc < k.N;                   // N % 32 == 0: the last N tile may end at any quarter
    const bool aok = !kMTail || mt * kTile + lc < k.M;        // M % 32 == 0: and so may the last M tile
    pixgemm::tile_loop(p0, p1,
        [&](long long g) { return aok ? arow + g * k.lda : nullptr; },
        [&](long long g) { return bok ? brow + g * k.ldb : nullptr; }, tot);
    float* w = k.ws + (long long)share * k.M * k.N;           // ws [share][m][n]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mt * kTile + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                const int n = nt * kTile + wn + j * 32 + (lane & 31);
                if ((!kMTail || m < k.M) && n < k.N) w[(long long)m * k.N + n] = tot[i][j][r];
            }
}

// The sibling for a 32-wide side (an ST block's 32 x 256, 256 x 32, 32 x 384; pg_narrow below): a WAVE owns one whole 32 x 32 output
// tile -- one v_mfma_f32_32x32x2_f32 accumulator (its 64-cycle dependent latency equals its issue interval, so one chain per
// wave does not by itself idle the pipe), no half of a padded tile is multiplied -- and reads its operands from
// global memory in the MFMA's own layout (lane l: pixel p + (l >> 5), column (l & 31) of the tile: two 128-byte rows per
// operand and instruction), kLoads pixel pairs in flight; no LDS, no barrier.  Four tiles to a workgroup (tile = 4 blockIdx.x
// + wave, mt fastest; here k.mt_n, k.nt_n count 32-wide tiles).  Chunks, chains, shares and the workspace as above.
// Measured (profiles/train_st.md, 20 frames of 45 x 80): 0.083 ms for 32 x 256 and 256 x 32, 0.100 ms for 32 x 384 with the
// reduction launch, 14-18 TFLOP/s where the 128 x 128 tile kernel reaches 53 at 256 x 256: the loads are not pipelined under
// the MFMAs (16 loads, a wait, 8 dependent MFMAs) and the K split gives 142-213 workgroups.  The three calls are 0.27 ms of a
// 7.4 ms block backward; a pipelined loader is the next step if that share ever matters.
constexpr int kLoads = 8;

__global__ __launch_bounds__(256) void pix_gemm32_kernel(const PgK k) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile = (int)blockIdx.x * 4 + wave, share = blockIdx.y;
    if (tile >= k.mt_n * k.nt_n) return;                       // uniform over the wave; the kernel has no barrier
    const int mt = tile % k.mt_n, nt = tile / k.mt_n;
    const int half = lane >> 5, col = lane & 31;

    const long long p0 = (long long)share * k.spp;
    long long p1 = p0 + k.spp;
    if (p1 > k.K) p1 = k.K;
    const float* ap = k.a + mt * 32 + col;
    const float* bp = k.b + nt * 32 + col;

    f32x16 tot, acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) { tot[r] = 0.f; acc[r] = 0.f; }
    for (long long c0 = p0; c0 < p1; c0 += UAVSAL_WGRAD_CHAIN) {      // a chain: at most UAVSAL_WGRAD_CHAIN products
        long long c1 = c0 + UAVSAL_WGRAD_CHAIN;
        if (c1 > p1) c1 = p1;
        for (long long q = c0; q < c1; q += 2 * kLoads) {
            float av[kLoads], bv[kLoads];
#pragma unroll
            for (int u = 0; u < kLoads; ++u) {
                const long long g = q + 2 * u + half;
                const bool ok = g < c1;                                 // rows at and behind p1 are zeros and never read
                av[u] = ok ? ap[g * k.lda] : 0.f;
                bv[u] = ok ? bp[g * k.ldb] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < kLoads; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
        }
        tot += acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    }
    float* w = k.ws + (long long)share * k.M * k.N;           // ws [share][m][n]
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        w[(long long)m * k.N + nt * 32 + col] = tot[r];
    }
}

// the 256 doubles of `red` summed in a fixed tree; the result in red[0]
__device__ __forceinline__ void tree256(double* red) {
    for (int s = 128; s > 0; s >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void pix_gemm_reduce_kernel(const PgK k) {
    __shared__ double red[256];
    const int m = blockIdx.x;
    const double rs = k.row_scale ? (double)k.row_scale[m] : 1.0;
    double dot = 0.0;
    for (int n = threadIdx.x; n < k.N; n += 256) {
        const float* p = k.ws + (long long)m * k.N + n;
        double s = 0.0;
        for (int sh = 0; sh < k.shares; ++sh) s += (double)p[(long long)sh * k.M * k.N];
        if (k.rowdot) dot += (double)k.w[(long long)m * k.ldw + n] * s;
        float* o = k.out + (long long)m * k.ldo + n;
        double v = rs * s;
        if (k.accumulate) v += (double)*o;
        *o = (float)v;
    }
    if (!k.rowdot) return;                                     // uniform over the workgroup
    red[threadIdx.x] = dot;
    tree256(red);
    if (threadIdx.x == 0) k.rowdot[m] = red[0];
}

// a 32-wide side (M == 32 or N == 32, the other a multiple of 32 from kNarrowMin to kNarrowMax): pix_gemm32_kernel.  At
// least one whole workgroup of four tiles; every tile of the wide side reads the narrow operand again, which is what the
// shapes of an ST block (256, 384) want.  Narrower and wider ones stay refused, as they always were: the cap only has to
// keep out what re-reading the narrow operand per tile would make slow (1920 x 32 is 60 tiles); 512 is the next power of two
// above the widest shape in use, not a tuned value.  The same kernel takes M a multiple of 64 with N an ODD multiple of 32
// under the same cap (the SRF-Net head's conv_lv3 64 x 32 -- two tiles, two idle waves -- and conv_lv4 128 x 96): the 128 x 128
// tile kernel cannot end a tile at column 32 or 96.
constexpr int kNarrowMin = 128, kNarrowMax = 512;
bool pg_narrow(int M, int N) {
    const int wide = M > N ? M : N;
    if ((M == 32 || N == 32) && !(wide % 32) && wide >= kNarrowMin && wide <= kNarrowMax) return true;
    return !(M % 64) && (N % 64) == 32 && M <= kNarrowMax && N <= kNarrowMax;
}
bool pg_shape_ok(int M, int N) { return pg_narrow(M, N) || (!(M % (kTile / 2)) && !(N % (kTile / 2))); }

// tails32 (uavsal_pix_gemm_desc: opt-in, the weight gradients of the MobileNetV2 blocks 8..17 -- 576 x 96, 960 x 160, 96 x 384,
// 96 x 576, 160 x 576, 160 x 960): every M, N multiple of 32 that the rules above refuse goes to pix_gemm_kernel<true>, whose
// last tile of either side may end at any quarter.  Their K is short (20 frames of 12 x 20 are 4800 pixels: under five chunks,
// on 3 to 16 tiles), so a share is a whole number of kShortUnit pixels, not of chunks, for about kShortWGs workgroups (two
// resident per CU): 960 x 160 at K = 4800 runs 16 tiles x 19 shares of 256 pixels = 304 workgroups where whole chunks give
// 80.  A share's chains still end every UAVSAL_WGRAD_CHAIN products counted from the share's first pixel.
constexpr int kShortUnit = 128, kShortWGs = 512;
bool pg_short_ok(int M, int N) { return M > 0 && N > 0 && !(M % 32) && !(N % 32) && !pg_shape_ok(M, N); }

bool pg_split_short(long long K, int tiles, long long& spp, int& shares_out) {
    const long long units = (K + kShortUnit - 1) / kShortUnit;
    long long want = kShortWGs / tiles;
    if (want < 1) want = 1;
    if (want > units) want = units;
    const long long ups = (units + want - 1) / want;
    const long long shares = (units + ups - 1) / ups;
    if (ups > 0x7fffffffll / kShortUnit || shares > 65535) return false;
    spp = ups * kShortUnit; shares_out = (int)shares;
    return true;
}

bool pg_plan(const uavsal_pix_gemm_desc* d, PgK& k) {
    if (!d || d->K <= 0 || d->M <= 0 || d->N <= 0) return false;
    const bool is_short = d->tails32 && pg_short_ok(d->M, d->N);
    if (!is_short && !pg_shape_ok(d->M, d->N)) return false;
    if (!is_short && pg_narrow(d->M, d->N)) {
        const long long tiles = (long long)(d->M / 32) * (d->N / 32);
        if ((long long)d->M * d->N > 0x7fffffffll || (tiles + 3) / 4 > 65535) return false;
        k.K = d->K; k.M = d->M; k.N = d->N; k.mt_n = d->M / 32; k.nt_n = d->N / 32;
        if (!pixgemm::split(k.K, (int)((tiles + 3) / 4), k.cps, k.shares)) return false;
        k.spp = (long long)k.cps * UAVSAL_WGRAD_CHAIN;
        return true;
    }
    const int mt_n = (d->M + kTile - 1) / kTile, nt_n = (d->N + kTile - 1) / kTile;
    if ((long long)d->M * d->N > 0x7fffffffll || (long long)mt_n * nt_n > 65535) return false;
    k.K = d->K; k.M = d->M; k.N = d->N; k.mt_n = mt_n; k.nt_n = nt_n;
    if (is_short) {
        k.cps = 0;
        return pg_split_short(k.K, mt_n * nt_n, k.spp, k.shares);
    }
    if (!pixgemm::split(k.K, k.mt_n * nt_n, k.cps, k.shares)) return false;
    k.spp = (long long)k.cps * UAVSAL_WGRAD_CHAIN;
    return true;
}

// ------------------------------------------------------------------------------------------------ channel sums
struct SumK {
    const float *gy, *y, *e, *d, *ga, *w3, *s3;
    double* ws;
    long long gi, gr, gc;
    long long rows;             // n_img * H
    int H, W, C, slab_rows, slabs;
};

__global__ __launch_bounds__(256) void dec_sums_kernel(const SumK p) {
    __shared__ double red[4 * kGroup];
    const int slab = blockIdx.x, cg = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = cg * kGroup + lane * 4;
    const long long r0 = (long long)slab * p.slab_rows;
    long long r1 = r0 + p.slab_rows;
    if (r1 > p.rows) r1 = p.rows;
    const long long q0 = r0 * p.W, q1 = r1 * p.W;              // global pixels of the slab

    const f32x4 w3 = ld4(p.w3 + c);
    const float s3 = p.s3[0];
    double acc[kNS][4];
#pragma unroll
    for (int j = 0; j < kNS; ++j)
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[j][u] = 0.0;
    double a3 = 0.0;

    for (long long q = q0 + wave; q < q1; q += 4) {
        const long long row = q / p.W;
        const int x = (int)(q - row * p.W);
        const int n = (int)(row / p.H);
        const int yy = (int)(row - (long long)n * p.H);
        const float yv = p.y[q];
        const float d3 = p.gy[n * p.gi + yy * p.gr + x * p.gc] * yv * (1.f - yv);
        const float a = d3 * s3;
        const f32x4 dv = ld4(p.d + q * p.C + c);
        const f32x4 gv = ld4(p.ga + q * p.C + c);
        f32x4 d2;
#pragma unroll
        for (int u = 0; u < 4; ++u) d2[u] = (dv[u] > 0.f && dv[u] < 6.f) ? a * w3[u] : 0.f;
        a3 += (double)d3;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc[0][u] += (double)d3 * (double)dv[u];
            acc[1][u] += (double)d2[u];
            acc[11][u] += (double)gv[u];
        }
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = yy + ky - 1;
            if (iy < 0 || iy >= p.H) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = x + kx - 1;
                if (ix < 0 || ix >= p.W) continue;
                const f32x4 ev = ld4(p.e + (q + (long long)(ky - 1) * p.W + (kx - 1)) * p.C + c);
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[2 + ky * 3 + kx][u] += (double)d2[u] * (double)ev[u];
            }
        }
    }
    // the four waves meet in wave order; ws [slab][kNS][C] doubles, then S3 of the slab behind the kNS * C
    double* o = p.ws + (long long)slab * ((long long)kNS * p.C + 1);
#pragma unroll
    for (int j = 0; j < kNS; ++j) sums::wave_meet(red, acc[j], o + (long long)j * p.C + cg * kGroup, kGroup);     // C % kGroup == 0
    if (cg == 0) {
        if (lane == 0) red[wave] = a3;
        __syncthreads();
        if (threadIdx.x == 0) o[(long long)kNS * p.C] = ((red[0] + red[1]) + red[2]) + red[3];
    }
}

bool sums_plan(const uavsal_dec_sums_desc* d, SumK& k) {
    if (!d || d->n_img <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0 || (d->C % kGroup)) return false;
    if ((long long)d->H * d->W > 0x7fffffffll || d->C / kGroup > 65535) return false;
    k.H = d->H; k.W = d->W; k.C = d->C;
    k.rows = (long long)d->n_img * d->H;
    return sums::slab_rule(k.rows, d->W, kSlabPixels, k.slab_rows, k.slabs);
}

// ------------------------------------------------------------------------------------------------ finalise
struct FinK {
    const double *ws, *rowdot;
    const float *wd, *w3, *s2, *s3, *r1, *mu1, *r2, *mu2, *r3, *mu3;
    float *g_gamma1, *g_beta1, *g_wd, *g_gamma2, *g_beta2, *g_w3, *g_gamma3, *g_beta3;
    int C, slabs, accumulate;
};

__global__ __launch_bounds__(256) void dec_finish_kernel(const FinK k) {
    __shared__ double red[256];
    const long long stride = (long long)kNS * k.C + 1;
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < k.C) {
        double s[kNS];
#pragma unroll
        for (int j = 0; j < kNS; ++j) s[j] = 0.0;
        for (int sl = 0; sl < k.slabs; ++sl) {
            const double* q = k.ws + sl * stride + c;
#pragma unroll
            for (int j = 0; j < kNS; ++j) s[j] += q[(long long)j * k.C];
        }
        const double s2 = (double)k.s2[c];
        double dotd = 0.0;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            put(k.g_wd + (long long)c * 9 + t, s2 * s[2 + t], k.accumulate);
            dotd += (double)k.wd[(long long)c * 9 + t] * s[2 + t];
        }
        put(k.g_w3 + c, (double)k.s3[0] * s[0], k.accumulate);
        put(k.g_beta2 + c, s[1], k.accumulate);
        put(k.g_gamma2 + c, (double)k.r2[c] * (dotd - (double)k.mu2[c] * s[1]), k.accumulate);
        put(k.g_beta1 + c, s[11], k.accumulate);
        put(k.g_gamma1 + c, (double)k.r1[c] * (k.rowdot[c] - (double)k.mu1[c] * s[11]), k.accumulate);
    }
    if (blockIdx.x != 0) return;
    double dot3 = 0.0;
    for (int ch = threadIdx.x; ch < k.C; ch += 256) {
        double g3 = 0.0;
        for (int sl = 0; sl < k.slabs; ++sl) g3 += k.ws[sl * stride + ch];
        dot3 += (double)k.w3[ch] * g3;
    }
    red[threadIdx.x] = dot3;
    tree256(red);
    if (threadIdx.x == 0) {
        double S3 = 0.0;
        for (int sl = 0; sl < k.slabs; ++sl) S3 += k.ws[sl * stride + (long long)kNS * k.C];
        put(k.g_beta3, S3, k.accumulate);
        put(k.g_gamma3, (double)k.r3[0] * (red[0] - (double)k.mu3[0] * S3), k.accumulate);
    }
}

}  // namespace

extern "C" int uavsal_train_decoder_sizeof_desc(int which) {
    return which == 0 ? (int)sizeof(uavsal_pix_gemm_desc) : which == 1 ? (int)sizeof(uavsal_dec_sums_desc)
         : which == 2 ? (int)sizeof(uavsal_dec_finish_desc) : -1;
}

extern "C" int uavsal_pix_gemm_shares(const uavsal_pix_gemm_desc* d) {
    PgK k;
    return pg_plan(d, k) ? k.shares : 0;
}

extern "C" int64_t uavsal_pix_gemm_workspace_bytes(const uavsal_pix_gemm_desc* d) {
    PgK k;
    if (!pg_plan(d, k)) return 0;
    return (int64_t)k.shares * k.M * k.N * (int64_t)sizeof(float);
}

extern "C" int uavsal_pix_gemm(const uavsal_pix_gemm_desc* d, uavsal_stream_t stream) {
    if (!d || !d->a || !d->b || !d->ws || !d->out) return UAVSAL_EINVAL;
    if (d->K <= 0 || d->M <= 0 || d->N <= 0) return UAVSAL_EINVAL;
    if (d->rowdot && !d->w) return UAVSAL_EINVAL;
    const bool is_short = d->tails32 && pg_short_ok(d->M, d->N);
    if (!is_short && !pg_shape_ok(d->M, d->N)) return UAVSAL_ESHAPE;
    PgK k;
    if (!pg_plan(d, k)) return UAVSAL_ESHAPE;
    if (d->ws_bytes < uavsal_pix_gemm_workspace_bytes(d)) return UAVSAL_EINVAL;
    if (d->lda < d->M || d->ldb < d->N || d->ldo < d->N || (d->rowdot && d->ldw < d->N)) return UAVSAL_EINVAL;
    if ((d->lda | d->ldb) & 3) return UAVSAL_EALIGN;
    if (!al16(d->a) || !al16(d->b) || !al16(d->ws) || !al4(d->out) || (d->row_scale && !al4(d->row_scale)) ||
        (d->rowdot && (!al8(d->rowdot) || !al4(d->w)))) return UAVSAL_EALIGN;
    k.a = d->a; k.b = d->b; k.row_scale = d->row_scale; k.w = d->w; k.rowdot = d->rowdot; k.ws = d->ws; k.out = d->out;
    k.lda = d->lda; k.ldb = d->ldb; k.ldw = d->ldw; k.ldo = d->ldo;
    k.accumulate = d->accumulate != 0;
    const dim3 grid((unsigned)(k.mt_n * k.nt_n), (unsigned)k.shares);
    if (!is_short && pg_narrow(k.M, k.N))
        hipLaunchKernelGGL(pix_gemm32_kernel, dim3((unsigned)((k.mt_n * k.nt_n + 3) / 4), (unsigned)k.shares), dim3(256), 0,
                           (hipStream_t)stream, k);
    else if (is_short || k.M % kTile) hipLaunchKernelGGL(pix_gemm_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, k);
    else hipLaunchKernelGGL(pix_gemm_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, k);
    hipLaunchKernelGGL(pix_gemm_reduce_kernel, dim3((unsigned)k.M), dim3(256), 0, (hipStream_t)stream, k);
    return uavsal_launch_status();
}

extern "C" int uavsal_dec_sums_slabs(const uavsal_dec_sums_desc* d) {
    SumK k;
    return sums_plan(d, k) ? k.slabs : 0;
}

extern "C" int uavsal_dec_sums_slab_rows(const uavsal_dec_sums_desc* d) {
    SumK k;
    return sums_plan(d, k) ? k.slab_rows : 0;
}

extern "C" int64_t uavsal_dec_sums_workspace_bytes(const uavsal_dec_sums_desc* d) {
    SumK k;
    if (!sums_plan(d, k)) return 0;
    return (int64_t)k.slabs * ((int64_t)kNS * k.C + 1) * (int64_t)sizeof(double);
}

extern "C" int uavsal_dec_sums(const uavsal_dec_sums_desc* d, uavsal_stream_t stream) {
    if (!d || !d->gy || !d->y || !d->e || !d->d || !d->ga || !d->w3 || !d->s3 || !d->ws) return UAVSAL_EINVAL;
    if (d->n_img <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0) return UAVSAL_EINVAL;
    if (d->gy_img_pitch < 0 || d->gy_row_pitch < 0 || d->gy_col_pitch < 0) return UAVSAL_EINVAL;
    if (d->C % kGroup) return UAVSAL_ESHAPE;
    SumK k;
    if (!sums_plan(d, k)) return UAVSAL_ESHAPE;
    if (d->ws_bytes < uavsal_dec_sums_workspace_bytes(d)) return UAVSAL_EINVAL;
    if (!al16(d->e) || !al16(d->d) || !al16(d->ga) || !al16(d->w3) || !al8(d->ws) || !al4(d->gy) || !al4(d->y) || !al4(d->s3))
        return UAVSAL_EALIGN;
    k.gy = d->gy; k.y = d->y; k.e = d->e; k.d = d->d; k.ga = d->ga; k.w3 = d->w3; k.s3 = d->s3; k.ws = d->ws;
    k.gi = d->gy_img_pitch; k.gr = d->gy_row_pitch; k.gc = d->gy_col_pitch;
    hipLaunchKernelGGL(dec_sums_kernel, dim3((unsigned)k.slabs, (unsigned)(k.C / kGroup)), dim3(256), 0, (hipStream_t)stream, k);
    return uavsal_launch_status();
}

extern "C" int uavsal_dec_finish(const uavsal_dec_finish_desc* d, uavsal_stream_t stream) {
    if (!d || !d->ws || !d->rowdot || !d->wd || !d->w3 || !d->s2 || !d->s3 || !d->r1 || !d->mu1 || !d->r2 || !d->mu2 ||
        !d->r3 || !d->mu3 || !d->g_gamma1 || !d->g_beta1 || !d->g_wd || !d->g_gamma2 || !d->g_beta2 || !d->g_w3 ||
        !d->g_gamma3 || !d->g_beta3) return UAVSAL_EINVAL;
    if (d->C <= 0 || d->slabs <= 0) return UAVSAL_EINVAL;
    if (d->C % kGroup) return UAVSAL_ESHAPE;
    if (d->ws_bytes < (int64_t)d->slabs * ((int64_t)kNS * d->C + 1) * (int64_t)sizeof(double)) return UAVSAL_EINVAL;
    const void* f4[] = {d->wd, d->w3, d->s2, d->s3, d->r1, d->mu1, d->r2, d->mu2, d->r3, d->mu3, d->g_gamma1, d->g_beta1,
                        d->g_wd, d->g_gamma2, d->g_beta2, d->g_w3, d->g_gamma3, d->g_beta3};
    for (const void* p : f4)
        if (!al4(p)) return UAVSAL_EALIGN;
    if (!al8(d->ws) || !al8(d->rowdot)) return UAVSAL_EALIGN;
    FinK k;
    k.ws = d->ws; k.rowdot = d->rowdot; k.wd = d->wd; k.w3 = d->w3; k.s2 = d->s2; k.s3 = d->s3;
    k.r1 = d->r1; k.mu1 = d->mu1; k.r2 = d->r2; k.mu2 = d->mu2; k.r3 = d->r3; k.mu3 = d->mu3;
    k.g_gamma1 = d->g_gamma1; k.g_beta1 = d->g_beta1; k.g_wd = d->g_wd; k.g_gamma2 = d->g_gamma2; k.g_beta2 = d->g_beta2;
    k.g_w3 = d->g_w3; k.g_gamma3 = d->g_gamma3; k.g_beta3 = d->g_beta3;
    k.C = d->C; k.slabs = d->slabs; k.accumulate = d->accumulate != 0;
    hipLaunchKernelGGL(dec_finish_kernel, dim3((unsigned)(d->C / 256)), dim3(256), 0, (hipStream_t)stream, k);
    return uavsal_launch_status();
}
