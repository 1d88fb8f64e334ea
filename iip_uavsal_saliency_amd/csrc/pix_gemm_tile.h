// The 128 x 128 tile loop of the GEMMs whose reduction runs over pixels (uavsal_twa_wgrad in csrc/train.hip,
// uavsal_pix_gemm in csrc/train_decoder.hip): out[m][n] = sum over pixels p of A[p][m] B[p][n], both operands pixel-major
// with the M / N index contiguous, which is what v_mfma_f32_32x32x2_f32 reads from LDS without a transpose.
//   K step  32 pixels: 2 x 20 KB of LDS (32 rows of 128 floats padded to 160), loaded as float4 by 256 threads, the next
//           step's global loads in flight while the current one multiplies.
//   wave    2 x 2 MFMA tiles of 32 x 32 (four independent accumulators).
//   chains  after UAVSAL_WGRAD_CHAIN / 32 K steps (and at the end) the chain's tile is added to a second fp32 register tile
//           and a new chain starts: no accumulation chain is longer than UAVSAL_WGRAD_CHAIN products.
// The operand loaders are the parameter: `fa(g)` / `fb(g)` return the address of the four floats this thread loads (column
// (tid & 31) * 4 of the tile) of the A / B row of global pixel g (p0 <= g < p1), or nullptr for zeros (a whole row, or this
// thread's four columns: uavsal_pix_gemm's last M tile and last N tile may end at column 64); rows behind p1 are zeros and are
// never asked for.
#pragma once
#include "common.h"

namespace pixgemm {

constexpr int kTile = 128, kStep = 32, kRow = 160;
constexpr int kTargetWGs = 1024;

using ::ld4;

// D of the wave's MFMA tile (i, j), register r: row m = wm + i * 32 + (r & 3) + 8 (r >> 2) + 4 (lane >> 5),
// column n = wn + j * 32 + (lane & 31), with wm = (wave & 1) * 64, wn = (wave >> 1) * 64.
template <class FetchA, class FetchB>
__device__ __forceinline__ void tile_loop(long long p0, long long p1, FetchA fa, FetchB fb, f32x16 (&tot)[2][2]) {
    __shared__ __attribute__((aligned(16))) float As[kStep * kRow];
    __shared__ __attribute__((aligned(16))) float Bs[kStep * kRow];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave & 1) * 64, wn = (wave >> 1) * 64;
    const int lrow = tid >> 5, lc = (tid & 31) * 4;           // loader: row lrow + 8 i of the step, 4 floats at lc
    const int steps = (int)((p1 - p0 + kStep - 1) / kStep);

    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[i][j][r] = 0.f; tot[i][j][r] = 0.f; }

    f32x4 ra[4], rb[4];
    auto fetch = [&](int s) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long g = p0 + (long long)s * kStep + lrow + 8 * i;
            const float* pa = g < p1 ? fa(g) : nullptr;
            const float* pb = g < p1 ? fb(g) : nullptr;
            ra[i] = pa ? ld4(pa) : zero4;
            rb[i] = pb ? ld4(pb) : zero4;
        }
    };
    if (steps > 0) fetch(0);
    for (int s = 0; s < steps; ++s) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<f32x4*>(&As[(lrow + 8 * i) * kRow + lc]) = ra[i];
            *reinterpret_cast<f32x4*>(&Bs[(lrow + 8 * i) * kRow + lc]) = rb[i];
        }
        __syncthreads();
        if (s + 1 < steps) fetch(s + 1);
        const float* ap = As + (lane >> 5) * kRow + wm + (lane & 31);
        const float* bp = Bs + (lane >> 5) * kRow + wn + (lane & 31);
#pragma unroll
        for (int kk = 0; kk < kStep / 2; ++kk) {
            const float a0 = ap[kk * 2 * kRow], a1 = ap[kk * 2 * kRow + 32];
            const float b0 = bp[kk * 2 * kRow], b1 = bp[kk * 2 * kRow + 32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        if ((s + 1) % (UAVSAL_WGRAD_CHAIN / kStep) == 0 || s + 1 == steps) {      // the chain ends: at most 1024 products
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    tot[i][j] += acc[i][j];
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
                }
        }
        __syncthreads();
    }
}

// The K split: the K pixels in chunks of UAVSAL_WGRAD_CHAIN; with `tiles` output tiles and a grid of about kTargetWGs
// workgroups at most kTargetWGs / tiles workgroups share a tile; every share is the same whole number `cps` of chunks, the
// smallest with which that many shares cover all chunks.  false: the sizes do not fit.
inline bool split(long long K, int tiles, int& cps_out, int& shares_out) {
    const long long chunks = (K + UAVSAL_WGRAD_CHAIN - 1) / UAVSAL_WGRAD_CHAIN;
    long long want = kTargetWGs / tiles;
    if (want < 1) want = 1;
    if (want > chunks) want = chunks;
    const long long cps = (chunks + want - 1) / want;
    const long long shares = (chunks + cps - 1) / cps;
    if (cps > 0x7fffffffll / UAVSAL_WGRAD_CHAIN || shares > 65535) return false;
    cps_out = (int)cps; shares_out = (int)shares;
    return true;
}

}  // namespace pixgemm
