// Input letterboxing of the reference caller, on device: per frame `padding(img, shape_r, shape_c, 3)`
// (reference utils_data.py:321-343, called from preprocess_videos, :255-287) and the channel swap that follows it
// (`ims[:, :, :, [2, 1, 0]]`, :269-270).  A source-size uint8 frame is resized with cv2.resize's 8-bit INTER_LINEAR
// rule to the largest size of its aspect ratio that fits R x C, centred, and everything outside is 0.
//
// The 8-bit rule is fixed-point, unlike the float rule of post.hip.  Per axis, for output index d:
//   f = float32((d + 0.5) * (n_in / n_out) - 0.5)   (product and difference in double), s = floor(f), f -= s,
//   s < 0 -> s = 0, f = 0;  s >= n_in - 1 -> s = n_in - 1, f = 0;  second tap min(s + 1, n_in - 1);
//   11-bit weights c1 = rint(f * 2048), c0 = rint((1 - f) * 2048) (float32 products, half to even).
// Horizontal pass t = S[s] * a0 + S[s1] * a1 on the two source rows, vertical pass
//   ((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16), then (that + 2) >> 2, stored as uint8.
// NOTE: cv2 is not available where this was written and the reference holds no fixture for this step: the rule is
// pinned by known answers that follow from it (tests/letterbox_ref.py), not by outputs of cv2.
//
// One launch.  A workgroup owns kRowsPerBlock output rows of one frame.  It builds the per-column (s, a0, a1) table
// once in LDS, then per output row copies the two source rows it blends (x3 planes for a planar source) into LDS with
// 16-byte loads from the enclosing 16-byte aligned range -- the source itself may start at any byte -- and every
// thread produces four adjacent output pixels of all three planes from LDS bytes: one dword store per plane.  Rows
// and columns of the bars are written as zeros by the same launch.
#include "common.h"
#include "resize_u8.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRowsPerBlock = 4;
constexpr int kMaxLds = 160 * 1024;

struct LbK {
    const unsigned char* src; unsigned char* dst;
    long long row_pitch, plane_pitch, img_pitch;
    int h0, w0, R, C;
    int new_r, new_c, y0, x0;          // picture area inside R x C
    int planar, swap, vec;             // vec: dword stores (dst 4-byte aligned, C % 4 == 0)
    int col_bytes, seg_pitch;          // LDS: column table, then the row segments
    double sy, sx;                     // n_in / n_out per axis
};

__global__ __launch_bounds__(kThreads) void letterbox_u8_kernel(const LbK p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lb_lds[];
    int2* col = reinterpret_cast<int2*>(lb_lds);           // [4 * nquad]: x = source column (-1: bar), y = a0 | a1 << 16
    unsigned char* seg = lb_lds + p.col_bytes;
    const int img = blockIdx.y;
    const int nquad = (p.C + 3) >> 2;
    for (int x = threadIdx.x; x < 4 * nquad; x += kThreads) {
        int2 e = {-1, 0};
        const int d = x - p.x0;
        if (x < p.C && d >= 0 && d < p.new_c) {
            int s, c0, c1;
            lb_tap(d, p.sx, p.w0, s, c0, c1);
            e.x = s; e.y = c0 | (c1 << 16);
        }
        col[x] = e;
    }
    const unsigned char* simg = p.src + (long long)img * p.img_pitch;
    unsigned char* dimg = p.dst + (long long)img * 3 * p.R * p.C;
    const int nseg = p.planar ? 6 : 2;                     // segment k: source row (k & 1) of plane k >> 1
    const int len = p.planar ? p.w0 : 3 * p.w0;
    const int ps = p.planar ? 1 : 3;
    for (int r = 0; r < kRowsPerBlock; ++r) {
        const int y = blockIdx.x * kRowsPerBlock + r;
        if (y >= p.R) break;
        const int dy = y - p.y0;
        const bool bar = dy < 0 || dy >= p.new_r;          // uniform over the workgroup
        int s0 = 0, b0 = 0, b1 = 0;
        if (!bar) lb_tap(dy, p.sy, p.h0, s0, b0, b1);
        const int s1 = min(s0 + 1, p.h0 - 1);
        __syncthreads();                                   // the previous row's readers are done with the segments
        if (!bar) {
            for (int k = 0; k < nseg; ++k) {
                const unsigned char* g = simg + (long long)(k >> 1) * p.plane_pitch + (long long)((k & 1) ? s1 : s0) * p.row_pitch;
                const unsigned a = (unsigned)(reinterpret_cast<uintptr_t>(g) & 15u);
                const uint4* gb = reinterpret_cast<const uint4*>(g - a);
                const int chunks = (int)(a + len + 15) >> 4;
                uint4* l = reinterpret_cast<uint4*>(seg + k * p.seg_pitch);
                for (int i = threadIdx.x; i < chunks; i += kThreads) l[i] = gb[i];
            }
        }
        __syncthreads();                                   // segments (and, the first time, the column table) are in LDS
        for (int q = threadIdx.x; q < nquad; q += kThreads) {
            unsigned w[3] = {0u, 0u, 0u};
            if (!bar) {
                int2 e[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) e[j] = col[4 * q + j];
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) {
                    const int sc = p.swap ? 2 - pl : pl;   // source channel of output plane pl
                    const int k0 = p.planar ? 2 * sc : 0;
                    const long long goff = (long long)(p.planar ? sc : 0) * p.plane_pitch;
                    const unsigned m0 = (unsigned)(reinterpret_cast<uintptr_t>(simg + goff + (long long)s0 * p.row_pitch) & 15u);
                    const unsigned m1 = (unsigned)(reinterpret_cast<uintptr_t>(simg + goff + (long long)s1 * p.row_pitch) & 15u);
                    const unsigned char* r0 = seg + k0 * p.seg_pitch + m0 + (p.planar ? 0 : sc);
                    const unsigned char* r1 = seg + (k0 + 1) * p.seg_pitch + m1 + (p.planar ? 0 : sc);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (e[j].x < 0) continue;
                        const int xa = e[j].x * ps, xb = min(e[j].x + 1, p.w0 - 1) * ps;
                        const int a0 = e[j].y & 0xffff, a1 = e[j].y >> 16;
                        const int v = lb_mix(r0[xa], r0[xb], r1[xa], r1[xb], a0, a1, b0, b1);
                        w[pl] |= (unsigned)v << (8 * j);
                    }
                }
            }
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                unsigned char* o = dimg + ((long long)pl * p.R + y) * p.C + 4 * q;
                if (p.vec) {
                    *reinterpret_cast<unsigned*>(o) = w[pl];
                } else {
                    for (int j = 0; j < 4; ++j)
                        if (4 * q + j < p.C) o[j] = (unsigned char)(w[pl] >> (8 * j));
                }
            }
        }
    }
}

}  // namespace

extern "C" int uavsal_letterbox_u8(const uavsal_letterbox_desc* d, uavsal_stream_t stream) {
    if (!d || !d->src || !d->dst) return UAVSAL_EINVAL;
    if (d->n_img <= 0 || d->h0 <= 0 || d->w0 <= 0 || d->R <= 0 || d->C <= 0) return UAVSAL_EINVAL;
    if (d->layout != UAVSAL_LETTERBOX_HWC && d->layout != UAVSAL_LETTERBOX_CHW) return UAVSAL_EINVAL;
    const int planar = d->layout == UAVSAL_LETTERBOX_CHW;
    const long long len = planar ? (long long)d->w0 : 3ll * d->w0;
    if (d->row_pitch < len) return UAVSAL_ESHAPE;
    const long long plane_extent = (long long)(d->h0 - 1) * d->row_pitch + len;
    if (planar && d->plane_pitch < plane_extent) return UAVSAL_ESHAPE;
    const long long img_extent = planar ? 2 * d->plane_pitch + plane_extent : plane_extent;
    if (d->n_img > 1 && d->img_pitch < img_extent) return UAVSAL_ESHAPE;
    if (d->n_img > 65535) return UAVSAL_ESHAPE;
    LbK k;
    k.src = d->src; k.dst = d->dst;
    k.row_pitch = d->row_pitch; k.plane_pitch = planar ? d->plane_pitch : 0; k.img_pitch = d->img_pitch;
    k.h0 = d->h0; k.w0 = d->w0; k.R = d->R; k.C = d->C;
    if ((double)d->h0 / d->R > (double)d->w0 / d->C) {      // utils_data.py:330-335
        k.new_r = d->R; k.new_c = (int)(((long long)d->w0 * d->R) / d->h0);
        k.y0 = 0; k.x0 = (d->C - k.new_c) / 2;
    } else {                                                // utils_data.py:336-341
        k.new_c = d->C; k.new_r = (int)(((long long)d->h0 * d->C) / d->w0);
        k.x0 = 0; k.y0 = (d->R - k.new_r) / 2;
    }
    if (k.new_r <= 0 || k.new_c <= 0 || k.new_r > d->R || k.new_c > d->C) return UAVSAL_ESHAPE;
    k.sy = (double)d->h0 / k.new_r; k.sx = (double)d->w0 / k.new_c;
    k.planar = planar; k.swap = d->swap_rb != 0;
    k.vec = (d->C % 4 == 0) && ((reinterpret_cast<uintptr_t>(d->dst) & 3u) == 0);
    k.col_bytes = 8 * 4 * ((d->C + 3) / 4);                 // a multiple of 16
    const long long seg_pitch = (len + 30) / 16 * 16;       // the 16-byte chunks that enclose a row at any misalignment
    const long long lds = k.col_bytes + (planar ? 6 : 2) * seg_pitch;
    if (lds > kMaxLds) return UAVSAL_ESHAPE;
    k.seg_pitch = (int)seg_pitch;
    if (lds > 64 * 1024) UAVSAL_LDS_OPTIN(letterbox_u8_kernel, kMaxLds);
    dim3 grid((unsigned)((d->R + kRowsPerBlock - 1) / kRowsPerBlock), (unsigned)d->n_img);
    hipLaunchKernelGGL(letterbox_u8_kernel, grid, dim3(kThreads), (size_t)lds, (hipStream_t)stream, k);
    return uavsal_launch_status();
}
