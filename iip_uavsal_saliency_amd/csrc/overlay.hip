// Heat-map overlay frames of the reference's visualisation, on device: the coloured path of `visual_vid`
// (reference utils_vis.py:103-212, with_color=1, with and without with_fix) and `heatmap_overlay` / `visual_img`
// (:34-101) as its special case without resizes.  Per frame:
//   1. the BGR uint8 frame goes to the mid size with cv2.resize's 8-bit INTER_LINEAR rule (:186; resize_u8.h, the
//      rule letterbox.hip states), the uint8 map to the same size by the same rule (:39-40; the identity at equal sizes);
//   2. map_color = LUT[map] (:46), img / (max(img) + EPS), m = map / (max(map) + EPS), map_color / max(map_color)
//      (:51-53; the maxima are per frame, the last one an integer maximum without EPS),
//      o = 0.8 * (1 - m ** 0.8) * img + m * map_color (:55), everything in double, EPS = 2.2204e-16;
//   3. o goes to the output size with cv2.resize's INTER_LINEAR rule for a 3-channel float64 image (:190):
//      f = float32((d + 0.5) * (n_in / n_out) - 0.5) (double, then cast), s = floor(f), f -= s, clamped to the edge
//      samples as in priors.resize_linear, weights 1 - f and f in float32, products and sums in double, the horizontal
//      pass first, then the vertical one;
//   4. every nonzero pixel (r, c) of the frame's fixation map is scattered to (rint(r * (out_h / H)), rint(c * (out_w / W)))
//      (resize_fixation, :16-31: quotient first, half to even, an index equal to the extent pulled back by one), dilated
//      with a 5x5 box (:204) and the overlay set to 1 under it (:206);
//   5. o / max(o) * 255, clipped to [0, 255], rint, uint8 (:208-209, im2uint8 :7-14).
// One deviation: where the reference's frame is undefined -- max(o) == 0 (black frame and empty map: 0 / 0), or
// max(map_color) == 0 (a colour table that is 0 wherever the map points: 0 / 0) -- the frame is written as zeros.
// NOTE: cv2 is not available where this was written; the two resize rules are restated (tests/letterbox_ref.py,
// tests/overlay_ref.py) and pinned by known answers that follow from them, not by outputs of cv2.
//
// Launches of one call, all on the caller's stream:
//   overlay_clear_kernel   zeroes the per-frame maxima and the fixation mask (the call clears its own workspace);
//   overlay_mid_kernel     step 1 into the workspace (mid frame, interleaved BGR, and mid map, rows padded to 16 pixels)
//                          and the three integer maxima of step 2 (atomicMax on ints);
//   overlay_stamp_kernel   step 4's scatter: constant bytes, plain vector stores, 5x5 blocks clipped at the border;
//   overlay_out_kernel<0>  steps 2-4 at the output size, maximum only: max(o) as the maximum of the bit patterns of
//                          non-negative doubles (atomicMax on 64-bit integers);
//   overlay_out_kernel<1>  the same arithmetic again, then step 5 and the stores.
// The double overlay is never stored (22 MB per 1280x720 frame): it is recomputed in the quantising pass.  Everything that
// depends only on a byte and the frame's maxima is a table in LDS: 0.8 * (1 - m ** 0.8) and the three m * colour / cmax
// terms per map byte (four doubles per entry, 8 KB, `pow` 256 times per workgroup instead of once per pixel) and
// v / (imax + EPS) per frame byte (2 KB).  A workgroup owns kOutRows output rows of one frame; it blends a mid row once,
// as doubles into one of two LDS slots (the row pair of the vertical pass; consecutive output rows reuse them), and a
// thread interpolates four adjacent pixels from the slots: three dword stores.  No float atomics: two runs are bitwise equal.
#include "common.h"
#include "resize_u8.h"

#pragma clang fp contract(off)      // numpy does not fuse: products and sums round one by one

namespace {

constexpr int kThreads = 256;
constexpr int kMidRows = 4;
constexpr int kOutRows = 8;
constexpr int kMaxLds = 160 * 1024;
constexpr int kStatInts = 8;             // per frame: imax, mmax, cmax, -, omax (64 bit), -
constexpr double kEps = 2.2204e-16;      // utils_vis.py:5

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

__global__ __launch_bounds__(kThreads) void overlay_clear_kernel(uint4* p, long long n16) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i < n16) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

struct OvMidK {
    const unsigned char* src; const unsigned char* map; const unsigned char* lut;
    unsigned char* midf; unsigned char* midm; int* stats;
    long long row_pitch, plane_pitch, img_pitch, map_img_pitch;
    int h0, w0, planar, map_h, map_w, mid_h, mid_w, mwp;
    int segf_pitch, segm_pitch;
    double sy, sx, msy, msx;
};

// copy `len` bytes at g (any address) into LDS as the 16-byte chunks that enclose them
__device__ __forceinline__ void stage_row(unsigned char* l, const unsigned char* g, int len) {
    const unsigned a = (unsigned)(reinterpret_cast<uintptr_t>(g) & 15u);
    const uint4* gb = reinterpret_cast<const uint4*>(g - a);
    const int chunks = (int)(a + len + 15) >> 4;
    uint4* l4 = reinterpret_cast<uint4*>(l);
    for (int i = threadIdx.x; i < chunks; i += kThreads) l4[i] = gb[i];
}

__global__ __launch_bounds__(kThreads) void overlay_mid_kernel(const OvMidK p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ov_lds[];
    int2* colf = reinterpret_cast<int2*>(ov_lds);                 // [mwp]: x = source column (-1: padding), y = a0 | a1 << 16
    int2* colm = colf + p.mwp;
    unsigned char* lmax = reinterpret_cast<unsigned char*>(colm + p.mwp);      // [256] max over the channels of a table row
    unsigned char* segf = lmax + 256;
    const int nsegf = p.planar ? 6 : 2;                            // segment k: source row (k & 1) of plane k >> 1
    unsigned char* segm = segf + nsegf * p.segf_pitch;
    const int img = blockIdx.y;
    for (int x = threadIdx.x; x < p.mwp; x += kThreads) {
        int2 ef = {-1, 0}, em = {-1, 0};
        if (x < p.mid_w) {
            int s, c0, c1;
            lb_tap(x, p.sx, p.w0, s, c0, c1);
            ef.x = s; ef.y = c0 | (c1 << 16);
            lb_tap(x, p.msx, p.map_w, s, c0, c1);
            em.x = s; em.y = c0 | (c1 << 16);
        }
        colf[x] = ef; colm[x] = em;
    }
    {
        const unsigned char* e = p.lut + 3 * threadIdx.x;      // kThreads == 256 table entries
        lmax[threadIdx.x] = max(e[0], max(e[1], e[2]));
    }
    const unsigned char* simg = p.src + (long long)img * p.img_pitch;
    const unsigned char* mimg = p.map + (long long)img * p.map_img_pitch;
    const int len = p.planar ? p.w0 : 3 * p.w0;
    const int ps = p.planar ? 1 : 3;
    const int nquad = p.mwp >> 2;
    int imx = 0, mmx = 0, cmx = 0;
    for (int r = 0; r < kMidRows; ++r) {
        const int y = blockIdx.x * kMidRows + r;
        if (y >= p.mid_h) break;
        int s0, b0, b1, ms0, mb0, mb1;
        lb_tap(y, p.sy, p.h0, s0, b0, b1);
        lb_tap(y, p.msy, p.map_h, ms0, mb0, mb1);
        const int s1 = min(s0 + 1, p.h0 - 1), ms1 = min(ms0 + 1, p.map_h - 1);
        __syncthreads();                                   // the previous row's readers are done with the segments
        for (int k = 0; k < nsegf; ++k)
            stage_row(segf + k * p.segf_pitch, simg + (long long)(k >> 1) * p.plane_pitch + (long long)((k & 1) ? s1 : s0) * p.row_pitch, len);
        stage_row(segm, mimg + (long long)ms0 * p.map_w, p.map_w);
        stage_row(segm + p.segm_pitch, mimg + (long long)ms1 * p.map_w, p.map_w);
        __syncthreads();                                   // segments (and, the first time, the tables) are in LDS
        const unsigned char* m0 = segm + (unsigned)(reinterpret_cast<uintptr_t>(mimg + (long long)ms0 * p.map_w) & 15u);
        const unsigned char* m1 = segm + p.segm_pitch + (unsigned)(reinterpret_cast<uintptr_t>(mimg + (long long)ms1 * p.map_w) & 15u);
        const unsigned char* f0[3];
        const unsigned char* f1[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const long long goff = (long long)(p.planar ? c : 0) * p.plane_pitch;
            const int k0 = p.planar ? 2 * c : 0;
            f0[c] = segf + k0 * p.segf_pitch + (unsigned)(reinterpret_cast<uintptr_t>(simg + goff + (long long)s0 * p.row_pitch) & 15u) + (p.planar ? 0 : c);
            f1[c] = segf + (k0 + 1) * p.segf_pitch + (unsigned)(reinterpret_cast<uintptr_t>(simg + goff + (long long)s1 * p.row_pitch) & 15u) + (p.planar ? 0 : c);
        }
        unsigned* of = reinterpret_cast<unsigned*>(p.midf + ((long long)img * p.mid_h + y) * 3 * p.mwp);
        unsigned* om = reinterpret_cast<unsigned*>(p.midm + ((long long)img * p.mid_h + y) * p.mwp);
        for (int q = threadIdx.x; q < nquad; q += kThreads) {
            unsigned w[3] = {0u, 0u, 0u}, wm = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int2 ef = colf[4 * q + j], em = colm[4 * q + j];
                if (ef.x < 0) continue;
                const int xa = ef.x * ps, xb = min(ef.x + 1, p.w0 - 1) * ps;
                const int a0 = ef.y & 0xffff, a1 = ef.y >> 16;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int v = lb_mix(f0[c][xa], f0[c][xb], f1[c][xa], f1[c][xb], a0, a1, b0, b1);
                    imx = max(imx, v);
                    w[(3 * j + c) >> 2] |= (unsigned)v << (8 * ((3 * j + c) & 3));
                }
                const int ma = em.x, mb = min(em.x + 1, p.map_w - 1);
                const int mv = lb_mix(m0[ma], m0[mb], m1[ma], m1[mb], em.y & 0xffff, em.y >> 16, mb0, mb1);
                mmx = max(mmx, mv);
                cmx = max(cmx, (int)lmax[mv]);
                wm |= (unsigned)mv << (8 * j);
            }
            of[3 * q] = w[0]; of[3 * q + 1] = w[1]; of[3 * q + 2] = w[2];
            om[q] = wm;
        }
    }
    imx = wave_max(imx); mmx = wave_max(mmx); cmx = wave_max(cmx);
    if ((threadIdx.x & 63) == 0) {
        int* st = p.stats + (long long)img * kStatInts;
        atomicMax(st, imx); atomicMax(st + 1, mmx); atomicMax(st + 2, cmx);
    }
}

struct OvStampK {
    const unsigned char* fix; unsigned char* mask;
    long long n;                              // F * fix_h * fix_w
    int fix_h, fix_w, out_h, out_w;
    double fr, fc;                            // out_h / fix_h, out_w / fix_w (resize_fixation, utils_vis.py:18-19)
};

__global__ __launch_bounds__(kThreads) void overlay_stamp_kernel(const OvStampK p) {
    const unsigned a = (unsigned)(reinterpret_cast<uintptr_t>(p.fix) & 15u);
    const long long chunk = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (chunk * 16 >= (long long)a + p.n) return;
    const uint4 v = reinterpret_cast<const uint4*>(p.fix - a)[chunk];
    if ((v.x | v.y | v.z | v.w) == 0u) return;
    const unsigned wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int b = 0; b < 16; ++b) {
        if (((wv[b >> 2] >> (8 * (b & 3))) & 0xffu) == 0u) continue;
        const long long i = chunk * 16 + b - a;            // index into [F][fix_h][fix_w]
        if (i < 0 || i >= p.n) continue;
        const long long plane = (long long)p.fix_h * p.fix_w;
        const int f = (int)(i / plane);
        const int rem = (int)(i - (long long)f * plane);
        const int r = rem / p.fix_w, c = rem - r * p.fix_w;
        int rr = (int)rint((double)r * p.fr), cc = (int)rint((double)c * p.fc);      // utils_vis.py:23-24, np.round: half to even
        if (rr == p.out_h) --rr;                           // :25-28
        if (cc == p.out_w) --cc;
        if (rr < 0 || rr >= p.out_h || cc < 0 || cc >= p.out_w) continue;
        unsigned char* m = p.mask + (long long)f * p.out_h * p.out_w;
        for (int y = max(rr - 2, 0); y <= min(rr + 2, p.out_h - 1); ++y)
            for (int x = max(cc - 2, 0); x <= min(cc + 2, p.out_w - 1); ++x) m[(long long)y * p.out_w + x] = 1;
    }
}

struct OvOutK {
    const unsigned char* midf; const unsigned char* midm; const unsigned char* mask; const unsigned char* lut;
    int* stats; unsigned char* out;
    int mid_h, mid_w, mwp, out_h, out_w, vec, col_bytes;
    double sy, sx;                            // mid / out per axis
};

// first tap and the float32 weight of the second one, for output index d of the float resize
__device__ __forceinline__ void lin_tap(int d, double scale, int n_in, int& s, float& f) {
    f = (float)(((double)d + 0.5) * scale - 0.5);
    s = (int)floorf(f);
    f = f - (float)s;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= n_in - 1) { s = n_in - 1; f = 0.f; }
}

template <int QUANT>
__global__ __launch_bounds__(kThreads) void overlay_out_kernel(const OvOutK p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ov_lds[];
    double* tab = reinterpret_cast<double*>(ov_lds);               // [256][4]: 0.8 * (1 - m ** 0.8), m * colour[c] / cmax
    double* imgn = tab + 1024;                                     // [256]: v / (imax + EPS)
    int2* col = reinterpret_cast<int2*>(imgn + 256);               // [4 * nquad]: x = first tap, y = bits of the float32 weight
    double* slot = reinterpret_cast<double*>(ov_lds + 10240 + p.col_bytes);      // [2][3 * mwp]: the blended mid row r in slot r & 1
    const int img = blockIdx.y;
    const int* st = p.stats + (long long)img * kStatInts;
    const int imax = st[0], mmax = st[1], cmax = st[2];
    unsigned long long* omax_p = reinterpret_cast<unsigned long long*>(p.stats + (long long)img * kStatInts + 4);
    double omax = 0.0;
    if (QUANT) omax = __longlong_as_double((long long)*omax_p);
    const bool undefined = cmax == 0 || (QUANT && omax == 0.0);    // uniform over the workgroup
    if (!QUANT && undefined) return;
    const int nquad = (p.out_w + 3) >> 2;
    {
        const int t = threadIdx.x;                                 // kThreads == 256 table entries
        const double m = (double)t / ((double)mmax + kEps);        // utils_vis.py:52
        tab[4 * t] = 0.8 * (1.0 - pow(m, 0.8));                    // :55
#pragma unroll
        for (int c = 0; c < 3; ++c) tab[4 * t + 1 + c] = m * ((double)p.lut[3 * t + c] / (double)cmax);      // :53, :55
        imgn[t] = (double)t / ((double)imax + kEps);               // :51
    }
    for (int x = threadIdx.x; x < 4 * nquad; x += kThreads) {
        int s = 0; float f = 0.f;
        if (x < p.out_w) lin_tap(x, p.sx, p.mid_w, s, f);
        col[x] = make_int2(s, __float_as_int(f));
    }
    const int frow = 3 * p.mwp;
    const unsigned char* fimg = p.midf + (long long)img * p.mid_h * frow;
    const unsigned char* mimg = p.midm + (long long)img * p.mid_h * p.mwp;
    int have[2] = {-1, -1};                                    // the mid row each slot holds (uniform over the workgroup)
    double mx = 0.0;
    for (int r = 0; r < kOutRows; ++r) {
        const int y = blockIdx.x * kOutRows + r;
        if (y >= p.out_h) break;
        int s0; float fy;
        lin_tap(y, p.sy, p.mid_h, s0, fy);
        const int s1 = min(s0 + 1, p.mid_h - 1);
        const double wy0 = (double)(1.f - fy), wy1 = (double)fy;
        __syncthreads();                                   // the previous row's readers are done; the first time: the tables are in LDS
        if (!undefined) {
            // o = 0.8 * (1 - m ** 0.8) * img + m * map_color (utils_vis.py:55) of a whole mid row, once per row: consecutive
            // output rows share their mid rows, and s0, s1 = s0 + 1 differ in parity
            for (int k = 0; k < 2; ++k) {
                const int row = k ? s1 : s0;
                if (have[row & 1] == row) continue;
                have[row & 1] = row;
                double* dst = slot + (row & 1) * frow;
                const unsigned* gm = reinterpret_cast<const unsigned*>(mimg + (long long)row * p.mwp);
                const unsigned* gf = reinterpret_cast<const unsigned*>(fimg + (long long)row * frow);
                for (int q = threadIdx.x; q < (p.mwp >> 2); q += kThreads) {
                    const unsigned mw = gm[q];
                    const unsigned fw[3] = {gf[3 * q], gf[3 * q + 1], gf[3 * q + 2]};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const double* t = tab + 4 * ((mw >> (8 * j)) & 0xffu);
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const unsigned fv = (fw[(3 * j + c) >> 2] >> (8 * ((3 * j + c) & 3))) & 0xffu;
                            dst[3 * (4 * q + j) + c] = t[0] * imgn[fv] + t[1 + c];
                        }
                    }
                }
            }
        }
        __syncthreads();                                   // both blended rows are in LDS
        const double* A0 = slot + (s0 & 1) * frow;
        const double* A1 = slot + (s1 & 1) * frow;
        const unsigned char* mrow = p.mask ? p.mask + ((long long)img * p.out_h + y) * p.out_w : nullptr;
        unsigned char* orow = p.out + ((long long)img * p.out_h + y) * 3 * p.out_w;
        for (int q = threadIdx.x; q < nquad; q += kThreads) {
            unsigned w[3] = {0u, 0u, 0u};
            if (!undefined) {
                unsigned fixed = 0u;
                if (mrow) {
                    if (p.vec) fixed = *reinterpret_cast<const unsigned*>(mrow + 4 * q);
                    else
                        for (int j = 0; j < 4; ++j)
                            if (4 * q + j < p.out_w) fixed |= (unsigned)mrow[4 * q + j] << (8 * j);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (4 * q + j >= p.out_w) continue;
                    const int2 e = col[4 * q + j];
                    const int x0 = e.x, x1 = min(e.x + 1, p.mid_w - 1);
                    const float fx = __int_as_float(e.y);
                    const double wx0 = (double)(1.f - fx), wx1 = (double)fx;
                    const bool fix = ((fixed >> (8 * j)) & 0xffu) != 0u;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const double h0 = A0[3 * x0 + c] * wx0 + A0[3 * x1 + c] * wx1;
                        const double h1 = A1[3 * x0 + c] * wx0 + A1[3 * x1 + c] * wx1;
                        double o = h0 * wy0 + h1 * wy1;
                        if (fix) o = 1.0;                                       // utils_vis.py:206
                        if (QUANT) {
                            double v = o / omax * 255.0;                        // :208
                            v = fmin(fmax(v, 0.0), 255.0);                      // :11-12
                            w[(3 * j + c) >> 2] |= (unsigned)(int)rint(v) << (8 * ((3 * j + c) & 3));
                        } else {
                            mx = fmax(mx, o);
                        }
                    }
                }
            }
            if (QUANT) {
                if (p.vec) {
                    unsigned* o4 = reinterpret_cast<unsigned*>(orow + 12 * q);
                    o4[0] = w[0]; o4[1] = w[1]; o4[2] = w[2];
                } else {
                    for (int k = 0; k < 12; ++k)
                        if (4 * q + k / 3 < p.out_w) orow[12 * q + k] = (unsigned char)(w[k >> 2] >> (8 * (k & 3)));
                }
            }
        }
    }
    if (!QUANT) {
        // o >= 0 everywhere: the order of non-negative doubles is the order of their bit patterns
        unsigned long long b = (unsigned long long)__double_as_longlong(mx);
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            const unsigned long long other = (unsigned long long)__shfl_xor((long long)b, o);
            b = other > b ? other : b;
        }
        if ((threadIdx.x & 63) == 0) atomicMax(omax_p, b);
    }
}

inline long long up(long long v, long long a) { return (v + a - 1) / a * a; }

struct OvLayout {
    int mwp;
    long long clear_bytes, mask_off, midf_off, midm_off, total;
};

// workspace: [per-frame maxima | fixation mask] (cleared by the call), mid frames, mid maps; every part 256-byte aligned
OvLayout ov_layout(const uavsal_overlay_desc* d) {
    OvLayout l;
    l.mwp = (int)up(d->mid_w, 16);
    l.mask_off = up((long long)d->n_img * kStatInts * 4, 256);
    const long long mask = d->fix ? (long long)d->n_img * d->out_h * d->out_w : 0;
    l.clear_bytes = up(l.mask_off + mask, 256);
    l.midf_off = l.clear_bytes;
    l.midm_off = l.midf_off + up((long long)d->n_img * d->mid_h * 3 * l.mwp, 256);
    l.total = l.midm_off + up((long long)d->n_img * d->mid_h * l.mwp, 256);
    return l;
}

int ov_check(const uavsal_overlay_desc* d) {
    if (!d) return UAVSAL_EINVAL;
    if (d->n_img <= 0 || d->h0 <= 0 || d->w0 <= 0 || d->map_h <= 0 || d->map_w <= 0) return UAVSAL_EINVAL;
    if (d->mid_h <= 0 || d->mid_w <= 0 || d->out_h <= 0 || d->out_w <= 0) return UAVSAL_EINVAL;
    if (d->layout != UAVSAL_LETTERBOX_HWC && d->layout != UAVSAL_LETTERBOX_CHW) return UAVSAL_EINVAL;
    if (d->fix && (d->fix_h <= 0 || d->fix_w <= 0)) return UAVSAL_EINVAL;
    if (d->n_img > 65535) return UAVSAL_ESHAPE;
    return 0;
}

}  // namespace

extern "C" int64_t uavsal_overlay_workspace_bytes(const uavsal_overlay_desc* d) {
    const int e = ov_check(d);
    if (e) return e;
    return ov_layout(d).total;
}

extern "C" int uavsal_overlay_u8(const uavsal_overlay_desc* d, uavsal_stream_t stream) {
    int e = ov_check(d);
    if (e) return e;
    if (!d->frames || !d->map || !d->lut || !d->out || !d->ws) return UAVSAL_EINVAL;
    const int planar = d->layout == UAVSAL_LETTERBOX_CHW;
    const long long len = planar ? (long long)d->w0 : 3ll * d->w0;
    if (d->row_pitch < len) return UAVSAL_ESHAPE;
    const long long plane_extent = (long long)(d->h0 - 1) * d->row_pitch + len;
    if (planar && d->plane_pitch < plane_extent) return UAVSAL_ESHAPE;
    const long long img_extent = planar ? 2 * d->plane_pitch + plane_extent : plane_extent;
    if (d->n_img > 1 && d->img_pitch < img_extent) return UAVSAL_ESHAPE;
    if (d->n_img > 1 && d->map_img_pitch < (long long)d->map_h * d->map_w) return UAVSAL_ESHAPE;
    const OvLayout l = ov_layout(d);
    if (d->ws_bytes < l.total) return UAVSAL_EINVAL;
    if (reinterpret_cast<uintptr_t>(d->ws) & 255u) return UAVSAL_EALIGN;
    unsigned char* ws = static_cast<unsigned char*>(d->ws);
    hipStream_t s = (hipStream_t)stream;

    OvMidK m;
    m.src = d->frames; m.map = d->map; m.lut = d->lut;
    m.midf = ws + l.midf_off; m.midm = ws + l.midm_off; m.stats = reinterpret_cast<int*>(ws);
    m.row_pitch = d->row_pitch; m.plane_pitch = planar ? d->plane_pitch : 0; m.img_pitch = d->img_pitch;
    m.map_img_pitch = d->map_img_pitch;
    m.h0 = d->h0; m.w0 = d->w0; m.planar = planar; m.map_h = d->map_h; m.map_w = d->map_w;
    m.mid_h = d->mid_h; m.mid_w = d->mid_w; m.mwp = l.mwp;
    m.sy = (double)d->h0 / d->mid_h; m.sx = (double)d->w0 / d->mid_w;
    m.msy = (double)d->map_h / d->mid_h; m.msx = (double)d->map_w / d->mid_w;
    const long long segf = (len + 30) / 16 * 16, segm = ((long long)d->map_w + 30) / 16 * 16;      // enclosing 16-byte chunks
    const long long lds_mid = 2ll * 8 * l.mwp + 256 + (planar ? 6 : 2) * segf + 2 * segm;
    if (lds_mid > kMaxLds) return UAVSAL_ESHAPE;
    m.segf_pitch = (int)segf; m.segm_pitch = (int)segm;

    OvOutK o;
    o.midf = m.midf; o.midm = m.midm; o.mask = d->fix ? ws + l.mask_off : nullptr; o.lut = d->lut;
    o.stats = m.stats; o.out = d->out;
    o.mid_h = d->mid_h; o.mid_w = d->mid_w; o.mwp = l.mwp; o.out_h = d->out_h; o.out_w = d->out_w;
    o.vec = (d->out_w % 4 == 0) && ((reinterpret_cast<uintptr_t>(d->out) & 3u) == 0);
    o.col_bytes = 8 * 4 * ((d->out_w + 3) / 4);
    o.sy = (double)d->mid_h / d->out_h; o.sx = (double)d->mid_w / d->out_w;
    const long long lds_out = 10240ll + o.col_bytes + 48ll * l.mwp;      // tables, columns, two blended rows of 3 * mwp doubles
    if (lds_out > kMaxLds) return UAVSAL_ESHAPE;

    if (lds_mid > 64 * 1024) UAVSAL_LDS_OPTIN(overlay_mid_kernel, kMaxLds);      // every opt-in before the first launch:
    if (lds_out > 64 * 1024) {                                                   // a failure leaves nothing half launched
        UAVSAL_LDS_OPTIN(overlay_out_kernel<0>, kMaxLds);
        UAVSAL_LDS_OPTIN(overlay_out_kernel<1>, kMaxLds);
    }
    const long long n16 = l.clear_bytes / 16;
    hipLaunchKernelGGL(overlay_clear_kernel, dim3((unsigned)((n16 + kThreads - 1) / kThreads)), dim3(kThreads), 0, s,
                       reinterpret_cast<uint4*>(ws), n16);
    hipLaunchKernelGGL(overlay_mid_kernel, dim3((unsigned)((d->mid_h + kMidRows - 1) / kMidRows), (unsigned)d->n_img),
                       dim3(kThreads), (size_t)lds_mid, s, m);
    if (d->fix) {
        OvStampK k;
        k.fix = d->fix; k.mask = ws + l.mask_off;
        k.n = (long long)d->n_img * d->fix_h * d->fix_w;
        k.fix_h = d->fix_h; k.fix_w = d->fix_w; k.out_h = d->out_h; k.out_w = d->out_w;
        k.fr = (double)d->out_h / d->fix_h; k.fc = (double)d->out_w / d->fix_w;
        const long long chunks = (k.n + 15 + 15) / 16;
        hipLaunchKernelGGL(overlay_stamp_kernel, dim3((unsigned)((chunks + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, k);
    }
    const dim3 grid((unsigned)((d->out_h + kOutRows - 1) / kOutRows), (unsigned)d->n_img);
    hipLaunchKernelGGL(overlay_out_kernel<0>, grid, dim3(kThreads), (size_t)lds_out, s, o);
    hipLaunchKernelGGL(overlay_out_kernel<1>, grid, dim3(kThreads), (size_t)lds_out, s, o);
    return uavsal_launch_status();
}
