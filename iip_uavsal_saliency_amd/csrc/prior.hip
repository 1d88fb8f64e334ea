// The observed prior of a dataset, the part of it that touches every byte of every video (utils_data.py:497-520, 569-574):
//     priormap   = np.mean(fixMap[:, :, 0, :num], axis=2)                                         float64
//     n_priormap = 255 * (priormap - priormap.min()) / (priormap.max() - priormap.min() + EPS)
//     cv2.imwrite(png, n_priormap);  maps[:, :, i] = padding(cv2.imread(png, 0), shape_r, shape_c, 1)
//
// 1. uavsal_prior_accumulate: acc[pixel] += sum over the frames of a chunk, int32 sums of uint8 values.  Integer sums are
//    exact in any order, and np.mean's float64 sum of them is too (they stay far below 2^53), so mean = sum / n is one
//    IEEE division and everything in front of it is integer work.
//    Flat kernel (a plane contiguous in memory, frames a multiple of 16 bytes apart, acc in the plane's pixel order): the
//    plane is a flat run of bytes whichever pixel axis is the fast one.  A lane owns 16 aligned bytes of it, loads them
//    from every frame of its slab (eight frames in flight) and keeps the sixteen int32 sums in registers; up to 15 bytes in
//    front of the first aligned address and behind the last one are summed a byte at a time by lanes of block 0.
//    Strided kernel (everything else: frame-fastest buffers, rows longer than the picture, odd frame pitches): a lane per
//    pixel, byte loads, the pixel axis of the smaller pitch across the lanes.  Correct for any pitches; not the fast path.
//
//    Slabs.  A 720 x 1280 plane has 57,600 such lanes, 900 waves: under four per CU.  So the frames are split into slabs
//    along grid.y and the slabs meet in global INTEGER atomic adds (no float atomics: the result does not depend on the
//    order of arrival, two runs give the same bytes).  Sizing, done before the kernel was written: a slab of S frames reads
//    S bytes per pixel and adds 4 atomic bytes per pixel.  The only measured atomic rate on this chip is the float one,
//    about 1.3 TB/s of added bytes against about 6 TB/s of streamed reads; the integer rate has not been measured by this
//    project and is assumed no better.  At that ratio the atomics of a slab cost as much as 4 * 6 / 1.3 = 18 frames of
//    reading: 15 % on top of S = 120, 6 % on top of S = 300, 58 % on top of S = 32.  A grid that keeps the chip reading comes
//    first, and how many waves that takes was measured (720 x 1280 x 600 resident frames, median of 40 runs, eight 16-byte
//    loads in flight per lane; profiles/ob_priors.md): 10 slabs of 60 frames 4593 GB/s, 5 x 120 4701, 3 x 200 4967, 2 x 300
//    5188 -- with 128 bytes in flight per lane, seven waves per CU already keep the memory system busy and every further
//    slab only adds atomics.  So the slab count is what brings the grid to kTargetWaves = 1024 waves (four per CU of 256),
//    S = F / ceil(1024 / waves per slab), and no slab is shorter than UAVSAL_PRIOR_MIN_SLAB = 32 frames, where the atomics
//    would begin to dominate.  720 x 1280 x 600 frames: 2 slabs of 300, 1800 waves.  360 x 640: 5 slabs of 120.  1080 x 1920
//    and larger: one slab for any F, and the atomics are a plain accumulate into the caller's sums.
//    The atomics are shaped for the memory side: the block's 4096 sums go through LDS so that one wave-instruction adds 256
//    contiguous bytes (a lane's own sixteen sums are 64 bytes apart), and a zero sum -- most of a fixation map -- is not sent.
//
// 2. uavsal_prior_finish: the integer min / max of the sums (wave shuffles, then integer atomics on two words), then per
//    output pixel of padding()'s picture area the four taps of resize_u8.h, each quantised in place:
//        m = s / n,   q = rint(255 * (m - min m) / (max m - min m + EPS))
//    in double with explicitly rounded operations so that nothing is contracted; min m = min s / n because a correctly
//    rounded division by a positive n is monotonic.  rint (half to even) is what cv2.imwrite does to a float64 picture
//    (convertTo(CV_8U) = saturate_cast); q never leaves 0..255.  The bars are written as zeros by the same launch, and the
//    source-size picture (the PNG) by further blocks of it when asked for.
#include "common.h"
#include "resize_u8.h"

namespace {

constexpr double kEps = 2.2204e-16;                        // utils_data.py:7
constexpr int kThreads = 256;
constexpr int kTargetWaves = 1024;                         // four waves on each of 256 CUs (measured: the header)
constexpr int kInFlight = 8;                               // frames a lane has in flight
constexpr long long kMaxFrames = 0x7fffffffll / 255;       // 255 * n < 2^31

struct AccK {
    const unsigned char* src; long long row, col, img;
    int* acc; long long arow, acol;
    int F, S, h0, w0;
    int head, tail;                    // flat: bytes of the plane in front of / behind the 16-byte lanes
    long long nvec;                    // flat: 16-byte lanes per plane
    int inner_w;                       // strided: columns across the lanes (else rows)
};

__device__ __forceinline__ void add16(int (&s)[16], const u32x4 v) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const unsigned w = v[q];
        s[4 * q] += (int)(w & 255u); s[4 * q + 1] += (int)((w >> 8) & 255u);
        s[4 * q + 2] += (int)((w >> 16) & 255u); s[4 * q + 3] += (int)(w >> 24);
    }
}

__global__ __launch_bounds__(kThreads) void prior_acc_flat_kernel(const AccK k) {
    __shared__ int lds[kThreads * 16];
    const int f0 = blockIdx.y * k.S, f1 = min(f0 + k.S, k.F);
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    int s[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) s[j] = 0;
    if (i < k.nvec) {
        const unsigned char* p = k.src + (long long)f0 * k.img + k.head + 16 * i;
        int f = f0;
        for (; f + kInFlight <= f1; f += kInFlight) {
            u32x4 v[kInFlight];
#pragma unroll
            for (int u = 0; u < kInFlight; ++u) v[u] = *reinterpret_cast<const u32x4*>(p + u * k.img);
#pragma unroll
            for (int u = 0; u < kInFlight; ++u) add16(s, v[u]);
            p += kInFlight * k.img;
        }
        for (; f < f1; ++f, p += k.img) add16(s, *reinterpret_cast<const u32x4*>(p));
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) lds[threadIdx.x * 16 + j] = s[j];
    __syncthreads();
    const long long base = (long long)blockIdx.x * (kThreads * 16), lim = k.nvec * 16;
    int* a = k.acc + k.head + base;
#pragma unroll
    for (int j = 0; j < 16; ++j) {                         // a wave adds 256 contiguous bytes per instruction
        const int idx = j * kThreads + threadIdx.x;
        const int v = lds[idx];
        if (v != 0 && base + idx < lim) atomicAdd(a + idx, v);
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < k.head + k.tail) {         // the unaligned ends of the plane
        const long long b = (int)threadIdx.x < k.head ? threadIdx.x : k.head + 16 * k.nvec + ((int)threadIdx.x - k.head);
        const unsigned char* p = k.src + (long long)f0 * k.img + b;
        int t = 0;
        for (int f = f0; f < f1; ++f, p += k.img) t += *p;
        if (t != 0) atomicAdd(k.acc + b, t);
    }
}

__global__ __launch_bounds__(kThreads) void prior_acc_strided_kernel(const AccK k) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (long long)k.h0 * k.w0) return;
    const int f0 = blockIdx.y * k.S, f1 = min(f0 + k.S, k.F);
    long long r, c;
    if (k.inner_w) { r = i / k.w0; c = i - r * k.w0; } else { c = i / k.h0; r = i - c * k.h0; }
    const unsigned char* p = k.src + (long long)f0 * k.img + r * k.row + c * k.col;
    int t = 0;
    for (int f = f0; f < f1; ++f, p += k.img) t += *p;
    if (t != 0) atomicAdd(k.acc + r * k.arow + c * k.acol, t);
}

int slab_frames(long long pixels, int F) {
    const long long lanes = pixels / 16 > 0 ? pixels / 16 : 1;
    const long long waves = (lanes + 63) / 64;                            // of one slab
    const long long slabs = (kTargetWaves + waves - 1) / waves;           // wanted
    long long S = (F + slabs - 1) / slabs;
    if (S < UAVSAL_PRIOR_MIN_SLAB) S = UAVSAL_PRIOR_MIN_SLAB;
    if ((F + S - 1) / S > 65535) S = ((long long)F + 65534) / 65535;      // grid.y
    return (int)S;
}

// a dimension of one element has no pitch to speak of
bool row_major(int h0, int w0, long long row, long long col) { return (w0 == 1 || col == 1) && (h0 == 1 || row == w0); }
bool col_major(int h0, int w0, long long row, long long col) { return (h0 == 1 || row == 1) && (w0 == 1 || col == h0); }

// ------------------------------------------------------------------------------------------------ finish

struct FinK {
    const int* acc; long long arow, acol;
    int* ws; unsigned char* out; unsigned char* image;
    int n, h0, w0, h, w;
    int new_r, new_c, y0, x0;          // picture area inside h x w (the geometry of letterbox.hip)
    int map_blocks, inner_w;
    double sy, sx;
};

__global__ void prior_clear_kernel(int* ws) { ws[0] = 0x7fffffff; ws[1] = -0x7fffffff - 1; }

__device__ __forceinline__ int acc_at(const FinK& k, long long r, long long c) { return k.acc[r * k.arow + c * k.acol]; }

__global__ __launch_bounds__(kThreads) void prior_minmax_kernel(const FinK k) {
    const long long P = (long long)k.h0 * k.w0;
    int lo = 0x7fffffff, hi = -0x7fffffff - 1;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < P; i += (long long)gridDim.x * kThreads) {
        long long r, c;
        if (k.inner_w) { r = i / k.w0; c = i - r * k.w0; } else { c = i / k.h0; r = i - c * k.h0; }
        const int v = acc_at(k, r, c);
        lo = min(lo, v); hi = max(hi, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lo = min(lo, __shfl_xor(lo, o)); hi = max(hi, __shfl_xor(hi, o)); }
    if ((threadIdx.x & 63) == 0) { atomicMin(k.ws, lo); atomicMax(k.ws + 1, hi); }
}

__device__ __forceinline__ int quantise(int s, double n, double mn, double den) {
    const double m = __ddiv_rn((double)s, n);
    return (int)rint(__ddiv_rn(__dmul_rn(255.0, __dsub_rn(m, mn)), den));
}

__global__ __launch_bounds__(kThreads) void prior_map_kernel(const FinK k) {
    const double n = (double)k.n;
    const double mn = __ddiv_rn((double)k.ws[0], n), mx = __ddiv_rn((double)k.ws[1], n);
    const double den = __dadd_rn(__dsub_rn(mx, mn), kEps);
    if ((int)blockIdx.x < k.map_blocks) {                  // one byte of the letterboxed map per thread, the bars included
        const int i = blockIdx.x * kThreads + threadIdx.x;
        if (i >= k.h * k.w) return;
        const int y = i / k.w, x = i - y * k.w;
        const int dy = y - k.y0, dx = x - k.x0;
        int v = 0;
        if (dy >= 0 && dy < k.new_r && dx >= 0 && dx < k.new_c) {
            int s0, b0, b1, c0, a0, a1;
            lb_tap(dy, k.sy, k.h0, s0, b0, b1);
            lb_tap(dx, k.sx, k.w0, c0, a0, a1);
            const int s1 = min(s0 + 1, k.h0 - 1), c1 = min(c0 + 1, k.w0 - 1);
            v = lb_mix(quantise(acc_at(k, s0, c0), n, mn, den), quantise(acc_at(k, s0, c1), n, mn, den),
                       quantise(acc_at(k, s1, c0), n, mn, den), quantise(acc_at(k, s1, c1), n, mn, den), a0, a1, b0, b1);
        }
        k.out[i] = (unsigned char)v;
        return;
    }
    const long long i = (long long)(blockIdx.x - k.map_blocks) * kThreads + threadIdx.x;      // the source-size picture
    if (i >= (long long)k.h0 * k.w0) return;
    const long long r = i / k.w0, c = i - r * k.w0;
    k.image[i] = (unsigned char)quantise(acc_at(k, r, c), n, mn, den);
}

}  // namespace

extern "C" int uavsal_prior_slab_frames(int64_t plane_pixels, int32_t n_img) {
    if (plane_pixels <= 0 || n_img <= 0) return 0;
    return slab_frames(plane_pixels, n_img);
}

extern "C" int uavsal_prior_sizeof_desc(int which) {
    return which == 0 ? (int)sizeof(uavsal_prior_acc_desc) : which == 1 ? (int)sizeof(uavsal_prior_finish_desc) : -1;
}

extern "C" int uavsal_prior_accumulate(const uavsal_prior_acc_desc* d, uavsal_stream_t stream) {
    if (!d || !d->frames || !d->acc) return UAVSAL_EINVAL;
    if (d->n_img <= 0 || d->h0 <= 0 || d->w0 <= 0) return UAVSAL_EINVAL;
    if (d->row_pitch < 0 || d->col_pitch < 0 || d->img_pitch < 0 || d->acc_row_pitch < 0 || d->acc_col_pitch < 0) return UAVSAL_EINVAL;
    if (reinterpret_cast<uintptr_t>(d->acc) & 3u) return UAVSAL_EALIGN;
    const long long P = (long long)d->h0 * d->w0;
    if (d->n_img > kMaxFrames || P > 0x7fffffffll) return UAVSAL_ESHAPE;
    AccK k;
    k.src = d->frames; k.row = d->row_pitch; k.col = d->col_pitch; k.img = d->img_pitch;
    k.acc = d->acc; k.arow = d->acc_row_pitch; k.acol = d->acc_col_pitch;
    k.F = d->n_img; k.h0 = d->h0; k.w0 = d->w0;
    k.S = slab_frames(P, d->n_img);
    k.head = k.tail = 0; k.nvec = 0;
    k.inner_w = d->col_pitch <= d->row_pitch;
    const unsigned slabs = (unsigned)((k.F + k.S - 1) / k.S);
    const bool flat = ((row_major(k.h0, k.w0, k.row, k.col) && row_major(k.h0, k.w0, k.arow, k.acol)) ||
                       (col_major(k.h0, k.w0, k.row, k.col) && col_major(k.h0, k.w0, k.arow, k.acol))) &&
                      (k.F == 1 || k.img % 16 == 0);
    if (flat) {
        const long long head = (16 - (long long)(reinterpret_cast<uintptr_t>(d->frames) & 15u)) & 15;
        k.head = (int)(head < P ? head : P);
        k.nvec = (P - k.head) / 16;
        k.tail = (int)(P - k.head - 16 * k.nvec);
        const long long blocks = k.nvec > 0 ? (k.nvec + kThreads - 1) / kThreads : 1;
        hipLaunchKernelGGL(prior_acc_flat_kernel, dim3((unsigned)blocks, slabs), dim3(kThreads), 0, (hipStream_t)stream, k);
    } else {
        hipLaunchKernelGGL(prior_acc_strided_kernel, dim3((unsigned)((P + kThreads - 1) / kThreads), slabs), dim3(kThreads), 0,
                           (hipStream_t)stream, k);
    }
    return uavsal_launch_status();
}

extern "C" int uavsal_prior_finish(const uavsal_prior_finish_desc* d, uavsal_stream_t stream) {
    if (!d || !d->acc || !d->ws || !d->out) return UAVSAL_EINVAL;
    if (d->n_frames <= 0 || d->h0 <= 0 || d->w0 <= 0 || d->h <= 0 || d->w <= 0) return UAVSAL_EINVAL;
    if (d->acc_row_pitch < 0 || d->acc_col_pitch < 0) return UAVSAL_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d->acc) | reinterpret_cast<uintptr_t>(d->ws)) & 3u) return UAVSAL_EALIGN;
    const long long P = (long long)d->h0 * d->w0;
    if (d->n_frames > kMaxFrames || P > 0x7fffffffll || (long long)d->h * d->w > 0x7fffffffll) return UAVSAL_ESHAPE;
    FinK k;
    k.acc = d->acc; k.arow = d->acc_row_pitch; k.acol = d->acc_col_pitch;
    k.ws = d->ws; k.out = d->out; k.image = d->image;
    k.n = d->n_frames; k.h0 = d->h0; k.w0 = d->w0; k.h = d->h; k.w = d->w;
    if ((double)d->h0 / d->h > (double)d->w0 / d->w) {      // utils_data.py:330-335
        k.new_r = d->h; k.new_c = (int)(((long long)d->w0 * d->h) / d->h0);
        k.y0 = 0; k.x0 = (d->w - k.new_c) / 2;
    } else {                                                // utils_data.py:336-341
        k.new_c = d->w; k.new_r = (int)(((long long)d->h0 * d->w) / d->w0);
        k.x0 = 0; k.y0 = (d->h - k.new_r) / 2;
    }
    if (k.new_r <= 0 || k.new_c <= 0 || k.new_r > d->h || k.new_c > d->w) return UAVSAL_ESHAPE;
    k.sy = (double)d->h0 / k.new_r; k.sx = (double)d->w0 / k.new_c;
    k.inner_w = k.acol <= k.arow;
    k.map_blocks = (int)(((long long)d->h * d->w + kThreads - 1) / kThreads);
    const long long image_blocks = d->image ? (P + kThreads - 1) / kThreads : 0;
    long long mm_blocks = (P + kThreads - 1) / kThreads;
    if (mm_blocks > 1024) mm_blocks = 1024;
    hipLaunchKernelGGL(prior_clear_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, k.ws);
    hipLaunchKernelGGL(prior_minmax_kernel, dim3((unsigned)mm_blocks), dim3(kThreads), 0, (hipStream_t)stream, k);
    hipLaunchKernelGGL(prior_map_kernel, dim3((unsigned)(k.map_blocks + image_blocks)), dim3(kThreads), 0, (hipStream_t)stream, k);
    return uavsal_launch_status();
}
