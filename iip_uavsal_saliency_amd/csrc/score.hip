// Saliency scoring: the seven metrics of the reference's scorer (utils_score_torch.py:53-229) over batches of frames.
// See uavsal_hip.h (uavsal_score_desc) for the contract and DESIGN.md "Scoring" for the exactness argument.
//
//   stats    [nblk x F]  per-block partial records (double; min / max are exact), no atomics
//   final    [F]         fixed-order merge of the partials -> stats[F][NSTAT]
//   pass2    [nblk x F]  centred moments, SIM and KLD sums (double partials); at fixations: the 11 threshold counts and
//                        the maximum of S (integer atomics), the AUC-Judd fixation values (gathered, sorted later)
//   sort     [runs]      bitonic sort of each run of <= RUN fixation values in LDS
//   hist     [nblk x runs] per pixel: upper_bound of S_jitter in the run -> LDS histogram -> integer atomics
//   judd     [F]         suffix sums -> #{pixels >= S_j}; merge ranks across runs; fp32 tp / fp; trapezoid
//   sample   [REPS x F x 2] AUC-shuffled / AUC-Borji: gathered samples, thresholds, trapezoid (numpy's order)
//   finish   [F]         NSS / CC / KLD / SIM from the moments, mean of the repetitions, NaN rows, [F][K] output
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 4096;                 // pixels per block of the per-pixel passes
constexpr int kRec1 = 12;                    // doubles per stats partial
constexpr int kRec2 = 8;                     // doubles per pass-2 partial
constexpr int kCnt = 16;                     // uint32 per frame: 0 gather slot, 1 max S bits (fixations), 2..12 counts
constexpr int kNthr = 11;                    // thresholds k * 0.1, k = 0..10 (S <= 1)
constexpr double kEps = 2.2204e-16;          // utils_score_torch.py:13
constexpr int kJuddThreads = 1024;

enum { M_AUC_S = 0, M_NSS = 1, M_AUC_J = 2, M_AUC_B = 3, M_KLD = 4, M_SIM = 5, M_CC = 6 };

struct Layout {
    int64_t nblk, part1, part2, cnt, fixv, hist, fpv, auc, judd, total;
};

inline int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

Layout layout(const uavsal_score_desc* d) {
    Layout L;
    const int64_t F = d->n_frames;
    L.nblk = ((int64_t)d->n_pix + kChunk - 1) / kChunk;
    int64_t o = 0;
    L.part1 = o; o = align256(o + F * L.nblk * kRec1 * 8);
    L.part2 = o; o = align256(o + F * L.nblk * kRec2 * 8);
    L.cnt = o;   o = align256(o + F * kCnt * 4);
    L.hist = o;  o = align256(o + (int64_t)d->total_runs * (UAVSAL_SCORE_RUN + 1) * 4);
    L.fixv = o;  o = align256(o + d->total_fix * 4);
    L.fpv = o;   o = align256(o + d->total_fix * 4);
    L.auc = o;   o = align256(o + 2 * F * UAVSAL_SCORE_REPS * 8);
    L.judd = o;  o = align256(o + F * 8);
    L.total = o;
    return L;
}

__device__ __forceinline__ float ld_val(const void* p, int u8, int64_t i) {
    return u8 ? (float)static_cast<const uint8_t*>(p)[i] : static_cast<const float*>(p)[i];
}

// S = (y - min) / (max - min + EPS) exactly as torch computes it in fp32 (utils_score_torch.py:74,122,163)
__device__ __forceinline__ float norm_s(float y, float mn, float mx) {
    const float eps = (float)kEps;
    return __fdiv_rn(__fsub_rn(y, mn), __fadd_rn(__fsub_rn(mx, mn), eps));
}

__device__ __forceinline__ uint32_t ld_u32(const uint32_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

template <typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, T* sm, Op op) {
    // fixed tree over kThreads lanes: deterministic
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] = op(sm[threadIdx.x], sm[threadIdx.x + s]);
        __syncthreads();
    }
    T r = sm[0];
    __syncthreads();
    return r;
}

struct Add { template <typename T> __device__ T operator()(T a, T b) const { return a + b; } };
struct Min { template <typename T> __device__ T operator()(T a, T b) const { return b < a ? b : a; } };
struct Max { template <typename T> __device__ T operator()(T a, T b) const { return b > a ? b : a; } };

// ------------------------------------------------------------------------------------------------ statistics
__global__ __launch_bounds__(kThreads) void stats_kernel(const uavsal_score_desc d, double* part) {
    __shared__ double sm[kThreads];
    const int f = blockIdx.y;
    const int64_t N = d.n_pix, base = (int64_t)f * N;
    const int64_t p0 = (int64_t)blockIdx.x * kChunk, p1 = p0 + kChunk < N ? p0 + kChunk : N;
    float pmin = INFINITY, pmax = -INFINITY, jmin = INFINITY, jmax = -INFINITY, fmin = INFINITY, fmax = -INFINITY;
    double sp = 0, sf = 0, sl = 0, nfix = 0, nzl = 0;
    for (int64_t i = p0 + threadIdx.x; i < p1; i += kThreads) {
        const float p = ld_val(d.sal, d.sal_u8, base + i);
        const float fm = d.fix_map[base + i];
        const float l = ld_val(d.fix_loc, d.loc_u8, base + i);
        pmin = fminf(pmin, p); pmax = fmaxf(pmax, p);
        if (d.jitter) {
            const float pj = __fadd_rn(p, d.jitter[base + i]);
            jmin = fminf(jmin, pj); jmax = fmaxf(jmax, pj);
        }
        fmin = fminf(fmin, fm); fmax = fmaxf(fmax, fm);
        sp += (double)p; sf += (double)fm; sl += (double)l;
        nfix += l > 0.5f ? 1.0 : 0.0;
        nzl += l != 0.0f ? 1.0 : 0.0;
    }
    double r[kRec1];
    r[0] = block_reduce((double)pmin, sm, Min());
    r[1] = block_reduce((double)pmax, sm, Max());
    r[2] = block_reduce((double)jmin, sm, Min());
    r[3] = block_reduce((double)jmax, sm, Max());
    r[4] = block_reduce(sp, sm, Add());
    r[5] = block_reduce((double)fmin, sm, Min());
    r[6] = block_reduce((double)fmax, sm, Max());
    r[7] = block_reduce(sf, sm, Add());
    r[8] = block_reduce(sl, sm, Add());
    r[9] = block_reduce(nfix, sm, Add());
    r[10] = block_reduce(nzl, sm, Add());
    r[11] = 0;
    if (threadIdx.x < kRec1) part[((int64_t)f * gridDim.x + blockIdx.x) * kRec1 + threadIdx.x] = r[threadIdx.x];
}

__global__ __launch_bounds__(kThreads) void stats_final_kernel(const uavsal_score_desc d, const double* part, int nblk) {
    __shared__ double sm[kThreads];
    const int f = blockIdx.x;
    const double* P = part + (int64_t)f * nblk * kRec1;
    double v[kRec1];
    for (int q = 0; q < kRec1; ++q) v[q] = (q == 0 || q == 2 || q == 5) ? INFINITY : (q == 1 || q == 3 || q == 6) ? -INFINITY : 0.0;
    for (int b = threadIdx.x; b < nblk; b += kThreads) {
        const double* r = P + (int64_t)b * kRec1;
        v[0] = fmin(v[0], r[0]); v[1] = fmax(v[1], r[1]); v[2] = fmin(v[2], r[2]); v[3] = fmax(v[3], r[3]);
        v[4] += r[4]; v[5] = fmin(v[5], r[5]); v[6] = fmax(v[6], r[6]);
        v[7] += r[7]; v[8] += r[8]; v[9] += r[9]; v[10] += r[10];
    }
    double o[UAVSAL_SCORE_NSTAT];
    o[0] = block_reduce(v[0], sm, Min()); o[1] = block_reduce(v[1], sm, Max());
    o[2] = block_reduce(v[2], sm, Min()); o[3] = block_reduce(v[3], sm, Max());
    o[4] = block_reduce(v[4], sm, Add());
    o[5] = block_reduce(v[5], sm, Min()); o[6] = block_reduce(v[6], sm, Max());
    o[7] = block_reduce(v[7], sm, Add()); o[8] = block_reduce(v[8], sm, Add());
    o[9] = block_reduce(v[9], sm, Add()); o[10] = block_reduce(v[10], sm, Add());
    if (!d.jitter) { o[2] = o[0]; o[3] = o[1]; }
    for (int q = 11; q < UAVSAL_SCORE_NSTAT; ++q) o[q] = 0;
    if (threadIdx.x < UAVSAL_SCORE_NSTAT) d.stats[(int64_t)f * UAVSAL_SCORE_NSTAT + threadIdx.x] = o[threadIdx.x];
}

// ------------------------------------------------------------------------------------------------ second pass
__global__ __launch_bounds__(kThreads) void pass2_kernel(const uavsal_score_desc d, double* part, uint32_t* cnt, float* fixv) {
    __shared__ double sm[kThreads];
    __shared__ uint32_t lc[kNthr];
    __shared__ uint32_t lmax;
    const int f = blockIdx.y;
    const double* st = d.stats + (int64_t)f * UAVSAL_SCORE_NSTAT;
    const int64_t N = d.n_pix, base = (int64_t)f * N;
    const double dN = (double)N;
    const float pmin = (float)st[0], pmax = (float)st[1], jmin = (float)st[2], jmax = (float)st[3];
    const double mp = st[4] / dN, fmn = st[5], fmx = st[6], mf = st[7] / dN;
    // SIM (utils_score_torch.py:206-218) and KLD (:180-185) normalisers, in double
    const double rT = (fmx - fmn) + kEps, rP = ((double)pmax - (double)pmin) + kEps;
    const double sumT = (st[7] - dN * fmn) / rT, sumP = (st[4] - dN * (double)pmin) / rP;
    const double kT = st[7] + kEps, kP = st[4] + kEps;
    const int64_t fo = d.fix_off ? d.fix_off[f] : 0;
    const int64_t cap = d.fix_off ? d.fix_off[f + 1] - fo : 0;
    if (threadIdx.x < kNthr) lc[threadIdx.x] = 0;
    if (threadIdx.x == 0) lmax = 0;
    __syncthreads();
    const int64_t p0 = (int64_t)blockIdx.x * kChunk, p1 = p0 + kChunk < N ? p0 + kChunk : N;
    double spp = 0, sff = 0, spf = 0, slp = 0, sim = 0, kl = 0;
    for (int64_t i = p0 + threadIdx.x; i < p1; i += kThreads) {
        const float p = ld_val(d.sal, d.sal_u8, base + i);
        const float fm = d.fix_map[base + i];
        const float l = ld_val(d.fix_loc, d.loc_u8, base + i);
        const double dp = (double)p - mp, df = (double)fm - mf;
        spp += dp * dp; sff += df * df; spf += dp * df; slp += (double)l * dp;
        const double tn = ((double)fm - fmn) / rT / (sumT + kEps);
        const double pn = ((double)p - (double)pmin) / rP / (sumP + kEps);
        sim += fmin(tn, pn);
        const double t = (double)fm / kT, q = (double)p / kP;
        kl += t * log(t / (q + kEps) + kEps);
        if (l > 0.5f) {
            const float s = norm_s(p, pmin, pmax);
            atomicMax(&lmax, __float_as_uint(s));
#pragma unroll
            for (int k = 0; k < kNthr; ++k)
                if ((double)s >= k * 0.1) atomicAdd(&lc[k], 1u);
            if (cap > 0) {
                const float pj = d.jitter ? __fadd_rn(p, d.jitter[base + i]) : p;
                const uint32_t slot = atomicAdd(&cnt[f * kCnt + 0], 1u);
                if ((int64_t)slot < cap) fixv[fo + slot] = norm_s(pj, jmin, jmax);
            }
        }
    }
    double r[6];
    r[0] = block_reduce(spp, sm, Add()); r[1] = block_reduce(sff, sm, Add()); r[2] = block_reduce(spf, sm, Add());
    r[3] = block_reduce(slp, sm, Add()); r[4] = block_reduce(sim, sm, Add()); r[5] = block_reduce(kl, sm, Add());
    if (threadIdx.x < kRec2) part[((int64_t)f * gridDim.x + blockIdx.x) * kRec2 + threadIdx.x] = threadIdx.x < 6 ? r[threadIdx.x] : 0.0;
    if (threadIdx.x < kNthr && lc[threadIdx.x]) atomicAdd(&cnt[f * kCnt + 2 + threadIdx.x], lc[threadIdx.x]);
    if (threadIdx.x == 0 && lmax) atomicMax(&cnt[f * kCnt + 1], lmax);
}

// frame of a run: run_off[f] <= r < run_off[f + 1]
__device__ __forceinline__ int run_frame(const int64_t* run_off, int F, int64_t r) {
    int lo = 0, hi = F;                       // find the last f with run_off[f] <= r
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (run_off[mid] <= r) lo = mid; else hi = mid; }
    return lo;
}

__device__ __forceinline__ int run_len(const uavsal_score_desc& d, int f, int64_t r, int64_t* first) {
    const int64_t k = r - d.run_off[f];
    const int64_t n = d.fix_off[f + 1] - d.fix_off[f];
    *first = d.fix_off[f] + k * UAVSAL_SCORE_RUN;
    const int64_t m = n - k * UAVSAL_SCORE_RUN;
    return (int)(m < UAVSAL_SCORE_RUN ? m : UAVSAL_SCORE_RUN);
}

// ------------------------------------------------------------------------------------------------ AUC-Judd
__global__ __launch_bounds__(1024) void sort_kernel(const uavsal_score_desc d, float* fixv) {
    __shared__ float v[UAVSAL_SCORE_RUN];
    const int64_t r = blockIdx.x;
    const int f = run_frame(d.run_off, d.n_frames, r);
    int64_t first;
    const int m = run_len(d, f, r, &first);
    int P = 64;
    while (P < m) P <<= 1;
    for (int i = threadIdx.x; i < P; i += blockDim.x) v[i] = i < m ? fixv[first + i] : INFINITY;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < P; i += blockDim.x) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const float a = v[i], b = v[ixj];
                    const bool up = (i & k) == 0;
                    if (up ? (a > b) : (a < b)) { v[i] = b; v[ixj] = a; }
                }
            }
            __syncthreads();
        }
    }
    for (int i = threadIdx.x; i < m; i += blockDim.x) fixv[first + i] = v[i];
}

__global__ __launch_bounds__(kThreads) void hist_kernel(const uavsal_score_desc d, const float* fixv, uint32_t* hist) {
    __shared__ float v[UAVSAL_SCORE_RUN];
    __shared__ uint32_t h[UAVSAL_SCORE_RUN + 1];
    const int64_t r = blockIdx.y;
    const int f = run_frame(d.run_off, d.n_frames, r);
    int64_t first;
    const int m = run_len(d, f, r, &first);
    const double* st = d.stats + (int64_t)f * UAVSAL_SCORE_NSTAT;
    const float jmin = (float)st[2], jmax = (float)st[3];
    for (int i = threadIdx.x; i < m; i += kThreads) v[i] = fixv[first + i];
    for (int i = threadIdx.x; i <= m; i += kThreads) h[i] = 0;
    __syncthreads();
    const float vlo = v[0];
    const int64_t N = d.n_pix, base = (int64_t)f * N;
    const int64_t p0 = (int64_t)blockIdx.x * kChunk, p1 = p0 + kChunk < N ? p0 + kChunk : N;
    for (int64_t i = p0 + threadIdx.x; i < p1; i += kThreads) {
        float p = ld_val(d.sal, d.sal_u8, base + i);
        if (d.jitter) p = __fadd_rn(p, d.jitter[base + i]);
        const float s = norm_s(p, jmin, jmax);
        if (!(s >= vlo)) continue;            // upper_bound = 0: counts nothing
        int lo = 0, hi = m;                   // upper_bound: first index with v[idx] > s
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (v[mid] <= s) lo = mid + 1; else hi = mid; }
        atomicAdd(&h[lo], 1u);
    }
    __syncthreads();
    uint32_t* H = hist + r * (UAVSAL_SCORE_RUN + 1);
    for (int i = 1 + threadIdx.x; i <= m; i += kThreads)
        if (h[i]) atomicAdd(&H[i], h[i]);
}

// #{q in run with c_q <= c} (le) or < c (lt); counts are non-increasing along the run
__device__ __forceinline__ int count_below(const uint32_t* c, int m, uint32_t x, bool le) {
    int lo = 0, hi = m;                       // first index whose count is <= x (le) / < x (lt)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const bool in = le ? c[mid] <= x : c[mid] < x;
        if (in) hi = mid; else lo = mid + 1;
    }
    return m - lo;
}

__global__ __launch_bounds__(kJuddThreads) void judd_kernel(const uavsal_score_desc d, uint32_t* hist, float* fpv, double* judd) {
    __shared__ uint32_t a[UAVSAL_SCORE_RUN];
    __shared__ uint32_t tsum[kJuddThreads];
    __shared__ double dsm[kJuddThreads];
    const int f = blockIdx.x;
    const double* st = d.stats + (int64_t)f * UAVSAL_SCORE_NSTAT;
    const int64_t n = d.fix_off[f + 1] - d.fix_off[f];
    const int64_t N = d.n_pix;
    if (n <= 0 || n != (int64_t)st[9] || !(st[3] > st[2])) {   // utils_score_torch.py:54-55
        if (threadIdx.x == 0) judd[f] = NAN;
        return;
    }
    const int64_t r0 = d.run_off[f], r1 = d.run_off[f + 1];
    // 1. per run: cnt_i = sum_{b > i} h[b] = #{pixels with S >= v_i}, written over the run's histogram
    for (int64_t r = r0; r < r1; ++r) {
        int64_t first;
        const int m = run_len(d, f, r, &first);
        uint32_t* H = hist + r * (UAVSAL_SCORE_RUN + 1);
        constexpr int per = UAVSAL_SCORE_RUN / kJuddThreads;
        // reversed order: b[k] = h[m - k], inclusive prefix over k gives cnt_{m-1-k}
        uint32_t loc[per], s = 0;
        for (int q = 0; q < per; ++q) {
            const int k = threadIdx.x * per + q;
            s += k < m ? H[m - k] : 0u;
            loc[q] = s;
        }
        tsum[threadIdx.x] = s;
        __syncthreads();
        for (int off = 1; off < kJuddThreads; off <<= 1) {
            const uint32_t add = threadIdx.x >= (unsigned)off ? tsum[threadIdx.x - off] : 0u;
            __syncthreads();
            tsum[threadIdx.x] += add;
            __syncthreads();
        }
        const uint32_t before = threadIdx.x ? tsum[threadIdx.x - 1] : 0u;
        for (int q = 0; q < per; ++q) {
            const int k = threadIdx.x * per + q;
            if (k < m) a[m - 1 - k] = before + loc[q];
        }
        __syncthreads();
        for (int i = threadIdx.x; i < m; i += kJuddThreads) H[i] = a[i];
        __syncthreads();
    }
    __threadfence_block();
    __syncthreads();
    // 2. rank of each count in the ascending order of all counts (stable merge of the runs); fp / tp of that rank
    const float fn = (float)n, fden = (float)(N - n);
    for (int64_t r = r0; r < r1; ++r) {
        int64_t first;
        const int m = run_len(d, f, r, &first);
        const uint32_t* H = hist + r * (UAVSAL_SCORE_RUN + 1);
        for (int i = threadIdx.x; i < m; i += kJuddThreads) {
            const uint32_t c = H[i];
            int64_t q = m - 1 - i;
            for (int64_t r2 = r0; r2 < r1; ++r2) {
                if (r2 == r) continue;
                int64_t f2;
                const int m2 = run_len(d, f, r2, &f2);
                q += count_below(hist + r2 * (UAVSAL_SCORE_RUN + 1), m2, c, r2 < r);
            }
            // utils_score_torch.py:68: fp = (above_th - arange - 1) / (n_pixels - n_fix), int64 -> fp32
            if (q < n) fpv[d.fix_off[f] + q] = __fdiv_rn((float)((int64_t)c - q - 1), fden);
        }
    }
    __threadfence_block();
    __syncthreads();
    // 3. torch.trapz(tp, fp) over the n + 2 points: sum of (fp[k+1] - fp[k]) * (tp[k] + tp[k+1]) / 2
    const float* FP = fpv + d.fix_off[f];
    double acc = 0;
    for (int64_t k = threadIdx.x; k <= n; k += kJuddThreads) {
        const float x0 = k == 0 ? 0.0f : FP[k - 1], x1 = k == n ? 1.0f : FP[k];
        const float y0 = k == 0 ? 0.0f : __fdiv_rn((float)k, fn), y1 = k == n ? 1.0f : __fdiv_rn((float)(k + 1), fn);
        acc += (double)__fmul_rn(__fadd_rn(y0, y1), __fsub_rn(x1, x0));
    }
    acc = block_reduce(acc, dsm, Add());
    if (threadIdx.x == 0) judd[f] = acc / 2.0;
}

// ------------------------------------------------------------------------------------------------ AUC-Borji / shuffled
// numpy's add.reduce of n <= 128 doubles (pairwise_sum: 8 accumulators; identity 0 added in front)
__device__ double np_sum(const double* a, int n) {
    double res;
    if (n < 8) {
        res = 0.0;
        for (int i = 0; i < n; ++i) res += a[i];
    } else {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        int i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] += a[i + j];
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
    }
    return 0.0 + res;
}

__global__ __launch_bounds__(kThreads) void sample_kernel(const uavsal_score_desc d, const uint32_t* cnt, double* auc) {
    __shared__ uint32_t lc[kNthr];
    __shared__ uint32_t lmax;
    const int rep = blockIdx.x, f = blockIdx.y, s = blockIdx.z;
    const int64_t* off = d.samp_off[s];
    if (!off || !d.samp[s]) return;
    const int64_t o = off[f], n = (off[f + 1] - o) / UAVSAL_SCORE_REPS;
    double* out = auc + ((int64_t)s * d.n_frames + f) * UAVSAL_SCORE_REPS + rep;
    if (n <= 0) { if (threadIdx.x == 0) *out = NAN; return; }
    const double* st = d.stats + (int64_t)f * UAVSAL_SCORE_NSTAT;
    const float pmin = (float)st[0], pmax = (float)st[1];
    const int64_t N = d.n_pix, base = (int64_t)f * N;
    if (threadIdx.x < kNthr) lc[threadIdx.x] = 0;
    if (threadIdx.x == 0) lmax = 0;
    __syncthreads();
    uint32_t c[kNthr] = {0};
    float mx = 0.0f;
    const int32_t* idx = d.samp[s] + o + (int64_t)rep * n;
    for (int64_t i = threadIdx.x; i < n; i += kThreads) {
        if (o + (int64_t)rep * n + i >= d.n_samp[s]) break;
        const int32_t px = idx[i];
        if (px < 0 || px >= N) continue;       // the host draws inside [0, N); never read outside the frame
        const float v = norm_s(ld_val(d.sal, d.sal_u8, base + px), pmin, pmax);
        mx = fmaxf(mx, v);
#pragma unroll
        for (int k = 0; k < kNthr; ++k) c[k] += (double)v >= k * 0.1 ? 1u : 0u;
    }
#pragma unroll
    for (int k = 0; k < kNthr; ++k) if (c[k]) atomicAdd(&lc[k], c[k]);
    atomicMax(&lmax, __float_as_uint(mx));
    __syncthreads();
    if (threadIdx.x != 0) return;
    const uint32_t* C = cnt + f * kCnt;
    // np.r_[0:m:0.1]: m the fp32 max over S_fix and this repetition's samples; length ceil(m / 0.1) in fp32
    const float m = fmaxf(__uint_as_float(ld_u32(&C[1])), __uint_as_float(lmax));
    int L = (int)ceilf(__fdiv_rn(m, 0.1f));
    L = L < 0 ? 0 : (L > kNthr ? kNthr : L);
    const double nfix = st[9], nden = s == 0 ? (double)n : nfix;   // AUC-shuffled: n_fix_oth (:147)
    double tp[kNthr + 2], fp[kNthr + 2], term[kNthr + 1];
    tp[0] = 0; fp[0] = 0; tp[L + 1] = 1; fp[L + 1] = 1;
    for (int i = 1; i <= L; ++i) {              // thresholds descending: (L - i) * 0.1
        tp[i] = (double)ld_u32(&C[2 + L - i]) / nfix;
        fp[i] = (double)lc[L - i] / nden;
    }
    for (int i = 0; i <= L; ++i) term[i] = (fp[i + 1] - fp[i]) * (tp[i + 1] + tp[i]) / 2.0;   // np.trapz
    *out = np_sum(term, L + 1);
}

// ------------------------------------------------------------------------------------------------ finish
__global__ __launch_bounds__(kThreads) void finish_kernel(const uavsal_score_desc d, const double* part, int nblk,
                                                          const double* auc, const double* judd) {
    __shared__ double sm[kThreads];
    const int f = blockIdx.x;
    const double* P = part + (int64_t)f * nblk * kRec2;
    double v[6] = {0, 0, 0, 0, 0, 0};
    for (int b = threadIdx.x; b < nblk; b += kThreads)
        for (int q = 0; q < 6; ++q) v[q] += P[(int64_t)b * kRec2 + q];
    for (int q = 0; q < 6; ++q) v[q] = block_reduce(v[q], sm, Add());
    if (threadIdx.x != 0) return;
    const double* st = d.stats + (int64_t)f * UAVSAL_SCORE_NSTAT;
    const double dN = (double)d.n_pix;
    const double spp = v[0], sff = v[1], spf = v[2], slp = v[3];
    const double sdp = sqrt(spp / (dN - 1.0)), sdf = sqrt(sff / (dN - 1.0));      // torch.std: unbiased
    double val[UAVSAL_SCORE_NKEY];
    val[M_NSS] = (slp / (sdp + kEps)) / (st[8] + kEps);                            // :196-200
    {
        const double a = 1.0 / (sdf + kEps), b = 1.0 / (sdp + kEps);              // :188-197
        val[M_CC] = (a * b * spf) / (sqrt((b * b * spp) * (a * a * sff)) + kEps);
    }
    val[M_KLD] = v[5];
    val[M_SIM] = v[4];
    val[M_AUC_J] = judd ? judd[f] : NAN;
    for (int s = 0; s < 2; ++s) {
        const int id = s == 0 ? M_AUC_S : M_AUC_B;
        if (!d.samp_off[s] || d.samp_off[s][f + 1] == d.samp_off[s][f]) { val[id] = NAN; continue; }
        val[id] = np_sum(auc + ((int64_t)s * d.n_frames + f) * UAVSAL_SCORE_REPS, UAVSAL_SCORE_REPS) / UAVSAL_SCORE_REPS;
    }
    const bool dead = d.nan_rows && ((st[0] == 0 && st[1] == 0) || (st[5] == 0 && st[6] == 0) || st[10] == 0);
    for (int k = 0; k < d.n_keys; ++k) d.out[(int64_t)f * d.n_keys + k] = dead ? NAN : (float)val[d.keys[k]];
}

int check_desc(const uavsal_score_desc* d) {
    if (!d || !d->sal || !d->fix_loc || !d->fix_map || !d->stats || !d->ws || d->n_frames <= 0 || d->n_pix <= 1)
        return UAVSAL_EINVAL;
    if (d->total_fix < 0 || d->total_runs < 0 || d->total_fix > (int64_t)d->n_frames * d->n_pix) return UAVSAL_EINVAL;
    if (d->ws_bytes < layout(d).total) return UAVSAL_EINVAL;
    if ((uintptr_t)d->fix_map & 3 || (!d->sal_u8 && ((uintptr_t)d->sal & 3)) || (!d->loc_u8 && ((uintptr_t)d->fix_loc & 3))
        || ((uintptr_t)d->jitter & 3) || ((uintptr_t)d->stats & 7) || ((uintptr_t)d->ws & 255))
        return UAVSAL_EALIGN;
    return 0;
}

}  // namespace

extern "C" int64_t uavsal_score_workspace_bytes(const uavsal_score_desc* d) {
    if (!d || d->n_frames <= 0 || d->n_pix <= 1 || d->total_fix < 0 || d->total_runs < 0) return UAVSAL_EINVAL;
    return layout(d).total;
}

extern "C" int uavsal_score_stats(const uavsal_score_desc* d, uavsal_stream_t stream) {
    if (const int e = check_desc(d)) return e;
    const Layout L = layout(d);
    char* ws = static_cast<char*>(d->ws);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(stats_kernel, dim3((unsigned)L.nblk, (unsigned)d->n_frames), dim3(kThreads), 0, s, *d,
                       reinterpret_cast<double*>(ws + L.part1));
    hipLaunchKernelGGL(stats_final_kernel, dim3((unsigned)d->n_frames), dim3(kThreads), 0, s, *d,
                       reinterpret_cast<const double*>(ws + L.part1), (int)L.nblk);
    return uavsal_launch_status();
}

extern "C" int uavsal_score_run(const uavsal_score_desc* d, uavsal_stream_t stream) {
    if (const int e = check_desc(d)) return e;
    if (!d->out || d->n_keys <= 0 || d->n_keys > UAVSAL_SCORE_NKEY) return UAVSAL_EINVAL;
    bool judd = false, samp = false;
    for (int k = 0; k < d->n_keys; ++k) {
        if (d->keys[k] < 0 || d->keys[k] >= UAVSAL_SCORE_NKEY) return UAVSAL_EINVAL;
        judd |= d->keys[k] == M_AUC_J;
        samp |= d->keys[k] == M_AUC_S || d->keys[k] == M_AUC_B;
    }
    if (judd && (!d->fix_off || !d->run_off)) return UAVSAL_EINVAL;
    if (!judd && (d->total_fix || d->total_runs)) return UAVSAL_EINVAL;
    for (int q = 0; q < 2; ++q)
        if (!d->samp[q] != !d->samp_off[q] || d->n_samp[q] < 0 || (!d->samp[q] && d->n_samp[q])) return UAVSAL_EINVAL;
    if ((uintptr_t)d->out & 3 || (uintptr_t)d->fix_off & 7 || (uintptr_t)d->run_off & 7 || (uintptr_t)d->samp[0] & 3
        || (uintptr_t)d->samp[1] & 3 || (uintptr_t)d->samp_off[0] & 7 || (uintptr_t)d->samp_off[1] & 7)
        return UAVSAL_EALIGN;
    const Layout L = layout(d);
    char* ws = static_cast<char*>(d->ws);
    hipStream_t s = (hipStream_t)stream;
    uint32_t* cnt = reinterpret_cast<uint32_t*>(ws + L.cnt);
    uint32_t* hist = reinterpret_cast<uint32_t*>(ws + L.hist);
    float* fixv = reinterpret_cast<float*>(ws + L.fixv);
    const int64_t F = d->n_frames;
    hipError_t e = hipMemsetAsync(cnt, 0, (L.hist - L.cnt) + (int64_t)d->total_runs * (UAVSAL_SCORE_RUN + 1) * 4, s);  // cnt, hist adjacent
    if (e != hipSuccess) return (int)e;
    uavsal_score_desc dj = *d;
    if (!judd) { dj.fix_off = nullptr; dj.run_off = nullptr; }
    hipLaunchKernelGGL(pass2_kernel, dim3((unsigned)L.nblk, (unsigned)F), dim3(kThreads), 0, s, dj,
                       reinterpret_cast<double*>(ws + L.part2), cnt, fixv);
    double* jd = nullptr;
    if (judd) {
        jd = reinterpret_cast<double*>(ws + L.judd);
        if (d->total_runs > 0) {
            hipLaunchKernelGGL(sort_kernel, dim3((unsigned)d->total_runs), dim3(1024), 0, s, *d, fixv);
            hipLaunchKernelGGL(hist_kernel, dim3((unsigned)L.nblk, (unsigned)d->total_runs), dim3(kThreads), 0, s, *d,
                               (const float*)fixv, hist);
        }
        hipLaunchKernelGGL(judd_kernel, dim3((unsigned)F), dim3(kJuddThreads), 0, s, *d, hist,
                           reinterpret_cast<float*>(ws + L.fpv), jd);
    }
    double* auc = reinterpret_cast<double*>(ws + L.auc);
    if (samp)
        hipLaunchKernelGGL(sample_kernel, dim3(UAVSAL_SCORE_REPS, (unsigned)F, 2), dim3(kThreads), 0, s, *d,
                           (const uint32_t*)cnt, auc);
    hipLaunchKernelGGL(finish_kernel, dim3((unsigned)F), dim3(kThreads), 0, s, *d,
                       reinterpret_cast<const double*>(ws + L.part2), (int)L.nblk, (const double*)auc, (const double*)jd);
    return uavsal_launch_status();
}
