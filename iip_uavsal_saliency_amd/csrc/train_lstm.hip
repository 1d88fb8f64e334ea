// Back-propagation through the ConvLSTM recurrence of UAVSAL_LSTM (model.rnn, model_convlstm.py:111-126, bias = False, one
// layer): the two launches the existing kernels cannot do (include/uavsal_hip.h states the formulas).  Everything else of the
// walk -- the recompute of the pre-activations, the carry and input-gradient convs, the weight gradient -- is
// uavsal_conv_gemm / uavsal_conv3_wgrad as they are.
//
// 1. uavsal_lstm_scan: the cell-state history c_t = f c_{t-1} + i g from the dense pre-activations of ALL frames.  A lane
//    owns four channels of one pixel and walks t = 0 .. T-1 itself with the state in registers: one launch for the whole
//    history, three 16-byte loads (the i, f and g rows; o is not read) and one 16-byte store per step.  64 lanes of a wave
//    cover the 256 channels of one gate of one pixel: 1 KB contiguous per load instruction.
//
// 2. uavsal_lstm_gate_bwd: one step of the walk, element-wise, 16 bytes per lane and access: nine loads (G, the two
//    carries, four gate rows, c_t, c_{t-1}) and five stores (four gate rows of dcc, carry_c).  The gates are recomputed from
//    cc_t here; no activation is stored anywhere.  Every factor keeps its RELATIVE accuracy in a saturated gate:
//      e = exp(-|z|), d = 1 + e:   sigmoid = 1 / d or e / d,   s (1 - s) = e / d^2        (1 - fl(s) would be 0 or 2^-24 steps)
//      e2 = exp(-2|z|), d2 = 1 + e2:   1 - tanh^2 = 4 e2 / d2^2
//      m = expm1(-2|z|):   |tanh| = -m / (2 + m)                                          ((1 - e2) / (1 + e2) cancels at small z)
//    Memory bound: 13 floats read and 5 written per channel and pixel; the seven transcendentals per element hide behind them.
#include "common.h"

namespace {

__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// s = sigmoid(z), sp = s (1 - s)
__device__ __forceinline__ void sigm(float z, float& s, float& sp) {
    const float e = expf(-fabsf(z)), d = 1.f + e;
    s = z >= 0.f ? 1.f / d : e / d;
    sp = e / (d * d);
}

// t = tanh(z), q = 1 - tanh(z)^2
__device__ __forceinline__ void tanhq(float z, float& t, float& q) {
    const float a = -2.f * fabsf(z);
    const float m = expm1f(a), e2 = expf(a), d = 1.f + e2;
    const float r = -m / (2.f + m);
    t = z >= 0.f ? r : -r;
    q = 4.f * e2 / (d * d);
}

// ------------------------------------------------------------------------------------------------ scan
struct ScanK {
    const float *cc, *c0;
    float* cs;
    long long n4, n_pix;
    int T, C, C4;
};

__global__ __launch_bounds__(256) void lstm_scan_kernel(const ScanK k) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= k.n4) return;
    const long long p = i / k.C4;
    const int c = (int)(i - p * k.C4) * 4;
    f32x4 cv = k.c0 ? ld4(k.c0 + p * k.C + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
    const float* row = k.cc + p * (4ll * k.C) + c;
    float* out = k.cs + p * k.C + c;
    const long long rs = k.n_pix * 4ll * k.C, os = k.n_pix * (long long)k.C;       // one frame of cc, of c_seq
    f32x4 zi = ld4(row), zf = ld4(row + k.C), zg = ld4(row + 3 * k.C);
    for (int t = 0; t < k.T; ++t) {
        const f32x4 ci = zi, cf = zf, cg = zg;
        if (t + 1 < k.T) {                                                           // next frame's rows in flight
            row += rs;
            zi = ld4(row); zf = ld4(row + k.C); zg = ld4(row + 3 * k.C);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float si, sf, tg, unused;
            sigm(ci[q], si, unused);
            sigm(cf[q], sf, unused);
            tanhq(cg[q], tg, unused);
            cv[q] = sf * cv[q] + si * tg;
        }
        st4(out, cv);
        out += os;
    }
}

// ------------------------------------------------------------------------------------------------ gate
struct GateK {
    const float *g, *ch, *ccar, *cc, *c, *cp;
    float *dcc, *co;
    long long n4;
    int C, C4, ldg;
};

__global__ __launch_bounds__(256) void lstm_gate_bwd_kernel(const GateK k) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= k.n4) return;
    const long long p = i / k.C4;
    const int c = (int)(i - p * k.C4) * 4;
    const long long o = p * k.C + c;
    const float* row = k.cc + p * (4ll * k.C) + c;
    f32x4 gh = ld4(k.g + p * k.ldg + c);
    if (k.ch) gh += ld4(k.ch + o);
    const f32x4 zi = ld4(row), zf = ld4(row + k.C), zo = ld4(row + 2 * k.C), zg = ld4(row + 3 * k.C);
    const f32x4 ct = ld4(k.c + o), cp = ld4(k.cp + o);
    const bool has_cc = k.ccar != nullptr;
    f32x4 cin = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (has_cc) cin = ld4(k.ccar + o);
    f32x4 di, df, dO, dg, co;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float si, spi, sf, spf, so, spo, tg, qg, tc, qc;
        sigm(zi[q], si, spi);
        sigm(zf[q], sf, spf);
        sigm(zo[q], so, spo);
        tanhq(zg[q], tg, qg);
        tanhq(ct[q], tc, qc);
        const float a = gh[q] * so * qc;
        const float dc = has_cc ? cin[q] + a : a;
        di[q] = dc * tg * spi;
        df[q] = dc * cp[q] * spf;
        dO[q] = gh[q] * tc * spo;
        dg[q] = dc * si * qg;
        co[q] = dc * sf;
    }
    float* dr = k.dcc + p * (4ll * k.C) + c;
    st4(dr, di); st4(dr + k.C, df); st4(dr + 2 * k.C, dO); st4(dr + 3 * k.C, dg);
    st4(k.co + o, co);
}


}  // namespace

extern "C" int uavsal_lstm_sizeof_desc(int which) {
    return which == 0 ? (int)sizeof(uavsal_lstm_scan_desc) : which == 1 ? (int)sizeof(uavsal_lstm_gate_desc) : -1;
}

extern "C" int uavsal_lstm_scan(const uavsal_lstm_scan_desc* d, uavsal_stream_t stream) {
    if (!d || !d->cc || !d->c_seq) return UAVSAL_EINVAL;
    if (d->T <= 0 || d->n_pix <= 0 || d->C <= 0) return UAVSAL_EINVAL;
    if (d->C & 3) return UAVSAL_EALIGN;
    if (!al16(d->cc) || !al16(d->c_seq) || (d->c0 && !al16(d->c0))) return UAVSAL_EALIGN;
    ScanK k;
    k.cc = d->cc; k.c0 = d->c0; k.cs = d->c_seq;
    k.T = d->T; k.C = d->C; k.C4 = d->C / 4; k.n_pix = d->n_pix;
    if (d->n_pix > 0x7fffffffffffll / d->C / d->T) return UAVSAL_ESHAPE;            // T * n_pix * 4C floats in 64 bits
    k.n4 = d->n_pix * k.C4;
    const long long blocks = (k.n4 + 255) / 256;
    if (blocks > 0x7fffffffll) return UAVSAL_ESHAPE;
    hipLaunchKernelGGL(lstm_scan_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, k);
    return uavsal_launch_status();
}

extern "C" int uavsal_lstm_gate_bwd(const uavsal_lstm_gate_desc* d, uavsal_stream_t stream) {
    if (!d || !d->g || !d->cc || !d->c || !d->c_prev || !d->dcc || !d->carry_c_out) return UAVSAL_EINVAL;
    if (d->n_pix <= 0 || d->C <= 0) return UAVSAL_EINVAL;
    if (d->C & 3) return UAVSAL_EALIGN;
    if (d->ldg < d->C) return UAVSAL_EINVAL;
    if (d->ldg & 3) return UAVSAL_EALIGN;
    if (!al16(d->g) || !al16(d->cc) || !al16(d->c) || !al16(d->c_prev) || !al16(d->dcc) || !al16(d->carry_c_out) ||
        (d->carry_h && !al16(d->carry_h)) || (d->carry_c && !al16(d->carry_c))) return UAVSAL_EALIGN;
    if (d->n_pix > 0x7fffffffffffll / d->C) return UAVSAL_ESHAPE;
    GateK k;
    k.g = d->g; k.ch = d->carry_h; k.ccar = d->carry_c; k.cc = d->cc; k.c = d->c; k.cp = d->c_prev;
    k.dcc = d->dcc; k.co = d->carry_c_out;
    k.C = d->C; k.C4 = d->C / 4; k.ldg = d->ldg; k.n4 = d->n_pix * k.C4;
    const long long blocks = (k.n4 + 255) / 256;
    if (blocks > 0x7fffffffll) return UAVSAL_ESHAPE;
    hipLaunchKernelGGL(lstm_gate_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, k);
    return uavsal_launch_status();
}
