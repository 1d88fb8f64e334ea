"""Float64 restatement of BatchNorm in TRAINING mode (csrc/train_bn.hip, train/bn.py) and of the decoder conv_out_st built on
it (train.decoder_forward_batch / decoder_backward_batch): the formulas of include/uavsal_hip.h, the seeded inputs of the
tests, wrong variants, and per-element bounds in the convention of tests/plan_ref64.py and tests/decoder_ref64.py:

    |kernel - ref| <= bound,      U = 2^-24 (unit roundoff of fp32), D = 2^-53, LAMBDA = 8, EPS = 8 U

The kernels are held STAGE BY STAGE: every stage function below takes the fp32 tensors the device's stage read (as float64)
and restates that one stage in float64, so a bound counts only the roundings of that stage, one by one, on sums of absolute
values -- unit roundoff x chain length x sum |a| |b|.  A ReLU6 mask is the DEVICE's (`mask=`: taken from the device's own
activation of the stored raw u, which every kernel recomputes by the same single fused multiply-add), as in
tests/backbone_ref64.py: a float64 pre-activation within one rounding of a clamp may fall on the other side, so no element
has to be excluded.  No factor is fitted to what a kernel gives.

  stats       S1 = sum u, S2 = sum u^2: fp32 u, products exact in double, P additions in double each: the mean carries
              e_mu = P D mean|u|, the variance e_var = P D mean(u^2) + 2 |mu| e_mu + e_mu^2; the five outputs are formed in
              double (under 16 operations: 16 D relative, `DS`) and rounded once (U):
                mu: (U + DS)|mu| + e_mu          var: (U + DS) var + e_var       r: (U + DS) r + r^3 e_var / 2
                s = gamma r: (U + DS)|s| + |gamma| r^3 e_var / 2
                b = beta - mu s: (U + DS)(|beta| + |mu s|) + |s| e_mu + |mu gamma| r^3 e_var / 2
  running     blended in double from the double mean / variance, rounded once: against fl32(float64 blend) the two roundings
              see values e_mu (e_var) apart, far below half an ulp, so they differ by at most ONE ulp (a value next to a
              rounding boundary); the test compares the bit patterns.
  apply       a = fma(u, s, b): one rounding, U |a|; ReLU6 is 1-Lipschitz and exact: U min(|a|, 6)(1 + U); sigmoid
              1 / (1 + expf(-a)): expf within 1 ulp = 2 U, the sum and the quotient one rounding each: 4 U y, plus the
              pre-activation's U |a| y (1 - y) (tests/train_ref64.py counts the same way).
  apply_dot   sum_c w[c] d[p][c] over C channels: a lane's chain of C / 64 fused multiply-adds and the 6 additions of the
              butterfly, (C / 64 + 6) U sum |w| |d|, plus sum |w| err(d).
  bwd_sums    g_a: exact for a given g under a mask (none / ReLU6); rank-one g = fl(g_pix g_chan): U |g|; sigmoid
              g fl(y fl(1 - y)): |g| (err(y) |1 - 2 y| + 2 U y (1 - y)).  xh = fl(fl(u - mu) r): 2 U |xh|.  Products and sums in
              double: P D on each sum of absolute values.  d beta: sum err(g_a); d gamma: sum (err(g_a) |xh| + 2 U |g_a xh|);
              the projection's weight gradient sum g_pix act(a): sum |g_pix| err(act).  The fp32 outputs add U |S|.
  bwd_apply   c1 = fl(S0 / P), c2 = fl(S1 / P): U each; t1 = fl(g_a - c1), t2 = fma(-xh, c2, t1), g_u = fl(s t2); with
              A = |g_a| + |c1| + |xh c2|:  |s| (err(g_a) + 5 U A)  (U |c1|; U for t1; 2 U |xh c2| + U |xh c2| for xh and c2;
              U for t2; U for the last product -- never more than five roundings on any term).
  dw_wgrad    products exact in double: P D sum |g| |e| + U |S|.
  dw_raw      uavsal_dw3x3 with unit scale, zero bias: nine fp32 products, (3 LAMBDA + 2) U sum |w| |x| (train_ref64's count
              for a nine-tap sum, two roundings for the epilogue).
  conv1x1     uavsal_conv_gemm: plan_ref64.rtol("f32", K) sum |w| |x| + EPS |y|.
  pix_gemm    decoder_ref64.pix_gemm_ref.

Shapes (T, H, W): (2, 5, 7) and (3, 5, 7) (odd in both directions, one slab), (3, 13, 17): 39 picture rows in slabs of
ceil(512 / 17) = 31 rows: two slabs, the last one 8 rows, the first ending inside frame 2 (`slab_partition` restates the rule).
Every function takes and returns float64 tensors on the device of its inputs unless it says numpy."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from plan_ref64 import EPS, LAMBDA, U, rtol
from saturate_bn import GAIN, SHIFT

C_IN, HID = 256, 1536
D = 2.0 ** -53
DS = 16 * D
NAMES = ("conv.0.0.weight", "conv.0.1.weight", "conv.0.1.bias", "conv.1.0.weight", "conv.1.1.weight", "conv.1.1.bias",
         "conv.2.weight", "conv.3.weight", "conv.3.bias")
SHAPES = [(2, 5, 7), (3, 13, 17)]
KERNEL_SHAPES = [(2, 5, 7), (3, 5, 7), (3, 13, 17)]
CHANNELS = [1, 8, 1536]
SLAB_SHAPE = (3, 13, 17)
SLAB_PIXELS, MAX_SLABS = 512, 256                               # csrc/train_bn.hip, restated
BN_EPS, MOMENTUM = 1e-5, 0.1                                    # torch's defaults, the reference's
ZERO_GAMMA = (37, 1201)                                         # decoder_case: gamma1, gamma2 of these channels are 0
W1_SUBSET = (slice(None, None, 5), slice(None, None, 7))        # the strided part of W1's gradient the goldens keep
GH_SUBSET = slice(None, None, 7)                                # the channels of grad_h the goldens keep
WRONG_STATS = ("per_frame", "unbiased_norm", "last_slab", "last_pixel")
WRONG_RUNNING = ("biased_running", "momentum_swapped")
WRONG_BWD = ("no_dgamma_term", "no_dbeta_term")
WRONG_SUMS = ("last_slab", "last_pixel")
WRONG_DW = ("across_frames",)
ACT_NONE, ACT_RELU6, ACT_SIGMOID = None, "relu6", "sigmoid"


def name(shape):
    return "decoder_bn_T%d_%dx%d" % shape


def slab_partition(T, H, W):
    """The slabs of every reduction of csrc/train_bn.hip: `(rows per slab, slabs)` over the T * H picture rows."""
    rows = T * H
    sr = max(-(-SLAB_PIXELS // W), -(-rows // MAX_SLABS))
    return sr, -(-rows // sr)


# ------------------------------------------------------------------------------------------------ inputs (float32 numpy)
def bn_inputs(c, shape, ld=None, seed=0):
    """One BatchNorm's teacher-forced inputs: `u` `[T,H,W,ld]` (the kernels read its first `c` channels: pitched when ld > c)
    with a per-channel offset and spread, `g` like it, gamma, beta, running statistics.  The ReLU6 behind it is saturated
    tests/saturate_bn.py's way -- gamma times GAIN, beta plus SHIFT: pre-activations of mean 3 and spread 4 reach both clamps --
    and channel 0 of a c >= 8 case has gamma = 0, beta = 1.5 (a constant inside the open range)."""
    T, H, W = shape
    ld = ld or c
    rs = np.random.RandomState(9000 + 131 * c + 17 * T * H * W + seed)
    u = (rs.standard_normal((T, H, W, ld)) * (0.5 + rs.random_sample(ld)) + rs.standard_normal(ld)).astype(np.float32)
    g = (rs.standard_normal((T, H, W, ld)) / (T * H * W)).astype(np.float32)
    gamma = ((0.5 + rs.random_sample(c)) * rs.choice([-1.0, 1.0], c) * GAIN).astype(np.float32)
    beta = (0.5 * rs.standard_normal(c) + SHIFT).astype(np.float32)
    if c >= 8:
        gamma[0], beta[0] = 0.0, 1.5
    return {"u": u, "g": g, "gamma": gamma, "beta": beta, "rm": rs.standard_normal(c).astype(np.float32),
            "rv": (0.5 + rs.random_sample(c)).astype(np.float32)}


def decoder_case(shape, zero_gamma=True, seed=0):
    """`(h [T,256,H,W] uniform in [0, 3), q, gy [T,1,H,W])`, float32 numpy: the decoder's MODULE numbers q = {w1, wd, w3, g*,
    be*, rm*, rv*} (* = 1, 2, 3).  In training mode a BatchNorm normalises whatever it is handed, so gamma = 3 and beta =
    1.5 + N(0, 1) give both ReLU6s pre-activations of spread 3 around 1.5 on any data: both clamps hold a sizeable share
    (asserted by the CPU test); the logits have spread 1.5.  The running statistics are not the initial 0 and 1."""
    T, H, W = shape
    rs = np.random.RandomState(7100 + T * H * W + seed)
    h = (3.0 * rs.random_sample((T, C_IN, H, W))).astype(np.float32)
    gy = (rs.standard_normal((T, 1, H, W)) / (H * W)).astype(np.float32)
    q = {"w1": (rs.standard_normal((HID, C_IN, 1, 1)) * math.sqrt(2.0 / HID)).astype(np.float32),
         "wd": (rs.standard_normal((HID, 1, 3, 3)) * math.sqrt(2.0 / (HID * 9))).astype(np.float32),
         "w3": (rs.standard_normal((1, HID, 1, 1)) * math.sqrt(2.0)).astype(np.float32)}
    for i, n in ((1, HID), (2, HID), (3, 1)):
        q["g%d" % i] = np.full(n, 3.0 if i < 3 else 1.5, np.float32) * rs.choice([-1.0, 1.0], n).astype(np.float32)
        q["be%d" % i] = (1.5 + rs.standard_normal(n)).astype(np.float32) if i < 3 else np.zeros(n, np.float32)
        q["rm%d" % i] = (0.1 * rs.standard_normal(n)).astype(np.float32)
        q["rv%d" % i] = (0.5 + rs.random_sample(n)).astype(np.float32)
    if zero_gamma:
        for i, c in ((1, ZERO_GAMMA[0]), (2, ZERO_GAMMA[1])):
            q["g%d" % i][c] = 0.0
            q["be%d" % i][c] = 1.5
    return h, q, gy


def load_block(block, q):
    """Put `decoder_case`'s numbers into a dwBlock(256, 1) (the package's or the reference's) and switch it to TRAINING mode."""
    seq = block.conv
    with torch.no_grad():
        for conv, k in ((seq[0][0], "w1"), (seq[1][0], "wd"), (seq[2], "w3")):
            conv.weight.copy_(torch.as_tensor(q[k]))
        for i, bn in ((1, seq[0][1]), (2, seq[1][1]), (3, seq[3])):
            bn.weight.copy_(torch.as_tensor(q["g%d" % i]))
            bn.bias.copy_(torch.as_tensor(q["be%d" % i]))
            bn.running_mean.copy_(torch.as_tensor(q["rm%d" % i]))
            bn.running_var.copy_(torch.as_tensor(q["rv%d" % i]))
            bn.eps, bn.momentum = BN_EPS, MOMENTUM
            bn.num_batches_tracked.zero_()
    return block.train()


def to64(d, device="cpu"):
    return {k: torch.as_tensor(v).to(device=device, dtype=torch.float64) for k, v in d.items()}


# ------------------------------------------------------------------------------------------------ the stages (NHWC float64)
def _pixel_weights(u, variant):
    """1 for every pixel a correct kernel counts; a WRONG kernel drops the last slab or the last pixel."""
    T, H, W, _ = u.shape
    wt = torch.ones(T * H, W, dtype=u.dtype, device=u.device)
    if variant == "last_slab":
        sr, slabs = slab_partition(T, H, W)
        wt[(slabs - 1) * sr:] = 0
    if variant == "last_pixel":
        wt[-1, -1] = 0
    return wt.view(T, H, W, 1)


def stats(u, gamma, beta, eps=BN_EPS, variant=None, bounds=False):
    """`uavsal_bn_stats` without the running update: dict(mu, var, r, s, b), each `[C]`; `bounds`: `(f, bounds)`.  `variant`:
    one of WRONG_STATS.  (per_frame: the statistics of frame 0 alone stand for the batch's.)"""
    x = u[:1] if variant == "per_frame" else u
    wt = _pixel_weights(x, variant)
    P = x.shape[0] * x.shape[1] * x.shape[2]
    mu = (x * wt).sum((0, 1, 2)) / P
    var = (x * x * wt).sum((0, 1, 2)) / P - mu * mu
    vn = var * P / (P - 1) if variant == "unbiased_norm" else var
    r = 1.0 / torch.sqrt(vn + eps)
    s = gamma * r
    f = {"mu": mu, "var": var, "r": r, "s": s, "b": beta - mu * s}
    if not bounds:
        return f
    e_mu = P * D * u.abs().mean((0, 1, 2))
    e_var = P * D * (u * u).mean((0, 1, 2)) + 2 * mu.abs() * e_mu + e_mu * e_mu
    dr = 0.5 * r ** 3 * e_var
    one = U + DS
    b = {"mu": one * mu.abs() + e_mu, "var": one * var + e_var, "r": one * r + dr, "s": one * s.abs() + gamma.abs() * dr,
         "b": one * (beta.abs() + (mu * s).abs()) + s.abs() * e_mu + (mu * gamma).abs() * dr}
    return f, b


def running(rm, rv, mu, var, P, momentum=MOMENTUM, variant=None):
    """The running statistics after one step (float64; the tests round them to fp32).  `variant`: one of WRONG_RUNNING."""
    m = 1.0 - momentum if variant == "momentum_swapped" else momentum
    vu = var if variant == "biased_running" else var * P / (P - 1)
    return (1 - m) * rm + m * mu, (1 - m) * rv + m * vu


def _activate(a, act):
    return a.clamp(0, 6) if act == ACT_RELU6 else torch.sigmoid(a) if act == ACT_SIGMOID else a


def _act_err(a, act):
    """the error of the device's act(fma(u, s, b)) against the float64 one"""
    if act == ACT_RELU6:
        return U * a.abs().clamp(max=6.0) * (1 + U)
    if act == ACT_SIGMOID:
        y = torch.sigmoid(a)
        return U * a.abs() * y * (1 - y) + 4 * U * y
    return U * a.abs()


def apply(u, f, act):
    """`uavsal_bn_apply` from the device's fold `f` (its fp32 s, b as float64): `(out, bound)`."""
    a = u * f["s"] + f["b"]
    return _activate(a, act), _act_err(a, act)


def apply_dot(u, f, w, act=ACT_RELU6):
    """`uavsal_bn_apply` with `dot_w`: `(out [T,H,W,1], bound)`."""
    a = u * f["s"] + f["b"]
    d = _activate(a, act)
    c = u.shape[-1]
    out = (d * w).sum(-1, keepdim=True)
    bound = (c / 64 + 6) * U * (d.abs() * w.abs()).sum(-1, keepdim=True) + (_act_err(a, act) * w.abs()).sum(-1, keepdim=True)
    return out, bound


def _g_a(g, u, f, act, mask):
    """`(g, g_a, err(g_a), a)`; `g` a tensor like `u` or the rank-one tuple `(g_pix [T,H,W,1], g_chan [C])`."""
    a = u * f["s"] + f["b"]
    eg = 0.0
    if isinstance(g, tuple):
        g = g[0] * g[1]
        eg = U * g.abs()
    if act == ACT_RELU6:
        m = (((a > 0) & (a < 6)) if mask is None else mask).to(u.dtype)
        return g, g * m, eg * m, a
    if act == ACT_SIGMOID:
        y = torch.sigmoid(a)
        return g, g * y * (1 - y), eg * y * (1 - y) + g.abs() * (_act_err(a, act) * (1 - 2 * y).abs() + 2 * U * y * (1 - y)), a
    return g, g, eg + 0 * g, a


def bwd_sums(g, u, f, act, mask=None, variant=None, bounds=False):
    """`uavsal_bn_bwd_sums` from the device's fold: `[2, C]` (d beta, d gamma), or `[3, C]` for a rank-one `g` (+ the
    projection's weight gradient); `bounds`: `(sums, bound of the double sums, bound of the fp32 outputs)`."""
    wt = _pixel_weights(u, variant if variant in WRONG_SUMS else None)
    gp = g[0] if isinstance(g, tuple) else None
    _, ga, ega, a = _g_a(g, u, f, act, mask)
    xh = (u - f["mu"]) * f["r"]
    rows = [(ga * wt).sum((0, 1, 2)), (ga * xh * wt).sum((0, 1, 2))]
    if gp is not None:
        rows.append((gp * _activate(a, act) * wt).sum((0, 1, 2)))
    S = torch.stack(rows)
    if not bounds:
        return S
    P = u.shape[0] * u.shape[1] * u.shape[2]
    eb = [(ega + P * D * ga.abs()).sum((0, 1, 2)), ((ega + (2 * U + P * D) * ga.abs()) * xh.abs()).sum((0, 1, 2))]
    if gp is not None:
        eb.append((gp.abs() * (_act_err(a, act) + P * D * _activate(a, act).abs())).sum((0, 1, 2)))
    eb = torch.stack(eb)
    return S, eb, eb + U * S.abs()


def bwd_apply(g, u, f, sums, act, mask=None, variant=None, bounds=False, sums_err=None):
    """`uavsal_bn_bwd_apply` from the device's fold and the device's `sums` (`[2, C]` float64): `g_u` like `u`.  `variant`: one
    of WRONG_BWD (no_dgamma_term is the EVAL-mode gradient with the mean term kept: what this feature exists to correct).
    `sums_err` (`[2, C]`): `sums` are the float64 ones, not the device's, and the device's lie that close (the bound of
    `bwd_sums`): the bound grows by |s| (err(S0) + |xh| err(S1)) / P."""
    P = u.shape[0] * u.shape[1] * u.shape[2]
    _, ga, ega, _ = _g_a(g, u, f, act, mask)
    xh = (u - f["mu"]) * f["r"]
    c1 = 0 * sums[0] if variant == "no_dbeta_term" else sums[0] / P
    c2 = 0 * sums[1] if variant == "no_dgamma_term" else sums[1] / P
    gu = f["s"] * (ga - c1 - xh * c2)
    if not bounds:
        return gu
    A = ga.abs() + c1.abs() + (xh * c2).abs()
    extra = 0.0 if sums_err is None else (sums_err[0] + xh.abs() * sums_err[1]) / P
    return gu, f["s"].abs() * (ega + 5 * U * A + extra)


def _tap_sums(a, b, across_frames=False):
    """NHWC a, b -> [C, 3, 3]: sum over frames and pixels of a[t, y, x, c] b[t, y + ky - 1, x + kx - 1, c], zero outside the
    picture.  `across_frames` (a WRONG kernel): the frames are one tall picture, a border row sees the neighbouring frame."""
    T, H, W, c = a.shape
    if across_frames:
        a, b = a.reshape(1, T * H, W, c), b.reshape(1, T * H, W, c)
    bp = F.pad(b, (0, 0, 1, 1, 1, 1))
    hh = a.shape[1]
    out = a.new_zeros((c, 3, 3))
    for ky in range(3):
        for kx in range(3):
            out[:, ky, kx] = (a * bp[:, ky:ky + hh, kx:kx + W]).sum((0, 1, 2))
    return out


def dw_wgrad(g, e, variant=None, bounds=False):
    """`uavsal_dw_wgrad`: `[C, 1, 3, 3]`."""
    c = g.shape[-1]
    S = _tap_sums(g, e, across_frames=variant == "across_frames")
    if not bounds:
        return S.view(c, 1, 3, 3)
    P = g.shape[0] * g.shape[1] * g.shape[2]
    return S.view(c, 1, 3, 3), (P * D * _tap_sums(g.abs(), e.abs()) + U * S.abs()).view(c, 1, 3, 3)


def dw_raw(x, wd, transpose=False):
    """The raw depthwise 3x3 (`wd` `[C,1,3,3]`) of NHWC `x`, or its transpose (the flipped taps): `(out, bound)`."""
    c = x.shape[-1]
    xs = x.permute(0, 3, 1, 2)
    w = wd.flip(2, 3) if transpose else wd
    out = F.conv2d(xs, w, padding=1, groups=c).permute(0, 2, 3, 1)
    B = F.conv2d(xs.abs(), w.abs(), padding=1, groups=c).permute(0, 2, 3, 1)
    return out, (3 * LAMBDA + 2) * U * B


def conv1x1(x, w, transpose=False):
    """`uavsal_conv_gemm` of NHWC `x` with the 1x1 weight `w` `[Co,Ci,1,1]` (or its transpose): `(out, bound)`."""
    m = w.reshape(w.shape[0], w.shape[1])
    m = m if transpose else m.t()
    out = x @ m
    return out, rtol("f32", m.shape[0]) * (x.abs() @ m.abs()) + EPS * out.abs()


def pix_gemm(a, b):
    """`uavsal_pix_gemm` with row_scale 1 on NHWC `a`, `b`: `(G [M,N], bound)` (decoder_ref64.pix_gemm_ref)."""
    n = a.shape[0] * a.shape[1] * a.shape[2]
    A, B = a.reshape(n, -1), b.reshape(n, -1)
    return A.T @ B, LAMBDA * U * math.sqrt(n) * (A.abs().T @ B.abs())


# ------------------------------------------------------------------------------------------------ the whole decoder
def decoder_train(q, h, gy, stats_variant=None, bwd_variant=None, dw_variant=None):
    """The decoder in training mode and its backward by the closed form of include/uavsal_hip.h, float64 throughout, from the
    MODULE's numbers `q` (float64 tensors), `h` `[T,256,H,W]`, `gy` `[T,1,H,W]`.  Returns a dict: y `[T,1,H,W]`, grad_h
    `[T,256,H,W]`, the nine gradients under NAMES, mu1..3 / var1..3 (batch mean, biased variance), rm1..3 / rv1..3 (the running
    statistics after the step), and the NHWC intermediates u1, e, u2, u3, g_u1, g_u2, g_u3, g_e.  The variants reach every
    BatchNorm (`stats`, `bwd_apply`) or the depthwise weight gradient."""
    hn, gyn = h.permute(0, 2, 3, 1), gy.permute(0, 2, 3, 1)
    T, H, W, _ = hn.shape
    P = T * H * W
    w3 = q["w3"].reshape(-1)
    u1, _ = conv1x1(hn, q["w1"])
    f1 = stats(u1, q["g1"], q["be1"], variant=stats_variant)
    e, _ = apply(u1, f1, ACT_RELU6)
    u2, _ = dw_raw(e, q["wd"])
    f2 = stats(u2, q["g2"], q["be2"], variant=stats_variant)
    u3, _ = apply_dot(u2, f2, w3)
    f3 = stats(u3, q["g3"], q["be3"], variant=stats_variant)
    y, _ = apply(u3, f3, ACT_SIGMOID)
    s3 = bwd_sums(gyn, u3, f3, ACT_SIGMOID)
    g_u3 = bwd_apply(gyn, u3, f3, s3, ACT_SIGMOID, variant=bwd_variant)
    s2 = bwd_sums((g_u3, w3), u2, f2, ACT_RELU6)
    g_u2 = bwd_apply((g_u3, w3), u2, f2, s2, ACT_RELU6, variant=bwd_variant)
    g_wd = dw_wgrad(g_u2, e, variant=dw_variant)
    g_e, _ = dw_raw(g_u2, q["wd"], transpose=True)
    s1 = bwd_sums(g_e, u1, f1, ACT_RELU6)
    g_u1 = bwd_apply(g_e, u1, f1, s1, ACT_RELU6, variant=bwd_variant)
    G1, _ = pix_gemm(g_u1, hn)
    gh, _ = conv1x1(g_u1, q["w1"], transpose=True)
    out = {"y": y.permute(0, 3, 1, 2), "grad_h": gh.permute(0, 3, 1, 2),
           NAMES[0]: G1.view(HID, C_IN, 1, 1), NAMES[1]: s1[1], NAMES[2]: s1[0], NAMES[3]: g_wd, NAMES[4]: s2[1], NAMES[5]: s2[0],
           NAMES[6]: s2[2].view(1, HID, 1, 1), NAMES[7]: s3[1], NAMES[8]: s3[0],
           "u1": u1, "e": e, "u2": u2, "u3": u3, "g_u1": g_u1, "g_u2": g_u2, "g_u3": g_u3, "g_e": g_e}
    for i, f in ((1, f1), (2, f2), (3, f3)):
        out["mu%d" % i], out["var%d" % i] = f["mu"], f["var"]
        out["rm%d" % i], out["rv%d" % i] = running(q["rm%d" % i], q["rv%d" % i], f["mu"], f["var"], P)
    return out


def decoder_autograd(q, h, gy):
    """torch's own `F.batch_norm(training=True)` and autograd in double, from the module's numbers: y, grad_h, the nine
    gradients under NAMES, and rm1..3 / rv1..3 as torch moved them."""
    keys = ("w1", "g1", "be1", "wd", "g2", "be2", "w3", "g3", "be3")
    leaves = {k: q[k].detach().clone().requires_grad_(True) for k in keys}
    hh = h.detach().clone().requires_grad_(True)
    run = {k: q[k].detach().clone() for k in q if k[:2] in ("rm", "rv")}

    def bn(x, i):
        return F.batch_norm(x, run["rm%d" % i], run["rv%d" % i], leaves["g%d" % i], leaves["be%d" % i], True, MOMENTUM, BN_EPS)
    e = F.relu6(bn(F.conv2d(hh, leaves["w1"]), 1))
    d = F.relu6(bn(F.conv2d(e, leaves["wd"], padding=1, groups=HID), 2))
    y = torch.sigmoid(bn(F.conv2d(d, leaves["w3"]), 3))
    gs = torch.autograd.grad(y, [leaves[k] for k in keys] + [hh], gy)
    out = dict(zip(NAMES, gs[:9]))
    out.update(y=y.detach(), grad_h=gs[9], **run)
    return out


def clamp_shares(t):
    """`(share at 0, share strictly inside, share at 6)` of a ReLU6 output."""
    n = t.numel()
    return float((t <= 0).sum()) / n, float(((t > 0) & (t < 6)).sum()) / n, float((t >= 6).sum()) / n
