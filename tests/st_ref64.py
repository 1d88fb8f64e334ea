"""Float64 restatement of an ST block (reference model.py:163-249), of the closed-form gradients its backward on the device
computes (train.st_block_backward, csrc/train_st.hip), and of per-tensor error bounds.

    x_sp = spconv(x);  r = ReLU6(BN(W_r x));  dif = tdiff(r);  t1 = sub_conv(dif);  a_te = ReLU6(BN(W_l t1));
    o = ReLU6(BN(W_last (x_sp + a_te)));  out = x + o

Everything here is TEACHER-FORCED: a stage's gradients are formed in float64 from the fp32 tensors the device stored (its
input, its own activation, the gradient that arrived), so a bound only has to cover that stage's own arithmetic.

Bounds.  The rounding model of block_ref64 / nets_ref64: every fp32 rounding on the path costs at most U = 2^-24 relative to
the magnitude it rounds, so an error is bounded by (number of roundings) x U x (the sum of the ABSOLUTE terms).
  * tdiff_bwd: at most six terms added in double, one rounding: U sum|terms| (+ U again: the double sum is not exact).
  * gp = g m6(y): no arithmetic -- compared bit for bit.  beta = S: double accumulation, one rounding: 2 U sum|gp|.
  * G[c][j] = sum_p gp[p][c] x[p][j] (uavsal_pix_gemm): an fp32 fused chain of at most GEMM_CHAIN products (one rounding per
    product added: the n-th partial sum is rounded n times at most), the chains of a share added in fp32 (one rounding per
    chain), the shares in double: (min(K, GEMM_CHAIN) + ceil(K / GEMM_CHAIN) + 1) U A, A = sum_p |gp||x|.  This is the worst
    case, not a statistical estimate: nothing measured enters it.
  * W: s G rounded once, s itself the fp32 fold (one rounding): the bound of G times |s|, + 2 U |s| A.
  * gamma = r (sum_j W G - mu S) from the unrounded sums in double, r rounded once, the result rounded once:
    |r| (sum_j |W| bound(G) + 3 U (sum_j |W| A + |mu| sum|gp|)).
  * grad_x = gp . (diag(s) W): one fp32 GEMM over C channels whose weights fl(s W) are rounded once (s: once more):
    (C + 3) U sum_c |gp| |s W| (+ U |res| when a tensor is added in the epilogue).
  * a dwBlock's nine gradients from the stored x, e, d, gd, ga, go: the same two GEMM bounds for W1 and W3; S and Gd are
    double sums of fp32 products formed in double (one rounding at the end: 2 U sum|terms|).

`WRONG`: plausible bad kernels; the tests demand that each is at least 4 bounds away from the truth on some case, so that a
pass means something."""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
GEMM_CHAIN = 1024
GEMM_TARGET_WGS = 1024
SLAB_PIXELS, MAX_SLABS = 512, 256
BN_EPS = 1e-5
WRONG = ("interior_at_first", "interior_at_last", "cross_border", "nonstrict_masks", "mask_post_residual", "no_mu_term",
         "s_twice", "last_tile_skipped", "no_residual")
TDIFF_WRONG = WRONG[:4]
CBR_WRONG = ("nonstrict_masks", "mask_post_residual", "no_mu_term", "s_twice", "last_tile_skipped")
CBR_SHAPES = {"reduce_conv": (256, 32), "last_conv": (32, 256), "stconv_last": (256, 256)}      # name: (Cin, Cout)
PICTURES = [(1, 1, 1), (1, 5, 7), (2, 9, 13), (1, 45, 80), (3, 45, 80)]
TDIFF_CASES = [(2, 2), (3, 3), (5, 5), (4, 2), (6, 3)]                                         # (N, seq_len)
GEMM32_SHAPES = [(32, 256), (256, 32), (32, 384)]
GEMM32_K = [1, 35, 234, 3600, 10800]


def m6(v, strict=True):
    return ((v > 0) & (v < 6)) if strict else ((v >= 0) & (v <= 6))


# ------------------------------------------------------------------------------------------------ partitions, restated
def slab_partition(n_img, H, W):
    """`(rows per slab, slabs)` of uavsal_cbr_sums: the rule of uavsal_ir_sums."""
    rows = n_img * H
    sr = max(-(-SLAB_PIXELS // W), -(-rows // MAX_SLABS))
    return sr, -(-rows // sr)


def gemm32_partition(K, M, N):
    """`(cps, shares)` of uavsal_pix_gemm with a 32-wide side: ceil((M / 32)(N / 32) / 4) workgroups per share."""
    wgs = -(-(M // 32) * (N // 32) // 4)
    chunks = -(-K // GEMM_CHAIN)
    most = max(1, min(GEMM_TARGET_WGS // wgs, chunks))
    cps = -(-chunks // most)
    return cps, -(-chunks // cps)


def gemm_n_eff(K):
    return min(K, GEMM_CHAIN) + -(-K // GEMM_CHAIN) + 1


# ------------------------------------------------------------------------------------------------ temporal difference
def tdiff(r, L):
    """`r` [N,h,w,C] -> [N,h,w,2C] (reference model.py:190-200), sequences of L frames."""
    out = []
    for n in range(r.shape[0]):
        j, b = n % L, n - n % L
        if j == 0:
            out.append(torch.cat([r[n + 1] - r[n], r[n] - r[n + 1]], -1))
        elif j == L - 1:
            out.append(torch.cat([r[n] - r[n - 1], r[n - 1] - r[n]], -1))
        else:
            out.append(torch.cat([r[n] - r[n - 1], r[n] - r[n + 1]], -1))
        assert b <= n - (1 if j else 0) and n + (1 if j < L - 1 else 0) < b + L
    return torch.stack(out)


def tdiff_bwd(g, r, L, variant=None, absolute=False):
    """The adjoint of `tdiff` times m6(r): `g` [N,h,w,2C], `r` [N,h,w,C] float64.  `absolute`: the sum of the absolute terms
    (the bound's magnitude).  Variants: the interior rule used at the first / last frame of a sequence, differences that cross
    a sequence border (the whole call taken as one sequence), a non-strict mask."""
    N, C = r.shape[0], r.shape[-1]
    if variant == "cross_border":
        L = N
    P, Q = g[..., :C], g[..., C:]
    out = torch.zeros_like(r)

    def add(n, t, sign):
        out[n] += t.abs() if absolute else sign * t
    for n in range(N):
        j = n % L
        first, last = j == 0, j == L - 1
        if first and variant != "interior_at_first":
            add(n, P[n], -1), add(n, Q[n], 1)
        elif last and variant != "interior_at_last":
            add(n, P[n], 1), add(n, Q[n], -1)
        else:
            add(n, P[n], 1), add(n, Q[n], 1)
        if j >= 1:
            if j - 1 == 0 and variant != "interior_at_first":
                add(n, P[n - 1], 1), add(n, Q[n - 1], -1)
            else:
                add(n, Q[n - 1], -1)
        if j <= L - 2:
            if j + 1 == L - 1 and variant != "interior_at_last":
                add(n, P[n + 1], -1), add(n, Q[n + 1], 1)
            else:
                add(n, P[n + 1], -1)
    return out * m6(r, strict=variant != "nonstrict_masks")


def tdiff_bwd_bound(g, r, L):
    return 2 * U * tdiff_bwd(g, r, L, absolute=True)


# ------------------------------------------------------------------------------------------------ conv + BN + ReLU6
def bn_fold(gamma, beta, mean, var, eps=BN_EPS):
    """float64 `(s, b, r)` of an eval BatchNorm."""
    r = 1.0 / torch.sqrt(var.double() + eps)
    s = gamma.double() * r
    return s, beta.double() - mean.double() * s, r


def cbr_grads(x, y, g, W, gamma, mean, var, res=None, gres=None, variant=None, bounds=False):
    """The gradients of y = ReLU6(s (W x) + b) from stored tensors: `x` [P,Cin], `y` [P,C] (the stage's own activation), `g`
    [P,C] = d loss / d output, `W` [C,Cin], all float64 (P pixels).  `res` [P,C]: what the forward added to y afterwards
    (only the variant "mask_post_residual" looks at it); `gres` [P,Cin]: what the device's grad_x GEMM adds.  Returns
    dict(gp, W, gamma, beta, x) and, with `bounds`, the dict of their bounds."""
    s, _, r = bn_fold(gamma, gamma, mean, var)
    mu = mean.double()
    ym = y + res if (variant == "mask_post_residual" and res is not None) else y
    gp = g * m6(ym, strict=variant != "nonstrict_masks")
    S = gp.sum(0)
    G = gp.t() @ x
    Gw = G.clone()
    if variant == "last_tile_skipped":
        Gw[:, -32:] = 0
    gW = (s * s if variant == "s_twice" else s).view(-1, 1) * Gw
    ggamma = r * ((W * Gw).sum(1) - (0 if variant == "no_mu_term" else mu * S))
    gx = gp @ (s.view(-1, 1) * W)
    if gres is not None:
        gx = gx + gres
    out = {"gp": gp, "W": gW, "gamma": ggamma, "beta": S, "x": gx}
    if not bounds:
        return out
    K, C = gp.shape
    A = gp.abs().t() @ x.abs()
    aS = gp.abs().sum(0)
    eG = gemm_n_eff(K) * U * A
    b = {"W": s.abs().view(-1, 1) * (eG + 2 * U * A),
         "gamma": r.abs() * ((W.abs() * eG).sum(1) + 3 * U * ((W.abs() * A).sum(1) + mu.abs() * aS)),
         "beta": 2 * U * aS,
         "x": (C + 3) * U * (gp.abs() @ (s.abs().view(-1, 1) * W.abs())) + (U * (gx.abs() + gres.abs()) if gres is not None else 0)}
    return out, b


# ------------------------------------------------------------------------------------------------ a dwBlock, teacher-forced
def tap_sums(d2, e):
    """Gd[c][ky][kx] = sum over pixels of d2[n][y][x][c] e[n][y-1+ky][x-1+kx][c] (zero outside); NHWC float64."""
    N, H, W, C = e.shape
    ep = F.pad(e, (0, 0, 1, 1, 1, 1))
    return torch.stack([torch.stack([(d2 * ep[:, ky:ky + H, kx:kx + W]).sum((0, 1, 2)) for kx in range(3)], -1)
                        for ky in range(3)], -2)


def block_grads(x, e, d, gd, ga, go, w1, wd, w3, bn1, bn2, bn3, variant=None):
    """The nine gradients of an inverted-residual block (stride 1) from the stored NHWC float64 tensors, keyed like
    train.BLOCK_PARAMS' order (W1, gamma1, beta1, Wd, gamma2, beta2, W3, gamma3, beta3), and their bounds.  bn* =
    (gamma, mean, var).  `variant` "last_tile_skipped": the last 32 columns of the W3 product are never written."""
    K = x.shape[0] * x.shape[1] * x.shape[2]
    fl = lambda t: t.reshape(K, -1)                                       # noqa: E731
    (s1, _, r1), (s2, _, r2), (s3, _, r3) = (bn_fold(b[0], b[0], b[1], b[2]) for b in (bn1, bn2, bn3))
    mu1, mu2, mu3 = (b[1].double() for b in (bn1, bn2, bn3))
    d2 = gd * m6(d)
    G1, A1 = fl(ga).t() @ fl(x), fl(ga).abs().t() @ fl(x).abs()
    G3, A3 = fl(go).t() @ fl(d), fl(go).abs().t() @ fl(d).abs()
    if variant == "last_tile_skipped":
        G3 = G3.clone()
        G3[:, -32:] = 0
    S1, S2, S3 = fl(ga).sum(0), fl(d2).sum(0), fl(go).sum(0)
    aS1, aS2, aS3 = fl(ga).abs().sum(0), fl(d2).abs().sum(0), fl(go).abs().sum(0)
    Gd, aGd = tap_sums(d2, e), tap_sums(d2.abs(), e.abs())
    w1m, w3m, wdm = w1.reshape(w1.shape[0], -1), w3.reshape(w3.shape[0], -1), wd.reshape(-1, 3, 3)
    n = gemm_n_eff(K)
    eG1, eG3 = n * U * A1, n * U * A3
    g = [s1.view(-1, 1) * G1, r1 * ((w1m * G1).sum(1) - mu1 * S1), S1,
         s2.view(-1, 1, 1) * Gd, r2 * ((wdm * Gd).sum((1, 2)) - mu2 * S2), S2,
         s3.view(-1, 1) * G3, r3 * ((w3m * G3).sum(1) - mu3 * S3), S3]
    b = [s1.abs().view(-1, 1) * (eG1 + 2 * U * A1), r1.abs() * ((w1m.abs() * eG1).sum(1) + 3 * U * ((w1m.abs() * A1).sum(1) + mu1.abs() * aS1)),
         2 * U * aS1,
         4 * U * s2.abs().view(-1, 1, 1) * aGd, r2.abs() * 5 * U * ((wdm.abs() * aGd).sum((1, 2)) + mu2.abs() * aS2), 2 * U * aS2,
         s3.abs().view(-1, 1) * (eG3 + 2 * U * A3), r3.abs() * ((w3m.abs() * eG3).sum(1) + 3 * U * ((w3m.abs() * A3).sum(1) + mu3.abs() * aS3)),
         2 * U * aS3]
    return g, b


# ------------------------------------------------------------------------------------------------ the whole block, autograd
def _cbr(x, W, bn):
    s, b, _ = bn_fold(*bn)
    return (F.conv2d(x, W) * s.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)).clamp(0, 6)


def _dw(x, w1, wd, w3, bn1, bn2, bn3):
    e = _cbr(x, w1, bn1)
    s2, b2, _ = bn_fold(*bn2)
    d = (F.conv2d(e, wd, padding=1, groups=wd.shape[0]) * s2.view(1, -1, 1, 1) + b2.view(1, -1, 1, 1)).clamp(0, 6)
    s3, b3, _ = bn_fold(*bn3)
    return F.conv2d(d, w3) * s3.view(1, -1, 1, 1) + b3.view(1, -1, 1, 1)


def block_params64(block):
    """`{name: float64 leaf}` of the 27 parameters of an STBlock module and `{bn prefix: (mean, var)}` of its buffers."""
    return ({n: p.detach().double().cpu().clone().requires_grad_(True) for n, p in block.named_parameters()},
            {n: b.detach().double().cpu() for n, b in block.named_buffers() if not n.endswith("num_batches_tracked")})


def forward64(P, B, x, L):
    """The block in float64 from `block_params64`'s dicts; `x` [N,256,h,w]; returns the output (with autograd)."""
    def bn(prefix):
        return (P[prefix + ".weight"], P[prefix + ".bias"], B[prefix + ".running_mean"], B[prefix + ".running_var"])

    def dw(prefix, t):
        return _dw(t, P[prefix + ".0.0.weight"], P[prefix + ".1.0.weight"], P[prefix + ".2.weight"],
                   bn(prefix + ".0.1"), bn(prefix + ".1.1"), bn(prefix + ".3"))
    x_sp = dw("stconv_sp.spconv.conv", x)
    r = _cbr(x, P["stconv_te.reduce_conv.0.weight"], bn("stconv_te.reduce_conv.1"))
    dif = tdiff(r.permute(0, 2, 3, 1), L).permute(0, 3, 1, 2)
    t1 = dw("stconv_te.sub_conv.conv", dif)
    a_te = _cbr(t1, P["stconv_te.last_conv.0.weight"], bn("stconv_te.last_conv.1"))
    o = _cbr(x_sp + a_te, P["stconv_last.0.weight"], bn("stconv_last.1"))
    return x + o


def norm2(ts):
    return math.sqrt(sum(float((t.double() ** 2).sum()) for t in ts))


# ------------------------------------------------------------------------------------------------ the whole block, closed form
def backward64(P, B, x, go, L, variant=None):
    """The 27 gradients and grad_x of sum(go * block(x)) from the CLOSED FORMS above (no autograd): a float64 forward that keeps
    every intermediate, then the walk of train.st_block_backward -- stconv_last, spconv, last_conv, sub_conv, `tdiff_bwd`,
    reduce_conv.  `P`, `B`: `block_params64`'s dicts (the leaves are only read); `x`, `go` [N,256,h,w] float64.  Returns
    `({name: gradient in the parameter's shape}, grad_x)`.  `variant` "no_residual": grad_x without the block's `+ x`."""
    P = {k: v.detach() for k, v in P.items()}
    nh = lambda t: t.permute(0, 2, 3, 1)                                  # noqa: E731
    fl = lambda t: nh(t).reshape(-1, t.shape[1])                          # noqa: E731

    def bn(prefix):
        return (P[prefix + ".weight"], P[prefix + ".bias"], B[prefix + ".running_mean"], B[prefix + ".running_var"])

    def dw_fwd(prefix, t):
        w1, wd, w3 = P[prefix + ".0.0.weight"], P[prefix + ".1.0.weight"], P[prefix + ".2.weight"]
        e = _cbr(t, w1, bn(prefix + ".0.1"))
        s2, b2, _ = bn_fold(*bn(prefix + ".1.1"))
        d = (F.conv2d(e, wd, padding=1, groups=wd.shape[0]) * s2.view(1, -1, 1, 1) + b2.view(1, -1, 1, 1)).clamp(0, 6)
        s3, b3, _ = bn_fold(*bn(prefix + ".3"))
        return e, d, F.conv2d(d, w3) * s3.view(1, -1, 1, 1) + b3.view(1, -1, 1, 1)

    def dw_bwd(prefix, t, e, d, g, out):
        """the block's nine gradients into `out`; returns its input gradient (no residual)"""
        w1, wd, w3 = P[prefix + ".0.0.weight"], P[prefix + ".1.0.weight"], P[prefix + ".2.weight"]
        s1 = bn_fold(*bn(prefix + ".0.1"))[0]
        s2 = bn_fold(*bn(prefix + ".1.1"))[0]
        s3 = bn_fold(*bn(prefix + ".3"))[0]
        gd = F.conv_transpose2d(g * s3.view(1, -1, 1, 1), w3)
        ga = F.conv_transpose2d(gd * m6(d), wd, padding=1, groups=wd.shape[0]) * s2.view(1, -1, 1, 1) * m6(e)
        b3 = lambda pre: (P[pre + ".weight"], B[pre + ".running_mean"], B[pre + ".running_var"])      # noqa: E731
        gs, _ = block_grads(nh(t), nh(e), nh(d), nh(gd), nh(ga), nh(g), w1, wd, w3, b3(prefix + ".0.1"), b3(prefix + ".1.1"),
                            b3(prefix + ".3"))
        names = (".0.0.weight", ".0.1.weight", ".0.1.bias", ".1.0.weight", ".1.1.weight", ".1.1.bias", ".2.weight", ".3.weight", ".3.bias")
        for n, v in zip(names, gs):
            out[prefix + n] = v.reshape(P[prefix + n].shape)
        return F.conv_transpose2d(ga * s1.view(1, -1, 1, 1), w1)

    def cbr_bwd(prefix, t, y, g, out):
        W = P[prefix + ".0.weight"]
        r = cbr_grads(fl(t), fl(y), fl(g), W.reshape(W.shape[0], -1), P[prefix + ".1.weight"], B[prefix + ".1.running_mean"],
                      B[prefix + ".1.running_var"])
        out[prefix + ".0.weight"], out[prefix + ".1.weight"], out[prefix + ".1.bias"] = r["W"].reshape(W.shape), r["gamma"], r["beta"]
        return r["x"].reshape(t.shape[0], t.shape[2], t.shape[3], -1).permute(0, 3, 1, 2), r["gp"]
    x = x.detach()
    e_sp, d_sp, x_sp = dw_fwd("stconv_sp.spconv.conv", x)
    r = _cbr(x, P["stconv_te.reduce_conv.0.weight"], bn("stconv_te.reduce_conv.1"))
    dif = tdiff(nh(r), L).permute(0, 3, 1, 2)
    e_te, d_te, t1 = dw_fwd("stconv_te.sub_conv.conv", dif)
    a_te = _cbr(t1, P["stconv_te.last_conv.0.weight"], bn("stconv_te.last_conv.1"))
    ssum = x_sp + a_te
    o = _cbr(ssum, P["stconv_last.0.weight"], bn("stconv_last.1"))
    out = {}
    g_sum, _ = cbr_bwd("stconv_last", ssum, o, go, out)
    gx_sp = dw_bwd("stconv_sp.spconv.conv", x, e_sp, d_sp, g_sum, out)
    g_t1, _ = cbr_bwd("stconv_te.last_conv", t1, a_te, g_sum, out)
    g_dif = dw_bwd("stconv_te.sub_conv.conv", dif, e_te, d_te, g_t1, out)
    gp_r = tdiff_bwd(nh(g_dif), nh(r), L).permute(0, 3, 1, 2)
    gx_red, _ = cbr_bwd("stconv_te.reduce_conv", x, r, gp_r, out)          # (the mask again: gp_r carries it already)
    gx = gx_sp + gx_red
    return out, gx if variant == "no_residual" else gx + go


# ------------------------------------------------------------------------------------------------ recorded reference results
# tests/golden/st_*.npz (tools/make_st_goldens.py): the reference's own STBlock under float64 autograd.  (N, h, w, L): L < N
# is N / L reference calls of L frames each -- the reference takes every call as one sequence
GOLDEN_CASES = [(2, 5, 7, 2), (5, 5, 7, 5), (6, 5, 7, 3)]
BIG = 4096                                                           # gradients with more elements are stored on W_SUBSET
W_SUBSET = (slice(None, None, 5), slice(None, None, 7))
GX_SUBSET = (slice(None), slice(None, None, 9), slice(None, None, 2), slice(None, None, 3))


def golden_name(case):
    return "st_N%d_%dx%d_L%d" % tuple(case)


def calibrate(blk, seed=3):
    """Seeded numbers into an STBlock module (the package's or the reference's: the same names): kaiming-scaled conv weights,
    and BatchNorms calibrated on a fixed population (float64, CPU) so that every ReLU6 stage sees pre-activations of mean about
    1.5 and spread about 3 -- all three ReLU6 classes in every masked tensor -- with running statistics and weights that are
    not the initial 0 and 1.  Returns `blk` in eval mode."""
    import numpy as np
    blk.eval()
    rs = np.random.RandomState(seed)
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, torch.nn.Conv2d):
                fan_out = m.weight.shape[0] * m.weight.shape[2] * m.weight.shape[3] // m.groups
                m.weight.copy_(torch.from_numpy(rs.standard_normal(tuple(m.weight.shape)) * math.sqrt(2.0 / fan_out)))
    x = torch.from_numpy(1.5 * rs.standard_normal((6, 256, 5, 7)))
    v = lambda t: t.double().view(1, -1, 1, 1)                            # noqa: E731

    def fix(bn, pre, mean, std):
        c = bn.weight.numel()
        with torch.no_grad():
            bn.running_mean.copy_(pre.mean((0, 2, 3)) + torch.from_numpy(0.1 * rs.standard_normal(c)) * pre.std((0, 2, 3)))
            bn.running_var.copy_(pre.var((0, 2, 3)).clamp_min(1e-8) * torch.from_numpy(0.8 + 0.4 * rs.random_sample(c)))
            bn.weight.copy_(std * torch.from_numpy(0.8 + 0.4 * rs.random_sample(c)))
            bn.bias.copy_(mean + torch.from_numpy(0.5 * rs.standard_normal(c)))
        return (pre - v(bn.running_mean)) / torch.sqrt(v(bn.running_var) + bn.eps) * v(bn.weight) + v(bn.bias)

    def cbr(m, t):
        return fix(m[1], F.conv2d(t, m[0].weight.detach().double()), 1.5, 3.0).clamp(0, 6)

    def dw(b, t):
        e = cbr(b.conv[0], t)
        d = fix(b.conv[1][1], F.conv2d(e, b.conv[1][0].weight.detach().double(), padding=1, groups=e.shape[1]), 1.5, 3.0).clamp(0, 6)
        return fix(b.conv[3], F.conv2d(d, b.conv[2].weight.detach().double()), 0.0, 1.5)
    te = blk.stconv_te
    x_sp = dw(blk.stconv_sp.spconv, x)
    r = cbr(te.reduce_conv, x)
    t1 = dw(te.sub_conv, tdiff(r.permute(0, 2, 3, 1), 3).permute(0, 3, 1, 2))
    cbr(blk.stconv_last, x_sp + cbr(te.last_conv, t1))
    return blk


def golden_inputs(case):
    """`(x, go)` float32 numpy [N,256,h,w] of a golden case."""
    import numpy as np
    N, h, w, L = case
    rs = np.random.RandomState(7000 + N * h * w + L)
    return ((1.5 * rs.standard_normal((N, 256, h, w))).astype(np.float32),
            (rs.standard_normal((N, 256, h, w)) / (h * w)).astype(np.float32))


def golden_digest(blk, x, go):
    """sha256 over the block's parameters and buffers (fp32 bytes, state_dict order) and the inputs."""
    import hashlib
    h = hashlib.sha256()
    for k, t in blk.state_dict().items():
        if not k.endswith("num_batches_tracked"):
            h.update(k.encode())
            h.update(t.detach().float().cpu().numpy().tobytes())
    h.update(x.tobytes())
    h.update(go.tobytes())
    return h.hexdigest()


def golden_pack(grads, gx):
    """What a golden file keeps of `{name: float64 gradient}` and grad_x: the small gradients whole, the big 1x1 weight
    gradients on W_SUBSET plus sum and L2 norm, grad_x on GX_SUBSET."""
    out = {"grad_x": gx[GX_SUBSET]}
    for n, g in grads.items():
        key = n.replace(".", "_")
        if g.size > BIG:
            m = g.reshape(g.shape[0], -1)
            out.update({key: m[W_SUBSET], key + "__sum": m.sum(), key + "__l2": (m * m).sum() ** 0.5})
        else:
            out[key] = g
    return out
