"""Float64 restatement of the SRF-Net head (reference model.py:110-158, eval mode), of the closed-form gradients its backward
on the device computes (train.srf_head_backward, csrc/train_srf.hip), and of per-tensor error bounds.

    a1 = CBR(lv5_aspp1, c5);  a_b = BN(W3 ReLU6(BN(dw_dil(CBR(expand, c5)))))  (b = 2, 3, 4; dilation 6, 12, 18)
    x5 = CBR(conv_lv5, cat[a1..a4]);  x4 = CBR(conv_lv4, c4);  x3 = CBR(conv_lv3, c3)
    y  = CBR3x3(conv_last, cat[up(x5), up(x4), x3])          (up: bilinear, align_corners=True, to the size of c3)

Everything is TEACHER-FORCED where a device tensor is compared: a stage's gradients are formed in float64 from the fp32
tensors the device stored, so a bound only has to cover that stage's own arithmetic.

Bounds: the rounding model of st_ref64 (U = 2^-24 per fp32 rounding, times the sum of the ABSOLUTE terms).
  * G[co][ci][ky][kx] (uavsal_conv3_wgrad): the chained GEMM over K = n H W pixels: st_ref64.gemm_n_eff(K) U A with
    A = sum |g| |x shifted|.  out = fl(s G): |s| (that + U A) for a given fp32 s, + U |s| A more when s is the fp32 fold.
    rowdot = sum w G from the unrounded sums in double: sum |w| bound(G).
  * ga (uavsal_ir_bwd_dil): nine fp32 products added in fp32 (at most one rounding per term added), the product with s2
    rounded once, s2 itself an fp32 fold (two roundings): 12 U |s2| sum_k |wd[k]| |delta2|.
  * S2, S1, S3, Gd (uavsal_ir_sums_dil): double sums of fp32 terms / products formed in double: 2 U sum |terms|; the
    gradients uavsal_ir_finish forms from them: st_ref64.block_grads' bounds with the dilated tap sums.

`WRONG`: plausible bad kernels.  The CPU tests demand that each is at least 4 bounds away from the truth on some case."""
import math

import torch
import torch.nn.functional as F

import st_ref64 as SR

U = SR.U
BN_EPS = SR.BN_EPS
m6 = SR.m6
gemm_n_eff = SR.gemm_n_eff
bn_fold = SR.bn_fold

CONV3_WRONG = ("kykx_swapped", "tap_flipped", "row_wrap", "frame_neighbour", "last_half_tile_skipped")
DIL_WRONG = ("dilation_1", "nonstrict_masks")
STAGE_WRONG = ("s_twice", "no_mu_term")
WRONG = CONV3_WRONG + DIL_WRONG + STAGE_WRONG

CONV3_SHAPES = [(128, 64), (128, 192), (256, 448)]                     # (Co, Ci)
CONV3_PICTURES = [(1, 1, 1), (1, 5, 7), (2, 9, 13), (3, 45, 80)]       # (n, H, W)
DIL_CASES = [(6, 5, 7), (6, 7, 13), (12, 12, 20), (18, 12, 20), (2, 9, 13)]   # (dil, H, W)
DIL_CH = (64, 192)
DIL_N = (1, 3)
GEMM_NEW_SHAPES = [(64, 32), (128, 96)]                                # uavsal_pix_gemm: conv_lv3, conv_lv4
GEMM_OLD_SHAPES = [(32, 256), (64, 64)]                                # one accepted shape of each kernel
HEAD = ("conv_lv3", "conv_lv4", "lv5_aspp1", "lv5_aspp2", "lv5_aspp3", "lv5_aspp4", "conv_lv5", "conv_last")
HEAD_BLOCKS = HEAD[3:6]
CBR_NAMES = ("0.weight", "1.weight", "1.bias")
BLOCK_NAMES = ("conv.0.0.weight", "conv.0.1.weight", "conv.0.1.bias", "conv.1.0.weight", "conv.1.1.weight", "conv.1.1.bias",
               "conv.2.weight", "conv.3.weight", "conv.3.bias")
HEAD_PARAMS = tuple("%s.%s" % (m, n) for m in HEAD for n in (BLOCK_NAMES if m in HEAD_BLOCKS else CBR_NAMES))
# (N, (h3, w3), (h4, w4), (h5, w5)): the taps of 72 x 224 frames (dilation 6 has live horizontal taps on the 3 x 7 map) and a
# small odd one whose 1/32 map is smaller than every dilation
GOLDEN_CASES = [(2, (9, 28), (5, 14), (3, 7)), (1, (5, 7), (3, 4), (2, 2))]
BIG = 4096
W_SUBSET = (slice(None, None, 13), slice(None, None, 17))


# ------------------------------------------------------------------------------------------------ partitions, restated
def conv3_partition(K, Co, Ci):
    """`(cps, shares)` of uavsal_conv3_wgrad: pixgemm::split over (Co / 128) * 9 * ceil(Ci / 128) tiles."""
    tiles = (Co // 128) * 9 * -(-Ci // 128)
    chunks = -(-K // SR.GEMM_CHAIN)
    most = max(1, min(SR.GEMM_TARGET_WGS // tiles, chunks))
    cps = -(-chunks // most)
    return cps, -(-chunks // cps)


slab_partition = SR.slab_partition                                    # uavsal_ir_sums_dil: the rule of uavsal_ir_sums


# ------------------------------------------------------------------------------------------------ dense 3x3 weight gradient
def _shift(x, dy, dx, variant=None):
    """x[n][y + dy][x + dx] (NHWC), zero outside the picture.  Variants: a row wrapping over the picture border (the shift
    taken in the row-major pixel index of the frame), a frame reading its neighbour (all frames one tall picture)."""
    N, H, W, C = x.shape
    if variant == "row_wrap":
        flat = x.reshape(N, H * W, C)
        out = torch.zeros_like(flat)
        s = dy * W + dx
        lo, hi = max(0, -s), min(H * W, H * W - s)
        if hi > lo:
            out[:, lo:hi] = flat[:, lo + s:hi + s]
        return out.reshape(N, H, W, C)
    if variant == "frame_neighbour":
        return _shift(x.reshape(1, N * H, W, C), dy, dx).reshape(N, H, W, C)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    return xp[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def conv3_wgrad(g, x, variant=None, absolute=False):
    """G[co][ci][ky][kx] = sum_p g[p][co] x[p + (ky-1, kx-1)][ci]; `g` [n,H,W,Co], `x` [n,H,W,Ci] float64 NHWC."""
    if absolute:
        g, x = g.abs(), x.abs()
    K, Co, Ci = g.shape[0] * g.shape[1] * g.shape[2], g.shape[3], x.shape[3]
    gm = g.reshape(K, Co).t()
    shift_variant = variant if variant in ("row_wrap", "frame_neighbour") else None
    G = torch.stack([torch.stack([gm @ _shift(x, ky - 1, kx - 1, shift_variant).reshape(K, Ci) for kx in range(3)], -1)
                     for ky in range(3)], -2)
    if variant == "kykx_swapped":
        G = G.transpose(2, 3).contiguous()
    if variant == "tap_flipped":
        G = G.flip(2, 3)
    if variant == "last_half_tile_skipped" and Ci % 128:
        G = G.clone()
        G[:, -64:] = 0
    return G


def conv3_wgrad_bound(g, x):
    K = g.shape[0] * g.shape[1] * g.shape[2]
    A = conv3_wgrad(g, x, absolute=True)
    return gemm_n_eff(K) * U * A, A


def cbr3_grads(x, y, g, W, gamma, mean, var, variant=None, bounds=False):
    """The gradients of y = ReLU6(s conv3x3(W, x) + b) from stored tensors: `x` [n,H,W,Ci], `y`, `g` [n,H,W,C] NHWC float64,
    `W` [C,Ci,3,3].  Returns dict(gp, W, gamma, beta, x) and, with `bounds`, the dict of their bounds (st_ref64.cbr_grads with
    the 3x3 products)."""
    s, _, r = bn_fold(gamma, gamma, mean, var)
    mu = mean.double()
    gp = g * m6(y, strict=variant != "nonstrict_masks")
    S = gp.sum((0, 1, 2))
    G = conv3_wgrad(gp, x, variant if variant in CONV3_WRONG else None)
    gW = (s * s if variant == "s_twice" else s).view(-1, 1, 1, 1) * G
    ggamma = r * ((W * G).sum((1, 2, 3)) - (0 if variant == "no_mu_term" else mu * S))
    sw = s.view(-1, 1, 1, 1) * W
    gx = F.conv_transpose2d(gp.permute(0, 3, 1, 2), sw, padding=1).permute(0, 2, 3, 1)
    out = {"gp": gp, "W": gW, "gamma": ggamma, "beta": S, "x": gx}
    if not bounds:
        return out
    eG, A = conv3_wgrad_bound(gp, x)
    aS = gp.abs().sum((0, 1, 2))
    C = gp.shape[3]
    b = {"W": s.abs().view(-1, 1, 1, 1) * (eG + 2 * U * A),
         "gamma": r.abs() * ((W.abs() * eG).sum((1, 2, 3)) + 3 * U * ((W.abs() * A).sum((1, 2, 3)) + mu.abs() * aS)),
         "beta": 2 * U * aS,
         "x": (9 * C + 3) * U * F.conv_transpose2d(gp.abs().permute(0, 3, 1, 2), sw.abs(), padding=1).permute(0, 2, 3, 1)}
    return out, b


# ------------------------------------------------------------------------------------------------ dilated depthwise backward
def _shift_dil(t, dy, dx):
    """t[n][y + dy][x + dx] (NHWC), zero outside the picture, for any shift."""
    N, H, W, C = t.shape
    out = torch.zeros_like(t)
    y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if y1 > y0 and x1 > x0:
        out[:, y0:y1, x0:x1] = t[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def ir_bwd_dil(gd, d, e, wd, s2, dil, variant=None, absolute=False):
    """ga[p][c] = m6(e) s2[c] sum_k wd[c][k] delta2[p - dil (k - (1,1))][c]; NHWC float64, `wd` [C,3,3], `s2` [C]."""
    strict = variant != "nonstrict_masks"
    dl = 1 if variant == "dilation_1" else dil
    d2 = gd * m6(d, strict)
    if absolute:
        d2, wd, s2 = d2.abs(), wd.abs(), s2.abs()
    acc = torch.zeros_like(d2)
    for ky in range(3):
        for kx in range(3):
            acc = acc + wd[:, ky, kx] * _shift_dil(d2, -dl * (ky - 1), -dl * (kx - 1))
    return acc * s2 * m6(e, strict)


def ir_bwd_dil_bound(gd, d, e, wd, s2, dil):
    return 12 * U * ir_bwd_dil(gd, d, e, wd, s2, dil, absolute=True)


def tap_sums_dil(d2, e, dil):
    """Gd[c][ky][kx] = sum over pixels of d2[p][c] e[p + dil (ky-1, kx-1)][c] (zero outside)."""
    return torch.stack([torch.stack([(d2 * _shift_dil(e, dil * (ky - 1), dil * (kx - 1))).sum((0, 1, 2)) for kx in range(3)], -1)
                        for ky in range(3)], -2)


def ir_sums_dil(gd, d, e, ga, go, dil, variant=None):
    """`(S2 [Ch], Gd [Ch,3,3], S1 [Ch], S3 [Co])` and the dict of their bounds."""
    dl = 1 if variant == "dilation_1" else dil
    d2 = gd * m6(d, variant != "nonstrict_masks")
    S2, S1, S3 = d2.sum((0, 1, 2)), ga.sum((0, 1, 2)), go.sum((0, 1, 2))
    Gd = tap_sums_dil(d2, e, dl)
    b = (2 * U * d2.abs().sum((0, 1, 2)), 2 * U * tap_sums_dil(d2.abs(), e.abs(), dl), 2 * U * ga.abs().sum((0, 1, 2)),
         2 * U * go.abs().sum((0, 1, 2)))
    return (S2, Gd, S1, S3), b


def block_grads_dil(x, e, d, gd, ga, go, w1, wd, w3, bn1, bn2, bn3, dil, variant=None):
    """st_ref64.block_grads for a block whose depthwise conv has dilation `dil`: the nine gradients (W1, gamma1, beta1, Wd,
    gamma2, beta2, W3, gamma3, beta3) from the stored NHWC float64 tensors, and their bounds."""
    g, b = SR.block_grads(x, e, d, gd, ga, go, w1, wd, w3, bn1, bn2, bn3)
    dl = 1 if variant == "dilation_1" else dil
    s2, _, r2 = bn_fold(bn2[0], bn2[0], bn2[1], bn2[2])
    mu2 = bn2[1].double()
    d2 = gd * m6(d, variant != "nonstrict_masks")
    Gd, aGd = tap_sums_dil(d2, e, dl), tap_sums_dil(d2.abs(), e.abs(), dl)
    S2, aS2 = d2.sum((0, 1, 2)), d2.abs().sum((0, 1, 2))
    wdm = wd.reshape(-1, 3, 3)
    g[3], g[4], g[5] = s2.view(-1, 1, 1) * Gd, r2 * ((wdm * Gd).sum((1, 2)) - mu2 * S2), S2
    b[3], b[4], b[5] = 4 * U * s2.abs().view(-1, 1, 1) * aGd, r2.abs() * 5 * U * ((wdm.abs() * aGd).sum((1, 2)) + mu2.abs() * aS2), 2 * U * aS2
    return g, b


# ------------------------------------------------------------------------------------------------ the whole head
def head_params64(sfnet):
    """`{name: float64 leaf}` of the head's 42 parameters and `{name: float64 buffer}` of its running statistics."""
    P = {n: p.detach().double().cpu().clone().requires_grad_(True) for n, p in sfnet.named_parameters() if n in HEAD_PARAMS}
    B = {n: b.detach().double().cpu() for n, b in sfnet.named_buffers()
         if n.split(".")[0] in HEAD and not n.endswith("num_batches_tracked")}
    return P, B


def _bn(P, B, prefix):
    return (P[prefix + ".weight"], P[prefix + ".bias"], B[prefix + ".running_mean"], B[prefix + ".running_var"])


def _affine(t, bn):
    s, b, _ = bn_fold(*bn)
    return t * s.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)


def _dilations(P):
    return {"lv5_aspp2": 6, "lv5_aspp3": 12, "lv5_aspp4": 18}


def forward64(P, B, c3, c4, c5, keep=None):
    """The head in float64 from `head_params64`'s dicts (NCHW inputs); with autograd when the leaves require it.  `keep`: a dict
    that receives every intermediate."""
    def cbr(m, t, pad=0):
        return _affine(F.conv2d(t, P[m + ".0.weight"], padding=pad), _bn(P, B, m + ".1")).clamp(0, 6)
    k = {} if keep is None else keep
    k["a1"] = cbr("lv5_aspp1", c5)
    for i, (m, dil) in enumerate(_dilations(P).items()):
        e = cbr(m + ".conv.0", c5)
        wd = P[m + ".conv.1.0.weight"]
        d = _affine(F.conv2d(e, wd, padding=dil, dilation=dil, groups=wd.shape[0]), _bn(P, B, m + ".conv.1.1")).clamp(0, 6)
        k["e%d" % (i + 2)], k["d%d" % (i + 2)] = e, d
        k["a%d" % (i + 2)] = _affine(F.conv2d(d, P[m + ".conv.2.weight"]), _bn(P, B, m + ".conv.3"))
    k["aspp"] = torch.cat([k["a1"], k["a2"], k["a3"], k["a4"]], 1)
    k["x5"], k["x4"], k["x3"] = cbr("conv_lv5", k["aspp"]), cbr("conv_lv4", c4), cbr("conv_lv3", c3)
    up = lambda t: F.interpolate(t, size=c3.shape[2:], mode="bilinear", align_corners=True)      # noqa: E731
    k["cat"] = torch.cat([up(k["x5"]), up(k["x4"]), k["x3"]], 1)
    k["y"] = cbr("conv_last", k["cat"], 1)
    return k["y"]


def _up_matrix(n_in, n_out):
    """[n_out, n_in]: the align_corners=True linear resize along one axis."""
    M = torch.zeros(n_out, n_in, dtype=torch.float64)
    for o in range(n_out):
        pos = o * (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
        i0 = min(int(math.floor(pos)), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        f = pos - i0
        M[o, i0] += 1 - f
        M[o, i1] += f
    return M


def up_bwd(g, hi, wi):
    """The adjoint of the align_corners resize: `g` [N,C,Ho,Wo] -> [N,C,hi,wi]."""
    My, Mx = _up_matrix(hi, g.shape[2]), _up_matrix(wi, g.shape[3])
    return torch.einsum("ncyx,yi,xj->ncij", g, My, Mx)


def backward64(P, B, c3, c4, c5, go, variant=None, keep=None):
    """The 42 gradients of sum(go * head(c3, c4, c5)) from the CLOSED FORMS (no autograd): a float64 forward that keeps every
    intermediate, then the walk of train.srf_head_backward.  Returns `{name: gradient in the parameter's shape}`."""
    P = {k: v.detach() for k, v in P.items()}
    k = {} if keep is None else keep
    forward64(P, B, c3, c4, c5, keep=k)
    nh = lambda t: t.permute(0, 2, 3, 1)                                  # noqa: E731
    fl = lambda t: nh(t).reshape(-1, t.shape[1])                          # noqa: E731
    b3 = lambda pre: (P[pre + ".weight"], B[pre + ".running_mean"], B[pre + ".running_var"])      # noqa: E731
    out = {}

    def cbr_bwd(m, t, y, g):
        W = P[m + ".0.weight"]
        r = SR.cbr_grads(fl(t), fl(y), fl(g), W.reshape(W.shape[0], -1), *b3(m + ".1"),
                         variant=variant if variant in STAGE_WRONG else None)
        out[m + ".0.weight"], out[m + ".1.weight"], out[m + ".1.bias"] = r["W"].reshape(W.shape), r["gamma"], r["beta"]
        return r["x"].reshape(t.shape[0], t.shape[2], t.shape[3], -1).permute(0, 3, 1, 2)
    r = cbr3_grads(nh(k["cat"]), nh(k["y"]), nh(go), P["conv_last.0.weight"], *b3("conv_last.1"),
                   variant=variant if variant in CONV3_WRONG + STAGE_WRONG + ("nonstrict_masks",) else None)
    out["conv_last.0.weight"], out["conv_last.1.weight"], out["conv_last.1.bias"] = r["W"], r["gamma"], r["beta"]
    g_cat = r["x"].permute(0, 3, 1, 2)
    n5, n4 = k["x5"].shape[1], k["x4"].shape[1]
    g_x5 = up_bwd(g_cat[:, :n5], *k["x5"].shape[2:])
    g_x4 = up_bwd(g_cat[:, n5:n5 + n4], *k["x4"].shape[2:])
    cbr_bwd("conv_lv3", c3, k["x3"], g_cat[:, n5 + n4:])
    cbr_bwd("conv_lv4", c4, k["x4"], g_x4)
    g_aspp = cbr_bwd("conv_lv5", k["aspp"], k["x5"], g_x5)
    w1 = k["a1"].shape[1]
    cbr_bwd("lv5_aspp1", c5, k["a1"], g_aspp[:, :w1])
    k.update(g_cat=g_cat, g_x5=g_x5, g_x4=g_x4, g_aspp=g_aspp)
    for i, (m, dil) in enumerate(_dilations(P).items()):
        e, d = k["e%d" % (i + 2)], k["d%d" % (i + 2)]
        gb = g_aspp[:, w1 + 256 * i:w1 + 256 * (i + 1)]
        pw, wd, w3 = P[m + ".conv.0.0.weight"], P[m + ".conv.1.0.weight"], P[m + ".conv.2.weight"]
        s2 = bn_fold(*_bn(P, B, m + ".conv.1.1"))[0]
        s3 = bn_fold(*_bn(P, B, m + ".conv.3"))[0]
        gd = F.conv_transpose2d(gb * s3.view(1, -1, 1, 1), w3)
        ga = ir_bwd_dil(nh(gd), nh(d), nh(e), wd.reshape(-1, 3, 3), s2, dil, variant if variant in DIL_WRONG else None)
        gs, _ = block_grads_dil(nh(c5), nh(e), nh(d), nh(gd), ga, nh(gb), pw, wd, w3, b3(m + ".conv.0.1"), b3(m + ".conv.1.1"),
                                b3(m + ".conv.3"), dil, variant if variant in DIL_WRONG else None)
        for n, v in zip(BLOCK_NAMES, gs):
            out["%s.%s" % (m, n)] = v.reshape(P["%s.%s" % (m, n)].shape)
        k["gd%d" % (i + 2)], k["ga%d" % (i + 2)] = gd, ga.permute(0, 3, 1, 2)
    return out


def norm2(ts):
    return math.sqrt(sum(float((t.double() ** 2).sum()) for t in ts))


# ------------------------------------------------------------------------------------------------ seeded numbers
def calibrate(sfnet, seed=5):
    """Seeded numbers into the head of an `uavsal_srfnet_aspp` (the package's or the reference's: the same names): kaiming-scaled
    conv weights and BatchNorms calibrated on a fixed population (float64, CPU) so that every ReLU6 stage sees pre-activations
    of mean about 1.5 and spread about 3, with running statistics and weights that are not the initial 0 and 1.  Returns
    `sfnet` in eval mode."""
    import numpy as np
    sfnet.eval()
    rs = np.random.RandomState(seed)
    head = [getattr(sfnet, n) for n in HEAD]
    with torch.no_grad():
        for h in head:
            for m in h.modules():
                if isinstance(m, torch.nn.Conv2d):
                    fan_out = m.weight.shape[0] * m.weight.shape[2] * m.weight.shape[3] // m.groups
                    m.weight.copy_(torch.from_numpy(rs.standard_normal(tuple(m.weight.shape)) * math.sqrt(2.0 / fan_out)))
    c3, c4, c5 = (torch.from_numpy(3.0 * rs.random_sample((4, c, h, w))) for c, (h, w) in ((32, (9, 28)), (96, (5, 14)), (320, (3, 7))))
    v = lambda t: t.double().view(1, -1, 1, 1)                            # noqa: E731

    def fix(bn, pre, mean, std):
        c = bn.weight.numel()
        with torch.no_grad():
            bn.running_mean.copy_(pre.mean((0, 2, 3)) + torch.from_numpy(0.1 * rs.standard_normal(c)) * pre.std((0, 2, 3)))
            bn.running_var.copy_(pre.var((0, 2, 3)).clamp_min(1e-8) * torch.from_numpy(0.8 + 0.4 * rs.random_sample(c)))
            bn.weight.copy_(std * torch.from_numpy(0.8 + 0.4 * rs.random_sample(c)))
            bn.bias.copy_(mean + torch.from_numpy(0.5 * rs.standard_normal(c)))
        return (pre - v(bn.running_mean)) / torch.sqrt(v(bn.running_var) + bn.eps) * v(bn.weight) + v(bn.bias)

    def cbr(m, t, pad=0):
        return fix(m[1], F.conv2d(t, m[0].weight.detach().double(), padding=pad), 1.5, 3.0).clamp(0, 6)

    def dw(b, t, dil):
        e = cbr(b.conv[0], t)
        d = fix(b.conv[1][1], F.conv2d(e, b.conv[1][0].weight.detach().double(), padding=dil, dilation=dil, groups=e.shape[1]),
                1.5, 3.0).clamp(0, 6)
        return fix(b.conv[3], F.conv2d(d, b.conv[2].weight.detach().double()), 1.5, 1.5)
    a = [cbr(sfnet.lv5_aspp1, c5)] + [dw(getattr(sfnet, n), c5, dil) for n, dil in _dilations(None).items()]
    x5, x4, x3 = cbr(sfnet.conv_lv5, torch.cat(a, 1)), cbr(sfnet.conv_lv4, c4), cbr(sfnet.conv_lv3, c3)
    up = lambda t: F.interpolate(t, size=c3.shape[2:], mode="bilinear", align_corners=True)      # noqa: E731
    cbr(sfnet.conv_last, torch.cat([up(x5), up(x4), x3], 1), 1)
    return sfnet


def golden_name(case):
    return "srf_N%d_%dx%d" % (case[0], case[1][0], case[1][1])


def golden_inputs(case):
    """`(c3, c4, c5, go)` float32 numpy NCHW of a golden case."""
    import numpy as np
    N, s3, s4, s5 = case
    rs = np.random.RandomState(9000 + N * s3[0] * s3[1])
    c3, c4, c5 = ((3.0 * rs.random_sample((N, c) + tuple(s))).astype(np.float32) for c, s in ((32, s3), (96, s4), (320, s5)))
    return c3, c4, c5, (rs.standard_normal((N, 256) + tuple(s3)) / (s3[0] * s3[1])).astype(np.float32)


def golden_digest(sfnet, *arrays):
    """sha256 over the head's parameters and buffers (fp32 bytes, state_dict order) and the inputs."""
    import hashlib
    h = hashlib.sha256()
    for k, t in sfnet.state_dict().items():
        if k.split(".")[0] in HEAD and not k.endswith("num_batches_tracked"):
            h.update(k.encode())
            h.update(t.detach().float().cpu().numpy().tobytes())
    for a in arrays:
        h.update(a.tobytes())
    return h.hexdigest()


def golden_pack(grads):
    """What a golden file keeps of `{name: float64 numpy gradient}`: the small gradients whole, the big weight gradients on
    W_SUBSET (of the [Cout, rest] matrix) plus their sum and L2 norm."""
    out = {}
    for n, g in grads.items():
        key = n.replace(".", "_")
        if g.size > BIG:
            m = g.reshape(g.shape[0], -1)
            out.update({key: m[W_SUBSET], key + "__sum": m.sum(), key + "__l2": (m * m).sum() ** 0.5})
        else:
            out[key] = g
    return out
