"""Float64 restatement of the backward of a general inverted-residual block (train.block_backward / block_param_grads,
csrc/train_block.hip), the seeded inputs of its tests and the per-element bounds, in the convention of
tests/decoder_ref64.py:

    |kernel - ref| <= bound,      U = 2^-24, LAMBDA = 8, EPS = 8 U (tests/plan_ref64.py),  D = 2^-53

Two configurations (CFG): "fucbst" = dwBlock(320, 256), 1920 hidden channels, no residual (model.fucbst_layer[0]) and "fust" =
dwBlock(256, 256), 1536 hidden channels, with the residual (model.fust_layer[0]).  The block of a case is built on its data
the way `train_ref64.decoder_params` builds the decoder: kaiming weights and folded BatchNorms under which the
pre-activations of both ReLU6s have std 3 and mean 1.5 + N(0, 1) per channel (both clamps of both hold a sizeable share,
asserted by the CPU test), the outputs mean 0 and std 1 per channel; the running statistics are `decoder_ref64.bn_stats`'
recipe (r from {0.5, 1, 2}, eps = 2^-20, so var + eps and the fold gamma r are exact in fp32; mu ~ N(0, 1)).

The kernels are tested teacher-forced: they are handed the float64 e, d, gd, ga ROUNDED to fp32 (e and d by
`teacher_round`: within 2 U, the mask kept), x and go are fp32 inputs, and the reference is the pure float64 closed form.
The bounds count every rounding, on sums of absolute values, n = T H W:

  delta2 = gd 1[d]        no arithmetic: the stored gd carries U |gd|:  err2 = U |gd| mask
  S2 = sum delta2         err2, + n D sum |delta2| for the double accumulation (every sum below carries that term)
  Gd = sum delta2 e'      err2 |e'| + 2 U |delta2| |e'| (the stored e); the product is formed in double
  S1 = sum ga             U |ga| (the stored ga is rounded once)
  S3 = sum go             go is an input: n D sum |go| alone
  G1 = sum ga x           (LAMBDA U sqrt(n) + U) sum |ga| |x|: the fp32 MFMA chains, the fp32 adds of the chains and the
                          double sum of the shares as for uavsal_twa_wgrad (tests/train_ref64.py), + U for the stored ga
  G3 = sum go d           (LAMBDA U sqrt(n) + 2 U) sum |go| |d|: the same GEMM, + 2 U for the stored d
Each final tensor takes the absolute-value chain of its formula and EPS on its absolute terms for the final rounding (s, r
and mu are exact inputs; the multiplications by them are done in double):
  W = s G:  |s| err(G) + EPS |s G|        beta = S:  err(S) + EPS |S|
  gamma = r (sum W G - mu S):  r (sum |W| err(G) + |mu| err(S)) + EPS r (sum |W G| + |mu S|)
uavsal_ir_bwd alone (handed the stored gd, d, e): (LAMBDA * 3 + 3) U on the absolute-value chain: a sum of 9 products
(LAMBDA sqrt(9)), the stored gd (U), the tap product's and the s2 product's rounding (2 U).
No factor is fitted to what a kernel gives.

The pixel GEMM's partition is restated with ceil(N / 128) N tiles (`gemm_partition`); `GEMM_SPLIT_T` is the smallest frame
count at 45 x 80 at which a share of the 1920 x 320 GEMM holds two chunks.

Every function takes and returns float64 tensors on the device of its inputs unless it says numpy."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import decoder_ref64 as DR
import train_ref64 as R
from plan_ref64 import EPS, LAMBDA, U, rtol

NAMES = DR.NAMES
CFG = {"fucbst": dict(cin=320, hid=1920, cout=256, res=False), "fust": dict(cin=256, hid=1536, cout=256, res=True)}
CFGS = tuple(CFG)
SHAPES, GOLDEN_SHAPES, SLAB_SHAPE = R.SHAPES, R.GOLDEN_SHAPES, DR.SLAB_SHAPE
BN_EPS = DR.BN_EPS
ZERO_GAMMA = (41, 1201)      # gamma1 = 0 / gamma2 = 0 (block_case(zero_gamma=True)); 41: its constant e = 1.5 gives an interior d
#                              strictly inside (0, 6) in both configurations at (3, 5, 7), so ga and its gamma1 gradient are not 0
GEMM_CHAIN, GEMM_TARGET_WGS, GEMM_TILE = DR.GEMM_CHAIN, DR.GEMM_TARGET_WGS, DR.GEMM_TILE
GROUP = 256                                                      # csrc/train_block.hip: channels of one workgroup of the sums
NSUM = 11
WRONG = ("taps_flipped", "halo_across_frames", "nonstrict_masks", "no_mu_term", "s3_twice", "last_share", "n_tail",
         "group_tail")                                            # + "no_residual" of grad_x (`grad_x_ref`)
W_SUBSET = (slice(None, None, 5), slice(None, None, 7))          # the strided part of the W1 / W3 gradients the goldens keep
GX_SUBSET = (slice(None), slice(None, None, 9), slice(None, None, 2), slice(None, None, 3))
D = DR.D


def name(cfg, shape):
    return "block_%s_T%d_%dx%d" % ((cfg,) + tuple(shape))


def _seed(cfg, shape):
    return R.SEED[shape] + 5000 + 100 * CFGS.index(cfg)


# ------------------------------------------------------------------------------------------------ inputs (float32 numpy)
def block_case(cfg, shape, zero_gamma=False):
    """`(x [T,Cin,H,W] uniform in [0, 3), q, go [T,Co,H,W])`: the block's input, its MODULE numbers q = {w1, wd, w3, g*, be*,
    mu*, var*} (* = 1, 2, 3; float32 numpy) and the gradient that arrives at its output.  `zero_gamma`: gamma1 of channel
    ZERO_GAMMA[0] and gamma2 of channel ZERO_GAMMA[1] are 0 and their beta 1.5."""
    c = CFG[cfg]
    cin, hid, cout = c["cin"], c["hid"], c["cout"]
    T, H, W = shape
    rs = np.random.RandomState(_seed(cfg, shape))
    x = (3.0 * rs.random_sample((T, cin, H, W))).astype(np.float32)
    go = (rs.standard_normal((T, cout, H, W)) / (H * W)).astype(np.float32)
    p = {"w1": (rs.standard_normal((hid, cin, 1, 1)) * math.sqrt(2.0 / hid)).astype(np.float32),
         "wd": (rs.standard_normal((hid, 1, 3, 3)) * math.sqrt(2.0 / (hid * 9))).astype(np.float32),
         "w3": (rs.standard_normal((cout, hid, 1, 1)) * math.sqrt(2.0 / cout)).astype(np.float32)}
    m1, m2 = rs.standard_normal(hid), rs.standard_normal(hid)
    v = lambda t: t.double().view(1, -1, 1, 1)                   # noqa: E731

    def norm(pre, mean, std):
        sd, mu = pre.std((0, 2, 3)), pre.mean((0, 2, 3))
        s = std / sd
        return s.float(), (mean - mu * s).float()
    xx = torch.as_tensor(x, dtype=torch.float64)
    pre = F.conv2d(xx, torch.as_tensor(p["w1"]).double())
    s1, b1 = norm(pre, 1.5 + torch.as_tensor(m1), 3.0)
    e = (pre * v(s1) + v(b1)).clamp(0, 6)
    pre = F.conv2d(e, torch.as_tensor(p["wd"]).double(), padding=1, groups=hid)
    s2, b2 = norm(pre, 1.5 + torch.as_tensor(m2), 3.0)
    d = (pre * v(s2) + v(b2)).clamp(0, 6)
    s3, b3 = norm(F.conv2d(d, torch.as_tensor(p["w3"]).double()), 0.0, 1.0)
    fold = {"s1": s1, "b1": b1, "s2": s2, "b2": b2, "s3": s3, "b3": b3}
    st = np.random.RandomState(_seed(cfg, shape) + 4000)
    q = dict(p)
    for i, n in ((1, hid), (2, hid), (3, cout)):
        r = st.choice(np.array([0.5, 1.0, 2.0], np.float32), n)
        mu = st.standard_normal(n).astype(np.float32)
        s, b = fold["s%d" % i].numpy(), fold["b%d" % i].numpy()
        var = 1.0 / r.astype(np.float64) ** 2 - BN_EPS
        assert np.all(var.astype(np.float32).astype(np.float64) == var)
        q["g%d" % i] = (s / r).astype(np.float32)
        q["be%d" % i] = (b.astype(np.float64) + mu.astype(np.float64) * s).astype(np.float32)
        q["mu%d" % i], q["var%d" % i] = mu, var.astype(np.float32)
    if zero_gamma:
        for i, ch in ((1, ZERO_GAMMA[0]), (2, ZERO_GAMMA[1])):
            q["g%d" % i][ch] = 0.0
            q["be%d" % i][ch] = 1.5
    return x, q, go


fold = DR.fold
load_block = DR.load_block                                       # the numbers into a dwBlock (the package's or the reference's)
teacher_round, mask_flips, to64 = DR.teacher_round, DR.mask_flips, DR.to64


def gemm_inputs(shape, M, N, seed=8000):
    """Random operands of the pixel GEMM: `(a [T,H,W,M], b [T,H,W,N])` float32 numpy NHWC."""
    T, H, W = shape
    rs = np.random.RandomState(seed + T * H * W + M + N)
    return (1e-2 * rs.standard_normal((T, H, W, M))).astype(np.float32), rs.standard_normal((T, H, W, N)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ partitions, restated
def gemm_partition(K, M, N):
    """The K split of uavsal_pix_gemm with N a multiple of 64: `(cps, shares, [(p0, p1) per share])` over
    (M / 128) ceil(N / 128) tiles (for N % 128 == 0 this is decoder_ref64.gemm_partition)."""
    tiles = (M // GEMM_TILE) * -(-N // GEMM_TILE)
    chunks = -(-K // GEMM_CHAIN)
    most = max(1, min(GEMM_TARGET_WGS // tiles, chunks))
    cps = -(-chunks // most)
    span = cps * GEMM_CHAIN
    spans = [(p, min(p + span, K)) for p in range(0, K, span)]
    return cps, len(spans), spans


def gemm_split_frames(M, N, H=45, W=80):
    """The smallest frame count at H x W at which a share of the M x N pixel GEMM holds two chunks."""
    return next(T for T in range(1, 1000) if gemm_partition(T * H * W, M, N)[0] == 2)


slab_partition = DR.slab_partition                               # the slabs of uavsal_ir_sums: the rule of uavsal_dec_sums


# ------------------------------------------------------------------------------------------------ the closed form
def _v(t):
    return t.reshape(1, -1, 1, 1)


def forward(p, x, res):
    """`p`: the eval fold as float64 tensors.  Returns dict(e_pre, e, d_pre, d, o)."""
    hid = p["w1"].shape[0]
    e_pre = F.conv2d(x, p["w1"]) * _v(p["s1"]) + _v(p["b1"])
    e = e_pre.clamp(0, 6)
    d_pre = F.conv2d(e, p["wd"], padding=1, groups=hid) * _v(p["s2"]) + _v(p["b2"])
    d = d_pre.clamp(0, 6)
    o = F.conv2d(d, p["w3"]) * _v(p["s3"]) + _v(p["b3"])
    return {"e_pre": e_pre, "e": e, "d_pre": d_pre, "d": d, "o": o + x if res else o}


def ir_bwd_ref(p, gd, d, e, variant=None, absolute=False):
    """uavsal_ir_bwd from the stored gd, d, e: `ga [T,Ch,H,W]`; `absolute`: the same chain on absolute values."""
    a = (lambda t: t.abs()) if absolute else (lambda t: t)
    hid = d.shape[1]
    if variant == "nonstrict_masks":
        me, md = (e >= 0) & (e <= 6), (d >= 0) & (d <= 6)
    else:
        me, md = (e > 0) & (e < 6), (d > 0) & (d < 6)
    d2 = a(gd) * md
    if variant == "taps_flipped":
        back = F.conv2d(d2, a(p["wd"]), padding=1, groups=hid)
    elif variant == "halo_across_frames":
        T, _, H, W = d2.shape
        tall = d2.permute(1, 0, 2, 3).reshape(1, hid, T * H, W)
        back = F.conv_transpose2d(tall, a(p["wd"]), padding=1, groups=hid).reshape(hid, T, H, W).permute(1, 0, 2, 3)
    else:
        back = F.conv_transpose2d(d2, a(p["wd"]), padding=1, groups=hid)
    return back * _v(a(p["s2"])) * me


def ir_bwd_bound(p, gd, d, e):
    return (LAMBDA * 3 + 3) * U * ir_bwd_ref(p, gd, d, e, absolute=True)


def param_grads(q, x, go, variant=None, bounds=False, parts=None):
    """The nine gradients of d sum(go o) / d parameter, keyed by NAMES, in the parameters' shapes (the residual does not enter
    them); `bounds`: returns `(grads, bounds)` with the per-element bounds of the docstring.  `variant`: one of WRONG, the
    result of a kernel that gets that one thing wrong.  `parts`: a dict that receives e, d, gd, ga (NCHW), grad_x WITHOUT the
    residual's go, e_pre and d_pre."""
    p = fold(q)
    f = forward(p, x, False)
    e, d = f["e"], f["d"]
    hid, cin = q["w1"].shape[:2]
    cout = q["w3"].shape[0]
    s1, s2, s3 = p["s1"], p["s2"], p["s3"]
    w1, wd, w3 = q["w1"].reshape(hid, cin), q["wd"], q["w3"].reshape(cout, hid)
    gd = F.conv_transpose2d(go * _v(s3), q["w3"])
    mask_variant = variant if variant == "nonstrict_masks" else None
    md = ((d >= 0) & (d <= 6)).double() if mask_variant else ((d > 0) & (d < 6)).double()
    d2 = gd * md
    ga = ir_bwd_ref(p, gd, d, e, variant=mask_variant)
    T, _, H, W = x.shape
    K = T * H * W
    gaw, gow = ga, go
    if variant == "last_share":
        for which, (M, N) in (("ga", (hid, cin)), ("go", (cout, hid))):
            wt = torch.ones(K, dtype=ga.dtype, device=ga.device)
            p0, p1 = gemm_partition(K, M, N)[2][-1]
            wt[p0:p1] = 0
            if which == "ga":
                gaw = ga * wt.view(T, 1, H, W)
            else:
                gow = go * wt.view(T, 1, H, W)
    G1 = torch.einsum("tchw,tjhw->cj", gaw, x)
    G3 = torch.einsum("tmhw,tchw->mc", gow, d)
    if variant == "n_tail":                                      # the columns of a half-filled last N tile are never written
        G1, G3 = G1.clone(), G3.clone()
        G1[:, cin // GEMM_TILE * GEMM_TILE:] = 0
        G3[:, hid // GEMM_TILE * GEMM_TILE:] = 0
    S1, S2, S3 = ga.sum((0, 2, 3)), d2.sum((0, 2, 3)), go.sum((0, 2, 3))
    Gd = DR._tap_sums(d2, e, across_frames=variant == "halo_across_frames")
    if variant == "taps_flipped":
        Gd = Gd.flip(1, 2)
    if variant == "group_tail":                                  # the channels behind the last whole group of 256 are left out
        S1, S2, Gd = S1.clone(), S2.clone(), Gd.clone()
        for t in (S1, S2, Gd):
            t[hid // GROUP * GROUP:] = 0
    wdm = wd.reshape(hid, 3, 3)
    mu1S = 0 if variant == "no_mu_term" else p["mu1"] * S1
    g = {NAMES[0]: s1.view(-1, 1) * G1,
         NAMES[1]: p["r1"] * ((w1 * G1).sum(1) - mu1S), NAMES[2]: S1,
         NAMES[3]: s2.view(-1, 1, 1) * Gd, NAMES[4]: p["r2"] * ((wdm * Gd).sum((1, 2)) - p["mu2"] * S2), NAMES[5]: S2,
         NAMES[6]: (s3 * s3 if variant == "s3_twice" else s3).view(-1, 1) * G3,
         NAMES[7]: p["r3"] * ((w3 * G3).sum(1) - p["mu3"] * S3), NAMES[8]: S3}
    shapes = {NAMES[0]: (hid, cin, 1, 1), NAMES[3]: (hid, 1, 3, 3), NAMES[6]: (cout, hid, 1, 1)}
    g = {k: t.reshape(shapes.get(k, t.shape)) for k, t in g.items()}
    if parts is not None:
        parts.update(e=e, d=d, gd=gd, ga=ga, grad_x=F.conv_transpose2d(ga * _v(s1), q["w1"]), e_pre=f["e_pre"], d_pre=f["d_pre"])
    if not bounds:
        return g
    n = K
    a2 = gd.abs() * md
    eS2 = ((U + n * D) * a2).sum((0, 2, 3))
    eGd = DR._tap_sums((3 * U + n * D) * a2, e.abs())
    eS1 = (U + n * D) * ga.abs().sum((0, 2, 3))
    eS3 = n * D * go.abs().sum((0, 2, 3))
    AG1 = torch.einsum("tchw,tjhw->cj", ga.abs(), x.abs())
    AG3 = torch.einsum("tmhw,tchw->mc", go.abs(), d.abs())
    eG1 = (LAMBDA * U * math.sqrt(n) + U) * AG1
    eG3 = (LAMBDA * U * math.sqrt(n) + 2 * U) * AG3
    aGd = DR._tap_sums(a2, e.abs())
    r1, r2, r3, mu1, mu2, mu3 = (p[k].abs() for k in ("r1", "r2", "r3", "mu1", "mu2", "mu3"))
    aS1, aS2, aS3 = ga.abs().sum((0, 2, 3)), a2.sum((0, 2, 3)), go.abs().sum((0, 2, 3))
    b = {NAMES[0]: s1.abs().view(-1, 1) * (eG1 + EPS * AG1),
         NAMES[1]: r1 * ((w1.abs() * eG1).sum(1) + mu1 * eS1) + EPS * r1 * ((w1.abs() * AG1).sum(1) + mu1 * aS1),
         NAMES[2]: eS1 + EPS * aS1,
         NAMES[3]: s2.abs().view(-1, 1, 1) * (eGd + EPS * aGd),
         NAMES[4]: r2 * ((wdm.abs() * eGd).sum((1, 2)) + mu2 * eS2) + EPS * r2 * ((wdm.abs() * aGd).sum((1, 2)) + mu2 * aS2),
         NAMES[5]: eS2 + EPS * aS2,
         NAMES[6]: s3.abs().view(-1, 1) * (eG3 + EPS * AG3),
         NAMES[7]: r3 * ((w3.abs() * eG3).sum(1) + mu3 * eS3) + EPS * r3 * ((w3.abs() * AG3).sum(1) + mu3 * aS3),
         NAMES[8]: eS3 + EPS * aS3}
    b = {k: t.reshape(g[k].shape) for k, t in b.items()}
    return g, b


def autograd_grads(q, x, go, res):
    """torch autograd through the restated forward, from the module's numbers: `(the nine gradients keyed by NAMES, grad_x)`."""
    keys = ("w1", "g1", "be1", "wd", "g2", "be2", "w3", "g3", "be3")
    leaves = {k: q[k].detach().clone().requires_grad_(True) for k in keys}
    xx = x.detach().clone().requires_grad_(True)
    qq = dict(q)
    qq.update(leaves)
    o = forward(fold(qq), xx, res)["o"]
    gs = torch.autograd.grad(o, [leaves[k] for k in keys] + [xx], go)
    return dict(zip(NAMES, gs[:-1])), gs[-1]


def grad_x_ref(q, x, go, res, variant=None):
    """grad_x of the block in float64 from the float64 forward; `variant` "no_residual": the + go of the residual left out."""
    parts = {}
    param_grads(q, x, go, parts=parts)
    return parts["grad_x"] + go if res and variant != "no_residual" else parts["grad_x"]


def block_e2e(q, x, go, res):
    """grad_x when the DEVICE recomputes e and d: `(grad_x, bound, undecided, f)`, the construction of
    `train_ref64.decoder_e2e`.  `bound` is the regular per-element bound: the gd GEMM's (a sum of Co products, + U for the
    product s3 W3 rounded once in the packed weights) and uavsal_ir_bwd's own, carried through the absolute-value chain, plus
    the Ch -> Cin GEMM's own (a sum of Ch products, + U for s1 W1) and EPS on the result and the residual.  `undecided` is
    the absolute contribution of every e and d element whose float64 pre-activation lies within its forward bound (plan_ref64's
    chain rule) of a clamp: its mask may legitimately differ on the device, which removes or adds the element's whole term."""
    p = fold(q)
    f = forward(p, x, res)
    hid, cin = q["w1"].shape[:2]
    cout = q["w3"].shape[0]
    w1a, wda, w3a = p["w1"].abs(), p["wd"].abs(), p["w3"].abs()
    be_pre = F.conv2d(x.abs(), w1a) * _v(p["s1"].abs()) + _v(p["b1"].abs())
    err_e = rtol("f32", cin) * be_pre + EPS * 2 * f["e_pre"].abs()
    bd_pre = F.conv2d(be_pre, wda, padding=1, groups=hid) * _v(p["s2"].abs()) + _v(p["b2"].abs())
    err_d = (rtol("f32", cin) + rtol("f32", 9)) * bd_pre + EPS * 2 * f["d_pre"].abs()
    near = lambda pre, err: ((pre.abs() <= err) | ((pre - 6).abs() <= err)).double()      # noqa: E731
    ue, ud = near(f["e_pre"], err_e), near(f["d_pre"], err_d)
    e, d = f["e"], f["d"]
    me, md = ((e > 0) & (e < 6)).double(), ((d > 0) & (d < 6)).double()
    gd = F.conv_transpose2d(go * _v(p["s3"]), p["w3"])
    gd_abs = F.conv_transpose2d(go.abs() * _v(p["s3"].abs()), w3a)
    ga = ir_bwd_ref(p, gd, d, e)
    ga_abs = F.conv_transpose2d(gd_abs * md, wda, padding=1, groups=hid) * _v(p["s2"].abs()) * me
    grad_x = F.conv_transpose2d(ga * _v(p["s1"]), p["w1"])
    rel = (rtol("f32", cout) + U + 2 * EPS) + (LAMBDA * 3 + 2) * U + (rtol("f32", hid) + U)
    bound = rel * F.conv_transpose2d(ga_abs * _v(p["s1"].abs()), w1a) + EPS * grad_x.abs()
    if res:
        grad_x = grad_x + go
        bound = bound + EPS * (go.abs() + grad_x.abs())
    from_d = F.conv_transpose2d(gd.abs() * ud, wda, padding=1, groups=hid) * _v(p["s2"].abs()) * me
    from_e = (F.conv_transpose2d(gd * md, p["wd"], padding=1, groups=hid) * _v(p["s2"])).abs() * ue
    undecided = F.conv_transpose2d((from_d + from_e) * _v(p["s1"].abs()), w1a)
    f.update(ue=ue, ud=ud, gd=gd, ga=ga)
    return grad_x, bound, undecided, f


def pix_gemm_ref(a, b):
    """uavsal_pix_gemm on NHWC float64 `a [T,H,W,M]`, `b [T,H,W,N]`: `(G [M,N], bound)` with row_scale 1."""
    return DR.pix_gemm_ref(a, b)


def class_shares(t):
    """(share of elements <= 0, strictly inside, >= 6) of a ReLU6 output."""
    lo, hi = float((t <= 0).double().mean()), float((t >= 6).double().mean())
    return lo, 1.0 - lo - hi, hi
