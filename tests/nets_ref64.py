"""Float64 restatement of the backward of the gauss / ob prior nets (train.narrow_block_param_grads, train.frame_sum,
train.prior_net_backward; csrc/train_nets.hip), the seeded inputs of their tests and the per-element bounds, in the convention
of tests/block_ref64.py:

    |kernel - ref| <= bound,      U = 2^-24, EPS = 8 U (tests/plan_ref64.py),  D = 2^-53

A prior net is two blocks: the NARROW block 0 (NARROW: "gauss0" 8 -> 48 -> 64, "ob0" 20 -> 120 -> 64, no residual; "tiny"
4 -> 4 -> 64 is the smallest shape the kernel takes) and block 1, 64 -> 384 -> 64 with the residual (ctx_ref64's "fucb64"
shape, whose gradients tests/mp_ref64.py restates).  A block of a case is calibrated on its input the way
`ctx_ref64.calibrated` does it (the same recipe, for any widths).

The narrow kernel is tested teacher-forced: it is handed the float64 e, d, gd, ga ROUNDED to fp32 (e and d by
`teacher_round`: within 2 U, the mask kept); x and go are fp32 inputs.  Its chain, rounding by rounding, on sums of absolute
values, n = pixels:

  delta2 = gd 1[d]        no arithmetic: the stored gd carries U |gd|
  S2 = sum delta2         U + n D      (every product and sum of the eleven sums and S3 is formed and added in double)
  Gd = sum delta2 e'      U (stored gd) + 2 U (stored e) + n D
  S1 = sum ga             U (stored ga) + n D
  S3 = sum go             n D          (go is an input)
  G1 = sum ga x           G (1 + U) + U + 2 n D,  G = CHUNK U / (1 - CHUNK U): a chunk of CHUNK = 32 pixels is a chain of fused
                          multiply-adds in fp32, one rounding per term (the standard gamma_k bound on sum |terms|); the chunk
                          sums are exact in double and added in double (n D for the chunks of a slab, n D for the slabs); U for
                          the stored ga
  G3 = sum go d           G (1 + 2 U) + 2 U + 2 n D  (2 U: the stored d)
Each final tensor takes the absolute-value chain of its formula and EPS on its absolute terms for the final rounding (the row
dots and the products with s, r, mu are formed in double), exactly as block_ref64.param_grads does:
  W = s G:  |s| err(G) + EPS |s G|        beta = S:  err(S) + EPS |S|
  gamma = r (sum W G - mu S):  r (sum |W| err(G) + |mu| err(S)) + EPS r (sum |W G| + |mu S|)
When the reference is fed the very fp32 tensors the device read (the stage-by-stage form), the U terms of the stored tensors
are slack.  The frame sum adds N frames in double and rounds once: N D sum |a| + U |sum|.  No factor is fitted to what a
kernel gives.

Every function takes and returns float64 tensors on the device of its inputs unless it says numpy."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import block_ref64 as BR
import ctx_ref64 as X
import decoder_ref64 as DR
import mp_ref64 as MP
from plan_ref64 import EPS, U

D = DR.D
NAMES = BR.NAMES
NARROW = {"gauss0": (8, 48, 64), "ob0": (20, 120, 64), "tiny": (4, 4, 64)}      # Cin, Ch, Co
NETS = {"gauss_cb_layer": "gauss0", "ob_cb_layer": "ob0"}
PICTURES = [(1, 1, 1), (1, 5, 7), (2, 9, 13), (1, 45, 80), (3, 45, 80)]      # n, H, W
CHUNK = 32                                                       # UAVSAL_NARROW_CHUNK
SLAB_PIXELS, MAX_SLABS = 256, 256                                # csrc/train_nets.hip
NSUM = BR.NSUM
ZERO = (1, 2)                                                    # gamma1 = 0 in channel 1, gamma2 = 0 in channel 2 (beta 1.5)
WRONG = ("no_mask", "gd_no_border", "gd_image_seam", "stop_at_64", "stop_at_16", "gamma_scaled")
GOLDEN_BIAS, GOLDEN_SHAPE, GOLDEN_T = [(1, 1, 1), (1, 1, 0), (1, 0, 0), (0, 1, 0)], (4, 9, 13), 2      # tests/golden/nets_train_*.npz
W_SUBSET = MP.W_SUBSET

m6, _v = X.m6, X._v


def golden_name(bias):
    return "nets_train_b%d%d%d_N%d_%dx%d" % (tuple(bias) + GOLDEN_SHAPE)


def slab_partition(n, H, W):
    """The slabs of uavsal_ir_narrow_grads: `(rows per slab, slabs)` over the n * H picture rows (the rule of uavsal_ir_sums)."""
    rows = n * H
    sr = max(-(-SLAB_PIXELS // W), -(-rows // MAX_SLABS))
    return sr, -(-rows // sr)


def slab_doubles(cin, hid, cout=64):
    return NSUM * hid + cout + hid * cin + cout * hid


# ------------------------------------------------------------------------------------------------ inputs (float32 numpy)
def calibrated(dims, x, rs, st, gain=1.0, shift=0.0):
    """`ctx_ref64.calibrated` for a stride-1 block of any widths `dims` = (Cin, Ch, Co): the MODULE numbers q (float32 numpy,
    block_ref64's keys) calibrated on the block's input `x` (float64 tensor)."""
    cin, hid, cout = dims
    p = {"w1": (rs.standard_normal((hid, cin, 1, 1)) * math.sqrt(2.0 / hid)).astype(np.float32),
         "wd": (rs.standard_normal((hid, 1, 3, 3)) * math.sqrt(2.0 / (hid * 9))).astype(np.float32),
         "w3": (rs.standard_normal((cout, hid, 1, 1)) * math.sqrt(2.0 / cout)).astype(np.float32)}
    m1, m2 = rs.standard_normal(hid), rs.standard_normal(hid)
    v = lambda t: t.double().view(1, -1, 1, 1)                   # noqa: E731

    def norm(pre, mean, std):
        sd, mu = pre.std((0, 2, 3), unbiased=False).clamp_min(1e-3), pre.mean((0, 2, 3))
        s = std / sd
        return s.float(), (mean - mu * s).float()
    pre = F.conv2d(x, torch.as_tensor(p["w1"]).double())
    s1, b1 = norm(pre, 1.5 + torch.as_tensor(m1), 3.0)
    e = (pre * v(s1) + v(b1)).clamp(0, 6)
    pre = F.conv2d(e, torch.as_tensor(p["wd"]).double(), padding=1, groups=hid)
    s2, b2 = norm(pre, 1.5 + torch.as_tensor(m2), 3.0)
    d = (pre * v(s2) + v(b2)).clamp(0, 6)
    s3, b3 = norm(F.conv2d(d, torch.as_tensor(p["w3"]).double()), 0.0, 1.0)
    fold = {"s1": s1 * gain, "b1": b1 * gain + shift, "s2": s2 * gain, "b2": b2 * gain + shift, "s3": s3, "b3": b3}
    q = dict(p)
    for i, c in ((1, hid), (2, hid), (3, cout)):
        r = st.choice(np.array([0.5, 1.0, 2.0], np.float32), c)
        mu = st.standard_normal(c).astype(np.float32)
        s, b = fold["s%d" % i].numpy().astype(np.float32), fold["b%d" % i].numpy().astype(np.float32)
        var = 1.0 / r.astype(np.float64) ** 2 - BR.BN_EPS
        q["g%d" % i] = (s / r).astype(np.float32)
        q["be%d" % i] = (b.astype(np.float64) + mu.astype(np.float64) * s).astype(np.float32)
        q["mu%d" % i], q["var%d" % i] = mu, var.astype(np.float32)
    return q


def narrow_case(name, shape, gain=1.0, shift=0.0, zero_gamma=False, seed=0):
    """`(x [n,Cin,H,W] uniform in [0, 3), q, go [n,64,H,W])` float32 numpy for the narrow block `name` of NARROW, calibrated on
    that x.  `gain`, `shift`: tests/saturate_bn.py's change of the two BatchNorms in front of a ReLU6.  `zero_gamma`: gamma1 of
    channel ZERO[0] and gamma2 of channel ZERO[1] are 0 and their beta 1.5."""
    cin, hid, cout = NARROW[name]
    n, H, W = shape
    base = 15000 + seed + 17 * sorted(NARROW).index(name) + n * H * W
    rs = np.random.RandomState(base)
    x = (3.0 * rs.random_sample((n, cin, H, W))).astype(np.float32)
    go = (rs.standard_normal((n, cout, H, W)) / (H * W)).astype(np.float32)
    q = calibrated(NARROW[name], torch.as_tensor(x, dtype=torch.float64), rs, np.random.RandomState(base + 4000), gain, shift)
    if zero_gamma:
        for i, ch in ((1, ZERO[0]), (2, ZERO[1])):
            q["g%d" % i][ch], q["be%d" % i][ch] = 0.0, 1.5
    return x, q, go


def make_block(dims, q, dwBlock):
    """The numbers of a case in a `dwBlock` (the package's or the reference's), eval mode.  (A ratio of exactly 1 builds a block
    without an expand conv: "tiny" takes the nearest ratio above it, which still rounds to 4 hidden channels.)"""
    ratio = dims[1] / dims[0] if dims[1] != dims[0] else 1.0 + 2.0 ** -20
    blk = dwBlock(dims[0], dims[2], kernel_size=3, expand_ratio=ratio)
    assert blk.conv[0][0].weight.shape[0] == dims[1]
    return BR.load_block(blk, q)


def net_case(net, shape, seed=0):
    """Both blocks of the prior net `net` (a key of NETS) calibrated on the activations they see: `(cb [n,8|20,H,W] uniform in
    [0, 1) like a prior map, (q0, q1), go [n,64,H,W])` float32 numpy."""
    dims = NARROW[NETS[net]]
    n, H, W = shape
    base = 16000 + seed + 29 * sorted(NETS).index(net) + n * H * W
    rs, st = np.random.RandomState(base), np.random.RandomState(base + 4000)
    cb = rs.random_sample((n, dims[0], H, W)).astype(np.float32)
    go = (rs.standard_normal((n, 64, H, W)) / (H * W)).astype(np.float32)
    x = torch.as_tensor(cb, dtype=torch.float64)
    q0 = calibrated(dims, x, rs, st)
    mid = X.forward(BR.fold(BR.to64(q0)), x, 1, False)["o"]
    q1 = calibrated((64, 384, 64), mid, rs, st)
    return cb, (q0, q1), go


def make_net(net, qs, dwBlock):
    dims = NARROW[NETS[net]]
    return torch.nn.Sequential(make_block(dims, qs[0], dwBlock), make_block((64, 384, 64), qs[1], dwBlock))


# ------------------------------------------------------------------------------------------------ the closed form
def _flat_tap_sums(a, b):
    """[c, ky, kx] = sum over the flat pixel index q of a[q] b[q + (ky - 1) W + (kx - 1)], zero outside the whole buffer: a WRONG
    kernel without the picture's zero border (a row's end sees the next row's start, an image's edge the next image)."""
    n, c, H, W = a.shape
    af, bf = a.permute(1, 0, 2, 3).reshape(c, -1), b.permute(1, 0, 2, 3).reshape(c, -1)
    pad = W + 1
    bp = F.pad(bf, (pad, pad))
    out = a.new_zeros((c, 3, 3))
    for ky in range(3):
        for kx in range(3):
            off = (ky - 1) * W + (kx - 1)
            out[:, ky, kx] = (af * bp[:, pad + off:pad + off + af.shape[1]]).sum(1)
    return out


def grads_from_parts(p, x, e, d, gd, ga, go, bounds=False, variant=None):
    """The nine gradients of a stride-1 block with the eval fold `p` from GIVEN x, e, d, gd, ga, go (NCHW float64): the closed
    form of include/uavsal_hip.h keyed by NAMES, in the parameters' shapes.  `bounds`: `(grads, bounds)` with the module
    docstring's per-element bounds of uavsal_ir_narrow_grads + uavsal_ir_narrow_finish.  `variant`: one of WRONG, the result of
    a kernel that gets that one thing wrong:
      "no_mask": delta2 = gd;  "gd_no_border": Gd reads e by the flat pixel index;  "gd_image_seam": Gd reads the neighbouring
      image at an image seam;  "stop_at_64" / "stop_at_16": the hidden channels from 64 on / behind the last whole 16 are left
      out;  "gamma_scaled": the gamma gradients' row dots take the SCALED sums (the weight gradients)."""
    hid, cin = p["w1"].shape[:2]
    cout = p["w3"].shape[0]
    s1, s2, s3 = p["s1"], p["s2"], p["s3"]
    w1, wdm, w3 = p["w1"].reshape(hid, cin), p["wd"].reshape(hid, 3, 3), p["w3"].reshape(cout, hid)
    md = m6(d).double()
    d2 = gd if variant == "no_mask" else gd * md
    if variant == "gd_no_border":
        Gd = _flat_tap_sums(d2, e)
    else:
        Gd = DR._tap_sums(d2, e, across_frames=variant == "gd_image_seam")
    S1, S2, S3 = ga.sum((0, 2, 3)), d2.sum((0, 2, 3)), go.sum((0, 2, 3))
    G1 = torch.einsum("tchw,tjhw->cj", ga, x)
    G3 = torch.einsum("tmhw,tchw->mc", go, d)
    if variant in ("stop_at_64", "stop_at_16"):
        stop = 64 if variant == "stop_at_64" else hid // 16 * 16
        S1, S2, Gd, G1, G3 = (t.clone() for t in (S1, S2, Gd, G1, G3))
        for t in (S1, S2, Gd, G1):
            t[stop:] = 0
        G3[:, stop:] = 0
    k1, kd, k3 = (s1.view(-1, 1), s2.view(-1, 1, 1), s3.view(-1, 1)) if variant == "gamma_scaled" else (1.0, 1.0, 1.0)
    g = {NAMES[0]: s1.view(-1, 1) * G1, NAMES[1]: p["r1"] * ((w1 * G1 * k1).sum(1) - p["mu1"] * S1), NAMES[2]: S1,
         NAMES[3]: s2.view(-1, 1, 1) * Gd, NAMES[4]: p["r2"] * ((wdm * Gd * kd).sum((1, 2)) - p["mu2"] * S2), NAMES[5]: S2,
         NAMES[6]: s3.view(-1, 1) * G3, NAMES[7]: p["r3"] * ((w3 * G3 * k3).sum(1) - p["mu3"] * S3), NAMES[8]: S3}
    shapes = {NAMES[0]: (hid, cin, 1, 1), NAMES[3]: (hid, 1, 3, 3), NAMES[6]: (cout, hid, 1, 1)}
    g = {k: t.reshape(shapes.get(k, t.shape)) for k, t in g.items()}
    if not bounds:
        return g
    n = x.shape[0] * x.shape[2] * x.shape[3]
    G = CHUNK * U / (1 - CHUNK * U)
    a2 = gd.abs() * md
    eS2 = ((U + n * D) * a2).sum((0, 2, 3))
    eGd = DR._tap_sums((3 * U + n * D) * a2, e.abs())
    eS1 = (U + n * D) * ga.abs().sum((0, 2, 3))
    eS3 = n * D * go.abs().sum((0, 2, 3))
    AG1 = torch.einsum("tchw,tjhw->cj", ga.abs(), x.abs())
    AG3 = torch.einsum("tmhw,tchw->mc", go.abs(), d.abs())
    eG1 = (G * (1 + U) + U + 2 * n * D) * AG1
    eG3 = (G * (1 + 2 * U) + 2 * U + 2 * n * D) * AG3
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
    return g, {k: t.reshape(g[k].shape) for k, t in b.items()}


def variant_applies(variant, dims, shape):
    """Does the WRONG kernel `variant` compute something else than the right one for these widths and this picture?"""
    n, H, W = shape
    hid = dims[1]
    return {"no_mask": n * H * W > 1, "gd_no_border": True, "gd_image_seam": n > 1, "stop_at_64": hid > 64,
            "stop_at_16": hid % 16 != 0, "gamma_scaled": True}[variant]


def param_grads(p, x, go, bounds=False, parts=None, variant=None):
    """The nine gradients of d sum(go o) / d parameter of a stride-1 block without the residual, from the float64 forward."""
    pt = MP.block_parts(p, x, go, 1)
    if parts is not None:
        parts.update(pt)
    return grads_from_parts(p, x, pt["e"], pt["d"], pt["gd"], pt["ga"], go, bounds=bounds, variant=variant)


def frame_sum_ref(a):
    """`(sum over the frames [1,...], bound)` of a float64 `a [N,...]` holding fp32 values."""
    s = a.sum(0, keepdim=True)
    return s, a.shape[0] * D * a.abs().sum(0, keepdim=True) + U * s.abs()


def net_inputs(P, cb, go, given=None):
    """What the walk of train.prior_net_backward hands each block, float64: `{"1": (mid, go), "0": (cb, g_mid)}`; `P` = (fold of
    block 0, fold of block 1).  `given`: float64 `mid` / `g_mid` that replace the float64 results of the stages before."""
    given = given or {}
    mid = given.get("mid")
    if mid is None:
        mid = X.forward(P[0], cb, 1, False)["o"]
    g_mid = given.get("g_mid")
    if g_mid is None:
        g_mid = X.input_grad_ref(P[1], mid, go, 1, True)
    return {"1": (mid, go), "0": (cb, g_mid)}


def net_param_grads(P, cb, go):
    """A net's 18 gradients in float64 closed form: `{"0": {NAMES: tensor}, "1": {...}}`."""
    return {k: param_grads(P[int(k)], x, g) for k, (x, g) in net_inputs(P, cb, go).items()}


def net_forward(P, cb):
    return X.forward(P[1], X.forward(P[0], cb, 1, False)["o"], 1, True)["o"]


def net_autograd(Q, cb, go):
    """torch autograd of sum(go out) through both blocks with respect to their 18 parameters, from the modules' numbers `Q` =
    (q0, q1) as float64 tensors: `{"0": {NAMES: tensor}, "1": {...}}`."""
    keys = ("w1", "g1", "be1", "wd", "g2", "be2", "w3", "g3", "be3")
    leaves = [{k: q[k].detach().clone().requires_grad_(True) for k in keys} for q in Q]
    P = []
    for q, lv in zip(Q, leaves):
        qq = dict(q)
        qq.update(lv)
        P.append(BR.fold(qq))
    out = net_forward(P, cb)
    gs = torch.autograd.grad(out, [lv[k] for lv in leaves for k in keys], go)
    return {str(i): dict(zip(NAMES, gs[9 * i:9 * i + 9])) for i in range(2)}


# ------------------------------------------------------------------------------------------------ the reference's recorded results
GOLDEN_MODES = ("frame", "repeat")                               # N different prior frames / ONE prior repeated over the frames
G_SUBSET = (slice(None), slice(None), slice(None, None, 3), slice(None, None, 4))      # the part of the nets' slices of g_cb the goldens keep


def golden_subset_names(block):
    """The weight gradients of block 0 / 1 of a net that the goldens keep on W_SUBSET (+ sum and L2 norm) only."""
    return (NAMES[6],) if block == 0 else (NAMES[0], NAMES[6])


def golden_case(bias, mode):
    """The seeded case of tests/golden/nets_train_*.npz: ctx_ref64.head_case's blocks behind the prior nets of `net_case`.
    Returns `(Q, st, None, go, nets)` with `nets` = {net: (cb [N,8|20,h,w] float32 numpy, (q0, q1))} for the enabled nets in
    concat order; `mode` "repeat": frame 0 of the prior, N times."""
    Q, st, _, go = X.head_case(tuple(bias), GOLDEN_SHAPE, GOLDEN_T)
    nets = {}
    for net, on in zip(NETS, bias[:2]):
        if on:
            cb, qs, _ = net_case(net, GOLDEN_SHAPE)
            if mode == "repeat":
                cb = np.repeat(cb[:1], GOLDEN_SHAPE[0], 0)
            nets[net] = (cb, qs)
    return Q, st, None, go, nets


def golden_digest(Q, st, go, nets):
    import train_ref64 as R
    arrays = [st, go]
    for key in sorted(Q):
        arrays += [Q[key][k] for k in sorted(Q[key])]
    for net in sorted(nets):
        cb, qs = nets[net]
        arrays.append(cb)
        for q in qs:
            arrays += [q[k] for k in sorted(q)]
    return R.digest(*arrays)


def golden_ref(bias, mode, summed=False):
    """The float64 closed form of what the goldens hold: `(g_cb [N,64 k,h,w], {net: {"0": {...}, "1": {...}}})`.  `summed` (only
    for "repeat"): the static-priors form of train.recurrence_step -- each net's slice of g_cb summed over the N frames, then the
    backward on ONE frame -- instead of the backward over the N copies."""
    Q, st, _, go, nets = golden_case(bias, mode)
    t64 = lambda a: torch.as_tensor(a, dtype=torch.float64)      # noqa: E731
    Pf = X.folds(Q)
    Pn = {net: [BR.fold(BR.to64(q)) for q in qs] for net, (cb, qs) in nets.items()}
    pri = torch.cat([net_forward(Pn[net], t64(cb)) for net, (cb, qs) in nets.items()], 1)
    hd = X.head_forward(Pf, t64(st), pri, GOLDEN_T, use_ctx=bool(bias[2]))
    gfu = X.input_grad_ref(Pf["fucbst"], hd["fu"], t64(go), 1, False)
    g_cb = X.input_grad_ref(Pf["fucb"], hd["cbcat"], gfu[:, 256:], 1, hd["cbcat"].shape[1] == 64)
    grads = {}
    for i, (net, (cb, qs)) in enumerate(nets.items()):
        g, c = g_cb[:, 64 * i:64 * i + 64], t64(cb)
        if summed:
            assert mode == "repeat"
            g, c = g.sum(0, keepdim=True), c[:1]
        grads[net] = net_param_grads(Pn[net], c, g)
    return g_cb, grads
