"""Float64 restatement of the input gradients of the frozen context-prior path (train.block_input_grad / fust_output_grad,
csrc/train_ctx.hip: uavsal_ir_bwd_s2, uavsal_bilinear_ac_bwd, uavsal_tsum_bwd), the seeded inputs of their tests and the
per-element bounds, in the convention of tests/block_ref64.py:

    |kernel - ref| <= bound,      U = 2^-24, LAMBDA = 8, EPS = 8 U (tests/plan_ref64.py),  D = 2^-53

uavsal_ir_bwd_s2 (handed the stored gd, d, e): (LAMBDA * 2 + 3) U on the absolute-value chain: a sum of at most 4 products
  (LAMBDA sqrt(4); an input pixel receives 1, 2 or 4 taps), the stored gd (U), the tap product's and the s2 product's
  rounding (2 U).  block_ref64's count for stride 1 with 4 in place of 9.
uavsal_bilinear_ac_bwd: the reference is the transpose of the EXACT interpolation matrix (float64 coordinates o (i-1)/(o-1));
  the kernel forms the forward's fp32 coordinates.  An fp32 coordinate is within 2 U pos of the exact one (the scale and the
  product are rounded once each), which moves weight between the two neighbours of the sample -- or, when the coordinate
  falls on the other side of an integer, between a neighbour and the next source pixel, by the same amount.  So a weight
  w[o][s] carries 2 U pos(o) on every source pixel within one step of the sample, + 2 U for ly = fy - y0 and hy = 1 - ly;
  the product wy wx and the sum are formed in double (n D on the absolute sum), the result is rounded once (EPS):
      bound = sum_o (cy[o][sy] Wx[ox][sx] + Wy[oy][sy] cx[ox][sx] + cy cx) |g| + EPS |gin|,   c = 2 U (pos + 1) on |s - pos| < 2
  This is plan_ref64.bilinear_ac's coordinate term X, transposed.
uavsal_tsum_bwd: one fp32 addition, exactly torch's: compared for equality.
block_input_grad (the device recomputes e and d): `input_grad_e2e`, the construction of block_ref64.block_e2e for stride 1 or
  2 and any channel counts: the regular bound (the Co -> Ch GEMM, the depthwise backward, the Ch -> Cin GEMM, each on the
  absolute-value chain), the `undecided` term of every e and d element whose float64 pre-activation lies within its forward
  bound of a clamp, and `go_err`, a bound on the incoming gradient's own error carried through the absolute-value chain
  (that is how `fust_output_grad_ref` composes the path's bound stage by stage).
The composed bound is rigorous and worthless: the absolute-value chain of each of these blocks is ~100 times its value (1536
hidden channels of both signs), so three blocks in a row turn the first stage's 1e-3 into more than the gradient itself.
The GPU tests therefore hold the path STAGE BY STAGE (`path_stages(given=...)`): every stage, handed in float64 what the
device handed it in fp32, must be within its own bound -- the teacher-forced convention of the kernel tests, one level up.
No factor is fitted to what a kernel gives.

A border pixel of the resize (y0 == y1 = Hi - 1) is read with hy + ly.  In exact arithmetic ly is 0 there, so an adjoint that
adds only hy equals the right one; in fp32 ly is at most one step of fy there, below the coordinate term above.  The
float64 reference therefore cannot tell the two apart (`border_once_is_invisible`); what it does tell apart is an adjoint
that DROPS the border pixel or counts its whole weight twice (`bilinear_bwd_ref(variant=...)`).

Every function takes and returns float64 tensors on the device of its inputs unless it says numpy."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import block_ref64 as BR
import decoder_ref64 as DR
from plan_ref64 import EPS, LAMBDA, U, rtol

D = DR.D
NAMES = BR.NAMES
S2_SHAPES = [(1, 1, 1, 64), (1, 2, 3, 64), (2, 5, 6, 64), (2, 45, 80, 1536), (2, 23, 40, 384)]          # (n, H, W, C)
BIL_SHAPES = [((12, 20), (45, 80)), ((3, 4), (9, 16)), ((2, 2), (5, 6)), ((3, 5), (3, 5)), ((1, 1), (3, 4))]
# frame maps of 4 output images: name -> (src_mod, src_div, n_src)
MAPS = {"tile": (2, 1, 2), "clip": (4, 2, 2), "plain": (4, 1, 4)}
# frozen blocks of the path: name -> (cin, hid, cout, stride)
BLOCKS = {"fucb192": (192, 1152, 64, 1), "fucb128": (128, 768, 64, 1), "fucb64": (64, 384, 64, 1),
          "ctx0": (256, 1536, 64, 2), "ctx1": (64, 384, 64, 2), "fust": (256, 1536, 256, 1), "fucbst": (320, 1920, 256, 1)}
FROZEN = ("fucb192", "fucb128", "fucb64", "ctx0", "ctx1")                 # what block_input_grad meets in the path
BLOCK_SHAPES = [(2, 45, 80), (2, 23, 40), (1, 3, 5)]                      # (n, H, W) of the block's INPUT


def down(v):
    return (v - 1) // 2 + 1


def _v(t):
    return t.reshape(1, -1, 1, 1)


def m6(t):
    return (t > 0) & (t < 6)


# ------------------------------------------------------------------------------------------------ uavsal_ir_bwd_s2
def s2_case(shape, seed=0):
    """Teacher-forced inputs of uavsal_ir_bwd_s2, float32 numpy NCHW: `(gd, d [n,C,Ho,Wo], e [n,C,H,W], wd [C,1,3,3], s2 [C])`.
    e and d are ReLU6 outputs of N(3, 3) pre-activations: about 16 % of each sit on either clamp."""
    n, H, W, C = shape
    rs = np.random.RandomState(9000 + seed + n * H * W + C)
    Ho, Wo = down(H), down(W)
    e = np.clip(3.0 + 3.0 * rs.standard_normal((n, C, H, W)), 0, 6).astype(np.float32)
    d = np.clip(3.0 + 3.0 * rs.standard_normal((n, C, Ho, Wo)), 0, 6).astype(np.float32)
    gd = rs.standard_normal((n, C, Ho, Wo)).astype(np.float32)
    wd = (rs.standard_normal((C, 1, 3, 3)) / 3.0).astype(np.float32)
    s2 = (rs.choice([-1.0, 1.0], C) * (0.5 + 1.5 * rs.random_sample(C))).astype(np.float32)
    return gd, d, e, wd, s2


def ir_bwd_s2_ref(wd, s2, gd, d, e, variant=None, absolute=False):
    """uavsal_ir_bwd_s2 from the stored gd, d, e: `ga [n,C,H,W]`; `absolute`: the same chain on absolute values.
    `variant` "stride1_parity" (a WRONG kernel): the taps an input pixel receives are chosen as on an unpadded grid,
    (y - ky) even with oy = (y - ky) / 2 -- the parity rule of uavsal_ir_bwd's patch (input pixel 2 ty + a reads tap row a
    of output ty) carried over to stride 2 without the padding's shift."""
    a = (lambda t: t.abs()) if absolute else (lambda t: t)
    C = d.shape[1]
    H, W = e.shape[2:]
    d2 = a(gd) * m6(d)
    if variant == "stride1_parity":
        back = F.conv_transpose2d(d2, a(wd), stride=2, padding=0, groups=C)[:, :, :H, :W]
        back = F.pad(back, (0, W - back.shape[3], 0, H - back.shape[2]))
    else:
        op = (H - (2 * d.shape[2] - 1), W - (2 * d.shape[3] - 1))
        back = F.conv_transpose2d(d2, a(wd), stride=2, padding=1, output_padding=op, groups=C)
    return back * _v(a(s2)) * m6(e)


def ir_bwd_s2_bound(wd, s2, gd, d, e):
    return (LAMBDA * 2 + 3) * U * ir_bwd_s2_ref(wd, s2, gd, d, e, absolute=True)


def ir_bwd_s2_formula(wd, s2, gd, d, e):
    """The formula of include/uavsal_hip.h written out tap by tap (slow: small shapes), to hold `ir_bwd_s2_ref` against."""
    n, C, H, W = e.shape
    Ho, Wo = d.shape[2:]
    d2 = gd * m6(d)
    ga = torch.zeros_like(e)
    for y in range(H):
        for x in range(W):
            for ky in range(3):
                for kx in range(3):
                    if (y + 1 - ky) % 2 or (x + 1 - kx) % 2:
                        continue
                    oy, ox = (y + 1 - ky) // 2, (x + 1 - kx) // 2
                    if 0 <= oy < Ho and 0 <= ox < Wo:
                        ga[:, :, y, x] += wd[:, 0, ky, kx] * d2[:, :, oy, ox]
    return ga * _v(s2) * m6(e)


# ------------------------------------------------------------------------------------------------ uavsal_bilinear_ac_bwd
def bil_case(hw_in, hw_out, C=64, n_out=4, seed=0):
    """`g [n_out,C,Ho,Wo]` float32 numpy, N(0, 1)."""
    rs = np.random.RandomState(9500 + seed + hw_in[0] * hw_in[1] + 7 * hw_out[0] * hw_out[1])
    return rs.standard_normal((n_out, C) + tuple(hw_out)).astype(np.float32)


def _axis(o, i, device, variant=None):
    """`(W [o, i], c [o, i])`: the exact interpolation matrix of one axis and the coordinate term of its entries."""
    sc = (i - 1) / (o - 1) if o > 1 else 0.0
    pos = torch.arange(o, dtype=torch.float64, device=device) * sc
    i0 = pos.floor().long().clamp(0, i - 1)
    i1 = (i0 + 1).clamp(max=i - 1)
    lam = pos - i0.double()
    Wm = torch.zeros(o, i, dtype=torch.float64, device=device)
    rows = torch.arange(o, device=device)
    border = i0 == i1
    if variant == "border_dropped":                          # a WRONG kernel: an output that samples the last source pixel is lost
        keep = (~border).double()
        Wm[rows, i0] += (1 - lam) * keep
        Wm[rows, i1] += lam * keep
    elif variant == "border_twice":                          # a WRONG kernel: hy for y0 and hy again for y1
        Wm[rows, i0] += 1 - lam
        Wm[rows, i1] += torch.where(border, 1 - lam, lam)
    else:
        Wm[rows, i0] += 1 - lam
        Wm[rows, i1] += lam
    src = torch.arange(i, dtype=torch.float64, device=device)
    c = 2 * U * (pos.view(-1, 1) + 1) * ((src.view(1, -1) - pos.view(-1, 1)).abs() < 2).double()
    if i == 1:
        c = torch.zeros_like(c)                              # one source pixel: every weight is exactly 1
    return Wm, c


def bilinear_bwd_ref(g, n_src, hi, wi, src_mod, src_div, variant=None, bounds=False):
    """The adjoint of the align_corners resize with the frame map: `gin [n_src,C,hi,wi]` (`bounds`: `(gin, bound)`).
    `variant`: "border_dropped" / "border_twice" (see `_axis`), "clip_map": the clip map (n // T) where `src_mod`, `src_div`
    say otherwise."""
    n_out, C, ho, wo = g.shape
    Wy, cy = _axis(ho, hi, g.device, variant)
    Wx, cx = _axis(wo, wi, g.device, variant)
    src = [(k % src_mod) // src_div for k in range(n_out)]
    if variant == "clip_map":
        T = n_out // n_src
        src = [k // T for k in range(n_out)]
    gin = g.new_zeros((n_src, C, hi, wi))
    bnd = g.new_zeros((n_src, C, hi, wi))
    for k, s in enumerate(src):
        gin[s] += torch.einsum("oy,coq,qx->cyx", Wy, g[k], Wx)
        if bounds:
            ga = g[k].abs()
            bnd[s] += (torch.einsum("oy,coq,qx->cyx", cy, ga, Wx) + torch.einsum("oy,coq,qx->cyx", Wy, ga, cx)
                       + torch.einsum("oy,coq,qx->cyx", cy, ga, cx) + n_out * ho * wo * D * torch.einsum("oy,coq,qx->cyx", Wy, ga, Wx))
    return (gin, bnd + EPS * gin.abs()) if bounds else gin


def bilinear_fwd_ref(x, ho, wo, src_mod, src_div, n_out):
    """F.interpolate(align_corners=True) + the frame map, float64: `[n_out,C,ho,wo]`."""
    src = [(k % src_mod) // src_div for k in range(n_out)]
    return F.interpolate(x[src], size=(ho, wo), mode="bilinear", align_corners=True)


def border_once_is_invisible(hi, ho):
    """True when, in exact arithmetic, every output row whose y0 == y1 has ly == 0 (module docstring)."""
    from fractions import Fraction
    for o in range(ho):
        pos = Fraction(o * (hi - 1), ho - 1) if ho > 1 else Fraction(0)
        i0 = min(pos.numerator // pos.denominator, hi - 1)
        if i0 == hi - 1 and pos - i0 != 0:
            return False
    return True


# ------------------------------------------------------------------------------------------------ frozen blocks
def calibrated(name, x, rs, st, gain=1.0, shift=0.0):
    """The MODULE numbers q (float32 numpy, block_ref64's keys) of block `name` calibrated on ITS input `x` (float64 tensor):
    kaiming weights and BatchNorms under which the pre-activations of both ReLU6s have std 3 and mean 1.5 + N(0, 1) per channel
    and the output mean 0 and std 1, with decoder_ref64.bn_stats' running statistics.  `rs`, `st`: the RandomStates of the
    weights and of the statistics."""
    cin, hid, cout, stride = BLOCKS[name]
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
    pre = F.conv2d(e, torch.as_tensor(p["wd"]).double(), padding=1, stride=stride, groups=hid)
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


def block_case(name, shape, gain=1.0, shift=0.0, seed=0):
    """`(x [n,Cin,H,W] uniform in [0, 3), q, go [n,Co,Ho,Wo])` float32 numpy for the block `name` of BLOCKS, `calibrated` on
    that x.  `gain`, `shift`: tests/saturate_bn.py's change of the two BatchNorms in front of a ReLU6 (gamma times gain, beta
    plus shift) applied afterwards: more of both tensors sits on the upper clamp."""
    cin, hid, cout, stride = BLOCKS[name]
    n, H, W = shape
    base = 9900 + seed + 13 * sorted(BLOCKS).index(name) + n * H * W
    rs = np.random.RandomState(base)
    x = (3.0 * rs.random_sample((n, cin, H, W))).astype(np.float32)
    Ho, Wo = ((H - 1) // stride + 1, (W - 1) // stride + 1)
    go = (rs.standard_normal((n, cout, Ho, Wo)) / (Ho * Wo)).astype(np.float32)
    q = calibrated(name, torch.as_tensor(x, dtype=torch.float64), rs, np.random.RandomState(base + 4000), gain, shift)
    return x, q, go


def head_case(bias, shape, T, seed=0):
    """The part of the model behind the ST blocks with every block calibrated on the activations it really sees.  `bias`:
    (gauss, observed, context) flags; `shape` (N, h, w) with N a multiple of T.  Returns `(Q, st, priors, go)`: the blocks'
    numbers keyed fust, fucbst, fucb, ctx0, ctx1 (float32 numpy), the input `st` [N,256,h,w], the prior nets' outputs
    [N,64 k,h,w] (None without one) and the gradient that arrives at fucbst's output [N,256,h,w] (float32 numpy)."""
    N, h, w = shape
    k = int(bias[0]) + int(bias[1])
    base = 12000 + seed + N * h * w + 7 * (4 * bias[0] + 2 * bias[1] + bias[2])
    rs, stt = np.random.RandomState(base), np.random.RandomState(base + 4000)
    st = (3.0 * rs.random_sample((N, 256, h, w))).astype(np.float32)
    priors = (3.0 * rs.random_sample((N, 64 * k, h, w))).astype(np.float32) if k else None
    go = (rs.standard_normal((N, 256, h, w)) / (h * w)).astype(np.float32)
    Q = {}
    t64 = lambda a: torch.as_tensor(a, dtype=torch.float64)      # noqa: E731
    Q["fust"] = calibrated("fust", t64(st), rs, stt)
    f = forward(BR.fold(BR.to64(Q["fust"])), t64(st), 1, True)["o"]
    parts = [t64(priors)] if k else []
    if bias[2]:
        c = f.view(N // T, T, 256, h, w).sum(1)
        Q["ctx0"] = calibrated("ctx0", c, rs, stt)
        c1 = forward(BR.fold(BR.to64(Q["ctx0"])), c, 2, False)["o"]
        Q["ctx1"] = calibrated("ctx1", c1, rs, stt)
        c2 = forward(BR.fold(BR.to64(Q["ctx1"])), c1, 2, False)["o"]
        # the prior maps are ReLU-free block outputs of mean 0 and std 1; the slice is brought to [0, 3)-like size by the
        # calibration of fucb below, whatever its scale
        parts.append(F.interpolate(c2, size=(h, w), mode="bilinear", align_corners=True).repeat(T, 1, 1, 1))
    cbcat = torch.cat(parts, 1)
    name = "fucb%d" % cbcat.shape[1]
    Q["fucb"] = calibrated(name, cbcat, rs, stt)
    cb = forward(BR.fold(BR.to64(Q["fucb"])), cbcat, 1, cbcat.shape[1] == 64)["o"]
    Q["fucbst"] = calibrated("fucbst", torch.cat([f, cb], 1), rs, stt)
    return Q, st, priors, go


GOLDEN_BIAS, GOLDEN_SHAPES, GOLDEN_T = [(1, 1, 1), (0, 0, 1)], [(4, 5, 7), (4, 12, 20)], 2      # tests/golden/fust_*.npz


def golden_name(bias, shape):
    return "fust_b%d%d%d_N%d_%dx%d" % (tuple(bias) + tuple(shape))


def head_digest(Q, st, priors, go):
    import train_ref64 as R
    arrays = [st, go] + ([priors] if priors is not None else [])
    for key in sorted(Q):
        arrays += [Q[key][k] for k in sorted(Q[key])]
    return R.digest(*arrays)


def folds(Q, device="cpu"):
    return {k: BR.fold(BR.to64(q, device)) for k, q in Q.items()}


def make_block(name, q, dwBlock):
    """The numbers of `block_case` in a `dwBlock` (the package's or the reference's), eval mode."""
    cin, hid, cout, stride = BLOCKS[name]
    blk = dwBlock(cin, cout, kernel_size=3, stride=stride)
    return BR.load_block(blk, q)


def fold_module(block):
    """The eval fold of a dwBlock with an expand conv, from the MODULE's tensors in float64 (any BatchNorm eps):
    {w1, wd, w3, s*, b*, r*, mu*} -- what `block_ref64.fold` gives for the numbers of a case."""
    seq = block.conv
    p = {"w1": seq[0][0].weight.detach().double(), "wd": seq[1][0].weight.detach().double(), "w3": seq[2].weight.detach().double()}
    for i, bn in ((1, seq[0][1]), (2, seq[1][1]), (3, seq[3])):
        r = 1.0 / torch.sqrt(bn.running_var.detach().double() + bn.eps)
        p["r%d" % i], p["mu%d" % i] = r, bn.running_mean.detach().double()
        p["s%d" % i] = bn.weight.detach().double() * r
        p["b%d" % i] = bn.bias.detach().double() - p["mu%d" % i] * p["s%d" % i]
    return p


def q_of_module(block):
    """A module's numbers in the form `block_ref64.param_grads` takes (its fold assumes eps = BN_EPS: the variance is shifted
    so that r is the module's)."""
    seq = block.conv
    q = {"w1": seq[0][0].weight.detach().double(), "wd": seq[1][0].weight.detach().double(), "w3": seq[2].weight.detach().double()}
    for i, bn in ((1, seq[0][1]), (2, seq[1][1]), (3, seq[3])):
        q["g%d" % i], q["be%d" % i] = bn.weight.detach().double(), bn.bias.detach().double()
        q["mu%d" % i] = bn.running_mean.detach().double()
        q["var%d" % i] = bn.running_var.detach().double() + bn.eps - BR.BN_EPS
    return q


def forward(p, x, stride, res):
    """`p`: the eval fold as float64 tensors.  Returns dict(e_pre, e, d_pre, d, o)."""
    hid = p["w1"].shape[0]
    e_pre = F.conv2d(x, p["w1"]) * _v(p["s1"]) + _v(p["b1"])
    e = e_pre.clamp(0, 6)
    d_pre = F.conv2d(e, p["wd"], padding=1, stride=stride, groups=hid) * _v(p["s2"]) + _v(p["b2"])
    d = d_pre.clamp(0, 6)
    o = F.conv2d(d, p["w3"]) * _v(p["s3"]) + _v(p["b3"])
    return {"e_pre": e_pre, "e": e, "d_pre": d_pre, "d": d, "o": o + x if res else o}


def forward_bound(p, x, stride):
    """A per-element bound on the block's output (without the residual) when the device computes it by three launches: the
    forward chain rule of plan_ref64 (ReLU6 is 1-Lipschitz, so an input error passes a clamp unchanged at most)."""
    f = forward(p, x, stride, False)
    hid, cin = p["w1"].shape[:2]
    w1a, wda, w3a = p["w1"].abs(), p["wd"].abs(), p["w3"].abs()
    be_pre = F.conv2d(x.abs(), w1a) * _v(p["s1"].abs()) + _v(p["b1"].abs())
    err_e = rtol("f32", cin) * be_pre + EPS * 2 * f["e_pre"].abs()
    bd_pre = F.conv2d(be_pre, wda, padding=1, stride=stride, groups=hid) * _v(p["s2"].abs()) + _v(p["b2"].abs())
    err_d = (rtol("f32", cin) + rtol("f32", 9)) * bd_pre + EPS * 2 * f["d_pre"].abs()
    bo = F.conv2d(f["d"].abs() + err_d, w3a) * _v(p["s3"].abs()) + _v(p["b3"].abs())
    return F.conv2d(err_d, w3a) * _v(p["s3"].abs()) + rtol("f32", hid) * bo + EPS * 2 * f["o"].abs()


def _dw_back(t, wd, stride, hw):
    """The transposed depthwise 3x3 (padding 1) back to a map of size `hw`."""
    H, W = hw
    if stride == 1:
        return F.conv_transpose2d(t, wd, padding=1, groups=wd.shape[0])
    op = (H - (2 * t.shape[2] - 1), W - (2 * t.shape[3] - 1))
    return F.conv_transpose2d(t, wd, stride=2, padding=1, output_padding=op, groups=wd.shape[0])


def input_grad_ref(p, x, go, stride, res, variant=None):
    """grad_x of the frozen block in float64 closed form.  `variant` "stride1_parity": `ir_bwd_s2_ref`'s wrong kernel."""
    f = forward(p, x, stride, False)
    gd = F.conv_transpose2d(go * _v(p["s3"]), p["w3"])
    if stride == 2:
        ga = ir_bwd_s2_ref(p["wd"], p["s2"], gd, f["d"], f["e"], variant=variant)
    else:
        ga = BR.ir_bwd_ref(p, gd, f["d"], f["e"])
    gx = F.conv_transpose2d(ga * _v(p["s1"]), p["w1"])
    return gx + go if res else gx


def input_grad_autograd(p, x, go, stride, res):
    xx = x.detach().clone().requires_grad_(True)
    (g,) = torch.autograd.grad(forward(p, xx, stride, res)["o"], xx, go)
    return g


def input_grad_e2e(p, x, go, stride, res, go_err=None):
    """grad_x when the DEVICE recomputes e and d: `(grad_x, bound, undecided)`, block_ref64.block_e2e for any stride and
    channel counts.  `go_err`: a per-element bound on the error of the `go` the device is handed (default: exact)."""
    f = forward(p, x, stride, res)
    hid, cin = p["w1"].shape[:2]
    cout = p["w3"].shape[0]
    hw = x.shape[2:]
    taps = 9 if stride == 1 else 4
    w1a, wda, w3a = p["w1"].abs(), p["wd"].abs(), p["w3"].abs()
    be_pre = F.conv2d(x.abs(), w1a) * _v(p["s1"].abs()) + _v(p["b1"].abs())
    err_e = rtol("f32", cin) * be_pre + EPS * 2 * f["e_pre"].abs()
    bd_pre = F.conv2d(be_pre, wda, padding=1, stride=stride, groups=hid) * _v(p["s2"].abs()) + _v(p["b2"].abs())
    err_d = (rtol("f32", cin) + rtol("f32", 9)) * bd_pre + EPS * 2 * f["d_pre"].abs()
    near = lambda pre, err: ((pre.abs() <= err) | ((pre - 6).abs() <= err)).double()      # noqa: E731
    ue, ud = near(f["e_pre"], err_e), near(f["d_pre"], err_d)
    e, d = f["e"], f["d"]
    me, md = m6(e).double(), m6(d).double()
    gd = F.conv_transpose2d(go * _v(p["s3"]), p["w3"])
    gd_abs = F.conv_transpose2d(go.abs() * _v(p["s3"].abs()), w3a)
    ga = _dw_back(gd * md, p["wd"], stride, hw) * _v(p["s2"]) * me
    ga_abs = _dw_back(gd_abs * md, wda, stride, hw) * _v(p["s2"].abs()) * me
    grad_x = F.conv_transpose2d(ga * _v(p["s1"]), p["w1"])
    rel = (rtol("f32", cout) + U + 2 * EPS) + (LAMBDA * math.sqrt(taps) + 2) * U + (rtol("f32", hid) + U)
    bound = rel * F.conv_transpose2d(ga_abs * _v(p["s1"].abs()), w1a) + EPS * grad_x.abs()
    if go_err is not None:                                       # the incoming error, through the absolute-value chain
        gde = F.conv_transpose2d(go_err * _v(p["s3"].abs()), w3a)
        bound = bound + F.conv_transpose2d(_dw_back(gde * md, wda, stride, hw) * _v(p["s2"].abs()) * me * _v(p["s1"].abs()), w1a)
    if res:
        grad_x = grad_x + go
        bound = bound + EPS * (go.abs() + grad_x.abs()) + (go_err if go_err is not None else 0)
    gtot = gd.abs() + (F.conv_transpose2d(go_err * _v(p["s3"].abs()), w3a) if go_err is not None else 0)
    from_d = _dw_back(gtot * ud, wda, stride, hw) * _v(p["s2"].abs()) * me
    from_e = _dw_back(gtot * md, wda, stride, hw) * _v(p["s2"].abs()) * ue
    undecided = F.conv_transpose2d((from_d + from_e) * _v(p["s1"].abs()), w1a)
    return grad_x, bound, undecided


# ------------------------------------------------------------------------------------------------ the whole path
def head_forward(P, st, priors, T, use_ctx=True, ctx_map="tile"):
    """The reference's model.py:344-365 behind the ST blocks, float64.  `P`: dict of folds {fust, fucbst, fucb, ctx0, ctx1};
    `st` [N,256,h,w]; `priors` [N,64 k,h,w] or None: the prior nets' outputs (k = 0..2).  Returns dict(f, fu, cbcat, o)."""
    return tail_forward(P, forward(P["fust"], st, 1, True)["o"], priors, T, use_ctx, ctx_map)


def tail_forward(P, f, priors, T, use_ctx=True, ctx_map="tile"):
    """`head_forward` from fust_layer's output `f` [N,256,h,w] on."""
    N, _, h, w = f.shape
    parts = [] if priors is None else [priors]
    if use_ctx:
        B = N // T
        c = f.view(B, T, 256, h, w).sum(1)
        c1 = forward(P["ctx0"], c, 2, False)["o"]
        c2 = forward(P["ctx1"], c1, 2, False)["o"]
        up = F.interpolate(c2, size=(h, w), mode="bilinear", align_corners=True)
        up = up.repeat(T, 1, 1, 1) if ctx_map == "tile" else up.repeat_interleave(T, 0)      # model.py:361 / the clip map
        parts.append(up)
    cbcat = torch.cat(parts, 1)
    cb = forward(P["fucb"], cbcat, 1, cbcat.shape[1] == 64)["o"]
    fu = torch.cat([f, cb], 1)
    return {"f": f, "fu": fu, "cbcat": cbcat, "o": forward(P["fucbst"], fu, 1, False)["o"]}


def path_stages(P, fu, cbcat, gfu, T, n_prior, given=None):
    """The stages of train.fust_output_grad, each in float64 with ITS OWN bound: dict g_cb -> (g, bound, undecided), g_ctx2 ->
    (g, bound), g_ctx1, g_sum -> (g, bound, undecided), g -> the result, ctx_sum, ctx1.  `given`: a dict of float64 tensors
    g_cb, g_ctx2, g_ctx1, g_sum, ctx1 (what the device handed each NEXT stage, `parts` of fust_output_grad): a stage then reads
    the given tensor in place of the float64 result of the stage before it -- the teacher-forced form the GPU test uses."""
    given = given or {}
    N, _, h, w = fu.shape
    B = N // T
    S = {}
    S["g_cb"] = input_grad_e2e(P["fucb"], cbcat, gfu[:, 256:], 1, cbcat.shape[1] == 64)
    sl = slice(64 * n_prior, 64 * n_prior + 64)
    S["g_ctx2"] = bilinear_bwd_ref(given.get("g_cb", S["g_cb"][0])[:, sl], B, down(down(h)), down(down(w)), B, 1, bounds=True)
    S["ctx_sum"] = fu[:, :256].reshape(B, T, 256, h, w).sum(1)
    S["ctx1"] = forward(P["ctx0"], S["ctx_sum"], 2, False)["o"]
    S["g_ctx1"] = input_grad_e2e(P["ctx1"], given.get("ctx1", S["ctx1"]), given.get("g_ctx2", S["g_ctx2"][0]), 2, False)
    S["g_sum"] = input_grad_e2e(P["ctx0"], S["ctx_sum"], given.get("g_ctx1", S["g_ctx1"][0]), 2, False)
    S["g"] = gfu[:, :256] + given.get("g_sum", S["g_sum"][0]).repeat_interleave(T, 0)        # frame b T + t <- chunk b
    return S


def fust_output_grad_ref(P, fu, cbcat, gfu, T, n_prior, gfu_err=None, variant=None):
    """train.fust_output_grad in float64 closed form from the float64 `fu` [N,320,h,w], `cbcat` [N,64 k,h,w] and `gfu` =
    d loss / d fu: `(g [N,256,h,w], bound, undecided)`, the bound composed stage by stage (`input_grad_e2e(go_err=...)`, the
    resize's, U on the final addition).  `n_prior`: prior nets in front of the context slice (0..2).
    `variant`: "direct_only", "clip_map" (WRONG kernels)."""
    N, _, h, w = fu.shape
    B = N // T
    g_dir = gfu[:, :256]
    e_dir = gfu_err[:, :256] if gfu_err is not None else torch.zeros_like(g_dir)
    if variant == "direct_only":
        return g_dir, e_dir + EPS * g_dir.abs(), torch.zeros_like(g_dir)
    res_cb = cbcat.shape[1] == 64
    g_cb, b_cb, u_cb = input_grad_e2e(P["fucb"], cbcat, gfu[:, 256:], 1, res_cb, gfu_err[:, 256:] if gfu_err is not None else None)
    sl = slice(64 * n_prior, 64 * n_prior + 64)
    h3, w3 = down(down(h)), down(down(w))
    mapv = "clip_map" if variant == "clip_map" else None
    g_c2, b_c2 = bilinear_bwd_ref(g_cb[:, sl], B, h3, w3, B, 1, variant=mapv, bounds=True)
    b_c2 = b_c2 + bilinear_bwd_ref((b_cb + u_cb)[:, sl], B, h3, w3, B, 1)
    csum = fu[:, :256].reshape(B, T, 256, h, w).sum(1)
    c1 = forward(P["ctx0"], csum, 2, False)["o"]
    g_c1, b_c1, u_c1 = input_grad_e2e(P["ctx1"], c1, g_c2, 2, False, b_c2)
    g_s, b_s, u_s = input_grad_e2e(P["ctx0"], csum, g_c1, 2, False, b_c1 + u_c1)
    rep = lambda t: t.repeat_interleave(T, 0)                    # noqa: E731  (frame b T + t <- chunk b)
    g = g_dir + rep(g_s)
    return g, e_dir + rep(b_s) + U * (g_dir.abs() + rep(g_s).abs()), rep(u_s)


def param_grads_abs(p, x, go_abs, e, d, me=None, md=None):
    """The absolute-value chain of block_ref64.param_grads: a per-element bound on the change of the nine gradients of a
    stride-1 block when its `go` changes by at most `go_abs` (masks `me`, `md`: default the strict masks of e and d)."""
    hid, cin = p["w1"].shape[:2]
    cout = p["w3"].shape[0]
    me = m6(e).double() if me is None else me
    md = m6(d).double() if md is None else md
    w1a, wda, w3a = p["w1"].abs().reshape(hid, cin), p["wd"].abs(), p["w3"].abs().reshape(cout, hid)
    gd = F.conv_transpose2d(go_abs * _v(p["s3"].abs()), p["w3"].abs())
    a2 = gd * md
    ga = F.conv_transpose2d(a2, wda, padding=1, groups=hid) * _v(p["s2"].abs()) * me
    G1 = torch.einsum("tchw,tjhw->cj", ga, x.abs())
    G3 = torch.einsum("tmhw,tchw->mc", go_abs, d.abs())
    S1, S2, S3 = ga.sum((0, 2, 3)), a2.sum((0, 2, 3)), go_abs.sum((0, 2, 3))
    Gd = DR._tap_sums(a2, e.abs())
    r1, r2, r3, mu1, mu2, mu3 = (p[k].abs() for k in ("r1", "r2", "r3", "mu1", "mu2", "mu3"))
    g = {NAMES[0]: (p["s1"].abs().view(-1, 1) * G1).reshape(hid, cin, 1, 1), NAMES[1]: r1 * ((w1a * G1).sum(1) + mu1 * S1),
         NAMES[2]: S1, NAMES[3]: (p["s2"].abs().view(-1, 1, 1) * Gd).reshape(hid, 1, 3, 3),
         NAMES[4]: r2 * ((wda.reshape(hid, 3, 3) * Gd).sum((1, 2)) + mu2 * S2), NAMES[5]: S2,
         NAMES[6]: (p["s3"].abs().view(-1, 1) * G3).reshape(cout, hid, 1, 1), NAMES[7]: r3 * ((w3a * G3).sum(1) + mu3 * S3),
         NAMES[8]: S3}
    return g


def param_grads_undecided(p, x, go, res=True):
    """A per-element bound on the change of the nine gradients of a stride-1 block when the device decides the masks of the
    e and d elements within their forward bound of a clamp the other way (`input_grad_e2e`'s `undecided`, for the parameter
    gradients): each such element removes or adds its whole term, and a changed e changes d within the same bound."""
    f = forward(p, x, 1, False)
    hid, cin = p["w1"].shape[:2]
    w1a, wda = p["w1"].abs(), p["wd"].abs()
    be_pre = F.conv2d(x.abs(), w1a) * _v(p["s1"].abs()) + _v(p["b1"].abs())
    err_e = rtol("f32", cin) * be_pre + EPS * 2 * f["e_pre"].abs()
    bd_pre = F.conv2d(be_pre, wda, padding=1, groups=hid) * _v(p["s2"].abs()) + _v(p["b2"].abs())
    err_d = (rtol("f32", cin) + rtol("f32", 9)) * bd_pre + EPS * 2 * f["d_pre"].abs()
    near = lambda pre, err: ((pre.abs() <= err) | ((pre - 6).abs() <= err)).double()      # noqa: E731
    ue, ud = near(f["e_pre"], err_e), near(f["d_pre"], err_d)
    e, d = f["e"], f["d"]
    me, md = m6(e).double(), m6(d).double()
    ga_ = param_grads_abs(p, x, go.abs(), e, d, me=ue, md=md)
    gb_ = param_grads_abs(p, x, go.abs(), e, d, me=torch.clamp(me + ue, max=1), md=ud)
    # the values of e and d themselves move within err_e, err_d: G3 = sum go d and Gd = sum delta2 e'
    gd = F.conv_transpose2d(go.abs() * _v(p["s3"].abs()), p["w3"].abs())
    dG3 = torch.einsum("tmhw,tchw->mc", go.abs(), err_d)
    dGd = DR._tap_sums(gd * md, err_e)
    out = {n: ga_[n] + gb_[n] for n in NAMES}
    cout = p["w3"].shape[0]
    out[NAMES[6]] = out[NAMES[6]] + (p["s3"].abs().view(-1, 1) * dG3).reshape(cout, hid, 1, 1)
    out[NAMES[7]] = out[NAMES[7]] + p["r3"].abs() * (p["w3"].abs().reshape(cout, hid) * dG3).sum(1)
    out[NAMES[3]] = out[NAMES[3]] + (p["s2"].abs().view(-1, 1, 1) * dGd).reshape(hid, 1, 3, 3)
    out[NAMES[4]] = out[NAMES[4]] + p["r2"].abs() * (wda.reshape(hid, 3, 3) * dGd).sum((1, 2))
    return out
