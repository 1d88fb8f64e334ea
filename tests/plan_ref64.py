"""Float64 references of every launch kind of the native plan, with per-element error bounds (tests/test_plan_ops_fp64.py).

Each reference takes the op's inputs as float64 NCHW tensors (engine.read_view) and the recorded torch modules, computes the
op with torch's own float64 operators (F.conv2d, matmul, elementwise) and returns `Ref(y, B, E, X)`:

    |kernel - y| <= rtol * B + EPS * E + X + atol          (element-wise)

* `B` is the same computation on absolute values: |input|, |weight|, |BN scale|, |BN bias|, |residual| (the size of the terms
  whose rounding the kernel's sums accumulate).  Through a chain of stages (expand -> depthwise -> project) B is carried as the
  abs-input of the next stage: an error e of an intermediate value reaches the output as at most |W| e (ReLU6 has Lipschitz
  constant 1), so the chain's error is at most (sum of the stages' rtol) * B.  A sigmoid has Lipschitz constant 1/4: B / 4.
  ConvTWA (i = sigmoid(z), out = i x + (1 - i) h):  B_out = |x - h| / 4 * B_z.  ConvLSTM: B_c = |c_prev| B_f / 4 +
  |tanh g| B_i / 4 + sigmoid(i) B_g,  B_h = |tanh c| B_o / 4 + sigmoid(o) B_c.
* `rtol(prec, K)` for a sum of K products in fp32:  LAMBDA * u * sqrt(K)  (u = 2^-24; the probabilistic bound of Higham & Mary,
  SIAM J. Sci. Comput. 41 (2019): |error| <= lambda sqrt(K) u sum|a_k b_k| fails with probability <= 2 exp(-lambda^2 / 2), which
  is ~1e-14 per element for lambda = 8), plus the representation error of the split 16-bit GEMMs, which adds linearly per
  product: f16x3 splits both operands into hi + lo fp16 with round-to-zero (each < 2^-20 relative) and drops lo * lo (< 2^-20),
  3 * 2^-20; bf16x3 the same with 8-bit mantissas, 3 * 2^-16 (a regression bound: bf16x3 is not a shipped precision).
* Winograd F(r x r, 3x3): B is not the direct convolution's but the Winograd chain on absolute values,
  |A^T| [ sum_c (|G| |g| |G^T|) .* (|B^T| |d| |B|) ] |A|  (exact per element, wino_abs), and rtol = (LAMBDA sqrt(Cin) + 20) u:
  the transforms add at most 8 (input) + 10 (output) roundings along any path, the filter transform one.  F(4x4) has larger
  transform coefficients than F(2x2); that is what its B carries.
* `E` scales the element-wise roundings of epilogues and transcendental functions (EPS = 8 u); `X` is an extra absolute term
  (bilinear: the source coordinate is computed in fp32, |d coord| <= 2 u coord, times the local slope of the map).
* atol: f16x3 underflows in the lo half (fp16 subnormals: 2^-24 of 16 x and of 64 w): 2^-28 |s| ||w||_1 + 2^-30 |s| K max|x|.
"""
import math
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

U = 2.0 ** -24
LAMBDA = 8.0
EPS = 8 * U
REP = {"f32": 0.0, "f16x3": 3 * 2.0 ** -20, "bf16x3": 3 * 2.0 ** -16}
SHADOW_REL, SHADOW_ABS = 2.0 ** -20, 2.0 ** -27     # split shadow (hi + lo, both round-to-zero) vs the fp32 value
ACT_NONE, ACT_RELU6, ACT_SIGMOID = 0, 1, 2
EPI_AFFINE, EPI_TWA, EPI_LSTM = 0, 1, 2


class Ref(NamedTuple):
    y: torch.Tensor
    B: torch.Tensor
    E: torch.Tensor
    X: Optional[torch.Tensor] = None
    rtol: float = 0.0
    atol: object = 0.0


def rtol(prec, k):
    return LAMBDA * U * math.sqrt(k) + REP[prec]


def bound(r: Ref):
    b = r.rtol * r.B + EPS * r.E
    if r.X is not None:
        b = b + r.X
    return b + (r.atol if r.atol is not None else 0.0)


def fold_bn(bn, device):
    """(scale, bias) of an eval BatchNorm in float64, or (None, None)."""
    if bn is None:
        return None, None
    if isinstance(bn, (list, tuple)):
        parts = [fold_bn(b_, device) for b_ in bn]
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    b = bn.bias.detach().double() - bn.running_mean.detach().double() * s
    return s.to(device), b.to(device)


def _w(conv, device, wslice=None, gate_interleave=0):
    w = torch.cat([c_.weight.detach() for c_ in conv], 0) if isinstance(conv, (list, tuple)) else conv.weight.detach()
    w = w.double()
    if wslice is not None:
        w = w[:, wslice[0]:wslice[1]]
    if gate_interleave:
        hid = gate_interleave
        w = w.reshape(4, hid, *w.shape[1:]).permute(1, 0, 2, 3, 4).reshape(4 * hid, *w.shape[1:])
    return w.to(device)


def _cb(conv, device, gate_interleave=0):
    """The conv's own bias (float64), if it has one."""
    convs = conv if isinstance(conv, (list, tuple)) else [conv]
    if all(c_.bias is None for c_ in convs):
        return None
    b = torch.cat([(c_.bias.detach() if c_.bias is not None else torch.zeros(c_.weight.shape[0])).double() for c_ in convs])
    if gate_interleave:
        b = b.reshape(4, gate_interleave).t().reshape(-1)
    return b.to(device)


def _vec(v):
    return v.view(1, -1, 1, 1)


def _pick_bias_channel(pre, b, act):
    """Output channel whose bias a mutation leaves out: the largest |bias| among channels the activation does not saturate
    everywhere (a ReLU6 at 0 or 6 would hide the change)."""
    if act == ACT_RELU6:
        live = ((pre > 0) & (pre < 6)).flatten(2).any(-1).any(0)
    else:
        live = torch.ones_like(b, dtype=torch.bool)
    return int(torch.argmax(b.abs() * live.double()))


def stage(v, B, w, s, b, act, stride=1, padding=0, dilation=1, groups=1, cbias=None, mut=None, pre=None):
    """One conv + affine + activation stage on (values, abs-bound) pairs (`mut`, `pre`: see activate)."""
    y = F.conv2d(v, w, stride=stride, padding=padding, dilation=dilation, groups=groups)
    yb = F.conv2d(B, w.abs(), stride=stride, padding=padding, dilation=dilation, groups=groups)
    if cbias is not None:
        y, yb = y + _vec(cbias), yb + _vec(cbias.abs())
    if s is not None:
        y, yb = y * _vec(s) + _vec(b), yb * _vec(s.abs()) + _vec(b.abs())
        if mut == "bias":
            c = _pick_bias_channel(y, b, act)
            y[:, c] -= b[c]
    return activate(y, yb, act, mut, pre)


def activate(y, yb, act, mut=None, pre=None):
    """`mut` = "no_hi": a ReLU6 loses its upper clamp (the wrong reference of a kernel that computes max(v, 0));
    `pre`: a list that receives the pre-activation of every ReLU6."""
    if act == ACT_RELU6:
        if pre is not None:
            pre.append(y)
        return (y.clamp(min=0.0) if mut == "no_hi" else y.clamp(0.0, 6.0)), yb
    if act == ACT_SIGMOID:
        return torch.sigmoid(y), yb / 4
    return y, yb


def mutate_input(x, mut):
    """(a) one input channel dropped (the one with the largest total magnitude), (b) the last input row zeroed."""
    if mut == "chan":
        x = x.clone()
        x[:, int(torch.argmax(x.abs().sum((0, 2, 3))))] = 0
    elif mut == "row":
        x = x.clone()
        x[:, :, -1, :] = 0
    return x


def _split_atol(prec, s, w, xmax, k):
    if prec != "f16x3":
        return 0.0
    wl1 = w.abs().flatten(1).sum(1)
    sc = s.abs() if s is not None else torch.ones_like(wl1)
    return _vec(sc * (2.0 ** -28 * wl1 + 2.0 ** -30 * k * xmax))


# ----------------------------------------------------------------------------------------------------------- GEMM-type ops
def ref_conv(rec, a, res=None, aux=None, mut=None, pre=None):
    """conv1 / conv3 launches: AFFINE (BN, act, residual), n_group, fused depthwise loader, TWA and LSTM epilogues.
    `a`: the A operand ([n, groups * Cin, H, W] for n_group; the expanded tensor for a fused depthwise), `res` / `aux` the
    epilogue operands (TWA: res = x_t, aux = the hoisted x half, h_{t-1} = a; LSTM: res = c_{t-1}, aux = the x half)."""
    dev = a.device
    prec, taps, act, epi = rec["prec"], rec["taps"], rec["act"], rec["epi"]
    gi = rec.get("gate_interleave", 0)
    w = _w(rec["conv"], dev, rec.get("wslice"), gi)
    cbias = _cb(rec["conv"], dev, gi) if rec.get("wslice") is None or rec["wslice"][0] == 0 else None
    s, b = fold_bn(rec["bn"], dev)
    pad = 1 if taps == 9 else 0
    x = mutate_input(a, mut if mut in ("chan", "row") else None)
    hi = mut if mut == "no_hi" else None
    B = a.abs()
    rt = 0.0
    if rec.get("dw") is not None:                         # depthwise 3x3 + BN + ReLU6 inside the loader
        dwc, dwbn, dstride = rec["dw"]
        ds, db = fold_bn(dwbn, dev)
        x, B = stage(x, B, _w(dwc, dev), ds, db, ACT_RELU6, stride=dstride, padding=1, groups=a.shape[1], mut=hi, pre=pre)
        rt += rtol("f32", 9)
    k = (w.shape[1]) * taps
    rt += rtol(prec, k)
    xmax = float(B.max()) if B.numel() else 0.0
    if rec.get("n_group"):
        ng, cin = rec["n_group"], rec["cin"]
        outs = [stage(x[:, g * cin:(g + 1) * cin], B[:, g * cin:(g + 1) * cin], w[g * ng:(g + 1) * ng], None, None, ACT_NONE)
                for g in range(w.shape[0] // ng)]
        y, yb = torch.cat([o[0] for o in outs], 1), torch.cat([o[1] for o in outs], 1)
        if s is not None:
            y, yb = y * _vec(s) + _vec(b), yb * _vec(s.abs()) + _vec(b.abs())
            if mut == "bias":
                c = _pick_bias_channel(y, b, act)
                y[:, c] -= b[c]
        y, yb = activate(y, yb, act, hi, pre)
    else:
        y, yb = stage(x, B, w, s, b, act if epi == EPI_AFFINE else ACT_NONE, padding=pad, cbias=cbias,
                      mut=mut if mut in ("bias", "no_hi") else None, pre=pre)
    atol = _split_atol(prec, s, w, xmax, k)
    if epi == EPI_AFFINE:
        E = y.abs()
        if res is not None:
            y, yb, E = y + res, yb + res.abs(), E + res.abs()
        return Ref(y, yb, E + y.abs(), None, rt, atol)
    if epi == EPI_TWA:
        return twa_update(y, yb, aux, res, a, rt, atol)
    if epi == EPI_LSTM:
        return lstm_update(y, yb, aux, res, rt, atol)
    raise ValueError("unknown epilogue %r" % (epi,))


def twa_update(acc, accb, pre, xt, h, rt, atol=0.0):
    """ConvTWA (model_convlstm.py:276-292): i = sigmoid(acc + pre), out = i x_t + (1 - i) h_{t-1}."""
    z, zb = acc + pre, accb + pre.abs()
    i = torch.sigmoid(z)
    y = i * xt + (1 - i) * h
    if not isinstance(atol, float):
        atol = atol * (xt - h).abs() / 4
    return Ref(y, (xt - h).abs() / 4 * zb, xt.abs() + h.abs() + y.abs() + (xt - h).abs(), None, rt, atol)


def lstm_update(acc, accb, pre, cprev, rt, atol=0.0):
    """ConvLSTM (model_convlstm.py:111-126) on gate-interleaved channels n = 4 c + gate, gates (i, f, o, g).
    Returns Ref of cat[h_t, c_t] on the channel axis."""
    z, zb = acc + pre, accb + pre.abs()
    n, c4, hh, ww = z.shape
    z, zb = z.view(n, c4 // 4, 4, hh, ww), zb.view(n, c4 // 4, 4, hh, ww)
    si, sf, so, tg = torch.sigmoid(z[:, :, 0]), torch.sigmoid(z[:, :, 1]), torch.sigmoid(z[:, :, 2]), torch.tanh(z[:, :, 3])
    c = sf * cprev + si * tg
    tc = torch.tanh(c)
    h = so * tc
    bc = cprev.abs() * zb[:, :, 1] / 4 + tg.abs() * zb[:, :, 0] / 4 + si * zb[:, :, 3]
    bh = tc.abs() * zb[:, :, 2] / 4 + so * bc
    ec = (sf * cprev).abs() + (si * tg).abs() + c.abs()
    eh = h.abs() + so * ec + (so * tc).abs()
    if not isinstance(atol, float):
        atol = atol.view(1, -1, 4, 1, 1).amax(2)
        atol = torch.cat([atol, atol], 1)
    return Ref(torch.cat([h, c], 1), torch.cat([bh, bc], 1), torch.cat([eh, ec], 1), None, rt, atol)


# Winograd transforms (Lavin & Gray 2016; G as packing.pack_wino_weight, B^T / A^T the matching interpolation points)
WINO = {
    2: ([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]],
        [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]],
        [[1, 1, 1, 0], [0, 1, -1, -1]]),
    4: ([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
         [0, 4, 0, -5, 0, 1]],
        [[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
         [0, 0, 1]],
        [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]),
}


def wino_conv(x, w, r, absolute=False):
    """3x3 / stride 1 / pad 1 convolution through the F(r x r, 3x3) transforms in float64 -- with `absolute`, every transform
    matrix, `x` and `w` taken by absolute value (the error scale of the Winograd chain; the CPU test checks that the signed
    form equals F.conv2d)."""
    bt, g, at = (torch.tensor(m_, dtype=torch.float64, device=x.device) for m_ in WINO[r])
    if absolute:
        bt, g, at, x, w = bt.abs(), g.abs(), at.abs(), x.abs(), w.abs()
    p = r + 2
    n, c, hh, ww = x.shape
    th, tw = (hh + r - 1) // r, (ww + r - 1) // r
    xp = F.pad(x, (1, tw * r + 1 - ww, 1, th * r + 1 - hh))
    tiles = xp.unfold(2, p, r).unfold(3, p, r)                       # [n, c, th, tw, p, p]
    v = torch.einsum("ip,ncxypq,jq->ijcnxy", bt, tiles, bt).reshape(p * p, c, n * th * tw)
    u = torch.einsum("ik,ockl,jl->ijoc", g, w, g).reshape(p * p, w.shape[0], c)
    m = torch.bmm(u, v).reshape(p, p, w.shape[0], n, th, tw)
    y = torch.einsum("ai,ijonxy,bj->noxayb", at, m, at).reshape(n, w.shape[0], th * r, tw * r)
    return y[:, :, :hh, :ww].contiguous()


def ref_wino(rec, a, twa=None, mut=None, pre=None):
    """Winograd triple (input transform, plane GEMM, output transform with BN / ReLU6 or the ConvTWA update), against the
    direct 3x3 convolution; `twa` = (x_t, pre) with h_{t-1} = a."""
    dev = a.device
    w = _w(rec["conv"], dev, rec.get("wslice"))
    s, b = fold_bn(rec["bn"], dev)
    x = mutate_input(a, mut if mut in ("chan", "row") else None)
    y = F.conv2d(x, w, padding=1)
    yb = wino_conv(a, w, rec["r"], absolute=True)
    cbias = _cb(rec["conv"], dev) if rec.get("wslice") is None or rec["wslice"][0] == 0 else None
    if cbias is not None:
        y, yb = y + _vec(cbias), yb + _vec(cbias.abs())
    rt = (LAMBDA * math.sqrt(w.shape[1]) + 20) * U
    if twa is not None:
        return twa_update(y, yb, twa[1], twa[0], a, rt)
    if s is not None:
        y, yb = y * _vec(s) + _vec(b), yb * _vec(s.abs()) + _vec(b.abs())
        if mut == "bias":
            c = _pick_bias_channel(y, b, rec["act"])
            y[:, c] -= b[c]
    y, yb = activate(y, yb, rec["act"], mut, pre)
    return Ref(y, yb, y.abs(), None, rt, 0.0)


# ------------------------------------------------------------------------------------------------------ depthwise family
def ref_dw(rec, a, mut=None, pre=None):
    """Depthwise 3x3 + BN + ReLU6, stride, dilation (pad = dilation), or channel groups with their own dilation."""
    dev = a.device
    x = mutate_input(a, mut if mut in ("chan", "row") else None)
    conv, bn, stride, dil = rec["conv"], rec["bn"], rec["stride"], rec["dilation"]
    if isinstance(conv, (list, tuple)):
        cg = a.shape[1] // len(conv)
        outs = [stage(x[:, i * cg:(i + 1) * cg], a[:, i * cg:(i + 1) * cg].abs(), _w(c_, dev), *fold_bn(b_, dev), ACT_RELU6,
                      padding=d_, dilation=d_, groups=cg, mut=mut if (mut == "bias" and i == 0) or mut == "no_hi" else None,
                      pre=pre)
                for i, (c_, b_, d_) in enumerate(zip(conv, bn, dil))]
        y, yb = torch.cat([o[0] for o in outs], 1), torch.cat([o[1] for o in outs], 1)
    else:
        y, yb = stage(x, a.abs(), _w(conv, dev), *fold_bn(bn, dev), ACT_RELU6, stride=stride, padding=dil, dilation=dil,
                      groups=a.shape[1], mut=mut if mut in ("bias", "no_hi") else None, pre=pre)
    if pre:                                               # (channel groups: one stage)
        pre[:] = [torch.cat(pre, 1)]
    return Ref(y, yb, y.abs(), None, rtol("f32", 9), 0.0)


def ref_dw_dot(rec, a, mut=None, pre=None):
    """Depthwise 3x3 + BN + ReLU6 -> projection to one channel + BN + act (conv_out_st)."""
    dev = a.device
    dwc, dwbn = rec["dw"]
    x = mutate_input(a, mut if mut in ("chan", "row") else None)
    hi = mut if mut == "no_hi" else None
    d, db = stage(x, a.abs(), _w(dwc, dev), *fold_bn(dwbn, dev), ACT_RELU6, padding=1, groups=a.shape[1], mut=hi, pre=pre)
    s, b = fold_bn(rec["bn"], dev)
    y, yb = stage(d, db, _w(rec["conv"], dev), s, b, ACT_NONE)
    if mut == "bias":
        y = y - b[0]
    y, yb = activate(y, yb, rec["act"], hi, pre)
    return Ref(y, yb, y.abs(), None, rtol("f32", 9) + rtol("f32", a.shape[1]), 0.0)


def ref_fused_ir(rec, a, mut=None, pre=None):
    """A whole inverted-residual block: expand 1x1 + BN + ReLU6 -> depthwise 3x3 (stride) + BN + ReLU6 -> project 1x1 + BN
    (+ the block input)."""
    dev = a.device
    blk = rec["blk"]
    seq = blk.conv
    x = mutate_input(a, mut if mut in ("chan", "row") else None)
    hi = mut if mut == "no_hi" else None
    B = a.abs()
    rt = 0.0
    if blk.expand_ratio != 1:
        x, B = stage(x, B, _w(seq[0][0], dev), *fold_bn(seq[0][1], dev), ACT_RELU6, mut=hi, pre=pre)
        rt += rtol("f32", a.shape[1])
        dwc, dwbn, pl, plbn = seq[1][0], seq[1][1], seq[2], seq[3]
    else:
        dwc, dwbn, pl, plbn = seq[0][0], seq[0][1], seq[1], seq[2]
    x, B = stage(x, B, _w(dwc, dev), *fold_bn(dwbn, dev), ACT_RELU6, stride=blk.stride, padding=1, groups=x.shape[1], mut=hi,
                 pre=pre)
    y, yb = stage(x, B, _w(pl, dev), *fold_bn(plbn, dev), ACT_NONE, mut=mut if mut == "bias" else None)
    rt += rtol("f32", 9) + rtol("f32", x.shape[1])
    if blk.use_res_connect:
        y, yb = y + a, yb + a.abs()
    return Ref(y, yb, y.abs(), None, rt, 0.0)


def ref_stem(rec, x, mut=None, pre=None):
    """features.0: 3x3 stride-2 conv 3 -> 32 + BN + ReLU6 of the caller's NCHW frames (uint8: normalised on load)."""
    dev = x.device
    rt = rtol("f32", 27)
    if rec["u8"]:
        mean = torch.tensor(rec["mean"], dtype=torch.float64, device=dev)
        std = torch.tensor(rec["stdv"], dtype=torch.float64, device=dev)
        x = (x / 255.0 - _vec(mean)) / _vec(std)
        rt += 4 * U                                        # the normalisation's own roundings, relative to |x|
    xm = mutate_input(x, mut if mut in ("chan", "row") else None)
    s, b = fold_bn(rec["bn"], dev)
    w = _w(rec["conv"], dev)
    y, yb = stage(xm, x.abs(), w, s, b, ACT_RELU6, stride=2, padding=1, mut=mut if mut in ("bias", "no_hi") else None, pre=pre)
    return Ref(y, yb, y.abs(), None, rt, 0.0)


# ------------------------------------------------------------------------------------------------------- data movement
def bilinear_ac(x, ho, wo, src=None):
    """F.interpolate(mode='bilinear', align_corners=True) in float64, output image n from source image src[n], with the
    bound's coordinate term: returns (y, B = the same interpolation of |x|, X)."""
    if src is not None:
        x = x[src]
    n, c, hi, wi = x.shape

    def axis(o, i):
        sc = (i - 1) / (o - 1) if o > 1 else 0.0
        pos = torch.arange(o, dtype=torch.float64, device=x.device) * sc
        i0 = pos.floor().long().clamp(0, i - 1)
        i1 = (i0 + 1).clamp(max=i - 1)
        lam = pos - i0.double()
        im = (i0 - 1).clamp(min=0)
        return pos, i0, i1, im, lam

    py, y0, y1, ym, ly = axis(ho, hi)
    px, x0, x1, xm, lx = axis(wo, wi)

    def interp(t):
        r0 = t[:, :, y0] * (1 - ly).view(1, 1, -1, 1) + t[:, :, y1] * ly.view(1, 1, -1, 1)
        return r0[..., x0] * (1 - lx) + r0[..., x1] * lx

    y = interp(x)
    B = interp(x.abs())
    # slopes on both sides of the sample (an fp32 coordinate can fall on the other side of an integer)
    ry = interp((x[:, :, 1:] - x[:, :, :-1]).abs().amax(2, keepdim=True).expand(-1, -1, hi, -1)) if hi > 1 else 0 * y
    rx = interp((x[..., 1:] - x[..., :-1]).abs().amax(3, keepdim=True).expand(-1, -1, -1, wi)) if wi > 1 else 0 * y
    X = 2 * U * (py.view(1, 1, -1, 1) * ry + px.view(1, 1, 1, -1) * rx)
    return y, B, X


def bilinear_src(n_out, src_mod, src_div):
    return [(k % src_mod) // src_div for k in range(n_out)]


def ref_bilinear(rec, x, out_hw, images, mut=None):
    ho, wo = out_hw
    x = mutate_input(x, mut if mut == "chan" else None)
    src = bilinear_src(max(images) + 1, rec["src_mod"], rec["src_div"])
    y, B, X = bilinear_ac(x, ho, wo, [src[k] for k in images])
    return Ref(y, B, y.abs(), X, 4 * U, 0.0)


def ref_tdiff(x, seq_len, mut=None):
    """teConv_sub's neighbour differences per sequence (model.py:194-200)."""
    x = mutate_input(x, mut if mut == "chan" else None)
    n = x.shape[0]
    prev = [t - 1 if t % seq_len else t + 1 for t in range(n)]
    nxt = [t + 1 if (t + 1) % seq_len else t - 1 for t in range(n)]
    a = torch.where(torch.tensor([t % seq_len == 0 for t in range(n)], device=x.device).view(-1, 1, 1, 1),
                    x[prev] - x, x - x[prev])          # t = 0: x[1] - x[0]
    last = torch.tensor([(t + 1) % seq_len == 0 for t in range(n)], device=x.device).view(-1, 1, 1, 1)
    b = torch.where(last, x[nxt] - x, x - x[nxt])     # t = last: x[last-1] - x[last]
    y = torch.cat([a, b], 1)
    B = torch.cat([x.abs() + x[prev].abs(), x.abs() + x[nxt].abs()], 1)
    return Ref(y, B, y.abs(), None, U, 0.0)


def ref_tsum(x, T, mut=None):
    """Sum over groups of T consecutive images (model.py:357-358)."""
    x = mutate_input(x, mut if mut == "chan" else None)
    n, c, h, w = x.shape
    y = x.view(n // T, T, c, h, w).sum(1)
    B = x.abs().view(n // T, T, c, h, w).sum(1)
    return Ref(y, B, y.abs(), None, T * U, 0.0)
