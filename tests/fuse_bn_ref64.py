"""Float64 restatement of the fusion block in TRAINING mode (train.block_forward_batch / block_backward_batch, csrc/train_bn.hip:
uavsal_bn_apply_res), of the recurrence forward from a given input sequence (train.twa_forward / lstm_forward) and of the
chain block -> ConvTWA -> decoder that `recurrence_step(block_stats=("fuse",), batch_stats=("decoder",))` trains.  Built on
tests/decoder_bn_ref64.py (stats, apply, bwd_sums, bwd_apply, dw_wgrad, dw_raw, conv1x1, pix_gemm and their bounds),
tests/block_ref64.py (CFG, the golden subsets), tests/train_ref64.py (`twa_forward`, `twa_bptt`) and tests/lstm_ref64.py
(`lstm_forward`), in their convention:

    |kernel - ref| <= bound,      U = 2^-24, LAMBDA = 8, EPS = 8 U, D = 2^-53

Every stage is held against float64 of the fp32 tensors the device's stage read.  The bounds this module adds, rounding by
rounding:

  apply_res   out = fl(act(fma(u, s, b)) + res): decoder_bn_ref64.apply's bound for act(a), plus ONE rounding of the sum,
              U |out|.  (res is an input: exact.)
  grad_x      g_u1 . W1 (+ go with the residual, the GEMM's residual operand): decoder_bn_ref64.conv1x1's bound, plus one
              rounding of the sum, U (|go| + |grad_x|), with the residual.
  twa_step    z = fl(acc + pre) with acc = W_h * h_{t-1} (the step's launch) and pre = W_x * x_t (the hoisted launch), each an
              implicit GEMM over K = 9 * 256 products: plan_ref64.rtol("f32", K) on each sum of absolute values, i.e. on
              zb = |W| * |cat[x_t, h_{t-1}]|; pre is stored (U |pre|), acc leaves the accumulator (U |acc|), their sum is
              rounded (U |z|): err(z) = rtol zb + U (|pre| + |acc| + |z|) <= (rtol + 3 U) zb.
              i = 1 / (1 + expf(-z)): expf within 1 ulp = 2 U, the sum and the quotient one rounding each: 4 U i (the count of
              tests/decoder_bn_ref64.py and tests/train_ref64.py for the same expression), plus the
              pre-activation's err(z) i (1 - i) (|sigmoid'| = i (1 - i)): err(i) = i (1 - i) err(z) + 4 U i.
              h_t = fl(fl(i x) + fl(fl(1 - i) h)), d h_t / d i = x - h: |x - h| err(i), plus U for fl(1 - i) on |h|, one rounding
              per product and one for the sum (or fewer when the compiler contracts): 3 U (|i x| + |(1 - i) h|) + U |h_t|.
  lstm_step   the same err(z) per gate (K = 9 * 256 per half); sigmoid as above; tanhf within 2 ulp = 4 U:
              err(tanh z) = (1 - tanh^2) err(z) + 4 U |tanh z|.  c_t = fl(fl(f c) + fl(i g)):
              err(c) = |c_prev| err(f) + |g| err(i) + i err(g) + 2 U (|f c_prev| + |i g|) + U |c_t|;
              h_t = fl(o tanhf(c_t)): err(h) = |tanh c| err(o) + o ((1 - tanh^2 c) err(c) + 4 U |tanh c|) + U |h_t|.
  CHAIN_TOL   the whole chain block -> ConvTWA -> decoder, forward and backward, in RELATIVE L2 NORM over a tensor (the only
              whole-chain assertion; per element the stages are held one by one).  The chain at (3,5,7) is 69 launches
              (block forward 14, recurrence 1 + 3, decoder forward 12, decoder backward 15, recurrence backward 5, block
              backward 19); none has a relative bound above the longest sum's, plan_ref64.rtol("f32", 9 * 256) = 2.3e-5 of its
              sum of absolute values, and an L2 norm over a tensor does not grow faster than the sum of what the stages add:
              69 * 2.3e-5 = 1.6e-3.  A ReLU6 mask that falls the other way removes one element's whole term: an e or d element
              lies within its own bound (U * 6 = 3.6e-7) of a clamp with probability below 1e-6 at a pre-activation spread of
              3, so the share of such terms is below 1e-6 and their L2 share below 1e-3.  CHAIN_TOL = 2.6e-3.  The CPU test
              holds every wrong variant of the block and of the recurrence at least 4 CHAIN_TOL away in a tensor it spoils
              -- but one: the biased running variance moves running_var by 1 / (10 P) of the batch variance, which no
              whole-chain tolerance sees; the ONE-ulp check of the stage tests holds that.
No factor is fitted to what a kernel gives.

Shapes (T, H, W): the block at (2, 5, 7) (one slab) and (3, 13, 17) (two slabs, the last one partial:
decoder_bn_ref64.SLAB_SHAPE); the recurrence at (3, 5, 7) with h0 (c0) None and (5, 12, 20) with a non-zero state
(train_ref64.twa_inputs / lstm_ref64.lstm_inputs); the chain at (3, 5, 7).
Every function takes and returns float64 tensors on the device of its inputs unless it says numpy."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import block_ref64 as KR
import decoder_bn_ref64 as BR
import lstm_ref64 as LR
import train_ref64 as R
from plan_ref64 import EPS, LAMBDA, U, rtol  # noqa: F401

CFG, CFGS = KR.CFG, KR.CFGS
NAMES = BR.NAMES
SHAPES = [(2, 5, 7), (3, 13, 17)]
SLAB_SHAPE = BR.SLAB_SHAPE
RNN_SHAPES = [(3, 5, 7), (5, 12, 20)]
CHAIN_SHAPE = (3, 5, 7)
W_SUBSET, GX_SUBSET = KR.W_SUBSET, KR.GX_SUBSET
WD_SUBSET = slice(None, None, 5)                                  # the channels of the depthwise gradient the goldens keep
# the chain's golden holds two blocks and the recurrence: coarser subsets (each with the whole tensor's sum and L2 norm)
CHAIN_W_SUBSET = (slice(None, None, 15), slice(None, None, 21))
CHAIN_WD_SUBSET, CHAIN_C_SUBSET, CHAIN_RNN_SUBSET = slice(None, None, 15), slice(None, None, 4), LR.DW_SUBSET
ZERO_GAMMA = (41, 1201)                                          # gamma1 = 0 / gamma2 = 0 of these channels, beta 1.5
BN_EPS, MOMENTUM = BR.BN_EPS, BR.MOMENTUM
K_RNN = 9 * 256
CHAIN_LAUNCHES = 14 + (1 + 3) + 12 + 15 + 5 + 19
CHAIN_TOL = CHAIN_LAUNCHES * rtol("f32", K_RNN) + 1e-3               # relative L2 norm of a whole-chain tensor (docstring)
WRONG_BLOCK = ("bn3_eval_grad", "no_residual_gx", "res_before_bn3", "per_frame", "dw3_from_u2", "biased_running", "last_slab")
WRONG_RNN = ("h_tm2", "h0_ignored", "swapped")
ACT_NONE, ACT_RELU6 = BR.ACT_NONE, BR.ACT_RELU6


def name(cfg, shape):
    return "fuse_bn_%s_T%d_%dx%d" % ((cfg,) + tuple(shape))


def chain_name(shape=CHAIN_SHAPE):
    return "fuse_bn_chain_T%d_%dx%d" % tuple(shape)


# ------------------------------------------------------------------------------------------------ inputs (float32 numpy)
def block_case(cfg, shape, zero_gamma=True, seed=0):
    """`(x [T,Cin,H,W] uniform in [0, 3), q, go [T,Co,H,W])`, float32 numpy: the block's MODULE numbers q = {w1, wd, w3, g*, be*,
    rm*, rv*} (* = 1, 2, 3), the keys of `decoder_bn_ref64.decoder_case`, so `decoder_bn_ref64.load_block` loads them.  In
    training mode a BatchNorm normalises whatever it is handed, so gamma = +-3 and beta = 1.5 + N(0, 1) give both ReLU6s
    pre-activations of spread 3 around 1.5 on any data: both clamps hold a sizeable share (asserted by the CPU test); BN3 has
    gamma of magnitude 0.5 .. 1.5 and beta N(0, 0.25).  The running statistics are not the initial 0 and 1."""
    c = CFG[cfg]
    cin, hid, cout = c["cin"], c["hid"], c["cout"]
    T, H, W = shape
    rs = np.random.RandomState(8200 + 1000 * CFGS.index(cfg) + T * H * W + seed)
    x = (3.0 * rs.random_sample((T, cin, H, W))).astype(np.float32)
    go = (rs.standard_normal((T, cout, H, W)) / (H * W)).astype(np.float32)
    q = {"w1": (rs.standard_normal((hid, cin, 1, 1)) * math.sqrt(2.0 / hid)).astype(np.float32),
         "wd": (rs.standard_normal((hid, 1, 3, 3)) * math.sqrt(2.0 / (hid * 9))).astype(np.float32),
         "w3": (rs.standard_normal((cout, hid, 1, 1)) * math.sqrt(2.0 / cout)).astype(np.float32)}
    for i, n in ((1, hid), (2, hid), (3, cout)):
        sign = rs.choice([-1.0, 1.0], n).astype(np.float32)
        if i < 3:
            q["g%d" % i] = np.full(n, 3.0, np.float32) * sign
            q["be%d" % i] = (1.5 + rs.standard_normal(n)).astype(np.float32)
        else:
            q["g%d" % i] = (0.5 + rs.random_sample(n)).astype(np.float32) * sign
            q["be%d" % i] = (0.5 * rs.standard_normal(n)).astype(np.float32)
        q["rm%d" % i] = (0.1 * rs.standard_normal(n)).astype(np.float32)
        q["rv%d" % i] = (0.5 + rs.random_sample(n)).astype(np.float32)
    if zero_gamma:
        for i, ch in ((1, ZERO_GAMMA[0]), (2, ZERO_GAMMA[1])):
            q["g%d" % i][ch] = 0.0
            q["be%d" % i][ch] = 1.5
    return x, q, go


load_block, to64 = BR.load_block, BR.to64


def chain_case(shape=CHAIN_SHAPE):
    """The chain's inputs, float32 numpy: `(x [T,320,H,W], qb, h0 [1,256,H,W], w [256,512,3,3], qd, gy [T,1,H,W])` -- the
    "fucbst" block's numbers (`block_case`), the ConvTWA weight and a NON-zero h0 of `train_ref64.twa_inputs` (the (5,12,20)
    recipe's scale), the decoder's numbers of `decoder_bn_ref64.decoder_case`."""
    T, H, W = shape
    x, qb, _ = block_case("fucbst", shape, seed=77)
    rs = np.random.RandomState(8900 + T * H * W)
    h0 = (0.5 * rs.standard_normal((1, 256, H, W))).astype(np.float32)
    w = (rs.standard_normal((256, 512, 3, 3)) * math.sqrt(2.0 / (256 * 9))).astype(np.float32)
    _, qd, gy = BR.decoder_case(shape, seed=77)
    return x, qb, h0, w, qd, gy


# ------------------------------------------------------------------------------------------------ the new stages
def apply_res(u, f, res, act=ACT_NONE):
    """`uavsal_bn_apply_res` from the device's fold `f`: `(out, bound)`."""
    a, b = BR.apply(u, f, act)
    out = a + res
    return out, b + U * out.abs()


def grad_x(g_u1, w1, go=None):
    """`grad_x = g_u1 . W1 (+ go)` (NHWC): `(out, bound)`."""
    out, b = BR.conv1x1(g_u1, w1, transpose=True)
    if go is None:
        return out, b
    return out + go, b + U * (go.abs() + (out + go).abs())


def _err_z(zb):
    return (rtol("f32", K_RNN) + 3 * U) * zb


def _sig(z, ez):
    s = torch.sigmoid(z)
    return s, s * torch.sigmoid(-z) * ez + 4 * U * s


def _tanh(z, ez):
    t = torch.tanh(z)
    return t, LR._q(z) * ez + 4 * U * t.abs()


def twa_step(x_t, hprev, w, variant=None, h_other=None):
    """One ConvTWA step `[1,256,H,W]`: `(h_t, bound)`.  `variant`: "swapped" (x_t and h_{t-1} swapped in the update), or
    "h_tm2" with `h_other` = h_{t-2} read in place of h_{t-1} (the bound stays the right one's)."""
    if variant == "h_tm2":
        hprev = h_other
    cat = torch.cat([x_t, hprev], 1)
    z = F.conv2d(cat, w, padding=1)
    zb = F.conv2d(cat.abs(), w.abs(), padding=1)
    i, ei = _sig(z, _err_z(zb))
    a, b = (hprev, x_t) if variant == "swapped" else (x_t, hprev)
    h = i * a + (1 - i) * b
    return h, (a - b).abs() * ei + 3 * U * ((i * a).abs() + ((1 - i) * b).abs()) + U * h.abs()


def lstm_step(x_t, hprev, cprev, w):
    """One ConvLSTM step: `(h_t, c_t, bound_h, bound_c)`."""
    cat = torch.cat([x_t, hprev], 1)
    z = LR.split(F.conv2d(cat, w, padding=1))
    ez = LR.split(_err_z(F.conv2d(cat.abs(), w.abs(), padding=1)))
    (i, ei), (f, ef), (o, eo) = (_sig(z[k], ez[k]) for k in "ifo")
    g, eg = _tanh(z["g"], ez["g"])
    c = f * cprev + i * g
    ec = cprev.abs() * ef + g.abs() * ei + i * eg + 2 * U * ((f * cprev).abs() + (i * g).abs()) + U * c.abs()
    tc = torch.tanh(c)
    h = o * tc
    return h, c, tc.abs() * eo + o * (LR._q(c) * ec + 4 * U * tc.abs()) + U * h.abs(), ec


def twa_forward(x, h0, w, variant=None):
    """`train_ref64.twa_forward`'s h_seq, or that of a WRONG recurrence (`variant` of WRONG_RNN)."""
    if variant is None:
        return R.twa_forward(x, h0, w)[0]
    hs = [torch.zeros_like(h0) if variant == "h0_ignored" else h0]
    for t in range(x.shape[0]):
        other = hs[-2] if len(hs) > 1 else torch.zeros_like(h0)
        hs.append(twa_step(x[t:t + 1], hs[-1], w, variant=variant if variant != "h0_ignored" else None, h_other=other)[0])
    return torch.cat(hs[1:], 0)


# ------------------------------------------------------------------------------------------------ the whole block
def block_train(q, x, go, res, variant=None):
    """The block in training mode and its backward by the closed form, float64 throughout, from the MODULE's numbers `q`
    (float64 tensors), `x` `[T,Cin,H,W]`, `go` `[T,Co,H,W]`.  Returns a dict: out, grad_x (NCHW), the nine gradients under
    NAMES, mu1..3 / var1..3, rm1..3 / rv1..3 (after the step) and the NHWC intermediates u1, e, u2, d, u3, g_u1, g_u2, g_u3,
    g_e, g_d.  `variant`: one of WRONG_BLOCK, the result of an implementation that gets that one thing wrong."""
    xn, gon = x.permute(0, 2, 3, 1), go.permute(0, 2, 3, 1)
    T, H, W, _ = xn.shape
    P = T * H * W
    hid, cin = q["w1"].shape[:2]
    cout = q["w3"].shape[0]
    sv = variant if variant in ("per_frame", "last_slab") else None
    u1, _ = BR.conv1x1(xn, q["w1"])
    f1 = BR.stats(u1, q["g1"], q["be1"], variant=sv)
    e, _ = BR.apply(u1, f1, ACT_RELU6)
    u2, _ = BR.dw_raw(e, q["wd"])
    f2 = BR.stats(u2, q["g2"], q["be2"], variant=sv)
    d, _ = BR.apply(u2, f2, ACT_RELU6)
    u3, _ = BR.conv1x1(d, q["w3"])
    if res and variant == "res_before_bn3":
        u3 = u3 + xn
    f3 = BR.stats(u3, q["g3"], q["be3"], variant=sv)
    out, _ = BR.apply(u3, f3, ACT_NONE)
    if res and variant != "res_before_bn3":
        out = out + xn
    s3 = BR.bwd_sums(gon, u3, f3, ACT_NONE)
    g_u3 = f3["s"] * gon if variant == "bn3_eval_grad" else BR.bwd_apply(gon, u3, f3, s3, ACT_NONE)
    G3, _ = BR.pix_gemm(g_u3, u2 if variant == "dw3_from_u2" else d)
    g_d, _ = BR.conv1x1(g_u3, q["w3"], transpose=True)
    s2 = BR.bwd_sums(g_d, u2, f2, ACT_RELU6)
    g_u2 = BR.bwd_apply(g_d, u2, f2, s2, ACT_RELU6)
    g_wd = BR.dw_wgrad(g_u2, e)
    g_e, _ = BR.dw_raw(g_u2, q["wd"], transpose=True)
    s1 = BR.bwd_sums(g_e, u1, f1, ACT_RELU6)
    g_u1 = BR.bwd_apply(g_e, u1, f1, s1, ACT_RELU6)
    G1, _ = BR.pix_gemm(g_u1, xn)
    gx, _ = grad_x(g_u1, q["w1"], gon if res and variant != "no_residual_gx" else None)
    r = {"out": out.permute(0, 3, 1, 2), "grad_x": gx.permute(0, 3, 1, 2),
         NAMES[0]: G1.view(hid, cin, 1, 1), NAMES[1]: s1[1], NAMES[2]: s1[0], NAMES[3]: g_wd, NAMES[4]: s2[1], NAMES[5]: s2[0],
         NAMES[6]: G3.view(cout, hid, 1, 1), NAMES[7]: s3[1], NAMES[8]: s3[0],
         "u1": u1, "e": e, "u2": u2, "d": d, "u3": u3, "g_u1": g_u1, "g_u2": g_u2, "g_u3": g_u3, "g_e": g_e, "g_d": g_d}
    for i, f in ((1, f1), (2, f2), (3, f3)):
        r["mu%d" % i], r["var%d" % i] = f["mu"], f["var"]
        r["rm%d" % i], r["rv%d" % i] = BR.running(q["rm%d" % i], q["rv%d" % i], f["mu"], f["var"], P,
                                                  variant="biased_running" if variant == "biased_running" else None)
    return r


def _bn(x, run, leaves, i):
    return F.batch_norm(x, run["rm%d" % i], run["rv%d" % i], leaves["g%d" % i], leaves["be%d" % i], True, MOMENTUM, BN_EPS)


_KEYS = ("w1", "g1", "be1", "wd", "g2", "be2", "w3", "g3", "be3")


def _block_graph(q, x, res):
    leaves = {k: q[k].detach().clone().requires_grad_(True) for k in _KEYS}
    run = {k: q[k].detach().clone() for k in q if k[:2] in ("rm", "rv")}
    hid = q["w1"].shape[0]
    e = F.relu6(_bn(F.conv2d(x, leaves["w1"]), run, leaves, 1))
    d = F.relu6(_bn(F.conv2d(e, leaves["wd"], padding=1, groups=hid), run, leaves, 2))
    out = _bn(F.conv2d(d, leaves["w3"]), run, leaves, 3)
    return (out + x if res else out), leaves, run


def block_autograd(q, x, go, res):
    """torch's own `F.batch_norm(training=True)` and autograd in double: out, grad_x, the nine gradients under NAMES, and
    rm1..3 / rv1..3 as torch moved them."""
    xx = x.detach().clone().requires_grad_(True)
    out, leaves, run = _block_graph(q, xx, res)
    gs = torch.autograd.grad(out, [leaves[k] for k in _KEYS] + [xx], go)
    r = dict(zip(NAMES, gs[:9]))
    r.update(out=out.detach(), grad_x=gs[9], **run)
    return r


# ------------------------------------------------------------------------------------------------ the chain
def chain_train(qb, x, h0, w, qd, gy):
    """block("fucbst").train() -> ConvTWA -> decoder.train() + sigmoid with the loss sum(gy y), by the closed forms: a dict with
    y, x_seq, h_seq, "rnn" (the ConvTWA weight's gradient), grad_x (of the block's input), "block" and "decoder": the dicts of
    `block_train` / `decoder_bn_ref64.decoder_train` (their nine gradients and moved statistics)."""
    fw = block_train(qb, x, torch.zeros(x.shape[0], 256, x.shape[2], x.shape[3], dtype=x.dtype, device=x.device), False)
    x_seq = fw["out"]
    h_seq = twa_forward(x_seq, h0, w)
    dec = BR.decoder_train(qd, h_seq, gy)
    gw, gx, _ = R.twa_bptt(x_seq, h0, w, dec["grad_h"])
    blk = block_train(qb, x, gx, False)
    return {"y": dec["y"], "x_seq": x_seq, "h_seq": h_seq, "rnn": gw, "grad_x": blk["grad_x"], "block": blk, "decoder": dec}


def chain_autograd(qb, x, h0, w, qd, gy):
    """The same chain by torch autograd in double: y, "rnn", grad_x, "block" / "decoder": the nine gradients each."""
    xx = x.detach().clone().requires_grad_(True)
    ww = w.detach().clone().requires_grad_(True)
    x_seq, lb, _ = _block_graph(qb, xx, False)
    h_seq = R.twa_forward(x_seq, h0, ww)[0]
    ld = {k: qd[k].detach().clone().requires_grad_(True) for k in _KEYS}
    run = {k: qd[k].detach().clone() for k in qd if k[:2] in ("rm", "rv")}
    e = F.relu6(_bn(F.conv2d(h_seq, ld["w1"]), run, ld, 1))
    d = F.relu6(_bn(F.conv2d(e, ld["wd"], padding=1, groups=BR.HID), run, ld, 2))
    y = torch.sigmoid(_bn(F.conv2d(d, ld["w3"]), run, ld, 3))
    gs = torch.autograd.grad(y, [lb[k] for k in _KEYS] + [ld[k] for k in _KEYS] + [ww, xx], gy)
    return {"y": y.detach(), "block": dict(zip(NAMES, gs[:9])), "decoder": dict(zip(NAMES, gs[9:18])), "rnn": gs[18],
            "grad_x": gs[19]}


clamp_shares = BR.clamp_shares
