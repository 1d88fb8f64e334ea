"""Float64 restatement of the backward of the deep backbone (train.backbone_backward, train.block_backward(backbone=True),
train.srf_head_backward(need_tap_grads=True), uavsal_pix_gemm with `tails32`), the seeded inputs of their tests and the
per-element bounds, in the convention of tests/block_ref64.py and tests/mp_ref64.py:

    |kernel - ref| <= bound,      U = 2^-24, LAMBDA = 8, EPS = 8 U (tests/plan_ref64.py),  D = 2^-53

The six block shapes of MobileNetV2 features[8:18] (BLOCKS: cin, hidden, cout, stride, residual) and their nine weight-gradient
GEMM shapes (GEMM_NEW: the six `tails32` takes, GEMM_OLD: the three the tile kernel always took).  The closed forms and their
bounds are mp_ref64's, which are written for any channel counts and stride 1 or 2 (`grads_from_parts`: x, e, ga on the INPUT
grid, d, gd, go on the OUTPUT grid) and ctx_ref64's (`ir_bwd_s2_ref`, `input_grad_e2e`); nothing is restated that they state.
What is new here:

  short_partition   the K split of the `tails32` shapes: units of 128 pixels, about 512 workgroups (include/uavsal_hip.h).
  pix_gemm_ref      decoder_ref64's: LAMBDA U sqrt(K) sum |a| |b| -- the fp32 MFMA chains, the fp32 adds of the chains and the
                    double sum of the shares.  Shorter shares only shorten chains: the bound does not depend on the split.
  gemm bound of a 1x1 conv with n inputs   (rtol("f32", n) + U) on the absolute-value chain + EPS on the result (+ EPS on a
                    `res=` operand and on the sum): block_ref64.block_e2e's count for the gd and grad_x GEMMs.
  chain             features[7:18] as float64 module numbers, every block calibrated on the activations it really sees
                    (ctx_ref64.calibrated's recipe: both ReLU6s of every block see std 3, mean 1.5 + N(0, 1) per channel, so
                    each holds a sizeable share at 0, at 6 and inside; asserted by the CPU test), and its autograd.

Wrong variants (`WRONG`): each is the result of a kernel or a walk that gets that one thing wrong; the CPU test holds each at
least 4 bounds away on the inputs used here.  No factor is fitted to what a kernel gives.

Every function takes and returns float64 tensors on the device of its inputs unless it says numpy."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import block_ref64 as BR
import ctx_ref64 as X
import decoder_ref64 as DR
import mp_ref64 as MP
from plan_ref64 import EPS, LAMBDA, U, rtol

NAMES = BR.NAMES
D = DR.D
FIRST, END, C4 = 8, 18, 13                                        # train.BACKBONE_FIRST / _END / _C4
PARAMS = tuple("%d.%s" % (i, n) for i in range(FIRST, END) for n in NAMES)
# the block shapes of features[7:18]: (cin, hid, cout, stride, residual)
FEATURES = {7: (32, 192, 64, 2, False), 8: (64, 384, 64, 1, True), 9: (64, 384, 64, 1, True), 10: (64, 384, 64, 1, True),
            11: (64, 384, 96, 1, False), 12: (96, 576, 96, 1, True), 13: (96, 576, 96, 1, True), 14: (96, 576, 160, 2, False),
            15: (160, 960, 160, 1, True), 16: (160, 960, 160, 1, True), 17: (160, 960, 320, 1, False)}
BLOCKS = {"b8": FEATURES[8], "b11": FEATURES[11], "b12": FEATURES[12], "b14": FEATURES[14], "b15": FEATURES[15], "b17": FEATURES[17]}
PICTURES = [(2, 9, 13), (2, 8, 12)]                                # (frames, h, w) of the 1/8-scale c3 grid
GEMM_NEW = [(576, 96), (960, 160), (96, 384), (96, 576), (160, 576), (160, 960)]
GEMM_OLD = [(384, 64), (64, 384), (320, 960)]
GEMM_K = [(1, 5, 7), (2, 9, 13), (3, 23, 40)]                      # 35 (no multiple of the 32-pixel step), 234, 2760 (22 units)
SHORT_UNIT, SHORT_WGS, TILE = 128, 512, BR.GEMM_TILE               # csrc/train_decoder.hip: kShortUnit, kShortWGs
WRONG = ("s2_anchor", "no_residual", "no_g_c4", "aspp_branch_missing", "m_tail", "n_tail", "last_share")

down = X.down


def in_grid(name, pic):
    """(n, H, W) of the INPUT of block `name` for the c3 grid `pic`: 1/16 for b8..b14, 1/32 for b15, b17."""
    n, h, w = pic
    h, w = down(h), down(w)
    return (n, h, w) if name in ("b8", "b11", "b12", "b14") else (n, down(h), down(w))


# ------------------------------------------------------------------------------------------------ partitions, restated
def short_partition(K, M, N):
    """The K split of a `tails32` shape: `(pixels per share, shares, [(p0, p1) per share])`."""
    tiles = -(-M // TILE) * -(-N // TILE)
    units = -(-K // SHORT_UNIT)
    want = max(1, min(SHORT_WGS // tiles, units))
    ups = -(-units // want)
    span = ups * SHORT_UNIT
    spans = [(p, min(p + span, K)) for p in range(0, K, span)]
    return span, len(spans), spans


def shares(K, M, N):
    """uavsal_pix_gemm_shares with tails32 = 1 for one of GEMM_NEW + GEMM_OLD."""
    return short_partition(K, M, N)[1] if (M, N) in GEMM_NEW else MP.gemm_partition(K, M, N)[1]


def workgroups(K, M, N):
    return -(-M // TILE) * -(-N // TILE) * shares(K, M, N)


# ------------------------------------------------------------------------------------------------ the pixel GEMM
def gemm_inputs(M, N, pic):
    """`(a [n,h,w,M], b [n,h,w,N], w [M,N], row_scale [M])` float32 numpy."""
    n, h, w = pic
    rs = np.random.RandomState(12000 + 7 * M + N + n * h * w)
    return ((1e-2 * rs.standard_normal((n, h, w, M))).astype(np.float32), rs.standard_normal((n, h, w, N)).astype(np.float32),
            rs.standard_normal((M, N)).astype(np.float32), (0.5 + rs.random_sample(M)).astype(np.float32))


def pix_gemm_ref(a, b, variant=None):
    """`(G [M,N], bound)`; `variant`: "m_tail" / "n_tail": the rows / columns behind the last whole 128 tile are left out,
    "last_share": the last share of `short_partition` is."""
    M, N = a.shape[-1], b.shape[-1]
    K = a.numel() // M
    G, bound = DR.pix_gemm_ref(a, b)
    if variant == "m_tail":
        G = G.clone()
        G[M // TILE * TILE:] = 0
    elif variant == "n_tail":
        G = G.clone()
        G[:, N // TILE * TILE:] = 0
    elif variant == "last_share":
        p0, p1 = short_partition(K, M, N)[2][-1]
        A, B = a.reshape(K, M), b.reshape(K, N)
        G = G - A[p0:p1].T @ B[p0:p1]
    return G, bound


# ------------------------------------------------------------------------------------------------ one block
def calibrated(cfg, x, rs, st):
    """ctx_ref64.calibrated for any `(cin, hid, cout, stride, res)`: the MODULE numbers q (float32 numpy, block_ref64's keys)
    calibrated on the block's input `x` (float64)."""
    cin, hid, cout, stride, _ = cfg
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
    fold = {"s1": s1, "b1": b1, "s2": s2, "b2": b2, "s3": s3, "b3": b3}
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


def block_case(name, pic):
    """`(x [n,Cin,H,W] uniform in [0, 3), q, go [n,Co,Ho,Wo])` float32 numpy for the block `name` of BLOCKS on the grid it has
    when the c3 grid is `pic`."""
    cfg = BLOCKS[name]
    cin, hid, cout, stride, _ = cfg
    n, H, W = in_grid(name, pic)
    base = 13000 + 17 * sorted(BLOCKS).index(name) + n * H * W
    rs = np.random.RandomState(base)
    x = (3.0 * rs.random_sample((n, cin, H, W))).astype(np.float32)
    Ho, Wo = ((H - 1) // stride + 1, (W - 1) // stride + 1)
    go = (rs.standard_normal((n, cout, Ho, Wo)) / (Ho * Wo)).astype(np.float32)
    return x, calibrated(cfg, torch.as_tensor(x, dtype=torch.float64), rs, np.random.RandomState(base + 4000)), go


W_SUBSET = (slice(None, None, 5), slice(None, None, 7))          # the strided part of the W1 / W3 gradients the goldens keep


def golden_name(name, pic):
    return "backbone_%s_N%d_%dx%d" % ((name,) + tuple(in_grid(name, pic)))


def golden_digest(x, q, go):
    import train_ref64 as R
    return R.digest(x, go, *[q[k] for k in sorted(q)])


def golden_pack(grads):
    """What a golden file keeps of the nine gradients `{name: float64 tensor or numpy}`: the seven small ones whole (keys with
    `_` for `.`), W1 / W3 on W_SUBSET plus their sum and L2 norm."""
    out = {}
    for n, g in grads.items():
        g = np.asarray(g)
        if n in (NAMES[0], NAMES[6]):
            key, w = ("W1" if n == NAMES[0] else "W3"), g[:, :, 0, 0]
            out.update({key: w[W_SUBSET], key + "_sum": w.sum(), key + "_l2": np.sqrt((w * w).sum())})
        else:
            out[n.replace(".", "_")] = g
    return out


def make_block(cfg, q, cls):
    """The numbers `q` in a `model_feature.InvertedResidual` or a `dwBlock` (`cls`), eval mode."""
    cin, hid, cout, stride, _ = cfg
    if cls.__name__ == "InvertedResidual":
        blk = cls(cin, cout, stride, hid // cin)                  # (cin, cout, stride, expand_ratio)
    else:
        blk = cls(cin, cout, kernel_size=3, stride=stride, expand_ratio=hid // cin)
    return BR.load_block(blk, q)


def ir_bwd(p, gd, d, e, stride, variant=None, absolute=False):
    """`ga` from stored gd, d, e (NCHW).  `variant` "s2_anchor": the stride-2 window anchored as on an unpadded grid."""
    if stride == 2:
        return X.ir_bwd_s2_ref(p["wd"], p["s2"], gd, d, e, variant="stride1_parity" if variant == "s2_anchor" else None,
                               absolute=absolute)
    return BR.ir_bwd_ref(p, gd, d, e, absolute=absolute)


def ir_bwd_bound(p, gd, d, e, stride):
    return X.ir_bwd_s2_bound(p["wd"], p["s2"], gd, d, e) if stride == 2 else BR.ir_bwd_bound(p, gd, d, e)


def conv_t(g, w, s, res=None, bounds=False):
    """`g . (diag(s) W)` (+ `res`): the 1x1 GEMM with the transposed weights that carry `s` in their rows; `w` [Co,Ci,1,1],
    `g` [n,Co,h,w] -> [n,Ci,h,w].  `bounds`: `(value, bound)`, the module docstring's count."""
    v = F.conv_transpose2d(g * X._v(s), w)
    out = v if res is None else v + res
    if not bounds:
        return out
    b = (rtol("f32", w.shape[0]) + U) * F.conv_transpose2d(g.abs() * X._v(s.abs()), w.abs()) + EPS * out.abs()
    if res is not None:
        b = b + EPS * (res.abs() + v.abs())
    return out, b


def block_stage(p, cfg, x, go, pt, res=None, variant=None):
    """The stage-by-stage references of ONE block of a walk, fed the very tensors the device held (float64 copies of fp32):
    `x`, `go` and the parts `pt` = dict(e, d, gd, ga) (NCHW).  Returns `{key: (want, bound)}` for gd, ga, grad_x and the nine
    gradients (mp_ref64.grads_from_parts).  `res`: what the walk adds to grad_x where the block has no residual."""
    stride, has_res = cfg[3], cfg[4]
    out = {"gd": conv_t(go, p["w3"], p["s3"], bounds=True),
           "ga": (ir_bwd(p, pt["gd"], pt["d"], pt["e"], stride, variant), ir_bwd_bound(p, pt["gd"], pt["d"], pt["e"], stride))}
    add = go if has_res and variant != "no_residual" else (res if not has_res and variant != "no_g_c4" else None)
    out["grad_x"] = conv_t(pt["ga"], p["w1"], p["s1"], res=add, bounds=True)
    g, b = MP.grads_from_parts(p, x, pt["e"], pt["d"], pt["gd"], pt["ga"], go, stride, bounds=True)
    out.update({k: (g[k], b[k]) for k in NAMES})
    return out


# ------------------------------------------------------------------------------------------------ the chain features[7:18]
def chain_case(pic, seed=0):
    """`(c3 [n,32,h,w], Q {i: q}, g_c4 [n,96,h4,w4], g_c5 [n,320,h5,w5])` float32 numpy: features[7:18] with every block
    calibrated on the float64 activations it sees from this c3."""
    n, h, w = pic
    base = 14000 + seed + n * h * w
    rs = np.random.RandomState(base)
    c3 = (3.0 * rs.random_sample((n, 32, h, w))).astype(np.float32)
    x = torch.as_tensor(c3, dtype=torch.float64)
    Q = {}
    for i in range(FIRST - 1, END):
        cfg = FEATURES[i]
        Q[i] = calibrated(cfg, x, rs, np.random.RandomState(base + 100 * i))
        x = X.forward(BR.fold(BR.to64(Q[i])), x, cfg[3], cfg[4])["o"]
    h4, w4 = down(h), down(w)
    g4 = (rs.standard_normal((n, 96, h4, w4)) / (h4 * w4)).astype(np.float32)
    g5 = (rs.standard_normal((n, 320, down(h4), down(w4))) / (down(h4) * down(w4))).astype(np.float32)
    return c3, Q, g4, g5


def make_features(Q, features):
    """The numbers of `chain_case` in a `model_feature.mobilenet_v2_features()` Sequential; eval mode."""
    for i, q in Q.items():
        BR.load_block(features[i], q)
    return features.eval()


def chain_forward(P, c3, keep=None):
    """x7 .. x17 in float64 from the folds `P` {i: fold}; `keep` receives `x<i>`, `e<i>`, `d<i>`."""
    x = c3
    xs = {}
    for i in range(FIRST - 1, END):
        f = X.forward(P[i], x, FEATURES[i][3], FEATURES[i][4])
        x = xs[i] = f["o"]
        if keep is not None:
            keep.update({"x%d" % i: x, "e%d" % i: f["e"], "d%d" % i: f["d"]})
    return xs


def _forward_masked(p, x, stride, res, m):
    """ctx_ref64.forward's output with the DERIVATIVES of the two ReLU6s taken from the given masks `m = (me, md)` (the values
    stay float64's own): what a backward that reads stored activations computes."""
    hid = p["w1"].shape[0]
    e_pre = F.conv2d(x, p["w1"]) * X._v(p["s1"]) + X._v(p["b1"])
    e = (e_pre - e_pre.detach()) * m[0] + e_pre.detach().clamp(0, 6)
    d_pre = F.conv2d(e, p["wd"], padding=1, stride=stride, groups=hid) * X._v(p["s2"]) + X._v(p["b2"])
    d = (d_pre - d_pre.detach()) * m[1] + d_pre.detach().clamp(0, 6)
    o = F.conv2d(d, p["w3"]) * X._v(p["s3"]) + X._v(p["b3"])
    return o + x if res else o


def chain_autograd(Q, c3, g4, g5, variant=None, masks=None):
    """The 90 gradients of sum(g4 x13) + sum(g5 x17) by torch autograd through the restated forward, from the module numbers
    `Q` (float64): `{"<i>.<name>": gradient}`.  `variant` "no_g_c4": the c4 term left out.  `masks` `{i: (me, md)}` (0 / 1
    float64 NCHW, blocks 8..17): the ReLU6 derivatives are the given ones (`_forward_masked`), float64's own without."""
    keys = ("w1", "g1", "be1", "wd", "g2", "be2", "w3", "g3", "be3")
    leaves, P = {}, {}
    for i, q in Q.items():
        qq = dict(q)
        if i >= FIRST:
            leaves[i] = {k: q[k].detach().clone().requires_grad_(True) for k in keys}
            qq.update(leaves[i])
        P[i] = BR.fold(qq)
    if masks is None:
        xs = chain_forward(P, c3)
    else:
        xs, x = {}, c3
        for i in range(FIRST - 1, END):
            cfg = FEATURES[i]
            x = xs[i] = _forward_masked(P[i], x, cfg[3], cfg[4], masks[i]) if i in masks else X.forward(P[i], x, cfg[3], cfg[4])["o"]
    loss = (g5 * xs[END - 1]).sum() + (0 if variant == "no_g_c4" else (g4 * xs[C4]).sum())
    flat = [leaves[i][k] for i in range(FIRST, END) for k in keys]
    return dict(zip(PARAMS, torch.autograd.grad(loss, flat)))


def chain_closed(P, c3, g4, g5, variant=None, keep=None):
    """The 90 gradients from the CLOSED FORMS (no autograd): the float64 forward, then the walk of train.backbone_backward --
    blocks 17 .. 14 from g5, + g4, blocks 13 .. 8.  `variant`: "no_g_c4", "no_residual" (every residual's gradient dropped),
    "s2_anchor" (block 14's window).  `keep` receives `g<i>` (the gradient of x_i) and the forward's tensors."""
    k = {} if keep is None else keep
    xs = chain_forward(P, c3, keep=k)
    xs[FIRST - 2] = c3
    out, g = {}, g5
    for i in range(END - 1, FIRST - 1, -1):
        _, _, _, stride, res = FEATURES[i]
        k["g%d" % i] = g
        x = xs[i - 1]
        pt = MP.block_parts(P[i], x, g, stride)
        if stride == 2:
            pt["ga"] = ir_bwd(P[i], pt["gd"], pt["d"], pt["e"], 2, variant)
        gr = MP.grads_from_parts(P[i], x, pt["e"], pt["d"], pt["gd"], pt["ga"], g, stride)
        out.update({"%d.%s" % (i, n): gr[n] for n in NAMES})
        gx = conv_t(pt["ga"], P[i]["w1"], P[i]["s1"])
        if res and variant != "no_residual":
            gx = gx + g
        if i == C4 + 1 and variant != "no_g_c4":
            gx = gx + g4
        g = gx
    return out


# ------------------------------------------------------------------------------------------------ the head's tap gradients
def head_tap_terms(P, B, k):
    """The GEMMs whose sums are g_c4 and g_c5, from srf_ref64's head numbers `P`, `B` and the tensors `k` of its backward (or of
    the device's walk, NCHW float64): `{"c4": [(g, w, s)], "c5": [(g, w, s)] * 4}`, each term `g . (diag(s) w)`; c5 in the order
    the walk chains them: lv5_aspp1, then the three dilated branches."""
    import srf_ref64 as SF
    fold = lambda pre: SF.bn_fold(*SF._bn(P, B, pre))[0]                  # noqa: E731
    w1 = k["a1"].shape[1]
    c5 = [(k["g_aspp"][:, :w1] * X.m6(k["a1"]), P["lv5_aspp1.0.weight"], fold("lv5_aspp1.1"))]
    for i, m in enumerate(SF.HEAD_BLOCKS):
        c5.append((k["ga%d" % (i + 2)], P[m + ".conv.0.0.weight"], fold(m + ".conv.0.1")))
    return {"c4": [(k["g_x4"] * X.m6(k["x4"]), P["conv_lv4.0.weight"], fold("conv_lv4.1"))], "c5": c5}


def sum_terms(terms):
    """`(sum, bound)` of `head_tap_terms`' GEMMs chained through their `res=` operand, each GEMM's own bound added up."""
    v = b = None
    for g, w, s in terms:
        v, bb = conv_t(g, w, s, res=v, bounds=True)
        b = bb if b is None else b + bb
    return v, b


def class_shares(t):
    return BR.class_shares(t)
