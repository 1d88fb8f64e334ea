"""Float64 restatement of the backward of the shallow backbone (train.shallow_backward, train.block_backward(shallow=True),
train.srf_head_backward(need_c3_grad=True), train.backbone_backward(need_x_grad=True), uavsal_skinny_wgrad, the channel sums with
`ch16`), the seeded inputs of their tests and the per-element bounds, in the convention of tests/backbone_ref64.py:

    |kernel - ref| <= bound,      U = 2^-24,  D = 2^-53

The five block shapes of MobileNetV2 features[2:8] (BLOCKS: cin, hidden, cout, stride, residual) and the five weight-gradient
products nothing but the skinny GEMM takes (GEMM).  The closed forms of a block and their bounds are mp_ref64's, ctx_ref64's and
backbone_ref64's (`block_stage`, `conv_t`), which are written for any channel counts and stride 1 or 2; nothing is restated
that they state.  What is new here:

  partition     the K split stated in include/uavsal_hip.h: units of 128 pixels, at most 1024 shares, a share one wave.
  skinny_ref    G = A^T B and the WORST-CASE bound of that partition, element by element: a chain is a sequence of at most
                L = min(pixels of a share, UAVSAL_WGRAD_CHAIN) fused multiply-adds in fp32 from zero (relative error at most
                L U on the absolute-value sum, to first order), the c = ceil(pixels of a share / UAVSAL_WGRAD_CHAIN) chains of
                a share are added in fp32 (c U), the shares in double (nothing at this scale), and the result is rounded once
                (U): (L + c + 2) U sum |a| |b|, the 2 covering the second-order terms (L U <= 2^-14).  Unlike
                decoder_ref64.pix_gemm_ref's LAMBDA U sqrt(K) it holds for ANY data, signs all equal included, and at K above a
                million it is eight times tighter, which is what lets a dropped share be seen there.
  sums_ref      the channel sums at hidden widths 96 and 144, stride 1 and 2, with mp_ref64's bounds.
  chain         features[2:8] as float64 module numbers behind the frozen stem and features[1] (`frozen_forward` restates those
                two: the package's modules only hold parameters), every block calibrated on the activations it really sees from
                the frames (backbone_ref64.calibrated), its autograd and the closed-form walk.

Wrong variants (`WRONG`, `CHAIN_WRONG`, `sums_ref`'s): each is the result of a kernel or a walk that gets that one thing wrong;
the CPU test holds each at least 4 bounds away on the inputs used here.  No factor is fitted to what a kernel gives.

Every function takes and returns float64 tensors on the device of its inputs unless it says numpy."""
import numpy as np
import torch
import torch.nn.functional as F

import backbone_ref64 as BK
import block_ref64 as BR
import ctx_ref64 as X
import decoder_ref64 as DR
import mp_ref64 as MP
from plan_ref64 import U

NAMES = BR.NAMES

UNIT, SHARES, CHAIN = 128, 1024, 1024                              # UAVSAL_SKINNY_UNIT, UAVSAL_SKINNY_SHARES, UAVSAL_WGRAD_CHAIN
MAX_NARROW, MAX_WIDE = 32, 192
# the five products of features[2:8] nothing else takes: G3 of block 2 (96 x 16 is G1: hidden x cin), ...
GEMM = [(96, 16), (144, 24), (24, 96), (24, 144), (32, 144)]
GEMM_REFUSED = [(96, 64), (200, 8), (20, 8), (48, 40)]             # both sides over 32; wider than 192; no multiple of 8; both over 32
GEMM_K = [(2, 5, 7), (3, 23, 40)]                                  # 70 pixels (under a chain, no multiple of the 2-pixel step's 16), 2760 (22 shares, the last of 72)
K_CHAINS = 8200 * UNIT - 37                                        # 1,049,563 pixels: 912 shares of 9 units = 1152 pixels, two chains each; the last holds 91
WRONG = ("narrow_pad", "last_pixel", "last_share")
# the five block shapes of features[2:8]: (cin, hid, cout, stride, residual); features[5] and [6] are one shape
BLOCKS = {"b2": (16, 96, 24, 2, False), "b3": (24, 144, 24, 1, True), "b4": (24, 144, 32, 2, False), "b5": (32, 192, 32, 1, True),
          "b7": (32, 192, 64, 2, False)}
PICTURES = [(2, 4, 6), (2, 5, 7)]                                  # (n, H, W) of a block's INPUT; the odd grid is what stride 2 gets wrong
SUMS_CH = (96, 144)                                                # the hidden widths uavsal_ir_sums refuses without ch16
SUMS_PICTURES = PICTURES + [(2, 23, 40)]                           # ... and one with more than one slab (stride 1: 4, stride 2: 12)
D = DR.D
W_SUBSET = BK.W_SUBSET


def accepted(M, N):
    return M > 0 and N > 0 and M % 8 == 0 and N % 8 == 0 and min(M, N) <= MAX_NARROW and max(M, N) <= MAX_WIDE


def partition(K):
    """The K split of uavsal_skinny_wgrad: `(pixels per share, shares, [(p0, p1) per share])`."""
    units = -(-K // UNIT)
    want = min(SHARES, units)
    ups = -(-units // want)
    span = ups * UNIT
    spans = [(p, min(p + span, K)) for p in range(0, K, span)]
    return span, len(spans), spans


def chains(K):
    """`(longest chain, chains of a share)` of that split."""
    span = min(partition(K)[0], K)
    return min(span, CHAIN), -(-span // CHAIN)


def reduce_groups(N, shares):
    """The second launch: `(groups, shares per group)`."""
    g = 1024 // N
    return g, -(-shares // g)


def gemm_inputs(M, N, pic, positive=False):
    """`(a [n,h,w,M], b [n,h,w,N], w [M,N], row_scale [M], pad [n,h,w,32])` float32 numpy; `pad` is what lies behind the
    narrow operand's last column in the fenced buffer of a wrong kernel."""
    n, h, w = pic
    rs = np.random.RandomState(13000 + 7 * M + N + n * h * w)
    a, b = 1e-2 * rs.standard_normal((n, h, w, M)), rs.standard_normal((n, h, w, N))
    if positive:
        a, b = np.abs(a), np.abs(b)
    return (a.astype(np.float32), b.astype(np.float32), rs.standard_normal((M, N)).astype(np.float32),
            (0.5 + rs.random_sample(M)).astype(np.float32), rs.standard_normal((n, h, w, 32)).astype(np.float32))


def skinny_ref(a, b, variant=None, pad=None):
    """`(G [M,N], bound)`.  `variant`: "last_pixel": pixel K - 1 is left out; "last_share": the last share of `partition`
    is; "narrow_pad": the N side's last 32-wide tile is taken whole, its padding columns filled from `pad` (the neighbouring
    channels) and not zeros, and the partial rows of that tile pitch are then read back with the pitch of the true width."""
    M, N = a.shape[-1], b.shape[-1]
    K = a.numel() // M
    A, B = a.reshape(K, M), b.reshape(K, N)
    G = A.T @ B
    L, c = chains(K)
    bound = (L + c + 2) * U * (A.abs().T @ B.abs())
    if variant == "last_pixel":
        G = G - torch.outer(A[K - 1], B[K - 1])
    elif variant == "last_share":
        p0, p1 = partition(K)[2][-1]
        G = G - A[p0:p1].T @ B[p0:p1]
    elif variant == "narrow_pad":
        Np = -(-N // 32) * 32                                       # N % 32 == 0 (24 x 96): the padding is rows only, which no
        P = pad.reshape(K, 32).to(A)                                # in-range element sees -- the variant is the right answer
        G = (A.T @ torch.cat([B, P[:, :Np - N]], 1)).reshape(-1)[:M * N].reshape(M, N)
    elif variant is not None:
        raise ValueError(variant)
    return G, bound


# ------------------------------------------------------------------------------------------------ one block
def block_case(name, pic):
    """`(x [n,Cin,H,W] uniform in [0, 3), q, go [n,Co,Ho,Wo])` float32 numpy for the block `name` of BLOCKS on the INPUT grid
    `pic`, calibrated as backbone_ref64.calibrated calibrates (both ReLU6s see 0, 6 and the interior)."""
    cfg = BLOCKS[name]
    cin, hid, cout, stride, _ = cfg
    n, H, W = pic
    base = 14000 + 17 * sorted(BLOCKS).index(name) + n * H * W
    rs = np.random.RandomState(base)
    x = (3.0 * rs.random_sample((n, cin, H, W))).astype(np.float32)
    Ho, Wo = ((H - 1) // stride + 1, (W - 1) // stride + 1)
    go = (rs.standard_normal((n, cout, Ho, Wo)) / (Ho * Wo)).astype(np.float32)
    return x, BK.calibrated(cfg, torch.as_tensor(x, dtype=torch.float64), rs, np.random.RandomState(base + 4000)), go


def golden_name(name, pic):
    return "shallow_%s_N%d_%dx%d" % ((name,) + tuple(pic))


golden_digest, golden_pack, make_block, block_stage, conv_t = BK.golden_digest, BK.golden_pack, BK.make_block, BK.block_stage, BK.conv_t


# ------------------------------------------------------------------------------------------------ the channel sums
def sums_case(pic, Ch, Co, stride):
    """Teacher-forced inputs of uavsal_ir_sums / uavsal_ir_sums_s2, float32 numpy NCHW: `(gd, d [n,Ch,Ho,Wo], e, ga [n,Ch,H,W],
    go [n,Co,Ho,Wo])`; d and e hold 0, 6 and the interior."""
    n, H, W = pic
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    rs = np.random.RandomState(15000 + 31 * Ch + Co + stride + n * H * W)
    act = lambda *sh: np.clip(1.5 + 3.0 * rs.standard_normal(sh), 0.0, 6.0).astype(np.float32)       # noqa: E731
    ga = (rs.standard_normal((n, Ch, H, W)) * (rs.random_sample((n, Ch, H, W)) < 0.7)).astype(np.float32)
    return (rs.standard_normal((n, Ch, Ho, Wo)).astype(np.float32), act(n, Ch, Ho, Wo), act(n, Ch, H, W), ga,
            rs.standard_normal((n, Co, Ho, Wo)).astype(np.float32))


def sums_ref(gd, d, e, ga, go, stride, variant=None):
    """`(sums, bounds)`: dict(S2 [Ch], Gd [Ch,3,3], S1 [Ch], S3 [Co]) of the workspace of uavsal_ir_sums (stride 1) or
    uavsal_ir_sums_s2 (stride 2) summed over its slabs, and mp_ref64's bounds (delta2 = gd m6(d) is exact in fp32, every
    product is rounded once to double and added in double).  `variant` "s2_anchor": the stride-2 window anchored as on an
    unpadded grid (mp_ref64's "no_top_pad"); "last_group": the channels behind the last whole group of 64 left at zero."""
    if stride == 2:
        S, b = MP.ir_sums_s2_ref(gd, d, e, ga, go, variant="no_top_pad" if variant == "s2_anchor" else None, bounds=True)
    else:
        d2, a2 = gd * X.m6(d), gd.abs() * X.m6(d)
        n = d.shape[0] * d.shape[2] * d.shape[3]
        S = {"S2": d2.sum((0, 2, 3)), "Gd": DR._tap_sums(d2, e), "S1": ga.sum((0, 2, 3)), "S3": go.sum((0, 2, 3))}
        b = {"S2": ((U + n * D) * a2).sum((0, 2, 3)), "Gd": DR._tap_sums((3 * U + n * D) * a2, e.abs()),
             "S1": (U + n * D) * ga.abs().sum((0, 2, 3)), "S3": n * D * go.abs().sum((0, 2, 3))}
    if variant == "last_group":
        Ch = d.shape[1]
        S = {k: v.clone() for k, v in S.items()}
        for k in ("S2", "Gd", "S1"):
            S[k][Ch // 64 * 64:] = 0
    return S, b


# ------------------------------------------------------------------------------------------------ the chain features[0:8]
FIRST, END, C3 = 2, 8, 6                                           # train.SHALLOW_FIRST / _END / _C3
PARAMS = tuple("%d.%s" % (i, n) for i in range(FIRST, END) for n in NAMES)
FEATURES = {2: BLOCKS["b2"], 3: BLOCKS["b3"], 4: BLOCKS["b4"], 5: BLOCKS["b5"], 6: BLOCKS["b5"], 7: BLOCKS["b7"]}
FRAMES = [(2, 38, 54), (2, 40, 56)]                                # (n, H, W): 19 x 27 -> 10 x 14 -> 5 x 7 -> 3 x 4, and 20 x 28 -> ... -> 3 x 4
CHAIN_WRONG = ("s2_anchor", "no_residual", "no_g_c3", "no_pass7")
down = X.down


def _bn64(bn, t):
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    return t * X._v(s) + X._v(bn.bias.detach().double() - bn.running_mean.detach().double() * s)


def frozen_forward(features, x):
    """`(x0, x1)` in float64: the stem (conv 3x3 stride 2 + BatchNorm + ReLU6) and features[1] (depthwise 3x3 + BatchNorm +
    ReLU6, 1x1 conv + BatchNorm; no expand conv, no residual) of a `model_feature.mobilenet_v2_features()` in eval mode, restated
    (the package's modules only hold parameters)."""
    w = lambda c: c.weight.detach().double()                              # noqa: E731
    stem, f1 = features[0], features[1].conv
    x0 = _bn64(stem[1], F.conv2d(x.double(), w(stem[0]), stride=2, padding=1)).clamp(0, 6)
    t = _bn64(f1[0][1], F.conv2d(x0, w(f1[0][0]), padding=1, groups=x0.shape[1])).clamp(0, 6)
    return x0, _bn64(f1[2], F.conv2d(t, w(f1[1])))


def chain_case(frame, features, seed=0):
    """`(x [n,3,H,W], Q {i: q}, g_c3 [n,32,h3,w3], g_x7 [n,64,h4,w4])` float32 numpy for `features`, a fresh
    `model_feature.mobilenet_v2_features()` whose stem and features[1] keep the weights they have (given non-trivial running
    statistics here, seeded): features[2:8] with every block calibrated on the float64 activations it sees from these frames."""
    n, H, W = frame
    base = 16000 + seed + n * H * W
    rs = np.random.RandomState(base)
    x = rs.standard_normal((n, 3, H, W)).astype(np.float32)
    gen = torch.Generator().manual_seed(base)
    with torch.no_grad():
        for m in list(features[0].modules()) + list(features[1].modules()):
            if isinstance(m, torch.nn.Conv2d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=gen) * (2.0 / (m.weight[0].numel())) ** 0.5)
            elif isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, generator=gen))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=gen))
                m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=gen))
                m.bias.copy_(0.5 + 0.5 * torch.randn(m.bias.shape, generator=gen))
    features.eval()
    xx = frozen_forward(features, torch.as_tensor(x))[1]
    Q = {}
    for i in range(FIRST, END):
        cfg = FEATURES[i]
        Q[i] = BK.calibrated(cfg, xx, rs, np.random.RandomState(base + 100 * i))
        xx = X.forward(BR.fold(BR.to64(Q[i])), xx, cfg[3], cfg[4])["o"]
    h3, w3 = down(down(down(H))), down(down(down(W)))
    g3 = (rs.standard_normal((n, 32, h3, w3)) / (h3 * w3)).astype(np.float32)
    g7 = (rs.standard_normal((n, 64, down(h3), down(w3))) / (down(h3) * down(w3))).astype(np.float32)
    return x, Q, g3, g7


def chain_forward(P, x1, keep=None):
    """x2 .. x7 in float64 from the folds `P` {i: fold}; `keep` receives `x<i>`, `e<i>`, `d<i>`."""
    x, xs = x1, {}
    for i in range(FIRST, END):
        f = X.forward(P[i], x, FEATURES[i][3], FEATURES[i][4])
        x = xs[i] = f["o"]
        if keep is not None:
            keep.update({"x%d" % i: x, "e%d" % i: f["e"], "d%d" % i: f["d"]})
    return xs


def chain_autograd(Q, x1, g3, g7, variant=None, masks=None):
    """The 54 gradients of sum(g3 x6) + sum(g7 x7) by torch autograd through the restated forward, from the module numbers `Q`
    (float64): `{"<i>.<name>": gradient}`.  `variant` "no_g_c3": the c3 term left out.  `masks` `{i: (me, md)}`: the ReLU6
    derivatives are the given ones (backbone_ref64._forward_masked), float64's own without."""
    keys = ("w1", "g1", "be1", "wd", "g2", "be2", "w3", "g3", "be3")
    leaves, P = {}, {}
    for i, q in Q.items():
        leaves[i] = {k: q[k].detach().clone().requires_grad_(True) for k in keys}
        qq = dict(q)
        qq.update(leaves[i])
        P[i] = BR.fold(qq)
    xs, x = {}, x1
    for i in range(FIRST, END):
        cfg = FEATURES[i]
        x = xs[i] = BK._forward_masked(P[i], x, cfg[3], cfg[4], masks[i]) if masks else X.forward(P[i], x, cfg[3], cfg[4])["o"]
    loss = (g7 * xs[END - 1]).sum() + (0 if variant == "no_g_c3" else (g3 * xs[C3]).sum())
    flat = [leaves[i][k] for i in range(FIRST, END) for k in keys]
    return dict(zip(PARAMS, torch.autograd.grad(loss, flat)))


def chain_closed(P, x1, g3, g7, variant=None, keep=None):
    """The 54 gradients from the CLOSED FORMS (no autograd): the float64 forward, then the walk of train.shallow_backward --
    block 7 from g7, + g3, blocks 6 .. 2.  `variant`: "no_g_c3", "no_residual" (every residual's gradient dropped), "s2_anchor"
    (the stride-2 windows), "no_pass7" (block 7's input gradient not passed on: block 6 sees g3 alone).  `keep` receives `g<i>`
    (the gradient of x_i) and the forward's tensors."""
    k = {} if keep is None else keep
    xs = chain_forward(P, x1, keep=k)
    xs[FIRST - 1] = x1
    out, g = {}, g7
    for i in range(END - 1, FIRST - 1, -1):
        _, _, _, stride, res = FEATURES[i]
        k["g%d" % i] = g
        x = xs[i - 1]
        pt = MP.block_parts(P[i], x, g, stride)
        if stride == 2:
            pt["ga"] = BK.ir_bwd(P[i], pt["gd"], pt["d"], pt["e"], 2, variant)
        gr = MP.grads_from_parts(P[i], x, pt["e"], pt["d"], pt["gd"], pt["ga"], g, stride)
        out.update({"%d.%s" % (i, n): gr[n] for n in NAMES})
        gx = conv_t(pt["ga"], P[i]["w1"], P[i]["s1"])
        if res and variant != "no_residual":
            gx = gx + g
        if i == C3 + 1:
            gx = (0 if variant == "no_pass7" else gx) + (0 if variant == "no_g_c3" else g3)
        g = gx
    return out
