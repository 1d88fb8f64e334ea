"""Float64 restatement of the parameter gradients of the multi-prior path (train.block_param_grads with stride 2 or 64 output
channels, train.prior_path_backward, csrc/train_ctx.hip: uavsal_ir_sums_s2, and the M tail of uavsal_pix_gemm), the seeded
inputs of their tests and the per-element bounds, in the convention of tests/block_ref64.py:

    |kernel - ref| <= bound,      U = 2^-24, LAMBDA = 8, EPS = 8 U (tests/plan_ref64.py),  D = 2^-53

The blocks are ctx_ref64.BLOCKS' "fucb192" / "fucb128" / "fucb64" (stride 1, 64 output channels, the last with the residual),
"ctx0" and "ctx1" (stride 2).  With stride 2 the tensors live on two grids: x, e, ga on the n H W INPUT pixels, d, gd, go on
the n Ho Wo OUTPUT pixels (Ho = (H-1)//2+1).  The sums (`ir_sums_s2_ref`):

    S2[c] = sum_out delta2      Gd[c][ky][kx] = sum_out delta2[oy][ox] e[2 oy - 1 + ky][2 ox - 1 + kx]  (zero outside)
    S3[m] = sum_out go          S1[c] = sum_in ga           G3 = sum_out go d          G1 = sum_in ga x

The kernels are tested teacher-forced, and every product is accumulated in double, so a sum's bound is the fp32 formation of
its terms plus the double accumulation (block_ref64's counts, n the number of pixels the sum runs over):

  delta2 = gd 1[d]        no arithmetic: the stored gd carries U |gd|:  err2 = U |gd| mask
  S2 = sum delta2         err2 + n_out D sum |delta2|
  Gd = sum delta2 e'      err2 |e'| + 2 U |delta2| |e'| (the stored e) + n_out D; the product is formed in double
  S1 = sum ga             U |ga| (the stored ga is rounded once) + n_in D
  S3 = sum go             go is an input: n_out D sum |go| alone
  G1 = sum ga x           (LAMBDA U sqrt(n_in) + U) sum |ga| |x|     (the fp32 MFMA chains of uavsal_pix_gemm; U: the stored ga)
  G3 = sum go d           (LAMBDA U sqrt(n_out) + 2 U) sum |go| |d|  (2 U: the stored d)
and each final tensor takes the absolute-value chain of its formula and EPS on its absolute terms for the final rounding,
exactly as block_ref64.param_grads does.  When the reference is fed the very fp32 tensors the device read (`grads_from_parts`
on the parts of a walk: the stage-by-stage form), the U terms of the stored tensors are slack, not error.  No factor is
fitted to what a kernel gives.

The slabs of uavsal_ir_sums_s2 are restated in `slab_partition_s2`, the tiles of uavsal_pix_gemm with an M tail in
`gemm_partition`.  Every function takes and returns float64 tensors on the device of its inputs unless it says numpy."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import block_ref64 as BR
import ctx_ref64 as X
import decoder_ref64 as DR
from plan_ref64 import EPS, LAMBDA, U

D = DR.D
NAMES = BR.NAMES
NSUM = BR.NSUM
SLAB_INPUT_PIXELS, MAX_SLABS = 256, 256                          # csrc/train_ctx.hip
PATH_BLOCKS = ("fucb_layer.0", "cxt_cb_prior.1", "cxt_cb_prior.0")      # train.PRIOR_PATH_BLOCKS
PATH_KEYS = dict(zip(PATH_BLOCKS, ("fucb", "ctx1", "ctx0")))     # -> the keys of ctx_ref64.head_case
SUMS_SHAPES = [(1, 1, 1, 64, 64), (2, 3, 2, 64, 64), (1, 5, 7, 384, 64), (2, 23, 40, 384, 64), (1, 45, 80, 1536, 64)]      # n, H, W, Ch, Co
SUMS_WRONG = ("stride1_e", "s1_output_grid", "no_top_pad")
TRAINED = ("fucb192", "fucb128", "fucb64", "ctx0", "ctx1")       # the real block shapes (ctx_ref64.BLOCKS)
TRAINED_SHAPES = [(2, 5, 7), (2, 23, 40)]                        # (n, H, W) of the block's INPUT
GOLDEN_BIAS, GOLDEN_SHAPE, GOLDEN_T = [(1, 1, 1), (0, 0, 1), (1, 1, 0)], (4, 9, 13), 2      # tests/golden/ctx_train_*.npz
GEMM_M, GEMM_N, GEMM_K = (64, 192), (64, 384), (1, 33, 1025)
W_SUBSET = (slice(None, None, 9), slice(None, None, 11))       # the strided part of the W1 / W3 gradients the goldens keep

down, m6, _v = X.down, X.m6, X._v


def golden_name(bias):
    return "ctx_train_b%d%d%d_N%d_%dx%d" % (tuple(bias) + GOLDEN_SHAPE)


# ------------------------------------------------------------------------------------------------ partitions, restated
def gemm_partition(K, M, N):
    """The K split of uavsal_pix_gemm with M and N multiples of 64: `(cps, shares)` over ceil(M / 128) ceil(N / 128) tiles
    (for M % 128 == 0 this is block_ref64.gemm_partition)."""
    tiles = -(-M // BR.GEMM_TILE) * -(-N // BR.GEMM_TILE)
    chunks = -(-K // BR.GEMM_CHAIN)
    most = max(1, min(BR.GEMM_TARGET_WGS // tiles, chunks))
    cps = -(-chunks // most)
    return cps, -(-chunks // cps)


def slab_partition_s2(n, H, W):
    """The slabs of uavsal_ir_sums_s2: `(OUTPUT rows per slab, slabs)` over the n * Ho output rows; a slab's input rows (two per
    output row) hold about SLAB_INPUT_PIXELS pixels."""
    rows = n * down(H)
    sr = max(-(-SLAB_INPUT_PIXELS // (2 * W)), -(-rows // MAX_SLABS))
    return sr, -(-rows // sr)


# ------------------------------------------------------------------------------------------------ the sums
def tap_sums(a, b, stride):
    """[c, ky, kx] = sum over images and OUTPUT pixels of a[n, c, oy, ox] b[n, c, s oy - 1 + ky, s ox - 1 + kx], zero outside."""
    if stride == 1:
        return DR._tap_sums(a, b)
    n, c, Ho, Wo = a.shape
    H, W = b.shape[2:]
    bp = F.pad(b, (1, 2 * Wo - W, 1, 2 * Ho - H))                # rows -1 .. 2 Ho - 1: everything a tap can reach
    out = a.new_zeros((c, 3, 3))
    for ky in range(3):
        for kx in range(3):
            out[:, ky, kx] = (a * bp[:, :, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2][:, :, :Ho, :Wo]).sum((0, 2, 3))
    return out


def ir_sums_s2_ref(gd, d, e, ga, go, variant=None, bounds=False):
    """uavsal_ir_sums_s2 + the slab sum of uavsal_ir_finish from stored NCHW tensors: dict(S2 [Ch], Gd [Ch,3,3], S1 [Ch],
    S3 [Co]); `bounds`: `(sums, bounds)`, the first four lines of the module docstring's list.
    `variant` (WRONG kernels): "stride1_e": Gd reads e at (oy - 1 + ky, ox - 1 + kx), the indexing of uavsal_ir_sums;
    "s1_output_grid": S1 runs over the Ho x Wo top-left pixels of ga only; "no_top_pad": Gd reads e at (2 oy + ky, 2 ox + kx):
    the taps of an unpadded grid, no zero row at -1."""
    Ho, Wo = d.shape[2:]
    d2 = gd * m6(d)
    if variant == "stride1_e":
        Gd = DR._tap_sums(d2, e[:, :, :Ho, :Wo])
    elif variant == "no_top_pad":
        Gd = tap_sums(d2, F.pad(e, (0, 1, 0, 1))[:, :, 1:, 1:], 2)
    else:
        Gd = tap_sums(d2, e, 2)
    S1 = (ga[:, :, :Ho, :Wo] if variant == "s1_output_grid" else ga).sum((0, 2, 3))
    s = {"S2": d2.sum((0, 2, 3)), "Gd": Gd, "S1": S1, "S3": go.sum((0, 2, 3))}
    if not bounds:
        return s
    n_out, n_in = d.shape[0] * Ho * Wo, e.shape[0] * e.shape[2] * e.shape[3]
    a2 = gd.abs() * m6(d)
    b = {"S2": ((U + n_out * D) * a2).sum((0, 2, 3)), "Gd": tap_sums((3 * U + n_out * D) * a2, e.abs(), 2),
         "S1": (U + n_in * D) * ga.abs().sum((0, 2, 3)), "S3": n_out * D * go.abs().sum((0, 2, 3))}
    return s, b


def sums_case(shape, seed=0):
    """Teacher-forced inputs of uavsal_ir_sums_s2, float32 numpy NCHW: ctx_ref64.s2_case's `(gd, d, e)` + `ga [n,Ch,H,W]`,
    `go [n,Co,Ho,Wo]`."""
    n, H, W, Ch, Co = shape
    gd, d, e, _, _ = X.s2_case((n, H, W, Ch), seed)
    rs = np.random.RandomState(9100 + seed + n * H * W + Ch)
    ga = (rs.standard_normal((n, Ch, H, W)) * (rs.random_sample((n, Ch, H, W)) < 0.7)).astype(np.float32)
    go = rs.standard_normal((n, Co, down(H), down(W))).astype(np.float32)
    return gd, d, e, ga, go


# ------------------------------------------------------------------------------------------------ the nine gradients
def grads_from_parts(p, x, e, d, gd, ga, go, stride, bounds=False, variant=None):
    """The nine gradients of a block with the eval fold `p` (block_ref64.fold's keys) from GIVEN x, e, d, gd, ga, go (NCHW
    float64; x, e, ga on the input grid, d, gd, go on the output grid): the closed form of include/uavsal_hip.h, keyed by
    NAMES, in the parameters' shapes.  `bounds`: `(grads, bounds)`, the module docstring's.  `variant`: one of SUMS_WRONG."""
    hid, cin = p["w1"].shape[:2]
    cout = p["w3"].shape[0]
    s1, s2, s3 = p["s1"], p["s2"], p["s3"]
    w1, wdm, w3 = p["w1"].reshape(hid, cin), p["wd"].reshape(hid, 3, 3), p["w3"].reshape(cout, hid)
    md = m6(d).double()
    d2 = gd * md
    if stride == 2:
        S = ir_sums_s2_ref(gd, d, e, ga, go, variant=variant)
        S1, S2, S3, Gd = S["S1"], S["S2"], S["S3"], S["Gd"]
    else:
        S1, S2, S3, Gd = ga.sum((0, 2, 3)), d2.sum((0, 2, 3)), go.sum((0, 2, 3)), DR._tap_sums(d2, e)
    G1 = torch.einsum("tchw,tjhw->cj", ga, x)
    G3 = torch.einsum("tmhw,tchw->mc", go, d)
    g = {NAMES[0]: s1.view(-1, 1) * G1, NAMES[1]: p["r1"] * ((w1 * G1).sum(1) - p["mu1"] * S1), NAMES[2]: S1,
         NAMES[3]: s2.view(-1, 1, 1) * Gd, NAMES[4]: p["r2"] * ((wdm * Gd).sum((1, 2)) - p["mu2"] * S2), NAMES[5]: S2,
         NAMES[6]: s3.view(-1, 1) * G3, NAMES[7]: p["r3"] * ((w3 * G3).sum(1) - p["mu3"] * S3), NAMES[8]: S3}
    shapes = {NAMES[0]: (hid, cin, 1, 1), NAMES[3]: (hid, 1, 3, 3), NAMES[6]: (cout, hid, 1, 1)}
    g = {k: t.reshape(shapes.get(k, t.shape)) for k, t in g.items()}
    if not bounds:
        return g
    n_in = x.shape[0] * x.shape[2] * x.shape[3]
    n_out = d.shape[0] * d.shape[2] * d.shape[3]
    a2 = gd.abs() * md
    eS2 = ((U + n_out * D) * a2).sum((0, 2, 3))
    eGd = tap_sums((3 * U + n_out * D) * a2, e.abs(), stride)
    eS1 = (U + n_in * D) * ga.abs().sum((0, 2, 3))
    eS3 = n_out * D * go.abs().sum((0, 2, 3))
    AG1 = torch.einsum("tchw,tjhw->cj", ga.abs(), x.abs())
    AG3 = torch.einsum("tmhw,tchw->mc", go.abs(), d.abs())
    eG1 = (LAMBDA * U * math.sqrt(n_in) + U) * AG1
    eG3 = (LAMBDA * U * math.sqrt(n_out) + 2 * U) * AG3
    aGd = tap_sums(a2, e.abs(), stride)
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


def block_parts(p, x, go, stride):
    """e, d, gd, ga (NCHW float64) of the block with fold `p` from its input and the gradient at its output."""
    f = X.forward(p, x, stride, False)
    gd = F.conv_transpose2d(go * _v(p["s3"]), p["w3"])
    ga = X._dw_back(gd * m6(f["d"]), p["wd"], stride, x.shape[2:]) * _v(p["s2"]) * m6(f["e"])
    return {"e": f["e"], "d": f["d"], "gd": gd, "ga": ga}


def param_grads(p, x, go, stride, bounds=False, parts=None, variant=None):
    """The nine gradients of d sum(go o) / d parameter of a block (fold `p`), stride 1 or 2, from the float64 forward."""
    pt = block_parts(p, x, go, stride)
    if parts is not None:
        parts.update(pt)
    return grads_from_parts(p, x, pt["e"], pt["d"], pt["gd"], pt["ga"], go, stride, bounds=bounds, variant=variant)


def autograd_grads(q, x, go, stride, res):
    """torch autograd through the restated forward, from the module's numbers `q`: the nine gradients keyed by NAMES."""
    keys = ("w1", "g1", "be1", "wd", "g2", "be2", "w3", "g3", "be3")
    leaves = {k: q[k].detach().clone().requires_grad_(True) for k in keys}
    qq = dict(q)
    qq.update(leaves)
    o = X.forward(BR.fold(qq), x, stride, res)["o"]
    return dict(zip(NAMES, torch.autograd.grad(o, [leaves[k] for k in keys], go)))


# ------------------------------------------------------------------------------------------------ the whole path
def path_inputs(P, fu, cbcat, gfu, T, n_prior, given=None, variant=None):
    """What the walk of train.prior_path_backward hands each trained block, float64: `{name of PATH_BLOCKS: (x, go, stride)}`
    (the context blocks only when `P` has them).  `given`: float64 tensors g_cb, g_ctx2, g_ctx1, ctx1, ctx_sum that replace the
    float64 results of the stages before (the teacher-forced form).  `variant` "per_frame" (a WRONG walk): cxt_cb_prior is fed
    the N frames, and the N-frame gradient, where the chunk sums over T frames (B = N / T images) belong."""
    given = given or {}
    N, _, h, w = fu.shape
    B = N // T
    out = {PATH_BLOCKS[0]: (cbcat, gfu[:, 256:], 1)}
    if "ctx0" not in P:
        return out
    g_cb = given.get("g_cb")
    if g_cb is None:
        g_cb = X.input_grad_ref(P["fucb"], cbcat, gfu[:, 256:], 1, cbcat.shape[1] == 64)
    sl = slice(64 * n_prior, 64 * n_prior + 64)
    h2, w2 = down(down(h)), down(down(w))
    if variant == "per_frame":
        g_c2 = X.bilinear_bwd_ref(g_cb[:, sl], N, h2, w2, N, 1)
        csum = fu[:, :256]
    else:
        g_c2 = given.get("g_ctx2")
        if g_c2 is None:
            g_c2 = X.bilinear_bwd_ref(g_cb[:, sl], B, h2, w2, B, 1)
        csum = given.get("ctx_sum")
        if csum is None:
            csum = fu[:, :256].reshape(B, T, 256, h, w).sum(1)
    c1 = given.get("ctx1") if variant is None else None
    if c1 is None:
        c1 = X.forward(P["ctx0"], csum, 2, False)["o"]
    g_c1 = given.get("g_ctx1") if variant is None else None
    if g_c1 is None:
        g_c1 = X.input_grad_ref(P["ctx1"], c1, g_c2, 2, False)
    out[PATH_BLOCKS[1]] = (c1, g_c2, 2)
    out[PATH_BLOCKS[2]] = (csum, g_c1, 2)
    return out


def path_param_grads(P, fu, cbcat, gfu, T, n_prior, variant=None):
    """The 9 (27 with the context prior) gradients of the path in float64 closed form: `{name: {NAMES: tensor}}`."""
    return {n: param_grads(P[PATH_KEYS[n]], x, go, s) for n, (x, go, s) in path_inputs(P, fu, cbcat, gfu, T, n_prior, variant=variant).items()}


def path_autograd(Q, f, priors, gfu, T, use_ctx):
    """torch autograd of sum(gfu fu) through ctx_ref64.tail_forward from fust_layer's output `f` on, with respect to the
    parameters of the path's blocks: `{name: {NAMES: tensor}}`.  `Q`: the blocks' numbers as float64 tensors."""
    keys = ("w1", "g1", "be1", "wd", "g2", "be2", "w3", "g3", "be3")
    names = [n for n in PATH_BLOCKS if PATH_KEYS[n] in Q and (use_ctx or n == PATH_BLOCKS[0])]
    leaves = {n: {k: Q[PATH_KEYS[n]][k].detach().clone().requires_grad_(True) for k in keys} for n in names}
    P = {}
    for key, q in Q.items():
        qq = dict(q)
        for n in names:
            if PATH_KEYS[n] == key:
                qq.update(leaves[n])
        P[key] = BR.fold(qq)
    fu = X.tail_forward(P, f, priors, T, use_ctx)["fu"]
    flat = [leaves[n][k] for n in names for k in keys]
    gs = torch.autograd.grad(fu, flat, gfu)
    return {n: dict(zip(NAMES, gs[9 * i:9 * i + 9])) for i, n in enumerate(names)}


def path_digest(Q, st, priors, go):
    return X.head_digest(Q, st, priors, go)
