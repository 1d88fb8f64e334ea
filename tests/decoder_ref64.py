"""Float64 restatement of the decoder's parameter gradients (train.decoder_param_grads, csrc/train_decoder.hip), the seeded
inputs of its tests and the per-element bounds, in the convention of tests/train_ref64.py:

    |kernel - ref| <= bound,      U = 2^-24, LAMBDA = 8, EPS = 8 U (tests/plan_ref64.py)

The decoder is `train_ref64.decoder_inputs(shape)` with BatchNorms whose running statistics are NOT trivial (`decoder_case`):
per channel r = 1 / sqrt(var + eps) drawn from {0.5, 1, 2}, eps = 2^-20, var = 1 / r^2 - 2^-20 (so var + eps and the fold
gamma r are exact in fp32), mu ~ N(0, 1), gamma = s / r, beta = fl(b + mu s) with (s, b) the fold of `decoder_inputs`.  The
restatement works from the MODULE's numbers (gamma, beta, mu, var as fp32 values, in float64 arithmetic), as autograd does.

The kernels are tested teacher-forced: they are handed the float64 e, d, y, ga ROUNDED to fp32, and the reference is the
pure float64 closed form (the one the committed autograd goldens confirm).  The bounds therefore count, on sums of absolute
values, the rounding of every fp32 input the kernels read and every fp32 operation they do, one by one (D = 2^-53):

  delta3 = gy y (1 - y)   the input y carries U y; through y (1 - y) that is U y |1 - 2 y| -- NOT relative to y (1 - y), which
                          a y near 1 would make large -- and the kernel rounds three times (gy y, 1 - y, the product):
                              err3 = |gy| U y |1 - 2 y| + 3 U |delta3|
  delta2 = delta3 s3 w3   two more products:  err2 = (err3 + 2 U |delta3|) |s3 w3| mask
  S3 = sum delta3         err3 summed, + n D sum |delta3| for the double accumulation over n = T H W terms (every sum below
                          carries that term on its own sum of absolute values; it is ~1e-11 of it)
  G3 = sum delta3 d       err3 |d| + 2 U |delta3| |d| (the stored d is within 2 U of the float64 d, see `teacher_round`; the
                          product is formed in double: exact)
  S2 = sum delta2         err2
  Gd = sum delta2 e'      err2 |e'| + 2 U |delta2| |e'| (the stored e, likewise)
  S1 = sum ga             U |ga| (the stored ga is rounded once)
  G1 = sum ga h           (LAMBDA U sqrt(T h w) + U) sum |ga| |h|: the exact-fp32 MFMA chains, the fp32 adds of the chains and
                          the double sum of the shares as for uavsal_twa_wgrad (tests/train_ref64.py), + U for the stored ga
Each final tensor takes the absolute-value chain of its formula and EPS on its absolute terms for the final rounding (the
scale s, r and mu are exact inputs; the multiplications by them are done in double):
  W = s G:  |s| err(G) + EPS |s G|        beta = S:  err(S) + EPS |S|
  gamma = r (sum W G - mu S):  r (sum |W| err(G) + |mu| err(S)) + EPS r (sum |W G| + |mu S|)
No factor is fitted to what a kernel gives.

Shapes beyond `train_ref64.SHAPES`:
* GEMM_SPLIT_SHAPE (12, 45, 80): K = 43200, 43 chunks of 1024, 24 tiles -> at most 1024 // 24 = 42 shares -> 2 chunks per
  share, 22 shares, the last one a single chunk of 192 pixels: the smallest K at which a share of uavsal_pix_gemm holds two
  chunks (one chain ends and another starts inside a workgroup).  Random operands (`gemm_inputs`).
* SLAB_SHAPE (2, 45, 80): 90 picture rows in slabs of ceil(512 / 80) = 7 rows: 13 slabs per channel group, the last one 6
  rows, and the slab [42, 49) holds the last rows of frame 0 and the first of frame 1.  It is one of SHAPES.

Every function takes and returns float64 tensors on the device of its inputs unless it says numpy."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import train_ref64 as R
from plan_ref64 import EPS, LAMBDA, U

HID, C = R.HID, R.C
NAMES = ("conv.0.0.weight", "conv.0.1.weight", "conv.0.1.bias", "conv.1.0.weight", "conv.1.1.weight", "conv.1.1.bias",
         "conv.2.weight", "conv.3.weight", "conv.3.bias")
SHAPES, GOLDEN_SHAPES = R.SHAPES, R.GOLDEN_SHAPES
GEMM_SPLIT_SHAPE = (12, 45, 80)
SLAB_SHAPE = (2, 45, 80)
BN_EPS = 2.0 ** -20
ZERO_GAMMA = (37, 1201)                        # channel with gamma1 = 0, channel with gamma2 = 0 (decoder_case(zero_gamma=True))
GEMM_CHAIN, GEMM_TARGET_WGS, GEMM_TILE = 1024, 1024, 128        # csrc/pix_gemm_tile.h, restated
SLAB_PIXELS, MAX_SLABS = 512, 256                               # csrc/train_decoder.hip, restated
WRONG = ("taps_flipped", "halo_across_frames", "nonstrict_masks", "no_mu_term", "s1_twice", "last_share")
W1_SUBSET = (slice(None, None, 5), slice(None, None, 7))        # the strided part of W1's gradient the goldens keep
D = 2.0 ** -53


def name(shape):
    return "decoder_T%d_%dx%d" % shape


# ------------------------------------------------------------------------------------------------ inputs (float32 numpy)
def bn_stats(shape):
    rs = np.random.RandomState(R.SEED[shape] + 4000)
    out = {}
    for i, n in ((1, HID), (2, HID), (3, 1)):
        out["r%d" % i] = rs.choice(np.array([0.5, 1.0, 2.0], np.float32), n)
        out["mu%d" % i] = rs.standard_normal(n).astype(np.float32)
    return out


def decoder_case(shape, zero_gamma=False):
    """`(h [T,256,H,W], q, gy [T,1,H,W])`: the history and the incoming gradient of `train_ref64.decoder_inputs` and the
    decoder's MODULE numbers q = {w1, wd, w3, g*, be*, mu*, var*} (* = 1, 2, 3; float32 numpy).  `zero_gamma`: gamma1 of
    channel ZERO_GAMMA[0] and gamma2 of channel ZERO_GAMMA[1] are 0 and their beta 1.5 (inside the ReLU6's open range: the
    channel is a constant that lets its gradient through)."""
    h, p, gy = R.decoder_inputs(shape)
    st = bn_stats(shape)
    q = {k: p[k] for k in ("w1", "wd", "w3")}
    for i in (1, 2, 3):
        r, mu, s, b = st["r%d" % i], st["mu%d" % i], p["s%d" % i], p["b%d" % i]
        var = 1.0 / r.astype(np.float64) ** 2 - BN_EPS
        assert np.all(var.astype(np.float32).astype(np.float64) == var)
        q["g%d" % i] = (s / r).astype(np.float32)
        q["be%d" % i] = (b.astype(np.float64) + mu.astype(np.float64) * s).astype(np.float32)
        q["mu%d" % i], q["var%d" % i] = mu, var.astype(np.float32)
    if zero_gamma:
        for i, c in ((1, ZERO_GAMMA[0]), (2, ZERO_GAMMA[1])):
            q["g%d" % i][c] = 0.0
            q["be%d" % i][c] = 1.5
    return h, q, gy


def fold(q):
    """`q` as float64 tensors -> the eval fold `train_ref64.decoder_forward` takes (s = gamma r, b = beta - mu s), + r*, mu*."""
    p = {k: q[k] for k in ("w1", "wd", "w3")}
    for i in (1, 2, 3):
        r = 1.0 / torch.sqrt(q["var%d" % i] + BN_EPS)
        p["r%d" % i], p["mu%d" % i] = r, q["mu%d" % i]
        p["s%d" % i] = q["g%d" % i] * r
        p["b%d" % i] = q["be%d" % i] - q["mu%d" % i] * p["s%d" % i]
    return p


def load_block(block, q):
    """Put `decoder_case`'s numbers into a dwBlock(256, 1) (the package's or the reference's) and switch it to eval mode."""
    seq = block.conv
    with torch.no_grad():
        for conv, k in ((seq[0][0], "w1"), (seq[1][0], "wd"), (seq[2], "w3")):
            conv.weight.copy_(torch.as_tensor(q[k]))
        for i, bn in ((1, seq[0][1]), (2, seq[1][1]), (3, seq[3])):
            bn.weight.copy_(torch.as_tensor(q["g%d" % i]))
            bn.bias.copy_(torch.as_tensor(q["be%d" % i]))
            bn.running_mean.copy_(torch.as_tensor(q["mu%d" % i]))
            bn.running_var.copy_(torch.as_tensor(q["var%d" % i]))
            bn.eps = BN_EPS
    return block.eval()


def gemm_inputs(shape, seed=7000):
    """Random operands of the pixel GEMM for a shape no decoder test uses: `(a [T,H,W,1536], b [T,H,W,256])` float32 numpy NHWC."""
    T, H, W = shape
    rs = np.random.RandomState(seed + T * H * W)
    return (1e-2 * rs.standard_normal((T, H, W, HID))).astype(np.float32), rs.standard_normal((T, H, W, C)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ partitions, restated
def gemm_partition(K, M=HID, N=C):
    """The K split of uavsal_pix_gemm: `(cps, shares, [(p0, p1) per share])` (the rule of train_ref64.wgrad_partition with
    (M / 128)(N / 128) tiles)."""
    tiles = (M // GEMM_TILE) * (N // GEMM_TILE)
    chunks = -(-K // GEMM_CHAIN)
    most = max(1, min(GEMM_TARGET_WGS // tiles, chunks))
    cps = -(-chunks // most)
    span = cps * GEMM_CHAIN
    spans = [(p, min(p + span, K)) for p in range(0, K, span)]
    return cps, len(spans), spans


def slab_partition(T, H, W):
    """The slabs of uavsal_dec_sums: `(rows per slab, slabs)` over the T * H picture rows."""
    rows = T * H
    sr = max(-(-SLAB_PIXELS // W), -(-rows // MAX_SLABS))
    return sr, -(-rows // sr)


# ------------------------------------------------------------------------------------------------ the closed form
def _v(t):
    return t.reshape(1, -1, 1, 1)


def _tap_sums(a, b, across_frames=False):
    """[c, ky, kx] = sum over frames and pixels of a[t, c, y, x] b[t, c, y + ky - 1, x + kx - 1], zero outside the picture.
    `across_frames` (a WRONG kernel): the frames are read as one tall picture, so a border row sees the neighbouring frame."""
    T, c, H, W = a.shape
    if across_frames:
        a, b = a.permute(1, 0, 2, 3).reshape(1, c, T * H, W), b.permute(1, 0, 2, 3).reshape(1, c, T * H, W)
    bp = F.pad(b, (1, 1, 1, 1))
    hh = a.shape[2]
    out = a.new_zeros((c, 3, 3))
    for ky in range(3):
        for kx in range(3):
            out[:, ky, kx] = (a * bp[:, :, ky:ky + hh, kx:kx + W]).sum((0, 2, 3))
    return out


def param_grads(q, h, gy, variant=None, bounds=False, parts=None):
    """The nine gradients of d sum(gy y) / d parameter, keyed by NAMES, in the parameters' shapes; `bounds`: returns
    `(grads, bounds)` with the per-element bounds of the docstring.  `variant`: one of WRONG, the result of a kernel that gets
    that one thing wrong.  `parts`: a dict that receives e, d, y, ga (NCHW) and grad_h."""
    p = fold(q)
    f = R.decoder_forward(p, h)
    e, d, y = f["e"], f["d"], f["y"]
    if variant == "nonstrict_masks":
        me, md = ((e >= 0) & (e <= 6)).double(), ((d >= 0) & (d <= 6)).double()
    else:
        me, md = ((e > 0) & (e < 6)).double(), ((d > 0) & (d < 6)).double()
    s1, s2, s3 = p["s1"], p["s2"], p["s3"]
    w1, wd, w3 = q["w1"].reshape(HID, C), q["wd"], q["w3"].reshape(-1)
    d3 = gy * y * (1 - y)
    d2 = d3 * s3 * _v(w3) * md
    ga = F.conv_transpose2d(d2, wd, padding=1, groups=HID) * _v(s2) * me
    T, _, H, W = h.shape
    K = T * H * W
    gaw = ga
    if variant == "last_share":
        wt = torch.ones(K, dtype=ga.dtype, device=ga.device)
        p0, p1 = gemm_partition(K)[2][-1]
        wt[p0:p1] = 0
        gaw = ga * wt.view(T, 1, H, W)
    G1 = torch.einsum("tchw,tjhw->cj", gaw, h)
    S1, S2, S3 = ga.sum((0, 2, 3)), d2.sum((0, 2, 3)), d3.sum()
    G3 = (d3 * d).sum((0, 2, 3))
    Gd = _tap_sums(d2, e, across_frames=variant == "halo_across_frames")
    if variant == "taps_flipped":
        Gd = Gd.flip(1, 2)
    wdm = wd.reshape(HID, 3, 3)
    mu1S = 0 if variant == "no_mu_term" else p["mu1"] * S1
    g = {NAMES[0]: (s1 * s1 if variant == "s1_twice" else s1).view(-1, 1) * G1,
         NAMES[1]: p["r1"] * ((w1 * G1).sum(1) - mu1S), NAMES[2]: S1,
         NAMES[3]: s2.view(-1, 1, 1) * Gd, NAMES[4]: p["r2"] * ((wdm * Gd).sum((1, 2)) - p["mu2"] * S2), NAMES[5]: S2,
         NAMES[6]: s3 * G3, NAMES[7]: p["r3"] * ((w3 * G3).sum() - p["mu3"] * S3), NAMES[8]: S3.reshape(1)}
    shapes = {NAMES[0]: (HID, C, 1, 1), NAMES[3]: (HID, 1, 3, 3), NAMES[6]: (1, HID, 1, 1), NAMES[7]: (1,)}
    g = {k: v.reshape(shapes.get(k, v.shape)) for k, v in g.items()}
    if parts is not None:
        parts.update(e=e, d=d, y=y, ga=ga, grad_h=F.conv_transpose2d(ga * _v(s1), q["w1"]), e_pre=f["e_pre"], d_pre=f["d_pre"])
    if not bounds:
        return g
    n = K
    a3 = d3.abs()
    err3 = gy.abs() * U * y * (1 - 2 * y).abs() + 3 * U * a3
    a2 = a3 * (s3 * _v(w3)).abs() * md
    err2 = (err3 + 2 * U * a3) * (s3 * _v(w3)).abs() * md
    eS3 = err3.sum() + n * D * a3.sum()
    eG3 = ((err3 + 2 * U * a3 + n * D * a3) * d.abs()).sum((0, 2, 3))
    eS2 = (err2 + n * D * a2).sum((0, 2, 3))
    eGd = _tap_sums(err2 + (2 * U + n * D) * a2, e.abs())
    eS1 = (U + n * D) * ga.abs().sum((0, 2, 3))
    AG1 = torch.einsum("tchw,tjhw->cj", ga.abs(), h.abs())
    eG1 = (LAMBDA * U * math.sqrt(n) + U) * AG1
    aGd = _tap_sums(a2, e.abs())
    aG3 = (a3 * d.abs()).sum((0, 2, 3))
    r1, r2, r3, mu1, mu2, mu3 = (p[k].abs() for k in ("r1", "r2", "r3", "mu1", "mu2", "mu3"))
    aS1, aS2, aS3 = ga.abs().sum((0, 2, 3)), a2.sum((0, 2, 3)), a3.sum()
    b = {NAMES[0]: s1.abs().view(-1, 1) * (eG1 + EPS * AG1),
         NAMES[1]: r1 * ((w1.abs() * eG1).sum(1) + mu1 * eS1) + EPS * r1 * ((w1.abs() * AG1).sum(1) + mu1 * aS1),
         NAMES[2]: eS1 + EPS * aS1,
         NAMES[3]: s2.abs().view(-1, 1, 1) * (eGd + EPS * aGd),
         NAMES[4]: r2 * ((wdm.abs() * eGd).sum((1, 2)) + mu2 * eS2) + EPS * r2 * ((wdm.abs() * aGd).sum((1, 2)) + mu2 * aS2),
         NAMES[5]: eS2 + EPS * aS2,
         NAMES[6]: s3.abs() * (eG3 + EPS * aG3),
         NAMES[7]: r3 * ((w3.abs() * eG3).sum() + mu3 * eS3) + EPS * r3 * ((w3.abs() * aG3).sum() + mu3 * aS3),
         NAMES[8]: (eS3 + EPS * aS3).reshape(1)}
    b = {k: v.reshape(g[k].shape) for k, v in b.items()}
    return g, b


def autograd_grads(q, h, gy):
    """torch autograd through the restated forward, from the module's numbers: the nine gradients keyed by NAMES."""
    leaves = {k: q[k].detach().clone().requires_grad_(True) for k in ("w1", "g1", "be1", "wd", "g2", "be2", "w3", "g3", "be3")}
    qq = dict(q)
    qq.update(leaves)
    y = R.decoder_forward(fold(qq), h)["y"]
    gs = torch.autograd.grad(y, [leaves[k] for k in ("w1", "g1", "be1", "wd", "g2", "be2", "w3", "g3", "be3")], gy)
    return dict(zip(NAMES, gs))


def pix_gemm_ref(a, b):
    """uavsal_pix_gemm on NHWC float64 `a [T,H,W,M]`, `b [T,H,W,N]`: `(G [M,N], bound)` with row_scale 1."""
    n = a.shape[0] * a.shape[1] * a.shape[2]
    A, B = a.reshape(n, -1), b.reshape(n, -1)
    return A.T @ B, LAMBDA * U * math.sqrt(n) * (A.abs().T @ B.abs())


def mask_flips(t64):
    """How many elements of a ReLU6 output change their strict mask 0 < t < 6 when t is rounded to fp32."""
    t32 = t64.float().double()
    return int((((t64 > 0) & (t64 < 6)) != ((t32 > 0) & (t32 < 6))).sum())


def teacher_round(t64):
    """A ReLU6 output as the fp32 tensor the teacher-forced tests hand to the kernels: rounded to nearest, except that an
    element strictly inside (0, 6) which rounding would carry ONTO a clamp (a float64 value within 2.4e-7 of 6: about one in
    1e7 elements) is kept one fp32 step inside, so that the stored value decides the mask as the float64 one does.  Such an
    element is within one fp32 step below 6, 2^-21 = 1.33 U * 6: every stored element is within 2 U of the float64 one."""
    t32 = t64.float()
    inside = (t64 > 0) & (t64 < 6)
    six, zero = torch.tensor(6.0, device=t64.device), torch.tensor(0.0, device=t64.device)
    t32 = torch.where(inside & (t32 >= 6), torch.nextafter(six, zero), t32)
    return torch.where(inside & (t32 <= 0), torch.nextafter(zero, six), t32)


def to64(d, device="cpu"):
    return R.to64(d, device)
