"""Float64 restatement of the trainable slice of train/ -- the ConvTWA cell, back-propagation through time, the decoder
conv_out_st + sigmoid and its input gradient -- written with torch's own operators, the seeded inputs of the tests, and the
per-element bounds of the three kernels of csrc/train.hip in the convention of tests/plan_ref64.py:

    |kernel - y| <= rtol * B + EPS * E                  U = 2^-24, LAMBDA = 8, EPS = 8 U (from there)

* weight gradient (a sum over T H W products per element): rtol = LAMBDA U sqrt(T H W), B = sum |dz| |cat|.
* input-gradient convs (sums over 9 * 256 products): plan_ref64.rtol("f32", 9 * 256), B = the conv on absolute values
  (+ |res|), E = |conv| + |res| + |y| as plan_ref64.ref_conv has it.
* uavsal_dec_bwd: (LAMBDA * 3 + 8) U on the absolute-value chain (a sum of 9 products, LAMBDA sqrt(9), and at most eight
  element-wise roundings: gy y, 1 - y, the product, s3, w3, the tap weight, s1 s2, the last product).
* uavsal_twa_gate_bwd: EPS * E with E the roundings counted one by one, in units of U / 8.  expf is 1 ulp = 2 U, so
  1 / (1 + e) carries at most 3 U and e / (1 + e) at most 5 U; g = G + carry and x - h one rounding each, relative to
  |G| + |carry| and |x| + |h|; three products.  dz: [(|G| + |carry|) |x - h| + |g| (|x| + |h|)] i (1 - i) + 11 |dz|;
  carry' = g (1 - i): (|G| + |carry|) (1 - i) + 6 |carry'|; dx = g i the same with i.

The weight gradient's K split (csrc/train.hip: chunks of 1024 pixels, `cps` whole chunks per workgroup = one share) is at
its degenerate value cps = 1 in every shape of SHAPES.  WGRAD_SPLIT_SHAPES are the smallest shapes with a real partition,
for the weight-gradient tests only (a 1536-channel float64 decoder at these sizes would gain nothing):
* (20,27,27): K = 14580, 15 chunks, cps = 2, 8 shares, the last one 244 pixels (7.6 K steps).  The smallest K with cps = 2:
  every share but the last ends one chain and starts another; frames of 729 pixels straddle every 32-pixel K step and every
  chunk border; h0 and then 19 history frames.
* (9,45,80): K = 32400, 32 chunks, cps = 3, 11 shares, the last one 1680 = 1024 + 656 pixels: fewer chunks than the others,
  and it ends in a partial chain whose final K step is half filled.  The real map.
`wgrad_partition` restates the split, `wgrad_wrong_refs` are the float64 results of four kernels that get it wrong (the
idiom of plan_ref64's chan / row / bias); the CPU test holds each at least 4 bounds from the right one.

Every function takes and returns float64 NCHW tensors on the device of its inputs."""
import hashlib
import math

import numpy as np
import torch
import torch.nn.functional as F

from plan_ref64 import EPS, LAMBDA, U, rtol

C = 256
HID = 1536
SHAPES = [(3, 5, 7), (1, 9, 16), (5, 12, 20), (2, 45, 80)]      # (T, H, W)
GOLDEN_SHAPES = [(3, 5, 7), (5, 12, 20)]
WGRAD_SPLIT_SHAPES = [(20, 27, 27), (9, 45, 80)]                  # weight gradient only: cps = 2 and cps = 3 (docstring)
H0_NONZERO = {(5, 12, 20), (2, 45, 80), (20, 27, 27), (9, 45, 80)}
SEED = {(3, 5, 7): 101, (1, 9, 16): 102, (5, 12, 20): 103, (2, 45, 80): 104, (20, 27, 27): 105, (9, 45, 80): 106}
WGRAD_CHAIN, WGRAD_KSTEP, WGRAD_TILES, WGRAD_TARGET_WGS = 1024, 32, 72, 1024      # csrc/train.hip, restated
WGRAD_WRONG = ("last_share", "chain_twice", "tail_step", "frame0_h0")
DW_SUBSET = (slice(None, None, 5), slice(None, None, 7))          # the strided part of dW the goldens keep: [52, 74, 3, 3]


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def name(shape):
    return "train_T%d_%dx%d" % shape


# ------------------------------------------------------------------------------------------------ inputs (float32 numpy)
def twa_inputs(shape, seed=None):
    """`x [T,256,H,W]`, `h0 [1,256,H,W]` (zeros unless the shape is in H0_NONZERO), `w [256,512,3,3]` kaiming fan_out
    (std sqrt(2 / (256 * 9)): pre-activations of std ~2, gates spread over (0, 1)), `gy [T,1,H,W]` the gradient that
    arrives at the prediction."""
    T, H, W = shape
    rs = np.random.RandomState(SEED[shape] if seed is None else seed)
    x = rs.standard_normal((T, C, H, W)).astype(np.float32)
    h0 = (0.5 * rs.standard_normal((1, C, H, W))).astype(np.float32)
    if shape not in H0_NONZERO:
        h0[:] = 0
    w = (rs.standard_normal((C, 2 * C, 3, 3)) * math.sqrt(2.0 / (C * 9))).astype(np.float32)
    gy = (rs.standard_normal((T, 1, H, W)) / (H * W)).astype(np.float32)
    return {"x": x, "h0": h0, "w": w, "gy": gy}


def teacher_inputs(shape, seed_off=1000):
    """Inputs of the teacher-forced kernel tests: independent random `G`, `carry`, `z`, `hist` (the history h_0..h_{T-1}), `dz`."""
    T, H, W = shape
    rs = np.random.RandomState(SEED[shape] + seed_off)
    mk = lambda s, *sh: (s * rs.standard_normal(sh)).astype(np.float32)      # noqa: E731
    return {"G": mk(1e-2, T, C, H, W), "carry": mk(1e-2, 1, C, H, W), "z": mk(2.0, T, C, H, W), "hist": mk(1.0, T, C, H, W),
            "dz": mk(1e-2, T, C, H, W)}


def decoder_params(h, seed):
    """The decoder of the tests for the history `h` [T,256,H,W] (uniform in [0, 3) in the teacher-forced tests): kaiming
    fan_out weights, and folded BatchNorms chosen on THIS data so that the pre-activations of both ReLU6s have std 3 and
    mean 1.5 + N(0, 1) per channel -- both clamps of both then hold a sizeable share of the elements (asserted by the
    tests) -- and the logits std 1.5, mean 0.  Returns float32 numpy arrays: w1 [1536,256,1,1], s1, b1, wd [1536,1,3,3],
    s2, b2, w3 [1,1536,1,1], s3 [1], b3 [1]."""
    rs = np.random.RandomState(seed)
    hh = torch.as_tensor(h, dtype=torch.float64)
    p = {}
    p["w1"] = (rs.standard_normal((HID, C, 1, 1)) * math.sqrt(2.0 / HID)).astype(np.float32)
    p["wd"] = (rs.standard_normal((HID, 1, 3, 3)) * math.sqrt(2.0 / (HID * 9))).astype(np.float32)
    p["w3"] = (rs.standard_normal((1, HID, 1, 1)) * math.sqrt(2.0)).astype(np.float32)
    m1, m2 = rs.standard_normal(HID), rs.standard_normal(HID)

    def norm(pre, m):
        sd, mu = pre.std((0, 2, 3)), pre.mean((0, 2, 3))
        s = 3.0 / sd
        b = (1.5 + torch.as_tensor(m)) - mu * s
        return s.float(), b.float()
    pre = F.conv2d(hh, torch.as_tensor(p["w1"]).double())
    s1, b1 = norm(pre, m1)
    e = (pre * s1.double().view(1, -1, 1, 1) + b1.double().view(1, -1, 1, 1)).clamp(0, 6)
    pre = F.conv2d(e, torch.as_tensor(p["wd"]).double(), padding=1, groups=HID)
    s2, b2 = norm(pre, m2)
    d = (pre * s2.double().view(1, -1, 1, 1) + b2.double().view(1, -1, 1, 1)).clamp(0, 6)
    lg = F.conv2d(d, torch.as_tensor(p["w3"]).double())
    s3 = (1.5 / lg.std()).float().reshape(1)
    b3 = (-lg.mean() * s3.double()).float().reshape(1)
    for k, v in (("s1", s1), ("b1", b1), ("s2", s2), ("b2", b2), ("s3", s3), ("b3", b3)):
        p[k] = v.numpy()
    return p


def load_block(block, p):
    """Put `decoder_params` into a dwBlock(256, 1) (the package's or the reference's: same layout) in eval mode: conv weights
    as they are, BatchNorms with running mean 0, eps 2^-20 and variance 1 - 2^-20 (their sum is exactly 1 in float32 and
    float64), so that the eval fold is exactly (s, b)."""
    seq = block.conv
    with torch.no_grad():
        for conv, wkey in ((seq[0][0], "w1"), (seq[1][0], "wd"), (seq[2], "w3")):
            conv.weight.copy_(torch.as_tensor(p[wkey]))
        for bn, s, b in ((seq[0][1], "s1", "b1"), (seq[1][1], "s2", "b2"), (seq[3], "s3", "b3")):
            bn.weight.copy_(torch.as_tensor(p[s]))
            bn.bias.copy_(torch.as_tensor(p[b]))
            bn.running_mean.zero_()
            bn.eps = 2.0 ** -20
            bn.running_var.fill_(1.0 - 2.0 ** -20)
    return block.eval()


# Seed offsets of the decoder tests' inputs, one per shape.  They are CHOSEN: the end-to-end decoder test needs inputs whose
# undecided term (decoder_e2e) stays below 6 % of ||grad_h||_2 in every frame, so that its widened bound cannot hide a
# structural error.  Over seeds 0..5 of this recipe the largest per-frame ratio of a shape lies between 4.9 % and 8.2 %
# (the smallest map has 35 pixels per frame and scatters most); these give 4.9 %, 5.0 %, 5.6 % and 5.7 %.  The CPU test asserts
# the condition on the float64 reference alone.
DEC_SEED = {(3, 5, 7): 5, (1, 9, 16): 1, (5, 12, 20): 2, (2, 45, 80): 0}


def decoder_inputs(shape):
    """`(h [T,256,H,W] uniform in [0, 3), decoder_params for it, gy [T,1,H,W])` of the decoder tests (float32 numpy)."""
    so = DEC_SEED[shape]
    h = uniform_history(shape, 2000 + so)
    return h, decoder_params(h, SEED[shape] + 11 + so), twa_inputs(shape)["gy"]


def uniform_history(shape, seed_off=2000):
    T, H, W = shape
    return (3.0 * np.random.RandomState(SEED[shape] + seed_off).random_sample((T, C, H, W))).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the recurrence
def twa_forward(x, h0, w):
    """`(h_seq [T,256,H,W], z [T,256,H,W])` of one sequence (model_convlstm.py:276-292, 368-371)."""
    h, hs, zs = h0, [], []
    for t in range(x.shape[0]):
        z = F.conv2d(torch.cat([x[t:t + 1], h], 1), w, padding=1)
        i = torch.sigmoid(z)
        h = i * x[t:t + 1] + (1 - i) * h
        hs.append(h)
        zs.append(z)
    return torch.cat(hs, 0), torch.cat(zs, 0)


def twa_bptt(x, h0, w, grad_h):
    """torch autograd through `twa_forward`: `(dW, grad_x, grad_h0)` for the direct gradients `grad_h` of every h_t."""
    x, h0, w = (t.detach().clone().requires_grad_(True) for t in (x, h0, w))
    h_seq, _ = twa_forward(x, h0, w)
    gw, gx, g0 = torch.autograd.grad(h_seq, (w, x, h0), grad_h)
    return gw, gx, g0


def gate_ref(G, carry, z, x, hprev):
    """uavsal_twa_gate_bwd: `{name: (y, E)}` for dz, carry, dx."""
    ca = torch.zeros_like(G) if carry is None else carry
    g = G + ca
    i = torch.sigmoid(z)
    om = torch.sigmoid(-z)
    ga = G.abs() + ca.abs()
    dz = g * (x - hprev) * i * om
    co, dx = g * om, g * i
    return {"dz": (dz, ((ga * (x - hprev).abs() + g.abs() * (x.abs() + hprev.abs())) * i * om + 11 * dz.abs()) / 8),
            "carry": (co, (ga * om + 6 * co.abs()) / 8),
            "dx": (dx, (ga * i + 6 * dx.abs()) / 8)}


def wgrad_inputs(shape):
    """The weight-gradient tests' operands (float32 numpy): `dz`, `hist` of `teacher_inputs`, `x` of `twa_inputs`, and `h0` =
    100 * `carry` (N(0, 1)) for the shapes in H0_NONZERO, zeros otherwise."""
    t = teacher_inputs(shape)
    h0 = np.float32(100.0) * t["carry"] if shape in H0_NONZERO else np.zeros_like(t["carry"])
    return {"dz": t["dz"], "x": twa_inputs(shape)["x"], "hist": t["hist"], "h0": h0}


def _wgrad_cat(x, hist, h0):
    return torch.cat([x, torch.cat([h0, hist[:x.shape[0] - 1]], 0)], 1)


def _wgrad_sum(a, b):
    """sum over frames t and pixels p of a[t, co, p] * unfold3x3(b)[t, (ci, ky, kx), p] -> [co, ci, 3, 3]; a frame at a time, so
    that only one frame's columns exist at once"""
    T, co, H, W = a.shape
    out = a.new_zeros((co, b.shape[1] * 9))
    for t in range(T):
        out += a[t].reshape(co, H * W) @ F.unfold(b[t:t + 1], 3, padding=1)[0].T       # rows (ci, ky, kx)
    return out.reshape(co, b.shape[1], 3, 3)


def wgrad_ref(dz, x, hist, h0):
    """uavsal_twa_wgrad: `(dW [co,512,3,3], bound)`; frame t pairs dz_t with cat[x_t, h_{t-1}], h_{-1} = h0.  `dz` may hold
    a slice of the 256 output channels."""
    T, _, H, W = dz.shape
    cat = _wgrad_cat(x, hist, h0)
    return _wgrad_sum(dz, cat), LAMBDA * U * math.sqrt(T * H * W) * _wgrad_sum(dz.abs(), cat.abs())


def wgrad_partition(T, H, W):
    """The K split of uavsal_twa_wgrad, restated: `(cps, shares, [(p0, p1) per share])`.  The K = T H W pixels are cut into
    chunks of 1024; with 72 tiles and a grid of about 1024 workgroups at most 14 workgroups share a tile; every share is the
    same whole number `cps` of chunks, the smallest with which 14 shares cover all chunks, and the last share takes what is left."""
    K = T * H * W
    chunks = -(-K // WGRAD_CHAIN)
    most = min(WGRAD_TARGET_WGS // WGRAD_TILES, chunks)
    cps = next(c for c in range(1, chunks + 1) if c * most >= chunks)
    span = cps * WGRAD_CHAIN
    spans = [(p, min(p + span, K)) for p in range(0, K, span)]
    return cps, len(spans), spans


def wgrad_wrong_weights(T, H, W):
    """How often three wrong kernels count each of the K pixels (`{name: float64 numpy [K]}`, 1 = right):
    last_share   the last share's pixels are left out (a grid one share short, or a short last share dropped);
    chain_twice  the first chunk of every share of more than one chunk counts twice: `acc` not cleared at the first chain end,
                 so the second chain's tile still holds the first when it is added to `tot`;
    tail_step    the pixels of the final, partial 32-pixel K step are left out (steps rounded down)."""
    _, _, spans = wgrad_partition(T, H, W)
    K = T * H * W
    w = {k: np.ones(K) for k in WGRAD_WRONG[:3]}
    p0, p1 = spans[-1]
    w["last_share"][p0:p1] = 0
    for a, b in spans:
        if b - a > WGRAD_CHAIN:
            w["chain_twice"][a:a + WGRAD_CHAIN] = 2
    w["tail_step"][p0 + (p1 - p0 - 1) // WGRAD_KSTEP * WGRAD_KSTEP:p1] = 0
    return w


def wgrad_wrong_refs(dz, x, hist, h0):
    """`{name: dW}` of the four wrong kernels of WGRAD_WRONG in float64: the three of `wgrad_wrong_weights` by weighting dz per
    pixel (one pass over the unfolded columns for all three), and frame0_h0, frame 0 paired with zeros instead of h0: the
    right sum less frame 0's terms in the history half of the input channels."""
    T, co, H, W = dz.shape
    cat = _wgrad_cat(x, hist, h0)
    wg = wgrad_wrong_weights(T, H, W)
    names = WGRAD_WRONG[:3]
    scaled = [dz * torch.as_tensor(wg[k]).to(dz).view(T, 1, H, W) for k in names]
    right, *wrong = _wgrad_sum(torch.cat([dz] + scaled, 1), cat).split(co, 0)
    out = dict(zip(names, wrong))
    f0 = right.clone()
    f0[:, C:] -= _wgrad_sum(dz[:1], h0)
    out["frame0_h0"] = f0
    return out


def input_grad_ref(dz, w_slice, res=None):
    """The transposed conv that carries dz back to one half of the cell's input, + res: `(y, bound)`."""
    y = F.conv_transpose2d(dz, w_slice, padding=1)
    B = F.conv_transpose2d(dz.abs(), w_slice.abs(), padding=1)
    E = y.abs()
    if res is not None:
        y, B, E = y + res, B + res.abs(), E + res.abs()
    return y, rtol("f32", 9 * C) * B + EPS * (E + y.abs())


# ------------------------------------------------------------------------------------------------ the decoder
def _v(t):
    return t.view(1, -1, 1, 1)


def decoder_forward(p, h):
    """`p`: decoder_params as float64 tensors.  Returns dict(e_pre, e, d_pre, d, logit, y)."""
    e_pre = F.conv2d(h, p["w1"]) * _v(p["s1"]) + _v(p["b1"])
    e = e_pre.clamp(0, 6)
    d_pre = F.conv2d(e, p["wd"], padding=1, groups=HID) * _v(p["s2"]) + _v(p["b2"])
    d = d_pre.clamp(0, 6)
    logit = F.conv2d(d, p["w3"]) * p["s3"] + p["b3"]
    return {"e_pre": e_pre, "e": e, "d_pre": d_pre, "d": d, "logit": logit, "y": torch.sigmoid(logit)}


def dec_bwd_ref(p, gy, y, e, d, absolute=False):
    """uavsal_dec_bwd from the stored e, d, y: `ge [T,1536,H,W]`; `absolute`: the same chain on absolute values."""
    a = lambda t: t.abs() if absolute else t                              # noqa: E731
    pix = a(gy) * y * (1 - y) * a(p["s3"])
    t = pix * _v(a(p["w3"]).reshape(-1)) * ((d > 0) & (d < 6))
    back = F.conv_transpose2d(t, a(p["wd"]), padding=1, groups=HID)
    return back * _v(a(p["s2"])) * _v(a(p["s1"])) * ((e > 0) & (e < 6))


def dec_bwd_bound(p, gy, y, e, d):
    return (LAMBDA * 3 + 8) * U * dec_bwd_ref(p, gy, y, e, d, absolute=True)


def decoder_grad_autograd(p, h, gy):
    """torch autograd through `decoder_forward`: d sum(gy * y) / d h."""
    h = h.detach().clone().requires_grad_(True)
    y = decoder_forward(p, h)["y"]
    return torch.autograd.grad(y, h, gy)[0]


def decoder_e2e(p, h, gy):
    """The decoder's input gradient when the DEVICE recomputes e, d and y: `(grad_h, bound, undecided, f)`.
    `bound` is the regular per-element bound: the dec_bwd bound carried through |W1| plus the 1536 -> 256 GEMM's own.  The
    prediction y is HANDED to the device (float64 y rounded to fp32, as `recurrence_step` hands over the forward's): an
    error of y would enter through y (1 - y) at every channel of a pixel at once, and the absolute-value chain through the
    1536 channels of |W1| overstates such a coherent term by their cancellation (about sqrt(1536)).  `undecided` is the absolute contribution of every e and d element whose
    float64 pre-activation lies within its forward bound (plan_ref64's chain rule) of a clamp: its mask may legitimately
    differ on the device, which removes or adds the element's whole term."""
    f = decoder_forward(p, h)
    w1a = p["w1"].abs()
    habs = h.abs()
    be_pre = F.conv2d(habs, w1a) * _v(p["s1"].abs()) + _v(p["b1"].abs())
    err_e = rtol("f32", C) * be_pre + EPS * 2 * f["e_pre"].abs()                     # E = 2 |y| (plan_ref64.ref_conv)
    bd_pre = F.conv2d(be_pre, p["wd"].abs(), padding=1, groups=HID) * _v(p["s2"].abs()) + _v(p["b2"].abs())
    rt_d = rtol("f32", C) + rtol("f32", 9)
    err_d = rt_d * bd_pre + EPS * 2 * f["d_pre"].abs()
    near = lambda pre, err: ((pre.abs() <= err) | ((pre - 6).abs() <= err)).double()      # noqa: E731
    ue, ud = near(f["e_pre"], err_e), near(f["d_pre"], err_d)
    y, e, d = f["y"], f["e"], f["d"]
    ge = dec_bwd_ref(p, gy, y, e, d)
    grad_h = F.conv_transpose2d(ge, p["w1"])
    # regular bound
    ge_abs = dec_bwd_ref(p, gy, y, e, d, absolute=True)
    bound = ((LAMBDA * 3 + 8) * U + rtol("f32", HID)) * F.conv_transpose2d(ge_abs, w1a)
    bound = bound + EPS * grad_h.abs()
    # undecided masks: the terms as they would be WITHOUT the mask in question
    pix = gy.abs() * y * (1 - y) * p["s3"].abs()
    t_all = pix * _v(p["w3"].abs().reshape(-1))
    s12 = _v(p["s2"].abs() * p["s1"].abs())
    from_d = F.conv_transpose2d(t_all * ud, p["wd"].abs(), padding=1, groups=HID) * s12 * ((e > 0) & (e < 6))
    t_sgn = gy * y * (1 - y) * p["s3"] * _v(p["w3"].reshape(-1)) * ((d > 0) & (d < 6))
    from_e = (F.conv_transpose2d(t_sgn, p["wd"], padding=1, groups=HID) * s12).abs() * ue      # |ge| as it is without e's mask
    undecided = F.conv_transpose2d(from_d + from_e, w1a)
    f.update(ue=ue, ud=ud)
    return grad_h, bound, undecided, f


def clamp_shares(pre):
    """(share of elements at or below 0, share at or above 6) of a ReLU6's pre-activation."""
    return float((pre <= 0).double().mean()), float((pre >= 6).double().mean())


def l2_per_frame(t):
    return t.flatten(1).norm(dim=1)


def to64(d, device="cpu"):
    return {k: torch.as_tensor(v).to(device=device, dtype=torch.float64) for k, v in d.items()}
