"""Float64 restatement of the ConvLSTM slice of train/recurrence.py -- the cell of reference model_convlstm.py:111-126 (bias = False, one
layer), back-propagation through time as `train.lstm_backward` walks it, the two kernels of csrc/train_lstm.hip -- written with
torch's own operators, the seeded inputs of the tests, and per-element bounds in the convention of tests/plan_ref64.py:

    |kernel - y| <= rtol * B + EPS * E                  U = 2^-24, LAMBDA = 8, EPS = 8 U (from there)

The two element-wise kernels are EPS * E with E the roundings counted one by one, in units of U / 8 (train_ref64's way for
uavsal_twa_gate_bwd).  expf and expm1f are 1 ulp = 2 U, every sum, product and quotient is one rounding = 1 U, all relative:

  e = expf(-|z|)                       2 U
  d = 1 + e                            2 U   (e <= 1: its 2 U weigh at most 1 U of d, plus the sum's rounding)
  s = 1 / d  or  e / d                 5 U   (3 U and 2 + 2 + 1 = 5 U; the larger is taken for both branches)
  s (1 - s) = e / (d d)                8 U   (d d: 2 + 2 + 1; the quotient 2 + 5 + 1)
  1 - tanh^2 = 4 e2 / (d2 d2)          8 U   (the same with e2 = expf(-2|z|); the 2 and the 4 are exact)
  m = expm1f(-2|z|), 2 + m             3 U   (|m| <= 1 <= 2 + m: m's 2 U weigh at most 2 U, plus the sum's rounding)
  tanh = -m / (2 + m)                  6 U   (2 + 3 + 1)

  uavsal_lstm_scan, step t:  c_t = f c_{t-1} + i g.  f c_{t-1}: 5 + 1 = 6 U; i g: 5 + 6 + 1 = 12 U; the sum 1 U of |c_t|; and the
  error c_{t-1} already carries arrives multiplied by f:
      err_t <= f err_{t-1} + U (6 f |c_{t-1}| + 12 i |g| + |c_t|)                  (SCAN_SLACK = 1 U |c_t| more for the second order)
  carried along t from err_{-1} = 0 (c0 is an input).  Contraction to an fma only removes a rounding.

  uavsal_lstm_gate_bwd:  gh = G + carry_h is one rounding, relative to ga = |G| + |carry_h|.  a = gh o q_c (q_c = 1 - tanh^2(c_t)):
  gh's 1 U of ga o q_c, then 5 + 8 + 2 = 15 U of |a| <= ga o q_c: 16 U ga o q_c.  dc = carry_c + a: 1 U of |dc| <= |carry_c| + ga o q_c:
      err(dc) <= U eD,   eD = |carry_c| + 17 ga o q_c
      dcc_i = dc g s_i'      U (eD |g| s_i' + (6 + 8 + 2) |dcc_i|)
      dcc_f = dc c_{t-1} s_f'     U (eD |c_{t-1}| s_f' + (8 + 2) |dcc_f|)         (c_{t-1} is an input)
      dcc_o = gh tc s_o'     U (ga |tc| s_o' + (6 + 8 + 2) |dcc_o|)
      dcc_g = dc i q_g       U (eD i q_g + (5 + 8 + 2) |dcc_g|)
      carry_c' = dc f        U (eD f + (5 + 1) |carry_c'|)
  and one more U of |y| on each for the second-order terms (the factors' relative errors multiply: (1 + 17 U)(1 + 16 U) - 1 -
  33 U < 2^-40).  Without carries every term is a pure product and the bound is RELATIVE to |y|: at most GATE_REL_MAX = 34 U |y|,
  the claim the saturated-gate test checks at |cc| in 10 .. 30, where s (1 - s) is down to 1e-13 and 1 - tanh^2 to 1e-26.

  The three convs as `lstm_backward` launches them and the weight gradient take the forms of train_ref64:
      cc = conv(W_x, x), then conv(W_h, h_prev) + res       plan_ref64.rtol("f32", 9 * 256), B = the conv on absolute values (+ |res|)
      carry_h = conv(flip(W_h)^T, dcc_t), grad_x likewise   plan_ref64.rtol("f32", 9 * 1024), the same B
      dW (uavsal_conv3_wgrad at Co = 1024, Ci = 512)        LAMBDA U sqrt(T H W) sum |dcc| |cat|
  each + EPS (E + |y|) as train_ref64.input_grad_ref has it.

The weight gradient's K split (pixgemm::split over 8 * 9 * 4 = 288 tiles, chunks of 1024 pixels, about 1024 workgroups: at most
3 shares per tile) is real at two of SHAPES: (5,12,20) K = 1200: 2 shares, the second 176 pixels; (2,45,80) K = 7200: cps = 3,
3 shares, the last one 1024 + 32 pixels.  `wgrad_partition` restates it (the CPU test holds it against the library's own
`uavsal_conv3_wgrad_shares`).

WRONG: seven plausible bad walks, computed here in float64; the CPU test holds each at least 4 bounds from the right result, the
GPU test passes the device against the right reference and fails it against each wrong one:
  carry_c_dropped  dc without carry_c            c_t_in_dcc_f   c_t where c_{t-1} belongs in dcc_f
  step0_zero_c     step 0 paired with zeros instead of c0        h_t_not_prev   frame t's weight gradient reads h_t, not h_{t-1}
  gate_order_ifgo  gate rows read as i, f, g, o  last_share     the last K share of the weight gradient left out
  carry_h_T2       carry_h not added at step T - 2

Every function takes and returns float64 NCHW tensors on the device of its inputs."""
import hashlib
import math

import numpy as np
import torch
import torch.nn.functional as F

from plan_ref64 import EPS, LAMBDA, U, rtol

C = 256
SHAPES = [(3, 5, 7), (1, 9, 16), (5, 12, 20), (2, 45, 80)]      # (T, H, W)
GOLDEN_SHAPES = [(3, 5, 7), (5, 12, 20)]
STATE_NONZERO = {(1, 9, 16), (5, 12, 20), (2, 45, 80)}           # h0 and c0 given; (3,5,7) passes None for both
SEED = {(3, 5, 7): 301, (1, 9, 16): 302, (5, 12, 20): 303, (2, 45, 80): 304}
DW_SUBSET = (slice(None, None, 11), slice(None, None, 13))        # the strided part of dW the goldens keep: [94, 40, 3, 3]
WGRAD_CHAIN, WGRAD_TILES, WGRAD_TARGET_WGS = 1024, 288, 1024      # csrc/pix_gemm_tile.h at Co = 1024, Ci = 512, restated
WRONG = ("carry_c_dropped", "c_t_in_dcc_f", "step0_zero_c", "h_t_not_prev", "gate_order_ifgo", "last_share", "carry_h_T2")
CC_STD = 4.0                                                      # teacher-forced pre-activations: P(|N(0, 16)| > 8) = 4.6 %
GATE_REL_MAX = 34
SCAN_SLACK = 1


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def name(shape):
    return "lstm_train_T%d_%dx%d" % shape


def to64(d, device="cpu"):
    return {k: torch.as_tensor(v).to(device=device, dtype=torch.float64) for k, v in d.items()}


# ------------------------------------------------------------------------------------------------ inputs (float32 numpy)
def lstm_inputs(shape):
    """The free-running inputs: `x [T,256,H,W]` N(0, 1), `h0`, `c0` `[1,256,H,W]` (zeros unless the shape is in STATE_NONZERO),
    `w [1024,512,3,3]` of std sqrt(2 / (256 * 9)) (pre-activations of std ~2: gates spread over (0, 1), some saturated), `G
    [T,256,H,W]` the direct gradient of every h_t."""
    T, H, W = shape
    rs = np.random.RandomState(SEED[shape])
    x = rs.standard_normal((T, C, H, W)).astype(np.float32)
    h0 = np.tanh(rs.standard_normal((1, C, H, W))).astype(np.float32)
    c0 = rs.standard_normal((1, C, H, W)).astype(np.float32)
    if shape not in STATE_NONZERO:
        h0[:], c0[:] = 0, 0
    w = (rs.standard_normal((4 * C, 2 * C, 3, 3)) * math.sqrt(2.0 / (C * 9))).astype(np.float32)
    G = (rs.standard_normal((T, C, H, W)) / (H * W)).astype(np.float32)
    return {"x": x, "h0": h0, "c0": c0, "w": w, "G": G}


def teacher_inputs(shape, seed_off=1000):
    """Inputs of the teacher-forced kernel tests, independent of each other: `cc [T,1024,H,W]` N(0, CC_STD^2) (saturated gates
    present, not dominant: the share of |cc| > 8 is checked on the CPU), `c0`, `G`, `carry_h`, `carry_c`, `hist` (a history
    h_0 .. h_{T-1} in (-1, 1)), `dcc [T,1024,H,W]`."""
    T, H, W = shape
    rs = np.random.RandomState(SEED[shape] + seed_off)
    mk = lambda s, *sh: (s * rs.standard_normal(sh)).astype(np.float32)      # noqa: E731
    t = {"cc": mk(CC_STD, T, 4 * C, H, W), "c0": mk(1.0, 1, C, H, W), "G": mk(1e-2, T, C, H, W), "carry_h": mk(1e-2, 1, C, H, W),
         "carry_c": mk(1e-2, 1, C, H, W), "hist": np.tanh(mk(1.0, T, C, H, W)), "dcc": mk(1e-2, T, 4 * C, H, W)}
    if shape not in STATE_NONZERO:
        t["c0"][:] = 0
    return t


def saturated_inputs(shape=(3, 5, 7), seed_off=2000):
    """Pre-activations of magnitude 10 .. 30 with random signs (every gate saturated: s (1 - s) between 5e-5 and 1e-13, 1 - g^2
    between 8e-9 and 4e-26), cell states N(0, 1.5^2), a gradient of order 1, no carries."""
    T, H, W = shape
    rs = np.random.RandomState(SEED[shape] + seed_off)
    mag = lambda *sh: ((10.0 + 20.0 * rs.random_sample(sh)) * rs.choice([-1.0, 1.0], sh)).astype(np.float32)      # noqa: E731
    nrm = lambda s, *sh: (s * rs.standard_normal(sh)).astype(np.float32)                                          # noqa: E731
    return {"cc": mag(1, 4 * C, H, W), "c": nrm(1.5, 1, C, H, W), "c_prev": nrm(1.5, 1, C, H, W), "G": nrm(1.0, 1, C, H, W)}


# fp32 underflow under the relative claim of the saturated test: a product below the smallest normal 2^-126 may be flushed or
# lose its low bits; what follows it multiplies by at most 2^5 (|c_{t-1}| s (1 - s) and the like)
SAT_FLOOR = 2.0 ** -121


# ------------------------------------------------------------------------------------------------ element-wise pieces
def _sg(z):
    """(s, 1 - s, s (1 - s)) of sigmoid(z), each to float64's relative accuracy in a saturated gate"""
    s, om = torch.sigmoid(z), torch.sigmoid(-z)
    return s, om, s * om


def _q(z):
    """1 - tanh(z)^2 = 4 e2 / (1 + e2)^2, e2 = exp(-2|z|): accurate where 1 - tanh^2 itself cancels"""
    e2 = torch.exp(-2 * z.abs())
    return 4 * e2 / (1 + e2) ** 2


def split(cc, order="ifog"):
    """the four gate slabs of `cc` [n,4C,H,W] as a dict by gate letter, rows `order`"""
    return dict(zip(order, cc.split(cc.shape[1] // 4, 1)))


def scan_ref(cc, c0):
    """uavsal_lstm_scan: `(c_seq [T,C,H,W], bound)`, the bound carried along t (docstring)."""
    z = split(cc)
    i, f, g = torch.sigmoid(z["i"]), torch.sigmoid(z["f"]), torch.tanh(z["g"])
    c, err = c0[0], torch.zeros_like(c0[0])
    cs, bs = [], []
    for t in range(cc.shape[0]):
        new = f[t] * c + i[t] * g[t]
        err = f[t] * err + U * (6 * f[t] * c.abs() + 12 * i[t] * g[t].abs() + (1 + SCAN_SLACK) * new.abs())
        c = new
        cs.append(c)
        bs.append(err)
    return torch.stack(cs), torch.stack(bs)


def gate_ref(G, carry_h, carry_c, cc, c, c_prev, variant=None):
    """uavsal_lstm_gate_bwd: `{name: (y, E)}` for dcc ([n,4C,H,W], rows i, f, o, g) and carry_c; the bound is EPS * E.
    `variant`: one of the element-wise entries of WRONG."""
    ch = torch.zeros_like(G) if carry_h is None else carry_h
    ccar = torch.zeros_like(G) if carry_c is None or variant == "carry_c_dropped" else carry_c
    z = split(cc, "ifgo" if variant == "gate_order_ifgo" else "ifog")
    (i, _, spi), (f, _, spf), (o, _, spo) = _sg(z["i"]), _sg(z["f"]), _sg(z["o"])
    g, qg, tc, qc = torch.tanh(z["g"]), _q(z["g"]), torch.tanh(c), _q(c)
    cp = c if variant == "c_t_in_dcc_f" else c_prev
    gh, ga = G + ch, G.abs() + ch.abs()
    dc = ccar + gh * o * qc
    eD = ccar.abs() + 17 * ga * o * qc
    di, df, do, dg, co = dc * g * spi, dc * cp * spf, gh * tc * spo, dc * i * qg, dc * f
    Ei = eD * g.abs() * spi + 17 * di.abs()
    Ef = eD * cp.abs() * spf + 11 * df.abs()
    Eo = ga * tc.abs() * spo + 17 * do.abs()
    Eg = eD * i * qg + 16 * dg.abs()
    Ec = eD * f + 7 * co.abs()
    return {"dcc": (torch.cat([di, df, do, dg], 1), torch.cat([Ei, Ef, Eo, Eg], 1) / 8), "carry_c": (co, Ec / 8)}


# ------------------------------------------------------------------------------------------------ convs, weight gradient
def conv_ref(a, w, res=None, k=9 * C):
    """conv3x3(w, a) + res: `(y, bound)` in train_ref64.input_grad_ref's form, k products per element."""
    y = F.conv2d(a, w, padding=1)
    B = F.conv2d(a.abs(), w.abs(), padding=1)
    E = y.abs()
    if res is not None:
        y, B, E = y + res, B + res.abs(), E + res.abs()
    return y, rtol("f32", k) * B + EPS * (E + y.abs())


def conv_t_ref(d, w_slice):
    """conv3x3(flip(w_slice)^T, d), 1024 -> 256: `(y, bound)`."""
    y = F.conv_transpose2d(d, w_slice, padding=1)
    B = F.conv_transpose2d(d.abs(), w_slice.abs(), padding=1)
    return y, rtol("f32", 9 * 4 * C) * B + EPS * 2 * y.abs()


def _wgrad_sum(a, b):
    """sum over frames and pixels of a[t, co, p] * unfold3x3(b)[t, (ci, ky, kx), p] -> [co, ci, 3, 3], a frame at a time"""
    T, co, H, W = a.shape
    out = a.new_zeros((co, b.shape[1] * 9))
    for t in range(T):
        out += a[t].reshape(co, H * W) @ F.unfold(b[t:t + 1], 3, padding=1)[0].T
    return out.reshape(co, b.shape[1], 3, 3)


def hprev_of(hist, h0):
    return torch.cat([h0, hist[:hist.shape[0] - 1]], 0)


def wgrad_partition(T, H, W):
    """The K split of uavsal_conv3_wgrad at Co = 1024, Ci = 512, restated: `(cps, shares, [(p0, p1) per share])`."""
    K = T * H * W
    chunks = -(-K // WGRAD_CHAIN)
    most = max(1, min(WGRAD_TARGET_WGS // WGRAD_TILES, chunks))
    cps = -(-chunks // most)
    span = cps * WGRAD_CHAIN
    spans = [(p, min(p + span, K)) for p in range(0, K, span)]
    return cps, len(spans), spans


def wgrad_ref(dcc, x, hist, h0, variant=None):
    """The weight gradient: `(dW [1024,512,3,3], bound)`; frame t pairs dcc_t with cat[x_t, h_{t-1}], h_{-1} = h0.  `variant`:
    "h_t_not_prev" or "last_share" of WRONG (the bound stays the right one's)."""
    T, _, H, W = dcc.shape
    cat = torch.cat([x, hprev_of(hist, h0)], 1)
    bound = LAMBDA * U * math.sqrt(T * H * W) * _wgrad_sum(dcc.abs(), cat.abs())
    if variant == "h_t_not_prev":
        cat = torch.cat([x, hist], 1)
    if variant == "last_share":
        keep = torch.ones(T * H * W, dtype=dcc.dtype, device=dcc.device)
        keep[wgrad_partition(T, H, W)[2][-1][0]:] = 0
        dcc = dcc * keep.view(T, 1, H, W)
    return _wgrad_sum(dcc, cat), bound


# ------------------------------------------------------------------------------------------------ the recurrence
def lstm_forward(x, h0, c0, w):
    """`(h_seq, c_seq, cc)` of one sequence (model_convlstm.py:111-126, 206-222)."""
    h, c, hs, cs, ccs = h0, c0, [], [], []
    for t in range(x.shape[0]):
        cc = F.conv2d(torch.cat([x[t:t + 1], h], 1), w, padding=1)
        z = split(cc)
        c = torch.sigmoid(z["f"]) * c + torch.sigmoid(z["i"]) * torch.tanh(z["g"])
        h = torch.sigmoid(z["o"]) * torch.tanh(c)
        hs.append(h)
        cs.append(c)
        ccs.append(cc)
    return torch.cat(hs, 0), torch.cat(cs, 0), torch.cat(ccs, 0)


def lstm_bptt(x, h0, c0, w, grad_h):
    """torch autograd through `lstm_forward`: `(dW, grad_x, grad_h0, grad_c0)` for the direct gradients `grad_h` of every h_t."""
    x, h0, c0, w = (t.detach().clone().requires_grad_(True) for t in (x, h0, c0, w))
    h_seq, _, _ = lstm_forward(x, h0, c0, w)
    return torch.autograd.grad(h_seq, (w, x, h0, c0), grad_h)


def lstm_walk(x, hist, h0, c0, w, grad_h, variant=None, bounds=True):
    """`train.lstm_backward` restated, from the KNOWN history `hist`: cc and c are recomputed, the carry runs step by step.
    Returns a dict: dW, grad_x, grad_h0, grad_c0, cc, c_seq, dcc, and `bounds` = the bounds of the final sums (dW, grad_x,
    grad_h0 by their own launch; grad_c0 by the last gate step; `bounds=False`: left out, and dW only).  `variant`: any entry
    of WRONG."""
    T = x.shape[0]
    hp = hprev_of(hist, h0)
    cc = F.conv2d(torch.cat([x, hp], 1), w, padding=1)
    cs, _ = scan_ref(cc, torch.zeros_like(c0) if variant == "step0_zero_c" else c0)
    cprev = torch.cat([torch.zeros_like(c0) if variant == "step0_zero_c" else c0, cs[:T - 1]], 0)
    ch, ccar, dccs = None, None, [None] * T
    ev = variant if variant in ("carry_c_dropped", "c_t_in_dcc_f", "gate_order_ifgo") else None
    wh, wx = w[:, C:], w[:, :C]
    for t in range(T - 1, -1, -1):
        skip = variant == "carry_h_T2" and t == T - 2
        r = gate_ref(grad_h[t:t + 1], None if skip else ch, ccar, cc[t:t + 1], cs[t:t + 1], cprev[t:t + 1], ev)
        dccs[t], (ccar, ec) = r["dcc"][0], r["carry_c"]
        ch, hb = conv_t_ref(dccs[t], wh) if bounds else (F.conv_transpose2d(dccs[t], wh, padding=1), None)
    dcc = torch.cat(dccs, 0)
    if not bounds:
        cat = torch.cat([x, hist if variant == "h_t_not_prev" else hp], 1)
        if variant == "last_share":
            keep = torch.ones(dcc.shape[0] * dcc.shape[2] * dcc.shape[3], dtype=dcc.dtype, device=dcc.device)
            keep[wgrad_partition(dcc.shape[0], dcc.shape[2], dcc.shape[3])[2][-1][0]:] = 0
            dcc = dcc * keep.view(dcc.shape[0], 1, dcc.shape[2], dcc.shape[3])
        return {"dW": _wgrad_sum(dcc, cat), "dcc": dcc}
    gx, xb = conv_t_ref(dcc, wx)
    gw, wb = wgrad_ref(dcc, x, hist, h0, variant if variant in ("h_t_not_prev", "last_share") else None)
    return {"dW": gw, "grad_x": gx, "grad_h0": ch, "grad_c0": ccar, "cc": cc, "c_seq": cs, "dcc": dcc,
            "bounds": {"dW": wb, "grad_x": xb, "grad_h0": hb, "grad_c0": EPS * ec}}
