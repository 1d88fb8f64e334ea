"""Saturating inputs, float64 references and deliberately wrong references for every ReLU6 site of the kernels
(tests/test_act_clamps_cpu.py, tests/test_act_clamps_gpu.py).

Recipe.  `rnd(shape, seed, scale)` as in tests/test_hip_kernels.py: x in +-2, weights in +-1 / sqrt(fan-in), depthwise weights
+-0.4.  A BatchNorm that feeds a ReLU6 gets scale = (rnd * 0.5 + 1) * G and bias = rnd + 3, with G = 5 where the stage reads
raw x and G = 2 where it reads a ReLU6 output in [0, 6]; the expanded tensor a caller hands to the fused depthwise loader or
to dwproj is (rnd * 5 + 3).clamp(0, 6), so it holds both 0 and 6.  A BatchNorm in front of no activation or of a sigmoid
keeps the old recipe (scale in [0.5, 1.5], bias in +-1).

Condition (`share_ok`, on the float64 pre-activations of the reference, never on kernel output): a ReLU6 stage with at least
1000 values holds >= 5 % of them at or below 0, >= 5 % at or above 6 and >= 25 % strictly inside; a smaller stage at least
one element of each.

Reference.  A `Problem` is one set of inputs with the float64 chain built from plan_ref64.stage / activate (values and the
abs-value companion B of every stage); `Problem.ref(prec)` is the plan_ref64.Ref whose `bound` is the per-element error
bound: the sum of the stages' rtol(prec, K) times B (ReLU6 has Lipschitz constant 1), `_split_atol` for f16x3, and for
Winograd B from `wino_conv(..., absolute=True)` with rtol = (LAMBDA sqrt(Cin) + 20) U as in plan_ref64.ref_wino.  Single-pass
bf16 has no entry in plan_ref64.REP: both operands of a product are within 2^-8 of their values, 2^-7 per product
(`REP_BF16`; a regression bound, as bf16x3's is).

Wrong references (`Problem.wrongs`): `no_hi@S` (stage S computes max(v, 0)), `no_lo@S` (min(v, 6)) for every ReLU6 stage S
of the op (E: expand, D: depthwise, out: the final epilogue), and `res_inside` (clamp(y + res) instead of clamp(y) + res)
where a residual follows a ReLU6.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import plan_ref64 as R

G_RAW, G_ACT = 5.0, 2.0
REP_BF16 = 2.0 ** -7            # single-pass bf16: regression bound (not a shipped precision)
RELU6 = R.ACT_RELU6


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def bn_sat(c, seed, gain):
    """Folded BatchNorm in front of a ReLU6: both clamps populated."""
    return (rnd((c,), seed) * 0.5 + 1.0) * gain, rnd((c,), seed + 1) + 3.0


def bn_old(c, seed):
    return rnd((c,), seed) * 0.5 + 1.0, rnd((c,), seed + 1)


def expanded(shape, seed):
    return (rnd(shape, seed) * 5.0 + 3.0).clamp(0, 6)


def rtol(prec, k):
    if prec == "bf16":
        return R.LAMBDA * R.U * math.sqrt(k) + REP_BF16
    return R.rtol(prec, k)


def shares(pre):
    n = pre.numel()
    lo, hi = int((pre <= 0).sum()), int((pre >= 6).sum())
    return n, lo, hi, n - lo - hi


def share_ok(pre):
    n, lo, hi, mid = shares(pre)
    if n >= 1000:
        return lo >= 0.05 * n and hi >= 0.05 * n and mid >= 0.25 * n
    return lo >= 1 and hi >= 1 and mid >= 1


def relu6(pre, stage, variant):
    """The ReLU6 of stage `stage`, or what the wrong reference `variant` puts in its place."""
    if variant == "no_hi@" + stage:
        return pre.clamp(min=0.0)
    if variant == "no_lo@" + stage:
        return pre.clamp(max=6.0)
    return R.activate(pre, pre, RELU6)[0]


def d64(t):
    return None if t is None else t.double()


class Problem:
    """One set of inputs and its float64 chain.  `chain(variant)` -> (y, B, E, pres: {stage: pre-activation}, extra atol);
    `gemm_k` the K of the stage that runs in the launch's precision, `f32_ks` the K of the stages that are always fp32;
    `out_res`: the residual added after the final ReLU6 (None: none); `wino`: (x, w, s, b) for the Winograd bound."""

    def __init__(self, key, family, inputs, chain, stages, gemm_k=None, f32_ks=(), out_res=None, split=None, wino=None,
                 extra_rt=0.0):
        self.key, self.family, self.inputs, self._chain, self.stages = key, family, inputs, chain, stages
        self.gemm_k, self.f32_ks, self.out_res, self.split, self.wino, self.extra_rt = gemm_k, f32_ks, out_res, split, wino, extra_rt
        self._cache = {}

    @property
    def wrongs(self):
        w = ["%s@%s" % (m, s) for s in self.stages for m in ("no_hi", "no_lo")]
        if self.out_res is not None and "out" in self.stages:
            w.append("res_inside")
        return w

    def chain(self, variant=None):
        if variant not in self._cache:
            self._cache[variant] = self._chain(variant)
        return self._cache[variant]

    def y(self, variant=None):
        return self.chain(variant)[0]

    def pres(self):
        return self.chain()[3]

    def ref(self, prec="f32", r=None):
        """plan_ref64.Ref of the right chain at `prec` (`r`: through Winograd F(r x r, 3x3))."""
        y, B, E, _, extra = self.chain()
        if r is not None:
            x, w, s, b = self.wino
            B = R.wino_conv(x, w, r, absolute=True) * R._vec(s.abs()) + R._vec(b.abs())
            if self.out_res is not None:
                B = B + self.out_res.abs()
            return R.Ref(y, B, E, None, (R.LAMBDA * math.sqrt(w.shape[1]) + 20) * R.U, extra)
        rt = sum(rtol("f32", k) for k in self.f32_ks) + (rtol(prec, self.gemm_k) if self.gemm_k else 0.0) + self.extra_rt
        atol = extra
        if self.split is not None:
            atol = atol + R._split_atol(prec, *self.split)
        return R.Ref(y, B, E, None, rt, atol)

    def bound(self, prec="f32", r=None):
        return R.bound(self.ref(prec, r))


_PROBLEMS = {}


def problem(key):
    """The problem of `key` = (family, *arguments), built once and shared (nothing may write to it)."""
    if key not in _PROBLEMS:
        _PROBLEMS[key] = BUILDERS[key[0]](key, *key[1:])
    return _PROBLEMS[key]


def forget(key):
    _PROBLEMS.pop(key, None)


def _finish(y_act, yb, res, pre, variant):
    """The AFFINE epilogue's tail as plan_ref64.ref_conv has it: activation, then the residual."""
    E = y_act.abs()
    y = y_act
    if res is not None:
        y = relu6(pre + res, "out", None) if variant == "res_inside" else y_act + res
        yb, E = yb + res.abs(), E + res.abs()
    return y, yb, E + y.abs()


# --------------------------------------------------------------------------------------------------------------- dense convs
def build_conv(key, n, h, w, cin, cout, k, use_res, seed=1):
    x = rnd((n, cin, h, w), seed, 2.0)
    wt = rnd((cout, cin, k, k), seed + 1, 1.0 / np.sqrt(cin * k * k))
    s, b = bn_sat(cout, seed + 2, G_RAW)
    res = rnd((n, cout, h, w), seed + 4) if use_res else None
    x6, w6, s6, b6, r6 = d64(x), d64(wt), d64(s), d64(b), d64(res)

    def chain(variant):
        pre, yb = R.stage(x6, x6.abs(), w6, s6, b6, R.ACT_NONE, padding=k // 2)
        y, yb, E = _finish(relu6(pre, "out", variant), yb, r6, pre, variant)
        return y, yb, E, {"out": pre}, 0.0

    return Problem(key, "conv", dict(x=x, w=wt, s=s, b=b, res=res), chain, ["out"], gemm_k=cin * k * k, out_res=r6,
                   split=(s6, w6, 2.0, cin * k * k), wino=(x6, w6, s6, b6) if k == 3 else None)


def build_ngroup(key, n, h, w, cin, ng, groups, seed=301):
    x = rnd((n, groups * cin, h, w), seed, 2.0)
    wt = rnd((groups * ng, cin, 1, 1), seed + 1, 1.0 / np.sqrt(cin))
    s, b = bn_sat(groups * ng, seed + 2, G_RAW)
    x6, w6, s6, b6 = d64(x), d64(wt), d64(s), d64(b)

    def chain(variant):
        outs = [R.stage(x6[:, g * cin:(g + 1) * cin], x6[:, g * cin:(g + 1) * cin].abs(), w6[g * ng:(g + 1) * ng], None, None,
                        R.ACT_NONE) for g in range(groups)]
        pre, yb = torch.cat([o[0] for o in outs], 1), torch.cat([o[1] for o in outs], 1)
        pre, yb = pre * R._vec(s6) + R._vec(b6), yb * R._vec(s6.abs()) + R._vec(b6.abs())
        y, yb, E = _finish(relu6(pre, "out", variant), yb, None, pre, variant)
        return y, yb, E, {"out": pre}, 0.0

    return Problem(key, "conv", dict(x=x, w=wt, s=s, b=b), chain, ["out"], gemm_k=cin, split=(s6, w6, 2.0, cin))


def build_vconcat(key, hw, segs, n, seed=80):
    """Winograd reading a virtual concat: the segments on a smaller map are resized first (bilinear, align_corners=True);
    the resize's own fp32 error (plan_ref64.bilinear_ac: 4 U B + X) reaches the output through |w| |s|."""
    h, w = hw
    xs = [rnd((n, c, sh, sw), seed + i, 2.0) for i, (c, sh, sw) in enumerate(segs)]
    cin, cout = sum(c for c, _, _ in segs), 32
    wt = rnd((cout, cin, 3, 3), seed + 10, 1.0 / np.sqrt(9 * cin))
    s, b = bn_sat(cout, seed + 11, G_RAW)
    parts, errs = [], []
    for t in xs:
        t6 = t.double()
        if tuple(t.shape[2:]) == (h, w):
            parts.append(t6)
            errs.append(torch.zeros_like(t6))
        else:
            y_, b_, x_ = R.bilinear_ac(t6, h, w)
            parts.append(y_)
            errs.append(4 * R.U * b_ + x_)
    cat, err_in = torch.cat(parts, 1), torch.cat(errs, 1)
    w6, s6, b6 = d64(wt), d64(s), d64(b)

    def chain(variant):
        pre, yb = R.stage(cat, cat.abs(), w6, s6, b6, R.ACT_NONE, padding=1)
        y, yb, E = _finish(relu6(pre, "out", variant), yb, None, pre, variant)
        return y, yb, E, {"out": pre}, F.conv2d(err_in, w6.abs(), padding=1) * R._vec(s6.abs())

    return Problem(key, "wino", dict(xs=xs, w=wt, s=s, b=b, size=(h, w)), chain, ["out"], gemm_k=9 * cin,
                   wino=(cat, w6, s6, b6))


# ----------------------------------------------------------------------------------------------------------- depthwise family
def build_dw(key, n, h, w, c, stride, dil, seed=51, gain=G_RAW):
    """`dil`: one dilation, or a tuple: equal channel groups with their own dilation.  `gain`: see DW_SAT_GROUPS."""
    x = rnd((n, c, h, w), seed, 2.0)
    wt = rnd((c, 1, 3, 3), seed + 1, 0.4)
    s, b = bn_sat(c, seed + 2, gain)
    x6, w6, s6, b6 = d64(x), d64(wt), d64(s), d64(b)

    def chain(variant):
        if isinstance(dil, tuple):
            g = c // len(dil)
            outs = [R.stage(x6[:, i * g:(i + 1) * g], x6[:, i * g:(i + 1) * g].abs(), w6[i * g:(i + 1) * g], s6[i * g:(i + 1) * g],
                            b6[i * g:(i + 1) * g], R.ACT_NONE, padding=d_, dilation=d_, groups=g) for i, d_ in enumerate(dil)]
            pre, yb = torch.cat([o[0] for o in outs], 1), torch.cat([o[1] for o in outs], 1)
        else:
            pre, yb = R.stage(x6, x6.abs(), w6, s6, b6, R.ACT_NONE, stride=stride, padding=dil, dilation=dil, groups=c)
        y = relu6(pre, "out", variant)
        return y, yb, y.abs(), {"out": pre}, 0.0

    return Problem(key, "dw", dict(x=x, w=wt, s=s, b=b), chain, ["out"], f32_ks=(9,))


def build_dwdot(key, n, h, w, c, act, seed=161):
    x = rnd((n, c, h, w), seed, 2.0)
    wd = rnd((c, 1, 3, 3), seed + 1, 0.4)
    sd, bd = bn_sat(c, seed + 2, G_RAW)
    w2 = rnd((1, c, 1, 1), seed + 4, 2.0 / np.sqrt(c))
    s2, b2 = torch.tensor([1.3]), torch.tensor([-0.2])                # fp32, as the kernel receives them
    x6 = d64(x)

    def chain(variant):
        pre, db = R.stage(x6, x6.abs(), d64(wd), d64(sd), d64(bd), R.ACT_NONE, padding=1, groups=c)
        z, zb = R.stage(relu6(pre, "D", variant), db, d64(w2), d64(s2), d64(b2), R.ACT_NONE)
        y, yb = R.activate(z, zb, act)
        return y, yb, y.abs(), {"D": pre}, 0.0

    return Problem(key, "dw_dot", dict(x=x, wd=wd, sd=sd, bd=bd, w2=w2, s2=1.3, b2=-0.2, act=act), chain, ["D"], f32_ks=(9, c))


def build_stem(key, n, H, W, u8=False, seed=61):
    from iip_uavsal_saliency_amd import synth
    if u8:
        raw = torch.from_numpy(synth.synth_frames_u8(n, H, W))
        x6 = (raw.double() / 255.0 - R._vec(torch.tensor(synth.IMAGENET_MEAN, dtype=torch.float64))) / R._vec(
            torch.tensor(synth.IMAGENET_STD, dtype=torch.float64))
    else:
        raw = rnd((n, 3, H, W), seed, 2.0)
        x6 = raw.double()
    wt = rnd((32, 3, 3, 3), seed + 1, 0.3)
    s, b = bn_sat(32, seed + 2, G_RAW)

    def chain(variant):
        pre, yb = R.stage(x6, x6.abs(), d64(wt), d64(s), d64(b), R.ACT_NONE, stride=2, padding=1)
        y = relu6(pre, "out", variant)
        return y, yb, y.abs(), {"out": pre}, 0.0

    return Problem(key, "stem", dict(x=raw, w=wt, s=s, b=b), chain, ["out"], f32_ks=(27,), extra_rt=4 * R.U if u8 else 0.0)


def build_fused(key, n, h, w, cin, hid, cout, stride, use_res, seed=101):
    """An inverted-residual block in one launch (fused_ir.hip / fused_mid.hip): E and D never reach memory."""
    x = rnd((n, cin, h, w), seed, 2.0)
    expand = not (hid == cin == 32)
    w1 = rnd((hid, cin, 1, 1), seed + 1, 1.0 / np.sqrt(cin)) if expand else None
    wd = rnd((hid, 1, 3, 3), seed + 2, 0.4)
    w2 = rnd((cout, hid, 1, 1), seed + 3, 1.0 / np.sqrt(hid))
    b1 = bn_sat(hid, seed + 4, G_RAW)
    bd = bn_sat(hid, seed + 6, G_ACT if expand else G_RAW)
    b2 = bn_old(cout, seed + 8)
    x6 = d64(x)

    def chain(variant):
        v, B, pres = x6, x6.abs(), {}
        if expand:
            pres["E"], B = R.stage(v, B, d64(w1), d64(b1[0]), d64(b1[1]), R.ACT_NONE)
            v = relu6(pres["E"], "E", variant)
        pres["D"], B = R.stage(v, B, d64(wd), d64(bd[0]), d64(bd[1]), R.ACT_NONE, stride=stride, padding=1, groups=hid)
        y, yb = R.stage(relu6(pres["D"], "D", variant), B, d64(w2), d64(b2[0]), d64(b2[1]), R.ACT_NONE)
        if use_res:
            y, yb = y + x6, yb + x6.abs()
        return y, yb, y.abs(), pres, 0.0

    return Problem(key, "fused_mid" if hid >= 384 else "fused_ir", dict(x=x, w1=w1, b1=b1, wd=wd, bd=bd, w2=w2, b2=b2), chain,
                   (["E"] if expand else []) + ["D"], f32_ks=((cin,) if expand else ()) + (9, hid))


def build_dwgemm(key, n, h, w, c, cout, stride, act, use_res, seed=151):
    """dw3x3 + BN + ReLU6 in front of a 1x1 GEMM in one launch (the fused loader of conv_gemm.hip, dwproj.hip)."""
    e = expanded((n, c, h, w), seed)
    wd = rnd((c, 1, 3, 3), seed + 1, 0.4)
    sd, bd = bn_sat(c, seed + 2, G_ACT)
    wp = rnd((cout, c, 1, 1), seed + 4, 1.0 / np.sqrt(c))
    sp, bp = bn_sat(cout, seed + 5, G_ACT) if act == RELU6 else bn_old(cout, seed + 5)
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    res = rnd((n, cout, ho, wo), seed + 7) if use_res else None
    e6, r6 = d64(e), d64(res)
    dmax = []

    def chain(variant):
        pres = {}
        pres["D"], B = R.stage(e6, e6.abs(), d64(wd), d64(sd), d64(bd), R.ACT_NONE, stride=stride, padding=1, groups=c)
        dmax.append(float(B.max()))
        pre, yb = R.stage(relu6(pres["D"], "D", variant), B, d64(wp), d64(sp), d64(bp), R.ACT_NONE)
        if act == RELU6:
            pres["out"] = pre
            y, yb, E = _finish(relu6(pre, "out", variant), yb, r6, pre, variant)
        else:
            y, yb, E = _finish(pre, yb, r6, pre, None)
        return y, yb, E, pres, 0.0

    p = Problem(key, "dwgemm", dict(e=e, wd=wd, sd=sd, bd=bd, wp=wp, sp=sp, bp=bp, res=res), chain,
                ["D"] + (["out"] if act == RELU6 else []), gemm_k=c, f32_ks=(9,), out_res=r6 if act == RELU6 else None)
    p.chain()
    p.split = (d64(sp), d64(wp), dmax[0], c)
    return p


BUILDERS = {"conv": build_conv, "ngroup": build_ngroup, "vconcat": build_vconcat, "dw": build_dw, "dwdot": build_dwdot,
            "stem": build_stem, "fused": build_fused, "dwgemm": build_dwgemm}


# ------------------------------------------------------------------------------------------------------------------- launches
class Launch:
    """One kernel call on a problem: `op` names the ops entry point and how it is called, `kw` its arguments."""

    def __init__(self, id, family, key, op, prec="f32", route=None, **kw):
        self.id, self.family, self.key, self.op, self.prec, self.route, self.kw = id, family, key, op, prec, route, kw

    def __repr__(self):
        return self.id


def _launches():
    from iip_uavsal_saliency_amd import _lib as L
    out = []

    def add(id, family, key, op, **kw):
        out.append(Launch(id, family, key, op, **kw))

    # ---- ops.conv_gemm, act = RELU6
    for use_res in (False, True):                                     # M = 286: ragged against every tile height
        key = ("conv", 2, 11, 13, 64, 160, 1, use_res)
        for prec in ("f32", "f16x3", "bf16x3"):
            for tile in range(1, 8):
                add("staged-%s-t%d%s" % (prec, tile, "-res" if use_res else ""), "conv/staged", key, "conv", prec=prec, tile=tile,
                    route=dict(tile=tile if prec == "f32" or tile < 7 else 1, ksplit=1))      # (tile 7 is fp32 only)
        add("staged-bf16-t0%s" % ("-res" if use_res else ""), "conv/bf16", key, "conv", prec="bf16", tile=0,
            route=dict(family=L.ROUTE_STAGED, ksplit=1))
    for tile in (8, 9, 10, 11):                                       # 32-float K stages
        add("k32-1x1-t%d" % tile, "conv/k32", ("conv", 3, 7, 5, 320, 256, 1, False), "conv", tile=tile,
            route=dict(family=L.ROUTE_K32, tile=tile, ksplit=1))
        add("k32-3x3-t%d-res" % tile, "conv/k32", ("conv", 1, 12, 20, 64, 96, 3, True), "conv", tile=tile,
            route=dict(family=L.ROUTE_K32, tile=tile, ksplit=1))
    add("scalar-cout33", "conv/scalar", ("conv", 2, 5, 7, 20, 33, 1, False), "conv", route=dict(ksplit=1))
    add("scalar-cout1", "conv/scalar", ("conv", 1, 5, 4, 1536, 1, 1, False, 11), "conv", route=dict(ksplit=1))
    add("scalar-slice-pitch193", "conv/scalar", ("conv", 2, 6, 9, 32, 64, 1, False), "conv", out_slice=(193, 64),
        route=dict(ksplit=1))
    add("ksplit-f16x3-t4", "conv/ksplit", ("conv", 1, 7, 9, 768, 36, 1, False), "conv", prec="f16x3", tile=4, stream_k=True,
        route=dict(family=L.ROUTE_STAGED, tile=4, ksplit=">1", reduce=L.REDUCE_LAUNCH))
    for tile in (8, 10, 11):
        add("ksplit-f32-t%d-res" % tile, "conv/ksplit", ("conv", 2, 12, 20, 1920, 256, 1, True), "conv", tile=tile, stream_k=True,
            route=dict(family=L.ROUTE_K32, tile=tile, ksplit=">1", reduce=L.REDUCE_LAUNCH if tile == 8 else L.REDUCE_IN_LAUNCH))
    add("streamk-f32-t1", "conv/streamk", ("conv", 5, 45, 80, 1024, 256, 1, False), "conv", tile=1, stream_k=True,
        route=dict(family=L.ROUTE_STREAMK, tile=1))
    for prec in ("f32", "f16x3", "bf16x3"):                           # fused depthwise loader: D is the ReLU6, the output linear
        add("dwloader-s2-%s" % prec, "conv/dwloader", ("dwgemm", 2, 23, 41, 96, 24, 2, 0, False), "dwgemm", prec=prec,
            route=dict(family=L.ROUTE_STAGED, ksplit=1))
        add("dwloader-s1-%s" % prec, "conv/dwloader", ("dwgemm", 1, 9, 13, 48, 64, 1, 0, False), "dwgemm", prec=prec,
            route=dict(family=L.ROUTE_STAGED if prec == "bf16x3" else L.ROUTE_DWPROJ, ksplit=1))    # (stride 1: dwproj has no bf16x3)
    add("presplit-1x1-t1", "conv/presplit", ("conv", 3, 7, 5, 320, 256, 1, False), "conv", prec="f16x3", tile=1, split_in=True,
        split_out=True, route=dict(family=L.ROUTE_PRESPLIT, tile=1))
    add("presplit-3x3-t1-res", "conv/presplit", ("conv", 2, 9, 11, 64, 96, 3, True), "conv", prec="f16x3", tile=1, split_in=True,
        split_out=True, route=dict(family=L.ROUTE_PRESPLIT, tile=1))
    add("ngroup-2x64", "conv/ngroup", ("ngroup", 2, 9, 13, 96, 64, 2), "conv", n_group=64, route=dict(ksplit=1))
    # ---- ops.conv3x3_winograd
    for r in (2, 4):
        add("wino%d-2x3-res" % r, "wino", ("conv", 2, 2, 3, 64, 64, 3, True), "wino", r=r)
        add("wino%d-12x20" % r, "wino", ("conv", 1, 12, 20, 64, 96, 3, False), "wino", r=r)
        add("wino%d-vconcat" % r, "wino", ("vconcat", (9, 13), ((8, 3, 4), (24, 5, 7)), 3), "wino", r=r)
    # ---- ops.dw3x3 (n, h, w, c, stride, dilation)
    for c_ in DW_SAT_CASES:
        add("dw-%s" % "x".join(str(v) for v in c_[:6]), "dw", ("dw",) + c_, "dw")
    for c_ in DW_SAT_GROUPS:
        add("dwgroups-%s-d%s" % ("x".join(str(v) for v in c_[:4]), "_".join(str(v) for v in c_[4])), "dw",
            ("dw",) + c_[:4] + (1, c_[4]) + c_[5:], "dw")
    add("dw-split-out", "dw", ("dw", 1, 23, 41, 96, 2, 1), "dw", split_out=True)
    # ---- ops.dw3x3_dot
    for c_ in [(1, 7, 9, 256), (1, 1, 1, 256), (3, 13, 17, 512)]:
        for act in (0, 2):
            seed = (201,) if c_ + (act,) == (1, 1, 1, 256, 2) else ()      # (one output value: a seed whose sigmoid is not saturated)
            add("dwdot-%s-act%d" % ("x".join(str(v) for v in c_), act), "dw_dot", ("dwdot",) + c_ + (act,) + seed, "dwdot")
    # ---- ops.stem_conv
    for c_ in [(2, 7, 9), (1, 17, 129), (1, 1, 1)]:
        add("stem-%dx%dx%d" % c_, "stem", ("stem",) + c_, "stem")
    add("stem-u8", "stem", ("stem", 2, 24, 300, True), "stem")
    # ---- ops.fused_ir (n, h, w, cin, hidden, cout, stride, residual)
    for c_ in [(2, 20, 36, 32, 32, 16, 1, False), (2, 21, 35, 16, 96, 24, 2, False), (1, 19, 27, 24, 144, 24, 1, True),
               (3, 9, 13, 32, 192, 64, 2, False), (1, 5, 3, 16, 96, 24, 2, False)]:
        for tile in (1, 2):
            add("fused_ir-%s-t%d" % ("x".join(str(int(v)) for v in c_), tile), "fused_ir", ("fused",) + c_, "fused", tile=tile)
    for c_ in [(3, 4, 8, 64, 384, 64), (1, 5, 9, 96, 576, 96), (1, 9, 13, 64, 384, 32), (1, 1, 1, 64, 384, 64)]:
        add("fused_mid-%s" % "x".join(str(v) for v in c_), "fused_mid", ("fused",) + c_ + (1, c_[3] == c_[5]), "fused", tile=0)
    # ---- dwproj (n, h, w, hidden, cout, act, residual, sliced), called as test_depthwise_projection_lds_halo calls it
    for c_ in DWPROJ_SAT_CASES:
        n, h, w, hid, cout, act, use_res, sliced = c_
        for prec in ("f32", "f16x3"):
            inst = 256 if cout > 128 else 128 if cout > 64 else 64 if cout > 32 else 32
            rt = dict(family=L.ROUTE_DWPROJ, dwproj=inst)
            if c_ == DWPROJ_SAT_CASES[-1]:
                rt.update(ksplit=">1", reduce=L.REDUCE_LAUNCH)
            add("dwproj-%s-%s" % ("x".join(str(int(v)) for v in c_), prec), "dwproj",
                ("dwgemm", n, h, w, hid, cout, 1, act, use_res, 251), "dwgemm", prec=prec, sliced=sliced, route=rt)
    return out


# (n, h, w, c, stride, dilation[, seed]).  One pixel: only the centre tap counts; seed 71 puts an element on each clamp.
DW_SAT_CASES = [(2, 9, 13, 48, 1, 1), (1, 5, 3, 144, 2, 1), (1, 1, 1, 64, 1, 1, 71), (1, 2, 2, 64, 2, 1),
                (1, 12, 20, 120, 1, 2), (2, 7, 5, 20, 1, 4),          # whole-map LDS, 16-channel slabs
                (1, 45, 80, 64, 1, 2),                                # generic dilated
                # the variants of uavsal_dw_variant that the older depthwise tests reach only at larger shapes, at the smallest
                # shapes that select them: 32-channel slabs (>= 256 slabs, last one narrower), 512-thread workgroups (>= 2048
                # items per slab), 4 x 4 patches (>= 512 workgroups of them; 5 x 5 maps: partial patches on both edges)
                (8, 4, 5, 1020, 1, 2), (1, 17, 31, 20, 1, 2), (32, 5, 5, 4096, 1, 1)]
# (n, h, w, c, dilations[, seed, gain]).  Dilation 40 on a 20 x 30 map leaves the centre tap alone: |x w| <= 0.8, and with G = 5
# only 2.9 % / 3.8 % of the pre-activations reach the clamps; G = 10 holds the condition (12 % / 13 %).
DW_SAT_GROUPS = [(2, 9, 13, 192, (2, 3, 5)), (2, 20, 30, 64, (40,), 51, 10.0), (3, 25, 33, 128, (30, 5))]
DWPROJ_SAT_CASES = [(3, 13, 21, 96, 192, 1, False, False), (2, 9, 17, 48, 128, 0, True, True), (2, 1, 37, 32, 40, 1, False, True),
                    (1, 23, 1, 16, 24, 0, False, False), (2, 9, 20, 384, 40, 1, True, True),
                    (1, 16, 32, 768, 1, 1, False, False)]             # K split over workgroups; ReLU6 on one output channel

_LAUNCHES = []


def launches():
    if not _LAUNCHES:
        _LAUNCHES.extend(_launches())
    return _LAUNCHES


def dw_variant(n, h, w, c, stride, dil):
    """uavsal_dw_variant (a host-side query) of a depthwise case; `dil` a tuple: channel groups."""
    import ctypes
    from iip_uavsal_saliency_amd import _lib as L
    d = L.DwDesc()
    d.n_img, d.H, d.W, d.C, d.stride, d.dilation = n, h, w, c, stride, 1 if isinstance(dil, tuple) else dil
    if isinstance(dil, tuple):
        d.dil_group_c = c // len(dil)
        for i, dd in enumerate(dil):
            d.dil_groups[i] = dd
    return int(L.load().uavsal_dw_variant(ctypes.byref(d)))


def conv_desc(lch):
    """The descriptor ops.conv_gemm fills for a conv / dwgemm launch, with dummy pointers: what the route query reads."""
    from iip_uavsal_saliency_amd import _lib as L
    PTR = 1 << 20
    kw, key = lch.kw, lch.key
    d = L.ConvDesc()
    if key[0] == "dwgemm":
        _, n, hin, win, cin, cout, stride, act, use_res = key[:9]
        h, w, taps = (hin - 1) // stride + 1, (win - 1) // stride + 1, 1
        d.dw_w9c, d.dw_scale, d.dw_bias, d.dw_stride, d.dw_Hin, d.dw_Win = PTR, PTR, PTR, stride, hin, win
        ws = True
    elif key[0] == "ngroup":
        _, n, h, w, cin, ng, groups = key[:7]
        hin, win, cout, taps, act, use_res, ws = h, w, ng * groups, 1, RELU6, False, False
        d.n_group, d.a_group_off = ng, cin
    else:
        _, n, h, w, cin, cout, k, use_res = key[:8]
        hin, win, taps, act, ws = h, w, k * k, RELU6, bool(kw.get("stream_k"))
    lda = cin * (key[6] if key[0] == "ngroup" else 1)
    ldc = kw["out_slice"][0] if kw.get("out_slice") else cout + (16 if kw.get("sliced") else 0)
    d.a, d.lda, d.a_img_stride = PTR, lda, hin * win
    d.w, d.out, d.ldc, d.o_img_stride = PTR, PTR, ldc, h * w
    d.scale, d.bias = PTR, PTR
    if use_res:
        d.res, d.ldr, d.r_img_stride = PTR, ldc if kw.get("sliced") else cout, h * w
    if kw.get("split_in"):
        d.a_split, d.ldas = PTR, 2 * cin
    if kw.get("split_out"):
        d.out_split, d.ldos = PTR, 2 * cout
    d.n_img, d.H, d.W, d.Cin, d.Cout, d.taps = n, h, w, cin, cout, taps
    d.prec, d.act, d.epi, d.tile = L.PREC[lch.prec], act, L.EPI_AFFINE, kw.get("tile", 0)
    if ws:
        d.sk_ws, d.sk_ws_bytes = PTR, int(L.load().uavsal_streamk_workspace_bytes())
    return d


def route_matches(rt, want):
    """`rt`: a route as a dict; `want`: the fields a launch fixes ('>1': more than one K share)."""
    return all((rt[f] > 1) if v == ">1" else (rt[f] == v) for f, v in (want or {}).items())
