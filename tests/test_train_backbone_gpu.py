"""Fine-tuning the deep backbone on the MI355X (uavsal_pix_gemm with `tails32`, train.block_backward(backbone=True),
train.srf_head_backward(need_tap_grads=True), train.backbone_backward, recurrence_step(backbone=True)) against the float64
restatement of tests/backbone_ref64.py.  The kernels are tested teacher-forced, the walks STAGE BY STAGE (every stage, handed
in float64 what the device handed it in fp32, within its own derived bound: ctx_ref64's docstring says why a bound composed
over a chain of blocks is worthless), and whole walks against float64 autograd to the accuracy an fp32 forward allows (masks
decided by fp32 activations may differ from float64's at a handful of elements: the loose 2e-3 of each tensor's norm that
tests/test_train_st_gpu.py and tests/test_train_srf_gpu.py use -- the stage-by-stage tests are the sharp ones)."""
import ctypes as C
import os
from functools import lru_cache

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from iip_uavsal_saliency_amd import _lib, losses, model_feature, ops, synth, train
from iip_uavsal_saliency_amd.model import uavsal_srfnet_aspp
from iip_uavsal_saliency_amd.weights import WeightCache

import backbone_ref64 as BK
import block_ref64 as BR
import ctx_ref64 as X
import mp_ref64 as MP
import srf_ref64 as SF
from plan_ref64 import EPS, rtol

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = BK.U
NAN = float("nan")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _check(got, want, bound, what):
    got, want, bound = got.detach().double().cpu(), want.double().cpu(), bound.double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), what
    r = float(((got - want).abs() / bound.clamp_min(1e-300)).max()) if got.numel() else 0.0
    print("%s: worst error / bound %.3f" % (what, r))
    assert r <= 1.0, (what, r)
    return r


def _loose(got, want, what, tol=2e-3):
    got, want = got.detach().double().cpu(), want.double().cpu()
    err = float((got - want).norm()) / max(float(want.norm()), 1e-300)
    print("%s: relative error in norm %.3e" % (what, err))
    assert err <= tol, (what, err)


def _fenced(t, pad=4):
    """An NHWC tensor as a channel slice between NaN columns."""
    whole = torch.full(t.shape[:-1] + (t.shape[-1] + 2 * pad,), NAN, dtype=t.dtype, device=t.device)
    whole[..., pad:-pad] = t
    return whole[..., pad:-pad]


c64 = lambda t: t.detach().double().cpu()                                 # noqa: E731
nchw = lambda t: t.permute(0, 3, 1, 2)                                    # noqa: E731
nhwc = lambda t: t.permute(0, 2, 3, 1)                                    # noqa: E731
ids3 = lambda p: "%dx%dx%d" % tuple(p)                                    # noqa: E731


def _cl(a):
    return torch.as_tensor(a).to(DEV).float().contiguous(memory_format=torch.channels_last)


# ------------------------------------------------------------------------------------------------ 1. the pixel GEMM
def _shares(K, M, N, tails32):
    d = _lib.PixGemmDesc()
    d.K, d.M, d.N, d.tails32 = K, M, N, int(tails32)
    return _lib.load().uavsal_pix_gemm_shares(C.byref(d))


@pytest.mark.parametrize("pic", BK.GEMM_K, ids=ids3)
@pytest.mark.parametrize("M,N", BK.GEMM_NEW + BK.GEMM_OLD)
def test_pix_gemm_against_float64(M, N, pic):
    a, b, w, s = (torch.from_numpy(t) for t in BK.gemm_inputs(M, N, pic))
    K = pic[0] * pic[1] * pic[2]
    G, eG = BK.pix_gemm_ref(a.double(), b.double())
    A = a.double().reshape(K, M).abs().T @ b.double().reshape(K, N).abs()
    av, bv = _fenced(a.to(DEV)), _fenced(b.to(DEV))                       # the neighbouring channels hold NaN
    wd, sd = w.to(DEV), s.to(DEV)
    box = torch.full(((M + 2) * N,), NAN, dtype=torch.float32, device=DEV)
    out = box[N:(M + 1) * N].view(M, N)
    rowdot = torch.full((M + 2,), NAN, dtype=torch.float64, device=DEV)
    new = (M, N) in BK.GEMM_NEW
    assert _shares(K, M, N, True) == BK.shares(K, M, N) and _shares(K, M, N, False) == (0 if new else BK.shares(K, M, N))
    if new and K == 2760:
        assert BK.shares(K, M, N) == 22                                   # shares are real: 22 units of 128 pixels
    tag = "pix_gemm %dx%d K=%d (%d shares)" % (M, N, K, BK.shares(K, M, N))
    train.pix_gemm(av, bv, out=out, row_scale=sd, w=wd, rowdot=rowdot[1:M + 1], tails32=True)
    s64 = s.double().view(-1, 1)
    _check(out, s64 * G, s64 * (eG + U * A) + 1e-300, tag)
    _check(rowdot[1:M + 1], (w.double() * G).sum(1), (w.double().abs() * eG).sum(1) + 1e-300, tag + " rowdot")
    assert bool(torch.isnan(box[:N]).all()) and bool(torch.isnan(box[(M + 1) * N:]).all()) and bool(torch.isnan(rowdot[[0, M + 1]]).all())
    first, dot = out.clone(), rowdot.clone()
    train.pix_gemm(av, bv, out=out, row_scale=sd, w=wd, rowdot=rowdot[1:M + 1], tails32=True)
    assert torch.equal(_bits(out), _bits(first)) and torch.equal(rowdot[1:M + 1], dot[1:M + 1])      # the same bits twice
    plain = train.pix_gemm(a.to(DEV), b.to(DEV), tails32=True)            # dense operands, no scale: the same sums
    _check(plain, G, eG + 1e-300, tag + " unscaled")
    train.pix_gemm(av, bv, out=out, row_scale=sd, accumulate=True, tails32=True)
    _check(out, 2 * first.double(), 4 * U * first.double().abs() + 1e-300, tag + " accumulate")
    assert bool(torch.isnan(box[:N]).all()) and bool(torch.isnan(box[(M + 1) * N:]).all())
    if new:                                                               # without the flag: refused, as it always was
        with pytest.raises(RuntimeError, match="ESHAPE|shape|rejected"):
            train.pix_gemm(a.to(DEV), b.to(DEV))
        for v in ("m_tail", "n_tail", "last_share"):
            wrong = BK.pix_gemm_ref(a.double(), b.double(), v)[0]
            if not torch.equal(wrong, G):
                assert float(((c64(plain) - wrong).abs() / eG).max()) > 1.0, v
    else:                                                                 # a shape it always took: its bits with and without
        assert torch.equal(_bits(train.pix_gemm(a.to(DEV), b.to(DEV))), _bits(plain))


# ------------------------------------------------------------------------------------------------ 2. one block
@lru_cache(maxsize=None)
def _block_case(name, pic):
    cfg = BK.BLOCKS[name]
    x, q, go = BK.block_case(name, pic)
    block = BK.make_block(cfg, q, model_feature.InvertedResidual).to(DEV)
    p = BR.fold(BR.to64(q))
    x64, go64 = torch.as_tensor(x).double(), torch.as_tensor(go).double()
    return cfg, block, p, x64, go64, _cl(x), _cl(go)


def _dense(t64, keep_masks=False):
    t = BR.teacher_round(t64) if keep_masks else t64.float()
    return nhwc(t.to(DEV)).contiguous()


@pytest.mark.parametrize("pic", BK.PICTURES, ids=ids3)
@pytest.mark.parametrize("name", list(BK.BLOCKS))
def test_block_param_grads_teacher_forced(name, pic):
    cfg, block, p, x64, go64, x, go = _block_case(name, pic)
    pt = MP.block_parts(p, x64, go64, cfg[3])
    for t in (pt["e"], pt["d"]):
        assert min(BR.class_shares(t)) > 0.02                            # 0, 6 and the interior
    e, d, gd, ga = _dense(pt["e"], True), _dense(pt["d"], True), _dense(pt["gd"]), _dense(pt["ga"])
    got = train.block_param_grads(block, x, e, d, go, gd=gd, ga=ga, backbone=True)
    want, bound = MP.grads_from_parts(p, x64, pt["e"], pt["d"], pt["gd"], pt["ga"], go64, cfg[3], bounds=True)
    for k in BK.NAMES:
        _check(got[k], want[k], bound[k] + 1e-300, "block %s %s teacher-forced %s" % (name, ids3(pic), k))
    assert all(q.grad is None for q in block.parameters())
    # ... and against the reference's own dwBlock under float64 autograd (tests/golden/backbone_*.npz), within the same bounds
    z = np.load(os.path.join(GOLDEN, BK.golden_name(name, pic) + ".npz"))
    assert str(z["digest"]) == BK.golden_digest(*BK.block_case(name, pic))
    mine, bnd = BK.golden_pack({k: c64(v) for k, v in got.items()}), BK.golden_pack({k: v for k, v in bound.items()})
    for k in mine:
        if not k.endswith("_sum") and not k.endswith("_l2"):
            _check(torch.as_tensor(mine[k]), torch.as_tensor(z[k]), torch.as_tensor(bnd[k]) + 1e-300, "block %s %s golden %s" % (name, ids3(pic), k))
    again = train.block_param_grads(block, x, e, d, go, gd=gd, ga=ga, backbone=True)
    assert all(torch.equal(_bits(got[k]), _bits(again[k])) for k in BK.NAMES)
    with pytest.raises(RuntimeError, match="expand conv|Cout"):            # without the keyword: what it always took
        train.block_backward(block, x, go)


def _forward_bounds(p, x, stride):
    """(err_e, err_d): ctx_ref64.forward_bound's first two lines, the recomputed e and d against the float64 forward."""
    f = X.forward(p, x, stride, False)
    hid, cin = p["w1"].shape[:2]
    be_pre = F.conv2d(x.abs(), p["w1"].abs()) * X._v(p["s1"].abs()) + X._v(p["b1"].abs())
    err_e = rtol("f32", cin) * be_pre + EPS * 2 * f["e_pre"].abs()
    bd_pre = F.conv2d(be_pre, p["wd"].abs(), padding=1, stride=stride, groups=hid) * X._v(p["s2"].abs()) + X._v(p["b2"].abs())
    return f, err_e, (rtol("f32", cin) + rtol("f32", 9)) * bd_pre + EPS * 2 * f["d_pre"].abs()


def _stage_check(p, cfg, x, go, pt, grads, gx, tag, res=None):
    """One block of a walk, stage by stage, on the tensors the device held (NHWC fp32 -> NCHW float64)."""
    pt64 = {k: nchw(c64(pt[k])) for k in ("e", "d", "gd", "ga")}
    x64, go64 = nchw(c64(x)), nchw(c64(go))
    want = BK.block_stage(p, cfg, x64, go64, pt64, res=None if res is None else nchw(c64(res)))
    f, err_e, err_d = _forward_bounds(p, x64, cfg[3])
    _check(nchw(pt["e"]), f["e"], err_e + 1e-300, tag + " e")
    # d from the device's own e: one depthwise launch
    d_pre = F.conv2d(pt64["e"], p["wd"], padding=1, stride=cfg[3], groups=p["wd"].shape[0]) * X._v(p["s2"]) + X._v(p["b2"])
    d_abs = F.conv2d(pt64["e"].abs(), p["wd"].abs(), padding=1, stride=cfg[3], groups=p["wd"].shape[0]) * X._v(p["s2"].abs()) + X._v(p["b2"].abs())
    _check(nchw(pt["d"]), d_pre.clamp(0, 6), rtol("f32", 9) * d_abs + EPS * 2 * d_pre.abs() + 1e-300, tag + " d")
    _check(nchw(pt["gd"]), *want["gd"], tag + " gd")
    _check(nchw(pt["ga"]), *want["ga"], tag + " ga")
    if gx is not None:
        _check(gx, *want["grad_x"], tag + " grad_x")
    for k in BK.NAMES:
        _check(grads[k], want[k][0], want[k][1] + 1e-300, "%s %s" % (tag, k))
    return want


@pytest.mark.parametrize("pic", BK.PICTURES, ids=ids3)
@pytest.mark.parametrize("name", list(BK.BLOCKS))
def test_block_backward_end_to_end(name, pic):
    cfg, block, p, x64, go64, x, go = _block_case(name, pic)
    pt = {}
    gx, grads = train.block_backward(block, x, go, parts=pt, backbone=True)
    n, H, W = BK.in_grid(name, pic)
    assert tuple(gx.shape) == (n, cfg[0], H, W) and tuple(pt["d"].shape) == (n, (H - 1) // cfg[3] + 1, (W - 1) // cfg[3] + 1, cfg[1])
    tag = "block %s %s" % (name, ids3(pic))
    want = _stage_check(p, cfg, nhwc(x), nhwc(go), pt, grads, gx, tag)
    # the whole block against float64 from its inputs alone: to what an fp32 forward allows
    auto = MP.autograd_grads({k: v for k, v in BR.to64(BK.block_case(name, pic)[1]).items()}, x64, go64, cfg[3], cfg[4])
    for k in BK.NAMES:
        _loose(grads[k], auto[k], "%s %s against autograd" % (tag, k))
    _loose(gx, X.input_grad_autograd(p, x64, go64, cfg[3], cfg[4]), tag + " grad_x against autograd")
    z = np.load(os.path.join(GOLDEN, BK.golden_name(name, pic) + ".npz"))                 # the reference's own block
    _loose(gx, torch.as_tensor(z["grad_x"]), tag + " grad_x against the reference golden")
    for k, v in BK.golden_pack({k: c64(v) for k, v in grads.items()}).items():
        if not k.endswith("_sum"):
            _loose(torch.as_tensor(v), torch.as_tensor(z[k]), "%s %s against the reference golden" % (tag, k))
    # wrong walks are rejected by the stage bounds
    pt64 = {k: nchw(c64(pt[k])) for k in ("e", "d", "gd", "ga")}
    if cfg[3] == 2:
        wrong = BK.block_stage(p, cfg, x64, go64, pt64, variant="s2_anchor")
        assert float(((nchw(c64(pt["ga"])) - wrong["ga"][0]).abs() / want["ga"][1].clamp_min(1e-300)).max()) > 1.0
    if cfg[4]:
        wrong = BK.block_stage(p, cfg, x64, go64, pt64, variant="no_residual")
        assert float(((c64(gx) - wrong["grad_x"][0]).abs() / want["grad_x"][1].clamp_min(1e-300)).max()) > 1.0
    # the same bits twice; no input gradient on request; accumulate doubles
    gx2, again = train.block_backward(block, x, go, backbone=True)
    assert torch.equal(_bits(gx), _bits(gx2)) and all(torch.equal(_bits(grads[k]), _bits(again[k])) for k in BK.NAMES)
    none, third = train.block_backward(block, x, go, need_x_grad=False, grads=again, accumulate=True, backbone=True)
    assert none is None
    for k in BK.NAMES:
        _check(third[k], 2 * grads[k].double(), 4 * U * grads[k].double().abs() + 1e-300, "%s accumulate %s" % (tag, k))


# ------------------------------------------------------------------------------------------------ 3. the head's tap gradients
@lru_cache(maxsize=None)
def _head():
    return SF.calibrate(uavsal_srfnet_aspp("mobilenet_v2")).to(DEV).eval()


@pytest.mark.parametrize("case", SF.GOLDEN_CASES, ids=SF.golden_name)
def test_srf_head_backward_tap_gradients(case):
    c3, c4, c5, go = (_cl(t) for t in SF.golden_inputs(case))
    sf = _head()
    tmp = {}
    train.srf_head_backward(sf, c3, c4, c5, torch.zeros_like(go), go, parts=tmp)
    cache = WeightCache(torch.device(DEV), {})
    y = nchw(train._conv(_lib.load(), cache, tmp["cat"], sf.conv_last[0], 256, 9, bn=sf.conv_last[1], act=_lib.ACT_RELU6))
    plain = train.srf_head_backward(sf, c3, c4, c5, y, go)
    pt = {}
    grads, g4, g5 = train.srf_head_backward(sf, c3, c4, c5, y, go, parts=pt, need_tap_grads=True)
    assert isinstance(plain, dict) and sorted(grads) == sorted(train.SRF_HEAD_PARAMS)
    assert all(torch.equal(_bits(grads[k]), _bits(plain[k])) for k in plain)           # the 42 gradients: the default call's bits
    assert g4.shape == c4.shape and g5.shape == c5.shape
    # stage by stage: the five GEMMs on the tensors the walk held
    P, B = SF.head_params64(sf)
    Pd = {k: v.detach() for k, v in P.items()}
    k64 = {k: nchw(c64(pt[k])) for k in ("a1", "x4", "g_aspp", "g_x4", "ga2", "ga3", "ga4")}
    terms = BK.head_tap_terms(Pd, B, k64)
    want5, b5 = BK.sum_terms(terms["c5"])
    want4, b4 = BK.sum_terms(terms["c4"])
    _check(g5, want5, b5 + 1e-300, "head %s g_c5" % SF.golden_name(case))
    _check(g4, want4, b4 + 1e-300, "head %s g_c4" % SF.golden_name(case))
    for drop in range(1, 4):                                              # a branch left out of the sum is rejected
        wrong, _ = BK.sum_terms([t for i, t in enumerate(terms["c5"]) if i != drop])
        assert float(((c64(g5) - wrong).abs() / b5.clamp_min(1e-300)).max()) > 1.0, drop
    # the whole head against float64 autograd
    t64 = [torch.as_tensor(t).double() for t in SF.golden_inputs(case)]
    c4r, c5r = t64[1].clone().requires_grad_(True), t64[2].clone().requires_grad_(True)
    a4, a5 = torch.autograd.grad(SF.forward64(P, B, t64[0], c4r, c5r), [c4r, c5r], t64[3])
    _loose(g4, a4, "head g_c4 against autograd")
    _loose(g5, a5, "head g_c5 against autograd")
    _, g4b, g5b = train.srf_head_backward(sf, c3, c4, c5, y, go, need_tap_grads=True)
    assert torch.equal(_bits(g4), _bits(g4b)) and torch.equal(_bits(g5), _bits(g5b))


# ------------------------------------------------------------------------------------------------ 4. the walk
@pytest.mark.parametrize("pic", BK.PICTURES, ids=ids3)
def test_backbone_backward_over_the_whole_chain(pic):
    c3, Q, g4, g5 = BK.chain_case(pic)
    feats = BK.make_features(Q, model_feature.mobilenet_v2_features()).to(DEV)
    c3d, g4d, g5d = _cl(c3), _cl(g4), _cl(g5)
    pt = {}
    grads = train.backbone_backward(feats, c3d, g4d, g5d, parts=pt)
    assert tuple(grads) == train.BACKBONE_PARAMS and all(q.grad is None for q in feats.parameters())
    n, h, w = pic
    assert tuple(pt["x13"].shape) == (n, BK.down(h), BK.down(w), 96) and tuple(pt["x17"].shape) == (n, BK.down(BK.down(h)), BK.down(BK.down(w)), 320)
    assert torch.equal(_bits(pt["g17"]), _bits(nhwc(g5d)))
    tag = "chain %s" % ids3(pic)
    worst_far = {}
    for i in range(BK.END - 1, BK.FIRST - 1, -1):
        cfg = BK.FEATURES[i]
        p = X.fold_module(feats[i].cpu())
        feats[i].to(DEV)
        x, go = pt["x%d" % (i - 1)], pt["g%d" % i]
        parts = {k: pt["%s%d" % (k, i)] for k in ("e", "d", "gd", "ga")}
        gx = nchw(pt["g%d" % (i - 1)]) if i > BK.FIRST else None
        res = nhwc(g4d) if i == BK.C4 + 1 else None
        want = _stage_check(p, cfg, x, go, parts, {k: grads["%d.%s" % (i, k)] for k in BK.NAMES}, gx, "%s block %d" % (tag, i), res=res)
        # the block's output, recomputed: the float64 forward of the device's own input (the projection GEMM of hid inputs + the residual)
        x64 = nchw(c64(x))
        d64 = nchw(c64(parts["d"]))
        o = F.conv2d(d64, p["w3"]) * X._v(p["s3"]) + X._v(p["b3"])
        oa = F.conv2d(d64.abs(), p["w3"].abs()) * X._v(p["s3"].abs()) + X._v(p["b3"].abs())
        bo = rtol("f32", cfg[1]) * oa + EPS * 2 * o.abs()
        if cfg[4]:
            o, bo = o + x64, bo + EPS * (x64.abs() + (o + x64).abs())
        _check(nchw(pt["x%d" % i]), o, bo + 1e-300, "%s x%d" % (tag, i))
        if i == BK.C4 + 1:                                                # g_c4 left out of block 14's grad_x is rejected
            pt64 = {k: nchw(c64(parts[k])) for k in parts}
            wrong = BK.block_stage(p, cfg, x64, nchw(c64(go)), pt64, res=nchw(c64(res)), variant="no_g_c4")
            worst_far["no_g_c4"] = float(((c64(gx) - wrong["grad_x"][0]).abs() / want["grad_x"][1].clamp_min(1e-300)).max())
    assert worst_far["no_g_c4"] > 1.0
    # the whole chain against float64 autograd of features[7:18].  On pictures of 24 to 70 pixels an fp32 forward decides a
    # handful of the 10 blocks' ReLU6 masks differently from float64, and ONE flipped mask moves every gradient below it by
    # about 1 / sqrt(pixels * channels), 0.7 % at 1/32 scale (measured without forcing: 1.6e-2 at block 8): a bound a chain this
    # deep cannot keep.  So autograd takes the derivatives of the ReLU6s from the device's stored e and d, as every
    # teacher-forced test does (the values stay float64's own), and the plain comparison is printed only.
    Q64 = {i: BR.to64(q) for i, q in Q.items()}
    t64 = [torch.as_tensor(t).double() for t in (c3, g4, g5)]
    masks = {i: tuple(X.m6(nchw(c64(pt["%s%d" % (k, i)]))).double() for k in ("e", "d")) for i in range(BK.FIRST, BK.END)}
    auto = BK.chain_autograd(Q64, *t64, masks=masks)
    free = BK.chain_autograd(Q64, *t64)
    for k in train.BACKBONE_PARAMS:
        print("%s %s against autograd with float64's own masks: %.3e" % (tag, k, float((c64(grads[k]) - free[k]).norm() / free[k].norm())))
        _loose(grads[k], auto[k], "%s %s against autograd" % (tag, k))
    xs = BK.chain_forward({i: BR.fold(q) for i, q in Q64.items()}, torch.as_tensor(c3).double())
    for i in (BK.C4, BK.END - 1):
        _loose(nchw(pt["x%d" % i]), xs[i], "%s x%d against float64" % (tag, i), tol=1e-4)
    # the same bits twice; accumulate doubles
    again = train.backbone_backward(feats, c3d, g4d, g5d)
    assert all(torch.equal(_bits(grads[k]), _bits(again[k])) for k in grads)
    train.backbone_backward(feats, c3d, g4d, g5d, grads=again, accumulate=True)
    for k in grads:
        _check(again[k], 2 * grads[k].double(), 4 * U * grads[k].double().abs() + 1e-300, "%s accumulate %s" % (tag, k))
    with pytest.raises(RuntimeError, match="g_c4"):
        train.backbone_backward(feats, c3d, g4d[:, :, :1], g5d)


# ------------------------------------------------------------------------------------------------ 5. the step and the drivers
H_, W_, T_ = 72, 224, 4
BIAS = {"b111": [1, 1, 1], "b000": [0, 0, 0]}


@lru_cache(maxsize=None)
def _step_inputs():
    n = 2 * T_
    x = torch.from_numpy(synth.normalize_frames(synth.synth_frames_u8(n, H_, W_, 3))).to(DEV)
    cb = [torch.from_numpy(synth.gauss_priors(n, H_ // 8, W_ // 8)).to(DEV), torch.from_numpy(synth.ob_priors(n, H_ // 8, W_ // 8, seed=3)).to(DEV)]
    loc = synth.synth_fix_points(n, 90, 280, 12, 4)
    fmap = np.rint(synth.synth_fix_maps(loc, 6.0) * 255).astype(np.uint8)
    y, has = ops.prepare_gaze(torch.from_numpy(fmap).to(DEV), torch.from_numpy(loc).to(DEV), H_ // 8, W_ // 8)
    assert bool(has.all())
    return x, cb, y


def _model(kind="b111"):
    from iip_uavsal_saliency_amd import UAVSal
    m = UAVSal(time_dims=T_, bias_type=BIAS[kind])
    synth.load_synth_weights(m, 0)
    with torch.no_grad():                                       # running statistics that are not the initial 0 and 1
        g = torch.Generator().manual_seed(11)
        for holder in [m.st_layer] + train.srf_head(m):
            for mod in holder.modules():
                if isinstance(mod, torch.nn.BatchNorm2d):
                    mod.running_mean.add_(0.05 * torch.randn(mod.running_mean.shape, generator=g))
                    mod.running_var.mul_(1.0 + 0.2 * torch.rand(mod.running_var.shape, generator=g))
    return m.to(DEV).eval()


def _kw(m, backbone=True):
    kw = dict(decoder=True, fuse=True, st=True, srf=True)
    if backbone:
        kw["backbone"] = True
    if m.num_cb:
        kw.update(fust=True, ctx=True)
        if train.prior_nets(m):
            kw.update(nets=True)
    return kw


def _names():
    return ["sfnet.features.features." + n for n in train.BACKBONE_PARAMS]


def _stats(m):
    return [b.detach().clone() for b in m.buffers()]


@pytest.mark.parametrize("kind", list(BIAS))
def test_recurrence_step_with_the_backbone(kind):
    m = _model(kind)
    x, cb, y = _step_inputs()
    names = _names()
    assert len(names) == 90
    stats = _stats(m)
    loss, out, st = train.recurrence_step(m, x, cb, None, y, **_kw(m))
    taps = {}
    m(x, cb, None, taps=taps)
    ref_out, ref_st = m(x, cb, None)
    assert tuple(taps["c3"].shape[2:]) == (9, 28) and tuple(taps["c4"].shape[2:]) == (5, 14) and tuple(taps["c5"].shape[2:]) == (3, 7)
    assert torch.equal(out, ref_out) and torch.equal(st[0], ref_st[0]) and loss.item() == losses.loss_fu(ref_out, y).item()
    params = dict(m.named_parameters())
    plain = _model(kind)
    train.recurrence_step(plain, x, cb, None, y, **_kw(plain, backbone=False))
    earlier = sorted(k for k, p in plain.named_parameters() if p.grad is not None)
    assert not any(k.startswith("sfnet.features.") for k in earlier)
    assert sorted(k for k, p in params.items() if p.grad is not None) == sorted(earlier + names)      # features[0..7] receive nothing
    g1 = {k: params[k].grad.clone() for k in earlier + names}
    assert all(torch.isfinite(v).all() and float(v.abs().max()) > 0 and v.is_contiguous() for v in g1.values())
    pp = dict(plain.named_parameters())
    assert all(torch.equal(_bits(g1[k]), _bits(pp[k].grad)) for k in earlier)             # every earlier stage: the same bits
    # the recomputed x13 / x17 against the taps: the rounding between fused and unfused forward launches
    pt = {}
    feats = m.sfnet.features.features
    train.backbone_backward(feats, taps["c3"], torch.zeros_like(taps["c4"]), torch.zeros_like(taps["c5"]), parts=pt)
    _loose(nchw(pt["x13"]), c64(taps["c4"]), "%s recomputed x13 against the c4 tap" % kind, tol=1e-4)
    _loose(nchw(pt["x17"]), c64(taps["c5"]), "%s recomputed x17 against the c5 tap" % kind, tol=1e-4)
    engines = {k: id(e) for k, e in m._engines.items()}
    again = _model(kind)
    train.recurrence_step(again, x, cb, None, y, **_kw(again))
    pa = dict(again.named_parameters())
    assert all(torch.equal(_bits(g1[k]), _bits(pa[k].grad)) for k in g1)                  # identical bits over two calls
    train.recurrence_step(m, x, cb, None, y, **_kw(m))                                    # .grad += as loss.backward() would
    for k in names:
        _check(params[k].grad, 2 * g1[k].double(), 4 * U * g1[k].double().abs() + 1e-300, "second call doubles %s" % k)
    assert all(torch.equal(a, b) for a, b in zip(stats, _stats(m)))
    # the directional derivative along the normalised backbone gradient against the central difference of the GPU forward
    # (the plumbing check of tests/test_train_srf_gpu.py, with its 10 % and for its reason).  The step is a QUARTER of that
    # test's 2e-2 / |grad|: the loss is only piecewise smooth in these weights (the ReLU6 kinks of ten blocks and of the head
    # behind them), and the central difference's own error falls about linearly with the step.  Measured at b000, fd / <grad, D>
    # at the SRF step and its halves: 0.898, 0.937, 0.960, 0.976, 0.988 (b111: 0.991, 0.994, 0.997); at the SRF step the
    # reference's own error alone is the whole margin.  The loss still moves by 5e-3 of about 16, far above fp32's resolution.
    blocks = train.backbone_blocks(m)
    with torch.no_grad():
        norm = SF.norm2([g1[k] for k in names])
        w0 = {k: params[k].detach().clone() for k in names}
        s = 5e-3 / norm
        vals = []
        for sign in (1.0, -1.0):
            for k in names:
                params[k].copy_(w0[k] + sign * s * g1[k] / norm)
            assert m.refresh_weights(*blocks) > 0
            vals.append(losses.loss_fu(m(x, cb, None)[0], y).item())
        for k in names:
            params[k].copy_(w0[k])
        m.refresh_weights(*blocks)
    fd = (vals[0] - vals[1]) / (2 * s)
    print("%s: backbone directional derivative: finite difference %.6e, <grad, D> %.6e, step %.3e" % (kind, fd, norm, s))
    assert abs(fd - norm) <= 0.10 * abs(norm)
    assert torch.equal(m(x, cb, None)[0], ref_out)                                        # the restored weights give the same bits
    assert {k: id(e) for k, e in m._engines.items()} == engines                           # no plan rebuilt


def _trained(m):
    mods = [m.rnn, m.conv_out_st, m.fucbst_layer, m.fust_layer, m.fucb_layer, m.cxt_cb_prior, *train.prior_nets(m).values(), m.st_layer,
            *train.srf_head(m), *train.backbone_blocks(m)]
    return mods, [p for mod in mods for p in mod.parameters()]


@pytest.mark.parametrize("fuse_blocks", [True, False])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_adam_steps_over_nine_stages_keep_the_plans(device, fuse_blocks):
    """Two Adam steps over all nine stages, with host and with device refresh, the backbone blocks as fused entries and as
    unfused launches.  With device refresh `model.winograd = False`, for the reason test_adam_steps_over_eight_stages_keep_the_plans
    gives: the device repack makes the Winograd filter transforms within one fp32 ulp, so with Winograd in the plan nothing behind
    `conv_last` is bit-comparable with a fresh model's host pack."""
    from iip_uavsal_saliency_amd import UAVSal
    x, cb, y = _step_inputs()
    m = _model()
    m.fuse_blocks = fuse_blocks
    m.winograd = not device
    mods, ps = _trained(m)
    opt = torch.optim.Adam(ps, lr=1e-4, betas=(0.9, 0.999), weight_decay=5e-5)
    b0 = [p.detach().clone() for mod in train.backbone_blocks(m) for p in mod.parameters()]
    before = m(x, cb, None)[0]
    first = None
    for _ in range(2):
        opt.zero_grad()
        loss, _, _ = train.recurrence_step(m, x, cb, None, y, **_kw(m))
        first = loss.item() if first is None else first
        engines = {k: id(e) for k, e in m._engines.items()}
        opt.step()
        assert m.refresh_weights(*mods, device=device) > 0
        after = m(x, cb, None)[0]
        assert {k: id(e) for k, e in m._engines.items()} == engines                       # the same engine objects
    last = losses.loss_fu(after, y).item()
    print("loss_fu on the group: %.6f before, %.6f after two Adam steps over nine stages (device=%r, fuse_blocks=%r)" % (first, last, device, fuse_blocks))
    assert last < first and not torch.equal(before, after)
    assert all(not torch.equal(a, b) for a, b in zip(b0, (p for mod in train.backbone_blocks(m) for p in mod.parameters())))      # the backbone moved
    fresh = UAVSal(time_dims=T_)
    fresh.load_state_dict(m.state_dict())
    fresh = fresh.to(DEV).eval()
    fresh.fuse_blocks, fresh.winograd = fuse_blocks, m.winograd
    taps, ftaps = {}, {}
    got, got_st = m(x, cb, None, taps=taps)
    want, want_st = fresh(x, cb, None, taps=ftaps)
    for k in ("c3", "c4", "c5", "sfnet", "prefuse"):
        assert torch.equal(taps[k], ftaps[k]), k
    assert torch.equal(got, want) and torch.equal(got_st[0], want_st[0])


def test_finetune_video_with_the_backbone_stage_is_the_manual_loop():
    from iip_uavsal_saliency_amd.stream import finetune_video
    n = 2 * T_ * 2
    frames = torch.from_numpy(synth.synth_frames_u8(n, H_, W_, 2)).to(DEV)
    gp = torch.from_numpy(synth.gauss_priors(1, H_ // 8, W_ // 8)[0]).to(DEV)
    op_ = torch.from_numpy(synth.ob_priors(1, H_ // 8, W_ // 8)[0]).to(DEV)
    loc = synth.synth_fix_points(n, 90, 280, 12, 9)
    fmap = np.rint(synth.synth_fix_maps(loc, 6.0) * 255).astype(np.uint8)
    fix_map, fix_loc = torch.from_numpy(fmap).to(DEV), torch.from_numpy(loc).to(DEV)
    stages = ("rnn", "decoder", "fuse", "fust", "ctx", "nets", "st", "srf", "backbone")

    def make():
        m = _model()
        return m, torch.optim.Adam(_trained(m)[1], lr=1e-4, betas=(0.9, 0.999), weight_decay=5e-5)
    m, opt = make()
    seen = []
    real = train.recurrence_step

    def spy(model, x, cb, state, y, criterion, **kw):
        assert kw == {s: True for s in stages[1:]}
        seen.append((x.clone(), cb, y.clone()))
        return real(model, x, cb, state, y, criterion, **kw)
    train.recurrence_step = spy
    try:
        res = finetune_video(m, frames, gp, op_, fix_map, fix_loc, opt, batch_size=2, stages=stages)
    finally:
        train.recurrence_step = real
    assert res["groups_run"] == 2 and len(seen) == 2
    m2, opt2 = make()
    state, manual = None, []
    for x, cb, y in seen:
        opt2.zero_grad()
        loss, _, state = train.recurrence_step(m2, x, cb, state, y, **{s: True for s in stages[1:]})
        opt2.step()
        m2.refresh_weights(*_trained(m2)[0])
        manual.append(loss.item())
    assert [float(v) for v in res["losses"].tolist()] == manual
    w0 = _model()
    assert not torch.equal(m.sfnet.features.features[12].conv[2].weight.detach(), w0.sfnet.features.features[12].conv[2].weight.detach())
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(m.parameters(), m2.parameters()))


def test_backbone_without_its_preconditions_raises_by_name():
    x, cb, y = _step_inputs()
    m = _model()
    with pytest.raises(RuntimeError, match="backbone=True needs srf=True"):
        train.recurrence_step(m, x, cb, None, y, decoder=True, fuse=True, fust=True, st=True, backbone=True)
    assert all(p.grad is None for p in m.parameters())
