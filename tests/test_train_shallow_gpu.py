"""The backward of the shallow backbone blocks (MobileNetV2 features[2:8]) on the MI355X against the float64 restatement of
tests/shallow_ref64.py: the skinny weight-gradient GEMM (uavsal_skinny_wgrad, train.skinny_wgrad) within the worst-case bound
derived from its partition -- operands as channel slices between NaN columns, results between NaN guards, the same bits
twice --, the channel sums and the finalise at hidden widths 96 and 144 (the Ch % 16 opt-in),
train.block_param_grads(shallow=True) teacher-forced / train.block_backward(shallow=True) stage by stage at the five block
shapes, the two new tap gradients (g_c3 of the head, g_x7 of the deep backbone), train.shallow_backward stage by stage,
recurrence_step(shallow=True), the in-place refresh of the transposed-layout fused entries on the host and on the device, and
the driver -- in the manner of tests/test_train_backbone_gpu.py, whose docstring says why the walks are tested stage by stage."""
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
import shallow_ref64 as SH
import srf_ref64 as SF
from plan_ref64 import EPS, rtol

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = SH.U
NAN = float("nan")


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


def _fenced(t, pad=4):
    """An NHWC tensor as a channel slice between NaN columns."""
    whole = torch.full(t.shape[:-1] + (t.shape[-1] + 2 * pad,), NAN, dtype=t.dtype, device=t.device)
    whole[..., pad:-pad] = t
    return whole[..., pad:-pad]


def _loose(got, want, what, tol=2e-3):
    got, want = got.detach().double().cpu(), want.double().cpu()
    err = float((got - want).norm()) / max(float(want.norm()), 1e-300)
    print("%s: relative error in norm %.3e" % (what, err))
    assert err <= tol, (what, err)


def _cl(a):
    return torch.as_tensor(a).to(DEV).float().contiguous(memory_format=torch.channels_last)


c64 = lambda t: t.detach().double().cpu()                                 # noqa: E731
nchw = lambda t: t.permute(0, 3, 1, 2)                                    # noqa: E731
nhwc = lambda t: t.permute(0, 2, 3, 1)                                    # noqa: E731
ids3 = lambda p: "%dx%dx%d" % tuple(p)                                    # noqa: E731


def _shares(K, M, N):
    d = _lib.SkinnyWgradDesc()
    d.K, d.M, d.N = K, M, N
    return _lib.load().uavsal_skinny_wgrad_shares(C.byref(d))


def _boxes(M, N):
    box = torch.full(((M + 2) * N,), NAN, dtype=torch.float32, device=DEV)
    rowdot = torch.full((M + 2,), NAN, dtype=torch.float64, device=DEV)
    return box, box[N:(M + 1) * N].view(M, N), rowdot


def _guards_hold(box, rowdot, M, N):
    return bool(torch.isnan(box[:N]).all()) and bool(torch.isnan(box[(M + 1) * N:]).all()) and bool(torch.isnan(rowdot[[0, M + 1]]).all())


@pytest.mark.parametrize("pic", SH.GEMM_K, ids=ids3)
@pytest.mark.parametrize("M,N", SH.GEMM)
def test_skinny_wgrad_against_float64(M, N, pic):
    a, b, w, s, pad = (torch.from_numpy(t) for t in SH.gemm_inputs(M, N, pic))
    K = pic[0] * pic[1] * pic[2]
    G, eG = SH.skinny_ref(a.double(), b.double())
    A = a.double().reshape(K, M).abs().T @ b.double().reshape(K, N).abs()
    av, bv = _fenced(a.to(DEV)), _fenced(b.to(DEV))                       # the neighbouring channels hold NaN
    wd, sd = w.to(DEV), s.to(DEV)
    box, out, rowdot = _boxes(M, N)
    span, shares, spans = SH.partition(K)
    assert _shares(K, M, N) == shares
    if K == 2760:
        assert shares == 22 and spans[-1][1] - spans[-1][0] == 72         # more than one share is real, the last one ragged
    else:
        assert shares == 1 and K < SH.CHAIN and K % 16                    # under a chain, no multiple of the K step
    tag = "skinny_wgrad %dx%d K=%d (%d shares)" % (M, N, K, shares)
    train.skinny_wgrad(av, bv, out=out, row_scale=sd, w=wd, rowdot=rowdot[1:M + 1])
    s64 = s.double().view(-1, 1)
    _check(out, s64 * G, s64 * (eG + U * A) + 1e-300, tag)
    _check(rowdot[1:M + 1], (w.double() * G).sum(1), (w.double().abs() * eG).sum(1) + 1e-300, tag + " rowdot")
    assert _guards_hold(box, rowdot, M, N)
    first, dot = out.clone(), rowdot.clone()
    train.skinny_wgrad(av, bv, out=out, row_scale=sd, w=wd, rowdot=rowdot[1:M + 1])
    assert torch.equal(_bits(out), _bits(first)) and torch.equal(rowdot[1:M + 1], dot[1:M + 1])      # the same bits twice
    plain = train.skinny_wgrad(a.to(DEV), b.to(DEV))                      # dense operands, no scale: the same sums
    _check(plain, G, eG + 1e-300, tag + " unscaled")
    train.skinny_wgrad(av, bv, out=out, row_scale=sd, accumulate=True)
    _check(out, 2 * first.double(), 4 * U * first.double().abs() + 1e-300, tag + " accumulate")
    assert _guards_hold(box, rowdot, M, N)
    with pytest.raises(RuntimeError, match="ESHAPE|shape|rejected"):      # the only way in: pix_gemm refuses the shape, as it always did
        train.pix_gemm(a.to(DEV), b.to(DEV), tails32=True)
    for v in SH.WRONG:
        wrong = SH.skinny_ref(a.double(), b.double(), v, pad.double())[0]
        if not torch.equal(wrong, G):
            assert float(((c64(plain) - wrong).abs() / eG).max()) > 1.0, v


@pytest.mark.parametrize("M,N", SH.GEMM_REFUSED)
def test_skinny_wgrad_refuses_by_name(M, N):
    a, b = torch.zeros(1, 5, 7, M, device=DEV), torch.zeros(1, 5, 7, N, device=DEV)
    assert _shares(35, M, N) == 0
    with pytest.raises(RuntimeError, match="uavsal_skinny_wgrad rejected its arguments"):
        train.skinny_wgrad(a, b)


def test_skinny_wgrad_where_a_share_holds_two_chains():
    """96 x 16 over K_CHAINS = 1,049,563 pixels (block 2's G1 at 20 frames of 360 x 640 has 1,152,000): 912 shares of 1152
    pixels -- a chain of 1024 and one of 128 --, the last of 91.  Operands of one sign, so that the worst-case bound is tight
    enough to see a dropped share (tests/test_train_shallow_cpu.py); the float64 reference is formed on the device in slices."""
    M, N, K = 96, 16, SH.K_CHAINS
    span, shares, spans = SH.partition(K)
    assert (span, shares) == (1152, 912) == (span, _shares(K, M, N)) and SH.chains(K) == (1024, 2) and spans[-1][1] - spans[-1][0] == 91
    gen = torch.Generator(device=DEV).manual_seed(7)
    buf = torch.full((1, 1, K, M + N + 12), NAN, dtype=torch.float32, device=DEV)      # both operands in ONE buffer, NaN between
    a, b = buf[..., 4:4 + M], buf[..., 8 + M:8 + M + N]
    a.copy_(torch.rand(a.shape, generator=gen, device=DEV) * 1e-2)
    b.copy_(torch.rand(b.shape, generator=gen, device=DEV))
    G = torch.zeros(M, N, dtype=torch.float64, device=DEV)
    for p in range(0, K, 1 << 16):
        G += a[0, 0, p:p + (1 << 16)].double().T @ b[0, 0, p:p + (1 << 16)].double()
    L, c = SH.chains(K)
    eG = (L + c + 2) * U * G                                               # all positive: G is its own absolute-value sum
    box, out, rowdot = _boxes(M, N)
    w = torch.rand(M, N, generator=gen, device=DEV)
    train.skinny_wgrad(a, b, out=out, w=w, rowdot=rowdot[1:M + 1])
    _check(out, G, eG + U * G, "skinny_wgrad 96x16 K=%d (%d shares of 2 chains)" % (K, shares))
    _check(rowdot[1:M + 1], (w.double() * G).sum(1), (w.double() * eG).sum(1), "its rowdot")
    assert _guards_hold(box, rowdot, M, N)
    first = out.clone()
    train.skinny_wgrad(a, b, out=out, w=w, rowdot=rowdot[1:M + 1])
    assert torch.equal(_bits(out), _bits(first))
    p0, p1 = spans[-2]                                                     # a kernel that drops a whole share is far
    wrong = G - a[0, 0, p0:p1].double().T @ b[0, 0, p0:p1].double()
    assert float(((out.double() - wrong).abs() / eG).min()) > 3.0


# ------------------------------------------------------------------------------------------------ 2. the channel sums
@pytest.mark.parametrize("pic", SH.SUMS_PICTURES, ids=ids3)
@pytest.mark.parametrize("stride", (1, 2))
@pytest.mark.parametrize("Ch", SH.SUMS_CH)
def test_sums_with_the_ch16_opt_in(Ch, stride, pic):
    Co = 24
    t64 = [torch.as_tensor(v).double() for v in SH.sums_case(pic, Ch, Co, stride)]
    S, b = SH.sums_ref(*t64, stride)
    gd, d, e, ga = (nhwc(v.float().to(DEV)).contiguous() for v in t64[:4])
    go = _fenced(nhwc(t64[4].float().to(DEV)).contiguous())               # a channel slice between NaN columns
    fn = train.ir_sums if stride == 1 else train.ir_sums_s2
    with pytest.raises(RuntimeError, match="ESHAPE|shape|rejected"):      # without the opt-in: refused, as it always was
        fn(gd, d, e, ga, go)
    ws, slabs = fn(gd, d, e, ga, go, ch16=True)
    if pic[1] > 7:
        assert slabs > 1
    tot = ws.view(slabs, _lib.IR_NSUM * Ch + Co).sum(0)
    tag = "sums Ch=%d stride %d %s (%d slabs)" % (Ch, stride, ids3(pic), slabs)
    _check(tot[:Ch], S["S2"], b["S2"] + 1e-300, tag + " S2")
    _check(tot[Ch:10 * Ch].view(9, Ch).T.reshape(Ch, 3, 3), S["Gd"], b["Gd"] + 1e-300, tag + " Gd")
    _check(tot[10 * Ch:11 * Ch], S["S1"], b["S1"] + 1e-300, tag + " S1")
    _check(tot[11 * Ch:], S["S3"], b["S3"] + 1e-300, tag + " S3")
    again, _ = fn(gd, d, e, ga, go, ch16=True)
    assert torch.equal(ws, again)                                         # the same bits twice
    for v in ("last_group",) + (("s2_anchor",) if stride == 2 else ()):
        W, _ = SH.sums_ref(*t64, stride, variant=v)
        got = {"S2": tot[:Ch], "Gd": tot[Ch:10 * Ch].view(9, Ch).T.reshape(Ch, 3, 3), "S1": tot[10 * Ch:11 * Ch]}
        assert max(float(((c64(got[k]) - W[k]).abs() / b[k].clamp_min(1e-300)).max()) for k in got) > 1.0, v


def test_sums_keep_their_bits_with_the_opt_in_where_they_always_ran():
    t64 = [torch.as_tensor(v).double() for v in SH.sums_case((2, 5, 7), 192, 32, 2)]
    gd, d, e, ga, go = (nhwc(v.float().to(DEV)).contiguous() for v in t64)
    a, b = train.ir_sums_s2(gd, d, e, ga, go), train.ir_sums_s2(gd, d, e, ga, go, ch16=True)
    assert a[1] == b[1] and torch.equal(a[0], b[0])


# ------------------------------------------------------------------------------------------------ 3. one block
@lru_cache(maxsize=None)
def _block_case(name, pic):
    cfg = SH.BLOCKS[name]
    x, q, go = SH.block_case(name, pic)
    block = SH.make_block(cfg, q, model_feature.InvertedResidual).to(DEV)
    p = BR.fold(BR.to64(q))
    x64, go64 = torch.as_tensor(x).double(), torch.as_tensor(go).double()
    return cfg, block, p, x64, go64, _cl(x), _cl(go)


def _dense(t64, keep_masks=False):
    t = BR.teacher_round(t64) if keep_masks else t64.float()
    return nhwc(t.to(DEV)).contiguous()


@pytest.mark.parametrize("pic", SH.PICTURES, ids=ids3)
@pytest.mark.parametrize("name", list(SH.BLOCKS))
def test_block_param_grads_teacher_forced(name, pic):
    cfg, block, p, x64, go64, x, go = _block_case(name, pic)
    pt = MP.block_parts(p, x64, go64, cfg[3])
    e, d, gd, ga = _dense(pt["e"], True), _dense(pt["d"], True), _dense(pt["gd"]), _dense(pt["ga"])
    got = train.block_param_grads(block, x, e, d, go, gd=gd, ga=ga, shallow=True)
    want, bound = MP.grads_from_parts(p, x64, pt["e"], pt["d"], pt["gd"], pt["ga"], go64, cfg[3], bounds=True)
    for k in SH.NAMES:
        _check(got[k], want[k], bound[k] + 1e-300, "block %s %s teacher-forced %s" % (name, ids3(pic), k))
    assert all(q.grad is None for q in block.parameters())
    # ... and against the reference's own dwBlock under float64 autograd (tests/golden/shallow_*.npz), within the same bounds
    z = np.load(os.path.join(GOLDEN, SH.golden_name(name, pic) + ".npz"))
    assert str(z["digest"]) == SH.golden_digest(*SH.block_case(name, pic))
    mine, bnd = SH.golden_pack({k: c64(v) for k, v in got.items()}), SH.golden_pack({k: v for k, v in bound.items()})
    for k in mine:
        if not k.endswith("_sum") and not k.endswith("_l2"):
            _check(torch.as_tensor(mine[k]), torch.as_tensor(z[k]), torch.as_tensor(bnd[k]) + 1e-300, "block %s %s golden %s" % (name, ids3(pic), k))
    again = train.block_param_grads(block, x, e, d, go, gd=gd, ga=ga, shallow=True)
    assert all(torch.equal(_bits(got[k]), _bits(again[k])) for k in SH.NAMES)
    # without the keyword: refused, as it always was (`backbone=True` alone always took 32 -> 192 -> 32 / 64: multiples of 32)
    for kw in ({},) + (({"backbone": True},) if cfg[0] % 32 or cfg[1] % 64 else ()):
        with pytest.raises(RuntimeError, match="Cout|Cin|hidden"):
            train.block_param_grads(block, x, e, d, go, gd=gd, ga=ga, **kw)
        with pytest.raises(RuntimeError, match="expand conv|Cout|Cin|hidden"):
            train.block_backward(block, x, go, **kw)


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
    want = SH.block_stage(p, cfg, x64, go64, pt64, res=None if res is None else nchw(c64(res)))
    f, err_e, err_d = _forward_bounds(p, x64, cfg[3])
    _check(nchw(pt["e"]), f["e"], err_e + 1e-300, tag + " e")
    d_pre = F.conv2d(pt64["e"], p["wd"], padding=1, stride=cfg[3], groups=p["wd"].shape[0]) * X._v(p["s2"]) + X._v(p["b2"])
    d_abs = F.conv2d(pt64["e"].abs(), p["wd"].abs(), padding=1, stride=cfg[3], groups=p["wd"].shape[0]) * X._v(p["s2"].abs()) + X._v(p["b2"].abs())
    _check(nchw(pt["d"]), d_pre.clamp(0, 6), rtol("f32", 9) * d_abs + EPS * 2 * d_pre.abs() + 1e-300, tag + " d")
    _check(nchw(pt["gd"]), *want["gd"], tag + " gd")
    _check(nchw(pt["ga"]), *want["ga"], tag + " ga")
    if gx is not None:
        _check(gx, *want["grad_x"], tag + " grad_x")
    for k in SH.NAMES:
        _check(grads[k], want[k][0], want[k][1] + 1e-300, "%s %s" % (tag, k))
    return want


@pytest.mark.parametrize("pic", SH.PICTURES, ids=ids3)
@pytest.mark.parametrize("name", list(SH.BLOCKS))
def test_block_backward_end_to_end(name, pic):
    cfg, block, p, x64, go64, x, go = _block_case(name, pic)
    pt = {}
    gx, grads = train.block_backward(block, x, go, parts=pt, shallow=True)
    n, H, W = pic
    assert tuple(gx.shape) == (n, cfg[0], H, W) and tuple(pt["d"].shape) == (n, (H - 1) // cfg[3] + 1, (W - 1) // cfg[3] + 1, cfg[1])
    tag = "block %s %s" % (name, ids3(pic))
    want = _stage_check(p, cfg, nhwc(x), nhwc(go), pt, grads, gx, tag)
    # the whole block against float64 from its inputs alone: to what an fp32 forward allows
    auto = MP.autograd_grads(BR.to64(SH.block_case(name, pic)[1]), x64, go64, cfg[3], cfg[4])
    for k in SH.NAMES:
        _loose(grads[k], auto[k], "%s %s against autograd" % (tag, k))
    _loose(gx, X.input_grad_autograd(p, x64, go64, cfg[3], cfg[4]), tag + " grad_x against autograd")
    z = np.load(os.path.join(GOLDEN, SH.golden_name(name, pic) + ".npz"))                 # the reference's own block
    _loose(gx, torch.as_tensor(z["grad_x"]), tag + " grad_x against the reference golden")
    for k, v in SH.golden_pack({k: c64(v) for k, v in grads.items()}).items():
        if not k.endswith("_sum"):
            _loose(torch.as_tensor(v), torch.as_tensor(z[k]), "%s %s against the reference golden" % (tag, k))
    # wrong walks are rejected by the stage bounds
    pt64 = {k: nchw(c64(pt[k])) for k in ("e", "d", "gd", "ga")}
    if cfg[3] == 2:
        wrong = SH.block_stage(p, cfg, x64, go64, pt64, variant="s2_anchor")
        assert float(((nchw(c64(pt["ga"])) - wrong["ga"][0]).abs() / want["ga"][1].clamp_min(1e-300)).max()) > 1.0
    if cfg[4]:
        wrong = SH.block_stage(p, cfg, x64, go64, pt64, variant="no_residual")
        assert float(((c64(gx) - wrong["grad_x"][0]).abs() / want["grad_x"][1].clamp_min(1e-300)).max()) > 1.0
    # the same bits twice; no input gradient on request; accumulate doubles
    gx2, again = train.block_backward(block, x, go, shallow=True)
    assert torch.equal(_bits(gx), _bits(gx2)) and all(torch.equal(_bits(grads[k]), _bits(again[k])) for k in SH.NAMES)
    none, third = train.block_backward(block, x, go, need_x_grad=False, grads=again, accumulate=True, shallow=True)
    assert none is None
    for k in SH.NAMES:
        _check(third[k], 2 * grads[k].double(), 4 * U * grads[k].double().abs() + 1e-300, "%s accumulate %s" % (tag, k))


# ------------------------------------------------------------------------------------------------ 4. the two new tap gradients
@lru_cache(maxsize=None)
def _head():
    return SF.calibrate(uavsal_srfnet_aspp("mobilenet_v2")).to(DEV).eval()


@pytest.mark.parametrize("case", SF.GOLDEN_CASES, ids=SF.golden_name)
def test_srf_head_backward_c3_gradient(case):
    c3, c4, c5, go = (_cl(t) for t in SF.golden_inputs(case))
    sf = _head()
    tmp = {}
    train.srf_head_backward(sf, c3, c4, c5, torch.zeros_like(go), go, parts=tmp)
    cache = WeightCache(torch.device(DEV), {})
    y = nchw(train._conv(_lib.load(), cache, tmp["cat"], sf.conv_last[0], 256, 9, bn=sf.conv_last[1], act=_lib.ACT_RELU6))
    plain = train.srf_head_backward(sf, c3, c4, c5, y, go)
    _, p4, p5 = train.srf_head_backward(sf, c3, c4, c5, y, go, need_tap_grads=True)
    pt = {}
    grads, g4, g5, g3 = train.srf_head_backward(sf, c3, c4, c5, y, go, parts=pt, need_tap_grads=True, need_c3_grad=True)
    assert sorted(grads) == sorted(train.SRF_HEAD_PARAMS) and g3.shape == c3.shape
    assert all(torch.equal(_bits(grads[k]), _bits(plain[k])) for k in plain)           # the 42 gradients: the default call's bits
    assert torch.equal(_bits(g4), _bits(p4)) and torch.equal(_bits(g5), _bits(p5))     # g_c4, g_c5: the ninth stage's bits
    only, g3b = train.srf_head_backward(sf, c3, c4, c5, y, go, need_c3_grad=True)      # without the other taps: (grads, g_c3)
    assert torch.equal(_bits(g3), _bits(g3b)) and all(torch.equal(_bits(only[k]), _bits(plain[k])) for k in plain)
    # the one GEMM on the tensors the walk held
    P, B = SF.head_params64(sf)
    Pd = {k: v.detach() for k, v in P.items()}
    n3 = pt["x3"].shape[3]
    g_x3, x3 = nchw(c64(pt["g_cat"][..., -n3:])), nchw(c64(pt["x3"]))
    fold = SF.bn_fold(*SF._bn(Pd, B, "conv_lv3.1"))[0]
    want, bound = BK.sum_terms([(g_x3 * X.m6(x3), Pd["conv_lv3.0.weight"], fold)])
    _check(g3, want, bound + 1e-300, "head %s g_c3" % SF.golden_name(case))
    wrong, _ = BK.sum_terms([(g_x3, Pd["conv_lv3.0.weight"], fold)])                   # the ReLU6 mask of x3 left out is rejected
    assert float(((c64(g3) - wrong).abs() / bound.clamp_min(1e-300)).max()) > 1.0
    t64 = [torch.as_tensor(t).double() for t in SF.golden_inputs(case)]                # the whole head against float64 autograd
    c3r = t64[0].clone().requires_grad_(True)
    (a3,) = torch.autograd.grad(SF.forward64(P, B, c3r, t64[1], t64[2]), [c3r], t64[3])
    _loose(g3, a3, "head g_c3 against autograd")


@pytest.mark.parametrize("pic", BK.PICTURES, ids=ids3)
def test_backbone_backward_input_gradient(pic):
    c3, Q, g4, g5 = BK.chain_case(pic)
    feats = BK.make_features(Q, model_feature.mobilenet_v2_features()).to(DEV)
    c3d, g4d, g5d = _cl(c3), _cl(g4), _cl(g5)
    plain = train.backbone_backward(feats, c3d, g4d, g5d)
    pt = {}
    grads, g7 = train.backbone_backward(feats, c3d, g4d, g5d, parts=pt, need_x_grad=True)
    assert isinstance(plain, dict) and tuple(grads) == train.BACKBONE_PARAMS
    assert all(torch.equal(_bits(grads[k]), _bits(plain[k])) for k in plain)           # the 90 gradients: the default call's bits
    assert tuple(g7.shape) == (pic[0], 64, BK.down(pic[1]), BK.down(pic[2])) and torch.equal(_bits(nhwc(g7)), _bits(pt["g7"]))
    p = X.fold_module(feats[8].cpu())
    feats[8].to(DEV)
    pt64 = {k: nchw(c64(pt["%s8" % k])) for k in ("e", "d", "gd", "ga")}
    want = BK.block_stage(p, BK.FEATURES[8], nchw(c64(pt["x7"])), nchw(c64(pt["g8"])), pt64)
    _check(g7, *want["grad_x"], "chain %s g_x7" % ids3(pic))
    wrong = BK.block_stage(p, BK.FEATURES[8], nchw(c64(pt["x7"])), nchw(c64(pt["g8"])), pt64, variant="no_residual")
    assert float(((c64(g7) - wrong["grad_x"][0]).abs() / want["grad_x"][1].clamp_min(1e-300)).max()) > 1.0


# ------------------------------------------------------------------------------------------------ 5. the walk
@pytest.mark.parametrize("frame", SH.FRAMES, ids=ids3)
def test_shallow_backward_over_the_whole_chain(frame):
    feats = model_feature.mobilenet_v2_features()
    x, Q, g3, g7 = SH.chain_case(frame, feats)
    x0_64, x1_64 = SH.frozen_forward(feats, torch.as_tensor(x))
    feats = BK.make_features(Q, feats).to(DEV)
    xd, g3d, g7d = torch.as_tensor(x).to(DEV), _cl(g3), _cl(g7)
    pt = {}
    grads = train.shallow_backward(feats, xd, g3d, g7d, parts=pt)
    assert tuple(grads) == train.SHALLOW_PARAMS and all(q.grad is None for q in feats.parameters())
    n, H, W = frame
    d = SH.down
    assert tuple(pt["x0"].shape) == (n, d(H), d(W), 32) and tuple(pt["x1"].shape) == (n, d(H), d(W), 16)
    assert tuple(pt["x6"].shape) == (n, d(d(d(H))), d(d(d(W))), 32) == tuple(nhwc(g3d).shape) and tuple(pt["x7"].shape) == tuple(nhwc(g7d).shape)
    assert torch.equal(_bits(pt["g7"]), _bits(nhwc(g7d)))
    _loose(nchw(pt["x0"]), x0_64, "frozen stem against float64", tol=1e-4)
    _loose(nchw(pt["x1"]), x1_64, "frozen features[1] against float64", tol=1e-4)
    tag = "shallow chain %s" % ids3(frame)
    far = {}
    for i in range(SH.END - 1, SH.FIRST - 1, -1):
        cfg = SH.FEATURES[i]
        p = X.fold_module(feats[i].cpu())
        feats[i].to(DEV)
        xin, go = pt["x%d" % (i - 1)], pt["g%d" % i]
        parts = {k: pt["%s%d" % (k, i)] for k in ("e", "d", "gd", "ga")}
        gx = nchw(pt["g%d" % (i - 1)]) if i > SH.FIRST else None
        res = nhwc(g3d) if i == SH.C3 + 1 else None
        want = _stage_check(p, cfg, xin, go, parts, {k: grads["%d.%s" % (i, k)] for k in SH.NAMES}, gx, "%s block %d" % (tag, i), res=res)
        x64, d64 = nchw(c64(xin)), nchw(c64(parts["d"]))                  # the block's output, recomputed
        o = F.conv2d(d64, p["w3"]) * X._v(p["s3"]) + X._v(p["b3"])
        oa = F.conv2d(d64.abs(), p["w3"].abs()) * X._v(p["s3"].abs()) + X._v(p["b3"].abs())
        bo = rtol("f32", cfg[1]) * oa + EPS * 2 * o.abs()
        if cfg[4]:
            o, bo = o + x64, bo + EPS * (x64.abs() + (o + x64).abs())
        _check(nchw(pt["x%d" % i]), o, bo + 1e-300, "%s x%d" % (tag, i))
        pt64 = {k: nchw(c64(parts[k])) for k in parts}
        if i == SH.C3 + 1:                                                # g_c3 left out of block 7's grad_x is rejected
            wrong = SH.block_stage(p, cfg, x64, nchw(c64(go)), pt64, res=nchw(c64(res)), variant="no_g_c4")
            far["no_g_c3"] = float(((c64(gx) - wrong["grad_x"][0]).abs() / want["grad_x"][1].clamp_min(1e-300)).max())
        if cfg[4]:                                                        # ... the residual gradient dropped at block 3 / 5 / 6
            wrong = SH.block_stage(p, cfg, x64, nchw(c64(go)), pt64, variant="no_residual")
            far["no_residual %d" % i] = float(((c64(gx) - wrong["grad_x"][0]).abs() / want["grad_x"][1].clamp_min(1e-300)).max())
        if cfg[3] == 2:                                                   # ... the stride-2 window anchored as on an unpadded grid
            wrong = SH.block_stage(p, cfg, x64, nchw(c64(go)), pt64, res=None if res is None else nchw(c64(res)), variant="s2_anchor")
            far["s2_anchor %d" % i] = float(((nchw(c64(parts["ga"])) - wrong["ga"][0]).abs() / want["ga"][1].clamp_min(1e-300)).max())
    assert len(far) == 7 and min(far.values()) > 1.0, far
    # the whole chain against float64 autograd of features[2:8], the ReLU6 derivatives taken from the device's stored e and d
    # (tests/test_train_backbone_gpu.py says why); the plain comparison is printed only
    Q64 = {i: BR.to64(q) for i, q in Q.items()}
    g3_64, g7_64 = torch.as_tensor(g3).double(), torch.as_tensor(g7).double()
    masks = {i: tuple(X.m6(nchw(c64(pt["%s%d" % (k, i)]))).double() for k in ("e", "d")) for i in range(SH.FIRST, SH.END)}
    auto = SH.chain_autograd(Q64, x1_64, g3_64, g7_64, masks=masks)
    free = SH.chain_autograd(Q64, x1_64, g3_64, g7_64)
    for k in train.SHALLOW_PARAMS:
        print("%s %s against autograd with float64's own masks: %.3e" % (tag, k, float((c64(grads[k]) - free[k]).norm() / free[k].norm())))
        _loose(grads[k], auto[k], "%s %s against autograd" % (tag, k))
    xs = SH.chain_forward({i: BR.fold(q) for i, q in Q64.items()}, x1_64)
    for i in (SH.C3, SH.END - 1):
        _loose(nchw(pt["x%d" % i]), xs[i], "%s x%d against float64" % (tag, i), tol=1e-4)
    again = train.shallow_backward(feats, xd, g3d, g7d)                   # the same bits twice; accumulate doubles
    assert all(torch.equal(_bits(grads[k]), _bits(again[k])) for k in grads)
    train.shallow_backward(feats, xd, g3d, g7d, grads=again, accumulate=True)
    for k in grads:
        _check(again[k], 2 * grads[k].double(), 4 * U * grads[k].double().abs() + 1e-300, "%s accumulate %s" % (tag, k))
    with pytest.raises(RuntimeError, match="g_c3"):
        train.shallow_backward(feats, xd, g3d[:, :, :1], g7d)
    with pytest.raises(RuntimeError, match="g_x7"):
        train.shallow_backward(feats, xd, g3d, g7d[:, :1])


# ------------------------------------------------------------------------------------------------ 6. the step and the drivers
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


def _kw(m, shallow=True):
    kw = dict(decoder=True, fuse=True, st=True, srf=True, backbone=True)
    if shallow:
        kw["shallow"] = True
    if m.num_cb:
        kw.update(fust=True, ctx=True)
        if train.prior_nets(m):
            kw.update(nets=True)
    return kw


def _names():
    return ["sfnet.features.features." + n for n in train.SHALLOW_PARAMS]


@pytest.mark.parametrize("kind", list(BIAS))
def test_recurrence_step_with_the_shallow_backbone(kind):
    m = _model(kind)
    x, cb, y = _step_inputs()
    names = _names()
    assert len(names) == 54
    stats = [b.detach().clone() for b in m.buffers()]
    loss, out, st = train.recurrence_step(m, x, cb, None, y, **_kw(m))
    taps = {}
    m(x, cb, None, taps=taps)
    ref_out, ref_st = m(x, cb, None)
    assert torch.equal(out, ref_out) and torch.equal(st[0], ref_st[0]) and loss.item() == losses.loss_fu(ref_out, y).item()
    params = dict(m.named_parameters())
    plain = _model(kind)
    train.recurrence_step(plain, x, cb, None, y, **_kw(plain, shallow=False))
    earlier = sorted(k for k, p in plain.named_parameters() if p.grad is not None)
    assert not any(k in names for k in earlier)
    assert sorted(k for k, p in params.items() if p.grad is not None) == sorted(earlier + names)
    for i in (0, 1, 18):                                                 # the stem, features[1] and the held last conv receive nothing
        assert all(p.grad is None for p in m.sfnet.features.features[i].parameters())
    g1 = {k: params[k].grad.clone() for k in earlier + names}
    assert all(torch.isfinite(v).all() and float(v.abs().max()) > 0 and v.is_contiguous() for v in g1.values())
    pp = dict(plain.named_parameters())
    assert all(torch.equal(_bits(g1[k]), _bits(pp[k].grad)) for k in earlier)             # every earlier stage: the same bits
    # the recomputed x6 against the c3 tap: the rounding between fused and unfused forward launches
    pt = {}
    feats = m.sfnet.features.features
    g7z = torch.zeros(x.shape[0], 64, taps["c4"].shape[2], taps["c4"].shape[3], device=DEV)
    train.shallow_backward(feats, x, torch.zeros_like(taps["c3"]), g7z, parts=pt)
    _loose(nchw(pt["x6"]), c64(taps["c3"]), "%s recomputed x6 against the c3 tap" % kind, tol=1e-4)
    engines = {k: id(e) for k, e in m._engines.items()}
    again = _model(kind)
    train.recurrence_step(again, x, cb, None, y, **_kw(again))
    pa = dict(again.named_parameters())
    assert all(torch.equal(_bits(g1[k]), _bits(pa[k].grad)) for k in g1)                  # identical bits over two calls
    train.recurrence_step(m, x, cb, None, y, **_kw(m))                                    # .grad += as loss.backward() would
    for k in names:
        _check(params[k].grad, 2 * g1[k].double(), 4 * U * g1[k].double().abs() + 1e-300, "second call doubles %s" % k)
    assert all(torch.equal(a, b) for a, b in zip(stats, [b.detach().clone() for b in m.buffers()]))
    # the directional derivative along the normalised shallow gradient against the central difference of the GPU forward: the
    # ninth stage's step (5e-3 / |grad|) and its 10 % margin (tests/test_train_backbone_gpu.py says where both come from)
    blocks = train.shallow_blocks(m)
    with torch.no_grad():
        norm = SF.norm2([g1[k] for k in names])
        w0 = {k: params[k].detach().clone() for k in names}
        s = 5e-3 / norm
        vals = []
        for sign in (1.0, -1.0):
            for k in names:
                params[k].copy_(w0[k] + sign * s * g1[k] / norm)
            assert m.refresh_weights(*blocks, fused_t=True) > 0
            vals.append(losses.loss_fu(m(x, cb, None)[0], y).item())
        for k in names:
            params[k].copy_(w0[k])
        m.refresh_weights(*blocks, fused_t=True)
    fd = (vals[0] - vals[1]) / (2 * s)
    print("%s: shallow directional derivative: finite difference %.6e, <grad, D> %.6e, step %.3e" % (kind, fd, norm, s))
    assert abs(fd - norm) <= 0.10 * abs(norm)
    assert torch.equal(m(x, cb, None)[0], ref_out)                                        # the restored weights give the same bits
    assert {k: id(e) for k, e in m._engines.items()} == engines                           # no plan rebuilt
    with pytest.raises(NotImplementedError, match="cannot be refreshed in place"):         # without the keyword: as it always was
        m.refresh_weights(*blocks)


def _trained(m):
    mods = [m.rnn, m.conv_out_st, m.fucbst_layer, m.fust_layer, m.fucb_layer, m.cxt_cb_prior, *train.prior_nets(m).values(), m.st_layer,
            *train.srf_head(m), *train.backbone_blocks(m), *train.shallow_blocks(m)]
    return mods, [p for mod in mods for p in mod.parameters()]


def _fused_t_bytes(m):
    """The transposed-layout fused entries of the six shallow blocks that the model's store holds, in block order."""
    store = m._wshared[str(torch.device(DEV))]
    keys = [("fused", id(list(b.conv)[1][0]), False) for b in train.shallow_blocks(m)]
    return [{n: t.detach().cpu().clone() for n, t in store[k].items()} for k in keys if k in store]


@pytest.mark.parametrize("fuse_blocks", [True, False])
def test_adam_steps_over_ten_stages_keep_the_plans(fuse_blocks):
    """Two Adam steps over all ten stages with host and with device refresh, the backbone blocks as fused entries and as unfused
    launches: no plan rebuilt, the forward after the refresh bit-equal to a freshly built model's, and the transposed-layout
    entries of the two refresh paths equal byte for byte.  `model.winograd = False` throughout, for the reason
    tests/test_train_backbone_gpu.py gives (the device repack makes the Winograd transforms within one ulp)."""
    from iip_uavsal_saliency_amd import UAVSal
    x, cb, y = _step_inputs()
    packed = {}
    for device in (False, True):
        m = _model()
        m.fuse_blocks, m.winograd = fuse_blocks, False
        mods, ps = _trained(m)
        opt = torch.optim.Adam(ps, lr=1e-4, betas=(0.9, 0.999), weight_decay=5e-5)
        b0 = [p.detach().clone() for mod in train.shallow_blocks(m) for p in mod.parameters()]
        before = m(x, cb, None)[0]
        first = None
        for _ in range(2):
            opt.zero_grad()
            loss, _, _ = train.recurrence_step(m, x, cb, None, y, **_kw(m))
            first = loss.item() if first is None else first
            engines = {k: id(e) for k, e in m._engines.items()}
            opt.step()
            assert m.refresh_weights(*mods, device=device, fused_t=True) > 0
            after = m(x, cb, None)[0]
            assert {k: id(e) for k, e in m._engines.items()} == engines                   # the same engine objects
        last = losses.loss_fu(after, y).item()
        print("loss_fu on the group: %.6f before, %.6f after two Adam steps over ten stages (device=%r, fuse_blocks=%r)" % (first, last, device, fuse_blocks))
        assert last < first and not torch.equal(before, after)
        assert all(not torch.equal(a, b) for a, b in zip(b0, (p for mod in train.shallow_blocks(m) for p in mod.parameters())))
        fresh = UAVSal(time_dims=T_)
        fresh.load_state_dict(m.state_dict())
        fresh = fresh.to(DEV).eval()
        fresh.fuse_blocks, fresh.winograd = fuse_blocks, False
        taps, ftaps = {}, {}
        got, got_st = m(x, cb, None, taps=taps)
        want, want_st = fresh(x, cb, None, taps=ftaps)
        for k in ("c3", "c4", "c5", "sfnet", "prefuse"):
            assert torch.equal(taps[k], ftaps[k]), k
        assert torch.equal(got, want) and torch.equal(got_st[0], want_st[0])
        packed[device] = _fused_t_bytes(m)
        if fuse_blocks:
            assert len(packed[device]) == 6                                               # the six blocks ARE transposed-layout entries
            for a, b in zip(packed[device], _fused_t_bytes(fresh)):                       # ... remade to a fresh pack's bytes
                assert sorted(a) == sorted(b) and all(torch.equal(_bits(a[n]), _bits(b[n])) for n in a)
    assert len(packed[False]) == len(packed[True])
    for a, b in zip(packed[False], packed[True]):                                         # the same optimiser path: the same bytes
        assert all(torch.equal(_bits(a[n]), _bits(b[n])) for n in a)


def test_finetune_video_with_the_shallow_stage_is_the_manual_loop():
    from iip_uavsal_saliency_amd.stream import finetune_video
    n = 2 * T_ * 2
    frames = torch.from_numpy(synth.synth_frames_u8(n, H_, W_, 2)).to(DEV)
    gp = torch.from_numpy(synth.gauss_priors(1, H_ // 8, W_ // 8)[0]).to(DEV)
    op_ = torch.from_numpy(synth.ob_priors(1, H_ // 8, W_ // 8)[0]).to(DEV)
    loc = synth.synth_fix_points(n, 90, 280, 12, 9)
    fmap = np.rint(synth.synth_fix_maps(loc, 6.0) * 255).astype(np.uint8)
    fix_map, fix_loc = torch.from_numpy(fmap).to(DEV), torch.from_numpy(loc).to(DEV)
    stages = ("rnn", "decoder", "fuse", "fust", "ctx", "nets", "st", "srf", "backbone", "shallow")

    def make():
        m = _model()
        return m, torch.optim.Adam(_trained(m)[1], lr=1e-4, betas=(0.9, 0.999), weight_decay=5e-5)
    m, opt = make()
    seen = []
    real = train.recurrence_step

    engines = []

    def spy(model, x, cb, state, y, criterion, **kw):
        assert kw == {s: True for s in stages[1:]}
        seen.append((x.clone(), cb, y.clone()))
        ret = real(model, x, cb, state, y, criterion, **kw)
        engines.append({k: id(e) for k, e in model._engines.items()})
        return ret
    train.recurrence_step = spy
    try:
        res = finetune_video(m, frames, gp, op_, fix_map, fix_loc, opt, batch_size=2, stages=stages, refresh="device")
    finally:
        train.recurrence_step = real
    assert res["groups_run"] == 2 and len(seen) == 2
    assert engines[0] and engines[0] == engines[1]                                        # no plan rebuilt behind the device refresh
    m2, opt2 = make()
    state, manual = None, []
    for x, cb, y in seen:
        opt2.zero_grad()
        loss, _, state = train.recurrence_step(m2, x, cb, state, y, **{s: True for s in stages[1:]})
        opt2.step()
        m2.refresh_weights(*_trained(m2)[0], device=True, fused_t=True)
        manual.append(loss.item())
    assert [float(v) for v in res["losses"].tolist()] == manual
    w0 = _model()
    f, f0 = m.sfnet.features.features, w0.sfnet.features.features
    assert not torch.equal(f[3].conv[2].weight.detach(), f0[3].conv[2].weight.detach())   # the shallow blocks moved
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(f[:2].parameters(), f0[:2].parameters()))      # the stem and features[1] did not
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(m.parameters(), m2.parameters()))


def test_shallow_without_its_preconditions_raises_by_name():
    x, cb, y = _step_inputs()
    m = _model()
    with pytest.raises(RuntimeError, match="shallow=True needs backbone=True"):
        train.recurrence_step(m, x, cb, None, y, decoder=True, fuse=True, fust=True, st=True, srf=True, shallow=True)
    assert all(p.grad is None for p in m.parameters())
