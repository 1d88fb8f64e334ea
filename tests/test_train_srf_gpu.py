"""Fine-tuning the SRF-Net head on the MI355X (train.srf_head_backward, recurrence_step(srf=True), csrc/train_srf.hip, the
64 x 32 and 128 x 96 pixel GEMMs of csrc/train_decoder.hip) against the float64 restatement of tests/srf_ref64.py,
teacher-forced stage by stage, and against the reference's recorded gradients (tests/golden/srf_*.npz).

Measured on the MI355X (the worst error / bound per kernel, printed by the tests): see profiles/train_srf.md."""
import ctypes as C
import os
from functools import lru_cache

import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import _lib, losses, ops, synth, train
from iip_uavsal_saliency_amd.model import BasicConv2d, dwBlock, uavsal_srfnet_aspp
from iip_uavsal_saliency_amd.weights import WeightCache

import ctx_ref64 as X
import srf_ref64 as SF
import st_ref64 as SR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = SF.U
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


def _far(wrong, want, bound):
    return float(((wrong.double().cpu() - want.double().cpu()).abs() / bound.double().cpu().clamp_min(1e-300)).max())


def _fenced(t, pad=4):
    """An NHWC tensor as a channel slice between NaN columns: `(view, whole)`."""
    whole = torch.full(t.shape[:-1] + (t.shape[-1] + 2 * pad,), NAN, dtype=t.dtype, device=t.device)
    whole[..., pad:-pad] = t
    return whole[..., pad:-pad], whole


c64 = lambda t: t.detach().double().cpu()                                 # noqa: E731
nchw = lambda t: t.permute(0, 3, 1, 2)                                    # noqa: E731


# ------------------------------------------------------------------------------------------------ 1. conv3_wgrad
@lru_cache(maxsize=None)
def _conv3_ref(co, ci, pic):
    """The inputs and the float64 results of one case, computed once."""
    n, h, w = pic
    rs = np.random.RandomState(31 * co + ci + n * h * w)
    g = torch.from_numpy((rs.standard_normal((n, h, w, co)) / (h * w)).astype(np.float32))
    x = torch.from_numpy((3.0 * rs.random_sample((n, h, w, ci))).astype(np.float32))
    wt = torch.from_numpy(rs.standard_normal((co, ci, 3, 3)).astype(np.float32))
    s = torch.from_numpy((0.5 + rs.random_sample(co)).astype(np.float32))
    G = SF.conv3_wgrad(g.double(), x.double())
    eG, A = SF.conv3_wgrad_bound(g.double(), x.double())
    return g, x, wt, s, G, eG, A


@pytest.mark.parametrize("pic", SF.CONV3_PICTURES, ids=lambda p: "%dx%dx%d" % p)
@pytest.mark.parametrize("co,ci", SF.CONV3_SHAPES)
def test_conv3_wgrad_against_float64(co, ci, pic):
    g, x, wt, s, G, eG, A = _conv3_ref(co, ci, pic)
    K = pic[0] * pic[1] * pic[2]
    xv, _ = _fenced(x.to(DEV))                                            # the operand as a channel slice between NaN columns
    gd, wd, sd = g.to(DEV), wt.to(DEV), s.to(DEV)
    box = torch.full((co + 2, ci, 3, 3), NAN, dtype=torch.float32, device=DEV)   # rows in front of 0 and behind Co stay NaN
    out = box[1:co + 1]
    rowdot = torch.full((co + 2,), NAN, dtype=torch.float64, device=DEV)
    train.conv3_wgrad(gd, xv, out=out, row_scale=sd, w=wd, rowdot=rowdot[1:co + 1])
    s64 = s.double().view(-1, 1, 1, 1)
    tag = "conv3_wgrad %dx%d %dx%dx%d" % ((co, ci) + pic)
    _check(out, s64 * G, s64 * (eG + U * A) + 1e-300, tag)
    _check(rowdot[1:co + 1], (wt.double() * G).sum((1, 2, 3)), (wt.double().abs() * eG).sum((1, 2, 3)) + 1e-300, tag + " rowdot")
    assert bool(torch.isnan(box[0]).all()) and bool(torch.isnan(box[co + 1]).all()) and bool(torch.isnan(rowdot[[0, co + 1]]).all())
    first = out.clone()
    train.conv3_wgrad(gd, xv, out=out, row_scale=sd)
    assert torch.equal(_bits(out), _bits(first))                          # same bits twice
    plain = train.conv3_wgrad(gd, x.to(DEV))                              # dense operand, no scale: the same sums
    _check(plain, G, eG + 1e-300, tag + " unscaled")
    train.conv3_wgrad(gd, xv, out=out, row_scale=sd, accumulate=True)
    _check(out, 2 * first.double(), 4 * U * first.double().abs() + 1e-300, tag + " accumulate")
    lib = _lib.load()
    d = _lib.Conv3WgradDesc()
    d.n_img, d.H, d.W, d.Co, d.Ci = pic[0], pic[1], pic[2], co, ci
    assert lib.uavsal_conv3_wgrad_shares(C.byref(d)) == SF.conv3_partition(K, co, ci)[1]
    if pic == (1, 1, 1):                                                  # every shifted tap leaves the frame
        off = first.clone()
        off[:, :, 1, 1] = 0
        assert float(off.abs().max()) == 0.0 and float(first[:, :, 1, 1].abs().min()) > 0
    elif pic[0] > 1 or pic[1] > 1:
        for v in SF.CONV3_WRONG:
            if v == "frame_neighbour" and pic[0] == 1 or v == "last_half_tile_skipped" and not ci % 128:
                continue
            wrong = SF.conv3_wgrad(g.double(), x.double(), v)
            assert _far(s64 * wrong, s64 * G, s64 * (eG + U * A) + 1e-300) >= 4.0, v


def test_conv3_wgrad_refuses_by_name():
    g = torch.zeros((1, 4, 4, 128), device=DEV)
    for co, ci in ((192, 64), (128, 96), (128, 32)):
        with pytest.raises(RuntimeError, match="Co % 128"):
            train.conv3_wgrad(torch.zeros((1, 4, 4, co), device=DEV), torch.zeros((1, 4, 4, ci), device=DEV))
    with pytest.raises(RuntimeError, match="same pixels"):
        train.conv3_wgrad(g, torch.zeros((1, 4, 5, 64), device=DEV))
    with pytest.raises(RuntimeError, match="accumulate"):
        train.conv3_wgrad(g, torch.zeros((1, 4, 4, 64), device=DEV), accumulate=True)
    with pytest.raises(RuntimeError, match="rowdot"):
        train.conv3_wgrad(g, torch.zeros((1, 4, 4, 64), device=DEV), rowdot=torch.zeros(128, dtype=torch.float64, device=DEV))


# ------------------------------------------------------------------------------------------------ 2. the dilated depthwise
def _dil_case(ch, n, h, w, dil):
    """gd, d, e with all three ReLU6 classes and both clamps themselves (exactly 0 and 6), wd, s2, go."""
    rs = np.random.RandomState(17 * ch + n * h * w + dil)
    shape = (n, h, w, ch)
    gd = torch.from_numpy((rs.standard_normal(shape) / (h * w)).astype(np.float32))
    d, e = (torch.from_numpy((-1.0 + 8.0 * rs.random_sample(shape)).clip(0, 6).astype(np.float32)) for _ in range(2))
    wd = torch.from_numpy(rs.standard_normal((ch, 3, 3)).astype(np.float32))
    s2 = torch.from_numpy((0.5 + rs.random_sample(ch)).astype(np.float32))
    go = torch.from_numpy((rs.standard_normal((n, h, w, 128)) / (h * w)).astype(np.float32))
    return gd, d, e, wd, s2, go


@pytest.mark.parametrize("n", SF.DIL_N)
@pytest.mark.parametrize("dil,h,w", SF.DIL_CASES)
@pytest.mark.parametrize("ch", SF.DIL_CH)
def test_ir_bwd_dil_and_ir_sums_dil_against_float64(ch, dil, h, w, n):
    gd, d, e, wd, s2, go = _dil_case(ch, n, h, w, dil)
    assert bool((d == 0).any()) and bool((d == 6).any()) and bool((e == 0).any()) and bool((e == 6).any())
    tag = "Ch%d dil%d %dx%dx%d" % (ch, dil, n, h, w)
    dev = lambda t: t.to(DEV)                                             # noqa: E731
    w9 = wd.reshape(ch, 9).t().contiguous()                               # tap-major [9][C], as uavsal_dw_desc takes it
    # inside NaN fences: dense tensors cut from a larger NaN buffer, so a read or write outside them shows
    def boxed(t):
        buf = torch.full((t.numel() + 2 * 64,), NAN, dtype=torch.float32, device=DEV)
        buf[64:-64] = dev(t).reshape(-1)
        return buf[64:-64].view(t.shape), buf
    (gdd, _), (dd, _), (ed, _) = boxed(gd), boxed(d), boxed(e)
    ga = train.ir_bwd_dil(gdd, dd, ed, dev(w9), dev(s2), dil)
    args = (gd.double(), d.double(), e.double(), wd.double(), s2.double(), dil)
    want, bound = SF.ir_bwd_dil(*args), SF.ir_bwd_dil_bound(*args)
    _check(ga, want, bound + 1e-300, "ir_bwd_dil " + tag)
    m = SF.m6(e.double())
    assert bool((ga.cpu()[~m] == 0).all())                                # e == 0 and e == 6 pass nothing
    assert torch.equal(_bits(ga), _bits(train.ir_bwd_dil(gdd, dd, ed, dev(w9), dev(s2), dil)))      # same bits twice
    gov, _ = _fenced(dev(go))
    ws, slabs = train.ir_sums_dil(gdd, dd, ed, ga, gov, dil)
    assert slabs == SF.slab_partition(n, h, w)[1] and ws.numel() == slabs * (_lib.IR_NSUM * ch + 128)
    tot = ws.view(slabs, -1).sum(0).cpu()
    (S2, Gd, S1, S3), (bS2, bGd, bS1, bS3) = SF.ir_sums_dil(gd.double(), d.double(), e.double(), c64(ga), go.double(), dil)
    got_Gd = tot[ch:10 * ch].view(3, 3, ch).permute(2, 0, 1)
    _check(tot[:ch], S2, bS2 + 1e-300, "ir_sums_dil S2 " + tag)
    _check(got_Gd, Gd, bGd + 1e-300, "ir_sums_dil Gd " + tag)
    _check(tot[10 * ch:11 * ch], S1, bS1 + 1e-300, "ir_sums_dil S1 " + tag)
    _check(tot[11 * ch:], S3, bS3 + 1e-300, "ir_sums_dil S3 " + tag)
    ws2, _ = train.ir_sums_dil(gdd, dd, ed, ga, gov, dil)
    assert torch.equal(ws.view(torch.int64).cpu(), ws2.view(torch.int64).cpu())               # same bits twice
    if dil < h or dil < w:                                                # a live off-centre tap: dilation 1 is another answer
        assert _far(SF.ir_bwd_dil(*args[:5], dil, "dilation_1"), want, bound + 1e-300) >= 4.0
        Gd1 = SF.ir_sums_dil(gd.double(), d.double(), e.double(), c64(ga), go.double(), dil, "dilation_1")[0][1]
        assert _far(Gd1, Gd, bGd + 1e-300) >= 4.0
    else:
        off = got_Gd.clone()
        off[:, 1, 1] = 0
        assert float(off.abs().max()) == 0.0
    assert _far(SF.ir_bwd_dil(*args[:5], dil, "nonstrict_masks"), want, bound + 1e-300) >= 4.0
    if dil == 2:                                                          # and the undilated kernels agree at dilation 1
        g1 = train.ir_bwd_dil(gdd, dd, ed, dev(w9), dev(s2), 1)
        _check(g1, c64(train.ir_bwd(gdd.contiguous(), dd.contiguous(), ed.contiguous(), dev(w9), dev(s2))),
               2 * SF.ir_bwd_dil_bound(*args[:5], 1) + 1e-300, "ir_bwd_dil at dilation 1 against ir_bwd " + tag)


# (n, H, W, Ch, Co), slabs: one slab and one channel group; 36 rows at 26 rows per slab are two slabs, the second partial, and
# Ch = 320 leaves the second channel group mostly idle
@pytest.mark.parametrize("n,h,w,ch,co,slabs_want", [(2, 5, 7, 64, 64, 1), (3, 12, 20, 320, 128, 2)])
def test_ir_sums_dil_at_dilation_1_has_the_bits_of_ir_sums(n, h, w, ch, co, slabs_want):
    """The instantiations of the channel-sums kernel share one order of additions: at dilation 1 the dilated launch reads
    the taps of the undilated one, so its workspace is the same bytes, slab for slab."""
    rs = np.random.RandomState(1000 * ch + n * h * w)
    gd, ga = (torch.from_numpy((rs.standard_normal((n, h, w, ch)) / (h * w)).astype(np.float32)).to(DEV) for _ in range(2))
    d, e = (torch.from_numpy((-1.0 + 8.0 * rs.random_sample((n, h, w, ch))).clip(0, 6).astype(np.float32)).to(DEV) for _ in range(2))
    go = torch.from_numpy((rs.standard_normal((n, h, w, co)) / (h * w)).astype(np.float32)).to(DEV)
    k = _lib.IrSumsDesc()
    k.n_img, k.H, k.W, k.Ch, k.Co = n, h, w, ch, co
    assert int(_lib.load().uavsal_ir_sums_slabs(C.byref(k))) == slabs_want
    ws, slabs = train.ir_sums(gd, d, e, ga, go)
    ws1, slabs1 = train.ir_sums_dil(gd, d, e, ga, go, 1)
    assert slabs == slabs1 == slabs_want
    assert ws.numel() == ws1.numel() == slabs * (_lib.IR_NSUM * ch + co)
    assert bool(torch.isfinite(ws).all()) and float(ws.abs().max()) > 0.0
    assert torch.equal(ws.view(torch.int64).cpu(), ws1.view(torch.int64).cpu())


# ------------------------------------------------------------------------------------------------ 3. the pixel GEMM's new shapes
@pytest.mark.parametrize("M,N", SF.GEMM_NEW_SHAPES + SF.GEMM_OLD_SHAPES)
def test_pix_gemm_shapes_of_the_head(M, N):
    worst = 0.0
    for K in SR.GEMM32_K:
        rs = np.random.RandomState(K + M + N)
        a = torch.from_numpy((1e-2 * rs.standard_normal((1, 1, K, M))).astype(np.float32))
        b = torch.from_numpy(rs.standard_normal((1, 1, K, N)).astype(np.float32))
        w = torch.from_numpy(rs.standard_normal((M, N)).astype(np.float32)).to(DEV)
        rsc = torch.from_numpy((0.5 + rs.random_sample(M)).astype(np.float32)).to(DEV)
        av, _ = _fenced(a.to(DEV))
        bv, _ = _fenced(b.to(DEV))
        box = torch.full((M + 2, N), NAN, dtype=torch.float32, device=DEV)
        out = box[1:M + 1]
        rowdot = torch.full((M + 2,), NAN, dtype=torch.float64, device=DEV)
        train.pix_gemm(av, bv, out=out, row_scale=rsc, w=w, rowdot=rowdot[1:M + 1])
        G = a.double().view(K, M).t() @ b.double().view(K, N)
        A = a.double().abs().view(K, M).t() @ b.double().abs().view(K, N)
        eG = SR.gemm_n_eff(K) * U * A
        s64 = rsc.double().cpu().view(-1, 1)
        worst = max(worst, _check(out, s64 * G, s64 * (eG + U * A), "pix_gemm %dx%d K%d" % (M, N, K)))
        _check(rowdot[1:M + 1], (w.double().cpu() * G).sum(1), (w.double().cpu().abs() * eG).sum(1) + 1e-300, "rowdot %dx%d K%d" % (M, N, K))
        assert bool(torch.isnan(box[0]).all()) and bool(torch.isnan(box[M + 1]).all()) and bool(torch.isnan(rowdot[[0, M + 1]]).all())
        first = out.clone()
        train.pix_gemm(av, bv, out=out, row_scale=rsc)
        assert torch.equal(_bits(out), _bits(first))                      # same bits twice
        train.pix_gemm(av, bv, out=out, row_scale=rsc, accumulate=True)
        _check(out, 2 * first.double(), 4 * U * first.double().abs() + 1e-300, "accumulate %dx%d K%d" % (M, N, K))
        wrong = (s64 * G).clone()
        wrong[:, -32:] = 0                                                # the last 32-column tile skipped
        assert _far(wrong, s64 * G, s64 * (eG + U * A)) >= 4.0
    print("pix_gemm %dx%d: worst error / bound %.3f" % (M, N, worst))


# ------------------------------------------------------------------------------------------------ 4. conv3_backward, a dilated block
def _rand_bn(bn, rs):
    c = bn.weight.numel()
    with torch.no_grad():
        bn.running_mean.copy_(torch.from_numpy(0.3 * rs.standard_normal(c)))
        bn.running_var.copy_(torch.from_numpy(rs.choice(np.array([0.25, 1.0, 4.0]), c) - SF.BN_EPS))
        bn.weight.copy_(torch.from_numpy(0.5 + rs.random_sample(c)))
        bn.bias.copy_(torch.from_numpy(1.5 + 0.5 * rs.standard_normal(c)))


@pytest.mark.parametrize("pic", [(1, 5, 7), (2, 9, 13)], ids=lambda p: "%dx%dx%d" % p)
def test_conv3_backward_teacher_forced_against_float64(pic):
    n, h, w = pic
    rs = np.random.RandomState(n * h * w + 5)
    m = BasicConv2d(64, 128, 3)
    with torch.no_grad():
        m[0].weight.copy_(torch.from_numpy(rs.standard_normal((128, 64, 3, 3)) * np.sqrt(2.0 / (128 * 9)) * 3.0))
    _rand_bn(m[1], rs)
    with torch.no_grad():
        m[1].weight[5] = 0.0                                              # gamma = 0: a zero weight-gradient row, a live gamma gradient
    m = m.to(DEV).eval()
    x = torch.from_numpy((2.0 * rs.random_sample((n, h, w, 64))).astype(np.float32)).to(DEV)
    g = torch.from_numpy((rs.standard_normal((n, h, w, 128)) / (h * w)).astype(np.float32)).to(DEV)
    lib = _lib.load()
    cache = WeightCache(torch.device(DEV), {})
    y = train._conv(lib, cache, x, m[0], 128, 9, bn=m[1], act=_lib.ACT_RELU6)
    yc = y.cpu()
    assert bool((yc == 0).any()) and bool((yc == 6).any()) and bool(((yc > 0) & (yc < 6)).any())
    gv, _ = _fenced(g)
    gx, grads = train.conv3_backward(m[0], m[1], nchw(x), y, nchw(gv), cache=cache)
    args = (c64(x), c64(y), c64(g), c64(m[0].weight), c64(m[1].weight), c64(m[1].running_mean), c64(m[1].running_var))
    want, bound = SF.cbr3_grads(*args, bounds=True)
    got = {"W": grads["0.weight"], "gamma": grads["1.weight"], "beta": grads["1.bias"], "x": gx.permute(0, 2, 3, 1)}
    for k in got:
        _check(got[k], want[k], bound[k] + 1e-300, "conv3_backward %dx%dx%d %s" % (pic + (k,)))
    assert float(grads["1.weight"][5].abs()) > 0 and float(grads["0.weight"][5].abs().max()) == 0
    gx2, grads2 = train.conv3_backward(m[0], m[1], nchw(x), y, nchw(gv), cache=cache)
    assert torch.equal(_bits(gx), _bits(gx2)) and all(torch.equal(_bits(grads[k]), _bits(grads2[k])) for k in grads)
    g0, _ = train.conv3_backward(m[0], m[1], nchw(x), y, nchw(gv), need_x_grad=False, cache=cache, grads=grads2, accumulate=True)
    assert g0 is None
    for k in grads:
        _check(grads2[k], 2 * grads[k].double(), 4 * U * grads[k].double().abs() + 1e-300, "conv3_backward accumulate %s" % k)
    for v in SF.STAGE_WRONG + SF.CONV3_WRONG[:3] + ("nonstrict_masks",):
        wr = SF.cbr3_grads(*args, variant=v)
        assert max(_far(wr[k], want[k], bound[k] + 1e-300) for k in ("W", "gamma", "beta")) >= 4.0, v


def _dil_block_check(blk, x, go, pt, grads, dil, tag):
    seq = blk.conv
    bn = lambda b: (c64(b.weight), c64(b.running_mean), c64(b.running_var))      # noqa: E731
    args = (c64(x), c64(pt["e"]), c64(pt["d"]), c64(pt["gd"]), c64(pt["ga"]), c64(go), c64(seq[0][0].weight), c64(seq[1][0].weight),
            c64(seq[2].weight), bn(seq[0][1]), bn(seq[1][1]), bn(seq[3]), dil)
    want, bound = SF.block_grads_dil(*args)
    worst = 0.0
    for i, n in enumerate(train.BLOCK_PARAMS):
        worst = max(worst, _check(grads[n].reshape(want[i].shape), want[i], bound[i] + 1e-300, "%s %s" % (tag, n)))
    wr, _ = SF.block_grads_dil(*args, variant="dilation_1")
    return worst, _far(wr[3], want[3], bound[3] + 1e-300)


def test_block_param_grads_of_a_dilated_block():
    n, h, w, dil = 2, 7, 13, 6
    rs = np.random.RandomState(77)
    blk = dwBlock(64, 128, 3, dilation=dil)
    for b in (blk.conv[0][1], blk.conv[1][1], blk.conv[3]):
        _rand_bn(b, rs)
    blk = blk.to(DEV).eval()
    x = torch.from_numpy((2.0 * rs.standard_normal((n, h, w, 64))).astype(np.float32)).to(DEV)
    go = torch.from_numpy((rs.standard_normal((n, h, w, 128)) / (h * w)).astype(np.float32)).to(DEV)
    lib = _lib.load()
    cache = WeightCache(torch.device(DEV), {})
    prt = train._param_grad_parts(blk)
    e, d = train._block_recompute(lib, cache, blk, x, 1, prt, dil)
    # the recomputed tensors are the dilated forward's: float64 from the stored e
    s2, b2, _ = SF.bn_fold(c64(prt[3].weight), c64(prt[3].bias), c64(prt[3].running_mean), c64(prt[3].running_var))
    d64 = (torch.nn.functional.conv2d(nchw(c64(e)), c64(prt[2].weight), padding=dil, dilation=dil, groups=384)
           * s2.view(1, -1, 1, 1) + b2.view(1, -1, 1, 1)).clamp(0, 6).permute(0, 2, 3, 1)
    assert float((c64(d) - d64).abs().max()) <= 1e-4
    grads = train.block_param_grads(blk, nchw(x), e, d, nchw(go), cache=cache)
    gd = train._conv(lib, cache, go, prt[4], 384, 1, tscale=prt[5])
    ga = train.ir_bwd_dil(gd, d, e, *cache.depthwise(prt[2], prt[3])[:2], dil)
    worst, far = _dil_block_check(blk, x, go, dict(e=e, d=d, gd=gd, ga=ga), grads, dil, "dilated block 64-384-128")
    assert far >= 4.0
    again = train.block_param_grads(blk, nchw(x), e, d, nchw(go), gd=gd, ga=ga, cache=cache)
    assert all(torch.equal(_bits(grads[k]), _bits(again[k])) for k in grads)


# ------------------------------------------------------------------------------------------------ 5. the head
@lru_cache(maxsize=None)
def _head():
    return SF.calibrate(uavsal_srfnet_aspp("mobilenet_v2")).to(DEV).eval()


@lru_cache(maxsize=None)
def _head_run(case):
    c3, c4, c5, go = (torch.from_numpy(t).to(DEV).contiguous(memory_format=torch.channels_last) for t in SF.golden_inputs(case))
    sf = _head()
    lib = _lib.load()
    pt = {}
    # y: conv_last's own activation, by the forward's launches (the walk recomputes `cat` the same way)
    tmp = {}
    train.srf_head_backward(sf, c3, c4, c5, torch.zeros_like(go), go, parts=tmp)
    cache = WeightCache(torch.device(DEV), {})
    y = train._conv(lib, cache, tmp["cat"], sf.conv_last[0], 256, 9, bn=sf.conv_last[1], act=_lib.ACT_RELU6)
    grads = train.srf_head_backward(sf, c3, c4, c5, nchw(y), go, parts=pt)
    return (c3, c4, c5, go), y, grads, pt


@pytest.mark.parametrize("case", SF.GOLDEN_CASES, ids=SF.golden_name)
def test_srf_head_backward_against_the_reference_goldens(case):
    """The whole walk against the reference's own float64 autograd: the gradients agree to the accuracy an fp32 forward allows
    (masks decided by fp32 activations may differ from float64's at a handful of elements: the loose 2e-3 of each tensor's
    norm that tests/test_train_st_gpu.py uses -- the stage-by-stage test is the sharp one, this one catches a wrong
    composition)."""
    _, _, grads, _ = _head_run(case)
    assert sorted(grads) == sorted(train.SRF_HEAD_PARAMS) and all(p.grad is None for p in _head().parameters())
    z = np.load(os.path.join(GOLDEN, SF.golden_name(case) + ".npz"))
    assert str(z["digest"]) == SF.golden_digest(_head(), *SF.golden_inputs(case))
    mine = SF.golden_pack({n: c64(g).numpy() for n, g in grads.items()})
    for k, v in mine.items():
        if k.endswith("__sum") or k.endswith("__l2"):
            continue
        err = float(np.sqrt(((v - z[k]) ** 2).sum())) / max(float(np.sqrt((z[k] ** 2).sum())), 1e-300)
        print("srf head vs the reference %s %s: relative error %.3e" % (SF.golden_name(case), k, err))
        assert err <= 2e-3, (k, err)
    for k in (k for k in mine if k.endswith("__l2")):
        assert abs(float(mine[k]) - float(z[k])) <= 2e-3 * float(z[k]), k


@pytest.mark.parametrize("case", SF.GOLDEN_CASES, ids=SF.golden_name)
def test_srf_head_backward_stage_by_stage(case):
    (c3, c4, c5, go), y, grads, pt = _head_run(case)
    sf = _head()
    nh = lambda t: t.permute(0, 2, 3, 1)                                  # noqa: E731
    fl = lambda t: c64(t).reshape(-1, t.shape[-1])                        # noqa: E731
    bn3 = lambda b: (c64(b.weight), c64(b.running_mean), c64(b.running_var))      # noqa: E731

    def cbr(name, xin, yv, g, gx_got=None):
        m = getattr(sf, name)
        want, bound = SR.cbr_grads(fl(xin), fl(yv), fl(g), c64(m[0].weight).reshape(m[0].weight.shape[0], -1), *bn3(m[1]), bounds=True)
        got = {"W": grads[name + ".0.weight"].view(want["W"].shape), "gamma": grads[name + ".1.weight"], "beta": grads[name + ".1.bias"]}
        if gx_got is not None:
            got["x"] = gx_got.reshape(want["x"].shape)
        for k in got:
            _check(got[k], want[k], bound[k] + 1e-300, "head %s %s" % (name, k))
    # the forward's own tensors
    n5, n4 = pt["x5"].shape[3], pt["x4"].shape[3]
    assert pt["cat"].shape[3] == 448 and torch.equal(_bits(pt["cat"][..., n5 + n4:]), _bits(pt["x3"]))
    assert torch.equal(_bits(pt["aspp"][..., 256:512]), _bits(pt["a2"])) and pt["aspp"].shape[3] == 1024
    up = torch.nn.functional.interpolate(nchw(c64(pt["x5"])), size=pt["cat"].shape[1:3], mode="bilinear", align_corners=True)
    assert float((c64(pt["cat"][..., :n5]) - nh(up)).abs().max()) <= 1e-4     # (the plan's resize: tests/test_plan_ops_fp64.py bounds it)
    # 1. conv_last
    m = sf.conv_last
    want, bound = SF.cbr3_grads(c64(pt["cat"]), c64(y), c64(nh(go)), c64(m[0].weight), *bn3(m[1]), bounds=True)
    for k, got in (("W", grads["conv_last.0.weight"]), ("gamma", grads["conv_last.1.weight"]), ("beta", grads["conv_last.1.bias"]),
                   ("x", pt["g_cat"])):
        _check(got, want[k], bound[k] + 1e-300, "head conv_last %s" % k)
    # 2. the upsamples' adjoints
    for name, sl in (("g_x5", slice(0, n5)), ("g_x4", slice(n5, n5 + n4))):
        src = nchw(c64(pt["g_cat"][..., sl]))
        w64, b64 = X.bilinear_bwd_ref(src, src.shape[0], *pt[name].shape[1:3], src.shape[0], 1, bounds=True)
        assert float((w64 - SF.up_bwd(src, *pt[name].shape[1:3])).abs().max()) <= 1e-12 * float(w64.abs().max())
        _check(pt[name], nh(w64), nh(b64) + 1e-300, "head %s" % name)
    # 3. the 1x1 stages
    cbr("conv_lv3", nh(c3), pt["x3"], pt["g_cat"][..., n5 + n4:])
    cbr("conv_lv4", nh(c4), pt["x4"], pt["g_x4"])
    cbr("conv_lv5", pt["aspp"], pt["x5"], pt["g_x5"], gx_got=pt["g_aspp"])
    cbr("lv5_aspp1", nh(c5), pt["a1"], pt["g_aspp"][..., :256])
    # 4. the dilated branches
    for i, name in enumerate(SF.HEAD_BLOCKS):
        b = getattr(sf, name)
        dil = b.dilation
        gb = pt["g_aspp"][..., 256 * (i + 1):256 * (i + 2)]
        parts = dict(e=pt["e%d" % (i + 2)], d=pt["d%d" % (i + 2)], gd=pt["gd%d" % (i + 2)], ga=pt["ga%d" % (i + 2)])
        args = (c64(parts["gd"]), c64(parts["d"]), c64(parts["e"]), c64(b.conv[1][0].weight).reshape(-1, 3, 3))
        s2 = SF.bn_fold(*(c64(t) for t in (b.conv[1][1].weight, b.conv[1][1].bias, b.conv[1][1].running_mean, b.conv[1][1].running_var)))[0]
        _check(parts["ga"], SF.ir_bwd_dil(*args, s2, dil), SF.ir_bwd_dil_bound(*args, s2, dil) + 1e-300, "head %s ga" % name)
        _dil_block_check(b, nh(c5), gb, parts, {n: grads["%s.%s" % (name, n)] for n in train.BLOCK_PARAMS}, dil, "head " + name)
    # the same bits twice; accumulate doubles
    again = train.srf_head_backward(sf, c3, c4, c5, nchw(y), go)
    assert all(torch.equal(_bits(grads[k]), _bits(again[k])) for k in grads)
    train.srf_head_backward(sf, c3, c4, c5, nchw(y), go, grads=again, accumulate=True)
    for k in grads:
        _check(again[k], 2 * grads[k].double(), 4 * U * grads[k].double().abs() + 1e-300, "head accumulate %s" % k)


# ------------------------------------------------------------------------------------------------ 6. the step and the driver
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


def _kw(m, srf=True):
    kw = dict(decoder=True, fuse=True, st=True, srf=srf)
    if m.num_cb:
        kw.update(fust=True, ctx=True)
        if train.prior_nets(m):
            kw.update(nets=True)
    return kw


def _srf_names():
    return ["sfnet." + n for n in train.SRF_HEAD_PARAMS]


def _stats(m):
    return [b.detach().clone() for b in m.buffers()]


@pytest.mark.parametrize("kind", list(BIAS))
def test_recurrence_step_with_the_srf_head(kind):
    m = _model(kind)
    x, cb, y = _step_inputs()
    names = _srf_names()
    assert len(names) == 42
    stats = _stats(m)
    loss, out, st = train.recurrence_step(m, x, cb, None, y, **_kw(m))
    taps = {}
    m(x, cb, None, taps=taps)
    assert tuple(taps["c5"].shape[2:]) == (3, 7) and tuple(taps["c3"].shape[2:]) == (9, 28)      # dilation 6 has live horizontal taps
    ref_out, ref_st = m(x, cb, None)
    assert torch.equal(out, ref_out) and torch.equal(st[0], ref_st[0]) and loss.item() == losses.loss_fu(ref_out, y).item()
    params = dict(m.named_parameters())
    plain = _model(kind)
    train.recurrence_step(plain, x, cb, None, y, **_kw(plain, srf=False))
    earlier = sorted(k for k, p in plain.named_parameters() if p.grad is not None)
    assert not any(k.startswith("sfnet.") for k in earlier)
    assert sorted(k for k, p in params.items() if p.grad is not None) == sorted(earlier + names)      # features receive nothing
    g1 = {k: params[k].grad.clone() for k in earlier + names}
    assert all(torch.isfinite(v).all() and float(v.abs().max()) > 0 and v.is_contiguous() for v in g1.values())
    pp = dict(plain.named_parameters())
    assert all(torch.equal(_bits(g1[k]), _bits(pp[k].grad)) for k in earlier)             # every earlier stage: the same bits
    engines = {k: id(e) for k, e in m._engines.items()}
    train.recurrence_step(m, x, cb, None, y, **_kw(m))                                    # .grad += as loss.backward() would
    for k in names:
        _check(params[k].grad, 2 * g1[k].double(), 4 * U * g1[k].double().abs() + 1e-300, "second call doubles %s" % k)
    assert all(torch.equal(a, b) for a, b in zip(stats, _stats(m)))
    # the directional derivative along the normalised head gradient against the central difference of the GPU forward
    # (the plumbing check of tests/test_train_ctx_gpu.py, with its 10 % and for its reason)
    head = train.srf_head(m)
    with torch.no_grad():
        norm = SF.norm2([g1[k] for k in names])
        w0 = {k: params[k].detach().clone() for k in names}
        s = 2e-2 / norm
        vals = []
        for sign in (1.0, -1.0):
            for k in names:
                params[k].copy_(w0[k] + sign * s * g1[k] / norm)
            assert m.refresh_weights(*head) > 0
            vals.append(losses.loss_fu(m(x, cb, None)[0], y).item())
        for k in names:
            params[k].copy_(w0[k])
        m.refresh_weights(*head)
    fd = (vals[0] - vals[1]) / (2 * s)
    print("%s: srf head directional derivative: finite difference %.6e, <grad, D> %.6e, step %.3e" % (kind, fd, norm, s))
    assert abs(fd - norm) <= 0.10 * abs(norm)
    assert torch.equal(m(x, cb, None)[0], ref_out)                                        # the restored weights give the same bits
    assert {k: id(e) for k, e in m._engines.items()} == engines                           # no plan rebuilt


def _trained(m):
    mods = [m.rnn, m.conv_out_st, m.fucbst_layer, m.fust_layer, m.fucb_layer, m.cxt_cb_prior, *train.prior_nets(m).values(), m.st_layer,
            *train.srf_head(m)]
    return mods, [p for mod in mods for p in mod.parameters()]


def test_adam_steps_over_eight_stages_keep_the_plans():
    """Two Adam steps over all eight stages, host refresh in the default configuration and host against device refresh with
    `model.winograd = False` (the comparison of test_adam_steps_over_seven_stages_keep_the_plans, for its reason: the device
    repack makes the Winograd filter transforms within one fp32 ulp, and the head's `conv_last` has one, so with Winograd in
    the plan nothing behind `conv_last` is bit-comparable between the two paths).  Device refresh in the default configuration
    runs too: the loss falls, the head moves, no plan is rebuilt, the frozen features' taps equal a fresh model's bit for bit
    and the head's output agrees with it to 1e-4 of its largest element (an ulp in a filter transform, carried through one
    256-channel 3x3 sum)."""
    from iip_uavsal_saliency_amd import UAVSal
    x, cb, y = _step_inputs()
    outs = {}
    for device, wino in ((False, True), (True, True), (False, False), (True, False)):
        m = _model()
        m.winograd = wino
        mods, ps = _trained(m)
        opt = torch.optim.Adam(ps, lr=1e-4, betas=(0.9, 0.999), weight_decay=5e-5)
        h0 = [p.detach().clone() for mod in train.srf_head(m) for p in mod.parameters()]
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
            assert {k: id(e) for k, e in m._engines.items()} == engines                   # the same engine objects
        last = losses.loss_fu(after, y).item()
        print("loss_fu on the group: %.6f before, %.6f after two Adam steps over eight stages (device=%r, winograd=%r)" % (first, last, device, wino))
        assert last < first and not torch.equal(before, after)
        assert all(not torch.equal(a, b) for a, b in zip(h0, (p for mod in train.srf_head(m) for p in mod.parameters())))      # the head moved
        fresh = UAVSal(time_dims=T_)
        fresh.load_state_dict(m.state_dict())
        fresh = fresh.to(DEV).eval()
        fresh.winograd = wino
        taps, ftaps = {}, {}
        got, got_st = m(x, cb, None, taps=taps)
        want, want_st = fresh(x, cb, None, taps=ftaps)
        assert all(torch.equal(taps[k], ftaps[k]) for k in ("c3", "c4", "c5"))              # the frozen features
        if not (device and wino):                                # (behind conv_last: its Winograd transform, see above)
            assert torch.equal(taps["sfnet"], ftaps["sfnet"]) and torch.equal(taps["prefuse"], ftaps["prefuse"])
            assert torch.equal(got, want) and torch.equal(got_st[0], want_st[0])
        else:
            assert float((taps["sfnet"] - ftaps["sfnet"]).abs().max()) <= 1e-4 * float(ftaps["sfnet"].abs().max())
        outs[device, wino] = (got.clone(), got_st[0].clone(), taps["sfnet"].clone())
    assert all(torch.equal(a, b) for a, b in zip(outs[False, False], outs[True, False]))                  # host and device refresh


def test_finetune_video_with_the_srf_stage_is_the_manual_loop():
    from iip_uavsal_saliency_amd.stream import finetune_video
    n = 2 * T_ * 2
    frames = torch.from_numpy(synth.synth_frames_u8(n, H_, W_, 2)).to(DEV)
    gp = torch.from_numpy(synth.gauss_priors(1, H_ // 8, W_ // 8)[0]).to(DEV)
    op_ = torch.from_numpy(synth.ob_priors(1, H_ // 8, W_ // 8)[0]).to(DEV)
    loc = synth.synth_fix_points(n, 90, 280, 12, 9)
    fmap = np.rint(synth.synth_fix_maps(loc, 6.0) * 255).astype(np.uint8)
    fix_map, fix_loc = torch.from_numpy(fmap).to(DEV), torch.from_numpy(loc).to(DEV)
    stages = ("rnn", "decoder", "fuse", "fust", "ctx", "nets", "st", "srf")

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
    assert not torch.equal(m.sfnet.conv_last[0].weight.detach(), w0.sfnet.conv_last[0].weight.detach())
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(m.parameters(), m2.parameters()))


def test_srf_without_its_preconditions_raises_by_name():
    x, cb, y = _step_inputs()
    m = _model()
    with pytest.raises(RuntimeError, match="st=True"):
        train.recurrence_step(m, x, cb, None, y, srf=True)
    with pytest.raises(RuntimeError, match="st=True"):
        train.recurrence_step(m, x, cb, None, y, fuse=True, fust=True, srf=True)
    assert all(p.grad is None for p in m.parameters())
    m(x, cb, None)
    with pytest.raises((NotImplementedError, RuntimeError)):              # the fused backbone blocks and the stem: not in place
        m.refresh_weights(m.sfnet)
