"""Fine-tuning the ST blocks on the MI355X (train.st_block_backward, recurrence_step(st=True), csrc/train_st.hip, the 32-wide
pixel GEMM of csrc/train_decoder.hip) against the float64 restatement of tests/st_ref64.py, teacher-forced stage by stage.

Measured on the MI355X (the worst error / bound per kernel, printed by the tests): see profiles/train_st.md."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import _lib, losses, ops, synth, train
from iip_uavsal_saliency_amd.model import BasicConv2d, STBlock, dwBlock
from iip_uavsal_saliency_amd.weights import WeightCache

import st_ref64 as SR
from saturate_bn import saturate_relu6_bn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = SR.U
NAN = float("nan")


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _ratio(got, want, bound, what):
    got, want, bound = got.detach().double().cpu(), want.double().cpu(), bound.double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), what
    ratio = float(((got - want).abs() / bound.clamp_min(1e-300)).max()) if got.numel() else 0.0
    return ratio


def _check(got, want, bound, what):
    r = _ratio(got, want, bound, what)
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


# ------------------------------------------------------------------------------------------------ 1. tdiff_bwd
def _tdiff_inputs(N, L, mode, C=32, h=5, w=7):
    rs = np.random.RandomState(100 * N + L)
    g = torch.from_numpy(rs.standard_normal((N, h, w, 2 * C)).astype(np.float32))
    if mode == "pass":
        r = torch.from_numpy((0.5 + 5.0 * rs.random_sample((N, h, w, C))).astype(np.float32))
    else:                                                        # all three classes and both clamps themselves
        r = torch.from_numpy(rs.choice(np.array([0.0, 6.0, 1.0, 3.0, 5.5, -0.0], np.float32), (N, h, w, C)))
    return g, r


@pytest.mark.parametrize("N,L", SR.TDIFF_CASES)
def test_tdiff_bwd_against_float64(N, L):
    worst = 0.0
    for mode in ("pass", "clamps"):
        g, r = _tdiff_inputs(N, L, mode)
        gv, _ = _fenced(g.to(DEV))
        rv, _ = _fenced(r.to(DEV))
        got = train.tdiff_bwd(gv, rv, L)
        want, bound = SR.tdiff_bwd(g.double(), r.double(), L), SR.tdiff_bwd_bound(g.double(), r.double(), L)
        worst = max(worst, _check(got, want, bound + 1e-300, "tdiff_bwd N%d L%d %s" % (N, L, mode)))
        assert torch.equal(_bits(got), _bits(train.tdiff_bwd(gv, rv, L)))                    # same bits twice
        if mode == "clamps":
            m = SR.m6(r.double())
            assert bool((got.cpu()[~m] == 0).all()) and bool(m.any()) and bool((~m).any())  # r == 0 and r == 6 pass nothing
            assert _far(SR.tdiff_bwd(g.double(), r.double(), L, "nonstrict_masks"), want, bound + 1e-30) >= 4.0
        else:
            # <tdiff(a), g> == <a, tdiff_bwd(g)> in double with an all-pass r
            a = torch.from_numpy(np.random.RandomState(7).standard_normal(tuple(r.shape))).double()
            lhs = float((SR.tdiff(a, L) * g.double()).sum())
            fwd = ops.tdiff(a.float().to(DEV), L).double().cpu()
            assert float((fwd - SR.tdiff(a.float().double(), L)).abs().max()) <= 2 * U * float(a.abs().max()) * 2
            rhs = float((a * got.double().cpu()).sum())
            assert abs(lhs - rhs) <= 4 * U * float((a.abs() * SR.tdiff_bwd(g.double(), r.double(), L, absolute=True)).sum())
            for v in SR.TDIFF_WRONG[:3]:
                if v == "cross_border" and N == L:
                    continue
                assert _far(SR.tdiff_bwd(g.double(), r.double(), L, v), want, bound + 1e-30) >= 4.0, v
    # inside NaN fences: a dense output tensor whose neighbours stay what they were
    g, r = _tdiff_inputs(N, L, "pass")
    lib = _lib.load()
    out = torch.full((N, 5, 7, 40), NAN, dtype=torch.float32, device=DEV)
    k = _lib.TdiffBwdDesc()
    gd_, rd_ = g.to(DEV), r.to(DEV)
    k.g, k.ldg, k.r, k.ldr, k.out, k.ldo = gd_.data_ptr(), 64, rd_.data_ptr(), 32, out.data_ptr() + 16, 40
    k.n_img, k.HW, k.C, k.seq_len = N, 35, 32, L
    _lib.check(lib.uavsal_tdiff_bwd(C.byref(k), None), "uavsal_tdiff_bwd")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[..., :4]).all()) and bool(torch.isnan(out[..., 36:]).all())
    assert torch.equal(_bits(out[..., 4:36]), _bits(train.tdiff_bwd(gd_, rd_, L)))


# ------------------------------------------------------------------------------------------------ 2. the 32-wide pixel GEMM
@pytest.mark.parametrize("M,N", SR.GEMM32_SHAPES)
def test_pix_gemm_with_a_32_wide_side(M, N):
    worst = 0.0
    for K in SR.GEMM32_K:
        rs = np.random.RandomState(K + M + N)
        a = torch.from_numpy((1e-2 * rs.standard_normal((1, 1, K, M))).astype(np.float32))
        b = torch.from_numpy(rs.standard_normal((1, 1, K, N)).astype(np.float32))
        w = torch.from_numpy(rs.standard_normal((M, N)).astype(np.float32)).to(DEV)
        rsc = torch.from_numpy((0.5 + rs.random_sample(M)).astype(np.float32)).to(DEV)
        av, _ = _fenced(a.to(DEV))
        bv, _ = _fenced(b.to(DEV))
        box = torch.full((M + 2, N), NAN, dtype=torch.float32, device=DEV)     # rows in front of 0 and behind M stay NaN
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
        assert torch.equal(_bits(out), _bits(first))                                      # same bits twice
        train.pix_gemm(av, bv, out=out, row_scale=rsc, accumulate=True)
        _check(out, 2 * first.double(), 4 * U * first.double().abs() + 1e-300, "accumulate %dx%d K%d" % (M, N, K))
        wrong = (s64 * G).clone()
        wrong[:, -32:] = 0                                                                # the last 32-column tile skipped
        assert _far(wrong, s64 * G, s64 * (eG + U * A)) >= 4.0
    print("pix_gemm32 %dx%d: worst error / bound %.3f" % (M, N, worst))


# ------------------------------------------------------------------------------------------------ 3. cbr_backward
def _cbr_case(name, pic, zero_gamma=True, saturate=False):
    """A BasicConv2d 1x1 with calibrated, non-trivial BatchNorm numbers, its input and the gradient at its output."""
    cin, cout = SR.CBR_SHAPES[name]
    n, h, w = pic
    rs = np.random.RandomState(1000 * cin + cout + n * h * w)
    m = BasicConv2d(cin, cout, 1)
    x = (3.0 * rs.random_sample((n, h, w, cin))).astype(np.float32)
    W = (rs.standard_normal((cout, cin)) * np.sqrt(2.0 / cout)).astype(np.float32)
    # calibrated over a fixed population (not this picture: one pixel has no spread): pre-activation mean 1.5 + noise, std 3
    pop = (3.0 * np.random.RandomState(5).random_sample((512, cin))) @ W.T.astype(np.float64)
    s = 3.0 / pop.std(0)
    b = 1.5 + rs.standard_normal(cout) - pop.mean(0) * s
    r = rs.choice(np.array([0.5, 1.0, 2.0]), cout)
    mu = rs.standard_normal(cout)
    with torch.no_grad():
        m[0].weight.copy_(torch.from_numpy(W).view(cout, cin, 1, 1))
        m[1].running_var.copy_(torch.from_numpy(1.0 / r ** 2 - SR.BN_EPS))
        m[1].running_mean.copy_(torch.from_numpy(mu))
        m[1].weight.copy_(torch.from_numpy(s / r))
        m[1].bias.copy_(torch.from_numpy(b + mu * s))
        if zero_gamma:
            m[1].weight[5] = 0.0
            m[1].bias[5] = 1.5
    if saturate:
        holder = torch.nn.Sequential(m)
        assert saturate_relu6_bn(holder, gains={"": (1.5, 3.0)}) == 1
    g = (rs.standard_normal((n, h, w, cout)) / (h * w)).astype(np.float32)
    return m.to(DEV).eval(), torch.from_numpy(x).to(DEV), torch.from_numpy(g).to(DEV)


def _cbr_run(m, x, g, res=None, accumulate=False, grads=None, need_x_grad=True):
    lib = _lib.load()
    cache = WeightCache(torch.device(DEV), {})
    cout = m[0].weight.shape[0]
    y = train._conv(lib, cache, x, m[0], cout, 1, bn=m[1], act=_lib.ACT_RELU6)
    gx, grads = train.cbr_backward(m[0], m[1], x.permute(0, 3, 1, 2), y, g.permute(0, 3, 1, 2), need_x_grad=need_x_grad,
                                   cache=cache, grads=grads, accumulate=accumulate)
    return y, gx, grads


def _cbr_ref(m, x, y, g, variant=None, gres=None, res=None):
    cin = x.shape[-1]
    f = lambda t: t.detach().double().cpu().reshape(-1, t.shape[-1])      # noqa: E731
    return SR.cbr_grads(f(x), f(y), f(g), m[0].weight.detach().double().cpu().view(-1, cin), m[1].weight.detach().cpu(),
                        m[1].running_mean.detach().cpu(), m[1].running_var.detach().cpu(), variant=variant, bounds=variant is None,
                        gres=None if gres is None else f(gres), res=None if res is None else f(res))


@pytest.mark.parametrize("name", list(SR.CBR_SHAPES))
def test_cbr_backward_teacher_forced_against_float64(name):
    worst, far = {}, {v: 0.0 for v in SR.CBR_WRONG}
    for pic in SR.PICTURES:
        for saturate in ((False, True) if pic == (2, 9, 13) else (False,)):
            m, x, g = _cbr_case(name, pic, saturate=saturate)
            gv, _ = _fenced(g)                                                            # the gradient as a channel slice
            y, gx, grads = _cbr_run(m, x, gv)
            want, bound = _cbr_ref(m, x, y, g)
            yc = y.cpu()
            if x.shape[0] * x.shape[1] * x.shape[2] > 1:
                assert bool((yc == 0).any()) and bool((yc == 6).any()) and bool(((yc > 0) & (yc < 6)).any())      # all three classes
            tag = "%s %dx%dx%d%s" % ((name,) + pic + (" saturated" if saturate else "",))
            got = {"W": grads["0.weight"].view(want["W"].shape), "gamma": grads["1.weight"], "beta": grads["1.bias"],
                   "x": gx.permute(0, 2, 3, 1).reshape(want["x"].shape)}
            for k in got:
                worst[k] = max(worst.get(k, 0.0), _check(got[k], want[k], bound[k] + 1e-300, "%s %s" % (tag, k)))
            if not saturate:
                assert float(grads["1.weight"][5].abs()) > 0 and float(grads["0.weight"][5].abs().max()) == 0      # gamma = 0
            y2, gx2, grads2 = _cbr_run(m, x, gv)
            assert all(torch.equal(_bits(grads[k]), _bits(grads2[k])) for k in grads) and torch.equal(_bits(gx), _bits(gx2))
            _cbr_run(m, x, gv, accumulate=True, grads=grads2, need_x_grad=False)
            for k in grads:
                _check(grads2[k], 2 * grads[k].double(), 4 * U * grads[k].double().abs() + 1e-300, "%s accumulate %s" % (tag, k))
            res = torch.full_like(y, 2.0)                                                 # what a later residual would add to y
            for v in SR.CBR_WRONG:
                wr = _cbr_ref(m, x, y, g, variant=v, res=res)
                far[v] = max(far[v], max(_far(wr[k], want[k], bound[k] + 1e-30) for k in got))
    print("cbr_backward %s: worst error / bound %r; wrong variants %r" % (name, worst, far))
    assert all(f >= 4.0 for f in far.values()), far


def test_cbr_sums_writes_the_masked_gradient_bit_for_bit():
    m, x, g = _cbr_case("stconv_last", (3, 45, 80))
    lib = _lib.load()
    y = train._conv(lib, WeightCache(torch.device(DEV), {}), x, m[0], 256, 1, bn=m[1], act=_lib.ACT_RELU6)
    gp, ws, slabs = train.cbr_sums(g, y)
    assert slabs == SR.slab_partition(3, 45, 80)[1] == 20 and 135 % 7 != 0                # slabs across frames, a partial last one
    want = g * ((y > 0) & (y < 6))
    assert torch.equal(_bits(gp), _bits(want + 0.0))
    S = ws.view(slabs, 256).sum(0)
    _check(S, want.double().sum((0, 1, 2)), 2 * U * want.double().abs().sum((0, 1, 2)) + 1e-300, "cbr_sums S")


# ------------------------------------------------------------------------------------------------ 4. a block with Cout = 32
def _rand_bn(bn, rs, spread=3.0):
    c = bn.weight.numel()
    with torch.no_grad():
        bn.running_mean.copy_(torch.from_numpy(0.3 * rs.standard_normal(c)))
        bn.running_var.copy_(torch.from_numpy(rs.choice(np.array([0.25, 1.0, 4.0]), c) - SR.BN_EPS))
        bn.weight.copy_(torch.from_numpy(0.5 + rs.random_sample(c)))
        bn.bias.copy_(torch.from_numpy(0.2 * rs.standard_normal(c)))


def _block_stage_check(blk, x, go, pt, grads, tag, variant_far=None):
    """`grads` (keyed by train.BLOCK_PARAMS) of the dwBlock `blk` against float64 from the stored NHWC tensors."""
    seq = blk.conv
    c64 = lambda t: t.detach().double().cpu()                             # noqa: E731
    bn = lambda b: (c64(b.weight), c64(b.running_mean), c64(b.running_var))      # noqa: E731
    args = (c64(x), c64(pt["e"]), c64(pt["d"]), c64(pt["gd"]), c64(pt["ga"]), c64(go), c64(seq[0][0].weight), c64(seq[1][0].weight),
            c64(seq[2].weight), bn(seq[0][1]), bn(seq[1][1]), bn(seq[3]))
    want, bound = SR.block_grads(*args)
    worst = 0.0
    for i, n in enumerate(train.BLOCK_PARAMS):
        worst = max(worst, _check(grads[n].reshape(want[i].shape), want[i], bound[i] + 1e-300, "%s %s" % (tag, n)))
    if variant_far is not None:
        wr, _ = SR.block_grads(*args, variant="last_tile_skipped")
        variant_far.append(_far(wr[6], want[6], bound[6] + 1e-30))
    return worst


@pytest.mark.parametrize("pic", SR.PICTURES, ids=lambda p: "%dx%dx%d" % p)
def test_block_param_grads_64_384_32(pic):
    n, h, w = pic
    rs = np.random.RandomState(n * h * w + 3)
    blk = dwBlock(64, 32, 3, res_connect=False)
    for b in (blk.conv[0][1], blk.conv[1][1], blk.conv[3]):
        _rand_bn(b, rs)
    blk = blk.to(DEV).eval()
    x = torch.from_numpy((2.0 * rs.standard_normal((n, h, w, 64))).astype(np.float32)).to(DEV)
    go = torch.from_numpy((rs.standard_normal((n, h, w, 32)) / (h * w)).astype(np.float32)).to(DEV)
    pt = {}
    train.block_input_grad(blk, x.permute(0, 3, 1, 2), go.permute(0, 3, 1, 2), parts=pt)
    grads = train.block_param_grads(blk, x.permute(0, 3, 1, 2), pt["e"], pt["d"], go.permute(0, 3, 1, 2), gd=pt["gd"], ga=pt["ga"])
    far = []
    _block_stage_check(blk, x, go, pt, grads, "block 64-384-32 %dx%dx%d" % pic, far)
    assert far[0] >= 4.0
    again = train.block_param_grads(blk, x.permute(0, 3, 1, 2), pt["e"], pt["d"], go.permute(0, 3, 1, 2), gd=pt["gd"], ga=pt["ga"])
    assert all(torch.equal(_bits(grads[k]), _bits(again[k])) for k in grads)


# ------------------------------------------------------------------------------------------------ 5. the ST block, stage by stage
def _st_block(seed=3):
    """An STBlock with the seeded, calibrated numbers of `st_ref64.calibrate` (the numbers of the recorded reference goldens)."""
    return SR.calibrate(STBlock(256, 256, time_dims=5, reduction=8, res_connect=True), seed).to(DEV).eval()


ST_CASES = [(2, 5, 7, None), (5, 5, 7, None), (4, 45, 80, None), (6, 5, 7, 3)]


@pytest.mark.parametrize("case", ST_CASES, ids=lambda c: "N%d_%dx%d_L%s" % c)
def test_st_block_backward_stage_by_stage(case):
    _st_stages(case)


def _st_stages(case):
    N, h, w, L = case
    blk = _st_block()
    rs = np.random.RandomState(N * h * w)
    x = torch.from_numpy((1.5 * rs.standard_normal((N, h, w, 256))).astype(np.float32)).to(DEV)
    go = torch.from_numpy((rs.standard_normal((N, h, w, 256)) / (h * w)).astype(np.float32)).to(DEV)
    nchw = lambda t: t.permute(0, 3, 1, 2)                                # noqa: E731
    pt = {}
    gx, grads = train.st_block_backward(blk, nchw(x), nchw(go), seq_len=L, parts=pt)
    assert sorted(grads) == sorted(train.ST_BLOCK_PARAMS) and all(p.grad is None for p in blk.parameters())      # no .grad touched
    Ls = N if L is None else L
    te = blk.stconv_te
    far = {v: 0.0 for v in SR.WRONG}
    c64 = lambda t: t.detach().double().cpu()                             # noqa: E731

    def cbr(name, m, xin, y, g, prefix, gres=None, gx_got=None, res=None):
        want, bound = _cbr_ref(m, xin, y, g, gres=gres)
        got = {"W": grads[prefix + "0.weight"].view(want["W"].shape), "gamma": grads[prefix + "1.weight"], "beta": grads[prefix + "1.bias"]}
        if gx_got is not None:
            got["x"] = gx_got.reshape(want["x"].shape)
        for k in got:
            _check(got[k], want[k], bound[k] + 1e-300, "st %s %s" % (name, k))
        for v in SR.CBR_WRONG:
            wr = _cbr_ref(m, xin, y, g, variant=v, res=res)
            far[v] = max(far[v], max(_far(wr[k], want[k], bound[k] + 1e-30) for k in got))
        return want
    # the forward's own tensors: ssum is the fp32 sum of its two branches, the masks' inputs reach both clamps
    assert torch.equal(_bits(pt["ssum"]), _bits(pt["x_sp"] + pt["a_te"]))
    for k in ("r", "a_te", "o"):
        assert bool((pt[k] == 0).any()) and bool((pt[k] == 6).any()) and bool(((pt[k] > 0) & (pt[k] < 6)).any()), k
    assert torch.equal(_bits(pt["dif"]), _bits(ops.tdiff(pt["r"], Ls)))
    # 1. stconv_last: x = ssum, y = o (NOT o + x, the block's output)
    cbr("stconv_last", blk.stconv_last, pt["ssum"], pt["o"], go, "stconv_last.", gx_got=pt["g_sum"], res=x)
    # 2. the spatial branch, teacher-forced from its stored tensors; its grad_x GEMM adds grad_out
    _block_stage_check(blk.stconv_sp.spconv, x, pt["g_sum"], pt["sp"], {n: grads["stconv_sp.spconv." + n] for n in train.BLOCK_PARAMS}, "st spconv")
    # 3. last_conv: y = a_te (NOT ssum)
    cbr("last_conv", te.last_conv, pt["t1"], pt["a_te"], pt["g_sum"], "stconv_te.last_conv.", gx_got=pt["g_t1"], res=pt["x_sp"])
    # 4. sub_conv
    lt = []
    _block_stage_check(te.sub_conv, pt["dif"], pt["g_t1"], pt["sub"], {n: grads["stconv_te.sub_conv." + n] for n in train.BLOCK_PARAMS}, "st sub_conv", lt)
    far["last_tile_skipped"] = max(far["last_tile_skipped"], lt[0])
    # 5. tdiff_bwd
    g64, r64 = c64(pt["g_dif"]), c64(pt["r"])
    want, bound = SR.tdiff_bwd(g64, r64, Ls), SR.tdiff_bwd_bound(g64, r64, Ls)
    _check(pt["gp_r"], want, bound + 1e-300, "st tdiff_bwd")
    for v in SR.TDIFF_WRONG:
        if not (v == "cross_border" and Ls == N):
            far[v] = max(far[v], _far(SR.tdiff_bwd(g64, r64, Ls, v), want, bound + 1e-30))
    # 6. reduce_conv: the gradient arrives masked; grad_x = (grad_out + spconv's) + reduce_conv's
    w6 = cbr("reduce_conv", te.reduce_conv, x, pt["r"], pt["gp_r"], "stconv_te.reduce_conv.", gres=pt["gx_sp"],
             gx_got=gx.permute(0, 2, 3, 1))
    b6 = _cbr_ref(te.reduce_conv, x, pt["r"], pt["gp_r"], gres=pt["gx_sp"])[1]["x"]
    no_res = w6["x"] - c64(go).reshape(w6["x"].shape)                                     # the residual term of grad_x dropped
    far["no_residual"] = _far(no_res, w6["x"], b6 + 1e-30)
    # grad_x's spatial part carries grad_out: gx_sp = spconv's grad_x + go, against float64 end to end with autograd
    gx2, grads2 = train.st_block_backward(blk, nchw(x), nchw(go), seq_len=L)
    assert torch.equal(_bits(gx), _bits(gx2)) and all(torch.equal(_bits(grads[k]), _bits(grads2[k])) for k in grads)
    g0, gr0 = train.st_block_backward(blk, nchw(x), nchw(go), seq_len=L, need_x_grad=False)
    assert g0 is None and all(torch.equal(_bits(grads[k]), _bits(gr0[k])) for k in grads)
    print("st_block_backward %r: wrong variants %r" % (case, far))
    return far


def test_every_wrong_variant_is_rejected_somewhere():
    far = {v: 0.0 for v in SR.WRONG}
    for case in (ST_CASES[1], ST_CASES[3]):
        for v, f in _st_stages(case).items():
            far[v] = max(far[v], f)
    assert all(f >= 4.0 for f in far.values()), far


def test_st_block_backward_against_float64_autograd():
    """The whole walk against torch autograd through the float64 restatement: the gradients agree to the accuracy an fp32
    forward allows (masks decided by fp32 activations may differ from float64's at a handful of elements: a loose 2e-3 of
    each tensor's norm -- the stage-by-stage test is the sharp one, this one catches a wrong composition)."""
    N, h, w, L = 6, 5, 7, 3
    blk = _st_block()
    rs = np.random.RandomState(99)
    x = torch.from_numpy((1.5 * rs.standard_normal((N, 256, h, w))).astype(np.float32))
    go = torch.from_numpy((rs.standard_normal((N, 256, h, w)) / (h * w)).astype(np.float32))
    gx, grads = train.st_block_backward(blk, x.to(DEV).contiguous(memory_format=torch.channels_last),
                                        go.to(DEV).contiguous(memory_format=torch.channels_last), seq_len=L)
    P, B = SR.block_params64(blk)
    xx = x.double().requires_grad_(True)
    out = SR.forward64(P, B, xx, L)
    names = list(P)
    gs = torch.autograd.grad(out, [P[n] for n in names] + [xx], go.double())
    for n, want in list(zip(names, gs[:-1])) + [("grad_x", gs[-1])]:
        got = (gx if n == "grad_x" else grads[n]).double().cpu()
        err = SR.norm2([got - want]) / max(SR.norm2([want]), 1e-300)
        print("st block vs float64 autograd %s: relative error %.3e" % (n, err))
        assert err <= 2e-3, (n, err)


def test_refusals_by_name():
    blk = _st_block()
    x = torch.zeros((2, 256, 5, 7), device=DEV).contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match="cuda"):
        train.st_block_backward(blk, x.cpu(), x.cpu())
    blk.train()
    with pytest.raises(RuntimeError, match="eval"):
        train.st_block_backward(blk, x, x)
    blk.eval()
    blk.fu_type = "concat"
    with pytest.raises(RuntimeError, match="fu_type"):
        train.st_block_backward(blk, x, x)
    blk.fu_type = "sum"
    with pytest.raises(RuntimeError, match="seq_len"):
        train.st_block_backward(blk, x, x, seq_len=3)


# ------------------------------------------------------------------------------------------------ 6. the step and the driver
H_, W_, T_ = 72, 104, 4
RNN = "rnn.cell_list.0.rnn_conv.weight"
BIAS = {"b111": [1, 1, 1], "b110": [1, 1, 0], "b000": [0, 0, 0]}


@lru_cache(maxsize=None)
def _step_inputs():
    n = 2 * T_
    x = torch.from_numpy(synth.normalize_frames(synth.synth_frames_u8(n, H_, W_, 3))).to(DEV)
    cb = [torch.from_numpy(synth.gauss_priors(n, H_ // 8, W_ // 8)).to(DEV), torch.from_numpy(synth.ob_priors(n, H_ // 8, W_ // 8, seed=3)).to(DEV)]
    loc = synth.synth_fix_points(n, 90, 130, 12, 4)
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
        for mod in m.st_layer.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.add_(0.05 * torch.randn(mod.running_mean.shape, generator=g))
                mod.running_var.mul_(1.0 + 0.2 * torch.rand(mod.running_var.shape, generator=g))
    return m.to(DEV).eval()


def _kw(m, st=True):
    kw = dict(decoder=True, fuse=True, st=st)
    if m.num_cb:
        kw.update(fust=True, ctx=True)
        if train.prior_nets(m):
            kw.update(nets=True)
    return kw


def _st_names(m):
    return ["st_layer.%d.%s" % (i, n) for i in range(len(m.st_layer)) for n in train.ST_BLOCK_PARAMS]


def _stats(m):
    return [b.detach().clone() for b in m.buffers()]


@pytest.mark.parametrize("kind", list(BIAS))
def test_recurrence_step_with_the_st_blocks(kind):
    m = _model(kind)
    x, cb, y = _step_inputs()
    names = _st_names(m)
    assert len(names) == 54
    stats = _stats(m)
    loss, out, st = train.recurrence_step(m, x, cb, None, y, **_kw(m))
    ref_out, ref_st = m(x, cb, None)
    assert torch.equal(out, ref_out) and torch.equal(st[0], ref_st[0]) and loss.item() == losses.loss_fu(ref_out, y).item()
    params = dict(m.named_parameters())
    plain = _model(kind)
    train.recurrence_step(plain, x, cb, None, y, **_kw(plain, st=False))
    earlier = sorted(k for k, p in plain.named_parameters() if p.grad is not None)
    assert not any(k.startswith("st_layer.") for k in earlier)
    assert sorted(k for k, p in params.items() if p.grad is not None) == sorted(earlier + names)
    g1 = {k: params[k].grad.clone() for k in earlier + names}
    assert all(torch.isfinite(v).all() and float(v.abs().max()) > 0 and v.is_contiguous() for v in g1.values())
    pp = dict(plain.named_parameters())
    assert all(torch.equal(_bits(g1[k]), _bits(pp[k].grad)) for k in earlier)             # every earlier stage: the same bits
    engines = {k: id(e) for k, e in m._engines.items()}
    train.recurrence_step(m, x, cb, None, y, **_kw(m))                                    # .grad += as loss.backward() would
    for k in names:
        _check(params[k].grad, 2 * g1[k].double(), 4 * U * g1[k].double().abs() + 1e-300, "second call doubles %s" % k)
    assert all(torch.equal(a, b) for a, b in zip(stats, _stats(m)))
    # the directional derivative along the normalised st_layer gradient against the central difference of the GPU forward
    # (the plumbing check of tests/test_train_ctx_gpu.py, with its 10 % and for its reason)
    with torch.no_grad():
        norm = SR.norm2([g1[k] for k in names])
        w0 = {k: params[k].detach().clone() for k in names}
        s = 2e-2 / norm
        vals = []
        for sign in (1.0, -1.0):
            for k in names:
                params[k].copy_(w0[k] + sign * s * g1[k] / norm)
            assert m.refresh_weights(m.st_layer) > 0
            vals.append(losses.loss_fu(m(x, cb, None)[0], y).item())
        for k in names:
            params[k].copy_(w0[k])
        m.refresh_weights(m.st_layer)
    fd = (vals[0] - vals[1]) / (2 * s)
    print("%s: st_layer directional derivative: finite difference %.6e, <grad, D> %.6e, step %.3e" % (kind, fd, norm, s))
    assert abs(fd - norm) <= 0.10 * abs(norm)
    assert torch.equal(m(x, cb, None)[0], ref_out)                                        # the restored weights give the same bits
    assert {k: id(e) for k, e in m._engines.items()} == engines                           # no plan rebuilt


def _trained(m):
    mods = [m.rnn, m.conv_out_st, m.fucbst_layer, m.fust_layer, m.fucb_layer, m.cxt_cb_prior, *train.prior_nets(m).values(), m.st_layer]
    return mods, [p for mod in mods for p in mod.parameters()]


def test_adam_steps_over_seven_stages_keep_the_plans():
    """Host refresh in the default configuration, and host against device refresh with `model.winograd = False`: the device
    repack writes the host packer's bytes for every entry kind except the Winograd filter transforms of the recurrence, which
    it makes within one fp32 ulp (tests/test_repack_gpu.py) -- with them in the plan the state behind the recurrence
    is not bit-comparable between the two paths, whatever stage is trained.  The ST blocks have no Winograd entry; without
    Winograd in the plan every assertion here is bit for bit on both paths.  Device refresh in the default configuration runs
    too: the loss falls, `st_layer` moves, no plan is rebuilt, and everything in front of the recurrence (the `st1` and
    `prefuse` taps: the ST blocks, `fust_layer`, the prior path) equals a fresh model's bit for bit."""
    from iip_uavsal_saliency_amd import UAVSal
    x, cb, y = _step_inputs()
    outs = {}
    for device, wino in ((False, True), (True, True), (False, False), (True, False)):
        m = _model()
        m.winograd = wino
        mods, ps = _trained(m)
        opt = torch.optim.Adam(ps, lr=1e-4, betas=(0.9, 0.999), weight_decay=5e-5)
        st0 = [p.detach().clone() for p in m.st_layer.parameters()]
        before = m(x, cb, None)[0]
        first = None
        for _ in range(3):
            opt.zero_grad()
            loss, _, _ = train.recurrence_step(m, x, cb, None, y, **_kw(m))
            first = loss.item() if first is None else first
            engines = {k: id(e) for k, e in m._engines.items()}
            opt.step()
            assert m.refresh_weights(*mods, device=device) > 0
            after = m(x, cb, None)[0]
            assert {k: id(e) for k, e in m._engines.items()} == engines                   # the same engine objects
        last = losses.loss_fu(after, y).item()
        print("loss_fu on the group: %.6f before, %.6f after three Adam steps over seven stages (device=%r, winograd=%r)" % (first, last, device, wino))
        assert last < first and not torch.equal(before, after)
        assert all(not torch.equal(a, b) for a, b in zip(st0, m.st_layer.parameters()))   # st_layer moved
        fresh = UAVSal(time_dims=T_)
        fresh.load_state_dict(m.state_dict())
        fresh = fresh.to(DEV).eval()
        fresh.winograd = wino
        taps, ftaps = {}, {}
        got, got_st = m(x, cb, None, taps=taps)
        want, want_st = fresh(x, cb, None, taps=ftaps)
        assert torch.equal(taps["st1"], ftaps["st1"]) and torch.equal(taps["prefuse"], ftaps["prefuse"])      # in front of the recurrence
        if not (device and wino):                                # (behind it: the Winograd transforms, see above)
            assert torch.equal(got, want) and torch.equal(got_st[0], want_st[0])
        outs[device, wino] = (got.clone(), got_st[0].clone(), taps["st1"].clone())
    assert all(torch.equal(a, b) for a, b in zip(outs[False, False], outs[True, False]))                  # host and device refresh


def test_finetune_video_with_the_st_stage_is_the_manual_loop():
    from iip_uavsal_saliency_amd.stream import finetune_video
    n = 2 * T_ * 2
    frames = torch.from_numpy(synth.synth_frames_u8(n, H_, W_, 2)).to(DEV)
    gp = torch.from_numpy(synth.gauss_priors(1, H_ // 8, W_ // 8)[0]).to(DEV)
    op_ = torch.from_numpy(synth.ob_priors(1, H_ // 8, W_ // 8)[0]).to(DEV)
    loc = synth.synth_fix_points(n, 90, 130, 12, 9)
    fmap = np.rint(synth.synth_fix_maps(loc, 6.0) * 255).astype(np.uint8)
    fix_map, fix_loc = torch.from_numpy(fmap).to(DEV), torch.from_numpy(loc).to(DEV)
    stages = ("rnn", "decoder", "fuse", "fust", "ctx", "nets", "st")

    def make():
        m = _model()
        return m, torch.optim.Adam(_trained(m)[1], lr=1e-4, betas=(0.9, 0.999), weight_decay=5e-5)
    m, opt = make()
    seen = []
    real = train.recurrence_step

    def spy(model, x, cb, state, y, criterion, **kw):
        assert kw == {s: True for s in stages[1:]}
        seen.append((x.clone(), cb, y.clone()))                                    # (cb: the zero-stride views themselves)
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
    assert not torch.equal(m.st_layer[0].stconv_te.reduce_conv[0].weight.detach(), w0.st_layer[0].stconv_te.reduce_conv[0].weight.detach())
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(m.parameters(), m2.parameters()))


def test_st_without_its_preconditions_raises_by_name():
    x, cb, y = _step_inputs()
    m = _model()
    with pytest.raises(RuntimeError, match="st=True"):
        train.recurrence_step(m, x, cb, None, y, st=True)
    with pytest.raises(RuntimeError, match="st=True"):
        train.recurrence_step(m, x, cb, None, y, fuse=True, st=True)                      # priors: fust=True is needed too
    assert all(p.grad is None for p in m.parameters())
