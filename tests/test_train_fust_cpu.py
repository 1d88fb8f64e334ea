"""Fine-tuning fust_layer behind the priors, without a GPU: the C ABI of csrc/train_ctx.hip, what the Python entry points and
the driver refuse, the GEMM routes `block_input_grad` sends, the `cb192` tap, the float64 restatements of tests/ctx_ref64.py
against torch autograd, and the conditions under which the GPU tests are meaningful: each wrong variant lies at least 4
bounds from the right result in the float64 reference alone.

The variant "a bilinear adjoint that counts a border pixel once where y0 == y1" is NOT among them and cannot be: in exact
arithmetic ly == 0 wherever y0 == y1 (`test_border_weight_is_whole_in_exact_arithmetic`), so that adjoint equals the right one
in any float64 reference, and in fp32 it differs by ly <= one step of fy, which is below the coordinate term every bound
against an exact-coordinate reference must carry (ctx_ref64's docstring).  What the reference does tell apart -- an adjoint
that drops the border pixel, or counts its whole weight twice -- is held to the 4 bounds instead, and the GPU test compares
the two resizes whose weights are exactly 0 and 1 for equality."""
import ctypes as C

import pytest
import torch

from iip_uavsal_saliency_amd import _lib, stream, train
from iip_uavsal_saliency_amd import packing as P

import block_ref64 as BR
import ctx_ref64 as X

W1 = BR.NAMES[0]


def t64(a):
    return torch.as_tensor(a, dtype=torch.float64)


@pytest.fixture(scope="module")
def lib():
    from iip_uavsal_saliency_amd import build
    build.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ the C ABI
def test_symbols_and_sizes(lib):
    names = [s[0] for s in _lib.SYMBOLS]
    for n in ("uavsal_ir_bwd_s2", "uavsal_bilinear_ac_bwd", "uavsal_tsum_bwd", "uavsal_ctx_sizeof_desc"):
        assert n in names and hasattr(lib, n)
    assert _lib.CTX_DESC_TYPES == [_lib.IrBwdS2Desc, _lib.BilinearBwdDesc, _lib.TsumBwdDesc]
    for i, t in enumerate(_lib.CTX_DESC_TYPES):
        assert lib.uavsal_ctx_sizeof_desc(i) == C.sizeof(t)
    assert lib.uavsal_ctx_sizeof_desc(3) < 0 and lib.uavsal_ctx_sizeof_desc(-1) < 0
    assert lib.uavsal_block_sizeof_desc(3) < 0 and lib.uavsal_abi_version() == 20             # the older lists stay closed
    assert len(_lib.DESC_TYPES) == 20 and lib.uavsal_sizeof_desc(20) < 0
    for n in ("ir_bwd_s2", "bilinear_bwd", "tsum_bwd", "block_input_grad", "fust_output_grad"):
        assert callable(getattr(train, n))


def test_argument_validation_without_gpu(lib):
    b = _lib.IrBwdS2Desc()
    assert lib.uavsal_ir_bwd_s2(C.byref(b), None) == -1
    b.gd = b.d = b.e = b.wd9 = b.s2 = b.ga = 256
    b.n_img, b.H, b.W, b.C = 1, 5, 5, 1922
    assert lib.uavsal_ir_bwd_s2(C.byref(b), None) == -3                  # C % 4: UAVSAL_ESHAPE
    b.C, b.e = 1920, 260
    assert lib.uavsal_ir_bwd_s2(C.byref(b), None) == -2
    b.e, b.W = 256, 0
    assert lib.uavsal_ir_bwd_s2(C.byref(b), None) == -1
    u = _lib.BilinearBwdDesc()
    assert lib.uavsal_bilinear_ac_bwd(C.byref(u), None) == -1
    u.gout = u.gin = 256
    u.ldo, u.Ho, u.Wo, u.Hi, u.Wi, u.n_out, u.n_src, u.C, u.src_mod, u.src_div = 64, 9, 16, 3, 4, 4, 1, 64, 2, 1
    assert lib.uavsal_bilinear_ac_bwd(C.byref(u), None) == -1            # the tile map reads source image 1: n_src too small
    u.n_src, u.src_div = 2, 0
    assert lib.uavsal_bilinear_ac_bwd(C.byref(u), None) == -1
    u.src_div, u.ldo = 1, 32
    assert lib.uavsal_bilinear_ac_bwd(C.byref(u), None) == -2            # rows shorter than C
    u.ldo, u.C = 64, 62
    assert lib.uavsal_bilinear_ac_bwd(C.byref(u), None) == -2
    u.C, u.gin = 64, 260
    assert lib.uavsal_bilinear_ac_bwd(C.byref(u), None) == -2
    t = _lib.TsumBwdDesc()
    assert lib.uavsal_tsum_bwd(C.byref(t), None) == -1
    t.a = t.g = t.out = 256
    t.lda, t.ldg, t.ldo, t.n_groups, t.T, t.HW, t.C = 320, 256, 256, 2, 0, 35, 256
    assert lib.uavsal_tsum_bwd(C.byref(t), None) == -1                   # T
    t.T, t.ldg = 2, 128
    assert lib.uavsal_tsum_bwd(C.byref(t), None) == -2
    t.ldg, t.lda = 256, 322
    assert lib.uavsal_tsum_bwd(C.byref(t), None) == -2
    t.lda, t.g = 320, 264
    assert lib.uavsal_tsum_bwd(C.byref(t), None) == -2


# ------------------------------------------------------------------------------------------------ refusals
def _blk(name, shape=(1, 3, 5)):
    from iip_uavsal_saliency_amd.model import dwBlock
    return X.make_block(name, X.block_case(name, shape)[1], dwBlock)


def test_python_entry_points_refuse_what_they_do_not_cover():
    from iip_uavsal_saliency_amd import UAVSal
    from iip_uavsal_saliency_amd.model import dwBlock
    blk = _blk("ctx0")
    assert blk.stride == 2 and not blk.use_res_connect and _blk("fucb64").use_res_connect and not _blk("fucb192").use_res_connect
    assert len(train._input_grad_parts(blk)) == 6
    x, g = torch.zeros(2, 256, 5, 7), torch.zeros(2, 64, 3, 4)
    with pytest.raises(RuntimeError, match="cuda"):
        train.block_input_grad(blk, x, g)
    with pytest.raises(RuntimeError, match="eval"):
        train.block_input_grad(blk.train(), x, g)
    for bad in (dwBlock(256, 64, kernel_size=3, expand_ratio=1), dwBlock(256, 64, kernel_size=3, dilation=6),
                dwBlock(20, 64, kernel_size=3), dwBlock(256, 8, kernel_size=3)):
        with pytest.raises(RuntimeError, match="expand conv|Cout"):
            train.block_input_grad(bad.eval(), x, g)
    with pytest.raises(RuntimeError, match="expand conv"):                # block_backward keeps refusing stride 2 and Cout = 64
        train.block_backward(blk.eval(), x, g)
    with pytest.raises(RuntimeError, match="Cout"):
        train.block_backward(_blk("fucb192"), torch.zeros(2, 192, 5, 7), torch.zeros(2, 64, 5, 7))
    t = torch.zeros(1, 4, 4, 64)
    with pytest.raises(RuntimeError, match="cuda"):
        train.ir_bwd_s2(torch.zeros(1, 2, 2, 64), torch.zeros(1, 2, 2, 64), t, torch.zeros(9, 64), torch.zeros(64))
    with pytest.raises(RuntimeError, match="cuda"):
        train.bilinear_bwd(t, 1, 2, 2)
    with pytest.raises(RuntimeError, match="cuda"):
        train.tsum_bwd(t, t, 1)
    m = UAVSal(time_dims=2).eval()
    fu, cb, gf = torch.zeros(4, 320, 5, 7), torch.zeros(4, 192, 5, 7), torch.zeros(4, 320, 5, 7)
    with pytest.raises(RuntimeError, match="cuda"):
        train.fust_output_grad(m, fu, cb, gf)
    with pytest.raises(RuntimeError, match="eval"):
        train.fust_output_grad(m.train(), fu, cb, gf)
    m.eval()
    m0 = UAVSal(time_dims=2, bias_type=[0, 0, 0]).eval()
    with pytest.raises(RuntimeError, match="prior"):
        train.fust_output_grad(m0, fu, cb, gf)
    for model, kw in ((m, dict(fust=True)), (m, dict(decoder=True, fust=True)), (m0, dict(fuse=True, fust=True))):
        with pytest.raises(RuntimeError, match="fuse=True and a model with at least one prior"):
            train.recurrence_step(model, fu, None, None, fu, **kw)
    with pytest.raises(RuntimeError, match="eval"):
        train.recurrence_step(m.train(), fu, None, None, fu, fuse=True, fust=True)
    with pytest.raises(RuntimeError, match="cuda"):
        train.recurrence_step(m.eval(), fu, None, None, fu, fuse=True, fust=True)


def test_stages_of_the_driver():
    for stages in (("rnn", "fust"), ("rnn", "decoder", "fust"), ("rnn", "fust", "fuse"), ("rnn", "fuse", "fust", "fust"),
                   ("rnn", "fuse", "decoder", "fust"), ("fust",), ("fuse", "fust"),
                   ("decoder",), ("fuse",), ("rnn", "fuse", "decoder"), ("rnn", "fuse", "fuse"), ()):
        with pytest.raises(ValueError, match="stages"):
            stream.finetune_video(None, None, None, None, None, None, None, stages=stages)


class _Stub:
    time_dims = 5

    def __init__(self):
        self.rnn, self.conv_out_st, self.fucbst_layer, self.fust_layer = object(), object(), object(), object()
        self.num_cb, self.refreshed = 3, []
        self.w = torch.nn.Parameter(torch.zeros(1))

    def parameters(self):
        return iter([self.w])

    def refresh_weights(self, *mods):
        self.refreshed.append(mods)


class _Opt:
    def zero_grad(self):
        pass

    def step(self):
        pass


def test_finetune_video_with_the_fust_stage(monkeypatch):
    n = 20
    frames = torch.zeros(n, 3, 72, 128, dtype=torch.uint8)
    has = torch.ones(n, 2, dtype=torch.bool)
    seen = []

    def step(model, x, cb, state, y, criterion, **kw):
        seen.append(kw)
        return torch.tensor(1.0), None, [torch.tensor(0.0)]
    monkeypatch.setattr(train, "recurrence_step", step)
    fix = torch.zeros(n, 4, 4, dtype=torch.uint8)
    for stages, kw in ((("rnn", "decoder", "fuse", "fust"), {"decoder": True, "fuse": True, "fust": True}),
                       (("rnn", "fuse", "fust"), {"fuse": True, "fust": True})):
        m = _Stub()
        del seen[:]
        r = stream.finetune_video(m, frames, torch.zeros(8, 9, 16), torch.zeros(20, 9, 16), fix, fix, _Opt(), batch_size=2,
                                  criterion=object(), prepare=lambda a, b, h, w, l: (torch.zeros(n, 2, h, w), has), stages=stages)
        assert r["groups_run"] == 2 and seen == [kw] * 2
        want = (m.rnn,) + ((m.conv_out_st,) if "decoder" in stages else ()) + (m.fucbst_layer, m.fust_layer)
        assert m.refreshed == [want] * 2


# ------------------------------------------------------------------------------------------------ routes and taps
def test_every_gemm_of_the_frozen_path_has_a_route(lib):
    """The 1x1 GEMMs block_input_grad sends (Co -> Ch with the transposed projection, Ch -> Cin with the transposed expand) at
    the map sizes of the path: the library's own table takes each of them, and the weight packer has the layout."""
    sent = set()
    for name in X.FROZEN:
        cin, hid, cout, _ = X.BLOCKS[name]
        sent |= {(cout, hid), (hid, cin)}
    assert sent == {(64, 1152), (1152, 192), (64, 768), (768, 128), (64, 384), (384, 64), (64, 1536), (1536, 256)}
    for (ci, co) in sorted(sent):
        for (n, h, w) in ((20, 45, 80), (2, 45, 80), (2, 23, 40), (2, 12, 20), (1, 3, 5), (1, 1, 1)):
            d = _lib.ConvDesc()
            d.a, d.lda, d.a_img_stride = 1 << 20, ci, h * w
            d.out, d.ldc, d.o_img_stride = 1 << 21, co, h * w
            d.n_img, d.H, d.W, d.Cin, d.Cout, d.taps = n, h, w, ci, co, 1
            d.prec, d.act, d.epi, d.tile = _lib.PREC["f32"], _lib.ACT_NONE, _lib.EPI_AFFINE, 0
            d.w = 1 << 20
            rt = _lib.conv_route(lib, d)
            layout = P.conv_weight_layout("f32", False, False, rt.tile, 1)
            wp = P.pack_conv_weight(torch.zeros(co, ci, 1, 1), layout)
            assert wp.numel() >= ci * co, (ci, co, rt)


def test_cb192_is_a_tap_on_request_and_stays_live_in_taps_plans():
    from iip_uavsal_saliency_amd import UAVSal
    from iip_uavsal_saliency_amd.engine import Engine
    assert Engine.TAPS_ON_REQUEST == ("fu320", "cb192") and "cb192" not in Engine.TAP_NAMES
    kw = dict(n_seq=1, seq_len=4, H=96, W=160, ctx_T=4, ctx_mode="tile", plan_only=True)
    for bias in ([1, 1, 1], [0, 0, 1]):
        m = UAVSal(time_dims=4, bias_type=bias).eval()
        last = {}
        for taps in (False, True):
            e = Engine(m, "cpu", taps=taps, **kw)
            lay = {t[0]: t for t in e.arena_layout()}
            last[taps] = {k: lay[k][4] for k in ("cb192", "fu320", "prefuse", "rnn")}
        assert last[True]["cb192"] == last[True]["fu320"] == last[True]["rnn"] == last[True]["prefuse"], (bias, last)
        if bias == [0, 0, 1]:                                             # not pinned: without taps it dies at fucb
            assert last[False]["cb192"] < last[False]["fu320"] <= last[False]["prefuse"], last


# ------------------------------------------------------------------------------------------------ restatements vs autograd
def _close(a, b, rel=1e-12):
    assert a.shape == b.shape and float((a - b).abs().max()) <= rel * max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("shape", [(1, 1, 1, 8), (1, 2, 3, 8), (2, 5, 6, 8), (1, 4, 4, 8), (1, 7, 3, 8)], ids=str)
def test_ir_bwd_s2_restatement_is_the_formula_and_autograd(shape):
    gd, d, e, wd, s2 = (t64(a) for a in X.s2_case(shape))
    ref = X.ir_bwd_s2_ref(wd, s2, gd, d, e)
    _close(ref, X.ir_bwd_s2_formula(wd, s2, gd, d, e))
    # autograd of the stride-2 depthwise conv itself: d a2 / d e, with both masks applied by hand
    ee = e.clone().requires_grad_(True)
    pre = torch.nn.functional.conv2d(ee, wd, padding=1, stride=2, groups=wd.shape[0]) * s2.view(1, -1, 1, 1)
    assert pre.shape == d.shape
    (g,) = torch.autograd.grad(pre, ee, gd * X.m6(d))
    _close(ref, g * X.m6(e))
    if e.numel() >= 400:                                                 # all three classes of both ReLU6s
        for t in (e, d):
            assert min(BR.class_shares(t)) > 0.05, BR.class_shares(t)


@pytest.mark.parametrize("hw", X.BIL_SHAPES, ids=str)
@pytest.mark.parametrize("fmap", list(X.MAPS))
def test_bilinear_restatement_is_autograd_and_an_adjoint(hw, fmap):
    (hi, wi), (ho, wo) = hw
    src_mod, src_div, n_src = X.MAPS[fmap]
    g = t64(X.bil_case((hi, wi), (ho, wo), C=8))
    x = torch.randn(n_src, 8, hi, wi, dtype=torch.float64, generator=torch.Generator().manual_seed(3), requires_grad=True)
    y = X.bilinear_fwd_ref(x, ho, wo, src_mod, src_div, 4)
    (want,) = torch.autograd.grad(y, x, g)
    got, bound = X.bilinear_bwd_ref(g, n_src, hi, wi, src_mod, src_div, bounds=True)
    _close(got, want)
    y, x = y.detach(), x.detach()
    assert abs(float((y * g).sum()) - float((x * got).sum())) <= 1e-12 * float((y * g).abs().sum())
    assert bool((bound >= X.EPS * got.abs()).all())
    if fmap == "tile":                                                   # model.py:361: repeat(T, 1, 1, 1) of B = 2 chunks, T = 2
        up = torch.nn.functional.interpolate(x, size=(ho, wo), mode="bilinear", align_corners=True).repeat(2, 1, 1, 1)
        assert torch.equal(up, y)


@pytest.mark.parametrize("name", X.FROZEN)
def test_input_grad_restatement_is_autograd(name):
    for shape in ((1, 3, 5), (2, 5, 6)):
        x, q, go = X.block_case(name, shape)
        p = BR.fold(BR.to64(q))
        cin, _, cout, stride = X.BLOCKS[name]
        res = stride == 1 and cin == cout
        want = X.input_grad_autograd(p, t64(x), t64(go), stride, res)
        _close(X.input_grad_ref(p, t64(x), t64(go), stride, res), want)
        gx, bound, und = X.input_grad_e2e(p, t64(x), t64(go), stride, res)
        _close(gx, want)
        assert bool((bound > 0).all()) and bool((und >= 0).all())
        f = X.forward(p, t64(x), stride, res)
        for k in ("e", "d"):                                             # all three classes of both ReLU6s
            shares = BR.class_shares(f[k])
            assert min(shares) >= 0.01, (name, shape, k, shares)
        blk = _blk(name, shape)                                          # the module's own fold is the case's
        pm = X.fold_module(blk)
        for k in ("s1", "b1", "s2", "b2", "s3", "b3"):
            assert float((pm[k] - p[k]).abs().max()) <= 1e-6 * float(p[k].abs().max()), k


HEAD = (4, 5, 7)                    # N = 4 frames as B = 2 chunks of T = 2


def _head(bias):
    Q, st, priors, go = X.head_case(bias, HEAD, 2)
    return X.folds(Q), Q, t64(st), (t64(priors) if priors is not None else None), t64(go)


@pytest.mark.parametrize("bias", [(1, 1, 1), (0, 0, 1), (1, 0, 1), (1, 1, 0)], ids=str)
def test_fust_output_grad_restatement_is_autograd(bias):
    Pf, _, st, priors, go = _head(bias)
    hd = X.head_forward(Pf, st, priors, 2, use_ctx=bool(bias[2]))
    f = hd["f"].detach().clone().requires_grad_(True)
    (want,) = torch.autograd.grad(X.tail_forward(Pf, f, priors, 2, use_ctx=bool(bias[2]))["o"], f, go)
    gfu = X.input_grad_ref(Pf["fucbst"], hd["fu"], go, 1, False)
    if bias[2]:
        got, bound, und = X.fust_output_grad_ref(Pf, hd["fu"], hd["cbcat"], gfu, 2, bias[0] + bias[1])
        assert bool((bound >= 0).all()) and bool((und >= 0).all())
    else:
        got = gfu[:, :256]
    _close(got, want, 1e-11)
    # ... and the nine gradients of fust from it are autograd's through the whole head
    q = BR.to64(X.head_case(bias, HEAD, 2)[0]["fust"])
    mine = BR.param_grads(q, st, got)
    keys = ("w1", "g1", "be1", "wd", "g2", "be2", "w3", "g3", "be3")
    leaves = {k: q[k].detach().clone().requires_grad_(True) for k in keys}
    qq = dict(q)
    qq.update(leaves)
    Pl = dict(Pf)
    Pl["fust"] = BR.fold(qq)
    o = X.head_forward(Pl, st, priors, 2, use_ctx=bool(bias[2]))["o"]
    auto = torch.autograd.grad(o, [leaves[k] for k in keys], go)
    for n, a in zip(BR.NAMES, auto):
        _close(mine[n], a, 1e-10)


@pytest.mark.parametrize("shape", X.GOLDEN_SHAPES, ids=str)
@pytest.mark.parametrize("bias", X.GOLDEN_BIAS, ids=str)
def test_closed_form_matches_the_reference_autograd(bias, shape, golden_dir):
    """tests/golden/fust_*.npz: the reference's own dwBlock through model.py:344-365 under autograd (tools/make_fust_goldens.py)."""
    import os
    import numpy as np
    g = np.load(os.path.join(golden_dir, X.golden_name(bias, shape) + ".npz"))
    Q, st, priors, go = X.head_case(bias, shape, X.GOLDEN_T)
    assert str(g["digest"]) == X.head_digest(Q, st, priors, go) and int(g["T"]) == X.GOLDEN_T
    Pf = X.folds(Q)
    hd = X.head_forward(Pf, t64(st), t64(priors) if priors is not None else None, X.GOLDEN_T)
    gfu = X.input_grad_ref(Pf["fucbst"], hd["fu"], t64(go), 1, False)
    gf = X.fust_output_grad_ref(Pf, hd["fu"], hd["cbcat"], gfu, X.GOLDEN_T, bias[0] + bias[1])[0]

    def close(a, b):
        assert float(np.abs(a - b).max()) <= 1e-10 * float(np.abs(b).max())
    close(gfu.numpy()[BR.GX_SUBSET], g["grad_fu"])
    close(gf.numpy()[BR.GX_SUBSET], g["grad_f"])
    got = BR.param_grads(BR.to64(Q["fust"]), t64(st), gf)
    for n in BR.NAMES:
        if n not in (BR.NAMES[0], BR.NAMES[6]):
            close(got[n].numpy(), g[n.replace(".", "_")])
    for key, n in (("W1", BR.NAMES[0]), ("W3", BR.NAMES[6])):
        w = got[n].numpy()[:, :, 0, 0]
        close(w[BR.W_SUBSET], g[key])
        assert abs(float(w.sum()) - float(g[key + "_sum"])) <= 1e-10 * float(g[key + "_l2"]) * np.sqrt(w.size)
        assert abs(float(np.sqrt((w * w).sum())) - float(g[key + "_l2"])) <= 1e-10 * float(g[key + "_l2"])


# ------------------------------------------------------------------------------------------------ sensitivity
@pytest.mark.parametrize("bias", [(1, 1, 1), (0, 0, 1)], ids=str)
def test_wrong_paths_lie_outside_the_bounds_of_their_stage(bias):
    """The GPU test holds every stage of the path to ITS OWN bound, handed what the device handed that stage (a bound
    composed over the three frozen blocks is worthless: every absolute-value chain is ~100 times its value, the figures are
    printed below).  Under those checks
      * the direct path alone is a result whose last stage added nothing: it passes only if the gradient of the chunk sum is
        within its stage's bound of ZERO, so that gradient must be at least 4 bounds large somewhere;
      * the clip map where the tile map belongs (B = 2 chunks of T = 2 frames, distinct by construction) must move the
        resize's adjoint by at least 4 of ITS bounds somewhere.
    Both also move fust's W1 gradient by a sizeable part of itself (printed)."""
    Pf, Q, st, priors, go = _head(bias)
    k = bias[0] + bias[1]
    q = BR.to64(Q["fust"])
    hd = X.head_forward(Pf, st, priors, 2)
    gfu = X.input_grad_ref(Pf["fucbst"], hd["fu"], go, 1, False)
    S = X.path_stages(Pf, hd["fu"], hd["cbcat"], gfu, 2, k)
    g_s, b_s, u_s = S["g_sum"]
    ratio = float((g_s.abs() / (b_s + u_s)).max())
    print("%s direct_only: the chunk-sum gradient is up to %.1f of its stage's bounds from zero" % (bias, ratio))
    assert ratio >= 4.0
    g_c2, b_c2 = S["g_ctx2"]
    csum = hd["fu"][:, :256].reshape(2, 2, 256, *HEAD[1:]).sum(1)
    assert float((csum[0] - csum[1]).abs().max()) > 0.1                  # distinct chunks
    wrong = X.bilinear_bwd_ref(S["g_cb"][0][:, 64 * k:64 * k + 64], 2, 2, 2, 2, 1, variant="clip_map")
    ratio = float(((wrong - g_c2).abs() / b_c2).max())
    print("%s clip_map: the resize's adjoint is up to %.1f of its bounds from the right one" % (bias, ratio))
    assert ratio >= 4.0
    right = BR.param_grads(q, st, S["g"])[W1]
    for v in ("direct_only", "clip_map"):
        gw = X.fust_output_grad_ref(Pf, hd["fu"], hd["cbcat"], gfu, 2, k, variant=v)[0]
        rel = float((BR.param_grads(q, st, gw)[W1] - right).norm() / right.norm())
        print("%s %s: moves fust's W1 gradient by %.3f of its L2 norm" % (bias, v, rel))
        assert rel >= 0.05
    _, bnd, und = X.fust_output_grad_ref(Pf, hd["fu"], hd["cbcat"], gfu, 2, k)
    print("%s: composed bound / |g| up to %.2e (own last stage: %.2e)" % (
        bias, float(((bnd + und) / S["g"].abs().clamp_min(1e-30)).median()), float(((b_s + u_s) / g_s.abs().clamp_min(1e-30)).median())))


@pytest.mark.parametrize("shape", X.S2_SHAPES[:3] + [(1, 9, 8, 64)], ids=str)
def test_stride1_parity_lies_outside_the_bound(shape):
    gd, d, e, wd, s2 = (t64(a) for a in X.s2_case(shape))
    right, bound = X.ir_bwd_s2_ref(wd, s2, gd, d, e), X.ir_bwd_s2_bound(wd, s2, gd, d, e)
    wrong = X.ir_bwd_s2_ref(wd, s2, gd, d, e, variant="stride1_parity")
    far = ((wrong - right).abs() >= 4 * bound) & (bound > 0)
    assert bool(far.any()), shape


def test_border_weight_is_whole_in_exact_arithmetic():
    for (hi, wi), (ho, wo) in X.BIL_SHAPES + [((12, 20), (45, 80)), ((6, 10), (23, 40))]:
        assert X.border_once_is_invisible(hi, ho) and X.border_once_is_invisible(wi, wo)


@pytest.mark.parametrize("hw", X.BIL_SHAPES, ids=str)
def test_wrong_border_handling_lies_outside_the_bound(hw):
    (hi, wi), (ho, wo) = hw
    g = t64(X.bil_case((hi, wi), (ho, wo)))
    right, bound = X.bilinear_bwd_ref(g, 2, hi, wi, 2, 1, bounds=True)
    for v in ("border_dropped", "border_twice", "clip_map"):
        wrong = X.bilinear_bwd_ref(g, 2, hi, wi, 2, 1, variant=v)
        assert float(((wrong - right).abs() / bound.clamp_min(1e-300)).max()) >= 4.0, v
