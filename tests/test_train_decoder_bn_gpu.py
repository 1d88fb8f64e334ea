"""BatchNorm on batch statistics on the GPU (csrc/train_bn.hip; train.bn_stats / bn_apply / bn_bwd_sums / bn_bwd_apply / dw_wgrad,
train.decoder_forward_batch / decoder_backward_batch, recurrence_step(batch_stats=("decoder",)), stream.finetune_video) against
the float64 restatement tests/decoder_bn_ref64.py, which runs on the device in torch float64.  Bounds: its docstring.
Every stage is held against float64 of the fp32 tensors the device's stage read, the ReLU6 masks taken from the device's own
activation of the stored raw u (no element excluded).  Kernel shapes (T, H, W): (2,5,7) and (3,5,7), odd in both directions,
and (3,13,17): two slabs, the last one partial (the count is read from the library's own query); C in {1, 8, 1536}, dense and
pitched."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import losses, ops, synth, train
from iip_uavsal_saliency_amd.train import bn as B

import decoder_bn_ref64 as BR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ACTS = (BR.ACT_NONE, BR.ACT_RELU6, BR.ACT_SIGMOID)
KERNEL_CASES = [(c, s, False) for c in BR.CHANNELS for s in BR.KERNEL_SHAPES] + [(c, (3, 5, 7), True) for c in BR.CHANNELS]
KERNEL_IDS = ["C%d_%s%s" % (c, BR.name(s)[11:], "_pitched" if p else "") for c, s, p in KERNEL_CASES]


def _check(got, want, bound, what):
    err = (got.double() - want).abs()
    bound = bound + torch.zeros_like(err)
    worst = float((err / bound.clamp_min(1e-300)).max())
    print("%s: worst error / bound %.4f (max |err| %.3e, max |ref| %.3e)" % (what, worst, float(err.max()), float(want.abs().max())))
    assert torch.isfinite(got).all() and bool((err <= bound).all()), what
    return worst


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _one_ulp(got, want64, what):
    """`got` (fp32) is the float64 value rounded to fp32, or its neighbour"""
    want = want64.float()
    gap = torch.maximum((torch.nextafter(want, want + 1) - want).abs(), (want - torch.nextafter(want, want - 1)).abs())
    off = (got - want).abs()
    print("%s: %d of %d one ulp off" % (what, int((off > 0).sum()), off.numel()))
    assert bool((off <= gap).all()), what


def _f64(fold):
    return {k: getattr(fold, k).double() for k in ("mu", "var", "r", "s", "b")}


def _mask(u, fold):
    a = train.bn_apply(u, fold, "relu6")
    return (a > 0) & (a < 6)


# ------------------------------------------------------------------------------------------------ 1. kernels 1 to 4, teacher-forced
@lru_cache(maxsize=None)
def _kcase(c, shape, pitched):
    x = BR.bn_inputs(c, shape, ld=(c + 4 if c > 1 else 4) if pitched else None)
    t = {k: torch.as_tensor(v).to(DEV) for k, v in x.items()}
    t["u"], t["g"] = t["u"][..., :c], t["g"][..., :c]
    if pitched:
        assert ops._nhwc_view(t["u"])[1] > c
    return t


def _stats(t, running=False):
    rm, rv = (t["rm"].clone(), t["rv"].clone()) if running else (None, None)
    f = train.bn_stats(t["u"], t["gamma"], t["beta"], BR.BN_EPS, rm, rv, momentum=BR.MOMENTUM)
    return f, rm, rv


@pytest.mark.parametrize("c,shape,pitched", KERNEL_CASES, ids=KERNEL_IDS)
def test_bn_stats_and_running_update(c, shape, pitched):
    t = _kcase(c, shape, pitched)
    T, H, W = shape
    assert B.slabs(T, H, W) == (BR.slab_partition(T, H, W)[1], BR.slab_partition(T, H, W)[0])
    if shape == BR.SLAB_SHAPE:
        slabs, rows = B.slabs(T, H, W)
        assert slabs >= 2 and (T * H) % rows != 0                          # at least two slabs, a partial last one
    f, rm, rv = _stats(t, running=True)
    u64 = t["u"].double()
    want, bound = BR.stats(u64, t["gamma"].double(), t["beta"].double(), bounds=True)
    for k in ("mu", "var", "r", "s", "b"):
        _check(getattr(f, k), want[k], bound[k], "C=%d %s %s" % (c, BR.name(shape), k))
    wm, wv = BR.running(t["rm"].double(), t["rv"].double(), want["mu"], want["var"], T * H * W)
    _one_ulp(rm, wm, "running_mean")
    _one_ulp(rv, wv, "running_var")
    assert rm._version > 0 and not torch.equal(rm, t["rm"]) and not torch.equal(rv, t["rv"])
    f2, rm2, rv2 = _stats(t, running=True)                                  # the same bits on a second call
    assert all(_same(a, b) for a, b in zip(f, f2)) and _same(rm, rm2) and _same(rv, rv2)
    f3, _, _ = _stats(t)                                                    # without the buffers: the same fold
    assert all(_same(a, b) for a, b in zip(f, f3))


@pytest.mark.parametrize("c,shape,pitched", KERNEL_CASES, ids=KERNEL_IDS)
def test_bn_apply(c, shape, pitched):
    t = _kcase(c, shape, pitched)
    f, _, _ = _stats(t)
    for act in ACTS:
        out = train.bn_apply(t["u"], f, act)
        assert out.is_contiguous() and tuple(out.shape) == tuple(t["u"].shape)
        want, bound = BR.apply(t["u"].double(), _f64(f), act)
        _check(out, want, bound, "apply %s" % act)
        assert _same(out, train.bn_apply(t["u"], f, act))
    if c > 1:
        e = train.bn_apply(t["u"], f, "relu6")[..., 1:]                     # both clamps hold elements (channel 0 is constant)
        assert float((e <= 0).float().mean()) >= 0.05 and float((e >= 6).float().mean()) >= 0.05
        w = t["gamma"]
        out = train.bn_apply(t["u"], f, "relu6", dot_w=w)
        want, bound = BR.apply_dot(t["u"].double(), _f64(f), w.double())
        _check(out, want, bound, "apply_dot")
        assert _same(out, train.bn_apply(t["u"], f, "relu6", dot_w=w))


@pytest.mark.parametrize("c,shape,pitched", KERNEL_CASES, ids=KERNEL_IDS)
def test_bn_backward(c, shape, pitched):
    t = _kcase(c, shape, pitched)
    f, _, _ = _stats(t)
    f64, u64, g64 = _f64(f), t["u"].double(), t["g"].double()
    mask = _mask(t["u"], f)
    for act in ACTS:
        m = mask if act == BR.ACT_RELU6 else None
        gg, gb = torch.full((c,), 7.0, device=DEV), torch.full((c,), 7.0, device=DEV)
        sums = train.bn_bwd_sums(t["g"], t["u"], f, act, g_weight=gg, g_bias=gb)
        S, eS, eF = BR.bwd_sums(g64, u64, f64, act, mask=m, bounds=True)
        _check(sums, S, eS, "sums %s" % act)
        _check(gb, S[0], eF[0], "d beta %s" % act)
        _check(gg, S[1], eF[1], "d gamma %s" % act)
        again = train.bn_bwd_sums(t["g"], t["u"], f, act)
        assert _same(sums, again)
        train.bn_bwd_sums(t["g"], t["u"], f, act, g_weight=gg, g_bias=gb, accumulate=True)      # adds, rounding once more
        _check(gb, 2 * S[0], 2 * eF[0] + 2 * BR.U * S[0].abs(), "d beta accumulated")
        _check(gg, 2 * S[1], 2 * eF[1] + 2 * BR.U * S[1].abs(), "d gamma accumulated")
        gu = train.bn_bwd_apply(t["g"], t["u"], f, sums, act)
        want, bound = BR.bwd_apply(g64, u64, f64, sums, act, mask=m, bounds=True)
        _check(gu, want, bound, "g_u %s" % act)
        assert gu.is_contiguous() and _same(gu, train.bn_bwd_apply(t["g"], t["u"], f, sums, act))
        if c > 1:                                                           # gamma = 0: no gradient into u, a gamma gradient all the same
            assert float(gu[..., 0].abs().max()) == 0.0 and float(sums[1, 0].abs()) > 0.0 and float(gg[0].abs()) > 0.0
    if c > 1:                                                               # the rank-one gradient of a projection to one channel
        gp = t["g"][..., :1].contiguous()
        pair, pair64 = (gp, t["beta"]), (gp.double(), t["beta"].double())
        gw = torch.empty(c, device=DEV)
        sums = train.bn_bwd_sums(pair, t["u"], f, "relu6", g_w=gw)
        S, eS, eF = BR.bwd_sums(pair64, u64, f64, BR.ACT_RELU6, mask=mask, bounds=True)
        _check(sums, S[:2], eS[:2], "rank-one sums")
        _check(gw, S[2], eF[2], "rank-one projection weight gradient")
        gu = train.bn_bwd_apply(pair, t["u"], f, sums, "relu6")
        want, bound = BR.bwd_apply(pair64, u64, f64, sums, BR.ACT_RELU6, mask=mask, bounds=True)
        _check(gu, want, bound, "rank-one g_u")
        dense = (gp * t["beta"]).contiguous()                               # the same products, stored: the same bits
        assert _same(sums, train.bn_bwd_sums(dense, t["u"], f, "relu6"))
        assert _same(gu, train.bn_bwd_apply(dense, t["u"], f, sums, "relu6"))
        # the depthwise weight gradient, halo inside each frame
        e = train.bn_apply(t["u"], f, "relu6")
        out = train.dw_wgrad(t["g"], e)
        want, bound = BR.dw_wgrad(g64, e.double(), bounds=True)
        _check(out, want, bound, "dw_wgrad")
        assert _same(out, train.dw_wgrad(t["g"], e))
        if shape[0] > 1:
            wrong = BR.dw_wgrad(g64, e.double(), variant="across_frames")
            assert float(((out.double() - wrong).abs() / bound).max()) >= 4.0
        acc = out.clone()
        train.dw_wgrad(t["g"], e, out=acc, accumulate=True)
        _check(acc, 2 * want, 2 * bound + 2 * BR.U * want.abs(), "dw_wgrad accumulated")


# ------------------------------------------------------------------------------------------------ 2. the decoder at its real widths
def _block(q):
    from iip_uavsal_saliency_amd.model import dwBlock
    return BR.load_block(dwBlock(256, 1, kernel_size=3), q).to(DEV)


def _walk(block, h, gy, saved, parts, grads, grad_h, y, q):
    """Every stage of the device's forward and backward against float64 of what that stage read on the device.  `q`: the
    module's numbers as float64 tensors (weights, gamma, beta)."""
    hn = h.permute(0, 2, 3, 1).double()
    gyn = gy.permute(0, 2, 3, 1).double()
    u1, e, u2, u3 = (saved[k] for k in ("u1", "e", "u2", "u3"))
    f1, f2, f3 = (_f64(saved[k]) for k in ("f1", "f2", "f3"))
    w3 = q["w3"].reshape(-1)
    N = BR.NAMES
    worst = {}
    ck = lambda k, got, want, bound: worst.__setitem__(k, _check(got, want, bound, k))      # noqa: E731
    ck("u1", u1, *BR.conv1x1(hn, q["w1"]))
    for i, u, f in ((1, u1, saved["f1"]), (2, u2, saved["f2"]), (3, u3, saved["f3"])):
        want, bound = BR.stats(u.double(), q["g%d" % i], q["be%d" % i], bounds=True)
        for k in ("mu", "var", "r", "s", "b"):
            ck("%s%d" % (k, i), getattr(f, k), want[k], bound[k])
    ck("e", e, *BR.apply(u1.double(), f1, BR.ACT_RELU6))
    ck("u2", u2, *BR.dw_raw(e.double(), q["wd"]))
    ck("u3", u3, *BR.apply_dot(u2.double(), f2, w3))
    ck("y", y.permute(0, 2, 3, 1), *BR.apply(u3.double(), f3, BR.ACT_SIGMOID))
    m1 = (e > 0) & (e < 6)
    m2 = _mask(u2, saved["f2"])
    g_u1, g_u2, g_u3, g_e = (parts[k] for k in ("g_u1", "g_u2", "g_u3", "g_e"))
    S3, e3, e3f = BR.bwd_sums(gyn, u3.double(), f3, BR.ACT_SIGMOID, bounds=True)
    ck(N[8], grads[N[8]], S3[0], e3f[0])
    ck(N[7], grads[N[7]], S3[1], e3f[1])
    ck("g_u3", g_u3, *BR.bwd_apply(gyn, u3.double(), f3, S3, BR.ACT_SIGMOID, bounds=True, sums_err=e3))
    pair = (g_u3.double(), w3)
    S2, e2, e2f = BR.bwd_sums(pair, u2.double(), f2, BR.ACT_RELU6, mask=m2, bounds=True)
    ck(N[5], grads[N[5]], S2[0], e2f[0])
    ck(N[4], grads[N[4]], S2[1], e2f[1])
    ck(N[6], grads[N[6]].reshape(-1), S2[2], e2f[2])
    ck("g_u2", g_u2, *BR.bwd_apply(pair, u2.double(), f2, S2, BR.ACT_RELU6, mask=m2, bounds=True, sums_err=e2))
    ck(N[3], grads[N[3]], *BR.dw_wgrad(g_u2.double(), e.double(), bounds=True))
    ck("g_e", g_e, *BR.dw_raw(g_u2.double(), q["wd"], transpose=True))
    S1, e1, e1f = BR.bwd_sums(g_e.double(), u1.double(), f1, BR.ACT_RELU6, mask=m1, bounds=True)
    ck(N[2], grads[N[2]], S1[0], e1f[0])
    ck(N[1], grads[N[1]], S1[1], e1f[1])
    ck("g_u1", g_u1, *BR.bwd_apply(g_e.double(), u1.double(), f1, S1, BR.ACT_RELU6, mask=m1, bounds=True, sums_err=e1))
    ck(N[0], grads[N[0]].reshape(BR.HID, BR.C_IN), *BR.pix_gemm(g_u1.double(), hn))
    ck("grad_h", grad_h.permute(0, 2, 3, 1), *BR.conv1x1(g_u1.double(), q["w1"], transpose=True))
    return worst


@pytest.mark.parametrize("shape", BR.SHAPES, ids=BR.name)
def test_decoder_forward_and_backward_batch(shape):
    hn, qn, gyn = BR.decoder_case(shape)
    block = _block(qn)
    q = BR.to64(qn, DEV)
    h = torch.as_tensor(hn).to(DEV).contiguous(memory_format=torch.channels_last)
    gy = torch.as_tensor(gyn).to(DEV)
    T, H, W = shape
    bns = (block.conv[0][1], block.conv[1][1], block.conv[3])
    y, saved = train.decoder_forward_batch(block, h)
    assert tuple(y.shape) == (T, 1, H, W) and sorted(saved) == ["e", "f1", "f2", "f3", "u1", "u2", "u3"]
    parts = {}
    grad_h, grads = train.decoder_backward_batch(block, h, gy, saved=saved, parts=parts)
    assert tuple(grads) == BR.NAMES and tuple(grad_h.shape) == (T, 256, H, W)
    _walk(block, h, gy, saved, parts, grads, grad_h, y, q)
    for t in (saved["e"], train.bn_apply(saved["u2"], saved["f2"], "relu6")):      # both clamps of both ReLU6s hold elements
        lo, mid, hi = BR.clamp_shares(t)
        assert lo >= 0.05 and hi >= 0.02 and mid >= 0.25
    # the running statistics moved as torch moves them: float64 from the device's own u, rounded to fp32, one ulp
    for i, (bn, u) in enumerate(zip(bns, (saved["u1"], saved["u2"], saved["u3"])), 1):
        st = BR.stats(u.double(), q["g%d" % i], q["be%d" % i])
        wm, wv = BR.running(q["rm%d" % i], q["rv%d" % i], st["mu"], st["var"], T * H * W)
        _one_ulp(bn.running_mean, wm, "running_mean %d" % i)
        _one_ulp(bn.running_var, wv, "running_var %d" % i)
        assert int(bn.num_batches_tracked) == 1
    # the whole chain against the float64 closed form from the module's numbers (figures: the fp32 forward may decide a mask
    # the other way, which no bound of a single stage covers; the stage walk above is the assertion)
    ref = BR.decoder_train(q, torch.as_tensor(hn).to(DEV).double(), gy.double())
    for n in BR.NAMES + ("grad_h", "y"):
        got = {"grad_h": grad_h, "y": y}.get(n, grads.get(n))
        print("%s whole chain %s: relative L2 distance %.3e" % (BR.name(shape), n, float((got.double() - ref[n]).norm() / ref[n].norm())))
    c1, c2 = BR.ZERO_GAMMA                                                  # gamma = 0: no gradient into u, a gamma gradient
    assert float(parts["g_u1"][..., c1].abs().max()) == 0.0 and float(grads[BR.NAMES[1]][c1].abs()) > 0.0
    assert float(parts["g_u2"][..., c2].abs().max()) == 0.0 and float(grads[BR.NAMES[4]][c2].abs()) > 0.0
    # a second forward returns the same bits and moves the statistics again; without `saved` the backward runs the forward
    # itself and leaves the statistics alone; given gradient tensors are written in place, or added to
    y2, _ = train.decoder_forward_batch(block, h)
    assert _same(y, y2) and int(bns[0].num_batches_tracked) == 2
    before = [b.clone() for b in block.buffers()]
    mine = {n: torch.zeros_like(v) for n, v in grads.items()}
    gh2, same = train.decoder_backward_batch(block, h, gy, grads=mine)
    assert same is mine and _same(gh2, grad_h) and all(_same(mine[n], grads[n]) for n in BR.NAMES)
    assert all(torch.equal(a, b) for a, b in zip(before, block.buffers()))
    train.decoder_backward_batch(block, h, gy, saved=saved, grads=mine, accumulate=True)
    for n in BR.NAMES:
        _check(mine[n], 2 * grads[n].double(), 4 * BR.U * grads[n].double().abs(), "accumulate doubles %s" % n)
    with pytest.raises(RuntimeError, match="decoder_backward, decoder_input_grad and decoder_param_grads"):
        train.decoder_forward_batch(block.eval(), h)
    block.train()


# ------------------------------------------------------------------------------------------------ 3. the step and the driver
H_, W_, T_ = 72, 104, 4
RNN = "rnn.cell_list.0.rnn_conv.weight"
DEC = ["conv_out_st." + n for n in BR.NAMES]


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


def _model():
    from iip_uavsal_saliency_amd import UAVSal
    m = UAVSal(time_dims=T_)
    synth.load_synth_weights(m, 0)
    with torch.no_grad():                                       # running statistics that are not the initial 0 and 1
        g = torch.Generator().manual_seed(11)
        for bn in (m.conv_out_st.conv[0][1], m.conv_out_st.conv[1][1], m.conv_out_st.conv[3]):
            bn.running_mean.add_(0.05 * torch.randn(bn.running_mean.shape, generator=g))
            bn.running_var.mul_(1.0 + 0.2 * torch.rand(bn.running_var.shape, generator=g))
    return m.to(DEV).eval()


def _fresh_like(m):
    from iip_uavsal_saliency_amd import UAVSal
    f = UAVSal(time_dims=T_)
    f.load_state_dict(m.state_dict())
    return f.to(DEV).eval()


def test_recurrence_step_on_batch_statistics():
    m = _model()
    x, cb, y = _step_inputs()
    dec = m.conv_out_st
    taps = {}
    eval_out, _ = m(x, cb, None, taps=taps)
    h_seq = taps["rnn"].contiguous(memory_format=torch.channels_last)
    x_seq = taps["prefuse"].contiguous(memory_format=torch.channels_last)
    stats0 = {k: v.clone() for k, v in dec.state_dict().items() if "running" in k or "tracked" in k}
    with pytest.raises(RuntimeError, match=r"conv_out_st\.train\(\)"):     # the keyword with the decoder in eval mode
        train.recurrence_step(m, x, cb, None, y, decoder=True, batch_stats=("decoder",))
    dec.train()
    assert not m.training and dec.training and all(p.grad is None for p in m.parameters())
    loss, out, st = train.recurrence_step(m, x, cb, None, y, decoder=True, batch_stats=("decoder",))
    # out and the loss are decoder_forward_batch of the rnn tap
    want_y, saved = train.decoder_forward_batch(dec, h_seq, update_running=False)
    assert _same(out, want_y) and not torch.equal(out, eval_out) and loss.item() == losses.loss_fu(want_y, y).item()
    params = dict(m.named_parameters())
    assert sorted(k for k, p in params.items() if p.grad is not None) == sorted([RNN] + DEC)
    # the nine gradients and grad_h: the bits of decoder_backward_batch on the device's h_seq, every stage of which is within
    # its bound of float64
    pred = want_y.detach().requires_grad_(True)
    with torch.enable_grad():
        (g_y,) = torch.autograd.grad(losses.loss_fu(pred, y), pred)
    parts = {}
    grad_h, grads = train.decoder_backward_batch(dec, h_seq, g_y, saved=saved, parts=parts)
    g1 = {k: params[k].grad.clone() for k in [RNN] + DEC}
    for n in BR.NAMES:
        assert _same(g1["conv_out_st." + n], grads[n]), n
        assert float(grads[n].abs().max()) > 0 and torch.isfinite(grads[n]).all()
    q = {k: v.detach().double() for k, v in (("w1", dec.conv[0][0].weight), ("wd", dec.conv[1][0].weight), ("w3", dec.conv[2].weight))}
    for i, bn in ((1, dec.conv[0][1]), (2, dec.conv[1][1]), (3, dec.conv[3])):
        q["g%d" % i], q["be%d" % i] = bn.weight.detach().double(), bn.bias.detach().double()
    _walk(dec, h_seq, g_y, saved, parts, grads, grad_h, want_y, q)
    # the recurrence received that grad_h unchanged
    rc = m.rnn.cell_list[0].rnn_conv
    gw, _, _ = train.twa_backward(x_seq, h_seq, None, rc.weight.detach(), grad_h)
    assert _same(g1[RNN], gw)
    # the running statistics moved, by the rule, and the counter went up by one
    for i, bn in ((1, dec.conv[0][1]), (2, dec.conv[1][1]), (3, dec.conv[3])):
        pre = "conv.%s." % ("0.1", "1.1", "3")[i - 1]
        u = saved["u%d" % i].double()
        fs = BR.stats(u, q["g%d" % i], q["be%d" % i])
        wm, wv = BR.running(stats0[pre + "running_mean"].double(), stats0[pre + "running_var"].double(), fs["mu"], fs["var"],
                            u.shape[0] * u.shape[1] * u.shape[2], momentum=bn.momentum)
        _one_ulp(bn.running_mean, wm, "running_mean %d" % i)
        _one_ulp(bn.running_var, wv, "running_var %d" % i)
        assert not torch.equal(bn.running_mean, stats0[pre + "running_mean"])
        assert int(bn.num_batches_tracked) == int(stats0[pre + "num_batches_tracked"]) + 1
    # a second step with .grad present adds to it (the weights did not move; the batch path does not read the running statistics)
    train.recurrence_step(m, x, cb, None, y, decoder=True, batch_stats=("decoder",))
    for k in DEC:
        _check(params[k].grad, 2 * g1[k].double(), 4 * BR.U * g1[k].double().abs(), "second call doubles %s" % k)
    assert int(dec.conv[3].num_batches_tracked) == int(stats0["conv.3.num_batches_tracked"]) + 2


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_refresh_refolds_the_eval_forms_from_the_moved_statistics(device):
    """After a step on batch statistics and an optimiser step, `refresh_weights` -- on the host, and `device=True` -- refolds the
    decoder's eval-mode packed forms from the MOVED running statistics: the eval forward is that of a freshly built model
    loaded with the same `state_dict`, bit for bit, and the plans were kept.  One thing of the device path is not the host
    packer's bytes by design, whatever was trained: the Winograd transform of the recurrence's 3x3 weight (csrc/repack.hip:
    within one fp32 ulp, tests/test_repack_gpu.py), so in the device case the fresh model's recurrence is refreshed on the
    device as well -- its decoder entries stay the host packer's, which is what the comparison is about."""
    m = _model()
    x, cb, y = _step_inputs()
    before, _ = m(x, cb, None)                                             # packs the weights, builds the plan
    m.conv_out_st.train()
    opt = torch.optim.Adam(list(m.rnn.parameters()) + list(m.conv_out_st.parameters()), lr=1e-4)
    train.recurrence_step(m, x, cb, None, y, decoder=True, batch_stats=("decoder",))
    engines = dict(m._engines)
    opt.step()
    assert m.refresh_weights(m.rnn, m.conv_out_st, device=device) > 0
    m.conv_out_st.eval()
    got, got_st = m(x, cb, None)
    assert {k: id(e) for k, e in m._engines.items()} == {k: id(e) for k, e in engines.items()}      # the plans were kept
    fresh = _fresh_like(m)
    if device:
        fresh(x, cb, None)
        assert fresh.refresh_weights(fresh.rnn, device=True) > 0
    want, want_st = fresh(x, cb, None)
    assert not torch.equal(got, before)
    assert torch.equal(got, want) and torch.equal(got_st[0], want_st[0])


def test_without_the_keyword_the_step_is_the_eval_mode_step():
    m = _model()
    x, cb, y = _step_inputs()
    stats = [b.clone() for b in m.conv_out_st.buffers()]
    loss, out, st = train.recurrence_step(m, x, cb, None, y, decoder=True, batch_stats=())
    taps = {}
    ref_out, ref_st = m(x, cb, None, taps=taps)
    assert torch.equal(out, ref_out) and torch.equal(st[0], ref_st[0]) and loss.item() == losses.loss_fu(ref_out, y).item()
    pred = ref_out.detach().requires_grad_(True)
    with torch.enable_grad():
        (g_y,) = torch.autograd.grad(losses.loss_fu(pred, y), pred)
    _, grads = train.decoder_backward(m.conv_out_st, taps["rnn"].contiguous(memory_format=torch.channels_last), g_y, y=ref_out)
    params = dict(m.named_parameters())
    assert all(_same(params["conv_out_st." + n].grad, grads[n]) for n in BR.NAMES)
    assert all(torch.equal(a, b) for a, b in zip(stats, m.conv_out_st.buffers()))                    # nothing moved
    m.conv_out_st.train()
    with pytest.raises(RuntimeError, match="eval"):                        # and a decoder in training mode still raises
        train.recurrence_step(m, x, cb, None, y, decoder=True)
    m.conv_out_st.eval()


def test_finetune_video_on_batch_statistics_restores_the_mode():
    from iip_uavsal_saliency_amd.stream import finetune_video, validate_video
    n = 2 * T_ * 3
    frames = torch.from_numpy(synth.synth_frames_u8(n, H_, W_, 2)).to(DEV)
    gp = torch.from_numpy(synth.gauss_priors(1, H_ // 8, W_ // 8)[0]).to(DEV)
    op_ = torch.from_numpy(synth.ob_priors(1, H_ // 8, W_ // 8)[0]).to(DEV)
    loc = synth.synth_fix_points(n, 90, 130, 12, 9)
    fmap = np.rint(synth.synth_fix_maps(loc, 6.0) * 255).astype(np.uint8)
    fix_map, fix_loc = torch.from_numpy(fmap).to(DEV), torch.from_numpy(loc).to(DEV)
    m = _model()
    opt = torch.optim.Adam(list(m.rnn.parameters()) + list(m.conv_out_st.parameters()), lr=1e-4, betas=(0.9, 0.999), weight_decay=5e-5)
    nbt = int(m.conv_out_st.conv[3].num_batches_tracked)
    rm0 = m.conv_out_st.conv[0][1].running_mean.clone()
    res = finetune_video(m, frames, gp, op_, fix_map, fix_loc, opt, batch_size=2, stages=("rnn", "decoder"), batch_stats=("decoder",))
    assert res["groups_run"] == 3 and torch.isfinite(res["losses"]).all()
    assert not m.training and not m.conv_out_st.training and not any(b.training for b in m.conv_out_st.modules())
    assert int(m.conv_out_st.conv[3].num_batches_tracked) == nbt + 3 and not torch.equal(m.conv_out_st.conv[0][1].running_mean, rm0)
    # the eval forward afterwards is that of a freshly built model with the same state: validation stays on running statistics
    val = validate_video(m, frames, gp, op_, fix_map, fix_loc, batch_size=2)
    ref = validate_video(_fresh_like(m), frames, gp, op_, fix_map, fix_loc, batch_size=2)
    assert torch.equal(val["losses"], ref["losses"])
    assert int(m.conv_out_st.conv[3].num_batches_tracked) == nbt + 3
