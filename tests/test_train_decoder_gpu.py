"""The decoder's parameter gradients on the GPU (train.decoder_param_grads / decoder_backward / recurrence_step(decoder=True),
csrc/train_decoder.hip) against the float64 closed form tests/decoder_ref64.py, which runs on the device in torch float64,
and the reference's recorded autograd results (tests/golden/decoder_*.npz).  Bounds: decoder_ref64's docstring.
The kernels are tested teacher-forced: e, d, y, ga are the float64 restatement's, rounded to fp32 (`teacher_round`: the
stored value decides every mask as the float64 one does).
Shapes (T, H, W): train_ref64.SHAPES -- (2,45,80) is also decoder_ref64.SLAB_SHAPE: 13 slabs of 7 picture rows per channel
group, the last one 6 rows, one slab across both frames -- and, for the pixel GEMM alone, decoder_ref64.GEMM_SPLIT_SHAPE
(12,45,80): 22 shares of 2 chunks, the last one a single chunk of 192 pixels."""
import math
import os
from functools import lru_cache

import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import losses, ops, synth, train

import decoder_ref64 as DR
import train_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPE_IDS = [DR.name(s) for s in DR.SHAPES]


def _cl(a):
    return torch.as_tensor(a).to(DEV).float().contiguous(memory_format=torch.channels_last)


def _dense_nhwc(t64, keep_masks=False):
    """a float64 NCHW tensor as the dense fp32 NHWC tensor the kernels read"""
    t32 = DR.teacher_round(t64) if keep_masks else t64.float()
    return t32.permute(0, 2, 3, 1).contiguous()


def _check(got, want, bound, what):
    err = (got.double() - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print("%s: worst error / bound %.4f (max |err| %.3e, max |ref| %.3e)" % (what, worst, float(err.max()), float(want.abs().max())))
    assert torch.isfinite(got).all() and bool((err <= bound).all()), what
    return worst


def _block(q):
    from iip_uavsal_saliency_amd.model import dwBlock
    return DR.load_block(dwBlock(256, 1, kernel_size=3), q).to(DEV)


@lru_cache(maxsize=None)
def _case(shape, zero_gamma=False):
    """the block, its float64 numbers, inputs, the closed form with bounds, and the teacher-forced fp32 tensors; once per shape"""
    hn, qn, gyn = DR.decoder_case(shape, zero_gamma)
    h, q, gy = torch.as_tensor(hn).to(DEV).double(), DR.to64(qn, DEV), torch.as_tensor(gyn).to(DEV).double()
    parts = {}
    want, bound = DR.param_grads(q, h, gy, bounds=True, parts=parts)
    t = {"h": _cl(hn), "gy": gy.float(), "e": _dense_nhwc(parts["e"], True), "d": _dense_nhwc(parts["d"], True),
         "y": parts["y"].float().contiguous(), "ga": _dense_nhwc(parts["ga"])}
    keep = {k: parts[k] for k in ("e", "d", "grad_h")}
    return _block(qn), q, h, gy, want, bound, t, keep


def _teacher_grads(shape, zero_gamma=False, **kw):
    block, _, _, _, _, _, t, _ = _case(shape, zero_gamma)
    return train.decoder_param_grads(block, t["h"], t["e"], t["d"], t["y"], t["gy"], ga=t["ga"], **kw)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. the pixel GEMM
@lru_cache(maxsize=None)
def _gemm_ops(shape):
    if shape == DR.GEMM_SPLIT_SHAPE:
        a, b = (torch.as_tensor(v).to(DEV) for v in DR.gemm_inputs(shape))
    else:
        t = _case(shape)[6]
        a, b = t["ga"], t["h"].permute(0, 2, 3, 1)
    return (a, b) + DR.pix_gemm_ref(a.double(), b.double())


@pytest.mark.parametrize("shape", DR.SHAPES + [DR.GEMM_SPLIT_SHAPE], ids=SHAPE_IDS + [DR.name(DR.GEMM_SPLIT_SHAPE)])
def test_pix_gemm_against_float64(shape):
    a, b, want, bound = _gemm_ops(shape)
    M, N = a.shape[3], b.shape[3]
    got = train.pix_gemm(a, b)
    _check(got, want, bound, "%s pix_gemm" % DR.name(shape))
    assert torch.equal(_bits(got), _bits(train.pix_gemm(a, b)))                   # two calls, the same bits
    # row_scale, rowdot and accumulate: out = fl(old + rs G), rowdot = sum_n w G in double
    rs = torch.linspace(-2.0, 2.0, M, device=DEV)
    w = torch.randn(M, N, device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    old = torch.randn(M, N, device=DEV, generator=torch.Generator(DEV).manual_seed(6)) * float(want.abs().max())
    out, rowdot = old.clone(), torch.empty(M, dtype=torch.float64, device=DEV)
    train.pix_gemm(a, b, out=out, row_scale=rs, w=w, rowdot=rowdot, accumulate=True)
    exp = old.double() + rs.double().view(-1, 1) * want
    _check(out, exp, rs.double().abs().view(-1, 1) * bound + R.EPS * (old.double().abs() + exp.abs()), "  + row_scale, accumulate")
    _check(rowdot, (w.double() * want).sum(1), (w.double().abs() * bound).sum(1), "  rowdot")
    r2 = torch.empty_like(rowdot)
    train.pix_gemm(a, b, w=w, rowdot=r2)
    assert torch.equal(rowdot.view(torch.int64), r2.view(torch.int64))
    if shape == DR.GEMM_SPLIT_SHAPE:
        # the split is real here: a kernel that drops the last share is rejected by the bound the right one passes
        cps, shares, spans = DR.gemm_partition(a.shape[0] * a.shape[1] * a.shape[2])
        assert (cps, shares, spans[-1][1] - spans[-1][0]) == (2, 22, 192)
        p0 = spans[-1][0]
        A, B = a.reshape(-1, M).double(), b.reshape(-1, N).double()
        wrong = A[:p0].T @ B[:p0]
        assert float(((wrong - want).abs() / bound).max()) >= 4.0
        assert not bool(((got.double() - wrong).abs() <= bound).all())


def test_pix_gemm_reads_channel_slices_in_place():
    a, b, _, _ = _gemm_ops((3, 5, 7))
    T, H, W, M = a.shape
    wide_a = torch.zeros((T, H, W, M + 256), device=DEV)
    wide_a[..., 128:128 + M] = a
    wide_b = torch.zeros((T, H, W, 512), device=DEV)
    wide_b[..., 256:] = b
    assert torch.equal(_bits(train.pix_gemm(a, b)), _bits(train.pix_gemm(wide_a[..., 128:128 + M], wide_b[..., 256:])))
    with pytest.raises(RuntimeError, match="same pixels"):
        train.pix_gemm(a, b[:2])
    with pytest.raises(RuntimeError, match="ESHAPE|shape|rejected"):
        train.pix_gemm(a[..., :100 * 4], b)


# ------------------------------------------------------------------------------------------------ 2. sums + finalise
@pytest.mark.parametrize("shape", DR.SHAPES, ids=SHAPE_IDS)
def test_param_grads_teacher_forced_against_float64(shape):
    """Per tensor against the float64 closed form.  (2,45,80) is SLAB_SHAPE: 13 slabs, a partial last one."""
    want, bound = _case(shape)[4:6]
    got = _teacher_grads(shape)
    assert tuple(got) == DR.NAMES
    for n in DR.NAMES:
        assert got[n].shape == want[n].shape and got[n].dtype == torch.float32
        _check(got[n], want[n], bound[n], "%s %s" % (DR.name(shape), n))
    again = _teacher_grads(shape)
    assert all(torch.equal(_bits(got[n]), _bits(again[n])) for n in DR.NAMES)      # two calls, the same bits
    # out= / accumulate=: added to what is there, rounded once
    old = {n: torch.full_like(got[n], 0.25) * float(want[n].abs().max()) for n in DR.NAMES}
    acc = {n: v.clone() for n, v in old.items()}
    assert _teacher_grads(shape, out=acc, accumulate=True) is acc
    for n in DR.NAMES:
        exp = old[n].double() + want[n]
        _check(acc[n], exp, bound[n] + R.EPS * (old[n].double().abs() + exp.abs()), "  accumulate %s" % n)
    if shape == DR.SLAB_SHAPE:
        assert DR.slab_partition(*shape) == (7, 13)


def test_param_grads_default_ga_is_dec_bwd_with_ones():
    """Without `ga` the function forms it by uavsal_dec_bwd handed ones for s1.  That ga is within dec_bwd's own bound
    (train_ref64.dec_bwd_bound, s1 = 1) of the float64 one; the three gradients that read ga take that bound through their
    sums on top of their own: sum gb |h| for G1, sum gb for S1."""
    shape = (5, 12, 20)
    block, q, h, gy, want, bound, t, keep = _case(shape)
    got = train.decoder_param_grads(block, t["h"], t["e"], t["d"], t["y"], t["gy"])
    p = DR.fold(q)
    ones = dict(p, s1=torch.ones_like(p["s1"]))
    y64 = R.decoder_forward(p, h)["y"]
    gb = R.dec_bwd_bound(ones, gy, y64, keep["e"], keep["d"])
    eG1, eS1 = torch.einsum("tchw,tjhw->cj", gb, h.abs()), gb.sum((0, 2, 3))
    w1 = q["w1"].reshape(DR.HID, DR.C).abs()
    extra = {DR.NAMES[0]: (p["s1"].abs().view(-1, 1) * eG1).view(DR.HID, DR.C, 1, 1),
             DR.NAMES[1]: p["r1"] * ((w1 * eG1).sum(1) + p["mu1"].abs() * eS1), DR.NAMES[2]: eS1}
    for n in DR.NAMES[:3]:                                                   # the three that read ga
        _check(got[n], want[n], bound[n] + extra[n], "%s %s (ga from the device)" % (DR.name(shape), n))
    for n in DR.NAMES[3:]:
        assert torch.equal(_bits(got[n]), _bits(_teacher_grads(shape)[n]))


def test_zero_gamma_channels_have_a_gamma_gradient():
    shape = (3, 5, 7)
    want, bound = _case(shape, True)[4:6]
    got = _teacher_grads(shape, True)
    for n in DR.NAMES:
        _check(got[n], want[n], bound[n], "zero gamma %s" % n)
    c1, c2 = DR.ZERO_GAMMA
    assert float(got[DR.NAMES[0]][c1].abs().max()) == 0 and float(got[DR.NAMES[3]][c2].abs().max()) == 0
    for n, c in ((DR.NAMES[1], c1), (DR.NAMES[4], c2)):
        assert float(got[n][c].abs()) > 0 and float((got[n][c].double() - want[n][c]).abs()) <= float(bound[n][c])


def test_zero_grad_out_gives_positive_zeros():
    shape = (3, 5, 7)
    block, _, _, _, _, _, t, _ = _case(shape)
    z = torch.zeros_like(t["gy"])
    got = train.decoder_param_grads(block, t["h"], t["e"], t["d"], t["y"], z, ga=torch.zeros_like(t["ga"]))
    for n in DR.NAMES:
        assert int(_bits(got[n]).abs().max()) == 0, n                               # +0.0: no sign bit either


@pytest.mark.parametrize("shape", DR.GOLDEN_SHAPES, ids=DR.name)
def test_param_grads_against_the_reference(shape, golden_dir):
    g = np.load(os.path.join(golden_dir, DR.name(shape) + ".npz"))
    hn, qn, gyn = DR.decoder_case(shape)
    assert str(g["digest"]) == R.digest(hn, gyn, *[qn[k] for k in sorted(qn)])
    bound = _case(shape)[5]
    got = _teacher_grads(shape)
    for n in DR.NAMES[1:]:
        _check(got[n].cpu(), torch.as_tensor(g[n.replace(".", "_")]), bound[n].cpu(), "%s %s vs the reference" % (DR.name(shape), n))
    w1 = got[DR.NAMES[0]][:, :, 0, 0]
    _check(w1[DR.W1_SUBSET].cpu(), torch.as_tensor(g["W1"]), bound[DR.NAMES[0]][:, :, 0, 0][DR.W1_SUBSET].cpu(), "%s W1 vs the reference" % DR.name(shape))
    tot = float(bound[DR.NAMES[0]].sum())
    assert abs(float(w1.double().sum()) - float(g["W1_sum"])) <= tot
    assert abs(float(w1.double().norm()) - float(g["W1_l2"])) <= tot


# ------------------------------------------------------------------------------------------------ 3. decoder_backward
@pytest.mark.parametrize("shape", DR.SHAPES, ids=SHAPE_IDS)
def test_decoder_backward_end_to_end(shape):
    """The device recomputes e and d.  The parameter gradients equal decoder_param_grads fed the call's own parts, bit for
    bit; grad_h is within the limit of the frozen path's end-to-end test (train_ref64.decoder_e2e: per frame in L2, the
    regular bound plus the term of the masks the device may decide the other way)."""
    block, q, h, gy, _, _, t, keep = _case(shape)
    p = DR.fold(q)
    f = R.decoder_forward(p, h)
    want, bound, und, _ = R.decoder_e2e(p, h, gy)
    assert float((want - keep["grad_h"]).abs().max()) <= 1e-12 * float(want.abs().max())
    parts = {}
    gh, grads = train.decoder_backward(block, t["h"], t["gy"], y=f["y"].float(), parts=parts)
    assert sorted(parts) == ["d", "e", "ga", "y"] and tuple(grads) == DR.NAMES
    again = train.decoder_param_grads(block, t["h"], parts["e"], parts["d"], parts["y"], t["gy"], ga=parts["ga"])
    for n in DR.NAMES:
        assert torch.equal(_bits(grads[n]), _bits(again[n])), n
    err, lim, ref = R.l2_per_frame(gh.double() - want), R.l2_per_frame(bound + und), R.l2_per_frame(want)
    print("%s: per frame ||err|| / ||grad_h|| %s, limit %s" % (DR.name(shape), ["%.2e" % v for v in (err / ref).tolist()],
                                                              ["%.2e" % v for v in (lim / ref).tolist()]))
    assert bool((err <= lim).all())
    frozen = train.decoder_input_grad(block, t["h"], t["gy"], y=f["y"].float())
    assert bool((R.l2_per_frame(gh.double() - frozen.double()) <= lim).all())      # the two paths may differ in the last bits
    # given gradient tensors are written in place, or added to
    mine = {n: torch.zeros_like(v) for n, v in grads.items()}
    _, same = train.decoder_backward(block, t["h"], t["gy"], y=f["y"].float(), grads=mine)
    assert same is mine and all(torch.equal(_bits(mine[n]), _bits(grads[n])) for n in DR.NAMES)
    with pytest.raises(RuntimeError, match="eval"):
        train.decoder_backward(block.train(), t["h"], t["gy"])
    block.eval()


# ------------------------------------------------------------------------------------------------ 4. the step and the driver
H_, W_, T_ = 72, 104, 4
RNN = "rnn.cell_list.0.rnn_conv.weight"


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


def _stats(m):
    return [b.detach().clone() for b in m.conv_out_st.buffers()]


def test_recurrence_step_with_the_decoder():
    m = _model()
    x, cb, y = _step_inputs()
    dec = ["conv_out_st." + n for n in DR.NAMES]
    stats = _stats(m)
    frozen = _model()
    train.recurrence_step(frozen, x, cb, None, y)
    g_frozen = frozen.rnn.cell_list[0].rnn_conv.weight.grad
    loss, out, st = train.recurrence_step(m, x, cb, None, y, decoder=True)
    ref_out, ref_st = m(x, cb, None)
    assert torch.equal(out, ref_out) and torch.equal(st[0], ref_st[0]) and loss.item() == losses.loss_fu(ref_out, y).item()
    assert sorted(k for k, p in m.named_parameters() if p.grad is not None) == sorted([RNN] + dec)      # exactly ten
    params = dict(m.named_parameters())
    g1 = {k: params[k].grad.clone() for k in [RNN] + dec}
    assert all(torch.isfinite(v).all() and float(v.abs().max()) > 0 and v.is_contiguous() for v in g1.values())
    # the recurrence gets decoder_backward's grad_h: s1 enters through the packed W1^T instead of inside uavsal_dec_bwd, a
    # reordering of two fp32 roundings per term of a 1536-term sum, carried through the recurrence's linear backward:
    # a relative L2 distance of rounding level: 2 U LAMBDA sqrt(1536) = 3.7e-5 in the convention of plan_ref64 (e and d
    # come from the same launches in both paths, so no mask differs)
    rel = float((g1[RNN].double() - g_frozen.double()).norm() / g_frozen.double().norm())
    print("recurrence gradient, decoder=True against decoder=False: relative L2 distance %.3e" % rel)
    assert rel <= 2 * R.U * R.LAMBDA * math.sqrt(1536)
    train.recurrence_step(m, x, cb, None, y, decoder=True)                       # .grad += as loss.backward() would
    for k in dec:
        _check(params[k].grad, 2 * g1[k].double(), 4 * R.U * g1[k].double().abs(), "second call doubles %s" % k)
    assert all(torch.equal(a, b) for a, b in zip(stats, _stats(m)))
    # the directional derivative along the normalised nine-tensor decoder gradient against the central difference (the
    # plumbing check of tests/test_train_gpu.py, with its 10 % and for its reason); weights edited in place and refreshed
    with torch.no_grad():
        norm = float(torch.sqrt(sum((g1[k].double() ** 2).sum() for k in dec)))
        w0 = {k: params[k].detach().clone() for k in dec}
        s = 2e-2 / norm
        vals = []
        for sign in (1.0, -1.0):
            for k in dec:
                params[k].copy_(w0[k] + sign * s * g1[k] / norm)
            assert m.refresh_weights(m.conv_out_st) > 0
            vals.append(losses.loss_fu(m(x, cb, None)[0], y).item())
        for k in dec:
            params[k].copy_(w0[k])
        m.refresh_weights(m.conv_out_st)
    fd = (vals[0] - vals[1]) / (2 * s)
    print("decoder directional derivative: finite difference %.6e, <grad, D> %.6e, step %.3e" % (fd, norm, s))
    assert abs(fd - norm) <= 0.10 * abs(norm)
    assert torch.equal(m(x, cb, None)[0], ref_out)                                # the restored weights give the same bits


def test_adam_steps_over_both_stages_keep_the_plans():
    from iip_uavsal_saliency_amd import UAVSal
    m = _model()
    x, cb, y = _step_inputs()
    stats = _stats(m)
    opt = torch.optim.Adam(list(m.rnn.parameters()) + list(m.conv_out_st.parameters()), lr=1e-4, betas=(0.9, 0.999),
                           weight_decay=5e-5)
    before = m(x, cb, None)[0]
    first = None
    for _ in range(5):
        opt.zero_grad()
        loss, _, _ = train.recurrence_step(m, x, cb, None, y, decoder=True)
        first = loss.item() if first is None else first
        engines = dict(m._engines)
        opt.step()
        assert m.refresh_weights(m.rnn, m.conv_out_st) > 0
        after = m(x, cb, None)[0]
        assert {k: id(e) for k, e in m._engines.items()} == {k: id(e) for k, e in engines.items()}      # the same engine objects
    last = losses.loss_fu(after, y).item()
    print("loss_fu on the group: %.6f before, %.6f after five Adam steps over both stages" % (first, last))
    assert last < first and not torch.equal(before, after)
    assert all(torch.equal(a, b) for a, b in zip(stats, _stats(m)))                # running statistics unchanged
    fresh = UAVSal(time_dims=T_)
    fresh.load_state_dict(m.state_dict())
    fresh = fresh.to(DEV).eval()
    taps, ftaps = {}, {}
    got, got_st = m(x, cb, None, taps=taps)
    want, want_st = fresh(x, cb, None, taps=ftaps)
    assert torch.equal(got, want) and torch.equal(got_st[0], want_st[0])           # bit for bit the repacked weights
    assert sorted(taps) == sorted(ftaps) and all(torch.equal(taps[k], ftaps[k]) for k in taps)
    got2, _ = m(x, cb, None)
    assert torch.equal(got2, want)


def test_refresh_with_the_decoder_drops_the_plans_when_another_parameter_moved():
    m = _model()
    x, cb, _ = _step_inputs()
    m(x, cb, None)
    with torch.no_grad():
        m.conv_out_st.conv[2].weight.mul_(1.5)
        m.fust_layer[0].conv[0][0].weight.mul_(1.01)
    assert m.refresh_weights(m.rnn, m.conv_out_st) == 0 and len(m._engines) == 0 and m._wversion is None


def test_finetune_video_with_the_decoder_is_the_manual_loop():
    from iip_uavsal_saliency_amd.stream import finetune_video
    n = 2 * T_ * 2
    frames = torch.from_numpy(synth.synth_frames_u8(n, H_, W_, 2)).to(DEV)
    gp = torch.from_numpy(synth.gauss_priors(1, H_ // 8, W_ // 8)[0]).to(DEV)
    op_ = torch.from_numpy(synth.ob_priors(1, H_ // 8, W_ // 8)[0]).to(DEV)
    loc = synth.synth_fix_points(n, 90, 130, 12, 9)
    fmap = np.rint(synth.synth_fix_maps(loc, 6.0) * 255).astype(np.uint8)
    fix_map, fix_loc = torch.from_numpy(fmap).to(DEV), torch.from_numpy(loc).to(DEV)

    def make():
        m = _model()
        ps = list(m.rnn.parameters()) + list(m.conv_out_st.parameters())
        return m, torch.optim.Adam(ps, lr=1e-4, betas=(0.9, 0.999), weight_decay=5e-5)
    m, opt = make()
    seen = []
    real = train.recurrence_step

    def spy(model, x, cb, state, y, criterion, **kw):
        assert kw == {"decoder": True}
        seen.append((x.clone(), [c.clone() for c in cb], y.clone()))
        return real(model, x, cb, state, y, criterion, **kw)
    train.recurrence_step = spy
    try:
        res = finetune_video(m, frames, gp, op_, fix_map, fix_loc, opt, batch_size=2, stages=("rnn", "decoder"))
    finally:
        train.recurrence_step = real
    assert res["groups_run"] == 2 and len(seen) == 2
    m2, opt2 = make()
    state, manual = None, []
    for x, cb, y in seen:
        opt2.zero_grad()
        loss, _, state = train.recurrence_step(m2, x, cb, state, y, decoder=True)
        opt2.step()
        m2.refresh_weights(m2.rnn, m2.conv_out_st)
        manual.append(loss.item())
    assert [float(v) for v in res["losses"].tolist()] == manual
    for (k, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    assert sorted(k for k, p in m.named_parameters() if p.grad is not None) == sorted([RNN] + ["conv_out_st." + n for n in DR.NAMES])
    w0 = _model().conv_out_st.conv[0][0].weight
    assert not torch.equal(m.conv_out_st.conv[0][0].weight.detach(), w0.detach())
