"""Criterion, gaze ground truth and validation driver on the GPU, against the float64 restatement (tests/loss_ref64.py) and
the reference's recorded outputs (tests/golden/loss_*.npz).

Tolerances.  The device accumulates in double and rounds once, so against the float64 restatement a value may be off by
the final rounding: one fp32 ulp of the value; a gradient element by one fp32 ulp of the frame's largest gradient
magnitude.  Against the reference's fp32 results the generator recorded, per case, the gap between the reference's fp32
and float64 runs -- the reference's own summation error --: twice that gap (another torch build sums in another order)
plus the ulp above.  Integer results (the ground truth) and repeated runs are compared for equality.

Batches: loss_ref64.RANDOM_CASES (B = 20 and 8, with goldens) keep the mean over the frames -- one wave, lane i takes frames
i, i + 64, ... -- inside its first stride.  loss_ref64.STRIDE_CASES go beyond it, against the restatement with the same
tolerances: 12x20_B65 (vector path, one frame in the second stride) and 9x15_B130 (scalar path, three strides, the last two
lanes wide); at B = 65 the mean over the first 64 frames only -- the loop without its second stride -- must be rejected."""
import os

import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import losses, ops, synth

import loss_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VALUES = ("metric_kl", "metric_cc", "metric_nss", "loss_fu", "loss_kl")


def _golden(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def _ulp(x):
    """one fp32 ulp at |x| (float64 in, float64 out)"""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def _frame_max(g):
    return np.abs(g).reshape(len(g), -1).max(1).reshape(-1, 1, 1, 1)


def _device_values(y_pred, y_true):
    p, t = torch.from_numpy(y_pred).to(DEV), torch.from_numpy(y_true).to(DEV)
    out, _ = losses.loss_components(p, t)
    out = out.cpu().numpy()
    got = dict(zip(VALUES[:4], out.tolist()))
    assert losses.metric_kl(p, t).shape == (1,) and losses.loss_fu(p, t).shape == ()
    assert losses.metric_kl(p, t).item() == got["metric_kl"] and losses.metric_cc(p, t).item() == got["metric_cc"]
    assert losses.metric_nss(p, t).item() == got["metric_nss"] and losses.loss_fu(p, t).item() == got["loss_fu"]
    got["loss_kl"] = losses.loss_kl(p, t).item()
    return got


def _device_grad(y_pred, y_true, fn):
    p = torch.from_numpy(y_pred).to(DEV).requires_grad_(True)
    fn(p, torch.from_numpy(y_true).to(DEV)).backward()
    return p.grad.cpu().numpy()


# ------------------------------------------------------------------------------------------------ ground truth

def _layouts(a):
    """a uint8 [F,H0,W0] array as device tensors in every layout prepare_gaze reads, with the `layout` argument"""
    t = torch.from_numpy(a).to(DEV)
    F, h0, w0 = a.shape
    big = torch.full((F + 2, h0 + 3, w0 + 5), 9, dtype=torch.uint8, device=DEV)
    big[1:F + 1, 2:h0 + 2, 1:w0 + 1] = t
    odd = torch.full((F * h0 * w0 + 3,), 9, dtype=torch.uint8, device=DEV)
    odd[3:] = t.reshape(-1)
    return [("FHW", t, None),
            ("HW1F", t.permute(1, 2, 0)[:, :, None, :].contiguous(), None),
            ("HWF", t.permute(1, 2, 0).contiguous(), "HWF"),
            ("matlab order", t.permute(0, 2, 1).contiguous().permute(2, 1, 0)[:, :, None, :], None),     # [H0,W0,1,F], rows fastest
            ("slice of a larger buffer", big[1:F + 1, 2:h0 + 2, 1:w0 + 1], None),
            ("odd byte offset", odd[3:].view(F, h0, w0), None)]


@pytest.mark.parametrize("h0,w0,h,w", R.SCATTER_CASES)
def test_prepare_gaze_is_bit_identical(golden_dir, h0, w0, h, w):
    g = _golden(golden_dir, "loss_scatter.npz")
    fmap, loc = R.scatter_inputs(h0, w0)
    want, want_has = R.prepare_gaze(fmap, loc, h, w)
    assert np.array_equal(want[:, 1], g["fix_%dx%d_to_%dx%d" % (h0, w0, h, w)].astype(np.float32))     # the reference's scatter
    first = None
    for (name, m, layout), (_, l, _) in zip(_layouts(fmap), _layouts(loc)):
        y, has = ops.prepare_gaze(m, l, h, w, layout)
        assert y.dtype == torch.float32 and tuple(y.shape) == (4, 2, h, w) and has.dtype == torch.bool, name
        y, has = y.cpu().numpy(), has.cpu().numpy()
        assert np.array_equal(y[:, 0], want[:, 0]), name
        assert np.array_equal(y[:, 1], want[:, 1]), name
        assert np.array_equal(has, want_has), name
        if first is None:
            first = y
            again, has2 = ops.prepare_gaze(m, l, h, w, layout)
            assert np.array_equal(again.cpu().numpy().view(np.uint32), y.view(np.uint32)) and np.array_equal(has2.cpu().numpy(), has)


def test_prepare_gaze_full_size_sources():
    """720x1280 sources to the model's 45x80, many frames; a frame subset of a longer video"""
    loc = synth.synth_fix_points(12, 720, 1280, 40, 4)
    loc[5] = 0
    fmap = np.rint(synth.synth_fix_maps(loc[:3], 20.0) * 255).astype(np.uint8)
    fmap = np.concatenate([fmap] * 4)
    fmap[7] = 0
    want, want_has = R.prepare_gaze(fmap, loc, 45, 80)
    y, has = ops.prepare_gaze(torch.from_numpy(fmap).to(DEV), torch.from_numpy(loc).to(DEV), 45, 80)
    assert np.array_equal(y.cpu().numpy(), want) and np.array_equal(has.cpu().numpy(), want_has)
    assert want_has.tolist()[5] == [True, False] and want_has.tolist()[7] == [False, True]
    y2, has2 = ops.prepare_gaze(torch.from_numpy(fmap).to(DEV)[3:9], torch.from_numpy(loc).to(DEV)[3:9], 45, 80)
    assert torch.equal(y2, y[3:9]) and torch.equal(has2, has[3:9])


# ------------------------------------------------------------------------------------------------ criterion

@pytest.mark.parametrize("name,h,w,B,seed", R.RANDOM_CASES + R.STRIDE_CASES)
def test_forward_and_gradient_against_the_restatement(name, h, w, B, seed):
    y_pred, y_true = R.random_inputs(h, w, B, seed)
    got = _device_values(y_pred, y_true)
    want = dict(zip(VALUES[:4], R.loss(y_pred, y_true)))
    want["loss_kl"] = R.loss(y_pred, y_true, R.LOSS_KL)[3]
    for k in VALUES:
        err, tol = abs(got[k] - want[k]), float(_ulp(want[k]))
        print("%s %s: device %.9g restatement %.17g |diff| %.3e (one ulp %.3e)" % (name, k, got[k], want[k], err, tol))
        assert err <= tol, k
    for fn, weights in ((losses.loss_fu, R.LOSS_FU), (losses.loss_kl, R.LOSS_KL)):
        grad = _device_grad(y_pred, y_true, fn).astype(np.float64)
        ref = R.loss_grad(y_pred, y_true, weights)
        err, tol = np.abs(grad - ref), _ulp(_frame_max(ref))
        print("%s gradient of %s: worst |diff| / ulp(frame max) %.3f" % (name, fn.__name__, (err / tol).max()))
        assert (err <= tol).all()


@pytest.mark.parametrize("name,h,w,B,seed", R.RANDOM_CASES)
def test_against_the_reference_fp32_goldens(golden_dir, name, h, w, B, seed):
    g = _golden(golden_dir, "loss_%s_f32.npz" % name)
    y_pred, y_true = R.random_inputs(h, w, B, seed)
    assert str(g["digest"]) == R.digest(y_pred, y_true)
    got = _device_values(y_pred, y_true)
    for k in VALUES:
        err, tol = abs(got[k] - float(g[k])), 2.0 * float(g["gap_" + k]) + float(_ulp(float(g[k])))
        print("%s %s: device %.9g reference fp32 %.9g |diff| %.3e (allowed %.3e, recorded gap %.3e)" % (
            name, k, got[k], float(g[k]), err, tol, float(g["gap_" + k])))
        assert err <= tol, k
    grad = _device_grad(y_pred, y_true, losses.loss_fu).astype(np.float64)
    ref = g["grad_loss_fu"].astype(np.float64)
    fmax = _frame_max(ref)
    tol = 2.0 * g["gap_grad_loss_fu"].reshape(-1, 1, 1, 1) * fmax + _ulp(fmax)      # the gap is relative to the frame's maximum
    err = np.abs(grad - ref)
    print("%s gradient: worst |diff| / allowed %.3f (recorded gaps up to %.2e)" % (name, (err / tol).max(), g["gap_grad_loss_fu"].max()))
    assert (err <= tol).all()


def test_two_runs_are_bit_identical_and_autograd_is_the_direct_call():
    y_pred, y_true = R.random_inputs(45, 80, 20, 11)
    p, t = torch.from_numpy(y_pred).to(DEV), torch.from_numpy(y_true).to(DEV)
    out1, stats1 = losses.loss_components(p, t)
    out2, stats2 = losses.loss_components(p, t)
    assert torch.equal(out1.view(torch.int32), out2.view(torch.int32)) and torch.equal(stats1.view(torch.int64), stats2.view(torch.int64))
    one = torch.ones((), device=DEV)
    g1, g2 = losses.loss_grad(p, t, stats1, one), losses.loss_grad(p, t, stats2, one)
    assert torch.equal(g1.view(torch.int32), g2.view(torch.int32))
    q = p.clone().requires_grad_(True)
    loss = losses.loss_fu(q, t)
    assert loss.item() == out1[3].item()
    loss.backward()
    assert torch.equal(q.grad.view(torch.int32), g1.view(torch.int32))
    # an incoming gradient other than 1, and the clip form [B,D,1,H,W]
    q2 = p.clone().requires_grad_(True)
    (losses.loss_fu(q2, t) * 0.5).backward()
    assert torch.equal(q2.grad, losses.loss_grad(p, t, stats1, 0.5))
    q5 = p.clone().reshape(4, 5, 1, 45, 80).requires_grad_(True)
    l5 = losses.loss_fu_dy(q5, t.reshape(4, 5, 2, 45, 80))
    l5.backward()
    assert l5.item() == out1[3].item() and torch.equal(q5.grad.reshape(20, 1, 45, 80), g1)
    # a non-contiguous prediction (a channel of a wider tensor) and no gradient asked for
    wide = torch.zeros(20, 3, 45, 80, device=DEV)
    wide[:, 1:2] = p
    with torch.no_grad():
        assert losses.loss_fu(wide[:, 1:2], t).item() == out1[3].item()
    # sizes that are not a multiple of four take the scalar path
    yp, yt = R.random_inputs(9, 15, 3, 5)
    got = losses.loss_components(torch.from_numpy(yp).to(DEV), torch.from_numpy(yt).to(DEV))[0].cpu().numpy()
    for a, b in zip(got.tolist(), R.loss(yp, yt)):
        assert abs(a - b) <= float(_ulp(b))
    gr = _device_grad(yp, yt, losses.loss_fu).astype(np.float64)
    ref = R.loss_grad(yp, yt)
    assert (np.abs(gr - ref) <= _ulp(_frame_max(ref))).all()


def test_mean_beyond_one_stride_of_the_wave():
    """B = 65: two runs give equal bits, and the mean the loop would give without its second stride (the first 64 frames
    only) is more than the value's one ulp away from every device value -- tests/test_losses_cpu.py holds that wrong
    reference at least 4 ulps from the right one."""
    name, h, w, B, seed = R.STRIDE_CASES[0]
    assert B == R.MEAN_LANES + 1
    y_pred, y_true = R.random_inputs(h, w, B, seed)
    p, t = torch.from_numpy(y_pred).to(DEV), torch.from_numpy(y_true).to(DEV)
    out1, stats1 = losses.loss_components(p, t)
    out2, stats2 = losses.loss_components(p, t)
    assert torch.equal(out1.view(torch.int32), out2.view(torch.int32)) and torch.equal(stats1.view(torch.int64), stats2.view(torch.int64))
    one = torch.ones((), device=DEV)
    assert torch.equal(losses.loss_grad(p, t, stats1, one).view(torch.int32), losses.loss_grad(p, t, stats2, one).view(torch.int32))
    got = _device_values(y_pred, y_true)
    assert [got[k] for k in VALUES[:4]] == out1.cpu().tolist()
    n = R.MEAN_LANES
    wrong = dict(zip(VALUES[:4], R.loss(y_pred[:n], y_true[:n])))
    wrong["loss_kl"] = R.loss(y_pred[:n], y_true[:n], R.LOSS_KL)[3]
    for k in VALUES:
        ratio = abs(got[k] - wrong[k]) / float(_ulp(wrong[k]))
        print("%s %s: device %.9g, mean of the first %d frames %.17g: %.0f ulps apart" % (name, k, got[k], n, wrong[k], ratio))
        assert ratio > 1.0, k


def test_degenerate_frames(golden_dir):
    g = _golden(golden_dir, "loss_edge_45x80.npz")
    y_pred, y_true = R.edge_inputs()
    assert str(g["digest"]) == R.digest(y_pred, y_true)
    got = _device_values(y_pred, y_true)
    want = dict(zip(VALUES[:4], R.loss(y_pred, y_true)))
    want["loss_kl"] = R.loss(y_pred, y_true, R.LOSS_KL)[3]
    for k in VALUES:
        assert abs(got[k] - want[k]) <= float(_ulp(want[k])), k
        tol = 2.0 * float(g["gap_" + k]) + float(_ulp(float(g["f32_" + k])))
        print("edge %s: device %.9g reference fp32 %.9g (allowed %.3e)" % (k, got[k], float(g["f32_" + k]), tol))
        assert abs(got[k] - float(g["f32_" + k])) <= tol, k
    # per frame: a constant prediction adds exactly 0 to cc and nss, the empty frame 0 to everything
    stats = losses.loss_components(torch.from_numpy(y_pred).to(DEV), torch.from_numpy(y_true).to(DEV))[1].cpu().numpy()
    for f in R.EDGE_CONSTANT:
        assert stats[f, 1] == 0.0 and stats[f, 2] == 0.0
    assert (stats[R.EDGE_ZERO_MAP, :3] == 0.0).all()
    # the gradient: NaN over the whole frame where the prediction is constant, finite everywhere else
    grad = _device_grad(y_pred, y_true, losses.loss_fu)
    for f in range(len(grad)):
        if f in R.EDGE_CONSTANT:
            assert np.isnan(grad[f]).all(), f
        else:
            assert np.isfinite(grad[f]).all(), f
    ref = R.loss_grad(y_pred, y_true)
    ok = [f for f in range(len(grad)) if f not in R.EDGE_CONSTANT]
    assert (np.abs(grad[ok].astype(np.float64) - ref[ok]) <= _ulp(_frame_max(ref[ok]))).all()
    # the frames on which the reference is finite too, against its fp32 gradient
    both = [f for f in ok if f != R.EDGE_ZERO_MAP]
    r32 = g["f32_grad_loss_fu"][both].astype(np.float64)
    fmax = _frame_max(r32)
    assert (np.abs(grad[both] - r32) <= 2.0 * g["gap_grad_loss_fu"][both].reshape(-1, 1, 1, 1) * fmax + _ulp(fmax)).all()
    # loss_kl has no std in it: finite on every frame, as in the reference
    gkl = _device_grad(y_pred, y_true, losses.loss_kl).astype(np.float64)
    rkl = R.loss_grad(y_pred, y_true, R.LOSS_KL)
    assert np.isfinite(gkl).all() and (np.abs(gkl - rkl) <= _ulp(np.maximum(_frame_max(rkl), 1e-30))).all()


# ------------------------------------------------------------------------------------------------ validation driver

@pytest.mark.parametrize("source_size", [None, (144, 200)], ids=["model-size frames", "source-size frames"])
def test_validate_video_is_the_manual_loop(source_size):
    """40 frames at 96x160, time_dims 5, batch_size 2: four groups of 10; a frame of the third group has no fixation, so that
    group is skipped before its forward and the fourth continues from the state the second left."""
    from iip_uavsal_saliency_amd import UAVSal
    from iip_uavsal_saliency_amd.stream import validate_video
    R_, C_ = 96, 160
    m = UAVSal(time_dims=5)
    synth.load_synth_weights(m, 0)
    m = m.to(DEV).eval()
    gp = torch.from_numpy(synth.gauss_priors(1, R_ // 8, C_ // 8)[0]).to(DEV)
    op_ = torch.from_numpy(synth.ob_priors(1, R_ // 8, C_ // 8)[0]).to(DEV)
    fh, fw = source_size or (R_, C_)
    frames = torch.from_numpy(synth.synth_frames_u8(43, fh, fw, 2)).to(DEV)
    loc = synth.synth_fix_points(41, 180, 320, 15, 9)
    fmap = np.rint(synth.synth_fix_maps(loc, 8.0) * 255).astype(np.uint8)
    loc[24] = 0
    fix_map = torch.from_numpy(fmap.transpose(1, 2, 0)[:, :, None, :].copy()).to(DEV)     # the .mat layout
    fix_loc = torch.from_numpy(loc.transpose(1, 2, 0)[:, :, None, :].copy()).to(DEV)
    kw = {} if source_size is None else {"model_size": (R_, C_)}
    res = validate_video(m, frames, gp, op_, fix_map, fix_loc, batch_size=2, **kw)

    y_gaze, has = ops.prepare_gaze(fix_map, fix_loc, R_ // 8, C_ // 8)
    assert tuple(y_gaze.shape) == (41, 2, 12, 20)
    state, want, steps = None, [], 0
    with torch.no_grad():
        for a in range(0, 40, 10):
            if not bool(has[a:a + 10].all()):
                want.append(float("nan"))
                continue
            x = frames[a:a + 10]
            if source_size is not None:
                x = ops.letterbox_frames(x, R_, C_, layout="CHW")
            cb = [gp.unsqueeze(0).expand(10, -1, -1, -1), op_.unsqueeze(0).expand(10, -1, -1, -1)]
            out, st = m(x, cb, state)
            state = [st[0].detach()]
            want.append(losses.loss_fu(out, y_gaze[a:a + 10]).item())
            steps += 1
    assert [np.isnan(v) for v in want] == [False, False, True, False]
    got = res["losses"].numpy()
    print("validate_video losses", got.tolist(), "manual loop", want)
    assert np.array_equal(got.view(np.uint32)[[0, 1, 3]], np.array(want, np.float32).view(np.uint32)[[0, 1, 3]]) and np.isnan(got[2])
    assert res["groups_run"] == 3 and res["num_step"] == 3
    total = want[0] + want[1] + want[3]
    assert res["run_loss"] == total and res["video_mean"] == total / 4
    again = validate_video(m, frames, gp, op_, fix_map, fix_loc, batch_size=2, **kw)
    assert np.array_equal(again["losses"].numpy().view(np.uint32), got.view(np.uint32))
    assert again["video_mean"] == res["video_mean"]
