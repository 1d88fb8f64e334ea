"""Criterion, gaze ground truth and validation driver: everything that needs no GPU.  The built library is inspected
through ctypes, the float64 restatement (tests/loss_ref64.py) is held against the reference's recorded outputs
(tests/golden/loss_*.npz, written by tools/make_loss_goldens.py), and `stream.validate_video` runs with the forward, the
criterion and the ground truth replaced by host stand-ins."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import _lib, losses, stream

import letterbox_ref
import loss_ref64 as R

VALUES = ("metric_kl", "metric_cc", "metric_nss", "loss_fu", "loss_kl")


def _golden(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def _frame_rel(a, b):
    """per frame: max |a - b| relative to the frame's largest |b| (0 for a frame where both are zero everywhere)"""
    n = len(a)
    return np.abs(a - b).reshape(n, -1).max(1) / np.maximum(np.abs(b).reshape(n, -1).max(1), np.finfo(np.float64).tiny)


# ------------------------------------------------------------------------------------------------ library

def test_library_has_the_loss_symbols():
    lib = _lib.load()
    for name in ("uavsal_gaze_prepare", "uavsal_loss_fu", "uavsal_loss_fu_grad"):
        assert hasattr(lib, name)
        assert name in [s[0] for s in _lib.SYMBOLS]
    assert lib.uavsal_abi_version() == 20


def test_descriptor_sizes():
    lib = _lib.load()
    assert _lib.DESC_TYPES[17] is _lib.GazeDesc and _lib.DESC_TYPES[18] is _lib.LossDesc
    assert lib.uavsal_sizeof_desc(17) == C.sizeof(_lib.GazeDesc)
    assert lib.uavsal_sizeof_desc(18) == C.sizeof(_lib.LossDesc)
    assert _lib.DESC_TYPES[19] is _lib.ConvRoute and lib.uavsal_sizeof_desc(19) == C.sizeof(_lib.ConvRoute)
    assert len(_lib.DESC_TYPES) == 20 and lib.uavsal_sizeof_desc(20) < 0


def test_arguments_are_checked_before_any_launch():
    lib = _lib.load()
    assert lib.uavsal_loss_fu(None, None) == -1
    assert lib.uavsal_loss_fu_grad(None, None) == -1
    assert lib.uavsal_gaze_prepare(None, None) == -1
    d = _lib.LossDesc()
    d.pred, d.truth, d.stats, d.out, d.n_img, d.n_pix = 4096, 8192, 16384, 32768, 3, 1
    assert lib.uavsal_loss_fu(C.byref(d), None) == -3          # the unbiased std of one pixel
    d.n_pix, d.out = 16, None
    assert lib.uavsal_loss_fu(C.byref(d), None) == -1
    assert lib.uavsal_loss_fu_grad(C.byref(d), None) == -1     # no grad / grad_out
    g = _lib.GazeDesc()
    g.fix_map, g.fix_loc, g.out, g.flags = 4096, 8192, 16384, 32768
    g.n_img, g.h0, g.w0, g.h, g.w = 1, 4000, 1, 45, 80         # the picture would have no column
    assert lib.uavsal_gaze_prepare(C.byref(g), None) == -3
    g.h0, g.w0, g.map_col_pitch = 180, 320, -1
    assert lib.uavsal_gaze_prepare(C.byref(g), None) == -1


def test_cpu_tensors_raise():
    p, t = torch.rand(2, 1, 9, 16), torch.rand(2, 2, 9, 16)
    for fn in (losses.loss_fu, losses.loss_kl, losses.metric_kl, losses.metric_cc, losses.metric_nss):
        with pytest.raises(RuntimeError, match="cuda"):
            fn(p, t)
    with pytest.raises(RuntimeError, match="cuda"):
        losses.loss_fu_dy(p[None], t[None])
    from iip_uavsal_saliency_amd import ops
    with pytest.raises(RuntimeError, match="cuda"):
        ops.prepare_gaze(torch.zeros(2, 18, 32, dtype=torch.uint8), torch.zeros(2, 18, 32, dtype=torch.uint8), 9, 16)


# ------------------------------------------------------------------------------------------------ restatement against the reference

@pytest.mark.parametrize("name,h,w,B,seed", R.RANDOM_CASES)
def test_restatement_reproduces_the_reference_float64(golden_dir, name, h, w, B, seed):
    g = _golden(golden_dir, "loss_%s_f64.npz" % name)
    y_pred, y_true = R.random_inputs(h, w, B, seed)
    assert str(g["digest"]) == R.digest(y_pred, y_true)
    kl, cc, nss, fu = R.loss(y_pred, y_true)
    got = {"metric_kl": kl, "metric_cc": cc, "metric_nss": nss, "loss_fu": fu, "loss_kl": R.loss(y_pred, y_true, R.LOSS_KL)[3]}
    for k in VALUES:
        rel = abs(got[k] - float(g[k])) / abs(float(g[k]))
        print("%s %s: restatement %.17g reference %.17g rel %.2e" % (name, k, got[k], float(g[k]), rel))
        assert rel <= 1e-12
    # the gradient: relative to the frame's largest magnitude (an element near a sign change has no digits of its own)
    rel = _frame_rel(R.loss_grad(y_pred, y_true), g["grad_loss_fu"])
    print("%s gradient of loss_fu: per-frame relative difference up to %.2e" % (name, rel.max()))
    assert rel.max() <= 1e-12


def test_mean_of_the_first_64_frames_is_not_the_mean():
    """The condition of the GPU test's wrong reference at B = 65, from the restatement alone: every value averaged over the first
    64 frames only lies at least 4 fp32 ulps from the value over all 65, so a device value within one ulp of the right one
    cannot also be within one ulp of the wrong one.  The cases beyond 64 frames are what their names say."""
    assert [c[:4] for c in R.STRIDE_CASES] == [("12x20_B65", 12, 20, 65), ("9x15_B130", 9, 15, 130)]
    assert (12 * 20) % 4 == 0 and (9 * 15) % 4 != 0                          # the vector and the scalar path of csrc/loss.hip
    assert not {c[0] for c in R.STRIDE_CASES} & {c[0] for c in R.RANDOM_CASES}
    name, h, w, B, seed = R.STRIDE_CASES[0]
    y_pred, y_true = R.random_inputs(h, w, B, seed)
    n = R.MEAN_LANES
    assert B == n + 1
    for weights, names in ((R.LOSS_FU, VALUES[:4]), (R.LOSS_KL, ("loss_kl",))):
        right, wrong = R.loss(y_pred, y_true, weights)[-len(names):], R.loss(y_pred[:n], y_true[:n], weights)[-len(names):]
        for k, a, b in zip(names, right, wrong):
            ulp = float(np.spacing(np.float32(abs(a))))
            print("%s %s: all %d frames %.17g, the first %d %.17g: %.0f ulps apart" % (name, k, B, a, n, b, abs(a - b) / ulp))
            assert abs(a - b) >= 4 * ulp, k
    for name, h, w, B, seed in R.STRIDE_CASES:                                # no degenerate frame in either case
        kl, cc, nss = R.frame_metrics(*R.random_inputs(h, w, B, seed))
        assert np.isfinite(kl).all() and np.isfinite(cc).all() and np.isfinite(nss).all() and len(kl) == B
        assert np.isfinite(R.loss_grad(*R.random_inputs(h, w, B, seed))).all()


def test_restatement_reproduces_the_reference_on_the_edge_batch(golden_dir):
    g = _golden(golden_dir, "loss_edge_45x80.npz")
    y_pred, y_true = R.edge_inputs()
    assert str(g["digest"]) == R.digest(y_pred, y_true)
    kl, cc, nss = R.frame_metrics(y_pred, y_true)
    for f in R.EDGE_CONSTANT:                                  # a constant prediction contributes exactly 0 to cc and nss
        assert cc[f] == 0.0 and nss[f] == 0.0
    assert kl[R.EDGE_ZERO_MAP] == 0.0 and cc[R.EDGE_ZERO_MAP] == 0.0 and nss[R.EDGE_ZERO_MAP] == 0.0
    got = dict(zip(VALUES, R.loss(y_pred, y_true)))
    got["loss_kl"] = R.loss(y_pred, y_true, R.LOSS_KL)[3]
    for k in VALUES:
        assert abs(got[k] - float(g["f64_" + k])) <= 1e-12 * abs(float(g["f64_" + k]))
    ref_fu, ref_kl = g["f64_grad_loss_fu"], g["f64_grad_loss_kl"]
    nan_frames = np.isnan(ref_fu).reshape(len(ref_fu), -1)
    # the reference: NaN over the whole frame for constant predictions (torch.std at zero) and for the all-zero map (sqrt at
    # zero inside r2), finite elsewhere; loss_kl finite everywhere
    assert nan_frames.all(1).nonzero()[0].tolist() == sorted([R.EDGE_ZERO_MAP] + list(R.EDGE_CONSTANT))
    assert nan_frames.any(1).tolist() == nan_frames.all(1).tolist()
    assert np.isfinite(ref_kl).all()
    fu, klg = R.loss_grad(y_pred, y_true), R.loss_grad(y_pred, y_true, R.LOSS_KL)
    for f in R.EDGE_CONSTANT:
        assert np.isnan(fu[f]).all()
    others = [f for f in range(len(fu)) if f not in R.EDGE_CONSTANT]
    assert np.isfinite(fu[others]).all() and np.isfinite(klg).all()
    both = [f for f in others if f != R.EDGE_ZERO_MAP]
    assert _frame_rel(fu[both], ref_fu[both]).max() <= 1e-12
    assert _frame_rel(klg, ref_kl).max() <= 1e-12


def test_fp32_goldens_record_their_gap(golden_dir):
    for name, *_ in R.RANDOM_CASES:
        g32, g64 = _golden(golden_dir, "loss_%s_f32.npz" % name), _golden(golden_dir, "loss_%s_f64.npz" % name)
        assert g32["grad_loss_fu"].dtype == np.float32 and g64["grad_loss_fu"].dtype == np.float64
        for k in VALUES:
            assert float(g32["gap_" + k]) == abs(float(g32[k]) - float(g64[k]))
            assert float(g32["gap_" + k]) <= 4e-6 * max(1.0, abs(float(g64[k])))      # fp32 summation noise, nothing else
        assert (g32["gap_grad_loss_fu"] == _frame_rel(g32["grad_loss_fu"].astype(np.float64), g64["grad_loss_fu"])).all()
        assert g32["gap_grad_loss_fu"].max() < 1e-5
        assert float(g32["cpu_s_fwd_45x80_B20"]) > 0 and float(g32["cpu_s_fwdbwd_90x160_B64"]) > 0


@pytest.mark.parametrize("h0,w0,h,w", R.SCATTER_CASES)
def test_fixation_scatter_is_bit_identical_to_the_reference(golden_dir, h0, w0, h, w):
    g = _golden(golden_dir, "loss_scatter.npz")
    key = "%dx%d_to_%dx%d" % (h0, w0, h, w)
    fmap, loc = R.scatter_inputs(h0, w0)
    assert str(g["digest_" + key]) == R.digest(fmap, loc)
    want = g["fix_" + key]
    got = np.stack([R.padding_fixation(loc[i], h, w) for i in range(len(loc))])
    assert got.dtype == want.dtype and np.array_equal(got, want)
    if (h0, w0) == (h, w):
        assert np.array_equal(got, loc) and got.max() == 7     # the identity branch hands the values through
    else:
        assert got.max() == 1 and not got[2].any()
    y, has = R.prepare_gaze(fmap, loc, h, w)
    assert np.array_equal(y[:, 1], want.astype(np.float32))
    assert has[:, 1].tolist() == [True, True, False, True]


def test_map_channel_is_the_shared_resize_rule():
    """channel 0 = letterbox_ref.resize_u8 inside the letterbox geometry: one map is the first plane of a grey frame"""
    for h0, w0, h, w in R.SCATTER_CASES:
        fmap, loc = R.scatter_inputs(h0, w0)
        y, has = R.prepare_gaze(fmap, loc, h, w)
        grey = np.repeat(fmap[:, :, :, None], 3, axis=3)
        want = letterbox_ref.letterbox(grey, h, w, layout="HWC")[:, 0]
        assert np.array_equal(y[:, 0], want.astype(np.float32))
        assert has[:, 0].tolist() == [True, True, False, True]
        if (h0, w0) == (h, w):
            assert np.array_equal(want, fmap)


# ------------------------------------------------------------------------------------------------ validation driver

class _StubModel:
    """counts its calls; the state it returns names the groups it has seen"""
    time_dims = 5

    def __init__(self):
        self.calls = []
        self._p = torch.zeros(1)

    def parameters(self):
        return iter([self._p])

    def __call__(self, x, cb, state):
        seen = 0.0 if state is None else float(state[0])
        assert cb[0].shape[0] == x.shape[0] and cb[1].shape[0] == x.shape[0]
        self.calls.append((int(x[0, 0, 0, 0]), x.shape[0], seen))
        return x[:, :1, :9, :16].float(), [torch.tensor(seen + 1.0)]


def _stub_video(n_frames, empty=()):
    frames = torch.zeros(n_frames, 3, 72, 128, dtype=torch.uint8)
    frames[:, 0, 0, 0] = torch.arange(n_frames, dtype=torch.uint8)            # a frame carries its index
    has = torch.ones(n_frames, 2, dtype=torch.bool)
    for f, c in empty:
        has[f, c] = False

    def prepare(fix_map, fix_loc, h, w, layout):
        assert (h, w) == (9, 16)
        return torch.zeros(n_frames, 2, h, w), has

    def criterion(out, y):
        assert out.shape[0] == y.shape[0]
        return out[0, 0, 0, 0] + 0.25 * out.shape[0]                          # first frame index + 0.25 * group size

    return frames, prepare, criterion


def _validate(model, n_frames, empty=(), batch_size=2):
    frames, prepare, criterion = _stub_video(n_frames, empty)
    fix = torch.zeros(n_frames, 4, 4, dtype=torch.uint8)
    return stream.validate_video(model, frames, torch.zeros(8, 9, 16), torch.zeros(20, 9, 16), fix, fix,
                                 batch_size=batch_size, criterion=criterion, prepare=prepare)


def test_validation_groups_follow_the_reference_loop():
    has = [[True, True]] * 43
    # 43 frames, time_dims 5: 8 chunks = 40 frames; groups of 2 chunks
    assert stream.validation_groups(43, 5, 2, has) == [(0, 10, True), (10, 20, True), (20, 30, True), (30, 40, True)]
    # 3 chunks per group: the last group is shorter
    assert stream.validation_groups(43, 5, 3, has) == [(0, 15, True), (15, 30, True), (30, 40, True)]
    has = [[True, True] for _ in range(43)]
    has[12][1] = False                                     # no fixation in one frame: its group is out
    has[41][0] = False                                     # beyond the cut: ignored
    assert [g[2] for g in stream.validation_groups(43, 5, 2, has)] == [True, False, True, True]
    has[25][0] = False                                     # an all-zero map in another
    assert [g[2] for g in stream.validation_groups(43, 5, 2, has)] == [True, False, False, True]


def test_validate_video_skips_before_the_forward_and_divides_by_all_groups():
    m = _StubModel()
    r = _validate(m, 43, empty=[(12, 1)])
    # groups start at frames 0, 10, 20, 30; the second is skipped before its forward: the third sees the state of the first
    assert m.calls == [(0, 10, 0.0), (20, 10, 1.0), (30, 10, 2.0)]
    want = [0 + 2.5, float("nan"), 20 + 2.5, 30 + 2.5]
    got = r["losses"].tolist()
    assert r["losses"].dtype == torch.float32 and len(got) == 4
    assert [math.isnan(v) for v in got] == [False, True, False, False]
    assert [v for v in got if not math.isnan(v)] == [v for v in want if not math.isnan(v)]
    assert r["groups_run"] == 3 and r["num_step"] == 3
    assert r["run_loss"] == 2.5 + 22.5 + 32.5
    assert r["video_mean"] == (2.5 + 22.5 + 32.5) / 4      # all four groups, the skipped one included
    assert r["run_loss"] / r["num_step"] != r["video_mean"]


def test_validate_video_short_last_group_and_all_skipped():
    m = _StubModel()
    r = _validate(m, 27, batch_size=2)                     # 5 chunks: groups of 10, 10, 5
    assert m.calls == [(0, 10, 0.0), (10, 10, 1.0), (20, 5, 2.0)]
    assert r["losses"].tolist() == [2.5, 12.5, 21.25]
    assert r["video_mean"] == (2.5 + 12.5 + 21.25) / 3
    m = _StubModel()
    r = _validate(m, 20, empty=[(3, 0), (15, 1)])
    assert m.calls == [] and r["groups_run"] == 0 and r["num_step"] == 0
    assert all(math.isnan(v) for v in r["losses"].tolist()) and r["video_mean"] == 0.0
    with pytest.raises(RuntimeError, match="full chunk"):
        _validate(_StubModel(), 4)


def test_validate_video_takes_the_shortest_of_frames_and_ground_truth():
    m = _StubModel()
    frames, prepare, criterion = _stub_video(43)

    def shorter(fix_map, fix_loc, h, w, layout):
        y, has = prepare(fix_map, fix_loc, h, w, layout)
        return y[:31], has[:31]                            # 31 ground-truth frames: 6 chunks

    fix = torch.zeros(31, 4, 4, dtype=torch.uint8)
    r = stream.validate_video(m, frames, torch.zeros(8, 9, 16), torch.zeros(20, 9, 16), fix, fix, batch_size=4,
                              criterion=criterion, prepare=shorter)
    assert m.calls == [(0, 20, 0.0), (20, 10, 1.0)] and len(r["losses"]) == 2


def test_validation_aggregates():
    a = stream.validation_aggregates([1.5, float("nan"), 2.0])
    assert a == {"video_mean": 3.5 / 3, "run_loss": 3.5, "num_step": 2}
