"""Recurrence modes on the MI355X: the seam launches and the zero initial state leave maps, returned state
and the `rnn` tap bit for bit what the recorded launches give -- compared with a second model on the same weights that has both
switches off -- on every calling surface; `uavsal_plan_mode_report` says what a run did; the plans and states that must run in
full do; and both modes together meet the committed goldens."""
import os

import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import synth

pytestmark = pytest.mark.gpu

# (H, W, frames per clip, clips): 9 x 13, 12 x 20 (one and two clips) and 5 x 7 maps
PLANS = [(72, 104, 3, 1), (96, 160, 4, 1), (96, 160, 4, 2), (40, 56, 2, 1)]

_MODELS = {}


def models(T, prec="f32", rnn="twa", **attrs):
    """(model with the modes, model with both switched off) on the same synthetic weights."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from iip_uavsal_saliency_amd import UAVSal
    key = (T, prec, rnn, tuple(sorted(attrs.items())))
    if key not in _MODELS:
        ms = []
        for on in (True, False):
            if rnn == "lstm":
                from iip_uavsal_saliency_amd import UAVSAL_LSTM
                m = UAVSAL_LSTM(time_dims=T, precision=prec)
            else:
                m = UAVSal(time_dims=T, precision=prec)
            synth.load_synth_weights(m, 0)
            m = m.cuda().eval()
            m.fuse_seams = m.skip_zero_state = on
            for k, v in attrs.items():
                setattr(m, k, v)
            ms.append(m)
        _MODELS[key] = ms
    return _MODELS[key]


def inputs(H, W, T, clips, seed=0, t0=0):
    n = T * clips
    h, w = (H + 7) // 8, (W + 7) // 8
    x = torch.from_numpy(synth.normalize_frames(synth.synth_frames_u8(n, H, W, seed, t0))).cuda()
    cb = [torch.from_numpy(synth.gauss_priors(n, h, w)).cuda(), torch.from_numpy(synth.ob_priors(n, h, w, seed=seed)).cuda()]
    return x, cb


def as_clips(x, cb, T, clips):
    return x.view(clips, T, *x.shape[1:]), [t.view(clips, T, *t.shape[1:]) for t in cb]


def eng_of(m):
    return list(m._engines.values())[-1]


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return all(torch.equal(bits(p), bits(q)) for p, q in zip(a, b))


def run(m, H, W, T, clips, state=None, taps=None, t0=0):
    """(map, state[, rnn tap]) of one call: `forward` for one clip, `forward_clips` for more."""
    x, cb = inputs(H, W, T, clips, t0=t0)
    if clips == 1:
        out, st = m(x, cb, None if state is None else [state], taps)
        st = st[0]
    else:
        xc, cbc = as_clips(x, cb, T, clips)
        out, st = m.forward_clips(xc, cbc, state, taps)
    torch.cuda.synchronize()
    return (out, st) + ((taps["rnn"],) if taps is not None else ())


@pytest.mark.parametrize("H,W,T,clips", PLANS)
def test_forward_and_forward_clips_bitwise(H, W, T, clips):
    """Zero state (None) and a carried state, with the `rnn` tap: maps, state and tap equal the full path's, T - 1 pairs are
    fused, the zero state leaves three ops out (the state layout, step 0's input transform and GEMM) and the op count of the
    run does not move."""
    on, off = models(T)
    a = run(on, H, W, T, clips, taps={})
    b = run(off, H, W, T, clips, taps={})
    assert same(a, b)
    ea, eb = eng_of(on), eng_of(off)
    assert ea.mode_report()[:2] == (T - 1, 3) and eb.mode_report()[:2] == (0, 0)
    assert ea.last_launches() == eb.last_launches()
    assert ea.mode_report()[2] == eb.mode_report()[2] - (T - 1) - 3
    # second call: the state the first returned (non-zero) -- the seams stay, step 0 runs in full
    a2 = run(on, H, W, T, clips, state=a[1], taps={}, t0=T * clips)
    b2 = run(off, H, W, T, clips, state=b[1], taps={}, t0=T * clips)
    assert same(a2, b2)
    assert eng_of(on).mode_report()[:2] == (T - 1, 0)
    # (forward_clips of one clip is a plan of its own)
    if clips == 1:
        x, cb = inputs(H, W, T, 1)
        xc, cbc = as_clips(x, cb, T, 1)
        assert same(on.forward_clips(xc, cbc), off.forward_clips(xc, cbc))
        assert eng_of(on).mode_report()[:2] == (T - 1, 3)


@pytest.mark.parametrize("H,W,T,clips", PLANS)
def test_persistent_state_and_run_streamed_bitwise(H, W, T, clips):
    """Resident state: a reset (None) arms the zero state, the resident view handed back does not; `run_streamed` arms it for
    the tail range of a reset group only."""
    on, off = models(T, persistent_state=True)
    outs = []
    for m in (on, off):
        a = run(m, H, W, T, clips)
        rep0 = eng_of(m).mode_report()
        first = (a[0].clone(), a[1].clone())
        b = run(m, H, W, T, clips, state=a[1], t0=T * clips)
        outs.append((first, (b[0].clone(), b[1].clone()), rep0, eng_of(m).mode_report()))
    assert same(outs[0][0], outs[1][0]) and same(outs[0][1], outs[1][1])
    assert outs[0][2][:2] == (T - 1, 2) and outs[0][3][:2] == (T - 1, 0)      # (a resident plan has no state layout to leave out)
    assert outs[1][2][:2] == (0, 0) and outs[1][3][:2] == (0, 0)
    streamed = []
    for m in (on, off):
        eng = eng_of(m)
        res = []
        for g in range(2):
            x, cb = inputs(H, W, T, clips, t0=g * T * clips)
            o = eng.run_streamed(x, cb[0], cb[1], prev=eng, reset=(g == 0))
            torch.cuda.synchronize()
            res.append((o.clone(), eng.named["h0"].t.clone(), eng.mode_report()))
        streamed.append(res)
    for g in range(2):
        assert same(streamed[0][g][:2], streamed[1][g][:2])
        assert streamed[0][g][2][:2] == (T - 1, 2 if g == 0 else 0) and streamed[1][g][2][:2] == (0, 0)
    # and the streamed groups are the sequential calls
    assert torch.equal(bits(streamed[0][0][0]), bits(outs[0][0][0].view_as(streamed[0][0][0])))


def test_plans_that_run_in_full():
    """A debug plan (poison fills between the transforms), a split-precision plan, a ConvLSTM model and a four-clip plan
    (F(4x4) steps): no pair fused, nothing left out, and -- where there is a twin -- the same bits as with the switches off."""
    H, W, T = 96, 160, 4
    for kw, clips in ((dict(arena_debug=True), 1), (dict(prec="f16x3"), 1), (dict(rnn="lstm"), 1), (dict(), 4)):
        on, off = models(T, **kw)
        if kw.get("rnn") == "lstm":
            x, cb = inputs(H, W, T, 1)
            outs = [m(x, cb)[0] for m in (on, off)]
            torch.cuda.synchronize()
            assert torch.equal(bits(outs[0]), bits(outs[1]))
        else:
            assert same(run(on, H, W, T, clips), run(off, H, W, T, clips)), kw
        assert eng_of(on).mode_report()[:2] == (0, 0), kw


def test_zero_state_arming():
    """None arms at once; a zeros tensor on the second call with it; an in-place edit is a miss, runs in full and equals the
    full path; -0.0, a non-zero tensor and `skip_zero_state = False` never arm."""
    H, W, T = 72, 104, 3
    on, off = models(T)
    h, w = 9, 13
    left_out = lambda m: eng_of(m).mode_report()[1]
    ref0 = run(off, H, W, T, 1)
    assert same(run(on, H, W, T, 1), ref0) and left_out(on) == 3
    z = torch.zeros(1, 256, h, w, device="cuda")
    assert same(run(on, H, W, T, 1, state=z), ref0) and left_out(on) == 0          # first sight: in full, test started
    assert same(run(on, H, W, T, 1, state=z), ref0) and left_out(on) == 3          # (run() synchronised: the answer is in)
    assert same(run(on, H, W, T, 1, state=z), ref0) and left_out(on) == 3
    z[0, 5, 2, 3] = 0.25                                                            # in place: the version moves
    ref1 = run(off, H, W, T, 1, state=z)
    assert not same(ref1, ref0)
    assert same(run(on, H, W, T, 1, state=z), ref1) and left_out(on) == 0
    assert same(run(on, H, W, T, 1, state=z), ref1) and left_out(on) == 0          # tested by now, and not zero
    z.zero_()
    assert same(run(on, H, W, T, 1, state=z), ref0) and left_out(on) == 0
    assert same(run(on, H, W, T, 1, state=z), ref0) and left_out(on) == 3
    on.invalidate_state()
    assert same(run(on, H, W, T, 1, state=z), ref0) and left_out(on) == 0
    neg = -torch.zeros(1, 256, h, w, device="cuda")
    refn = run(off, H, W, T, 1, state=neg)
    for _ in range(3):
        assert same(run(on, H, W, T, 1, state=neg), refn) and left_out(on) == 0
    nz = torch.full((1, 256, h, w), 0.5, device="cuda")
    refz = run(off, H, W, T, 1, state=nz)
    for _ in range(3):
        assert same(run(on, H, W, T, 1, state=nz), refz) and left_out(on) == 0
    # the switch alone: seams stay, nothing is left out
    on.skip_zero_state = False
    try:
        assert same(run(on, H, W, T, 1), ref0) and eng_of(on).mode_report()[:2] == (T - 1, 0)
    finally:
        on.skip_zero_state = True
    # op by op (the float64 walkers, the per-op timer) everything runs in full
    eng = eng_of(on)
    run(on, H, W, T, 1)
    for i in range(len(eng.ops_meta)):
        eng.run_ops(i, i + 1)
    torch.cuda.synchronize()
    assert eng.mode_report()[:2] == (0, 0)
    # the native plan takes neighbours only: with another op between the two transforms the pair is refused
    steps = eng.rec.twa_steps
    assert eng.lib.uavsal_plan_seam(eng.plan, steps[0]["xout"], steps[2]["xin"], 1) == 0
    assert eng.lib.uavsal_plan_seam(eng.plan, steps[0]["xout"], steps[1]["xin"], 1) == 1
    assert same(run(on, H, W, T, 1), ref0) and eng_of(on).mode_report()[:2] == (T - 1, 3)


@pytest.mark.parametrize("name", ["e2e_72x104_T3", "e2e_96x160_T4"])
def test_both_modes_against_the_goldens(golden_dir, name):
    from test_hip_e2e import MAP_TOL, STATE_TOL
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    H, W, T, B = int(g["H"]), int(g["W"]), int(g["T"]), int(g["B"])
    assert B == 1 and int(g["calls"]) == 1
    on, _ = models(T)
    x = torch.from_numpy(synth.normalize_frames(synth.synth_frames_u8(T, H, W, int(g["seed"]), 0))).cuda()
    cb = [torch.from_numpy(synth.gauss_priors(T, H // 8, W // 8)).cuda(),
          torch.from_numpy(synth.ob_priors(T, H // 8, W // 8, seed=int(g["seed"]))).cuda()]
    out, st = on(x, cb, None)
    torch.cuda.synchronize()
    assert eng_of(on).mode_report()[:2] == (T - 1, 3)
    assert np.abs(out.cpu().numpy() - g["out"]).max() <= MAP_TOL["f32"]
    assert np.abs(st[0].cpu().contiguous().view(-1).numpy()[::int(g["state_stride"])] - g["state"]).max() <= STATE_TOL["f32"]
