"""The ConvLSTM backward on the GPU (train.lstm_backward, csrc/train_lstm.hip) against the float64 restatement
tests/lstm_ref64.py, which runs on the device in torch float64, and the reference's recorded autograd results
(tests/golden/lstm_train_*.npz).
Shapes (T, H, W): (3,5,7) 35 pixels, odd, h0 = c0 = None; (1,9,16) one step: no carry, c0 feeds step 0 directly; (5,12,20) a
non-zero state, the weight gradient in 2 K shares (the second 176 pixels); (2,45,80) the real map, 3 shares, the last one
1024 + 32 pixels.  Bounds: lstm_ref64's docstring.  Teacher-forced tests hand every kernel the float64 reference's inputs
rounded to fp32; each kernel must also be REJECTED, by the bound it passes, against the wrong kernels of lstm_ref64.WRONG
(the CPU test holds each at least 4 bounds away).  Free-running walks (the whole `lstm_backward`, the reference's goldens, the
step at the real map) are held to the rule of test_train_gpu.test_twa_backward_against_the_reference: twice an fp32
implementation's own gap to float64 plus the bound of the tensor's final sum."""
import math
import os
from functools import lru_cache

import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import _lib as L
from iip_uavsal_saliency_amd import losses, ops, synth, train
from iip_uavsal_saliency_amd.weights import WeightCache

import lstm_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPE_IDS = [R.name(s) for s in R.SHAPES]
RNN_W = "rnn.cell_list.0.rnn_conv.weight"


def _dev(a):
    return torch.as_tensor(a).to(DEV)


def _cl(a):
    """float32 [n,c,h,w] on the device, channels-last (what the kernels read in place)"""
    return _dev(a).float().contiguous(memory_format=torch.channels_last)


def _nhwc(a):
    return _cl(a).permute(0, 2, 3, 1)


def _dense(a):
    return _nhwc(a).contiguous()


def _nchw64(t_nhwc):
    return t_nhwc.permute(0, 3, 1, 2).double()


def _ratio(got, want, bound):
    return float(((got.double() - want).abs() / bound.clamp_min(1e-300)).max())


def _check(got, want, bound, what):
    err = (got.double() - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print("%s: worst error / bound %.4f (max |err| %.3e, max |ref| %.3e)" % (what, worst, float(err.max()), float(want.abs().max())))
    assert torch.isfinite(got).all() and bool((err <= bound).all()), what


def _reject(got, wrong, bound, what):
    worst = _ratio(got, wrong, bound)
    print("%s: worst error / bound %.1f against the wrong reference" % (what, worst))
    assert worst > 1.0, what


@lru_cache(maxsize=None)
def _teacher(shape):
    """teacher_inputs on the device (fp32), x / h0 / w of lstm_inputs, and the float64 scan of cc rounded to fp32"""
    t = {k: _dev(v) for k, v in R.teacher_inputs(shape).items()}
    inp = R.lstm_inputs(shape)
    t["x"], t["w"], t["h0"] = _dev(inp["x"]), _dev(inp["w"]), _dev(inp["h0"])
    cs, cb = R.scan_ref(t["cc"].double(), t["c0"].double())
    t["cs64"], t["cs_bound"], t["cs"] = cs, cb, cs.float()
    t["has_state"] = shape in R.STATE_NONZERO
    return t


# ------------------------------------------------------------------------------------------------ 1. teacher-forced kernels
@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_scan_kernel(shape):
    t = _teacher(shape)
    got = train.lstm_scan(_dense(t["cc"]), _dense(t["c0"]) if t["has_state"] else None)
    _check(_nchw64(got), t["cs64"], t["cs_bound"], "scan " + R.name(shape))
    z = R.split(t["cc"].double(), "ifgo")                                      # gate rows read as i, f, g, o
    bad, c = [], t["c0"].double()[0]
    for k in range(shape[0]):
        c = torch.sigmoid(z["f"][k]) * c + torch.sigmoid(z["i"][k]) * torch.tanh(z["g"][k])
        bad.append(c)
    _reject(_nchw64(got), torch.stack(bad), t["cs_bound"], "scan, gate order i f g o, " + R.name(shape))
    if t["has_state"]:                                                         # step 0 paired with zeros instead of c0
        bad, _ = R.scan_ref(t["cc"].double(), torch.zeros_like(t["c0"]).double())
        _reject(_nchw64(got), bad, t["cs_bound"], "scan, zeros for c0, " + R.name(shape))
        zero = train.lstm_scan(_dense(t["cc"]), torch.zeros_like(_dense(t["c0"])))
        none = train.lstm_scan(_dense(t["cc"]), None)
        assert torch.equal(zero.view(torch.int32), none.view(torch.int32))     # None IS zeros


def _gate_args(shape, with_carry):
    t = _teacher(shape)
    k = shape[0] - 1                                                           # the last frame: c_{t-1} is c0 when T = 1
    cp = t["cs"][k - 1:k] if k else t["c0"]
    return (t["G"][k:k + 1], t["carry_h"] if with_carry else None, t["carry_c"] if with_carry else None, t["cc"][k:k + 1],
            t["cs"][k:k + 1], cp)


def _gate(args, G=None):
    G_, ch, ccar, cc, c, cp = args
    return train.lstm_gate_bwd(_nhwc(G_) if G is None else G, None if ch is None else _dense(ch), None if ccar is None else _dense(ccar),
                               _dense(cc), _dense(c), _dense(cp))


@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("with_carry", [True, False], ids=["carries", "no carry"])
def test_gate_kernel(shape, with_carry):
    args = _gate_args(shape, with_carry)
    dcc, co = _gate(args)
    a64 = [None if a is None else a.double() for a in args]
    ref = R.gate_ref(*a64)
    for name, got in (("dcc", dcc), ("carry_c", co)):
        y, E = ref[name]
        _check(_nchw64(got), y, R.EPS * E, "gate %s %s" % (name, R.name(shape)))
    for k in ("carry_c_dropped", "c_t_in_dcc_f", "gate_order_ifgo"):
        if k == "carry_c_dropped" and not with_carry:
            continue
        bad = R.gate_ref(*a64, variant=k)
        worst = max(_ratio(_nchw64(g), bad[n][0], R.EPS * ref[n][1]) for n, g in (("dcc", dcc), ("carry_c", co)))
        print("gate %s against %s: worst error / bound %.1e" % (R.name(shape), k, worst))
        assert worst > 1.0, k


def test_gate_kernel_reads_a_channel_slice_and_writes_the_carry_in_place():
    shape = (3, 5, 7)
    args = _gate_args(shape, True)
    dense = _gate(args)
    G = args[0]
    big = torch.full((1, 512) + tuple(G.shape[2:]), 1.0e6, device=DEV).contiguous(memory_format=torch.channels_last)
    big[:, 128:384] = G
    v = big[:, 128:384].permute(0, 2, 3, 1)
    assert v.stride(2) == 512 and not v.is_contiguous()
    sliced = _gate(args, G=v)
    for a, b in zip(dense, sliced):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    ccar = _dense(args[2])
    keep = ccar.clone()
    _, co = train.lstm_gate_bwd(_nhwc(G), _dense(args[1]), ccar, _dense(args[3]), _dense(args[4]), _dense(args[5]), carry_c_out=ccar)
    assert co is ccar and not torch.equal(ccar, keep) and torch.equal(ccar.view(torch.int32), dense[1].view(torch.int32))


def test_saturated_gates_keep_their_relative_accuracy():
    """|cc| in 10 .. 30: s (1 - s) down to 1e-13, 1 - g^2 down to 4e-26.  The bound is RELATIVE to the float64 value (plus the
    fp32 underflow floor), not to 1: 1 - fl(s) would be off by 100 % here."""
    s = {k: _dev(v) for k, v in R.saturated_inputs().items()}
    dcc, co = train.lstm_gate_bwd(_nhwc(s["G"]), None, None, _dense(s["cc"]), _dense(s["c"]), _dense(s["c_prev"]))
    ref = R.gate_ref(s["G"].double(), None, None, s["cc"].double(), s["c"].double(), s["c_prev"].double())
    for name, got in (("dcc", dcc), ("carry_c", co)):
        y, E = ref[name]
        assert bool((R.EPS * E <= R.GATE_REL_MAX * R.U * y.abs() * (1 + 1e-12)).all())
        rel = ((_nchw64(got) - y).abs() / y.abs().clamp_min(1e-300))[y.abs() * R.U > R.SAT_FLOOR]
        print("saturated %s: worst relative error %.2f U over %d elements" % (name, float(rel.max()) / R.U, rel.numel()))
        _check(_nchw64(got), y, R.EPS * E + R.SAT_FLOOR, "saturated gate " + name)


@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_convs_as_lstm_backward_launches_them(shape):
    """cc = conv(W_x, x) then conv(W_h, h_prev) + res (cout 1024, gate-major rows); carry_h = conv(flip(W_h)^T, dcc_t) and
    grad_x = conv(flip(W_x)^T, dcc) over all frames (1024 -> 256)"""
    t = _teacher(shape)
    lib = L.load()
    cache, mod = WeightCache(torch.device(DEV), {}), type("W", (), {"weight": t["w"]})()
    w64 = t["w"].double()
    hp = R.hprev_of(t["hist"], t["h0"])
    first = train._conv(lib, cache, _nhwc(t["x"]), mod, 1024, 9, wslice=(0, 256))
    want, bound = R.conv_ref(t["x"].double(), w64[:, :256])
    _check(_nchw64(first), want, bound, "cc from x " + R.name(shape))
    second = train._conv(lib, cache, _dense(hp), mod, 1024, 9, wslice=(256, 512), res=first)
    want, bound = R.conv_ref(hp.double(), w64[:, 256:], _nchw64(first))
    _check(_nchw64(second), want, bound, "cc from h_prev + res " + R.name(shape))
    dcc = _dense(t["dcc"])
    got = train._conv(lib, cache, dcc[:1], mod, 256, 9, wslice=(256, 512), transposed=True)
    want, bound = R.conv_t_ref(t["dcc"][:1].double(), w64[:, 256:])
    _check(_nchw64(got), want, bound, "carry_h " + R.name(shape))
    got = train._conv(lib, cache, dcc, mod, 256, 9, wslice=(0, 256), transposed=True)
    want, bound = R.conv_t_ref(t["dcc"].double(), w64[:, :256])
    _check(_nchw64(got), want, bound, "grad_x " + R.name(shape))


@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_weight_gradient_at_1024_x_512(shape):
    t = _teacher(shape)
    hp = R.hprev_of(t["hist"], t["h0"])
    got = train.conv3_wgrad(_dense(t["dcc"]), torch.cat([_nhwc(t["x"]), _nhwc(hp)], 3))
    a64 = (t["dcc"].double(), t["x"].double(), t["hist"].double(), t["h0"].double())
    want, bound = R.wgrad_ref(*a64)
    _check(got, want, bound, "wgrad 1024 x 512 " + R.name(shape))
    if shape[0] > 1:
        _reject(got, R.wgrad_ref(*a64, "h_t_not_prev")[0], bound, "wgrad, frame t reads h_t, " + R.name(shape))
    if R.wgrad_partition(*shape)[1] > 1:
        _reject(got, R.wgrad_ref(*a64, "last_share")[0], bound, "wgrad, last K share dropped, " + R.name(shape))


# ------------------------------------------------------------------------------------------------ 2. the whole walk
NAMES = ("dW", "grad_x", "grad_h0", "grad_c0")


def _walk_tolerances(x, hist, h0, c0, w, G):
    """the float64 walk, and per tensor `2 * gap + final bound` per element: gap = max |the same walk in torch fp32 - float64|"""
    w64 = R.lstm_walk(*(a.double() for a in (x, hist, h0, c0, w, G)))
    w32 = R.lstm_walk(*(a.float() for a in (x, hist, h0, c0, w, G)))
    tol = {}
    for k in NAMES:
        gap = float((w32[k].double() - w64[k]).abs().max())
        tol[k] = 2 * gap + w64["bounds"][k]
        print("%s: torch fp32 gap %.3e, largest final bound %.3e, max |ref| %.3e" % (k, gap, float(w64["bounds"][k].max()), float(w64[k].abs().max())))
    return w64, tol


@lru_cache(maxsize=None)
def _walk_case(shape):
    t = _teacher(shape)
    inp = R.lstm_inputs(shape)
    args = (t["x"], t["hist"], t["h0"], _dev(inp["c0"]), t["w"], t["G"])
    got = train.lstm_backward(_cl(args[0]), _cl(args[1]), _cl(args[2]) if t["has_state"] else None,
                              _cl(args[3]) if t["has_state"] else None, args[4], _cl(args[5]), need_x_grad=True)
    return args, got


@lru_cache(maxsize=None)
def _walk_ref(shape):
    return _walk_tolerances(*_walk_case(shape)[0])


@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_lstm_backward_against_the_float64_walk(shape):
    """`lstm_backward` from a given history (x, state and weight of lstm_inputs, history and G of teacher_inputs) against
    lstm_ref64.lstm_walk; h0 = c0 = None at (3,5,7)."""
    args, got = _walk_case(shape)
    w64, tol = _walk_ref(shape)
    for k, g in zip(NAMES, got):
        _check(g, w64[k], tol[k], "lstm_backward %s %s" % (k, R.name(shape)))


def test_lstm_backward_is_rejected_against_every_wrong_walk():
    shape = (5, 12, 20)
    args, got = _walk_case(shape)
    w64, tol = _walk_ref(shape)
    assert bool(((got[0].double() - w64["dW"]).abs() <= tol["dW"]).all())
    a64 = [a.double() for a in args]
    for k in R.WRONG:
        bad = R.lstm_walk(*a64, variant=k, bounds=False)
        _reject(got[0], bad["dW"], tol["dW"], "lstm_backward dW against %s" % k)


@pytest.mark.parametrize("shape", R.GOLDEN_SHAPES, ids=R.name)
def test_lstm_backward_against_the_reference(shape, golden_dir):
    """Against the reference's own ConvLSTM under float64 autograd.  Per tensor in max-abs: twice the reference's own
    fp32-vs-float64 gap (a second fp32 implementation sums in another order) plus the bound of the tensor's final sum."""
    g = np.load(os.path.join(golden_dir, R.name(shape) + ".npz"))
    inp = {k: _dev(v) for k, v in R.lstm_inputs(shape).items()}
    assert str(g["digest"]) == R.digest(*(inp[k].cpu().numpy() for k in ("x", "h0", "c0", "w", "G")))
    i64 = {k: v.double() for k, v in inp.items()}
    hist, _, _ = R.lstm_forward(i64["x"], i64["h0"], i64["c0"], i64["w"])
    state = shape in R.STATE_NONZERO
    gw, gx, g0, gc = train.lstm_backward(_cl(inp["x"]), _cl(hist), _cl(inp["h0"]) if state else None, _cl(inp["c0"]) if state else None,
                                         inp["w"], _cl(inp["G"]), need_x_grad=True)
    b = R.lstm_walk(i64["x"], hist, i64["h0"], i64["c0"], i64["w"], i64["G"])["bounds"]
    for name, got, sub in (("dW", gw, R.DW_SUBSET), ("grad_x", gx, (slice(None), slice(None, None, 16))),
                           ("grad_h0", g0, (slice(None), slice(None, None, 8))), ("grad_c0", gc, (slice(None), slice(None, None, 8)))):
        gap = float(g["gap_" + name])
        err = float((got[sub].double().cpu() - torch.as_tensor(g[name])).abs().max())
        tol = 2 * gap + float(b[name].max())
        print("%s %s: max |err| %.3e = %.2f x the reference's fp32 gap %.3e; tolerance %.3e" % (R.name(shape), name, err, err / gap, gap, tol))
        assert err <= tol, name
    lim = (2 * float(g["gap_dW"]) + float(b["dW"].max())) * math.sqrt(gw.numel())
    assert abs(float(gw.double().sum()) - float(g["dW_sum"])) <= lim
    assert abs(float(gw.double().norm()) - float(g["dW_l2"])) <= lim


def test_two_calls_return_the_same_bits_and_accumulate_adds():
    shape = (5, 12, 20)
    args, first = _walk_case(shape)
    call = lambda **kw: train.lstm_backward(_cl(args[0]), _cl(args[1]), _cl(args[2]), _cl(args[3]), args[4], _cl(args[5]),      # noqa: E731
                                            need_x_grad=True, **kw)
    again = call()
    for u, v in zip(first, again):
        assert torch.equal(u.contiguous().view(torch.int32), v.contiguous().view(torch.int32))
    prev = (0.01 * torch.randn(first[0].shape, generator=torch.Generator().manual_seed(5))).to(DEV)
    out = prev.clone()
    assert call(out=out, accumulate=True)[0] is out
    want = first[0].double() + prev.double()                                   # fl(s + prev) against fl(s) + prev
    _check(out, want, 1.001 * R.U * (want.abs() + first[0].double().abs()), "lstm_backward accumulate")
    out2 = prev.clone()
    call(out=out2)
    assert torch.equal(out2, first[0])                                         # overwrite ignores the content


def test_zero_gradient_gives_zero():
    shape = (5, 12, 20)
    args, _ = _walk_case(shape)
    res = train.lstm_backward(_cl(args[0]), _cl(args[1]), _cl(args[2]), _cl(args[3]), args[4], torch.zeros_like(_cl(args[5])),
                              need_x_grad=True)
    for g in res:
        assert bool((g == 0).all())
    gw, gx, g0, gc = train.lstm_backward(_cl(args[0]), _cl(args[1]), _cl(args[2]), _cl(args[3]), args[4], _cl(args[5]))
    assert gx is None and tuple(gw.shape) == (1024, 512, 3, 3) and tuple(g0.shape) == tuple(gc.shape) == (1, 256, 12, 20)


# ------------------------------------------------------------------------------------------------ 3. the step and the driver
H_, W_, T_ = 72, 104, 4


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


def _model(time_dims=T_):
    from iip_uavsal_saliency_amd import UAVSAL_LSTM
    m = UAVSAL_LSTM(time_dims=time_dims)
    synth.load_synth_weights(m, 0)
    return m.to(DEV).eval()


def _with_grad(m):
    return [k for k, p in m.named_parameters() if p.grad is not None]


def test_recurrence_step_sets_only_the_recurrence_gradient():
    m = _model()
    x, cb, y = _step_inputs()
    rc = m.rnn.cell_list[0].rnn_conv
    assert tuple(rc.weight.shape) == (1024, 512, 3, 3)
    with pytest.raises(RuntimeError, match="UAVSAL_LSTM"):
        train.recurrence_step(m, x, cb, None, y)                                   # without the keyword: as it always was
    loss, out, st = train.recurrence_step(m, x, cb, None, y, lstm=True)
    ref_out, ref_st = m(x, cb, None)
    assert len(st) == 2 and all(torch.equal(a, b) and not a.requires_grad for a, b in zip(st, ref_st))
    assert torch.equal(out, ref_out) and loss.item() == losses.loss_fu(ref_out, y).item()
    assert _with_grad(m) == [RNN_W]
    g1 = rc.weight.grad.clone()
    assert torch.isfinite(g1).all() and float(g1.abs().max()) > 0
    train.recurrence_step(m, x, cb, None, y, lstm=True)                            # .grad += as loss.backward() would
    _check(rc.weight.grad, 2 * g1.double(), 4 * R.U * g1.double().abs(), "second call doubles the gradient")
    # a directional derivative, as in test_train_gpu: the plumbing (which buffer goes where, the decoder in between)
    with torch.no_grad():
        D = g1 / g1.norm()
        w0 = rc.weight.detach().clone()
        s = 2e-2 / float(g1.norm())
        vals = []
        for sign in (1.0, -1.0):
            rc.weight.copy_(w0 + sign * s * D)
            m.refresh_weights(m.rnn)
            vals.append(losses.loss_fu(m(x, cb, None)[0], y).item())
        rc.weight.copy_(w0)
        m.refresh_weights(m.rnn)
    fd, an = (vals[0] - vals[1]) / (2 * s), float(g1.norm())
    print("directional derivative: finite difference %.6e, <grad, D> %.6e, step %.3e" % (fd, an, s))
    assert abs(fd - an) <= 0.10 * abs(an)


def test_recurrence_step_from_a_carried_state_at_the_real_map():
    """360x640, time_dims 5, one group of five frames that starts from the (h, c) the forward left after five OTHER frames: the
    45x80 map.  The gradient agrees with lstm_ref64's walk fed the device's own taps (the recurrence's input and history) and
    the device's own grad_h."""
    HH, WW, T = 360, 640, 5
    h, w = HH // 8, WW // 8
    m = _model(T)
    frames = torch.from_numpy(synth.normalize_frames(synth.synth_frames_u8(2 * T, HH, WW, 3))).to(DEV)
    cb = [torch.from_numpy(synth.gauss_priors(T, h, w)).to(DEV), torch.from_numpy(synth.ob_priors(T, h, w, seed=3)).to(DEV)]
    loc = synth.synth_fix_points(T, 180, 320, 12, 4)
    fmap = np.rint(synth.synth_fix_maps(loc, 6.0) * 255).astype(np.uint8)
    y, has = ops.prepare_gaze(torch.from_numpy(fmap).to(DEV), torch.from_numpy(loc).to(DEV), h, w)
    assert bool(has.all())
    _, st0 = m(frames[:T], cb, None)
    state = [(st0[0].detach().clone(), st0[1].detach().clone())]
    assert all(tuple(s.shape) == (1, 256, h, w) and float(s.abs().max()) > 0 for s in state[0])
    keep = [s.clone() for s in state[0]]
    x = frames[T:]
    rc = m.rnn.cell_list[0].rnn_conv
    loss, out, st = train.recurrence_step(m, x, cb, state, y, lstm=True)
    assert all(torch.equal(a, b) for a, b in zip(state[0], keep))                  # the step left the caller's state alone
    taps = {}
    ref_out, ref_st = m(x, cb, state, taps=taps)
    assert torch.equal(out, ref_out) and all(torch.equal(a, b) for a, b in zip(st, ref_st))
    assert not torch.equal(ref_out, m(x, cb, None)[0])                             # the state matters to this group
    assert _with_grad(m) == [RNN_W]
    pred = ref_out.detach().requires_grad_(True)
    with torch.enable_grad():
        (g_y,) = torch.autograd.grad(losses.loss_fu(pred, y), pred)
    cl = torch.channels_last
    h_seq, x_seq = taps["rnn"].contiguous(memory_format=cl), taps["prefuse"].contiguous(memory_format=cl)
    grad_h = train.decoder_input_grad(m.conv_out_st, h_seq, g_y, y=ref_out)
    w64, tol = _walk_tolerances(x_seq, h_seq, state[0][0], state[0][1], rc.weight.detach(), grad_h)
    _check(rc.weight.grad, w64["dW"], tol["dW"], "the step's dW at 45x80 from a carried (h, c)")
    bad = R.lstm_walk(*(a.double() for a in (x_seq, h_seq, state[0][0], state[0][1], rc.weight.detach(), grad_h)),
                      variant="step0_zero_c", bounds=False)
    _reject(rc.weight.grad, bad["dW"], tol["dW"], "the step's dW against a walk that forgot c0")


def test_decoder_and_fuse_stages_work_behind_the_keyword():
    m = _model()
    x, cb, y = _step_inputs()
    train.recurrence_step(m, x, cb, None, y, lstm=True, decoder=True, fuse=True)
    blk, _ = train.fuse_block(m)
    want = {RNN_W} | {"conv_out_st." + n for n, _ in m.conv_out_st.named_parameters()}
    want |= {k for k, p in m.named_parameters() if any(p is q for q in blk.parameters())}
    got = _with_grad(m)
    assert set(got) == want and len(want) == 19
    assert all(torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0 for p in m.parameters() if p.grad is not None)
    rnn_only = _model()
    train.recurrence_step(rnn_only, x, cb, None, y, lstm=True)
    # a frozen decoder scales by s1 in the kernel, a trained one in the weights: the last bits of grad_h may differ
    a, b = m.rnn.cell_list[0].rnn_conv.weight.grad, rnn_only.rnn.cell_list[0].rnn_conv.weight.grad
    assert float((a - b).norm()) <= 1e-4 * float(b.norm())


@pytest.mark.parametrize("refresh", ["host", "device"])
def test_two_adam_steps_and_refresh_keep_the_plans(refresh):
    from iip_uavsal_saliency_amd import UAVSAL_LSTM
    m = _model()
    x, cb, y = _step_inputs()
    opt = torch.optim.Adam(m.rnn.parameters(), lr=1e-4, betas=(0.9, 0.999), weight_decay=5e-5)
    before = m(x, cb, None)[0]
    for _ in range(2):
        opt.zero_grad()
        train.recurrence_step(m, x, cb, None, y, lstm=True)
        engines = {k: id(e) for k, e in m._engines.items()}
        opt.step()
        assert m.refresh_weights(m.rnn, device=refresh == "device") > 0
        after = m(x, cb, None)[0]
        assert {k: id(e) for k, e in m._engines.items()} == engines                # no engine was rebuilt
    assert not torch.equal(before, after)
    fresh = UAVSAL_LSTM(time_dims=T_)
    fresh.load_state_dict(m.state_dict())
    fresh = fresh.to(DEV).eval()
    want, want_st = fresh(x, cb, None)
    got, got_st = m(x, cb, None)
    assert torch.equal(got, want) and all(torch.equal(a, b) for a, b in zip(got_st, want_st))      # bit for bit
    # the backward's own packed forms (plain and transposed, under the same module id) were refreshed too
    m.rnn.cell_list[0].rnn_conv.weight.grad = None
    fresh_loss, _, _ = train.recurrence_step(fresh, x, cb, None, y, lstm=True)
    loss, _, _ = train.recurrence_step(m, x, cb, None, y, lstm=True)
    assert loss.item() == fresh_loss.item()
    assert torch.equal(m.rnn.cell_list[0].rnn_conv.weight.grad, fresh.rnn.cell_list[0].rnn_conv.weight.grad)


@pytest.mark.parametrize("refresh", ["host", "device"])
def test_finetune_video_is_the_manual_loop(refresh):
    from iip_uavsal_saliency_amd.stream import finetune_video
    n = 4 * T_
    frames = torch.from_numpy(synth.synth_frames_u8(n, H_, W_, 2)).to(DEV)
    gp = torch.from_numpy(synth.gauss_priors(1, H_ // 8, W_ // 8)[0]).to(DEV)
    op_ = torch.from_numpy(synth.ob_priors(1, H_ // 8, W_ // 8)[0]).to(DEV)
    loc = synth.synth_fix_points(n, 90, 130, 12, 9)
    fmap = np.rint(synth.synth_fix_maps(loc, 6.0) * 255).astype(np.uint8)
    fix_map, fix_loc = torch.from_numpy(fmap).to(DEV), torch.from_numpy(loc).to(DEV)
    adam = lambda m: torch.optim.Adam(m.rnn.parameters(), lr=1e-4, betas=(0.9, 0.999), weight_decay=5e-5)      # noqa: E731
    a = _model()
    res = finetune_video(a, frames, gp, op_, fix_map, fix_loc, adam(a), batch_size=2, refresh=refresh)
    assert res["groups_run"] == 2 and not bool(torch.isnan(res["losses"]).any())
    b = _model()
    opt = adam(b)
    y, has = ops.prepare_gaze(fix_map, fix_loc, H_ // 8, W_ // 8)
    assert bool(has.all())
    state, manual = None, []
    for lo in range(0, n, 2 * T_):
        x = frames[lo:lo + 2 * T_]
        cb = [gp.unsqueeze(0).expand(2 * T_, -1, -1, -1), op_.unsqueeze(0).expand(2 * T_, -1, -1, -1)]
        opt.zero_grad()
        loss, _, st = train.recurrence_step(b, x, cb, state, y[lo:lo + 2 * T_], lstm=True)
        state = [(st[0].detach(), st[1].detach())]
        opt.step()
        b.refresh_weights(b.rnn, device=refresh == "device")
        manual.append(loss.item())
    assert res["losses"].tolist() == manual                                        # bit for bit
    assert torch.equal(a.rnn.cell_list[0].rnn_conv.weight, b.rnn.cell_list[0].rnn_conv.weight)
    assert _with_grad(a) == [RNN_W]
