"""The ConvLSTM backward without a GPU: the C ABI of csrc/train_lstm.hip (sizes, every refusal before a launch), the float64
restatement tests/lstm_ref64.py against torch autograd and against the reference's recorded results
(tests/golden/lstm_train_*.npz), the weight gradient's K split against the library's own query, the argument errors of
`recurrence_step(lstm=...)`, and the conditions under which the GPU tests say something, asserted on float64 alone: the share
of saturated pre-activations in the seeded inputs, and every wrong walk of lstm_ref64.WRONG at least 4 bounds from the right one."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import _lib, train

import lstm_ref64 as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def lib():
    from iip_uavsal_saliency_amd import build
    build.build()
    return _lib.load()


def test_symbols_sizes_and_abi(lib):
    names = [s[0] for s in _lib.SYMBOLS]
    for n in ("uavsal_lstm_scan", "uavsal_lstm_gate_bwd", "uavsal_lstm_sizeof_desc"):
        assert n in names and hasattr(lib, n)
    assert _lib.LSTM_DESC_TYPES == [_lib.LstmScanDesc, _lib.LstmGateDesc]
    for i, t in enumerate(_lib.LSTM_DESC_TYPES):
        assert lib.uavsal_lstm_sizeof_desc(i) == C.sizeof(t)
    assert lib.uavsal_lstm_sizeof_desc(2) < 0 and lib.uavsal_lstm_sizeof_desc(-1) < 0
    assert lib.uavsal_abi_version() == 20 and len(_lib.DESC_TYPES) == 20            # additions only
    from iip_uavsal_saliency_amd import build
    assert "train_lstm.hip" in build.SOURCES


def test_every_refusal_comes_back_before_a_launch(lib):
    """No GPU here: a call that reached hipLaunchKernel would not return one of these codes."""
    s = _lib.LstmScanDesc()
    assert lib.uavsal_lstm_scan(None, None) == -1
    assert lib.uavsal_lstm_scan(C.byref(s), None) == -1                      # null pointers
    s.cc = s.c_seq = 256
    assert lib.uavsal_lstm_scan(C.byref(s), None) == -1                      # sizes <= 0
    s.T, s.n_pix, s.C = 2, 12, 6
    assert lib.uavsal_lstm_scan(C.byref(s), None) == -2                      # C % 4: UAVSAL_EALIGN
    s.C = 8
    s.cc = 260
    assert lib.uavsal_lstm_scan(C.byref(s), None) == -2                      # a misaligned pointer
    s.cc, s.c0 = 256, 264
    assert lib.uavsal_lstm_scan(C.byref(s), None) == -2                      # c0 is optional, but aligned when given
    s.c0, s.c_seq = 0, 520
    assert lib.uavsal_lstm_scan(C.byref(s), None) == -2
    s.c_seq, s.n_pix = 512, 1 << 45
    assert lib.uavsal_lstm_scan(C.byref(s), None) == -3                      # more than one launch indexes: UAVSAL_ESHAPE
    g = _lib.LstmGateDesc()
    assert lib.uavsal_lstm_gate_bwd(None, None) == -1
    assert lib.uavsal_lstm_gate_bwd(C.byref(g), None) == -1
    ptrs = ("g", "cc", "c", "c_prev", "dcc", "carry_c_out")
    for p in ptrs:
        setattr(g, p, 256)
    g.n_pix, g.C, g.ldg = 12, 8, 8
    for p in ptrs:                                                            # each required pointer on its own
        setattr(g, p, 0)
        assert lib.uavsal_lstm_gate_bwd(C.byref(g), None) == -1, p
        setattr(g, p, 260)
        assert lib.uavsal_lstm_gate_bwd(C.byref(g), None) == -2, p
        setattr(g, p, 256)
    for p in ("carry_h", "carry_c"):                                          # optional, aligned when given
        setattr(g, p, 264)
        assert lib.uavsal_lstm_gate_bwd(C.byref(g), None) == -2, p
        setattr(g, p, 0)
    g.C = 6
    assert lib.uavsal_lstm_gate_bwd(C.byref(g), None) == -2                  # C % 4
    g.C, g.ldg = 8, 4
    assert lib.uavsal_lstm_gate_bwd(C.byref(g), None) == -1                  # rows shorter than C
    g.ldg = 10
    assert lib.uavsal_lstm_gate_bwd(C.byref(g), None) == -2                  # ldg % 4
    g.ldg, g.n_pix = 8, 0
    assert lib.uavsal_lstm_gate_bwd(C.byref(g), None) == -1
    g.n_pix = 1 << 45
    assert lib.uavsal_lstm_gate_bwd(C.byref(g), None) == -3


def test_wgrad_share_count_is_the_restated_partition(lib):
    """`uavsal_conv3_wgrad_shares` at Co = 1024, Ci = 512 against lstm_ref64.wgrad_partition; the split is real at two of SHAPES."""
    table = {(3, 5, 7): (1, 1, 105), (1, 9, 16): (1, 1, 144), (5, 12, 20): (1, 2, 176), (2, 45, 80): (3, 3, 1056),
             (20, 45, 80): (24, 3, 22848)}                                                    # (cps, shares, last share)
    for shape in R.SHAPES + [(5, 45, 80), (20, 45, 80)]:
        T, H, W = shape
        cps, shares, spans = R.wgrad_partition(T, H, W)
        d = _lib.Conv3WgradDesc()
        d.n_img, d.H, d.W, d.Co, d.Ci = T, H, W, 1024, 512
        assert lib.uavsal_conv3_wgrad_shares(C.byref(d)) == shares == len(spans), shape
        assert lib.uavsal_conv3_wgrad_workspace_bytes(C.byref(d)) == shares * 1024 * 9 * 512 * 4
        assert spans[0][0] == 0 and spans[-1][1] == T * H * W and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        assert all(p1 - p0 == cps * R.WGRAD_CHAIN for p0, p1 in spans[:-1])
        if shape in table:
            assert (cps, shares, spans[-1][1] - spans[-1][0]) == table[shape], shape


def test_python_entry_points_refuse_what_they_do_not_cover():
    from iip_uavsal_saliency_amd import UAVSal, UAVSAL_LSTM
    x = torch.zeros(4, 3, 72, 104)
    y = torch.zeros(4, 2, 9, 13)
    with pytest.raises(RuntimeError, match="lstm=True is for a UAVSAL_LSTM"):
        train.recurrence_step(UAVSal(time_dims=4).eval(), x, None, None, y, lstm=True)
    m = UAVSAL_LSTM(time_dims=4).eval()
    with pytest.raises(RuntimeError, match="UAVSAL_LSTM"):                   # without the keyword: as it always was
        train.recurrence_step(m, x, None, None, y)
    with pytest.raises(RuntimeError, match="cuda"):                          # with it: the next refusal is the CPU tensors'
        train.recurrence_step(m, x, None, None, y, lstm=True)
    with pytest.raises(RuntimeError, match="model.eval"):
        train.recurrence_step(UAVSAL_LSTM(time_dims=4).train(), x, None, None, y, lstm=True)
    with pytest.raises(RuntimeError, match="fust=True needs"):               # the stage rules are unchanged behind the keyword
        train.recurrence_step(m, x, None, None, y, lstm=True, fust=True)
    t = torch.zeros(1, 256, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        train.lstm_backward(t, t, None, None, torch.zeros(1024, 512, 3, 3), t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        train.lstm_scan(torch.zeros(1, 4, 4, 1024))
    with pytest.raises(RuntimeError):
        train.lstm_gate_bwd(t.permute(0, 2, 3, 1), None, None, torch.zeros(1, 4, 4, 1024), t, t)


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_the_walk_is_autograd():
    """lstm_ref64.lstm_walk -- the walk train.lstm_backward launches -- against torch autograd through the plain cell, in float64,
    at a width small enough for the CPU: every formula, the gate order, the carries, the pairing of frames."""
    C0, R.C = R.C, 8
    try:
        torch.manual_seed(0)
        T, H, W = 4, 5, 7
        dd = torch.float64
        x, G = torch.randn(T, 8, H, W, dtype=dd), torch.randn(T, 8, H, W, dtype=dd)
        h0, c0 = torch.randn(1, 8, H, W, dtype=dd), torch.randn(1, 8, H, W, dtype=dd)
        w = 0.3 * torch.randn(32, 16, 3, 3, dtype=dd)
        hist, cs, cc = R.lstm_forward(x, h0, c0, w)
        want = R.lstm_bptt(x, h0, c0, w, G)
        got = R.lstm_walk(x, hist, h0, c0, w, G)
        assert float((got["c_seq"] - cs).abs().max()) <= 1e-14 and float((got["cc"] - cc).abs().max()) <= 1e-13
        for k, v in zip(("dW", "grad_x", "grad_h0", "grad_c0"), want):
            assert float((got[k] - v).abs().max()) <= 1e-13 * max(1.0, float(v.abs().max())), k
        for k in R.WRONG:
            if k == "last_share":
                continue                                                      # one share at 140 pixels: nothing to drop
            bad = R.lstm_walk(x, hist, h0, c0, w, G, k, bounds=False)
            assert float((bad["dW"] - want[0]).abs().max()) > 1e-3 * float(want[0].abs().max()), k
    finally:
        R.C = C0


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.name)
def test_seeded_preactivations_hold_saturated_gates_but_not_mostly(shape):
    cc = R.teacher_inputs(shape)["cc"]
    share = float((np.abs(cc) > 8).mean())
    print("%s: share of |cc| > 8: %.3f" % (R.name(shape), share))
    assert 0.01 <= share <= 0.20
    t = R.teacher_inputs(shape)
    assert (float(np.abs(t["c0"]).max()) > 0) == (shape in R.STATE_NONZERO)
    i = R.lstm_inputs(shape)
    assert (float(np.abs(i["h0"]).max()) > 0) == (float(np.abs(i["c0"]).max()) > 0) == (shape in R.STATE_NONZERO)
    assert any(s in R.STATE_NONZERO for s in R.SHAPES) and any(s not in R.STATE_NONZERO for s in R.SHAPES)


def test_saturated_inputs_and_their_relative_bound():
    s = R.to64(R.saturated_inputs())
    assert 10 <= float(s["cc"].abs().min()) and float(s["cc"].abs().max()) <= 30
    r = R.gate_ref(s["G"], None, None, s["cc"], s["c"], s["c_prev"])
    for k, (y, E) in r.items():
        assert bool((R.EPS * E <= R.GATE_REL_MAX * R.U * y.abs() * (1 + 1e-12)).all()), k      # relative to the float64 value
        live = float((y.abs() * R.U > R.SAT_FLOOR).double().mean())
        print("saturated %s: |y| from %.1e to %.1e, %.0f %% above the underflow floor" % (k, float(y.abs().min()), float(y.abs().max()), 100 * live))
        assert live > 0.9, k


def _teacher_walk_inputs(shape):
    """the teacher-forced inputs of the walk: x and the state of lstm_inputs, the history and G of teacher_inputs"""
    i, t = R.to64(R.lstm_inputs(shape)), R.to64(R.teacher_inputs(shape))
    return i["x"], t["hist"], i["h0"], i["c0"], i["w"], t["G"]


ELEMENTWISE_WRONG = ("carry_c_dropped", "c_t_in_dcc_f", "gate_order_ifgo")


@pytest.mark.parametrize("shape", [(3, 5, 7), (1, 9, 16)], ids=R.name)
def test_wrong_gate_kernels_lie_outside_the_bound(shape):
    """uavsal_lstm_gate_bwd's GPU test rejects the kernel against three wrong kernels by the bound it passes: each must be at
    least 4 bounds away on some element, from float64 alone, on the GPU test's inputs (frame 0)."""
    t = R.to64(R.teacher_inputs(shape))
    cs, _ = R.scan_ref(t["cc"], t["c0"])
    args = (t["G"][:1], t["carry_h"], t["carry_c"], t["cc"][:1], cs[:1], t["c0"])
    right = R.gate_ref(*args)
    for k in ELEMENTWISE_WRONG:
        bad = R.gate_ref(*args, variant=k)
        ratio = max(float(((bad[n][0] - right[n][0]).abs() / (R.EPS * right[n][1]).clamp_min(1e-300)).max()) for n in right)
        print("%s %s: up to %.1e bounds from the right kernel" % (R.name(shape), k, ratio))
        assert ratio >= 4.0, k


def test_wrong_scan_lies_outside_the_bound():
    shape = (1, 9, 16)                                                        # T = 1: c0 feeds step 0 directly
    t = R.to64(R.teacher_inputs(shape))
    right, bound = R.scan_ref(t["cc"], t["c0"])
    bad, _ = R.scan_ref(t["cc"], torch.zeros_like(t["c0"]))                   # step0_zero_c
    assert float(((bad - right).abs() / bound.clamp_min(1e-300)).max()) >= 4.0
    z = R.split(t["cc"], "ifgo")                                              # gate_order_ifgo
    bad = torch.sigmoid(z["f"]) * t["c0"] + torch.sigmoid(z["i"]) * torch.tanh(z["g"])
    assert float(((bad - right).abs() / bound.clamp_min(1e-300)).max()) >= 4.0


@pytest.mark.parametrize("shape", [(5, 12, 20), (2, 45, 80)], ids=R.name)
def test_wrong_weight_gradients_lie_outside_the_bound(shape):
    """The two wrong pairings of the weight gradient, at the two shapes whose K split is real, over 16 of the 1024 rows."""
    assert R.wgrad_partition(*shape)[1] > 1
    i, t = R.to64(R.lstm_inputs(shape)), R.to64(R.teacher_inputs(shape))
    dcc = t["dcc"][:, ::64]
    right, bound = R.wgrad_ref(dcc, i["x"], t["hist"], i["h0"])
    for k in ("h_t_not_prev", "last_share"):
        bad, _ = R.wgrad_ref(dcc, i["x"], t["hist"], i["h0"], k)
        ratio = float(((bad - right).abs() / bound.clamp_min(1e-300)).max())
        print("%s %s: up to %.1f bounds from the right sum" % (R.name(shape), k, ratio))
        assert ratio >= 4.0, k


def test_wrong_walks_lie_outside_the_final_bounds():
    """Every entry of WRONG moves the walk's dW by at least 4 of its bounds at (5,12,20) -- T = 5, a non-zero state, two K
    shares -- on the inputs the GPU test feeds `train.lstm_backward`."""
    shape = (5, 12, 20)
    args = _teacher_walk_inputs(shape)
    right = R.lstm_walk(*args)
    b = right["bounds"]["dW"]
    for k in R.WRONG:
        bad = R.lstm_walk(*args, variant=k, bounds=False)
        ratio = float(((bad["dW"] - right["dW"]).abs() / b.clamp_min(1e-300)).max())
        print("%s %s: dW up to %.1f bounds from the right walk" % (R.name(shape), k, ratio))
        assert ratio >= 4.0, k


# ------------------------------------------------------------------------------------------------ the reference's goldens
@pytest.mark.parametrize("shape", R.GOLDEN_SHAPES, ids=R.name)
def test_restatement_against_the_reference(shape):
    """lstm_ref64's autograd and its walk against the reference's own ConvLSTM under autograd (float64, recorded)."""
    path = os.path.join(GOLDEN, R.name(shape) + ".npz")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(GOLDEN, "train_T5_12x20.npz"))
    g = np.load(path)
    inp = R.lstm_inputs(shape)
    assert str(g["digest"]) == R.digest(*(inp[k] for k in ("x", "h0", "c0", "w", "G")))
    i = R.to64(inp)
    hist, cs, _ = R.lstm_forward(i["x"], i["h0"], i["c0"], i["w"])
    assert float((hist[:, ::64] - torch.as_tensor(g["h_seq"])).abs().max()) <= 1e-12
    walk = R.lstm_walk(i["x"], hist, i["h0"], i["c0"], i["w"], i["G"])
    auto = dict(zip(("dW", "grad_x", "grad_h0", "grad_c0"), R.lstm_bptt(i["x"], i["h0"], i["c0"], i["w"], i["G"])))
    for src in (walk, auto):
        for k, sub in (("dW", R.DW_SUBSET), ("grad_x", (slice(None), slice(None, None, 16))),
                       ("grad_h0", (slice(None), slice(None, None, 8))), ("grad_c0", (slice(None), slice(None, None, 8)))):
            assert float((src[k][sub] - torch.as_tensor(g[k])).abs().max()) <= 1e-11 * float(g["max_" + k]), k
        assert abs(float(src["dW"].sum()) - float(g["dW_sum"])) <= 1e-9 * float(g["dW_l2"])
        assert abs(float(src["dW"].norm()) - float(g["dW_l2"])) <= 1e-11 * float(g["dW_l2"])
    for k in ("dW", "grad_x", "grad_h0", "grad_c0"):
        assert 0 < float(g["gap_" + k]) < 1e-4 * float(g["max_" + k]), k
