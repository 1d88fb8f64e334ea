"""The trainable slice without a GPU: the C ABI of csrc/train.hip, the float64 restatement (tests/train_ref64.py) against the
reference's recorded autograd results (tests/golden/train_*.npz), the driver's group logic, argument errors, and the
conditions under which two GPU tests are meaningful, asserted on the float64 reference alone: the decoder's end-to-end test,
and the weight gradient's wrong references at the shapes with a real K split (train_ref64.WGRAD_SPLIT_SHAPES).  The K split
itself is held to train_ref64.wgrad_partition: the exact share count of every tested shape and of the two real calls,
(20,45,80) and (80,45,80)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import _lib, stream, train

import train_ref64 as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def lib():
    from iip_uavsal_saliency_amd import build
    build.build()
    return _lib.load()


def test_symbols_sizes_and_abi(lib):
    names = [s[0] for s in _lib.SYMBOLS]
    for n in ("uavsal_twa_gate_bwd", "uavsal_twa_wgrad", "uavsal_twa_wgrad_workspace_bytes", "uavsal_twa_wgrad_shares",
              "uavsal_dec_bwd", "uavsal_train_sizeof_desc"):
        assert n in names and hasattr(lib, n)
    for i, t in enumerate(_lib.TRAIN_DESC_TYPES):
        assert lib.uavsal_train_sizeof_desc(i) == C.sizeof(t)
    assert lib.uavsal_train_sizeof_desc(3) < 0
    assert lib.uavsal_abi_version() == 20 and len(_lib.DESC_TYPES) == 20 and lib.uavsal_sizeof_desc(20) < 0


def test_wgrad_split_keeps_every_chain_short(lib):
    """Shares are whole chunks of 1024 pixels, the workspace is one partial [256][9][512] tile set per share."""
    for T, H, W in R.SHAPES + [(20, 45, 80), (5, 45, 80), (64, 90, 160)]:
        d = _lib.TwaWgradDesc()
        d.T, d.H, d.W, d.C = T, H, W, 256
        shares = lib.uavsal_twa_wgrad_shares(C.byref(d))
        chunks = math.ceil(T * H * W / _lib.WGRAD_CHAIN)
        assert 1 <= shares <= min(chunks, 14)
        assert lib.uavsal_twa_wgrad_workspace_bytes(C.byref(d)) == shares * 256 * 9 * 512 * 4
    d.T, d.H, d.W = 20, 45, 80
    assert lib.uavsal_twa_wgrad_shares(C.byref(d)) == 12                  # 71 chunks, 6 per share


def test_wgrad_share_count_is_the_restated_partition(lib):
    """`uavsal_twa_wgrad_shares` against train_ref64.wgrad_partition, and the restated shares tile [0, K)."""
    table = {(20, 27, 27): (2, 8, 244), (9, 45, 80): (3, 11, 1680), (5, 45, 80): (2, 9, 1616),       # (cps, shares, last share)
             (20, 45, 80): (6, 12, 4416), (80, 45, 80): (21, 14, 8448)}
    for shape in R.SHAPES + R.WGRAD_SPLIT_SHAPES + [(5, 45, 80), (20, 45, 80), (80, 45, 80)]:
        T, H, W = shape
        K = T * H * W
        cps, shares, spans = R.wgrad_partition(T, H, W)
        d = _lib.TwaWgradDesc()
        d.T, d.H, d.W, d.C = T, H, W, 256
        assert lib.uavsal_twa_wgrad_shares(C.byref(d)) == shares == len(spans), shape
        assert lib.uavsal_twa_wgrad_workspace_bytes(C.byref(d)) == shares * 256 * 9 * 512 * 4
        assert spans[0][0] == 0 and spans[-1][1] == K
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))             # no gap, no overlap
        assert all(p1 - p0 == cps * _lib.WGRAD_CHAIN for p0, p1 in spans[:-1])
        assert 0 < spans[-1][1] - spans[-1][0] <= cps * _lib.WGRAD_CHAIN
        if shape in R.SHAPES:
            assert cps == 1                                                    # why WGRAD_SPLIT_SHAPES exist
        if shape in table:
            assert (cps, shares, spans[-1][1] - spans[-1][0]) == table[shape], shape
    assert R.WGRAD_CHAIN == _lib.WGRAD_CHAIN


@pytest.mark.parametrize("shape", R.WGRAD_SPLIT_SHAPES, ids=R.name)
def test_wgrad_wrong_references_lie_outside_the_bound(shape):
    """The GPU test rejects the kernel's result against four wrong references by the bound it passes against the right one.
    That says something only if each wrong reference lies well outside the bound: at least 4 bounds from the right one on
    some element, so that the kernel's own error of at most 1 bound cannot bring it back inside.  From the float64 reference
    alone, on the GPU test's inputs, over 16 of the 256 output channels (the GPU test takes the maximum over all)."""
    T, H, W = shape
    w = R.wgrad_wrong_weights(T, H, W)
    cps, shares, spans = R.wgrad_partition(T, H, W)
    gone = lambda k: int((w[k] == 0).sum())                                   # noqa: E731
    assert gone("last_share") == spans[-1][1] - spans[-1][0] and 0 < gone("tail_step") < R.WGRAD_KSTEP
    assert int((w["chain_twice"] == 2).sum()) == R.WGRAD_CHAIN * sum(b - a > R.WGRAD_CHAIN for a, b in spans) > 0
    i64 = R.to64(R.wgrad_inputs(shape))
    assert float(i64["h0"].abs().max()) > 0
    dz = i64["dz"][:, ::16]
    right, bound = R.wgrad_ref(dz, i64["x"], i64["hist"], i64["h0"])
    wrong = R.wgrad_wrong_refs(dz, i64["x"], i64["hist"], i64["h0"])
    assert sorted(wrong) == sorted(R.WGRAD_WRONG)
    for k in R.WGRAD_WRONG:
        ratio = float(((wrong[k] - right).abs() / bound).max())
        print("%s %s: the wrong reference is up to %.1f bounds from the right one" % (R.name(shape), k, ratio))
        assert ratio >= 4.0, k


def test_argument_validation_without_gpu(lib):
    w = _lib.TwaWgradDesc()
    assert lib.uavsal_twa_wgrad(C.byref(w), None) == -1
    w.dz = w.x = w.h = w.h0 = w.ws = w.out = 256
    w.T, w.H, w.W, w.C, w.ldx, w.ldh, w.ldh0 = 2, 4, 4, 128, 128, 128, 128
    assert lib.uavsal_twa_wgrad(C.byref(w), None) == -3                   # C = 256 only
    w.C = w.ldx = w.ldh = w.ldh0 = 256
    assert lib.uavsal_twa_wgrad(C.byref(w), None) == -1                   # workspace too small
    w.ws_bytes = lib.uavsal_twa_wgrad_workspace_bytes(C.byref(w))
    w.ldx = 258
    assert lib.uavsal_twa_wgrad(C.byref(w), None) == -2
    g = _lib.TwaGateDesc()
    assert lib.uavsal_twa_gate_bwd(C.byref(g), None) == -1
    g.g = g.z = g.x = g.hprev = g.dz = g.carry_out = 256
    g.n_pix, g.C, g.ldg, g.ldx, g.ldh = 4, 64, 64, 64, 64
    assert lib.uavsal_twa_gate_bwd(C.byref(g), None) == -3
    g.C = g.ldg = g.ldx = g.ldh = 256
    g.dz = 260
    assert lib.uavsal_twa_gate_bwd(C.byref(g), None) == -2
    b = _lib.DecBwdDesc()
    assert lib.uavsal_dec_bwd(C.byref(b), None) == -1
    b.gy = b.y = b.e = b.d = b.s1 = b.wd9 = b.s2 = b.w3 = b.s3 = b.ge = 256
    b.n_img, b.H, b.W, b.C = 1, 4, 4, 6
    assert lib.uavsal_dec_bwd(C.byref(b), None) == -2


def test_python_entry_points_refuse_what_they_do_not_cover():
    from iip_uavsal_saliency_amd import UAVSal, UAVSAL_LSTM
    x = torch.zeros(4, 3, 72, 104)
    y = torch.zeros(4, 2, 9, 13)
    m = UAVSal(time_dims=4)
    with pytest.raises(RuntimeError, match="eval"):
        train.recurrence_step(m.train(), x, None, None, y)
    m.eval()
    with pytest.raises(RuntimeError, match="cuda"):
        train.recurrence_step(m, x, None, None, y)
    m.precision = "f16x3"
    with pytest.raises(RuntimeError, match="f32"):
        train.recurrence_step(m, x, None, None, y)
    with pytest.raises(RuntimeError, match="UAVSAL_LSTM"):
        train.recurrence_step(UAVSAL_LSTM(time_dims=4).eval(), x, None, None, y)
    t = torch.zeros(2, 256, 4, 4)
    with pytest.raises(RuntimeError, match="cuda"):
        train.twa_backward(t, t, None, torch.zeros(256, 512, 3, 3), t)
    with pytest.raises(RuntimeError, match="cuda"):
        train.decoder_input_grad(m.conv_out_st, t, torch.zeros(2, 1, 4, 4))
    with pytest.raises(RuntimeError, match="conv_out_st"):
        train.decoder_input_grad(m.fust_layer[0], t, torch.zeros(2, 1, 4, 4))
    assert m.refresh_weights(m.rnn) == 0 and m._wversion is None           # nothing packed yet: nothing to do


# ------------------------------------------------------------------------------------------------ restatement vs goldens
@pytest.mark.parametrize("shape", R.GOLDEN_SHAPES, ids=R.name)
def test_restatement_matches_the_reference_autograd(shape):
    g = np.load(os.path.join(GOLDEN, R.name(shape) + ".npz"))
    inp = R.twa_inputs(shape)
    assert str(g["digest"]) == R.digest(inp["x"], inp["h0"], inp["w"], inp["gy"]) and int(g["seed"]) == R.SEED[shape]
    i64 = R.to64(inp)
    h_seq, _ = R.twa_forward(i64["x"], i64["h0"], i64["w"])
    p = R.decoder_params(h_seq.numpy(), R.SEED[shape] + 7)
    for k in ("s1", "b1", "s2", "b2", "s3", "b3"):                          # the fold depends on the history: the recorded one
        np.testing.assert_allclose(p[k], g[k], rtol=1e-5, atol=1e-6)
        p[k] = g[k]
    grad_h = R.decoder_grad_autograd(R.to64(p), h_seq, i64["gy"])
    # the explicit formula of the kernel is the autograd gradient
    f = R.decoder_forward(R.to64(p), h_seq)
    ge = R.dec_bwd_ref(R.to64(p), i64["gy"], f["y"], f["e"], f["d"])
    explicit = torch.nn.functional.conv_transpose2d(ge, R.to64(p)["w1"])
    assert float((explicit - grad_h).abs().max()) <= 1e-12 * float(grad_h.abs().max())
    gw, gx, g0 = R.twa_bptt(i64["x"], i64["h0"], i64["w"], grad_h)

    def close(a, b):
        assert float(np.abs(a - b).max()) <= 1e-10 * float(np.abs(b).max())
    close(grad_h.numpy()[:, ::16], g["grad_h"])
    close(gx.numpy()[:, ::16], g["grad_x"])
    close(g0.numpy()[:, ::8], g["grad_h0"])
    close(gw.numpy()[R.DW_SUBSET], g["dW"])
    assert abs(float(gw.sum()) - float(g["dW_sum"])) <= 1e-10 * float(g["dW_l2"]) * math.sqrt(gw.numel())
    assert abs(float(gw.norm()) - float(g["dW_l2"])) <= 1e-10 * float(g["dW_l2"])
    # the manual BPTT of train.twa_backward, restated: gate_ref + the two transposed convs + wgrad_ref
    T = shape[0]
    x, h0, w = i64["x"], i64["h0"], i64["w"]
    _, z = R.twa_forward(x, h0, w)
    hprev = torch.cat([h0, h_seq[:T - 1]], 0)
    carry, dzs, dxs = None, [None] * T, [None] * T
    for t in range(T - 1, -1, -1):
        r = R.gate_ref(grad_h[t:t + 1], carry, z[t:t + 1], x[t:t + 1], hprev[t:t + 1])
        dzs[t], dxs[t] = r["dz"][0], r["dx"][0]
        carry = R.input_grad_ref(dzs[t], w[:, 256:], r["carry"][0])[0]
    dz = torch.cat(dzs, 0)
    close(carry.numpy(), g0.numpy())
    close(R.input_grad_ref(dz, w[:, :256], torch.cat(dxs, 0))[0].numpy(), gx.numpy())
    close(R.wgrad_ref(dz, x, h_seq, h0)[0].numpy(), gw.numpy())


# ------------------------------------------------------------------------------------------------ the decoder's condition
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.name)
def test_decoder_inputs_hit_both_clamps_and_leave_few_masks_undecided(shape):
    """With the decoder recipe of the tests, both clamps of both ReLU6s hold at least 5 % of the elements, and the part of the
    gradient that hangs on masks the device may legitimately decide the other way is at most 6 % of ||grad_h||_2 per frame:
    the widened bound of the end-to-end GPU test cannot hide a structural error, which is of order 1."""
    h, p, gy = R.decoder_inputs(shape)
    h, p, gy = torch.as_tensor(h).double(), R.to64(p), torch.as_tensor(gy).double()
    grad_h, bound, und, f = R.decoder_e2e(p, h, gy)
    for pre in (f["e_pre"], f["d_pre"]):
        lo, hi = R.clamp_shares(pre)
        assert lo >= 0.05 and hi >= 0.05, (lo, hi)
    ratio = R.l2_per_frame(und) / R.l2_per_frame(grad_h)
    reg = R.l2_per_frame(bound) / R.l2_per_frame(grad_h)
    print("%s: undecided e %.1e d %.1e of the elements; undecided / ||grad_h|| per frame %s, regular bound %s" % (
        R.name(shape), float(f["ue"].mean()), float(f["ud"].mean()),
        ["%.3f" % v for v in ratio.tolist()], ["%.1e" % v for v in reg.tolist()]))
    assert float(ratio.max()) <= 0.06
    assert float((grad_h - R.decoder_grad_autograd(p, h, gy)).abs().max()) <= 1e-12 * float(grad_h.abs().max())


# ------------------------------------------------------------------------------------------------ the driver
class _Rnn(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


class _StubModel:
    time_dims = 5

    def __init__(self):
        self.rnn, self.refreshed = _Rnn(), []

    def parameters(self):
        return iter(self.rnn.parameters())

    def refresh_weights(self, *mods):
        self.refreshed.append(mods)


class _StubOpt:
    def __init__(self):
        self.log = []

    def zero_grad(self):
        self.log.append("zero")

    def step(self):
        self.log.append("step")


def test_finetune_video_walks_the_groups_of_validate_video(monkeypatch):
    n = 43
    frames = torch.zeros(n, 3, 72, 128, dtype=torch.uint8)
    frames[:, 0, 0, 0] = torch.arange(n, dtype=torch.uint8)
    has = torch.ones(n, 2, dtype=torch.bool)
    has[12, 1] = False
    seen_groups = []
    real = stream.validation_groups

    def groups(*a):
        seen_groups.append(a[:3])
        return real(*a)
    monkeypatch.setattr(stream, "validation_groups", groups)
    calls = []

    def step(model, x, cb, state, y, criterion):
        seen = 0.0 if state is None else float(state[0])
        assert cb[0].shape[0] == x.shape[0] == y.shape[0] and criterion is crit
        calls.append((int(x[0, 0, 0, 0]), x.shape[0], seen))
        return torch.tensor(float(x[0, 0, 0, 0]) + 0.5), None, [torch.tensor(seen + 1.0)]
    monkeypatch.setattr(train, "recurrence_step", step)
    crit = object()
    m, opt = _StubModel(), _StubOpt()
    fix = torch.zeros(n, 4, 4, dtype=torch.uint8)
    r = stream.finetune_video(m, frames, torch.zeros(8, 9, 16), torch.zeros(20, 9, 16), fix, fix, opt, batch_size=2,
                              criterion=crit, prepare=lambda a, b, h, w, l: (torch.zeros(n, 2, h, w), has))
    assert seen_groups == [(43, 5, 2)]
    assert calls == [(0, 10, 0.0), (20, 10, 1.0), (30, 10, 2.0)]           # the second group is skipped before its forward
    assert opt.log == ["zero", "step"] * 3 and m.refreshed == [(m.rnn,)] * 3
    got = r["losses"].tolist()
    assert [math.isnan(v) for v in got] == [False, True, False, False] and got[0] == 0.5 and got[2] == 20.5
    assert sorted(r) == sorted(["losses", "groups_run", "video_mean", "run_loss", "num_step"])
    assert r["groups_run"] == 3 and r["video_mean"] == (0.5 + 20.5 + 30.5) / 4
