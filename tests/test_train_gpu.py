"""The trainable slice on the GPU (train.py, csrc/train.hip) against the float64 restatement tests/train_ref64.py, which
runs on the device in torch float64, and the reference's recorded autograd results (tests/golden/train_*.npz).
Shapes (T, H, W): (3,5,7) 35 pixels, below one tile and odd; (1,9,16) one step, no carry; (5,12,20) a non-zero h0;
(2,45,80) the real map: 3600 rows are no multiple of 128, K is split into several shares and over both frames.
In all four a workgroup of the weight gradient owns ONE chunk of 1024 pixels (cps = 1).  The weight gradient alone also runs
at train_ref64.WGRAD_SPLIT_SHAPES: (20,27,27), cps = 2, 8 shares -- a chain ends in the middle of a share, the second
register tile matters, the last share is 244 pixels, frames straddle every K step and chunk border, h0 and 19 history
frames --, and (9,45,80), cps = 3, 11 shares -- the last share owns fewer chunks than the others and ends in a partial chain
with a half-filled K step.  There the kernel's result must also be REJECTED, by the bound it passes, against four wrong
references (train_ref64.wgrad_wrong_refs; the CPU test holds each at least 4 bounds away).  The step from a carried state
runs at 360x640 with five frames: the 45x80 map, cps = 2, 9 shares, the last one 1024 + 592 pixels.
Bounds: train_ref64's docstring.  Teacher-forced tests hand every kernel the float64 reference's inputs rounded to fp32."""
import math
import os
from functools import lru_cache

import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import _lib as L
from iip_uavsal_saliency_amd import losses, ops, synth, train
from iip_uavsal_saliency_amd import packing as P
from iip_uavsal_saliency_amd.weights import WeightCache

import train_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPE_IDS = [R.name(s) for s in R.SHAPES]


def _dev(a):
    return torch.as_tensor(a).to(DEV)


def _cl(a):
    """float32 [n,c,h,w] on the device, channels-last (what the kernels read in place)"""
    return _dev(a).float().contiguous(memory_format=torch.channels_last)


def _nhwc(a):
    return _cl(a).permute(0, 2, 3, 1)


def _nchw64(t_nhwc):
    return t_nhwc.permute(0, 3, 1, 2).double()


def _check(got, want, bound, what):
    err = (got.double() - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print("%s: worst error / bound %.4f (max |err| %.3e, max |ref| %.3e)" % (what, worst, float(err.max()), float(want.abs().max())))
    assert torch.isfinite(got).all() and bool((err <= bound).all()), what


@lru_cache(maxsize=None)
def _teacher(shape):
    t = {k: _dev(v) for k, v in R.teacher_inputs(shape).items()}
    inp = R.twa_inputs(shape)
    t["x"], t["w"] = _dev(inp["x"]), _dev(inp["w"])
    t["h0"] = 100.0 * t["carry"] if shape in R.H0_NONZERO else torch.zeros_like(t["carry"])
    return t


@lru_cache(maxsize=None)
def _wgrad_ref(shape):
    t = _teacher(shape)
    return R.wgrad_ref(t["dz"].double(), t["x"].double(), t["hist"].double(), t["h0"].double())


def _wgrad(shape, **kw):
    t = _teacher(shape)
    return train.twa_wgrad(_nhwc(t["dz"]).contiguous(), _nhwc(t["x"]), _nhwc(t["hist"]), _nhwc(t["h0"]), **kw)


# ------------------------------------------------------------------------------------------------ 1. teacher-forced kernels
@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("with_carry", [True, False], ids=["carry", "no carry"])
def test_gate_kernel(shape, with_carry):
    t = _teacher(shape)
    G, z, x, hp = t["G"], t["z"], t["x"], t["hist"]
    carry = t["dz"] if with_carry else None
    dz, co, dx = train.twa_gate_bwd(_nhwc(G), _nhwc(carry).contiguous() if with_carry else None, _nhwc(z).contiguous(), _nhwc(x),
                                    _nhwc(hp), need_dx=True)
    ref = R.gate_ref(G.double(), carry.double() if with_carry else None, z.double(), x.double(), hp.double())
    for name, got in (("dz", dz), ("carry", co), ("dx", dx)):
        y, E = ref[name]
        _check(_nchw64(got), y, R.EPS * E, "gate %s %s" % (name, R.name(shape)))


@pytest.mark.parametrize("shape", R.SHAPES + R.WGRAD_SPLIT_SHAPES, ids=R.name)
def test_wgrad_kernel(shape):
    want, bound = _wgrad_ref(shape)
    _check(_wgrad(shape), want, bound, "wgrad " + R.name(shape))


@pytest.mark.parametrize("shape", R.WGRAD_SPLIT_SHAPES, ids=R.name)
def test_wgrad_kernel_is_rejected_against_wrong_partitions(shape):
    """The bound that accepts the kernel against the right reference rejects it against each wrong one: a last share left
    out, a chain counted twice, the final partial K step left out, frame 0 paired with zeros instead of h0."""
    t = _teacher(shape)
    inp = R.wgrad_inputs(shape)
    assert all(torch.equal(t[k].cpu(), torch.as_tensor(inp[k])) for k in ("dz", "x", "hist", "h0"))      # the CPU test's inputs
    want, bound = _wgrad_ref(shape)
    got = _wgrad(shape).double()
    assert bool(((got - want).abs() <= bound).all())
    wrong = R.wgrad_wrong_refs(t["dz"].double(), t["x"].double(), t["hist"].double(), t["h0"].double())
    assert sorted(wrong) == sorted(R.WGRAD_WRONG)
    for k in R.WGRAD_WRONG:
        ratio = float(((got - wrong[k]).abs() / bound.clamp_min(1e-300)).max())
        print("wgrad %s against %s: worst error / bound %.1f" % (R.name(shape), k, ratio))
        assert ratio > 1.0, k


@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_input_gradient_convs(shape):
    """carry = carry' + conv3x3(flip(W_h)^T, dz_t) and dx += conv3x3(flip(W_x)^T, dz_all) as train.twa_backward launches them"""
    t = _teacher(shape)
    lib = L.load()
    cache, mod = WeightCache(torch.device(DEV), {}), type("W", (), {"weight": t["w"]})()
    dz, res = t["dz"], t["G"]
    for half, sl in (("W_h", (256, 512)), ("W_x", (0, 256))):
        got = train._conv(lib, cache, _nhwc(dz).contiguous(), mod, 256, 9, wslice=sl, transposed=True, res=_nhwc(res).contiguous())
        want, bound = R.input_grad_ref(dz.double(), t["w"].double()[:, sl[0]:sl[1]], res.double())
        _check(_nchw64(got), want, bound, "input gradient %s %s" % (half, R.name(shape)))


@lru_cache(maxsize=None)
def _decoder(shape):
    """the decoder block on the device with the test's parameters, its folded values in float64, and the float64 forward"""
    from iip_uavsal_saliency_amd.model import dwBlock
    h, p, gy = R.decoder_inputs(shape)
    block = R.load_block(dwBlock(256, 1, kernel_size=3), p).to(DEV)
    seq = block.conv
    for bn, s, b in ((seq[0][1], "s1", "b1"), (seq[1][1], "s2", "b2"), (seq[3], "s3", "b3")):
        fs, fb = P.fold_bn(bn)
        assert np.array_equal(fs.numpy(), p[s]) and np.array_equal(fb.numpy(), p[b])          # the fold is exact
    p64 = R.to64(p, DEV)
    h64, gy64 = _dev(h).double(), _dev(gy).double()
    return block, p64, h64, gy64, R.decoder_forward(p64, h64)


@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_dec_bwd_kernel(shape):
    """e, d and y are given (the float64 forward rounded to fp32): both sides evaluate the masks on identical numbers"""
    block, p, h, gy, f = _decoder(shape)
    for pre in (f["e_pre"], f["d_pre"]):
        lo, hi = R.clamp_shares(pre)
        assert lo >= 0.05 and hi >= 0.05, (lo, hi)
    e, d, y = f["e"].float(), f["d"].float(), f["y"].float()
    up = lambda k: p[k].float().reshape(-1).contiguous()                       # noqa: E731
    wd9 = P.pack_dw_weight(p["wd"].float().cpu()).to(DEV)
    ge = train.dec_bwd(gy.float(), y.contiguous(), _nhwc(e).contiguous(), _nhwc(d).contiguous(), up("s1"), wd9, up("s2"), up("w3"), up("s3"))
    want = R.dec_bwd_ref(p, gy, y.double(), e.double(), d.double())
    assert float((want != 0).double().mean()) > 0.3
    _check(_nchw64(ge), want, R.dec_bwd_bound(p, gy, y.double(), e.double(), d.double()), "dec_bwd " + R.name(shape))


# ------------------------------------------------------------------------------------------------ 2. weight gradient details
def test_wgrad_border_taps():
    """dz is non-zero only in the four corner pixels of every frame: every tap that would read across a border reads zero,
    and no frame reads its neighbour"""
    shape = (5, 12, 20)
    t = _teacher(shape)
    dz = torch.zeros_like(t["dz"])
    for yy in (0, -1):
        for xx in (0, -1):
            dz[:, :, yy, xx] = 100.0 * t["dz"][:, :, yy, xx]
    got = train.twa_wgrad(_nhwc(dz).contiguous(), _nhwc(t["x"]), _nhwc(t["hist"]), _nhwc(t["h0"]))
    want, bound = R.wgrad_ref(dz.double(), t["x"].double(), t["hist"].double(), t["h0"].double())
    assert float(want.abs().max()) > 0
    _check(got, want, bound, "wgrad corners")


def test_wgrad_two_calls_equal_bits_with_two_chains_per_share():
    first, again = _wgrad((20, 27, 27)), _wgrad((20, 27, 27))
    assert torch.equal(first.view(torch.int32), again.view(torch.int32))


def test_wgrad_reads_channel_slices_in_place():
    """x, h and h0 as the channels 32..287 of 320-channel channels-last buffers (ldx = ldh = ldh0 = 320) whose other channels
    hold a large constant: the same bits as from dense operands"""
    shape = (3, 5, 7)
    t = _teacher(shape)
    dz = _nhwc(t["dz"]).contiguous()

    def sliced(a):
        big = torch.full((a.shape[0], 320) + tuple(a.shape[2:]), 1.0e6, device=DEV).contiguous(memory_format=torch.channels_last)
        big[:, 32:288] = a
        v = big[:, 32:288].permute(0, 2, 3, 1)
        assert v.stride(2) == 320 and not v.is_contiguous() and torch.equal(v, _nhwc(a))
        return v
    dense = train.twa_wgrad(dz, _nhwc(t["x"]), _nhwc(t["hist"]), _nhwc(t["h0"]))
    assert float(dense.abs().max()) > 0 and float(t["h0"].abs().max()) == 0
    got = train.twa_wgrad(dz, sliced(t["x"]), sliced(t["hist"]), sliced(t["h0"]))
    assert torch.equal(got.view(torch.int32), dense.view(torch.int32))
    # h0 is zeros at this shape: once more with the carry as a non-zero h0
    h0 = 100.0 * t["carry"]
    dense = train.twa_wgrad(dz, _nhwc(t["x"]), _nhwc(t["hist"]), _nhwc(h0))
    got = train.twa_wgrad(dz, sliced(t["x"]), sliced(t["hist"]), sliced(h0))
    assert torch.equal(got.view(torch.int32), dense.view(torch.int32))
    want, bound = R.wgrad_ref(t["dz"].double(), t["x"].double(), t["hist"].double(), h0.double())
    _check(got, want, bound, "wgrad from channel slices, non-zero h0")


@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 45, 80)], ids=R.name)
def test_wgrad_accumulate_and_determinism(shape):
    first = _wgrad(shape)
    again = _wgrad(shape)
    assert torch.equal(first.view(torch.int32), again.view(torch.int32))          # two calls, equal bits
    prev = (0.01 * torch.randn(first.shape, generator=torch.Generator().manual_seed(5))).to(DEV)
    out = prev.clone()
    assert _wgrad(shape, out=out, accumulate=True) is out
    # fl(s + prev) against fl(s) + prev: one rounding of the sum and one of s
    want = first.double() + prev.double()
    _check(out, want, 1.001 * R.U * (want.abs() + first.double().abs()), "wgrad accumulate")
    out2 = prev.clone()
    _wgrad(shape, out=out2)
    assert torch.equal(out2, first)                                                # overwrite ignores the content


def test_zero_gradient_gives_zero():
    shape = (5, 12, 20)
    t = _teacher(shape)
    gw, gx, g0 = train.twa_backward(_cl(t["x"]), _cl(t["hist"]), _cl(t["h0"]), t["w"], torch.zeros_like(_cl(t["G"])), need_x_grad=True)
    for g in (gw, gx, g0):
        assert bool((g.contiguous().view(torch.int32) == 0).all())                 # +0.0 in every element, not -0.0


def test_twa_backward_returns_the_same_bits_twice():
    shape = (5, 12, 20)
    t = _teacher(shape)
    args = (_cl(t["x"]), _cl(t["hist"]), _cl(t["h0"]), t["w"], _cl(t["G"]))
    a = train.twa_backward(*args, need_x_grad=True)
    b = train.twa_backward(*args, need_x_grad=True)
    for u, v in zip(a, b):
        assert torch.equal(u.contiguous().view(torch.int32), v.contiguous().view(torch.int32))


def test_non_contiguous_gradients():
    """grad_h as a channel slice of a wider channels-last buffer, grad_out as a window of a larger map"""
    shape = (3, 5, 7)
    t = _teacher(shape)
    T, H, W = shape
    x, hist, h0, G = _cl(t["x"]), _cl(t["hist"]), _cl(t["h0"]), _cl(t["G"])
    big = torch.zeros((T, 512, H, W), device=DEV).contiguous(memory_format=torch.channels_last)
    big[:, 128:384] = G
    a = train.twa_backward(x, hist, h0, t["w"], G, need_x_grad=True)
    b = train.twa_backward(x, hist, h0, t["w"], big[:, 128:384], need_x_grad=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    block, p, h, gy, f = _decoder(shape)
    wide = torch.zeros((T, 1, H + 3, W + 5), device=DEV)
    wide[:, :, 1:H + 1, 2:W + 2] = gy.float()
    y = f["y"].float()
    g1 = train.decoder_input_grad(block, _cl(h), gy.float(), y=y)
    g2 = train.decoder_input_grad(block, _cl(h), wide[:, :, 1:H + 1, 2:W + 2], y=y)
    assert torch.equal(g1, g2)


# ------------------------------------------------------------------------------------------------ 3. free-running BPTT
@pytest.mark.parametrize("shape", R.GOLDEN_SHAPES, ids=R.name)
def test_twa_backward_against_the_reference(shape, golden_dir):
    """Against the reference's float64 autograd results.  Per tensor in max-abs: twice the reference's own fp32-vs-float64
    gap (a second fp32 implementation sums in another order) plus the bound of the tensor's final sum."""
    g = np.load(os.path.join(golden_dir, R.name(shape) + ".npz"))
    inp = {k: _dev(v) for k, v in R.twa_inputs(shape).items()}
    assert str(g["digest"]) == R.digest(*(inp[k].cpu().numpy() for k in ("x", "h0", "w", "gy")))
    x64, h064, w64 = inp["x"].double(), inp["h0"].double(), inp["w"].double()
    h_seq, z = R.twa_forward(x64, h064, w64)
    p = R.decoder_params(h_seq.cpu().numpy(), R.SEED[shape] + 7)
    p.update({k: g[k] for k in ("s1", "b1", "s2", "b2", "s3", "b3")})
    grad_h = R.decoder_grad_autograd(R.to64(p, DEV), h_seq, inp["gy"].double())
    assert float((grad_h[:, ::16].cpu() - torch.as_tensor(g["grad_h"])).abs().max()) <= 1e-10 * float(np.abs(g["grad_h"]).max())
    gw, gx, g0 = train.twa_backward(_cl(inp["x"]), _cl(h_seq), _cl(inp["h0"]), inp["w"], _cl(grad_h), need_x_grad=True)
    # the bounds of the final sums, from the float64 restatement alone: dz by gate_ref over twa_forward's z
    T = shape[0]
    hprev = torch.cat([h064, h_seq[:T - 1]], 0)
    carry, dzs = None, [None] * T
    for t in range(T - 1, -1, -1):
        r = R.gate_ref(grad_h[t:t + 1], carry, z[t:t + 1], x64[t:t + 1], hprev[t:t + 1])
        dzs[t] = r["dz"][0]
        carry = R.input_grad_ref(dzs[t], w64[:, 256:], r["carry"][0])[0]
    dz = torch.cat(dzs, 0)
    _, wb = R.wgrad_ref(dz, x64, h_seq, h064)
    _, xb = R.input_grad_ref(dz, w64[:, :256], grad_h.abs())
    _, hb = R.input_grad_ref(dz[:1], w64[:, 256:], grad_h[:1].abs())
    for name, got, want, gap, fin in (("dW", gw[R.DW_SUBSET], g["dW"], g["gap_dW"], wb[R.DW_SUBSET]),
                                      ("grad_x", gx[:, ::16], g["grad_x"], g["gap_grad_x"], xb[:, ::16]),
                                      ("grad_h0", g0[:, ::8], g["grad_h0"], g["gap_grad_h0"], hb[:, ::8])):
        err = float((got.double().cpu() - torch.as_tensor(want)).abs().max())
        tol = 2 * float(gap) + float(fin.max())
        print("%s %s: max |err| %.3e = %.2f x the reference's fp32 gap %.3e; tolerance %.3e" % (R.name(shape), name, err, err / float(gap), float(gap), tol))
        assert err <= tol
    assert abs(float(gw.double().sum()) - float(g["dW_sum"])) <= (2 * float(g["gap_dW"]) + float(wb.max())) * math.sqrt(gw.numel())
    assert abs(float(gw.double().norm()) - float(g["dW_l2"])) <= (2 * float(g["gap_dW"]) + float(wb.max())) * math.sqrt(gw.numel())


# ------------------------------------------------------------------------------------------------ 4. decoder end to end
@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_decoder_input_grad_end_to_end(shape):
    """The device recomputes e and d.  A mask within rounding of a clamp may fall the other way, which removes a whole term,
    so the comparison is per frame in L2 against the regular bound plus the undecided term (train_ref64.decoder_e2e); the CPU
    test asserts that term is at most 6 % of ||grad_h||_2 for these inputs, a structural error is of order 1."""
    block, p, h, gy, f = _decoder(shape)
    want, bound, und, _ = R.decoder_e2e(p, h, gy)
    parts = {}
    got = train.decoder_input_grad(block, _cl(h), gy.float(), y=f["y"].float(), parts=parts)
    flips_e = float(((_nchw64(parts["e"]) > 0) & (_nchw64(parts["e"]) < 6)).ne((f["e"] > 0) & (f["e"] < 6)).double().mean())
    flips_d = float(((_nchw64(parts["d"]) > 0) & (_nchw64(parts["d"]) < 6)).ne((f["d"] > 0) & (f["d"] < 6)).double().mean())
    err, lim, ref = R.l2_per_frame(got.double() - want), R.l2_per_frame(bound + und), R.l2_per_frame(want)
    print("%s: masks that fell the other way: e %.1e, d %.1e of the elements; per frame ||err|| / ||grad_h|| %s, limit %s, undecided %s" % (
        R.name(shape), flips_e, flips_d, ["%.2e" % v for v in (err / ref).tolist()], ["%.2e" % v for v in (lim / ref).tolist()],
        ["%.3f" % v for v in (R.l2_per_frame(und) / ref).tolist()]))
    assert float((R.l2_per_frame(und) / ref).max()) <= 0.06
    assert bool((err <= lim).all())
    # y recomputed on the device as well: the same limit plus the effect of y's own forward error is not modelled; it must
    # stay a small multiple
    again = train.decoder_input_grad(block, _cl(h), gy.float())
    assert bool((R.l2_per_frame(again.double() - want) <= 0.06 * ref).all())


# ------------------------------------------------------------------------------------------------ 5. the step and the driver
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


def _model():
    from iip_uavsal_saliency_amd import UAVSal
    m = UAVSal(time_dims=T_)
    synth.load_synth_weights(m, 0)
    return m.to(DEV).eval()


def test_recurrence_step_sets_only_the_recurrence_gradient():
    m = _model()
    x, cb, y = _step_inputs()
    rc = m.rnn.cell_list[0].rnn_conv
    loss, out, st = train.recurrence_step(m, x, cb, None, y)
    ref_out, ref_st = m(x, cb, None)
    assert torch.equal(out, ref_out) and torch.equal(st[0], ref_st[0]) and not st[0].requires_grad
    assert loss.item() == losses.loss_fu(ref_out, y).item()
    assert [k for k, p in m.named_parameters() if p.grad is not None] == ["rnn.cell_list.0.rnn_conv.weight"]
    g1 = rc.weight.grad.clone()
    assert torch.isfinite(g1).all() and float(g1.abs().max()) > 0
    train.recurrence_step(m, x, cb, None, y)                                       # .grad += as loss.backward() would
    _check(rc.weight.grad, 2 * g1.double(), 4 * R.U * g1.double().abs(), "second call doubles the gradient")
    # a directional derivative: loss(W + s D) - loss(W - s D) over 2 s against <grad, D>, D = grad / ||grad||.  The kernels are
    # held to their bounds one by one above; this checks the plumbing (which buffer goes where, the carried state, the
    # decoder in between), whose errors are of order 1.  10 %: the central difference's own truncation and the fp32
    # forward's noise in a difference of two losses
    with torch.no_grad():
        D = g1 / g1.norm()
        w0 = rc.weight.detach().clone()
        s = 2e-2 / float(g1.norm())            # the loss moves by about 0.02 to either side: linear there, far above fp32 noise
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
    """360x640, time_dims 5, one group of five frames that starts from the state the forward left after five OTHER frames:
    the 45x80 map, K = 18000, two chunks per share, 9 shares, the last one 1024 + 592 pixels.  in_state[0] is h0: the start of
    the history, frame 0's partner in the weight gradient, and it arrives as the forward hands it over."""
    from iip_uavsal_saliency_amd import UAVSal
    HH, WW, T = 360, 640, 5
    h, w = HH // 8, WW // 8
    assert R.wgrad_partition(T, h, w)[:2] == (2, 9)
    m = UAVSal(time_dims=T)
    synth.load_synth_weights(m, 0)
    m = m.to(DEV).eval()
    frames = torch.from_numpy(synth.normalize_frames(synth.synth_frames_u8(2 * T, HH, WW, 3))).to(DEV)
    cb = [torch.from_numpy(synth.gauss_priors(T, h, w)).to(DEV), torch.from_numpy(synth.ob_priors(T, h, w, seed=3)).to(DEV)]
    loc = synth.synth_fix_points(T, 180, 320, 12, 4)
    fmap = np.rint(synth.synth_fix_maps(loc, 6.0) * 255).astype(np.uint8)
    y, has = ops.prepare_gaze(torch.from_numpy(fmap).to(DEV), torch.from_numpy(loc).to(DEV), h, w)
    assert bool(has.all())
    _, state = m(frames[:T], cb, None)
    x = frames[T:]
    state = [state[0].detach()]
    assert tuple(state[0].shape) == (1, 256, h, w) and float(state[0].abs().max()) > 0
    s0 = state[0].clone()
    rc = m.rnn.cell_list[0].rnn_conv
    loss, out, st = train.recurrence_step(m, x, cb, state, y)
    assert torch.equal(state[0], s0)                                               # the step left the caller's state alone
    ref_out, ref_st = m(x, cb, state)
    assert torch.equal(out, ref_out) and torch.equal(st[0], ref_st[0]) and not st[0].requires_grad
    assert loss.item() == losses.loss_fu(ref_out, y).item()
    assert not torch.equal(ref_out, m(x, cb, None)[0])                             # the state matters to this group
    assert [k for k, p in m.named_parameters() if p.grad is not None] == ["rnn.cell_list.0.rnn_conv.weight"]
    g1 = rc.weight.grad.clone()
    assert torch.isfinite(g1).all() and float(g1.abs().max()) > 0
    # the directional derivative of test_recurrence_step_sets_only_the_recurrence_gradient, from the same in_state
    with torch.no_grad():
        D = g1 / g1.norm()
        w0 = rc.weight.detach().clone()
        s = 2e-2 / float(g1.norm())
        vals = []
        for sign in (1.0, -1.0):
            rc.weight.copy_(w0 + sign * s * D)
            m.refresh_weights(m.rnn)
            vals.append(losses.loss_fu(m(x, cb, state)[0], y).item())
        rc.weight.copy_(w0)
        m.refresh_weights(m.rnn)
    fd, an = (vals[0] - vals[1]) / (2 * s), float(g1.norm())
    print("carried state, 45x80 map: finite difference %.6e, <grad, D> %.6e, step %.3e" % (fd, an, s))
    assert abs(fd - an) <= 0.10 * abs(an)


def test_optimizer_step_and_refresh_keep_the_plans():
    from iip_uavsal_saliency_amd import UAVSal
    m = _model()
    x, cb, y = _step_inputs()
    opt = torch.optim.Adam(m.rnn.parameters(), lr=1e-4, betas=(0.9, 0.999), weight_decay=5e-5)
    before = m(x, cb, None)[0]
    first = None
    for _ in range(5):
        opt.zero_grad()
        loss, _, _ = train.recurrence_step(m, x, cb, None, y)
        first = loss.item() if first is None else first
        engines = dict(m._engines)
        opt.step()
        assert m.refresh_weights(m.rnn) > 0
        after = m(x, cb, None)[0]
        assert {k: id(e) for k, e in m._engines.items()} == {k: id(e) for k, e in engines.items()}      # the same engine objects
    last = losses.loss_fu(after, y).item()
    print("loss_fu on the group: %.6f before, %.6f after five Adam steps" % (first, last))
    assert last < first and not torch.equal(before, after)
    fresh = UAVSal(time_dims=T_)
    fresh.load_state_dict(m.state_dict())
    fresh = fresh.to(DEV).eval()
    want, want_st = fresh(x, cb, None)
    got, got_st = m(x, cb, None)
    assert torch.equal(got, want) and torch.equal(got_st[0], want_st[0])           # bit for bit the repacked weights
    taps = {}
    m(x, cb, None, taps=taps)
    ftaps = {}
    fresh(x, cb, None, taps=ftaps)
    assert torch.equal(taps["rnn"], ftaps["rnn"])


def test_refresh_drops_the_plans_when_another_parameter_moved():
    """only the named modules are repacked in place: an in-place edit elsewhere makes refresh_weights drop everything"""
    from iip_uavsal_saliency_amd import UAVSal
    m = _model()
    x, cb, _ = _step_inputs()
    m(x, cb, None)
    with torch.no_grad():
        m.rnn.cell_list[0].rnn_conv.weight.mul_(1.01)
        m.conv_out_st.conv[2].weight.mul_(1.5)
    assert m.refresh_weights(m.rnn) == 0 and len(m._engines) == 0 and m._wversion is None
    fresh = UAVSal(time_dims=T_)
    fresh.load_state_dict(m.state_dict())
    assert torch.equal(m(x, cb, None)[0], fresh.to(DEV).eval()(x, cb, None)[0])


def test_public_wrappers_check_shapes():
    t = _teacher((3, 5, 7))
    dz, x, hist, h0 = _nhwc(t["dz"]).contiguous(), _nhwc(t["x"]), _nhwc(t["hist"]), _nhwc(t["h0"])
    with pytest.raises(RuntimeError, match="twa_wgrad"):
        train.twa_wgrad(dz, x[:2], hist, h0)
    with pytest.raises(RuntimeError, match="twa_wgrad"):
        train.twa_wgrad(dz, x, hist, hist)
    with pytest.raises(RuntimeError, match="twa_gate_bwd"):
        train.twa_gate_bwd(dz, None, dz[:2], x, hist)
    with pytest.raises(RuntimeError, match="twa_gate_bwd"):
        train.twa_gate_bwd(dz, dz[:, :, :, :128], dz, x, hist)


def test_finetune_video_is_the_manual_loop():
    from iip_uavsal_saliency_amd.stream import finetune_video, validate_video
    m = _model()
    n = 5 * T_ + 1
    frames = torch.from_numpy(synth.synth_frames_u8(n, H_, W_, 2)).to(DEV)
    gp = torch.from_numpy(synth.gauss_priors(1, H_ // 8, W_ // 8)[0]).to(DEV)
    op_ = torch.from_numpy(synth.ob_priors(1, H_ // 8, W_ // 8)[0]).to(DEV)
    loc = synth.synth_fix_points(n, 90, 130, 12, 9)
    fmap = np.rint(synth.synth_fix_maps(loc, 6.0) * 255).astype(np.uint8)
    loc[2 * T_ + 1] = 0                                                            # the second group of two chunks is skipped
    fix_map, fix_loc = torch.from_numpy(fmap).to(DEV), torch.from_numpy(loc).to(DEV)
    val = validate_video(m, frames, gp, op_, fix_map, fix_loc, batch_size=2)
    opt = torch.optim.Adam(m.rnn.parameters(), lr=1e-4, betas=(0.9, 0.999), weight_decay=5e-5)
    w0 = m.rnn.cell_list[0].rnn_conv.weight.detach().clone()
    res = finetune_video(m, frames, gp, op_, fix_map, fix_loc, opt, batch_size=2)
    assert sorted(res) == sorted(val) and res["losses"].shape == val["losses"].shape
    got, want = res["losses"].numpy(), val["losses"].numpy()
    assert [bool(np.isnan(v)) for v in got] == [bool(np.isnan(v)) for v in want] == [False, True, False]
    assert got[0] == want[0]                                                       # the first group sees the untouched weights
    assert res["groups_run"] == 2 and res["num_step"] == 2 and res["video_mean"] == (float(got[0]) + float(got[2])) / 3
    assert not torch.equal(m.rnn.cell_list[0].rnn_conv.weight.detach(), w0)
    assert [k for k, p in m.named_parameters() if p.grad is not None] == ["rnn.cell_list.0.rnn_conv.weight"]
