"""The fusion block on batch statistics on the GPU (csrc/train_bn.hip: uavsal_bn_apply_res; train.bn_apply(res=),
train.block_forward_batch / block_backward_batch, train.twa_forward / lstm_forward, recurrence_step(block_stats=("fuse",)),
stream.finetune_video(block_stats=...)) against the float64 restatement tests/fuse_bn_ref64.py, which runs on the device in
torch float64.  Bounds: its docstring and tests/decoder_bn_ref64.py's.  Every stage is held against float64 of the fp32
tensors the device's stage read, the ReLU6 masks taken from the device's own activations (no element excluded).  Block shapes
(T, H, W): (2,5,7), odd in both directions, and (3,13,17): two slabs, the last one partial (the count is read from the
library's own query); the recurrence at (3,5,7) from a zero state and (5,12,20) from a given one."""

import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import losses, ops, synth, train
from iip_uavsal_saliency_amd.train import bn as B

import decoder_bn_ref64 as BR
import fuse_bn_ref64 as FR
import lstm_ref64 as LR
import train_ref64 as R
from test_train_decoder_bn_gpu import _bits, _check, _f64, _one_ulp, _same, _step_inputs  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last
ACTS = (BR.ACT_NONE, BR.ACT_RELU6, BR.ACT_SIGMOID)
CASES = [(cfg, shape) for cfg in FR.CFGS for shape in FR.SHAPES]
IDS = [FR.name(c, s) for c, s in CASES]


def _dev(a):
    return torch.as_tensor(a).to(DEV)


# ------------------------------------------------------------------------------------------------ 1. uavsal_bn_apply_res
@pytest.mark.parametrize("shape", FR.SHAPES, ids=lambda s: "T%d_%dx%d" % s)
@pytest.mark.parametrize("c", [8, 256])
def test_bn_apply_with_a_residual(c, shape):
    x = BR.bn_inputs(c, shape)
    t = {k: _dev(v) for k, v in x.items()}
    f = train.bn_stats(t["u"], t["gamma"], t["beta"], BR.BN_EPS)
    T, H, W = shape
    rs = np.random.RandomState(31 + c + T * H * W)
    wide = _dev(rs.standard_normal((T, H, W, c + 8)).astype(np.float32))
    for what, res in (("dense", wide[..., :c].contiguous()), ("channel slice", wide[..., 4:c + 4])):
        if what != "dense":
            assert ops._nhwc_view(res)[1] == c + 8 and res.data_ptr() % 16 == 0
        for act in ACTS:
            out = train.bn_apply(t["u"], f, act, res=res)
            assert out.is_contiguous() and tuple(out.shape) == (T, H, W, c)
            want, bound = FR.apply_res(t["u"].double(), _f64(f), res.double(), act)
            _check(out, want, bound, "apply_res %s %s" % (what, act))
            assert _same(out, train.bn_apply(t["u"], f, act, res=res))                     # the same bits twice
            plain = train.bn_apply(t["u"], f, act)
            assert _same(plain, train.bn_apply(t["u"], f, act, res=None))                  # without it: today's launch, today's bits
            assert _same(out, plain + res)                                                 # one more rounding of the sum, nothing else
    e = train.bn_apply(t["u"], f, "relu6")[..., 1:]                                        # both clamps hold elements
    assert float((e <= 0).float().mean()) >= 0.05 and float((e >= 6).float().mean()) >= 0.05
    with pytest.raises(RuntimeError, match="res must be"):
        train.bn_apply(t["u"], f, None, res=wide)
    with pytest.raises(RuntimeError, match="do not combine"):
        train.bn_apply(t["u"], f, None, dot_w=t["gamma"], res=wide[..., :c])


# ------------------------------------------------------------------------------------------------ 2. the block at its real widths
def _block(cfg, q):
    from iip_uavsal_saliency_amd.model import dwBlock
    c = FR.CFG[cfg]
    return FR.load_block(dwBlock(c["cin"], c["cout"], kernel_size=3), q).to(DEV)


def _module_numbers(block):
    q = {k: v.detach().double() for k, v in (("w1", block.conv[0][0].weight), ("wd", block.conv[1][0].weight),
                                             ("w3", block.conv[2].weight))}
    for i, bn in ((1, block.conv[0][1]), (2, block.conv[1][1]), (3, block.conv[3])):
        q["g%d" % i], q["be%d" % i] = bn.weight.detach().double(), bn.bias.detach().double()
    return q


def _walk(block, x, go, saved, parts, grads, grad_x, out, q):
    """Every stage of the device's forward and backward against float64 of what that stage read on the device.  `q`: the
    module's numbers as float64 tensors (weights, gamma, beta)."""
    res = block.use_res_connect
    xn, gon = x.permute(0, 2, 3, 1).double(), go.permute(0, 2, 3, 1).double()
    u1, e, u2, d, u3 = (saved[k] for k in ("u1", "e", "u2", "d", "u3"))
    f1, f2, f3 = (_f64(saved[k]) for k in ("f1", "f2", "f3"))
    hid, cin = q["w1"].shape[:2]
    cout = q["w3"].shape[0]
    N = FR.NAMES
    worst = {}
    ck = lambda k, got, want, bound: worst.__setitem__(k, _check(got, want, bound, k))      # noqa: E731
    ck("u1", u1, *BR.conv1x1(xn, q["w1"]))
    for i, u, f in ((1, u1, saved["f1"]), (2, u2, saved["f2"]), (3, u3, saved["f3"])):
        want, bound = BR.stats(u.double(), q["g%d" % i], q["be%d" % i], bounds=True)
        for k in ("mu", "var", "r", "s", "b"):
            ck("%s%d" % (k, i), getattr(f, k), want[k], bound[k])
    ck("e", e, *BR.apply(u1.double(), f1, BR.ACT_RELU6))
    ck("u2", u2, *BR.dw_raw(e.double(), q["wd"]))
    ck("d", d, *BR.apply(u2.double(), f2, BR.ACT_RELU6))
    ck("u3", u3, *BR.conv1x1(d.double(), q["w3"]))
    ck("out", out.permute(0, 2, 3, 1), *(FR.apply_res(u3.double(), f3, xn) if res else BR.apply(u3.double(), f3, BR.ACT_NONE)))
    m1, m2 = (e > 0) & (e < 6), (d > 0) & (d < 6)                          # the device's own activations decide the masks
    g_u1, g_u2, g_u3, g_e, g_d = (parts[k] for k in ("g_u1", "g_u2", "g_u3", "g_e", "g_d"))
    S3, e3, e3f = BR.bwd_sums(gon, u3.double(), f3, BR.ACT_NONE, bounds=True)
    ck(N[8], grads[N[8]], S3[0], e3f[0])
    ck(N[7], grads[N[7]], S3[1], e3f[1])
    ck("g_u3", g_u3, *BR.bwd_apply(gon, u3.double(), f3, S3, BR.ACT_NONE, bounds=True, sums_err=e3))
    ck(N[6], grads[N[6]].reshape(cout, hid), *BR.pix_gemm(g_u3.double(), d.double()))
    ck("g_d", g_d, *BR.conv1x1(g_u3.double(), q["w3"], transpose=True))
    S2, e2, e2f = BR.bwd_sums(g_d.double(), u2.double(), f2, BR.ACT_RELU6, mask=m2, bounds=True)
    ck(N[5], grads[N[5]], S2[0], e2f[0])
    ck(N[4], grads[N[4]], S2[1], e2f[1])
    ck("g_u2", g_u2, *BR.bwd_apply(g_d.double(), u2.double(), f2, S2, BR.ACT_RELU6, mask=m2, bounds=True, sums_err=e2))
    ck(N[3], grads[N[3]], *BR.dw_wgrad(g_u2.double(), e.double(), bounds=True))
    ck("g_e", g_e, *BR.dw_raw(g_u2.double(), q["wd"], transpose=True))
    S1, e1, e1f = BR.bwd_sums(g_e.double(), u1.double(), f1, BR.ACT_RELU6, mask=m1, bounds=True)
    ck(N[2], grads[N[2]], S1[0], e1f[0])
    ck(N[1], grads[N[1]], S1[1], e1f[1])
    ck("g_u1", g_u1, *BR.bwd_apply(g_e.double(), u1.double(), f1, S1, BR.ACT_RELU6, mask=m1, bounds=True, sums_err=e1))
    ck(N[0], grads[N[0]].reshape(hid, cin), *BR.pix_gemm(g_u1.double(), xn))
    if grad_x is not None:
        ck("grad_x", grad_x.permute(0, 2, 3, 1), *FR.grad_x(g_u1.double(), q["w1"], gon if res else None))
    return worst


@pytest.mark.parametrize("cfg,shape", CASES, ids=IDS)
def test_block_forward_and_backward_batch(cfg, shape):
    xn, qn, gon = FR.block_case(cfg, shape)
    block = _block(cfg, qn)
    q = FR.to64(qn, DEV)
    x = _dev(xn).contiguous(memory_format=CL)
    go = _dev(gon)
    T, H, W = shape
    c = FR.CFG[cfg]
    if shape == FR.SLAB_SHAPE:
        slabs, rows = B.slabs(T, H, W)
        assert slabs == 2 and (T * H) % rows != 0                          # two slabs, a partial last one
    bns = (block.conv[0][1], block.conv[1][1], block.conv[3])
    out, saved = train.block_forward_batch(block, x)
    assert tuple(out.shape) == (T, c["cout"], H, W) and sorted(saved) == ["d", "e", "f1", "f2", "f3", "u1", "u2", "u3"]
    parts = {}
    grad_x, grads = train.block_backward_batch(block, x, go, saved=saved, parts=parts)
    assert tuple(grads) == FR.NAMES and tuple(grad_x.shape) == (T, c["cin"], H, W)
    assert sorted(parts) == ["g_d", "g_e", "g_u1", "g_u2", "g_u3"]
    _walk(block, x, go, saved, parts, grads, grad_x, out, q)
    for t in (saved["e"], saved["d"]):                                     # at least 5 % of e and of d in each clamp
        lo, mid, hi = FR.clamp_shares(t)
        assert lo >= 0.05 and hi >= 0.05 and mid >= 0.25
    # the running statistics moved as torch moves them: float64 from the device's own u, rounded to fp32, one ulp
    for i, (bn, u) in enumerate(zip(bns, (saved["u1"], saved["u2"], saved["u3"])), 1):
        st = BR.stats(u.double(), q["g%d" % i], q["be%d" % i])
        wm, wv = BR.running(q["rm%d" % i], q["rv%d" % i], st["mu"], st["var"], T * H * W)
        _one_ulp(bn.running_mean, wm, "running_mean %d" % i)
        _one_ulp(bn.running_var, wv, "running_var %d" % i)
        assert int(bn.num_batches_tracked) == 1
    # the whole chain against the float64 closed form from the module's numbers: figures, not assertions (the fp32 forward may
    # decide a mask the other way, which no bound of a single stage covers; the stage walk above is the assertion)
    ref = FR.block_train(q, _dev(xn).double(), go.double(), c["res"])
    for n in FR.NAMES + ("grad_x", "out"):
        got = {"grad_x": grad_x, "out": out}.get(n, grads.get(n))
        print("%s whole chain %s: relative L2 distance %.3e" % (FR.name(cfg, shape), n,
                                                                float((got.double() - ref[n]).norm() / ref[n].norm())))
    c1, c2 = FR.ZERO_GAMMA                                                 # gamma = 0: no gradient into u, a gamma gradient
    assert float(parts["g_u1"][..., c1].abs().max()) == 0.0 and float(grads[FR.NAMES[1]][c1].abs()) > 0.0
    assert float(parts["g_u2"][..., c2].abs().max()) == 0.0 and float(grads[FR.NAMES[4]][c2].abs()) > 0.0
    # a second forward returns the same bits and moves the statistics again; without `saved` the backward runs the forward
    # itself and leaves the statistics alone; given gradient tensors are written in place, or added to
    out2, _ = train.block_forward_batch(block, x)
    assert _same(out, out2) and int(bns[0].num_batches_tracked) == 2
    before = [b.clone() for b in block.buffers()]
    mine = {n: torch.zeros_like(v) for n, v in grads.items()}
    gx2, same = train.block_backward_batch(block, x, go, grads=mine)
    assert same is mine and _same(gx2, grad_x) and all(_same(mine[n], grads[n]) for n in FR.NAMES)
    assert all(torch.equal(a, b) for a, b in zip(before, block.buffers()))
    none, _ = train.block_backward_batch(block, x, go, saved=saved, need_x_grad=False, grads=mine, accumulate=True)
    assert none is None
    for n in FR.NAMES:
        _check(mine[n], 2 * grads[n].double(), 4 * BR.U * grads[n].double().abs(), "accumulate doubles %s" % n)
    with pytest.raises(RuntimeError, match="block_backward / block_input_grad"):
        train.block_forward_batch(block.eval(), x)
    block.train()
    with pytest.raises(RuntimeError, match=r"model\.eval\(\)"):            # the eval-mode backward keeps refusing a training block
        train.block_backward(block, x, go)


# ------------------------------------------------------------------------------------------------ 3. the recurrence forward
def _pitched(x):
    """`x` `[T,256,H,W]` as a channel slice of a wider NHWC tensor (pitch 264, 16-byte aligned)"""
    T, c, H, W = x.shape
    wide = torch.zeros((T, H, W, c + 8), dtype=torch.float32, device=x.device)
    wide[..., 4:c + 4] = x.permute(0, 2, 3, 1)
    v = wide[..., 4:c + 4].permute(0, 3, 1, 2)
    assert ops._nhwc_view(v.permute(0, 2, 3, 1))[1] == c + 8
    return v


@pytest.mark.parametrize("shape", FR.RNN_SHAPES, ids=R.name)
def test_twa_forward(shape):
    t = {k: _dev(v) for k, v in R.twa_inputs(shape).items()}
    x, w = t["x"].contiguous(memory_format=CL), t["w"]
    h0 = t["h0"] if shape in R.H0_NONZERO else None
    h_seq = train.twa_forward(x, h0, w)
    T, H, W = shape
    assert tuple(h_seq.shape) == (T, 256, H, W) and h_seq.is_contiguous(memory_format=CL)
    w64, prev = w.double(), t["h0"].double()
    for k in range(T):                                                     # every step, teacher-forced on the device's own h_{t-1}
        want, bound = FR.twa_step(x[k:k + 1].double(), prev, w64)
        _check(h_seq[k:k + 1], want, bound, "%s step %d" % (R.name(shape), k))
        prev = h_seq[k:k + 1].double()
    ref = FR.twa_forward(x.double(), t["h0"].double(), w64)
    print("%s free-running: relative L2 distance %.3e" % (R.name(shape), float((h_seq.double() - ref).norm() / ref.norm())))
    assert _same(h_seq, train.twa_forward(x, h0, w))                       # the same bits twice
    assert _same(h_seq, train.twa_forward(t["x"], h0, w))                  # NCHW memory: copied once, the same bits
    assert _same(h_seq, train.twa_forward(_pitched(t["x"]), h0, w))        # a channel slice is read in place
    if h0 is not None:
        assert not torch.equal(h_seq, train.twa_forward(x, None, w))
    with pytest.raises(RuntimeError, match="ConvTWA weight"):
        train.twa_forward(x, h0, w[:, :256])


@pytest.mark.parametrize("shape", FR.RNN_SHAPES, ids=LR.name)
def test_lstm_forward(shape):
    t = {k: _dev(v) for k, v in LR.lstm_inputs(shape).items()}
    x, w = t["x"].contiguous(memory_format=CL), t["w"]
    given = shape in LR.STATE_NONZERO
    h0, c0 = (t["h0"], t["c0"]) if given else (None, None)
    h_seq, c_last = train.lstm_forward(x, h0, c0, w)
    T, H, W = shape
    assert tuple(h_seq.shape) == (T, 256, H, W) and tuple(c_last.shape) == (1, 256, H, W)
    w64, hp, cp = w.double(), t["h0"].double(), t["c0"].double()
    for k in range(T):                 # every step, teacher-forced on the device's own h_{t-1} and c_{t-1} (that of the first k frames)
        c_k = train.lstm_forward(x[:k + 1], h0, c0, w)[1]
        wh, wc, bh, bc = FR.lstm_step(x[k:k + 1].double(), hp, cp, w64)
        _check(h_seq[k:k + 1], wh, bh, "%s h step %d" % (LR.name(shape), k))
        _check(c_k, wc, bc, "%s c step %d" % (LR.name(shape), k))
        hp, cp = h_seq[k:k + 1].double(), c_k.double()
    assert _same(c_k, c_last)
    h2, c2 = train.lstm_forward(x, h0, c0, w)
    assert _same(h_seq, h2) and _same(c_last, c2)
    hp_, cp_ = train.lstm_forward(_pitched(t["x"]), h0, c0, w)
    assert _same(h_seq, hp_) and _same(c_last, cp_)
    if given:
        assert not torch.equal(h_seq, train.lstm_forward(x, None, None, w)[0])
        keep = LR.lstm_inputs(shape)                                       # the caller's state is only read
        assert torch.equal(t["h0"].cpu(), torch.as_tensor(keep["h0"])) and torch.equal(t["c0"].cpu(), torch.as_tensor(keep["c0"]))
        ch0, cc0 = t["h0"].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), t["c0"].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        h3, c3 = train.lstm_forward(x, ch0, cc0, w)                        # ... also where it is NHWC memory, read in place
        assert _same(h3, h_seq) and _same(c3, c_last) and torch.equal(cc0, t["c0"]) and torch.equal(ch0, t["h0"])


# ------------------------------------------------------------------------------------------------ 4. the step and the driver
H_, W_, T_ = 72, 104, 4
RNN = "rnn.cell_list.0.rnn_conv.weight"
BIAS = {"priors": [1, 1, 1], "plain": [0, 0, 0]}


def _box_name(m):
    return "fucbst_layer" if m.num_cb else "fust_layer"


def _model(kind="priors", lstm=False):
    from iip_uavsal_saliency_amd import UAVSAL_LSTM, UAVSal
    m = UAVSAL_LSTM(time_dims=T_) if lstm else UAVSal(time_dims=T_, bias_type=BIAS[kind])
    synth.load_synth_weights(m, 0)
    with torch.no_grad():                                       # running statistics that are not the initial 0 and 1
        g = torch.Generator().manual_seed(13)
        for bn in [b for b in train.fuse_block(m)[0].modules() if isinstance(b, torch.nn.BatchNorm2d)]:
            bn.running_mean.add_(0.05 * torch.randn(bn.running_mean.shape, generator=g))
            bn.running_var.mul_(1.0 + 0.2 * torch.rand(bn.running_var.shape, generator=g))
    return m.to(DEV).eval()


def _fresh_like(m, kind):
    from iip_uavsal_saliency_amd import UAVSal
    f = UAVSal(time_dims=T_, bias_type=BIAS[kind])
    f.load_state_dict(m.state_dict())
    return f.to(DEV).eval()


def _grad_of(out, y):
    pred = out.detach().requires_grad_(True)
    with torch.enable_grad():
        (g_y,) = torch.autograd.grad(losses.loss_fu(pred, y), pred)
    return g_y


def _eval_decoder(dec, h_seq):
    """the eval-mode decoder's prediction on `h_seq` by the forward's own launches, through a public function"""
    parts = {}
    train.decoder_input_grad(dec, h_seq, torch.zeros_like(h_seq[:, :1]), parts=parts)
    y = parts["y"]
    return y.view(y.shape[0], 1, y.shape[1], y.shape[2])


@pytest.mark.parametrize("kind,lstm,both", [("priors", False, False), ("plain", False, False), ("priors", True, False),
                                             ("priors", False, True)], ids=["bias111", "bias000", "lstm", "both_keywords"])
def test_recurrence_step_on_the_fuse_blocks_batch_statistics(kind, lstm, both):
    m = _model(kind, lstm)
    x, cb, y = _step_inputs()
    blk, src = train.fuse_block(m)
    box = getattr(m, _box_name(m))
    pre = _box_name(m) + ".0."
    assert blk.use_res_connect == (kind == "plain")
    dec, rc = m.conv_out_st, m.rnn.cell_list[0].rnn_conv
    kw = dict(fuse=True, block_stats=("fuse",), **({"lstm": True} if lstm else {}))
    if both:
        kw.update(decoder=True, batch_stats=("decoder",))
    behind = kind == "priors" and not lstm and not both                    # fust and ctx hang off the block's grad_x
    if behind:
        kw.update(fust=True, ctx=True)
    taps = {src: None, "cb192": None} if m.num_cb else {src: None}
    plan_out, _ = m(x, cb, None, taps=taps)
    fu = taps[src].contiguous(memory_format=CL)
    stats0 = {k: v.clone() for k, v in blk.state_dict().items() if "running" in k or "tracked" in k}
    if both:
        dec.train()
    with pytest.raises(RuntimeError, match=_box_name(m) + r"\.train\(\)"):     # the keyword with the block in eval mode
        train.recurrence_step(m, x, cb, None, y, **kw)
    box.train()
    assert not m.training and blk.training and all(p.grad is None for p in m.parameters())
    loss, out, st = train.recurrence_step(m, x, cb, None, y, **kw)
    # out, the loss and the state are the composition of the public functions on the plan's tap, bit for bit
    want_x, bsaved = train.block_forward_batch(blk, fu, update_running=False)
    if lstm:
        want_h, want_c = train.lstm_forward(want_x, None, None, rc.weight.detach())
        assert len(st) == 2 and _same(st[1], want_c)
    else:
        want_h = train.twa_forward(want_x, None, rc.weight.detach())
        assert len(st) == 1
    if both:
        want_y, dsaved = train.decoder_forward_batch(dec, want_h, update_running=False)
    else:
        want_y = _eval_decoder(dec, want_h)
    assert _same(out, want_y) and _same(st[0], want_h[-1:]) and loss.item() == losses.loss_fu(want_y, y).item()
    assert not torch.equal(out, plan_out) and not any(t.requires_grad for t in st)
    print("%s: the plan's prefuse against the batch-statistics one: relative L2 distance %.3e; out: %.3e"
          % (kind, float((want_x - taps["prefuse"]).norm() / taps["prefuse"].norm()), float((out - plan_out).norm() / plan_out.norm())))
    # the recurrence forward on the plan's OWN prefuse tap against the plan's rnn tap: a figure (the plan's route -- Winograd
    # for the ConvTWA steps -- differs by design)
    if lstm:
        mine = train.lstm_forward(taps["prefuse"].contiguous(memory_format=CL), None, None, rc.weight.detach())[0]
    else:
        mine = train.twa_forward(taps["prefuse"].contiguous(memory_format=CL), None, rc.weight.detach())
    print("%s: %s_forward on the plan's prefuse tap against the plan's rnn tap: max |diff| %.3e, relative L2 distance %.3e"
          % (kind, "lstm" if lstm else "twa", float((mine - taps["rnn"]).abs().max()), float((mine - taps["rnn"]).norm() / taps["rnn"].norm())))
    # exactly the expected .grads are set, and they are that composition's
    params = dict(m.named_parameters())
    expect = [RNN] + [pre + n for n in FR.NAMES]
    if both:
        expect += ["conv_out_st." + n for n in FR.NAMES]
    if behind:
        expect += ["fust_layer.0." + n for n in FR.NAMES]
        expect += [k for k in params if k.startswith("fucb_layer.") or k.startswith("cxt_cb_prior.")]
    assert sorted(k for k, p in params.items() if p.grad is not None) == sorted(expect)
    g_y = _grad_of(want_y, y)
    if both:
        grad_h, dgrads = train.decoder_backward_batch(dec, want_h, g_y, saved=dsaved)
        assert all(_same(params["conv_out_st." + n].grad, dgrads[n]) for n in FR.NAMES)
    else:
        grad_h = train.decoder_input_grad(dec, want_h, g_y, y=want_y)
    if lstm:
        gw, grad_x, _, _ = train.lstm_backward(want_x, want_h, None, None, rc.weight.detach(), grad_h, need_x_grad=True)
    else:
        gw, grad_x, _ = train.twa_backward(want_x, want_h, None, rc.weight.detach(), grad_h, need_x_grad=True)
    assert _same(params[RNN].grad, gw)
    parts = {}
    grad_fu, bgrads = train.block_backward_batch(blk, fu, grad_x, saved=bsaved, need_x_grad=True, parts=parts)
    g1 = {k: params[k].grad.clone() for k in expect}
    for n in FR.NAMES:
        assert _same(g1[pre + n], bgrads[n]), n
        assert float(bgrads[n].abs().max()) > 0 and torch.isfinite(bgrads[n]).all()
    # ... every stage of which is within its bound of float64 of what it read
    _walk(blk, fu, grad_x, bsaved, parts, bgrads, grad_fu, want_x, _module_numbers(blk))
    if behind:                                                             # the stages behind received that grad_x unchanged
        g_fust, pgrads = train.prior_path_backward(m, fu, taps["cb192"], grad_fu, grads={n: None for n in train.prior_path_blocks(m)})
        for name, b in train.prior_path_blocks(m).items():
            for n, p in b.named_parameters():
                assert _same(p.grad, pgrads[name][n]), (name, n)
        st_tap = taps["st%d" % (len(m.st_layer) - 1)]
        _, fgrads = train.block_backward(m.fust_layer[0], st_tap.contiguous(memory_format=CL), g_fust, need_x_grad=False)
        assert all(_same(params["fust_layer.0." + n].grad, fgrads[n]) for n in FR.NAMES)
    # the running statistics moved, by the rule, and the counters went up by one
    q = _module_numbers(blk)
    for i, bn in ((1, blk.conv[0][1]), (2, blk.conv[1][1]), (3, blk.conv[3])):
        p_ = "conv.%s." % ("0.1", "1.1", "3")[i - 1]
        u = bsaved["u%d" % i].double()
        fs = BR.stats(u, q["g%d" % i], q["be%d" % i])
        wm, wv = BR.running(stats0[p_ + "running_mean"].double(), stats0[p_ + "running_var"].double(), fs["mu"], fs["var"],
                            u.shape[0] * u.shape[1] * u.shape[2], momentum=bn.momentum)
        _one_ulp(bn.running_mean, wm, "running_mean %d" % i)
        _one_ulp(bn.running_var, wv, "running_var %d" % i)
        assert not torch.equal(bn.running_mean, stats0[p_ + "running_mean"])
        assert int(bn.num_batches_tracked) == int(stats0[p_ + "num_batches_tracked"]) + 1
    if not both:
        assert int(dec.conv[3].num_batches_tracked) == 0                   # the eval-mode decoder's statistics stayed
    # a second step with .grad present adds to it (no weight moved; the batch path does not read the running statistics)
    train.recurrence_step(m, x, cb, None, y, **kw)
    for k in expect:
        _check(params[k].grad, 2 * g1[k].double(), 4 * BR.U * g1[k].double().abs(), "second call doubles %s" % k)
    assert int(blk.conv[3].num_batches_tracked) == int(stats0["conv.3.num_batches_tracked"]) + 2


def test_both_keywords_are_the_chain_goldens_configuration():
    """block.train() -> ConvTWA -> decoder.train() + sigmoid, the chain tests/golden/fuse_bn_chain_T3_5x7.npz records from the
    reference's modules, composed from the public functions the step composes (the step's own bits ARE that composition:
    test_recurrence_step_on_the_fuse_blocks_batch_statistics[both_keywords]): within rounding of the float64 chain, whose
    distance the CPU test holds to the reference's at 1e-11.  The per-element assertions are the stage walks; here every tensor
    of the chain is held in relative L2 norm to `FR.CHAIN_TOL` (its derivation: tests/fuse_bn_ref64.py), loose enough for a
    mask that falls the other way and far below what a wrong chain gives (the CPU test holds the wrong variants to it)."""
    from iip_uavsal_saliency_amd.model import dwBlock
    xn, qb, h0n, wn, qd, gyn = FR.chain_case()
    blk = FR.load_block(dwBlock(320, 256, kernel_size=3), qb).to(DEV)
    dec = FR.load_block(dwBlock(256, 1, kernel_size=3), qd).to(DEV)
    x, h0, w, gy = _dev(xn).contiguous(memory_format=CL), _dev(h0n), _dev(wn), _dev(gyn)
    x_seq, bsaved = train.block_forward_batch(blk, x)
    h_seq = train.twa_forward(x_seq, h0, w)
    yv, dsaved = train.decoder_forward_batch(dec, h_seq)
    grad_h, dgrads = train.decoder_backward_batch(dec, h_seq, gy, saved=dsaved)
    gw, grad_x, _ = train.twa_backward(x_seq, h_seq, h0, w, grad_h, need_x_grad=True)
    grad_in, bgrads = train.block_backward_batch(blk, x, grad_x, saved=bsaved)
    ref = FR.chain_train(FR.to64(qb, DEV), x.double(), h0.double(), w.double(), FR.to64(qd, DEV), gy.double())
    rel = lambda a, b: float((a.double() - b).norm() / b.norm())           # noqa: E731
    print("chain y: max |diff| %.3e" % float((yv.double() - ref["y"]).abs().max()))
    print("chain rnn weight gradient: relative L2 distance %.3e; grad_x: %.3e" % (rel(gw, ref["rnn"]), rel(grad_in, ref["grad_x"])))
    for n in FR.NAMES:
        print("chain block %s: %.3e; decoder %s: %.3e" % (n, rel(bgrads[n], ref["block"][n]), n, rel(dgrads[n], ref["decoder"][n])))
    print("chain h_seq: relative L2 distance %.3e; x_seq: %.3e" % (rel(h_seq, ref["h_seq"]), rel(x_seq, ref["x_seq"])))
    held = [("y", yv, ref["y"]), ("x_seq", x_seq, ref["x_seq"]), ("h_seq", h_seq, ref["h_seq"]), ("rnn", gw, ref["rnn"]),
            ("grad_x", grad_in, ref["grad_x"])]
    held += [("block " + n, bgrads[n], ref["block"][n]) for n in FR.NAMES] + [("decoder " + n, dgrads[n], ref["decoder"][n]) for n in FR.NAMES]
    for what, got, want in held:
        assert bool(torch.isfinite(got).all()) and rel(got, want) <= FR.CHAIN_TOL, what
    for i, (bn, part) in enumerate([(b, "block") for b in (blk.conv[0][1], blk.conv[1][1], blk.conv[3])]
                                   + [(b, "decoder") for b in (dec.conv[0][1], dec.conv[1][1], dec.conv[3])]):
        k = i % 3 + 1                                                      # the moved running statistics of both blocks
        assert rel(bn.running_mean, ref[part]["rm%d" % k]) <= FR.CHAIN_TOL and rel(bn.running_var, ref[part]["rv%d" % k]) <= FR.CHAIN_TOL


@pytest.mark.parametrize("kind", ["priors", "plain"], ids=["bias111", "bias000"])
def test_without_the_keyword_the_step_is_the_eval_mode_step(kind):
    m = _model(kind)
    x, cb, y = _step_inputs()
    blk, src = train.fuse_block(m)
    stats = [b.clone() for b in m.buffers()]
    loss, out, st = train.recurrence_step(m, x, cb, None, y, fuse=True, block_stats=())
    taps = {src: None}
    ref_out, ref_st = m(x, cb, None, taps=taps)
    assert torch.equal(out, ref_out) and torch.equal(st[0], ref_st[0]) and loss.item() == losses.loss_fu(ref_out, y).item()
    g_y = _grad_of(ref_out, y)
    h_seq, x_seq = taps["rnn"].contiguous(memory_format=CL), taps["prefuse"].contiguous(memory_format=CL)
    grad_h = train.decoder_input_grad(m.conv_out_st, h_seq, g_y, y=ref_out)
    rc = m.rnn.cell_list[0].rnn_conv
    gw, grad_x, _ = train.twa_backward(x_seq, h_seq, None, rc.weight.detach(), grad_h, need_x_grad=True)
    _, grads = train.block_backward(blk, taps[src].contiguous(memory_format=CL), grad_x, need_x_grad=False)
    params = dict(m.named_parameters())
    pre = _box_name(m) + ".0."
    assert _same(params[RNN].grad, gw) and all(_same(params[pre + n].grad, grads[n]) for n in FR.NAMES)
    assert all(torch.equal(a, b) for a, b in zip(stats, m.buffers()))                                # no buffer moved
    getattr(m, _box_name(m)).train()
    with pytest.raises(RuntimeError, match="eval"):                        # and a block in training mode still raises without it
        train.recurrence_step(m, x, cb, None, y, fuse=True)
    getattr(m, _box_name(m)).eval()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_refresh_refolds_the_eval_forms_from_the_moved_statistics(device):
    """After a step on the fuse block's batch statistics and an optimiser step, `refresh_weights` -- on the host, and
    `device=True` -- refolds the block's eval-mode packed forms from the MOVED running statistics: the eval forward is that of a
    freshly built model loaded with the same `state_dict`, bit for bit, and the plans were kept.  One thing of the device path
    is not the host packer's bytes by design, whatever was trained: the Winograd transform of the recurrence's 3x3 weight
    (csrc/repack.hip: within one fp32 ulp, tests/test_repack_gpu.py), so in the device case the fresh model's recurrence is
    refreshed on the device as well -- its fuse-block entries stay the host packer's, which is what the comparison is about."""
    m = _model("priors")
    x, cb, y = _step_inputs()
    before, _ = m(x, cb, None)                                             # packs the weights, builds the plan
    m.fucbst_layer.train()
    opt = torch.optim.Adam(list(m.rnn.parameters()) + list(m.fucbst_layer.parameters()), lr=1e-4)
    train.recurrence_step(m, x, cb, None, y, fuse=True, block_stats=("fuse",))
    engines = dict(m._engines)
    opt.step()
    assert m.refresh_weights(m.rnn, m.fucbst_layer, device=device) > 0
    m.fucbst_layer.eval()
    got, got_st = m(x, cb, None)
    assert {k: id(e) for k, e in m._engines.items()} == {k: id(e) for k, e in engines.items()}      # the plans were kept
    fresh = _fresh_like(m, "priors")
    if device:
        fresh(x, cb, None)
        assert fresh.refresh_weights(fresh.rnn, device=True) > 0
    want, want_st = fresh(x, cb, None)
    assert not torch.equal(got, before)
    assert torch.equal(got, want) and torch.equal(got_st[0], want_st[0])


def test_finetune_video_on_the_fuse_blocks_batch_statistics_restores_the_modes():
    from iip_uavsal_saliency_amd.stream import finetune_video, validate_video
    n = 2 * T_ * 3
    frames = torch.from_numpy(synth.synth_frames_u8(n, H_, W_, 2)).to(DEV)
    gp = torch.from_numpy(synth.gauss_priors(1, H_ // 8, W_ // 8)[0]).to(DEV)
    op_ = torch.from_numpy(synth.ob_priors(1, H_ // 8, W_ // 8)[0]).to(DEV)
    loc = synth.synth_fix_points(n, 90, 130, 12, 9)
    fmap = np.rint(synth.synth_fix_maps(loc, 6.0) * 255).astype(np.uint8)
    fix_map, fix_loc = torch.from_numpy(fmap).to(DEV), torch.from_numpy(loc).to(DEV)
    m = _model("priors")
    blk = m.fucbst_layer[0]
    opt = torch.optim.Adam(list(m.rnn.parameters()) + list(m.conv_out_st.parameters()) + list(m.fucbst_layer.parameters()),
                           lr=1e-4, betas=(0.9, 0.999), weight_decay=5e-5)
    nbt = int(blk.conv[3].num_batches_tracked)
    rm0 = blk.conv[0][1].running_mean.clone()
    res = finetune_video(m, frames, gp, op_, fix_map, fix_loc, opt, batch_size=2, stages=("rnn", "decoder", "fuse"),
                         block_stats=("fuse",))
    assert res["groups_run"] == 3 and torch.isfinite(res["losses"]).all()
    assert not m.training and not any(b.training for b in m.modules())
    assert int(blk.conv[3].num_batches_tracked) == nbt + 3 and not torch.equal(blk.conv[0][1].running_mean, rm0)
    assert int(m.conv_out_st.conv[3].num_batches_tracked) == 0             # the decoder stayed on its running statistics
    # the eval forward afterwards is that of a freshly built model with the same state: validation stays on running statistics
    val = validate_video(m, frames, gp, op_, fix_map, fix_loc, batch_size=2)
    ref = validate_video(_fresh_like(m, "priors"), frames, gp, op_, fix_map, fix_loc, batch_size=2)
    assert torch.equal(val["losses"], ref["losses"])
    assert int(blk.conv[3].num_batches_tracked) == nbt + 3
