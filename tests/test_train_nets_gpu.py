"""Fine-tuning the gauss / ob prior nets on the device (train.narrow_block_param_grads, train.frame_sum,
train.prior_net_backward, train.recurrence_step(nets=True), stream.finetune_video(stages=(..., "nets")); csrc/train_nets.hip)
against the float64 restatement tests/nets_ref64.py, whose docstring derives every bound."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import _lib, losses, ops, synth, train

import block_ref64 as BR
import ctx_ref64 as X
import mp_ref64 as MP
import nets_ref64 as NR
import train_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _nhwc(t, keep_masks=False):
    """a float64 (or numpy) NCHW tensor as the dense fp32 NHWC tensor the kernels read"""
    t = torch.as_tensor(t).to(DEV)
    t32 = BR.teacher_round(t.double()) if keep_masks else t.float()
    return t32.permute(0, 2, 3, 1).contiguous()


def _nchw64(t):
    return t.permute(0, 3, 1, 2).double()


def _d64(a):
    return torch.as_tensor(a).to(DEV).double()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(got, want, bound, what):
    err = (got.double() - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print("%s: worst error / bound %.4f (max |err| %.3e, max |ref| %.3e)" % (what, worst, float(err.max()), float(want.abs().max())))
    assert torch.isfinite(got).all() and bool((err <= bound).all()), what
    return worst


def _within(got, want, bound):
    return bool(((got.double() - want).abs() <= bound).all())


# ------------------------------------------------------------------------------------------------ 1. the narrow kernels
def _block(name, q):
    from iip_uavsal_saliency_amd.model import dwBlock
    return NR.make_block(NR.NARROW[name], q, dwBlock).to(DEV)


@lru_cache(maxsize=None)
def _case(name, shape, gain=1.0, shift=0.0, zero_gamma=False):
    """the block, its fold, the teacher-forced fp32 tensors (go a slice between NaN columns) and the float64 closed form with
    bounds on exactly what the kernel reads; once per case"""
    xn, qn, gon = NR.narrow_case(name, shape, gain=gain, shift=shift, zero_gamma=zero_gamma)
    p = BR.fold(BR.to64(qn, DEV))
    pt = MP.block_parts(p, _d64(xn), _d64(gon), 1)
    n, H, W = shape
    wide = torch.full((n, H, W, 192), NAN, device=DEV)
    wide[..., 64:128] = _nhwc(gon)
    t = {"x": _nhwc(xn), "go": wide[..., 64:128], "e": _nhwc(pt["e"], True), "d": _nhwc(pt["d"], True), "gd": _nhwc(pt["gd"]),
         "ga": _nhwc(pt["ga"])}
    r = {k: _nchw64(v) for k, v in t.items()}                                            # what the kernel reads
    want, bound = NR.grads_from_parts(p, r["x"], r["e"], r["d"], r["gd"], r["ga"], r["go"], bounds=True)
    return _block(name, qn), p, want, bound, t, r


def _fenced(block):
    """a dict of gradient tensors that are the middle of NaN-filled buffers: `(out, buffers)`"""
    out, bufs = {}, {}
    for n, q in block.named_parameters():
        buf = torch.full((q.numel() + 64,), NAN, device=DEV)
        bufs[n] = buf
        out[n] = buf[32:32 + q.numel()].view(q.shape)
    return out, bufs


def _teacher(name, shape, *a, **kw):
    block, _, _, _, t, _ = _case(name, shape, *a)
    nchw = lambda v: v.permute(0, 3, 1, 2)                                                # noqa: E731
    return train.narrow_block_param_grads(block, nchw(t["x"]), t["e"], t["d"], nchw(t["go"]), gd=t["gd"], ga=t["ga"], **kw)


SLABS = {(1, 1, 1): 1, (1, 5, 7): 1, (2, 9, 13): 1, (1, 45, 80): 12, (3, 45, 80): 34}


@pytest.mark.parametrize("shape", NR.PICTURES, ids=lambda s: "n%d_%dx%d" % s)
@pytest.mark.parametrize("name", list(NR.NARROW))
def test_narrow_grads_teacher_forced_against_float64(name, shape):
    """One pixel; odd edges; (2,9,13): an image boundary inside the one slab; (1,45,80): the first shape with more than one slab
    (12 slabs of 4 rows, the last of 1); (3,45,80): 34 slabs, slabs that straddle an image boundary (45 is no multiple of 4) and
    a partial last slab of 3 rows.  Ch = 48 and 120 are no multiple of 64 (120 none of 16), Cin = 8 and 20 none of 32; (4, 4, 64) is the smallest block."""
    cin, hid, cout = NR.NARROW[name]
    n, H, W = shape
    block, p, want, bound, t, r = _case(name, shape)
    # the first launch alone, its workspace inside a NaN-filled buffer
    k = _lib.IrNarrowDesc()
    k.n_img, k.H, k.W, k.Cin, k.Ch, k.Co = n, H, W, cin, hid, cout
    lib = _lib.load()
    slabs, rows = int(lib.uavsal_ir_narrow_slabs(C.byref(k))), int(lib.uavsal_ir_narrow_slab_rows(C.byref(k)))
    assert (rows, slabs) == NR.slab_partition(n, H, W) and slabs == SLABS[shape]
    nd = slabs * NR.slab_doubles(cin, hid)
    assert int(lib.uavsal_ir_narrow_workspace_bytes(C.byref(k))) == 8 * nd
    buf = torch.full((nd + 32,), NAN, dtype=torch.float64, device=DEV)
    k.x, k.e, k.d, k.gd, k.ga = (t[v].data_ptr() for v in ("x", "e", "d", "gd", "ga"))
    k.go, k.ldgo = t["go"].data_ptr(), 192
    k.ws, k.ws_bytes = buf[16:].data_ptr(), 8 * nd
    _lib.check(lib.uavsal_ir_narrow_grads(C.byref(k), ops._stream(buf)), "uavsal_ir_narrow_grads")
    assert torch.isnan(buf[:16]).all() and torch.isnan(buf[16 + nd:]).all() and torch.isfinite(buf[16:16 + nd]).all()
    ws, slabs2 = train.ir_narrow_grads(t["x"], t["e"], t["d"], t["gd"], t["ga"], t["go"])
    assert slabs2 == slabs and torch.equal(ws.view(torch.int64), buf[16:16 + nd].view(torch.int64))      # two calls, the same bits
    dense, _ = train.ir_narrow_grads(t["x"], t["e"], t["d"], t["gd"], t["ga"], t["go"].contiguous())
    assert torch.equal(ws.view(torch.int64), dense.view(torch.int64))
    # both launches: every gradient inside NaN fences
    out, bufs = _fenced(block)
    got = _teacher(name, shape, out=out)
    for nme in BR.NAMES:
        _check(got[nme], want[nme], bound[nme], "narrow %s %r %s" % (name, shape, nme))
        b, q = bufs[nme], got[nme].numel()
        assert torch.isnan(b[:32]).all() and torch.isnan(b[32 + q:]).all()
    again = _teacher(name, shape)
    assert all(torch.equal(_bits(got[nme]), _bits(again[nme])) for nme in BR.NAMES)
    # accumulate: added to what is there, rounded once
    base = {nme: torch.full_like(v, 0.25) for nme, v in again.items()}
    acc = _teacher(name, shape, out={nme: v.clone() for nme, v in base.items()}, accumulate=True)
    for nme in BR.NAMES:
        _check(acc[nme], want[nme] + 0.25, bound[nme] + R.U * (want[nme] + 0.25).abs(), "  accumulate %s" % nme)
    # the wrong kernels are told apart
    told = []
    for v in NR.WRONG:
        if not NR.variant_applies(v, NR.NARROW[name], shape):
            continue
        wrong = NR.grads_from_parts(p, r["x"], r["e"], r["d"], r["gd"], r["ga"], r["go"], variant=v)
        assert any(not _within(got[nme], wrong[nme], bound[nme]) for nme in BR.NAMES), v
        told.append(v)
    print("rejected: %s" % ", ".join(told))


def test_narrow_variants_all_met():
    """every WRONG variant applies to (and is rejected at) one of the cases above"""
    met = {v for v in NR.WRONG for name in NR.NARROW for s in NR.PICTURES if NR.variant_applies(v, NR.NARROW[name], s)}
    assert met == set(NR.WRONG)


@pytest.mark.parametrize("name", ["gauss0", "ob0", "tiny"])
def test_zero_gamma_channels_have_a_gamma_gradient(name):
    shape = (2, 9, 13)
    block, p, want, bound, t, r = _case(name, shape, 1.0, 0.0, True)
    assert float(p["s1"][NR.ZERO[0]]) == 0.0 and float(p["s2"][NR.ZERO[1]]) == 0.0
    got = _teacher(name, shape, 1.0, 0.0, True)
    for nme in BR.NAMES:
        _check(got[nme], want[nme], bound[nme], "zero gamma %s %s" % (name, nme))
    assert float(got[BR.NAMES[1]][NR.ZERO[0]].abs()) > 0 and float(got[BR.NAMES[4]][NR.ZERO[1]].abs()) > 0
    assert float(got[BR.NAMES[0]][NR.ZERO[0]].abs().max()) == 0.0 and float(got[BR.NAMES[3]][NR.ZERO[1]].abs().max()) == 0.0


@pytest.mark.parametrize("name", ["gauss0", "ob0"])
def test_param_grads_of_a_saturated_narrow_block(name):
    """e and d under tests/saturate_bn.py's gain and shift for the prior nets' first expand: both clamps occur in both."""
    import saturate_bn
    shape = (2, 9, 13)
    block, p, want, bound, t, r = _case(name, shape, saturate_bn.GAIN, saturate_bn.SHIFT)
    got = _teacher(name, shape, saturate_bn.GAIN, saturate_bn.SHIFT)
    for nme in BR.NAMES:
        _check(got[nme], want[nme], bound[nme], "saturated %s %s" % (name, nme))
    for k in ("e", "d"):
        lo, mid, hi = BR.class_shares(r[k])
        print("saturated %s %s: shares at or below 0 / inside / at or above 6: %.3f %.3f %.3f" % (name, k, lo, mid, hi))
        assert hi >= 0.05 and mid >= 0.05


def test_default_gd_and_ga_come_from_the_device():
    """gd from the 64 -> Ch GEMM the conv route takes, ga from uavsal_ir_bwd with C = 48 / 120: within the bounds of
    block_ref64.block_e2e's gd and ga stages carried to the gradients is more than this needs -- the teacher-forced result is
    the reference, at 1e-4 of each tensor's largest element (a plumbing check)."""
    for name in ("gauss0", "ob0"):
        shape = (2, 9, 13)
        block, p, want, bound, t, r = _case(name, shape)
        nchw = lambda v: v.permute(0, 3, 1, 2)                                            # noqa: E731
        got = train.narrow_block_param_grads(block, nchw(t["x"]), t["e"], t["d"], nchw(t["go"]))
        for nme in BR.NAMES:
            err = float((got[nme].double() - want[nme]).abs().max())
            assert err <= 1e-4 * float(want[nme].abs().max()) + 1e-30, (name, nme, err)


def test_narrow_refusals_by_name():
    from iip_uavsal_saliency_amd.model import dwBlock
    z = torch.zeros(1, 64, 3, 3, device=DEV)
    for blk, what in ((dwBlock(64, 64), "Cin"), (dwBlock(8, 64, stride=2), "stride 1"), (dwBlock(8, 32), "Cout == 64")):
        with pytest.raises(RuntimeError, match="narrow_block_param_grads"):
            train.narrow_block_param_grads(blk.to(DEV).eval(), z, z, z, z)
    with pytest.raises(RuntimeError, match="model.eval"):
        train.narrow_block_param_grads(dwBlock(8, 64).to(DEV).train(), z, z, z, z)
    t = torch.zeros(1, 3, 3, 132, device=DEV)
    with pytest.raises(RuntimeError, match="ESHAPE|shape|rejected"):
        train.ir_narrow_grads(torch.zeros(1, 3, 3, 8, device=DEV), t, t, t, t, torch.zeros(1, 3, 3, 64, device=DEV))


@pytest.mark.parametrize("N", [1, 2, 5])
def test_frame_sum(N):
    gen = torch.Generator(DEV).manual_seed(N)
    wide = torch.full((N, 5, 7, 192), NAN, device=DEV)
    wide[..., 64:128] = torch.randn(N, 5, 7, 64, device=DEV, generator=gen)
    wide[0, 0, 0, 64] = -0.0
    a = wide[..., 64:128]
    got = train.frame_sum(a)
    assert tuple(got.shape) == (1, 5, 7, 64)
    want, bound = NR.frame_sum_ref(a.double())
    _check(got, want, bound, "frame_sum N=%d" % N)
    assert torch.equal(_bits(got), _bits(train.frame_sum(a)))
    if N == 1:
        assert torch.equal(_bits(got), _bits(a))
    else:
        assert not _within(got, a[:-1].double().sum(0, keepdim=True), bound)             # a kernel that stops one frame short


# ------------------------------------------------------------------------------------------------ 2. a whole net
@pytest.mark.parametrize("shape", [(1, 5, 7), (4, 5, 7), (1, 45, 80), (4, 45, 80)], ids=lambda s: "n%d_%dx%d" % s)
@pytest.mark.parametrize("net", list(NR.NETS))
def test_prior_net_backward_stage_by_stage(net, shape):
    """Each block's nine gradients against float64 fed the tensors the walk handed it (mp_ref64's bounds for block 1,
    nets_ref64's for block 0), and the walk's own stages against the float64 ones."""
    from iip_uavsal_saliency_amd.model import dwBlock
    cbn, qs, gon = NR.net_case(net, shape)
    m = NR.make_net(net, qs, dwBlock).to(DEV)
    n, H, W = shape
    wide = torch.full((n, H, W, 192), NAN, device=DEV)
    wide[..., 64:128] = _nhwc(gon)
    cb = torch.as_tensor(cbn).to(DEV)
    parts = {}
    got = train.prior_net_backward(m, cb, wide[..., 64:128], parts=parts)
    assert sorted(got) == ["0", "1"] and all(sorted(got[k]) == sorted(BR.NAMES) for k in got)
    for k, blk in (("1", m[1]), ("0", m[0])):
        p = X.fold_module(blk)
        pt = parts[k]
        xx, go, e, d, gd, ga = (_nchw64(pt[v]) for v in ("x", "go", "e", "d", "gd", "ga"))
        if k == "1":
            want, bound = MP.grads_from_parts(p, xx, e, d, gd, ga, go, 1, bounds=True)
        else:
            want, bound = NR.grads_from_parts(p, xx, e, d, gd, ga, go, bounds=True)
        for nme in BR.NAMES:
            # (the device's folds s = gamma r and r are the float64 ones rounded once: U on every tensor they scale, twice)
            _check(got[k][nme], want[nme], bound[nme] + 2 * R.U * want[nme].abs(), "%s %r block %s %s" % (net, shape, k, nme))
    # the walk is the float64 one at a plumbing check's 1e-3 of each tensor's norm
    P = [X.fold_module(m[0]), X.fold_module(m[1])]
    ref = NR.net_param_grads(P, cb.double(), _d64(gon))
    for k in got:
        for nme in BR.NAMES:
            rel = float((got[k][nme].double() - ref[k][nme]).norm() / ref[k][nme].norm().clamp_min(1e-300))
            assert rel <= 1e-3, (k, nme, rel)
    again = train.prior_net_backward(m, cb, wide[..., 64:128])
    assert all(torch.equal(_bits(got[k][nme]), _bits(again[k][nme])) for k in got for nme in BR.NAMES)
    assert all(q.grad is None for q in m.parameters())


# ------------------------------------------------------------------------------------------------ 3. the step and the driver
H_, W_, T_ = 72, 104, 4
RNN = "rnn.cell_list.0.rnn_conv.weight"
BIAS = {"all": [1, 1, 1], "no_context": [1, 1, 0], "gauss": [1, 0, 0], "ob_context": [0, 1, 1]}


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


def _names(box, i=0):
    return ["%s.%d.%s" % (box, i, n) for n in BR.NAMES]


def _net_names(m):
    return [n for box in train.prior_nets(m) for i in (0, 1) for n in _names(box, i)]


def _other_names(m):
    names = [RNN] + ["conv_out_st." + n for n in BR.NAMES] + _names("fucbst_layer") + _names("fust_layer") + _names("fucb_layer")
    if m.use_context_prior:
        names += _names("cxt_cb_prior", 1) + _names("cxt_cb_prior", 0)
    return names


def _model(kind="all"):
    from iip_uavsal_saliency_amd import UAVSal
    m = UAVSal(time_dims=T_, bias_type=BIAS[kind])
    synth.load_synth_weights(m, 0)
    with torch.no_grad():                                       # running statistics that are not the initial 0 and 1
        g = torch.Generator().manual_seed(11)
        blocks = [m.conv_out_st, m.fucbst_layer[0], m.fust_layer[0], m.fucb_layer[0]] + (list(m.cxt_cb_prior) if BIAS[kind][2] else [])
        for net in train.prior_nets(m).values():
            blocks += list(net)
        for blk in blocks:
            for bn in (blk.conv[0][1], blk.conv[1][1], blk.conv[3]):
                bn.running_mean.add_(0.05 * torch.randn(bn.running_mean.shape, generator=g))
                bn.running_var.mul_(1.0 + 0.2 * torch.rand(bn.running_var.shape, generator=g))
    return m.to(DEV).eval()


def _stats(m):
    return [b.detach().clone() for b in m.buffers()]


def _grads(m, names):
    params = dict(m.named_parameters())
    return {k: params[k].grad.clone() for k in names}


def _has_grad(m):
    return sorted(n for n, p in m.named_parameters() if p.grad is not None)


def _all_mods(m):
    mods = [m.rnn, m.conv_out_st, m.fucbst_layer, m.fust_layer, m.fucb_layer] + ([m.cxt_cb_prior] if m.use_context_prior else [])
    return mods + list(train.prior_nets(m).values())


ALL = dict(decoder=True, fuse=True, fust=True, ctx=True)


@pytest.mark.parametrize("kind", list(BIAS))
def test_recurrence_step_with_nets(kind):
    """THE test that fails without the feature: the parent knows no `nets`."""
    m = _model(kind)
    x, cb, y = _step_inputs()
    nets = _net_names(m)
    assert len(nets) == 18 * (BIAS[kind][0] + BIAS[kind][1])
    others = _other_names(m)
    stats = _stats(m)
    loss, out, st = train.recurrence_step(m, x, cb, None, y, nets=True, **ALL)
    ref_out, ref_st = m(x, cb, None)
    assert torch.equal(out, ref_out) and torch.equal(st[0], ref_st[0]) and loss.item() == losses.loss_fu(ref_out, y).item()
    assert _has_grad(m) == sorted(others + nets)
    # with every stage on, the step has set the gradient of every parameter the reference's optimiser holds
    frozen = [n for n, _ in m.named_parameters() if n.startswith(("sfnet.", "st_layer."))]
    assert sorted(frozen + others + nets) == sorted(n for n, _ in m.named_parameters())
    g1 = _grads(m, others + nets)
    assert all(torch.isfinite(v).all() and float(v.abs().max()) > 0 and v.is_contiguous() for v in g1.values())
    assert all(torch.equal(a, b) for a, b in zip(stats, _stats(m)))
    # every other stage's gradients are those of a step without nets, bit for bit -- with the other stages and without them
    plain = _model(kind)
    train.recurrence_step(plain, x, cb, None, y, **ALL)
    assert _has_grad(plain) == sorted(others)
    g0 = _grads(plain, others)
    assert all(torch.equal(g0[n], g1[n]) for n in g0)
    lone = _model(kind)
    train.recurrence_step(lone, x, cb, None, y, decoder=True, fuse=True, nets=True)
    dec = ["conv_out_st." + n for n in BR.NAMES]
    assert _has_grad(lone) == sorted([RNN] + dec + _names("fucbst_layer") + nets)
    gl = _grads(lone, [RNN] + dec + _names("fucbst_layer") + nets)
    assert all(torch.equal(gl[n], g1[n]) for n in gl)
    # .grad += as loss.backward() would
    train.recurrence_step(m, x, cb, None, y, nets=True, **ALL)
    params = dict(m.named_parameters())
    for n in nets:
        _check(params[n].grad, 2 * g1[n].double(), 4 * R.U * g1[n].double().abs(), "second call doubles %s" % n)
    # the directional derivative along the normalised gradient of the nets' 18 / 36 tensors against the central difference of
    # the GPU forward (the plumbing check of tests/test_train_ctx_gpu.py, with its 10 % and for its reason); the refresh is in
    # place -- the engines stay the objects they were -- and drops the prior record: the SAME prior tensors give new maps
    engines = {k: id(e) for k, e in m._engines.items()}
    mods = list(train.prior_nets(m).values())
    with torch.no_grad():
        norm = float(torch.sqrt(sum((g1[n].double() ** 2).sum() for n in nets)))
        w0 = {n: params[n].detach().clone() for n in nets}
        s = 2e-2 / norm
        vals = []
        for sign in (1.0, -1.0):
            for n in nets:
                params[n].copy_(w0[n] + sign * s * g1[n] / norm)
            assert m.refresh_weights(*mods) > 0
            vals.append(losses.loss_fu(m(x, cb, None)[0], y).item())
        for n in nets:
            params[n].copy_(w0[n])
        assert m.refresh_weights(*mods) > 0
    fd = (vals[0] - vals[1]) / (2 * s)
    print("%s: nets directional derivative: finite difference %.6e, <grad, D> %.6e, step %.3e" % (kind, fd, norm, s))
    assert vals[0] != vals[1] and abs(fd - norm) <= 0.10 * abs(norm)
    assert torch.equal(m(x, cb, None)[0], ref_out)                                # the restored weights give the same bits
    assert {k: id(e) for k, e in m._engines.items()} == engines


def test_nets_needs_a_prior_net_and_fuse():
    from iip_uavsal_saliency_amd import UAVSal
    x, cb, y = _step_inputs()
    m = UAVSal(time_dims=T_, bias_type=[0, 0, 1])
    synth.load_synth_weights(m, 0)
    m = m.to(DEV).eval()
    with pytest.raises(RuntimeError, match="nets=True"):
        train.recurrence_step(m, x, cb, None, y, fuse=True, nets=True)
    with pytest.raises(RuntimeError, match="nets=True"):
        train.recurrence_step(_model("all"), x, cb, None, y, nets=True)
    assert train.prior_nets(m) == {} and list(train.prior_nets(_model("ob_context"))) == ["ob_cb_layer"]


def test_static_priors_give_the_gradients_of_materialised_ones():
    """Frame-invariant priors as zero-stride views run each net on ONE frame: the step sums the net's slice of g_cb over the
    frames and walks back on one frame.  Against materialised copies (N frames, N-frame backward) the 36 gradients agree within
    the float64 form's own statement of the two orders of summation -- not bit for bit: 1e-3 of each tensor's norm, the
    plumbing bound of tests/test_train_ctx_gpu.py's static test, for its reason (the one-frame launches may pick other tiles)."""
    x, cb, y = _step_inputs()
    n = x.shape[0]
    view = [c[:1].expand(n, -1, -1, -1) for c in cb]
    mat = [c[:1].repeat(n, 1, 1, 1) for c in cb]
    ms, mm = _model(), _model()
    names = _net_names(ms)
    train.recurrence_step(ms, x, view, None, y, fuse=True, nets=True)
    train.recurrence_step(mm, x, mat, None, y, fuse=True, nets=True)
    assert {e.static_priors for e in ms._engines.values() if e.keep_taps} == {True}
    assert {e.static_priors for e in mm._engines.values() if e.keep_taps} == {False}
    gs, gm = _grads(ms, names), _grads(mm, names)
    for k in names:
        assert torch.isfinite(gs[k]).all() and float(gs[k].abs().max()) > 0
        rel = float((gs[k].double() - gm[k].double()).norm() / gm[k].double().norm())
        print("static vs materialised priors %s: ||difference|| / ||gradient|| %.3e" % (k, rel))
        assert rel <= 1e-3, k


def _trained(m):
    return [p for mod in _all_mods(m) for p in mod.parameters()]


@pytest.mark.parametrize("static", [True, False], ids=["static", "per_frame"])
def test_adam_steps_over_six_stages_keep_the_plans(static):
    """`cache_priors` on and the SAME prior tensor objects in every call: the forward after a step must not serve cb192 from
    the old weights (the prior record is dropped by the refresh), and no packed form of the four blocks may be missed."""
    from iip_uavsal_saliency_amd import UAVSal
    m = _model("all")
    assert m.cache_priors
    x, cb, y = _step_inputs()
    if static:
        cb = [c[:1].expand(x.shape[0], -1, -1, -1) for c in cb]
    stats = _stats(m)
    opt = torch.optim.Adam(_trained(m), lr=1e-4, betas=(0.9, 0.999), weight_decay=5e-5)
    before = m(x, cb, None)[0]
    first = None
    for _ in range(3):
        opt.zero_grad()
        loss, _, _ = train.recurrence_step(m, x, cb, None, y, nets=True, **ALL)
        first = loss.item() if first is None else first
        engines = dict(m._engines)
        opt.step()
        assert m.refresh_weights(*_all_mods(m)) > 0
        after = m(x, cb, None)[0]
        assert {k: id(e) for k, e in m._engines.items()} == {k: id(e) for k, e in engines.items()}      # no plan is rebuilt
    assert {e.static_priors for e in m._engines.values()} == {static}
    last = losses.loss_fu(after, y).item()
    print("static=%s: loss_fu on the group: %.6f before, %.6f after three Adam steps over six stages" % (static, first, last))
    assert last < first and not torch.equal(before, after)
    assert all(torch.equal(a, b) for a, b in zip(stats, _stats(m)))                # running statistics unchanged
    w0 = _model("all")
    for box in train.prior_nets(m):                                                # ... and the nets did move
        for i in (0, 1):
            assert not torch.equal(getattr(m, box)[i].conv[0][0].weight.detach(), getattr(w0, box)[i].conv[0][0].weight.detach())
    fresh = UAVSal(time_dims=T_, bias_type=BIAS["all"])
    fresh.load_state_dict(m.state_dict())
    fresh = fresh.to(DEV).eval()
    taps, ftaps = {"cb192": None}, {"cb192": None}
    got, got_st = m(x, cb, None, taps=taps)
    want, want_st = fresh(x, cb, None, taps=ftaps)
    assert torch.equal(taps["cb192"], ftaps["cb192"])
    assert torch.equal(got, want) and torch.equal(got_st[0], want_st[0])           # bit for bit the repacked weights
    got2, _ = m(x, cb, None)                                                       # ... and on the plan without taps, from its cache
    want2, _ = fresh(x, cb, None)
    assert torch.equal(got2, want2)


def test_refresh_of_another_stage_keeps_the_prior_record():
    m = _model("all")
    x, cb, y = _step_inputs()
    m(x, cb, None)
    eng = next(iter(m._engines.values()))
    assert eng._prior_rec is not None
    with torch.no_grad():
        m.rnn.cell_list[0].rnn_conv.weight.mul_(1.0)
    assert m.refresh_weights(m.rnn) > 0 and eng._prior_rec is not None
    with torch.no_grad():
        m.gauss_cb_layer[1].conv[2].weight.mul_(1.0)
    assert m.refresh_weights(m.gauss_cb_layer) > 0 and eng._prior_rec is None


def test_finetune_video_with_six_stages_is_the_manual_loop():
    from iip_uavsal_saliency_amd.stream import finetune_video
    n = 2 * T_ * 2
    frames = torch.from_numpy(synth.synth_frames_u8(n, H_, W_, 2)).to(DEV)
    gp = torch.from_numpy(synth.gauss_priors(1, H_ // 8, W_ // 8)[0]).to(DEV)
    op_ = torch.from_numpy(synth.ob_priors(1, H_ // 8, W_ // 8)[0]).to(DEV)
    loc = synth.synth_fix_points(n, 90, 130, 12, 9)
    fmap = np.rint(synth.synth_fix_maps(loc, 6.0) * 255).astype(np.uint8)
    fix_map, fix_loc = torch.from_numpy(fmap).to(DEV), torch.from_numpy(loc).to(DEV)
    stages = ("rnn", "decoder", "fuse", "fust", "ctx", "nets")
    kw = {s: True for s in stages[1:]}

    def make():
        m = _model()
        return m, torch.optim.Adam(_trained(m), lr=1e-4, betas=(0.9, 0.999), weight_decay=5e-5)
    m, opt = make()
    seen = []
    real = train.recurrence_step

    def spy(model, x, cb, state, y, criterion, **k):
        assert k == kw
        seen.append((x.clone(), cb, y.clone()))                                    # (cb: the zero-stride views themselves)
        return real(model, x, cb, state, y, criterion, **k)
    train.recurrence_step = spy
    try:
        res = finetune_video(m, frames, gp, op_, fix_map, fix_loc, opt, batch_size=2, stages=stages)
    finally:
        train.recurrence_step = real
    assert res["groups_run"] == 2 and len(seen) == 2
    m2, opt2 = make()
    state, manual = None, []
    for x, cb, y in seen:
        opt2.zero_grad()
        loss, _, state = train.recurrence_step(m2, x, cb, state, y, **kw)
        opt2.step()
        m2.refresh_weights(*_all_mods(m2))
        manual.append(loss.item())
    assert [float(v) for v in res["losses"].tolist()] == manual
    for (k, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    w0 = _model()
    for box in ("gauss_cb_layer", "ob_cb_layer"):
        assert not torch.equal(getattr(m, box)[0].conv[0][0].weight.detach(), getattr(w0, box)[0].conv[0][0].weight.detach())
    # (stage tuples: "nets" last of all, behind "fuse", with or without "fust" / "ctx")
    for ok in (("rnn", "fuse", "nets"), ("rnn", "decoder", "fuse", "fust", "nets"), ("rnn", "fuse", "ctx", "nets")):
        kw2 = {}

        def probe(model, x, cb, state, y, criterion, **k):
            kw2.update(k)
            raise StopIteration
        train.recurrence_step = probe
        try:
            with pytest.raises(StopIteration):
                finetune_video(m, frames, gp, op_, fix_map, fix_loc, opt, batch_size=2, stages=ok)
        finally:
            train.recurrence_step = real
        assert kw2 == {s: True for s in ok[1:]}
    for bad in (("rnn", "nets"), ("rnn", "fuse", "nets", "ctx"), ("rnn", "decoder", "nets")):
        with pytest.raises(ValueError):
            finetune_video(m, frames, gp, op_, fix_map, fix_loc, opt, batch_size=2, stages=bad)
