"""The backward of a general inverted-residual block on the GPU (train.block_param_grads / block_backward /
recurrence_step(fuse=True), csrc/train_block.hip, and the N tail of uavsal_pix_gemm) against the float64 closed form
tests/block_ref64.py, which runs on the device in torch float64, and the reference's recorded autograd results
(tests/golden/block_*.npz).  Bounds: block_ref64's docstring.
The kernels are tested teacher-forced: e, d, gd, ga are the float64 restatement's, rounded to fp32 (`teacher_round` for e
and d: the stored value decides every mask as the float64 one does).
Configurations: "fucbst" (320 -> 1920 -> 256, no residual: an N tail of 64 columns in the W1 and W3 GEMMs, a last channel
group of 128) and "fust" (256 -> 1536 -> 256, with the residual).  Shapes (T, H, W): train_ref64.SHAPES -- (2,45,80) is the
slab shape: 13 slabs of 7 picture rows, the last one 6 rows, one slab across both frames -- and, for the pixel GEMM alone,
(7,45,80): 13 shares of 2 chunks for 1920 x 320, the last one a single chunk of 624 pixels."""
import os
from functools import lru_cache

import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import losses, ops, synth, train
from iip_uavsal_saliency_amd.weights import WeightCache

import block_ref64 as BR
import decoder_ref64 as DR
import train_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(c, s) for c in BR.CFGS for s in BR.SHAPES]
SMALL = [(c, s) for c in BR.CFGS for s in BR.GOLDEN_SHAPES]
W1, W3 = BR.NAMES[0], BR.NAMES[6]


def _id(cs):
    return BR.name(*cs)


def _cl(a):
    return torch.as_tensor(a).to(DEV).float().contiguous(memory_format=torch.channels_last)


def _dense_nhwc(t64, keep_masks=False):
    """a float64 NCHW tensor as the dense fp32 NHWC tensor the kernels read"""
    t32 = BR.teacher_round(t64) if keep_masks else t64.float()
    return t32.permute(0, 2, 3, 1).contiguous()


def _check(got, want, bound, what):
    err = (got.double() - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print("%s: worst error / bound %.4f (max |err| %.3e, max |ref| %.3e)" % (what, worst, float(err.max()), float(want.abs().max())))
    assert torch.isfinite(got).all() and bool((err <= bound).all()), what
    return worst


def _block(cfg, q):
    from iip_uavsal_saliency_amd.model import dwBlock
    c = BR.CFG[cfg]
    blk = BR.load_block(dwBlock(c["cin"], c["cout"], kernel_size=3), q).to(DEV)
    assert bool(blk.use_res_connect) == c["res"]
    return blk


@lru_cache(maxsize=None)
def _case(cfg, shape, zero_gamma=False):
    """the block, its float64 numbers, inputs, the closed form with bounds, and the teacher-forced fp32 tensors; once per case"""
    xn, qn, gon = BR.block_case(cfg, shape, zero_gamma)
    x, q, go = torch.as_tensor(xn).to(DEV).double(), BR.to64(qn, DEV), torch.as_tensor(gon).to(DEV).double()
    parts = {}
    want, bound = BR.param_grads(q, x, go, bounds=True, parts=parts)
    t = {"x": _cl(xn), "go": _cl(gon), "e": _dense_nhwc(parts["e"], True), "d": _dense_nhwc(parts["d"], True),
         "gd": _dense_nhwc(parts["gd"]), "ga": _dense_nhwc(parts["ga"])}
    keep = {k: parts[k] for k in ("e", "d", "gd", "ga")}
    return _block(cfg, qn), q, x, go, want, bound, t, keep


def _teacher_grads(cfg, shape, zero_gamma=False, **kw):
    block, _, _, _, _, _, t, _ = _case(cfg, shape, zero_gamma)
    return train.block_param_grads(block, t["x"], t["e"], t["d"], t["go"], gd=t["gd"], ga=t["ga"], **kw)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. the pixel GEMM's N tail
SPLIT_SHAPE = (7, 45, 80)


@lru_cache(maxsize=None)
def _gemm_ops(shape):
    if shape == SPLIT_SHAPE:
        a, b = (torch.as_tensor(v).to(DEV) for v in BR.gemm_inputs(shape, 1920, 320))
    else:
        t = _case("fucbst", shape)[6]
        a, b = t["ga"], t["x"].permute(0, 2, 3, 1)
    return (a, b) + BR.pix_gemm_ref(a.double(), b.double())


@pytest.mark.parametrize("shape", BR.SHAPES + [SPLIT_SHAPE], ids=lambda s: "T%d_%dx%d" % s)
def test_pix_gemm_n_tail_against_float64(shape):
    """M = 1920, N = 320: two whole N tiles and half a tile."""
    a, b, want, bound = _gemm_ops(shape)
    M, N = a.shape[3], b.shape[3]
    assert (M, N) == (1920, 320)
    got = train.pix_gemm(a, b)
    _check(got, want, bound, "T%d_%dx%d pix_gemm 1920 x 320" % shape)
    assert torch.equal(_bits(got), _bits(train.pix_gemm(a, b)))                   # two calls, the same bits
    # nothing at or behind column N is read: the slice of a 384-wide tensor whose last 64 columns are NaN gives the dense bits
    wide = torch.full(b.shape[:3] + (384,), float("nan"), device=DEV)
    wide[..., :N] = b
    assert torch.equal(_bits(got), _bits(train.pix_gemm(a, wide[..., :N])))
    # row_scale, rowdot and accumulate: out = fl(old + rs G), rowdot = sum_n w G in double
    rs = torch.linspace(-2.0, 2.0, M, device=DEV)
    w = torch.randn(M, N, device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    old = torch.randn(M, N, device=DEV, generator=torch.Generator(DEV).manual_seed(6)) * float(want.abs().max())
    out, rowdot = old.clone(), torch.empty(M, dtype=torch.float64, device=DEV)
    train.pix_gemm(a, b, out=out, row_scale=rs, w=w, rowdot=rowdot, accumulate=True)
    exp = old.double() + rs.double().view(-1, 1) * want
    _check(out, exp, rs.double().abs().view(-1, 1) * bound + R.EPS * (old.double().abs() + exp.abs()), "  + row_scale, accumulate")
    _check(rowdot, (w.double() * want).sum(1), (w.double().abs() * bound).sum(1), "  rowdot")
    if shape == SPLIT_SHAPE:
        # the split is real here: a kernel that drops the last share is rejected by the bound the right one passes
        from iip_uavsal_saliency_amd import _lib
        import ctypes as C
        K = a.shape[0] * a.shape[1] * a.shape[2]
        assert shape[0] == BR.gemm_split_frames(M, N)
        cps, shares, spans = BR.gemm_partition(K, M, N)
        assert (cps, shares, spans[-1][1] - spans[-1][0]) == (2, 13, 624)
        d = _lib.PixGemmDesc()
        d.K, d.M, d.N = K, M, N
        assert _lib.load().uavsal_pix_gemm_shares(C.byref(d)) == shares
        p0 = spans[-1][0]
        A, B = a.reshape(-1, M).double(), b.reshape(-1, N).double()
        wrong = A[:p0].T @ B[:p0]
        assert float(((wrong - want).abs() / bound).max()) >= 4.0
        assert not bool(((got.double() - wrong).abs() <= bound).all())
        tail = want.clone()
        tail[:, 256:] = 0                                                          # ... and one that drops the N tail
        assert not bool(((got.double() - tail).abs() <= bound).all())


def test_pix_gemm_keeps_the_bits_of_the_shapes_it_took_before(golden_dir):
    """M and N multiples of 128 return the bytes the kernel returned before it learnt the N tail: tests/golden/pix_gemm_bits.json
    holds the hashes of its results on the decoder tests' seeded GEMM operands (`decoder_ref64.gemm_inputs`), recorded with
    the library built from the commit in front of the tail, for 1536 x 256 and 256 x 1536 at every shape of the decoder's
    GEMM test -- (12,45,80) with its 22 shares of 2 chunks among them."""
    import hashlib
    import json
    with open(os.path.join(golden_dir, "pix_gemm_bits.json")) as f:
        rec = json.load(f)["shapes"]
    assert sorted(rec) == sorted("%dx%dx%d" % s for s in DR.SHAPES + [DR.GEMM_SPLIT_SHAPE])
    for shape in DR.SHAPES + [DR.GEMM_SPLIT_SHAPE]:
        a, b = (torch.as_tensor(v).to(DEV) for v in DR.gemm_inputs(shape))
        got = [hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for t in (train.pix_gemm(a, b), train.pix_gemm(b, a))]
        assert got == rec["%dx%dx%d" % shape], shape


def test_pix_gemm_whole_tiles_do_not_depend_on_the_tail():
    """The decoder's test operands (1536 x 256, K = 7200: 8 shares of one chunk with 24 tiles and with 36) keep their bits
    when 64 more columns follow them: the tail changes nothing in a whole tile.  M = 400 is still refused."""
    hn, qn, gyn = DR.decoder_case((2, 45, 80))
    rs = np.random.RandomState(17)
    a = torch.as_tensor((1e-2 * rs.standard_normal((2, 45, 80, 1536))).astype(np.float32)).to(DEV)
    b = _cl(hn).permute(0, 2, 3, 1)
    assert DR.gemm_partition(7200)[:2] == BR.gemm_partition(7200, 1536, 320)[:2] == (1, 8)
    dense = train.pix_gemm(a, b)
    want, bound = BR.pix_gemm_ref(a.double(), b.double())
    _check(dense, want, bound, "1536 x 256")
    wide = torch.randn(2, 45, 80, 320, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    wide[..., :256] = b
    got = train.pix_gemm(a, wide)
    assert torch.equal(_bits(got[:, :256]), _bits(dense))
    with pytest.raises(RuntimeError, match="ESHAPE|shape|rejected"):
        train.pix_gemm(a[..., :400], b)
    with pytest.raises(RuntimeError, match="ESHAPE|shape|rejected"):
        train.pix_gemm(a, wide[..., :288])


# ------------------------------------------------------------------------------------------------ 2. uavsal_ir_bwd
@pytest.mark.parametrize("cs", CASES, ids=_id)
def test_ir_bwd_teacher_forced_against_float64(cs):
    cfg, shape = cs
    block, q, _, _, _, _, t, keep = _case(cfg, shape)
    _, _, dwc, dwbn, _, _ = train._block_parts(block)
    w9, s2, _ = WeightCache(DEV, {}).depthwise(dwc, dwbn)
    got = train.ir_bwd(t["gd"], t["d"], t["e"], w9, s2)
    p = BR.fold(q)
    bound = BR.ir_bwd_bound(p, keep["gd"], keep["d"], keep["e"])
    _check(got.permute(0, 3, 1, 2), keep["ga"], bound, "%s uavsal_ir_bwd" % BR.name(cfg, shape))
    assert torch.equal(_bits(got), _bits(train.ir_bwd(t["gd"], t["d"], t["e"], w9, s2)))
    for v in ("taps_flipped", "halo_across_frames", "nonstrict_masks"):             # the wrong kernels are told apart
        if v != "halo_across_frames" or shape[0] > 1:
            wrong = BR.ir_bwd_ref(p, keep["gd"], keep["d"], keep["e"], variant=v)
            assert not bool(((got.permute(0, 3, 1, 2).double() - wrong).abs() <= bound).all()), v


# ------------------------------------------------------------------------------------------------ 3. sums + finalise
@pytest.mark.parametrize("cs", CASES, ids=_id)
def test_param_grads_teacher_forced_against_float64(cs):
    """Per tensor against the float64 closed form.  (2,45,80) is the slab shape: 13 slabs, a partial last one."""
    cfg, shape = cs
    want, bound = _case(cfg, shape)[4:6]
    got = _teacher_grads(cfg, shape)
    assert tuple(got) == BR.NAMES
    for n in BR.NAMES:
        assert got[n].shape == want[n].shape and got[n].dtype == torch.float32
        _check(got[n], want[n], bound[n], "%s %s" % (BR.name(cfg, shape), n))
    again = _teacher_grads(cfg, shape)
    assert all(torch.equal(_bits(got[n]), _bits(again[n])) for n in BR.NAMES)      # two calls, the same bits
    # out= / accumulate=: added to what is there, rounded once
    old = {n: torch.full_like(got[n], 0.25) * float(want[n].abs().max()) for n in BR.NAMES}
    acc = {n: v.clone() for n, v in old.items()}
    assert _teacher_grads(cfg, shape, out=acc, accumulate=True) is acc
    for n in BR.NAMES:
        exp = old[n].double() + want[n]
        _check(acc[n], exp, bound[n] + R.EPS * (old[n].double().abs() + exp.abs()), "  accumulate %s" % n)
    if shape == BR.SLAB_SHAPE:
        assert BR.slab_partition(*shape) == (7, 13)
    # the wrong kernels of the tails are told apart by the bound
    _, q, x, go = _case(cfg, shape)[:4]
    for v in ("n_tail", "group_tail"):
        if BR.CFG[cfg]["hid"] % 256:
            wrong = BR.param_grads(q, x, go, variant=v)
            assert any(not bool(((got[n].double() - wrong[n]).abs() <= bound[n]).all()) for n in BR.NAMES), v


def test_param_grads_default_gd_and_ga_come_from_the_device():
    """Without `gd` / `ga` the function forms them by one GEMM (the projection's transposed weights with s3 in their rows) and
    one uavsal_ir_bwd: the same bits as the call that is handed those two tensors.  That gd is within the GEMM's bound of the
    float64 one (a sum of 256 products, + U for the product s3 W3 rounded once in the packed weights), and that ga within
    uavsal_ir_bwd's own bound plus gd's error carried through its absolute-value chain."""
    from iip_uavsal_saliency_amd import _lib
    cfg, shape = "fucbst", (5, 12, 20)
    block, q, x, go, want, bound, t, keep = _case(cfg, shape)
    _, _, dwc, dwbn, pl, plbn = train._block_parts(block)
    cache = WeightCache(DEV, {})
    gd = train._conv(_lib.load(), cache, t["go"].permute(0, 2, 3, 1), pl, BR.CFG[cfg]["hid"], 1, tscale=plbn)
    ga = train.ir_bwd(gd, t["d"], t["e"], *cache.depthwise(dwc, dwbn)[:2])
    p = BR.fold(q)
    gd_abs = torch.nn.functional.conv_transpose2d(go.abs() * p["s3"].abs().view(1, -1, 1, 1), p["w3"].abs())
    gd_err = (R.rtol("f32", 256) + R.U) * gd_abs + R.EPS * 2 * keep["gd"].abs()
    _check(gd.permute(0, 3, 1, 2), keep["gd"], gd_err, "gd from the device")
    ga_err = (R.LAMBDA * 3 + 2) * R.U * BR.ir_bwd_ref(p, keep["gd"], keep["d"], keep["e"], absolute=True) \
        + BR.ir_bwd_ref(p, gd_err, keep["d"], keep["e"], absolute=True)
    _check(ga.permute(0, 3, 1, 2), keep["ga"], ga_err, "ga from the device")
    got = train.block_param_grads(block, t["x"], t["e"], t["d"], t["go"])
    ref = train.block_param_grads(block, t["x"], t["e"], t["d"], t["go"], gd=gd, ga=ga)
    for n in BR.NAMES:
        assert torch.equal(_bits(got[n]), _bits(ref[n])), n
    for n in BR.NAMES[6:]:                                                          # W3, gamma3, beta3 read neither
        assert torch.equal(_bits(got[n]), _bits(_teacher_grads(cfg, shape)[n])), n


@pytest.mark.parametrize("cfg", BR.CFGS)
def test_zero_gamma_channels_have_a_gamma_gradient(cfg):
    shape = (3, 5, 7)
    want, bound = _case(cfg, shape, True)[4:6]
    got = _teacher_grads(cfg, shape, True)
    for n in BR.NAMES:
        _check(got[n], want[n], bound[n], "zero gamma %s" % n)
    c1, c2 = BR.ZERO_GAMMA
    assert float(got[BR.NAMES[0]][c1].abs().max()) == 0 and float(got[BR.NAMES[3]][c2].abs().max()) == 0
    for n, c in ((BR.NAMES[1], c1), (BR.NAMES[4], c2)):
        assert float(got[n][c].abs()) > 0 and float((got[n][c].double() - want[n][c]).abs()) <= float(bound[n][c])


@pytest.mark.parametrize("cfg", BR.CFGS)
def test_zero_grad_out_gives_positive_zeros(cfg):
    shape = (3, 5, 7)
    block, _, _, _, _, _, t, _ = _case(cfg, shape)
    z = torch.zeros_like(t["go"])
    got = train.block_param_grads(block, t["x"], t["e"], t["d"], z)                 # gd and ga from the device: zeros too
    for n in BR.NAMES:
        assert int(_bits(got[n]).abs().max()) == 0, n                               # +0.0: no sign bit either


@pytest.mark.parametrize("cs", SMALL, ids=_id)
def test_param_grads_against_the_reference(cs, golden_dir):
    cfg, shape = cs
    g = np.load(os.path.join(golden_dir, BR.name(cfg, shape) + ".npz"))
    xn, qn, gon = BR.block_case(cfg, shape)
    assert str(g["digest"]) == R.digest(xn, gon, *[qn[k] for k in sorted(qn)])
    bound = _case(cfg, shape)[5]
    got = _teacher_grads(cfg, shape)
    for n in BR.NAMES:
        if n not in (W1, W3):
            _check(got[n].cpu(), torch.as_tensor(g[n.replace(".", "_")]), bound[n].cpu(), "%s %s vs the reference" % (BR.name(cfg, shape), n))
    for key, n in (("W1", W1), ("W3", W3)):
        w = got[n][:, :, 0, 0]
        _check(w[BR.W_SUBSET].cpu(), torch.as_tensor(g[key]), bound[n][:, :, 0, 0][BR.W_SUBSET].cpu(),
               "%s %s vs the reference" % (BR.name(cfg, shape), key))
        tot = float(bound[n].sum())
        assert abs(float(w.double().sum()) - float(g[key + "_sum"])) <= tot
        assert abs(float(w.double().norm()) - float(g[key + "_l2"])) <= tot


# ------------------------------------------------------------------------------------------------ 4. block_backward
@pytest.mark.parametrize("cs", CASES, ids=_id)
def test_block_backward_end_to_end(cs, golden_dir):
    """The device recomputes e and d.  The parameter gradients equal block_param_grads fed the call's own parts, bit for
    bit; grad_x is within block_ref64.block_e2e's limit: per frame in L2, the regular bound plus the term of the masks the
    device may decide the other way.  With the residual, grad_x is the no-residual result plus grad_out."""
    cfg, shape = cs
    block, q, x, go, _, _, t, _ = _case(cfg, shape)
    res = BR.CFG[cfg]["res"]
    want, bound, und, _ = BR.block_e2e(q, x, go, res)
    parts = {}
    gx, grads = train.block_backward(block, t["x"], t["go"], parts=parts)
    assert sorted(parts) == ["d", "e", "ga", "gd"] and tuple(grads) == BR.NAMES and gx.shape == t["x"].shape
    again = train.block_param_grads(block, t["x"], parts["e"], parts["d"], t["go"], gd=parts["gd"], ga=parts["ga"])
    for n in BR.NAMES:
        assert torch.equal(_bits(grads[n]), _bits(again[n])), n
    err, lim, ref = R.l2_per_frame(gx.double() - want), R.l2_per_frame(bound + und), R.l2_per_frame(want)
    print("%s: per frame ||err|| / ||grad_x|| %s, limit %s" % (BR.name(cfg, shape), ["%.2e" % v for v in (err / ref).tolist()],
                                                              ["%.2e" % v for v in (lim / ref).tolist()]))
    assert bool((err <= lim).all())
    if shape in BR.GOLDEN_SHAPES:                                                   # ... and the reference's own grad_x
        g = np.load(os.path.join(golden_dir, BR.name(cfg, shape) + ".npz"))
        assert float((want[BR.GX_SUBSET].cpu() - torch.as_tensor(g["grad_x"])).abs().max()) <= 1e-10 * float(want.abs().max())
    none, same = train.block_backward(block, t["x"], t["go"], need_x_grad=False, grads={n: torch.zeros_like(v) for n, v in grads.items()})
    assert none is None and all(torch.equal(_bits(same[n]), _bits(grads[n])) for n in BR.NAMES)
    if res:
        block.use_res_connect = False
        try:
            plain, _ = train.block_backward(block, t["x"], t["go"])
        finally:
            block.use_res_connect = True
        exp = plain.double() + go
        assert bool(((gx.double() - exp).abs() <= 2 * R.EPS * (plain.double().abs() + go.abs())).all())
        assert float((gx - plain).abs().max()) > 0
    with pytest.raises(RuntimeError, match="eval"):
        train.block_backward(block.train(), t["x"], t["go"])
    block.eval()
    with pytest.raises(RuntimeError, match="grad_out"):
        train.block_backward(block, t["x"], t["go"][:, :128])


# ------------------------------------------------------------------------------------------------ 5. the step and the driver
H_, W_, T_ = 72, 104, 4
RNN = "rnn.cell_list.0.rnn_conv.weight"
BIAS = {"priors": [1, 1, 1], "no_priors": [0, 0, 0]}


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


def _fuse(m):
    """(the trained block, the container refresh_weights takes, its parameter names in the model)"""
    box, name = (m.fucbst_layer, "fucbst_layer") if m.num_cb else (m.fust_layer, "fust_layer")
    return box[0], box, ["%s.0.%s" % (name, n) for n in BR.NAMES]


def _model(kind="priors"):
    from iip_uavsal_saliency_amd import UAVSal
    m = UAVSal(time_dims=T_, bias_type=BIAS[kind])
    synth.load_synth_weights(m, 0)
    with torch.no_grad():                                       # running statistics that are not the initial 0 and 1
        g = torch.Generator().manual_seed(11)
        for blk in (m.conv_out_st, _fuse(m)[0]):
            for bn in (blk.conv[0][1], blk.conv[1][1], blk.conv[3]):
                bn.running_mean.add_(0.05 * torch.randn(bn.running_mean.shape, generator=g))
                bn.running_var.mul_(1.0 + 0.2 * torch.rand(bn.running_var.shape, generator=g))
    return m.to(DEV).eval()


def _stats(m):
    return [b.detach().clone() for b in m.buffers()]


@pytest.mark.parametrize("kind", list(BIAS))
def test_recurrence_step_with_the_fuse_block(kind):
    m = _model(kind)
    x, cb, y = _step_inputs()
    blk, box, names = _fuse(m)
    assert train.fuse_block(m)[0] is blk
    stats = _stats(m)
    loss, out, st = train.recurrence_step(m, x, cb, None, y, fuse=True)
    ref_out, ref_st = m(x, cb, None)
    assert torch.equal(out, ref_out) and torch.equal(st[0], ref_st[0]) and loss.item() == losses.loss_fu(ref_out, y).item()
    assert sorted(k for k, p in m.named_parameters() if p.grad is not None) == sorted([RNN] + names)      # exactly ten
    params = dict(m.named_parameters())
    g1 = {k: params[k].grad.clone() for k in [RNN] + names}
    assert all(torch.isfinite(v).all() and float(v.abs().max()) > 0 and v.is_contiguous() for v in g1.values())
    plain = _model(kind)
    train.recurrence_step(plain, x, cb, None, y)                                  # the recurrence's own gradient does not change
    assert torch.equal(g1[RNN], plain.rnn.cell_list[0].rnn_conv.weight.grad)
    train.recurrence_step(m, x, cb, None, y, fuse=True)                           # .grad += as loss.backward() would
    for k in names:
        _check(params[k].grad, 2 * g1[k].double(), 4 * R.U * g1[k].double().abs(), "second call doubles %s" % k)
    assert all(torch.equal(a, b) for a, b in zip(stats, _stats(m)))
    # the directional derivative along the normalised nine-tensor block gradient against the central difference (the
    # plumbing check of tests/test_train_gpu.py, with its 10 % and for its reason); weights edited in place and refreshed
    with torch.no_grad():
        norm = float(torch.sqrt(sum((g1[k].double() ** 2).sum() for k in names)))
        w0 = {k: params[k].detach().clone() for k in names}
        s = 2e-2 / norm
        vals = []
        for sign in (1.0, -1.0):
            for k in names:
                params[k].copy_(w0[k] + sign * s * g1[k] / norm)
            assert m.refresh_weights(box) > 0
            vals.append(losses.loss_fu(m(x, cb, None)[0], y).item())
        for k in names:
            params[k].copy_(w0[k])
        m.refresh_weights(box)
    fd = (vals[0] - vals[1]) / (2 * s)
    print("%s: fuse block directional derivative: finite difference %.6e, <grad, D> %.6e, step %.3e" % (kind, fd, norm, s))
    assert abs(fd - norm) <= 0.10 * abs(norm)
    assert torch.equal(m(x, cb, None)[0], ref_out)                                # the restored weights give the same bits


def test_adam_steps_over_three_stages_keep_the_plans():
    from iip_uavsal_saliency_amd import UAVSal
    m = _model()
    x, cb, y = _step_inputs()
    blk, box, names = _fuse(m)
    stats = _stats(m)
    opt = torch.optim.Adam(list(m.rnn.parameters()) + list(m.conv_out_st.parameters()) + list(box.parameters()), lr=1e-4,
                           betas=(0.9, 0.999), weight_decay=5e-5)
    before = m(x, cb, None)[0]
    first = None
    for _ in range(5):
        opt.zero_grad()
        loss, _, _ = train.recurrence_step(m, x, cb, None, y, decoder=True, fuse=True)
        first = loss.item() if first is None else first
        engines = dict(m._engines)
        opt.step()
        assert m.refresh_weights(m.rnn, m.conv_out_st, box) > 0
        after = m(x, cb, None)[0]
        assert {k: id(e) for k, e in m._engines.items()} == {k: id(e) for k, e in engines.items()}      # the same engine objects
    assert sorted(k for k, p in m.named_parameters() if p.grad is not None) == sorted(
        [RNN] + names + ["conv_out_st." + n for n in BR.NAMES])
    last = losses.loss_fu(after, y).item()
    print("loss_fu on the group: %.6f before, %.6f after five Adam steps over three stages" % (first, last))
    assert last < first and not torch.equal(before, after)
    assert all(torch.equal(a, b) for a, b in zip(stats, _stats(m)))                # running statistics unchanged
    fresh = UAVSal(time_dims=T_)
    fresh.load_state_dict(m.state_dict())
    fresh = fresh.to(DEV).eval()
    taps, ftaps = {}, {}
    got, got_st = m(x, cb, None, taps=taps)
    want, want_st = fresh(x, cb, None, taps=ftaps)
    assert torch.equal(got, want) and torch.equal(got_st[0], want_st[0])           # bit for bit the repacked weights
    assert "fu320" not in taps                                                     # the block's input is read back on request only
    taps, ftaps = {"fu320": None}, {"fu320": None}
    m(x, cb, None, taps=taps), fresh(x, cb, None, taps=ftaps)
    assert tuple(taps["fu320"].shape) == (2 * T_, 320, H_ // 8, W_ // 8) and taps["fu320"].is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(taps["fu320"][:, 256:], taps["fust_in_cb"])
    assert sorted(taps) == sorted(ftaps) and all(torch.equal(taps[k], ftaps[k]) for k in taps)
    got2, _ = m(x, cb, None)
    assert torch.equal(got2, want)


def test_finetune_video_with_three_stages_is_the_manual_loop():
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
        ps = list(m.rnn.parameters()) + list(m.conv_out_st.parameters()) + list(m.fucbst_layer.parameters())
        return m, torch.optim.Adam(ps, lr=1e-4, betas=(0.9, 0.999), weight_decay=5e-5)
    m, opt = make()
    seen = []
    real = train.recurrence_step

    def spy(model, x, cb, state, y, criterion, **kw):
        assert kw == {"decoder": True, "fuse": True}
        seen.append((x.clone(), [c.clone() for c in cb], y.clone()))
        return real(model, x, cb, state, y, criterion, **kw)
    train.recurrence_step = spy
    try:
        res = finetune_video(m, frames, gp, op_, fix_map, fix_loc, opt, batch_size=2, stages=("rnn", "decoder", "fuse"))
    finally:
        train.recurrence_step = real
    assert res["groups_run"] == 2 and len(seen) == 2
    m2, opt2 = make()
    state, manual = None, []
    for x, cb, y in seen:
        opt2.zero_grad()
        loss, _, state = train.recurrence_step(m2, x, cb, state, y, decoder=True, fuse=True)
        opt2.step()
        m2.refresh_weights(m2.rnn, m2.conv_out_st, m2.fucbst_layer)
        manual.append(loss.item())
    assert [float(v) for v in res["losses"].tolist()] == manual
    for (k, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    w0 = _model().fucbst_layer[0].conv[0][0].weight
    assert not torch.equal(m.fucbst_layer[0].conv[0][0].weight.detach(), w0.detach())
