"""Fine-tuning the multi-prior path on the GPU (the M tail of uavsal_pix_gemm, uavsal_ir_sums_s2, train.block_param_grads with
stride 2 or 64 output channels, train.prior_path_backward, recurrence_step(ctx=True), the in-place refresh of fucb_layer and
cxt_cb_prior) against the float64 restatement tests/mp_ref64.py, which runs on the device in torch float64.  Bounds:
mp_ref64's docstring.
The kernels are tested teacher-forced (the stored e and d decide every mask as the float64 ones do), and the path STAGE BY
STAGE: each trained block's nine gradients against float64 fed the very tensors the walk handed that block (ctx_ref64's
docstring says why a bound composed over three blocks is worthless).  The goldens (tests/golden/ctx_train_*.npz) are held
against the float64 restatement by tests/test_train_ctx_cpu.py; no test here reads the reference."""
import ctypes as C
import types
from functools import lru_cache

import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import _lib, losses, ops, synth, train

import block_ref64 as BR
import ctx_ref64 as X
import mp_ref64 as MP
import train_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W1, WD, W3 = BR.NAMES[0], BR.NAMES[3], BR.NAMES[6]


def _cl(a):
    return torch.as_tensor(a).to(DEV).float().contiguous(memory_format=torch.channels_last)


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


# ------------------------------------------------------------------------------------------------ 1. the pixel GEMM's M tail
def _shares(K, M, N):
    d = _lib.PixGemmDesc()
    d.K, d.M, d.N = K, M, N
    return int(_lib.load().uavsal_pix_gemm_shares(C.byref(d)))


@pytest.mark.parametrize("K", MP.GEMM_K)
@pytest.mark.parametrize("N", MP.GEMM_N)
@pytest.mark.parametrize("M", MP.GEMM_M)
def test_pix_gemm_m_tail_against_float64(M, N, K):
    """M = 64: half a tile; M = 192: a whole tile and half a one.  K = 1025 pixels is two chunks: the K split is real.  `a` is
    a channel slice of a wider tensor whose other columns are NaN: nothing at or behind row M is read."""
    gen = torch.Generator(DEV).manual_seed(1000 * M + 10 * N + K)
    wide = torch.full((1, 1, K, M + 128), float("nan"), device=DEV)
    wide[..., 64:64 + M] = 1e-2 * torch.randn(1, 1, K, M, device=DEV, generator=gen)
    a = wide[..., 64:64 + M]
    b = torch.randn(1, 1, K, N, device=DEV, generator=gen)
    want, bound = BR.pix_gemm_ref(a.double(), b.double())
    assert _shares(K, M, N) == MP.gemm_partition(K, M, N)[1] == (2 if K > 1024 else 1)
    got = train.pix_gemm(a, b)
    assert tuple(got.shape) == (M, N)
    _check(got, want, bound, "pix_gemm %d x %d, K %d" % (M, N, K))
    assert torch.equal(_bits(got), _bits(train.pix_gemm(a, b)))                   # two calls, the same bits
    assert torch.equal(_bits(got), _bits(train.pix_gemm(a.contiguous(), b)))      # the slice is the dense tensor
    # row_scale, rowdot and accumulate into an oversized buffer: the rows at and behind M stay what they were
    rs = torch.linspace(-2.0, 2.0, M, device=DEV)
    w = torch.randn(M, N, device=DEV, generator=gen)
    big = torch.full(((M + 64) * N,), float("nan"), device=DEV)
    old = torch.randn(M, N, device=DEV, generator=gen) * float(want.abs().max())
    big[:M * N] = old.reshape(-1)
    rowdot = torch.full((M + 64,), float("nan"), dtype=torch.float64, device=DEV)
    out = train.pix_gemm(a, b, out=big[:M * N].view(M, N), row_scale=rs, w=w, rowdot=rowdot[:M], accumulate=True)
    exp = old.double() + rs.double().view(-1, 1) * want
    _check(out, exp, rs.double().abs().view(-1, 1) * bound + R.EPS * (old.double().abs() + exp.abs()), "  + row_scale, accumulate")
    _check(rowdot[:M], (w.double() * want).sum(1), (w.double().abs() * bound).sum(1), "  rowdot")
    assert bool(torch.isnan(big[M * N:]).all()) and bool(torch.isnan(rowdot[M:]).all())
    plain = torch.full(((M + 64) * N,), float("nan"), device=DEV)
    train.pix_gemm(a, b, out=plain[:M * N].view(M, N))
    assert torch.equal(_bits(plain[:M * N].view(M, N)), _bits(got)) and bool(torch.isnan(plain[M * N:]).all())
    # a kernel that leaves the half tile out, or takes one chunk only, is rejected by the bound
    tail = want.clone()
    tail[M // 128 * 128:] = 0
    assert not _within(got, tail, bound)
    if K > 1024:
        A, B = a.reshape(-1, M).double(), b.reshape(-1, N).double()
        assert not _within(got, A[:1024].T @ B[:1024], bound)


@pytest.mark.parametrize("K", [33, 1025, 3 * 1024 + 5])
def test_pix_gemm_one_tile_is_its_two_halves(K):
    """M = 128 (the tile it always took) returns, row for row, the bits of the two M = 64 calls on its halves: an element's
    chain does not depend on where in the tile it sits, and the share count is the same (one M tile either way)."""
    N = 384
    gen = torch.Generator(DEV).manual_seed(K)
    a = 1e-2 * torch.randn(1, 1, K, 128, device=DEV, generator=gen)
    b = torch.randn(1, 1, K, N, device=DEV, generator=gen)
    assert _shares(K, 128, N) == _shares(K, 64, N) == MP.gemm_partition(K, 64, N)[1]
    whole = train.pix_gemm(a, b)
    lo, hi = train.pix_gemm(a[..., :64], b), train.pix_gemm(a[..., 64:], b)
    assert torch.equal(_bits(whole[:64]), _bits(lo)) and torch.equal(_bits(whole[64:]), _bits(hi))
    with pytest.raises(RuntimeError, match="ESHAPE|shape|rejected"):
        train.pix_gemm(a[..., :96], b)


# ------------------------------------------------------------------------------------------------ 2. uavsal_ir_sums_s2 + finish
def _finish(ws, slabs, Ch, Co, num):
    """uavsal_ir_finish on the workspace of the sums; `num`: wd [Ch,3,3], s2, r1, mu1, r2, mu2 [Ch], r3, mu3 [Co] fp32 and rowdot1
    [Ch], rowdot3 [Co] float64 on the device.  Returns the seven small gradients."""
    out = {"g_gamma1": (Ch,), "g_beta1": (Ch,), "g_wd": (Ch, 3, 3), "g_gamma2": (Ch,), "g_beta2": (Ch,), "g_gamma3": (Co,), "g_beta3": (Co,)}
    out = {k: torch.empty(s, dtype=torch.float32, device=DEV) for k, s in out.items()}
    k = _lib.IrFinishDesc()
    k.ws, k.ws_bytes, k.rowdot1, k.rowdot3 = ws.data_ptr(), ws.numel() * 8, num["rowdot1"].data_ptr(), num["rowdot3"].data_ptr()
    for n in ("wd", "s2", "r1", "mu1", "r2", "mu2", "r3", "mu3"):
        setattr(k, n, num[n].data_ptr())
    for n, t in out.items():
        setattr(k, n, t.data_ptr())
    k.Ch, k.Co, k.slabs, k.accumulate = Ch, Co, slabs, 0
    _lib.check(_lib.load().uavsal_ir_finish(C.byref(k), ops._stream(ws)), "uavsal_ir_finish")
    return out


@pytest.mark.parametrize("shape", MP.SUMS_SHAPES, ids=lambda s: "n%d_%dx%d_c%d_o%d" % s)
def test_ir_sums_s2_teacher_forced_against_float64(shape):
    """Odd H or W: the last input row / column is read by one output only (45 -> 23, 23 -> 12, 5 -> 3, 3 -> 2, 1 -> 1), and
    2 oy - 1 + ky reaches -1 and H.  (2,23,40): 6 slabs of 4 output rows, one of them across both images; 384 = 256 + 128: a
    partial last channel group."""
    n, H, W, Ch, Co = shape
    gd, d, e, ga, go = MP.sums_case(shape)
    wide = torch.full((n, X.down(H), X.down(W), Co + 64), float("nan"), device=DEV)      # go: a channel slice, its neighbours NaN
    wide[..., 32:32 + Co] = _nhwc(go)
    t = (_nhwc(gd), _nhwc(d, True), _nhwc(e, True), _nhwc(ga), wide[..., 32:32 + Co])
    gd, d, e, ga, go = (_nchw64(v) for v in t)                                            # what the kernel reads
    ws, slabs = train.ir_sums_s2(*t)
    assert slabs == MP.slab_partition_s2(n, H, W)[1] and ws.numel() == slabs * (MP.NSUM * Ch + Co)
    ws2, _ = train.ir_sums_s2(*t)
    assert torch.equal(ws.view(torch.int64), ws2.view(torch.int64))                      # two calls, the same bits
    dense, _ = train.ir_sums_s2(*t[:4], t[4].contiguous())
    assert torch.equal(ws.view(torch.int64), dense.view(torch.int64))
    tot = ws.view(slabs, MP.NSUM * Ch + Co).sum(0)
    got = {"S2": tot[:Ch], "Gd": tot[Ch:10 * Ch].view(9, Ch).t().reshape(Ch, 3, 3), "S1": tot[10 * Ch:11 * Ch], "S3": tot[11 * Ch:]}
    want, bound = MP.ir_sums_s2_ref(gd, d, e, ga, go, bounds=True)
    slack = {k: bound[k] + slabs * MP.D * want[k].abs() for k in want}                    # + this test's own sum of the slabs
    for k in ("S2", "Gd", "S1", "S3"):
        _check(got[k], want[k], slack[k], "uavsal_ir_sums_s2 %r %s" % (shape, k))
    if H >= 3:                                                                            # the wrong kernels are told apart
        for v, k in (("stride1_e", "Gd"), ("no_top_pad", "Gd"), ("s1_output_grid", "S1")):
            wrong = MP.ir_sums_s2_ref(gd, d, e, ga, go, variant=v)
            assert not _within(got[k], wrong[k], slack[k]), v
    # uavsal_ir_finish, unchanged, on that workspace
    gen = torch.Generator(DEV).manual_seed(n * H * W + Ch)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=gen)                           # noqa: E731
    num = {"wd": rnd(Ch, 3, 3) / 3, "s2": rnd(Ch), "r1": rnd(Ch).abs() + 0.5, "mu1": rnd(Ch), "r2": rnd(Ch).abs() + 0.5, "mu2": rnd(Ch),
           "r3": rnd(Co).abs() + 0.5, "mu3": rnd(Co), "rowdot1": rnd(Ch).double() * 3, "rowdot3": rnd(Co).double() * 3}
    fin = _finish(ws, slabs, Ch, Co, num)
    q = {k: v.double() for k, v in num.items()}
    A = MP.ir_sums_s2_ref(gd.abs(), d, e.abs(), ga.abs(), go.abs())
    E = R.EPS
    ref = {"g_beta1": (want["S1"], bound["S1"] + E * A["S1"]), "g_beta2": (want["S2"], bound["S2"] + E * A["S2"]),
           "g_beta3": (want["S3"], bound["S3"] + E * A["S3"]),
           "g_wd": (q["s2"].view(-1, 1, 1) * want["Gd"], q["s2"].abs().view(-1, 1, 1) * (bound["Gd"] + E * A["Gd"])),
           "g_gamma2": (q["r2"] * ((q["wd"] * want["Gd"]).sum((1, 2)) - q["mu2"] * want["S2"]),
                        q["r2"] * ((q["wd"].abs() * bound["Gd"]).sum((1, 2)) + q["mu2"].abs() * bound["S2"])
                        + E * q["r2"] * ((q["wd"].abs() * A["Gd"]).sum((1, 2)) + q["mu2"].abs() * A["S2"])),
           "g_gamma1": (q["r1"] * (q["rowdot1"] - q["mu1"] * want["S1"]),
                        q["r1"] * q["mu1"].abs() * bound["S1"] + E * q["r1"] * (q["rowdot1"].abs() + q["mu1"].abs() * A["S1"])),
           "g_gamma3": (q["r3"] * (q["rowdot3"] - q["mu3"] * want["S3"]),
                        q["r3"] * q["mu3"].abs() * bound["S3"] + E * q["r3"] * (q["rowdot3"].abs() + q["mu3"].abs() * A["S3"]))}
    for k, (w_, b_) in ref.items():
        _check(fin[k], w_, b_, "  uavsal_ir_finish %s" % k)


def test_ir_sums_s2_refuses_what_it_does_not_cover():
    t = torch.zeros(1, 4, 4, 64, device=DEV)
    o = torch.zeros(1, 2, 2, 64, device=DEV)
    with pytest.raises(RuntimeError, match="ir_sums_s2"):
        train.ir_sums_s2(o, o, t, t, torch.zeros(1, 4, 4, 64, device=DEV))              # go on the input grid
    with pytest.raises(RuntimeError, match="ir_sums_s2"):
        train.ir_sums_s2(t, t, t, t, o)                                                  # gd, d on the input grid
    z = torch.zeros(1, 4, 4, 96, device=DEV)
    with pytest.raises(RuntimeError, match="ESHAPE|shape|rejected"):
        train.ir_sums_s2(torch.zeros(1, 2, 2, 96, device=DEV), torch.zeros(1, 2, 2, 96, device=DEV), z, z, o)


# ------------------------------------------------------------------------------------------------ 3. block_param_grads
ZERO = (5, 17)                          # gamma1 = 0 in channel 5, gamma2 = 0 in channel 17 (their beta 1.5)


def _block(name, q):
    from iip_uavsal_saliency_amd.model import dwBlock
    return X.make_block(name, q, dwBlock).to(DEV)


@lru_cache(maxsize=None)
def _case(name, shape, gain=1.0, shift=0.0, zero_gamma=False):
    """the block, its fold, the float64 closed form with bounds and the teacher-forced fp32 tensors; once per case"""
    xn, qn, gon = X.block_case(name, shape, gain=gain, shift=shift)
    if zero_gamma:
        qn = {k: v.copy() for k, v in qn.items()}
        for i, c in ((1, ZERO[0]), (2, ZERO[1])):
            qn["g%d" % i][c], qn["be%d" % i][c] = 0.0, 1.5
    stride = X.BLOCKS[name][3]
    p = BR.fold(BR.to64(qn, DEV))
    x, go = _d64(xn), _d64(gon)
    pt = MP.block_parts(p, x, go, stride)
    want, bound = MP.grads_from_parts(p, x, pt["e"], pt["d"], pt["gd"], pt["ga"], go, stride, bounds=True)
    t = {"x": _cl(xn), "go": _cl(gon), "e": _nhwc(pt["e"], True), "d": _nhwc(pt["d"], True), "gd": _nhwc(pt["gd"]), "ga": _nhwc(pt["ga"])}
    return _block(name, qn), p, want, bound, t, pt


def _teacher(name, shape, *a, **kw):
    block, _, _, _, t, _ = _case(name, shape, *a)
    return train.block_param_grads(block, t["x"], t["e"], t["d"], t["go"], gd=t["gd"], ga=t["ga"], **kw)


@pytest.mark.parametrize("shape", MP.TRAINED_SHAPES, ids=lambda s: "n%d_%dx%d" % s)
@pytest.mark.parametrize("name", MP.TRAINED)
def test_param_grads_of_the_path_blocks_teacher_forced(name, shape):
    """192 -> 1152 -> 64, 128 -> 768 -> 64, 64 -> 384 -> 64 with the residual (stride 1, 64 output channels: the M tail of the
    projection's weight gradient) and 256 -> 1536 -> 64, 64 -> 384 -> 64 with stride 2, at 5 x 7 and 23 x 40."""
    cin, hid, cout, stride = X.BLOCKS[name]
    block, p, want, bound, t, pt = _case(name, shape)
    assert block.stride == stride and bool(block.use_res_connect) == (stride == 1 and cin == cout)
    n, H, W = shape
    assert tuple(t["d"].shape) == ((n, X.down(H), X.down(W), hid) if stride == 2 else (n, H, W, hid))
    got = _teacher(name, shape)
    assert tuple(got) == BR.NAMES
    for k in BR.NAMES:
        assert got[k].shape == want[k].shape and got[k].dtype == torch.float32
        _check(got[k], want[k], bound[k], "%s %r %s" % (name, shape, k))
    again = _teacher(name, shape)
    assert all(torch.equal(_bits(got[k]), _bits(again[k])) for k in BR.NAMES)      # two calls, the same bits
    old = {k: torch.full_like(got[k], 0.25) * float(want[k].abs().max()) for k in BR.NAMES}
    acc = {k: v.clone() for k, v in old.items()}
    assert _teacher(name, shape, out=acc, accumulate=True) is acc                  # accumulate adds, rounded once
    for k in BR.NAMES:
        exp = old[k].double() + want[k]
        _check(acc[k], exp, bound[k] + R.EPS * (old[k].double().abs() + exp.abs()), "  accumulate %s" % k)
    if stride == 2:                                                                # the wrong sums are told apart through the finish
        x, go = t["x"].double(), t["go"].double()
        for v, k in (("stride1_e", WD), ("no_top_pad", WD), ("s1_output_grid", BR.NAMES[2])):
            wrong = MP.grads_from_parts(p, x, pt["e"], pt["d"], pt["gd"], pt["ga"], go, 2, variant=v)
            assert not _within(got[k], wrong[k], bound[k]), v
    else:                                                                          # ... and a projection gradient without its M tail
        tail = want[W3].clone()
        tail[cout // 128 * 128:] = 0
        assert not _within(got[W3], tail, bound[W3])


@pytest.mark.parametrize("name", ["ctx1", "ctx0", "fucb64"])
def test_default_gd_and_ga_come_from_the_device(name):
    """Without `gd` / `ga` block_param_grads forms them by the launches of block_input_grad (uavsal_ir_bwd_s2 for stride 2): the
    bits of the call that is handed block_input_grad's own parts."""
    shape = MP.TRAINED_SHAPES[0]
    block, _, _, _, t, _ = _case(name, shape)
    parts = {}
    train.block_input_grad(block, t["x"], t["go"], parts=parts)
    mine = train.block_param_grads(block, t["x"], parts["e"], parts["d"], t["go"])
    ref = train.block_param_grads(block, t["x"], parts["e"], parts["d"], t["go"], gd=parts["gd"], ga=parts["ga"])
    assert all(torch.equal(_bits(mine[k]), _bits(ref[k])) for k in BR.NAMES)
    assert all(q.grad is None for q in block.parameters())
    with pytest.raises(RuntimeError, match="expand conv|Cout"):                    # block_backward keeps to what it took
        train.block_backward(block, t["x"], t["go"])
    with pytest.raises(RuntimeError, match="dense float32 NHWC"):
        train.block_param_grads(block, t["x"], parts["e"], parts["e"][:, :1], t["go"])


@pytest.mark.parametrize("name", ["ctx1", "ctx0", "fucb64"])
def test_zero_gamma_channels_have_a_gamma_gradient(name):
    shape = MP.TRAINED_SHAPES[0]
    _, _, want, bound, _, _ = _case(name, shape, 1.0, 0.0, True)
    got = _teacher(name, shape, 1.0, 0.0, True)
    for k in BR.NAMES:
        _check(got[k], want[k], bound[k], "zero gamma %s %s" % (name, k))
    c1, c2 = ZERO
    assert float(got[W1][c1].abs().max()) == 0 and float(got[WD][c2].abs().max()) == 0
    for k, c in ((BR.NAMES[1], c1), (BR.NAMES[4], c2)):
        assert float(got[k][c].abs()) > 0 and float((got[k][c].double() - want[k][c]).abs()) <= float(bound[k][c])


@pytest.mark.parametrize("name", ["ctx0", "ctx1"])
def test_param_grads_of_a_saturated_stride_2_block(name):
    """e and d of a stride-2 block whose two ReLU6 BatchNorms got tests/saturate_bn.py's gain and shift: both clamps occur in
    both tensors, the upper one in more than a fifth of each."""
    shape = MP.TRAINED_SHAPES[1]
    _, _, want, bound, _, pt = _case(name, shape, 1.5, 3.0)
    got = _teacher(name, shape, 1.5, 3.0)
    for k in BR.NAMES:
        _check(got[k], want[k], bound[k], "saturated %s %s" % (name, k))
    for k in ("e", "d"):
        lo, mid, hi = BR.class_shares(pt[k])
        print("saturated %s %s: shares at or below 0 / inside / at or above 6: %.3f %.3f %.3f" % (name, k, lo, mid, hi))
        assert lo >= 0.01 and mid >= 0.1 and hi >= 0.2


# ------------------------------------------------------------------------------------------------ 4. the path, stage by stage
T2 = MP.GOLDEN_T


@lru_cache(maxsize=None)
def _head(bias):
    """a stand-in for the model (the attributes prior_path_backward reads) over ctx_ref64.head_case's calibrated blocks, N = 2 T
    frames at 9 x 13"""
    Q, st, priors, go = X.head_case(bias, MP.GOLDEN_SHAPE, T2)
    Pf = X.folds(Q, DEV)
    m = types.SimpleNamespace(num_cb=sum(bias), training=False, time_dims=T2, use_gauss_prior=bias[0], use_ob_prior=bias[1],
                              use_context_prior=bias[2])
    m.fucb_layer = [_block("fucb%d" % (64 * sum(bias)), Q["fucb"])]
    if bias[2]:
        m.cxt_cb_prior = [_block("ctx0", Q["ctx0"]), _block("ctx1", Q["ctx1"])]
    hd = X.head_forward(Pf, _d64(st), _d64(priors) if priors is not None else None, T2, use_ctx=bool(bias[2]))
    gfu = X.input_grad_ref(Pf["fucbst"], hd["fu"], _d64(go), 1, False)
    return m, Pf, _cl(hd["fu"]), _cl(hd["cbcat"]), _cl(gfu)


@pytest.mark.parametrize("bias", MP.GOLDEN_BIAS, ids=str)
def test_prior_path_backward_stage_by_stage(bias):
    m, Pf, fu, cb, gfu = _head(bias)
    k = bias[0] + bias[1]
    blocks = train.prior_path_blocks(m)
    assert tuple(blocks) == MP.PATH_BLOCKS[:3 if bias[2] else 1]
    parts = {}
    g, grads = train.prior_path_backward(m, fu, cb, gfu, parts=parts, grads={n: None for n in blocks})
    assert tuple(grads) == tuple(blocks) and all(q.grad is None for b in blocks.values() for q in b.parameters())
    frozen = train.fust_output_grad(m, fu, cb, gfu)
    assert torch.equal(_bits(g), _bits(frozen))                                    # the walk is the frozen one
    N, h, w = MP.GOLDEN_SHAPE
    B = N // T2
    for name, blk in blocks.items():
        pt = parts[name]
        stride = blk.stride
        x, go, e, d, gd, ga = (_nchw64(pt[v]) for v in ("x", "go", "e", "d", "gd", "ga"))
        assert x.shape[0] == (N if name == MP.PATH_BLOCKS[0] else B), name       # cxt_cb_prior sees the chunk sums: B images
        want, bound = MP.grads_from_parts(Pf[MP.PATH_KEYS[name]], x, e, d, gd, ga, go, stride, bounds=True)
        for n in BR.NAMES:
            _check(grads[name][n], want[n], bound[n], "%r %s %s" % (bias, name, n))
    if bias[2]:
        # a walk that feeds cxt_cb_prior the N frames is told apart in every tensor but the one it cannot change
        wrong = MP.path_param_grads(Pf, fu.double(), cb.double(), gfu.double(), T2, k, variant="per_frame")
        for name in MP.PATH_BLOCKS[1:]:
            pt = parts[name]
            x, go, e, d, gd, ga = (_nchw64(pt[v]) for v in ("x", "go", "e", "d", "gd", "ga"))
            _, bound = MP.grads_from_parts(Pf[MP.PATH_KEYS[name]], x, e, d, gd, ga, go, 2, bounds=True)
            for n in BR.NAMES:
                if (name, n) != (MP.PATH_BLOCKS[1], BR.NAMES[8]):
                    assert not _within(grads[name][n], wrong[name][n], bound[n]), (name, n)
        # the slices are read in place
        assert parts[MP.PATH_BLOCKS[0]]["x"].data_ptr() == cb.data_ptr()
        assert parts[MP.PATH_BLOCKS[0]]["go"].data_ptr() == gfu.data_ptr() + 4 * 256
    else:
        assert torch.equal(g, gfu[:, :256])
    # only the parameter gradients: None in the output gradient's place, the same bits; a part of the blocks; accumulate
    g2, again = train.prior_path_backward(m, fu, cb, gfu, grads={n: None for n in blocks}, need_fust_grad=False)
    assert g2 is None and all(torch.equal(_bits(again[b][n]), _bits(grads[b][n])) for b in blocks for n in BR.NAMES)
    first = MP.PATH_BLOCKS[0]
    acc = {first: {n: v.clone() for n, v in grads[first].items()}}
    _, out = train.prior_path_backward(m, fu, cb, gfu, grads=acc, accumulate=True, need_fust_grad=False)
    assert out[first] is acc[first] and tuple(out) == (first,)
    for n in BR.NAMES:
        _check(acc[first][n], 2 * grads[first][n].double(), 4 * R.U * grads[first][n].double().abs(), "accumulate doubles %s" % n)
    if bias[2]:
        last = MP.PATH_BLOCKS[2]
        _, only = train.prior_path_backward(m, fu, cb, gfu, grads={last: None}, need_fust_grad=False)
        assert all(torch.equal(_bits(only[last][n]), _bits(grads[last][n])) for n in BR.NAMES)
    with pytest.raises(RuntimeError, match="eval"):
        m.training = True
        try:
            train.prior_path_backward(m, fu, cb, gfu, grads={n: None for n in blocks})
        finally:
            m.training = False


# ------------------------------------------------------------------------------------------------ 5. the step and the driver
H_, W_, T_ = 72, 104, 4
RNN = "rnn.cell_list.0.rnn_conv.weight"
BIAS = {"all": [1, 1, 1], "context": [0, 0, 1], "no_context": [1, 1, 0]}


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


FUST, FUCBST, DEC = _names("fust_layer"), _names("fucbst_layer"), ["conv_out_st." + n for n in BR.NAMES]
PATH = {"all": _names("fucb_layer") + _names("cxt_cb_prior", 1) + _names("cxt_cb_prior", 0)}
PATH["context"], PATH["no_context"] = PATH["all"], _names("fucb_layer")


def _model(kind="all"):
    from iip_uavsal_saliency_amd import UAVSal
    m = UAVSal(time_dims=T_, bias_type=BIAS[kind])
    synth.load_synth_weights(m, 0)
    with torch.no_grad():                                       # running statistics that are not the initial 0 and 1
        g = torch.Generator().manual_seed(11)
        for blk in [m.conv_out_st, m.fucbst_layer[0], m.fust_layer[0], m.fucb_layer[0]] + (list(m.cxt_cb_prior) if BIAS[kind][2] else []):
            for bn in (blk.conv[0][1], blk.conv[1][1], blk.conv[3]):
                bn.running_mean.add_(0.05 * torch.randn(bn.running_mean.shape, generator=g))
                bn.running_var.mul_(1.0 + 0.2 * torch.rand(bn.running_var.shape, generator=g))
    return m.to(DEV).eval()


def _stats(m):
    return [b.detach().clone() for b in m.buffers()]


def _grads(m, names):
    params = dict(m.named_parameters())
    return {k: params[k].grad.clone() for k in names}


def _path_mods(m):
    return (m.fucb_layer,) + ((m.cxt_cb_prior,) if m.use_context_prior else ())


def _has_grad(m):
    return sorted(n for n, p in m.named_parameters() if p.grad is not None)


@pytest.mark.parametrize("kind", list(BIAS))
def test_recurrence_step_with_ctx(kind):
    """"context" is the single-prior model: its fucb_layer[0] is 64 -> 384 -> 64 with the residual and runs as ONE fused_mid
    launch at this size (a natural-layout `fused` entry), which the refresh below remakes in place."""
    m = _model(kind)
    x, cb, y = _step_inputs()
    names = PATH[kind]
    assert len(names) == (27 if BIAS[kind][2] else 9)
    stats = _stats(m)
    loss, out, st = train.recurrence_step(m, x, cb, None, y, decoder=True, fuse=True, fust=True, ctx=True)
    ref_out, ref_st = m(x, cb, None)
    assert torch.equal(out, ref_out) and torch.equal(st[0], ref_st[0]) and loss.item() == losses.loss_fu(ref_out, y).item()
    assert _has_grad(m) == sorted([RNN] + DEC + FUCBST + FUST + names)
    g1 = _grads(m, [RNN] + DEC + FUCBST + FUST + names)
    assert all(torch.isfinite(v).all() and float(v.abs().max()) > 0 and v.is_contiguous() for v in g1.values())
    assert all(torch.equal(a, b) for a, b in zip(stats, _stats(m)))
    # every other stage's gradients are those of a step without ctx, bit for bit -- with fust and without it
    plain = _model(kind)
    train.recurrence_step(plain, x, cb, None, y, decoder=True, fuse=True, fust=True)
    assert _has_grad(plain) == sorted([RNN] + DEC + FUCBST + FUST)
    g0 = _grads(plain, [RNN] + DEC + FUCBST + FUST)
    assert all(torch.equal(g0[n], g1[n]) for n in g0)
    nofust = _model(kind)
    train.recurrence_step(nofust, x, cb, None, y, decoder=True, fuse=True, ctx=True)
    assert _has_grad(nofust) == sorted([RNN] + DEC + FUCBST + names)
    gn = _grads(nofust, [RNN] + DEC + FUCBST + names)
    assert all(torch.equal(gn[n], g1[n]) for n in gn)
    # the path's gradients are prior_path_backward's on the taps, and each block's are within its stage's bound
    taps, fu, gfu = _grad_fu(m, x, cb, y, decoder=True)
    assert tuple(taps["cb192"].shape) == (2 * T_, 64 * m.num_cb, H_ // 8, W_ // 8)
    parts = {}
    _, mine = train.prior_path_backward(m, fu, taps["cb192"], gfu, parts=parts,
                                        grads={n: None for n in train.prior_path_blocks(m)}, need_fust_grad=False)
    for name, blk in train.prior_path_blocks(m).items():
        p = X.fold_module(blk)
        pt = parts[name]
        xx, go, e, d, gd, ga = (_nchw64(pt[v]) for v in ("x", "go", "e", "d", "gd", "ga"))
        want, bound = MP.grads_from_parts(p, xx, e, d, gd, ga, go, blk.stride, bounds=True)
        for n in BR.NAMES:
            assert torch.equal(_bits(mine[name][n]), _bits(g1["%s.%s" % (name, n)])), (name, n)
            # (the device's folds s = gamma r and r are the float64 ones rounded once: U on every tensor they scale, twice)
            _check(mine[name][n], want[n], bound[n] + 2 * R.U * want[n].abs(), "step %s %s %s" % (kind, name, n))
    # .grad += as loss.backward() would
    train.recurrence_step(m, x, cb, None, y, decoder=True, fuse=True, fust=True, ctx=True)
    params = dict(m.named_parameters())
    for n in names:
        _check(params[n].grad, 2 * g1[n].double(), 4 * R.U * g1[n].double().abs(), "second call doubles %s" % n)
    # the directional derivative along the normalised gradient of the path's 9 / 27 tensors against the central difference
    # of the GPU forward (the plumbing check of tests/test_train_gpu.py, with its 10 % and for its reason); the refresh is in
    # place: the engines stay the objects they were
    engines = {k: id(e) for k, e in m._engines.items()}
    with torch.no_grad():
        norm = float(torch.sqrt(sum((g1[n].double() ** 2).sum() for n in names)))
        w0 = {n: params[n].detach().clone() for n in names}
        s = 2e-2 / norm
        vals = []
        for sign in (1.0, -1.0):
            for n in names:
                params[n].copy_(w0[n] + sign * s * g1[n] / norm)
            assert m.refresh_weights(*_path_mods(m)) > 0
            vals.append(losses.loss_fu(m(x, cb, None)[0], y).item())
        for n in names:
            params[n].copy_(w0[n])
        assert m.refresh_weights(*_path_mods(m)) > 0
    fd = (vals[0] - vals[1]) / (2 * s)
    print("%s: path directional derivative: finite difference %.6e, <grad, D> %.6e, step %.3e" % (kind, fd, norm, s))
    assert abs(fd - norm) <= 0.10 * abs(norm)
    assert torch.equal(m(x, cb, None)[0], ref_out)                                # the restored weights give the same bits
    assert {k: id(e) for k, e in m._engines.items()} == engines
    if kind == "context":
        store = m._wshared[str(torch.device(DEV))]
        dwc = m.fucb_layer[0].conv[1][0]
        assert ("fused", id(dwc), True) in store                                  # fused_mid took it, and it was remade in place


def _grad_fu(m, x, cb, y, decoder):
    """what recurrence_step hands the walk, by hand: `(taps, fu320, d loss / d fu320)`"""
    taps = {"fu320": None, "cb192": None}
    out, _ = m(x, cb, None, taps=taps)
    pred = out.detach().requires_grad_(True)
    with torch.enable_grad():
        (g_y,) = torch.autograd.grad(losses.loss_fu(pred, y), pred)
    cl = torch.channels_last
    h_seq, x_seq = taps["rnn"].contiguous(memory_format=cl), taps["prefuse"].contiguous(memory_format=cl)
    if decoder:
        grad_h = train.decoder_backward(m.conv_out_st, h_seq, g_y, y=out)[0]
    else:
        grad_h = train.decoder_input_grad(m.conv_out_st, h_seq, g_y, y=out)
    gx = train.twa_backward(x_seq, h_seq, None, m.rnn.cell_list[0].rnn_conv.weight.detach(), grad_h, need_x_grad=True)[1]
    fu = taps["fu320"].contiguous(memory_format=cl)
    return taps, fu, train.block_backward(m.fucbst_layer[0], fu, gx)[0]


def _trained(m):
    mods = [m.rnn, m.conv_out_st, m.fucbst_layer, m.fust_layer] + list(_path_mods(m))
    return [p for mod in mods for p in mod.parameters()]


@pytest.mark.parametrize("kind", ["all", "context"])
def test_adam_steps_over_five_stages_keep_the_plans(kind):
    from iip_uavsal_saliency_amd import UAVSal
    m = _model(kind)
    x, cb, y = _step_inputs()
    stats = _stats(m)
    opt = torch.optim.Adam(_trained(m), lr=1e-4, betas=(0.9, 0.999), weight_decay=5e-5)
    before = m(x, cb, None)[0]
    first = None
    for _ in range(5):
        opt.zero_grad()
        loss, _, _ = train.recurrence_step(m, x, cb, None, y, decoder=True, fuse=True, fust=True, ctx=True)
        first = loss.item() if first is None else first
        engines = dict(m._engines)
        opt.step()
        assert m.refresh_weights(m.rnn, m.conv_out_st, m.fucbst_layer, m.fust_layer, *_path_mods(m)) > 0
        after = m(x, cb, None)[0]
        assert {k: id(e) for k, e in m._engines.items()} == {k: id(e) for k, e in engines.items()}      # the same engine objects
    last = losses.loss_fu(after, y).item()
    print("%s: loss_fu on the group: %.6f before, %.6f after five Adam steps over five stages" % (kind, first, last))
    assert last < first and not torch.equal(before, after)
    assert all(torch.equal(a, b) for a, b in zip(stats, _stats(m)))                # running statistics unchanged
    w0 = _model(kind)
    for box in ("fucb_layer",) + (("cxt_cb_prior",) if BIAS[kind][2] else ()):     # ... and the path did move
        assert not torch.equal(getattr(m, box)[0].conv[0][0].weight.detach(), getattr(w0, box)[0].conv[0][0].weight.detach())
    fresh = UAVSal(time_dims=T_, bias_type=BIAS[kind])
    fresh.load_state_dict(m.state_dict())
    fresh = fresh.to(DEV).eval()
    got, got_st = m(x, cb, None)
    want, want_st = fresh(x, cb, None)
    assert torch.equal(got, want) and torch.equal(got_st[0], want_st[0])           # bit for bit the repacked weights
    taps, ftaps = {"cb192": None}, {"cb192": None}
    m(x, cb, None, taps=taps), fresh(x, cb, None, taps=ftaps)
    assert torch.equal(taps["cb192"], ftaps["cb192"])


def test_finetune_video_with_five_stages_is_the_manual_loop():
    from iip_uavsal_saliency_amd.stream import finetune_video
    n = 2 * T_ * 2
    frames = torch.from_numpy(synth.synth_frames_u8(n, H_, W_, 2)).to(DEV)
    gp = torch.from_numpy(synth.gauss_priors(1, H_ // 8, W_ // 8)[0]).to(DEV)
    op_ = torch.from_numpy(synth.ob_priors(1, H_ // 8, W_ // 8)[0]).to(DEV)
    loc = synth.synth_fix_points(n, 90, 130, 12, 9)
    fmap = np.rint(synth.synth_fix_maps(loc, 6.0) * 255).astype(np.uint8)
    fix_map, fix_loc = torch.from_numpy(fmap).to(DEV), torch.from_numpy(loc).to(DEV)
    stages = ("rnn", "decoder", "fuse", "fust", "ctx")
    kw = {s: True for s in stages[1:]}

    def make():
        m = _model()
        return m, torch.optim.Adam(_trained(m), lr=1e-4, betas=(0.9, 0.999), weight_decay=5e-5)
    m, opt = make()
    seen = []
    real = train.recurrence_step

    def spy(model, x, cb, state, y, criterion, **k):
        assert k == kw
        seen.append((x.clone(), [c.clone() for c in cb], y.clone()))
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
        m2.refresh_weights(m2.rnn, m2.conv_out_st, m2.fucbst_layer, m2.fust_layer, m2.fucb_layer, m2.cxt_cb_prior)
        manual.append(loss.item())
    assert [float(v) for v in res["losses"].tolist()] == manual
    for (k, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    w0 = _model()
    for blk, blk0 in ((m.fucb_layer[0], w0.fucb_layer[0]), (m.cxt_cb_prior[0], w0.cxt_cb_prior[0]), (m.cxt_cb_prior[1], w0.cxt_cb_prior[1])):
        assert not torch.equal(blk.conv[0][0].weight.detach(), blk0.conv[0][0].weight.detach())


def test_static_priors_give_the_gradients_of_materialised_ones():
    """Frame-invariant priors as zero-stride views run the prior nets on one frame (model.dedupe_priors); cb192 is still whole.
    The step's path gradients on that plan are prior_path_backward's on ITS taps, bit for bit, and they are the gradients of the
    step on materialised priors: equal bits where the two plans' cb192 are equal bits, else (the one-frame launches may pick
    other tiles: the 1e-4 of tests/test_hip_e2e.py on the maps) within 1e-3 of each tensor's norm -- a plumbing check, like the
    directional derivative's 10 %."""
    x, cb, y = _step_inputs()
    n = x.shape[0]
    view = [c[:1].expand(n, -1, -1, -1) for c in cb]
    mat = [c[:1].repeat(n, 1, 1, 1) for c in cb]
    names = PATH["all"]
    ms, mm = _model(), _model()
    train.recurrence_step(ms, x, view, None, y, fuse=True, ctx=True)
    train.recurrence_step(mm, x, mat, None, y, fuse=True, ctx=True)
    assert {e.static_priors for e in ms._engines.values() if e.keep_taps} == {True}
    gs, gm = _grads(ms, names), _grads(mm, names)
    ts, tm = {"cb192": None, "fu320": None}, {"cb192": None, "fu320": None}
    ms(x, view, None, taps=ts), mm(x, mat, None, taps=tm)
    assert torch.isfinite(ts["cb192"]).all() and float((ts["cb192"] - tm["cb192"]).abs().max()) <= 1e-4
    same = torch.equal(ts["cb192"], tm["cb192"]) and torch.equal(ts["fu320"], tm["fu320"])
    for k in names:
        assert torch.isfinite(gs[k]).all() and float(gs[k].abs().max()) > 0
        if same:
            assert torch.equal(gs[k], gm[k]), k
        else:
            rel = float((gs[k].double() - gm[k].double()).norm() / gm[k].double().norm())
            print("static vs materialised priors %s: ||difference|| / ||gradient|| %.3e" % (k, rel))
            assert rel <= 1e-3, k
    print("static priors: cb192 and fu320 %s those of materialised priors" % ("are bit for bit" if same else "differ in rounding from"))
    # on its own taps: the walk by hand
    taps, fu, gfu = _grad_fu(ms, x, view, y, decoder=False)
    _, mine = train.prior_path_backward(ms, fu, taps["cb192"], gfu, grads={b: None for b in train.prior_path_blocks(ms)},
                                        need_fust_grad=False)
    for b in mine:
        for k in BR.NAMES:
            assert torch.equal(_bits(mine[b][k]), _bits(gs["%s.%s" % (b, k)])), (b, k)
