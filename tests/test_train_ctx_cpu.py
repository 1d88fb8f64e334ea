"""Fine-tuning the multi-prior path (fucb_layer, cxt_cb_prior) without a GPU: the C ABI of uavsal_ir_sums_s2 and of the pixel
GEMM's M tail, the float64 restatements of tests/mp_ref64.py against torch autograd and against the reference's recorded
results (tests/golden/ctx_train_*.npz), what the Python entry points and the driver refuse, the GEMM routes the new calls
send, the in-place refresh of a natural-layout fused entry, and the conditions under which the GPU tests are meaningful: each
wrong variant lies at least 4 bounds from the right result in the float64 reference alone."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import _lib, stream, train
from iip_uavsal_saliency_amd import packing as P
from iip_uavsal_saliency_amd.weights import WeightCache

import block_ref64 as BR
import ctx_ref64 as X
import mp_ref64 as MP


def t64(a):
    return torch.as_tensor(a, dtype=torch.float64)


@pytest.fixture(scope="module")
def lib():
    from iip_uavsal_saliency_amd import build
    build.build()
    return _lib.load()


def _close(a, b, rel=1e-10):
    assert a.shape == b.shape and float((a - b).abs().max()) <= rel * max(float(b.abs().max()), 1e-300)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_symbols_and_sizes(lib):
    names = [s[0] for s in _lib.SYMBOLS]
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "uavsal_hip.h")).read()
    for n in ("uavsal_ir_sums_s2", "uavsal_ir_sums_s2_slabs", "uavsal_ir_sums_s2_slab_rows", "uavsal_ir_sums_s2_workspace_bytes",
              "uavsal_mp_sizeof_desc"):
        assert n in names and hasattr(lib, n) and n + "(" in hdr
    assert _lib.MP_DESC_TYPES == [_lib.IrSumsS2Desc]
    assert lib.uavsal_mp_sizeof_desc(0) == C.sizeof(_lib.IrSumsS2Desc) == C.sizeof(_lib.IrSumsDesc)
    assert lib.uavsal_mp_sizeof_desc(1) < 0 and lib.uavsal_mp_sizeof_desc(-1) < 0
    assert lib.uavsal_ctx_sizeof_desc(3) < 0 and lib.uavsal_abi_version() == 20               # the older lists stay closed
    assert len(_lib.DESC_TYPES) == 20 and lib.uavsal_sizeof_desc(20) < 0
    for n in ("ir_sums_s2", "prior_path_backward", "prior_path_blocks", "fust_output_grad", "block_param_grads"):
        assert callable(getattr(train, n))
    assert train.PRIOR_PATH_BLOCKS == MP.PATH_BLOCKS and _lib.IR_NSUM == MP.NSUM == 11


def test_slab_count_of_the_stride_2_sums_is_the_restated_partition(lib):
    d = _lib.IrSumsS2Desc()
    for (n, H, W, Ch, Co) in MP.SUMS_SHAPES + [(4, 45, 80, 1536, 64), (20, 23, 40, 384, 64), (300, 4, 4, 64, 64), (1, 7, 300, 64, 64),
                                              (2000, 5, 300, 64, 8)]:
        d.n_img, d.H, d.W, d.Ch, d.Co = n, H, W, Ch, Co
        sr, slabs = MP.slab_partition_s2(n, H, W)
        assert lib.uavsal_ir_sums_s2_slab_rows(C.byref(d)) == sr and lib.uavsal_ir_sums_s2_slabs(C.byref(d)) == slabs, (n, H, W)
        assert lib.uavsal_ir_sums_s2_workspace_bytes(C.byref(d)) == slabs * (11 * Ch + Co) * 8
        assert slabs <= 256 and sr * slabs >= n * X.down(H) > sr * (slabs - 1)
    assert MP.slab_partition_s2(1, 45, 80) == (2, 12) and MP.slab_partition_s2(2, 23, 40) == (4, 6)      # a slab across two images
    assert MP.slab_partition_s2(2000, 5, 300) == (24, 250)                                                    # the cap on the slab count
    d.Ch = 96
    assert lib.uavsal_ir_sums_s2_slabs(C.byref(d)) == 0 and lib.uavsal_ir_sums_s2_workspace_bytes(C.byref(d)) == 0


def test_gemm_share_count_with_an_m_tail_is_the_restated_partition(lib):
    d = _lib.PixGemmDesc()
    for M in (64, 128, 192, 320, 1536):
        for N in (64, 128, 384, 1152, 1536):
            for K in MP.GEMM_K + (35, 920, 3600, 20 * 45 * 80, 4 * 23 * 40):
                d.K, d.M, d.N = K, M, N
                cps, shares = MP.gemm_partition(K, M, N)
                assert lib.uavsal_pix_gemm_shares(C.byref(d)) == shares, (M, N, K)
                assert lib.uavsal_pix_gemm_workspace_bytes(C.byref(d)) == shares * M * N * 4
                if M % 128 == 0:                                             # whole M tiles keep the partition they had
                    assert (cps, shares) == BR.gemm_partition(K, M, N)[:2]
    # M = 64 and M = 128 are one M tile each: the same shares for every K (the GPU test compares their bits)
    for K in (1, 1025, 72000):
        assert MP.gemm_partition(K, 64, 384) == MP.gemm_partition(K, 128, 384)
    for M in (32, 96, 400, 1500):
        d.K, d.M, d.N = 1000, M, 64
        assert lib.uavsal_pix_gemm_shares(C.byref(d)) == 0 and lib.uavsal_pix_gemm_workspace_bytes(C.byref(d)) == 0


def test_argument_validation_without_gpu(lib):
    s = _lib.IrSumsS2Desc()
    assert lib.uavsal_ir_sums_s2(C.byref(s), None) == -1
    s.gd = s.d = s.e = s.ga = s.go = s.ws = 256
    s.n_img, s.H, s.W, s.Ch, s.Co, s.ldgo = 1, 5, 7, 96, 64, 64
    assert lib.uavsal_ir_sums_s2(C.byref(s), None) == -3                  # Ch % 64: UAVSAL_ESHAPE
    s.Ch, s.Co = 64, 62
    assert lib.uavsal_ir_sums_s2(C.byref(s), None) == -2
    s.Co, s.ldgo = 64, 32
    assert lib.uavsal_ir_sums_s2(C.byref(s), None) == -1                  # rows shorter than Co
    s.ldgo = 64
    assert lib.uavsal_ir_sums_s2(C.byref(s), None) == -1                  # accepted so far: the workspace is too small
    s.ws_bytes = lib.uavsal_ir_sums_s2_workspace_bytes(C.byref(s))
    s.e = 260
    assert lib.uavsal_ir_sums_s2(C.byref(s), None) == -2
    s.e, s.W = 256, 0
    assert lib.uavsal_ir_sums_s2(C.byref(s), None) == -1
    g = _lib.PixGemmDesc()
    g.a = g.b = g.ws = g.out = 256
    g.K, g.M, g.N, g.lda, g.ldb, g.ldo = 100, 96, 64, 96, 64, 64
    assert lib.uavsal_pix_gemm(C.byref(g), None) == -3                    # M % 64
    g.M, g.lda = 64, 64
    assert lib.uavsal_pix_gemm(C.byref(g), None) == -1                    # accepted: the workspace is too small
    g.ws_bytes = lib.uavsal_pix_gemm_workspace_bytes(C.byref(g))
    g.lda = 32
    assert lib.uavsal_pix_gemm(C.byref(g), None) == -1                    # rows shorter than M


# ------------------------------------------------------------------------------------------------ refusals
def _blk(name, shape=(1, 3, 5)):
    from iip_uavsal_saliency_amd.model import dwBlock
    return X.make_block(name, X.block_case(name, shape)[1], dwBlock)


def test_python_entry_points_refuse_what_they_do_not_cover():
    from iip_uavsal_saliency_amd import UAVSal
    from iip_uavsal_saliency_amd.model import dwBlock
    for name in MP.TRAINED:
        assert len(train._param_grad_parts(_blk(name))) == 6
    blk = _blk("ctx0")
    x, g = torch.zeros(2, 256, 5, 7), torch.zeros(2, 64, 3, 4)
    with pytest.raises(RuntimeError, match="cuda"):                       # stride 2 and Cout = 64 are taken: the tensors are not
        train.block_param_grads(blk, x, None, None, g)
    with pytest.raises(RuntimeError, match="cuda"):
        train.block_param_grads(_blk("fucb192"), torch.zeros(2, 192, 5, 7), None, None, torch.zeros(2, 64, 5, 7))
    with pytest.raises(RuntimeError, match="eval"):
        train.block_param_grads(blk.train(), x, None, None, g)
    for bad in (dwBlock(256, 64, kernel_size=3, expand_ratio=1), dwBlock(256, 64, kernel_size=3, dilation=6),
                dwBlock(20, 64, kernel_size=3), dwBlock(256, 32, kernel_size=3), dwBlock(256, 8, kernel_size=3, stride=2)):
        with pytest.raises(RuntimeError, match="expand conv|Cout"):
            train.block_param_grads(bad.eval(), x, None, None, g)
    odd = dwBlock(64, 64, kernel_size=3, stride=2).eval()
    odd.use_res_connect = True
    with pytest.raises(RuntimeError, match="residual"):
        train.block_param_grads(odd, x, None, None, g)
    t = torch.zeros(1, 4, 4, 64)
    with pytest.raises(RuntimeError, match="cuda"):
        train.ir_sums_s2(torch.zeros(1, 2, 2, 64), torch.zeros(1, 2, 2, 64), t, t, torch.zeros(1, 64, 2, 2))
    m = UAVSal(time_dims=2).eval()
    fu, cb, gf = torch.zeros(4, 320, 5, 7), torch.zeros(4, 192, 5, 7), torch.zeros(4, 320, 5, 7)
    assert tuple(train.prior_path_blocks(m)) == train.PRIOR_PATH_BLOCKS
    assert list(train.prior_path_blocks(m).values()) == [m.fucb_layer[0], m.cxt_cb_prior[1], m.cxt_cb_prior[0]]
    m110 = UAVSal(time_dims=2, bias_type=[1, 1, 0]).eval()
    assert list(train.prior_path_blocks(m110).values()) == [m110.fucb_layer[0]]
    m0 = UAVSal(time_dims=2, bias_type=[0, 0, 0]).eval()
    assert train.prior_path_blocks(m0) == {}
    grads = {n: None for n in train.PRIOR_PATH_BLOCKS}
    with pytest.raises(RuntimeError, match="cuda"):
        train.prior_path_backward(m, fu, cb, gf, grads=dict(grads))
    with pytest.raises(RuntimeError, match="eval"):
        train.prior_path_backward(m.train(), fu, cb, gf, grads=dict(grads))
    m.eval()
    with pytest.raises(RuntimeError, match="blocks of this model's prior path"):
        train.prior_path_backward(m110, fu, cb, gf, grads=dict(grads))
    with pytest.raises(RuntimeError, match="blocks of this model's prior path"):
        train.prior_path_backward(m, fu, cb, gf, grads={})
    with pytest.raises(RuntimeError, match="accumulate needs"):
        train.prior_path_backward(m, fu, cb, gf, grads=dict(grads), accumulate=True)
    with pytest.raises(RuntimeError, match="prior"):
        train.prior_path_backward(m0, fu, cb, gf, grads=dict(grads))
    # the step: ctx needs fuse and a model with priors; it does not need fust
    for model, kw in ((m, dict(ctx=True)), (m, dict(decoder=True, ctx=True)), (m, dict(decoder=True, fust=True, ctx=True)),
                      (m0, dict(fuse=True, ctx=True))):
        with pytest.raises(RuntimeError, match="fuse=True and a model with at least one prior"):
            train.recurrence_step(model, fu, None, None, fu, **kw)
    with pytest.raises(RuntimeError, match="ctx=True needs"):
        train.recurrence_step(m0, fu, None, None, fu, fuse=True, ctx=True)
    with pytest.raises(RuntimeError, match="eval"):
        train.recurrence_step(m.train(), fu, None, None, fu, fuse=True, ctx=True)
    with pytest.raises(RuntimeError, match="cuda"):
        train.recurrence_step(m.eval(), fu, None, None, fu, fuse=True, ctx=True)


def test_stages_of_the_driver():
    for stages in (("rnn", "ctx"), ("rnn", "decoder", "ctx"), ("rnn", "fuse", "ctx", "fust"), ("rnn", "fuse", "ctx", "ctx"),
                   ("rnn", "ctx", "fuse"), ("ctx",), ("fuse", "ctx"), ("rnn", "fust", "ctx")):
        with pytest.raises(ValueError, match="stages"):
            stream.finetune_video(None, None, None, None, None, None, None, stages=stages)


class _Stub:
    time_dims = 5

    def __init__(self, context):
        self.rnn, self.conv_out_st, self.fucbst_layer, self.fust_layer = object(), object(), object(), object()
        self.fucb_layer, self.cxt_cb_prior = object(), object()
        self.num_cb, self.use_context_prior, self.refreshed = 3 if context else 2, context, []
        self.w = torch.nn.Parameter(torch.zeros(1))

    def parameters(self):
        return iter([self.w])

    def refresh_weights(self, *mods):
        self.refreshed.append(mods)


class _Opt:
    def zero_grad(self):
        pass

    def step(self):
        pass


def test_finetune_video_with_the_ctx_stage(monkeypatch):
    n = 20
    frames = torch.zeros(n, 3, 72, 128, dtype=torch.uint8)
    has = torch.ones(n, 2, dtype=torch.bool)
    seen = []

    def step(model, x, cb, state, y, criterion, **kw):
        seen.append(kw)
        return torch.tensor(1.0), None, [torch.tensor(0.0)]
    monkeypatch.setattr(train, "recurrence_step", step)
    fix = torch.zeros(n, 4, 4, dtype=torch.uint8)
    for stages in (("rnn", "decoder", "fuse", "fust", "ctx"), ("rnn", "fuse", "fust", "ctx"), ("rnn", "fuse", "ctx"),
                   ("rnn", "decoder", "fuse", "ctx")):
        for context in (True, False):
            m = _Stub(context)
            del seen[:]
            r = stream.finetune_video(m, frames, torch.zeros(8, 9, 16), torch.zeros(20, 9, 16), fix, fix, _Opt(), batch_size=2,
                                      criterion=object(), prepare=lambda a, b, h, w, l: (torch.zeros(n, 2, h, w), has), stages=stages)
            assert r["groups_run"] == 2 and seen == [{s: True for s in stages[1:]}] * 2
            want = (m.rnn,) + ((m.conv_out_st,) if "decoder" in stages else ()) + (m.fucbst_layer,)
            want += ((m.fust_layer,) if "fust" in stages else ()) + (m.fucb_layer,) + ((m.cxt_cb_prior,) if context else ())
            assert m.refreshed == [want] * 2


# ------------------------------------------------------------------------------------------------ routes
def test_every_gemm_of_the_trained_path_has_a_route(lib):
    """The 1x1 GEMMs the walk sends for a trained block (Co -> Ch with the transposed projection, Ch -> Cin with the transposed
    expand; the forward's own expand Cin -> Ch and ctx0's projection) at the map sizes of the path, and the two pixel GEMMs of
    every block's weight gradients (M = Ch, N = Cin and M = Co = 64, N = Ch)."""
    sent, pix = set(), set()
    for name in MP.TRAINED:
        cin, hid, cout, _ = X.BLOCKS[name]
        sent |= {(cout, hid), (hid, cin), (cin, hid), (hid, cout)}
        pix |= {(hid, cin), (cout, hid)}
    for (ci, co) in sorted(sent):
        for (n, h, w) in ((20, 45, 80), (4, 45, 80), (4, 23, 40), (4, 12, 20), (2, 9, 13), (2, 5, 7), (2, 3, 4), (1, 1, 1)):
            d = _lib.ConvDesc()
            d.a, d.lda, d.a_img_stride = 1 << 20, ci, h * w
            d.out, d.ldc, d.o_img_stride = 1 << 21, co, h * w
            d.n_img, d.H, d.W, d.Cin, d.Cout, d.taps = n, h, w, ci, co, 1
            d.prec, d.act, d.epi, d.tile = _lib.PREC["f32"], _lib.ACT_NONE, _lib.EPI_AFFINE, 0
            d.w = 1 << 20
            rt = _lib.conv_route(lib, d)
            layout = P.conv_weight_layout("f32", False, False, rt.tile, 1)
            assert P.pack_conv_weight(torch.zeros(co, ci, 1, 1), layout).numel() >= ci * co, (ci, co, rt)
    assert (64, 1536) in pix and (64, 384) in pix and (1152, 192) in pix
    g = _lib.PixGemmDesc()
    for (M, N) in sorted(pix):
        for K in (1, 2 * 3 * 4, 4 * 9 * 13, 20 * 45 * 80):
            g.K, g.M, g.N = K, M, N
            assert lib.uavsal_pix_gemm_shares(C.byref(g)) >= 1, (M, N, K)


# ------------------------------------------------------------------------------------------------ refresh in place
def _entry_tensors(ent):
    return [ent[k] for k in sorted(ent)]


def test_a_natural_fused_entry_refreshes_in_place_and_a_transposed_one_still_raises():
    blk = _blk("fucb64")                                                  # 64 -> 384 -> 64, stride 1: fucb_layer[0] with one prior
    dwc = blk.conv[1][0]
    store = {}
    c = WeightCache("cpu", store)
    ent = c.fused_block(blk, True)
    assert list(store) == [("fused", id(dwc), True)] and sorted(ent) == ["b1", "b2", "bd", "s1", "s2", "sd", "w1", "w2", "wd"]
    assert torch.equal(ent["w1"], blk.conv[0][0].weight.detach().reshape(384, 64))      # the module's own [Cout][Cin]
    assert torch.equal(ent["w2"], blk.conv[2].weight.detach().reshape(64, 384))
    ptrs = [t.data_ptr() for t in _entry_tensors(ent)]
    before = [t.clone() for t in _entry_tensors(ent)]
    with torch.no_grad():
        for p_ in blk.parameters():
            p_.mul_(1.25).add_(0.01)
    mods = {id(m): m for m in blk.modules()}
    assert c.refresh(mods, dry=True) == 1
    assert all(torch.equal(a, b) for a, b in zip(before, _entry_tensors(ent)))            # the dry pass copies nothing
    assert c.refresh(mods) == 1 and list(store) == [("fused", id(dwc), True)] and store[("fused", id(dwc), True)] is ent
    assert ptrs == [t.data_ptr() for t in _entry_tensors(ent)]
    fresh = WeightCache("cpu", {}).fused_block(blk, True)
    for k in ent:
        assert ent[k].dtype == fresh[k].dtype and ent[k].shape == fresh[k].shape and torch.equal(ent[k], fresh[k]), k
    assert not any(torch.equal(a, b) for a, b in zip(before, _entry_tensors(ent)))
    # the container rule of the depthwise entries: the conv alone does not name its neighbours
    with pytest.raises(RuntimeError, match="whole block"):
        c.refresh({id(dwc): dwc}, dry=True)
    # a block without an expand conv has no w1 / s1 / b1, and refreshes the same way
    from iip_uavsal_saliency_amd.model import dwBlock
    b1 = dwBlock(64, 64, kernel_size=3, expand_ratio=1).eval()
    c1 = WeightCache("cpu", {})
    e1 = c1.fused_block(b1, True)
    with torch.no_grad():
        for p_ in b1.parameters():
            p_.mul_(0.5).add_(0.02)
    assert sorted(e1) == ["b2", "bd", "s2", "sd", "w2", "wd"] and c1.refresh({id(m): m for m in b1.modules()}) == 1
    f1 = WeightCache("cpu", {}).fused_block(b1, True)
    assert all(torch.equal(e1[k], f1[k]) for k in e1)
    # the transposed layout of csrc/fused_ir.hip keeps raising, before anything is copied
    c.fused_block(blk, False)
    kept = [t.clone() for t in _entry_tensors(ent)]
    with torch.no_grad():
        for p_ in blk.parameters():
            p_.add_(0.5)
    with pytest.raises(NotImplementedError, match="invalidate_engines"):
        c.refresh(mods, dry=True)                                         # the pass model.refresh_weights makes first
    assert all(torch.equal(a, b) for a, b in zip(kept, _entry_tensors(ent)))


# ------------------------------------------------------------------------------------------------ restatements vs autograd
def _gd_formula(gd, d, e):
    """Gd of include/uavsal_hip.h written out pixel by pixel (slow: small shapes)."""
    n, c, Ho, Wo = d.shape
    H, W = e.shape[2:]
    d2 = gd * X.m6(d)
    out = torch.zeros(c, 3, 3, dtype=torch.float64)
    for oy in range(Ho):
        for ox in range(Wo):
            for ky in range(3):
                for kx in range(3):
                    y, x = 2 * oy - 1 + ky, 2 * ox - 1 + kx
                    if 0 <= y < H and 0 <= x < W:
                        out[:, ky, kx] += (d2[:, :, oy, ox] * e[:, :, y, x]).sum(0)
    return out


@pytest.mark.parametrize("shape", [(1, 1, 1, 8, 4), (2, 3, 2, 8, 4), (1, 5, 7, 8, 4), (2, 4, 6, 8, 4), (1, 2, 1, 8, 4)], ids=str)
def test_sums_restatement_is_the_formula_and_autograd(shape):
    gd, d, e, ga, go = (t64(a) for a in MP.sums_case(shape))
    s, b = MP.ir_sums_s2_ref(gd, d, e, ga, go, bounds=True)
    _close(s["Gd"], _gd_formula(gd, d, e), 1e-13)
    _close(s["S1"], ga.sum((0, 2, 3)), 1e-13)
    _close(s["S3"], go.sum((0, 2, 3)), 1e-13)
    assert all(bool((b[k] >= 0).all()) for k in b)
    # Gd is the gradient of the stride-2 depthwise conv with respect to its weights
    wd = torch.zeros(shape[3], 1, 3, 3, dtype=torch.float64, requires_grad=True)
    pre = torch.nn.functional.conv2d(e, wd, padding=1, stride=2, groups=shape[3])
    assert pre.shape == d.shape
    (want,) = torch.autograd.grad(pre, wd, gd * X.m6(d))
    _close(s["Gd"], want[:, 0], 1e-13)


@pytest.mark.parametrize("name", MP.TRAINED)
def test_block_restatement_is_autograd(name):
    cin, _, cout, stride = X.BLOCKS[name]
    res = stride == 1 and cin == cout
    for shape in ((1, 3, 5), (2, 5, 6), (2, 4, 4)):
        x, q, go = X.block_case(name, shape)
        q64 = BR.to64(q)
        p = BR.fold(q64)
        want = MP.autograd_grads(q64, t64(x), t64(go), stride, res)
        got, bound = MP.param_grads(p, t64(x), t64(go), stride, bounds=True)
        for n in BR.NAMES:
            _close(got[n], want[n])
            assert bool((bound[n] >= 0).all()) and got[n].shape == bound[n].shape
        if stride == 1:                                                   # block_ref64's closed form is the stride-1 case
            old, oldb = BR.param_grads(q64, t64(x), t64(go), bounds=True)
            for n in BR.NAMES:
                _close(got[n], old[n], 1e-13)
                _close(bound[n], oldb[n], 1e-12)


HEAD, T = (4, 5, 7), 2                  # N = 4 frames as B = 2 chunks of T = 2


def _head(bias, shape=HEAD):
    Q, st, priors, go = X.head_case(bias, shape, T)
    Pf = X.folds(Q)
    pri = t64(priors) if priors is not None else None
    hd = X.head_forward(Pf, t64(st), pri, T, use_ctx=bool(bias[2]))
    gfu = X.input_grad_ref(Pf["fucbst"], hd["fu"], t64(go), 1, False)
    return Q, Pf, hd, pri, gfu


@pytest.mark.parametrize("bias", [(1, 1, 1), (0, 0, 1), (1, 0, 1), (1, 1, 0)], ids=str)
def test_path_restatement_is_autograd(bias):
    Q, Pf, hd, pri, gfu = _head(bias)
    got = MP.path_param_grads(Pf, hd["fu"], hd["cbcat"], gfu, T, bias[0] + bias[1])
    want = MP.path_autograd({k: BR.to64(q) for k, q in Q.items()}, hd["f"].detach(), pri, gfu, T, bool(bias[2]))
    assert list(got) == list(want) == list(MP.PATH_BLOCKS[:3 if bias[2] else 1])
    for name in got:
        for n in BR.NAMES:
            _close(got[name][n], want[name][n])
    # ... and autograd of the loss behind fucbst gives the same: gfu carries everything behind fu
    if bias == (1, 1, 1):
        q = BR.to64(Q["ctx0"])
        keys = ("w1", "g1", "be1", "wd", "g2", "be2", "w3", "g3", "be3")
        leaves = {k: q[k].detach().clone().requires_grad_(True) for k in keys}
        qq = dict(q)
        qq.update(leaves)
        Pl = dict(Pf)
        Pl["ctx0"] = BR.fold(qq)
        o = X.tail_forward(Pl, hd["f"].detach(), pri, T)["o"]
        go = t64(X.head_case(bias, HEAD, T)[3])
        for n, a in zip(BR.NAMES, torch.autograd.grad(o, [leaves[k] for k in keys], go)):
            _close(got[MP.PATH_BLOCKS[2]][n], a)


@pytest.mark.parametrize("bias", MP.GOLDEN_BIAS, ids=str)
def test_closed_form_matches_the_reference_autograd(bias, golden_dir):
    """tests/golden/ctx_train_*.npz: the reference's own dwBlock through model.py:344-365 under autograd
    (tools/make_ctx_goldens.py)."""
    g = np.load(os.path.join(golden_dir, MP.golden_name(bias) + ".npz"))
    Q, st, priors, go = X.head_case(bias, MP.GOLDEN_SHAPE, MP.GOLDEN_T)
    assert str(g["digest"]) == MP.path_digest(Q, st, priors, go) and int(g["T"]) == MP.GOLDEN_T
    Pf = X.folds(Q)
    hd = X.head_forward(Pf, t64(st), t64(priors) if priors is not None else None, MP.GOLDEN_T, use_ctx=bool(bias[2]))
    gfu = X.input_grad_ref(Pf["fucbst"], hd["fu"], t64(go), 1, False)
    got = MP.path_param_grads(Pf, hd["fu"], hd["cbcat"], gfu, MP.GOLDEN_T, bias[0] + bias[1])
    assert len(got) == (3 if bias[2] else 1)

    def close(a, b):
        assert a.shape == b.shape and float(np.abs(a - b).max()) <= 1e-10 * float(np.abs(b).max())
    for name, grads in got.items():
        key = MP.PATH_KEYS[name]
        for n in BR.NAMES:
            if n not in (BR.NAMES[0], BR.NAMES[6]):
                close(grads[n].numpy(), g["%s_%s" % (key, n.replace(".", "_"))])
        for tag, n in (("W1", BR.NAMES[0]), ("W3", BR.NAMES[6])):
            w = grads[n].numpy()[:, :, 0, 0]
            close(w[MP.W_SUBSET], g["%s_%s" % (key, tag)])
            l2 = float(g["%s_%s_l2" % (key, tag)])
            assert abs(float(w.sum()) - float(g["%s_%s_sum" % (key, tag)])) <= 1e-10 * l2 * np.sqrt(w.size)
            assert abs(float(np.sqrt((w * w).sum())) - l2) <= 1e-10 * l2


# ------------------------------------------------------------------------------------------------ sensitivity
@pytest.mark.parametrize("shape", [s for s in MP.SUMS_SHAPES if s[1] >= 3 and s[3] <= 384], ids=str)
def test_wrong_sums_lie_outside_the_bounds(shape):
    """The wrong variants of uavsal_ir_sums_s2 the GPU test must reject are at least 4 bounds from the right sums in float64."""
    gd, d, e, ga, go = (t64(a) for a in MP.sums_case(shape))
    s, b = MP.ir_sums_s2_ref(gd, d, e, ga, go, bounds=True)
    for v, k in (("stride1_e", "Gd"), ("no_top_pad", "Gd"), ("s1_output_grid", "S1")):
        wrong = MP.ir_sums_s2_ref(gd, d, e, ga, go, variant=v)
        assert float(((wrong[k] - s[k]).abs() / b[k].clamp_min(1e-300)).max()) >= 4.0, v
        for other in s:
            if other != k:
                assert torch.equal(wrong[other], s[other])


@pytest.mark.parametrize("bias", [(1, 1, 1), (0, 0, 1)], ids=str)
def test_a_per_frame_walk_lies_outside_the_bounds(bias):
    """cxt_cb_prior sees the chunk sums (B images): a walk that feeds it the N frames is at least 4 bounds away in every one of
    its tensors' worst element -- but for beta3 of cxt_cb_prior[1], the plain sum of the resize's adjoint over all images, which
    is the same number whichever images it was split over."""
    Q, Pf, hd, pri, gfu = _head(bias, MP.GOLDEN_SHAPE)
    k = bias[0] + bias[1]
    right = MP.path_inputs(Pf, hd["fu"], hd["cbcat"], gfu, T, k)
    wrong = MP.path_param_grads(Pf, hd["fu"], hd["cbcat"], gfu, T, k, variant="per_frame")
    for name in MP.PATH_BLOCKS[1:]:
        x, go, s = right[name]
        g, b = MP.param_grads(Pf[MP.PATH_KEYS[name]], x, go, s, bounds=True)
        for n in BR.NAMES:
            far = float(((wrong[name][n] - g[n]).abs() / b[n].clamp_min(1e-300)).max())
            if (name, n) == (MP.PATH_BLOCKS[1], BR.NAMES[8]):
                assert far <= 1e-6, far
            else:
                assert far >= 4.0, (name, n)
