"""The backward of the shallow backbone blocks (MobileNetV2 features[2:8]) without a GPU: the partition of the skinny
weight-gradient GEMM (uavsal_skinny_wgrad) restated in tests/shallow_ref64.py against the library's own host entry points, the
Ch % 16 opt-in of the channel sums, the float64 restatement of the five block shapes against torch.autograd and against goldens
recorded from the reference's own dwBlock, the power of the wrong variants on the inputs the GPU tests use, the refusals, and
that nothing pinned on uavsal_pix_gemm, uavsal_ir_sums or block_backward moved."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import _lib, model_feature, repack, train
from iip_uavsal_saliency_amd.model import dwBlock
from iip_uavsal_saliency_amd.weights import WeightCache

import block_ref64 as BR
import ctx_ref64 as X
import mp_ref64 as MP
import repack_ref as RR
import shallow_ref64 as SH

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ids3 = lambda p: "%dx%dx%d" % tuple(p)                                    # noqa: E731


def _close(a, b, rel=1e-9):
    return float((a - b).abs().max()) <= rel * max(float(b.abs().max()), 1e-300)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _far(wrong, want, bound):
    return float(((wrong - want).abs() / bound.clamp_min(1e-300)).max())


def _desc(K, M, N):
    d = _lib.SkinnyWgradDesc()
    d.K, d.M, d.N = K, M, N
    return d


def test_the_partition_through_the_host_entry_points(lib):
    assert SH.partition(70)[:2] == (128, 1) and SH.chains(70) == (70, 1)
    assert SH.partition(2760)[:2] == (128, 22) and SH.partition(2760)[2][-1] == (2688, 2760)      # the last share is ragged: 72 pixels
    assert SH.partition(20 * 360 * 640 // 4)[:2] == (1152, 1000)                                   # 96 x 16 at 20 frames: two chains a share
    assert SH.partition(SH.K_CHAINS)[:2] == (1152, 912) and SH.chains(SH.K_CHAINS) == (1024, 2)
    p0, p1 = SH.partition(SH.K_CHAINS)[2][-1]
    assert p1 - p0 == 91
    for K in [p[0] * p[1] * p[2] for p in SH.GEMM_K] + [1, 127, 128, 129, 128 * 1024, 128 * 1024 + 1, 18400, 72000, 288000, 1152000,
                                                         SH.K_CHAINS, 10 ** 9]:
        span, shares, spans = SH.partition(K) if K < 10 ** 8 else (None, None, None)
        for M, N in SH.GEMM + [(8, 8), (32, 32), (192, 32), (32, 192), (8, 192)]:
            assert SH.accepted(M, N)
            d = _desc(K, M, N)
            got = lib.uavsal_skinny_wgrad_shares(C.byref(d))
            assert 1 <= got <= SH.SHARES
            if shares is not None:
                assert got == shares, (K, M, N)                       # a function of K alone
                assert span % SH.UNIT == 0 and spans[-1][1] == K and (shares - 1) * span < K <= shares * span
            assert lib.uavsal_skinny_wgrad_workspace_bytes(C.byref(d)) == got * M * N * 4
            g, spg = SH.reduce_groups(N, got)
            assert g * N <= 1024 and g * spg >= got
    assert C.sizeof(_lib.SkinnyWgradDesc) == lib.uavsal_shallow_sizeof_desc(0) and lib.uavsal_shallow_sizeof_desc(1) < 0


def test_refusals_by_code(lib):
    for M, N in SH.GEMM_REFUSED + [(0, 8), (8, 0), (40, 33), (192, 40), (256, 32)]:
        assert not SH.accepted(M, N)
        d = _desc(2760, M, N)
        assert lib.uavsal_skinny_wgrad_shares(C.byref(d)) == 0 and lib.uavsal_skinny_wgrad_workspace_bytes(C.byref(d)) == 0
        d.a = d.b = d.ws = d.out = 256
        d.lda, d.ldb, d.ldo = 256, 256, 256
        assert lib.uavsal_skinny_wgrad(C.byref(d), None) == (-3 if M > 0 and N > 0 else -1), (M, N)      # UAVSAL_ESHAPE
    g = _desc(100, 144, 24)
    assert lib.uavsal_skinny_wgrad(C.byref(g), None) == -1                # null operands
    g.a = g.b = g.ws = g.out = 256
    g.lda, g.ldb, g.ldo = 144, 24, 24
    assert lib.uavsal_skinny_wgrad(C.byref(g), None) == -1                # accepted: the workspace is too small
    g.ws_bytes = lib.uavsal_skinny_wgrad_workspace_bytes(C.byref(g))
    g.lda = 140
    assert lib.uavsal_skinny_wgrad(C.byref(g), None) == -1                # rows shorter than M
    g.lda = 146
    assert lib.uavsal_skinny_wgrad(C.byref(g), None) == -2                # lda % 4
    g.lda, g.b = 144, 260
    assert lib.uavsal_skinny_wgrad(C.byref(g), None) == -2                # b not 16-byte aligned
    g.b, g.rowdot = 256, 256
    assert lib.uavsal_skinny_wgrad(C.byref(g), None) == -1                # rowdot without w
    d = _desc(0, 144, 24)
    assert lib.uavsal_skinny_wgrad_shares(C.byref(d)) == 0
    with pytest.raises(RuntimeError, match="cuda"):
        train.skinny_wgrad(torch.zeros(1, 2, 2, 144), torch.zeros(1, 2, 2, 24))


def test_what_pix_gemm_refuses_stays_refused(lib):
    """The new entry point is the only way in: uavsal_pix_gemm keeps refusing the five shapes, with and without tails32."""
    for M, N in SH.GEMM:
        for tails32 in (0, 1):
            d = _lib.PixGemmDesc()
            d.K, d.M, d.N, d.tails32 = 2760, M, N, tails32
            assert lib.uavsal_pix_gemm_shares(C.byref(d)) == 0, (M, N, tails32)


@pytest.mark.parametrize("M,N", SH.GEMM)
def test_gemm_wrong_variants_are_far(M, N):
    for pic in SH.GEMM_K:
        a, b, _, _, pad = (torch.as_tensor(t).double() for t in SH.gemm_inputs(M, N, pic))
        G, bound = SH.skinny_ref(a, b)
        K = pic[0] * pic[1] * pic[2]
        variants = [v for v, on in (("narrow_pad", N % 32), ("last_pixel", True), ("last_share", SH.partition(K)[1] > 1)) if on]
        for v in variants:
            assert _far(SH.skinny_ref(a, b, v, pad)[0], G, bound) >= 4.0, (M, N, pic, v)
        if not N % 32:
            assert torch.equal(SH.skinny_ref(a, b, "narrow_pad", pad)[0], G)


def test_a_dropped_share_is_far_where_a_share_holds_two_chains():
    """At K_CHAINS the worst-case bound is 1028 U of the absolute-value sum: with operands of one sign (the GPU test's) the
    last share of 91 pixels out of a million is 1.4 bounds only, a whole share of 1152 is more than 4."""
    K, M, N = SH.K_CHAINS, 96, 16
    L, c = SH.chains(K)
    assert (L, c) == (1024, 2)
    span, shares, spans = SH.partition(K)
    gen = torch.Generator().manual_seed(5)
    p0, p1 = spans[-2]                                              # a whole share; |a| |b| of the others enters through its mean
    a, b = torch.rand(p1 - p0, M, generator=gen, dtype=torch.float64), torch.rand(p1 - p0, N, generator=gen, dtype=torch.float64)
    part = a.T @ b                                                  # all positive: equal to its absolute-value sum
    total = part * (K / (p1 - p0))                                  # the mean share, K pixels' worth
    assert float((part / ((L + c + 2) * SH.U * total)).min()) >= 4.0


# ------------------------------------------------------------------------------------------------ the blocks of features[2:8]
@pytest.mark.parametrize("pic", SH.PICTURES, ids=ids3)
@pytest.mark.parametrize("name", list(SH.BLOCKS))
def test_block_closed_forms_equal_autograd_and_the_reference_goldens(name, pic):
    """tests/golden/shallow_*.npz: the reference's own dwBlock under float64 autograd (tools/make_shallow_goldens.py)."""
    cfg = SH.BLOCKS[name]
    x, q, go = SH.block_case(name, pic)
    z = np.load(os.path.join(GOLDEN, SH.golden_name(name, pic) + ".npz"))
    assert str(z["digest"]) == SH.golden_digest(x, q, go) and tuple(z["shape"]) == pic
    q64 = BR.to64(q)
    p = BR.fold(q64)
    x, go = torch.as_tensor(x).double(), torch.as_tensor(go).double()
    pt = {}
    closed = MP.param_grads(p, x, go, cfg[3], parts=pt)
    auto = MP.autograd_grads(q64, x, go, cfg[3], cfg[4])
    assert all(_close(closed[k], auto[k]) for k in SH.NAMES)
    for k, v in SH.golden_pack(closed).items():
        assert _close(torch.as_tensor(v), torch.as_tensor(z[k]), 1e-9), k
    gx = SH.conv_t(pt["ga"], p["w1"], p["s1"], res=go if cfg[4] else None)
    assert _close(gx, X.input_grad_autograd(p, x, go, cfg[3], cfg[4])) and _close(gx, torch.as_tensor(z["grad_x"]), 1e-9)
    for t in (pt["e"], pt["d"]):                                  # 0, 6 and the interior
        assert min(BR.class_shares(t)) > 0.02, (name, BR.class_shares(t))
    a, b = SH.make_block(cfg, q, model_feature.InvertedResidual), SH.make_block(cfg, q, dwBlock)
    assert [(n, tuple(v.shape)) for n, v in a.state_dict().items()] == [(n, tuple(v.shape)) for n, v in b.state_dict().items()]
    assert (a.stride, a.use_res_connect, a.dilation) == (b.stride, b.use_res_connect, b.dilation) == (cfg[3], cfg[4], 1)
    assert os.path.getsize(os.path.join(GOLDEN, SH.golden_name(name, pic) + ".npz")) < 77920      # the smallest backbone_*.npz


@pytest.mark.parametrize("pic", SH.PICTURES, ids=ids3)
@pytest.mark.parametrize("name", list(SH.BLOCKS))
def test_block_wrong_variants_are_far(name, pic):
    """The stride-2 window anchored as on an unpadded grid (b2, b4, b7); the residual gradient dropped (b3, b5); an outside
    gradient that the walk adds at the block's input (g_c3 at block 7: backbone_ref64's "no_g_c4" is that variant) dropped."""
    cfg = SH.BLOCKS[name]
    x, q, go = SH.block_case(name, pic)
    x, go = torch.as_tensor(x).double(), torch.as_tensor(go).double()
    p = BR.fold(BR.to64(q))
    pt = MP.block_parts(p, x, go, cfg[3])
    res = torch.as_tensor(np.random.RandomState(7).standard_normal(tuple(x.shape))) / (x.shape[2] * x.shape[3]) if not cfg[4] else None
    want = SH.block_stage(p, cfg, x, go, pt, res=res)
    for v in (("no_residual",) if cfg[4] else ("s2_anchor", "no_g_c4")):
        wrong = SH.block_stage(p, cfg, x, go, pt, res=res, variant=v)
        key = "ga" if v == "s2_anchor" else "grad_x"
        assert _far(wrong[key][0], want[key][0], want[key][1]) >= 4.0, (name, v)


@pytest.mark.parametrize("stride", (1, 2))
@pytest.mark.parametrize("Ch", SH.SUMS_CH)
def test_sums_wrong_variants_are_far(Ch, stride):
    for pic in SH.SUMS_PICTURES:
        t = [torch.as_tensor(v).double() for v in SH.sums_case(pic, Ch, 24, stride)]
        S, b = SH.sums_ref(*t, stride)
        for v in ("last_group",) + (("s2_anchor",) if stride == 2 else ()):
            W, _ = SH.sums_ref(*t, stride, variant=v)
            assert max(_far(W[k], S[k], b[k]) for k in ("S2", "Gd", "S1")) >= 4.0, (pic, v)


def test_sums_ch16_through_the_host_entry_points(lib):
    """Without the opt-in the refusal of Ch % 64 != 0 stays; with it the slabs are those of the shape, whatever Ch."""
    for cls, name in ((_lib.IrSumsDesc, "uavsal_ir_sums"), (_lib.IrSumsS2Desc, "uavsal_ir_sums_s2")):
        for Ch in (96, 144, 16, 192, 24):
            d = cls()
            d.n_img, d.H, d.W, d.Ch, d.Co = 2, 23, 40, Ch, 24
            slabs, nbytes = getattr(lib, name + "_slabs"), getattr(lib, name + "_workspace_bytes")
            ref = cls()
            ref.n_img, ref.H, ref.W, ref.Ch, ref.Co = 2, 23, 40, 64, 24
            want = slabs(C.byref(ref))
            assert want > 1
            assert slabs(C.byref(d)) == (want if Ch % 64 == 0 else 0)
            d.ch16 = 1
            assert slabs(C.byref(d)) == (want if Ch % 16 == 0 else 0), (name, Ch)
            assert nbytes(C.byref(d)) == (want * (_lib.IR_NSUM * Ch + 24) * 8 if Ch % 16 == 0 else 0)
            d.gd = d.d = d.e = d.ga = d.go = d.ws = 256
            d.ldgo = 24
            assert getattr(lib, name)(C.byref(d), None) == (-1 if Ch % 16 == 0 else -3)      # accepted: the workspace is too small
            d.ch16 = 0
            assert getattr(lib, name)(C.byref(d), None) == (-1 if Ch % 64 == 0 else -3)
    assert C.sizeof(_lib.IrSumsDesc) == lib.uavsal_block_sizeof_desc(1) == C.sizeof(_lib.IrSumsS2Desc) == lib.uavsal_mp_sizeof_desc(0)
    assert C.sizeof(_lib.IrSumsDilDesc) == lib.uavsal_srf_sizeof_desc(2)
    f = _lib.IrFinishDesc()
    for n, _ in _lib.IrFinishDesc._fields_:
        if n not in ("ws_bytes", "Ch", "Co", "slabs", "accumulate"):
            setattr(f, n, 256)
    f.Ch, f.Co, f.slabs = 96, 24, 1
    assert lib.uavsal_ir_finish(C.byref(f), None) == -3 and lib.uavsal_ir_finish_c16(C.byref(f), None) == -1      # refused; accepted, ws too small
    f.Ch = 24
    assert lib.uavsal_ir_finish_c16(C.byref(f), None) == -3


def test_block_refusals_by_name():
    blk = SH.make_block(SH.BLOCKS["b3"], SH.block_case("b3", SH.PICTURES[0])[1], model_feature.InvertedResidual)
    x, g = torch.zeros(1, 24, 4, 4), torch.zeros(1, 24, 4, 4)
    with pytest.raises(RuntimeError, match="cuda"):
        train.block_backward(blk, x, g, shallow=True)
    for kw in ({}, {"backbone": True}):                                    # without the keyword every refusal stays
        with pytest.raises(RuntimeError, match="Cout|Cin|hidden"):
            train.block_backward(blk, x, g, **kw)
    with pytest.raises(RuntimeError, match="eval"):
        train.block_backward(blk.train(), x, g, shallow=True)
    blk.eval()
    no_expand = model_feature.InvertedResidual(32, 16, 1, 1).eval()        # features[1]: no expand conv
    with pytest.raises(RuntimeError, match="expand conv"):
        train.block_backward(no_expand, torch.zeros(1, 32, 4, 4), torch.zeros(1, 16, 4, 4), shallow=True)
    with pytest.raises(RuntimeError, match="Cout %% 8|Cout % 8"):
        train.block_backward(dwBlock(24, 20, kernel_size=3).eval(), x, torch.zeros(1, 20, 4, 4), shallow=True)
    with pytest.raises(RuntimeError, match="dilated block with stride 2"):
        train.block_backward(dwBlock(24, 24, kernel_size=3, stride=2, dilation=2).eval(), x, g, shallow=True)


# ------------------------------------------------------------------------------------------------ the walk
def test_shallow_names_the_54_parameters_in_order():
    feats = model_feature.mobilenet_v2_features()
    names = ["%d.%s" % (i, n) for i in range(2, 8) for n, _ in feats[i].named_parameters()]
    assert tuple(names) == train.SHALLOW_PARAMS == SH.PARAMS and len(names) == 54
    assert (train.SHALLOW_FIRST, train.SHALLOW_END, train.SHALLOW_C3) == (SH.FIRST, SH.END, SH.C3)
    holder = type("M", (), {"features": type("F", (), {"features": feats})()})()
    assert [id(b) for b in train.shallow_blocks(holder)] == [id(feats[i]) for i in range(2, 8)]
    for i in range(2, 8):
        cin, hid, cout, stride, res = SH.FEATURES[i]
        assert tuple(feats[i].conv[0][0].weight.shape[:2]) == (hid, cin) and feats[i].conv[2].weight.shape[0] == cout
        assert (feats[i].stride, feats[i].use_res_connect) == (stride, res)
    assert feats[1].expand_ratio == 1 and len(list(feats[1].parameters())) + len(list(feats[0].parameters())) == 9      # what stays frozen


@pytest.mark.parametrize("frame", SH.FRAMES, ids=ids3)
def test_chain_closed_forms_equal_autograd_and_wrong_walks_are_far(frame):
    feats = model_feature.mobilenet_v2_features()
    x, Q, g3, g7 = SH.chain_case(frame, feats)
    Q = {i: BR.to64(q) for i, q in Q.items()}
    P = {i: BR.fold(q) for i, q in Q.items()}
    x1 = SH.frozen_forward(feats, torch.as_tensor(x))[1]
    g3, g7 = torch.as_tensor(g3).double(), torch.as_tensor(g7).double()
    keep = {}
    closed = SH.chain_closed(P, x1, g3, g7, keep=keep)
    auto = SH.chain_autograd(Q, x1, g3, g7)
    assert sorted(closed) == sorted(SH.PARAMS)
    for k in SH.PARAMS:
        assert _close(closed[k], auto[k], 1e-8), k
    n, H, W = frame
    assert tuple(x1.shape) == (n, 16, SH.down(H), SH.down(W)) and tuple(keep["x6"].shape) == tuple(g3.shape) and tuple(keep["x7"].shape) == tuple(g7.shape)
    for i in range(SH.FIRST, SH.END):
        for t in (keep["e%d" % i], keep["d%d" % i]):
            assert min(BR.class_shares(t)) > 0.02, (i, BR.class_shares(t))
    # each wrong walk is at least 4 stage bounds away at the block that meets it first
    for v, i in (("no_g_c3", 6), ("no_pass7", 6), ("no_residual", 5), ("no_residual", 2), ("s2_anchor", 7), ("s2_anchor", 4), ("s2_anchor", 2)):
        wrong = SH.chain_closed(P, x1, g3, g7, variant=v)
        xin = keep["x%d" % (i - 1)] if i > SH.FIRST else x1
        st = SH.FEATURES[i][3]
        pt = MP.block_parts(P[i], xin, keep["g%d" % i], st)
        _, b = MP.grads_from_parts(P[i], xin, pt["e"], pt["d"], pt["gd"], pt["ga"], keep["g%d" % i], st, bounds=True)
        assert max(_far(wrong["%d.%s" % (i, k)], closed["%d.%s" % (i, k)], b[k]) for k in SH.NAMES) >= 4.0, (v, i)
    no3 = SH.chain_autograd(Q, x1, g3, g7, variant="no_g_c3")              # ... and autograd's own gradients see a missing g_c3
    pt = MP.block_parts(P[6], keep["x5"], keep["g6"], 1)
    _, b = MP.grads_from_parts(P[6], keep["x5"], pt["e"], pt["d"], pt["gd"], pt["ga"], keep["g6"], 1, bounds=True)
    assert max(_far(no3["6." + k], auto["6." + k], b[k]) for k in SH.NAMES) >= 4.0


def test_walk_and_step_refusals_by_name():
    feats = model_feature.mobilenet_v2_features().eval()
    x, g3, g7 = torch.zeros(1, 3, 16, 16), torch.zeros(1, 32, 2, 2), torch.zeros(1, 64, 1, 1)
    with pytest.raises(RuntimeError, match="cuda"):
        train.shallow_backward(feats, x, g3, g7)
    with pytest.raises(RuntimeError, match="features.features"):
        train.shallow_backward(feats[:5], x, g3, g7)
    feats[4].train()
    with pytest.raises(RuntimeError, match="eval"):
        train.shallow_backward(feats, x, g3, g7)
    feats[4].eval()
    feats[1].train()
    with pytest.raises(RuntimeError, match="eval"):
        train.shallow_backward(feats, x, g3, g7)
    model = type("M", (), {"rnn_type": "twa", "num_cb": 0, "training": False})()
    with pytest.raises(RuntimeError, match="shallow=True needs backbone=True"):
        train.recurrence_step(model, None, None, None, None, fuse=True, st=True, srf=True, shallow=True)
    from iip_uavsal_saliency_amd import stream
    for stages in (("rnn", "shallow"), ("rnn", "fuse", "st", "srf", "shallow"), ("rnn", "fuse", "st", "srf", "shallow", "backbone"),
                   ("rnn", "fuse", "st", "srf", "backbone", "shallow", "shallow")):
        with pytest.raises(ValueError, match="stages"):
            stream.finetune_video(model, None, None, None, None, None, None, stages=stages)


# ------------------------------------------------------------------------------------------------ the refresh in place
@pytest.mark.parametrize("name", ["b2", "b3", "b7"])
def test_refresh_with_fused_t_remakes_a_transposed_layout_entry(name):
    """Host refresh with the keyword remakes the entry, in place, to the bytes of a freshly packed one; without it the
    NotImplementedError stays, message and all; `repack.entries` builds the same entry with the new COPY_T kind, and the kernel's
    per-element function restated over it (tests/repack_ref.py's conventions: `pack(e)` against `raw(e.dst)`) gives those bytes."""
    cfg = SH.BLOCKS[name]
    blk = SH.make_block(cfg, SH.block_case(name, SH.PICTURES[0])[1], model_feature.InvertedResidual)
    cache = WeightCache("cpu", {})
    stored = cache.fused_block(blk, False)
    (key,) = list(cache.store)
    assert key[0] == "fused" and key[2] is False and tuple(stored["w1"].shape) == (cfg[0], cfg[1]) and tuple(stored["w2"].shape) == (cfg[1], cfg[2])
    mods = {id(m): m for m in blk.modules()}
    msg = "packed 'fused' weights cannot be refreshed in place: call model.invalidate_engines()"
    for call in (lambda: cache.refresh(mods), lambda: cache.refresh(mods, dry=True), lambda: repack.entries(cache, mods)):
        with pytest.raises(NotImplementedError) as err:
            call()
        assert str(err.value) == msg
    where = {n: t.data_ptr() for n, t in stored.items()}
    old = {n: t.clone() for n, t in stored.items()}
    gen = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for t in list(blk.parameters()) + [b for b in blk.buffers() if b.dtype == torch.float32]:
            t.mul_(1.0 + 0.1 * torch.rand(t.shape, generator=gen)).add_(0.01 * torch.randn(t.shape, generator=gen))
    assert cache.refresh(mods, dry=True, fused_t=True) == 1
    assert all(torch.equal(stored[n], old[n]) for n in old)                                # the dry pass copies nothing
    ents = repack.entries(cache, mods, fused_t=True)                                       # (before the refresh: dst still holds the old bytes)
    assert [e.kind for e in ents] == [_lib.REPACK_COPY_T, _lib.REPACK_FOLD, _lib.REPACK_FOLD, _lib.REPACK_DW, _lib.REPACK_FOLD,
                                      _lib.REPACK_FOLD, _lib.REPACK_COPY_T, _lib.REPACK_FOLD, _lib.REPACK_FOLD]
    assert all(e.key == key for e in ents) and [(e.N, e.C) for e in ents if e.kind == _lib.REPACK_COPY_T] == [(cfg[1], cfg[0]), (cfg[2], cfg[1])]
    assert cache.refresh(mods, fused_t=True) == 1
    fresh = WeightCache("cpu", {}).fused_block(blk, False)
    for n in fresh:
        assert stored[n].data_ptr() == where[n] and np.array_equal(RR.raw(stored[n]), RR.raw(fresh[n])), n
        assert not torch.equal(stored[n], old[n]), n
    for e in ents:
        if e.kind == _lib.REPACK_COPY_T:                                                   # dst[c * N + n] = src[n * C + c]
            u = np.arange(e.units, dtype=np.int64)
            src = e.src[0].detach().reshape(-1).numpy()
            got = src[(u % e.N) * e.C + u // e.N].astype(np.float32).view(np.uint8)
            assert e.nbytes == got.size == 4 * e.N * e.C
        else:
            got = RR.pack(e)
        assert np.array_equal(got, RR.raw(e.dst)), (e.kind, e.layout)
    with pytest.raises(RuntimeError, match="pass the whole block"):                        # the dry pass raises when the block is missing
        cache.refresh({key[1]: mods[key[1]]}, dry=True, fused_t=True)
    stem = model_feature.mobilenet_v2_features()[0]                                        # the stem keeps raising either way
    sc = WeightCache("cpu", {})
    sc.stem(stem[0], stem[1])
    with pytest.raises(NotImplementedError, match="'stem'"):
        sc.refresh({id(m): m for m in stem.modules()}, fused_t=True)
    with pytest.raises(NotImplementedError, match="'stem'"):
        repack.entries(sc, {id(m): m for m in stem.modules()}, fused_t=True)
