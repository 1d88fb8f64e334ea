"""The deep backbone (MobileNetV2 features[8:18]) as a ninth training stage, without a GPU: the float64 restatement of
tests/backbone_ref64.py against torch.autograd, the power of its wrong variants on the inputs the GPU tests use, the share
partition of the `tails32` pixel GEMM against the library's own host entry points, and the refusals of the public surface."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import _lib, model_feature, stream, train
from iip_uavsal_saliency_amd.model import dwBlock, uavsal_srfnet_aspp

import backbone_ref64 as BK
import block_ref64 as BR
import ctx_ref64 as X
import mp_ref64 as MP
import srf_ref64 as SF

U = BK.U
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _far(wrong, want, bound):
    return float(((wrong - want).abs() / bound.clamp_min(1e-300)).max())


def _close(a, b, rel=1e-9):
    return float((a - b).abs().max()) <= rel * max(float(b.abs().max()), 1e-300)


def test_backbone_names_the_90_parameters_in_order():
    sf = uavsal_srfnet_aspp("mobilenet_v2")
    feats = sf.features.features
    want = ["%d.%s" % (i, n) for i in range(8, 18) for n, _ in feats[i].named_parameters()]
    assert len(train.BACKBONE_PARAMS) == 90 and list(train.BACKBONE_PARAMS) == want == list(BK.PARAMS)
    assert (train.BACKBONE_FIRST, train.BACKBONE_END, train.BACKBONE_C4) == (BK.FIRST, BK.END, BK.C4)
    blocks = train.backbone_blocks(sf)
    assert [id(b) for b in blocks] == [id(feats[i]) for i in range(8, 18)]
    assert [id(b) for b in train.backbone_blocks(type("M", (), {"sfnet": sf})())] == [id(b) for b in blocks]
    for i, b in enumerate(blocks, 8):
        cin, hid, cout, stride, res = BK.FEATURES[i]
        assert (b.cin, b.hidden, b.cout, b.stride, b.use_res_connect) == (cin, hid, cout, stride, res)
        assert tuple(n for n, _ in b.named_parameters()) == train.BLOCK_PARAMS        # InvertedResidual = dwBlock to the backward
        assert train._param_grad_parts(b.eval(), True)[0] is b.conv[0][0]
    assert sorted(set(BK.BLOCKS.values())) == sorted(set(BK.FEATURES[i] for i in range(8, 18)))
    shapes = {(h, c) for c, h, _, _, _ in BK.BLOCKS.values()} | {(o, h) for _, h, o, _, _ in BK.BLOCKS.values()}
    assert shapes == set(BK.GEMM_NEW + BK.GEMM_OLD)
    assert not any(p is q for b in blocks for p in b.parameters() for n in train.SRF_HEAD for q in getattr(sf, n).parameters())


@pytest.mark.parametrize("pic", BK.PICTURES, ids=lambda p: "%dx%dx%d" % p)
@pytest.mark.parametrize("name", list(BK.BLOCKS))
def test_block_closed_forms_equal_autograd_and_every_relu6_class_is_hit(name, pic):
    cfg = BK.BLOCKS[name]
    x, q, go = BK.block_case(name, pic)
    q64 = BR.to64(q)
    x, go = torch.as_tensor(x).double(), torch.as_tensor(go).double()
    p = BR.fold(q64)
    pt = {}
    closed = MP.param_grads(p, x, go, cfg[3], parts=pt)
    auto = MP.autograd_grads(q64, x, go, cfg[3], cfg[4])
    assert all(_close(closed[k], auto[k]) for k in BK.NAMES)
    gx = BK.conv_t(pt["ga"], p["w1"], p["s1"], res=go if cfg[4] else None)
    assert _close(gx, X.input_grad_autograd(p, x, go, cfg[3], cfg[4]))
    for t in (pt["e"], pt["d"]):                                  # 0, 6 and the interior
        assert min(BR.class_shares(t)) > 0.02, (name, BR.class_shares(t))
    # the module classes agree: the numbers load into torchvision's table and into the reference's dwBlock alike
    a, b = BK.make_block(cfg, q, model_feature.InvertedResidual), BK.make_block(cfg, q, dwBlock)
    assert [(n, tuple(v.shape)) for n, v in a.state_dict().items()] == [(n, tuple(v.shape)) for n, v in b.state_dict().items()]
    assert (a.stride, a.use_res_connect, a.dilation) == (b.stride, b.use_res_connect, b.dilation) == (cfg[3], cfg[4], 1)


@pytest.mark.parametrize("pic", BK.PICTURES, ids=lambda p: "%dx%dx%d" % p)
@pytest.mark.parametrize("name", list(BK.BLOCKS))
def test_block_closed_forms_equal_the_reference_goldens(name, pic):
    """tests/golden/backbone_*.npz: the reference's own dwBlock under float64 autograd (tools/make_backbone_goldens.py)."""
    cfg = BK.BLOCKS[name]
    x, q, go = BK.block_case(name, pic)
    z = np.load(os.path.join(GOLDEN, BK.golden_name(name, pic) + ".npz"))
    assert str(z["digest"]) == BK.golden_digest(x, q, go) and tuple(z["shape"]) == BK.in_grid(name, pic)
    p = BR.fold(BR.to64(q))
    x, go = torch.as_tensor(x).double(), torch.as_tensor(go).double()
    pt = {}
    closed = MP.param_grads(p, x, go, cfg[3], parts=pt)
    for k, v in BK.golden_pack(closed).items():
        assert _close(torch.as_tensor(v), torch.as_tensor(z[k]), 1e-9), k
    gx = BK.conv_t(pt["ga"], p["w1"], p["s1"], res=go if cfg[4] else None)
    assert _close(gx, torch.as_tensor(z["grad_x"]), 1e-9)


@pytest.fixture(scope="module")
def chains():
    runs = {}
    for pic in BK.PICTURES:
        c3, Q, g4, g5 = BK.chain_case(pic)
        Q64 = {i: BR.to64(q) for i, q in Q.items()}
        c3, g4, g5 = (torch.as_tensor(t).double() for t in (c3, g4, g5))
        runs[pic] = (Q64, {i: BR.fold(q) for i, q in Q64.items()}, c3, g4, g5)
    return runs


@pytest.mark.parametrize("pic", BK.PICTURES, ids=lambda p: "%dx%dx%d" % p)
def test_chain_closed_forms_equal_autograd(chains, pic):
    Q, P, c3, g4, g5 = chains[pic]
    keep = {}
    closed = BK.chain_closed(P, c3, g4, g5, keep=keep)
    auto = BK.chain_autograd(Q, c3, g4, g5)
    assert list(closed) == sorted(closed, key=lambda k: -int(k.split(".")[0])) and sorted(closed) == sorted(BK.PARAMS)
    for k in BK.PARAMS:
        assert _close(closed[k], auto[k], 1e-8), k
    n, h, w = pic
    assert tuple(keep["x13"].shape) == (n, 96, BK.down(h), BK.down(w)) and tuple(keep["x17"].shape[2:]) == (BK.down(BK.down(h)), BK.down(BK.down(w)))
    for i in range(BK.FIRST, BK.END):
        for t in (keep["e%d" % i], keep["d%d" % i]):
            assert min(BR.class_shares(t)) > 0.02, (i, BR.class_shares(t))
    # the walk's wrong variants, each seen by autograd's own gradients: at least 4 stage bounds away at the block that meets it
    no4 = BK.chain_autograd(Q, c3, g4, g5, variant="no_g_c4")
    cfg, x13 = BK.FEATURES[13], keep["x12"]
    pt = MP.block_parts(P[13], x13, keep["g13"], 1)
    _, b = MP.grads_from_parts(P[13], x13, pt["e"], pt["d"], pt["gd"], pt["ga"], keep["g13"], 1, bounds=True)
    assert max(_far(no4["13." + k], auto["13." + k], b[k]) for k in BK.NAMES) >= 4.0
    for v, blk in (("no_residual", 15), ("s2_anchor", 14), ("no_g_c4", 13)):
        wrong = BK.chain_closed(P, c3, g4, g5, variant=v)
        i = blk if v == "s2_anchor" else blk - 1                  # the block BEHIND the wrong grad_x; s2_anchor spoils block 14's own W1
        xin = keep["x%d" % (i - 1)]
        pt = MP.block_parts(P[i], xin, keep["g%d" % i], BK.FEATURES[i][3])
        _, b = MP.grads_from_parts(P[i], xin, pt["e"], pt["d"], pt["gd"], pt["ga"], keep["g%d" % i], BK.FEATURES[i][3], bounds=True)
        assert max(_far(wrong["%d.%s" % (i, k)], closed["%d.%s" % (i, k)], b[k]) for k in BK.NAMES) >= 4.0, v
    assert cfg[4]


@pytest.mark.parametrize("name,pic", [("b14", p) for p in BK.PICTURES] + [("b8", BK.PICTURES[0]), ("b15", BK.PICTURES[1])])
def test_block_wrong_variants_are_far(name, pic):
    cfg = BK.BLOCKS[name]
    x, q, go = BK.block_case(name, pic)
    x, go = torch.as_tensor(x).double(), torch.as_tensor(go).double()
    p = BR.fold(BR.to64(q))
    pt = MP.block_parts(p, x, go, cfg[3])
    g4 = torch.as_tensor(BK.chain_case(pic)[2]).double() if name == "b14" else None
    want = BK.block_stage(p, cfg, x, go, pt, res=g4)
    for v in (("s2_anchor", "no_g_c4") if name == "b14" else ("no_residual",)):
        wrong = BK.block_stage(p, cfg, x, go, pt, res=g4, variant=v)
        key = "ga" if v == "s2_anchor" else "grad_x"
        assert _far(wrong[key][0], want[key][0], want[key][1]) >= 4.0, (name, v)


def test_a_missing_aspp_branch_is_far_from_g_c5():
    """g_c5 = lv5_aspp1's input gradient + three `ga_b . (diag(s1) W1_b)`: leaving one branch out is at least 4 of the chained
    GEMM bounds away, on the head and the inputs the GPU test uses."""
    head = SF.calibrate(uavsal_srfnet_aspp("mobilenet_v2"))
    P, B = SF.head_params64(head)
    for case in SF.GOLDEN_CASES:
        c3, c4, c5, go = (torch.as_tensor(t).double() for t in SF.golden_inputs(case))
        c4r, c5r = c4.clone().requires_grad_(True), c5.clone().requires_grad_(True)
        a4, a5 = torch.autograd.grad(SF.forward64(P, B, c3, c4r, c5r), [c4r, c5r], go)
        keep = {}
        SF.backward64(P, B, c3, c4, c5, go, keep=keep)
        Pd = {k: v.detach() for k, v in P.items()}
        terms = BK.head_tap_terms(Pd, B, keep)
        g5, b5 = BK.sum_terms(terms["c5"])
        g4, _ = BK.sum_terms(terms["c4"])
        assert _close(g5, a5, 1e-9) and _close(g4, a4, 1e-9)
        for drop in range(1, 4):
            wrong, _ = BK.sum_terms([t for i, t in enumerate(terms["c5"]) if i != drop])
            assert _far(wrong, g5, b5) >= 4.0, drop


@pytest.mark.parametrize("M,N", BK.GEMM_NEW)
def test_gemm_wrong_variants_are_far(M, N):
    for pic in BK.GEMM_K:
        a, b, _, _ = BK.gemm_inputs(M, N, pic)
        a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
        G, bound = BK.pix_gemm_ref(a, b)
        K = pic[0] * pic[1] * pic[2]
        variants = [v for v, on in (("m_tail", M % 128), ("n_tail", N % 128), ("last_share", BK.short_partition(K, M, N)[1] > 1)) if on]
        assert variants
        for v in variants:
            assert _far(BK.pix_gemm_ref(a, b, v)[0], G, bound) >= 4.0, (M, N, pic, v)


def test_partitions_through_the_host_entry_points(lib):
    assert BK.short_partition(4800, 960, 160)[:2] == (256, 19) and BK.workgroups(4800, 960, 160) == 304
    assert BK.short_partition(35, 96, 384)[:2] == (128, 1) and BK.short_partition(2760, 576, 96)[:2] == (128, 22)
    for K in [p[0] * p[1] * p[2] for p in BK.GEMM_K] + [20 * 12 * 20, 20 * 23 * 40, 10 ** 7]:
        for M, N in BK.GEMM_NEW + BK.GEMM_OLD:
            d = _lib.PixGemmDesc()
            d.K, d.M, d.N = K, M, N
            plain = lib.uavsal_pix_gemm_shares(C.byref(d))
            assert plain == (0 if (M, N) in BK.GEMM_NEW else MP.gemm_partition(K, M, N)[1]), (M, N, K)      # without the flag: as before
            assert lib.uavsal_pix_gemm_workspace_bytes(C.byref(d)) == plain * M * N * 4
            d.tails32 = 1
            sh = BK.shares(K, M, N)
            assert lib.uavsal_pix_gemm_shares(C.byref(d)) == sh, (M, N, K)
            assert lib.uavsal_pix_gemm_workspace_bytes(C.byref(d)) == sh * M * N * 4
            if (M, N) in BK.GEMM_NEW:
                span, _, spans = BK.short_partition(K, M, N)
                assert span % BK.SHORT_UNIT == 0 and spans[-1][1] == K and (sh - 1) * span < K <= sh * span
    d = _lib.PixGemmDesc()
    d.K, d.tails32 = 4800, 1
    for M, N, want in ((96, 48, 0), (100, 96, 0), (96, 64, 38), (32, 32, 38), (1920, 1888, 2), (1920, 1920, 3)):      # the last: the rule it always had
        d.M, d.N = M, N
        assert lib.uavsal_pix_gemm_shares(C.byref(d)) == want, (M, N)
    g = _lib.PixGemmDesc()
    g.a = g.b = g.ws = g.out = 256
    g.K, g.M, g.N, g.lda, g.ldb, g.ldo = 100, 96, 384, 96, 384, 384
    assert lib.uavsal_pix_gemm(C.byref(g), None) == -3                    # UAVSAL_ESHAPE without the flag, as before
    g.tails32 = 1
    assert lib.uavsal_pix_gemm(C.byref(g), None) == -1                    # accepted: the workspace is too small
    g.ws_bytes = lib.uavsal_pix_gemm_workspace_bytes(C.byref(g))
    g.lda = 64
    assert lib.uavsal_pix_gemm(C.byref(g), None) == -1                    # rows shorter than M
    g.lda, g.a = 98, 256
    assert lib.uavsal_pix_gemm(C.byref(g), None) == -2                    # lda % 4
    assert C.sizeof(_lib.PixGemmDesc) == lib.uavsal_train_decoder_sizeof_desc(0)


def test_refusals_by_name():
    sf = uavsal_srfnet_aspp("mobilenet_v2").eval()
    feats = sf.features.features
    c3 = torch.zeros(1, 32, 8, 8)
    g4, g5 = torch.zeros(1, 96, 4, 4), torch.zeros(1, 320, 2, 2)
    with pytest.raises(RuntimeError, match="cuda"):
        train.backbone_backward(feats, c3, g4, g5)
    with pytest.raises(RuntimeError, match="features.features"):
        train.backbone_backward(feats[:5], c3, g4, g5)
    feats[9].train()
    with pytest.raises(RuntimeError, match="eval"):
        train.backbone_backward(feats, c3, g4, g5)
    feats[9].eval()
    x, g = torch.zeros(1, 64, 4, 4), torch.zeros(1, 64, 4, 4)
    with pytest.raises(RuntimeError, match="cuda"):
        train.block_backward(feats[8], x, g, backbone=True)
    with pytest.raises(RuntimeError, match="expand conv|Cout"):            # without the keyword block_backward keeps to what it took
        train.block_backward(feats[8], x, g)
    with pytest.raises(RuntimeError, match="eval"):
        train.block_backward(feats[8].train(), x, g, backbone=True)
    feats[8].eval()
    for bad in (feats[1], feats[0]):                                       # no expand conv; the stem
        with pytest.raises(RuntimeError, match="expand conv"):
            train.block_backward(bad, x, g, backbone=True)
    odd = dwBlock(64, 64, kernel_size=3, stride=2, dilation=2).eval()
    with pytest.raises(RuntimeError, match="dilated block with stride 2"):
        train.block_backward(odd, x, g, backbone=True)
    with pytest.raises(RuntimeError, match="Cout"):
        train.block_backward(dwBlock(64, 48, kernel_size=3).eval(), x, g, backbone=True)
    model = type("M", (), {"rnn_type": "twa", "num_cb": 0, "training": False})()
    with pytest.raises(RuntimeError, match="backbone=True needs srf=True"):
        train.recurrence_step(model, None, None, None, None, fuse=True, st=True, backbone=True)
    for stages in (("rnn", "backbone"), ("rnn", "fuse", "st", "backbone"), ("rnn", "fuse", "st", "backbone", "srf"),
                   ("rnn", "fuse", "st", "srf", "backbone", "backbone")):
        with pytest.raises(ValueError, match="stages"):
            stream.finetune_video(model, None, None, None, None, None, None, stages=stages)


class _Stub:
    time_dims = 5
    num_cb = 0

    def __init__(self, sfnet):
        self.rnn, self.fust_layer, self.st_layer, self.sfnet = object(), object(), object(), sfnet
        self.refreshed = []

    def refresh_weights(self, *mods, **kw):
        self.refreshed.append((mods, kw))


@pytest.mark.parametrize("refresh", ["host", "device"])
def test_finetune_video_hands_backbone_to_the_step_and_refreshes_the_ten_modules(monkeypatch, refresh):
    seen = []

    def step(model, x, cb, state, y, criterion, **kw):
        seen.append(kw)
        return torch.zeros(()), None, [torch.zeros(1)]
    monkeypatch.setattr(train, "recurrence_step", step)
    monkeypatch.setattr(stream, "_gaze_groups_loop", lambda model, *a: a[-1](None, None, None, None))
    m = _Stub(uavsal_srfnet_aspp("mobilenet_v2"))
    opt = type("O", (), {"zero_grad": lambda self: None, "step": lambda self: None})()
    stream.finetune_video(m, None, None, None, None, None, opt, stages=("rnn", "fuse", "st", "srf", "backbone"), refresh=refresh)
    assert seen == [{"fuse": True, "st": True, "srf": True, "backbone": True}]
    ((mods, kw),) = m.refreshed
    assert kw == ({"device": True} if refresh == "device" else {})
    assert [id(x) for x in mods[-10:]] == [id(x) for x in train.backbone_blocks(m)] and len(mods) == 21
    assert [id(x) for x in mods[-18:-10]] == [id(x) for x in train.srf_head(m)] and m.sfnet not in mods
