"""The SRF-Net head as an eighth training stage, without a GPU: the float64 restatement of tests/srf_ref64.py against
torch.autograd and against the reference's recorded gradients (tests/golden/srf_*.npz), the power of its wrong variants, the
partitions the GPU tests assume against the library's own entry points, and the refusals of the public surface."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from iip_uavsal_saliency_amd import _lib, stream, train
from iip_uavsal_saliency_amd.model import BasicConv2d, dwBlock, uavsal_srfnet_aspp

import srf_ref64 as SF
import st_ref64 as SR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = SF.U


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def head():
    return SF.calibrate(uavsal_srfnet_aspp("mobilenet_v2"))


@pytest.fixture(scope="module")
def golden_runs(head):
    """Per golden case: the inputs (float64 torch), the closed-form gradients and autograd's, computed once."""
    runs = {}
    P, B = SF.head_params64(head)
    for case in SF.GOLDEN_CASES:
        c3, c4, c5, go = (torch.as_tensor(t).double() for t in SF.golden_inputs(case))
        auto = torch.autograd.grad(SF.forward64(P, B, c3, c4, c5), [P[n] for n in SF.HEAD_PARAMS], go)
        keep = {}
        closed = SF.backward64(P, B, c3, c4, c5, go, keep=keep)
        runs[SF.golden_name(case)] = dict(inputs=(c3, c4, c5, go), auto=dict(zip(SF.HEAD_PARAMS, auto)), closed=closed, keep=keep)
    return runs


def test_srf_head_names_the_42_parameters_in_order(head):
    assert len(train.SRF_HEAD_PARAMS) == 42 and train.SRF_HEAD_PARAMS == SF.HEAD_PARAMS
    assert [n for n, _ in head.named_parameters() if not n.startswith("features.")] == list(train.SRF_HEAD_PARAMS)
    mods = train.srf_head(head)
    assert [id(m) for m in mods] == [id(getattr(head, n)) for n in train.SRF_HEAD] and len(mods) == 8
    holder = type("M", (), {"sfnet": head})()
    assert [id(m) for m in train.srf_head(holder)] == [id(m) for m in mods]
    assert sum(p.numel() for m in mods for p in m.parameters()) == sum(dict(head.named_parameters())[n].numel() for n in SF.HEAD_PARAMS)
    assert not any(p is q for m in mods for p in m.parameters() for q in head.features.parameters())


def test_closed_forms_equal_autograd(golden_runs):
    for name, run in golden_runs.items():
        for n in SF.HEAD_PARAMS:
            a, c = run["auto"][n], run["closed"][n]
            assert a.shape == c.shape, (name, n)
            err = float((a - c).abs().max()) / max(float(a.abs().max()), 1e-300)
            assert err <= 1e-10, (name, n, err)
        assert all(float(run["auto"][n].abs().max()) > 0 for n in SF.HEAD_PARAMS), name


def test_closed_forms_match_the_reference_goldens(head, golden_runs):
    for case in SF.GOLDEN_CASES:
        name = SF.golden_name(case)
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        assert str(z["digest"]) == SF.golden_digest(head, *SF.golden_inputs(case)), name
        mine = SF.golden_pack({n: g.numpy() for n, g in golden_runs[name]["closed"].items()})
        assert sorted(mine) == sorted(k for k in z.files if k != "digest")
        for k, v in mine.items():
            ref = z[k]
            scale = max(float(np.abs(ref).max()), 1e-300)
            assert np.shape(v) == ref.shape and float(np.abs(v - ref).max()) <= 1e-10 * scale, (name, k)


def _conv3_case(co, ci, pic, seed=0):
    n, h, w = pic
    rs = np.random.RandomState(31 * co + ci + n * h * w + seed)
    g = torch.from_numpy((rs.standard_normal((n, h, w, co)) / (h * w)).astype(np.float32))
    x = torch.from_numpy((3.0 * rs.random_sample((n, h, w, ci))).astype(np.float32))
    return g, x


def test_conv3_wgrad_variants_are_at_least_4_bounds_away():
    far = {v: 0.0 for v in SF.CONV3_WRONG}
    for co, ci in SF.CONV3_SHAPES:
        for pic in SF.CONV3_PICTURES[:3]:                                  # (the 45 x 80 case adds nothing a 9 x 13 one lacks)
            g, x = (t.double() for t in _conv3_case(co, ci, pic))
            want = SF.conv3_wgrad(g, x)
            eG, A = SF.conv3_wgrad_bound(g, x)
            bound = eG + U * A
            for v in SF.CONV3_WRONG:
                d = ((SF.conv3_wgrad(g, x, v) - want).abs() / bound.clamp_min(1e-300)).max()
                far[v] = max(far[v], float(d))
    assert all(f >= 4.0 for f in far.values()), far
    # a 1 x 1 picture: every shifted tap leaves the frame, only the centre is live
    g, x = (t.double() for t in _conv3_case(128, 64, (1, 1, 1)))
    G = SF.conv3_wgrad(g, x)
    centre = G[:, :, 1, 1].clone()
    G[:, :, 1, 1] = 0
    assert float(centre.abs().min()) > 0 and float(G.abs().max()) == 0.0
    # the restatement is conv2d's weight gradient
    g, x = (t.double() for t in _conv3_case(128, 64, (2, 9, 13)))
    W = torch.zeros(128, 64, 3, 3, dtype=torch.float64, requires_grad=True)
    (gw,) = torch.autograd.grad(F.conv2d(x.permute(0, 3, 1, 2), W, padding=1), W, g.permute(0, 3, 1, 2))
    assert float((gw - SF.conv3_wgrad(g, x)).abs().max()) <= 1e-12 * float(gw.abs().max())


def _dil_case(ch, n, h, w, dil, clamps=False):
    rs = np.random.RandomState(17 * ch + n * h * w + dil)
    shape = (n, h, w, ch)
    gd = torch.from_numpy((rs.standard_normal(shape) / (h * w)).astype(np.float32))
    if clamps:                                                            # all three classes and both clamps themselves
        vals = np.array([0.0, 6.0, 1.0, 3.0, 5.5, -0.0], np.float32)
        d, e = (torch.from_numpy(rs.choice(vals, shape)) for _ in range(2))
    else:
        d, e = (torch.from_numpy((-1.0 + 8.0 * rs.random_sample(shape)).clip(0, 6).astype(np.float32)) for _ in range(2))
    wd = torch.from_numpy(rs.standard_normal((ch, 3, 3)).astype(np.float32))
    s2 = torch.from_numpy((0.5 + rs.random_sample(ch)).astype(np.float32))
    go = torch.from_numpy((rs.standard_normal((n, h, w, 128)) / (h * w)).astype(np.float32))
    return gd, d, e, wd, s2, go


def _live_off_centre(dil, h, w):
    return dil < h or dil < w


def test_dilated_variants_are_at_least_4_bounds_away():
    for dil, h, w in SF.DIL_CASES:
        for clamps in (False, True):
            gd, d, e, wd, s2, go = (t.double() for t in _dil_case(64, 3, h, w, dil, clamps))
            want = SF.ir_bwd_dil(gd, d, e, wd, s2, dil)
            bound = SF.ir_bwd_dil_bound(gd, d, e, wd, s2, dil)
            (S2, Gd, S1, S3), (bS2, bGd, _, _) = SF.ir_sums_dil(gd, d, e, want, go, dil)
            if _live_off_centre(dil, h, w):                              # else both dilations see the centre tap alone
                v = SF.ir_bwd_dil(gd, d, e, wd, s2, dil, "dilation_1")
                assert float(((v - want).abs() / bound.clamp_min(1e-300)).max()) >= 4.0, (dil, h, w)
                Gd1 = SF.ir_sums_dil(gd, d, e, want, go, dil, "dilation_1")[0][1]
                assert float(((Gd1 - Gd).abs() / bGd.clamp_min(1e-300)).max()) >= 4.0, (dil, h, w)
            else:
                off = torch.ones(3, 3, dtype=torch.bool)
                off[1, 1] = False
                assert float(Gd[:, off].abs().max()) == 0.0
            if clamps:
                v = SF.ir_bwd_dil(gd, d, e, wd, s2, dil, "nonstrict_masks")
                assert float(((v - want).abs() / bound.clamp_min(1e-300)).max()) >= 4.0, (dil, h, w)
                S2n = SF.ir_sums_dil(gd, d, e, want, go, dil, "nonstrict_masks")[0][0]
                assert float(((S2n - S2).abs() / bS2.clamp_min(1e-300)).max()) >= 4.0, (dil, h, w)
    assert not _live_off_centre(6, 5, 5) and _live_off_centre(6, 5, 7) and not _live_off_centre(18, 12, 18)
    # the restatement is the adjoint of the dilated depthwise conv
    gd, d, e, wd, s2, _ = (t.double() for t in _dil_case(64, 2, 7, 13, 6))
    d[:] = 3.0
    e[:] = 3.0
    eg = e.clone().permute(0, 3, 1, 2).requires_grad_(True)
    (ge,) = torch.autograd.grad(F.conv2d(eg, wd.view(64, 1, 3, 3), padding=6, dilation=6, groups=64) * s2.view(1, -1, 1, 1), eg,
                                gd.permute(0, 3, 1, 2))
    assert float((ge.permute(0, 2, 3, 1) - SF.ir_bwd_dil(gd, d, e, wd, s2, 6)).abs().max()) <= 1e-12 * float(ge.abs().max())


def test_stage_variants_are_at_least_4_bounds_away(golden_runs, head):
    P, B = SF.head_params64(head)
    case = SF.GOLDEN_CASES[0]
    run = golden_runs[SF.golden_name(case)]
    k = run["keep"]
    nh = lambda t: t.permute(0, 2, 3, 1)                                  # noqa: E731
    go = run["inputs"][3]
    b3 = (P["conv_last.1.weight"].detach(), B["conv_last.1.running_mean"], B["conv_last.1.running_var"])
    W = P["conv_last.0.weight"].detach()
    want, bound = SF.cbr3_grads(nh(k["cat"]), nh(k["y"]), nh(go), W, *b3, bounds=True)
    w2 = SF.cbr3_grads(nh(k["cat"]), nh(k["y"]), nh(go), W, *b3, variant="s_twice")
    assert float(((w2["W"] - want["W"]).abs() / bound["W"].clamp_min(1e-300)).max()) >= 4.0
    w3 = SF.cbr3_grads(nh(k["cat"]), nh(k["y"]), nh(go), W, *b3, variant="no_mu_term")
    assert float(((w3["gamma"] - want["gamma"]).abs() / bound["gamma"].clamp_min(1e-300)).max()) >= 4.0
    for v in SF.WRONG:                                                    # and each one moves some gradient of the whole head
        wrong = SF.backward64(P, B, *run["inputs"], variant=v)
        rel = max(float((wrong[n] - run["closed"][n]).abs().max()) / float(run["closed"][n].abs().max()) for n in SF.HEAD_PARAMS)
        assert rel >= 1e-4, (v, rel)


def test_slab_and_share_counts_are_the_restated_partitions(lib):
    for co, ci in SF.CONV3_SHAPES + [(256, 512)]:
        for n, h, w in SF.CONV3_PICTURES + [(20, 45, 80), (64, 90, 160)]:
            d = _lib.Conv3WgradDesc()
            d.n_img, d.H, d.W, d.Co, d.Ci = n, h, w, co, ci
            cps, shares = SF.conv3_partition(n * h * w, co, ci)
            assert lib.uavsal_conv3_wgrad_shares(C.byref(d)) == shares, (co, ci, n, h, w)
            assert lib.uavsal_conv3_wgrad_workspace_bytes(C.byref(d)) == shares * co * 9 * ci * 4
            assert (shares - 1) * cps * SR.GEMM_CHAIN < n * h * w <= shares * cps * SR.GEMM_CHAIN
    assert SF.conv3_partition(20 * 45 * 80, 256, 448) == (6, 12)          # 72 tiles: the split of uavsal_twa_wgrad at that K
    t = _lib.TwaWgradDesc()
    t.T, t.H, t.W, t.C = 20, 45, 80, 256
    assert lib.uavsal_twa_wgrad_shares(C.byref(t)) == 12
    assert SF.conv3_partition(3 * 45 * 80, 256, 448)[1] > 1 and SF.conv3_partition(2 * 9 * 13, 128, 64) == (1, 1)
    for n in SF.DIL_N + (20,):
        for dil, h, w in SF.DIL_CASES:
            for ch in SF.DIL_CH + (1920,):
                d, u = _lib.IrSumsDilDesc(), _lib.IrSumsDesc()
                d.n_img, d.H, d.W, d.Ch, d.Co, d.dil = n, h, w, ch, 256, dil
                u.n_img, u.H, u.W, u.Ch, u.Co = n, h, w, ch, 256
                sr, slabs = SF.slab_partition(n, h, w)
                assert (lib.uavsal_ir_sums_dil_slab_rows(C.byref(d)), lib.uavsal_ir_sums_dil_slabs(C.byref(d))) == (sr, slabs)
                assert lib.uavsal_ir_sums_dil_slabs(C.byref(d)) == lib.uavsal_ir_sums_slabs(C.byref(u))
                assert lib.uavsal_ir_sums_dil_workspace_bytes(C.byref(d)) == lib.uavsal_ir_sums_workspace_bytes(C.byref(u)) \
                    == slabs * (_lib.IR_NSUM * ch + 256) * 8
    p = _lib.PixGemmDesc()
    for M, N in SF.GEMM_NEW_SHAPES:
        for K in SR.GEMM32_K + [20 * 45 * 80]:
            p.K, p.M, p.N = K, M, N
            cps, shares = SR.gemm32_partition(K, M, N)
            assert lib.uavsal_pix_gemm_shares(C.byref(p)) == shares, (M, N, K)
            assert lib.uavsal_pix_gemm_workspace_bytes(C.byref(p)) == shares * M * N * 4
    p.K = 72000
    for M, N, want in ((64, 32, 71), (128, 96, 71), (512, 480, SR.gemm32_partition(72000, 512, 480)[1]), (576, 32, 0), (64, 544, 0), (96, 32, 0), (64, 48, 0)):
        p.M, p.N = M, N
        assert lib.uavsal_pix_gemm_shares(C.byref(p)) == want, (M, N)
    for i, t in enumerate(_lib.SRF_DESC_TYPES):
        assert lib.uavsal_srf_sizeof_desc(i) == C.sizeof(t)
    assert lib.uavsal_srf_sizeof_desc(3) == -1 and lib.uavsal_abi_version() == 20


def test_argument_validation_without_gpu(lib):
    d = _lib.Conv3WgradDesc()
    assert lib.uavsal_conv3_wgrad(C.byref(d), None) == -1
    d.g = d.x = d.ws = d.out = 256
    d.n_img, d.H, d.W, d.Co, d.Ci, d.ldx = 1, 4, 4, 192, 64, 64
    assert lib.uavsal_conv3_wgrad(C.byref(d), None) == -3                  # Co % 128: UAVSAL_ESHAPE
    d.Co, d.Ci, d.ldx = 128, 96, 96
    assert lib.uavsal_conv3_wgrad(C.byref(d), None) == -3                  # Ci % 64
    d.Ci, d.ldx = 64, 64
    assert lib.uavsal_conv3_wgrad(C.byref(d), None) == -1                  # accepted so far: the workspace is too small
    d.ws_bytes = lib.uavsal_conv3_wgrad_workspace_bytes(C.byref(d))
    d.ldx = 32
    assert lib.uavsal_conv3_wgrad(C.byref(d), None) == -1                  # rows shorter than Ci
    d.ldx = 66
    assert lib.uavsal_conv3_wgrad(C.byref(d), None) == -2                  # ldx % 4: UAVSAL_EALIGN
    d.ldx, d.x = 64, 260
    assert lib.uavsal_conv3_wgrad(C.byref(d), None) == -2
    d.x, d.rowdot = 256, 256
    assert lib.uavsal_conv3_wgrad(C.byref(d), None) == -1                  # rowdot without w
    b = _lib.IrBwdDilDesc()
    b.gd = b.d = b.e = b.wd9 = b.s2 = b.ga = 256
    b.n_img, b.H, b.W, b.C, b.dil = 1, 4, 4, 64, 0
    assert lib.uavsal_ir_bwd_dil(C.byref(b), None) == -1                   # dil < 1
    b.C, b.dil = 66, 6
    assert lib.uavsal_ir_bwd_dil(C.byref(b), None) == -2                   # C % 4
    s = _lib.IrSumsDilDesc()
    s.gd = s.d = s.e = s.ga = s.go = s.ws = 256
    s.n_img, s.H, s.W, s.Ch, s.Co, s.ldgo, s.dil = 1, 4, 4, 96, 128, 128, 6
    assert lib.uavsal_ir_sums_dil(C.byref(s), None) == -3                  # Ch % 64
    s.Ch, s.dil = 64, 0
    assert lib.uavsal_ir_sums_dil(C.byref(s), None) == -1
    s.dil = 6
    assert lib.uavsal_ir_sums_dil(C.byref(s), None) == -1                  # accepted so far: the workspace is too small


def test_public_surface_refusals_without_gpu(head):
    t = torch.zeros(1, 4, 4, 128)
    with pytest.raises(RuntimeError, match="cuda"):
        train.conv3_wgrad(t, torch.zeros(1, 4, 4, 64))
    with pytest.raises(RuntimeError, match="cuda"):
        train.ir_bwd_dil(t, t, t, torch.zeros(9, 128), torch.zeros(128), 6)
    with pytest.raises(RuntimeError, match="cuda"):
        train.ir_sums_dil(t, t, t, t, t, 6)
    conv = BasicConv2d(64, 128, 3).eval()
    x, g = torch.zeros(1, 64, 4, 4), torch.zeros(1, 128, 4, 4)
    with pytest.raises(RuntimeError, match="cuda"):
        train.conv3_backward(conv[0], conv[1], x, None, g)
    with pytest.raises(RuntimeError, match="eval"):
        train.conv3_backward(conv[0], conv[1].train(), x, None, g)
    for bad in (BasicConv2d(64, 128, 1), BasicConv2d(64, 128, 3, stride=2), BasicConv2d(64, 128, 3, dilation=2),
                BasicConv2d(64, 96, 3), BasicConv2d(32, 128, 3), BasicConv2d(128, 128, 3, groups=128)):
        with pytest.raises(RuntimeError, match="dense 3x3|Cout"):
            train.conv3_backward(bad[0], bad[1].eval(), x, None, g)
    blk = dwBlock(64, 128, kernel_size=3, dilation=6).eval()               # a dilated stride-1 block is taken: the tensors are not
    with pytest.raises(RuntimeError, match="cuda"):
        train.block_param_grads(blk, x, None, None, g)
    odd = dwBlock(64, 128, kernel_size=3, dilation=6).eval()
    odd.conv[1][0].dilation = (1, 1)                                       # the block and its conv disagree: not taken on trust
    with pytest.raises(RuntimeError, match="expand conv"):
        train.block_param_grads(odd, x, None, None, g)
    with pytest.raises(RuntimeError, match="Cout"):
        train.block_param_grads(dwBlock(64, 64, kernel_size=3, dilation=6).eval(), x, None, None, g)
    with pytest.raises(RuntimeError, match="expand conv|Cout"):            # block_backward keeps refusing a dilation
        train.block_backward(blk, x, g)
    c3, c4, c5 = torch.zeros(1, 32, 8, 8), torch.zeros(1, 96, 4, 4), torch.zeros(1, 320, 2, 2)
    y = torch.zeros(1, 256, 8, 8)
    with pytest.raises(RuntimeError, match="cuda"):
        train.srf_head_backward(head, c3, c4, c5, y, y)
    with pytest.raises(RuntimeError, match="eval"):
        train.srf_head_backward(head.train(), c3, c4, c5, y, y)
    head.eval()
    with pytest.raises(RuntimeError, match="sfnet"):
        train.srf_head_backward(conv, c3, c4, c5, y, y)
    model = type("M", (), {"rnn_type": "twa", "num_cb": 0, "training": False})()
    with pytest.raises(RuntimeError, match="st=True"):
        train.recurrence_step(model, None, None, None, None, fuse=True, srf=True)
    for stages in (("rnn", "srf"), ("rnn", "fuse", "srf"), ("rnn", "fuse", "srf", "st"), ("rnn", "fuse", "st", "srf", "srf")):
        with pytest.raises(ValueError, match="stages"):
            stream.finetune_video(model, None, None, None, None, None, None, stages=stages)


class _Stub:
    time_dims = 5
    num_cb = 0

    def __init__(self, sfnet):
        self.rnn, self.fust_layer, self.st_layer, self.sfnet = object(), object(), object(), sfnet
        self.refreshed = []
        self.w = torch.nn.Parameter(torch.zeros(1))

    def refresh_weights(self, *mods):
        self.refreshed.append(mods)


def test_finetune_video_hands_srf_to_the_step_and_refreshes_the_eight_modules(head, monkeypatch):
    seen = []

    def step(model, x, cb, state, y, criterion, **kw):
        seen.append(kw)
        return torch.zeros(()), None, [torch.zeros(1)]
    monkeypatch.setattr(train, "recurrence_step", step)
    monkeypatch.setattr(stream, "_gaze_groups_loop", lambda model, *a: a[-1](None, None, None, None))
    m = _Stub(head)
    opt = type("O", (), {"zero_grad": lambda self: None, "step": lambda self: None})()
    stream.finetune_video(m, None, None, None, None, None, opt, stages=("rnn", "fuse", "st", "srf"))
    assert seen == [{"fuse": True, "st": True, "srf": True}]
    (mods,) = m.refreshed
    assert [id(x) for x in mods[-8:]] == [id(x) for x in train.srf_head(m)] and m.sfnet not in mods and len(mods) == 11
