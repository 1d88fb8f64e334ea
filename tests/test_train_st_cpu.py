"""The ST stage without a GPU: the float64 restatement of tests/st_ref64.py against torch autograd, the library's partitions
against the restated ones, the conditions that make tests/test_train_st_gpu.py meaningful (every WRONG variant at least 4
bounds away, all three ReLU6 classes populated, no mask decided differently by the stored fp32 tensors), the C ABI, argument
validation, refusals by name, and the host refresh of an ST block's packed weights against a fresh pack."""
import ctypes as C
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from iip_uavsal_saliency_amd import _lib, train
from iip_uavsal_saliency_amd import packing as P
from iip_uavsal_saliency_amd.model import STBlock
from iip_uavsal_saliency_amd.weights import WeightCache

import st_ref64 as SR

U = SR.U


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ------------------------------------------------------------------------------------------------ the C ABI
def test_symbols_struct_sizes_and_abi(lib):
    assert lib.uavsal_abi_version() == 20
    names = [s[0] for s in _lib.SYMBOLS]
    for n in ("uavsal_cbr_sums", "uavsal_cbr_sums_workspace_bytes", "uavsal_cbr_sums_slabs", "uavsal_cbr_sums_slab_rows",
              "uavsal_cbr_finish", "uavsal_tdiff_bwd", "uavsal_st_sizeof_desc"):
        assert names.count(n) == 1 and hasattr(lib, n)
    for i, t in enumerate(_lib.ST_DESC_TYPES):
        assert lib.uavsal_st_sizeof_desc(i) == C.sizeof(t)
    assert lib.uavsal_st_sizeof_desc(len(_lib.ST_DESC_TYPES)) == -1 and lib.uavsal_nets_sizeof_desc(3) == -1
    assert len(train.ST_BLOCK_PARAMS) == 27 and len(set(train.ST_BLOCK_PARAMS)) == 27
    blk = STBlock(256, 256, time_dims=5, reduction=8)
    assert [n for n, _ in blk.named_parameters()] == list(train.ST_BLOCK_PARAMS)


def test_slab_and_share_counts_are_the_restated_partitions(lib):
    for n, h, w in SR.PICTURES + [(20, 45, 80), (300, 4, 4), (64, 90, 160)]:
        sr, slabs = SR.slab_partition(n, h, w)
        for c in (32, 256):
            d = _lib.CbrSumsDesc()
            d.n_img, d.H, d.W, d.C = n, h, w, c
            assert lib.uavsal_cbr_sums_slab_rows(C.byref(d)) == sr and lib.uavsal_cbr_sums_slabs(C.byref(d)) == slabs
            assert lib.uavsal_cbr_sums_workspace_bytes(C.byref(d)) == slabs * c * 8
            assert (slabs - 1) * sr < n * h <= slabs * sr and slabs <= SR.MAX_SLABS
    assert SR.slab_partition(1, 45, 80) == (7, 7) and SR.slab_partition(3, 45, 80) == (7, 20) and 135 % 7 and 45 % 7
    assert SR.slab_partition(2, 9, 13)[1] == 1                                            # a frame border inside one slab
    for M, N in SR.GEMM32_SHAPES:
        for K in SR.GEMM32_K + [20 * 45 * 80, 10 ** 7]:
            d = _lib.PixGemmDesc()
            d.K, d.M, d.N = K, M, N
            cps, shares = SR.gemm32_partition(K, M, N)
            assert lib.uavsal_pix_gemm_shares(C.byref(d)) == shares, (M, N, K)
            assert lib.uavsal_pix_gemm_workspace_bytes(C.byref(d)) == shares * M * N * 4
            assert (shares - 1) * cps * SR.GEMM_CHAIN < K <= shares * cps * SR.GEMM_CHAIN
    assert SR.gemm32_partition(10800, 32, 256) == (1, 11) and SR.gemm32_partition(234, 32, 384) == (1, 1)
    d = _lib.PixGemmDesc()
    d.K = 72000
    for M, N, want in ((96, 64, 0), (1920, 32, 0), (32, 544, 0), (32, 512, 71), (128, 32, 71), (32, 64, 0), (32, 32, 0), (32, 48, 0), (48, 32, 0), (1536, 256, 36), (64, 64, 71)):      # refused / as before
        d.M, d.N = M, N
        assert lib.uavsal_pix_gemm_shares(C.byref(d)) == want, (M, N)


def test_argument_validation_without_gpu(lib):
    s = _lib.CbrSumsDesc()
    assert lib.uavsal_cbr_sums(C.byref(s), None) == -1
    s.g = s.y = s.gp = s.ws = 256
    s.n_img, s.H, s.W, s.C, s.ldg, s.ldy = 1, 4, 4, 48, 48, 48
    assert lib.uavsal_cbr_sums(C.byref(s), None) == -3                    # C % 32: UAVSAL_ESHAPE
    s.C, s.ldg, s.ldy = 32, 34, 32
    assert lib.uavsal_cbr_sums(C.byref(s), None) == -2                    # ldg % 4: UAVSAL_EALIGN
    s.ldg = 16
    assert lib.uavsal_cbr_sums(C.byref(s), None) == -1                    # rows shorter than C
    s.ldg = 32
    assert lib.uavsal_cbr_sums(C.byref(s), None) == -1                    # accepted so far: the workspace is too small
    s.ws_bytes = lib.uavsal_cbr_sums_workspace_bytes(C.byref(s))
    s.y = 260
    assert lib.uavsal_cbr_sums(C.byref(s), None) == -2
    f = _lib.CbrFinishDesc()
    assert lib.uavsal_cbr_finish(C.byref(f), None) == -1
    f.ws = f.rowdot = f.r = f.mu = f.g_gamma = f.g_beta = 256
    f.C, f.slabs = 32, 2
    assert lib.uavsal_cbr_finish(C.byref(f), None) == -1                  # workspace too small
    f.ws_bytes, f.C = 2 * 48 * 8, 48
    assert lib.uavsal_cbr_finish(C.byref(f), None) == -3
    f.C, f.rowdot = 32, 260
    assert lib.uavsal_cbr_finish(C.byref(f), None) == -2
    t = _lib.TdiffBwdDesc()
    assert lib.uavsal_tdiff_bwd(C.byref(t), None) == -1
    t.g = t.r = t.out = 256
    t.n_img, t.HW, t.C, t.seq_len, t.ldg, t.ldr, t.ldo = 4, 35, 32, 1, 64, 32, 32
    assert lib.uavsal_tdiff_bwd(C.byref(t), None) == -3                   # one frame per sequence
    t.seq_len = 3
    assert lib.uavsal_tdiff_bwd(C.byref(t), None) == -3                   # 4 % 3
    t.seq_len, t.C = 2, 6
    assert lib.uavsal_tdiff_bwd(C.byref(t), None) == -2
    t.C, t.ldg = 32, 32
    assert lib.uavsal_tdiff_bwd(C.byref(t), None) == -2                   # rows shorter than 2 C
    t.ldg, t.r = 64, 264
    assert lib.uavsal_tdiff_bwd(C.byref(t), None) == -2
    g = _lib.PixGemmDesc()
    g.a = g.b = g.ws = g.out = 256
    g.K, g.M, g.N, g.lda, g.ldb, g.ldo = 100, 32, 48, 32, 48, 48
    assert lib.uavsal_pix_gemm(C.byref(g), None) == -3                    # N % 32
    g.N = 64
    assert lib.uavsal_pix_gemm(C.byref(g), None) == -3                    # less than one workgroup of tiles
    g.N, g.ldb, g.ldo = 256, 256, 256
    assert lib.uavsal_pix_gemm(C.byref(g), None) == -1                    # accepted: the workspace is too small
    g.ws_bytes = lib.uavsal_pix_gemm_workspace_bytes(C.byref(g))
    g.lda = 16
    assert lib.uavsal_pix_gemm(C.byref(g), None) == -1                    # rows shorter than M


# ------------------------------------------------------------------------------------------------ restatement vs autograd
def _cbr_numbers(seed, P_=400, cin=64, c=32):
    rs = np.random.RandomState(seed)
    x = torch.from_numpy((3.0 * rs.random_sample((P_, cin))).astype(np.float32)).double()
    W = torch.from_numpy((rs.standard_normal((c, cin)) * np.sqrt(2.0 / c)).astype(np.float32)).double()
    pre = x @ W.t()
    r = torch.from_numpy(rs.choice(np.array([0.5, 1.0, 2.0]), c))
    mean = torch.from_numpy(rs.standard_normal(c).astype(np.float32)).double()
    var = (1.0 / r ** 2 - SR.BN_EPS).float().double()
    s = 3.0 / pre.std(0)
    gamma = (s * torch.sqrt(var + SR.BN_EPS)).float().double()
    beta = (1.5 + torch.from_numpy(rs.standard_normal(c)) - pre.mean(0) * s + mean * s).float().double()
    gamma[5], beta[5] = 0.0, 1.5
    g = torch.from_numpy((rs.standard_normal((P_, c)) / P_).astype(np.float32)).double()
    return x, W, gamma, beta, mean, var, g


def test_closed_forms_match_float64_autograd():
    for N, L in SR.TDIFF_CASES:
        rs = np.random.RandomState(N * 10 + L)
        r = torch.from_numpy(6.5 * rs.random_sample((N, 2, 3, 4)) - 0.25).requires_grad_(True)
        g = torch.from_numpy(rs.standard_normal((N, 2, 3, 8)))
        (ga,) = torch.autograd.grad(SR.tdiff(r, L), r, g)
        assert torch.allclose(ga * SR.m6(r), SR.tdiff_bwd(g, r.detach(), L), rtol=0, atol=1e-13)
    x, W, gamma, beta, mean, var, g = _cbr_numbers(1)
    leaves = [t.clone().requires_grad_(True) for t in (W, gamma, beta, x)]
    s, b, _ = SR.bn_fold(leaves[1], leaves[2], mean, var)
    y = ((leaves[3] @ leaves[0].t()) * s + b).clamp(0, 6)
    want = torch.autograd.grad(y, leaves, g)
    got = SR.cbr_grads(x, y.detach(), g, W, gamma, mean, var)
    for a, k in zip(want, ("W", "gamma", "beta", "x")):
        assert float((a - got[k]).abs().max()) <= 1e-12 * max(1.0, float(a.abs().max())), k
    assert float(got["gamma"][5].abs()) > 0 and float(got["W"][5].abs().max()) == 0       # gamma = 0: from the unscaled sums
    # a dwBlock 64 -> 384 -> 32 from its stored tensors
    rs = np.random.RandomState(3)
    xb = torch.from_numpy(rs.standard_normal((2, 64, 5, 7)))
    w1, wd, w3 = (torch.from_numpy(rs.standard_normal(sh) * 0.2) for sh in ((384, 64, 1, 1), (384, 1, 3, 3), (32, 384, 1, 1)))
    bns = [tuple(torch.from_numpy(v) for v in (0.5 + rs.random_sample(c), 0.5 + 0.2 * rs.standard_normal(c), 0.1 * rs.standard_normal(c),
                                               0.5 + rs.random_sample(c))) for c in (384, 384, 32)]
    leaves = [t.clone().requires_grad_(True) for t in (w1, bns[0][0], bns[0][1], wd, bns[1][0], bns[1][1], w3, bns[2][0], bns[2][1])]
    bl = [(leaves[1], leaves[2]) + bns[0][2:], (leaves[4], leaves[5]) + bns[1][2:], (leaves[7], leaves[8]) + bns[2][2:]]
    e = SR._cbr(xb, leaves[0], bl[0])
    s2, b2, _ = SR.bn_fold(*bl[1])
    d = (F.conv2d(e, leaves[3], padding=1, groups=384) * s2.view(1, -1, 1, 1) + b2.view(1, -1, 1, 1)).clamp(0, 6)
    s3, b3, _ = SR.bn_fold(*bl[2])
    o = F.conv2d(d, leaves[6]) * s3.view(1, -1, 1, 1) + b3.view(1, -1, 1, 1)
    go = torch.from_numpy(rs.standard_normal(tuple(o.shape)))
    gd, ge_pre = torch.autograd.grad(o, [d, e], go, retain_graph=True)
    want = torch.autograd.grad(o, leaves, go)
    nh = lambda t: t.detach().permute(0, 2, 3, 1)                          # noqa: E731
    ga = ge_pre * SR.m6(e)
    got, _ = SR.block_grads(nh(xb), nh(e), nh(d), nh(gd), nh(ga), nh(go), w1, wd, w3, *[(b[0], b[2], b[3]) for b in bns])
    for a, b_ in zip(want, got):
        assert float((a.reshape(b_.shape) - b_).abs().max()) <= 1e-11 * max(1.0, float(a.abs().max()))


def test_the_conditions_that_make_the_gpu_tests_meaningful():
    far = {v: 0.0 for v in SR.CBR_WRONG}
    for seed in (1, 2):
        x, W, gamma, beta, mean, var, g = _cbr_numbers(seed)
        s, b, _ = SR.bn_fold(gamma, beta, mean, var)
        pre = (x @ W.t()) * s + b
        y = pre.clamp(0, 6).float().double()                                              # what a device would store
        assert bool((y == 0).any()) and bool((y == 6).any()) and bool(SR.m6(y).any())   # all three ReLU6 classes
        assert torch.equal(SR.m6(y), SR.m6(pre) & SR.m6(y))                               # the stored fp32 y decides no mask ...
        assert int((SR.m6(pre) ^ SR.m6(y)).sum()) == 0                                    # ... differently from float64
        want, bound = SR.cbr_grads(x, y, g, W, gamma, mean, var, bounds=True)
        res = torch.full_like(y, 2.0)
        for v in SR.CBR_WRONG:
            wr = SR.cbr_grads(x, y, g, W, gamma, mean, var, variant=v, res=res)
            far[v] = max(far[v], max(float(((wr[k] - want[k]).abs() / (bound[k] + 1e-30)).max()) for k in bound))
    assert all(f >= 4.0 for f in far.values()), far
    tf = {v: 0.0 for v in SR.TDIFF_WRONG}
    for N, L in SR.TDIFF_CASES:
        rs = np.random.RandomState(N + L)
        g = torch.from_numpy(rs.standard_normal((N, 5, 7, 64)).astype(np.float32)).double()
        r = torch.from_numpy(rs.choice(np.array([0.0, 6.0, 1.0, 3.0, 5.5], np.float32), (N, 5, 7, 32))).double()
        want, bound = SR.tdiff_bwd(g, r, L), SR.tdiff_bwd_bound(g, r, L) + 1e-30
        for v in SR.TDIFF_WRONG:
            if not (v == "cross_border" and N == L):
                tf[v] = max(tf[v], float(((SR.tdiff_bwd(g, r, L, v) - want).abs() / bound).max()))
    assert all(f >= 4.0 for f in tf.values()), tf
    assert set(SR.TDIFF_WRONG) | set(SR.CBR_WRONG) | {"no_residual"} == set(SR.WRONG)


# ------------------------------------------------------------------------------------------------ drivers and refusals
def test_finetune_video_stage_tuples():
    from iip_uavsal_saliency_amd.stream import finetune_video
    priors, plain = types.SimpleNamespace(num_cb=3), types.SimpleNamespace(num_cb=0)
    bad = [(priors, ("rnn", "st")), (priors, ("rnn", "fuse", "st")), (priors, ("rnn", "fuse", "ctx", "st")), (plain, ("rnn", "st")),
           (priors, ("rnn", "fuse", "fust", "st", "nets")), (priors, ("rnn", "st", "fuse", "fust"))]
    for m, stages in bad:
        with pytest.raises(ValueError, match="'st' the very last"):
            finetune_video(m, None, None, None, None, None, None, stages=stages)
    good = [(priors, ("rnn", "fuse", "fust", "st")), (priors, ("rnn", "decoder", "fuse", "fust", "ctx", "nets", "st")),
            (plain, ("rnn", "fuse", "st")), (plain, ("rnn", "decoder", "fuse", "st"))]
    for m, stages in good:
        with pytest.raises(Exception) as ei:                                              # past the validation: no frames to read
            finetune_video(m, None, None, None, None, None, None, stages=stages)
        assert "stages must be" not in str(ei.value)


def test_refusals_by_name():
    blk = STBlock(256, 256, time_dims=5, reduction=8).eval()
    x = torch.zeros((2, 256, 5, 7))
    with pytest.raises(RuntimeError, match="cuda"):
        train.st_block_backward(blk, x, x)
    with pytest.raises(RuntimeError, match="cuda"):
        train.cbr_backward(blk.stconv_last[0], blk.stconv_last[1], x, x.permute(0, 2, 3, 1), x)
    blk.train()
    with pytest.raises(RuntimeError, match="eval"):
        train.st_block_backward(blk, x, x)
    blk.eval()
    blk.fu_type = "concat"
    with pytest.raises(RuntimeError, match="fu_type"):
        train.st_block_backward(blk, x, x)
    with pytest.raises(RuntimeError, match="STBlock"):
        train.st_block_backward(blk.stconv_last, x, x)
    for m in (types.SimpleNamespace(num_cb=3, rnn_type="twa"), types.SimpleNamespace(num_cb=0, rnn_type="twa")):
        with pytest.raises(RuntimeError, match="st=True"):
            train.recurrence_step(m, None, None, None, None, st=True)
    with pytest.raises(RuntimeError, match="st=True"):
        train.recurrence_step(types.SimpleNamespace(num_cb=3, rnn_type="twa"), None, None, None, None, fuse=True, st=True)


# ------------------------------------------------------------------------------------------------ packed weights of an ST block
def _pack(blk, cache):
    """Every packed entry the forward plan and the backward walk make of an ST block's modules."""
    te = blk.stconv_te
    for m in (te.reduce_conv, te.last_conv, blk.stconv_last):
        cout = m[0].weight.shape[0]
        for layout in ("f32", "f32k32"):
            cache.conv(m[0], None, 0, layout)
        cache.affine(m[1], cout), cache.bn_stats(m[1]), cache.conv_t_scaled(m[0], m[1], "f32")
    for b in (blk.stconv_sp.spconv, te.sub_conv):
        seq = b.conv
        cache.conv(seq[0][0], None, 0, "f32"), cache.conv(seq[2], None, 0, "f32")
        cache.affine(seq[0][1], b.hidden), cache.affine(seq[3], b.cout), cache.depthwise(seq[1][0], seq[1][1])
        for cv, bn in ((seq[0][0], seq[0][1]), (seq[2], seq[3])):
            cache.conv_t_scaled(cv, bn, "f32"), cache.bn_stats(bn)
        cache.bn_stats(seq[1][1])
    cache.fused_block(te.sub_conv, True)                                                  # csrc/fused_mid.hip: 64 -> 384 -> 32


def _flat(v):
    return [v] if torch.is_tensor(v) else [v[k] for k in sorted(v)] if isinstance(v, dict) else list(v)


def test_host_refresh_of_an_st_block_is_a_fresh_pack():
    torch.manual_seed(5)
    blk = STBlock(256, 256, time_dims=5, reduction=8).eval()
    cache = WeightCache("cpu", {})
    _pack(blk, cache)
    kinds = sorted({k[0] for k in cache.store})
    assert kinds == ["bn", "bnstat", "dw", "fused", "w", "wTs"]                           # every kind WeightCache.refresh remakes
    held = {k: [t.data_ptr() for t in _flat(v)] for k, v in cache.store.items()}
    with torch.no_grad():
        for p in blk.parameters():
            p.add_(0.01 * torch.randn_like(p))
        for b in blk.buffers():
            if b.dtype.is_floating_point:
                b.mul_(1.1)
    mods = {id(s): s for s in blk.modules()}
    n = cache.refresh(mods, dry=True)
    assert n == len(cache.store) == cache.refresh(mods)
    fresh = WeightCache("cpu", {})
    _pack(blk, fresh)
    assert list(fresh.store) == list(cache.store)
    for k in cache.store:
        assert [t.data_ptr() for t in _flat(cache.store[k])] == held[k]                   # in place: plans hold the addresses
        for a, b in zip(_flat(cache.store[k]), _flat(fresh.store[k])):
            assert torch.equal(a, b) and a.dtype == b.dtype, k
    assert P.roundup(32, 32) == 32


# ------------------------------------------------------------------------------------------------ the reference's own STBlock
@pytest.mark.parametrize("case", SR.GOLDEN_CASES, ids=SR.golden_name)
def test_restatement_matches_the_recorded_reference_autograd(case, golden_dir):
    """tests/golden/st_*.npz: the reference's own `STBlock` under float64 autograd (tools/make_st_goldens.py).  Against them:
    torch autograd through `st_ref64.forward64`, and the closed forms (`cbr_grads`, `block_grads`, `tdiff_bwd`) composed by
    `st_ref64.backward64` -- the boundary rules of the temporal difference (a case with L < N is N / L reference calls), where
    the residuals enter and which tensor each mask looks at are the reference's, not a reading of it."""
    import os
    N, h, w, L = case
    g = np.load(os.path.join(golden_dir, SR.golden_name(case) + ".npz"))
    blk = SR.calibrate(STBlock(256, 256, time_dims=L, reduction=8))
    x, go = SR.golden_inputs(case)
    assert str(g["digest"]) == SR.golden_digest(blk, x, go) and tuple(g["case"]) == tuple(case)      # the same numbers went in
    P_, B = SR.block_params64(blk)
    names = list(P_)
    assert names == list(train.ST_BLOCK_PARAMS)
    xx = torch.from_numpy(x).double().requires_grad_(True)
    gs = torch.autograd.grad(SR.forward64(P_, B, xx, L), [P_[n] for n in names] + [xx], torch.from_numpy(go).double())
    auto = ({n: t.numpy() for n, t in zip(names, gs[:-1])}, gs[-1].numpy())
    cg, cx = SR.backward64(P_, B, torch.from_numpy(x).double(), torch.from_numpy(go).double(), L)
    closed = ({n: cg[n].numpy() for n in names}, cx.numpy())
    assert set(cg) == set(names)
    for what, (grads, gx) in (("autograd of forward64", auto), ("closed form", closed)):
        got = SR.golden_pack(grads, gx)
        assert set(got) | {"case", "digest"} == set(g.files)
        for k, v in got.items():
            want = g[k]
            scale = max(float(np.abs(want).max()), 1e-300)
            if k.endswith("__sum"):                              # behind a BatchNorm a weight gradient's sum cancels: its norm is the scale
                scale = float(g[k[:-5] + "__l2"]) * np.sqrt(grads[next(n for n in names if n.replace(".", "_") == k[:-5])].size)
            assert np.shape(v) == want.shape and float(np.abs(v - want).max()) <= 1e-9 * scale, (what, k)
    # the goldens tell the wrong variants apart: the whole call as one sequence where the reference ran two, no residual
    if L < N:
        wg, wx = SR.backward64(P_, B, torch.from_numpy(x).double(), torch.from_numpy(go).double(), N)
        k = "stconv_te.reduce_conv.1.bias".replace(".", "_")
        assert float(np.abs(wg["stconv_te.reduce_conv.1.bias"].numpy() - g[k]).max()) > 1e-3 * float(np.abs(g[k]).max())
    _, nx = SR.backward64(P_, B, torch.from_numpy(x).double(), torch.from_numpy(go).double(), L, variant="no_residual")
    assert float(np.abs(nx.numpy()[SR.GX_SUBSET] - g["grad_x"]).max()) > 1e-3 * float(np.abs(g["grad_x"]).max())
