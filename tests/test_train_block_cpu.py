"""The backward of a general inverted-residual block without a GPU: the C ABI of csrc/train_block.hip and of the pixel GEMM's
N tail, the float64 closed form of tests/block_ref64.py against the reference's recorded autograd results
(tests/golden/block_*.npz) and against torch autograd, the restated partitions against what the library answers, the
conditions under which the GPU tests are meaningful (all three classes of both ReLU6s populated, no mask decided differently
by the stored fp32 e and d, every wrong kernel at least 4 bounds away), the weight cache's entries of the block and their
refresh, the driver's `stages`, and what the Python entry points refuse."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import _lib, stream, train
from iip_uavsal_saliency_amd.weights import WeightCache

import block_ref64 as BR
import train_ref64 as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [(c, s) for c in BR.CFGS for s in BR.SHAPES]
SMALL = [(c, s) for c in BR.CFGS for s in BR.GOLDEN_SHAPES]
_cases = {}


def _id(cs):
    return BR.name(*cs)


def case(cfg, shape, zero_gamma=False):
    """(x, q, go) as float64 tensors + the closed form with bounds and parts, computed once per case."""
    key = (cfg, shape, zero_gamma)
    if key not in _cases:
        x, q, go = BR.block_case(cfg, shape, zero_gamma)
        x, q, go = torch.as_tensor(x).double(), BR.to64(q), torch.as_tensor(go).double()
        parts = {}
        g, b = BR.param_grads(q, x, go, bounds=True, parts=parts)
        _cases[key] = (x, q, go, g, b, parts)
    return _cases[key]


@pytest.fixture(scope="module")
def lib():
    from iip_uavsal_saliency_amd import build
    build.build()
    return _lib.load()


def test_symbols_and_sizes(lib):
    names = [s[0] for s in _lib.SYMBOLS]
    for n in ("uavsal_ir_bwd", "uavsal_ir_sums", "uavsal_ir_sums_workspace_bytes", "uavsal_ir_sums_slabs",
              "uavsal_ir_sums_slab_rows", "uavsal_ir_finish", "uavsal_block_sizeof_desc"):
        assert n in names and hasattr(lib, n)
    assert len(_lib.BLOCK_DESC_TYPES) == 3
    for i, t in enumerate(_lib.BLOCK_DESC_TYPES):
        assert lib.uavsal_block_sizeof_desc(i) == C.sizeof(t)
    assert lib.uavsal_block_sizeof_desc(3) < 0
    assert lib.uavsal_train_decoder_sizeof_desc(3) < 0 and lib.uavsal_abi_version() == 20      # the older lists stay closed
    assert _lib.IR_NSUM == BR.NSUM == 11
    assert train.BLOCK_PARAMS == BR.NAMES == train.DECODER_PARAMS


def test_gemm_share_count_with_an_n_tail_is_the_restated_partition(lib):
    d = _lib.PixGemmDesc()
    for (M, N) in ((1920, 320), (256, 1920), (1536, 256), (256, 1536), (128, 64)):
        for shape in BR.SHAPES + [(5, 45, 80), (6, 45, 80), (7, 45, 80), (20, 45, 80)]:
            K = shape[0] * shape[1] * shape[2]
            cps, shares, spans = BR.gemm_partition(K, M, N)
            d.K, d.M, d.N = K, M, N
            assert lib.uavsal_pix_gemm_shares(C.byref(d)) == shares == len(spans), (M, N, shape)
            assert lib.uavsal_pix_gemm_workspace_bytes(C.byref(d)) == shares * M * N * 4
            assert spans[0][0] == 0 and spans[-1][1] == K and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    # the smallest frame count at 45 x 80 at which a share of the 1920 x 320 GEMM holds two chunks: 45 tiles -> at most 22
    # shares; T = 6 is 22 chunks, T = 7 is 25 chunks in 13 shares of 2, the last one a single chunk of 624 pixels
    assert BR.gemm_split_frames(1920, 320) == 7
    cps, shares, spans = BR.gemm_partition(7 * 45 * 80, 1920, 320)
    assert (cps, shares, spans[-1][1] - spans[-1][0], -(-7 * 45 * 80 // 1024)) == (2, 13, 624, 25)
    assert BR.gemm_partition(6 * 45 * 80, 1920, 320)[0] == 1
    # a multiple of 128 keeps the decoder's partition
    import decoder_ref64 as DR
    for K in (105, 43200, 72000):
        assert BR.gemm_partition(K, 1536, 256) == DR.gemm_partition(K)
    for M, N in ((1920, 200), (1920, 32), (400, 256), (1500, 320)):                 # N % 64, M % 128
        d.K, d.M, d.N = 1000, M, N
        assert lib.uavsal_pix_gemm_shares(C.byref(d)) == 0 and lib.uavsal_pix_gemm_workspace_bytes(C.byref(d)) == 0


def test_slab_count_is_the_restated_partition(lib):
    for cfg in BR.CFGS:
        hid, cout = BR.CFG[cfg]["hid"], BR.CFG[cfg]["cout"]
        for shape in BR.SHAPES + [(20, 45, 80), (64, 90, 160), (300, 4, 4)]:
            T, H, W = shape
            sr, slabs = BR.slab_partition(T, H, W)
            d = _lib.IrSumsDesc()
            d.n_img, d.H, d.W, d.Ch, d.Co = T, H, W, hid, cout
            assert lib.uavsal_ir_sums_slab_rows(C.byref(d)) == sr and lib.uavsal_ir_sums_slabs(C.byref(d)) == slabs, shape
            assert lib.uavsal_ir_sums_workspace_bytes(C.byref(d)) == slabs * (11 * hid + cout) * 8
    assert BR.slab_partition(*BR.SLAB_SHAPE) == (7, 13) and 90 - 12 * 7 == 6 and 45 % 7 != 0
    assert 1920 % BR.GROUP == 128 and 1536 % BR.GROUP == 0                          # a partial last channel group in fucbst alone


def test_argument_validation_without_gpu(lib):
    g = _lib.PixGemmDesc()
    g.a = g.b = g.ws = g.out = 256
    g.K, g.M, g.N, g.lda, g.ldb, g.ldo = 100, 1920, 200, 1920, 320, 320
    assert lib.uavsal_pix_gemm(C.byref(g), None) == -3                    # N % 64
    g.N = 320
    assert lib.uavsal_pix_gemm(C.byref(g), None) == -1                    # accepted: the workspace is too small
    g.ws_bytes = lib.uavsal_pix_gemm_workspace_bytes(C.byref(g))
    g.ldb = 256
    assert lib.uavsal_pix_gemm(C.byref(g), None) == -1                    # rows shorter than N
    g.ldb, g.M = 320, 400
    assert lib.uavsal_pix_gemm(C.byref(g), None) == -3                    # M % 128
    b = _lib.IrBwdDesc()
    assert lib.uavsal_ir_bwd(C.byref(b), None) == -1
    b.gd = b.d = b.e = b.wd9 = b.s2 = b.ga = 256
    b.n_img, b.H, b.W, b.C = 1, 4, 4, 1922
    assert lib.uavsal_ir_bwd(C.byref(b), None) == -2                      # C % 4
    b.C, b.gd = 1920, 260
    assert lib.uavsal_ir_bwd(C.byref(b), None) == -2
    b.gd, b.H = 256, 0
    assert lib.uavsal_ir_bwd(C.byref(b), None) == -1
    s = _lib.IrSumsDesc()
    assert lib.uavsal_ir_sums(C.byref(s), None) == -1
    s.gd = s.d = s.e = s.ga = s.go = s.ws = 256
    s.n_img, s.H, s.W, s.Ch, s.Co, s.ldgo = 1, 4, 4, 1900, 256, 256
    assert lib.uavsal_ir_sums(C.byref(s), None) == -3                     # Ch % 64
    s.Ch = 1920
    assert lib.uavsal_ir_sums(C.byref(s), None) == -1                     # workspace too small
    s.ws_bytes = lib.uavsal_ir_sums_workspace_bytes(C.byref(s))
    s.ldgo = 128
    assert lib.uavsal_ir_sums(C.byref(s), None) == -1                     # rows shorter than Co
    s.ldgo = 258
    assert lib.uavsal_ir_sums(C.byref(s), None) == -2
    s.ldgo, s.ga = 256, 264
    assert lib.uavsal_ir_sums(C.byref(s), None) == -2
    f = _lib.IrFinishDesc()
    assert lib.uavsal_ir_finish(C.byref(f), None) == -1
    for n, _t in _lib.IrFinishDesc._fields_[:19]:
        if n != "ws_bytes":
            setattr(f, n, 256)
    f.Ch, f.Co, f.slabs = 1920, 256, 2
    assert lib.uavsal_ir_finish(C.byref(f), None) == -1                   # workspace too small
    f.ws_bytes = 2 * (11 * 1920 + 256) * 8
    f.rowdot3 = 260
    assert lib.uavsal_ir_finish(C.byref(f), None) == -2
    f.rowdot3, f.Ch = 256, 100
    assert lib.uavsal_ir_finish(C.byref(f), None) == -3


# ------------------------------------------------------------------------------------------------ restatement vs goldens
@pytest.mark.parametrize("cs", SMALL, ids=_id)
def test_closed_form_matches_the_reference_autograd(cs):
    cfg, shape = cs
    g = np.load(os.path.join(GOLDEN, BR.name(cfg, shape) + ".npz"))
    xn, qn, gon = BR.block_case(cfg, shape)
    assert str(g["digest"]) == R.digest(xn, gon, *[qn[k] for k in sorted(qn)]) and int(g["seed"]) == BR._seed(cfg, shape)
    x, q, go, got, _, _ = case(cfg, shape)

    def close(a, b):
        assert float(np.abs(a - b).max()) <= 1e-10 * float(np.abs(b).max())
    for n in BR.NAMES:
        if n not in (BR.NAMES[0], BR.NAMES[6]):
            close(got[n].numpy(), g[n.replace(".", "_")])
    for key, n in (("W1", BR.NAMES[0]), ("W3", BR.NAMES[6])):
        w = got[n].numpy()[:, :, 0, 0]
        close(w[BR.W_SUBSET], g[key])
        assert abs(float(w.sum()) - float(g[key + "_sum"])) <= 1e-10 * float(g[key + "_l2"]) * np.sqrt(w.size)
        assert abs(float(np.sqrt((w * w).sum())) - float(g[key + "_l2"])) <= 1e-10 * float(g[key + "_l2"])
    close(BR.grad_x_ref(q, x, go, BR.CFG[cfg]["res"]).numpy()[BR.GX_SUBSET], g["grad_x"])


@pytest.mark.parametrize("cfg", BR.CFGS)
@pytest.mark.parametrize("zero_gamma", [False, True])
def test_closed_form_is_torch_autograd(cfg, zero_gamma):
    """Also with a zero gamma: the gamma gradients of those channels are not zero, their weight-gradient rows are."""
    shape = (3, 5, 7)
    x, q, go, got, _, parts = case(cfg, shape, zero_gamma)
    res = BR.CFG[cfg]["res"]
    ref, gx = BR.autograd_grads(q, x, go, res)
    for n in BR.NAMES:
        assert float((got[n] - ref[n]).abs().max()) <= 1e-12 * float(ref[n].abs().max()), n
    mine = parts["grad_x"] + go if res else parts["grad_x"]
    assert float((mine - gx).abs().max()) <= 1e-12 * float(gx.abs().max())
    e2e = BR.block_e2e(q, x, go, res)[0]
    assert float((e2e - gx).abs().max()) <= 1e-12 * float(gx.abs().max())
    if zero_gamma:
        c1, c2 = BR.ZERO_GAMMA
        assert float(got[BR.NAMES[0]][c1].abs().max()) == 0 and float(got[BR.NAMES[1]][c1].abs()) > 0
        assert float(got[BR.NAMES[3]][c2].abs().max()) == 0 and float(got[BR.NAMES[4]][c2].abs()) > 0


@pytest.mark.parametrize("cs", CASES, ids=_id)
def test_inputs_populate_every_class_and_stored_values_keep_every_mask(cs):
    cfg, shape = cs
    x, q, go, _, bounds, parts = case(cfg, shape)
    for k in ("e", "d"):
        shares = BR.class_shares(parts[k])
        print("%s %s: shares at or below 0 / inside / at or above 6: %.3f %.3f %.3f" % ((BR.name(cfg, shape), k) + shares))
        assert min(shares) >= 0.01, (k, shares)
        t = parts[k]                                                         # what the GPU tests hand over flips no mask
        t32 = BR.teacher_round(t).double()
        assert bool((((t > 0) & (t < 6)) == ((t32 > 0) & (t32 < 6))).all())
        assert bool(((t32 - t).abs() <= 2 * BR.U * t.abs()).all())
    for i in (1, 2, 3):                                                      # the statistics are not trivial
        assert sorted(set((1.0 / torch.sqrt(q["var%d" % i] + BR.BN_EPS)).tolist())) == [0.5, 1.0, 2.0]
        assert float(q["mu%d" % i].abs().mean()) > 0.5
    assert all(bool((b > 0).all()) for b in bounds.values())
    # the end-to-end test's widened limit cannot hide a structural error: the undecided masks' term stays a small part of grad_x
    gx, bound, und, _ = BR.block_e2e(q, x, go, BR.CFG[cfg]["res"])
    ratio = (R.l2_per_frame(bound + und) / R.l2_per_frame(gx)).max()
    print("%s: end-to-end limit / ||grad_x|| per frame at most %.3f" % (BR.name(cfg, shape), float(ratio)))
    assert float(ratio) <= 0.15


@pytest.mark.parametrize("cs", SMALL, ids=_id)
def test_wrong_kernels_lie_outside_the_bound(cs):
    """Each wrong kernel of block_ref64.WRONG is at least 4 bounds from the right result on some element of some tensor, so
    that a kernel within 1 bound of the right result cannot be one of them.  (At these shapes uavsal_pix_gemm runs one
    share: dropping the last share drops everything; the GPU test at T = 7 drops a real last share.  The N tail and the
    channel-group tail exist in fucbst alone: 320 = 2.5 tiles, 1920 = 7.5 groups.)"""
    cfg, shape = cs
    x, q, go, right, bound, parts = case(cfg, shape)
    c = BR.CFG[cfg]
    for v in BR.WRONG:
        if v in ("n_tail", "group_tail") and c["hid"] % 256 == 0:
            continue
        wrong = BR.param_grads(q, x, go, variant=v)
        ratio = {n: float(((wrong[n] - right[n]).abs() / bound[n]).max()) for n in BR.NAMES}
        worst = max(ratio, key=ratio.get)
        print("%s %s: up to %.1f bounds from the right result (%s)" % (BR.name(cfg, shape), v, ratio[worst], worst))
        assert ratio[worst] >= 4.0, v
    # uavsal_ir_bwd's own wrong kernels against its own bound
    p = BR.fold(q)
    ga_bound = BR.ir_bwd_bound(p, parts["gd"], parts["d"], parts["e"])
    for v in ("taps_flipped", "halo_across_frames", "nonstrict_masks"):
        wrong = BR.ir_bwd_ref(p, parts["gd"], parts["d"], parts["e"], variant=v)
        far = (wrong - parts["ga"]).abs() >= 4 * ga_bound
        assert bool((far & (ga_bound > 0)).any()), v
    if c["res"]:                                                             # the residual term of grad_x
        gx, b, und, _ = BR.block_e2e(q, x, go, True)
        miss = BR.grad_x_ref(q, x, go, True, variant="no_residual")
        assert bool((R.l2_per_frame(miss - gx) >= 4 * R.l2_per_frame(b + und)).all())


# ------------------------------------------------------------------------------------------------ the weight cache
def _block(cfg="fucbst"):
    from iip_uavsal_saliency_amd.model import dwBlock
    _, q, _ = BR.block_case(cfg, (3, 5, 7))
    c = BR.CFG[cfg]
    return BR.load_block(dwBlock(c["cin"], c["cout"], kernel_size=3), q)


@pytest.mark.parametrize("cfg", BR.CFGS)
def test_cache_entries_of_the_block_refresh_in_place(cfg):
    from iip_uavsal_saliency_amd import packing as P
    blk = _block(cfg)
    assert bool(blk.use_res_connect) == BR.CFG[cfg]["res"]
    pw, pwbn, dwc, dwbn, pl, plbn = train._block_parts(blk)
    hid, cout = BR.CFG[cfg]["hid"], BR.CFG[cfg]["cout"]

    def entries(c):
        return {"bn1": c.affine(pwbn, hid), "bn3": c.affine(plbn, cout), "dw": c.depthwise(dwc, dwbn),
                "wTs1": c.conv_t_scaled(pw, pwbn, "f32"), "wTs3": c.conv_t_scaled(pl, plbn, "f32"),
                "st1": c.bn_stats(pwbn), "st2": c.bn_stats(dwbn), "st3": c.bn_stats(plbn),
                "w1": c.conv(pw, None, 0, "f32"), "w3": c.conv(pl, None, 0, "f32")}
    store = {}
    c = WeightCache("cpu", store)
    ent = entries(c)
    keys = set(store)
    assert len(keys) == len(ent) and {k[0] for k in keys} == {"bn", "dw", "wTs", "bnstat", "w"}
    s3 = P.fold_bn(plbn)[0]
    want = P.pack_conv_weight((pl.weight.detach() * s3.view(-1, 1, 1, 1)).transpose(0, 1), "f32")
    assert torch.equal(ent["wTs3"], want)
    as_tuple = lambda v: v if isinstance(v, tuple) else (v,)               # noqa: E731
    ptrs = {k: [t.data_ptr() for t in as_tuple(v)] for k, v in store.items()}
    with torch.no_grad():
        for p_ in blk.parameters():
            p_.mul_(1.25).add_(0.01)
    mods = {id(m): m for m in torch.nn.Sequential(blk).modules()}          # the container, as model.fucbst_layer is
    assert c.refresh(mods, dry=True) == len(keys)
    assert torch.equal(ent["wTs3"], want)                                  # the dry pass copies nothing
    assert c.refresh(mods) == len(keys) and set(store) == keys
    assert ptrs == {k: [t.data_ptr() for t in as_tuple(v)] for k, v in store.items()}
    again = entries(WeightCache("cpu", {}))
    for k in ent:
        for a, b in zip(as_tuple(ent[k]), as_tuple(again[k])):
            assert torch.equal(a, b), k
    assert not torch.equal(ent["wTs3"], want)


def test_python_entry_points_refuse_what_they_do_not_cover():
    from iip_uavsal_saliency_amd.model import dwBlock
    blk = _block()
    x = torch.zeros(2, 320, 4, 4)
    g = torch.zeros(2, 256, 4, 4)
    with pytest.raises(RuntimeError, match="cuda"):
        train.block_backward(blk, x, g)
    with pytest.raises(RuntimeError, match="cuda"):
        train.block_param_grads(blk, x, None, None, g)
    with pytest.raises(RuntimeError, match="eval"):
        train.block_backward(blk.train(), x, g)
    with pytest.raises(RuntimeError, match="eval"):
        train.block_param_grads(blk, x, None, None, g)
    for bad in (dwBlock(256, 256, kernel_size=3, expand_ratio=1), dwBlock(256, 256, kernel_size=3, stride=2),
                dwBlock(256, 256, kernel_size=3, dilation=6), dwBlock(256, 64, kernel_size=3), dwBlock(96, 128, kernel_size=3),
                dwBlock(256, 1, kernel_size=3)):
        with pytest.raises(RuntimeError, match="expand conv|Cout"):
            train.block_backward(bad.eval(), x, g)
    foreign = dwBlock(256, 256, kernel_size=3).eval()                       # a block that does not say its stride: not taken on trust
    del foreign.stride
    with pytest.raises(RuntimeError, match="expand conv"):
        train.block_backward(foreign, x, g)
    t = torch.zeros(1, 4, 4, 64)
    with pytest.raises(RuntimeError, match="cuda"):
        train.ir_bwd(t, t, t, torch.zeros(9, 64), torch.zeros(64))
    with pytest.raises(RuntimeError, match="cuda"):
        train.ir_sums(t, t, t, t, torch.zeros(1, 128, 4, 4))
    for stages in (("decoder",), ("fuse",), ("rnn", "fuse", "decoder"), ("rnn", "fuse", "fuse"), ()):
        with pytest.raises(ValueError, match="stages"):
            stream.finetune_video(None, None, None, None, None, None, None, stages=stages)


class _Stub:
    time_dims = 5

    def __init__(self, num_cb):
        self.rnn, self.conv_out_st, self.fucbst_layer, self.fust_layer = object(), object(), object(), object()
        self.num_cb, self.refreshed = num_cb, []
        self.w = torch.nn.Parameter(torch.zeros(1))

    def parameters(self):
        return iter([self.w])

    def refresh_weights(self, *mods):
        self.refreshed.append(mods)


class _Opt:
    def __init__(self):
        self.log = []

    def zero_grad(self):
        self.log.append("zero")

    def step(self):
        self.log.append("step")


def test_finetune_video_stages(monkeypatch):
    """Every group's step passes exactly the stages' keyword arguments and refreshes exactly the trained stages."""
    n = 20
    frames = torch.zeros(n, 3, 72, 128, dtype=torch.uint8)
    has = torch.ones(n, 2, dtype=torch.bool)
    seen = []

    def step(model, x, cb, state, y, criterion, **kw):
        seen.append(kw)
        return torch.tensor(1.0), None, [torch.tensor(0.0)]
    monkeypatch.setattr(train, "recurrence_step", step)
    fix = torch.zeros(n, 4, 4, dtype=torch.uint8)
    for stages, kw in ((("rnn", "decoder", "fuse"), {"decoder": True, "fuse": True}), (("rnn", "fuse"), {"fuse": True}),
                       (("rnn", "decoder"), {"decoder": True}), (("rnn",), {})):
        for num_cb in (2, 0):
            m, opt = _Stub(num_cb), _Opt()
            del seen[:]
            r = stream.finetune_video(m, frames, torch.zeros(8, 9, 16), torch.zeros(20, 9, 16), fix, fix, opt, batch_size=2,
                                      criterion=object(), prepare=lambda a, b, h, w, l: (torch.zeros(n, 2, h, w), has),
                                      stages=stages)
            assert r["groups_run"] == 2 and seen == [kw] * 2 and opt.log == ["zero", "step"] * 2
            want = (m.rnn,) + ((m.conv_out_st,) if "decoder" in stages else ())
            if "fuse" in stages:
                want += (m.fucbst_layer if num_cb else m.fust_layer,)
            assert m.refreshed == [want] * 2


def test_fuse_block_of_a_model():
    from iip_uavsal_saliency_amd import UAVSal
    m = UAVSal(time_dims=4)
    blk, src = train.fuse_block(m)
    assert blk is m.fucbst_layer[0] and src == "fu320" and (blk.cin, blk.hidden, blk.cout, blk.use_res_connect) == (320, 1920, 256, False)
    train._block_parts(blk.eval())
    m0 = UAVSal(time_dims=4, bias_type=[0, 0, 0])
    blk, src = train.fuse_block(m0)
    assert blk is m0.fust_layer[0] and src == "st1" and (blk.cin, blk.hidden, blk.cout, blk.use_res_connect) == (256, 1536, 256, True)
    train._block_parts(blk.eval())
    from iip_uavsal_saliency_amd.engine import Engine
    assert "fu320" in Engine.TAPS_ON_REQUEST and "fu320" not in Engine.TAP_NAMES and "st1" in Engine.TAP_NAMES
