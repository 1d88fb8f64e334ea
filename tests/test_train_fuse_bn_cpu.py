"""The fusion block on batch statistics without a GPU: the new symbol, its descriptor's size query and argument checks
(csrc/train_bn.hip: uavsal_bn_apply_res), the float64 restatement tests/fuse_bn_ref64.py against torch's own
`F.batch_norm(training=True)` autograd and against the goldens recorded from the reference's `dwBlock` / `ConvTWA` in `.train()`
mode, the wrong variants each at least 4 test bounds from the right answer, and the refusals and keyword plumbing of
`recurrence_step(block_stats=...)` and `stream.finetune_video(block_stats=...)` against stubbed entry points."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import _lib, stream, train

import decoder_bn_ref64 as BR
import fuse_bn_ref64 as FR
import lstm_ref64 as LR
import train_ref64 as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [(cfg, shape) for cfg in FR.CFGS for shape in FR.SHAPES]
IDS = [FR.name(c, s) for c, s in CASES]
_cases = {}


def t64(a):
    return torch.as_tensor(a).double()


def case(cfg, shape):
    """(x, q, go) as float64 tensors and the closed form, once per case"""
    if (cfg, shape) not in _cases:
        x, q, go = FR.block_case(cfg, shape)
        x, q, go = t64(x), FR.to64(q), t64(go)
        _cases[cfg, shape] = (x, q, go, FR.block_train(q, x, go, FR.CFG[cfg]["res"]))
    return _cases[cfg, shape]


def chain():
    if "chain" not in _cases:
        x, qb, h0, w, qd, gy = FR.chain_case()
        args = (FR.to64(qb), t64(x), t64(h0), t64(w), FR.to64(qd), t64(gy))
        _cases["chain"] = (args, FR.chain_train(*args))
    return _cases["chain"]


@pytest.fixture(scope="module")
def lib():
    from iip_uavsal_saliency_amd import build
    build.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ the library
def test_symbols_sizes_and_constants(lib):
    names = [s[0] for s in _lib.SYMBOLS]
    for n in ("uavsal_bn_apply_res", "uavsal_block_bn_sizeof_desc"):
        assert n in names and hasattr(lib, n)
    assert len(_lib.BLOCK_BN_DESC_TYPES) == 1
    for i, t in enumerate(_lib.BLOCK_BN_DESC_TYPES):
        assert lib.uavsal_block_bn_sizeof_desc(i) == C.sizeof(t)
    assert lib.uavsal_block_bn_sizeof_desc(len(_lib.BLOCK_BN_DESC_TYPES)) < 0 and lib.uavsal_block_bn_sizeof_desc(-1) < 0
    assert lib.uavsal_bn_sizeof_desc(4) < 0 and len(_lib.BN_DESC_TYPES) == 4 and lib.uavsal_abi_version() == 20
    assert train.BLOCK_STATS == ("fuse",) and train.BATCH_STATS == ("decoder",)
    for f in ("block_forward_batch", "block_backward_batch", "twa_forward", "lstm_forward", "fuse_container"):
        assert callable(getattr(train, f))


def test_argument_validation_without_gpu(lib):
    a = _lib.BnApplyResDesc()
    assert lib.uavsal_bn_apply_res(C.byref(a), None) == -1
    a.u = a.s = a.b = a.out = 256
    a.n_pix, a.C, a.ld, a.ldr, a.act = 70, 8, 8, 8, 0
    assert lib.uavsal_bn_apply_res(C.byref(a), None) == -1                # no residual: that is uavsal_bn_apply
    a.res = 256
    a.act = 3
    assert lib.uavsal_bn_apply_res(C.byref(a), None) == -1                # no such activation
    a.act, a.C, a.ld, a.ldr = 0, 6, 8, 8
    assert lib.uavsal_bn_apply_res(C.byref(a), None) == -3                # C % 4
    a.C, a.ldr = 8, 4
    assert lib.uavsal_bn_apply_res(C.byref(a), None) == -1                # the residual's pitch below C
    a.ldr = 10
    assert lib.uavsal_bn_apply_res(C.byref(a), None) == -2                # ... not a multiple of 4
    a.ldr, a.res = 12, 260
    assert lib.uavsal_bn_apply_res(C.byref(a), None) == -2                # ... its pointer not 16-byte aligned
    a.res, a.ld = 256, 4
    assert lib.uavsal_bn_apply_res(C.byref(a), None) == -1
    a.ld, a.ldr, a.n_pix = 8, 8, 2 ** 62
    assert lib.uavsal_bn_apply_res(C.byref(a), None) == -3                # n_pix * C / 4 does not fit 64 bits


# ------------------------------------------------------------------------------------------------ the restatement
def _close(a, b, rel=1e-11):
    b = torch.as_tensor(b)
    return float((a - b).abs().max()) <= rel * max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("cfg,shape", CASES, ids=IDS)
def test_closed_form_is_torch_autograd_in_training_mode(cfg, shape):
    x, q, go, mine = case(cfg, shape)
    auto = FR.block_autograd(q, x, go, FR.CFG[cfg]["res"])
    for n in FR.NAMES + ("out", "grad_x"):
        assert mine[n].shape == auto[n].shape and _close(mine[n], auto[n]), n
    for i in (1, 2, 3):
        assert _close(mine["rm%d" % i], auto["rm%d" % i]) and _close(mine["rv%d" % i], auto["rv%d" % i])
        assert not _close(mine["rm%d" % i], q["rm%d" % i], 1e-3)          # they moved
    c1, c2 = FR.ZERO_GAMMA                                                # gamma = 0: no gradient into u, a gamma gradient
    assert float(mine["g_u1"][..., c1].abs().max()) == 0 and float(mine[FR.NAMES[1]][c1].abs()) > 0
    assert float(mine["g_u2"][..., c2].abs().max()) == 0 and float(mine[FR.NAMES[4]][c2].abs()) > 0


def _summed(g, key, t, subset):
    """the subset and the L2 norm to 1e-11 relative; the sum to 1e-11 of sqrt(n) ||t||_2 >= sum |t|, the scale of its terms (a
    gradient behind a BatchNorm on batch statistics sums to ZERO over the pixels, up to rounding)"""
    scale = 1e-11 * float(t.norm()) * t.numel() ** 0.5
    return (_close(t[subset], g[key]) and abs(float(t.sum()) - float(g[key + "_sum"])) <= scale and _close(t.norm(), g[key + "_l2"]))


def _grads_match(g, mine, pre, w_subset, wd_subset):
    for n in (FR.NAMES[1], FR.NAMES[2], FR.NAMES[4], FR.NAMES[5], FR.NAMES[7], FR.NAMES[8]):
        assert _close(mine[n], torch.as_tensor(g[pre + n.replace(".", "_")]).reshape(mine[n].shape)), pre + n
    w3 = mine[FR.NAMES[6]][:, :, 0, 0]
    assert _summed(g, pre + "W1", mine[FR.NAMES[0]][:, :, 0, 0], w_subset)
    assert _summed(g, pre + "W3", w3, w_subset if w3.shape[0] > 1 else (slice(None), slice(None)))
    assert _summed(g, pre + "Wd", mine[FR.NAMES[3]], wd_subset)


@pytest.mark.parametrize("cfg,shape", CASES, ids=IDS)
def test_closed_form_matches_the_reference_block_in_train_mode(cfg, shape):
    g = np.load(os.path.join(GOLDEN, FR.name(cfg, shape) + ".npz"))
    xn, qn, gon = FR.block_case(cfg, shape)
    assert str(g["digest"]) == R.digest(xn, gon, *[qn[k] for k in sorted(qn)]) and tuple(g["shape"]) == shape
    _, _, _, mine = case(cfg, shape)
    _grads_match(g, mine, "", FR.W_SUBSET, FR.WD_SUBSET)
    assert _summed(g, "out", mine["out"], FR.GX_SUBSET) and _summed(g, "grad_x", mine["grad_x"], FR.GX_SUBSET)
    assert int(g["nbt"]) == 1
    for i in (1, 2, 3):
        for k in ("mu%d", "var%d", "rm%d", "rv%d"):
            assert _close(mine[k % i], g[k % i]), k % i


def test_chain_is_torch_autograd_and_the_reference_chain():
    args, mine = chain()
    auto = FR.chain_autograd(*args)
    assert _close(mine["y"], auto["y"]) and _close(mine["rnn"], auto["rnn"]) and _close(mine["grad_x"], auto["grad_x"])
    for part in ("block", "decoder"):
        for n in FR.NAMES:
            assert _close(mine[part][n], auto[part][n].reshape(mine[part][n].shape)), (part, n)
    g = np.load(os.path.join(GOLDEN, FR.chain_name() + ".npz"))
    x, qb, h0, w, qd, gy = FR.chain_case()
    assert str(g["digest"]) == R.digest(x, h0, w, gy, *[qb[k] for k in sorted(qb)], *[qd[k] for k in sorted(qd)])
    assert _close(mine["y"], g["y"]) and _summed(g, "h_seq", mine["h_seq"], FR.GX_SUBSET)
    assert _summed(g, "rnn", mine["rnn"], FR.CHAIN_RNN_SUBSET) and _summed(g, "grad_x", mine["grad_x"], FR.GX_SUBSET)
    for part in ("block", "decoder"):
        _grads_match(g, mine[part], part + "_", FR.CHAIN_W_SUBSET, FR.CHAIN_WD_SUBSET)
        for i in (1, 2, 3):
            for k in ("mu%d", "var%d", "rm%d", "rv%d"):
                assert _summed(g, part + "_" + k % i, mine[part][k % i], FR.CHAIN_C_SUBSET), (part, k % i)
    assert float(args[2].abs().max()) > 0                                  # the chain starts from a non-zero state


@pytest.mark.parametrize("cfg,shape", CASES, ids=IDS)
def test_inputs_hit_both_clamps(cfg, shape):
    """The condition of the GPU test, on the same seeds: at least 5 % of e and of d in each clamp."""
    _, _, _, mine = case(cfg, shape)
    for what in ("e", "d"):
        lo, mid, hi = FR.clamp_shares(mine[what])
        print("%s %s: %.1f %% at 0, %.1f %% inside, %.1f %% at 6" % (FR.name(cfg, shape), what, 100 * lo, 100 * mid, 100 * hi))
        assert lo >= 0.05 and hi >= 0.05 and mid >= 0.25


# ------------------------------------------------------------------------------------------------ wrong variants
def _ratio(wrong, right, bound):
    return float(((wrong - right).abs() / bound.clamp_min(1e-300)).max())


@pytest.mark.parametrize("cfg,shape", CASES, ids=IDS)
def test_wrong_blocks_lie_outside_the_bound(cfg, shape):
    """Each wrong implementation is at least 4 bounds of the stage test that holds it (tests/test_train_fuse_bn_gpu.py's walk)
    from the right result, teacher-forced on the float64 tensors of the right chain; the running statistics: 4 fp32 ulps where
    the test allows one.  (Dropping the last slab needs a shape with two: SLAB_SHAPE; at (2,5,7) the one slab is everything.)"""
    x, q, go, m = case(cfg, shape)
    res = FR.CFG[cfg]["res"]
    xn, gon = x.permute(0, 2, 3, 1), go.permute(0, 2, 3, 1)
    f = {i: BR.stats(m["u%d" % i], q["g%d" % i], q["be%d" % i]) for i in (1, 2, 3)}
    seen = {}
    # BN3's eval-mode gradient (both statistics terms dropped)
    s3 = BR.bwd_sums(gon, m["u3"], f[3], FR.ACT_NONE)
    right, bound = BR.bwd_apply(gon, m["u3"], f[3], s3, FR.ACT_NONE, bounds=True)
    seen["bn3_eval_grad"] = _ratio(f[3]["s"] * gon, right, bound)
    # dW3 from u2 instead of d
    right, bound = BR.pix_gemm(m["g_u3"], m["d"])
    seen["dw3_from_u2"] = _ratio(BR.pix_gemm(m["g_u3"], m["u2"])[0], right, bound)
    # the statistics of frame 0 alone / without the last slab, in every BatchNorm
    for v in ("per_frame", "last_slab"):
        worst = 1e300
        for i in (1, 2, 3):
            right, bound = BR.stats(m["u%d" % i], q["g%d" % i], q["be%d" % i], bounds=True)
            wrong = BR.stats(m["u%d" % i], q["g%d" % i], q["be%d" % i], variant=v)
            worst = min(worst, max(_ratio(wrong[k], right[k], bound[k]) for k in ("mu", "var", "r", "s", "b")))
        seen[v] = worst
    # biased running variance
    P = xn.shape[0] * xn.shape[1] * xn.shape[2]
    _, rv = BR.running(q["rm1"], q["rv1"], f[1]["mu"], f[1]["var"], P)
    _, wv = BR.running(q["rm1"], q["rv1"], f[1]["mu"], f[1]["var"], P, variant="biased_running")
    seen["biased_running"] = float(((wv - rv).abs() / (rv.abs() * 2 * BR.U)).max())
    if res:
        right, bound = FR.grad_x(m["g_u1"], q["w1"], gon)
        seen["no_residual_gx"] = _ratio(FR.grad_x(m["g_u1"], q["w1"])[0], right, bound)
        right, bound = FR.apply_res(m["u3"], f[3], xn)
        wrong = FR.block_train(q, x, go, True, variant="res_before_bn3")["out"].permute(0, 2, 3, 1)
        seen["res_before_bn3"] = _ratio(wrong, right, bound)
    for v, r in seen.items():
        print("%s %s: %.3g bounds" % (FR.name(cfg, shape), v, r))
        assert r >= 4.0, v
    assert set(seen) == set(FR.WRONG_BLOCK) - (set() if res else {"no_residual_gx", "res_before_bn3"})


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def test_wrong_chains_lie_outside_the_whole_chain_tolerance():
    """`FR.CHAIN_TOL`, the relative L2 tolerance of the GPU test's whole chain, separates right from wrong: every wrong block
    (at SLAB_SHAPE, where dropping the last slab is not dropping everything) and every wrong recurrence (the chain's inputs)
    moves a tensor by at least 4 of it -- all but the biased running variance (fuse_bn_ref64's docstring)."""
    assert 2.5e-3 < FR.CHAIN_TOL < 2.7e-3
    for cfg in FR.CFGS:
        x, q, go, right = case(cfg, FR.SLAB_SHAPE)
        res = FR.CFG[cfg]["res"]
        for v in FR.WRONG_BLOCK:
            if v == "biased_running" or (not res and v in ("no_residual_gx", "res_before_bn3")):
                continue
            wrong = FR.block_train(q, x, go, res, variant=v)
            worst = max(_rel(wrong[n], right[n]) for n in FR.NAMES + ("out", "grad_x"))
            print("%s %s: %.3g CHAIN_TOL" % (cfg, v, worst / FR.CHAIN_TOL))
            assert worst >= 4 * FR.CHAIN_TOL, (cfg, v)
        wrong = FR.block_train(q, x, go, res, variant="biased_running")
        assert 0 < _rel(wrong["rv1"], right["rv1"]) < FR.CHAIN_TOL          # the exception, as stated
    args, mine = chain()
    for v in FR.WRONG_RNN:
        d = _rel(FR.twa_forward(mine["x_seq"], args[2], args[3], variant=v), mine["h_seq"])
        print("chain %s: %.3g CHAIN_TOL" % (v, d / FR.CHAIN_TOL))
        assert d >= 4 * FR.CHAIN_TOL, v


@pytest.mark.parametrize("shape", FR.RNN_SHAPES, ids=R.name)
def test_wrong_recurrences_lie_outside_the_step_bound(shape):
    t = FR.to64(R.twa_inputs(shape))
    x, h0, w = t["x"], t["h0"], t["w"]
    hs = FR.twa_forward(x, h0, w)
    T = x.shape[0]
    k = T - 1                                                              # the last step, teacher-forced on the right history
    right, bound = FR.twa_step(x[k:k + 1], hs[k - 1:k], w)
    seen = {"h_tm2": _ratio(FR.twa_step(x[k:k + 1], hs[k - 1:k], w, variant="h_tm2", h_other=hs[k - 2:k - 1])[0], right, bound),
            "swapped": _ratio(FR.twa_step(x[k:k + 1], hs[k - 1:k], w, variant="swapped")[0], right, bound)}
    if shape in R.H0_NONZERO:                                              # (with a zero state there is nothing to ignore)
        right0, bound0 = FR.twa_step(x[:1], h0, w)
        seen["h0_ignored"] = _ratio(FR.twa_step(x[:1], torch.zeros_like(h0), w)[0], right0, bound0)
    for v, r in seen.items():
        print("%s %s: %.3g bounds" % (R.name(shape), v, r))
        assert r >= 4.0, v
    # and carried through the whole sequence they move the history far outside float64's own agreement
    for v in FR.WRONG_RNN:
        if v == "h0_ignored" and shape not in R.H0_NONZERO:
            continue
        assert float((FR.twa_forward(x, h0, w, variant=v) - hs).abs().max()) >= 1e-3, v
    assert float(bound.max()) < 1e-2 and _close(FR.twa_step(x[:1], h0, w)[0], hs[:1])


def test_lstm_step_restates_the_reference_recurrence():
    shape = FR.RNN_SHAPES[1]
    t = FR.to64(LR.lstm_inputs(shape))
    hs, cs, _ = LR.lstm_forward(t["x"], t["h0"], t["c0"], t["w"])
    h, c = t["h0"], t["c0"]
    for k in range(shape[0]):
        h, c, bh, bc = FR.lstm_step(t["x"][k:k + 1], h, c, t["w"])
        assert _close(h, hs[k:k + 1]) and _close(c, cs[k:k + 1]) and float(bh.max()) < 1e-2 and float(bc.max()) < 1e-2


# ------------------------------------------------------------------------------------------------ refusals and plumbing
def _block(cfg="fust", shape=(2, 5, 7)):
    from iip_uavsal_saliency_amd.model import dwBlock
    c = FR.CFG[cfg]
    _, q, _ = FR.block_case(cfg, shape)
    return FR.load_block(dwBlock(c["cin"], c["cout"], kernel_size=3), q)


def test_python_entry_points_refuse_what_they_do_not_cover():
    blk = _block()
    t = torch.zeros(2, 256, 4, 4)
    for fn, args in ((train.block_forward_batch, (t,)), (train.block_backward_batch, (t, t))):
        with pytest.raises(RuntimeError, match="block_backward / block_input_grad"):
            fn(blk.eval(), *args)                                          # eval mode: the message names the eval-mode functions
        with pytest.raises(RuntimeError, match="cuda"):
            fn(blk.train(), *args)
    with pytest.raises(RuntimeError, match=r"model\.eval\(\)"):            # the eval-mode function keeps its refusal
        train.block_backward(blk.train(), t, t)
    from iip_uavsal_saliency_amd.model import dwBlock
    with pytest.raises(RuntimeError, match="stride 1 and dilation 1"):
        train.block_forward_batch(dwBlock(256, 256, kernel_size=3, stride=2).train(), t)
    with pytest.raises(RuntimeError, match="Cout % 128"):
        train.block_forward_batch(dwBlock(64, 64, kernel_size=3).train(), torch.zeros(2, 64, 4, 4))
    with pytest.raises(RuntimeError, match="cuda"):
        train.bn_apply(torch.zeros(2, 4, 4, 8), None, res=torch.zeros(2, 4, 4, 8))
    with pytest.raises(RuntimeError, match="cuda"):
        train.twa_forward(torch.zeros(2, 256, 4, 4), None, torch.zeros(256, 512, 3, 3))
    with pytest.raises(RuntimeError, match="cuda"):
        train.lstm_forward(torch.zeros(2, 256, 4, 4), None, None, torch.zeros(1024, 512, 3, 3))


class _Model:
    """what recurrence_step looks at before its first launch"""
    rnn_type, precision, training, num_cb = "twa", "f32", False, 0

    def __init__(self, box_training, num_cb=0):
        self.num_cb = num_cb
        self.fust_layer = torch.nn.Sequential(torch.nn.BatchNorm2d(1)).train(box_training and not num_cb)
        self.fucbst_layer = torch.nn.Sequential(torch.nn.BatchNorm2d(1)).train(box_training and bool(num_cb))
        self.conv_out_st = torch.nn.BatchNorm2d(1).eval()
        self.st_layer = [None]
        self.called = False

    def __call__(self, *a, **k):
        self.called = True
        raise AssertionError("a launch")


@pytest.mark.parametrize("num_cb", [0, 2])
def test_recurrence_step_refuses_before_any_launch(num_cb):
    x = torch.zeros(2, 3, 8, 8)
    box = "fucbst_layer" if num_cb else "fust_layer"
    m = _Model(True, num_cb)
    with pytest.raises(NotImplementedError, match="'fust'"):
        train.recurrence_step(m, x, None, None, x, fuse=True, block_stats=("fuse", "fust"))
    with pytest.raises(NotImplementedError, match="'decoder'"):           # the decoder's keyword is batch_stats
        train.recurrence_step(m, x, None, None, x, fuse=True, decoder=True, block_stats=("decoder",))
    with pytest.raises(NotImplementedError, match="fuse"):                 # and batch_stats keeps refusing the fuse stage
        train.recurrence_step(m, x, None, None, x, decoder=True, fuse=True, batch_stats=("decoder", "fuse"))
    with pytest.raises(RuntimeError, match="fuse=True"):
        train.recurrence_step(m, x, None, None, x, block_stats=("fuse",))
    with pytest.raises(RuntimeError, match=box + r"\.train\(\)"):
        train.recurrence_step(_Model(False, num_cb), x, None, None, x, fuse=True, block_stats=("fuse",))
    m.training = True
    with pytest.raises(RuntimeError, match=r"model\.eval\(\)"):
        train.recurrence_step(m, x, None, None, x, fuse=True, block_stats="fuse")
    m.training = False
    with pytest.raises(RuntimeError, match=r"conv_out_st\.train\(\)"):     # both keywords: each keeps its own precondition
        train.recurrence_step(m, x, None, None, x, fuse=True, decoder=True, block_stats=("fuse",), batch_stats=("decoder",))
    with pytest.raises(RuntimeError, match="cuda"):                        # everything the keyword asks is met: the CPU tensors stop it
        train.recurrence_step(m, x, None, None, x, fuse=True, block_stats=("fuse",))
    assert not m.called


class _Stub:
    time_dims, num_cb = 5, 2

    def __init__(self):
        self.rnn, self.refreshed = object(), []
        self.conv_out_st = torch.nn.BatchNorm2d(1).eval()
        self.fucbst_layer = torch.nn.Sequential(torch.nn.BatchNorm2d(1)).eval()
        self.fust_layer = torch.nn.Sequential(torch.nn.BatchNorm2d(1)).eval()
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


def test_finetune_video_passes_block_stats_and_restores_the_mode(monkeypatch):
    n = 30
    frames = torch.zeros(n, 3, 72, 128, dtype=torch.uint8)
    has = torch.ones(n, 2, dtype=torch.bool)
    fix = torch.zeros(n, 4, 4, dtype=torch.uint8)
    seen = []

    def step(model, x, cb, state, y, criterion, **kw):
        seen.append((kw, model.fucbst_layer.training, model.fucbst_layer[0].training, model.conv_out_st.training,
                     model.fust_layer.training))
        return torch.tensor(1.0), None, [torch.tensor(0.0)]
    monkeypatch.setattr(train, "recurrence_step", step)

    def run(m, **kw):
        return stream.finetune_video(m, frames, torch.zeros(8, 9, 16), torch.zeros(20, 9, 16), fix, fix, _Opt(), batch_size=2,
                                     criterion=object(), prepare=lambda a, b, h, w, l: (torch.zeros(n, 2, h, w), has), **kw)
    m = _Stub()
    r = run(m, stages=("rnn", "decoder", "fuse"), block_stats=("fuse",))
    assert r["groups_run"] == 3
    assert seen == [({"decoder": True, "fuse": True, "block_stats": ("fuse",)}, True, True, False, False)] * 3
    assert not m.fucbst_layer.training and not m.fucbst_layer[0].training
    assert m.refreshed == [(m.rnn, m.conv_out_st, m.fucbst_layer)] * 3
    del seen[:]
    m.fucbst_layer.train()                                                 # a caller's own modes are restored too, per module
    m.fucbst_layer[0].eval()
    run(m, stages=("rnn", "fuse"), block_stats="fuse", batch_stats=())
    assert m.fucbst_layer.training and not m.fucbst_layer[0].training and seen[0][1:3] == (True, True)
    del seen[:]
    m = _Stub()
    run(m, stages=("rnn", "decoder", "fuse"), block_stats=("fuse",), batch_stats=("decoder",))      # the two keywords combine
    assert seen == [({"decoder": True, "fuse": True, "block_stats": ("fuse",), "batch_stats": ("decoder",)}, True, True, True,
                     False)] * 3
    assert not m.fucbst_layer.training and not m.conv_out_st.training
    del seen[:]
    m = _Stub()
    run(m, stages=("rnn", "decoder", "fuse"))                              # without the keyword: the call it always made
    assert seen == [({"decoder": True, "fuse": True}, False, False, False, False)] * 3
    with pytest.raises(ValueError, match="'fuse' in stages"):
        run(_Stub(), stages=("rnn", "decoder"), block_stats=("fuse",))
    with pytest.raises(NotImplementedError, match="'fust'"):
        run(_Stub(), stages=("rnn", "fuse", "fust"), block_stats=("fuse", "fust"))

    def boom(model, x, cb, state, y, criterion, **kw):
        raise KeyError("stop")
    monkeypatch.setattr(train, "recurrence_step", boom)
    m = _Stub()
    with pytest.raises(KeyError):
        run(m, stages=("rnn", "fuse"), block_stats=("fuse",))
    assert not m.fucbst_layer.training and not m.fucbst_layer[0].training  # restored when a step raises
