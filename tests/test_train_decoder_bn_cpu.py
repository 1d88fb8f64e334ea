"""BatchNorm on batch statistics without a GPU: the library's symbols, sizes, slab query and argument checks (csrc/train_bn.hip),
the float64 restatement tests/decoder_bn_ref64.py against torch's own `F.batch_norm(training=True)` autograd and against the
goldens recorded from the reference's `dwBlock` in `.train()` mode, the wrong variants each at least 4 test bounds from the
right answer, and the refusals and keyword plumbing of train/ and stream.finetune_video against stubbed entry points."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import _lib, stream, train

import decoder_bn_ref64 as BR
import train_ref64 as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_cases = {}


def case(shape):
    """(h, q, gy) as float64 tensors and the closed form, once per shape"""
    if shape not in _cases:
        h, q, gy = BR.decoder_case(shape)
        h, q, gy = torch.as_tensor(h).double(), BR.to64(q), torch.as_tensor(gy).double()
        _cases[shape] = (h, q, gy, BR.decoder_train(q, h, gy))
    return _cases[shape]


@pytest.fixture(scope="module")
def lib():
    from iip_uavsal_saliency_amd import build
    build.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ the library
def test_symbols_and_sizes(lib):
    names = [s[0] for s in _lib.SYMBOLS]
    for n in ("uavsal_bn_stats", "uavsal_bn_stats_workspace_bytes", "uavsal_bn_apply", "uavsal_bn_bwd_sums", "uavsal_bn_bwd_apply",
              "uavsal_bn_bwd_workspace_bytes", "uavsal_dw_wgrad", "uavsal_dw_wgrad_workspace_bytes", "uavsal_bn_slabs",
              "uavsal_bn_slab_rows", "uavsal_bn_sizeof_desc"):
        assert n in names and hasattr(lib, n)
    assert len(_lib.BN_DESC_TYPES) == 4
    for i, t in enumerate(_lib.BN_DESC_TYPES):
        assert lib.uavsal_bn_sizeof_desc(i) == C.sizeof(t)
    assert lib.uavsal_bn_sizeof_desc(4) < 0 and lib.uavsal_abi_version() == 20
    assert lib.uavsal_shallow_sizeof_desc(1) < 0 and lib.uavsal_train_decoder_sizeof_desc(3) < 0      # the older lists stay closed
    assert train.DECODER_PARAMS == BR.NAMES and train.BATCH_STATS == ("decoder",)
    for f in ("bn_stats", "bn_apply", "bn_bwd_sums", "bn_bwd_apply", "decoder_forward_batch", "decoder_backward_batch"):
        assert callable(getattr(train, f))


def test_slab_count_is_the_restated_partition(lib):
    for shape in BR.KERNEL_SHAPES + [(20, 45, 80), (64, 90, 160), (300, 4, 4)]:
        T, H, W = shape
        sr, slabs = BR.slab_partition(T, H, W)
        assert (lib.uavsal_bn_slab_rows(T, H, W), lib.uavsal_bn_slabs(T, H, W)) == (sr, slabs), shape
        assert (slabs - 1) * sr < T * H <= slabs * sr and slabs <= BR.MAX_SLABS
        d = _lib.BnStatsDesc()
        d.n_img, d.H, d.W, d.C = T, H, W, 8
        assert lib.uavsal_bn_stats_workspace_bytes(C.byref(d)) == slabs * 2 * 8 * 8
        b = _lib.BnBwdDesc()
        b.n_img, b.H, b.W, b.C = T, H, W, 8
        assert lib.uavsal_bn_bwd_workspace_bytes(C.byref(b)) == slabs * 3 * 8 * 8
        w = _lib.DwWgradDesc()
        w.n_img, w.H, w.W, w.C = T, H, W, 8
        assert lib.uavsal_dw_wgrad_workspace_bytes(C.byref(w)) == slabs * 9 * 8 * 8
    # SLAB_SHAPE: two slabs, a partial last one, and the first ends inside a frame
    assert BR.slab_partition(*BR.SLAB_SHAPE) == (31, 2) and 39 - 31 == 8 and 31 % 13 != 0
    assert BR.slab_partition(2, 5, 7)[1] == 1 and BR.slab_partition(3, 5, 7)[1] == 1
    assert lib.uavsal_bn_slabs(0, 5, 7) == 0


def test_argument_validation_without_gpu(lib):
    s = _lib.BnStatsDesc()
    assert lib.uavsal_bn_stats(C.byref(s), None) == -1
    s.u = s.gamma = s.beta = s.ws = s.mu = s.var = s.r = s.s = s.b = 256
    s.n_img, s.H, s.W, s.C, s.ld, s.eps, s.momentum = 2, 5, 7, 6, 8, 1e-5, 0.1
    assert lib.uavsal_bn_stats(C.byref(s), None) == -3                    # C % 4 and C != 1
    s.C = 8
    assert lib.uavsal_bn_stats(C.byref(s), None) == -1                    # workspace too small
    s.ws_bytes = lib.uavsal_bn_stats_workspace_bytes(C.byref(s))
    s.ld = 6
    assert lib.uavsal_bn_stats(C.byref(s), None) == -1                    # pitch below C
    s.ld = 10
    assert lib.uavsal_bn_stats(C.byref(s), None) == -2                    # pitch not a multiple of 4
    s.ld, s.u = 8, 260
    assert lib.uavsal_bn_stats(C.byref(s), None) == -2
    s.u, s.momentum = 256, 1.5
    assert lib.uavsal_bn_stats(C.byref(s), None) == -1
    s.momentum, s.n_img, s.H, s.W, s.running_mean, s.running_var = 0.1, 1, 1, 1, 256, 256
    assert lib.uavsal_bn_stats(C.byref(s), None) == -3                    # one value has no unbiased variance
    a = _lib.BnApplyDesc()
    assert lib.uavsal_bn_apply(C.byref(a), None) == -1
    a.u = a.s = a.b = a.out = 256
    a.n_pix, a.C, a.ld, a.act = 70, 1, 1, 3
    assert lib.uavsal_bn_apply(C.byref(a), None) == -1                    # no such activation
    a.act, a.dot_w = 1, 256
    assert lib.uavsal_bn_apply(C.byref(a), None) == -3                    # the dot needs C % 4 == 0
    a.dot_w, a.C, a.ld = None, 10, 12
    assert lib.uavsal_bn_apply(C.byref(a), None) == -3
    b = _lib.BnBwdDesc()
    assert lib.uavsal_bn_bwd_sums(C.byref(b), None) == -1 and lib.uavsal_bn_bwd_apply(C.byref(b), None) == -1
    b.u = b.s = b.b = b.mu = b.r = b.sums = b.ws = 256
    b.n_img, b.H, b.W, b.C, b.ld = 2, 5, 7, 8, 8
    assert lib.uavsal_bn_bwd_sums(C.byref(b), None) == -1                 # neither g nor the rank-one pair
    b.g_pix = b.g_chan = 256
    assert lib.uavsal_bn_bwd_sums(C.byref(b), None) == -1                 # workspace too small
    assert lib.uavsal_bn_bwd_apply(C.byref(b), None) == -1                # no output
    b.g_chan = 260
    b.ws_bytes = lib.uavsal_bn_bwd_workspace_bytes(C.byref(b))
    assert lib.uavsal_bn_bwd_sums(C.byref(b), None) == -2
    w = _lib.DwWgradDesc()
    assert lib.uavsal_dw_wgrad(C.byref(w), None) == -1
    w.g = w.e = w.ws = w.out = 256
    w.n_img, w.H, w.W, w.C, w.ldg, w.lde = 2, 5, 7, 1, 4, 4
    assert lib.uavsal_dw_wgrad(C.byref(w), None) == -3
    w.C = 8
    assert lib.uavsal_dw_wgrad(C.byref(w), None) == -1                    # pitches below C


# ------------------------------------------------------------------------------------------------ the restatement
def _close(a, b, rel=1e-11):
    return float((a - b).abs().max()) <= rel * max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("shape", BR.SHAPES, ids=BR.name)
def test_closed_form_is_torch_autograd_in_training_mode(shape):
    h, q, gy, mine = case(shape)
    auto = BR.decoder_autograd(q, h, gy)
    for n in BR.NAMES + ("y", "grad_h"):
        assert mine[n].shape == auto[n].shape and _close(mine[n], auto[n]), n
    for i in (1, 2, 3):
        assert _close(mine["rm%d" % i], auto["rm%d" % i]) and _close(mine["rv%d" % i], auto["rv%d" % i])
        assert not _close(mine["rm%d" % i], q["rm%d" % i], 1e-3)          # they moved
    # the zero-gamma channels: no gradient into u, a gamma gradient all the same
    c1, c2 = BR.ZERO_GAMMA
    assert float(mine["g_u1"][..., c1].abs().max()) == 0 and float(mine[BR.NAMES[1]][c1].abs()) > 0
    assert float(mine["g_u2"][..., c2].abs().max()) == 0 and float(mine[BR.NAMES[4]][c2].abs()) > 0


@pytest.mark.parametrize("shape", BR.SHAPES, ids=BR.name)
def test_closed_form_matches_the_reference_block_in_train_mode(shape):
    g = np.load(os.path.join(GOLDEN, BR.name(shape) + ".npz"))
    hn, qn, gyn = BR.decoder_case(shape)
    assert str(g["digest"]) == R.digest(hn, gyn, *[qn[k] for k in sorted(qn)]) and tuple(g["shape"]) == shape
    assert np.array_equal(g["gy"], gyn) and ("h" not in g.files or np.array_equal(g["h"], hn))
    _, _, _, mine = case(shape)
    t = lambda k: torch.as_tensor(g[k])                                    # noqa: E731
    for n in BR.NAMES[1:]:
        assert _close(mine[n], t(n.replace(".", "_")).reshape(mine[n].shape)), n
    w1 = mine[BR.NAMES[0]][:, :, 0, 0]
    assert _close(w1[BR.W1_SUBSET], t("W1")) and _close(w1.sum(), t("W1_sum")) and _close(w1.norm(), t("W1_l2"))
    assert _close(mine["grad_h"][:, BR.GH_SUBSET], t("grad_h")) and _close(mine["grad_h"].norm(), t("grad_h_l2"))
    assert _close(mine["y"], t("y")) and int(g["nbt"]) == 1
    for i in (1, 2, 3):
        for k in ("mu%d", "var%d", "rm%d", "rv%d"):
            assert _close(mine[k % i], t(k % i)), k % i


@pytest.mark.parametrize("shape", BR.SHAPES, ids=BR.name)
def test_inputs_hit_both_clamps(shape):
    _, q, _, mine = case(shape)
    d = BR.apply(mine["u2"], BR.stats(mine["u2"], q["g2"], q["be2"]), BR.ACT_RELU6)[0]
    for what, t in (("e", mine["e"]), ("d", d)):
        lo, mid, hi = BR.clamp_shares(t)
        print("%s %s: %.1f %% at 0, %.1f %% inside, %.1f %% at 6" % (BR.name(shape), what, 100 * lo, 100 * mid, 100 * hi))
        assert lo >= 0.05 and hi >= 0.02 and mid >= 0.25
    for c in (8, 1536):
        x = BR.to64(BR.bn_inputs(c, shape))
        a = BR.apply(x["u"], BR.stats(x["u"], x["gamma"], x["beta"]), BR.ACT_RELU6)[0]
        lo, mid, hi = BR.clamp_shares(a[..., 1:])                           # (channel 0 is the constant zero-gamma channel)
        assert lo >= 0.05 and hi >= 0.05 and mid >= 0.25, (c, lo, mid, hi)


# ------------------------------------------------------------------------------------------------ wrong variants
def _ratio(wrong, right, bound):
    return float(((wrong - right).abs() / bound.clamp_min(1e-300)).max())


@pytest.mark.parametrize("shape", [(3, 5, 7), BR.SLAB_SHAPE], ids=BR.name)
@pytest.mark.parametrize("c", [8, 1536])
def test_wrong_kernels_lie_outside_the_bound(shape, c):
    """Each wrong kernel is at least 4 bounds of ITS stage's test from the right result on the teacher-forced inputs of the GPU
    tests, so that a kernel within 1 bound of the right result cannot be one of them.  (Dropping the last slab needs a shape
    with two: SLAB_SHAPE; at (3,5,7) the one slab is everything, which is 4 bounds away all the more.)"""
    x = BR.to64(BR.bn_inputs(c, shape))
    u, g = x["u"], x["g"]
    P = u.shape[0] * u.shape[1] * u.shape[2]
    f, fb = BR.stats(u, x["gamma"], x["beta"], bounds=True)
    for v in BR.WRONG_STATS:
        w = BR.stats(u, x["gamma"], x["beta"], variant=v)
        worst = max(_ratio(w[k], f[k], fb[k]) for k in ("mu", "var", "r", "s", "b"))
        print("%s C=%d stats %s: %.3g bounds" % (BR.name(shape), c, v, worst))
        assert worst >= 4.0, v
    # the running statistics: the test allows one ulp of fp32
    rm, rv = BR.running(x["rm"], x["rv"], f["mu"], f["var"], P)
    for v in BR.WRONG_RUNNING:
        wm, wv = BR.running(x["rm"], x["rv"], f["mu"], f["var"], P, variant=v)
        ulps = max(float(((wm - rm).abs() / (rm.abs() * 2 * BR.U).clamp_min(1e-300)).max()),
                   float(((wv - rv).abs() / (rv.abs() * 2 * BR.U).clamp_min(1e-300)).max()))
        print("%s C=%d running %s: %.3g ulps" % (BR.name(shape), c, v, ulps))
        assert ulps >= 4.0, v
    for act in (BR.ACT_RELU6, BR.ACT_SIGMOID, BR.ACT_NONE):
        S, _, sb = BR.bwd_sums(g, u, f, act, bounds=True)
        for v in BR.WRONG_SUMS:
            worst = _ratio(BR.bwd_sums(g, u, f, act, variant=v), S, sb)
            print("%s C=%d sums %s %s: %.3g bounds" % (BR.name(shape), c, act, v, worst))
            assert worst >= 4.0, (act, v)
        gu, gb = BR.bwd_apply(g, u, f, S, act, bounds=True)
        for v in BR.WRONG_BWD:
            worst = _ratio(BR.bwd_apply(g, u, f, S, act, variant=v), gu, gb)
            print("%s C=%d bwd_apply %s %s: %.3g bounds" % (BR.name(shape), c, act, v, worst))
            assert worst >= 4.0, (act, v)
    e = BR.apply(u, f, BR.ACT_RELU6)[0]
    W, wb = BR.dw_wgrad(g, e, bounds=True)
    worst = _ratio(BR.dw_wgrad(g, e, variant="across_frames"), W, wb)
    print("%s C=%d dw_wgrad across_frames: %.3g bounds" % (BR.name(shape), c, worst))
    assert worst >= 4.0


def test_wrong_decoders_lie_outside_the_goldens():
    """The same variants carried through the whole decoder move the gradients far outside what separates the closed form from
    the reference's recorded autograd (1e-11 relative)."""
    shape = BR.SHAPES[0]
    h, q, gy, right = case(shape)
    for kw in ([{"stats_variant": v} for v in BR.WRONG_STATS] + [{"bwd_variant": v} for v in BR.WRONG_BWD]
               + [{"dw_variant": "across_frames"}]):
        wrong = BR.decoder_train(q, h, gy, **kw)
        rel = max(float((wrong[n] - right[n]).abs().max() / right[n].abs().max()) for n in BR.NAMES + ("grad_h",))
        print("%s: relative distance %.3e" % (kw, rel))
        assert rel >= 1e-6, kw


# ------------------------------------------------------------------------------------------------ refusals and plumbing
def _block():
    from iip_uavsal_saliency_amd.model import dwBlock
    _, q, _ = BR.decoder_case((2, 5, 7))
    return BR.load_block(dwBlock(256, 1, kernel_size=3), q)


def test_python_entry_points_refuse_what_they_do_not_cover():
    blk = _block()
    t, g = torch.zeros(2, 256, 4, 4), torch.zeros(2, 1, 4, 4)
    for fn, args in ((train.decoder_forward_batch, (t,)), (train.decoder_backward_batch, (t, g))):
        with pytest.raises(RuntimeError, match="decoder_backward, decoder_input_grad and decoder_param_grads"):
            fn(blk.eval(), *args)                                          # eval mode: the message names the eval-mode functions
        with pytest.raises(RuntimeError, match="cuda"):
            fn(blk.train(), *args)
    with pytest.raises(RuntimeError, match="eval"):                        # the eval-mode functions keep their refusal
        train.decoder_backward(blk.train(), t, g)
    with pytest.raises(RuntimeError, match="cuda"):
        train.bn_stats(torch.zeros(2, 4, 4, 8), torch.ones(8), torch.zeros(8), 1e-5)
    with pytest.raises(RuntimeError, match="act must be"):
        train.bn._act("tanh")


class _Model:
    """what recurrence_step looks at before its first launch"""
    rnn_type, precision, training, num_cb = "twa", "f32", False, 0

    def __init__(self, decoder_training):
        self.conv_out_st = torch.nn.BatchNorm2d(1).train(decoder_training)
        self.called = False

    def __call__(self, *a, **k):
        self.called = True
        raise AssertionError("a launch")


def test_recurrence_step_refuses_before_any_launch():
    x = torch.zeros(2, 3, 8, 8)
    m = _Model(True)
    with pytest.raises(NotImplementedError, match="fuse"):
        train.recurrence_step(m, x, None, None, x, decoder=True, fuse=True, batch_stats=("decoder", "fuse"))
    with pytest.raises(RuntimeError, match="decoder=True"):
        train.recurrence_step(m, x, None, None, x, batch_stats=("decoder",))
    with pytest.raises(RuntimeError, match=r"conv_out_st\.train\(\)"):
        train.recurrence_step(_Model(False), x, None, None, x, decoder=True, batch_stats=("decoder",))
    m.training = True
    with pytest.raises(RuntimeError, match=r"model\.eval\(\)"):
        train.recurrence_step(m, x, None, None, x, decoder=True, batch_stats=("decoder",))
    m.training = False
    with pytest.raises(RuntimeError, match="cuda"):                        # everything the keyword asks is met: the CPU tensors stop it
        train.recurrence_step(m, x, None, None, x, decoder=True, batch_stats=("decoder",))
    assert not m.called


class _Stub:
    time_dims = 5

    def __init__(self):
        self.rnn, self.refreshed = object(), []
        self.conv_out_st = torch.nn.BatchNorm2d(1).eval()
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


def test_finetune_video_passes_batch_stats_and_restores_the_mode(monkeypatch):
    n = 30
    frames = torch.zeros(n, 3, 72, 128, dtype=torch.uint8)
    has = torch.ones(n, 2, dtype=torch.bool)
    fix = torch.zeros(n, 4, 4, dtype=torch.uint8)
    seen = []

    def step(model, x, cb, state, y, criterion, **kw):
        seen.append((kw, model.conv_out_st.training))
        return torch.tensor(1.0), None, [torch.tensor(0.0)]
    monkeypatch.setattr(train, "recurrence_step", step)

    def run(m, **kw):
        return stream.finetune_video(m, frames, torch.zeros(8, 9, 16), torch.zeros(20, 9, 16), fix, fix, _Opt(), batch_size=2,
                                     criterion=object(), prepare=lambda a, b, h, w, l: (torch.zeros(n, 2, h, w), has), **kw)
    m = _Stub()
    r = run(m, stages=("rnn", "decoder"), batch_stats=("decoder",))
    assert r["groups_run"] == 3 and seen == [({"decoder": True, "batch_stats": ("decoder",)}, True)] * 3
    assert not m.conv_out_st.training and m.refreshed == [(m.rnn, m.conv_out_st)] * 3
    m.conv_out_st.train()                                                  # a caller's own training mode is restored too
    run(m, stages=("rnn", "decoder"), batch_stats="decoder")
    assert m.conv_out_st.training
    del seen[:]
    m = _Stub()
    run(m, stages=("rnn", "decoder"))                                      # without the keyword: the call it always made
    assert seen == [({"decoder": True}, False)] * 3
    with pytest.raises(ValueError, match="'decoder' in stages"):
        run(_Stub(), stages=("rnn",), batch_stats=("decoder",))
    with pytest.raises(NotImplementedError, match="fuse"):
        run(_Stub(), stages=("rnn", "decoder", "fuse"), batch_stats=("decoder", "fuse"))

    def boom(model, x, cb, state, y, criterion, **kw):
        raise KeyError("stop")
    monkeypatch.setattr(train, "recurrence_step", boom)
    m = _Stub()
    with pytest.raises(KeyError):
        run(m, stages=("rnn", "decoder"), batch_stats=("decoder",))
    assert not m.conv_out_st.training                                      # restored when a step raises
