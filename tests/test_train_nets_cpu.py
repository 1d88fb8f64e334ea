"""Fine-tuning the gauss / ob prior nets without a GPU: the C ABI of csrc/train_nets.hip, the float64 restatements of
tests/nets_ref64.py against torch autograd and against the reference's recorded results (tests/golden/nets_train_*.npz), the
summed one-frame form of static priors against the per-frame form, what the Python entry points and the driver refuse, the
GEMM routes the new calls send, the prior record under `refresh_weights`, and the conditions under which the GPU tests are
meaningful: each wrong variant lies at least 4 bounds from the right result in the float64 reference alone."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import _lib, stream, train
from iip_uavsal_saliency_amd import packing as P

import block_ref64 as BR
import mp_ref64 as MP
import nets_ref64 as NR


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
    for n in ("uavsal_ir_narrow_grads", "uavsal_ir_narrow_finish", "uavsal_ir_narrow_slabs", "uavsal_ir_narrow_slab_rows",
              "uavsal_ir_narrow_workspace_bytes", "uavsal_frame_sum", "uavsal_nets_sizeof_desc"):
        assert n in names and hasattr(lib, n) and n + "(" in hdr
    assert _lib.NETS_DESC_TYPES == [_lib.IrNarrowDesc, _lib.IrNarrowFinishDesc, _lib.FrameSumDesc]
    for i, t in enumerate(_lib.NETS_DESC_TYPES):
        assert lib.uavsal_nets_sizeof_desc(i) == C.sizeof(t)
    assert lib.uavsal_nets_sizeof_desc(3) < 0 and lib.uavsal_nets_sizeof_desc(-1) < 0
    assert lib.uavsal_mp_sizeof_desc(1) < 0 and lib.uavsal_abi_version() == 20                # the older lists stay closed
    assert len(_lib.DESC_TYPES) == 20 and lib.uavsal_sizeof_desc(20) < 0
    assert _lib.NARROW_CHUNK == NR.CHUNK == 32 and "#define UAVSAL_NARROW_CHUNK 32" in hdr
    for n in ("narrow_block_param_grads", "ir_narrow_grads", "frame_sum", "prior_nets", "prior_net_backward"):
        assert callable(getattr(train, n))
    assert train.PRIOR_NETS == tuple(NR.NETS) and train.BLOCK_PARAMS == NR.NAMES


def test_slab_count_is_the_restated_partition(lib):
    d = _lib.IrNarrowDesc()
    d.Co = 64
    for cin, hid, _ in NR.NARROW.values():
        for (n, H, W) in NR.PICTURES + [(20, 45, 80), (8, 45, 80), (300, 4, 4), (1, 7, 300), (2000, 5, 300)]:
            d.n_img, d.H, d.W, d.Cin, d.Ch = n, H, W, cin, hid
            sr, slabs = NR.slab_partition(n, H, W)
            assert lib.uavsal_ir_narrow_slab_rows(C.byref(d)) == sr and lib.uavsal_ir_narrow_slabs(C.byref(d)) == slabs, (n, H, W)
            assert lib.uavsal_ir_narrow_workspace_bytes(C.byref(d)) == slabs * NR.slab_doubles(cin, hid) * 8
            assert slabs <= 256 and sr * slabs >= n * H > sr * (slabs - 1)
    # (1,45,80) is the first of the test pictures with more than one slab; (3,45,80) ends in a partial slab of 3 rows; in both
    # (2,9,13) and (3,45,80) a slab holds rows of two images
    assert [NR.slab_partition(*s) for s in NR.PICTURES] == [(256, 1), (37, 1), (20, 1), (4, 12), (4, 34)]
    assert 3 * 45 - 33 * 4 == 3 and 45 % 4 != 0
    assert NR.slab_partition(2000, 5, 300) == (40, 250)                                      # the cap on the slab count
    for cin, hid, co in ((8, 132, 64), (36, 48, 64), (8, 46, 64), (6, 48, 64), (8, 48, 32), (8, 48, 128)):
        d.Cin, d.Ch, d.Co = cin, hid, co
        assert lib.uavsal_ir_narrow_slabs(C.byref(d)) == 0 and lib.uavsal_ir_narrow_workspace_bytes(C.byref(d)) == 0


def test_argument_validation_without_gpu(lib):
    s = _lib.IrNarrowDesc()
    assert lib.uavsal_ir_narrow_grads(C.byref(s), None) == -1
    s.x = s.e = s.d = s.gd = s.ga = s.go = s.ws = 256
    s.n_img, s.H, s.W, s.Cin, s.Ch, s.Co, s.ldgo = 1, 5, 7, 8, 132, 64, 64
    assert lib.uavsal_ir_narrow_grads(C.byref(s), None) == -3             # Ch > 128: UAVSAL_ESHAPE
    s.Ch = 46
    assert lib.uavsal_ir_narrow_grads(C.byref(s), None) == -3             # Ch % 4
    s.Ch, s.Cin = 48, 64
    assert lib.uavsal_ir_narrow_grads(C.byref(s), None) == -3             # Cin > 32
    s.Cin, s.Co = 8, 128
    assert lib.uavsal_ir_narrow_grads(C.byref(s), None) == -3             # Co != 64
    s.Co, s.ldgo = 64, 66
    assert lib.uavsal_ir_narrow_grads(C.byref(s), None) == -2             # UAVSAL_EALIGN
    s.ldgo = 32
    assert lib.uavsal_ir_narrow_grads(C.byref(s), None) == -1             # rows shorter than Co
    s.ldgo = 192
    assert lib.uavsal_ir_narrow_grads(C.byref(s), None) == -1             # accepted so far: the workspace is too small
    s.ws_bytes = lib.uavsal_ir_narrow_workspace_bytes(C.byref(s))
    s.e = 260
    assert lib.uavsal_ir_narrow_grads(C.byref(s), None) == -2
    f = _lib.IrNarrowFinishDesc()
    assert lib.uavsal_ir_narrow_finish(C.byref(f), None) == -1
    for n, _ in _lib.IrNarrowFinishDesc._fields_[:23]:
        if n != "ws_bytes":
            setattr(f, n, 256)
    f.Cin, f.Ch, f.Co, f.slabs = 8, 48, 64, 2
    assert lib.uavsal_ir_narrow_finish(C.byref(f), None) == -1            # the workspace is too small for two slabs
    f.ws_bytes = 2 * NR.slab_doubles(8, 48) * 8
    f.Ch = 192
    assert lib.uavsal_ir_narrow_finish(C.byref(f), None) == -3
    f.Ch, f.g_w1 = 48, 258
    assert lib.uavsal_ir_narrow_finish(C.byref(f), None) == -2
    q = _lib.FrameSumDesc()
    assert lib.uavsal_frame_sum(C.byref(q), None) == -1
    q.a = q.out = 256
    q.N, q.HW, q.C, q.lda, q.ldo = 2, 35, 64, 192, 64
    q.C = 62
    assert lib.uavsal_frame_sum(C.byref(q), None) == -2
    q.C, q.lda = 64, 32
    assert lib.uavsal_frame_sum(C.byref(q), None) == -1
    q.lda, q.N = 192, 0
    assert lib.uavsal_frame_sum(C.byref(q), None) == -1


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", ["gauss0", "ob0"])
def test_narrow_closed_form_is_autograd_of_the_dwblock(name):
    """dwBlock(8, 64) and dwBlock(20, 64): the closed form against torch autograd through the restated forward AND through the
    package's own module tree (eval mode) in float64."""
    from iip_uavsal_saliency_amd.model import dwBlock
    shape = (2, 5, 7)
    x, q, go = NR.narrow_case(name, shape)
    got = NR.param_grads(BR.fold(BR.to64(q)), t64(x), t64(go))
    want = MP.autograd_grads(BR.to64(q), t64(x), t64(go), 1, False)
    for n in NR.NAMES:
        _close(got[n], want[n])
    blk = NR.make_block(NR.NARROW[name], q, dwBlock).double()
    assert (blk.cin, blk.hidden, blk.cout) == NR.NARROW[name] and not blk.use_res_connect
    seq = blk.conv                                                        # (the package's modules hold parameters only)
    bn = lambda t, b: torch.nn.functional.batch_norm(t, b.running_mean, b.running_var, b.weight, b.bias, False, 0.0, b.eps)      # noqa: E731
    e = bn(torch.nn.functional.conv2d(t64(x), seq[0][0].weight), seq[0][1]).clamp(0, 6)
    d = bn(torch.nn.functional.conv2d(e, seq[1][0].weight, padding=1, groups=blk.hidden), seq[1][1]).clamp(0, 6)
    o = bn(torch.nn.functional.conv2d(d, seq[2].weight), seq[3])
    params = dict(blk.named_parameters())
    gs = torch.autograd.grad(o, [params[n] for n in NR.NAMES], t64(go))
    for n, g in zip(NR.NAMES, gs):
        _close(got[n], g)


@pytest.mark.parametrize("net", list(NR.NETS))
def test_net_closed_form_is_autograd(net):
    cb, qs, go = NR.net_case(net, (2, 5, 7))
    Q = [BR.to64(q) for q in qs]
    got = NR.net_param_grads([BR.fold(q) for q in Q], t64(cb), t64(go))
    want = NR.net_autograd(Q, t64(cb), t64(go))
    for k in ("0", "1"):
        for n in NR.NAMES:
            _close(got[k][n], want[k][n])


def test_frame_sum_restated():
    a = t64(np.random.RandomState(3).standard_normal((5, 3, 4, 8)).astype(np.float32))
    s, b = NR.frame_sum_ref(a)
    assert s.shape == (1, 3, 4, 8) and torch.equal(NR.frame_sum_ref(a[:1])[0], a[:1]) and bool((b > 0).all())
    assert float(((a[:-1].sum(0, keepdim=True) - s).abs() / b).min()) >= 4.0                  # one frame short is far outside


@pytest.mark.parametrize("bias", NR.GOLDEN_BIAS, ids=str)
def test_closed_form_matches_the_reference_autograd(bias, golden_dir):
    """tests/golden/nets_train_*.npz: the reference's own dwBlock through model.py:346-365 under autograd
    (tools/make_nets_goldens.py), the margin of tests/test_train_ctx_cpu.py's goldens."""
    g = np.load(os.path.join(golden_dir, NR.golden_name(bias) + ".npz"))
    assert int(g["T"]) == NR.GOLDEN_T and tuple(g["shape"]) == NR.GOLDEN_SHAPE

    def close(a, b):
        assert a.shape == b.shape and float(np.abs(a - b).max()) <= 1e-10 * float(np.abs(b).max())
    for mode in NR.GOLDEN_MODES:
        Q, st, _, go, nets = NR.golden_case(bias, mode)
        assert str(g[mode + "_digest"]) == NR.golden_digest(Q, st, go, nets) and len(nets) == bias[0] + bias[1]
        g_cb, grads = NR.golden_ref(bias, mode)
        g_cb = g_cb[:, :64 * len(nets)].numpy()
        close(g_cb[NR.G_SUBSET], g[mode + "_g_cb"])
        close(g_cb.sum((0, 2, 3)), g[mode + "_g_cb_sum"])
        for net, (cb, qs) in nets.items():
            tag = NR.NETS[net][:-1]
            assert np.array_equal(cb, g[tag + "_cb"] if mode == "frame" else np.repeat(g[tag + "_cb"][:1], cb.shape[0], 0))
            for i in (0, 1):
                pre = "%s_%s%d" % (mode, tag, i)
                for n in NR.NAMES:
                    key = "%s_%s" % (pre, n.replace(".", "_"))
                    mine = grads[net][str(i)][n].numpy()
                    if n in NR.golden_subset_names(i):
                        w = mine[:, :, 0, 0]
                        close(w[NR.W_SUBSET], g[key])
                        l2 = float(g[key + "_l2"])
                        assert abs(float(w.sum()) - float(g[key + "_sum"])) <= 1e-10 * l2 * np.sqrt(w.size)
                        assert abs(float(np.sqrt((w * w).sum())) - l2) <= 1e-10 * l2
                    else:
                        close(mine, g[key])


@pytest.mark.parametrize("bias", NR.GOLDEN_BIAS, ids=str)
def test_one_repeated_prior_summed_then_one_frame_is_the_per_frame_form(bias):
    """What train.recurrence_step does with static priors -- the net's slice of g_cb summed over the N frames, the backward on
    ONE frame -- is the gradient of the N-copies form the reference computes (every block of a net is per-pixel arithmetic on
    its own frame): equal in float64 to rounding.  With N DIFFERENT prior frames it is not."""
    _, per_frame = NR.golden_ref(bias, "repeat")
    _, summed = NR.golden_ref(bias, "repeat", summed=True)
    for net in per_frame:
        for k in ("0", "1"):
            for n in NR.NAMES:
                _close(summed[net][k][n], per_frame[net][k][n], rel=1e-12)
    Q, st, _, go, nets = NR.golden_case(bias, "frame")
    g_cb, right = NR.golden_ref(bias, "frame")
    for i, (net, (cb, qs)) in enumerate(nets.items()):
        P = [BR.fold(BR.to64(q)) for q in qs]
        wrong = NR.net_param_grads(P, t64(cb)[:1], g_cb[:, 64 * i:64 * i + 64].sum(0, keepdim=True))
        x0, g0 = NR.net_inputs(P, t64(cb), g_cb[:, 64 * i:64 * i + 64])["0"]
        _, b = NR.param_grads(P[0], x0, g0, bounds=True)
        for n in (NR.NAMES[0], NR.NAMES[3]):
            assert float(((wrong["0"][n] - right[net]["0"][n]).abs() / b[n].clamp_min(1e-300)).max()) >= 4.0, (net, n)


# ------------------------------------------------------------------------------------------------ sensitivity
@pytest.mark.parametrize("shape", [s for s in NR.PICTURES if s[1] * s[2] <= 9 * 13], ids=str)
@pytest.mark.parametrize("name", list(NR.NARROW))
def test_wrong_variants_lie_outside_the_bounds(name, shape):
    """Every wrong variant the GPU test must reject is at least 4 bounds from the right result in its worst element of the
    tensors it changes, in float64 alone -- where it computes something else at all (`variant_applies`)."""
    x, q, go = NR.narrow_case(name, shape)
    p = BR.fold(BR.to64(q))
    g, b = NR.param_grads(p, t64(x), t64(go), bounds=True)
    touched = {"no_mask": (3, 4, 5), "gd_no_border": (3, 4), "gd_image_seam": (3, 4), "stop_at_64": (0, 1, 2, 3, 4, 5, 6, 7),
               "stop_at_16": (0, 1, 2, 3, 4, 5, 6, 7), "gamma_scaled": (1, 4, 7)}
    for v in NR.WRONG:
        wrong = NR.param_grads(p, t64(x), t64(go), variant=v)
        far = {i: float(((wrong[NR.NAMES[i]] - g[NR.NAMES[i]]).abs() / b[NR.NAMES[i]].clamp_min(1e-300)).max()) for i in range(9)}
        for i in range(9):
            if i not in touched[v]:
                assert far[i] == 0.0, (v, i)
        if NR.variant_applies(v, NR.NARROW[name], shape):
            assert max(far[i] for i in touched[v]) >= 4.0, (v, far)
            if v in ("no_mask", "gamma_scaled") or shape[1] >= 5:
                assert all(far[i] >= 4.0 for i in touched[v] if not (v.startswith("stop") and i in (7,))), (v, far)
        else:
            assert max(far.values()) == 0.0 or v == "no_mask", v
    met = {v for v in NR.WRONG for nm in NR.NARROW for s in NR.PICTURES if NR.variant_applies(v, NR.NARROW[nm], s)}
    assert met == set(NR.WRONG)


def test_cases_hold_both_clamps_and_zero_gamma_channels():
    import saturate_bn
    for name in ("gauss0", "ob0"):
        x, q, go = NR.narrow_case(name, (2, 9, 13))
        parts = {}
        NR.param_grads(BR.fold(BR.to64(q)), t64(x), t64(go), parts=parts)
        for k in ("e", "d"):
            lo, mid, hi = BR.class_shares(parts[k])
            assert lo >= 0.05 and mid >= 0.25 and hi >= 0.03, (name, k, lo, mid, hi)
        x, q, go = NR.narrow_case(name, (2, 9, 13), gain=saturate_bn.GAIN, shift=saturate_bn.SHIFT)
        parts = {}
        NR.param_grads(BR.fold(BR.to64(q)), t64(x), t64(go), parts=parts)
        for k in ("e", "d"):
            lo, mid, hi = BR.class_shares(parts[k])
            assert hi >= 0.3 and mid >= 0.05, (name, k, lo, mid, hi)
        x, q, go = NR.narrow_case(name, (2, 9, 13), zero_gamma=True)
        p = BR.fold(BR.to64(q))
        g = NR.param_grads(p, t64(x), t64(go))
        assert float(p["s1"][NR.ZERO[0]]) == 0.0 and float(p["s2"][NR.ZERO[1]]) == 0.0
        assert float(g[NR.NAMES[1]][NR.ZERO[0]].abs()) > 0 and float(g[NR.NAMES[4]][NR.ZERO[1]].abs()) > 0


# ------------------------------------------------------------------------------------------------ refusals
def test_python_entry_points_refuse_what_they_do_not_cover():
    from iip_uavsal_saliency_amd import UAVSal
    from iip_uavsal_saliency_amd.model import dwBlock
    for name in ("gauss0", "ob0", "tiny"):
        blk = NR.make_block(NR.NARROW[name], NR.narrow_case(name, (1, 3, 5))[1], dwBlock)
        assert len(train._narrow_parts(blk)) == 6
        with pytest.raises(RuntimeError, match="Cin"):                    # the wide path keeps its refusal, and its message
            train._param_grad_parts(blk)
        with pytest.raises(RuntimeError, match="block_backward needs"):
            train._block_parts(blk)
    x8, g64 = torch.zeros(2, 8, 5, 7), torch.zeros(2, 64, 5, 7)
    blk = dwBlock(8, 64, kernel_size=3).eval()
    with pytest.raises(RuntimeError, match="cuda"):                       # the shape is taken: the tensors are not
        train.narrow_block_param_grads(blk, x8, None, None, g64)
    with pytest.raises(RuntimeError, match="eval"):
        train.narrow_block_param_grads(dwBlock(8, 64, kernel_size=3).train(), x8, None, None, g64)
    for bad in (dwBlock(8, 64, kernel_size=3, expand_ratio=1), dwBlock(8, 64, kernel_size=3, dilation=6), dwBlock(8, 64, kernel_size=3, stride=2),
                dwBlock(64, 64, kernel_size=3), dwBlock(8, 32, kernel_size=3), dwBlock(8, 128, kernel_size=3), dwBlock(6, 64, kernel_size=3),
                dwBlock(24, 64, kernel_size=3)):
        with pytest.raises(RuntimeError, match="narrow_block_param_grads (takes|needs)"):
            train.narrow_block_param_grads(bad.eval(), x8, None, None, g64)
    res = dwBlock(64, 64, kernel_size=3, expand_ratio=1.5).eval()         # 64 -> 96 -> 64: inside the widths but for Cin, residual
    with pytest.raises(RuntimeError, match="narrow_block_param_grads"):
        train.narrow_block_param_grads(res, x8, None, None, g64)
    with pytest.raises(RuntimeError, match="cuda|NHWC"):
        train.frame_sum(torch.zeros(2, 5, 7, 64))
    with pytest.raises(RuntimeError, match="cuda"):
        train.ir_narrow_grads(*(torch.zeros(1, 3, 3, 8),) * 5, torch.zeros(1, 3, 3, 64))
    m = UAVSal(time_dims=2).eval()
    assert list(train.prior_nets(m)) == ["gauss_cb_layer", "ob_cb_layer"]
    assert list(train.prior_nets(m).values()) == [m.gauss_cb_layer, m.ob_cb_layer]
    assert list(train.prior_nets(UAVSal(time_dims=2, bias_type=[0, 1, 1]))) == ["ob_cb_layer"]
    assert list(train.prior_nets(UAVSal(time_dims=2, bias_type=[1, 0, 0]))) == ["gauss_cb_layer"]
    m001, m000 = UAVSal(time_dims=2, bias_type=[0, 0, 1]).eval(), UAVSal(time_dims=2, bias_type=[0, 0, 0]).eval()
    assert train.prior_nets(m001) == {} and train.prior_nets(m000) == {}
    cb, go = torch.zeros(2, 8, 5, 7), torch.zeros(2, 5, 7, 64)
    with pytest.raises(RuntimeError, match="cuda"):
        train.prior_net_backward(m.gauss_cb_layer, cb, go)
    with pytest.raises(RuntimeError, match="eval"):
        train.prior_net_backward(UAVSal(time_dims=2).train().gauss_cb_layer, cb, go)
    with pytest.raises(RuntimeError, match="prior_net_backward takes"):
        train.prior_net_backward(m.fucb_layer, cb, go)
    with pytest.raises(RuntimeError, match="narrow_block_param_grads"):
        train.prior_net_backward(m.cxt_cb_prior, cb, go)
    fu = torch.zeros(4, 320, 5, 7)
    # the step: nets needs fuse and a prior NET; it needs neither fust nor ctx
    for model, kw in ((m, dict(nets=True)), (m, dict(decoder=True, nets=True)), (m001, dict(fuse=True, nets=True)),
                      (m001, dict(fuse=True, ctx=True, nets=True)), (m000, dict(fuse=True, nets=True))):
        with pytest.raises(RuntimeError, match="nets=True needs fuse=True and a model with the gauss or the ob prior"):
            train.recurrence_step(model, fu, None, None, fu, **kw)
    with pytest.raises(RuntimeError, match="eval"):
        train.recurrence_step(UAVSal(time_dims=2).train(), fu, None, None, fu, fuse=True, nets=True)
    with pytest.raises(RuntimeError, match="cuda"):
        train.recurrence_step(m, fu, None, None, fu, fuse=True, nets=True)
    # the walk hands out g_cb on request only: the default call returns what it returned
    import inspect
    sig = inspect.signature(train.prior_path_backward)
    assert sig.parameters["need_cb_grad"].default is False and sig.parameters["need_fust_grad"].default is True
    assert inspect.signature(train.recurrence_step).parameters["nets"].default is False


def test_stages_of_the_driver():
    for stages in (("rnn", "nets"), ("rnn", "decoder", "nets"), ("rnn", "fuse", "nets", "ctx"), ("rnn", "fuse", "nets", "fust"),
                   ("rnn", "fuse", "nets", "nets"), ("rnn", "nets", "fuse"), ("nets",), ("fuse", "nets"), ("rnn", "fust", "nets"),
                   ("rnn", "ctx", "nets"),
                   # ... and every tuple that raised before this stage existed
                   ("rnn", "ctx"), ("rnn", "decoder", "ctx"), ("rnn", "fuse", "ctx", "fust"), ("rnn", "fuse", "ctx", "ctx"),
                   ("rnn", "ctx", "fuse"), ("ctx",), ("fuse", "ctx"), ("rnn", "fust", "ctx")):
        with pytest.raises(ValueError, match="stages"):
            stream.finetune_video(None, None, None, None, None, None, None, stages=stages)


class _Stub:
    time_dims = 5

    def __init__(self, bias):
        for n in ("rnn", "conv_out_st", "fucbst_layer", "fust_layer", "fucb_layer", "cxt_cb_prior", "gauss_cb_layer", "ob_cb_layer"):
            setattr(self, n, object())
        self.use_gauss_prior, self.use_ob_prior, self.use_context_prior = bias
        self.num_cb, self.refreshed = sum(bias), []
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


def test_finetune_video_with_the_nets_stage(monkeypatch):
    n = 20
    frames = torch.zeros(n, 3, 72, 128, dtype=torch.uint8)
    has = torch.ones(n, 2, dtype=torch.bool)
    seen = []

    def step(model, x, cb, state, y, criterion, **kw):
        seen.append(kw)
        return torch.tensor(1.0), None, [torch.tensor(0.0)]
    monkeypatch.setattr(train, "recurrence_step", step)
    fix = torch.zeros(n, 4, 4, dtype=torch.uint8)
    for stages in (("rnn", "decoder", "fuse", "fust", "ctx", "nets"), ("rnn", "fuse", "nets"), ("rnn", "fuse", "fust", "nets"),
                   ("rnn", "decoder", "fuse", "ctx", "nets")):
        for bias in ((1, 1, 1), (1, 1, 0), (1, 0, 0), (0, 1, 1)):
            m = _Stub(bias)
            del seen[:]
            r = stream.finetune_video(m, frames, torch.zeros(8, 9, 16), torch.zeros(20, 9, 16), fix, fix, _Opt(), batch_size=2,
                                      criterion=object(), prepare=lambda a, b, h, w, l: (torch.zeros(n, 2, h, w), has), stages=stages)
            assert r["groups_run"] == 2 and seen == [{s: True for s in stages[1:]}] * 2
            want = (m.rnn,) + ((m.conv_out_st,) if "decoder" in stages else ()) + (m.fucbst_layer,)
            want += ((m.fust_layer,) if "fust" in stages else ())
            want += ((m.fucb_layer,) + ((m.cxt_cb_prior,) if bias[2] else ())) if "ctx" in stages else ()
            want += ((m.gauss_cb_layer,) if bias[0] else ()) + ((m.ob_cb_layer,) if bias[1] else ())      # "nets" comes last of all
            assert m.refreshed == [want] * 2


# ------------------------------------------------------------------------------------------------ routes
def test_every_gemm_of_a_trained_net_has_a_route(lib):
    """The 1x1 GEMMs the walk of a net sends -- the forward's own expand (8 -> 48, 20 -> 120) and projection (48 -> 64, 120 ->
    64), block 0's gd GEMM with the transposed projection (64 -> 48, 64 -> 120), and block 1's three (64 <-> 384) -- at one
    45 x 80 frame (static priors) and at 8 and 20 of them: none is folded into csrc/train_nets.hip."""
    sent = {(8, 48), (48, 64), (64, 48), (20, 120), (120, 64), (64, 120), (64, 384), (384, 64)}
    for (ci, co) in sorted(sent):
        for (n, h, w) in ((1, 45, 80), (8, 45, 80), (20, 45, 80), (4, 9, 13), (1, 5, 7), (1, 1, 1)):
            d = _lib.ConvDesc()
            d.a, d.lda, d.a_img_stride = 1 << 20, ci, h * w
            d.out, d.ldc, d.o_img_stride = 1 << 21, co, h * w
            d.n_img, d.H, d.W, d.Cin, d.Cout, d.taps = n, h, w, ci, co, 1
            d.prec, d.act, d.epi, d.tile = _lib.PREC["f32"], _lib.ACT_NONE, _lib.EPI_AFFINE, 0
            d.w = 1 << 20
            rt = _lib.conv_route(lib, d)
            layout = P.conv_weight_layout("f32", False, False, rt.tile, 1)
            assert P.pack_conv_weight(torch.zeros(co, ci, 1, 1), layout).numel() >= ci * co, (ci, co, rt)
    k = _lib.IrBwdDesc()                                                   # uavsal_ir_bwd takes C % 4: 48 and 120
    k.gd = k.d = k.e = k.wd9 = k.s2 = k.ga = 256
    k.n_img, k.H, k.W = 1, 0, 7
    for c in (48, 120):
        k.C = c
        assert lib.uavsal_ir_bwd(C.byref(k), None) == -1                  # (H = 0 is what it objects to, not C)
    k.C = 46
    k.H = 5
    assert lib.uavsal_ir_bwd(C.byref(k), None) == -2


# ------------------------------------------------------------------------------------------------ refresh and the prior cache
class _Eng:
    def __init__(self):
        self.dropped = 0

    def drop_prior_record(self):
        self.dropped += 1


def _packed_model(bias=(1, 1, 1)):
    """a model whose weights count as packed (nothing is on a device: the store is empty) with stub engines, and a stream
    replica with one of its own"""
    from iip_uavsal_saliency_amd import UAVSal
    m = UAVSal(time_dims=2, bias_type=list(bias)).eval()
    m._check_weights()
    m._wshared = {"cpu": {}}
    r = m.replica()
    m._engines["a"], m._engines["b"], r._engines = _Eng(), _Eng(), {"c": _Eng()}
    m._stream_replicas = [r]
    return m, [m._engines["a"], m._engines["b"], r._engines["c"]]


def test_refresh_of_a_prior_net_drops_the_prior_record_and_other_modules_do_not():
    m, engs = _packed_model()
    with torch.no_grad():
        m.rnn.cell_list[0].rnn_conv.weight.mul_(1.0)
    m.refresh_weights(m.rnn)
    assert [e.dropped for e in engs] == [0, 0, 0] and m._wversion == m._weights_version()
    for i, mods in enumerate(((m.fucb_layer, m.cxt_cb_prior), (m.fucbst_layer, m.fust_layer, m.conv_out_st))):
        m.refresh_weights(*mods)
        assert [e.dropped for e in engs] == [0, 0, 0]
    with torch.no_grad():
        m.gauss_cb_layer[0].conv[0][0].weight.mul_(1.0)
    m.refresh_weights(m.rnn, m.gauss_cb_layer)
    assert [e.dropped for e in engs] == [1, 1, 1]                         # every engine of the model and of its stream replicas
    m.refresh_weights(m.ob_cb_layer[1])                                   # a block inside a net
    assert [e.dropped for e in engs] == [2, 2, 2]
    m.refresh_weights(m.ob_cb_layer[0].conv[1][1])                        # a BatchNorm inside a net
    assert [e.dropped for e in engs] == [3, 3, 3]
    assert m._wversion == m._weights_version() and set(m._engines) == {"a", "b"}      # no plan was dropped
    # a model without prior nets has nothing to drop
    m2, engs2 = _packed_model((0, 0, 1))
    m2.refresh_weights(m2.fucb_layer, m2.cxt_cb_prior)
    assert [e.dropped for e in engs2] == [0, 0, 0]


def test_every_packed_form_of_a_net_is_refreshable_in_both_plans(lib):
    """The kinds the forward packs for the four blocks -- static plan (one 45 x 80 frame: block 1 is a natural-layout fused_mid
    entry) and per-frame plan (expand GEMM + depthwise / projection) -- and the kinds the backward adds are all kinds
    `WeightCache.refresh` remakes in place; none is a transposed fused_ir entry."""
    import mock_plan
    from iip_uavsal_saliency_amd import UAVSal
    from iip_uavsal_saliency_amd.weights import WeightCache, _REFRESH_IDS
    m = UAVSal(time_dims=4).eval()
    for static in (True, False):
        store = {}
        eng, mock = mock_plan.record(m, n_seq=1, seq_len=8, H=360, W=640, ctx_T=4, ctx_mode="tile", precision="f32", taps=True,
                                     in_dtype=torch.float32, use_graph=False, fuse_dw=None, use_lanes=True, stream_k=True,
                                     persistent=False, wcache=store, static_priors=static)
        ids = {id(s): s for net in train.prior_nets(m).values() for s in net.modules()}
        kinds = {}
        for key in store:
            if isinstance(key, tuple) and any(isinstance(i, int) and i in ids for i in key[1:]):
                kinds.setdefault(key[0], []).append(key)
        assert kinds and set(kinds) <= {"w", "bn", "dw", "fused"}, sorted(kinds)
        assert all(k in _REFRESH_IDS for k in kinds)
        assert all(key[2] for key in kinds.get("fused", []))              # natural layout only
        if static:
            assert len(kinds.get("fused", [])) == 2                       # block 1 of either net on one frame
        cache = WeightCache("cpu", store)
        n = cache.refresh(ids, dry=True)
        assert n == sum(len(v) for v in kinds.values())
        with torch.no_grad():
            for net in train.prior_nets(m).values():
                for q in net.parameters():
                    q.mul_(1.5)
        assert cache.refresh(ids) == n
        for key in kinds.get("fused", []):
            blk = next(b for net in train.prior_nets(m).values() for b in net if id(b.conv[1][0]) == key[1])
            assert torch.equal(store[key]["w1"], blk.conv[0][0].weight.detach().reshape(blk.hidden, blk.cin))
        with torch.no_grad():
            for net in train.prior_nets(m).values():
                for q in net.parameters():
                    q.div_(1.5)
    # what the backward packs on top: transposed-and-scaled weights and BatchNorm statistics
    assert {"wTs", "bnstat", "wT"} <= set(_REFRESH_IDS)
