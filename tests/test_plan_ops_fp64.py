"""Every launch of the real forward plans against a float64 reference of that launch, teacher-forced.

For a plan built the way the model builds it (`model._engine`), the caller's tensors are bound (`Engine._bind_in_place`) and
the plan is walked op by op: the inputs an op reads are copied out (engine.read_view, float64), the op alone is launched
(`run_ops(i, i + 1)`), its outputs are read, and they are compared with a float64 reference of that op computed from the inputs
just read (tests/plan_ref64.py: references, and the per-element bound rtol * B + EPS * E + X + atol with its derivation).  Each
op is judged on the data it really received, so errors do not compound and the bounds are those of one launch.

Rules: every kind has a reference (only sync / poison / guard are skipped; an unknown kind fails), the number of ops checked is
asserted; the inputs of every op are finite (the headline configs run with `arena_debug`, where released arena ranges are
NaN-filled); in f16x3 plans every output split shadow equals its fp32 output and every GEMM that reads its A operand pre-split
passes from the merged shadow and from the fp32 values; in the headline f32 plan three deliberately wrong references (an input
channel dropped, the last input row zeroed, one output channel's bias left out) must be rejected on a fixed list of ops.
A Winograd triple (input transform, plane GEMM, output transform) is checked as one launch: its input and its output.

`test_dispatch_cover` walks the configurations of `plan_census.WALKS` the same way: together with the cases above they reach every
dispatch signature (kernel instance x edge path, tests/plan_census.py) of the model sizes in `plan_census.DOMAIN`; the first op of
every signature that no earlier walk visits carries the wrong references too.

`test_saturated_relu6_walk` walks two small plans whose BatchNorms saturate the ReLU6 behind them (tests/saturate_bn.py): every op
with a ReLU6 stage holds the share condition of tests/act_ref64.py in its reference and rejects the reference without the
upper clamps (`mut="no_hi"`).
"""
import time

import pytest
import torch

import act_ref64 as A
import plan_census as PC
import plan_ref64 as R
from iip_uavsal_saliency_amd import engine as E
from iip_uavsal_saliency_amd import synth

pytestmark = pytest.mark.gpu

SKIP = ("sync", "poison", "guard")
IMG_BUDGET = 96 << 20           # float64 elements of one operand above which an op is checked on a sample of its images

# headline f32 plan: ops and the wrong references each must reject (a: channel, b: last row, c: bias)
MUTATIONS = {
    "features.0": ("chan", "row", "bias"),            # stem
    "features.1": ("chan", "row", "bias"),            # fused_ir (small-channel kernel)
    "features.9": ("chan", "row", "bias"),            # fused_ir (mid-channel kernel)
    "features.14.pw": ("chan", "bias"),               # conv1, K = 96
    "features.14.dw": ("chan", "row", "bias"),        # dw, stride 2
    "aspp.dw": ("chan", "row", "bias"),               # dw, dilation groups
    "aspp.pl": ("chan", "bias"),                      # conv1, n_group, K = 1920
    "st0.sub.dwpl": ("chan", "row", "bias"),          # conv1 with the fused depthwise loader, K = 384
    "st0.tdiff": ("chan",),
    "ctx.sum": ("chan",),
    "up_c5": ("chan",),                               # bilinear
    "twa.step3.xout": ("chan", "row"),                # Winograd F(2x2) triple, ConvTWA epilogue, K = 2304 (no bias)
    "twa.wx.xout": ("chan", "row"),                   # Winograd F(4x4) triple, K = 2304 (no bias)
    "conv_last.xout": ("chan", "row", "bias"),        # Winograd F(4x4) triple, BN + ReLU6, K = 4032
    "conv_out_st.dwpl": ("chan", "row", "bias"),      # dw_dot + sigmoid
}


def _images(d, n=None):
    n = d.n if n is None else n
    if n * d.h * d.w * max(d.c, 1) <= IMG_BUDGET or n <= 3:
        return list(range(n))
    return sorted({0, n // 2, n - 1})


def _ratio(err, bnd):
    """Worst err / bound (an exact element counts 0 whatever its bound; a non-finite output counts inf)."""
    if not err.numel():
        return 0.0
    r = torch.where(err == 0, torch.zeros_like(err), err / bnd)
    return torch.nan_to_num(r, nan=float("inf"), posinf=float("inf")).max().item()


def _rd(eng, d, images=None, shadow=False):
    return E.read_view(eng, d, shadow=shadow, images=images, device="cuda")


def relu6_kind(rec):
    """The kind under which the saturated walk counts an op with a ReLU6 stage ("" if it has none)."""
    k = rec["kind"]
    if "triple" in rec:                             # a part of a Winograd triple: counted with the triple's last op
        return ""
    if k in ("dw", "dw_dot", "fused_ir", "stem"):
        return k
    if k in ("conv1", "conv3"):
        if rec.get("dw") is not None:
            return k + "/fused-dw"
        return k if rec["epi"] == R.EPI_AFFINE and rec["act"] == R.ACT_RELU6 else ""
    if k == "wino":
        return "wino" if rec["twa"] is None and rec["act"] == R.ACT_RELU6 else ""
    return ""


class Walk:
    def __init__(self, eng, tag, mutations=None, saturated=False):
        self.eng, self.tag, self.mutations = eng, tag, mutations or {}
        self.sat = {} if saturated else None        # kind -> [ops with a ReLU6 stage checked, smallest `no_hi` err / bound]
        self.worst = {}                 # kind -> worst err / bound
        self.step_cmp = {}              # recurrence step -> (max |err|, worst err / the direct-f32 bound of that step)
        self.checked = 0
        self.mut_results = {}
        self.shadow_out = self.shadow_in = 0
        self.sampled = []               # ops checked on a sample of their images

    def _imgs(self, name, d, n=None):
        imgs = _images(d, n)
        if len(imgs) < (d.n if n is None else n):
            self.sampled.append(name)
        return imgs

    def _finite(self, name, *ts):
        for t in ts:
            if t is not None:
                assert bool(torch.isfinite(t).all()), "%s %s: an input is not finite (released or unwritten range)" % (self.tag, name)

    def _judge(self, name, kind, got, ref: R.Ref, extra=None, key=None):
        bnd = R.bound(ref)
        if extra is not None:
            bnd = bnd + extra
        err = (got - ref.y).abs()
        ratio = _ratio(err, bnd)
        self.worst[key or kind] = max(self.worst.get(key or kind, 0.0), ratio)
        assert ratio <= 1.0, "%s %s (%s): error %.3g x its bound (max err %.3g)" % (self.tag, name, kind, ratio, err.max().item())
        return bnd

    def _step_cmp(self, name, got, ref):
        err = (got - ref.y).abs()
        self.step_cmp[name] = (err.max().item(), _ratio(err, R.bound(ref)))

    def _mutants(self, name, got, bnd, fn):
        for m in self.mutations.get(name, ()):
            ref_m = fn(m)
            ratio = _ratio((got - ref_m.y).abs(), bnd)
            self.mut_results[(name, m)] = ratio
            assert ratio > 1.0, "%s %s: the wrong reference '%s' passes (%.3g x the bound): the bound is too loose" % (
                self.tag, name, m, ratio)

    def _clamps(self, name, kind, got, bnd, fn):
        """Saturated walk, an op with a ReLU6 stage: the share condition (tests/act_ref64.py) holds on the float64
        pre-activations of every such stage of its reference, and the reference without the upper clamps is rejected.
        `fn(mut, pre)` -> Ref."""
        if self.sat is None:
            return
        pre = []
        fn(None, pre)
        assert pre, "%s %s: no ReLU6 stage in the reference" % (self.tag, name)
        for k, v in enumerate(pre):
            assert A.share_ok(v), "%s %s (%s) ReLU6 stage %d: (n, <= 0, >= 6, inside) = %s" % (self.tag, name, kind, k, A.shares(v))
        ratio = _ratio((got - fn("no_hi", None).y).abs(), bnd)
        n, least = self.sat.get(kind, (0, float("inf")))
        self.sat[kind] = (n + 1, min(least, ratio))
        assert ratio > 1.0, "%s %s (%s): the reference without the upper clamp passes (%.3g x the bound)" % (self.tag, name, kind, ratio)

    def _check_out_shadow(self, name, od, got, images):
        if od.sp is None or od.buf is None:
            return
        merged = _rd(self.eng, od, images, shadow=True)
        lim = R.SHADOW_REL * got.abs() + R.SHADOW_ABS
        assert bool(((merged - got).abs() <= lim).all()), "%s %s: split shadow differs from the fp32 output" % (self.tag, name)
        self.shadow_out += 1

    def run(self):
        eng = self.eng
        n_ops = len(eng.ops_meta)
        assert len(eng.op_args) == n_ops == int(eng.lib.uavsal_plan_size(eng.plan))
        expect = sum(1 for r in eng.op_args if r["kind"] not in SKIP)
        i = 0
        while i < n_ops:
            rec = eng.op_args[i]
            kind = rec["kind"]
            if kind in SKIP:
                eng.run_ops(i, i + 1)
                i += 1
                continue
            last = i
            if "triple" in rec:            # a Winograd triple: judged from its input to its output
                last = eng._op_idx[rec["triple"]]
                rec = eng.op_args[last]
                assert rec["kind"] == "wino" and all("triple" in eng.op_args[j] or eng.op_args[j]["kind"] == "poison"
                                                     for j in range(i, last))
            fn = getattr(self, "op_" + rec["kind"], None)
            if fn is None:
                raise AssertionError("%s: op %d %s has kind %r, which this test has no reference for" % (
                    self.tag, i, rec["name"], rec["kind"]))
            fn(i, last, rec)
            self.checked += sum(1 for j in range(i, last + 1) if eng.op_args[j]["kind"] not in SKIP)
            i = last + 1
        torch.cuda.synchronize()
        assert self.checked == expect and self.checked == sum(1 for m in eng.ops_meta if m["kind"] not in SKIP)
        return self

    def launch(self, i, last):
        self.eng.run_ops(i, last + 1)
        torch.cuda.synchronize()

    def summary(self):
        return "[plan-ops-fp64] %s: %d ops checked; worst err/bound %s" % (
            self.tag, self.checked, ", ".join("%s %.3f" % kv for kv in sorted(self.worst.items())))

    # ---------------------------------------------------------------------------------------------- one method per kind
    def op_conv1(self, i, last, rec):
        eng, name = self.eng, rec["name"]
        ad, od = rec["a"], rec["out"]
        imgs = self._imgs(name, od if rec.get("dw") is None else ad)
        a_fp = _rd(eng, ad, imgs) if ad.buf is not None else None
        a_sh = _rd(eng, ad, imgs, shadow=True) if rec.get("split_in") else None
        res = _rd(eng, rec["res"], imgs) if rec["res"] is not None else None
        aux = _rd(eng, rec["aux"], imgs) if rec["aux"] is not None else None
        self._finite(name, a_fp, a_sh, res, aux)
        self.launch(i, last)
        got = _rd(eng, od, imgs)
        if rec["epi"] == R.EPI_LSTM:
            got = torch.cat([got, _rd(eng, rec["out2"], imgs)], 1)
        inputs = [x for x in (a_sh, a_fp) if x is not None]
        bnd = None
        for a in inputs:                       # the shadow the kernel read, and the fp32 values it was split from
            ref = R.ref_conv(rec, a, res=res, aux=aux)
            b_ = self._judge(name, rec["kind"], got, ref, key=rec["kind"] + ("/split" if rec.get("split_in") else ""))
            bnd = b_ if bnd is None else bnd
        if rec.get("split_in"):
            self.shadow_in += 1
        if rec["epi"] == R.EPI_TWA:
            self._step_cmp(name, got, R.ref_conv(dict(rec, prec="f32"), inputs[-1], res=res, aux=aux))
        self._check_out_shadow(name, od, got if rec["epi"] != R.EPI_LSTM else None, imgs)
        self._mutants(name, got, bnd, lambda m: R.ref_conv(rec, inputs[0], res=res, aux=aux, mut=m))
        if relu6_kind(rec):
            self._clamps(name, relu6_kind(rec), got, bnd, lambda m, pre: R.ref_conv(rec, inputs[0], res=res, aux=aux, mut=m, pre=pre))

    op_conv3 = op_conv1

    def op_wino(self, i, last, rec):
        eng, name = self.eng, rec["name"]
        od = rec["out"]
        imgs = self._imgs(name, od)
        if rec["segs"]:
            parts = []
            for sg in rec["segs"]:
                x = _rd(eng, sg, imgs)
                if (sg.h, sg.w) != (od.h, od.w):
                    x = R.bilinear_ac(x, od.h, od.w)[0]
                parts.append(x)
            a = torch.cat(parts, 1)
        else:
            a = _rd(eng, rec["a"], imgs)
        twa = None if rec["twa"] is None else tuple(_rd(eng, t, imgs) for t in rec["twa"])
        self._finite(name, a, *(twa or ()))
        self.launch(i, last)
        got = _rd(eng, od, imgs)
        ref = R.ref_wino(rec, a, twa)
        bnd = self._judge(name, "wino%d%s" % (rec["r"], "/twa" if twa else ""), got, ref)
        if twa is not None:                    # the same step judged by the direct fp32 convolution's bound
            w = R._w(rec["conv"], a.device, rec.get("wslice"))
            d = R.twa_update(torch.nn.functional.conv2d(a, w, padding=1), torch.nn.functional.conv2d(a.abs(), w.abs(), padding=1),
                             twa[1], twa[0], a, R.rtol("f32", 9 * w.shape[1]))
            self._step_cmp(name, got, d)
        self._mutants(name, got, bnd, lambda m: R.ref_wino(rec, a, twa, mut=m))
        if relu6_kind(rec):
            self._clamps(name, relu6_kind(rec), got, bnd, lambda m, pre: R.ref_wino(rec, a, twa, mut=m, pre=pre))

    def op_dw(self, i, last, rec):
        eng, name = self.eng, rec["name"]
        ad, od = rec["a"], rec["out"]
        imgs = self._imgs(name, ad)
        a = _rd(eng, ad, imgs)
        self._finite(name, a)
        self.launch(i, last)
        ref = R.ref_dw(rec, a)
        if od.buf is None:                     # written only as a split shadow
            got = _rd(eng, od, imgs, shadow=True)
            bnd = self._judge(name, "dw/shadow-out", got, ref, extra=R.SHADOW_REL * ref.y.abs() + R.SHADOW_ABS)
            self.shadow_out += 1
        else:
            got = _rd(eng, od, imgs)
            bnd = self._judge(name, "dw", got, ref)
        self._mutants(name, got, bnd, lambda m: R.ref_dw(rec, a, mut=m))
        self._clamps(name, "dw", got, bnd, lambda m, pre: R.ref_dw(rec, a, mut=m, pre=pre))

    def op_dw_dot(self, i, last, rec):
        eng, name = self.eng, rec["name"]
        imgs = self._imgs(name, rec["a"])
        a = _rd(eng, rec["a"], imgs)
        self._finite(name, a)
        self.launch(i, last)
        got = _rd(eng, rec["out"], imgs)
        bnd = self._judge(name, "dw_dot", got, R.ref_dw_dot(rec, a))
        self._mutants(name, got, bnd, lambda m: R.ref_dw_dot(rec, a, mut=m))
        self._clamps(name, "dw_dot", got, bnd, lambda m, pre: R.ref_dw_dot(rec, a, mut=m, pre=pre))

    def op_fused_ir(self, i, last, rec):
        eng, name = self.eng, rec["name"]
        imgs = self._imgs(name, rec["a"])
        a = _rd(eng, rec["a"], imgs)
        self._finite(name, a)
        self.launch(i, last)
        got = _rd(eng, rec["out"], imgs)
        bnd = self._judge(name, "fused_ir", got, R.ref_fused_ir(rec, a))
        self._mutants(name, got, bnd, lambda m: R.ref_fused_ir(rec, a, mut=m))
        self._clamps(name, "fused_ir", got, bnd, lambda m, pre: R.ref_fused_ir(rec, a, mut=m, pre=pre))

    def op_stem(self, i, last, rec):
        eng, name = self.eng, rec["name"]
        imgs = self._imgs(name, rec["out"])
        x = _rd(eng, rec["a"], imgs)
        self._finite(name, x)
        self.launch(i, last)
        got = _rd(eng, rec["out"], imgs)
        bnd = self._judge(name, "stem/u8" if rec["u8"] else "stem", got, R.ref_stem(rec, x))
        self._mutants(name, got, bnd, lambda m: R.ref_stem(rec, x, mut=m))
        self._clamps(name, "stem", got, bnd, lambda m, pre: R.ref_stem(rec, x, mut=m, pre=pre))

    def op_bilinear(self, i, last, rec):
        eng, name = self.eng, rec["name"]
        od = rec["out"]
        imgs = self._imgs(name, od)
        x = _rd(eng, rec["a"])
        self._finite(name, x)
        self.launch(i, last)
        got = _rd(eng, od, imgs)
        ref = R.ref_bilinear(rec, x, (od.h, od.w), imgs)
        bnd = self._judge(name, "bilinear", got, ref)
        self._check_out_shadow(name, od, got, imgs)
        self._mutants(name, got, bnd, lambda m: R.ref_bilinear(rec, x, (od.h, od.w), imgs, mut=m))

    def op_tdiff(self, i, last, rec):
        eng, name = self.eng, rec["name"]
        x = _rd(eng, rec["a"])
        self._finite(name, x)
        self.launch(i, last)
        got = _rd(eng, rec["out"])
        bnd = self._judge(name, "tdiff", got, R.ref_tdiff(x, rec["seq_len"]))
        self._mutants(name, got, bnd, lambda m: R.ref_tdiff(x, rec["seq_len"], mut=m))

    def op_tsum(self, i, last, rec):
        eng, name = self.eng, rec["name"]
        od, T = rec["out"], rec["T"]
        groups = self._imgs(name, od)
        x = _rd(eng, rec["a"], [g * T + t for g in groups for t in range(T)])
        self._finite(name, x)
        self.launch(i, last)
        got = _rd(eng, od, groups)
        bnd = self._judge(name, "tsum", got, R.ref_tsum(x, T))
        self._mutants(name, got, bnd, lambda m: R.ref_tsum(x, T, mut=m))

    def _bitwise(self, i, last, rec, kind):
        eng, name = self.eng, rec["name"]
        x = _rd(eng, rec["a"])
        self._finite(name, x)
        self.launch(i, last)
        got = _rd(eng, rec["out"])
        assert torch.equal(got, x), "%s %s: %s is not an exact copy" % (self.tag, name, kind)
        if rec.get("cpad"):
            raise AssertionError("layout with channel padding: not recorded by the engine")
        self.worst[kind] = max(self.worst.get(kind, 0.0), 0.0)

    def op_layout(self, i, last, rec):
        self._bitwise(i, last, rec, "layout")

    def op_copy(self, i, last, rec):
        self._bitwise(i, last, rec, "copy")


# ------------------------------------------------------------------------------------------------------------- configs
def _inputs(N, H, W, seed=0, u8=False, t0=0):
    h, w = (E._down(E._down(E._down(n))) for n in (H, W))      # the engine's 1/8-scale map (sizes that are no multiple of 8 round up)
    f = synth.synth_frames_u8(N, H, W, seed, t0)
    x = torch.from_numpy(f if u8 else synth.normalize_frames(f)).cuda()
    cb0 = torch.from_numpy(synth.gauss_priors(N, h, w)).cuda()
    cb1 = torch.from_numpy(synth.ob_priors(N, h, w, seed=seed)).cuda()
    return x, cb0, cb1


def _model(T, **kw):
    from iip_uavsal_saliency_amd.model import UAVSal, UAVSAL_LSTM
    cls = UAVSAL_LSTM if kw.pop("lstm", False) else UAVSal
    m = cls(time_dims=T, **({"bias_type": kw.pop("bias_type")} if "bias_type" in kw else {}))
    synth.load_synth_weights(m, 0)
    m = m.cuda().eval()
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def _engine(m, C, T, H, W, prec, static=False, u8=False):
    m.precision = prec
    dev = torch.device("cuda", torch.cuda.current_device())
    return m._engine(dev, C, T, H, W, "tile" if C == 1 else "clip", in_dtype=torch.uint8 if u8 else torch.float32,
                     static_priors=static)


def _walk(m, C, T, H, W, prec, tag, static=False, u8=False, calls=1, mutations=None, rand_state=False, saturated=False):
    """`mutations`: {op name: wrong references}, or a function of the engine that returns it; `rand_state`: the call starts from
    a non-zero recurrent state (with the zero state the first step's h operand is all zeros, and so is any mutation of it)."""
    eng = _engine(m, C, T, H, W, prec, static, u8)
    lstm = getattr(m, "rnn_type", "twa") == "lstm"
    state = cstate = None
    if rand_state:
        state = (0.5 * torch.rand((C, 256, eng.h, eng.w), generator=torch.Generator().manual_seed(1))).cuda()
    if callable(mutations):
        mutations = mutations(eng)
    x, cb0, cb1 = _inputs(C * T, H, W, 0, u8)
    for call in range(calls - 1):                          # earlier calls run whole; the last is walked
        eng.run(x, cb0, cb1, state, cstate=cstate)
        torch.cuda.synchronize()
        if eng.persistent:
            state, cstate = eng.h_view, eng.c_view
        x, cb0, cb1 = _inputs(C * T, H, W, 0, u8, t0=(call + 1) * T)
    eng._bind_in_place(x, cb0, cb1, state, cstate, lstm)
    t0 = time.perf_counter()
    w = Walk(eng, tag, mutations, saturated).run()
    print(w.summary() + " (%.1f s)" % (time.perf_counter() - t0))
    return w


@pytest.fixture(scope="module", autouse=True)
def _fp64_on_device():
    """The float64 references run on the GPU: torch's float64 conv / matmul are checked there against the CPU first."""
    g = torch.Generator().manual_seed(0)
    x, w = torch.randn(2, 8, 9, 11, dtype=torch.float64, generator=g), torch.randn(6, 8, 3, 3, dtype=torch.float64, generator=g)
    cpu = torch.nn.functional.conv2d(x, w, padding=1)
    gpu = torch.nn.functional.conv2d(x.cuda(), w.cuda(), padding=1).cpu()
    assert (gpu - cpu).abs().max().item() <= 1e-12 * cpu.abs().max().item()
    yield


def test_headline_f32_with_sensitivity():
    """A: 360x640, 1 clip x 8 frames, exact fp32 (the benchmark's workload), released arena ranges NaN-filled, and the
    deliberately wrong references rejected."""
    m = _model(8, arena_debug=True)
    w = _walk(m, 1, 8, 360, 640, "f32", "A f32", mutations=MUTATIONS)
    missing = [nm for nm in MUTATIONS if nm not in w.eng._op_idx]
    assert not missing, missing
    kinds = {w.eng.op_args[w.eng._op_idx[nm]]["kind"] for nm in MUTATIONS}
    plan_kinds = {r["kind"] for r in w.eng.op_args if r["kind"] not in SKIP + ("layout", "copy") and "triple" not in r}
    assert kinds >= plan_kinds, plan_kinds - kinds      # at least one op of every numeric kind of the plan
    assert len(w.mut_results) == sum(len(v) for v in MUTATIONS.values())
    print("[plan-ops-fp64] A f32 sensitivity: %d wrong references rejected, smallest err/bound %.3g (%s %s)" % (
        len(w.mut_results), min(w.mut_results.values()), *min(w.mut_results, key=w.mut_results.get)))


@pytest.mark.parametrize("prec", ["f16x3", "bf16x3"])
def test_headline_split_precisions(prec):
    """A: the same plan shape in the split 16-bit precisions (bf16x3: regression bound)."""
    m = _model(8, arena_debug=True)
    _walk(m, 1, 8, 360, 640, prec, "A " + prec)


def test_headline_static_priors():
    """A': the frame-invariant-priors plan (prior nets on one frame, broadcast)."""
    m = _model(8)
    _walk(m, 1, 8, 360, 640, "f32", "A' f32 static", static=True)


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_eight_clips(prec):
    """B: 360x640, 8 clips x 8 frames -- F(4x4) recurrence steps on tile 11, ST lanes, prior nets forked at features.5."""
    m = _model(8)
    _walk(m, 8, 8, 360, 640, prec, "B " + prec)


def test_f16x3_step_forms_via_model_winograd():
    """B / f16x3: the recurrence step as fp32 Winograd F(4x4) (default) and as the direct split-fp16 step
    (`model.winograd = False`); both within their bounds, and their accuracy in units of B reported."""
    rel = {}
    for form, flag in (("wino F(4x4)", 1), ("direct f16x3", 0)):
        m = _model(8, winograd=bool(flag))
        w = _walk(m, 8, 8, 360, 640, "f16x3", "B f16x3 steps=" + form)
        steps = {k.split(".xout")[0]: v for k, v in w.step_cmp.items()}
        assert sorted(steps) == ["twa.step%d" % t for t in range(8)], sorted(steps)
        kinds = {w.eng.op_args[w.eng._op_idx[k + (".xout" if flag else "")]]["kind"] for k in steps}
        assert kinds == ({"wino"} if flag else {"conv3"}), kinds
        rel[form] = (max(v[0] for v in steps.values()), max(v[1] for v in steps.values()))
    print("[plan-ops-fp64] B f16x3 twa.step0-7, max |err| and worst err / (direct fp32 bound): %s" % ", ".join(
        "%s %.3g, %.3g" % (k, *v) for k, v in rel.items()))


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_ragged_small_maps(prec):
    """C: 72x104, 1 x 3 -- 9x13 feature maps (f32 with uint8 frames: the stem's normalising path)."""
    m = _model(3)
    _walk(m, 1, 3, 72, 104, prec, "C " + prec, u8=prec == "f32")


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_saturated_relu6_walk(prec):
    """C and D's sizes (72x104 1 x 3, 96x160 1 x 4) with BatchNorms that saturate the ReLU6 behind them (tests/saturate_bn.py):
    every op with a ReLU6 stage keeps its bound, has both clamps populated in its reference's pre-activations, and rejects the
    reference whose ReLU6 stages lack the upper clamp."""
    import saturate_bn
    for T, H, W in ((3, 72, 104), (4, 96, 160)):
        m = _model(T)
        assert saturate_bn.saturate_relu6_bn(m) > 0
        w = _walk(m, 1, T, H, W, prec, "saturated %dx%d %s" % (H, W, prec), saturated=True)
        present = {relu6_kind(r) for r in w.eng.op_args if r["kind"] not in SKIP} - {""}
        assert present >= {"conv1", "dw", "dw_dot", "fused_ir", "stem"} and present & {"wino", "conv3"}, present
        assert set(w.sat) == present and all(n > 0 for n, _ in w.sat.values()), (w.sat, present)
        print("[plan-ops-fp64] saturated %dx%d %s: ops with a ReLU6 stage and smallest no_hi err/bound: %s" % (
            H, W, prec, ", ".join("%s %d %.3g" % (k, n, r) for k, (n, r) in sorted(w.sat.items()))))


def test_persistent_state_second_call():
    """D: 96x160, 4 clips x 5 frames, resident state, the second call walked (reads the carried state, copies it back)."""
    m = _model(5, persistent_state=True)
    w = _walk(m, 4, 5, 96, 160, "f32", "D f32 persistent", calls=2)
    assert any(r["kind"] == "copy" for r in w.eng.op_args)


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
@pytest.mark.parametrize("variant", ["lstm", "bias101", "bias000"])
def test_lstm_and_prior_subsets(variant, prec):
    """E: 96x160, 4 frames -- the ConvLSTM epilogue with gate-interleaved weights, and plans without some prior nets."""
    kw = {"lstm": dict(lstm=True), "bias101": dict(bias_type=[1, 0, 1]), "bias000": dict(bias_type=[0, 0, 0])}[variant]
    m = _model(4, **kw)
    _walk(m, 1, 4, 96, 160, prec, "E %s %s" % (variant, prec))


def test_big_maps():
    """F: 720x1280, 4 clips x 16 frames (row-class depthwise, big maps; ops checked on a sample of their images)."""
    m = _model(16)
    _walk(m, 4, 16, 720, 1280, "f32", "F f32")


# ------------------------------------------------------------------------------------------------ the dispatch-signature cover
SPATIAL = ("conv3", "wino", "dw", "dw_dot", "fused_ir", "stem")          # kinds whose output pixel reads a 3x3 neighbourhood
HAS_BIAS = ("dw", "dw_dot", "fused_ir", "stem")                          # kinds that always end in a folded BatchNorm


def _wrong_refs_for(rec):
    """The wrong references an op carries: always `chan`; `row` when the kind has spatial support; `bias` when it has a bias.
    (layout / copy are compared bit for bit: any wrong reference is rejected by construction, none is tried.)"""
    k = rec["kind"]
    if k in ("layout", "copy"):
        return ()
    muts = ["chan"]
    if k in SPATIAL or (k == "conv1" and rec.get("dw") is not None):
        muts.append("row")
    if k in HAS_BIAS or (k in ("conv1", "conv3", "wino") and rec.get("bn") is not None):
        muts.append("bias")
    return tuple(muts)


def _cover_mutations(eng, dev_sigs, new):
    """{op name: wrong references} for the first op of every signature in `new` (a part of a Winograd triple: the triple)."""
    by_op, seen = {}, set()
    for i, name, sig in dev_sigs:
        if sig not in new or sig in seen:
            continue
        seen.add(sig)
        key = eng.op_args[i].get("triple", name)
        by_op[key] = _wrong_refs_for(eng.op_args[eng._op_idx[key]])
    assert seen == set(new), set(new) - seen
    return by_op


@pytest.mark.parametrize("cfg", PC.WALKS, ids=lambda c: "%dx%d-%dx%d-%s" % c[:5])
def test_dispatch_cover(cfg):
    """One entry of `plan_census.WALKS`: the plan walked like every other; the engine built on the device has every dispatch
    signature the CPU census recorded for this configuration; the first op of every signature that neither the cases above nor
    an earlier entry visits rejects its wrong references; ops are checked on a sample of their images only where the census
    says so (an operand above IMG_BUDGET: tests/test_plan_census_cpu.py holds which entries may have such ops)."""
    C, T, H, W, prec, variant = cfg
    assert variant == "" and PC.IMG_BUDGET == IMG_BUDGET
    cpu, new = PC.config_signatures(cfg), PC.new_signatures(cfg)
    assert new, "%s reaches nothing new" % (cfg,)
    got = {}

    def mutations(eng):
        dev = PC.plan_signatures(eng)
        missing = cpu - {s for _, _, s in dev}
        assert not missing, "the plan built on the device lacks signatures the CPU census recorded: %s" % sorted(missing, key=str)
        got.update(_cover_mutations(eng, dev, new))
        return got

    tag = "cover %dx%d %dx%d %s" % (H, W, C, T, prec)
    w = _walk(_model(T), C, T, H, W, prec, tag, mutations=mutations, rand_state=True)
    expect = sum(len(v) for v in got.values())
    assert len(w.mut_results) == expect and all(r > 1.0 for r in w.mut_results.values())
    assert sorted(w.sampled) == sorted(PC.config_sampled(cfg)), (w.sampled, PC.config_sampled(cfg))
    exact = sum(1 for v in got.values() if not v)
    print("[plan-ops-fp64] %s: %d new signatures on %d ops (%d of them bit-exact copies); %d wrong references rejected%s; "
          "%d ops sampled%s" % (tag, len(new), len(got), exact, len(w.mut_results),
                                 ", smallest err/bound %.3g (%s %s)" % (min(w.mut_results.values()), *min(w.mut_results, key=w.mut_results.get))
                                 if w.mut_results else "", len(w.sampled), " (%s ...)" % ", ".join(w.sampled[:3]) if w.sampled else ""))
