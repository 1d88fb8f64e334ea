"""Both clamps of every ReLU6 site of the kernels on the MI355X, on the saturating cases of tests/act_ref64.py (recipe, share
condition, float64 references, bounds and wrong references are described there; tests/test_act_clamps_cpu.py checks the cases
themselves without a device).  For every launch:

  (a) |got - ref| <= bound element-wise (plan_ref64.bound of the chain at the launch's precision);
  (b) every wrong reference of the op (`no_hi@S`, `no_lo@S` per ReLU6 stage S, `res_inside`) is more than 1 bound away at
      some element;
  (c) where the float64 pre-activation of a final ReLU6 is >= 6 + bound the output is float32(6) exactly (with a residual:
      float32(6) + res, rounded once), where it is <= -bound the output is 0 (or res; the sign of zero is not checked); a
      split shadow of such an output merges to exactly 6 and 0.

The last test prints the worst error / bound and the smallest rejection ratio per family.
"""
import collections

import pytest
import torch

import act_ref64 as A
import plan_ref64 as R

pytestmark = pytest.mark.gpu

LAUNCHES = A.launches()
WORST = collections.defaultdict(float)                       # family -> worst err / bound
REJECT = {}                                                  # family -> (smallest rejection ratio, launch, wrong reference)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from iip_uavsal_saliency_amd import ops as o
    return o


def nhwc(t):
    return None if t is None else t.permute(0, 2, 3, 1).contiguous().cuda()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous().cpu()


def _ratio(err, bnd):
    r = torch.where(err == 0, torch.zeros_like(err), err / bnd)
    return torch.nan_to_num(r, nan=float("inf"), posinf=float("inf")).max().item()


def _sliced(n, h, w, pitch, off, cout, fill):
    buf = torch.full((n, h, w, pitch), fill, device="cuda")
    return buf, buf[..., off:off + cout]


def _untouched(buf, off, cout, fill):
    return bool((buf[..., :off] == fill).all()) and bool((buf[..., off + cout:] == fill).all())


def _run(ops, lch, p):
    """-> (output NCHW fp32 on the host, merged split shadow or None, True if the output IS the merged shadow)."""
    from iip_uavsal_saliency_amd import _lib as L
    I, kw = p.inputs, lch.kw
    shadow = None
    if lch.op == "conv":
        x, res = nhwc(I["x"]), nhwc(I.get("res"))
        n, h, w, _ = x.shape
        cout = I["w"].shape[0]
        buf = out = None
        if kw.get("out_slice"):                              # a channel slice of a buffer whose pitch is no multiple of 4
            buf, out = _sliced(n, h, w, kw["out_slice"][0], kw["out_slice"][1], cout, -7.0)
        rt = {}
        got = ops.conv_gemm(x, I["w"], I["s"], I["b"], act=L.ACT_RELU6, res=res, out=out, prec=lch.prec, tile=kw.get("tile", 0),
                            stream_k=kw.get("stream_k", False), split_in=kw.get("split_in", False),
                            split_out=kw.get("split_out", False), n_group=kw.get("n_group", 0), route=rt)
        if kw.get("split_out"):
            got, sp = got
            shadow = nchw(ops.merge_shadow(sp))
        assert A.route_matches(rt, lch.route), (lch, rt)
        if buf is not None:
            assert _untouched(buf, kw["out_slice"][1], cout, -7.0), lch
        return nchw(got), shadow, False
    if lch.op == "dwgemm":
        stride, act = lch.key[6], lch.key[7]
        e, res = nhwc(I["e"]), I["res"]
        n, cout = e.shape[0], I["wp"].shape[0]
        ho, wo = (e.shape[1] - 1) // stride + 1, (e.shape[2] - 1) // stride + 1
        pad = 8 if kw.get("sliced") else 0                   # the output (and residual) are channel slices of wider buffers
        buf, out = _sliced(n, ho, wo, cout + 2 * pad, pad, cout, 7.0)
        rd = None
        if res is not None:
            rbuf = torch.zeros((n, ho, wo, cout + 2 * pad), device="cuda")
            rbuf[..., pad:pad + cout] = nhwc(res)
            rd = rbuf[..., pad:pad + cout]
        rt = {}
        got = ops.conv_gemm(e, I["wp"], I["sp"], I["bp"], act=act, res=rd, out=out, prec=lch.prec,
                            dw=(I["wd"], I["sd"], I["bd"], stride), route=rt)
        assert A.route_matches(rt, lch.route), (lch, rt)
        assert _untouched(buf, pad, cout, 7.0), lch
        return nchw(got.contiguous()), None, False
    if lch.op == "wino":
        if "xs" in I:
            got = ops.conv3x3_winograd([nhwc(t) for t in I["xs"]], I["w"], I["s"], I["b"], act=L.ACT_RELU6, r=kw["r"], size=I["size"])
        else:
            got = ops.conv3x3_winograd(nhwc(I["x"]), I["w"], I["s"], I["b"], act=L.ACT_RELU6, res=nhwc(I.get("res")), r=kw["r"])
        return nchw(got), None, False
    if lch.op == "dw":
        stride, dil = lch.key[5], lch.key[6]
        groups = list(dil) if isinstance(dil, tuple) else None
        got = ops.dw3x3(nhwc(I["x"]), I["w"], I["s"], I["b"], stride=stride, dilation=1 if groups else dil, dil_groups=groups,
                        split_out=kw.get("split_out", False))
        if kw.get("split_out"):
            return nchw(ops.merge_shadow(got)), None, True
        return nchw(got), None, False
    if lch.op == "dwdot":
        args = (nhwc(I["x"]), I["wd"], I["sd"], I["bd"], I["w2"], I["s2"], I["b2"])
        got, again = ops.dw3x3_dot(*args, act=I["act"]), ops.dw3x3_dot(*args, act=I["act"])
        assert torch.equal(got, again), lch                  # fixed summation order
        return nchw(got), None, False
    if lch.op == "stem":
        return nchw(ops.stem_conv(I["x"].cuda(), I["w"], I["s"], I["b"])), None, False
    if lch.op == "fused":
        stride, use_res = lch.key[7], lch.key[8]
        got = ops.fused_ir(nhwc(I["x"]), I["w1"], I["b1"], I["wd"], I["bd"], I["w2"], I["b2"], stride=stride, residual=use_res,
                           tile=kw.get("tile", 0))
        return nchw(got), None, False
    raise AssertionError("no runner for %r" % (lch.op,))


def _exact(lch, got32, p, bnd, what):
    """(c): the elements whose pre-activation is beyond a clamp by more than the bound."""
    pre = p.pres()["out"]
    six = torch.full(got32.shape, 6.0, dtype=torch.float32)
    zero = torch.zeros(got32.shape, dtype=torch.float32)
    if p.out_res is not None and what == "output":
        res32 = p.inputs["res"].float()
        six, zero = six + res32, zero + res32                # one fp32 rounding, as the epilogue adds it
    hi, lo = pre >= 6.0 + bnd, pre <= -bnd
    assert int(hi.sum()) > 0 and int(lo.sum()) > 0, (lch, what)
    assert bool((got32[hi] == six[hi]).all()), "%s: %s is not exactly 6%s where the pre-activation is beyond 6 + bound (%d of %d)" % (
        lch, what, " + res" if p.out_res is not None and what == "output" else "", int((got32[hi] != six[hi]).sum()), int(hi.sum()))
    assert bool((got32[lo] == zero[lo]).all()), "%s: %s is not exactly 0%s where the pre-activation is below -bound (%d of %d)" % (
        lch, what, " + res" if p.out_res is not None and what == "output" else "", int((got32[lo] != zero[lo]).sum()), int(lo.sum()))
    return int(hi.sum()), int(lo.sum())


@pytest.mark.parametrize("lch", LAUNCHES, ids=repr)
def test_both_clamps(ops, lch):
    p = A.problem(lch.key)
    r = lch.kw.get("r") if lch.op == "wino" else None
    ref = p.ref(lch.prec, r)
    bnd = R.bound(ref)
    got32, shadow, is_shadow = _run(ops, lch, p)
    got = got32.double()
    assert tuple(got.shape) == tuple(ref.y.shape), (lch, got.shape, ref.y.shape)
    if is_shadow:                                            # written only as a split shadow: its own two roundings
        bnd = bnd + R.SHADOW_REL * ref.y.abs() + R.SHADOW_ABS
    ratio = _ratio((got - ref.y).abs(), bnd)
    rej = {wr: _ratio((got - p.y(wr)).abs(), bnd) for wr in p.wrongs}
    exact = None
    print("[act-clamps] %s: err/bound %.3f (max err %.3g); wrong references %s" % (
        lch, ratio, (got - ref.y).abs().max().item(), ", ".join("%s %.3g" % kv for kv in rej.items())))
    WORST[lch.family] = max(WORST[lch.family], ratio)
    for wr, v in rej.items():
        if lch.family not in REJECT or v < REJECT[lch.family][0]:
            REJECT[lch.family] = (v, lch.id, wr)
    assert ratio <= 1.0, "%s: error %.3g x its bound" % (lch, ratio)                                            # (a)
    for wr, v in rej.items():                                                                                    # (b)
        assert v > 1.0, "%s: the wrong reference '%s' passes (%.3g x the bound)" % (lch, wr, v)
    if "out" in p.stages:                                                                                        # (c)
        if is_shadow:
            exact = _exact(lch, got32, p, bnd, "the merged shadow")
        else:
            exact = _exact(lch, got32, p, bnd, "output")
        if shadow is not None:
            lim = R.SHADOW_REL * got.abs() + R.SHADOW_ABS
            assert bool(((shadow.double() - got).abs() <= lim).all()), "%s: split shadow differs from the fp32 output" % (lch,)
            if p.out_res is None:
                _exact(lch, shadow, p, bnd, "the merged shadow")
    if lch.family == "conv/streamk":                         # (the one large problem: not kept)
        A.forget(lch.key)
    assert exact is not None or "out" not in p.stages


def test_report():
    """Worst error / bound and smallest rejection ratio per family (what DESIGN.md quotes); every family was run."""
    fams = sorted({l.family for l in LAUNCHES})
    if not WORST:                                            # (run on its own: nothing to report)
        return
    for f in fams:
        print("[act-clamps] family %-14s worst err/bound %.3f; smallest rejection %.3g (%s %s)" % ((f, WORST[f]) + REJECT[f]))
    assert sorted(WORST) == fams
