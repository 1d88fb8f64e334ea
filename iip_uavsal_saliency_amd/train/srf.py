"""The head of the backbone `model.sfnet` (without its MobileNetV2 `features`), the eighth stage: everything in it the
reference initialises itself (`srf_head`, `srf_head_backward`; csrc/train_srf.hip).  Its 1x1 stages go through `cbr_backward`,
its dilated ASPP branches through `block_param_grads` (`uavsal_ir_bwd_dil`, `uavsal_ir_sums_dil`) and the dense 3x3 `conv_last`
through `conv3_backward` (`uavsal_conv3_wgrad`).
`recurrence_step(srf=True)` (needs `st=True`, and so everything `st` needs): only the ImageNet `features` stay frozen.  ST
block 0 is then walked with `need_x_grad=True`, and `srf_head_backward` carries its input gradient (d loss / d
`taps["sfnet"]`) over the `c3` / `c4` / `c5` taps to the head's 42 parameters (`.grad` set, or added to); no gradient is
formed for the taps themselves.  Refresh `*train.srf_head(model)` afterwards as well (not `model.sfnet`: the stem and
`features[1]` cannot be refreshed in place, and the transposed-layout fused blocks only with `fused_t=True`)."""
import ctypes as C

import torch

from .. import _lib as L
from ..ops import _nhwc_view, _stream
from ..weights import WeightCache
from ._common import _block_grad_out, _conv, _grad_slots, _nhwc, conv3_wgrad
from .block import BLOCK_PARAMS, _block_recompute, _param_grad_parts, block_param_grads, ir_bwd_dil
from .ctx import bilinear_bwd
from .st import ST_CBR_PARAMS, _cbr_parts, _cbr_walk, cbr_backward

SRF_HEAD = ("conv_lv3", "conv_lv4", "lv5_aspp1", "lv5_aspp2", "lv5_aspp3", "lv5_aspp4", "conv_lv5", "conv_last")
SRF_HEAD_BLOCKS = ("lv5_aspp2", "lv5_aspp3", "lv5_aspp4")           # the dilated inverted-residual branches; the rest conv + BN + ReLU6
SRF_HEAD_PARAMS = tuple("%s.%s" % (m, n) for m in SRF_HEAD                 # the 42 names, relative to sfnet, in named_parameters() order
                        for n in (BLOCK_PARAMS if m in SRF_HEAD_BLOCKS else ST_CBR_PARAMS))


def srf_head(model):
    """The eight trainable modules of the SRF-Net head, in `SRF_HEAD` order: what the reference initialises itself in
    `uavsal_srfnet_aspp` (model.py:120-131).  Hand their parameters to the optimiser and the modules to
    `model.refresh_weights(*train.srf_head(model))` -- never `model.sfnet` itself, whose frozen `features` hold the stem and
    `features[1]`, which cannot be refreshed in place."""
    sf = getattr(model, "sfnet", model)
    return [getattr(sf, n) for n in SRF_HEAD]


def _conv3_parts(conv, bn):
    if (not isinstance(conv, torch.nn.Conv2d) or not isinstance(bn, torch.nn.BatchNorm2d) or conv.kernel_size != (3, 3)
            or conv.stride != (1, 1) or conv.padding != (1, 1) or conv.dilation != (1, 1) or conv.groups != 1
            or conv.bias is not None):
        raise RuntimeError("conv3_backward takes the dense 3x3 conv (no bias, stride 1, padding 1, dilation 1, one group) and the "
                           "BatchNorm of a BasicConv2d")
    cout, cin = conv.weight.shape[:2]
    if cout % 128 or cin % 64:
        raise RuntimeError("conv3_backward needs Cout %% 128 == 0 and Cin %% 64 == 0, got %d -> %d" % (cin, cout))
    if bn.training:
        raise RuntimeError("the BatchNorm uses its running statistics: call model.eval()")
    return cin, cout


def conv3_backward(conv, bn, x, y, grad_out, need_x_grad=True, cache=None, grads=None, accumulate=False):
    """`cbr_backward` for a dense 3x3 conv + BatchNorm + ReLU6 (the head's `conv_last`; eval mode, teacher-forced): `x`
    `[N,Cin,h,w]` its input, `y` an NHWC view `[N,h,w,C]` of its activation, `grad_out` `[N,C,h,w]`.  Returns
    `(grad_x [N,Cin,h,w] | None, grads)`, `grads` keyed by `ST_CBR_PARAMS`.  `uavsal_cbr_sums` forms `gp` and its channel sums,
    `uavsal_conv3_wgrad` `s[c] G[c][j][ky][kx]` and the row dots, `uavsal_cbr_finish` beta and gamma, and `grad_x` is one 3x3
    GEMM with the flipped, transposed weights that carry s in their rows.  Accepted: C % 128 == 0, Cin % 64 == 0."""
    lib = L.load()
    return _cbr_walk(lib, _conv3_parts(conv, bn), conv3_wgrad, 9, conv, bn, x, y, grad_out, need_x_grad, cache, grads, accumulate)


def _resize(x, ho, wo, out):
    """`uavsal_bilinear_ac` on the current stream, no synchronisation: the NHWC `x` resized (`align_corners`) into the NHWC
    view `out` `[n,ho,wo,C]` (a channel slice is written in place)."""
    lib = L.load()
    ip, ldi, n, h, w, c = _nhwc_view(x)
    op, ldo, *_ = _nhwc_view(out)
    d = L.BilinearDesc()
    d.inp, d.ldi, d.Hi, d.Wi, d.out, d.ldo, d.Ho, d.Wo = ip, ldi, h, w, op, ldo, ho, wo
    d.n_out, d.C, d.src_mod, d.src_div = n, c, n, 1
    L.check(lib.uavsal_bilinear_ac(C.byref(d), _stream(x)), "uavsal_bilinear_ac")


def _srf_parts(sfnet):
    """The head's modules checked: `(lv3, lv4, aspp1, [(branch, parts, dilation)] * 3, lv5, last)`, or a RuntimeError."""
    if not all(hasattr(sfnet, n) for n in SRF_HEAD):
        raise RuntimeError("srf_head_backward takes model.sfnet (an uavsal_srfnet_aspp)")
    if sfnet.training:
        raise RuntimeError("the head's BatchNorms use their running statistics: call model.eval()")
    lv3, lv4, a1, lv5, last = (getattr(sfnet, n) for n in ("conv_lv3", "conv_lv4", "lv5_aspp1", "conv_lv5", "conv_last"))
    for cv in (lv3, lv4, a1, lv5):
        _cbr_parts(cv[0], cv[1])
    _conv3_parts(last[0], last[1])
    branches = []
    for n in SRF_HEAD_BLOCKS:
        b = getattr(sfnet, n)
        prt = _param_grad_parts(b)
        if b.use_res_connect or b.stride != 1:
            raise RuntimeError("srf_head_backward: the ASPP branch %s has stride 1 and no residual" % n)
        branches.append((b, prt, prt[2].dilation[0]))
    return lv3, lv4, a1, branches, lv5, last


def srf_head_backward(sfnet, c3, c4, c5, y, grad_out, cache=None, parts=None, grads=None, accumulate=False, need_tap_grads=False,
                      need_c3_grad=False):
    """Backward of the SRF-Net head that is TRAINED (`model.sfnet` behind its frozen `features`, reference model.py:139-158;
    eval mode: every BatchNorm on its running statistics, which are not updated): `c3` `[N,32,h,w]`, `c4` `[N,96,h4,w4]`, `c5`
    `[N,320,h5,w5]` the backbone taps, `y` `[N,256,h,w]` the head's output (`taps["sfnet"]`, `conv_last`'s own activation),
    `grad_out` `[N,256,h,w]` = d loss / d `y`.  Returns `grads`, keyed by the 42 parameter names relative to `sfnet`
    (`SRF_HEAD_PARAMS`), written into the given dict of dense tensors or with `accumulate` added to it.  No input gradient is
    formed for `c3` / `c4` / `c5`: the features stay frozen.
        a1 = CBR(lv5_aspp1, c5);  a_b = BN(W3 ReLU6(BN(dw_dil(CBR(expand, c5)))))  (b = 2, 3, 4; dilation 6, 12, 18)
        x5 = CBR(conv_lv5, cat[a1, a2, a3, a4]);  x4 = CBR(conv_lv4, c4);  x3 = CBR(conv_lv3, c3)
        y = CBR3x3(conv_last, cat[up(x5), up(x4), x3])
    The intermediates are recomputed by the forward's own launches, each once.  The walk: `conv_last` (`conv3_backward`), the
    two upsamples (`bilinear_bwd`), `conv_lv3`, `conv_lv4`, `conv_lv5` (`cbr_backward`; only `conv_lv5` forms its input
    gradient), `lv5_aspp1` (`cbr_backward`) and the three dilated branches (one 256 -> 1920 GEMM with s3 in its rows,
    `uavsal_ir_bwd_dil`, `block_param_grads`).  `parts` receives every intermediate (NHWC): `a1`, `e2..4`, `d2..4`, `a2..4`,
    `aspp`, `x5`, `x4`, `x3`, `cat`, `g_cat`, `g_x5`, `g_x4`, `g_aspp`, `gd2..4`, `ga2..4`.  A head in training mode or CPU tensors
    raise.
    `need_tap_grads=True` (the backbone stage, `backbone_backward`): returns `(grads, g_c4, g_c5)`, the gradients of the `c4`
    `[N,96,h4,w4]` and `c5` `[N,320,h5,w5]` taps as well.  `g_c4` is `conv_lv4`'s input gradient (`cbr_backward` forms it);
    `g_c5` is the sum of `lv5_aspp1`'s input gradient and the three branches' `ga_b . (diag(s1) W1_b)`, each one GEMM with the
    transposed scaled expand weights whose `res=` operand is the sum so far: no pass over the sum of its own.  `c3` gets no
    gradient (its producers stay frozen).  The 42 parameter gradients are the default call's, bit for bit; the default call
    runs the launches it always ran.
    `need_c3_grad=True` (the shallow-backbone stage, `shallow_backward`): `g_c3` `[N,32,h,w]`, `conv_lv3`'s input gradient
    (`cbr_backward` forms it: one more GEMM), is appended to what the call returns -- `(grads, g_c4, g_c5, g_c3)` with
    `need_tap_grads`, `(grads, g_c3)` without.  Every other result keeps its launches and bits."""
    lib = L.load()
    lv3, lv4, a1m, branches, lv5, last = _srf_parts(sfnet)
    c3n, c4n, c5n = (_nhwc(t, nm, cv[0].weight.shape[1]) for t, nm, cv in ((c3, "c3", lv3), (c4, "c4", lv4), (c5, "c5", a1m)))
    N, hh, ww, _ = c3n.shape
    if c4n.shape[0] != N or c5n.shape[0] != N or any(t.device != c3n.device for t in (c4n, c5n)):
        raise RuntimeError("c3, c4, c5 must hold the same frames on one device")
    cout = last[0].weight.shape[0]
    go = _block_grad_out(grad_out, c3n, cout)
    yn = _nhwc(y, "y", cout)
    if yn.shape != go.shape or yn.device != go.device:
        raise RuntimeError("y must be [%d,%d,%d,%d] on the device of c3" % (N, cout, hh, ww))
    dev = c3n.device
    params = dict(sfnet.named_parameters())
    if any(n not in params for n in SRF_HEAD_PARAMS):
        raise RuntimeError("the head's parameters must be %r" % (SRF_HEAD_PARAMS,))
    grads = _grad_slots({n: params[n] for n in SRF_HEAD_PARAMS}, grads, accumulate, "grads")      # raise before anything is launched
    sub_g = lambda m, names: {n: grads["%s.%s" % (m, n)] for n in names}  # noqa: E731
    nchw = lambda t: t.permute(0, 3, 1, 2)                                # noqa: E731
    cbr = lambda cv, x: _conv(lib, cache, x, cv[0], cv[0].weight.shape[0], 1, bn=cv[1], act=L.ACT_RELU6)               # noqa: E731
    with torch.cuda.device(dev):
        cache = cache or WeightCache(dev, {})
        # ---- the forward's intermediates
        a = [cbr(a1m, c5n)]
        eds = []
        for b, prt, dil in branches:
            e, d = _block_recompute(lib, cache, b, c5n, 1, prt, dil)
            eds.append((e, d))
            a.append(_conv(lib, cache, d, prt[4], prt[4].weight.shape[0], 1, bn=prt[5]))
        aspp = torch.cat(a, 3)
        x5, x4, x3 = cbr(lv5, aspp), cbr(lv4, c4n), cbr(lv3, c3n)
        n5, n4, n3 = x5.shape[3], x4.shape[3], x3.shape[3]
        cat = torch.empty((N, hh, ww, n5 + n4 + n3), dtype=torch.float32, device=dev)
        _resize(x5, hh, ww, cat[..., :n5])
        _resize(x4, hh, ww, cat[..., n5:n5 + n4])
        cat[..., n5 + n4:].copy_(x3)
        # ---- the walk back
        g_cat, _ = conv3_backward(last[0], last[1], nchw(cat), yn, nchw(go), cache=cache, grads=sub_g("conv_last", ST_CBR_PARAMS),
                                  accumulate=accumulate)
        g_cat = g_cat.permute(0, 2, 3, 1)
        g_x5 = bilinear_bwd(g_cat[..., :n5], N, x5.shape[1], x5.shape[2])
        g_x4 = bilinear_bwd(g_cat[..., n5:n5 + n4], N, x4.shape[1], x4.shape[2])
        g_c3, _ = cbr_backward(lv3[0], lv3[1], nchw(c3n), x3, nchw(g_cat[..., n5 + n4:]), need_x_grad=bool(need_c3_grad), cache=cache,
                               grads=sub_g("conv_lv3", ST_CBR_PARAMS), accumulate=accumulate)
        g_c4, _ = cbr_backward(lv4[0], lv4[1], nchw(c4n), x4, nchw(g_x4), need_x_grad=bool(need_tap_grads), cache=cache,
                               grads=sub_g("conv_lv4", ST_CBR_PARAMS), accumulate=accumulate)
        g_aspp, _ = cbr_backward(lv5[0], lv5[1], nchw(aspp), x5, nchw(g_x5), cache=cache, grads=sub_g("conv_lv5", ST_CBR_PARAMS),
                                 accumulate=accumulate)
        g_aspp = g_aspp.permute(0, 2, 3, 1)
        w1 = a[0].shape[3]
        g_c5, _ = cbr_backward(a1m[0], a1m[1], nchw(c5n), a[0], nchw(g_aspp[..., :w1]), need_x_grad=bool(need_tap_grads), cache=cache,
                               grads=sub_g("lv5_aspp1", ST_CBR_PARAMS), accumulate=accumulate)
        if need_tap_grads:
            g_c5 = g_c5.permute(0, 2, 3, 1)
        gds, gas = [], []
        for i, ((b, prt, dil), (e, d)) in enumerate(zip(branches, eds)):
            wb = prt[4].weight.shape[0]
            gb = g_aspp[..., w1 + i * wb:w1 + (i + 1) * wb]
            gd = _conv(lib, cache, gb, prt[4], prt[0].weight.shape[0], 1, tscale=prt[5])
            ga = ir_bwd_dil(gd, d, e, *cache.depthwise(prt[2], prt[3])[:2], dil)
            block_param_grads(b, nchw(c5n), e, d, nchw(gb), gd=gd, ga=ga, cache=cache, out=sub_g(SRF_HEAD_BLOCKS[i], BLOCK_PARAMS),
                              accumulate=accumulate)
            gds.append(gd)
            gas.append(ga)
            if need_tap_grads:                                           # + ga_b . (diag(s1) W1_b), added to the sum so far
                g_c5 = _conv(lib, cache, ga, prt[0], prt[0].weight.shape[1], 1, tscale=prt[1], res=g_c5)
        if parts is not None:
            parts.update(a1=a[0], aspp=aspp, x5=x5, x4=x4, x3=x3, cat=cat, g_cat=g_cat, g_x5=g_x5, g_x4=g_x4, g_aspp=g_aspp)
            for i in range(len(branches)):
                parts.update({"e%d" % (i + 2): eds[i][0], "d%d" % (i + 2): eds[i][1], "a%d" % (i + 2): a[i + 1],
                              "gd%d" % (i + 2): gds[i], "ga%d" % (i + 2): gas[i]})
    ret = (grads, g_c4, nchw(g_c5)) if need_tap_grads else (grads,)
    if need_c3_grad:
        ret += (g_c3,)
    return ret if len(ret) > 1 else grads
