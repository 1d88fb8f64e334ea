"""The MobileNetV2 backbone `model.sfnet.features.features` as two stages; only the stem and `features[1]` stay frozen, and
BatchNorm in eval mode remains the documented difference from the reference.
The ninth, the deep backbone `features[8:18]` (`backbone_blocks`, `backbone_backward`), what the reference's unfrozen form
does (Demo_Train_Test.py:58 freezes only "to improve the training speed"): the ten blocks at 1/16 and 1/32 resolution go
through `block_backward(backbone=True)` (their widths are multiples of 32: `uavsal_pix_gemm` with `tails32`).
`recurrence_step(backbone=True)` (needs `srf=True`, and so everything `srf` needs): `srf_head_backward` then also returns the
gradients of the `c4` / `c5` taps and `backbone_backward` walks blocks 17 .. 8 over the `c3` tap, setting -- or adding to --
the `.grad` of their 90 parameters.  `features[0..7]` stay frozen (`features[2:8]` unless `shallow` is given).  Refresh
`*train.backbone_blocks(model)` afterwards as well.
The tenth, the shallow backbone `features[2:8]` (`shallow_blocks`, `shallow_backward`; csrc/train_shallow.hip): the six
blocks with an expand conv, at 1/4 to 1/16 resolution, go through `block_backward(shallow=True)` (widths of 16 to 192:
`skinny_wgrad` for the weight gradients `uavsal_pix_gemm` refuses, the channel sums with their Ch % 16 opt-in).
`recurrence_step(shallow=True)` (needs `backbone=True`, and so everything `backbone` needs): `srf_head_backward` then also
returns the gradient of the `c3` tap, `backbone_backward` the gradient of block 7's output, and `shallow_backward` walks
blocks 7 .. 2 over the input frames `x`, setting -- or adding to -- the `.grad` of their 54 parameters.  Refresh
`*train.shallow_blocks(model)` with `fused_t=True` afterwards as well."""
import ctypes as C

import torch

from .. import _lib as L
from ..ops import _nhwc_view, _stream
from ..synth import IMAGENET_MEAN, IMAGENET_STD
from ..weights import WeightCache
from ._common import _conv, _grad_slots, _nhwc
from .block import BLOCK_PARAMS, _block_backward, _block_recompute, _input_grad_parts, _param_grad_parts

BACKBONE_FIRST, BACKBONE_END = 8, 18                                 # features[8:18]: the blocks at 1/16 and 1/32 resolution
BACKBONE_C4 = 13                                                     # the block whose output is the c4 tap (c5: block 17)
BACKBONE_PARAMS = tuple("%d.%s" % (i, n) for i in range(BACKBONE_FIRST, BACKBONE_END) for n in BLOCK_PARAMS)      # the 90 names


def _feature_params(features, first, end):
    """`{"<i>.<name>": parameter}` of `features[first:end]`, in `named_parameters()` order."""
    return {"%d.%s" % (i, n): q for i in range(first, end) for n, q in features[i].named_parameters()}


def _unfused_forward(lib, cache, blk, prt, x):
    """`(e, d, output)` of a block by the forward's own UNFUSED launches, the residual as the projection's `res=` operand."""
    e, d = _block_recompute(lib, cache, blk, x, prt[2].stride[0], prt)
    return e, d, _conv(lib, cache, d, prt[4], prt[4].weight.shape[0], 1, bn=prt[5], res=x if blk.use_res_connect else None)


def backbone_blocks(model):
    """The ten trainable backbone blocks `model.sfnet.features.features[8:18]`, in forward order: 64 -> 384 -> 64 (three), 64 ->
    384 -> 96, 96 -> 576 -> 96 (two) at 1/16 resolution, 96 -> 576 -> 160 with stride 2, 160 -> 960 -> 160 (two) and 160 -> 960
    -> 320 at 1/32.  Hand their parameters to the optimiser and the modules to `model.refresh_weights(*train.backbone_blocks(
    model))`: their packed forms (natural-layout fused entries or unfused launches) are remade in place.  `features[2:8]`
    are the next stage (`shallow_blocks`); the stem and `features[1]` stay frozen."""
    sf = getattr(model, "sfnet", model)
    return list(sf.features.features[BACKBONE_FIRST:BACKBONE_END])


def backbone_backward(features, c3, g_c4, g_c5, cache=None, parts=None, grads=None, accumulate=False, need_x_grad=False):
    """Backward of the backbone blocks that are TRAINED, `features[8:18]` of `features = model.sfnet.features.features` (eval
    mode: every BatchNorm on its running statistics, which are not updated): `c3` `[N,32,h,w]` the 1/8-scale tap (the output
    of the frozen `features[6]`), `g_c4` `[N,96,h4,w4]` and `g_c5` `[N,320,h5,w5]` the gradients of the `c4` / `c5` taps
    (`srf_head_backward(need_tap_grads=True)`; `h4 = (h-1)//2+1`, `h5 = (h4-1)//2+1`).  Returns `grads`, keyed
    `"<i>.<BLOCK_PARAMS name>"` (`BACKBONE_PARAMS`, 90 names), written into the given dict of dense tensors or with `accumulate`
    added to it.
    Recompute: `x7 .. x17` (`x_i` the output of `features[i]`) from `c3` by the forward's own UNFUSED launches -- expand conv,
    `uavsal_dw3x3`, projection with the residual as its `res=` operand; block 7 (32 -> 192 -> 64, stride 2) is recomputed
    frozen.  The recomputed `x13` / `x17` differ from the `c4` / `c5` taps only by the rounding between the fused and unfused
    forward launches (blocks 7..13 may have run as fused entries), as the other stages' recomputes do from theirs.
    Walk: from `g_c5` through blocks 17 .. 14 (`block_backward(backbone=True)`; block 14 has stride 2 and no residual, so its
    `grad_x` GEMM adds `g_c4` as its `res=` operand), then blocks 13 .. 8; block 8 forms no input gradient.
    `parts` receives `x7..x17`, `e8..e17`, `d8..d17`, `gd8..gd17`, `ga8..ga17` (dense NHWC) and `g8..g17`, the gradient of
    each `x_i` the walk held (`g17` is `g_c5`, `g13` has `g_c4` added; no `g7`).  A block in training mode or CPU tensors raise.
    `need_x_grad=True` (the shallow-backbone stage, `shallow_backward`): block 8 forms its input gradient too (one more GEMM)
    and the call returns `(grads, g_x7)`, `g_x7` `[N,64,h4,w4]` the gradient of block 7's output; `parts` then holds it as `g7`.
    The 90 gradients keep their launches and bits."""
    lib = L.load()
    if not hasattr(features, "__getitem__") or len(features) < BACKBONE_END:
        raise RuntimeError("backbone_backward takes model.sfnet.features.features (the MobileNetV2 Sequential)")
    p7 = _input_grad_parts(features[BACKBONE_FIRST - 1])
    prts = {i: _param_grad_parts(features[i], True) for i in range(BACKBONE_FIRST, BACKBONE_END)}
    c3n = _nhwc(c3, "c3", p7[0].weight.shape[1])
    N, hh, ww, _ = c3n.shape
    dev = c3n.device
    down = lambda v: (v - 1) // 2 + 1                                     # noqa: E731
    nchw = lambda t: t.permute(0, 3, 1, 2)                                # noqa: E731
    h4, w4 = down(hh), down(ww)
    for nm, g, c, a, b in (("g_c4", g_c4, 96, h4, w4), ("g_c5", g_c5, 320, down(h4), down(w4))):
        if (not torch.is_tensor(g) or not g.is_cuda or g.dtype != torch.float32 or g.device != dev
                or tuple(g.shape) != (N, prts[BACKBONE_C4 if nm == "g_c4" else BACKBONE_END - 1][4].weight.shape[0], a, b)):
            raise RuntimeError("%s must be a float32 cuda tensor [%d,%d,%d,%d] on the device of c3" % (nm, N, c, a, b))
    params = _feature_params(features, BACKBONE_FIRST, BACKBONE_END)
    if tuple(params) != BACKBONE_PARAMS:
        raise RuntimeError("the backbone's parameters must be %r of features[%d:%d]" % (BLOCK_PARAMS, BACKBONE_FIRST, BACKBONE_END))
    grads = _grad_slots(params, grads, accumulate, "grads")              # raise before anything is launched
    sub_g = lambda i: {n: grads["%d.%s" % (i, n)] for n in BLOCK_PARAMS}  # noqa: E731
    g4 = _nhwc(g_c4, "g_c4")
    with torch.cuda.device(dev):
        cache = cache or WeightCache(dev, {})
        xs, eds = {BACKBONE_FIRST - 2: c3n}, {}
        xs[BACKBONE_FIRST - 1] = _unfused_forward(lib, cache, features[BACKBONE_FIRST - 1], p7, c3n)[2]
        for i in range(BACKBONE_FIRST, BACKBONE_END):
            e, d, xs[i] = _unfused_forward(lib, cache, features[i], prts[i], xs[i - 1])
            eds[i] = (e, d)
        g, gs, pts = g_c5, {}, {}
        for i in range(BACKBONE_END - 1, BACKBONE_FIRST - 1, -1):
            gs[i] = g
            pts[i] = {}
            g, _ = _block_backward(features[i], nchw(xs[i - 1]), g, i > BACKBONE_FIRST or bool(need_x_grad), cache, pts[i], sub_g(i), accumulate,
                                   ed=eds[i], res=g4 if i == BACKBONE_C4 + 1 else None, backbone=True)
        if parts is not None:
            for i in range(BACKBONE_FIRST - 1, BACKBONE_END):
                parts["x%d" % i] = xs[i]
            for i in range(BACKBONE_FIRST, BACKBONE_END):
                parts.update({"%s%d" % (k, i): v for k, v in pts[i].items()})
                parts["g%d" % i] = _nhwc(gs[i], "g")
            if need_x_grad:
                parts["g%d" % (BACKBONE_FIRST - 1)] = _nhwc(g, "g")
    return (grads, g) if need_x_grad else grads


SHALLOW_FIRST, SHALLOW_END = 2, 8                                    # features[2:8]: the blocks at 1/4, 1/8 and (block 7's output) 1/16
SHALLOW_C3 = 6                                                       # the block whose output is the c3 tap
SHALLOW_PARAMS = tuple("%d.%s" % (i, n) for i in range(SHALLOW_FIRST, SHALLOW_END) for n in BLOCK_PARAMS)         # the 54 names


def shallow_blocks(model):
    """The six trainable shallow backbone blocks `model.sfnet.features.features[2:8]`, in forward order: 16 -> 96 -> 24 with
    stride 2, 24 -> 144 -> 24 at 1/4 resolution, 24 -> 144 -> 32 with stride 2, 32 -> 192 -> 32 (two) at 1/8, 32 -> 192 -> 64
    with stride 2.  Hand their parameters to the optimiser and the modules to `model.refresh_weights(*train.shallow_blocks(
    model), fused_t=True)`: their packed forms are transposed-layout fused entries, which that keyword remakes in place.  The
    stem and `features[1]` (the one block without an expand conv) stay frozen."""
    sf = getattr(model, "sfnet", model)
    return list(sf.features.features[SHALLOW_FIRST:SHALLOW_END])


def _stem_forward(lib, cache, stem, x):
    """`features[0]` (conv 3x3 stride 2 + BatchNorm + ReLU6) on the frames `x` `[N,3,H,W]` (fp32, or uint8 RGB that the kernel
    normalises on load) -> NHWC `[N,(H-1)//2+1,(W-1)//2+1,32]`: the forward's own `uavsal_stem_conv`, no synchronisation."""
    n, _, H, W = x.shape
    out = torch.empty((n, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 32), dtype=torch.float32, device=x.device)
    ws, s, b = cache.stem(stem[0], stem[1])
    d = L.StemDesc()
    if x.dtype == torch.uint8:
        d.inp, d.in_u8 = None, x.data_ptr()
    else:
        d.inp, d.in_u8 = x.data_ptr(), None
    d.w, d.scale, d.bias, d.out, d.ldo = ws.data_ptr(), s.data_ptr(), b.data_ptr(), out.data_ptr(), 32
    d.n_img, d.H, d.W = n, H, W
    for i in range(3):
        d.mean[i], d.stdv[i] = IMAGENET_MEAN[i], IMAGENET_STD[i]
    L.check(lib.uavsal_stem_conv(C.byref(d), _stream(out)), "uavsal_stem_conv")
    return out


def _fused_forward(lib, cache, blk, x):
    """One FROZEN small-channel inverted-residual block as the forward's one launch (`uavsal_fused_ir`, transposed-layout
    weights from `cache.fused_block`): `x` NHWC -> its output NHWC.  No synchronisation."""
    ip, ldi, n, h, w, cin = _nhwc_view(x)
    dwc = list(blk.conv)[0 if blk.expand_ratio == 1 else 1][0]
    hid, cout, stride = dwc.weight.shape[0], blk.conv[-2].weight.shape[0], dwc.stride[0]
    out = torch.empty((n, (h - 1) // stride + 1, (w - 1) // stride + 1, cout), dtype=torch.float32, device=x.device)
    d = L.FusedIrDesc()
    d.inp, d.ldi = ip, ldi
    d.n_img, d.H, d.W, d.Cin, d.hidden, d.Cout, d.stride, d.tile = n, h, w, cin, hid, cout, stride, 0
    d.w1 = (1 << 20) if blk.expand_ratio != 1 else None
    if int(lib.uavsal_fused_ir_supported(C.byref(d))) != 1:
        raise RuntimeError("no transposed-layout fused instance for (Cin, hidden, Cout, stride) = %s" % ((cin, hid, cout, stride),))
    ws = cache.fused_block(blk, False)
    if blk.expand_ratio != 1:
        d.w1, d.scale1, d.bias1 = ws["w1"].data_ptr(), ws["s1"].data_ptr(), ws["b1"].data_ptr()
    else:
        d.w1 = None
    d.wd, d.scale_d, d.bias_d = ws["wd"].data_ptr(), ws["sd"].data_ptr(), ws["bd"].data_ptr()
    d.w2, d.scale2, d.bias2 = ws["w2"].data_ptr(), ws["s2"].data_ptr(), ws["b2"].data_ptr()
    if blk.use_res_connect:
        d.res, d.ldr = ip, ldi
    d.out, d.ldo = out.data_ptr(), cout
    L.check(lib.uavsal_fused_ir(C.byref(d), _stream(x)), "uavsal_fused_ir")
    return out


def shallow_backward(features, x, g_c3, g_x7, cache=None, parts=None, grads=None, accumulate=False):
    """Backward of the shallow backbone blocks that are TRAINED, `features[2:8]` of `features = model.sfnet.features.features`
    (eval mode: every BatchNorm on its running statistics, which are not updated): `x` `[N,3,H,W]` the model's input frames as
    `recurrence_step` receives them, `g_c3` `[N,32,h,w]` the gradient of the `c3` tap (`srf_head_backward(need_c3_grad=True)`;
    `h` is `H` halved three times, each time `(v-1)//2+1`) and `g_x7` `[N,64,h4,w4]` the gradient of block 7's output
    (`backbone_backward(need_x_grad=True)`).  Returns `grads`, keyed `"<i>.<BLOCK_PARAMS name>"` (`SHALLOW_PARAMS`, 54 names),
    written into the given dict of dense tensors or with `accumulate` added to it.
    Recompute: `x0` by the stem's launch and `x1` by `features[1]`'s one fused launch, both frozen; then `x2 .. x7` and every
    block's `(e, d)` by the forward's own UNFUSED launches (expand conv, `uavsal_dw3x3`, projection with the residual as its
    `res=` operand), as `backbone_backward` does -- block 7 a second time, here trained.
    Walk: `g_x7` enters block 7 (stride 2, no residual), whose `grad_x` GEMM adds `g_c3` as its `res=` operand; blocks 6 and 5
    (residual), 4 (stride 2), 3 (residual) and 2, which forms no input gradient (`block_backward(shallow=True)`).
    `parts` receives `x0..x7`, `e2..e7`, `d2..d7`, `gd2..gd7`, `ga2..ga7` (dense NHWC) and `g2..g7`, the gradient of each `x_i`
    the walk held (`g7` is `g_x7`, `g6` has `g_c3` added).  A block in training mode or CPU tensors raise."""
    lib = L.load()
    if not hasattr(features, "__getitem__") or len(features) < SHALLOW_END:
        raise RuntimeError("shallow_backward takes model.sfnet.features.features (the MobileNetV2 Sequential)")
    prts = {i: _param_grad_parts(features[i], False, True) for i in range(SHALLOW_FIRST, SHALLOW_END)}
    stem, f1 = features[0], features[1]
    if stem.training or f1.training:
        raise RuntimeError("the stem and features[1] are frozen: their BatchNorms are folded in eval mode (call model.eval())")
    if (not torch.is_tensor(x) or not x.is_cuda or x.dim() != 4 or x.shape[1] != 3 or x.dtype not in (torch.float32, torch.uint8)):
        raise RuntimeError("x must be the input frames, a float32 (or uint8) cuda tensor [N,3,H,W] (no CPU fallback)")
    dev = x.device
    down = lambda v: (v - 1) // 2 + 1                                     # noqa: E731
    nchw = lambda t: t.permute(0, 3, 1, 2)                                # noqa: E731
    N = x.shape[0]
    h3, w3 = down(down(down(x.shape[2]))), down(down(down(x.shape[3])))
    for nm, g, i, a, b in (("g_c3", g_c3, SHALLOW_C3, h3, w3), ("g_x7", g_x7, SHALLOW_END - 1, down(h3), down(w3))):
        c = prts[i][4].weight.shape[0]
        if (not torch.is_tensor(g) or not g.is_cuda or g.dtype != torch.float32 or g.device != dev or tuple(g.shape) != (N, c, a, b)):
            raise RuntimeError("%s must be a float32 cuda tensor [%d,%d,%d,%d] on the device of x" % (nm, N, c, a, b))
    params = _feature_params(features, SHALLOW_FIRST, SHALLOW_END)
    if tuple(params) != SHALLOW_PARAMS:
        raise RuntimeError("the shallow backbone's parameters must be %r of features[%d:%d]" % (BLOCK_PARAMS, SHALLOW_FIRST, SHALLOW_END))
    grads = _grad_slots(params, grads, accumulate, "grads")              # raise before anything is launched
    sub_g = lambda i: {n: grads["%d.%s" % (i, n)] for n in BLOCK_PARAMS}  # noqa: E731
    g3 = _nhwc(g_c3, "g_c3")
    with torch.cuda.device(dev):
        cache = cache or WeightCache(dev, {})
        xs, eds = {0: _stem_forward(lib, cache, stem, x.contiguous())}, {}
        xs[1] = _fused_forward(lib, cache, f1, xs[0])
        for i in range(SHALLOW_FIRST, SHALLOW_END):
            e, d, xs[i] = _unfused_forward(lib, cache, features[i], prts[i], xs[i - 1])
            eds[i] = (e, d)
        g, gs, pts = g_x7, {}, {}
        for i in range(SHALLOW_END - 1, SHALLOW_FIRST - 1, -1):
            gs[i] = g
            pts[i] = {}
            g, _ = _block_backward(features[i], nchw(xs[i - 1]), g, i > SHALLOW_FIRST, cache, pts[i], sub_g(i), accumulate,
                                   ed=eds[i], res=g3 if i == SHALLOW_C3 + 1 else None, shallow=True)
        if parts is not None:
            for i in range(SHALLOW_END):
                parts["x%d" % i] = xs[i]
            for i in range(SHALLOW_FIRST, SHALLOW_END):
                parts.update({"%s%d" % (k, i): v for k, v in pts[i].items()})
                parts["g%d" % i] = _nhwc(gs[i], "g")
    return grads
