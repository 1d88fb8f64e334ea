"""The backward of a general inverted-residual block (`dwBlock`, `model_feature.InvertedResidual`), which every stage in front
of the recurrence goes through: trained (`block_backward`, `block_param_grads`; csrc/train_block.hip: `uavsal_ir_bwd`,
`uavsal_ir_sums`, `uavsal_ir_finish`, and `uavsal_pix_gemm` for both 1x1 weight gradients) or frozen (`block_input_grad`), with
the stride-2 launches (`uavsal_ir_bwd_s2` of csrc/train_ctx.hip, `uavsal_ir_sums_s2`), the dilated ones (`uavsal_ir_bwd_dil` of
csrc/train_srf.hip, `uavsal_ir_sums_dil`; the three sums are one kernel in csrc/train_block.hip) and the Ch % 16 opt-in of
csrc/train_shallow.hip.
The third stage is one such block, the fusion block that produces the recurrence's input (`fuse_block`:
`model.fucbst_layer[0]`, or `model.fust_layer[0]` without priors).  `recurrence_step(fuse=True)`: the recurrence's backward
also returns the gradient of its input, which `block_backward` carries to that block's nine parameters (`.grad` set, or added
to); everything in front of the block stays frozen, and nothing of `prefuse` bypasses the recurrence, so the gradient is
exact.  Refresh `model.fucbst_layer` (or `model.fust_layer` in a model without priors) afterwards as well."""
import ctypes as C

import torch

from .. import _lib as L
from ..ops import _nhwc_view, _stream
from ..weights import WeightCache
from ._common import _block_grad_out, _conv, _dense_nhwc, _grad_slots, _nhwc, pix_gemm, skinny_wgrad
from .decoder import DECODER_PARAMS

BLOCK_PARAMS = DECODER_PARAMS                                        # a dwBlock with an expand conv: the same nine names

_BLOCK_SHAPE = "(expand 1x1, depthwise 3x3, projection 1x1)"
_FEATURES_SHAPE = ("an inverted-residual block with an expand conv (expand 1x1, depthwise 3x3, projection 1x1: features[2..17]), "
                   "not features[1] or the stem", "stride 1 or 2 at dilation 1 (a dilated block with stride 2 is not covered)")
# The block-shape rule, one row per kind: the noun of its messages, the strides it takes, whether a dilation above 1 is taken
# (at stride 1), the moduli of (Cin, hidden, Cout), whether the nine parameter names are compared, and what it says it takes:
# the block and -- where that is a message of its own -- the strides.
_PARTS_RULES = {
    "block_param_grads": ("block_param_grads", (1, 2), True, (64, 64, 64), False,
                          ("a dwBlock with an expand conv, stride 1 or 2 and dilation 1, or stride 1 and a dilation above 1 "
                           + _BLOCK_SHAPE, None)),
    "block_backward": ("block_backward", (1,), False, (64, 64, 128), False,
                       ("a dwBlock with an expand conv, stride 1 and dilation 1 " + _BLOCK_SHAPE, None)),
    "block_batch": ("block_forward_batch / block_backward_batch", (1,), False, (64, 64, 128), False,
                    ("a dwBlock with an expand conv, stride 1 and dilation 1 " + _BLOCK_SHAPE, None)),
    "backbone": ("the backbone backward", (1, 2), False, (32, 64, 32), True, _FEATURES_SHAPE),
    "shallow": ("the shallow backward", (1, 2), False, (8, 16, 8), True, _FEATURES_SHAPE),
}


_BATCH_REFUSAL = ("block_forward_batch / block_backward_batch run the block's BatchNorms on BATCH statistics: call block.train() "
                  "(its container's .train() under model.eval()); a block in eval mode goes through the eval-mode functions "
                  "block_backward / block_input_grad")


def _checked_parts(block, kind):
    """`(pw, pwbn, dwc, dwbn, pl, plbn)` of an inverted-residual `block` that the row `kind` of `_PARTS_RULES` takes, or a
    RuntimeError.  The special cases of `block_param_grads` are its row's alone (`own`).  The row "block_batch" (block_bn.py)
    takes the shapes of "block_backward" in TRAINING mode, with affine BatchNorms that track their statistics."""
    noun, strides, dilated, (mod_in, mod_hid, mod_out), named, (what, what_strides) = _PARTS_RULES[kind]
    own = kind == "block_param_grads"
    seq = getattr(block, "conv", None)
    stride = getattr(block, "stride", None)
    dil = getattr(block, "dilation", None)
    shaped = seq is not None and getattr(block, "expand_ratio", 1) != 1 and len(seq) == 4
    if named and shaped:
        shaped = tuple(n for n, _ in block.named_parameters()) == BLOCK_PARAMS
    if what_strides and not shaped:
        raise RuntimeError("%s takes %s" % (noun, what))
    placed = (isinstance(dil, int) and dil >= 1 and (dil == 1 or stride == 1)) if dilated else dil == 1
    if (not shaped or stride not in strides or not placed or seq[1][0].stride != (stride, stride)
            or seq[1][0].dilation != (dil, dil)):
        raise RuntimeError("%s takes %s" % (noun, what_strides or what))
    pw, pwbn, dwc, dwbn, pl, plbn = seq[0][0], seq[0][1], seq[1][0], seq[1][1], seq[2], seq[3]
    hid, cin, cout = pw.weight.shape[0], pw.weight.shape[1], pl.weight.shape[0]
    if own and dil > 1 and cout % 128:                              # the ASPP branches of the SRF-Net head: 320 -> 1920 -> 256
        raise RuntimeError("block_param_grads takes a dilated block with Cout %% 128 == 0 only, got %d -> %d -> %d, dilation %d"
                           % (cin, hid, cout, dil))
    narrow = own and cout == 32 and 128 <= hid <= 512               # an ST block's sub_conv, 64 -> 384 -> 32 (uavsal_pix_gemm's 32-wide side)
    if (cout % mod_out and not narrow) or hid % mod_hid or cin % mod_in:
        raise RuntimeError("%s needs Cout %% %d == 0%s, hidden %% %d == 0 and Cin %% %d == 0, got %d -> %d -> %d"
                           % (noun, mod_out, " (or Cout == 32 with 128 <= hidden <= 512)" if own else "", mod_hid, mod_in,
                              cin, hid, cout))
    if own and stride == 2 and block.use_res_connect:
        raise RuntimeError("block_param_grads: a block with stride 2 has no residual")
    if kind == "block_batch":
        bns = (pwbn, dwbn, plbn)
        if not block.training or not all(b.training for b in bns):
            raise RuntimeError(_BATCH_REFUSAL)
        if not all(b.track_running_stats and b.affine and b.running_mean is not None for b in bns):
            raise RuntimeError("%s needs affine BatchNorms that track their running statistics" % noun)
    elif block.training:
        raise RuntimeError("the block's BatchNorms use their running statistics: call model.eval()")
    return pw, pwbn, dwc, dwbn, pl, plbn


def _block_parts(block, backbone=False, shallow=False):
    """`(pw, pwbn, dwc, dwbn, pl, plbn)` of an inverted-residual block the block backward covers (stride 1, dilation 1,
    Cout % 128 == 0, hidden % 64 == 0, Cin % 64 == 0), or a RuntimeError.  `backbone`: the shapes of MobileNetV2
    `features[8:18]` instead, `shallow`: those of `features[2:8]` (`_param_grad_parts`)."""
    return _checked_parts(block, "shallow" if shallow else "backbone" if backbone else "block_backward")


def _param_grad_parts(block, backbone=False, shallow=False):
    """`(pw, pwbn, dwc, dwbn, pl, plbn)` of an inverted-residual block whose nine gradients `block_param_grads` forms: what
    `_block_parts` takes, and stride 2 and Cout % 64 == 0 besides (the blocks of the multi-prior path), or a RuntimeError.
    `backbone` (MobileNetV2 `features[8:18]`, with or without the residual), `shallow` (`features[2:8]`, an expand conv present;
    it takes what `backbone` takes as well): their rows of `_PARTS_RULES` instead; `block_param_grads` lists the shapes.
    `model_feature.InvertedResidual` and `dwBlock` are the same module to this code: the same `conv` Sequential, the same nine
    parameter names (`BLOCK_PARAMS`), which is checked for those two."""
    return _checked_parts(block, "shallow" if shallow else "backbone" if backbone else "block_param_grads")


def _block_slots(block, out, accumulate):
    params = dict(block.named_parameters())
    if sorted(params) != sorted(BLOCK_PARAMS):
        raise RuntimeError("the block's parameters must be %r" % (BLOCK_PARAMS,))
    return params, _grad_slots({n: params[n] for n in BLOCK_PARAMS}, out, accumulate, "out")


# What each launch says when `gd`, `d`, `e` (and `ga`) do not fit each other: `gd` and `d` on the output grid of the depthwise
# conv, `e` and `ga` on its input grid, all on one device.
_GRID_MSG = {
    "ir_bwd": "gd, d, e must be dense float32 NHWC cuda tensors of one shape",
    "ir_bwd_s2": "gd and d must be [n,(H-1)//2+1,(W-1)//2+1,C] for e [n,H,W,C], on one device",
    "ir_bwd_dil": "gd, d, e must have one shape on one device",
    "ir_sums": "gd, d, e, ga must be dense float32 NHWC cuda tensors of one shape on one device",
    "ir_sums_s2": "gd and d must be [n,(H-1)//2+1,(W-1)//2+1,Ch] for e and ga [n,H,W,Ch], on one device",
    "ir_sums_dil": "gd, d, e, ga must have one shape on one device",
}


def _ir_grid(stem, stride, fields, gd, d, e, ga=None):
    """The checks the six launches share -> `(n, ho, wo, c)`, the shape of `gd` and `d` for `e` (and `ga`) `[n,h,w,c]` and a
    depthwise conv of `stride`; `fields["dil"]`, where the launch has a dilation, is checked behind them."""
    ts = (gd, d, e) if ga is None else (gd, d, e, ga)
    _dense_nhwc(stem, "gd, d, e" if ga is None else "gd, d, e, ga", *ts)
    n, hh, ww, c = e.shape
    grid = (n, (hh - 1) // stride + 1, (ww - 1) // stride + 1, c)
    if (tuple(gd.shape) != grid or tuple(d.shape) != grid or (ga is not None and ga.shape != e.shape)
            or any(t.device != e.device for t in ts)):
        raise RuntimeError("%s: %s" % (stem, _GRID_MSG[stem]))
    dil = fields.get("dil", 1)
    if not isinstance(dil, int) or dil < 1:
        raise RuntimeError("%s: the dilation must be an integer >= 1, got %r" % (stem, dil))
    return grid


def _ir_bwd(desc, stem, stride, gd, d, e, wd9, s2, **fields):
    """`ir_bwd`, `ir_bwd_s2` and `ir_bwd_dil`: `desc` the descriptor class, `stem` the function's name (its symbol is
    `uavsal_<stem>`), `stride` that of the `gd` / `d` grid; `fields`: what the descriptor holds besides (`dil`)."""
    lib = L.load()
    n, _, _, c = _ir_grid(stem, stride, fields, gd, d, e)
    for name, t, m in (("wd9", wd9, 9 * c), ("s2", s2, c)):
        if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.device == e.device and t.is_contiguous() and t.numel() >= m):
            raise RuntimeError("%s: %s must be a dense float32 tensor of at least %d elements on the device of e" % (stem, name, m))
    ga = torch.empty_like(e)
    k = desc()
    k.gd, k.d, k.e, k.wd9, k.s2, k.ga = gd.data_ptr(), d.data_ptr(), e.data_ptr(), wd9.data_ptr(), s2.data_ptr(), ga.data_ptr()
    k.n_img, k.H, k.W, k.C = n, e.shape[1], e.shape[2], c
    for f, v in fields.items():
        setattr(k, f, v)
    L.check(getattr(lib, "uavsal_" + stem)(C.byref(k), _stream(e)), "uavsal_" + stem)
    return ga


def _ir_sums(desc, stem, stride, gd, d, e, ga, go, **fields):
    """`ir_sums`, `ir_sums_s2` and `ir_sums_dil`: the arguments of `_ir_bwd`; `fields`: `ch16` or `dil`."""
    lib = L.load()
    n, ho, wo, c = _ir_grid(stem, stride, fields, gd, d, e, ga)
    if not torch.is_tensor(go) or go.dtype != torch.float32 or go.device != e.device:
        raise RuntimeError("%s: go must be a float32 tensor on the device of e" % stem)
    gp, ldgo, *gs = _nhwc_view(go)
    if gs[:3] != [n, ho, wo]:
        raise RuntimeError("%s: go must cover the pixels of %s" % (stem, "e" if stride == 1 else "d"))
    k = desc()
    k.gd, k.d, k.e, k.ga, k.go, k.ldgo = gd.data_ptr(), d.data_ptr(), e.data_ptr(), ga.data_ptr(), gp, ldgo
    k.n_img, k.H, k.W, k.Ch, k.Co = n, e.shape[1], e.shape[2], c, gs[3]
    for f, v in fields.items():
        setattr(k, f, v)
    symbol = "uavsal_" + stem
    nbytes = int(getattr(lib, symbol + "_workspace_bytes")(C.byref(k)))
    if nbytes <= 0:
        L.check(-3, symbol)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=e.device)
    k.ws, k.ws_bytes = ws.data_ptr(), nbytes
    L.check(getattr(lib, symbol)(C.byref(k), _stream(e)), symbol)
    return ws, int(getattr(lib, symbol + "_slabs")(C.byref(k)))


def ir_bwd(gd, d, e, wd9, s2):
    """`uavsal_ir_bwd` on the current stream: `gd`, `d`, `e` dense NHWC `[T,h,w,C]`, the tap-major depthwise weights and the
    folded scale of the depthwise BatchNorm on the device -> `ga` = d loss / d a1, dense NHWC."""
    return _ir_bwd(L.IrBwdDesc, "ir_bwd", 1, gd, d, e, wd9, s2)


def ir_bwd_s2(gd, d, e, wd9, s2):
    """`uavsal_ir_bwd_s2` on the current stream: `ir_bwd` for a depthwise 3x3 with stride 2.  `gd`, `d` dense NHWC
    `[n,Ho,Wo,C]` with `Ho = (H-1)//2+1`, `Wo = (W-1)//2+1`, `e` dense NHWC `[n,H,W,C]`, the tap-major depthwise weights and
    the folded scale of the depthwise BatchNorm on the device -> `ga` = d loss / d a1, dense NHWC like `e`."""
    return _ir_bwd(L.IrBwdS2Desc, "ir_bwd_s2", 2, gd, d, e, wd9, s2)


def ir_bwd_dil(gd, d, e, wd9, s2, dil):
    """`uavsal_ir_bwd_dil` on the current stream: `ir_bwd` for a depthwise 3x3 with stride 1 and dilation `dil` >= 1 (the ASPP
    branches of the SRF-Net head): `gd`, `d`, `e` dense NHWC `[T,h,w,C]` -> `ga` = d loss / d a1, dense NHWC."""
    return _ir_bwd(L.IrBwdDilDesc, "ir_bwd_dil", 1, gd, d, e, wd9, s2, dil=dil)


def ir_sums(gd, d, e, ga, go, ch16=False):
    """`uavsal_ir_sums` on the current stream -> `(ws, slabs)`: the per-slab partial sums (float64, the layout of
    include/uavsal_hip.h) that `uavsal_ir_finish` takes.  `gd`, `d`, `e`, `ga` dense NHWC `[T,h,w,Ch]`; `go` an NHWC view
    `[T,h,w,Co]` of the same pixels (a channel slice is read in place).  `ch16=True`: any Ch % 16 == 0 is taken, not only
    Ch % 64 == 0 (the descriptor's opt-in; `ir_finish(..., ch16=True)` takes the workspace)."""
    return _ir_sums(L.IrSumsDesc, "ir_sums", 1, gd, d, e, ga, go, ch16=int(bool(ch16)))


def ir_sums_s2(gd, d, e, ga, go, ch16=False):
    """`uavsal_ir_sums_s2` on the current stream -> `(ws, slabs)`: `ir_sums` for a depthwise 3x3 with stride 2, in the same
    workspace layout.  `e`, `ga` dense NHWC `[n,H,W,Ch]`; `gd`, `d` dense NHWC `[n,Ho,Wo,Ch]` with `Ho = (H-1)//2+1`,
    `Wo = (W-1)//2+1`; `go` an NHWC view `[n,Ho,Wo,Co]` (a channel slice is read in place).  `ch16`: as in `ir_sums`."""
    return _ir_sums(L.IrSumsS2Desc, "ir_sums_s2", 2, gd, d, e, ga, go, ch16=int(bool(ch16)))


def ir_sums_dil(gd, d, e, ga, go, dil):
    """`uavsal_ir_sums_dil` on the current stream -> `(ws, slabs)`: `ir_sums` for a depthwise 3x3 with stride 1 and dilation
    `dil` >= 1, in the same workspace layout.  `gd`, `d`, `e`, `ga` dense NHWC `[T,h,w,Ch]`; `go` an NHWC view `[T,h,w,Co]` of
    the same pixels (a channel slice is read in place)."""
    return _ir_sums(L.IrSumsDilDesc, "ir_sums_dil", 1, gd, d, e, ga, go, dil=dil)


def _takes_pix_gemm(lib, M, N, K):
    """Whether `uavsal_pix_gemm` with `tails32` takes an M x N product (a host query, no launch)."""
    k = L.PixGemmDesc()
    k.K, k.M, k.N, k.tails32 = K, M, N, 1
    return int(lib.uavsal_pix_gemm_shares(C.byref(k))) > 0


def block_param_grads(block, x, e, d, grad_out, gd=None, ga=None, cache=None, out=None, accumulate=False, backbone=False,
                      shallow=False):
    """The gradients of the nine parameters of an inverted-residual `block` (a `dwBlock` with an expand conv, stride 1 or 2,
    dilation 1, with or without the residual; eval mode: the BatchNorms on their running statistics, which are not updated)
    from given tensors, teacher-forced: `x` `[T,Cin,h,w]` the block's input, `e` dense NHWC `[T,h,w,Ch]` its expanded and `d`
    dense NHWC `[T,ho,wo,Ch]` its depthwise tensor (`ho = (h-1)//stride+1`), `grad_out` `[T,Co,ho,wo]` = d loss / d output,
    `gd` dense NHWC like `d` = d loss / d d (default: one 1x1 conv with the projection's transposed weights carrying s3 in
    their rows), `ga` dense NHWC like `e` = d loss / d a1 (default: one `uavsal_ir_bwd`, or `uavsal_ir_bwd_s2`).  With stride 2
    `ga` x `x` and S1 run over the input pixels, `grad_out` x `d`, S2, Gd and S3 over the output pixels
    (`uavsal_ir_sums_s2`).  Returns a dict keyed by the block's parameter names (`BLOCK_PARAMS`), the values `torch.autograd`
    gives for the reference's `dwBlock` (include/uavsal_hip.h states the formulas); `out`: such a dict of dense tensors to
    write into, or (`accumulate`) to add to.  Nothing of the forward is recomputed; six launches (two pixel GEMMs with their
    reductions -- `ga` x `x` for W1, `grad_out` x `d` for W3 --, channel sums, finalise) on the current stream, no
    synchronisation.  Accepted: Co % 64 == 0 -- or Co == 32 with 128 <= Ch <= 512, the temporal sub-block of an ST block
    (64 -> 384 -> 32), whose W3 product is the pixel GEMM's 32-wide side --, Ch % 64 == 0, Cin % 64 == 0 (`block_backward`, which recomputes `e` and `d`
    itself, keeps to stride 1 and Co % 128 == 0).  A block with stride 1 and a DILATED depthwise conv (the ASPP branches of the
    SRF-Net head, 320 -> 1920 -> 256 at dilation 6 / 12 / 18) is taken with Co % 128 == 0: `uavsal_ir_bwd_dil` and
    `uavsal_ir_sums_dil` stand in for the undilated launches, everything else is the same.
    `backbone=True`: Cin % 32 == 0, Ch % 64 == 0, Co % 32 == 0 at dilation 1, stride 1 or 2, instead -- the blocks of MobileNetV2
    `features[8:18]` (64 -> 384 -> 64 / 96, 96 -> 576 -> 96 / 160, 160 -> 960 -> 160 / 320): the two pixel GEMMs run with
    `tails32` (quarter-tile tails, shares of 128-pixel units), everything else is the same six launches.
    `shallow=True`: Cin % 8 == 0, Ch % 16 == 0, Co % 8 == 0 at dilation 1, stride 1 or 2, instead -- the blocks of MobileNetV2
    `features[2:8]` (16 -> 96 -> 24, 24 -> 144 -> 24 / 32, 32 -> 192 -> 32 / 64).  A weight-gradient product that
    `uavsal_pix_gemm` takes (192 x 32, 32 x 192, 64 x 192) keeps that launch; the others (96 x 16, 144 x 24, 24 x 96, 24 x 144,
    32 x 144) go to `skinny_wgrad`; the channel sums and the finalise run with their Ch % 16 opt-in.  The same six launches."""
    lib = L.load()
    pw, pwbn, dwc, dwbn, pl, plbn = _param_grad_parts(block, backbone, shallow)
    hid, cin, cout = pw.weight.shape[0], pw.weight.shape[1], pl.weight.shape[0]
    stride, dil = dwc.stride[0], dwc.dilation[0]
    xn = _nhwc(x, "x", cin)
    T, hh, ww, _ = xn.shape
    ho, wo = (hh - 1) // stride + 1, (ww - 1) // stride + 1
    dev = xn.device
    for name, t, (a, b) in ((("e", e, (hh, ww)), ("d", d, (ho, wo)))
                            + tuple((n, t, s) for n, t, s in (("gd", gd, (ho, wo)), ("ga", ga, (hh, ww))) if t is not None)):
        if (not torch.is_tensor(t) or t.dtype != torch.float32 or t.device != dev or tuple(t.shape) != (T, a, b, hid)
                or not t.is_contiguous()):
            raise RuntimeError("%s must be a dense float32 NHWC tensor [%d,%d,%d,%d] on the device" % (name, T, a, b, hid))
    go = _block_grad_out(grad_out, xn, cout, stride)
    params, out = _block_slots(block, out, accumulate)
    if any(q.device != dev or not q.is_contiguous() for q in params.values()):
        raise RuntimeError("the block's parameters must be dense tensors on the device of `x`")
    with torch.cuda.device(dev):
        cache = cache or WeightCache(dev, {})
        w9, s2, _ = cache.depthwise(dwc, dwbn)
        s1, s3 = cache.affine(pwbn, hid)[0], cache.affine(plbn, cout)[0]
        if gd is None:
            gd = _conv(lib, cache, go, pl, hid, 1, tscale=plbn)
        if ga is None:
            ga = ir_bwd_dil(gd, d, e, w9, s2, dil) if dil > 1 else (ir_bwd if stride == 1 else ir_bwd_s2)(gd, d, e, w9, s2)
        (r1, mu1), (r2, mu2), (r3, mu3) = (cache.bn_stats(b) for b in (pwbn, dwbn, plbn))
        rd1 = torch.empty(hid, dtype=torch.float64, device=dev)
        rd3 = torch.empty(cout, dtype=torch.float64, device=dev)
        for a, b, name, s, wt, rd in ((ga, xn, BLOCK_PARAMS[0], s1, pw, rd1), (go, d, BLOCK_PARAMS[6], s3, pl, rd3)):
            kw = dict(out=out[name], row_scale=s, w=wt.weight.detach(), rowdot=rd, accumulate=accumulate)
            if shallow and not _takes_pix_gemm(lib, a.shape[-1], b.shape[-1], b.shape[0] * b.shape[1] * b.shape[2]):
                skinny_wgrad(a, b, **kw)
            else:
                pix_gemm(a, b, tails32=backbone or shallow, **kw)
        sums, kw = (ir_sums_dil, dict(dil=dil)) if dil > 1 else (ir_sums if stride == 1 else ir_sums_s2, dict(ch16=shallow))
        ws, slabs = sums(gd, d, e, ga, go, **kw)
        k = L.IrFinishDesc()
        k.ws, k.ws_bytes, k.rowdot1, k.rowdot3 = ws.data_ptr(), ws.numel() * 8, rd1.data_ptr(), rd3.data_ptr()
        k.wd, k.s2 = dwc.weight.data_ptr(), s2.data_ptr()
        k.r1, k.mu1, k.r2, k.mu2, k.r3, k.mu3 = (t.data_ptr() for t in (r1, mu1, r2, mu2, r3, mu3))
        (k.g_gamma1, k.g_beta1, k.g_wd, k.g_gamma2, k.g_beta2) = (out[n].data_ptr() for n in BLOCK_PARAMS[1:6])
        k.g_gamma3, k.g_beta3 = out[BLOCK_PARAMS[7]].data_ptr(), out[BLOCK_PARAMS[8]].data_ptr()
        k.Ch, k.Co, k.slabs, k.accumulate = hid, cout, slabs, int(bool(accumulate))
        if shallow:
            L.check(lib.uavsal_ir_finish_c16(C.byref(k), _stream(xn)), "uavsal_ir_finish_c16")
        else:
            L.check(lib.uavsal_ir_finish(C.byref(k), _stream(xn)), "uavsal_ir_finish")
    return out


def _block_recompute(lib, cache, block, x, stride=1, prt=None, dilation=1):
    """`e`, `d` (dense NHWC) from the NHWC `x` by the forward's own launches (expand conv, `uavsal_dw3x3`); `stride` 2: `d` is
    `[T, (h-1)/2+1, (w-1)/2+1, Ch]`.  `prt`: the block's parts when the caller has checked them (`_input_grad_parts`);
    `dilation`: that of the depthwise conv (stride 1: `srf_head_backward`)."""
    pw, pwbn, dwc, dwbn, _, _ = prt or _block_parts(block)
    T, hh, ww, _ = x.shape
    hid = pw.weight.shape[0]
    e = _conv(lib, cache, x, pw, hid, 1, bn=pwbn, act=L.ACT_RELU6)
    w9, s2, b2 = cache.depthwise(dwc, dwbn)
    dd = torch.empty((T, (hh - 1) // stride + 1, (ww - 1) // stride + 1, hid), dtype=torch.float32, device=x.device)
    q = L.DwDesc()
    q.inp, q.ldi, q.w9c, q.scale, q.bias = e.data_ptr(), hid, w9.data_ptr(), s2.data_ptr(), b2.data_ptr()
    q.out, q.ldo = dd.data_ptr(), hid
    q.n_img, q.H, q.W, q.C, q.stride, q.dilation, q.act = T, hh, ww, hid, stride, dilation, L.ACT_RELU6
    L.check(lib.uavsal_dw3x3(C.byref(q), _stream(x)), "uavsal_dw3x3")
    return e, dd


def block_backward(block, x, grad_out, need_x_grad=True, cache=None, parts=None, grads=None, accumulate=False, backbone=False,
                   shallow=False):
    """Backward of an inverted-residual `block` that is TRAINED (the blocks `block_param_grads` covers): `x` `[T,Cin,h,w]` its
    input, `grad_out` `[T,Co,h,w]` = d loss / d output.  Returns `(grad_x [T,Cin,h,w] | None, grads)` with `grads` the dict
    of `block_param_grads` (written into `grads`, or with `accumulate` added to it, when given).  `e` and `d` are recomputed
    from `x` by the forward's own launches; `gd = grad_out . (diag(s3) W3)` is one 256 -> Ch GEMM whose transposed weights
    carry s3 in their rows (`WeightCache.conv_t_scaled`), `ga` comes from `uavsal_ir_bwd`, and `grad_x = ga . (diag(s1) W1)`
    (+ `grad_out` when the block has the residual) from one Ch -> Cin GEMM of the same kind.  `parts` receives `e`, `d`,
    `gd`, `ga` (dense NHWC).  A block in training mode raises: the BatchNorms use their running statistics (which are not
    updated), as everywhere in this package.
    `backbone=True`: a block of MobileNetV2 `features[8:18]` instead (Cin % 32 == 0, hidden % 64 == 0, Cout % 32 == 0, with or
    without the residual, stride 1 or 2): with stride 2 `grad_out` is `[T,Co,(h-1)//2+1,(w-1)//2+1]`, the depthwise conv is
    recomputed with its stride, `ga` comes from `uavsal_ir_bwd_s2`, the sums from `uavsal_ir_sums_s2`, and `grad_x` runs
    over the input grid -- the walk `prior_path_backward` makes through its stride-2 blocks (`_input_grad`: one copy).
    `shallow=True`: a block of MobileNetV2 `features[2:8]` instead (Cin % 8 == 0, hidden % 16 == 0, Cout % 8 == 0): the same
    walk, with the skinny weight gradients and the Ch % 16 sums of `block_param_grads(shallow=True)`."""
    return _block_backward(block, x, grad_out, need_x_grad, cache, parts, grads, accumulate, backbone=backbone, shallow=shallow)


def _block_backward(block, x, grad_out, need_x_grad, cache, parts, grads, accumulate, ed=None, res=None, backbone=False,
                    shallow=False):
    """`block_backward`; `ed`: the block's `(e, d)` when the caller has recomputed them; `res`: an NHWC tensor the `grad_x` GEMM
    adds where the block has no residual (`st_block_backward`, `backbone_backward`)."""
    lib = L.load()
    prt = _block_parts(block, backbone, shallow)
    pw, dwc, pl = prt[0], prt[2], prt[4]
    cin, cout = pw.weight.shape[1], pl.weight.shape[0]
    xn = _nhwc(x, "x", cin)
    go = _block_grad_out(grad_out, xn, cout, dwc.stride[0])
    dev = xn.device
    _block_slots(block, grads, accumulate)                    # raise before anything is launched
    with torch.cuda.device(dev):
        cache = cache or WeightCache(dev, {})
        pt = {}
        g = _input_grad(lib, cache, block, prt, xn, go, ed=ed, parts=pt, need_x_grad=need_x_grad, res=res)
        grads = block_param_grads(block, xn.permute(0, 3, 1, 2), pt["e"], pt["d"], go.permute(0, 3, 1, 2), gd=pt["gd"], ga=pt["ga"],
                                  cache=cache, out=grads, accumulate=accumulate, backbone=backbone, shallow=shallow)
        if parts is not None:
            parts.update(pt)
    return (g.permute(0, 3, 1, 2) if need_x_grad else None), grads


def _input_grad_parts(block):
    """`(pw, pwbn, dwc, dwbn, pl, plbn)` of a FROZEN inverted-residual block `block_input_grad` covers, or a RuntimeError."""
    seq = getattr(block, "conv", None)
    stride = getattr(block, "stride", None)
    if (seq is None or getattr(block, "expand_ratio", 1) == 1 or len(seq) != 4 or stride not in (1, 2)
            or getattr(block, "dilation", None) != 1 or seq[1][0].stride != (stride, stride) or seq[1][0].dilation != (1, 1)):
        raise RuntimeError("block_input_grad takes a dwBlock with an expand conv, stride 1 or 2 and dilation 1 "
                           "(expand 1x1, depthwise 3x3, projection 1x1)")
    pw, pwbn, dwc, dwbn, pl, plbn = seq[0][0], seq[0][1], seq[1][0], seq[1][1], seq[2], seq[3]
    hid, cin, cout = pw.weight.shape[0], pw.weight.shape[1], pl.weight.shape[0]
    if cout % 32 or hid % 64 or cin % 32:
        raise RuntimeError("block_input_grad needs Cout %% 32 == 0, hidden %% 64 == 0 and Cin %% 32 == 0, got %d -> %d -> %d"
                           % (cin, hid, cout))
    if block.training:
        raise RuntimeError("the block is frozen: its BatchNorms are folded in eval mode (call model.eval())")
    return pw, pwbn, dwc, dwbn, pl, plbn


def _input_grad(lib, cache, block, prt, xn, go, ed=None, parts=None, need_x_grad=True, res=None):
    """`block_input_grad` on checked NHWC views; `ed`: the block's `(e, d)` when the caller has them.  `need_x_grad=False`:
    only `parts` is wanted (the operands of the block's parameter gradients), the last GEMM is left out and None returned.
    `res`: an NHWC tensor on the input grid that the last GEMM adds where the block has no residual.  The one walk through a
    block, trained (`_block_backward`) or frozen, stride 1 or 2."""
    pw, pwbn, dwc, dwbn, pl, plbn = prt
    hid, cin = pw.weight.shape[:2]
    stride = dwc.stride[0]
    e, dd = ed or _block_recompute(lib, cache, block, xn, stride, prt)
    gd = _conv(lib, cache, go, pl, hid, 1, tscale=plbn)
    ga = (ir_bwd if stride == 1 else ir_bwd_s2)(gd, dd, e, *cache.depthwise(dwc, dwbn)[:2])
    g = None
    if need_x_grad:
        g = _conv(lib, cache, ga, pw, cin, 1, tscale=pwbn, res=go if block.use_res_connect else res)
    if parts is not None:
        parts.update(e=e, d=dd, gd=gd, ga=ga)
    return g


def block_input_grad(block, x, grad_out, cache=None, parts=None):
    """The gradient with respect to the input `x` `[n,Cin,h,w]` of a FROZEN inverted-residual `block` (a `dwBlock` with an
    expand conv, stride 1 or 2, dilation 1, with or without the residual; eval mode, its BatchNorms folded), given `grad_out`
    `[n,Co,ho,wo]` = d loss / d output (`ho = (h-1)//stride+1`).  The frozen path beside `block_backward`, as
    `decoder_input_grad` is beside `decoder_backward`: `e` and `d` are recomputed by the forward's own launches, `gd` is one
    Co -> Ch GEMM with the transposed projection weights that carry s3, `ga` comes from `uavsal_ir_bwd` (stride 1) or
    `uavsal_ir_bwd_s2` (stride 2), and `grad_x` from one Ch -> Cin GEMM with the transposed expand weights that carry s1
    (+ `grad_out` with the residual).  No parameter gradient is computed and no `.grad` touched.  Accepted: Cin % 32 == 0,
    Ch % 64 == 0, Co % 32 == 0.  `parts` receives `e`, `d`, `gd`, `ga` (dense NHWC)."""
    lib = L.load()
    prt = _input_grad_parts(block)
    pw, pl, stride = prt[0], prt[4], prt[2].stride[0]
    cin, cout = pw.weight.shape[1], pl.weight.shape[0]
    xn = _nhwc(x, "x", cin)
    go = _block_grad_out(grad_out, xn, cout, stride)
    with torch.cuda.device(xn.device):
        cache = cache or WeightCache(xn.device, {})
        g = _input_grad(lib, cache, block, prt, xn, go, parts=parts)
    return g.permute(0, 3, 1, 2)
