"""The gauss / ob prior nets `model.gauss_cb_layer` / `model.ob_cb_layer`, the sixth stage and the last the reference trains
(`prior_net_backward`; csrc/train_nets.hip): block 1 of either is a shape the walk of block.py takes, block 0 (8 -> 48 -> 64,
20 -> 120 -> 64) is too narrow for those kernels and goes through `narrow_block_param_grads` (`uavsal_ir_narrow_grads`,
`uavsal_ir_narrow_finish`, and `uavsal_frame_sum` for priors that are one map for every frame).
`recurrence_step(nets=True)` (needs `fuse=True` and a gauss or ob prior; independent of `fust` and `ctx`): with it, the step
sets the gradients of every parameter the reference's optimiser holds by default (`sfnet` and `st_layer` are frozen there:
Demo_Train_Test.py:58-62).  The walk of ctx.py hands out `g_cb` = d loss / d `cb192`, whose gauss and ob slices are the nets'
output gradients; `prior_net_backward` forms each net's 18 parameter gradients (`.grad` set, or added to).  Static priors --
decided exactly as the forward decides them, `model.dedupe_priors and model._static(cb0, cb1, 1)` with more than one frame --
ran each net on ONE frame whose output every frame reads: the slice is summed over the frames (`frame_sum`) and the backward
runs on one frame too; else it runs over all N frames.  Refresh `model.gauss_cb_layer` / `model.ob_cb_layer` afterwards as
well (which also drops the engines' prior records, `model.refresh_weights`)."""
import ctypes as C

import torch

from .. import _lib as L
from ..ops import _nhwc_view, _stream, to_nhwc
from ..weights import WeightCache
from ._common import _block_grad_out, _conv, _dense_nhwc, _nhwc
from .block import (BLOCK_PARAMS, _block_recompute, _block_slots, _input_grad, _input_grad_parts, _param_grad_parts,
                    block_param_grads, ir_bwd)

PRIOR_NETS = ("gauss_cb_layer", "ob_cb_layer")                       # in concat order


def _narrow_parts(block):
    """`(pw, pwbn, dwc, dwbn, pl, plbn)` of a narrow inverted-residual block `narrow_block_param_grads` covers, or a
    RuntimeError."""
    seq = getattr(block, "conv", None)
    if (seq is None or getattr(block, "expand_ratio", 1) == 1 or len(seq) != 4 or getattr(block, "stride", None) != 1
            or getattr(block, "dilation", None) != 1 or seq[1][0].stride != (1, 1) or seq[1][0].dilation != (1, 1)):
        raise RuntimeError("narrow_block_param_grads takes a dwBlock with an expand conv, stride 1 and dilation 1 "
                           "(expand 1x1, depthwise 3x3, projection 1x1)")
    pw, pwbn, dwc, dwbn, pl, plbn = seq[0][0], seq[0][1], seq[1][0], seq[1][1], seq[2], seq[3]
    hid, cin, cout = pw.weight.shape[0], pw.weight.shape[1], pl.weight.shape[0]
    if cin % 4 or cin > 32 or hid % 4 or hid > 128 or cout != 64:
        raise RuntimeError("narrow_block_param_grads needs Cin %% 4 == 0 and Cin <= 32, hidden %% 4 == 0 and hidden <= 128 and "
                           "Cout == 64, got %d -> %d -> %d" % (cin, hid, cout))
    if block.use_res_connect:
        raise RuntimeError("narrow_block_param_grads: a block with the residual is not covered (block_param_grads takes 64 -> 384 -> 64)")
    if block.training:
        raise RuntimeError("the block's BatchNorms use their running statistics: call model.eval()")
    return pw, pwbn, dwc, dwbn, pl, plbn


def ir_narrow_grads(x, e, d, gd, ga, go):
    """`uavsal_ir_narrow_grads` on the current stream -> `(ws, slabs)`: the per-slab partials (float64, the layout of
    include/uavsal_hip.h) that `uavsal_ir_narrow_finish` takes.  `x` dense NHWC `[n,h,w,Cin]`; `e`, `d`, `gd`, `ga` dense NHWC
    `[n,h,w,Ch]`; `go` an NHWC view `[n,h,w,64]` of the same pixels (a channel slice is read in place)."""
    lib = L.load()
    _dense_nhwc("ir_narrow_grads", "x, e, d, gd, ga", x, e, d, gd, ga)
    n, hh, ww, c = e.shape
    if (any(t.shape != e.shape or t.device != e.device for t in (d, gd, ga)) or tuple(x.shape[:3]) != (n, hh, ww)
            or x.device != e.device):
        raise RuntimeError("ir_narrow_grads: e, d, gd, ga must have one shape [n,h,w,Ch] and x cover the same pixels, on one device")
    if not torch.is_tensor(go) or go.dtype != torch.float32 or go.device != e.device:
        raise RuntimeError("ir_narrow_grads: go must be a float32 tensor on the device of e")
    gp, ldgo, *gs = _nhwc_view(go)
    if gs[:3] != [n, hh, ww]:
        raise RuntimeError("ir_narrow_grads: go must cover the pixels of e")
    k = L.IrNarrowDesc()
    k.x, k.e, k.d, k.gd, k.ga, k.go, k.ldgo = x.data_ptr(), e.data_ptr(), d.data_ptr(), gd.data_ptr(), ga.data_ptr(), gp, ldgo
    k.n_img, k.H, k.W, k.Cin, k.Ch, k.Co = n, hh, ww, x.shape[3], c, gs[3]
    nbytes = int(lib.uavsal_ir_narrow_workspace_bytes(C.byref(k)))
    if nbytes <= 0:
        L.check(-3, "uavsal_ir_narrow_grads")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=e.device)
    k.ws, k.ws_bytes = ws.data_ptr(), nbytes
    L.check(lib.uavsal_ir_narrow_grads(C.byref(k), _stream(e)), "uavsal_ir_narrow_grads")
    return ws, int(lib.uavsal_ir_narrow_slabs(C.byref(k)))


def narrow_block_param_grads(block, x, e, d, grad_out, gd=None, ga=None, cache=None, out=None, accumulate=False):
    """`block_param_grads` for a NARROW inverted-residual `block` (block 0 of a prior net: 8 -> 48 -> 64, 20 -> 120 -> 64): the
    gradients of its nine parameters from given tensors, teacher-forced, with the same arguments, the same dict
    (`BLOCK_PARAMS`) and the same `out` / `accumulate` rule.  Accepted: stride 1, dilation 1, no residual, eval mode,
    Cin % 4 == 0 and Cin <= 32, hidden % 4 == 0 and hidden <= 128, Cout == 64.  `gd` defaults to the one 64 -> Ch 1x1 conv with
    the projection's transposed weights carrying s3, `ga` to one `uavsal_ir_bwd`.  Nothing of the forward is recomputed; TWO
    launches (`uavsal_ir_narrow_grads`: every product and sum of the block in one pass over the pixels; `uavsal_ir_narrow_finish`)
    where `block_param_grads` takes six, on the current stream, no synchronisation."""
    lib = L.load()
    pw, pwbn, dwc, dwbn, pl, plbn = _narrow_parts(block)
    hid, cin, cout = pw.weight.shape[0], pw.weight.shape[1], pl.weight.shape[0]
    xn = _nhwc(x, "x", cin).contiguous()
    T, hh, ww, _ = xn.shape
    dev = xn.device
    for name, t in (("e", e), ("d", d)) + tuple((n, t) for n, t in (("gd", gd), ("ga", ga)) if t is not None):
        if (not torch.is_tensor(t) or t.dtype != torch.float32 or t.device != dev or tuple(t.shape) != (T, hh, ww, hid)
                or not t.is_contiguous()):
            raise RuntimeError("%s must be a dense float32 NHWC tensor [%d,%d,%d,%d] on the device" % (name, T, hh, ww, hid))
    go = _block_grad_out(grad_out, xn, cout)
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
            ga = ir_bwd(gd, d, e, w9, s2)
        (r1, mu1), (r2, mu2), (r3, mu3) = (cache.bn_stats(b) for b in (pwbn, dwbn, plbn))
        ws, slabs = ir_narrow_grads(xn, e, d, gd, ga, go)
        k = L.IrNarrowFinishDesc()
        k.ws, k.ws_bytes = ws.data_ptr(), ws.numel() * 8
        k.w1, k.wd, k.w3 = pw.weight.data_ptr(), dwc.weight.data_ptr(), pl.weight.data_ptr()
        k.s1, k.s2, k.s3 = s1.data_ptr(), s2.data_ptr(), s3.data_ptr()
        k.r1, k.mu1, k.r2, k.mu2, k.r3, k.mu3 = (t.data_ptr() for t in (r1, mu1, r2, mu2, r3, mu3))
        (k.g_w1, k.g_gamma1, k.g_beta1, k.g_wd, k.g_gamma2, k.g_beta2, k.g_w3, k.g_gamma3, k.g_beta3) = (
            out[n].data_ptr() for n in BLOCK_PARAMS)
        k.Cin, k.Ch, k.Co, k.slabs, k.accumulate = cin, hid, cout, slabs, int(bool(accumulate))
        L.check(lib.uavsal_ir_narrow_finish(C.byref(k), _stream(xn)), "uavsal_ir_narrow_finish")
    return out


def frame_sum(a):
    """`uavsal_frame_sum` on the current stream: `a` an NHWC view `[N,h,w,C]` (a channel slice is read in place) ->
    `[1,h,w,C]` dense, the sum over the frames in frame order in double, rounded once (`N = 1`: the input's bits)."""
    lib = L.load()
    ap, lda, n, hh, ww, c = _nhwc_view(a)
    out = torch.empty((1, hh, ww, c), dtype=torch.float32, device=a.device)
    k = L.FrameSumDesc()
    k.a, k.lda, k.out, k.ldo, k.N, k.HW, k.C = ap, lda, out.data_ptr(), c, n, hh * ww, c
    L.check(lib.uavsal_frame_sum(C.byref(k), _stream(a)), "uavsal_frame_sum")
    return out


def prior_nets(model):
    """`{name: net}` of the prior nets `model` has (`gauss_cb_layer`, `ob_cb_layer`), in concat order."""
    return {n: getattr(model, n) for n, on in zip(PRIOR_NETS, (getattr(model, "use_gauss_prior", 0), getattr(model, "use_ob_prior", 0)))
            if on}


def _prior_net_blocks(net):
    if not isinstance(net, torch.nn.Sequential) or len(net) != 2:
        raise RuntimeError("prior_net_backward takes model.gauss_cb_layer or model.ob_cb_layer (two dwBlocks)")
    return net[0], net[1]


def prior_net_backward(net, cb, grad_out, cache=None, parts=None, grads=None, accumulate=False):
    """Backward of a prior net that is TRAINED: `net` = `model.gauss_cb_layer` or `model.ob_cb_layer` (two `dwBlock`s: the
    narrow block 0, then 64 -> 384 -> 64 with the residual), `cb` `[Np,8|20,h,w]` the caller's prior (NCHW, as the forward
    takes it), `grad_out` an NHWC view `[Np,h,w,64]` = d loss / d the net's output (the net's slice of `g_cb` is read in
    place).  Block 0's `e`, `d` and output are recomputed by the forward's own launches (the layout launch, expand conv and
    depthwise, the projection); block 1 goes through the walk of `block_input_grad` and `block_param_grads`, block 0 through
    its `gd` GEMM, `uavsal_ir_bwd` and `narrow_block_param_grads`.  The priors are data: no input gradient is formed.  Nothing
    of the forward is recomputed twice.  Returns `{"0": {...}, "1": {...}}`, each block's nine gradients keyed by
    `BLOCK_PARAMS`, written into `grads` of that form (a block's entry None: allocated) or with `accumulate` (a bool, or a dict
    of bools by block name) added to it.  `parts` receives per block `name: dict(x=, go=, e=, d=, gd=, ga=)` (NHWC)."""
    lib = L.load()
    b0, b1 = _prior_net_blocks(net)
    p0 = _narrow_parts(b0)
    _param_grad_parts(b1)
    p1 = _input_grad_parts(b1)
    cin = p0[0].weight.shape[1]
    if (not torch.is_tensor(cb) or not cb.is_cuda or cb.dtype != torch.float32 or cb.dim() != 4 or cb.shape[1] != cin):
        raise RuntimeError("cb must be a float32 cuda tensor [n,%d,h,w] (no CPU fallback)" % cin)
    n, _, hh, ww = cb.shape
    if (not torch.is_tensor(grad_out) or grad_out.dtype != torch.float32 or grad_out.device != cb.device
            or tuple(grad_out.shape) != (n, hh, ww, 64)):
        raise RuntimeError("grad_out must be a float32 NHWC view [%d,%d,%d,64] on the device of cb" % (n, hh, ww))
    grads = dict(grads) if grads is not None else {"0": None, "1": None}
    if sorted(grads) != ["0", "1"]:
        raise RuntimeError("grads must be {'0': dict | None, '1': dict | None}")
    acc = {k: (accumulate[k] if isinstance(accumulate, dict) else accumulate) for k in grads}
    for k, b in (("0", b0), ("1", b1)):
        _block_slots(b, grads[k], acc[k])                     # raise before anything is launched
    nchw = lambda t: t.permute(0, 3, 1, 2)                                # noqa: E731
    with torch.cuda.device(cb.device):
        cache = cache or WeightCache(cb.device, {})
        x0 = to_nhwc(cb)
        e0, d0 = _block_recompute(lib, cache, b0, x0, 1, p0)
        mid = _conv(lib, cache, d0, p0[4], 64, 1, bn=p0[5])
        pt = {}
        g_mid = _input_grad(lib, cache, b1, p1, mid, grad_out, parts=pt)
        grads["1"] = block_param_grads(b1, nchw(mid), pt["e"], pt["d"], nchw(grad_out), gd=pt["gd"], ga=pt["ga"], cache=cache,
                                       out=grads["1"], accumulate=acc["1"])
        hid = p0[0].weight.shape[0]
        gd0 = _conv(lib, cache, g_mid, p0[4], hid, 1, tscale=p0[5])
        ga0 = ir_bwd(gd0, d0, e0, *cache.depthwise(p0[2], p0[3])[:2])
        grads["0"] = narrow_block_param_grads(b0, nchw(x0), e0, d0, nchw(g_mid), gd=gd0, ga=ga0, cache=cache, out=grads["0"],
                                              accumulate=acc["0"])
        if parts is not None:
            parts["1"] = dict(pt, x=mid, go=grad_out)
            parts["0"] = dict(x=x0, go=g_mid, e=e0, d=d0, gd=gd0, ga=ga0)
    return grads
