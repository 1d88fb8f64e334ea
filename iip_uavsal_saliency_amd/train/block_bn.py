"""An inverted-residual block (`dwBlock` with an expand conv, stride 1, dilation 1, with or without the residual) in TRAINING
mode: its three BatchNorms on the statistics of the batch, the gradient through those statistics, the running statistics moved
-- torch's rules for `nn.BatchNorm2d.train()`, composed from the per-BatchNorm launches of train/bn.py (csrc/train_bn.hip) the
way decoder.py composes the decoder's:

    u1 = W1 x                e = ReLU6(BN1(u1))
    u2 = dw3x3(Wd, e)        d = ReLU6(BN2(u2))
    u3 = W3 d                out = BN3(u3) (+ x with the residual)

with the fold `a = fma(u, s, b)` everywhere.  The one launch composition cannot express is the residual behind BN3:
`uavsal_bn_apply_res`.  `recurrence_step(fuse=True, block_stats=("fuse",))` runs the fusion block in front of the recurrence
this way (`train.fuse_block`); a block in eval mode goes through block.py."""
import torch

from .. import _lib as L
from ..weights import WeightCache
from . import bn as B
from ._common import _block_grad_out, _conv, _nhwc, pix_gemm
from .block import BLOCK_PARAMS, _block_slots, _checked_parts
from .decoder import _dw_raw


def block_forward_batch(block, x, update_running=True, parts=None, cache=None):
    """`block` (a `dwBlock` with an expand conv, stride 1, dilation 1; Cin % 64 == 0, hidden % 64 == 0, Cout % 128 == 0 --
    `block_backward`'s shapes) in TRAINING mode on `x` `[T,Cin,h,w]`: every BatchNorm normalises with the statistics of all
    `T*h*w` pixels together.  Returns `(out [T,Co,h,w], saved)`; `saved` holds what `block_backward_batch` needs: the raw
    `u1`, `u2`, `u3`, the activated `e`, `d` (dense NHWC) and the three `bn.BnFold`s `f1`, `f2`, `f3`.  `update_running`
    (default): the running statistics of the three BatchNorms move on the device as torch moves them (momentum, unbiased
    variance) and `num_batches_tracked` goes up by one -- afterwards `model.refresh_weights(<the block's container>)` refolds
    the eval-mode packed forms from them.  Launches: the raw expand GEMM, per BatchNorm `uavsal_bn_stats` (two) and
    `uavsal_bn_apply` (one; BN3 with the residual: `uavsal_bn_apply_res`), the raw `uavsal_dw3x3` and the raw projection GEMM
    between them; no synchronisation, two calls return the same bits.  A block in eval mode raises.  `parts` receives `saved`."""
    lib = L.load()
    pw, bn1, dwc, bn2, pl, bn3 = _checked_parts(block, "block_batch")
    hid, cin, cout = pw.weight.shape[0], pw.weight.shape[1], pl.weight.shape[0]
    xn = _nhwc(x, "x", cin)
    dev = xn.device
    if update_running and any(b.momentum is None for b in (bn1, bn2, bn3)):
        raise RuntimeError("block_forward_batch: momentum=None (the cumulative average) is not covered")

    def stats(u, b):
        run = (b.running_mean, b.running_var) if update_running else (None, None)
        f = B.bn_stats(u, b.weight, b.bias, b.eps, *run, momentum=b.momentum)
        if update_running:
            b.num_batches_tracked.add_(1)
        return f
    with torch.cuda.device(dev):
        cache = cache or WeightCache(dev, {})
        u1 = _conv(lib, cache, xn, pw, hid, 1)
        f1 = stats(u1, bn1)
        e = B.bn_apply(u1, f1, "relu6")
        u2 = _dw_raw(lib, e, cache.depthwise(dwc, bn2)[0])
        f2 = stats(u2, bn2)
        d = B.bn_apply(u2, f2, "relu6")
        u3 = _conv(lib, cache, d, pl, cout, 1)
        f3 = stats(u3, bn3)
        out = B.bn_apply(u3, f3, None, res=xn if block.use_res_connect else None)
    saved = dict(u1=u1, e=e, u2=u2, d=d, u3=u3, f1=f1, f2=f2, f3=f3)
    if parts is not None:
        parts.update(saved)
    return out.permute(0, 3, 1, 2), saved


def block_backward_batch(block, x, grad_out, saved=None, need_x_grad=True, grads=None, accumulate=False, parts=None, cache=None):
    """The backward of `block_forward_batch`: returns `(grad_x [T,Cin,h,w] | None, grads)`, `grads` keyed by the nine names of
    `BLOCK_PARAMS`, the values `torch.autograd` gives for the reference's `dwBlock` in `.train()` mode -- per BatchNorm
    `g_u = s (g_a - d beta / P - xh d gamma / P)` -- written into `grads`, or with `accumulate` added to it, as
    `block_backward` does.  `grad_out` `[T,Co,h,w]` = d loss / d output; `saved`: what the forward returned for this `x`
    (default: the forward is run again WITHOUT moving the running statistics).  BN3 (no activation, `g = grad_out`), then BN2,
    then BN1: `uavsal_bn_bwd_sums` and `uavsal_bn_bwd_apply` each; `dW3 = pix_gemm(g_u3, d)`, `g_d` one GEMM with the plain
    W3^T, `dWd = uavsal_dw_wgrad(g_u2, e)`, `g_e` the flipped raw `uavsal_dw3x3`, `dW1 = pix_gemm(g_u1, x)`, and
    `grad_x = g_u1 . W1` (+ `grad_out` with the residual, the GEMM's residual operand) unless `need_x_grad` is False.  The
    ReLU6 masks and xh come from the stored raw `u1`, `u2`.  No atomics: a second call returns the same bits.  A block in
    eval mode raises.  `parts` receives `g_u1`, `g_u2`, `g_u3`, `g_e`, `g_d` (dense NHWC)."""
    lib = L.load()
    pw, bn1, dwc, bn2, pl, bn3 = _checked_parts(block, "block_batch")
    hid, cin, cout = pw.weight.shape[0], pw.weight.shape[1], pl.weight.shape[0]
    xn = _nhwc(x, "x", cin)
    T, hh, ww, _ = xn.shape
    go = _block_grad_out(grad_out, xn, cout)
    dev = xn.device
    params, grads = _block_slots(block, grads, accumulate)            # raises before anything is launched
    if any(q.device != dev or not q.is_contiguous() for q in params.values()):
        raise RuntimeError("the block's parameters must be dense tensors on the device of `x`")
    N = BLOCK_PARAMS
    with torch.cuda.device(dev):
        cache = cache or WeightCache(dev, {})
        if saved is None:
            _, saved = block_forward_batch(block, x, update_running=False, cache=cache)
        u1, e, u2, d, u3, f1, f2, f3 = (saved[k] for k in ("u1", "e", "u2", "d", "u3", "f1", "f2", "f3"))
        if tuple(u1.shape) != (T, hh, ww, hid) or tuple(u3.shape) != (T, hh, ww, cout):
            raise RuntimeError("saved does not belong to this x")
        s3 = B.bn_bwd_sums(go, u3, f3, None, g_weight=grads[N[7]], g_bias=grads[N[8]], accumulate=accumulate)
        g_u3 = B.bn_bwd_apply(go, u3, f3, s3, None)
        pix_gemm(g_u3, d, out=grads[N[6]], accumulate=accumulate)
        g_d = _conv(lib, cache, g_u3, pl, hid, 1, transposed=True)
        s2 = B.bn_bwd_sums(g_d, u2, f2, "relu6", g_weight=grads[N[4]], g_bias=grads[N[5]], accumulate=accumulate)
        g_u2 = B.bn_bwd_apply(g_d, u2, f2, s2, "relu6")
        B.dw_wgrad(g_u2, e, out=grads[N[3]], accumulate=accumulate)
        g_e = _dw_raw(lib, g_u2, cache.depthwise(dwc, bn2)[0].flip(0).contiguous())
        s1 = B.bn_bwd_sums(g_e, u1, f1, "relu6", g_weight=grads[N[1]], g_bias=grads[N[2]], accumulate=accumulate)
        g_u1 = B.bn_bwd_apply(g_e, u1, f1, s1, "relu6")
        pix_gemm(g_u1, xn, out=grads[N[0]], accumulate=accumulate)
        g = None
        if need_x_grad:
            g = _conv(lib, cache, g_u1, pw, cin, 1, transposed=True, res=go if block.use_res_connect else None)
        if parts is not None:
            parts.update(g_u1=g_u1, g_u2=g_u2, g_u3=g_u3, g_e=g_e, g_d=g_d)
    return (g.permute(0, 3, 1, 2) if need_x_grad else None), grads
