"""The decoder `model.conv_out_st` behind the recurrence: frozen (`decoder_input_grad`; csrc/train.hip: `uavsal_dec_bwd`) or
the second stage, trained (`decoder_backward`, `decoder_param_grads`; csrc/train_decoder.hip: `uavsal_pix_gemm`,
`uavsal_dec_sums`, `uavsal_dec_finish`), its BatchNorms on their running statistics.
`recurrence_step(decoder=True)`: the decoder's nine parameters' `.grad` are set as well, or added to, and the recurrence
receives that path's `grad_h`; afterwards call `model.refresh_weights(model.rnn, model.conv_out_st)`.
`decoder_forward_batch` / `decoder_backward_batch` (csrc/train_bn.hip, train/bn.py) are the same block in TRAINING mode: the
BatchNorms on the statistics of the batch, the gradient through those statistics, the running statistics moved;
`recurrence_step(decoder=True, batch_stats=("decoder",))` with `model.conv_out_st.train()` under `model.eval()`."""
import ctypes as C

import torch

from .. import _lib as L
from ..ops import _stream
from ..weights import WeightCache
from ._common import _conv, _grad_slots, _nhwc, pix_gemm


def _decoder_parts(block, trained=False):
    seq = block.conv
    if getattr(block, "expand_ratio", 0) == 1 or len(seq) != 4 or seq[2].weight.shape[0] != 1:
        raise RuntimeError("decoder_input_grad takes model.conv_out_st (expand 1x1, depthwise 3x3, projection to one channel)")
    if block.training:
        raise RuntimeError("the decoder's BatchNorms use their running statistics: call model.eval()" if trained else
                           "the decoder is frozen: its BatchNorms are folded in eval mode (call model.eval())")
    return seq[0][0], seq[0][1], seq[1][0], seq[1][1], seq[2], seq[3]


def _decoder_recompute(lib, cache, block, h, y):
    """`e`, `d` (dense NHWC) from the NHWC `h` by the forward's own launches, and `y` dense `[T,h,w,1]` when it is not given
    (`[T,1,h,w]`); plus the packed `(wd9, s2, w3, s3)`."""
    pw, pwbn, dwc, dwbn, pl, plbn = _decoder_parts(block)
    T, hh, ww, _ = h.shape
    dev, hid = h.device, pw.weight.shape[0]
    st = _stream(h)
    e = _conv(lib, cache, h, pw, hid, 1, bn=pwbn, act=L.ACT_RELU6)
    w9, s2, b2 = cache.depthwise(dwc, dwbn)
    dd = torch.empty_like(e)
    q = L.DwDesc()
    q.inp, q.ldi, q.w9c, q.scale, q.bias = e.data_ptr(), hid, w9.data_ptr(), s2.data_ptr(), b2.data_ptr()
    q.out, q.ldo = dd.data_ptr(), hid
    q.n_img, q.H, q.W, q.C, q.stride, q.dilation, q.act = T, hh, ww, hid, 1, 1, L.ACT_RELU6
    L.check(lib.uavsal_dw3x3(C.byref(q), st), "uavsal_dw3x3")
    _, _, _, w3, s3, b3 = cache.dw_dot(dwc, dwbn, pl, plbn)
    if y is None:
        y = torch.empty((T, hh, ww, 1), dtype=torch.float32, device=dev)
        k = L.DwDotDesc()
        k.inp, k.ldi = e.data_ptr(), hid
        k.w9c, k.scale, k.bias, k.w2, k.scale2, k.bias2 = (t.data_ptr() for t in (w9, s2, b2, w3, s3, b3))
        k.out, k.ldo = y.data_ptr(), 1
        k.n_img, k.H, k.W, k.C, k.act = T, hh, ww, hid, L.ACT_SIGMOID
        L.check(lib.uavsal_dw3x3_dot(C.byref(k), st), "uavsal_dw3x3_dot")
    else:
        if tuple(y.shape) != (T, 1, hh, ww) or y.dtype != torch.float32 or y.device != dev:
            raise RuntimeError("y must be the prediction [%d,1,%d,%d] on the same device" % (T, hh, ww))
        y = y.detach().contiguous()
    return e, dd, y, (w9, s2, w3, s3)


def decoder_input_grad(block, h_seq, grad_out, cache=None, y=None, parts=None):
    """The gradient of the loss with respect to the recurrence output `h_seq` `[T,256,h,w]`, given `grad_out` `[T,1,h,w]` =
    d loss / d prediction, through the frozen decoder `block` = `model.conv_out_st` + sigmoid (model.py:372-373) with its
    eval BatchNorms folded.  `e` and `d` (the expanded and the depthwise tensor) are recomputed from `h_seq` by the forward's
    own launches, `uavsal_dec_bwd` goes back to `e` and a 1536 -> 256 GEMM with W1^T to `h`.
    `cache`: the `WeightCache` to take packed weights from (default: packed for this call); `y`: the prediction of the
    forward `[T,1,h,w]` (default: recomputed); `parts`: a dict that receives the intermediate NHWC tensors (tests)."""
    lib = L.load()
    pw, pwbn, dwc, dwbn, pl, plbn = _decoder_parts(block)
    h = _nhwc(h_seq, "h_seq", pw.weight.shape[1])
    T, hh, ww, _ = h.shape
    if (not torch.is_tensor(grad_out) or not grad_out.is_cuda or grad_out.dtype != torch.float32
            or tuple(grad_out.shape) != (T, 1, hh, ww)):
        raise RuntimeError("grad_out must be a float32 cuda tensor [%d,1,%d,%d]" % (T, hh, ww))
    dev = h.device
    hid = pw.weight.shape[0]
    with torch.cuda.device(dev):
        cache = cache or WeightCache(dev, {})
        e, dd, y, (w9, s2, w3, s3) = _decoder_recompute(lib, cache, block, h, y)
        ge = dec_bwd(grad_out, y, e, dd, cache.affine(pwbn, hid)[0], w9, s2, w3, s3)
        g = _conv(lib, cache, ge, pw, pw.weight.shape[1], 1, transposed=True)
        if parts is not None:
            parts.update(e=e, d=dd, y=y, ge=ge)
    return g.permute(0, 3, 1, 2)


def dec_bwd(grad_out, y, e, d, s1, wd9, s2, w3, s3):
    """`uavsal_dec_bwd` on the current stream: `grad_out` `[T,1,h,w]` (any strides), `y` dense `[T,h,w]` in any shape,
    `e`, `d` dense NHWC `[T,h,w,C]`, the folded scales and the tap-major depthwise weights on the device -> `ge` NHWC."""
    lib = L.load()
    T, hh, ww, c = e.shape
    if not (e.is_contiguous() and d.is_contiguous() and y.is_contiguous()) or e.shape != d.shape or y.numel() != T * hh * ww:
        raise RuntimeError("dec_bwd: e, d must be dense NHWC tensors of one shape and y dense [T,h,w]")
    ge = torch.empty_like(e)
    k = L.DecBwdDesc()
    k.gy = grad_out.data_ptr()
    k.gy_img_pitch, _, k.gy_row_pitch, k.gy_col_pitch = grad_out.stride()
    k.y, k.e, k.d, k.ge = y.data_ptr(), e.data_ptr(), d.data_ptr(), ge.data_ptr()
    k.s1, k.wd9, k.s2, k.w3, k.s3 = s1.data_ptr(), wd9.data_ptr(), s2.data_ptr(), w3.data_ptr(), s3.data_ptr()
    k.n_img, k.H, k.W, k.C = T, hh, ww, c
    L.check(lib.uavsal_dec_bwd(C.byref(k), _stream(e)), "uavsal_dec_bwd")
    return ge


DECODER_PARAMS = ("conv.0.0.weight", "conv.0.1.weight", "conv.0.1.bias", "conv.1.0.weight", "conv.1.1.weight", "conv.1.1.bias",
                  "conv.2.weight", "conv.3.weight", "conv.3.bias")      # W1, gamma1, beta1, Wd, gamma2, beta2, W3, gamma3, beta3


def dec_sums(grad_out, y, e, d, ga, w3, s3):
    """`uavsal_dec_sums` on the current stream -> `(ws, slabs)`: the per-slab partial sums (float64, the layout of
    include/uavsal_hip.h) that `uavsal_dec_finish` takes.  Arguments as `dec_bwd`'s; `ga` dense NHWC like `e`."""
    lib = L.load()
    T, hh, ww, c = e.shape
    if (not (e.is_contiguous() and d.is_contiguous() and ga.is_contiguous() and y.is_contiguous()) or e.shape != d.shape
            or e.shape != ga.shape or y.numel() != T * hh * ww):
        raise RuntimeError("dec_sums: e, d, ga must be dense NHWC tensors of one shape and y dense [T,h,w]")
    k = L.DecSumsDesc()
    k.gy = grad_out.data_ptr()
    k.gy_img_pitch, _, k.gy_row_pitch, k.gy_col_pitch = grad_out.stride()
    k.y, k.e, k.d, k.ga, k.w3, k.s3 = y.data_ptr(), e.data_ptr(), d.data_ptr(), ga.data_ptr(), w3.data_ptr(), s3.data_ptr()
    k.n_img, k.H, k.W, k.C = T, hh, ww, c
    nbytes = int(lib.uavsal_dec_sums_workspace_bytes(C.byref(k)))
    if nbytes <= 0:
        L.check(-3, "uavsal_dec_sums")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=e.device)
    k.ws, k.ws_bytes = ws.data_ptr(), nbytes
    L.check(lib.uavsal_dec_sums(C.byref(k), _stream(e)), "uavsal_dec_sums")
    return ws, int(lib.uavsal_dec_sums_slabs(C.byref(k)))


def _decoder_slots(block, out, accumulate):
    params = dict(block.named_parameters())
    if sorted(params) != sorted(DECODER_PARAMS):
        raise RuntimeError("the decoder's parameters must be %r" % (DECODER_PARAMS,))
    return params, _grad_slots({n: params[n] for n in DECODER_PARAMS}, out, accumulate, "out")


def decoder_param_grads(block, h, e, d, y, grad_out, ga=None, cache=None, out=None, accumulate=False):
    """The gradients of the nine parameters of the decoder `block` = `model.conv_out_st` (eval mode: the BatchNorms on their
    running statistics, which are not updated) from given tensors, teacher-forced: `h` `[T,256,h,w]` the block's input,
    `e`, `d` dense NHWC `[T,h,w,1536]` its expanded and depthwise tensors, `y` `[T,1,h,w]` the prediction, `grad_out`
    `[T,1,h,w]` = d loss / d y, `ga` dense NHWC = d loss / d a1 (default: one `uavsal_dec_bwd` with ones for s1).  Returns a
    dict keyed by the block's parameter names (`DECODER_PARAMS`), the values `torch.autograd` gives for the reference's
    `dwBlock` (include/uavsal_hip.h states the formulas); `out`: such a dict of dense tensors to write into, or
    (`accumulate`) to add to.  Nothing of the forward is recomputed; four launches (GEMM, its reduction, channel sums,
    finalise) on the current stream, no synchronisation."""
    lib = L.load()
    pw, pwbn, dwc, dwbn, pl, plbn = _decoder_parts(block, trained=True)
    hn = _nhwc(h, "h", pw.weight.shape[1])
    T, hh, ww, _ = hn.shape
    hid = pw.weight.shape[0]
    dev = hn.device
    for name, t in (("e", e), ("d", d)) + ((("ga", ga),) if ga is not None else ()):
        if (not torch.is_tensor(t) or t.dtype != torch.float32 or t.device != dev or tuple(t.shape) != (T, hh, ww, hid)
                or not t.is_contiguous()):
            raise RuntimeError("%s must be a dense float32 NHWC tensor [%d,%d,%d,%d] on the device" % (name, T, hh, ww, hid))
    if (not torch.is_tensor(grad_out) or grad_out.device != dev or grad_out.dtype != torch.float32
            or tuple(grad_out.shape) != (T, 1, hh, ww)):
        raise RuntimeError("grad_out must be a float32 cuda tensor [%d,1,%d,%d]" % (T, hh, ww))
    if not torch.is_tensor(y) or y.dtype != torch.float32 or y.device != dev or y.numel() != T * hh * ww:
        raise RuntimeError("y must be the prediction [%d,1,%d,%d] on the same device" % (T, hh, ww))
    params, out = _decoder_slots(block, out, accumulate)
    if any(q.device != dev or not q.is_contiguous() for q in params.values()):
        raise RuntimeError("the decoder's parameters must be dense tensors on the device of `h`")
    with torch.cuda.device(dev):
        cache = cache or WeightCache(dev, {})
        y = y.detach().contiguous()
        w9, s2, _ = cache.depthwise(dwc, dwbn)
        _, _, _, w3, s3, _ = cache.dw_dot(dwc, dwbn, pl, plbn)
        s1 = cache.affine(pwbn, hid)[0]
        if ga is None:
            ga = dec_bwd(grad_out, y, e, d, torch.ones(hid, dtype=torch.float32, device=dev), w9, s2, w3, s3)
        (r1, mu1), (r2, mu2), (r3, mu3) = (cache.bn_stats(b) for b in (pwbn, dwbn, plbn))
        rowdot = torch.empty(hid, dtype=torch.float64, device=dev)
        pix_gemm(ga, hn, out=out[DECODER_PARAMS[0]], row_scale=s1, w=pw.weight.detach(), rowdot=rowdot, accumulate=accumulate)
        ws, slabs = dec_sums(grad_out, y, e, d, ga, w3, s3)
        k = L.DecFinishDesc()
        k.ws, k.ws_bytes, k.rowdot = ws.data_ptr(), ws.numel() * 8, rowdot.data_ptr()
        k.wd, k.w3, k.s2, k.s3 = dwc.weight.data_ptr(), pl.weight.data_ptr(), s2.data_ptr(), s3.data_ptr()
        k.r1, k.mu1, k.r2, k.mu2, k.r3, k.mu3 = (t.data_ptr() for t in (r1, mu1, r2, mu2, r3, mu3))
        (k.g_gamma1, k.g_beta1, k.g_wd, k.g_gamma2, k.g_beta2, k.g_w3, k.g_gamma3, k.g_beta3) = (
            out[n].data_ptr() for n in DECODER_PARAMS[1:])
        k.C, k.slabs, k.accumulate = hid, slabs, int(bool(accumulate))
        L.check(lib.uavsal_dec_finish(C.byref(k), _stream(hn)), "uavsal_dec_finish")
    return out


def decoder_backward(block, h_seq, grad_out, cache=None, y=None, parts=None, grads=None, accumulate=False):
    """`decoder_input_grad` for a decoder that is TRAINED: returns `(grad_h [T,256,h,w], grads)` with `grads` the dict of
    `decoder_param_grads` (written into `grads`, or with `accumulate` added to it, when given).  `e` and `d` are recomputed
    from `h_seq` by the forward's own launches, `ga` = d loss / d a1 comes from `uavsal_dec_bwd` handed ones for s1, and
    `grad_h = ga . (diag(s1) W1)` from one 1536 -> 256 GEMM whose transposed weights carry s1 in their rows
    (`WeightCache.conv_t_scaled`) -- the gamma gradients need the unscaled `ga`.  `decoder_input_grad` scales by s1 in the
    kernel and multiplies by the plain W1^T instead: the two paths round in a different order and may differ in the last
    bits of `grad_h`.  `parts` receives `e`, `d`, `y`, `ga` (dense NHWC).  A block in training mode raises: the BatchNorms use
    their running statistics (which are not updated), as everywhere in this package."""
    lib = L.load()
    pw, pwbn, dwc, dwbn, pl, plbn = _decoder_parts(block, trained=True)
    h = _nhwc(h_seq, "h_seq", pw.weight.shape[1])
    T, hh, ww, _ = h.shape
    if (not torch.is_tensor(grad_out) or not grad_out.is_cuda or grad_out.dtype != torch.float32
            or tuple(grad_out.shape) != (T, 1, hh, ww)):
        raise RuntimeError("grad_out must be a float32 cuda tensor [%d,1,%d,%d]" % (T, hh, ww))
    dev = h.device
    hid = pw.weight.shape[0]
    _decoder_slots(block, grads, accumulate)                          # raise before anything is launched
    with torch.cuda.device(dev):
        cache = cache or WeightCache(dev, {})
        e, dd, y, (w9, s2, w3, s3) = _decoder_recompute(lib, cache, block, h, y)
        ga = dec_bwd(grad_out, y, e, dd, torch.ones(hid, dtype=torch.float32, device=dev), w9, s2, w3, s3)
        g = _conv(lib, cache, ga, pw, pw.weight.shape[1], 1, tscale=pwbn)
        grads = decoder_param_grads(block, h.permute(0, 3, 1, 2), e, dd, y, grad_out, ga=ga, cache=cache, out=grads,
                                    accumulate=accumulate)
        if parts is not None:
            parts.update(e=e, d=dd, y=y, ga=ga)
    return g.permute(0, 3, 1, 2), grads


# ---------------------------------------------------------------------------------------------- batch statistics (training mode)
_BATCH_REFUSAL = ("decoder_forward_batch / decoder_backward_batch run the decoder's BatchNorms on BATCH statistics: call "
                  "block.train() (model.conv_out_st.train() under model.eval()); a block in eval mode goes through the eval-mode "
                  "functions decoder_backward, decoder_input_grad and decoder_param_grads")


def _decoder_parts_batch(block, who):
    seq = block.conv
    if getattr(block, "expand_ratio", 0) == 1 or len(seq) != 4 or seq[2].weight.shape[0] != 1:
        raise RuntimeError("%s takes model.conv_out_st (expand 1x1, depthwise 3x3, projection to one channel)" % who)
    bns = (seq[0][1], seq[1][1], seq[3])
    if not block.training or not all(b.training for b in bns):
        raise RuntimeError(_BATCH_REFUSAL)
    if not all(b.track_running_stats and b.affine and b.running_mean is not None for b in bns):
        raise RuntimeError("%s needs affine BatchNorms that track their running statistics" % who)
    return seq[0][0], bns[0], seq[1][0], bns[1], seq[2], bns[2]


def _dw_raw(lib, x, w9):
    """The raw depthwise 3x3 of the dense NHWC `x` with the tap-major weights `w9`: `uavsal_dw3x3` with unit scale, zero bias
    and no activation."""
    T, hh, ww, c = x.shape
    out = torch.empty_like(x)
    one, zero = torch.ones(c, dtype=torch.float32, device=x.device), torch.zeros(c, dtype=torch.float32, device=x.device)
    q = L.DwDesc()
    q.inp, q.ldi, q.w9c, q.scale, q.bias = x.data_ptr(), c, w9.data_ptr(), one.data_ptr(), zero.data_ptr()
    q.out, q.ldo = out.data_ptr(), c
    q.n_img, q.H, q.W, q.C, q.stride, q.dilation, q.act = T, hh, ww, c, 1, 1, L.ACT_NONE
    L.check(lib.uavsal_dw3x3(C.byref(q), _stream(x)), "uavsal_dw3x3")
    return out


def decoder_forward_batch(block, h_seq, update_running=True, parts=None, cache=None):
    """The decoder `block` = `model.conv_out_st` + sigmoid in TRAINING mode, torch's rules for `nn.BatchNorm2d`: every
    BatchNorm normalises with the statistics of all `T*h*w` pixels of `h_seq` `[T,256,h,w]` together.  Returns
    `(y [T,1,h,w], saved)`; `saved` holds what `decoder_backward_batch` needs: the raw `u1 = W1 h`, `u2 = dw3x3(Wd, e)`,
    `u3 = w3 . d` and `e = ReLU6(BN1(u1))` (dense NHWC; `d` is never stored: the projection reads `u2`) and the three
    `bn.BnFold`s `f1`, `f2`, `f3` (batch mean, biased variance, r and the fold s, b).  `update_running` (default): the running
    statistics of the three BatchNorms move on the device as torch moves them (momentum, unbiased variance) and
    `num_batches_tracked` goes up by one -- afterwards `model.refresh_weights(model.conv_out_st)` refolds the eval-mode packed
    forms from them.  Launches: the 256 -> 1536 GEMM, then per BatchNorm `uavsal_bn_stats` (two) and `uavsal_bn_apply` (one),
    with `uavsal_dw3x3` between the first two; no synchronisation.  A block in eval mode raises.  `parts` receives `saved`."""
    from . import bn as B
    lib = L.load()
    pw, bn1, dwc, bn2, pl, bn3 = _decoder_parts_batch(block, "decoder_forward_batch")
    h = _nhwc(h_seq, "h_seq", pw.weight.shape[1])
    T, hh, ww, _ = h.shape
    dev, hid = h.device, pw.weight.shape[0]
    if update_running and any(b.momentum is None for b in (bn1, bn2, bn3)):
        raise RuntimeError("decoder_forward_batch: momentum=None (the cumulative average) is not covered")

    def stats(u, b):
        run = (b.running_mean, b.running_var) if update_running else (None, None)
        f = B.bn_stats(u, b.weight, b.bias, b.eps, *run, momentum=b.momentum)
        if update_running:
            b.num_batches_tracked.add_(1)
        return f
    with torch.cuda.device(dev):
        cache = cache or WeightCache(dev, {})
        u1 = _conv(lib, cache, h, pw, hid, 1)
        f1 = stats(u1, bn1)
        e = B.bn_apply(u1, f1, "relu6")
        u2 = _dw_raw(lib, e, cache.depthwise(dwc, bn2)[0])
        f2 = stats(u2, bn2)
        u3 = B.bn_apply(u2, f2, "relu6", dot_w=pl.weight.detach().reshape(-1))
        f3 = stats(u3, bn3)
        y = B.bn_apply(u3, f3, "sigmoid")
    saved = dict(u1=u1, e=e, u2=u2, u3=u3, f1=f1, f2=f2, f3=f3)
    if parts is not None:
        parts.update(saved)
    return y.view(T, 1, hh, ww), saved


def decoder_backward_batch(block, h_seq, grad_out, saved=None, grads=None, accumulate=False, parts=None, cache=None):
    """The backward of `decoder_forward_batch`: returns `(grad_h [T,256,h,w], grads)`, `grads` keyed by the nine names of
    `DECODER_PARAMS`, the values `torch.autograd` gives for the reference's `dwBlock` in `.train()` mode + sigmoid -- the
    gradient flows through the batch statistics: per BatchNorm `g_u = s (g_a - d beta / P - xh d gamma / P)` -- written into
    `grads`, or with `accumulate` added to it, as `decoder_backward` does.  `grad_out` `[T,1,h,w]` = d loss / d y; `saved`:
    what the forward returned for this `h_seq` (default: the forward is run again WITHOUT moving the running statistics).
    BN3, then BN2, then BN1: `uavsal_bn_bwd_sums` and `uavsal_bn_bwd_apply` each (the adjoint of the projection is formed
    inside BN2's launches, which also give W3's gradient), `uavsal_dw_wgrad` and the flipped `uavsal_dw3x3` between BN2 and
    BN1, `uavsal_pix_gemm` for W1 and one transposed GEMM for `grad_h`.  The ReLU6 masks and xh come from the stored raw
    `u1`, `u2`.  A block in eval mode raises.  `parts` receives `g_u1`, `g_u2`, `g_u3`, `g_e` (dense NHWC)."""
    from . import bn as B
    lib = L.load()
    pw, bn1, dwc, bn2, pl, bn3 = _decoder_parts_batch(block, "decoder_backward_batch")
    h = _nhwc(h_seq, "h_seq", pw.weight.shape[1])
    T, hh, ww, _ = h.shape
    if (not torch.is_tensor(grad_out) or not grad_out.is_cuda or grad_out.dtype != torch.float32
            or tuple(grad_out.shape) != (T, 1, hh, ww)):
        raise RuntimeError("grad_out must be a float32 cuda tensor [%d,1,%d,%d]" % (T, hh, ww))
    dev, hid = h.device, pw.weight.shape[0]
    params, grads = _decoder_slots(block, grads, accumulate)          # raises before anything is launched
    if any(q.device != dev or not q.is_contiguous() for q in params.values()):
        raise RuntimeError("the decoder's parameters must be dense tensors on the device of `h_seq`")
    N = DECODER_PARAMS
    with torch.cuda.device(dev):
        cache = cache or WeightCache(dev, {})
        if saved is None:
            _, saved = decoder_forward_batch(block, h_seq, update_running=False, cache=cache)
        u1, e, u2, u3, f1, f2, f3 = (saved[k] for k in ("u1", "e", "u2", "u3", "f1", "f2", "f3"))
        if tuple(u1.shape) != (T, hh, ww, hid) or tuple(u3.shape) != (T, hh, ww, 1):
            raise RuntimeError("saved does not belong to this h_seq")
        gy = grad_out.detach().contiguous().view(T, hh, ww, 1)
        w3 = pl.weight.detach().reshape(-1)
        s3 = B.bn_bwd_sums(gy, u3, f3, "sigmoid", g_weight=grads[N[7]], g_bias=grads[N[8]], accumulate=accumulate)
        g_u3 = B.bn_bwd_apply(gy, u3, f3, s3, "sigmoid")
        g2 = (g_u3, w3)
        s2 = B.bn_bwd_sums(g2, u2, f2, "relu6", g_weight=grads[N[4]], g_bias=grads[N[5]], g_w=grads[N[6]], accumulate=accumulate)
        g_u2 = B.bn_bwd_apply(g2, u2, f2, s2, "relu6")
        B.dw_wgrad(g_u2, e, out=grads[N[3]], accumulate=accumulate)
        g_e = _dw_raw(lib, g_u2, cache.depthwise(dwc, bn2)[0].flip(0).contiguous())
        s1 = B.bn_bwd_sums(g_e, u1, f1, "relu6", g_weight=grads[N[1]], g_bias=grads[N[2]], accumulate=accumulate)
        g_u1 = B.bn_bwd_apply(g_e, u1, f1, s1, "relu6")
        pix_gemm(g_u1, h, out=grads[N[0]], accumulate=accumulate)
        g = _conv(lib, cache, g_u1, pw, pw.weight.shape[1], 1, transposed=True)
        if parts is not None:
            parts.update(g_u1=g_u1, g_u2=g_u2, g_u3=g_u3, g_e=g_e)
    return g.permute(0, 3, 1, 2), grads
