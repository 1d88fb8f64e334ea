"""The decoder `model.conv_out_st` behind the recurrence: frozen (`decoder_input_grad`; csrc/train.hip: `uavsal_dec_bwd`) or
the second stage, trained (`decoder_backward`, `decoder_param_grads`; csrc/train_decoder.hip: `uavsal_pix_gemm`,
`uavsal_dec_sums`, `uavsal_dec_finish`), its BatchNorms on their running statistics.
`recurrence_step(decoder=True)`: the decoder's nine parameters' `.grad` are set as well, or added to, and the recurrence
receives that path's `grad_h`; afterwards call `model.refresh_weights(model.rnn, model.conv_out_st)`."""
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
