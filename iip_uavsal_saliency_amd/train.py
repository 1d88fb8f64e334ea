"""Fine-tuning the Temporal Weighted Average recurrence (`model.rnn`, reference model_convlstm.py:238-295) on the device.

This is ONE stage of the reference's `train()` (Demo_Train_Test.py:35-174): the loss gradient is carried through the
frozen decoder `conv_out_st` and back through time over the ConvTWA steps to the recurrence's only parameter, the
`[256, 512, 3, 3]` weight `W = [W_x | W_h]` of `rnn_conv`, and to the recurrence's input.  Everything else stays frozen
and in eval mode -- a deliberate difference from the reference, whose `train()` also trains `fust_layer`, the prior nets
and the decoder and runs every BatchNorm on batch statistics.  The recurrence has no BatchNorm and no
bias, so ITS gradient is the same in both modes.

    z_t = conv3x3(W, cat[x_t, h_{t-1}]),   i_t = sigmoid(z_t),   h_t = i_t x_t + (1 - i_t) h_{t-1}

A second stage can be trained with it: the decoder `model.conv_out_st` (`decoder_backward`, `decoder_param_grads`,
`recurrence_step(decoder=True)`; csrc/train_decoder.hip: `uavsal_pix_gemm`, `uavsal_dec_sums`, `uavsal_dec_finish`), its
BatchNorms on their running statistics.  A third one as well: the fusion block that produces the recurrence's input
(`fuse_block`: `model.fucbst_layer[0]`, or `model.fust_layer[0]` without priors), through the backward of a general
inverted-residual block (`block_backward`, `block_param_grads`, `recurrence_step(fuse=True)`; csrc/train_block.hip:
`uavsal_ir_bwd`, `uavsal_ir_sums`, `uavsal_ir_finish`, and `uavsal_pix_gemm` for both 1x1 weight gradients).  A fourth one
in a model with priors: `model.fust_layer[0]` behind them (`recurrence_step(fust=True)`), whose output gradient comes
through the fusion block's input directly and through the frozen context-prior path (`fust_output_grad`,
`block_input_grad`; csrc/train_ctx.hip: `uavsal_ir_bwd_s2`, `uavsal_bilinear_ac_bwd`, `uavsal_tsum_bwd`).  And a fifth: that
path itself, `model.fucb_layer[0]` and the two stride-2 blocks of `model.cxt_cb_prior` (`recurrence_step(ctx=True)`): the one
walk `prior_path_backward` hands each block's tensors to `block_param_grads`, which takes 64 output channels (`uavsal_pix_gemm`
with M a multiple of 64) and stride 2 (`uavsal_ir_sums_s2`).  And a sixth, the last the reference trains: the gauss / ob prior
nets `model.gauss_cb_layer` / `model.ob_cb_layer` (`recurrence_step(nets=True)`, `prior_net_backward`): block 1 of either is a
shape the walk above takes, block 0 (8 -> 48 -> 64, 20 -> 120 -> 64) goes through `narrow_block_param_grads`
(csrc/train_nets.hip: `uavsal_ir_narrow_grads`, `uavsal_ir_narrow_finish`, and `uavsal_frame_sum` for priors that are one map
for every frame).  With all six, a step sets the gradient of every parameter the reference's optimiser holds by default
(`sfnet` and `st_layer` are frozen there: Demo_Train_Test.py:58-62).  And a seventh, what deleting the reference's lines 61-62
gives: the ST blocks `model.st_layer` (`recurrence_step(st=True)`, `st_block_backward`): the two inverted-residual blocks of an
ST block go through the walks above (`block_param_grads` takes the temporal sub-block's 64 -> 384 -> 32, `uavsal_pix_gemm` its
32-wide side), the three 1x1 conv + BatchNorm + ReLU6 stages through `cbr_backward` and the temporal difference through
`tdiff_bwd` (csrc/train_st.hip: `uavsal_cbr_sums`, `uavsal_cbr_finish`, `uavsal_tdiff_bwd`).  And an eighth: the head of the backbone
`sfnet` -- everything in it the reference initialises itself (`recurrence_step(srf=True)`, `srf_head`, `srf_head_backward`): its 1x1
stages go through `cbr_backward`, its dilated ASPP branches through `block_param_grads` (csrc/train_srf.hip: `uavsal_ir_bwd_dil`,
`uavsal_ir_sums_dil`) and the dense 3x3 `conv_last` through `conv3_backward` (`uavsal_conv3_wgrad`).  And a ninth: the deep
backbone, MobileNetV2 `features[8:18]` (`recurrence_step(backbone=True)`, `backbone_blocks`, `backbone_backward`): the head also
hands out the gradients of its `c4` / `c5` taps and the ten blocks at 1/16 and 1/32 resolution go through `block_backward(
backbone=True)` (their widths are multiples of 32: `uavsal_pix_gemm` with `tails32`).  And a tenth: the shallow backbone,
`features[2:8]` (`recurrence_step(shallow=True)`, `shallow_blocks`, `shallow_backward`; csrc/train_shallow.hip): the head also
hands out the gradient of its `c3` tap, the ninth stage that of block 7's output, and the six blocks at 1/4 to 1/16 resolution go
through `block_backward(shallow=True)` (widths of 16 to 192: `skinny_wgrad` for the weight gradients `uavsal_pix_gemm` refuses,
the channel sums with their Ch % 16 opt-in).  Only the stem and `features[1]` stay frozen; BatchNorm in eval mode remains the
documented difference.

The second model, `UAVSAL_LSTM` (the reference's ConvLSTM ablation, model_convlstm.py:111-126: `cc_t = conv3x3(W, cat[x_t, h_{t-1}])`,
`i, f, o = sigmoid`, `g = tanh`, `c_t = f c_{t-1} + i g`, `h_t = o tanh(c_t)`; `W` `[1024,512,3,3]`), is trained through the same step
with `recurrence_step(lstm=True)`: `lstm_backward` stands where `twa_backward` stands (csrc/train_lstm.hip: `uavsal_lstm_scan` recomputes
the cell-state history in one launch, `uavsal_lstm_gate_bwd` is one step of the walk; the weight gradient is `uavsal_conv3_wgrad` at
1024 x 512), and every stage above works unchanged behind it -- they hang off the recurrence's `grad_x` and `grad_h`.

New launches (csrc/train.hip): `uavsal_dec_bwd`, `uavsal_twa_gate_bwd`, `uavsal_twa_wgrad`; (csrc/train_lstm.hip): `uavsal_lstm_scan`,
`uavsal_lstm_gate_bwd`.  Everything else is one
`uavsal_conv_gemm` / `uavsal_dw3x3` call each, routed by the library's own table, with repacked weights.
Tensors are float32 on the GPU with the logical shape `[T, C, h, w]`; a channels-last tensor (NHWC in memory, or a channel
slice of one) is read in place, anything else is copied once.  Returned gradients are channels-last.  `f32` only; one
sequence per call.  CPU tensors raise: this package has no CPU fallback."""
from __future__ import annotations

import ctypes as C
import types

import torch

from . import _lib as L
from . import packing as P
from .ops import _nhwc_view, _stream
from .ops import tsum as _tsum
from .weights import WeightCache

HID = 256


def _nhwc(t, name, c=None):
    """`t` `[n,c,h,w]` as an NHWC view `[n,h,w,c]` the kernels can read (a copy only when its memory is not NHWC)."""
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4:
        raise RuntimeError("%s must be a float32 cuda tensor [n,c,h,w] (no CPU fallback)" % name)
    if c is not None and t.shape[1] != c:
        raise RuntimeError("%s must have %d channels, got %r" % (name, c, tuple(t.shape)))
    v = t.detach().permute(0, 2, 3, 1)
    try:
        p, ld, *_ = _nhwc_view(v)
        if p % 16 == 0 and ld % 4 == 0:
            return v
    except RuntimeError:
        pass
    return v.contiguous()


def _conv(lib, cache, x, conv, cout, taps, wslice=None, transposed=False, bn=None, act=L.ACT_NONE, res=None, tscale=None):
    """One `uavsal_conv_gemm` launch on the current stream (no synchronisation): `x` NHWC, the weights of `conv` (or of its
    transposed conv; `tscale`: with the folded scale of that BatchNorm in its rows) from `cache` in the layout the route of
    this launch takes."""
    ap, lda, n, h, w, cin = _nhwc_view(x)
    out = torch.empty((n, h, w, cout), dtype=torch.float32, device=x.device)
    d = L.ConvDesc()
    d.a, d.lda, d.a_img_stride = ap, lda, h * w
    d.out, d.ldc, d.o_img_stride = out.data_ptr(), cout, h * w
    if bn is not None:
        s, b = cache.affine(bn, cout)
        d.scale, d.bias = s.data_ptr(), b.data_ptr()
    if res is not None:
        rp, ldr, *_ = _nhwc_view(res)
        d.res, d.ldr, d.r_img_stride = rp, ldr, h * w
    d.n_img, d.H, d.W, d.Cin, d.Cout, d.taps = n, h, w, cin, cout, taps
    d.prec, d.act, d.epi, d.tile = L.PREC["f32"], act, L.EPI_AFFINE, 0
    d.w = 1 << 20
    rt = L.conv_route(lib, d)
    layout = P.conv_weight_layout("f32", False, False, rt.tile, 3 if taps == 9 else 1)
    if tscale is not None:
        wp = cache.conv_t_scaled(conv, tscale, layout)
    else:
        wp = cache.conv_t(conv, wslice, layout) if transposed else cache.conv(conv, wslice, 0, layout)
    d.w = wp.data_ptr()
    L.check(lib.uavsal_conv_gemm(C.byref(d), _stream(x)), "uavsal_conv_gemm")
    return out


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


def pix_gemm(a, b, out=None, row_scale=None, w=None, rowdot=None, accumulate=False, tails32=False):
    """`uavsal_pix_gemm` on the current stream: `a` `[..., M]`, `b` `[..., N]` NHWC tensors of the same pixels (channel slices
    are read in place) -> `out[m][n] = row_scale[m] sum_p a[p][m] b[p][n]` (dense `[M, N]`; `accumulate`: added to `out`), and
    with `w` `[M, N]` and `rowdot` (float64 `[M]`) `rowdot[m] = sum_n w[m][n] G[m][n]`.  Two launches, no synchronisation.
    `tails32=True`: every M, N multiple of 32 the default call refuses is taken too (the weight gradients of the backbone
    blocks: quarter-tile tails, shares of 128-pixel units; include/uavsal_hip.h); what the default takes keeps its bits."""
    lib = L.load()
    ap, lda, *sa = _nhwc_view(a)
    bp, ldb, *sb = _nhwc_view(b)
    M, N = sa[3], sb[3]
    if sa[:3] != sb[:3] or a.device != b.device:
        raise RuntimeError("pix_gemm: a and b must cover the same pixels on one device")
    dev = a.device
    if out is None:
        if accumulate:
            raise RuntimeError("accumulate needs `out`")
        out = torch.empty((M, N), dtype=torch.float32, device=dev)
    if out.numel() != M * N or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
        raise RuntimeError("out must be a dense float32 tensor of %d x %d elements on the device" % (M, N))
    k = L.PixGemmDesc()
    k.a, k.lda, k.b, k.ldb = ap, lda, bp, ldb
    k.K, k.M, k.N, k.accumulate = sa[0] * sa[1] * sa[2], M, N, int(bool(accumulate))
    k.tails32 = int(bool(tails32))
    if row_scale is not None:
        if row_scale.dtype != torch.float32 or row_scale.device != dev or row_scale.numel() < M or not row_scale.is_contiguous():
            raise RuntimeError("row_scale must be a dense float32 vector of at least %d elements on the device" % M)
        k.row_scale = row_scale.data_ptr()
    if rowdot is not None:
        if (w is None or w.numel() != M * N or not w.is_contiguous() or w.dtype != torch.float32 or w.device != dev
                or rowdot.dtype != torch.float64 or rowdot.numel() != M or not rowdot.is_contiguous() or rowdot.device != dev):
            raise RuntimeError("rowdot needs a dense float32 `w` of %d x %d elements and a dense float64 [%d] on the device" % (M, N, M))
        k.w, k.ldw, k.rowdot = w.data_ptr(), N, rowdot.data_ptr()
    k.out, k.ldo = out.data_ptr(), N
    nbytes = int(lib.uavsal_pix_gemm_workspace_bytes(C.byref(k)))
    if nbytes <= 0:
        L.check(-3, "uavsal_pix_gemm")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    k.ws, k.ws_bytes = ws.data_ptr(), nbytes
    L.check(lib.uavsal_pix_gemm(C.byref(k), _stream(a)), "uavsal_pix_gemm")
    return out


def skinny_wgrad(a, b, out=None, row_scale=None, w=None, rowdot=None, accumulate=False):
    """`uavsal_skinny_wgrad` on the current stream: `pix_gemm`'s arguments and results for the skinny products it refuses,
    M and N multiples of 8 with `min(M, N) <= 32` and `max(M, N) <= 192` (the 1x1 weight gradients of MobileNetV2
    `features[2:8]`: 96 x 16, 144 x 24, 24 x 96, 24 x 144, 32 x 144).  One pass over both operands, a wave per share of the
    pixels (csrc/train_shallow.hip; the partition is stated in include/uavsal_hip.h).  Two launches, no synchronisation."""
    lib = L.load()
    ap, lda, *sa = _nhwc_view(a)
    bp, ldb, *sb = _nhwc_view(b)
    M, N = sa[3], sb[3]
    if sa[:3] != sb[:3] or a.device != b.device:
        raise RuntimeError("skinny_wgrad: a and b must cover the same pixels on one device")
    dev = a.device
    if out is None:
        if accumulate:
            raise RuntimeError("accumulate needs `out`")
        out = torch.empty((M, N), dtype=torch.float32, device=dev)
    if out.numel() != M * N or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
        raise RuntimeError("out must be a dense float32 tensor of %d x %d elements on the device" % (M, N))
    k = L.SkinnyWgradDesc()
    k.a, k.lda, k.b, k.ldb = ap, lda, bp, ldb
    k.K, k.M, k.N, k.accumulate = sa[0] * sa[1] * sa[2], M, N, int(bool(accumulate))
    if row_scale is not None:
        if row_scale.dtype != torch.float32 or row_scale.device != dev or row_scale.numel() < M or not row_scale.is_contiguous():
            raise RuntimeError("row_scale must be a dense float32 vector of at least %d elements on the device" % M)
        k.row_scale = row_scale.data_ptr()
    if rowdot is not None:
        if (w is None or w.numel() != M * N or not w.is_contiguous() or w.dtype != torch.float32 or w.device != dev
                or rowdot.dtype != torch.float64 or rowdot.numel() != M or not rowdot.is_contiguous() or rowdot.device != dev):
            raise RuntimeError("rowdot needs a dense float32 `w` of %d x %d elements and a dense float64 [%d] on the device" % (M, N, M))
        k.w, k.ldw, k.rowdot = w.data_ptr(), N, rowdot.data_ptr()
    k.out, k.ldo = out.data_ptr(), N
    nbytes = int(lib.uavsal_skinny_wgrad_workspace_bytes(C.byref(k)))
    if nbytes <= 0:
        L.check(-3, "uavsal_skinny_wgrad")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    k.ws, k.ws_bytes = ws.data_ptr(), nbytes
    with torch.cuda.device(dev):
        L.check(lib.uavsal_skinny_wgrad(C.byref(k), _stream(a)), "uavsal_skinny_wgrad")
    return out


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


def _grad_tensors(block, out, accumulate):
    params = dict(block.named_parameters())
    if sorted(params) != sorted(DECODER_PARAMS):
        raise RuntimeError("the decoder's parameters must be %r" % (DECODER_PARAMS,))
    if out is None:
        if accumulate:
            raise RuntimeError("accumulate needs `out`")
        out = {n: torch.empty_like(params[n], memory_format=torch.contiguous_format) for n in DECODER_PARAMS}
    for n in DECODER_PARAMS:
        t, q = out.get(n), params[n]
        if (not torch.is_tensor(t) or t.shape != q.shape or t.dtype != torch.float32 or t.device != q.device
                or not t.is_contiguous()):
            raise RuntimeError("out[%r] must be a dense float32 tensor of the parameter's shape on its device" % n)
    return params, out


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
    params, out = _grad_tensors(block, out, accumulate)
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
    _grad_tensors(block, grads, accumulate)                          # raise before anything is launched
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


BLOCK_PARAMS = DECODER_PARAMS                                        # a dwBlock with an expand conv: the same nine names


def _block_parts(block, backbone=False, shallow=False):
    """`(pw, pwbn, dwc, dwbn, pl, plbn)` of an inverted-residual block the block backward covers, or a RuntimeError.
    `backbone`: the shapes of MobileNetV2 `features[8:18]` instead, `shallow`: those of `features[2:8]` (`_param_grad_parts`)."""
    if backbone or shallow:
        return _param_grad_parts(block, backbone, shallow)
    seq = getattr(block, "conv", None)
    if (seq is None or getattr(block, "expand_ratio", 1) == 1 or len(seq) != 4 or getattr(block, "stride", None) != 1
            or getattr(block, "dilation", None) != 1 or seq[1][0].stride != (1, 1) or seq[1][0].dilation != (1, 1)):
        raise RuntimeError("block_backward takes a dwBlock with an expand conv, stride 1 and dilation 1 "
                           "(expand 1x1, depthwise 3x3, projection 1x1)")
    pw, pwbn, dwc, dwbn, pl, plbn = seq[0][0], seq[0][1], seq[1][0], seq[1][1], seq[2], seq[3]
    hid, cin, cout = pw.weight.shape[0], pw.weight.shape[1], pl.weight.shape[0]
    if cout % 128 or hid % 64 or cin % 64:
        raise RuntimeError("block_backward needs Cout %% 128 == 0, hidden %% 64 == 0 and Cin %% 64 == 0, got %d -> %d -> %d"
                           % (cin, hid, cout))
    if block.training:
        raise RuntimeError("the block's BatchNorms use their running statistics: call model.eval()")
    return pw, pwbn, dwc, dwbn, pl, plbn


def _param_grad_parts(block, backbone=False, shallow=False):
    """`(pw, pwbn, dwc, dwbn, pl, plbn)` of an inverted-residual block whose nine gradients `block_param_grads` forms: what
    `_block_parts` takes, and stride 2 and Cout % 64 == 0 besides (the blocks of the multi-prior path), or a RuntimeError.
    `backbone`: Cin % 32 == 0, hidden % 64 == 0, Cout % 32 == 0 at dilation 1 instead, stride 1 (with or without the residual)
    or 2 -- MobileNetV2 `features[8:18]`.  `model_feature.InvertedResidual` and `dwBlock` are the same module to this code:
    the same `conv` Sequential, the same nine parameter names (`BLOCK_PARAMS`), which is checked here.
    `shallow`: Cin % 8 == 0, hidden % 16 == 0, Cout % 8 == 0 at dilation 1, stride 1 or 2, an expand conv present -- MobileNetV2
    `features[2:8]` (16 -> 96 -> 24, 24 -> 144 -> 24 / 32, 32 -> 192 -> 32 / 64); it takes what `backbone` takes as well."""
    seq = getattr(block, "conv", None)
    stride = getattr(block, "stride", None)
    dil = getattr(block, "dilation", None)
    if shallow:
        if (seq is None or getattr(block, "expand_ratio", 1) == 1 or len(seq) != 4
                or tuple(n for n, _ in block.named_parameters()) != BLOCK_PARAMS):
            raise RuntimeError("the shallow backward takes an inverted-residual block with an expand conv (expand 1x1, depthwise "
                               "3x3, projection 1x1: features[2..17]), not features[1] or the stem")
        if stride not in (1, 2) or dil != 1 or seq[1][0].stride != (stride, stride) or seq[1][0].dilation != (1, 1):
            raise RuntimeError("the shallow backward takes stride 1 or 2 at dilation 1 (a dilated block with stride 2 is not covered)")
        pw, pwbn, dwc, dwbn, pl, plbn = seq[0][0], seq[0][1], seq[1][0], seq[1][1], seq[2], seq[3]
        hid, cin, cout = pw.weight.shape[0], pw.weight.shape[1], pl.weight.shape[0]
        if cout % 8 or hid % 16 or cin % 8:
            raise RuntimeError("the shallow backward needs Cout %% 8 == 0, hidden %% 16 == 0 and Cin %% 8 == 0, got %d -> %d -> %d"
                               % (cin, hid, cout))
        if block.training:
            raise RuntimeError("the block's BatchNorms use their running statistics: call model.eval()")
        return pw, pwbn, dwc, dwbn, pl, plbn
    if backbone:
        if (seq is None or getattr(block, "expand_ratio", 1) == 1 or len(seq) != 4
                or tuple(n for n, _ in block.named_parameters()) != BLOCK_PARAMS):
            raise RuntimeError("the backbone backward takes an inverted-residual block with an expand conv (expand 1x1, depthwise "
                               "3x3, projection 1x1: features[2..17]), not features[1] or the stem")
        if stride not in (1, 2) or dil != 1 or seq[1][0].stride != (stride, stride) or seq[1][0].dilation != (1, 1):
            raise RuntimeError("the backbone backward takes stride 1 or 2 at dilation 1 (a dilated block with stride 2 is not covered)")
        pw, pwbn, dwc, dwbn, pl, plbn = seq[0][0], seq[0][1], seq[1][0], seq[1][1], seq[2], seq[3]
        hid, cin, cout = pw.weight.shape[0], pw.weight.shape[1], pl.weight.shape[0]
        if cout % 32 or hid % 64 or cin % 32:
            raise RuntimeError("the backbone backward needs Cout %% 32 == 0, hidden %% 64 == 0 and Cin %% 32 == 0, got %d -> %d -> %d"
                               % (cin, hid, cout))
        if block.training:
            raise RuntimeError("the block's BatchNorms use their running statistics: call model.eval()")
        return pw, pwbn, dwc, dwbn, pl, plbn
    if (seq is None or getattr(block, "expand_ratio", 1) == 1 or len(seq) != 4 or stride not in (1, 2)
            or not isinstance(dil, int) or dil < 1 or (dil > 1 and stride != 1)
            or seq[1][0].stride != (stride, stride) or seq[1][0].dilation != (dil, dil)):
        raise RuntimeError("block_param_grads takes a dwBlock with an expand conv, stride 1 or 2 and dilation 1, or stride 1 and "
                           "a dilation above 1 (expand 1x1, depthwise 3x3, projection 1x1)")
    pw, pwbn, dwc, dwbn, pl, plbn = seq[0][0], seq[0][1], seq[1][0], seq[1][1], seq[2], seq[3]
    hid, cin, cout = pw.weight.shape[0], pw.weight.shape[1], pl.weight.shape[0]
    if dil > 1 and cout % 128:                                      # the ASPP branches of the SRF-Net head: 320 -> 1920 -> 256
        raise RuntimeError("block_param_grads takes a dilated block with Cout %% 128 == 0 only, got %d -> %d -> %d, dilation %d"
                           % (cin, hid, cout, dil))
    narrow = cout == 32 and 128 <= hid <= 512                       # an ST block's sub_conv, 64 -> 384 -> 32 (uavsal_pix_gemm's 32-wide side)
    if (cout % 64 and not narrow) or hid % 64 or cin % 64:
        raise RuntimeError("block_param_grads needs Cout %% 64 == 0 (or Cout == 32 with 128 <= hidden <= 512), hidden %% 64 == 0 "
                           "and Cin %% 64 == 0, got %d -> %d -> %d" % (cin, hid, cout))
    if stride == 2 and block.use_res_connect:
        raise RuntimeError("block_param_grads: a block with stride 2 has no residual")
    if block.training:
        raise RuntimeError("the block's BatchNorms use their running statistics: call model.eval()")
    return pw, pwbn, dwc, dwbn, pl, plbn


def _block_grad_out(grad_out, x, cout, stride=1):
    T, hh, ww, _ = x.shape
    hh, ww = (hh - 1) // stride + 1, (ww - 1) // stride + 1
    if (not torch.is_tensor(grad_out) or not grad_out.is_cuda or grad_out.dtype != torch.float32 or grad_out.device != x.device
            or tuple(grad_out.shape) != (T, cout, hh, ww)):
        raise RuntimeError("grad_out must be a float32 cuda tensor [%d,%d,%d,%d]" % (T, cout, hh, ww))
    return _nhwc(grad_out, "grad_out", cout)


def _block_grad_tensors(block, out, accumulate):
    params = dict(block.named_parameters())
    if sorted(params) != sorted(BLOCK_PARAMS):
        raise RuntimeError("the block's parameters must be %r" % (BLOCK_PARAMS,))
    if out is None:
        if accumulate:
            raise RuntimeError("accumulate needs `out`")
        out = {n: torch.empty_like(params[n], memory_format=torch.contiguous_format) for n in BLOCK_PARAMS}
    for n in BLOCK_PARAMS:
        t, q = out.get(n), params[n]
        if (not torch.is_tensor(t) or t.shape != q.shape or t.dtype != torch.float32 or t.device != q.device
                or not t.is_contiguous()):
            raise RuntimeError("out[%r] must be a dense float32 tensor of the parameter's shape on its device" % n)
    return params, out


def ir_bwd(gd, d, e, wd9, s2):
    """`uavsal_ir_bwd` on the current stream: `gd`, `d`, `e` dense NHWC `[T,h,w,C]`, the tap-major depthwise weights and the
    folded scale of the depthwise BatchNorm on the device -> `ga` = d loss / d a1, dense NHWC."""
    lib = L.load()
    if (not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.is_contiguous()
                for t in (gd, d, e)) or gd.shape != d.shape or e.shape != d.shape):
        raise RuntimeError("ir_bwd: gd, d, e must be dense float32 NHWC cuda tensors of one shape")
    T, hh, ww, c = e.shape
    for name, t, n in (("wd9", wd9, 9 * c), ("s2", s2, c)):
        if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.device == e.device and t.is_contiguous() and t.numel() >= n):
            raise RuntimeError("ir_bwd: %s must be a dense float32 tensor of at least %d elements on the device of e" % (name, n))
    ga = torch.empty_like(e)
    k = L.IrBwdDesc()
    k.gd, k.d, k.e, k.wd9, k.s2, k.ga = gd.data_ptr(), d.data_ptr(), e.data_ptr(), wd9.data_ptr(), s2.data_ptr(), ga.data_ptr()
    k.n_img, k.H, k.W, k.C = T, hh, ww, c
    L.check(lib.uavsal_ir_bwd(C.byref(k), _stream(e)), "uavsal_ir_bwd")
    return ga


def ir_sums(gd, d, e, ga, go, ch16=False):
    """`uavsal_ir_sums` on the current stream -> `(ws, slabs)`: the per-slab partial sums (float64, the layout of
    include/uavsal_hip.h) that `uavsal_ir_finish` takes.  `gd`, `d`, `e`, `ga` dense NHWC `[T,h,w,Ch]`; `go` an NHWC view
    `[T,h,w,Co]` of the same pixels (a channel slice is read in place).  `ch16=True`: any Ch % 16 == 0 is taken, not only
    Ch % 64 == 0 (the descriptor's opt-in; `ir_finish(..., ch16=True)` takes the workspace)."""
    lib = L.load()
    if (not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.is_contiguous()
                for t in (gd, d, e, ga)) or not all(t.shape == e.shape and t.device == e.device for t in (gd, d, ga))):
        raise RuntimeError("ir_sums: gd, d, e, ga must be dense float32 NHWC cuda tensors of one shape on one device")
    T, hh, ww, c = e.shape
    if not torch.is_tensor(go) or go.dtype != torch.float32 or go.device != e.device:
        raise RuntimeError("ir_sums: go must be a float32 tensor on the device of e")
    gp, ldgo, *gs = _nhwc_view(go)
    if gs[:3] != [T, hh, ww]:
        raise RuntimeError("ir_sums: go must cover the pixels of e")
    k = L.IrSumsDesc()
    k.gd, k.d, k.e, k.ga, k.go, k.ldgo = gd.data_ptr(), d.data_ptr(), e.data_ptr(), ga.data_ptr(), gp, ldgo
    k.n_img, k.H, k.W, k.Ch, k.Co, k.ch16 = T, hh, ww, c, gs[3], int(bool(ch16))
    nbytes = int(lib.uavsal_ir_sums_workspace_bytes(C.byref(k)))
    if nbytes <= 0:
        L.check(-3, "uavsal_ir_sums")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=e.device)
    k.ws, k.ws_bytes = ws.data_ptr(), nbytes
    L.check(lib.uavsal_ir_sums(C.byref(k), _stream(e)), "uavsal_ir_sums")
    return ws, int(lib.uavsal_ir_sums_slabs(C.byref(k)))


def ir_sums_s2(gd, d, e, ga, go, ch16=False):
    """`uavsal_ir_sums_s2` on the current stream -> `(ws, slabs)`: `ir_sums` for a depthwise 3x3 with stride 2, in the same
    workspace layout.  `e`, `ga` dense NHWC `[n,H,W,Ch]`; `gd`, `d` dense NHWC `[n,Ho,Wo,Ch]` with `Ho = (H-1)//2+1`,
    `Wo = (W-1)//2+1`; `go` an NHWC view `[n,Ho,Wo,Co]` (a channel slice is read in place).  `ch16`: as in `ir_sums`."""
    lib = L.load()
    _dense_nhwc("ir_sums_s2", "gd, d, e, ga", gd, d, e, ga)
    n, hh, ww, c = e.shape
    ho, wo = (hh - 1) // 2 + 1, (ww - 1) // 2 + 1
    if (ga.shape != e.shape or gd.shape != d.shape or tuple(d.shape) != (n, ho, wo, c)
            or any(t.device != e.device for t in (gd, d, ga))):
        raise RuntimeError("ir_sums_s2: gd and d must be [n,(H-1)//2+1,(W-1)//2+1,Ch] for e and ga [n,H,W,Ch], on one device")
    if not torch.is_tensor(go) or go.dtype != torch.float32 or go.device != e.device:
        raise RuntimeError("ir_sums_s2: go must be a float32 tensor on the device of e")
    gp, ldgo, *gs = _nhwc_view(go)
    if gs[:3] != [n, ho, wo]:
        raise RuntimeError("ir_sums_s2: go must cover the pixels of d")
    k = L.IrSumsS2Desc()
    k.gd, k.d, k.e, k.ga, k.go, k.ldgo = gd.data_ptr(), d.data_ptr(), e.data_ptr(), ga.data_ptr(), gp, ldgo
    k.n_img, k.H, k.W, k.Ch, k.Co, k.ch16 = n, hh, ww, c, gs[3], int(bool(ch16))
    nbytes = int(lib.uavsal_ir_sums_s2_workspace_bytes(C.byref(k)))
    if nbytes <= 0:
        L.check(-3, "uavsal_ir_sums_s2")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=e.device)
    k.ws, k.ws_bytes = ws.data_ptr(), nbytes
    L.check(lib.uavsal_ir_sums_s2(C.byref(k), _stream(e)), "uavsal_ir_sums_s2")
    return ws, int(lib.uavsal_ir_sums_s2_slabs(C.byref(k)))


def ir_bwd_dil(gd, d, e, wd9, s2, dil):
    """`uavsal_ir_bwd_dil` on the current stream: `ir_bwd` for a depthwise 3x3 with stride 1 and dilation `dil` >= 1 (the ASPP
    branches of the SRF-Net head): `gd`, `d`, `e` dense NHWC `[T,h,w,C]` -> `ga` = d loss / d a1, dense NHWC."""
    lib = L.load()
    _dense_nhwc("ir_bwd_dil", "gd, d, e", gd, d, e)
    if gd.shape != d.shape or e.shape != d.shape or any(t.device != e.device for t in (gd, d)):
        raise RuntimeError("ir_bwd_dil: gd, d, e must have one shape on one device")
    if not isinstance(dil, int) or dil < 1:
        raise RuntimeError("ir_bwd_dil: the dilation must be an integer >= 1, got %r" % (dil,))
    T, hh, ww, c = e.shape
    for name, t, n in (("wd9", wd9, 9 * c), ("s2", s2, c)):
        if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.device == e.device and t.is_contiguous() and t.numel() >= n):
            raise RuntimeError("ir_bwd_dil: %s must be a dense float32 tensor of at least %d elements on the device of e" % (name, n))
    ga = torch.empty_like(e)
    k = L.IrBwdDilDesc()
    k.gd, k.d, k.e, k.wd9, k.s2, k.ga = gd.data_ptr(), d.data_ptr(), e.data_ptr(), wd9.data_ptr(), s2.data_ptr(), ga.data_ptr()
    k.n_img, k.H, k.W, k.C, k.dil = T, hh, ww, c, dil
    L.check(lib.uavsal_ir_bwd_dil(C.byref(k), _stream(e)), "uavsal_ir_bwd_dil")
    return ga


def ir_sums_dil(gd, d, e, ga, go, dil):
    """`uavsal_ir_sums_dil` on the current stream -> `(ws, slabs)`: `ir_sums` for a depthwise 3x3 with stride 1 and dilation
    `dil` >= 1, in the same workspace layout.  `gd`, `d`, `e`, `ga` dense NHWC `[T,h,w,Ch]`; `go` an NHWC view `[T,h,w,Co]` of
    the same pixels (a channel slice is read in place)."""
    lib = L.load()
    _dense_nhwc("ir_sums_dil", "gd, d, e, ga", gd, d, e, ga)
    if not all(t.shape == e.shape and t.device == e.device for t in (gd, d, ga)):
        raise RuntimeError("ir_sums_dil: gd, d, e, ga must have one shape on one device")
    if not isinstance(dil, int) or dil < 1:
        raise RuntimeError("ir_sums_dil: the dilation must be an integer >= 1, got %r" % (dil,))
    T, hh, ww, c = e.shape
    if not torch.is_tensor(go) or go.dtype != torch.float32 or go.device != e.device:
        raise RuntimeError("ir_sums_dil: go must be a float32 tensor on the device of e")
    gp, ldgo, *gs = _nhwc_view(go)
    if gs[:3] != [T, hh, ww]:
        raise RuntimeError("ir_sums_dil: go must cover the pixels of e")
    k = L.IrSumsDilDesc()
    k.gd, k.d, k.e, k.ga, k.go, k.ldgo = gd.data_ptr(), d.data_ptr(), e.data_ptr(), ga.data_ptr(), gp, ldgo
    k.n_img, k.H, k.W, k.Ch, k.Co, k.dil = T, hh, ww, c, gs[3], dil
    nbytes = int(lib.uavsal_ir_sums_dil_workspace_bytes(C.byref(k)))
    if nbytes <= 0:
        L.check(-3, "uavsal_ir_sums_dil")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=e.device)
    k.ws, k.ws_bytes = ws.data_ptr(), nbytes
    L.check(lib.uavsal_ir_sums_dil(C.byref(k), _stream(e)), "uavsal_ir_sums_dil")
    return ws, int(lib.uavsal_ir_sums_dil_slabs(C.byref(k)))


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
    params, out = _block_grad_tensors(block, out, accumulate)
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
        if dil > 1:
            ws, slabs = ir_sums_dil(gd, d, e, ga, go, dil)
        elif shallow:
            ws, slabs = (ir_sums if stride == 1 else ir_sums_s2)(gd, d, e, ga, go, ch16=True)
        else:
            ws, slabs = (ir_sums if stride == 1 else ir_sums_s2)(gd, d, e, ga, go)
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
    _block_grad_tensors(block, grads, accumulate)                    # raise before anything is launched
    with torch.cuda.device(dev):
        cache = cache or WeightCache(dev, {})
        pt = {}
        g = _input_grad(lib, cache, block, prt, xn, go, ed=ed, parts=pt, need_x_grad=need_x_grad, res=res)
        grads = block_param_grads(block, xn.permute(0, 3, 1, 2), pt["e"], pt["d"], go.permute(0, 3, 1, 2), gd=pt["gd"], ga=pt["ga"],
                                  cache=cache, out=grads, accumulate=accumulate, backbone=backbone, shallow=shallow)
        if parts is not None:
            parts.update(pt)
    return (g.permute(0, 3, 1, 2) if need_x_grad else None), grads


# ---------------------------------------------------------------------------------------------------------------------------
# Input gradients of FROZEN blocks and of the context-prior path behind fust_layer (csrc/train_ctx.hip)
def _dense_nhwc(name, what, *ts):
    if not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.is_contiguous() for t in ts):
        raise RuntimeError("%s: %s must be dense float32 NHWC cuda tensors" % (name, what))


def ir_bwd_s2(gd, d, e, wd9, s2):
    """`uavsal_ir_bwd_s2` on the current stream: `ir_bwd` for a depthwise 3x3 with stride 2.  `gd`, `d` dense NHWC
    `[n,Ho,Wo,C]` with `Ho = (H-1)//2+1`, `Wo = (W-1)//2+1`, `e` dense NHWC `[n,H,W,C]`, the tap-major depthwise weights and
    the folded scale of the depthwise BatchNorm on the device -> `ga` = d loss / d a1, dense NHWC like `e`."""
    lib = L.load()
    _dense_nhwc("ir_bwd_s2", "gd, d, e", gd, d, e)
    n, hh, ww, c = e.shape
    if gd.shape != d.shape or tuple(d.shape) != (n, (hh - 1) // 2 + 1, (ww - 1) // 2 + 1, c) or d.device != e.device or gd.device != e.device:
        raise RuntimeError("ir_bwd_s2: gd and d must be [n,(H-1)//2+1,(W-1)//2+1,C] for e [n,H,W,C], on one device")
    for name, t, m in (("wd9", wd9, 9 * c), ("s2", s2, c)):
        if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.device == e.device and t.is_contiguous() and t.numel() >= m):
            raise RuntimeError("ir_bwd_s2: %s must be a dense float32 tensor of at least %d elements on the device of e" % (name, m))
    ga = torch.empty_like(e)
    k = L.IrBwdS2Desc()
    k.gd, k.d, k.e, k.wd9, k.s2, k.ga = gd.data_ptr(), d.data_ptr(), e.data_ptr(), wd9.data_ptr(), s2.data_ptr(), ga.data_ptr()
    k.n_img, k.H, k.W, k.C = n, hh, ww, c
    L.check(lib.uavsal_ir_bwd_s2(C.byref(k), _stream(e)), "uavsal_ir_bwd_s2")
    return ga


def bilinear_bwd(gout, n_src, hi, wi, src_mod=None, src_div=1):
    """`uavsal_bilinear_ac_bwd` on the current stream: the adjoint of the `align_corners=True` resize `[n_src,hi,wi,C]` ->
    `[n_out,Ho,Wo,C]` in which output image `n` reads source image `(n % src_mod) // src_div` (default `src_mod = n_out`).
    `gout`: an NHWC view `[n_out,Ho,Wo,C]` (a channel slice is read in place) -> the gradient of the source, dense NHWC."""
    lib = L.load()
    gp, ldo, n_out, ho, wo, c = _nhwc_view(gout)
    src_mod = n_out if src_mod is None else int(src_mod)
    gin = torch.empty((n_src, hi, wi, c), dtype=torch.float32, device=gout.device)
    k = L.BilinearBwdDesc()
    k.gout, k.ldo, k.Ho, k.Wo, k.gin, k.Hi, k.Wi = gp, ldo, ho, wo, gin.data_ptr(), hi, wi
    k.n_out, k.n_src, k.C, k.src_mod, k.src_div = n_out, n_src, c, src_mod, int(src_div)
    L.check(lib.uavsal_bilinear_ac_bwd(C.byref(k), _stream(gout)), "uavsal_bilinear_ac_bwd")
    return gin


def tsum_bwd(a, g, T):
    """`uavsal_tsum_bwd` on the current stream: `out[b*T+t] = a[b*T+t] + g[b]`, the adjoint of the sum over chunks of `T` frames
    added to a gradient that is already there.  `a` `[N,h,w,C]`, `g` `[N//T,h,w,C]` NHWC views (channel slices are read in
    place) -> dense NHWC `[N,h,w,C]`."""
    lib = L.load()
    ap, lda, n, hh, ww, c = _nhwc_view(a)
    gp, ldg, *gs = _nhwc_view(g)
    if T <= 0 or n % T or gs != [n // T, hh, ww, c] or g.device != a.device:
        raise RuntimeError("tsum_bwd: g must be [%d // T,%d,%d,%d] on the device of a, T a divisor of %d" % (n, hh, ww, c, n))
    out = torch.empty((n, hh, ww, c), dtype=torch.float32, device=a.device)
    k = L.TsumBwdDesc()
    k.a, k.lda, k.g, k.ldg, k.out, k.ldo = ap, lda, gp, ldg, out.data_ptr(), c
    k.n_groups, k.T, k.HW, k.C = n // T, T, hh * ww, c
    L.check(lib.uavsal_tsum_bwd(C.byref(k), _stream(a)), "uavsal_tsum_bwd")
    return out


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
    n, hh, ww, _ = xn.shape
    ho, wo = (hh - 1) // stride + 1, (ww - 1) // stride + 1
    if (not torch.is_tensor(grad_out) or not grad_out.is_cuda or grad_out.dtype != torch.float32 or grad_out.device != xn.device
            or tuple(grad_out.shape) != (n, cout, ho, wo)):
        raise RuntimeError("grad_out must be a float32 cuda tensor [%d,%d,%d,%d]" % (n, cout, ho, wo))
    go = _nhwc(grad_out, "grad_out", cout)
    with torch.cuda.device(xn.device):
        cache = cache or WeightCache(xn.device, {})
        g = _input_grad(lib, cache, block, prt, xn, go, parts=parts)
    return g.permute(0, 3, 1, 2)


PRIOR_PATH_BLOCKS = ("fucb_layer.0", "cxt_cb_prior.1", "cxt_cb_prior.0")      # in the order the backward walk meets them


def prior_path_blocks(model):
    """`{name: block}` of the blocks of the multi-prior path that `prior_path_backward` trains in `model`, in the order of
    `PRIOR_PATH_BLOCKS`: `fucb_layer[0]` with any prior, the two `cxt_cb_prior` blocks with the context prior."""
    if not getattr(model, "num_cb", 0):
        return {}
    blocks = {PRIOR_PATH_BLOCKS[0]: model.fucb_layer[0]}
    if model.use_context_prior:
        blocks[PRIOR_PATH_BLOCKS[1]], blocks[PRIOR_PATH_BLOCKS[2]] = model.cxt_cb_prior[1], model.cxt_cb_prior[0]
    return blocks


def prior_path_backward(model, fu320, cb192, grad_fu, cache=None, parts=None, grads=None, accumulate=False, need_fust_grad=True,
                        need_cb_grad=False):
    """ONE backward walk of the multi-prior path of a model with priors (reference model.py:344-365), given `grad_fu`
    `[N,320,h,w]` = d loss / d `fu320` (the input of `model.fucbst_layer[0]`; `block_backward(..., need_x_grad=True)` returns
    it).  The output of `model.fust_layer[0]` is channels 0..255 of `fu320`, and with the context prior it also feeds channels
    256..319: chunk sum, `cxt_cb_prior[0]`, `cxt_cb_prior[1]` (both stride 2), bilinear upsample with the tiling frame map of
    `forward()` (frame k reads chunk k % B, B = N // time_dims), concat with the other priors, `fucb_layer[0]`.  The walk goes
    back through them (`_input_grad`, `bilinear_bwd`, `tsum_bwd`) and serves two ends:
    `need_fust_grad`: the gradient with respect to fust_layer's output `[N,256,h,w]`, the path's part added to
    `grad_fu[:, :256]` (without the context prior it IS `grad_fu[:, :256]`); else None is returned in its place and what only
    it needs is not launched.
    `grads`: None -- the path is frozen, nothing but the walk is launched -- or a dict `{name: dict | None}` over
    `prior_path_blocks(model)`: each named block's nine parameter gradients (`block_param_grads`, fed the `x`, `e`, `d`, `gd`,
    `ga` and `grad_out` the walk already holds: nothing of the forward is recomputed twice) are written into the given dict of
    dense tensors, or with `accumulate` (a bool, or a dict of bools by name) added to it; None: allocated.  The gauss / ob
    prior nets are not part of this walk (`prior_net_backward`, fed by `need_cb_grad`).  The chunk sum feeds `cxt_cb_prior` B images, not N: its gradients are sums over B images.
    `fu320` `[N,320,h,w]`, `cb192` `[N,64*num_cb,h,w]`: the taps of those names, read in place as channel slices.  Returns
    `(grad_fust | None, grads | None)`.  `parts` receives `g_cb`, `g_ctx2`, `g_ctx1`, `g_sum` (NHWC), `ctx_sum`, `ctx1` and,
    per trained block, `name: dict(x=, go=, e=, d=, gd=, ga=)`.
    `need_cb_grad`: `g_cb` `[N,h,w,64*num_cb]` (NHWC) = d loss / d `cb192` is wanted as well -- the output gradients of the
    gauss / ob prior nets are its slices (`prior_net_backward`) -- and returned as a third value: `fucb_layer[0]`'s input GEMM
    is launched even where neither the context prior nor a trained block asks for it.  The default call launches what it
    always launched."""
    lib = L.load()
    if not getattr(model, "num_cb", 0):
        raise RuntimeError("fust_output_grad takes a model with at least one prior (without priors nothing lies behind fust_layer "
                           "but the recurrence)")
    if model.training:
        raise RuntimeError("the prior path is frozen: its BatchNorms are folded in eval mode (call model.eval())"
                           if grads is None else "the prior path's BatchNorms use their running statistics: call model.eval()")
    blocks = prior_path_blocks(model)
    if grads is not None:
        if not grads or any(n not in blocks for n in grads):
            raise RuntimeError("grads must name blocks of this model's prior path: %r" % (tuple(blocks),))
        for n in grads:
            _param_grad_parts(blocks[n])
            acc = accumulate[n] if isinstance(accumulate, dict) else accumulate
            _block_grad_tensors(blocks[n], grads[n], acc)              # raise before anything is launched
    train = grads or {}
    fu = _nhwc(fu320, "fu320", 320)
    N, hh, ww, _ = fu.shape
    gf = _block_grad_out(grad_fu, fu, 320)
    ctx = bool(model.use_context_prior)
    if not ctx and not train and not need_cb_grad:
        return (gf[..., :HID].permute(0, 3, 1, 2) if need_fust_grad else None), grads
    ret = lambda g, gr, gcb: (g, gr, gcb) if need_cb_grad else (g, gr)      # noqa: E731
    T = model.time_dims
    if ctx and N % T:
        raise RuntimeError("fu320 holds %d frames, not a multiple of time_dims = %d" % (N, T))
    B = N // T
    fucb = model.fucb_layer[0]
    p_cb = _input_grad_parts(fucb)
    cb = _nhwc(cb192, "cb192", 64 * model.num_cb)
    if tuple(cb.shape[:3]) != (N, hh, ww) or cb.device != fu.device:
        raise RuntimeError("cb192 must be [%d,%d,%d,%d] on the device of fu320" % (N, 64 * model.num_cb, hh, ww))
    off = 64 * (int(bool(model.use_gauss_prior)) + int(bool(model.use_ob_prior)))
    down = lambda v: (v - 1) // 2 + 1                                     # noqa: E731
    nchw = lambda t: t.permute(0, 3, 1, 2)                                # noqa: E731

    def param_grads(name, block, x, go, pt):
        if name not in train:
            return
        acc = accumulate[name] if isinstance(accumulate, dict) else accumulate
        grads[name] = block_param_grads(block, nchw(x), pt["e"], pt["d"], nchw(go), gd=pt["gd"], ga=pt["ga"], cache=cache,
                                        out=grads[name], accumulate=acc)
        if parts is not None:
            parts[name] = dict(pt, x=x, go=go)

    with torch.cuda.device(fu.device):
        cache = cache or WeightCache(fu.device, {})
        walk = ctx and (need_fust_grad or any(n in train for n in PRIOR_PATH_BLOCKS[1:]))
        pt = {}
        g_cb = _input_grad(lib, cache, fucb, p_cb, cb, gf[..., HID:], parts=pt, need_x_grad=walk or need_cb_grad)
        param_grads(PRIOR_PATH_BLOCKS[0], fucb, cb, gf[..., HID:], pt)
        if not walk:
            return ret((gf[..., :HID].permute(0, 3, 1, 2) if need_fust_grad else None), grads, g_cb)
        ctx0, ctx1b = model.cxt_cb_prior[0], model.cxt_cb_prior[1]
        p_0, p_1 = _input_grad_parts(ctx0), _input_grad_parts(ctx1b)
        g_c2 = bilinear_bwd(g_cb[..., off:off + 64], B, down(down(hh)), down(down(ww)), src_mod=B, src_div=1)
        ctx_sum = _tsum(fu[..., :HID], T)
        ed0 = _block_recompute(lib, cache, ctx0, ctx_sum, 2, p_0)
        c1 = _conv(lib, cache, ed0[1], p_0[4], p_0[4].weight.shape[0], 1, bn=p_0[5])
        pt = {}
        need1 = need_fust_grad or PRIOR_PATH_BLOCKS[2] in train
        g_c1 = _input_grad(lib, cache, ctx1b, p_1, c1, g_c2, parts=pt, need_x_grad=need1)
        param_grads(PRIOR_PATH_BLOCKS[1], ctx1b, c1, g_c2, pt)
        g_sum = g = None
        if need1:
            pt = {}
            g_sum = _input_grad(lib, cache, ctx0, p_0, ctx_sum, g_c1, ed=ed0, parts=pt, need_x_grad=need_fust_grad)
            param_grads(PRIOR_PATH_BLOCKS[2], ctx0, ctx_sum, g_c1, pt)
        if need_fust_grad:
            g = tsum_bwd(gf[..., :HID], g_sum, T)
        if parts is not None:
            parts.update(g_cb=g_cb, g_ctx2=g_c2, g_ctx1=g_c1, g_sum=g_sum, ctx_sum=ctx_sum, ctx1=c1)
    return ret((g.permute(0, 3, 1, 2) if need_fust_grad else None), grads, g_cb)


def fust_output_grad(model, fu320, cb192, grad_fu, cache=None, parts=None):
    """The gradient with respect to the OUTPUT of `model.fust_layer[0]` `[N,256,h,w]` in a model with priors, given `grad_fu`
    `[N,320,h,w]` = d loss / d `fu320`: `prior_path_backward` with the whole path frozen (no parameter gradient is computed and
    no `.grad` touched).  Without the context prior the result IS `grad_fu[:, :256]`.  The chunk sum and `cxt_cb_prior[0]`'s
    output are recomputed (B images).  `parts` receives `g_cb`, `g_ctx2`, `g_ctx1`, `g_sum` (NHWC) and `ctx_sum`, `ctx1`."""
    return prior_path_backward(model, fu320, cb192, grad_fu, cache=cache, parts=parts)[0]


# ---------------------------------------------------------------------------------------------------------------------------
# The gauss / ob prior nets (csrc/train_nets.hip): block 0 of either is too narrow for the kernels above
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
    params, out = _block_grad_tensors(block, out, accumulate)
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
    from .ops import to_nhwc
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
        _block_grad_tensors(b, grads[k], acc[k])                     # raise before anything is launched
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


# ---------------------------------------------------------------------------------------------------------------------------
# The ST blocks (csrc/train_st.hip): 1x1 conv + BatchNorm + ReLU6 stages, the adjoint of the temporal difference
ST_CBR_PARAMS = ("0.weight", "1.weight", "1.bias")                   # a BasicConv2d 1x1: W, gamma, beta
ST_BLOCK_PARTS = (("stconv_sp.spconv.", BLOCK_PARAMS), ("stconv_te.reduce_conv.", ST_CBR_PARAMS),
                  ("stconv_te.sub_conv.", BLOCK_PARAMS), ("stconv_te.last_conv.", ST_CBR_PARAMS), ("stconv_last.", ST_CBR_PARAMS))
ST_BLOCK_PARAMS = tuple(p + n for p, names in ST_BLOCK_PARTS for n in names)      # the 27 names, in named_parameters() order


def cbr_sums(g, y):
    """`uavsal_cbr_sums` on the current stream: `g`, `y` NHWC views `[N,h,w,C]` of the same pixels (channel slices are read in
    place) -> `(gp, ws, slabs)`: `gp = g * 1[0 < y < 6]` dense NHWC and the per-slab channel sums (float64 `[slab][C]`) that
    `uavsal_cbr_finish` takes."""
    lib = L.load()
    gptr, ldg, *gs = _nhwc_view(g)
    yptr, ldy, *ys = _nhwc_view(y)
    if gs != ys or g.device != y.device:
        raise RuntimeError("cbr_sums: g and y must have one shape [n,h,w,C] on one device")
    n, hh, ww, c = gs
    gp = torch.empty((n, hh, ww, c), dtype=torch.float32, device=g.device)
    k = L.CbrSumsDesc()
    k.g, k.ldg, k.y, k.ldy, k.gp = gptr, ldg, yptr, ldy, gp.data_ptr()
    k.n_img, k.H, k.W, k.C = n, hh, ww, c
    nbytes = int(lib.uavsal_cbr_sums_workspace_bytes(C.byref(k)))
    if nbytes <= 0:
        L.check(-3, "uavsal_cbr_sums")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=g.device)
    k.ws, k.ws_bytes = ws.data_ptr(), nbytes
    L.check(lib.uavsal_cbr_sums(C.byref(k), _stream(g)), "uavsal_cbr_sums")
    return gp, ws, int(lib.uavsal_cbr_sums_slabs(C.byref(k)))


def tdiff_bwd(g_dif, r, seq_len):
    """`uavsal_tdiff_bwd` on the current stream: the adjoint of `ops.tdiff` fused with the ReLU6 mask of the stage that made
    its input.  `g_dif` `[N,h,w,2C]` = d loss / d dif, `r` `[N,h,w,C]` the difference's input (NHWC views, channel slices are
    read in place), `seq_len` frames per sequence -> `gp_r` dense NHWC `[N,h,w,C]` = `1[0 < r < 6]` times the gradient with
    respect to `r`."""
    lib = L.load()
    gptr, ldg, *gs = _nhwc_view(g_dif)
    rptr, ldr, n, hh, ww, c = _nhwc_view(r)
    if gs != [n, hh, ww, 2 * c] or g_dif.device != r.device:
        raise RuntimeError("tdiff_bwd: g_dif must be [%d,%d,%d,%d] on the device of r" % (n, hh, ww, 2 * c))
    out = torch.empty((n, hh, ww, c), dtype=torch.float32, device=r.device)
    k = L.TdiffBwdDesc()
    k.g, k.ldg, k.r, k.ldr, k.out, k.ldo = gptr, ldg, rptr, ldr, out.data_ptr(), c
    k.n_img, k.HW, k.C, k.seq_len = n, hh * ww, c, int(seq_len)
    L.check(lib.uavsal_tdiff_bwd(C.byref(k), _stream(r)), "uavsal_tdiff_bwd")
    return out


def _cbr_parts(conv, bn):
    if (not isinstance(conv, torch.nn.Conv2d) or not isinstance(bn, torch.nn.BatchNorm2d) or conv.kernel_size != (1, 1)
            or conv.stride != (1, 1) or conv.groups != 1 or conv.bias is not None):
        raise RuntimeError("cbr_backward takes the 1x1 conv (no bias, stride 1) and the BatchNorm of a BasicConv2d")
    cout, cin = conv.weight.shape[:2]
    if cout % 32 or cin % 32:
        raise RuntimeError("cbr_backward needs Cout %% 32 == 0 and Cin %% 32 == 0, got %d -> %d" % (cin, cout))
    if bn.training:
        raise RuntimeError("the BatchNorm uses its running statistics: call model.eval()")
    return cin, cout


def _cbr_grad_tensors(conv, bn, out, accumulate):
    params = dict(zip(ST_CBR_PARAMS, (conv.weight, bn.weight, bn.bias)))
    if out is None:
        if accumulate:
            raise RuntimeError("accumulate needs `grads`")
        out = {n: torch.empty_like(q, memory_format=torch.contiguous_format) for n, q in params.items()}
    for n, q in params.items():
        t = out.get(n)
        if (not torch.is_tensor(t) or t.shape != q.shape or t.dtype != torch.float32 or t.device != q.device
                or not t.is_contiguous()):
            raise RuntimeError("grads[%r] must be a dense float32 tensor of the parameter's shape on its device" % n)
    return params, out


def cbr_backward(conv, bn, x, y, grad_out, need_x_grad=True, cache=None, grads=None, accumulate=False):
    """Backward of ONE 1x1 conv + BatchNorm + ReLU6 (`BasicConv2d`, eval mode: the BatchNorm on its running statistics, which
    are not updated), teacher-forced: `x` `[N,Cin,h,w]` its input, `y` an NHWC view `[N,h,w,C]` of its own activation (before
    any residual is added), `grad_out` `[N,C,h,w]` = d loss / d output.  Returns `(grad_x [N,Cin,h,w] | None, grads)`; `grads`
    keyed by `ST_CBR_PARAMS` (W, gamma, beta), the values `torch.autograd` gives, written into the given dict of dense tensors or
    with `accumulate` added to it.  `uavsal_cbr_sums` forms `gp = grad_out * 1[0 < y < 6]` and its channel sums,
    `uavsal_pix_gemm` `s[c] G[c][j]` and the row dots, `uavsal_cbr_finish` beta and gamma (from the UNSCALED sums), and
    `grad_x = gp . (diag(s) W)` is one GEMM whose transposed weights carry s in their rows (`WeightCache.conv_t_scaled`).
    Accepted: Cin % 32 == 0, C % 32 == 0.  Four launches (+ the GEMM), on the current stream, no synchronisation."""
    return _cbr_backward(conv, bn, x, y, grad_out, need_x_grad, cache, grads, accumulate)


def _cbr_backward(conv, bn, x, y, grad_out, need_x_grad, cache, grads, accumulate, res=None):
    """`cbr_backward`; `res`: an NHWC tensor the `grad_x` GEMM adds (`st_block_backward`)."""
    lib = L.load()
    cin, cout = _cbr_parts(conv, bn)
    xn = _nhwc(x, "x", cin)
    go = _block_grad_out(grad_out, xn, cout)
    dev = xn.device
    if (not torch.is_tensor(y) or y.dtype != torch.float32 or y.device != dev or tuple(y.shape) != tuple(go.shape)):
        raise RuntimeError("y must be a float32 NHWC view %r on the device of x" % (tuple(go.shape),))
    params, grads = _cbr_grad_tensors(conv, bn, grads, accumulate)
    if any(q.device != dev or not q.is_contiguous() for q in params.values()):
        raise RuntimeError("the parameters must be dense tensors on the device of `x`")
    with torch.cuda.device(dev):
        cache = cache or WeightCache(dev, {})
        s = cache.affine(bn, cout)[0]
        r, mu = cache.bn_stats(bn)
        gp, ws, slabs = cbr_sums(go, y)
        rowdot = torch.empty(cout, dtype=torch.float64, device=dev)
        pix_gemm(gp, xn, out=grads[ST_CBR_PARAMS[0]], row_scale=s, w=conv.weight.detach(), rowdot=rowdot, accumulate=accumulate)
        k = L.CbrFinishDesc()
        k.ws, k.ws_bytes, k.rowdot, k.r, k.mu = ws.data_ptr(), ws.numel() * 8, rowdot.data_ptr(), r.data_ptr(), mu.data_ptr()
        k.g_gamma, k.g_beta = grads[ST_CBR_PARAMS[1]].data_ptr(), grads[ST_CBR_PARAMS[2]].data_ptr()
        k.C, k.slabs, k.accumulate = cout, slabs, int(bool(accumulate))
        L.check(lib.uavsal_cbr_finish(C.byref(k), _stream(xn)), "uavsal_cbr_finish")
        g = _conv(lib, cache, gp, conv, cin, 1, tscale=bn, res=res) if need_x_grad else None
    return (g.permute(0, 3, 1, 2) if need_x_grad else None), grads


def _st_parts(block):
    """The sub-modules of an `STBlock` `st_block_backward` covers, or a RuntimeError."""
    sp, te, last = getattr(block, "stconv_sp", None), getattr(block, "stconv_te", None), getattr(block, "stconv_last", None)
    if sp is None or te is None or last is None or not hasattr(sp, "spconv"):
        raise RuntimeError("st_block_backward takes an STBlock (model.st_layer[i])")
    if str(getattr(block, "fu_type", "sum")).lower() != "sum":
        raise RuntimeError("st_block_backward covers fu_type='sum' only, got fu_type=%r" % (block.fu_type,))
    if block.training:
        raise RuntimeError("the ST block's BatchNorms use their running statistics: call model.eval()")
    if sp.spconv.use_res_connect or te.sub_conv.use_res_connect:
        raise RuntimeError("st_block_backward: spconv and sub_conv have no residual in an STBlock")
    return sp.spconv, te.reduce_conv, te.sub_conv, te.last_conv, last


def _st_grad_tensors(block, out, accumulate):
    params = dict(block.named_parameters())
    if sorted(params) != sorted(ST_BLOCK_PARAMS):
        raise RuntimeError("the ST block's parameters must be %r" % (ST_BLOCK_PARAMS,))
    if out is None:
        if accumulate:
            raise RuntimeError("accumulate needs `grads`")
        out = {n: torch.empty_like(params[n], memory_format=torch.contiguous_format) for n in ST_BLOCK_PARAMS}
    for n in ST_BLOCK_PARAMS:
        t, q = out.get(n), params[n]
        if (not torch.is_tensor(t) or t.shape != q.shape or t.dtype != torch.float32 or t.device != q.device
                or not t.is_contiguous()):
            raise RuntimeError("grads[%r] must be a dense float32 tensor of the parameter's shape on its device" % n)
    return params, out


def st_block_backward(block, x, grad_out, seq_len=None, need_x_grad=True, cache=None, parts=None, grads=None, accumulate=False):
    """Backward of an ST block that is TRAINED (`model.st_layer[i]`, reference model.py:163-249; eval mode: every BatchNorm on
    its running statistics, which are not updated): `x` `[N,256,h,w]` its input, `grad_out` `[N,256,h,w]` = d loss / d output,
    `seq_len` the frames per sequence of the temporal difference (default: all N -- `forward()`; one clip's T for
    `forward_clips`).  Returns `(grad_x [N,256,h,w] | None, grads)`, `grads` keyed by the block's 27 parameter names
    (`ST_BLOCK_PARAMS`), written into the given dict of dense tensors or with `accumulate` added to it.
        x_sp = spconv(x);  r = ReLU6(BN(W_r x));  dif = tdiff(r);  t1 = sub_conv(dif);  a_te = ReLU6(BN(W_l t1));
        o = ReLU6(BN(W_last (x_sp + a_te)));  out = x + o
    The intermediates are recomputed by the forward's own launches, each once (`a_te` and `o` WITHOUT the residual their
    launches add in the plan: the ReLU6 masks are those of the stages' own activations; `x_sp + a_te` is one `uavsal_tsum_bwd`
    launch with T = 1, the fp32 sum the plan's epilogue forms).  The walk: `stconv_last` (`cbr_backward`), the spatial branch
    (`block_backward` on `spconv`), `last_conv` (`cbr_backward`), `sub_conv` (the input-gradient walk + `block_param_grads`),
    `tdiff_bwd`, `reduce_conv` (`cbr_backward`; the mask is already in `tdiff_bwd`'s output, applying it again changes no
    bit).  `grad_x = (grad_out + spconv's) + reduce_conv's`: each GEMM adds what is already there.  `need_x_grad=False` (block
    0: the backbone is frozen) leaves the two GEMMs out.  `parts` receives every intermediate (NHWC): `e_sp`, `d_sp`, `x_sp`,
    `r`, `dif`, `e_te`, `d_te`, `t1`, `a_te`, `ssum`, `o`, `g_sum`, `g_t1`, `g_dif`, `gp_r`, `gx_sp` and `sp` / `sub`, the two
    blocks' `dict(e=, d=, gd=, ga=)`.  A block in training mode, `fu_type != 'sum'` or CPU tensors raise."""
    lib = L.load()
    spc, red, sub, lastc, stl = _st_parts(block)
    p_sub = _input_grad_parts(sub)
    _param_grad_parts(sub)
    p_sp = _block_parts(spc)
    for cv in (red, lastc, stl):
        _cbr_parts(cv[0], cv[1])
    cin = spc.cin
    xn = _nhwc(x, "x", cin)
    go = _block_grad_out(grad_out, xn, stl[0].weight.shape[0])
    N, hh, ww, _ = xn.shape
    seq_len = N if seq_len is None else int(seq_len)
    if seq_len < 2 or N % seq_len:
        raise RuntimeError("seq_len must be at least 2 and divide the %d frames, got %r" % (N, seq_len))
    dev = xn.device
    _, grads = _st_grad_tensors(block, grads, accumulate)                # raise before anything is launched
    sub_g = lambda prefix, names: {n: grads[prefix + n] for n in names}   # noqa: E731
    g_sp, g_red, g_sub, g_last, g_stl = (sub_g(p, names) for p, names in ST_BLOCK_PARTS)
    nchw = lambda t: t.permute(0, 3, 1, 2)                                # noqa: E731
    from .ops import tdiff as _tdiff
    with torch.cuda.device(dev):
        cache = cache or WeightCache(dev, {})
        # ---- the forward's intermediates
        e_sp, d_sp = _block_recompute(lib, cache, spc, xn, 1, p_sp)
        x_sp = _conv(lib, cache, d_sp, p_sp[4], p_sp[4].weight.shape[0], 1, bn=p_sp[5])
        r = _conv(lib, cache, xn, red[0], red[0].weight.shape[0], 1, bn=red[1], act=L.ACT_RELU6)
        dif = _tdiff(r, seq_len)
        e_te, d_te = _block_recompute(lib, cache, sub, dif, 1, p_sub)
        t1 = _conv(lib, cache, d_te, p_sub[4], p_sub[4].weight.shape[0], 1, bn=p_sub[5])
        a_te = _conv(lib, cache, t1, lastc[0], lastc[0].weight.shape[0], 1, bn=lastc[1], act=L.ACT_RELU6)
        ssum = tsum_bwd(a_te, x_sp, 1)
        o = _conv(lib, cache, ssum, stl[0], stl[0].weight.shape[0], 1, bn=stl[1], act=L.ACT_RELU6)
        # ---- the walk back
        g_sum, _ = cbr_backward(stl[0], stl[1], nchw(ssum), o, nchw(go), cache=cache, grads=g_stl, accumulate=accumulate)
        pt_sp = {}
        gx, _ = _block_backward(spc, nchw(xn), g_sum, need_x_grad, cache, pt_sp, g_sp, accumulate, ed=(e_sp, d_sp), res=go)
        g_t1, _ = cbr_backward(lastc[0], lastc[1], nchw(t1), a_te, g_sum, cache=cache, grads=g_last, accumulate=accumulate)
        g_t1n = g_t1.permute(0, 2, 3, 1)
        pt_sub = {}
        g_dif = _input_grad(lib, cache, sub, p_sub, dif, g_t1n, ed=(e_te, d_te), parts=pt_sub)
        block_param_grads(sub, nchw(dif), e_te, d_te, g_t1, gd=pt_sub["gd"], ga=pt_sub["ga"], cache=cache, out=g_sub,
                          accumulate=accumulate)
        gp_r = tdiff_bwd(g_dif, r, seq_len)
        g, _ = _cbr_backward(red[0], red[1], nchw(xn), r, nchw(gp_r), need_x_grad, cache, g_red, accumulate,
                             res=gx.permute(0, 2, 3, 1) if need_x_grad else None)
        if parts is not None:
            parts.update(e_sp=e_sp, d_sp=d_sp, x_sp=x_sp, r=r, dif=dif, e_te=e_te, d_te=d_te, t1=t1, a_te=a_te, ssum=ssum, o=o,
                         g_sum=g_sum.permute(0, 2, 3, 1), g_t1=g_t1n, g_dif=g_dif, gp_r=gp_r,
                         gx_sp=gx.permute(0, 2, 3, 1) if need_x_grad else None, sp=pt_sp, sub=pt_sub)
    return g, grads


# ---------------------------------------------------------------------------------------------------------------------------
# The SRF-Net head (model.sfnet without its MobileNetV2 `features`): an eighth stage (csrc/train_srf.hip)
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


def conv3_wgrad(g, x, out=None, row_scale=None, w=None, rowdot=None, accumulate=False):
    """`uavsal_conv3_wgrad` on the current stream: `g` dense NHWC `[n,h,w,Co]`, `x` an NHWC view `[n,h,w,Ci]` of the same pixels
    (a channel slice is read in place) -> `out[co][ci][ky][kx] = row_scale[co] sum_p g[p][co] x[p + (ky-1, kx-1)][ci]` (dense
    `[Co,Ci,3,3]`, zero outside the picture, never across frames; `accumulate`: added to `out`), and with `w` `[Co,Ci,3,3]` and
    `rowdot` (float64 `[Co]`) `rowdot[co] = sum w[co] G[co]`.  Co % 128 == 0, Ci % 64 == 0.  Two launches, no synchronisation."""
    lib = L.load()
    _dense_nhwc("conv3_wgrad", "g", g)
    xp, ldx, *xs = _nhwc_view(x)
    n, hh, ww, co = g.shape
    if xs[:3] != [n, hh, ww] or x.device != g.device:
        raise RuntimeError("conv3_wgrad: g and x must cover the same pixels on one device")
    ci, dev = xs[3], g.device
    if co % 128 or ci % 64:
        raise RuntimeError("conv3_wgrad takes Co %% 128 == 0 and Ci %% 64 == 0, got Co = %d, Ci = %d" % (co, ci))
    if out is None:
        if accumulate:
            raise RuntimeError("accumulate needs `out`")
        out = torch.empty((co, ci, 3, 3), dtype=torch.float32, device=dev)
    if tuple(out.shape) != (co, ci, 3, 3) or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
        raise RuntimeError("out must be a dense float32 [%d,%d,3,3] tensor on the device" % (co, ci))
    k = L.Conv3WgradDesc()
    k.g, k.x, k.ldx = g.data_ptr(), xp, ldx
    k.n_img, k.H, k.W, k.Co, k.Ci, k.accumulate = n, hh, ww, co, ci, int(bool(accumulate))
    if row_scale is not None:
        if row_scale.dtype != torch.float32 or row_scale.device != dev or row_scale.numel() < co or not row_scale.is_contiguous():
            raise RuntimeError("row_scale must be a dense float32 vector of at least %d elements on the device" % co)
        k.row_scale = row_scale.data_ptr()
    if rowdot is not None:
        if (w is None or tuple(w.shape) != (co, ci, 3, 3) or not w.is_contiguous() or w.dtype != torch.float32 or w.device != dev
                or rowdot.dtype != torch.float64 or rowdot.numel() != co or not rowdot.is_contiguous() or rowdot.device != dev):
            raise RuntimeError("rowdot needs a dense float32 `w` [%d,%d,3,3] and a dense float64 [%d] on the device" % (co, ci, co))
        k.w, k.rowdot = w.data_ptr(), rowdot.data_ptr()
    nbytes = int(lib.uavsal_conv3_wgrad_workspace_bytes(C.byref(k)))
    if nbytes <= 0:
        L.check(-3, "uavsal_conv3_wgrad")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    k.ws, k.ws_bytes, k.out = ws.data_ptr(), nbytes, out.data_ptr()
    L.check(lib.uavsal_conv3_wgrad(C.byref(k), _stream(g)), "uavsal_conv3_wgrad")
    return out


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
    cin, cout = _conv3_parts(conv, bn)
    xn = _nhwc(x, "x", cin)
    go = _block_grad_out(grad_out, xn, cout)
    dev = xn.device
    if (not torch.is_tensor(y) or y.dtype != torch.float32 or y.device != dev or tuple(y.shape) != tuple(go.shape)):
        raise RuntimeError("y must be a float32 NHWC view %r on the device of x" % (tuple(go.shape),))
    params, grads = _cbr_grad_tensors(conv, bn, grads, accumulate)
    if any(q.device != dev or not q.is_contiguous() for q in params.values()):
        raise RuntimeError("the parameters must be dense tensors on the device of `x`")
    with torch.cuda.device(dev):
        cache = cache or WeightCache(dev, {})
        s = cache.affine(bn, cout)[0]
        r, mu = cache.bn_stats(bn)
        gp, ws, slabs = cbr_sums(go, y)
        rowdot = torch.empty(cout, dtype=torch.float64, device=dev)
        conv3_wgrad(gp, xn, out=grads[ST_CBR_PARAMS[0]], row_scale=s, w=conv.weight.detach(), rowdot=rowdot, accumulate=accumulate)
        k = L.CbrFinishDesc()
        k.ws, k.ws_bytes, k.rowdot, k.r, k.mu = ws.data_ptr(), ws.numel() * 8, rowdot.data_ptr(), r.data_ptr(), mu.data_ptr()
        k.g_gamma, k.g_beta = grads[ST_CBR_PARAMS[1]].data_ptr(), grads[ST_CBR_PARAMS[2]].data_ptr()
        k.C, k.slabs, k.accumulate = cout, slabs, int(bool(accumulate))
        L.check(lib.uavsal_cbr_finish(C.byref(k), _stream(xn)), "uavsal_cbr_finish")
        g = _conv(lib, cache, gp, conv, cin, 9, tscale=bn) if need_x_grad else None
    return (g.permute(0, 3, 1, 2) if need_x_grad else None), grads


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


def _srf_grad_tensors(sfnet, out, accumulate):
    params = dict(sfnet.named_parameters())
    if any(n not in params for n in SRF_HEAD_PARAMS):
        raise RuntimeError("the head's parameters must be %r" % (SRF_HEAD_PARAMS,))
    if out is None:
        if accumulate:
            raise RuntimeError("accumulate needs `grads`")
        out = {n: torch.empty_like(params[n], memory_format=torch.contiguous_format) for n in SRF_HEAD_PARAMS}
    for n in SRF_HEAD_PARAMS:
        t, q = out.get(n), params[n]
        if (not torch.is_tensor(t) or t.shape != q.shape or t.dtype != torch.float32 or t.device != q.device
                or not t.is_contiguous()):
            raise RuntimeError("grads[%r] must be a dense float32 tensor of the parameter's shape on its device" % n)
    return params, out


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
    _, grads = _srf_grad_tensors(sfnet, grads, accumulate)               # raise before anything is launched
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


# ---------------------------------------------------------------------------------------------------------------------------
# The deep backbone as a ninth stage: MobileNetV2 features[8:18] behind the frozen features[0:8]
BACKBONE_FIRST, BACKBONE_END = 8, 18                                 # features[8:18]: the blocks at 1/16 and 1/32 resolution
BACKBONE_C4 = 13                                                     # the block whose output is the c4 tap (c5: block 17)
BACKBONE_PARAMS = tuple("%d.%s" % (i, n) for i in range(BACKBONE_FIRST, BACKBONE_END) for n in BLOCK_PARAMS)      # the 90 names


def backbone_blocks(model):
    """The ten trainable backbone blocks `model.sfnet.features.features[8:18]`, in forward order: 64 -> 384 -> 64 (three), 64 ->
    384 -> 96, 96 -> 576 -> 96 (two) at 1/16 resolution, 96 -> 576 -> 160 with stride 2, 160 -> 960 -> 160 (two) and 160 -> 960
    -> 320 at 1/32.  Hand their parameters to the optimiser and the modules to `model.refresh_weights(*train.backbone_blocks(
    model))`: their packed forms (natural-layout fused entries or unfused launches) are remade in place.  `features[2:8]`
    are the next stage (`shallow_blocks`); the stem and `features[1]` stay frozen."""
    sf = getattr(model, "sfnet", model)
    return list(sf.features.features[BACKBONE_FIRST:BACKBONE_END])


def _backbone_grad_tensors(features, out, accumulate):
    params = {"%d.%s" % (i, n): q for i in range(BACKBONE_FIRST, BACKBONE_END) for n, q in features[i].named_parameters()}
    if tuple(params) != BACKBONE_PARAMS:
        raise RuntimeError("the backbone's parameters must be %r of features[%d:%d]" % (BLOCK_PARAMS, BACKBONE_FIRST, BACKBONE_END))
    if out is None:
        if accumulate:
            raise RuntimeError("accumulate needs `grads`")
        out = {n: torch.empty_like(q, memory_format=torch.contiguous_format) for n, q in params.items()}
    for n, q in params.items():
        t = out.get(n)
        if (not torch.is_tensor(t) or t.shape != q.shape or t.dtype != torch.float32 or t.device != q.device
                or not t.is_contiguous()):
            raise RuntimeError("grads[%r] must be a dense float32 tensor of the parameter's shape on its device" % n)
    return params, out


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
    _, grads = _backbone_grad_tensors(features, grads, accumulate)       # raise before anything is launched
    sub_g = lambda i: {n: grads["%d.%s" % (i, n)] for n in BLOCK_PARAMS}  # noqa: E731
    g4 = _nhwc(g_c4, "g_c4")

    def forward(blk, prt, x):
        e, d = _block_recompute(lib, cache, blk, x, prt[2].stride[0], prt)
        return e, d, _conv(lib, cache, d, prt[4], prt[4].weight.shape[0], 1, bn=prt[5], res=x if blk.use_res_connect else None)

    with torch.cuda.device(dev):
        cache = cache or WeightCache(dev, {})
        xs, eds = {BACKBONE_FIRST - 2: c3n}, {}
        xs[BACKBONE_FIRST - 1] = forward(features[BACKBONE_FIRST - 1], p7, c3n)[2]
        for i in range(BACKBONE_FIRST, BACKBONE_END):
            e, d, xs[i] = forward(features[i], prts[i], xs[i - 1])
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


# ---------------------------------------------------------------------------------------------------------------------------
# The shallow backbone as a tenth stage: MobileNetV2 features[2:8] behind the frozen stem and features[1]
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


def _shallow_grad_tensors(features, out, accumulate):
    params = {"%d.%s" % (i, n): q for i in range(SHALLOW_FIRST, SHALLOW_END) for n, q in features[i].named_parameters()}
    if tuple(params) != SHALLOW_PARAMS:
        raise RuntimeError("the shallow backbone's parameters must be %r of features[%d:%d]" % (BLOCK_PARAMS, SHALLOW_FIRST, SHALLOW_END))
    if out is None:
        if accumulate:
            raise RuntimeError("accumulate needs `grads`")
        out = {n: torch.empty_like(q, memory_format=torch.contiguous_format) for n, q in params.items()}
    for n, q in params.items():
        t = out.get(n)
        if (not torch.is_tensor(t) or t.shape != q.shape or t.dtype != torch.float32 or t.device != q.device
                or not t.is_contiguous()):
            raise RuntimeError("grads[%r] must be a dense float32 tensor of the parameter's shape on its device" % n)
    return params, out


def _stem_forward(lib, cache, stem, x):
    """`features[0]` (conv 3x3 stride 2 + BatchNorm + ReLU6) on the frames `x` `[N,3,H,W]` (fp32, or uint8 RGB that the kernel
    normalises on load) -> NHWC `[N,(H-1)//2+1,(W-1)//2+1,32]`: the forward's own `uavsal_stem_conv`, no synchronisation."""
    from .synth import IMAGENET_MEAN, IMAGENET_STD
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
    _, grads = _shallow_grad_tensors(features, grads, accumulate)        # raise before anything is launched
    sub_g = lambda i: {n: grads["%d.%s" % (i, n)] for n in BLOCK_PARAMS}  # noqa: E731
    g3 = _nhwc(g_c3, "g_c3")

    def forward(blk, prt, xin):
        e, d = _block_recompute(lib, cache, blk, xin, prt[2].stride[0], prt)
        return e, d, _conv(lib, cache, d, prt[4], prt[4].weight.shape[0], 1, bn=prt[5], res=xin if blk.use_res_connect else None)

    with torch.cuda.device(dev):
        cache = cache or WeightCache(dev, {})
        xs, eds = {0: _stem_forward(lib, cache, stem, x.contiguous())}, {}
        xs[1] = _fused_forward(lib, cache, f1, xs[0])
        for i in range(SHALLOW_FIRST, SHALLOW_END):
            e, d, xs[i] = forward(features[i], prts[i], xs[i - 1])
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


def twa_gate_bwd(g, carry, z, x, hprev, need_dx=False):
    """`uavsal_twa_gate_bwd` on NHWC tensors `[1,h,w,256]` (`g`, `x`, `hprev` may be channel slices; `carry` dense or None):
    returns `(dz, carry_out, dx | None)`, dense."""
    lib = L.load()
    gp, ldg, n, hh, ww, c = _nhwc_view(g)
    xp, ldx, *xs = _nhwc_view(x)
    hp, ldh, *hs = _nhwc_view(hprev)
    if xs != [n, hh, ww, c] or hs != [n, hh, ww, c] or x.device != g.device or hprev.device != g.device:
        raise RuntimeError("twa_gate_bwd: g, x and hprev must have one shape [n,h,w,256] on one device")
    for name, t in (("z", z), ("carry", carry)):
        if t is not None and not (torch.is_tensor(t) and t.dtype == torch.float32 and t.device == g.device
                                  and tuple(t.shape) == (n, hh, ww, c) and t.is_contiguous()):
            raise RuntimeError("twa_gate_bwd: %s must be a dense float32 [n,h,w,256] tensor of g's shape and device" % name)
    dz = torch.empty((n, hh, ww, c), dtype=torch.float32, device=g.device)
    co = torch.empty_like(dz)
    dx = torch.empty_like(dz) if need_dx else None
    _gate(lib, gp, ldg, carry, z, xp, ldx, hp, ldh, dz, co, dx, n * hh * ww, c, _stream(g))
    return dz, co, dx


def _gate(lib, gp, ldg, carry, z, xp, ldx, hp, ldh, dz, co, dx, n_pix, c, st):
    k = L.TwaGateDesc()
    k.g, k.ldg, k.carry, k.z = gp, ldg, (carry.data_ptr() if carry is not None else None), z.data_ptr()
    k.x, k.ldx, k.hprev, k.ldh = xp, ldx, hp, ldh
    k.dz, k.carry_out, k.dx = dz.data_ptr(), co.data_ptr(), (dx.data_ptr() if dx is not None else None)
    k.n_pix, k.C = n_pix, c
    L.check(lib.uavsal_twa_gate_bwd(C.byref(k), st), "uavsal_twa_gate_bwd")


def twa_wgrad(dz, x, h, h0, out=None, accumulate=False):
    """`uavsal_twa_wgrad` on NHWC tensors: `dz` dense `[T,h,w,256]`, `x`, `h` `[T,h,w,256]`, `h0` `[1,h,w,256]` (channel slices
    allowed) -> `dW` `[256,512,3,3]`, written to `out` or (`accumulate`) added to it.  Two launches, no synchronisation."""
    lib = L.load()
    if not torch.is_tensor(dz) or dz.dim() != 4 or not dz.is_contiguous():
        raise RuntimeError("twa_wgrad: dz must be a dense [T,h,w,256] tensor")
    T, hh, ww, c = dz.shape
    if dz.dim() != 4 or dz.dtype != torch.float32 or not dz.is_cuda:
        raise RuntimeError("twa_wgrad: dz must be a float32 cuda tensor [T,h,w,256]")
    xp, ldx, *xs = _nhwc_view(x)
    hp, ldh, *hs = _nhwc_view(h)
    h0p, ldh0, *h0s = _nhwc_view(h0)
    if xs != [T, hh, ww, c] or hs != [T, hh, ww, c] or h0s != [1, hh, ww, c] or any(t.device != dz.device for t in (x, h, h0)):
        raise RuntimeError("twa_wgrad: x and h must be [T,h,w,256] like dz and h0 [1,h,w,256], all on one device")
    if out is None:
        if accumulate:
            raise RuntimeError("accumulate needs `out`")
        out = torch.empty((c, 2 * c, 3, 3), dtype=torch.float32, device=dz.device)
    if (tuple(out.shape) != (c, 2 * c, 3, 3) or out.dtype != torch.float32 or out.device != dz.device or not out.is_contiguous()):
        raise RuntimeError("out must be a dense float32 [%d,%d,3,3] tensor on the device" % (c, 2 * c))
    k = L.TwaWgradDesc()
    k.dz, k.x, k.ldx, k.h, k.ldh, k.h0, k.ldh0 = dz.data_ptr(), xp, ldx, hp, ldh, h0p, ldh0
    k.T, k.H, k.W, k.C, k.accumulate = T, hh, ww, c, int(bool(accumulate))
    nbytes = int(lib.uavsal_twa_wgrad_workspace_bytes(C.byref(k)))
    if nbytes <= 0:
        L.check(-3, "uavsal_twa_wgrad")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dz.device)
    k.ws, k.ws_bytes, k.out = ws.data_ptr(), nbytes, out.data_ptr()
    L.check(lib.uavsal_twa_wgrad(C.byref(k), _stream(dz)), "uavsal_twa_wgrad")
    return out


def twa_backward(x_seq, h_seq, h0, weight, grad_h, need_x_grad=False, out=None, accumulate=False, cache=None, module=None,
                 parts=None):
    """Back-propagation through time over one ConvTWA sequence.  `x_seq` `[T,256,h,w]` the recurrence input, `h_seq`
    `[T,256,h,w]` its output history, `h0` `[1,256,h,w]` the state it started from (None = zeros), `weight` `[256,512,3,3]`,
    `grad_h` `[T,256,h,w]` the gradient of the loss with respect to every `h_t` (the carried part excluded).
    Returns `(grad_weight [256,512,3,3], grad_x [T,256,h,w] | None, grad_h0 [1,256,h,w])`; `out` / `accumulate`: the weight
    gradient is written to `out` or added to it (`.grad +=`).
    The gates are recomputed from the known history by two batched 3x3 convs over all frames, so the forward stays what it is
    and only the carry runs step by step: per step one `uavsal_twa_gate_bwd` and one 3x3 conv with flip(W_h)^T.
    `cache` + `module`: take the packed forms of the weight from a `WeightCache` under the id of `module` (the conv that
    owns `weight`); default: packed on the host for this call.  `parts`: a dict that receives `z`, `dz` (NHWC; tests)."""
    lib = L.load()
    x = _nhwc(x_seq, "x_seq", HID)
    h = _nhwc(h_seq, "h_seq", HID)
    G = _nhwc(grad_h, "grad_h", HID)
    T, hh, ww, _ = x.shape
    if h.shape != x.shape or G.shape != x.shape:
        raise RuntimeError("x_seq, h_seq and grad_h must have one shape [T,256,h,w]")
    dev = x.device
    if (not torch.is_tensor(weight) or tuple(weight.shape) != (HID, 2 * HID, 3, 3) or weight.dtype != torch.float32
            or weight.device != dev):
        raise RuntimeError("weight must be the float32 [256,512,3,3] ConvTWA weight on the device")
    with torch.cuda.device(dev):
        if h0 is None:
            h0n = torch.zeros((1, hh, ww, HID), dtype=torch.float32, device=dev)
        else:
            h0n = _nhwc(h0, "h0", HID)
            if tuple(h0n.shape) != (1, hh, ww, HID):
                raise RuntimeError("h0 must be [1,256,%d,%d]" % (hh, ww))
        if cache is None or module is None:
            cache, module = WeightCache(dev, {}), types.SimpleNamespace(weight=weight)
        st = _stream(x)
        hprev = torch.cat([h0n, h[:T - 1]], 0)                       # h_{t-1} of every frame, dense
        z = _conv(lib, cache, x, module, HID, 9, wslice=(0, HID))
        z = _conv(lib, cache, hprev, module, HID, 9, wslice=(HID, 2 * HID), res=z)
        dz = torch.empty((T, hh, ww, HID), dtype=torch.float32, device=dev)
        dx = torch.empty_like(dz) if need_x_grad else None
        cbuf = torch.empty((1, hh, ww, HID), dtype=torch.float32, device=dev)
        carry = None
        hw = hh * ww
        gp, ldg, *_ = _nhwc_view(G)
        xp, ldx, *_ = _nhwc_view(x)
        for t in range(T - 1, -1, -1):
            _gate(lib, gp + 4 * t * hw * ldg, ldg, carry, z[t], xp + 4 * t * hw * ldx, ldx, hprev[t].data_ptr(), HID,
                  dz[t], cbuf, dx[t] if need_x_grad else None, hw, HID, st)
            carry = _conv(lib, cache, dz[t:t + 1], module, HID, 9, wslice=(HID, 2 * HID), transposed=True, res=cbuf)
        if need_x_grad:
            dx = _conv(lib, cache, dz, module, HID, 9, wslice=(0, HID), transposed=True, res=dx)
        gw = twa_wgrad(dz, x, h, h0n, out=out, accumulate=accumulate)
        if parts is not None:
            parts.update(z=z, dz=dz)
    return gw, (dx.permute(0, 3, 1, 2) if need_x_grad else None), carry.permute(0, 3, 1, 2)


def _dense(name, what, t, shape, dev):
    if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.device == dev and tuple(t.shape) == tuple(shape)
            and t.is_contiguous()):
        raise RuntimeError("%s: %s must be a dense float32 %r tensor on the device" % (name, what, list(shape)))


def lstm_scan(cc, c0=None):
    """`uavsal_lstm_scan` on the current stream: `cc` dense NHWC `[T,h,w,4C]` (rows gate * C + c, gates i, f, o, g), `c0` dense
    `[1,h,w,C]` or None (zeros) -> the cell-state history `c_seq` dense `[T,h,w,C]`, `c_t = f c_{t-1} + i g`.  One launch."""
    lib = L.load()
    if not torch.is_tensor(cc) or not cc.is_cuda or cc.dim() != 4 or cc.shape[3] % 4:
        raise RuntimeError("lstm_scan: cc must be a dense float32 cuda tensor [T,h,w,4C] (no CPU fallback)")
    T, hh, ww, c4 = cc.shape
    c = c4 // 4
    _dense("lstm_scan", "cc", cc, cc.shape, cc.device)
    if c0 is not None:
        _dense("lstm_scan", "c0", c0, (1, hh, ww, c), cc.device)
    cs = torch.empty((T, hh, ww, c), dtype=torch.float32, device=cc.device)
    k = L.LstmScanDesc()
    k.cc, k.c0, k.c_seq = cc.data_ptr(), (c0.data_ptr() if c0 is not None else None), cs.data_ptr()
    k.n_pix, k.T, k.C = hh * ww, T, c
    with torch.cuda.device(cc.device):
        L.check(lib.uavsal_lstm_scan(C.byref(k), _stream(cc)), "uavsal_lstm_scan")
    return cs


def lstm_gate_bwd(g, carry_h, carry_c, cc, c, c_prev, dcc=None, carry_c_out=None):
    """`uavsal_lstm_gate_bwd` on NHWC tensors: `g` `[1,h,w,C]` (may be a channel slice), `carry_h`, `carry_c` dense or None,
    `cc` dense `[1,h,w,4C]`, `c`, `c_prev` dense `[1,h,w,C]` -> `(dcc [1,h,w,4C], carry_c_out [1,h,w,C])`, dense; written into
    `dcc` / `carry_c_out` when given (`carry_c_out` may be `carry_c`)."""
    lib = L.load()
    gp, ldg, n, hh, ww, ch = _nhwc_view(g)
    dev = g.device
    for name, t in (("carry_h", carry_h), ("carry_c", carry_c), ("c", c), ("c_prev", c_prev), ("carry_c_out", carry_c_out)):
        if t is not None or name in ("c", "c_prev"):
            _dense("lstm_gate_bwd", name, t, (n, hh, ww, ch), dev)
    _dense("lstm_gate_bwd", "cc", cc, (n, hh, ww, 4 * ch), dev)
    if dcc is None:
        dcc = torch.empty((n, hh, ww, 4 * ch), dtype=torch.float32, device=dev)
    _dense("lstm_gate_bwd", "dcc", dcc, (n, hh, ww, 4 * ch), dev)
    if carry_c_out is None:
        carry_c_out = torch.empty((n, hh, ww, ch), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lstm_gate(lib, gp, ldg, carry_h, carry_c, cc, c, c_prev, dcc, carry_c_out, n * hh * ww, ch, _stream(g))
    return dcc, carry_c_out


def _lstm_gate(lib, gp, ldg, carry_h, carry_c, cc, c, c_prev, dcc, co, n_pix, ch, st):
    k = L.LstmGateDesc()
    k.g, k.ldg = gp, ldg
    k.carry_h = carry_h.data_ptr() if carry_h is not None else None
    k.carry_c = carry_c.data_ptr() if carry_c is not None else None
    k.cc, k.c, k.c_prev, k.dcc, k.carry_c_out = cc.data_ptr(), c.data_ptr(), c_prev.data_ptr(), dcc.data_ptr(), co.data_ptr()
    k.n_pix, k.C = n_pix, ch
    L.check(lib.uavsal_lstm_gate_bwd(C.byref(k), st), "uavsal_lstm_gate_bwd")


def lstm_backward(x_seq, h_seq, h0, c0, weight, grad_h, need_x_grad=False, out=None, accumulate=False, cache=None, module=None,
                  parts=None):
    """Back-propagation through time over one ConvLSTM sequence (`UAVSAL_LSTM`; reference model_convlstm.py:111-126, no bias,
    one layer): the counterpart of `twa_backward`.  `x_seq` `[T,256,h,w]` the recurrence input, `h_seq` `[T,256,h,w]` its
    output history, `h0`, `c0` `[1,256,h,w]` the state it started from (None = zeros), `weight` `[1024,512,3,3]` (rows
    gate * 256 + c, gates i, f, o, g), `grad_h` `[T,256,h,w]` the gradient of the loss with respect to every `h_t` (the carried
    part excluded; the returned state is detached, so nothing arrives at `c_t` directly).
    Returns `(grad_weight [1024,512,3,3], grad_x [T,256,h,w] | None, grad_h0 [1,256,h,w], grad_c0 [1,256,h,w])`; `out` /
    `accumulate`: the weight gradient is written to `out` or added to it (`.grad +=`).
    The pre-activations `cc` are recomputed from the known history by two batched 3x3 convs over all frames and the cell
    states from them by ONE `uavsal_lstm_scan`, so the forward stays what it is (no new tap, no arena change) and only the
    carry runs step by step: per step one `uavsal_lstm_gate_bwd` (which keeps `carry_c`) and one 3x3 conv 1024 -> 256 with
    flip(W_h)^T.  `grad_x` is one such conv with flip(W_x)^T over all frames, the weight gradient one `uavsal_conv3_wgrad`
    (Co = 1024, Ci = 512) over `cat[x, h_prev]`.
    `cache` + `module`: take the packed forms of the weight from a `WeightCache` under the id of `module` (the conv that
    owns `weight`); default: packed on the host for this call.  `parts`: a dict that receives `cc`, `c_seq`, `dcc` (NHWC;
    tests)."""
    lib = L.load()
    x = _nhwc(x_seq, "x_seq", HID)
    h = _nhwc(h_seq, "h_seq", HID)
    G = _nhwc(grad_h, "grad_h", HID)
    T, hh, ww, _ = x.shape
    if h.shape != x.shape or G.shape != x.shape:
        raise RuntimeError("x_seq, h_seq and grad_h must have one shape [T,256,h,w]")
    dev = x.device
    if (not torch.is_tensor(weight) or tuple(weight.shape) != (4 * HID, 2 * HID, 3, 3) or weight.dtype != torch.float32
            or weight.device != dev):
        raise RuntimeError("weight must be the float32 [1024,512,3,3] ConvLSTM weight on the device")
    with torch.cuda.device(dev):
        st0 = []
        for name, s in (("h0", h0), ("c0", c0)):
            if s is None:
                st0.append(torch.zeros((1, hh, ww, HID), dtype=torch.float32, device=dev))
            else:
                s = _nhwc(s, name, HID).contiguous()
                if tuple(s.shape) != (1, hh, ww, HID):
                    raise RuntimeError("%s must be [1,256,%d,%d]" % (name, hh, ww))
                st0.append(s)
        h0n, c0n = st0
        if cache is None or module is None:
            cache, module = WeightCache(dev, {}), types.SimpleNamespace(weight=weight)
        st = _stream(x)
        hprev = torch.cat([h0n, h[:T - 1]], 0)                       # h_{t-1} of every frame, dense
        cc = _conv(lib, cache, x, module, 4 * HID, 9, wslice=(0, HID))
        cc = _conv(lib, cache, hprev, module, 4 * HID, 9, wslice=(HID, 2 * HID), res=cc)
        cs = lstm_scan(cc, c0n if c0 is not None else None)
        dcc = torch.empty_like(cc)
        cbuf = torch.empty((1, hh, ww, HID), dtype=torch.float32, device=dev)
        carry = None
        hw = hh * ww
        gp, ldg, *_ = _nhwc_view(G)
        for t in range(T - 1, -1, -1):
            _lstm_gate(lib, gp + 4 * t * hw * ldg, ldg, carry, cbuf if carry is not None else None, cc[t], cs[t],
                       cs[t - 1] if t else c0n, dcc[t], cbuf, hw, HID, st)
            carry = _conv(lib, cache, dcc[t:t + 1], module, HID, 9, wslice=(HID, 2 * HID), transposed=True)
        dx = _conv(lib, cache, dcc, module, HID, 9, wslice=(0, HID), transposed=True) if need_x_grad else None
        gw = conv3_wgrad(dcc, torch.cat([x, hprev], 3), out=out, accumulate=accumulate)
        if parts is not None:
            parts.update(cc=cc, c_seq=cs, dcc=dcc)
    return gw, (dx.permute(0, 3, 1, 2) if need_x_grad else None), carry.permute(0, 3, 1, 2), cbuf.permute(0, 3, 1, 2)


def fuse_block(model):
    """The block that produces the recurrence's input (the `prefuse` tap), and the name of the tap that holds ITS input:
    `model.fucbst_layer[0]` reading `fu320` with any prior enabled, else `model.fust_layer[0]` reading the last ST block's
    output."""
    if model.num_cb:
        return model.fucbst_layer[0], "fu320"
    return model.fust_layer[0], "st%d" % (len(model.st_layer) - 1)


def _param_grad_tensors(blk):
    """`({name: .grad}, accumulate)` of a block whose nine gradients a backward writes: missing `.grad`s are created, zeroed
    when some but not all exist (the existing ones are added to, as `loss.backward()` would)."""
    params = dict(blk.named_parameters())
    acc = any(q.grad is not None for q in params.values())
    for q in params.values():
        if q.grad is None:
            q.grad = (torch.zeros_like if acc else torch.empty_like)(q, memory_format=torch.contiguous_format)
    return {n: q.grad for n, q in params.items()}, acc


def recurrence_step(model, x, cb, in_state, y_gaze, criterion=None, decoder=False, fuse=False, fust=False, ctx=False, nets=False,
                    st=False, srf=False, backbone=False, shallow=False, lstm=False):
    """One training step's forward and backward for the recurrence: `model(x, cb, in_state)` through the launch plan, the
    criterion (default `losses.loss_fu`) and its gradient, the decoder's input gradient and `twa_backward`.  Ends with
    `model.rnn.cell_list[0].rnn_conv.weight.grad` set -- or added to when it already exists, as `loss.backward()` would --
    and no other parameter touched.  Returns `(loss, out, [h_last.detach()])`, the forward's contract plus the loss.
    The model is in eval mode (every other stage is frozen, its BatchNorms folded); a model in training mode, CPU tensors,
    a precision other than 'f32' or -- without `lstm=True` -- `UAVSAL_LSTM` raise.  After `optimizer.step()` call `model.refresh_weights(model.rnn)`.
    `decoder=True`: the decoder `model.conv_out_st` is trained too (`decoder_backward`): its nine parameters' `.grad` are set
    as well, or added to, and the recurrence receives that path's `grad_h`; afterwards call
    `model.refresh_weights(model.rnn, model.conv_out_st)`.  The BatchNorms still use their running statistics.
    `fuse=True`: the fusion block in front of the recurrence (`fuse_block`) is trained too: `twa_backward` also returns the
    gradient of the recurrence's input, which `block_backward` carries to that block's nine parameters (`.grad` set, or added
    to); everything in front of the block stays frozen, and nothing of `prefuse` bypasses the recurrence, so the gradient is
    exact.  Refresh `model.fucbst_layer` (or `model.fust_layer` in a model without priors) afterwards as well.  Combines
    freely with `decoder=True`; the default call runs the launches -- and the copies of taps -- it always ran.
    `fust=True` (needs `fuse=True` and a model with at least one prior; without priors the `fuse` stage already IS
    `model.fust_layer[0]`): the block behind the priors, `model.fust_layer[0]`, is trained as well.  `block_backward` of the
    fusion block also returns the gradient of its input `fu320`, `fust_output_grad` carries it to fust_layer's output --
    directly and, with the context prior, through the frozen `fucb_layer`, upsample, `cxt_cb_prior` and chunk sum -- and a
    second `block_backward` to fust_layer's nine parameters (`.grad` set, or added to).  The ST blocks in front of it, the
    prior nets, `fucb_layer` and `cxt_cb_prior` stay frozen.  Refresh `model.fust_layer` afterwards as well.
    `ctx=True` (needs `fuse=True` and a model with at least one prior; independent of `fust`): the multi-prior path is trained
    as well -- `model.fucb_layer[0]` and, with the context prior, `model.cxt_cb_prior[1]` and `[0]` (`prior_path_blocks`): the
    same ONE walk of `prior_path_backward` that yields fust_layer's output gradient also forms their 9, or 27, parameter
    gradients (`.grad` set, or added to).  The gauss / ob prior nets stay frozen unless `nets` is given.  Refresh
    `model.fucb_layer` and `model.cxt_cb_prior` afterwards as well.
    `nets=True` (needs `fuse=True` and a gauss or ob prior; independent of `fust` and `ctx`): the prior nets `prior_nets(model)`
    are trained as well -- with it, the step sets the gradients of every parameter the reference's optimiser holds.  The walk
    hands out `g_cb` = d loss / d `cb192`, whose gauss and ob slices are the nets' output gradients; `prior_net_backward` forms
    each net's 18 parameter gradients (`.grad` set, or added to).  Static priors -- decided exactly as the forward decides
    them, `model.dedupe_priors and model._static(cb0, cb1, 1)` with more than one frame -- ran each net on ONE frame whose
    output every frame reads: the slice is summed over the frames (`frame_sum`) and the backward runs on one frame too; else
    it runs over all N frames.  Refresh `model.gauss_cb_layer` / `model.ob_cb_layer` afterwards as well (which also drops the
    engines' prior records, `model.refresh_weights`).
    `st=True` (needs `fuse=True`, and `fust=True` as well in a model with priors: the gradient must reach `fust_layer[0]`'s
    input): the ST blocks `model.st_layer` are trained as well -- what a user of the reference gets by deleting the two lines
    that freeze them (Demo_Train_Test.py:61-62).  The `block_backward` of `model.fust_layer[0]` also returns the gradient of
    its input, and `st_block_backward` walks from the last ST block to the first over the `st{i}` and `sfnet` taps (one
    sequence of all the call's frames, as `forward()` runs them; no input gradient at block 0: the backbone `sfnet` stays
    frozen), setting -- or adding to -- the `.grad` of the 27 parameters of every block.  Refresh `model.st_layer` afterwards
    as well.  A call without `st` runs the launches, and copies the taps, it always ran.
    `srf=True` (needs `st=True`, and so everything `st` needs): the SRF-Net head `srf_head(model)` is trained as well -- every
    parameter of `model.sfnet` the reference initialises itself; only the ImageNet `features` stay frozen.  ST block 0 is then
    walked with `need_x_grad=True`, and `srf_head_backward` carries its input gradient (d loss / d `taps["sfnet"]`) over the
    `c3` / `c4` / `c5` taps to the head's 42 parameters (`.grad` set, or added to); no gradient is formed for the taps
    themselves.  Refresh `*train.srf_head(model)` afterwards as well (not `model.sfnet`: the stem and `features[1]` cannot be
    refreshed in place, and the transposed-layout fused blocks only with `fused_t=True`).  A call without `srf` runs the launches, and copies the taps, it always ran.
    `backbone=True` (needs `srf=True`, and so everything `srf` needs): the deep backbone `backbone_blocks(model)` --
    MobileNetV2 `features[8:18]`, the ten blocks at 1/16 and 1/32 resolution -- is trained as well, what the reference's
    unfrozen form does (Demo_Train_Test.py:58 freezes only "to improve the training speed").  `srf_head_backward` then also
    returns the gradients of the `c4` / `c5` taps and `backbone_backward` walks blocks 17 .. 8 over the `c3` tap, setting -- or
    adding to -- the `.grad` of their 90 parameters.  `features[0..7]` stay frozen (`features[2:8]` unless `shallow` is given).
    Refresh `*train.backbone_blocks(model)` afterwards as well.  A call without `backbone` runs the launches it always ran.
    `shallow=True` (needs `backbone=True`, and so everything `backbone` needs): the shallow backbone `shallow_blocks(model)` --
    MobileNetV2 `features[2:8]`, the six blocks with an expand conv in front of the c3 tap and behind it -- is trained as well.
    `srf_head_backward` then also returns the gradient of the `c3` tap, `backbone_backward` the gradient of block 7's output,
    and `shallow_backward` walks blocks 7 .. 2 over the input frames `x`, setting -- or adding to -- the `.grad` of their 54
    parameters.  Only the stem and `features[1]` stay frozen.  Refresh `*train.shallow_blocks(model)` with `fused_t=True`
    afterwards as well.  A call without `shallow` runs the launches it always ran.
    `lstm=True` (opt-in, for a `UAVSAL_LSTM` model; with a ConvTWA model it raises before any launch): the recurrence is the
    reference's ConvLSTM ablation.  `in_state` is None or `[(h, c)]`, the forward runs through the plan as it always did, and
    `lstm_backward` stands where `twa_backward` stands (csrc/train_lstm.hip: `uavsal_lstm_scan`, `uavsal_lstm_gate_bwd`; the
    weight gradient is `uavsal_conv3_wgrad` at 1024 x 512), setting -- or adding to -- the `.grad` of the `[1024,512,3,3]`
    `rnn_conv.weight`.  Every other keyword works unchanged behind it: the stages hang off the recurrence's `grad_x` and
    `grad_h`, which are the same tensors in both models.  Returns `(loss, out, [h_last.detach(), c_last.detach()])`, the
    forward's contract for this model; refresh `model.rnn` as usual.  Without the keyword a `UAVSAL_LSTM` model raises, as it
    always did, and a `UAVSal` call runs the launches it always ran."""
    from . import losses as _losses
    criterion = criterion or _losses.loss_fu
    is_lstm = getattr(model, "rnn_type", "twa") != "twa"
    if is_lstm and not lstm:
        raise RuntimeError("recurrence_step covers the ConvTWA recurrence, not UAVSAL_LSTM")
    if lstm and not is_lstm:
        raise RuntimeError("lstm=True is for a UAVSAL_LSTM model (the ConvLSTM recurrence); this model's recurrence is ConvTWA")
    if fust and not (fuse and getattr(model, "num_cb", 0)):
        raise RuntimeError("fust=True needs fuse=True and a model with at least one prior (without priors the fuse stage "
                           "already is model.fust_layer[0])")
    if ctx and not (fuse and getattr(model, "num_cb", 0)):
        raise RuntimeError("ctx=True needs fuse=True and a model with at least one prior (without priors there is no "
                           "multi-prior path)")
    if nets and not (fuse and prior_nets(model)):
        raise RuntimeError("nets=True needs fuse=True and a model with the gauss or the ob prior (bias_type [0,0,1] and [0,0,0] "
                           "have no prior net)")
    if st and not (fuse and (fust or not getattr(model, "num_cb", 0))):
        raise RuntimeError("st=True needs fuse=True, and in a model with priors fust=True as well (the gradient reaches "
                           "model.st_layer through model.fust_layer[0]'s input)")
    if srf and not st:
        raise RuntimeError("srf=True needs st=True (and what st needs): the gradient reaches model.sfnet's head through the "
                           "input of model.st_layer[0]")
    if backbone and not srf:
        raise RuntimeError("backbone=True needs srf=True (and what srf needs): the gradient reaches the backbone blocks through "
                           "the c4 / c5 taps of model.sfnet's head")
    if shallow and not backbone:
        raise RuntimeError("shallow=True needs backbone=True (and what backbone needs): the gradient reaches the shallow blocks "
                           "through the c3 tap of model.sfnet's head and the input of features[8]")
    if model.training:
        raise RuntimeError("recurrence_step needs model.eval(): only the recurrence is trained, every BatchNorm stays folded")
    if model.precision != "f32":
        raise RuntimeError("recurrence_step supports precision 'f32' only, got %r" % (model.precision,))
    if not torch.is_tensor(x) or not x.is_cuda or not torch.is_tensor(y_gaze) or not y_gaze.is_cuda:
        raise RuntimeError("recurrence_step needs tensors on the MI355X (cuda) device; there is no CPU fallback")
    rc = model.rnn.cell_list[0].rnn_conv
    blk, src = fuse_block(model) if fuse else (None, None)
    taps = {src: None} if fuse else {}                               # (fu320 is read back on request only: engine.TAPS_ON_REQUEST)
    if fust or ctx or nets:
        taps["cb192"] = None                                         # (likewise)
    out, h_last = model(x, cb, in_state, taps=taps)
    pred = out.detach().requires_grad_(True)
    with torch.enable_grad():
        loss = criterion(pred, y_gaze)
        (g_y,) = torch.autograd.grad(loss, pred)
    dev = x.device
    cache = WeightCache(dev, model._wshared.setdefault(str(torch.device(dev)), {}))
    cl = torch.channels_last
    h_seq, x_seq = taps["rnn"].contiguous(memory_format=cl), taps["prefuse"].contiguous(memory_format=cl)
    if decoder:
        grads, acc = _param_grad_tensors(model.conv_out_st)
        grad_h, _ = decoder_backward(model.conv_out_st, h_seq, g_y, cache=cache, y=out, grads=grads, accumulate=acc)
    else:
        grad_h = decoder_input_grad(model.conv_out_st, h_seq, g_y, cache=cache, y=out)
    h0 = None if in_state is None else in_state[0]
    w = rc.weight
    had = w.grad is not None
    if not had:
        w.grad = torch.empty_like(w, memory_format=torch.contiguous_format)
    if lstm:
        h0, c0 = (None, None) if h0 is None else h0
        _, grad_x, _, _ = lstm_backward(x_seq, h_seq, h0, c0, w.detach(), grad_h, need_x_grad=bool(fuse), out=w.grad,
                                        accumulate=had, cache=cache, module=rc)
    else:
        _, grad_x, _ = twa_backward(x_seq, h_seq, h0, w.detach(), grad_h, need_x_grad=bool(fuse), out=w.grad, accumulate=had,
                                    cache=cache, module=rc)
    if fuse:
        grads, acc = _param_grad_tensors(blk)
        fu = taps[src].contiguous(memory_format=cl)
        grad_fu, _ = block_backward(blk, fu, grad_x, need_x_grad=bool(fust or ctx or nets or st), cache=cache, grads=grads,
                                    accumulate=acc)
        g_cb, g_st = None, grad_fu                                   # (without priors the fuse stage IS fust_layer[0])
        if ctx:
            pg = {n: _param_grad_tensors(b) for n, b in prior_path_blocks(model).items()}
            g, _, *g_cb = prior_path_backward(model, fu, taps["cb192"], grad_fu, cache=cache, grads={n: v[0] for n, v in pg.items()},
                                              accumulate={n: v[1] for n, v in pg.items()}, need_fust_grad=bool(fust),
                                              need_cb_grad=bool(nets))
        elif nets:
            g, _, *g_cb = prior_path_backward(model, fu, taps["cb192"], grad_fu, cache=cache, need_fust_grad=bool(fust),
                                              need_cb_grad=True)
        elif fust:
            g = fust_output_grad(model, fu, taps["cb192"], grad_fu, cache=cache)
        if nets:
            (g_cb,) = g_cb
            cbs = dict(zip(PRIOR_NETS, model._used_cb(cb)))
            static = bool(model.dedupe_priors and x.shape[0] > 1 and model._static(*model._used_cb(cb), 1))
            for i, (name, net) in enumerate(prior_nets(model).items()):
                go, c = g_cb[..., 64 * i:64 * i + 64], cbs[name]
                if static:                                           # the net ran on ONE frame that every frame reads
                    go, c = frame_sum(go), c[:1]
                pg = {k: _param_grad_tensors(b) for k, b in zip("01", net)}
                prior_net_backward(net, c, go, cache=cache, grads={k: v[0] for k, v in pg.items()},
                                   accumulate={k: v[1] for k, v in pg.items()})
        if fust:
            fb = model.fust_layer[0]
            grads, acc = _param_grad_tensors(fb)
            g_st, _ = block_backward(fb, taps["st%d" % (len(model.st_layer) - 1)].contiguous(memory_format=cl), g,
                                     need_x_grad=bool(st), cache=cache, grads=grads, accumulate=acc)
        if st:
            for i in range(len(model.st_layer) - 1, -1, -1):         # one sequence of all frames, as forward() runs them
                grads, acc = _param_grad_tensors(model.st_layer[i])
                xin = taps["st%d" % (i - 1)] if i else taps["sfnet"]
                g_st, _ = st_block_backward(model.st_layer[i], xin.contiguous(memory_format=cl), g_st, seq_len=x.shape[0],
                                            need_x_grad=i > 0 or bool(srf), cache=cache, grads=grads, accumulate=acc)
        if srf:
            hp = dict(model.sfnet.named_parameters())
            acc = any(hp[n].grad is not None for n in SRF_HEAD_PARAMS)
            for n in SRF_HEAD_PARAMS:
                if hp[n].grad is None:
                    hp[n].grad = (torch.zeros_like if acc else torch.empty_like)(hp[n], memory_format=torch.contiguous_format)
            ret = srf_head_backward(model.sfnet, taps["c3"], taps["c4"], taps["c5"], taps["sfnet"], g_st, cache=cache,
                                    grads={n: hp[n].grad for n in SRF_HEAD_PARAMS}, accumulate=acc, need_tap_grads=bool(backbone),
                                    **({"need_c3_grad": True} if shallow else {}))
        if backbone:
            feats = model.sfnet.features.features
            bp = {"%d.%s" % (i, n): q for i in range(BACKBONE_FIRST, BACKBONE_END) for n, q in feats[i].named_parameters()}
            acc = any(q.grad is not None for q in bp.values())
            for q in bp.values():
                if q.grad is None:
                    q.grad = (torch.zeros_like if acc else torch.empty_like)(q, memory_format=torch.contiguous_format)
            bret = backbone_backward(feats, taps["c3"], ret[1], ret[2], cache=cache, grads={n: q.grad for n, q in bp.items()},
                                     accumulate=acc, **({"need_x_grad": True} if shallow else {}))
        if shallow:
            sp = {"%d.%s" % (i, n): q for i in range(SHALLOW_FIRST, SHALLOW_END) for n, q in feats[i].named_parameters()}
            acc = any(q.grad is not None for q in sp.values())
            for q in sp.values():
                if q.grad is None:
                    q.grad = (torch.zeros_like if acc else torch.empty_like)(q, memory_format=torch.contiguous_format)
            shallow_backward(feats, x, ret[3], bret[1], cache=cache, grads={n: q.grad for n, q in sp.items()}, accumulate=acc)
    return loss.detach(), out, [t.detach() for t in h_last]
