"""What every training stage shares: the tensor checks, the one `uavsal_conv_gemm` launch, the gradient slots of a stage's
parameters and the weight-gradient products (`pix_gemm`: csrc/train_decoder.hip; `skinny_wgrad`: csrc/train_shallow.hip;
`conv3_wgrad`: csrc/train_srf.hip).  Tensors are float32 on the GPU with the logical shape `[T, C, h, w]`; a channels-last
tensor (NHWC in memory, or a channel slice of one) is read in place, anything else is copied once."""
import ctypes as C

import torch

from .. import _lib as L
from .. import packing as P
from ..ops import _nhwc_view, _stream

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


def _conv(lib, cache, x, conv, cout, taps, wslice=None, transposed=False, bn=None, act=L.ACT_NONE, res=None, tscale=None,
          epi=L.EPI_AFFINE, aux=None, out=None, out2=None, gate_interleave=0):
    """One `uavsal_conv_gemm` launch on the current stream (no synchronisation): `x` NHWC, the weights of `conv` (or of its
    transposed conv; `tscale`: with the folded scale of that BatchNorm in its rows) from `cache` in the layout the route of
    this launch takes.  `epi` with `aux` (and `out2`): a step of the recurrence as the launch's epilogue (`UAVSAL_EPI_TWA`:
    `res` = x_t, `aux` = the hoisted W_x half; `UAVSAL_EPI_LSTM`: `res` = c_{t-1}, `out2` = c_t, the weights' gate rows
    interleaved, `gate_interleave` = the hidden size); `out`: a dense NHWC tensor to write instead of a new one."""
    ap, lda, n, h, w, cin = _nhwc_view(x)
    if out is None:
        out = torch.empty((n, h, w, cout), dtype=torch.float32, device=x.device)
    d = L.ConvDesc()
    d.a, d.lda, d.a_img_stride = ap, lda, h * w
    d.out, d.ldc, d.o_img_stride = out.data_ptr(), out.shape[3], h * w
    if bn is not None:
        s, b = cache.affine(bn, cout)
        d.scale, d.bias = s.data_ptr(), b.data_ptr()
    if res is not None:
        rp, ldr, *_ = _nhwc_view(res)
        d.res, d.ldr, d.r_img_stride = rp, ldr, h * w
    if aux is not None:
        xp, ldx, *_ = _nhwc_view(aux)
        d.aux, d.ldx, d.x_img_stride = xp, ldx, h * w
    if out2 is not None:
        d.out2, d.ld2 = out2.data_ptr(), out2.shape[3]
    d.n_img, d.H, d.W, d.Cin, d.Cout, d.taps = n, h, w, cin, cout, taps
    d.prec, d.act, d.epi, d.tile = L.PREC["f32"], act, epi, 0
    d.w = 1 << 20
    rt = L.conv_route(lib, d)
    layout = P.conv_weight_layout("f32", False, False, rt.tile, 3 if taps == 9 else 1)
    if tscale is not None:
        wp = cache.conv_t_scaled(conv, tscale, layout)
    else:
        wp = cache.conv_t(conv, wslice, layout) if transposed else cache.conv(conv, wslice, gate_interleave, layout)
    d.w = wp.data_ptr()
    L.check(lib.uavsal_conv_gemm(C.byref(d), _stream(x)), "uavsal_conv_gemm")
    return out


def _block_grad_out(grad_out, x, cout, stride=1):
    T, hh, ww, _ = x.shape
    hh, ww = (hh - 1) // stride + 1, (ww - 1) // stride + 1
    if (not torch.is_tensor(grad_out) or not grad_out.is_cuda or grad_out.dtype != torch.float32 or grad_out.device != x.device
            or tuple(grad_out.shape) != (T, cout, hh, ww)):
        raise RuntimeError("grad_out must be a float32 cuda tensor [%d,%d,%d,%d]" % (T, cout, hh, ww))
    return _nhwc(grad_out, "grad_out", cout)


def _dense_nhwc(name, what, *ts):
    if not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.is_contiguous() for t in ts):
        raise RuntimeError("%s: %s must be dense float32 NHWC cuda tensors" % (name, what))


def _dense(name, what, t, shape, dev):
    if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.device == dev and tuple(t.shape) == tuple(shape)
            and t.is_contiguous()):
        raise RuntimeError("%s: %s must be a dense float32 %r tensor on the device" % (name, what, list(shape)))


def _grad_slots(params, out, accumulate, arg):
    """The tensors a backward writes the gradients of `params` (an ordered `{name: parameter}`) into: `out`, such a dict of
    dense tensors, checked -- or, None, allocated in the order of `params`.  `arg`: what the caller's signature calls `out`
    (`"out"` or `"grads"`).  The caller has compared the names with its own list."""
    if out is None:
        if accumulate:
            raise RuntimeError("accumulate needs `%s`" % arg)
        out = {n: torch.empty_like(q, memory_format=torch.contiguous_format) for n, q in params.items()}
    for n, q in params.items():
        t = out.get(n)
        if (not torch.is_tensor(t) or t.shape != q.shape or t.dtype != torch.float32 or t.device != q.device
                or not t.is_contiguous()):
            raise RuntimeError("%s[%r] must be a dense float32 tensor of the parameter's shape on its device" % (arg, n))
    return out


def _param_grad_tensors(params):
    """`({name: .grad}, accumulate)` of the parameters `params` (`{name: parameter}`) whose gradients a backward writes:
    missing `.grad`s are created, zeroed when some but not all exist (the existing ones are added to, as `loss.backward()`
    would)."""
    acc = any(q.grad is not None for q in params.values())
    for q in params.values():
        if q.grad is None:
            q.grad = (torch.zeros_like if acc else torch.empty_like)(q, memory_format=torch.contiguous_format)
    return {n: q.grad for n, q in params.items()}, acc


_FLAT_TEXTS = ("out must be a dense float32 tensor of %d x %d elements on the device",
               "rowdot needs a dense float32 `w` of %d x %d elements and a dense float64 [%d] on the device")
_TAPS_TEXTS = ("out must be a dense float32 [%d,%d,3,3] tensor on the device",
               "rowdot needs a dense float32 `w` [%d,%d,3,3] and a dense float64 [%d] on the device")


def _wgrad_launch(lib, fn, who, k, a, b, sa, sb, out, row_scale, w, rowdot, accumulate, taps=False, refuse=None, guard=False):
    """What the three weight-gradient products share: `k` is the descriptor of the library call `fn` with its operands and
    sizes set, `a` `[..., M]` and `b` `[..., N]` the operands with the NHWC shapes `sa`, `sb`.  Checks that they cover the
    same pixels, `out` (allocated when None: `[M, N]`, with `taps` `[M, N, 3, 3]`), `row_scale` and `w` + `rowdot`, asks the
    library for the workspace, allocates it and launches on the stream of `a`.  `refuse`: the message of the caller's own
    precondition when it is not met (raised behind the same-pixels check); `guard`: launch inside `torch.cuda.device`."""
    M, N = sa[3], sb[3]
    if sa[:3] != sb[:3] or a.device != b.device:
        raise RuntimeError("%s must cover the same pixels on one device" % who)
    if refuse:
        raise RuntimeError(refuse)
    dev = a.device
    out_text, w_text = _TAPS_TEXTS if taps else _FLAT_TEXTS
    if out is None:
        if accumulate:
            raise RuntimeError("accumulate needs `out`")
        out = torch.empty((M, N, 3, 3) if taps else (M, N), dtype=torch.float32, device=dev)
    if ((tuple(out.shape) != (M, N, 3, 3) if taps else out.numel() != M * N) or out.dtype != torch.float32 or out.device != dev
            or not out.is_contiguous()):
        raise RuntimeError(out_text % (M, N))
    if row_scale is not None:
        if row_scale.dtype != torch.float32 or row_scale.device != dev or row_scale.numel() < M or not row_scale.is_contiguous():
            raise RuntimeError("row_scale must be a dense float32 vector of at least %d elements on the device" % M)
        k.row_scale = row_scale.data_ptr()
    if rowdot is not None:
        if (w is None or (tuple(w.shape) != (M, N, 3, 3) if taps else w.numel() != M * N) or not w.is_contiguous()
                or w.dtype != torch.float32 or w.device != dev
                or rowdot.dtype != torch.float64 or rowdot.numel() != M or not rowdot.is_contiguous() or rowdot.device != dev):
            raise RuntimeError(w_text % (M, N, M))
        k.w, k.rowdot = w.data_ptr(), rowdot.data_ptr()
    k.out = out.data_ptr()
    nbytes = int(getattr(lib, fn + "_workspace_bytes")(C.byref(k)))
    if nbytes <= 0:
        L.check(-3, fn)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    k.ws, k.ws_bytes = ws.data_ptr(), nbytes
    if guard:
        with torch.cuda.device(dev):
            L.check(getattr(lib, fn)(C.byref(k), _stream(a)), fn)
    else:
        L.check(getattr(lib, fn)(C.byref(k), _stream(a)), fn)
    return out


def pix_gemm(a, b, out=None, row_scale=None, w=None, rowdot=None, accumulate=False, tails32=False):
    """`uavsal_pix_gemm` on the current stream: `a` `[..., M]`, `b` `[..., N]` NHWC tensors of the same pixels (channel slices
    are read in place) -> `out[m][n] = row_scale[m] sum_p a[p][m] b[p][n]` (dense `[M, N]`; `accumulate`: added to `out`), and
    with `w` `[M, N]` and `rowdot` (float64 `[M]`) `rowdot[m] = sum_n w[m][n] G[m][n]`.  Two launches, no synchronisation.
    `tails32=True`: every M, N multiple of 32 the default call refuses is taken too (the weight gradients of the backbone
    blocks: quarter-tile tails, shares of 128-pixel units; include/uavsal_hip.h); what the default takes keeps its bits."""
    lib = L.load()
    ap, lda, *sa = _nhwc_view(a)
    bp, ldb, *sb = _nhwc_view(b)
    k = L.PixGemmDesc()
    k.a, k.lda, k.b, k.ldb = ap, lda, bp, ldb
    k.K, k.M, k.N, k.accumulate = sa[0] * sa[1] * sa[2], sa[3], sb[3], int(bool(accumulate))
    k.tails32, k.ldw, k.ldo = int(bool(tails32)), (sb[3] if rowdot is not None else 0), sb[3]
    return _wgrad_launch(lib, "uavsal_pix_gemm", "pix_gemm: a and b", k, a, b, sa, sb, out, row_scale, w, rowdot, accumulate)


def skinny_wgrad(a, b, out=None, row_scale=None, w=None, rowdot=None, accumulate=False):
    """`uavsal_skinny_wgrad` on the current stream: `pix_gemm`'s arguments and results for the skinny products it refuses,
    M and N multiples of 8 with `min(M, N) <= 32` and `max(M, N) <= 192` (the 1x1 weight gradients of MobileNetV2
    `features[2:8]`: 96 x 16, 144 x 24, 24 x 96, 24 x 144, 32 x 144).  One pass over both operands, a wave per share of the
    pixels (csrc/train_shallow.hip; the partition is stated in include/uavsal_hip.h).  Two launches, no synchronisation."""
    lib = L.load()
    ap, lda, *sa = _nhwc_view(a)
    bp, ldb, *sb = _nhwc_view(b)
    k = L.SkinnyWgradDesc()
    k.a, k.lda, k.b, k.ldb = ap, lda, bp, ldb
    k.K, k.M, k.N, k.accumulate = sa[0] * sa[1] * sa[2], sa[3], sb[3], int(bool(accumulate))
    k.ldw, k.ldo = (sb[3] if rowdot is not None else 0), sb[3]
    return _wgrad_launch(lib, "uavsal_skinny_wgrad", "skinny_wgrad: a and b", k, a, b, sa, sb, out, row_scale, w, rowdot,
                         accumulate, guard=True)


def conv3_wgrad(g, x, out=None, row_scale=None, w=None, rowdot=None, accumulate=False):
    """`uavsal_conv3_wgrad` on the current stream: `g` dense NHWC `[n,h,w,Co]`, `x` an NHWC view `[n,h,w,Ci]` of the same pixels
    (a channel slice is read in place) -> `out[co][ci][ky][kx] = row_scale[co] sum_p g[p][co] x[p + (ky-1, kx-1)][ci]` (dense
    `[Co,Ci,3,3]`, zero outside the picture, never across frames; `accumulate`: added to `out`), and with `w` `[Co,Ci,3,3]` and
    `rowdot` (float64 `[Co]`) `rowdot[co] = sum w[co] G[co]`.  Co % 128 == 0, Ci % 64 == 0.  Two launches, no synchronisation."""
    lib = L.load()
    _dense_nhwc("conv3_wgrad", "g", g)
    xp, ldx, *xs = _nhwc_view(x)
    n, hh, ww, co = g.shape
    ci = xs[3]
    k = L.Conv3WgradDesc()
    k.g, k.x, k.ldx = g.data_ptr(), xp, ldx
    k.n_img, k.H, k.W, k.Co, k.Ci, k.accumulate = n, hh, ww, co, ci, int(bool(accumulate))
    refuse = None
    if co % 128 or ci % 64:
        refuse = "conv3_wgrad takes Co %% 128 == 0 and Ci %% 64 == 0, got Co = %d, Ci = %d" % (co, ci)
    return _wgrad_launch(lib, "uavsal_conv3_wgrad", "conv3_wgrad: g and x", k, g, x, list(g.shape), xs, out, row_scale, w, rowdot,
                         accumulate, taps=True, refuse=refuse)
