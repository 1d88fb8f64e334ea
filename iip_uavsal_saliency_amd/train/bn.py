"""BatchNorm on BATCH statistics -- `nn.BatchNorm2d` in training mode -- for a general NHWC tensor: thin wrappers of the
kernels of csrc/train_bn.hip (`uavsal_bn_stats`, `uavsal_bn_apply`, `uavsal_bn_bwd_sums`, `uavsal_bn_bwd_apply`,
`uavsal_dw_wgrad`; include/uavsal_hip.h states the formulas and the order of every sum).  Teacher-forced on given tensors,
as `st.cbr_sums` is; `decoder.decoder_forward_batch` / `decoder_backward_batch` compose them into the decoder's training-mode
forward and backward, and block_bn.py an inverted-residual block's (`uavsal_bn_apply_res`: `bn_apply(res=)`).  `u` is an NHWC
view `[n,h,w,C]` (a channel slice is read in place), `C % 4 == 0` or `C == 1`; the statistics run over all `n*h*w` pixels of
the call.  Every call runs on the current stream without synchronisation; two calls return the same bits."""
import ctypes as C
from typing import NamedTuple

import torch

from .. import _lib as L
from ..ops import _nhwc_view, _stream

ACTS = {None: L.ACT_NONE, "none": L.ACT_NONE, "relu6": L.ACT_RELU6, "sigmoid": L.ACT_SIGMOID}


class BnFold(NamedTuple):
    """What `bn_stats` returns, fp32 `[C]` each: the batch mean, the biased batch variance, `r = 1 / sqrt(var + eps)`, and
    the fold `s = gamma r`, `b = beta - mu s` that `bn_apply` and the backward take."""
    mu: torch.Tensor
    var: torch.Tensor
    r: torch.Tensor
    s: torch.Tensor
    b: torch.Tensor


def _act(act):
    if act not in ACTS:
        raise RuntimeError("act must be one of None, 'relu6', 'sigmoid', got %r" % (act,))
    return ACTS[act]


def _view(t, name):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4:
        raise RuntimeError("%s must be a float32 cuda NHWC view [n,h,w,C] (no CPU fallback)" % name)
    return _nhwc_view(t)


def _vec(t, name, c, dev, dtype=torch.float32):
    if not torch.is_tensor(t) or t.dtype != dtype or t.device != dev or t.numel() != c or not t.is_contiguous():
        raise RuntimeError("%s must be a dense %s tensor of %d elements on the device" % (name, str(dtype).split(".")[-1], c))
    return t.data_ptr()


def slabs(n, h, w):
    """`(slabs, picture rows per slab)` of every reduction of csrc/train_bn.hip over `n` frames of `h` x `w`: the library's own
    answer, a function of the shape alone."""
    lib = L.load()
    return int(lib.uavsal_bn_slabs(n, h, w)), int(lib.uavsal_bn_slab_rows(n, h, w))


def bump_version(*tensors):
    """Tell torch that a kernel wrote `tensors` in place (their version counters move, as an in-place torch op's would):
    `model._check_weights` / `refresh_weights` decide from those counters what was modified."""
    for t in tensors:
        torch.autograd.graph.increment_version(t)


def bn_stats(u, weight, bias, eps, running_mean=None, running_var=None, momentum=0.1):
    """`uavsal_bn_stats`: the batch statistics of `u` and the fold with `weight` (gamma) and `bias` (beta) -> `BnFold`.
    With `running_mean` / `running_var` (the module's buffers) those are blended IN PLACE on the device, in double, rounded
    once: `(1 - momentum) running + momentum batch`, the variance unbiased (`P / (P - 1)`); their version counters move.
    Two launches."""
    lib = L.load()
    up, ld, n, hh, ww, c = _view(u, "u")
    dev = u.device
    k = L.BnStatsDesc()
    k.u, k.ld, k.gamma, k.beta = up, ld, _vec(weight.detach(), "weight", c, dev), _vec(bias.detach(), "bias", c, dev)
    if (running_mean is None) != (running_var is None):
        raise RuntimeError("bn_stats takes running_mean and running_var together")
    if running_mean is not None:
        if momentum is None:
            raise RuntimeError("bn_stats: momentum=None (the cumulative average) is not covered")
        k.running_mean, k.running_var = _vec(running_mean, "running_mean", c, dev), _vec(running_var, "running_var", c, dev)
    k.eps, k.momentum = float(eps), float(momentum if momentum is not None else 0.0)
    k.n_img, k.H, k.W, k.C = n, hh, ww, c
    nbytes = int(lib.uavsal_bn_stats_workspace_bytes(C.byref(k)))
    if nbytes <= 0:
        L.check(-3, "uavsal_bn_stats")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    out = torch.empty((5, c), dtype=torch.float32, device=dev)
    k.ws, k.ws_bytes = ws.data_ptr(), nbytes
    k.mu, k.var, k.r, k.s, k.b = (out[i].data_ptr() for i in range(5))
    with torch.cuda.device(dev):
        L.check(lib.uavsal_bn_stats(C.byref(k), _stream(u)), "uavsal_bn_stats")
    if running_mean is not None:
        bump_version(running_mean, running_var)
    return BnFold(*out.unbind(0))


def bn_apply(u, fold, act=None, dot_w=None, res=None):
    """`uavsal_bn_apply`: `act(s u + b)` as a dense NHWC tensor `[n,h,w,C]`; with `dot_w` `[C]` the dot of that tensor with
    `dot_w` over the channels instead, dense `[n,h,w,1]` (the activated tensor is not stored).  `res` (an NHWC view like `u`,
    `C % 4 == 0`; not with `dot_w`): `uavsal_bn_apply_res`, `act(s u + b) + res`, the sum rounded once more -- the residual
    of an inverted-residual block behind its last BatchNorm.  One launch."""
    lib = L.load()
    up, ld, n, hh, ww, c = _view(u, "u")
    dev = u.device
    if res is not None:
        if dot_w is not None:
            raise RuntimeError("bn_apply: res and dot_w do not combine")
        rp, ldr, *rs = _view(res, "res")
        if rs != [n, hh, ww, c] or res.device != dev:
            raise RuntimeError("res must be [%d,%d,%d,%d] on the device of u" % (n, hh, ww, c))
        q = L.BnApplyResDesc()
        q.u, q.ld, q.s, q.b = up, ld, _vec(fold.s, "fold.s", c, dev), _vec(fold.b, "fold.b", c, dev)
        q.res, q.ldr = rp, ldr
        out = torch.empty((n, hh, ww, c), dtype=torch.float32, device=dev)
        q.out, q.n_pix, q.C, q.act = out.data_ptr(), n * hh * ww, c, _act(act)
        with torch.cuda.device(dev):
            L.check(lib.uavsal_bn_apply_res(C.byref(q), _stream(u)), "uavsal_bn_apply_res")
        return out
    k = L.BnApplyDesc()
    k.u, k.ld, k.s, k.b = up, ld, _vec(fold.s, "fold.s", c, dev), _vec(fold.b, "fold.b", c, dev)
    if dot_w is not None:
        k.dot_w = _vec(dot_w, "dot_w", c, dev)
    out = torch.empty((n, hh, ww, 1 if dot_w is not None else c), dtype=torch.float32, device=dev)
    k.out, k.n_pix, k.C, k.act = out.data_ptr(), n * hh * ww, c, _act(act)
    with torch.cuda.device(dev):
        L.check(lib.uavsal_bn_apply(C.byref(k), _stream(u)), "uavsal_bn_apply")
    return out


def _bwd_desc(g, u, fold, act, sums):
    up, ld, n, hh, ww, c = _view(u, "u")
    dev = u.device
    k = L.BnBwdDesc()
    if isinstance(g, tuple):                                           # rank-one: (g_pix [n,h,w(,1)], g_chan [C])
        g_pix, g_chan = g
        k.g_pix, k.g_chan = _vec(g_pix, "g[0]", n * hh * ww, dev), _vec(g_chan, "g[1]", c, dev)
    else:
        gp, ldg, *gs = _view(g, "g")
        if gs != [n, hh, ww, c] or g.device != dev:
            raise RuntimeError("g must be [%d,%d,%d,%d] on the device of u" % (n, hh, ww, c))
        k.g, k.ldg = gp, ldg
    k.u, k.ld = up, ld
    k.s, k.b, k.mu, k.r = (_vec(t, "fold.%s" % f, c, dev) for f, t in zip("sbmr", (fold.s, fold.b, fold.mu, fold.r)))
    k.sums = _vec(sums, "sums", 2 * c, dev, torch.float64)
    k.n_img, k.H, k.W, k.C, k.act = n, hh, ww, c, _act(act)
    return k, (n, hh, ww, c), dev


def bn_bwd_sums(g, u, fold, act=None, g_weight=None, g_bias=None, g_w=None, accumulate=False):
    """`uavsal_bn_bwd_sums`: `g` = d loss / d act(a), an NHWC view like `u` -- or a tuple `(g_pix [n,h,w], g_chan [C])` for
    the rank-one `g[p][c] = g_pix[p] g_chan[c]` (the adjoint of a projection to one channel, never stored).  Returns `sums`,
    float64 `[2, C]`: d beta, d gamma -- what `bn_bwd_apply` takes.  `g_weight`, `g_bias` (dense `[C]`): d gamma and d beta
    are written there as well, or with `accumulate` added; `g_w` (rank-one only): likewise `sum_p g_pix[p] act(a)[p][c]`, the
    gradient of the projection's weight.  Two launches."""
    lib = L.load()
    c = u.shape[-1]
    sums = torch.empty((2, c), dtype=torch.float64, device=u.device)
    k, _, dev = _bwd_desc(g, u, fold, act, sums)
    if g_w is not None and not isinstance(g, tuple):
        raise RuntimeError("bn_bwd_sums: g_w belongs to the rank-one gradient (g a tuple)")
    for name, t in (("g_gamma", g_weight), ("g_beta", g_bias), ("g_w", g_w)):
        if t is not None:
            setattr(k, name, _vec(t, name, c, dev))
    k.accumulate = int(bool(accumulate))
    nbytes = int(lib.uavsal_bn_bwd_workspace_bytes(C.byref(k)))
    if nbytes <= 0:
        L.check(-3, "uavsal_bn_bwd_sums")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    k.ws, k.ws_bytes = ws.data_ptr(), nbytes
    with torch.cuda.device(dev):
        L.check(lib.uavsal_bn_bwd_sums(C.byref(k), _stream(u)), "uavsal_bn_bwd_sums")
    return sums


def bn_bwd_apply(g, u, fold, sums, act=None):
    """`uavsal_bn_bwd_apply`: `g_u = s (g_a - d beta / P - xh d gamma / P)` as a dense NHWC tensor like `u`, from the `sums` of
    `bn_bwd_sums` on the same arguments.  One launch."""
    lib = L.load()
    k, shape, dev = _bwd_desc(g, u, fold, act, sums)
    gu = torch.empty(shape, dtype=torch.float32, device=dev)
    k.gu = gu.data_ptr()
    with torch.cuda.device(dev):
        L.check(lib.uavsal_bn_bwd_apply(C.byref(k), _stream(u)), "uavsal_bn_bwd_apply")
    return gu


def dw_wgrad(g, e, out=None, accumulate=False):
    """`uavsal_dw_wgrad`: the weight gradient of a depthwise 3x3 (stride 1, padding 1) from `g` = d loss / d its output and
    `e` its input (NHWC views of one shape): `out[c][ky][kx] = sum_p g[p][c] e[p + (ky-1, kx-1)][c]`, zero outside the picture,
    never across frames; `out` dense with `C * 9` elements (`[C,1,3,3]`), written or with `accumulate` added to.  Two launches."""
    lib = L.load()
    gp, ldg, *gs = _view(g, "g")
    ep, lde, *es = _view(e, "e")
    if gs != es or g.device != e.device:
        raise RuntimeError("dw_wgrad: g and e must have one shape [n,h,w,C] on one device")
    n, hh, ww, c = gs
    dev = g.device
    if out is None:
        if accumulate:
            raise RuntimeError("accumulate needs `out`")
        out = torch.empty((c, 1, 3, 3), dtype=torch.float32, device=dev)
    k = L.DwWgradDesc()
    k.g, k.ldg, k.e, k.lde, k.out = gp, ldg, ep, lde, _vec(out, "out", c * 9, dev)
    k.n_img, k.H, k.W, k.C, k.accumulate = n, hh, ww, c, int(bool(accumulate))
    nbytes = int(lib.uavsal_dw_wgrad_workspace_bytes(C.byref(k)))
    if nbytes <= 0:
        L.check(-3, "uavsal_dw_wgrad")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    k.ws, k.ws_bytes = ws.data_ptr(), nbytes
    with torch.cuda.device(dev):
        L.check(lib.uavsal_dw_wgrad(C.byref(k), _stream(g)), "uavsal_dw_wgrad")
    return out
