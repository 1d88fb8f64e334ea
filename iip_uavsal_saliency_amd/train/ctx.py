"""The multi-prior path behind `model.fust_layer[0]` in a model with priors (csrc/train_ctx.hip: `uavsal_ir_bwd_s2`,
`uavsal_bilinear_ac_bwd`, `uavsal_tsum_bwd`, `uavsal_ir_sums_s2`): ONE walk, `prior_path_backward`, serves two stages.
The fourth, `recurrence_step(fust=True)` (needs `fuse=True` and a model with at least one prior; without priors the `fuse`
stage already IS `model.fust_layer[0]`): `block_backward` of the fusion block also returns the gradient of its input `fu320`,
`fust_output_grad` carries it to fust_layer's output -- directly and, with the context prior, through the frozen `fucb_layer`,
upsample, `cxt_cb_prior` and chunk sum -- and a second `block_backward` to fust_layer's nine parameters (`.grad` set, or added
to).  The ST blocks in front of it, the prior nets, `fucb_layer` and `cxt_cb_prior` stay frozen.  Refresh `model.fust_layer`
afterwards as well.
The fifth, `recurrence_step(ctx=True)` (needs `fuse=True` and a model with at least one prior; independent of `fust`): the
path itself is trained -- `model.fucb_layer[0]` and, with the context prior, `model.cxt_cb_prior[1]` and `[0]`
(`prior_path_blocks`): the same walk hands each block's tensors to `block_param_grads`, which takes 64 output channels
(`uavsal_pix_gemm` with M a multiple of 64) and stride 2 (`uavsal_ir_sums_s2`), and forms their 9, or 27, parameter gradients
(`.grad` set, or added to).  The gauss / ob prior nets stay frozen unless `nets` is given.  Refresh `model.fucb_layer` and
`model.cxt_cb_prior` afterwards as well."""
import ctypes as C

import torch

from .. import _lib as L
from ..ops import _nhwc_view, _stream
from ..ops import tsum as _tsum
from ..weights import WeightCache
from ._common import HID, _block_grad_out, _conv, _nhwc
from .block import _block_recompute, _block_slots, _input_grad, _input_grad_parts, _param_grad_parts, block_param_grads


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
            _block_slots(blocks[n], grads[n], acc)              # raise before anything is launched
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
