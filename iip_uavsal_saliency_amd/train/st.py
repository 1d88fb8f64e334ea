"""The ST blocks `model.st_layer`, the seventh stage -- what deleting the reference's lines that freeze them gives
(Demo_Train_Test.py:61-62; the first thing to unfreeze on a new dataset) -- (`st_block_backward`; csrc/train_st.hip:
`uavsal_cbr_sums`, `uavsal_cbr_finish`, `uavsal_tdiff_bwd`): the two inverted-residual blocks of an ST block go through the
walks of block.py (`block_param_grads` takes the temporal sub-block's 64 -> 384 -> 32, `uavsal_pix_gemm` its 32-wide side),
the three 1x1 conv + BatchNorm + ReLU6 stages through `cbr_backward` and the temporal difference through `tdiff_bwd`.
`recurrence_step(st=True)` (needs `fuse=True`, and `fust=True` as well in a model with priors: the gradient must reach
`fust_layer[0]`'s input): the `block_backward` of `model.fust_layer[0]` also returns the gradient of its input, and
`st_block_backward` walks from the last ST block to the first over the `st{i}` and `sfnet` taps (one sequence of all the
call's frames, as `forward()` runs them; no input gradient at block 0: the backbone `sfnet` stays frozen), setting -- or
adding to -- the `.grad` of the 27 parameters of every block.  Refresh `model.st_layer` afterwards as well."""
import ctypes as C

import torch

from .. import _lib as L
from ..ops import _nhwc_view, _stream
from ..ops import tdiff as _tdiff
from ..weights import WeightCache
from ._common import _block_grad_out, _conv, _grad_slots, _nhwc, pix_gemm
from .block import BLOCK_PARAMS, _block_backward, _block_parts, _block_recompute, _input_grad, _input_grad_parts, _param_grad_parts
from .block import block_param_grads
from .ctx import tsum_bwd

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


def cbr_backward(conv, bn, x, y, grad_out, need_x_grad=True, cache=None, grads=None, accumulate=False):
    """Backward of ONE 1x1 conv + BatchNorm + ReLU6 (`BasicConv2d`, eval mode: the BatchNorm on its running statistics, which
    are not updated), teacher-forced: `x` `[N,Cin,h,w]` its input, `y` an NHWC view `[N,h,w,C]` of its own activation (before
    any residual is added), `grad_out` `[N,C,h,w]` = d loss / d output.  Returns `(grad_x [N,Cin,h,w] | None, grads)`; `grads`
    keyed by `ST_CBR_PARAMS` (W, gamma, beta), the values `torch.autograd` gives, written into the given dict of dense tensors or
    with `accumulate` added to it.  `uavsal_cbr_sums` forms `gp = grad_out * 1[0 < y < 6]` and its channel sums,
    `uavsal_pix_gemm` `s[c] G[c][j]` and the row dots, `uavsal_cbr_finish` beta and gamma (from the UNSCALED sums), and
    `grad_x = gp . (diag(s) W)` is one GEMM whose transposed weights carry s in their rows (`WeightCache.conv_t_scaled`).
    Accepted: Cin % 32 == 0, C % 32 == 0.  Four launches (+ the GEMM), on the current stream, no synchronisation."""
    lib = L.load()
    return _cbr_walk(lib, _cbr_parts(conv, bn), pix_gemm, 1, conv, bn, x, y, grad_out, need_x_grad, cache, grads, accumulate)


def _cbr_backward(conv, bn, x, y, grad_out, need_x_grad, cache, grads, accumulate, res=None):
    """`cbr_backward`; `res`: an NHWC tensor the `grad_x` GEMM adds (`st_block_backward`)."""
    lib = L.load()
    return _cbr_walk(lib, _cbr_parts(conv, bn), pix_gemm, 1, conv, bn, x, y, grad_out, need_x_grad, cache, grads, accumulate, res)


def _cbr_walk(lib, dims, wgrad, taps, conv, bn, x, y, grad_out, need_x_grad, cache, grads, accumulate, res=None):
    """The body of `cbr_backward` and of `conv3_backward` (srf.py): `dims` the checked stage's `(Cin, Cout)`, `wgrad` its
    weight-gradient product (`pix_gemm`, `conv3_wgrad`), `taps` those of the conv that forms `grad_x` (1, 9)."""
    cin, cout = dims
    xn = _nhwc(x, "x", cin)
    go = _block_grad_out(grad_out, xn, cout)
    dev = xn.device
    if (not torch.is_tensor(y) or y.dtype != torch.float32 or y.device != dev or tuple(y.shape) != tuple(go.shape)):
        raise RuntimeError("y must be a float32 NHWC view %r on the device of x" % (tuple(go.shape),))
    params = dict(zip(ST_CBR_PARAMS, (conv.weight, bn.weight, bn.bias)))
    grads = _grad_slots(params, grads, accumulate, "grads")
    if any(q.device != dev or not q.is_contiguous() for q in params.values()):
        raise RuntimeError("the parameters must be dense tensors on the device of `x`")
    with torch.cuda.device(dev):
        cache = cache or WeightCache(dev, {})
        s = cache.affine(bn, cout)[0]
        r, mu = cache.bn_stats(bn)
        gp, ws, slabs = cbr_sums(go, y)
        rowdot = torch.empty(cout, dtype=torch.float64, device=dev)
        wgrad(gp, xn, out=grads[ST_CBR_PARAMS[0]], row_scale=s, w=conv.weight.detach(), rowdot=rowdot, accumulate=accumulate)
        k = L.CbrFinishDesc()
        k.ws, k.ws_bytes, k.rowdot, k.r, k.mu = ws.data_ptr(), ws.numel() * 8, rowdot.data_ptr(), r.data_ptr(), mu.data_ptr()
        k.g_gamma, k.g_beta = grads[ST_CBR_PARAMS[1]].data_ptr(), grads[ST_CBR_PARAMS[2]].data_ptr()
        k.C, k.slabs, k.accumulate = cout, slabs, int(bool(accumulate))
        L.check(lib.uavsal_cbr_finish(C.byref(k), _stream(xn)), "uavsal_cbr_finish")
        g = _conv(lib, cache, gp, conv, cin, taps, tscale=bn, res=res) if need_x_grad else None
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
    params = dict(block.named_parameters())
    if sorted(params) != sorted(ST_BLOCK_PARAMS):
        raise RuntimeError("the ST block's parameters must be %r" % (ST_BLOCK_PARAMS,))
    grads = _grad_slots({n: params[n] for n in ST_BLOCK_PARAMS}, grads, accumulate, "grads")      # raise before anything is launched
    sub_g = lambda prefix, names: {n: grads[prefix + n] for n in names}   # noqa: E731
    g_sp, g_red, g_sub, g_last, g_stl = (sub_g(p, names) for p, names in ST_BLOCK_PARTS)
    nchw = lambda t: t.permute(0, 3, 1, 2)                                # noqa: E731
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
