"""The criterion of the reference's training script on the device: `loss_fu = 10 * KL - 2 * CC - NSS`
(loss_functions.py:43-50, 64-86) and its gradient with respect to the prediction, as fused HIP launches
(csrc/loss.hip: `uavsal_loss_fu` two launches, `uavsal_loss_fu_grad` one) instead of about sixty eager ones.

The functions take the reference's signatures and return its shapes, so they drop in as
`criterion = loss_fu` (Demo_Train_Test.py:66): `y_pred` `[B,1,h,w]`, `y_true` `[B,2,h,w]` (channel 0 the fixation
map in any scale -- the loss normalises; `preprocess_vidmaps` leaves 0..255 --, channel 1 the fixation points),
float32 on the GPU.  `loss_fu` / `loss_kl` are differentiable in `y_pred` (`loss.backward()`); the `metric_*`
values are plain numbers like everything computed without a gradient.  Sums are taken in double and rounded
once, in a fixed order: two calls return the same bits.  CPU tensors raise: this package has no CPU fallback.
`loss_ml` and `metric_sim` are not used by the reference's `train()` and are not provided."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L


def _check(y_pred, y_true):
    for name, t in (("y_pred", y_pred), ("y_true", y_true)):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4:
            raise RuntimeError("%s must be a float32 cuda tensor [B,C,h,w] (no CPU fallback)" % name)
    B, c, h, w = y_pred.shape
    if c != 1 or tuple(y_true.shape) != (B, 2, h, w) or y_true.device != y_pred.device:
        raise RuntimeError("expected y_pred [B,1,h,w] and y_true [B,2,h,w] on one device, got %r and %r" % (
            tuple(y_pred.shape), tuple(y_true.shape)))
    if B == 0:
        raise RuntimeError("an empty batch has no loss")
    return B, h * w


def _desc(y_pred, y_true, stats, weights):
    d = L.LossDesc()
    d.pred, d.truth, d.stats = y_pred.data_ptr(), y_true.data_ptr(), stats.data_ptr()
    d.n_img, d.n_pix = y_pred.shape[0], y_pred.shape[2] * y_pred.shape[3]
    d.w_kl, d.w_cc, d.w_nss = weights
    return d


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _forward(y_pred, y_true, weights):
    """`(out, stats, y_pred, y_true)`: `out` float32 `[4]` = (mean kl, mean cc, mean nss, weighted loss); `stats` double
    `[B, 16]`, what the backward reads; the two inputs as the dense tensors the launches read."""
    _check(y_pred, y_true)
    lib = L.load()
    y_pred, y_true = y_pred.detach().contiguous(), y_true.detach().contiguous()
    with torch.cuda.device(y_pred.device):
        stats = torch.empty((y_pred.shape[0], L.LOSS_NSTAT), dtype=torch.float64, device=y_pred.device)
        out = torch.empty((4,), dtype=torch.float32, device=y_pred.device)
        d = _desc(y_pred, y_true, stats, weights)
        d.out = out.data_ptr()
        L.check(lib.uavsal_loss_fu(C.byref(d), _stream(y_pred)), "uavsal_loss_fu")
    return out, stats, y_pred, y_true


def loss_grad(y_pred, y_true, stats, grad_out, weights=L.LOSS_FU_WEIGHTS):
    """`grad_out * d loss / d y_pred` `[B,1,h,w]` from the statistics a forward saved (`loss_components(...)[1]`):
    one launch.  `grad_out`: a float32 scalar tensor on the device (or a number)."""
    _check(y_pred, y_true)
    lib = L.load()
    y_pred, y_true = y_pred.detach().contiguous(), y_true.detach().contiguous()
    if not torch.is_tensor(grad_out):
        grad_out = torch.tensor(float(grad_out), dtype=torch.float32)
    grad_out = grad_out.detach().to(device=y_pred.device, dtype=torch.float32).reshape(1).contiguous()
    with torch.cuda.device(y_pred.device):
        grad = torch.empty_like(y_pred)
        d = _desc(y_pred, y_true, stats, weights)
        d.grad_out, d.grad = grad_out.data_ptr(), grad.data_ptr()
        L.check(lib.uavsal_loss_fu_grad(C.byref(d), _stream(y_pred)), "uavsal_loss_fu_grad")
    return grad


def loss_components(y_pred, y_true, weights=L.LOSS_FU_WEIGHTS):
    """`(out, stats)`: `out` float32 `[4]` on the device = (metric_kl, metric_cc, metric_nss, the weighted loss) of the
    batch, and the per-frame statistics `[B,16]` (double; columns 0..2 are the per-frame kl, cc and nss)."""
    out, stats, _, _ = _forward(y_pred, y_true, weights)
    return out, stats


class _Criterion(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y_pred, y_true, weights):
        out, stats, p, t = _forward(y_pred, y_true, weights)
        ctx.save_for_backward(p, t, stats)
        ctx.weights = weights
        return out[3]

    @staticmethod
    def backward(ctx, grad_out):
        p, t, stats = ctx.saved_tensors
        return loss_grad(p, t, stats, grad_out, ctx.weights), None, None


def loss_fu(y_pred, y_true):
    """10 * KL - 2 * CC - NSS, a 0-d tensor (loss_functions.py:43-50)."""
    return _Criterion.apply(y_pred, y_true, L.LOSS_FU_WEIGHTS)


def loss_kl(y_pred, y_true):
    """10 * KL (loss_functions.py:37-41)."""
    return _Criterion.apply(y_pred, y_true, L.LOSS_KL_WEIGHTS)


def loss_fu_dy(y_pred, y_true):
    """`loss_fu` of `[B,D,C,H,W]` clips, frames folded into the batch (loss_functions.py:52-62)."""
    if y_pred.dim() != 5 or y_true.dim() != 5:
        raise RuntimeError("loss_fu_dy takes y_pred [B,D,1,H,W] and y_true [B,D,2,H,W]")
    B, D, c, H, W = y_pred.shape
    return loss_fu(y_pred.reshape(B * D, c, H, W), y_true.reshape(B * D, 2, H, W))


def metric_kl(y_pred, y_true):
    """float32 `[1]` (loss_functions.py:64-69)."""
    return loss_components(y_pred, y_true)[0][0:1]


def metric_cc(y_pred, y_true):
    """float32 `[1]` (loss_functions.py:71-80)."""
    return loss_components(y_pred, y_true)[0][1:2]


def metric_nss(y_pred, y_true):
    """float32 `[1]` (loss_functions.py:82-86)."""
    return loss_components(y_pred, y_true)[0][2:3]
