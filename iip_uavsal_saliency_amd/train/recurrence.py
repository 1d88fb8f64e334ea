"""Back-propagation through time over the recurrence `model.rnn`, the first stage (csrc/train.hip: `uavsal_twa_gate_bwd`,
`uavsal_twa_wgrad`; csrc/train_lstm.hip: `uavsal_lstm_scan`, `uavsal_lstm_gate_bwd`).
`UAVSal`: the Temporal Weighted Average recurrence (reference model_convlstm.py:238-295), whose only parameter is the
`[256, 512, 3, 3]` weight `W = [W_x | W_h]` of `rnn_conv` (`twa_backward`).  It has no BatchNorm and no bias, so ITS gradient is
the same in the reference's training mode and in this package's eval mode.

    z_t = conv3x3(W, cat[x_t, h_{t-1}]),   i_t = sigmoid(z_t),   h_t = i_t x_t + (1 - i_t) h_{t-1}

`UAVSAL_LSTM` (the reference's ConvLSTM ablation, model_convlstm.py:111-126: `cc_t = conv3x3(W, cat[x_t, h_{t-1}])`,
`i, f, o = sigmoid`, `g = tanh`, `c_t = f c_{t-1} + i g`, `h_t = o tanh(c_t)`; `W` `[1024,512,3,3]`): `lstm_backward` stands
where `twa_backward` stands (`uavsal_lstm_scan` recomputes the cell-state history in one launch, `uavsal_lstm_gate_bwd` is one
step of the walk; the weight gradient is `uavsal_conv3_wgrad` at 1024 x 512), and every other stage works unchanged behind
it -- they hang off the recurrence's `grad_x` and `grad_h`, which are the same tensors in both models."""
import ctypes as C
import types

import torch

from .. import _lib as L
from ..ops import _nhwc_view, _stream
from ..weights import WeightCache
from ._common import HID, _conv, _dense, _nhwc, conv3_wgrad


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


# ---------------------------------------------------------------------------------------------- the forward from a given input
def _state(s, name, hh, ww, dev):
    """A carried state `[1,256,h,w]` as a dense NHWC tensor; None: zeros."""
    if s is None:
        return torch.zeros((1, hh, ww, HID), dtype=torch.float32, device=dev)
    s = _nhwc(s, name, HID).contiguous()
    if tuple(s.shape) != (1, hh, ww, HID) or s.device != dev:
        raise RuntimeError("%s must be [1,256,%d,%d] on the device of x_seq" % (name, hh, ww))
    return s


def _forward_args(x_seq, weight, rows, what):
    x = _nhwc(x_seq, "x_seq", HID)
    if (not torch.is_tensor(weight) or tuple(weight.shape) != (rows, 2 * HID, 3, 3) or weight.dtype != torch.float32
            or weight.device != x.device):
        raise RuntimeError("weight must be the float32 [%d,512,3,3] %s weight on the device" % (rows, what))
    return x


def twa_forward(x_seq, h0, weight, cache=None, module=None):
    """The ConvTWA recurrence forward from a GIVEN input sequence, outside the launch plan: `x_seq` `[T,256,h,w]`, `h0`
    `[1,256,h,w]` (None = zeros), `weight` `[256,512,3,3]` -> `h_seq` `[T,256,h,w]` (channels-last),
    `h_t = i_t x_t + (1 - i_t) h_{t-1}`, `i_t = sigmoid(conv3x3(W, cat[x_t, h_{t-1}]))`.  What a stage in FRONT of the
    recurrence needs once its output is no longer the plan's (`recurrence_step(block_stats=...)`).  No new kernel: one batched
    3x3 `uavsal_conv_gemm` of all frames with the W_x half (the hoisted `aux`), then per step one `uavsal_conv_gemm` of
    `h_{t-1}` with the W_h half whose epilogue is the step (`UAVSAL_EPI_TWA`), written straight into `h_seq[t]`.  Both go the
    DIRECT implicit-GEMM route, the tile `uavsal_conv_route` gives each launch -- never a Winograd route, whatever the launch
    plan takes for its steps -- so the result is within rounding of the plan's `rnn` tap and need not be its bits.  `cache` + `module`: take
    the packed forms from a `WeightCache` under the id of `module` (the conv that owns `weight`), the entries the plan's
    direct route uses; default: packed on the host for this call.  No synchronisation; two calls return the same bits."""
    lib = L.load()
    x = _forward_args(x_seq, weight, HID, "ConvTWA")
    T, hh, ww, _ = x.shape
    dev = x.device
    with torch.cuda.device(dev):
        hprev = _state(h0, "h0", hh, ww, dev)
        if cache is None or module is None:
            cache, module = WeightCache(dev, {}), types.SimpleNamespace(weight=weight)
        aux = _conv(lib, cache, x, module, HID, 9, wslice=(0, HID))      # W_x * x_t of all frames: the steps' `aux`
        h_seq = torch.empty((T, hh, ww, HID), dtype=torch.float32, device=dev)
        for t in range(T):
            _conv(lib, cache, hprev, module, HID, 9, wslice=(HID, 2 * HID), epi=L.EPI_TWA, res=x[t:t + 1], aux=aux[t:t + 1],
                  out=h_seq[t:t + 1])
            hprev = h_seq[t:t + 1]
    return h_seq.permute(0, 3, 1, 2)


def lstm_forward(x_seq, h0, c0, weight, cache=None, module=None):
    """`twa_forward` for the ConvLSTM of `UAVSAL_LSTM` (model_convlstm.py:111-126, no bias): `h0`, `c0` `[1,256,h,w]` (None =
    zeros), `weight` `[1024,512,3,3]` (rows gate * 256 + c, gates i, f, o, g) -> `(h_seq [T,256,h,w], c_last [1,256,h,w])`,
    `c_t = f c_{t-1} + i g`, `h_t = o tanh(c_t)`.  The hoisted W_x conv writes the gate-interleaved pre-activations (column
    4 c + gate, `WeightCache.conv(gate_interleave=256)`), and each step is one `uavsal_conv_gemm` 256 -> 1024 of `h_{t-1}` with
    the `UAVSAL_EPI_LSTM` epilogue, which writes `h_t` into `h_seq[t]` and `c_t` into one of two cell-state maps that take turns.  The direct route, as the plan's
    own ConvLSTM steps."""
    lib = L.load()
    x = _forward_args(x_seq, weight, 4 * HID, "ConvLSTM")
    T, hh, ww, _ = x.shape
    dev = x.device
    with torch.cuda.device(dev):
        hprev, cprev = _state(h0, "h0", hh, ww, dev), _state(c0, "c0", hh, ww, dev)
        if cache is None or module is None:
            cache, module = WeightCache(dev, {}), types.SimpleNamespace(weight=weight)
        aux = _conv(lib, cache, x, module, 4 * HID, 9, wslice=(0, HID), gate_interleave=HID)
        h_seq = torch.empty((T, hh, ww, HID), dtype=torch.float32, device=dev)
        cs = (torch.empty_like(cprev), torch.empty_like(cprev))      # c_t and c_{t-1} take turns in two maps, whatever T (c0 is only read)
        for t in range(T):
            _conv(lib, cache, hprev, module, 4 * HID, 9, wslice=(HID, 2 * HID), epi=L.EPI_LSTM, res=cprev, aux=aux[t:t + 1],
                  out=h_seq[t:t + 1], out2=cs[t % 2], gate_interleave=HID)
            hprev, cprev = h_seq[t:t + 1], cs[t % 2]
    return h_seq.permute(0, 3, 1, 2), cprev.permute(0, 3, 1, 2)
