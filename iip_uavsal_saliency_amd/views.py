"""What the recorders and the checks address: `V` while a plan is recorded, `OpView` in the record of a finished plan."""
import torch

from .arena import _ArenaRef


def _down(n: int) -> int:
    return (n - 1) // 2 + 1      # 3x3, stride 2, pad 1


class _Fake:
    """Stand-in tensor for the sizing pass."""
    def data_ptr(self):
        return 0

    def numel(self):
        return 0


class Caller:
    """Stands in `V.t` for a tensor of the caller's side (Recorder.caller): `name` is its key in the recorder's table, `t` the
    table's tensor (None in the sizing pass).  `named`: `Engine.run` binds the call's own tensor in its place, so the record
    of an op (OpView.buf) carries the name, not the tensor."""
    __slots__ = ("name", "t", "named")

    def __init__(self, name, t, named=True):
        self.name, self.t, self.named = name, t, named

    def data_ptr(self):
        return 0 if self.t is None else self.t.data_ptr()


class V:
    """A channel slice [coff, coff+C) of an NHWC buffer `[n*h*w, ld]`.  `sp`: the buffer's split shadow (fp16,
    `[pixel][ld/32][hi 32 | lo 32]`, include/uavsal_hip.h) when some GEMM stages this tensor pre-split; `t` is
    None for a tensor that only exists as its shadow (depthwise outputs)."""
    __slots__ = ("t", "ld", "coff", "n", "h", "w", "c", "sp", "key")

    def __init__(self, t, n, h, w, c, ld=None, coff=0, sp=None, key=None):
        self.t, self.n, self.h, self.w, self.c = t, n, h, w, c
        self.ld = ld if ld is not None else c
        self.coff = coff
        self.sp, self.key = sp, key

    @property
    def ptr(self):
        return None if self.t is None else self.t.data_ptr() + 4 * self.coff

    @property
    def sp_ptr(self):
        """Address of this view inside the shadow: `coff` = pixel offset * ld + channel offset (a multiple of 32)."""
        pix, ch = divmod(self.coff, self.ld)
        assert ch % 32 == 0 and self.ld % 32 == 0
        return self.sp.data_ptr() + 2 * (pix * 2 * self.ld + (ch // 32) * 64)

    def slice(self, coff, c):
        return V(self.t, self.n, self.h, self.w, c, self.ld, self.coff + coff, self.sp, self.key)

    def frames(self, first, count):
        """Images [first, first+count) as a view (pointer offset only)."""
        return V(self.t, count, self.h, self.w, self.c, self.ld, self.coff + first * self.h * self.w * self.ld,
                 self.sp, self.key)


class OpView:
    """What one operand of a recorded op addresses: images [0, n) of `h x w` pixels, channels [0, c) of rows `ld` floats apart,
    starting `off` floats into `buf`; image i starts `img` pixels after image i - 1.  `buf` is the tensor, the arena buffer
    (_ArenaRef), or the name of a caller tensor that `run` binds into the plan ("x", "out", "state_in", ...; Engine.bound).
    `sp` / `sp_off`: the split shadow (fp16, `[pixel][ld/32][hi 32 | lo 32]`) and the view's first half in it, or None.
    `nchw`: the operand is a caller-side NCHW tensor ([n, c, h*w] at `off`; `ld` and `img` unused)."""
    __slots__ = ("buf", "off", "n", "h", "w", "c", "ld", "img", "sp", "sp_off", "nchw")

    def __init__(self, buf, off, n, h, w, c, ld, img, sp=None, sp_off=0, nchw=False):
        self.buf, self.off, self.n, self.h, self.w, self.c, self.ld, self.img = buf, off, n, h, w, c, ld, img
        self.sp, self.sp_off, self.nchw = sp, sp_off, nchw

    @staticmethod
    def of(v: "V", img=None) -> "OpView":
        buf = v.t
        if isinstance(buf, Caller):
            buf = buf.name if buf.named else buf.t
        sp, sp_off = None, 0
        if v.sp is not None and not isinstance(v.sp, _Fake):
            pix, ch = divmod(v.coff, v.ld)
            sp, sp_off = v.sp, pix * 2 * v.ld + (ch // 32) * 64
        return OpView(buf, v.coff, v.n, v.h, v.w, v.c, v.ld, v.h * v.w if img is None else img, sp, sp_off)

    def __repr__(self):
        return "OpView(%s+%d, n=%d, %dx%d, c=%d, ld=%d, img=%d%s)" % (
            getattr(self.buf, "aid", self.buf if isinstance(self.buf, str) else "tensor"), self.off, self.n, self.h, self.w,
            self.c, self.ld, self.img, ", shadow" if self.sp is not None else "")


def read_view(eng, d: OpView, shadow=False, images=None, device=None) -> torch.Tensor:
    """Operand `d` of `eng`'s plan as float64 NCHW `[n, c, h, w]` (images `images` only, when given), read from the fp32
    buffer or -- `shadow` -- merged from its split shadow (ops.merge_shadow's arithmetic).  `eng` may be None for views whose
    `buf` is a tensor.  A copy: later launches do not change it."""
    if shadow:
        if d.sp is None:
            raise ValueError("%r has no split shadow" % (d,))
        sp = d.sp.reshape(-1)
        t = sp.as_strided((d.n, d.h, d.w, d.c // 32, 2, 32), (d.img * 2 * d.ld, d.w * 2 * d.ld, 2 * d.ld, 64, 32, 1),
                          sp.storage_offset() + d.sp_off)
        if images is not None:
            t = t[list(images)]
        t = t.double()
        t = ((t[..., 0, :] + t[..., 1, :]) / 16.0).reshape(t.shape[0], d.h, d.w, d.c)
    else:
        buf = d.buf
        if isinstance(buf, str):
            buf = eng.bound(buf)
        elif isinstance(buf, _ArenaRef):
            buf = buf.tensor()
        if buf is None:
            raise ValueError("%r has no fp32 buffer (shadow only)" % (d,))
        flat = buf.reshape(-1)
        if d.nchw:
            t = flat.as_strided((d.n, d.c, d.h, d.w), (d.c * d.h * d.w, d.h * d.w, d.w, 1), flat.storage_offset() + d.off)
            t = t if images is None else t[list(images)]
            return t.to(device=device, dtype=torch.float64)
        t = flat.as_strided((d.n, d.h, d.w, d.c), (d.img * d.ld, d.w * d.ld, d.ld, 1), flat.storage_offset() + d.off)
        if images is not None:
            t = t[list(images)]
        t = t.double() if t.dtype != torch.uint8 else t
    return t.permute(0, 3, 1, 2).to(device=device, dtype=torch.float64).contiguous()
