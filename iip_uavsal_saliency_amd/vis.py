"""Heat-map overlay frames on the device: the third call of the reference's driver, `visual_vid(..., with_color=1)`
(reference utils_vis.py:103-212, Demo_Test.py:130), and `heatmap_overlay` / `visual_img` (:34-101) as its special case
without resizes.  The arithmetic is csrc/overlay.hip (`uavsal_overlay_u8`); this module holds the host side: the geometry
of visual_vid, the default colour table, the op and the per-video loop in groups.  Encoding and writing the video stays
with the caller: the product is the uint8 BGR frames the reference hands to `VideoWriter.write`.

The default colour table is OpenCV's JET restated from its published construction -- the 64 knots of jet(64) interpolated
linearly at 256 evenly spaced points, times 255, rounded half to even -- and shipped as a constant.  cv2 is not installed
where this was written: the table is NOT checked against cv2.  A caller with cv2 passes
`colormap=cv2.applyColorMap(np.arange(256, dtype=np.uint8), cv2.COLORMAP_JET)` to use cv2's own."""
from __future__ import annotations

import ctypes as C
from typing import Callable, Optional

import numpy as np
import torch

from . import _lib as L
from .ops import _stream

JET_BGR = np.frombuffer(bytes.fromhex(
    "8f00009300009700009b00009f0000a30000a70000ab0000af0000b30000b70000bb0000bf0000c30000c70000cb0000ce0000d20000d60000da0000"
    "de0000e20000e60000ea0000ee0000f20000f60000fa0000fe0000ff0300ff0700ff0b00ff0e00ff1200ff1600ff1a00ff1e00ff2200ff2600ff2a00"
    "ff2e00ff3200ff3600ff3a00ff3e00ff4200ff4600ff4a00ff4d00ff5100ff5500ff5900ff5d00ff6100ff6500ff6900ff6d00ff7100ff7500ff7900"
    "ff7d00ff8100ff8500ff8900ff8c00ff9000ff9400ff9800ff9c00ffa000ffa400ffa800ffac00ffb000ffb400ffb800ffbc00ffc000ffc400ffc800"
    "ffcb00ffcf00ffd300ffd700ffdb00ffdf00ffe300ffe700ffeb00ffef00fff300fff700fffb00ffff00fbff04f7ff08f4ff0bf0ff0fecff13e8ff17"
    "e4ff1be0ff1fdcff23d8ff27d4ff2bd0ff2fccff33c8ff37c4ff3bc0ff3fbcff43b8ff47b5ff4ab1ff4eadff52a9ff56a5ff5aa1ff5e9dff6299ff66"
    "95ff6a91ff6e8dff7289ff7685ff7a81ff7e7dff8279ff8676ff8972ff8d6eff916aff9566ff9962ff9d5effa15affa556ffa952ffad4effb14affb5"
    "46ffb942ffbd3effc13affc437ffc833ffcc2fffd02bffd427ffd823ffdc1fffe01bffe417ffe813ffec0ffff00bfff407fff803fffc00feff00faff"
    "00f7ff00f3ff00efff00ebff00e7ff00e3ff00dfff00dbff00d7ff00d3ff00cfff00cbff00c7ff00c3ff00bfff00bcff00b8ff00b4ff00b0ff00acff"
    "00a8ff00a4ff00a0ff009cff0098ff0094ff0090ff008cff0088ff0084ff0080ff007cff0079ff0075ff0071ff006dff0069ff0065ff0061ff005dff"
    "0059ff0055ff0051ff004dff0049ff0045ff0041ff003eff003aff0036ff0032ff002eff002aff0026ff0022ff001eff001aff0016ff0012ff000eff"
    "000aff0006ff0002ff0000fe0000fa0000f60000f20000ee0000ea0000e60000e20000de0000da0000d60000d20000ce0000ca0000c60000c20000be"
    "0000bb0000b70000b30000af0000ab0000a70000a300009f00009b00009700009300008f00008b000087000083000080"), dtype=np.uint8).reshape(256, 3)
JET_BGR.flags.writeable = False
_LUT_CACHE = {}


def visual_geometry(vid_h: int, vid_w: int):
    """`(mid_h, mid_w, out_h, out_w)` of visual_vid for a `vid_h x vid_w` video, integers and Python floats exactly as the
    reference writes them: the frame is first reduced by `ratio = max(1, max(vid_w // 640, vid_h // 360))`
    (utils_vis.py:185-186), the overlay is then resized to `int(vid_w * min(1280 / vid_w, 720 / vid_h))` columns and
    `int(vid_h * min(720 / vid_h, 720 / vid_h))` rows (:168-170 -- the reference names `max_h` twice in the second line, so
    the height is `int(vid_h * (720 / vid_h))`, whatever `int()` makes of a product just below an integer)."""
    vid_h, vid_w = int(vid_h), int(vid_w)
    if vid_h <= 0 or vid_w <= 0:
        raise RuntimeError("visual_geometry: sizes must be positive, got %r" % ((vid_h, vid_w),))
    ratio = max(1, max(vid_w // 640, vid_h // 360))
    max_w, max_h = 1280, 720
    out_w = int(vid_w * min(max_w / vid_w, max_h / vid_h))
    out_h = int(vid_h * min(max_h / vid_h, max_h / vid_h))
    mid_h, mid_w = vid_h // ratio, vid_w // ratio
    if min(mid_h, mid_w, out_h, out_w) <= 0:
        raise RuntimeError("visual_geometry: a %dx%d video has no picture (%r)" % (vid_h, vid_w, (mid_h, mid_w, out_h, out_w)))
    return mid_h, mid_w, out_h, out_w


def _lut(colormap, dev):
    """The `[256, 3]` uint8 BGR table on `dev`; the default (JET_BGR) is uploaded once per device."""
    if colormap is None:
        key = str(dev)
        if key not in _LUT_CACHE:
            _LUT_CACHE[key] = torch.from_numpy(JET_BGR.copy()).to(dev)
        return _LUT_CACHE[key]
    if torch.is_tensor(colormap) and colormap.device == torch.device(dev) and colormap.dtype == torch.uint8 \
            and tuple(colormap.shape) == (256, 3) and colormap.is_contiguous():
        return colormap                                   # already resolved (visual_video does it once per video)
    t = torch.as_tensor(np.ascontiguousarray(colormap) if isinstance(colormap, np.ndarray) else colormap)
    if t.dtype != torch.uint8 or t.numel() != 768 or t.shape[0] != 256:
        raise RuntimeError("colormap must be a uint8 table of shape [256, 3] (or cv2's [256, 1, 3]), got %s %r" % (t.dtype, tuple(t.shape)))
    return t.reshape(256, 3).contiguous().to(dev)


def overlay_frames(frames_u8, sal_u8, fix=None, mid_size=None, out_size=None, layout="HWC", colormap=None):
    """Device version of `heatmap_overlay` and of one group of visual_vid's coloured loop (utils_vis.py:34-56, 176-209):
    uint8 BGR frames `[F, H0, W0, 3]` (`layout="HWC"`) or `[F, 3, H0, W0]` (`"CHW"`) and uint8 maps `[F, h, w]` on the
    device -> uint8 `[F, out_h, out_w, 3]` on the device, the frames `VideoWriter.write` receives.  `mid_size`: the frame
    is first resized to it (8-bit rule, :186); `out_size`: the double overlay is resized to it (:190); either left as None
    means no resize there, which is `visual_img`'s path.  `fix`: uint8 or bool `[F, Hf, Wf]`, nonzero = a fixation; its
    positions are scaled to the output size, dilated 5x5 and drawn as 1 (:199-206).  `colormap`: a `[256, 3]` uint8 BGR
    table (default: the restated JET, see the module docstring).  Frames are read in place through their strides as
    `ops.letterbox_frames` reads them.  Five launches on the current stream, no synchronisation."""
    lib = L.load()
    if not torch.is_tensor(frames_u8) or not frames_u8.is_cuda or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4:
        raise RuntimeError("expected uint8 cuda frames [F,H0,W0,3] (layout='HWC') or [F,3,H0,W0] (layout='CHW')")
    if layout not in ("HWC", "CHW"):
        raise RuntimeError("layout must be 'HWC' or 'CHW', got %r" % (layout,))
    dev = frames_u8.device
    F = frames_u8.shape[0]
    st = frames_u8.stride()
    if layout == "HWC":
        _, h0, w0, c = frames_u8.shape
        dense = (st[3] == 1 or c == 1) and (st[2] == 3 or w0 == 1)
        row, plane, img = (st[1] if h0 > 1 else 3 * w0), 0, st[0]
    else:
        _, c, h0, w0 = frames_u8.shape
        dense = st[3] == 1 or w0 == 1
        row, plane, img = (st[2] if h0 > 1 else w0), st[1], st[0]
    if c != 3:
        raise RuntimeError("expected 3 channels in dimension %d of %s frames, got shape %r" % (
            3 if layout == "HWC" else 1, layout, tuple(frames_u8.shape)))
    if not torch.is_tensor(sal_u8) or sal_u8.device != dev or sal_u8.dtype != torch.uint8 or sal_u8.dim() != 3 or sal_u8.shape[0] != F:
        raise RuntimeError("expected uint8 maps [F,h,w] on the frames' device, one per frame")
    if min(h0, w0, sal_u8.shape[1], sal_u8.shape[2]) <= 0:
        raise RuntimeError("empty frames or maps")
    if not dense or row < (3 * w0 if layout == "HWC" else w0):
        raise RuntimeError("frames are not a %s buffer (or a slice of one): strides %r" % (layout, tuple(st)))
    mid_h, mid_w = (h0, w0) if mid_size is None else (int(mid_size[0]), int(mid_size[1]))
    out_h, out_w = (mid_h, mid_w) if out_size is None else (int(out_size[0]), int(out_size[1]))
    if min(mid_h, mid_w, out_h, out_w) <= 0:
        raise RuntimeError("mid_size and out_size must be positive")
    if fix is not None:
        if not torch.is_tensor(fix) or fix.device != dev or fix.dtype not in (torch.uint8, torch.bool) or fix.dim() != 3 \
                or fix.shape[0] != F or min(fix.shape[1:]) <= 0:
            raise RuntimeError("expected uint8 or bool fixation maps [F,Hf,Wf] on the frames' device, one per frame")
        fix = fix.contiguous()
        fix = fix.view(torch.uint8) if fix.dtype == torch.bool else fix
    lut = _lut(colormap, dev)
    out = torch.empty((F, out_h, out_w, 3), dtype=torch.uint8, device=dev)
    if F == 0:
        return out
    sal_u8 = sal_u8 if sal_u8[0].is_contiguous() and (F == 1 or sal_u8.stride(0) >= sal_u8[0].numel()) else sal_u8.contiguous()
    d = L.OverlayDesc()
    d.frames, d.row_pitch, d.plane_pitch, d.img_pitch = frames_u8.data_ptr(), row, plane, (img if F > 1 else 0)
    d.map, d.map_img_pitch = sal_u8.data_ptr(), (sal_u8.stride(0) if F > 1 else 0)
    d.fix, d.lut, d.out = (fix.data_ptr() if fix is not None else None), lut.data_ptr(), out.data_ptr()
    d.n_img, d.layout, d.h0, d.w0 = F, (L.LETTERBOX_HWC if layout == "HWC" else L.LETTERBOX_CHW), h0, w0
    d.map_h, d.map_w = sal_u8.shape[1], sal_u8.shape[2]
    d.fix_h, d.fix_w = (fix.shape[1], fix.shape[2]) if fix is not None else (0, 0)
    d.mid_h, d.mid_w, d.out_h, d.out_w = mid_h, mid_w, out_h, out_w
    need = lib.uavsal_overlay_workspace_bytes(C.byref(d))
    if need < 0:
        L.check(int(need), "uavsal_overlay_workspace_bytes")
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)          # the allocator hands out 512-byte aligned blocks
    d.ws, d.ws_bytes = ws.data_ptr(), need
    L.check(lib.uavsal_overlay_u8(C.byref(d), _stream(frames_u8)), "uavsal_overlay_u8")
    return out


@torch.no_grad()
def visual_video(frames, salmap, fix=None, with_fix=0, group: int = 20, sink: Optional[Callable] = None, layout="HWC",
                 colormap=None, host: bool = False):
    """The reference's per-video loop (utils_vis.py:150-212, with_color=1) in groups of `group` frames: uint8 BGR source
    frames `[F, H0, W0, 3]` (or `[F, 3, H0, W0]` with `layout="CHW"`; on the device, or in host memory -- each group is
    then uploaded here, on the current stream) and the video's uint8 maps `[F', h, w]` on the device -> the uint8 BGR frames `[n, out_h, out_w, 3]` of
    `visual_geometry(H0, W0)`, `n = min(F, F')` (and of the fixation frames when they are drawn, :158-162).
    `with_fix` and `fix` (`[F'', Hf, Wf]` uint8 / bool, the video's `fixLoc`): draw the fixations (:199-206).
    `sink(i0, frames_u8)` receives each finished group, `i0` its first frame; nothing is returned then.  The group is a
    device tensor, ordered on the current stream, unless `host=True`: each group is then copied into one of two pinned host
    buffers on a copy stream and `sink` is called once that copy has landed, while the next group already renders -- the
    buffer is reused two groups later, so `sink` encodes (or copies) before it returns.  Without a sink the whole video is
    returned, on the device or (`host=True`) in pinned host memory."""
    if not torch.is_tensor(frames) or frames.dim() != 4 or frames.dtype != torch.uint8:
        raise RuntimeError("expected uint8 frames [F,H0,W0,3] (layout='HWC') or [F,3,H0,W0] (layout='CHW')")
    if layout not in ("HWC", "CHW"):
        raise RuntimeError("layout must be 'HWC' or 'CHW', got %r" % (layout,))
    if not torch.is_tensor(salmap) or not salmap.is_cuda:
        raise RuntimeError("expected the video's uint8 maps [F,h,w] on the device")
    dev = salmap.device
    h0, w0 = frames.shape[1:3] if layout == "HWC" else frames.shape[2:4]
    mid_h, mid_w, out_h, out_w = visual_geometry(h0, w0)
    n = min(frames.shape[0], salmap.shape[0])                          # utils_vis.py:158
    draw = bool(with_fix) and fix is not None                          # :160, :199
    if draw:
        n = min(n, fix.shape[0])                                       # :162
        fix = fix.to(dev)
    group = max(1, int(group))
    colormap = _lut(colormap, dev)                        # one conversion and upload per video, not per group
    whole = None
    if sink is None:
        whole = torch.empty((n, out_h, out_w, 3), dtype=torch.uint8, device="cpu" if host else dev, pin_memory=host)
    cur = torch.cuda.current_stream(dev)
    if host:
        copy = torch.cuda.Stream(dev)
        bufs = [] if sink is None else [torch.empty((min(group, n), out_h, out_w, 3), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
    pending = None                                                     # (i0, host tensor, event) of the previous group
    for k, i0 in enumerate(range(0, n, group)):
        i1 = min(i0 + group, n)
        fr = frames[i0:i1]
        if not fr.is_cuda:
            fr = fr.to(dev, non_blocking=True)
        o = overlay_frames(fr, salmap[i0:i1], fix[i0:i1] if draw else None, (mid_h, mid_w), (out_h, out_w), layout, colormap)
        if host:
            dst = whole[i0:i1] if sink is None else bufs[k % 2][:i1 - i0]
            copy.wait_stream(cur)
            with torch.cuda.stream(copy):
                dst.copy_(o, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(copy)
            o.record_stream(copy)
            if pending is not None and sink is not None:
                pending[2].synchronize()
                sink(pending[0], pending[1])
            pending = (i0, dst, ev)
        elif sink is not None:
            sink(i0, o)
        else:
            whole[i0:i1] = o
    if host and pending is not None:
        pending[2].synchronize()
        if sink is not None:
            sink(pending[0], pending[1])
        else:
            copy.synchronize()
    return whole
