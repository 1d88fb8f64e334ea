"""Heat-map overlay frames on the GPU: `vis.overlay_frames` (csrc/overlay.hip) against the numpy float64 restatement and
the known answers of tests/overlay_ref.py, `vis.visual_video` against one call over the whole video, and
`stream.predict_video(overlay=...)` against both.

Comparison rule for output bytes: the device works in double wherever the reference does, so it can differ from numpy
only through `pow` and contraction -- a few ulps of double times 255, about 1e-12.  A byte must equal rint(v) of the
restatement's pre-rounding v unless v lies within 1e-9 of a half-integer, where either neighbour is accepted
(tests/test_overlay_cpu.py bounds the share of such bytes by 1e-5 for every input compared that way, `overlay_ref.COMPARED`).
The known answers of `overlay_ref.cases()` are compared with exact equality."""
import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import synth, vis

import overlay_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _check(got, want, v, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.uint8, what
    wrong, excused = R.compare(got, want, v)
    print("%s: %d bytes, %d differ from rint(v), %d excused, %d wrong" % (
        what, want.size, int(np.count_nonzero(got != want)), excused, wrong))
    if wrong:
        bad = np.argwhere((got != want) & ~R.excused(v))
        raise AssertionError("%s: %d of %d bytes wrong, first at %r: got %d, want %d (v = %r)" % (
            what, wrong, want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])], v[tuple(bad[0])]))


def _device_input(g):
    fr = g["frames"] if g["layout"] == "HWC" else np.ascontiguousarray(g["frames"].transpose(0, 3, 1, 2))
    fix = None if g["fix"] is None else torch.from_numpy(g["fix"]).to(DEV)
    return torch.from_numpy(fr).to(DEV), torch.from_numpy(g["sal"]).to(DEV), fix


@pytest.mark.parametrize("name", [g[0] for g in R.GPU_INPUTS])
def test_kernel_equals_the_restatement(name):
    g = R.gpu_input(name)
    want, v = R.gpu_want(name)
    fr, sal, fix = _device_input(g)
    for F in (1, len(fr)):
        kw = dict(mid_size=g["mid"], out_size=g["out"], layout=g["layout"], colormap=g["lut"])
        got = vis.overlay_frames(fr[:F], sal[:F], None if fix is None else fix[:F], **kw)
        _check(got, want[:F], v[:F], "%s F=%d" % (name, F))
        again = vis.overlay_frames(fr[:F], sal[:F], None if fix is None else fix[:F], **kw)
        assert torch.equal(got, again), "two runs differ"
    if fix is not None:                                                 # the same input without its fixations, and as bool
        w2, v2 = R.gpu_want(name + "_nofix")
        _check(vis.overlay_frames(fr[:1], sal[:1], None, **kw), w2, v2, name + " without fixations")
        assert torch.equal(vis.overlay_frames(fr, sal, fix != 0, **kw), got)


def test_default_table_and_default_sizes():
    """No colormap: the shipped JET; no sizes: visual_img's path."""
    g = R.gpu_input("img_path")
    fr, sal, fix = _device_input(g)
    want, v = R.gpu_want("img_path_jet")
    _check(vis.overlay_frames(fr, sal, fix), want, v, "defaults")
    cv2_shaped = torch.from_numpy(R.jet_table()).reshape(256, 1, 3)            # what cv2.applyColorMap returns for arange(256)
    assert torch.equal(vis.overlay_frames(fr, sal, fix, colormap=cv2_shaped), vis.overlay_frames(fr, sal, fix))


CASES = list(R.cases())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kernel_gives_the_known_answers(case):
    name, kw, want = case
    hwc = torch.from_numpy(kw["frames"]).to(DEV)
    sal = torch.from_numpy(kw["sal"]).to(DEV)
    fix = torch.from_numpy(kw["fix"]).to(DEV) if kw.get("fix") is not None else None
    args = dict(mid_size=kw.get("mid_size"), out_size=kw.get("out_size"), colormap=kw["lut"])
    for what, got in (("HWC", vis.overlay_frames(hwc, sal, fix, **args)),
                      ("CHW", vis.overlay_frames(hwc.permute(0, 3, 1, 2).contiguous(), sal, fix, layout="CHW", **args))):
        got = got.cpu().numpy()                             # exact equality: no byte of a known answer is excused
        assert got.shape == want.shape and got.dtype == np.uint8, name
        assert np.array_equal(got, want), "%s %s: %d of %d bytes differ" % (name, what, np.count_nonzero(got != want), want.size)


@pytest.mark.parametrize("layout", ["HWC", "CHW"])
def test_slices_of_a_larger_buffer_at_odd_offsets(layout):
    """`buf[1:]` of a byte buffer (odd address), rows and planes further apart than their content, a leading-dimension slice
    and a width slice, maps and fixations at odd addresses: read in place."""
    F, h0, w0 = 3, 90, 161
    g = R.gpu_input("odd_sizes")
    src, lut = g["frames"][:F], g["lut"]
    salnp, fixnp = g["sal"][:F], g["fix"][:F]
    t = torch.from_numpy(src if layout == "HWC" else np.ascontiguousarray(src.transpose(0, 3, 1, 2))).to(DEV)
    if layout == "HWC":
        row = 3 * w0 + 5
        shape, strides = (F, h0, w0, 3), (row * h0 + 7, row, 3, 1)
    else:
        row = w0 + 3
        plane = row * h0 + 11
        shape, strides = (F, 3, h0, w0), (3 * plane + 1, plane, row, 1)
    buf = torch.full((strides[0] * F + 64,), 255, dtype=torch.uint8, device=DEV)
    view = buf[1:].as_strided(shape, strides)
    assert view.data_ptr() % 2 == 1
    view.copy_(t)
    sal = torch.zeros((salnp.size + 3,), dtype=torch.uint8, device=DEV)[3:].view(salnp.shape)
    sal.copy_(torch.from_numpy(salnp))
    fix = torch.zeros((fixnp.size + 5,), dtype=torch.uint8, device=DEV)[5:].view(fixnp.shape)
    fix.copy_(torch.from_numpy(fixnp))
    assert sal.data_ptr() % 2 == 1 and fix.data_ptr() % 2 == 1
    kw = dict(mid_size=(45, 80), out_size=(97, 173), layout=layout, colormap=lut)
    want, v = (a[:F] for a in R.gpu_want("odd_sizes"))
    assert tuple(g["mid"]) == (45, 80) and tuple(g["out"]) == (97, 173)
    _check(vis.overlay_frames(view, sal, fix, **kw), want, v, "strided " + layout)
    _check(vis.overlay_frames(view[1:], sal[1:], fix[1:], **kw), want[1:], v[1:], "view[1:]")
    narrow = view[:, :, :100, :] if layout == "HWC" else view[:, :, :, :100]
    w2, v2 = R.gpu_want("odd_sizes_narrow")
    _check(vis.overlay_frames(narrow, sal, fix, **kw), w2, v2, "width slice")
    with pytest.raises(RuntimeError, match="not a"):
        vis.overlay_frames(t[:, :, ::2, :] if layout == "HWC" else t[:, :, :, ::2], sal, **kw)      # not pixel-dense
    with pytest.raises(RuntimeError, match="3 channels"):
        vis.overlay_frames(t, sal, mid_size=(45, 80), out_size=(97, 173), layout="CHW" if layout == "HWC" else "HWC")
    with pytest.raises(RuntimeError, match="layout"):
        vis.overlay_frames(t, sal, layout="NHWC")
    with pytest.raises(RuntimeError, match="uint8 cuda frames"):
        vis.overlay_frames(t.float(), sal, **kw)
    with pytest.raises(RuntimeError, match="uint8 cuda frames"):
        vis.overlay_frames(t.cpu(), sal, **kw)
    with pytest.raises(RuntimeError, match="uint8 maps"):
        vis.overlay_frames(view, sal.float(), **kw)
    with pytest.raises(RuntimeError, match="uint8 maps"):
        vis.overlay_frames(view, sal.cpu(), **kw)
    with pytest.raises(RuntimeError, match="fixation maps"):
        vis.overlay_frames(view, sal, fix.float(), **kw)
    with pytest.raises(RuntimeError, match="colormap"):
        vis.overlay_frames(view, sal, fix, mid_size=(45, 80), out_size=(97, 173), layout=layout, colormap=np.zeros((255, 3), np.uint8))


def test_visual_video_with_a_sink_equals_one_call_over_the_video():
    g = R.gpu_input("405x719")
    fr, sal, fix = _device_input(g)
    fr, sal, fix = fr.repeat(3, 1, 1, 1)[:13], sal.repeat(3, 1, 1)[:13], fix.repeat(3, 1, 1)[:13]
    mid_h, mid_w, out_h, out_w = vis.visual_geometry(405, 719)
    whole = vis.overlay_frames(fr, sal, fix, (mid_h, mid_w), (out_h, out_w))
    want, v = R.gpu_want("405x719")                                                      # (its table is the default one)
    _check(whole[:5], want, v, "whole video, first frames")
    assert torch.equal(vis.visual_video(fr, sal, fix, with_fix=1, group=4), whole)
    assert not torch.equal(vis.visual_video(fr, sal, fix, with_fix=0, group=4), whole)   # fixations only when asked
    assert torch.equal(vis.visual_video(fr, sal[:11], fix, with_fix=1), whole[:11])      # min over the lengths
    for host in (False, True):
        seen = []
        assert vis.visual_video(fr, sal, fix, with_fix=1, group=4, host=host,
                                sink=lambda i0, x: seen.append((i0, x.is_cuda, x.cpu().clone()))) is None
        assert [s[0] for s in seen] == [0, 4, 8, 12] and all(s[1] != host for s in seen)
        assert torch.equal(torch.cat([s[2] for s in seen]), whole.cpu())
    back = vis.visual_video(fr.cpu().pin_memory(), sal, fix, with_fix=1, group=5, host=True)      # host frames, host result
    assert not back.is_cuda and back.is_pinned() and torch.equal(back, whole.cpu())


def _video(h0, w0, n):
    base = synth.synth_frames_u8(11, h0, w0, 5)
    return np.concatenate([np.roll(base, 13 * k, axis=3) for k in range((n + 10) // 11)])[:n]


@pytest.mark.parametrize("overlap", [False, True])
def test_predict_video_with_overlay(overlap):
    """The maps are those of the same call without `overlay`, bit for bit; the frames are `visual_video` on those maps."""
    from iip_uavsal_saliency_amd import UAVSal
    from iip_uavsal_saliency_amd.stream import predict_video
    h0, w0, rows, cols = 720, 1280, 360, 640
    m = UAVSal(time_dims=4)
    synth.load_synth_weights(m, 0)
    m = m.to(DEV).eval()
    gen = torch.Generator().manual_seed(3)
    gp, op_ = torch.rand((8, rows // 8, cols // 8), generator=gen), torch.rand((20, rows // 8, cols // 8), generator=gen)
    src = _video(h0, w0, 44)                                                               # [44, 3, h0, w0] RGB
    bgr_hwc = torch.from_numpy(np.ascontiguousarray(src[:, ::-1].transpose(0, 2, 3, 1)))   # what cv2.VideoCapture yields
    kw = dict(batch_size=2, overlap=overlap, model_size=(rows, cols), frame_layout="HWC", bgr=True)
    plain = predict_video(m, bgr_hwc.to(DEV), gp, op_, **kw)
    want = vis.visual_video(bgr_hwc.to(DEV), plain)
    assert want.shape == (44, 720, 1280, 3)
    for name, frames in (("device", bgr_hwc.to(DEV)), ("pinned", bgr_hwc.pin_memory())):
        sal, over = predict_video(m, frames, gp, op_, overlay=True, **kw)
        assert torch.equal(sal, plain), name
        assert over.is_cuda and torch.equal(over, want), name
    # fixations, another table and a sink through the dict; raw maps still come second
    fix = torch.zeros((44, h0, w0), dtype=torch.uint8, device=DEV)
    fix[:, 100:700:37, 50:1250:91] = 1
    lut = R.random_table()
    seen = []
    sal, maps, over = predict_video(m, bgr_hwc.to(DEV), gp, op_, return_maps=True,
                                    overlay=dict(fix=fix, colormap=lut, sink=lambda i0, x: seen.append(x.clone())), **kw)
    assert over is None and torch.equal(sal, plain) and maps.shape[0] == 44
    assert torch.equal(torch.cat(seen), vis.visual_video(bgr_hwc.to(DEV), plain, fix, with_fix=1, colormap=lut))
    # RGB planar frames: the overlay keeps the frames' channel order, the table is flipped
    chw = torch.from_numpy(src).to(DEV)
    sal, over = predict_video(m, chw, gp, op_, batch_size=2, overlap=overlap, model_size=(rows, cols), overlay=True)
    assert torch.equal(sal, plain) and torch.equal(over, want.flip(3))
    with pytest.raises(RuntimeError, match="model_size"):
        predict_video(m, torch.zeros((8, 3, rows, cols), dtype=torch.uint8, device=DEV), gp, op_, batch_size=2, overlay=True)
