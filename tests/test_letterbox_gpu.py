"""Input letterboxing on the GPU: `ops.letterbox_frames` (csrc/letterbox.hip) against the numpy restatement and the known
answers of tests/letterbox_ref.py, and `stream.predict_video(model_size=...)` against the same driver fed with frames the
restatement letterboxed.  Integer arithmetic: every comparison is exact equality."""
import functools

import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import ops, synth

import letterbox_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=2)
def _source(kind, h0, w0):
    """Five source frames [5, h0, w0, 3] (interleaved)."""
    if kind == "synth":
        return np.ascontiguousarray(synth.synth_frames_u8(5, h0, w0, 3).transpose(0, 2, 3, 1))
    return np.random.RandomState(h0 * 7 + w0).randint(0, 256, (5, h0, w0, 3)).astype(np.uint8)


def _check(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.uint8, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d bytes differ, first at %r: got %d, want %d" % (
            what, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


@pytest.mark.parametrize("kind", ["synth", "random"])
@pytest.mark.parametrize("size", R.SOURCE_SIZES, ids=["%dx%d" % s for s in R.SOURCE_SIZES])
def test_kernel_equals_the_restatement(size, kind):
    h0, w0 = size
    src = _source(kind, h0, w0)
    hwc = torch.from_numpy(src).to(DEV)
    chw = hwc.permute(0, 3, 1, 2).contiguous()
    for rows, cols in R.MODEL_SIZES:
        want = R.letterbox(src, rows, cols)
        for layout, frames in (("HWC", hwc), ("CHW", chw)):
            for bgr in (False, True):
                for F in (1, 5):
                    got = ops.letterbox_frames(frames[:F], rows, cols, layout=layout, bgr=bgr)
                    w = want[:F, ::-1] if bgr else want[:F]
                    _check(got, np.ascontiguousarray(w), "%dx%d -> %dx%d %s bgr=%s F=%d" % (h0, w0, rows, cols, layout, bgr, F))


CASES = list(R.cases())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kernel_gives_the_known_answers(case):
    name, src, rows, cols, bgr, want = case
    hwc = torch.from_numpy(src).to(DEV)
    _check(ops.letterbox_frames(hwc, rows, cols, bgr=bgr), want, name + " HWC")
    _check(ops.letterbox_frames(hwc.permute(0, 3, 1, 2).contiguous(), rows, cols, layout="CHW", bgr=bgr), want, name + " CHW")


@pytest.mark.parametrize("layout", ["HWC", "CHW"])
def test_slices_of_a_larger_buffer_at_odd_offsets(layout):
    """`buf[1:]` of a byte buffer (odd address), rows and planes further apart than their content, a leading-dimension slice
    and a width slice: read in place through the pitches."""
    F, h0, w0 = 3, 90, 161
    src = np.random.RandomState(9).randint(0, 256, (F, h0, w0, 3)).astype(np.uint8)
    want = R.letterbox(src, 36, 64)
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
    _check(ops.letterbox_frames(view, 36, 64, layout=layout), want, "strided " + layout)
    _check(ops.letterbox_frames(view[1:], 36, 64, layout=layout, bgr=True), np.ascontiguousarray(want[1:, ::-1]), "view[1:]")
    # a picture that is the left part of wider rows
    narrow = view[:, :, :100, :] if layout == "HWC" else view[:, :, :, :100]
    _check(ops.letterbox_frames(narrow, 36, 64, layout=layout), R.letterbox(src[:, :, :100], 36, 64), "width slice")
    # a model size that is no multiple of four, into an odd-sized picture
    _check(ops.letterbox_frames(view, 37, 53, layout=layout), R.letterbox(src, 37, 53), "37x53")
    with pytest.raises(RuntimeError, match="not a"):
        ops.letterbox_frames(t[:, :, ::2, :] if layout == "HWC" else t[:, :, :, ::2], 36, 64, layout=layout)      # not pixel-dense
    with pytest.raises(RuntimeError, match="3 channels"):
        ops.letterbox_frames(t, 36, 64, layout="CHW" if layout == "HWC" else "HWC")
    with pytest.raises(RuntimeError, match="uint8 cuda frames"):
        ops.letterbox_frames(t.float(), 36, 64, layout=layout)


def test_one_2160p_group_and_two_runs_are_identical():
    src = np.random.RandomState(4).randint(0, 256, (8, 2160, 3840, 3)).astype(np.uint8)
    dev = torch.from_numpy(src).to(DEV)
    a = ops.letterbox_frames(dev, 360, 640, bgr=True)
    b = ops.letterbox_frames(dev, 360, 640, bgr=True)
    assert torch.equal(a, b)
    _check(a, R.letterbox(src, 360, 640, bgr=True), "2160x3840 x 8")


def _video(h0, w0, n):
    """n distinct source frames [n, 3, h0, w0]: eleven generated ones, shifted sideways from one repetition to the next."""
    base = synth.synth_frames_u8(11, h0, w0, 5)
    return np.concatenate([np.roll(base, 13 * k, axis=3) for k in range((n + 10) // 11)])[:n]


@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("size", [(720, 1280), (480, 640)], ids=["720x1280", "480x640_bars"])
def test_predict_video_from_source_size_frames(size, overlap):
    """44 source-size frames, time_dims 4, batch_size 2: five whole groups of 8 and a ragged group of 4.  Letterboxing inside
    the driver (device frames, pinned and pageable host frames, interleaved BGR as a decoder yields them) gives the maps of the
    same driver fed with frames the restatement letterboxed, bit for bit, at the source size."""
    from iip_uavsal_saliency_amd import UAVSal
    from iip_uavsal_saliency_amd.stream import predict_video
    h0, w0 = size
    rows, cols = 360, 640
    m = UAVSal(time_dims=4)
    synth.load_synth_weights(m, 0)
    m = m.to(DEV).eval()
    g = torch.Generator().manual_seed(3)
    gp, op_ = torch.rand((8, rows // 8, cols // 8), generator=g), torch.rand((20, rows // 8, cols // 8), generator=g)
    src = _video(h0, w0, 44)                                           # [44, 3, h0, w0] RGB
    boxed = torch.from_numpy(R.letterbox(src, rows, cols, "CHW")).to(DEV)
    want, wmaps = predict_video(m, boxed, gp, op_, batch_size=2, overlap=overlap, return_maps=True, out_size=(h0, w0))
    assert want.shape == (44, h0, w0) and wmaps.shape[0] == 44
    chw = torch.from_numpy(src)
    for name, frames in (("device", chw.to(DEV)), ("pinned", chw.pin_memory()), ("pageable", chw)):
        got, gmaps = predict_video(m, frames, gp, op_, batch_size=2, overlap=overlap, return_maps=True, model_size=(rows, cols))
        assert got.shape == (44, h0, w0), name
        assert torch.equal(gmaps, wmaps) and torch.equal(got, want), name
    bgr_hwc = torch.from_numpy(np.ascontiguousarray(src[:, ::-1].transpose(0, 2, 3, 1)))       # what cv2.VideoCapture yields
    for name, frames in (("device HWC BGR", bgr_hwc.to(DEV)), ("pinned HWC BGR", bgr_hwc.pin_memory())):
        got, gmaps = predict_video(m, frames, gp, op_, batch_size=2, overlap=overlap, return_maps=True, model_size=(rows, cols),
                                   frame_layout="HWC", bgr=True)
        assert torch.equal(gmaps, wmaps) and torch.equal(got, want), name
    # an explicit out_size still wins; without model_size the new keywords are refused
    small = predict_video(m, chw.to(DEV), gp, op_, batch_size=2, overlap=overlap, model_size=(rows, cols), out_size=(rows, cols))
    assert torch.equal(small, predict_video(m, boxed, gp, op_, batch_size=2, overlap=overlap))
    with pytest.raises(RuntimeError, match="model_size"):
        predict_video(m, boxed, gp, op_, batch_size=2, frame_layout="HWC")
