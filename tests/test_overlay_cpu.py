"""Heat-map overlay without a GPU: the numpy restatement (tests/overlay_ref.py) against its known answers, the host geometry
against answers worked by hand, the default colour table against what its construction implies, the C entry point's symbols,
descriptor and argument checks, the Python surface, and the condition on the inputs of the GPU comparison."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import _lib, stream, vis

import overlay_ref as R

CASES = list(R.cases())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_gives_the_known_answers(case):
    _, kw, want = case
    got, v = R.overlay(**kw)
    assert got.dtype == np.uint8 and got.shape == want.shape and v.shape == want.shape
    assert np.array_equal(got, want)


def test_geometry_helper_equals_hand_worked_answers_and_the_restatement():
    known = R.geometry_cases()
    assert sorted(known) == sorted(R.GEOMETRY_SIZES)
    for (h, w), want in known.items():
        assert vis.visual_geometry(h, w) == want == R.visual_geometry(h, w)
    for h in (1, 2, 100, 359, 360, 361, 405, 719, 720, 721, 1080, 1280, 2160):
        for w in (1, 3, 100, 639, 640, 641, 719, 720, 1279, 1280, 1281, 1920, 3840):
            if min(R.visual_geometry(h, w)) <= 0:                       # e.g. 1 x 1280: ratio 2, no mid rows
                with pytest.raises(RuntimeError, match="no picture"):
                    vis.visual_geometry(h, w)
            else:
                assert vis.visual_geometry(h, w) == R.visual_geometry(h, w)
    with pytest.raises(RuntimeError):
        vis.visual_geometry(0, 640)


def test_float_resize_rule_identity_and_exact_doubling():
    a = np.random.RandomState(1).rand(5, 7, 3)
    assert np.array_equal(R.resize_f64(a, 5, 7), a)
    s, s1, f = R.lin_taps(8, 4)
    assert list(s) == [0, 0, 0, 1, 1, 2, 2, 3] and list(s1) == [1, 1, 1, 2, 2, 3, 3, 3]
    assert list(f) == [0.0, 0.25, 0.75, 0.25, 0.75, 0.25, 0.75, 0.0]


def test_default_table_is_what_its_construction_implies():
    t = vis.JET_BGR
    assert t.shape == (256, 3) and t.dtype == np.uint8
    assert np.array_equal(t, R.jet_table())
    b, g, r = R.jet_knots()
    # the endpoints are the end knots: blue starts at 9/16 and ends at 0, green is 0 at both ends, red ends at 8/16
    assert (b[0], g[0], r[0]) == (0.5625, 0.0, 0.0) and (b[63], g[63], r[63]) == (0.0, 0.0, 0.5)
    assert tuple(t[0]) == (143, 0, 0) and tuple(t[255]) == (0, 0, 128)          # 143.4375 -> 143; 127.5 -> 128, half to even
    for ch, k in enumerate((b, g, r)):
        col = t[:, ch].astype(int)
        top = np.flatnonzero(col == 255)
        assert len(top) and np.all(np.diff(top) == 1)                           # one plateau at 255
        assert np.all(np.diff(col[:top[0] + 1]) >= 0) and np.all(np.diff(col[top[-1]:]) <= 0)      # rises to it, falls from it
        ones = np.flatnonzero(k == 1.0)                                          # the knots' plateau, in table indices
        assert top[0] == int(np.ceil(ones[0] * 255 / 63 - 1e-9)) or col[top[0] - 1] < 255
        assert abs(top[0] - ones[0] * 255 / 63) < 4.1 and abs(top[-1] - ones[-1] * 255 / 63) < 4.1
        zero = np.flatnonzero(k == 0.0)
        for z in zero:                                                           # a zero knot between zero knots is a zero entry
            if z - 1 in zero and z + 1 in zero:
                assert col[int(round(z * 255 / 63))] == 0


# ------------------------------------------------------------------------------------------------ C ABI

def test_overlay_symbols_descriptor_and_abi_version():
    lib = _lib.load()
    assert hasattr(lib, "uavsal_overlay_u8") and hasattr(lib, "uavsal_overlay_workspace_bytes")
    assert lib.uavsal_sizeof_desc(16) == C.sizeof(_lib.OverlayDesc)
    assert _lib.DESC_TYPES[16] is _lib.OverlayDesc
    assert lib.uavsal_abi_version() == 20


def _desc(**kw):
    d = _lib.OverlayDesc()
    d.frames, d.map, d.lut, d.out, d.ws = 0x10001, 0x20003, 0x30000, 0x40000, 0x50000
    d.n_img, d.layout, d.h0, d.w0, d.map_h, d.map_w = 2, _lib.LETTERBOX_HWC, 72, 128, 72, 128
    d.row_pitch, d.plane_pitch, d.img_pitch, d.map_img_pitch = 3 * 128, 0, 3 * 128 * 72, 128 * 72
    d.mid_h, d.mid_w, d.out_h, d.out_w = 36, 64, 72, 128
    d.ws_bytes = 1 << 30
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("kw,code", [
    (dict(frames=0), -1), (dict(map=0), -1), (dict(lut=0), -1), (dict(out=0), -1), (dict(ws=0), -1), (dict(n_img=0), -1),
    (dict(h0=0), -1), (dict(map_w=0), -1), (dict(mid_h=0), -1), (dict(out_w=-1), -1), (dict(layout=2), -1),
    (dict(fix=0x60000, fix_h=0, fix_w=4), -1),
    (dict(ws_bytes=1024), -1),                                           # smaller than uavsal_overlay_workspace_bytes
    (dict(ws=0x50010), -2),                                              # workspace not 256-byte aligned
    (dict(row_pitch=3 * 128 - 1), -3),                                   # rows overlap
    (dict(img_pitch=3 * 128 * 72 - 1), -3),                              # images overlap
    (dict(map_img_pitch=128 * 72 - 1), -3),
    (dict(layout=1, row_pitch=128, plane_pitch=128 * 72 - 1, img_pitch=3 * 128 * 72), -3),
    (dict(n_img=65536), -3),
    (dict(n_img=1, h0=8, w0=40000, row_pitch=120000), -3),               # source rows beyond the LDS staging
    (dict(n_img=1, mid_w=30000), -3),                                    # mid rows beyond it
    (dict(n_img=1, out_w=20000), -3),                                    # the output's column table beyond it
])
def test_overlay_entry_point_rejects_bad_descriptors(kw, code):
    """Argument errors come back as negative codes before anything is launched (no device needed)."""
    lib = _lib.load()
    assert lib.uavsal_overlay_u8(C.byref(_desc(**kw)), None) == code
    assert lib.uavsal_overlay_u8(None, None) == -1


def test_workspace_size_covers_the_parts():
    lib = _lib.load()
    d = _desc(n_img=20, h0=720, w0=1280, mid_h=360, mid_w=640, out_h=720, out_w=1280)
    plain = lib.uavsal_overlay_workspace_bytes(C.byref(d))
    assert plain >= 20 * (32 + 360 * 640 * 4) and plain % 256 == 0
    d.fix, d.fix_h, d.fix_w = 0x60000, 720, 1280
    assert lib.uavsal_overlay_workspace_bytes(C.byref(d)) >= plain + 20 * 720 * 1280
    assert lib.uavsal_overlay_workspace_bytes(None) == -1


# ------------------------------------------------------------------------------------------------ Python surface

def test_python_surface():
    import iip_uavsal_saliency_amd as P
    assert P.overlay_frames is vis.overlay_frames and P.visual_video is vis.visual_video and P.visual_geometry is vis.visual_geometry
    sig = inspect.signature(vis.overlay_frames)
    assert list(sig.parameters) == ["frames_u8", "sal_u8", "fix", "mid_size", "out_size", "layout", "colormap"]
    assert sig.parameters["layout"].default == "HWC"
    sig = inspect.signature(vis.visual_video)
    assert list(sig.parameters)[:6] == ["frames", "salmap", "fix", "with_fix", "group", "sink"]
    assert sig.parameters["group"].default == 20 and sig.parameters["with_fix"].default == 0
    assert inspect.signature(stream.predict_video).parameters["overlay"].default is None
    for bad in (torch.zeros((2, 8, 8, 3), dtype=torch.uint8), np.zeros((2, 8, 8, 3), np.uint8)):
        with pytest.raises(RuntimeError, match="uint8 cuda frames"):
            vis.overlay_frames(bad, torch.zeros((2, 8, 8), dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------ the GPU test's inputs

@pytest.mark.parametrize("name", R.COMPARED)
def test_excused_share_of_every_gpu_input_is_within_the_cap(name):
    """The GPU comparison accepts either neighbour where the restatement's double lies within 1e-9 of a half-integer.  That
    excuse may cover at most 1e-5 of the bytes of any input -- the seeded inputs and everything the GPU tests derive from
    them (`overlay_ref.COMPARED`) -- checked here from the restatement alone.  The known answers of `cases()` are compared
    on the GPU with exact equality: nothing is excused there."""
    want, v = R.gpu_want(name)
    share = float(np.count_nonzero(R.excused(v))) / v.size
    print("%s: %d bytes, excused share %.3g" % (name, v.size, share))
    assert share <= 1e-5
    assert want.max() == 255 and np.isfinite(v).all()


def test_a_known_answer_holds_an_exact_tie():
    """`empty_map` puts bytes exactly at 127.5, so the exact comparison of the known answers pins half-to-even (128)."""
    kw, want = [(k, w) for n, k, w in R.cases() if n == "empty_map"][0]
    _, v = R.overlay(**kw)
    assert np.count_nonzero(v == 127.5) == 16 and np.all(want[v == 127.5] == 128)
