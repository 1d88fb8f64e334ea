"""Observed priors of a dataset without a GPU: the host path (`device="cpu"`, the specification of the device path) against
what the reference itself made of the same dataset trees (tests/golden/ob_priors.npz, see tests/prior_ref.py for what that
pins), the rounding rule, the PNG reader / writer, the file contract of `read_ob_priors` / `get_bias`, and the C ABI's
argument checks.  Every comparison is for equality."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

from iip_uavsal_saliency_amd import matio, pngio, priors

import prior_ref as R


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "ob_priors.npz"))


@pytest.fixture(scope="module")
def lib():
    from iip_uavsal_saliency_amd import build, _lib
    build.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ host path vs the reference

@pytest.mark.parametrize("name", sorted(R.DATASETS))
def test_mean_prior_map_cpu_reproduces_the_reference_pictures(golden, name):
    d = R.DATASETS[name]
    want = golden["png_" + name]
    for i, (vname, fix) in enumerate(R.videos(name)):
        out, image = priors.mean_prior_map(fix, d["out"][0], d["out"][1], device="cpu", with_image=True)
        assert image.dtype == np.uint8 and np.array_equal(image, want[i]), vname
        assert out.dtype == np.uint8 and np.array_equal(out, priors.letterbox_u8(want[i], *d["out"])), vname
        assert np.array_equal(out, priors.mean_prior_map(fix, d["out"][0], d["out"][1], device="cpu")), vname
    # the other layouts and a frame limit give what the same frames give
    vname, fix = R.videos(name)[0]
    fhw = np.ascontiguousarray(fix[:, :, 0, :].transpose(2, 0, 1))
    assert np.array_equal(priors.mean_prior_map(fhw, *d["out"], device="cpu"), priors.mean_prior_map(fix, *d["out"], device="cpu"))
    assert np.array_equal(priors.mean_prior_map(np.ascontiguousarray(fix[:, :, 0, :]), *d["out"], device="cpu", layout="HWF"),
                          priors.mean_prior_map(fix, *d["out"], device="cpu"))
    assert np.array_equal(priors.mean_prior_map(fix, *d["out"], frames=2, device="cpu"),
                          priors.mean_prior_map(fix[:, :, :, :2], *d["out"], device="cpu"))


@pytest.mark.parametrize("name", sorted(R.DATASETS))
def test_build_ob_priors_cpu_reproduces_the_reference_file(golden, tmp_path, name):
    d = R.DATASETS[name]
    tree = str(tmp_path / "data")
    vids = R.write_tree(tree, name)
    out_path = str(tmp_path / "out.mat")
    maps = priors.build_ob_priors(tree, out_path, d["phase_gen"], d["out"][0], d["out"][1], R.CHANNELS, device="cpu")
    want = golden["maps_" + name]
    assert maps.dtype == np.float32 and maps.shape == want.shape == (d["out"][0], d["out"][1], R.CHANNELS)
    assert np.array_equal(maps, want)
    assert np.array_equal(matio.loadmat(out_path)["PriorMaps"], want)
    for i, (vname, _) in enumerate(vids):
        assert np.array_equal(pngio.read_gray(os.path.join(tree, "priors", vname + ".png")), golden["png_" + name][i]), vname
    # the state after the first run: the pictures are read, maps/ is not needed any more
    os.rename(os.path.join(tree, "maps"), os.path.join(tree, "maps_moved"))
    again = priors.build_ob_priors(tree, None, d["phase_gen"], d["out"][0], d["out"][1], R.CHANNELS, device="cpu")
    assert np.array_equal(again, want)


def test_dataset_shapes_cover_what_they_claim():
    from iip_uavsal_saliency_amd.ops import letterbox_geometry
    branches = {n: letterbox_geometry(*d["src"], *d["out"])[4] for n, d in R.DATASETS.items()}
    assert set(branches.values()) == {"cols", "rows"}, branches
    counts = {n: d["train"] + d["val"] for n, d in R.DATASETS.items()}
    assert counts == {"p3": 3, "p20": 20, "p41": 41, "p47": 47}
    for n, last in (("p41", 3), ("p47", 9)):                # videos in the last channel's mean: P - (20 * count - count)
        count = counts[n] // R.CHANNELS
        assert count == 2 and counts[n] - (R.CHANNELS * count - count) == last
    assert [n for n, d in R.DATASETS.items() if d["phase_gen"] == "train_val"] == ["p41"]
    assert R.DATASETS["p41"]["src"] == R.DATASETS["p41"]["out"]


def test_no_write_png_leaves_the_tree_alone(tmp_path):
    tree = str(tmp_path / "data")
    R.write_tree(tree, "p3")
    priors.build_ob_priors(tree, None, "train", 9, 16, R.CHANNELS, device="cpu", write_png=False)
    assert not os.path.exists(os.path.join(tree, "priors"))


# ------------------------------------------------------------------------------------------------ rounding

def test_means_on_a_tie_round_half_to_even():
    a, want = R.tie_video()
    assert a.astype(np.int64).sum(0).tolist() == [[0, 1, 3, 5, 510]]
    assert 255.0 + priors.EPS == 255.0
    out, image = priors.mean_prior_map(a, 1, 5, device="cpu", with_image=True)
    assert image.tolist() == want.tolist() == [[0, 0, 2, 2, 255]]
    assert np.array_equal(out, want)                       # same size: the resize is the identity


def test_constant_video_is_an_all_zero_map():
    a, want = R.constant_video()
    with np.errstate(all="raise"):                         # no 0 / 0 on the way
        out, image = priors.mean_prior_map(a, 9, 16, device="cpu", with_image=True)
    assert np.array_equal(image, want) and not out.any() and out.shape == (9, 16)


def test_bad_inputs_are_refused():
    a, _ = R.tie_video()
    with pytest.raises(ValueError):
        priors.mean_prior_map(a.astype(np.float32), 1, 5, device="cpu")
    with pytest.raises(ValueError):
        priors.mean_prior_map(a[:0], 1, 5, device="cpu")
    with pytest.raises(ValueError):
        priors.mean_prior_map(np.zeros((2, 3, 2, 4), np.uint8), 1, 5, device="cpu")     # 4-d but not [H0,W0,1,F]
    with pytest.raises(NotImplementedError):
        priors.ob_priors_file("uav2", "test")


# ------------------------------------------------------------------------------------------------ pngio

def _png(w, h, rows, colour=0, depth=8, interlace=0, split=False):
    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)
    z = zlib.compress(rows)
    idat = chunk(b"IDAT", z[:5]) + chunk(b"IDAT", z[5:]) if split else chunk(b"IDAT", z)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour, 0, 0, interlace))
            + chunk(b"tEXt", b"k\x00v") + idat + chunk(b"IEND", b""))


def _filter_rows(img, ft):
    """the PNG filters applied forwards, straight from the specification (bytes modulo 256)"""
    h, w = img.shape
    a = img.astype(np.int64)
    out = bytearray()
    for y in range(h):
        out.append(ft)
        for x in range(w):
            left = a[y, x - 1] if x else 0
            up = a[y - 1, x] if y else 0
            ul = a[y - 1, x - 1] if x and y else 0
            if ft == 1:
                pred = left
            elif ft == 2:
                pred = up
            elif ft == 3:
                pred = (left + up) // 2
            else:
                p = left + up - ul
                pa, pb, pc = abs(p - left), abs(p - up), abs(p - ul)
                pred = left if pa <= pb and pa <= pc else (up if pb <= pc else ul)
            out.append(int(a[y, x] - pred) & 255)
    return bytes(out)


def test_png_round_trip(tmp_path):
    rng = np.random.RandomState(5)
    for shape in [(1, 1), (7, 13), (45, 80)]:
        img = rng.randint(0, 256, shape).astype(np.uint8)
        path = str(tmp_path / ("a%dx%d.png" % shape))
        pngio.write_gray(path, img)
        back = pngio.read_gray(path)
        assert back.dtype == np.uint8 and np.array_equal(back, img)
    with pytest.raises(ValueError):
        pngio.write_gray(str(tmp_path / "f.png"), img.astype(np.float64))


@pytest.mark.parametrize("ft", [1, 2, 3, 4])
def test_png_reader_undoes_every_filter(ft):
    rng = np.random.RandomState(ft)
    img = rng.randint(0, 256, (6, 11)).astype(np.uint8)
    img[2] = 255                                            # wrap-arounds in both directions
    img[3] = 0
    assert np.array_equal(pngio.decode_gray(_png(11, 6, _filter_rows(img, ft), split=True)), img)


def test_png_reader_mixes_filters_per_row():
    rng = np.random.RandomState(9)
    img = rng.randint(0, 256, (5, 8)).astype(np.uint8)
    rows = b"".join(_filter_rows(img, ft)[9 * y:9 * y + 9] if ft else bytes([0]) + img[y].tobytes()
                    for y, ft in enumerate([0, 4, 1, 3, 2]))
    assert np.array_equal(pngio.decode_gray(_png(8, 5, rows)), img)


def test_png_reader_refuses_what_it_does_not_decode():
    grey = bytes([0]) + bytes(4)
    assert pngio.decode_gray(_png(4, 1, grey)).tolist() == [[0, 0, 0, 0]]
    for kw, rows in [(dict(colour=2), bytes([0]) + bytes(12)), (dict(colour=3), grey), (dict(colour=4), bytes([0]) + bytes(8)),
                     (dict(depth=16), bytes([0]) + bytes(8)), (dict(interlace=1), grey)]:
        with pytest.raises(ValueError):
            pngio.decode_gray(_png(4, 1, rows, **kw))
    with pytest.raises(ValueError):
        pngio.decode_gray(b"GIF89a" + bytes(20))
    bad = bytearray(_png(4, 1, grey))
    bad[-20] ^= 1                                           # inside the IDAT chunk: its CRC no longer matches
    with pytest.raises(ValueError):
        pngio.decode_gray(bytes(bad))


# ------------------------------------------------------------------------------------------------ the file contract

def test_read_ob_priors_loads_or_builds(golden, tmp_path):
    d = R.DATASETS["p41"]
    tree, pdir = str(tmp_path / "data"), str(tmp_path / "files")
    os.makedirs(pdir)
    want = golden["maps_p41"]
    # an existing file is loaded; the dataset is not opened (there is none)
    path = priors.ob_priors_file("p41", "train_val", pdir)
    assert os.path.basename(path) == "P41_ob_priors_train_val.mat"
    assert os.path.basename(priors.ob_priors_file("uav2", "train")) == "UAV2_ob_priors_train.mat"
    matio.savemat(path, {"PriorMaps": want})
    got = priors.read_ob_priors(str(tmp_path / "nowhere"), "p41", "train_val", 9, 16, R.CHANNELS, priors_dir=pdir, device="cpu")
    assert np.array_equal(got, want)
    # a missing file is built and written, and found by the second call
    os.remove(path)
    R.write_tree(tree, "p41")
    got = priors.read_ob_priors(tree, "p41", "train_val", 9, 16, R.CHANNELS, priors_dir=pdir, device="cpu")
    assert np.array_equal(got, want) and os.path.exists(path)
    os.rename(tree, tree + "_moved")
    got = priors.read_ob_priors(tree, "p41", "train_val", 9, 16, R.CHANNELS, priors_dir=pdir, device="cpu")
    assert np.array_equal(got, want)


def test_get_ob_priors_and_get_bias_build_a_missing_file(golden, tmp_path):
    tree = str(tmp_path / "data")
    R.write_tree(tree, "p47")
    path = str(tmp_path / "P47_ob_priors_train.mat")
    with pytest.raises(ValueError):
        priors.get_ob_priors(path, 2, 12, 10)              # today's behaviour without a dataset
    with pytest.raises(ValueError):
        priors.get_bias((0, 1, 1), 2, 12, 10, ob_prior_path=path, device="cpu")
    assert not os.path.exists(path)
    want = golden["maps_p47"]
    g, o = priors.get_bias((0, 1, 1), 3, 12, 10, ob_prior_path=path, device="cpu", datapath=tree, dataset="p47")
    assert g.numel() == 0 and tuple(o.shape) == (3, R.CHANNELS, 12, 10)
    assert np.array_equal(o[1].numpy(), want.transpose(2, 0, 1))
    assert np.array_equal(matio.loadmat(path)["PriorMaps"], want)
    ims = priors.get_ob_priors(path, 2, 12, 10)            # found now, no dataset needed
    assert ims.shape == (2, 12, 10, R.CHANNELS) and np.array_equal(ims[0], want)


# ------------------------------------------------------------------------------------------------ C ABI

def test_prior_descriptors_and_symbols(lib):
    from iip_uavsal_saliency_amd import _lib
    names = [s[0] for s in _lib.SYMBOLS]
    for n in ("uavsal_prior_accumulate", "uavsal_prior_finish", "uavsal_prior_slab_frames", "uavsal_prior_sizeof_desc"):
        assert n in names
    assert lib.uavsal_prior_sizeof_desc(0) == C.sizeof(_lib.PriorAccDesc)
    assert lib.uavsal_prior_sizeof_desc(1) == C.sizeof(_lib.PriorFinishDesc)
    assert lib.uavsal_prior_sizeof_desc(2) < 0
    assert lib.uavsal_abi_version() == 20
    # slabs: never shorter than the documented minimum; 720p x 600 frames is 2 slabs of 300, 360p x 600 is 5 of 120
    assert lib.uavsal_prior_slab_frames(16 * 16, 67) == _lib.PRIOR_MIN_SLAB == 32
    assert lib.uavsal_prior_slab_frames(720 * 1280, 600) == 300
    assert lib.uavsal_prior_slab_frames(360 * 640, 600) == 120
    assert lib.uavsal_prior_slab_frames(2160 * 3840, 600) == 600
    assert lib.uavsal_prior_slab_frames(0, 5) == 0 and lib.uavsal_prior_slab_frames(5, 0) == 0


def test_prior_argument_validation_without_gpu(lib):
    """Rejected descriptors return before any HIP call, so this runs without a device."""
    from iip_uavsal_saliency_amd import _lib as L
    d = L.PriorAccDesc()
    assert lib.uavsal_prior_accumulate(None, None) == -1
    assert lib.uavsal_prior_accumulate(C.byref(d), None) == -1                 # null pointers
    d.frames, d.acc = 16, 16
    assert lib.uavsal_prior_accumulate(C.byref(d), None) == -1                 # non-positive sizes
    d.n_img, d.h0, d.w0 = 1, 4, 0
    assert lib.uavsal_prior_accumulate(C.byref(d), None) == -1
    d.w0, d.row_pitch = 4, -4
    assert lib.uavsal_prior_accumulate(C.byref(d), None) == -1                 # a negative pitch
    d.row_pitch, d.acc = 4, 18
    assert lib.uavsal_prior_accumulate(C.byref(d), None) == -2                 # acc not an int32 address
    d.acc, d.n_img = 16, L.PRIOR_MAX_FRAMES + 1
    assert lib.uavsal_prior_accumulate(C.byref(d), None) == -3                 # 255 * n_img >= 2^31
    d.n_img, d.h0, d.w0 = 1, 65536, 65536
    assert lib.uavsal_prior_accumulate(C.byref(d), None) == -3                 # h0 * w0 >= 2^31

    f = L.PriorFinishDesc()
    assert lib.uavsal_prior_finish(None, None) == -1
    assert lib.uavsal_prior_finish(C.byref(f), None) == -1                     # null pointers
    f.acc, f.ws, f.out = 16, 16, 16
    f.h0, f.w0, f.h, f.w = 4, 4, 4, 4
    assert lib.uavsal_prior_finish(C.byref(f), None) == -1                     # n_frames == 0
    f.n_frames = -3
    assert lib.uavsal_prior_finish(C.byref(f), None) == -1
    f.n_frames, f.h = 2, 0
    assert lib.uavsal_prior_finish(C.byref(f), None) == -1                     # non-positive size
    f.h, f.ws = 4, 18
    assert lib.uavsal_prior_finish(C.byref(f), None) == -2
    f.ws, f.n_frames = 16, L.PRIOR_MAX_FRAMES + 1
    assert lib.uavsal_prior_finish(C.byref(f), None) == -3
    f.n_frames, f.h0, f.w0, f.h, f.w = 2, 100, 1, 9, 16
    assert lib.uavsal_prior_finish(C.byref(f), None) == -3                     # a picture of zero columns (1 * 9 // 100)
