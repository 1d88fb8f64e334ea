"""Observed priors on the GPU: the streaming sum (`ops.fixmap_accumulate`) against numpy's integer sum, the finish step
(`ops.prior_map_from_sum`) and the dataset pass (`priors.build_ob_priors`) against the host path, which
tests/test_ob_priors_cpu.py holds to the reference's own output.  Everything here is integer-exact or a handful of IEEE
double operations: every comparison is for equality.

Shapes are the smallest at which the kernels can go wrong: a 37x53 plane (no multiple of 16 either way, frames an odd
number of bytes apart: the byte-wise kernel), 72x80 planes (a multiple of 16 bytes: the 16-byte kernel, two blocks of
lanes, with and without unaligned ends), a 16x16 plane with frames across three slabs, and sums beyond 16 bits."""
import os

import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import _lib, matio, ops, pngio, priors

import prior_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _layouts(a):
    """a uint8 [F,H0,W0] array as device tensors in every layout prepare_gaze reads, with the `layout` argument"""
    t = torch.from_numpy(a).to(DEV)
    F, h0, w0 = a.shape
    big = torch.full((F + 2, h0 + 3, w0 + 5), 9, dtype=torch.uint8, device=DEV)
    big[1:F + 1, 2:h0 + 2, 1:w0 + 1] = t
    odd = torch.full((F * h0 * w0 + 3,), 9, dtype=torch.uint8, device=DEV)
    odd[3:] = t.reshape(-1)
    return [("FHW", t, None),
            ("HW1F", t.permute(1, 2, 0)[:, :, None, :].contiguous(), None),
            ("HWF", t.permute(1, 2, 0).contiguous(), "HWF"),
            ("matlab order", t.permute(0, 2, 1).contiguous().permute(2, 1, 0)[:, :, None, :], None),     # [H0,W0,1,F], rows fastest
            ("slice of a larger buffer", big[1:F + 1, 2:h0 + 2, 1:w0 + 1], None),
            ("odd byte offset", odd[3:].view(F, h0, w0), None)]


def _video(F, h0, w0, seed):
    rng = np.random.RandomState(seed)
    return (rng.randint(0, 256, (F, h0, w0)) * (rng.rand(F, h0, w0) < 0.6)).astype(np.uint8)


def _sum(a):
    return a.sum(axis=0, dtype=np.int64).astype(np.int32)


# ------------------------------------------------------------------------------------------------ accumulate

@pytest.fixture(scope="module")
def video67():
    a = _video(67, 37, 53, 1)
    return a, _sum(a)


@pytest.mark.parametrize("F", [1, 7, 67])
def test_accumulate_matches_numpy_in_every_layout(video67, F):
    a = video67[0][:F]
    want = _sum(a)
    for name, t, layout in _layouts(a):
        acc = ops.fixmap_accumulate(t, layout=layout)
        assert acc.dtype == torch.int32 and tuple(acc.shape) == (37, 53) and acc.n_frames == F, name
        assert np.array_equal(acc.cpu().numpy(), want), name


def test_two_chunks_equal_one(video67):
    a, want = video67
    for name, t, layout in _layouts(a):
        if layout == "HWF":
            first, second = t[:, :, :40], t[:, :, 40:]
        elif t.dim() == 4:
            first, second = t[:, :, :, :40], t[:, :, :, 40:]
        else:
            first, second = t[:40], t[40:]
        acc = ops.fixmap_accumulate(first, layout=layout)
        back = ops.fixmap_accumulate(second, acc, layout=layout)
        assert back is acc and acc.n_frames == 67, name
        assert np.array_equal(acc.cpu().numpy(), want), name


@pytest.mark.parametrize("F", [1, 9, 67])
@pytest.mark.parametrize("offset", [0, 5, 16])
def test_accumulate_contiguous_planes_of_16_byte_multiples(F, offset):
    """72 x 80 = 5760 bytes = 360 lanes of 16 bytes: the vector kernel, two blocks; `offset` 5 puts 11 bytes in front of the
    first aligned address and 5 behind the last.  Row-major planes and MATLAB order (a transposed `acc`)."""
    a = _video(F, 72, 80, 10 + F)
    want = _sum(a)
    buf = torch.full((offset + a.size + 7,), 201, dtype=torch.uint8, device=DEV)
    buf[offset:offset + a.size] = torch.from_numpy(a).to(DEV).reshape(-1)
    acc = ops.fixmap_accumulate(buf[offset:offset + a.size].view(F, 72, 80))
    assert acc.is_contiguous() and np.array_equal(acc.cpu().numpy(), want)
    buf[offset:offset + a.size] = torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 1))).to(DEV).reshape(-1)
    m = buf[offset:offset + a.size].view(F, 80, 72).permute(2, 1, 0)[:, :, None, :]      # [H0,W0,1,F] as loadmat yields it
    acc = ops.fixmap_accumulate(m)
    assert acc.stride() == (1, 72) and np.array_equal(acc.cpu().numpy(), want)
    # a given acc in the other pixel order is still summed correctly (the byte-wise kernel)
    acc = ops.fixmap_accumulate(m, torch.zeros((72, 80), dtype=torch.int32, device=DEV))
    assert np.array_equal(acc.cpu().numpy(), want)


def test_sums_need_more_than_sixteen_bits():
    a = np.full((300, 5, 19), 255, dtype=np.uint8)
    for name, t, layout in _layouts(a):
        acc = ops.fixmap_accumulate(t, layout=layout)
        assert acc.cpu().numpy().tolist() == [[76500] * 19] * 5, name
    b = np.full((300, 4, 16), 255, dtype=np.uint8)          # 64-byte planes: the vector kernel
    acc = ops.fixmap_accumulate(torch.from_numpy(b).to(DEV))
    assert acc.cpu().numpy().tolist() == [[76500] * 16] * 4


def test_frames_across_slabs_equal_one_slab():
    S = _lib.PRIOR_MIN_SLAB
    F = 2 * S + 3
    assert ops.prior_slab_frames(16 * 16, F) == S           # three slabs: S, S and 3 frames
    a = _video(F, 16, 16, 4)
    t = torch.from_numpy(a).to(DEV)
    acc = ops.fixmap_accumulate(t)
    assert np.array_equal(acc.cpu().numpy(), _sum(a))
    one = None                                              # the same frames, never more than one slab per call
    for f0 in range(0, F, S):
        assert ops.prior_slab_frames(16 * 16, min(S, F - f0)) >= min(S, F - f0)
        one = ops.fixmap_accumulate(t[f0:f0 + S], one)
    assert torch.equal(one, acc)
    m = t.permute(0, 2, 1).contiguous().permute(2, 1, 0)[:, :, None, :]
    assert np.array_equal(ops.fixmap_accumulate(m).cpu().numpy(), _sum(a))
    assert np.array_equal(ops.fixmap_accumulate(t.permute(1, 2, 0).contiguous(), layout="HWF").cpu().numpy(), _sum(a))


def test_two_runs_give_the_same_bytes(video67):
    a = _video(67, 72, 80, 8)
    for t in (torch.from_numpy(a).to(DEV), torch.from_numpy(video67[0]).to(DEV)):
        first, second = ops.fixmap_accumulate(t), ops.fixmap_accumulate(t)
        assert torch.equal(first, second)
        x = ops.prior_map_from_sum(first, 67, 9, 16, with_image=True)
        y = ops.prior_map_from_sum(second, 67, 9, 16, with_image=True)
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])


def test_accumulate_refuses_what_does_not_fit(video67):
    t = torch.from_numpy(video67[0][:3]).to(DEV)
    with pytest.raises(RuntimeError):
        ops.fixmap_accumulate(t, torch.zeros((37, 54), dtype=torch.int32, device=DEV))       # another size
    with pytest.raises(RuntimeError):
        ops.fixmap_accumulate(t, torch.zeros((37, 53), dtype=torch.int32))                   # another device
    with pytest.raises(RuntimeError):
        ops.fixmap_accumulate(t, torch.zeros((37, 53), dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError):
        ops.fixmap_accumulate(t.cpu())
    with pytest.raises(RuntimeError):
        ops.fixmap_accumulate(t.float())
    acc = torch.zeros((37, 53), dtype=torch.int32, device=DEV)
    acc.n_frames = _lib.PRIOR_MAX_FRAMES - 2                # 255 * (this + 3) does not fit an int32
    with pytest.raises(RuntimeError):
        ops.fixmap_accumulate(t, acc)
    assert not acc.any()
    with pytest.raises(RuntimeError):
        ops.prior_map_from_sum(acc, 0, 9, 16)
    with pytest.raises(RuntimeError):
        ops.prior_map_from_sum(acc.cpu(), 3, 9, 16)


# ------------------------------------------------------------------------------------------------ finish

def _finish_cases():
    for name in sorted(R.DATASETS):
        d = R.DATASETS[name]
        for vname, fix in R.videos(name)[:4]:
            yield vname, fix, d["out"]
    yield "tie", R.tie_video()[0], (1, 5)
    yield "tie letterboxed", R.tie_video()[0], (4, 7)
    yield "constant", R.constant_video()[0], (9, 16)
    yield "rows branch", _video(5, 24, 64, 2), (36, 64)
    yield "cols branch", _video(5, 48, 30, 3), (12, 10)
    yield "same size", _video(6, 9, 16, 5), (9, 16)
    yield "reduced 720p-like", _video(3, 90, 160, 6), (45, 80)


def test_finish_matches_the_host_path():
    for name, fix, (h, w) in _finish_cases():
        want, want_image = priors.mean_prior_map(fix, h, w, device="cpu", with_image=True)
        t = torch.from_numpy(fix).to(DEV)
        acc = ops.fixmap_accumulate(t)
        n = fix.shape[3] if fix.ndim == 4 else fix.shape[0]
        out, image = ops.prior_map_from_sum(acc, n, h, w, with_image=True)
        assert out.dtype == torch.uint8 and tuple(out.shape) == (h, w), name
        assert np.array_equal(image.cpu().numpy(), want_image), name
        assert np.array_equal(out.cpu().numpy(), want), name
        alone = ops.prior_map_from_sum(acc, n, h, w)
        assert torch.is_tensor(alone) and np.array_equal(alone.cpu().numpy(), want), name
        # the whole device path, from host data in chunks and from device data
        got = priors.mean_prior_map(fix, h, w, device=DEV, chunk_frames=2, with_image=True)
        assert np.array_equal(got[0], want) and np.array_equal(got[1], want_image), name
        assert np.array_equal(priors.mean_prior_map(t, h, w, device=DEV), want), name
    a, q = R.tie_video()
    acc = ops.fixmap_accumulate(torch.from_numpy(a).to(DEV))
    assert ops.prior_map_from_sum(acc, 2, 1, 5, with_image=True)[1].cpu().numpy().tolist() == q.tolist() == [[0, 0, 2, 2, 255]]


def test_frame_limit_and_host_layouts():
    a = _video(9, 16, 24, 12)
    want = priors.mean_prior_map(a[:4], 9, 16, device="cpu")
    assert np.array_equal(priors.mean_prior_map(a, 9, 16, frames=4, device=DEV, chunk_frames=3), want)
    hwf = np.ascontiguousarray(a.transpose(1, 2, 0))
    assert np.array_equal(priors.mean_prior_map(hwf, 9, 16, frames=4, device=DEV, layout="HWF"), want)
    assert np.array_equal(priors.mean_prior_map(torch.from_numpy(hwf).to(DEV), 9, 16, frames=4, device=DEV, layout="HWF"), want)


# ------------------------------------------------------------------------------------------------ a dataset

def test_build_ob_priors_on_the_device_equals_the_host_path(golden_dir, tmp_path):
    d = R.DATASETS["p47"]
    trees = {}
    for dev in ("cpu", DEV):
        tree = str(tmp_path / dev.replace(":", "_"))
        vids = R.write_tree(tree, "p47")
        out_path = os.path.join(tree, "P47_ob_priors_train.mat")
        maps = priors.build_ob_priors(tree, out_path, d["phase_gen"], d["out"][0], d["out"][1], R.CHANNELS, device=dev)
        trees[dev] = (tree, out_path, maps)
    want = np.load(os.path.join(golden_dir, "ob_priors.npz"))["maps_p47"]
    assert np.array_equal(trees["cpu"][2], want) and np.array_equal(trees[DEV][2], want)
    # (the first 512 bytes of a v7.3 .mat are a text header with the time of writing)
    assert open(trees["cpu"][1], "rb").read()[512:] == open(trees[DEV][1], "rb").read()[512:]
    assert np.array_equal(matio.loadmat(trees[DEV][1])["PriorMaps"], want)
    for vname, _ in vids:
        a, b = (open(os.path.join(trees[k][0], "priors", vname + ".png"), "rb").read() for k in ("cpu", DEV))
        assert a == b, vname
    assert np.array_equal(pngio.read_gray(os.path.join(trees[DEV][0], "priors", vids[0][0] + ".png")),
                          np.load(os.path.join(golden_dir, "ob_priors.npz"))["png_p47"][0])
