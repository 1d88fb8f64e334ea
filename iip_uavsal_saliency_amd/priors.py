"""Centre-bias priors of the reference caller without cv2 / hdf5storage.

`get_bias` mirrors `Demo_Test.get_bias` (Demo_Test.py:14-27): it returns the two NCHW float32
tensors `[gauss [n,8,h,w], ob [n,20,h,w]]` the model's `cb` argument expects.
  * gaussian priors: `get_guasspriors` (utils_data.py:449-469) -- the closed form of
    `st_get_gaussmaps` + per-channel min-max, which is bit-identical to the shipped
    `gauss_priors.mat` (checked in tests/test_host_cpu.py), or the file itself if given;
  * observed priors: `get_ob_priors` / `read_ob_priors` (utils_data.py:552-604) read
    `<DATASET>_ob_priors_train.mat` (MATLAB v7.3 = HDF5) through `matio.loadmat`.
Resized priors: when the stored map size differs from the requested one the reference letterboxes
each map with `padding()` (utils_data.py:321-343) -- cv2.resize (INTER_LINEAR) to the largest size of the
same aspect ratio that fits, pasted centred into a zero array of dtype **uint8** (utils_data.py:460-464,
595-599) -- so the [0,1] floats are truncated to {0,1} (only exact 1.0 survives).  `quirk=True` (default)
reproduces that rule -- pinned to cv2's DOCUMENTED half-pixel INTER_LINEAR mapping, not to cv2 itself (absent here), and the
maps are resized in float32 where cv2 would resize a float64 prior file in double: a value that lands within one float32 ulp
of 1.0 can fall on the other side of the truncation; `quirk=False` keeps the resized floats.
Host-side numpy; this is caller code, not part of the device path.

Building the observed priors of a new dataset (`read_ob_priors` -> `get_meanmaps`, utils_data.py:497-589) is here too:
`mean_prior_map` (one video's `fixMap` -> its prior picture, the streaming sum on the device through
`ops.fixmap_accumulate` / `ops.prior_map_from_sum`, or `device="cpu"`: the same bytes in numpy, the specification the
device path is tested against), `build_ob_priors` (a dataset tree -> `priors/<video>.png` and the 20-channel file) and
`read_ob_priors` (load the file, or build it when it is missing).  cv2's part -- rounding a float64 picture on
`imwrite`, the 8-bit INTER_LINEAR resize of `padding` -- is pinned to the documented rules (round half to even; the rule
of csrc/resize_u8.h), not checked against cv2 itself.
"""
from __future__ import annotations

import os
from typing import List, Optional

import numpy as np
import torch

from . import matio, pngio, synth

EPS = 2.2204e-16                       # utils_data.py:7


def _load_maps(path: str) -> np.ndarray:
    if path.endswith(".npz"):
        return np.load(path)["PriorMaps"].astype(np.float32)
    return matio.loadmat(path)["PriorMaps"].astype(np.float32)


def resize_linear(img: np.ndarray, out_h: int, out_w: int) -> np.ndarray:
    """cv2.resize(img, (out_w, out_h)) for a 2-D float32 map with the default INTER_LINEAR: half-pixel centres
    (`src = (dst + 0.5) * (src_size / dst_size) - 0.5`, computed in double, cast to float), edge samples replicated,
    horizontal pass then vertical pass in fp32."""
    h, w = img.shape
    img = np.asarray(img, dtype=np.float32)

    def taps(n_out, n_in):
        f = ((np.arange(n_out, dtype=np.float64) + 0.5) * (float(n_in) / float(n_out)) - 0.5).astype(np.float32)
        i0 = np.floor(f).astype(np.int64)
        f = (f - i0.astype(np.float32)).astype(np.float32)
        f[i0 < 0] = 0.0
        i0[i0 < 0] = 0
        f[i0 >= n_in - 1] = 0.0
        i0[i0 >= n_in - 1] = n_in - 1
        return i0, np.minimum(i0 + 1, n_in - 1), f

    x0, x1, fx = taps(out_w, w)
    y0, y1, fy = taps(out_h, h)
    rows = (img[:, x0] * (np.float32(1) - fx)[None, :]).astype(np.float32) + (img[:, x1] * fx[None, :]).astype(np.float32)
    out = (rows[y0] * (np.float32(1) - fy)[:, None]).astype(np.float32) + (rows[y1] * fy[:, None]).astype(np.float32)
    return out.astype(np.float32)


def letterbox(img: np.ndarray, shape_r: int, shape_c: int, quirk: bool = True) -> np.ndarray:
    """`padding(img, shape_r, shape_c, 1)` of the reference (utils_data.py:321-343) for one 2-D map: resize to the
    largest size of the source's aspect ratio that fits `shape_r x shape_c` (integer floor, as the reference computes
    it) and paste it centred into zeros.  `quirk=True`: the destination is uint8, as in the reference -- the float
    values are truncated toward zero on assignment; `quirk=False`: a float32 destination."""
    out = np.zeros((shape_r, shape_c), dtype=np.uint8 if quirk else np.float32)
    r0, c0 = img.shape
    if r0 / shape_r > c0 / shape_c:
        new_cols = min((c0 * shape_r) // r0, shape_c)
        rs = resize_linear(img, shape_r, (c0 * shape_r) // r0)[:, :new_cols]
        x = (shape_c - new_cols) // 2
        out[:, x:x + new_cols] = rs          # (uint8 destination: C cast, i.e. truncation)
    else:
        new_rows = min((r0 * shape_c) // c0, shape_r)
        rs = resize_linear(img, (r0 * shape_c) // c0, shape_c)[:new_rows]
        y = (shape_r - new_rows) // 2
        out[y:y + new_rows, :] = rs
    return out


def _fit(ims: np.ndarray, shape_r: int, shape_c: int, quirk: bool) -> np.ndarray:
    """utils_data.py:460-464 / 595-599: maps stored at another size are letterboxed channel by channel."""
    if ims.shape[0] == shape_r and ims.shape[1] == shape_c:
        return ims
    out = np.zeros((shape_r, shape_c, ims.shape[2]), dtype=np.uint8 if quirk else np.float32)
    for i in range(ims.shape[2]):
        out[:, :, i] = letterbox(ims[:, :, i], shape_r, shape_c, quirk)
    return out


def get_guasspriors(b_s: int = 2, shape_r: int = 45, shape_c: int = 80, channels: int = 8,
                    path: Optional[str] = None, quirk: bool = True) -> np.ndarray:
    """`[b_s, shape_r, shape_c, channels]` (utils_data.py:449-469): float32, or uint8 {0,1} when the file's maps had to
    be resized and `quirk` is set (the reference's behaviour).  Without a file: the closed form at the requested size
    (what the reference computes -- and saves -- when `gauss_priors.mat` does not exist yet)."""
    if path and os.path.exists(path):
        ims = _fit(_load_maps(path), shape_r, shape_c, quirk)
    else:
        ims = synth.gauss_priors(1, shape_r, shape_c, channels)[0].transpose(1, 2, 0)
    return np.repeat(ims[None], b_s, axis=0)


def _taps_u8(n_out: int, n_in: int):
    """first tap, second tap and the two 11-bit weights of cv2.resize's 8-bit INTER_LINEAR rule (csrc/resize_u8.h: lb_tap)"""
    f = ((np.arange(n_out, dtype=np.float64) + 0.5) * (float(n_in) / float(n_out)) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    f[s < 0] = 0.0
    s[s < 0] = 0
    f[s >= n_in - 1] = 0.0
    s[s >= n_in - 1] = n_in - 1
    c1 = np.rint((f * np.float32(2048.0)).astype(np.float32)).astype(np.int64)
    c0 = np.rint(((np.float32(1.0) - f).astype(np.float32) * np.float32(2048.0)).astype(np.float32)).astype(np.int64)
    return s, np.minimum(s + 1, n_in - 1), c0, c1


def letterbox_u8(img: np.ndarray, shape_r: int, shape_c: int) -> np.ndarray:
    """`padding(img, shape_r, shape_c, 1)` (utils_data.py:321-343) of a 2-d uint8 picture: cv2.resize's 8-bit INTER_LINEAR
    rule in integers (csrc/resize_u8.h: lb_tap / lb_mix) to the largest size of the source's aspect ratio that fits, pasted
    centred between zero bars."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 2:
        raise ValueError("letterbox_u8: expected a 2-d uint8 picture, got %s %r" % (img.dtype, img.shape))
    h0, w0 = img.shape
    if h0 / shape_r > w0 / shape_c:
        new_r, new_c = shape_r, (w0 * shape_r) // h0
    else:
        new_r, new_c = (h0 * shape_c) // w0, shape_c
    if new_r <= 0 or new_c <= 0:
        raise ValueError("a %dx%d picture has no area inside %dx%d" % (h0, w0, shape_r, shape_c))
    sy, sy1, b0, b1 = _taps_u8(new_r, h0)
    sx, sx1, a0, a1 = _taps_u8(new_c, w0)
    src = img.astype(np.int64)
    top, bot = src[sy], src[sy1]
    t0 = top[:, sx] * a0 + top[:, sx1] * a1
    t1 = bot[:, sx] * a0 + bot[:, sx1] * a1
    v = ((b0[:, None] * (t0 >> 4)) >> 16) + ((b1[:, None] * (t1 >> 4)) >> 16)
    out = np.zeros((shape_r, shape_c), dtype=np.uint8)
    y0, x0 = (shape_r - new_r) // 2, (shape_c - new_c) // 2
    out[y0:y0 + new_r, x0:x0 + new_c] = np.minimum((v + 2) >> 2, 255)
    return out


def _fhw_view(fix_map, layout):
    """`fix_map` (numpy array or tensor) as a `[F,H0,W0]` view: `[H0,W0,1,F]`, `[F,H0,W0]` or `[H0,W0,F]` (layout="HWF")"""
    if fix_map.dtype not in (np.uint8, torch.uint8):
        raise ValueError("fix_map must be uint8, got %s" % (fix_map.dtype,))
    nd = fix_map.dim() if torch.is_tensor(fix_map) else fix_map.ndim
    perm = (lambda a, p: a.permute(*p)) if torch.is_tensor(fix_map) else (lambda a, p: a.transpose(*p))
    if nd == 4:
        if fix_map.shape[2] != 1:
            raise ValueError("a 4-d fix_map is the .mat layout [H0,W0,1,F], got %r" % (tuple(fix_map.shape),))
        return perm(fix_map[:, :, 0, :], (2, 0, 1))
    if nd != 3 or layout not in (None, "FHW", "HWF"):
        raise ValueError("fix_map must be [F,H0,W0], [H0,W0,F] (layout='HWF') or [H0,W0,1,F]")
    return perm(fix_map, (2, 0, 1)) if layout == "HWF" else fix_map


def quantise_mean(total: np.ndarray, n: int) -> np.ndarray:
    """the uint8 picture the reference writes as `<video>.png` from the per-pixel integer sums of `n` frames
    (utils_data.py:517-520): the mean and the min-max scaling in float64 exactly as written there, then what `cv2.imwrite`
    does to a float64 picture (saturate_cast: round half to even)."""
    priormap = total.astype(np.float64) / n                # np.mean: an exact float64 sum divided by the count
    n_priormap = 255 * (priormap - np.min(priormap)) / (np.max(priormap) - np.min(priormap) + EPS)
    return np.clip(np.rint(n_priormap), 0, 255).astype(np.uint8)


def mean_prior_map(fix_map, h: int, w: int, frames=float("inf"), chunk_frames: int = 64, device="cuda",
                   with_image: bool = False, layout: Optional[str] = None):
    """One video's prior map: uint8 numpy `[h,w]` = `padding(png, h, w, 1)` of the picture `get_meanmaps` writes for the
    first `min(frames, F)` frames of `fix_map` (utils_data.py:516-520, 571-574); `(map, png [H0,W0])` with `with_image`.
    `fix_map`: a uint8 numpy array or tensor `[H0,W0,1,F]` (what `matio.loadmat` yields), `[F,H0,W0]`, or `[H0,W0,F]` with
    `layout="HWF"`.  Host data goes up `chunk_frames` frames at a time through two pinned buffers, so a video never has to
    fit on the device; data already there is read in place.  `device="cpu"`: the same bytes from numpy."""
    m = _fhw_view(fix_map, layout)
    F, h0, w0 = m.shape
    num = int(min(frames, F))
    if num <= 0 or h0 <= 0 or w0 <= 0:
        raise ValueError("mean_prior_map: no frames to average (fix_map %r, frames=%r)" % (tuple(fix_map.shape), frames))
    dev = torch.device(device)
    if dev.type == "cpu":
        a = m.cpu().numpy() if torch.is_tensor(m) else m
        total = np.zeros((h0, w0), dtype=np.int64)
        for f0 in range(0, num, 256):                      # integer sums: exact, whatever the order
            total += a[f0:min(f0 + 256, num)].sum(axis=0, dtype=np.int64)
        image = quantise_mean(total, num)
        out = letterbox_u8(image, h, w)
        return (out, image) if with_image else out
    from . import ops
    if torch.is_tensor(m) and m.is_cuda:
        acc = ops.fixmap_accumulate(m[:num])
    else:
        # host data: frames copied in memory order (no transposition on the host) into pinned chunks, uploaded behind the
        # kernel that sums the previous one
        a = m.numpy() if torch.is_tensor(m) else m
        matlab_order = a.strides[1] == 1 and a.strides[2] == h0 and a.strides[0] == h0 * w0
        if matlab_order:
            a = a.transpose(0, 2, 1)                       # [F,W0,H0], C-contiguous
        chunk = max(1, min(int(chunk_frames), num))
        pinned = [torch.empty((chunk,) + a.shape[1:], dtype=torch.uint8).pin_memory() for _ in range(2)]
        staged = [torch.empty((chunk,) + a.shape[1:], dtype=torch.uint8, device=dev) for _ in range(2)]
        done = [None, None]
        acc = None
        with torch.cuda.device(dev):
            for i, f0 in enumerate(range(0, num, chunk)):
                n = min(chunk, num - f0)
                b = i & 1
                if done[b] is not None:
                    done[b].synchronize()                  # the upload that read this pinned buffer is over
                np.copyto(pinned[b].numpy()[:n], a[f0:f0 + n])
                staged[b][:n].copy_(pinned[b][:n], non_blocking=True)
                done[b] = torch.cuda.Event()
                done[b].record()
                view = staged[b][:n].permute(0, 2, 1) if matlab_order else staged[b][:n]
                acc = ops.fixmap_accumulate(view, acc)
    res = ops.prior_map_from_sum(acc, num, h, w, with_image)
    if with_image:
        return res[0].cpu().numpy(), res[1].cpu().numpy()
    return res.cpu().numpy()


def _prior_list(datapath: str, phase_gen: str) -> List[str]:
    """`read_ob_prior_list` (utils_data.py:522-550): priors/<name>.png for the names of txt/train.txt (and val.txt), sorted"""
    if phase_gen not in ("train", "train_val"):
        raise NotImplementedError(phase_gen)
    lines = []
    for name in ("train.txt", "val.txt")[:1 if phase_gen == "train" else 2]:
        with open(os.path.join(datapath, "txt", name)) as f:
            lines += f.readlines()
    return sorted(os.path.join(datapath, "priors", t.strip("\n") + ".png") for t in lines)


def fold_prior_maps(maps: np.ndarray, n_priors: int, channels: int = 20) -> np.ndarray:
    """utils_data.py:576-584 on the uint8 `[shape_r, shape_c, max(channels, n_priors)]` stack of the videos' maps: more
    videos than channels are averaged in groups of `count = n_priors // channels` (float64 means), the last channel being
    the mean of every video from `channels * count - count` on; then float32 / 255."""
    if channels < n_priors:
        count = n_priors // channels
        frames = channels * count
        tmp = np.mean(maps[:, :, frames - count:], axis=2)
        maps = maps[:, :, :frames].reshape((maps.shape[0], maps.shape[1], channels, count))
        maps = np.mean(maps, axis=3)
        maps[:, :, -1] = tmp
    return maps.astype(np.float32) / 255


def build_ob_priors(datapath: str, out_path: Optional[str], phase_gen: str = "train", shape_r: int = 45, shape_c: int = 80,
                    channels: int = 20, device="cuda", write_png: bool = True, save_frames=float("inf")) -> np.ndarray:
    """The observed priors of a dataset, as `read_ob_priors` builds them when the file does not exist (utils_data.py:563-585):
    float32 `[shape_r, shape_c, max(channels, videos) folded to channels]`, written as `{'PriorMaps': maps}` to `out_path`
    (None: not written).  `datapath/txt/train.txt` (+ `val.txt` for "train_val") names the videos, `datapath/priors/<name>.png`
    is each video's picture: one that exists is read, one that does not is computed from `datapath/maps/<name>_fixMaps.mat`
    (`mean_prior_map` on `device`) and, with `write_png`, written -- the state the reference leaves after its first run."""
    priors = _prior_list(datapath, phase_gen)
    if not priors:
        raise ValueError("no videos listed under %s" % os.path.join(datapath, "txt"))
    maps = np.zeros((shape_r, shape_c, max(channels, len(priors))), np.uint8)
    for i, path in enumerate(priors):
        if os.path.exists(path):
            maps[:, :, i] = letterbox_u8(pngio.read_gray(path), shape_r, shape_c)
            continue
        name = os.path.basename(path)[:-4]
        fix = matio.loadmat(os.path.join(datapath, "maps", name + "_fixMaps.mat"))["fixMap"]
        maps[:, :, i], image = mean_prior_map(fix, shape_r, shape_c, frames=save_frames, device=device, with_image=True)
        if write_png:
            os.makedirs(os.path.dirname(path), exist_ok=True)
            pngio.write_gray(path, image)
    out = fold_prior_maps(maps, len(priors), channels)
    if out_path:
        matio.savemat(out_path, {"PriorMaps": out})
    return out


def ob_priors_file(DataSet: str, phase_gen: str = "train", priors_dir: str = "") -> str:
    """the reference's file name (utils_data.py:556-561)"""
    if phase_gen not in ("train", "train_val"):
        raise NotImplementedError(phase_gen)
    return os.path.join(priors_dir, DataSet.upper() + "_ob_priors_" + phase_gen + ".mat")


def read_ob_priors(datapath: str, DataSet: str = "", phase_gen: str = "train", shape_r: int = 45, shape_c: int = 80,
                   channels: int = 20, priors_dir: str = "", device="cuda") -> np.ndarray:
    """`read_ob_priors` of the reference (utils_data.py:552-589): `<DATASET>_ob_priors_train[_val].mat` under `priors_dir`
    (the reference: the working directory) is loaded when it exists -- the dataset is not touched then -- and built from
    `datapath` by `build_ob_priors` and written when it does not."""
    path = ob_priors_file(DataSet, phase_gen, priors_dir)
    if os.path.exists(path):
        return matio.loadmat(path)["PriorMaps"]
    return build_ob_priors(datapath, path, phase_gen, shape_r, shape_c, channels, device=device)


def get_ob_priors(path: str, b_s: int = 2, shape_r: int = 45, shape_c: int = 80, quirk: bool = True,
                  datapath: Optional[str] = None, dataset: Optional[str] = None, device="cuda") -> np.ndarray:
    """`[b_s, shape_r, shape_c, 20]` from `<DATASET>_ob_priors_train.mat` (utils_data.py:591-604); resized maps as in
    `get_guasspriors`.  A missing file is an error -- unless `datapath` and `dataset` name the dataset to build it from
    (`build_ob_priors` at `shape_r x shape_c`, written to `path`), which is what the reference does."""
    if not os.path.exists(path):
        if datapath is None or dataset is None:
            raise ValueError("observed-prior file not found: %s" % path)
        build_ob_priors(datapath, path, "train_val" if path.endswith("_train_val.mat") else "train", shape_r, shape_c,
                        device=device)
    ims = _fit(_load_maps(path), shape_r, shape_c, quirk)
    return np.repeat(ims[None], b_s, axis=0)


def get_bias(bias_type=(1, 1, 1), batch_size: int = 2, shape_r: int = 45, shape_c: int = 80,
             ob_prior_path: Optional[str] = None, gauss_prior_path: Optional[str] = None,
             device="cuda", quirk: bool = True, broadcast: bool = True,
             datapath: Optional[str] = None, dataset: Optional[str] = None) -> List[torch.Tensor]:
    """`[x_cb_gauss [n,8,h,w], x_cb_ob [n,20,h,w]]` float32 on `device` (Demo_Test.py:14-27).  `quirk`: see the module
    docstring (resized priors become {0,1} maps in the reference; False keeps the bilinear floats).
    `broadcast` (default): the n frames are a zero-stride view of ONE map set on the device -- the same values as the
    reference's `np.repeat` (utils_data.py:466-467, 601-602) without n copies, and `UAVSal.forward` recognises the view and
    runs its prior nets once (model.dedupe_priors); False materialises the n copies as the reference does.
    `datapath` / `dataset`: the dataset tree to build a missing `ob_prior_path` from (`get_ob_priors`); `ob_prior_path`
    defaults to the reference's `<DATASET>_ob_priors_train.mat` in the working directory then."""
    def frames(maps_hwc):
        t = torch.from_numpy(np.ascontiguousarray(maps_hwc.transpose(2, 0, 1))).float().to(device)[None]
        return t.expand(batch_size, -1, -1, -1) if broadcast else t.repeat(batch_size, 1, 1, 1)
    if bias_type[0]:
        g = frames(get_guasspriors(1, shape_r, shape_c, 8, gauss_prior_path, quirk)[0])
    else:
        g = torch.tensor([]).float().to(device)
    if bias_type[1]:
        if ob_prior_path is None and datapath is not None and dataset is not None:
            ob_prior_path = ob_priors_file(dataset)
        if ob_prior_path is None:
            raise ValueError("ob_prior_path (e.g. UAV2_ob_priors_train.mat) is required when bias_type[1] is set")
        o = frames(get_ob_priors(ob_prior_path, 1, shape_r, shape_c, quirk, datapath, dataset, device)[0])
    else:
        o = torch.tensor([]).float().to(device)
    return [g, o]
