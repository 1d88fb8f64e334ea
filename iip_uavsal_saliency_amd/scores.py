"""Saliency scores on the device: the metrics and the per-video loop of the reference's scorer
(utils_score_torch.py:17, 53-229, 302-365, 473-582) over `libuavsal_hip` kernels (csrc/score.hip).

`metrics` is a drop-in for the reference's dict of metric functions (same names, call signatures and [B,1] float32
results); `evalscores_vid` is its `evalscores_vid_torch` loop over the same directory layout; `score_frames` scores
device tensors directly (e.g. `stream.predict_video`'s uint8 output, no file round trip); `mean_scores` is the rule of
`Tools/Vid_MeanScore.m`.

Random draws stay on the host, in the reference's order, so that under the same `np.random.seed` /
`torch.manual_seed` the scores are the reference's: within a video, key order, then batch order, then frame order;
AUC-shuffled draws `B` shuffle maps per batch (`getshufmap`), then per frame `randint(0, n_ind, [n_ind, 100])`;
AUC-Borji draws `randint(0, N, [n_fix, 100])` per frame; AUC-Judd draws one `torch.rand([B,1,H,W])` per batch on the
CPU generator.  A frame whose AUC is NaN (`not any(S > 0)` or no fixation) draws nothing.  See DESIGN.md "Scoring".
"""
from __future__ import annotations

import ctypes as C
import os
import time
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from . import matio

EPS = 2.2204e-16                                                     # utils_score_torch.py:13
KEYS_ORDER = ['AUC_shuffled', 'NSS', 'AUC_Judd', 'AUC_Borji', 'KLD', 'SIM', 'CC']   # :17
N_REP = L.SCORE_REPS
_ID = {k: i for i, k in enumerate(KEYS_ORDER)}

# stats columns written by uavsal_score_stats (include/uavsal_hip.h)
ST_PMIN, ST_PMAX, ST_JMIN, ST_JMAX, ST_NFIX, ST_NZL = 0, 1, 2, 3, 9, 10


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _as_input(t, dev, what, allow_u8):
    """The reference's `torch.tensor(x).float()`: uint8 stays uint8 where the kernel reads it (same values), every other
    dtype becomes fp32 (a float64 fixMap is rounded to fp32 before any metric)."""
    if not isinstance(t, torch.Tensor):
        t = torch.from_numpy(np.ascontiguousarray(t))
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    if not (allow_u8 and t.dtype == torch.uint8) and t.dtype != torch.float32:
        t = t.float()
    if t.dim() != 3:
        raise ValueError("%s: expected [F, H, W], got %s" % (what, tuple(t.shape)))
    return t.to(dev).contiguous()


def _valid_auc(st) -> bool:
    """`np.any(S > 0) and np.any(F > 0)` (utils_score_torch.py:54, 87, 133): S > 0 somewhere iff max > min."""
    return st[ST_PMAX] > st[ST_PMIN] and st[ST_NFIX] > 0


def _draw_borji(st, n_pix):
    if not _valid_auc(st):
        return None
    r = np.random.randint(0, n_pix, [int(st[ST_NFIX]), N_REP])                    # :95
    return np.ascontiguousarray(r.T, dtype=np.int32)


def _draw_shuffled(st, oth):
    if not _valid_auc(st):
        return None
    n_fix = int(st[ST_NFIX])
    ind = np.nonzero(np.asarray(oth).reshape(-1))[0]                               # :141
    n_ind = len(ind)
    n_fix_oth = min(n_fix, n_ind)
    r = np.random.randint(0, n_ind, [n_ind, N_REP])[:n_fix_oth, :]                 # :145: the whole array is drawn
    return np.ascontiguousarray(ind[r].T, dtype=np.int32)


def _pack(draws, dev):
    """per-frame [REPS, n] int32 index arrays (None: no draw) -> (indices, offsets[F+1]) device tensors."""
    sizes = [0 if a is None else a.size for a in draws]
    off = np.zeros(len(draws) + 1, dtype=np.int64)
    off[1:] = np.cumsum(sizes)
    flat = np.concatenate([a.reshape(-1) for a in draws if a is not None] or [np.zeros(1, np.int32)])
    return torch.from_numpy(flat).to(dev), torch.from_numpy(off).to(dev), int(off[-1])


def host_draws(keys, host_stats, n_pix, shuffle_maps):
    """Every numpy draw of a video, in the reference's order: key, then batch, then frame.  `host_stats`: per batch the
    `[B, SCORE_NSTAT]` statistics (columns ST_PMIN, ST_PMAX, ST_NFIX are read).  Returns per batch
    `[AUC_shuffled, AUC_Borji]` lists of per-frame `[100, n]` int32 pixel indices (None: no draw)."""
    draws = [[None, None] for _ in host_stats]
    for k in keys:
        for bi, st in enumerate(host_stats):
            if k == 'AUC_shuffled':
                omaps = shuffle_maps(bi, len(st))
                draws[bi][0] = [_draw_shuffled(st[i], omaps[i]) for i in range(len(st))]
            elif k == 'AUC_Borji':
                draws[bi][1] = [_draw_borji(st[i], n_pix) for i in range(len(st))]
    return draws


class _Batch:
    """One batch of frames on the device and its descriptor."""

    def __init__(self, sal, fmap, floc, nan_rows):
        self.sal, self.fmap, self.floc = sal, fmap, floc
        self.B, H, W = sal.shape
        self.N = H * W
        self.dev = sal.device
        self.stats = torch.empty((self.B, L.SCORE_NSTAT), dtype=torch.float64, device=self.dev)
        d = L.ScoreDesc()
        d.sal, d.sal_u8 = sal.data_ptr(), int(sal.dtype == torch.uint8)
        d.fix_loc, d.loc_u8 = floc.data_ptr(), int(floc.dtype == torch.uint8)
        d.fix_map = fmap.data_ptr()
        d.n_frames, d.n_pix = self.B, self.N
        d.stats = self.stats.data_ptr()
        d.nan_rows = int(bool(nan_rows))
        self.d = d
        self.keep = []
        self._ws()

    def _ws(self):
        lib = L.load()
        nb = lib.uavsal_score_workspace_bytes(C.byref(self.d))
        if nb < 0:
            L.check(int(nb), "uavsal_score_workspace_bytes")
        self.ws = torch.empty(int(nb), dtype=torch.uint8, device=self.dev)
        self.d.ws, self.d.ws_bytes = self.ws.data_ptr(), int(nb)

    def run_stats(self, jitter=None):
        self.d.jitter = 0 if jitter is None else jitter.data_ptr()
        self.keep.append(jitter)
        L.check(L.load().uavsal_score_stats(C.byref(self.d), _stream()), "uavsal_score_stats")

    def run(self, keys, host_stats, draws):
        """Launch everything after the statistics; returns the fp32 [B, K] device tensor."""
        d = self.d
        ids = [_ID[k] for k in keys]
        if 'AUC_Judd' in keys:
            nfix = np.array([int(s[ST_NFIX]) for s in host_stats], dtype=np.int64)
            runs = (nfix + L.SCORE_RUN - 1) // L.SCORE_RUN
            fo = np.concatenate([[0], np.cumsum(nfix)]).astype(np.int64)
            ro = np.concatenate([[0], np.cumsum(runs)]).astype(np.int64)
            fo_t, ro_t = torch.from_numpy(fo).to(self.dev), torch.from_numpy(ro).to(self.dev)
            self.keep += [fo_t, ro_t]
            d.fix_off, d.run_off, d.total_fix, d.total_runs = fo_t.data_ptr(), ro_t.data_ptr(), int(fo[-1]), int(ro[-1])
            self._ws()
        for s in range(2):
            if draws[s] is None:
                d.samp[s], d.samp_off[s], d.n_samp[s] = 0, 0, 0
            else:
                idx, off, n = _pack(draws[s], self.dev)
                self.keep += [idx, off]
                d.samp[s], d.samp_off[s], d.n_samp[s] = idx.data_ptr(), off.data_ptr(), n
        out = torch.empty((self.B, len(ids)), dtype=torch.float32, device=self.dev)
        d.out, d.n_keys = out.data_ptr(), len(ids)
        for k, i in enumerate(ids):
            d.keys[k] = i
        L.check(L.load().uavsal_score_run(C.byref(d), _stream()), "uavsal_score_run")
        return out


def _score(sal, fmap, floc, keys, batch_size, shuffle_maps, jitter, nan_rows, timing=None):
    """Score device tensors `[F, H, W]` in batches; the reference's draw order (module docstring).  `shuffle_maps(bi, B)`
    returns the B host shuffle maps of batch `bi` (it may draw).  Returns the fp32 [F, K] device tensor."""
    for k in keys:
        if k not in _ID:
            raise KeyError("unknown metric %r (known: %s)" % (k, KEYS_ORDER))
    if len(set(keys)) != len(keys):
        raise ValueError("keys_order repeats a metric")
    F = sal.shape[0]
    bounds = [(s, min(s + batch_size, F)) for s in range(0, F, batch_size)]
    batches = [_Batch(sal[s:e], fmap[s:e], floc[s:e], nan_rows) for s, e in bounds]
    t_host = 0.0
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ev[0].record()
    for b in batches:                               # phase A: what the draws depend on
        b.run_stats()
    ev[1].record()
    host = [b.stats.cpu().numpy() for b in batches]
    t0 = time.perf_counter()
    draws = host_draws(keys, host, sal.shape[1] * sal.shape[2], shuffle_maps)
    t_host += time.perf_counter() - t0
    outs = []
    H, W = sal.shape[1:]
    dev_ms = ev[0].elapsed_time(ev[1]) if timing is not None else 0.0     # the copies above waited for ev[1]
    for bi, b in enumerate(batches):                # phase B
        jit = None
        if 'AUC_Judd' in keys and jitter:
            t0 = time.perf_counter()
            jit = (torch.rand([b.B, 1, H, W]) * 1e-7).to(b.dev)      # utils_score_torch.py:72
            t_host += time.perf_counter() - t0
        ev[2].record()
        b.run_stats(jit)                            # again, with the jittered map's min / max for AUC-Judd
        outs.append(b.run(keys, host[bi], draws[bi]))
        ev[3].record()
        if timing is not None:
            torch.cuda.synchronize()
            dev_ms += ev[2].elapsed_time(ev[3])
    out = torch.cat(outs, 0) if len(outs) > 1 else outs[0]
    if timing is not None:
        torch.cuda.synchronize()
        timing["host_draw_s"] = timing.get("host_draw_s", 0.0) + t_host
        timing["device_ms"] = timing.get("device_ms", 0.0) + dev_ms
    return out


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("scores: the metrics run on the GPU (libuavsal_hip); no device is visible")
    return torch.device("cuda", torch.cuda.current_device())


def _check_sizes(sal, fmap, floc):
    if tuple(sal.shape[1:]) != tuple(fmap.shape[1:]) or tuple(floc.shape[1:]) != tuple(fmap.shape[1:]):
        raise ValueError("saliency map size %s differs from the fixation size %s / %s: the reference resizes with "
                         "cv2.resize here (utils_score_torch.py:537-542), which is not reproduced"
                         % (tuple(sal.shape[1:]), tuple(fmap.shape[1:]), tuple(floc.shape[1:])))
    if sal.shape[0] != fmap.shape[0] or floc.shape[0] != fmap.shape[0]:
        raise ValueError("frame counts differ: %d / %d / %d" % (sal.shape[0], fmap.shape[0], floc.shape[0]))


def score_frames(sal, fix_map, fix_pts, keys_order: Sequence[str] = KEYS_ORDER, all_fix_points=None,
                 batch_size: int = 64, timing: Optional[dict] = None) -> np.ndarray:
    """Score `F` frames: `sal` `[F,H,W]` uint8 or float, `fix_map` (fixMap) and `fix_pts` (fixLoc) `[F,H,W]`, device
    or host tensors / arrays.  Returns the float64 `[F, len(keys_order)]` array of the reference's `iscores`
    (utils_score_torch.py:544-571), NaN rows included.  AUC_shuffled needs `all_fix_points` (see `all_fix_points`).
    `timing` (optional dict): accumulates `host_draw_s` and `device_ms`."""
    keys = list(keys_order)
    sal = sal if isinstance(sal, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(sal))
    fix_map = fix_map if isinstance(fix_map, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(fix_map))
    fix_pts = fix_pts if isinstance(fix_pts, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(fix_pts))
    _check_sizes(sal, fix_map, fix_pts)
    if 'AUC_shuffled' in keys and all_fix_points is None:
        raise ValueError("AUC_shuffled needs all_fix_points")
    dev = _device()
    s = _as_input(sal, dev, "sal", True)
    fm = _as_input(fix_map, dev, "fix_map", False)
    fl = _as_input(fix_pts, dev, "fix_pts", True)
    size = tuple(s.shape[1:])

    def shuffle_maps(bi, B):                         # :551-553
        return [shuffle_map(all_fix_points, size) for _ in range(B)]

    with torch.cuda.device(dev):
        out = _score(s, fm, fl, keys, int(batch_size), shuffle_maps, True, True, timing)
        return out.cpu().numpy().astype(np.float64)


# ------------------------------------------------------------------------------------------------ drop-in metrics

def _split(y_pred, y_true):
    if y_pred.dim() != 4 or y_pred.shape[1] != 1 or y_true.dim() != 4 or y_true.shape[1] != 2:
        raise ValueError("expected y_pred [B,1,H,W] and y_true [B,2,H,W], got %s and %s"
                         % (tuple(y_pred.shape), tuple(y_true.shape)))
    return None, y_pred[:, 0], y_true[:, 0], y_true[:, 1]


def _metric(key, y_pred, y_true, shuff_map=None, jitter=True):
    _, p, fmv, flv = _split(y_pred, y_true)
    _check_sizes(p, fmv, flv)
    dev = _device()
    s = _as_input(p, dev, "y_pred", True)
    fm = _as_input(fmv, dev, "y_true[:,0]", False)
    fl = _as_input(flv, dev, "y_true[:,1]", True)
    B = s.shape[0]
    oth = None
    if shuff_map is not None:
        o = shuff_map.detach().float().cpu().numpy() if isinstance(shuff_map, torch.Tensor) else np.asarray(shuff_map)
        oth = o.reshape(o.shape[0], -1)

    def shuffle_maps(bi, n):
        return [oth[i] for i in range(n)]

    with torch.cuda.device(dev):
        out = _score(s, fm, fl, [key], B, shuffle_maps, jitter, False)
    return out.to(y_pred.device)


def metric_auc_s(y_pred, y_true, shuff_map):
    return _metric('AUC_shuffled', y_pred, y_true, shuff_map)


def metric_auc_j(y_pred, y_true, jitter=1):
    return _metric('AUC_Judd', y_pred, y_true, jitter=bool(jitter))


def metric_auc_b(y_pred, y_true):
    return _metric('AUC_Borji', y_pred, y_true)


def metric_kl(y_pred, y_true):
    return _metric('KLD', y_pred, y_true)


def metric_cc(y_pred, y_true):
    return _metric('CC', y_pred, y_true)


def metric_nss(y_pred, y_true):
    return _metric('NSS', y_pred, y_true)


def metric_sim(y_pred, y_true):
    return _metric('SIM', y_pred, y_true)


metrics = {                                                          # utils_score_torch.py:221-229
    "AUC_shuffled": metric_auc_s,
    "AUC_Judd": metric_auc_j,
    "AUC_Borji": metric_auc_b,
    "NSS": metric_nss,
    "CC": metric_cc,
    "SIM": metric_sim,
    "KLD": metric_kl,
}


# ------------------------------------------------------------------------------------------------ host helpers

def all_fix_points(fixs_dir: str, dataset: str = 'DIEM20', maxframes=float('inf')) -> List[np.ndarray]:
    """`getALLFix_vid` (utils_score_torch.py:302-331): per frame of every `*_fixPts.mat` (sorted names), the fixation
    coordinates `[n, 2]` as fractions of the frame size (row / H, column / W)."""
    names = sorted(f for f in os.listdir(fixs_dir) if f.endswith('.mat'))
    num = len(names)
    dataset = dataset.upper()
    if dataset == 'CITIUS':
        num = 45
    if dataset == 'DIEM20':
        maxframes = 300
    pts = []
    for i in range(num):
        fixpts = matio.loadmat(os.path.join(fixs_dir, names[i]))["fixLoc"]
        use = min(maxframes, fixpts.shape[3])
        fixpts = fixpts[:, :, :, :use]
        for j in range(use):
            fx, fy = np.where(fixpts[:, :, 0, j])
            fx = fx / fixpts.shape[0]
            fy = fy / fixpts.shape[1]
            pts.append(np.concatenate((np.expand_dims(fx, 1), np.expand_dims(fy, 1)), 1))
    return pts


def shuffle_map(all_fix_points: Sequence[np.ndarray], size=(480, 640), nframes: int = 10) -> np.ndarray:
    """`getshufmap` (utils_score_torch.py:334-355): the uint8 map of the fixations of `nframes` frames drawn with
    `np.random.randint`, scaled to `size`, rounded half to even, truncated to int and bounded by `size`."""
    nframes = min(nframes, len(all_fix_points))
    idx = np.random.randint(0, len(all_fix_points), int(nframes))
    fix_nf = all_fix_points[idx[0]]
    for i in range(1, nframes):
        fix_nf = np.concatenate((fix_nf, all_fix_points[idx[i]]), 0)
    fix_nf[:, 0] *= size[0]          # in place, as the reference (a single drawn frame scales the list's own array)
    fix_nf[:, 1] *= size[1]
    fix_nf = np.round(fix_nf).astype(int)
    bound = (fix_nf[:, 0] < size[0]) * (fix_nf[:, 1] < size[1])
    fix_nf = fix_nf[bound]
    out = np.zeros(size, dtype=np.uint8)
    out[fix_nf[:, 0], fix_nf[:, 1]] = 1
    return out


def _load_all_fix_points(path: str):
    a = np.load(path, allow_pickle=True)
    return [np.array(x, dtype=np.float64) for x in a] if a.dtype == object else [x for x in a]


def _save_all_fix_points(path: str, pts) -> None:
    a = np.empty(len(pts), dtype=object)          # explicit object array: np.save of a ragged list fails on NumPy >= 1.24
    for i, p in enumerate(pts):
        a[i] = p
    np.save(path, a, allow_pickle=True)


def evalscores_vid(root_dir: str, sal_dir: str, dataset: str, method_names: Sequence[str],
                   keys_order: Sequence[str] = KEYS_ORDER, batch_size: int = 64) -> None:
    """`evalscores_vid_torch` (utils_score_torch.py:473-582): for every method and video, score
    `<sal_dir>/Saliency/<method>/<name>.mat` (salmap) against `<root_dir>/maps/<name>_fixMaps.mat` (fixMap) and
    `<root_dir>/fixations/maps/<name>_fixPts.mat` (fixLoc) over `nframes = min` of the three, and write
    `<sal_dir>/Scores/<method>/Score_<name>.mat` (`iscore`, float64 `[nframes, K]`).  Videos whose score file exists are
    skipped.  `ALLFixPts_<DATASET>.npy` under `root_dir` caches the AUC-shuffled fixation list."""
    keys = list(keys_order)
    maps_dir = os.path.join(root_dir, 'maps')
    fixs_dir = os.path.join(root_dir, 'fixations', 'maps')
    sals_dir = os.path.join(sal_dir, 'Saliency')
    score_dir = os.path.join(sal_dir, 'Scores')
    os.makedirs(score_dir, exist_ok=True)
    pts = None
    if 'AUC_shuffled' in keys:
        path = os.path.join(root_dir, 'ALLFixPts_' + dataset.upper() + '.npy')
        if not os.path.exists(path):
            pts = all_fix_points(fixs_dir, dataset)
            _save_all_fix_points(path, pts)
        else:
            pts = _load_all_fix_points(path)
    for method in method_names:
        if os.path.exists(os.path.join(score_dir, 'Score_' + method + '.mat')):
            continue
        iscore_dir = os.path.join(score_dir, method)
        os.makedirs(iscore_dir, exist_ok=True)
        salmap_dir = os.path.join(sals_dir, method)
        for fname in sorted(f for f in os.listdir(salmap_dir) if f.endswith('.mat')):
            name = fname[:-4]
            iscore_path = os.path.join(iscore_dir, 'Score_' + name + '.mat')
            if os.path.exists(iscore_path):
                continue
            salmap = matio.loadmat(os.path.join(salmap_dir, fname))["salmap"]
            fixmap = matio.loadmat(os.path.join(maps_dir, name + '_fixMaps.mat'))["fixMap"]
            fixpts = matio.loadmat(os.path.join(fixs_dir, name + '_fixPts.mat'))["fixLoc"]
            nframes = min(salmap.shape[3], min(fixpts.shape[3], fixmap.shape[3]))
            if salmap.shape[:2] != fixmap.shape[:2]:
                raise ValueError("%s: salmap size %s differs from the fixation size %s (the reference's cv2.resize "
                                 "branch is not reproduced)" % (name, salmap.shape[:2], fixmap.shape[:2]))
            sal = torch.from_numpy(np.ascontiguousarray(salmap[:, :, 0, :nframes].transpose(2, 0, 1)))
            fm = torch.from_numpy(np.ascontiguousarray(fixmap[:, :, 0, :nframes].transpose(2, 0, 1)))
            fl = torch.from_numpy(np.ascontiguousarray(fixpts[:, :, 0, :nframes].transpose(2, 0, 1)))
            if fl.dtype not in (torch.uint8, torch.float32):
                fl = fl.float()
            dev = _device()
            iscores = score_frames(sal.to(dev), fm.float().to(dev), fl.to(dev), keys, pts, batch_size)
            matio.savemat(iscore_path, {'iscore': iscores})


def mean_scores(sal_dir: str, max_videos=None) -> Dict[str, np.ndarray]:
    """`Tools/Vid_MeanScore.m`: for every method directory under `<sal_dir>/Scores/`, the rows without NaN of every
    video's `iscore`, pooled, and their column means.  Returns `{method: float64 [K]}`."""
    score_dir = os.path.join(sal_dir, 'Scores')
    out = {}
    for method in sorted(d for d in os.listdir(score_dir) if os.path.isdir(os.path.join(score_dir, d))):
        mdir = os.path.join(score_dir, method)
        files = sorted(f for f in os.listdir(mdir) if f.endswith('.mat') and not os.path.isdir(os.path.join(mdir, f)))
        if max_videos is not None:
            files = files[:max_videos]
        rows = [np.asarray(matio.loadmat(os.path.join(mdir, f))["iscore"], dtype=np.float64) for f in files]
        rows = [r[~np.isnan(r.sum(axis=1))] for r in rows]
        out[method] = np.concatenate(rows, 0).mean(axis=0) if rows else np.zeros(0)
    return out
