"""Float64 numpy restatement of the seven metrics of the reference's scorer (utils_score_torch.py:53-218), fed with the
same host-drawn sample indices and AUC-Judd jitter as the device path (`scores.host_draws`).  AUC-Judd counts
#{pixels >= S_j} with np.sort + np.searchsorted, so it is exact and fast for any number of fixations.  The normalised
map S is fp32 as in the reference (its comparisons decide the counts); everything else is float64."""
import numpy as np
import torch

from iip_uavsal_saliency_amd import scores

EPS = 2.2204e-16
N_REP = 100
_trapz = getattr(np, "trapezoid", None) or np.trapz      # the same function under NumPy 2's name


def norm_f32(y):
    y = np.asarray(y, dtype=np.float32)
    mn, mx = y.min(), y.max()
    return (y - mn) / ((mx - mn) + np.float32(EPS))


def auc_judd(pred, loc, jit=None):
    y = np.asarray(pred, dtype=np.float32)
    if jit is not None:
        y = y + np.asarray(jit, dtype=np.float32)
    S = norm_f32(y)
    F = np.asarray(loc, dtype=np.float32) > 0.5
    if not (S > 0).any() or not F.any():
        return np.nan
    N, sfix = S.size, np.sort(S[F])[::-1]
    n = sfix.size
    above = N - np.searchsorted(np.sort(S), sfix, side="left")             # #{S >= S_j}
    j = np.arange(n)
    tp = np.concatenate([[0], (j + 1).astype(np.float32) / np.float32(n), [1]]).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        fp = np.concatenate([[0], (above - j - 1).astype(np.float32) / np.float32(N - n), [1]]).astype(np.float32)
        terms = (tp[:-1] + tp[1:]) * (fp[1:] - fp[:-1])                     # fp32, as torch.trapz
    return float(np.sum(terms.astype(np.float64)) / 2.0)


def auc_sampled(pred, loc, idx):
    """AUC-Borji / AUC-shuffled (:82-117, :132-160) from the drawn pixel indices `idx` [100, n]."""
    S = norm_f32(pred)
    F = np.asarray(loc, dtype=np.float32) > 0.5
    if idx is None:
        return np.nan
    sfix = S[F]
    auc = np.zeros(N_REP)
    for rep in range(N_REP):
        sr = S[idx[rep]]
        thr = np.r_[0:np.max(np.r_[sfix, sr]):0.1][::-1]
        tp = np.zeros(len(thr) + 2)
        fp = np.zeros(len(thr) + 2)
        tp[-1] = fp[-1] = 1
        for k, t in enumerate(thr):
            tp[k + 1] = np.sum(sfix >= t) / float(sfix.size)
            fp[k + 1] = np.sum(sr >= t) / float(sr.size)
        auc[rep] = _trapz(tp, fp)
    return float(np.mean(auc))


def nss(pred, fmap, loc):
    p, l = np.asarray(pred, np.float64), np.asarray(loc, np.float32).astype(np.float64)
    return float(np.sum(l * (p - p.mean()) / (p.std(ddof=1) + EPS)) / (l.sum() + EPS))


def cc(pred, fmap, loc):
    p, t = np.asarray(pred, np.float64), np.asarray(fmap, np.float32).astype(np.float64)
    t = (t - t.mean()) / (t.std(ddof=1) + EPS)
    p = (p - p.mean()) / (p.std(ddof=1) + EPS)
    t, p = t - t.mean(), p - p.mean()
    return float(np.sum(t * p) / (np.sqrt(np.sum(p * p) * np.sum(t * t)) + EPS))


def kld(pred, fmap, loc):
    p, t = np.asarray(pred, np.float64), np.asarray(fmap, np.float32).astype(np.float64)
    t = t / (t.sum() + EPS)
    p = p / (p.sum() + EPS)
    return float(np.sum(t * np.log(t / (p + EPS) + EPS)))


def sim(pred, fmap, loc):
    p, t = np.asarray(pred, np.float64), np.asarray(fmap, np.float32).astype(np.float64)
    t = (t - t.min()) / (t.max() - t.min() + EPS)
    p = (p - p.min()) / (p.max() - p.min() + EPS)
    t = t / (t.sum() + EPS)
    p = p / (p.sum() + EPS)
    return float(np.sum(np.minimum(t, p)))


_PLAIN = {"NSS": nss, "CC": cc, "KLD": kld, "SIM": sim}


def host_stats(sal, loc):
    """the columns of uavsal_score_stats that the draws read, computed on the host."""
    B = sal.shape[0]
    st = np.zeros((B, 16))
    s = sal.reshape(B, -1).astype(np.float32)
    st[:, scores.ST_PMIN] = s.min(1)
    st[:, scores.ST_PMAX] = s.max(1)
    st[:, scores.ST_NFIX] = (loc.reshape(B, -1).astype(np.float32) > 0.5).sum(1)
    return st


def score_frames_ref(sal, fmap, loc, keys, batch_size, shuffle_maps, jitter=True, nan_rows=True):
    """`scores.score_frames` restated: the same host draws (`scores.host_draws`), the same jitter stream, float64
    metrics.  `sal`, `fmap`, `loc`: numpy `[F, H, W]`; `shuffle_maps(bi, B)` as in scores._score."""
    keys = list(keys)
    F, H, W = sal.shape
    N = H * W
    bounds = [(s, min(s + batch_size, F)) for s in range(0, F, batch_size)]
    host = [host_stats(sal[s:e], loc[s:e]) for s, e in bounds]
    draws = scores.host_draws(keys, host, N, shuffle_maps)
    out = np.zeros((F, len(keys)))
    for bi, (s, e) in enumerate(bounds):
        jit = None
        if "AUC_Judd" in keys and jitter:
            jit = (torch.rand([e - s, 1, H, W]) * 1e-7).numpy().reshape(e - s, -1)
        for i in range(e - s):
            p = sal[s + i].reshape(-1).astype(np.float32)
            fm = fmap[s + i].reshape(-1).astype(np.float32)
            lc = loc[s + i].reshape(-1).astype(np.float32)
            for k, key in enumerate(keys):
                if key == "AUC_Judd":
                    v = auc_judd(p, lc, None if jit is None else jit[i])
                elif key == "AUC_shuffled":
                    v = auc_sampled(p, lc, draws[bi][0][i])
                elif key == "AUC_Borji":
                    v = auc_sampled(p, lc, draws[bi][1][i])
                else:
                    v = _PLAIN[key](p, fm, lc)
                out[s + i, k] = np.float32(v)
            if nan_rows and (not p.any() or not fm.any() or not lc.any()):
                out[s + i] = np.nan
    return out


def metric_ref(key, sal, fmap, loc, seed, shuff=None):
    """`metrics[key]` of one batch under `np.random.seed(seed)` / `torch.manual_seed(seed)`: float64 `[B]`."""
    np.random.seed(seed)
    torch.manual_seed(seed)
    oth = None if shuff is None else np.asarray(shuff).reshape(sal.shape[0], -1)
    return score_frames_ref(sal, fmap, loc, [key], sal.shape[0], lambda bi, n: [oth[i] for i in range(n)],
                            True, False)[:, 0]
