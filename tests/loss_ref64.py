"""Helper of the loss tests (not a test): the project's own float64 numpy restatement of the reference's criterion
(`loss_fu = 10 * KL - 2 * CC - NSS`, loss_functions.py:43-50, 64-86), of its gradient with respect to the prediction,
and of the gaze ground truth (`padding` / `padding_fixation`, utils_data.py:321-385), plus the synthetic inputs that the
golden generator (tools/make_loss_goldens.py) and the tests both build.

The forward follows the reference's expressions literally, in float64.  The gradient is derived by hand from the three
terms (the same algebra as csrc/loss.hip, written independently in numpy); tests/test_losses_cpu.py holds it against the
reference's own float64 autograd recorded in tests/golden/.

Pin of channel 0: OpenCV is not installed where this was written.  The map is resized with `letterbox_ref.resize_u8`, the
restatement of cv2.resize's 8-bit INTER_LINEAR rule that pins the input letterboxing too -- by known answers that follow
from the rule, NOT by outputs of cv2.  The fixation scatter (channel 1) is pure numpy in the reference and is held
bit for bit against its recorded outputs.
"""
import hashlib

import numpy as np

import letterbox_ref

EPS = 2.2204e-16
LOSS_FU, LOSS_KL = (10.0, -2.0, -1.0), (10.0, 0.0, 0.0)

# (name, h, w, B, seed): the random cases of the goldens
RANDOM_CASES = [("45x80_B20", 45, 80, 20, 11), ("90x160_B8", 90, 160, 8, 12)]
# More than 64 frames, against this restatement only (no goldens): one wave of csrc/loss.hip averages the per-frame records,
# lane i taking frames i, i + 64, ...  12x20_B65: the vector path (240 pixels), ONE frame in the second stride; 9x15_B130: the
# scalar path (135 pixels), three strides, the last one two lanes wide.  The default validation / fine-tuning group is 80 frames.
STRIDE_CASES = [("12x20_B65", 12, 20, 65, 21), ("9x15_B130", 9, 15, 130, 22)]
MEAN_LANES = 64
EDGE_SHAPE = (6, 45, 80)
EDGE_CONSTANT = {3: 0.0, 4: 0.5, 5: 1.0}          # frame -> its constant prediction
EDGE_ZERO_MAP, EDGE_SINGLE_FIX = 1, 2
# (h0, w0, h, w): both letterbox branches, the identity branch, odd sizes
SCATTER_CASES = [(180, 320, 45, 80), (360, 480, 45, 80), (101, 77, 45, 80), (180, 320, 60, 80), (360, 480, 60, 80),
                 (101, 77, 60, 80), (45, 80, 45, 80), (60, 80, 60, 80), (77, 101, 45, 80)]


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------ inputs

def random_inputs(h, w, B, seed):
    """`(y_pred [B,1,h,w] float32, y_true [B,2,h,w] float32)`: a sigmoid of hashed logits of std ~2.5, a fixation map in
    0..255 (uint8 values, as preprocess_vidmaps leaves them) and 0 / 1 fixation points."""
    from iip_uavsal_saliency_amd import synth
    logits = synth.synth_tensor("loss.pred.weight", (B, 1, h, w), seed).astype(np.float64) * np.sqrt(h * w / 2.0) * 2.5
    y_pred = (1.0 / (1.0 + np.exp(-logits))).astype(np.float32)
    loc = synth.synth_fix_points(B, h, w, 12, seed)
    fmap = np.rint(synth.synth_fix_maps(loc, 3.0) * 255.0).astype(np.uint8)
    y_true = np.stack([fmap, loc], 1).astype(np.float32)
    return y_pred, y_true


def edge_inputs():
    """The edge batch `[6, ., 45, 80]`: 0 ordinary; 1 an all-zero map and no fixation; 2 a single fixation; 3, 4, 5
    constant predictions 0, 0.5 and 1 (their fp32 mean is exact) over ordinary ground truth."""
    B, h, w = EDGE_SHAPE
    y_pred, y_true = random_inputs(h, w, B, 13)
    y_true[EDGE_ZERO_MAP] = 0
    y_true[EDGE_SINGLE_FIX, 1] = 0
    y_true[EDGE_SINGLE_FIX, 1, h // 3, w // 5] = 1
    for f, v in EDGE_CONSTANT.items():
        y_pred[f] = v
    return y_pred, y_true


def scatter_inputs(h0, w0, seed=0):
    """`(fix_map, fix_loc)` uint8 `[4, h0, w0]`: frame 0 ordinary; 1 with fixations on the last source row and column and in
    the corners; 2 empty; 3 values other than 1 (they survive only where the reference returns its input)."""
    from iip_uavsal_saliency_amd import synth
    loc = synth.synth_fix_points(4, h0, w0, 25, seed + h0 * 1000 + w0)
    loc[1, h0 - 1, :: max(1, w0 // 9)] = 1
    loc[1, :: max(1, h0 // 7), w0 - 1] = 1
    loc[1, h0 - 1, w0 - 1] = 1
    loc[1, 0, 0] = 1
    loc[2] = 0
    loc[3] *= 7
    fmap = np.rint(synth.synth_fix_maps((loc != 0).astype(np.uint8), max(2.0, h0 / 30.0)) * 255.0).astype(np.uint8)
    return fmap, loc


# ------------------------------------------------------------------------------------------------ gaze ground truth

def resize_fixation(img, rows, cols):
    """utils_data.py:345-360 without the Python loop: np.round is round-half-to-even on the float64 product."""
    out = np.zeros((rows, cols), np.uint8)
    rr, cc = np.nonzero(img)
    r = np.rint(rr * (rows / img.shape[0])).astype(np.int64)
    c = np.rint(cc * (cols / img.shape[1])).astype(np.int64)
    r[r == rows] -= 1
    c[c == cols] -= 1
    out[r, c] = 1
    return out


def padding_fixation(img, h, w):
    """utils_data.py:362-385, the identity branch (:366-367) included."""
    h0, w0 = img.shape
    if h0 == h and w0 == w:
        return img
    new_r, new_c, y0, x0, _ = letterbox_ref.geometry(h0, w0, h, w)
    out = np.zeros((h, w), np.uint8)
    out[y0:y0 + new_r, x0:x0 + new_c] = resize_fixation(img, new_r, new_c)
    return out


def padding_map(img, h, w):
    """`padding(img, h, w, 1)` (utils_data.py:321-343) with the restated 8-bit resize."""
    h0, w0 = img.shape
    new_r, new_c, y0, x0, _ = letterbox_ref.geometry(h0, w0, h, w)
    out = np.zeros((h, w), np.uint8)
    out[y0:y0 + new_r, x0:x0 + new_c] = letterbox_ref.resize_u8(img[:, :, None], new_r, new_c)[:, :, 0]
    return out


def prepare_gaze(fix_map, fix_loc, h, w):
    """`(y_gaze float32 [F,2,h,w], has_gaze bool [F,2])` from uint8 `[F,h0,w0]` maps and points."""
    F = fix_map.shape[0]
    y = np.zeros((F, 2, h, w), np.float32)
    for i in range(F):
        y[i, 0] = padding_map(fix_map[i], h, w)
        y[i, 1] = padding_fixation(fix_loc[i], h, w)
    return y, np.any(y, axis=(2, 3))


# ------------------------------------------------------------------------------------------------ criterion

def _sum(x):
    return np.sum(x, axis=(2, 3), keepdims=True)


def _mean(x):
    return np.mean(x, axis=(2, 3), keepdims=True)


def _std(x):
    return np.std(x, axis=(2, 3), keepdims=True, ddof=1)


def frame_metrics(y_pred, y_true):
    """Per-frame `(kl, cc, nss)`, float64 `[B]` each: loss_functions.py:64-86 line by line."""
    p = np.asarray(y_pred, np.float64)
    t, f = np.asarray(y_true, np.float64)[:, 0:1], np.asarray(y_true, np.float64)[:, 1:2]
    tn = t / (_sum(t) + EPS)
    pn = p / (_sum(p) + EPS)
    with np.errstate(divide="ignore", invalid="ignore"):
        kl = np.sum(tn * np.log(tn / (pn + EPS) + EPS), axis=(2, 3))[:, 0]
        ts = (t - _mean(t)) / (_std(t) + EPS)
        ps = (p - _mean(p)) / (_std(p) + EPS)
        t2, p2 = ts - _mean(ts), ps - _mean(ps)
        r1 = np.sum(t2 * p2, axis=(2, 3))
        r2 = np.sqrt(np.sum(p2 * p2, axis=(2, 3)) * np.sum(t2 * t2, axis=(2, 3)))
        cc = (r1 / (r2 + EPS))[:, 0]
        nss = (np.sum(f * ps, axis=(2, 3)) / (np.sum(f, axis=(2, 3)) + EPS))[:, 0]
    return kl, cc, nss


def loss(y_pred, y_true, weights=LOSS_FU):
    """`(metric_kl, metric_cc, metric_nss, loss)` of the batch as float64 numbers."""
    kl, cc, nss = (float(np.mean(v)) for v in frame_metrics(y_pred, y_true))
    return kl, cc, nss, weights[0] * kl + weights[1] * cc + weights[2] * nss


def loss_grad(y_pred, y_true, weights=LOSS_FU, grad_out=1.0):
    """`grad_out * d loss / d y_pred`, float64 `[B,1,h,w]`, by hand.  A term whose weight is 0 is left out.  A frame of
    constant predictions (std 0) gets NaN from the cc / nss terms, as autograd gives for the reference.  (For a frame
    with an all-zero fixation map the reference's autograd returns NaN as well -- `sqrt` at zero inside r2 -- where this
    derivative is finite: the cc term vanishes with the map.  The loop never evaluates such a frame,
    Demo_Train_Test.py:125.)"""
    p = np.asarray(y_pred, np.float64)
    t, f = np.asarray(y_true, np.float64)[:, 0:1], np.asarray(y_true, np.float64)[:, 1:2]
    B, _, h, w = p.shape
    N = h * w
    g = grad_out / B
    out = np.zeros_like(p)
    with np.errstate(divide="ignore", invalid="ignore"):
        if weights[0] != 0:
            D = _sum(p) + EPS
            tn, pn = t / (_sum(t) + EPS), p / D
            den = pn + EPS
            A = -(tn * tn) / ((tn / den + EPS) * den * den)
            out += weights[0] * (A - _sum(A * pn)) / D
        if weights[1] != 0 or weights[2] != 0:
            q, tc = p - _mean(p), t - _mean(t)
            ssp, sst = _sum(q * q), _sum(tc * tc)
            sp = np.sqrt(ssp / (N - 1))
            Y, c = sp + EPS, np.sqrt(sst / (N - 1)) + EPS
            gam = 1.0 / ((N - 1) * sp)
            if weights[1] != 0:
                X, Z = _sum(tc * q), np.sqrt(ssp * sst)
                r1, e = X / (c * Y), Z / (c * Y) + EPS
                beta = -X * gam / (c * Y * Y * e) - r1 / (e * e) * (Z / (ssp * c * Y) - Z * gam / (c * Y * Y))
                out += weights[1] * (tc / (c * Y * e) + beta * q)
            if weights[2] != 0:
                sf = _sum(f)
                out += weights[2] * ((f - sf / N) / Y - _sum(f * q) * gam * q / (Y * Y)) / (sf + EPS)
    return g * out
