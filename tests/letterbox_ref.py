"""Helper of the letterbox tests (not a test): the numpy restatement of the input letterboxing -- `padding()` per frame
and the channel swap of preprocess_videos (reference utils_data.py:255-287, 321-343) with cv2.resize's 8-bit INTER_LINEAR
rule in integers -- and `cases()`, known answers that need neither cv2 nor the restatement.

Pin: OpenCV is not installed where this was written and the reference holds no fixture for this step.  The rule below is
restated from OpenCV's 8-bit linear resize (half-pixel centres in double cast to float, 11-bit coefficients, horizontal
pass in integers, vertical pass with the `>> 4`, `>> 16`, `(+ 2) >> 2` shifts) and pinned by the known answers of
`cases()`, which follow from that rule and from the geometry of utils_data.py:321-343 alone, NOT by outputs of cv2.
"""
from fractions import Fraction

import numpy as np

SOURCE_SIZES = [(720, 1280), (1080, 1920), (2160, 3840), (480, 640), (1280, 720), (360, 640), (540, 960), (405, 719),
                (721, 1280), (300, 500)]
MODEL_SIZES = [(360, 640), (288, 512)]


def geometry(h0, w0, R, C):
    """(new_r, new_c, y0, x0, branch) with the reference's own expressions (utils_data.py:326-341)."""
    rows_rate = h0 / R
    cols_rate = w0 / C
    if rows_rate > cols_rate:
        new_cols = (w0 * R) // h0
        return R, new_cols, 0, (C - new_cols) // 2, "cols"
    new_rows = (h0 * C) // w0
    return new_rows, C, (R - new_rows) // 2, 0, "rows"


def taps(n_out, n_in):
    """Per output index: first tap, second tap and the two 11-bit weights."""
    scale = float(n_in) / float(n_out)
    f = ((np.arange(n_out, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    lo = s < 0
    s[lo] = 0
    f[lo] = 0.0
    hi = s >= n_in - 1
    s[hi] = n_in - 1
    f[hi] = 0.0
    s1 = np.minimum(s + 1, n_in - 1)
    c1 = np.rint((f * np.float32(2048.0)).astype(np.float32)).astype(np.int64)
    c0 = np.rint(((np.float32(1.0) - f).astype(np.float32) * np.float32(2048.0)).astype(np.float32)).astype(np.int64)
    return s, s1, c0, c1


def resize_u8(img, out_h, out_w):
    """`cv2.resize(img, (out_w, out_h))` for a uint8 image `[..., h, w, c]` (leading dimensions are a batch)."""
    h, w = img.shape[-3], img.shape[-2]
    sy, sy1, b0, b1 = taps(out_h, h)
    sx, sx1, a0, a1 = taps(out_w, w)
    a0, a1 = a0[:, None], a1[:, None]
    b0, b1 = b0[:, None, None], b1[:, None, None]
    top, bot = img[..., sy, :, :].astype(np.int64), img[..., sy1, :, :].astype(np.int64)
    t0 = top[..., sx, :] * a0 + top[..., sx1, :] * a1
    t1 = bot[..., sx, :] * a0 + bot[..., sx1, :] * a1
    v = ((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16)
    return np.clip((v + 2) >> 2, 0, 255).astype(np.uint8)


def letterbox(frames, R, C, layout="HWC", bgr=False):
    """uint8 frames `[F, h0, w0, 3]` (or `[F, 3, h0, w0]` with layout="CHW") -> `[F, 3, R, C]`."""
    frames = np.asarray(frames)
    if layout == "CHW":
        frames = frames.transpose(0, 2, 3, 1)
    F, h0, w0, _ = frames.shape
    new_r, new_c, y0, x0, _ = geometry(h0, w0, R, C)
    if new_r <= 0 or new_c <= 0:
        raise ValueError("degenerate picture")
    out = np.zeros((F, R, C, 3), dtype=np.uint8)
    for i in range(0, F, 4):                              # a few frames at a time: the intermediates are int64
        out[i:i + 4, y0:y0 + new_r, x0:x0 + new_c] = resize_u8(frames[i:i + 4], new_r, new_c)
    if bgr:
        out = out[..., ::-1]
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2))


def exact_weights(n_out, n_in):
    """The taps from rational arithmetic, for sizes where no rounding decision is close (checked): the coordinate
    (d + 1/2) * n_in / n_out - 1/2 exactly, the weights as the nearest integers to frac * 2048 and (1 - frac) * 2048."""
    out = []
    for d in range(n_out):
        x = (Fraction(2 * d + 1, 2) * Fraction(n_in, n_out)) - Fraction(1, 2)
        s = x.numerator // x.denominator
        fr = x - s
        if s < 0:
            s, fr = 0, Fraction(0)
        if s >= n_in - 1:
            s, fr = n_in - 1, Fraction(0)
        w = []
        for q in (fr * 2048, (1 - fr) * 2048):
            assert abs((q % 1) - Fraction(1, 2)) > Fraction(1, 100), "a tie: not a case for exact arithmetic"
            w.append(int(round(q)))
        out.append((s, min(s + 1, n_in - 1), w[1], w[0]))
    return out


def _one_hot_enlarged(h0, w0, R, C, ys, xs, ch, v):
    """Expected output for one source pixel of value v: only the outputs whose taps name (ys, xs) are non-zero."""
    new_r, new_c, y0, x0, _ = geometry(h0, w0, R, C)
    want = np.zeros((1, 3, R, C), dtype=np.uint8)
    rows = [(d, sum(wt for tap, wt in ((s, c0), (s1, c1)) if tap == ys))
            for d, (s, s1, c0, c1) in enumerate(exact_weights(new_r, h0))]
    cols = [(d, sum(wt for tap, wt in ((s, c0), (s1, c1)) if tap == xs))
            for d, (s, s1, c0, c1) in enumerate(exact_weights(new_c, w0))]
    for dy, b in rows:
        for dx, a in cols:
            if a and b:
                want[0, ch, y0 + dy, x0 + dx] = (((b * ((v * a) >> 4)) >> 16) + 2) >> 2
    return want


def cases():
    """(name, src uint8 [F, h0, w0, 3], R, C, bgr, want uint8 [F, 3, R, C]) known answers."""
    rng = np.random.RandomState(20)
    # same size: the identity
    a = rng.randint(0, 256, (2, 36, 64, 3)).astype(np.uint8)
    yield "identity", a, 36, 64, False, a.transpose(0, 3, 1, 2).copy()
    # the BGR swap moves planes 0 and 2
    yield "identity_bgr", a, 36, 64, True, a[..., ::-1].transpose(0, 3, 1, 2).copy()
    # exact 2x: the rounded mean of each 2x2 block
    b = rng.randint(0, 256, (2, 72, 128, 3)).astype(np.uint8)
    m = b.astype(np.int64).reshape(2, 36, 2, 64, 2, 3).sum(axis=(2, 4))
    yield "half", b, 36, 64, False, ((m + 2) >> 2).astype(np.uint8).transpose(0, 3, 1, 2).copy()
    # a constant picture stays constant, the bars are 0, their extents come from the geometry formulas
    for (h0, w0), (R, C), bars in [((48, 64), (36, 64), ("cols", 8, 8)),            # 4:3 into 16:9: pillars
                                   ((128, 72), (36, 64), ("cols", 22, 22)),          # portrait: wide pillars
                                   ((24, 64), (36, 64), ("rows", 6, 6)),             # wider than the model: rows
                                   ((405, 719), (360, 640), ("cols", 0, 1)),         # one-pixel bar on one side only
                                   ((721, 1280), (360, 640), ("cols", 0, 1)),
                                   ((300, 500), (288, 512), ("cols", 16, 16))]:
        new_r, new_c, y0, x0, branch = geometry(h0, w0, R, C)
        lead, trail = (x0, C - x0 - new_c) if branch == "cols" else (y0, R - y0 - new_r)
        assert (branch, lead, trail) == bars, (h0, w0, R, C, branch, lead, trail)
        for v in (255, 77):
            want = np.zeros((1, 3, R, C), dtype=np.uint8)
            want[:, :, y0:y0 + new_r, x0:x0 + new_c] = v
            yield "const%d_%dx%d_in_%dx%d" % (v, h0, w0, R, C), np.full((1, h0, w0, 3), v, np.uint8), R, C, False, want
    # a one-hot pixel under an exact 2x reduction lands in one output as (v + 2) >> 2
    for (ys, xs, ch, v) in [(0, 0, 0, 255), (71, 127, 2, 201), (33, 70, 1, 6), (10, 11, 1, 1)]:
        src = np.zeros((1, 72, 128, 3), dtype=np.uint8)
        src[0, ys, xs, ch] = v
        want = np.zeros((1, 3, 36, 64), dtype=np.uint8)
        want[0, ch, ys // 2, xs // 2] = (v + 2) >> 2
        yield "onehot_half_%d_%d" % (ys, xs), src, 36, 64, False, want
    # ... and under an enlargement its footprint and values follow from the 11-bit weights of the rows / columns that name it
    for (ys, xs, ch, v) in [(0, 0, 0, 255), (299, 499, 2, 255), (150, 251, 1, 200), (7, 498, 0, 131)]:
        src = np.zeros((1, 300, 500, 3), dtype=np.uint8)
        src[0, ys, xs, ch] = v
        yield "onehot_enlarged_%d_%d" % (ys, xs), src, 360, 640, False, _one_hot_enlarged(300, 500, 360, 640, ys, xs, ch, v)
