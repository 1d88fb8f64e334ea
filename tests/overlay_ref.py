"""Helper of the overlay tests (not a test): the numpy float64 restatement of the reference's heat-map overlay -- the
coloured path of `visual_vid` (utils_vis.py:103-212) with `heatmap_overlay` (:34-56), `resize_fixation` (:16-31) and
`im2uint8` (:7-14), line for line -- and `cases()`, known answers that follow from the rules alone.

Pin: OpenCV is not installed where this was written.  The 8-bit resize is `letterbox_ref.resize_u8`; the float64 resize is
the half-pixel INTER_LINEAR map of `priors.resize_linear` with float32 coordinates and weights and double products; the
5x5 dilation is a box maximum clipped at the border; the colour table is data.  They are pinned by `cases()`, NOT by outputs
of cv2.  One deviation from the reference: a frame it leaves undefined (0 / 0: max(o) == 0, or max(map_color) == 0) is zeros.
"""
import numpy as np

import letterbox_ref as L

EPS = 2.2204e-16                                                       # utils_vis.py:5

GEOMETRY_SIZES = [(360, 640), (720, 1280), (1080, 1920), (2160, 3840), (1280, 720), (405, 719)]


def visual_geometry(vid_h, vid_w):
    """(mid_h, mid_w, out_h, out_w) with the reference's own expressions (utils_vis.py:168-170, 185-186)."""
    ratio = max(1, max(vid_w // 640, vid_h // 360))
    max_w, max_h = 1280, 720
    out_w = int(vid_w * min(max_w / vid_w, max_h / vid_h))
    out_h = int(vid_h * min(max_h / vid_h, max_h / vid_h))
    return vid_h // ratio, vid_w // ratio, out_h, out_w


def jet_knots():
    """The 64 knots of OpenCV's JET (MATLAB's jet(64)) per channel, as (b, g, r): u = 1/16 .. 1, fifteen ones, 1 .. 1/16,
    placed at 9..55 for green, sixteen later for red and sixteen earlier for blue, cut at the ends."""
    n = 16
    u = np.concatenate([np.arange(1, n + 1) / n, np.ones(n - 1), np.arange(n, 0, -1) / n])
    chan = []
    for shift in (-n, 0, n):                                           # b, g, r
        k = np.zeros(64)
        idx = 8 + shift + np.arange(len(u))                            # 0-based positions of u
        ok = (idx >= 0) & (idx < 64)
        k[idx[ok]] = u[ok]
        chan.append(k)
    return chan


def jet_table():
    """[256, 3] uint8 BGR: the knots interpolated linearly at 256 evenly spaced points, times 255, rounded half to even."""
    x = np.linspace(0.0, 1.0, 64)
    q = np.linspace(0.0, 1.0, 256)
    return np.stack([np.rint(np.interp(q, x, k) * 255.0) for k in jet_knots()], axis=1).astype(np.uint8)


def identity_table():
    return np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)


def random_table(seed=5):
    return np.random.RandomState(seed).randint(0, 256, (256, 3)).astype(np.uint8)


def lin_taps(n_out, n_in):
    """First tap, second tap and the float32 weight of the second tap of cv2's float INTER_LINEAR resize."""
    f = ((np.arange(n_out, dtype=np.float64) + 0.5) * (float(n_in) / float(n_out)) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    f[s < 0] = 0.0
    s[s < 0] = 0
    f[s >= n_in - 1] = 0.0
    s[s >= n_in - 1] = n_in - 1
    return s, np.minimum(s + 1, n_in - 1), f


def resize_f64(img, out_h, out_w):
    """`cv2.resize(img, (out_w, out_h))` for a float64 image [h, w, c]: horizontal pass, then vertical, in double."""
    h, w = img.shape[:2]
    x0, x1, fx = lin_taps(out_w, w)
    y0, y1, fy = lin_taps(out_h, h)
    wx0, wx1 = (np.float32(1) - fx).astype(np.float64)[None, :, None], fx.astype(np.float64)[None, :, None]
    wy0, wy1 = (np.float32(1) - fy).astype(np.float64)[:, None, None], fy.astype(np.float64)[:, None, None]
    rows = img[:, x0] * wx0 + img[:, x1] * wx1
    return rows[y0] * wy0 + rows[y1] * wy1


def resize_fixation(img, rows, cols):
    """utils_vis.py:16-31."""
    out = np.zeros((rows, cols), np.uint8)
    factor_scale_r = rows / img.shape[0]
    factor_scale_c = cols / img.shape[1]
    for coord in np.argwhere(img):
        r = int(np.round(coord[0] * factor_scale_r))
        c = int(np.round(coord[1] * factor_scale_c))
        if r == rows:
            r -= 1
        if c == cols:
            c -= 1
        out[r, c] = 1
    return out


def dilate5(mask):
    """cv2.dilate(mask, np.ones((5, 5))): the maximum over the 5x5 box around each pixel, clipped at the border."""
    h, w = mask.shape
    pad = np.zeros((h + 4, w + 4), mask.dtype)
    pad[2:-2, 2:-2] = mask
    out = np.zeros_like(mask)
    for dy in range(5):
        for dx in range(5):
            out = np.maximum(out, pad[dy:dy + h, dx:dx + w])
    return out


def heatmap_overlay(img, heatmap, lut):
    """utils_vis.py:34-56 for a uint8 BGR image and a uint8 one-channel map; `lut` stands for cv2.applyColorMap's table."""
    if img.shape[:2] != heatmap.shape[:2]:
        heatmap = L.resize_u8(heatmap[:, :, None], img.shape[0], img.shape[1])[:, :, 0]      # :39-40
    map_color = lut[heatmap]                                            # :46
    m3 = np.repeat(heatmap[:, :, None], 3, axis=2)                      # :42-43
    with np.errstate(invalid="ignore", divide="ignore"):
        img = img / (np.max(img) + EPS)                                 # :51
        m3 = m3 / (np.max(m3) + EPS)                                    # :52
        map_color = map_color / np.max(map_color)                       # :53
        return 0.8 * (1 - m3 ** 0.8) * img + m3 * map_color             # :55


def overlay_frame(frame, salmap, lut, fix=None, mid_size=None, out_size=None):
    """One frame of visual_vid's coloured path (utils_vis.py:176-209): (uint8 [out_h, out_w, 3], the double of every byte
    before clipping and rounding).  Sizes left as None: no resize (visual_img, :94-101)."""
    if mid_size is not None and tuple(mid_size) != frame.shape[:2]:
        frame = L.resize_u8(frame, mid_size[0], mid_size[1])            # :186
    o = heatmap_overlay(frame, salmap, lut)                             # :187
    if out_size is None:
        out_size = o.shape[:2]
    o = resize_f64(o, out_size[0], out_size[1])                         # :190 (the identity at equal sizes)
    if fix is not None:
        pts = dilate5(resize_fixation(fix, out_size[0], out_size[1]))   # :202-204
        o[np.repeat(pts[:, :, None], 3, axis=2) > 0.5] = 1              # :205-206
    mx = np.max(o)
    if not (mx > 0):                                                    # the deviation: 0 / 0 (or NaN) in the reference
        return np.zeros(o.shape, np.uint8), np.zeros(o.shape)
    v = o / mx * 255                                                    # :208
    return np.rint(np.clip(v, 0, 255)).astype(np.uint8), v              # :11-13


def overlay(frames, sal, lut, fix=None, mid_size=None, out_size=None, layout="HWC"):
    """Frames [F, H0, W0, 3] (or [F, 3, H0, W0]), maps [F, h, w], fix None or [F, Hf, Wf] -> (bytes, doubles) [F, out_h, out_w, 3]."""
    frames = np.asarray(frames)
    if layout == "CHW":
        frames = frames.transpose(0, 2, 3, 1)
    res = [overlay_frame(frames[i], sal[i], lut, None if fix is None else fix[i], mid_size, out_size) for i in range(len(frames))]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def excused(v, delta=1e-9):
    """Bytes whose pre-rounding double lies within `delta` of a half-integer: either neighbour is accepted there."""
    return np.abs(np.abs(v - np.floor(v)) - 0.5) <= delta


def compare(got, want_u8, v, delta=1e-9):
    """The comparison rule for output bytes.  Returns (number of wrong bytes, number of excused bytes)."""
    got = np.asarray(got).astype(np.int64)
    ex = excused(v, delta)
    ok = got == want_u8
    near = ex & ((got == np.floor(np.clip(v, 0, 255))) | (got == np.ceil(np.clip(v, 0, 255))))
    return int(np.count_nonzero(~(ok | near))), int(np.count_nonzero(ex))


def geometry_cases():
    """(vid_h, vid_w) -> (mid_h, mid_w, out_h, out_w), worked by hand from utils_vis.py:168-170, 185-186."""
    return {(360, 640): (360, 640, 720, 1280),        # ratio 1; 640 * min(2, 2) = 1280, 360 * 2 = 720
            (720, 1280): (360, 640, 720, 1280),       # ratio 2; scale 1
            (1080, 1920): (360, 640, 720, 1280),      # ratio 3; 1920 * (2 / 3): the product 1280.0 survives int()
            (2160, 3840): (360, 640, 720, 1280),      # ratio 6
            (1280, 720): (426, 240, 720, 405),        # portrait: ratio max(1, 3); 720 * 0.5625 = 405
            (405, 719): (405, 719, 720, 1278)}        # ratio 1; 719 * min(1.78.., 1.77..) = 1278.2.. -> 1278


def cases():
    """(name, kwargs of overlay(), want uint8 [F, out_h, out_w, 3]) known answers that follow from the rules alone."""
    ident = identity_table()
    # identity table, constant map 100 and constant frame 50: img = 50 / (50 + EPS) -> 1.0 - 2^-53-ish, m likewise, colour
    # 100 / 100 = 1; o = 0.8 * (1 - m^0.8) * img + m is constant, so o / max(o) * 255 = 255 everywhere
    yield ("constant", dict(frames=np.full((1, 6, 8, 3), 50, np.uint8), sal=np.full((1, 6, 8), 100, np.uint8), lut=ident),
           np.full((1, 6, 8, 3), 255, np.uint8))
    # the same through both resizes: constants stay constant under either rule
    yield ("constant_resized", dict(frames=np.full((2, 12, 16, 3), 50, np.uint8), sal=np.full((2, 5, 7), 100, np.uint8), lut=ident,
                                    mid_size=(6, 8), out_size=(9, 11)), np.full((2, 9, 11, 3), 255, np.uint8))
    # a map whose maximum is 0: m = 0, o = 0.8 * img, the byte is rint(img / max(img) * 255) whatever the table holds at 0
    # (its maximum must not be 0: the table [7, 9, 11] at 0)
    lut0 = ident.copy()
    lut0[0] = (7, 9, 11)
    fr = np.zeros((1, 4, 4, 3), np.uint8)
    fr[0, :, :, 0], fr[0, :, :, 1], fr[0, :, :, 2] = 200, 100, 40
    want = np.zeros((1, 4, 4, 3), np.uint8)
    want[..., 0], want[..., 1], want[..., 2] = 255, 128, 51             # 127.5 -> 128 (half to even), 51.0
    yield ("empty_map", dict(frames=fr, sal=np.zeros((1, 4, 4), np.uint8), lut=lut0), want)
    # an all-black frame and an empty map: 0 / 0 in the reference, zeros here (the deviation)
    yield ("black_and_empty", dict(frames=np.zeros((1, 4, 4, 3), np.uint8), sal=np.zeros((1, 4, 4), np.uint8), lut=lut0),
           np.zeros((1, 4, 4, 3), np.uint8))
    # ... with a fixation the maximum is 1: the 5x5 block is 255 and the rest 0
    fx = np.zeros((1, 8, 8), np.uint8)
    fx[0, 0, 0] = 1
    want = np.zeros((1, 8, 8, 3), np.uint8)
    want[0, :3, :3] = 255
    yield ("black_fix_corner", dict(frames=np.zeros((1, 8, 8, 3), np.uint8), sal=np.zeros((1, 8, 8), np.uint8), lut=lut0, fix=fx), want)
    # fixations under a resize of the positions, on a black frame with an empty map (so the bytes are the mask x 255):
    # 8x8 -> 20x12, factors 2.5 and 1.5.  (1, 1) -> (2.5, 1.5) -> (2, 2) half to even; (3, 3) -> (7.5, 4.5) -> (8, 4);
    # (7, 7) -> (17.5, 10.5) -> (18, 10): blocks clipped at the bottom-right; (0, 5) -> (0, 7.5) -> (0, 8): top edge
    fx = np.zeros((1, 8, 8), np.uint8)
    for r, c in ((1, 1), (3, 3), (7, 7), (0, 5)):
        fx[0, r, c] = 9
    want = np.zeros((1, 20, 12, 3), np.uint8)
    for r, c in ((2, 2), (8, 4), (18, 10), (0, 8)):
        want[0, max(r - 2, 0):r + 3, max(c - 2, 0):c + 3] = 255
    yield ("fix_half_even", dict(frames=np.zeros((1, 4, 4, 3), np.uint8), sal=np.zeros((1, 4, 4), np.uint8), lut=lut0, fix=fx,
                                 out_size=(20, 12)), want)
    # the pulled-back index: 8 rows -> 1, row 7 -> rint(7 * (1 / 8) = 0.875) = 1, which EQUALS the extent and becomes 0
    # (utils_vis.py:25-28); the one output pixel is under the block
    fx = np.zeros((1, 8, 8), np.uint8)
    fx[0, 7, 7] = 1
    want = np.full((1, 1, 1, 3), 255, np.uint8)
    yield ("fix_pulled_back", dict(frames=np.zeros((1, 4, 4, 3), np.uint8), sal=np.zeros((1, 4, 4), np.uint8), lut=lut0, fix=fx,
                                   out_size=(1, 1)), want)
    # the float resize alone, made visible: an empty map (o = 0.8 * img) and a frame whose brightest pixel is 255, so
    # that byte = rint(resized(img) / max(resized) * 255).  Exact 2x enlargement of the row [0, 255, 0, 255] (all rows
    # equal): weights 0.25 / 0.75 inside, the edge samples replicated -> 0, 63.75, 191.25, 191.25, 63.75, 63.75, 191.25, 255
    # in units of img * 255 / max; the maximum of the resized row is the full 255 at the edge, so the bytes are those rounded
    fr = np.zeros((1, 2, 4, 3), np.uint8)
    fr[0, :, 1] = 255
    fr[0, :, 3] = 255
    row = np.array([0, 64, 191, 191, 64, 64, 191, 255], np.uint8)      # 63.75 -> 64, 191.25 -> 191
    yield ("enlarge_2x", dict(frames=fr, sal=np.zeros((1, 2, 4), np.uint8), lut=lut0, out_size=(4, 8)),
           np.repeat(np.repeat(row[None, :, None], 4, axis=0), 3, axis=2)[None])
    # the same frame at the same size: the float resize is the identity
    same = np.zeros((1, 2, 4, 3), np.uint8)
    same[0, :, 1] = 255
    same[0, :, 3] = 255
    yield ("same_size_identity", dict(frames=fr, sal=np.zeros((1, 2, 4), np.uint8), lut=lut0, out_size=(2, 4)), same)


# ------------------------------------------------------------------------------------------------ inputs of the GPU tests

TABLES = {"jet": jet_table, "identity": identity_table, "random": random_table}

# (name, (H0, W0), F, layout, table, fixations, map size or None for the source size, (mid, out) or None for visual_vid's)
GPU_INPUTS = [
    ("360x640", (360, 640), 5, "HWC", "jet", True, None, None),
    ("720x1280", (720, 1280), 5, "CHW", "random", False, None, None),
    ("1080x1920", (1080, 1920), 5, "HWC", "identity", True, None, None),
    ("2160x3840", (2160, 3840), 3, "HWC", "jet", False, None, None),
    ("1280x720", (1280, 720), 5, "CHW", "random", True, None, None),
    ("405x719", (405, 719), 5, "HWC", "jet", True, None, None),
    ("405x719_planar", (405, 719), 5, "CHW", "identity", False, None, None),
    ("720x1280_small_map", (720, 1280), 5, "HWC", "jet", True, (360, 640), None),
    ("img_path", (90, 161), 5, "HWC", "random", True, None, ((90, 161), (90, 161))),          # visual_img: no resizes
    ("odd_sizes", (90, 161), 5, "CHW", "jet", True, (37, 53), ((45, 80), (97, 173))),
]


def gpu_input(name):
    """The seeded input of one GPU comparison: dict(frames [F, H0, W0, 3], sal, fix or None, lut, layout, mid, out)."""
    i = [g[0] for g in GPU_INPUTS].index(name)
    _, (h0, w0), F, layout, table, with_fix, map_size, sizes = GPU_INPUTS[i]
    rng = np.random.RandomState(100 + i)
    frames = rng.randint(0, 256, (F, h0, w0, 3)).astype(np.uint8)
    mh, mw = map_size or (h0, w0)
    sal = np.zeros((F, mh, mw), np.uint8)
    # a blob somewhere plus a little noise that is never 0: where the map is 0 the overlay is 0.8 * img, and under a 2x
    # enlargement of a frame with a fixation (max(o) = 1) its bytes 0.05 * (9 a + 3 b + 3 c + d) tie exactly, often
    for f in range(F):
        cy, cx, sg = rng.uniform(0, mh), rng.uniform(0, mw), rng.uniform(0.05, 0.3) * max(mh, mw)
        gy = np.exp(-0.5 * ((np.arange(mh) - cy) / sg) ** 2)
        gx = np.exp(-0.5 * ((np.arange(mw) - cx) / sg) ** 2)
        sal[f] = np.clip(np.rint(gy[:, None] * gx[None, :] * 250) + rng.randint(1, 7, (mh, mw)), 0, 255).astype(np.uint8)
    fix = None
    if with_fix:
        fix = np.zeros((F, h0, w0), np.uint8)
        for f in range(F):
            fix[f, rng.randint(0, h0, 30), rng.randint(0, w0, 30)] = 1
            fix[f, 0, 0] = fix[f, h0 - 1, w0 - 1] = fix[f, 0, w0 - 1] = 1
    if sizes is None:
        g = visual_geometry(h0, w0)
        sizes = (g[:2], g[2:])
    return dict(frames=frames, sal=sal, fix=fix, lut=TABLES[table](), layout=layout, mid=sizes[0], out=sizes[1])


# Inputs the GPU tests derive from the ones above and compare under the same rule: (name, base, what changes)
GPU_DERIVED = ([(g[0] + "_nofix", g[0], "first frame without its fixations") for g in GPU_INPUTS if g[5]] +
               [("odd_sizes_narrow", "odd_sizes", "the first three frames, their left 100 columns"),
                ("img_path_jet", "img_path", "the default table")])
COMPARED = [g[0] for g in GPU_INPUTS] + [d[0] for d in GPU_DERIVED]


def compared_input(name):
    """`gpu_input` for every name in COMPARED."""
    if name in [g[0] for g in GPU_INPUTS]:
        return gpu_input(name)
    base = [d[1] for d in GPU_DERIVED if d[0] == name][0]
    g = dict(gpu_input(base))
    if name.endswith("_nofix"):
        g.update(frames=g["frames"][:1], sal=g["sal"][:1], fix=None)
    elif name == "odd_sizes_narrow":
        g.update(frames=np.ascontiguousarray(g["frames"][:3, :, :100]), sal=g["sal"][:3], fix=g["fix"][:3])
    elif name == "img_path_jet":
        g.update(lut=jet_table())
    return g


_WANT = {}


def gpu_want(name):
    """(bytes, doubles) of the restatement for `compared_input(name)`, computed once per process."""
    if name not in _WANT:
        g = compared_input(name)
        _WANT[name] = overlay(g["frames"], g["sal"], g["lut"], g["fix"], g["mid"], g["out"])
    return _WANT[name]
