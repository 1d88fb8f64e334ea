"""Helper of the observed-prior tests (not a test): small synthetic dataset trees in the reference's directory contract
(`txt/train.txt`, `txt/val.txt`, `maps/<name>_fixMaps.mat`), generated from seeds, and known-answer videos.

tests/golden/ob_priors.npz (tools/make_prior_goldens.py) holds what the reference's own `get_meanmaps` and
`read_ob_priors` (utils_data.py:497-589, imported unmodified) made of these trees: per dataset the pictures it wrote to
`priors/` (`png_<name>`, in the order of `videos()`) and the `PriorMaps` it saved (`maps_<name>`).  The fixture holds
results only; the inputs come from here.

What the golden pins: the reference's control flow (listing, sorting by path, the first-picture test), its numpy
arithmetic (np.mean over the frames, the min-max scaling with EPS in float64, in the order written there) and its grouping
of more videos than channels (count, the reshape, the last channel's mean, float64 means rounded once to float32, / 255).
What it does NOT pin: cv2.  The reference ran with a stand-in cv2 whose `resize` is tests/letterbox_ref.resize_u8 (the
restated 8-bit INTER_LINEAR rule), whose `imwrite` rounds half to even and saturates (the documented saturate_cast of
convertTo(CV_8U)) and whose `imread` returns the stored bytes: cv2's resize and its rounding on write are pinned to their
documented rules, not to cv2 itself.
"""
import os

import numpy as np

from iip_uavsal_saliency_amd import matio

# name: videos in train.txt, in val.txt, phase_gen, source size, output size.
#   p3   fewer videos than channels: 17 zero channels, no averaging; sides padded ("cols" branch)
#   p20  exactly the channels: no grouping; top and bottom padded ("rows" branch)
#   p41  count = 2, the last channel averages 3 videos; train_val; source size = output size
#   p47  count = 2, the last channel averages 9 videos; "cols" branch
DATASETS = {
    "p3": dict(train=3, val=0, phase_gen="train", src=(15, 20), out=(9, 16), seed=3),
    "p20": dict(train=20, val=0, phase_gen="train", src=(12, 25), out=(12, 10), seed=20),
    "p41": dict(train=30, val=11, phase_gen="train_val", src=(9, 16), out=(9, 16), seed=41),
    "p47": dict(train=47, val=0, phase_gen="train", src=(17, 10), out=(12, 10), seed=47),
}
CHANNELS = 20


def videos(name):
    """[(video name, fixMap uint8 [H0,W0,1,F])] in the order the txt files list them: names without zero padding, so that
    sorting by path reorders them; 3..9 frames; a few bright blobs on a mostly empty map, as a fixation map is."""
    d = DATASETS[name]
    rng = np.random.RandomState(d["seed"])
    h0, w0 = d["src"]
    out = []
    for i in range(d["train"] + d["val"]):
        F = int(rng.randint(3, 10))
        m = rng.randint(0, 256, (h0, w0, 1, F)) * (rng.rand(h0, w0, 1, F) < 0.35)
        out.append(("%s_clip%d" % (name, i), m.astype(np.uint8)))
    return out


def write_tree(root, name):
    """the dataset tree of `name` under `root` (txt/ and maps/; priors/ is for the code under test); returns videos(name)"""
    d = DATASETS[name]
    vids = videos(name)
    os.makedirs(os.path.join(root, "txt"), exist_ok=True)
    os.makedirs(os.path.join(root, "maps"), exist_ok=True)
    with open(os.path.join(root, "txt", "train.txt"), "w") as f:
        f.write("".join(v[0] + "\n" for v in vids[:d["train"]]))
    if d["val"]:
        with open(os.path.join(root, "txt", "val.txt"), "w") as f:
            f.write("".join(v[0] + "\n" for v in vids[d["train"]:]))
    for vname, m in vids:
        matio.savemat(os.path.join(root, "maps", vname + "_fixMaps.mat"), {"fixMap": m})
    return vids


def tie_video():
    """two frames whose per-pixel sums are 0, 1, 3, 5 and 510: means 0, 0.5, 1.5, 2.5 and 255, min 0, max 255, and
    255 + EPS == 255 in double, so the scaled picture is the mean itself and must round half to EVEN: 0, 0, 2, 2, 255
    (round half up would give 1, 2, 3 for the middle three).  `[F=2, H0=1, W0=5]`."""
    a = np.array([[[0, 1, 2, 3, 255]], [[0, 0, 1, 2, 255]]], dtype=np.uint8)
    return a, np.array([[0, 0, 2, 2, 255]], dtype=np.uint8)


def constant_video(h0=6, w0=7, F=4, v=37):
    """max == min: 255 * 0 / (0 + EPS) = 0 everywhere, no NaN"""
    return np.full((F, h0, w0), v, dtype=np.uint8), np.zeros((h0, w0), dtype=np.uint8)
