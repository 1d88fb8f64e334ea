"""Generate tests/golden/scores_*.npz by running the reference's own scorer (`utils_score_torch.py`, imported
unmodified) on the CPU.  Run by hand where a checkout of the reference is available; only the .npz files are committed,
and the GPU tests read nothing else.

`utils_score_torch` imports `hdf5storage` and `cv2`, which this image lacks, and uses `np.int` / `np.NaN`, which
NumPy 2 removed.  Before the import: `hdf5storage` is a stand-in backed by the package's `matio` (loadmat / savemat),
`cv2` is an empty module (only the resize branch, not exercised, would use it), and the two NumPy names are restored.
Inputs come from `iip_uavsal_saliency_amd.synth`; each file stores outputs, seeds, shapes and a digest of the inputs.

  1. scores_metrics_90x160.npz: every `metrics[k]` on `synth.score_edge_batch(90, 160)` (8 edge frames);
  2. scores_evalvid_180x320.npz: `evalscores_vid_torch` on `synth.write_score_tree` (3 videos, ragged batches of 16),
     seeds set once before the call; the `ALLFixPts` cache written first from the reference's `getALLFix_vid`;
  3. scores_metrics_720x1280.npz: every `metrics[k]` on 3 full-size frames with ~150 fixations each, plus the CPU
     seconds per frame of each reference metric function (the comparison line of tools/score_bench.py).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_score_goldens.py REFERENCE_DIR
"""
import hashlib
import os
import sys
import tempfile
import time
import types

sys.dont_write_bytecode = True

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden")

from iip_uavsal_saliency_amd import matio, synth      # noqa: E402

KEYS = ['AUC_shuffled', 'NSS', 'AUC_Judd', 'AUC_Borji', 'KLD', 'SIM', 'CC']
SEED = 1234

# shared with the tests (tests/test_scores_*.py regenerate the same inputs)
EVAL_VIDEOS = [("vid_a", 21), ("vid_b", 16), ("vid_c", 35)]
EVAL_SIZE = (180, 320)
FULL_FRAMES, FULL_FIX = 3, 150


def import_reference(ref_dir):
    h5 = types.ModuleType("hdf5storage")
    h5.loadmat = matio.loadmat
    h5.savemat = matio.savemat
    sys.modules["hdf5storage"] = h5
    sys.modules["cv2"] = types.ModuleType("cv2")
    np.int = int
    np.NaN = np.nan
    sys.path.insert(0, ref_dir)
    import utils_score_torch as ref
    return ref


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def tree_digest(root):
    """digest of every input array of a `synth.write_score_tree` tree (the score files excluded)."""
    files = sorted(os.path.relpath(os.path.join(dp, f), root) for dp, _, fs in os.walk(root) for f in fs
                   if f.endswith(".mat") and not os.path.relpath(dp, root).startswith("Scores"))
    return digest(*[a for f in files for a in matio.loadmat(os.path.join(root, f)).values()])


def metric_inputs(sal, fmap, loc):
    y_pred = torch.tensor(sal[:, None]).float()
    y_true = torch.tensor(np.concatenate([fmap[:, None], loc[:, None]], 1)).float()   # float64 concat, then fp32
    return y_pred, y_true


def shuffle_maps_for(n, h, w):
    """the AUC-shuffled `shuff_map` [B,1,H,W] of the per-metric cases: other frames' fixations (hashed points)."""
    return torch.tensor(synth.synth_fix_points(n, h, w, 60, 77)[:, None]).float()


def run_metrics(ref, sal, fmap, loc, timing=False):
    y_pred, y_true = metric_inputs(sal, fmap, loc)
    shuff = shuffle_maps_for(*sal.shape)
    out, secs = {}, {}
    for i, k in enumerate(KEYS):
        np.random.seed(SEED + i)
        torch.manual_seed(SEED + i)
        t0 = time.perf_counter()
        if k == 'AUC_shuffled':
            m = ref.metrics[k](y_pred, y_true, shuff)
        else:
            m = ref.metrics[k](y_pred, y_true)
        secs[k] = (time.perf_counter() - t0) / sal.shape[0]
        out[k] = m.numpy().astype(np.float32)
        print("  %-13s %s  (%.3f s/frame)" % (k, np.array2string(out[k][:, 0], precision=6), secs[k]), flush=True)
    return out, secs


def full_inputs():
    h, w = 720, 1280
    sal = synth.synth_salmaps_u8(FULL_FRAMES, h, w, 5)
    loc = synth.synth_fix_points(FULL_FRAMES, h, w, FULL_FIX, 5)
    fmap = synth.synth_fix_maps(loc, 12.0)
    return sal, fmap, loc


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = import_reference(os.path.abspath(sys.argv[1]))
    os.makedirs(OUT, exist_ok=True)

    print("1. per metric, 90x160 edge batch", flush=True)
    sal, fmap, loc = synth.score_edge_batch(90, 160)
    out, _ = run_metrics(ref, sal, fmap, loc)
    np.savez_compressed(os.path.join(OUT, "scores_metrics_90x160.npz"), keys=np.array(KEYS), seed=SEED,
                        shape=np.array(sal.shape), digest=digest(sal, fmap, loc),
                        **{"out_" + k: v for k, v in out.items()})

    print("2. evalscores_vid_torch, 180x320 tree", flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        root = tmp + "/"
        synth.write_score_tree(tmp, EVAL_VIDEOS, *EVAL_SIZE, methods=("M1",))
        pts = ref.getALLFix_vid(root + "fixations/maps/", "UAV2")
        cache = np.empty(len(pts), dtype=object)
        for i, p in enumerate(pts):
            cache[i] = p
        np.save(root + "ALLFixPts_UAV2.npy", cache, allow_pickle=True)
        np.random.seed(SEED)
        torch.manual_seed(SEED)
        ref.evalscores_vid_torch(root, root, "UAV2", ["M1"], batch_size=16)
        iscores = {}
        for name, _ in EVAL_VIDEOS:
            iscores["iscore_" + name] = matio.loadmat(root + "Scores/M1/Score_%s.mat" % name)["iscore"]
            print("  %s %s, NaN rows %d" % (name, iscores["iscore_" + name].shape,
                                            np.isnan(iscores["iscore_" + name]).any(1).sum()), flush=True)
        dg = tree_digest(tmp)
    np.savez_compressed(os.path.join(OUT, "scores_evalvid_180x320.npz"), keys=np.array(KEYS), seed=SEED,
                        shape=np.array(EVAL_SIZE), videos=np.array([n for n, _ in EVAL_VIDEOS]),
                        frames=np.array([f for _, f in EVAL_VIDEOS]), batch_size=16, digest=dg, **iscores)

    print("3. per metric, 720x1280", flush=True)
    sal, fmap, loc = full_inputs()
    out, secs = run_metrics(ref, sal, fmap, loc)
    np.savez_compressed(os.path.join(OUT, "scores_metrics_720x1280.npz"), keys=np.array(KEYS), seed=SEED,
                        shape=np.array(sal.shape), digest=digest(sal, fmap, loc),
                        **{"out_" + k: v for k, v in out.items()},
                        **{"cpu_s_per_frame_" + k: v for k, v in secs.items()})


if __name__ == "__main__":
    main()
