"""Generate tests/golden/loss_*.npz by running the reference's own criterion (`loss_functions.py`) and fixation
ground truth (`utils_data.py`), both imported unmodified, on the CPU.  Run by hand where a checkout of the reference
is available; only the .npz files are committed, and the tests read nothing else.

`utils_data` imports `cv2` and `hdf5storage`, which this image lacks: `cv2` is an empty module and `hdf5storage` a
stand-in backed by the package's `matio`, as in tools/make_score_goldens.py.  `padding_fixation` / `resize_fixation`
are pure numpy and run as they are; `padding` calls cv2.resize and is NOT run (channel 0 of the ground truth is pinned
by tests/letterbox_ref.py, not by cv2).  Inputs come from tests/loss_ref64.py (built on `iip_uavsal_saliency_amd.synth`);
each file stores outputs, seeds, shapes and a digest of the inputs.

  a. loss_<h>x<w>_B<n>_f32.npz / _f64.npz (45x80 B=20, 90x160 B=8): metric_kl / metric_cc / metric_nss / loss_fu / loss_kl
     and the autograd gradient of loss_fu, in float32 and in float64 (two files: the gradients are the bulk; the gradient
     of loss_kl is recorded on the edge batch only, to keep the files small).
     The f32 file also holds the gaps |fp32 - float64| of every value and, per frame, of the gradient relative to the
     frame's largest gradient -- the reference's own summation error, which the GPU test's tolerance is built from --
     and the CPU seconds per call of the reference (forward, forward + backward) at the shapes tools/loss_bench.py times.
  b. loss_edge_45x80.npz: the same for the edge batch (`loss_ref64.edge_inputs`), the gradients of loss_fu and loss_kl in
     both precisions.
  c. loss_scatter.npz: `padding_fixation` of `loss_ref64.scatter_inputs` for every case of `loss_ref64.SCATTER_CASES`.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_loss_goldens.py REFERENCE_DIR
"""
import os
import sys
import time
import types

sys.dont_write_bytecode = True

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden")

from iip_uavsal_saliency_amd import matio      # noqa: E402
import loss_ref64 as R                         # noqa: E402

BENCH_SHAPES = [(45, 80, 20), (90, 160, 64)]


def import_reference(ref_dir):
    h5 = types.ModuleType("hdf5storage")
    h5.loadmat = matio.loadmat
    h5.savemat = matio.savemat
    sys.modules["hdf5storage"] = h5
    sys.modules["cv2"] = types.ModuleType("cv2")
    sys.path.insert(0, ref_dir)
    import loss_functions
    import utils_data
    return loss_functions, utils_data


def run_loss(lf, y_pred, y_true, dtype, kl_grad=False):
    """every value of the reference at `dtype` and the gradient of loss_fu (of loss_kl too with `kl_grad`), as numpy arrays of
    that precision"""
    out = {}
    t = torch.tensor(y_true).to(dtype)
    for name in ("metric_kl", "metric_cc", "metric_nss", "loss_fu", "loss_kl"):
        p = torch.tensor(y_pred).to(dtype).requires_grad_(True)
        v = getattr(lf, name)(p, t)
        out[name] = v.detach().numpy().reshape(-1)[0]
        if name == "loss_fu" or (kl_grad and name == "loss_kl"):
            v.backward()
            out["grad_" + name] = p.grad.numpy().copy()
    return out


def gaps(o32, o64):
    """|fp32 - float64| of the values; of the gradients per frame, relative to the frame's largest float64 magnitude
    (NaN where either is not finite)"""
    g = {}
    for k in ("metric_kl", "metric_cc", "metric_nss", "loss_fu", "loss_kl"):
        g["gap_" + k] = abs(float(o32[k]) - float(o64[k]))
    for k in [k for k in ("grad_loss_fu", "grad_loss_kl") if k in o32]:
        a, b = o32[k].astype(np.float64), o64[k]
        with np.errstate(invalid="ignore"):
            g["gap_" + k] = np.abs(a - b).reshape(len(a), -1).max(1) / np.abs(b).reshape(len(b), -1).max(1)
    return g


def time_reference(lf, h, w, B):
    y_pred, y_true = R.random_inputs(h, w, B, 21)
    p, t = torch.tensor(y_pred), torch.tensor(y_true)
    best_f = best_fb = float("inf")
    for _ in range(5):
        t0 = time.perf_counter()
        with torch.no_grad():
            lf.loss_fu(p, t)
        best_f = min(best_f, time.perf_counter() - t0)
        q = p.clone().requires_grad_(True)
        t0 = time.perf_counter()
        lf.loss_fu(q, t).backward()
        best_fb = min(best_fb, time.perf_counter() - t0)
    return best_f, best_fb


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    lf, ud = import_reference(os.path.abspath(sys.argv[1]))
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(1)

    timing = {}
    for h, w, B in BENCH_SHAPES:
        f, fb = time_reference(lf, h, w, B)
        timing["cpu_s_fwd_%dx%d_B%d" % (h, w, B)] = f
        timing["cpu_s_fwdbwd_%dx%d_B%d" % (h, w, B)] = fb
        print("reference on the CPU (1 thread), %dx%d B=%d: forward %.3f ms, forward + backward %.3f ms" % (
            h, w, B, f * 1e3, fb * 1e3), flush=True)

    for name, h, w, B, seed in R.RANDOM_CASES:
        y_pred, y_true = R.random_inputs(h, w, B, seed)
        o32, o64 = run_loss(lf, y_pred, y_true, torch.float32), run_loss(lf, y_pred, y_true, torch.float64)
        g = gaps(o32, o64)
        meta = dict(seed=seed, shape=np.array([B, h, w]), digest=R.digest(y_pred, y_true))
        print("a. %s: loss_fu %.7f (f64 %.15f), gaps %s, gradient gaps up to %.2e" % (
            name, o32["loss_fu"], o64["loss_fu"], {k: "%.1e" % v for k, v in g.items() if np.isscalar(v)},
            g["gap_grad_loss_fu"].max()), flush=True)
        np.savez_compressed(os.path.join(OUT, "loss_%s_f32.npz" % name), **meta, **o32, **g, **timing)
        np.savez_compressed(os.path.join(OUT, "loss_%s_f64.npz" % name), **meta, **o64)

    y_pred, y_true = R.edge_inputs()
    o32, o64 = run_loss(lf, y_pred, y_true, torch.float32, True), run_loss(lf, y_pred, y_true, torch.float64, True)
    g = gaps(o32, o64)
    nan32 = np.isnan(o32["grad_loss_fu"]).reshape(len(y_pred), -1)
    print("b. edge batch: loss_fu %.7f (f64 %.15f); frames whose loss_fu gradient is NaN everywhere: %s, anywhere: %s; "
          "loss_kl gradient NaN anywhere: %s" % (o32["loss_fu"], o64["loss_fu"], nan32.all(1).nonzero()[0].tolist(),
                                                 nan32.any(1).nonzero()[0].tolist(),
                                                 bool(np.isnan(o32["grad_loss_kl"]).any())), flush=True)
    np.savez_compressed(os.path.join(OUT, "loss_edge_45x80.npz"), seed=13, shape=np.array(R.EDGE_SHAPE),
                        digest=R.digest(y_pred, y_true), **{"f32_" + k: v for k, v in o32.items()},
                        **{"f64_" + k: v for k, v in o64.items()}, **g)

    out = {}
    for h0, w0, h, w in R.SCATTER_CASES:
        fmap, loc = R.scatter_inputs(h0, w0)
        res = np.stack([ud.padding_fixation(loc[i], h, w) for i in range(len(loc))])
        key = "%dx%d_to_%dx%d" % (h0, w0, h, w)
        out["fix_" + key] = res
        out["digest_" + key] = R.digest(fmap, loc)
        print("c. padding_fixation %s: %s points kept of %s" % (key, (res != 0).reshape(len(res), -1).sum(1).tolist(),
                                                             (loc != 0).reshape(len(loc), -1).sum(1).tolist()), flush=True)
    np.savez_compressed(os.path.join(OUT, "loss_scatter.npz"), cases=np.array(R.SCATTER_CASES), **out)


if __name__ == "__main__":
    main()
