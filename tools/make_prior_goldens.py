"""Generate tests/golden/ob_priors.npz by running the reference's own `get_meanmaps` and `read_ob_priors`
(`utils_data.py`, imported unmodified) over the synthetic dataset trees of tests/prior_ref.py.  Run by hand where a
checkout of the reference is available; only the .npz file is committed, and the tests read nothing else.

`utils_data` imports `cv2` and `hdf5storage`, which this image lacks.  `hdf5storage` is a stand-in backed by the package's
`matio`, as in tools/make_loss_goldens.py.  `cv2` is a stub of the three functions the prior code calls:
  resize(img, (w, h))   tests/letterbox_ref.resize_u8, the restated 8-bit INTER_LINEAR rule
  imwrite(path, img)    rint (half to even) and saturate to uint8 -- the documented convertTo(CV_8U) -- through pngio
  imread(path, 0)       pngio
so the file pins the reference's control flow, numpy arithmetic and grouping, not cv2 (see tests/prior_ref.py).
Every tree is built in a temporary directory, and the reference runs with a temporary working directory: it writes its
`<DATASET>_ob_priors_*.mat` into the cwd.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_prior_goldens.py REFERENCE_DIR
"""
import contextlib
import io
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden")

from iip_uavsal_saliency_amd import matio, pngio     # noqa: E402
import letterbox_ref                                 # noqa: E402
import prior_ref as R                                # noqa: E402


def import_reference(ref_dir):
    h5 = types.ModuleType("hdf5storage")
    h5.loadmat = matio.loadmat
    h5.savemat = matio.savemat
    sys.modules["hdf5storage"] = h5
    cv2 = types.ModuleType("cv2")
    cv2.resize = lambda img, size: letterbox_ref.resize_u8(np.asarray(img)[:, :, None], size[1], size[0])[:, :, 0]
    cv2.imwrite = lambda path, img: pngio.write_gray(path, np.clip(np.rint(img), 0, 255).astype(np.uint8))
    cv2.imread = lambda path, flag: pngio.read_gray(path)
    sys.modules["cv2"] = cv2
    sys.path.insert(0, ref_dir)
    import utils_data
    return utils_data


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ud = import_reference(os.path.abspath(sys.argv[1]))
    os.makedirs(OUT, exist_ok=True)
    out = {}
    home = os.getcwd()
    for name, d in R.DATASETS.items():
        with tempfile.TemporaryDirectory() as tree, tempfile.TemporaryDirectory() as cwd:
            vids = R.write_tree(tree, name)
            os.chdir(cwd)
            try:
                with contextlib.redirect_stdout(io.StringIO()):
                    maps = ud.read_ob_priors(tree, name, d["phase_gen"], d["out"][0], d["out"][1], R.CHANNELS)
                written = sorted(os.listdir(cwd))
                again = ud.read_ob_priors(tree, name, d["phase_gen"], d["out"][0], d["out"][1], R.CHANNELS)
            finally:
                os.chdir(home)
            assert np.array_equal(maps, again) and maps.dtype == np.float32
            out["png_" + name] = np.stack([pngio.read_gray(os.path.join(tree, "priors", v[0] + ".png")) for v in vids])
            out["maps_" + name] = maps
            print("%s: %d videos -> %s, PriorMaps %s %s, channels in use %d, last channel mean %.6f" % (
                name, len(vids), written, maps.shape, maps.dtype, int((maps.reshape(-1, maps.shape[2]).max(0) > 0).sum()),
                float(maps[:, :, -1].mean())), flush=True)
    np.savez_compressed(os.path.join(OUT, "ob_priors.npz"), **out)
    print("wrote %s (%d bytes)" % (os.path.join(OUT, "ob_priors.npz"), os.path.getsize(os.path.join(OUT, "ob_priors.npz"))))


if __name__ == "__main__":
    main()
