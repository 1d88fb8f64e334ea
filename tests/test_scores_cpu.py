"""Scoring (iip_uavsal_saliency_amd.scores) without a GPU: argument checks of the C entry points, the threshold rule of
AUC-Borji / AUC-shuffled, the host helpers (shuffle maps, fixation lists, mean scores) and the host draw sequence,
driven through the float64 restatement (tests/score_ref64.py) against the reference's goldens."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import _lib, matio, scores, synth

import score_ref64 as R

KEYS = scores.KEYS_ORDER
EVAL_VIDEOS = [("vid_a", 21), ("vid_b", 16), ("vid_c", 35)]   # tools/make_score_goldens.py
EVAL_SIZE = (180, 320)


def _golden(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def _digest(*arrays):
    import hashlib
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------ C ABI

def test_score_desc_size_and_symbols():
    lib = _lib.load()
    assert lib.uavsal_sizeof_desc(14) == C.sizeof(_lib.ScoreDesc)
    assert lib.uavsal_abi_version() == 20


def _desc(**kw):
    d = _lib.ScoreDesc()
    d.sal, d.fix_loc, d.fix_map, d.stats, d.out = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    d.sal_u8, d.loc_u8, d.n_frames, d.n_pix = 1, 1, 2, 100
    d.n_keys = 1
    d.keys[0] = 1
    lib = _lib.load()
    d.ws, d.ws_bytes = 0x100000, lib.uavsal_score_workspace_bytes(C.byref(d))
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("field,value,code", [
    ("sal", 0, -1), ("fix_map", 0, -1), ("fix_loc", 0, -1), ("stats", 0, -1), ("ws", 0, -1),
    ("n_frames", 0, -1), ("n_pix", 1, -1), ("ws_bytes", 256, -1), ("total_fix", -1, -1),
    ("fix_map", 0x30002, -2), ("ws", 0x100010, -2), ("stats", 0x40004, -2),
])
def test_score_entry_points_reject_bad_descriptors(field, value, code):
    lib = _lib.load()
    d = _desc(**{field: value})
    assert lib.uavsal_score_stats(C.byref(d), None) == code
    assert lib.uavsal_score_run(C.byref(d), None) == code


def test_score_run_rejects_bad_keys_and_tables():
    lib = _lib.load()
    assert lib.uavsal_score_stats(None, None) == -1
    assert lib.uavsal_score_workspace_bytes(None) == -1
    d = _desc(n_keys=0)
    assert lib.uavsal_score_run(C.byref(d), None) == -1
    d = _desc(n_keys=8)
    assert lib.uavsal_score_run(C.byref(d), None) == -1
    d = _desc()
    d.keys[0] = 7
    assert lib.uavsal_score_run(C.byref(d), None) == -1
    d = _desc()
    d.keys[0] = 2                                   # AUC_Judd without the fixation tables
    assert lib.uavsal_score_run(C.byref(d), None) == -1
    d = _desc(out=0)
    assert lib.uavsal_score_run(C.byref(d), None) == -1
    d = _desc()
    d.samp[0] = 0x60000                             # indices without offsets
    assert lib.uavsal_score_run(C.byref(d), None) == -1


# ------------------------------------------------------------------------------------------------ threshold rule

def _n_thresholds(m):
    """the rule the kernel uses (csrc/score.hip sample_kernel): ceil(f32(m) / f32(0.1)) in fp32."""
    return int(np.ceil(np.float32(m) / np.float32(0.1)))


def test_threshold_count_rule_matches_np_r():
    ms = [np.float32(k * 0.1) for k in range(11)] + [np.float32(0.3), np.float32(0.7), np.float32(1.0), np.float32(0.0)]
    ms += [np.nextafter(np.float32(k * 0.1), np.float32(2)) for k in range(11)]
    ms += [np.nextafter(np.float32(k * 0.1), np.float32(-1)) for k in range(1, 11)]
    rng = np.random.default_rng(5)
    ms += list(rng.random(20000).astype(np.float32))
    ms += list((rng.integers(0, 256, 2000) / np.float32(255)).astype(np.float32))
    for m in ms:
        m = np.float32(m)
        r = np.r_[0:m:0.1]
        assert len(r) == _n_thresholds(m), m
        assert r.dtype == np.float64 and np.array_equal(r, np.arange(len(r)) * 0.1), m
    assert _n_thresholds(np.float32(0.3)) == 3 and int(np.ceil(np.float64(np.float32(0.3)) / 0.1)) == 4


# ------------------------------------------------------------------------------------------------ host helpers

def test_all_fix_points_and_shuffle_map():
    with tempfile.TemporaryDirectory() as td:
        synth.write_score_tree(td, [("a", 4), ("b", 3)], 30, 40)
        fixs = os.path.join(td, "fixations", "maps")
        pts = scores.all_fix_points(fixs, "UAV2")
        assert len(pts) == 7
        loc = matio.loadmat(os.path.join(fixs, "a_fixPts.mat"))["fixLoc"]
        r, c = np.where(loc[:, :, 0, 1])
        assert np.array_equal(pts[1], np.stack([r / 30, c / 40], 1))
        assert len(scores.all_fix_points(fixs, "DIEM20")) == 7
        with pytest.raises(IndexError):                     # CITIUS: 45 files, as the reference
            scores.all_fix_points(fixs, "CITIUS")
    # rounding: half to even, then the < size bound
    pts = [np.array([[2.5 / 10, 3.5 / 10], [9.6 / 10, 0.0], [0.25, 1.0]])] * 3
    np.random.seed(3)
    got = scores.shuffle_map([p.copy() for p in pts], size=(10, 10), nframes=2)
    np.random.seed(3)
    np.random.randint(0, 3, 2)
    exp = np.zeros((10, 10), np.uint8)
    exp[2, 4] = 1          # (2.5, 3.5) -> (2, 4); (9.6, 0) -> (10, 0) and (2.5, 10) -> (2, 10) are out of bounds
    assert np.array_equal(got, exp)
    # the draw: randint(0, len, nframes) and nothing else
    np.random.seed(4)
    scores.shuffle_map([p.copy() for p in pts], size=(10, 10))
    a = np.random.randint(0, 1000)
    np.random.seed(4)
    np.random.randint(0, 3, 3)
    assert np.random.randint(0, 1000) == a


def test_mean_scores_pools_rows_without_nan():
    with tempfile.TemporaryDirectory() as td:
        for m, vids in (("A", {"v1": [[1, 2], [np.nan, 4]], "v2": [[3, 4], [5, np.nan], [7, 8]]}), ("B", {"v": [[0, 1]]})):
            os.makedirs(os.path.join(td, "Scores", m))
            for v, rows in vids.items():
                matio.savemat(os.path.join(td, "Scores", m, "Score_%s.mat" % v), {"iscore": np.array(rows, float)})
        ms = scores.mean_scores(td)
        assert set(ms) == {"A", "B"}
        assert np.allclose(ms["A"], [(1 + 3 + 7) / 3, (2 + 4 + 8) / 3])
        assert np.allclose(ms["B"], [0, 1])


def test_size_mismatch_raises_value_error():
    sal = torch.zeros(2, 10, 12, dtype=torch.uint8)
    fm = torch.zeros(2, 10, 14)
    fl = torch.zeros(2, 10, 14, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"\(10, 12\).*\(10, 14\)"):
        scores.score_frames(sal, fm, fl)
    with pytest.raises(ValueError):
        scores.metric_nss(sal[:, None].float(), torch.cat([fm[:, None], fl[:, None].float()], 1))
    with tempfile.TemporaryDirectory() as td:
        synth.write_score_tree(td, [("a", 2)], 20, 24)
        matio.savemat(os.path.join(td, "Saliency", "M1", "a.mat"), {"salmap": np.zeros((20, 30, 1, 2), np.uint8)})
        with pytest.raises(ValueError, match="a: salmap size"):
            scores.evalscores_vid(td, td, "UAV2", ["M1"], keys_order=["NSS"])


# ------------------------------------------------------------------------------------------------ draw sequence

def test_host_draws_reproduce_reference_auc_per_metric(golden_dir):
    g = _golden(golden_dir, "scores_metrics_90x160.npz")
    sal, fmap, loc = synth.score_edge_batch(90, 160)
    assert str(g["digest"]) == _digest(sal, fmap, loc)
    shuff = synth.synth_fix_points(8, 90, 160, 60, 77)
    seed = int(g["seed"])
    for k in ("AUC_shuffled", "AUC_Borji", "AUC_Judd", "NSS", "CC", "KLD", "SIM"):
        ref = g["out_" + k][:, 0].astype(np.float64)
        got = R.metric_ref(k, sal, fmap, loc, seed + KEYS.index(k), shuff if k == "AUC_shuffled" else None)
        assert np.array_equal(np.isnan(ref), np.isnan(got)), k
        tol = 1e-6 if k.startswith("AUC") else 2e-5 * np.maximum(1, np.abs(np.nan_to_num(ref)))
        assert np.all(np.abs(np.nan_to_num(got - ref)) <= tol), (k, got, ref)


def _load_tree(td, name):
    s = matio.loadmat(os.path.join(td, "Saliency", "M1", name + ".mat"))["salmap"]
    fm = matio.loadmat(os.path.join(td, "maps", name + "_fixMaps.mat"))["fixMap"]
    fl = matio.loadmat(os.path.join(td, "fixations", "maps", name + "_fixPts.mat"))["fixLoc"]
    n = min(s.shape[3], fm.shape[3], fl.shape[3])
    return [np.ascontiguousarray(a[:, :, 0, :n].transpose(2, 0, 1)) for a in (s, fm, fl)]


def test_host_draws_reproduce_reference_evalscores(golden_dir):
    g = _golden(golden_dir, "scores_evalvid_180x320.npz")
    with tempfile.TemporaryDirectory() as td:
        synth.write_score_tree(td, EVAL_VIDEOS, *EVAL_SIZE, methods=("M1",))
        pts = scores.all_fix_points(os.path.join(td, "fixations", "maps"), "UAV2")
        np.random.seed(int(g["seed"]))
        torch.manual_seed(int(g["seed"]))
        for name, _ in EVAL_VIDEOS:
            sal, fm, fl = _load_tree(td, name)
            got = R.score_frames_ref(sal, fm, fl, KEYS, 16,
                                     lambda bi, n: [scores.shuffle_map(pts, sal.shape[1:]) for _ in range(n)])
            ref = g["iscore_" + name]
            assert got.shape == ref.shape
            assert np.array_equal(np.isnan(got), np.isnan(ref)), name
            for k, key in enumerate(KEYS):
                tol = 1e-6 if key.startswith("AUC") else 2e-5 * np.maximum(1, np.abs(np.nan_to_num(ref[:, k])))
                assert np.all(np.abs(np.nan_to_num(got[:, k] - ref[:, k])) <= tol), (name, key)
