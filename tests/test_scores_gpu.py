"""Scoring on the MI355X (csrc/score.hip through iip_uavsal_saliency_amd.scores) against the reference's own outputs
(tests/golden/scores_*.npz, tools/make_score_goldens.py) and the float64 restatement (tests/score_ref64.py)."""
import os
import tempfile

import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import matio, scores, synth

import score_ref64 as R

pytestmark = pytest.mark.gpu

KEYS = scores.KEYS_ORDER
EVAL_VIDEOS = [("vid_a", 21), ("vid_b", 16), ("vid_c", 35)]   # tools/make_score_goldens.py
EVAL_SIZE = (180, 320)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _close(got, ref, key, what, rel=2e-5):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, key, got, ref)
    tol = 1e-6 if key.startswith("AUC") else rel * np.maximum(1, np.abs(np.nan_to_num(ref)))
    err = np.abs(np.nan_to_num(got - ref))
    assert np.all(err <= tol), (what, key, err.max(), got, ref)


def _device_metric(key, sal, fmap, loc, seed, shuff):
    y_pred = torch.tensor(sal[:, None]).float().cuda()
    y_true = torch.tensor(np.concatenate([fmap[:, None], loc[:, None]], 1)).float().cuda()
    np.random.seed(seed)
    torch.manual_seed(seed)
    if key == "AUC_shuffled":
        out = scores.metrics[key](y_pred, y_true, torch.tensor(shuff[:, None]).float())
    else:
        out = scores.metrics[key](y_pred, y_true)
    assert out.shape == (sal.shape[0], 1) and out.dtype == torch.float32
    return out.cpu().numpy()[:, 0]


def _check_metrics(g, sal, fmap, loc, shuff):
    seed = int(g["seed"])
    for i, key in enumerate(KEYS):
        got = _device_metric(key, sal, fmap, loc, seed + i, shuff)
        _close(got, g["out_" + key][:, 0], key, "golden")
        r64 = R.metric_ref(key, sal, fmap, loc, seed + i, shuff if key == "AUC_shuffled" else None)
        if key.startswith("AUC"):
            # same fp32 S, same draws: the counts agree exactly, so only the summation order differs
            assert np.array_equal(np.isnan(got), np.isnan(r64)), key
            assert np.all(np.abs(np.nan_to_num(got - r64)) <= 1e-7), (key, got, r64)
        else:
            _close(got, r64, key, "float64", rel=1e-6)


def test_metrics_match_reference_edge_batch(golden_dir):
    g = np.load(os.path.join(golden_dir, "scores_metrics_90x160.npz"))
    sal, fmap, loc = synth.score_edge_batch(90, 160)
    _check_metrics(g, sal, fmap, loc, synth.synth_fix_points(8, 90, 160, 60, 77))


def test_metrics_match_reference_full_size(golden_dir):
    g = np.load(os.path.join(golden_dir, "scores_metrics_720x1280.npz"))
    sal = synth.synth_salmaps_u8(3, 720, 1280, 5)
    loc = synth.synth_fix_points(3, 720, 1280, 150, 5)
    fmap = synth.synth_fix_maps(loc, 12.0)
    _check_metrics(g, sal, fmap, loc, synth.synth_fix_points(3, 720, 1280, 60, 77))


def test_auc_judd_beyond_one_sorted_run():
    """20000 fixations on a uint8 map (5 runs of the LDS sort, ties across runs) and a frame where every pixel is a
    fixation (N == n_fix: IEEE results, as torch)."""
    h, w = 200, 320
    sal = synth.synth_salmaps_u8(3, h, w, 9)
    loc = np.zeros((3, h, w), np.uint8)
    loc[0].reshape(-1)[synth.hash_uniform("many", 20000, 9).argsort()[:20000]] = 1
    loc[1].reshape(-1)[::3] = 1
    loc[2] = 1
    fmap = synth.synth_fix_maps(loc[:, :, :], 2.0)
    got = _device_metric("AUC_Judd", sal, fmap, loc, 7, None)
    r64 = R.metric_ref("AUC_Judd", sal, fmap, loc, 7)
    assert int(loc[0].sum()) == 20000
    assert np.array_equal(np.isnan(got), np.isnan(r64))
    assert np.all(np.abs(np.nan_to_num(got - r64)) <= 1e-7), (got, r64)


def test_evalscores_vid_matches_reference_tree(golden_dir):
    g = np.load(os.path.join(golden_dir, "scores_evalvid_180x320.npz"))
    with tempfile.TemporaryDirectory() as td:
        synth.write_score_tree(td, EVAL_VIDEOS, *EVAL_SIZE, methods=("M1",))
        np.random.seed(int(g["seed"]))
        torch.manual_seed(int(g["seed"]))
        scores.evalscores_vid(td, td, "UAV2", ["M1"], batch_size=16)
        assert os.path.exists(os.path.join(td, "ALLFixPts_UAV2.npy"))
        for name, _ in EVAL_VIDEOS:
            got = matio.loadmat(os.path.join(td, "Scores", "M1", "Score_%s.mat" % name))["iscore"]
            ref = g["iscore_" + name]
            assert got.dtype == np.float64 and got.shape == ref.shape
            for k, key in enumerate(KEYS):
                _close(got[:, k], ref[:, k], key, name)
        # a second call skips the videos already scored; the mean table pools the rows without NaN
        before = os.path.getmtime(os.path.join(td, "Scores", "M1", "Score_vid_a.mat"))
        scores.evalscores_vid(td, td, "UAV2", ["M1"], batch_size=16)
        assert os.path.getmtime(os.path.join(td, "Scores", "M1", "Score_vid_a.mat")) == before
        ms = scores.mean_scores(td)["M1"]
        rows = np.concatenate([g["iscore_" + n] for n, _ in EVAL_VIDEOS])
        rows = rows[~np.isnan(rows).any(1)]
        assert np.allclose(ms, rows.mean(0), rtol=2e-5, atol=1e-6)


def test_score_frames_of_predict_video_output_equals_scored_mat():
    from iip_uavsal_saliency_amd import UAVSal
    from iip_uavsal_saliency_amd.stream import predict_video
    m = UAVSal(time_dims=2)
    synth.load_synth_weights(m, 0)
    m = m.cuda().eval()
    H, W = 72, 104
    u8 = torch.from_numpy(synth.synth_frames_u8(8, H, W)).cuda()
    gp = torch.from_numpy(synth.gauss_priors(1, 9, 13))[0].cuda()
    op = torch.from_numpy(synth.ob_priors(1, 9, 13))[0].cuda()
    loc = synth.synth_fix_points(8, H, W, 15, 4)
    fmap = synth.synth_fix_maps(loc, 3.0)
    pts = [np.stack(np.where(l), 1) / np.array([H, W]) for l in synth.synth_fix_points(12, H, W, 10, 6)]
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "v.mat")
        sal = predict_video(m, u8, gp, op, batch_size=2, out_path=path)
        assert sal.is_cuda and sal.dtype == torch.uint8
        np.random.seed(11)
        torch.manual_seed(11)
        a = scores.score_frames(sal, torch.from_numpy(fmap).cuda(), torch.from_numpy(loc).cuda(), KEYS,
                                [p.copy() for p in pts], batch_size=3)
        mat = matio.loadmat(path)["salmap"][:, :, 0, :].transpose(2, 0, 1)
        np.random.seed(11)
        torch.manual_seed(11)
        b = scores.score_frames(np.ascontiguousarray(mat), fmap, loc, KEYS, [p.copy() for p in pts], batch_size=3)
    assert a.shape == (8, 7) and a.dtype == np.float64
    assert np.array_equal(a, b, equal_nan=True)


def test_two_runs_are_bitwise_equal():
    h, w = 360, 640
    sal = torch.from_numpy(synth.synth_salmaps_u8(10, h, w, 2)).cuda()
    loc = synth.synth_fix_points(10, h, w, 80, 2)
    fmap = torch.from_numpy(synth.synth_fix_maps(loc, 6.0)).float().cuda()
    loc = torch.from_numpy(loc).cuda()
    pts = [np.stack(np.where(l), 1) / np.array([h, w]) for l in synth.synth_fix_points(20, h, w, 30, 8)]
    outs = []
    for _ in range(2):
        np.random.seed(5)
        torch.manual_seed(5)
        outs.append(scores.score_frames(sal, fmap, loc, KEYS, [p.copy() for p in pts], batch_size=4))
    assert np.array_equal(outs[0].view(np.uint64), outs[1].view(np.uint64))
    assert not np.isnan(outs[0]).any()
