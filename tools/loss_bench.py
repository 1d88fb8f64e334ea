"""What the criterion and the gaze ground truth cost on the device.  Prints one JSON line.

  1. the fused loss (`losses.loss_fu`: two launches; with the backward three) against a plain eager-torch statement of
     the same formulas on the same device, time per call at 45x80 B=20 and 90x160 B=64, forward and forward + backward;
     both are timed as a host clock around `--iters` back-to-back calls ending in a synchronise (what a training step
     pays, launch overhead included), alternating the two, best of `--repeats`.  The reference's own CPU seconds
     (tools/make_loss_goldens.py, one thread) are read from tests/golden/loss_45x80_B20_f32.npz and labelled as CPU.
  2. `ops.prepare_gaze` frames/s from 720x1280 sources to 45x80 (device-resident uint8 `[F,720,1280]`).
  3. `stream.validate_video` frames/s on the 192-frame 360x640 synthetic video (groups of 8, time_dims 4) and
     `stream.predict_video` on the same video in the same process, sequential and overlapped: the ratio to the sequential
     loop is what ground truth and criterion add to the forward.

Usage:  python tools/loss_bench.py [--iters 2000] [--repeats 5] [--gaze-frames 256] [--video-frames 192] [--skip-video]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from iip_uavsal_saliency_amd import losses, ops, synth      # noqa: E402
import loss_ref64 as R                                       # noqa: E402

EPS = 2.2204e-16


def eager_loss_fu(y_pred, y_true):
    """the formulas of the reference's loss_fu in eager torch, with broadcasting instead of its `.repeat`s"""
    t, f = y_true[:, 0:1], y_true[:, 1:2]

    def std(x):
        return (x - x.mean((2, 3), keepdim=True)) / (x.std((2, 3), keepdim=True) + EPS)
    tn = t / (t.sum((2, 3), keepdim=True) + EPS)
    pn = y_pred / (y_pred.sum((2, 3), keepdim=True) + EPS)
    kl = (tn * torch.log(tn / (pn + EPS) + EPS)).sum((2, 3)).mean(0)
    ts, ps = std(t), std(y_pred)
    t2, p2 = ts - ts.mean((2, 3), keepdim=True), ps - ps.mean((2, 3), keepdim=True)
    cc = ((t2 * p2).sum((2, 3)) / (torch.sqrt((p2 * p2).sum((2, 3)) * (t2 * t2).sum((2, 3))) + EPS)).mean(0)
    nss = ((f * ps).sum((2, 3)) / (f.sum((2, 3)) + EPS)).mean(0)
    return (10 * kl - 2 * cc - nss).mean(0)


def per_call(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def bench_loss(h, w, B, iters, repeats, dev):
    y_pred, y_true = R.random_inputs(h, w, B, 21)
    p, t = torch.from_numpy(y_pred).to(dev), torch.from_numpy(y_true).to(dev)
    q = p.clone().requires_grad_(True)

    def fwd(fn):
        def run():
            with torch.no_grad():
                fn(p, t)
        return run

    def fwdbwd(fn):
        def run():
            q.grad = None
            fn(q, t).backward()
        return run
    cases = {"fused_fwd": fwd(losses.loss_fu), "eager_fwd": fwd(eager_loss_fu),
             "fused_fwdbwd": fwdbwd(losses.loss_fu), "eager_fwdbwd": fwdbwd(eager_loss_fu)}
    for fn in cases.values():                                # warm up every shape and both paths
        per_call(fn, 10)
    best = {k: float("inf") for k in cases}
    for _ in range(repeats):                                 # alternate the candidates inside every repeat
        for k, fn in cases.items():
            best[k] = min(best[k], per_call(fn, iters))
    res = {"size": [h, w], "batch": B}
    res.update({k + "_us": round(v * 1e6, 2) for k, v in best.items()})
    res["eager_over_fused_fwd"] = round(best["eager_fwd"] / best["fused_fwd"], 2)
    res["eager_over_fused_fwdbwd"] = round(best["eager_fwdbwd"] / best["fused_fwdbwd"], 2)
    res["fused_loss"] = float(losses.loss_fu(p, t).item())
    res["eager_loss"] = float(eager_loss_fu(p, t).item())
    g = os.path.join(ROOT, "tests", "golden", "loss_45x80_B20_f32.npz")
    key = "%dx%d_B%d" % (h, w, B)
    if os.path.exists(g):
        z = np.load(g)
        if "cpu_s_fwd_" + key in z:
            res["reference_cpu_fwd_us"] = round(float(z["cpu_s_fwd_" + key]) * 1e6, 1)
            res["reference_cpu_fwdbwd_us"] = round(float(z["cpu_s_fwdbwd_" + key]) * 1e6, 1)
    return res


def bench_gaze(F, repeats, dev):
    k = 8
    loc = synth.synth_fix_points(k, 720, 1280, 40, 3)
    fmap = np.rint(synth.synth_fix_maps(loc, 20.0) * 255).astype(np.uint8)
    rep = [i % k for i in range(F)]
    m, l = torch.from_numpy(fmap[rep]).to(dev), torch.from_numpy(loc[rep]).to(dev)
    ops.prepare_gaze(m, l, 45, 80)
    best = min(per_call(lambda: ops.prepare_gaze(m, l, 45, 80), 200) for _ in range(repeats))
    return {"frames": F, "source": [720, 1280], "target": [45, 80], "ms_per_call": round(best * 1e3, 3),
            "frames_per_s": round(F / best, 1), "source_GB_per_s": round(2 * F * 720 * 1280 / best / 1e9, 1)}


def bench_video(F, repeats, dev):
    from iip_uavsal_saliency_amd import UAVSal
    from iip_uavsal_saliency_amd.stream import predict_video, validate_video
    H, W, T, bs = 360, 640, 4, 2
    m = UAVSal(time_dims=T)
    synth.load_synth_weights(m, 0)
    m = m.to(dev).eval()
    frames = torch.from_numpy(synth.synth_frames_u8(F, H, W, 1)).to(dev)
    gp = torch.from_numpy(synth.gauss_priors(1, H // 8, W // 8)[0]).to(dev)
    op_ = torch.from_numpy(synth.ob_priors(1, H // 8, W // 8)[0]).to(dev)
    k = 8
    loc = synth.synth_fix_points(k, H, W, 25, 6)
    fmap = np.rint(synth.synth_fix_maps(loc, 10.0) * 255).astype(np.uint8)
    rep = [i % k for i in range(F)]
    fix_map, fix_loc = torch.from_numpy(fmap[rep]).to(dev), torch.from_numpy(loc[rep]).to(dev)
    cases = {"validate_video": lambda: validate_video(m, frames, gp, op_, fix_map, fix_loc, batch_size=bs),
             "predict_video_sequential": lambda: predict_video(m, frames, gp, op_, batch_size=bs, overlap=False),
             "predict_video_overlapped": lambda: predict_video(m, frames, gp, op_, batch_size=bs)}
    for fn in cases.values():
        fn()
        fn()
    best = {k_: float("inf") for k_ in cases}
    for _ in range(repeats):
        for k_, fn in cases.items():
            best[k_] = min(best[k_], per_call(fn, 5))
    res = {"frames": F, "size": [H, W], "group": bs * T}
    res.update({k_ + "_frames_per_s": round(F / v, 1) for k_, v in best.items()})
    res["validate_over_sequential_predict"] = round(best["validate_video"] / best["predict_video_sequential"], 3)
    r = validate_video(m, frames, gp, op_, fix_map, fix_loc, batch_size=bs)
    res["groups_run"], res["video_mean"] = r["groups_run"], r["video_mean"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--gaze-frames", type=int, default=256)
    ap.add_argument("--video-frames", type=int, default=192)
    ap.add_argument("--skip-video", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_bench needs the GPU: a CPU run measures nothing")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0),
           "loss": [bench_loss(45, 80, 20, a.iters, a.repeats, dev), bench_loss(90, 160, 64, a.iters, a.repeats, dev)],
           "prepare_gaze": bench_gaze(a.gaze_frames, a.repeats, dev)}
    if not a.skip_video:
        res["video"] = bench_video(a.video_frames, a.repeats, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
