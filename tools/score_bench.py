"""Scoring throughput: `scores.score_frames` on a device-resident synthetic video (default 256 frames at 720x1280,
~150 fixations per frame, all seven metrics, the reference's random streams), end to end and split into host draw time
and device time (events).  Prints one JSON line.  The reference's own metric functions, timed on the CPU by
tools/make_score_goldens.py, are read from tests/golden/scores_metrics_720x1280.npz and labelled as CPU.

Per-kernel bandwidth: run the same command under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python
tools/score_bench.py ...`, then run it again with the same arguments and `--kernel-stats DIR/..._kernel_stats.csv`:
that run only reads the CSV and prints each kernel's time and its least bytes (`kernel_bytes`) over that time against
8 TB/s.

Usage:  python tools/score_bench.py [--frames 256] [--height 720] [--width 1280] [--fix 150] [--batch 64] [--iters 2]
                                   [--kernel-stats FILE_kernel_stats.csv]
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from iip_uavsal_saliency_amd import scores, synth      # noqa: E402

PEAK = 8e12


def make_video(F, H, W, n_fix, dev):
    """F frames from 16 distinct generated ones (synthesis is the slow part, not what is measured)."""
    k = min(F, 16)
    sal = synth.synth_salmaps_u8(k, H, W, 1)
    loc = synth.synth_fix_points(k, H, W, n_fix, 1)
    fmap = synth.synth_fix_maps(loc, 12.0).astype(np.float32)
    rep = [i % k for i in range(F)]
    return (torch.from_numpy(sal[rep]).to(dev), torch.from_numpy(fmap[rep]).to(dev), torch.from_numpy(loc[rep]).to(dev),
            loc)


def kernel_bytes(F, N, n_fix):
    """least bytes each kernel moves for the whole video (uint8 map / fixLoc, fp32 fixMap / jitter)."""
    return {
        "stats_kernel": F * N * ((1 + 4 + 1) + (1 + 4 + 1 + 4)),   # two sweeps: without, then with the jitter
        "pass2_kernel": F * N * (1 + 4 + 1) + F * n_fix * 4,
        "hist_kernel": F * N * (1 + 4),
    }


def kernel_table(path, F, N, n_fix):
    need = kernel_bytes(F, N, n_fix)
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Name"]
            short = next((k for k in need if k in name), None) or name.split("(")[0].split("::")[-1]
            total_ns = float(r["TotalDurationNs"])
            calls = int(r["Calls"])
            e = rows.setdefault(short, {"calls": 0, "total_ms": 0.0})
            e["calls"] += calls
            e["total_ms"] += total_ns / 1e6
    return rows, need


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--fix", type=int, default=150)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    F, H, W = a.frames, a.height, a.width
    if a.kernel_stats:
        # every frame the profiled process scored: the timed iterations and the warm-up batch
        rows, need = kernel_table(a.kernel_stats, F * a.iters + a.batch, H * W, a.fix)
        table = {}
        for k, r in rows.items():
            e = {"calls": r["calls"], "total_ms": round(r["total_ms"], 3)}
            if k in need:
                e["share_of_8TBs"] = round(need[k] / (r["total_ms"] / 1e3) / PEAK, 3)
            table[k] = e
        print(json.dumps({"kernels": table}))
        return
    dev = torch.device("cuda", 0)
    sal, fmap, loc, loc_host = make_video(F, H, W, a.fix, dev)
    n_fix = float((loc_host > 0).sum(axis=(1, 2)).mean())
    pts = [np.stack(np.where(l), 1) / np.array([H, W]) for l in loc_host]
    res = {"frames": F, "size": [H, W], "fix_per_frame": n_fix, "batch": a.batch, "keys": scores.KEYS_ORDER}
    scores.score_frames(sal[:a.batch], fmap[:a.batch], loc[:a.batch], all_fix_points=pts, batch_size=a.batch)  # warm-up
    runs = []
    for it in range(a.iters):
        np.random.seed(it)
        torch.manual_seed(it)
        timing = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = scores.score_frames(sal, fmap, loc, all_fix_points=[p.copy() for p in pts], batch_size=a.batch,
                                  timing=timing)
        t = time.perf_counter() - t0
        runs.append({"s": t, "host_draw_s": timing["host_draw_s"], "device_ms": timing["device_ms"]})
    best = min(runs, key=lambda r: r["s"])
    res.update({"frames_per_s": F / best["s"], "end_to_end_s": best["s"], "host_draw_s": best["host_draw_s"],
                "device_ms": best["device_ms"], "device_frames_per_s": F / (best["device_ms"] / 1e3),
                "nan_rows": int(np.isnan(out).any(1).sum()), "mean_scores": dict(zip(scores.KEYS_ORDER,
                                                                                np.nanmean(out, 0).round(6).tolist()))})
    g = os.path.join(ROOT, "tests", "golden", "scores_metrics_720x1280.npz")
    if os.path.exists(g):
        z = np.load(g)
        cpu = {k: float(z["cpu_s_per_frame_" + k]) for k in scores.KEYS_ORDER}
        res["reference_cpu_s_per_frame"] = cpu
        res["reference_cpu_frames_per_s"] = 1.0 / sum(cpu.values())
        res["reference_cpu_note"] = "the reference's metric functions on the build machine's CPU, 720x1280, 150 fixations"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
