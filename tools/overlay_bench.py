"""Heat-map overlay frames: the call alone and a video end to end.  Prints one JSON line.

kernel:  `vis.overlay_frames` on 20 interleaved BGR frames per call at 360x640, 720x1280, 1080x1920 and 2160x3840 with
         source-size maps and fixations, through the sizes of `vis.visual_geometry`, timed with device events over
         back-to-back calls that fill a second (or `--calls N`), and the least bytes a call has to move (the source rows
         its taps name, whole rows, the map rows likewise, the fixation maps, the output) over that time against 8 TB/s.
video:   a 192-frame 720x1280 video through `stream.predict_video(model_size=(360, 640))` with and without
         `overlay=True`, device frames, alternated in one process, three windows each.
cpu:     the numpy restatement (tests/overlay_ref.py) on the host, frames per second -- a CPU restatement for scale, not cv2.

Kernel times from a trace: run `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python
tools/overlay_bench.py --what kernel --calls 50`, then `python tools/overlay_bench.py --calls 50 --kernel-stats
DIR/..._kernel_trace.csv`: that run only reads the CSV (the dispatches of the `overlay_*` kernels in order: per size three
warm-up calls and `--calls` timed ones) and prints each size's median duration per kernel and per call.

Usage:  python tools/overlay_bench.py [--what kernel,video,cpu] [--calls N] [--frames 20] [--kernel-stats FILE]
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8e12
SIZES = [(360, 640), (720, 1280), (1080, 1920), (2160, 3840)]
WARMUP = 3
KERNELS = ["overlay_clear_kernel", "overlay_mid_kernel", "overlay_stamp_kernel", "overlay_out_kernel<0>", "overlay_out_kernel<1>"]


def touched_rows(n_out, n_in):
    """Number of distinct source rows the taps of `n_out` outputs name (csrc/resize_u8.h states the rule)."""
    f = ((np.arange(n_out, dtype=np.float64) + 0.5) * (float(n_in) / n_out) - 0.5).astype(np.float32)
    s = np.clip(np.floor(f).astype(np.int64), 0, n_in - 1)
    return len(np.union1d(s, np.minimum(s + 1, n_in - 1)))


def least_bytes(F, h0, w0):
    from iip_uavsal_saliency_amd import vis
    mid_h, _, out_h, out_w = vis.visual_geometry(h0, w0)
    rows = touched_rows(mid_h, h0)
    return F * (rows * w0 * 3 + rows * w0 + h0 * w0 + 3 * out_h * out_w)      # frame rows, map rows, fixation map, output


def kernel_stats(path, F, calls):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            if "overlay_" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    per = (WARMUP + calls) * len(KERNELS)
    if len(rows) != per * len(SIZES):
        raise SystemExit("expected %d overlay dispatches (%d sizes x (%d + %d) calls x %d kernels), the trace has %d" % (
            per * len(SIZES), len(SIZES), WARMUP, calls, len(KERNELS), len(rows)))
    out = {}
    for i, (h0, w0) in enumerate(SIZES):
        d = rows[i * per + WARMUP * len(KERNELS):(i + 1) * per]
        by = {}
        for k, name in enumerate(KERNELS):
            by[name] = round(statistics.median(e - s for s, e, _ in d[k::len(KERNELS)]) / 1e3, 2)
        busy = [sum(e - s for s, e, _ in d[c * len(KERNELS):(c + 1) * len(KERNELS)]) for c in range(calls)]
        span = [d[(c + 1) * len(KERNELS) - 1][1] - d[c * len(KERNELS)][0] for c in range(calls)]
        b = least_bytes(F, h0, w0)
        out["%dx%d" % (h0, w0)] = {"calls": calls, "median_us_per_kernel": by,
                                   "kernels_us_per_call_median": round(statistics.median(busy) / 1e3, 2),
                                   "first_start_to_last_end_us_median": round(statistics.median(span) / 1e3, 2),
                                   "least_mb": round(b / 1e6, 2),
                                   "share_of_8TBs_kernels": round(b / (statistics.median(busy) / 1e9) / PEAK, 4)}
    print(json.dumps({"kernel_trace": out, "frames_per_call": F}))


def _inputs(torch, F, h0, w0, dev):
    g = torch.Generator(device="cpu").manual_seed(h0)
    src = torch.randint(0, 256, (F, h0, w0, 3), dtype=torch.uint8, generator=g).to(dev)
    yy = torch.linspace(-1, 1, h0)[:, None]
    xx = torch.linspace(-1, 1, w0)[None, :]
    sal = (torch.exp(-4 * (yy * yy + xx * xx)) * 250 + 1).round().to(torch.uint8)[None].repeat(F, 1, 1).to(dev)
    fix = (torch.rand((F, h0, w0), generator=g) < 3e-5).to(torch.uint8).to(dev)
    return src, sal, fix


def bench_kernel(a, dev):
    import torch
    from iip_uavsal_saliency_amd import vis
    out = {}
    for h0, w0 in SIZES:
        src, sal, fix = _inputs(torch, a.frames, h0, w0, dev)
        mid_h, mid_w, out_h, out_w = vis.visual_geometry(h0, w0)

        def call():
            return vis.overlay_frames(src, sal, fix, (mid_h, mid_w), (out_h, out_w))
        for _ in range(WARMUP):
            call()
        torch.cuda.synchronize(dev)
        calls = a.calls
        if not calls:                                        # enough calls to fill a second, sized from a probe
            t0 = time.perf_counter()
            for _ in range(10):
                call()
            torch.cuda.synchronize(dev)
            calls = max(30, int(1.2 * 10 / (time.perf_counter() - t0)))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            call()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        us = ms * 1e3 / calls
        b = least_bytes(a.frames, h0, w0)
        out["%dx%d" % (h0, w0)] = {"calls": calls, "window_ms": round(ms, 1), "us_per_call_events": round(us, 2),
                                   "frames_per_s": round(a.frames / (us / 1e6)), "mid": [mid_h, mid_w], "out": [out_h, out_w],
                                   "least_mb": round(b / 1e6, 2), "share_of_8TBs_events": round(b / (us / 1e6) / PEAK, 4)}
        del src, sal, fix
    return out


def bench_video(a, dev):
    import torch
    from iip_uavsal_saliency_amd import UAVSal, synth, vis
    from iip_uavsal_saliency_amd.stream import predict_video
    h0, w0, T, n = 720, 1280, 8, 192
    R, C = 360, 640
    m = UAVSal(time_dims=T)
    synth.load_synth_weights(m, 0)
    m = m.to(dev).eval()
    gp = torch.from_numpy(synth.gauss_priors(1, R // 8, C // 8))[0].to(dev)
    op_ = torch.from_numpy(synth.ob_priors(1, R // 8, C // 8))[0].to(dev)
    src = torch.from_numpy(synth.synth_frames_u8(T, h0, w0, 0)).repeat(n // T, 1, 1, 1).to(dev)       # [192, 3, 720, 1280]
    legs = {"plain": {}, "overlay": {"overlay": True}}
    ref = None
    for name, kw in legs.items():                             # warm-up: plans, replicas, streams, allocator
        for _ in range(2):
            predict_video(m, src[:4 * T], gp, op_, batch_size=1, model_size=(R, C), **kw)
        res = predict_video(m, src, gp, op_, batch_size=1, model_size=(R, C), **kw)
        sal = res[0] if kw else res
        ref = sal if ref is None else ref
        if not torch.equal(sal, ref):
            raise SystemExit("leg %s: maps differ from the run without overlay" % name)
        del res
    torch.cuda.synchronize(dev)
    win = {k: [] for k in legs}
    for _ in range(3):
        for name, kw in legs.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            res = predict_video(m, src, gp, op_, batch_size=1, model_size=(R, C), **kw)
            torch.cuda.synchronize(dev)
            win[name].append((time.perf_counter() - t0) * 1e3)
            del res
    # the overlay of the whole video alone, on maps already there
    sal = predict_video(m, src, gp, op_, batch_size=1, model_size=(R, C))
    for _ in range(2):
        vis.visual_video(src, sal, layout="CHW")
    torch.cuda.synchronize(dev)
    alone = []
    for _ in range(3):
        t0 = time.perf_counter()
        vis.visual_video(src, sal, layout="CHW")
        torch.cuda.synchronize(dev)
        alone.append((time.perf_counter() - t0) * 1e3)
    p, o = win["plain"], win["overlay"]
    return {"frames": n, "source": [h0, w0], "windows_ms": {k: [round(x, 2) for x in v] for k, v in win.items()},
            "median_ms": {k: round(statistics.median(v), 2) for k, v in win.items()},
            "spread_ms": {k: round(max(v) - min(v), 2) for k, v in win.items()},
            "frames_per_s_median": {k: round(n / (statistics.median(v) / 1e3), 1) for k, v in win.items()},
            "added_ms_median": round(statistics.median(o) - statistics.median(p), 2),
            "visual_video_alone_ms": [round(x, 2) for x in alone], "maps_bit_identical": True}


def bench_cpu():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import overlay_ref as R
    out = {}
    for h0, w0 in SIZES:
        rng = np.random.RandomState(0)
        src = rng.randint(0, 256, (3, h0, w0, 3)).astype(np.uint8)
        sal = rng.randint(1, 256, (3, h0, w0)).astype(np.uint8)
        fix = (rng.rand(3, h0, w0) < 3e-5).astype(np.uint8)
        g = R.visual_geometry(h0, w0)
        R.overlay(src[:1], sal[:1], R.jet_table(), fix[:1], g[:2], g[2:])
        t0 = time.perf_counter()
        R.overlay(src, sal, R.jet_table(), fix, g[:2], g[2:])
        out["%dx%d" % (h0, w0)] = round(3 / (time.perf_counter() - t0), 2)
    return {"frames_per_s": out, "note": "numpy float64 restatement on the host CPU (tests/overlay_ref.py), NOT cv2"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="kernel,video,cpu")
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        if not a.calls:
            raise SystemExit("--kernel-stats needs the --calls N of the traced run")
        kernel_stats(a.kernel_stats, a.frames, a.calls)
        return
    what = a.what.split(",")
    res = {"frames_per_call": a.frames}
    if "kernel" in what or "video" in what:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("overlay_bench: no GPU (kernel and video legs measure on the device only)")
        dev = torch.device("cuda", 0)
        if "kernel" in what:
            res["kernel"] = bench_kernel(a, dev)
        if "video" in what:
            res["video"] = bench_video(a, dev)
    if "cpu" in what:
        res["cpu_restatement"] = bench_cpu()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
