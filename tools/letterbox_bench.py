"""Input letterboxing: the kernel alone and a video end to end.  Prints one JSON line.

kernel:  `ops.letterbox_frames` on 20 interleaved BGR frames per call at 720x1280, 1080x1920 and 2160x3840 into 360x640,
         timed with device events over enough calls to fill a second (or `--calls N`), and the least bytes the call has to
         move (the source rows its taps name, whole rows, plus the destination) over that time against 8 TB/s.
video:   a 192-frame 720x1280 video through `stream.predict_video(model_size=(360, 640))` against the same video
         letterboxed beforehand (the path that existed before the option), device frames and pinned host frames,
         alternated in one process, three windows each.
cpu:     the numpy restatement (tests/letterbox_ref.py) on the host, frames per second -- a CPU restatement for scale, not cv2.

Kernel times from a trace: run `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python
tools/letterbox_bench.py --what kernel --calls 200`, then `python tools/letterbox_bench.py --calls 200 --kernel-stats
DIR/..._kernel_trace.csv`: that run only reads the CSV (the dispatches of `letterbox_u8_kernel` in order: per size three
warm-up calls and `--calls` timed ones) and prints each size's median and mean duration and the same share of 8 TB/s.

Usage:  python tools/letterbox_bench.py [--what kernel,video,cpu] [--calls N] [--frames 20] [--kernel-stats FILE]
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
SIZES = [(720, 1280), (1080, 1920), (2160, 3840)]
MODEL = (360, 640)
WARMUP = 3


def touched_rows(n_out, n_in):
    """Number of distinct source rows the taps of `n_out` outputs name (csrc/letterbox.hip states the rule)."""
    f = ((np.arange(n_out, dtype=np.float64) + 0.5) * (float(n_in) / n_out) - 0.5).astype(np.float32)
    s = np.clip(np.floor(f).astype(np.int64), 0, n_in - 1)
    return len(np.union1d(s, np.minimum(s + 1, n_in - 1)))


def least_bytes(F, h0, w0, R, C):
    from iip_uavsal_saliency_amd import ops
    new_r, _, _, _, _ = ops.letterbox_geometry(h0, w0, R, C)
    return F * (touched_rows(new_r, h0) * w0 * 3 + 3 * R * C)


def kernel_stats(path, F, calls):
    durs = []
    with open(path) as f:
        for r in csv.DictReader(f):
            if "letterbox_u8_kernel" in r["Kernel_Name"]:
                durs.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    durs = [d for _, d in sorted(durs)]
    per = WARMUP + calls
    if len(durs) != per * len(SIZES):
        raise SystemExit("expected %d dispatches of letterbox_u8_kernel (%d sizes x (%d + %d)), the trace has %d" % (
            per * len(SIZES), len(SIZES), WARMUP, calls, len(durs)))
    out = {}
    for i, (h0, w0) in enumerate(SIZES):
        d = durs[i * per + WARMUP:(i + 1) * per]
        med = statistics.median(d) / 1e3
        b = least_bytes(F, h0, w0, *MODEL)
        out["%dx%d" % (h0, w0)] = {"calls": len(d), "median_us": round(med, 2), "mean_us": round(sum(d) / len(d) / 1e3, 2),
                                   "min_us": round(min(d) / 1e3, 2), "least_mb": round(b / 1e6, 2),
                                   "share_of_8TBs_median": round(b / (med / 1e6) / PEAK, 3)}
    print(json.dumps({"kernel_trace": out, "frames_per_call": F}))


def bench_kernel(a, dev):
    import torch
    from iip_uavsal_saliency_amd import ops
    out = {}
    for h0, w0 in SIZES:
        src = torch.randint(0, 256, (a.frames, h0, w0, 3), dtype=torch.uint8, device=dev)
        for _ in range(WARMUP):
            ops.letterbox_frames(src, *MODEL, bgr=True)
        torch.cuda.synchronize(dev)
        calls = a.calls
        if not calls:                                        # enough calls to fill a second, sized from a probe
            t0 = time.perf_counter()
            for _ in range(20):
                ops.letterbox_frames(src, *MODEL, bgr=True)
            torch.cuda.synchronize(dev)
            calls = max(50, int(1.2 * 20 / (time.perf_counter() - t0)))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            ops.letterbox_frames(src, *MODEL, bgr=True)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        us = ms * 1e3 / calls
        b = least_bytes(a.frames, h0, w0, *MODEL)
        out["%dx%d" % (h0, w0)] = {"calls": calls, "window_ms": round(ms, 1), "us_per_call_events": round(us, 2),
                                   "frames_per_s": round(a.frames / (us / 1e6)), "least_mb": round(b / 1e6, 2),
                                   "source_mb": round(a.frames * h0 * w0 * 3 / 1e6, 2),
                                   "share_of_8TBs_events": round(b / (us / 1e6) / PEAK, 3)}
        del src
    return out


def bench_video(a, dev):
    import torch
    from iip_uavsal_saliency_amd import UAVSal, ops, synth
    from iip_uavsal_saliency_amd.stream import predict_video
    h0, w0, T, n = 720, 1280, 8, 192
    R, C = MODEL
    m = UAVSal(time_dims=T)
    synth.load_synth_weights(m, 0)
    m = m.to(dev).eval()
    gp = torch.from_numpy(synth.gauss_priors(1, R // 8, C // 8))[0].to(dev)
    op_ = torch.from_numpy(synth.ob_priors(1, R // 8, C // 8))[0].to(dev)
    src = torch.from_numpy(synth.synth_frames_u8(T, h0, w0, 0)).repeat(n // T, 1, 1, 1).to(dev)       # [192, 3, 720, 1280]
    pre = ops.letterbox_frames(src, R, C, layout="CHW")
    legs = {"pre_device": (pre, {}), "src_device": (src, {"model_size": MODEL}),
            "pre_pinned": (pre.cpu().pin_memory(), {}), "src_pinned": (src.cpu().pin_memory(), {"model_size": MODEL})}
    ref = None
    for name, (fr, kw) in legs.items():                       # warm-up: plans, replicas, streams, allocator
        for _ in range(2):
            sal = predict_video(m, fr[:4 * T], gp, op_, batch_size=1, out_size=(h0, w0), **kw)
        sal = predict_video(m, fr, gp, op_, batch_size=1, out_size=(h0, w0), **kw)
        ref = sal if ref is None else ref
        if not torch.equal(sal, ref):
            raise SystemExit("leg %s: maps differ from the pre-letterboxed device run" % name)
    torch.cuda.synchronize(dev)
    win = {k: [] for k in legs}
    for _ in range(3):
        for name, (fr, kw) in legs.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            predict_video(m, fr, gp, op_, batch_size=1, out_size=(h0, w0), **kw)
            torch.cuda.synchronize(dev)
            win[name].append((time.perf_counter() - t0) * 1e3)
    # the letterbox launch of one group (8 frames), from events
    g = src[:T]
    for _ in range(WARMUP):
        ops.letterbox_frames(g, R, C, layout="CHW")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(200):
        ops.letterbox_frames(g, R, C, layout="CHW")
    e1.record()
    e1.synchronize()
    group_us = e0.elapsed_time(e1) * 1e3 / 200
    out = {"frames": n, "groups": n // T, "source": [h0, w0], "windows_ms": {k: [round(x, 2) for x in v] for k, v in win.items()},
           "frames_per_s_median": {k: round(n / (statistics.median(v) / 1e3), 1) for k, v in win.items()},
           "letterbox_group_us_events": round(group_us, 2), "letterbox_per_video_ms": round(group_us * (n // T) / 1e3, 3),
           "bit_identical_to_pre_letterboxed": True}
    for kind in ("device", "pinned"):
        p, s = win["pre_" + kind], win["src_" + kind]
        out["gap_ms_" + kind] = round(statistics.median(s) - statistics.median(p), 3)
        out["pre_spread_ms_" + kind] = round(max(p) - min(p), 3)
    out["upload_GBs_src_pinned"] = round(n * 3 * h0 * w0 / (statistics.median(win["src_pinned"]) / 1e3) / 1e9, 2)
    return out


def bench_cpu():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import letterbox_ref as R
    out = {}
    for h0, w0 in SIZES:
        src = np.random.RandomState(0).randint(0, 256, (4, h0, w0, 3)).astype(np.uint8)
        R.letterbox(src[:1], *MODEL)
        t0 = time.perf_counter()
        R.letterbox(src, *MODEL, bgr=True)
        out["%dx%d" % (h0, w0)] = round(4 / (time.perf_counter() - t0), 1)
    return {"frames_per_s": out, "note": "numpy restatement of the integer rule on the host CPU (tests/letterbox_ref.py), NOT cv2"}


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
    res = {"model_size": list(MODEL), "frames_per_call": a.frames}
    if "kernel" in what or "video" in what:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("letterbox_bench: no GPU (kernel and video legs measure on the device only)")
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
