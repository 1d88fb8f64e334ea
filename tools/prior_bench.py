"""Time `ops.fixmap_accumulate` at the size of a real video, next to a yardstick outside the code under test.

  * 720 x 1280 x 600 frames of uint8 (553 MB, larger than the last-level cache), resident on the device, in both
    contiguous plane orders: row-major planes `[F,H0,W0]` and the MATLAB order `matio.loadmat(...)["fixMap"]` has
    (memory `[F][W0][H0]`).
  * The yardstick, in the same process on the same tensor in the same layout: `fix_map.sum(dim=0, dtype=torch.int32)`.
  * Warm-up first, then `--reps` timed runs of each, alternating the two; device events around each run.  Reported: the
    median, the fastest and slowest run and the quartiles of each (the run-to-run spread), achieved GB/s of source bytes
    read at the median, and that as a fraction of the 8 TB/s peak.  Both results are compared with each other for equality.
  * End to end: `priors.mean_prior_map` of the same video from host memory, uploaded chunk by chunk through pinned
    buffers (what a dataset pass costs per video), host clock around a call that ends in a device-to-host copy.

Usage:  python tools/prior_bench.py [--frames 600] [--reps 30] [--json OUT.json]
Needs a GPU; there is no CPU fallback for a measurement.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from iip_uavsal_saliency_amd import ops, priors     # noqa: E402

PEAK_GBS = 8000.0


def _stats(ms, nbytes):
    ms = np.sort(np.asarray(ms, np.float64))
    med = float(np.median(ms))
    return dict(median_ms=med, min_ms=float(ms[0]), max_ms=float(ms[-1]), q1_ms=float(np.percentile(ms, 25)),
                q3_ms=float(np.percentile(ms, 75)), gb_per_s=nbytes / med * 1e-6, of_peak=nbytes / med * 1e-6 / PEAK_GBS)


def _time(fn, reps_out):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    reps_out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prior_bench: no GPU; a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    F, h0, w0 = args.frames, args.height, args.width
    nbytes = F * h0 * w0
    g = torch.Generator(device=dev).manual_seed(7)
    base = torch.randint(0, 256, (F, h0, w0), dtype=torch.uint8, device=dev, generator=g)
    base *= (torch.rand((F, h0, w0), device=dev, generator=g) < 0.3)          # a fixation map is mostly empty
    result = dict(shape=[F, h0, w0], bytes=nbytes, reps=args.reps, slab_frames=ops.prior_slab_frames(h0 * w0, F),
                  device=torch.cuda.get_device_name(dev))
    layouts = {"row_major": base,                                             # [F,H0,W0]
               "matlab_order": base.permute(0, 2, 1).contiguous().permute(0, 2, 1)}      # [F,H0,W0] view of memory [F][W0][H0]
    for name, t in layouts.items():
        kernel = lambda: ops.fixmap_accumulate(t)
        torch_sum = lambda: t.sum(dim=0, dtype=torch.int32)
        for _ in range(args.warmup):
            x, y = kernel(), torch_sum()
        torch.cuda.synchronize()
        if not torch.equal(x, y):
            raise SystemExit("prior_bench: %s: fixmap_accumulate and torch's sum differ" % name)
        k_ms, t_ms = [], []
        for _ in range(args.reps):                                            # alternating: both see the same neighbours
            _time(kernel, k_ms)
            _time(torch_sum, t_ms)
        result[name] = dict(fixmap_accumulate=_stats(k_ms, nbytes), torch_sum_int32=_stats(t_ms, nbytes))
        k, s = result[name]["fixmap_accumulate"], result[name]["torch_sum_int32"]
        print("%-12s fixmap_accumulate median %.3f ms (min %.3f, q1 %.3f, q3 %.3f, max %.3f) = %.0f GB/s = %.1f %% of 8 TB/s" % (
            name, k["median_ms"], k["min_ms"], k["q1_ms"], k["q3_ms"], k["max_ms"], k["gb_per_s"], 100 * k["of_peak"]), flush=True)
        print("%-12s torch sum int32   median %.3f ms (min %.3f, q1 %.3f, q3 %.3f, max %.3f) = %.0f GB/s = %.1f %% of 8 TB/s" % (
            name, s["median_ms"], s["min_ms"], s["q1_ms"], s["q3_ms"], s["max_ms"], s["gb_per_s"], 100 * s["of_peak"]), flush=True)
    # the finish step and the end-to-end pass from host memory
    acc = ops.fixmap_accumulate(base)
    f_ms = []
    for i in range(args.warmup + args.reps):
        _time(lambda: ops.prior_map_from_sum(acc, F, 45, 80, with_image=True), f_ms)
    result["prior_map_from_sum_with_image"] = _stats(f_ms[args.warmup:], 4 * h0 * w0)
    print("prior_map_from_sum (45x80 map + source-size picture) median %.3f ms" % result["prior_map_from_sum_with_image"]["median_ms"])
    host = np.ascontiguousarray(base.cpu().numpy().transpose(0, 2, 1))                    # memory [F][W0][H0]
    host = host.transpose(2, 1, 0)[:, :, None, :]                                         # [H0,W0,1,F] as loadmat yields it
    del layouts, base
    want = priors.mean_prior_map(host, 45, 80, device=dev, chunk_frames=args.chunk)       # warm-up: pinned allocation, code
    e_s = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = priors.mean_prior_map(host, 45, 80, device=dev, chunk_frames=args.chunk)
        e_s.append(time.perf_counter() - t0)
    assert np.array_equal(got, want)
    result["mean_prior_map_from_host"] = dict(chunk_frames=args.chunk, seconds=e_s, median_s=float(np.median(e_s)),
                                              gb_per_s=nbytes / float(np.median(e_s)) * 1e-9)
    print("mean_prior_map from host memory, chunks of %d frames: %s s (median %.3f s = %.2f GB/s)" % (
        args.chunk, ["%.3f" % s for s in e_s], float(np.median(e_s)), nbytes / float(np.median(e_s)) * 1e-9), flush=True)
    print(json.dumps(result))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
