#!/usr/bin/env python3
"""Benchmark of the UAVSal HIP path: saliency frames/s at 360x640 on N MI355X.

A "step" is one pass of the hot path (`UAVSal.forward_clips`) over one batch of
synthetic clips that are already resident in HBM.  Default workload (N=1) is
BASELINE.json configs[1]: 360x640, batch=1 clip, seq=8 frames, exact-fp32 MFMA.
For N>1 every rank runs the same per-GPU workload on its own clips (weak
scaling, clips are independent) and the output maps are exchanged with ONE RCCL
all-gather per step.  Rank 0 prints one JSON line.

A plain run sets up, warms up, times exactly --steps steps (one window) and prints
the headline.  --dump-outputs DIR also writes what the last timed step returned
(maps, state) as DIR/<name>.npy.  --full adds the objects below (each can still be
left out with its --no-* option) and times the headline over three windows.

Extra objects on a --full line:
  roofline      dominant kernel (largest summed device time): algorithmic FLOP/s
                (or bytes/s) per launch / average launch duration measured with
                hipEvents on the launch stream, against the MI355X peak.
  roofline_dw   the depthwise 3x3 kernel against the HBM roofline (north_star
                asks >= 60 %), algorithmic bytes per SURVEY.md 8(d).
  cpu_baseline  the oracle (CPU restatement, torch fp32) timed on this box's
                host cores on ONE clip of the same workload (bounded sample).
  parity        max-abs of the saliency map vs that CPU run on the same inputs.
  extra         the same workload and BASELINE.json's configs[2] shape (8 clips) in split-fp16 MFMA.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.distributed as dist

PEAK_TFLOPS = {"f32": 157.3, "f16x3": 2500.0 / 3, "bf16x3": 2500.0 / 3, "bf16": 2500.0}   # dense; MI355X_MICROARCH.md
PEAK_HBM_GBS = 8000.0
DTYPE_NAME = {"f32": "f32", "f16x3": "f32 (3x f16 split MFMA, f32 accumulate)",
              "bf16x3": "f32 (3x bf16 split MFMA, f32 accumulate)", "bf16": "bf16"}
TILE_NAME = {1: "128x128", 2: "128x64", 3: "128x32", 4: "64x64", 5: "128x256", 6: "256x256", 7: "256x128",
             8: "128x128 (32-float K stages)", 9: "256x128 (32-float K stages)", 10: "128x128 (32-float K stages, flat pipeline)",
             11: "64x64 (32-float K stages)"}
PREC_ID = {"f32": 0, "bf16x3": 1, "bf16": 2, "f16x3": 3}
# template arguments of the kernel instance each (precision, tile) launches, as rocprofv3 prints them
F32_INST = {1: "2, 2, 2, 2, %d, 3, 1, false", 2: "4, 1, 1, 2, %d, 4, 1, false", 3: "4, 1, 1, 1, %d, 4, 1, false",
            4: "2, 2, 1, 1, %d, 3, 4, false", 7: "4, 2, 2, 2, %d, 3, 1, false"}
F32_SK_INST = {1: "2, 2, 2, 2, %d, 3, 1, true", 3: "4, 1, 1, 1, %d, 4, 1, true", 4: "2, 2, 1, 1, %d, 3, 2, true"}   # stream-K
H16_INST = {1: "%d, 2, 2, 2, 2, %d", 2: "%d, 4, 1, 1, 2, %d", 3: "%d, 4, 1, 1, 1, %d", 4: "%d, 2, 2, 1, 1, %d",
            5: "%d, 2, 4, 2, 2, %d", 6: "%d, 2, 4, 4, 2, %d"}


H16_DMA_INST = {1: "2, 2, 2, 2, %d, 2", 5: "2, 4, 2, 2, %d, 3", 6: "2, 4, 4, 2, %d, 2"}    # pre-split LDS-DMA path


def kernel_symbol(prec, tile, taps, streamk=0, split=False):
    if split:
        return "conv_gemm_h16_dma_kernel<%s>" % (H16_DMA_INST[tile] % taps)
    if prec == "f32" and tile in (8, 9, 10):      # conv_gemm_k32.hip
        return "conv_gemm_f32_k32%s_kernel<%s, 2, %d, 2>" % ("p" if tile == 10 else "", 4 if tile == 9 else 2, taps)
    if prec == "f32" and tile == 11:              # 64 x 64; with the workspace the K-split instance (..., true>) may run
        return "conv_gemm_f32_k32s_kernel<%d>" % taps
    if prec == "f32":
        return "conv_gemm_f32_dma_kernel<%s>" % ((F32_SK_INST if streamk else F32_INST)[tile] % taps)
    return "conv_gemm_kernel<%s>" % (H16_INST[tile] % (PREC_ID[prec], taps))


PROFILE_ROUND = "r5"
PER_OP_TIMING = ("isolated: hipEvents around each op of the plan on the launch stream; per op the MIN of 2 x 5-launch means "
                 "(rounds 1-3: one 5-launch mean), back to back on the same buffers, after one run of the ops in front of it")


def _wl_tag(C, T, H, W, prec):
    """File tag of a workload's committed profile summaries: f32_c1 for the 8-frame 360x640 ones, f32_c4_720x1280_t16 otherwise."""
    return "%s_c%d" % (prec, C) + ("" if (T, H, W) == (8, 360, 640) else "_%dx%d_t%d" % (H, W, T))


def traffic_file(C, prec, T=8, H=360, W=640):
    return os.path.join("profiles", "%s_hbm_traffic_%s.json" % (PROFILE_ROUND, _wl_tag(C, T, H, W, prec)))


def inloop_file(C, prec, T=8, H=360, W=640, lanes0=False):
    """Committed rocprofv3 kernel-stats summary of this workload's bench command; `lanes0`: the same command with --lanes 0 (every
    kernel alone on the chip, in plan order)."""
    return os.path.join("profiles", "%s_kernel_stats_%s%s.json" % (PROFILE_ROUND, _wl_tag(C, T, H, W, prec), "_lanes0" if lanes0 else ""))


def _stamped(path, T, H, W):
    """A committed profile summary, or (None, why): it must exist (one file per workload, `_wl_tag`) and carry the hash of
    the kernel sources of THIS build."""
    full = os.path.join(ROOT, path)
    if not os.path.exists(full):
        return None, "no collection for this workload"
    blob = json.load(open(full))
    if blob.get("__stamp__", {}).get("kernel_sources_sha16") != kernel_sources_sha16():
        return None, "stale: kernel sources changed since the collection"
    return blob, "ok"


def measured_traffic(symbol, C, T, H, W, prec):
    """(HBM bytes per launch, source) from the committed rocprofv3 PMC passes: two separate `--pmc` runs of
    this bench command (FETCH_SIZE doubled per the gfx950 note of MI355X_MICROARCH.md, + WRITE_SIZE),
    summarised by tools/traffic_report.py.  The counters cannot be collected by the run that prints the
    line (rocprofv3 wraps the process), so the file carries a stamp -- a hash of the kernel sources it was
    collected on -- and the figure is withheld (null) when the stamp does not match this build or there is no
    collection for the workload (tools/collect_profiles.sh: 1 and 8 clips in f32, 8 clips in f16x3)."""
    src = {"file": traffic_file(C, prec, T, H, W), "method": "rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate passes), FETCH x2 (gfx950)"}
    blob, why = _stamped(src["file"], T, H, W)
    src["status"] = why
    if blob is None:
        return None, src
    src["stamp"] = blob.get("__stamp__", {})
    rec = blob.get(symbol)
    if rec is None:
        src["status"] = "kernel not in the PMC summary"
        return None, src
    return round(rec["hbm_mb_per_launch"] * 1e6), src


def in_loop_timing(symbol, C, T, H, W, prec, lanes0=False):
    """Average duration of the kernel instance INSIDE the timed loop (rocprofv3 --kernel-trace --stats of this bench
    command, tools/kernel_stats_report.py): lanes overlap there and kernels queue behind each other, so it differs from
    the isolated per-op hipEvent timing the `roofline` objects are computed from."""
    f = inloop_file(C, prec, T, H, W, lanes0)
    blob, why = _stamped(f, T, H, W)
    if blob is None or symbol not in blob:
        return {"status": why if blob is None else "kernel not in the summary", "file": f}
    return {"status": "ok", "file": f, "avg_launch_us": blob[symbol]["avg_us"], "calls": blob[symbol]["calls"]}


def kernel_sources_sha16():
    import hashlib
    h = hashlib.sha256()
    base = os.path.join(ROOT, "iip_uavsal_saliency_amd", "csrc")
    for name in sorted(os.listdir(base)):
        if name.endswith((".hip", ".h")):
            h.update(name.encode())
            h.update(open(os.path.join(base, name), "rb").read())
    h.update(open(os.path.join(ROOT, "include", "uavsal_hip.h"), "rb").read())
    return h.hexdigest()[:16]


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def log(msg):
    if int(os.environ.get("RANK", "0")) == 0:
        print("[bench %.1fs] %s" % (time.perf_counter() - _T0, msg), file=sys.stderr, flush=True)


_T0 = time.perf_counter()


def host_cores():
    """CPU share of this process (the GPU box gives a 1-GPU job 16 cores; os.cpu_count() would
    report the whole host and oversubscribe oneDNN)."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(n, 16))


def make_clips(C, T, H, W, seed=0):
    from iip_uavsal_saliency_amd import synth
    h, w = H // 8, W // 8
    xs, g, o = [], [], []
    for c in range(C):
        xs.append(torch.from_numpy(synth.normalize_frames(synth.synth_frames_u8(T, H, W, seed + c))))
        g.append(torch.from_numpy(synth.gauss_priors(T, h, w)))
        o.append(torch.from_numpy(synth.ob_priors(T, h, w, seed=seed + c)))
    return torch.stack(xs), [torch.stack(g), torch.stack(o)]


DUMP_BUDGET_BYTES = 60 * 1000 * 1000


def dump_outputs(path, arrays):
    """Write each output tensor as `path/<name>.npy` in float32.  When they exceed DUMP_BUDGET_BYTES together, each is
    replaced by the same share of its elements, drawn with a fixed seed (flattened order, indices sorted), so that two
    builds run with the same arguments still compare element for element."""
    os.makedirs(path, exist_ok=True)
    host = {k: v.detach().float().cpu().numpy() for k, v in arrays.items()}
    total = sum(a.nbytes for a in host.values())
    for name, a in host.items():
        if total > DUMP_BUDGET_BYTES:
            keep = a.size * DUMP_BUDGET_BYTES // total
            a = a.reshape(-1)[np.sort(np.random.default_rng(0).choice(a.size, keep, replace=False))]
        np.save(os.path.join(path, name + ".npy"), a)
    return sorted(host)


def kernel_rooflines(eng, prec, iters=5):
    """Per-op device time (hipEvents on the launch stream) grouped by kernel instance."""
    groups = {}
    for i, m in enumerate(eng.ops_meta):
        # two measurements, the smaller one: a one-off stall of the box (tens of ms, seen a few times per hour on this pool) inside
        # a 5-launch average would otherwise own the whole family figure.  The ops in front of it are run once first: activations
        # share addresses by liveness (engine.py, arena), so after a full forward an op's inputs have been overwritten by later
        # buffers -- the timed launches must read the data they read in a forward (ReLU6 zeros and all: the fp32 GEMMs run ~15 %
        # slower on random operands than on half-zero ones)
        eng.run_ops(0, i)
        ms = min(eng.time_ops(i, i + 1, iters), eng.time_ops(i, i + 1, iters))
        mp = m.get("prec") or prec          # (an op may run in another precision than the plan's: the exact-fp32 Winograd steps of an f16x3 plan)
        if m["kind"].startswith("conv"):
            key = kernel_symbol(mp, m["tile"], 9 if m["kind"] == "conv3" else 1, m.get("streamk", 0), m.get("split", False))
            if m.get("dwproj"):
                key = "dwproj_kernel<%d, %s, 0>" % (PREC_ID[mp], {256: "2, 4, 2, 2", 128: "2, 4, 2, 1", 64: "4, 2, 1, 1", 32: "4, 1, 1, 1"}[m["dwproj"]])
            elif m.get("fused_dw"):
                key = "conv_gemm_kernel<%s, true>" % (H16_INST[m["tile"]] % (PREC_ID[mp], 1))
        elif m["kind"] in ("dw", "dw_dot", "fused_ir"):
            key = m["kernel"]                  # uavsal_dw_variant / the fused block instance the library launches
        else:
            key = m["kind"]
        if os.environ.get("UAVSAL_BENCH_OPS"):
            print("[op %3d] %-28s %-8s %9.1f us %8.1f GB/s %8.2f TFLOP/s" % (
                i, m["name"], key[-22:], ms * 1e3, m["bytes"] / ms / 1e6, m["flops"] / ms / 1e9), file=sys.stderr)
        g = groups.setdefault(key, {"ms": 0.0, "flops": 0.0, "bytes": 0.0, "launches": 0, "kind": m["kind"], "unfused_bytes": 0.0, "prec": mp})
        g["unfused_bytes"] += m.get("unfused_bytes", 0.0)
        g["flops_executed"] = g.get("flops_executed", 0.0) + m.get("flops_executed", 0.0)
        g["ms"] += ms
        g["flops"] += m["flops"]
        g["bytes"] += m["bytes"]
        g["launches"] += 1
    return groups


def roofline_obj(name, g, prec):
    prec = g.get("prec") or prec
    sec = g["ms"] * 1e-3
    if g["kind"].startswith("conv"):
        ach = g["flops"] / sec / 1e12
        peak = PEAK_TFLOPS[prec]
        return {"kernel": name, "bound": "mfma", "achieved": round(ach, 2), "peak": round(peak, 1), "unit": "TFLOP/s",
                "frac": round(ach / peak, 4), "traffic": None, "launches_per_step": g["launches"],
                "avg_launch_us": round(g["ms"] * 1e3 / g["launches"], 2),
                "alg_gflop_per_launch": round(g["flops"] / g["launches"] / 1e9, 3),
                "alg_mb_per_launch": round(g["bytes"] / g["launches"] / 1e6, 3)}
    ach = g["bytes"] / sec / 1e9
    return {"kernel": name, "bound": "hbm", "achieved": round(ach, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
            "frac": round(ach / PEAK_HBM_GBS, 4), "traffic": None, "launches_per_step": g["launches"],
            "avg_launch_us": round(g["ms"] * 1e3 / g["launches"], 2),
            "alg_mb_per_launch": round(g["bytes"] / g["launches"] / 1e6, 3)}


def depthwise_family(groups):
    """every stand-alone depthwise launch of the forward, algorithmic bytes
    N*C*(HiWi+HoWo)*4 + 44*C summed over the layers / their summed kernel time, against the HBM peak; the
    per-instance split is kept beside the family figure.  Depthwise layers that run inside a fused
    inverted-residual launch (features[1..7]) have no launch of their own: they are reported by
    `roofline_fused` (fused-floor bytes / time), as 8(d) prescribes."""
    dw = {k: g for k, g in groups.items() if g["kind"] == "dw"}
    if not dw:
        return None
    byts = sum(g["bytes"] for g in dw.values())
    ms = sum(g["ms"] for g in dw.values())
    fam = {"kernel": "depthwise 3x3 family (all stand-alone dw launches of the forward)", "bound": "hbm",
           "achieved": round(byts / ms / 1e6, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
           "frac": round(byts / ms / 1e6 / PEAK_HBM_GBS, 4), "traffic": None,
           "launches_per_step": sum(g["launches"] for g in dw.values()),
           "alg_mb_per_step": round(byts / 1e6, 3), "kernel_ms_per_step": round(ms, 4), "instances": {}}
    for k, g in sorted(dw.items(), key=lambda kv: -kv[1]["ms"]):
        fam["instances"][k] = {"launches": g["launches"], "ms": round(g["ms"], 4), "alg_mb": round(g["bytes"] / 1e6, 3),
                               "frac": round(g["bytes"] / g["ms"] / 1e6 / PEAK_HBM_GBS, 4)}
    return fam


def family_in_loop(fam, C, T, H, W, prec, lanes0=False):
    """The same depthwise launches INSIDE the timed loop: per instance the rocprofv3 average duration (committed kernel-stats
    summary of this bench command, stamped with the kernel sources) x its launches per step; neither warmed by back-to-back
    repeats on the same buffers (the isolated figure is) -- but stretched wherever another lane's kernels share the chip."""
    us, miss = 0.0, []
    for inst, rec in fam["instances"].items():
        il = in_loop_timing(inst, C, T, H, W, prec, lanes0)
        if il.get("status") != "ok":
            miss.append(inst)
            status = il.get("status")
            continue
        us += il["avg_launch_us"] * rec["launches"]
    if miss:
        return {"status": status, "missing": miss, "file": inloop_file(C, prec, T, H, W, lanes0)}
    gbs = fam["alg_mb_per_step"] * 1e6 / (us * 1e-6) / 1e9
    return {"status": "ok", "file": inloop_file(C, prec, T, H, W, lanes0), "kernel_ms_per_step": round(us * 1e-3, 4),
            "achieved": round(gbs, 1), "frac": round(gbs / PEAK_HBM_GBS, 4)}


def fused_family(groups, mid=False):
    """Fused inverted-residual launches: fused-floor bytes (block input + output [+ residual read]) / time.
    `mid`: the mid-channel kernel's launches (features[8..13]) instead of the small-channel kernel's (features[1..7]) -- a
    different regime: weights of 0.2-0.4 MB streamed by every workgroup, bound by the matrix pipe / the CU's LDS-DMA rate,
    so its `frac` against HBM says little; `tflops_fp32` (halo recompute not counted) is the figure to read."""
    fu = {k: g for k, g in groups.items() if g["kind"] == "fused_ir" and k.startswith("fused_mid") == mid}
    if not fu:
        return None
    byts = sum(g["bytes"] for g in fu.values())
    ms = sum(g["ms"] for g in fu.values())
    fl = sum(g["flops"] for g in fu.values())
    return {"kernel": ("fused_mid_kernel (features[8..13] where the launch is about one round of the chip: expand + depthwise + project per launch)"
                       if mid else "fused_ir_kernel (features[1..7], expand + depthwise + project per launch)"), "bound": "hbm",
            "achieved": round(byts / ms / 1e6, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
            "frac": round(byts / ms / 1e6 / PEAK_HBM_GBS, 4), "traffic": None,
            "launches_per_step": sum(g["launches"] for g in fu.values()), "fused_floor_mb_per_step": round(byts / 1e6, 3),
            "kernel_ms_per_step": round(ms, 4), "tflops_fp32": round(fl / ms / 1e9, 2),
            "instances": {k: {"launches": g["launches"], "ms": round(g["ms"], 4), "fused_floor_mb": round(g["bytes"] / 1e6, 3),
                              "frac_hbm": round(g["bytes"] / g["ms"] / 1e6 / PEAK_HBM_GBS, 4), "tflops_fp32": round(g["flops"] / g["ms"] / 1e9, 2)}
                          for k, g in sorted(fu.items(), key=lambda kv: -kv[1]["ms"])},
            "note": "unfused, the same seven blocks move %.0f MB per step" % (sum(g.get("unfused_bytes", 0.0) for g in fu.values()) / 1e6)}


def dwproj_family(groups, prec):
    """Depthwise -> projection launches with the LDS halo tile (the dwBlocks of the head / decoder): D never reaches
    HBM.  MFMA-bound (fp32 matrix peak) with the depthwise's FLOPs counted; fused-floor bytes (E read + output)
    beside it."""
    fu = {k: g for k, g in groups.items() if k.startswith("dwproj_kernel")}      # (template arguments: precision, tile, producer waves)
    if not fu:
        return None
    byts = sum(g["bytes"] for g in fu.values())
    ms = sum(g["ms"] for g in fu.values())
    fl = sum(g["flops"] for g in fu.values())
    return {"kernel": "dwproj_kernel (depthwise 3x3 + projection per launch, LDS halo)", "bound": "mfma",
            "achieved": round(fl / ms / 1e9, 2), "peak": round(PEAK_TFLOPS[prec], 1), "unit": "TFLOP/s",
            "frac": round(fl / ms / 1e9 / PEAK_TFLOPS[prec], 4), "traffic": None,
            "launches_per_step": sum(g["launches"] for g in fu.values()), "fused_floor_mb_per_step": round(byts / 1e6, 3),
            "kernel_ms_per_step": round(ms, 4), "hbm_gbs": round(byts / ms / 1e6, 1),
            "instances": {k: {"launches": g["launches"], "ms": round(g["ms"], 4)} for k, g in fu.items()}}


def reference_shape(model, args, device, H, W, n, time_dims, surface, with_cpu):
    """One of the reference's own call shapes on the HIP path: frames/s over the same timed windows as the headline, first
    call of the new shape, parity and speed of the CPU oracle on the same inputs."""
    from iip_uavsal_saliency_amd import synth
    h, w = H // 8, W // 8
    x = torch.from_numpy(synth.normalize_frames(synth.synth_frames_u8(n, H, W, 0)))
    cb = [torch.from_numpy(synth.gauss_priors(n, h, w)), torch.from_numpy(synth.ob_priors(n, h, w, seed=0))]
    xd, cbd = x.to(device), [cb[0].to(device), cb[1].to(device)]
    model.time_dims = time_dims
    if surface == "forward":            # UAVSal.forward(x [B*T,3,H,W], cb, [state]) as Demo_Test.py:85 calls it
        st0 = torch.zeros((1, 256, h, w), device=device)
        fn = lambda: model(xd, cbd, [st0])
    else:
        xc, cbc = xd[None], [cbd[0][None], cbd[1][None]]
        fn = lambda: model.forward_clips(xc, cbc, None)
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    out, _ = fn()
    torch.cuda.synchronize(device)
    first = (time.perf_counter() - t0) * 1e3
    wins = [timed_steps(fn, args.steps, args.warmup if i == 0 else 0, False, device) for i in range(max(1, args.windows))]
    dt = sorted(wins)[len(wins) // 2]
    rec = {"workload": "%dx%d, %d frames, time_dims=%d, UAVSal.%s, prec=%s" % (H, W, n, time_dims, surface, args.prec),
           "value": round(n * args.steps / dt, 2), "unit": "frames/s", "ms_per_call": round(dt / args.steps * 1e3, 4),
           "windows_ms_per_call": [round(w_ / args.steps * 1e3, 4) for w_ in wins], "steps": args.steps,
           "first_call_ms": round(first, 1),
           "note": "forward() waits for its own launches before returning (the reference's caller reads the map at once, Demo_Test.py:87)"
           if surface == "forward" else "forward_clips: asynchronous, as the headline"}
    if with_cpu:
        from oracle.uavsal_ref import build_oracle       # checker / baseline only
        oracle = build_oracle(time_dims=time_dims, seed=0)
        t0 = time.perf_counter()
        ref, _ = oracle(x, cb, None)
        cpu_s = time.perf_counter() - t0
        rec["max_abs_map_vs_cpu_ref"] = float("%.3e" % (out.reshape(ref.shape).cpu() - ref).abs().max().item())
        rec["cpu_oracle_frames_per_s"] = round(n / cpu_s, 3)
        rec["cpu_oracle_sample"] = "one pass of the same %d frames on %d host threads (%.1f s)" % (n, torch.get_num_threads(), cpu_s)
    return rec


def timed_steps(fn, steps, warmup, distributed, device):
    for _ in range(warmup):
        fn()
    if distributed:
        dist.barrier()
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize(device)
    if distributed:
        dist.barrier()
    dt = time.perf_counter() - t0
    if distributed:
        t = torch.tensor([dt], dtype=torch.float64, device="cpu" if dist.get_backend() == "gloo" else device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    return dt


def visible_gpus():
    """GPUs this process could use, counted WITHOUT a HIP call: the visibility variables first, else the KFD topology
    (/sys/class/kfd/kfd/topology/nodes/*/properties: a node with simd_count > 0 is a GPU).  Only when neither can be read
    does it fall back to torch.cuda.device_count(), which on this image may call hipGetDeviceCount (amdsmi absent) -- that is
    harmless here because the launcher never execs and never runs under rocprofv3: its ranks are fresh child processes.
    `UAVSAL_BENCH_VISIBLE_GPUS` overrides the count for the CPU test of the launcher."""
    if "UAVSAL_BENCH_VISIBLE_GPUS" in os.environ:
        return int(os.environ["UAVSAL_BENCH_VISIBLE_GPUS"])
    for var in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            return len([t for t in v.split(",") if t.strip() != ""])
    base = "/sys/class/kfd/kfd/topology/nodes"
    try:
        n = 0
        for node in os.listdir(base):
            for line in open(os.path.join(base, node, "properties")):
                k, _, val = line.partition(" ")
                if k == "simd_count" and int(val) > 0:
                    n += 1
        return n
    except (OSError, ValueError):
        return int(torch.cuda.device_count())


def self_launch(n, argv, worker=None, poll_s=0.2, deadline_s=None):
    """`python bench.py --gpus N` without a launcher around it: start N fresh rank processes of this script (one per
    GPU, RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT set, rendezvous on 127.0.0.1), let rank 0's JSON line
    through on stdout, and return non-zero if any rank fails (the surviving ranks are stopped by PID: they would wait in
    a collective for ever).  Fails loudly when fewer than N GPUs are visible -- it never measures a smaller job.
    `worker`: the command to run per rank (default: this script with the same arguments); tests pass a stub.
    `deadline_s` (default `UAVSAL_BENCH_DEADLINE_S`, 3000): wall-clock limit for the whole job -- ranks stuck in a collective
    or on a hung GPU never exit by themselves; on expiry the ranks still alive are named, stopped by PID, and the launcher
    returns 124."""
    import socket
    import subprocess
    have = visible_gpus()
    if "--rehearse-on-one-gpu" in argv:
        have = n if have >= 1 else 0           # every rank uses cuda:0 (see --rehearse-on-one-gpu)
    if have < n:
        print("bench.py: --gpus %d asked for but only %d GPU(s) visible; not measuring a smaller job" % (n, have),
              file=sys.stderr, flush=True)
        return 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = list(worker) if worker else [sys.executable, os.path.abspath(__file__)] + list(argv)
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), UAVSAL_BENCH_SELF_LAUNCHED="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # dmabuf IPC only on this driver (RCCL needs it)
        procs.append(subprocess.Popen(cmd, env=env))
    failed = None
    live = set(range(n))
    if deadline_s is None:
        deadline_s = float(os.environ.get("UAVSAL_BENCH_DEADLINE_S", "3000"))
    t_end = time.monotonic() + deadline_s
    while live and failed is None:
        if time.monotonic() > t_end:
            failed = (-1, 124)
            break
        for r in sorted(live):
            rc = procs[r].poll()
            if rc is None:
                continue
            live.discard(r)
            if rc != 0:
                failed = (r, rc)
                break
        if live and failed is None:
            time.sleep(poll_s)
    if failed is not None:
        for r in sorted(live):
            procs[r].terminate()
        for r in sorted(live):
            try:
                procs[r].wait(timeout=20)
            except subprocess.TimeoutExpired:
                procs[r].kill()
                procs[r].wait()
        if failed[0] < 0:
            print("bench.py: no result after %.0f s; rank(s) %s were still running and have been stopped" % (deadline_s, sorted(live)),
                  file=sys.stderr, flush=True)
            return 124
        print("bench.py: rank %d exited with code %d; %d other rank(s) stopped" % (failed[0], failed[1], len(live)),
              file=sys.stderr, flush=True)
        return failed[1] if 0 < failed[1] < 256 else 1
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--clips", type=int, default=0, help="clips per GPU; default 1 on one GPU (BASELINE configs[1]) "
                    "and 8 per GPU when --gpus > 1 (configs[3]: 8 clips/GPU); pass --clips 8 --gpus 1 for the "
                    "matching single-GPU point of a scaling curve")
    ap.add_argument("--windows", type=int, default=None, help="timed windows of --steps steps each; the median is reported "
                    "(default 1, with --full 3)")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=360)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--prec", default="f32", choices=["f32", "f16x3", "bf16x3", "bf16"])
    ap.add_argument("--graph", type=int, default=0, help="1: replay the launch plan as one hipGraph (measured slower "
                    "than the native launch loop on ROCm 7.2: 1227-1247 vs 1268-1288 frames/s)")
    ap.add_argument("--lanes", type=int, default=1, help="run independent branches on parallel streams / graph branches")
    ap.add_argument("--fuse-dw", type=int, default=-1, help="-1 engine default, 0/1 force the fused depthwise->projection GEMM")
    ap.add_argument("--stream-k", type=int, default=1, help="fp32 GEMMs: stream-K when whole tiles would idle CUs")
    ap.add_argument("--presplit", type=int, default=-1, help="f16x3: producers also write split shadows and the eligible GEMMs "
                    "stage both operands by LDS-DMA (0: every GEMM re-splits its fp32 input while staging)")
    ap.add_argument("--fuse-blocks", type=int, default=1, help="features[1..7] as one fused launch per block (0: three launches)")
    ap.add_argument("--sync-errors", type=int, default=-1, help="-1: model default (forward_clips is asynchronous: device errors "
                    "poison the outputs and raise at the next call); 1: wait for every call's launches and raise before returning")
    ap.add_argument("--persistent-state", type=int, default=0, help="1: BASELINE configs[4]'s mode -- the recurrent state stays in the "
                    "engine's HBM buffer between steps (model.persistent_state) and every step continues from the previous one's state; "
                    "0: every step gets a caller-owned state tensor (staged NCHW -> NHWC, returned as a fresh NCHW tensor)")
    ap.add_argument("--inflight", type=int, default=1, help="N > 1: the K steps are issued through stream.RequestPipeline, N independent requests "
                    "in flight on N host streams / lane-less model handles (per-request results bitwise unchanged; one GPU, caller-owned state).  "
                    "NOT the default: `value` of `python bench.py` is one request at a time; the same figure is in its `extra_two_requests_in_flight`")
    ap.add_argument("--rehearse-on-one-gpu", action="store_true", help="with --gpus N: the N ranks all use cuda:0 and rendezvous over gloo "
                    "(maps gathered through the host).  NOT a measurement of anything -- it runs the launcher, the rank environment, the "
                    "clip partition, the gather and the barrier-bracketed timing with the HIP engine on a one-GPU box; the line says so")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-extra", action="store_true")
    ap.add_argument("--full", action="store_true", help="also measure and check what the headline does not need: per-kernel "
                    "rooflines, the CPU oracle baseline and parity, the scaling reference, the reference's shapes and the extras "
                    "(--no-roofline / --no-cpu-baseline / --no-extra leave parts out)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the maps and the state the last timed step "
                    "returned as DIR/<name>.npy (float32; a fixed, seeded sample when they exceed 60 MB together)")
    args = ap.parse_args()
    if not args.full:
        args.no_cpu_baseline = args.no_roofline = args.no_extra = True
    if args.windows is None:
        args.windows = 3 if args.full else 1

    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # started the way the one-GPU bench is (no torch.distributed.run around it): become the launcher.  Nothing in
        # this process has touched the GPU yet (device_count() does not initialise HIP on this image)
        raise SystemExit(self_launch(args.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    distributed = world > 1
    if args.gpus != world:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d: refusing to measure a different job than the one asked for"
                         % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X; there is no CPU path to measure")
    rehearsal = bool(args.rehearse_on_one_gpu) and distributed
    device = torch.device("cuda", 0 if rehearsal else local_rank)
    torch.cuda.set_device(device)
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rehearsal:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)

    from iip_uavsal_saliency_amd import UAVSal, synth
    from iip_uavsal_saliency_amd.parallel import ClipShard, gather_maps

    if args.clips <= 0:
        args.clips = 8 if world > 1 else 1
    C, T, H, W = args.clips, args.frames, args.height, args.width
    h, w = H // 8, W // 8
    shard = ClipShard(total_clips=C * world, world_size=world, rank=rank)
    model = UAVSal(time_dims=T, precision=args.prec)
    synth.load_synth_weights(model, 0)
    model = model.to(device).eval()
    model.use_graph = bool(args.graph)
    model.fuse_dw = None if args.fuse_dw < 0 else bool(args.fuse_dw)
    model.use_lanes = bool(args.lanes)
    model.stream_k = bool(args.stream_k)
    model.presplit = None if args.presplit < 0 else bool(args.presplit)
    model.fuse_blocks = bool(args.fuse_blocks)
    model.sync_errors = None if args.sync_errors < 0 else bool(args.sync_errors)
    model.persistent_state = bool(args.persistent_state)

    x_cpu, cb_cpu = make_clips(C, T, H, W, seed=shard.first)       # this rank's clips
    x = x_cpu.to(device)
    cb = [cb_cpu[0].to(device), cb_cpu[1].to(device)]
    state = torch.zeros((C, 256, h, w), device=device)
    gathered = torch.empty((C * world, T, 1, h, w), device=device) if distributed else None
    last = {}

    pipe = None
    if args.inflight > 1:
        if distributed or args.persistent_state or args.graph:
            raise SystemExit("--inflight N > 1 is a one-GPU, launch-loop, caller-owned-state measurement")
        from iip_uavsal_saliency_amd.stream import RequestPipeline
        pipe = RequestPipeline(model, streams=args.inflight)

    def step():
        if pipe is not None:      # independent requests (zero state each), N in flight; timed_steps synchronises the whole device
            last["out"], last["state"], _ = pipe.forward_clips(x, cb, state)
            return
        # persistent mode: continue from the state the previous step left in HBM (recognised by address: no copy)
        out, st = model.forward_clips(x, cb, last.get("state", None) if args.persistent_state else state)
        if distributed:
            gather_maps(out, gathered)
        last["out"], last["state"] = out, st

    # first-call latency: weight packing (BN folding, GEMM / Winograd layouts, upload) + sizing pass + plan recording + the
    # first launches.  Demo_Test.py:75-86 pays it once per video shape -- and once more (plan only) for a short last group
    torch.cuda.synchronize(device)
    t_first = time.perf_counter()
    for _ in range(max(1, args.inflight)):          # (every in-flight handle records its plan)
        step()
    torch.cuda.synchronize(device)
    first_call_ms = (time.perf_counter() - t_first) * 1e3
    log("model + inputs ready (first call %.0f ms); timing %d steps" % (first_call_ms, args.steps))
    # every window is exactly --steps steps between barrier + synchronize on both sides (max over ranks);
    # the median window is the reported one, all of them are listed
    wins = [timed_steps(step, args.steps, args.warmup if i == 0 else 0, distributed, device)
            for i in range(max(1, args.windows))]
    dt = sorted(wins)[len(wins) // 2]
    log("timed region done: %.3f ms/step (windows: %s)" % (dt / args.steps * 1e3,
                                                           ", ".join("%.3f" % (w / args.steps * 1e3) for w in wins)))
    if args.dump_outputs and rank == 0:
        # what a caller of the timed path holds after its last step: the maps (all ranks' after the gather) and the state
        names = dump_outputs(args.dump_outputs, {"maps": gathered if distributed else last["out"], "state": last["state"]})
        log("outputs of the last timed step written to %s: %s" % (args.dump_outputs, ", ".join(names)))
    frames = C * T * world * args.steps
    fps = frames / dt
    result = {
        "metric": "saliency frames/sec at 360x640" if (H, W) == (360, 640) else "saliency frames/sec at %dx%d" % (H, W),
        "value": round(fps, 2), "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(dt / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
        "windows_ms_per_step": [round(w / args.steps * 1e3, 4) for w in wins],
        "vs_baseline": None, "dtype": DTYPE_NAME[args.prec], "data": "synthetic",
        "config": {"workload": "%dx%d batch=%d clip(s)/GPU seq=%d, UAVSal.forward_clips, prec=%s, %s%s" % (
            H, W, C, T, args.prec, "hipGraph replay" if args.graph else "launch loop",
            ", %d independent requests in flight (stream.RequestPipeline)" % args.inflight if pipe is not None else ""),
            "requests_in_flight": max(1, args.inflight),
            "clips_per_gpu": C, "seq_len": T, "height": H, "width": W, "precision": args.prec,
            "persistent_state": bool(args.persistent_state),
            "parallelism": "clip-sharded x%d, one all-gather of maps per step" % world if distributed else "single GPU"},
    }

    result["ranks_seen"] = dist.get_world_size() if distributed else 1
    if pipe is not None and args.full:
        pipe.synchronize()
        so, ss = model.forward_clips(x, cb, state)
        result["bit_identical_to_one_at_a_time"] = bool(torch.equal(last["out"], so) and torch.equal(last["state"], ss))
    if rehearsal:
        result["n_gpus"] = 1
        result["rehearsal"] = ("%d ranks SHARING one GPU over gloo (maps gathered through the host): exercises launcher, rank env, clip "
                               "partition, gather and timing protocol only; value is NOT a multi-GPU figure" % world)
        result["config"]["parallelism"] = "REHEARSAL: %d ranks on one GPU, gloo" % world
    result["peak_device_memory_mb"] = round(torch.cuda.max_memory_allocated(device) / 1e6, 1)      # weights + plan buffers + inputs
    result["first_call_ms"] = round(first_call_ms, 1)
    result["first_call_note"] = "weight packing + upload + plan sizing / recording + first launches of this workload (one per model and shape)"
    try:
        eng0 = list(model._engines.values())[-1]
        result["activation_arena"] = dict({k: round(v, 1) if isinstance(v, float) else v for k, v in eng0.arena_stats.items()},
                                          note="one pool per plan placed by liveness; unshared_mb = one allocation per activation (rounds 1-4)")
    except Exception:
        pass
    if distributed and not args.no_extra:
        # the like-for-like origin of the weak-scaling curve, in the line itself: the SAME per-GPU workload on rank 0's GPU
        # alone (no gather, the other ranks wait in the barrier), and value / (N x that)
        dist.barrier()
        if rank == 0:
            ks = max(3, args.steps // 4)
            dt1 = timed_steps(lambda: model.forward_clips(x, cb, state), ks, 1, False, device)
            one = C * T * ks / dt1
            result["scaling_reference"] = {
                "workload": "%dx%d batch=%d clip(s) seq=%d, prec=%s on ONE GPU (rank 0 alone, other ranks idle)" % (H, W, C, T, args.prec),
                "value": round(one, 2), "unit": "frames/s", "n_gpus": 1, "steps": ks,
                "efficiency": round(fps / (world * one), 4)}
        dist.barrier()

    if rank == 0 and world == 1:
        eng = model._engine(device, C, T, H, W, "clip", False, torch.float32)
        result["config"]["fused_dw"] = sum(1 for m in eng.ops_meta if m.get("fused_dw"))    # launches with the depthwise inside
        if not args.no_roofline:
            log("per-kernel hipEvent timing of %d launches" % len(eng.ops_meta))
            groups = kernel_rooflines(eng, args.prec)
            tot = sum(g["ms"] for g in groups.values())
            dom = max(groups.items(), key=lambda kv: kv[1]["ms"])
            result["roofline"] = roofline_obj(dom[0], dom[1], args.prec)
            result["roofline"]["share_of_kernel_time"] = round(dom[1]["ms"] / tot, 3)
            result["roofline"]["traffic"], result["roofline"]["traffic_source"] = measured_traffic(dom[0], C, T, H, W, args.prec)
            result["roofline"]["timing"] = PER_OP_TIMING
            result["per_op_timing"] = PER_OP_TIMING
            il = in_loop_timing(dom[0], C, T, H, W, args.prec)
            if il.get("status") == "ok":       # the same launches inside the overlapped timed loop (rocprofv3 average)
                per_launch = dom[1]["flops"] / dom[1]["launches"]
                il["achieved"] = round(per_launch / (il["avg_launch_us"] * 1e-6) / 1e12, 2)
                il["frac"] = round(il["achieved"] / PEAK_TFLOPS[args.prec], 4)
            result["roofline"]["in_loop"] = il
            result["roofline"]["clock_note"] = ("peak is the 2.4 GHz figure; under these GEMMs the chip holds 2.0-2.15 GHz "
                                                "(in-kernel s_memtime / s_memrealtime, profiles/r3_gemm_k32.md)")
            fam = depthwise_family(groups)
            if fam:
                fam["share_of_kernel_time"] = round(fam["kernel_ms_per_step"] / tot, 3)
                big = "dw3x3_kernel<1, 4, 4>"
                if big in fam["instances"]:
                    fam["instances"][big]["traffic"], _ = measured_traffic(big, C, T, H, W, args.prec)
                fam["in_loop"] = family_in_loop(fam, C, T, H, W, args.prec)
                fam["in_loop_lanes_off"] = family_in_loop(fam, C, T, H, W, args.prec, lanes0=True)
                fam["timing"] = PER_OP_TIMING
                result["roofline_dw"] = fam
            dots = {k: g for k, g in groups.items() if g["kind"] == "dw_dot"}
            for k, g in dots.items():
                # the decoder's depthwise 3x3 + one-channel projection launch: a depthwise conv whose output is a dot product per pixel
                # (bytes: the expanded tensor once + one float per pixel); reported by itself, NOT inside the stand-alone family above
                # (whose members write C channels per pixel and are comparable with the earlier rounds)
                result["roofline_dw_dot"] = roofline_obj(k, g, args.prec)
                result["roofline_dw_dot"]["share_of_kernel_time"] = round(g["ms"] / tot, 3)
                result["roofline_dw_dot"]["traffic"], _ = measured_traffic(k, C, T, H, W, args.prec)
            fus = fused_family(groups)
            if fus:
                fus["share_of_kernel_time"] = round(fus["kernel_ms_per_step"] / tot, 3)
                result["roofline_fused"] = fus
            fmid = fused_family(groups, mid=True)
            if fmid:
                fmid["share_of_kernel_time"] = round(fmid["kernel_ms_per_step"] / tot, 3)
                fmid["frac_mfma"] = round(fmid["tflops_fp32"] / PEAK_TFLOPS["f32"], 4)
                ex = sum(g["flops_executed"] for k, g in groups.items() if k.startswith("fused_mid"))
                fmid["tflops_executed"] = round(ex / fmid["kernel_ms_per_step"] / 1e9, 2)
                fmid["frac_mfma_executed"] = round(fmid["tflops_executed"] / PEAK_TFLOPS["f32"], 4)
                fmid["executed_note"] = ("MFMA flops the kernel issues: a 4 x 8 output patch expands its whole 6 x 10 halo (64 rows for 32 "
                                         "outputs) and 23 rows are covered by 6 patch rows -- 1.5-1.57 x the block's own flops; "
                                         "tflops_fp32 / frac_mfma count the block's flops only")
                result["roofline_fused_mid"] = fmid
            dwp = dwproj_family(groups, args.prec)
            if dwp:
                dwp["share_of_kernel_time"] = round(dwp["kernel_ms_per_step"] / tot, 3)
                for inst, rec in dwp["instances"].items():       # measured HBM bytes per launch beside the fused-floor bytes
                    rec["traffic"], _ = measured_traffic(inst, C, T, H, W, args.prec)
                    rec["fused_floor_mb_per_launch"] = round(groups[inst]["bytes"] / groups[inst]["launches"] / 1e6, 3)
                result["roofline_dwproj"] = dwp
            result["kernel_time_ms"] = {k: round(v["ms"], 4) for k, v in sorted(groups.items(), key=lambda kv: -kv[1]["ms"])}
            result["stage_time_ms"] = {}
            for k, (a, b) in eng.stage_ranges.items():
                eng.run_ops(0, a)
                result["stage_time_ms"][k] = round(eng.time_ops(a, b, 5), 4)
        if not args.no_cpu_baseline:
            # the parity check below compares a fresh zero-state call (the per-op timing above re-ran single launches of the plan
            # into the last step's output tensors)
            model.persistent_state = False
            last["out"], last["state"] = model.forward_clips(x, cb, state)
            model.persistent_state = bool(args.persistent_state)
            from oracle.uavsal_ref import build_oracle       # checker / baseline only
            cores = host_cores()
            torch.set_num_threads(cores)
            log("cpu baseline: oracle on %d host threads" % cores)
            oracle = build_oracle(time_dims=T, seed=0)
            xc, cbc = x_cpu[:1], [cb_cpu[0][:1], cb_cpu[1][:1]]
            oracle.forward_clips(xc, cbc)                    # warm-up
            best = 1e30
            for _ in range(3):
                t0 = time.perf_counter()
                ref_out, ref_state = oracle.forward_clips(xc, cbc)
                best = min(best, time.perf_counter() - t0)
                log("cpu baseline pass: %.2f s" % best)
            result["cpu_baseline"] = {"value": round(T / best, 3), "unit": "frames/s", "cores": torch.get_num_threads(),
                                      "kind": "port", "cpu_model": cpu_model(),
                                      "sample": "1 clip x %d frames at %dx%d, best of 3 after 1 warm-up, "
                                      "torch-CPU fp32 oracle (oracle/uavsal_ref.py)" % (T, H, W)}
            torch.set_num_threads(1)                          # also the 1-thread figure
            t0 = time.perf_counter()
            oracle.forward_clips(xc, cbc)
            one = time.perf_counter() - t0
            log("cpu baseline, 1 thread: %.2f s" % one)
            result["cpu_baseline"]["value_1_thread"] = round(T / one, 3)
            result["cpu_baseline"]["sample_1_thread"] = "the same clip once on 1 thread (%.1f s)" % one
            torch.set_num_threads(cores)
            err = (last["out"][:1].cpu() - ref_out).abs().max().item()
            serr = (last["state"][:1].cpu() - ref_state).abs().max().item()
            result["parity"] = {"max_abs_map_vs_cpu_ref": float("%.3e" % err), "max_abs_state_vs_cpu_ref": float("%.3e" % serr),
                                "tolerance": 1e-3}
        if not args.no_extra and C != 8:
            # the single-GPU point of the multi-GPU curve: `--gpus N` (N > 1) runs configs[3]'s 8 clips per GPU,
            # so the matching 1-GPU figure (same per-GPU workload, same precision) is measured here
            log("scaling reference: 8 clips on this GPU, %s" % args.prec)
            x8, cb8 = make_clips(8, T, H, W)
            x8 = x8.to(device)
            cb8 = [cb8[0].to(device), cb8[1].to(device)]
            ks = args.steps
            w8 = [timed_steps(lambda: model.forward_clips(x8, cb8, None), ks, args.warmup if i == 0 else 0, False, device)
                  for i in range(max(1, args.windows))]
            dt8 = sorted(w8)[len(w8) // 2]
            result["scaling_reference"] = {"workload": "%dx%d batch=8 clip(s)/GPU seq=%d, prec=%s (what --gpus N>1 runs per GPU)" % (H, W, T, args.prec),
                                           "value": round(8 * T * ks / dt8, 2), "unit": "frames/s", "n_gpus": 1, "steps": ks,
                                           "ms_per_step": round(dt8 / ks * 1e3, 4),
                                           "windows_ms_per_step": [round(w_ / ks * 1e3, 4) for w_ in w8],
                                           "note": "origin of the weak-scaling curve: an N-GPU line's efficiency is value / (N x this), "
                                                   "NOT value / (N x this line's 1-clip value)"}
            if not args.no_roofline:
                # the depthwise family (north_star: >= 60 % of the HBM roofline) on THIS leg too: at one clip its launches sit on
                # the per-launch floor, at eight clips per GPU (what every GPU of configs[3] runs) they are bandwidth-bound
                eng8 = model._engine(device, 8, T, H, W, "clip", False, torch.float32)
                g8 = kernel_rooflines(eng8, args.prec, iters=5)
                fam8 = depthwise_family(g8)
                if fam8:
                    fam8["workload"] = result["scaling_reference"]["workload"]
                    fam8["share_of_kernel_time"] = round(fam8["kernel_ms_per_step"] / sum(g["ms"] for g in g8.values()), 3)
                    fam8["in_loop"] = family_in_loop(fam8, 8, T, H, W, args.prec)
                    fam8["in_loop_lanes_off"] = family_in_loop(fam8, 8, T, H, W, args.prec, lanes0=True)
                    fam8["timing"] = PER_OP_TIMING
                    result["scaling_reference"]["roofline_dw"] = fam8
                fus8 = fused_family(g8)
                if fus8:
                    result["scaling_reference"]["roofline_fused"] = fus8
            del x8, cb8
            model.invalidate_engines()
        if not args.no_extra and (H, W, T, C) == (360, 640, 8, 1):
            # the reference's own shapes, timed (they were parity runs only): the ONE call its caller makes (Demo_Test.py:110-125:
            # batch_size 4 x time_dims 5 -> forward() of 20 frames at 360x640, state carried) and the only speed it publishes
            # (README.md:104: 288x512, "85FPS", hardware not stated).  Each with max-abs vs the CPU oracle on the same inputs
            # and the oracle's own frames/s (one pass, all host threads).  Same model object: weights are packed already, so
            # `first_call_ms` here is what a second shape costs (plan sizing + recording + first launches)
            for tag, (h2, w2, n2, td, surface) in (("extra_demo_default", (360, 640, 20, 5, "forward")),
                                                   ("extra_288x512", (288, 512, 8, 8, "forward_clips"))):
                try:
                    log("%s: %d frames at %dx%d through %s" % (tag, n2, h2, w2, surface))
                    result[tag] = reference_shape(model, args, device, h2, w2, n2, td, surface, not args.no_cpu_baseline)
                except Exception as e:
                    result[tag] = {"error": repr(e)[:300]}
            model.time_dims = T
            model.invalidate_engines()
        if not args.no_extra and args.prec == "f32":
            # the same workload, and BASELINE.json's configs[2] shape, in the split-fp16 precision
            # (fp32-class: held to the 5e-4 parity bound by tests/test_hip_e2e.py); informative only
            log("extra: f16x3 at 1 and 8 clips")
            try:
                m2 = UAVSal(time_dims=T, precision="f16x3")
                synth.load_synth_weights(m2, 0)
                m2 = m2.to(device).eval()
                extra = {"precision": "f16x3 (3x f16 split MFMA, f32 accumulate)", "unit": "frames/s"}
                ksteps = max(5, args.steps // 2)
                for c2 in (1, 8):
                    x8, cb8 = make_clips(c2, T, H, W)
                    x8 = x8.to(device)
                    cb8 = [cb8[0].to(device), cb8[1].to(device)]
                    dt8 = timed_steps(lambda: m2.forward_clips(x8, cb8, None), ksteps, 2, False, device)
                    extra["%dx%d batch=%d seq=%d" % (H, W, c2, T)] = round(c2 * T * ksteps / dt8, 2)
                    if c2 == 1 and "cpu_baseline" in result:
                        o1, _ = m2.forward_clips(x8, cb8, None)
                        extra["max_abs_map_vs_cpu_ref"] = float("%.3e" % (o1.cpu() - ref_out).abs().max().item())
                result["extra"] = extra
            except Exception as e:  # extra is informative only
                result["extra"] = {"error": repr(e)[:200]}

        if not args.no_extra and C == 1:
            # idle capacity of one forward: the SAME requests, independent of each other, kept two deep in flight on
            # two host streams / model replicas (stream.RequestPipeline).  Informative only -- `value` above is one
            # request at a time
            try:
                from iip_uavsal_saliency_amd.stream import RequestPipeline
                log("extra: two independent requests in flight")
                pipe = RequestPipeline(model, streams=2)
                wp = [timed_steps(lambda: pipe.forward_clips(x, cb, None), args.steps, 4 if i == 0 else 0, False, device)
                      for i in range(max(1, args.windows))]
                pipe.synchronize()
                dtp = sorted(wp)[len(wp) // 2]
                po, ps, _ = pipe.forward_clips(x, cb, None)
                pipe.synchronize()
                so, ss = model.forward_clips(x, cb, None)
                result["extra_two_requests_in_flight"] = {
                    "value": round(C * T * args.steps / dtp, 2), "unit": "frames/s", "precision": args.prec,
                    "ms_per_step": round(dtp / args.steps * 1e3, 4), "steps": args.steps,
                    "windows_ms_per_step": [round(w_ / args.steps * 1e3, 4) for w_ in wp],
                    "bit_identical_to_one_at_a_time": bool(torch.equal(po, so) and torch.equal(ps, ss)),
                    "note": "the SAME requests as `value` (one 8-frame clip, per-frame priors, zero state, exact fp32), independent of each "
                            "other, round-robin on 2 high-priority host streams / lane-less model handles (stream.RequestPipeline); "
                            "windows timed like `value`: barrier-free synchronize on both sides of exactly `steps` requests"}
            except Exception as e:
                result["extra_two_requests_in_flight"] = {"error": repr(e)[:200]}
        if not args.no_extra and (H, W, T, C) == (360, 640, 8, 1):
            # ONE video, the reference's unit of work (Demo_Test.py:65-95: consecutive groups, the recurrent state carried from
            # group to group): 24 groups of 8 uint8 frames through stream.predict_video -- frames normalised in the stem, priors
            # as one broadcast map set, state resident, maps post-processed on the device -- as the reference's loop runs them
            # (one after the other) and with the groups two deep in flight (`overlap=True`: only a group's recurrence waits for the
            # previous group).  Same maps, bit for bit; informative only -- `value` above is one independent request at a time
            try:
                from iip_uavsal_saliency_amd.stream import predict_video
                log("extra: one video of 24 groups x 8 frames, sequential and overlapped")
                u8 = torch.from_numpy(synth.synth_frames_u8(8, H, W, 0)).repeat(24, 1, 1, 1).to(device)
                gp, op_ = cb[0][0, 0], cb[1][0, 0]
                res_v = {}
                for ov in (False, True):
                    predict_video(model, u8[:32], gp, op_, batch_size=1, overlap=ov)          # warm-up (plans, replica)
                    predict_video(model, u8[:32], gp, op_, batch_size=1, overlap=ov)
                    torch.cuda.synchronize(device)
                    t0 = time.perf_counter()
                    sal = predict_video(model, u8, gp, op_, batch_size=1, overlap=ov)
                    torch.cuda.synchronize(device)
                    res_v[ov] = (u8.shape[0] / (time.perf_counter() - t0), sal)
                u8h = u8.cpu().pin_memory()          # the same video from pinned host memory: uploaded group by group on a copy stream
                predict_video(model, u8h[:32], gp, op_, batch_size=1, overlap=True)
                torch.cuda.synchronize(device)
                t0 = time.perf_counter()
                sal_h = predict_video(model, u8h, gp, op_, batch_size=1, overlap=True)
                torch.cuda.synchronize(device)
                fps_h = u8h.shape[0] / (time.perf_counter() - t0)
                result["extra_video_stream"] = {
                    "overlapped_from_host": round(fps_h, 2), "from_host_bit_identical": bool(torch.equal(sal_h, res_v[True][1])),
                    "workload": "one video, %d frames at %dx%d uint8 in groups of %d, state carried, stream.predict_video (incl. device post-processing), prec=%s" % (
                        u8.shape[0], H, W, T, args.prec),
                    "sequential": round(res_v[False][0], 2), "overlapped": round(res_v[True][0], 2), "unit": "frames/s",
                    "bit_identical": bool(torch.equal(res_v[False][1], res_v[True][1])),
                    "note": "overlapped: group k + 1's launches in front of its recurrence run under group k's recurrence and decoder "
                            "(two replicas, two host streams, Engine.run_streamed); priors as one broadcast map set (the caller's form); "
                            "overlapped_from_host: the frames start in pinned host memory (PCIe-inclusive) and are uploaded two groups ahead "
                            "on a copy stream"}
                # the reference's own loop at ITS defaults (Demo_Test.py:110-125: batch_size 4 x time_dims 5 = groups of 20 frames)
                model.time_dims = 5
                model.invalidate_engines()
                try:
                    u5 = u8[:8].repeat(25, 1, 1, 1)             # 200 frames = 10 groups
                    res5 = {}
                    for ov in (False, True):
                        predict_video(model, u5[:40], gp, op_, batch_size=4, overlap=ov)
                        predict_video(model, u5[:40], gp, op_, batch_size=4, overlap=ov)
                        torch.cuda.synchronize(device)
                        t0 = time.perf_counter()
                        sal5 = predict_video(model, u5, gp, op_, batch_size=4, overlap=ov)
                        torch.cuda.synchronize(device)
                        res5[ov] = (u5.shape[0] / (time.perf_counter() - t0), sal5)
                    result["extra_video_stream"]["demo_default_groups_of_20"] = {
                        "workload": "one video, 200 frames in groups of batch_size 4 x time_dims 5 (the reference's defaults), state carried",
                        "sequential": round(res5[False][0], 2), "overlapped": round(res5[True][0], 2),
                        "bit_identical": bool(torch.equal(res5[False][1], res5[True][1]))}
                    del u5, res5
                finally:
                    model.time_dims = T
                    model.invalidate_engines()
                del u8, res_v, u8h
            except Exception as e:
                result["extra_video_stream"] = {"error": repr(e)[:300]}
        if not args.no_extra and (H, W, T, C) == (360, 640, 8, 1):
            # PCIe-inclusive: the boundary of this package takes device tensors, but the reference's caller starts from host frames
            # (Demo_Test.py:78-85: numpy -> normalise -> .to(device)) and reads the maps back (Demo_Test.py:87): the same request with
            # the uint8 frames in pinned host memory copied in per step (5.5 MB; normalisation happens in the stem kernel) and the
            # 8 maps copied back (115 KB), everything on one stream.  Never `value`.
            try:
                log("extra: host frames in, host maps out")
                u8h = torch.from_numpy(synth.synth_frames_u8(T, H, W, 0)).pin_memory()
                maps_h = torch.empty((1, T, 1, h, w), dtype=torch.float32).pin_memory()
                xd8 = torch.empty((1, T, 3, H, W), dtype=torch.uint8, device=device)

                def host_step():
                    xd8[0].copy_(u8h, non_blocking=True)
                    o_, _ = model.forward_clips(xd8, cb, state)
                    maps_h.copy_(o_, non_blocking=True)
                dth = timed_steps(host_step, args.steps, 3, False, device)
                o_dev, _ = model.forward_clips(xd8, cb, state)
                result["extra_host_frames"] = {
                    "value": round(T * args.steps / dth, 2), "unit": "frames/s", "ms_per_step": round(dth / args.steps * 1e3, 4),
                    "max_abs_vs_value_path": float("%.3e" % (o_dev - last["out"]).abs().max().item()),
                    "note": "PCIe-inclusive: uint8 frames from pinned host memory per step (H2D 5.5 MB), normalised in the stem kernel, "
                            "maps copied back to pinned host memory; same stream, asynchronous copies"}
            except Exception as e:
                result["extra_host_frames"] = {"error": repr(e)[:300]}
        if not args.no_extra:
            # the SAME inputs handed over the way priors.get_bias hands them: the synthetic priors -- like the reference caller's
            # (np.repeat of one prior file over the frames, utils_data.py:466-467, 601-602) -- are one map set for every frame; as
            # a zero-stride view the model runs its two prior nets on one frame instead of on all C x T (model.dedupe_priors).
            # `value` above does NOT use this: its priors are materialised per frame, as the reference's caller materialises them
            try:
                if all(bool((c[:, :1] == c).all()) and bool((c[:1] == c).all()) for c in cb):
                    log("extra: priors as one broadcast map set")
                    cbv = [c[:1, :1].expand(C, T, -1, -1, -1) for c in cb]
                    dts = timed_steps(lambda: model.forward_clips(x, cbv, state), args.steps, 3, False, device)
                    ov, _ = model.forward_clips(x, cbv, state)
                    last["out"], _ = model.forward_clips(x, cb, state)
                    result["extra_frame_invariant_priors"] = {
                        "value": round(C * T * args.steps / dts, 2), "unit": "frames/s", "ms_per_step": round(dts / args.steps * 1e3, 4),
                        "max_abs_vs_value_path": float("%.3e" % (ov - last["out"]).abs().max().item()),
                        "note": "same frames and the same prior VALUES, handed over as a zero-stride view of one map set "
                                "(priors.get_bias default): prior nets on 1 frame + broadcast instead of on every frame"}
            except Exception as e:
                result["extra_frame_invariant_priors"] = {"error": repr(e)[:200]}

    if rank == 0:
        print(json.dumps(result), flush=True)
    if distributed:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
