"""Census of dispatch signatures: which kernel instance and which edge path every launch of a plan takes, per model size.

Which code a launch runs is decided from its shape: `conv_route` (`route_tile` / `pick_tile` / `streamk_plan` / `split_eligible` /
`dwproj_eligible`, csrc/conv_gemm.hip; csrc/conv_route.h), `dw_variant` / `map_lds_slab` / `rowclass_fits` (csrc/dw_conv.hip), the patch shape of the
fused blocks (csrc/fused_ir.hip), and in engine.py the Winograd `r`, the step tile and the fused-block choices.  A *dispatch
signature* (`signature`) is the tuple of everything that selects code or an edge path in one recorded op: the instance, and how
ragged the work lies against that instance's tile (`M % BM`, `Cout % BN`, odd maps under stride 2, maps smaller than a patch).

`census` records plans on the CPU (tests/mock_plan.py: the library's real shape queries, nothing launched) and returns
{signature: [configurations]}.  `DOMAIN` is the set of model sizes, call shapes and precisions the suite answers for; `BASE` the
configurations tests/test_plan_ops_fp64.py walked before the census existed; `WALKS` what it walks in addition so that every
signature of `DOMAIN` is checked launch by launch against float64 (`propose_walks`: cheapest configuration first).
tests/test_plan_census_cpu.py holds the three together; `python tests/plan_census.py` prints the proposal.
"""
import itertools
import os
import sys
import time

import torch

SKIP = ("sync", "poison", "guard")

# block tile (BM, BN) of the GEMM instance a `tile` number names (csrc/conv_gemm.hip: launch_f32 / launch_h16 / launch_variant,
# csrc/conv_gemm_k32.hip)
GEMM_TILE = {1: (128, 128), 2: (128, 64), 3: (128, 32), 4: (64, 64), 5: (128, 256), 6: (256, 256), 7: (256, 128),
             8: (128, 128), 9: (256, 128), 10: (128, 128), 11: (64, 64)}
# output patch (rows, columns) of a thread of the direct depthwise kernels (csrc/dw_conv.hip: dw3x3_kernel<S, TY, TX>)
DW_PATCH = {"dw3x3_kernel<1, 4, 4>": (4, 4), "dw3x3_kernel<1, 2, 2>": (2, 2), "dw3x3_kernel<2, 2, 2>": (2, 2)}
STEM_TILE = (4, 64)                 # csrc/glue.hip: ST_TY x ST_TX output pixels per workgroup
DOT_PATCH = (4, 4)                  # csrc/dw_conv.hip: dw3x3_dot_kernel<4, 4>
FUSED_BIG_MIN = 400                 # csrc/fused_ir.hip: UAVSAL_FUSED_BIG_MIN, launch_fused_shape
ITEMS = 256                         # element-wise kernels: items per workgroup (csrc/glue.hip grid_for, csrc/winograd.hip)


IMG_BUDGET = 96 << 20               # tests/test_plan_ops_fp64.py: float64 elements of an operand above which its images are sampled


def _ragged(n, t):
    return "ragged" if n % t else "full"


def _fused_patch(meta, a, stride):
    """Output patch of the fused block launch (the choice is made inside the launcher, from the shape only: mirrored here)."""
    if meta["kernel"].startswith("fused_mid_kernel"):
        return 4, 8
    ho, wo = (a.h - 1) // stride + 1, (a.w - 1) // stride + 1
    cin, _, cout = (int(s) for s in meta["kernel"].split("<")[1].split(">")[0].split(",")[:3])
    bty = 16 if stride == 1 else 8
    big = a.n * ((ho + bty - 1) // bty) * ((wo + 15) // 16)
    return (bty, 16) if not (cin == 32 and cout == 64) and big >= FUSED_BIG_MIN else (4, 16)


def signature(meta, args):
    """Everything that selects code or an edge path in one recorded op (`Engine.ops_meta[i]`, `Engine.op_args[i]`), as a tuple
    of plain values.  Total: an op kind it does not know raises (only sync / poison / guard have none: `SKIP`)."""
    k = meta["kind"]
    if k in SKIP:
        raise ValueError("%s ops have no dispatch signature" % k)
    if k in ("conv1", "conv3"):
        M, N = meta["M"], meta["Nc"]
        bm, bn = GEMM_TILE[meta["tile"]]
        plane = "triple" in args            # the plane GEMM of a Winograd triple (per-plane weights, M padded to 128 per plane)
        return (k, meta["prec"], "tile%d" % meta["tile"], "presplit" if meta["split"] else "", "streamK" if meta["streamk"] > 0 else "",
                "dwproj%d" % meta["dwproj"] if meta["dwproj"] else "", "fused-dw" if meta.get("fused_dw") else "",
                "wino-planes" if plane else "", "M:" + _ragged(M, bm), "M<tile" if M < bm else "", "N:" + _ragged(N, bn),
                "" if plane else "epi%d" % args["epi"], "groups" if args.get("n_group") else "")
    if k == "dw":
        a, s = args["a"], meta["stride"]
        ho, wo = (a.h - 1) // s + 1, (a.w - 1) // s + 1
        ty, tx = DW_PATCH.get(meta["kernel"], (1, 1))
        dil = args["dilation"]
        return (k, meta["kernel"], "s%d" % s, "shadow-out" if meta.get("split_out") else "",
                "oddH" if s == 2 and a.h % 2 else "", "oddW" if s == 2 and a.w % 2 else "",
                "dil:groups" if isinstance(dil, tuple) else ("dil:1" if dil == 1 else "dil>1"),
                "rows:" + _ragged(ho, ty), "cols:" + _ragged(wo, tx), "map<patch" if ho < ty or wo < tx else "")
    if k == "dw_dot":
        a = args["a"]
        return (k, meta["kernel"], "rows:" + _ragged(a.h, DOT_PATCH[0]), "cols:" + _ragged(a.w, DOT_PATCH[1]),
                "map<patch" if a.h < DOT_PATCH[0] or a.w < DOT_PATCH[1] else "")
    if k == "fused_ir":
        a, s = args["a"], args["blk"].stride
        ho, wo = (a.h - 1) // s + 1, (a.w - 1) // s + 1
        ty, tx = _fused_patch(meta, a, s)
        return (k, meta["kernel"], "patch%dx%d" % (ty, tx), "rows:" + _ragged(ho, ty), "cols:" + _ragged(wo, tx),
                "map<patch" if ho < ty or wo < tx else "", "oddH" if s == 2 and a.h % 2 else "", "oddW" if s == 2 and a.w % 2 else "",
                "res" if args["res"] is not None else "")
    if k in ("wino_in", "wino_out"):
        # (the triple's closing record carries the operands; the input transform's own record names it)
        return (k,) + _wino_part(args, args["cout"]) if k == "wino_out" else (k,)
    if k == "stem":
        a = args["a"]
        ho, wo = (a.h - 1) // 2 + 1, (a.w - 1) // 2 + 1
        return (k, "u8" if args["u8"] else "f32", "rows:" + _ragged(ho, STEM_TILE[0]), "cols:" + _ragged(wo, STEM_TILE[1]),
                "oddH" if a.h % 2 else "", "oddW" if a.w % 2 else "")
    if k == "bilinear":
        a, o = args["a"], args["out"]
        src = "same" if (args["src_mod"], args["src_div"]) == (o.n, 1) else ("mod" if args["src_div"] == 1 else "div")
        return (k, "last:" + _ragged(o.n * o.h * o.w * (a.c // 4), ITEMS), "shadow-out" if o.sp is not None else "", "src:" + src,
                "copy" if (a.h, a.w) == (o.h, o.w) else "resize", "1-pixel-side" if a.h == 1 or a.w == 1 else "")
    if k in ("tdiff", "tsum"):
        o = args["out"]
        return (k, "last:" + _ragged(o.n * o.h * o.w * (args["a"].c // 4), ITEMS))
    if k == "layout":
        v = args["out"] if args["to_nhwc"] else args["a"]
        return (k, "to-nhwc" if args["to_nhwc"] else "to-nchw", "pixels:" + _ragged(v.h * v.w, 32), "chans:" + _ragged(v.c, 32))
    if k == "copy":
        return (k,)
    raise ValueError("op kind %r has no dispatch signature: add it to tests/plan_census.py" % (k,))


def _wino_part(args, c):
    a, r = args["a"], args["r"]
    return ("F%d" % r, "rows:" + _ragged(a.h, r), "cols:" + _ragged(a.w, r),
            "last:" + _ragged(a.n * ((a.h + r - 1) // r) * ((a.w + r - 1) // r) * (c // 4), ITEMS),
            "twa" if args["twa"] is not None else "", "bn" if args["bn"] is not None else "", "act%d" % args["act"])


def plan_signatures(eng):
    """[(op index, op name, signature)] of an engine's recorded plan (device or mock).  The input transform of a Winograd triple
    takes the signature parts of its triple (r, raggedness), which its own record does not carry."""
    out = []
    for i, (meta, args) in enumerate(zip(eng.ops_meta, eng.op_args)):
        if meta["kind"] in SKIP:
            continue
        sig = signature(meta, args)
        if meta["kind"] == "wino_in":
            tr = eng.op_args[eng._op_idx[args["triple"]]]
            sig = sig + _wino_part(tr, tr["cin"])[:4]
        out.append((i, meta["name"], sig))
    return out


def sampled_ops(eng):
    """Names of the ops of a plan that the walk of tests/test_plan_ops_fp64.py checks on a sample of their images (`_images`:
    the operand it sizes an op by exceeds IMG_BUDGET and has more than three images) rather than whole."""
    out = []
    for rec in eng.op_args:
        k = rec["kind"]
        if k in ("conv1", "conv3"):
            d = None if "triple" in rec else (rec["out"] if rec.get("dw") is None else rec["a"])
        elif k in ("wino", "stem", "bilinear", "tsum"):
            d = rec["out"]
        elif k in ("dw", "dw_dot", "fused_ir"):
            d = rec["a"]
        else:
            d = None
        if d is not None and d.n > 3 and d.n * d.h * d.w * max(d.c, 1) > IMG_BUDGET:
            out.append(rec["name"])
    return out


# ---------------------------------------------------------------------------------------------------------- configurations
# A configuration: (clips, frames per clip, H, W, precision, variant).  Variants ("" = none) are the model / call options the
# walks of tests/test_plan_ops_fp64.py use: "static" (frame-invariant priors), "u8" (uint8 frames), "persistent" (resident
# state), "lstm" (ConvLSTM model), "bias101" / "bias000" (prior subsets), "direct-steps" (model.winograd = False).
def cost(cfg):
    c, t, h, w = cfg[:4]
    return c * t * h * w


_models = {}


def model_for(cfg):
    """The (randomly initialised, CPU) model a configuration is recorded with, and the weight cache its plans share."""
    from iip_uavsal_saliency_amd.model import UAVSal, UAVSAL_LSTM
    t, var = cfg[1], cfg[5]
    key = (t, var if var in ("lstm", "bias101", "bias000", "persistent", "direct-steps") else "")
    if key not in _models:
        kw = {"bias101": dict(bias_type=[1, 0, 1]), "bias000": dict(bias_type=[0, 0, 0])}.get(var, {})
        m = (UAVSAL_LSTM if var == "lstm" else UAVSal)(time_dims=t, **kw).eval()
        if var == "persistent":
            m.persistent_state = True
        if var == "direct-steps":
            m.winograd = False
        _models[key] = (m, {})
    return _models[key]


def engine_kwargs(m, cfg):
    """What `model._engine` passes to `Engine` for this configuration."""
    c, t, h, w, prec, var = cfg
    return dict(n_seq=c, seq_len=t, H=h, W=w, ctx_T=t, ctx_mode="tile" if c == 1 else "clip", precision=prec,
                in_dtype=torch.uint8 if var == "u8" else torch.float32, fuse_dw=m.fuse_dw, use_lanes=m.use_lanes,
                stream_k=m.stream_k, persistent=m.persistent_state, static_priors=var == "static")


def record(cfg):
    import mock_plan
    m, wcache = model_for(cfg)
    eng, _ = mock_plan.record(m, wcache=wcache, **engine_kwargs(m, cfg))
    return eng


_sig_cache = {}


def _recorded(cfg):
    if cfg not in _sig_cache:
        eng = record(cfg)
        _sig_cache[cfg] = (frozenset(s for _, _, s in plan_signatures(eng)), tuple(sampled_ops(eng)))
    return _sig_cache[cfg]


def config_signatures(cfg):
    """Signatures of one configuration's plan, recorded on the CPU (no exception is caught: a plan that does not record fails)."""
    return _recorded(cfg)[0]


def config_sampled(cfg):
    """Ops of the configuration's plan that a walk checks on a sample of their images (`sampled_ops`)."""
    return _recorded(cfg)[1]


def census(configs):
    """{signature: [configurations that reach it]} over `configs`."""
    out = {}
    for cfg in configs:
        for s in config_signatures(cfg):
            out.setdefault(s, []).append(cfg)
    return out


# what tests/test_plan_ops_fp64.py walked before the census (its cases A, A', B, C, D, E, F)
BASE = (
    (1, 8, 360, 640, "f32", ""), (1, 8, 360, 640, "f16x3", ""), (1, 8, 360, 640, "bf16x3", ""), (1, 8, 360, 640, "f32", "static"),
    (8, 8, 360, 640, "f32", ""), (8, 8, 360, 640, "f16x3", ""), (8, 8, 360, 640, "f16x3", "direct-steps"),
    (1, 3, 72, 104, "f32", "u8"), (1, 3, 72, 104, "f16x3", ""), (4, 5, 96, 160, "f32", "persistent"),
    (1, 4, 96, 160, "f32", "lstm"), (1, 4, 96, 160, "f16x3", "lstm"), (1, 4, 96, 160, "f32", "bias101"),
    (1, 4, 96, 160, "f16x3", "bias101"), (1, 4, 96, 160, "f32", "bias000"), (1, 4, 96, 160, "f16x3", "bias000"),
    (4, 16, 720, 1280, "f32", ""),
)

SIZES = ((288, 512), (270, 480), (180, 320), (240, 320), (480, 640), (480, 854), (540, 960), (640, 360), (1080, 1920),
         (224, 384), (352, 1216), (256, 256), (100, 100), (360, 644), (64, 64), (32, 32))
CALLS = ((1, 8), (2, 5), (4, 5), (8, 8), (1, 20), (16, 4))          # clips x frames per clip
PRECISIONS = ("f32", "f16x3")

# The sizes x call shapes x precisions the census answers for, and the walked shapes.  It may grow; dropping an entry needs
# a reason written here.  Dropped: nothing.
DOMAIN = tuple((c, t, h, w, p, "") for (h, w), (c, t), p in itertools.product(SIZES, CALLS, PRECISIONS)) + BASE


def propose_walks(domain=DOMAIN, base=BASE):
    """Configurations to walk beside `base` so that every signature of `domain` is walked: a greedy cover, cheapest
    configuration first (cost = clips x frames x H x W) -- a configuration is taken when it reaches a signature that neither
    `base` nor a cheaper one reaches, so a big one appears only where nothing smaller reaches a signature -- and then, most
    expensive first, every pick whose signatures the others cover anyway is dropped again.  Configurations whose every op is
    checked whole (`config_sampled` empty) go first, whatever their cost: one with sampled ops is taken only for a signature
    that no whole one reaches."""
    covered = set().union(*(config_signatures(c) for c in base))
    picks = []
    for cfg in sorted(set(domain) - set(base), key=lambda c: (bool(config_sampled(c)), cost(c), c)):
        new = config_signatures(cfg) - covered
        if new:
            picks.append(cfg)
            covered |= new
    base_sigs = set().union(*(config_signatures(c) for c in base))
    for cfg in sorted(picks, key=lambda c: (-cost(c), c)):
        others = base_sigs.union(*(config_signatures(c) for c in picks if c != cfg))
        if config_signatures(cfg) <= others:
            picks.remove(cfg)
    return picks


# `propose_walks()` as committed (tests/test_plan_census_cpu.py checks that it covers DOMAIN and that no entry is idle)
WALKS = (
    (1, 8, 32, 32, 'f16x3', ''),        # 11 new
    (2, 5, 32, 32, 'f32', ''),        # 3 new
    (1, 20, 100, 100, 'f32', ''),        # 6 new
    (8, 8, 64, 64, 'f16x3', ''),        # 9 new
    (1, 8, 180, 320, 'f16x3', ''),        # 9 new
    (1, 8, 256, 256, 'f16x3', ''),        # 10 new
    (1, 8, 256, 256, 'f32', ''),        # 2 new
    (2, 5, 180, 320, 'f16x3', ''),        # 2 new
    (1, 8, 270, 480, 'f32', ''),        # 9 new
    (4, 5, 180, 320, 'f16x3', ''),        # 4 new
    (2, 5, 270, 480, 'f16x3', ''),        # 3 new
    (2, 5, 270, 480, 'f32', ''),        # 3 new
    (4, 5, 256, 256, 'f16x3', ''),        # 3 new
    (2, 5, 288, 512, 'f16x3', ''),        # 2 new
    (1, 8, 640, 360, 'f32', ''),        # 13 new
    (1, 8, 360, 644, 'f16x3', ''),        # 6 new
    (2, 5, 480, 640, 'f16x3', ''),        # 2 new
    (2, 5, 480, 854, 'f32', ''),        # 13 new
    (8, 8, 256, 256, 'f16x3', ''),        # 4 new
    (8, 8, 256, 256, 'f32', ''),        # 3 new
    (2, 5, 352, 1216, 'f16x3', ''),        # 7 new
    (2, 5, 352, 1216, 'f32', ''),        # 2 new
    (4, 5, 360, 644, 'f16x3', ''),        # 7 new
    (2, 5, 540, 960, 'f16x3', ''),        # 3 new
    (1, 20, 352, 1216, 'f32', ''),        # 1 new
    (4, 5, 352, 1216, 'f16x3', ''),        # 2 new
    (4, 5, 540, 960, 'f16x3', ''),        # 1 new
    (8, 8, 640, 360, 'f16x3', ''),        # 5 new
    (1, 8, 1080, 1920, 'f16x3', ''),        # 3 new
    (1, 8, 1080, 1920, 'f32', ''),        # 1 new
    (8, 8, 480, 640, 'f32', ''),        # 1 new
)


def new_signatures(cfg, walks=None):
    """Signatures of `cfg` that neither `BASE` nor an entry of `WALKS` in front of it reaches: the ones whose first op carries
    the wrong references in `test_dispatch_cover`."""
    walks = WALKS if walks is None else walks
    earlier = BASE + tuple(walks[:walks.index(cfg)])
    return config_signatures(cfg) - set().union(*(config_signatures(c) for c in earlier))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    t0 = time.time()
    base_sigs = set().union(*(config_signatures(c) for c in BASE))
    all_sigs = census(DOMAIN)
    picks = propose_walks()
    print("# %d configurations, %d signatures, %d reached by BASE, %d more by this cover (%.0f s)" % (
        len(DOMAIN), len(all_sigs), len(base_sigs), len(set(all_sigs) - base_sigs), time.time() - t0))
    print("WALKS = (")
    seen = set(base_sigs)
    for cfg in picks:
        n = len(config_signatures(cfg) - seen)
        seen |= config_signatures(cfg)
        print("    %r,        # %d new" % (cfg, n))
    print(")")
    if "-v" in sys.argv:
        for s in sorted(set(all_sigs) - base_sigs, key=str):
            print(s, len(all_sigs[s]), min(all_sigs[s], key=cost))
