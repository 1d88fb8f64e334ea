"""Frame repeat on the MI355X (uavsal_plan_frame_repeat; DESIGN.md "Frame repeat"): when the caller's priors are ONE map set
repeated over the frames, the fusion block behind them (`fucb.pw`, `fucb.dwpl`) computes one frame per clip (`forward_clips`)
or per chunk position (`forward`) on a prior-cache hit and stores it to every frame that repeats it.  Every case is compared
BIT FOR BIT with a second model that has `cache_priors = False` (which never arms the mode), and the workgroup counts of the
two launches say whether the mode ran.

The default plan runs `fucb` as that pair of launches only on maps that fill the depthwise-projection kernel's 8 x 16 pixel
patches with enough work (recorder.py: FUSE_DW_MAX_WASTE, FUSE_DW_MIN_WORK: the 45 x 80 map of the 360 x 640 step, 16 x 16); on
the small odd maps that make GEMM tiles straddle frames -- 9 x 13, 12 x 20, 13 x 21 -- it is three launches, which the mode leaves
alone.  Those sizes therefore run with `fuse_dw = True`, the switch that asks for the pair everywhere (both models of a pair get
it); the 128 x 128 cases and the f16x3 case are default plans, and one case shows the default 72 x 104 plan running in full."""
import pytest
import torch

from iip_uavsal_saliency_amd import synth

pytestmark = pytest.mark.gpu

SIZES = [(72, 104), (96, 160)]       # 9 x 13 = 117 pixels per frame (every GEMM tile straddles frames) / 12 x 20 = 240
SURFACES = ["clips2x3", "clips1x4", "forward6"]      # forward: 6 frames, time_dims 3 -> two chunks, frame k <- chunk k mod 2


def geometry(surface):
    """(clips or None, frames per clip / per call, time_dims)"""
    return {"clips2x3": (2, 3, 3), "clips1x4": (1, 4, 4), "forward6": (None, 6, 3), "clips3x8": (3, 8, 8)}[surface]


def make_inputs(surface, H, W, seed=0, t0=0, expand=False):
    """Frames and priors of a call; the priors are one map set for every frame, as `synth.gauss_priors` / `synth.ob_priors`
    (and the reference's caller) build them: materialised copies, or with `expand` one map set broadcast by stride 0."""
    C, T, _ = geometry(surface)
    n = (C or 1) * T
    h, w = (H + 7) // 8, (W + 7) // 8
    x = torch.from_numpy(synth.normalize_frames(synth.synth_frames_u8(n, H, W, seed, t0))).cuda()
    cb = [torch.from_numpy(synth.gauss_priors(n, h, w)).cuda(), torch.from_numpy(synth.ob_priors(n, h, w, seed=seed)).cuda()]
    assert all(bool((t == t[:1]).all()) for t in cb)
    if expand:
        cb = [t[:1].expand(n, -1, -1, -1) for t in cb]
    if C is not None:
        x = x.view(C, T, 3, H, W)
        cb = [t.view(C, T, *t.shape[1:]) for t in cb]
    return x, cb


_PAIRS = {}


def pair(surface, prec="f32", **attrs):
    """(model with the prior cache, model without) on the same synthetic weights; kept per configuration."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from iip_uavsal_saliency_amd import UAVSal
    key = (geometry(surface)[2], prec, tuple(sorted(attrs.items())))
    if key not in _PAIRS:
        ms = []
        for cache in (True, False):
            m = UAVSal(time_dims=key[0], precision=prec)
            synth.load_synth_weights(m, 0)
            m = m.cuda().eval()
            m.cache_priors = cache
            for k, v in attrs.items():
                setattr(m, k, v)
            ms.append(m)
        _PAIRS[key] = ms
    for m in _PAIRS[key]:
        m.invalidate_priors()
    return _PAIRS[key]


def call(m, surface, x, cb):
    out, st = m.forward_clips(x, cb) if geometry(surface)[0] is not None else m(x, cb)
    return out, (st[0] if isinstance(st, (list, tuple)) else st)


def eng_of(m):
    return list(m._engines.values())[-1]


def same(a, b):
    """maps and state, bit for bit (NaN included)"""
    return all(torch.equal(s.contiguous().view(torch.int32), t.contiguous().view(torch.int32)) for s, t in zip(a, b))


def hit_runs_in_full(mc, mu, surface, x, cb, first_wg):
    """A call of `mc` that is a prior-cache hit and still runs the two launches in full, equal to the uncached model."""
    a, b = call(mc, surface, x, cb), call(mu, surface, x, cb)
    e = eng_of(mc)
    assert e.last_launches() == eng_of(mu).last_launches() - e.prior_group_launches      # a hit ...
    assert not e.repeat_armed and e.repeat_workgroups() == first_wg                      # ... in full
    assert same(a, b)
    return a


def check_armed_calls(surface, H, W, expand=False, tile=None, **attrs):
    mc, mu = pair(surface, **attrs)
    x0, cb = make_inputs(surface, H, W, 0, expand=expand)
    x1, _ = make_inputs(surface, H, W, 0, t0=geometry(surface)[1])
    first = call(mc, surface, x0, cb)
    e = eng_of(mc)
    if tile is not None:
        assert e.ops_meta[e._op_idx["fucb.pw"]]["tile"] == tile
    assert e.static_priors == expand
    full, grp, wg_full = e.last_launches(), e.prior_group_launches, e.repeat_workgroups()
    assert not e.repeat_armed and min(wg_full) > 0 and grp >= 5
    assert same(first, call(mu, surface, x0, cb)) and eng_of(mu).repeat_workgroups() == wg_full
    # second call: a hit, the comparison the miss started is over (the gate has waited for that run), the mode runs
    second = call(mc, surface, x0, cb)
    assert e.repeat_armed and e.last_launches() == full - grp
    wg = e.repeat_workgroups()
    assert 0 < wg[0] < wg_full[0] and 0 < wg[1] < wg_full[1], (wg, wg_full)
    assert same(second, first)                     # x unchanged: the same model's own full call
    # third call, other frames
    third, ref = call(mc, surface, x1, cb), call(mu, surface, x1, cb)
    assert e.repeat_armed and e.repeat_workgroups() == wg and e.last_launches() == full - grp
    assert same(third, ref) and not torch.equal(third[0], first[0])
    assert not eng_of(mu).repeat_armed and eng_of(mu).repeat_workgroups() == wg_full
    # single ops and partial ranges stay full whatever the last call was: fucb.pw by itself, then the block
    i, j = e._op_idx["fucb.pw"], e._op_idx["fucb.dwpl"]
    e.run_ops(i, i + 1)
    e.run_ops(i, j + 1)
    assert e.repeat_workgroups() == wg_full
    assert all(en.streamk_clean() for en in mc._engines.values())
    return e


@pytest.mark.parametrize("surface", SURFACES)
@pytest.mark.parametrize("size", SIZES)
def test_repeated_priors_run_the_fusion_block_once_per_source_frame(size, surface):
    check_armed_calls(surface, *size, fuse_dw=True)


def test_zero_stride_priors_arm_the_static_plan_without_a_comparison():
    e = check_armed_calls("clips2x3", 128, 128, expand=True)
    assert e._prior_rec["same"] is True            # decided from the strides: nothing was compared


def test_the_128_row_tile_of_the_headline_step_straddles_frames():
    """104 x 168 frames: 13 x 21 = 273 pixels, 24 of them: `fucb.pw` takes the 128 x 128 instance that the 360 x 640 step
    runs (tile 8), and no frame starts on a tile boundary."""
    check_armed_calls("clips3x8", 104, 168, tile=8, fuse_dw=True)


def test_default_plan_on_a_map_that_fills_the_patches():
    check_armed_calls("clips2x3", 128, 128, tile=11)


def test_default_plan_with_a_three_launch_block_runs_in_full():
    surface, (H, W) = "clips2x3", SIZES[0]
    mc, mu = pair(surface)
    x, cb = make_inputs(surface, H, W, 6)
    assert same(call(mc, surface, x, cb), call(mu, surface, x, cb))
    assert eng_of(mc)._fr is None and "fucb.pl" in eng_of(mc)._op_idx
    hit_runs_in_full(mc, mu, surface, x, cb, (0, 0))


def test_priors_whose_frames_differ_run_in_full():
    surface, (H, W) = "clips2x3", SIZES[0]
    mc, mu = pair(surface, fuse_dw=True)
    x, cb = make_inputs(surface, H, W, 1)
    cb[1][1, 2, 3, 4, 5] += 0.25                   # one element of one frame, before the first call
    assert same(call(mc, surface, x, cb), call(mu, surface, x, cb))
    wg_full = eng_of(mc).repeat_workgroups()
    hit_runs_in_full(mc, mu, surface, x, cb, wg_full)
    hit_runs_in_full(mc, mu, surface, x, cb, wg_full)


def test_a_frame_edited_in_place_after_a_hit_is_a_miss_and_then_full():
    surface, (H, W) = "forward6", SIZES[0]
    mc, mu = pair(surface, fuse_dw=True)
    x, cb = make_inputs(surface, H, W, 2)
    first = call(mc, surface, x, cb)
    e = eng_of(mc)
    full, wg_full = e.last_launches(), e.repeat_workgroups()
    call(mc, surface, x, cb)
    assert e.repeat_armed
    cb[0][3, 1, 2:4].mul_(0.5)                     # frame 3 no longer equals its source, frame 1: the version counter moves
    a, b = call(mc, surface, x, cb), call(mu, surface, x, cb)
    assert e.last_launches() == full and not e.repeat_armed and e.repeat_workgroups() == wg_full
    assert same(a, b) and not torch.equal(a[0], first[0])
    hit_runs_in_full(mc, mu, surface, x, cb, wg_full)


def test_nan_priors_run_in_full():
    surface, (H, W) = "clips1x4", SIZES[0]
    mc, mu = pair(surface, fuse_dw=True)
    x, cb = make_inputs(surface, H, W, 3)
    cb[1][:, :, 0, 1, 1] = float("nan")            # the same NaN in every frame: bitwise one map set, and still unequal
    assert same(call(mc, surface, x, cb), call(mu, surface, x, cb))
    wg_full = eng_of(mc).repeat_workgroups()
    hit_runs_in_full(mc, mu, surface, x, cb, wg_full)


@pytest.mark.parametrize("attrs", [dict(dedupe_priors=False), dict(use_graph=True)], ids=["no_dedupe", "graph"])
def test_switches_that_keep_the_full_path(attrs):
    surface, (H, W) = "clips2x3", SIZES[0]
    mc, mu = pair(surface, fuse_dw=True, **attrs)
    x, cb = make_inputs(surface, H, W, 4)
    assert same(call(mc, surface, x, cb), call(mu, surface, x, cb))
    e = eng_of(mc)
    wg_full = e.repeat_workgroups()
    for _ in range(2):
        a, b = call(mc, surface, x, cb), call(mu, surface, x, cb)
        assert not e.repeat_armed and e.repeat_workgroups() == wg_full and same(a, b)
    if "dedupe_priors" in attrs:                   # (still a prior-cache hit; a captured graph is never one)
        assert e.last_launches() == eng_of(mu).last_launches() - e.prior_group_launches


def test_f16x3_routes_are_refused():
    surface, (H, W) = "clips2x3", (128, 128)
    mc, mu = pair(surface, prec="f16x3")
    x, cb = make_inputs(surface, H, W, 5)
    assert same(call(mc, surface, x, cb), call(mu, surface, x, cb))
    e = eng_of(mc)
    assert e._fr is not None and e.ops_meta[e._fr[1]]["dwproj"] != 0     # the pair exists; its expand is no 32-float-K GEMM
    wg_full = e.repeat_workgroups()
    hit_runs_in_full(mc, mu, surface, x, cb, wg_full)
    hit_runs_in_full(mc, mu, surface, x, cb, wg_full)
