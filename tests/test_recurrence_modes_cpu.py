"""Recurrence modes on the host: the recorded plan is what it was, every seam pair the engine arms is safe in
the planned arena, a forced overlap is refused, and the arena grew by what DESIGN says.  Plans are recorded against the stubs of
tests/mock_plan.py: nothing is launched."""
import json
import os

import pytest

import mock_plan
from iip_uavsal_saliency_amd import UAVSal
from iip_uavsal_saliency_amd.engine import Engine
from tools.recurrence_plan_ops import PLANS, plan_ops

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def headline():
    return mock_plan.record(UAVSal(time_dims=8).eval(), **PLANS["360x640_1x8"])[0]


@pytest.mark.parametrize("key", sorted(PLANS))
def test_recorded_ops_are_the_parents(key):
    """Same ops, names and kinds, in the same order, as the commit in front of the modes recorded (the committed list)."""
    with open(os.path.join(HERE, "golden", "recurrence_plan_ops.json")) as f:
        want = json.load(f)[key]
    assert plan_ops(PLANS[key]) == want


def _overlap(a, b):
    return a is not None and b is not None and a[0] < b[1] and b[0] < a[1]


def test_armed_pairs_are_safe_in_the_planned_arena(headline):
    """The headline plan arms its seven seams, and for each the V planes of step t + 1 overlap nothing the output transform
    of step t reads or writes: M_t, the history, x_t, pre_t, h_{t-1}.  Checked here on the planned offsets, independently of
    the engine's own test."""
    eng = headline
    steps = eng.rec.twa_steps
    assert [s["name"] for s in steps] == ["twa.step%d" % t for t in range(8)]
    assert eng._seams == [(a["xout"], b["xin"]) for a, b in zip(steps, steps[1:])] and len(eng._seams) == 7
    names = [m["name"] for m in eng.ops_meta]
    for t, (xo, xi) in enumerate(eng._seams):
        assert names[xo] == "twa.step%d.xout" % t and names[xi] == "twa.step%d.xin" % (t + 1) and xi == xo + 1
    for a, b in zip(steps, steps[1:]):
        v = b["v"].t
        lo, hi = v.off, v.off + v.numel_
        for k in ("m", "out", "a", "x", "pre"):
            r = a[k].t
            if hasattr(r, "off"):
                assert r.off + r.numel_ <= lo or hi <= r.off, (a["name"], k)
            else:                                    # (the state buffer of step 0 lives outside the arena)
                assert not _overlap(eng._extent(a[k]), eng._extent(b["v"]))
    # the zero state: the state layout (op 0) and the three ops of step 0
    s0 = steps[0]
    assert eng._zs == (names.index("state.in"), names.index("state.in"), s0["xin"], s0["gemm"], s0["xout"])
    assert (names[s0["xin"]], names[s0["gemm"]], names[s0["xout"]]) == ("twa.step0.xin", "twa.step0", "twa.step0.xout")


def test_forced_overlap_is_refused(headline):
    """Move the V planes of step 3 onto M of step 2 in the planned arena: the engine's plan-build check drops that pair and
    keeps the others."""
    eng = headline
    steps = eng.rec.twa_steps
    v, m = steps[3]["v"].t, steps[2]["m"].t
    keep, before = v.off, list(eng._seams)
    try:
        v.off = m.off
        assert eng.seam_conflicts(steps[2], steps[3]) == ["m"]
        eng._plan_recurrence_modes()
        assert eng._seams == [p for p in before if p != (steps[2]["xout"], steps[3]["xin"])] and len(eng._seams) == 6
    finally:
        v.off = keep
        eng._plan_recurrence_modes()
    assert eng._seams == before


@pytest.mark.parametrize("kw,why", [
    (dict(n_seq=4, seq_len=4, H=96, W=160, ctx_T=4, ctx_mode="clip"), "F(4x4) steps"),
    (dict(n_seq=1, seq_len=4, H=96, W=160, ctx_T=4, ctx_mode="tile", precision="f16x3"), "split-precision direct steps"),
    (dict(n_seq=1, seq_len=4, H=96, W=160, ctx_T=4, ctx_mode="tile", use_graph=True), "a graph plan"),
])
def test_plans_that_never_arm(kw, why):
    eng = mock_plan.record(UAVSal(time_dims=4).eval(), **kw)[0]
    assert eng._seams == [] and eng._zs is None, why


def test_debug_plan_arms_no_seam():
    m = UAVSal(time_dims=4).eval()
    m.arena_debug = True
    eng = mock_plan.record(m, n_seq=1, seq_len=4, H=96, W=160, ctx_T=4, ctx_mode="tile")[0]
    assert eng._seams == []


def test_arena_growth_at_one_clip():
    """Keeping what an output transform touches live for one more op costs the headline plan no arena at all: the pool is the
    size the parent planned."""
    e = Engine(UAVSal(time_dims=8).eval(), "cpu", plan_only=True, **PLANS["360x640_1x8"])
    assert round(e.arena_stats["arena_mb"], 2) == ARENA_MB_PARENT + ARENA_GROWTH_MB


ARENA_MB_PARENT = 360.53       # arena_mb of the headline plan at the commit in front of the modes
ARENA_GROWTH_MB = 0.0       # what the modes add to it
