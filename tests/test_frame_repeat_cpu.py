"""Frame repeat, without a device: the entry points exist, are declared in the header and bound with their argument types, the ABI
version is still 20, and a plan without the named pair refuses the call before any HIP call."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from iip_uavsal_saliency_amd import build, _lib
    build.build()
    return _lib.load()


def test_frame_repeat_entry_points_are_declared_and_the_abi_version_stays(lib):
    from iip_uavsal_saliency_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "uavsal_hip.h")).read()
    bound = {s[0]: s for s in _lib.SYMBOLS}
    for name, nargs in (("uavsal_plan_frame_repeat", 6), ("uavsal_plan_frame_repeat_workgroups", 2)):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and len(bound[name][2]) == nargs
    assert lib.uavsal_abi_version() == 20
    assert re.search(r"#define\s+UAVSAL_ABI_VERSION\s+20\b", hdr)


def _recorded_pair(lib, prec, **kw):
    """A native plan that holds just the `fucb.pw` / `fucb.dwpl` descriptors of a plan recorded on the host (nothing is ever
    launched: the addresses are host memory), with (the plan, the recorded engine, the tile of fucb.pw)."""
    import ctypes as C
    import torch
    import mock_plan
    from iip_uavsal_saliency_amd.model import UAVSal
    torch.manual_seed(0)
    m = UAVSal(time_dims=kw["ctx_T"], precision=prec).eval()
    eng, mock = mock_plan.record(m, precision=prec, **kw)
    adds = [c for c in mock.calls if c[0].startswith("uavsal_plan_add_")]
    assert len(adds) == len(eng.ops_meta)
    plan = C.c_void_p(lib.uavsal_plan_create())
    for k, nm in enumerate(("fucb.pw", "fucb.dwpl")):
        name, d = adds[eng._op_idx[nm]]
        assert name == "uavsal_plan_add_conv"
        assert lib.uavsal_plan_add_conv(plan, C.byref(d)) == k
    return plan, eng, eng.ops_meta[eng._op_idx["fucb.pw"]]["tile"]


# The default plan runs `fucb` as expand + depthwise-projection only on maps that fill the kernel's 8 x 16 pixel patches
# (recorder.py: FUSE_DW_MAX_WASTE) with enough work (FUSE_DW_MIN_WORK) -- 45 x 80, 16 x 16; on the small odd maps of the suite
# the block is three launches, which the mode leaves alone, unless `fuse_dw = True` (the tests' switch) asks for the pair.
@pytest.mark.parametrize("case", [
    # (precision, engine arguments, (src_mod, src_div) of ctx.up, expected tile of fucb.pw, armed?)
    ("f32", dict(n_seq=2, seq_len=3, H=72, W=104, ctx_T=3, ctx_mode="clip", fuse_dw=True), (6, 3), 11, 1),
    ("f32", dict(n_seq=1, seq_len=6, H=96, W=160, ctx_T=3, ctx_mode="tile", fuse_dw=True), (2, 1), 11, 1),
    ("f32", dict(n_seq=3, seq_len=8, H=104, W=168, ctx_T=8, ctx_mode="clip", fuse_dw=True), (24, 8), 8, 1),
    ("f32", dict(n_seq=2, seq_len=3, H=128, W=128, ctx_T=3, ctx_mode="clip"), (6, 3), 11, 1),         # default plans from here on
    ("f32", dict(n_seq=1, seq_len=8, H=360, W=640, ctx_T=8, ctx_mode="clip"), (8, 8), 8, 1),          # the headline step
    ("f32", dict(n_seq=1, seq_len=8, H=360, W=640, ctx_T=8, ctx_mode="clip", static_priors=True), (8, 8), 8, 1),
    ("f16x3", dict(n_seq=2, seq_len=3, H=128, W=128, ctx_T=3, ctx_mode="clip"), (6, 3), None, 0),     # no 32-float-K expand
], ids=["clips2x3", "forward6", "clips3x8_tile8", "default_128", "headline", "headline_static", "f16x3"])
def test_frame_repeat_arms_the_recorded_pair_by_its_routes(lib, case):
    prec, kw, (mod, div), tile, armed = case
    plan, eng, got_tile = _recorded_pair(lib, prec, **kw)
    try:
        assert eng._fr == (eng._op_idx["fucb.pw"], eng._op_idx["fucb.dwpl"], mod, div)        # what the engine will ask for
        assert tile is None or got_tile == tile
        assert lib.uavsal_plan_frame_repeat(plan, 0, 1, mod, div, 1) == armed
        assert lib.uavsal_plan_frame_repeat(plan, 0, 1, mod, div, 0) == 0
        n = kw["n_seq"] * kw["seq_len"]
        assert lib.uavsal_plan_frame_repeat(plan, 0, 1, n, 1, 1) == 0            # every frame its own source: nothing to leave out
        assert lib.uavsal_plan_frame_repeat(plan, 0, 1, 2 * n, 1, 1) == 0        # a map that points past the frames
        assert lib.uavsal_plan_frame_repeat(plan, 1, 0, mod, div, 1) == -1
    finally:
        lib.uavsal_plan_destroy(plan)


def test_small_odd_maps_run_the_block_as_three_launches_and_have_no_pair():
    import torch
    import mock_plan
    from iip_uavsal_saliency_amd.model import UAVSal
    torch.manual_seed(0)
    eng, _ = mock_plan.record(UAVSal(time_dims=3).eval(), n_seq=2, seq_len=3, H=72, W=104, ctx_T=3, ctx_mode="clip")
    assert "fucb.dwpl" not in eng._op_idx and "fucb.pl" in eng._op_idx and eng._fr is None


def test_frame_repeat_rejects_ops_that_are_no_pair(lib):
    import ctypes as C
    from iip_uavsal_saliency_amd import _lib as L
    assert lib.uavsal_plan_frame_repeat(None, 0, 1, 1, 1, 1) == -1
    plan = C.c_void_p(lib.uavsal_plan_create())
    try:
        assert lib.uavsal_plan_frame_repeat(plan, 0, 1, 1, 1, 1) == -1            # an empty plan has no op 0 / 1
        assert lib.uavsal_plan_frame_repeat_workgroups(plan, 0) == 0 and lib.uavsal_plan_frame_repeat_workgroups(plan, 2) == -1
        d = L.FillDesc()
        d.out, d.n, d.bits = 4096, 4, 0
        assert lib.uavsal_plan_add_fill(plan, C.byref(d)) == 0 and lib.uavsal_plan_add_fill(plan, C.byref(d)) == 1
        assert lib.uavsal_plan_frame_repeat(plan, 0, 1, 1, 1, 1) == -1            # fills are no conv ops
        assert lib.uavsal_plan_frame_repeat(plan, 1, 0, 1, 1, 0) == -1            # the expand comes first
    finally:
        lib.uavsal_plan_destroy(plan)
