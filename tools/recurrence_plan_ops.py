"""Writes the op list -- [index, name, kind] of every recorded op -- of the headline plan (360x640, one clip of 8 frames) and of
the 720x1280 4 x 16 plan, recorded on the CPU against the stubs of tests/mock_plan.py, as JSON.  tests/golden/recurrence_plan_ops.json
is this script's output at the commit in front of the recurrence modes, which must not change the recorded
plan: `python tools/recurrence_plan_ops.py tests/golden/recurrence_plan_ops.json`."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

PLANS = {"360x640_1x8": dict(n_seq=1, seq_len=8, H=360, W=640, ctx_T=8, ctx_mode="clip"),
         "720x1280_4x16": dict(n_seq=4, seq_len=16, H=720, W=1280, ctx_T=16, ctx_mode="clip")}


def plan_ops(kw):
    import mock_plan
    from iip_uavsal_saliency_amd import UAVSal
    eng, _ = mock_plan.record(UAVSal(time_dims=kw["ctx_T"]).eval(), **kw)
    return [[i, m.get("name"), m.get("kind")] for i, m in enumerate(eng.ops_meta)]


if __name__ == "__main__":
    out = {k: plan_ops(kw) for k, kw in PLANS.items()}
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print({k: len(v) for k, v in out.items()})
