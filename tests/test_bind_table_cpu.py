"""The bind table of a recorded plan (Recorder.binds): `Engine._bind_in_place` re-points exactly the descriptor slots that hold
a caller-side address.  Plans are recorded on the CPU (tests/mock_plan.py), the `uavsal_plan_patch_ptr` calls are the mock's.

The expectation is written out from the ABI comment of `uavsal_plan_patch_ptr` (include/uavsal_hip.h), not read from the table:
a recorder that forgets to register an address fails here, not at the first run on a device."""
import pytest
import torch

import mock_plan
from iip_uavsal_saliency_amd.model import UAVSal, UAVSAL_LSTM

SMALL = dict(H=96, W=160, ctx_T=4)
CONFIGS = {
    "tile": (UAVSal, (1, 1, 1), dict(n_seq=1, seq_len=4, ctx_mode="tile", **SMALL)),
    "lstm-clip": (UAVSAL_LSTM, (1, 1, 1), dict(n_seq=2, seq_len=4, ctx_mode="clip", **SMALL)),
    "uint8": (UAVSal, (1, 1, 1), dict(n_seq=1, seq_len=4, ctx_mode="tile", in_dtype=torch.uint8, **SMALL)),
    "taps": (UAVSal, (1, 1, 1), dict(n_seq=1, seq_len=4, ctx_mode="tile", taps=True, **SMALL)),
    "static": (UAVSal, (1, 1, 1), dict(n_seq=1, seq_len=4, ctx_mode="clip", static_priors=True, **SMALL)),
    "bias000": (UAVSal, (0, 0, 0), dict(n_seq=1, seq_len=4, ctx_mode="tile", **SMALL)),
    "bias101": (UAVSal, (1, 0, 1), dict(n_seq=1, seq_len=4, ctx_mode="tile", **SMALL)),
    "72x104": (UAVSal, (1, 1, 1), dict(n_seq=1, seq_len=3, H=72, W=104, ctx_T=3, ctx_mode="clip")),
}


def _expected(eng, bias, lstm, priors=True):
    """{(op name, slot, caller name, byte offset)} by the ABI: stem 0 = in (fp32) / 1 = in_u8; layout 0 = in, 1 = out; conv (and
    the depthwise-dot tail) 1 = out; guard 0..2 = buf[slot]."""
    exp = {("features.0", 1 if eng.in_dtype == torch.uint8 else 0, "x", 0)}
    if priors:
        exp |= {(op, 0, name, 0) for op, name, on in (("gauss.in", "cb0", bias[0]), ("ob.in", "cb1", bias[1])) if on}
    writers = [r["name"] for r in eng.op_args if getattr(r.get("out"), "buf", None) == "out"]
    assert len(writers) == 1, writers                   # the one op that writes the map
    exp |= {(writers[0], 1, "out", 0), ("guard", 0, "out", 0)}
    per = 4 * 256 * eng.h * eng.w
    for gslot, nm in ((1, "state"), (2, "cstate")) if lstm else ((1, "state"),):
        exp.add((nm + ".in", 0, nm + "_in", 0))
        exp |= {("%s.out%d" % (nm, c), 1, nm + "_out", c * per) for c in range(eng.n_seq)}
        exp.add(("guard", gslot, nm + "_out", 0))
    return exp


def _patched(eng, mock, n0):
    return sorted((eng.ops_meta[a[0]]["name"], a[1], a[2]) for name, a in mock.calls[n0:] if name == "uavsal_plan_patch_ptr")


@pytest.mark.parametrize("cfg", list(CONFIGS), ids=list(CONFIGS))
def test_bind_in_place_patches_what_the_abi_says(cfg):
    cls, bias, kw = CONFIGS[cfg]
    torch.manual_seed(0)
    m = cls(time_dims=4, bias_type=list(bias)).eval()
    eng, mock = mock_plan.record(m, **kw)
    lstm = cls is UAVSAL_LSTM
    N, h, w = eng.N, eng.h, eng.w
    x = torch.zeros(N, 3, eng.H, eng.W, dtype=eng.in_dtype)
    cb0, cb1 = torch.zeros(N, 8, h, w), torch.zeros(N, 20, h, w)
    # (with a recurrent state of the caller's for the ConvLSTM plan, so that its two inputs are two tensors; None elsewhere)
    state, cstate = (torch.zeros(eng.n_seq, 256, h, w), torch.zeros(eng.n_seq, 256, h, w)) if lstm else (None, None)
    n0 = len(mock.calls)
    assert eng._prior_gate((cb0, cb1)) is False          # the first call on these priors: the prior group runs
    with eng.priors.launches():
        out, st = eng._bind_in_place(x, cb0, cb1, state, cstate, lstm)
    assert len(mock.calls) - n0 == len(_patched(eng, mock, n0))          # binding records nothing but patches
    exp = _expected(eng, bias, lstm)
    assert _patched(eng, mock, n0) == sorted((op, slot, eng.bound(name).data_ptr() + off) for op, slot, name, off in exp)

    # Engine.bound: the tensors that were bound, for every name
    assert eng.bound("x").data_ptr() == x.data_ptr() and eng.bound("x").shape == x.shape
    for name, t, on in (("cb0", cb0, bias[0]), ("cb1", cb1, bias[1])):
        if on:
            assert eng.bound(name).data_ptr() == t.data_ptr()
            assert tuple(eng.bound(name).shape) == ((1 if eng.static_priors else N,) + tuple(t.shape[1:]))
        else:
            with pytest.raises(KeyError):
                eng.bound(name)
    assert eng.bound("out") is out and tuple(out.shape) == (N, h * w)
    if lstm:
        assert eng.bound("state_out") is st[0] and eng.bound("cstate_out") is st[1]
        assert eng.bound("state_in").data_ptr() == state.data_ptr() and eng.bound("cstate_in").data_ptr() == cstate.data_ptr()
    else:
        assert eng.bound("state_out") is st and eng.bound("state_in") is eng.zero_state
        with pytest.raises(KeyError):
            eng.bound("cstate_out")
    priors = {k: eng.bound(k) for k in ("cb0", "cb1") if k in exp_names(exp)}

    # the prior group left out: its inputs stay as the remembered call bound them, everything else is bound anew
    n1 = len(mock.calls)
    skip = eng._prior_gate((cb0, cb1))                   # the same prior tensors again
    assert skip is bool(bias[0] or bias[1])              # (a model without prior nets has no group to leave out)
    out2, _ = eng._bind_in_place(x, cb0, cb1, state, cstate, lstm, skip_priors=skip)
    exp2 = _expected(eng, bias, lstm, priors=False)
    assert exp - exp2 == {e for e in exp if e[2] in ("cb0", "cb1")}
    assert _patched(eng, mock, n1) == sorted((op, slot, eng.bound(name).data_ptr() + off) for op, slot, name, off in exp2)
    assert eng.bound("out") is out2 and out2 is not out
    assert all(eng.bound(k) is t for k, t in priors.items())


def exp_names(exp):
    return {e[2] for e in exp}
