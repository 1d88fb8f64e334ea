"""Generate tests/golden/lstm_train_*.npz by running the reference's own ConvLSTM (`model_convlstm.py`: `ConvLSTM`, imported
unmodified) under torch autograd on the CPU, in float64 and in float32.  Run by hand where a checkout of the reference is
available; only the .npz files are committed, and the tests read nothing else.

Per shape (T, H, W) of `lstm_ref64.GOLDEN_SHAPES`, with the seeded inputs of `lstm_ref64.lstm_inputs`:
  1. `ConvLSTM(x, hidden_state=[(h0, c0)])` (the state is passed explicitly: `_init_hidden` calls `.cuda()`; bias=False, one
     layer, as UAVSAL_LSTM builds it) -> the history h_seq;
  2. `G`, the direct gradient of every h_t, back through the recurrence: dW, grad_x, grad_h0, grad_c0 (what
     `train.lstm_backward` returns).
The float32 run is given the same inputs; its gap to float64 is the recurrence's own rounding.

Stored (float64 unless said): `h_seq` on every 64th channel, `grad_x` on every 16th, `grad_h0` and `grad_c0` on every 8th, dW on
`lstm_ref64.DW_SUBSET` plus its sum and L2 norm, the largest magnitude of every tensor, the reference's own
max |fp32 - float64| gap per tensor (over ALL elements), the seed and a digest of the inputs.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_lstm_goldens.py REFERENCE_DIR
"""
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden")

import lstm_ref64 as R                         # noqa: E402

NAMES = ("dW", "grad_x", "grad_h0", "grad_c0")


def run(ref, shape, inp, dtype):
    T, H, W = shape
    rnn = ref.ConvLSTM(input_size=(H, W), input_dim=R.C, hidden_dim=R.C, kernel_size=(3, 3), num_layers=1,
                       batch_first=True, bias=False, return_all_layers=False).to(dtype)
    wt = rnn.cell_list[0].rnn_conv.weight
    with torch.no_grad():
        wt.copy_(torch.as_tensor(inp["w"]).to(dtype))
    x = torch.as_tensor(inp["x"]).to(dtype)[None].requires_grad_(True)
    h0 = torch.as_tensor(inp["h0"]).to(dtype).requires_grad_(True)
    c0 = torch.as_tensor(inp["c0"]).to(dtype).requires_grad_(True)
    out, _ = rnn(x, hidden_state=[(h0, c0)])
    h_seq = out[0]
    gw, gx, g0, gc = torch.autograd.grad(h_seq, (wt, x, h0, c0), torch.as_tensor(inp["G"]).to(dtype))
    return {"h_seq": h_seq.detach().numpy(), "dW": gw.numpy(), "grad_x": gx[0].numpy(), "grad_h0": g0.numpy(), "grad_c0": gc.numpy()}


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    import model_convlstm as ref
    os.makedirs(OUT, exist_ok=True)
    for shape in R.GOLDEN_SHAPES:
        inp = R.lstm_inputs(shape)
        o64, o32 = run(ref, shape, inp, torch.float64), run(ref, shape, inp, torch.float32)
        gaps = {"gap_" + k: np.abs(o32[k].astype(np.float64) - o64[k]).max() for k in NAMES}
        dw = o64["dW"]
        np.savez_compressed(
            os.path.join(OUT, R.name(shape) + ".npz"), seed=R.SEED[shape], shape=np.array(shape),
            digest=R.digest(*(inp[k] for k in ("x", "h0", "c0", "w", "G"))),
            h_seq=o64["h_seq"][:, ::64], grad_x=o64["grad_x"][:, ::16], grad_h0=o64["grad_h0"][:, ::8], grad_c0=o64["grad_c0"][:, ::8],
            dW=dw[R.DW_SUBSET], dW_sum=dw.sum(), dW_l2=np.sqrt((dw * dw).sum()),
            **{"max_" + k: np.abs(o64[k]).max() for k in NAMES}, **gaps)
        print("%s: |dW| max %.3e l2 %.6e, gaps %s" % (R.name(shape), np.abs(dw).max(), np.sqrt((dw * dw).sum()),
                                                      {k: "%.2e" % v for k, v in gaps.items()}), flush=True)


if __name__ == "__main__":
    main()
