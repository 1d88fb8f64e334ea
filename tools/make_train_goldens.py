"""Generate tests/golden/train_*.npz by running the reference's own recurrence and decoder block (`model_convlstm.py`:
`ConvTWA` and `dwBlock`, imported unmodified) under torch autograd on the CPU, in float64 and in float32.  Run by hand
where a checkout of the reference is available; only the .npz files are committed, and the tests read nothing else.

Per shape (T, H, W) of `train_ref64.GOLDEN_SHAPES`, with the seeded inputs of `train_ref64.twa_inputs`:
  1. `ConvTWA(x, hidden_state=[h0])` (the state is passed explicitly: `_init_hidden` calls `.cuda()`) -> the history h_seq;
  2. a `dwBlock(256, 1)` in eval mode with `train_ref64.decoder_params` of that history, + sigmoid -> y, and
     `grad_h = d sum(gy * y) / d h_seq` with the history detached (the DIRECT gradient of every h_t, what
     `train.twa_backward` takes);
  3. `grad_h` back through the recurrence: dW, grad_x, grad_h0.
The float32 run of step 3 is given the float64 `grad_h` rounded to float32, so that its gap to float64 is the recurrence's
own rounding and not a ReLU6 mask of the decoder that fell the other way.

Stored (float64 unless said): the decoder's folded scales and biases (they depend on the history), `grad_h`, `grad_x` on
every 16th channel, `grad_h0` on every 8th, dW on `train_ref64.DW_SUBSET` plus its sum and L2 norm, the reference's own
max |fp32 - float64| gap per tensor (over ALL elements), the seed and a digest of the inputs.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_train_goldens.py REFERENCE_DIR
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

import train_ref64 as R                        # noqa: E402


def run(ref, shape, inp, dtype, p=None, grad_h=None):
    T, H, W = shape
    twa = ref.ConvTWA(input_size=(H, W), input_dim=R.C, hidden_dim=R.C, kernel_size=(3, 3), num_layers=1,
                      batch_first=True, bias=False, return_all_layers=False).to(dtype)
    wt = twa.cell_list[0].rnn_conv.weight
    with torch.no_grad():
        wt.copy_(torch.as_tensor(inp["w"]).to(dtype))
    x = torch.as_tensor(inp["x"]).to(dtype)[None].requires_grad_(True)
    h0 = torch.as_tensor(inp["h0"]).to(dtype).requires_grad_(True)
    out, _ = twa(x, hidden_state=[h0])
    h_seq = out[0]
    if p is None:
        p = R.decoder_params(h_seq.detach().numpy(), R.SEED[shape] + 7)
    if grad_h is None:
        block = R.load_block(ref.dwBlock(R.C, 1, kernel_size=3), p).to(dtype)
        hd = h_seq.detach().clone().requires_grad_(True)
        y = torch.sigmoid(block(hd))
        grad_h = torch.autograd.grad(y, hd, torch.as_tensor(inp["gy"]).to(dtype))[0]
    gw, gx, g0 = torch.autograd.grad(h_seq, (wt, x, h0), grad_h.to(dtype))
    return p, {"grad_h": grad_h.detach().numpy(), "grad_x": gx[0].numpy(), "grad_h0": g0.numpy(), "dW": gw.numpy()}


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    import model_convlstm as ref
    os.makedirs(OUT, exist_ok=True)
    for shape in R.GOLDEN_SHAPES:
        inp = R.twa_inputs(shape)
        p, o64 = run(ref, shape, inp, torch.float64)
        _, o32 = run(ref, shape, inp, torch.float32, p, torch.as_tensor(o64["grad_h"]).float())
        gaps = {"gap_" + k: np.abs(o32[k].astype(np.float64) - o64[k]).max() for k in ("grad_x", "grad_h0", "dW")}
        dw = o64["dW"]
        np.savez_compressed(
            os.path.join(OUT, R.name(shape) + ".npz"), seed=R.SEED[shape], shape=np.array(shape),
            digest=R.digest(inp["x"], inp["h0"], inp["w"], inp["gy"]),
            **{k: p[k] for k in ("s1", "b1", "s2", "b2", "s3", "b3")},
            grad_h=o64["grad_h"][:, ::16], grad_x=o64["grad_x"][:, ::16], grad_h0=o64["grad_h0"][:, ::8],
            dW=dw[R.DW_SUBSET], dW_sum=dw.sum(), dW_l2=np.sqrt((dw * dw).sum()),
            max_grad_x=np.abs(o64["grad_x"]).max(), max_grad_h0=np.abs(o64["grad_h0"]).max(), max_dW=np.abs(dw).max(), **gaps)
        print("%s: |dW| max %.3e l2 %.6e, gaps %s" % (R.name(shape), np.abs(dw).max(), np.sqrt((dw * dw).sum()),
                                                      {k: "%.2e" % v for k, v in gaps.items()}), flush=True)


if __name__ == "__main__":
    main()
