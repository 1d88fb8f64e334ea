"""Generate tests/golden/decoder_*.npz by running the reference's own decoder block (`model_convlstm.py`: `dwBlock`, imported
unmodified) under torch autograd on the CPU in float64.  Run by hand where a checkout of the reference is available; only
the .npz files are committed, and the tests read nothing else.

Per shape (T, H, W) of `decoder_ref64.GOLDEN_SHAPES`, with the seeded inputs of `decoder_ref64.decoder_case` (BatchNorms
with non-trivial running statistics): a `dwBlock(256, 1)` in eval mode + sigmoid -> y, and the gradients of sum(gy * y) with
respect to the block's nine parameters.  The running statistics are checked to be what they were afterwards.

Stored (float64): the eight small gradients whole, the gradient of the expand conv's weight on `decoder_ref64.W1_SUBSET`
plus its sum and L2 norm, the seed and a digest of the inputs.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_decoder_goldens.py REFERENCE_DIR
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

import decoder_ref64 as DR                     # noqa: E402
import train_ref64 as R                        # noqa: E402


def input_digest(h, q, gy):
    return R.digest(h, gy, *[q[k] for k in sorted(q)])


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    import model_convlstm as ref
    os.makedirs(OUT, exist_ok=True)
    for shape in DR.GOLDEN_SHAPES:
        h, q, gy = DR.decoder_case(shape)
        block = DR.load_block(ref.dwBlock(R.C, 1, kernel_size=3), q).double()
        for bn in (block.conv[0][1], block.conv[1][1], block.conv[3]):
            bn.eps = DR.BN_EPS
        assert not block.training
        y = torch.sigmoid(block(torch.as_tensor(h).double()))
        params = dict(block.named_parameters())
        assert sorted(params) == sorted(DR.NAMES)
        gs = torch.autograd.grad(y, [params[n] for n in DR.NAMES], torch.as_tensor(gy).double())
        g = {n: t.numpy() for n, t in zip(DR.NAMES, gs)}
        for i, bn in ((1, block.conv[0][1]), (2, block.conv[1][1]), (3, block.conv[3])):
            assert np.array_equal(bn.running_mean.numpy(), q["mu%d" % i].astype(np.float64))
            assert np.array_equal(bn.running_var.numpy(), q["var%d" % i].astype(np.float64))
        w1 = g[DR.NAMES[0]][:, :, 0, 0]
        np.savez_compressed(
            os.path.join(OUT, DR.name(shape) + ".npz"), seed=R.SEED[shape], shape=np.array(shape), digest=input_digest(h, q, gy),
            W1=w1[DR.W1_SUBSET], W1_sum=w1.sum(), W1_l2=np.sqrt((w1 * w1).sum()),
            **{n.replace(".", "_"): g[n] for n in DR.NAMES[1:]})
        print("%s: |dW1| max %.3e l2 %.6e; %s" % (DR.name(shape), np.abs(w1).max(), np.sqrt((w1 * w1).sum()), {
            n: "%.2e" % np.abs(g[n]).max() for n in DR.NAMES[1:]}), flush=True)


if __name__ == "__main__":
    main()
