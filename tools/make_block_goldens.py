"""Generate tests/golden/block_*.npz by running the reference's own inverted-residual block (`model_convlstm.py`: `dwBlock`,
imported unmodified) under torch autograd on the CPU in float64.  Run by hand where a checkout of the reference is
available; only the .npz files are committed, and the tests read nothing else.

Per configuration of `block_ref64.CFG` ("fucbst": `dwBlock(320, 256)`, no residual; "fust": `dwBlock(256, 256)`, with the
residual) and shape (T, H, W) of `block_ref64.GOLDEN_SHAPES`, with the seeded inputs of `block_ref64.block_case` (BatchNorms
with non-trivial running statistics): the block in eval mode -> o, and the gradients of sum(go * o) with respect to the
block's nine parameters and its input.  The running statistics are checked to be what they were afterwards.

Stored (float64): the seven small gradients whole, the gradients of the expand and the projection conv's weights on
`block_ref64.W_SUBSET` plus their sum and L2 norm, grad_x on `block_ref64.GX_SUBSET`, the seed and a digest of the inputs.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_block_goldens.py REFERENCE_DIR
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

import block_ref64 as BR                       # noqa: E402
import train_ref64 as R                        # noqa: E402


def input_digest(x, q, go):
    return R.digest(x, go, *[q[k] for k in sorted(q)])


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    import model_convlstm as ref
    os.makedirs(OUT, exist_ok=True)
    for cfg in BR.CFGS:
        c = BR.CFG[cfg]
        for shape in BR.GOLDEN_SHAPES:
            x, q, go = BR.block_case(cfg, shape)
            block = BR.load_block(ref.dwBlock(c["cin"], c["cout"], kernel_size=3), q).double()
            for bn in (block.conv[0][1], block.conv[1][1], block.conv[3]):
                bn.eps = BR.BN_EPS
            assert not block.training and bool(block.use_res_connect) == c["res"]
            xx = torch.as_tensor(x).double().requires_grad_(True)
            o = block(xx)
            params = dict(block.named_parameters())
            assert sorted(params) == sorted(BR.NAMES)
            gs = torch.autograd.grad(o, [params[n] for n in BR.NAMES] + [xx], torch.as_tensor(go).double())
            g = {n: t.numpy() for n, t in zip(BR.NAMES, gs)}
            for i, bn in ((1, block.conv[0][1]), (2, block.conv[1][1]), (3, block.conv[3])):
                assert np.array_equal(bn.running_mean.numpy(), q["mu%d" % i].astype(np.float64))
                assert np.array_equal(bn.running_var.numpy(), q["var%d" % i].astype(np.float64))
            big = {}
            for key, n in (("W1", BR.NAMES[0]), ("W3", BR.NAMES[6])):
                w = g[n][:, :, 0, 0]
                big.update({key: w[BR.W_SUBSET], key + "_sum": w.sum(), key + "_l2": np.sqrt((w * w).sum())})
            small = [n for n in BR.NAMES if n not in (BR.NAMES[0], BR.NAMES[6])]
            np.savez_compressed(
                os.path.join(OUT, BR.name(cfg, shape) + ".npz"), seed=BR._seed(cfg, shape), shape=np.array(shape),
                digest=input_digest(x, q, go), grad_x=gs[-1].numpy()[BR.GX_SUBSET], **big,
                **{n.replace(".", "_"): g[n] for n in small})
            print("%s: |dW1| l2 %.6e |dW3| l2 %.6e; %s" % (BR.name(cfg, shape), big["W1_l2"], big["W3_l2"], {
                n: "%.2e" % np.abs(g[n]).max() for n in small}), flush=True)


if __name__ == "__main__":
    main()
