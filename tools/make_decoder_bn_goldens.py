"""Generate tests/golden/decoder_bn_*.npz by running the reference's own decoder block (`model_convlstm.py`: `dwBlock`,
imported unmodified) in `.train()` mode under torch autograd on the CPU in float64.  Run by hand where a checkout of the
reference is available; only the .npz files are committed, and the tests read nothing else.

Per shape (T, H, W) of `decoder_bn_ref64.SHAPES`, with the seeded inputs of `decoder_bn_ref64.decoder_case`: a
`dwBlock(256, 1)` in training mode + sigmoid -> y, the gradients of sum(gy * y) with respect to the block's nine parameters
and to its input, the batch mean and biased variance each BatchNorm saw (forward hooks on the BatchNorms' inputs), and the
running statistics and `num_batches_tracked` after that one step.

Stored: the inputs gy and -- where it is small, under 100 pixels -- h (float32; a digest of h, gy and the module's numbers always:
the tests regenerate them from the seed), y, the eight small gradients whole, the gradient of the expand conv's weight on
`decoder_bn_ref64.W1_SUBSET` plus its sum and L2 norm, grad_h on the channels `decoder_bn_ref64.GH_SUBSET` plus its L2 norm,
mu1..3 / var1..3, rm1..3 / rv1..3, nbt (float64 unless said).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_decoder_bn_goldens.py REFERENCE_DIR
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

import decoder_bn_ref64 as BR                  # noqa: E402
import train_ref64 as R                        # noqa: E402


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    import model_convlstm as ref
    os.makedirs(OUT, exist_ok=True)
    for shape in BR.SHAPES:
        h, q, gy = BR.decoder_case(shape)
        block = BR.load_block(ref.dwBlock(BR.C_IN, 1, kernel_size=3), q).double()
        bns = (block.conv[0][1], block.conv[1][1], block.conv[3])
        assert block.training and all(b.training for b in bns)
        seen = {}
        hooks = [b.register_forward_hook(lambda m, inp, out, i=i: seen.__setitem__(i, inp[0].detach())) for i, b in enumerate(bns, 1)]
        x = torch.as_tensor(h).double().requires_grad_(True)
        y = torch.sigmoid(block(x))
        for hk in hooks:
            hk.remove()
        params = dict(block.named_parameters())
        assert sorted(params) == sorted(BR.NAMES)
        gs = torch.autograd.grad(y, [params[n] for n in BR.NAMES] + [x], torch.as_tensor(gy).double())
        g = {n: t.numpy() for n, t in zip(BR.NAMES, gs[:9])}
        gh = gs[9].numpy()
        extra = {}
        for i, b in enumerate(bns, 1):
            u = seen[i]
            extra["mu%d" % i] = u.mean((0, 2, 3)).numpy()
            extra["var%d" % i] = u.var((0, 2, 3), unbiased=False).numpy()
            extra["rm%d" % i], extra["rv%d" % i] = b.running_mean.numpy(), b.running_var.numpy()
            assert int(b.num_batches_tracked) == 1
        w1 = g[BR.NAMES[0]][:, :, 0, 0]
        np.savez_compressed(
            os.path.join(OUT, BR.name(shape) + ".npz"), shape=np.array(shape), gy=gy,
            digest=R.digest(h, gy, *[q[k] for k in sorted(q)]), **({"h": h} if h.shape[0] * h.shape[2] * h.shape[3] < 100 else {}), y=y.detach().numpy(), nbt=np.array(1),
            W1=w1[BR.W1_SUBSET], W1_sum=w1.sum(), W1_l2=np.sqrt((w1 * w1).sum()),
            grad_h=gh[:, BR.GH_SUBSET], grad_h_l2=np.sqrt((gh * gh).sum()),
            **{n.replace(".", "_"): g[n] for n in BR.NAMES[1:]}, **extra)
        print("%s: |dW1| max %.3e; |grad_h| max %.3e; %s" % (BR.name(shape), np.abs(w1).max(), np.abs(gh).max(), {
            n: "%.2e" % np.abs(g[n]).max() for n in BR.NAMES[1:]}), flush=True)


if __name__ == "__main__":
    main()
