"""Generate tests/golden/fust_*.npz by running the reference's own inverted-residual block (`model_convlstm.py`: `dwBlock`,
imported unmodified) through the part of the reference's forward behind the ST blocks (reference model.py:344-365, rebuilt
here around that block) under torch autograd on the CPU in float64.  Run by hand where a checkout of the reference is
available; only the .npz files are committed, and the tests read nothing else.

Per prior set of `ctx_ref64.GOLDEN_BIAS` and shape (N, h, w) of `ctx_ref64.GOLDEN_SHAPES` (N frames as N / T chunks of T =
`ctx_ref64.GOLDEN_T`), with the seeded blocks and inputs of `ctx_ref64.head_case` (every block calibrated on the activations
it sees, BatchNorms in eval mode with non-trivial running statistics):

    f = fust(st);  c = f.view(B, T, ...).sum(1);  c = cxt_cb_prior[1](cxt_cb_prior[0](c));
    u = F.interpolate(c, (h, w), mode="bilinear", align_corners=True).repeat(T, 1, 1, 1);
    fu = cat[f, fucb(cat[priors, u])];  o = fucbst(fu)

and the gradients of sum(go * o) with respect to fust's nine parameters, to f and to fu.  The running statistics are checked
to be what they were afterwards.

Stored (float64): the seven small gradients whole, the gradients of the expand and the projection conv's weights on
`block_ref64.W_SUBSET` plus their sum and L2 norm, the gradients of f and of fu on `block_ref64.GX_SUBSET`, and a digest of
the inputs.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_fust_goldens.py REFERENCE_DIR
"""
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden")

import block_ref64 as BR                       # noqa: E402
import ctx_ref64 as X                          # noqa: E402


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    import model_convlstm as ref
    os.makedirs(OUT, exist_ok=True)
    T = X.GOLDEN_T
    for bias in X.GOLDEN_BIAS:
        for shape in X.GOLDEN_SHAPES:
            Q, st, priors, go = X.head_case(bias, shape, T)
            N, h, w = shape
            blocks = {}
            for key, q in Q.items():
                name = key if key != "fucb" else "fucb%d" % (64 * sum(bias))
                blocks[key] = X.make_block(name, q, ref.dwBlock).double()
                assert not blocks[key].training
            assert blocks["fust"].use_res_connect and not blocks["fucbst"].use_res_connect
            x = torch.as_tensor(st).double()
            f = blocks["fust"](x)
            f.retain_grad()
            c = f.view(N // T, T, 256, h, w).sum(1)
            c = blocks["ctx1"](blocks["ctx0"](c))
            u = F.interpolate(c, size=(h, w), mode="bilinear", align_corners=True).repeat(T, 1, 1, 1)
            cat = torch.cat(([torch.as_tensor(priors).double()] if priors is not None else []) + [u], 1)
            fu = torch.cat([f, blocks["fucb"](cat)], 1)
            fu.retain_grad()
            o = blocks["fucbst"](fu)
            params = dict(blocks["fust"].named_parameters())
            assert sorted(params) == sorted(BR.NAMES)
            (o * torch.as_tensor(go).double()).sum().backward()
            g = {n: params[n].grad.numpy() for n in BR.NAMES}
            for key, q in Q.items():
                b = blocks[key]
                for i, bn in ((1, b.conv[0][1]), (2, b.conv[1][1]), (3, b.conv[3])):
                    assert np.array_equal(bn.running_mean.numpy(), q["mu%d" % i].astype(np.float64))
                    assert np.array_equal(bn.running_var.numpy(), q["var%d" % i].astype(np.float64))
            big = {}
            for key, n in (("W1", BR.NAMES[0]), ("W3", BR.NAMES[6])):
                wg = g[n][:, :, 0, 0]
                big.update({key: wg[BR.W_SUBSET], key + "_sum": wg.sum(), key + "_l2": np.sqrt((wg * wg).sum())})
            small = [n for n in BR.NAMES if n not in (BR.NAMES[0], BR.NAMES[6])]
            np.savez_compressed(
                os.path.join(OUT, X.golden_name(bias, shape) + ".npz"), shape=np.array(shape), T=T, bias=np.array(bias),
                digest=X.head_digest(Q, st, priors, go), grad_f=f.grad.numpy()[BR.GX_SUBSET], grad_fu=fu.grad.numpy()[BR.GX_SUBSET],
                **big, **{n.replace(".", "_"): g[n] for n in small})
            print("%s: |dW1| l2 %.6e |dW3| l2 %.6e; %s" % (X.golden_name(bias, shape), big["W1_l2"], big["W3_l2"], {
                n: "%.2e" % np.abs(g[n]).max() for n in small}), flush=True)


if __name__ == "__main__":
    main()
