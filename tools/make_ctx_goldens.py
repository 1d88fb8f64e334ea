"""Generate tests/golden/ctx_train_*.npz by running the reference's own inverted-residual block (`model_convlstm.py`: `dwBlock`,
imported unmodified at run time, nothing of it copied) through the part of the reference's forward behind the ST blocks
(reference model.py:344-365, rebuilt here around that block) under torch autograd on the CPU in float64, in eval mode.  Run by
hand where a checkout of the reference is available; only the .npz files are committed, and the tests read nothing else.

Per prior set of `mp_ref64.GOLDEN_BIAS` at the shape (N, h, w) = `mp_ref64.GOLDEN_SHAPE` (N frames as N / T chunks of T =
`mp_ref64.GOLDEN_T`), with the seeded blocks and inputs of `ctx_ref64.head_case`:

    f = fust(st);  c = f.view(B, T, ...).sum(1);  c = cxt_cb_prior[1](cxt_cb_prior[0](c));
    u = F.interpolate(c, (h, w), mode="bilinear", align_corners=True).repeat(T, 1, 1, 1);
    fu = cat[f, fucb(cat[priors, u])];  o = fucbst(fu)

and the gradients of sum(go * o) with respect to the nine parameters of fucb_layer[0] and -- with the context prior -- of
cxt_cb_prior[1] and cxt_cb_prior[0]: the multi-prior path `train.prior_path_backward` trains.  The running statistics are
checked to be what they were afterwards.

Stored (float64), per block under the prefix fucb_ / ctx1_ / ctx0_: the seven small gradients whole, the gradients of the
expand and the projection conv's weights on `W_SUBSET` plus their sum and L2 norm; and a digest of the inputs.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_ctx_goldens.py REFERENCE_DIR
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
import mp_ref64 as MP                          # noqa: E402


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    import model_convlstm as ref
    os.makedirs(OUT, exist_ok=True)
    T, shape = MP.GOLDEN_T, MP.GOLDEN_SHAPE
    N, h, w = shape
    for bias in MP.GOLDEN_BIAS:
        Q, st, priors, go = X.head_case(bias, shape, T)
        blocks = {}
        for key, q in Q.items():
            name = key if key != "fucb" else "fucb%d" % (64 * sum(bias))
            blocks[key] = X.make_block(name, q, ref.dwBlock).double()
            assert not blocks[key].training
        f = blocks["fust"](torch.as_tensor(st).double())
        parts = [torch.as_tensor(priors).double()] if priors is not None else []
        if bias[2]:
            c = f.view(N // T, T, 256, h, w).sum(1)
            c = blocks["ctx1"](blocks["ctx0"](c))
            parts.append(F.interpolate(c, size=(h, w), mode="bilinear", align_corners=True).repeat(T, 1, 1, 1))
        fu = torch.cat([f, blocks["fucb"](torch.cat(parts, 1))], 1)
        o = blocks["fucbst"](fu)
        (o * torch.as_tensor(go).double()).sum().backward()
        for key, q in Q.items():
            b = blocks[key]
            for i, bn in ((1, b.conv[0][1]), (2, b.conv[1][1]), (3, b.conv[3])):
                assert np.array_equal(bn.running_mean.numpy(), q["mu%d" % i].astype(np.float64))
                assert np.array_equal(bn.running_var.numpy(), q["var%d" % i].astype(np.float64))
        store, said = {}, []
        for name in MP.PATH_BLOCKS:
            key = MP.PATH_KEYS[name]
            if key not in blocks:
                continue
            params = dict(blocks[key].named_parameters())
            assert sorted(params) == sorted(BR.NAMES)
            g = {n: params[n].grad.numpy() for n in BR.NAMES}
            for tag, n in (("W1", BR.NAMES[0]), ("W3", BR.NAMES[6])):
                wg = g[n][:, :, 0, 0]
                store.update({"%s_%s" % (key, tag): wg[MP.W_SUBSET], "%s_%s_sum" % (key, tag): wg.sum(),
                              "%s_%s_l2" % (key, tag): np.sqrt((wg * wg).sum())})
            for n in BR.NAMES:
                if n not in (BR.NAMES[0], BR.NAMES[6]):
                    store["%s_%s" % (key, n.replace(".", "_"))] = g[n]
            said.append("%s |dW1| l2 %.3e |dW3| l2 %.3e" % (key, store[key + "_W1_l2"], store[key + "_W3_l2"]))
        path = os.path.join(OUT, MP.golden_name(bias) + ".npz")
        np.savez_compressed(path, shape=np.array(shape), T=T, bias=np.array(bias), digest=MP.path_digest(Q, st, priors, go), **store)
        print("%s (%d bytes): %s" % (MP.golden_name(bias), os.path.getsize(path), "; ".join(said)), flush=True)


if __name__ == "__main__":
    main()
