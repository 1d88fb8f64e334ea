"""Generate tests/golden/nets_train_*.npz by running the reference's own inverted-residual block (`model_convlstm.py`: `dwBlock`,
imported unmodified at run time, nothing of it copied) through the part of the reference's forward behind the ST blocks WITH
the two prior nets in front of it (reference model.py:346-365, rebuilt here around that block) under torch autograd on the CPU
in float64, in eval mode.  Run by hand where a checkout of the reference is available; only the .npz files are committed, and
the tests read nothing else.

Per prior set of `nets_ref64.GOLDEN_BIAS` at the shape (N, h, w) = `nets_ref64.GOLDEN_SHAPE` (N frames as N / T chunks of T =
`nets_ref64.GOLDEN_T`), with the seeded head of `ctx_ref64.head_case` and the seeded nets of `nets_ref64.net_case`:

    p = cat[gauss_cb_layer(cb0), ob_cb_layer(cb1)];  f = fust(st);  c = f.view(B, T, ...).sum(1);
    c = cxt_cb_prior[1](cxt_cb_prior[0](c));  u = F.interpolate(c, (h, w), mode="bilinear", align_corners=True).repeat(T, 1, 1, 1);
    fu = cat[f, fucb(cat[p, u])];  o = fucbst(fu)

and the gradients of sum(go * o) with respect to the 18 parameters of each enabled net, twice: once with the priors
materialised per frame ("frame": N different prior frames) and once with ONE prior repeated over the frames ("repeat": the
nets run on the N copies, as the reference does).  The running statistics are checked to be what they were afterwards.

Stored: the inputs gauss_cb / ob_cb (float32; "repeat" is frame 0 of them N times) and, per mode under the prefix frame_ /
repeat_, the nets' slices of `g_cb` = d loss / d cat[p, u] on `G_SUBSET` plus their per-channel sums, and per net and block (gauss0_, gauss1_, ob0_, ob1_) the seven small gradients whole,
block 0's expand weight gradient whole, its projection's and block 1's two on `W_SUBSET` plus their sum and L2 norm; and a digest of the inputs.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_nets_goldens.py REFERENCE_DIR
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
import nets_ref64 as NR                        # noqa: E402


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    import model_convlstm as ref
    os.makedirs(OUT, exist_ok=True)
    T, shape = NR.GOLDEN_T, NR.GOLDEN_SHAPE
    N, h, w = shape
    t64 = lambda a: torch.as_tensor(a).double()      # noqa: E731
    for bias in NR.GOLDEN_BIAS:
        store, said = {}, []
        for mode in NR.GOLDEN_MODES:
            Q, st, _, go, nets = NR.golden_case(bias, mode)
            blocks = {}
            for key, q in Q.items():
                name = key if key != "fucb" else "fucb%d" % (64 * sum(bias))
                blocks[key] = X.make_block(name, q, ref.dwBlock).double()
                assert not blocks[key].training
            mods = {net: NR.make_net(net, qs, ref.dwBlock).double() for net, (cb, qs) in nets.items()}
            parts = [mods[net](t64(cb)) for net, (cb, qs) in nets.items()]
            f = blocks["fust"](t64(st))
            if bias[2]:
                c = f.view(N // T, T, 256, h, w).sum(1)
                c = blocks["ctx1"](blocks["ctx0"](c))
                parts.append(F.interpolate(c, size=(h, w), mode="bilinear", align_corners=True).repeat(T, 1, 1, 1))
            cbcat = torch.cat(parts, 1)
            cbcat.retain_grad()
            fu = torch.cat([f, blocks["fucb"](cbcat)], 1)
            o = blocks["fucbst"](fu)
            (o * t64(go)).sum().backward()
            for net, (cb, qs) in nets.items():
                for b, q in zip(mods[net], qs):
                    for i, bn in ((1, b.conv[0][1]), (2, b.conv[1][1]), (3, b.conv[3])):
                        assert np.array_equal(bn.running_mean.numpy(), q["mu%d" % i].astype(np.float64))
                        assert np.array_equal(bn.running_var.numpy(), q["var%d" % i].astype(np.float64))
            g_cb = cbcat.grad.numpy()
            g_cb = g_cb[:, :64 * len(nets)]                      # the nets' slices
            store[mode + "_g_cb"] = g_cb[NR.G_SUBSET]
            store[mode + "_g_cb_sum"] = g_cb.sum((0, 2, 3))
            for net, (cb, qs) in nets.items():
                tag = NR.NETS[net][:-1]
                if mode == "frame":                              # ("repeat" is frame 0 of it, N times)
                    store["%s_cb" % tag] = cb
                for i, b in enumerate(mods[net]):
                    params = dict(b.named_parameters())
                    assert sorted(params) == sorted(BR.NAMES)
                    pre = "%s_%s%d" % (mode, tag, i)
                    for n in BR.NAMES:
                        g = params[n].grad.numpy()
                        if n in NR.golden_subset_names(i):
                            wg = g[:, :, 0, 0]
                            store.update({"%s_%s" % (pre, n.replace(".", "_")): wg[NR.W_SUBSET], "%s_%s_sum" % (pre, n.replace(".", "_")): wg.sum(),
                                          "%s_%s_l2" % (pre, n.replace(".", "_")): np.sqrt((wg * wg).sum())})
                        else:
                            store["%s_%s" % (pre, n.replace(".", "_"))] = g
                    said.append("%s |dW1| max %.3e" % (pre, np.abs(params[BR.NAMES[0]].grad.numpy()).max()))
            store[mode + "_digest"] = NR.golden_digest(Q, st, go, nets)
        path = os.path.join(OUT, NR.golden_name(bias) + ".npz")
        np.savez_compressed(path, shape=np.array(shape), T=T, bias=np.array(bias), **store)
        print("%s (%d bytes): %s" % (NR.golden_name(bias), os.path.getsize(path), "; ".join(said)), flush=True)


if __name__ == "__main__":
    main()
