"""Generate tests/golden/fuse_bn_*.npz by running the reference's own modules (`model_convlstm.py`: `dwBlock`, `ConvTWA`, imported
unmodified) in `.train()` mode under torch autograd on the CPU in float64.  Run by hand where a checkout of the reference is
available; only the .npz files are committed, and the tests read nothing else.

Per configuration of `fuse_bn_ref64.CFG` ("fucbst": `dwBlock(320, 256)`, "fust": `dwBlock(256, 256)` with the residual) and
shape (T, H, W) of `fuse_bn_ref64.SHAPES`, with the seeded inputs of `fuse_bn_ref64.block_case`: the block in training mode ->
out, the gradients of sum(go * out) with respect to its nine parameters and to its input, the batch mean and biased variance
each BatchNorm saw (forward hooks on the BatchNorms' inputs), the running statistics and `num_batches_tracked` after the step.
One chain at `fuse_bn_ref64.CHAIN_SHAPE` (`chain_case`): `dwBlock(320, 256).train()` -> `ConvTWA` (its state given) ->
`dwBlock(256, 1).train()` + sigmoid with the loss sum(gy * y): y, the gradients of both blocks' parameters, of the ConvTWA
weight and of the chain's input, and both blocks' moved statistics.

Stored (float64 unless said): a digest of the inputs and the module's numbers (the tests regenerate them from the seed); the six
BatchNorm gradients whole; the 1x1 weight gradients on `fuse_bn_ref64.W_SUBSET`, the depthwise one on `WD_SUBSET`, out / y and
grad_x on `GX_SUBSET`, each with its sum and L2 norm over the WHOLE tensor; mu1..3 / var1..3, rm1..3 / rv1..3, nbt.  The chain
holds two blocks and the recurrence, so it keeps the coarser `CHAIN_*` subsets (the ConvTWA gradient on `CHAIN_RNN_SUBSET`, the
statistics on `CHAIN_C_SUBSET` with their sums).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_fuse_bn_goldens.py REFERENCE_DIR
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

import fuse_bn_ref64 as FR                     # noqa: E402
import train_ref64 as R                        # noqa: E402


def _bns(block):
    return block.conv[0][1], block.conv[1][1], block.conv[3]


def _hook(block, seen, tag):
    return [b.register_forward_hook(lambda m, inp, out, i=i: seen.__setitem__("%s%d" % (tag, i), inp[0].detach()))
            for i, b in enumerate(_bns(block), 1)]


def _stats(block, seen, tag, pre="", subset=None):
    out = {}
    for i, b in enumerate(_bns(block), 1):
        u = seen["%s%d" % (tag, i)]
        vals = {"mu": u.mean((0, 2, 3)).numpy(), "var": u.var((0, 2, 3), unbiased=False).numpy(),
                "rm": b.running_mean.numpy(), "rv": b.running_var.numpy()}
        for k, v in vals.items():
            if subset is None:
                out["%s%s%d" % (pre, k, i)] = v
            else:
                out.update(summed("%s%s%d" % (pre, k, i), v, subset))
        assert int(b.num_batches_tracked) == 1
    return out


def summed(key, t, subset):
    """a tensor on `subset` with its whole sum and L2 norm"""
    return {key: t[subset], key + "_sum": t.sum(), key + "_l2": np.sqrt((t * t).sum())}


def block_grads(g, pre="", w_subset=FR.W_SUBSET, wd_subset=FR.WD_SUBSET):
    """the nine gradients of a block (numpy, keyed by NAMES) as the goldens keep them"""
    out = {}
    for n in (FR.NAMES[1], FR.NAMES[2], FR.NAMES[4], FR.NAMES[5], FR.NAMES[7], FR.NAMES[8]):
        out[pre + n.replace(".", "_")] = g[n]
    out.update(summed(pre + "W1", g[FR.NAMES[0]][:, :, 0, 0], w_subset))
    w3 = g[FR.NAMES[6]][:, :, 0, 0]
    out.update(summed(pre + "W3", w3, w_subset if w3.shape[0] > 1 else (slice(None), slice(None))))
    out.update(summed(pre + "Wd", g[FR.NAMES[3]], wd_subset))
    return out


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    import model_convlstm as ref
    os.makedirs(OUT, exist_ok=True)
    for cfg in FR.CFGS:
        c = FR.CFG[cfg]
        for shape in FR.SHAPES:
            x, q, go = FR.block_case(cfg, shape)
            block = FR.load_block(ref.dwBlock(c["cin"], c["cout"], kernel_size=3), q).double()
            assert block.training and all(b.training for b in _bns(block)) and block.use_res_connect == c["res"]
            seen = {}
            hooks = _hook(block, seen, "b")
            xx = torch.as_tensor(x).double().requires_grad_(True)
            out = block(xx)
            for hk in hooks:
                hk.remove()
            params = dict(block.named_parameters())
            assert sorted(params) == sorted(FR.NAMES)
            gs = torch.autograd.grad(out, [params[n] for n in FR.NAMES] + [xx], torch.as_tensor(go).double())
            g = {n: t.numpy() for n, t in zip(FR.NAMES, gs[:9])}
            path = os.path.join(OUT, FR.name(cfg, shape) + ".npz")
            np.savez_compressed(path, shape=np.array(shape), digest=R.digest(x, go, *[q[k] for k in sorted(q)]), nbt=np.array(1),
                                **summed("out", out.detach().numpy(), FR.GX_SUBSET), **summed("grad_x", gs[9].numpy(), FR.GX_SUBSET),
                                **block_grads(g), **_stats(block, seen, "b"))
            print("%s: %d bytes; |out| max %.3e; |grad_x| max %.3e" % (FR.name(cfg, shape), os.path.getsize(path),
                                                                       float(out.detach().abs().max()), float(gs[9].abs().max())), flush=True)
    # the chain
    shape = FR.CHAIN_SHAPE
    T, H, W = shape
    x, qb, h0, w, qd, gy = FR.chain_case(shape)
    blk = FR.load_block(ref.dwBlock(320, 256, kernel_size=3), qb).double()
    dec = FR.load_block(ref.dwBlock(256, 1, kernel_size=3), qd).double()
    rnn = ref.ConvTWA((H, W), 256, 256, kernel_size=(3, 3), num_layers=1, batch_first=True, bias=False,
                      return_all_layers=False).double()
    rc = rnn.cell_list[0].rnn_conv
    with torch.no_grad():
        rc.weight.copy_(torch.as_tensor(w))
    seen = {}
    hooks = _hook(blk, seen, "b") + _hook(dec, seen, "d")
    xx = torch.as_tensor(x).double().requires_grad_(True)
    x_seq = blk(xx)
    h_seq, _ = rnn(x_seq.contiguous().view(1, T, 256, H, W), [torch.as_tensor(h0).double()])
    h_seq = h_seq.contiguous().view(T, 256, H, W)
    y = torch.sigmoid(dec(h_seq))
    for hk in hooks:
        hk.remove()
    pb, pd = dict(blk.named_parameters()), dict(dec.named_parameters())
    gs = torch.autograd.grad(y, [pb[n] for n in FR.NAMES] + [pd[n] for n in FR.NAMES] + [rc.weight, xx], torch.as_tensor(gy).double())
    gb = {n: t.numpy() for n, t in zip(FR.NAMES, gs[:9])}
    gd = {n: t.numpy() for n, t in zip(FR.NAMES, gs[9:18])}
    path = os.path.join(OUT, FR.chain_name(shape) + ".npz")
    np.savez_compressed(path, shape=np.array(shape), nbt=np.array(1),
                        digest=R.digest(x, h0, w, gy, *[qb[k] for k in sorted(qb)], *[qd[k] for k in sorted(qd)]),
                        y=y.detach().numpy(), **summed("h_seq", h_seq.detach().numpy(), FR.GX_SUBSET),
                        **summed("rnn", gs[18].numpy(), FR.CHAIN_RNN_SUBSET), **summed("grad_x", gs[19].numpy(), FR.GX_SUBSET),
                        **block_grads(gb, "block_", FR.CHAIN_W_SUBSET, FR.CHAIN_WD_SUBSET),
                        **block_grads(gd, "decoder_", FR.CHAIN_W_SUBSET, FR.CHAIN_WD_SUBSET),
                        **_stats(blk, seen, "b", "block_", FR.CHAIN_C_SUBSET), **_stats(dec, seen, "d", "decoder_", FR.CHAIN_C_SUBSET))
    print("%s: %d bytes; |y| max %.3e; |d rnn| max %.3e" % (FR.chain_name(shape), os.path.getsize(path), float(y.detach().abs().max()),
                                                            float(gs[18].abs().max())), flush=True)


if __name__ == "__main__":
    main()
