"""Generate tests/golden/shallow_*.npz by running the reference's own inverted-residual block (`model.py`: `dwBlock`, imported
unmodified) under torch autograd on the CPU in float64, at the five block shapes of MobileNetV2 features[2:8].  Run by hand
where a checkout of the reference is available; only the .npz files are committed, and the tests read nothing else.

`model.py` imports `model_feature`, which needs torchvision; a block needs no backbone, so a module of that name with
placeholder classes stands in for it (the way tools/make_backbone_goldens.py imports `model.py`).  torchvision's
`InvertedResidual` and the reference's `dwBlock` are the same nine-parameter module, so `dwBlock(cin, cout, stride=...,
expand_ratio=6)` stands for the backbone's blocks.

Per block of `shallow_ref64.BLOCKS` (16 -> 96 -> 24 with stride 2, 24 -> 144 -> 24 with the residual, 24 -> 144 -> 32 with
stride 2, 32 -> 192 -> 32 with the residual, 32 -> 192 -> 64 with stride 2) and input grid of `shallow_ref64.PICTURES`
(4 x 6 and the odd 5 x 7), with the seeded inputs of `shallow_ref64.block_case`: the block in eval mode -> o, and the gradients
of sum(go * o) with respect to the block's nine parameters and its input.  The running statistics are checked to be what they
were afterwards.

Stored (float64): the seven small gradients whole, the gradients of the expand and the projection conv's weights on
`shallow_ref64.W_SUBSET` plus their sum and L2 norm, grad_x whole (at most 2 x 32 x 5 x 7 numbers), and a digest of the inputs.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_shallow_goldens.py REFERENCE_DIR
"""
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden")

import block_ref64 as BR                       # noqa: E402
import shallow_ref64 as SH                     # noqa: E402


class _Absent(torch.nn.Module):
    """Stands in for the backbone classes `model.py` imports by name; never built here."""


def import_reference(ref_dir):
    mf = types.ModuleType("model_feature")
    mf.ReMobileNetV2 = mf.ReVGG = mf.ReResNet = _Absent
    sys.modules["model_feature"] = mf
    sys.path.insert(0, os.path.abspath(ref_dir))
    import model as ref_model
    return ref_model


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = import_reference(sys.argv[1])
    os.makedirs(OUT, exist_ok=True)
    for name, cfg in SH.BLOCKS.items():
        cin, hid, cout, stride, res = cfg
        for pic in SH.PICTURES:
            x, q, go = SH.block_case(name, pic)
            block = BR.load_block(ref.dwBlock(cin, cout, kernel_size=3, stride=stride, expand_ratio=hid // cin), q).double()
            for bn in (block.conv[0][1], block.conv[1][1], block.conv[3]):
                bn.eps = BR.BN_EPS
            assert not block.training and bool(block.use_res_connect) == res
            xx = torch.as_tensor(x).double().requires_grad_(True)
            o = block(xx)
            assert tuple(o.shape) == go.shape
            params = dict(block.named_parameters())
            assert tuple(params) == SH.NAMES
            gs = torch.autograd.grad(o, [params[n] for n in SH.NAMES] + [xx], torch.as_tensor(go).double())
            g = {n: t.numpy() for n, t in zip(SH.NAMES, gs)}
            for i, bn in ((1, block.conv[0][1]), (2, block.conv[1][1]), (3, block.conv[3])):
                assert np.array_equal(bn.running_mean.numpy(), q["mu%d" % i].astype(np.float64))
                assert np.array_equal(bn.running_var.numpy(), q["var%d" % i].astype(np.float64))
            path = os.path.join(OUT, SH.golden_name(name, pic) + ".npz")
            np.savez_compressed(path, shape=np.array(pic), digest=SH.golden_digest(x, q, go), grad_x=gs[-1].numpy(), **SH.golden_pack(g))
            print("%s (%d bytes)" % (SH.golden_name(name, pic), os.path.getsize(path)), flush=True)


if __name__ == "__main__":
    main()
