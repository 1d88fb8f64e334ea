"""Generate tests/golden/st_*.npz by running the reference's own ST block (`model.py`: `STBlock`, imported unmodified) under
torch autograd on the CPU in float64.  Run by hand where a checkout of the reference is available; only the .npz files are
committed, and the tests read nothing else.

`model.py` imports `model_feature`, which needs torchvision; an ST block needs no backbone, so a module of that name with
placeholder classes stands in for it (the way oracle/make_goldens.py imports `model.py`).  Per case (N, h, w, L) of
`st_ref64.GOLDEN_CASES`: `STBlock(256, 256, time_dims=L, reduction=8)` in eval mode with the seeded numbers of
`st_ref64.calibrate` (non-trivial running statistics; `time_dims` does not enter the arithmetic) and the inputs of
`st_ref64.golden_inputs`; the gradients of sum(go * block(x)) with respect to the 27 parameters and the input.  The reference
takes every call as ONE sequence for the temporal difference, so a case with L < N is N / L calls of L frames whose parameter
gradients add.  The running statistics are checked to be what they were afterwards.

Stored (float64, `st_ref64.golden_pack`): the small gradients whole, the gradients of the big 1x1 weights on
`st_ref64.W_SUBSET` plus their sum and L2 norm, grad_x on `st_ref64.GX_SUBSET`, and a digest of the inputs.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_st_goldens.py REFERENCE_DIR
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

import st_ref64 as SR                          # noqa: E402


def import_reference(ref_dir):
    mf = types.ModuleType("model_feature")
    mf.ReMobileNetV2 = mf.ReVGG = mf.ReResNet = type("Backbone", (torch.nn.Module,), {})
    sys.modules["model_feature"] = mf
    sys.path.insert(0, os.path.abspath(ref_dir))
    import model as ref_model
    return ref_model


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = import_reference(sys.argv[1])
    os.makedirs(OUT, exist_ok=True)
    for case in SR.GOLDEN_CASES:
        N, h, w, L = case
        block = SR.calibrate(ref.STBlock(256, 256, time_dims=L, reduction=8, res_connect=True))
        x, go = SR.golden_inputs(case)
        digest = SR.golden_digest(block, x, go)
        stats = {k: t.clone() for k, t in block.state_dict().items()}
        block = block.double()
        assert not block.training and block.res_connect and block.fu_type == "sum"
        params = dict(block.named_parameters())
        names = list(params)
        total, gxs = None, []
        for c0 in range(0, N, L):                                # every reference call is one sequence
            xx = torch.as_tensor(x[c0:c0 + L]).double().requires_grad_(True)
            gs = torch.autograd.grad(block(xx), [params[n] for n in names] + [xx], torch.as_tensor(go[c0:c0 + L]).double())
            total = list(gs[:-1]) if total is None else [a + b for a, b in zip(total, gs[:-1])]
            gxs.append(gs[-1])
        for k, t in block.state_dict().items():
            assert torch.equal(t.float() if t.is_floating_point() else t, stats[k]), k
        grads = {n: g.numpy() for n, g in zip(names, total)}
        np.savez_compressed(os.path.join(OUT, SR.golden_name(case) + ".npz"), case=np.array(case), digest=digest,
                            **SR.golden_pack(grads, torch.cat(gxs).numpy()))
        print("%s: %d gradients, |grad_x| max %.3e, digest %s" % (SR.golden_name(case), len(grads), float(torch.cat(gxs).abs().max()),
                                                                   digest[:16]), flush=True)


if __name__ == "__main__":
    main()
