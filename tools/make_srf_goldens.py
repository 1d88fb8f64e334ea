"""Generate tests/golden/srf_*.npz by running the reference's own SRF-Net head (`model.py`: `uavsal_srfnet_aspp`, imported
unmodified) under torch autograd on the CPU in float64.  Run by hand where a checkout of the reference is available; only the
.npz files are committed, and the tests read nothing else.

`model.py` imports `model_feature`, which needs torchvision; the head needs no backbone, so a module of that name with
placeholder classes stands in for it (the way tools/make_st_goldens.py imports `model.py`), and the head's `features` is a
stub that returns the given `(None, None, c3, c4, c5)`.  Per case of `srf_ref64.GOLDEN_CASES`: the reference's `forward` in
eval mode with the seeded numbers of `srf_ref64.calibrate` (non-trivial running statistics) and the inputs of
`srf_ref64.golden_inputs`; the gradients of sum(go * head(c3, c4, c5)) with respect to the head's 42 parameters.  The running
statistics are checked to be what they were afterwards.

Stored (float64, `srf_ref64.golden_pack`): the small gradients whole, the gradients of the big weights on
`srf_ref64.W_SUBSET` plus their sum and L2 norm, and a digest of the parameters and inputs.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_srf_goldens.py REFERENCE_DIR
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

import srf_ref64 as SF                         # noqa: E402


class _Taps(torch.nn.Module):
    """Stands in for the backbone: hands the head the feature maps it was given."""

    def __init__(self, name=None):
        super().__init__()
        self.taps = None

    def forward(self, x):
        return (None, None) + tuple(self.taps)


def import_reference(ref_dir):
    mf = types.ModuleType("model_feature")
    mf.ReMobileNetV2 = mf.ReVGG = mf.ReResNet = _Taps
    sys.modules["model_feature"] = mf
    sys.path.insert(0, os.path.abspath(ref_dir))
    import model as ref_model
    return ref_model


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = import_reference(sys.argv[1])
    os.makedirs(OUT, exist_ok=True)
    for case in SF.GOLDEN_CASES:
        head = SF.calibrate(ref.uavsal_srfnet_aspp("mobilenet_v2"))
        assert isinstance(head.features, _Taps) and not head.training
        c3, c4, c5, go = SF.golden_inputs(case)
        digest = SF.golden_digest(head, c3, c4, c5, go)
        stats = {k: t.clone() for k, t in head.state_dict().items()}
        head = head.double()
        params = dict(head.named_parameters())
        assert sorted(params) == sorted(SF.HEAD_PARAMS)
        head.features.taps = [torch.as_tensor(t).double() for t in (c3, c4, c5)]
        gs = torch.autograd.grad(head(None), [params[n] for n in SF.HEAD_PARAMS], torch.as_tensor(go).double())
        for k, t in head.state_dict().items():
            assert torch.equal(t.float() if t.is_floating_point() else t, stats[k]), k
        grads = {n: g.numpy() for n, g in zip(SF.HEAD_PARAMS, gs)}
        np.savez_compressed(os.path.join(OUT, SF.golden_name(case) + ".npz"), digest=digest, **SF.golden_pack(grads))
        print("%s: %d gradients, digest %s" % (SF.golden_name(case), len(grads), digest[:16]), flush=True)


if __name__ == "__main__":
    main()
