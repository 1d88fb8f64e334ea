"""The census of dispatch signatures (tests/plan_census.py), on the CPU: every kernel instance and edge path that some model size
of `DOMAIN` reaches is walked launch by launch against float64 by tests/test_plan_ops_fp64.py -- by the configurations it always
walked (`BASE`) or by `WALKS`.  Fails when a dispatcher threshold moves or a kernel instance is added without such a check."""
import time

import pytest

import plan_census as PC


@pytest.fixture(scope="module")
def domain_census():
    """{signature: [configurations]} over DOMAIN.  Every plan is recorded here: a configuration that does not record raises."""
    t0 = time.perf_counter()
    cen = PC.census(PC.DOMAIN)
    dt = time.perf_counter() - t0
    print("[plan-census] %d plans recorded on the CPU in %.1f s: %d signatures" % (len(set(PC.DOMAIN)), dt, len(cen)))
    return cen


def _sigs(configs):
    return set().union(*(PC.config_signatures(c) for c in configs))


def _fmt(cen, sigs):
    return "\n".join("  %s   cheapest at %s" % (s, min(cen[s], key=PC.cost)) for s in sorted(sigs, key=str))


def test_every_domain_plan_records(domain_census):
    """No entry is skipped: all of DOMAIN is in the census, the split-mode f16x3 plans (four clips and more) included -- those
    need host allocations aligned like the device's (mock_plan._AlignedTorch)."""
    seen = {c for cs in domain_census.values() for c in cs}
    assert seen == set(PC.DOMAIN)
    split = [c for c in PC.DOMAIN if c[4] == "f16x3" and c[0] >= 4 and c[5] == ""]
    assert len(split) >= 3 * len(PC.SIZES)
    # ... and they really are split-mode plans: some GEMM reads its A operand pre-split (the smallest maps never give a GEMM
    # the 128-row tiles that path has), some depthwise output exists only as its shadow
    presplit = [c for c in split if any(s[0] in ("conv1", "conv3") and s[3] == "presplit" for s in PC.config_signatures(c))]
    assert (8, 8, 360, 640, "f16x3", "") in presplit and len(presplit) > len(split) // 2
    shadow_only = [c for c in split if any(s[0] == "dw" and s[3] == "shadow-out" for s in PC.config_signatures(c))]
    assert (8, 8, 360, 640, "f16x3", "") in shadow_only and len(shadow_only) >= len(split) // 3


def test_every_signature_of_the_domain_is_walked(domain_census):
    walked = _sigs(PC.BASE + PC.WALKS)
    orphans = set(domain_census) - walked
    assert not orphans, "%d dispatch signatures are reached in DOMAIN but walked by no configuration of BASE + WALKS:\n%s" % (
        len(orphans), _fmt(domain_census, orphans))
    assert set(PC.WALKS) <= set(PC.DOMAIN) and not set(PC.WALKS) & set(PC.BASE) and len(set(PC.WALKS)) == len(PC.WALKS)
    print("[plan-census] BASE reaches %d signatures, WALKS %d more" % (len(_sigs(PC.BASE)), len(walked) - len(_sigs(PC.BASE))))


def test_every_walk_contributes(domain_census):
    """The list cannot bloat: each entry reaches a signature that nothing else walked reaches."""
    for cfg in PC.WALKS:
        others = _sigs(tuple(c for c in PC.BASE + PC.WALKS if c != cfg))
        assert PC.config_signatures(cfg) - others, "%s contributes no signature of its own" % (cfg,)


def test_walks_is_the_committed_proposal(domain_census):
    assert tuple(PC.propose_walks()) == PC.WALKS, "WALKS is not what `python tests/plan_census.py` prints"


def test_sampled_walks_are_needed(domain_census):
    """A walk checks an op on a sample of its images where an operand exceeds IMG_BUDGET.  An entry of WALKS with such ops is
    either a 1080x1920 one or there for a signature that no configuration of DOMAIN checked whole reaches."""
    whole = _sigs(c for c in PC.DOMAIN if not PC.config_sampled(c))
    n = 0
    for cfg in PC.WALKS:
        if not PC.config_sampled(cfg) or cfg[2] * cfg[3] >= 1080 * 1920:
            continue
        n += 1
        only = PC.config_signatures(cfg) - _sigs(tuple(c for c in PC.BASE + PC.WALKS if c != cfg)) - whole
        assert only, "%s has sampled ops (%s) but every signature it contributes is reached by a plan checked whole" % (
            cfg, ", ".join(PC.config_sampled(cfg)[:4]))
    print("[plan-census] %d entries of WALKS below 1080x1920 have sampled ops, each for a signature no whole plan reaches" % n)


def test_signature_is_total():
    eng = PC.record(PC.BASE[0])
    for meta, args in zip(eng.ops_meta, eng.op_args):
        if meta["kind"] in PC.SKIP:
            with pytest.raises(ValueError):
                PC.signature(meta, args)
        else:
            assert PC.signature(meta, args)[0] == meta["kind"]
    with pytest.raises(ValueError, match="no dispatch signature"):
        PC.signature(dict(kind="conv5", name="x"), dict(kind="conv5", name="x"))
