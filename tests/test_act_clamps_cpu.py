"""The saturating cases of tests/act_ref64.py, checked in float64 without a device: both clamps of every ReLU6 stage are
populated (the share condition), every wrong reference is at least 4 bounds from the right one at some element (so a kernel
within 1 bound of the right reference is at least 3 bounds from every wrong one), clamped outputs sit on the ragged edges, the
depthwise cases reach every kernel variant the older depthwise tests reach, the dwproj cases every instance, and the GEMM
launches take the routes they are meant for (the library's host-side queries)."""
import collections

import pytest
import torch

import act_ref64 as A
import plan_ref64 as R

LAUNCHES = A.launches()
KEYS = list(collections.OrderedDict((l.key, None) for l in LAUNCHES))
BIG = [k for k in KEYS if k[0] == "conv" and k[1] * k[2] * k[3] * k[4] * k[5] > 1 << 31]      # (the stream-K case)


def _kid(key):
    return "-".join(str(v).replace(" ", "") for v in key)


def _bounds(key):
    """The bound of every (precision, Winograd r) a launch of this problem is judged with."""
    p = A.problem(key)
    seen = collections.OrderedDict(((l.prec, l.kw.get("r") if l.op == "wino" else None), None) for l in LAUNCHES if l.key == key)
    return [(pr, r, p.bound(pr, r)) for pr, r in seen]


@pytest.mark.parametrize("key", KEYS, ids=_kid)
def test_share_condition_and_wrong_references(key):
    p = A.problem(key)
    assert p.stages and set(p.pres()) == set(p.stages), (key, p.stages)
    for st, pre in p.pres().items():
        assert A.share_ok(pre), "%s stage %s: (n, <= 0, >= 6, inside) = %s" % (key, st, A.shares(pre))
    y = p.y()
    assert bool(torch.isfinite(y).all())
    worst = None
    for prec, r, bnd in _bounds(key):
        assert bool((bnd > 0).all()) and bool(torch.isfinite(bnd).all())
        for wr in p.wrongs:
            ratio = ((p.y(wr) - y).abs() / bnd).max().item()
            worst = ratio if worst is None else min(worst, ratio)
            assert ratio >= 4.0, "%s %s%s: the wrong reference '%s' is only %.3g bounds from the right one" % (
                key, prec, " r=%d" % r if r else "", wr, ratio)
    assert len(p.wrongs) >= 2 * len(p.stages)
    if key in BIG:
        A.forget(key)
    print("[act-clamps] %s: stages %s; smallest wrong-reference distance %.3g bounds" % (
        _kid(key), ", ".join("%s %d/%d/%d/%d" % ((s,) + A.shares(v)) for s, v in p.pres().items()), worst))


def test_clamped_outputs_on_the_ragged_edges():
    """Per family: among the cases whose output is a ReLU6, elements at 6 and elements at 0 in the last row, the last column,
    the last channel and the last image (where an epilogue variant differs: partial tiles, scalar tails)."""
    hit = collections.defaultdict(lambda: [False] * 8)
    for l in LAUNCHES:
        if l.key in BIG:
            continue
        p = A.problem(l.key)
        if "out" not in p.stages:
            continue
        pre = p.pres()["out"]
        for j, m in enumerate((pre >= 6, pre <= 0)):
            for i, part in enumerate((m[:, :, -1, :], m[:, :, :, -1], m[:, -1], m[-1])):
                hit[l.family][4 * j + i] |= bool(part.any())
    assert {"conv/staged", "conv/bf16", "conv/k32", "conv/scalar", "conv/ksplit", "conv/presplit", "conv/ngroup", "wino", "dw",
            "stem", "dwproj"} <= set(hit), sorted(hit)
    for fam, h in hit.items():
        assert all(h), (fam, h)


def test_depthwise_cases_reach_every_variant_of_the_older_tests():
    import test_hip_kernels as K
    marks = K.test_depthwise_channel_groups_with_their_own_dilation.pytestmark
    groups = [m.args[1] for m in marks if m.name == "parametrize" and m.args[0] == "case"][0]
    old = {A.dw_variant(*c) for c in K.DW_CASES} | {A.dw_variant(n, h, w, c, 1, tuple(d)) for n, h, w, c, d in groups}
    new = {A.dw_variant(*l.key[1:7]) for l in LAUNCHES if l.key[0] == "dw"}
    assert all(v > 0 for v in old | new), (old, new)
    assert old <= new, "variants no saturated case reaches: %s" % sorted(old - new)


def test_dwproj_cases_reach_all_four_instances():
    import ctypes as C
    from iip_uavsal_saliency_amd import _lib as L
    seen = set()
    for l in LAUNCHES:
        if l.family == "dwproj":
            seen.add(int(L.load().uavsal_conv_dwproj(C.byref(A.conv_desc(l)))))
    assert seen == {256, 128, 64, 32}, seen


@pytest.mark.parametrize("lch", [l for l in LAUNCHES if l.op in ("conv", "dwgemm")], ids=repr)
def test_gemm_launches_take_their_routes(lch):
    """(the stream-K family is not asked here: its grid comes from the occupancy query, which needs a device)"""
    from iip_uavsal_saliency_amd import _lib as L
    if lch.family == "conv/streamk":
        return
    rt = L.conv_route(L.load(), A.conv_desc(lch))._asdict()
    assert A.route_matches(rt, lch.route), (lch, rt)
    if lch.family == "conv/dwloader":
        assert rt["family"] != L.ROUTE_DWPROJ or lch.key[6] == 1, rt
