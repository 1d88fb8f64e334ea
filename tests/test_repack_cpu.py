"""The device repack's table (repack.entries) and the restatement of its kernel (tests/repack_ref.py) against the host packer
(packing.py / weights.py), without a GPU: every kind and layout byte for byte, the Winograd transform byte for byte where the
arithmetic is exact and within one fp32 ulp elsewhere, and the walk over a whole recorded store against
`WeightCache.refresh(dry=True)` -- the same keys, the same exceptions."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import _lib as L
from iip_uavsal_saliency_amd import packing as P
from iip_uavsal_saliency_amd import repack
from iip_uavsal_saliency_amd.weights import WeightCache

import mock_plan
import repack_ref as RR


@lru_cache(maxsize=None)
def _cases():
    cache, mods, exact = RR.make_cases("cpu")
    return cache, mods, exact, repack.entries(cache, mods)


def _what(e):
    return "%s %s" % (e.key[0], e.layout_name if e.kind == L.REPACK_CONV else e.layout)


def test_entries_cover_what_refresh_counts():
    cache, mods, _, ents = _cases()
    keys = [k for k in cache.store]
    assert sorted({e.key for e in ents}, key=repr) == sorted(keys, key=repr)
    assert len({e.key for e in ents}) == cache.refresh(mods, dry=True) == len(keys)
    assert {k[0] for k in keys} == {"w", "wT", "wTs", "wino", "bn", "bnstat", "dw", "dwdot", "fused"}
    assert {e.layout_name for e in ents if e.kind == L.REPACK_CONV} == set(RR.LAYOUTS)
    assert repack.TABLE_KIND not in {"fused", "w", "wino", "wT", "wTs", "bn", "bnstat", "dw", "dwdot", "stem"}


def test_every_kind_and_layout_matches_the_host_packer_byte_for_byte():
    """The store was packed by packing.py / weights.py; the restatement of the kernel over the entries gives the same bytes."""
    cache, mods, _, ents = _cases()
    n = 0
    for e in ents:
        if e.kind == L.REPACK_WINO:
            continue
        assert np.array_equal(RR.pack(e), RR.raw(e.dst)), _what(e)
        n += 1
    assert n > 150
    shapes = {(e.N, e.C, e.taps) for e in ents if e.kind == L.REPACK_CONV and e.key[0] == "w" and len(e.src) == 1 and not e.gi}
    assert {(1, 8, 1), (20, 48, 1), (64, 120, 1), (256, 320, 1), (32, 32, 9), (64, 64, 9), (256, 128, 1), (64, 32, 9)} <= shapes
    assert any(e.gi == 8 and e.N == 32 for e in ents) and any(len(e.src) == 2 and e.kind == L.REPACK_CONV for e in ents)
    assert any(e.kind == L.REPACK_FOLD and e.N == 84 and e.Npad == 96 for e in ents)


def test_winograd_is_exact_on_the_grid_and_within_one_ulp_elsewhere():
    """r = 2 with weights that are multiples of 2^-12 in [-1, 1]: every product and partial sum is exact in double, so any
    order of summation gives the same double and the one rounding the same float -- byte-equal.  Otherwise (r = 4, normal
    weights) both sides round a double that lies a few 2^-53 (relative) from the same exact value: the floats are the same or
    neighbours."""
    cache, mods, exact, ents = _cases()
    winos = [e for e in ents if e.kind == L.REPACK_WINO]
    assert {e.P for e in winos} == {4, 6} and any(e.key in exact for e in winos)
    for e in winos:
        got, want = RR.pack(e), RR.raw(e.dst)
        d = RR.ulps(got, want)
        print("wino r=%d %dx%d: %.4f %% of the elements differ, worst %d ulp" % (e.P - 2, e.N, e.C, 100.0 * float((d > 0).mean()), int(d.max())))
        if e.key in exact:
            assert np.array_equal(got, want)
        assert int(d.max()) <= 1
        pad = np.ones((e.P * e.P, e.Npad, e.Kpad), bool)
        pad[:, :e.N, :e.C] = False
        assert not got.view(np.float32).reshape(pad.shape)[pad].any()


def test_the_winograd_constants_are_the_host_packers():
    cache, mods, _, ents = _cases()
    for e in ents:
        if e.kind == L.REPACK_WINO:
            assert e.G == [v for row in P._WINO_G[e.P - 2] for v in row]
    assert P._WINO_G[4][1][0] == -1 / 6 and float.hex(1 / 24) == "0x1.5555555555555p-5"


# ------------------------------------------------------------------------------------------------------ the whole-store walk
@lru_cache(maxsize=None)
def _recorded():
    from iip_uavsal_saliency_amd import UAVSal, synth
    m = UAVSal(time_dims=4, bias_type=[1, 1, 1])
    synth.load_synth_weights(m, 0)
    m.eval()
    eng, _ = mock_plan.record(m, n_seq=1, seq_len=4, H=96, W=160, ctx_T=4, ctx_mode="tile", precision="f32")
    return m, eng.weights


def _mods(*modules):
    return {id(s): s for m in modules for s in m.modules()}


def test_whole_store_walk_covers_the_keys_of_the_dry_refresh():
    """The forward plan of the whole model, recorded on the CPU (the mock records no training plan): the trained stages'
    keys are the keys `refresh(dry=True)` counts, entry for entry, and the restatement gives the store's own bytes."""
    m, cache = _recorded()
    from iip_uavsal_saliency_amd import train
    stages = [m.rnn, m.conv_out_st, m.fucbst_layer, m.fust_layer, m.fucb_layer, m.cxt_cb_prior] + list(train.prior_nets(m).values())
    mods = _mods(*stages)
    ents = repack.entries(cache, mods)
    keys = repack.touched_keys(cache.store, mods)
    assert len(keys) == cache.refresh(mods, dry=True) > 10
    assert [k for k in dict.fromkeys(e.key for e in ents)] == keys
    for e in ents:
        got, want = RR.pack(e), RR.raw(e.dst)
        if e.kind == L.REPACK_WINO:
            assert int(RR.ulps(got, want).max()) <= 1
        else:
            assert np.array_equal(got, want), _what(e)
    # module by module the two walks agree too
    for s in stages:
        one = _mods(s)
        assert len({e.key for e in repack.entries(cache, one)}) == cache.refresh(one, dry=True)


def _same_error(cache, mods):
    with pytest.raises(Exception) as host:
        cache.refresh(mods, dry=True)
    with pytest.raises(type(host.value)) as dev:
        repack.entries(cache, mods)
    assert str(dev.value) == str(host.value)
    return host.value


def test_the_same_inputs_raise_the_same_exceptions():
    m, cache = _recorded()
    stem_keys = [k for k in cache.store if isinstance(k, tuple) and k[0] == "stem"]
    assert stem_keys
    stem_mods = {i: s for i, s in _mods(m.sfnet).items() if i == stem_keys[0][1]}
    assert isinstance(_same_error(cache, stem_mods), NotImplementedError)
    # a transposed-layout fused block
    fused = [k for k in cache.store if isinstance(k, tuple) and k[0] == "fused" and not k[2]]
    if fused:
        mods = {i: s for i, s in _mods(m.sfnet).items() if i == fused[0][1]}
        assert isinstance(_same_error(cache, mods), NotImplementedError)
    small, mods, _, _ = _cases()
    fkey = next(k for k in small.store if k[0] == "fused")
    blk = next(s for s in mods.values() if hasattr(s, "expand_ratio") and id(list(s.conv)[0 if s.expand_ratio == 1 else 1][0]) == fkey[1])
    tr = WeightCache("cpu", {})
    tr.fused_block(blk, False)
    assert isinstance(_same_error(tr, _mods(blk)), NotImplementedError)
    # half of a joined key; a depthwise conv without its block
    joined = next(k for k in small.store if k[0] == "w" and len(k) == 6)
    assert isinstance(_same_error(small, {joined[1]: mods[joined[1]]}), RuntimeError)
    dwkey = next(k for k in small.store if k[0] == "dw" and len(k) == 2)
    assert isinstance(_same_error(small, {dwkey[1]: mods[dwkey[1]]}), RuntimeError)
    assert isinstance(_same_error(small, {fkey[1]: mods[fkey[1]]}), RuntimeError)


def test_refresh_device_refuses_a_cpu_store():
    cache, mods, _, _ = _cases()
    with pytest.raises(ValueError, match="CPU"):
        cache.refresh_device(mods)
    assert all(not (isinstance(k, tuple) and k[0] == repack.TABLE_KIND) for k in cache.store)
