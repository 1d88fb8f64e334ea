"""Repacking refreshed weights on the device (csrc/repack.hip, repack.py, `WeightCache.refresh_device`,
`UAVSal.refresh_weights(device=True)`, `stream.finetune_video(refresh="device")`) against the host packer: byte for byte,
the Winograd transforms byte for byte where the arithmetic is exact (r = 2 on the 2^-12 grid) and within one fp32 ulp
elsewhere -- tests/test_repack_cpu.py's docstrings say why."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from iip_uavsal_saliency_amd import _lib as L
from iip_uavsal_saliency_amd import ops, repack, synth, train
from iip_uavsal_saliency_amd.weights import WeightCache

import repack_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H_, W_, T_ = 96, 160, 4
STAGES = ("rnn", "decoder", "fuse", "fust", "ctx", "nets")
ALL = {s: True for s in STAGES[1:]}


def _tensors(v):
    return list(v.values()) if isinstance(v, dict) else list(v) if isinstance(v, tuple) else [v]


def _snapshot(store):
    """key -> clones (on the device) of the packed tensors of every weight entry of a store"""
    return {k: [t.clone() for t in _tensors(v)] for k, v in store.items() if isinstance(k, tuple) and k[0] != repack.TABLE_KIND}


def _compare(dev, host, what=""):
    """Every entry byte-equal; a Winograd entry may be one ulp apart.  Returns the Winograd keys that were not byte-equal."""
    assert list(dev) == list(host)
    off = []
    for k in dev:
        for a, b in zip(dev[k], host[k]):
            if torch.equal(a.view(torch.uint8).reshape(-1), b.view(torch.uint8).reshape(-1)):
                continue
            assert k[0] == "wino", "%s%r is not the host packer's bytes" % (what, k)
            d = RR.ulps(RR.raw(a), RR.raw(b))
            print("%swino %r: %d of %d elements one ulp apart" % (what, k[2:], int((d > 0).sum()), d.size))
            assert int(d.max()) <= 1, k
            off.append(k)
    return off


# ----------------------------------------------------------------------------------------------- 1. the kernel, kind by kind
def test_kernel_matches_the_host_packer_on_every_kind_and_layout():
    """The shapes of tests/test_repack_cpu.py.  The store is packed by the host packer, every packed tensor is then filled
    with NaN (all bytes 0xff: a NaN as float, as half and as bfloat16) and the device repack must bring back the same bytes --
    the zeros of the padding and the identity of the BatchNorm padding among them."""
    cache, mods, exact = RR.make_cases(DEV)
    want = _snapshot(cache.store)
    # (on a device store `dw_dot` keeps the one-channel projection's weight as a view of the parameter itself: that one
    # packed tensor IS its source, the repack copies it onto itself, and filling it would destroy the parameter)
    params = {p.data_ptr() for s in mods.values() for p in s.parameters(recurse=False)}
    alias = [(k, i) for k, v in cache.store.items() for i, t in enumerate(_tensors(v)) if t.data_ptr() in params]
    assert alias == [(next(k for k in cache.store if k[0] == "dwdot"), 3)]
    for v in cache.store.values():
        for t in _tensors(v):
            if t.data_ptr() not in params:
                t.view(torch.uint8).fill_(0xFF)
    n = cache.refresh_device(mods)
    assert n == len(want) == cache.refresh(mods, dry=True)
    got = _snapshot(cache.store)
    off = _compare(got, want)
    assert not set(off) & exact and all(k[3] == 4 for k in off)
    # the identity padding of a BatchNorm list whose channels are no multiple of 32
    s, b = cache.store[next(k for k in cache.store if k[0] == "bn" and k[-1] == 84)]
    assert s.numel() == 96 and bool((s[84:] == 1).all()) and bool((b[84:] == 0).all())
    # a second launch from the kept table gives the same bytes; nothing but the one table joined the store
    assert cache.refresh_device(mods) == n
    assert not _compare(_snapshot(cache.store), got)
    assert [k[0] for k in cache.store if k[0] == repack.TABLE_KIND] == [repack.TABLE_KIND]
    ents = repack.entries(cache, mods)
    print("%d entries, %d bytes, one launch of %d blocks" % (len(ents), sum(e.nbytes for e in ents), cache.store[next(k for k in cache.store if k[0] == repack.TABLE_KIND)].blocks))


# ------------------------------------------------------------------------------------------------------- 2. the whole store
def _model(r=None):
    from iip_uavsal_saliency_amd import UAVSal
    m = UAVSal(time_dims=T_, bias_type=[1, 1, 1])
    synth.load_synth_weights(m, 0)
    if r is not None:
        m.winograd_r = r
    with torch.no_grad():                                       # running statistics that are not the initial 0 and 1
        g = torch.Generator().manual_seed(11)
        for bn in (s for box in _all_mods(m) for s in box.modules() if isinstance(s, torch.nn.BatchNorm2d)):
            bn.running_mean.add_(0.05 * torch.randn(bn.running_mean.shape, generator=g))
            bn.running_var.mul_(1.0 + 0.2 * torch.rand(bn.running_var.shape, generator=g))
    return m.to(DEV).eval()


def _all_mods(m):
    return [m.rnn, m.conv_out_st, m.fucbst_layer, m.fust_layer, m.fucb_layer, m.cxt_cb_prior] + list(train.prior_nets(m).values())


def _trained(m):
    return [p for mod in _all_mods(m) for p in mod.parameters()]


@lru_cache(maxsize=None)
def _step_inputs():
    n = T_
    x = torch.from_numpy(synth.normalize_frames(synth.synth_frames_u8(n, H_, W_, 3))).to(DEV)
    cb = [torch.from_numpy(synth.gauss_priors(n, H_ // 8, W_ // 8)).to(DEV), torch.from_numpy(synth.ob_priors(n, H_ // 8, W_ // 8, seed=3)).to(DEV)]
    loc = synth.synth_fix_points(n, 90, 130, 12, 4)
    fmap = np.rint(synth.synth_fix_maps(loc, 6.0) * 255).astype(np.uint8)
    y, has = ops.prepare_gaze(torch.from_numpy(fmap).to(DEV), torch.from_numpy(loc).to(DEV), H_ // 8, W_ // 8)
    assert bool(has.all())
    return x, cb, y


def _perturb(m, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    with torch.no_grad():
        for p in _trained(m):
            p.add_(1e-3 * torch.randn(p.shape, generator=g, device=DEV))


def _stepped():
    m = _model()
    x, cb, y = _step_inputs()
    m(x, cb, None)
    train.recurrence_step(m, x, cb, None, y, **ALL)
    return m


def test_whole_store_after_one_step_matches_the_host_refresh():
    m = _stepped()
    store = m._wshared[DEV]
    assert {"w", "wT", "wTs", "wino", "bn", "bnstat", "dw", "dwdot"} <= {k[0] for k in store}
    engines = {k: id(e) for k, e in m._engines.items()}
    assert any(e._prior_rec is not None for e in m._engines.values())
    _perturb(m, 3)
    before = _snapshot(store)
    n = m.refresh_weights(*_all_mods(m), device=True)
    assert all(e._prior_rec is None for e in m._engines.values())                 # the prior record was dropped ...
    assert {k: id(e) for k, e in m._engines.items()} == engines                    # ... and no plan rebuilt
    dev = _snapshot(store)
    assert n == m.refresh_weights(*_all_mods(m)) > 20                              # the host path, into the same tensors
    host = _snapshot(store)
    assert {k: id(e) for k, e in m._engines.items()} == engines
    off = _compare(dev, host)
    print("%d entries refreshed, %d Winograd entries not byte-equal" % (n, len(off)))
    moved = [k for k in dev if any(not torch.equal(a, b) for a, b in zip(dev[k], before[k]))]
    assert len(moved) > n // 2                      # the refresh did write (the BatchNorm statistics' entries alone have nothing new)
    # a parameter that was REPLACED (a new address behind the same Parameter) rebuilds the table, and the bytes still match
    key = next(k for k in store if k[0] == repack.TABLE_KIND)
    table = store[key]
    p = m.rnn.cell_list[0].rnn_conv.weight
    p.data = p.data.clone()
    _perturb(m, 4)
    assert m.refresh_weights(*_all_mods(m), device=True) == n and store[key] is not table
    dev = _snapshot(store)
    again = store[key]
    assert m.refresh_weights(*_all_mods(m)) == n
    _compare(dev, _snapshot(store))
    _perturb(m, 5)                                  # nothing moved: the table is kept
    assert m.refresh_weights(*_all_mods(m), device=True) == n and store[key] is again
    dev = _snapshot(store)
    m.refresh_weights(*_all_mods(m))
    _compare(dev, _snapshot(store))


# ------------------------------------------------------------------------------------------------------ 3. finetune_video
def _video(groups):
    n = T_ * groups
    frames = torch.from_numpy(synth.synth_frames_u8(n, H_, W_, 2)).to(DEV)
    gp = torch.from_numpy(synth.gauss_priors(1, H_ // 8, W_ // 8)[0]).to(DEV)
    op_ = torch.from_numpy(synth.ob_priors(1, H_ // 8, W_ // 8)[0]).to(DEV)
    loc = synth.synth_fix_points(n, 90, 130, 12, 9)
    fmap = np.rint(synth.synth_fix_maps(loc, 6.0) * 255).astype(np.uint8)
    return frames, gp, op_, torch.from_numpy(fmap).to(DEV), torch.from_numpy(loc).to(DEV)


def _host_packing(store, mods):
    """The host packer's bytes for the CURRENT parameters of `mods`, made OUT OF PLACE: `WeightCache.refresh` writes into a
    shadow store of clones, never into the model's store -- one of whose tensors (the `dwdot` projection weight) is a view of
    a parameter, so that a write through it would move the parameter's version counter and make the next call drop every
    plan.  Returns (the model's tensors, the shadow's) for the touched keys, as `_snapshot` does."""
    keys = repack.touched_keys(store, mods)

    def clone(v):
        return {n: t.clone() for n, t in v.items()} if isinstance(v, dict) else tuple(t.clone() for t in v) if isinstance(v, tuple) else v.clone()
    shadow = {k: clone(store[k]) for k in keys}
    assert WeightCache(DEV, shadow).refresh(mods) == len(keys)
    return {k: _tensors(store[k]) for k in keys}, {k: _tensors(shadow[k]) for k in keys}


def test_two_runs_of_finetune_video_host_and_device():
    """Three groups, six stages, Adam with the reference's settings, winograd_r = 2.  After EVERY group the device run's store
    is compared with the host packing of its current parameters, made out of place (`_host_packing`): nothing the run reads is
    written by the check.  In the device run no plan may be dropped or rebuilt and the table must be the one the first group
    built: the forwards of groups 2 and 3 read what the kernel wrote.  When every Winograd entry was byte-equal throughout,
    the two runs are the same computation: losses and final parameters bit for bit."""
    from iip_uavsal_saliency_amd.stream import finetune_video
    video = _video(3)
    with pytest.raises(ValueError, match="refresh"):
        finetune_video(_model(), *video, None, batch_size=1, stages=STAGES, refresh="gpu")
    runs, off = {}, []
    for how in ("host", "device"):
        m = _model(r=2)
        opt = torch.optim.Adam(_trained(m), lr=1e-4, betas=(0.9, 0.999), weight_decay=5e-5)
        real, calls, seen = m.refresh_weights, [], []

        def spy(*mods, device=False, m=m, real=real, calls=calls, seen=seen):
            n = real(*mods, device=device)
            calls.append(device)
            assert n > 20                                                       # (0: the plans were dropped instead)
            store = m._wshared[DEV]
            tables = [v for k, v in store.items() if k[0] == repack.TABLE_KIND]
            seen.append(({k: id(e) for k, e in m._engines.items()}, [id(t) for t in tables], id(store)))
            if device:
                assert len(tables) == 1
                off.extend(_compare(*_host_packing(store, {id(s): s for b in mods for s in b.modules()}), "group %d: " % len(calls)))
            assert m._weights_version() == m._wversion                          # the check moved no version counter
            return n
        m.refresh_weights = spy
        res = finetune_video(m, *video, opt, batch_size=1, stages=STAGES, refresh=how)
        assert res["groups_run"] == 3 and calls == [how == "device"] * 3
        assert seen[0] == seen[1] == seen[2], "a plan, the store or the table was replaced between groups"
        assert {k: id(e) for k, e in m._engines.items()} == seen[0][0] and id(m._wshared[DEV]) == seen[0][2]
        runs[how] = ([float(v) for v in res["losses"].tolist()], [p.detach().clone() for p in _trained(m)])
    print("losses: host %r, device %r; %d Winograd entries not byte-equal" % (runs["host"][0], runs["device"][0], len(off)))
    assert all(a != b for a, b in zip(runs["device"][0], runs["device"][0][1:]))  # the weights did move from group to group
    if off:
        pytest.skip("a Winograd entry differed from the host packer's by one ulp (%r): the runs are not compared bit for bit" % (off[0],))
    assert runs["host"][0] == runs["device"][0]
    assert all(torch.equal(a, b) for a, b in zip(runs["host"][1], runs["device"][1]))


# ------------------------------------------------------------------------------------------------------- 4. what is refused
def test_refresh_on_a_cpu_store_or_foreign_parameters_raises():
    cache, mods, _ = RR.make_cases("cpu")
    with pytest.raises(ValueError):
        cache.refresh_device(mods)
    m = _stepped()
    m._wshared["cpu"] = {}                                                          # a model that also holds a CPU store
    before = _snapshot(m._wshared[DEV])
    with pytest.raises(ValueError, match="CPU"):
        m.refresh_weights(m.rnn, device=True)
    del m._wshared["cpu"]
    # a parameter that is not fp32 on the store's device: raised while the table is built, before anything is written
    gpu, gmods, _ = RR.make_cases(DEV)
    kept = _snapshot(gpu.store)
    conv = next(s for s in gmods.values() if isinstance(s, torch.nn.Conv2d) and tuple(s.weight.shape[:2]) == (64, 120))
    conv.weight.data = conv.weight.data.double()
    with pytest.raises(ValueError, match="fp32"):
        gpu.refresh_device(gmods, dry=True)
    with pytest.raises(ValueError, match="fp32"):
        gpu.refresh_device(gmods)
    assert not _compare(_snapshot(gpu.store), kept) and not _compare(_snapshot(m._wshared[DEV]), before)
