"""Pinned arena buffers (Arena.pin, no GPU): a buffer that outlives the call -- the output of the prior nets, which a later call
with the same prior tensors reads without running the nets again -- has a range of its own, is never poison-filled, and
moves nothing else."""
from types import SimpleNamespace

from iip_uavsal_saliency_amd.arena import ARENA_ALIGN, Arena

rnd = lambda n: (n + ARENA_ALIGN - 1) // ARENA_ALIGN * ARENA_ALIGN

# (buffer, floats, [(logical op, lane), ...] uses): a main-lane chain whose neighbours overlap, two buffers private to side
# lane 1 (forked at op 2, joined at op 9), "keep" written on the lane and read on the main lane behind the join, and buffers
# with disjoint live ranges that today share addresses with one another and with "keep"
SEQ = [("a", 5000, [(0, 0), (1, 0)]),
       ("b", 3000, [(1, 0), (4, 0)]),
       ("l1", 2500, [(3, 1)]),
       ("l2", 2500, [(5, 1)]),
       ("keep", 4000, [(5, 1), (10, 0)]),
       ("c", 5000, [(4, 0), (6, 0)]),
       ("d", 1500, [(6, 0), (7, 0), (10, 0)]),
       ("e", 6000, [(11, 0), (12, 0)]),
       ("f", 4000, [(12, 0), (13, 0)]),
       ("g", 700, [(13, 0), (14, 0)]),
       ("whole", 900, [(0, 0), (14, 0)])]               # live from the first op to the last: shares with nobody
N_OPS, FORK, JOIN = 15, 2, 9


def _plan(pinned=()):
    """Sizing pass over SEQ, then the recording pass in debug mode: (arena, {buffer: offset}, [poisoned buffers])."""
    ar = Arena()
    refs = {name: ar.ref(name, n) for name, n, _ in SEQ}
    for dry in (True, False):
        if not dry:
            ar.begin(dry=False)
        poisoned = []
        for op in range(N_OPS):
            if not dry:
                poisoned += [r.aid for r, _ in ar.due()]
            ar.lop += 1
            if op == FORK:
                ar.fork(1)
            if op == JOIN:
                ar.join(1)
            for name, _, uses in SEQ:
                for at, lane in uses:
                    if at == op:
                        ar.lane = lane
                        ar.touch(SimpleNamespace(t=refs[name]))
                        ar.lane = 0
        if dry:
            for name in pinned:
                ar.pin(refs[name])
            ar.close(N_OPS)
            total = ar.place(N_OPS)
        else:
            poisoned += [r.aid for r, _ in ar.due(final=True)]
    return ar, {name: refs[name].off for name, _, _ in SEQ}, poisoned, total


def test_pinned_buffer_has_a_range_of_its_own_and_is_never_poisoned():
    ar0, off0, poison0, total0 = _plan()
    ar1, off1, poison1, total1 = _plan(pinned=("keep",))
    size = {name: n for name, n, _ in SEQ}
    # today "keep" shares its range with buffers it is never live together with, and is poison-filled behind its last use
    shares0 = [n for n in off0 if n != "keep" and not (off0[n] + rnd(size[n]) <= off0["keep"] or off0["keep"] + rnd(size["keep"]) <= off0[n])]
    assert shares0 and "keep" in poison0
    # pinned: its range intersects no other range, whatever the liveness ...
    lo, hi = off1["keep"], off1["keep"] + rnd(size["keep"])
    assert lo % ARENA_ALIGN == 0 and hi <= total1
    for n in off1:
        if n != "keep":
            assert off1[n] + rnd(size[n]) <= lo or hi <= off1[n], n
    # ... it is never in the poison list, and every other buffer still is, in the same order
    assert "keep" not in poison1 and poison1 == [n for n in poison0 if n != "keep"]
    # unpinned placement is unchanged from what the same sequence gives today
    assert {n: o for n, o in off1.items() if n != "keep"} == {n: o for n, o in off0.items() if n != "keep"}
    assert total1 == total0 + rnd(size["keep"])
    assert abs(ar1.stats["pinned_mb"] - 4 * rnd(size["keep"]) / 1e6) < 1e-9 and ar0.stats["pinned_mb"] == 0
    assert ar1.stats["pinned_extra_mb"] == ar1.stats["pinned_mb"]
    # and it counts as live to the end of the plan: `data_ptr` hands its address out to the last op
    assert [t for t in ar1.layout() if t[0] == "keep"][0][4] == N_OPS


def test_pinned_buffer_that_shares_with_nobody_stays_where_it_is():
    _, off0, poison0, total0 = _plan()
    size = {name: n for name, n, _ in SEQ}
    alone = [n for n in off0 if not any(m != n and off0[m] < off0[n] + rnd(size[n]) and off0[n] < off0[m] + rnd(size[m]) for m in off0)]
    assert alone
    for name in alone:
        ar1, off1, poison1, total1 = _plan(pinned=(name,))
        assert off1 == off0 and total1 == total0 and ar1.stats["pinned_extra_mb"] == 0
        assert name not in poison1 and poison1 == [n for n in poison0 if n != name]


def test_prior_net_outputs_are_pinned_in_the_real_plans():
    """Sizing pass of the real plans (`plan_only`): the concatenated prior maps (and the one-frame buffer of static priors)
    are pinned, disjoint from every other buffer; a model without prior nets pins nothing."""
    from iip_uavsal_saliency_amd import UAVSal
    from iip_uavsal_saliency_amd.engine import Engine
    kw = dict(n_seq=1, seq_len=4, H=96, W=160, ctx_T=4, ctx_mode="tile", plan_only=True)
    for bias, static, want in (((1, 1, 1), False, {"cb192"}), ((1, 0, 1), True, {"cb192", "cb_static"}),
                               ((0, 0, 1), False, set()), ((0, 0, 0), False, set())):
        e = Engine(UAVSal(time_dims=4, bias_type=list(bias)).eval(), "cpu", static_priors=static, **kw)
        pinned = {r.aid for r in e.arena.refs.values() if r.pinned}
        assert pinned == want, (bias, static, pinned)
        lay = e.arena_layout()
        for t in lay:
            if t[0] in want:
                for u in lay:
                    if u[0] != t[0]:
                        assert t[1] + rnd(t[2]) <= u[1] or u[1] + rnd(u[2]) <= t[1], (t[0], u[0])
        assert abs(e.arena_stats["pinned_mb"] - sum(4 * rnd(t[2]) for t in lay if t[0] in want) / 1e6) < 1e-9
        assert e.arena_stats["pinned_extra_mb"] <= e.arena_stats["pinned_mb"]
    # the headline plan (360x640, one clip of 8 frames): nothing shared the prior maps' range before, so they stay in place --
    # no address changes and the pool does not grow
    e = Engine(UAVSal(time_dims=8).eval(), "cpu", n_seq=1, seq_len=8, H=360, W=640, ctx_T=8, ctx_mode="clip", plan_only=True)
    assert e.arena_stats["pinned_extra_mb"] == 0 and abs(e.arena_stats["pinned_mb"] - 4 * 8 * 45 * 80 * 192 / 1e6) < 1e-9
