"""Everything a recorded launch plan consists of, as one canonical JSON document -- to prove that a change to the host side
(engine.py and what it is built from) left every plan as it was: record the document before and after, compare the bytes.

Plans are recorded on the CPU (tests/mock_plan.py: real shape queries, stubbed recording, nothing launched).  Per configuration
the document holds `ops_meta`, `op_args` (torch modules as their dotted name inside the model, `OpView`s as their `repr`),
`stage_ranges`, `arena_layout()`, `arena_stats`, every field of every descriptor handed to the plan in recording order (with
the arguments of the guard / fork / join / set_lane calls between them) and the weight cache as {key: sha256 of
the tensor bytes, dtype and shape}.  Every configuration that is not `persistent` is also bound once to zero-filled host
tensors of the plan's shapes, without a state (`Engine._bind_in_place`): `bind` holds the resulting patch_ptr calls as
(op, slot, pointer), sorted by (op, slot) -- their order within a call means nothing to the native plan.  Addresses differ from run to run, so a pointer field -- the `c_void_p` fields and arrays
of `_lib`'s structures -- is written as (owner, byte offset): the arena, a weight-cache key, a shadow or resident buffer's name,
a scratch key, a staging tensor's name, a bound tensor's name, a lane's stream-K workspace or the mock's error word.  A non-null pointer that
resolves to no owner is an error.

Configurations: the variants of tests/test_host_cpu.py::test_recording_pass_addresses_every_activation_inside_its_live_range
for its four `bias_type`s with `arena_debug` off and on, then `BASE` and `WALKS` of tests/plan_census.py.

  python tools/plan_fingerprint.py | sha256sum          (or: -o FILE, the digest then goes to stdout)

The document pins today's plans, kernel choices included: it is a tool for before / after comparisons, not a golden to commit."""
import bisect
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch

import mock_plan
import plan_census
from iip_uavsal_saliency_amd import UAVSal
from iip_uavsal_saliency_amd.engine import OpView

STAGING = ("x_in", "cb0_in", "cb1_in", "state_in", "zero_state", "state_out", "cstate_in", "cstate_out", "out", "logits")
BOUND = ("x", "cb0", "cb1", "out", "state_in", "state_out", "cstate_in", "cstate_out")
ERR_WORD = 4096                     # mock_plan.MockLib: uavsal_plan_error_word


def variant_configs():
    """(label, model arguments, arena_debug, Engine arguments) of the recording-pass test."""
    small = dict(H=96, W=160, ctx_T=4)
    for bias in ((1, 1, 1), (0, 0, 0), (1, 0, 1), (0, 1, 0)):
        variants = [dict(n_seq=1, seq_len=4, ctx_mode="tile", **small), dict(n_seq=1, seq_len=8, ctx_mode="tile", taps=True, **small),
                    dict(n_seq=2, seq_len=4, ctx_mode="clip", persistent=True, **small),
                    dict(n_seq=4, seq_len=4, ctx_mode="clip", precision="f16x3", **small),
                    dict(n_seq=1, seq_len=3, H=72, W=104, ctx_T=3, ctx_mode="clip", use_lanes=False)]
        if bias[0] or bias[1]:
            variants.append(dict(n_seq=1, seq_len=4, ctx_mode="clip", static_priors=True, **small))
        for kw in variants:
            for debug in (False, True):
                yield bias, debug, kw


def _extent(t):
    """[first, last) byte addresses that tensor `t` may address: from its first element to the end of its storage."""
    st = t.untyped_storage()
    return t.data_ptr(), st.data_ptr() + st.nbytes()


class Owners:
    """Maps an address to (owner, byte offset)."""

    def __init__(self):
        self.spans = {}

    def add(self, owner, t):
        if isinstance(t, torch.Tensor) and t.numel():
            self.spans.setdefault(_extent(t), owner)          # (one tensor under two names: the first one)

    def freeze(self):
        self.sorted = sorted(self.spans)
        for (_, hi), (lo, _) in zip(self.sorted, self.sorted[1:]):
            if lo < hi:
                raise RuntimeError("two owners overlap: %r" % ([self.spans[s] for s in self.sorted if s[0] <= lo < s[1]],))
        self.starts = [s[0] for s in self.sorted]

    def __call__(self, ptr):
        ptr = getattr(ptr, "value", ptr)
        if not ptr:
            return None
        if ptr == ERR_WORD:
            return ["err", 0]
        i = bisect.bisect_right(self.starts, ptr) - 1
        if i < 0 or ptr >= self.sorted[i][1]:
            raise RuntimeError("pointer %#x belongs to no owner" % ptr)
        return [self.spans[self.sorted[i]], ptr - self.sorted[i][0]]


def canon(v, names):
    """`v` with modules as dotted names, views as their repr, tuples as lists, dictionaries with text keys."""
    if isinstance(v, torch.nn.Module):
        return "module:" + names[id(v)]
    if isinstance(v, OpView):
        return repr(v)
    if isinstance(v, dict):
        return {str(canon(k, names)): canon(x, names) for k, x in v.items()}
    if isinstance(v, (list, tuple, set, frozenset)):
        return [canon(x, names) for x in (sorted(v, key=repr) if isinstance(v, (set, frozenset)) else v)]
    if isinstance(v, (torch.dtype, torch.device)):
        return str(v)
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    raise TypeError("no canonical form for %r" % (type(v),))


def key_text(key, names):
    return repr(tuple(names.get(k, k) if isinstance(k, int) and not isinstance(k, bool) else k for k in key))


def leaves(key_txt, val):
    """(owner name, tensor) of a weight-cache entry: a tensor, a tuple of tensors or a dictionary of tensors."""
    if isinstance(val, torch.Tensor):
        return [(key_txt, val)]
    items = val.items() if isinstance(val, dict) else enumerate(val)
    return [("%s[%s]" % (key_txt, i), t) for i, t in sorted(items, key=lambda kv: str(kv[0]))]


def desc_fields(d, resolve):
    out = {}
    for name, typ in d._fields_:
        v = getattr(d, name)
        if typ is C.c_void_p:
            out[name] = resolve(v)
        elif issubclass(typ, C.Array):
            out[name] = [resolve(x) for x in v] if typ._type_ is C.c_void_p else list(v)
        else:
            out[name] = v
    return out


def fingerprint(model, store, eng, mock):
    names = {id(mod): name or "<model>" for name, mod in model.named_modules()}
    own = Owners()
    own.add("arena", eng._arena)
    weights = {}
    for key, val in store.items():
        for owner, t in leaves(key_text(key, names), val):
            own.add("w:" + owner, t)
            weights[owner] = hashlib.sha256(repr((str(t.dtype), tuple(t.shape))).encode()
                                            + t.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()
    for name, v in eng.named.items():
        own.add("shadow:" + name, v.sp)
        own.add("buffer:" + name, v.t)                       # (a resident buffer outside the arena)
    for key, t in eng._scratch.items():
        own.add("scratch:%r" % (key,), t)
    for name in STAGING:
        own.add("stage:" + name, getattr(eng, name, None))
    for lane, t in eng._sk_ws.items():
        own.add("streamk:%d" % lane, t)
    if not eng.persistent:
        x, cb0, cb1 = (torch.zeros(t.shape, dtype=t.dtype) for t in (eng.x_in, eng.cb0_in, eng.cb1_in))
        eng._bind_in_place(x, cb0, cb1, None, None, eng.lstm)
        for name in BOUND:
            try:
                own.add("bound:" + name, eng.bound(name))
            except KeyError:
                pass
    own.freeze()
    calls, bind = [], []
    for name, a in mock.calls:
        if isinstance(a, C.Structure):
            calls.append([name, desc_fields(a, own)])
        elif name == "uavsal_plan_add_guard":
            calls.append([name, [own(x) if i % 2 == 0 else x for i, x in enumerate(a)]])
        elif name == "uavsal_plan_patch_ptr":
            bind.append([a[0], a[1], own(a[2])])
        else:
            calls.append([name, list(a)])
    return dict(ops_meta=canon(eng.ops_meta, names), op_args=canon(eng.op_args, names), stage_ranges=canon(eng.stage_ranges, names),
                arena_layout=canon(eng.arena_layout(), names), arena_stats=canon(eng.arena_stats, names), calls=calls,
                bind=sorted(bind, key=lambda b: b[:2]),
                weights=dict(sorted(weights.items())))


def document(log=None):
    doc = {}
    models = {}
    for bias, debug, kw in variant_configs():
        if bias not in models:
            torch.manual_seed(0)
            models[bias] = UAVSal(time_dims=4, bias_type=list(bias)).eval()
        m, store = models[bias], {}
        m.arena_debug = debug
        eng, mock = mock_plan.record(m, wcache=store, **kw)
        label = "variant bias=%r debug=%d %s" % (bias, debug, json.dumps(kw, sort_keys=True))
        doc[label] = fingerprint(m, store, eng, mock)
        if log:
            log(label)
    for cfg in plan_census.BASE + plan_census.WALKS:
        torch.manual_seed(0)
        m, store = plan_census.model_for(cfg)
        eng, mock = mock_plan.record(m, wcache=store, **plan_census.engine_kwargs(m, cfg))
        doc["census %r" % (cfg,)] = fingerprint(m, store, eng, mock)
        if log:
            log("census %r" % (cfg,))
    return json.dumps(doc, sort_keys=True, indent=0, allow_nan=False)


if __name__ == "__main__":
    text = document(log=(lambda s: print(s, file=sys.stderr, flush=True)) if "-v" in sys.argv else None)
    if "-o" in sys.argv:
        with open(sys.argv[sys.argv.index("-o") + 1], "w") as f:
            f.write(text + "\n")
        print(hashlib.sha256((text + "\n").encode()).hexdigest())
    else:
        print(text)
