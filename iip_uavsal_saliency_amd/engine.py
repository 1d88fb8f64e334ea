"""Host side of the HIP path: turns a `UAVSal` parameter tree into a native launch plan.

Built once per (device, clip count, sequence length, frame size, precision):
  1. folds every BatchNorm and packs every conv weight, uploads them (weights.py, packing.py);
  2. lays the NHWC fp32 activation buffers out in HBM (concatenations become channel
     slices of one wider buffer; buffers share one arena by liveness: arena.py);
  3. records every kernel launch of reference `UAVSal.forward` (model.py:341-375) into a
     `uavsal_plan` (C ABI, include/uavsal_hip.h) that is then replayed natively --
     as a launch loop or as one captured hipGraph.
`run()` only stages the caller's tensors and launches the plan on torch's current
stream.  PyTorch is used for device memory and streams, not for arithmetic (one exception, off the hot path: the call that runs
the prior nets compares the prior frames with their source frames, `PriorCache.compare_frames`).
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Dict, Optional

import torch

from . import _lib as L
from .arena import ARENA_ALIGN, Arena, _ArenaRef, arena_conflict, plan_arena      # (the planner's names and the views' stay
from .views import OpView, V, _down, read_view                                    # importable from here)
from .recorder import PRIOR_GROUP, Recorder
from .topology import record_forward
from .weights import WeightCache


class PriorCache:
    """The prior nets run once per prior tensor, not once per call: everything recorded on their side lane, with its fork and
    its join (`ops`), is one group of the native plan that a run leaves out while the caller's prior tensors are the ones the
    nets last ran on.  Holds whether the group is marked / switched off in the plan, the record of the run that last executed
    it (`rec`: sig, bound, confirmed) and the record the call in progress is putting together (`new`: sig, bound; None when
    the call is not to be remembered)."""

    def __init__(self, lib, plan, ops):
        self.lib, self.plan, self.ops = lib, plan, sorted(ops)
        self.marked = self.off = False
        self.rec = self.new = None
        self.group_launches = 0

    def mark(self):
        """Hands the prior group to the native plan (once, before the plan first runs) -- as ranges of consecutive ops."""
        if self.marked:
            return
        self.marked = True
        ops = self.ops
        i = 0
        while i < len(ops):
            j = i
            while j + 1 < len(ops) and ops[j + 1] == ops[j] + 1:
                j += 1
            L.check(self.lib.uavsal_plan_group_mark(self.plan, PRIOR_GROUP, ops[i], ops[j] + 1), "plan_group_mark")
            i = j + 1
        self.group_launches = int(self.lib.uavsal_plan_group_launches(self.plan, PRIOR_GROUP)) if ops else 0

    def gate(self, sig, check) -> bool:
        """May the call whose prior tensors are `sig` (Engine._prior_sig; None: never cached) leave the prior group out?  Only
        if a completed, error-free run of this plan executed the group on the very tensors `sig` names -- same objects, same
        version -- since the plan was built (its output then still stands in the pinned buffers, Arena.pin).  `check()`
        waits for that run and drops the record if it reported a device error.  Sets the group's switch in the native plan
        accordingly; the call's launches then go inside `launches()`, which closes the record."""
        self.mark()
        self.new = None
        if not self.ops:
            return False
        skip = False
        rec = self.rec
        if sig is not None and rec is not None and len(rec["sig"]) == len(sig) and all(
                a[0] is b[0] and a[1:] == b[1:] for a, b in zip(rec["sig"], sig)):
            if not rec["confirmed"]:
                check()                         # (raises, and drops the record, if that run reported a device error)
            skip = self.rec is not None
        if not skip:
            self.rec = None                     # replaced once this run is launched
            self.new = None if sig is None else dict(sig=sig, bound={})
        if skip != self.off:
            L.check(self.lib.uavsal_plan_group_enable(self.plan, PRIOR_GROUP, 0 if skip else 1), "plan_group_enable")
            self.off = skip
        return skip

    def note(self, bound):
        """The prior tensors {caller name: tensor} the call in progress binds: the contiguous forms the plan reads, which must
        stay alive while they may be bound."""
        if self.new is not None:
            self.new["bound"].update(bound)

    def compare_frames(self, src_idx):
        """Frame repeat (Engine._arm_repeat): the call in progress runs the prior nets, so it also finds out whether every
        frame f of each prior tensor it bound equals, element for element, its source frame `src_idx[f]` (a device index
        tensor).  Started on the current stream in FRONT of the run's launches -- a later call that may leave the group out
        has waited for this run (`gate`) and so for the answer -- into a pinned host word behind an event: nobody waits for
        it.  NaN compares unequal.  One frame (the static-priors plan: a zero frame stride) is every frame without looking."""
        if self.new is None:
            return
        ts = [t for t in self.new["bound"].values() if t.shape[0] > 1]
        if not ts:
            self.new["same"] = True
            return
        ok = None
        for t in ts:
            e = (t == t.index_select(0, src_idx)).all()
            ok = e if ok is None else ok & e
        word = torch.zeros(1, dtype=torch.bool).pin_memory()
        word.copy_(ok.reshape(1), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.new["same"] = (ev, word)

    def frames_repeat(self) -> bool:
        """Did the run the record comes from find every prior frame identical to its source frame?  False while that is not
        known yet (no wait)."""
        s = self.rec.get("same") if self.rec is not None else None
        if isinstance(s, tuple):
            ev, word = s
            if not ev.query():
                return False
            s = self.rec["same"] = bool(word[0])
        return s is True

    def bound(self):
        """{caller name: tensor} the group last ran on (a call that leaves the group out keeps them bound)."""
        return self.rec["bound"]

    @contextlib.contextmanager
    def launches(self):
        """Around the launches of a call that went through `gate`: once they are all issued, the tensors the prior group
        ran on become the record; if issuing them fails there is no record at all."""
        try:
            yield
        except Exception:
            self.rec = self.new = None
            raise
        if self.new is not None:
            self.rec = dict(self.new, confirmed=False)
            self.new = None

    def confirm(self):
        if self.rec is not None:
            self.rec["confirmed"] = True

    def drop(self):
        self.rec = None


class Engine:
    def __init__(self, model, device, n_seq, seq_len, H, W, ctx_T, ctx_mode="tile",
                 precision="f32", taps=False, in_dtype=torch.float32, use_graph=False, fuse_dw=None,
                 use_lanes=True, stream_k=True, sync_errors=True, persistent=False,
                 wcache=None, static_priors=False, plan_only=False):
        """`plan_only`: sizing pass and arena placement only -- no device, nothing allocated, nothing recorded (memory planning
        questions and the CPU tests of the arena: `arena_stats`, `arena_layout()`)."""
        if precision not in L.PREC:
            raise ValueError("precision must be one of %s" % list(L.PREC))
        self.lib = L.load()
        self.device = torch.device(device)
        self.plan_only = bool(plan_only)
        if self.device.type != "cuda" and not self.plan_only:
            raise RuntimeError("Engine needs a cuda (ROCm) device; there is no CPU fallback")
        self.model, self.n_seq, self.seq_len = model, n_seq, seq_len
        self.N = n_seq * seq_len
        self.H, self.W = H, W
        self.ctx_T, self.ctx_mode = ctx_T, ctx_mode
        self.prec_name, self.prec = precision, L.PREC[precision]
        self.keep_taps = taps
        self.in_dtype = in_dtype
        # the caller's priors are ONE map set for every frame (what the reference's own caller builds: np.repeat of the prior
        # file over b_s frames, utils_data.py:466-467, 601-602; recognised by the model from a zero frame stride, never from the
        # values): the two prior nets run on one frame and their output is broadcast over the frames
        self.static_priors = bool(static_priors)
        self.use_graph = use_graph
        self.stream_k = bool(stream_k)
        # device-side errors (a stream-K hand-off that timed out) are never silent: the guard op at the end of
        # the plan overwrites the outputs with NaN, and `run` raises -- before it returns when `sync_errors`
        # (one event wait per call), else at the next call / `check()` once the run is known to be over
        self.sync_errors = bool(sync_errors)
        self._first_run_verified = False
        self._sk_debug = tuple(getattr(model, "_sk_debug", (0, 0)))
        # fused depthwise->projection GEMM (uavsal_conv_desc.dw_*): D never reaches HBM.
        #   None (default): the LDS-halo kernel (dwproj_kernel, fp32 and f16x3) on the blocks where it wins -- stride 1,
        #     dilation 1, hidden % 16 == 0 and at least FUSE_DW_MIN_WORK expanded values (the 45x80 / 90x160 dwBlocks
        #     of the head and the decoder: profiles/r2_dwproj.md); other precisions keep the three-launch form;
        #   True: every dilation-1 block with an expand conv (strides 2 and the 16-bit precisions then run the
        #     round-1 register-staged loader, which is correct but ~1.5x slower: tests only);  False: never.
        self.fuse_dw = fuse_dw if fuse_dw is None else bool(fuse_dw)
        if self.N % ctx_T:
            raise RuntimeError("frame count %d is not a multiple of time_dims %d" % (self.N, ctx_T))
        self.h = _down(_down(_down(H)))
        self.w = _down(_down(_down(W)))
        # packed device weights, keyed by (kind, id(module), ...): one copy per model, shared by its engines
        self.weights = WeightCache(self.device, wcache if wcache is not None else {})
        self.lstm = getattr(model, "rnn_type", "twa") == "lstm"      # the recurrence: ConvLSTM, else ConvTWA
        # persistent-state mode: the recurrent state lives in `hprev` (NHWC) across calls, see run()
        self.persistent = bool(persistent)
        # f16x3: tensors that an eligible GEMM consumes are ALSO kept as split shadows (hi/lo fp16 planes) written
        # by their producers, so that GEMM stages both operands by LDS-DMA with no conversion work.  The sizing
        # pass finds out which buffers are wanted (`Recorder.split_want`) and which cannot have one because a producer
        # does not write shadows (`Recorder.no_shadow`).
        presplit = getattr(model, "presplit", None)
        # per-layer precision (diagnostics: profiles/r4_precision.md): {op-name prefix: precision}, longest prefix wins; the
        # GEMM of that op (and the weights packed for it) then run in that precision, everything else in the plan's
        self.prec_overrides = dict(getattr(model, "prec_overrides", None) or {})
        for v in self.prec_overrides.values():
            if v not in L.PREC:
                raise ValueError("prec_overrides: unknown precision %r" % (v,))
        self.split_mode = (precision == "f16x3" and not self.prec_overrides
                           and (bool(presplit) if presplit is not None else n_seq >= 4))
        # exact-fp32 mode: the dense 3x3 convs (conv_last, the ConvTWA gate conv) as Winograd F(2x2, 3x3)
        # (model.winograd, default on; the per-step convolutions of the recurrence too)
        self.winograd = (precision == "f32" or bool(getattr(model, "prec_overrides", None))) and bool(getattr(model, "winograd", True))
        # output tile of the transforms: 2 = F(2x2, 3x3), 4 = F(4x4, 3x3); for the all-frames convs / for the recurrence steps
        # NOTE: with the defaults the arithmetic of "exact fp32" depends on the number of clips in the call -- F(2x2) steps below
        # four clips, F(4x4) (coefficients up to 8, ~20x less accurate per conv, map moves by ~5e-5) from four up -- so the same
        # clip gives maps that differ by ~1e-4 when batched differently (all inside the 5e-4 gate).  `model.winograd_r = 2`
        # (also for the steps) is the strict setting: F(2x2) everywhere, whatever the batch; `model.winograd = False`: direct.
        self.winograd_r = int(getattr(model, "winograd_r", None) or 4)
        self.winograd_step_r = int(getattr(model, "winograd_step_r", None)
                                   or (2 if getattr(model, "winograd_r", None) == 2 else 0))   # 0: by the number of clips
        self.fuse_blocks = bool(getattr(model, "fuse_blocks", True))
        # which priors this model has (reference model.py:281-324: a disabled prior has no net)
        self.use_priors = tuple(bool(getattr(model, a, 1)) for a in ("use_gauss_prior", "use_ob_prior", "use_context_prior"))
        # launch-loop mode reads the caller's tensors in place and writes straight into fresh outputs
        # (uavsal_plan_patch_ptr); a captured graph replays fixed addresses and keeps the staging copies
        self.inplace = not use_graph
        self._bound_t: Dict[str, torch.Tensor] = {}     # what `_bind_in_place` bound last, by caller name (kept alive here)
        self.priors = None                              # the prior cache (PriorCache), once the plan is recorded
        # activation arena (liveness-based, arena.py): see Recorder.buf / _size
        self.use_arena = bool(getattr(model, "arena", True))
        self.arena_debug = bool(getattr(model, "arena_debug", False))
        # (the recorder allocates through this module's `torch`: what tests/mock_plan.py replaces to record on the host)
        self.rec = Recorder(torch, self.lib, self.device, self.weights, precision, self.prec_overrides, self.split_mode, self.stream_k,
                            self._sk_debug, self.fuse_dw, self.fuse_blocks, self.use_arena, self.arena_debug)
        # everything below allocates on, or creates native objects for, the CURRENT device (the plan's error word, its
        # `done` event, workspaces, occupancy queries): make that the engine's device, whatever the caller's is
        if self.plan_only:
            self._size()
            return
        with torch.cuda.device(self.device):
            self._init_on_device(use_lanes)

    # what the recorder holds, read-only for everybody else
    plan = property(lambda self: self.rec.plan)
    ops_meta = property(lambda self: self.rec.ops_meta)
    op_args = property(lambda self: self.rec.op_args)
    _op_idx = property(lambda self: self.rec.op_idx)
    named = property(lambda self: self.rec.named)
    stage_ranges = property(lambda self: self.rec.stage_ranges)
    arena = property(lambda self: self.rec.arena)
    _scratch = property(lambda self: self.rec.scratch)
    _sk_ws = property(lambda self: self.rec.sk_ws)
    # the caller-side tensors of the plan (staging copies for a captured graph, shapes only for the launch loop)
    x_in = property(lambda self: self.rec.callers["x"])
    cb0_in = property(lambda self: self.rec.callers["cb0"])
    cb1_in = property(lambda self: self.rec.callers["cb1"])
    state_in = property(lambda self: self.rec.callers["state_in"])
    state_out = property(lambda self: self.rec.callers["state_out"])
    cstate_in = property(lambda self: self.rec.callers["cstate_in"])
    cstate_out = property(lambda self: self.rec.callers["cstate_out"])
    zero_state = property(lambda self: self.rec.callers["zero_state"])
    out = property(lambda self: self.rec.callers["out"])
    logits = property(lambda self: self.rec.callers.get("logits"))
    _prior_rec = property(lambda self: self.priors.rec)         # the record of the run that last executed the prior group
    prior_group_launches = property(lambda self: self.priors.group_launches if self.priors else 0)
    _arena = property(lambda self: self.arena.buf)              # the pool (one float32 tensor)
    arena_stats = property(lambda self: self.arena.stats)
    TAP_NAMES = ("c3", "c4", "c5", "sfnet", "st0", "st1", "fust_in_cb", "prefuse", "rnn")
    # kept like the taps, but read back only when the caller asks for them by handing a `taps` dict that already holds the
    # name (any value): fucbst_layer's whole input, as ONE channels-last copy (train.recurrence_step(fuse=True) reads it NHWC),
    # and fucb_layer's whole input, the concatenated prior maps (train.recurrence_step(fust=True))
    TAPS_ON_REQUEST = ("fu320", "cb192")

    def _size(self):
        """Pass 1: sizes the shared scratch and lays the arena out (nothing allocated, nothing recorded)."""
        self.rec.begin(dry=True)
        record_forward(self.rec, self)
        self.rec.place(self.TAP_NAMES + self.TAPS_ON_REQUEST if self.keep_taps else ())      # (what `tap` reads back after the run stays live to the end)

    def arena_layout(self):
        """[(buffer id, offset, floats, first op, last op, lane key, first / last op in recording order)], by offset."""
        return self.arena.layout()

    def _init_on_device(self, use_lanes, resume=False):
        """Pass 1, then pass 2: allocates what pass 1 sized and records the launches (`resume`: pass 1 already ran -- plan_only)."""
        if not resume:
            self._size()
        N, h, w = self.N, self.h, self.w
        f32, state = torch.float32, (self.n_seq, 256, h, w)
        # boundary tensors (NCHW, as the reference caller hands them over).  Launch-loop mode binds the caller's tensors into the
        # plan before every run: the frames and priors are then shapes only, and `launch` refuses to run a plan that was never bound
        stage = "shape" if self.inplace else "empty"
        np_ = 1 if self.static_priors else N
        callers = {"x": ((N, 3, self.H, self.W), self.in_dtype, stage), "cb0": ((np_, 8, h, w), f32, stage),
                   "cb1": ((np_, 20, h, w), f32, stage), "state_in": (state, f32, "zeros"),
                   "zero_state": (state, f32, "zeros"),                                            # never written
                   "state_out": (state, f32, "empty"), "cstate_in": (state, f32, "zeros"), "cstate_out": (state, f32, "empty"),
                   "out": ((N, h * w), f32, "empty")}
        if self.keep_taps:
            callers["logits"] = ((N, h * w), f32, "empty")
        rec = self.rec
        rec.allocate(callers)
        rec.begin(dry=False)
        record_forward(rec, self)
        rec.end()
        if self.persistent:      # what the caller gets back: channels-last views of the resident buffers
            self.h_view, self.c_view = (rec.named[k].t.view(self.n_seq, h, w, 256).permute(0, 3, 1, 2) if k in rec.named else None
                                        for k in ("h0", "c0"))
        self.priors = PriorCache(self.lib, rec.plan, rec.prior_ops)
        # frame repeat: the fusion block behind the priors (`fucb`, topology.py) reads cat[gauss, ob, ctx].  The context map
        # of frame f is that of frame (f // div * div) % mod (the map of `ctx.up`), so when the caller's priors repeat over
        # the frames in the same way the block's output does too, and its two launches compute the source frames only
        # (uavsal_plan_frame_repeat; `_arm_repeat`).  (pw op, dwpl op, mod, div), or None for a plan without that pair
        pw, dwpl = rec.op_idx.get("fucb.pw"), rec.op_idx.get("fucb.dwpl")
        self._fr = None
        if pw is not None and dwpl is not None and rec.ops_meta[pw]["kind"] == "conv1" and rec.ops_meta[dwpl]["kind"] == "conv1":
            self._fr = (pw, dwpl) + ((N // self.ctx_T, 1) if self.ctx_mode == "tile" else (N, self.ctx_T))
        self._fr_idx = None                  # source frame of every frame, on the device (built by the first miss)
        self.repeat_armed = False            # did the most recent run apply the mode?
        self._plan_recurrence_modes()
        self.use_lanes = bool(use_lanes)
        L.check(self.lib.uavsal_plan_enable_lanes(self.plan, 1 if self.use_lanes else 0), "plan_enable_lanes")
        self._graph_ready = False

    # ------------------------------------------------------------------ recurrence modes
    @staticmethod
    def _extent(v):
        """(first byte, one past the last) of the whole buffer a view lies in; None for a buffer outside the arena and the
        engine's own allocations (the caller's)."""
        t = v.t
        if isinstance(t, _ArenaRef):
            lo = t.arena.buf.data_ptr() + 4 * t.off
            return lo, lo + 4 * t.numel_
        if isinstance(t, torch.Tensor):
            return t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()
        return None

    def seam_conflicts(self, prev, nxt):
        """Names of the buffers the output transform of step `prev` reads or writes that the V planes of step `nxt` overlap
        (Recorder.twa_steps entries): a seam launch writes those planes while it runs that transform, so any is a refusal."""
        v = self._extent(nxt["v"])
        bad = []
        for k in ("m", "out", "a", "x", "pre"):
            e = self._extent(prev[k])
            if v is None or (e is not None and e[0] < v[1] and v[0] < e[1]):
                bad.append(k)
        return bad

    def _plan_recurrence_modes(self):
        """At plan build: which run-time modes of the native plan this plan can take.  `_seams`: the (xout of step t, xin of
        step t + 1) op pairs of an F(2x2) ConvTWA recurrence that are neighbours in the plan (a debug plan has poison fills
        between them) and whose V planes overlap nothing the output transform touches in the planned arena.  `_zs`: the ops
        of a zero initial state (state layouts first / last or -1, step 0's xin / gemm / xout).  Launch-loop plans only, and
        not the debug plans (`model.arena_debug`), which are there to run every recorded op; the pairs are handed to the
        native plan in front of the first run (`_arm_modes`)."""
        self._seams, self._zs = [], None
        self._seams_on = None                # what the native plan was told last (None: nothing yet)
        self._zs_rec = None                  # zero test of a caller's state tensor: dict(base, sig, zero = (event, pinned word) | bool)
        self.zero_armed = False
        steps = self.rec.twa_steps
        if self.lstm or not self.inplace or self.arena_debug or not steps or any(s["r"] != 2 for s in steps):
            return
        for a, b in zip(steps, steps[1:]):
            if b["xin"] == a["xout"] + 1 and not self.seam_conflicts(a, b):
                self._seams.append((a["xout"], b["xin"]))
        lay = [i for i, m in enumerate(self.ops_meta) if m.get("name") == "state.in"]
        s0 = steps[0]
        if s0["gemm"] == s0["xin"] + 1 and s0["xout"] == s0["gemm"] + 1:
            self._zs = ((lay[0], lay[-1]) if lay else (-1, -1)) + (s0["xin"], s0["gemm"], s0["xout"])

    def _state_is_zero(self, state) -> bool:
        """Is the state this call binds known to be all +0 bits?  None is (the engine's own zeros, never written).  A caller's
        tensor goes by object and version, like the prior cache: the first call with it starts a device-side test of its bit
        pattern into a pinned host word behind an event and runs in full -- nobody waits; a later call with the same object
        and version says yes once the event is over and the word says zero.  -0.0 is not zero here: (1 - g) * -0 has the
        other sign."""
        if state is None:
            return True
        try:
            base = state._base if state._base is not None else state
            sig = (state.data_ptr(), tuple(state.shape), tuple(state.stride()), state._version)
        except RuntimeError:
            return False
        if state.dtype != torch.float32 or state.device != self.device:
            return False
        r = self._zs_rec
        if r is not None and r["base"] is base and r["sig"] == sig:
            if isinstance(r["zero"], tuple):
                ev, word = r["zero"]
                if not ev.query():
                    return False
                r["zero"] = bool(word[0])
            return r["zero"]
        src = state if state.is_contiguous() else state.contiguous()
        ok = (src.view(torch.int32) == 0).all()
        word = torch.zeros(1, dtype=torch.bool).pin_memory()
        word.copy_(ok.reshape(1), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._zs_rec = dict(base=base, sig=sig, zero=(ev, word))
        return False

    def invalidate_zero_state(self):
        """Forget what is known about the caller's state tensor: the next call with it runs in full and tests it again."""
        self._zs_rec = None

    def _arm_modes(self, zero):
        """In front of a call's launches: hands the seam pairs to the native plan (when `model.fuse_seams`, default on, changes)
        and switches the zero-state mode on for this run when `zero` (the state step 0 reads is all +0 bits) and
        `model.skip_zero_state` (default on).  `_disarm_modes` follows the launches."""
        self.zero_armed = False
        want = bool(getattr(self.model, "fuse_seams", True))
        if self._seams and want != self._seams_on:
            for xo, xi in self._seams:
                r = self.lib.uavsal_plan_seam(self.plan, xo, xi, 1 if want else 0)
                if r < 0:
                    L.check(r, "plan_seam")
            self._seams_on = want
        if zero and self._zs is not None and bool(getattr(self.model, "skip_zero_state", True)):
            r = self.lib.uavsal_plan_zero_state(self.plan, *self._zs, 1)
            if r < 0:
                L.check(r, "plan_zero_state")
            self.zero_armed = r == 1

    def _disarm_modes(self):
        """Behind a call's launches: whatever runs next on another state, or as ranges of its own, runs step 0 in full."""
        if self.zero_armed:
            self.lib.uavsal_plan_zero_state(self.plan, *self._zs, 0)

    def mode_report(self):
        """(seam pairs fused, ops left out by the zero state, launch calls issued) of the most recent run of the plan."""
        out = (C.c_int * 4)()
        L.check(self.lib.uavsal_plan_mode_report(self.plan, C.byref(out)), "plan_mode_report")
        return int(out[0]), int(out[1]), int(out[2])

    def __del__(self):
        try:
            if getattr(self, "plan", None) and not getattr(self, "plan_only", False):
                self.lib.uavsal_plan_destroy(self.plan)
                self.rec.plan = None
        except Exception:
            pass

    def bound(self, name) -> torch.Tensor:
        """The caller-side tensor an OpView names ("x", "cb0", "cb1", "out", "state_in", "state_out", "cstate_in",
        "cstate_out"): what `run` bound into the plan last (launch loop), or the staging tensor (graph)."""
        return self._bound_t[name] if self.inplace else self.rec.callers[name]

    # ------------------------------------------------------------------ execution
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _prior_sig(self, srcs):
        """What identifies the caller's prior tensors of a call: per used prior the tensor object (of a view: its base, with
        the view's address, shape and strides) and torch's version counter, which every in-place operation on the tensor or on
        any view of it advances.  None when a tensor has no version counter (inference tensors): such a call is never cached."""
        sig = []
        for t, on in zip(srcs, self.use_priors[:2]):
            if not on:
                continue
            try:
                base = t._base if t._base is not None else t
                sig.append((base, t.data_ptr(), tuple(t.shape), tuple(t.stride()), t._version))
            except RuntimeError:
                return None
        return sig

    def drop_prior_record(self):
        """Forget the run the prior nets' output in the arena comes from: the next call runs them again."""
        self.priors.drop()

    def _prior_gate(self, srcs) -> bool:
        """May this call leave the prior group out (PriorCache.gate)?  The call's launches then go inside `priors.launches()`."""
        sig = self._prior_sig(srcs) if (self.inplace and bool(getattr(self.model, "cache_priors", True))) else None
        return self.priors.gate(sig, lambda: self.check(wait=True))

    def _arm_repeat(self, skip):
        """In front of a call's launches (after the binding).  A miss -- the call runs the prior nets -- starts the comparison
        of the prior frames it bound and runs in full.  A hit arms the frame-repeat mode of the plan when that comparison is
        over and said "identical", `dedupe_priors` and `cache_priors` are on and the plan is a launch loop; the native side
        still refuses routes it cannot take (f16x3 plans, a three-launch block).  `_disarm_repeat` follows the launches."""
        self.repeat_armed = False
        if self._fr is None or not self.inplace:
            return
        pw, dwpl, mod, div = self._fr
        if not skip:
            if self._fr_idx is None:
                self._fr_idx = torch.tensor([(f // div * div) % mod for f in range(self.N)], dtype=torch.int64, device=self.device)
            self.priors.compare_frames(self._fr_idx)
        on = (skip and bool(getattr(self.model, "dedupe_priors", True)) and bool(getattr(self.model, "cache_priors", True))
              and self.priors.frames_repeat())
        r = self.lib.uavsal_plan_frame_repeat(self.plan, pw, dwpl, mod, div, 1 if on else 0)
        if r < 0:
            L.check(r, "plan_frame_repeat")
        self.repeat_armed = r == 1

    def _disarm_repeat(self):
        """Behind a call's launches: whatever runs next -- single ops, partial ranges, the per-op timer -- runs in full."""
        if self.repeat_armed:
            pw, dwpl, mod, div = self._fr
            self.lib.uavsal_plan_frame_repeat(self.plan, pw, dwpl, mod, div, 0)

    def repeat_workgroups(self):
        """(workgroups of `fucb.pw`, of `fucb.dwpl`) in the most recent run of the plan: fewer when the mode was applied."""
        return tuple(int(self.lib.uavsal_plan_frame_repeat_workgroups(self.plan, i)) for i in (0, 1))

    def last_launches(self) -> int:
        """Plan ops that launched in the most recent run of the plan (an op with a split-K reduction is two kernels, one op)."""
        return int(self.lib.uavsal_plan_last_launches(self.plan))

    def launch(self):
        """Launch the recorded plan once on torch's current stream (no staging, no sync)."""
        self.priors.mark()
        if self.use_graph:
            # the legacy default stream cannot be captured: capture and replay on a private
            # stream, fenced against torch's current stream on both sides
            cur = torch.cuda.current_stream(self.device)
            if not self._graph_ready:
                self._gstream = torch.cuda.Stream(self.device)
                self._gstream.wait_stream(cur)
                gs = C.c_void_p(self._gstream.cuda_stream)
                L.check(self.lib.uavsal_plan_run(self.plan, 0, -1, gs), "plan_run (warm-up)")
                self._gstream.synchronize()
                L.check(self.lib.uavsal_plan_graph_build(self.plan, gs), "plan_graph_build")
                self._graph_ready = True
            self._gstream.wait_stream(cur)
            L.check(self.lib.uavsal_plan_graph_launch(self.plan, C.c_void_p(self._gstream.cuda_stream)),
                    "plan_graph_launch")
            cur.wait_stream(self._gstream)
        else:
            if self.inplace and not self._bound_t:
                raise RuntimeError("launch-loop plan was never bound to the caller's tensors (Engine.run does that)")
            L.check(self.lib.uavsal_plan_run(self.plan, 0, -1, self._stream()), "plan_run")

    def _is_resident(self, t, view) -> bool:
        return (t is not None and view is not None and t.data_ptr() == view.data_ptr()
                and t.numel() == view.numel() and t.reshape(view.shape).stride() == view.stride())

    def _stage_state_persistent(self, state, cstate):
        """Persistent mode: the caller's state is already resident when it is the view `run` returned (or a
        detach of it, Demo_Test.py:86); None resets it (model_convlstm.py:356); any other tensor is loaded."""
        pairs = [(state, self.h_view, self.state_in, "h0")]
        if self.c_view is not None:
            pairs.append((cstate, self.c_view, self.cstate_in, "c0"))
        self._resident_zero = False
        for t, view, stage, name in pairs:
            if self._is_resident(t, view):
                continue
            buf = self.named[name]
            if t is None:
                buf.t.zero_()
                if name == "h0":
                    self._resident_zero = True           # a reset: step 0 reads all-zero bits
                continue
            stage.copy_(t.reshape(stage.shape))
            d = L.LayoutDesc()
            d.inp, d.out, d.n_img, d.C, d.HW, d.ld, d.to_nhwc, d.Cpad = (
                stage.data_ptr(), buf.ptr, self.n_seq, 256, self.h * self.w, 256, 1, 0)
            L.check(self.lib.uavsal_layout(C.byref(d), self._stream()), "uavsal_layout(state)")

    def _bind_in_place(self, x, cb0, cb1, state, cstate, lstm, skip_priors=False):
        """Point the plan at the caller's tensors and at freshly allocated outputs (no staging copies, no
        clones).  Non-contiguous inputs are made contiguous first; everything bound is kept referenced until
        the next call.  `skip_priors`: the prior group is left out of this run, its input slots stay as the run
        that last executed it left them (the record keeps those tensors alive)."""
        dev, callers = self.device, self.rec.callers
        bound = {"x": x.reshape(callers["x"].shape).contiguous()}
        if not skip_priors:
            for name, t, on in (("cb0", cb0, self.use_priors[0]), ("cb1", cb1, self.use_priors[1])):
                if not on:              # a prior this model does not have is never read (reference model.py:347-353)
                    continue
                if self.static_priors:      # (zero frame stride, checked by the model: frame 0 is every frame)
                    t = t[:1]
                bound[name] = t.reshape(callers[name].shape).contiguous()
            self.priors.note({k: bound[k] for k in ("cb0", "cb1") if k in bound})
        out = bound["out"] = torch.empty((self.N, self.h * self.w), dtype=torch.float32, device=dev)
        st = None
        if self.persistent:
            self._stage_state_persistent(state, cstate)
        else:
            shape = callers["state_in"].shape
            for nm, t in [("state", state)] + ([("cstate", cstate)] if lstm else []):
                bound[nm + "_in"] = callers["zero_state"] if t is None else t.reshape(shape).contiguous()
                bound[nm + "_out"] = torch.empty(shape, dtype=torch.float32, device=dev)
            st = (bound["state_out"], bound["cstate_out"]) if lstm else bound["state_out"]
        for name, op, slot, off in self.rec.binds:
            if name in bound:
                L.check(self.lib.uavsal_plan_patch_ptr(self.plan, op, slot, bound[name].data_ptr() + off), "plan_patch_ptr(%s)" % name)
        if skip_priors:
            bound.update(self.priors.bound())
        self._bound_t = bound
        return out, st

    def stage_inputs(self, x, cb0, cb1, state, cstate=None):
        self.x_in.copy_(x.reshape(self.x_in.shape))
        for t, stage, on in ((cb0, self.cb0_in, self.use_priors[0]), (cb1, self.cb1_in, self.use_priors[1])):
            if on:
                stage.copy_((t[:1] if self.static_priors else t).reshape(stage.shape))
        if self.persistent:
            return self._stage_state_persistent(state, cstate)
        if state is None:
            self.state_in.zero_()
        else:
            self.state_in.copy_(state.reshape(self.state_in.shape))
        if cstate is None:
            self.cstate_in.zero_()
        else:
            self.cstate_in.copy_(cstate.reshape(self.cstate_in.shape))

    def run(self, x, cb0, cb1, state=None, taps: Optional[dict] = None, cstate=None, prior_src=None):
        """`prior_src`: the caller's own prior tensor objects when `cb0` / `cb1` are forms the model derived from them (a
        reshape): the prior cache goes by the caller's objects."""
        if x.dtype != self.in_dtype:
            raise RuntimeError("engine built for %s frames, got %s" % (self.in_dtype, x.dtype))
        lstm = self.lstm
        with torch.cuda.device(self.device):
            self.check(wait=False)               # a previous asynchronous run that is over by now
            skip = self._prior_gate(prior_src if prior_src is not None else (cb0, cb1))
            if self.inplace:
                out, st = self._bind_in_place(x, cb0, cb1, state, cstate, lstm, skip)
            else:
                self.stage_inputs(x, cb0, cb1, state, cstate)
            self._arm_repeat(skip)
            modes = self.inplace and bool(self._seams or self._zs)      # (a plan without either: nothing to look at)
            if modes:
                self._arm_modes(self._resident_zero if self.persistent else self._state_is_zero(state))
            with self.priors.launches():
                try:
                    self.launch()
                finally:
                    self._disarm_repeat()
                    if modes:
                        self._disarm_modes()
            if self.sync_errors:
                self.check(wait=True)
            if not self._first_run_verified and self.split_mode:
                # once per plan (this first call is therefore synchronous even with sync_errors off): a split shadow
                # nobody wrote (see _buf) shows up as NaN in the maps.  Device errors are raised first, under their own
                # name: the guard's NaN fill after a stream-K time-out must not be reported as a missing shadow
                self._first_run_verified = True
                self.check(wait=True)
                res = out if self.inplace else self.out
                if bool(torch.isnan(res).any().item()) and not bool(torch.isnan(x.float()).any().item()):
                    raise RuntimeError("the first run of this plan produced NaN maps from finite frames: a split shadow "
                                       "was read that no producer wrote (Recorder.no_shadow is missing a buffer)")
            if not self.inplace:
                out = self.out.clone()
                if self.persistent:
                    st = None
                else:
                    st = self.state_out.clone()
                    if lstm:
                        st = (st, self.cstate_out.clone())
            if self.persistent:          # opt-in aliasing: views of the resident state, overwritten by the next call
                st = (self.h_view, self.c_view) if lstm else self.h_view
            if taps is not None:
                if not self.keep_taps:
                    raise RuntimeError("engine was built without taps")
                for k in self.TAPS_ON_REQUEST:
                    if k in taps:
                        if k not in self.named:
                            raise RuntimeError("this plan has no buffer %r to tap (a model without priors)" % k)
                        taps[k] = self.tap(k, channels_last=True)
                for k in self.TAP_NAMES:
                    if k in self.named:          # (no "fust_in_cb" in a model without priors)
                        taps[k] = self.tap(k)
                taps["logits"] = self.logits.clone().view(self.N, 1, self.h, self.w)
        return out, st

    def state_split(self) -> int:
        """Index of the first op that reads the recurrent state (the recurrence's first step; in resident-state mode nothing in
        front of it does): ops [0, state_split) of a forward do not depend on the previous forward of the same video."""
        for i, m in enumerate(self.ops_meta):
            if m.get("name", "").startswith(("twa.step0", "lstm.step0")):
                return i
        raise RuntimeError("plan has no recurrence step")

    def run_streamed(self, x, cb0, cb1, prev: Optional["Engine"] = None, prev_done: Optional[torch.cuda.Event] = None, reset=False):
        """One group of a VIDEO whose previous group ran (or is still running) on `prev` -- this engine or another replica's --
        in resident-state mode: everything in front of the recurrence is launched at once, then the launch stream waits for
        `prev_done`, takes over `prev`'s recurrent state (a device copy of the NHWC state buffer; `reset`: zeros -- the first
        group, model_convlstm.py:356) and runs the recurrence, the decoder and the guard.  The arithmetic of a group is that of
        `run` (same plan, same order per lane-less launch): maps are bit-identical to the sequential loop; what changes is that
        the head of group k + 1 overlaps the tail of group k (Demo_Test.py:75-86 runs them back to back)."""
        if not (self.persistent and self.inplace):
            raise RuntimeError("run_streamed needs the resident-state launch-loop plan (model.persistent_state = True, no graph)")
        lstm = self.lstm
        with torch.cuda.device(self.device):
            self.check(wait=False)
            skip = self._prior_gate((cb0, cb1))
            out, _ = self._bind_in_place(x, cb0, cb1, self.h_view, self.c_view, lstm, skip)      # (resident views: nothing is staged)
            split = self.state_split()
            self._arm_repeat(skip)
            with self.priors.launches():
                try:
                    L.check(self.lib.uavsal_plan_run(self.plan, 0, split, self._stream()), "plan_run(head)")
                finally:
                    self._disarm_repeat()
                cur = torch.cuda.current_stream(self.device)
                if prev_done is not None:
                    cur.wait_event(prev_done)
                for name in ("h0", "c0") if lstm else ("h0",):
                    mine = self.named[name].t
                    if reset:
                        mine.zero_()
                    elif prev is not None and prev is not self:
                        mine.copy_(prev.named[name].t)
                self._arm_modes(bool(reset))
                try:
                    L.check(self.lib.uavsal_plan_run(self.plan, split, -1, self._stream()), "plan_run(tail)")
                finally:
                    self._disarm_modes()
        return out

    def check(self, wait=True):
        """Raise if the most recent run reported a device-side error (its outputs were overwritten with NaN).
        `wait=False` only looks when that run is known to have finished."""
        code = self.lib.uavsal_plan_status(self.plan, 1 if wait else 0)
        if code == 0:
            if wait:
                self.priors.confirm()       # the run that executed the prior group is over, without an error
            return
        self.priors.drop()           # (the prior nets' GEMMs may be what failed: never reuse their output)
        if code == -5:
            # a piece published after its owner gave up would be consumed by the next launch: start clean
            torch.cuda.synchronize(self.device)
            for ws in self._sk_ws.values():
                ws[:65536].zero_()
            raise RuntimeError("UAVSal HIP path: a stream-K hand-off timed out on the device "
                               "(UAVSAL_ERR_STREAMK); the maps and state of that call are invalid (NaN-filled)")
        L.check(code, "uavsal_plan_status")

    def streamk_clean(self) -> bool:
        """True when the stream-K workspace's flag block is all zero, as every launch must leave it (a set
        word is a published piece that nobody collected, or a bounded wait that gave up).  Synchronises."""
        torch.cuda.synchronize(self.device)
        return all(int(ws[:65536].view(torch.int32).abs().sum().item()) == 0 for ws in self._sk_ws.values())

    def tap(self, name, channels_last=False) -> torch.Tensor:
        """NCHW copy of a named NHWC buffer (debug / parity tests); `channels_last`: the copy keeps the buffer's NHWC memory
        (shape NCHW, `torch.channels_last` strides), which costs no transposition."""
        v = self.named[name]
        base = v.t.tensor() if isinstance(v.t, _ArenaRef) else v.t
        t = base.view(v.n, v.h, v.w, v.ld) if base.numel() == v.n * v.h * v.w * v.ld else None
        if t is None:
            raise RuntimeError("tap %s is not a dense buffer" % name)
        t = t[..., v.coff:v.coff + v.c]
        return t.contiguous().permute(0, 3, 1, 2) if channels_last else t.permute(0, 3, 1, 2).contiguous()

    def run_ops(self, first, last):
        """Launch ops [first, last) once, flat on the current stream (no lanes, no staging): puts the activations an op reads
        back in place before it is timed by itself -- buffers share addresses by liveness."""
        if last > first:
            L.check(self.lib.uavsal_plan_run(self.plan, first, last, self._stream()), "plan_run")

    def time_ops(self, first, last, iters=10) -> float:
        """Average device milliseconds for ops [first,last) measured with hipEvents on the launch stream."""
        ms = C.c_float(0.0)
        L.check(self.lib.uavsal_plan_time(self.plan, first, last, iters, self._stream(), C.byref(ms)), "plan_time")
        return float(ms.value)

