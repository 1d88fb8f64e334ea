"""Turns "this op on these views" into entries of the native plan (`uavsal_plan`, include/uavsal_hip.h): one recorder method
per op kind fills the op's descriptor, its `ops_meta` and `op_args` entries, declares the op's buffers to the arena and --
where the descriptor holds the address of a caller-side tensor -- registers it in the bind table.  The only module that
allocates device memory while a plan is built.  A plan is recorded in two passes over the same topology (topology.py):
`begin(dry=True)` sizes the scratch and the arena, `allocate()` hands the result over, `begin(dry=False)` records."""
import ctypes as C
from typing import Dict, List, Optional

import torch

from . import _lib as L
from . import synth
from .arena import Arena, _ArenaRef
from .packing import conv_weight_layout, roundup
from .views import Caller, OpView, V, _Fake

# expanded values (pixels x hidden channels) from which the fused depthwise -> projection launch beats depthwise +
# projection launches (tools/dwproj_probe.py: 2 x 23 x 41 x 96 loses).  Round 2 had 8 x 45 x 80 x 512 here, which kept the
# 384-hidden blocks at 45x80 (temporal sub-blocks, prior nets) unfused at one clip: fused they take 29-32 us instead of 44-46
# (one clip fp32 4.521 -> 4.452 ms, f16x3 3.25 -> 3.19)
FUSE_DW_MIN_WORK = 1 << 20
# ... and the share of a map's 8 x 16 pixel patches that lies outside the map must be small: the kernel computes whole
# patches (45x80: 1.07, 23x40: 1.25, 12x20: 2.13).  Eight clips, fp32, features.8-17 on the 23x40 / 12x20 maps: 1259 us fused
# against 911 us as depthwise + projection launches (features.17 alone 282 vs 128)
FUSE_DW_MAX_WASTE = 1.15


# the mid-channel fused block kernel (csrc/fused_mid.hip): workgroups (4 x 8 output patches) of a launch for which it is taken
MID_MIN_WGS = 1
MID_MAX_WGS = 288


def _dwproj_patch_waste(h, w):
    return ((h + 7) // 8 * 8) * ((w + 15) // 16 * 16) / float(h * w)


BLOCK_CHUNK_BYTES = 6 << 30                                   # see Recorder.ir_block

# the two prior nets: everything recorded on their side lane, with its fork and its join, is one group of the native plan
# (uavsal_plan_group_mark) that a run leaves out while the caller's prior tensors are the ones the nets last ran on
PRIOR_LANE = 1
PRIOR_GROUP = 0


# `slot` of uavsal_plan_patch_ptr (include/uavsal_hip.h) per descriptor: which of its pointers a bind-table entry re-points
SLOT_CONV_A, SLOT_CONV_OUT = 0, 1              # conv and dw_dot
SLOT_STEM_F32, SLOT_STEM_U8 = 0, 1
SLOT_LAYOUT_IN, SLOT_LAYOUT_OUT = 0, 1         # (guard: slot i = its i-th buffer)


class Recorder:
    def __init__(self, alloc, lib, device, weights, precision, prec_overrides, split_mode, stream_k, sk_debug, fuse_dw, fuse_blocks,
                 use_arena, arena_debug):
        self.torch = alloc                     # the `torch` every allocation goes through
        self.lib, self.device, self.weights = lib, device, weights
        self.prec_name, self.prec, self.prec_overrides = precision, L.PREC[precision], prec_overrides
        self.split_mode, self.stream_k, self.sk_debug = split_mode, stream_k, sk_debug
        self.fuse_dw, self.fuse_blocks = fuse_dw, fuse_blocks
        self.use_arena, self.arena_debug = use_arena, arena_debug
        self.arena = Arena()
        self.plan, self.err = None, None
        # what the sizing pass finds out for the recording pass: the buffers some GEMM wants as split shadows and those that
        # cannot have one because a producer does not write shadows; the (kind, lane) scratch pools' sizes; the arena's size
        self.split_want, self.no_shadow = set(), set()
        self.scratch_need: Dict[tuple, int] = {}
        self.arena_floats = 0
        # device memory of the recording: scratch pools, one stream-K workspace per lane, the caller-side tensors by the name
        # OpView.buf / Engine.bound use, and everything else that must stay alive (resident state, shadows)
        self.scratch: Dict[tuple, torch.Tensor] = {}
        self.sk_ws: Dict[int, torch.Tensor] = {}
        self.callers: Dict[str, torch.Tensor] = {}
        self.keep: List[torch.Tensor] = []

    def begin(self, dry):
        """Start a pass over the topology -- the sizing pass (`dry`: nothing allocated, no plan) or the recording pass.  All
        per-pass state starts here, for both."""
        self.dry = dry
        self.lane = 0
        self.arena.begin(dry)
        self.ops_meta: List[dict] = []
        # op_args[i]: what op i of the native plan reads and writes (kind, torch modules, epilogue, OpView operands), filled by
        # the recorders in the recording pass -- Python references only (tests/test_plan_ops_fp64.py checks every launch with it)
        self.op_args: List[dict] = []
        self.op_idx: Dict[str, int] = {}
        self.stage_ranges: Dict[str, tuple] = {}
        self.named: Dict[str, V] = {}
        self.prior_ops: List[int] = []          # ops of the prior group (lane PRIOR_LANE, its fork and its join)
        # bind table: (caller name, op index, ABI slot, byte offset) of every caller-side address in a descriptor
        self.binds: List[tuple] = []
        # ConvTWA steps recorded as Winograd triples, in order: dict(name, r, xin / gemm / xout op indices, and the views the
        # output transform touches: v, m, out, a = h_{t-1}, x, pre) -- what the engine's recurrence modes go by
        self.twa_steps: List[dict] = []
        self._twa_prev = None                   # (op index of the last twa step's output transform, the views it touched)
        if not dry:
            self.plan = C.c_void_p(self.lib.uavsal_plan_create())
            if not self.plan:
                raise RuntimeError("uavsal_plan_create failed")
            self.err = self.lib.uavsal_plan_error_word(self.plan)

    def place(self, keep_names=()):
        """End of the sizing pass: lays the arena out; buffers named `keep_names` are read back after the run."""
        self.arena.close(len(self.ops_meta))
        if self.use_arena:
            keep = [self.named[k].t for k in keep_names if k in self.named]
            self.arena_floats = self.arena.place(len(self.ops_meta), [t for t in keep if isinstance(t, _ArenaRef)])

    def allocate(self, callers):
        """Between the passes: the pool the sizing pass placed, the scratch it sized and the caller-side tensors, `callers` =
        {name: (shape, dtype, "zeros" | "empty" | "shape")} -- "shape": a tensor `run` rebinds before every launch, so a
        zero-stride view of one 4 KB block (not 0.8 GB at 64 frames of 720x1280)."""
        self.split_want -= self.no_shadow
        if self.use_arena:
            self.arena.buf = self.torch.empty(max(self.arena_floats, 4), dtype=torch.float32, device=self.device)
            if self.arena_debug:
                self.arena.buf.fill_(float("nan"))
        for k, need in self.scratch_need.items():
            # (the Winograd V planes are zero-filled once: their padding rows are multiplied by the GEMM, never read back)
            alloc = self.torch.zeros if k[0] == "WV" else self.torch.empty
            self.scratch[k] = alloc(max(need, 4), dtype=torch.float16 if k[0] == "Ds" else torch.float32,
                                    device=self.device)
        for name, (shape, dtype, how) in callers.items():
            if how == "shape":
                t = self.torch.zeros(1024, dtype=dtype, device=self.device)[:1].expand(shape)
            else:
                t = (self.torch.zeros if how == "zeros" else self.torch.empty)(shape, dtype=dtype, device=self.device)
            self.callers[name] = t

    def end(self):
        """End of the recording pass."""
        self._flush_poison(final=True)
        self.arena.recording = False

    def caller(self, name, n, h, w, c) -> V:
        """Caller-side tensor `name` of the table as a view (NCHW tensors: the shape only says how many floats)."""
        return V(Caller(name, self.callers.get(name), named=name != "logits"), n, h, w, c)      # (the logits tap is never rebound)

    def _bind(self, v, slot):
        """The descriptor of the op just opened holds `v`'s address in `slot`: enter it in the bind table if it is the caller's."""
        if v is not None and isinstance(v.t, Caller):
            self.binds.append((v.t.name, len(self.ops_meta) - 1, slot, 4 * v.coff))

    def pin(self, *vs):
        """These buffers outlive the call (Arena.pin); decided by the sizing pass."""
        if self.use_arena and self.dry:
            for t in {id(v.t): v.t for v in vs}.values():
                self.arena.pin(t)

    # ------------------------------------------------------------------ memory helpers
    def buf(self, name, n, h, w, c, pinned=False) -> V:
        """A named NHWC activation.  With the arena (default) it is `n*h*w*c` floats of ONE pool, placed so that it shares
        addresses only with buffers it is never live together with (first declared use .. last declared use of the recorded
        plan); `pinned`: survives the call (the resident recurrent state), its own allocation."""
        sp = None
        numel = n * h * w * c
        if self.use_arena and not pinned:
            t = self.arena.ref(name, numel)
        elif self.dry:
            t = _Fake()
        else:
            t = self.torch.empty(numel, dtype=torch.float32, device=self.device)
            self.keep.append(t)
        if not self.dry and name in self.split_want and c % 32 == 0:
            # NaN-filled, not empty: if a producer that cannot write shadows were ever added without entering
            # its output in `no_shadow`, the GEMM reading this shadow would multiply NaNs -- the first run of the
            # plan then fails loudly (run(): `_verify_first_run`) instead of returning plausible wrong maps.
            # (Shadows stay outside the arena for that reason: a recycled range would hold somebody's finite data)
            sp = self.torch.full((2 * numel,), float("nan"), dtype=torch.float16, device=self.device)
            self.keep.append(sp)
        v = V(t, n, h, w, c, sp=sp, key=name)
        if name:
            self.named[name] = v
        return v

    def _flush_poison(self, final=False):
        """Debug mode: once the op that ends a buffer's live range has been recorded -- and before anything of the next op,
        a fork included -- the range is filled with NaN (on the lane Arena.due names), so a use after release cannot go unnoticed."""
        if not (self.arena_debug and self.use_arena) or self.dry:
            return
        cur = self.lane
        for r, lane in self.arena.due(final):
            if lane != cur:
                L.check(self.lib.uavsal_plan_set_lane(self.plan, lane), "plan_set_lane")
                cur = lane
            self.op_idx["poison:%s" % (r.aid,)] = len(self.ops_meta)
            if lane == PRIOR_LANE:
                self.prior_ops.append(len(self.ops_meta))
            self.ops_meta.append(dict(kind="poison", name="poison:%s" % (r.aid,), flops=0.0, bytes=4.0 * r.numel_, lane=lane))
            self.op_args.append(dict(kind="poison", name="poison:%s" % (r.aid,)))
            d = L.FillDesc()
            d.out, d.n, d.bits = self.arena.buf.data_ptr() + 4 * r.off, r.numel_, 0x7FC00000
            self._add(self.lib.uavsal_plan_add_fill, d, "plan_add_fill")
        if cur != self.lane:
            L.check(self.lib.uavsal_plan_set_lane(self.plan, self.lane), "plan_set_lane")

    def scr_split(self, n, h, w, c) -> V:
        """A depthwise output that exists only as its split shadow (scratch, per lane)."""
        numel = 2 * n * h * w * c
        k = ("Ds", self.lane)
        if self.dry:
            self.scratch_need[k] = max(self.scratch_need.get(k, 0), numel)
            return V(None, n, h, w, c, sp=_Fake(), key=k)
        return V(None, n, h, w, c, sp=self.scratch[k], key=k)

    def _would_split(self, n_img, h, w, cin, cout, taps, act, has_res, ldc=None, ldr=None) -> bool:
        """Would `uavsal_conv_gemm` take the pre-split LDS-DMA path for this GEMM if its A operand had a
        shadow?  (Shape question only: asked with dummy aligned pointers.)"""
        if not self.split_mode:
            return False
        d = L.ConvDesc()
        P_ = 1 << 20
        d.a, d.lda, d.a_img_stride = P_, cin, h * w
        d.a_split, d.ldas = P_, 2 * cin
        d.w, d.out, d.ldc, d.o_img_stride = P_, P_, (cout if ldc is None else ldc), h * w
        if has_res:
            d.res, d.ldr, d.r_img_stride = P_, (cout if ldr is None else ldr), h * w
        d.n_img, d.H, d.W, d.Cin, d.Cout, d.taps = n_img, h, w, cin, cout, taps
        d.prec, d.act, d.epi, d.tile = self.prec, act, L.EPI_AFFINE, 0
        return L.conv_route(self.lib, d).family == L.ROUTE_PRESPLIT

    def scr(self, kind, n, h, w, c) -> V:
        """Scratch for the expanded tensors of an inverted-residual block and the Winograd planes.  With the arena: an
        anonymous buffer of the pool, live from its producer to its last reader (blocks that run back to back end up on the
        same addresses, concurrent lanes never do).  Without: one pool per (kind, lane)."""
        numel = n * h * w * c
        if self.use_arena:
            return V(self.arena.scratch(kind, numel), n, h, w, c)
        key = (kind, self.lane)
        if self.dry:
            self.scratch_need[key] = max(self.scratch_need.get(key, 0), numel)
            return V(_Fake(), n, h, w, c)
        return V(self.scratch[key], n, h, w, c)

    # ---- parallel branches (uavsal_plan lanes) -----------------------------------------
    def fork(self, lane):
        """Following ops (until `main()`) go to `lane`, which starts after everything recorded on
        lane 0 so far."""
        self._meta(kind="sync", name="fork%d" % lane, flops=0.0, bytes=0.0, group_lane=lane)
        self.arena.fork(lane)
        if not self.dry:
            r = self.lib.uavsal_plan_add_fork(self.plan, lane)
            if r < 0:
                L.check(r, "plan_add_fork")
            L.check(self.lib.uavsal_plan_set_lane(self.plan, lane), "plan_set_lane")
        self.lane = self.arena.lane = lane

    def main(self):
        if not self.dry:
            L.check(self.lib.uavsal_plan_set_lane(self.plan, 0), "plan_set_lane")
        self.lane = self.arena.lane = 0

    def join(self, lane):
        self._meta(kind="sync", name="join%d" % lane, flops=0.0, bytes=0.0, group_lane=lane)
        self.arena.join(lane)
        if not self.dry:
            r = self.lib.uavsal_plan_add_join(self.plan, lane)
            if r < 0:
                L.check(r, "plan_add_join")

    def prec_for(self, name) -> str:
        best, val = -1, self.prec_name
        for k, v in self.prec_overrides.items():
            if name.startswith(k) and len(k) > best:
                best, val = len(k), v
        return val

    def _tile_of(self, n_img, h, w, cout, epi) -> int:
        d = L.ConvDesc()
        d.n_img, d.H, d.W, d.Cout, d.prec, d.epi, d.tile = n_img, h, w, cout, self.prec, epi, 0
        d.out = 1 << 20
        return L.conv_route(self.lib, d).tile

    # ------------------------------------------------------------------ op recorders
    def _meta(self, **kw):
        self._flush_poison()
        self.arena.lop += 1
        if kw.pop("group_lane", self.lane) == PRIOR_LANE:      # (a fork / join belongs to the lane it names)
            self.prior_ops.append(len(self.ops_meta))
        self.op_idx[kw.get("name")] = len(self.ops_meta)       # == index of the op in the native plan
        self.ops_meta.append(kw)
        self.op_args.append(dict(kind=kw.get("kind"), name=kw.get("name")))

    def _ov(self, v, img=None):
        return None if v is None else OpView.of(v, img)

    def _add(self, fn, desc, what):
        r = fn(self.plan, C.byref(desc))
        if r < 0:
            L.check(r, what)

    def conv(self, name, a: V, conv, bn, out: V, act, taps=1, res: Optional[V] = None, wslice=None,
             epi=L.EPI_AFFINE, aux: Optional[V] = None, n_img=None, strides=None, cout=None,
             out2: Optional[V] = None, gate_interleave=0, dw=None, n_group=0):
        """`dw=(dw_conv, dw_bn, stride)`: `a` is the expanded tensor and the depthwise 3x3 + BN + ReLU6
        is produced inside this GEMM's loader (uavsal_conv_desc.dw_*).
        `n_group`: `conv` / `bn` are lists of 1x1 convs with `n_group` outputs each whose inputs lie side by side in `a`'s rows
        (a = the first one's view): one launch (uavsal_conv_desc.n_group / a_group_off)."""
        cin = a.c
        cout = out.c if cout is None else cout
        n_img = a.n if n_img is None else n_img
        hin, win = a.h, a.w
        a_in = a
        if dw is not None:
            a = V(a.t, a.n, (hin - 1) // dw[2] + 1, (win - 1) // dw[2] + 1, a.c, a.ld, a.coff)
        hw = a.h * a.w
        flops = 2.0 * n_img * hw * cin * cout * taps
        byts = 4.0 * n_img * hw * (cin + cout) + 4.0 * cin * cout * taps
        if dw is not None:      # the launch also does the depthwise: reads E (hin x win), D never exists
            flops += 18.0 * n_img * hw * cin
            byts = 4.0 * n_img * (hin * win * cin + hw * cout) + 4.0 * cin * (cout + 11)
        self._meta(kind="conv%d" % (3 if taps == 9 else 1), name=name, flops=flops, bytes=byts,
                   M=n_img * hw, K=cin * taps, Nc=cout)
        self.arena.touch(a, out, res, aux, out2)
        # split shadows (f16x3): can this launch write one for its output / read its input pre-split?
        shadow_out = False
        if self.split_mode:
            aligned = cout % 4 == 0 and out.ld % 4 == 0 and (res is None or res.ld % 4 == 0)
            if epi == L.EPI_AFFINE:
                shadow_out = aligned and act != L.ACT_SIGMOID
            elif epi == L.EPI_TWA:       # the vector ConvTWA update only exists in the 1x1-fragment tiles
                shadow_out = aligned and self._tile_of(n_img, a.h, a.w, cout, epi) in (3, 4)
            if self.dry:
                if not shadow_out and out.key is not None:
                    self.no_shadow.add(out.key)
                if (a.key is not None and a.key not in self.no_shadow and dw is None and strides is None
                        and epi == L.EPI_AFFINE and a.ld % 32 == 0 and (a.coff % a.ld) % 32 == 0 and self._would_split(
                            n_img, a.h, a.w, cin, cout, taps, act, res is not None, out.ld, res.ld if res is not None else None)):
                    self.split_want.add(a.key)
        if self.dry:
            return
        d = L.ConvDesc()
        st = strides or {}
        d.a, d.lda, d.a_img_stride = a.ptr, a.ld, st.get("a", hin * win if dw is not None else hw)
        self._bind(a, SLOT_CONV_A)
        self._bind(out, SLOT_CONV_OUT)
        if a.sp is not None and dw is None and strides is None and epi == L.EPI_AFFINE:
            d.a_split, d.ldas = a.sp_ptr, 2 * a.ld
        if out.sp is not None and shadow_out:
            d.out_split, d.ldos = out.sp_ptr, 2 * out.ld
        if dw is not None:
            w9, s_, b_ = self.weights.depthwise(dw[0], dw[1])
            d.dw_w9c, d.dw_scale, d.dw_bias = w9.data_ptr(), s_.data_ptr(), b_.data_ptr()
            d.dw_stride, d.dw_Hin, d.dw_Win = dw[2], hin, win
            self.ops_meta[-1]["fused_dw"] = True
        if bn is not None:
            s, b = self.weights.affine(bn, cout)
            d.scale, d.bias = s.data_ptr(), b.data_ptr()
        else:
            d.scale, d.bias = None, None
        d.out, d.ldc, d.o_img_stride = out.ptr, out.ld, st.get("o", hw)
        if res is not None:
            d.res, d.ldr, d.r_img_stride = res.ptr, res.ld, st.get("r", hw)
        else:
            d.res, d.ldr, d.r_img_stride = None, 0, hw
        if aux is not None:
            d.aux, d.ldx, d.x_img_stride = aux.ptr, aux.ld, st.get("x", hw)
        else:
            d.aux, d.ldx, d.x_img_stride = None, 0, hw
        d.n_img, d.H, d.W = n_img, a.h, a.w
        d.Cin, d.Cout, d.taps = cin, cout, taps
        pn = self.prec_for(name)
        d.prec, d.act, d.epi, d.tile = L.PREC[pn], act, epi, 0
        d.n_group, d.a_group_off = n_group, (cin if n_group else 0)
        # GEMMs on a side lane run beside grid-filling GEMMs of the main lane: the 64 x 64 instance with 32-float K stages
        # needs 32 KB of LDS and 122 VGPRs, so one of its workgroups fits on a CU next to two of the main lane's
        # (64 KB, 155 VGPRs each) instead of waiting for them to retire
        # (5.155 vs 5.17 ms per step, same box, two runs each)
        if self.lane != 0 and pn == "f32" and epi == L.EPI_AFFINE and dw is None and cin % 32 == 0:
            d.tile = 11
        if out2 is not None:
            d.out2, d.ld2 = out2.ptr, out2.ld
        if self.stream_k:
            # one workspace per lane: launches on a lane are ordered on one stream (uavsal_conv_desc.sk_ws)
            ws = self.sk_ws.get(self.lane)
            if ws is None:
                ws = self.sk_ws[self.lane] = self.torch.zeros(int(self.lib.uavsal_streamk_workspace_bytes()),
                                                           dtype=torch.uint8, device=self.device)
            d.sk_ws, d.sk_ws_bytes = ws.data_ptr(), ws.numel()
        d.err = self.err
        d.sk_spin_limit, d.sk_debug_drop = self.sk_debug      # test hooks (model._sk_debug), normally (0, 0)
        # weights last: their 16-bit packing depends on which kernel the descriptor selects
        d.w = 1 << 20
        route = L.conv_route(self.lib, d)
        split, dwproj, tile = route.family == L.ROUTE_PRESPLIT, route.dwproj, route.tile
        if a.t is None and not split:
            raise RuntimeError("%s: its input only exists as a split shadow but the GEMM is not eligible" % name)
        ksize = (conv[0] if isinstance(conv, (list, tuple)) else conv).weight.shape[-1]
        d.w = self.weights.conv(conv, wslice, gate_interleave, conv_weight_layout(pn, split, dwproj != 0, tile, ksize)).data_ptr()
        self.ops_meta[-1]["prec"] = pn
        self.ops_meta[-1]["split"] = split
        self.ops_meta[-1]["tile"] = tile
        self.ops_meta[-1]["streamk"] = route.streamk
        self.ops_meta[-1]["dwproj"] = dwproj
        groups = cout // n_group if n_group else 1
        ad = self._ov(V(a_in.t, n_img, hin, win, cin + (groups - 1) * cin, a_in.ld, a_in.coff, a_in.sp, a_in.key),
                      d.a_img_stride)
        if not split:
            ad.sp = None
        od = self._ov(out, d.o_img_stride)
        if not d.out_split:
            od.sp = None
        self.op_args[-1].update(conv=conv, bn=bn, act=act, epi=epi, taps=taps, wslice=wslice, gate_interleave=gate_interleave,
                                n_group=n_group, dw=dw, prec=pn, split_in=split, cin=cin, cout=cout, a=ad, out=od,
                                res=self._ov(res, d.r_img_stride), aux=self._ov(aux, d.x_img_stride),
                                out2=self._ov(out2, d.o_img_stride))
        self._add(self.lib.uavsal_plan_add_conv, d, "plan_add_conv(%s)" % name)

    def conv3_wino(self, name, a: V, conv, bn, out: V, act, wslice=None, n_img=None, strides=None, twa=None, gemm_tile=0, r=2):
        """Dense 3x3 conv (stride 1, padding 1) as Winograd F(r x r, 3x3), exact-fp32 mode only: input transform, ONE GEMM
        launch over the (r + 2)^2 transform planes (per-plane weights), output transform with the epilogue -- 2.25x (r = 2)
        or 4x (r = 4) fewer MFMA FLOPs than the implicit GEMM (csrc/winograd.hip).  `twa=(x_t, pre_t)`: ConvTWA update in the output transform."""
        cin, cout = a.c, out.c
        n = a.n if n_img is None else n_img
        hw = a.h * a.w
        tiles = n * ((a.h + r - 1) // r) * ((a.w + r - 1) // r)
        pp = (r + 2) * (r + 2)
        mp = roundup(tiles, 128)
        st = strides or {}
        v = self.scr("WV", pp, mp, 1, cin)
        mm = self.scr("WM", pp, mp, 1, cout)
        self._meta(kind="wino_in", name=name + ".xin", flops=0.0, bytes=4.0 * n * hw * cin + 4.0 * float(pp) * tiles * cin)
        self.op_args[-1].update(triple=name + ".xout")
        self.arena.touch(a, v)
        if twa is not None and r == 2 and self._twa_prev is not None and self._twa_prev[0] == self.arena.lop - 1:
            # a seam launch (uavsal_plan_seam) writes this step's V planes while it still runs the previous step's output
            # transform: everything that op reads or writes stays live one op longer, so V is never placed on it
            self.arena.touch(*self._twa_prev[1])
        xin_op = len(self.ops_meta) - 1
        if not self.dry:
            wi = L.WinoDesc()
            wi.inp, wi.ldi, wi.in_img_stride = a.ptr, a.ld, st.get("a", hw)
            wi.out, wi.ldo = v.ptr, cin
            wi.n_img, wi.H, wi.W, wi.C, wi.Mp, wi.R = n, a.h, a.w, cin, mp, r
            self._add(self.lib.uavsal_plan_add_wino_input, wi, "plan_add_wino_input(%s)" % name)
        self._meta(kind="conv1", name=name, flops=2.0 * pp * tiles * cin * cout,
                   bytes=4.0 * pp * (tiles * (cin + cout) + cin * cout), M=pp * mp, K=cin, Nc=cout,
                   direct_flops=2.0 * n * hw * cin * cout * 9)
        self.arena.touch(v, mm)
        self.op_args[-1].update(triple=name + ".xout")
        if not self.dry:
            d = L.ConvDesc()
            d.a, d.lda, d.a_img_stride = v.ptr, cin, mp
            d.w, d.w_group_stride = self.weights.wino(conv, wslice, r).data_ptr(), roundup(cout, 32) * roundup(cin, 32)
            d.out, d.ldc, d.o_img_stride = mm.ptr, cout, mp
            d.n_img, d.H, d.W, d.Cin, d.Cout, d.taps = pp, mp, 1, cin, cout, 1
            d.prec, d.act, d.epi, d.tile = L.PREC["f32"], L.ACT_NONE, L.EPI_AFFINE, gemm_tile      # Winograd plans are exact fp32
            d.err = self.err
            m_ = self.ops_meta[-1]
            m_["split"], m_["tile"], m_["streamk"], m_["dwproj"] = False, L.conv_route(self.lib, d).tile, 0, 0
            m_["prec"] = "f32"
            self._add(self.lib.uavsal_plan_add_conv, d, "plan_add_conv(%s)" % name)
        self._meta(kind="wino_out", name=name + ".xout", flops=0.0, bytes=4.0 * (float(pp) * tiles * cout + n * hw * cout))
        self.arena.touch(mm, out, *(twa or ()), *((a,) if twa is not None else ()))
        if twa is not None:
            self._twa_prev = (self.arena.lop, (mm, out, twa[0], twa[1], a))
            self.twa_steps.append(dict(name=name, r=r, xin=xin_op, gemm=len(self.ops_meta) - 2, xout=len(self.ops_meta) - 1,
                                       v=v, m=mm, out=out, a=a, x=twa[0], pre=twa[1]))
        if out.key is not None and self.dry:
            self.no_shadow.add(out.key)            # the output transform does not write split shadows
        if not self.dry:
            wo = L.WinoDesc()
            wo.inp, wo.ldi = mm.ptr, cout
            wo.out, wo.ldo, wo.out_img_stride = out.ptr, out.ld, st.get("o", hw)
            wo.n_img, wo.H, wo.W, wo.C, wo.Mp, wo.R = n, a.h, a.w, cout, mp, r
            if bn is not None:
                s_, b_ = self.weights.affine(bn, cout)
                wo.scale, wo.bias = s_.data_ptr(), b_.data_ptr()
            wo.act, wo.epi = act, L.EPI_AFFINE
            if twa is not None:
                xt, pre = twa
                wo.epi = L.EPI_TWA
                wo.res, wo.ldr, wo.res_img_stride = xt.ptr, xt.ld, st.get("r", hw)
                wo.aux, wo.ldx, wo.aux_img_stride = pre.ptr, pre.ld, st.get("x", hw)
                wo.hprev, wo.ldh, wo.h_img_stride = a.ptr, a.ld, st.get("a", hw)
            ai = st.get("a", hw)
            # (`segs`: the views of a segmented input, uavsal_wino_desc.n_seg -- a form of the ABI the plans do not take, so
            # always None; the field stays in the record that tests/test_plan_ops_fp64.py reads)
            self.op_args[-1].update(kind="wino", triple_first=name + ".xin", conv=conv, bn=bn, act=act, wslice=wslice, r=r, cin=cin,
                                    cout=cout, a=self._ov(a, ai), segs=None, out=self._ov(out, wo.out_img_stride),
                                    twa=None if twa is None else (self._ov(twa[0], wo.res_img_stride), self._ov(twa[1], wo.aux_img_stride)))
            self._add(self.lib.uavsal_plan_add_wino_output, wo, "plan_add_wino_output(%s)" % name)

    def dw(self, name, a: V, conv, bn, out: V, stride, dilation):
        c = a.c
        ho, wo = (a.h - 1) // stride + 1, (a.w - 1) // stride + 1
        byts = 4.0 * a.n * c * (a.h * a.w + ho * wo) + 4.0 * 9 * c + 4.0 * 2 * c
        self._meta(kind="dw", name=name, flops=2.0 * 9 * a.n * ho * wo * c, bytes=byts, stride=stride,
                   dil=dilation if not isinstance(dilation, (list, tuple)) else tuple(dilation), patches44=a.n * ((ho + 3) // 4) * ((wo + 3) // 4) * (c // 4))
        self.arena.touch(a, out)
        if self.dry:
            return
        grouped = isinstance(conv, (list, tuple))      # several dilated branches of one map: channel groups with their own dilation
        w9, s, b = self.weights.depthwise(conv, bn)
        d = L.DwDesc()
        if grouped:
            d.dil_group_c = c // len(conv)
            for gi, dl in enumerate(dilation):
                d.dil_groups[gi] = dl
            dilation = dilation[0]
        d.inp, d.ldi = a.ptr, a.ld
        d.w9c, d.scale, d.bias = w9.data_ptr(), s.data_ptr(), b.data_ptr()
        if out.t is None:            # the projection GEMM stages this tensor pre-split: no fp32 copy
            d.out, d.ldo = None, out.ld
            d.out_split, d.ldos = out.sp_ptr, 2 * out.ld
            self.ops_meta[-1]["split_out"] = True
        else:
            d.out, d.ldo = out.ptr, out.ld
        d.n_img, d.H, d.W, d.C = a.n, a.h, a.w, c
        d.stride, d.dilation, d.act = stride, dilation, L.ACT_RELU6
        self.ops_meta[-1]["kernel"] = L.DW_KERNEL.get(int(self.lib.uavsal_dw_variant(C.byref(d))), "dw3x3")
        self.op_args[-1].update(conv=conv, bn=bn, stride=stride, dilation=(tuple(d.dil_groups[:len(conv)]) if grouped else dilation),
                                a=self._ov(a), out=self._ov(out))
        self._add(self.lib.uavsal_plan_add_dw, d, "plan_add_dw(%s)" % name)

    def dw_dot(self, name, a: V, dwc, dwbn, pl, plbn, out: V, act):
        """Depthwise 3x3 + BN + ReLU6 -> projection to ONE channel + BN + act as one bandwidth-bound launch (uavsal_dw3x3_dot):
        the tail of conv_out_st (model.py:333-334, 372-373).  Exact fp32 in every precision mode of the plan."""
        c = a.c
        self._meta(kind="dw_dot", name=name, flops=2.0 * 10 * a.n * a.h * a.w * c, bytes=4.0 * a.n * a.h * a.w * (c + 1) + 4.0 * 12 * c,
                   stride=1, dil=1, kernel="dw3x3_dot_kernel<4, 4>")
        self.arena.touch(a, out)
        if self.dry:
            return
        w9, s, b, w2, s2, b2 = self.weights.dw_dot(dwc, dwbn, pl, plbn)
        d = L.DwDotDesc()
        d.inp, d.ldi = a.ptr, a.ld
        d.w9c, d.scale, d.bias, d.w2, d.scale2, d.bias2 = (t.data_ptr() for t in (w9, s, b, w2, s2, b2))
        d.out, d.ldo = out.ptr, out.ld
        self._bind(out, SLOT_CONV_OUT)
        d.n_img, d.H, d.W, d.C, d.act = a.n, a.h, a.w, c, act
        self.op_args[-1].update(dw=(dwc, dwbn), conv=pl, bn=plbn, act=act, a=self._ov(a), out=self._ov(out))
        self._add(self.lib.uavsal_plan_add_dw_dot, d, "plan_add_dw_dot(%s)" % name)

    def bilinear(self, name, a: V, out: V, src_mod=None, src_div=1):
        self._meta(kind="bilinear", name=name, flops=0.0, bytes=4.0 * out.n * out.h * out.w * out.c * 2)
        self.arena.touch(a, out)
        if self.dry:
            return
        d = L.BilinearDesc()
        d.inp, d.ldi, d.Hi, d.Wi = a.ptr, a.ld, a.h, a.w
        d.out, d.ldo, d.Ho, d.Wo = out.ptr, out.ld, out.h, out.w
        d.n_out, d.C = out.n, a.c
        if out.sp is not None:
            d.out_split, d.ldos = out.sp_ptr, 2 * out.ld
        d.src_mod, d.src_div = (out.n if src_mod is None else src_mod), src_div
        self.op_args[-1].update(a=self._ov(a), out=self._ov(out), src_mod=d.src_mod, src_div=src_div)
        self._add(self.lib.uavsal_plan_add_bilinear, d, "plan_add_bilinear(%s)" % name)

    def layout(self, name, src: V, dst: V, to_nhwc, cpad=0):
        """NCHW <-> NHWC between a caller-side tensor (Recorder.caller) and a buffer of the plan, whose shape the op takes."""
        nhwc, nchw = (dst, src) if to_nhwc else (src, dst)
        n, c, hw = nhwc.n, nhwc.c, nhwc.h * nhwc.w
        self._meta(kind="layout", name=name, flops=0.0, bytes=8.0 * n * c * hw)
        self.arena.touch(src, dst)
        if self.dry:
            return
        d = L.LayoutDesc()
        d.inp, d.out, d.n_img, d.C, d.HW, d.ld, d.to_nhwc, d.Cpad = src.ptr, dst.ptr, n, c, hw, nhwc.ld, to_nhwc, cpad
        self._bind(src, SLOT_LAYOUT_IN)
        self._bind(dst, SLOT_LAYOUT_OUT)
        ov = self._ov(nhwc)
        cv = OpView(nchw.t.name, nchw.coff, n, nhwc.h, nhwc.w, c, c, hw, nchw=True)
        self.op_args[-1].update(to_nhwc=to_nhwc, cpad=cpad, a=cv if to_nhwc else ov, out=ov if to_nhwc else cv)
        self._add(self.lib.uavsal_plan_add_layout, d, "plan_add_layout(%s)" % name)

    def stem(self, name, x: V, conv0, bn0, out: V, u8):
        """features[0] on the caller's NCHW frames `x` (fp32, or `u8`: raw bytes), ImageNet normalisation included."""
        self._meta(kind="stem", name=name, flops=2.0 * 27 * 32 * out.n * out.h * out.w,
                   bytes=(1.0 if u8 else 4.0) * x.n * 3 * x.h * x.w + 4.0 * out.n * out.h * out.w * 32)
        self.arena.touch(out)
        if self.dry:
            return
        ws, ss, bs = self.weights.stem(conv0, bn0)
        d = L.StemDesc()
        d.inp, d.in_u8 = (None, x.ptr) if u8 else (x.ptr, None)
        self._bind(x, SLOT_STEM_U8 if u8 else SLOT_STEM_F32)
        d.w, d.scale, d.bias = ws.data_ptr(), ss.data_ptr(), bs.data_ptr()
        d.out, d.ldo = out.ptr, 32
        d.n_img, d.H, d.W = x.n, x.h, x.w
        for i in range(3):
            d.mean[i], d.stdv[i] = synth.IMAGENET_MEAN[i], synth.IMAGENET_STD[i]
        self.op_args[-1].update(conv=conv0, bn=bn0, u8=u8, mean=tuple(synth.IMAGENET_MEAN), stdv=tuple(synth.IMAGENET_STD),
                                a=OpView(x.t.name, 0, x.n, x.h, x.w, 3, 3, 0, nchw=True), out=self._ov(out))
        self._add(self.lib.uavsal_plan_add_stem, d, "plan_add_stem")

    def tdiff(self, name, a: V, out: V, seq_len):
        self._meta(kind="tdiff", name=name, flops=0.0, bytes=4.0 * a.n * a.h * a.w * (a.c + out.c))
        self.arena.touch(a, out)
        if self.dry:
            return
        d = L.TdiffDesc()
        d.inp, d.ldi, d.out, d.ldo = a.ptr, a.ld, out.ptr, out.ld
        d.n_img, d.HW, d.C, d.seq_len = a.n, a.h * a.w, a.c, seq_len
        self.op_args[-1].update(a=self._ov(a), out=self._ov(out), seq_len=seq_len)
        self._add(self.lib.uavsal_plan_add_tdiff, d, "plan_add_tdiff")

    def tsum(self, name, a: V, out: V, T):
        """Sum over each group of `T` consecutive frames of `a`."""
        self._meta(kind="tsum", name=name, flops=0.0, bytes=4.0 * (a.n + out.n) * a.h * a.w * out.c)
        self.arena.touch(a, out)
        if self.dry:
            return
        d = L.TsumDesc()
        d.inp, d.ldi, d.out, d.ldo = a.ptr, a.ld, out.ptr, out.ld
        d.n_groups, d.T, d.HW, d.C = out.n, T, a.h * a.w, out.c
        self.op_args[-1].update(a=self._ov(a), out=self._ov(out), T=T)
        self._add(self.lib.uavsal_plan_add_tsum, d, "plan_add_tsum")

    def copy(self, name, hist: V, keep: V, seq_len):
        """The last frame of every clip of `hist` (NHWC rows of the history) -> `keep`, one strided copy."""
        hw, n = hist.h * hist.w, keep.n
        self._meta(kind="copy", name=name, flops=0.0, bytes=8.0 * n * hist.c * hw)
        self.arena.touch(hist, keep)
        if self.dry:
            return
        d = L.CopyDesc()
        d.inp, d.out = hist.frames(seq_len - 1, 1).ptr, keep.ptr
        d.in_pitch, d.out_pitch, d.row_floats, d.rows = seq_len * hw * hist.c, hw * hist.c, hw * hist.c, n
        self.op_args[-1].update(a=self._ov(hist.frames(seq_len - 1, n), seq_len * hw), out=self._ov(keep))
        self._add(self.lib.uavsal_plan_add_copy, d, "plan_add_copy")

    def guard(self, *bufs):
        """Error guard: poisons what the caller will see -- up to three whole buffers, None for one the plan does not have --
        if any kernel of this run set the error word."""
        self._meta(kind="guard", name="guard", flops=0.0, bytes=0.0)
        self.arena.touch(*bufs)
        if self.dry:
            return
        args = []
        for slot, v in enumerate((bufs + (None, None))[:3]):
            args += [None, 0] if v is None else [v.ptr, v.n * v.h * v.w * v.c]
            self._bind(v, slot)
        r = self.lib.uavsal_plan_add_guard(self.plan, *args)
        if r < 0:
            L.check(r, "plan_add_guard")

    def fused_block(self, name, x: V, blk, out: V) -> bool:
        """The whole inverted-residual block as ONE launch (uavsal_fused_ir: the expanded tensors stay in LDS),
        where an instance exists -- the bandwidth-bound small-channel blocks features[1..7].  False = not taken."""
        if not self.fuse_blocks or getattr(blk, "dilation", 1) != 1:
            return False
        d = L.FusedIrDesc()
        d.Cin, d.hidden, d.Cout, d.stride = x.c, blk.hidden, out.c, blk.stride
        d.w1 = (1 << 20) if blk.expand_ratio != 1 else None
        kind = int(self.lib.uavsal_fused_ir_supported(C.byref(d)))
        if not kind:
            return False
        natural = kind == 2          # csrc/fused_mid.hip: 1x1 weights in their own layout
        if natural:
            # one workgroup per 4 x 8 output patch and CU-wide LDS: taken where the launch is about one round of the chip
            # (the 23x40 backbone maps at one clip); bigger launches keep expand GEMM + depthwise / projection launches
            wgs = x.n * ((x.h + 3) // 4) * ((x.w + 7) // 8)
            if not (MID_MIN_WGS <= wgs <= MID_MAX_WGS):
                return False
        ho, wo = (x.h - 1) // blk.stride + 1, (x.w - 1) // blk.stride + 1
        self._meta(kind="fused_ir", name=name, kernel="%s<%d, %d, %d%s>" % ("fused_mid_kernel" if natural else "fused_ir_kernel", x.c, blk.hidden, out.c,
                                                                    "" if natural else ", %d" % blk.stride),
                   flops=2.0 * x.n * ((x.h * x.w * x.c * blk.hidden if blk.expand_ratio != 1 else 0)
                                      + ho * wo * blk.hidden * (9 + out.c)),
                   bytes=4.0 * x.n * (x.h * x.w * x.c + ho * wo * out.c * (2 if blk.use_res_connect else 1)),
                   unfused_bytes=4.0 * x.n * (x.h * x.w * (x.c + (2 * blk.hidden if blk.expand_ratio != 1 else 0))
                                              + ho * wo * (2 * blk.hidden + out.c)),
                   # what the matrix pipe executes in the mid kernel: every 4 x 8 patch expands its whole 6 x 10 halo (64 MFMA
                   # rows) and projects 32 rows, edge patches included
                   **({"flops_executed": 2.0 * wgs * blk.hidden * (64 * x.c + 32 * out.c)} if natural else {}))
        self.arena.touch(x, out)
        if out.key is not None:
            self.no_shadow.add(out.key)            # this kernel does not write split shadows
        if self.dry:
            return True
        ws = self.weights.fused_block(blk, natural)
        d.inp, d.ldi = x.ptr, x.ld
        if "w1" in ws:
            d.w1, d.scale1, d.bias1 = ws["w1"].data_ptr(), ws["s1"].data_ptr(), ws["b1"].data_ptr()
        d.wd, d.scale_d, d.bias_d = ws["wd"].data_ptr(), ws["sd"].data_ptr(), ws["bd"].data_ptr()
        d.w2, d.scale2, d.bias2 = ws["w2"].data_ptr(), ws["s2"].data_ptr(), ws["b2"].data_ptr()
        if blk.use_res_connect:
            d.res, d.ldr = x.ptr, x.ld
        d.out, d.ldo = out.ptr, out.ld
        d.n_img, d.H, d.W = x.n, x.h, x.w
        self.op_args[-1].update(blk=blk, a=self._ov(x), out=self._ov(out), res=self._ov(x) if blk.use_res_connect else None)
        self._add(self.lib.uavsal_plan_add_fused_ir, d, "plan_add_fused_ir(%s)" % name)
        return True

    def ir_block(self, name, x: V, blk, out: V, final_act=L.ACT_NONE, expanded: Optional[V] = None):
        """pw-expand + BN + ReLU6 -> dw3x3 + BN + ReLU6 -> pw-linear + BN [+ x]
        (dwBlock, reference model.py:74-103; torchvision InvertedResidual).
        `expanded`: the block's expanded tensor already exists (several blocks' expands run as one GEMM)."""
        if expanded is None and final_act == L.ACT_NONE and self.fused_block(name, x, blk, out):
            return
        # a block whose expanded tensor would be bigger than BLOCK_CHUNK_BYTES runs in chunks of whole frames (the block is
        # per-frame arithmetic; the launches stay many rounds of the chip): the arena's peak is set by the biggest E, not by
        # the layer count -- 720x1280 x 64 frames: fucbst's 7.1 GB E in two halves, peak 16.97 -> ~13 GB
        if (expanded is None and blk.expand_ratio != 1 and x.n > 1 and self.use_arena and out.c > 1      # (the decoder's map is one launch)
                and 4 * x.n * x.h * x.w * blk.hidden > BLOCK_CHUNK_BYTES):
            per = 4 * x.h * x.w * blk.hidden
            step = max(1, BLOCK_CHUNK_BYTES // per)
            nchunk = (x.n + step - 1) // step
            step = (x.n + nchunk - 1) // nchunk                     # equal chunks
            for ci, f0 in enumerate(range(0, x.n, step)):
                cnt = min(step, x.n - f0)
                self._ir_block_one("%s#%d" % (name, ci) if nchunk > 1 else name, x.frames(f0, cnt), blk, out.frames(f0, cnt), final_act)
            return
        self._ir_block_one(name, x, blk, out, final_act, expanded)

    def _ir_block_one(self, name, x: V, blk, out: V, final_act=L.ACT_NONE, expanded: Optional[V] = None):
        seq = blk.conv
        stride, dil = blk.stride, getattr(blk, "dilation", 1)
        if blk.expand_ratio != 1:
            if expanded is not None:
                e = expanded
            else:
                e = self.scr("E", x.n, x.h, x.w, blk.hidden)
                self.conv(name + ".pw", x, seq[0][0], seq[0][1], e, L.ACT_RELU6)
            dwc, dwbn, pl, plbn = seq[1][0], seq[1][1], seq[2], seq[3]
        else:
            e = x
            dwc, dwbn, pl, plbn = seq[0][0], seq[0][1], seq[1], seq[2]
        ho, wo = (x.h - 1) // stride + 1, (x.w - 1) // stride + 1
        if (out.c == 1 and stride == 1 and dil == 1 and blk.expand_ratio != 1 and not blk.use_res_connect
                and blk.hidden % 256 == 0 and blk.hidden <= 2048 and self.fuse_dw is not False):
            self.dw_dot(name + ".dwpl", e, dwc, dwbn, pl, plbn, out, final_act)      # a dot product per pixel: bandwidth-bound
            return
        if dil == 1 and blk.expand_ratio != 1 and (self.fuse_dw or (
                self.fuse_dw is None and self.prec_for(name + ".dwpl") in ("f32", "f16x3") and stride == 1 and blk.hidden % 16 == 0
                and x.n * x.h * x.w * blk.hidden >= FUSE_DW_MIN_WORK and _dwproj_patch_waste(x.h, x.w) <= FUSE_DW_MAX_WASTE)):
            # depthwise computed inside the projection GEMM's loader: D never reaches HBM
            self.conv(name + ".dwpl", e, pl, plbn, out, final_act, res=x if blk.use_res_connect else None,
                      dw=(dwc, dwbn, stride))
            return
        res = x if blk.use_res_connect else None
        if dil == 1 and self._would_split(x.n, ho, wo, blk.hidden, out.c, 1, final_act, res is not None, out.ld,
                                          res.ld if res is not None else None):
            dd = self.scr_split(x.n, ho, wo, blk.hidden)      # D only ever exists as hi/lo fp16 planes
        else:
            dd = self.scr("D", x.n, ho, wo, blk.hidden)
        self.dw(name + ".dw", e, dwc, dwbn, dd, stride, dil)
        self.conv(name + ".pl", dd, pl, plbn, out, final_act, res=res)

    def mark(self, stage, start):
        self.stage_ranges[stage] = (start, len(self.ops_meta))
