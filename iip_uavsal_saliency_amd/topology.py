"""Reference `UAVSal.forward` (model.py:341-375) as calls on a Recorder: which op runs on which views, on which lane, in which
order -- and every launch-shape decision that depends on the plan's sizes, each with the measurement it rests on.  Knows
nothing of descriptors, addresses, allocation or which pass is running (recorder.py)."""
import torch

from . import _lib as L
from .views import V, _down


def record_forward(rec, cfg):
    """One pass over the plan: every op of the forward on `rec` (a Recorder), in launch order.  `cfg`: the engine's parsed
    settings, read only.  The sizing pass and the recording pass are the same calls."""
    m, N, h, w = cfg.model, cfg.N, cfg.h, cfg.w
    hw = h * w
    R6, NONE = L.ACT_RELU6, L.ACT_NONE
    feats = m.sfnet.features.features

    # ---- boundary: state and priors NCHW -> NHWC
    s0 = len(rec.ops_meta)
    h0 = rec.buf("h0", cfg.n_seq, h, w, 256, pinned=cfg.persistent)
    # buffers written by kernels that do not produce split shadows
    rec.no_shadow.update(("h0", "c0", "gauss_in", "ob_in", "f0", "ctx_sum", "lstm_pre", "lstm_c", "twa_pre"))
    rec.no_shadow.update("st%d_dif" % i for i in range(len(m.st_layer)))
    lstm = cfg.lstm
    c0 = rec.buf("c0", cfg.n_seq, h, w, 256, pinned=cfg.persistent) if lstm else None
    Np = 1 if cfg.static_priors else N
    # which priors this model has (reference model.py:281-324: a disabled prior has no net, and with none at all the two
    # fusion blocks do not exist either); enabled priors keep the reference's concat order gauss | observed | context
    use_g, use_o, use_c = cfg.use_priors
    num_cb = int(use_g) + int(use_o) + int(use_c)
    cb_off = {}
    for nm_, on_ in (("gauss", use_g), ("ob", use_o), ("ctx", use_c)):
        if on_:
            cb_off[nm_] = 64 * len(cb_off)
    g0 = rec.buf("gauss_in", Np, h, w, 8) if use_g else None
    o0 = rec.buf("ob_in", Np, h, w, 20) if use_o else None
    if not cfg.persistent:          # persistent mode: h0 / c0 ARE the state, staged only on demand (run())
        names = ["state.in"] + (["cstate.in"] if lstm else [])
        for nm, src, dst in zip(names, ("state_in", "cstate_in"), (h0, c0)):
            rec.layout(nm, rec.caller(src, cfg.n_seq, h, w, 256), dst, 1)
    rec.mark("boundary_in", s0)

    # ---- backbone: MobileNetV2 features[0:18] (model_feature.py:62-69)
    s0 = len(rec.ops_meta)
    H1, W1 = _down(cfg.H), _down(cfg.W)
    x = rec.buf("f0", N, H1, W1, 32)
    rec.stem("features.0", rec.caller("x", N, cfg.H, cfg.W, 3), feats[0][0], feats[0][1], x, u8=cfg.in_dtype == torch.uint8)
    tapsrc = {}
    cb = None
    # where the prior nets' side lane forks off: beside features.11-17 while those launches are latency-bound (one round of the
    # chip each: up to two clips of 8 frames; 4.26 -> 4.25 ms at one clip), beside features.5-10 from there on (8 clips: 27.92
    # vs 27.97 ms).  A function of the frame count only
    priors_at = 11 if N <= 16 else 5
    for i in range(1, 18):
        if i == priors_at:
            rec.mark("backbone.0-%d" % (priors_at - 1), s0)
            # ---- gaussian / observed prior nets (model.py:349,352): they depend only on the caller's
            #      priors and are needed at fucb_layer, so they run on lanes 1 and 2 beside the backbone.
            #      Recorded HERE, not at the top of the plan: the host launches in recording order, and
            #      with these 14 small launches (+ 4 event operations) in front of it the stem reached
            #      the GPU ~100 us late on every call (rocprofv3 kernel trace, profiles/r2_step_timeline.md).
            s0 = len(rec.ops_meta)
            cb = rec.buf("cb192", N, h, w, 64 * num_cb) if num_cb else None
            cbs = rec.buf("cb_static", 1, h, w, 128) if cfg.static_priors else cb
            rec.no_shadow.add("cb_static")
            # what the prior nets leave behind outlives the call: a later call with the same prior tensors does not run
            # them again (PriorCache.gate), so nothing else may ever be placed on these ranges (the `ctx` slice of cb192 is
            # still rewritten by every call; split shadows are allocations of their own anyway)
            if use_g or use_o:
                rec.pin(cb, cbs)
            # both nets on lane 1: one fork / join pair (two event operations fewer on the main stream than a lane each:
            # 4.29 -> 4.26 ms at one clip)
            priors_forked = use_g or use_o
            if priors_forked:
                rec.fork(1)
            for nm, src, dst, c, on in (("gauss", "cb0", g0, 8, use_g), ("ob", "cb1", o0, 20, use_o)):
                if not on:
                    continue
                blocks = m.gauss_cb_layer if nm == "gauss" else m.ob_cb_layer
                mid = rec.buf(nm + "1", Np, h, w, 64)
                sl = cb_off[nm]
                rec.layout(nm + ".in", rec.caller(src, Np, h, w, c), dst, 1)
                rec.ir_block(nm + ".0", dst, blocks[0], mid)
                rec.ir_block(nm + ".1", mid, blocks[1], cbs.slice(sl, 64))
                if cfg.static_priors:      # frame 0 of the net's output -> every frame (same-size resize: an exact copy)
                    rec.bilinear(nm + ".bcast", cbs.slice(sl, 64), cb.slice(sl, 64), src_mod=1)
            if priors_forked:
                rec.main()
            rec.mark("priors_side", s0)
            s0 = len(rec.ops_meta)
        blk = feats[i]
        ho, wo = (x.h - 1) // blk.stride + 1, (x.w - 1) // blk.stride + 1
        y = rec.buf("f%d" % i, N, ho, wo, blk.cout)
        rec.ir_block("features.%d" % i, x, blk, y)
        x = y
        tapsrc[i] = y
    c3, c4, c5 = tapsrc[6], tapsrc[13], tapsrc[17]
    rec.named.update(c3=c3, c4=c4, c5=c5)
    rec.mark("backbone.%d-17" % priors_at, s0)

    # ---- SRF-Net head (model.py:139-158)
    s0 = len(rec.ops_meta)
    sf = m.sfnet
    aspp = rec.buf("aspp", N, c5.h, c5.w, 1024)
    # the four ASPP branches and the two lateral convs are independent small launches on the
    # 1/32 and 1/16 scale maps: spread them over lanes so they fill the chip together
    x5 = rec.buf("x5", N, c5.h, c5.w, 256)
    x4 = rec.buf("x4", N, c4.h, c4.w, 128)
    # conv_last reads cat[interpolate(x5), interpolate(x4), conv_lv3(c3)] (model.py:151-156)
    cat = rec.buf("srf_cat", N, h, w, 448)
    branches = (sf.lv5_aspp2, sf.lv5_aspp3, sf.lv5_aspp4)
    # the three dilated branches expand the SAME map with the same shape: one GEMM with their output channels side by side
    # (320 -> 3 x 1920: 675 tiles instead of three launches of 225 fighting for the chip on three lanes)
    hid = branches[0].hidden
    e3 = rec.scr("E3", N, c5.h, c5.w, 3 * hid)
    rec.conv("aspp.pw", c5, [b.conv[0][0] for b in branches], [b.conv[0][1] for b in branches], e3, R6)
    aspp_grouped = cfg.prec_name == "f32"
    if aspp_grouped:
        # fp32: their three dilated depthwise convs are ONE launch too -- channel groups with their own dilation in the
        # whole-map kernel (uavsal_dw_desc.dil_group_c; three launches on three lanes cost six event operations on the main
        # stream, ~25 us between aspp.pw and aspp.pl, for ~10 us of overlap) -- and so are their three projections (1920 ->
        # 256 each, different inputs): output-channel groups with their own A columns (uavsal_conv_desc.n_group), K shared
        # out over workgroups
        d3 = rec.scr("D3", N, c5.h, c5.w, 3 * hid)
        rec.dw("aspp.dw", e3, [b.conv[1][0] for b in branches], [b.conv[1][1] for b in branches], d3, 1,
                [getattr(b, "dilation", 1) for b in branches])
    else:
        # every branch's depthwise + projection on its own lane, reading its slice
        for bi, b in enumerate(branches):
            rec.fork(3 + bi)
            rec.ir_block("aspp%d" % (bi + 2), c5, b, aspp.slice(256 * (bi + 1), 256), expanded=e3.slice(bi * hid, hid))
            rec.main()
    rec.fork(6)
    rec.conv("conv_lv4", c4, sf.conv_lv4[0], sf.conv_lv4[1], x4, R6)
    rec.bilinear("up_c4", x4, cat.slice(256, 128))
    rec.conv("conv_lv3", c3, sf.conv_lv3[0], sf.conv_lv3[1], cat.slice(384, 64), R6)
    rec.main()
    rec.conv("aspp1", c5, sf.lv5_aspp1[0], sf.lv5_aspp1[1], aspp.slice(0, 256), R6)
    if aspp_grouped:
        rec.conv("aspp.pl", d3.slice(0, hid), [b.conv[2] for b in branches], [b.conv[3] for b in branches],
                  aspp.slice(256, 768), NONE, cout=768, n_group=256)
    else:
        for lane in (3, 4, 5):
            rec.join(lane)
    rec.conv("conv_lv5", aspp, sf.conv_lv5[0], sf.conv_lv5[1], x5, R6)
    rec.bilinear("up_c5", x5, cat.slice(0, 256))
    rec.join(6)
    x = rec.buf("sfnet", N, h, w, 256)
    if cfg.winograd and rec.prec_for("conv_last") == "f32":
        rec.conv3_wino("conv_last", cat, sf.conv_last[0], sf.conv_last[1], x, R6, r=cfg.winograd_r)
    else:
        rec.conv("conv_last", cat, sf.conv_last[0], sf.conv_last[1], x, R6, taps=9)
    rec.mark("srf_head", s0)

    # ---- ST blocks (model.py:235-249)
    s0 = len(rec.ops_meta)
    for i, st in enumerate(m.st_layer):
        sp = rec.buf("st%d_sp" % i, N, h, w, 256)
        te = st.stconv_te
        r = rec.buf("st%d_red" % i, N, h, w, 32)
        dif = rec.buf("st%d_dif" % i, N, h, w, 64)
        t1 = rec.buf("st%d_te1" % i, N, h, w, 32)
        # temporal branch (small launches): from nine frames up its first two launches on the main lane (they would
        # otherwise queue behind a grid-filling GEMM for the whole of it), the rest on lane 6 next to the spatial branch's
        # big GEMMs; up to eight frames no side lane
        # (round 2, same box, two runs each: 5.26 / 5.25 / 5.22 ms for all on lane 6 / no lane / this split.  Round 5, one
        # clip: 4.234 / 4.221 for split / no lane -- the fork / join pair costs more than the overlap buys while the spatial
        # branch's GEMMs fill the chip anyway; eight clips: 27.97-28.10 / 28.31 for split / no lane)
        st_lane = N > 8
        rec.conv("st%d.reduce" % i, x, te.reduce_conv[0], te.reduce_conv[1], r, R6)
        rec.tdiff("st%d.tdiff" % i, r, dif, cfg.seq_len)
        if st_lane:
            rec.fork(6)
        rec.ir_block("st%d.sub" % i, dif, te.sub_conv, t1)
        if st_lane:
            rec.main()
        rec.ir_block("st%d.sp" % i, x, st.stconv_sp.spconv, sp)
        if st_lane:
            rec.join(6)
        ssum = rec.buf("st%d_sum" % i, N, h, w, 256)
        rec.conv("st%d.te_last" % i, t1, te.last_conv[0], te.last_conv[1], ssum, R6, res=sp)   # x_sp + x_te
        y = rec.buf("st%d" % i, N, h, w, 256)
        rec.conv("st%d.last" % i, ssum, st.stconv_last[0], st.stconv_last[1], y, R6, res=x)    # x + out
        x = y
    rec.mark("st_blocks", s0)

    # ---- fuse + multi-prior net (model.py:344-365)
    s0 = len(rec.ops_meta)
    if not num_cb:                   # no prior at all: the recurrence reads fust_layer's output (model.py:346, 367)
        xf = rec.buf("prefuse", N, h, w, 256)
        rec.ir_block("fust", x, m.fust_layer[0], xf)
    else:
        fu = rec.buf("fu320", N, h, w, 320)
        xs = fu.slice(0, 256)
        rec.ir_block("fust", x, m.fust_layer[0], xs)
        if use_c:
            B = N // cfg.ctx_T
            tsum = rec.buf("ctx_sum", B, h, w, 256)
            rec.tsum("ctx.sum", xs, tsum, cfg.ctx_T)
            h2, w2 = _down(h), _down(w)
            cx1 = rec.buf("ctx1", B, h2, w2, 64)
            rec.ir_block("ctx.0", tsum, m.cxt_cb_prior[0], cx1)
            h3, w3 = _down(h2), _down(w2)
            cx2 = rec.buf("ctx2", B, h3, w3, 64)
            rec.ir_block("ctx.1", cx1, m.cxt_cb_prior[1], cx2)
            cslot = cb.slice(cb_off["ctx"], 64)
            if cfg.ctx_mode == "tile":      # cb_cxt.repeat(T,1,1,1): frame k <- chunk k % B (model.py:361)
                rec.bilinear("ctx.up", cx2, cslot, src_mod=B, src_div=1)
            else:                            # independent clips: frame (c,t) <- clip c
                rec.bilinear("ctx.up", cx2, cslot, src_mod=N, src_div=cfg.ctx_T)
        if priors_forked:
            rec.join(1)
        rec.ir_block("fucb", cb, m.fucb_layer[0], fu.slice(256, 64))
        rec.named["fust_in_cb"] = fu.slice(256, 64)
        xf = rec.buf("prefuse", N, h, w, 256)
        rec.ir_block("fucbst", fu, m.fucbst_layer[0], xf)
    rec.mark("prior_fuse", s0)

    # ---- recurrence: ConvTWA (model_convlstm.py:276-292, 368-371) or ConvLSTM (:111-126, 206-222)
    s0 = len(rec.ops_meta)
    rc = m.rnn.cell_list[0].rnn_conv
    Lq = cfg.seq_len
    ro = rec.buf("rnn", N, h, w, 256)
    if lstm:
        pre = rec.buf("lstm_pre", N, h, w, 1024)      # W[:, :256] * x_t for all t, rows 4*c+gate
        rec.conv("lstm.wx", xf, rc, None, pre, NONE, taps=9, wslice=(0, 256), gate_interleave=256)
        co = rec.buf("lstm_c", N, h, w, 256)          # cell-state history
        for t in range(Lq):
            hp = rec.named["h0"] if t == 0 else ro.frames(t - 1, cfg.n_seq)
            cp = c0 if t == 0 else co.frames(t - 1, cfg.n_seq)
            a = V(hp.t, cfg.n_seq, h, w, 256, 256, hp.coff)
            st = hw if t == 0 else Lq * hw
            strides = {"a": st, "r": st, "o": Lq * hw, "x": Lq * hw}
            rec.conv("lstm.step%d" % t, a, rc, None, ro.frames(t, cfg.n_seq), NONE, taps=9,
                      wslice=(256, 512), gate_interleave=256, epi=L.EPI_LSTM, cout=1024,
                      res=V(cp.t, cfg.n_seq, h, w, 256, 256, cp.coff), aux=pre.frames(t, cfg.n_seq),
                      out2=co.frames(t, cfg.n_seq), n_img=cfg.n_seq, strides=strides)
        rec.named["lstm_c"] = co
    else:
        pre = rec.buf("twa_pre", N, h, w, 256)
        if cfg.winograd and rec.prec_for("twa.wx") == "f32":
            rec.conv3_wino("twa.wx", xf, rc, None, pre, NONE, wslice=(0, 256), r=cfg.winograd_r)
        else:
            rec.conv("twa.wx", xf, rc, None, pre, NONE, taps=9, wslice=(0, 256))    # W[:, :256] * x_t, all t
    for t in range(0 if lstm else Lq):
        a = h0 if t == 0 else ro.frames(t - 1, cfg.n_seq)
        a = V(a.t, cfg.n_seq, h, w, 256, 256, a.coff)
        strides = {"a": hw if t == 0 else Lq * hw, "o": Lq * hw, "r": Lq * hw, "x": Lq * hw}
        # (split-fp16 plans from four clips up: the per-step gate convolution in exact fp32 through Winograd F(4x4) as well -- 1.78x
        # fewer MFMA FLOPs than the direct 3x3 and it beats the split-fp16 implicit GEMM there: 136 vs 160 us per step at eight
        # clips, 17.89 -> 17.67 ms per eight-clip step.  Not more accurate: per launch at eight clips (tests/test_plan_ops_fp64.py,
        # teacher-forced against float64) its worst error is 2.0e-6 against 1.0e-6 for the direct split-fp16 step, both well inside
        # their bounds.  `model.winograd = False`: the direct split-fp16 step)
        f16_wino = (cfg.prec_name == "f16x3" and not cfg.prec_overrides and cfg.n_seq >= 4
                    and bool(getattr(m, "winograd", True)))
        if (cfg.winograd or f16_wino) and (f16_wino or rec.prec_for("twa.step") == "f32"):
            # one clip: 920 tiles of 2x2 fill the chip with 128x128 GEMM tiles; four clips and more: F(4x4) (1.78x
            # fewer FLOPs, smaller transforms) on 64x64 tiles (measured: 4.54 vs 4.61 ms at one clip, 29.47 vs 28.80 at eight)
            many = cfg.n_seq >= 4
            rec.conv3_wino("twa.step%d" % t, a, rc, None, ro.frames(t, cfg.n_seq), NONE, wslice=(256, 512),
                            n_img=cfg.n_seq, strides=strides, twa=(xf.frames(t, cfg.n_seq), pre.frames(t, cfg.n_seq)),
                            gemm_tile=11 if many else 8,
                            r=cfg.winograd_step_r or (4 if many else 2))
            continue
        rec.conv("twa.step%d" % t, a, rc, None, ro.frames(t, cfg.n_seq), NONE, taps=9, wslice=(256, 512),
                  epi=L.EPI_TWA, res=xf.frames(t, cfg.n_seq), aux=pre.frames(t, cfg.n_seq),
                  n_img=cfg.n_seq, strides=strides)
    rec.mark("twa", s0)

    # ---- decoder + sigmoid (model.py:372-373), state back to NCHW
    s0 = len(rec.ops_meta)
    outv = rec.caller("out", N, h, w, 1)
    if cfg.keep_taps:
        rec.ir_block("conv_out_st.logits", ro, m.conv_out_st, rec.caller("logits", N, h, w, 1), final_act=NONE)
    rec.ir_block("conv_out_st", ro, m.conv_out_st, outv, final_act=L.ACT_SIGMOID)
    outs = [(ro, "state_out", h0)] + ([(rec.named["lstm_c"], "cstate_out", c0)] if lstm else [])
    if cfg.persistent:
        # h_last of every clip (NHWC rows of the history) -> the resident state buffer, one strided copy
        for hist, _, keep in outs:
            rec.copy("state.keep", hist, keep, Lq)
        rec.guard(outv, h0, c0)
    else:
        for c in range(cfg.n_seq):
            for hist, dst, _ in outs:
                nm = "%s%d" % (dst.replace("_", "."), c)           # state.out0, cstate.out0, ...
                rec.layout(nm, hist.frames(c * Lq + Lq - 1, 1), rec.caller(dst, cfg.n_seq, h, w, 256).frames(c, 1), 0)
        rec.guard(outv, *(rec.caller(dst, cfg.n_seq, h, w, 256) for _, dst, _ in outs))
    rec.mark("decoder", s0)
