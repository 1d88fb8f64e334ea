"""What one fine-tuning step of the ConvTWA recurrence costs on the device, phase by phase.  Prints one JSON line.

At 360x640 frames (45x80 maps), one sequence of T = 20 (the reference's batch_size 4 x time_dims 5) and of T = 5 frames:
  forward      `model(x, cb, None, taps=...)`, the plan `train.recurrence_step` runs (it keeps prefuse and rnn);
  dec_grad     `train.decoder_input_grad`: e and d recomputed, `uavsal_dec_bwd`, the 1536 -> 256 GEMM;
  twa_backward the whole of `train.twa_backward` without the input gradient (what `recurrence_step` runs);
  wgrad        `uavsal_twa_wgrad` alone (two launches), with its TFLOP/s (2 * 256 * 4608 * T*45*80 FLOP) against the
               157.3 TFLOP/s fp32 MFMA peak; bptt = twa_backward - wgrad: the two gate convs, and per step the gate kernel and
               the 3x3 conv with flip(W_h)^T;
  step         `train.recurrence_step` as a whole (forward, criterion, its gradient, the two above);
  refresh      `model.refresh_weights(model.rnn)` after an in-place edit of the weight (host repacking and uploads);
  decoder      the decoder trained too: `train.decoder_backward` (dec_bwd_grad, beside dec_grad), its three new launches
               one by one -- `uavsal_pix_gemm` (pix_gemm: two launches, TFLOP/s from 2 * 1536 * 256 * T*45*80 FLOP),
               `uavsal_dec_sums` (dec_sums: GB/s from the e halo-free, d and ga bytes, 3 * 1536 * 4 per pixel, beside
               `uavsal_dec_bwd` at the same shape and byte count) and `uavsal_dec_finish` (dec_finish) --,
               `recurrence_step(decoder=True)` (step_dec, alternated with step in the same run) and
               `refresh_weights(model.rnn, model.conv_out_st)` (refresh_dec);
  fuse         the fusion block in front of the recurrence trained too (`train.fuse_block`: fucbst_layer[0], 320 -> 1920 ->
               256): `train.block_backward` as the step runs it (block_bwd, no input gradient) and with it (block_bwd_x),
               `uavsal_ir_bwd` and `uavsal_ir_sums` alone (GB/s from the bytes each must move: gd, d, e, ga = 4 * 1920 * 4
               per pixel, the sums' go on top; beside dec_bwd_kernel and dec_sums of the same run), both pixel GEMMs
               (pix_gemm_w1: ga x x, 1920 x 320 with its N tail; pix_gemm_w3: go x d, 256 x 1920; TFLOP/s),
               `recurrence_step(fuse=True)` (step_fuse, alternated with step in the same run),
               `refresh_weights(model.rnn, model.fucbst_layer)` (refresh_fuse), and an eager torch-autograd step of the
               same block (eager_block: forward + the nine parameter gradients from the same input and output gradient);
  fust         fust_layer[0] behind the priors trained too, the fourth stage: `recurrence_step(decoder=True, fuse=True)`
               (step3) and the same with `fust=True` (step4), alternated in the same run, every run listed (step3_all,
               step4_all: the spread); `train.fust_output_grad` as a whole (the frozen context-prior path: B = T / 5 images),
               the second `block_backward` (fust_block_bwd), the three launches of csrc/train_ctx.hip alone at the path's
               shapes (ir_bwd_s2: cxt_cb_prior[0], B x 45 x 80 x 1536; bilinear_bwd: T x 45 x 80 x 64 out of cb192 ->
               B x 12 x 20 x 64; tsum_bwd: T x 45 x 80 x 256), and `refresh_weights` over the four stages (refresh4);
  ctx          the multi-prior path trained too, the fifth stage (fucb_layer[0], cxt_cb_prior[1], cxt_cb_prior[0]): the
               four-stage step (step4b) and the same with `ctx=True` (step5), and `recurrence_step(decoder=True, fuse=True,
               ctx=True)` without fust (step4c), alternated in the same run, every run listed (the spread);
               `train.prior_path_backward` frozen (prior_path_frozen: what `fust_output_grad` runs) and with the 27 gradients
               (prior_path_trained); per trained block (fucb / ctx1 / ctx0) its channel sums alone (`uavsal_ir_sums` for the
               stride-1 fucb_layer[0], `uavsal_ir_sums_s2` for the two stride-2 blocks; GB/s from the bytes they must move:
               e and ga on the input grid, gd, d and go on the output grid) and its two pixel GEMMs with their reductions
               (w1: ga x x; w3: go x d with M = 64, half a tile); and `refresh_weights` over the five stages (refresh5);
  nets         the gauss / ob prior nets trained too, the sixth stage (both blocks of `gauss_cb_layer` and `ob_cb_layer`): the
               five-stage step (step5b) and the same with `nets=True` (step6), alternated in the same run, every run listed
               (the spread); the nets' backward alone as the step runs it on this benchmark's one prior map broadcast over
               the frames (nets_backward: per net `train.frame_sum` + `train.prior_net_backward` on ONE frame) and on
               materialised per-frame priors (nets_backward_frames: N frames); per net's narrow block 0 (gauss0: 8 -> 48 ->
               64, ob0: 20 -> 120 -> 64) `train.narrow_block_param_grads` from given parts (two launches) and its first
               launch `uavsal_ir_narrow_grads` alone, with the slab count; `uavsal_frame_sum` of one 64-channel slice of
               g_cb; and `refresh_weights` over the six stages (refresh6);
  st           the ST blocks trained too, the seventh stage (`model.st_layer`, 27 parameters per block): the six-stage step
               (step6b) and the same with `st=True` (step7), alternated in the same run, every run listed (the spread);
               `train.st_block_backward` of the last block (st_block_bwd_x: with the input gradient) and of block 0
               (st_block_bwd: without); and per launch family at a block's shapes, from the tensors the walk hands out:
               the forward's recompute (st_recompute: the nine launches), the spatial branch's `train.block_backward`
               (st_spconv_bwd), the sub-block's input-gradient walk and `train.block_param_grads` at 64 -> 384 -> 32
               (st_sub_walk, st_sub_param_grads), `train.cbr_backward` of the three 1x1 stages (st_cbr_last 256 -> 256,
               st_cbr_te_last 32 -> 256, st_cbr_reduce 256 -> 32), `uavsal_cbr_sums` alone at 256 and at 32 channels (GB/s
               from g, y read and gp written), `uavsal_tdiff_bwd` alone (GB/s from g_dif, r read and gp_r written), the
               pixel GEMM with its reduction at 256 x 256 (the 128 x 128 tile kernel) and at the three 32-wide shapes
               (st_pix_gemm_32x256, _256x32, _32x384: the sibling kernel; shares and TFLOP/s), and `refresh_weights` over
               the seven stages on the host and on the device (refresh7, refresh7_device).  Alone: --st-only;
  srf          the SRF-Net head trained too, the eighth stage (`train.srf_head`, 42 parameters): the seven-stage step (step7b)
               and the same with `srf=True` (step8), alternated in the same run, every run listed (the spread);
               `train.srf_head_backward` alone (srf_head_bwd) and per launch family at the head's shapes, from the tensors the
               walk hands out: `train.conv3_backward` of `conv_last` (srf_conv_last_bwd), `uavsal_conv3_wgrad` alone at
               [256,448,3,3] beside `uavsal_twa_wgrad` at the same K (srf_conv3_wgrad, srf_twa_wgrad_same_k: 72 tiles and the
               same loop; TFLOP/s of the useful and of the issued products), `uavsal_cbr_sums` at 256 channels, the resize's
               adjoint, `train.cbr_backward` of `conv_lv3`, `conv_lv4`, `conv_lv5`, one dilated branch's
               `train.block_param_grads` with `uavsal_ir_bwd_dil` and `uavsal_ir_sums_dil` alone, the pixel GEMM at 64 x 32,
               128 x 96 (the wave-per-tile kernel) and 256 x 1024, and `refresh_weights` over the eight stages on the host and
               on the device (refresh8, refresh8_device).  Alone: --srf-only;
  backbone     the deep backbone trained too, the ninth stage (`train.backbone_blocks`, 90 parameters): `backbone_phases`' docstring.
               Alone: --backbone-only;
  shallow      the shallow backbone trained too, the tenth stage (`train.shallow_blocks`, 54 parameters): `shallow_phases`' docstring.
               Alone: --shallow-only;
  lstm         the second model, `UAVSAL_LSTM`, trained through `recurrence_step(lstm=True)`: `lstm_phases`' docstring.
               Only with --lstm-only (a second model is built for it);
  fuse_bn      the fusion block on batch statistics, `recurrence_step(block_stats=("fuse",))`: `fuse_bn_phases`' docstring.
               Only with --fuse-bn-only (medians with every window listed);
  refresh pairs beside every refresh case above its `_device` twin: the same in-place edit, then `refresh_weights(...,
               device=True)` (csrc/repack.hip: one launch, no host copy); and at the end (or alone: --refresh-only) the
               host and device refresh of 1, 4, 5 and 6 stages (refreshN_alt / refreshN_device_alt) and one whole six-stage
               iteration -- step, `torch.optim.Adam.step`, refresh -- with either (iter6 / iter6_device), all alternated in
               the same run, every run listed (`_all_ms`: the spread), with the device path's launches, entries and bytes and the
               launch alone back to back (`refreshN_device_kernel_ms`);
  eager        torch autograd of the restated recurrence + decoder (float32, eval BatchNorm folded) on the same device,
               forward + backward from the same inputs, if torch's conv kernels run there.
Each is a host clock around `--iters` back-to-back calls ending in a synchronise, best of `--repeats`.

Usage:  python tools/train_bench.py [--iters 10] [--repeats 3] [--skip-eager] [--refresh-only] [--st-only] [--srf-only] [--backbone-only]
        [--shallow-only] [--lstm-only] [--decoder-bn-only] [--fuse-bn-only] [--frames 20 5]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from iip_uavsal_saliency_amd import UAVSal, losses, ops, synth, train      # noqa: E402
from iip_uavsal_saliency_amd import UAVSAL_LSTM                            # noqa: E402
from iip_uavsal_saliency_amd import _lib as L                              # noqa: E402
from iip_uavsal_saliency_amd import packing as P                           # noqa: E402
from iip_uavsal_saliency_amd.weights import WeightCache                    # noqa: E402

PEAK_TFLOPS = 157.3


def per_call(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def best_of(fn, iters, repeats):
    per_call(fn, 2)
    return min(per_call(fn, iters) for _ in range(repeats))


def eager_step(model, x_seq, h0, gy):
    """the restated recurrence + decoder under torch autograd: returns a function that runs forward + backward"""
    rc = model.rnn.cell_list[0].rnn_conv
    seq = model.conv_out_st.conv
    dev = x_seq.device
    fold = [tuple(t.to(dev).view(1, -1, 1, 1) for t in P.fold_bn(bn)) for bn in (seq[0][1], seq[1][1], seq[3])]
    w1, wd, w3 = seq[0][0].weight.detach(), seq[1][0].weight.detach(), seq[2].weight.detach()

    def run():
        w = rc.weight.detach().clone().requires_grad_(True)
        h, hs = h0, []
        for t in range(x_seq.shape[0]):
            i = torch.sigmoid(F.conv2d(torch.cat([x_seq[t:t + 1], h], 1), w, padding=1))
            h = i * x_seq[t:t + 1] + (1 - i) * h
            hs.append(h)
        hh = torch.cat(hs, 0)
        e = (F.conv2d(hh, w1) * fold[0][0] + fold[0][1]).clamp(0, 6)
        d = (F.conv2d(e, wd, padding=1, groups=wd.shape[0]) * fold[1][0] + fold[1][1]).clamp(0, 6)
        y = torch.sigmoid(F.conv2d(d, w3) * fold[2][0] + fold[2][1])
        return torch.autograd.grad(y, w, gy)[0]
    return run


def eager_block(blk, x, go):
    """the block (eval BatchNorm, as the package runs it) under torch autograd: forward + the nine parameter gradients"""
    seq = blk.conv
    bns = (seq[0][1], seq[1][1], seq[3])
    hid = seq[1][0].weight.shape[0]

    def bn(t, b, gamma, beta):
        return F.batch_norm(t, b.running_mean, b.running_var, gamma, beta, False, 0.0, b.eps)

    def run():
        ps = [q.detach().clone().requires_grad_(True) for q in blk.parameters()]
        w1, g1, b1, wd, g2, b2, w3, g3, b3 = ps
        e = bn(F.conv2d(x, w1), bns[0], g1, b1).clamp(0, 6)
        d = bn(F.conv2d(e, wd, padding=1, groups=hid), bns[1], g2, b2).clamp(0, 6)
        o = bn(F.conv2d(d, w3), bns[2], g3, b3)
        return torch.autograd.grad(o, ps, go)
    return run


def fuse_phases(res, m, x, cb, y_gaze, taps, grad_h, cache, iters, repeats, skip_eager):
    """the phases of the trained fusion block, added to `res`"""
    lib = L.load()
    dev = x.device
    cl = torch.channels_last
    rc = m.rnn.cell_list[0].rnn_conv
    blk, src = train.fuse_block(m)
    box = m.fucbst_layer if m.num_cb else m.fust_layer
    x_in = taps[src].contiguous(memory_format=cl)
    x_seq, h_seq = taps["prefuse"].contiguous(memory_format=cl), taps["rnn"].contiguous(memory_format=cl)
    _, grad_x, _ = train.twa_backward(x_seq, h_seq, None, rc.weight.detach(), grad_h, need_x_grad=True, cache=cache, module=rc)
    grad_x = grad_x.contiguous(memory_format=cl)
    parts = {}
    _, grads = train.block_backward(blk, x_in, grad_x, need_x_grad=False, cache=cache, parts=parts)
    e_, d_, gd_, ga_ = (parts[k] for k in ("e", "d", "gd", "ga"))
    pw, pwbn, dwc, dwbn, pl, plbn = train._block_parts(blk)
    hid, cin, cout = pw.weight.shape[0], pw.weight.shape[1], pl.weight.shape[0]
    w9, s2, _ = cache.depthwise(dwc, dwbn)
    s1, s3 = cache.affine(pwbn, hid)[0], cache.affine(plbn, cout)[0]
    xn, gon = x_in.permute(0, 2, 3, 1), grad_x.permute(0, 2, 3, 1)
    rd1 = torch.empty(hid, dtype=torch.float64, device=dev)
    rd3 = torch.empty(cout, dtype=torch.float64, device=dev)
    g1, g3 = grads[train.BLOCK_PARAMS[0]], grads[train.BLOCK_PARAMS[6]]
    n_pix = x_in.shape[0] * x_in.shape[2] * x_in.shape[3]

    def step():
        rc.weight.grad = None
        train.recurrence_step(m, x, cb, None, y_gaze)

    def step_fuse():
        for q in list(m.rnn.parameters()) + list(blk.parameters()):
            q.grad = None
        train.recurrence_step(m, x, cb, None, y_gaze, fuse=True)

    def refresh_fuse(device=False):
        with torch.no_grad():
            rc.weight.mul_(1.0)
            for q in blk.parameters():
                q.mul_(1.0)
        m.refresh_weights(m.rnn, box, device=device)
    cases = {"block_bwd": lambda: train.block_backward(blk, x_in, grad_x, need_x_grad=False, cache=cache, grads=grads),
             "block_bwd_x": lambda: train.block_backward(blk, x_in, grad_x, cache=cache, grads=grads),
             "ir_bwd": lambda: train.ir_bwd(gd_, d_, e_, w9, s2),
             "ir_sums": lambda: train.ir_sums(gd_, d_, e_, ga_, gon),
             "pix_gemm_w1": lambda: train.pix_gemm(ga_, xn, out=g1, row_scale=s1, w=pw.weight.detach(), rowdot=rd1),
             "pix_gemm_w3": lambda: train.pix_gemm(gon, d_, out=g3, row_scale=s3, w=pl.weight.detach(), rowdot=rd3),
             "refresh_fuse": refresh_fuse, "refresh_fuse_device": lambda: refresh_fuse(True)}
    for k, fn in cases.items():
        res[k + "_ms"] = 1e3 * best_of(fn, iters, repeats)
    alt = {"step": [], "step_fuse": []}                      # the two steps alternated in the same run
    for _ in range(repeats):
        alt["step"].append(per_call(step, iters))
        alt["step_fuse"].append(per_call(step_fuse, iters))
    res["step_alt2_ms"], res["step_fuse_ms"] = 1e3 * min(alt["step"]), 1e3 * min(alt["step_fuse"])
    for q in blk.parameters():
        q.grad = None
    res["fuse_block"] = [cin, hid, cout]
    res["ir_bwd_gbs"] = 4.0 * hid * 4 * n_pix / (res["ir_bwd_ms"] * 1e-3) / 1e9
    res["ir_sums_gbs"] = (4.0 * hid + cout) * 4 * n_pix / (res["ir_sums_ms"] * 1e-3) / 1e9
    for key, (M, N) in (("pix_gemm_w1", (hid, cin)), ("pix_gemm_w3", (cout, hid))):
        gd = L.PixGemmDesc()
        gd.K, gd.M, gd.N = n_pix, M, N
        res[key + "_shares"] = int(lib.uavsal_pix_gemm_shares(C.byref(gd)))
        res[key + "_tflops"] = 2.0 * M * N * n_pix / (res[key + "_ms"] * 1e-3) / 1e12
        res[key + "_of_peak"] = res[key + "_tflops"] / PEAK_TFLOPS
    if not skip_eager:
        try:
            run = eager_block(blk, x_in, grad_x)
            ge = run()
            res["eager_block_ms"] = 1e3 * best_of(run, max(1, iters // 2), repeats)
            train.block_backward(blk, x_in, grad_x, need_x_grad=False, cache=cache, grads=grads)
            res["eager_block_vs_hip_rel_l2"] = max(float((a - grads[n]).norm() / a.norm()) for a, n in zip(ge, train.BLOCK_PARAMS))
        except RuntimeError as e:                     # torch's own conv kernels may not exist for this device
            res["eager_block_error"] = str(e).splitlines()[0][:200]


def fust_phases(res, m, x, cb, y_gaze, grad_h, cache, iters, repeats):
    """the phases of the trained fust_layer behind the priors, added to `res`"""
    cl = torch.channels_last
    rc = m.rnn.cell_list[0].rnn_conv
    taps = {"fu320": None, "cb192": None}
    m(x, cb, None, taps=taps)
    fu, cb192 = taps["fu320"], taps["cb192"]
    st = taps["st%d" % (len(m.st_layer) - 1)].contiguous(memory_format=cl)
    x_seq, h_seq = taps["prefuse"].contiguous(memory_format=cl), taps["rnn"].contiguous(memory_format=cl)
    _, grad_x, _ = train.twa_backward(x_seq, h_seq, None, rc.weight.detach(), grad_h, need_x_grad=True, cache=cache, module=rc)
    grad_fu, _ = train.block_backward(m.fucbst_layer[0], fu, grad_x.contiguous(memory_format=cl), cache=cache)
    parts = {}
    g = train.fust_output_grad(m, fu, cb192, grad_fu, cache=cache, parts=parts)
    fb = m.fust_layer[0]
    _, grads = train.block_backward(fb, st, g, need_x_grad=False, cache=cache)
    # the three new launches at the shapes of the path: cxt_cb_prior[0]'s depthwise backward, the resize's adjoint, the chunk sum's
    ip = {}
    train.block_input_grad(m.cxt_cb_prior[0], parts["ctx_sum"].permute(0, 3, 1, 2), parts["g_ctx1"].permute(0, 3, 1, 2), cache=cache,
                           parts=ip)
    _, _, dwc, dwbn, _, _ = train._input_grad_parts(m.cxt_cb_prior[0])
    w9, s2, _ = cache.depthwise(dwc, dwbn)
    T, _, h, w = fu.shape
    B = T // m.time_dims
    off = 64 * (int(bool(m.use_gauss_prior)) + int(bool(m.use_ob_prior)))
    g_up = parts["g_cb"][..., off:off + 64]
    trained = [q for mod in (m.rnn, m.conv_out_st, m.fucbst_layer, m.fust_layer) for q in mod.parameters()]

    def step3():
        for q in trained:
            q.grad = None
        train.recurrence_step(m, x, cb, None, y_gaze, decoder=True, fuse=True)

    def step4():
        for q in trained:
            q.grad = None
        train.recurrence_step(m, x, cb, None, y_gaze, decoder=True, fuse=True, fust=True)

    def refresh4(device=False):
        with torch.no_grad():
            for q in trained:
                q.mul_(1.0)
        m.refresh_weights(m.rnn, m.conv_out_st, m.fucbst_layer, m.fust_layer, device=device)
    cases = {"fust_output_grad": lambda: train.fust_output_grad(m, fu, cb192, grad_fu, cache=cache),
             "fust_block_bwd": lambda: train.block_backward(fb, st, g, need_x_grad=False, cache=cache, grads=grads),
             "ir_bwd_s2": lambda: train.ir_bwd_s2(ip["gd"], ip["d"], ip["e"], w9, s2),
             "bilinear_bwd": lambda: train.bilinear_bwd(g_up, B, parts["g_ctx2"].shape[1], parts["g_ctx2"].shape[2], src_mod=B),
             "tsum_bwd": lambda: train.tsum_bwd(grad_fu.permute(0, 2, 3, 1)[..., :256], parts["g_sum"], m.time_dims),
             "refresh4": refresh4, "refresh4_device": lambda: refresh4(True)}
    for k, fn in cases.items():
        res[k + "_ms"] = 1e3 * best_of(fn, iters, repeats)
    alt = {"step3": [], "step4": []}                         # the two steps alternated in the same run
    for _ in range(repeats):
        alt["step3"].append(per_call(step3, iters))
        alt["step4"].append(per_call(step4, iters))
    res["step3_ms"], res["step4_ms"] = 1e3 * min(alt["step3"]), 1e3 * min(alt["step4"])
    res["step3_all_ms"], res["step4_all_ms"] = [1e3 * v for v in alt["step3"]], [1e3 * v for v in alt["step4"]]
    for q in trained:
        q.grad = None
    res["ir_bwd_s2_shape"], res["bilinear_bwd_shape"] = list(ip["e"].shape), [list(g_up.shape), list(parts["g_ctx2"].shape)]


def ctx_phases(res, m, x, cb, y_gaze, grad_h, cache, iters, repeats):
    """the phases of the trained multi-prior path (fucb_layer[0], cxt_cb_prior), the fifth stage, added to `res`"""
    lib = L.load()
    dev = x.device
    cl = torch.channels_last
    rc = m.rnn.cell_list[0].rnn_conv
    taps = {"fu320": None, "cb192": None}
    m(x, cb, None, taps=taps)
    fu, cb192 = taps["fu320"], taps["cb192"]
    x_seq, h_seq = taps["prefuse"].contiguous(memory_format=cl), taps["rnn"].contiguous(memory_format=cl)
    _, grad_x, _ = train.twa_backward(x_seq, h_seq, None, rc.weight.detach(), grad_h, need_x_grad=True, cache=cache, module=rc)
    grad_fu, _ = train.block_backward(m.fucbst_layer[0], fu, grad_x.contiguous(memory_format=cl), cache=cache)
    blocks = train.prior_path_blocks(m)
    parts = {}
    _, grads = train.prior_path_backward(m, fu, cb192, grad_fu, cache=cache, parts=parts, grads={n: None for n in blocks})
    boxes = (m.rnn, m.conv_out_st, m.fucbst_layer, m.fust_layer, m.fucb_layer, m.cxt_cb_prior)
    trained = [q for mod in boxes for q in mod.parameters()]

    def stepper(**kw):
        def run():
            for q in trained:
                q.grad = None
            train.recurrence_step(m, x, cb, None, y_gaze, decoder=True, fuse=True, **kw)
        return run

    def refresh5(device=False):
        with torch.no_grad():
            for q in trained:
                q.mul_(1.0)
        m.refresh_weights(*boxes, device=device)
    cases = {"prior_path_frozen": lambda: train.fust_output_grad(m, fu, cb192, grad_fu, cache=cache),
             "prior_path_trained": lambda: train.prior_path_backward(m, fu, cb192, grad_fu, cache=cache, grads=grads),
             "refresh5": refresh5, "refresh5_device": lambda: refresh5(True)}
    shapes = {}
    for name, blk in blocks.items():
        key = {"fucb_layer.0": "fucb", "cxt_cb_prior.1": "ctx1", "cxt_cb_prior.0": "ctx0"}[name]
        pt = parts[name]
        pw, pwbn, _, _, pl, plbn = train._param_grad_parts(blk)
        hid, cin, cout = pw.weight.shape[0], pw.weight.shape[1], pl.weight.shape[0]
        s1, s3 = cache.affine(pwbn, hid)[0], cache.affine(plbn, cout)[0]
        rd1 = torch.empty(hid, dtype=torch.float64, device=dev)
        rd3 = torch.empty(cout, dtype=torch.float64, device=dev)
        g1, g3 = grads[name][train.BLOCK_PARAMS[0]], grads[name][train.BLOCK_PARAMS[6]]
        sums = train.ir_sums if blk.stride == 1 else train.ir_sums_s2
        cases["%s_sums" % key] = lambda pt=pt, sums=sums: sums(pt["gd"], pt["d"], pt["e"], pt["ga"], pt["go"])
        cases["%s_pix_gemm_w1" % key] = lambda pt=pt, g1=g1, s1=s1, pw=pw, rd1=rd1: train.pix_gemm(
            pt["ga"], pt["x"], out=g1, row_scale=s1, w=pw.weight.detach(), rowdot=rd1)
        cases["%s_pix_gemm_w3" % key] = lambda pt=pt, g3=g3, s3=s3, pl=pl, rd3=rd3: train.pix_gemm(
            pt["go"], pt["d"], out=g3, row_scale=s3, w=pl.weight.detach(), rowdot=rd3)
        n_in = pt["e"].shape[0] * pt["e"].shape[1] * pt["e"].shape[2]
        n_out = pt["d"].shape[0] * pt["d"].shape[1] * pt["d"].shape[2]
        shapes[key] = dict(block=[cin, hid, cout], stride=blk.stride, e=list(pt["e"].shape), d=list(pt["d"].shape), n_in=n_in, n_out=n_out)
    for k, fn in cases.items():
        res[k + "_ms"] = 1e3 * best_of(fn, iters, repeats)
    for key, sh in shapes.items():
        cin, hid, cout = sh["block"]
        nbytes = 4.0 * (2 * hid * sh["n_in"] + (2 * hid + cout) * sh["n_out"])
        res["%s_sums_gbs" % key] = nbytes / (res["%s_sums_ms" % key] * 1e-3) / 1e9
        for tag, (M, N, K) in (("w1", (hid, cin, sh["n_in"])), ("w3", (cout, hid, sh["n_out"]))):
            gd = L.PixGemmDesc()
            gd.K, gd.M, gd.N = K, M, N
            res["%s_pix_gemm_%s_shares" % (key, tag)] = int(lib.uavsal_pix_gemm_shares(C.byref(gd)))
            res["%s_pix_gemm_%s_tflops" % (key, tag)] = 2.0 * M * N * K / (res["%s_pix_gemm_%s_ms" % (key, tag)] * 1e-3) / 1e12
    res["ctx_shapes"] = shapes
    runs = {"step4b": stepper(fust=True), "step5": stepper(fust=True, ctx=True), "step4c": stepper(ctx=True)}
    alt = {k: [] for k in runs}                               # the three steps alternated in the same run
    for _ in range(repeats):
        for k, fn in runs.items():
            alt[k].append(per_call(fn, iters))
    for k, v in alt.items():
        res[k + "_ms"], res[k + "_all_ms"] = 1e3 * min(v), [1e3 * t for t in v]
    for q in trained:
        q.grad = None


def nets_phases(res, m, x, cb, y_gaze, cache, iters, repeats):
    """the phases of the trained prior nets (gauss_cb_layer, ob_cb_layer), the sixth stage, added to `res`"""
    lib = L.load()
    taps = {"cb192": None}
    m(x, cb, None, taps=taps)
    g_cb = torch.randn_like(taps["cb192"]).permute(0, 2, 3, 1).contiguous()      # (timing only: any gradient of the right shape)
    nets = train.prior_nets(m)
    boxes = (m.rnn, m.conv_out_st, m.fucbst_layer, m.fust_layer, m.fucb_layer, m.cxt_cb_prior) + tuple(nets.values())
    trained = [q for mod in boxes for q in mod.parameters()]
    frames = [c.contiguous() for c in cb]                      # the same priors materialised per frame
    nchw = lambda t: t.permute(0, 3, 1, 2)                     # noqa: E731

    def stepper(**kw):
        def run():
            for q in trained:
                q.grad = None
            train.recurrence_step(m, x, cb, None, y_gaze, decoder=True, fuse=True, fust=True, ctx=True, **kw)
        return run

    def backward(static):
        def run():
            for i, net in enumerate(nets.values()):
                go, c = g_cb[..., 64 * i:64 * i + 64], (cb if static else frames)[i]
                if static:
                    go, c = train.frame_sum(go), c[:1]
                train.prior_net_backward(net, c, go, cache=cache)
        return run

    def refresh6(device=False):
        with torch.no_grad():
            for q in trained:
                q.mul_(1.0)
        m.refresh_weights(*boxes, device=device)
    cases = {"nets_backward": backward(True), "nets_backward_frames": backward(False), "refresh6": refresh6,
             "refresh6_device": lambda: refresh6(True),
             "frame_sum": lambda: train.frame_sum(g_cb[..., :64])}
    for i, (name, net) in enumerate(nets.items()):
        key = name.split("_")[0] + "0"
        for static in (True, False):
            go, c = g_cb[..., 64 * i:64 * i + 64], (cb if static else frames)[i]
            if static:
                go, c = train.frame_sum(go), c[:1]
            parts = {}
            train.prior_net_backward(net, c, go, cache=cache, parts=parts)
            p0 = parts["0"]
            tag = "%s_%s" % (key, "one_frame" if static else "frames")
            cases[tag + "_narrow"] = lambda p0=p0, net=net: train.narrow_block_param_grads(
                net[0], nchw(p0["x"]), p0["e"], p0["d"], nchw(p0["go"]), gd=p0["gd"], ga=p0["ga"], cache=cache)
            cases[tag + "_narrow_first"] = lambda p0=p0: train.ir_narrow_grads(p0["x"], p0["e"], p0["d"], p0["gd"], p0["ga"], p0["go"])
            d = L.IrNarrowDesc()
            d.n_img, d.H, d.W, d.Cin, d.Ch, d.Co = p0["e"].shape[0], p0["e"].shape[1], p0["e"].shape[2], p0["x"].shape[3], p0["e"].shape[3], 64
            res[tag + "_slabs"] = int(lib.uavsal_ir_narrow_slabs(C.byref(d)))
    for k, fn in cases.items():
        res[k + "_ms"] = 1e3 * best_of(fn, iters, repeats)
    runs = {"step5b": stepper(), "step6": stepper(nets=True)}
    alt = {k: [] for k in runs}                               # the two steps alternated in the same run
    for _ in range(repeats):
        for k, fn in runs.items():
            alt[k].append(per_call(fn, iters))
    for k, v in alt.items():
        res[k + "_ms"], res[k + "_all_ms"] = 1e3 * min(v), [1e3 * t for t in v]
    for q in trained:
        q.grad = None


def st_phases(res, m, x, cb, y_gaze, cache, iters, repeats):
    """the phases of the trained ST blocks (model.st_layer), the seventh stage, added to `res`"""
    lib = L.load()
    dev = x.device
    cl = torch.channels_last
    nets = tuple(train.prior_nets(m).values())
    boxes = (m.rnn, m.conv_out_st, m.fucbst_layer, m.fust_layer, m.fucb_layer, m.cxt_cb_prior) + nets + (m.st_layer,)
    trained = [q for mod in boxes for q in mod.parameters()]
    kw6 = dict(decoder=True, fuse=True, fust=True, ctx=True, nets=True)
    taps = {}
    m(x, cb, None, taps=taps)
    n_st = len(m.st_layer)
    blk = m.st_layer[n_st - 1]
    x_in = (taps["st%d" % (n_st - 2)] if n_st > 1 else taps["sfnet"]).contiguous(memory_format=cl)
    x0 = taps["sfnet"].contiguous(memory_format=cl)
    go = (torch.randn_like(x_in) / x_in[0].numel()).contiguous(memory_format=cl)      # (timing only: any gradient of the right shape)
    T = x_in.shape[0]
    pt = {}
    _, grads = train.st_block_backward(blk, x_in, go, seq_len=T, cache=cache, parts=pt)
    _, grads0 = train.st_block_backward(m.st_layer[0], x0, go, seq_len=T, need_x_grad=False, cache=cache)
    nchw = lambda t: t.permute(0, 3, 1, 2)                     # noqa: E731
    te = blk.stconv_te
    xn, gon = x_in.permute(0, 2, 3, 1), go.permute(0, 2, 3, 1)
    n_pix = xn.shape[0] * xn.shape[1] * xn.shape[2]
    sub = {n: grads["stconv_te.sub_conv." + n] for n in train.BLOCK_PARAMS}
    spg = {n: grads["stconv_sp.spconv." + n] for n in train.BLOCK_PARAMS}
    cbr = {k: {n: grads[p + n] for n in train.ST_CBR_PARAMS}
           for k, p in (("last", "stconv_last."), ("te_last", "stconv_te.last_conv."), ("reduce", "stconv_te.reduce_conv."))}
    p_sub = train._input_grad_parts(te.sub_conv)

    def recompute():
        train._block_recompute(lib, cache, blk.stconv_sp.spconv, xn)
        train._conv(lib, cache, pt["d_sp"], blk.stconv_sp.spconv.conv[2], 256, 1, bn=blk.stconv_sp.spconv.conv[3])
        train._conv(lib, cache, xn, te.reduce_conv[0], 32, 1, bn=te.reduce_conv[1], act=L.ACT_RELU6)
        ops.tdiff(pt["r"], T)
        train._block_recompute(lib, cache, te.sub_conv, pt["dif"], 1, p_sub)
        train._conv(lib, cache, pt["d_te"], p_sub[4], 32, 1, bn=p_sub[5])
        train._conv(lib, cache, pt["t1"], te.last_conv[0], 256, 1, bn=te.last_conv[1], act=L.ACT_RELU6)
        train.tsum_bwd(pt["a_te"], pt["x_sp"], 1)
        train._conv(lib, cache, pt["ssum"], blk.stconv_last[0], 256, 1, bn=blk.stconv_last[1], act=L.ACT_RELU6)

    def stepper(**kw):
        def run():
            for q in trained:
                q.grad = None
            train.recurrence_step(m, x, cb, None, y_gaze, **kw6, **kw)
        return run

    def refresh7(device=False):
        with torch.no_grad():
            for q in trained:
                q.mul_(1.0)
        m.refresh_weights(*boxes, device=device)
    gems = {}
    for tag, (a, b, M, N) in (("256x256", (pt["g_sum"], pt["ssum"], 256, 256)), ("32x256", (pt["gp_r"], xn, 32, 256)),
                              ("256x32", (pt["g_sum"], pt["t1"], 256, 32)), ("32x384", (pt["g_t1"], pt["d_te"], 32, 384))):
        out = torch.empty((M, N), dtype=torch.float32, device=dev)
        rd = torch.empty(M, dtype=torch.float64, device=dev)
        w = torch.randn((M, N), dtype=torch.float32, device=dev)
        rsc = torch.ones(M, dtype=torch.float32, device=dev)
        gems[tag] = (M, N, lambda a=a, b=b, out=out, rd=rd, w=w, rsc=rsc: train.pix_gemm(a, b, out=out, row_scale=rsc, w=w, rowdot=rd))
    cases = {"st_block_bwd_x": lambda: train.st_block_backward(blk, x_in, go, seq_len=T, cache=cache, grads=grads),
             "st_block_bwd": lambda: train.st_block_backward(m.st_layer[0], x0, go, seq_len=T, need_x_grad=False, cache=cache, grads=grads0),
             "st_recompute": recompute,
             "st_spconv_bwd": lambda: train._block_backward(blk.stconv_sp.spconv, x_in, nchw(pt["g_sum"]), True, cache, None, spg, False,
                                                            ed=(pt["e_sp"], pt["d_sp"]), res=gon),
             "st_sub_walk": lambda: train._input_grad(lib, cache, te.sub_conv, p_sub, pt["dif"], pt["g_t1"], ed=(pt["e_te"], pt["d_te"])),
             "st_sub_param_grads": lambda: train.block_param_grads(te.sub_conv, nchw(pt["dif"]), pt["e_te"], pt["d_te"], nchw(pt["g_t1"]),
                                                                   gd=pt["sub"]["gd"], ga=pt["sub"]["ga"], cache=cache, out=sub),
             "st_cbr_last": lambda: train.cbr_backward(blk.stconv_last[0], blk.stconv_last[1], nchw(pt["ssum"]), pt["o"], go, cache=cache,
                                                       grads=cbr["last"]),
             "st_cbr_te_last": lambda: train.cbr_backward(te.last_conv[0], te.last_conv[1], nchw(pt["t1"]), pt["a_te"], nchw(pt["g_sum"]),
                                                          cache=cache, grads=cbr["te_last"]),
             "st_cbr_reduce": lambda: train._cbr_backward(te.reduce_conv[0], te.reduce_conv[1], x_in, pt["r"], nchw(pt["gp_r"]), True, cache,
                                                          cbr["reduce"], False, res=pt["gx_sp"]),
             "st_cbr_sums_256": lambda: train.cbr_sums(gon, pt["o"]),
             "st_cbr_sums_32": lambda: train.cbr_sums(pt["gp_r"], pt["r"]),
             "st_tdiff_bwd": lambda: train.tdiff_bwd(pt["g_dif"], pt["r"], T),
             "refresh7": refresh7, "refresh7_device": lambda: refresh7(True)}
    for tag, (_, _, fn) in gems.items():
        cases["st_pix_gemm_" + tag] = fn
    for k, fn in cases.items():
        res[k + "_ms"] = 1e3 * best_of(fn, iters, repeats)
    for tag, (M, N, _) in gems.items():
        gd = L.PixGemmDesc()
        gd.K, gd.M, gd.N = n_pix, M, N
        res["st_pix_gemm_%s_shares" % tag] = int(lib.uavsal_pix_gemm_shares(C.byref(gd)))
        res["st_pix_gemm_%s_tflops" % tag] = 2.0 * M * N * n_pix / (res["st_pix_gemm_%s_ms" % tag] * 1e-3) / 1e12
    res["st_cbr_sums_256_gbs"] = 3.0 * 256 * 4 * n_pix / (res["st_cbr_sums_256_ms"] * 1e-3) / 1e9
    res["st_cbr_sums_32_gbs"] = 3.0 * 32 * 4 * n_pix / (res["st_cbr_sums_32_ms"] * 1e-3) / 1e9
    res["st_tdiff_bwd_gbs"] = 4.0 * 32 * 4 * n_pix / (res["st_tdiff_bwd_ms"] * 1e-3) / 1e9
    runs = {"step6b": stepper(), "step7": stepper(st=True)}
    for fn in runs.values():
        per_call(fn, 2)
    alt = {k: [] for k in runs}                               # the two steps alternated in the same run
    for _ in range(repeats):
        for k, fn in runs.items():
            alt[k].append(per_call(fn, iters))
    for k, v in alt.items():
        res[k + "_ms"], res[k + "_all_ms"] = 1e3 * min(v), [1e3 * t for t in v]
    for q in trained:
        q.grad = None


def srf_phases(res, m, x, cb, y_gaze, cache, iters, repeats):
    """the phases of the trained SRF-Net head (train.srf_head), the eighth stage, added to `res`"""
    lib = L.load()
    dev = x.device
    cl = torch.channels_last
    nets = tuple(train.prior_nets(m).values())
    head = tuple(train.srf_head(m))
    boxes = (m.rnn, m.conv_out_st, m.fucbst_layer, m.fust_layer, m.fucb_layer, m.cxt_cb_prior) + nets + (m.st_layer,) + head
    trained = [q for mod in boxes for q in mod.parameters()]
    kw7 = dict(decoder=True, fuse=True, fust=True, ctx=True, nets=True, st=True)
    taps = {}
    m(x, cb, None, taps=taps)
    c3, c4, c5, y = (taps[k].contiguous(memory_format=cl) for k in ("c3", "c4", "c5", "sfnet"))
    go = (torch.randn_like(y) / y[0].numel()).contiguous(memory_format=cl)      # (timing only: any gradient of the right shape)
    pt = {}
    grads = train.srf_head_backward(m.sfnet, c3, c4, c5, y, go, cache=cache, parts=pt)
    sf = m.sfnet
    nchw = lambda t: t.permute(0, 3, 1, 2)                     # noqa: E731
    yn, gon = y.permute(0, 2, 3, 1), go.permute(0, 2, 3, 1)
    T, hh, ww, _ = yn.shape
    n_pix, n5 = T * hh * ww, T * c5.shape[2] * c5.shape[3]
    sub = lambda name, names: {n: grads["%s.%s" % (name, n)] for n in names}      # noqa: E731
    gp, _, _ = train.cbr_sums(gon, yn)
    b2 = sf.lv5_aspp2
    prt = train._param_grad_parts(b2)
    w9, s2 = cache.depthwise(prt[2], prt[3])[:2]
    # uavsal_twa_wgrad at the same K, 72 tiles and the same loop: the recurrence's own operands stand in (256-wide x, h, h0)
    tw = [torch.randn((T, hh, ww, 256), device=dev) for _ in range(3)] + [torch.zeros((1, hh, ww, 256), device=dev)]
    gw_twa = torch.empty((256, 512, 3, 3), device=dev)
    gw_c3 = torch.empty_like(sf.conv_last[0].weight)

    def stepper(**kw):
        def run():
            for q in trained:
                q.grad = None
            train.recurrence_step(m, x, cb, None, y_gaze, **kw7, **kw)
        return run

    def refresh8(device=False):
        with torch.no_grad():
            for q in trained:
                q.mul_(1.0)
        m.refresh_weights(*boxes, device=device)
    gems = {}
    for tag, (a, b, M, N) in (("64x32", (pt["g_cat"][..., 384:], c3.permute(0, 2, 3, 1), 64, 32)),
                              ("128x96", (pt["g_x4"], c4.permute(0, 2, 3, 1), 128, 96)),
                              ("256x1024", (pt["g_x5"], pt["aspp"], 256, 1024))):
        out = torch.empty((M, N), dtype=torch.float32, device=dev)
        gems[tag] = (M, N, a.shape[0] * a.shape[1] * a.shape[2], lambda a=a, b=b, out=out: train.pix_gemm(a, b, out=out))
    cases = {"srf_head_bwd": lambda: train.srf_head_backward(sf, c3, c4, c5, y, go, cache=cache, grads=grads),
             "srf_conv_last_bwd": lambda: train.conv3_backward(sf.conv_last[0], sf.conv_last[1], nchw(pt["cat"]), yn, go, cache=cache,
                                                               grads=sub("conv_last", train.ST_CBR_PARAMS)),
             "srf_conv3_wgrad": lambda: train.conv3_wgrad(gp, pt["cat"], out=gw_c3),
             "srf_twa_wgrad_same_k": lambda: train.twa_wgrad(tw[0], tw[1], tw[2], tw[3], out=gw_twa),
             "srf_cbr_sums_256": lambda: train.cbr_sums(gon, yn),
             "srf_bilinear_bwd_256": lambda: train.bilinear_bwd(pt["g_cat"][..., :256], T, c5.shape[2], c5.shape[3]),
             "srf_cbr_lv3": lambda: train.cbr_backward(sf.conv_lv3[0], sf.conv_lv3[1], c3, pt["x3"], nchw(pt["g_cat"][..., 384:]),
                                                       need_x_grad=False, cache=cache, grads=sub("conv_lv3", train.ST_CBR_PARAMS)),
             "srf_cbr_lv4": lambda: train.cbr_backward(sf.conv_lv4[0], sf.conv_lv4[1], c4, pt["x4"], nchw(pt["g_x4"]), need_x_grad=False,
                                                       cache=cache, grads=sub("conv_lv4", train.ST_CBR_PARAMS)),
             "srf_cbr_lv5": lambda: train.cbr_backward(sf.conv_lv5[0], sf.conv_lv5[1], nchw(pt["aspp"]), pt["x5"], nchw(pt["g_x5"]),
                                                       cache=cache, grads=sub("conv_lv5", train.ST_CBR_PARAMS)),
             "srf_aspp_branch_param_grads": lambda: train.block_param_grads(b2, c5, pt["e2"], pt["d2"], nchw(pt["g_aspp"][..., 256:512]),
                                                                            gd=pt["gd2"], ga=pt["ga2"], cache=cache,
                                                                            out=sub("lv5_aspp2", train.BLOCK_PARAMS)),
             "srf_ir_bwd_dil": lambda: train.ir_bwd_dil(pt["gd2"], pt["d2"], pt["e2"], w9, s2, b2.dilation),
             "srf_ir_sums_dil": lambda: train.ir_sums_dil(pt["gd2"], pt["d2"], pt["e2"], pt["ga2"], pt["g_aspp"][..., 256:512], b2.dilation),
             "refresh8": refresh8, "refresh8_device": lambda: refresh8(True)}
    for tag, (_, _, _, fn) in gems.items():
        cases["srf_pix_gemm_" + tag] = fn
    for k, fn in cases.items():
        res[k + "_ms"] = 1e3 * best_of(fn, iters, repeats)
    for tag, (M, N, K, _) in gems.items():
        gd = L.PixGemmDesc()
        gd.K, gd.M, gd.N = K, M, N
        res["srf_pix_gemm_%s_shares" % tag] = int(lib.uavsal_pix_gemm_shares(C.byref(gd)))
        res["srf_pix_gemm_%s_tflops" % tag] = 2.0 * M * N * K / (res["srf_pix_gemm_%s_ms" % tag] * 1e-3) / 1e12
    d = L.Conv3WgradDesc()
    d.n_img, d.H, d.W, d.Co, d.Ci = T, hh, ww, 256, 448
    res["srf_conv3_wgrad_shares"] = int(lib.uavsal_conv3_wgrad_shares(C.byref(d)))
    res["srf_conv3_wgrad_tflops"] = 2.0 * 256 * 9 * 448 * n_pix / (res["srf_conv3_wgrad_ms"] * 1e-3) / 1e12
    res["srf_conv3_wgrad_issued_tflops"] = 2.0 * 256 * 9 * 512 * n_pix / (res["srf_conv3_wgrad_ms"] * 1e-3) / 1e12
    res["srf_twa_wgrad_same_k_tflops"] = 2.0 * 256 * 9 * 512 * n_pix / (res["srf_twa_wgrad_same_k_ms"] * 1e-3) / 1e12
    res["srf_ir_bwd_dil_gbs"] = 4.0 * 1920 * 4 * n5 / (res["srf_ir_bwd_dil_ms"] * 1e-3) / 1e9
    runs = {"step7b": stepper(), "step8": stepper(srf=True)}
    for fn in runs.values():
        per_call(fn, 2)
    alt = {k: [] for k in runs}                               # the two steps alternated in the same run
    for _ in range(repeats):
        for k, fn in runs.items():
            alt[k].append(per_call(fn, iters))
    for k, v in alt.items():
        res[k + "_ms"], res[k + "_all_ms"] = 1e3 * min(v), [1e3 * t for t in v]
    for q in trained:
        q.grad = None


def backbone_phases(res, m, x, cb, y_gaze, cache, iters, repeats):
    """the phases of the trained deep backbone (train.backbone_blocks: MobileNetV2 features[8:18]), the ninth stage, added to
    `res`: the six weight-gradient shapes `uavsal_pix_gemm` takes with `tails32`, alone, at the K they have in the walk (1/16
    scale: 23 x 40, 1/32: 12 x 20 per frame) beside 256 x 256 at the 1/16 K (ms, TFLOP/s, shares, workgroups);
    `train.backbone_backward` alone; the eight-stage step (step8b) and the same with `backbone=True` (step9), and one whole
    nine-stage iteration -- step, Adam, refresh -- with host and with device refresh (iter9 / iter9_device), all alternated in
    the same run, every run listed (`_all_ms`: the spread)."""
    lib = L.load()
    dev = x.device
    cl = torch.channels_last
    nets = tuple(train.prior_nets(m).values())
    boxes = ((m.rnn, m.conv_out_st, m.fucbst_layer, m.fust_layer, m.fucb_layer, m.cxt_cb_prior) + nets + (m.st_layer,)
             + tuple(train.srf_head(m)) + tuple(train.backbone_blocks(m)))
    trained = [q for mod in boxes for q in mod.parameters()]
    kw8 = dict(decoder=True, fuse=True, fust=True, ctx=True, nets=True, st=True, srf=True)
    taps = {}
    m(x, cb, None, taps=taps)
    c3, c4, c5 = (taps[k].contiguous(memory_format=cl) for k in ("c3", "c4", "c5"))
    T = c3.shape[0]
    g4 = (torch.randn_like(c4) / c4[0].numel()).contiguous(memory_format=cl)      # (timing only: any gradient of the right shape)
    g5 = (torch.randn_like(c5) / c5[0].numel()).contiguous(memory_format=cl)
    feats = m.sfnet.features.features
    grads = train.backbone_backward(feats, c3, g4, g5, cache=cache)
    grids = {16: tuple(c4.shape[2:]), 32: tuple(c5.shape[2:])}
    gems = {}
    for M, N, scale in ((576, 96, 16), (960, 160, 32), (96, 384, 16), (96, 576, 16), (160, 576, 32), (160, 960, 32), (256, 256, 16)):
        hh, ww = grids[scale]
        a = 1e-2 * torch.randn((T, hh, ww, M), device=dev)
        b = torch.randn((T, hh, ww, N), device=dev)
        out = torch.empty((M, N), dtype=torch.float32, device=dev)
        gems["%dx%d" % (M, N)] = (M, N, T * hh * ww, lambda a=a, b=b, out=out: train.pix_gemm(a, b, out=out, tails32=True))
    cases = {"backbone_bwd": lambda: train.backbone_backward(feats, c3, g4, g5, cache=cache, grads=grads)}
    for tag, (_, _, _, fn) in gems.items():
        cases["backbone_pix_gemm_" + tag] = fn
    for k, fn in cases.items():
        res[k + "_ms"] = 1e3 * best_of(fn, iters, repeats)
    for tag, (M, N, K, _) in gems.items():
        gd = L.PixGemmDesc()
        gd.K, gd.M, gd.N, gd.tails32 = K, M, N, 1
        sh = int(lib.uavsal_pix_gemm_shares(C.byref(gd)))
        res["backbone_pix_gemm_%s_K" % tag], res["backbone_pix_gemm_%s_shares" % tag] = K, sh
        res["backbone_pix_gemm_%s_workgroups" % tag] = -(-M // 128) * -(-N // 128) * sh
        res["backbone_pix_gemm_%s_tflops" % tag] = 2.0 * M * N * K / (res["backbone_pix_gemm_%s_ms" % tag] * 1e-3) / 1e12
    opt = torch.optim.Adam(trained, lr=1e-4, betas=(0.9, 0.999), weight_decay=5e-5)

    def stepper(**kw):
        def run():
            for q in trained:
                q.grad = None
            train.recurrence_step(m, x, cb, None, y_gaze, **kw8, **kw)
        return run

    def iteration(device):
        def run():
            opt.zero_grad()
            train.recurrence_step(m, x, cb, None, y_gaze, backbone=True, **kw8)
            opt.step()
            m.refresh_weights(*boxes, device=device)
        return run
    runs = {"step8b": stepper(), "step9": stepper(backbone=True), "iter9": iteration(False), "iter9_device": iteration(True)}
    for fn in runs.values():
        per_call(fn, 2)
    alt = {k: [] for k in runs}                               # alternated in the same run, every run listed
    for _ in range(repeats):
        for k, fn in runs.items():
            alt[k].append(per_call(fn, iters))
    for k, v in alt.items():
        res[k + "_ms"], res[k + "_all_ms"] = 1e3 * min(v), [1e3 * t for t in v]
    for q in trained:
        q.grad = None


def shallow_phases(res, m, x, cb, y_gaze, cache, iters, repeats):
    """the phases of the trained shallow backbone (train.shallow_blocks: MobileNetV2 features[2:8]), the tenth stage, added to
    `res`: the five weight-gradient shapes `uavsal_skinny_wgrad` takes, alone with their reduce launch, at the K they have in
    the walk (ms, operand bytes / time as a fraction of 8 TB/s, shares) beside the only way the parent forms them -- operands
    zero-padded to multiples of 32 in torch (not timed), then `train.pix_gemm(tails32=True)` (`_padded_ms`);
    `train.shallow_backward` alone; the nine-stage step (step9b) and the same with `shallow=True` (step10), and one whole
    ten-stage iteration -- step, Adam, refresh -- with host and with device refresh (iter10 / iter10_device), all alternated in
    the same run, every run listed (`_all_ms`: the spread); the peak device memory of the ten-stage step."""
    lib = L.load()
    dev = x.device
    cl = torch.channels_last
    nets = tuple(train.prior_nets(m).values())
    boxes = ((m.rnn, m.conv_out_st, m.fucbst_layer, m.fust_layer, m.fucb_layer, m.cxt_cb_prior) + nets + (m.st_layer,)
             + tuple(train.srf_head(m)) + tuple(train.backbone_blocks(m)) + tuple(train.shallow_blocks(m)))
    trained = [q for mod in boxes for q in mod.parameters()]
    kw9 = dict(decoder=True, fuse=True, fust=True, ctx=True, nets=True, st=True, srf=True, backbone=True)
    taps = {}
    m(x, cb, None, taps=taps)
    c3, c4 = (taps[k].contiguous(memory_format=cl) for k in ("c3", "c4"))
    T, H, W = x.shape[0], x.shape[2], x.shape[3]
    down = lambda v: (v - 1) // 2 + 1                                     # noqa: E731
    g3 = (torch.randn_like(c3) / c3[0].numel()).contiguous(memory_format=cl)      # (timing only: any gradient of the right shape)
    g7 = (torch.randn((T, 64) + tuple(c4.shape[2:]), device=dev) / c4[0].numel()).contiguous(memory_format=cl)
    feats = m.sfnet.features.features
    grads = train.shallow_backward(feats, x, g3, g7, cache=cache)
    grids = {2: (down(H), down(W)), 4: (down(down(H)), down(down(W))), 8: tuple(c3.shape[2:])}
    gems = {}
    pad32 = lambda t: F.pad(t, (0, -t.shape[-1] % 32))                    # noqa: E731
    for M, N, scale in ((96, 16, 2), (144, 24, 4), (24, 96, 4), (24, 144, 4), (32, 144, 8)):
        hh, ww = grids[scale]
        a = 1e-2 * torch.randn((T, hh, ww, M), device=dev)
        b = torch.randn((T, hh, ww, N), device=dev)
        out = torch.empty((M, N), dtype=torch.float32, device=dev)
        ap, bp = pad32(a), pad32(b)
        outp = torch.empty((ap.shape[-1], bp.shape[-1]), dtype=torch.float32, device=dev)
        gems["%dx%d" % (M, N)] = (M, N, T * hh * ww, lambda a=a, b=b, out=out: train.skinny_wgrad(a, b, out=out),
                                  lambda a=ap, b=bp, out=outp: train.pix_gemm(a, b, out=out, tails32=True))
    res["shallow_bwd_ms"] = 1e3 * best_of(lambda: train.shallow_backward(feats, x, g3, g7, cache=cache, grads=grads), iters, repeats)
    for tag, (M, N, K, fn, fnp) in gems.items():                          # the pair alternated, every run listed
        per_call(fn, 2), per_call(fnp, 2)
        mine, theirs = [], []
        for _ in range(repeats):
            mine.append(1e3 * per_call(fn, 4 * iters))
            theirs.append(1e3 * per_call(fnp, 4 * iters))
        gd = L.SkinnyWgradDesc()
        gd.K, gd.M, gd.N = K, M, N
        k = "shallow_skinny_wgrad_" + tag
        res[k + "_ms"], res[k + "_all_ms"], res[k + "_padded_ms"], res[k + "_padded_all_ms"] = min(mine), mine, min(theirs), theirs
        res[k + "_K"], res[k + "_shares"] = K, int(lib.uavsal_skinny_wgrad_shares(C.byref(gd)))
        res[k + "_of_8TBs"] = (M + N) * K * 4 / (min(mine) * 1e-3) / 8e12
    del gems
    opt = torch.optim.Adam(trained, lr=1e-4, betas=(0.9, 0.999), weight_decay=5e-5)

    def stepper(**kw):
        def run():
            for q in trained:
                q.grad = None
            train.recurrence_step(m, x, cb, None, y_gaze, **kw9, **kw)
        return run

    def iteration(device):
        def run():
            opt.zero_grad()
            train.recurrence_step(m, x, cb, None, y_gaze, shallow=True, **kw9)
            opt.step()
            m.refresh_weights(*boxes, device=device, fused_t=True)
        return run
    runs = {"step9b": stepper(), "step10": stepper(shallow=True), "iter10": iteration(False), "iter10_device": iteration(True)}
    for fn in runs.values():
        per_call(fn, 2)
    alt = {k: [] for k in runs}                               # alternated in the same run, every run listed
    for _ in range(repeats):
        for k, fn in runs.items():
            alt[k].append(per_call(fn, iters))
    for k, v in alt.items():
        res[k + "_ms"], res[k + "_all_ms"] = 1e3 * min(v), [1e3 * t for t in v]
    for name, fn in (("step9b", runs["step9b"]), ("step10", runs["step10"])):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        fn()
        torch.cuda.synchronize()
        res[name + "_peak_MB"] = torch.cuda.max_memory_allocated(dev) / 1e6
    for q in trained:
        q.grad = None


def lstm_phases(res, m, x, cb, y_gaze, iters, repeats):
    """the phases of the ConvLSTM backward (train.lstm_backward, csrc/train_lstm.hip), added to `res`; `m` is the ConvTWA model
    of the other phases, a `UAVSAL_LSTM` with the same synthetic weights is built beside it.  `lstm_backward` alone with and
    without `grad_x`; its launches alone from the tensors the walk hands out: the recompute of `cc` (two convs), `uavsal_lstm_scan`
    and ONE `uavsal_lstm_gate_bwd` with both carries (ms and operand bytes / time as a fraction of 8 TB/s: 3 C floats read per frame and
    C written, and 13 C read and 5 C written, per pixel), one carry conv, the T-step loop (gate kernel + carry conv per step: `loop_ms`,
    and per step), `grad_x`'s conv, `uavsal_conv3_wgrad` at [1024,512,3,3] (shares, TFLOP/s); and, alternated in the same run with every
    run listed (`_all_ms`: the spread), the ("rnn",) step and the ten-stage Adam iteration with device refresh of both models."""
    lib = L.load()
    dev = x.device
    cl = torch.channels_last
    T = x.shape[0]
    ml = UAVSAL_LSTM(time_dims=m.time_dims)
    synth.load_synth_weights(ml, 0)
    ml = ml.to(dev).eval()
    rc = ml.rnn.cell_list[0].rnn_conv
    cache = WeightCache(torch.device(dev), ml._wshared.setdefault(str(torch.device(dev)), {}))
    taps = {}
    out, _ = ml(x, cb, None, taps=taps)
    x_seq, h_seq = taps["prefuse"].contiguous(memory_format=cl), taps["rnn"].contiguous(memory_format=cl)
    pred = out.detach().requires_grad_(True)
    g_y = torch.autograd.grad(losses.loss_fu(pred, y_gaze), pred)[0]
    grad_h = train.decoder_input_grad(ml.conv_out_st, h_seq, g_y, cache=cache, y=out)
    w = rc.weight.detach()
    gw = torch.empty_like(rc.weight)
    parts = {}
    _, _, g0, gc0 = train.lstm_backward(x_seq, h_seq, None, None, w, grad_h, need_x_grad=True, out=gw, cache=cache, module=rc, parts=parts)
    cc, cs, dcc = parts["cc"], parts["c_seq"], parts["dcc"]
    hh, ww = cc.shape[1:3]
    xn, hn = x_seq.permute(0, 2, 3, 1), h_seq.permute(0, 2, 3, 1)
    hprev = torch.cat([torch.zeros_like(hn[:1]), hn[:T - 1]], 0).contiguous()
    cat = torch.cat([xn, hprev], 3)
    Gn = grad_h.permute(0, 2, 3, 1)
    ch, ccar = g0.permute(0, 2, 3, 1).contiguous(), gc0.permute(0, 2, 3, 1).contiguous()
    zero = torch.zeros_like(ccar)
    d1, co1 = torch.empty_like(cc[:1]), torch.empty_like(ccar)

    def recompute():
        a = train._conv(lib, cache, xn, rc, 1024, 9, wslice=(0, 256))
        return train._conv(lib, cache, hprev, rc, 1024, 9, wslice=(256, 512), res=a)

    def loop():
        carry = None
        for t in range(T - 1, -1, -1):
            train.lstm_gate_bwd(Gn[t:t + 1], carry, co1 if carry is not None else None, cc[t:t + 1], cs[t:t + 1],
                                cs[t - 1:t] if t else zero, dcc=dcc[t:t + 1], carry_c_out=co1)
            carry = train._conv(lib, cache, dcc[t:t + 1], rc, 256, 9, wslice=(256, 512), transposed=True)
    cases = {"lstm_backward": lambda: train.lstm_backward(x_seq, h_seq, None, None, w, grad_h, out=gw, cache=cache, module=rc),
             "lstm_backward_x": lambda: train.lstm_backward(x_seq, h_seq, None, None, w, grad_h, need_x_grad=True, out=gw, cache=cache, module=rc),
             "lstm_cc": recompute,
             "lstm_scan": lambda: train.lstm_scan(cc, None),
             "lstm_gate": lambda: train.lstm_gate_bwd(Gn[:1], ch, ccar, cc[:1], cs[:1], zero, dcc=d1, carry_c_out=co1),
             "lstm_carry_conv": lambda: train._conv(lib, cache, dcc[:1], rc, 256, 9, wslice=(256, 512), transposed=True),
             "lstm_loop": loop,
             "lstm_grad_x": lambda: train._conv(lib, cache, dcc, rc, 256, 9, wslice=(0, 256), transposed=True),
             "lstm_wgrad": lambda: train.conv3_wgrad(dcc, cat, out=gw)}
    for k, fn in cases.items():
        res[k + "_ms"] = 1e3 * best_of(fn, 4 * iters if k in ("lstm_scan", "lstm_gate", "lstm_carry_conv") else iters, repeats)
    px = hh * ww
    res["lstm_loop_per_step_ms"] = res["lstm_loop_ms"] / T
    res["lstm_scan_of_8TBs"] = 4.0 * 256 * 4 * T * px / (res["lstm_scan_ms"] * 1e-3) / 8e12
    res["lstm_gate_of_8TBs"] = 18.0 * 256 * 4 * px / (res["lstm_gate_ms"] * 1e-3) / 8e12
    flop = 2.0 * 1024 * 4608 * T * px
    gd = L.Conv3WgradDesc()
    gd.n_img, gd.H, gd.W, gd.Co, gd.Ci = T, hh, ww, 1024, 512
    res["lstm_wgrad_shares"] = int(lib.uavsal_conv3_wgrad_shares(C.byref(gd)))
    res["lstm_wgrad_tflops"] = flop / (res["lstm_wgrad_ms"] * 1e-3) / 1e12
    res["lstm_cc_tflops"] = flop / (res["lstm_cc_ms"] * 1e-3) / 1e12
    res["lstm_grad_x_tflops"] = 0.5 * flop / (res["lstm_grad_x_ms"] * 1e-3) / 1e12
    res["lstm_carry_conv_tflops"] = 0.5 * flop / T / (res["lstm_carry_conv_ms"] * 1e-3) / 1e12
    del parts, cc, cs, dcc, cat
    kw10 = dict(decoder=True, fuse=True, fust=True, ctx=True, nets=True, st=True, srf=True, backbone=True, shallow=True)

    def boxes_of(mm):
        return ((mm.rnn, mm.conv_out_st, mm.fucbst_layer, mm.fust_layer, mm.fucb_layer, mm.cxt_cb_prior) + tuple(train.prior_nets(mm).values())
                + (mm.st_layer,) + tuple(train.srf_head(mm)) + tuple(train.backbone_blocks(mm)) + tuple(train.shallow_blocks(mm)))

    def stepper(mm, **kw):
        w_ = mm.rnn.cell_list[0].rnn_conv.weight

        def run():
            w_.grad = None
            train.recurrence_step(mm, x, cb, None, y_gaze, **kw)
        return run

    def iteration(mm, **kw):
        boxes = boxes_of(mm)
        opt = torch.optim.Adam([q for b in boxes for q in b.parameters()], lr=1e-4, betas=(0.9, 0.999), weight_decay=5e-5)

        def run():
            opt.zero_grad()
            train.recurrence_step(mm, x, cb, None, y_gaze, **kw10, **kw)
            opt.step()
            mm.refresh_weights(*boxes, device=True, fused_t=True)
        return run
    runs = {"step_twa": stepper(m), "step_lstm": stepper(ml, lstm=True),
            "iter10_device_twa": iteration(m), "iter10_device_lstm": iteration(ml, lstm=True)}
    for fn in runs.values():
        per_call(fn, 2)
    alt = {k: [] for k in runs}                               # alternated in the same run, every run listed
    for _ in range(repeats):
        for k, fn in runs.items():
            alt[k].append(per_call(fn, iters))
    for k, v in alt.items():
        res[k + "_ms"], res[k + "_all_ms"] = 1e3 * min(v), [1e3 * t for t in v]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    runs["step_lstm"]()
    torch.cuda.synchronize()
    res["step_lstm_peak_MB"] = torch.cuda.max_memory_allocated(dev) / 1e6
    for mm in (m, ml):
        for q in mm.parameters():
            q.grad = None


def decoder_bn_phases(res, m, x, cb, y_gaze, cache, iters, repeats):
    """the phases of the decoder on BATCH statistics (train.decoder_forward_batch / decoder_backward_batch, csrc/train_bn.hip),
    added to `res`: the two batch functions alone; every launch of theirs alone from the tensors the walk hands out (`bn_*_ms`
    and, for the memory-bound ones, the bytes the launch must move over its time as a fraction of 8 TB/s: `*_of_8TBs`; a
    1536-channel tensor at T frames of 45 x 80 is T * 22.1 MB); and, alternated in the same run with every run listed
    (`_all_ms`: the spread), the two-stage step ("rnn", "decoder") without the keyword and with `batch_stats=("decoder",)`,
    each followed by the device refresh of both stages as a training loop follows it (`iter_dec*`: a step on batch statistics
    moves the running statistics, so a forward WITHOUT the refresh behind it drops and rebuilds the plans -- no loop does that,
    and a step timed alone would time the rebuild), the refresh alone, the step without the keyword alone (`step_dec_ms`, timed
    before any batch step ran), and the peak memory of either iteration."""
    from iip_uavsal_saliency_amd.train import bn as B
    lib = L.load()
    dev = x.device
    cl = torch.channels_last
    blk = m.conv_out_st
    taps = {}
    m(x, cb, None, taps=taps)
    h_seq = taps["rnn"].contiguous(memory_format=cl)
    hn = h_seq.permute(0, 2, 3, 1)
    T, hh, ww, _ = hn.shape
    blk.train()
    y, sv = train.decoder_forward_batch(blk, h_seq, update_running=False, cache=cache)
    pred = y.detach().requires_grad_(True)
    g_y = torch.autograd.grad(losses.loss_fu(pred, y_gaze), pred)[0]
    parts = {}
    _, grads = train.decoder_backward_batch(blk, h_seq, g_y, saved=sv, parts=parts, cache=cache)
    pw, bn1, dwc, bn2, pl, bn3 = train.decoder._decoder_parts_batch(blk, "train_bench")
    u1, e, u2, u3, f1, f2, f3 = (sv[k] for k in ("u1", "e", "u2", "u3", "f1", "f2", "f3"))
    g_u1, g_u2, g_u3, g_e = (parts[k] for k in ("g_u1", "g_u2", "g_u3", "g_e"))
    gy = g_y.contiguous().view(T, hh, ww, 1)
    w3 = pl.weight.detach().reshape(-1)
    w9 = cache.depthwise(dwc, bn2)[0]
    s3 = B.bn_bwd_sums(gy, u3, f3, "sigmoid")
    s2 = B.bn_bwd_sums((g_u3, w3), u2, f2, "relu6")
    s1 = B.bn_bwd_sums(g_e, u1, f1, "relu6")
    big = 1536.0 * 4 * T * hh * ww                              # bytes of one 1536-channel tensor
    launches = {                                               # name: (call, 1536-channel tensors moved; 0: not memory bound / tiny)
        "bn_gemm_u1": (lambda: train._conv(lib, cache, hn, pw, 1536, 1), 0),
        "bn_stats1": (lambda: B.bn_stats(u1, bn1.weight, bn1.bias, bn1.eps), 1),
        "bn_apply1": (lambda: B.bn_apply(u1, f1, "relu6"), 2),
        "bn_dw_raw": (lambda: train.decoder._dw_raw(lib, e, w9), 2),
        "bn_stats2": (lambda: B.bn_stats(u2, bn2.weight, bn2.bias, bn2.eps), 1),
        "bn_apply_dot": (lambda: B.bn_apply(u2, f2, "relu6", dot_w=w3), 1),
        "bn_stats3": (lambda: B.bn_stats(u3, bn3.weight, bn3.bias, bn3.eps), 0),
        "bn_apply3": (lambda: B.bn_apply(u3, f3, "sigmoid"), 0),
        "bn_bwd_sums3": (lambda: B.bn_bwd_sums(gy, u3, f3, "sigmoid"), 0),
        "bn_bwd_apply3": (lambda: B.bn_bwd_apply(gy, u3, f3, s3, "sigmoid"), 0),
        "bn_bwd_sums2": (lambda: B.bn_bwd_sums((g_u3, w3), u2, f2, "relu6"), 1),
        "bn_bwd_apply2": (lambda: B.bn_bwd_apply((g_u3, w3), u2, f2, s2, "relu6"), 2),
        "bn_dw_wgrad": (lambda: B.dw_wgrad(g_u2, e, out=grads[train.DECODER_PARAMS[3]]), 2),
        "bn_dw_raw_t": (lambda: train.decoder._dw_raw(lib, g_u2, w9.flip(0).contiguous()), 2),
        "bn_bwd_sums1": (lambda: B.bn_bwd_sums(g_e, u1, f1, "relu6"), 2),
        "bn_bwd_apply1": (lambda: B.bn_bwd_apply(g_e, u1, f1, s1, "relu6"), 3),
        "bn_pix_gemm": (lambda: train.pix_gemm(g_u1, hn, out=grads[train.DECODER_PARAMS[0]]), 0),
        "bn_gemm_grad_h": (lambda: train._conv(lib, cache, g_u1, pw, 256, 1, transposed=True), 0)}
    for k, (fn, tensors) in launches.items():
        res[k + "_ms"] = 1e3 * best_of(fn, iters, repeats)
        if tensors:
            res[k + "_of_8TBs"] = tensors * big / (res[k + "_ms"] * 1e-3) / 8e12
    res["bn_slabs"], res["bn_slab_rows"] = B.slabs(T, hh, ww)
    res["bn_tensor_MB"] = big / 1e6
    res["dec_forward_batch_ms"] = 1e3 * best_of(lambda: train.decoder_forward_batch(blk, h_seq, update_running=False, cache=cache), iters, repeats)
    res["dec_forward_batch_running_ms"] = 1e3 * best_of(lambda: train.decoder_forward_batch(blk, h_seq, cache=cache), iters, repeats)
    res["dec_backward_batch_ms"] = 1e3 * best_of(lambda: train.decoder_backward_batch(blk, h_seq, g_y, saved=sv, grads=grads, cache=cache), iters, repeats)
    blk.eval()
    res["dec_backward_eval_ms"] = 1e3 * best_of(lambda: train.decoder_backward(blk, h_seq, g_y, cache=cache, grads=grads), iters, repeats)
    del parts, sv, u1, e, u2, g_u1, g_u2, g_e
    trained = list(m.rnn.parameters()) + list(blk.parameters())

    def stepper(batch, refresh=True):
        def run():
            for q in trained:
                q.grad = None
            blk.train(batch)
            train.recurrence_step(m, x, cb, None, y_gaze, decoder=True, **({"batch_stats": ("decoder",)} if batch else {}))
            blk.eval()
            if refresh:
                m.refresh_weights(m.rnn, blk, device=True)
        return run
    res["step_dec_ms"] = 1e3 * best_of(stepper(False, refresh=False), iters, repeats)
    runs = {"iter_dec": stepper(False), "iter_dec_batch": stepper(True)}
    for fn in runs.values():
        per_call(fn, 2)
    alt = {k: [] for k in runs}                               # alternated in the same run, every run listed
    for _ in range(repeats):
        for k, fn in runs.items():
            alt[k].append(per_call(fn, iters))
    for k, v in alt.items():
        res[k + "_ms"], res[k + "_all_ms"] = 1e3 * min(v), [1e3 * t for t in v]
    for k, fn in runs.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        fn()
        torch.cuda.synchronize()
        res[k + "_peak_MB"] = torch.cuda.max_memory_allocated(dev) / 1e6
    res["refresh_dec_device_ms"] = 1e3 * best_of(lambda: m.refresh_weights(m.rnn, blk, device=True), iters, repeats)
    for q in trained:
        q.grad = None


def _median(v):
    v = sorted(v)
    return 0.5 * (v[(len(v) - 1) // 2] + v[len(v) // 2])


def fuse_bn_phases(res, m, x, cb, y_gaze, cache, iters, repeats):
    """the phases of the fusion block on BATCH statistics (train.block_forward_batch / block_backward_batch, train.twa_forward;
    csrc/train_bn.hip: uavsal_bn_apply_res), added to `res`.  Every figure is the MEDIAN of `--repeats` windows of `--iters`
    back-to-back calls ending in a synchronise, with every window listed (`_all_ms`: the spread): the two block functions and
    `twa_forward` alone on the plan's own taps (`lstm_forward`: a second model, `lstm_forward_ms`); `uavsal_bn_apply_res` alone at
    256 channels beside `uavsal_bn_apply` (`*_of_8TBs`: the bytes the launch must move over its time as a fraction of 8 TB/s);
    the eval-mode `block_backward` beside them; and, alternated in the same run, one iteration -- the three-stage step
    ("rnn", "decoder", "fuse") followed by the device refresh of the three stages, as a training loop follows it (a step on
    batch statistics moves the running statistics, so a forward WITHOUT the refresh behind it drops and rebuilds the plans) --
    without a keyword (`iter_fuse`), with `block_stats=("fuse",)` (`iter_fuse_block`) and with `batch_stats=("decoder",)` as well
    (`iter_fuse_both`), the step without the keywords alone (`step_fuse3_ms`, timed before any batch step ran), and the peak
    memory of each iteration."""
    from iip_uavsal_saliency_amd.train import bn as B
    dev = x.device
    cl = torch.channels_last
    blk, src = train.fuse_block(m)
    box = train.fuse_container(m)
    dec, rc = m.conv_out_st, m.rnn.cell_list[0].rnn_conv
    taps = {src: None}
    m(x, cb, None, taps=taps)
    fu = taps[src].contiguous(memory_format=cl)
    x_seq = taps["prefuse"].contiguous(memory_format=cl)
    T, _, hh, ww = fu.shape

    def timed(key, fn):
        per_call(fn, 2)
        v = [1e3 * per_call(fn, iters) for _ in range(repeats)]
        res[key + "_ms"], res[key + "_all_ms"] = _median(v), v
    box.train()
    out, sv = train.block_forward_batch(blk, fu, update_running=False, cache=cache)
    go = torch.randn_like(out) / (hh * ww)
    grads = train.block_backward_batch(blk, fu, go, saved=sv, cache=cache)[1]
    timed("block_forward_batch", lambda: train.block_forward_batch(blk, fu, update_running=False, cache=cache))
    timed("block_forward_batch_running", lambda: train.block_forward_batch(blk, fu, cache=cache))
    timed("block_backward_batch", lambda: train.block_backward_batch(blk, fu, go, saved=sv, grads=grads, cache=cache))
    f3, u3 = sv["f3"], sv["u3"]
    resid = x_seq.permute(0, 2, 3, 1)
    small = 256.0 * 4 * T * hh * ww                              # bytes of one 256-channel tensor
    timed("bn_apply_res256", lambda: B.bn_apply(u3, f3, None, res=resid))
    timed("bn_apply256", lambda: B.bn_apply(u3, f3, None))
    res["bn_apply_res256_of_8TBs"] = 3 * small / (res["bn_apply_res256_ms"] * 1e-3) / 8e12
    res["bn_apply256_of_8TBs"] = 2 * small / (res["bn_apply256_ms"] * 1e-3) / 8e12
    del sv, f3, u3
    box.eval()
    timed("block_backward_eval", lambda: train.block_backward(blk, fu, go, cache=cache, grads=grads))
    timed("twa_forward", lambda: train.twa_forward(x_seq, None, rc.weight.detach(), cache=cache, module=rc))
    mine = train.twa_forward(x_seq, None, rc.weight.detach(), cache=cache, module=rc)
    res["twa_forward_vs_plan_max_abs"] = float((mine - taps["rnn"]).abs().max())
    res["twa_forward_vs_plan_rel_l2"] = float((mine - taps["rnn"]).norm() / taps["rnn"].norm())
    del mine
    trained = list(m.rnn.parameters()) + list(dec.parameters()) + list(box.parameters())

    def stepper(block, batch, refresh=True):
        kw = dict(decoder=True, fuse=True)
        if block:
            kw["block_stats"] = ("fuse",)
        if batch:
            kw["batch_stats"] = ("decoder",)

        def run():
            for q in trained:
                q.grad = None
            box.train(block)
            dec.train(batch)
            train.recurrence_step(m, x, cb, None, y_gaze, **kw)
            box.eval()
            dec.eval()
            if refresh:
                m.refresh_weights(m.rnn, dec, box, device=True)
        return run
    timed("step_fuse3", stepper(False, False, refresh=False))
    runs = {"iter_fuse": stepper(False, False), "iter_fuse_block": stepper(True, False), "iter_fuse_both": stepper(True, True)}
    for fn in runs.values():
        per_call(fn, 2)
    alt = {k: [] for k in runs}                               # alternated in the same run, every run listed
    for _ in range(repeats):
        for k, fn in runs.items():
            alt[k].append(1e3 * per_call(fn, iters))
    for k, v in alt.items():
        res[k + "_ms"], res[k + "_all_ms"] = _median(v), v
    for k, fn in runs.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        fn()
        torch.cuda.synchronize()
        res[k + "_peak_MB"] = torch.cuda.max_memory_allocated(dev) / 1e6
    timed("refresh_fuse3_device", lambda: m.refresh_weights(m.rnn, dec, box, device=True))
    for q in trained:
        q.grad = None
    # the ConvLSTM forward: the second model, its own plan's prefuse tap
    ml = UAVSAL_LSTM(time_dims=m.time_dims)
    synth.load_synth_weights(ml, 0)
    ml = ml.to(dev).eval()
    tl = {}
    ml(x, cb, None, taps=tl)
    xl = tl["prefuse"].contiguous(memory_format=cl)
    rl = ml.rnn.cell_list[0].rnn_conv
    lcache = WeightCache(torch.device(dev), ml._wshared.setdefault(str(torch.device(dev)), {}))
    timed("lstm_forward", lambda: train.lstm_forward(xl, None, None, rl.weight.detach(), cache=lcache, module=rl))
    hl = train.lstm_forward(xl, None, None, rl.weight.detach(), cache=lcache, module=rl)[0]
    res["lstm_forward_vs_plan_max_abs"] = float((hl - tl["rnn"]).abs().max())
    res["lstm_forward_vs_plan_rel_l2"] = float((hl - tl["rnn"]).norm() / tl["rnn"].norm())


def refresh_phases(res, m, x, cb, y_gaze, iters, repeats):
    """host and device refresh of 1, 4, 5 and 6 stages and one whole six-stage iteration with either, added to `res`"""
    from iip_uavsal_saliency_amd import repack
    nets = tuple(train.prior_nets(m).values())
    sets = {1: (m.rnn,), 4: (m.rnn, m.conv_out_st, m.fucbst_layer, m.fust_layer)}
    sets[5] = sets[4] + (m.fucb_layer, m.cxt_cb_prior)
    sets[6] = sets[5] + nets
    trained = [q for mod in sets[6] for q in mod.parameters()]
    kw = dict(decoder=True, fuse=True, fust=True, ctx=True, nets=True)
    for q in trained:
        q.grad = None
    train.recurrence_step(m, x, cb, None, y_gaze, **kw)           # the store holds every packed form a six-stage step reads

    def refresher(boxes, device):
        mine = [q for mod in boxes for q in mod.parameters()]

        def run():
            with torch.no_grad():
                for q in mine:
                    q.mul_(1.0)
            m.refresh_weights(*boxes, device=device)
        return run
    opt = torch.optim.Adam(trained, lr=1e-4, betas=(0.9, 0.999), weight_decay=5e-5)

    def iteration(device):
        def run():
            opt.zero_grad()
            train.recurrence_step(m, x, cb, None, y_gaze, **kw)
            opt.step()
            m.refresh_weights(*sets[6], device=device)
        return run
    runs = {}
    for n, boxes in sets.items():
        runs["refresh%d_alt" % n], runs["refresh%d_device_alt" % n] = refresher(boxes, False), refresher(boxes, True)
    runs["iter6"], runs["iter6_device"] = iteration(False), iteration(True)
    for fn in runs.values():
        per_call(fn, 2)
    alt = {k: [] for k in runs}                               # every pair alternated in the same run, every run listed
    for _ in range(repeats):
        for k, fn in runs.items():
            alt[k].append(per_call(fn, iters))
    for k, v in alt.items():
        res[k + "_ms"], res[k + "_all_ms"] = 1e3 * min(v), [1e3 * t for t in v]
    store = m._wshared[str(x.device)]
    for n, boxes in sets.items():                             # what one device refresh is: launches, entries, bytes written
        rec = store[(repack.TABLE_KIND, tuple(sorted(id(s) for b in boxes for s in b.modules())))]
        res["refresh%d_device_launches" % n] = 1 if rec.table is not None else 0
        res["refresh%d_device_entries" % n], res["refresh%d_device_blocks" % n] = rec.n_entries, rec.blocks
        res["refresh%d_device_bytes" % n], res["refresh%d_keys" % n] = rec.bytes_written, rec.count
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)       # the launch alone, back to back: the kernel's own time
        res["refresh%d_device_kernel_ms" % n] = 1e3 * best_of(lambda rec=rec: L.check(L.load().uavsal_repack(
            C.c_void_p(rec.table.data_ptr()), rec.n_entries, rec.blocks, stream), "uavsal_repack"), 4 * iters, repeats)
    for q in trained:
        q.grad = None


def bench(T, iters, repeats, dev, skip_eager, refresh_only=False, st_only=False, srf_only=False, backbone_only=False,
          shallow_only=False, lstm_only=False, decoder_bn_only=False, fuse_bn_only=False):
    H, W, h, w = 360, 640, 45, 80
    m = UAVSal(time_dims=5 if T % 5 == 0 else 4)            # (--frames 8: two chunks of four)
    synth.load_synth_weights(m, 0)
    m = m.to(dev).eval()
    x = torch.from_numpy(synth.normalize_frames(synth.synth_frames_u8(T, H, W, 3))).to(dev)
    gp = torch.from_numpy(synth.gauss_priors(1, h, w)[0]).to(dev)
    op_ = torch.from_numpy(synth.ob_priors(1, h, w)[0]).to(dev)
    cb = [gp.unsqueeze(0).expand(T, -1, -1, -1), op_.unsqueeze(0).expand(T, -1, -1, -1)]
    loc = synth.synth_fix_points(T, 360, 640, 20, 4)
    fmap = np.rint(synth.synth_fix_maps(loc, 8.0) * 255).astype(np.uint8)
    y_gaze, _ = ops.prepare_gaze(torch.from_numpy(fmap).to(dev), torch.from_numpy(loc).to(dev), h, w)
    rc = m.rnn.cell_list[0].rnn_conv
    cache = WeightCache(torch.device(dev), m._wshared.setdefault(str(torch.device(dev)), {}))
    taps = {train.fuse_block(m)[1]: None}                    # the fusion block's input is read back on request
    out, _ = m(x, cb, None, taps=taps)
    if refresh_only:
        res = {"T": T}
        refresh_phases(res, m, x, cb, y_gaze, iters, repeats)
        return res
    if st_only:
        res = {"T": T}
        st_phases(res, m, x, cb, y_gaze, cache, iters, repeats)
        return res
    if srf_only:
        res = {"T": T}
        srf_phases(res, m, x, cb, y_gaze, cache, iters, repeats)
        return res
    if backbone_only:
        res = {"T": T}
        backbone_phases(res, m, x, cb, y_gaze, cache, iters, repeats)
        return res
    if shallow_only:
        res = {"T": T}
        shallow_phases(res, m, x, cb, y_gaze, cache, iters, repeats)
        return res
    if lstm_only:
        res = {"T": T}
        lstm_phases(res, m, x, cb, y_gaze, iters, repeats)
        return res
    if decoder_bn_only:
        res = {"T": T}
        decoder_bn_phases(res, m, x, cb, y_gaze, cache, iters, repeats)
        return res
    if fuse_bn_only:
        res = {"T": T}
        fuse_bn_phases(res, m, x, cb, y_gaze, cache, iters, repeats)
        return res
    cl = torch.channels_last
    x_seq, h_seq = taps["prefuse"].contiguous(memory_format=cl), taps["rnn"].contiguous(memory_format=cl)
    pred = out.detach().requires_grad_(True)
    g_y = torch.autograd.grad(losses.loss_fu(pred, y_gaze), pred)[0]
    grad_h = train.decoder_input_grad(m.conv_out_st, h_seq, g_y, cache=cache, y=out)
    parts = {}
    train.twa_backward(x_seq, h_seq, None, rc.weight.detach(), grad_h, cache=cache, module=rc, parts=parts)
    dz = parts["dz"]
    xn, hn = x_seq.permute(0, 2, 3, 1), h_seq.permute(0, 2, 3, 1)
    h0n = torch.zeros((1, h, w, 256), device=dev)
    gw = torch.empty_like(rc.weight)

    def refresh(device=False):
        with torch.no_grad():
            rc.weight.mul_(1.0)
        m.refresh_weights(m.rnn, device=device)

    def step():
        rc.weight.grad = None
        train.recurrence_step(m, x, cb, None, y_gaze)

    blk = m.conv_out_st
    dparts = {}
    _, dgrads = train.decoder_backward(blk, h_seq, g_y, cache=cache, y=out, parts=dparts)
    e_, d_, y_, ga_ = (dparts[k] for k in ("e", "d", "y", "ga"))
    pw, pwbn, dwc, dwbn, pl, plbn = train._decoder_parts(blk)
    w9, s2, _ = cache.depthwise(dwc, dwbn)
    _, _, _, w3, s3, _ = cache.dw_dot(dwc, dwbn, pl, plbn)
    s1 = cache.affine(pwbn, 1536)[0]
    rowdot = torch.empty(1536, dtype=torch.float64, device=dev)
    g1 = dgrads[train.DECODER_PARAMS[0]]
    ws, slabs = train.dec_sums(g_y, y_, e_, d_, ga_, w3, s3)
    fin = L.DecFinishDesc()
    fin.ws, fin.ws_bytes, fin.rowdot = ws.data_ptr(), ws.numel() * 8, rowdot.data_ptr()
    fin.wd, fin.w3, fin.s2, fin.s3 = dwc.weight.data_ptr(), pl.weight.data_ptr(), s2.data_ptr(), s3.data_ptr()
    (fin.r1, fin.mu1), (fin.r2, fin.mu2), (fin.r3, fin.mu3) = ((t.data_ptr() for t in cache.bn_stats(b)) for b in (pwbn, dwbn, plbn))
    (fin.g_gamma1, fin.g_beta1, fin.g_wd, fin.g_gamma2, fin.g_beta2, fin.g_w3, fin.g_gamma3, fin.g_beta3) = (
        dgrads[n].data_ptr() for n in train.DECODER_PARAMS[1:])
    fin.C, fin.slabs, fin.accumulate = 1536, slabs, 0
    lib = L.load()
    train.pix_gemm(ga_, hn, out=g1, row_scale=s1, w=pw.weight.detach(), rowdot=rowdot)
    stream = torch.cuda.current_stream().cuda_stream

    def step_dec():
        for q in list(m.rnn.parameters()) + list(blk.parameters()):
            q.grad = None
        train.recurrence_step(m, x, cb, None, y_gaze, decoder=True)

    def refresh_dec(device=False):
        with torch.no_grad():
            rc.weight.mul_(1.0)
            for q in blk.parameters():
                q.mul_(1.0)
        m.refresh_weights(m.rnn, blk, device=device)
    res = {"T": T}
    cases = {"forward": lambda: m(x, cb, None, taps={}),
             "dec_grad": lambda: train.decoder_input_grad(m.conv_out_st, h_seq, g_y, cache=cache, y=out),
             "twa_backward": lambda: train.twa_backward(x_seq, h_seq, None, rc.weight.detach(), grad_h, out=gw, cache=cache, module=rc),
             "wgrad": lambda: train.twa_wgrad(dz, xn, hn, h0n, out=gw),
             "step": step, "refresh": refresh, "refresh_device": lambda: refresh(True),
             "dec_bwd_grad": lambda: train.decoder_backward(blk, h_seq, g_y, cache=cache, y=out, grads=dgrads),
             "dec_bwd_kernel": lambda: train.dec_bwd(g_y, y_, e_, d_, s1, w9, s2, w3, s3),
             "pix_gemm": lambda: train.pix_gemm(ga_, hn, out=g1, row_scale=s1, w=pw.weight.detach(), rowdot=rowdot),
             "dec_sums": lambda: train.dec_sums(g_y, y_, e_, d_, ga_, w3, s3),
             "dec_finish": lambda: L.check(lib.uavsal_dec_finish(C.byref(fin), stream), "uavsal_dec_finish"),
             "refresh_dec": refresh_dec, "refresh_dec_device": lambda: refresh_dec(True)}
    for k, fn in cases.items():
        res[k + "_ms"] = 1e3 * best_of(fn, iters, repeats)
    alt = {"step": [], "step_dec": []}                       # the two steps alternated in the same run
    for _ in range(repeats):
        alt["step"].append(per_call(step, iters))
        alt["step_dec"].append(per_call(step_dec, iters))
    res["step_alt_ms"], res["step_dec_ms"] = 1e3 * min(alt["step"]), 1e3 * min(alt["step_dec"])
    for q in blk.parameters():
        q.grad = None
    pflop = 2.0 * 1536 * 256 * T * h * w
    gd = L.PixGemmDesc()
    gd.K, gd.M, gd.N = T * h * w, 1536, 256
    res["pix_gemm_shares"] = int(lib.uavsal_pix_gemm_shares(C.byref(gd)))
    res["pix_gemm_tflops"] = pflop / (res["pix_gemm_ms"] * 1e-3) / 1e12
    res["pix_gemm_of_peak"] = res["pix_gemm_tflops"] / PEAK_TFLOPS
    nbytes = 3.0 * 1536 * 4 * T * h * w
    res["dec_sums_slabs"] = slabs
    res["dec_sums_gbs"] = nbytes / (res["dec_sums_ms"] * 1e-3) / 1e9
    res["dec_bwd_kernel_gbs"] = nbytes / (res["dec_bwd_kernel_ms"] * 1e-3) / 1e9
    res["bptt_ms"] = res["twa_backward_ms"] - res["wgrad_ms"]
    flop = 2.0 * 256 * 4608 * T * h * w
    res["wgrad_gflop"] = flop / 1e9
    d = L.TwaWgradDesc()
    d.T, d.H, d.W, d.C = T, h, w, 256
    res["wgrad_shares"] = int(L.load().uavsal_twa_wgrad_shares(C.byref(d)))
    res["wgrad_tflops"] = flop / (res["wgrad_ms"] * 1e-3) / 1e12
    res["wgrad_of_peak"] = res["wgrad_tflops"] / PEAK_TFLOPS
    fuse_phases(res, m, x, cb, y_gaze, taps, grad_h, cache, iters, repeats, skip_eager)
    fust_phases(res, m, x, cb, y_gaze, grad_h, cache, iters, repeats)
    ctx_phases(res, m, x, cb, y_gaze, grad_h, cache, iters, repeats)
    nets_phases(res, m, x, cb, y_gaze, cache, iters, repeats)
    st_phases(res, m, x, cb, y_gaze, cache, iters, repeats)
    srf_phases(res, m, x, cb, y_gaze, cache, iters, repeats)
    refresh_phases(res, m, x, cb, y_gaze, iters, repeats)
    backbone_phases(res, m, x, cb, y_gaze, cache, iters, repeats)
    if not skip_eager:
        try:
            run = eager_step(m, taps["prefuse"], torch.zeros((1, 256, h, w), device=dev), g_y)
            ge = run()
            res["eager_fwdbwd_ms"] = 1e3 * best_of(run, max(1, iters // 2), repeats)
            train.twa_wgrad(dz, xn, hn, h0n, out=gw)
            res["eager_vs_hip_grad_rel_l2"] = float((ge - gw).norm() / ge.norm())
        except RuntimeError as e:                     # torch's own conv kernels may not exist for this device
            res["eager_error"] = str(e).splitlines()[0][:200]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-eager", action="store_true")
    ap.add_argument("--refresh-only", action="store_true", help="only the refresh / iteration pairs (refresh_phases)")
    ap.add_argument("--st-only", action="store_true", help="only the phases of the seventh stage (st_phases)")
    ap.add_argument("--srf-only", action="store_true", help="only the phases of the eighth stage (srf_phases)")
    ap.add_argument("--backbone-only", action="store_true", help="only the phases of the ninth stage (backbone_phases)")
    ap.add_argument("--shallow-only", action="store_true", help="only the phases of the tenth stage (shallow_phases)")
    ap.add_argument("--lstm-only", action="store_true", help="only the phases of the ConvLSTM backward (lstm_phases)")
    ap.add_argument("--decoder-bn-only", action="store_true",
                    help="only the phases of the decoder on batch statistics (decoder_bn_phases)")
    ap.add_argument("--fuse-bn-only", action="store_true",
                    help="only the phases of the fusion block on batch statistics (fuse_bn_phases)")
    ap.add_argument("--frames", type=int, nargs="+", default=[20, 5], help="sequence lengths to run (multiples of 5, or of 4)")
    a = ap.parse_args()
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "map": [45, 80],
           "cases": [bench(T, a.iters, a.repeats, dev, a.skip_eager, a.refresh_only, a.st_only, a.srf_only, a.backbone_only, a.shallow_only,
                           a.lstm_only, a.decoder_bn_only, a.fuse_bn_only)
                     for T in a.frames]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
