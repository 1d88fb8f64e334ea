"""Fine-tuning on the device: one step, `recurrence_step`, and behind its keywords the ten stages the reference can train.

The first stage is ONE stage of the reference's `train()` (Demo_Train_Test.py:35-174): the loss gradient is carried through
the frozen decoder `conv_out_st` and back through time to the recurrence's only parameter and to the recurrence's input.
Everything else stays frozen and in eval mode -- a deliberate difference from the reference, whose `train()` also trains
`fust_layer`, the prior nets and the decoder and runs every BatchNorm on batch statistics.  Each further
stage is a keyword of the step; its module tells what it trains, what it needs and what to refresh afterwards:

    stage                        keyword    module          kernels
    1  model.rnn                 (always)   recurrence.py   csrc/train.hip, csrc/train_lstm.hip (`lstm=True`: UAVSAL_LSTM)
    2  model.conv_out_st         decoder    decoder.py      csrc/train_decoder.hip (frozen: csrc/train.hip)
    3  the fusion block          fuse       block.py        csrc/train_block.hip
    4  model.fust_layer[0]       fust       ctx.py          csrc/train_ctx.hip
    5  fucb_layer, cxt_cb_prior  ctx        ctx.py          csrc/train_ctx.hip
    6  gauss / ob prior nets     nets       nets.py         csrc/train_nets.hip
    7  model.st_layer            st         st.py           csrc/train_st.hip
    8  the head of model.sfnet   srf        srf.py          csrc/train_srf.hip
    9  features[8:18]            backbone   backbone.py     csrc/train_block.hip (`tails32`: csrc/train_decoder.hip)
    10 features[2:8]             shallow    backbone.py     csrc/train_shallow.hip

`batch_stats=("decoder",)` runs the decoder's BatchNorms on the statistics of the batch instead (bn.py, decoder.py:
csrc/train_bn.hip), the first stage for which the reference's `model.train()` behaviour exists; every other stage's
BatchNorms stay on their running statistics.  `block_stats=("fuse",)` does the same for the fusion block in FRONT of the
recurrence (block_bn.py: `block_forward_batch` / `block_backward_batch`, `uavsal_bn_apply_res`), whose new output the recurrence
and the decoder then run on again outside the plan (recurrence.py: `twa_forward` / `lstm_forward`):

    keyword                      stage          module          what runs outside the plan
    batch_stats=("decoder",)     conv_out_st    decoder.py      the decoder on the plan's `rnn` tap
    block_stats=("fuse",)        fusion block   block_bn.py     the block on its input tap, the recurrence, the decoder

`STAGES` below is the same list as data: what each keyword needs and which modules it refreshes.  `_common.py` holds what the
stages share.  The imports run one way: block <- ctx <- {nets, st}, st <- srf, block <- backbone; the step combines them here.
Apart from the launches named above everything is one `uavsal_conv_gemm` / `uavsal_dw3x3` call each, routed by the library's
own table, with repacked weights.  Returned gradients are channels-last.  `f32` only; one sequence per call.  CPU tensors
raise: this package has no CPU fallback."""
from typing import Callable, NamedTuple, Optional

import torch

from .. import _lib as _L
from .. import losses as _losses
from ..weights import WeightCache
from ._common import HID, _conv, _param_grad_tensors, conv3_wgrad, pix_gemm, skinny_wgrad  # noqa: F401
from .backbone import (BACKBONE_C4, BACKBONE_END, BACKBONE_FIRST, BACKBONE_PARAMS, SHALLOW_C3, SHALLOW_END,  # noqa: F401
                       SHALLOW_FIRST, SHALLOW_PARAMS, _feature_params, backbone_backward, backbone_blocks, shallow_backward,
                       shallow_blocks)
from .block import (BLOCK_PARAMS, _block_backward, _block_parts, _block_recompute, _input_grad, _input_grad_parts,  # noqa: F401
                    _param_grad_parts, block_backward, block_input_grad, block_param_grads, ir_bwd, ir_bwd_dil, ir_bwd_s2, ir_sums,
                    ir_sums_dil, ir_sums_s2)
from .block_bn import block_backward_batch, block_forward_batch  # noqa: F401
from .ctx import PRIOR_PATH_BLOCKS, bilinear_bwd, fust_output_grad, prior_path_backward, prior_path_blocks, tsum_bwd  # noqa: F401
from . import bn  # noqa: F401
from .bn import bn_apply, bn_bwd_apply, bn_bwd_sums, bn_stats, dw_wgrad  # noqa: F401
from .decoder import (DECODER_PARAMS, _decoder_parts, _decoder_recompute, dec_bwd, dec_sums, decoder_backward, decoder_backward_batch,  # noqa: F401
                      decoder_forward_batch, decoder_input_grad, decoder_param_grads)
from .nets import (PRIOR_NETS, _narrow_parts, frame_sum, ir_narrow_grads, narrow_block_param_grads, prior_net_backward,  # noqa: F401
                   prior_nets)
from .recurrence import (lstm_backward, lstm_forward, lstm_gate_bwd, lstm_scan, twa_backward, twa_forward, twa_gate_bwd,  # noqa: F401
                         twa_wgrad)
from .srf import SRF_HEAD, SRF_HEAD_BLOCKS, SRF_HEAD_PARAMS, conv3_backward, srf_head, srf_head_backward  # noqa: F401
from .st import (ST_BLOCK_PARAMS, ST_BLOCK_PARTS, ST_CBR_PARAMS, _cbr_backward, cbr_backward, cbr_sums, st_block_backward,  # noqa: F401
                 tdiff_bwd)


def fuse_block(model):
    """The block that produces the recurrence's input (the `prefuse` tap), and the name of the tap that holds ITS input:
    `model.fucbst_layer[0]` reading `fu320` with any prior enabled, else `model.fust_layer[0]` reading the last ST block's
    output."""
    if model.num_cb:
        return model.fucbst_layer[0], "fu320"
    return model.fust_layer[0], "st%d" % (len(model.st_layer) - 1)


class Stage(NamedTuple):
    """One row of `STAGES`.  `needs(on, model)`: what the stage asks of the other keywords (`on`: `{keyword: truthy}`) --
    `stream.finetune_video` refuses a `stages` tuple that does not meet it; `model_needs(model)`: what it asks of the model
    besides, which only the step checks; `refusal`: what `recurrence_step` raises when either is not met; `modules(model)`:
    what to hand to `model.refresh_weights` after an optimiser step."""
    keyword: str
    needs: Optional[Callable]
    model_needs: Optional[Callable]
    refusal: Optional[str]
    modules: Callable


# The ten stages in the order `finetune_video(stages=...)` names them, which is the order their modules are refreshed in.
STAGES = (
    Stage("rnn", None, None, None, lambda m: [m.rnn]),
    Stage("decoder", None, None, None, lambda m: [m.conv_out_st]),
    Stage("fuse", None, None, None, lambda m: [m.fucbst_layer if m.num_cb else m.fust_layer]),
    Stage("fust", lambda on, m: on.get("fuse"), lambda m: getattr(m, "num_cb", 0),
          "fust=True needs fuse=True and a model with at least one prior (without priors the fuse stage "
          "already is model.fust_layer[0])", lambda m: [m.fust_layer]),
    Stage("ctx", lambda on, m: on.get("fuse"), lambda m: getattr(m, "num_cb", 0),
          "ctx=True needs fuse=True and a model with at least one prior (without priors there is no "
          "multi-prior path)",
          lambda m: [m.fucb_layer] + ([m.cxt_cb_prior] if getattr(m, "use_context_prior", False) else [])),
    Stage("nets", lambda on, m: on.get("fuse"), prior_nets,
          "nets=True needs fuse=True and a model with the gauss or the ob prior (bias_type [0,0,1] and [0,0,0] "
          "have no prior net)", lambda m: list(prior_nets(m).values())),
    Stage("st", lambda on, m: on.get("fuse") and (on.get("fust") or not getattr(m, "num_cb", 0)), None,
          "st=True needs fuse=True, and in a model with priors fust=True as well (the gradient reaches "
          "model.st_layer through model.fust_layer[0]'s input)", lambda m: [m.st_layer]),
    Stage("srf", lambda on, m: on.get("st"), None,
          "srf=True needs st=True (and what st needs): the gradient reaches model.sfnet's head through the "
          "input of model.st_layer[0]", srf_head),
    Stage("backbone", lambda on, m: on.get("srf"), None,
          "backbone=True needs srf=True (and what srf needs): the gradient reaches the backbone blocks through "
          "the c4 / c5 taps of model.sfnet's head", backbone_blocks),
    Stage("shallow", lambda on, m: on.get("backbone"), None,
          "shallow=True needs backbone=True (and what backbone needs): the gradient reaches the shallow blocks "
          "through the c3 tap of model.sfnet's head and the input of features[8]", shallow_blocks),
)


BATCH_STATS = ("decoder",)       # the stages whose BatchNorms `recurrence_step(batch_stats=...)` can run on batch statistics
BLOCK_STATS = ("fuse",)          # the stages in FRONT of the recurrence that `recurrence_step(block_stats=...)` can run that way


def fuse_container(model):
    """The module that holds `fuse_block(model)`'s block: what `.train()` is called on for `block_stats=("fuse",)` and what
    `model.refresh_weights` takes afterwards."""
    return model.fucbst_layer if model.num_cb else model.fust_layer


def _names(value):
    return (value,) if isinstance(value, str) else tuple(value)


def stages_allowed(model, stages):
    """Whether `stages` is a tuple `stream.finetune_video` trains: `"rnn"` first, then names of `STAGES` in its order, none
    twice, each with what it `needs`."""
    if tuple(stages[:1]) != ("rnn",) or list(stages) != [s.keyword for s in STAGES if s.keyword in stages]:
        return False
    on = dict.fromkeys(stages, True)
    return all(s.needs is None or s.needs(on, model) for s in STAGES if s.keyword in on)


def stage_modules(model, on):
    """The modules to refresh after an optimiser step over the stages whose keywords are in `on`, `model.rnn` first."""
    return [m for s in STAGES if s.keyword == "rnn" or s.keyword in on for m in s.modules(model)]


def _grads_of(module):
    return _param_grad_tensors(dict(module.named_parameters()))


def recurrence_step(model, x, cb, in_state, y_gaze, criterion=None, decoder=False, fuse=False, fust=False, ctx=False, nets=False,
                    st=False, srf=False, backbone=False, shallow=False, lstm=False, batch_stats=(), block_stats=()):
    """One training step's forward and backward for the recurrence: `model(x, cb, in_state)` through the launch plan, the
    criterion (default `losses.loss_fu`) and its gradient, the decoder's input gradient and `twa_backward`.  Ends with
    `model.rnn.cell_list[0].rnn_conv.weight.grad` set -- or added to when it already exists, as `loss.backward()` would --
    and no other parameter touched.  Returns `(loss, out, [h_last.detach()])`, the forward's contract plus the loss.
    The model is in eval mode (every other stage is frozen, its BatchNorms folded); a model in training mode, CPU tensors,
    a precision other than 'f32' or -- without `lstm=True` -- `UAVSAL_LSTM` raise.  After `optimizer.step()` call
    `model.refresh_weights(model.rnn)`.
    `decoder`, `fuse`, `fust`, `ctx`, `nets`, `st`, `srf`, `backbone`, `shallow`: the stage of that keyword in `STAGES` is
    trained as well -- the `.grad` of its parameters set, or added to; the BatchNorms still use their running statistics.
    Each stage's module says what it needs and what to refresh; a keyword without what it needs raises the stage's `refusal`
    before any launch.  The stages combine freely within those rules; a call without a keyword runs the launches -- and the
    copies of taps -- it always ran.
    `lstm=True` (opt-in, for a `UAVSAL_LSTM` model, the reference's ConvLSTM ablation; with a ConvTWA model it raises before
    any launch): `in_state` is None or `[(h, c)]`, the forward runs through the plan as it always did, and `lstm_backward`
    stands where `twa_backward` stands, setting -- or adding to -- the `.grad` of the `[1024,512,3,3]` `rnn_conv.weight`; every
    other keyword works unchanged behind it.  Returns `(loss, out, [h_last.detach(), c_last.detach()])`, the forward's
    contract for this model; refresh `model.rnn` as usual.  Without the keyword a `UAVSAL_LSTM` model raises, as it always did.
    `batch_stats=("decoder",)` (opt-in; the default `()` runs the launches it ran and returns the bits it returned; needs
    `decoder=True`): the decoder runs as the reference's `train()` runs it, its BatchNorms on the statistics of the batch
    (`BATCH_STATS`).  The model stays in eval mode and `model.conv_out_st.train()` has been called -- a configuration torch
    itself defines; anything else raises a `RuntimeError` that names what is missing, before any launch, and any other stage
    name in the tuple a `NotImplementedError` that names it.  The plan runs as always (a child in training mode changes
    nothing in it: the plan and the weight cache read the running statistics where they lie), its own prediction is dropped,
    and `out` and the loss come from `decoder_forward_batch` on the `rnn` tap, which also moves the decoder's running
    statistics; `decoder_backward_batch` sets -- or adds to -- the nine `.grad`s and hands its `grad_h` to the recurrence
    unchanged.  The returned `out` is the batch-statistics prediction.  Afterwards
    `model.refresh_weights(model.rnn, model.conv_out_st)` refolds the eval-mode packed forms from the moved statistics.
    `block_stats=("fuse",)` (opt-in, a keyword of its own because it names a stage in FRONT of the recurrence; the default `()`
    runs the launches it ran and returns the bits it returned; needs `fuse=True`; combines freely with `batch_stats`): the
    fusion block `fuse_block(model)` runs as the reference's `train()` runs it (`BLOCK_STATS`).  The model stays in eval mode
    and the block's container (`fuse_container(model)`: `model.fucbst_layer`, or `model.fust_layer` without priors) has been
    put into `.train()`; anything else raises a `RuntimeError` that names what is missing, before any launch, and any other
    name in the tuple a `NotImplementedError` that names it.  The plan runs as always and delivers the block's input tap;
    `block_forward_batch` gives the new `prefuse` and moves the block's running statistics; `twa_forward` (`lstm=True`:
    `lstm_forward`) gives the new history and state from it; the decoder runs on that history, in eval mode by the forward's
    own launches or, under `batch_stats=("decoder",)`, through `decoder_forward_batch`.  The plan's own `prefuse`, `rnn`,
    prediction and state are dropped: `out`, the loss and the returned state are the rerun's.  The backward runs as always on
    the new tensors, `block_backward_batch` standing where `block_backward` stands; the `grad_x` it returns feeds the stages
    behind it (`fust`, `ctx`, `nets`, `st`, ...) unchanged -- they stay in eval mode.  Afterwards
    `model.refresh_weights(model.rnn, fuse_container(model))` refolds the block's eval-mode packed forms."""
    batch_stats, block_stats = _names(batch_stats), _names(block_stats)
    for name in block_stats:
        if name not in BLOCK_STATS:
            raise NotImplementedError("block_stats covers %r only; the BatchNorms of stage %r stay on their running statistics"
                                      % (BLOCK_STATS, name))
    for name in batch_stats:
        if name not in BATCH_STATS:
            raise NotImplementedError("batch_stats covers %r only; the BatchNorms of stage %r stay on their running statistics"
                                      % (BATCH_STATS, name))
    criterion = criterion or _losses.loss_fu
    is_lstm = getattr(model, "rnn_type", "twa") != "twa"
    if is_lstm and not lstm:
        raise RuntimeError("recurrence_step covers the ConvTWA recurrence, not UAVSAL_LSTM")
    if lstm and not is_lstm:
        raise RuntimeError("lstm=True is for a UAVSAL_LSTM model (the ConvLSTM recurrence); this model's recurrence is ConvTWA")
    on = dict(decoder=decoder, fuse=fuse, fust=fust, ctx=ctx, nets=nets, st=st, srf=srf, backbone=backbone, shallow=shallow)
    for s in STAGES:
        if on.get(s.keyword) and s.needs and not (s.needs(on, model) and (s.model_needs is None or s.model_needs(model))):
            raise RuntimeError(s.refusal)
    if model.training:
        raise RuntimeError("recurrence_step needs model.eval(): only the recurrence is trained, every BatchNorm stays folded")
    if model.precision != "f32":
        raise RuntimeError("recurrence_step supports precision 'f32' only, got %r" % (model.precision,))
    if batch_stats:
        if not decoder:
            raise RuntimeError("batch_stats=('decoder',) needs decoder=True: the batch statistics belong to the trained decoder")
        if not model.conv_out_st.training:
            raise RuntimeError("batch_stats=('decoder',) needs model.conv_out_st.train() (under model.eval()): the decoder's "
                               "BatchNorms are in eval mode")
    if block_stats:
        if not fuse:
            raise RuntimeError("block_stats=('fuse',) needs fuse=True: the batch statistics belong to the trained fusion block")
        box = fuse_container(model)
        if not box.training or not fuse_block(model)[0].training:
            raise RuntimeError("block_stats=('fuse',) needs model.%s.train() (under model.eval()): the fusion block's BatchNorms "
                               "are in eval mode" % ("fucbst_layer" if model.num_cb else "fust_layer"))
    if not torch.is_tensor(x) or not x.is_cuda or not torch.is_tensor(y_gaze) or not y_gaze.is_cuda:
        raise RuntimeError("recurrence_step needs tensors on the MI355X (cuda) device; there is no CPU fallback")
    rc = model.rnn.cell_list[0].rnn_conv
    blk, src = fuse_block(model) if fuse else (None, None)
    taps = {src: None} if fuse else {}                               # (fu320 is read back on request only: engine.TAPS_ON_REQUEST)
    if fust or ctx or nets:
        taps["cb192"] = None                                         # (likewise)
    out, h_last = model(x, cb, in_state, taps=taps)
    dev = x.device
    cache = WeightCache(dev, model._wshared.setdefault(str(torch.device(dev)), {}))
    cl = torch.channels_last
    h0 = None if in_state is None else in_state[0]
    if lstm:
        h0, c0 = (None, None) if h0 is None else h0
    if block_stats:                                                  # the plan's own prefuse, rnn, prediction and state are dropped
        fu = taps[src].contiguous(memory_format=cl)
        x_seq, blk_saved = block_forward_batch(blk, fu, cache=cache)
        if lstm:
            h_seq, c_last = lstm_forward(x_seq, h0, c0, rc.weight.detach(), cache=cache, module=rc)
            h_last = [h_seq[-1:].contiguous(), c_last.contiguous()]
        else:
            h_seq = twa_forward(x_seq, h0, rc.weight.detach(), cache=cache, module=rc)
            h_last = [h_seq[-1:].contiguous()]
        if not batch_stats:                                          # the eval-mode decoder by the forward's own launches
            y = _decoder_recompute(_L.load(), cache, model.conv_out_st, h_seq.permute(0, 2, 3, 1), None)[2]
            out = y.view(y.shape[0], 1, y.shape[1], y.shape[2])
    else:
        h_seq, x_seq = taps["rnn"].contiguous(memory_format=cl), taps["prefuse"].contiguous(memory_format=cl)
    if batch_stats:                                                  # the plan's own prediction is dropped
        out, saved = decoder_forward_batch(model.conv_out_st, h_seq, cache=cache)
    pred = out.detach().requires_grad_(True)
    with torch.enable_grad():
        loss = criterion(pred, y_gaze)
        (g_y,) = torch.autograd.grad(loss, pred)
    if decoder and batch_stats:
        grads, acc = _grads_of(model.conv_out_st)
        grad_h, _ = decoder_backward_batch(model.conv_out_st, h_seq, g_y, saved=saved, grads=grads, accumulate=acc, cache=cache)
    elif decoder:
        grads, acc = _grads_of(model.conv_out_st)
        grad_h, _ = decoder_backward(model.conv_out_st, h_seq, g_y, cache=cache, y=out, grads=grads, accumulate=acc)
    else:
        grad_h = decoder_input_grad(model.conv_out_st, h_seq, g_y, cache=cache, y=out)
    w = rc.weight
    had = w.grad is not None
    if not had:
        w.grad = torch.empty_like(w, memory_format=torch.contiguous_format)
    if lstm:
        _, grad_x, _, _ = lstm_backward(x_seq, h_seq, h0, c0, w.detach(), grad_h, need_x_grad=bool(fuse), out=w.grad,
                                        accumulate=had, cache=cache, module=rc)
    else:
        _, grad_x, _ = twa_backward(x_seq, h_seq, h0, w.detach(), grad_h, need_x_grad=bool(fuse), out=w.grad, accumulate=had,
                                    cache=cache, module=rc)
    if fuse:
        grads, acc = _grads_of(blk)
        if block_stats:
            grad_fu, _ = block_backward_batch(blk, fu, grad_x, saved=blk_saved, need_x_grad=bool(fust or ctx or nets or st),
                                              cache=cache, grads=grads, accumulate=acc)
        else:
            fu = taps[src].contiguous(memory_format=cl)
            grad_fu, _ = block_backward(blk, fu, grad_x, need_x_grad=bool(fust or ctx or nets or st), cache=cache, grads=grads,
                                        accumulate=acc)
        g_cb, g_st = None, grad_fu                                   # (without priors the fuse stage IS fust_layer[0])
        if ctx:
            pg = {n: _grads_of(b) for n, b in prior_path_blocks(model).items()}
            g, _, *g_cb = prior_path_backward(model, fu, taps["cb192"], grad_fu, cache=cache, grads={n: v[0] for n, v in pg.items()},
                                              accumulate={n: v[1] for n, v in pg.items()}, need_fust_grad=bool(fust),
                                              need_cb_grad=bool(nets))
        elif nets:
            g, _, *g_cb = prior_path_backward(model, fu, taps["cb192"], grad_fu, cache=cache, need_fust_grad=bool(fust),
                                              need_cb_grad=True)
        elif fust:
            g = fust_output_grad(model, fu, taps["cb192"], grad_fu, cache=cache)
        if nets:
            (g_cb,) = g_cb
            cbs = dict(zip(PRIOR_NETS, model._used_cb(cb)))
            static = bool(model.dedupe_priors and x.shape[0] > 1 and model._static(*model._used_cb(cb), 1))
            for i, (name, net) in enumerate(prior_nets(model).items()):
                go, c = g_cb[..., 64 * i:64 * i + 64], cbs[name]
                if static:                                           # the net ran on ONE frame that every frame reads
                    go, c = frame_sum(go), c[:1]
                pg = {k: _grads_of(b) for k, b in zip("01", net)}
                prior_net_backward(net, c, go, cache=cache, grads={k: v[0] for k, v in pg.items()},
                                   accumulate={k: v[1] for k, v in pg.items()})
        if fust:
            fb = model.fust_layer[0]
            grads, acc = _grads_of(fb)
            g_st, _ = block_backward(fb, taps["st%d" % (len(model.st_layer) - 1)].contiguous(memory_format=cl), g,
                                     need_x_grad=bool(st), cache=cache, grads=grads, accumulate=acc)
        if st:
            for i in range(len(model.st_layer) - 1, -1, -1):         # one sequence of all frames, as forward() runs them
                grads, acc = _grads_of(model.st_layer[i])
                xin = taps["st%d" % (i - 1)] if i else taps["sfnet"]
                g_st, _ = st_block_backward(model.st_layer[i], xin.contiguous(memory_format=cl), g_st, seq_len=x.shape[0],
                                            need_x_grad=i > 0 or bool(srf), cache=cache, grads=grads, accumulate=acc)
        if srf:
            hp = dict(model.sfnet.named_parameters())
            grads, acc = _param_grad_tensors({n: hp[n] for n in SRF_HEAD_PARAMS})
            ret = srf_head_backward(model.sfnet, taps["c3"], taps["c4"], taps["c5"], taps["sfnet"], g_st, cache=cache,
                                    grads=grads, accumulate=acc, need_tap_grads=bool(backbone),
                                    **({"need_c3_grad": True} if shallow else {}))
        if backbone:
            feats = model.sfnet.features.features
            grads, acc = _param_grad_tensors(_feature_params(feats, BACKBONE_FIRST, BACKBONE_END))
            bret = backbone_backward(feats, taps["c3"], ret[1], ret[2], cache=cache, grads=grads, accumulate=acc,
                                     **({"need_x_grad": True} if shallow else {}))
        if shallow:
            grads, acc = _param_grad_tensors(_feature_params(feats, SHALLOW_FIRST, SHALLOW_END))
            shallow_backward(feats, x, ret[3], bret[1], cache=cache, grads=grads, accumulate=acc)
    return loss.detach(), out, [t.detach() for t in h_last]
