"""Video-level driver: the loop of the reference's `test()` (Demo_Test.py:65-95) with frames,
recurrent state and outputs kept on the device.  The reference decodes a video with cv2,
normalises each group of `batch_size * time_dims` frames on the host, copies it to the GPU, runs
`model(x, cb, state)`, copies the maps back and resizes them one by one with cv2.  Here the
caller hands over the uint8 RGB frames as a tensor (decoding is out of scope: no video codec in
this image); normalisation happens inside the stem kernel, the state never leaves HBM, and the
maps are resized / normalised / quantised by `uavsal_postprocess`.  With `model_size` the frames are
the decoder's source-size ones and `uavsal_letterbox_u8` letterboxes them on the device first
(preprocess_videos / padding, utils_data.py:255-287, 321-343)."""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import matio, ops


def save_salmap(path: str, sal_u8: torch.Tensor, save_frames: Optional[int] = None) -> None:
    """The result file of the reference's loop (Demo_Test.py:92-95): `salmap` uint8 `[H, W, 1, F]` as MATLAB v7.3, the
    first `save_frames` frames (`saveFrames`, Demo_Test.py:92).  `sal_u8`: uint8 `[F, H, W]` (what `predict_video` returns)."""
    a = sal_u8.detach().cpu().numpy()
    if a.dtype.name != "uint8" or a.ndim != 3:
        raise ValueError("save_salmap takes the uint8 [F, H, W] maps of predict_video")
    if save_frames is not None:
        a = a[:max(0, int(save_frames))]
    matio.savemat(path, {"salmap": a[:, :, :, None].transpose(1, 2, 3, 0)})


def _host_streams(dev, n):
    """`n` host streams that really run side by side.  The HIP runtime multiplexes the streams of one priority onto
    GPU_MAX_HW_QUEUES (default 4) hardware queues, a stream taking the least used one when it is created; two streams on one
    queue execute strictly in submission order.  With the plans' lane streams and torch's pool around, two ordinary streams can
    end up on one queue, and the overlap is gone without a word (measured: 2077 frames/s -> 1851, below the 1888 of the plain
    loop; profiles/r5_experiments.md).  High-priority streams draw from a queue pool of their own, which nothing else in this
    package uses; consecutive ones get different queues."""
    return [torch.cuda.Stream(dev, priority=-1) for _ in range(n)]


_CACHE_KEYS = ("_stream_replicas", "_stream_streams", "_stream_copy")


class _Groups:
    """The groups of a video as device tensors.  Frames already on the device are sliced; frames in host memory (what a decoder
    hands over, Demo_Test.py:78-85) are uploaded group by group on a copy stream of their own, `ahead` groups in front of the
    one being launched, so that the copy of group k + 1 runs under the launches of group k instead of in front of the whole
    video (pinned memory: asynchronous; pageable memory: the host thread stages it, the GPU keeps computing).
    `letterbox=(R, C, layout, bgr)`: the frames are source-size (Demo_Test.py:72-74 hands them to preprocess_videos); each group
    is letterboxed to `R x C` by one `ops.letterbox_frames` launch on the copy stream -- behind its upload for host frames -- so
    that the launch runs under the previous groups instead of between two of them on a compute stream.  A group's source-size
    staging buffer goes back to the allocator as soon as that launch is enqueued: it was allocated, written and read on the copy
    stream only, whose order protects its reuse."""

    def __init__(self, model, frames_u8, group, steps, dev, ahead=2, letterbox=None):
        self.frames, self.group, self.steps, self.dev, self.ahead = frames_u8, group, steps, dev, ahead
        self.host = not frames_u8.is_cuda
        self.letterbox = letterbox
        self.side = self.host or letterbox is not None
        self.pending = {}
        if self.side:
            cs = model.__dict__.get("_stream_copy")
            if cs is None or cs.device != torch.device(dev):
                cs = model.__dict__["_stream_copy"] = _host_streams(dev, 1)[0]
            self.copy_stream = cs
            if not self.host:
                cs.wait_stream(torch.cuda.current_stream(dev))      # device frames were produced on the caller's stream

    def _fetch(self, i):
        if i < self.steps and i not in self.pending:
            with torch.cuda.stream(self.copy_stream):
                t = self.frames[i * self.group:(i + 1) * self.group]
                if self.host:
                    t = t.to(self.dev, non_blocking=True)
                if self.letterbox is not None:
                    R, C, layout, bgr = self.letterbox
                    t = ops.letterbox_frames(t, R, C, layout=layout, bgr=bgr)
                ev = torch.cuda.Event()
                ev.record(self.copy_stream)
            self.pending[i] = (t, ev)

    def get(self, i, stream=None):
        """Group `i`, ready on `stream` (default: the current one)."""
        if not self.side:
            return self.frames[i * self.group:(i + 1) * self.group]
        for k in range(i, i + 1 + self.ahead):
            self._fetch(k)
        t, ev = self.pending.pop(i)
        stream = stream or torch.cuda.current_stream(self.dev)
        stream.wait_event(ev)
        t.record_stream(stream)
        return t


def _inflight_replicas(model, n):
    """`n` handles on `model`'s weights for forwards that overlap on the GPU, cached on the model.  They run WITHOUT lanes: a
    plan's lanes are worth +0.8 % by themselves (fp32, one clip), but with two plans in flight their five streams each compete
    with the host streams for four hardware queues, and the overlap varies between 1884 and 2059 frames/s with the order things
    were created in; lane-less plans give 2075-2087 in every order (profiles/r5_experiments.md).  Same kernels, same order per
    buffer: the maps do not change."""
    model._check_weights()                    # (the model itself may never run: its handles must not inherit stale weights)
    reps = model.__dict__.get("_stream_replicas") or []
    while len(reps) < n:
        reps.append(model.replica())
    for rep in reps:
        engines = rep._engines if rep.__dict__.get("_wshared") is model.__dict__.get("_wshared") else None
        rep.__dict__.update({k: v for k, v in model.__dict__.items() if k not in _CACHE_KEYS})
        rep._engines = engines if engines is not None else type(model._engines)()
        rep.use_lanes = False
        for k in _CACHE_KEYS:
            rep.__dict__.pop(k, None)
    model.__dict__["_stream_replicas"] = reps
    return reps[:n]


@torch.no_grad()
def _predict_overlapped(model, groups, gauss_prior, ob_prior, steps, dev):
    """The groups of ONE video two deep in flight: group k runs on replica k % 2 and host stream k % 2; everything in front of
    the recurrence -- backbone, SRF-Net, ST blocks, prior fusion, the hoisted half of the gate convolution: 3.5 of a group's 4.2 ms
    at 8 frames -- does not depend on the previous group and is launched at once; the recurrence waits for the previous group's
    last launch and takes over its state (`Engine.run_streamed`).  The maps are those of the sequential loop, bit for bit."""
    # the two handles are kept on the model between videos (their launch plans cost ~50 ms to build); they follow the model's
    # current settings, and lose their plans when the model's packed weights were dropped (load_state_dict, in-place edits)
    models = _inflight_replicas(model, 2)
    streams = model.__dict__.get("_stream_streams")
    if streams is None or streams[0].device != torch.device(dev):
        streams = model.__dict__["_stream_streams"] = _host_streams(dev, 2)
    caller = torch.cuda.current_stream(dev)
    maps, prev_eng, prev_done = [], None, None
    for s_ in streams:
        s_.wait_stream(caller)                    # the frames / priors were produced on the caller's stream
    for i in range(steps):
        m_, s_ = models[i % 2], streams[i % 2]
        x = groups.get(i, s_)
        n = x.shape[0]
        with torch.cuda.stream(s_):
            cb = [gauss_prior.unsqueeze(0).expand(n, -1, -1, -1), ob_prior.unsqueeze(0).expand(n, -1, -1, -1)]
            cb0, cb1 = m_._used_cb(cb)
            static = m_.dedupe_priors and m_._static(cb0, cb1, 1)
            eng = m_._engine(dev, 1, n, x.shape[2], x.shape[3], "tile", False, x.dtype, static_priors=static)
            m_._check_cb(cb0, cb1, n, eng.h, eng.w)
            out = eng.run_streamed(x, cb0, cb1, prev=prev_eng, prev_done=prev_done, reset=(i == 0))
            prev_done = torch.cuda.Event()
            prev_done.record(s_)
            prev_eng = eng
            out.record_stream(caller)             # read on the caller's stream below
            maps.append(out.view(n, 1, eng.h, eng.w))
    for s_ in streams:
        caller.wait_stream(s_)
    for m_ in models:
        m_.check_errors()
    lstm = getattr(model, "rnn_type", "twa") == "lstm"
    return maps, ([(prev_eng.h_view, prev_eng.c_view)] if lstm else [prev_eng.h_view])


@torch.no_grad()
def predict_video(model, frames_u8: torch.Tensor, gauss_prior: torch.Tensor, ob_prior: torch.Tensor,
                  batch_size: int = 4, out_size: Optional[tuple] = None, return_maps: bool = False,
                  persistent_state: bool = True, out_path: Optional[str] = None, save_frames: Optional[int] = None,
                  overlap: Optional[bool] = None, model_size: Optional[tuple] = None, frame_layout: str = "CHW",
                  bgr: bool = False, overlay=None):
    """`frames_u8` uint8 `[F,3,H,W]` RGB (already letterboxed to the model size, as
    preprocess_videos does, utils_data.py:255-287) on the device, or in host memory (pinned for asynchronous copies): host
    frames are uploaded group by group on a copy stream, two groups ahead of the launches (`_Groups`), `gauss_prior` `[8,h,w]`, `ob_prior` `[20,h,w]`
    float32 (one map set, repeated per frame like get_bias, Demo_Test.py:14-27).
    `model_size=(R, C)`: `frames_u8` are the decoded SOURCE-size frames instead -- `[F,3,H0,W0]`, or `[F,H0,W0,3]` with
    `frame_layout="HWC"` (what cv2's `VideoCapture` yields; `bgr=True` for its channel order) -- and each group is letterboxed to
    `R x C` on the device before it reaches the model (`ops.letterbox_frames`: `padding()` and the channel swap of
    preprocess_videos, utils_data.py:269-270, 321-343; cv2's 8-bit INTER_LINEAR rule restated, not checked against cv2 itself);
    `out_size` then defaults to `(H0, W0)`, the reference's loop (Demo_Test.py:65-91).  Device and host frames both work; the
    letterbox launch of a group runs on the copy stream, behind the group's upload and ahead of the model's launches.  With
    `model_size=None` (default) `frame_layout` and `bgr` must be left alone and nothing changes.
    Frames beyond the last full `time_dims` chunk are dropped (Demo_Test.py:68-70); groups of
    `batch_size * time_dims` frames are pushed through `model.forward` with the state carried
    (Demo_Test.py:75-86).  Returns uint8 `[F', H_out, W_out]` on the device (the reference's
    `pred_mat[..., 0]`), and the raw maps if asked; with `out_path` the maps are also written as the reference's
    `salmap` `[H,W,1,F]` v7.3 .mat file (Demo_Test.py:93-95).
    `overlap`: consecutive groups two deep in flight on two replicas -- only the recurrence of a group waits for the previous
    group (`_predict_overlapped`); same maps, bit for bit, 1833 -> 2006 frames/s on a 192-frame video at 360x640 in groups of 8.
    None (default): whenever it applies -- resident state, launch-loop plans, at least two whole groups (a shorter last group
    follows them on its own plan, taking over the state); True: insist (raises where it does not apply); False: the reference's
    one-after-the-other loop.
    `overlay`: True, or a dict of `fix=` (the video's `fixLoc` maps `[F,Hf,Wf]`, drawn when given), `colormap=`, `sink=`,
    `group=`, `host=` (see `vis.visual_video`), with `model_size`: the source frames and the fresh maps go through
    `vis.visual_video` on the device -- the reference driver's third call, `visual_vid(..., with_color=1)`
    (Demo_Test.py:130); device frames are read in place, host frames are uploaded a second time, group by group (the
    source-size staging of the forward is gone by then) -- and the overlay frames `[F', out_h, out_w, 3]` (None with a sink) are returned as the last
    element beside the maps.  They carry the channel order of the source frames: for RGB frames (`bgr=False`) the colour
    table, which is BGR, is flipped.  None (default): nothing changes."""
    dev = next(model.parameters()).device
    T = model.time_dims
    F = frames_u8.shape[0]
    count_bs = F // T
    keep = count_bs * T
    if keep < 2:
        raise RuntimeError("need at least one full chunk of time_dims >= 2 frames")
    frames_u8 = frames_u8[:keep]
    if frames_u8.is_cuda and frames_u8.device != torch.device(dev):
        frames_u8 = frames_u8.to(dev)
    letterbox = None
    if model_size is None:
        if frame_layout != "CHW" or bgr:
            raise RuntimeError("frame_layout / bgr describe source-size frames: pass model_size=(R, C) with them")
        H, W = frames_u8.shape[2:]
    else:
        if frame_layout not in ("CHW", "HWC") or frames_u8.dim() != 4 or frames_u8.dtype != torch.uint8:
            raise RuntimeError("model_size needs uint8 frames [F,3,H0,W0] (frame_layout='CHW') or [F,H0,W0,3] ('HWC')")
        H, W = (frames_u8.shape[2:] if frame_layout == "CHW" else frames_u8.shape[1:3])      # the source size
        if frames_u8.shape[1 if frame_layout == "CHW" else 3] != 3:
            raise RuntimeError("expected 3 channels, got %s frames of shape %r" % (frame_layout, tuple(frames_u8.shape)))
        R, C = int(model_size[0]), int(model_size[1])
        ops.letterbox_geometry(H, W, R, C)                # a degenerate picture raises here, before anything is launched
        letterbox = (R, C, frame_layout, bool(bgr))
    if overlay is not None and overlay is not False and model_size is None:
        raise RuntimeError("overlay needs the source-size frames: pass model_size=(R, C) with it")
    out_size = out_size or (H, W)
    group = batch_size * T
    steps = math.ceil(count_bs / batch_size)
    state = None
    maps = []
    was = model.persistent_state
    model.persistent_state = bool(persistent_state)
    try:
        whole = frames_u8.shape[0] // group              # a shorter last group runs on a plan of its own, after the others
        applies = bool(persistent_state) and not model.use_graph and whole >= 2
        if overlap is None:
            overlap = applies
        if overlap and not applies:
            raise RuntimeError("overlap=True needs persistent_state=True, the launch-loop plan and at least two whole groups of "
                               "batch_size * time_dims frames")
        groups = _Groups(model, frames_u8, group, steps, dev, letterbox=letterbox)
        first = 0
        # on the device once, not per group: the groups then hand over views of the SAME tensors, which the model's prior
        # cache recognises (model.cache_priors: the prior nets run once per video and plan)
        gauss_prior, ob_prior = gauss_prior.to(dev), ob_prior.to(dev)
        if overlap:
            maps, state = _predict_overlapped(model, groups, gauss_prior, ob_prior, whole, dev)
            first = whole
        for i in range(first, steps):
            x = groups.get(i)
            n = x.shape[0]
            # one map set for every frame, handed over as a zero-stride view: the model runs its prior nets once per call
            # (model.dedupe_priors) instead of once per frame
            cb = [gauss_prior.unsqueeze(0).expand(n, -1, -1, -1), ob_prior.unsqueeze(0).expand(n, -1, -1, -1)]
            out, st = model(x, cb, state)
            # persistent mode: st[0] is a view of the engine's state buffer (valid until the next call, which
            # recognises it by address); a shorter last group runs on another plan, which loads it as a tensor
            # (the ConvLSTM variant carries (h, c): reference model_convlstm.py:204)
            state = [(st[0].detach(), st[1].detach())] if getattr(model, "rnn_type", "twa") == "lstm" else [st[0].detach()]
            maps.append(out)
    finally:
        model.persistent_state = was
    maps = torch.cat(maps, 0)
    sal = ops.postprocess_predictions(maps, out_size[0], out_size[1])
    if out_path is not None:
        save_salmap(out_path, sal, save_frames)
    if overlay is not None and overlay is not False:
        from . import vis
        kw = dict(overlay) if isinstance(overlay, dict) else {}
        unknown = set(kw) - {"fix", "colormap", "sink", "group", "host"}
        if unknown:
            raise RuntimeError("overlay: unknown keys %r" % sorted(unknown))
        cmap = kw.pop("colormap", None)
        if not bgr:
            cmap = vis.JET_BGR if cmap is None else cmap
            cmap = torch.as_tensor(cmap.copy() if hasattr(cmap, "copy") else cmap).reshape(256, 3).flip(1)
        fix = kw.pop("fix", None)
        over = vis.visual_video(frames_u8, sal, fix=fix, with_fix=fix is not None, layout=frame_layout, colormap=cmap, **kw)
        return (sal, maps, over) if return_maps else (sal, over)
    return (sal, maps) if return_maps else sal


def validation_groups(n_frames, time_dims, batch_size, has_gaze):
    """The groups of the reference's loop over one video (Demo_Train_Test.py:111-126) as `[(first, last, run), ...]`: the
    video is cut to `(n_frames // time_dims) * time_dims` frames, a group is `batch_size * time_dims` frames (the last one
    may be shorter), and a group runs only if every frame of it has a non-zero fixation map AND a fixation
    (`np.any(y_gaze, axis=(2, 3)).all()`).  `has_gaze`: `[F,2]` booleans (rows beyond the cut are ignored)."""
    count_bs = int(n_frames) // int(time_dims)
    keep = count_bs * time_dims
    group = batch_size * time_dims
    steps = math.ceil(count_bs / batch_size)
    out = []
    for i in range(steps):
        a, b = i * group, min((i + 1) * group, keep)
        out.append((a, b, all(bool(has_gaze[f][0]) and bool(has_gaze[f][1]) for f in range(a, b))))
    return out


def validation_aggregates(losses):
    """The reference's bookkeeping for one video from its per-group losses (NaN = a skipped group):
    `video_mean` = `video_loss / bs_steps`, the sum over the groups that ran divided by ALL groups, skipped ones included
    (Demo_Train_Test.py:147, 153); `run_loss` and `num_step`, this video's share of the epoch's `run_loss / num_step`
    (:148-149, 155).  Sums are Python floats added in group order, as `loss.data.item()` is there."""
    video_loss, num_step = 0.0, 0
    for v in losses:
        v = float(v)
        if not math.isnan(v):
            video_loss += v
            num_step += 1
    return {"video_mean": video_loss / len(losses), "run_loss": video_loss, "num_step": num_step}


def _gaze_groups_loop(model, frames_u8, gauss_prior, ob_prior, fix_map, fix_loc, batch_size, model_size, frame_layout, bgr,
                      gaze_layout, prepare, step):
    """The loop over one video that `validate_video` and `finetune_video` share (Demo_Train_Test.py:105-153): argument
    checks, the ground truth of the whole video by one `prepare` call, the groups and their skip rule, frames uploaded and
    letterboxed per group, priors as zero-stride views, the carried state, the per-group table and the aggregates.
    `step(x, cb, state, y_gaze_of_the_group) -> (loss 0-d tensor, next state)` is what a group that runs does."""
    prepare = prepare or ops.prepare_gaze
    dev = next(model.parameters()).device
    T = model.time_dims
    letterbox = None
    if model_size is None:
        if frame_layout != "CHW" or bgr:
            raise RuntimeError("frame_layout / bgr describe source-size frames: pass model_size=(R, C) with them")
    else:
        if frame_layout not in ("CHW", "HWC") or frames_u8.dim() != 4 or frames_u8.dtype != torch.uint8:
            raise RuntimeError("model_size needs uint8 frames [F,3,H0,W0] (frame_layout='CHW') or [F,H0,W0,3] ('HWC')")
        R, C = int(model_size[0]), int(model_size[1])
        h0, w0 = (frames_u8.shape[2:] if frame_layout == "CHW" else frames_u8.shape[1:3])
        ops.letterbox_geometry(h0, w0, R, C)              # a degenerate picture raises here, before anything is launched
        letterbox = (R, C, frame_layout, bool(bgr))
    # the output size of the model is the size of its prior maps (shape_r_out x shape_c_out, Demo_Train_Test.py:64, 105-106)
    with torch.no_grad():
        y_gaze, has_gaze = prepare(fix_map.to(dev), fix_loc.to(dev), gauss_prior.shape[-2], gauss_prior.shape[-1], gaze_layout)
    n_frames = min(frames_u8.shape[0], y_gaze.shape[0])                 # Demo_Train_Test.py:109
    if (n_frames // T) * T < 2:
        raise RuntimeError("need at least one full chunk of time_dims >= 2 frames")
    groups = validation_groups(n_frames, T, batch_size, has_gaze.cpu().tolist())     # the one wait for the device
    gauss_prior, ob_prior = gauss_prior.to(dev), ob_prior.to(dev)
    state, ran = None, []
    for a, b, run in groups:
        if not run:
            continue
        x = frames_u8[a:b]
        if x.device != torch.device(dev):
            x = x.to(dev, non_blocking=True)
        if letterbox is not None:
            x = ops.letterbox_frames(x, letterbox[0], letterbox[1], layout=letterbox[2], bgr=letterbox[3])
        n = b - a
        cb = [gauss_prior.unsqueeze(0).expand(n, -1, -1, -1), ob_prior.unsqueeze(0).expand(n, -1, -1, -1)]
        loss, state = step(x, cb, state, y_gaze[a:b])
        ran.append(loss.reshape(()))
    vals = torch.stack(ran).cpu().tolist() if ran else []                # the one copy back
    per_group = torch.full((len(groups),), float("nan"), dtype=torch.float32)
    for i, v in zip([i for i, g in enumerate(groups) if g[2]], vals):
        per_group[i] = v
    res = {"losses": per_group, "groups_run": len(ran)}
    res.update(validation_aggregates(per_group.tolist()))
    return res


@torch.no_grad()
def validate_video(model, frames_u8: torch.Tensor, gauss_prior: torch.Tensor, ob_prior: torch.Tensor,
                   fix_map: torch.Tensor, fix_loc: torch.Tensor, batch_size: int = 4, model_size: Optional[tuple] = None,
                   frame_layout: str = "CHW", bgr: bool = False, gaze_layout: Optional[str] = None, criterion=None,
                   prepare=None):
    """The inner loop of the reference's `val` phase for one video (Demo_Train_Test.py:105-153, `model.eval()`, no
    gradient): forward, criterion and gaze ground truth on the device.  `frames_u8`, `gauss_prior`, `ob_prior`,
    `batch_size`, `model_size`, `frame_layout`, `bgr` as in `predict_video`; `fix_map` / `fix_loc` the video's source-size
    uint8 `fixMap` / `fixLoc` in any layout `ops.prepare_gaze` reads (`gaze_layout` is its `layout`).
    Kept from the reference: the video is cut to whole `time_dims` chunks (of the shortest of frames, maps and fixations);
    groups are `batch_size * time_dims` frames, the last one shorter; a group in which a frame lacks a non-zero map or a
    fixation is skipped BEFORE its forward, so the carried state does not advance over it; the maps stay in 0..255; the
    video's mean divides by all groups.  Groups run one after the other through `model(...)`.
    The ground truth of the whole video is prepared by one call up front and its flags are the only thing the host waits
    for; the forwards and the loss launches are then queued without synchronisation and the losses come back in one copy.
    Returns a dict: `losses` float32 `[groups]` on the host (NaN for a skipped group), `groups_run`, `video_mean`,
    `run_loss`, `num_step` (see `validation_aggregates`).
    `criterion` (default `losses.loss_fu`) and `prepare` (default `ops.prepare_gaze`) may be replaced."""
    from . import losses as _losses
    criterion = criterion or _losses.loss_fu
    lstm = getattr(model, "rnn_type", "twa") == "lstm"

    def step(x, cb, state, y):
        out, st = model(x, cb, state)
        return criterion(out, y), ([(st[0].detach(), st[1].detach())] if lstm else [st[0].detach()])
    return _gaze_groups_loop(model, frames_u8, gauss_prior, ob_prior, fix_map, fix_loc, batch_size, model_size, frame_layout,
                             bgr, gaze_layout, prepare, step)


def finetune_video(model, frames_u8: torch.Tensor, gauss_prior: torch.Tensor, ob_prior: torch.Tensor,
                   fix_map: torch.Tensor, fix_loc: torch.Tensor, optimizer, batch_size: int = 4,
                   model_size: Optional[tuple] = None, frame_layout: str = "CHW", bgr: bool = False,
                   gaze_layout: Optional[str] = None, criterion=None, prepare=None, stages=("rnn",), refresh="host",
                   batch_stats=(), block_stats=()):
    """The inner loop of the reference's `train` phase for one video (Demo_Train_Test.py:105-153), for the stage this package
    trains: the ConvTWA recurrence `model.rnn` (train/).  Arguments, groups, skip rule, carried detached state and returned
    aggregates are `validate_video`'s (one loop serves both); every group that runs does
    `optimizer.zero_grad()`, `train.recurrence_step(...)`, `optimizer.step()`, `model.refresh_weights(model.rnn)`.
    `optimizer` is the caller's `torch.optim` object over `model.rnn.parameters()`; the reference uses
    `Adam(lr=1e-4, betas=(0.9, 0.999), weight_decay=5e-5)` (Demo_Train_Test.py:68-69) over ALL parameters.  Different from
    the reference on purpose: the model stays in `eval()` -- every other stage is frozen and every BatchNorm uses its running
    statistics.  A group's loss is the loss BEFORE its step, as `loss.data.item()` is there.
    `stages`: `("rnn",)` or `("rnn", "decoder")`: with the decoder, `recurrence_step(..., decoder=True)` also sets the
    gradients of `model.conv_out_st` (the optimiser then holds its parameters too) and both stages are refreshed.
    `"fuse"` (after `"rnn"` and, when present, `"decoder"`): `recurrence_step(..., fuse=True)` also sets the gradients of
    the fusion block in front of the recurrence (`train.fuse_block`: `model.fucbst_layer[0]` with any prior enabled, else
    `model.fust_layer[0]`), and that block's container is refreshed with the other trained stages.
    `"fust"` (last, and only behind `"fuse"`; a model with at least one prior): `recurrence_step(..., fust=True)` also sets
    the gradients of `model.fust_layer[0]` behind the priors, and `model.fust_layer` is refreshed as well.
    `"ctx"` (last of all, only behind `"fuse"`, with or without `"fust"`; a model with at least one prior):
    `recurrence_step(..., ctx=True)` also sets the gradients of the multi-prior path -- `model.fucb_layer[0]` and, with the
    context prior, both blocks of `model.cxt_cb_prior` -- and those containers are refreshed as well.
    `"nets"` (last of all, only behind `"fuse"`, with or without `"fust"` / `"ctx"`; a model with the gauss or the ob prior):
    `recurrence_step(..., nets=True)` also sets the gradients of the prior nets `model.gauss_cb_layer` / `model.ob_cb_layer`,
    and the enabled nets' containers are refreshed as well (which makes the next call run them again on the priors it is
    handed).  With every stage named, the optimiser may hold exactly the parameters the reference's does.
    `"st"` (the very last stage, only behind `"fuse"` and, in a model with priors, `"fust"`): `recurrence_step(..., st=True)`
    also sets the gradients of the ST blocks `model.st_layer` -- frozen in the reference's own `train()`, the first thing to
    unfreeze on a new dataset -- and `model.st_layer` is refreshed as well.
    `"srf"` (the very last stage of all, only behind `"st"`): `recurrence_step(..., srf=True)` also sets the gradients of the
    SRF-Net head `train.srf_head(model)` -- everything in `model.sfnet` but the ImageNet `features` -- and those eight modules
    are refreshed as well.
    `"backbone"` (only behind `"srf"`): `recurrence_step(..., backbone=True)` also sets the gradients of the deep backbone
    `train.backbone_blocks(model)` -- MobileNetV2 `features[8:18]` -- and those ten modules are refreshed as well;
    `features[0..7]` stay frozen unless `"shallow"` follows.
    `"shallow"` (only behind `"backbone"`): `recurrence_step(..., shallow=True)` also sets the gradients of the shallow backbone
    `train.shallow_blocks(model)` -- MobileNetV2 `features[2:8]` -- and those six modules are refreshed as well, with
    `fused_t=True` (their packed forms are transposed-layout fused entries); the stem and `features[1]` stay frozen.
    `refresh`: `"host"` (the default) repacks the trained stages' weights on the host after every step; `"device"` repacks
    them on the GPU (`model.refresh_weights(..., device=True)`: the same bytes, no copy through the host).
    A `UAVSAL_LSTM` model (`rnn_type == "lstm"`) is trained the same way: the step is `recurrence_step(..., lstm=True)`
    (`train.lstm_backward`), the carried state is `[(h.detach(), c.detach())]` as in `validate_video`, and `stages`, their
    order rules and `refresh` are unchanged -- `"rnn"` is then the ConvLSTM's `[1024,512,3,3]` weight.
    `batch_stats=("decoder",)` (needs `"decoder"` in `stages`): the keyword is passed through to `recurrence_step`, which then
    runs the decoder's BatchNorms on the statistics of each group and moves their running statistics, as the reference's
    `train` phase does; `model.conv_out_st` is put into training mode for the steps and its mode restored afterwards (the
    model itself stays in `eval()`).  `validate_video` stays on the running statistics, as the reference's `val` phase does.
    `block_stats=("fuse",)` (needs `"fuse"` in `stages`; combines with `batch_stats`): likewise for the fusion block in front of
    the recurrence -- the keyword is passed through to `recurrence_step`, the block's container (`train.fuse_container`) is put
    into training mode for the steps and its mode restored afterwards, also when a step raises."""
    from . import losses as _losses
    from . import train as _train
    criterion = criterion or _losses.loss_fu
    stages = tuple(stages)
    if refresh not in ("host", "device"):
        raise ValueError("refresh must be 'host' or 'device', got %r" % (refresh,))
    if not _train.stages_allowed(model, stages):
        raise ValueError("stages must be 'rnn' followed by any of 'decoder', 'fuse' in that order, and 'fust' last behind "
                         "'fuse' (then 'ctx', then 'nets', behind 'fuse' too; 'st' the very last, behind 'fuse' and, in a "
                         "model with priors, 'fust'; only 'srf' may follow 'st', only 'backbone' 'srf', only 'shallow' 'backbone'), got %r" % (stages,))
    kw = {s: True for s in stages[1:]}
    batch_stats = (batch_stats,) if isinstance(batch_stats, str) else tuple(batch_stats)
    if batch_stats:
        for name in batch_stats:
            if name not in _train.BATCH_STATS:
                raise NotImplementedError("batch_stats covers %r only; the BatchNorms of stage %r stay on their running "
                                          "statistics" % (_train.BATCH_STATS, name))
        if "decoder" not in stages:
            raise ValueError("batch_stats=('decoder',) needs 'decoder' in stages, got %r" % (stages,))
        kw["batch_stats"] = batch_stats                   # (without it the call keeps the keywords it always had)
    block_stats = (block_stats,) if isinstance(block_stats, str) else tuple(block_stats)
    if block_stats:
        for name in block_stats:
            if name not in _train.BLOCK_STATS:
                raise NotImplementedError("block_stats covers %r only; the BatchNorms of stage %r stay on their running "
                                          "statistics" % (_train.BLOCK_STATS, name))
        if "fuse" not in stages:
            raise ValueError("block_stats=('fuse',) needs 'fuse' in stages, got %r" % (stages,))
        kw["block_stats"] = block_stats                   # (likewise)
    lstm = getattr(model, "rnn_type", "twa") == "lstm"
    if lstm:
        kw["lstm"] = True                                 # (a ConvTWA model's call keeps the keywords it always had)

    def step(x, cb, state, y):
        optimizer.zero_grad()
        loss, _, state = _train.recurrence_step(model, x, cb, state, y, criterion, **kw)
        if lstm:                                          # the ConvLSTM carries (h, c), as in validate_video
            state = [(state[0].detach(), state[1].detach())]
        optimizer.step()
        mods = _train.stage_modules(model, kw)
        if "shallow" in kw:
            model.refresh_weights(*mods, device=refresh == "device", fused_t=True)
        elif refresh == "device":
            model.refresh_weights(*mods, device=True)
        else:
            model.refresh_weights(*mods)                  # (no keyword: a model-like object without `device=` keeps working)
        return loss, state
    was = model.conv_out_st.training if batch_stats else None
    box = _train.fuse_container(model) if block_stats else None
    box_was = [(m, m.training) for m in box.modules()] if block_stats else []
    try:
        if batch_stats:
            model.conv_out_st.train()
        if block_stats:
            box.train()
        return _gaze_groups_loop(model, frames_u8, gauss_prior, ob_prior, fix_map, fix_loc, batch_size, model_size, frame_layout,
                                 bgr, gaze_layout, prepare, step)
    finally:
        if batch_stats:
            model.conv_out_st.train(was)
        for m, mode in box_was:
            m.training = mode


class RequestPipeline:
    """Independent requests (clips of DIFFERENT videos: no carried state between them) kept `streams` deep in
    flight: request k runs on host stream k % streams through its own handle on the model (`_inflight_replicas`: same weights,
    own lane-less launch plans), so the tail of one forward (ConvTWA steps, decoder) overlaps the head of the next.
    Per-request arithmetic and results are unchanged (bitwise: tests/test_hip_e2e.py); one request's latency grows,
    throughput rises -- 1890 -> 2068-2087 frames/s fp32 at one 8-frame clip per request, two streams
    (profiles/r5_experiments.md; round 2: 1505 -> 1607).
    Requests of the SAME video are ordered by their state: `predict_video` overlaps those up to the recurrence."""

    def __init__(self, model, streams: int = 2):
        self.model = model
        self.models = _inflight_replicas(model, max(1, int(streams)))      # lane-less handles, see there
        self._streams = None
        self._k = 0

    @torch.no_grad()
    def forward_clips(self, x, cb, state=None):
        """As `UAVSal.forward_clips`, asynchronous: returns (maps, state, event).  The outputs are produced on the
        replica's stream: wait for `event` (or call `synchronize()`) before using them on another stream."""
        dev = x.device
        if self._streams is None:
            self._streams = _host_streams(dev, len(self.models))
        i = self._k % len(self.models)
        if self._k % len(self.models) == 0:
            self.models = _inflight_replicas(self.model, len(self.models))      # follow the model's settings / weight edits
        self._k += 1
        s = self._streams[i]
        s.wait_stream(torch.cuda.current_stream(dev))        # inputs were produced on the caller's stream
        with torch.cuda.stream(s):
            for t in [x, *cb] + ([state] if torch.is_tensor(state) else []):
                t.record_stream(s)
            out, st = self.models[i].forward_clips(x, cb, state)
            ev = torch.cuda.Event()
            ev.record(s)
        return out, st, ev

    def synchronize(self):
        """Waits for every request in flight and raises if any of them reported a device error."""
        for s in self._streams or []:
            s.synchronize()
        for m in self.models:
            m.check_errors()
