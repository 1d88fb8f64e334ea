"""Packed device weights of a model: BatchNorm folded, weights in the layouts of packing.py, uploaded once and remembered.

`WeightCache(device, store)` wraps the dictionary a model keeps per device (`model._wshared[device]`); the dictionary stays
the store, so every engine of the model -- whatever its precision -- and every replica share one copy, and dropping the
dictionary drops the weights.  One method per kind of parameter set; each is the only place where that kind's key is built
and its tensors are made.  Keys carry `id(module)`: an entry holds that module's parameters as they were when it was packed
(`model.invalidate_engines()` after an edit)."""
import torch

from . import packing as P


def _seq(x):
    return list(x) if isinstance(x, (list, tuple)) else [x]


def _ids(mods):
    return tuple(id(m) for m in mods)


def _folded(bns):
    """(scale, bias) of BatchNorms whose channels lie side by side."""
    parts = [P.fold_bn(b) for b in bns]
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])


def _weight(convs, wslice):
    w = torch.cat([c.weight.detach() for c in convs], 0)
    return w if wslice is None else w[:, wslice[0]:wslice[1]]


def _scaled_t(conv, bn):
    s = P.fold_bn(bn)[0]
    return (conv.weight.detach().float().cpu() * s.view(-1, 1, 1, 1)).transpose(0, 1).flip(2, 3)


def _bn_stats(bn):
    r = 1.0 / torch.sqrt(bn.running_var.detach().double().cpu() + bn.eps)
    return r.float(), bn.running_mean.detach().float().cpu()


def _bn_after(mods, conv):
    """The BatchNorm that follows `conv` in the container (among `mods`) that holds both."""
    for m in mods.values():
        ch = list(m.children())
        for a, b in zip(ch, ch[1:]):
            if a is conv and isinstance(b, torch.nn.BatchNorm2d):
                return b
    raise RuntimeError("the BatchNorm of a packed depthwise entry is not among the refreshed modules: pass the whole block")


def _block_of(mods, dwc):
    """The inverted-residual block (among `mods`) whose depthwise conv is `dwc`."""
    for m in mods.values():
        seq = list(getattr(m, "conv", None) or []) if hasattr(m, "expand_ratio") else []
        i = 0 if getattr(m, "expand_ratio", None) == 1 else 1
        if len(seq) > i and isinstance(seq[i], torch.nn.Sequential) and len(seq[i]) and seq[i][0] is dwc:
            return m
    raise RuntimeError("the block of a packed fused entry is not among the refreshed modules: pass the whole block")


def _fused_host(blk, natural):
    """The host tensors of a fused-block entry, by name (`WeightCache.fused_block`)."""
    seq = list(blk.conv)
    pw, pwbn = (None, None) if blk.expand_ratio == 1 else (seq[0][0], seq.pop(0)[1])
    dwc, dwbn, pl, plbn = seq[0][0], seq[0][1], seq[1], seq[2]

    def mat(conv):
        w = conv.weight.detach().float().cpu().reshape(conv.weight.shape[:2])
        return w.clone() if natural else w.t()           # (a copy: on a CPU store the entry must not alias the parameter)
    ws = {}
    if pw is not None:
        ws["w1"], ws["s1"], ws["b1"] = (mat(pw), *P.fold_bn(pwbn))
    ws["wd"], ws["sd"], ws["bd"] = (P.pack_dw_weight(dwc.weight), *P.fold_bn(dwbn))
    ws["w2"], ws["s2"], ws["b2"] = (mat(pl), *P.fold_bn(plbn))
    return ws


# kind -> the module ids of a key of that kind (everything `refresh` can remake); "fused": the natural-layout entries only
_REFRESH_IDS = {"fused": lambda k: k[1:2], "w": lambda k: k[1:-3], "wino": lambda k: k[1:2], "wT": lambda k: k[1:2], "wTs": lambda k: k[1:3],
                "bn": lambda k: k[1:-1], "bnstat": lambda k: k[1:2], "dw": lambda k: k[1:], "dwdot": lambda k: k[1:3]}


class WeightCache:
    def __init__(self, device, store):
        self.device, self.store = torch.device(device), store

    def _get(self, key, make):
        if key not in self.store:
            self.store[key] = make()
        return self.store[key]

    def _up(self, *ts):
        return tuple(t.contiguous().to(self.device) for t in ts)      # kept alive by the store

    def affine(self, bn, cout):
        """(scale, bias) of one BatchNorm or a list (several convs of the same input as ONE GEMM: outputs side by side), padded
        to `roundup(cout, 32)` with the identity."""
        bns, n = _seq(bn), P.roundup(cout, 32)

        def make():
            s, b = _folded(bns)
            return self._up(P.pad_vec(s, n, 1.0), P.pad_vec(b, n, 0.0))
        return self._get(("bn",) + _ids(bns) + (cout,), make)

    def conv(self, conv, wslice, gate_interleave, layout):
        """The weights of one conv or a list (output channels side by side), input channels `wslice` = (first, end) of them,
        packed for `layout` (packing.conv_weight_layout).  `gate_interleave` = hidden size of a ConvLSTM whose gate rows are
        interleaved: row g * hid + c -> 4 * c + g (gates i, f, o, g adjacent)."""
        convs = _seq(conv)

        def make():
            w = _weight(convs, wslice)
            if gate_interleave:
                w = w.reshape(4, gate_interleave, *w.shape[1:]).permute(1, 0, 2, 3, 4).reshape(w.shape)
            return self._up(P.pack_conv_weight(w, layout))[0]
        return self._get(("w",) + _ids(convs) + (wslice, layout, gate_interleave), make)

    def wino(self, conv, wslice, r):
        """The Winograd F(r x r, 3x3) filter transform of a dense 3x3 conv (input channels `wslice`)."""
        return self._get(("wino", id(conv), wslice, r), lambda: self._up(P.pack_wino_weight(_weight([conv], wslice), r))[0])

    def conv_t(self, conv, wslice, layout):
        """The weights of the TRANSPOSED conv of `conv` (input channels `wslice`), packed for `layout`: input and output channels
        swapped and the taps flipped, `Wt[ci, co, ky, kx] = W[co, ci, 2 - ky, 2 - kx]` -- the conv that carries a gradient with
        respect to `conv`'s output back to its input (train/)."""
        def make():
            w = _weight([conv], wslice).transpose(0, 1).flip(2, 3)
            return self._up(P.pack_conv_weight(w, layout))[0]
        return self._get(("wT", id(conv), wslice, layout), make)

    def conv_t_scaled(self, conv, bn, layout):
        """The weights of the transposed 1x1 conv of `conv` + BatchNorm `bn` with the BatchNorm's folded scale s in its rows,
        `Wt[ci, co] = s[co] W[co, ci]` (the product rounded once), packed for `layout`: it carries the gradient with respect
        to the BatchNorm's OUTPUT back to the conv's input (train.decoder_backward)."""
        def make():
            return self._up(P.pack_conv_weight(_scaled_t(conv, bn), layout))[0]
        return self._get(("wTs", id(conv), id(bn), layout), make)

    def bn_stats(self, bn):
        """(r, mu) of one BatchNorm on the device: r = 1 / sqrt(running_var + eps) computed in double and rounded once, mu the
        running mean -- what the gradient of the BatchNorm's weight needs beside the fold (train.decoder_param_grads)."""
        return self._get(("bnstat", id(bn)), lambda: self._up(*_bn_stats(bn)))

    def refresh(self, mods, dry=False, fused_t=False):
        """Repack, INTO THE EXISTING DEVICE TENSORS, every entry whose key holds the id of a module in `mods` (id -> module)
        from the module's current parameters: launch plans that recorded the tensors' addresses stay valid.  Conv weights in
        every layout, their Winograd transforms and transposed forms, BatchNorm folds (with their identity padding) and
        statistics, depthwise and depthwise-dot entries and the natural-layout fused blocks (csrc/fused_mid.hip: the 1x1
        weights as the module holds them; the key holds the depthwise conv alone, its neighbours are found in the block that
        holds it, which must be in `mods`) are refreshable; a transposed-layout fused block or a stem that names such a module
        raises -- `model.invalidate_engines()` is for those.  A key that joins several modules needs all of them in `mods`;
        a depthwise entry's key holds its conv alone: its BatchNorm is the module that follows the conv in the container
        that holds both, which must be in `mods` too (pass the block, not the conv).
        `dry`: only check that every such entry can be remade (raise otherwise), pack and copy nothing.
        `fused_t=True` (opt-in): a transposed-layout fused block (csrc/fused_ir.hip: the 1x1 weights as [Cin][Cout] -- MobileNetV2
        `features[1:8]`) whose block is among `mods` is remade in place as well, from `_fused_host(blk, False)`, and checked in
        the dry pass like the natural-layout ones.  Without it such an entry raises, as it always did; the stem raises either way.
        Returns the number of entries refreshed (that would be)."""
        n = 0
        for key in list(self.store):
            if not isinstance(key, tuple) or not any(isinstance(i, int) and i in mods for i in key[1:]):
                continue
            kind = key[0]
            if kind not in _REFRESH_IDS or (kind == "fused" and not key[2] and not fused_t):
                raise NotImplementedError("packed %r weights cannot be refreshed in place: call model.invalidate_engines()" % (kind,))
            ids = _REFRESH_IDS[kind](key)
            if not all(i in mods for i in ids):
                raise RuntimeError("a packed %r entry joins several modules: refresh all of them together" % (kind,))
            if kind == "fused":
                new = _fused_host(_block_of(mods, mods[key[1]]), bool(key[2]))   # raises in the dry pass when the block is missing
                if sorted(new) != sorted(self.store[key]):
                    raise RuntimeError("a packed fused entry does not match its block any more: call model.invalidate_engines()")
                if not dry:
                    for name, src in new.items():
                        self.store[key][name].copy_(src.contiguous().to(self.device, non_blocking=False))
                n += 1
                continue
            if kind in ("bn", "bnstat", "dw", "dwdot", "wTs"):
                new = self._remake(kind, key, [mods[i] for i in ids], mods)      # small: made in the dry pass too, so that it can raise
                if not dry:
                    for dst, src in zip(self.store[key] if isinstance(self.store[key], tuple) else (self.store[key],), new):
                        dst.copy_(src.to(self.device, non_blocking=False))
                n += 1
                continue
            if dry:
                n += 1
                continue
            if kind == "w":
                ids, (wslice, layout, gi) = key[1:-3], key[-3:]
                w = _weight([mods[i] for i in ids], wslice)
                if gi:
                    w = w.reshape(4, gi, *w.shape[1:]).permute(1, 0, 2, 3, 4).reshape(w.shape)
                new = P.pack_conv_weight(w, layout)
            elif kind == "wino":
                new = P.pack_wino_weight(_weight([mods[key[1]]], key[2]), key[3])
            else:
                new = P.pack_conv_weight(_weight([mods[key[1]]], key[2]).transpose(0, 1).flip(2, 3), key[3])
            self.store[key].copy_(new.to(self.device, non_blocking=False))
            n += 1
        return n

    def refresh_device(self, mods, dry=False, fused_t=False):
        """`refresh` without the host: every entry `refresh` would remake is remade by ONE launch of csrc/repack.hip on torch's
        current stream, from the fp32 parameters and buffers where they lie on this device into the same packed tensors, to
        the same bytes (the Winograd transforms: within one fp32 ulp).  The table of entries (repack.py) is built
        and uploaded at the first call and kept in the store under a key `refresh` passes over; before every reuse the
        addresses of every source and destination and the set of keys are compared with what it recorded, and it is rebuilt
        when one differs.  Once the table exists a call copies nothing to or from the host and waits for nothing.
        Raises what `refresh` raises, and ValueError -- before anything is written -- for what only the host path can do: a
        CPU store, a parameter or buffer that is not fp32 ON THIS DEVICE (so a model whose packed weights live on two GPUs
        cannot refresh the second store this way: its parameters are on one), or one that is not contiguous (a 3x3 weight kept
        in `channels_last`).
        `dry`: build and check the table, launch nothing.  Returns the number of entries refreshed, as `refresh` does.
        `fused_t`: as in `refresh`; the transposed 1x1 weights are written by the same launch (entry kind COPY_T)."""
        from . import repack
        return repack.refresh(self, mods, dry, fused_t)

    def _remake(self, kind, key, ms, mods):
        """The host tensors of one refreshable non-conv entry, in the order of the stored tuple."""
        if kind == "bn":
            s, b = _folded(ms)
            n = P.roundup(key[-1], 32)
            return P.pad_vec(s, n, 1.0), P.pad_vec(b, n, 0.0)
        if kind == "bnstat":
            return _bn_stats(ms[0])
        if kind == "wTs":
            return (P.pack_conv_weight(_scaled_t(ms[0], ms[1]), key[3]),)
        if kind == "dw":
            return (torch.cat([P.pack_dw_weight(c.weight) for c in ms], 1), *_folded([_bn_after(mods, c) for c in ms]))
        dwc, pl = ms
        return (P.pack_dw_weight(dwc.weight), *P.fold_bn(_bn_after(mods, dwc)), pl.weight.detach().float().cpu().reshape(-1),
                *(t.reshape(1) for t in P.fold_bn(_bn_after(mods, pl))))

    def depthwise(self, conv, bn):
        """(tap-major weights, scale, bias) of a depthwise 3x3 + BatchNorm, or of a list of them as channel groups.  The
        standalone launch and the depthwise inside a projection GEMM's loader share the entry."""
        convs = _seq(conv)
        return self._get(("dw",) + _ids(convs), lambda: self._up(torch.cat([P.pack_dw_weight(c.weight) for c in convs], 1),
                                                                *_folded(_seq(bn))))

    def dw_dot(self, dwc, dwbn, pl, plbn):
        """Depthwise 3x3 + BatchNorm -> projection to ONE channel + BatchNorm: (w9, scale, bias, w2, scale2, bias2)."""
        return self._get(("dwdot", id(dwc), id(pl)), lambda: self._up(
            P.pack_dw_weight(dwc.weight), *P.fold_bn(dwbn), pl.weight.detach().float().reshape(-1),
            *(t.reshape(1) for t in P.fold_bn(plbn))))

    def fused_block(self, blk, natural):
        """An inverted-residual block for the one-launch kernels: {w1, s1, b1 (with an expand conv), wd, sd, bd, w2, s2, b2}.
        The 1x1 weights are [Cin][Cout], or -- `natural` (csrc/fused_mid.hip) -- as the module holds them, [Cout][Cin]."""
        dwc = list(blk.conv)[0 if blk.expand_ratio == 1 else 1][0]
        return self._get(("fused", id(dwc), natural), lambda: {k: self._up(v)[0] for k, v in _fused_host(blk, natural).items()})

    def stem(self, conv, bn):
        """(weights [27, 32], scale, bias) of the stem conv + BatchNorm."""
        return self._get(("stem", id(conv)), lambda: self._up(P.pack_stem_weight(conv.weight), *P.fold_bn(bn)))
