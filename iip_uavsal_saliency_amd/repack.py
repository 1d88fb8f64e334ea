"""Repack refreshed weights ON THE DEVICE: the second path of `WeightCache.refresh` (weights.py), for the step after
`optimizer.step()`.  The parameters are on the device and so are their packed copies; `entries` describes, per packed tensor,
how csrc/repack.hip makes the one from the other (the bytes packing.py makes on the host), `refresh` keeps the table of
them in device memory and launches it -- one launch, no copy to or from the host once the table exists.

`entries` is pure Python (no device call): it walks the store exactly as `WeightCache.refresh` does -- same key tests, same
`_REFRESH_IDS`, same neighbours (`_bn_after`, `_block_of`), same errors -- and tests/repack_ref.py restates the kernel's
per-element function over what it returns."""
import ctypes as C

import torch

from . import _lib as L
from . import packing as P
from . import weights as W

THREADS = 256                     # threads of a workgroup of repack_kernel: one unit each
MAX_BLOCKS = 1 << 24              # UAVSAL_REPACK_MAX_BLOCKS: 2^32 threads of one launch / 256
TABLE_KIND = "repack"             # first element of the store key of a table: in no kind list of weights.py


class Entry:
    """One packed tensor and how it is made (include/uavsal_hip.h, uavsal_repack_entry).  `dst`, `src`, `beta`, `mean`, `var`,
    `sg`, `sv` are tensors here; `owners` lists (module, attribute) of every source so that a replaced parameter is seen."""

    def __init__(self, key, kind, dst, **kw):
        self.key, self.kind, self.dst = key, kind, dst
        self.layout, self.layout_name = 0, None
        self.src, self.beta, self.mean, self.var, self.eps, self.rows = [], [], [], [], [], []
        self.N = self.C = self.Npad = self.Kpad = self.P = 0
        self.taps, self.kt, self.flip, self.gi = 1, 16, 0, 0
        self.sN = self.sC = self.off = 0
        self.sg = self.sv = None
        self.seps, self.pad, self.G = 0.0, 0.0, []
        self.units, self.nbytes, self.owners = 0, 0, []
        for k, v in kw.items():
            setattr(self, k, v)

    def own(self, mod, name):
        t = getattr(mod, name)
        self.owners.append((mod, name))
        return t

    def sources(self):
        return self.src + self.beta + self.mean + self.var + [t for t in (self.sg, self.sv) if t is not None]


def _cum(ns):
    out, s = [], 0
    for n in ns:
        s += int(n)
        out.append(s)
    return out


def _limit(ms):
    if len(ms) > L.REPACK_MAX_SRC:
        raise NotImplementedError("a packed entry joins %d modules side by side: the device repack takes %d" % (len(ms), L.REPACK_MAX_SRC))


def _conv(key, dst, convs, wslice, layout, gi=0, transposed=False, scale_bn=None):
    """A `pack_conv_weight` entry: `convs` side by side over Cout, input channels `wslice`; `transposed`: the conv that swaps
    input and output channels and flips the taps (one conv); `scale_bn`: its folded scale in the rows (1x1, transposed)."""
    _limit(convs)
    e = Entry(key, L.REPACK_CONV, dst, layout=L.REPACK_LAYOUT[layout], layout_name=layout, gi=int(gi or 0))
    e.src = [e.own(c, "weight") for c in convs]
    cin_full, kh, kw = (int(v) for v in e.src[0].shape[1:])
    if any(tuple(w.shape[1:]) != (cin_full, kh, kw) for w in e.src):
        raise RuntimeError("convs packed side by side differ in their input channels or taps")
    e.taps = kh * kw
    assert e.taps in (1, 9) and kh == kw
    lo, hi = (0, cin_full) if wslice is None else (int(wslice[0]), int(wslice[1]))
    cout = sum(int(w.shape[0]) for w in e.src)
    e.off = lo * e.taps
    if transposed:
        assert len(convs) == 1
        e.N, e.C, e.sN, e.sC, e.flip, e.rows = hi - lo, cout, e.taps, cin_full * e.taps, 1, [hi - lo]
    else:
        e.N, e.C, e.sN, e.sC, e.rows = cout, hi - lo, cin_full * e.taps, e.taps, _cum(w.shape[0] for w in e.src)
    if scale_bn is not None:
        e.sg, e.sv, e.seps = e.own(scale_bn, "weight"), e.own(scale_bn, "running_var"), float(scale_bn.eps)
    if e.gi and e.N != 4 * e.gi:
        raise RuntimeError("gate_interleave %d does not match %d rows" % (e.gi, e.N))
    e.kt = 16 if layout == "f32" else 32
    if e.taps == 9 and e.C % 32:
        raise RuntimeError("3x3 dense conv needs Cin % 32 == 0")
    assert layout != "f16x3j" or e.taps == 1
    e.Kpad, e.Npad = P.roundup(e.taps * e.C, e.kt), P.roundup(e.N, 32)
    n = e.Npad * e.Kpad
    if e.layout == L.REPACK_LAYOUT["f32"]:
        e.units, e.nbytes = n // 4, 4 * n
    else:
        halves = n if layout == "bf16" else 2 * n
        e.units, e.nbytes = halves // 8, 2 * halves
    return e


def _wino(key, dst, conv, wslice, r):
    e = Entry(key, L.REPACK_WINO, dst, taps=9, P=r + 2, G=[float(v) for row in P._WINO_G[r] for v in row])
    e.src = [e.own(conv, "weight")]
    cout, cin_full, kh, kw = (int(v) for v in e.src[0].shape)
    assert kh == 3 and kw == 3
    lo, hi = (0, cin_full) if wslice is None else (int(wslice[0]), int(wslice[1]))
    e.N, e.C, e.sN, e.sC, e.off, e.rows = cout, hi - lo, cin_full * 9, 9, lo * 9, [cout]
    e.Kpad, e.Npad = P.roundup(e.C, 32), P.roundup(e.N, 32)
    e.units = e.Npad * e.Kpad
    e.nbytes = 4 * e.P * e.P * e.units
    return e


def _fold(key, dst, bns, which, npad=None, pad=0.0):
    """One vector of the BatchNorms `bns` lying side by side, padded to `npad` channels with `pad`."""
    _limit(bns)
    e = Entry(key, L.REPACK_FOLD, dst, layout=which, pad=float(pad))
    for b in bns:
        e.src.append(e.own(b, "weight"))
        e.beta.append(e.own(b, "bias"))
        e.mean.append(e.own(b, "running_mean"))
        e.var.append(e.own(b, "running_var"))
        e.eps.append(float(b.eps))
    e.rows = _cum(t.numel() for t in e.var)
    e.N = e.rows[-1]
    e.Npad = e.N if npad is None else int(npad)
    if e.Npad < e.N:
        raise RuntimeError("a packed BatchNorm entry is shorter than its BatchNorms")
    e.units, e.nbytes = e.Npad, 4 * e.Npad
    return e


def _affine(key, dsts, bns, npad=None):
    return [_fold(key, dsts[0], bns, L.REPACK_SCALE, npad, 1.0), _fold(key, dsts[1], bns, L.REPACK_BIAS, npad, 0.0)]


def _dw(key, dst, convs):
    _limit(convs)
    e = Entry(key, L.REPACK_DW, dst, taps=9)
    e.src = [e.own(c, "weight") for c in convs]
    e.rows = _cum(w.shape[0] for w in e.src)
    e.N = e.rows[-1]
    e.units, e.nbytes = 9 * e.N, 36 * e.N
    return e


def _copy(key, dst, mod, name="weight"):
    e = Entry(key, L.REPACK_COPY, dst)
    e.src = [e.own(mod, name)]
    e.units = e.N = e.src[0].numel()
    e.nbytes = 4 * e.units
    return e


def _copy_t(key, dst, mod, name="weight"):
    """A 1x1 conv weight [Cout][Cin] written transposed, [Cin][Cout]: what `weights._fused_host(blk, False)` holds."""
    e = Entry(key, L.REPACK_COPY_T, dst)
    e.src = [e.own(mod, name)]
    e.N, e.C = int(e.src[0].shape[0]), int(e.src[0].shape[1])
    e.units = e.N * e.C
    e.nbytes = 4 * e.units
    return e


def _fused(key, stored, blk, natural=True):
    """The dictionary of a fused block, name by name as `weights._fused_host` makes it: `natural` the 1x1 weights as the module
    holds them, else transposed."""
    seq = list(blk.conv)
    pw, pwbn = (None, None) if blk.expand_ratio == 1 else (seq[0][0], seq.pop(0)[1])
    dwc, dwbn, pl, plbn = seq[0][0], seq[0][1], seq[1], seq[2]
    names = (["w1", "s1", "b1"] if pw is not None else []) + ["wd", "sd", "bd", "w2", "s2", "b2"]
    if sorted(names) != sorted(stored):
        raise RuntimeError("a packed fused entry does not match its block any more: call model.invalidate_engines()")
    out = []
    mat = _copy if natural else _copy_t
    if pw is not None:
        out += [mat(key, stored["w1"], pw)] + _affine(key, (stored["s1"], stored["b1"]), [pwbn])
    out += [_dw(key, stored["wd"], [dwc])] + _affine(key, (stored["sd"], stored["bd"]), [dwbn])
    return out + [mat(key, stored["w2"], pl)] + _affine(key, (stored["s2"], stored["b2"]), [plbn])


def _of_key(store, key, ms, mods):
    kind, dst = key[0], store[key]
    if kind == "w":
        wslice, layout, gi = key[-3:]
        return [_conv(key, dst, ms, wslice, layout, gi)]
    if kind == "wT":
        return [_conv(key, dst, ms, key[2], key[3], transposed=True)]
    if kind == "wTs":
        return [_conv(key, dst, ms[:1], None, key[3], transposed=True, scale_bn=ms[1])]
    if kind == "wino":
        return [_wino(key, dst, ms[0], key[2], key[3])]
    if kind == "bn":
        return _affine(key, dst, ms, P.roundup(key[-1], 32))
    if kind == "bnstat":
        return [_fold(key, dst[0], ms, L.REPACK_RSTD), _fold(key, dst[1], ms, L.REPACK_MEAN)]
    if kind == "dw":
        return [_dw(key, dst[0], ms)] + _affine(key, dst[1:3], [W._bn_after(mods, c) for c in ms])
    if kind == "dwdot":
        dwc, pl = ms
        return ([_dw(key, dst[0], [dwc])] + _affine(key, dst[1:3], [W._bn_after(mods, dwc)]) + [_copy(key, dst[3], pl)]
                + _affine(key, dst[4:6], [W._bn_after(mods, pl)]))
    return _fused(key, dst, W._block_of(mods, ms[0]), bool(key[2]))


def touched_keys(store, mods):
    """The keys of `store` that hold the id of a module in `mods`: what `WeightCache.refresh` visits, in its order."""
    return [k for k in store if isinstance(k, tuple) and k[0] != TABLE_KIND and any(isinstance(i, int) and i in mods for i in k[1:])]


def entries(cache, mods, fused_t=False):
    """One `Entry` per packed tensor of every store entry whose key holds the id of a module in `mods` (id -> module), in the
    order `WeightCache.refresh` visits them; the keys they carry are the entries `refresh` counts.  Raises what `refresh`
    raises: NotImplementedError for a transposed-layout fused block or the stem, RuntimeError for a key that joins modules
    not all given or whose neighbours (`_bn_after`, `_block_of`) are not among `mods`.  `fused_t=True`: a transposed-layout fused
    block is taken as well (its 1x1 weights as COPY_T entries), as `WeightCache.refresh(fused_t=True)` takes it."""
    out = []
    for key in touched_keys(cache.store, mods):
        kind = key[0]
        if kind not in W._REFRESH_IDS or (kind == "fused" and not key[2] and not fused_t):
            raise NotImplementedError("packed %r weights cannot be refreshed in place: call model.invalidate_engines()" % (kind,))
        ids = W._REFRESH_IDS[kind](key)
        if not all(i in mods for i in ids):
            raise RuntimeError("a packed %r entry joins several modules: refresh all of them together" % (kind,))
        made = _of_key(cache.store, key, [mods[i] for i in ids], mods)
        for e in made:
            if e.dst.numel() * e.dst.element_size() != e.nbytes:
                raise RuntimeError("a packed %r entry does not have the size of its layout any more: call model.invalidate_engines()" % (kind,))
        out.extend(made)
    return out


def _on(t, device):
    return t.device.type == device.type and (device.index is None or t.device.index == device.index)


def _table(ents, device):
    """(host bytes of the table: the descriptors, then the prefix of block counts; blocks) for tensors on `device`."""
    arr = (L.RepackEntry * len(ents))()
    first = (C.c_int32 * (len(ents) + 1))()
    blocks = 0
    for d, e in zip(arr, ents):
        for t in e.sources():
            if not _on(t, device) or t.dtype != torch.float32:
                raise ValueError("the device repack reads fp32 parameters on %s: found %s on %s (use the host path)" % (device, t.dtype, t.device))
            if not t.is_contiguous():
                raise ValueError("the device repack reads contiguous parameters (use the host path)")
        if not _on(e.dst, device) or not e.dst.is_contiguous() or e.dst.data_ptr() % 16:
            raise ValueError("a packed tensor is not a 16-byte aligned dense tensor on %s" % (device,))
        d.kind, d.layout, d.dst, d.units = e.kind, e.layout, e.dst.data_ptr(), e.units
        for name in ("src", "beta", "mean", "var"):
            for i, t in enumerate(getattr(e, name)):
                getattr(d, name)[i] = t.data_ptr()
        for i, v in enumerate(e.eps):
            d.eps[i] = v
        for i, v in enumerate(e.rows):
            d.rows[i] = v
        d.n_src = len(e.rows)
        d.N, d.C, d.taps, d.Npad, d.Kpad, d.kt, d.flip, d.gi, d.P = e.N, e.C, e.taps, e.Npad, e.Kpad, e.kt, e.flip, e.gi, e.P
        d.sN, d.sC, d.off = e.sN, e.sC, e.off
        if e.sg is not None:
            d.sg, d.sv, d.seps = e.sg.data_ptr(), e.sv.data_ptr(), e.seps
        d.pad = e.pad
        for i, v in enumerate(e.G):
            d.G[i] = v
    for i, e in enumerate(ents):
        first[i] = blocks
        blocks += (e.units + THREADS - 1) // THREADS
    first[len(ents)] = blocks
    if blocks >= MAX_BLOCKS:
        raise ValueError("too many blocks for one repack launch")
    return bytes(arr) + bytes(first), blocks


def _dst_ptrs(store, keys):
    """the addresses of the packed tensors the store holds NOW under `keys`"""
    out = []
    for k in keys:
        v = store[k]
        out += [t.data_ptr() for t in (v.values() if isinstance(v, dict) else v if isinstance(v, tuple) else (v,))]
    return out


class _Record:
    """A table in device memory and what it was made from: rebuilt when a key joined the store or a tensor moved.
    It lives in the store under a key made of the sorted module ids and holds, through `owners`, a reference to every module it
    reads: each DISTINCT set of modules a caller refreshes leaves its own table and record there (a training loop has one), and
    nothing evicts one before the store itself is dropped (`model.invalidate_engines()`, a load, an edit of another module)."""

    def __init__(self, cache, mods, fused_t=False):
        self.keys = touched_keys(cache.store, mods)
        ents = entries(cache, mods, fused_t)
        self.n_entries, self.count = len(ents), len(self.keys)
        self.owners = [(m, n, getattr(m, n).data_ptr()) for e in ents for m, n in e.owners]
        self.dsts = _dst_ptrs(cache.store, self.keys)
        self.table, self.blocks, self.bytes_written = None, 0, sum(e.nbytes for e in ents)
        if ents:
            host, self.blocks = _table(ents, cache.device)
            self.table = torch.frombuffer(bytearray(host), dtype=torch.uint8).to(cache.device)      # the one upload

    def current(self, cache, mods):
        return (self.keys == touched_keys(cache.store, mods)
                and all(getattr(m, n).data_ptr() == p for m, n, p in self.owners)
                and self.dsts == _dst_ptrs(cache.store, self.keys))


def refresh(cache, mods, dry=False, fused_t=False):
    """`WeightCache.refresh_device`: see there."""
    if cache.device.type == "cpu":
        raise ValueError("refresh_weights(device=True) needs packed weights on a GPU: this store is on the CPU")
    key = (TABLE_KIND, tuple(sorted(mods))) + ((True,) if fused_t else ())
    rec = cache.store.get(key)
    if rec is None or not rec.current(cache, mods):
        rec = cache.store[key] = _Record(cache, mods, fused_t)
    if not dry and rec.table is not None:
        with torch.cuda.device(cache.device):
            stream = C.c_void_p(torch.cuda.current_stream(cache.device).cuda_stream)
            L.check(L.load().uavsal_repack(C.c_void_p(rec.table.data_ptr()), rec.n_entries, rec.blocks, stream), "uavsal_repack")
    return rec.count
