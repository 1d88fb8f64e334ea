"""A numpy restatement of the per-element function of csrc/repack.hip (include/uavsal_hip.h states it), over the entries
`repack.entries` produces: `pack(e)` returns the bytes the kernel writes into `e.dst`.  Written from the destination's side as
the kernel is -- every destination element is decoded into (row, k, panel), gathered and split -- not by reshuffling as
packing.py does, so that agreement with packing.py checks the kernel's arithmetic and not packing.py against itself.
The Winograd transform is summed in float64 in the kernel's fixed order.

`make_cases(device)` builds the small modules and store entries both test files share."""
import numpy as np
import torch

from iip_uavsal_saliency_amd import _lib as L
from iip_uavsal_saliency_amd.weights import WeightCache


def _np(t):
    return t.detach().cpu().numpy()


def _flat_sources(ts):
    arrs = [_np(t).reshape(-1) for t in ts]
    base = np.cumsum([0] + [a.size for a in arrs[:-1]])
    return np.concatenate(arrs), base


def _src_of(rows, m):
    """(source index, row inside it) of rows `m` for cumulative row counts `rows`"""
    rows = np.asarray(rows)
    s = np.searchsorted(rows, m, side="right")
    s = np.minimum(s, len(rows) - 1)
    lo = np.concatenate([[0], rows[:-1]])[s]
    return s, m - lo


def conv_value(e, n, k):
    """the logical matrix m[n][k] of a CONV entry (float32), for index arrays n, k"""
    n, k = np.asarray(n, np.int64), np.asarray(k, np.int64)
    valid = (n < e.N) & (k < e.C * e.taps)
    if e.taps == 9:
        blk, rem = k // (9 * e.kt), k % (9 * e.kt)
        tap, c = rem // e.kt, blk * e.kt + rem % e.kt
    else:
        tap, c = np.zeros_like(k), k
    m = (n % 4) * e.gi + n // 4 if e.gi else n
    nv, cv, tv, mv = (np.where(valid, a, 0) for a in (n, c, tap, m))
    s, local = _src_of(e.rows, mv)
    cat, base = _flat_sources(e.src)
    st = e.taps - 1 - tv if e.flip else tv
    v = cat[base[s] + e.off + local * e.sN + cv * e.sC + st].astype(np.float32)
    if e.sg is not None:
        sc = (_np(e.sg).astype(np.float64) / np.sqrt(_np(e.sv).astype(np.float64) + e.seps)).astype(np.float32)
        v = v * sc[cv]                                              # one fp32 multiply
    return np.where(valid, v, np.float32(0)).astype(np.float32)


def _bf16(x):
    u = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + (0x7FFF + ((u >> 16) & 1))) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), r)


def _bf16_to_f32(h):
    return (h.astype(np.uint32) << 16).view(np.float32)


def _perm(j):
    return 16 * ((j // 4) % 2) + 4 * (j // 8) + j % 4


def _conv(e):
    npad, kpad = e.Npad, e.Kpad
    if e.layout == L.REPACK_LAYOUT["f32"]:
        i = np.arange(npad * kpad, dtype=np.int64)
        return conv_value(e, i // kpad, i % kpad).view(np.uint8)
    name = e.layout_name
    two = name != "bf16"
    i = np.arange(npad * kpad * (2 if two else 1), dtype=np.int64)
    if name == "f16x3j":
        j, panel, n, k0 = i % 16, (i // 16) % 2, (i // 32) % npad, (i // 32) // npad * 16
    elif name == "f16x3i":
        j, panel, n, k0 = i % 32, (i // 32) % 2, (i // 64) % npad, (i // 64) // npad * 32
    elif name == "bf16":
        j, panel, n, k0 = _perm(i % 32), 0 * i, (i // 32) % npad, (i // 32) // npad * 32
    else:
        run = i // 32
        j, panel, n, k0 = _perm(i % 32), (run // npad) % 2, run % npad, run // (2 * npad) * 32
    m = conv_value(e, n, k0 + j)
    with np.errstate(over="ignore", invalid="ignore"):
        if name in ("bf16", "bf16x3"):
            hi = _bf16(m)
            lo = _bf16(m - _bf16_to_f32(hi))
            return np.where(panel == 0, hi, lo).astype(np.uint16).view(np.uint8)
        x = m * np.float32(64.0)
        hi = x.astype(np.float16)
        lo = (x - hi.astype(np.float32)).astype(np.float16)
        return np.where(panel == 0, hi.view(np.uint16), lo.view(np.uint16)).astype(np.uint16).view(np.uint8)


def wino_u(e):
    """U [P*P][N][C] in float64, summed in the kernel's order (before the one rounding)"""
    w = _np(e.src[0]).reshape(-1)
    o, c, q = np.meshgrid(np.arange(e.N), np.arange(e.C), np.arange(9), indexing="ij")
    g = w[e.off + o * e.sN + c * e.sC + q].astype(np.float64).reshape(e.N, e.C, 3, 3)
    G = np.asarray(e.G, np.float64).reshape(e.P, 3)
    u = np.zeros((e.P, e.P, e.N, e.C))
    for i in range(e.P):
        t = [(G[i, 0] * g[:, :, 0, k] + G[i, 1] * g[:, :, 1, k]) + G[i, 2] * g[:, :, 2, k] for k in range(3)]
        for l in range(e.P):
            u[i, l] = (t[0] * G[l, 0] + t[1] * G[l, 1]) + t[2] * G[l, 2]
    return u.reshape(e.P * e.P, e.N, e.C)


def _wino(e):
    out = np.zeros((e.P * e.P, e.Npad, e.Kpad), np.float32)
    out[:, :e.N, :e.C] = wino_u(e).astype(np.float32)
    return out.view(np.uint8).reshape(-1)


def _fold(e):
    out = np.full(e.Npad, e.pad, np.float32)
    g, b, m, v = (np.concatenate([_np(t).reshape(-1) for t in ts]).astype(np.float64) for ts in (e.src, e.beta, e.mean, e.var))
    eps = np.concatenate([np.full(t.numel(), x) for t, x in zip(e.var, e.eps)])
    root = np.sqrt(v + eps)
    scale = g / root
    out[:e.N] = {L.REPACK_SCALE: scale, L.REPACK_BIAS: b - m * scale, L.REPACK_RSTD: 1.0 / root, L.REPACK_MEAN: m}[e.layout].astype(np.float32)
    return out.view(np.uint8)


def _dw(e):
    u = np.arange(9 * e.N, dtype=np.int64)
    tap, c = u // e.N, u % e.N
    s, local = _src_of(e.rows, c)
    cat, base = _flat_sources(e.src)
    return cat[base[s] + local * 9 + tap].astype(np.float32).view(np.uint8)


def pack(e):
    """the bytes of `e.dst` after the kernel ran on entry `e`: uint8, flat"""
    if e.kind == L.REPACK_CONV:
        out = _conv(e)
    elif e.kind == L.REPACK_WINO:
        out = _wino(e)
    elif e.kind == L.REPACK_FOLD:
        out = _fold(e)
    elif e.kind == L.REPACK_DW:
        out = _dw(e)
    else:
        out = _np(e.src[0]).reshape(-1).astype(np.float32).view(np.uint8)
    out = np.ascontiguousarray(out).reshape(-1)
    assert out.size == e.nbytes
    return out


def raw(t):
    """the bytes of a tensor: uint8, flat"""
    return t.detach().contiguous().cpu().view(torch.uint8).reshape(-1).numpy()


def ulps(a, b):
    """distance of two float32 byte strings in units of the last place, elementwise"""
    x, y = (np.ascontiguousarray(v).view(np.int32).astype(np.int64) for v in (a, b))
    x, y = (np.where(v < 0, -(v & 0x7FFFFFFF), v) for v in (x, y))
    return np.abs(x - y)


# ------------------------------------------------------------------------------------------------------------- the cases
LAYOUTS = ("f32", "f32k32", "f16x3", "f16x3i", "f16x3j", "bf16", "bf16x3")
SHAPES_1X1 = ((1, 8), (20, 48), (64, 120), (256, 320))
SHAPES_3X3 = ((32, 32), (64, 64))


def _bn(c, g):
    bn = torch.nn.BatchNorm2d(c)
    with torch.no_grad():
        bn.weight.copy_(1.0 + 0.3 * torch.randn(c, generator=g))
        bn.bias.copy_(0.2 * torch.randn(c, generator=g))
        bn.running_mean.copy_(0.5 * torch.randn(c, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(c, generator=g))
    return bn


def _conv2d(cout, cin, k, g, groups=1, grid=False):
    conv = torch.nn.Conv2d(cin, cout, k, padding=k // 2, bias=False, groups=groups)
    with torch.no_grad():
        if grid:                # multiples of 2^-12 in [-1, 1]: every product and partial sum of the r = 2 transform is exact in double
            conv.weight.copy_(torch.randint(-4096, 4097, conv.weight.shape, generator=g).float() / 4096.0)
        else:
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * 0.1)
    return conv


def make_cases(device, seed=5):
    """(cache, mods, wino_exact): a store on `device` that holds, packed by the host packer, every kind and layout at the
    shapes of the issue; `mods` (id -> module) names every module in it; `wino_exact` = the keys of the Winograd entries
    whose weights lie on the 2^-12 grid (r = 2: byte-equal), the others are within one ulp."""
    from iip_uavsal_saliency_amd.model_feature import InvertedResidual
    g = torch.Generator().manual_seed(seed)
    built = []

    def keep(m):
        built.append(m)
        return m

    boxes = []
    for cout, cin in SHAPES_1X1:
        boxes.append(keep(torch.nn.Sequential(_conv2d(cout, cin, 1, g), _bn(cout, g))))
    for cout, cin in SHAPES_3X3:
        boxes.append(keep(torch.nn.Sequential(_conv2d(cout, cin, 3, g), _bn(cout, g))))
    grid = keep(torch.nn.Sequential(_conv2d(64, 64, 3, g, grid=True)))
    lstm = keep(torch.nn.Sequential(_conv2d(32, 64, 3, g)))                      # gate_interleave = 8, Cout = 32, a slice of 64 inputs
    side = keep(torch.nn.Sequential(torch.nn.Sequential(_conv2d(20, 48, 1, g), _bn(20, g)),
                                    torch.nn.Sequential(_conv2d(64, 48, 1, g), _bn(64, g))))
    dws = keep(torch.nn.Sequential(torch.nn.Sequential(_conv2d(24, 24, 3, g, groups=24), _bn(24, g)),
                                   torch.nn.Sequential(_conv2d(40, 40, 3, g, groups=40), _bn(40, g))))
    dot = keep(torch.nn.Sequential(_conv2d(48, 48, 3, g, groups=48), _bn(48, g), _conv2d(1, 48, 1, g), _bn(1, g)))
    blocks = [keep(InvertedResidual(24, 40, 1, 6)), keep(InvertedResidual(16, 16, 1, 1))]
    with torch.no_grad():
        for blk in blocks:
            for m in blk.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.running_mean.copy_(0.5 * torch.randn(m.running_mean.shape, generator=g))
                    m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))
                    m.weight.copy_(1.0 + 0.3 * torch.randn(m.weight.shape, generator=g))
    for m in built:
        m.to(device).eval()

    cache = WeightCache(device, {})
    wino_exact = set()
    for box in boxes:
        conv, bn = box[0], box[1]
        one = conv.kernel_size == (1, 1)
        for layout in LAYOUTS:
            if layout == "f16x3j" and not one:
                continue
            cache.conv(conv, None, 0, layout)
            cache.conv_t(conv, None, layout)
            if one:
                cache.conv_t_scaled(conv, bn, layout)
        cache.affine(bn, conv.out_channels)
        cache.bn_stats(bn)
        if not one:
            for r in (2, 4):
                cache.wino(conv, None, r)
    for layout in LAYOUTS:                                                          # a slice of the input channels
        cache.conv(boxes[3][0], (64, 192), 0, layout)                               # 1x1, 256 x 320 -> channels 64..192
        if layout != "f16x3j":
            cache.conv(boxes[5][0], (32, 64), 0, layout)                            # 3x3, 64 x 64 -> channels 32..64
            cache.conv_t(boxes[5][0], (32, 64), layout)
            cache.conv(lstm[0], (32, 64), 8, layout)
            cache.conv(grid[0], None, 0, layout)
        cache.conv([side[0][0], side[1][0]], None, 0, layout)
    cache.affine([side[0][1], side[1][1]], 84)
    cache.wino(boxes[5][0], (32, 64), 4)
    cache.wino(lstm[0], (0, 32), 2)
    cache.wino(grid[0], None, 2)                    # (r = 2 alone: at r = 4 the grid makes sums that cancel to 0 exactly, where the
    wino_exact.add(("wino", id(grid[0]), None, 2))  # order of summation decides between 0 and 1e-17 and no ulp bound holds)
    cache.depthwise(dws[0][0], dws[0][1])
    cache.depthwise([dws[0][0], dws[1][0]], [dws[0][1], dws[1][1]])
    cache.dw_dot(dot[0], dot[1], dot[2], dot[3])
    for blk in blocks:
        cache.fused_block(blk, True)
    mods = {id(s): s for m in built for s in m.modules()}
    return cache, mods, wino_exact
