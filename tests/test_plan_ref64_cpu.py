"""CPU checks of the yardstick of tests/test_plan_ops_fp64.py: the float64 references of tests/plan_ref64.py against the torch
modules of oracle/uavsal_ref.py and F.conv2d, their error bounds against real fp32 arithmetic (and the wrong references they
must reject), and engine.read_view on strided NHWC views, channel slices and split shadows."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import plan_ref64 as R
from iip_uavsal_saliency_amd import engine as E
from oracle import uavsal_ref as O


def _rand_bn(bn, g):
    c = bn.num_features
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(c, generator=g) * 0.5)
        bn.running_mean.copy_(torch.randn(c, generator=g) * 0.2)
        bn.running_var.copy_(torch.rand(c, generator=g) + 0.5)
    return bn


def _init(mod, seed=0):
    g = torch.Generator().manual_seed(seed)
    for m in mod.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            _rand_bn(m, g)
        elif isinstance(m, torch.nn.Conv2d):
            with torch.no_grad():
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / (m.weight[0].numel() ** 0.5))
    return mod.eval()


def _x(shape, seed=1, lo=None):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return x.clamp(min=lo) if lo is not None else x


def _close(a, b, tol=1e-11):
    assert (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


def _within(y32, ref):
    ratio = ((y32.double() - ref.y).abs() / R.bound(ref)).max().item()
    assert ratio <= 1.0, ratio
    return ratio


@pytest.mark.parametrize("r", [2, 4])
@pytest.mark.parametrize("hw", [(8, 8), (9, 13), (5, 7)])
def test_winograd_transforms_are_the_direct_conv(r, hw):
    """The signed transform matrices whose absolute values make the Winograd bound reproduce F.conv2d exactly (G as packed)."""
    x, w = _x((2, 6) + hw), _x((5, 6, 3, 3), 2)
    _close(R.wino_conv(x, w, r), F.conv2d(x, w, padding=1))
    assert bool((R.wino_conv(x, w, r, absolute=True) >= F.conv2d(x.abs(), w.abs(), padding=1) * (1 - 1e-12)).all())


@pytest.mark.parametrize("cin,cout,stride,expand", [(16, 24, 2, 6), (24, 24, 1, 6), (32, 16, 1, 1)])
def test_fused_ir_reference_is_the_oracle_block(cin, cout, stride, expand):
    blk = _init(O._IRBlock(cin, cout, stride, expand)).double()
    wrap = SimpleNamespace(conv=blk.conv, expand_ratio=expand, stride=stride, use_res_connect=blk.residual)
    x = _x((2, cin, 11, 13))
    ref = R.ref_fused_ir({"blk": wrap}, x)
    _close(ref.y, blk(x))
    _within(blk.float()(x.float()), ref)
    blk.double()
    for m in ("chan", "row", "bias"):       # the wrong references are rejected by the fp32 result too
        assert ((blk.float()(x.float()).double() - R.ref_fused_ir({"blk": wrap}, x, mut=m).y).abs() / R.bound(ref)).max() > 1
        blk.double()


@pytest.mark.parametrize("taps", [1, 9])
def test_conv_affine_with_residual_and_mutations(taps):
    cbr = _init(O._cbr(64, 48, 3 if taps == 9 else 1))
    x, res = _x((2, 64, 9, 12), 3, lo=0.0), _x((2, 48, 9, 12), 4)
    rec = dict(conv=cbr[0], bn=cbr[1], act=R.ACT_RELU6, epi=R.EPI_AFFINE, taps=taps, prec="f32", dw=None, n_group=0)
    ref = R.ref_conv(rec, x, res=res)
    _close(ref.y, cbr.double()(x) + res)
    y32 = cbr.float()(x.float()) + res.float()
    _within(y32, ref)
    for m in ("chan", "bias") + (("row",) if taps == 9 else ()):
        assert ((y32.double() - R.ref_conv(rec, x, res=res, mut=m).y).abs() / R.bound(ref)).max() > 1, m


def test_conv_n_group_and_fused_depthwise():
    g = torch.Generator().manual_seed(5)
    pls = [_init(torch.nn.Conv2d(64, 64, 1, bias=False), i) for i in range(3)]
    bns = [_rand_bn(torch.nn.BatchNorm2d(64), g).eval() for _ in range(3)]
    x = _x((1, 192, 5, 6), 6)
    rec = dict(conv=pls, bn=bns, act=R.ACT_NONE, epi=R.EPI_AFFINE, taps=1, prec="f32", dw=None, n_group=64, cin=64)
    want = torch.cat([bns[i].double()(F.conv2d(x[:, 64 * i:64 * (i + 1)], pls[i].weight.double())) for i in range(3)], 1)
    _close(R.ref_conv(rec, x).y, want)
    dwc = _init(O._cbr(32, 32, 3, 2, groups=32))
    pl, plbn = _init(torch.nn.Conv2d(32, 16, 1, bias=False)), _rand_bn(torch.nn.BatchNorm2d(16), g).eval()
    rec = dict(conv=pl, bn=plbn, act=R.ACT_NONE, epi=R.EPI_AFFINE, taps=1, prec="f16x3", dw=(dwc[0], dwc[1], 2), n_group=0)
    e = _x((2, 32, 9, 11), 7, lo=0.0)
    _close(R.ref_conv(rec, e).y, plbn.double()(pl.double()(dwc.double()(e))))


def test_twa_and_lstm_epilogues_are_the_oracle_cells():
    hid = 8
    cell = _init(O._TWACell(hid, hid)).double()
    xt, h = _x((2, hid, 6, 7), 8), _x((2, hid, 6, 7), 9)
    w = cell.rnn_conv.weight
    pre = F.conv2d(xt, w[:, :hid], padding=1)
    rec = dict(conv=cell.rnn_conv, bn=None, act=R.ACT_NONE, epi=R.EPI_TWA, taps=9, prec="f32", wslice=(hid, 2 * hid), dw=None,
               n_group=0)
    ref = R.ref_conv(rec, h, res=xt, aux=pre)
    _close(ref.y, cell(xt, h))
    _within(cell.float()(xt.float(), h.float()), ref)
    cell.double()
    for r in (2, 4):
        refw = R.ref_wino(dict(conv=cell.rnn_conv, bn=None, act=R.ACT_NONE, wslice=(hid, 2 * hid), r=r), h, twa=(xt, pre))
        _close(refw.y, cell(xt, h))
        assert bool((refw.B >= ref.B * (1 - 1e-12)).all())          # the Winograd chain's error scale is never below the direct one
    conv = torch.nn.Conv2d(2 * hid, 4 * hid, 3, padding=1, bias=False)
    _init(conv)
    c = _x((2, hid, 6, 7), 10)
    wd = conv.weight.double()
    wi = wd[:, :hid].reshape(4, hid, hid, 3, 3).permute(1, 0, 2, 3, 4).reshape(4 * hid, hid, 3, 3)
    pre = F.conv2d(xt, wi, padding=1)
    rec = dict(conv=conv, bn=None, act=R.ACT_NONE, epi=R.EPI_LSTM, taps=9, prec="f32", wslice=(hid, 2 * hid), gate_interleave=hid,
               dw=None, n_group=0)
    ref = R.ref_conv(rec, h, res=c, aux=pre)
    h1, c1 = O.convlstm_cell_step(wd, xt, h, c)
    _close(ref.y, torch.cat([h1, c1], 1))


def test_depthwise_dilation_groups_stem_bilinear_tdiff_tsum():
    dws = [_init(O._cbr(16, 16, 3, 1, d, groups=16), i) for i, d in enumerate((6, 12, 18))]
    x = _x((1, 48, 20, 23), 11)
    rec = dict(conv=[m[0] for m in dws], bn=[m[1] for m in dws], stride=1, dilation=(6, 12, 18))
    want = torch.cat([dws[i].double()(x[:, 16 * i:16 * (i + 1)]) for i in range(3)], 1)
    _close(R.ref_dw(rec, x).y, want)
    dw2 = _init(O._cbr(16, 16, 3, 2, groups=16))
    _close(R.ref_dw(dict(conv=dw2[0], bn=dw2[1], stride=2, dilation=1), x[:, :16]).y, dw2.double()(x[:, :16]))
    stem = _init(O._cbr(3, 32, 3, 2))
    u8 = torch.randint(0, 256, (2, 3, 15, 17), generator=torch.Generator().manual_seed(12)).double()
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    xn = (u8 / 255 - torch.tensor(mean, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(std, dtype=torch.float64).view(1, 3, 1, 1)
    rec = dict(conv=stem[0], bn=stem[1], u8=True, mean=mean, stdv=std)
    _close(R.ref_stem(rec, u8).y, stem.double()(xn))
    small = _x((3, 5, 4, 6), 13)
    y, B, X = R.bilinear_ac(small, 9, 13, [2, 0, 1, 2])
    _close(y, F.interpolate(small[[2, 0, 1, 2]], size=(9, 13), mode="bilinear", align_corners=True))
    assert R.bilinear_src(8, 2, 1) == [0, 1, 0, 1, 0, 1, 0, 1] and R.bilinear_src(8, 8, 4) == [0, 0, 0, 0, 1, 1, 1, 1]
    seq = _x((6, 4, 3, 3), 14)
    got = R.ref_tdiff(seq, 3).y
    _close(got, torch.cat([O.temporal_differences(seq[:3]), O.temporal_differences(seq[3:])]))
    _close(R.ref_tsum(seq, 3).y, torch.stack([seq[:3].sum(0), seq[3:].sum(0)]))


def _shadow(buf, ld):
    """Split shadow of an fp32 NHWC buffer [pixels * ld]: [pixel][ld/32][hi 32 | lo 32] of 16 x (round-to-zero not needed here)."""
    v = 16.0 * buf.view(-1, ld // 32, 1, 32)
    hi = v.half()
    lo = (v - hi.float()).half()
    return torch.cat([hi, lo], 2).reshape(-1)


def test_read_view_strides_slices_and_shadow():
    n, h, w, ld = 6, 3, 5, 96
    buf = torch.randn(n * h * w * ld, generator=torch.Generator().manual_seed(15))
    nhwc = buf.view(n, h, w, ld)
    sp = _shadow(buf, ld)
    # frames 1, 3, 5 (frame stride 2 images) of channels [32, 96): the recurrence's view of one step over three clips
    d = E.OpView(buf, 1 * h * w * ld + 32, 3, h, w, 64, ld, 2 * h * w, sp, 1 * h * w * 2 * ld + 64)
    want = nhwc[1::2, :, :, 32:96].permute(0, 3, 1, 2).double()
    assert torch.equal(E.read_view(None, d), want)
    assert torch.equal(E.read_view(None, d, images=[2, 0]), want[[2, 0]])
    merged = E.read_view(None, d, shadow=True)
    assert (merged - want).abs().max().item() <= 2 ** -20 * want.abs().max().item()
    # an engine view (V) with a channel offset and a shadow: OpView.of computes the shadow offset as V.sp_ptr does
    v = E.V(buf, n, h, w, 64, ld=ld, coff=32, sp=sp).frames(2, 2)
    od = E.OpView.of(v)
    assert od.sp_off * 2 == v.sp_ptr - sp.data_ptr()
    assert torch.equal(E.read_view(None, od), nhwc[2:4, :, :, 32:96].permute(0, 3, 1, 2).double())
    # an odd channel slice without a shadow, and the NCHW side of a layout op
    d2 = E.OpView(buf, 5, n, h, w, 7, ld, h * w)
    assert torch.equal(E.read_view(None, d2), nhwc[..., 5:12].permute(0, 3, 1, 2).double())
    nchw = E.OpView(buf, 10, 2, h, w, 4, 4, 0, nchw=True)
    assert torch.equal(E.read_view(None, nchw), buf[10:10 + 2 * 4 * h * w].view(2, 4, h, w).double())


def _operands(rec):
    out = [rec.get(k) for k in ("a", "out", "res", "aux", "out2")]
    out += list(rec.get("segs") or ()) + list(rec.get("twa") or ())
    return [d for d in out if d is not None]


@pytest.mark.parametrize("kw", [dict(n_seq=1, seq_len=4, ctx_mode="tile"),
                                dict(n_seq=2, seq_len=4, ctx_mode="clip", persistent=True),
                                dict(n_seq=4, seq_len=4, ctx_mode="clip", precision="f16x3"),
                                dict(n_seq=1, seq_len=4, ctx_mode="clip", static_priors=True, lstm=True)],
                         ids=["tile", "persistent", "f16x3", "static-lstm"])
def test_op_args_cover_the_recorded_plan(kw):
    """Engine.op_args on a plan recorded on the CPU (tests/mock_plan.py): one entry per native op, every launch but sync / poison /
    guard carries its operands (a Winograd triple's on its output transform), and every operand view lies inside its buffer
    (read_view of it works: as_strided refuses a view past the storage)."""
    import mock_plan
    from iip_uavsal_saliency_amd.model import UAVSal, UAVSAL_LSTM
    kw = dict(kw)
    m = (UAVSAL_LSTM if kw.pop("lstm", False) else UAVSal)(time_dims=4).eval()
    m.arena_debug = True
    eng, mock = mock_plan.record(m, H=96, W=160, ctx_T=4, **kw)
    assert len(eng.op_args) == len(eng.ops_meta) == mock.n
    assert [r["name"] for r in eng.op_args] == [mt["name"] for mt in eng.ops_meta]
    eng._bound_t = {k: torch.zeros(t.shape, dtype=t.dtype) for k, t in (
        ("x", eng.x_in), ("cb0", eng.cb0_in), ("cb1", eng.cb1_in), ("out", eng.out), ("state_in", eng.state_in),
        ("state_out", eng.state_out), ("cstate_in", eng.cstate_in), ("cstate_out", eng.cstate_out))}
    kinds = set()
    for i, rec in enumerate(eng.op_args):
        if rec["kind"] in ("sync", "poison", "guard"):
            continue
        if "triple" in rec:
            assert eng.op_args[eng._op_idx[rec["triple"]]]["kind"] == "wino" and eng._op_idx[rec["triple"]] > i
            continue
        kinds.add(rec["kind"])
        ds = _operands(rec)
        assert ds and "out" in rec, rec["name"]
        for d in ds:
            if d.buf is not None:
                E.read_view(eng, d, images=[0, d.n - 1])
            if d.sp is not None:
                E.read_view(eng, d, shadow=True, images=[0, d.n - 1])
    assert kinds >= {"stem", "fused_ir", "conv1", "dw", "dw_dot", "bilinear", "tdiff", "layout"}
