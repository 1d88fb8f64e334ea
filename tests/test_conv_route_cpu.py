"""The GEMM route (uavsal_conv_route: kernel family, tile, K shares per tile) through the library's real query, no device.

The route is what `uavsal_conv_gemm` switches on, so what is pinned here is what launches: `PINNED` holds the descriptors of
the K-split kernel tests (tests/test_hip_kernels.py) with the family, tile and shares their launches took BEFORE the route
existed in one place (read from launchers that printed their decision); the plan tests hold the four older single-field
queries to the route for every conv descriptor of a recorded plan.  The stream-K grid is not pinned: it depends on the
occupancy query, which has no device here."""
import ctypes as C

import pytest

from iip_uavsal_saliency_amd import _lib as L

PTR = 1 << 20       # a dummy device address with the alignment of a real allocation


def desc(n, h, w, cin, cout, taps=1, prec="f32", act=L.ACT_NONE, twa=False, tile=0, res=False, ws=True, dw=False):
    """The descriptor ops.conv_gemm / ops.twa_step fill for these arguments (dense NHWC tensors, `ws`: stream_k=True)."""
    d = L.ConvDesc()
    d.a, d.lda, d.a_img_stride = PTR, cin, h * w
    d.w, d.out, d.ldc, d.o_img_stride = PTR, PTR, cout, h * w
    if twa:
        d.res, d.ldr, d.r_img_stride, d.aux, d.ldx, d.x_img_stride = PTR, cout, h * w, PTR, cout, h * w
    else:
        d.scale, d.bias = PTR, PTR
        if res:
            d.res, d.ldr, d.r_img_stride = PTR, cout, h * w
    if dw:
        d.dw_w9c, d.dw_scale, d.dw_bias, d.dw_stride, d.dw_Hin, d.dw_Win = PTR, PTR, PTR, 1, h, w
    d.n_img, d.H, d.W, d.Cin, d.Cout, d.taps = n, h, w, cin, cout, taps
    d.prec, d.act, d.epi, d.tile = L.PREC[prec], act, (L.EPI_TWA if twa else L.EPI_AFFINE), tile
    if ws:
        d.sk_ws, d.sk_ws_bytes = PTR, int(L.load().uavsal_streamk_workspace_bytes())
    return d


TWA = dict(cin=256, cout=256, taps=9, twa=True)
# (case, descriptor arguments, family, tile, K shares, where the shares meet)
PINNED = [
    # test_twa_step_f32_full_line_split_k: forced tiles 8 / 10 / 11 and the automatic choice
    ("twa-f32-45x80-t8", dict(n=1, h=45, w=80, tile=8, **TWA), L.ROUTE_K32, 8, 4, L.REDUCE_LAUNCH),
    ("twa-f32-45x80-t10", dict(n=1, h=45, w=80, tile=10, **TWA), L.ROUTE_K32, 10, 4, L.REDUCE_IN_LAUNCH),
    ("twa-f32-45x80-t11", dict(n=1, h=45, w=80, tile=11, **TWA), L.ROUTE_K32, 11, 4, L.REDUCE_IN_LAUNCH),
    ("twa-f32-45x80-auto", dict(n=1, h=45, w=80, **TWA), L.ROUTE_K32, 8, 4, L.REDUCE_LAUNCH),
    ("twa-f32-3x9x13-t8", dict(n=3, h=9, w=13, tile=8, **TWA), L.ROUTE_K32, 8, 4, L.REDUCE_LAUNCH),
    # test_conv_f32_full_line_split_k
    ("aspp-f32-t8", dict(n=2, h=12, w=20, cin=1920, cout=256, act=1, res=True, tile=8), L.ROUTE_K32, 8, 4, L.REDUCE_LAUNCH),
    ("conv3-f32-t10", dict(n=2, h=12, w=20, cin=256, cout=256, taps=9, act=1, res=True, tile=10), L.ROUTE_K32, 10, 4,
     L.REDUCE_IN_LAUNCH),
    ("tail-f32-t11", dict(n=1, h=23, w=40, cin=960, cout=160, tile=11), L.ROUTE_K32, 11, 4, L.REDUCE_IN_LAUNCH),
    # test_twa_step_split_k, test_conv1x1_small_map_split_k, test_conv1x1_split_k_ragged, test_conv3x3_small_map_split_k
    ("twa-f16x3-45x80", dict(n=1, h=45, w=80, prec="f16x3", **TWA), L.ROUTE_STAGED, 4, 4, L.REDUCE_LAUNCH),
    ("aspp-f16x3-t4", dict(n=2, h=12, w=20, cin=1920, cout=256, prec="f16x3", res=True, tile=4), L.ROUTE_STAGED, 4, 4,
     L.REDUCE_LAUNCH),
    ("ragged-f16x3-t4", dict(n=1, h=7, w=9, cin=768, cout=36, prec="f16x3", act=1, tile=4), L.ROUTE_STAGED, 4, 2, L.REDUCE_LAUNCH),
    ("conv3-f16x3-t4", dict(n=2, h=23, w=40, cin=64, cout=64, taps=9, prec="f16x3", act=1, res=True, tile=4), L.ROUTE_STAGED, 4,
     1, L.REDUCE_NONE),
    # test_depthwise_projection_lds_halo, the narrow-output cases (ops.conv_gemm hands every dw= launch the workspace)
    ("dwproj-f32-768-1", dict(n=1, h=16, w=32, cin=768, cout=1, act=2, dw=True), L.ROUTE_DWPROJ, 3, 4, L.REDUCE_LAUNCH),
    ("dwproj-f16x3-384-40", dict(n=2, h=9, w=20, cin=384, cout=40, prec="f16x3", act=1, res=True, dw=True), L.ROUTE_DWPROJ, 4,
     1, L.REDUCE_NONE),
]


@pytest.mark.parametrize("case", PINNED, ids=[c[0] for c in PINNED])
def test_route_of_the_k_split_kernel_tests(case):
    _, kw, family, tile, ksplit, reduce = case
    r = L.conv_route(L.load(), desc(**kw))
    assert (r.family, r.tile, r.ksplit, r.reduce) == (family, tile, ksplit, reduce), r


def _plan_descs(cfg):
    import mock_plan
    import plan_census
    m, wcache = plan_census.model_for(cfg)
    _, mock = mock_plan.record(m, wcache=wcache, **plan_census.engine_kwargs(m, cfg))
    return [a for name, a in mock.calls if name == "uavsal_plan_add_conv"]


@pytest.mark.parametrize("cfg", [0, 5], ids=["BASE[0]-f32", "BASE[5]-f16x3-split-mode"])
def test_old_queries_are_fields_of_the_route(cfg):
    """Every conv descriptor a plan hands the library: the four single-field queries answer what the route holds, a second
    query gives the same route, and every family the precision has occurs (so the comparison is not vacuous)."""
    import plan_census
    lib = L.load()
    assert plan_census.BASE[5][4] == "f16x3" and plan_census.BASE[5][0] >= 4         # (split mode: f16x3 from four clips on)
    descs = _plan_descs(plan_census.BASE[cfg])
    assert len(descs) >= 40
    seen = set()
    for d in descs:
        r = L.conv_route(lib, d)
        assert r == L.conv_route(lib, d)
        assert int(lib.uavsal_conv_tile(C.byref(d))) == r.tile and 1 <= r.tile <= 11
        assert int(lib.uavsal_conv_uses_split(C.byref(d))) == (r.family == L.ROUTE_PRESPLIT)
        assert int(lib.uavsal_conv_dwproj(C.byref(d))) == r.dwproj and (r.dwproj != 0) == (r.family == L.ROUTE_DWPROJ)
        assert int(lib.uavsal_conv_streamk_grid(C.byref(d))) == r.streamk and (r.streamk != 0) == (r.family == L.ROUTE_STREAMK)
        assert r.ksplit >= 1 and (r.ksplit > 1) == (r.reduce != L.REDUCE_NONE)
        seen.add(r.family)
    want = {L.ROUTE_DWPROJ, L.ROUTE_K32} if cfg == 0 else {L.ROUTE_PRESPLIT, L.ROUTE_DWPROJ, L.ROUTE_STAGED}
    assert want <= seen, seen


def test_route_query_rejects_what_has_no_route():
    lib = L.load()
    d = desc(1, 45, 80, 256, 256)
    assert lib.uavsal_conv_route_of(C.byref(d), None) == -1
    d.Cout = 0
    assert lib.uavsal_conv_route_of(C.byref(d), C.byref(L.ConvRoute())) == -1
    assert lib.uavsal_conv_tile(C.byref(d)) == -1 and lib.uavsal_conv_uses_split(C.byref(d)) == 0
