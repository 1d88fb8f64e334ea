"""uavsal_wino_seam against the two launches it replaces -- uavsal_wino_output (EPI_TWA) followed by uavsal_wino_input -- bit for
bit, through ctypes, at the map sizes where its 8x8 blocks, their one-pixel ring and the 2x2 tiles can go wrong; the zero-h
forms against the full launches on an all-zero state; and every refusal."""
import ctypes as C

import pytest
import torch

from iip_uavsal_saliency_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LQ = 3                       # frames in the history: the step under test writes frame 1
SHAPES = [(1, 1), (2, 2), (5, 7), (8, 8), (9, 13), (16, 24), (45, 80)]
CHANNELS = [4, 32, 64, 96, 256]
SENTINEL = 7.0


def _case(H, W, Cc, n_img, h_in_history, seed=0, zero_h=False):
    """Buffers of one step: history [n_img, LQ, H*W, C], x / pre the same, h0 [n_img, H*W, C], M / V [16, Mp, C]."""
    g = torch.Generator().manual_seed(seed * 1000 + H * 100 + W)
    rnd = lambda *s: torch.randn(*s, generator=g).to(DEV)
    hw = H * W
    tiles = n_img * ((H + 1) // 2) * ((W + 1) // 2)
    mp = (tiles + 127) // 128 * 128
    b = dict(hist=rnd(n_img, LQ, hw, Cc), x=rnd(n_img, LQ, hw, Cc), pre=rnd(n_img, LQ, hw, Cc), h0=rnd(n_img, hw, Cc),
             M=rnd(16, mp, Cc), V=torch.full((16, mp, Cc), SENTINEL, device=DEV))
    if zero_h:
        b["M"].zero_(); b["h0"].zero_(); b["hist"][:, 0].zero_()
    frame = lambda t, f: t.data_ptr() + 4 * f * hw * Cc
    wo = L.WinoDesc()
    wo.inp, wo.ldi = b["M"].data_ptr(), Cc
    wo.out, wo.ldo, wo.out_img_stride = frame(b["hist"], 1), Cc, LQ * hw
    wo.n_img, wo.H, wo.W, wo.C, wo.Mp, wo.R = n_img, H, W, Cc, mp, 2
    wo.act, wo.epi = L.ACT_NONE, L.EPI_TWA
    wo.res, wo.ldr, wo.res_img_stride = frame(b["x"], 1), Cc, LQ * hw
    wo.aux, wo.ldx, wo.aux_img_stride = frame(b["pre"], 1), Cc, LQ * hw
    if h_in_history:
        wo.hprev, wo.ldh, wo.h_img_stride = frame(b["hist"], 0), Cc, LQ * hw
    else:
        wo.hprev, wo.ldh, wo.h_img_stride = b["h0"].data_ptr(), Cc, hw
    wi = L.WinoDesc()
    wi.inp, wi.ldi, wi.in_img_stride = frame(b["hist"], 1), Cc, LQ * hw
    wi.out, wi.ldo = b["V"].data_ptr(), Cc
    wi.n_img, wi.H, wi.W, wi.C, wi.Mp, wi.R = n_img, H, W, Cc, mp, 2
    return b, wo, wi


def _bits(t):
    return t.view(torch.int32)


def _two_launches(lib, wo, wi, s):
    L.check(lib.uavsal_wino_output(C.byref(wo), s), "wino_output")
    L.check(lib.uavsal_wino_input(C.byref(wi), s), "wino_input")


@pytest.mark.parametrize("H,W", SHAPES)
def test_seam_equals_the_two_launches(H, W):
    """h_t and the V planes, every channel count and image count, both forms of `hprev` (the state buffer, image stride hw,
    and the previous frame of the history, image stride L * hw).  The whole buffers are compared: what the two launches
    leave alone -- other frames of the history, V rows past the real tiles -- the seam launch leaves alone too."""
    lib = L.load()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for Cc in CHANNELS:
        for n_img in (1, 3):
            for in_hist in (False, True):
                ref, wo, wi = _case(H, W, Cc, n_img, in_hist)
                _two_launches(lib, wo, wi, s)
                got, so, si = _case(H, W, Cc, n_img, in_hist)
                L.check(lib.uavsal_wino_seam(C.byref(so), C.byref(si), s), "wino_seam")
                torch.cuda.synchronize()
                what = (H, W, Cc, n_img, in_hist)
                assert torch.equal(_bits(got["hist"]), _bits(ref["hist"])), what
                assert torch.equal(_bits(got["V"]), _bits(ref["V"])), what
                tiles = n_img * ((H + 1) // 2) * ((W + 1) // 2)
                assert bool((ref["V"][:, tiles:] == SENTINEL).all()) and not bool((ref["V"][:, :tiles] == SENTINEL).all())


@pytest.mark.parametrize("H,W", [(5, 7), (9, 13), (45, 80)])
def test_zero_h_forms_equal_the_full_launches_on_a_zero_state(H, W):
    """M = +0 (what the step GEMM makes of V = +0) and h_{t-1} = +0: uavsal_wino_output_zero_h and uavsal_wino_seam_zero_h,
    which load neither, write the bits of the full launches."""
    lib = L.load()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for Cc in (4, 96, 256):
        for n_img in (1, 3):
            ref, wo, wi = _case(H, W, Cc, n_img, False, zero_h=True)
            _two_launches(lib, wo, wi, s)
            a, ao, ai = _case(H, W, Cc, n_img, False, zero_h=True)
            L.check(lib.uavsal_wino_output_zero_h(C.byref(ao), s), "wino_output_zero_h")
            b, bo, bi = _case(H, W, Cc, n_img, False, zero_h=True)
            b["M"].fill_(float("nan")); b["h0"].fill_(float("nan"))          # (never loaded)
            L.check(lib.uavsal_wino_seam_zero_h(C.byref(bo), C.byref(bi), s), "wino_seam_zero_h")
            torch.cuda.synchronize()
            assert torch.equal(_bits(a["hist"]), _bits(ref["hist"])), (H, W, Cc, n_img)
            assert torch.equal(_bits(b["hist"]), _bits(ref["hist"])), (H, W, Cc, n_img)
            assert torch.equal(_bits(b["V"]), _bits(ref["V"])), (H, W, Cc, n_img)


def test_refusals_launch_nothing():
    lib = L.load()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    H, W, Cc, n = 9, 13, 32, 2
    ESHAPE, EALIGN = -3, -2

    def refused(edit, status):
        b, wo, wi = _case(H, W, Cc, n, True)
        keep = {k: v.clone() for k, v in b.items()}
        edit(b, wo, wi)
        assert lib.uavsal_wino_seam_check(C.byref(wo), C.byref(wi)) == status
        assert lib.uavsal_wino_seam(C.byref(wo), C.byref(wi), s) == status
        assert lib.uavsal_wino_seam_zero_h(C.byref(wo), C.byref(wi), s) == status
        torch.cuda.synchronize()
        for k in ("hist", "V"):
            assert torch.equal(_bits(b[k]), _bits(keep[k])), k

    def not_the_next_input(b, wo, wi):
        wi.inp = b["hist"].data_ptr()                       # reads frame 0, not the frame the output transform writes

    def other_stride(b, wo, wi):
        wi.in_img_stride = H * W

    def other_shape(b, wo, wi):
        wi.H, wi.W = W, H

    def other_channels(b, wo, wi):
        wi.C = Cc - 4

    def c_not_a_quad(b, wo, wi):
        wo.C = wi.C = Cc - 2

    def r4(b, wo, wi):
        wo.R = wi.R = 4

    def affine(b, wo, wi):
        wo.epi = L.EPI_AFFINE

    for edit, status in ((not_the_next_input, ESHAPE), (other_stride, ESHAPE), (other_shape, ESHAPE), (other_channels, ESHAPE),
                         (c_not_a_quad, EALIGN), (r4, ESHAPE), (affine, ESHAPE)):
        refused(edit, status)
    # and the unedited pair is taken
    b, wo, wi = _case(H, W, Cc, n, True)
    assert lib.uavsal_wino_seam_check(C.byref(wo), C.byref(wi)) == 0
