"""ctypes binding of libuavsal_hip.so (C ABI: include/uavsal_hip.h).

The product path has no CPU fallback: if the shared library is missing or a
launch fails, a RuntimeError is raised.
"""
from __future__ import annotations

import collections
import ctypes as C
import os

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("UAVSAL_HIP_LIB") or os.path.join(PKG, "libuavsal_hip.so")   # override: A/B builds

PREC = {"f32": 0, "bf16x3": 1, "bf16": 2, "f16x3": 3}
ACT_NONE, ACT_RELU6, ACT_SIGMOID = 0, 1, 2
EPI_AFFINE, EPI_TWA, EPI_LSTM = 0, 1, 2
SK_TICKET_BASE = 4096      # words of stream-K flags in front of the K-split ticket counters (csrc/conv_gemm_common.h)

_ERR = {-1: "UAVSAL_EINVAL (null pointer / non-positive size)",
        -2: "UAVSAL_EALIGN (channel count / ld / pointer not 16-byte aligned)",
        -3: "UAVSAL_ESHAPE (shape not supported by the kernel)",
        -4: "UAVSAL_ESTATE (plan used in the wrong state)",
        -5: "UAVSAL_EDEVICE (a kernel reported a device-side error; the run's outputs are invalid)"}
ERR_STREAMK = 1
DW_KERNEL = {1: "dw3x3_kernel<1, 4, 4>", 2: "dw3x3_kernel<1, 2, 2>", 3: "dw3x3_kernel<2, 2, 2>", 4: "dw3x3_dilated_kernel",
             16: "dw3x3_map_lds_kernel<16, 256>", 32: "dw3x3_map_lds_kernel<32, 256>",
             528: "dw3x3_map_lds_kernel<16, 512>", 544: "dw3x3_map_lds_kernel<32, 512>",
             2048: "dw3x3_rowclass_kernel<256>"}

_f = C.c_void_p   # device pointers travel as integers


class ConvDesc(C.Structure):
    _fields_ = [("a", _f), ("lda", C.c_int32), ("a_img_stride", C.c_int64),
                ("w", _f), ("scale", _f), ("bias", _f),
                ("out", _f), ("ldc", C.c_int32), ("o_img_stride", C.c_int64),
                ("res", _f), ("ldr", C.c_int32), ("r_img_stride", C.c_int64),
                ("aux", _f), ("ldx", C.c_int32), ("x_img_stride", C.c_int64),
                ("n_img", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("Cin", C.c_int32), ("Cout", C.c_int32), ("taps", C.c_int32),
                ("prec", C.c_int32), ("act", C.c_int32), ("epi", C.c_int32), ("tile", C.c_int32),
                ("out2", _f), ("ld2", C.c_int32),
                ("dw_w9c", _f), ("dw_scale", _f), ("dw_bias", _f),
                ("dw_stride", C.c_int32), ("dw_Hin", C.c_int32), ("dw_Win", C.c_int32),
                ("sk_ws", _f), ("sk_ws_bytes", C.c_int64),
                ("a_split", _f), ("ldas", C.c_int32),
                ("out_split", _f), ("ldos", C.c_int32),
                ("err", _f), ("sk_spin_limit", C.c_int32), ("sk_debug_drop", C.c_int32),
                ("w_group_stride", C.c_int64), ("n_group", C.c_int32), ("a_group_off", C.c_int32)]


ROUTE_PRESPLIT, ROUTE_DWPROJ, ROUTE_STREAMK, ROUTE_K32, ROUTE_F32_DMA, ROUTE_STAGED = 1, 2, 3, 4, 5, 6
REDUCE_NONE, REDUCE_LAUNCH, REDUCE_IN_LAUNCH = 0, 1, 2


class ConvRoute(C.Structure):
    """uavsal_conv_route: what uavsal_conv_gemm runs for a descriptor (include/uavsal_hip.h)."""
    _fields_ = [("family", C.c_int32), ("tile", C.c_int32), ("dwproj", C.c_int32), ("streamk", C.c_int32),
                ("ksplit", C.c_int32), ("reduce", C.c_int32)]


Route = collections.namedtuple("Route", [f for f, _ in ConvRoute._fields_])


def conv_route(lib, d: ConvDesc) -> Route:
    """The route of `d`, asked once (no launch; pointers may be dummies with the real alignment)."""
    r = ConvRoute()
    check(lib.uavsal_conv_route_of(C.byref(d), C.byref(r)), "uavsal_conv_route_of")
    return Route(*(int(getattr(r, f)) for f in Route._fields))


class DwDesc(C.Structure):
    _fields_ = [("inp", _f), ("ldi", C.c_int32), ("w9c", _f), ("scale", _f), ("bias", _f),
                ("out", _f), ("ldo", C.c_int32),
                ("n_img", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32),
                ("stride", C.c_int32), ("dilation", C.c_int32), ("act", C.c_int32),
                ("out_split", _f), ("ldos", C.c_int32), ("dil_group_c", C.c_int32), ("dil_groups", C.c_int32 * 4)]


class DwDotDesc(C.Structure):
    _fields_ = [("inp", _f), ("ldi", C.c_int32), ("w9c", _f), ("scale", _f), ("bias", _f),
                ("w2", _f), ("scale2", _f), ("bias2", _f), ("out", _f), ("ldo", C.c_int32),
                ("n_img", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("act", C.c_int32)]


class StemDesc(C.Structure):
    _fields_ = [("inp", _f), ("in_u8", _f), ("w", _f), ("scale", _f), ("bias", _f),
                ("out", _f), ("ldo", C.c_int32),
                ("n_img", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("mean", C.c_float * 3), ("stdv", C.c_float * 3)]


class BilinearDesc(C.Structure):
    _fields_ = [("inp", _f), ("ldi", C.c_int32), ("Hi", C.c_int32), ("Wi", C.c_int32),
                ("out", _f), ("ldo", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32),
                ("n_out", C.c_int32), ("C", C.c_int32), ("src_mod", C.c_int32), ("src_div", C.c_int32),
                ("out_split", _f), ("ldos", C.c_int32)]


class TdiffDesc(C.Structure):
    _fields_ = [("inp", _f), ("ldi", C.c_int32), ("out", _f), ("ldo", C.c_int32),
                ("n_img", C.c_int32), ("HW", C.c_int32), ("C", C.c_int32), ("seq_len", C.c_int32)]


class TsumDesc(C.Structure):
    _fields_ = [("inp", _f), ("ldi", C.c_int32), ("out", _f), ("ldo", C.c_int32),
                ("n_groups", C.c_int32), ("T", C.c_int32), ("HW", C.c_int32), ("C", C.c_int32)]


class LayoutDesc(C.Structure):
    _fields_ = [("inp", _f), ("out", _f), ("n_img", C.c_int32), ("C", C.c_int32), ("HW", C.c_int32),
                ("ld", C.c_int32), ("to_nhwc", C.c_int32), ("Cpad", C.c_int32)]


class PostDesc(C.Structure):
    _fields_ = [("inp", _f), ("out", _f), ("scratch", _f), ("n_img", C.c_int32), ("h", C.c_int32),
                ("w", C.c_int32), ("H", C.c_int32), ("W", C.c_int32)]


class GuardDesc(C.Structure):
    _fields_ = [("err", _f), ("host_err", _f), ("buf", _f * 3), ("n", C.c_int64 * 3)]


class CopyDesc(C.Structure):
    _fields_ = [("inp", _f), ("out", _f), ("in_pitch", C.c_int64), ("out_pitch", C.c_int64),
                ("row_floats", C.c_int64), ("rows", C.c_int32)]


class FillDesc(C.Structure):
    _fields_ = [("out", _f), ("n", C.c_int64), ("bits", C.c_uint32)]


class FusedIrDesc(C.Structure):
    _fields_ = [("inp", _f), ("ldi", C.c_int32), ("w1", _f), ("scale1", _f), ("bias1", _f),
                ("wd", _f), ("scale_d", _f), ("bias_d", _f), ("w2", _f), ("scale2", _f), ("bias2", _f),
                ("res", _f), ("ldr", C.c_int32), ("out", _f), ("ldo", C.c_int32),
                ("n_img", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Cin", C.c_int32),
                ("hidden", C.c_int32), ("Cout", C.c_int32), ("stride", C.c_int32), ("tile", C.c_int32)]


class WinoDesc(C.Structure):
    _fields_ = [("inp", _f), ("ldi", C.c_int32), ("in_img_stride", C.c_int64),
                ("out", _f), ("ldo", C.c_int32), ("out_img_stride", C.c_int64),
                ("n_img", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32),
                ("Mp", C.c_int64), ("R", C.c_int32),
                ("scale", _f), ("bias", _f), ("act", C.c_int32), ("epi", C.c_int32),
                ("res", _f), ("ldr", C.c_int32), ("res_img_stride", C.c_int64),
                ("aux", _f), ("ldx", C.c_int32), ("aux_img_stride", C.c_int64),
                ("hprev", _f), ("ldh", C.c_int32), ("h_img_stride", C.c_int64),
                ("n_seg", C.c_int32), ("seg_in", _f * 3), ("seg_ld", C.c_int32 * 3), ("seg_c", C.c_int32 * 3),
                ("seg_H", C.c_int32 * 3), ("seg_W", C.c_int32 * 3)]


SCORE_NSTAT, SCORE_REPS, SCORE_RUN, SCORE_NKEY = 16, 100, 4096, 7


class ScoreDesc(C.Structure):
    _fields_ = [("sal", _f), ("fix_loc", _f), ("fix_map", _f), ("jitter", _f),
                ("sal_u8", C.c_int32), ("loc_u8", C.c_int32), ("n_frames", C.c_int32), ("n_pix", C.c_int32),
                ("stats", _f), ("fix_off", _f), ("run_off", _f), ("total_fix", C.c_int64), ("total_runs", C.c_int32),
                ("nan_rows", C.c_int32), ("samp", _f * 2), ("samp_off", _f * 2), ("n_samp", C.c_int64 * 2),
                ("ws", _f), ("ws_bytes", C.c_int64),
                ("out", _f), ("n_keys", C.c_int32), ("keys", C.c_int32 * SCORE_NKEY)]


LETTERBOX_HWC, LETTERBOX_CHW = 0, 1


class LetterboxDesc(C.Structure):
    _fields_ = [("src", _f), ("dst", _f), ("row_pitch", C.c_int64), ("plane_pitch", C.c_int64), ("img_pitch", C.c_int64),
                ("n_img", C.c_int32), ("h0", C.c_int32), ("w0", C.c_int32), ("R", C.c_int32), ("C", C.c_int32),
                ("layout", C.c_int32), ("swap_rb", C.c_int32)]


class OverlayDesc(C.Structure):
    _fields_ = [("frames", _f), ("row_pitch", C.c_int64), ("plane_pitch", C.c_int64), ("img_pitch", C.c_int64),
                ("map", _f), ("map_img_pitch", C.c_int64), ("fix", _f), ("lut", _f),
                ("out", _f), ("ws", _f), ("ws_bytes", C.c_int64),
                ("n_img", C.c_int32), ("layout", C.c_int32), ("h0", C.c_int32), ("w0", C.c_int32),
                ("map_h", C.c_int32), ("map_w", C.c_int32), ("fix_h", C.c_int32), ("fix_w", C.c_int32),
                ("mid_h", C.c_int32), ("mid_w", C.c_int32), ("out_h", C.c_int32), ("out_w", C.c_int32)]


class GazeDesc(C.Structure):
    _fields_ = [("fix_map", _f), ("map_row_pitch", C.c_int64), ("map_col_pitch", C.c_int64), ("map_img_pitch", C.c_int64),
                ("fix_loc", _f), ("loc_row_pitch", C.c_int64), ("loc_col_pitch", C.c_int64), ("loc_img_pitch", C.c_int64),
                ("out", _f), ("flags", _f),
                ("n_img", C.c_int32), ("h0", C.c_int32), ("w0", C.c_int32), ("h", C.c_int32), ("w", C.c_int32)]


LOSS_NSTAT = 16
LOSS_FU_WEIGHTS, LOSS_KL_WEIGHTS = (10.0, -2.0, -1.0), (10.0, 0.0, 0.0)      # loss_functions.py:37-50


class LossDesc(C.Structure):
    _fields_ = [("pred", _f), ("truth", _f), ("stats", _f), ("out", _f), ("grad_out", _f), ("grad", _f),
                ("n_img", C.c_int32), ("n_pix", C.c_int32),
                ("w_kl", C.c_double), ("w_cc", C.c_double), ("w_nss", C.c_double)]


PRIOR_MIN_SLAB = 32           # UAVSAL_PRIOR_MIN_SLAB: no slab of uavsal_prior_accumulate is shorter (csrc/prior.hip)
PRIOR_MAX_FRAMES = (2 ** 31 - 1) // 255


class PriorAccDesc(C.Structure):
    _fields_ = [("frames", _f), ("row_pitch", C.c_int64), ("col_pitch", C.c_int64), ("img_pitch", C.c_int64),
                ("acc", _f), ("acc_row_pitch", C.c_int64), ("acc_col_pitch", C.c_int64),
                ("n_img", C.c_int32), ("h0", C.c_int32), ("w0", C.c_int32)]


class PriorFinishDesc(C.Structure):
    _fields_ = [("acc", _f), ("acc_row_pitch", C.c_int64), ("acc_col_pitch", C.c_int64),
                ("ws", _f), ("out", _f), ("image", _f),
                ("n_frames", C.c_int32), ("h0", C.c_int32), ("w0", C.c_int32), ("h", C.c_int32), ("w", C.c_int32)]


PRIOR_DESC_TYPES = [PriorAccDesc, PriorFinishDesc]        # sized by uavsal_prior_sizeof_desc

WGRAD_CHAIN = 1024            # UAVSAL_WGRAD_CHAIN: the longest MFMA accumulation chain of uavsal_twa_wgrad (csrc/train.hip)


class TwaGateDesc(C.Structure):
    _fields_ = [("g", _f), ("ldg", C.c_int32), ("carry", _f), ("z", _f), ("x", _f), ("ldx", C.c_int32),
                ("hprev", _f), ("ldh", C.c_int32), ("dz", _f), ("carry_out", _f), ("dx", _f),
                ("n_pix", C.c_int64), ("C", C.c_int32)]


class TwaWgradDesc(C.Structure):
    _fields_ = [("dz", _f), ("x", _f), ("ldx", C.c_int32), ("h", _f), ("ldh", C.c_int32), ("h0", _f), ("ldh0", C.c_int32),
                ("ws", _f), ("ws_bytes", C.c_int64), ("out", _f),
                ("T", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("accumulate", C.c_int32)]


class DecBwdDesc(C.Structure):
    _fields_ = [("gy", _f), ("gy_img_pitch", C.c_int64), ("gy_row_pitch", C.c_int64), ("gy_col_pitch", C.c_int64),
                ("y", _f), ("e", _f), ("d", _f), ("s1", _f), ("wd9", _f), ("s2", _f), ("w3", _f), ("s3", _f), ("ge", _f),
                ("n_img", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32)]


TRAIN_DESC_TYPES = [TwaGateDesc, TwaWgradDesc, DecBwdDesc]        # sized by uavsal_train_sizeof_desc


class LstmScanDesc(C.Structure):
    _fields_ = [("cc", _f), ("c0", _f), ("c_seq", _f), ("n_pix", C.c_int64), ("T", C.c_int32), ("C", C.c_int32)]


class LstmGateDesc(C.Structure):
    _fields_ = [("g", _f), ("ldg", C.c_int32), ("carry_h", _f), ("carry_c", _f), ("cc", _f), ("c", _f), ("c_prev", _f),
                ("dcc", _f), ("carry_c_out", _f), ("n_pix", C.c_int64), ("C", C.c_int32)]


LSTM_DESC_TYPES = [LstmScanDesc, LstmGateDesc]                    # sized by uavsal_lstm_sizeof_desc (csrc/train_lstm.hip)

class PixGemmDesc(C.Structure):
    _fields_ = [("a", _f), ("lda", C.c_int32), ("b", _f), ("ldb", C.c_int32), ("row_scale", _f),
                ("w", _f), ("ldw", C.c_int32), ("rowdot", C.c_void_p), ("ws", _f), ("ws_bytes", C.c_int64),
                ("out", _f), ("ldo", C.c_int32), ("K", C.c_int64), ("M", C.c_int32), ("N", C.c_int32), ("accumulate", C.c_int32),
                ("tails32", C.c_int32)]


class DecSumsDesc(C.Structure):
    _fields_ = [("gy", _f), ("gy_img_pitch", C.c_int64), ("gy_row_pitch", C.c_int64), ("gy_col_pitch", C.c_int64),
                ("y", _f), ("e", _f), ("d", _f), ("ga", _f), ("w3", _f), ("s3", _f),
                ("ws", C.c_void_p), ("ws_bytes", C.c_int64),
                ("n_img", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32)]


class DecFinishDesc(C.Structure):
    _fields_ = [("ws", C.c_void_p), ("ws_bytes", C.c_int64), ("rowdot", C.c_void_p)] + [(n, _f) for n in (
        "wd", "w3", "s2", "s3", "r1", "mu1", "r2", "mu2", "r3", "mu3",
        "g_gamma1", "g_beta1", "g_wd", "g_gamma2", "g_beta2", "g_w3", "g_gamma3", "g_beta3")] + [
        ("C", C.c_int32), ("slabs", C.c_int32), ("accumulate", C.c_int32)]


DEC_NSUM = 12                 # UAVSAL_DEC_NSUM: sums per channel in the workspace of uavsal_dec_sums (csrc/train_decoder.hip)
TRAIN_DECODER_DESC_TYPES = [PixGemmDesc, DecSumsDesc, DecFinishDesc]        # sized by uavsal_train_decoder_sizeof_desc


class IrBwdDesc(C.Structure):
    _fields_ = [("gd", _f), ("d", _f), ("e", _f), ("wd9", _f), ("s2", _f), ("ga", _f),
                ("n_img", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32)]


_IR_SUMS_FIELDS = [("gd", _f), ("d", _f), ("e", _f), ("ga", _f), ("go", _f), ("ldgo", C.c_int32),
                   ("ws", C.c_void_p), ("ws_bytes", C.c_int64),
                   ("n_img", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Ch", C.c_int32), ("Co", C.c_int32)]


class IrSumsDesc(C.Structure):
    _fields_ = _IR_SUMS_FIELDS + [("ch16", C.c_int32)]         # ch16: in what was tail padding (the size did not change)


class IrFinishDesc(C.Structure):
    _fields_ = [("ws", C.c_void_p), ("ws_bytes", C.c_int64), ("rowdot1", C.c_void_p), ("rowdot3", C.c_void_p)] + [(n, _f) for n in (
        "wd", "s2", "r1", "mu1", "r2", "mu2", "r3", "mu3",
        "g_gamma1", "g_beta1", "g_wd", "g_gamma2", "g_beta2", "g_gamma3", "g_beta3")] + [
        ("Ch", C.c_int32), ("Co", C.c_int32), ("slabs", C.c_int32), ("accumulate", C.c_int32)]


IR_NSUM = 11                  # UAVSAL_IR_NSUM: sums per hidden channel in the workspace of uavsal_ir_sums (csrc/train_block.hip)
BLOCK_DESC_TYPES = [IrBwdDesc, IrSumsDesc, IrFinishDesc]        # sized by uavsal_block_sizeof_desc


class IrBwdS2Desc(C.Structure):
    _fields_ = [("gd", _f), ("d", _f), ("e", _f), ("wd9", _f), ("s2", _f), ("ga", _f),
                ("n_img", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32)]


class BilinearBwdDesc(C.Structure):
    _fields_ = [("gout", _f), ("ldo", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32),
                ("gin", _f), ("Hi", C.c_int32), ("Wi", C.c_int32),
                ("n_out", C.c_int32), ("n_src", C.c_int32), ("C", C.c_int32), ("src_mod", C.c_int32), ("src_div", C.c_int32)]


class TsumBwdDesc(C.Structure):
    _fields_ = [("a", _f), ("lda", C.c_int32), ("g", _f), ("ldg", C.c_int32), ("out", _f), ("ldo", C.c_int32),
                ("n_groups", C.c_int32), ("T", C.c_int32), ("HW", C.c_int32), ("C", C.c_int32)]


CTX_DESC_TYPES = [IrBwdS2Desc, BilinearBwdDesc, TsumBwdDesc]    # sized by uavsal_ctx_sizeof_desc (csrc/train_ctx.hip)


class IrSumsS2Desc(C.Structure):
    _fields_ = IrSumsDesc._fields_          # the same fields; H, W are the INPUT's, gd / d / go live on the stride-2 grid


MP_DESC_TYPES = [IrSumsS2Desc]              # sized by uavsal_mp_sizeof_desc (csrc/train_ctx.hip)


class IrNarrowDesc(C.Structure):
    _fields_ = [("x", _f), ("e", _f), ("d", _f), ("gd", _f), ("ga", _f), ("go", _f), ("ldgo", C.c_int32),
                ("ws", C.c_void_p), ("ws_bytes", C.c_int64),
                ("n_img", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Cin", C.c_int32), ("Ch", C.c_int32), ("Co", C.c_int32)]


class IrNarrowFinishDesc(C.Structure):
    _fields_ = [("ws", C.c_void_p), ("ws_bytes", C.c_int64)] + [(n, _f) for n in (
        "w1", "wd", "w3", "s1", "s2", "s3", "r1", "mu1", "r2", "mu2", "r3", "mu3",
        "g_w1", "g_gamma1", "g_beta1", "g_wd", "g_gamma2", "g_beta2", "g_w3", "g_gamma3", "g_beta3")] + [
        ("Cin", C.c_int32), ("Ch", C.c_int32), ("Co", C.c_int32), ("slabs", C.c_int32), ("accumulate", C.c_int32)]


class FrameSumDesc(C.Structure):
    _fields_ = [("a", _f), ("lda", C.c_int32), ("out", _f), ("ldo", C.c_int32),
                ("N", C.c_int32), ("HW", C.c_int32), ("C", C.c_int32)]


NARROW_CHUNK = 32             # UAVSAL_NARROW_CHUNK: pixels whose G1 / G3 products uavsal_ir_narrow_grads adds in fp32 (csrc/train_nets.hip)
NETS_DESC_TYPES = [IrNarrowDesc, IrNarrowFinishDesc, FrameSumDesc]      # sized by uavsal_nets_sizeof_desc


class CbrSumsDesc(C.Structure):
    _fields_ = [("g", _f), ("ldg", C.c_int32), ("y", _f), ("ldy", C.c_int32), ("gp", _f),
                ("ws", C.c_void_p), ("ws_bytes", C.c_int64),
                ("n_img", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32)]


class CbrFinishDesc(C.Structure):
    _fields_ = [("ws", C.c_void_p), ("ws_bytes", C.c_int64), ("rowdot", C.c_void_p), ("r", _f), ("mu", _f),
                ("g_gamma", _f), ("g_beta", _f), ("C", C.c_int32), ("slabs", C.c_int32), ("accumulate", C.c_int32)]


class TdiffBwdDesc(C.Structure):
    _fields_ = [("g", _f), ("ldg", C.c_int32), ("r", _f), ("ldr", C.c_int32), ("out", _f), ("ldo", C.c_int32),
                ("n_img", C.c_int32), ("HW", C.c_int32), ("C", C.c_int32), ("seq_len", C.c_int32)]


ST_DESC_TYPES = [CbrSumsDesc, CbrFinishDesc, TdiffBwdDesc]      # sized by uavsal_st_sizeof_desc (csrc/train_st.hip)


class Conv3WgradDesc(C.Structure):
    _fields_ = [("g", _f), ("x", _f), ("ldx", C.c_int32), ("row_scale", _f), ("w", _f), ("rowdot", C.c_void_p),
                ("ws", _f), ("ws_bytes", C.c_int64), ("out", _f),
                ("n_img", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Co", C.c_int32), ("Ci", C.c_int32),
                ("accumulate", C.c_int32)]


class IrBwdDilDesc(C.Structure):
    _fields_ = IrBwdDesc._fields_ + [("dil", C.c_int32)]


class IrSumsDilDesc(C.Structure):
    _fields_ = _IR_SUMS_FIELDS + [("dil", C.c_int32)]


SRF_DESC_TYPES = [Conv3WgradDesc, IrBwdDilDesc, IrSumsDilDesc]  # sized by uavsal_srf_sizeof_desc (csrc/train_srf.hip)


class SkinnyWgradDesc(C.Structure):
    _fields_ = [("a", _f), ("lda", C.c_int32), ("b", _f), ("ldb", C.c_int32), ("row_scale", _f),
                ("w", _f), ("ldw", C.c_int32), ("rowdot", C.c_void_p), ("ws", _f), ("ws_bytes", C.c_int64),
                ("out", _f), ("ldo", C.c_int32), ("K", C.c_int64), ("M", C.c_int32), ("N", C.c_int32), ("accumulate", C.c_int32)]


SKINNY_UNIT, SKINNY_SHARES = 128, 1024       # UAVSAL_SKINNY_UNIT, UAVSAL_SKINNY_SHARES: the K split of uavsal_skinny_wgrad
SKINNY_MAX_NARROW, SKINNY_MAX_WIDE = 32, 192
SHALLOW_DESC_TYPES = [SkinnyWgradDesc]      # sized by uavsal_shallow_sizeof_desc (csrc/train_shallow.hip)

class BnStatsDesc(C.Structure):
    _fields_ = [("u", _f), ("ld", C.c_int32), ("gamma", _f), ("beta", _f), ("running_mean", _f), ("running_var", _f),
                ("eps", C.c_double), ("momentum", C.c_double), ("ws", C.c_void_p), ("ws_bytes", C.c_int64),
                ("mu", _f), ("var", _f), ("r", _f), ("s", _f), ("b", _f),
                ("n_img", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32)]


class BnApplyDesc(C.Structure):
    _fields_ = [("u", _f), ("ld", C.c_int32), ("s", _f), ("b", _f), ("dot_w", _f), ("out", _f),
                ("n_pix", C.c_int64), ("C", C.c_int32), ("act", C.c_int32)]


class BnBwdDesc(C.Structure):
    _fields_ = [("g", _f), ("ldg", C.c_int32), ("g_pix", _f), ("g_chan", _f), ("u", _f), ("ld", C.c_int32),
                ("s", _f), ("b", _f), ("mu", _f), ("r", _f), ("ws", C.c_void_p), ("ws_bytes", C.c_int64), ("sums", C.c_void_p),
                ("g_gamma", _f), ("g_beta", _f), ("g_w", _f), ("gu", _f),
                ("n_img", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("act", C.c_int32),
                ("accumulate", C.c_int32)]


class DwWgradDesc(C.Structure):
    _fields_ = [("g", _f), ("ldg", C.c_int32), ("e", _f), ("lde", C.c_int32), ("ws", C.c_void_p), ("ws_bytes", C.c_int64),
                ("out", _f), ("n_img", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("accumulate", C.c_int32)]


BN_DESC_TYPES = [BnStatsDesc, BnApplyDesc, BnBwdDesc, DwWgradDesc]      # sized by uavsal_bn_sizeof_desc (csrc/train_bn.hip)


class BnApplyResDesc(C.Structure):
    _fields_ = [("u", _f), ("ld", C.c_int32), ("s", _f), ("b", _f), ("res", _f), ("ldr", C.c_int32), ("out", _f),
                ("n_pix", C.c_int64), ("C", C.c_int32), ("act", C.c_int32)]


BLOCK_BN_DESC_TYPES = [BnApplyResDesc]      # sized by uavsal_block_bn_sizeof_desc (csrc/train_bn.hip)

REPACK_MAX_SRC = 4            # UAVSAL_REPACK_MAX_SRC: weights / BatchNorms side by side in one entry (csrc/repack.hip)
REPACK_CONV, REPACK_WINO, REPACK_FOLD, REPACK_DW, REPACK_COPY, REPACK_COPY_T = range(6)
REPACK_LAYOUT = {"f32": 0, "f32k32": 0, "f16x3": 1, "f16x3i": 2, "f16x3j": 3, "bf16": 4, "bf16x3": 5}
REPACK_SCALE, REPACK_BIAS, REPACK_RSTD, REPACK_MEAN = range(4)


class RepackEntry(C.Structure):
    _fields_ = [("kind", C.c_int32), ("layout", C.c_int32), ("dst", _f), ("units", C.c_int64),
                ("src", _f * REPACK_MAX_SRC), ("beta", _f * REPACK_MAX_SRC), ("mean", _f * REPACK_MAX_SRC),
                ("var", _f * REPACK_MAX_SRC), ("eps", C.c_double * REPACK_MAX_SRC), ("rows", C.c_int32 * REPACK_MAX_SRC),
                ("n_src", C.c_int32), ("N", C.c_int32), ("C", C.c_int32), ("taps", C.c_int32), ("Npad", C.c_int32),
                ("Kpad", C.c_int32), ("kt", C.c_int32), ("flip", C.c_int32), ("gi", C.c_int32), ("P", C.c_int32),
                ("sN", C.c_int64), ("sC", C.c_int64), ("off", C.c_int64),
                ("sg", _f), ("sv", _f), ("seps", C.c_double), ("pad", C.c_float), ("reserved", C.c_int32),
                ("G", C.c_double * 18)]


DESC_TYPES = [ConvDesc, DwDesc, StemDesc, BilinearDesc, TdiffDesc, TsumDesc, LayoutDesc, PostDesc, GuardDesc, CopyDesc,
              FusedIrDesc, WinoDesc, DwDotDesc, FillDesc, ScoreDesc, LetterboxDesc, OverlayDesc, GazeDesc, LossDesc, ConvRoute]

# every symbol include/uavsal_hip.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("uavsal_conv_gemm", C.c_int, [C.POINTER(ConvDesc), C.c_void_p]),
    ("uavsal_conv_route_of", C.c_int, [C.POINTER(ConvDesc), C.POINTER(ConvRoute)]),
    ("uavsal_conv_tile", C.c_int, [C.POINTER(ConvDesc)]),
    ("uavsal_conv_uses_split", C.c_int, [C.POINTER(ConvDesc)]),
    ("uavsal_conv_dwproj", C.c_int, [C.POINTER(ConvDesc)]),
    ("uavsal_streamk_workspace_bytes", C.c_longlong, []),
    ("uavsal_conv_streamk_grid", C.c_int, [C.POINTER(ConvDesc)]),
    ("uavsal_dw3x3", C.c_int, [C.POINTER(DwDesc), C.c_void_p]),
    ("uavsal_dw3x3_dot", C.c_int, [C.POINTER(DwDotDesc), C.c_void_p]),
    ("uavsal_dw_variant", C.c_int, [C.POINTER(DwDesc)]),
    ("uavsal_stem_conv", C.c_int, [C.POINTER(StemDesc), C.c_void_p]),
    ("uavsal_bilinear_ac", C.c_int, [C.POINTER(BilinearDesc), C.c_void_p]),
    ("uavsal_tdiff", C.c_int, [C.POINTER(TdiffDesc), C.c_void_p]),
    ("uavsal_tsum", C.c_int, [C.POINTER(TsumDesc), C.c_void_p]),
    ("uavsal_layout", C.c_int, [C.POINTER(LayoutDesc), C.c_void_p]),
    ("uavsal_postprocess", C.c_int, [C.POINTER(PostDesc), C.c_void_p]),
    ("uavsal_letterbox_u8", C.c_int, [C.POINTER(LetterboxDesc), C.c_void_p]),
    ("uavsal_overlay_workspace_bytes", C.c_int64, [C.POINTER(OverlayDesc)]),
    ("uavsal_overlay_u8", C.c_int, [C.POINTER(OverlayDesc), C.c_void_p]),
    ("uavsal_gaze_prepare", C.c_int, [C.POINTER(GazeDesc), C.c_void_p]),
    ("uavsal_loss_fu", C.c_int, [C.POINTER(LossDesc), C.c_void_p]),
    ("uavsal_loss_fu_grad", C.c_int, [C.POINTER(LossDesc), C.c_void_p]),
    ("uavsal_prior_accumulate", C.c_int, [C.POINTER(PriorAccDesc), C.c_void_p]),
    ("uavsal_prior_finish", C.c_int, [C.POINTER(PriorFinishDesc), C.c_void_p]),
    ("uavsal_prior_slab_frames", C.c_int, [C.c_int64, C.c_int32]),
    ("uavsal_prior_sizeof_desc", C.c_int, [C.c_int]),
    ("uavsal_twa_gate_bwd", C.c_int, [C.POINTER(TwaGateDesc), C.c_void_p]),
    ("uavsal_twa_wgrad_workspace_bytes", C.c_int64, [C.POINTER(TwaWgradDesc)]),
    ("uavsal_twa_wgrad_shares", C.c_int, [C.POINTER(TwaWgradDesc)]),
    ("uavsal_twa_wgrad", C.c_int, [C.POINTER(TwaWgradDesc), C.c_void_p]),
    ("uavsal_dec_bwd", C.c_int, [C.POINTER(DecBwdDesc), C.c_void_p]),
    ("uavsal_train_sizeof_desc", C.c_int, [C.c_int]),
    ("uavsal_lstm_scan", C.c_int, [C.POINTER(LstmScanDesc), C.c_void_p]),
    ("uavsal_lstm_gate_bwd", C.c_int, [C.POINTER(LstmGateDesc), C.c_void_p]),
    ("uavsal_lstm_sizeof_desc", C.c_int, [C.c_int]),
    ("uavsal_pix_gemm_workspace_bytes", C.c_int64, [C.POINTER(PixGemmDesc)]),
    ("uavsal_pix_gemm_shares", C.c_int, [C.POINTER(PixGemmDesc)]),
    ("uavsal_pix_gemm", C.c_int, [C.POINTER(PixGemmDesc), C.c_void_p]),
    ("uavsal_dec_sums_workspace_bytes", C.c_int64, [C.POINTER(DecSumsDesc)]),
    ("uavsal_dec_sums_slabs", C.c_int, [C.POINTER(DecSumsDesc)]),
    ("uavsal_dec_sums_slab_rows", C.c_int, [C.POINTER(DecSumsDesc)]),
    ("uavsal_dec_sums", C.c_int, [C.POINTER(DecSumsDesc), C.c_void_p]),
    ("uavsal_dec_finish", C.c_int, [C.POINTER(DecFinishDesc), C.c_void_p]),
    ("uavsal_train_decoder_sizeof_desc", C.c_int, [C.c_int]),
    ("uavsal_ir_bwd", C.c_int, [C.POINTER(IrBwdDesc), C.c_void_p]),
    ("uavsal_ir_sums_workspace_bytes", C.c_int64, [C.POINTER(IrSumsDesc)]),
    ("uavsal_ir_sums_slabs", C.c_int, [C.POINTER(IrSumsDesc)]),
    ("uavsal_ir_sums_slab_rows", C.c_int, [C.POINTER(IrSumsDesc)]),
    ("uavsal_ir_sums", C.c_int, [C.POINTER(IrSumsDesc), C.c_void_p]),
    ("uavsal_ir_finish", C.c_int, [C.POINTER(IrFinishDesc), C.c_void_p]),
    ("uavsal_ir_finish_c16", C.c_int, [C.POINTER(IrFinishDesc), C.c_void_p]),
    ("uavsal_block_sizeof_desc", C.c_int, [C.c_int]),
    ("uavsal_ir_bwd_s2", C.c_int, [C.POINTER(IrBwdS2Desc), C.c_void_p]),
    ("uavsal_bilinear_ac_bwd", C.c_int, [C.POINTER(BilinearBwdDesc), C.c_void_p]),
    ("uavsal_tsum_bwd", C.c_int, [C.POINTER(TsumBwdDesc), C.c_void_p]),
    ("uavsal_ctx_sizeof_desc", C.c_int, [C.c_int]),
    ("uavsal_ir_sums_s2_workspace_bytes", C.c_int64, [C.POINTER(IrSumsS2Desc)]),
    ("uavsal_ir_sums_s2_slabs", C.c_int, [C.POINTER(IrSumsS2Desc)]),
    ("uavsal_ir_sums_s2_slab_rows", C.c_int, [C.POINTER(IrSumsS2Desc)]),
    ("uavsal_ir_sums_s2", C.c_int, [C.POINTER(IrSumsS2Desc), C.c_void_p]),
    ("uavsal_mp_sizeof_desc", C.c_int, [C.c_int]),
    ("uavsal_ir_narrow_workspace_bytes", C.c_int64, [C.POINTER(IrNarrowDesc)]),
    ("uavsal_ir_narrow_slabs", C.c_int, [C.POINTER(IrNarrowDesc)]),
    ("uavsal_ir_narrow_slab_rows", C.c_int, [C.POINTER(IrNarrowDesc)]),
    ("uavsal_ir_narrow_grads", C.c_int, [C.POINTER(IrNarrowDesc), C.c_void_p]),
    ("uavsal_ir_narrow_finish", C.c_int, [C.POINTER(IrNarrowFinishDesc), C.c_void_p]),
    ("uavsal_frame_sum", C.c_int, [C.POINTER(FrameSumDesc), C.c_void_p]),
    ("uavsal_nets_sizeof_desc", C.c_int, [C.c_int]),
    ("uavsal_cbr_sums_workspace_bytes", C.c_int64, [C.POINTER(CbrSumsDesc)]),
    ("uavsal_cbr_sums_slabs", C.c_int, [C.POINTER(CbrSumsDesc)]),
    ("uavsal_cbr_sums_slab_rows", C.c_int, [C.POINTER(CbrSumsDesc)]),
    ("uavsal_cbr_sums", C.c_int, [C.POINTER(CbrSumsDesc), C.c_void_p]),
    ("uavsal_cbr_finish", C.c_int, [C.POINTER(CbrFinishDesc), C.c_void_p]),
    ("uavsal_tdiff_bwd", C.c_int, [C.POINTER(TdiffBwdDesc), C.c_void_p]),
    ("uavsal_st_sizeof_desc", C.c_int, [C.c_int]),
    ("uavsal_conv3_wgrad_workspace_bytes", C.c_int64, [C.POINTER(Conv3WgradDesc)]),
    ("uavsal_conv3_wgrad_shares", C.c_int, [C.POINTER(Conv3WgradDesc)]),
    ("uavsal_conv3_wgrad", C.c_int, [C.POINTER(Conv3WgradDesc), C.c_void_p]),
    ("uavsal_ir_bwd_dil", C.c_int, [C.POINTER(IrBwdDilDesc), C.c_void_p]),
    ("uavsal_ir_sums_dil_workspace_bytes", C.c_int64, [C.POINTER(IrSumsDilDesc)]),
    ("uavsal_ir_sums_dil_slabs", C.c_int, [C.POINTER(IrSumsDilDesc)]),
    ("uavsal_ir_sums_dil_slab_rows", C.c_int, [C.POINTER(IrSumsDilDesc)]),
    ("uavsal_ir_sums_dil", C.c_int, [C.POINTER(IrSumsDilDesc), C.c_void_p]),
    ("uavsal_srf_sizeof_desc", C.c_int, [C.c_int]),
    ("uavsal_skinny_wgrad_workspace_bytes", C.c_int64, [C.POINTER(SkinnyWgradDesc)]),
    ("uavsal_skinny_wgrad_shares", C.c_int, [C.POINTER(SkinnyWgradDesc)]),
    ("uavsal_skinny_wgrad", C.c_int, [C.POINTER(SkinnyWgradDesc), C.c_void_p]),
    ("uavsal_shallow_sizeof_desc", C.c_int, [C.c_int]),
    ("uavsal_bn_slabs", C.c_int, [C.c_int, C.c_int, C.c_int]),
    ("uavsal_bn_slab_rows", C.c_int, [C.c_int, C.c_int, C.c_int]),
    ("uavsal_bn_stats_workspace_bytes", C.c_int64, [C.POINTER(BnStatsDesc)]),
    ("uavsal_bn_stats", C.c_int, [C.POINTER(BnStatsDesc), C.c_void_p]),
    ("uavsal_bn_apply", C.c_int, [C.POINTER(BnApplyDesc), C.c_void_p]),
    ("uavsal_bn_bwd_workspace_bytes", C.c_int64, [C.POINTER(BnBwdDesc)]),
    ("uavsal_bn_bwd_sums", C.c_int, [C.POINTER(BnBwdDesc), C.c_void_p]),
    ("uavsal_bn_bwd_apply", C.c_int, [C.POINTER(BnBwdDesc), C.c_void_p]),
    ("uavsal_dw_wgrad_workspace_bytes", C.c_int64, [C.POINTER(DwWgradDesc)]),
    ("uavsal_dw_wgrad", C.c_int, [C.POINTER(DwWgradDesc), C.c_void_p]),
    ("uavsal_bn_sizeof_desc", C.c_int, [C.c_int]),
    ("uavsal_bn_apply_res", C.c_int, [C.POINTER(BnApplyResDesc), C.c_void_p]),
    ("uavsal_block_bn_sizeof_desc", C.c_int, [C.c_int]),
    ("uavsal_repack", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    ("uavsal_repack_sizeof_desc", C.c_int, []),
    ("uavsal_guard", C.c_int, [C.POINTER(GuardDesc), C.c_void_p]),
    ("uavsal_copy_rows", C.c_int, [C.POINTER(CopyDesc), C.c_void_p]),
    ("uavsal_fill", C.c_int, [C.POINTER(FillDesc), C.c_void_p]),
    ("uavsal_plan_add_fill", C.c_int, [C.c_void_p, C.POINTER(FillDesc)]),
    ("uavsal_fused_ir", C.c_int, [C.POINTER(FusedIrDesc), C.c_void_p]),
    ("uavsal_fused_ir_supported", C.c_int, [C.POINTER(FusedIrDesc)]),
    ("uavsal_plan_add_fused_ir", C.c_int, [C.c_void_p, C.POINTER(FusedIrDesc)]),
    ("uavsal_wino_input", C.c_int, [C.POINTER(WinoDesc), C.c_void_p]),
    ("uavsal_wino_output", C.c_int, [C.POINTER(WinoDesc), C.c_void_p]),
    ("uavsal_wino_output_zero_h", C.c_int, [C.POINTER(WinoDesc), C.c_void_p]),
    ("uavsal_wino_seam", C.c_int, [C.POINTER(WinoDesc), C.POINTER(WinoDesc), C.c_void_p]),
    ("uavsal_wino_seam_zero_h", C.c_int, [C.POINTER(WinoDesc), C.POINTER(WinoDesc), C.c_void_p]),
    ("uavsal_wino_seam_check", C.c_int, [C.POINTER(WinoDesc), C.POINTER(WinoDesc)]),
    ("uavsal_plan_add_wino_input", C.c_int, [C.c_void_p, C.POINTER(WinoDesc)]),
    ("uavsal_plan_add_wino_output", C.c_int, [C.c_void_p, C.POINTER(WinoDesc)]),
    ("uavsal_plan_add_copy", C.c_int, [C.c_void_p, C.POINTER(CopyDesc)]),
    ("uavsal_plan_create", C.c_void_p, []),
    ("uavsal_plan_destroy", None, [C.c_void_p]),
    ("uavsal_plan_add_conv", C.c_int, [C.c_void_p, C.POINTER(ConvDesc)]),
    ("uavsal_plan_add_dw", C.c_int, [C.c_void_p, C.POINTER(DwDesc)]),
    ("uavsal_plan_add_dw_dot", C.c_int, [C.c_void_p, C.POINTER(DwDotDesc)]),
    ("uavsal_plan_add_stem", C.c_int, [C.c_void_p, C.POINTER(StemDesc)]),
    ("uavsal_plan_add_bilinear", C.c_int, [C.c_void_p, C.POINTER(BilinearDesc)]),
    ("uavsal_plan_add_tdiff", C.c_int, [C.c_void_p, C.POINTER(TdiffDesc)]),
    ("uavsal_plan_add_tsum", C.c_int, [C.c_void_p, C.POINTER(TsumDesc)]),
    ("uavsal_plan_add_layout", C.c_int, [C.c_void_p, C.POINTER(LayoutDesc)]),
    ("uavsal_plan_error_word", C.c_void_p, [C.c_void_p]),
    ("uavsal_plan_add_guard", C.c_int, [C.c_void_p, _f, C.c_int64, _f, C.c_int64, _f, C.c_int64]),
    ("uavsal_plan_status", C.c_int, [C.c_void_p, C.c_int]),
    ("uavsal_plan_patch_ptr", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    ("uavsal_plan_set_lane", C.c_int, [C.c_void_p, C.c_int]),
    ("uavsal_plan_add_fork", C.c_int, [C.c_void_p, C.c_int]),
    ("uavsal_plan_add_join", C.c_int, [C.c_void_p, C.c_int]),
    ("uavsal_plan_enable_lanes", C.c_int, [C.c_void_p, C.c_int]),
    ("uavsal_plan_size", C.c_int, [C.c_void_p]),
    ("uavsal_plan_run", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    ("uavsal_plan_group_mark", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    ("uavsal_plan_group_enable", C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ("uavsal_plan_group_launches", C.c_int, [C.c_void_p, C.c_int]),
    ("uavsal_plan_last_launches", C.c_int, [C.c_void_p]),
    ("uavsal_plan_frame_repeat", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    ("uavsal_plan_frame_repeat_workgroups", C.c_int, [C.c_void_p, C.c_int]),
    ("uavsal_plan_seam", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    ("uavsal_plan_zero_state", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    ("uavsal_plan_mode_report", C.c_int, [C.c_void_p, C.POINTER(C.c_int * 4)]),
    ("uavsal_plan_graph_build", C.c_int, [C.c_void_p, C.c_void_p]),
    ("uavsal_plan_graph_launch", C.c_int, [C.c_void_p, C.c_void_p]),
    ("uavsal_plan_time", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_float)]),
    ("uavsal_score_workspace_bytes", C.c_int64, [C.POINTER(ScoreDesc)]),
    ("uavsal_score_stats", C.c_int, [C.POINTER(ScoreDesc), C.c_void_p]),
    ("uavsal_score_run", C.c_int, [C.POINTER(ScoreDesc), C.c_void_p]),
    ("uavsal_abi_version", C.c_int, []),
    ("uavsal_sizeof_desc", C.c_int, [C.c_int]),
    ("uavsal_build_info", C.c_char_p, []),
]

_lib = None


def load():
    """Load (once) and type the shared library.  Raises RuntimeError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libuavsal_hip.so is not built (%s). Run `python -m iip_uavsal_saliency_amd.build` "
            "(needs hipcc). There is no CPU fallback for the UAVSal HIP path." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)          # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    if lib.uavsal_abi_version() != 20:
        raise RuntimeError("libuavsal_hip.so ABI version mismatch")
    for i, t in enumerate(DESC_TYPES):
        if lib.uavsal_sizeof_desc(i) != C.sizeof(t):
            raise RuntimeError("descriptor %s: ctypes size %d != C size %d" % (
                t.__name__, C.sizeof(t), lib.uavsal_sizeof_desc(i)))
    for sizeof, types in ((lib.uavsal_prior_sizeof_desc, PRIOR_DESC_TYPES), (lib.uavsal_train_sizeof_desc, TRAIN_DESC_TYPES),
                          (lib.uavsal_train_decoder_sizeof_desc, TRAIN_DECODER_DESC_TYPES),
                          (lib.uavsal_block_sizeof_desc, BLOCK_DESC_TYPES), (lib.uavsal_ctx_sizeof_desc, CTX_DESC_TYPES),
                          (lib.uavsal_mp_sizeof_desc, MP_DESC_TYPES), (lib.uavsal_nets_sizeof_desc, NETS_DESC_TYPES),
                          (lib.uavsal_st_sizeof_desc, ST_DESC_TYPES), (lib.uavsal_srf_sizeof_desc, SRF_DESC_TYPES),
                          (lib.uavsal_shallow_sizeof_desc, SHALLOW_DESC_TYPES), (lib.uavsal_lstm_sizeof_desc, LSTM_DESC_TYPES),
                          (lib.uavsal_bn_sizeof_desc, BN_DESC_TYPES), (lib.uavsal_block_bn_sizeof_desc, BLOCK_BN_DESC_TYPES)):
        for i, t in enumerate(types):
            if sizeof(i) != C.sizeof(t):
                raise RuntimeError("descriptor %s: ctypes size %d != C size %d" % (t.__name__, C.sizeof(t), sizeof(i)))
    if lib.uavsal_repack_sizeof_desc() != C.sizeof(RepackEntry):
        raise RuntimeError("descriptor RepackEntry: ctypes size %d != C size %d" % (C.sizeof(RepackEntry), lib.uavsal_repack_sizeof_desc()))
    _lib = lib
    return lib


def check(code: int, what: str = "uavsal call"):
    if code == 0:
        return
    if code == -5:
        raise RuntimeError("%s: %s" % (what, _ERR[-5]))
    if code < 0:
        raise RuntimeError("%s rejected its arguments: %s" % (what, _ERR.get(code, str(code))))
    raise RuntimeError("%s failed with hipError_t %d" % (what, code))
