/*
 * uavsal_hip.h -- C ABI of libuavsal_hip.so, the MI355X (gfx950) kernels behind
 * UAVSal.forward.
 *
 * The reference (zhangkao/IIP_UAVSal_Saliency) is pure Python: it has no native
 * boundary of its own.  Every arithmetic step of `UAVSal.forward`
 * (model.py:341-375) is a stock torch.nn operator.  This header therefore
 * defines the native boundary the drop-in needs: one entry point per operator
 * class of the hot path, each citing the reference expression (file:line,
 * relative to the reference root) it replaces.  Plain pointers and sizes only:
 * no torch types, no allocation, no ownership transfer, no global state.
 *
 * Conventions
 *   - all tensors are fp32 device pointers, activations NHWC
 *     ([image][y][x][channel]); `ld*` is the channel stride of the buffer in
 *     floats, so a pointer + ld pair can address a channel slice of a wider
 *     buffer (this is how torch.cat, model.py:146,155,363,365, disappears);
 *   - `*_img_stride` is the distance between consecutive images in PIXELS
 *     (H*W for a dense batch; T*H*W when one time step of C clips is addressed,
 *     model_convlstm.py:368-371);
 *   - channel counts, ld's and slice offsets are multiples of 4 floats (16 B);
 *   - `stream` is a hipStream_t passed as void*; kernels are launched on it and
 *     nothing synchronises;
 *   - every function returns 0 on success, a positive hipError_t if the launch
 *     failed, or a negative UAVSAL_E* code if the arguments were rejected.
 *
 * Built for gfx950 only.  No CUDA path, no CPU fallback.
 */
#ifndef UAVSAL_HIP_H
#define UAVSAL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UAVSAL_ABI_VERSION 20

/* argument errors */
#define UAVSAL_EINVAL   (-1)  /* null pointer / non-positive size */
#define UAVSAL_EALIGN   (-2)  /* channel count / ld / pointer not 16-byte aligned */
#define UAVSAL_ESHAPE   (-3)  /* shape not supported by the kernel (see entry point) */
#define UAVSAL_ESTATE   (-4)  /* plan used in the wrong state */
#define UAVSAL_EDEVICE  (-5)  /* a kernel reported that it could not complete its work (uavsal_conv_desc.err):
                                 the outputs of that run are invalid and were overwritten with NaN */

/* bits of the device error word (uavsal_conv_desc.err) */
#define UAVSAL_ERR_STREAMK  1 /* a stream-K owner gave up waiting for a partial tile another workgroup owed it */

/* GEMM operand precision (how fp32 activations/weights are fed to the matrix cores) */
#define UAVSAL_PREC_F32     0 /* v_mfma_f32_32x32x2_f32: exact fp32 fma chain */
#define UAVSAL_PREC_BF16X3  1 /* 3x v_mfma_f32_32x32x16_bf16 on a hi/lo bf16 split, fp32 accumulate */
#define UAVSAL_PREC_BF16    2 /* 1x bf16 MFMA, fp32 accumulate */
#define UAVSAL_PREC_F16X3   3 /* 3x v_mfma_f32_32x32x16_f16 on a hi/lo fp16 split (22 mantissa bits), fp32 accumulate;
                                 activations are pre-scaled by 2^4 (finite for any finite x: saturates near |x| = 8188), weights by 2^6 */

#define UAVSAL_ACT_NONE     0
#define UAVSAL_ACT_RELU6    1 /* nn.ReLU6, model.py:71 */
#define UAVSAL_ACT_SIGMOID  2 /* torch.sigmoid, model.py:373 */

#define UAVSAL_EPI_AFFINE   0 /* y = act(acc*scale + bias) [+ res] */
#define UAVSAL_EPI_TWA      1 /* ConvTWA gate + state update, see uavsal_conv_desc */
#define UAVSAL_EPI_LSTM     2 /* ConvLSTM gates + cell/hidden update, see uavsal_conv_desc */

typedef void* uavsal_stream_t;

/*
 * Dense 1x1 or 3x3 (stride 1, pad 1) convolution as an implicit GEMM on the
 * matrix cores, with the folded BatchNorm, activation, residual add and the
 * ConvTWA state update fused into the epilogue.
 *
 * Replaces: BasicConv2d k=1 / k=3 (model.py:65-72: Conv2d(bias=False) + BatchNorm2d
 * (eval: scale = gamma/sqrt(var+1e-5), bias = beta - mean*scale) + ReLU6); the
 * pw-linear Conv2d+BatchNorm2d tail of dwBlock (model.py:94-95) with its residual
 * (model.py:100-101); torchvision InvertedResidual's pointwise convs; STBlock's
 * `x_sp + x_te` and `x + out` adds (model.py:241,247) as post-activation residuals;
 * the final torch.sigmoid (model.py:373); and, with epi=UAVSAL_EPI_TWA,
 * ConvTWACell.forward (model_convlstm.py:276-292).
 *
 * EPI_AFFINE: out[m, n] = act(acc[m, n] * scale[n] + bias[n]) + (res ? res[m, n] : 0)
 *             (scale == NULL -> raw accumulator, bias ignored)
 * EPI_TWA:    a = h_{t-1} (Cin == Cout), w = the W[:, Cin:, :, :] half of rnn_conv,
 *             aux = conv3x3(W[:, :Cin], x_t) precomputed for this step, res = x_t:
 *             i = sigmoid(acc + aux);  out = i * res + (1 - i) * a
 * EPI_LSTM:   ConvLSTMCell.forward (model_convlstm.py:111-126, bias=False) with the x half of the
 *             conv hoisted: a = h_{t-1} (Cin = hid), Cout = 4*hid with the rows of W[:, hid:] (and
 *             of the hoisted aux) interleaved as n = 4*c + gate, gate order (i, f, o, g);
 *             res = c_{t-1} [hid], out = h_t [hid], out2 = c_t [hid]:
 *             z = acc + aux;  c_t = sigmoid(z_f)*c_{t-1} + sigmoid(z_i)*tanh(z_g);
 *             h_t = sigmoid(z_o)*tanh(c_t).   Runs on the 64x64 tile; needs 16-byte aligned ld's.
 *
 * Weights `w` are pre-packed by the host (iip_uavsal_saliency_amd/packing.py):
 *   k index = ci for taps == 1; for taps == 9 (tap = ky*3 + kx) channel-block-major, tap-minor:
 *   k = ((ci / KT) * 9 + tap) * KT + ci % KT, so that the nine taps of one channel chunk are
 *   nine consecutive K steps; rows padded to Npad = roundup(Cout, 32), K padded to
 *   Kpad = roundup(taps * Cin, KT) with zeros, KT = 16 (F32) or 32 (BF16*, F16X3);
 *   F32:    float  [Npad][Kpad]
 *   The 16-bit layouts are K-step-major, so that the weight rows one K step needs are ONE
 *   contiguous run of whole cache lines (measured +4..7 % on the split GEMMs; the LDS-DMA
 *   fp32 kernel measured 2..6 % slower with it and keeps the row-major layout):
 *   BF16:   uint16 [Kpad/32][Npad][32]     (bf16 bits, round-to-nearest-even)
 *   BF16X3: uint16 [Kpad/32][2][Npad][32]  ([.][0] = hi, [.][1] = lo = bf16(w - hi))
 *   F16X3:  as BF16X3 with fp16 bits of ws = 64*w: hi = fp16(ws), lo = fp16(ws - hi)
 *   in the BF16* / F16X3 layouts each group of 32 k's is stored in the order
 *   {0-3,16-19, 4-7,20-23, 8-11,24-27, 12-15,28-31} (matches the A staging).
 * taps == 9 requires Cin % 32 == 0.
 */
typedef struct uavsal_conv_desc {
    const float* a;      int32_t lda;  int64_t a_img_stride;
    const void*  w;
    const float* scale;  const float* bias;          /* [>= Cout] each, or NULL */
    float*       out;    int32_t ldc;  int64_t o_img_stride;
    const float* res;    int32_t ldr;  int64_t r_img_stride;   /* NULL = none */
    const float* aux;    int32_t ldx;  int64_t x_img_stride;   /* EPI_TWA only */
    int32_t n_img, H, W;         /* output == input spatial size */
    int32_t Cin, Cout, taps;     /* taps: 1 or 9 */
    int32_t prec, act, epi;
    int32_t tile;                /* 0 = auto; else 1: 128x128, 2: 128x64, 3: 128x32, 4: 64x64, 5: 128x256, 6: 256x256 (split
                                  * 16-bit precisions; others run them as 1), 7: 256x128 on 8 waves (F32; others as 1);
                                  * F32 with Cin % 32 == 0, K stages of 32 floats = one cache line per tile row
                                  * (conv_gemm_k32.hip; 3x3 weights then in the 'f32k32' K order, see `w`): 8: 128x128,
                                  * 9: 256x128 on 8 waves, 10: 128x128 as one continuous stage stream (vector affine
                                  * epilogue only), 11: 64x64.  Shapes an instance cannot take fall back: 10 -> 8 -> 1,
                                  * 9 -> 7, 11 -> 4.  What a descriptor actually runs -- kernel family, tile, K shares per
                                  * tile -- is decided in one place and uavsal_conv_route_of tells it (uavsal_conv_route). */
    float*       out2;   int32_t ld2;                 /* EPI_LSTM only: c_t (image stride = o_img_stride) */
    /* Fused depthwise producer (taps == 1, EPI_AFFINE): when dw_w9c != NULL, `a` is the EXPANDED tensor E
     * [n_img, dw_Hin, dw_Win, Cin] of an inverted-residual block and the GEMM's A operand is computed on the
     * fly as relu6(dw_scale * depthwise3x3(E; dw_w9c, stride dw_stride, pad 1) + dw_bias), i.e. the
     * groups=hidden BasicConv2d of dwBlock (model.py:92) feeding its pw-linear conv (model.py:94) without the
     * intermediate tensor ever reaching HBM.  H, W are the OUTPUT sizes ((dw_Hin-1)/dw_stride+1, ...);
     * dw_w9c is tap-major [9][Cin] as in uavsal_dw_desc; a_img_stride counts input pixels.
     * F32 / F16X3, dw_stride 1, Cin % 16 == 0 (<= 4096) run the LDS-halo kernel (a workgroup stages the 10 x 18
     * halo of an 8 x 16 pixel patch per 16 channels, computes the depthwise in LDS and feeds the MFMA loop:
     * uavsal_conv_dwproj tells; its F16X3 form takes the weights as [Cin/16][Npad][hi 16 | lo 16] fp16 lines of
     * 64 w, packing.py 'f16x3j'); everything else the register-staged loader of round 1 (correct, latency-bound).
     * With `sk_ws` set, narrow outputs (Cout <= 32) whose tiles would leave workgroup slots empty split K over 2-4
     * workgroups per tile: raw partial sums go to the partial-tile area of `sk_ws` and a second small launch sums them
     * in a fixed order and applies BN / activation / residual (deterministic; no atomics). */
    const float* dw_w9c; const float* dw_scale; const float* dw_bias;
    int32_t dw_stride, dw_Hin, dw_Win;
    /* Optional stream-K workspace (fp32, 128x128 and 64x64 tiles; 64 KB of flags, then partial tiles): `uavsal_streamk_workspace_bytes()` bytes of device
     * memory, 16-byte aligned, ZERO-filled once by the caller and then owned by launches that are ordered
     * on one stream (the kernels leave it zeroed).  With it, launches whose tile count would idle part of
     * the chip in the last round split the K loop of some tiles across workgroups; the summation order
     * stays a function of the shape only.  NULL = whole-tile scheduling.
     * Progress: a workgroup computes the piece it owes another tile BEFORE it waits for anything, and it only
     * ever waits for workgroups with a higher block id, so the launch completes whenever the hardware starts
     * workgroups in block order (it does; HIP does not promise it).  The wait is therefore bounded
     * (`sk_spin_limit` polls): an owner that gives up leaves the missing piece OUT of its sum and sets
     * UAVSAL_ERR_STREAMK in `*err` -- the caller must treat the output as invalid and re-zero the flag block
     * (uavsal_guard / uavsal_plan_status do both checks for a plan). */
    void* sk_ws; int64_t sk_ws_bytes;
    /* Pre-split operands (UAVSAL_PREC_F16X3 only).  The "split shadow" of an fp32 NHWC activation tensor x with
     * channel stride ld (ld % 32 == 0) is an fp16 buffer [pixel][ld / 32][2][32]: for every group of 32
     * channels, 32 halves hi = fp16_rtz(16*x) followed by 32 halves lo = fp16_rtz(16*x - hi) -- exactly what the
     * register-staged kernel computes from `a` on every load, in the same number of bytes as x, laid out so
     * that the 32 channels one K step needs are ONE 128-byte line per pixel (planar hi / lo planes made every
     * request half a line and the L1 <- L2 traffic 1.5x the useful bytes: profiles/r2_presplit_pmc.md).
     * Row stride `ld*s` is in halves (2 * ld for a dense shadow); a channel slice starts at a multiple of 32.
     * When a_split is given (and Cin % 32 == 0, tile 1 / 5 / 6, vector epilogue) the GEMM stages BOTH operands
     * with LDS-DMA and does no conversion work; `w` must then be packed 'f16x3i' (packing.py: per K step and
     * output channel the same [32 hi | 32 lo] line; uavsal_conv_uses_split tells which).  `a` may be NULL
     * then unless epi == UAVSAL_EPI_TWA.
     * out_split (UAVSAL_PREC_F16X3, vector epilogue only; Cout % 32 == 0): the result is additionally written as
     * a split shadow for the GEMMs that consume it -- the fp32 copy stays for every other consumer. */
    const void* a_split;  int32_t ldas;
    void* out_split;      int32_t ldos;
    int32_t* err;            /* device word OR-ed with UAVSAL_ERR_* (NULL: the last int32 of sk_ws' 64 KB flag block) */
    int32_t sk_spin_limit;   /* polls before a stream-K owner gives up on one piece; 0 = default (1 << 22, seconds) */
    int32_t sk_debug_drop;   /* TEST HOOK: 1 + index of the stream-K workgroup that withholds its "published" flag (< 0: all do); 0 = none */
    /* Per-image weights (F32, taps == 1, tiles 8 / 11; 0 = one weight matrix for all images): image g multiplies with
     * the packed matrix at w + g * w_group_stride floats, and H * W must be a multiple of 128 so that no GEMM tile
     * straddles two images.  This is how the sixteen GEMMs of a Winograd 3x3 convolution run as one launch
     * (uavsal_wino_input / uavsal_wino_output: the images are the sixteen transform planes). */
    int64_t w_group_stride;
    /* Several convs of different inputs as ONE launch (F32, taps == 1, tile 11; 0 = off): output channels
     * [g * n_group, (g + 1) * n_group) are computed from the A columns [g * a_group_off, g * a_group_off + Cin), i.e. the
     * inputs lie side by side in the rows of `a` (lda >= groups * a_group_off) and the weight rows of the groups are stacked
     * ([Cout][Kpad], the ordinary layout).  n_group % 64 == 0, Cout % n_group == 0.  The three dilated ASPP projections
     * (model.py:142-147) run this way. */
    int32_t n_group, a_group_off;
} uavsal_conv_desc;

int uavsal_conv_gemm(const uavsal_conv_desc* d, uavsal_stream_t stream);
/* size of the optional stream-K workspace (see uavsal_conv_desc.sk_ws) */
long long uavsal_streamk_workspace_bytes(void);

/* What `uavsal_conv_gemm` runs for a descriptor: everything that is decided from the descriptor before a kernel starts.
 * It is decided once per launch, by one function (conv_route in csrc/conv_gemm.hip; the K-split rules and the fp32
 * 32-float-K eligibility it uses are in csrc/conv_route.h), in this order of families:
 *   PRESPLIT   both operands by LDS-DMA from split shadows (a_split set, shape eligible): `w` packed 'f16x3i'
 *   DWPROJ     LDS-halo depthwise -> projection, output-channel tile `dwproj` = dwproj_kernel<PREC,2,4,2,2> (256) /
 *              <PREC,2,4,2,1> (128) / <PREC,4,2,1,1> (64) / <PREC,4,1,1,1> (32); F16X3 weights packed 'f16x3j'
 *   STREAMK    fp32 LDS-DMA kernel, tiles 1 / 3 / 4, `streamk` workgroups share the K loops of some tiles
 *   K32        fp32 kernels with 32-float K stages, tiles 8 .. 11: 3x3 weights in the K order with 32-channel blocks
 *              (k = ((ci / 32) * 9 + tap) * 32 + ci % 32, packing.py 'f32k32'; every other family 16-channel blocks)
 *   F32_DMA    fp32 LDS-DMA kernel, whole tiles
 *   STAGED     register-staged kernel of the descriptor's precision (and fp32 with the fused depthwise producer)
 * `ksplit` > 1: that many workgroups share the K loop of every tile (needs `sk_ws`; the count is a function of the shape and
 * of fixed constants only), and `reduce` says where their sums meet: in splitk_reduce_kernel, a second launch that adds
 * them in share order, or inside the launch, where the last share to arrive adds them in share order. */
enum { UAVSAL_ROUTE_PRESPLIT = 1, UAVSAL_ROUTE_DWPROJ, UAVSAL_ROUTE_STREAMK, UAVSAL_ROUTE_K32, UAVSAL_ROUTE_F32_DMA,
       UAVSAL_ROUTE_STAGED };
enum { UAVSAL_REDUCE_NONE = 0, UAVSAL_REDUCE_LAUNCH, UAVSAL_REDUCE_IN_LAUNCH };
typedef struct uavsal_conv_route {
    int32_t family;   /* UAVSAL_ROUTE_* */
    int32_t tile;     /* 1 .. 11, see uavsal_conv_desc.tile */
    int32_t dwproj;   /* 0, or the output-channel tile of the DWPROJ instance: 32 / 64 / 128 / 256 */
    int32_t streamk;  /* workgroups of the stream-K launch, 0 = whole tiles */
    int32_t ksplit;   /* K shares per tile, 1 = none */
    int32_t reduce;   /* UAVSAL_REDUCE_* */
} uavsal_conv_route;
/* fills `*r` for `d`; no launch and no pointer of `d` is read (their alignment is).  0, or UAVSAL_EINVAL (null / non-positive size) */
int uavsal_conv_route_of(const uavsal_conv_desc* d, uavsal_conv_route* r);
/* single fields of the route, 0 where the descriptor has none: tile; family == PRESPLIT; dwproj; streamk */
int uavsal_conv_tile(const uavsal_conv_desc* d);
int uavsal_conv_uses_split(const uavsal_conv_desc* d);
int uavsal_conv_dwproj(const uavsal_conv_desc* d);
int uavsal_conv_streamk_grid(const uavsal_conv_desc* d);

/*
 * Depthwise 3x3 convolution + folded BatchNorm + ReLU6, NHWC, stride 1 or 2,
 * dilation d (padding = d), one launch for the whole batch.
 * Replaces: the `groups=hidden_dim` BasicConv2d of dwBlock (model.py:92) and
 * torchvision InvertedResidual's depthwise ConvBNReLU.
 * w9c is tap-major: w9c[(ky*3+kx)*C + c] = weight[c, 0, ky, kx].
 * Ho = (H - 1) / stride + 1, Wo likewise (pad = dilation, kernel 3).
 * stride 2 requires dilation 1.
 */
typedef struct uavsal_dw_desc {
    const float* in;   int32_t ldi;
    const float* w9c;  const float* scale;  const float* bias;
    float*       out;  int32_t ldo;
    int32_t n_img, H, W, C, stride, dilation, act;
    /* optional: write the result as a split shadow (see uavsal_conv_desc) INSTEAD of fp32 -- the only consumer
     * of a depthwise output is the projection GEMM (model.py:94).  `out` may then be NULL.  dilation 1 only. */
    void* out_split;  int32_t ldos;
    /* optional: several dilated branches of the SAME map in one launch (the three dilated ASPP depthwise convs, model.py:125-127,
     * on the channel slices of their merged expand): dil_group_c > 0 (a multiple of 4, C <= 4 * dil_group_c) gives channel c the
     * dilation dil_groups[c / dil_group_c]; `dilation` is then ignored.  Stride 1, no split output. */
    int32_t dil_group_c;  int32_t dil_groups[4];
} uavsal_dw_desc;

int uavsal_dw3x3(const uavsal_dw_desc* d, uavsal_stream_t stream);
/* kernel instance `uavsal_dw3x3` will use for this descriptor; no launch.  1: dw3x3_kernel<1,4,4> (4x4 output
 * patch per thread), 2: <1,2,2>, 3: <2,2,2> (stride 2), 4: dw3x3_dilated_kernel (one pixel per thread),
 * 16 / 32: dw3x3_map_lds_kernel<CB, 256> (whole map of a CB-channel slab staged in LDS by LDS-DMA; small maps, any
 * dilation), + 512 (528 / 544) for its 512-thread instance (slabs of >= 2048 float4 items),
 * 2048: dw3x3_rowclass_kernel<256> (merged dilated branches on a map too big for 32-channel whole-map slabs: a workgroup stages
 * the rows of one residue class oy % dilation for a 32..256-channel slab) */
int uavsal_dw_variant(const uavsal_dw_desc* d);

/*
 * Depthwise 3x3 (stride 1, pad 1) + BN + ReLU6 followed by a 1x1 projection to ONE channel + BN + activation, one launch:
 *   out[pixel] = act(scale2 * sum_c w2[c] * relu6(scale[c] * dw3x3(in)[pixel, c] + bias[c]) + bias2)
 * Replaces the depthwise BasicConv2d + pw-linear conv + BN of dwBlock(256 -> 1) = conv_out_st and the final sigmoid
 * (model.py:92-96, 333-334, 372-373): a dot product per pixel, bandwidth-bound on the expanded tensor.  Exact fp32
 * whatever the GEMM precision of the plan; the summation order is a function of C only.
 * C % 256 == 0, C <= 2048; w9c tap-major as in uavsal_dw_desc; scale2 / bias2 point at ONE value each (device memory).
 * act: UAVSAL_ACT_NONE | UAVSAL_ACT_RELU6 | UAVSAL_ACT_SIGMOID.
 */
typedef struct uavsal_dw_dot_desc {
    const float* in;   int32_t ldi;                              /* [n_img, H, W, C] NHWC, row pitch ldi floats */
    const float* w9c;  const float* scale;  const float* bias;   /* depthwise taps [9][C], folded BN [C] */
    const float* w2;   const float* scale2; const float* bias2;  /* projection weights [C]; folded BN of its one output */
    float*       out;  int32_t ldo;                              /* [n_img * H * W] values, ldo floats apart */
    int32_t n_img, H, W, C, act;
} uavsal_dw_dot_desc;

int uavsal_dw3x3_dot(const uavsal_dw_dot_desc* d, uavsal_stream_t stream);

/*
 * Fused inverted-residual block: pw-expand + BN + ReLU6 -> depthwise 3x3 (stride 1 / 2, pad 1) + BN + ReLU6 ->
 * pw-linear + BN [+ x], ONE launch, the 6x-expanded tensors stay in LDS.  Replaces a whole torchvision
 * InvertedResidual / dwBlock (model.py:74-103, model_feature.py:62-66) where the block is bandwidth-bound:
 * instances exist for (Cin, hidden, Cout, stride) of MobileNetV2 features[1..7] -- (32,32,16,1) with w1 == NULL
 * (t = 1: no expand conv), (16,96,24,2), (24,144,24,1), (24,144,32,2), (32,192,32,1), (32,192,64,2);
 * uavsal_fused_ir_supported tells.  Exact fp32 FMA arithmetic whatever the GEMM precision of the plan.
 * Weights (host-packed, fp32): w1 [Cin][hidden] (= conv weight transposed), wd [9][hidden] tap-major as in
 * uavsal_dw_desc, w2 [hidden][Cout]; scale* / bias* are the folded BatchNorms.  res (or NULL) is the block
 * input for the residual connection (stride 1, Cin == Cout): out = bn3(...) + res.  in / out / res rows and every
 * per-channel vector are read and written 16 bytes at a time: 16-byte aligned bases, ld* multiples of 4.
 */
typedef struct uavsal_fused_ir_desc {
    const float* in;   int32_t ldi;
    const float* w1;   const float* scale1;  const float* bias1;      /* NULL for a block without expand conv */
    const float* wd;   const float* scale_d; const float* bias_d;
    const float* w2;   const float* scale2;  const float* bias2;
    const float* res;  int32_t ldr;
    float*       out;  int32_t ldo;
    int32_t n_img, H, W, Cin, hidden, Cout, stride;
    int32_t tile;                /* output patch per workgroup: 0 = by the launch size, 1 = 4x16, 2 = 16x16 (stride 1) / 8x16 (stride 2) */
} uavsal_fused_ir_desc;

int uavsal_fused_ir(const uavsal_fused_ir_desc* d, uavsal_stream_t stream);
/* 0: no instance.  1: an instance of the small-channel kernel (features[1..7]); w1 is [Cin][hidden], w2 [hidden][Cout]
 * (the 1x1 weights transposed).  2: an instance of the mid-channel kernel (csrc/fused_mid.hip: stride 1, (Cin, hidden, Cout)
 * in {(64,384,64), (64,384,96), (64,384,32), (96,576,96)}); w1 is [hidden][Cin], w2 [Cout][hidden] -- the conv weights' own
 * layout -- 16-byte aligned.  No launch. */
int uavsal_fused_ir_supported(const uavsal_fused_ir_desc* d);

/*
 * Stem: dense 3x3 stride-2 pad-1 convolution 3 -> 32 + BatchNorm + ReLU6 reading the
 * caller's NCHW fp32 frames and writing NHWC.  Replaces torchvision
 * mobilenet_v2().features[0] as run by ReMobileNetV2.forward (model_feature.py:63).
 * w is [27][32]: w[(ci*9 + ky*3 + kx)*32 + co] = weight[co, ci, ky, kx].
 * If `in_u8` is non-NULL it is used instead of `in`: uint8 RGB frames [n,3,H,W] that are
 * normalised on load, (v/255 - mean[c]) / stdv[c]  (utils_data.py:43-65 normalize_data).
 */
typedef struct uavsal_stem_desc {
    const float*   in;     /* [n_img, 3, H, W] fp32 NCHW, or NULL */
    const uint8_t* in_u8;  /* [n_img, 3, H, W] uint8, or NULL */
    const float* w;  const float* scale;  const float* bias;
    float* out;  int32_t ldo;            /* [n_img, Ho, Wo, 32] */
    int32_t n_img, H, W;
    float mean[3], stdv[3];
} uavsal_stem_desc;

int uavsal_stem_conv(const uavsal_stem_desc* d, uavsal_stream_t stream);

/*
 * Bilinear resize, align_corners=True, NHWC, writing into a channel slice.
 * Replaces F.interpolate(..., mode='bilinear', align_corners=True) at model.py:152-153
 * and :360, and -- through the source-image map -- `cb_cxt.repeat(time_dims,1,1,1)`
 * (model.py:361):  source image of output image n is (n % src_mod) / src_div.
 *   reference semantics (tiling quirk): src_mod = B, src_div = 1
 *   batched clips:                      src_mod = n_out, src_div = T
 *   plain resize:                       src_mod = n_out, src_div = 1
 */
typedef struct uavsal_bilinear_desc {
    const float* in;  int32_t ldi;  int32_t Hi, Wi;
    float* out;       int32_t ldo;  int32_t Ho, Wo;
    int32_t n_out, C, src_mod, src_div;
    void* out_split;  int32_t ldos;              /* optional split shadow, written IN ADDITION to `out` */
} uavsal_bilinear_desc;

int uavsal_bilinear_ac(const uavsal_bilinear_desc* d, uavsal_stream_t stream);

/*
 * Temporal neighbour differences of teConv_sub (model.py:194-200), per sequence of
 * `seq_len` consecutive images: out[:, 0:C] = x[t]-x[t-1] (t=0: x[1]-x[0]);
 * out[:, C:2C] = x[t]-x[t+1] (t=last: x[last-1]-x[last]).  seq_len >= 2.
 */
typedef struct uavsal_tdiff_desc {
    const float* in;  int32_t ldi;
    float* out;       int32_t ldo;
    int32_t n_img, HW, C, seq_len;
} uavsal_tdiff_desc;

int uavsal_tdiff(const uavsal_tdiff_desc* d, uavsal_stream_t stream);

/*
 * Winograd F(R x R, 3x3) transforms (R = 2 or 4, P = R + 2) of a dense 3x3 convolution with stride 1 and padding 1
 * (csrc/winograd.hip), fp32.
 *   uavsal_wino_input : `in` NHWC [n_img, H, W, C] (row stride ldi)  ->  `out` = V[P*P][Mp][ldo]: plane k = P i + j holds
 *                       (B^T d B)_{ij} of every R x R output tile (tile = (image, ty, tx), row-major), channels C.
 *   uavsal_wino_output: `in` = M[P*P][Mp][ldi] (the P*P GEMM results, channels C = Cout)  ->  `out` NHWC
 *                       [n_img, H, W, C]: y = A^T m A, then scale / bias (or NULL), ACT_NONE / ACT_RELU6, optional residual
 *                       (EPI_AFFINE), or the ConvTWA update h_t = g x_t + (1 - g) h_{t-1}, g = sigmoid(y + aux) with
 *                       res = x_t, hprev = h_{t-1} (EPI_TWA).
 * Mp (rows per plane) >= n_img * ceil(H/R) * ceil(W/R), a multiple of 128; rows past the tiles are not written.
 * The GEMM between them: uavsal_conv_gemm with a = V, n_img = P*P, H = Mp, W = 1, taps = 1, w = the P*P
 * transformed filter matrices (G g G^T)_k packed one after another, w_group_stride = their size in floats
 * (packing.pack_wino_weight).  Image strides are in pixels, 0 = H * W.
 */
typedef struct uavsal_wino_desc {
    const float* in;   int32_t ldi;  int64_t in_img_stride;
    float* out;        int32_t ldo;  int64_t out_img_stride;
    int32_t n_img, H, W, C;
    int64_t Mp;
    int32_t R;                   /* output tile: 2 = F(2x2, 3x3), 16 planes; 4 = F(4x4, 3x3), 36 planes */
    const float* scale; const float* bias;
    int32_t act, epi;
    const float* res;   int32_t ldr;  int64_t res_img_stride;
    const float* aux;   int32_t ldx;  int64_t aux_img_stride;
    const float* hprev; int32_t ldh;  int64_t h_img_stride;
    /* uavsal_wino_input only, n_seg = 1..3 (else 0 and `in` as above): the input is the channel concatenation of n_seg tensors,
     * seg_in[s] = [n_img][seg_H[s]][seg_W[s]][seg_ld[s]] NHWC with seg_c[s] channels (sum = C).  A segment on a map of another
     * size is resized to H x W on the fly, bilinear with align_corners=True, with uavsal_bilinear_ac's arithmetic -- the head of
     * the SRF-Net feeds conv_last with cat[interpolate(x5), interpolate(x4), lv3] (reference model.py:151-156): neither the
     * resized maps nor the concat buffer exist then.  `in`, `ldi`, `in_img_stride` are ignored. */
    int32_t n_seg;
    const float* seg_in[3];  int32_t seg_ld[3], seg_c[3], seg_H[3], seg_W[3];
} uavsal_wino_desc;

int uavsal_wino_input(const uavsal_wino_desc* d, uavsal_stream_t stream);
int uavsal_wino_output(const uavsal_wino_desc* d, uavsal_stream_t stream);
/* The output transform of an F(2x2) ConvTWA step whose previous state is all +0 bits: M and y are then +0 as well, so neither
 * the M planes nor `hprev` are loaded (both must still be named); bit-identical to uavsal_wino_output on such a state with
 * finite weights.  UAVSAL_ESHAPE unless R = 2 and epi = UAVSAL_EPI_TWA. */
int uavsal_wino_output_zero_h(const uavsal_wino_desc* d, uavsal_stream_t stream);
/* Seam of the F(2x2) ConvTWA recurrence: uavsal_wino_output(xout) followed by uavsal_wino_input(xin) as ONE launch that writes
 * exactly the bytes the two launches write, bit for bit -- h_t into `xout->out` and the V planes (rows of real tiles) into
 * `xin->out` -- without reading h_t back.  Taken when `xout` is an EPI_TWA output transform without scale / bias / activation
 * and `xin` the input transform of the next step: R = 2 in both, xin->in == xout->out with the same row stride, image stride,
 * n_img, H, W, C and Mp, no segments.  Anything else is refused and nothing is launched: the status the transforms themselves
 * give for a bad descriptor (UAVSAL_EINVAL, UAVSAL_EALIGN: C % 4 != 0, ...), else UAVSAL_ESHAPE (R = 4, an affine epilogue,
 * two transforms that are not consecutive).  _check: the same answer without a launch.  _zero_h: step t in the zero-h form. */
int uavsal_wino_seam(const uavsal_wino_desc* xout, const uavsal_wino_desc* xin, uavsal_stream_t stream);
int uavsal_wino_seam_zero_h(const uavsal_wino_desc* xout, const uavsal_wino_desc* xin, uavsal_stream_t stream);
int uavsal_wino_seam_check(const uavsal_wino_desc* xout, const uavsal_wino_desc* xin);

/* Sum over groups of T consecutive images (model.py:357-358): out[b] = sum_t in[b*T+t]. */
typedef struct uavsal_tsum_desc {
    const float* in;  int32_t ldi;
    float* out;       int32_t ldo;
    int32_t n_groups, T, HW, C;
} uavsal_tsum_desc;

int uavsal_tsum(const uavsal_tsum_desc* d, uavsal_stream_t stream);

/*
 * Layout change between the caller's NCHW tensors (priors cb[0], cb[1], recurrent
 * state; Demo_Test.py:14-27,85-86) and the NHWC working buffers.
 * to_nhwc != 0: nchw -> nhwc (channels C..Cpad-1 of the destination are zero-filled),
 * else nhwc -> nchw.  `ld` is the NHWC channel stride.
 */
typedef struct uavsal_layout_desc {
    const float* in;  float* out;
    int32_t n_img, C, HW, ld, to_nhwc, Cpad;
} uavsal_layout_desc;

int uavsal_layout(const uavsal_layout_desc* d, uavsal_stream_t stream);

/*
 * Output post-processing of the caller, replacing per frame
 * postprocess_predictions (utils_data.py:289-303: cv2.resize INTER_LINEAR to the source frame
 * size, centre crop, `img / max(img) * 255`) and np2mat/im2uint8 (utils_data.py:68-82: clip,
 * round half to even, uint8) as used at Demo_Test.py:89-91.
 * in: [n_img, h, w] fp32 maps; out: [n_img, H, W] uint8; scratch: >= 4*n_img bytes (zeroed here).
 */
typedef struct uavsal_post_desc {
    const float* in;  uint8_t* out;  void* scratch;
    int32_t n_img, h, w, H, W;
} uavsal_post_desc;

int uavsal_postprocess(const uavsal_post_desc* d, uavsal_stream_t stream);

/*
 * Input letterboxing of the caller, replacing per frame `padding(img, shape_r, shape_c, 3)` (utils_data.py:321-343,
 * called from preprocess_videos, :255-287) and the BGR -> RGB swap behind it (`ims[:, :, :, [2, 1, 0]]`, :269-270):
 * a source-size uint8 frame h0 x w0 is resized with cv2.resize's 8-bit INTER_LINEAR rule (fixed point, 11-bit
 * weights; csrc/letterbox.hip states it) to R x new_c (if h0 / R > w0 / C: new_c = w0 * R / h0, placed at column
 * (C - new_c) / 2) or to new_r x C (new_r = h0 * C / w0, placed at row (R - new_r) / 2); everything outside is 0.
 * The library computes the geometry.  cv2 was not available to pin the rule: it is pinned by known answers that
 * follow from it (tests/letterbox_ref.py), not by outputs of cv2.
 * src: layout UAVSAL_LETTERBOX_HWC = interleaved [n_img, h0, w0, 3] (what a decoder produces) or UAVSAL_LETTERBOX_CHW
 * = planar [n_img, 3, h0, w0]; a row is dense, rows are row_pitch bytes apart, planes plane_pitch (planar only),
 * images img_pitch: a slice of a larger buffer works and no alignment is required (the kernel reads the 16-byte
 * aligned ranges that enclose each row).  swap_rb != 0: output plane 0 is source channel 2 and the other way round.
 * dst: [n_img, 3, R, C] uint8 planar, dense -- what uavsal_stem_desc.in_u8 reads.  ONE launch, bars included; no
 * allocation, no synchronisation.  UAVSAL_ESHAPE: a degenerate picture (new_r or new_c = 0), pitches smaller than
 * what they separate, n_img > 65535, or source rows too long for the LDS staging (8 C + 6 w0 bytes + padding
 * above 160 KB).
 */
#define UAVSAL_LETTERBOX_HWC 0
#define UAVSAL_LETTERBOX_CHW 1

typedef struct uavsal_letterbox_desc {
    const uint8_t* src;  uint8_t* dst;
    int64_t row_pitch, plane_pitch, img_pitch;     /* bytes */
    int32_t n_img, h0, w0, R, C;
    int32_t layout, swap_rb;
} uavsal_letterbox_desc;

int uavsal_letterbox_u8(const uavsal_letterbox_desc* d, uavsal_stream_t stream);

/*
 * Heat-map overlay frames of the reference's visualisation: the coloured path of `visual_vid` (utils_vis.py:103-212,
 * with_color=1, with and without with_fix) and `heatmap_overlay` / `visual_img` (:34-101) as the case without resizes.
 * Per frame: the BGR uint8 frame h0 x w0 and the uint8 map map_h x map_w go to mid_h x mid_w with cv2.resize's 8-bit
 * INTER_LINEAR rule (the rule of uavsal_letterbox_u8; the identity at equal sizes), map_color = lut[map],
 * o = 0.8 * (1 - m ** 0.8) * img + m * map_color with img, m, map_color normalised by their per-frame maxima (in double,
 * EPS = 2.2204e-16), o goes to out_h x out_w with cv2.resize's float INTER_LINEAR rule (half-pixel centres in double cast
 * to float32, float32 weights, products and sums in double, horizontal pass then vertical), the nonzero pixels of the
 * frame's fixation map are scattered to the output size (resize_fixation, :16-31), dilated 5x5 and set to 1, and
 * o / max(o) * 255 is clipped, rounded half to even and stored as interleaved BGR uint8 [n_img][out_h][out_w][3].
 * A frame the reference leaves undefined (max(o) == 0 or max(map_color) == 0: 0 / 0) is written as zeros.
 * csrc/overlay.hip states the rules line by line; neither resize rule was checked against cv2 itself.
 * frames: layout / row_pitch / plane_pitch / img_pitch as in uavsal_letterbox_desc: any byte offset; the channel
 * order is kept (BGR in, BGR out).  map: dense [n_img][map_h][map_w] images map_img_pitch bytes apart, any byte offset.
 * fix: NULL, or dense uint8 [n_img][fix_h][fix_w] (nonzero = a fixation), any byte offset.  lut: [256][3] uint8 BGR.
 * ws: uavsal_overlay_workspace_bytes(d) bytes, 256-byte aligned; the call clears what it needs cleared.
 * UAVSAL_ESHAPE: rows longer than the LDS staging allows (or more than 65535 frames).  Mid / out sizes are the caller's:
 * the visual_vid geometry is host arithmetic (vis.visual_geometry).  Bitwise reproducible: integer atomics only.
 */
typedef struct uavsal_overlay_desc {
    const uint8_t* frames;  int64_t row_pitch, plane_pitch, img_pitch;     /* bytes */
    const uint8_t* map;  int64_t map_img_pitch;
    const uint8_t* fix;  const uint8_t* lut;
    uint8_t* out;  void* ws;  int64_t ws_bytes;
    int32_t n_img, layout, h0, w0, map_h, map_w, fix_h, fix_w;
    int32_t mid_h, mid_w, out_h, out_w;
} uavsal_overlay_desc;

int64_t uavsal_overlay_workspace_bytes(const uavsal_overlay_desc* d);
int uavsal_overlay_u8(const uavsal_overlay_desc* d, uavsal_stream_t stream);

/*
 * Strided row copy, device to device: `rows` rows of `row_floats` contiguous floats (a multiple of 4),
 * row r read at in + r*in_pitch and written at out + r*out_pitch (pitches in floats).  Used by the
 * persistent-state mode to carry h_last (NHWC, last frame of every clip of the ConvTWA history, which
 * IS the state: model_convlstm.py:377-381) into the resident state buffer that step 0 of the next call
 * reads -- the device-side form of `x_state = [out_state[0].detach()]` (Demo_Test.py:86).
 */
typedef struct uavsal_copy_desc {
    const float* in;  float* out;
    int64_t in_pitch, out_pitch, row_floats;  int32_t rows;
} uavsal_copy_desc;

int uavsal_copy_rows(const uavsal_copy_desc* d, uavsal_stream_t stream);

/*
 * Fill `n` 32-bit words at `out` with the bit pattern `bits`.  The activation arena's debug mode records one after
 * the last reader of every buffer (bits = a quiet NaN), so that a kernel that still reads a released range -- or a
 * later buffer placed over a live one -- shows up as NaN in the maps instead of as a plausible number
 * (the reference keeps O(group) memory per call, Demo_Test.py:75-86; here liveness does: engine.py).
 */
typedef struct uavsal_fill_desc {
    uint32_t* out;  int64_t n;  uint32_t bits;
} uavsal_fill_desc;

int uavsal_fill(const uavsal_fill_desc* d, uavsal_stream_t stream);

/*
 * Error guard: the last launch of a forward.  If `*err` is non-zero (a kernel of this run reported
 * UAVSAL_ERR_*), every listed buffer is overwritten with NaN, so that no caller can mistake the result
 * for a saliency map; `*err` is then copied to `*host_err` (a device-visible host word, may be NULL).
 * The caller-facing contract (SURVEY.md 8(b) "Errors: never silent") is completed on the host by
 * uavsal_plan_status.
 */
typedef struct uavsal_guard_desc {
    const int32_t* err;  int32_t* host_err;
    float* buf[3];  int64_t n[3];          /* fp32 buffers to poison; unused entries NULL / 0 */
} uavsal_guard_desc;

int uavsal_guard(const uavsal_guard_desc* d, uavsal_stream_t stream);

/* ---- saliency scoring: the metrics of the reference's scorer (utils_score_torch.py:17, 53-229) ----------------
 * One descriptor covers a batch of F frames of N = H*W pixels.  `sal` is uint8 (sal_u8 = 1) or fp32, `fix_loc` uint8
 * (loc_u8 = 1) or fp32, `fix_map` fp32, all [F][N] dense.  Metric ids are the positions in the reference's keys_order:
 * 0 AUC_shuffled, 1 NSS, 2 AUC_Judd, 3 AUC_Borji, 4 KLD, 5 SIM, 6 CC.
 *
 * uavsal_score_stats: per-frame statistics into stats[F][UAVSAL_SCORE_NSTAT] (double): 0 min / 1 max of the map,
 *   2 min / 3 max of the map + jitter (= 0 / 1 without jitter), 4 sum of the map, 5 min / 6 max / 7 sum of fix_map,
 *   8 sum of fix_loc, 9 count of fix_loc > 0.5, 10 count of fix_loc != 0.  The host reads them to draw the random
 *   samples (the draws stay on the host, in the reference's order).
 * uavsal_score_run: everything else, after uavsal_score_stats on the same descriptor: out[F][n_keys] (fp32, column k =
 *   metric keys[k]).  AUC-Judd reads the fixation values gathered into runs of at most UAVSAL_SCORE_RUN: fix_off[F+1]
 *   is the prefix of the per-frame fixation counts (0 for a frame whose AUC-Judd is NaN), run_off[F+1] the prefix of
 *   ceil(count / UAVSAL_SCORE_RUN); both device arrays, totals in total_fix / total_runs.  samp[0] (AUC_shuffled) and
 *   samp[1] (AUC_Borji) hold pixel indices: frame f at samp_off[s][f], UAVSAL_SCORE_REPS rows of n indices
 *   (n = (samp_off[s][f+1] - samp_off[s][f]) / REPS; n = 0: no draw, the score is NaN).  nan_rows != 0: a frame whose
 *   map, fix_map or fix_loc is all zero scores NaN everywhere (utils_score_torch.py:565-571).
 * Scores are bitwise reproducible: no float atomics, fixed reduction orders.
 */
#define UAVSAL_SCORE_NSTAT 16
#define UAVSAL_SCORE_REPS  100
#define UAVSAL_SCORE_RUN   4096
#define UAVSAL_SCORE_NKEY  7

typedef struct uavsal_score_desc {
    const void* sal;  const void* fix_loc;  const float* fix_map;
    const float* jitter;                  /* [F][N] fp32 term added to the map for AUC-Judd, or NULL */
    int32_t sal_u8, loc_u8, n_frames, n_pix;
    double* stats;                        /* [F][UAVSAL_SCORE_NSTAT] */
    const int64_t* fix_off;  const int64_t* run_off;  int64_t total_fix;  int32_t total_runs;
    int32_t nan_rows;
    const int32_t* samp[2];  const int64_t* samp_off[2];  int64_t n_samp[2];
    void* ws;  int64_t ws_bytes;          /* workspace, uavsal_score_workspace_bytes() */
    float* out;  int32_t n_keys;  int32_t keys[UAVSAL_SCORE_NKEY];
} uavsal_score_desc;

int64_t uavsal_score_workspace_bytes(const uavsal_score_desc* d);
int uavsal_score_stats(const uavsal_score_desc* d, uavsal_stream_t stream);
int uavsal_score_run(const uavsal_score_desc* d, uavsal_stream_t stream);

/* ---- training criterion and gaze ground truth: the pieces of the reference's `val` phase around the forward ----------
 * (Demo_Train_Test.py:87-156; csrc/loss.hip states the rules line by line)
 *
 * uavsal_gaze_prepare: y_gaze [n_img][2][h][w] fp32 from the source-size uint8 fixMap / fixLoc of a video, replacing per
 * frame `padding(fixMap, h, w, 1)` and `padding_fixation(fixLoc, h, w)` (utils_data.py:229-253, 321-385).
 *   channel 0: the map resized with cv2.resize's 8-bit INTER_LINEAR rule (csrc/resize_u8.h, the rule of
 *     uavsal_letterbox_u8 with its geometry), centred between zero bars; values stay 0..255.
 *   channel 1: every non-zero source pixel (r, c) writes 1 at (rint(r * rows / h0), rint(c * cols / w0)) of the picture
 *     area (rows x cols, the letterbox geometry; product and rint in double, an index equal to rows / cols pulled in by
 *     one); with h0 == h and w0 == w the source VALUES are copied instead (utils_data.py:366-367 returns the input).
 *   flags [n_img][2] uint8: 1 where a channel of a frame holds a non-zero (np.any(y_gaze, axis=(2, 3))).
 * Both sources are read in place: element (img, r, c) at base + img * img_pitch + r * row_pitch + c * col_pitch bytes, any
 * non-negative pitches (so [F,H0,W0] and the .mat layouts [H0,W0,1,F] / [H0,W0,F] are views).  The caller zeroes `out`
 * and `flags` on the stream first; ONE launch; writers of one cell all store the same value: no atomics.
 * UAVSAL_ESHAPE: a degenerate picture, or n_img > 65535.
 */
typedef struct uavsal_gaze_desc {
    const uint8_t* fix_map;  int64_t map_row_pitch, map_col_pitch, map_img_pitch;     /* bytes */
    const uint8_t* fix_loc;  int64_t loc_row_pitch, loc_col_pitch, loc_img_pitch;
    float* out;  uint8_t* flags;
    int32_t n_img, h0, w0, h, w;
} uavsal_gaze_desc;

int uavsal_gaze_prepare(const uavsal_gaze_desc* d, uavsal_stream_t stream);

/*
 * The criterion of the reference (loss_functions.py:43-50, 64-86): per frame, on pred [B][1][h][w] and truth [B][2][h][w]
 * (channel 0 the fixation map, channel 1 the fixation points), dense fp32,
 *   kl  = sum t' * log(t' / (p' + EPS) + EPS),  t' = t / (sum t + EPS),  p' = p / (sum p + EPS)
 *   cc  = r1 / (r2 + EPS) of the standardised maps ((x - mean) / (std + EPS), unbiased std)
 *   nss = sum(f * p_std) / (sum f + EPS)
 * and out[0..2] = their means over the B frames, out[3] = w_kl * out[0] + w_cc * out[1] + w_nss * out[2]: (10, -2, -1) is
 * loss_fu, (10, 0, 0) loss_kl.  Everything is accumulated in double and rounded to fp32 once.
 * uavsal_loss_fu: one workgroup per frame writes stats[B][UAVSAL_LOSS_NSTAT] (double: 0 kl, 1 cc, 2 nss, 3 sum p,
 *   4 mean p, 5 mean t, 6 sum (p - mean)^2, 7 sum (t - mean)^2, 8 sum (t - mean)(p - mean), 9 sum f (p - mean), 10 sum f,
 *   11 sum A p' with A = d kl / d p', 12 sum t), then a second one-wave launch takes the means over the frames in a
 *   fixed order: no float atomics, two runs are bit-identical.  No allocation, no synchronisation.
 * uavsal_loss_fu_grad: grad [B][1][h][w] = *grad_out * d out[3] / d pred from pred, truth and the saved stats, one pass
 *   over the pixels, ONE launch.  `grad_out` is a device scalar (autograd's incoming gradient).  A term whose weight
 *   is 0 is left out.  A frame of constant predictions has std 0: its cc / nss gradient is NaN, as in the reference.
 * UAVSAL_ESHAPE: fewer than 2 pixels per frame.
 */
#define UAVSAL_LOSS_NSTAT 16

typedef struct uavsal_loss_desc {
    const float* pred;  const float* truth;
    double* stats;                        /* [B][UAVSAL_LOSS_NSTAT] */
    float* out;                           /* [4] (forward) */
    const float* grad_out;  float* grad;  /* (backward) */
    int32_t n_img, n_pix;
    double w_kl, w_cc, w_nss;
} uavsal_loss_desc;

int uavsal_loss_fu(const uavsal_loss_desc* d, uavsal_stream_t stream);
int uavsal_loss_fu_grad(const uavsal_loss_desc* d, uavsal_stream_t stream);

/* ---- observed prior of a dataset: the mean fixation map of a video (utils_data.py:497-520, 569-574) ------------------
 * (csrc/prior.hip states the rules and the sizing)
 *
 * uavsal_prior_accumulate: acc[r][c] += sum over the n_img frames of frames[img][r][c], int32 sums of uint8 values.
 *   Element (img, r, c) of the frames at base + img * img_pitch + r * row_pitch + c * col_pitch BYTES, any non-negative
 *   pitches and any byte offset, read in place (the contract of uavsal_gaze_prepare); element (r, c) of the sums at
 *   acc + r * acc_row_pitch + c * acc_col_pitch ELEMENTS.  The caller zeroes `acc` once per video and may add any number
 *   of chunks; it keeps the total below 2^31 / 255 frames.  A plane that is contiguous in memory in either pixel order
 *   (rows of w0 bytes, or MATLAB's columns of h0 bytes), frames a multiple of 16 bytes apart and an `acc` in the same
 *   pixel order stream at 16 bytes per lane; everything else is summed a byte at a time.  The frames are split into
 *   slabs of uavsal_prior_slab_frames() across the grid and the slabs meet in INTEGER atomic adds: the result does not
 *   depend on the order of arrival.  ONE launch, no allocation, no synchronisation.
 *   UAVSAL_EALIGN: acc not 4-byte aligned.  UAVSAL_ESHAPE: 255 * n_img or h0 * w0 does not fit an int32.
 * uavsal_prior_slab_frames: the slab length that call uses for a plane of `plane_pixels` and `n_img` frames (no launch;
 *   0 for non-positive arguments).  Never below UAVSAL_PRIOR_MIN_SLAB.
 * uavsal_prior_finish: out [h][w] uint8 = padding(q, h, w, 1) and, when `image` is not NULL, image [h0][w0] uint8 = q, the
 *   picture the reference writes as <video>.png, with
 *     m = acc / n_frames,   q = rint(255 * (m - min m) / (max m - min m + EPS))            EPS = 2.2204e-16
 *   in double, every operation rounded on its own, the product in front of the quotient, rint to even (np.mean, :517-518;
 *   cv2.imwrite's saturate_cast).  min / max are taken on the integer sums.  padding(): the geometry and the 8-bit
 *   INTER_LINEAR rule of uavsal_letterbox_u8, zero bars; every byte of `out` is written.  `ws`: two device words the
 *   call owns while it runs.  THREE launches (clear, min / max, map), no allocation, no synchronisation.
 *   UAVSAL_EALIGN: acc / ws not 4-byte aligned.  UAVSAL_ESHAPE: a degenerate picture, 255 * n_frames or h0 * w0 beyond int32.
 */
#define UAVSAL_PRIOR_MIN_SLAB 32

typedef struct uavsal_prior_acc_desc {
    const uint8_t* frames;  int64_t row_pitch, col_pitch, img_pitch;   /* bytes */
    int32_t* acc;  int64_t acc_row_pitch, acc_col_pitch;               /* elements */
    int32_t n_img, h0, w0;
} uavsal_prior_acc_desc;

typedef struct uavsal_prior_finish_desc {
    const int32_t* acc;  int64_t acc_row_pitch, acc_col_pitch;         /* elements */
    int32_t* ws;                                                       /* [2] */
    uint8_t* out;                                                      /* [h][w] */
    uint8_t* image;                                                    /* [h0][w0] or NULL */
    int32_t n_frames, h0, w0, h, w;
} uavsal_prior_finish_desc;

int uavsal_prior_accumulate(const uavsal_prior_acc_desc* d, uavsal_stream_t stream);
int uavsal_prior_finish(const uavsal_prior_finish_desc* d, uavsal_stream_t stream);
int uavsal_prior_slab_frames(int64_t plane_pixels, int32_t n_img);
int uavsal_prior_sizeof_desc(int which);  /* 0 prior_acc, 1 prior_finish (uavsal_sizeof_desc's list is closed at 20) */

/* ---- fine-tuning the ConvTWA recurrence: backward of model.rnn and of the frozen decoder (csrc/train.hip) --------------
 * All activations NHWC fp32, C = 256 hidden channels (anything else: UAVSAL_ESHAPE), one sequence per call.
 * Notation: x_t the recurrence input, h_t the output history (h_{-1} = h0), W = [W_x | W_h] along the input channels,
 *   z_t = conv3x3(W, cat[x_t, h_{t-1}]),  i_t = sigmoid(z_t),  h_t = i_t x_t + (1 - i_t) h_{t-1}   (model_convlstm.py:276-292)
 *
 * uavsal_twa_gate_bwd: one step of back-propagation through time, element-wise, ONE launch.  With g = G_t + carry (the
 *   direct gradient of h_t plus what step t+1 hands back; carry NULL = none):
 *     dz = g (x_t - h_{t-1}) i (1 - i),   carry_out = g (1 - i),   dx = g i  (dx NULL = not wanted)
 *   i and 1 - i are both computed from exp(-|z|), so neither loses its relative accuracy in a saturated gate.
 *   Rows of C floats `ld*` floats apart; dz, carry_out and dx may alias nothing they are computed from except that
 *   carry_out may be `carry`.  UAVSAL_EALIGN: a pointer or ld not 16-byte aligned.
 *
 * uavsal_twa_wgrad: dW[co][ci][ky][kx] = sum over t and pixels p of dz_t[p][co] * cat_t[p + (ky-1, kx-1)][ci], zero outside
 *   the picture, never across frames; cat_t is not materialised (ci < C reads x_t, ci >= C reads h_{t-1}; frame 0 reads h0).
 *   A GEMM whose reduction runs over the T*H*W pixels (M = C, N = 9 * 2C) on the exact-fp32 MFMA, 128 x 128 tiles.  The
 *   pixels are cut into chunks of UAVSAL_WGRAD_CHAIN = 1024: no MFMA accumulation chain is longer than that; a workgroup
 *   owns one tile and a share of whole chunks, adds its chunks' tiles in fp32 and writes the partial tile to `ws`.  A
 *   second launch sums the shares in a fixed order in double, rounds once and overwrites `out` [C][2C][3][3] or
 *   (`accumulate`) adds it to what is there.  No atomics: two calls return the same bits.  TWO launches, no allocation.
 *   `ws`: uavsal_twa_wgrad_workspace_bytes(d) bytes, 16-byte aligned (UAVSAL_EINVAL when ws_bytes is smaller).
 *
 * uavsal_dec_bwd: the input gradient of the middle of the frozen decoder conv_out_st (eval BatchNorm folded),
 *     e = ReLU6(s1 (W1 h) + b1),  d = ReLU6(s2 dw3x3(e) + b2),  y = sigmoid(s3 (w3 . d) + b3):
 *     ge[p][c] = s1[c] 1[0 < e[p][c] < 6] s2[c] sum over taps k of wd[k][c] t[p - (k - (1,1))][c],
 *     t[q][c]  = gy[q] y[q] (1 - y[q]) s3 w3[c] 1[0 < d[q][c] < 6]
 *   from the stored e and d (the masks are torch's: strict inequalities).  gy is read at
 *   img * gy_img_pitch + row * gy_row_pitch + col * gy_col_pitch elements; y is dense [n_img][H][W]; e, d, ge dense
 *   [n_img][H][W][C], C % 4 == 0; wd9 tap-major [9][C] as in uavsal_dw_desc.  ONE launch, memory bound.
 */
#define UAVSAL_WGRAD_CHAIN 1024

typedef struct uavsal_twa_gate_desc {
    const float* g;      int32_t ldg;       /* G_t */
    const float* carry;                     /* dense [n_pix][C] or NULL */
    const float* z;                         /* dense */
    const float* x;      int32_t ldx;
    const float* hprev;  int32_t ldh;
    float* dz;  float* carry_out;  float* dx;           /* dense; dx may be NULL */
    int64_t n_pix;  int32_t C;
} uavsal_twa_gate_desc;

typedef struct uavsal_twa_wgrad_desc {
    const float* dz;                        /* dense [T][H][W][C] */
    const float* x;      int32_t ldx;       /* [T][H][W] rows */
    const float* h;      int32_t ldh;       /* [T][H][W] rows: the history h_0 .. h_{T-1} (frame t reads h_{t-1}) */
    const float* h0;     int32_t ldh0;      /* [H][W] rows */
    float* ws;  int64_t ws_bytes;
    float* out;                             /* [C][2C][3][3] */
    int32_t T, H, W, C, accumulate;
} uavsal_twa_wgrad_desc;

typedef struct uavsal_dec_bwd_desc {
    const float* gy;  int64_t gy_img_pitch, gy_row_pitch, gy_col_pitch;
    const float* y;
    const float* e;  const float* d;
    const float* s1;  const float* wd9;  const float* s2;  const float* w3;  const float* s3;   /* s3: one float */
    float* ge;
    int32_t n_img, H, W, C;
} uavsal_dec_bwd_desc;

int uavsal_twa_gate_bwd(const uavsal_twa_gate_desc* d, uavsal_stream_t stream);
int64_t uavsal_twa_wgrad_workspace_bytes(const uavsal_twa_wgrad_desc* d);
int uavsal_twa_wgrad_shares(const uavsal_twa_wgrad_desc* d);   /* K shares per tile of that call (no launch) */
int uavsal_twa_wgrad(const uavsal_twa_wgrad_desc* d, uavsal_stream_t stream);
int uavsal_dec_bwd(const uavsal_dec_bwd_desc* d, uavsal_stream_t stream);
int uavsal_train_sizeof_desc(int which);  /* 0 twa_gate, 1 twa_wgrad, 2 dec_bwd (uavsal_sizeof_desc's list is closed at 20) */

/* ---- fine-tuning the ConvLSTM recurrence of UAVSAL_LSTM: backward of model.rnn (csrc/train_lstm.hip) -------------------
 * All activations NHWC fp32, one sequence per call, C hidden channels (C % 4 == 0, else UAVSAL_EALIGN; the model builds 256).
 * Notation: W = [W_x | W_h] [4C][2C][3][3], rows gate * C + c in gate order i, f, o, g (model_convlstm.py:111-126, no bias):
 *   cc_t = conv3x3(W, cat[x_t, h_{t-1}]),  i, f, o = sigmoid(cc_i, cc_f, cc_o),  g = tanh(cc_g),
 *   c_t = f c_{t-1} + i g,  h_t = o tanh(c_t).
 * `cc` and `dcc` are dense rows of 4C floats per pixel in that gate-major order: [gate][c] (what uavsal_conv_gemm writes for
 * the weight as the module holds it; the forward plan's own packed form interleaves the gates and is not read here).
 *
 * uavsal_lstm_scan: the cell-state history from the pre-activations of all frames, ONE launch: c_seq[t] = f_t c_{t-1} + i_t g_t
 *   for t = 0 .. T-1 with c_{-1} = c0 (NULL = zeros).  A lane owns four channels of one pixel and walks t itself.
 *
 * uavsal_lstm_gate_bwd: one step of back-propagation through time, element-wise, ONE launch.  With gh = G_t + carry_h (the
 *   direct gradient of h_t plus what step t+1 hands back through W_h; NULL = none), carry_c what step t+1 hands back through
 *   its forget gate (NULL = none) and tc = tanh(c_t):
 *     dc = carry_c + gh o (1 - tc^2)
 *     dcc_i = dc g i (1 - i),  dcc_f = dc c_{t-1} f (1 - f),  dcc_o = gh tc o (1 - o),  dcc_g = dc i (1 - g^2)
 *     carry_c_out = dc f
 *   The gates are recomputed from cc_t; s (1 - s) = e / (1 + e)^2 with e = exp(-|z|) and 1 - tanh^2 = 4 e2 / (1 + e2)^2 with
 *   e2 = exp(-2|z|), so every factor keeps its relative accuracy in a saturated gate.  Rows of G are `ldg` floats apart (a
 *   channel slice is read in place); everything else is dense.  carry_c_out may be `carry_c`; no other output may alias an
 *   input.  UAVSAL_EALIGN: C % 4, ldg % 4 or a pointer not 16-byte aligned; UAVSAL_EINVAL: a missing pointer, a size <= 0,
 *   ldg < C; UAVSAL_ESHAPE: more elements than one launch indexes.  No atomics, no allocation: two calls return the same bits.
 */
typedef struct uavsal_lstm_scan_desc {
    const float* cc;                        /* dense [T][n_pix][4C] */
    const float* c0;                        /* dense [n_pix][C] or NULL */
    float* c_seq;                           /* dense [T][n_pix][C] */
    int64_t n_pix;  int32_t T, C;
} uavsal_lstm_scan_desc;

typedef struct uavsal_lstm_gate_desc {
    const float* g;      int32_t ldg;       /* G_t */
    const float* carry_h;                   /* dense [n_pix][C] or NULL */
    const float* carry_c;                   /* dense [n_pix][C] or NULL */
    const float* cc;                        /* dense [n_pix][4C]: cc_t */
    const float* c;                         /* dense [n_pix][C]: c_t */
    const float* c_prev;                    /* dense [n_pix][C]: c_{t-1} */
    float* dcc;                             /* dense [n_pix][4C] */
    float* carry_c_out;                     /* dense [n_pix][C] */
    int64_t n_pix;  int32_t C;
} uavsal_lstm_gate_desc;

int uavsal_lstm_scan(const uavsal_lstm_scan_desc* d, uavsal_stream_t stream);
int uavsal_lstm_gate_bwd(const uavsal_lstm_gate_desc* d, uavsal_stream_t stream);
int uavsal_lstm_sizeof_desc(int which);   /* 0 lstm_scan, 1 lstm_gate (additions: UAVSAL_ABI_VERSION stays 20) */

/* ---- fine-tuning the decoder conv_out_st: its nine parameter gradients (csrc/train_decoder.hip) -----------------------
 * The decoder in eval mode, r = 1 / sqrt(var + eps), s = gamma r, b = beta - mu s per BatchNorm:
 *     u1 = W1 h, a1 = s1 u1 + b1, e = ReLU6(a1);  u2 = dw3x3(Wd, e), a2 = s2 u2 + b2, d = ReLU6(a2);
 *     a3 = s3 (w3 . d) + b3, y = sigmoid(a3).
 * With gy = d loss / d y:
 *     delta3[p]    = gy[p] y[p] (1 - y[p])
 *     delta2[p][c] = delta3[p] s3 w3[c] 1[0 < d[p][c] < 6]
 *     ga[p][c]     = 1[0 < e[p][c] < 6] s2[c] sum over taps k of wd[k][c] delta2[p - (k - (1,1))][c]      (= d loss / d a1:
 *                    what uavsal_dec_bwd writes when it is handed ones for s1)
 * and the sums over all n_img * H * W pixels p
 *     S3 = sum delta3,  G3[c] = sum delta3[p] d[p][c],  S2[c] = sum delta2[p][c],  S1[c] = sum ga[p][c],
 *     Gd[c][ky][kx] = sum delta2[p][c] e[p + (ky-1, kx-1)][c]   (zero outside the picture, never across frames),
 *     G1[c][j] = sum ga[p][c] h[p][j]
 * the gradients are
 *     W1[c][j]: s1[c] G1[c][j]    beta1: S1    gamma1[c]: r1[c] (sum_j W1[c][j] G1[c][j] - mu1[c] S1[c])
 *     Wd[c][k]: s2[c] Gd[c][k]    beta2: S2    gamma2[c]: r2[c] (sum_k Wd[c][k] Gd[c][k] - mu2[c] S2[c])
 *     W3[c]:    s3 G3[c]          beta3: S3    gamma3:    r3 (sum_c W3[c] G3[c] - mu3 S3)
 * The gamma gradients come from the UNSCALED sums: nothing divides by gamma or s (a channel with gamma = 0 has a zero
 * weight-gradient row and a non-zero gamma gradient).
 *
 * uavsal_pix_gemm: out[m][n] = fl(row_scale[m] G[m][n]) (+ the old value with `accumulate`), G[m][n] = sum over the K
 *   pixels p of a[p][m] b[p][n]; row p of a / b at p * lda / p * ldb floats (channel slices are read in place).  M and N
 *   multiples of 64 (multiples of 32: below; the last M tile and the last N tile may be half empty: nothing at or behind row
 *   M or column N is read, written or enters rowdot).  The tile loop and the K split of uavsal_twa_wgrad: chunks of
 *   UAVSAL_WGRAD_CHAIN pixels, shares of whole chunks for about 1024 workgroups over the ceil(M / 128) ceil(N / 128) tiles, partial
 *   tiles in `ws`; a second launch sums the shares in share order in double and rounds once.  row_scale NULL = 1.
 *   rowdot (optional, [M] doubles) = sum_n w[m][n] G[m][n] in double in a fixed order, w rows ldw floats apart.
 *   No atomics: two calls return the same bits.  TWO launches, no allocation.  UAVSAL_EALIGN: a, b, ws not 16-byte
 *   aligned or lda / ldb not a multiple of 4.
 *   M == 32 or N == 32, the other side a multiple of 32 from 128 to 512 (the 32-wide sides of an ST block: 32 x 256, 256 x 32, 32 x 384): a sibling
 *   kernel behind the same entry point, in which a WAVE owns one whole 32 x 32 tile (one v_mfma_f32_32x32x2_f32 accumulator,
 *   no padded half tile, operands read from global memory in the MFMA's own layout, not pipelined under the MFMAs: 14-18
 *   TFLOP/s measured at 20 frames of 45 x 80, profiles/train_st.md), four tiles to a workgroup; the same
 *   chunks, chains, shares rule (over ceil((M / 32)(N / 32) / 4) workgroups per share), workspace layout, reduction launch,
 *   row_scale, rowdot and accumulate.  Every call with M and N multiples of 64 keeps the kernel, grid, workspace and bits it
 *   had.  The same kernel takes M a multiple of 64 with N an odd multiple of 32, neither above 512 (the 1x1 convs of the
 *   SRF-Net head on c3 and c4: 64 x 32, 128 x 96); a last workgroup with fewer than four tiles leaves its other waves idle.
 *   Anything else (96 x 64: M is no multiple of 64; 32 x 64, 32 x 32: a 32-wide M below 128 columns; 1920 x 32: wider than
 *   512): UAVSAL_ESHAPE, as before.
 *   tails32 != 0 (opt-in; the field lies in what was the struct's tail padding, so a zeroed descriptor keeps every rule
 *   above, every refusal included): any M, N multiple of 32 that those rules refuse is taken as well -- the W1 / W3 gradients
 *   of MobileNetV2 blocks 8..17: 576 x 96, 960 x 160, 96 x 384, 96 x 576, 160 x 576, 160 x 960 -- by the 128 x 128 tile kernel,
 *   whose last tile of either side may then end at ANY quarter (32, 64, 96 rows or columns; nothing at or behind row M or
 *   column N is read, written or enters rowdot).  A shape the rules above take keeps its kernel, K split and bits with the
 *   flag set.  The K split of these shapes only: K is short there (4800 to 18400 pixels on 3 to 16 tiles), so a share is a
 *   whole number `ups` of UNITS of 128 pixels instead of chunks: units = ceil(K / 128), want = clamp(512 / tiles, 1, units)
 *   with tiles = ceil(M / 128) ceil(N / 128), ups = ceil(units / want), shares = ceil(units / ups)
 *   (uavsal_pix_gemm_shares returns it); share s owns pixels [s ups 128, (s + 1) ups 128) cut at K, its accumulation chains
 *   end every UAVSAL_WGRAD_CHAIN products counted from its first pixel.  Workspace: shares * M * N floats, [share][M][N], as
 *   for every other partition; the reduction launch, row_scale, rowdot and accumulate are the same code.
 * uavsal_dec_sums: per slab of picture rows the partial sums S3, G3, S2, Gd, S1 -> `ws` (doubles), from gy (pitched as in
 *   uavsal_dec_bwd_desc), y dense [n_img][H][W], e, d, ga dense [n_img][H][W][C], C % 256 == 0 (else UAVSAL_ESHAPE).
 *   delta3 and delta2 are formed in fp32 exactly as uavsal_dec_bwd forms them; every product is accumulated in double.
 *   ws layout: per slab UAVSAL_DEC_NSUM * C + 1 doubles: [0] G3, [1] S2, [2 + ky * 3 + kx] Gd, [11] S1, each [C], then S3.
 *   The slabs depend on the shape alone (uavsal_dec_sums_slabs / _slab_rows): bit-reproducible.  ONE launch.
 * uavsal_dec_finish: sums the slabs in slab order in double and writes the eight small gradients in the parameters' own
 *   layouts (g_wd [C][3][3], the others [C] or one element), each rounded once, overwritten or (`accumulate`) added to.
 *   rowdot: uavsal_pix_gemm's, with w = W1.  wd is the parameter [C][3][3], not the tap-major packing.  ONE launch.
 */
#define UAVSAL_DEC_NSUM 12

typedef struct uavsal_pix_gemm_desc {
    const float* a;  int32_t lda;           /* [K] rows of M floats */
    const float* b;  int32_t ldb;           /* [K] rows of N floats */
    const float* row_scale;                 /* [M] or NULL */
    const float* w;  int32_t ldw;           /* [M] rows of N floats (needed with rowdot) */
    double* rowdot;                         /* [M] or NULL */
    float* ws;  int64_t ws_bytes;
    float* out;  int32_t ldo;               /* [M] rows of N floats */
    int64_t K;  int32_t M, N, accumulate;
    int32_t tails32;                        /* 0: the rules above.  1: every other M, N multiple of 32 is taken too (below) */
} uavsal_pix_gemm_desc;

typedef struct uavsal_dec_sums_desc {
    const float* gy;  int64_t gy_img_pitch, gy_row_pitch, gy_col_pitch;
    const float* y;
    const float* e;  const float* d;  const float* ga;
    const float* w3;  const float* s3;      /* s3: one float */
    double* ws;  int64_t ws_bytes;
    int32_t n_img, H, W, C;
} uavsal_dec_sums_desc;

typedef struct uavsal_dec_finish_desc {
    const double* ws;  int64_t ws_bytes;  const double* rowdot;
    const float* wd;  const float* w3;  const float* s2;  const float* s3;
    const float* r1;  const float* mu1;  const float* r2;  const float* mu2;  const float* r3;  const float* mu3;
    float* g_gamma1;  float* g_beta1;  float* g_wd;  float* g_gamma2;  float* g_beta2;
    float* g_w3;  float* g_gamma3;  float* g_beta3;
    int32_t C, slabs, accumulate;
} uavsal_dec_finish_desc;

int64_t uavsal_pix_gemm_workspace_bytes(const uavsal_pix_gemm_desc* d);
int uavsal_pix_gemm_shares(const uavsal_pix_gemm_desc* d);      /* K shares per tile of that call (no launch) */
int uavsal_pix_gemm(const uavsal_pix_gemm_desc* d, uavsal_stream_t stream);
int64_t uavsal_dec_sums_workspace_bytes(const uavsal_dec_sums_desc* d);
int uavsal_dec_sums_slabs(const uavsal_dec_sums_desc* d);       /* slabs of that call (no launch) */
int uavsal_dec_sums_slab_rows(const uavsal_dec_sums_desc* d);   /* picture rows per slab */
int uavsal_dec_sums(const uavsal_dec_sums_desc* d, uavsal_stream_t stream);
int uavsal_dec_finish(const uavsal_dec_finish_desc* d, uavsal_stream_t stream);
int uavsal_train_decoder_sizeof_desc(int which);  /* 0 pix_gemm, 1 dec_sums, 2 dec_finish (uavsal_train_sizeof_desc is closed at 3) */

/* ---- fine-tuning a general inverted-residual block: its backward (csrc/train_block.hip) --------------------------------
 * A dwBlock with an expand conv, stride 1, dilation 1, in eval mode (r, s, b per BatchNorm as above); x is [P][Cin] with
 * P = n_img * H * W pixels, Ch hidden and Co output channels:
 *     u1 = W1 x, a1 = s1 u1 + b1, e = ReLU6(a1);  u2 = dw3x3(Wd, e), a2 = s2 u2 + b2, d = ReLU6(a2);
 *     o = s3 (W3 d) + b3  (+ x when the block has the residual).
 * With go = d loss / d o:
 *     gd[p][c]     = sum_m go[p][m] s3[m] W3[m][c]
 *     delta2[p][c] = gd[p][c] 1[0 < d[p][c] < 6]
 *     ga[p][c]     = 1[0 < e[p][c] < 6] s2[c] sum over taps k of wd[k][c] delta2[p - (k - (1,1))][c]
 *                    (zero outside the picture, never across frames)
 *     gx[p][j]     = sum_c ga[p][c] s1[c] W1[c][j]  (+ go[p][j] with the residual)
 * and the sums over all pixels
 *     S3[m] = sum go[p][m],  G3[m][c] = sum go[p][m] d[p][c],  S2[c] = sum delta2[p][c],  S1[c] = sum ga[p][c],
 *     Gd[c][ky][kx] = sum delta2[p][c] e[p + (ky-1, kx-1)][c],  G1[c][j] = sum ga[p][c] x[p][j]
 * the gradients are
 *     W1[c][j]: s1[c] G1[c][j]    beta1: S1    gamma1[c]: r1[c] (sum_j W1[c][j] G1[c][j] - mu1[c] S1[c])
 *     Wd[c][k]: s2[c] Gd[c][k]    beta2: S2    gamma2[c]: r2[c] (sum_k Wd[c][k] Gd[c][k] - mu2[c] S2[c])
 *     W3[m][c]: s3[m] G3[m][c]    beta3: S3    gamma3[m]: r3[m] (sum_c W3[m][c] G3[m][c] - mu3[m] S3[m])
 * from the UNSCALED sums, as for the decoder.  gd and gx are 1x1 convs (uavsal_conv_gemm with the transposed weights that
 * carry s3 / s1 in their rows); G1 and G3 with their row dots are two uavsal_pix_gemm calls (a = ga, b = x, w = W1 and
 * a = go, b = d, w = W3); the rest is here.  The masks are torch's: strict inequalities on the stored e and d.
 *
 * uavsal_ir_bwd: ga from gd, d, e dense [n_img][H][W][C], wd9 tap-major [9][C] as in uavsal_dw_desc and s2 [C]; delta2 is
 *   not materialised.  C % 4 == 0 and 16-byte aligned pointers (else UAVSAL_EALIGN).  ONE launch, memory bound.
 * uavsal_ir_sums: per slab of picture rows the partial sums S2, Gd, S1 and S3 -> `ws` (doubles), from gd, d, e, ga dense
 *   [n_img][H][W][Ch] and go, rows of Co floats ldgo floats apart.  Ch % 64 == 0 (else UAVSAL_ESHAPE), Co and ldgo
 *   multiples of 4.  delta2 is formed in fp32 exactly as uavsal_ir_bwd forms it; every product is accumulated in double.
 *   ws layout: per slab UAVSAL_IR_NSUM * Ch + Co doubles: [0] S2, [1 + ky * 3 + kx] Gd, [10] S1, each [Ch], then S3 [Co].
 *   The slabs follow the rule of uavsal_dec_sums and depend on the shape alone (uavsal_ir_sums_slabs / _slab_rows): no
 *   atomics, bit-reproducible.  ONE launch.
 * uavsal_ir_finish: sums the slabs in slab order in double and writes gamma1, beta1 [Ch], Wd [Ch][3][3], gamma2, beta2
 *   [Ch], gamma3, beta3 [Co] in the parameters' own layouts, each rounded once, overwritten or (`accumulate`) added to.
 *   rowdot1 [Ch]: uavsal_pix_gemm's with w = W1; rowdot3 [Co]: with w = W3.  wd is the parameter [Ch][3][3].  ONE launch.
 * ch16 != 0 (uavsal_ir_sums_desc and uavsal_ir_sums_s2_desc; opt-in, the field lies in what was the structs' tail padding, so a
 *   zeroed descriptor keeps every rule above, the refusal included): any Ch % 16 == 0 is taken -- the hidden widths 96 and 144
 *   of MobileNetV2 features[2:5].  The same kernels, slabs, workspace layout and summation order: a lane owns four channels,
 *   so the lanes behind Ch / 4 of the last channel group idle (at Ch = 96, 24 of 64 work); a Ch the default rule takes
 *   keeps its launch and bits with the flag set.  uavsal_ir_finish_c16 is uavsal_ir_finish for such a workspace: Ch % 16 == 0
 *   where uavsal_ir_finish wants Ch % 64 == 0, every other rule, the kernel and the order of the sums the same.
 * block_param_grads is SIX launches (two GEMMs with their reductions, sums, finish); block_backward adds the recomputation
 * of e and d (two), gd, uavsal_ir_bwd and, when wanted, gx.
 */
#define UAVSAL_IR_NSUM 11

typedef struct uavsal_ir_bwd_desc {
    const float* gd;  const float* d;  const float* e;
    const float* wd9;  const float* s2;
    float* ga;
    int32_t n_img, H, W, C;
} uavsal_ir_bwd_desc;

typedef struct uavsal_ir_sums_desc {
    const float* gd;  const float* d;  const float* e;  const float* ga;
    const float* go;  int32_t ldgo;         /* [n_img * H * W] rows of Co floats */
    double* ws;  int64_t ws_bytes;
    int32_t n_img, H, W, Ch, Co;
    int32_t ch16;                           /* 0: Ch % 64 == 0.  1: any Ch % 16 == 0 is taken (below); in what was tail padding */
} uavsal_ir_sums_desc;

typedef struct uavsal_ir_finish_desc {
    const double* ws;  int64_t ws_bytes;  const double* rowdot1;  const double* rowdot3;
    const float* wd;  const float* s2;
    const float* r1;  const float* mu1;  const float* r2;  const float* mu2;  const float* r3;  const float* mu3;
    float* g_gamma1;  float* g_beta1;  float* g_wd;  float* g_gamma2;  float* g_beta2;  float* g_gamma3;  float* g_beta3;
    int32_t Ch, Co, slabs, accumulate;
} uavsal_ir_finish_desc;

int uavsal_ir_bwd(const uavsal_ir_bwd_desc* d, uavsal_stream_t stream);
int64_t uavsal_ir_sums_workspace_bytes(const uavsal_ir_sums_desc* d);
int uavsal_ir_sums_slabs(const uavsal_ir_sums_desc* d);         /* slabs of that call (no launch) */
int uavsal_ir_sums_slab_rows(const uavsal_ir_sums_desc* d);     /* picture rows per slab */
int uavsal_ir_sums(const uavsal_ir_sums_desc* d, uavsal_stream_t stream);
int uavsal_ir_finish(const uavsal_ir_finish_desc* d, uavsal_stream_t stream);
int uavsal_ir_finish_c16(const uavsal_ir_finish_desc* d, uavsal_stream_t stream);     /* Ch % 16 == 0 */
int uavsal_block_sizeof_desc(int which);  /* 0 ir_bwd, 1 ir_sums, 2 ir_finish (uavsal_train_decoder_sizeof_desc is closed at 3) */

/* ---- input gradients of the frozen context-prior path (csrc/train_ctx.hip) ----------------------------------------------
 * With any prior enabled the output f of fust_layer[0] reaches the fusion block's input fu320 twice (model.py:344-365):
 * directly (channels 0..255) and through the context prior
 *     c[b] = sum_t f[b T + t];  c1 = cxt_cb_prior[0](c) (stride 2);  c2 = cxt_cb_prior[1](c1) (stride 2);
 *     u[n] = bilinear_ac(c2[(n % src_mod) / src_div]);  fu320[:, 256:] = fucb_layer[0](cat[priors..., u]).
 * The three blocks are frozen; only their INPUT gradients are needed (train.block_input_grad: gd and gx as in the block
 * backward above, ga from uavsal_ir_bwd or, for stride 2, from uavsal_ir_bwd_s2).
 *
 * uavsal_ir_bwd_s2: uavsal_ir_bwd for a depthwise 3x3 with stride 2, padding 1, dilation 1.  gd, d dense [n_img][Ho][Wo][C]
 *   with Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1; e, ga dense [n_img][H][W][C]; wd9 tap-major [9][C], s2 [C].  With
 *   m6(v) = 1[0 < v < 6]:
 *     ga[y][x] = m6(e[y][x]) s2 sum over (ky, kx) with y + 1 - ky and x + 1 - kx even, oy = (y + 1 - ky) / 2 in [0, Ho),
 *                ox = (x + 1 - kx) / 2 in [0, Wo), of wd[ky][kx] m6(d[oy][ox]) gd[oy][ox]
 *   (the sum, then * s2, then the mask by e: the order of uavsal_ir_bwd).  C % 4 == 0 (else UAVSAL_ESHAPE), 16-byte
 *   aligned pointers.  ONE launch.
 * uavsal_bilinear_ac_bwd: the adjoint of uavsal_bilinear_ac with its frame map.  gout: [n_out][Ho][Wo] rows of C floats ldo
 *   floats apart (a channel slice is read in place); gin dense [n_src][Hi][Wi][C], every element written:
 *     gin[ns][sy][sx] = sum over n with (n % src_mod) / src_div == ns, over (oy, ox), of wy(oy, sy) wx(ox, sx) gout[n][oy][ox]
 *     wy(oy, sy) = hy 1[y0 == sy] + ly 1[y1 == sy]   with the forward's fp32 fy = sy_scale oy, y0 = (int)fy,
 *                  y1 = y0 + (y0 < Hi - 1), ly = fy - y0, hy = 1 - ly (both terms where the border makes y0 == y1)
 *   and wx likewise.  A gather: n, then oy, then ox in increasing order, accumulated in double and rounded once; no
 *   atomics, bit-reproducible, a function of the shape alone.  n_src must cover the largest source image of the map.
 * uavsal_tsum_bwd: out[b T + t] = a[b T + t] + g[b], the adjoint of uavsal_tsum added to a given gradient `a` (rows lda
 *   floats apart: a channel slice is read in place); g rows ldg, out rows ldo floats apart.  ONE launch.
 */
typedef struct uavsal_ir_bwd_s2_desc {
    const float* gd;  const float* d;       /* [n_img][Ho][Wo][C] */
    const float* e;                         /* [n_img][H][W][C] */
    const float* wd9;  const float* s2;
    float* ga;                              /* [n_img][H][W][C] */
    int32_t n_img, H, W, C;
} uavsal_ir_bwd_s2_desc;

typedef struct uavsal_bilinear_bwd_desc {
    const float* gout;  int32_t ldo;  int32_t Ho, Wo;
    float* gin;         int32_t Hi, Wi;
    int32_t n_out, n_src, C, src_mod, src_div;
} uavsal_bilinear_bwd_desc;

typedef struct uavsal_tsum_bwd_desc {
    const float* a;  int32_t lda;
    const float* g;  int32_t ldg;
    float* out;      int32_t ldo;
    int32_t n_groups, T, HW, C;
} uavsal_tsum_bwd_desc;

int uavsal_ir_bwd_s2(const uavsal_ir_bwd_s2_desc* d, uavsal_stream_t stream);
int uavsal_bilinear_ac_bwd(const uavsal_bilinear_bwd_desc* d, uavsal_stream_t stream);
int uavsal_tsum_bwd(const uavsal_tsum_bwd_desc* d, uavsal_stream_t stream);
int uavsal_ctx_sizeof_desc(int which);    /* 0 ir_bwd_s2, 1 bilinear_bwd, 2 tsum_bwd (uavsal_block_sizeof_desc is closed at 3) */

/* ---- fine-tuning the multi-prior path: the sums of a stride-2 block (csrc/train_ctx.hip) --------------------------------
 * The three blocks of the path above, TRAINED (train.prior_path_backward): their parameter gradients are those of the block
 * backward (uavsal_pix_gemm for G1 over the INPUT pixels and G3 over the OUTPUT pixels, uavsal_ir_finish); for the two
 * stride-2 blocks the channel sums come from
 *
 * uavsal_ir_sums_s2: uavsal_ir_sums for a depthwise 3x3 with stride 2, padding 1, dilation 1.  d, gd dense
 *   [n_img][Ho][Wo][Ch] with Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1; e, ga dense [n_img][H][W][Ch]; go rows of Co floats
 *   ldgo floats apart over the n_img Ho Wo output pixels.  With delta2 = gd m6(d) formed in fp32 as uavsal_ir_bwd_s2 forms it:
 *     S2[c]         = sum over OUTPUT pixels of delta2[n][oy][ox][c]
 *     Gd[c][ky][kx] = sum over OUTPUT pixels of delta2[n][oy][ox][c] e[n][2 oy - 1 + ky][2 ox - 1 + kx][c]  (zero outside)
 *     S3[m]         = sum over OUTPUT pixels of go[n][oy][ox][m]
 *     S1[c]         = sum over INPUT pixels of ga[n][y][x][c]
 *   every product accumulated in double.  The workspace layout is uavsal_ir_sums' ([slab][UAVSAL_IR_NSUM * Ch + Co] doubles),
 *   so uavsal_ir_finish is used unchanged.  A slab is a run of whole output rows counted through all images (about 256
 *   input pixels, at most 256 slabs) with the input rows 2 oy and 2 oy + 1 of each; it depends on the shape alone
 *   (uavsal_ir_sums_s2_slabs / _slab_rows): no atomics, bit-reproducible.  Ch % 64 == 0 (else UAVSAL_ESHAPE), Co and ldgo
 *   multiples of 4, 16-byte aligned pointers (else UAVSAL_EALIGN).  ONE launch.
 */
typedef struct uavsal_ir_sums_s2_desc {
    const float* gd;  const float* d;       /* [n_img][Ho][Wo][Ch] */
    const float* e;  const float* ga;       /* [n_img][H][W][Ch] */
    const float* go;  int32_t ldgo;         /* [n_img * Ho * Wo] rows of Co floats */
    double* ws;  int64_t ws_bytes;
    int32_t n_img, H, W, Ch, Co;
    int32_t ch16;                           /* as in uavsal_ir_sums_desc */
} uavsal_ir_sums_s2_desc;

int64_t uavsal_ir_sums_s2_workspace_bytes(const uavsal_ir_sums_s2_desc* d);
int uavsal_ir_sums_s2_slabs(const uavsal_ir_sums_s2_desc* d);       /* slabs of that call (no launch) */
int uavsal_ir_sums_s2_slab_rows(const uavsal_ir_sums_s2_desc* d);   /* OUTPUT rows per slab */
int uavsal_ir_sums_s2(const uavsal_ir_sums_s2_desc* d, uavsal_stream_t stream);
int uavsal_mp_sizeof_desc(int which);     /* 0 ir_sums_s2 (uavsal_ctx_sizeof_desc is closed at 3) */

/* ---- fine-tuning the gauss / ob prior nets: a narrow block's gradients, the sum over frames (csrc/train_nets.hip) --------
 * Block 0 of either prior net is 8 -> 48 -> 64 or 20 -> 120 -> 64 (stride 1, dilation 1, no residual): widths that
 * uavsal_pix_gemm, uavsal_ir_sums and uavsal_ir_finish refuse.  The formulas are those of the block backward above.
 *
 * uavsal_ir_narrow_grads: from x dense [n_img][H][W][Cin], e, d, gd, ga dense [n_img][H][W][Ch] and go, rows of Co floats ldgo
 *   floats apart (a channel slice is read in place), per slab of picture rows the partials of G1 = ga x x, G3 = go x d, S2,
 *   Gd[9], S1 and S3 -> `ws` (doubles).  ws layout per slab: UAVSAL_IR_NSUM * Ch sums as in uavsal_ir_sums, S3 [Co],
 *   G1 [Ch][Cin], G3 [Co][Ch].  delta2 = gd m6(d) is formed in fp32 as uavsal_ir_bwd forms it; the sums add every product in
 *   double; G1 and G3 add the products of UAVSAL_NARROW_CHUNK consecutive pixels of the slab in fp32 (fused multiply-add, in
 *   pixel order) and the chunks in double.  A slab is a run of whole picture rows counted through all images, about 256 pixels
 *   and at most 256 slabs (the rule of uavsal_ir_sums at half its slab size; uavsal_ir_narrow_slabs / _slab_rows): a function of
 *   the shape alone, no atomics, bit-reproducible.  Accepted: Cin % 4 == 0, Cin <= 32, Ch % 4 == 0,
 *   Ch <= 128, Co == 64 (else UAVSAL_ESHAPE); ldgo % 4 == 0 and 16-byte aligned pointers (else UAVSAL_EALIGN).  Nothing at
 *   or behind Cin, Ch or Co is read.  ONE launch.
 * uavsal_ir_narrow_finish: sums the slabs in slab order in double and writes the nine gradients in the parameters' own
 *   layouts (w1 [Ch][Cin], wd [Ch][3][3], w3 [Co][Ch]): W = s G, beta = S, gamma = r (sum W G - mu S) with the row dots taken
 *   in index order in double from the unscaled sums, each result rounded once, overwritten or (`accumulate`) added to.
 *   s1, s2, s3 the folded scales, r, mu as above.  ONE launch.
 * uavsal_frame_sum: out[p][c] = sum over n of a[n][p][c] for HW pixels and C channels; a: N images of HW rows lda floats
 *   apart (a channel slice is read in place), out rows ldo floats apart.  Frames are added in frame order in double and the
 *   sum is rounded once; N == 1 returns the input's bits.  C, lda, ldo multiples of 4, 16-byte aligned pointers.  ONE launch.
 */
#define UAVSAL_NARROW_CHUNK 32

typedef struct uavsal_ir_narrow_desc {
    const float* x;                         /* [n_img][H][W][Cin] */
    const float* e;  const float* d;  const float* gd;  const float* ga;      /* [n_img][H][W][Ch] */
    const float* go;  int32_t ldgo;         /* [n_img * H * W] rows of Co floats */
    double* ws;  int64_t ws_bytes;
    int32_t n_img, H, W, Cin, Ch, Co;
} uavsal_ir_narrow_desc;

typedef struct uavsal_ir_narrow_finish_desc {
    const double* ws;  int64_t ws_bytes;
    const float* w1;  const float* wd;  const float* w3;
    const float* s1;  const float* s2;  const float* s3;
    const float* r1;  const float* mu1;  const float* r2;  const float* mu2;  const float* r3;  const float* mu3;
    float* g_w1;  float* g_gamma1;  float* g_beta1;  float* g_wd;  float* g_gamma2;  float* g_beta2;
    float* g_w3;  float* g_gamma3;  float* g_beta3;
    int32_t Cin, Ch, Co, slabs, accumulate;
} uavsal_ir_narrow_finish_desc;

typedef struct uavsal_frame_sum_desc {
    const float* a;  int32_t lda;
    float* out;      int32_t ldo;
    int32_t N, HW, C;
} uavsal_frame_sum_desc;

int64_t uavsal_ir_narrow_workspace_bytes(const uavsal_ir_narrow_desc* d);
int uavsal_ir_narrow_slabs(const uavsal_ir_narrow_desc* d);         /* slabs of that call (no launch) */
int uavsal_ir_narrow_slab_rows(const uavsal_ir_narrow_desc* d);     /* picture rows per slab */
int uavsal_ir_narrow_grads(const uavsal_ir_narrow_desc* d, uavsal_stream_t stream);
int uavsal_ir_narrow_finish(const uavsal_ir_narrow_finish_desc* d, uavsal_stream_t stream);
int uavsal_frame_sum(const uavsal_frame_sum_desc* d, uavsal_stream_t stream);
int uavsal_nets_sizeof_desc(int which);   /* 0 ir_narrow, 1 ir_narrow_finish, 2 frame_sum (uavsal_mp_sizeof_desc is closed at 1) */

/* ---- fine-tuning the ST blocks: conv + BN + ReLU6 sums, the adjoint of the temporal difference (csrc/train_st.hip) --------
 * An ST block (model.py:163-249) with x [N][256]:  x_sp = spconv(x);  r = ReLU6(BN(W_r x)) (256 -> 32);  dif = tdiff(r);
 * t1 = sub_conv(dif) (64 -> 384 -> 32);  a_te = ReLU6(BN(W_l t1)) (32 -> 256);  o = ReLU6(BN(W_last (x_sp + a_te)));
 * out = x + o.  The two inverted-residual blocks go through the block backward above (uavsal_pix_gemm takes their 32-wide
 * sides); the three 1x1 conv + BatchNorm + ReLU6 stages y = ReLU6(s (W x) + b), in eval mode, with m6(v) = 1[0 < v < 6],
 *     gp[p][c] = g[p][c] m6(y[p][c])     S[c] = sum_p gp[p][c]     G[c][j] = sum_p gp[p][c] x[p][j]
 * have the gradients
 *     W[c][j]: s[c] G[c][j]    beta: S    gamma[c]: r[c] (sum_j W[c][j] G[c][j] - mu[c] S[c])    x: gp . (diag(s) W)
 * (G, the row scale and the row dot from uavsal_pix_gemm(gp, x); the gamma gradient from the UNSCALED sums).
 *
 * uavsal_cbr_sums: g rows of C floats ldg floats apart (a channel slice is read in place) = d loss / d output; y rows ldy
 *   floats apart = the stage's own activation (before any residual is added); writes gp dense [n_img H W][C] and per slab
 *   of picture rows the partial sums S -> `ws` ([slab][C] doubles), every term added in double.  A slab is a run of whole
 *   picture rows counted through all images, about 512 pixels and at most 256 slabs (the rule of uavsal_ir_sums;
 *   uavsal_cbr_sums_slabs / _slab_rows): a function of the shape alone, no atomics, bit-reproducible.  C % 32 == 0 (else
 *   UAVSAL_ESHAPE); ldg, ldy multiples of 4 and 16-byte aligned pointers (else UAVSAL_EALIGN).  ONE launch.
 * uavsal_cbr_finish: sums the slabs in slab order in double and writes beta: S and gamma[c]: r[c] (rowdot[c] - mu[c] S[c]),
 *   each rounded once, overwritten or (`accumulate`) added to.  rowdot: uavsal_pix_gemm's, with w = W.  ONE launch.
 * uavsal_tdiff_bwd: the adjoint of uavsal_tdiff fused with the ReLU6 mask of the stage that made its input.  g rows of 2 C
 *   floats ldg floats apart = d loss / d dif, P_i = g[i][:C], Q_i = g[i][C:]; r rows ldr floats apart = uavsal_tdiff's input;
 *   out rows ldo floats apart.  For frame j of a sequence of L = seq_len frames (n_img % L == 0, L >= 2; nothing crosses a
 *   sequence border), the at most six terms in this order, added in double and rounded once:
 *     own frame:   j == 0: -P_0 + Q_0;   j == L-1: +P_j - Q_j;   else +P_j + Q_j
 *     frame j - 1: j - 1 == 0: +P_0 - Q_0;   0 < j - 1: -Q_{j-1}                (j >= 1)
 *     frame j + 1: j + 1 == L-1: -P_{j+1} + Q_{j+1};   j + 1 < L-1: -P_{j+1}    (j <= L-2)
 *   (frame 0 takes the first rule and frame L-1 the last, L == 2 included), then out[j] = m6(r[j]) * that sum.  A gather:
 *   bit-reproducible.  C, ldg, ldr, ldo multiples of 4, 16-byte aligned pointers (else UAVSAL_EALIGN); seq_len < 2 or
 *   n_img % seq_len != 0: UAVSAL_ESHAPE.  ONE launch.
 */
typedef struct uavsal_cbr_sums_desc {
    const float* g;  int32_t ldg;           /* [n_img * H * W] rows of C floats */
    const float* y;  int32_t ldy;           /* [n_img * H * W] rows of C floats */
    float* gp;                              /* dense [n_img][H][W][C] */
    double* ws;  int64_t ws_bytes;
    int32_t n_img, H, W, C;
} uavsal_cbr_sums_desc;

typedef struct uavsal_cbr_finish_desc {
    const double* ws;  int64_t ws_bytes;
    const double* rowdot;                   /* [C] */
    const float* r;  const float* mu;       /* [C] */
    float* g_gamma;  float* g_beta;         /* [C] */
    int32_t C, slabs, accumulate;
} uavsal_cbr_finish_desc;

typedef struct uavsal_tdiff_bwd_desc {
    const float* g;  int32_t ldg;           /* [n_img * HW] rows of 2 C floats */
    const float* r;  int32_t ldr;           /* [n_img * HW] rows of C floats */
    float* out;      int32_t ldo;           /* [n_img * HW] rows of C floats */
    int32_t n_img, HW, C, seq_len;
} uavsal_tdiff_bwd_desc;

int64_t uavsal_cbr_sums_workspace_bytes(const uavsal_cbr_sums_desc* d);
int uavsal_cbr_sums_slabs(const uavsal_cbr_sums_desc* d);           /* slabs of that call (no launch) */
int uavsal_cbr_sums_slab_rows(const uavsal_cbr_sums_desc* d);       /* picture rows per slab */
int uavsal_cbr_sums(const uavsal_cbr_sums_desc* d, uavsal_stream_t stream);
int uavsal_cbr_finish(const uavsal_cbr_finish_desc* d, uavsal_stream_t stream);
int uavsal_tdiff_bwd(const uavsal_tdiff_bwd_desc* d, uavsal_stream_t stream);
int uavsal_st_sizeof_desc(int which);     /* 0 cbr_sums, 1 cbr_finish, 2 tdiff_bwd (uavsal_nets_sizeof_desc is closed at 3) */

/* ---- fine-tuning the SRF-Net head: a dense 3x3 weight gradient, the dilated depthwise backward (csrc/train_srf.hip) --------
 * The head of model.sfnet (model.py:120-158) behind the frozen MobileNetV2 features: three 1x1 conv + BatchNorm + ReLU6
 * stages on c3 / c4 / c5 and one on the 1024-wide ASPP concat (uavsal_cbr_sums, uavsal_pix_gemm, uavsal_cbr_finish above;
 * uavsal_pix_gemm takes their 64 x 32 and 128 x 96), three dilated inverted-residual blocks 320 -> 1920 -> 256 (dilation 6,
 * 12, 18; the block backward above with the two kernels below in place of uavsal_ir_bwd / uavsal_ir_sums) and the dense 3x3
 * conv_last 448 -> 256 + BatchNorm + ReLU6, whose stage is the cbr stage above with G[co][ci][ky][kx] in place of G[c][j].
 *
 * uavsal_conv3_wgrad: out[co][ci][ky][kx] = fl(row_scale[co] G[co][ci][ky][kx]) (+ the old value with `accumulate`),
 *   G[co][ci][ky][kx] = sum over images and pixels p of g[p][co] x[p + (ky-1, kx-1)][ci], zero outside the picture, never
 *   across frames.  g dense [n_img][H][W][Co]; x rows of Ci floats ldx floats apart (a channel slice is read in place); out
 *   the parameter's own [Co][Ci][3][3].  row_scale NULL = 1.  rowdot (optional, [Co] doubles) = sum over ci, ky, kx of
 *   w[co][ci][ky][kx] G[co][ci][ky][kx] (w dense like out) in double in a fixed order: uavsal_pix_gemm's contract, so
 *   uavsal_cbr_finish forms the gamma gradient.  The tile loop, chunks, chains and K split of uavsal_twa_wgrad: 128 x 128
 *   tiles of ONE tap, (Co / 128) * 9 * ceil(Ci / 128) of them, shares of whole chunks of UAVSAL_WGRAD_CHAIN pixels, partial
 *   tiles [share][co][tap][ci] in `ws`; a second launch (a workgroup per co) sums the shares in share order in double and
 *   rounds once.  Co % 128 == 0 and Ci % 64 == 0 (else UAVSAL_ESHAPE; the last tile of a tap may be half empty: nothing at
 *   or behind column Ci is read, written or enters rowdot); g, x, ws 16-byte aligned, ldx a multiple of 4 (else
 *   UAVSAL_EALIGN).  No atomics: two calls return the same bits.  TWO launches, no allocation.
 * uavsal_ir_bwd_dil / uavsal_ir_sums_dil: uavsal_ir_bwd / uavsal_ir_sums for a depthwise 3x3 with stride 1, padding dil and
 *   dilation dil >= 1 (else UAVSAL_EINVAL): the taps lie at p -/+ dil (k - (1,1)),
 *     ga[p][c]      = 1[0 < e[p][c] < 6] s2[c] sum over taps k of wd[k][c] delta2[p - dil (k - (1,1))][c]
 *     Gd[c][ky][kx] = sum delta2[p][c] e[p + dil (ky-1, kx-1)][c]
 *   with delta2 = gd 1[0 < d < 6] formed in fp32 as uavsal_ir_bwd forms it, the sum over the taps in the order k = 8 .. 0 of
 *   wd, then * s2, then the mask by e.  A lane owns four channels of ONE pixel and nine bounds-checked taps (the 2 x 2
 *   patch with a 4 x 4 halo of the undilated kernels gives nothing at a dilation of 6 to 18 on a 1/32-scale map).  The sums'
 *   slabs, workspace layout and byte count are those of uavsal_ir_sums for the same shape (uavsal_ir_sums_dil_slabs /
 *   _slab_rows / _workspace_bytes), so uavsal_ir_finish takes the workspace as it is.  C % 4 == 0 (uavsal_ir_bwd_dil, else
 *   UAVSAL_EALIGN), Ch % 64 == 0 (uavsal_ir_sums_dil, else UAVSAL_ESHAPE).  ONE launch each, no atomics, bit-reproducible.
 */
typedef struct uavsal_conv3_wgrad_desc {
    const float* g;                         /* dense [n_img][H][W][Co] */
    const float* x;      int32_t ldx;       /* [n_img * H * W] rows of Ci floats */
    const float* row_scale;                 /* [Co] or NULL */
    const float* w;                         /* dense [Co][Ci][3][3] (needed with rowdot) */
    double* rowdot;                         /* [Co] or NULL */
    float* ws;  int64_t ws_bytes;
    float* out;                             /* [Co][Ci][3][3] */
    int32_t n_img, H, W, Co, Ci, accumulate;
} uavsal_conv3_wgrad_desc;

typedef struct uavsal_ir_bwd_dil_desc {
    const float* gd;  const float* d;  const float* e;
    const float* wd9;  const float* s2;
    float* ga;
    int32_t n_img, H, W, C, dil;
} uavsal_ir_bwd_dil_desc;

typedef struct uavsal_ir_sums_dil_desc {
    const float* gd;  const float* d;  const float* e;  const float* ga;
    const float* go;  int32_t ldgo;         /* [n_img * H * W] rows of Co floats */
    double* ws;  int64_t ws_bytes;
    int32_t n_img, H, W, Ch, Co, dil;
} uavsal_ir_sums_dil_desc;

int64_t uavsal_conv3_wgrad_workspace_bytes(const uavsal_conv3_wgrad_desc* d);
int uavsal_conv3_wgrad_shares(const uavsal_conv3_wgrad_desc* d);    /* K shares per tile of that call (no launch) */
int uavsal_conv3_wgrad(const uavsal_conv3_wgrad_desc* d, uavsal_stream_t stream);
int uavsal_ir_bwd_dil(const uavsal_ir_bwd_dil_desc* d, uavsal_stream_t stream);
int64_t uavsal_ir_sums_dil_workspace_bytes(const uavsal_ir_sums_dil_desc* d);
int uavsal_ir_sums_dil_slabs(const uavsal_ir_sums_dil_desc* d);     /* slabs of that call (no launch) */
int uavsal_ir_sums_dil_slab_rows(const uavsal_ir_sums_dil_desc* d); /* picture rows per slab */
int uavsal_ir_sums_dil(const uavsal_ir_sums_dil_desc* d, uavsal_stream_t stream);
int uavsal_srf_sizeof_desc(int which);    /* 0 conv3_wgrad, 1 ir_bwd_dil, 2 ir_sums_dil (uavsal_st_sizeof_desc is closed at 3) */

/* ---- fine-tuning the shallow backbone: the skinny weight-gradient GEMM (csrc/train_shallow.hip) ---------------------------
 * The 1x1 weight gradients of MobileNetV2 features[2:8] that uavsal_pix_gemm refuses: 96 x 16, 144 x 24, 24 x 96, 24 x 144 and
 * 32 x 144 over 72,000 to 1,152,000 pixels at 20 frames of 360 x 640.  Under 30 flop per operand byte: the memory sets the
 * time, so the kernel makes ONE pass over both operands and multiplies no padded 128 x 128 tile.
 *
 * uavsal_skinny_wgrad: uavsal_pix_gemm's contract -- out[m][n] = fl(row_scale[m] G[m][n]) (+ the old value with
 *   `accumulate`), G[m][n] = sum over the K pixels p of a[p][m] b[p][n]; row p of a / b at p * lda / p * ldb floats (channel
 *   slices are read in place); row_scale NULL = 1; rowdot (optional, [M] doubles) = sum_n w[m][n] G[m][n] in double in a fixed
 *   order, w rows ldw floats apart -- for M and N multiples of 8 with min(M, N) <= 32 and max(M, N) <= 192 (else
 *   UAVSAL_ESHAPE).  Nothing at or behind column M of a, column N of b, row M or column N of out / w is read or written.
 *   The partition: the K pixels are cut into UNITS of UAVSAL_SKINNY_UNIT = 128; units = ceil(K / 128),
 *   want = min(UAVSAL_SKINNY_SHARES, units), ups = ceil(units / want), shares = ceil(units / ups) (uavsal_skinny_wgrad_shares
 *   returns it: a function of K alone, at most UAVSAL_SKINNY_SHARES = 1024, one wave per SIMD of 256 CUs).  Share s owns the
 *   pixels [s ups 128, (s + 1) ups 128) cut at K and is the work of ONE wave, which holds the whole M x N result: the narrow
 *   side in one 32-wide MFMA tile (its columns from min(M, N) on are zeros in registers, never read), the wide side in
 *   ceil(max(M, N) / 32) tiles, the last cut at its width in the same way.  The wave reads its pixels two at a time in the
 *   layout of v_mfma_f32_32x32x2_f32 (128 contiguous bytes per tile and pixel; every operand byte is fetched once) and adds
 *   pixel pair after pixel pair, in pixel order, to one fp32 accumulator per tile; an accumulation chain ends every
 *   UAVSAL_WGRAD_CHAIN products counted from the share's first pixel and is added in fp32 to the share's total.  The totals
 *   go to `ws` as [share][M][N] floats (uavsal_skinny_wgrad_workspace_bytes: shares * M * N * 4).  A second launch, one
 *   workgroup per row m, sums them in double in a FIXED order that depends on the shape alone: with g = floor(1024 / N)
 *   groups and spg = ceil(shares / g), group j adds the shares [j spg, (j + 1) spg) cut at `shares` in share order, then the
 *   groups are added in group order; the sum is scaled, rounded once and stored; rowdot's N products meet in a fixed tree.
 *   No atomics: two calls return the same bits.  TWO launches, no allocation.  UAVSAL_EALIGN: a, b, ws not 16-byte aligned
 *   or lda / ldb not a multiple of 4; UAVSAL_EINVAL: a null operand, ws_bytes too small, a pitch below its width, rowdot
 *   without w. */
#define UAVSAL_SKINNY_UNIT 128
#define UAVSAL_SKINNY_SHARES 1024
#define UAVSAL_SKINNY_MAX_NARROW 32
#define UAVSAL_SKINNY_MAX_WIDE 192

typedef struct uavsal_skinny_wgrad_desc {
    const float* a;  int32_t lda;           /* [K] rows of M floats */
    const float* b;  int32_t ldb;           /* [K] rows of N floats */
    const float* row_scale;                 /* [M] or NULL */
    const float* w;  int32_t ldw;           /* [M] rows of N floats (needed with rowdot) */
    double* rowdot;                         /* [M] or NULL */
    float* ws;  int64_t ws_bytes;
    float* out;  int32_t ldo;               /* [M] rows of N floats */
    int64_t K;  int32_t M, N, accumulate;
} uavsal_skinny_wgrad_desc;

int64_t uavsal_skinny_wgrad_workspace_bytes(const uavsal_skinny_wgrad_desc* d);
int uavsal_skinny_wgrad_shares(const uavsal_skinny_wgrad_desc* d);  /* K shares of that call (no launch); 0: refused */
int uavsal_skinny_wgrad(const uavsal_skinny_wgrad_desc* d, uavsal_stream_t stream);
int uavsal_shallow_sizeof_desc(int which);    /* 0 skinny_wgrad (uavsal_srf_sizeof_desc is closed at 3) */

/* ---- BatchNorm on BATCH statistics (training mode) and the decoder built on it (csrc/train_bn.hip) -----------------------
 * torch's rules for nn.BatchNorm2d in training mode.  For one BatchNorm over u [P][C], P = n_img * H * W pixels of ALL frames
 * of the call together, rows `ld` floats apart (a channel slice is read in place), C % 4 == 0 or C == 1 (else UAVSAL_ESHAPE):
 *     mu = mean_p u,  var = mean_p (u - mu)^2 (biased),  r = 1 / sqrt(var + eps),  xh = (u - mu) r,  a = gamma xh + beta
 * and with g = d loss / d act(a), g_a = g act'(a):
 *     d beta = sum_p g_a,  d gamma = sum_p g_a xh,  d loss / d u = gamma r (g_a - d beta / P - xh d gamma / P).
 * The running statistics move as running_mean <- (1 - m) running_mean + m mu, running_var <- (1 - m) running_var +
 * m var P / (P - 1).  The kernels work from the FOLD s = gamma r, b = beta - mu s: a = fma(u, s, b) in fp32 -- every kernel
 * below forms a by that one fused multiply-add, so a mask or a sigmoid recomputed in the backward is the forward's -- and
 * xh = fl(fl(u - mu) r) from the fp32 mu, r.  Nothing divides by gamma: a channel with gamma = 0 has g_u = 0 and a non-zero
 * d gamma.
 *
 * The reductions share one geometry.  A lane owns 4 consecutive channels of a pixel (16-byte accesses; C == 1: one), lc lanes
 * side by side (the smallest power of two >= C / 4, at most 64), the 256 / lc pixel lanes of a workgroup take the pixels of a
 * SLAB in turn (pixel lane i: the slab's pixels i, i + 256 / lc, ...).  Slabs are whole picture rows counted through all
 * frames: rows per slab = max(ceil(512 / W), ceil(n_img H / 256)) (uavsal_bn_slab_rows), slabs = ceil(n_img H / rows per slab)
 * (uavsal_bn_slabs): a function of the shape alone.  Order of every sum: a thread adds its pixels in pixel order in double;
 * the pixel lanes of a channel are added in pixel-lane order in double; the finish launch adds the slabs in slab order in
 * double and rounds once.  No atomics, no host round trip, no synchronisation: two calls return the same bits.
 *
 * uavsal_bn_stats: sum u and sum u^2 (the products exact in double) -> mu = S1 / P, var = max(S2 / P - mu^2, 0) in double;
 *   writes mu, var, r, s, b [C] fp32, each rounded once from double, and -- running_mean / running_var not NULL -- blends the
 *   running statistics in place in double, rounded once (P >= 2 then, else UAVSAL_ESHAPE).  ws: uavsal_bn_stats_workspace_bytes
 *   = slabs * 2 * C doubles, [slab][2][C].  TWO launches.
 * uavsal_bn_apply: out[p][c] = act(fma(u, s, b)), dense [n_pix][C]; act none / ReLU6 / sigmoid (apply_act: 1 / (1 + expf(-a))).
 *   dot_w != NULL (C % 4 == 0): out[p] = sum_c dot_w[c] act(...)[p][c] instead, dense [n_pix] (the decoder's projection to one
 *   channel; the activated tensor is not stored): a wave per pixel, lane l adds its channels 4 l + 256 j, j = 0, 1, ... (the
 *   four of a load in channel order) to one fp32 accumulator by fused multiply-adds, the 64 lanes meet in a butterfly
 *   (xor 32, 16, ..., 1).  ONE launch.
 * uavsal_bn_bwd_sums: g [P][C] rows ldg apart, or (g == NULL) the rank-one g[p][c] = fl(g_pix[p] g_chan[c]) -- the adjoint of a
 *   projection to one channel, formed in the launch instead of being stored.  g_a = g 1[0 < a < 6] (ReLU6), g fl(y fl(1 - y)),
 *   y = act(a) (sigmoid), g (none).  Accumulates g_a and g_a xh (and, rank-one, g_pix act(a): the projection's weight
 *   gradient); the finish writes `sums` [2][C] doubles = d beta, d gamma (kept for uavsal_bn_bwd_apply) and, each where the
 *   pointer is not NULL, g_beta, g_gamma, g_w [C], rounded once, overwritten or (`accumulate`) added to.
 *   ws: uavsal_bn_bwd_workspace_bytes = slabs * 3 * C doubles, [slab][2 or 3][C].  TWO launches.
 * uavsal_bn_bwd_apply: gu[p][c] = fl(s fma(-xh, c2, fl(g_a - c1))), c1 = fl(sums[c] / P), c2 = fl(sums[C + c] / P), g_a and
 *   xh formed as in uavsal_bn_bwd_sums; dense [P][C].  The same descriptor.  ONE launch.
 * uavsal_dw_wgrad: out[c][ky][kx] = sum_p g[p][c] e[p + (ky-1, kx-1)][c], zero outside the picture, never across frames (the
 *   halo is masked by the row inside ITS frame), C % 4 == 0; nine sums per channel in double per slab, the geometry and order
 *   above; out [C][3][3] rounded once, overwritten or (`accumulate`) added to.  ws: slabs * 9 * C doubles.  TWO launches.
 * The raw depthwise conv of the decoder and its transpose are uavsal_dw3x3 with unit scale, zero bias and no activation, the
 * transpose with the taps flipped.
 * UAVSAL_EALIGN: a 4-wide tensor or its pitch not 16-byte aligned, a workspace not 8-byte aligned; UAVSAL_EINVAL: a missing
 * pointer, a size <= 0, a pitch below C, a workspace too small, eps < 0 or momentum outside [0, 1].
 */
typedef struct uavsal_bn_stats_desc {
    const float* u;  int32_t ld;
    const float* gamma;  const float* beta;         /* [C] */
    float* running_mean;  float* running_var;       /* [C], updated in place; NULL: left alone */
    double eps, momentum;
    double* ws;  int64_t ws_bytes;
    float* mu;  float* var;  float* r;  float* s;  float* b;     /* [C] each */
    int32_t n_img, H, W, C;
} uavsal_bn_stats_desc;

typedef struct uavsal_bn_apply_desc {
    const float* u;  int32_t ld;
    const float* s;  const float* b;                /* [C] */
    const float* dot_w;                             /* NULL, or [C]: the dot over the channels */
    float* out;                                     /* dense [n_pix][C], or [n_pix] with dot_w */
    int64_t n_pix;  int32_t C, act;
} uavsal_bn_apply_desc;

typedef struct uavsal_bn_bwd_desc {
    const float* g;  int32_t ldg;                   /* [P] rows of C floats, or NULL: */
    const float* g_pix;  const float* g_chan;       /* [P], [C]: g[p][c] = g_pix[p] g_chan[c] */
    const float* u;  int32_t ld;
    const float* s;  const float* b;  const float* mu;  const float* r;     /* uavsal_bn_stats's */
    double* ws;  int64_t ws_bytes;                  /* bwd_sums only */
    double* sums;                                   /* [2][C]: bwd_sums writes, bwd_apply reads */
    float* g_gamma;  float* g_beta;  float* g_w;    /* [C] each or NULL (bwd_sums) */
    float* gu;                                      /* dense [P][C] (bwd_apply) */
    int32_t n_img, H, W, C, act, accumulate;
} uavsal_bn_bwd_desc;

typedef struct uavsal_dw_wgrad_desc {
    const float* g;  int32_t ldg;
    const float* e;  int32_t lde;
    double* ws;  int64_t ws_bytes;
    float* out;                                     /* [C][3][3] */
    int32_t n_img, H, W, C, accumulate;
} uavsal_dw_wgrad_desc;

int uavsal_bn_slabs(int n_img, int H, int W);       /* slabs of every reduction above for that shape (no launch); 0: refused */
int uavsal_bn_slab_rows(int n_img, int H, int W);   /* picture rows per slab */
int64_t uavsal_bn_stats_workspace_bytes(const uavsal_bn_stats_desc* d);
int uavsal_bn_stats(const uavsal_bn_stats_desc* d, uavsal_stream_t stream);
int uavsal_bn_apply(const uavsal_bn_apply_desc* d, uavsal_stream_t stream);
int64_t uavsal_bn_bwd_workspace_bytes(const uavsal_bn_bwd_desc* d);
int uavsal_bn_bwd_sums(const uavsal_bn_bwd_desc* d, uavsal_stream_t stream);
int uavsal_bn_bwd_apply(const uavsal_bn_bwd_desc* d, uavsal_stream_t stream);
int64_t uavsal_dw_wgrad_workspace_bytes(const uavsal_dw_wgrad_desc* d);
int uavsal_dw_wgrad(const uavsal_dw_wgrad_desc* d, uavsal_stream_t stream);
int uavsal_bn_sizeof_desc(int which);         /* 0 bn_stats, 1 bn_apply, 2 bn_bwd, 3 dw_wgrad (additions: UAVSAL_ABI_VERSION stays 20) */

/* uavsal_bn_apply_res (csrc/train_bn.hip): out[p][c] = fl(act(fma(u, s, b)) + res[p][c]), dense [n_pix][C] -- the last
 * BatchNorm of an inverted-residual block in training mode with the block's residual (train.block_forward_batch): the
 * pre-activation is uavsal_bn_apply's one fused multiply-add, the sum one more rounding.  `res` is an NHWC view with its own
 * pitch ldr >= C (a channel slice is read in place).  C % 4 == 0: a lane owns four channels of a pixel, 16-byte accesses, the
 * item order of uavsal_bn_apply.  ONE launch; element-wise, so two calls return the same bits.  Errors as uavsal_bn_apply. */
typedef struct uavsal_bn_apply_res_desc {
    const float* u;  int32_t ld;
    const float* s;  const float* b;                /* [C] */
    const float* res;  int32_t ldr;                 /* [n_pix] rows of C floats, ldr apart */
    float* out;                                     /* dense [n_pix][C] */
    int64_t n_pix;  int32_t C, act;
} uavsal_bn_apply_res_desc;

int uavsal_bn_apply_res(const uavsal_bn_apply_res_desc* d, uavsal_stream_t stream);
int uavsal_block_bn_sizeof_desc(int which);   /* 0 bn_apply_res; uavsal_bn_sizeof_desc's list stays closed (UAVSAL_ABI_VERSION stays 20) */

/* ---- repacking refreshed weights on the device (csrc/repack.hip) ---------------------------------------------------------
 * After an optimiser step the packed copies of a module's weights are remade FROM the fp32 parameters and buffers where they
 * lie INTO the packed device tensors that exist (launch plans hold their addresses): the bytes packing.py / weights.py make
 * on the host, made by one launch.  uavsal_repack reads a table in DEVICE memory: `n_entries` uavsal_repack_entry, one per
 * packed tensor, followed by n_entries + 1 int32 `first_block` (a prefix sum of ceil(units / 256); the last is `n_blocks`,
 * the grid).  A workgroup finds its entry in the prefix array; a thread writes one unit of the destination, once.
 *
 * kind CONV (pack_conv_weight): the logical matrix m[n][k], n < Npad, k < Kpad, is 0 at n >= N or k >= C * taps; else with
 *   c, tap from k (taps == 1: c = k; taps == 9: k = ((c / kt) * 9 + tap) * kt + c % kt), the row r = n (gi > 0, a ConvLSTM's
 *   gate interleave: r = (n % 4) * gi + n / 4) falls into source s (rows[] are the cumulative row counts of up to
 *   UAVSAL_REPACK_MAX_SRC weights side by side) at row r', and m = src[s][off + r' * sN + c * sC + (flip ? taps - 1 - tap : tap)]
 *   (element strides: a plain weight has sN = Cin_full * taps, sC = taps, off = first channel of the slice * taps; the
 *   transposed conv swaps sN and sC and sets flip).  With `sg` the value is fl32(m * s[c]), s[c] = fl32(sg[c] / sqrt(sv[c] +
 *   seps)) folded in double -- one fp32 multiply.  Layouts (Kpad a multiple of kt: 16 for F32, 32 for the others and for the
 *   32-float-K form of F32, which differs from F32 only through kt):
 *     F32     float [Npad][Kpad]                                         unit = 4 consecutive k
 *     F16X3   half  [Kpad/32][hi | lo][Npad][32], k order of a run permuted: position j holds k = 16 * ((j / 4) % 2) + 4 * (j / 8) + j % 4
 *     F16X3I  half  [Kpad/32][Npad][hi 32 | lo 32], natural k order
 *     F16X3J  half  [Kpad/16][Npad][hi 16 | lo 16], natural k order
 *     BF16    bf16  [Kpad/32][Npad][32], permuted;  BF16X3  bf16 [Kpad/32][hi | lo][Npad][32], permuted
 *   (unit = 8 consecutive halves).  The split: x = fl32(64 m), hi = half(x) to nearest even, lo = half(fl32(x - float(hi))) (the
 *   difference is exact); bf16: the same without the 64.
 * kind WINO (pack_wino_weight): float [P * P][Npad][Kpad], U[P i + l][o][c] = fl32(sum_jk G[i][j] g[j][k] G[l][k]) of the 3x3
 *   taps g of (o, c), in double in ONE order: t[i][k] = (G[i][0] g[0][k] + G[i][1] g[1][k]) + G[i][2] g[2][k], then
 *   U = (t[i][0] G[l][0] + t[i][1] G[l][1]) + t[i][2] G[l][2]; no product is fused with a sum.  G ([P][3], row-major in `G`)
 *   comes from the caller.  Zero at o >= N or c >= C.  unit = one (o, c) of [Npad][Kpad].
 * kind FOLD: float [Npad]; `layout` says which vector of the BatchNorms lying side by side (src = gamma, beta, mean, var,
 *   eps; rows[] cumulative): SCALE g / sqrt(v + eps), BIAS b - m * scale (the unrounded scale), RSTD 1 / sqrt(v + eps), each in
 *   double and rounded once, MEAN copied; channels N .. Npad hold `pad`.  unit = one channel.
 * kind DW: float [9][N], tap-major, of depthwise weights [C_s][1][3][3] side by side.  kind COPY: `units` floats of src[0].
 * kind COPY_T: float [C][N], the transpose of src[0] = [N][C] (a 1x1 conv weight [Cout][Cin] as the small-channel fused block
 *   kernel holds it, [Cin][Cout]: csrc/fused_ir.hip); unit = one element of the destination, units = N * C.
 * Every divide and square root is the correctly rounded one.  The caller answers for the table: every pointer a device
 * pointer to fp32 data of the stated extent, dst 16-byte aligned and as large as the layout says.  uavsal_repack itself
 * checks only what it can see from the host: a non-null 16-byte aligned table, positive counts, n_blocks below
 * UAVSAL_REPACK_MAX_BLOCKS. */
#define UAVSAL_REPACK_MAX_SRC 4
#define UAVSAL_REPACK_MAX_BLOCKS (1 << 24)  /* n_blocks at or above it: UAVSAL_ESHAPE (256 threads each, under 2^32 a launch) */
enum { UAVSAL_REPACK_CONV = 0, UAVSAL_REPACK_WINO = 1, UAVSAL_REPACK_FOLD = 2, UAVSAL_REPACK_DW = 3, UAVSAL_REPACK_COPY = 4,
       UAVSAL_REPACK_COPY_T = 5 };
enum { UAVSAL_REPACK_F32 = 0, UAVSAL_REPACK_F16X3 = 1, UAVSAL_REPACK_F16X3I = 2, UAVSAL_REPACK_F16X3J = 3, UAVSAL_REPACK_BF16 = 4,
       UAVSAL_REPACK_BF16X3 = 5 };
enum { UAVSAL_REPACK_SCALE = 0, UAVSAL_REPACK_BIAS = 1, UAVSAL_REPACK_RSTD = 2, UAVSAL_REPACK_MEAN = 3 };

typedef struct uavsal_repack_entry {
    int32_t kind, layout;                   /* layout: the conv layout, or which vector a FOLD entry writes */
    void* dst;
    int64_t units;                          /* threads of this entry */
    const float* src[UAVSAL_REPACK_MAX_SRC];        /* weights; FOLD: gamma */
    const float* beta[UAVSAL_REPACK_MAX_SRC];
    const float* mean[UAVSAL_REPACK_MAX_SRC];
    const float* var[UAVSAL_REPACK_MAX_SRC];
    double eps[UAVSAL_REPACK_MAX_SRC];
    int32_t rows[UAVSAL_REPACK_MAX_SRC];    /* cumulative rows (channels) of the sources */
    int32_t n_src;
    int32_t N, C, taps, Npad, Kpad, kt, flip, gi;
    int32_t P;                              /* WINO: r + 2 */
    int64_t sN, sC, off;
    const float* sg;  const float* sv;  double seps;        /* CONV: gamma, var, eps of the scale in the rows, or null */
    float pad;  int32_t reserved;
    double G[18];
} uavsal_repack_entry;

int uavsal_repack(const void* table, int n_entries, int n_blocks, uavsal_stream_t stream);
int uavsal_repack_sizeof_desc(void);

/* ---- launch plan: a recorded sequence of the calls above, run natively ------------ */
typedef struct uavsal_plan uavsal_plan;

uavsal_plan* uavsal_plan_create(void);
void uavsal_plan_destroy(uavsal_plan* p);
int uavsal_plan_add_conv(uavsal_plan* p, const uavsal_conv_desc* d);
int uavsal_plan_add_dw(uavsal_plan* p, const uavsal_dw_desc* d);
int uavsal_plan_add_dw_dot(uavsal_plan* p, const uavsal_dw_dot_desc* d);
int uavsal_plan_add_stem(uavsal_plan* p, const uavsal_stem_desc* d);
int uavsal_plan_add_bilinear(uavsal_plan* p, const uavsal_bilinear_desc* d);
int uavsal_plan_add_tdiff(uavsal_plan* p, const uavsal_tdiff_desc* d);
int uavsal_plan_add_wino_input(uavsal_plan* p, const uavsal_wino_desc* d);
int uavsal_plan_add_wino_output(uavsal_plan* p, const uavsal_wino_desc* d);
int uavsal_plan_add_tsum(uavsal_plan* p, const uavsal_tsum_desc* d);
int uavsal_plan_add_layout(uavsal_plan* p, const uavsal_layout_desc* d);
int uavsal_plan_add_copy(uavsal_plan* p, const uavsal_copy_desc* d);
int uavsal_plan_add_fused_ir(uavsal_plan* p, const uavsal_fused_ir_desc* d);
int uavsal_plan_add_fill(uavsal_plan* p, const uavsal_fill_desc* d);
/* The plan owns one device error word (for uavsal_conv_desc.err of its convs) and a host mirror of it.
 * add_guard records a uavsal_guard over up to three output buffers with those words filled in. */
int32_t* uavsal_plan_error_word(uavsal_plan* p);
int uavsal_plan_add_guard(uavsal_plan* p, float* b0, int64_t n0, float* b1, int64_t n1, float* b2, int64_t n2);
/* Outcome of the most recent uavsal_plan_run / uavsal_plan_graph_launch: 0 = completed without a device
 * error (or, with wait == 0, still running); UAVSAL_EDEVICE = a kernel set the error word (returned
 * once: the words are cleared; the caller re-zeroes its stream-K workspaces).  wait != 0 blocks until
 * the run has finished. */
int uavsal_plan_status(uavsal_plan* p, int wait);
/* Re-point one tensor of a recorded op at the caller's buffer, so that a forward reads the caller's frames /
 * priors / state in place and writes the map / state straight into freshly allocated outputs (no staging
 * copies, no clones; SURVEY.md 8(b): inputs are not modified, outputs are owned by the caller).
 * `slot`: conv 0 = a, 1 = out;  stem 0 = in (fp32), 1 = in_u8 (the other is cleared);  layout 0 = in, 1 = out;
 * guard 0..2 = buf[slot].  Shapes, strides and every other field stay as recorded.  Not available once the
 * plan has been captured into a graph (UAVSAL_ESTATE): a graph replays fixed addresses. */
int uavsal_plan_patch_ptr(uavsal_plan* p, int op, int slot, void* ptr);
/* Parallel branches: ops are recorded on the current lane (0 = the caller's stream, 1..7 = private
 * streams).  fork(l): lane l starts after everything recorded on lane 0 so far; join(l): lane 0 waits
 * for lane l.  Every forked lane must be joined before the plan ends.  A captured plan keeps the
 * branches as parallel graph nodes.  enable_lanes(0) runs everything on the caller's stream. */
int uavsal_plan_set_lane(uavsal_plan* p, int lane);
int uavsal_plan_add_fork(uavsal_plan* p, int lane);
int uavsal_plan_add_join(uavsal_plan* p, int lane);
int uavsal_plan_enable_lanes(uavsal_plan* p, int on);
int uavsal_plan_size(const uavsal_plan* p);
/* launch ops [first, last) in order on `stream` (last < 0: to the end).  Lanes are honoured when the whole plan runs; a sub-range is
 * launched flat on `stream`.  A run that reaches the end of the plan -- whole, or the second of two ranges (the streaming driver issues
 * everything in front of the recurrence, waits for the previous group's state, then the rest) -- is the one uavsal_plan_status reports on. */
int uavsal_plan_run(uavsal_plan* p, int first, int last, uavsal_stream_t stream);
/* Groups of ops that a run can leave out -- work whose inputs did not change since the run that last did it and whose
 * outputs are still in place (the engine's prior nets).  group_mark: ops [first, last) belong to `group` (0..31); a group
 * that runs on a side lane takes its fork and its join with it, and several calls may add ranges to one group (the join
 * is usually recorded later than the branch).  group_enable(on = 0): runs leave the group out entirely -- its kernels and
 * its fork / join event operations; nothing of it needs patch_ptr then -- until it is enabled again.  Holds for whole
 * runs, sub-ranges and the capture; only the per-op timer below ignores the switch.  A captured graph holds the ops it
 * was captured with: once it is built, marking and CHANGING a switch return UAVSAL_ESTATE.
 * group_launches: plan ops of the group that launch (everything but its fork / join).  last_launches: plan ops that
 * launched in the most recent run (a run issued as two ranges: both; a graph launch: what was captured).  Both count
 * ops, not kernels: an op may issue more than one kernel (a GEMM with a split-K reduction is two). */
int uavsal_plan_group_mark(uavsal_plan* p, int group, int first, int last);
int uavsal_plan_group_enable(uavsal_plan* p, int group, int on);
int uavsal_plan_group_launches(const uavsal_plan* p, int group);
int uavsal_plan_last_launches(const uavsal_plan* p);
/* Frame repeat: a run-time mode of ONE pair of conv ops of a recorded plan -- the 1x1 expand `op_pw` of an inverted-residual
 * block and the depthwise -> projection launch `op_dwpl` that alone reads the expand's output -- for calls in which the
 * block's input is the same for image f and image (f / src_div * src_div) % src_mod (the image map of uavsal_bilinear_desc:
 * the fusion block behind the priors, model.py:363-364, when the caller's priors are one map set repeated over the frames).
 * While it is on, a run that starts at the plan's first op and reaches past the pair (the whole plan, or the head range of
 * a streamed run) computes only the src_mod / src_div "source" images: the expand walks the M tiles that hold a row of a
 * source image (a tile that straddles into a neighbour is computed whole) with the kernel, tile, K shares, workspace and
 * ticket layout of the full launch and leaves the other rows of the hidden tensor unwritten; the projection walks the
 * patches of the source images and stores each to every image that repeats it.  The outputs are bit-identical to the
 * full launches'.  Any other range, the per-op timer and a captured graph run the pair in full, and so does a pair whose
 * routes could change an element's summation order with its tile's position or do not carry the map: armed are the
 * expand routes UAVSAL_ROUTE_K32 with tile 8 / 10 / 11 (any K shares) and the projection route UAVSAL_ROUTE_DWPROJ with
 * whole-K tiles, both UAVSAL_EPI_AFFINE on dense images, without residual or split shadow.
 * Called at run time (not while recording); returns 1 when the following runs apply the mode, 0 when they run in full
 * (`on` == 0, a refused pair, nothing to leave out, a built graph), negative on bad arguments.
 * frame_repeat_workgroups: the grid that the kernel of op_pw (`which` = 0) / op_dwpl (1) was started with in the most
 * recent uavsal_plan_run that launched it, in full or not. */
int uavsal_plan_frame_repeat(uavsal_plan* p, int op_pw, int op_dwpl, int src_mod, int src_div, int on);
int uavsal_plan_frame_repeat_workgroups(const uavsal_plan* p, int which);
/* Recurrence modes: run-time modes of the F(2x2) ConvTWA steps of a recorded plan, in the manner of frame repeat -- they apply
 * to uavsal_plan_run outside a stream capture and only to a range that holds every op concerned; any other range, the per-op
 * timer and a captured graph run the recorded ops in full.  Outputs are bit-identical either way.
 * plan_seam: registers (on = 1) or drops (0) the pair `op_xout` (output transform of step t) / `op_xin` (input transform of
 *   step t + 1); while registered, a run whose range holds both issues uavsal_wino_seam in their place.  Returns 1 when
 *   registered, 0 when not (on == 0; another op between the two or different lanes; descriptors uavsal_wino_seam refuses; a
 *   built graph), negative on bad arguments.  The caller answers for the memory: the V planes of step t + 1 must not overlap
 *   anything op_xout reads or writes (the engine checks its arena before it registers a pair).
 * plan_zero_state: names the layouts that stage the caller's initial state (ops op_state_in_first .. op_state_in_last,
 *   inclusive; -1, -1: the plan has none, the state is resident) and the three ops of step 0, and switches the mode on / off
 *   for the runs that follow.  While on -- the caller vouches that the state step 0 reads is all +0 bits -- a run whose range
 *   holds them leaves the layouts, the input transform and the GEMM out and launches the output transform in the zero-h form
 *   (uavsal_wino_output_zero_h, or the seam's).  Returns 1 / 0 as above (0 also for a step that is not F(2x2) ConvTWA).
 *   Not covered: non-finite recurrent weights (0 * inf), which the full path turns into NaN.
 * Neither mode moves uavsal_plan_last_launches: an op served by a seam launch or left out still counts.
 * plan_mode_report: what the most recent run did -- out[0] seam pairs fused, out[1] ops left out by the zero state, out[2]
 *   launch calls actually issued for plan ops (one per op that ran, one per fused pair), out[3] reserved (0). */
int uavsal_plan_seam(uavsal_plan* p, int op_xout, int op_xin, int on);
int uavsal_plan_zero_state(uavsal_plan* p, int op_state_in_first, int op_state_in_last, int op_xin0, int op_gemm0, int op_xout0, int on);
int uavsal_plan_mode_report(const uavsal_plan* p, int out[4]);
/* capture the whole plan into a hipGraph once, then replay it */
int uavsal_plan_graph_build(uavsal_plan* p, uavsal_stream_t stream);
int uavsal_plan_graph_launch(uavsal_plan* p, uavsal_stream_t stream);

/* ---- device timing on the launch stream (hipEvent) and introspection --------------- */
/* run ops [first,last) `iters` times on `stream`, return average ms per iteration in *ms
 * (hipEventRecord on `stream` around the loop, hipEventSynchronize on the stop event).  Switched-off groups are timed too. */
int uavsal_plan_time(uavsal_plan* p, int first, int last, int iters, uavsal_stream_t stream, float* ms);

int uavsal_abi_version(void);
int uavsal_sizeof_desc(int which); /* 0 conv,1 dw,2 stem,3 bilinear,4 tdiff,5 tsum,6 layout,7 post,8 guard,9 copy,10 fused_ir,11 wino,12 dw_dot,13 fill,14 score,15 letterbox,16 overlay,17 gaze,18 loss,19 conv_route */
const char* uavsal_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* UAVSAL_HIP_H */
