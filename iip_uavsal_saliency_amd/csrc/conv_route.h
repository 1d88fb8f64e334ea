// Host-side rules of the GEMM route (uavsal_conv_route, include/uavsal_hip.h) that are functions of the descriptor alone:
// which descriptors the fp32 kernels with 32-float K stages take, and every K-split rule -- how many workgroups share
// the K loop of a tile.  conv_route (conv_gemm.hip) is their only caller: it adds the rules that need kernel symbols (the
// stream-K plan) and the order of the families; the launchers receive its answer in ConvK.ksplit.
//
// K-split decisions count work units against a FIXED number of workgroup slots (two per CU of a 256-CU part, or four for
// the 32 KB instances), not against what the occupancy query returns on the device at hand: the number of shares, hence
// the fp32 summation order, is a function of the shape only (same results on every SKU / partition mode).
#pragma once
#include "conv_gemm_common.h"

namespace uavsal_route {

inline long long rows(const uavsal_conv_desc* d) { return (long long)d->H * d->W * d->n_img; }
inline int npad(const uavsal_conv_desc* d) { return (d->Cout + 31) / 32 * 32; }
inline long long tiles(const uavsal_conv_desc* d, int bm, int bn) { return ((rows(d) + bm - 1) / bm) * ((d->Cout + bn - 1) / bn); }
// room for K shares: the partial-tile area of the caller's stream-K workspace behind its 64 KB of flags (launches on one
// lane are ordered), 0 = none
inline long long kpart_room(const uavsal_conv_desc* d) {
    return d->sk_ws && uavsal_aligned16(d->sk_ws) && d->sk_ws_bytes > 65536 ? d->sk_ws_bytes - 65536 : 0;
}

// ---- fp32, 32-float K stages (conv_gemm_k32.hip, tiles 8 .. 11) ------------------------------------------------------
// K shares per tile for `tiles` 128 x 128 tiles with `stages` 32-float K stages each (1: no split)
inline int k32_share_count(long long tiles, int stages) {
    if (tiles <= 0 || tiles * 2 > 512) return 1;
    // measured on the ConvTWA step (58 tiles x 72 stages, one clip): 2 / 3 / 4 / 6 / 8 shares = 90 / 68 / 57 / 72 / 62 us
    // (kernel + reduce launch), the 64 x 64 stream-K instance it replaces 65 -- profiles/r3_gemm_k32.md
    int ksp = (int)(512 / tiles);
    if (ksp > 4) ksp = 4;
    while (ksp > 1 && stages / ksp < 6) --ksp;
    return ksp;
}

// the gates every K split of these kernels needs: ticket region and partial area there, an epilogue the reducing share (or
// the reduce launch) carries, vector alignment, tile count inside the ticket region
inline bool k32_split_gates(const uavsal_conv_desc* d, long long ntiles) {
    if (!kpart_room(d) || (d->epi != UAVSAL_EPI_AFFINE && d->epi != UAVSAL_EPI_TWA) || d->act == UAVSAL_ACT_SIGMOID) return false;
    if (ntiles <= 0 || ntiles >= UAVSAL_SK_TICKET_MAX) return false;
    if ((d->Cout & 3) || (d->ldc & 3) || !uavsal_aligned16(d->out)) return false;
    if (d->res && ((d->ldr & 3) || !uavsal_aligned16(d->res))) return false;
    if (d->epi == UAVSAL_EPI_TWA && ((d->ldx & 3) || (d->lda & 3) || !d->res || !d->aux || !uavsal_aligned16(d->aux))) return false;
    return true;
}

// Tiles 8 / 9 / 10 (128 rows of 128 / 256 x 128).  Too few tiles for the chip and a long K walk (the ConvTWA step: 58 tiles x
// 72 stages; the 12x20 / 23x40 maps of the backbone tail): K is split over up to 4 workgroups per tile, when the partial
// area has room for 8 shares of the unpadded output.  Tiles 8 / 9: the shares meet in splitk_reduce_kernel (fixed order,
// no atomics); tile 10: in the launch, the last share to arrive adds them.
inline int k32_shares(const uavsal_conv_desc* d, int tile) {
    const long long ntiles = tiles(d, tile == 9 ? 256 : 128, 128);
    if (!k32_split_gates(d, ntiles) || 8LL * rows(d) * npad(d) * 4 > kpart_room(d)) return 1;
    return k32_share_count(ntiles, d->taps * d->Cin / 32);
}

// Tile 11 (64 x 64), shares reduced in the launch: at most 4, when the tiles alone leave most of the chip idle -- the count
// that brings the work units to about four per CU of a 256-CU part -- at least 4 stages each, whole 64 x 64 partial tiles
inline int k32s_shares(const uavsal_conv_desc* d) {
    const long long ntiles = tiles(d, 64, 64);
    if (!k32_split_gates(d, ntiles)) return 1;
    int ksp = (int)(1024 / ntiles);
    if (ksp > 4) ksp = 4;
    while (ksp > 1 && d->taps * d->Cin / 32 / ksp < 4) --ksp;
    if (ksp < 1 || ntiles * ksp * 64 * 64 * 4 > kpart_room(d)) ksp = 1;
    return ksp;
}

inline bool k32_eligible(const uavsal_conv_desc* d, int tile) {
    if (tile < 8 || tile > 11) return false;
    if (d->w_group_stride && ((tile != 8 && tile != 11) || d->taps != 1 || (((long long)d->H * d->W) & 127))) return false;
    if (d->n_group && (tile != 11 || d->taps != 1 || d->w_group_stride || d->epi != UAVSAL_EPI_AFFINE || (d->n_group & 63) ||
                       d->Cout % d->n_group || d->a_group_off < d->Cin || (d->a_group_off & 3) ||
                       (long long)d->lda < (long long)(d->Cout / d->n_group - 1) * d->a_group_off + d->Cin)) return false;
    if (d->prec != UAVSAL_PREC_F32 || d->dw_w9c || d->epi == UAVSAL_EPI_LSTM) return false;
    if (tile == 11 && d->epi == UAVSAL_EPI_TWA && ((d->ldx & 3) || (d->lda & 3) || (d->ldc & 3) || (d->Cout & 3))) return false;
    if ((d->Cin % 32) || d->Cin > UAVSAL_DWPROJ_MAX_C) return false;
    // the flat-pipeline kernel carries the vector affine epilogue; only with K split (few tiles, long K, workspace given:
    // the gates above hold then) does the reducing share also do the ConvTWA update
    if (tile == 10 && k32_shares(d, 10) <= 1 &&
        !(d->epi == UAVSAL_EPI_AFFINE && d->scale && d->bias && d->act != UAVSAL_ACT_SIGMOID && !(d->ldc & 3) && !(d->Cout & 3) &&
          uavsal_aligned16(d->out) && (!d->res || (!(d->ldr & 3) && uavsal_aligned16(d->res)))))
        return false;
    return d->taps == 1 || d->taps == 9;
}

// ---- register-staged kernel, split 16-bit precisions, the tiles of one 32 x 32 fragment per wave (3: 128 x 32, 4: 64 x 64) ---
// Fewer tiles than slots (32 KB of LDS: four workgroups per CU) and a long K walk -- the ConvTWA step, 228 tiles of 64 x 64
// x 72 K steps; the 1920 -> 256 ASPP projections at 12x20 -- split K over 2 or 4 workgroups per tile, whole taps and at
// least 12 (1x1) / 18 (3x3) K steps each; the shares' sums meet in splitk_reduce_kernel
inline int staged_shares(const uavsal_conv_desc* d, int tile, int ktiles) {
    if ((tile != 3 && tile != 4) || !kpart_room(d) || d->dw_w9c || (d->prec != UAVSAL_PREC_F16X3 && d->prec != UAVSAL_PREC_BF16X3) ||
        !(d->epi == UAVSAL_EPI_AFFINE || (d->epi == UAVSAL_EPI_TWA && d->taps == 9)))
        return 1;
    const long long ntiles = tile == 3 ? tiles(d, 128, 32) : tiles(d, 64, 64);
    int ksp = (int)(1024 / (ntiles > 0 ? ntiles : 1));
    ksp = ksp >= 4 ? 4 : (ksp >= 2 ? 2 : 1);
    while (ksp > 1 && (ktiles % (d->taps * ksp) || ktiles / ksp < (d->taps == 1 ? 12 : 18))) ksp >>= 1;
    const bool ok = (long long)ksp * rows(d) * npad(d) * 4 <= kpart_room(d) && !(d->Cout & 3) && !(d->ldc & 3) &&
                    (d->epi != UAVSAL_EPI_TWA || (!(d->ldx & 3) && !(d->lda & 3) && !(d->ldr & 3)));
    return ok ? ksp : 1;
}

// ---- LDS-halo depthwise -> projection (dwproj.hip) --------------------------------------------------------------------
// The narrowest outputs (Cout <= 32: the 1536 -> 1 decoder projection) are bound by the serial depthwise / request
// segments of a K step, not by the matrix pipe, and their 74 KB ring leaves room for two workgroups per CU: when the tiles
// (8 x 16 pixel patches) alone would leave resident slots empty, K is split over 2-4 workgroups per tile of at least 12
// 16-channel steps each (raw partial sums into the caller's workspace, summed in a fixed order by splitk_reduce_kernel):
// 96 -> 72 us fp32, 88 -> 64 f16x3 for 8 x 45 x 80 x 1536 -> 1.  The 64-wide instance gains nothing (81 vs 77 us: one
// workgroup per CU by registers in fp32, and 7 MB of partial sums to re-read), so it is not split.
inline int dwproj_shares(const uavsal_conv_desc* d) {
    if (d->Cout > 32 || !kpart_room(d)) return 1;
    const long long ntiles = (long long)d->n_img * ((d->H + 7) / 8) * ((d->W + 15) / 16);
    int ksp = (int)(512 / (ntiles > 0 ? ntiles : 1));
    if (ksp > 4) ksp = 4;
    while (ksp > 1 && (d->Cin / 16) / ksp < 12) --ksp;
    return ksp > 1 && (long long)ksp * rows(d) * npad(d) * 4 <= kpart_room(d) ? ksp : 1;
}

}  // namespace uavsal_route
