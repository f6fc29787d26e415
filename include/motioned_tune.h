/*
 * motioned_tune.h -- entry points of libmotioned.so (csrc/tune.hip) that widen stage-1 tuning (train_bg.py's trainable_modules) from the dense
 * transformer-block projections to the 3x3 convolutions and the GroupNorm affine parameters of the UNet.  Same library, same conventions and
 * error codes as motioned.h (raw DEVICE pointers owned by the caller, strides in ELEMENTS, every call only enqueues work on `stream`, 0 on success,
 * ME_E* otherwise with the message in me_last_error(), the launched kernel in me_last_kernel()); declared apart from motioned.h because they are
 * not part of the denoising-step ABI that ME_ABI_VERSION numbers.  Python binds them from capi.TUNE_SYMBOLS.
 *
 * None of them uses atomics: reductions go through fixed-order fp32 partials, two identical calls are bitwise equal.
 */
#ifndef MOTIONED_TUNE_H
#define MOTIONED_TUNE_H

#include <stdint.h>

#include "motioned.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Weight gradient of a 3x3 convolution (padding 1), all nine taps in one call:
 *     dW[n][tap][k] += alpha * sum_m dY[m, n] * X[src(m, tap), k]        tap = 3 ky + kx
 * with src exactly the ME_GATHER_CONV3 gather of me_gemm: output row m = (image, oy, ox) of an Hout x Wout grid reads the virtual pixel
 * (oy * stride + ky - 1, ox * stride + kx - 1) of the image's (Hin << ups) x (Win << ups) grid, which is input pixel (vy >> ups, vx >> ups);
 * a tap outside the virtual grid contributes a zero row, and no tap ever reads the neighbouring image or pixel row.
 * stride 1 or 2; ups 0 or 1 (nearest 2x in front of the convolution) with stride 1 only.  pad0 (the VAE encoder's pad-(0,1,0,1) form), ups 2 / 3
 * and stride 2 together with ups: ME_EINVAL.  Hout = ((Hin << ups) - 1) / stride + 1, Wout alike, M a multiple of Hout * Wout; X holds
 * (M / (Hout * Wout)) * Hin * Win rows.
 * Arithmetic as me_gemm_dw: both operands reach the MFMA as fp16 (dY cast from fp32, or given as fp16: dy_is_f16), fp32 accumulation; the row
 * axis is split into me_conv_dw_splits(M, N, K) fixed ranges whose fp32 partials a second kernel adds in index order.
 * N, K, ldx multiples of 8, lddy of 4 (fp32) / 8 (fp16), every pointer 16-byte aligned. */
typedef struct me_conv_dw_args {
  const void* dY;     /* [M, lddy] fp32 or fp16 */
  const void* X;      /* fp16 [(M / (Hout Wout)) Hin Win, ldx] */
  void* dW;           /* fp32 [N][9][K], accumulated into */
  void* work;         /* scratch of me_conv_dw_work_bytes(M, N, K) bytes, 16-byte aligned */
  int32_t M, N, K, lddy, ldx, dy_is_f16;
  int32_t Hin, Win, Hout, Wout, stride, ups, pad0;
  float alpha;
} me_conv_dw_args;

int me_conv_dw(const me_conv_dw_args* a, void* stream);
/* <= 256 MiB for every shape: the number of row splits is capped by it. */
int64_t me_conv_dw_work_bytes(int32_t M, int32_t N, int32_t K);
/* The number of row ranges me_conv_dw splits M rows into (>= 1; 0 for a non-positive size). */
int32_t me_conv_dw_splits(int32_t M, int32_t N, int32_t K);

/* GroupNorm affine gradients.  With xhat the normalised input (statistics over rows_per_group rows x C / groups channels, as me_groupnorm_bwd
 * takes them: rows_per_group = frames * pixels for the 5-D all-frames form, pixels for the per-frame form), z = gamma * xhat + beta and
 * dz = dy * silu'(z) when silu != 0 (dy otherwise):
 *     dgamma[c] += alpha * sum_rows dz * xhat        dbeta[c] += alpha * sum_rows dz
 * x, gamma, beta fp16, dy fp32, dgamma / dbeta fp32 [C]; either output may be NULL (not both).  Limits as me_groupnorm_bwd: rows a multiple of
 * rows_per_group, 1 <= groups <= 64, C a multiple of groups and of 8, C <= 2560, ldx a multiple of 8, lddy of 4, x / dy / gamma / beta / work 16-byte
 * aligned.  work: me_groupnorm_bwd_params_work_bytes(rows, rows_per_group, C, groups) bytes. */
int me_groupnorm_bwd_params(float* dgamma, float* dbeta, const void* x, int32_t ldx, const void* gamma, const void* beta, const void* dy, int32_t lddy, int64_t rows,
                            int32_t rows_per_group, int32_t C, int32_t groups, float eps, int32_t silu, float alpha, void* work, void* stream);
int64_t me_groupnorm_bwd_params_work_bytes(int64_t rows, int32_t rows_per_group, int32_t C, int32_t groups);

/* The folded weight of a convolution behind a nearest-2x upsample (me_gemm gather mode ups = 3), rewritten in place from a trained fp32 master:
 * dst fp16 [N][16][K], middle index 4 (2 py + px) + 2 ty + tx = the sum, in fp32 and in (ky, kx) order, of the taps master[n][3 ky + kx][k] with
 * (py + ky + 1) / 2 - py == ty and (px + kx + 1) / 2 - px == tx, rounded once.  master fp32 [N][9][K] contiguous and 16-byte aligned, dst 8-byte
 * aligned, K a multiple of 4. */
int me_refresh_ups4(void* dst, const float* master, int32_t N, int32_t K, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MOTIONED_TUNE_H */
