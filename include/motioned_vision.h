/*
 * motioned_vision.h -- the entry points of libmotioned.so (csrc/clip_vision.hip) behind the CLIP image encoder and the CLIP metrics: what transformers'
 * CLIPVisionModelWithProjection and CLIPImageProcessor need beyond the dense projections, LayerNorm and quick-GELU of motioned.h, and the cosine the two
 * metrics (text alignment, frame consistency) are made of.  Same library, same conventions and error codes as motioned.h (raw DEVICE pointers owned by the
 * caller, strides in ELEMENTS, every call only enqueues work on `stream`, 0 on success, ME_E* otherwise with the message in the library's last-error string
 * and the launched kernel in its last-kernel string); declared apart from motioned.h because scoring an edit is not part of the denoising-step ABI that
 * ME_ABI_VERSION numbers.  Python binds them from capi.VISION_SYMBOLS.  No entry uses atomics: two identical calls are bitwise equal.
 */
#ifndef MOTIONED_VISION_H
#define MOTIONED_VISION_H

#include <stdint.h>

#include "motioned.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The largest token count me_attn_full serves (257 = ViT-L/14 at 224 pixels, 197 = ViT-B/16, 50 = ViT-B/32). */
#define ME_ATTN_FULL_NMAX 288
int me_attn_full_nmax(void); /* ME_ATTN_FULL_NMAX of the library that was built */

/* Bidirectional self-attention of n_seq sequences of n tokens at head size 64:
 *   O[s * n + i, h * 64 + d] = sum_j softmax_j(scale * Q[s * n + i, h] . K[s * n + j, h]) V[s * n + j, h * 64 + d]
 * Q, K, V fp16 row tensors (column slices of a fused [rows, 3 * heads * 64] projection work: ldq, ldk, ldv are their row strides), O an fp16 row tensor.
 * fp16 operands on the matrix units, fp32 sums, fp32 softmax over all keys with the row maximum subtracted.
 * Refused with ME_EINVAL before any launch: dh != 64; n < 1 or n > ME_ATTN_FULL_NMAX; a row stride that is not a multiple of 8 or is < heads * 64; a pointer
 * that is null or not 16-byte aligned; scale <= 0. */
int me_attn_full(void* O, int32_t ldo, const void* Q, int32_t ldq, const void* K, int32_t ldk, const void* V, int32_t ldv, int32_t n_seq, int32_t heads, int32_t dh,
                 int32_t n, float scale, void* stream);

/* fp32 pix [n, 3, S, S] (strides img_stride, ch_stride, row_stride, unit stride along x) -> fp16 rows out[n * g * g][Kpad], g = S / patch:
 *   out[(i * g + gy) * g + gx][(c * patch + py) * patch + px] = pix[i][c][gy * patch + py][gx * patch + px]
 * -- the column order of a flattened [C, 3, patch, patch] convolution weight.  K = 3 * patch^2 is padded with zero columns to Kpad, the next multiple of 8
 * (patch 14: 588 -> 592), which the kernel writes.  ldo a multiple of 8 >= Kpad, out 16-byte aligned, S a multiple of patch. */
int me_patch_rows(void* out, int32_t ldo, const float* pix, int64_t img_stride, int64_t ch_stride, int32_t row_stride, int32_t n, int32_t S, int32_t patch, void* stream);

/* x[i * (g2 + 1)] = cls + pos[0];  x[i * (g2 + 1) + 1 + p] = patch_out[i * g2 + p] + pos[1 + p]  for i < n, p < g2: fp16 operands, fp32 sum, one rounding.
 * cls fp16 [C], pos fp16 [g2 + 1, C] contiguous; x, patch_out fp16 rows with strides ldx, ldp (multiples of 8, >= C); C a multiple of 8. */
int me_vit_tokens(void* x, int32_t ldx, const void* patch_out, int32_t ldp, const void* cls, const void* pos, int32_t n, int32_t g2, int32_t C, void* stream);

/* One axis of PIL's antialiased resampling of 8-bit images, in PIL's integer form: for output index o along the axis
 *   out = clip((sum_{k < bounds[2 o + 1]} coef[o * ksize + k] * in[bounds[2 o] + k] + 2^21) >> 22, 0, 255)       (int32, arithmetic shift)
 * axis 0: along x, src [n, H, W, C] -> out [n, H, out_size, C];  axis 1: along y, -> out [n, out_size, W, C].  uint8 HWC, C 1 or 3, unit stride along the
 * channels, C along x; row and image strides in elements.  bounds int32 [out_size, 2] and coef int32 [out_size, ksize] are built by the caller (the 22-bit
 * coefficients of the filter); a tap that would fall outside the image is skipped. */
int me_resample_u8(uint8_t* out, int64_t out_img_stride, int32_t out_row_stride, const uint8_t* src, int64_t src_img_stride, int32_t src_row_stride, int32_t n, int32_t H,
                   int32_t W, int32_t C, int32_t out_size, int32_t axis, const int32_t* bounds, const int32_t* coef, int32_t ksize, void* stream);

/* out[i][c][y][x] = ((float)src[i][top + y][left + x][c] / 255.0f - mean_c) / std_c as three separately rounded fp32 operations: uint8 [n, H, W, 3] ->
 * fp32 [n, 3, crop_h, crop_w] (strides out_img_stride, out_ch_stride, out_row_stride).  The window must lie inside the image. */
int me_crop_normalize(float* out, int64_t out_img_stride, int64_t out_ch_stride, int32_t out_row_stride, const uint8_t* src, int64_t src_img_stride,
                      int32_t src_row_stride, int32_t n, int32_t H, int32_t W, int32_t top, int32_t left, int32_t crop_h, int32_t crop_w, float mean0, float mean1,
                      float mean2, float std0, float std1, float std2, void* stream);

/* out[r] = a_r . b_r / (sqrt(a_r . a_r) sqrt(b_r . b_r)) in fp32 for fp32 rows a [rows, C] (row stride lda) and b (row stride ldb; ldb == 0: one shared row).
 * Fixed-order reduction: one wavefront per row. */
int me_cosine_rows(float* out, const float* a, int64_t lda, const float* b, int64_t ldb, int64_t rows, int32_t C, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MOTIONED_VISION_H */
