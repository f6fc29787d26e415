/*
 * motioned_io.h -- clip I/O entry points of libmotioned.so (csrc/image.hip): the pixels between image files and the tensors of the
 * MotionEditor pipeline.  Same library, same conventions and error codes as motioned.h (raw DEVICE pointers owned by the caller, strides in
 * ELEMENTS, every call only enqueues work on `stream`, 0 on success, ME_E* otherwise with the message in me_last_error(), the launched kernel
 * in me_last_kernel()); declared apart from motioned.h because they are not part of the denoising-step ABI that ME_ABI_VERSION numbers.
 * Python binds them from capi.IO_SYMBOLS.
 *
 * Neither entry assumes contiguity: images, channels and rows carry explicit strides, so both work on views inside larger allocations.
 * Neither uses atomics; results are bitwise reproducible.
 */
#ifndef MOTIONED_IO_H
#define MOTIONED_IO_H

#include <stdint.h>

#include "motioned.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ME_RESIZE_BILINEAR 0
#define ME_RESIZE_NEAREST 1

/* n decoded images, uint8 [n][H][W][C] (C = 1 or 3 interleaved; src_row_stride >= W * C, src_img_stride >= H * src_row_stride), resized to
 * fp32 [n][C][oh][ow] (out_row_stride >= ow, out_ch_stride >= oh * out_row_stride, out_img_stride >= C * out_ch_stride; out 4-byte aligned,
 * 16-byte stores where the address allows) with  out = resized / div + add  -- a true division, then an addition, separately rounded.
 * Replaces motion_editor/data/dataset.py:121-123, 127-130, 134-137 (F.interpolate(x.float(), size=(height, width), mode='bilinear') on frames and
 * conditions, `/ 255`), :139-141 (mode='nearest' on the masks, after dataset.py:104-105 `/= 255`) and :144 (`video / 127.5 - 1.0`).
 * Semantics of F.interpolate with align_corners=False, no antialiasing, in fp32; per axis, with scale = (float)H / oh:
 *   bilinear: src = max(scale * (dst + 0.5f) - 0.5f, 0); i0 = min((int)src, H - 1); i1 = min(i0 + 1, H - 1); w1 = src - i0; w0 = 1 - w1;
 *             value = w0y * (w0x * a + w1x * b) + w1y * (w0x * c + w1x * d)
 *   nearest:  i = min((int)floorf(dst * scale), H - 1)
 * One launch per tensor of a clip. */
int me_image_resize(float* out, int64_t out_img_stride, int64_t out_ch_stride, int32_t out_row_stride, const uint8_t* src, int64_t src_img_stride,
                    int32_t src_row_stride, int32_t n, int32_t H, int32_t W, int32_t C, int32_t oh, int32_t ow, int32_t mode, float div, float add, void* stream);

/* fp32 video [b][c][f][h][w] (c = 1 or 3; strides per batch entry, channel, frame and row, unit stride along x) to uint8 frames
 * [f][Hg][Wg][3] (out_row_stride >= 3 * Wg, out_frame_stride >= Hg * out_row_stride): per frame torchvision.utils.make_grid(x, nrow=n_rows),
 * then `(x + 1.0) / 2.0` when rescale != 0, then `(x * 255).astype(np.uint8)`.  Replaces motion_editor/util.py:35-43 (save_videos_grid) and,
 * with b = 1, util.py:18-24 (save_videos_as_images).
 * make_grid, restated: one channel is replicated to three; b == 1: the frame is the image (Hg = h, Wg = w); otherwise xmaps = min(n_rows, b),
 * ymaps = ceil(b / xmaps), Hg = (h + 2) * ymaps + 2, Wg = (w + 2) * xmaps + 2, image k = y * xmaps + x at rows y * (h + 2) + 2, columns
 * x * (w + 2) + 2, every other pixel of the grid -- the cells of an incomplete last row too -- 0.  The padding is part of the grid the
 * conversion is applied to, as in the reference: it ends as 0 without rescale and as (int)(0.5 * 255) = 127 with it.
 * The conversion truncates toward zero.  One documented deviation: values outside [0, 255] after the multiplication are clamped (NaN -> 0) where
 * numpy's cast wraps; the pipeline clamps its images to [0, 1] before they get here. */
int me_video_grid_u8(uint8_t* out, int64_t out_frame_stride, int32_t out_row_stride, const float* vid, int64_t b_stride, int64_t c_stride, int64_t f_stride,
                     int32_t row_stride, int32_t b, int32_t c, int32_t f, int32_t h, int32_t w, int32_t n_rows, int32_t rescale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MOTIONED_IO_H */
