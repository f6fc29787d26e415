/*
 * motioned_long.h -- entry points of libmotioned.so (csrc/tattn_bwd_long.hip) that differentiate the causal temporal attention on clips of 65 to 256
 * frames.  Same library, same conventions and error codes as motioned.h (raw DEVICE pointers owned by the caller, strides in ELEMENTS, every call only
 * enqueues work on `stream`, 0 on success, ME_E* otherwise with the message in me_last_error(), the launched kernels in me_last_kernel()); declared apart
 * from motioned.h because they are not part of the denoising-step ABI that ME_ABI_VERSION numbers.  Python binds them from capi.LONG_SYMBOLS.
 *
 * The reference reaches this arithmetic through torch autograd of TemporalSelfAttention._attention (models/attention_2d.py: the "(b f) d c -> (b d) f c"
 * rearrange, softmax(causal(scale q k^T)) v per pixel and head) in its three preparation stages: null-text optimisation
 * (p2p/null_text_optimization.py), adapter training (train_adaptor.py) and stage-1 background tuning (train_bg.py).
 *
 * No atomics: every output element has one owner and a fixed stage order, two identical calls are bitwise equal.
 */
#ifndef MOTIONED_LONG_H
#define MOTIONED_LONG_H

#include <stdint.h>

#include "motioned.h"

#ifdef __cplusplus
extern "C" {
#endif

/* (dq, dk, dv) of me_tattn in the plain row order, row = (b * frames + frame) * npix + pixel, for 64 < frames <= 256 (me_tattn_bwd serves frames <= 64
 * and refuses more).  The operand contract of me_tattn_bwd: q, k, v fp16 [rows, ld*], dout fp32 [rows, lddo], dq / dk / dv fp32, WRITTEN (=, not
 * accumulated), rows = batch * frames * npix, columns heads * dh, `scale` as the forward took it.
 *     P = softmax_j<=i(scale q_i . k_j),  dP = dO V^T,  dS = P o (dP - sum_j P dP),  dQ = scale dS K,  dK = scale dS^T Q,  dV = P^T dO
 * dout reaches the matrix units rounded to fp16 (P and dS too, fp32 accumulation); a query whose dout row is zero gets an exactly zero dq row.  The
 * forward stashes no log-sum-exp: the call rebuilds it, and sum_j P dP, per (row, head) in `work`.
 * Limits, each refused with ME_EINVAL before any launch:
 *   frames 65 .. 256;  dh 40, 80 or 160;  batch, npix, heads > 0 (a block takes one head: any head count) and batch * frames * npix * heads < 2^31;
 *   ldq, ldk, ldv multiples of 8, lddo, lddq, lddk, lddv of 4, every one >= heads * dh;  every pointer 16-byte aligned;
 *   work non-null, 16-byte aligned, work_bytes >= me_tattn_bwd_long_work_bytes(batch, frames, npix, heads).
 * Rows >= frames of the last 64-frame block are neither read nor written. */
int me_tattn_bwd_long(void* dq, int32_t lddq, void* dk, int32_t lddk, void* dv, int32_t lddv, const void* q, int32_t ldq, const void* k, int32_t ldk,
                      const void* v, int32_t ldv, const void* dout, int32_t lddo, int32_t batch, int32_t frames, int32_t npix, int32_t heads, int32_t dh,
                      float scale, void* work, int64_t work_bytes, void* stream);
/* 8 * batch * frames * npix * heads: two fp32 per (row, head); 0 for a non-positive size. */
int64_t me_tattn_bwd_long_work_bytes(int32_t batch, int32_t frames, int32_t npix, int32_t heads);

#ifdef __cplusplus
}
#endif
#endif /* MOTIONED_LONG_H */
