/*
 * motioned_probe.h -- the entry point of libmotioned.so (csrc/attn_probs.hip) that makes the text cross-attention visible: the head-mean softmax
 * probability of every query over the text keys.  Same library, same conventions and error codes as motioned.h (raw DEVICE pointers owned by the
 * caller, strides in ELEMENTS, every call only enqueues work on `stream`, 0 on success, ME_E* otherwise with the message in me_last_error(), the
 * launched kernel in me_last_kernel()); declared apart from motioned.h because it is not part of the denoising-step ABI that ME_ABI_VERSION numbers:
 * a step that collects no maps never calls it.  Python binds it from capi.PROBE_SYMBOLS.
 *
 * The reference materialises these maps on its way to the output, attn = softmax(sim) (attn_control/fully_control_utils.py:48-66), and its editors
 * keep the head mean of every 16 x 16 cross-attention, attn.reshape(-1, heads, N, 77).mean(1) (fully_control.py:430-432).  The fused attention kernels
 * of this library never hold a normalised probability, so the map is a computation of its own: one more pass over Q, against the 77 text keys.
 */
#ifndef MOTIONED_PROBE_H
#define MOTIONED_PROBE_H

#include <stdint.h>

#include "motioned.h"

#ifdef __cplusplus
extern "C" {
#endif

/* P[item * nq + q][key] = beta * P[..] + alpha * (1 / heads) * sum_h softmax_key(scale * Q[qitem, q, h] . K[kv_item[item], key, h]),
 * qitem = q_items > 0 ? item % q_items : item.
 * The softmax is fp32 with the row maximum subtracted (QK^T on the matrix units, fp16 operands, fp32 sums); the heads are summed in ascending order in
 * registers, every output element is stored once and read at most once (only when beta != 0: beta == 0 never reads P, whatever it holds).  No atomics:
 * two identical calls are bitwise equal.
 * Limits, each refused with ME_EINVAL before any launch:
 *   every pointer non-null; Q, K 16-byte aligned, P and kv_item 4-byte aligned;  dh 40, 80 or 160;  1 <= nk <= 128;  ldp >= nk;
 *   ldq, ldk, hsq, hsk multiples of 8 (hsq, hsk >= 0);  heads, n_items, nq > 0;  q_items >= 0;  n_items * nq * heads < 2^31. */
typedef struct me_attn_probs_args {
  const void* Q;           /* fp16, rows (item*nq + q); element (row, head, d) at row*ldq + head*(hsq ? hsq : dh) + d, as in me_attn */
  const void* K;           /* fp16, rows (kv_item*nk + key); hsk as in me_attn */
  float* P;                /* fp32 [n_items*nq][ldp], ldp >= nk; columns >= nk are never touched */
  int32_t ldq, ldk, ldp;
  int32_t heads, dh;       /* dh in {40, 80, 160} */
  int32_t n_items, nq, nk; /* 1 <= nk <= 128 (77 in the model) */
  const int32_t* kv_item;  /* device int32 [n_items]: text row of each item */
  int32_t q_items;         /* as in me_attn: > 0, item i reads query item i % q_items */
  int64_t hsq, hsk;
  float scale, alpha, beta; /* P = beta*P + alpha * (1/heads) * sum_h softmax_keys(scale * q_h . k_h) */
} me_attn_probs_args;
int me_attn_probs(const me_attn_probs_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MOTIONED_PROBE_H */
