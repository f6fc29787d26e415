"""ops.attention_probs: the wrapper of me_attn_probs (include/motioned_probe.h, csrc/attn_probs.hip), the head-mean softmax probabilities of a text
cross-attention.  It is `motioneditor_amd.ops.attention_probs` -- ops.py re-exports it -- and lives in a file of its own because it is no part of a step
unless an editor collects attention maps (attn_control.MutualAttentionBase.collect_cross_attention)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import capi


def attention_probs(q: torch.Tensor, k: torch.Tensor, *, heads: int, dh: int, n_items: int, nq: int, nk: int, kv_item: torch.Tensor, out: torch.Tensor,
                    alpha: float = 1.0, beta: float = 0.0, q_items: int = 0, scale: Optional[float] = None) -> torch.Tensor:
    """out[item * nq + q, key] = beta * out + alpha * mean_h softmax_key(scale * q_h . k_h) over the nk <= 128 keys of kv item kv_item[item]
    (include/motioned_probe.h): the head-mean map the reference's editors keep of a text cross-attention.  q, k as ops.attention takes them (2-D row
    tensors, or [heads, rows, dh] panels); kv_item int32 [n_items] (a one-segment seg_item table is one); out fp32 [n_items * nq, >= nk], unit column
    stride, columns >= nk untouched.  beta == 0 never reads out."""
    from . import ops
    for t, n in ((q, "q"), (k, "k")):
        if t.dim() == 3:
            if t.shape[0] != heads or t.shape[2] != dh or t.stride(2) != 1 or t.dtype != ops.F16 or not t.is_cuda:
                raise ValueError(f"attention_probs: head-major {n} must be a CUDA fp16 [heads, rows, dh] tensor with unit column stride")
        else:
            ops._chk2d(t, "attention_probs." + n)
    qhm, khm = q.dim() == 3, k.dim() == 3
    if q.shape[1 if qhm else 0] < (q_items or n_items) * nq:
        raise ValueError("attention_probs: q has fewer rows than the items read")
    if kv_item.dtype != torch.int32 or kv_item.numel() != n_items or not kv_item.is_contiguous() or kv_item.device != q.device:
        raise ValueError("attention_probs: kv_item must be a contiguous int32 tensor of n_items entries on q's device")
    if out.dtype != torch.float32 or out.dim() != 2 or out.stride(1) != 1 or out.shape[0] < n_items * nq or out.shape[1] < nk or out.device != q.device:
        raise ValueError("attention_probs: out must be an fp32 [n_items * nq, >= nk] tensor with unit column stride on q's device")
    a = capi.AttnProbsArgs()
    a.Q, a.K, a.P = q.data_ptr(), k.data_ptr(), out.data_ptr()
    a.ldq, a.ldk, a.ldp = q.stride(1 if qhm else 0), k.stride(1 if khm else 0), out.stride(0)
    if qhm:
        a.hsq = q.stride(0)
    if khm:
        a.hsk = k.stride(0)
    a.heads, a.dh = heads, dh
    a.n_items, a.nq, a.nk = n_items, nq, nk
    a.kv_item, a.q_items = kv_item.data_ptr(), q_items
    a.scale = dh ** -0.5 if scale is None else scale
    a.alpha, a.beta = alpha, beta
    e0 = ops._pb()
    capi.check(capi.lib().me_attn_probs(C.byref(a), ops._stream()), "me_attn_probs")
    if e0 is not None:
        ops._pe(e0, f"attn_probs_dh{dh}", 2.0 * n_items * heads * nq * nk * dh, 2.0 * n_items * nq * heads * dh + (8.0 if beta else 4.0) * n_items * nq * nk, "", ops._last_kernel())
    return out
