"""TEST INFRASTRUCTURE: ops.attention_probs (include/motioned_probe.h) restated in fp64 on the operator's own arguments -- the reference of
tests/test_probe_cpu.py (for the fp32 emulation) and tests/test_probe_gpu.py (for the kernel).  Inputs are the fp16 tensors the kernel reads, so the
only error left in a result is its own arithmetic."""
from __future__ import annotations

import torch


def heads_of(t, heads, dh):
    """[rows, heads, dh] of a row tensor [rows, >= heads * dh] or of head-major panels [heads, rows, dh]."""
    if t.dim() == 3:
        return t.permute(1, 0, 2)
    return t[:, :heads * dh].reshape(t.shape[0], heads, dh)


def head_mean_probs(q, k, *, heads, dh, n_items, nq, nk, kv_item, q_items=0, scale=None, dtype=torch.float64):
    """[n_items * nq, nk]: mean over the heads of softmax_key(scale * q_h . k_h), every operation in `dtype`."""
    scale = dh ** -0.5 if scale is None else scale
    qh, kh = heads_of(q, heads, dh).to(dtype), heads_of(k, heads, dh).to(dtype)
    out = torch.empty((n_items * nq, nk), dtype=dtype)
    for it, kit in enumerate(kv_item.tolist()):
        iq = it % q_items if q_items else it
        qi = qh[iq * nq:(iq + 1) * nq].permute(1, 0, 2)          # [H, nq, dh]
        ki = kh[kit * nk:(kit + 1) * nk].permute(1, 0, 2)        # [H, nk, dh]
        s = (qi @ ki.transpose(-1, -2)) * scale
        out[it * nq:(it + 1) * nq] = torch.softmax(s, dim=-1).sum(0) * (1.0 / heads)
    return out


def attention_probs(q, k, *, heads, dh, n_items, nq, nk, kv_item, out, alpha=1.0, beta=0.0, q_items=0, scale=None):
    """fp64 `out` [n_items * nq, >= nk]: columns < nk become beta * out + alpha * mean; beta == 0 never reads them."""
    p = head_mean_probs(q, k, heads=heads, dh=dh, n_items=n_items, nq=nq, nk=nk, kv_item=kv_item, q_items=q_items, scale=scale)
    view = out[:n_items * nq, :nk]
    view.copy_(alpha * p if beta == 0 else beta * view.double() + alpha * p)
    return out


def max_logit(q, k, *, heads, dh, n_items, nq, nk, kv_item, q_items=0, scale=None):
    scale = dh ** -0.5 if scale is None else scale
    qh, kh = heads_of(q, heads, dh).double(), heads_of(k, heads, dh).double()
    best, sq, n = 0.0, 0.0, 0
    for it, kit in enumerate(kv_item.tolist()):
        iq = it % q_items if q_items else it
        s = (qh[iq * nq:(iq + 1) * nq].permute(1, 0, 2) @ kh[kit * nk:(kit + 1) * nk].permute(1, 2, 0)) * scale
        best, sq, n = max(best, float(s.abs().max())), sq + float((s * s).sum()), n + s.numel()
    return best, (sq / n) ** 0.5
