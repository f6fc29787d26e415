"""TEST INFRASTRUCTURE: tests/emu_ops.py (the fp32 torch-CPU emulation of every ``motioneditor_amd.ops`` entry point) plus the operator of the
cross-attention probe (ops.attention_probs, csrc/attn_probs.hip), same argument conventions.  Tests assign this module as ``ops`` where an editor
collects attention maps; the GPU tests take the operator's own error against fp64 from it (tests/probe_cases.py: the kernel's bound is 4 x that + 2e-6)."""
from __future__ import annotations

import emu_ops
import torch
from emu_ops import *  # noqa: F401,F403

globals().update({k: v for k, v in vars(emu_ops).items() if k.startswith("_") and not k.startswith("__")})


def attention_probs(q, k, *, heads, dh, n_items, nq, nk, kv_item, out, alpha=1.0, beta=0.0, q_items=0, scale=None):
    """out[item * nq + q, key] = beta * out + alpha * mean_h softmax_key(scale * q_h . k_h) in fp32; columns >= nk untouched, beta == 0 never reads out."""
    if not 1 <= nk <= 128 or dh not in (40, 80, 160) or out.shape[1] < nk or out.dtype != torch.float32:
        raise ValueError("me_attn_probs: emulated refusal (nk 1 .. 128, dh 40 / 80 / 160, fp32 out of >= nk columns)")
    scale = dh ** -0.5 if scale is None else scale
    sp = lambda t: (t.permute(1, 0, 2) if t.dim() == 3 else t[:, :heads * dh].reshape(t.shape[0], heads, dh)).float()   # noqa: E731
    qh, kh = sp(q), sp(k)
    w = torch.tensor(alpha, dtype=torch.float32) * (torch.tensor(1.0, dtype=torch.float32) / heads)
    for it, kit in enumerate(kv_item.reshape(-1).tolist()):
        iq = it % q_items if q_items else it
        s = torch.einsum("qhd,khd->hqk", qh[iq * nq:(iq + 1) * nq], kh[kit * nk:(kit + 1) * nk]) * scale
        acc = torch.zeros((nq, nk), dtype=torch.float32)
        for h in range(heads):   # the kernel's order: one head after the other into the running sum
            acc += torch.softmax(s[h], dim=-1)
        view = out[it * nq:(it + 1) * nq, :nk]
        view.copy_(w * acc if beta == 0 else beta * view + w * acc)
    return out
