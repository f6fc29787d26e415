"""TEST INFRASTRUCTURE: tests/emu_ops.py (the fp32 torch-CPU emulation of every ``motioneditor_amd.ops`` entry point) plus the three
operators of the CLIP text encoder (ops.embed_rows / ops.attention_causal / ops.quick_gelu, csrc/clip.hip), same argument conventions.
Tests assign this module as ``ops`` where the encoder runs; the GPU tests use the three functions as the kernels' fp32 reference."""
from __future__ import annotations

import emu_ops
import torch
from emu_ops import *  # noqa: F401,F403

globals().update({k: v for k, v in vars(emu_ops).items() if k.startswith("_") and not k.startswith("__")})


def quick_gelu(x):
    xf = x.float()
    return (xf * torch.sigmoid(1.702 * xf)).to(x.dtype)


def embed_rows(tok, pos, ids, seq):
    """out[r] = tok[ids[r]] + pos[r % seq], summed in fp32 and rounded once to the tables' dtype."""
    r = torch.arange(ids.numel(), device=ids.device)
    return (tok.float()[ids.reshape(-1).long()] + pos.float()[r % seq]).to(tok.dtype)


def attention_causal(q, k, v, *, heads, dh, n_seq, nq, scale=None):
    """O[s, i, h] = softmax_{j <= i}(scale * Q[s, i, h] . K[s, j, h]) V[s, j, h] on [n_seq * nq, heads * dh] views."""
    scale = dh ** -0.5 if scale is None else scale
    sp = lambda t: t.float()[:n_seq * nq, :heads * dh].reshape(n_seq, nq, heads, dh).permute(0, 2, 1, 3)   # noqa: E731
    s = (sp(q) @ sp(k).transpose(-1, -2)) * scale
    keep = torch.ones(nq, nq, dtype=torch.bool, device=s.device).tril()
    p = torch.softmax(s.masked_fill(~keep, float("-inf")), dim=-1)
    return (p @ sp(v)).permute(0, 2, 1, 3).reshape(n_seq * nq, heads * dh).to(q.dtype)
