"""TEST INFRASTRUCTURE: tests/emu_clip_ops.py (the fp32 torch-CPU emulation of ``motioneditor_amd.ops`` with the text encoder's operators) plus the six
operators of include/motioned_vision.h (csrc/clip_vision.hip; wrappers in motioneditor_amd/vision.py), same argument conventions, and the two clip I/O
operators of tests/emu_image_ops.py that the metrics call.  Tests assign this module as ``ops`` where the vision tower, the image processor or the metrics
run; the GPU tests use the functions as the kernels' fp32 / integer reference.

The resampling is PIL's integer arithmetic restated on int64 tensors; its coefficient tables come from `motioneditor_amd.vision.resample_tables`, which
tests/test_clip_vision_cpu.py holds to PIL's recorded output (tests/golden/clip_image_processor.npz) through this very function."""
from __future__ import annotations

import emu_clip_ops
import numpy as np
import torch
from emu_clip_ops import *  # noqa: F401,F403
from emu_image_ops import grid_size, video_grid_u8  # noqa: F401

globals().update({k: v for k, v in vars(emu_clip_ops).items() if k.startswith("_") and not k.startswith("__")})


def attention_full(q, k, v, *, heads, dh, n_seq, n, scale=None):
    """O[s, i, h] = softmax_j(scale * Q[s, i, h] . K[s, j, h]) V[s, j, h] on [n_seq * n, heads * dh] views; no mask."""
    scale = dh ** -0.5 if scale is None else scale
    sp = lambda t: t.float()[:n_seq * n, :heads * dh].reshape(n_seq, n, heads, dh).permute(0, 2, 1, 3)   # noqa: E731
    p = torch.softmax((sp(q) @ sp(k).transpose(-1, -2)) * scale, dim=-1)
    return (p @ sp(v)).permute(0, 2, 1, 3).reshape(n_seq * n, heads * dh).to(q.dtype)


def patch_rows(pixel_values, patch, out=None, dtype=None):
    """[n, 3, S, S] -> [n g^2, Kpad]: column (c, py, px), zero columns from K = 3 patch^2 to the next multiple of 8; rounded once to `dtype`
    (default: the emulation's fp32, which rounds nothing)."""
    n, c, S, _ = pixel_values.shape
    g = S // patch
    K = c * patch * patch
    rows = pixel_values.reshape(n, c, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(n * g * g, K)
    y = torch.zeros((n * g * g, (K + 7) // 8 * 8), dtype=dtype or emu_clip_ops._EMU_DTYPE)
    y[:, :K] = rows.to(y.dtype)
    return y


def vit_tokens(patch_out, cls, pos, n, out=None):
    """row i T = cls + pos[0]; row i T + 1 + p = patch_out[i g2 + p] + pos[1 + p]; fp32 sum, one rounding to patch_out's dtype."""
    g2, C = patch_out.shape[0] // n, patch_out.shape[1]
    x = torch.cat([cls.float().reshape(1, 1, C).expand(n, 1, C), patch_out.float().reshape(n, g2, C)], dim=1) + pos.float().reshape(1, g2 + 1, C)
    return x.reshape(n * (g2 + 1), C).to(patch_out.dtype)


def resample_u8(src, out_size, axis, bounds=None, coef=None, out=None):
    """One axis of PIL's 8-bit resampling: clip((sum_k coef[o, k] * in[first[o] + k] + 2^21) >> 22, 0, 255) on integers."""
    from motioneditor_amd import vision
    n, H, W, C = src.shape
    if bounds is None or coef is None:
        b, c, _ = vision.resample_tables(H if axis else W, out_size)
        bounds, coef = torch.from_numpy(b), torch.from_numpy(c)
    x = src.long().cpu()
    x = x if axis else x.transpose(1, 2)             # [n, size along the axis, other, C]
    res = torch.empty((n, out_size) + tuple(x.shape[2:]), dtype=torch.int64)
    for o in range(out_size):
        first, cnt = int(bounds[o, 0]), int(bounds[o, 1])
        acc = (coef[o, :cnt].long().reshape(1, cnt, 1, 1) * x[:, first:first + cnt]).sum(dim=1) + (1 << 21)
        res[:, o] = (acc >> 22).clamp(0, 255)
    res = res if axis else res.transpose(1, 2)
    return res.to(torch.uint8).contiguous()


def crop_normalize(src, top, left, size, mean, std, out=None):
    """((x / 255 - mean) / std) as three separately rounded fp32 operations (numpy's), uint8 [n, H, W, 3] -> fp32 [n, 3, ch, cw]."""
    ch, cw = size
    x = src.cpu().numpy()[:, top:top + ch, left:left + cw].astype(np.float32)
    x = x / np.float32(255.0)
    x = (x - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
    return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2)))


def cosine_rows(a, b, out=None):
    if b.dim() == 1:
        b = b[None]
    a, b = a.float(), b.float()
    return (a * b).sum(dim=1) / (a.pow(2).sum(dim=1).sqrt() * b.pow(2).sum(dim=1).sqrt())
