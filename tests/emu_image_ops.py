"""TEST INFRASTRUCTURE: the two clip I/O operations of ``motioneditor_amd.ops`` (ops.image_resize / ops.video_grid_u8, csrc/image.hip) as plain torch on
CPU tensors, with the wrappers' signatures.  The formulas are those of include/motioned_io.h, one separately rounded fp32 torch operation per operation of
the kernels.  Tests monkeypatch these over ``ops`` where the dataset and the savers run without a GPU; the GPU tests use them as the kernels' reference."""
from __future__ import annotations

import torch

F32 = torch.float32


def grid_size(b, h, w, n_rows=4):
    if b == 1:
        return h, w
    xmaps = min(n_rows, b)
    ymaps = (b + xmaps - 1) // xmaps
    return (h + 2) * ymaps + 2, (w + 2) * xmaps + 2


def _bilinear_axis(size, osize):
    scale = torch.tensor(float(size), dtype=F32) / torch.tensor(float(osize), dtype=F32)
    dst = torch.arange(osize, dtype=F32)
    src = (scale * (dst + 0.5) - 0.5).clamp_min(0.0)
    i0 = src.to(torch.int64).clamp_max(size - 1)
    i1 = (i0 + 1).clamp_max(size - 1)
    w1 = src - i0.to(F32)
    return i0, i1, 1.0 - w1, w1


def _nearest_axis(size, osize):
    scale = torch.tensor(float(size), dtype=F32) / torch.tensor(float(osize), dtype=F32)
    return torch.floor(torch.arange(osize, dtype=F32) * scale).to(torch.int64).clamp_max(size - 1)


def image_resize(src, size, mode="bilinear", *, div=1.0, add=0.0, out=None):
    if mode not in ("bilinear", "nearest"):
        raise ValueError(f"image_resize: mode must be 'bilinear' or 'nearest', got {mode!r}")
    if src.dtype != torch.uint8 or src.dim() not in (3, 4):
        raise ValueError(f"image_resize: expected uint8 images [n, H, W, C] or [n, H, W], got {src.dtype} {tuple(src.shape)}")
    x = src if src.dim() == 4 else src[..., None]
    n, H, W, Cc = x.shape
    oh, ow = int(size[0]), int(size[1])
    if Cc not in (1, 3) or min(n, H, W) <= 0 or oh <= 0 or ow <= 0:
        raise ValueError(f"image_resize: C must be 1 or 3 and every size positive, got src {tuple(src.shape)} -> {(oh, ow)}")
    x = x.permute(0, 3, 1, 2).to(F32)                                   # [n, C, H, W]
    if mode == "bilinear":
        y0, y1, wy0, wy1 = _bilinear_axis(H, oh)
        x0, x1, wx0, wx1 = _bilinear_axis(W, ow)
        wy0, wy1 = wy0[:, None], wy1[:, None]
        r0, r1 = x[:, :, y0], x[:, :, y1]
        a, b, c, d = r0[..., x0], r0[..., x1], r1[..., x0], r1[..., x1]
        v = wy0 * (wx0 * a + wx1 * b) + wy1 * (wx0 * c + wx1 * d)
    else:
        v = x[:, :, _nearest_axis(H, oh)][..., _nearest_axis(W, ow)]
    res = v / torch.tensor(float(div), dtype=F32) + torch.tensor(float(add), dtype=F32)
    if out is not None:
        out.copy_(res)
        return out
    return res.contiguous()


def video_grid_u8(videos, n_rows=4, rescale=False, out=None):
    if videos.dtype != F32 or videos.dim() != 5:
        raise ValueError(f"video_grid_u8: expected an fp32 video [b, c, f, h, w], got {videos.dtype} {tuple(videos.shape)}")
    b, c, f, h, w = videos.shape
    if c not in (1, 3) or min(b, f, h, w) <= 0 or int(n_rows) <= 0:
        raise ValueError(f"video_grid_u8: c must be 1 or 3, every size and n_rows positive, got {tuple(videos.shape)}, n_rows {n_rows}")
    Hg, Wg = grid_size(b, h, w, int(n_rows))
    x = videos.expand(b, 3, f, h, w).permute(2, 0, 3, 4, 1)               # [f, b, h, w, 3]
    if b == 1:
        grid = x[:, 0]
    else:
        xmaps = min(int(n_rows), b)
        grid = torch.zeros(f, Hg, Wg, 3, dtype=F32)
        for k in range(b):
            gy, gx = (k // xmaps) * (h + 2) + 2, (k % xmaps) * (w + 2) + 2
            grid[:, gy:gy + h, gx:gx + w] = x[:, k]
    if rescale:
        grid = (grid + 1.0) / 2.0
    res = torch.nan_to_num(grid * 255.0, nan=0.0).clamp(0.0, 255.0).to(torch.uint8)    # the cast truncates
    if out is not None:
        out.copy_(res)
        return out
    return res.contiguous()
