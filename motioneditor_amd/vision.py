"""Wrappers of include/motioned_vision.h (csrc/clip_vision.hip, capi.VISION_SYMBOLS): the kernels of the CLIP image encoder, of the image processor and of
the CLIP metrics.  They are `motioneditor_amd.ops.attention_full / patch_rows / vit_tokens / resample_u8 / crop_normalize / cosine_rows` -- ops.py re-exports
them -- and live in a file of their own because scoring an edit is no part of a denoising step: every one refuses to run while a step plan records.

`resample_tables` is the host half of the image processor: PIL's antialiased bicubic coefficients (ImagingResample, 8 bits per channel) in fp64, rounded to
the 22-bit integers the kernel multiplies."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import capi

PRECISION_BITS = 32 - 8 - 2     # PIL: coefficients are integers of this many fractional bits, the accumulator is an int32


def attn_full_nmax() -> int:
    return int(capi.lib().me_attn_full_nmax())


def attention_full(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, heads: int, dh: int, n_seq: int, n: int, scale: Optional[float] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Bidirectional self-attention of n_seq sequences of n <= 288 tokens at dh = 64 (me_attn_full): q, k, v are [n_seq * n, heads * dh] views (column slices
    of the fused q | k | v projection), the result is a row tensor of the same shape (`out`, when given, may be a view with a larger row stride)."""
    from . import ops
    ops._not_in_a_plan("attention_full")
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        ops._chk2d(t, "attention_full." + name)
        if t.shape[0] < n_seq * n or t.shape[1] < heads * dh:
            raise ValueError(f"attention_full.{name}: expected at least [{n_seq * n}, {heads * dh}], got {tuple(t.shape)}")
    if out is None:
        out = ops.empty(n_seq * n, heads * dh, q)
    ops._chk2d(out, "attention_full.out")
    if tuple(out.shape) != (n_seq * n, heads * dh):
        raise ValueError(f"attention_full.out: expected {(n_seq * n, heads * dh)}, got {tuple(out.shape)}")
    capi.check(capi.lib().me_attn_full(out.data_ptr(), out.stride(0), q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
                                       n_seq, heads, dh, n, dh ** -0.5 if scale is None else scale, ops._stream()), "me_attn_full")
    return out


def patch_rows(pixel_values: torch.Tensor, patch: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 pixel_values [n, 3, S, S] on the device -> fp16 rows [n (S / patch)^2, Kpad], columns in (channel, py, px) order, K = 3 patch^2 padded with zero
    columns to a multiple of 8 (me_patch_rows).  pixel_values may be a view with unit stride along x."""
    from . import ops
    ops._not_in_a_plan("patch_rows")
    x = pixel_values
    if x.dtype != torch.float32 or x.dim() != 4 or not x.is_cuda or x.shape[1] != 3 or x.shape[2] != x.shape[3]:
        raise ValueError(f"patch_rows: expected CUDA fp32 pixel_values [n, 3, S, S], got {x.dtype} {tuple(x.shape)} on {x.device}")
    n, _, S, _ = x.shape
    patch = int(patch)
    if n <= 0 or patch <= 0 or S <= 0 or S % patch:
        raise ValueError(f"patch_rows: the image size {S} must be a positive multiple of the patch size {patch}")
    if x.stride(3) != 1 and S > 1:
        raise ValueError(f"patch_rows: pixel_values must have unit stride along x, got strides {x.stride()}")
    g = S // patch
    kpad = (3 * patch * patch + 7) // 8 * 8
    if out is None:
        out = ops.empty(n * g * g, kpad, x)
    ops._chk2d(out, "patch_rows.out")
    if tuple(out.shape) != (n * g * g, kpad) or out.device != x.device:
        raise ValueError(f"patch_rows: out must be fp16 {(n * g * g, kpad)} on {x.device}, got {tuple(out.shape)}")
    s_row = x.stride(2)
    s_ch = x.stride(1)
    s_img = x.stride(0) if n > 1 else 3 * s_ch
    capi.check(capi.lib().me_patch_rows(out.data_ptr(), out.stride(0), x.data_ptr(), s_img, s_ch, s_row, n, S, patch, ops._stream()), "me_patch_rows")
    return out


def vit_tokens(patch_out: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, n: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Token rows [n (g2 + 1), C] of a ViT: row i (g2 + 1) = cls + pos[0], row i (g2 + 1) + 1 + p = patch_out[i g2 + p] + pos[1 + p]; fp32 sum rounded once
    (me_vit_tokens).  patch_out fp16 [n g2, C] (a view works), cls fp16 [C], pos fp16 [g2 + 1, C] contiguous."""
    from . import ops
    ops._not_in_a_plan("vit_tokens")
    ops._chk2d(patch_out, "vit_tokens.patch_out")
    Cc = patch_out.shape[1]
    if n <= 0 or patch_out.shape[0] % n or patch_out.shape[0] == 0:
        raise ValueError(f"vit_tokens: {patch_out.shape[0]} patch rows are not a multiple of n = {n}")
    g2 = patch_out.shape[0] // n
    if cls.dtype != ops.F16 or pos.dtype != ops.F16 or not cls.is_contiguous() or not pos.is_contiguous() or cls.numel() != Cc or tuple(pos.shape) != (g2 + 1, Cc) \
            or cls.device != patch_out.device or pos.device != patch_out.device:
        raise ValueError(f"vit_tokens: cls must be a contiguous fp16 [{Cc}] and pos a contiguous fp16 [{g2 + 1}, {Cc}] on the device, got {tuple(cls.shape)}, {tuple(pos.shape)}")
    if out is None:
        out = ops.empty(n * (g2 + 1), Cc, patch_out)
    ops._chk2d(out, "vit_tokens.out")
    if tuple(out.shape) != (n * (g2 + 1), Cc):
        raise ValueError(f"vit_tokens: out must be fp16 {(n * (g2 + 1), Cc)}, got {tuple(out.shape)}")
    capi.check(capi.lib().me_vit_tokens(out.data_ptr(), out.stride(0), patch_out.data_ptr(), patch_out.stride(0), cls.data_ptr(), pos.data_ptr(), n, g2, Cc,
                                        ops._stream()), "me_vit_tokens")
    return out


# ---- the image processor's resampling: PIL's coefficients on the host, its integer arithmetic on the device ----
def _bicubic(x: np.ndarray) -> np.ndarray:
    """Keys cubic, a = -0.5 (PIL's bicubic_filter), fp64."""
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def resample_tables(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray, int]:
    """(bounds int32 [out_size, 2] = (first input index, taps), coef int32 [out_size, ksize], ksize): PIL's precompute_coeffs + normalize_coeffs_8bpc for
    the bicubic filter with antialiasing (the support grows with the scale when shrinking), one axis, the whole axis as the box."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size <= 0 or out_size <= 0:
        raise ValueError(f"resample_tables: sizes must be positive, got {in_size} -> {out_size}")
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((out_size, 2), np.int32)
    coef = np.zeros((out_size, ksize), np.int32)
    for x in range(out_size):
        center = (x + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = _bicubic((np.arange(xmax, dtype=np.float64) + xmin - center + 0.5) * ss)
        ww = float(np.add.accumulate(w)[-1]) if xmax else 0.0        # (PIL sums in ascending order)
        if ww != 0.0:
            w = w / ww
        scaled = w * float(1 << PRECISION_BITS)
        coef[x, :xmax] = np.where(w < 0, np.trunc(-0.5 + scaled), np.trunc(0.5 + scaled)).astype(np.int32)
        bounds[x] = (xmin, xmax)
    return bounds, coef, ksize


_TABLES = {}


def _device_tables(in_size: int, out_size: int, device) -> Tuple[torch.Tensor, torch.Tensor, int]:
    key = (int(in_size), int(out_size), str(device))
    hit = _TABLES.get(key)
    if hit is None:
        b, c, ks = resample_tables(in_size, out_size)
        hit = _TABLES[key] = (torch.from_numpy(b).to(device), torch.from_numpy(c).to(device), ks)
        if len(_TABLES) > 64:
            _TABLES.pop(next(iter(_TABLES)))
    return hit


def resample_u8(src: torch.Tensor, out_size: int, axis: int, bounds: Optional[torch.Tensor] = None, coef: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One axis of PIL's antialiased bicubic resize of uint8 images [n, H, W, C] (C = 1 or 3) on the device, bit for bit (me_resample_u8): axis 0 resamples
    along x -> [n, H, out_size, C], axis 1 along y -> [n, out_size, W, C].  bounds int32 [out_size, 2] / coef int32 [out_size, ksize] default to
    resample_tables(size along the axis, out_size).  PIL's resize is resample_u8(resample_u8(x, ow, 0), oh, 1): horizontal pass first, stored as uint8."""
    from . import ops
    ops._not_in_a_plan("resample_u8")
    if src.dtype != torch.uint8 or src.dim() != 4 or not src.is_cuda:
        raise ValueError(f"resample_u8: expected CUDA uint8 images [n, H, W, C], got {src.dtype} {tuple(src.shape)} on {src.device}")
    n, H, W, Cc = src.shape
    out_size = int(out_size)
    if axis not in (0, 1) or Cc not in (1, 3) or min(n, H, W) <= 0 or out_size <= 0:
        raise ValueError(f"resample_u8: axis must be 0 or 1, C 1 or 3 and every size positive, got src {tuple(src.shape)}, axis {axis}, out_size {out_size}")
    if (W > 1 and src.stride(2) != Cc) or (Cc > 1 and src.stride(3) != 1):
        raise ValueError(f"resample_u8: src must be interleaved along x (pixel stride C, channel stride 1), got strides {src.stride()}")
    in_size = H if axis else W
    if bounds is None or coef is None:
        bounds, coef, _ = _device_tables(in_size, out_size, src.device)
    if bounds.dtype != torch.int32 or coef.dtype != torch.int32 or tuple(bounds.shape) != (out_size, 2) or coef.dim() != 2 or coef.shape[0] != out_size \
            or not bounds.is_contiguous() or not coef.is_contiguous() or bounds.device != src.device or coef.device != src.device:
        raise ValueError(f"resample_u8: bounds must be a contiguous int32 [{out_size}, 2] and coef a contiguous int32 [{out_size}, ksize] on {src.device}")
    oh, ow = (out_size, W) if axis else (H, out_size)
    if out is None:
        out = torch.empty((n, oh, ow, Cc), dtype=torch.uint8, device=src.device)
    if out.dtype != torch.uint8 or tuple(out.shape) != (n, oh, ow, Cc) or out.device != src.device or (ow > 1 and out.stride(2) != Cc) or (Cc > 1 and out.stride(3) != 1):
        raise ValueError(f"resample_u8: out must be uint8 {(n, oh, ow, Cc)} on {src.device}, interleaved along x, got {out.dtype} {tuple(out.shape)} {out.stride()}")
    s_row = src.stride(1) if H > 1 else W * Cc
    s_img = src.stride(0) if n > 1 else H * s_row
    o_row = out.stride(1) if oh > 1 else ow * Cc
    o_img = out.stride(0) if n > 1 else oh * o_row
    capi.check(capi.lib().me_resample_u8(out.data_ptr(), o_img, o_row, src.data_ptr(), s_img, s_row, n, H, W, Cc, out_size, axis, bounds.data_ptr(), coef.data_ptr(),
                                         coef.shape[1], ops._stream()), "me_resample_u8")
    return out


def crop_normalize(src: torch.Tensor, top: int, left: int, size: Tuple[int, int], mean: Sequence[float], std: Sequence[float],
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 images [n, H, W, 3] on the device -> fp32 [n, 3, ch, cw] = ((x[top: top + ch, left: left + cw] / 255 - mean) / std), three separately rounded
    fp32 operations per element (me_crop_normalize)."""
    from . import ops
    ops._not_in_a_plan("crop_normalize")
    if src.dtype != torch.uint8 or src.dim() != 4 or not src.is_cuda or src.shape[3] != 3:
        raise ValueError(f"crop_normalize: expected CUDA uint8 images [n, H, W, 3], got {src.dtype} {tuple(src.shape)} on {src.device}")
    n, H, W, _ = src.shape
    ch, cw = int(size[0]), int(size[1])
    top, left = int(top), int(left)
    if n <= 0 or ch <= 0 or cw <= 0 or top < 0 or left < 0 or top + ch > H or left + cw > W:
        raise ValueError(f"crop_normalize: the window {(top, left, ch, cw)} must lie inside the {H} x {W} image")
    if len(mean) != 3 or len(std) != 3 or any(float(s) == 0.0 for s in std):
        raise ValueError("crop_normalize: mean and std must have three entries, every std non-zero")
    if (W > 1 and src.stride(2) != 3) or src.stride(3) != 1:
        raise ValueError(f"crop_normalize: src must be interleaved along x (pixel stride 3, channel stride 1), got strides {src.stride()}")
    if out is None:
        out = torch.empty((n, 3, ch, cw), dtype=torch.float32, device=src.device)
    if out.dtype != torch.float32 or tuple(out.shape) != (n, 3, ch, cw) or out.device != src.device or (cw > 1 and out.stride(3) != 1):
        raise ValueError(f"crop_normalize: out must be fp32 {(n, 3, ch, cw)} on {src.device} with unit stride along x, got {out.dtype} {tuple(out.shape)} {out.stride()}")
    s_row = src.stride(1) if H > 1 else W * 3
    s_img = src.stride(0) if n > 1 else H * s_row
    o_row = out.stride(2) if ch > 1 else cw
    o_ch = out.stride(1)
    o_img = out.stride(0) if n > 1 else 3 * o_ch
    capi.check(capi.lib().me_crop_normalize(out.data_ptr(), o_img, o_ch, o_row, src.data_ptr(), s_img, s_row, n, H, W, top, left, ch, cw,
                                            float(mean[0]), float(mean[1]), float(mean[2]), float(std[0]), float(std[1]), float(std[2]), ops._stream()), "me_crop_normalize")
    return out


def cosine_rows(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[r] = a_r . b_r / (|a_r| |b_r|) in fp32 for fp32 rows a [rows, C] and b [rows, C], or b [C] / [1, C] as one row shared by all (me_cosine_rows).
    Views with unit column stride work."""
    from . import ops
    ops._not_in_a_plan("cosine_rows")
    if b.dim() == 1:
        b = b[None]
    for t, name in ((a, "a"), (b, "b")):
        if t.dtype != torch.float32 or t.dim() != 2 or not t.is_cuda or (t.shape[1] > 1 and t.stride(1) != 1):
            raise ValueError(f"cosine_rows.{name}: expected a CUDA fp32 2-D tensor with unit column stride, got {t.dtype} {tuple(t.shape)} {t.stride()}")
    rows, Cc = a.shape
    if rows <= 0 or Cc <= 0 or b.shape[1] != Cc or b.shape[0] not in (1, rows) or b.device != a.device:
        raise ValueError(f"cosine_rows: a {tuple(a.shape)} and b {tuple(b.shape)} must have one width and b one row or a's rows")
    shared = b.shape[0] == 1 and rows > 1
    if out is None:
        out = torch.empty((rows,), dtype=torch.float32, device=a.device)
    if out.dtype != torch.float32 or tuple(out.shape) != (rows,) or not out.is_contiguous() or out.device != a.device:
        raise ValueError(f"cosine_rows: out must be a contiguous fp32 [{rows}] on {a.device}")
    lda = a.stride(0) if rows > 1 else Cc
    ldb = 0 if shared else (b.stride(0) if rows > 1 else Cc)
    capi.check(capi.lib().me_cosine_rows(out.data_ptr(), a.data_ptr(), lda, b.data_ptr(), ldb, rows, Cc, ops._stream()), "me_cosine_rows")
    return out
