"""TEST INFRASTRUCTURE: a seeded clip folder in the reference's data/case-N layout, written with PIL (tests/test_clip_io_cpu.py, test_clip_io_gpu.py),
the resize cases both suites share, and the bound they assert."""
from __future__ import annotations

import hashlib
import os

import numpy as np
import torch

# (H, W) -> (oh, ow): up, down, down, identity
RESIZE_CASES = [((37, 53), (64, 48)), ((96, 80), (64, 64)), ((50, 70), (32, 32)), ((64, 64), (64, 64))]
# bilinear: a four-term convex combination of integers below 256 in fp32 -- 16 ulp(256) in pixel units, before the affine
BILINEAR_ATOL = 16 * 2.0 ** -15      # ulp(256) = 2^-15 for values in [128, 256): 4.9e-4


def images_u8(n, H, W, C, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (n, H, W, C) if C else (n, H, W)
    return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)


def write_clip(root, n_frames=10, H=40, W=56, *, seed=5, frame_list=True, cond="openposefull", suffix=".png", mask_dir="man.mask"):
    """images/, <mask_dir>/ (0 / 255), source_condition/<cond>/, target_condition/<cond>/ and (optionally) frame_list.txt under `root`.
    Returns {"names", "images", "source", "target", "masks"}: the frame names and the uint8 arrays that were written ([f, H, W, 3]; masks [f, H, W])."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    names = [f"{i + 1:04d}" for i in range(n_frames)]
    arrays = {"images": rng.integers(0, 256, (n_frames, H, W, 3), dtype=np.uint8), "source": rng.integers(0, 256, (n_frames, H, W, 3), dtype=np.uint8),
              "target": rng.integers(0, 256, (n_frames, H, W, 3), dtype=np.uint8), "masks": (rng.integers(0, 2, (n_frames, H, W), dtype=np.uint8) * 255)}
    folders = {"images": ("images", suffix), "source": (os.path.join("source_condition", cond), ".png"), "target": (os.path.join("target_condition", cond), ".png"),
               "masks": (mask_dir, ".png")}
    for key, (folder, suf) in folders.items():
        os.makedirs(os.path.join(root, folder), exist_ok=True)
        for name, a in zip(names, arrays[key]):
            Image.fromarray(a).save(os.path.join(root, folder, name + suf))
    if frame_list:
        with open(os.path.join(root, "frame_list.txt"), "w") as fh:
            fh.write("\n".join(names) + "\n")
    return {"names": names, **arrays}


def tree_digest(root):
    """{relative path: sha256} of every file under root."""
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            with open(p, "rb") as fh:
                out[os.path.relpath(p, root)] = hashlib.sha256(fh.read()).hexdigest()
    return out


def make_grid_numpy(videos, n_rows=4, rescale=False):
    """torchvision.utils.make_grid per frame + (x + 1) / 2 + (x * 255) -> uint8, restated in numpy (include/motioned_io.h): [b, c, f, h, w] -> [f, Hg, Wg, 3].
    Inputs in range only (the cast is numpy's, which wraps outside [0, 255])."""
    v = np.asarray(videos, dtype=np.float32)
    b, c, f, h, w = v.shape
    if c == 1:
        v = np.repeat(v, 3, axis=1)
    frames = []
    for t in range(f):
        x = v[:, :, t]                                  # [b, 3, h, w]
        if b == 1:
            grid = x[0]
        else:
            xmaps = min(n_rows, b)
            ymaps = int(np.ceil(b / xmaps))
            grid = np.zeros((3, (h + 2) * ymaps + 2, (w + 2) * xmaps + 2), dtype=np.float32)
            k = 0
            for y in range(ymaps):
                for xx in range(xmaps):
                    if k >= b:
                        break
                    grid[:, y * (h + 2) + 2:y * (h + 2) + 2 + h, xx * (w + 2) + 2:xx * (w + 2) + 2 + w] = x[k]
                    k += 1
        grid = grid.transpose(1, 2, 0)
        if rescale:
            grid = (grid + np.float32(1.0)) / np.float32(2.0)
        frames.append((grid * np.float32(255)).astype(np.uint8))
    return np.stack(frames)
