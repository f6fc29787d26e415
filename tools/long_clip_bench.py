"""Time me_tattn (csrc/tattn.hip) at the UNet's temporal shapes for clips on both sides of 64 frames, by stream events, and report the achieved bytes per
second of the key-tiled kernel (tattn_long_kernel<dh>, 72 ... 256 frames) beside the 64-frame launch of tattn_mfma_kernel<dh,64> in the same process.

    python tools/long_clip_bench.py [--out profiles/long_clip_tattn.json] [--warmup 5 --reps 7 --calls 10]

Shapes: batch 4 (the two-branch step under classifier-free guidance), (C, npix) = (320, 4096), (640, 1024), (1280, 256), (1280, 64): the temporal layers of a
512 x 512 clip.  Bytes = 4 tensors x rows x C x 2 (algorithmic: Q, K, V read and O written once).  The yardstick is the 64-frame kernel, which reads K and V
once; the key-tiled kernel's blocks re-stage the keys below their diagonal, (nqb + 1) / 2 reads of K / V for nqb query blocks, served from L2 if the block
order works (`kv_reads` in the output; DESIGN.md 7.5 holds the measured table and what paces the kernel).  The frame counts alternate inside every
repetition, so drift of the box lands on all of them alike."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

SHAPES = ((320, 4096), (640, 1024), (1280, 256), (1280, 64))      # (C, npix); dh = C / 8
FRAMES = (48, 64, 72, 96, 128, 256)
BATCH = 4


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    from motioneditor_amd import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for C, npix in SHAPES:
        dh = C // 8
        top = BATCH * max(FRAMES) * npix
        qkv = torch.randn(top, 3 * C, generator=g, device="cuda", dtype=torch.float16).mul_(0.7)    # the fused projection's output, as the UNet hands it over
        out = torch.empty((top, C), dtype=torch.float16, device="cuda")
        calls, kernels, ms = {}, {}, {F: [] for F in FRAMES}
        for F in FRAMES:
            n = BATCH * F * npix
            calls[F] = lambda n=n, F=F: ops.temporal_attention(qkv[:n, :C], qkv[:n, C:2 * C], qkv[:n, 2 * C:], heads=8, dh=dh, batch=BATCH, frames=F, npix=npix, out=out[:n])
            for _ in range(a.warmup):
                calls[F]()
            kernels[F] = ops._last_kernel()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for F in FRAMES:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    calls[F]()
                e1.record()
                torch.cuda.synchronize()
                ms[F].append(e0.elapsed_time(e1) / a.calls)
        tbs = {}
        for F in FRAMES:
            m = sorted(ms[F])
            nbytes = 4 * BATCH * F * npix * C * 2
            tbs[F] = nbytes / m[len(m) // 2] / 1e9
        for F in FRAMES:
            m = sorted(ms[F])
            nqb = (F + 63) // 64
            rows.append(dict(C=C, npix=npix, dh=dh, frames=F, kernel=kernels[F], ms=round(m[len(m) // 2], 4), ms_min=round(m[0], 4), ms_max=round(m[-1], 4),
                             bytes=4 * BATCH * F * npix * C * 2, tb_per_s=round(tbs[F], 3), ratio_to_64_frames=round(tbs[F] / tbs[64], 3),
                             kv_reads=(nqb + 1) / 2 if F > 64 else 1.0))
            print(json.dumps(rows[-1]), flush=True)
        del qkv, out, calls
        torch.cuda.empty_cache()
    res = dict(device=torch.cuda.get_device_name(0), batch=BATCH, warmup=a.warmup, reps=a.reps, calls_per_rep=a.calls, cases=rows)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
