"""Time the CLIP image encoder by stream events: the full ViT-L/14 tower (24 layers, 1024 wide, 257 tokens; seeded synthetic weights) on 24 frames, and
me_attn_full alone at (24 sequences, 16 heads, 257 tokens) beside a device-to-device copy of the bytes the attention must move, on the same box.

    python tools/clip_vision_bench.py [--out profiles/clip_vision_bench.txt] [--frames 24 --warmup 3 --reps 7 --calls 5]

Bytes of the attention = q, k, v read once + o written once (algorithmic, not fetched: every 64-query block stages all keys of its head again, from L2).
FLOPs = 4 n^2 dh per (sequence, head).  The image processor (24 x 512 x 512 frames -> pixel_values) is timed too."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def timed(fn, warmup: int, reps: int, calls: int):
    """Milliseconds per call: the median and the range over `reps` groups of `calls` back-to-back calls between two events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    from motioneditor_amd import ops
    from motioneditor_amd.models.clip import CLIPImageProcessor, CLIPVisionModelWithProjection
    g = torch.Generator().manual_seed(0)
    lines = []

    def report(**row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    f, heads, n, C = a.frames, 16, 257, 1024
    qkv = (torch.randn(f * n, 3 * C, generator=g) * 0.5).to(torch.float16).cuda()
    out = torch.empty((f * n, C), dtype=torch.float16, device="cuda")
    med, lo, hi = timed(lambda: ops.attention_full(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], heads=heads, dh=64, n_seq=f, n=n, out=out), a.warmup, a.reps, a.calls * 4)
    nbytes = 2 * (qkv.numel() + out.numel())
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    cmed, _, _ = timed(lambda: dst.copy_(src), a.warmup, a.reps, a.calls * 4)
    flops = 4.0 * f * heads * n * n * 64
    report(case=f"me_attn_full ({f}, {heads}, {n})", kernel=ops._last_kernel(), ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), bytes=nbytes,
           gb_per_s=round(nbytes / med / 1e6, 1), tflops=round(flops / med / 1e9, 2), copy_same_bytes_ms=round(cmed, 4), copy_gb_per_s=round(nbytes / cmed / 1e6, 1))

    frames = torch.randint(0, 256, (f, 512, 512, 3), generator=g, dtype=torch.uint8).cuda()
    proc = CLIPImageProcessor()
    med, lo, hi = timed(lambda: proc(images=frames), a.warmup, a.reps, a.calls)
    report(case=f"CLIPImageProcessor {f} x 512 x 512 x 3 -> [{f}, 3, 224, 224]", ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4))

    tower = CLIPVisionModelWithProjection.from_synthetic("cuda")
    pv = proc(images=frames).pixel_values
    med, lo, hi = timed(lambda: tower(pv), a.warmup, a.reps, a.calls)
    c = tower.config
    report(case=f"CLIPVisionModelWithProjection ViT-L/14 ({c.num_hidden_layers} layers, {c.hidden_size} wide, {tower.tokens} tokens), {f} frames", ms=round(med, 3),
           ms_min=round(lo, 3), ms_max=round(hi, 3), ms_per_frame=round(med / f, 3), device=torch.cuda.get_device_name(0), warmup=a.warmup, reps=a.reps, calls_per_rep=a.calls)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
