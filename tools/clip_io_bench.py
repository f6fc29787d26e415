"""Time the two clip I/O kernels (csrc/image.hip) by stream events and report the achieved bytes per second beside a device-to-device copy of the same
bytes on the same box.

    python tools/clip_io_bench.py [--out profiles/clip_io.json] [--warmup 5 --reps 7 --calls 10]

Cases: me_image_resize at 24 x 512 x 512 x 3 uint8 -> fp32 [24, 3, 512, 512] bilinear (one tensor of a case-1 clip, identity size) and from a 480 x 854 source;
me_video_grid_u8 at [2, 3, 24, 512, 512] fp32 -> uint8 [24, 516, 1030, 3].  Bytes = what the call must read + write once (algorithmic, not fetched)."""
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
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    from motioneditor_amd import ops
    g = torch.Generator().manual_seed(0)
    rows = []

    def case(name, fn, nbytes):
        med, lo, hi = timed(fn, a.warmup, a.reps, a.calls)
        buf = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")      # a copy that moves the same bytes: nbytes / 2 read + nbytes / 2 written
        dst = torch.empty_like(buf)
        cmed, _, _ = timed(lambda: dst.copy_(buf), a.warmup, a.reps, a.calls)
        rows.append(dict(case=name, kernel=ops._last_kernel() if "copy" not in name else "", ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), bytes=nbytes,
                         gb_per_s=round(nbytes / med / 1e6, 1), copy_same_bytes_ms=round(cmed, 4), copy_gb_per_s=round(nbytes / cmed / 1e6, 1)))
        print(json.dumps(rows[-1]), flush=True)

    for H, W in ((512, 512), (480, 854)):
        src = torch.randint(0, 256, (24, H, W, 3), generator=g, dtype=torch.uint8).cuda()
        out = torch.empty((24, 3, 512, 512), dtype=torch.float32, device="cuda")
        case(f"image_resize bilinear 24x{H}x{W}x3 -> 512x512", lambda: ops.image_resize(src, (512, 512), "bilinear", div=127.5, add=-1.0, out=out),
             src.numel() + out.numel() * 4)
    vid = torch.rand(2, 3, 24, 512, 512, generator=g).cuda()
    frames = torch.empty((24, *ops.grid_size(2, 512, 512, 4), 3), dtype=torch.uint8, device="cuda")
    case("video_grid_u8 [2,3,24,512,512] -> [24,516,1030,3]", lambda: ops.video_grid_u8(vid, out=frames), vid.numel() * 4 + frames.numel())
    res = dict(device=torch.cuda.get_device_name(0), warmup=a.warmup, reps=a.reps, calls_per_rep=a.calls, cases=rows)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
