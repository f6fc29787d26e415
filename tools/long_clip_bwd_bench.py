"""Time ops.temporal_attention_bwd above 64 frames (me_tattn_bwd_long, csrc/tattn_bwd_long.hip) at the UNet's temporal shapes, by stream events, beside two
yardsticks that are not the code under test and run in the same process: the forward tattn_long_kernel<dh> at the same frame count, and me_tattn_bwd at 64
frames (dh 40 / 80; at dh 160 it refuses 64 frames, its LDS tile does not fit).

    python tools/long_clip_bwd_bench.py [--out profiles/long_clip_tattn_bwd.json] [--warmup 5 --reps 7 --calls 10] [--model]

Shapes: batch 1 (training and null-text optimisation differentiate one clip), (C, npix) = (320, 4096), (640, 1024), (1280, 256), (1280, 64): the temporal
layers of a 512 x 512 clip.  The frame counts alternate inside every repetition, so drift of the box lands on all of them alike.

The expectation, written down before measuring: with nqb = ceil(frames / 64) blocks, the forward walks nqb (nqb + 1) / 2 stage passes of 64 x 64 scores
with 2 matrix products each (S, P V); the backward walks the same passes three times -- sweep 1 of the query-centric kernel with 2 products (S, dP),
sweep 2 with 3 (S, dP, dS K), the key-centric kernel with 4 (S, dP, P^T dO, dS^T Q) -- 9 products against 2, `products_vs_forward` = 4.5 in the output.
No ratio is fixed in advance: the column beside it is what was measured.

--model adds one adapter training step (examples/train_adapter.py's step) and one null-text inner iteration (util.null_optimization, one DDIM step, one
inner step) at 96 frames of 512 x 512 pixels on synthetic weights: wall time after one warm-up run and peak allocated memory."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPES = ((320, 4096), (640, 1024), (1280, 256), (1280, 64))      # (C, npix); dh = C / 8
FRAMES = (64, 72, 96, 128, 256)
BATCH = 1
PRODUCTS_FWD, PRODUCTS_BWD = 2, 2 + 3 + 4


def stage_passes(frames: int) -> int:
    nqb = (frames + 63) // 64
    return nqb * (nqb + 1) // 2


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def kernels(a) -> list:
    from motioneditor_amd import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for C, npix in SHAPES:
        dh = C // 8
        top = BATCH * max(FRAMES) * npix
        qkv = torch.randn(top, 3 * C, generator=g, device="cuda", dtype=torch.float16).mul_(0.7)    # the fused projection's output, as the UNet hands it over
        dout = torch.randn(top, C, generator=g, device="cuda", dtype=torch.float32)
        out = torch.empty((top, C), dtype=torch.float16, device="cuda")
        frames = [F for F in FRAMES if F > 64 or dh <= 80]
        calls, names, ms = {}, {}, {}
        for F in frames:
            n = BATCH * F * npix
            kw = dict(heads=8, dh=dh, batch=BATCH, frames=F, npix=npix)
            calls[F, "fwd"] = lambda n=n, kw=kw: ops.temporal_attention(qkv[:n, :C], qkv[:n, C:2 * C], qkv[:n, 2 * C:], out=out[:n], **kw)
            calls[F, "bwd"] = lambda n=n, kw=kw: ops.temporal_attention_bwd(qkv[:n, :C], qkv[:n, C:2 * C], qkv[:n, 2 * C:], None, dout[:n], **kw)
        for key, fn in calls.items():
            for _ in range(a.warmup):
                fn()
            names[key], ms[key] = ops._last_kernel(), []
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for key, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                ms[key].append(e0.elapsed_time(e1) / a.calls)
        for F in frames:
            f_ms, b_ms = median(ms[F, "fwd"]), median(ms[F, "bwd"])
            row = dict(C=C, npix=npix, dh=dh, frames=F, bwd_kernel=names[F, "bwd"], bwd_ms=round(b_ms, 4), bwd_ms_min=round(min(ms[F, "bwd"]), 4),
                       bwd_ms_max=round(max(ms[F, "bwd"]), 4), fwd_kernel=names[F, "fwd"], fwd_ms=round(f_ms, 4), bwd_over_fwd=round(b_ms / f_ms, 2),
                       products_vs_forward=PRODUCTS_BWD / PRODUCTS_FWD if F > 64 else None, stage_passes=stage_passes(F),
                       bwd_ms_per_frame=round(b_ms / F, 5))
            if (64, "bwd") in ms:
                row["bwd_ms_per_frame_vs_64_frames"] = round((b_ms / F) / (median(ms[64, "bwd"]) / 64), 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
        del qkv, dout, out, calls
        torch.cuda.empty_cache()
    return rows


def model(frames: int = 96, size: int = 512) -> dict:
    sys.path.insert(0, str(ROOT / "examples"))
    import train_adapter as ex
    from motioneditor_amd import util
    from motioneditor_amd.models.controlnet import ControlNetModel
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    from motioneditor_amd.models.vae import AutoencoderKL
    from motioneditor_amd.schedulers import DDIMScheduler
    res = {}
    vae, unet, cn = AutoencoderKL.from_synthetic("cuda"), UNet2DConditionModel.from_synthetic("cuda"), ControlNetModel.from_synthetic("cuda")

    def timed(fn):
        fn()                                                            # warm-up: scratch, transposed-weight cache, allocator
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return round((time.perf_counter() - t0) * 1e3, 1), round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    tr = util.AdapterTrainer(unet, lr=3e-5)
    batch = ex.training_batch(frames, size, size)
    ms, gib = timed(lambda: ex.step(tr, vae, cn, batch, 501))
    res["adapter_step"] = dict(frames=frames, size=size, ms=ms, peak_allocated_gib=gib, what="VAE encode, ControlNet, UNet + adapter forward / backward, clip, AdamW")
    print(json.dumps(res["adapter_step"]), flush=True)
    del tr
    torch.cuda.empty_cache()
    g = torch.Generator().manual_seed(123)
    latents = [torch.randn(1, 4, frames, size // 8, size // 8, generator=g) for _ in range(2)]
    context = torch.randn(2, 77, 768, generator=g) * 0.3
    sched = DDIMScheduler()
    sched.set_timesteps(50)

    class Pipe:
        pass
    pipe = Pipe()
    pipe.unet = unet
    ms, gib = timed(lambda: util.null_optimization(pipe, sched, latents, context, 1, 1e-5, num_ddim_steps=1))
    res["null_text_iteration"] = dict(frames=frames, size=size, ms=ms, peak_allocated_gib=gib,
                                      what="one DDIM step with one inner step: conditional forward, unconditional forward + backward + Adam, the two-branch forward that advances the latent")
    print(json.dumps(res["null_text_iteration"]), flush=True)
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--model", action="store_true", help="also one adapter step and one null-text inner iteration at 96 frames x 512 x 512")
    ap.add_argument("--no-kernels", action="store_true")
    a = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), batch=BATCH, warmup=a.warmup, reps=a.reps, calls_per_rep=a.calls,
               products=dict(forward=PRODUCTS_FWD, backward=PRODUCTS_BWD, sweep1=2, sweep2=3, key_centric=4))
    if not a.no_kernels:
        res["cases"] = kernels(a)
    if a.model:
        res["model"] = model()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
