"""Peak memory and wall time of the two preparation steps that differentiate the UNet, in the three forms of the autodiff tape:

    parent  the tape keeps every tensor every call touched and releases nothing during the walk (ME_TAPE_PARENT=1: the behaviour before 7.7)
    lean    recorded towards the trained tensors / the text rows: only what a rule reads is kept, everything is released as the walk passes it
    ckpt    lean + gradient checkpointing: the segments of models/graph.py keep their boundary tensors and are recomputed in the walk

    python tools/train_memory_bench.py --frames 96 [128 256] [--size 512] [--forms parent lean ckpt] [--workloads adapter null_text] [--rounds 1] [--keep-cache] [--out profiles/train_memory.json]

adapter: examples/train_adapter.py's `step` (VAE encode, ControlNet, UNet + adapter forward / backward, clip, AdamW).  null_text: util.null_optimization, one DDIM
step with one inner step (conditional forward, unconditional forward + backward + Adam, the two-branch forward that advances the latent).  Both as
tools/long_clip_bwd_bench.py --model measures them: wall time of the SECOND run and torch.cuda.max_memory_allocated() of that run.

Every (workload, frames, form) runs in a fresh child process, one after the other (the forms of one workload alternate within a round), each under its own
time limit; the first child that fails ends the run -- an out-of-memory error is reported with the allocator's message (the request that failed) and what was allocated at that moment, and is a finding,
not something to retry.  This process never opens the GPU."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
FORMS = ("parent", "lean", "ckpt")


def child(workload: str, frames: int, size: int, form: str, keep_cache: bool = False) -> dict:
    import torch
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "examples"))
    from motioneditor_amd import util
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    unet = UNet2DConditionModel.from_synthetic("cuda")
    if form == "ckpt":
        unet.enable_gradient_checkpointing()
    stats = {}

    def timed(fn):
        fn()                                                            # warm-up: scratch, transposed-weight cache, allocator
        torch.cuda.synchronize()
        if not keep_cache:                                              # the timed run then also pays for growing the allocator's pool again: right for the peak, unfair to the time of a large form
            torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return round((time.perf_counter() - t0) * 1e3, 1), round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    if workload == "adapter":
        import train_adapter as ex
        from motioneditor_amd.models.controlnet import ControlNetModel
        from motioneditor_amd.models.vae import AutoencoderKL
        vae, cn = AutoencoderKL.from_synthetic("cuda"), ControlNetModel.from_synthetic("cuda")
        tr = util.AdapterTrainer(unet, lr=3e-5)
        tr.tape_stats = stats
        batch = ex.training_batch(frames, size, size)
        ms, gib = timed(lambda: ex.step(tr, vae, cn, batch, 501))
    else:
        from motioneditor_amd.schedulers import DDIMScheduler
        g = torch.Generator().manual_seed(123)
        latents = [torch.randn(1, 4, frames, size // 8, size // 8, generator=g) for _ in range(2)]
        context = torch.randn(2, 77, 768, generator=g) * 0.3
        sched = DDIMScheduler()
        sched.set_timesteps(50)

        class Pipe:
            pass
        pipe = Pipe()
        pipe.unet = unet
        ms, gib = timed(lambda: util.null_optimization(pipe, sched, latents, context, 1, 1e-5, num_ddim_steps=1, stats=stats))
    return dict(workload=workload, frames=frames, size=size, form=form, allocator="warm" if keep_cache else "emptied before the timed run", ms=ms, peak_allocated_gib=gib,
                tape_stashed_gib=round(stats.get("stashed_bytes", 0) / 2 ** 30, 2), grad_buffers_peak_gib=round(stats.get("grad_peak_bytes", 0) / 2 ** 30, 2),
                grad_buffers_total_gib=round(stats.get("grad_total_bytes", 0) / 2 ** 30, 2))


def child_main(a) -> int:
    import torch
    try:
        print("RESULT " + json.dumps(child(a.child[0], int(a.child[1]), a.size, a.child[2], a.keep_cache)), flush=True)
        return 0
    except torch.OutOfMemoryError as e:
        # the finding: what was being asked for, and what held the card
        print("RESULT " + json.dumps(dict(workload=a.child[0], frames=int(a.child[1]), size=a.size, form=a.child[2], out_of_memory=str(e).split("\n")[0][:400],
                                          allocated_gib=round(torch.cuda.memory_allocated() / 2 ** 30, 2), peak_allocated_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))), flush=True)
        return 3


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[96])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--forms", nargs="+", default=list(FORMS), choices=FORMS)
    ap.add_argument("--workloads", nargs="+", default=["adapter", "null_text"], choices=["adapter", "null_text"])
    ap.add_argument("--rounds", type=int, default=1, help="repeat the alternating sequence of forms this many times (the spread of a form's own repeats is the margin of any comparison)")
    ap.add_argument("--limit", type=int, default=420, help="seconds each child may take")
    ap.add_argument("--keep-cache", action="store_true", help="do not empty the allocator's cache between the warm-up and the timed run (times as tools/long_clip_bwd_bench.py --model takes them)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=3, metavar=("WORKLOAD", "FRAMES", "FORM"), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child_main(a)
    runs, failed = [], None
    for frames in a.frames:
        for workload in a.workloads:
            for rnd in range(a.rounds):
                for form in a.forms:
                    env = dict(os.environ)
                    env.pop("ME_TAPE_PARENT", None)
                    if form == "parent":
                        env["ME_TAPE_PARENT"] = "1"
                    cmd = [sys.executable, str(Path(__file__).resolve()), "--size", str(a.size), *(["--keep-cache"] if a.keep_cache else []), "--child", workload, str(frames), form]
                    try:
                        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.limit)
                        rc, out, err = r.returncode, r.stdout, r.stderr
                    except subprocess.TimeoutExpired as e:
                        rc, out, err = 124, (e.stdout or b"").decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or ""), "time limit"
                    line = next((ln[7:] for ln in out.splitlines() if ln.startswith("RESULT ")), None)
                    rec = json.loads(line) if line else dict(workload=workload, frames=frames, size=a.size, form=form)
                    rec.update(round=rnd, rc=rc)
                    if rc != 0 and "out_of_memory" not in rec:
                        rec["error"] = err.strip().splitlines()[-1][:400] if err.strip() else "no output"
                    print(json.dumps(rec), flush=True)
                    runs.append(rec)
                    if rc != 0:
                        failed = rec
                        break
                if failed:
                    break
            if failed:
                break
        if failed:
            break
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(dict(runs=runs, stopped_at=failed), indent=1) + "\n")
    return 0 if failed is None else 1


if __name__ == "__main__":
    sys.exit(main())
