"""What editing one clip towards N targets in ONE denoising pass costs, against N two-row passes (pipelines.MotionEditorPipeline, latents [1 + N, ...]).

    python tools/multi_edit_bench.py [--frames 24 --latent 64 --targets 1 2 3 --rounds 5 --window 3] [--out profiles/multi_edit.json]

The planned step (denoise_step_planned: one me_denoise_step call per step) at the benchmark's UNet shape, ControlNet + adapter + both editors active, synthetic
weights and inputs.  For every N, in ONE process: `rounds` alternations of
    A: `window` batched steps of N targets               (UNet batch 2 (1 + N))
    B: `window` x N two-row steps, back to back           (UNet batch 4, N times: what N separate calls cost per step)
each window timed by a pair of stream events after a warm-up that records every plan; the medians over the rounds are reported as ms per step and ms per
edit, beside the row model (1 + N) / (2 N): the batch rows computed per edit, relative to the two-row step.  N = 1 runs the same code on both sides: its
A / B ratio is the spread of the measurement.  --families adds, per N, one eagerly enqueued step on ONE stream with an event pair around every launch (ops.PROFILE): the busy
time of each kernel family, beside the row model's share of the N = 1 figure -- where the batched step falls short of the model, this
says in which family.  One JSON line on stdout; --out also writes it to a file."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--latent", type=int, default=64, help="latent height = width (image size / 8)")
    ap.add_argument("--targets", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--rounds", type=int, default=5, help="alternations of (batched, separate) per N; the median is reported")
    ap.add_argument("--window", type=int, default=3, help="steps per timed window")
    ap.add_argument("--families", action="store_true", help="per N, one eager step with an event pair around every launch: busy ms per kernel family")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("multi_edit_bench: needs a GPU (a timing taken anywhere else says nothing)")
    from motioneditor_amd import ops, synth
    from motioneditor_amd.attn_control import (FullySelfAttentionControlMask, TemporalSelfAttentionControl,
                                               regiter_fully_attention_editor_diffusers, regiter_temporal_attention_editor_diffusers)
    from motioneditor_amd.models.controlnet import ControlNetModel
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    from motioneditor_amd.pipelines import MotionEditorPipeline

    f, hw = a.frames, a.latent
    x = synth.bench_inputs(f, hw, hw)
    pipe = MotionEditorPipeline(unet=UNet2DConditionModel.from_synthetic("cuda"), controlnet=ControlNetModel.from_synthetic("cuda"))
    ted = TemporalSelfAttentionControl(start_step=4, start_layer=10)
    regiter_temporal_attention_editor_diffusers(pipe, ted)
    sed = FullySelfAttentionControlMask(start_step=4, start_layer=10, source_masks=x["masks"])
    regiter_fully_attention_editor_diffusers(pipe, sed)
    pipe.scheduler.set_timesteps(50)
    pipe.max_cached_steps = 2            # the pair's plan and the current N's: each pins one step's activations
    step_index = 4                      # editors active
    t = pipe.scheduler.timesteps[step_index]

    def inputs(n):
        """[recon, edit x n]: the inversion latent repeated, one prompt per target (target 1's embedding, scaled apart), one skeleton per target."""
        lat = x["latents"][[0] + [1] * n].cuda().contiguous()
        cond = torch.cat([x["cond"][:1]] + [x["cond"][1:2] * (1.0 + 0.05 * k) for k in range(n)])
        emb = torch.cat([x["uncond"][step_index].expand(1 + n, 77, 768), cond]).cuda().contiguous()
        sk = x["skeleton"].expand(n, *x["skeleton"].shape[1:])
        images = torch.cat([sk] * 2).reshape(-1, *sk.shape[2:]).cuda().contiguous()
        return lat, emb, images

    def run(inp, count):
        for _ in range(count):
            sed.cur_step = ted.cur_step = step_index
            sed.cur_att_layer = ted.cur_att_layer = 0
            pipe.denoise_step_planned(inp[0], t, inp[1], inp[2], 7.5)

    def timed(inp, count):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(inp, count)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def family_ms(inp):
        """Busy time per kernel family of ONE eagerly enqueued step, everything on one stream (an event pair around a launch that shares the GPU with the other
        stream's launches would time both)."""
        sed.cur_step = ted.cur_step = step_index
        sed.cur_att_layer = ted.cur_att_layer = 0
        overlap, pipe.overlap_controlnet = pipe.overlap_controlnet, False
        ops.PROFILE = []
        try:
            pipe.denoise_step(inp[0], t, inp[1], inp[2], 7.5)
            torch.cuda.synchronize()
            prof = ops.PROFILE
        finally:
            ops.PROFILE = None
            pipe.overlap_controlnet = overlap
        out = {}
        for rec in prof:
            out[rec[0]] = out.get(rec[0], 0.0) + rec[3].elapsed_time(rec[4])
        return {k: round(v, 3) for k, v in sorted(out.items(), key=lambda kv: -kv[1])}

    pair = inputs(1)
    run(pair, 2)
    torch.cuda.synchronize()
    res = []
    for n in a.targets:
        inp = pair if n == 1 else inputs(n)
        run(inp, 2)                      # records the plan of this batch, then one replay
        torch.cuda.synchronize()
        batched, separate = [], []
        for _ in range(a.rounds):
            batched.append(timed(inp, a.window) / a.window)
            separate.append(timed(pair, a.window * n) / a.window)
        mb, ms = statistics.median(batched), statistics.median(separate)
        res.append(dict(targets=n, unet_batch=2 * (1 + n), batched_ms_per_step=round(mb, 3), separate_ms_per_step=round(ms, 3),
                        batched_ms_per_edit=round(mb / n, 3), separate_ms_per_edit=round(ms / n, 3), ratio=round(mb / ms, 4),
                        row_model=round((1 + n) / (2 * n), 4), batched_min_max=[round(min(batched), 3), round(max(batched), 3)],
                        separate_min_max=[round(min(separate), 3), round(max(separate), 3)]))
        if a.families:
            res[-1]["family_ms"] = family_ms(inp)
        print(f"[multi_edit_bench] N={n}: batched {mb:.2f} ms/step ({mb / n:.2f} per edit), {n} two-row steps {ms:.2f} ms ({ms / n:.2f} per edit); "
              f"ratio {mb / ms:.3f}, row model {(1 + n) / (2 * n):.3f}", file=sys.stderr, flush=True)
    pipe.release_plans()
    line = json.dumps(dict(tool="multi_edit_bench", device=torch.cuda.get_device_name(0), frames=f, latent=hw, executor="plan", editors="active",
                           rounds=a.rounds, window=a.window, results=res))
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
