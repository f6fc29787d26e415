"""What collecting cross-attention maps costs (MutualAttentionBase.collect_cross_attention -> ops.attention_probs, csrc/attn_probs.hip).

    python tools/xattn_maps_bench.py [--frames 24 --latent 64 --rounds 5 --window 3 --reps 20] [--out profiles/xattn_maps_bench.json] [--skip-step]

Two measurements, one process:
  1. the kernel alone on the model's three shapes at `frames` x `latent`^2 (batch 4): level 0 (latent^2 tokens, dh 40), level 1 (a quarter, dh 80), level 2
     (a sixteenth, dh 160) -- at 24 f x 64^2 the 256-token layers the default collection takes are level 2 -- with beta = 1 as the editor calls it, timed by
     an event pair over `reps` launches after a warm-up, beside a library copy (ops.copy_rows) that moves the same bytes: the kernel reads Q once and reads
     and writes P, the copy reads and writes half that sum each.  The model to compare with is bytes over the copy's rate.
  2. the planned step (denoise_step_planned, ControlNet + adapter + both editors active) with collection on and off, alternating windows of `window` steps,
     `rounds` times: medians and ranges in ms per step, and their difference beside five times the kernel's time at the collected level.
One JSON line on stdout; --out also writes it to a file; a markdown table on stderr."""
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
    ap.add_argument("--tokens", type=int, default=256, help="token count collected in the step measurement")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-step", action="store_true", help="the kernel measurement only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("xattn_maps_bench: needs a GPU (a timing taken anywhere else says nothing)")
    from motioneditor_amd import ops, synth

    def timed(fn, reps):
        fn()
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    f, hw = a.frames, a.latent
    items, heads = 4 * f, 8
    g = torch.Generator(device="cuda").manual_seed(3)
    kernel = []
    for level, dh in enumerate((40, 80, 160)):
        nq = (hw >> level) ** 2
        C = heads * dh
        q = torch.randn((items * nq, C), generator=g, device="cuda", dtype=torch.float16)
        k = torch.randn((4 * 77, C), generator=g, device="cuda", dtype=torch.float16)
        kv = (torch.arange(items, device="cuda", dtype=torch.int32) // f).contiguous()
        P = torch.zeros((items * nq, 80), dtype=torch.float32, device="cuda")
        nbytes = q.numel() * 2 + 2 * items * nq * 77 * 4
        half = nbytes // 2 // 2 // 1024 * 1024           # fp16 elements of a copy that reads and writes nbytes in all
        src, dst = torch.randn((half // 1024, 1024), generator=g, device="cuda", dtype=torch.float16), torch.empty((half // 1024, 1024), device="cuda", dtype=torch.float16)
        samples_k, samples_c = [], []
        for _ in range(a.rounds):
            samples_k.append(timed(lambda: ops.attention_probs(q, k, heads=heads, dh=dh, n_items=items, nq=nq, nk=77, kv_item=kv, out=P, beta=1.0), a.reps))
            samples_c.append(timed(lambda: ops.copy_rows(dst, src), a.reps))
        mk, mc = statistics.median(samples_k), statistics.median(samples_c)
        copy_rate = 2 * src.numel() * 2 / mc / 1e6          # GB/s
        kernel.append(dict(level=level, tokens=nq, dh=dh, items=items, mbytes=round(nbytes / 1e6, 1), kernel_ms=round(mk, 4), kernel_min_max=[round(min(samples_k), 4), round(max(samples_k), 4)],
                           kernel_gbps=round(nbytes / mk / 1e6, 1), copy_ms=round(mc, 4), copy_min_max=[round(min(samples_c), 4), round(max(samples_c), 4)],
                           copy_gbps=round(copy_rate, 1), model_ms=round(nbytes / copy_rate / 1e6, 4), kernel_over_model=round(mk / (nbytes / copy_rate / 1e6), 3)))
        del q, P, src, dst
        torch.cuda.empty_cache()

    step = None
    if not a.skip_step:
        from motioneditor_amd.attn_control import (FullySelfAttentionControlMask, TemporalSelfAttentionControl,
                                                   regiter_fully_attention_editor_diffusers, regiter_temporal_attention_editor_diffusers)
        from motioneditor_amd.models.controlnet import ControlNetModel
        from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
        from motioneditor_amd.pipelines import MotionEditorPipeline
        x = synth.bench_inputs(f, hw, hw)
        pipe = MotionEditorPipeline(unet=UNet2DConditionModel.from_synthetic("cuda"), controlnet=ControlNetModel.from_synthetic("cuda"))
        ted = TemporalSelfAttentionControl(start_step=4, start_layer=10)
        regiter_temporal_attention_editor_diffusers(pipe, ted)
        sed = FullySelfAttentionControlMask(start_step=4, start_layer=10, source_masks=x["masks"])
        regiter_fully_attention_editor_diffusers(pipe, sed)
        pipe.scheduler.set_timesteps(50)
        pipe.max_cached_steps = 2            # the plan with the probes and the one without: each pins one step's activations
        step_index = 4
        t = pipe.scheduler.timesteps[step_index]
        lat = x["latents"].cuda().contiguous()
        emb = torch.cat([x["uncond"][step_index].expand(2, 77, 768), x["cond"]]).cuda().contiguous()
        sk = x["skeleton"]
        images = torch.cat([sk] * 2).reshape(-1, *sk.shape[2:]).cuda().contiguous()

        def run(count, collect):
            if collect:
                sed.collect_cross_attention(tokens=a.tokens)
            else:
                sed.stop_collecting()
            for _ in range(count):
                sed.cur_step = ted.cur_step = step_index
                sed.cur_att_layer = ted.cur_att_layer = 0
                pipe.denoise_step_planned(lat, t, emb, images, 7.5)

        def window(collect):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(a.window, collect)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / a.window

        run(2, True)
        run(2, False)
        torch.cuda.synchronize()
        entries = sed._xa_count // 2
        on, off = [], []
        for _ in range(a.rounds):
            off.append(window(False))
            on.append(window(True))
        m_on, m_off = statistics.median(on), statistics.median(off)
        lvl = next((r for r in kernel if r["tokens"] == a.tokens), None)
        step = dict(tokens=a.tokens, entries_per_step=entries, on_ms=round(m_on, 3), off_ms=round(m_off, 3), on_min_max=[round(min(on), 3), round(max(on), 3)],
                    off_min_max=[round(min(off), 3), round(max(off), 3)], delta_ms=round(m_on - m_off, 3),
                    kernel_ms_times_entries=None if lvl is None else round(entries * lvl["kernel_ms"], 3))
        pipe.release_plans()

    print("| level | tokens | dh | MB moved | kernel ms (min .. max) | GB/s | copy GB/s | model ms | kernel / model |", file=sys.stderr)
    print("|---|---|---|---|---|---|---|---|---|", file=sys.stderr)
    for r in kernel:
        print(f"| {r['level']} | {r['tokens']} | {r['dh']} | {r['mbytes']} | {r['kernel_ms']} ({r['kernel_min_max'][0]} .. {r['kernel_min_max'][1]}) | {r['kernel_gbps']} | "
              f"{r['copy_gbps']} | {r['model_ms']} | {r['kernel_over_model']} |", file=sys.stderr)
    if step is not None:
        print(f"planned step, {f} f x {hw}^2, tokens {a.tokens}: on {step['on_ms']} ms ({step['on_min_max']}), off {step['off_ms']} ms ({step['off_min_max']}), "
              f"delta {step['delta_ms']} ms, {step['entries_per_step']} x kernel = {step['kernel_ms_times_entries']} ms", file=sys.stderr, flush=True)
    line = json.dumps(dict(tool="xattn_maps_bench", device=torch.cuda.get_device_name(0), frames=f, latent=hw, rounds=a.rounds, window=a.window, reps=a.reps,
                           kernel=kernel, step=step))
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
