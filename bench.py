"""bench.py -- denoise-steps/sec of MotionEditor's two-branch DDIM step on MI355X (BASELINE.json metric).

  python bench.py [--gpus N] [--steps K] [--warmup W]
      N = 1 runs in this process.  N > 1 without WORLD_SIZE in the environment re-launches itself as
      `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py <same flags>`;
      under torchrun (RANK / LOCAL_RANK / WORLD_SIZE set) it is one rank of that job.

One "step" = one iteration of the reference loop body (pipeline_motion_editor.py:603-648): ControlNet on
the two edit rows, one batch-4 UNet3D forward with the content-aware motion adapter and both attention
editors ACTIVE (steps >= 4, i.e. 46 of the 50 steps of a run), classifier-free guidance, DDIM update.
Workload = BASELINE.json configs[2]: 24 frames x 512^2 (64x64 latents), synthetic inputs, seeded random
weights of the SD-1.5 / ControlNet-openpose / adapter architectures (no checkpoints exist offline).

Multi-GPU: ONE clip, strong scaling (the metric is "24f x 512^2 at 1/2/4/8 MI355X"), one process per GPU, RCCL:
  --parallel auto (default)  N = 2: cfg (the two classifier-free-guidance halves; one all-gather of the noise prediction per
                             step); N = 4, 8: cfg-frames = CFG pair x frame shards of N/2 ranks (K|V halos,
                             frame<->pixel all-to-all, TemporalConv halos, GroupNorm-statistic all-reduce, each at batch 2); odd N: frames
  --parallel frames          the frame axis over all N ranks (BASELINE configs[3]/[4] as written)
  --parallel cfg | replicas  CFG pairs x N/2 clips, or one independent clip per GPU (weak scaling, no data-path collective)
value = clips * steps / max-over-ranks time.  `comm` in the JSON = data-path exchanges per step of rank 0.

Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times --steps steps and reports them; everything else is
measured only with `--full`: `roofline` / `kernels` / `kernel_families` (a second, HIP-event-instrumented pass of the same steps),
`cpu_baseline` (the CPU oracle on a bounded sample, rank 0, N = 1), the exchanges' stream-held times of the multi-GPU modes
(two more untimed steps), the per-iteration split of --null-text and the kernel families of --vae-decode.
`--dump-outputs DIR` writes what the timed path returned at its last timed step as DIR/<name>.npy (float32; seeded inputs, so two
builds can be compared output for output).
`--emulate` (test plumbing only) runs the product host code on tests/emu_ops.py (torch CPU, gloo) at tiny shapes.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

PEAK_MFMA_TFLOPS = 2500.0   # dense fp16/bf16 MFMA, MI355X_MICROARCH.md
PEAK_HBM_GBS = 8000.0
# reference-semantics TFLOP of one two-branch step (2*MAC; edited layers count their 5N keys)
REF_TFLOP = {(8, 32, 32): 9.3, (24, 64, 64): 145.7, (48, 96, 96): 918.1}


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--latent", type=int, default=64, help="latent height = width (image size / 8)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-baseline", choices=["sample", "full", "off"], default="sample",
                    help="'sample' (default; measured with --full only): the CPU oracle timed on ONE step at BASELINE configs[0] (bounded, ~1 min) next to the committed full-config measurement "
                         "(profiles/cpu_baseline_full.json); 'full': time ONE oracle step at the bench workload itself (24 f x 64x64 latents: minutes to a quarter of an hour of host "
                         "time, no GPU involved), print it as one JSON line and exit -- run once per round on the GPU box, commit the line as profiles/cpu_baseline_full.json")
    ap.add_argument("--single-branch", action="store_true",
                    help="BASELINE configs[1]: ONE clip through the single-branch UNet3D (batch 2 = the classifier-free-guidance pair), no ControlNet / adapter input / editors; "
                         "use with --frames 8")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--parallel", choices=["auto", "cfg", "replicas", "frames", "cfg-frames"], default="auto")
    ap.add_argument("--shard-exchange", choices=["lean", "gather"], default="lean",
                    help="frame sharding A/B: 'lean' = frame<->pixel all-to-all for temporal attention + two-frame halos for the adapter (default); "
                         "'gather' = the K|V all-gathers BASELINE configs[3] names")
    ap.add_argument("--shapes", action="store_true", help="print the GEMM shapes with the largest time share to stderr (from the --full roofline pass)")
    ap.add_argument("--editors", choices=["active", "inactive"], default="active",
                    help="secondary measurement: 'inactive' times the un-edited step (steps 0-3 of a 50-step run); the headline metric is 'active'")
    ap.add_argument("--inversion", action="store_true",
                    help="secondary measurement (SURVEY 8f rank 1): DDIM-inversion steps/s -- single-branch UNet with normal_infer + next_step, B = 1")
    ap.add_argument("--vae-decode", action="store_true",
                    help="secondary measurement (SURVEY 8f rank 2): frames/s of the VAE decoder (64x64 latents -> 512x512), no UNet involved")
    ap.add_argument("--null-text", action="store_true",
                    help="secondary measurement: inner iterations of the null-text optimisation (UNet forward on a tape + backward + Adam, batch 1)")
    ap.add_argument("--no-overlap", action="store_true", help="A/B: run ControlNet on the main stream instead of beside the UNet's down path")
    ap.add_argument("--no-cfg-prefix-sharing", action="store_true",
                    help="execute the classifier-free-guidance prefix (conv_in .. first cross-attention queries) for both halves of the batch, as the reference does (A/B)")
    ap.add_argument("--shard-overlap", action="store_true",
                    help="frame-sharded modes: ControlNet + content-aware adapter on the side stream beside the UNet's down path and mid block, the adapter's exchanges on "
                         "a second communicator per shard group (parallel.FrameShard.side_shard).  Off by default: bitwise the serialised sharded step on 4 ranks sharing one "
                         "GPU (tests/test_frame_shard_gpu.py), never measured between physical GPUs")
    ap.add_argument("--graph", action="store_true",
                    help="replay the step from a captured hipGraph (MotionEditorPipeline.denoise_step_graphed) instead of enqueueing its ~1100 launches from Python -- "
                         "in every mode: the sharded / CFG-parallel steps are captured with their RCCL exchanges as graph nodes.  Off by default: on one GPU it is "
                         "measured neutral (the GPU, not the host, paces the step); across GPUs it could only be validated on a world-1 RCCL group")
    ap.add_argument("--plan", action="store_true",
                    help="execute the step behind the C ABI's step-level entry point (me_plan_* / me_denoise_step, csrc/plan.hip: the launch list recorded once, "
                         "re-issued from C on the two live HIP streams; bitwise the eager result) instead of enqueueing its ~1100 launches from Python.  This is the "
                         "DEFAULT of the single-process modes up to the benchmark's size (24 f x 64^2 latents); larger shapes keep the eager executor unless --plan "
                         "is given (the plan holds one step's activations in a private pool beside the roofline pass's)")
    ap.add_argument("--eager", action="store_true", help="A/B: enqueue the launches of the step from Python (the default before round 4's me_denoise_step)")
    ap.add_argument("--main-priority", type=int, default=0, choices=[-1, 0],
                    help="A/B: HIP priority of the stream the step runs on (-1 = high: the side stream's ControlNet / adapter kernels then only take what the main "
                         "stream's kernels leave idle; 0 = torch's default stream)")
    ap.add_argument("--side-priority", type=int, default=0, choices=[-1, 0], help="A/B: HIP priority of the side stream (ControlNet + adapter)")
    ap.add_argument("--comm", choices=["auto", "torch", "rccl"], default="auto",
                    help="who issues the data-path exchanges of the sharded modes: 'torch' = torch.distributed's nccl (= RCCL) process group; 'rccl' = RCCL called "
                         "directly on our own communicators (motioneditor_amd/rccl.py: no watchdog, capturable); auto = rccl with --graph, else torch")
    ap.add_argument("--zero-tconv", action="store_true",
                    help="secondary measurement: UNet TemporalConv weights exactly zero, as in real checkpoints (resnet_2d.py:15-16) -> the launch is skipped")
    ap.add_argument("--emulate", action="store_true", help="test plumbing: torch-CPU emulation of the C ABI (tests/emu_ops.py), gloo backend")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: the roofline / per-kernel pass, the CPU baseline, the exchanges' stream-held "
                         "times (multi-GPU), the per-iteration split of --null-text, the kernel families of --vae-decode.  Off by default: a plain run "
                         "only sets up, warms up, times the steps and prints the result line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path returned at its last step as DIR/<name>.npy (float32; at most 64 MB in all, "
                         "larger outputs as a fixed seeded sample).  Multi-process runs: one file per rank, <name>.rank<r>.npy")
    return ap.parse_args()


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, arrays, rank=0, world=1):
    """Write {name: tensor | array} as out_dir/<name>.npy in float32.  If the arrays hold more than DUMP_LIMIT_BYTES in all, each is replaced by the
    same fixed, seeded sample of its flattened elements (a share of the limit proportional to its size), so that two runs stay comparable."""
    import numpy as np
    out = {}
    for k, v in arrays.items():
        if hasattr(v, "detach"):
            v = v.detach().float().cpu().numpy()
        out[k] = np.ascontiguousarray(np.asarray(v, dtype=np.float32))
    total = sum(a.size for a in out.values())
    budget = DUMP_LIMIT_BYTES // 4 - 1024 * len(out)     # float32 elements, less room for the .npy headers
    if total > budget:
        for k, a in out.items():
            idx = np.sort(np.random.default_rng(0).choice(a.size, size=max(1, a.size * budget // total), replace=False))
            out[k] = a.reshape(-1)[idx]
    d = Path(out_dir)
    d.mkdir(parents=True, exist_ok=True)
    for k, a in out.items():
        np.save(d / (f"{k}.npy" if world == 1 else f"{k}.rank{rank}.npy"), a)


def timestep_index(i, i0, n):
    """Step i of the run -> the index into the 50 DDIM timesteps (and the editors' step counter): i itself up to the last timestep, then round again
    from i0, so that any number of warm-up + timed steps stays on steps i0 .. n - 1 (the editors' active range when i0 = 4)."""
    return i if i < n else i0 + (i - i0) % (n - i0)


def free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def spawn_self(args) -> int:
    """`python bench.py --gpus N` outside torchrun: become the launcher of N ranks of this very command."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), str(Path(__file__).resolve())] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // args.gpus)))
    return subprocess.call(cmd, env=env)


def build_inputs(f, h, w, seed=33):
    from motioneditor_amd import synth
    return synth.bench_inputs(f, h, w, seed)


def make_pipeline(device, usd, csd, masks, dtype=None):
    from motioneditor_amd.attn_control import (FullySelfAttentionControlMask, TemporalSelfAttentionControl,
                                               regiter_fully_attention_editor_diffusers, regiter_temporal_attention_editor_diffusers)
    from motioneditor_amd.models.controlnet import ControlNetModel
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    from motioneditor_amd.pipelines import MotionEditorPipeline
    kw = {} if dtype is None else {"dtype": dtype}
    pipe = MotionEditorPipeline(unet=UNet2DConditionModel(usd, device, **kw), controlnet=ControlNetModel(csd, device, **kw))
    ted = TemporalSelfAttentionControl(start_step=4, start_layer=10)
    regiter_temporal_attention_editor_diffusers(pipe, ted)
    sed = FullySelfAttentionControlMask(start_step=4, start_layer=10, source_masks=masks)
    regiter_fully_attention_editor_diffusers(pipe, sed)
    pipe.scheduler.set_timesteps(50)
    return pipe, sed, ted


def planned_or_eager(pipe, state, lat, t, emb, images, guidance=7.5):
    """One step through me_denoise_step (pipe.denoise_step_planned); if RECORDING the plan fails -- before anything was ever replayed -- the run falls back to
    the Python-enqueued step for good and says so in the JSON (`launch_plan_error`): the recorded executor changes who issues the launches, not what is
    computed, and must never cost the measurement.  A plan that has been recorded and then fails to replay is a fault and propagates."""
    if state["on"]:
        try:
            return pipe.denoise_step_planned(lat, t, emb, images, guidance)
        except Exception as e:   # noqa: BLE001
            if pipe._plans:
                raise
            # denoise_step_planned has put the editors' step / layer counters back where they were before its warm-up / recording pass
            # (and dropped the half-built plan), so the eager step below IS this step.
            state["on"], state["error"] = False, f"{type(e).__name__}: {e}"
            print(f"[bench] recording the step's launch plan failed ({state['error']}); continuing with the eager executor", file=sys.stderr, flush=True)
    return pipe.denoise_step(lat, t, emb, images, guidance)


def step_tflop(f, h, w):
    """Reference-semantics TFLOP of one two-branch step: BASELINE.md's figure for the three configurations it lists, else
    scaled from config 3 by token count (attention scales super-linearly in h*w: approximate, labelled so)."""
    if (f, h, w) in REF_TFLOP:
        return REF_TFLOP[(f, h, w)], True
    return REF_TFLOP[(24, 64, 64)] * (f * h * w) / (24 * 64 * 64), False


def cpu_model() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(usd, csd, f=8, h=32, w=32):
    """CPU oracle (oracle/ref_cpu.py, fp32 torch, the validated restatement of the reference step) timed on ONE full
    two-branch step with both editors active.  Default size: BASELINE configs[0] -- 8 frames x 256^2 (32x32 latents), 9.3 TFLOP --
    the bounded sample of the default run; --cpu-baseline full times the bench workload itself."""
    import torch
    from oracle import ref_cpu
    cores = torch.get_num_threads()   # torch's default (physical cores); forcing every SMT thread measured 20x slower
    x = build_inputs(f, h, w)
    to = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}  # noqa: E731
    u, c = to(usd), to(csd)
    ddim = ref_cpu.DDIM()
    sp, tp = ref_cpu.SpatialEditor(x["masks"]), ref_cpu.TemporalEditor()
    sp.cur_step = tp.cur_step = 4
    images = torch.cat([x["skeleton"]] * 2).reshape(2 * f, 3, 8 * h, 8 * w)
    t0 = time.perf_counter()
    with torch.no_grad():
        ref_cpu.denoise_step(u, c, ddim, x["latents"], ddim.timesteps[4], x["uncond"][4], x["cond"], images, sp, tp, 7.5)
    return time.perf_counter() - t0, cores, f, h, w


def resolve_mode(args, world):
    """-> (mode, n_cfg, n_shards, n_clips)"""
    m = args.parallel
    if world == 1:
        if m == "frames":     # the frame-sharded code path on ONE rank (a world-1 RCCL group): launch-overhead / graph-capture measurements
            return "frames", 1, 1, 1
        return "single", 1, 1, 1
    if m == "auto":
        m = "cfg" if world == 2 else ("cfg-frames" if world % 2 == 0 else "frames")
    if m == "cfg":
        if world % 2:
            raise SystemExit("--parallel cfg needs an even number of GPUs")
        return m, 2, 1, world // 2
    if m == "cfg-frames":
        if world % 2 or world < 4:
            raise SystemExit("--parallel cfg-frames needs an even number of GPUs >= 4")
        return m, 2, world // 2, 1
    if m == "frames":
        return m, 1, world, 1
    return "replicas", 1, 1, world


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_self(args))

    import numpy as np
    import torch

    if args.cpu_baseline == "full":   # host-only measurement: ONE oracle step at the bench workload, clocked; no GPU, no extrapolation
        from motioneditor_amd import synth
        usd = synth.synth_state_dict(synth.unet_schema())
        csd = synth.synth_state_dict(synth.controlnet_schema(), salt="controlnet.")
        cdt, cores, cf, ch, cw = cpu_baseline(usd, csd, args.frames, args.latent, args.latent)
        ctf, exact = step_tflop(cf, ch, cw)
        import hashlib
        print(json.dumps({"cpu_baseline_full": {"oracle_sha16": hashlib.sha1((ROOT / "oracle" / "ref_cpu.py").read_bytes()).hexdigest()[:16], "seconds": round(cdt, 1), "steps_per_s": round(1.0 / cdt, 6), "cores": cores, "cpu": cpu_model(), "host": socket.gethostname(),
                                                "threads_available": os.cpu_count(), "workload": f"{cf} frames x {8*ch}x{8*cw} ({ch}x{cw} latents), two-branch + ControlNet + adapter, editors active",
                                                "tflop_reference_semantics": ctf, "tflops": round(ctf / cdt, 3), "kind": "port", "extrapolated": False,
                                                "what": "oracle/ref_cpu.denoise_step (fp32 torch CPU restatement of pipeline_motion_editor.py:603-648), one step, wall clock"}}), flush=True)
        return

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dist_on = world > 1 or (args.parallel == "frames" and not args.emulate)
    if args.emulate:
        device = "cpu"
        torch.set_num_threads(max(1, (os.cpu_count() or 8) // world))
    else:
        torch.cuda.set_device(local)
        device = f"cuda:{local}"
    dist = None
    if dist_on:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(free_port()))
        if args.emulate:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(device))

    def sync():
        if not args.emulate:
            torch.cuda.synchronize()

    from motioneditor_amd import ops, synth
    emu_dtype = None
    if args.emulate:
        import emu_ops
        import motioneditor_amd.models.unet_2d_condition as u_mod
        import motioneditor_amd.pipelines.pipeline_motion_editor as pm_mod
        from motioneditor_amd import schedulers as sch_mod
        from motioneditor_amd.models import graph as graph_mod
        for m in (graph_mod, u_mod, pm_mod, sch_mod):
            m.ops = emu_ops
        emu_dtype = torch.float32
    else:
        from motioneditor_amd import capi
        capi.lib()  # no HIP library -> hard failure (no fallback path exists)

    if args.null_text:
        if dist_on or args.emulate:
            raise SystemExit("--null-text is a single-GPU secondary measurement")
        from motioneditor_amd import util
        from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
        from motioneditor_amd.schedulers import DDIMScheduler
        usd = synth.synth_state_dict(synth.unet_schema())

        class Pipe:
            pass
        pipe = Pipe()
        pipe.unet = UNet2DConditionModel(usd, device)
        sched = DDIMScheduler()
        sched.set_timesteps(50)
        f, h = args.frames, args.latent
        lat = [torch.from_numpy(synth.synth_normal(f"bench.nt{i}", (1, 4, f, h, h), 33)).to(device) for i in range(2)]
        ctx = torch.from_numpy(synth.synth_normal("bench.ntctx", (2, 77, 768), 33, 0.3)).to(device)
        run = lambda k: util.null_optimization(pipe, sched, lat, ctx, k, -1.0, num_ddim_steps=1)   # epsilon < 0: no early stop  # noqa: E731
        if args.warmup:
            run(args.warmup)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        emb_out = run(args.steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, {f"uncond_embeddings{i}": e for i, e in enumerate(emb_out)})
        split = {}
        if args.full:
            # the DDIM step around the inner loop costs a conditional forward before it and a batch-2 forward after it: a second run with twice the inner
            # iterations separates the per-iteration time (slope) from that per-step overhead (intercept)
            t1 = time.perf_counter()
            run(2 * args.steps)
            torch.cuda.synchronize()
            dt2 = time.perf_counter() - t1
            inner = (dt2 - dt) / args.steps
            split = {"inner_iteration_ms": round(inner * 1e3, 1), "ddim_step_overhead_ms": round((dt - inner * args.steps) * 1e3, 1)}
        print(json.dumps({"metric": "null-text inner iterations/sec (UNet forward on a tape + backward + Adam, batch 1; each timed call also runs the 2 plain forwards of its DDIM step)",
                          "value": round(args.steps / dt, 4), "unit": "iterations/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": round(dt / args.steps * 1e3, 1), **split,
                          "higher_is_better": True, "dtype": "f16 (fp32 gradient buffers, loss-scaled fp16 between layers)",
                          "data": "synthetic", "config": {"workload": f"{f} frames x {8*h}x{8*h}, single-branch UNet3D, sparse-causal attn1 (normal_infer=False as the reference hard-codes)",
                                                          "attention_backward": "fused flash-style me_attn_bwd (P rebuilt from the stashed log-sum-exp; key-centric dK / dV + query-centric dQ kernels)",
                                                          "loss_and_optimiser": "device kernels (me_mse_seed, me_sumsq_absmax, me_adamw); two floats read by the host per iteration"}}))
        return

    if args.vae_decode:
        if dist_on or args.emulate:
            raise SystemExit("--vae-decode is a single-GPU secondary measurement")
        from motioneditor_amd.models.vae import AutoencoderKL
        vae = AutoencoderKL.from_synthetic(device)
        z = torch.from_numpy(synth.synth_normal("bench.vae", (args.frames, 4, args.latent, args.latent), 33)).to(device)
        for _ in range(args.warmup):
            vae.decode(z)
        torch.cuda.synchronize()
        ops.PROFILE = [] if args.full else None     # --full: an event pair around every launch of the timed steps (kernel_families)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            img = vae.decode(z).sample
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        prof, ops.PROFILE = ops.PROFILE, None
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, {"images": img})
        fam = {}
        for rec in prof or []:
            d = fam.setdefault(rec[0], [0.0, 0.0])
            d[0] += rec[3].elapsed_time(rec[4]) * 1e-3
            d[1] += rec[1]
        assert torch.isfinite(img).all()
        out = {"metric": "vae-decode frames/sec (SD-1.5 AutoencoderKL decoder)", "value": round(args.frames * args.steps / dt, 3), "unit": "frames/s",
               "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 2), "higher_is_better": True,
               "dtype": "f16", "data": "synthetic", "config": {"workload": f"{args.frames} latent frames {args.latent}x{args.latent} -> {8 * args.latent}x{8 * args.latent} images"}}
        if args.full:
            out["kernel_families"] = {k: {"ms_per_step": round(v[0] / args.steps * 1e3, 2), "tflops": round(v[1] / v[0] / 1e12, 1) if v[0] else 0} for k, v in sorted(fam.items())}
        print(json.dumps(out))
        return

    usd = synth.synth_state_dict(synth.unet_schema())
    csd = synth.synth_state_dict(synth.controlnet_schema(), salt="controlnet.")
    if args.zero_tconv:
        usd = {k: (np.zeros_like(v) if ".temp_conv" in k and not k.startswith("controlnet_adapter.") else v) for k, v in usd.items()}
    f, h, w = args.frames, args.latent, args.latent
    mode, n_cfg, n_shards, n_clips = resolve_mode(args, world)
    if f % n_shards:
        raise SystemExit(f"{f} frames do not split over {n_shards} frame shards")
    # rank layout: rank = (clip * n_shards + shard) * n_cfg + cfg half  (CFG pairs are neighbouring ranks)
    cfg_r = rank % n_cfg
    shard_i = (rank // n_cfg) % n_shards
    clip = rank // (n_cfg * n_shards)
    cfg_group = shard_group = side_group = None
    if dist_on:   # every rank creates every group, in the same order
        if n_cfg == 2:
            for c in range(n_clips):
                for s_ in range(n_shards):
                    ranks = [(c * n_shards + s_) * 2 + k for k in range(2)]
                    g = dist.new_group(ranks)
                    if rank in ranks:
                        cfg_group = g
        if n_shards > 1:
            for c in range(n_clips):
                for k in range(n_cfg):
                    ranks = [(c * n_shards + s_) * n_cfg + k for s_ in range(n_shards)]
                    g = dist.new_group(ranks)
                    g2 = dist.new_group(ranks) if args.shard_overlap else None     # the adapter's own communicator (--shard-overlap)
                    if rank in ranks:
                        shard_group, side_group = g, g2
    if dist_on and args.shard_overlap and mode == "frames" and n_shards == 1:   # the sharded code path on ONE rank: the adapter's second communicator over the default group
        side_group = dist.new_group(list(range(world)))
    shard = None
    comm = "torch" if args.emulate else (args.comm if args.comm != "auto" else ("rccl" if args.graph else "torch"))
    comm_backend = comm     # (`comm` is re-used for the exchange statistics further down)
    if dist_on and comm == "rccl":   # our own communicators (every rank of a group creates it together); the pipeline takes the adapter in place of the group
        from motioneditor_amd import parallel
        if cfg_group is not None:
            cfg_group = parallel.exchange(cfg_group, "rccl")
    if n_shards > 1 or mode == "frames":
        from motioneditor_amd import parallel
        lean = args.shard_exchange == "lean"
        shard = parallel.FrameShard(f, shard_group, temporal="a2a" if lean else "gather", adapter="halo" if lean else "gather", comm=comm,   # f / n_shards frames per rank
                                    side_group=side_group)
        assert shard.rank == shard_i
    x = build_inputs(f, h, w, seed=33 + clip)   # one clip per rank (replicas), per GPU pair (cfg), or for all ranks
    pipe, sed, ted = make_pipeline(device, usd, csd, x["masks"], emu_dtype)
    pipe.overlap_controlnet = pipe.overlap_adapter = not (args.no_overlap or args.emulate)
    pipe.dedup_cfg_prefix = not args.no_cfg_prefix_sharing
    pipe.shard_overlap = bool(args.shard_overlap and not args.emulate)
    images = torch.cat([x["skeleton"]] * 2).reshape(2 * f, 3, 8 * h, 8 * w).to(device)
    lat = x["latents"].to(device)
    if shard is not None:   # this rank's frames only
        lo, hi = shard.frame0, shard.frame0 + shard.f_loc
        images = images[lo:hi].contiguous()
        lat = lat[:, :, lo:hi].contiguous()
    cond = x["cond"].to(device)
    unc = [u.to(device) for u in x["uncond"]]
    ts = pipe.scheduler.timesteps

    if args.inversion:
        from motioneditor_amd import util
        pipe.unet.spatial_editor = pipe.unet.temporal_editor = None
        lat = lat[:1].contiguous()
    if args.single_branch:   # BASELINE configs[1]: one clip, UNet3D only
        if dist_on or args.inversion:
            raise SystemExit("--single-branch is a single-GPU measurement of the plain UNet3D step")
        pipe.unet.spatial_editor = pipe.unet.temporal_editor = None
        pipe.controlnet = None
        lat = lat[:1].contiguous()

    use_graph = args.graph and not (args.emulate or args.inversion)
    single_process = not dist_on and shard is None and n_cfg == 1
    if args.plan and not single_process:
        raise SystemExit("--plan covers the single-process steps (the sharded steps' RCCL exchanges are not library launches); use --graph there")
    plan_default = single_process and f * h * w <= 24 * 64 * 64 and not args.eager
    use_plan = (args.plan or plan_default) and not (args.emulate or args.inversion or use_graph or args.null_text or args.vae_decode)
    plan_state = {"on": bool(use_plan), "error": None}

    def run_step(i, lat):
        if args.inversion:   # one body of util.ddim_loop (reference util.py:118-123)
            return util.ddim_loop(pipe, pipe.scheduler, lat, 1, normal_infer=True, text_embeddings=cond[:1])[-1]
        i = timestep_index(i, i0, len(ts))
        if args.editors == "inactive":
            sed.cur_step = ted.cur_step = 0      # the editors count steps themselves: hold them before start_step
        else:
            sed.cur_step = ted.cur_step = i      # what they count to by themselves, up to the last timestep; then round again with i
        if args.single_branch:
            emb1 = torch.cat([unc[i], cond[:1]])
            if use_graph and ops.PROFILE is None:
                return pipe.denoise_step_graphed(lat, ts[i], emb1, None, 7.5)
            if plan_state["on"] and ops.PROFILE is None:
                return planned_or_eager(pipe, plan_state, lat, ts[i], emb1, None)
            return pipe.denoise_step(lat, ts[i], emb1, None, 7.5)
        emb = torch.cat([unc[i].expand(2, 77, 768), cond])
        graphed = use_graph and ops.PROFILE is None
        if shard is not None:
            if graphed:
                return pipe.denoise_step_graphed(lat, ts[i], emb, images, 7.5, shard=shard, cfg_group=cfg_group)
            return pipe.denoise_step_frame_sharded(lat, ts[i], emb, images, 7.5, shard, cfg_group=cfg_group)
        if n_cfg == 2:
            if graphed:
                return pipe.denoise_step_graphed(lat, ts[i], emb, images, 7.5, cfg_parallel_group=cfg_group)
            return pipe.denoise_step_cfg_parallel(lat, ts[i], emb, images, 7.5, group=cfg_group)
        if graphed:
            return pipe.denoise_step_graphed(lat, ts[i], emb, images, 7.5)
        if plan_state["on"] and ops.PROFILE is None:
            return planned_or_eager(pipe, plan_state, lat, ts[i], emb, images)
        return pipe.denoise_step(lat, ts[i], emb, images, 7.5)

    sed.cur_step = ted.cur_step = 4 if args.editors == "active" else 0   # active: the steady-state step (46 of 50)
    i0 = 4
    pipe.side_stream_priority = args.side_priority
    if args.main_priority != 0 and not args.emulate:
        sync()
        torch.cuda.set_stream(torch.cuda.Stream(priority=args.main_priority))
    for k in range(args.warmup):
        lat = run_step(i0 + k, lat)
    sync()
    if dist_on:
        dist.barrier()
        from motioneditor_amd import parallel
        parallel.reset_stats()
    sync()
    t0 = time.perf_counter()
    host_dt = None
    for k in range(args.steps):
        lat = run_step(i0 + args.warmup + k, lat)
        if k == 0:   # the host's share: time to ENQUEUE one step into an empty queue (later steps block on the launch queue's depth)
            host_dt = time.perf_counter() - t0
    sync()
    if dist_on:
        dist.barrier()
    sync()
    dt = time.perf_counter() - t0
    if args.dump_outputs:   # the updated latents the last timed step returned (this rank's frames when the clip is sharded)
        dump_outputs(args.dump_outputs, {"latents": lat}, rank, world)
    comm = None
    if dist_on:
        from motioneditor_amd import parallel
        comm = parallel.stats_summary(args.steps)
        if args.full and not use_graph and args.steps + args.warmup + i0 + 2 <= len(ts):
            # which exchanges hold the step's stream, and for how long: TWO more steps, untimed, with an event pair (CUDA) / clock pair (CPU tensors) around
            # every blocking exchange and every join of an asynchronous one (parallel.TIMING).  Kept out of the timed region (~400 event records per step);
            # every rank runs them (they contain the same collectives).  Not under --graph: events cannot be timed inside a captured step.
            parallel.reset_stats()
            parallel.TIMING = True
            try:
                for k in range(2):
                    lat = run_step(i0 + args.warmup + args.steps + k, lat)
                sync()
                dist.barrier()
                held = parallel.stats_summary(2)
            finally:
                parallel.TIMING = False
            for k, v in held.items():
                if "stream_held_ms_per_step" in v:
                    comm.setdefault(k, {})["stream_held_ms_per_step"] = v["stream_held_ms_per_step"]
            comm["stream_held_note"] = ("stream_held_ms_per_step: time this rank's stream spent inside exchanges of that kind (waiting for the peers + the transfer), from an event pair "
                                        "around every blocking exchange / join, measured on two extra untimed steps after the timed region; 'join <kind>' = the join of an exchange "
                                        "posted earlier (what was NOT hidden behind the launches in between)")
    # Roofline pass: the SAME steps once more, eagerly, with a HIP event pair around every launch and on a single stream.
    # It is not folded into the timed region because (a) ~1100 event pairs per step cost ~6 % of the step and (b) the timed
    # region overlaps two streams (ControlNet + adapter beside the UNet),
    # which stretches every kernel's own duration by whatever shares the GPU with it.
    prof = None
    plan_stats = None
    for st in pipe._plans.values():
        plan_stats = st["plan"].stats()
    if args.full and not args.no_profile and not args.emulate:
        ov = (pipe.overlap_controlnet, pipe.overlap_adapter)
        for st in pipe._plans.values():      # the recorded step's private pool goes back to the allocator before the eager pass needs the memory
            plan_stats = st["plan"].stats()
        pipe.release_plans()
        pipe.overlap_controlnet = pipe.overlap_adapter = False
        if rank == 0:
            ops.PROFILE = []
        lat2 = lat
        for k in range(args.steps):
            lat2 = run_step(i0 + args.warmup + k, lat2)
        sync()
        prof, ops.PROFILE = ops.PROFILE, None
        pipe.overlap_controlnet, pipe.overlap_adapter = ov
    if dist_on:
        tt = torch.tensor([dt], device=device, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    assert torch.isfinite(lat).all(), "non-finite latents"

    if rank == 0:
        ms = dt / args.steps * 1e3
        value = n_clips * args.steps / dt
        tf_ref, tf_exact = step_tflop(f, h, w)
        if args.single_branch or args.inversion:   # the two-branch figure does not apply: report executed FLOPs only (below)
            tf_ref, tf_exact = 0.0, False
        xch = ("frame<->pixel all-to-all for temporal attention (RCCL), <= 2 halo frames of K|V for the adapter's sparse-causal attention (p2p)"
               if args.shard_exchange == "lean" else "RCCL all-gather of K|V (adapter sparse-causal + temporal attention)")
        desc = {"single": "single GPU",
                "cfg": f"cfg2 x dp{n_clips}: each GPU pair splits one clip along the classifier-free-guidance axis (one RCCL all-gather of the noise prediction per step)"
                       + (f", {n_clips} clips side by side" if n_clips > 1 else ""),
                "cfg-frames": f"cfg2 x frames{n_shards}: one clip; GPU pairs split the CFG axis, {f // max(n_shards, 1)} frames per GPU; per layer: attn1 one-frame K|V halo (p2p), "
                              f"{xch}, TemporalConv halos, GroupNorm-statistic all-reduce, all at batch 2",
                "frames": f"frames{n_shards}: one clip, {f // max(n_shards, 1)} frames per GPU; per layer: attn1 one-frame K|V halo (p2p), {xch}, "
                          f"TemporalConv halos, GroupNorm-statistic all-reduce",
                "replicas": f"dp{world}: one independent clip per GPU, no data-path collective"}[mode]
        out = {"metric": ("ddim-inversion steps/sec (single-branch UNet3D, normal_infer)" if args.inversion else
                          f"denoise-steps/sec, {f}f x {8 * h}^2 single-branch UNet3D (BASELINE configs[1])" if args.single_branch else
                          f"denoise-steps/sec, {f}f x {8 * h}^2 two-branch UNet3D+ControlNet(+adapter+K/V injection)"), "value": round(value, 4),
               "unit": "steps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 2),
               "higher_is_better": True, "scaling": "weak" if n_clips > 1 else "strong", "vs_baseline": None,
               "dtype": "f32 (CPU emulation of the C ABI: plumbing test, not a measurement)" if args.emulate else "f16", "data": "synthetic",
               "config": {"workload": (f"BASELINE configs[1]: case-1 shape, {f} frames x {8*h}x{8*w}, ONE clip, single-branch UNet3D only (classifier-free-guidance pair = batch 2), "
                                       f"1 DDIM step = 1 unit; seeded random SD-1.5-architecture weights" if args.single_branch else
                                       f"BASELINE configs[2]: case-1 shape, {f} frames x {8*h}x{8*w}, two-branch + ControlNet + adapter + K/V injection "
                                       f"(editors {args.editors}), 1 DDIM step = 1 unit; seeded random SD-1.5-architecture weights"),
                          "frames": f, "latent_hw": [h, w], "batch": 2 if args.single_branch else 4, "guidance": 7.5, "editors": args.editors, "zero_temporal_conv": bool(args.zero_tconv),
                          "controlnet_dedup": bool(pipe.dedup_controlnet and f % 2 == 0),
                          "cfg_prefix_shared": bool(pipe.dedup_cfg_prefix and n_cfg == 1), "shard_overlap": bool(pipe.shard_overlap and shard is not None),
                          "layernorm_folded": bool(getattr(__import__("motioneditor_amd.models.graph", fromlist=["LN_FOLD"]), "LN_FOLD", False)), "controlnet_side_stream": bool(pipe.overlap_controlnet and world == 1),
                          "step_invariant_reuse": "ControlNet conditioning embedding of the (unchanged) skeleton computed at the first step and kept (exact); "
                                                  "text K|V of all transformer blocks projected by one GEMM per model",
                          "hip_graph_replay": bool(use_graph), "launch_plan_replay": bool(plan_state["on"]), "launch_plan_error": plan_state["error"], "main_stream_priority": args.main_priority, "side_stream_priority": args.side_priority, "exchange_backend": comm_backend if dist_on else None, "parallel_mode": mode, "shard_exchange": args.shard_exchange if n_shards > 1 else None, "parallelism": desc,
                          "oracle_pins": "UNet3D / adapter / editors / DDIM pinned by reference-generated goldens; ControlNet (diffusers, source not in the reference tree): TRUNK pinned "
                                         "against the reference's own 2-D-degenerate SD-1.5 blocks (tests/golden/controlnet_trunk.npz), its 8 conditioning-embedding convolutions and "
                                         "13 1x1 zero-convolutions self-pinned"},
               "step_tflop_reference_semantics": round(tf_ref, 2) if tf_ref else None, "step_tflop_is_baseline_md_figure": tf_exact,
               "achieved_tflops_reference_semantics": round(tf_ref * n_clips * args.steps / dt, 1) if tf_ref else None}
        if plan_stats is not None:   # the recorded step behind me_denoise_step: launches, cross-stream event records / waits, argument bytes, replays so far
            out["launch_plan"] = plan_stats
        out["host_enqueue_ms_per_step"] = round(host_dt * 1e3, 2)   # < ms_per_step: the GPU, not the Python launch loop, is the limit
        if comm is not None:
            out["comm"] = comm
        if prof:
            fam, kern, shapes = {}, {}, {}
            for name, fl, by, e0, e1, detail, kname, xfl in prof:
                sec = e0.elapsed_time(e1) * 1e-3
                for table, key in ((fam, name), (kern, kname)):
                    d = table.setdefault(key, [0.0, 0.0, 0.0, 0, 0.0])
                    d[0] += sec
                    d[1] += fl
                    d[2] += by
                    d[3] += 1
                    d[4] += xfl
                if detail:
                    sd = shapes.setdefault(detail + " " + kname, [0.0, 0.0, 0])
                    sd[0] += sec
                    sd[1] += fl
                    sd[2] += 1
            if args.shapes:
                for k, v in sorted(shapes.items(), key=lambda kv: -kv[1][0])[:160]:
                    print(f"[shape] {k:64s} {v[0] / args.steps * 1e3:8.2f} ms/step {v[2] // args.steps:4d} launches {v[1] / v[0] / 1e12:7.1f} TF/s", file=sys.stderr)
            tot = sum(v[0] for v in fam.values())
            exec_tf = sum(v[4] for v in fam.values()) / args.steps / 1e12
            out["executed_tflop_per_step"] = round(exec_tf, 2)
            out["achieved_tflops_executed"] = round(exec_tf * n_clips * args.steps / dt, 1)
            out["mfma_frac_reference_semantics"] = round(tf_ref * n_clips * args.steps / dt / PEAK_MFMA_TFLOPS / world, 4) if tf_ref else None
            out["mfma_frac_executed"] = round(exec_tf * n_clips * args.steps / dt / PEAK_MFMA_TFLOPS / world, 4)
            dom = max(kern, key=lambda k: kern[k][0])
            tsec, fl, by, n, xfl = kern[dom]
            # HBM bytes per launch of the dominant kernel: NOT measured in this run -- PMC counters need their own rocprofv3 --pmc passes
            # (tools/collect_profiles.sh -> tools/pmc_summary.py -> profiles/pmc_traffic.json, same workload).  The file names the kernels it was
            # collected for; if the dominant kernel of THIS run is not among them (the kernel set changed since), no figure is reported.
            traffic, traffic_src = None, None
            pmc = ROOT / "profiles" / "pmc_traffic.json"
            if pmc.exists() and (f, h, w) == (24, 64, 64) and world == 1:
                pt = json.loads(pmc.read_text())
                ent = pt.get(dom)
                if ent is not None and all(k in pt for k in list(sorted(kern, key=lambda k: -kern[k][0]))[:3] if not k.startswith(("groupnorm", "layernorm"))):
                    traffic = ent.get("hbm_bytes_per_launch")
                    traffic_src = "profiles/pmc_traffic.json: separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this workload (2 x FETCH_SIZE + WRITE_SIZE, gfx950 correction), not this run"
                else:
                    traffic_src = "profiles/pmc_traffic.json does not cover this run's dominant kernels (kernel set changed since it was collected): not reported"
            PEAK_HBM_GBS = 8000.0                      # MI355X_MICROARCH.md: 8 TB/s HBM3E (spec; a copy kernel measures ~6.3)
            ridge = PEAK_MFMA_TFLOPS * 1e12 / (PEAK_HBM_GBS * 1e9)    # flop per algorithmic HBM byte at which the two roofs meet (312)

            def roofs(fl_, by_, sec_):
                """which roof bounds a kernel, from its ALGORITHMIC intensity (launch-weighted over its launches), and the fraction of each roof it reaches"""
                inten = fl_ / by_ if by_ else float("inf")
                return {"intensity_flop_per_byte": round(inten, 1) if by_ else None, "bound": "mfma" if inten >= ridge else "hbm",
                        "frac_mfma": round(fl_ / sec_ / 1e12 / PEAK_MFMA_TFLOPS, 4) if sec_ else 0, "frac_hbm": round(by_ / sec_ / 1e9 / PEAK_HBM_GBS, 4) if sec_ else 0}
            rf = roofs(fl, by, tsec)
            out["roofline"] = {"kernel": dom, "bound": rf["bound"], "intensity_flop_per_byte": rf["intensity_flop_per_byte"], "ridge_flop_per_byte": round(ridge, 1),
                               "frac_hbm": rf["frac_hbm"], "achieved": round(fl / tsec / 1e12, 1), "peak": PEAK_MFMA_TFLOPS, "unit": "TFLOP/s",
                               "frac": round(fl / tsec / 1e12 / PEAK_MFMA_TFLOPS, 4), "traffic": None if traffic is None else round(traffic), "traffic_source": traffic_src,
                               "achieved_executed": round(xfl / tsec / 1e12, 1), "frac_executed": round(xfl / tsec / 1e12 / PEAK_MFMA_TFLOPS, 4),
                               "flops_counted": "achieved = reference-semantics FLOPs of the launches (SURVEY 8d: a binary dual segment counts its 2 nk materialised keys); "
                                                "achieved_executed = FLOPs the kernel multiplies (without MFMA tile padding)",
                               "algorithmic_bytes_per_launch": round(by / n), "launches_per_step": n // args.steps, "avg_launch_ms": round(tsec / n * 1e3, 4),
                               "share_of_gpu_time": round(tsec / tot, 3),
                               "measured_in": "event-instrumented single-stream eager pass of the same steps inside this run, right after the timed region "
                                              "(the timed region is un-instrumented and overlaps two streams)"}
            # per kernel / family: BOTH roofs (round-5 verdict: the K <= 640 GEMM launches sit between them, GroupNorm / LayerNorm / temporal attention are HBM kernels)
            out["kernels"] = {k: dict({"ms_per_step": round(v[0] / args.steps * 1e3, 2), "tflops": round(v[1] / v[0] / 1e12, 1) if v[0] else 0,
                                       "tflops_executed": round(v[4] / v[0] / 1e12, 1) if v[0] else 0, "gbs": round(v[2] / v[0] / 1e9, 1) if v[0] else 0,
                                       "launches_per_step": v[3] // args.steps}, **roofs(v[1], v[2], v[0]))
                              for k, v in sorted(kern.items(), key=lambda kv: -kv[1][0])[:8]}
            out["kernel_families"] = {k: dict({"ms_per_step": round(v[0] / args.steps * 1e3, 2), "tflops": round(v[1] / v[0] / 1e12, 1) if v[0] else 0,
                                               "gbs": round(v[2] / v[0] / 1e9, 1) if v[0] else 0, "launches_per_step": v[3] // args.steps}, **roofs(v[1], v[2], v[0]))
                                      for k, v in sorted(fam.items())}
        if args.full and world == 1 and not args.no_cpu_baseline and args.cpu_baseline != "off" and not args.emulate and not (args.single_branch or args.inversion):
            cdt, cores, cf, ch, cw = cpu_baseline(usd, csd)
            ctf, _ = step_tflop(cf, ch, cw)
            scale = tf_ref / ctf
            cb = {"value": round(1.0 / (cdt * scale), 6), "unit": "steps/s", "cores": cores, "kind": "port", "cpu": cpu_model(), "extrapolated": True,
                  "sample": f"oracle/ref_cpu.py (fp32 torch CPU restatement of the reference step) timed on ONE full two-branch step, editors active, at BASELINE "
                            f"configs[0] = {cf} frames x {8*ch}x{8*cw} ({ch}x{cw} latents, {ctf} TFLOP): {cdt:.1f} s on {cores} threads = {ctf / cdt:.2f} TFLOP/s; "
                            f"scaled to the bench workload by the reference-semantics FLOP ratio x{scale:.1f}",
                  "sample_seconds": round(cdt, 2), "sample_steps_per_s": round(1.0 / cdt, 5), "sample_extrapolated_steps_per_s": round(1.0 / (cdt * scale), 6)}
            # `value` is ALWAYS what this run measured (the bounded sample, scaled by the FLOP ratio).  The bench workload itself clocked once on a GPU box's
            # host cores (python bench.py --cpu-baseline full, committed under profiles/) is reported NEXT to it, never in its place (round-4 advisor finding:
            # a file from another host / day must not silently become the headline CPU number), with the hash of the oracle it was taken with.
            full = ROOT / "profiles" / "cpu_baseline_full.json"
            if full.exists():
                fj = json.loads(full.read_text()).get("cpu_baseline_full", {})
                if fj.get("workload", "").startswith(f"{f} frames x {8*h}x{8*w} "):
                    import hashlib
                    now = hashlib.sha1((ROOT / "oracle" / "ref_cpu.py").read_bytes()).hexdigest()[:16]
                    cb["full_config_measurement"] = dict(fj, source="profiles/cpu_baseline_full.json: one oracle step at this very workload clocked on a GPU box's host cores "
                                                                    "(NOT in this run)", oracle_sha16_now=now,
                                                         oracle_unchanged=(fj.get("oracle_sha16") == now) if fj.get("oracle_sha16") else None)
            out["cpu_baseline"] = cb
        print(json.dumps(out), flush=True)
    if dist_on:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
