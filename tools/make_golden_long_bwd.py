"""Generate tests/golden/long_bwd_f72.npz: what oracle.ref_cpu leaves under torch autograd at 72 frames on 8 x 8 latents, for tests/test_long_bwd_gpu.py.

Test infrastructure, not product code.  Two computations on the synthetic UNet weights, each on seeded inputs the test rebuilds itself
(tests/bwd_run.training_clip(0, f=72, h=8); tests/long_bwd_cases.null_text_inputs):
  * one adapter training step's loss and gradients (train_adaptor.py:364-368 as tests/golden/adapter_train.npz holds them at 8 frames): the norm of every
    controlnet_adapter parameter's gradient and the two tensors of long_bwd_cases.ADAPTER_FULL in full;
  * the first gradient of the null-text optimisation (ref_cpu.null_optimization's grads= hook; one DDIM step, one inner step).
Both take tens of seconds on a CPU at 72 frames, which is why the GPU tests read them from a fixture.

Usage:  python tools/make_golden_long_bwd.py
"""
from __future__ import annotations

import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import bwd_run as br  # noqa: E402
import long_bwd_cases as lb  # noqa: E402
from motioneditor_amd import synth  # noqa: E402
from oracle import ref_cpu  # noqa: E402


def main() -> None:
    sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(synth.unet_schema()).items()}
    f = lb.MODEL_FRAMES
    t0 = time.time()
    c = br.training_clip(0, f=f, h=8)
    names = [k for k in sd if k.startswith("controlnet_adapter.")]
    sd2 = dict(sd)
    for k in names:
        sd2[k] = sd[k].clone().requires_grad_(True)
    loss = torch.nn.functional.mse_loss(ref_cpu.unet_forward(sd2, c["noisy"], c["t"], c["ehs"], c["down"], c["mid"]), c["noise"])
    grads = dict(zip(names, torch.autograd.grad(loss, [sd2[k] for k in names])))
    print(f"adapter training at {f} frames: loss {float(loss):.6f}, {len(names)} parameters, {time.time() - t0:.1f} s")
    t0 = time.time()
    latents, context = lb.null_text_inputs(f)
    g0 = []
    ref_cpu.null_optimization(sd, ref_cpu.DDIM(), latents, context, 1, 1e-5, num_steps=1, grads=g0)
    print(f"null-text first gradient at {f} frames: norm {float(g0[0].norm()):.4e}, {time.time() - t0:.1f} s")
    out = ROOT / "tests" / "golden" / lb.GOLDEN
    np.savez_compressed(out, frames=f, adapter_loss=float(loss.detach()), adapter_names=np.array(names),
                        adapter_grad_norms=np.array([float(grads[k].norm()) for k in names], dtype=np.float64),
                        **{f"adapter_full_{i}": grads[k].numpy() for i, k in enumerate(lb.ADAPTER_FULL)}, adapter_full_names=np.array(lb.ADAPTER_FULL),
                        null_grad0=g0[0].numpy())
    print(out, out.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
