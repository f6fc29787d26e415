"""Stage 1 of the reference workflow (train_bg.py): background tuning of the UNet's attn1.to_q, attn2.to_q and attn_temp on the source clip, with
synthetic tensors in place of the dataset, CLIP and the SD-1.5 checkpoint (none exist offline):

    pixel_values [1, f, 3, H, W] --vae.encode(...).latent_dist.sample() * 0.18215--> latents [1, 4, f, h, w]     (:323-330)
    noise ~ N(0, 1); t ~ U{0..999}; noisy = sqrt(a_t) latents + sqrt(1 - a_t) noise  (DDPMScheduler.add_noise)   (:332-337)
    model_pred = unet(noisy, t, ehs).sample; loss = mse(model_pred, noise); backward; clip_grad_norm_(1.0); AdamW  (:346-353)

and the tuned UNet written as checkpoint-<steps>/model.safetensors -- what train_adaptor.py (one_stage_checkpoint) and inference.py
(resume_from_checkpoint) read.

    python examples/train_bg.py [--frames 8 --size 512 --steps 3 --lr 3e-5 --out runs/bg] [--prompt "a girl is dancing" [--checkpoint SD15_DIR]]
--trainable-modules M [M ...]: train_bg.py's `trainable_modules` (module-path suffixes; default attn1.to_q attn2.to_q attn_temp).  Beside the dense
transformer-block projections the tuner takes the 3x3 convolutions of the residual blocks and the down- / upsamplers, conv_shortcut, proj_in / proj_out and
the GroupNorm affine parameters, e.g. `--trainable-modules attn1.to_q attn2.to_q attn_temp .conv1 .conv2 resnets.0.norm1` (a bare `conv1` would also match
temp_conv1, which -- like time_emb_proj, the time embedding, conv_in / conv_out and the LayerNorms -- is refused by name).
--prompt: `encoder_hidden_states = text_encoder(prompt_ids)[0]` (:333) with the native CLIP classes instead of a synthetic embedding.
--video-dir DIR [--mask-dir man.mask --condition openposefull --suffix .png]: pixel_values come from data.dataset.VideoDataset (train_bg.py:323) instead of
synthetic tensors; --frames and --size are its n_sample_frames and width / height.
Across GPUs: run under torchrun; util.UNetTuner averages the gradients over the ranks in one all-reduced bucket.
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "examples"))

from run_edit import add_clip_arguments  # noqa: E402
from train_adapter import alphas_cumprod, clip_training_batch, encode_prompt, training_batch  # noqa: E402


def step(tuner, vae, batch: dict, t: int) -> float:
    """train_bg.py:323-353 for one clip."""
    pv = batch["pixel_values"]
    f, H, W = pv.shape[1], pv.shape[3], pv.shape[4]
    h, w = H // 8, W // 8
    lat = vae.encode(pv.reshape(f, 3, H, W)).latent_dist.sample(noise=batch["encode_noise"])                    # (:326)
    lat = lat.reshape(1, f, 4, h, w).permute(0, 2, 1, 3, 4).contiguous().float().cpu() * 0.18215                  # (:328-330)
    a = float(alphas_cumprod()[t])
    noise = batch["noise"]
    noisy = a ** 0.5 * lat + (1.0 - a) ** 0.5 * noise                                                             # (:337)
    return tuner.step(noisy, t, batch["ehs"], noise)                                                              # (:346-353)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--lr", type=float, default=3e-5)
    ap.add_argument("--out", default="runs/bg")
    ap.add_argument("--prompt", default=None, help="encode this prompt with the native CLIP text encoder instead of a synthetic embedding")
    ap.add_argument("--checkpoint", default=None, help="SD-1.5 directory whose text_encoder/ and tokenizer/ serve --prompt (default: synthetic weights and vocabulary)")
    ap.add_argument("--trainable-modules", nargs="+", default=["attn1.to_q", "attn2.to_q", "attn_temp"], metavar="M",
                    help="train_bg.py's trainable_modules: every parameter under a module whose path ends with one of these is trained")
    ap.add_argument("--gradient-checkpointing", action="store_true",
                    help="unet.enable_gradient_checkpointing(), the reference's default: keep block boundaries only, recompute the blocks in the backward (long clips)")
    add_clip_arguments(ap)
    args = ap.parse_args()
    from motioneditor_amd import util
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    from motioneditor_amd.models.vae import AutoencoderKL
    dev = "cuda"
    vae, unet = AutoencoderKL.from_synthetic(dev), UNet2DConditionModel.from_synthetic(dev)
    if args.gradient_checkpointing:
        unet.enable_gradient_checkpointing()                                                                       # (train_bg.py:182-183)
    tuner = util.UNetTuner(unet, trainable_modules=tuple(args.trainable_modules), lr=args.lr)
    print(f"training {len(tuner.names)} parameters ({tuner.master.numel() / 1e6:.1f} M values); {len(tuner.unreached)} selected parameters of the "
          "adapter are not reached by this forward and stay frozen")
    ehs = encode_prompt(args.prompt, args.checkpoint, dev) if args.prompt is not None else None
    g = torch.Generator().manual_seed(0)
    for i in range(args.steps):
        t = int(torch.randint(0, 1000, (1,), generator=g))                                                         # (:334)
        batch = training_batch(args.frames, args.size, args.size, seed=7 + i)
        if ehs is not None:
            batch["ehs"] = ehs
        if args.video_dir:
            batch = clip_training_batch(args, batch)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = step(tuner, vae, batch, t)
        torch.cuda.synchronize()
        print(f"step {i}: t = {t}, loss = {loss:.5f}   ({(time.perf_counter() - t0) * 1e3:.0f} ms/step: VAE encode, UNet forward / backward, clip, AdamW, "
              "weight refresh)", flush=True)
    out = Path(args.out) / f"checkpoint-{args.steps}"
    print("saved", tuner.save_checkpoint(out))


if __name__ == "__main__":
    main()
