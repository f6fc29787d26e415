"""The reference harness sequence (inference.py:255-323) on motioneditor_amd, with synthetic tensors in place of the dataset,
CLIP and the checkpoints (none exist offline) unless a clip folder is given (--video-dir):

    pixels [1, f, 3, H, W]  --vae.encode(...).latent_dist.sample() * 0.18215-->  latents [1, 4, f, h, w]      (:260-265)
    ddim_inversion(pipeline, scheduler, latents, num_inv_steps, prompt="", normal_infer=True)[-1]               (:288-293)
    ddim_inv_latent.repeat(2, 1, 1, 1, 1)                                                                       (:296)
    prompts = [source prompt, target prompt]; skeleton = cat([0, target, 0, target])                            (:298-302)
    TemporalSelfAttentionControl(4, 10) + FullySelfAttentionControlMask(4, 10, source_masks=...) registered     (:307-313)
    pipeline(prompts, generator, latents=ddim_inv_latent, uncond_embeddings=None, skeleton=skeleton, ...)       (:315-323)
    sample_inv, sample_gen = sample.chunk(2)                                                                    (:326)

    python examples/run_edit.py [--frames 8 --size 128 --steps 10 --inv-steps 10]      (defaults finish in seconds on one MI355X)
    python examples/run_edit.py --frames 24 --size 512 --steps 50 --inv-steps 50        (the reference's case-1 geometry)
Without a text encoder the prompt embeddings enter as tensors (`text_embeddings`, `negative_text_embeddings`).
    python examples/run_edit.py --prompt "a girl is dancing" --target-prompt "a boy is dancing" [--checkpoint SD15_DIR]
encodes the prompts with the native CLIP classes instead (models.clip.CLIPTextModel, tokenizer.CLIPTokenizer): `text_encoder/` and `tokenizer/` of
the checkpoint directory, or seeded synthetic weights and a byte-level vocabulary when none is given.
    python examples/run_edit.py --video-dir data/case-1 --mask-dir man.mask [--condition openposefull --suffix .png] --out outputs/case-1
reads the clip with data.dataset.VideoDataset (images/, man.mask/, source_condition/openposefull/, target_condition/openposefull/; --frames and --size are
its n_sample_frames and width / height) and saves the edit and the reconstruction as sample/{target prompt}.gif and sample/{target prompt}-inv.gif under
--out (inference.py:328-329).
    python examples/run_edit.py --prompt "a girl is dancing" --target-prompt "a boy is dancing" --target-prompt "a robot is dancing" --out outputs/case-1
edits the clip towards every --target-prompt (up to 3) in ONE call -- the reference loops over its prompts, one whole run each (inference.py:298-323); here
the reconstruction branch is computed once per step and shared -- and saves sample/{target}.gif per target plus one -inv.gif.
    python examples/run_edit.py --prompt "a girl is dancing" --target-prompt "a boy is dancing" --attention-maps girl --out outputs/case-1
additionally collects the head-mean text cross-attention of the 16 x 16-token layers over the denoising steps (MutualAttentionBase.collect_cross_attention;
the reference's cross_attns / aggregate_cross_attn_map, fully_control.py:257-277) and saves where the word's tokens look: sample/attn-girl-inv.gif (the
reconstruction's conditional rows, tokens of the word in the source prompt) and sample/attn-girl.gif (the edits' conditional rows, tokens of the word in each
target prompt).  --attention-map-tokens 1,2 names token positions instead of a word and works with the synthetic embeddings as well.
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def harness_inputs(f: int, H: int, W: int, seed: int = 33) -> dict:
    """Synthetic stand-ins for one batch of the reference's dataset (data/dataset.py): seeded, layout and value ranges as
    inference.py consumes them."""
    from motioneditor_amd import synth
    T = torch.from_numpy
    return dict(pixel_values=T(np.tanh(synth.synth_normal("harness.pixels", (1, f, 3, H, W), seed)).astype(np.float32)),             # [-1, 1]
                target_skeleton=T(np.clip(synth.synth_normal("harness.skel", (1, f, 3, H, W), seed, 0.5) + 0.5, 0, 1).astype(np.float32)),  # openposefull / 255
                source_masks=T(synth.synth_masks(f, H, W)),                                                                              # [1, f, 1, H, W] in {0, 1}
                text_embeddings=T(synth.synth_normal("harness.cond", (2, 77, 768), seed, 0.3)),        # CLIP(source prompt), CLIP(target prompt)
                negative_text_embeddings=T(synth.synth_normal("harness.uncond", (1, 77, 768), seed, 0.3)),  # CLIP("")
                encode_noise=T(synth.synth_normal("harness.vae_noise", (f, 4, H // 8, W // 8), seed)))


def add_clip_arguments(ap: argparse.ArgumentParser) -> None:
    """The flags that replace the synthetic clip by a folder on disk (shared by the three examples)."""
    ap.add_argument("--video-dir", default=None, help="clip folder in the reference's data/case-N layout: images/, source_condition/<condition>/, target_condition/<condition>/, "
                                                      "optionally <mask dir>/ and frame_list.txt (default: synthetic tensors)")
    ap.add_argument("--mask-dir", default=None, help="folder of 0 / 255 foreground masks (.png) inside --video-dir, e.g. man.mask (default: all-ones masks)")
    ap.add_argument("--condition", default="openposefull", help="condition folder name under source_condition/ and target_condition/")
    ap.add_argument("--suffix", default=".png", help="file suffix of the frames in images/")


def clip_batch(video_dir: str, f: int, H: int, W: int, *, prompt: str = "", mask_dir=None, condition: str = "openposefull", suffix: str = ".png",
               device: str = "cuda") -> dict:
    """One batch of VideoDataset as a DataLoader of batch size 1 delivers it (inference.py:249): every tensor with a leading 1."""
    from motioneditor_amd.data.dataset import VideoDataset
    ds = VideoDataset(video_dir, prompt, width=W, height=H, n_sample_frames=f, condition=[condition], video_suffix=suffix, source_mask_dir=mask_dir, device=device)
    ex = ds[0]
    lead = lambda t: t[None]   # noqa: E731
    return dict(pixel_values=lead(ex["pixel_values"]), source_masks=lead(ex["source_masks"]), sample_indices=lead(ex["sample_indices"]),
                source_conditions={k: lead(v) for k, v in ex["source_conditions"].items()}, target_conditions={k: lead(v) for k, v in ex["target_conditions"].items()},
                prompt=[ex["prompt"]])


def clip_inputs(a, device: str = "cuda") -> dict:
    """harness_inputs with the clip of --video-dir in place of the synthetic pixels, target skeleton and masks (inference.py:254, 268, 270); the
    embeddings and the VAE noise stay the seeded ones."""
    x = {k: v.to(device) for k, v in harness_inputs(a.frames, a.size, a.size).items()}
    b = clip_batch(a.video_dir, a.frames, a.size, a.size, prompt=a.prompt or "", mask_dir=a.mask_dir, condition=a.condition, suffix=a.suffix, device=device)
    x.update(pixel_values=b["pixel_values"], target_skeleton=b["target_conditions"][a.condition], source_masks=b["source_masks"])
    return x


def save_samples(out_dir: str, target_prompt, sample_inv, sample_gen) -> list:
    """inference.py:328-329.  target_prompt: a string, or the list of target prompts of a several-target run (sample_gen then holds one edit per
    target): sample/{target}.gif for each, and the one reconstruction as sample/{first target}-inv.gif."""
    from motioneditor_amd import util
    targets = [target_prompt] if isinstance(target_prompt, str) else list(target_prompt)
    if len(targets) != sample_gen.shape[0]:
        raise ValueError(f"{len(targets)} target prompts for {sample_gen.shape[0]} edits")
    paths = [f"{out_dir}/sample/{t}.gif" for t in targets] + [f"{out_dir}/sample/{targets[0]}-inv.gif"]
    for k, path in enumerate(paths[:-1]):
        util.save_videos_grid(sample_gen[k:k + 1], path)
    util.save_videos_grid(sample_inv, paths[-1])
    return paths


def extra_target_embeddings(n: int, seed: int = 33) -> torch.Tensor:
    """Synthetic stand-ins for CLIP(target prompt 2 .. n) beside harness_inputs' pinned (source, target 1) pair."""
    from motioneditor_amd import synth
    return torch.from_numpy(synth.synth_normal("harness.cond.more", (n - 1, 77, 768), seed, 0.3))


def attention_tokens(a, prompts, tokenizer) -> dict:
    """name -> [token positions per prompt]: --attention-maps WORD looks the word up in every prompt (tokenizer.word_indices = the reference's
    get_word_inds, inference.py:304-311), --attention-map-tokens gives the positions themselves, the same for every prompt."""
    out = {}
    for word in a.attention_maps or []:
        if prompts is None:
            raise SystemExit("--attention-maps WORD looks the word up in the prompts: give --prompt (or name the token positions with --attention-map-tokens)")
        out[word] = [tokenizer.word_indices(p, word) for p in prompts]
        if not any(out[word]):
            raise SystemExit(f"--attention-maps {word}: no prompt holds that word")
    for spec in a.attention_map_tokens or []:
        idx = [int(t) for t in spec.split(",")]
        if not idx or min(idx) < 0 or max(idx) > 76:
            raise SystemExit(f"--attention-map-tokens {spec}: token positions are 0 .. 76")
        out["tokens-" + "-".join(map(str, idx))] = idx if prompts is None else [idx] * len(prompts)
    return out


def cross_attention_maps(sed, tokens, n_targets: int, f: int):
    """(reconstruction maps [1, f, res, res], edit maps [N, f, res, res]) of the conditional rows of the batch [u.rec, u.e_1 .. u.e_N, c.rec, c.e_1 .. c.e_N].
    tokens: one list of positions, or one list per prompt [source, target_1 .. target_N]; a prompt without the word gets a black map."""
    per_prompt = tokens if tokens and isinstance(tokens[0], (list, tuple)) else [list(tokens)] * (1 + n_targets)
    nb = 1 + n_targets
    rows = []
    for k, idx in enumerate(per_prompt):
        b = nb + k                                                        # the conditional row of prompt k
        if idx:
            rows.append(sed.aggregate_cross_attn_map(list(idx))[b * f:(b + 1) * f])
        else:
            res = int(round(sed._xa_tokens ** 0.5))
            rows.append(torch.zeros((f, res, res), device=sed._xa_acc.device))
    maps = torch.stack(rows)
    return maps[:1], maps[1:]


def run(pipe, x: dict, *, steps: int, inv_steps: int, guidance: float = 7.5, output_type: str = "tensor", graphed: bool = False, prompts=None, n_targets: int = 1,
        attention_tokens=None, maps_out=None):
    """inference.py:259-326 for one (source prompt, target prompt) pair.  Returns (sample_inv, sample_gen, ddim_inv_latent).
    prompts = [source, target]: the pipeline's own text encoder and tokenizer encode them (and the empty prompt) instead of the tensors in `x`.
    prompts = [source, target_1 .. target_N] (or n_targets = N with the synthetic embeddings): every target in the one call, all towards the clip's one target
    skeleton as the reference's loop over its prompts does (:298-302); sample_gen then holds the N edits."""
    n_targets = len(prompts) - 1 if prompts else n_targets
    from motioneditor_amd import util
    from motioneditor_amd.attn_control import (FullySelfAttentionControlMask, TemporalSelfAttentionControl,
                                               regiter_fully_attention_editor_diffusers, regiter_temporal_attention_editor_diffusers)
    from motioneditor_amd.schedulers import DDIMScheduler
    pv = x["pixel_values"]
    f, H, W = pv.shape[1], pv.shape[3], pv.shape[4]
    latents = pipe.vae.encode(pv.reshape(f, 3, H, W)).latent_dist.sample(noise=x["encode_noise"])       # "b f c h w -> (b f) c h w" (:261-262)
    latents = latents.reshape(1, f, 4, H // 8, W // 8).permute(0, 2, 1, 3, 4).contiguous() * 0.18215      # (:264-265)
    inv_sched = DDIMScheduler()
    inv_sched.set_timesteps(inv_steps)
    ddim_inv_latent = util.ddim_inversion(pipe, inv_sched, latents, inv_steps, prompt="", normal_infer=True,
                                          text_embeddings=None if prompts else x["negative_text_embeddings"])[-1]   # (:288-293; prompt "" = the empty-prompt embedding)
    ddim_inv_latent = ddim_inv_latent.repeat(1 + n_targets, 1, 1, 1, 1)                                    # (:296)
    tgt = x["target_skeleton"]
    skeleton = torch.cat([torch.zeros_like(tgt), tgt, torch.zeros_like(tgt), tgt], dim=0)                  # (:300-302)
    ted = TemporalSelfAttentionControl(start_step=4, start_layer=10)
    regiter_temporal_attention_editor_diffusers(pipe, ted)
    sed = FullySelfAttentionControlMask(start_step=4, start_layer=10, source_masks=x["source_masks"], target_masks=None, rectangle_source_masks=None)
    regiter_fully_attention_editor_diffusers(pipe, sed)
    if attention_tokens:
        sed.collect_cross_attention()        # the 16 x 16-token layers, every step, into one accumulator (the inversion above runs without editors: nothing collected)
    emb = {} if prompts else dict(text_embeddings=x["text_embeddings"], negative_text_embeddings=x["negative_text_embeddings"])
    if not prompts and n_targets > 1:
        emb["text_embeddings"] = torch.cat([x["text_embeddings"], extra_target_embeddings(n_targets).to(x["text_embeddings"].device)])
    sample = pipe(list(prompts) if prompts else ["a source prompt"] + ["a target prompt"] * n_targets, video_length=f, height=H, width=W, num_inference_steps=steps,
                  guidance_scale=guidance, latents=ddim_inv_latent, uncond_embeddings=None, skeleton=skeleton, source_masks=None, target_masks=None,
                  rectangle_source_masks=None, background_latents=None, output_type=output_type, **emb).images
    assert sample.shape[0] == 1 + n_targets
    if attention_tokens:
        sed.stop_collecting()
        for name, tokens in attention_tokens.items():
            maps_out[name] = cross_attention_maps(sed, tokens, n_targets, f)
    sample_inv, sample_gen = sample[:1], sample[1:]
    return sample_inv, sample_gen, ddim_inv_latent


# `--metrics synthetic`: the token geometry of ViT-L/14 (257 tokens) at a reduced width, seeded weights
SYNTHETIC_CLIP_VISION = dict(hidden_size=256, num_hidden_layers=3, num_attention_heads=4, intermediate_size=1024, image_size=224, patch_size=14, projection_dim=64)
SYNTHETIC_CLIP_TEXT = dict(hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, projection_dim=64)


def metric_models(spec: str, device: str = "cuda"):
    """(CLIPModel, CLIPImageProcessor, CLIPTokenizer) of --metrics: one CLIP checkpoint directory, or "synthetic"."""
    from motioneditor_amd.models.clip import CLIPImageProcessor, CLIPModel
    from motioneditor_amd.tokenizer import CLIPTokenizer
    if spec == "synthetic":
        tok = CLIPTokenizer.from_synthetic()
        text = dict(SYNTHETIC_CLIP_TEXT, vocab_size=len(tok), eos_token_id=tok.eos_token_id)
        return CLIPModel.from_synthetic(device, text_config=text, vision_config=SYNTHETIC_CLIP_VISION), CLIPImageProcessor(device=device), tok
    return CLIPModel.from_pretrained(spec, device=device), CLIPImageProcessor.from_pretrained(spec, device=device), CLIPTokenizer.from_pretrained(spec, subfolder=None)


def score(spec: str, x: dict, sample_inv, sample_gen, prompts=None, names=None, device: str = "cuda") -> dict:
    """The CLIP metrics of one run: {"source": {...}, "reconstruction": {...}, "edits": {name: {...}}}.  Frame consistency of all three; text alignment (with
    `prompts` = [source, target_1 .. target_N]) of the reconstruction against the source prompt and of every edit against its own target."""
    from motioneditor_amd import metrics
    model, processor, tok = metric_models(spec, device)
    source = ((x["pixel_values"].float() + 1.0) / 2.0).permute(0, 2, 1, 3, 4).contiguous()       # [1, f, 3, H, W] in [-1, 1] -> [1, 3, f, H, W] in [0, 1]
    names = list(names) if names else [f"edit {k + 1}" for k in range(sample_gen.shape[0])]
    out = {"clip": spec, "source": metrics.clip_metrics(source, None, model, processor),
           "reconstruction": metrics.clip_metrics(sample_inv, prompts[0] if prompts else None, model, processor, tok), "edits": {}}
    for k, name in enumerate(names):
        out["edits"][name] = metrics.clip_metrics(sample_gen[k:k + 1], prompts[1 + k] if prompts else None, model, processor, tok)
    return out


def text_models(checkpoint=None, device: str = "cuda"):
    """(text_encoder, tokenizer): the native CLIP classes from an SD-1.5 checkpoint directory, or synthetic ones."""
    from motioneditor_amd.models.clip import CLIPTextModel
    from motioneditor_amd.tokenizer import CLIPTokenizer
    if checkpoint:
        return CLIPTextModel.from_pretrained(checkpoint, subfolder="text_encoder", device=device), CLIPTokenizer.from_pretrained(checkpoint, subfolder="tokenizer")
    return CLIPTextModel.from_synthetic(device), CLIPTokenizer.from_synthetic()


def build_pipeline(device: str = "cuda"):
    from motioneditor_amd.models.controlnet import ControlNetModel
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    from motioneditor_amd.models.vae import AutoencoderKL
    from motioneditor_amd.pipelines import MotionEditorPipeline
    return MotionEditorPipeline(vae=AutoencoderKL.from_synthetic(device), unet=UNet2DConditionModel.from_synthetic(device),
                                controlnet=ControlNetModel.from_synthetic(device))


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--inv-steps", type=int, default=10)
    ap.add_argument("--executor", choices=["eager", "plan"], default="plan",
                    help="who issues the ~1100 launches of a denoising step: 'plan' = one me_denoise_step call per step (the launch list is recorded at the first step of "
                         "each editor gating, csrc/plan.hip), 'eager' = Python, launch by launch; the results are bitwise the same")
    ap.add_argument("--prompt", default=None, help="source prompt: encode the prompts with the native CLIP text encoder instead of feeding synthetic embeddings")
    ap.add_argument("--target-prompt", action="append", default=None,
                    help="target prompt (default: the source prompt); give it several times (up to 3) to edit the clip towards every one of them in one call")
    ap.add_argument("--checkpoint", default=None, help="SD-1.5 directory whose text_encoder/ and tokenizer/ serve --prompt (default: synthetic weights and vocabulary)")
    ap.add_argument("--attention-maps", action="append", default=None, metavar="WORD",
                    help="with --prompt and --out: save where the tokens of WORD look (head-mean text cross-attention of the 16 x 16 layers, averaged over the steps) as "
                         "sample/attn-WORD-inv.gif (reconstruction) and sample/attn-WORD.gif (edits); repeatable")
    ap.add_argument("--attention-map-tokens", action="append", default=None, metavar="I,J",
                    help="the same for the token positions I,J (1 = the first token after the start token); works with the synthetic embeddings; repeatable")
    ap.add_argument("--metrics", default=None, metavar="CLIP_DIR|synthetic",
                    help="with --out: score source, reconstruction and edits with the CLIP metrics (frame consistency; text alignment with --prompt) on the native CLIP "
                         "image encoder and write sample/metrics.json; CLIP_DIR = one CLIP checkpoint directory, 'synthetic' = small seeded towers")
    add_clip_arguments(ap)
    ap.add_argument("--out", default=None, help="directory that receives sample/{target prompt}.gif (the edit) and sample/{target prompt}-inv.gif (the reconstruction)")
    return ap


def main():
    a = parser().parse_args()
    pipe = build_pipeline()
    pipe.step_executor = a.executor
    prompts = None
    if a.prompt is not None:
        pipe.text_encoder, pipe.tokenizer = text_models(a.checkpoint)
        prompts = [a.prompt] + (a.target_prompt if a.target_prompt else [a.prompt])
    x = clip_inputs(a) if a.video_dir else {k: v.cuda() for k, v in harness_inputs(a.frames, a.size, a.size).items()}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want_maps = attention_tokens(a, prompts, pipe.tokenizer)
    if want_maps and not a.out:
        raise SystemExit("--attention-maps / --attention-map-tokens write GIFs: give --out")
    if a.metrics and not a.out:
        raise SystemExit("--metrics writes sample/metrics.json: give --out")
    maps = {}
    inv, gen, _ = run(pipe, x, steps=a.steps, inv_steps=a.inv_steps, prompts=prompts, n_targets=len(a.target_prompt or [None]), attention_tokens=want_maps, maps_out=maps)
    torch.cuda.synchronize()
    print(f"{a.frames} frames {a.size}x{a.size}: encode + {a.inv_steps} inversion steps + {a.steps} denoising steps + decode in {time.perf_counter() - t0:.2f} s; "
          f"reconstruction {tuple(inv.shape)}, edit {tuple(gen.shape)}, range [{float(gen.min()):.3f}, {float(gen.max()):.3f}]")
    if a.out:
        names = prompts[1:] if prompts else (a.target_prompt or ["a target prompt"])
        if len(set(names)) != len(names):     # the same target twice: keep the files apart
            names = [f"{t} ({k + 1})" for k, t in enumerate(names)]
        print("saved", *save_samples(a.out, names, inv, gen))
        from motioneditor_amd import util
        for name, (m_inv, m_gen) in maps.items():
            print("saved", util.save_attention_maps(m_inv, f"{a.out}/sample/attn-{name}-inv.gif", size=a.size),
                  util.save_attention_maps(m_gen, f"{a.out}/sample/attn-{name}.gif", size=a.size))
        if a.metrics:
            import json
            result = score(a.metrics, x, inv, gen, prompts, names)
            Path(f"{a.out}/sample/metrics.json").write_text(json.dumps(result, indent=1))
            print("metrics", json.dumps(result))
            print("saved", f"{a.out}/sample/metrics.json")


if __name__ == "__main__":
    main()
