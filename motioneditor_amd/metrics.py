"""The two CLIP metrics the MotionEditor, Tune-A-Video and vid2vid-zero papers report for an edited clip, on this package's CLIP (models.clip) and the
cosine kernel of libmotioned (ops.cosine_rows, me_cosine_rows):

  text alignment      mean over the frames of cos(image embedding of the frame, text embedding of the target prompt)
  frame consistency   mean over consecutive frames of cos(image embedding of frame t, image embedding of frame t + 1)

The frames that are scored are the frames a user sees: `clip_metrics` quantises the video exactly as `util.save_videos_grid` does (ops.video_grid_u8 with
b = 1: `(x * 255)` truncated to uint8), then runs the image processor and the vision tower on those bytes."""
from __future__ import annotations

from typing import Dict

import torch

from . import ops


def _rows(t: torch.Tensor, name: str) -> torch.Tensor:
    if not torch.is_tensor(t) or t.dim() not in (1, 2) or t.numel() == 0:
        raise ValueError(f"{name}: expected embeddings [n, D] (or one [D]), got {tuple(getattr(t, 'shape', ()))}")
    t = t.detach()
    if t.dim() == 1:
        t = t[None]
    return t if t.dtype == torch.float32 else t.float()


def frame_consistency(image_embeds: torch.Tensor) -> float:
    """Mean cosine between the embeddings of consecutive frames; image_embeds fp32 [f, D], f >= 2."""
    e = _rows(image_embeds, "frame_consistency")
    if e.shape[0] < 2:
        raise ValueError("frame_consistency: needs at least two frames")
    return float(ops.cosine_rows(e[:-1], e[1:]).double().mean())


def text_alignment(image_embeds: torch.Tensor, text_embeds: torch.Tensor) -> float:
    """Mean cosine between every frame's embedding and the ONE text embedding; image_embeds fp32 [f, D], text_embeds fp32 [D] or [1, D]."""
    e, t = _rows(image_embeds, "text_alignment"), _rows(text_embeds, "text_alignment")
    if t.shape[0] != 1 or t.shape[1] != e.shape[1]:
        raise ValueError(f"text_alignment: one text embedding of width {e.shape[1]} expected, got {tuple(t.shape)}")
    return float(ops.cosine_rows(e, t.to(e.device)).double().mean())


def video_frames_u8(video: torch.Tensor) -> torch.Tensor:
    """fp32 video [1, 3, f, h, w] in [0, 1] -> uint8 frames [f, h, w, 3] on the device, quantised as util.save_videos_grid quantises a GIF's frames."""
    if not torch.is_tensor(video) or video.dim() != 5 or video.shape[0] != 1 or video.shape[1] != 3:
        raise ValueError(f"clip_metrics: expected a video [1, 3, f, h, w], got {tuple(getattr(video, 'shape', ()))}")
    v = video.detach()
    if v.dtype != torch.float32:
        v = v.float()
    return ops.video_grid_u8(v, n_rows=4, rescale=False)


@torch.no_grad()
def image_embeddings(video: torch.Tensor, model, processor) -> torch.Tensor:
    """fp32 [f, projection_dim]: the CLIP image embedding of every frame of an fp32 [1, 3, f, h, w] video in [0, 1]."""
    frames = video_frames_u8(video.to(model.device))
    return model.get_image_features(processor(images=frames, return_tensors="pt").pixel_values)


@torch.no_grad()
def clip_metrics(video: torch.Tensor, prompt, model, processor, tokenizer=None) -> Dict[str, float]:
    """{"frame_consistency": ..., "text_alignment": ...} of an fp32 [1, 3, f, h, w] video in [0, 1] against `prompt` (a string; None or a missing tokenizer
    leaves the text alignment out).  `model` has get_image_features / get_text_features (models.clip.CLIPModel), `processor` is a CLIPImageProcessor."""
    emb = image_embeddings(video, model, processor)
    out = {"frame_consistency": frame_consistency(emb)} if emb.shape[0] > 1 else {}
    if prompt is not None and tokenizer is not None:
        ids = tokenizer([prompt], padding="max_length", max_length=tokenizer.model_max_length, truncation=True, return_tensors="pt").input_ids
        out["text_alignment"] = text_alignment(emb, model.get_text_features(ids))
    return out
