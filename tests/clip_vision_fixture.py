"""TEST INFRASTRUCTURE shared by tools/make_golden_clip_vision.py and the CLIP vision tests: the weights and inputs behind tests/golden/clip_vision.npz
and tests/golden/clip_image_processor.npz.

The fixtures store outputs only.  Weights are regenerated here: the project's seeded synthetic towers (`models.clip.clip_vision_schema` /
`clip_text_schema` through `synth.synth_state_dict`), then the seeded perturbation of tests/clip_fixture.py (q / k projection weights x QK_GAIN, LayerNorm
gains 1 + N(0, 0.2), every bias N(0, 0.05)).  Inputs are regenerated from seeded numpy Philox streams.

The parity configuration keeps the REAL token geometry at a reduced width: image 224 at patch 14 is 257 tokens (16 key tiles plus one key: the odd tail of
me_attn_full) and K = 588 -> 592 patch columns; the second configuration, patch 32, is 50 tokens.

QK_GAIN: the synthetic q / k projections of a 256-wide tower give logits of std ~ 0.35 after the 1 / 8 scale -- near-uniform attention, under which one
altered patch out of 256 moves the class embedding by ~ 1 / 256 of its norm, the size of the fp16 floor.  x 3 makes the tower ill-conditioned (torch's own
fp16 evaluation is 5.7e-3 from its fp32 one); x 2 gives a floor of 2.4e-3 with the last patch moving the class embedding by 5.4e-2.
POS_GAIN: the synthetic position table has std 1 / 16 beside patch features of std ~ 1, so swapping two patches moved the embedding by 1.3e-2 only, below
10 floors; real CLIP position embeddings are of the features' size.  x 8 (std 0.5) makes a swap move it by 4.5e-2.
The generator measures the sensitivities it asserts (last patch altered, two patches swapped: both > 10 x fp16_floor), prints and stores them."""
from __future__ import annotations

import numpy as np

SEED = 41
PERTURB_SEED = 2025
QK_GAIN = 2.0
POS_GAIN = 8.0

VISION = dict(hidden_size=256, num_hidden_layers=3, num_attention_heads=4, intermediate_size=1024, image_size=224, patch_size=14, num_channels=3,
              projection_dim=64, hidden_act="quick_gelu", layer_norm_eps=1e-5)
VISION32 = dict(VISION, patch_size=32)
TEXT = dict(vocab_size=1000, hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512, max_position_embeddings=77,
            hidden_act="quick_gelu", layer_norm_eps=1e-5)
TEXT_PROJECTION = 64
EOS = TEXT["vocab_size"] - 1          # the largest id: transformers' two pooling rules (first eos position / argmax of the ids) agree
N_IMAGES = 2


def _perturb(sd, seed):
    g = np.random.Generator(np.random.Philox(key=seed))
    out = {}
    for k in sorted(sd):                      # (a fixed order of draws, whatever the schema's)
        v = np.array(sd[k], dtype=np.float32)
        if k.endswith(("q_proj.weight", "k_proj.weight")):
            v = v * QK_GAIN
        elif k == "embeddings.position_embedding.weight" and "embeddings.class_embedding" in sd:     # (the vision tower's)
            v = v * POS_GAIN
        elif k.endswith(".bias"):
            v = (0.05 * g.standard_normal(v.shape)).astype(np.float32)
        elif ("layer_norm" in k or "layrnorm" in k or "layernorm" in k) and k.endswith(".weight"):
            v = (1.0 + 0.2 * g.standard_normal(v.shape)).astype(np.float32)
        out[k] = v
    return out


def vision_state_dict(config=None) -> "dict[str, np.ndarray]":
    from motioneditor_amd import synth
    from motioneditor_amd.models.clip import clip_vision_schema
    return _perturb(dict(synth.synth_state_dict(clip_vision_schema(config or VISION), SEED, salt="clip_vision.")), PERTURB_SEED)


def text_state_dict() -> "dict[str, np.ndarray]":
    from motioneditor_amd import synth
    from motioneditor_amd.models.clip import clip_text_schema
    schema = clip_text_schema(TEXT)
    schema["text_projection.weight"] = (TEXT_PROJECTION, TEXT["hidden_size"])
    return _perturb(dict(synth.synth_state_dict(schema, SEED, salt="clip.")), PERTURB_SEED + 1)


def pixel_values(n: int = N_IMAGES, size: int = 224, seed: int = 7) -> np.ndarray:
    """fp32 [n, 3, size, size]: a smooth field plus noise, roughly what normalised pixels look like (std ~ 1)."""
    g = np.random.Generator(np.random.Philox(key=seed))
    y, x = np.meshgrid(np.linspace(-1, 1, size, dtype=np.float32), np.linspace(-1, 1, size, dtype=np.float32), indexing="ij")
    out = np.empty((n, 3, size, size), np.float32)
    for i in range(n):
        for c in range(3):
            out[i, c] = np.sin(3.0 * x * (i + 1) + c) * np.cos(2.0 * y + 0.5 * c * (i + 1)) + 0.7 * g.standard_normal((size, size)).astype(np.float32)
    return out


def text_ids() -> np.ndarray:
    """int64 [3, 77]: the empty prompt, a 6-token prompt, a prompt that fills every position; bos = vocab - 2, eos = pad = vocab - 1."""
    bos, V = TEXT["vocab_size"] - 2, TEXT["vocab_size"] - 2
    g = np.random.Generator(np.random.Philox(key=78))
    ids = np.full((3, 77), EOS, dtype=np.int64)
    ids[:, 0] = bos
    ids[1, 1:7] = g.integers(0, V, 6)
    ids[2, 1:76] = g.integers(0, V, 75)
    return ids


IMAGE_SIZES = ((96, 128), (150, 113), (64, 48), (224, 224))       # (H, W): landscape, portrait, a 4.67x upscale, identity


def images() -> "list[np.ndarray]":
    """Four uint8 HWC images: a smooth colour field plus a fine texture (so that both the antialiasing support and the rounding are exercised)."""
    g = np.random.Generator(np.random.Philox(key=99))
    out = []
    for i, (H, W) in enumerate(IMAGE_SIZES):
        y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        im = np.empty((H, W, 3), np.float64)
        for c in range(3):
            im[..., c] = 128 + 90 * np.sin(x / (7.0 + c) + i) * np.cos(y / (5.0 + 2 * c)) + 25 * g.standard_normal((H, W))
        im[:H // 4, :W // 4] = 255.0           # saturated corners: the negative lobes of the cubic overshoot here, the clip to [0, 255] is exercised
        im[-(H // 4):, -(W // 4):] = 0.0
        out.append(np.clip(np.rint(im), 0, 255).astype(np.uint8))
    return out
