"""TEST INFRASTRUCTURE shared by tools/make_golden_clip.py and the CLIP tests: the weights behind tests/golden/clip_text.npz.

The fixture stores inputs and outputs only; the weights are regenerated here: the project's seeded synthetic CLIP text encoder
(`models.clip.clip_text_schema` through `synth.synth_state_dict`, SD-1.5 configuration), then a seeded perturbation, because plain
random projections give near-uniform attention, under which a missing causal mask or a wrong softmax would barely show:
q / k projection weights x QK_GAIN, LayerNorm gains 1 + N(0, 0.2), every bias N(0, 0.05).

QK_GAIN: the synthetic projections have std 1 / sqrt(768) = 0.036, so a query / key element has std ~ QK_GAIN and a logit std ~ QK_GAIN^2.
At x 4 (logit std 16, attention close to one-hot) the encoder is ill-conditioned: torch's own fp16 evaluation of it is 17 % away from its fp32
one (measured by the generator), x 3 gives 3.7e-2, x 2.2 6.7e-3, and no fp16 implementation can be judged against such a target.  x 1.5 keeps the
logits at std ~ 2.3 -- softmax weights spread over e^(+-2.3), far from uniform: moving one token moves the later rows by 16 % -- with an fp16
floor of 1.7e-3 (x 1, no gain at all: 1.35e-3)."""
from __future__ import annotations

import numpy as np

SEED = 33
PERTURB_SEED = 2024
QK_GAIN = 1.5


def perturbed_state_dict(config=None) -> "dict[str, np.ndarray]":
    from motioneditor_amd import synth
    from motioneditor_amd.models.clip import clip_text_schema
    sd = dict(synth.synth_state_dict(clip_text_schema(config), SEED, salt="clip."))
    g = np.random.Generator(np.random.Philox(key=PERTURB_SEED))
    out = {}
    for k in sorted(sd):                      # (a fixed order of draws, whatever the schema's)
        v = np.array(sd[k], dtype=np.float32)
        if k.endswith(("q_proj.weight", "k_proj.weight")):
            v = v * QK_GAIN
        elif k.endswith(".bias"):
            v = (0.05 * g.standard_normal(v.shape)).astype(np.float32)
        elif "layer_norm" in k and k.endswith(".weight"):
            v = (1.0 + 0.2 * g.standard_normal(v.shape)).astype(np.float32)
        out[k] = v
    return out
