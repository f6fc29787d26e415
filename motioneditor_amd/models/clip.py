"""CLIP text encoder on libmotioned: transformers' `CLIPTextModel` as the reference calls it -- `text_encoder(input_ids)[0]` in
`pipeline_motion_editor.py:262-274`, `util.py:59-71`, `null_text_optimization.py:94-105`, `train_bg.py:333` -- so that prompts enter
the pipeline as strings with this package alone (`motioneditor_amd.tokenizer.CLIPTokenizer` makes the ids).

Same constructor contract as the other models here: a state dict with transformers' keys (with or without the `text_model.`
prefix), packed by `weights.Packed`; fp16 storage, fp32 accumulation, fp16 residual stream.

Launch graph, 2 + 8 per layer (98 for SD-1.5's 12 layers):
    me_embed_rows                                  x = tok[ids] + pos
    per layer   me_layernorm                       LN1(x)
                me_gemm (+bias)                    q | k | v as one [3C, C] projection
                me_attn_causal                     softmax_{j <= i}(q k^T / sqrt(64)) v per (prompt, head)
                me_gemm (+bias, +res)              x += out_proj(.)
                me_layernorm                       LN2(x)
                me_gemm (+bias)                    fc1
                me_quick_gelu                      h * sigmoid(1.702 h)
                me_gemm (+bias, +res)              x += fc2(.)
    me_layernorm                                   final_layer_norm
and one me_rows_to_nchw launch as the fp16 -> fp32 cast of the result.  Only the causal mask is applied (`attention_mask=None` is
what the reference passes for SD-1.5); the pooled output is not used anywhere in the reference and is not computed.  The encoder is
not part of a recorded step (`plan.StepPlan` is bound to a step's latents and text rows): it refuses to run while one records.
"""
from __future__ import annotations

import json
import re
from collections import OrderedDict
from pathlib import Path
from types import SimpleNamespace
from typing import Dict, Mapping, Optional, Tuple

import numpy as np
import torch

from .. import ops, plan
from ..weights import Packed
from .compat import ModuleShims

# SD-1.5 `text_encoder/config.json` (openai/clip-vit-large-patch14's text tower)
DEFAULT_CONFIG = dict(vocab_size=49408, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                      max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5)
HEAD_DIM = 64   # me_attn_causal
_PREFIX = "text_model."
_IGNORED = ("embeddings.position_ids",)


def clip_text_schema(config: Optional[Mapping[str, object]] = None) -> "OrderedDict[str, Tuple[int, ...]]":
    """Key -> shape of transformers' `CLIPTextModel` without the `text_model.` prefix (what `synth.synth_state_dict` draws the synthetic
    encoder from, and the key set a checkpoint is checked against)."""
    c = dict(DEFAULT_CONFIG, **dict(config or {}))
    C, ff = int(c["hidden_size"]), int(c["intermediate_size"])
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    s["embeddings.token_embedding.weight"] = (int(c["vocab_size"]), C)
    s["embeddings.position_embedding.weight"] = (int(c["max_position_embeddings"]), C)
    for i in range(int(c["num_hidden_layers"])):
        p = f"encoder.layers.{i}."
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):       # (transformers' own parameter order)
            s[p + f"self_attn.{n}.weight"] = (C, C)
            s[p + f"self_attn.{n}.bias"] = (C,)
        s[p + "layer_norm1.weight"] = s[p + "layer_norm1.bias"] = (C,)
        s[p + "mlp.fc1.weight"], s[p + "mlp.fc1.bias"] = (ff, C), (ff,)
        s[p + "mlp.fc2.weight"], s[p + "mlp.fc2.bias"] = (C, ff), (C,)
        s[p + "layer_norm2.weight"] = s[p + "layer_norm2.bias"] = (C,)
    s["final_layer_norm.weight"] = s["final_layer_norm.bias"] = (C,)
    return s


def _canonical(state_dict: Mapping[str, object]) -> Dict[str, object]:
    """Strip the `text_model.` prefix (SD-1.5's text_encoder/model.safetensors has it, transformers 5.x names the parameters without it)
    and drop the `position_ids` buffer."""
    out = {}
    for k, v in state_dict.items():
        k = k[len(_PREFIX):] if k.startswith(_PREFIX) else k
        if k not in _IGNORED:
            out[k] = v
    return out


class CLIPTextModelOutput:
    """`out[0]` / `out.last_hidden_state`: fp32 [n, seq, C] on the device."""

    def __init__(self, last_hidden_state: torch.Tensor):
        self.last_hidden_state = last_hidden_state

    def __getitem__(self, i):
        return (self.last_hidden_state,)[i]


class CLIPTextModel(ModuleShims):
    def __init__(self, state_dict, config: Optional[Mapping[str, object]] = None, device: str = "cuda", dtype: torch.dtype = torch.float16):
        sd = _canonical(state_dict)
        for k in ("embeddings.token_embedding.weight", "embeddings.position_embedding.weight"):
            if k not in sd:
                raise KeyError(f"CLIPTextModel: the state dict lacks {k}")
        layers = [int(m.group(1)) for m in (re.match(r"encoder\.layers\.(\d+)\.", k) for k in sd) if m]
        cfg = dict(DEFAULT_CONFIG, **{k: v for k, v in dict(config or {}).items() if k in DEFAULT_CONFIG})
        # layer count, vocabulary size and position count follow the state dict (so do the two widths)
        cfg["num_hidden_layers"] = max(layers) + 1 if layers else 0
        cfg["vocab_size"], cfg["hidden_size"] = (int(d) for d in sd["embeddings.token_embedding.weight"].shape)
        cfg["max_position_embeddings"] = int(sd["embeddings.position_embedding.weight"].shape[0])
        fc1 = sd.get("encoder.layers.0.mlp.fc1.weight")
        if fc1 is not None:
            cfg["intermediate_size"] = int(fc1.shape[0])
        if cfg["hidden_act"] != "quick_gelu":
            raise NotImplementedError(f"CLIPTextModel: hidden_act={cfg['hidden_act']!r} (only 'quick_gelu', SD-1.5's, has a kernel: me_quick_gelu)")
        heads = int(cfg["num_attention_heads"])
        if heads <= 0 or cfg["hidden_size"] % heads or cfg["hidden_size"] // heads != HEAD_DIM:
            raise NotImplementedError(f"CLIPTextModel: head size {cfg['hidden_size']}/{heads} = {cfg['hidden_size'] / max(heads, 1):g} (me_attn_causal serves {HEAD_DIM})")
        schema = clip_text_schema(cfg)
        for k in sd:
            if k not in schema:
                raise KeyError(f"CLIPTextModel: unexpected key {k!r} in the state dict")
        for k, shape in schema.items():
            if k not in sd:
                raise KeyError(f"CLIPTextModel: the state dict lacks {k}")
            if tuple(sd[k].shape) != tuple(shape):
                raise ValueError(f"CLIPTextModel: {k} has shape {tuple(sd[k].shape)}, expected {tuple(shape)}")
        self.config = SimpleNamespace(**cfg)
        self.P = Packed(sd, device, dtype=dtype)
        self.device = torch.device(device)
        self.dtype = dtype

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, subfolder="text_encoder", device="cuda", **kwargs) -> "CLIPTextModel":
        """transformers' signature for a local directory (inference.py:152: CLIPTextModel.from_pretrained(path, subfolder="text_encoder")):
        reads `config.json` and `model.safetensors` / `pytorch_model.bin`."""
        from .. import checkpoint
        d = Path(pretrained_model_name_or_path) / subfolder if subfolder else Path(pretrained_model_name_or_path)
        cfg = json.loads((d / "config.json").read_text()) if (d / "config.json").exists() else None
        return cls(checkpoint.load_file(checkpoint.find_weights(pretrained_model_name_or_path, subfolder)), cfg, device)

    @classmethod
    def from_synthetic(cls, device: str = "cuda", seed: int = 33, config: Optional[Mapping[str, object]] = None) -> "CLIPTextModel":
        from .. import synth
        return cls(synth.synth_state_dict(clip_text_schema(config), seed, salt="clip."), config, device)

    def _encode(self, input_ids: torch.Tensor, attention_mask=None, position_ids=None):
        """The checks and the launch graph of `forward`: (fp16 rows [n * seq, C] after final_layer_norm, the ids on the host [n, seq])."""
        c = self.config
        if attention_mask is not None:
            raise NotImplementedError("CLIPTextModel: attention_mask is not supported (the reference passes None for SD-1.5; only the causal mask is applied)")
        if position_ids is not None:
            raise NotImplementedError("CLIPTextModel: position_ids is not supported (positions are 0 .. seq - 1)")
        if plan.ACTIVE is not None:
            raise RuntimeError("CLIPTextModel: a denoising step is being recorded (plan.StepPlan.recording); encode the prompts before the step, "
                               "the encoder's launches do not belong in the step's plan")
        ids = torch.as_tensor(input_ids).detach().cpu()      # the ids come from the host (the tokenizer): checked here, not on the device
        if ids.dim() == 1:
            ids = ids[None]
        if ids.dim() != 2 or ids.dtype not in (torch.int64, torch.int32) or ids.numel() == 0:
            raise ValueError(f"CLIPTextModel: input_ids must be an integer [n, seq] tensor, got {ids.dtype} {tuple(ids.shape)}")
        n, seq = ids.shape
        if seq > c.max_position_embeddings:
            raise ValueError(f"CLIPTextModel: {seq} tokens per prompt, the position table has {c.max_position_embeddings}")
        lo, hi = int(ids.min()), int(ids.max())
        if lo < 0 or hi >= c.vocab_size:
            raise ValueError(f"CLIPTextModel: token id {lo if lo < 0 else hi} is outside the vocabulary [0, {c.vocab_size})")
        P, C, heads = self.P, c.hidden_size, c.num_attention_heads
        ids_dev = ids.to(torch.int32).reshape(-1).contiguous().to(self.device)
        x = ops.embed_rows(P.mat("embeddings.token_embedding.weight").reshape(c.vocab_size, C),
                           P.mat("embeddings.position_embedding.weight").reshape(c.max_position_embeddings, C), ids_dev, seq)
        for i in range(c.num_hidden_layers):
            p = f"encoder.layers.{i}."
            a = p + "self_attn."
            h = ops.layernorm(x, P.vec(p + "layer_norm1.weight"), P.vec(p + "layer_norm1.bias"), c.layer_norm_eps)
            qkv = ops.gemm(h, P.fused([a + "q_proj.weight", a + "k_proj.weight", a + "v_proj.weight"]),
                           bias=P.fused_vec([a + "q_proj.bias", a + "k_proj.bias", a + "v_proj.bias"]))
            o = ops.attention_causal(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], heads=heads, dh=HEAD_DIM, n_seq=n, nq=seq)
            x = ops.gemm(o, P.mat(a + "out_proj.weight"), bias=P.vec(a + "out_proj.bias"), res=x)
            h = ops.layernorm(x, P.vec(p + "layer_norm2.weight"), P.vec(p + "layer_norm2.bias"), c.layer_norm_eps)
            m = ops.quick_gelu(ops.gemm(h, P.mat(p + "mlp.fc1.weight"), bias=P.vec(p + "mlp.fc1.bias")))
            x = ops.gemm(m, P.mat(p + "mlp.fc2.weight"), bias=P.vec(p + "mlp.fc2.bias"), res=x)
        x = ops.layernorm(x, P.vec("final_layer_norm.weight"), P.vec("final_layer_norm.bias"), c.layer_norm_eps)
        return x, ids

    @torch.no_grad()
    def forward(self, input_ids: torch.Tensor, attention_mask=None, position_ids=None, **kwargs) -> CLIPTextModelOutput:
        x, ids = self._encode(input_ids, attention_mask, position_ids)
        n, seq = ids.shape
        return CLIPTextModelOutput(ops.rows_to_nchw(x, n * seq, self.config.hidden_size, 1).reshape(n, seq, self.config.hidden_size))     # (the fp16 -> fp32 cast)

    def __call__(self, *args, **kwargs):
        return self.forward(*args, **kwargs)


# ======================================================================================================================================================
# The other half of CLIP: the vision tower with its projection, the text tower's projected pooled output, the image processor.  Together they give the
# two embeddings the CLIP metrics compare (motioneditor_amd.metrics).
#
# Launch graph of the vision tower, 4 + 8 per layer + 2 (198 for ViT-L/14's 24 layers):
#     me_patch_rows                                  pixel_values -> rows of flattened patches, K = 3 p^2 padded to a multiple of 8
#     me_gemm                                        the stride = kernel patch convolution, no bias
#     me_vit_tokens                                  [class | patches] + position embedding
#     me_layernorm                                   pre_layrnorm (upstream's spelling)
#     per layer   the text tower's eight launches with me_attn_full in place of me_attn_causal
#     me_layernorm                                   post_layernorm on the class rows only (a strided view, one row per image)
#     me_gemm                                        visual_projection, no bias
# and me_rows_to_nchw launches as the fp16 -> fp32 casts of the results.
# ======================================================================================================================================================
# openai/clip-vit-large-patch14's vision tower
DEFAULT_VISION_CONFIG = dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096, image_size=224, patch_size=14, num_channels=3,
                             projection_dim=768, hidden_act="quick_gelu", layer_norm_eps=1e-5)
_VISION_PREFIX = "vision_model."
OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
PIL_BICUBIC = 3         # PIL.Image.Resampling.BICUBIC, the `resample` of CLIP's preprocessor_config.json


def _layer_schema(s, C: int, ff: int, layers: int) -> None:
    for i in range(layers):
        p = f"encoder.layers.{i}."
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            s[p + f"self_attn.{n}.weight"] = (C, C)
            s[p + f"self_attn.{n}.bias"] = (C,)
        s[p + "layer_norm1.weight"] = s[p + "layer_norm1.bias"] = (C,)
        s[p + "mlp.fc1.weight"], s[p + "mlp.fc1.bias"] = (ff, C), (ff,)
        s[p + "mlp.fc2.weight"], s[p + "mlp.fc2.bias"] = (C, ff), (C,)
        s[p + "layer_norm2.weight"] = s[p + "layer_norm2.bias"] = (C,)


def clip_vision_schema(config: Optional[Mapping[str, object]] = None) -> "OrderedDict[str, Tuple[int, ...]]":
    """Key -> shape of transformers' `CLIPVisionModelWithProjection` without the `vision_model.` prefix (`visual_projection.weight` never has one)."""
    c = dict(DEFAULT_VISION_CONFIG, **dict(config or {}))
    C, ff, ps = int(c["hidden_size"]), int(c["intermediate_size"]), int(c["patch_size"])
    tokens = (int(c["image_size"]) // ps) ** 2 + 1
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    s["embeddings.class_embedding"] = (C,)
    s["embeddings.patch_embedding.weight"] = (C, int(c["num_channels"]), ps, ps)
    s["embeddings.position_embedding.weight"] = (tokens, C)
    s["pre_layrnorm.weight"] = s["pre_layrnorm.bias"] = (C,)
    _layer_schema(s, C, ff, int(c["num_hidden_layers"]))
    s["post_layernorm.weight"] = s["post_layernorm.bias"] = (C,)
    s["visual_projection.weight"] = (int(c["projection_dim"]), C)
    return s


def _canonical_vision(state_dict: Mapping[str, object]) -> Dict[str, object]:
    out = {}
    for k, v in state_dict.items():
        k = k[len(_VISION_PREFIX):] if k.startswith(_VISION_PREFIX) else k
        if k not in _IGNORED:
            out[k] = v
    return out


def _encoder_layer(P, x, p: str, heads: int, eps: float, attend):
    """The eight launches of one CLIP encoder layer; `attend(q, k, v)` is the tower's attention."""
    C = x.shape[1]
    a = p + "self_attn."
    h = ops.layernorm(x, P.vec(p + "layer_norm1.weight"), P.vec(p + "layer_norm1.bias"), eps)
    qkv = ops.gemm(h, P.fused([a + "q_proj.weight", a + "k_proj.weight", a + "v_proj.weight"]),
                   bias=P.fused_vec([a + "q_proj.bias", a + "k_proj.bias", a + "v_proj.bias"]))
    o = attend(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:])
    x = ops.gemm(o, P.mat(a + "out_proj.weight"), bias=P.vec(a + "out_proj.bias"), res=x)
    h = ops.layernorm(x, P.vec(p + "layer_norm2.weight"), P.vec(p + "layer_norm2.bias"), eps)
    m = ops.quick_gelu(ops.gemm(h, P.mat(p + "mlp.fc1.weight"), bias=P.vec(p + "mlp.fc1.bias")))
    return ops.gemm(m, P.mat(p + "mlp.fc2.weight"), bias=P.vec(p + "mlp.fc2.bias"), res=x)


class CLIPVisionModelOutput:
    """`.image_embeds` fp32 [n, projection_dim], `.last_hidden_state` fp32 [n, tokens, C] (the encoder's output, before post_layernorm), on the device."""

    def __init__(self, image_embeds: torch.Tensor, last_hidden_state: torch.Tensor):
        self.image_embeds, self.last_hidden_state = image_embeds, last_hidden_state

    def __getitem__(self, i):
        return (self.image_embeds, self.last_hidden_state)[i]


class CLIPVisionModelWithProjection(ModuleShims):
    def __init__(self, state_dict, config: Optional[Mapping[str, object]] = None, device: str = "cuda", dtype: torch.dtype = torch.float16):
        sd = _canonical_vision(state_dict)
        name = "CLIPVisionModelWithProjection"
        for k in ("embeddings.class_embedding", "embeddings.patch_embedding.weight", "embeddings.position_embedding.weight", "visual_projection.weight"):
            if k not in sd:
                raise KeyError(f"{name}: the state dict lacks {k}")
        layers = [int(m.group(1)) for m in (re.match(r"encoder\.layers\.(\d+)\.", k) for k in sd) if m]
        cfg = dict(DEFAULT_VISION_CONFIG, **{k: v for k, v in dict(config or {}).items() if k in DEFAULT_VISION_CONFIG})
        # layer count, widths, patch size and projection size follow the state dict; the image size is the configuration's and must match the position table
        cfg["num_hidden_layers"] = max(layers) + 1 if layers else 0
        pw = tuple(int(d) for d in sd["embeddings.patch_embedding.weight"].shape)
        if len(pw) != 4 or pw[1] != 3 or pw[2] != pw[3]:
            raise ValueError(f"{name}: embeddings.patch_embedding.weight has shape {pw}, expected [C, 3, patch, patch]")
        cfg["hidden_size"], cfg["num_channels"], cfg["patch_size"] = pw[0], 3, pw[2]
        cfg["projection_dim"] = int(sd["visual_projection.weight"].shape[0])
        fc1 = sd.get("encoder.layers.0.mlp.fc1.weight")
        if fc1 is not None:
            cfg["intermediate_size"] = int(fc1.shape[0])
        if cfg["hidden_act"] != "quick_gelu":
            raise NotImplementedError(f"{name}: hidden_act={cfg['hidden_act']!r} (only 'quick_gelu' has a kernel: me_quick_gelu)")
        heads = int(cfg["num_attention_heads"])
        if heads <= 0 or cfg["hidden_size"] % heads or cfg["hidden_size"] // heads != HEAD_DIM:
            raise NotImplementedError(f"{name}: head size {cfg['hidden_size']}/{heads} = {cfg['hidden_size'] / max(heads, 1):g} (me_attn_full serves {HEAD_DIM})")
        size, ps = int(cfg["image_size"]), cfg["patch_size"]
        tokens = int(sd["embeddings.position_embedding.weight"].shape[0])
        if size <= 0 or size % ps or (size // ps) ** 2 + 1 != tokens:
            raise ValueError(f"{name}: image_size {size} at patch size {ps} does not match the position table of {tokens} tokens")
        schema = clip_vision_schema(cfg)
        for k in sd:
            if k not in schema:
                raise KeyError(f"{name}: unexpected key {k!r} in the state dict")
        for k, shape in schema.items():
            if k not in sd:
                raise KeyError(f"{name}: the state dict lacks {k}")
            if tuple(sd[k].shape) != tuple(shape):
                raise ValueError(f"{name}: {k} has shape {tuple(sd[k].shape)}, expected {tuple(shape)}")
        self.config = SimpleNamespace(**cfg)
        self.tokens = tokens
        self.P = Packed(sd, device, dtype=dtype)
        self.device = torch.device(device)
        self.dtype = dtype

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, subfolder="image_encoder", device="cuda", **kwargs) -> "CLIPVisionModelWithProjection":
        """transformers' signature for a local directory: reads `config.json` (a CLIP model's `vision_config` and `projection_dim` are understood too) and
        `model.safetensors` / `pytorch_model.bin`; the keys of the other tower of a whole CLIP checkpoint are left aside."""
        from .. import checkpoint
        d = Path(pretrained_model_name_or_path) / subfolder if subfolder else Path(pretrained_model_name_or_path)
        cfg = _tower_config(d, "vision_config")
        sd = checkpoint.load_file(checkpoint.find_weights(pretrained_model_name_or_path, subfolder))
        return cls(_vision_keys(sd), cfg, device)

    @classmethod
    def from_synthetic(cls, device: str = "cuda", seed: int = 33, config: Optional[Mapping[str, object]] = None) -> "CLIPVisionModelWithProjection":
        from .. import synth
        return cls(synth.synth_state_dict(clip_vision_schema(config), seed, salt="clip_vision."), config, device)

    def _patch_weight(self) -> torch.Tensor:
        """[C, 1, Kpad]: the convolution weight flattened in its own (channel, py, px) order, K = 3 p^2 padded with zero columns as me_patch_rows pads its rows."""
        key = "patch:embeddings.patch_embedding.weight"
        hit = self.P.cache.get(key)
        if hit is None:
            w = self.P.raw("embeddings.patch_embedding.weight")
            C, K = w.shape[0], w.shape[1] * w.shape[2] * w.shape[3]
            pad = torch.zeros((C, 1, (K + 7) // 8 * 8), dtype=torch.float32)
            pad[:, 0, :K] = w.reshape(C, K)
            hit = self.P._put(key, pad)
        return hit

    @torch.no_grad()
    def forward(self, pixel_values: torch.Tensor, **kwargs) -> CLIPVisionModelOutput:
        c, name = self.config, "CLIPVisionModelWithProjection"
        if plan.ACTIVE is not None:
            raise RuntimeError(f"{name}: a denoising step is being recorded (plan.StepPlan.recording); score the frames after the step, "
                               "the encoder's launches do not belong in the step's plan")
        pv = getattr(pixel_values, "pixel_values", pixel_values)
        if not torch.is_tensor(pv) or pv.dim() != 4 or pv.dtype != torch.float32 or pv.shape[0] == 0:
            raise ValueError(f"{name}: pixel_values must be an fp32 [n, 3, S, S] tensor, got {getattr(pv, 'dtype', type(pv))} {tuple(getattr(pv, 'shape', ()))}")
        if tuple(pv.shape[1:]) != (3, c.image_size, c.image_size):
            raise ValueError(f"{name}: pixel_values {tuple(pv.shape)} do not match the image size {c.image_size} of the position table ({self.tokens} tokens)")
        pv = pv.to(self.device)
        P, C, heads, n, T = self.P, c.hidden_size, c.num_attention_heads, pv.shape[0], self.tokens
        rows = ops.patch_rows(pv, c.patch_size)
        po = ops.gemm(rows, self._patch_weight())
        x = ops.vit_tokens(po, P.vec("embeddings.class_embedding"), P.mat("embeddings.position_embedding.weight").reshape(T, C), n)
        x = ops.layernorm(x, P.vec("pre_layrnorm.weight"), P.vec("pre_layrnorm.bias"), c.layer_norm_eps)
        attend = lambda q, k, v: ops.attention_full(q, k, v, heads=heads, dh=HEAD_DIM, n_seq=n, n=T)   # noqa: E731
        for i in range(c.num_hidden_layers):
            x = _encoder_layer(P, x, f"encoder.layers.{i}.", heads, c.layer_norm_eps, attend)
        pooled = ops.layernorm(x[::T], P.vec("post_layernorm.weight"), P.vec("post_layernorm.bias"), c.layer_norm_eps)    # the class rows: row stride T * C
        emb = ops.gemm(pooled, P.mat("visual_projection.weight"))
        return CLIPVisionModelOutput(ops.rows_to_nchw(emb, n, c.projection_dim, 1).reshape(n, c.projection_dim),
                                     ops.rows_to_nchw(x, n * T, C, 1).reshape(n, T, C))

    def __call__(self, *args, **kwargs):
        return self.forward(*args, **kwargs)


def _tower_config(d: Path, tower: str) -> Optional[dict]:
    """config.json of a model directory; a whole CLIP model's (`text_config`, `vision_config`, `projection_dim`) is flattened to the tower's."""
    if not (d / "config.json").exists():
        return None
    cfg = json.loads((d / "config.json").read_text())
    if isinstance(cfg.get(tower), Mapping):
        cfg = dict(cfg[tower], **({"projection_dim": cfg["projection_dim"]} if "projection_dim" in cfg else {}))
    return cfg


def _vision_keys(sd: Mapping[str, object]) -> Dict[str, object]:
    """A checkpoint's vision tower: `vision_model.*` and `visual_projection.weight`; with neither prefix present, everything."""
    if any(k.startswith(_VISION_PREFIX) for k in sd):
        return {k: v for k, v in sd.items() if k.startswith(_VISION_PREFIX) or k == "visual_projection.weight"}
    return dict(sd)


def _text_keys(sd: Mapping[str, object]) -> Dict[str, object]:
    if any(k.startswith(_PREFIX) for k in sd):
        return {k: v for k, v in sd.items() if k.startswith(_PREFIX) or k == "text_projection.weight"}
    return dict(sd)


class CLIPTextModelWithProjectionOutput(CLIPTextModelOutput):
    """`.text_embeds` fp32 [n, projection_dim], `.last_hidden_state` fp32 [n, seq, C]."""

    def __init__(self, text_embeds: torch.Tensor, last_hidden_state: torch.Tensor):
        super().__init__(last_hidden_state)
        self.text_embeds = text_embeds

    def __getitem__(self, i):
        return (self.text_embeds, self.last_hidden_state)[i]


class CLIPTextModelWithProjection(CLIPTextModel):
    """The text graph of `CLIPTextModel`, then per prompt the row at the first position that holds `eos_token_id` (a configuration with the legacy
    `eos_token_id = 2` pools at the largest id, as transformers does) through `text_projection` (no bias): one me_gemm of one row per prompt."""

    def __init__(self, state_dict, config: Optional[Mapping[str, object]] = None, device: str = "cuda", dtype: torch.dtype = torch.float16):
        sd = dict(state_dict)
        if "text_projection.weight" not in sd:
            raise KeyError("CLIPTextModelWithProjection: the state dict lacks text_projection.weight (SD-1.5's text_encoder/ has none: text alignment needs a "
                           "whole CLIP checkpoint)")
        proj = sd.pop("text_projection.weight")
        super().__init__(sd, config, device, dtype)
        if proj.ndim != 2 or int(proj.shape[1]) != self.config.hidden_size:
            raise ValueError(f"CLIPTextModelWithProjection: text_projection.weight has shape {tuple(proj.shape)}, expected [projection_dim, {self.config.hidden_size}]")
        self.config.projection_dim = int(proj.shape[0])
        eos = dict(config or {}).get("eos_token_id")
        self.config.eos_token_id = self.config.vocab_size - 1 if eos is None else int(eos)
        self.P.make_private()         # the tower's store (lazy: nothing is on the device yet) takes the projection as one more name
        self.P.state["text_projection.weight"] = proj

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, subfolder="text_encoder", device="cuda", **kwargs) -> "CLIPTextModelWithProjection":
        from .. import checkpoint
        d = Path(pretrained_model_name_or_path) / subfolder if subfolder else Path(pretrained_model_name_or_path)
        return cls(_text_keys(checkpoint.load_file(checkpoint.find_weights(pretrained_model_name_or_path, subfolder))), _tower_config(d, "text_config"), device)

    @classmethod
    def from_synthetic(cls, device: str = "cuda", seed: int = 33, config: Optional[Mapping[str, object]] = None) -> "CLIPTextModelWithProjection":
        from .. import synth
        c = dict(DEFAULT_CONFIG, **dict(config or {}))
        schema = clip_text_schema(config)
        schema["text_projection.weight"] = (int(c.get("projection_dim", 768)), int(c["hidden_size"]))
        return cls(synth.synth_state_dict(schema, seed, salt="clip."), config, device)

    def pooled_positions(self, ids: torch.Tensor) -> torch.Tensor:
        eos = self.config.eos_token_id
        if eos == 2:
            return ids.argmax(dim=-1)
        hit = ids == eos
        if not bool(hit.any(dim=-1).all()):
            raise ValueError(f"CLIPTextModelWithProjection: a prompt holds no end-of-text token ({eos}); the pooled output is taken at its first position")
        return hit.int().argmax(dim=-1)

    @torch.no_grad()
    def forward(self, input_ids: torch.Tensor, attention_mask=None, position_ids=None, **kwargs) -> CLIPTextModelWithProjectionOutput:
        ids = torch.as_tensor(input_ids).detach().cpu()
        if ids.dim() == 1:
            ids = ids[None]
        if ids.dim() == 2 and ids.numel() and ids.dtype in (torch.int64, torch.int32):
            pos = self.pooled_positions(ids)          # (checked before any launch; _encode checks the rest)
        x, ids = self._encode(input_ids, attention_mask, position_ids)
        n, seq = ids.shape
        C, D = self.config.hidden_size, self.config.projection_dim
        W = self.P.mat("text_projection.weight")
        emb = ops.empty(n, D, x)
        for i in range(n):
            r = i * seq + int(pos[i])
            ops.gemm(x[r:r + 1], W, out=emb[i:i + 1])
        return CLIPTextModelWithProjectionOutput(ops.rows_to_nchw(emb, n, D, 1).reshape(n, D), ops.rows_to_nchw(x, n * seq, C, 1).reshape(n, seq, C))


class CLIPModel:
    """One CLIP checkpoint directory (`text_model.*`, `vision_model.*`, `visual_projection`, `text_projection`; `logit_scale` is not used) as the two towers:
    `get_image_features(pixel_values)` and `get_text_features(input_ids)` return the projected, un-normalised fp32 embeddings."""

    def __init__(self, text_model: CLIPTextModelWithProjection, vision_model: CLIPVisionModelWithProjection):
        self.text_model, self.vision_model = text_model, vision_model
        self.device = vision_model.device

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, subfolder=None, device="cuda", **kwargs) -> "CLIPModel":
        from .. import checkpoint
        d = Path(pretrained_model_name_or_path) / subfolder if subfolder else Path(pretrained_model_name_or_path)
        sd = checkpoint.load_file(checkpoint.find_weights(pretrained_model_name_or_path, subfolder))
        known = lambda k: k.startswith((_PREFIX, _VISION_PREFIX)) or k in ("visual_projection.weight", "text_projection.weight", "logit_scale")   # noqa: E731
        unknown = [k for k in sd if not known(k)]
        if unknown:
            raise KeyError(f"CLIPModel: unexpected key {unknown[0]!r} in {d}")
        for k in ("visual_projection.weight", "text_projection.weight"):
            if k not in sd:
                raise KeyError(f"CLIPModel: {d} lacks {k}")
        return cls(CLIPTextModelWithProjection(_text_keys(sd), _tower_config(d, "text_config"), device),
                   CLIPVisionModelWithProjection(_vision_keys(sd), _tower_config(d, "vision_config"), device))

    @classmethod
    def from_synthetic(cls, device: str = "cuda", seed: int = 33, text_config: Optional[Mapping[str, object]] = None,
                       vision_config: Optional[Mapping[str, object]] = None) -> "CLIPModel":
        return cls(CLIPTextModelWithProjection.from_synthetic(device, seed, text_config), CLIPVisionModelWithProjection.from_synthetic(device, seed, vision_config))

    def get_image_features(self, pixel_values, **kwargs) -> torch.Tensor:
        return self.vision_model(pixel_values).image_embeds

    def get_text_features(self, input_ids, **kwargs) -> torch.Tensor:
        return self.text_model(input_ids).text_embeds


class ImageBatch(dict):
    """What the processor returns: `.pixel_values` / `["pixel_values"]`, fp32 [n, 3, crop, crop] on the device."""

    @property
    def pixel_values(self) -> torch.Tensor:
        return self["pixel_values"]


class CLIPImageProcessor:
    """transformers' `CLIPImageProcessor` at its CLIP defaults, on the device: resize the shortest edge to `size` with PIL's antialiased bicubic filter
    (me_resample_u8, horizontal pass then vertical pass, bit for bit PIL's uint8 result), centre crop to `crop_size`, (x / 255 - mean) / std
    (me_crop_normalize).  Takes a uint8 [n, H, W, 3] tensor on either device, one numpy HWC image, or a list of images of one size."""

    def __init__(self, size=224, crop_size=224, image_mean=OPENAI_CLIP_MEAN, image_std=OPENAI_CLIP_STD, device: str = "cuda", **kwargs):
        pick = lambda v, key: int(v[key] if isinstance(v, Mapping) and key in v else (v["height"] if isinstance(v, Mapping) else v))   # noqa: E731
        self.size, self.crop_size = pick(size, "shortest_edge"), pick(crop_size, "height")
        self.image_mean, self.image_std = tuple(float(m) for m in image_mean), tuple(float(s) for s in image_std)
        if self.size <= 0 or self.crop_size <= 0 or self.crop_size > self.size:
            raise ValueError(f"CLIPImageProcessor: crop_size {self.crop_size} must be positive and at most size {self.size} (padding a crop is not built)")
        if len(self.image_mean) != 3 or len(self.image_std) != 3:
            raise ValueError("CLIPImageProcessor: image_mean and image_std have three entries")
        # the one pipeline that is built: every step on, bicubic, 1 / 255.  A configuration that asks for another one is refused, not processed this way.
        for k in ("do_resize", "do_center_crop", "do_rescale", "do_normalize"):
            if kwargs.get(k) is False:
                raise NotImplementedError(f"CLIPImageProcessor: {k}=False (resize, centre crop, rescale and normalise always run)")
        resample = kwargs.get("resample")
        if resample is not None and int(resample) != PIL_BICUBIC:
            raise NotImplementedError(f"CLIPImageProcessor: resample={resample!r} (only PIL's BICUBIC, {PIL_BICUBIC}, has a kernel: me_resample_u8)")
        factor = kwargs.get("rescale_factor")
        if factor is not None and float(factor) != 1 / 255:
            raise NotImplementedError(f"CLIPImageProcessor: rescale_factor={factor!r} (me_crop_normalize divides by 255)")
        self.device = torch.device(device)

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, subfolder=None, device="cuda", **kwargs) -> "CLIPImageProcessor":
        d = Path(pretrained_model_name_or_path) / subfolder if subfolder else Path(pretrained_model_name_or_path)
        cfg = json.loads((d / "preprocessor_config.json").read_text()) if (d / "preprocessor_config.json").exists() else {}
        keep = {k: cfg[k] for k in ("size", "crop_size", "image_mean", "image_std", "do_resize", "do_center_crop", "do_rescale", "do_normalize", "resample",
                                    "rescale_factor") if k in cfg}
        return cls(device=device, **keep)

    def output_size(self, H: int, W: int) -> Tuple[int, int]:
        """(oh, ow): the shortest edge becomes `size`, the other int(size * long / short)."""
        short, long = (W, H) if W <= H else (H, W)
        new_long = int(self.size * long / short)
        return (new_long, self.size) if W <= H else (self.size, new_long)

    def resize(self, images: torch.Tensor) -> torch.Tensor:
        """uint8 [n, H, W, 3] on the device -> uint8 [n, oh, ow, 3]: PIL's `resize((ow, oh), BICUBIC)`."""
        oh, ow = self.output_size(images.shape[1], images.shape[2])
        return ops.resample_u8(ops.resample_u8(images, ow, 0), oh, 1)

    def __call__(self, images=None, return_tensors="pt", **kwargs) -> ImageBatch:
        if images is None:
            raise ValueError("CLIPImageProcessor: no images")
        if return_tensors not in ("pt", None):
            raise NotImplementedError(f"CLIPImageProcessor: return_tensors={return_tensors!r} (only 'pt')")
        if isinstance(images, (list, tuple)):
            images = np.stack([im.cpu().numpy() if torch.is_tensor(im) else np.asarray(im) for im in images])
        x = torch.from_numpy(np.array(images)) if isinstance(images, np.ndarray) else torch.as_tensor(images)     # (a decoded image is often read-only: copied)
        if x.dim() == 3:
            x = x[None]
        if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3 or x.numel() == 0:
            raise ValueError(f"CLIPImageProcessor: expected uint8 images [n, H, W, 3] (or one [H, W, 3]), got {x.dtype} {tuple(x.shape)}")
        x = x.to(self.device).contiguous()
        r = self.resize(x)
        oh, ow = r.shape[1], r.shape[2]
        cs = self.crop_size
        return ImageBatch(pixel_values=ops.crop_normalize(r, (oh - cs) // 2, (ow - cs) // 2, (cs, cs), self.image_mean, self.image_std))

    preprocess = __call__
