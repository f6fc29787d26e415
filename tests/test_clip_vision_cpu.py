"""The CLIP image encoder, the text projection, the image processor and the CLIP metrics without a GPU: the launch graphs of models/clip.py on the emulated
ABI (tests/emu_clip_vision_ops.py) against transformers' recorded fp32 outputs (tests/golden/clip_vision.npz) and PIL's / CLIPImageProcessor's recorded
bytes (tests/golden/clip_image_processor.npz; generator tools/make_golden_clip_vision.py, weights and inputs tests/clip_vision_fixture.py); five deliberately
wrong emulations that must fail the fixture; key spellings, refusals, the from_pretrained round trips; the ABI table of include/motioned_vision.h."""
import ctypes
import json
import re
import types
from pathlib import Path

import numpy as np
import pytest
import torch

import clip_vision_fixture as fx
import emu_clip_vision_ops as emu_ops_v
from conftest import GOLD
from motioneditor_amd import metrics, vision
from motioneditor_amd.models import clip

ROOT = Path(__file__).resolve().parent.parent
TINY = dict(hidden_size=64, num_hidden_layers=1, num_attention_heads=1, intermediate_size=128, image_size=28, patch_size=14, projection_dim=16)   # 5 tokens
TINY_TEXT = dict(vocab_size=300, hidden_size=64, num_hidden_layers=1, num_attention_heads=1, intermediate_size=128, projection_dim=16)


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())


@pytest.fixture()
def emu(monkeypatch):
    monkeypatch.setattr(clip, "ops", emu_ops_v)
    monkeypatch.setattr(metrics, "ops", emu_ops_v)
    return emu_ops_v


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD / "clip_vision.npz")


def run_vision(cfg, suffix, gold):
    model = clip.CLIPVisionModelWithProjection(fx.vision_state_dict(cfg), cfg, device="cpu", dtype=torch.float32)
    out = model(torch.from_numpy(fx.pixel_values()))
    T = (224 // cfg["patch_size"]) ** 2 + 1
    assert out.image_embeds.dtype == torch.float32 and tuple(out.image_embeds.shape) == (2, 64) and tuple(out.last_hidden_state.shape) == (2, T, 256)
    return rel(out.image_embeds, gold["image_embeds" + suffix]), rel(out.last_hidden_state[:, [0, T - 1]], gold["hidden_rows" + suffix])


# ------------------------------------------------------------------ 1. launch graphs vs transformers
@pytest.mark.parametrize("cfg,suffix", [(fx.VISION, ""), (fx.VISION32, "32")], ids=["patch14-257tok", "patch32-50tok"])
def test_vision_graph_matches_transformers_fp32(emu, gold, cfg, suffix):
    e, h = run_vision(cfg, suffix, gold)
    floor = float(gold["fp16_floor" + suffix])
    print(f"emulated vision graph vs transformers fp32: image_embeds rel-L2 {e:.3e}, class / last rows {h:.3e} (2 x fp16_floor = {2 * floor:.3e})")
    assert e <= 2 * floor and h <= 2 * floor
    assert float(gold["qk_gain"]) == fx.QK_GAIN
    if not suffix:
        assert min(float(gold["moved_last_patch"]), float(gold["moved_swap"])) > 10 * floor


def test_text_projection_matches_transformers_fp32(emu, gold):
    model = clip.CLIPTextModelWithProjection(fx.text_state_dict(), dict(fx.TEXT, eos_token_id=fx.EOS), device="cpu", dtype=torch.float32)
    ids = torch.from_numpy(fx.text_ids())
    assert model.pooled_positions(ids).tolist() == [1, 7, 76]
    out = model(ids)
    e = rel(out.text_embeds, gold["text_embeds"])
    print(f"emulated text projection vs transformers fp32: rel-L2 {e:.3e} (2 x fp16_floor = {2 * float(gold['text_fp16_floor']):.3e})")
    assert tuple(out.text_embeds.shape) == (3, fx.TEXT_PROJECTION) and e <= 2 * float(gold["text_fp16_floor"])
    plain = clip.CLIPTextModel({k: v for k, v in fx.text_state_dict().items() if k != "text_projection.weight"}, fx.TEXT, device="cpu", dtype=torch.float32)
    assert torch.equal(out.last_hidden_state, plain(ids)[0]) and out[0] is out.text_embeds
    legacy = clip.CLIPTextModelWithProjection(fx.text_state_dict(), dict(fx.TEXT, eos_token_id=2), device="cpu", dtype=torch.float32)
    assert torch.equal(legacy(ids).text_embeds, out.text_embeds)          # eos is the largest id of the fixture: both pooling rules agree
    with pytest.raises(ValueError, match="end-of-text"):
        model(torch.zeros(1, 77, dtype=torch.int64))
    with pytest.raises(KeyError, match="text_projection.weight"):
        clip.CLIPTextModelWithProjection({k: v for k, v in fx.text_state_dict().items() if k != "text_projection.weight"}, fx.TEXT, device="cpu")


# ------------------------------------------------------------------ 2. five wrong emulations, each of which must fail the fixture
def _attn_last_key_dropped(q, k, v, *, heads, dh, n_seq, n, scale=None):
    sp = lambda t: t.float()[:n_seq * n, :heads * dh].reshape(n_seq, n, heads, dh).permute(0, 2, 1, 3)   # noqa: E731
    p = torch.softmax((sp(q) @ sp(k)[:, :, :n - 1].transpose(-1, -2)) * dh ** -0.5, dim=-1)
    return (p @ sp(v)[:, :, :n - 1]).permute(0, 2, 1, 3).reshape(n_seq * n, heads * dh).to(q.dtype)


def _attn_causal(q, k, v, *, heads, dh, n_seq, n, scale=None):
    return emu_ops_v.attention_causal(q, k, v, heads=heads, dh=dh, n_seq=n_seq, nq=n, scale=scale)


def _tokens_no_pos(patch_out, cls, pos, n, out=None):
    return emu_ops_v.vit_tokens(patch_out, cls, torch.zeros_like(pos), n)


def _tokens_class_last(patch_out, cls, pos, n, out=None):
    g2, C = patch_out.shape[0] // n, patch_out.shape[1]
    x = torch.cat([patch_out.float().reshape(n, g2, C), cls.float().reshape(1, 1, C).expand(n, 1, C)], dim=1) + pos.float().reshape(1, g2 + 1, C)
    return x.reshape(n * (g2 + 1), C).to(patch_out.dtype)


def _patch_rows_hwc(pixel_values, patch, out=None, dtype=None):
    n, c, S, _ = pixel_values.shape
    g, K = S // patch, c * patch * patch
    y = torch.zeros((n * g * g, (K + 7) // 8 * 8), dtype=torch.float32)
    y[:, :K] = pixel_values.reshape(n, c, g, patch, g, patch).permute(0, 2, 4, 3, 5, 1).reshape(n * g * g, K)
    return y


WRONG = {"last-key-dropped": ("attention_full", _attn_last_key_dropped), "causal-mask": ("attention_full", _attn_causal),
         "no-position-embedding": ("vit_tokens", _tokens_no_pos), "class-token-last": ("vit_tokens", _tokens_class_last),
         "patch-columns-py-px-c": ("patch_rows", _patch_rows_hwc)}


@pytest.mark.parametrize("name", sorted(WRONG))
def test_a_wrong_emulation_fails_the_fixture(monkeypatch, gold, name):
    fn_name, fn = WRONG[name]
    wrong = types.SimpleNamespace(**{k: v for k, v in vars(emu_ops_v).items() if not k.startswith("__")})
    setattr(wrong, fn_name, fn)
    monkeypatch.setattr(clip, "ops", wrong)
    e, h = run_vision(fx.VISION, "", gold)
    print(f"{name}: image_embeds rel-L2 {e:.3e}, rows {h:.3e} (bound {2 * float(gold['fp16_floor']):.3e})")
    assert e > 2 * float(gold["fp16_floor"]), f"the fixture does not see '{name}'"


# ------------------------------------------------------------------ 3. the image processor: PIL's and CLIPImageProcessor's bytes
def test_image_processor_emulation_is_bitwise_pil_and_transformers(emu):
    g = np.load(GOLD / "clip_image_processor.npz")
    proc = clip.CLIPImageProcessor(device="cpu")
    assert (proc.size, proc.crop_size, proc.image_mean, proc.image_std) == (224, 224, clip.OPENAI_CLIP_MEAN, clip.OPENAI_CLIP_STD)
    for i, (im, (H, W)) in enumerate(zip(fx.images(), fx.IMAGE_SIZES)):
        assert im.shape == (H, W, 3)
        oh, ow = proc.output_size(H, W)
        assert min(oh, ow) == 224 and max(oh, ow) == int(224 * max(H, W) / min(H, W))
        r = proc.resize(torch.from_numpy(im)[None])
        assert r.dtype == torch.uint8 and tuple(r.shape) == (1, oh, ow, 3)
        top, left = (oh - 224) // 2, (ow - 224) // 2
        want = g[f"resized_{i}"]
        diff = int((r[0, top:top + 224, left:left + 224].numpy() != want).sum())
        assert diff == 0, f"image {i} ({H} x {W}): {diff} bytes differ from PIL's resize"
    out = proc(images=fx.images()[0], return_tensors="pt")
    pv = out.pixel_values
    assert out["pixel_values"] is pv and pv.dtype == torch.float32 and tuple(pv.shape) == (1, 3, 224, 224)
    assert np.array_equal(pv[0].numpy().view(np.int32), g["pixel_values_0"].view(np.int32)), "pixel_values differ from CLIPImageProcessor's bits"
    both = proc([fx.images()[3], fx.images()[3]]).pixel_values
    assert tuple(both.shape) == (2, 3, 224, 224) and torch.equal(both[0], both[1])
    assert torch.equal(proc(torch.from_numpy(fx.images()[0])[None]).pixel_values, pv)
    with pytest.raises(ValueError, match="uint8"):
        proc(images=np.zeros((8, 8, 3), np.float32))
    with pytest.raises(ValueError, match="crop_size"):
        clip.CLIPImageProcessor(size=224, crop_size=256, device="cpu")
    assert clip.CLIPImageProcessor(size={"shortest_edge": 224}, crop_size={"height": 224, "width": 224}, device="cpu").crop_size == 224


def test_image_processor_refuses_a_configuration_it_would_not_follow(tmp_path):
    """CLIP's own preprocessor_config.json loads; one that asks for another pipeline is refused by the key's name, from the constructor and from a directory."""
    import json
    default = dict(crop_size={"height": 224, "width": 224}, do_center_crop=True, do_convert_rgb=True, do_normalize=True, do_rescale=True, do_resize=True,
                   image_mean=list(clip.OPENAI_CLIP_MEAN), image_std=list(clip.OPENAI_CLIP_STD), image_processor_type="CLIPImageProcessor", resample=3,
                   rescale_factor=0.00392156862745098, size={"shortest_edge": 224})
    (tmp_path / "preprocessor_config.json").write_text(json.dumps(default))
    proc = clip.CLIPImageProcessor.from_pretrained(tmp_path, device="cpu")
    assert (proc.size, proc.crop_size, proc.image_mean) == (224, 224, clip.OPENAI_CLIP_MEAN)
    for key, value in (("do_resize", False), ("do_center_crop", False), ("do_rescale", False), ("do_normalize", False), ("resample", 2), ("rescale_factor", 1 / 256)):
        with pytest.raises(NotImplementedError, match=key):
            clip.CLIPImageProcessor(device="cpu", **{key: value})
        (tmp_path / "preprocessor_config.json").write_text(json.dumps(dict(default, **{key: value})))
        with pytest.raises(NotImplementedError, match=key):
            clip.CLIPImageProcessor.from_pretrained(tmp_path, device="cpu")


def _tables_scalar(in_size, out_size):
    """The coefficient rule stated one output index at a time in Python floats (fp64)."""
    def cubic(x, a=-0.5):
        x = abs(x)
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * a
        return 0.0
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    rows = []
    for x in range(out_size):
        center = (x + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        w = [cubic((k - center + 0.5) * (1.0 / fs)) for k in range(xmin, xmax)]
        tot = 0.0
        for v in w:
            tot += v
        w = [v / tot for v in w]
        rows.append((xmin, [int(v * (1 << 22) + 0.5) if v >= 0 else int(v * (1 << 22) - 0.5) for v in w]))
    return rows


@pytest.mark.parametrize("in_size,out_size", [(48, 224), (512, 224), (224, 224), (113, 224), (300, 7)], ids=["upscale", "downscale", "identity", "odd-up", "steep-down"])
def test_coefficient_tables(in_size, out_size):
    bounds, coef, ksize = vision.resample_tables(in_size, out_size)
    assert bounds.dtype == coef.dtype == np.int32 and bounds.shape == (out_size, 2) and coef.shape == (out_size, ksize)
    assert ksize == int(np.ceil(2.0 * max(in_size / out_size, 1.0))) * 2 + 1
    for x, (xmin, w) in enumerate(_tables_scalar(in_size, out_size)):
        assert (int(bounds[x, 0]), int(bounds[x, 1])) == (xmin, len(w)) and coef[x, :len(w)].tolist() == w and not coef[x, len(w):].any(), x
        assert 0 <= xmin and xmin + len(w) <= in_size and 0 < len(w) <= ksize
        assert abs(sum(w) - (1 << 22)) <= len(w)                      # the weights sum to one up to their own rounding
    if in_size == out_size:   # the cubic is 1 at 0 and 0 at the other integers: resampling to the same size is the identity
        for x in range(out_size):
            row = dict(zip(range(int(bounds[x, 0]), int(bounds[x, 0]) + int(bounds[x, 1])), coef[x].tolist()))
            assert row.pop(x) == 1 << 22 and not any(row.values())
        im = torch.from_numpy(fx.images()[3])[None]
        assert torch.equal(emu_ops_v.resample_u8(emu_ops_v.resample_u8(im, 224, 0), 224, 1), im)


# ------------------------------------------------------------------ 4. keys, refusals, round trips
def tiny_sd(seed=5):
    from motioneditor_amd import synth
    return dict(synth.synth_state_dict(clip.clip_vision_schema(TINY), seed, salt="clip_vision."))


def test_vision_key_spellings_and_refusals(emu, monkeypatch):
    sd = tiny_sd()
    assert "pre_layrnorm.weight" in sd and "post_layernorm.bias" in sd and sd["embeddings.patch_embedding.weight"].shape == (64, 3, 14, 14)
    pv = torch.from_numpy(fx.pixel_values(3, 28))
    a = clip.CLIPVisionModelWithProjection(sd, TINY, device="cpu", dtype=torch.float32)
    pre = {("vision_model." + k if k != "visual_projection.weight" else k): v for k, v in sd.items()}
    pre["vision_model.embeddings.position_ids"] = np.arange(5)[None]
    b = clip.CLIPVisionModelWithProjection(pre, TINY, device="cpu", dtype=torch.float32)
    ya = a(pv)
    assert a.config.num_hidden_layers == 1 and a.config.patch_size == 14 and a.config.projection_dim == 16 and a.tokens == 5
    assert torch.equal(ya.image_embeds, b(pv).image_embeds) and tuple(ya.image_embeds.shape) == (3, 16) and tuple(ya.last_hidden_state.shape) == (3, 5, 64)
    assert torch.equal(a(types.SimpleNamespace(pixel_values=pv)).image_embeds, ya.image_embeds)
    assert a.requires_grad_(False) is a and a.eval() is a and a.device == torch.device("cpu")
    # image independence and batch permutation on the emulation
    assert torch.equal(a(pv[[2, 0, 1]]).image_embeds, ya.image_embeds[[2, 0, 1]])
    with pytest.raises(KeyError, match="pre_layernorm"):
        clip.CLIPVisionModelWithProjection(dict(sd, **{"pre_layernorm.weight": np.ones(64, np.float32)}), TINY, device="cpu")
    with pytest.raises(KeyError, match="post_layernorm.bias"):
        clip.CLIPVisionModelWithProjection({k: v for k, v in sd.items() if k != "post_layernorm.bias"}, TINY, device="cpu")
    with pytest.raises(KeyError, match="visual_projection.weight"):
        clip.CLIPVisionModelWithProjection({k: v for k, v in sd.items() if k != "visual_projection.weight"}, TINY, device="cpu")
    with pytest.raises(NotImplementedError, match="'gelu'"):
        clip.CLIPVisionModelWithProjection(sd, dict(TINY, hidden_act="gelu"), device="cpu")
    with pytest.raises(NotImplementedError, match="32"):
        clip.CLIPVisionModelWithProjection(sd, dict(TINY, num_attention_heads=2), device="cpu")
    with pytest.raises(ValueError, match="position table"):
        clip.CLIPVisionModelWithProjection(sd, dict(TINY, image_size=42), device="cpu")

    def boom(*args, **kw):
        raise AssertionError("launched before the arguments were checked")
    for name in ("patch_rows", "gemm", "vit_tokens", "layernorm", "attention_full", "quick_gelu"):
        monkeypatch.setattr(emu_ops_v, name, boom)
    with pytest.raises(ValueError, match="image size 28"):
        a(torch.zeros(1, 3, 42, 42))
    with pytest.raises(ValueError, match="fp32"):
        a(torch.zeros(1, 3, 28, 28, dtype=torch.float16))
    from motioneditor_amd import plan
    monkeypatch.setattr(plan, "ACTIVE", object())
    with pytest.raises(RuntimeError, match="being recorded"):
        a(pv)


def test_wrappers_refuse_while_a_plan_records_and_check_arguments(monkeypatch):
    from motioneditor_amd import ops, plan
    for name in ("attention_full", "patch_rows", "vit_tokens", "resample_u8", "crop_normalize", "cosine_rows"):
        assert getattr(ops, name) is getattr(vision, name)
    x = torch.zeros(4, 8)
    with pytest.raises(ValueError, match="CUDA fp32"):
        ops.cosine_rows(x, x)
    with pytest.raises(ValueError, match="CUDA uint8"):
        ops.resample_u8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), 8, 0)
    with pytest.raises(ValueError, match="CUDA uint8"):
        ops.crop_normalize(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), 0, 0, (2, 2), clip.OPENAI_CLIP_MEAN, clip.OPENAI_CLIP_STD)
    with pytest.raises(ValueError, match="CUDA fp32"):
        ops.patch_rows(torch.zeros(1, 3, 28, 28), 14)
    with pytest.raises(ValueError, match="CUDA fp16"):
        ops.attention_full(x, x, x, heads=1, dh=64, n_seq=1, n=4)
    with pytest.raises(ValueError, match="CUDA fp16"):
        ops.vit_tokens(x, x[0], x, 1)
    monkeypatch.setattr(plan, "ACTIVE", object())
    for call in (lambda: ops.cosine_rows(x, x), lambda: ops.resample_u8(x, 8, 0), lambda: ops.crop_normalize(x, 0, 0, (2, 2), (0,) * 3, (1,) * 3),
                 lambda: ops.patch_rows(x, 14), lambda: ops.attention_full(x, x, x, heads=1, dh=64, n_seq=1, n=4), lambda: ops.vit_tokens(x, x, x, 1)):
        with pytest.raises(RuntimeError, match="being recorded"):
            call()


def test_from_pretrained_round_trips(emu, tmp_path):
    from safetensors.torch import save_file
    from motioneditor_amd import synth
    vsd = tiny_sd()
    tschema = clip.clip_text_schema(TINY_TEXT)
    tschema["text_projection.weight"] = (16, 64)
    tsd = dict(synth.synth_state_dict(tschema, 5, salt="clip."))
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v))   # noqa: E731
    vis = {("vision_model." + k if k != "visual_projection.weight" else k): t(v) for k, v in vsd.items()}
    txt = {("text_model." + k if k != "text_projection.weight" else k): t(v) for k, v in tsd.items()}
    # an image_encoder/ folder as diffusers pipelines hold it
    ie = tmp_path / "sd" / "image_encoder"
    ie.mkdir(parents=True)
    (ie / "config.json").write_text(json.dumps(dict(clip.DEFAULT_VISION_CONFIG, **TINY, architectures=["CLIPVisionModelWithProjection"])))
    save_file(vis, str(ie / "model.safetensors"))
    pv = torch.from_numpy(fx.pixel_values(2, 28))
    direct = clip.CLIPVisionModelWithProjection(vsd, TINY, device="cpu", dtype=torch.float32)
    enc = clip.CLIPVisionModelWithProjection.from_pretrained(tmp_path / "sd", subfolder="image_encoder", device="cpu")
    assert enc.config.image_size == 28 and enc.config.num_attention_heads == 1 and enc.dtype == torch.float16
    enc.P = type(enc.P)(enc.P.state, "cpu", dtype=torch.float32)      # (the emulated ABI computes in fp32)
    assert torch.equal(enc(pv).image_embeds, direct(pv).image_embeds)
    # one CLIP checkpoint directory: both towers, both projections, logit_scale
    cd = tmp_path / "clip"
    cd.mkdir()
    (cd / "config.json").write_text(json.dumps(dict(model_type="clip", projection_dim=16, text_config=dict(clip.DEFAULT_CONFIG, **TINY_TEXT, eos_token_id=299),
                                                    vision_config=dict(clip.DEFAULT_VISION_CONFIG, **TINY))))
    (cd / "preprocessor_config.json").write_text(json.dumps(dict(size={"shortest_edge": 28}, crop_size={"height": 28, "width": 28}, image_mean=[0.5] * 3, image_std=[0.25] * 3)))
    save_file(dict(vis, **txt, logit_scale=torch.tensor(4.6)), str(cd / "model.safetensors"))
    model = clip.CLIPModel.from_pretrained(cd, device="cpu")
    for tower in (model.text_model, model.vision_model):
        tower.P = type(tower.P)(tower.P.state, "cpu", dtype=torch.float32)
    assert model.text_model.config.eos_token_id == 299 and model.text_model.config.projection_dim == 16 and model.vision_model.config.image_size == 28
    assert torch.equal(model.get_image_features(pv), direct(pv).image_embeds)
    ids = torch.full((2, 77), 299, dtype=torch.int64)
    ids[:, 0], ids[1, 1:4] = 298, torch.tensor([5, 6, 7])
    want = clip.CLIPTextModelWithProjection(tsd, dict(TINY_TEXT, eos_token_id=299), device="cpu", dtype=torch.float32)(ids).text_embeds
    assert torch.equal(model.get_text_features(ids), want) and tuple(want.shape) == (2, 16)
    proc = clip.CLIPImageProcessor.from_pretrained(cd, device="cpu")
    assert (proc.size, proc.crop_size, proc.image_mean, proc.image_std) == (28, 28, (0.5,) * 3, (0.25,) * 3)
    # the towers read their half of the whole checkpoint as well; SD-1.5's text_encoder/ (no text_projection) is refused by name
    alone = clip.CLIPVisionModelWithProjection.from_pretrained(cd, subfolder=None, device="cpu")
    assert alone.config.projection_dim == 16 and alone.config.image_size == 28
    save_file({k: v for k, v in txt.items() if k != "text_projection.weight"}, str(tmp_path / "model.safetensors"))
    with pytest.raises(KeyError, match="text_projection.weight"):
        clip.CLIPTextModelWithProjection.from_pretrained(tmp_path, subfolder=None, device="cpu")
    save_file(dict(vis, **txt, extra=torch.zeros(1)), str(cd / "model.safetensors"))
    with pytest.raises(KeyError, match="extra"):
        clip.CLIPModel.from_pretrained(cd, device="cpu")


# ------------------------------------------------------------------ 5. metrics
def test_metrics_match_an_fp64_restatement(emu):
    g = np.random.Generator(np.random.Philox(key=3))
    e = g.standard_normal((8, 64)).astype(np.float32) + 0.5
    t = g.standard_normal(64).astype(np.float32)
    e64, t64 = e.astype(np.float64), t.astype(np.float64)
    unit = lambda a: a / np.linalg.norm(a, axis=-1, keepdims=True)   # noqa: E731
    fc = float((unit(e64[:-1]) * unit(e64[1:])).sum(-1).mean())
    ta = float((unit(e64) @ unit(t64)).mean())
    assert abs(metrics.frame_consistency(torch.from_numpy(e)) - fc) < 1e-6
    assert abs(metrics.text_alignment(torch.from_numpy(e), torch.from_numpy(t)) - ta) < 1e-6
    assert abs(metrics.text_alignment(torch.from_numpy(e), torch.from_numpy(t)[None]) - ta) < 1e-6
    assert abs(metrics.frame_consistency(torch.from_numpy(np.stack([e[0], 3.0 * e[0]]))) - 1.0) < 1e-6
    with pytest.raises(ValueError, match="two frames"):
        metrics.frame_consistency(torch.from_numpy(e[:1]))
    with pytest.raises(ValueError, match="one text embedding"):
        metrics.text_alignment(torch.from_numpy(e), torch.from_numpy(e[:2]))


def test_clip_metrics_scores_the_frames_a_gif_holds(emu):
    from motioneditor_amd import tokenizer as tk
    gold = json.loads((GOLD / "clip_tokenizer.json").read_text())
    tok = tk.CLIPTokenizer(vocab=gold["vocab"], merges=gold["merges"])
    tcfg = dict(TINY_TEXT, vocab_size=len(tok), eos_token_id=tok.eos_token_id)
    model = clip.CLIPModel.from_synthetic("cpu", 5, tcfg, TINY)
    for tower in (model.text_model, model.vision_model):
        tower.P = type(tower.P)(tower.P.state, "cpu", dtype=torch.float32)
    proc = clip.CLIPImageProcessor(size=28, crop_size=28, device="cpu")
    video = torch.from_numpy(np.random.Generator(np.random.Philox(key=4)).random((1, 3, 4, 20, 24), dtype=np.float32))
    out = metrics.clip_metrics(video, "a girl is dancing", model, proc, tok)
    assert sorted(out) == ["frame_consistency", "text_alignment"] and all(np.isfinite(v) and -1 <= v <= 1 for v in out.values())
    frames = (video[0].permute(1, 2, 3, 0) * 255).to(torch.uint8)            # util.save_videos_grid's quantisation, b = 1
    emb = model.get_image_features(proc(images=frames).pixel_values)
    ids = tok(["a girl is dancing"], padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
    assert out["frame_consistency"] == metrics.frame_consistency(emb) and out["text_alignment"] == metrics.text_alignment(emb, model.get_text_features(ids))
    assert sorted(metrics.clip_metrics(video, None, model, proc)) == ["frame_consistency"]


def test_dataset_image_embeddings(emu, tmp_path):
    from PIL import Image
    from motioneditor_amd.data.dataset import VideoDataset
    (tmp_path / "images").mkdir()
    for i in range(3):
        Image.fromarray(fx.images()[2] // (i + 1)).save(tmp_path / "images" / f"{i:04d}.png")
    ds = VideoDataset(str(tmp_path), "a girl", width=32, height=32, n_sample_frames=2, video_suffix=".png", device="cpu")
    with pytest.raises(NotImplementedError, match="no CLIP image encoder"):
        ds.preprocess_img_embedding(None, None)
    enc = clip.CLIPVisionModelWithProjection(tiny_sd(), TINY, device="cpu", dtype=torch.float32)
    proc = clip.CLIPImageProcessor(size=28, crop_size=28, device="cpu")
    ds.preprocess_img_embedding(proc, enc)
    assert len(ds.source_img_embeddings) == 3 and all(tuple(e.shape) == (16,) and e.dtype == torch.float32 for e in ds.source_img_embeddings)
    # the folder goes through as one batch: bit for bit the batched call (the device kernels are batch-invariant; torch's CPU matmul, which the emulation
    # uses, is so only to fp32 rounding, hence the second comparison with a call per frame)
    batch = enc(proc([fx.images()[2] // (i + 1) for i in range(3)]).pixel_values).image_embeds
    assert all(torch.equal(e, b) for e, b in zip(ds.source_img_embeddings, batch))
    want = enc(proc(images=fx.images()[2] // 2).pixel_values).image_embeds[0]
    torch.testing.assert_close(ds.source_img_embeddings[1], want, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------ 6. the ABI table of include/motioned_vision.h
LAUNCHING = {"me_attn_full", "me_patch_rows", "me_vit_tokens", "me_resample_u8", "me_crop_normalize", "me_cosine_rows"}


def test_vision_symbols_are_declared_exported_and_apart_from_the_other_tables():
    from motioneditor_amd import build, capi
    build.build_lib(verbose=False)
    assert "clip_vision.hip" in build.SOURCES and "clip_vision.hip" not in build.EXTRA_FLAGS          # the library's default flags
    assert "#pragma clang fp contract(off)" in (build.CSRC / "clip_vision.hip").read_text()             # (the normalisation's three roundings)
    others = set(capi.SYMBOLS) | set(capi.IO_SYMBOLS) | set(capi.TUNE_SYMBOLS) | set(capi.LONG_SYMBOLS) | set(capi.PROBE_SYMBOLS)
    assert not set(capi.VISION_SYMBOLS) & others
    assert set(capi.IO_SYMBOLS) == {"me_image_resize", "me_video_grid_u8"} and set(capi.PROBE_SYMBOLS) == {"me_attn_probs"}
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "motioned_vision.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(me_[a-z0-9_]+)\s*\(", header))
    assert declared == set(capi.VISION_SYMBOLS) == LAUNCHING | {"me_attn_full_nmax"}
    L = ctypes.CDLL(str(capi.LIB_PATH))
    for name in declared:
        getattr(L, name)
    bound = capi.lib()
    for name, (res, args) in capi.VISION_SYMBOLS.items():
        assert getattr(bound, name).argtypes == args and getattr(bound, name).restype is res
        n_args = len(re.search(name + r"\s*\((.*?)\)\s*;", header, re.S).group(1).split(",")) if args else 0
        assert n_args == len(args), name
    assert bound.me_abi_version() == capi.ABI_VERSION == 9       # ABI 9 stays: no existing struct or symbol changed
    for other in ("motioned.h", "motioned_io.h", "motioned_tune.h", "motioned_long.h", "motioned_probe.h"):
        text = (ROOT / "include" / other).read_text()
        assert not any(name in text for name in declared)
    nmax = bound.me_attn_full_nmax()
    assert nmax >= 257 and nmax == int(re.search(r"#define ME_ATTN_FULL_NMAX (\d+)", header).group(1)) == vision.attn_full_nmax()


def test_every_launching_vision_symbol_is_named_by_a_guard_case():
    from motioneditor_amd import capi
    import test_guard_vision_gpu
    guarded = set()
    for syms in test_guard_vision_gpu.GUARDED.values():
        guarded |= set(syms)
    assert guarded == LAUNCHING == set(capi.VISION_SYMBOLS) - {"me_attn_full_nmax"}


def test_entries_refuse_on_the_host_what_they_do_not_serve():
    from motioneditor_amd import capi
    L, P, f = capi.lib(), 4096, ctypes.c_float      # P is never dereferenced: every call below is refused before a launch
    nmax = L.me_attn_full_nmax()
    attn = lambda **o: L.me_attn_full(*[o.get(k, d) for k, d in (("O", P), ("ldo", 1024), ("Q", P), ("ldq", 3072), ("K", P), ("ldk", 3072), ("V", P), ("ldv", 3072),   # noqa: E731
                                                                ("n_seq", 2), ("heads", 16), ("dh", 64), ("n", 257), ("scale", f(0.125)), ("stream", None))])
    for bad, word in ((dict(n=nmax + 1), b"nq = nk <="), (dict(dh=40), b"dh = 64"), (dict(n=0), b"bad arguments"), (dict(ldq=3076), b"multiples of 8"),
                      (dict(ldo=1016), b">= heads * dh"), (dict(Q=P + 8), b"16-byte"), (dict(V=None), b"bad arguments"), (dict(scale=f(0.0)), b"bad arguments")):
        assert attn(**bad) == capi.ME_EINVAL and word in L.me_last_error(), (bad, L.me_last_error())
    assert L.me_patch_rows(P, 592, P, 3 * 224 * 224, 224 * 224, 224, 1, 224, 15, None) == capi.ME_EINVAL and b"multiple of patch" in L.me_last_error()
    assert L.me_patch_rows(P, 588, P, 3 * 224 * 224, 224 * 224, 224, 1, 224, 14, None) == capi.ME_EINVAL and b"Kpad" in L.me_last_error()
    assert L.me_patch_rows(P, 592, P, 3 * 224 * 224, 224 * 224, 223, 1, 224, 14, None) == capi.ME_EINVAL
    assert L.me_vit_tokens(P, 1024, P, 1024, P, P, 1, 256, 1020, None) == capi.ME_EINVAL and b"multiples of 8" in L.me_last_error()
    assert L.me_vit_tokens(P, 1024, P, 512, P, P, 1, 256, 1024, None) == capi.ME_EINVAL
    assert L.me_resample_u8(P, 224 * 96 * 3, 224 * 3, P, 96 * 128 * 3, 128 * 3, 1, 96, 128, 3, 224, 2, P, P, 5, None) == capi.ME_EINVAL and b"axis" in L.me_last_error()
    assert L.me_resample_u8(P, 224 * 96 * 3, 224 * 3, P, 96 * 128 * 3, 128 * 3, 1, 96, 128, 2, 224, 0, P, P, 5, None) == capi.ME_EINVAL and b"C must be" in L.me_last_error()
    assert L.me_resample_u8(P, 224 * 96 * 3, 223 * 3, P, 96 * 128 * 3, 128 * 3, 1, 96, 128, 3, 224, 0, P, P, 5, None) == capi.ME_EINVAL and b"strides" in L.me_last_error()
    crop = lambda top, std0: L.me_crop_normalize(P, 3 * 224 * 224, 224 * 224, 224, P, 224 * 298 * 3, 298 * 3, 1, 224, 298, top, 37, 224, 224,   # noqa: E731
                                                 f(0.5), f(0.5), f(0.5), f(std0), f(0.25), f(0.25), None)
    assert crop(1, 0.25) == capi.ME_EINVAL and b"inside the image" in L.me_last_error()
    assert crop(0, 0.0) == capi.ME_EINVAL and b"non-zero" in L.me_last_error()
    assert L.me_cosine_rows(P, P, 32, P, 0, 4, 64, None) == capi.ME_EINVAL and b"lda >= C" in L.me_last_error()
    assert L.me_cosine_rows(P, P, 64, P, 32, 4, 64, None) == capi.ME_EINVAL
    assert L.me_cosine_rows(P, P, 64, None, 0, 4, 64, None) == capi.ME_EINVAL
