"""Generate tests/golden/clip_vision.npz and tests/golden/clip_image_processor.npz: what `transformers` (CLIPVisionModelWithProjection,
CLIPTextModelWithProjection, CLIPImageProcessor) and PIL compute for the inputs the CLIP vision tests feed `motioneditor_amd.models.clip`.

Test infrastructure, not product code, run by hand on a machine that has `transformers` and PIL; no test imports `transformers`.

clip_vision.npz           the weights and inputs of tests/clip_vision_fixture.py, fp32 on the CPU.  For the patch-14 configuration (257 tokens) and the
                          patch-32 one (50 tokens, keys with the suffix `32`): image_embeds [2, 64]; hidden_rows [2, 2, 256], the class row and the last
                          token's row of last_hidden_state; fp16_floor, rel-L2 of image_embeds of the same model evaluated with .half() against fp32.
                          text_embeds [3, 64] of CLIPTextModelWithProjection for fixture.text_ids(), text_fp16_floor alike.
                          Asserted before writing (patch 14): changing image 1 leaves image 0's outputs bitwise unchanged; altering only the LAST patch
                          (token 256) moves image 0's class embedding by more than 10 x fp16_floor; swapping the pixel blocks of two patches moves
                          image_embeds by more than 10 x fp16_floor.  The three figures are stored too (moved_*).
clip_image_processor.npz  for the four images of fixture.images(): resized_i, PIL's `resize((ow, oh), BICUBIC)` of image i, centre-cropped to 224 x 224
                          (uint8 HWC); pixel_values_0, CLIPImageProcessor's output for image 0.  Asserted before writing: the product's host tables and
                          the integer emulation (tests/emu_clip_vision_ops.py) reproduce every array bit for bit.

Usage:  python tools/make_golden_clip_vision.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import clip_vision_fixture as fx  # noqa: E402

GOLD = ROOT / "tests" / "golden"
rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())   # noqa: E731


def _load(model, sd, prefix, top):
    own = [k for k in model.state_dict() if not k.endswith("position_ids")]
    pre = prefix if any(k.startswith(prefix) for k in own) else ""
    missing, unexpected = model.load_state_dict({(k if k in top else pre + k): torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.endswith("position_ids") for k in missing), (missing, unexpected)
    return model.eval()


def vision_outputs(cfg, pv):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    c = CLIPVisionConfig(**{k: cfg[k] for k in ("hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size", "image_size", "patch_size",
                                                   "num_channels", "projection_dim", "hidden_act", "layer_norm_eps")})
    model = _load(CLIPVisionModelWithProjection(c), fx.vision_state_dict(cfg), "vision_model.", ("visual_projection.weight",))
    run = lambda m, x: m(pixel_values=x)   # noqa: E731
    with torch.no_grad():
        o = run(model, torch.from_numpy(pv))
        extra = []
        T = (cfg["image_size"] // cfg["patch_size"]) ** 2 + 1
        if cfg["patch_size"] == 14:
            ps, g = 14, 16
            other = pv.copy()
            other[1] = other[1][:, ::-1].copy()
            last = pv.copy()
            last[0, :, -ps:, -ps:] = last[0, :, -ps:, -ps:][:, ::-1, ::-1] * -1.5 + 0.5
            swap = pv.copy()
            a, b = (3 * ps, 5 * ps), (11 * ps, 9 * ps)
            swap[0, :, a[0]:a[0] + ps, a[1]:a[1] + ps] = pv[0, :, b[0]:b[0] + ps, b[1]:b[1] + ps]
            swap[0, :, b[0]:b[0] + ps, b[1]:b[1] + ps] = pv[0, :, a[0]:a[0] + ps, a[1]:a[1] + ps]
            extra = [run(model, torch.from_numpy(t)) for t in (other, last, swap)]
        o16 = run(model.half(), torch.from_numpy(pv).half())
    floor = rel(o16.image_embeds.float(), o.image_embeds)
    assert o.last_hidden_state.shape[1] == T
    out = dict(image_embeds=o.image_embeds.numpy(), hidden_rows=o.last_hidden_state[:, [0, T - 1]].numpy(), fp16_floor=np.float64(floor))
    print(f"patch {cfg['patch_size']}: {T} tokens, fp16_floor {floor:.3e}, |image_embeds| max {float(o.image_embeds.abs().max()):.2f}")
    if extra:
        other, last, swap = extra
        assert torch.equal(other.image_embeds[0], o.image_embeds[0]) and torch.equal(other.last_hidden_state[0], o.last_hidden_state[0]), "image 1 reached image 0"
        assert not torch.equal(other.image_embeds[1], o.image_embeds[1])
        m_last = rel(last.image_embeds[0], o.image_embeds[0])
        m_swap = rel(swap.image_embeds[0], o.image_embeds[0])
        print(f"    QK_GAIN {fx.QK_GAIN}: last patch altered -> class embedding moved by {m_last:.3e}; two patches swapped -> {m_swap:.3e}  (10 x floor = {10 * floor:.3e})")
        assert m_last > 10 * floor and m_swap > 10 * floor, (m_last, m_swap, floor)
        out.update(moved_last_patch=np.float64(m_last), moved_swap=np.float64(m_swap))
    return out


def text_outputs():
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    c = fx.TEXT
    cfg = CLIPTextConfig(vocab_size=c["vocab_size"], hidden_size=c["hidden_size"], intermediate_size=c["intermediate_size"], num_hidden_layers=c["num_hidden_layers"],
                         num_attention_heads=c["num_attention_heads"], max_position_embeddings=c["max_position_embeddings"], hidden_act=c["hidden_act"],
                         layer_norm_eps=c["layer_norm_eps"], projection_dim=fx.TEXT_PROJECTION, bos_token_id=c["vocab_size"] - 2, eos_token_id=fx.EOS, pad_token_id=fx.EOS)
    model = _load(CLIPTextModelWithProjection(cfg), fx.text_state_dict(), "text_model.", ("text_projection.weight",))
    ids = torch.from_numpy(fx.text_ids())
    with torch.no_grad():
        y = model(ids).text_embeds
        y16 = model.half()(ids).text_embeds.float()
    print(f"text: fp16_floor {rel(y16, y):.3e}")
    return dict(text_embeds=y.numpy(), text_fp16_floor=np.float64(rel(y16, y)))


def make_vision_fixture() -> None:
    pv = fx.pixel_values()
    out = vision_outputs(fx.VISION, pv)
    out.update({k + "32": v for k, v in vision_outputs(fx.VISION32, pv).items()})
    out.update(text_outputs())
    out["qk_gain"] = np.float64(fx.QK_GAIN)
    path = GOLD / "clip_vision.npz"
    np.savez_compressed(path, **out)
    print(path, "written:", path.stat().st_size, "bytes")
    assert path.stat().st_size < (1 << 20)


def make_processor_fixture() -> None:
    from PIL import Image
    import emu_clip_vision_ops as emu
    from motioneditor_amd.models import clip
    import transformers
    proc_cls = getattr(transformers, "CLIPImageProcessorPil", None) or transformers.CLIPImageProcessor
    try:
        hf = proc_cls(use_fast=False)
    except TypeError:
        hf = proc_cls()
    print("processor:", type(hf).__name__)
    own = clip.CLIPImageProcessor(device="cpu")
    out = {}
    for i, im in enumerate(fx.images()):
        oh, ow = own.output_size(*im.shape[:2])
        r = np.asarray(Image.fromarray(im).resize((ow, oh), Image.BICUBIC))
        got = emu.resample_u8(emu.resample_u8(torch.from_numpy(im)[None], ow, 0), oh, 1)[0].numpy()
        assert got.shape == r.shape and np.array_equal(got, r), f"image {i}: {int((got != r).sum())} pixels differ from PIL"
        top, left = (oh - 224) // 2, (ow - 224) // 2
        out[f"resized_{i}"] = np.ascontiguousarray(r[top:top + 224, left:left + 224])
        want = np.asarray(hf(images=im, return_tensors="np")["pixel_values"])[0]
        mine = emu.crop_normalize(torch.from_numpy(r)[None], top, left, (224, 224), clip.OPENAI_CLIP_MEAN, clip.OPENAI_CLIP_STD)[0].numpy()
        assert want.dtype == np.float32 and np.array_equal(mine.view(np.int32), want.view(np.int32)), \
            f"image {i}: pixel_values differ in {int((mine != want).sum())} elements, max {float(np.abs(mine - want).max()):.3e}"
        if i == 0:
            out["pixel_values_0"] = want
        print(f"image {i}: {im.shape[:2]} -> {(oh, ow)}: PIL and CLIPImageProcessor reproduced bit for bit")
    path = GOLD / "clip_image_processor.npz"
    np.savez_compressed(path, **out)
    print(path, "written:", path.stat().st_size, "bytes")
    assert path.stat().st_size < (1 << 20)


if __name__ == "__main__":
    make_processor_fixture()
    make_vision_fixture()
