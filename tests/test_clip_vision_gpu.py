"""The native CLIP image encoder, image processor and CLIP metrics on a real MI355X: the six kernels of csrc/clip_vision.hip against their emulation
(tests/emu_clip_vision_ops.py), the whole vision tower and the text projection against transformers' recorded fp32 outputs (tests/golden/clip_vision.npz),
the image processor against PIL's and CLIPImageProcessor's recorded bytes (tests/golden/clip_image_processor.npz), bitwise reproducibility, batch
permutation and image independence, a two-layer tower at ViT-L/14's widths, the metrics of a synthetic video and examples/run_edit.py --metrics.

Measured on an MI355X (profiles/clip_vision_parity.jsonl): vision tower vs transformers fp32 at 257 tokens rel-L2 2.69e-3 (bound 2 x fp16_floor = 4.82e-3), at
50 tokens 2.77e-3 (6.32e-3), text projection 2.95e-3 (5.74e-3); me_attn_full vs its emulation rel-L2 9.0e-5 ... 1.4e-4 on the eight shapes."""
import json
import sys

import numpy as np
import pytest
import torch

import clip_vision_fixture as fx
import emu_clip_vision_ops as emu
from conftest import GOLD, ROOT

pytestmark = pytest.mark.gpu

# The defaults of check() in tests/test_kernels_gpu.py (fp16 storage, fp32 accumulation).  Restated, not chosen here.
REL_L2 = 2e-3
MAX_REL = 2e-2


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the HIP library is the only compute path")
    from motioneditor_amd import capi, ops as _ops
    capi.lib()
    return _ops


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD / "clip_vision.npz")


@pytest.fixture(scope="module")
def tower(ops):
    from motioneditor_amd.models.clip import CLIPVisionModelWithProjection
    return CLIPVisionModelWithProjection(fx.vision_state_dict(), fx.VISION, device="cuda")


@pytest.fixture(scope="module")
def pv():
    return torch.from_numpy(fx.pixel_values()).cuda()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.float16)


def errs(got, want):
    got, want = got.detach().float().cpu().double(), want.detach().float().cpu().double()
    assert got.shape == want.shape and torch.isfinite(got).all()
    return float((got - want).norm() / want.norm().clamp_min(1e-30)), float((got - want).abs().max() / want.abs().mean().clamp_min(1e-30))


def rel(a, b):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return float((a - b).norm() / b.norm())


def nmax():
    from motioneditor_amd import vision
    return vision.attn_full_nmax()


# ------------------------------------------------------------------ 1. me_attn_full
ATTN_SHAPES = [(1, 16, 257), (3, 12, 50), (2, 2, 197), (2, 4, 1), (1, 2, 16), (1, 2, 17), (1, 2, 33), (2, 16, "NMAX")]


@pytest.mark.parametrize("n_seq,heads,n", ATTN_SHAPES, ids=[f"{s}x{h}x{n}" for s, h, n in ATTN_SHAPES])
def test_attention_full_matches_the_emulation(ops, n_seq, heads, n):
    n = nmax() if n == "NMAX" else n
    assert nmax() >= 257
    C = heads * 64
    qkv = rnd(n_seq * n, 3 * C, seed=n + heads)
    qkv[:, :2 * C] *= 3          # q, k x 3: logits of std ~ 9, a peaked softmax (as test_attn_causal does)
    d = qkv.cuda()
    q, k, v = d[:, :C], d[:, C:2 * C], d[:, 2 * C:]
    got = ops.attention_full(q, k, v, heads=heads, dh=64, n_seq=n_seq, n=n)
    want = emu.attention_full(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], heads=heads, dh=64, n_seq=n_seq, n=n)
    r, m = errs(got, want)
    print(f"attention_full {n_seq} x {heads} x {n}: rel-L2 {r:.3e}, max/mean {m:.3e}")
    assert r <= REL_L2 and m <= MAX_REL
    assert torch.equal(ops.attention_full(q, k, v, heads=heads, dh=64, n_seq=n_seq, n=n), got)        # two runs, bitwise
    if n > 1:
        # The LAST key / value row of sequence 0 reaches every query row of that sequence and no other sequence (at n_seq = 1, 257 keys included -- key 256
        # alone in tile 16 -- there is no other sequence and the second half holds of nothing).  On un-scaled q / k (logits of std 1, so
        # that no weight underflows in the fp16 P operand) the last key becomes 0 -- logit exactly 0 for every query, weight >= e^-6 / (n e^0.5) ~ 6e-6 --
        # and its value 2000: every output element moves by >= 1e-2, far above an fp16 ulp of the O(0.1) outputs.
        base = rnd(n_seq * n, 3 * C, seed=n + heads).cuda()
        d2 = base.clone()
        d2[n - 1, C:2 * C] = 0.0
        d2[n - 1, 2 * C:] = 2000.0
        run = lambda t: ops.attention_full(t[:, :C], t[:, C:2 * C], t[:, 2 * C:], heads=heads, dh=64, n_seq=n_seq, n=n)   # noqa: E731
        o1, o2 = run(base), run(d2)
        changed = (o2[:n] != o1[:n]).reshape(n, heads, 64).all(dim=2)
        assert bool(changed.all()), f"{int((~changed).sum())} (query, head) pairs of sequence 0 do not see the last key"
        assert torch.equal(o2[n:], o1[n:]) and torch.isfinite(o2).all()


def test_attention_full_refuses_what_it_does_not_serve(ops):
    n = nmax() + 1
    x = rnd(n, 3 * 64).cuda()
    with pytest.raises(ValueError, match="nq = nk <="):
        ops.attention_full(x[:, :64], x[:, 64:128], x[:, 128:], heads=1, dh=64, n_seq=1, n=n)
    y = rnd(50, 3 * 80).cuda()
    with pytest.raises(ValueError, match="dh = 64"):
        ops.attention_full(y[:, :80], y[:, 80:160], y[:, 160:], heads=2, dh=40, n_seq=1, n=50)


# ------------------------------------------------------------------ 2. me_patch_rows, me_vit_tokens: one rounding
@pytest.mark.parametrize("n,S,patch", [(2, 224, 14), (1, 224, 32), (3, 28, 14)])
def test_patch_rows_is_exact_to_one_rounding(ops, n, S, patch):
    x = torch.from_numpy(fx.pixel_values(n, S))
    got = ops.patch_rows(x.cuda(), patch).cpu()
    K, kpad = 3 * patch * patch, (3 * patch * patch + 7) // 8 * 8
    assert tuple(got.shape) == (n * (S // patch) ** 2, kpad) and got.dtype == torch.float16
    assert torch.equal(got, emu.patch_rows(x, patch, dtype=torch.float16)) and not got[:, K:].any()
    view = torch.zeros(n, 3, S + 3, S + 5).cuda()          # a view inside a larger allocation
    view[:, :, 2:2 + S, 1:1 + S] = x.cuda()
    assert torch.equal(ops.patch_rows(view[:, :, 2:2 + S, 1:1 + S], patch).cpu(), got)


@pytest.mark.parametrize("n,g2,C", [(2, 256, 1024), (3, 49, 256), (1, 4, 64)])
def test_vit_tokens_is_exact_to_one_rounding(ops, n, g2, C):
    po, cls, pos = rnd(n * g2, C, seed=1), rnd(C, seed=2), rnd(g2 + 1, C, seed=3)
    got = ops.vit_tokens(po.cuda(), cls.cuda(), pos.cuda(), n).cpu()
    assert torch.equal(got, emu.vit_tokens(po, cls, pos, n)) and tuple(got.shape) == (n * (g2 + 1), C)


# ------------------------------------------------------------------ 3. the image processor: bitwise PIL / CLIPImageProcessor
def test_image_processor_is_bitwise_pil_and_transformers(ops):
    from motioneditor_amd.models.clip import CLIPImageProcessor
    g = np.load(GOLD / "clip_image_processor.npz")
    proc = CLIPImageProcessor()
    for i, im in enumerate(fx.images()):
        r = proc.resize(torch.from_numpy(im)[None].cuda())
        oh, ow = proc.output_size(*im.shape[:2])
        assert tuple(r.shape) == (1, oh, ow, 3)
        top, left = (oh - 224) // 2, (ow - 224) // 2
        diff = int((r[0, top:top + 224, left:left + 224].cpu().numpy() != g[f"resized_{i}"]).sum())
        assert diff == 0, f"image {i}: {diff} bytes differ from PIL's resize"
        assert torch.equal(r.cpu(), emu.resample_u8(emu.resample_u8(torch.from_numpy(im)[None], ow, 0), oh, 1))     # outside the crop too
    pv0 = proc(images=fx.images()[0], return_tensors="pt").pixel_values
    assert pv0.is_cuda and np.array_equal(pv0[0].cpu().numpy().view(np.int32), g["pixel_values_0"].view(np.int32))
    batch = proc(torch.from_numpy(np.stack([fx.images()[3], fx.images()[3][::-1].copy()]))).pixel_values
    assert torch.equal(batch[0], proc(fx.images()[3]).pixel_values[0]) and tuple(batch.shape) == (2, 3, 224, 224)


# ------------------------------------------------------------------ 4. me_cosine_rows
def test_cosine_rows_against_fp64(ops):
    """Bound: the fp32 emulation's own error against fp64 on the same inputs, times 4 for the reduction order, per shape.  Measured on an MI355X: kernel
    1.5e-8 ... 3.0e-8, emulation 1.5e-8 ... 3.1e-8 on the five shapes (never 0), so the bounds are 6e-8 ... 1.2e-7."""
    for rows, C, shared in ((24, 768, False), (23, 768, True), (5, 64, False), (1, 33, True), (300, 1000, False)):
        g = np.random.Generator(np.random.Philox(key=rows * 1000 + C))
        a = torch.from_numpy(g.standard_normal((rows, C)).astype(np.float32) + 0.25)
        b = torch.from_numpy(g.standard_normal((1 if shared else rows, C)).astype(np.float32) + 0.25)
        want = (a.double() * b.double()).sum(1) / (a.double().norm(dim=1) * b.double().norm(dim=1))
        emu_err = float((emu.cosine_rows(a, b).double() - want).abs().max())
        bound = 4 * emu_err
        got = ops.cosine_rows(a.cuda(), b.cuda())
        err = float((got.cpu().double() - want).abs().max())
        print(f"cosine_rows {rows} x {C}{' shared' if shared else ''}: |err| {err:.3e}, fp32 emulation {emu_err:.3e}, bound {bound:.3e}")
        assert err <= bound and torch.equal(ops.cosine_rows(a.cuda(), b.cuda()), got)
    big = torch.zeros(10, 80).cuda()
    big[:, 8:72] = 1.0
    assert torch.equal(ops.cosine_rows(big[:, 8:72], big[0, 8:72]).cpu(), torch.ones(10))      # views


# ------------------------------------------------------------------ 5. the encoder against transformers
def test_encoder_matches_transformers_fp32(ops, tower, pv, gold):
    out = tower(pv)
    floor = float(gold["fp16_floor"])
    e, h = rel(out.image_embeds, gold["image_embeds"]), rel(out.last_hidden_state[:, [0, 256]], gold["hidden_rows"])
    print(json.dumps(dict(test="clip_vision_parity", tokens=257, image_embeds_rel_l2=e, hidden_rows_rel_l2=h, fp16_floor=floor, bound=2 * floor)))
    assert out.image_embeds.dtype == torch.float32 and tuple(out.image_embeds.shape) == (2, 64) and tuple(out.last_hidden_state.shape) == (2, 257, 256)
    assert e <= 2 * floor and h <= 2 * floor
    assert torch.equal(tower(pv).image_embeds, out.image_embeds)


def test_encoder_patch32_and_text_projection_match_transformers_fp32(ops, pv, gold):
    from motioneditor_amd.models.clip import CLIPTextModelWithProjection, CLIPVisionModelWithProjection
    t32 = CLIPVisionModelWithProjection(fx.vision_state_dict(fx.VISION32), fx.VISION32, device="cuda")
    e = rel(t32(pv).image_embeds, gold["image_embeds32"])
    text = CLIPTextModelWithProjection(fx.text_state_dict(), dict(fx.TEXT, eos_token_id=fx.EOS), device="cuda")
    t = rel(text(torch.from_numpy(fx.text_ids())).text_embeds, gold["text_embeds"])
    print(json.dumps(dict(test="clip_vision_parity", tokens=50, image_embeds_rel_l2=e, bound=2 * float(gold["fp16_floor32"]), text_embeds_rel_l2=t,
                          text_bound=2 * float(gold["text_fp16_floor"]))))
    assert e <= 2 * float(gold["fp16_floor32"]) and t <= 2 * float(gold["text_fp16_floor"])


def test_encoder_batch_permutation_and_image_independence_are_bitwise(ops, tower):
    x = torch.from_numpy(fx.pixel_values(3)).cuda()
    a = tower(x)
    b = tower(x[[2, 0, 1]].contiguous())
    assert torch.equal(b.image_embeds, a.image_embeds[[2, 0, 1]]) and torch.equal(b.last_hidden_state, a.last_hidden_state[[2, 0, 1]])
    y = x.clone()
    y[1] = y[1].flip(-1)
    c = tower(y)
    assert torch.equal(c.image_embeds[[0, 2]], a.image_embeds[[0, 2]]) and not torch.equal(c.image_embeds[1], a.image_embeds[1])
    assert torch.equal(tower(x[:1]).image_embeds, a.image_embeds[:1])


def test_two_layers_at_production_widths(ops):
    """hidden 1024, 16 heads, intermediate 4096, projection 768, 3 images: whatever kernels me_gemm's dispatch picks for M = 771 / 768 / 3."""
    from motioneditor_amd.models.clip import CLIPVisionModelWithProjection
    cfg = dict(num_hidden_layers=2)
    tower = CLIPVisionModelWithProjection.from_synthetic("cuda", 7, cfg)
    assert tower.config.hidden_size == 1024 and tower.config.num_attention_heads == 16 and tower.config.projection_dim == 768 and tower.tokens == 257
    x = torch.from_numpy(fx.pixel_values(3)).cuda()
    a = tower(x)
    assert tuple(a.image_embeds.shape) == (3, 768) and torch.isfinite(a.image_embeds).all() and torch.isfinite(a.last_hidden_state).all()
    assert float(a.image_embeds.abs().max()) > 0
    b = tower(x)
    assert torch.equal(a.image_embeds, b.image_embeds) and torch.equal(a.last_hidden_state, b.last_hidden_state)


# ------------------------------------------------------------------ 6. metrics
def test_clip_metrics_of_a_synthetic_video(ops, monkeypatch):
    """The processor is bitwise, so the cosines of the device pipeline and of the emulated pipeline (same weights, fp32) differ by the encoder's error only:
    the cosines are held to the encoder bound, 2 x fp16_floor.  (Embeddings within 2 x fp16_floor of each other in rel-L2 could move a cosine by twice that --
    |cos(a + da, b + db) - cos(a, b)| <= |da| / |a| + |db| / |b| -- but the error of an embedding is mostly along it, which a cosine does not see.)  Measured on
    an MI355X: frame consistency differs by 9.6e-5, text alignment by 3.9e-4; the bound is 4.8e-3."""
    from motioneditor_amd import metrics
    from motioneditor_amd.models import clip
    from motioneditor_amd.tokenizer import CLIPTokenizer
    tok = CLIPTokenizer.from_synthetic()
    tcfg = dict(fx.TEXT, vocab_size=len(tok), eos_token_id=tok.eos_token_id)
    from motioneditor_amd import synth
    tschema = clip.clip_text_schema(tcfg)
    tschema["text_projection.weight"] = (64, 256)
    tsd = dict(synth.synth_state_dict(tschema, 5, salt="clip."))
    vsd = fx.vision_state_dict()
    video = torch.from_numpy(np.random.Generator(np.random.Philox(key=4)).random((1, 3, 8, 64, 64), dtype=np.float32))
    dev = clip.CLIPModel(clip.CLIPTextModelWithProjection(tsd, tcfg, "cuda"), clip.CLIPVisionModelWithProjection(vsd, fx.VISION, "cuda"))
    got = metrics.clip_metrics(video.cuda(), "a girl is dancing", dev, clip.CLIPImageProcessor(), tok)
    frames = metrics.video_frames_u8(video.cuda())
    assert torch.equal(frames.cpu(), (video[0].permute(1, 2, 3, 0) * 255).to(torch.uint8))          # what save_videos_grid writes
    monkeypatch.setattr(clip, "ops", emu)
    monkeypatch.setattr(metrics, "ops", emu)
    ref = clip.CLIPModel(clip.CLIPTextModelWithProjection(tsd, tcfg, "cpu", torch.float32), clip.CLIPVisionModelWithProjection(vsd, fx.VISION, "cpu", torch.float32))
    want = metrics.clip_metrics(video, "a girl is dancing", ref, clip.CLIPImageProcessor(device="cpu"), tok)
    floor = float(np.load(GOLD / "clip_vision.npz")["fp16_floor"])
    for k in ("frame_consistency", "text_alignment"):
        print(f"clip_metrics {k}: device {got[k]:.6f}, emulated {want[k]:.6f}, |diff| {abs(got[k] - want[k]):.3e} (bound {2 * floor:.3e})")
        assert np.isfinite(got[k]) and abs(got[k] - want[k]) <= 2 * floor


def test_run_edit_metrics_flag(ops, unet_sd_np, cn_sd_np, tmp_path, monkeypatch, capsys):
    """examples/run_edit.py --metrics synthetic at 8 frames x 64^2 with 2 steps: a finite metrics.json with the expected keys; the GIFs are bitwise what the
    same command writes without the flag."""
    sys.path.insert(0, str(ROOT / "examples"))
    import run_edit
    from motioneditor_amd.models.controlnet import ControlNetModel
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    from motioneditor_amd.models.vae import AutoencoderKL
    from motioneditor_amd.pipelines import MotionEditorPipeline
    vae, unet, cn = AutoencoderKL.from_synthetic("cuda"), UNet2DConditionModel(unet_sd_np, "cuda:0"), ControlNetModel(cn_sd_np, "cuda:0")
    monkeypatch.setattr(run_edit, "build_pipeline", lambda device="cuda": MotionEditorPipeline(vae=vae, unet=unet, controlnet=cn))
    base = ["run_edit.py", "--frames", "8", "--size", "64", "--steps", "2", "--inv-steps", "2", "--prompt", "a girl is dancing", "--target-prompt", "a boy is dancing"]
    monkeypatch.setattr(sys, "argv", base + ["--out", str(tmp_path / "plain")])
    run_edit.main()
    unet.spatial_editor = unet.temporal_editor = None
    monkeypatch.setattr(sys, "argv", base + ["--out", str(tmp_path / "scored"), "--metrics", "synthetic"])
    run_edit.main()
    assert "metrics.json" in capsys.readouterr().out
    gifs = sorted(p.name for p in (tmp_path / "plain" / "sample").iterdir())
    assert gifs == ["a boy is dancing-inv.gif", "a boy is dancing.gif"] and not (tmp_path / "plain" / "sample" / "metrics.json").exists()
    for name in gifs:
        assert (tmp_path / "plain" / "sample" / name).read_bytes() == (tmp_path / "scored" / "sample" / name).read_bytes(), name
    m = json.loads((tmp_path / "scored" / "sample" / "metrics.json").read_text())
    assert sorted(m) == ["clip", "edits", "reconstruction", "source"] and m["clip"] == "synthetic" and list(m["edits"]) == ["a boy is dancing"]
    assert sorted(m["source"]) == ["frame_consistency"]
    for part in (m["reconstruction"], m["edits"]["a boy is dancing"]):
        assert sorted(part) == ["frame_consistency", "text_alignment"]
    flat = [m["source"]["frame_consistency"]] + [v for part in (m["reconstruction"], m["edits"]["a boy is dancing"]) for v in part.values()]
    assert all(np.isfinite(v) and -1.0 <= v <= 1.0 for v in flat)
