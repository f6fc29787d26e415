"""The native CLIP text encoder on a real MI355X: the three kernels of csrc/clip.hip against their fp32 emulation (tests/emu_clip_ops.py), the whole
encoder against transformers' recorded fp32 output (tests/golden/clip_text.npz, generator tools/make_golden_clip.py), causality and reproducibility
bit for bit, and a denoising step fed with natively encoded prompts.

Measured on an MI355X (profiles/clip_parity.jsonl): encoder vs transformers fp32 rel-L2 1.71e-3, bound 2 x fp16_floor = 3.43e-3."""
import json

import numpy as np
import pytest
import torch

import clip_fixture
import emu_clip_ops as emu
from conftest import GOLD

pytestmark = pytest.mark.gpu

# The defaults of check() in tests/test_kernels_gpu.py (fp16 storage, fp32 accumulation): what test_attention_cross_text_77_keys and the SiLU
# epilogue case are held to against emu_ops.  Restated, not chosen here.
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
def encoder(ops):
    from motioneditor_amd.models.clip import CLIPTextModel
    return CLIPTextModel(clip_fixture.perturbed_state_dict(), device="cuda")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD / "clip_text.npz")


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.float16)


def errs(got, want):
    got, want = got.detach().float().cpu().double(), want.detach().float().cpu().double()
    assert got.shape == want.shape and torch.isfinite(got).all()
    return float((got - want).norm() / want.norm().clamp_min(1e-30)), float((got - want).abs().max() / want.abs().mean().clamp_min(1e-30))


def check(got, want, name):
    r, m = errs(got, want)
    print(f"{name}: rel-L2 {r:.3e}, max/mean {m:.3e}")
    assert r <= REL_L2 and m <= MAX_REL, f"{name}: rel-L2 {r:.3e} (<= {REL_L2}), max/mean {m:.3e} (<= {MAX_REL})"


# ------------------------------------------------------------------ 6. the kernels
@pytest.mark.parametrize("n_seq,seq,vocab,C", [(3, 77, 49408, 768), (1, 5, 300, 64), (4, 128, 1000, 8)])
def test_embed_rows_is_exact_to_one_rounding(ops, n_seq, seq, vocab, C):
    tok, pos = rnd(vocab, C, seed=1, scale=0.05), rnd(seq + 3, C, seed=2, scale=0.05)
    ids = torch.randint(0, vocab, (n_seq * seq,), generator=torch.Generator().manual_seed(3), dtype=torch.int32)
    ids[0], ids[-1] = vocab - 1, 0
    got = ops.embed_rows(tok.cuda(), pos.cuda(), ids.cuda(), seq)
    want = emu.embed_rows(tok, pos, ids, seq)               # the fp32 sum rounded once to fp16
    assert got.dtype == torch.float16 and torch.equal(got.cpu(), want)
    with pytest.raises(ValueError):
        ops.embed_rows(tok.cuda(), pos.cuda(), ids.cuda(), seq + 4)            # longer than the position table
    with pytest.raises(ValueError):
        ops.embed_rows(tok.cuda(), pos.cuda(), ids.cuda().long(), seq)         # ids must be int32


@pytest.mark.parametrize("n_seq,heads,nq", [(1, 12, 77), (4, 12, 77), (3, 2, 16), (2, 12, 128)])
def test_attn_causal(ops, n_seq, heads, nq):
    """High-gain q / k (logits of std ~ 9 before the mask): the rows are peaky, so a wrong mask, maximum or denominator shows.  q, k, v are the column slices of
    one fused [rows, 3 * heads * 64] tensor, as the encoder passes them."""
    C = heads * 64
    qkv = rnd(n_seq * nq, 3 * C, seed=4)
    qkv[:, :2 * C] *= 3.0
    d = qkv.cuda()
    args = dict(heads=heads, dh=64, n_seq=n_seq, nq=nq)
    got = ops.attention_causal(d[:, :C], d[:, C:2 * C], d[:, 2 * C:], **args)
    assert ops._last_kernel() == "attn_causal_kernel"
    want = emu.attention_causal(qkv[:, :C].float(), qkv[:, C:2 * C].float(), qkv[:, 2 * C:].float(), **args)
    check(got, want, f"attn_causal n_seq={n_seq} heads={heads} nq={nq}")
    assert torch.equal(got, ops.attention_causal(d[:, :C], d[:, C:2 * C], d[:, 2 * C:], **args))       # no atomics: bitwise
    # position 0 sees only itself: O[s, 0] = V[s, 0] exactly
    assert torch.equal(got.reshape(n_seq, nq, C)[:, 0], d[:, 2 * C:].reshape(n_seq, nq, C)[:, 0])
    # a later key never reaches an earlier query: overwrite the last key / value row of every sequence
    d2 = d.clone()
    d2.reshape(n_seq, nq, 3 * C)[:, nq - 1, C:] = 7.0
    got2 = ops.attention_causal(d2[:, :C], d2[:, C:2 * C], d2[:, 2 * C:], **args)
    assert torch.equal(got2.reshape(n_seq, nq, C)[:, :nq - 1], got.reshape(n_seq, nq, C)[:, :nq - 1])


def test_attn_causal_refuses_what_it_does_not_serve(ops):
    x = rnd(2 * 129, 3 * 320, seed=5).cuda()
    with pytest.raises(ValueError, match="dh = 64"):
        ops.attention_causal(x[:77, :320], x[:77, 320:640], x[:77, 640:], heads=8, dh=40, n_seq=1, nq=77)
    with pytest.raises(ValueError, match="128"):
        ops.attention_causal(x[:, :320], x[:, 320:640], x[:, 640:], heads=5, dh=64, n_seq=2, nq=129)


def test_quick_gelu(ops):
    x = torch.cat([torch.linspace(-30, 30, 4096), rnd(3 * 77 * 3072 - 4096 - 5, seed=6, scale=2.0).float(), torch.tensor([-65504.0, 65504.0, 0.0, -0.0, 11.0])]).to(torch.float16)
    x = x[:x.numel() // 8 * 8].contiguous()
    got = ops.quick_gelu(x.cuda())
    want = emu.quick_gelu(x.float())
    check(got, want, "quick_gelu")
    big = x.float().abs() > 10
    assert int(big.sum()) > 1000
    check(got.cpu()[big], want[big], "quick_gelu |x| > 10")
    small = x.float().abs() <= 3
    check(got.cpu()[small], want[small], "quick_gelu |x| <= 3")


# ------------------------------------------------------------------ 7. the encoder vs transformers
def test_encoder_matches_transformers_within_twice_the_fp16_floor(encoder, gold):
    """rel-L2 against transformers' fp32 output <= 2 x fp16_floor, the floor read from the fixture (torch's own fp16 evaluation of the same model against its
    fp32 one).  Measured: 1.71e-3 (per prompt 1.45e-3 / 1.60e-3 / 2.02e-3) against a bound of 3.43e-3."""
    floor = float(gold["fp16_floor"])
    got = encoder(torch.from_numpy(gold["input_ids"]).long())[0]
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (3, 77, 768)
    r, m = errs(got, torch.from_numpy(gold["last_hidden_state"]))
    per = [errs(got[i], torch.from_numpy(gold["last_hidden_state"][i]))[0] for i in range(3)]
    print("clip_parity " + json.dumps(dict(rel_l2=r, max_over_mean=m, per_prompt=per, fp16_floor=floor, bound=2 * floor)))
    assert r <= 2 * floor, (r, floor)
    r2, _ = errs(encoder(torch.from_numpy(gold["input_ids2"]).long())[0][2], torch.from_numpy(gold["last_hidden_state2_row2"]))
    assert r2 <= 2 * floor, (r2, floor)


# ------------------------------------------------------------------ 8. causality and reproducibility, bit for bit
def test_encoder_is_causal_and_reproducible_bitwise(encoder, gold):
    ids, ids2 = torch.from_numpy(gold["input_ids"]).long(), torch.from_numpy(gold["input_ids2"]).long()
    assert (ids != ids2).nonzero().tolist() == [[2, 50]]
    a, b = encoder(ids)[0], encoder(ids2)[0]
    assert torch.equal(a[:2], b[:2]) and torch.equal(a[2, :50], b[2, :50])
    assert all(not torch.equal(a[2, r], b[2, r]) for r in range(50, 77))
    assert torch.equal(a, encoder(ids)[0])                                  # two runs
    perm = [2, 0, 1]
    assert torch.equal(encoder(ids[perm])[0], a[perm])                      # a permuted batch permutes the outputs
    # another batch size may select another GEMM kernel / split for the other row count: close, not necessarily bitwise
    for i in range(3):
        r, _ = errs(encoder(ids[i:i + 1])[0][0], a[i])
        assert r <= REL_L2, (i, r)


# ------------------------------------------------------------------ 9. a denoising step on natively encoded prompts
def test_denoise_step_on_natively_encoded_prompts(ops, encoder, unet_sd_np, cn_sd_np):
    """The step fed with `_encode_prompt`'s result equals the step fed the same numbers as a plain tensor, bit for bit, eager and planned, with the encoder
    running again between the steps (between a plan's recording and its replay too): it disturbs neither the step's streams nor its plans nor its scratch."""
    from motioneditor_amd import tokenizer
    from motioneditor_amd.attn_control import (FullySelfAttentionControlMask, TemporalSelfAttentionControl,
                                               regiter_fully_attention_editor_diffusers, regiter_temporal_attention_editor_diffusers)
    from motioneditor_amd.models.controlnet import ControlNetModel
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    from motioneditor_amd.pipelines import MotionEditorPipeline
    from test_step_cpu import step_inputs
    tg = json.loads((GOLD / "clip_tokenizer.json").read_text())
    tok = tokenizer.CLIPTokenizer(vocab=tg["vocab"], merges=tg["merges"])
    x = step_inputs()
    f = x["latents"].shape[2]
    pipe = MotionEditorPipeline(unet=UNet2DConditionModel(unet_sd_np, "cuda:0"), controlnet=ControlNetModel(cn_sd_np, "cuda:0"), text_encoder=encoder, tokenizer=tok)
    ted = TemporalSelfAttentionControl(start_step=4, start_layer=10)
    regiter_temporal_attention_editor_diffusers(pipe, ted)
    sed = FullySelfAttentionControlMask(start_step=4, start_layer=10, source_masks=x["masks"])
    regiter_fully_attention_editor_diffusers(pipe, sed)
    pipe.scheduler.set_timesteps(50)
    step = 4
    t = pipe.scheduler.timesteps[step]
    images = torch.cat([x["skeleton"]] * 2).reshape(2 * f, 3, 64, 64).cuda()
    lat = x["latents"].cuda()
    prompts = ["a girl is dancing", "a boy is dancing"]

    def run(fn, emb):
        ted.cur_step = sed.cur_step = step
        out = fn(lat, t, emb, images, 7.5)
        torch.cuda.synchronize()
        return out

    emb = pipe._encode_prompt(prompts, "cuda", 1, True, None)
    assert tuple(emb.shape) == (4, 77, 768) and emb.is_cuda and torch.isfinite(emb).all()
    plain = emb.cpu().clone().cuda()                                   # the same numbers as a tensor that never saw the encoder
    ref = run(pipe.denoise_step, plain)
    got = run(pipe.denoise_step, pipe._encode_prompt(prompts, "cuda", 1, True, None))
    assert torch.isfinite(got).all() and torch.equal(got, ref)
    p1 = run(pipe.denoise_step_planned, pipe._encode_prompt(prompts, "cuda", 1, True, None))     # records the plan
    emb2 = pipe._encode_prompt(prompts, "cuda", 1, True, None)                                    # the encoder between recording and replay
    p2 = run(pipe.denoise_step_planned, emb2)                                                      # replays it
    assert torch.equal(emb2, emb) and torch.equal(p1, ref) and torch.equal(p2, ref)
    assert torch.equal(run(pipe.denoise_step_planned, plain), ref)
    pipe.release_plans()


def test_run_edit_example_with_prompts_equals_the_same_run_on_tensors(ops, encoder, unet_sd_np, cn_sd_np):
    """examples/run_edit.py --prompt / --target-prompt: the harness sequence with the pipeline's native text encoder and tokenizer (empty prompt for the
    inversion, [""] * 2 + the two prompts for the loop) gives, bit for bit, what the same sequence gives when it is handed those encodings as tensors."""
    import sys
    from conftest import ROOT
    sys.path.insert(0, str(ROOT / "examples"))
    import run_edit
    from motioneditor_amd.models.controlnet import ControlNetModel
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    from motioneditor_amd.models.vae import AutoencoderKL
    from motioneditor_amd.pipelines import MotionEditorPipeline
    from motioneditor_amd.tokenizer import CLIPTokenizer
    tok = CLIPTokenizer.from_synthetic()
    assert len(tok) == 514 and tok.decode(tok.encode("a girl")) == "<|startoftext|>a girl <|endoftext|>"
    f, H = 8, 64
    pipe = MotionEditorPipeline(vae=AutoencoderKL.from_synthetic("cuda"), unet=UNet2DConditionModel(unet_sd_np, "cuda:0"), controlnet=ControlNetModel(cn_sd_np, "cuda:0"),
                                text_encoder=encoder, tokenizer=tok)
    xs = {k: v.cuda() for k, v in run_edit.harness_inputs(f, H, H).items()}
    prompts = ["a girl is dancing", "a boy is dancing"]
    s_inv, s_gen, inv_lat = run_edit.run(pipe, xs, steps=2, inv_steps=2, prompts=prompts)
    ids = lambda texts: tok(texts, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids   # noqa: E731
    xs["negative_text_embeddings"] = encoder(ids([""]))[0]
    xs["text_embeddings"] = torch.cat([encoder(ids([""] * 2))[0], encoder(ids(prompts))[0]])          # all 2 * len(prompts) rows: cat([uncond, text])
    pipe.unet.spatial_editor = pipe.unet.temporal_editor = None
    t_inv, t_gen, t_lat = run_edit.run(pipe, xs, steps=2, inv_steps=2)
    assert s_gen.shape == (1, 3, f, H, H) and torch.isfinite(s_gen).all()
    assert torch.equal(inv_lat, t_lat) and torch.equal(s_inv, t_inv) and torch.equal(s_gen, t_gen)
