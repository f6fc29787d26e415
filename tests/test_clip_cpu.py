"""The native CLIP text encoder and tokenizer without a GPU: the tokenizer against transformers' recorded ids (tests/golden/clip_tokenizer.json), the
launch graph of models/clip.py on the emulated ABI against transformers' recorded fp32 output (tests/golden/clip_text.npz; generator
tools/make_golden_clip.py, weights tests/clip_fixture.py), key spellings, refusals, the from_pretrained round trip and the pipeline's prompt encoding."""
import json

import numpy as np
import pytest
import torch

import clip_fixture
import emu_clip_ops
from conftest import GOLD, max_rel
from motioneditor_amd import tokenizer as tk
from motioneditor_amd.models import clip

SMALL = dict(num_hidden_layers=2, vocab_size=600, hidden_size=768, num_attention_heads=12, intermediate_size=256)   # a 2-layer encoder for the plumbing tests


@pytest.fixture()
def emu(monkeypatch):
    monkeypatch.setattr(clip, "ops", emu_clip_ops)
    return emu_clip_ops


@pytest.fixture(scope="module")
def tok_gold():
    return json.loads((GOLD / "clip_tokenizer.json").read_text())


@pytest.fixture(scope="module")
def tok(tok_gold):
    return tk.CLIPTokenizer(vocab=tok_gold["vocab"], merges=tok_gold["merges"])


def get_word_inds(text, word_place, tokenizer):
    """inference.py:52-71 / ptp_utils.py:281-299, as the reference uses a tokenizer's encode / decode."""
    split_text = text.split(" ")
    if type(word_place) is str:
        word_place = [i for i, word in enumerate(split_text) if word_place == word]
    elif type(word_place) is int:
        word_place = [word_place]
    out = []
    if len(word_place) > 0:
        words_encode = [tokenizer.decode([item]).strip("#") for item in tokenizer.encode(text)][1:-1]
        cur_len, ptr = 0, 0
        for i in range(len(words_encode)):
            cur_len += len(words_encode[i])
            if ptr in word_place:
                out.append(i + 1)
            if cur_len >= len(split_text[ptr]):
                ptr += 1
                cur_len = 0
    return out


# ------------------------------------------------------------------ 1. tokenizer
def test_tokenizer_matches_transformers_on_every_fixture_string(tok, tok_gold):
    strings, want = tok_gold["strings"], tok_gold["input_ids"]
    assert len(strings) >= 30 and len(tok) == len(tok_gold["vocab"]) and tok.model_max_length == 77
    got = tok(strings, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
    assert got.dtype == torch.int64 and tuple(got.shape) == (len(strings), 77)
    for s, g, w, e in zip(strings, got.tolist(), want, tok_gold["encode"]):
        assert g == w, (s, g, w)
        assert tok.encode(s) == e, s                                       # untruncated, with the two specials
        assert tok(s, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids.tolist() == [w]   # a str is a batch of one
    eos, bos = tok_gold["vocab"]["<|endoftext|>"], tok_gold["vocab"]["<|startoftext|>"]
    assert tok.eos_token_id == tok.pad_token_id == eos and tok.bos_token_id == bos
    assert want[2] == [bos] + [eos] * 76                                   # the empty prompt
    long = tok_gold["encode"][-1]
    assert len(long) > 77 and got[-1].tolist() == long[:76] + [eos]        # truncation keeps end-of-text last
    for i, text in tok_gold["decode_single"].items():
        assert tok.decode([int(i)]) == text, (i, text)
    for s, text in tok_gold["decode_full"].items():
        assert tok.decode(tok.encode(s)) == text, s


def test_tokenizer_serves_get_word_inds(tok):
    assert [tok.decoder[i] for i in tok.encode("a girl is dancing")[1:-1]] == ["a</w>", "girl</w>", "is</w>", "danc", "ing</w>"]
    assert get_word_inds("a girl is dancing", "girl", tok) == [2]
    assert get_word_inds("a girl is dancing", "dancing", tok) == [4, 5]
    assert get_word_inds("a girl is dancing", 0, tok) == [1]
    assert get_word_inds("a girl is dancing", "boy", tok) == []


def test_tokenizer_reads_vocab_and_merges_files(tmp_path, tok, tok_gold):
    d = tmp_path / "tokenizer"
    d.mkdir()
    (d / "vocab.json").write_text(json.dumps(tok_gold["vocab"]), encoding="utf-8")
    (d / "merges.txt").write_text("#version: 0.2\n" + "\n".join(" ".join(m) for m in tok_gold["merges"]) + "\n", encoding="utf-8")
    t2 = tk.CLIPTokenizer.from_pretrained(tmp_path, subfolder="tokenizer")
    t3 = tk.CLIPTokenizer(d / "vocab.json", d / "merges.txt")
    for s in tok_gold["strings"]:
        assert t2.encode(s) == t3.encode(s) == tok.encode(s)
    with pytest.raises(FileNotFoundError):
        tk.CLIPTokenizer.from_pretrained(tmp_path, subfolder="nope")


# ------------------------------------------------------------------ 2. launch graph vs transformers
def test_encoder_graph_matches_transformers_fp32(emu):
    """Against clip_text.npz["last_hidden_state"] itself (transformers in fp32 with the fp32 weights): on the emulated ABI `Packed` keeps the
    weights in fp32 (dtype=torch.float32), so no fp16-rounded variant of the fixture is needed.  Bound: tests/test_vae_cpu.py's 2e-4."""
    g = np.load(GOLD / "clip_text.npz")
    model = clip.CLIPTextModel(clip_fixture.perturbed_state_dict(), device="cpu", dtype=torch.float32)
    assert vars(model.config) == clip.DEFAULT_CONFIG
    out = model(torch.from_numpy(g["input_ids"]).long())
    got, want = out[0], torch.from_numpy(g["last_hidden_state"])
    assert out.last_hidden_state is got and got.dtype == torch.float32 and tuple(got.shape) == (3, 77, 768)
    err = max_rel(got, want)
    print(f"emulated graph vs transformers fp32: max-relative {err:.3e}")
    assert err < 2e-4
    got2 = model(torch.from_numpy(g["input_ids2"]).long())[0]
    assert max_rel(got2[2], torch.from_numpy(g["last_hidden_state2_row2"])) < 2e-4
    assert torch.equal(got2[:2], got[:2]) and torch.equal(got2[2, :50], got[2, :50]) and not torch.equal(got2[2, 50:], got[2, 50:])


# ------------------------------------------------------------------ 3. keys and refusals
def small_sd():
    from motioneditor_amd import synth
    return dict(synth.synth_state_dict(clip.clip_text_schema(SMALL), 5, salt="clip."))


def test_key_spellings_and_refusals(emu, monkeypatch):
    sd = small_sd()
    ids = torch.randint(0, SMALL["vocab_size"], (2, 77), generator=torch.Generator().manual_seed(0))
    a = clip.CLIPTextModel(sd, SMALL, device="cpu", dtype=torch.float32)
    pre = {"text_model." + k: v for k, v in sd.items()}
    pre["text_model.embeddings.position_ids"] = np.arange(77)[None]
    b = clip.CLIPTextModel(pre, SMALL, device="cpu", dtype=torch.float32)
    assert a.config.num_hidden_layers == b.config.num_hidden_layers == 2 and a.config.vocab_size == 600 and a.config.intermediate_size == 256
    ya = a(ids)[0]
    assert torch.equal(ya, b(ids)[0]) and tuple(ya.shape) == (2, 77, 768) and torch.isfinite(ya).all()
    # the nn.Module surface the harness touches
    assert a.requires_grad_(False) is a and a.eval() is a and a.to("cpu") is a and a.device == torch.device("cpu") and a.dtype == torch.float16
    with pytest.raises(KeyError, match="rotary_emb.inv_freq"):
        clip.CLIPTextModel(dict(sd, **{"encoder.layers.0.self_attn.rotary_emb.inv_freq": np.zeros(4, np.float32)}), SMALL, device="cpu")
    with pytest.raises(KeyError, match="final_layer_norm.bias"):
        clip.CLIPTextModel({k: v for k, v in sd.items() if k != "final_layer_norm.bias"}, SMALL, device="cpu")
    with pytest.raises(NotImplementedError, match="'gelu'"):
        clip.CLIPTextModel(sd, dict(SMALL, hidden_act="gelu"), device="cpu")
    with pytest.raises(NotImplementedError, match="96"):
        clip.CLIPTextModel(sd, dict(SMALL, num_attention_heads=8), device="cpu")
    with pytest.raises(NotImplementedError, match="attention_mask"):
        a(ids, attention_mask=torch.ones(2, 77))

    def boom(*args, **kw):
        raise AssertionError("launched before the arguments were checked")
    for name in ("embed_rows", "gemm", "layernorm", "attention_causal", "quick_gelu"):
        monkeypatch.setattr(emu_clip_ops, name, boom)
    with pytest.raises(ValueError, match="position table"):
        a(torch.zeros(1, 78, dtype=torch.int64))
    for bad in (SMALL["vocab_size"], -1):
        with pytest.raises(ValueError, match="outside the vocabulary"):
            a(torch.tensor([[0, bad, 1]]))
    from motioneditor_amd import plan
    monkeypatch.setattr(plan, "ACTIVE", object())
    with pytest.raises(RuntimeError, match="being recorded"):
        a(ids)


# ------------------------------------------------------------------ 4. from_pretrained + the pipeline's prompt encoding
def test_from_pretrained_round_trip_and_pipeline_prompts(emu, tmp_path, tok_gold):
    from types import SimpleNamespace

    from safetensors.torch import save_file
    from motioneditor_amd.pipelines import MotionEditorPipeline
    cfg = dict(SMALL, vocab_size=len(tok_gold["vocab"]))
    from motioneditor_amd import synth
    sd = dict(synth.synth_state_dict(clip.clip_text_schema(cfg), 5, salt="clip."))
    te, td = tmp_path / "text_encoder", tmp_path / "tokenizer"
    te.mkdir()
    td.mkdir()
    (te / "config.json").write_text(json.dumps(dict(clip.DEFAULT_CONFIG, **cfg, architectures=["CLIPTextModel"], model_type="clip_text_model", projection_dim=768)))
    save_file({"text_model." + k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, str(te / "model.safetensors"))
    (td / "vocab.json").write_text(json.dumps(tok_gold["vocab"]), encoding="utf-8")
    (td / "merges.txt").write_text("#version: 0.2\n" + "\n".join(" ".join(m) for m in tok_gold["merges"]), encoding="utf-8")

    enc = clip.CLIPTextModel.from_pretrained(tmp_path, subfolder="text_encoder", device="cpu")
    tok = tk.CLIPTokenizer.from_pretrained(tmp_path, subfolder="tokenizer")
    assert enc.config.num_hidden_layers == 2 and enc.config.vocab_size == len(tok) and enc.config.intermediate_size == 256
    enc.P = type(enc.P)(enc.P.state, "cpu", dtype=torch.float32)      # (the emulated ABI computes in fp32)
    direct = clip.CLIPTextModel(sd, cfg, device="cpu", dtype=torch.float32)
    prompts = ["a girl is dancing", "a boy is dancing"]
    ids = tok(prompts, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
    assert torch.equal(enc(ids)[0], direct(ids)[0])

    pipe = MotionEditorPipeline(text_encoder=enc, tokenizer=tok, unet=SimpleNamespace(device=torch.device("cpu")))
    emb = pipe._encode_prompt(prompts, "cpu", 1, True, None)
    unc = direct(tok([""] * 2, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids)[0]
    assert tuple(emb.shape) == (4, 77, 768) and torch.equal(emb, torch.cat([unc, direct(ids)[0]]))
    assert torch.equal(pipe._encode_prompt(prompts, "cpu", 1, False, None), direct(ids)[0])
    from motioneditor_amd import util
    assert torch.equal(util._context(pipe, prompts[0], None), direct(ids[:1])[0])
    with pytest.raises(ValueError, match="no text_encoder/tokenizer"):
        MotionEditorPipeline(unet=SimpleNamespace(device=torch.device("cpu")))._encode_prompt(prompts, "cpu", 1, True, None)


# ------------------------------------------------------------------ 5. ABI
def test_abi_has_the_clip_entries_and_stays_at_9():
    import ctypes

    from motioneditor_amd import build, capi
    for name in ("me_embed_rows", "me_attn_causal", "me_quick_gelu"):
        assert name in capi.SYMBOLS
    assert "clip.hip" in build.SOURCES
    L = capi.lib()
    assert L.me_abi_version() == 9
    # arguments the entries do not serve come back as ME_EINVAL, without a device
    assert L.me_attn_causal(4096, 768, 4096, 2304, 4096, 2304, 4096, 2304, 1, 12, 40, 77, ctypes.c_float(0.125), None) == capi.ME_EINVAL and b"dh = 64" in L.me_last_error()
    assert L.me_attn_causal(4096, 768, 4096, 2304, 4096, 2304, 4096, 2304, 1, 12, 64, 129, ctypes.c_float(0.125), None) == capi.ME_EINVAL
    assert L.me_attn_causal(4096, 768, 4096, 2300, 4096, 2304, 4096, 2304, 1, 12, 64, 77, ctypes.c_float(0.125), None) == capi.ME_EINVAL
    assert L.me_embed_rows(4096, 4096, 4096, 4096, 77, 77, 772, 100, None) == capi.ME_EINVAL
    assert L.me_quick_gelu(None, None, 0, None) == capi.ME_EINVAL
