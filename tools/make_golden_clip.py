"""Generate tests/golden/clip_text.npz and tests/golden/clip_tokenizer.json: what `transformers` (CLIPTextModel, CLIPTokenizer) computes
for the inputs the CLIP tests feed `motioneditor_amd.models.clip` / `motioneditor_amd.tokenizer`.

Test infrastructure, not product code, run by hand on a machine that has `transformers`; no test imports that package.

clip_text.npz       SD-1.5 configuration, the weights of tests/clip_fixture.py loaded by key name into transformers.CLIPTextModel, fp32 on the CPU:
                    input_ids [3, 77] (the empty prompt, a 5-token prompt, a prompt that fills all 77 positions) -> last_hidden_state [3, 77, 768];
                    input_ids2 differs from the third prompt at position 50 only -> last_hidden_state2_row2 [77, 768] (its other two outputs are
                    asserted equal to the first run's); fp16_floor = rel-L2 of the same model evaluated with .half() against its fp32 output.
                    Asserted before writing: rows 0 .. 49 of the third prompt bitwise unchanged by the edit, rows 50 .. 76 moved by more than
                    10 x fp16_floor -- a missing causal mask cannot pass.
clip_tokenizer.json a synthetic vocabulary (byte alphabet, the same with </w>, merges that build words of the test strings, the bare </w>, the
                    two specials last), its merges, the test strings and transformers.CLIPTokenizer(vocab=, merges=)'s input_ids for them
                    (padding="max_length", max_length=77, truncation=True), encode() of each and decode() of single ids.

Usage:  python tools/make_golden_clip.py
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import clip_fixture  # noqa: E402
from motioneditor_amd.models.clip import DEFAULT_CONFIG  # noqa: E402
from motioneditor_amd.tokenizer import BOS, EOS, EOW, bytes_to_unicode  # noqa: E402

GOLD = ROOT / "tests" / "golden"

STRINGS = [
    "a girl is dancing", "a boy is dancing", "", "girl", "A Girl Is DANCING", "a  girl   is\tdancing\n", "  leading and trailing  ",
    "a man, dancing; a woman: singing!", "it's the girl's dance, isn't it?", "they're dancing, we've danced, i'm dancing, she'll dance, he'd dance",
    "3 girls and 12 boys in 2024", "room 101, 7th floor", "price: $9.99 (about 8.50 euros)", "e-mail me @ home... or not?!", "\"quoted\" and 'single' quotes",
    "a café in málaga", "el niño está bailando", "über das mädchen", "a crème brûlée, s'il vous plaît", "façade naïve coöperate",
    "under_score and CamelCase and ALLCAPS", "tabs\tand\nnewlines\r\nmixed", "a robot dancing on the moon, highly detailed, 4k", "don't can't won't 'tis",
    "hello!!!???...", "x=y+z*2/3", "100% cotton & 50% wool", "dancing dancing dancing", "spiderman is dancing on the beach",
    "an iron man is dancing in the street " * 12,      # longer than 77 tokens: truncated, last id = end-of-text
]
WORDS = ["girl", "boy", "is", "a", "dan", "ing", "dance", "man", "woman", "the", "and", "on", "in", "sing", "it", "they", "robot", "moon", "street", "iron", "beach",
         "café", "niño", "quot", "ed", "'s", "'t", "'re", "ll"]
DECODE_OF = ["a girl is dancing", "it's the girl's dance, isn't it?", "a café in málaga", "3 girls and 12 boys in 2024"]


def synthetic_vocab():
    """Byte alphabet, the same with </w>, one merge chain per word of WORDS as a word-final token (g i -> gi, gi r -> gir, gir l</w> -> girl</w>) and, for
    some, as a word-initial piece (d a -> da, da n -> dan), the bare </w>, the two specials last."""
    b2u = bytes_to_unicode()
    alphabet = [b2u[b] for b in range(256)]
    vocab = {}
    for t in alphabet + [c + EOW for c in alphabet]:
        vocab[t] = len(vocab)
    merges = []

    def chain(sym):
        while len(sym) > 1:
            pair = (sym[0], sym[1])
            if pair not in merges:
                merges.append(pair)
                vocab.setdefault(pair[0] + pair[1], len(vocab))
            sym = [sym[0] + sym[1]] + sym[2:]

    for w in WORDS:
        sym = [b2u[b] for b in w.encode("utf-8")]
        if w in ("dan", "quot", "sing"):          # pieces inside a word only
            chain(sym)
            continue
        chain(sym[:-1] + [sym[-1] + EOW])
    vocab.setdefault(EOW, len(vocab))
    vocab[BOS] = len(vocab)
    vocab[EOS] = len(vocab)
    return vocab, merges


def make_tokenizer_fixture() -> None:
    from transformers import CLIPTokenizer
    vocab, merges = synthetic_vocab()
    tok = CLIPTokenizer(vocab=dict(vocab), merges=[tuple(m) for m in merges])
    assert len(tok) == len(vocab), (len(tok), len(vocab))
    ids = tok(STRINGS, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
    assert ids.shape == (len(STRINGS), 77)
    assert int(ids[-1, -1]) == vocab[EOS] and int(ids[-1, -2]) != vocab[EOS], "the long string must be truncated"
    seen = " ".join(tok.convert_ids_to_tokens(tok.encode("a girl is dancing")))
    assert seen == f"{BOS} a</w> girl</w> is</w> danc ing</w> {EOS}", seen
    enc = [tok.encode(s) for s in STRINGS]
    dec = {}
    for s in DECODE_OF:
        for i in tok.encode(s):
            dec[str(i)] = tok.decode([i])
    out = GOLD / "clip_tokenizer.json"
    out.write_text(json.dumps(dict(vocab=vocab, merges=[list(m) for m in merges], strings=STRINGS, input_ids=ids.tolist(), encode=enc, decode_single=dec,
                                   decode_full={s: tok.decode(tok.encode(s)) for s in DECODE_OF}), ensure_ascii=True, separators=(",", ":")))
    print(out, "written:", out.stat().st_size, "bytes;", len(vocab), "tokens,", len(merges), "merges,", len(STRINGS), "strings")


def make_text_fixture() -> None:
    from transformers import CLIPTextConfig, CLIPTextModel
    c = DEFAULT_CONFIG
    cfg = CLIPTextConfig(vocab_size=c["vocab_size"], hidden_size=c["hidden_size"], intermediate_size=c["intermediate_size"], num_hidden_layers=c["num_hidden_layers"],
                         num_attention_heads=c["num_attention_heads"], max_position_embeddings=c["max_position_embeddings"], hidden_act=c["hidden_act"],
                         layer_norm_eps=c["layer_norm_eps"], bos_token_id=c["vocab_size"] - 2, eos_token_id=c["vocab_size"] - 1, pad_token_id=c["vocab_size"] - 1)
    model = CLIPTextModel(cfg).eval()
    sd = {k: torch.from_numpy(v) for k, v in clip_fixture.perturbed_state_dict().items()}
    own = [k for k in model.state_dict() if not k.endswith("position_ids")]
    prefix = "text_model." if own[0].startswith("text_model.") else ""
    missing, unexpected = model.load_state_dict({prefix + k: v for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.endswith("position_ids") for k in missing), (missing, unexpected)

    bos, eos, V = c["vocab_size"] - 2, c["vocab_size"] - 1, c["vocab_size"] - 2
    g = np.random.Generator(np.random.Philox(key=77))
    ids = np.full((3, 77), eos, dtype=np.int64)
    ids[:, 0] = bos
    ids[1, 1:6] = g.integers(0, V, 5)
    ids[2, 1:76] = g.integers(0, V, 75)
    ids2 = ids.copy()
    ids2[2, 50] = (ids[2, 50] + 12345) % V
    with torch.no_grad():
        y = model(torch.from_numpy(ids)).last_hidden_state
        y2 = model(torch.from_numpy(ids2)).last_hidden_state
        y16 = model.half()(torch.from_numpy(ids)).last_hidden_state.float()
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())   # noqa: E731
    floor = rel(y16, y)
    moved = rel(y2[2, 50:], y[2, 50:])
    print(f"fp16_floor {floor:.3e}; |max| {float(y.abs().max()):.2f}; rows 50..76 moved by {moved:.3e}")
    assert torch.equal(y2[:2], y[:2]) and torch.equal(y2[2, :50], y[2, :50]), "a change at position 50 must leave everything before it bitwise unchanged"
    assert moved > 10 * floor, (moved, floor)
    out = GOLD / "clip_text.npz"
    np.savez_compressed(out, input_ids=ids.astype(np.int32), last_hidden_state=y.numpy(), input_ids2=ids2.astype(np.int32), last_hidden_state2_row2=y2[2].numpy(),
                        fp16_floor=np.float64(floor))
    print(out, "written:", out.stat().st_size, "bytes")
    assert out.stat().st_size < (1 << 20)


if __name__ == "__main__":
    make_tokenizer_fixture()
    make_text_fixture()
