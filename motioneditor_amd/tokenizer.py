"""CLIP's tokenizer on the host, standard library only: lower-casing byte-level BPE with `</w>` word ends, `<|startoftext|>` /
`<|endoftext|>`, pad = end-of-text, 77 positions.  The surface is what the reference calls on `transformers.CLIPTokenizer`
(pipeline_motion_editor.py:262-274, util.py:59-71, ptp_utils.py:281-299) and nothing more:

    tok(texts, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids      int64 [n, 77]
    tok.encode(text)   ids with the two specials        tok.decode(ids)   text (`get_word_inds` decodes single ids)
    tok.model_max_length, len(tok)

Text is normalised as CLIP does (NFC, runs of white space -> one blank, lower case) and split by CLIP's pattern
    <|startoftext|> | <|endoftext|> | 's | 't | 're | 've | 'm | 'll | 'd | \\p{L}+ | \\p{N} | [^\\s\\p{L}\\p{N}]+
Python's `re` has no \\p{..} classes, so the split is a scanner over `unicodedata.category`: a letter is a character of a category
L*, a number one of N*, which is the definition of \\p{L} / \\p{N}.  What can differ from a tokenizer built on the `regex` /
`tokenizers` libraries: the Unicode version of the tables (this interpreter's `unicodedata` against theirs: characters assigned
or re-classified between the two versions), white space (`str.isspace` counts the information separators U+001C..U+001F, the
White_Space property behind \\s does not), and `str.lower` against Rust's `to_lowercase` on a handful of special-casing code
points.  ASCII and Latin-1 / Latin Extended text -- English prompts, accented words -- is split identically
(tests/golden/clip_tokenizer.json).
"""
from __future__ import annotations

import json
import unicodedata
from pathlib import Path
from types import SimpleNamespace
from typing import Dict, Iterable, List, Sequence, Tuple, Union

BOS, EOS = "<|startoftext|>", "<|endoftext|>"
EOW = "</w>"
_CONTRACTIONS = ("'s", "'t", "'re", "'ve", "'m", "'ll", "'d")     # in the pattern's order: the first alternative that matches wins


def bytes_to_unicode() -> Dict[int, str]:
    """GPT-2's byte alphabet: the printable Latin-1 bytes stand for themselves, the other 68 are mapped to U+0100 onwards."""
    keep = set(range(ord("!"), ord("~") + 1)) | set(range(0xA1, 0xAC + 1)) | set(range(0xAE, 0xFF + 1))
    out, n = {}, 0
    for b in range(256):
        if b in keep:
            out[b] = chr(b)
        else:
            out[b] = chr(256 + n)
            n += 1
    return out


def _normalise(text: str) -> str:
    """NFC, \\s+ -> one blank, lower case."""
    out, blank = [], False
    for ch in unicodedata.normalize("NFC", text):
        if ch.isspace():
            if not blank:
                out.append(" ")
            blank = True
        else:
            out.append(ch)
            blank = False
    return "".join(out).lower()


def _split(text: str) -> List[str]:
    """CLIP's pattern over normalised text, as a scanner (module docstring)."""
    out, i, n = [], 0, len(text)
    while i < n:
        ch = text[i]
        if ch.isspace():
            i += 1
            continue
        fixed = next((s for s in (BOS, EOS) + _CONTRACTIONS if text.startswith(s, i)), None)
        if fixed is not None:
            out.append(fixed)
            i += len(fixed)
            continue
        cat = unicodedata.category(ch)[0]
        j = i + 1
        if cat == "L":
            while j < n and unicodedata.category(text[j])[0] == "L":
                j += 1
        elif cat != "N":     # (a number is one character per token)
            while j < n and not text[j].isspace() and unicodedata.category(text[j])[0] not in "LN":
                j += 1
        out.append(text[i:j])
        i = j
    return out


class CLIPTokenizer:
    def __init__(self, vocab_file=None, merges_file=None, *, vocab: Dict[str, int] = None, merges: Sequence = None, model_max_length: int = 77):
        """`vocab_file` / `merges_file`: the `vocab.json` / `merges.txt` of a checkpoint's `tokenizer/` folder; or the same contents as `vocab` (token ->
        id) and `merges` ("a b" strings or pairs, best first)."""
        if vocab is None:
            vocab = json.loads(Path(vocab_file).read_text(encoding="utf-8"))
        if merges is None:
            lines = Path(merges_file).read_text(encoding="utf-8").split("\n")
            merges = [ln for ln in lines if ln.strip() and not ln.startswith("#version")]
        self.encoder: Dict[str, int] = dict(vocab)
        self.decoder: Dict[int, str] = {i: t for t, i in self.encoder.items()}
        pairs = [tuple(m.split()) if isinstance(m, str) else tuple(m) for m in merges]
        if any(len(p) != 2 for p in pairs):
            raise ValueError("CLIPTokenizer: every merge must name two symbols")
        self.ranks: Dict[Tuple[str, str], int] = {p: r for r, p in enumerate(pairs)}
        for sp in (BOS, EOS):
            if sp not in self.encoder:
                raise ValueError(f"CLIPTokenizer: the vocabulary lacks {sp}")
        self.bos_token, self.eos_token, self.pad_token, self.unk_token = BOS, EOS, EOS, EOS
        self.bos_token_id = self.encoder[BOS]
        self.eos_token_id = self.pad_token_id = self.unk_token_id = self.encoder[EOS]
        self.model_max_length = int(model_max_length)
        self._b2u = bytes_to_unicode()
        self._u2b = {u: b for b, u in self._b2u.items()}
        self._cache: Dict[str, List[str]] = {}

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, subfolder="tokenizer", **kwargs) -> "CLIPTokenizer":
        """transformers' signature for a local directory (inference.py:151: CLIPTokenizer.from_pretrained(path, subfolder="tokenizer"))."""
        d = Path(pretrained_model_name_or_path) / subfolder if subfolder else Path(pretrained_model_name_or_path)
        for f in ("vocab.json", "merges.txt"):
            if not (d / f).exists():
                raise FileNotFoundError(f"{d / f} not found")
        n = 77
        cfg = d / "tokenizer_config.json"
        if cfg.exists():
            n = int(json.loads(cfg.read_text(encoding="utf-8")).get("model_max_length", 77))
        return cls(d / "vocab.json", d / "merges.txt", model_max_length=n)

    @classmethod
    def from_synthetic(cls) -> "CLIPTokenizer":
        """A small vocabulary for runs without a checkpoint (examples/): the byte alphabet, the same with `</w>`, the two specials, no merges --
        every string tokenises, one token per byte."""
        alphabet = list(bytes_to_unicode().values())
        vocab = {t: i for i, t in enumerate(alphabet + [c + EOW for c in alphabet] + [BOS, EOS])}
        return cls(vocab=vocab, merges=[])

    def __len__(self) -> int:
        return len(self.encoder)

    # -- text -> ids
    def _bpe(self, word: str) -> List[str]:
        """The symbols of one pre-token: its UTF-8 bytes in the byte alphabet, `</w>` on the last, then the best-ranked adjacent pair merged until
        no pair of the word is a known merge."""
        hit = self._cache.get(word)
        if hit is not None:
            return hit
        sym = [self._b2u[b] for b in word.encode("utf-8")]
        sym[-1] += EOW
        while len(sym) > 1:
            best, at = None, -1
            for k in range(len(sym) - 1):
                r = self.ranks.get((sym[k], sym[k + 1]))
                if r is not None and (best is None or r < best):
                    best, at = r, k
            if best is None:
                break
            a, b = sym[at], sym[at + 1]
            merged, k = [], 0
            while k < len(sym):       # every occurrence of the pair, left to right
                if k < len(sym) - 1 and sym[k] == a and sym[k + 1] == b:
                    merged.append(a + b)
                    k += 2
                else:
                    merged.append(sym[k])
                    k += 1
            sym = merged
        self._cache[word] = sym
        return sym

    def tokenize(self, text: str) -> List[str]:
        out: List[str] = []
        for piece in _split(_normalise(text)):
            if piece in (BOS, EOS):
                out.append(piece)
            else:
                out.extend(self._bpe(piece))
        return out

    def convert_tokens_to_ids(self, tokens: Iterable[str]) -> List[int]:
        return [self.encoder.get(t, self.unk_token_id) for t in tokens]

    def encode(self, text: str, max_length: int = None, truncation: bool = False) -> List[int]:
        """<|startoftext|> + the tokens of `text` + <|endoftext|>; truncation to max_length keeps the end-of-text token last."""
        ids = [self.bos_token_id] + self.convert_tokens_to_ids(self.tokenize(text)) + [self.eos_token_id]
        if truncation and max_length is not None and len(ids) > max_length:
            ids = ids[:max_length - 1] + [self.eos_token_id]
        return ids

    # -- ids -> text
    def decode(self, ids) -> str:
        if hasattr(ids, "tolist"):
            ids = ids.tolist()
        if isinstance(ids, int):
            ids = [ids]
        toks = []
        for i in ids:
            if int(i) not in self.decoder:
                raise ValueError(f"CLIPTokenizer.decode: id {i} is outside the vocabulary of {len(self)} tokens")
            toks.append(self.decoder[int(i)])
        raw = bytearray()
        for ch in "".join(toks):
            b = self._u2b.get(ch)
            raw.extend(bytes([b]) if b is not None else ch.encode("utf-8"))
        return raw.decode("utf-8", errors="replace").replace(EOW, " ").strip()

    # -- word -> token positions
    def word_indices(self, text: str, word) -> List[int]:
        """Positions (1-based: 0 is the start token) of the tokens of `word` in the encoding of `text`: get_word_inds of the reference
        (inference.py:52-71, p2p/seq_aligner.py:118-136).  `word` is a word of `text.split(" ")` (every occurrence counts), or an int: the place of the
        word in that split.  A word the prompt does not hold gives []; a word of several tokens gives every one of them.  Tokens are assigned
        to the split words by length: a word is complete once the decoded tokens since the last word boundary cover its characters."""
        words = text.split(" ")
        wanted = {i for i, w in enumerate(words) if w == word} if isinstance(word, str) else ({int(word)} if isinstance(word, int) else {int(i) for i in word})
        if not wanted:
            return []
        pieces = [self.decode([i]).strip("#") for i in self.encode(text)[1:-1]]
        hits: List[int] = []
        at, seen = 0, 0                      # the split word being spelt, and how many of its characters the tokens so far have covered
        for pos, piece in enumerate(pieces, start=1):
            if at >= len(words):
                break
            if at in wanted:
                hits.append(pos)
            seen += len(piece)
            if seen >= len(words[at]):
                at, seen = at + 1, 0
        return hits

    # -- the call of the pipeline
    def __call__(self, text: Union[str, Sequence[str]], padding="max_length", max_length: int = None, truncation: bool = True, return_tensors: str = "pt"):
        if padding != "max_length" or return_tensors != "pt":
            raise NotImplementedError(f"CLIPTokenizer: padding={padding!r}, return_tensors={return_tensors!r} (the reference pads to max_length and asks for 'pt')")
        import torch
        n = self.model_max_length if max_length is None else int(max_length)
        rows = []
        for t in ([text] if isinstance(text, str) else list(text)):
            ids = self.encode(t, max_length=n, truncation=bool(truncation))
            if len(ids) > n:
                raise ValueError(f"CLIPTokenizer: {len(ids)} tokens exceed max_length={n} and truncation is off")
            rows.append(ids + [self.pad_token_id] * (n - len(ids)))
        return SimpleNamespace(input_ids=torch.tensor(rows, dtype=torch.int64))
