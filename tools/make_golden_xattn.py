"""Generate tests/golden/xattn_maps.npz and tests/golden/word_indices.json from the REFERENCE's own code (generation time only: it needs the reference
tree and the stub packages of oracle/shim, neither of which a test touches).

xattn_maps.npz: the reference UNet, two-branch with both editors registered (FullySelfAttentionControlMask, TemporalSelfAttentionControl, active step 4),
batch 4 = [u.rec, u.edit, c.rec, c.edit], 8 frames x 16 x 16 latents, the synthetic weights and the `two` inputs of tests/golden/unet_two_active.npz at that
size.  Level 0 has 16 * 16 = 256 tokens (dh 40): its two down and three up transformer blocks each append their head-mean text cross-attention map
[32, 256, 77] to the editor's `cross_attns` (fully_control.py:430-432) -- five entries per forward.  Stored:
    mean        torch.stack(cross_attns, 1).mean(1), frames {b, b + 4} of batch row b (every frame occurs once)       [8, 256, 77]
    first       cross_attns[0] (the first down block: the layer that runs on the shared CFG prefix here), frame b + 2  [4, 256, 77]
    agg_1       aggregate_cross_attn_map([1]) (fully_control.py:257-268), every row                                   [32, 16, 16]
    agg_1_2     aggregate_cross_attn_map([1, 2])                                                                      [32, 16, 16]
    mean_rows / first_rows: the "(b f)" rows stored; entries = 5; step = 4
The maps are fp32, not fp16: with these weights every probability lies near 1 / 77 = 0.013, where half an fp16 ulp (3.8e-6) is 2.9e-4 of the mean -- more
than the 2e-4 the maps are compared within (oracle/make_golden.py's bound for oracle == reference).  Fewer rows keep the file below the size limit instead.

word_indices.json: get_word_inds (inference.py:52-71) of the reference on a handful of prompts, with this project's tokenizer on the committed test
vocabulary (tests/golden/clip_tokenizer.json): a word of two tokens, a repeated word, a missing word, an integer place.

Usage:  python tools/make_golden_xattn.py
"""
from __future__ import annotations

import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from oracle import make_golden as mg  # noqa: E402  (puts oracle/shim and the reference on sys.path)
from motioneditor_amd import synth  # noqa: E402
from motioneditor_amd.synth import make_case_inputs  # noqa: E402
from motioneditor_amd.tokenizer import CLIPTokenizer  # noqa: E402

GOLD = ROOT / "tests" / "golden"
STEP = 4

WORD_CASES = [("a girl is dancing", "girl"), ("a girl is dancing", "dancing"), ("a girl is dancing", "boy"), ("a girl and a girl", "girl"),
              ("the man is dancing and the woman is dancing", "dancing"), ("a boy is dancing", "a"), ("a girl is dancing", 2), ("a girl is dancing", 3),
              ("girl", "girl"), ("a man, dancing; a woman: singing!", "man,"), ("a man, dancing; a woman: singing!", "man")]


def word_indices_golden():
    tg = json.loads((GOLD / "clip_tokenizer.json").read_text())
    tok = CLIPTokenizer(vocab=tg["vocab"], merges=tg["merges"])
    get_word_inds = mg._ref_function(mg.REF / "inference.py", "get_word_inds")
    cases = []
    for text, word in WORD_CASES:
        got = mg.quiet(get_word_inds, text, word, tok)
        cases.append({"text": text, "word": word, "indices": [int(i) for i in got], "tokens": [tok.decode([i]) for i in tok.encode(text)]})
    (GOLD / "word_indices.json").write_text(json.dumps({"vocabulary": "tests/golden/clip_tokenizer.json", "cases": cases}, indent=1, ensure_ascii=False) + "\n")
    print("word_indices.json written:", [(c["word"], c["indices"]) for c in cases])


def maps_golden():
    sd_np = synth.synth_state_dict(synth.unet_schema())
    unet = mg.build_reference_unet(sd_np)
    from motion_editor.attn_control.fully_control import FullySelfAttentionControlMask, FullySelfAttentionControlMaskAuto
    from motion_editor.attn_control.fully_control_utils import regiter_fully_attention_editor_diffusers
    from motion_editor.attn_control.temporal_control import TemporalSelfAttentionControl
    from motion_editor.attn_control.temporal_control_utils import regiter_temporal_attention_editor_diffusers
    cb = make_case_inputs("two", B=4, f=8, h=16, w=16)

    class Holder:
        pass

    holder = Holder()
    holder.unet = unet
    ted = mg.quiet(TemporalSelfAttentionControl, start_step=4, start_layer=10)
    mg.quiet(regiter_temporal_attention_editor_diffusers, holder, ted)
    sed = mg.quiet(FullySelfAttentionControlMask, start_step=4, start_layer=10, source_masks=cb["source_masks"])
    mg.quiet(regiter_fully_attention_editor_diffusers, holder, sed)
    ted.reset(); sed.reset()
    ted.cur_step = sed.cur_step = STEP
    sed.cross_attns = []
    with torch.no_grad():
        t0 = time.time()
        out = mg.quiet(unet, cb["sample"], torch.tensor(cb["t"]), cb["ehs"], down_block_additional_residuals=cb["down_res"], mid_block_additional_residual=cb["mid_res"]).sample
        print(f"reference two-branch forward, editors active, 8 f x 16x16 (B = 4): {time.time() - t0:.0f} s")
    assert len(sed.cross_attns) == 5 and all(tuple(c.shape) == (32, 256, 77) for c in sed.cross_attns), [tuple(c.shape) for c in sed.cross_attns]
    mean = torch.stack(sed.cross_attns, dim=1).mean(1)
    assert float((mean.sum(-1) - 1).abs().max()) < 1e-5
    aggregate = FullySelfAttentionControlMaskAuto.aggregate_cross_attn_map      # (the method lives on the ...MaskAuto sibling, :257-268; it reads self.cross_attns only)
    agg_1, agg_12 = aggregate(sed, [1]), aggregate(sed, [1, 2])
    mean_rows = np.array([b * 8 + i for b in range(4) for i in (b, b + 4)])
    first_rows = np.array([b * 8 + b + 2 for b in range(4)])
    path = GOLD / "xattn_maps.npz"
    np.savez_compressed(path, mean=mean[mean_rows].numpy().astype(np.float32), first=sed.cross_attns[0][first_rows].numpy().astype(np.float32),
                        agg_1=agg_1.numpy().astype(np.float32), agg_1_2=agg_12.numpy().astype(np.float32), mean_rows=mean_rows, first_rows=first_rows,
                        entries=5, step=STEP, out_stats=mg.stats(out))
    print(f"xattn_maps.npz written: {path.stat().st_size} bytes; mean range [{float(mean.min()):.3e}, {float(mean.max()):.3e}]")
    assert path.stat().st_size < (1 << 20)


if __name__ == "__main__":
    torch.manual_seed(0)
    word_indices_golden()
    maps_golden()
