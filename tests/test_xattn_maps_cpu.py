"""Cross-attention maps per prompt token without a GPU: MutualAttentionBase.collect_cross_attention on the emulated C ABI (tests/emu_probe_ops.py) against
what the REFERENCE's editor collects (tests/golden/xattn_maps.npz, tools/make_golden_xattn.py: `cross_attns` of FullySelfAttentionControlMask over one
two-branch forward at 8 frames x 16 x 16 latents, five entries), within the 2e-4 that oracle/make_golden.py asserts for oracle == reference; row order, the
entry count, reset / stop / step_idx / tokens, the launch list and the counters with and without collection, and tokenizer.word_indices against the
reference's get_word_inds (tests/golden/word_indices.json)."""
import json

import numpy as np
import pytest
import torch

import emu_probe_ops
from conftest import GOLD, max_rel
from motioneditor_amd import synth
from motioneditor_amd.attn_control import (FullySelfAttentionControlMask, TemporalSelfAttentionControl,
                                           regiter_fully_attention_editor_diffusers, regiter_temporal_attention_editor_diffusers)
from motioneditor_amd.models import graph
from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel

BOUND = 2e-4      # oracle/make_golden.py: oracle == reference


class Recorder:
    """The emulated ops with every call's name appended to `calls` (the launch list of a forward)."""

    def __init__(self, mod):
        object.__setattr__(self, "mod", mod)
        object.__setattr__(self, "calls", [])

    def __getattr__(self, name):
        v = getattr(self.mod, name)
        if callable(v) and not name.startswith("_") and not isinstance(v, type):
            def logged(*a, **k):
                self.calls.append(name)
                return v(*a, **k)
            return logged
        return v


def forward(unet_sd_np, h, step, setup=None, editors=None, monkeypatch=None):
    """One two-branch forward (both editors, batch 4, 8 frames, h x h latents) on the recording emulation.  Returns (sed, ted, output, launch list)."""
    import motioneditor_amd.models.unet_2d_condition as u
    rec = Recorder(emu_probe_ops)
    mp = pytest.MonkeyPatch() if monkeypatch is None else monkeypatch
    mp.setattr(graph, "ops", rec)
    mp.setattr(u, "ops", rec)
    try:
        c = synth.make_case_inputs("two", B=4, f=8, h=h, w=h)
        if editors is None:
            unet = UNet2DConditionModel(unet_sd_np, device="cpu", dtype=torch.float32)

            class Holder:
                pass

            pipe = Holder()
            pipe.unet = unet
            ted = TemporalSelfAttentionControl(start_step=4, start_layer=10)
            regiter_temporal_attention_editor_diffusers(pipe, ted)
            sed = FullySelfAttentionControlMask(start_step=4, start_layer=10, source_masks=c["source_masks"])
            regiter_fully_attention_editor_diffusers(pipe, sed)
            ted.cur_step = sed.cur_step = step
            if setup is not None:
                setup(sed)
        else:
            unet, sed, ted = editors
        out = unet(c["sample"], c["t"], c["ehs"], down_block_additional_residuals=c["down_res"], mid_block_additional_residual=c["mid_res"]).sample
        return (unet, sed, ted), out, list(rec.calls)
    finally:
        if monkeypatch is None:
            mp.undo()


@pytest.fixture(scope="module")
def collected(unet_sd_np):
    """The golden's forward, once with collection (keep_entries) and once without; shared, never modified."""
    on = forward(unet_sd_np, 16, 4, setup=lambda sed: sed.collect_cross_attention(keep_entries=True))
    off = forward(unet_sd_np, 16, 4)
    return dict(on=on, off=off, gold=np.load(GOLD / "xattn_maps.npz"))


def test_mean_first_entry_and_aggregates_match_the_reference(collected):
    (_, sed, _), _, _ = collected["on"]
    g = collected["gold"]
    assert sed._xa_count == int(g["entries"]) == 5
    mean = sed.cross_attention_mean()
    assert mean.shape == (32, 256, 77) and mean.dtype == torch.float32
    e_mean = max_rel(mean[torch.from_numpy(g["mean_rows"])], torch.from_numpy(g["mean"]))
    e_first = max_rel(sed.cross_attns[0][torch.from_numpy(g["first_rows"])], torch.from_numpy(g["first"]))
    e_a1 = max_rel(sed.aggregate_cross_attn_map([1]), torch.from_numpy(g["agg_1"]))
    e_a12 = max_rel(sed.aggregate_cross_attn_map([1, 2]), torch.from_numpy(g["agg_1_2"]))
    print(f"emulated ABI against the reference: mean {e_mean:.3e}, first entry {e_first:.3e}, aggregate [1] {e_a1:.3e}, aggregate [1, 2] {e_a12:.3e}")
    assert max(e_mean, e_first, e_a1, e_a12) < BOUND
    # an int index is the list of one token, as in the reference
    assert torch.equal(sed.aggregate_cross_attn_map(1), sed.aggregate_cross_attn_map([1]))
    assert float((mean.sum(-1) - 1).abs().max()) < 1e-5


def test_rows_are_in_the_reference_order_and_rows_of_different_text_differ(collected):
    """Rows are "(b f)" over the full batch [u.rec, u.edit, c.rec, c.edit]: the golden's stored rows sit where the golden says; swapping two batch rows
    would put a map of another text row there (the four text rows of the fixture differ)."""
    (_, sed, _), _, _ = collected["on"]
    g = collected["gold"]
    mean = sed.cross_attention_mean()
    rows, want = g["mean_rows"].tolist(), torch.from_numpy(g["mean"])
    assert rows == [b * 8 + i for b in range(4) for i in (b, b + 4)]
    for k, r in enumerate(rows):
        wrong = (r + 8) % 32      # the same frame of the next batch row
        assert max_rel(mean[r], want[k]) < BOUND < max_rel(mean[wrong], want[k])


def test_keep_entries_fills_cross_attns_like_the_reference(collected):
    (_, sed, _), _, _ = collected["on"]
    assert len(sed.cross_attns) == 5 and all(tuple(c.shape) == (32, 256, 77) for c in sed.cross_attns)
    assert max_rel(torch.stack(sed.cross_attns, 1).mean(1), sed.cross_attention_mean()) < 1e-6


def test_collection_changes_neither_output_nor_counters_nor_the_other_launches(collected):
    (_, sed, ted), out_on, calls_on = collected["on"]
    (_, sed0, ted0), out_off, calls_off = collected["off"]
    assert torch.equal(out_on, out_off)
    assert (sed.cur_step, sed.cur_att_layer, ted.cur_step, ted.cur_att_layer) == (sed0.cur_step, sed0.cur_att_layer, ted0.cur_step, ted0.cur_att_layer) == (5, 0, 5, 0)
    # never enabled: not one probe launch; enabled: the same list with the probes inserted (two per entry with keep_entries: the sum and the entry)
    assert "attention_probs" not in calls_off and sed0._xa_acc is None and sed0.cross_attns == []
    assert calls_on.count("attention_probs") == 10
    assert [c for c in calls_on if c != "attention_probs"] == calls_off
    # each probe stands right behind the attention launch of its cross-attention
    assert all(calls_on[i - 1] in ("attention", "attention_probs") for i, c in enumerate(calls_on) if c == "attention_probs")


def test_reset_stop_and_step_idx(unet_sd_np):
    """8 x 8 latents: level 0 has 64 tokens.  step_idx = [5]: the forward of step 4 collects nothing, that of step 5 five entries; reset zeroes in place;
    after stop_collecting nothing is added and the maps stay readable."""
    ed, _, calls = forward(unet_sd_np, 8, 4, setup=lambda sed: sed.collect_cross_attention(tokens=64, step_idx=[5]))
    sed = ed[1]
    assert sed._xa_count == 0 and "attention_probs" not in calls and not sed.collects_in_step(4) and sed.collects_in_step()
    with pytest.raises(ValueError, match="no cross-attention map"):
        sed.cross_attention_mean()
    _, _, calls = forward(unet_sd_np, 8, 5, editors=ed)
    assert sed._xa_count == 5 and calls.count("attention_probs") == 5 and sed.cur_step == 6
    first = sed.cross_attention_mean().clone()
    assert first.shape == (32, 64, 77) and float((first.sum(-1) - 1).abs().max()) < 1e-5
    acc = sed._xa_acc
    sed.reset_cross_attention()
    assert sed._xa_count == 0 and sed._xa_acc is acc and float(acc.abs().max()) == 0.0
    sed.collect_cross_attention(tokens=64)               # every step from now on
    sed.cur_step = ed[2].cur_step = 5
    forward(unet_sd_np, 8, 5, editors=ed)
    assert sed._xa_count == 5 and sed._xa_acc is acc and torch.equal(sed.cross_attention_mean(), first)
    sed.stop_collecting()
    _, _, calls = forward(unet_sd_np, 8, 6, editors=ed)
    assert "attention_probs" not in calls and sed._xa_count == 5 and torch.equal(sed.cross_attention_mean(), first)
    with pytest.raises(ValueError, match="tokens"):
        sed.collect_cross_attention(tokens=256)


def test_tokens_64_collects_the_level_1_layers(unet_sd_np):
    ed, _, calls = forward(unet_sd_np, 16, 4, setup=lambda sed: sed.collect_cross_attention(tokens=64))
    sed = ed[1]
    assert sed._xa_count == 5 and calls.count("attention_probs") == 5         # two down and three up transformer blocks at 8 x 8 tokens
    m = sed.cross_attention_mean()
    assert m.shape == (32, 64, 77) and float((m.sum(-1) - 1).abs().max()) < 1e-5
    assert sed.aggregate_cross_attn_map([1, 2]).shape == (32, 8, 8)


def test_a_constant_map_divides_by_zero_as_in_the_reference():
    from motioneditor_amd.attn_control import MutualAttentionBase
    ed = MutualAttentionBase()
    ed._xa_acc, ed._xa_items, ed._xa_tokens, ed._xa_count = torch.full((2 * 16, 80), 0.25), 2, 16, 1
    assert torch.isnan(ed.aggregate_cross_attn_map([1])).all()


def test_mask_save_dir_writes_the_edit_rows(unet_sd_np, tmp_path):
    def setup(sed):
        sed.mask_save_dir = str(tmp_path)
        sed.collect_cross_attention(tokens=64)
    ed, _, _ = forward(unet_sd_np, 8, 4, setup=setup)
    names = sorted(p.name for p in tmp_path.iterdir())
    assert names == [f"cross_attn_step005_row{r:03d}.png" for r in ed[1].edit_rows()] and ed[1].edit_rows() == list(range(8, 16)) + list(range(24, 32))
    import PIL.Image
    assert PIL.Image.open(tmp_path / names[0]).size == (8, 8)


def test_word_indices_match_the_reference():
    from motioneditor_amd.tokenizer import CLIPTokenizer
    tg = json.loads((GOLD / "clip_tokenizer.json").read_text())
    tok = CLIPTokenizer(vocab=tg["vocab"], merges=tg["merges"])
    cases = json.loads((GOLD / "word_indices.json").read_text())["cases"]
    assert any(len(c["indices"]) == 2 and isinstance(c["word"], str) for c in cases) and any(c["indices"] == [] for c in cases) and any(len(c["indices"]) == 4 for c in cases)
    for c in cases:
        assert tok.word_indices(c["text"], c["word"]) == c["indices"], c


def test_save_attention_maps_writes_nearest_upsampled_grey_frames(monkeypatch, tmp_path):
    import PIL.Image
    import emu_image_ops
    from motioneditor_amd import util
    monkeypatch.setattr(util, "ops", emu_image_ops)
    monkeypatch.setattr(util, "UPLOAD_DEVICE", "cpu")
    maps = torch.zeros(1, 3, 2, 2)
    maps[0, 0, 0, 1] = maps[0, 1, 1, 0] = maps[0, 2, 1, 1] = 1.0        # (three different frames: PIL merges equal neighbours)
    maps[0, 1, 0, 0] = float("nan")                                      # a constant map's 0 / 0: shown black
    path = util.save_attention_maps(maps, str(tmp_path / "a" / "attn.gif"), size=8, fps=4)
    im = PIL.Image.open(path)
    assert im.n_frames == 3 and im.size == (8, 8) and im.info["duration"] == 250
    px = np.asarray(im.convert("L"))
    assert (px[:4, 4:] == 255).all() and (px[:4, :4] == 0).all() and (px[4:] == 0).all()
    im.seek(1)
    px = np.asarray(im.convert("L"))
    assert (px[4:, :4] == 255).all() and (px[:4] == 0).all() and (px[4:, 4:] == 0).all()
    with pytest.raises(ValueError):
        util.save_attention_maps(maps[0], str(tmp_path / "b.gif"))
