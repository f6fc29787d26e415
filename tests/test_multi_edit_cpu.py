"""One clip edited towards several targets in ONE denoising pass, on the emulated C ABI (tests/emu_ops.py): the UNet batch is [rec, e_1 .. e_N] per
classifier-free-guidance half, and (rec, e_k) must be what the oracle's separate two-row step of (source, target k) gives (oracle/ref_cpu.denoise_step), at the
geometry and to the bound of tests/test_step_cpu.py.  N = 3 is an odd batch half: a leftover `b % 2` finds itself there."""
import pytest
import torch

import emu_ops
from conftest import max_rel
from motioneditor_amd import schedulers, segments
from motioneditor_amd.attn_control import (FullySelfAttentionControlMask, TemporalSelfAttentionControl,
                                           regiter_fully_attention_editor_diffusers, regiter_temporal_attention_editor_diffusers)
from motioneditor_amd.capi import SEG_DUAL_BIN, SEG_DUAL_CUR, SEG_DUAL_PREV, SEG_PLAIN
from motioneditor_amd.models import graph
from motioneditor_amd.models.controlnet import ControlNetModel
from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
from motioneditor_amd.pipelines import MotionEditorPipeline
from multi_edit_common import batch_of, multi_inputs, oracle_pair

BOUND = 2e-4    # tests/test_step_cpu.py: max |got - want| / mean |want| of the emulated-ABI step against the oracle


@pytest.fixture
def emu(monkeypatch):
    import motioneditor_amd.models.unet_2d_condition as u
    import motioneditor_amd.pipelines.pipeline_motion_editor as pm
    for m in (graph, u, pm, schedulers):
        monkeypatch.setattr(m, "ops", emu_ops)


@pytest.fixture(scope="module")
def models(unet_sd_np, cn_sd_np):
    return (UNet2DConditionModel(unet_sd_np, device="cpu", dtype=torch.float32), ControlNetModel(cn_sd_np, device="cpu", dtype=torch.float32))


def make_pipe(models, masks, step=0):
    unet, cn = models
    pipe = MotionEditorPipeline(unet=unet, controlnet=cn)
    ted = TemporalSelfAttentionControl(start_step=4, start_layer=10)
    regiter_temporal_attention_editor_diffusers(pipe, ted)
    sed = FullySelfAttentionControlMask(start_step=4, start_layer=10, source_masks=masks)
    regiter_fully_attention_editor_diffusers(pipe, sed)
    ted.cur_step = sed.cur_step = step
    pipe.scheduler.set_timesteps(50)
    return pipe, sed, ted


@pytest.mark.parametrize("step", [4, 0], ids=["editors-active", "editors-inactive"])
@pytest.mark.parametrize("n", [2, 3])
def test_batched_step_equals_the_separate_two_row_steps(emu, models, unet_sd_torch, cn_sd_torch, n, step):
    """ControlNet + adapter + both editors (gated active at step 4, inactive at step 0): every (rec, e_k) of the batched step against the oracle's own
    two-row step of target k."""
    x = multi_inputs()
    pipe, sed, ted = make_pipe(models, x["masks"], step)
    lat, emb, images = batch_of(x, range(1, n + 1))
    got = pipe.denoise_step(lat, pipe.scheduler.timesteps[step], emb, images, 7.5)
    assert got.shape == lat.shape
    # counters advance once per attention layer and step, whatever N is
    assert (sed.cur_step, sed.cur_att_layer, ted.cur_step, ted.cur_att_layer) == (step + 1, 0, step + 1, 0)
    for k in range(1, n + 1):
        want, _ = oracle_pair(x, "cpu8", k, step, unet_sd_torch, cn_sd_torch)
        e_rec, e_edit = max_rel(got[0], want[0]), max_rel(got[k], want[1])
        print(f"N={n} step={step} target {k}: rec {e_rec:.2e} edit {e_edit:.2e}")
        assert e_rec < BOUND and e_edit < BOUND, (k, e_rec, e_edit)
    if step == 4:   # the targets are different edits
        assert max_rel(got[1], got[2]) > 1e-2


def test_n3_without_the_controlnet_dedup(emu, models, unet_sd_torch, cn_sd_torch):
    """dedup_controlnet = False executes one ControlNet entry per (guidance copy, target) as the reference would: the same step."""
    x = multi_inputs()
    pipe, sed, ted = make_pipe(models, x["masks"], 4)
    pipe.dedup_controlnet = False
    lat, emb, images = batch_of(x, (1, 2, 3))
    got = pipe.denoise_step(lat, pipe.scheduler.timesteps[4], emb, images, 7.5)
    for k in (1, 2, 3):
        want, _ = oracle_pair(x, "cpu8", k, 4, unet_sd_torch, cn_sd_torch)
        assert max_rel(got[0], want[0]) < BOUND and max_rel(got[k], want[1]) < BOUND, k


def test_segment_tables_for_three_targets():
    """edited_spatial and the temporal kv_map at N = 3: sources, modes, order, and no edit item that references another edit."""
    f, n = 4, 3
    br = segments.Branches.targets(n)
    B = 2 * (1 + n)
    assert br.src == (0, 0, 0, 0, 4, 4, 4, 4) and br.edit_rows == (1, 2, 3, 5, 6, 7) and br.edits_of(4) == (5, 6, 7)
    assert segments.Branches.targets(1) == segments.Branches.pairs(4) and segments.Branches.pairs(2).src == (0, 0)
    with pytest.raises(ValueError):
        segments.Branches((0, 0, 1))        # an edit naming an edit as its source
    for binary in (True, False):
        item, mode = segments.edited_spatial(f, "cpu", binary, B, None, br)
        item, mode = item.tolist(), mode.tolist()
        dual = [SEG_DUAL_BIN, SEG_DUAL_BIN] if binary else [SEG_DUAL_PREV, SEG_DUAL_CUR]
        for b in range(B):
            s = br.src[b]
            for g in range(f):
                if s == b:
                    assert item[b * f + g] == [b * f + max(g - 1, 0), b * f + g, -1] and mode[b * f + g] == [SEG_PLAIN] * 3
                else:
                    assert item[b * f + g] == [s * f + max(g - 1, 0), s * f + g, b * f + g] and mode[b * f + g] == dual + [SEG_PLAIN]
                    others = {e * f + i for e in br.edit_rows if e != b for i in range(f)}
                    assert not others & set(item[b * f + g])
        order = segments.ITEM_ORDER[segments.edited_spatial(f, "cpu", binary, B, None, br)[0].data_ptr()].tolist()
        # source frame g, then every edit's frame g: half by half
        assert order == [b * f + g for s in (0, 4) for g in range(f) for b in range(s, s + 4)]
    # the pair's table is the object it was before there was a branch description
    assert segments.edited_spatial(f, "cpu", True, 4, None, segments.Branches.targets(1))[0] is segments.edited_spatial(f, "cpu", True, 4)[0]

    class Call:
        B, branches = 8, br

        def run(self, kv_map=None):
            return kv_map

    ted = TemporalSelfAttentionControl(start_step=0, start_layer=0)
    ted.num_att_layers = 16
    assert ted(call=Call(), is_cross=False, place_in_unet="down", num_heads=8) == [0, 0, 0, 0, 4, 4, 4, 4]
    Call.B, Call.branches = 10, segments.Branches.targets(4)
    with pytest.raises(ValueError, match="8 batch rows"):
        ted(call=Call(), is_cross=False, place_in_unet="down", num_heads=8)
    Call.B, Call.branches = 6, None            # no description and not a pair layout
    with pytest.raises(ValueError):
        ted(call=Call(), is_cross=False, place_in_unet="down", num_heads=8)


def test_call_shapes_errors_and_the_shared_skeleton_form(emu, models):
    x = multi_inputs()
    f = x["latents"].shape[2]
    pipe, sed, ted = make_pipe(models, x["masks"])
    sed.step_idx = ted.step_idx = [0]          # editors active in the one step
    lat, cond = x["latents"][:3] * 0.5, x["cond"][:3]
    z = torch.zeros_like(x["skeletons"][0])
    s1 = x["skeletons"][0]
    kw = dict(video_length=f, height=64, width=64, num_inference_steps=1, guidance_scale=7.5, uncond_embeddings=[x["uncond"]], output_type="latent")

    def run(prompts, **k):
        sed.reset(), ted.reset()
        return pipe(prompts, **{**kw, **k}).images

    six = run(["src", "t1", "t2"], latents=lat, text_embeddings=cond, skeleton=torch.stack([z, s1, s1, z, s1, s1]))
    assert six.shape == (3, 4, f, 8, 8) and bool(torch.isfinite(six).all())
    assert (sed.cur_step, ted.cur_step) == (1, 1)
    four = run(["src", "t1", "t2"], latents=lat, text_embeddings=cond, skeleton=torch.stack([z, s1, z, s1]))
    assert max_rel(four, six) < 1e-5            # one skeleton shared by both targets == the same skeleton given twice (up to BLAS blocking)
    assert max_rel(six[1], six[2]) > 1e-3       # ... and the two targets still differ (prompts)
    with pytest.raises(ValueError, match="3 rows"):
        run(["src", "t1", "t2"], latents=lat[:2], text_embeddings=cond, skeleton=torch.stack([z, s1, z, s1]))
    with pytest.raises(ValueError, match="6 entries"):
        run(["src", "t1", "t2"], latents=lat, text_embeddings=cond, skeleton=torch.stack([z, s1, s1, z, s1]))
    with pytest.raises(ValueError, match="at most 3 targets"):
        run(["src", "a", "b", "c", "d"], latents=x["latents"][[0, 1, 2, 3, 1]], text_embeddings=x["cond"][[0, 1, 2, 3, 1]], skeleton=torch.stack([z, s1, z, s1]))
    with pytest.raises(NotImplementedError):
        run(["src"], latents=lat[:1], text_embeddings=cond[:1], skeleton=torch.stack([z, s1, z, s1]))
    for fn in (pipe.denoise_step_graphed,):
        with pytest.raises(NotImplementedError, match="N > 1"):
            fn(lat, 1, torch.cat([cond, cond]), None, 7.5)
    with pytest.raises(NotImplementedError, match="N > 1"):
        pipe.denoise_step_cfg_parallel(lat, 1, torch.cat([cond, cond]), None, 7.5)
    with pytest.raises(NotImplementedError, match="N > 1"):
        pipe.denoise_step_frame_sharded(lat, 1, torch.cat([cond, cond]), None, 7.5, shard=None)


def test_run_edit_takes_several_target_prompts_and_writes_one_gif_per_target(monkeypatch, tmp_path):
    """examples/run_edit.py: --target-prompt several times; sample/{target}.gif per target plus one -inv.gif (a single target: the two files as before)."""
    import sys
    import emu_image_ops as emu_img
    from conftest import ROOT
    from motioneditor_amd import ops, util
    monkeypatch.syspath_prepend(str(ROOT / "examples"))
    monkeypatch.setattr(ops, "image_resize", emu_img.image_resize)
    monkeypatch.setattr(ops, "video_grid_u8", emu_img.video_grid_u8)
    monkeypatch.setattr(util, "UPLOAD_DEVICE", "cpu")
    import run_edit
    a = run_edit.parser().parse_args(["--prompt", "a girl", "--target-prompt", "a boy", "--target-prompt", "a robot", "--out", str(tmp_path)])
    assert a.target_prompt == ["a boy", "a robot"] and run_edit.parser().parse_args([]).target_prompt is None
    v = torch.rand(3, 3, 4, 32, 32, generator=torch.Generator().manual_seed(1))
    paths = run_edit.save_samples(a.out, a.target_prompt, v[:1], v[1:])
    assert paths == [f"{a.out}/sample/a boy.gif", f"{a.out}/sample/a robot.gif", f"{a.out}/sample/a boy-inv.gif"]
    assert all(__import__("os").path.isfile(p) for p in paths)
    assert run_edit.save_samples(a.out, "one", v[:1], v[1:2]) == [f"{a.out}/sample/one.gif", f"{a.out}/sample/one-inv.gif"]
    with pytest.raises(ValueError):
        run_edit.save_samples(a.out, ["one"], v[:1], v[1:])
    assert run_edit.extra_target_embeddings(3).shape == (2, 77, 768)
