"""Cross-attention maps per prompt token on a real MI355X (MutualAttentionBase.collect_cross_attention -> ops.attention_probs, csrc/attn_probs.hip):

  * the golden forward of tests/golden/xattn_maps.npz (the REFERENCE's editor over one two-branch forward, 8 frames x 16 x 16 latents): the collected mean,
    the first entry and both aggregates.  The maps inherit the fp16 error of the activations that feed them, so the bound is the one tests/test_model_gpu.py
    holds the UNet output of that fixture to (UNET_TOL, rel-L2); measured values go to the parity record.
  * collection changes no latent (bitwise, three steps across the editors' start); the planned executor's accumulator is bitwise the eager one over those
    steps -- its first step of each gating is computed three times (warm-up, recording, replay), which the save / restore protects -- and the count after the
    first planned step is 5, not 15;
  * two targets: the rows of the targets swap with the targets; 8 frames x 32 x 32 latents with tokens = 256 (level 1, dh 80): rows sum to 1, planned ==
    eager; the graphed step refuses; examples/run_edit.py --attention-map-tokens 1 writes the two GIFs."""
import sys

import numpy as np
import pytest
import torch

from conftest import GOLD, ROOT, rel_l2
from multi_edit_common import batch_of, multi_inputs
from test_model_gpu import UNET_TOL, record

pytestmark = pytest.mark.gpu

F, HW = 8, 16


@pytest.fixture(scope="module")
def unet(unet_sd_np):
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    return UNet2DConditionModel(unet_sd_np, device="cuda")


@pytest.fixture(scope="module")
def controlnet(cn_sd_np):
    from motioneditor_amd.models.controlnet import ControlNetModel
    return ControlNetModel(cn_sd_np, device="cuda")


@pytest.fixture(scope="module")
def x():
    return multi_inputs(F, HW, HW)


@pytest.fixture
def pipe(unet, controlnet):
    from motioneditor_amd.pipelines import MotionEditorPipeline
    p = MotionEditorPipeline(unet=unet, controlnet=controlnet)
    p.scheduler.set_timesteps(50)
    yield p
    unet.spatial_editor = unet.temporal_editor = None
    p.release_plans()


def editors(holder, masks, start_step=4, cur_step=0):
    from motioneditor_amd.attn_control import (FullySelfAttentionControlMask, TemporalSelfAttentionControl,
                                               regiter_fully_attention_editor_diffusers, regiter_temporal_attention_editor_diffusers)
    ted = TemporalSelfAttentionControl(start_step=start_step, start_layer=10)
    regiter_temporal_attention_editor_diffusers(holder, ted)
    sed = FullySelfAttentionControlMask(start_step=start_step, start_layer=10, source_masks=masks)
    regiter_fully_attention_editor_diffusers(holder, sed)
    sed.cur_step = ted.cur_step = cur_step
    return sed, ted


def test_maps_vs_reference_golden(unet):
    from motioneditor_amd import synth

    class H:
        pass

    h = H()
    h.unet = unet
    g = np.load(GOLD / "xattn_maps.npz")
    c = synth.make_case_inputs("two", B=4, f=8, h=16, w=16)
    sed, ted = editors(h, c["source_masks"], cur_step=int(g["step"]))
    sed.collect_cross_attention(keep_entries=True)
    try:
        unet(c["sample"].cuda(), c["t"], c["ehs"].cuda(), down_block_additional_residuals=[d.cuda() for d in c["down_res"]], mid_block_additional_residual=c["mid_res"].cuda())
    finally:
        unet.spatial_editor = unet.temporal_editor = None
    assert sed._xa_count == int(g["entries"]) == 5 and len(sed.cross_attns) == 5
    mean = sed.cross_attention_mean()
    assert tuple(mean.shape) == (32, 256, 77) and float((mean.sum(-1) - 1).abs().max()) < 1e-5
    errs = {"mean": rel_l2(mean[torch.from_numpy(g["mean_rows"]).cuda()], torch.from_numpy(g["mean"])),
            "first": rel_l2(sed.cross_attns[0][torch.from_numpy(g["first_rows"]).cuda()], torch.from_numpy(g["first"])),
            "agg_1": rel_l2(sed.aggregate_cross_attn_map([1]), torch.from_numpy(g["agg_1"])),
            "agg_1_2": rel_l2(sed.aggregate_cross_attn_map([1, 2]), torch.from_numpy(g["agg_1_2"]))}
    for k, e in errs.items():
        print(f"xattn maps vs the reference, {k}: rel-L2 {e:.3e} (bound {UNET_TOL})")
        record(f"xattn_maps_{k}", e)
    assert max(errs.values()) <= UNET_TOL, errs


def run_steps(pipe, x, mode, collect, n_steps=3, targets=(1,), tokens=256):
    """Steps 0 .. n_steps - 1 with the editors starting at step 1 (two gatings), new embeddings every step.  Returns (latents, editor, counts per step)."""
    g = torch.Generator().manual_seed(5)
    lat0, emb0, images = batch_of(x, list(targets))
    nb = 1 + len(targets)
    uncs = [x["uncond"] + 0.05 * i * torch.randn(x["uncond"].shape, generator=g) for i in range(n_steps)]
    sed, ted = editors(pipe, x["masks"], start_step=1)
    if collect:
        sed.collect_cross_attention(tokens=tokens)
    lat, images, counts = lat0.cuda(), images.cuda(), []
    for i in range(n_steps):
        emb = torch.cat([uncs[i].expand(nb, 77, 768), emb0[nb:]]).cuda()
        fn = pipe.denoise_step if mode == "eager" else pipe.denoise_step_planned
        lat = fn(lat, pipe.scheduler.timesteps[i], emb, images, 7.5)
        counts.append(sed._xa_count)
    torch.cuda.synchronize()
    return lat.clone(), sed, counts


def test_collection_leaves_the_latents_alone_and_planned_equals_eager(pipe, x):
    off, _, _ = run_steps(pipe, x, "eager", False)
    on, sed_e, counts_e = run_steps(pipe, x, "eager", True)
    assert torch.equal(on, off), rel_l2(on, off)
    assert counts_e == [5, 10, 15]
    pipe.release_plans()
    pl, sed_p, counts_p = run_steps(pipe, x, "plan", True)
    assert counts_p == [5, 10, 15], counts_p            # the first planned step of a gating runs three times and counts once
    assert torch.equal(pl, off), rel_l2(pl, off)
    assert len(pipe._plans) == 2 and all(k[4][-1] == ("xattn", 256, id(sed_p)) for k in pipe._plans)          # collecting is part of the plan key
    acc_e, acc_p = sed_e._xa_acc[:, :77], sed_p._xa_acc[:, :77]
    assert torch.equal(acc_p, acc_e), rel_l2(acc_p, acc_e)
    m = sed_p.cross_attention_mean()
    assert tuple(m.shape) == (4 * F, 256, 77) and float((m.sum(-1) - 1).abs().max()) < 1e-5
    # a plan recorded while collecting is not replayed once collection stops (and the reverse): a third and fourth plan, the same latents
    sed_p.stop_collecting()
    before = sed_p._xa_acc.clone()
    lat = pipe.denoise_step_planned(off, pipe.scheduler.timesteps[3], torch.cat([x["uncond"].expand(2, 77, 768), x["cond"][[0, 1]]]).cuda(),
                                    batch_of(x, [1])[2].cuda(), 7.5)
    torch.cuda.synchronize()
    assert len(pipe._plans) == 3 and torch.equal(sed_p._xa_acc, before) and sed_p._xa_count == 15 and bool(torch.isfinite(lat).all())


def test_planned_step_refuses_keep_entries_and_graphed_step_refuses_collection(pipe, x):
    lat, emb, images = (t.cuda() for t in batch_of(x, [1]))
    sed, ted = editors(pipe, x["masks"], start_step=1)
    sed.collect_cross_attention(keep_entries=True)
    with pytest.raises(ValueError, match="keep_entries"):
        pipe.denoise_step_planned(lat, pipe.scheduler.timesteps[0], emb, images, 7.5)
    assert (sed.cur_step, sed.cur_att_layer, sed._xa_count) == (0, 0, 0)
    sed.collect_cross_attention()
    with pytest.raises(NotImplementedError, match="collection"):
        pipe.denoise_step_graphed(lat, pipe.scheduler.timesteps[0], emb, images, 7.5)
    assert (sed.cur_step, sed.cur_att_layer, sed._xa_count) == (0, 0, 0)


def test_two_targets_rows_follow_the_targets(pipe, x):
    """Batch [u.rec, u.e_1, u.e_2, c.rec, c.e_1, c.e_2]: rows 2 (1 + N) f.  Swapping the targets swaps their rows, bitwise; the reconstruction's stay."""
    maps = {}
    for targets in ((1, 2), (2, 1)):
        _, sed, counts = run_steps(pipe, x, "eager", True, n_steps=2, targets=targets)
        assert counts == [5, 10]
        maps[targets] = sed.cross_attention_mean().reshape(6, F, 256, 77).clone()
    a, s = maps[(1, 2)], maps[(2, 1)]
    assert float((a.sum(-1) - 1).abs().max()) < 1e-5
    for half in (0, 3):
        assert torch.equal(s[half], a[half]) and torch.equal(s[half + 1], a[half + 2]) and torch.equal(s[half + 2], a[half + 1])
    assert not torch.equal(a[4], a[5])                       # the two targets do look elsewhere


def test_level_1_maps_at_32x32_latents(pipe):
    """8 frames x 32 x 32 latents: the 256-token layers are level 1 (dh 80), five per step."""
    x32 = multi_inputs(F, 32, 32)
    _, sed_e, counts = run_steps(pipe, x32, "eager", True, n_steps=1)
    assert counts == [5]
    m = sed_e.cross_attention_mean()
    assert tuple(m.shape) == (4 * F, 256, 77) and float((m.sum(-1) - 1).abs().max()) < 1e-5
    _, sed_p, counts = run_steps(pipe, x32, "plan", True, n_steps=1)
    assert counts == [5] and torch.equal(sed_p._xa_acc[:, :77], sed_e._xa_acc[:, :77])


def test_run_edit_writes_the_attention_gifs(unet, controlnet, tmp_path, monkeypatch):
    from PIL import Image
    sys.path.insert(0, str(ROOT / "examples"))
    import run_edit
    from motioneditor_amd.models.vae import AutoencoderKL
    from motioneditor_amd.pipelines import MotionEditorPipeline
    monkeypatch.setattr(run_edit, "build_pipeline", lambda device="cuda": MotionEditorPipeline(vae=AutoencoderKL.from_synthetic("cuda"), unet=unet, controlnet=controlnet))
    monkeypatch.setattr(sys, "argv", ["run_edit.py", "--frames", "8", "--size", "128", "--steps", "2", "--inv-steps", "2", "--attention-map-tokens", "1",
                                      "--out", str(tmp_path)])
    try:
        run_edit.main()
    finally:
        unet.spatial_editor = unet.temporal_editor = None
    for name in ("attn-tokens-1-inv.gif", "attn-tokens-1.gif"):
        with Image.open(tmp_path / "sample" / name) as im:
            assert im.size == (128, 128) and im.n_frames >= 2
            im.seek(1)
            px = np.asarray(im.convert("L"))
            assert px.min() == 0 and px.max() == 255          # a min-max normalised map reaches both ends somewhere in the clip
