"""Clips longer than 64 frames, without a GPU: the case table of tests/long_clip_cases.py against itself and against the restated dispatch, the INPUTS of
every case (the fp32 emulation of tests/fwd_run.py lands inside the bound tests/test_long_clip_gpu.py applies to tattn_long_kernel on the same tensors; the
rising inputs move the running maximum in every stage, the falling ones leave it in the first), the refusal above 256 frames on the host, and one 72-frame
denoising step of the product pipeline on the emulated ABI against the oracle (the host path: nothing but me_tattn depended on the frame count)."""
import ctypes

import pytest
import torch

import fwd_cases as fc
import fwd_run as fr
import long_clip_cases as lc
import ref64_fwd as ref


def test_the_table_holds_every_edge_and_the_restated_dispatch_predicts_it():
    ids = [c.id for c in lc.CASES]
    assert len(ids) == len(set(ids))
    assert {c.path for c in lc.CASES} == set(lc.LONG_TARGETS)
    assert all(c.path == lc.tattn_target(c.p) and c.entry == "temporal_attention" and c.bound is None and c.twice for c in lc.CASES)
    edges = {(c.p["dh"], c.p["frames"], c.p["kind"]) for c in lc.CASES if "kind" in c.p}
    assert edges == {(dh, F, k) for dh in lc.LONG_DH for F in lc.FRAME_EDGES for k in lc.KINDS}
    assert set(lc.GUARDED) <= set(lc.BY_ID)
    # the dispatch: at and below 64 frames what fwd_cases states, the key-tiled kernel up to 256, nothing beyond; other head sizes as before
    for dh in lc.LONG_DH:
        assert lc.tattn_target(dict(dh=dh, frames=64)) == fc.tattn_target(dict(dh=dh, frames=64)) == f"tattn_mfma_kernel<{dh},64>"
        assert lc.tattn_target(dict(dh=dh, frames=65)) == lc.tattn_target(dict(dh=dh, frames=256)) == f"tattn_long_kernel<{dh}>"
        assert lc.tattn_target(dict(dh=dh, frames=257)) is None
    assert lc.tattn_target(lc.REFUSED_FRAMES) is None
    assert lc.tattn_target(dict(dh=32, frames=72)) is None and lc.tattn_target(dict(dh=32, frames=48)) == "tattn_kernel<48>"
    assert all(lc.tattn_target(c.p) == c.path for c in fc.CASES if c.entry == "temporal_attention")
    # the geometry the frame counts were chosen for
    g = {F: lc.geometry(dict(frames=F)) for F in lc.FRAME_EDGES}
    assert g[65] == (2, [1, 2]) and g[128] == (2, [1, 2]) and g[129] == (3, [1, 2, 3]) and g[200] == (4, [1, 2, 3, 4]) and g[256] == (4, [1, 2, 3, 4])
    assert lc.geometry(lc.BY_ID["long-q-frames-inside-a-stage"].p) == (1, [2]) and lc.geometry(lc.BY_ID["long-q-frames-last-shard"].p) == (1, [2])


def _host_checks(p):
    """me_tattn's argument checks, restated."""
    assert 0 < p["batch"] <= 8 and p["dh"] % 8 == 0 and 320 % p["dh"] == 0 and (p["heads"] * p["dh"]) % 320 == 0 and lc.STAGE < p["frames"] <= lc.MAX_FRAMES
    qf, q0, kp, qp = p.get("q_frames", 0), p.get("q_frame0", 0), p.get("kv_parts", 1), p.get("q_parts", 1)
    assert q0 + qf <= p["frames"] and (kp <= 1 or p["frames"] % kp == 0) and (qp <= 1 or (qp == kp and not qf))
    assert all(0 <= m < p["batch"] for m in p.get("kv_map") or ())


@pytest.mark.parametrize("case", lc.CASES, ids=lambda c: c.id)
def test_fp32_emulation_agrees_with_the_fp64_reference_inside_the_gpu_bound(case):
    _host_checks(case.p)
    t = lc.build(case)
    assert all(bool(torch.isfinite(v).all()) for v in t.values())
    want = fr.run(case, ref, t, fr.REF)
    figures = fr.compare(case, fr.run(case, fr.Emu(), t, fr.EMU), want, who="fp32 emulation")
    print(case.id, {k: (f"{r:.2e}", f"{m:.2e}") for k, (r, m) in figures.items()})


@pytest.mark.parametrize("case", [c for c in lc.CASES if c.p.get("kind") in ("rising", "falling")], ids=lambda c: c.id)
def test_the_moving_maximum_inputs_move_the_maximum(case):
    """rising: the score trend is + 0.25 per frame against noise of about one unit, so a stage in which a query sees at least 32 keys tops every stage before
    it: the running maximum of such a query changes in every stage.  falling: the first stage holds the maximum of every query."""
    m = lc.stage_maxima(case, lc.build(case))          # [b, p, h, i, stage]
    F = case.p["frames"]
    i = torch.arange(F)
    for st in range(1, m.shape[-1]):
        if case.p["kind"] == "rising":
            rows = (i >= st * lc.STAGE + 31)           # >= 32 keys of stage st below the diagonal
            assert bool((m[..., rows, st] > m[..., rows, :st].max(dim=-1).values).all()), (case.id, st)
        else:
            rows = i >= st * lc.STAGE
            assert bool((m[..., rows, st] < m[..., rows, 0] - 4.0).all()), (case.id, st)
    if case.p["kind"] == "rising" and F >= 96:
        assert bool((i >= lc.STAGE + 31).any())


def test_a_deliberately_stale_maximum_fails_the_rising_case():
    """An online softmax that never rescales what earlier stages accumulated (every stage weighted by its own maximum): the rising inputs tell it apart."""
    case = lc.BY_ID["long-F136-dh40-rising"]
    t = lc.build(case)
    p = case.p
    heads, dh, F, npix, batch = p["heads"], p["dh"], p["frames"], p["npix"], p["batch"]
    C = heads * dh
    shp = lambda x: x.float().reshape(batch, F, npix, heads, dh).permute(0, 2, 3, 1, 4)    # noqa: E731
    q, k, v = shp(t["q"]), shp(t["kv"][:, :C]), shp(t["kv"][:, C:])
    s = (q @ k.transpose(-1, -2)) * dh ** -0.5
    s = s.masked_fill(torch.arange(F)[None, :] > torch.arange(F)[:, None], -1.0e30)
    o, l = torch.zeros_like(q), torch.zeros(q.shape[:-1] + (1,))
    for k0 in range(0, F, lc.STAGE):
        blk = s[..., k0:k0 + lc.STAGE]
        e = (blk - blk.max(dim=-1, keepdim=True).values.clamp_min(-1.0e4)).exp()
        o, l = o + e @ v[..., k0:k0 + lc.STAGE, :], l + e.sum(-1, keepdim=True)
    got = {"y": (o / l).permute(0, 3, 1, 2, 4).reshape(batch * F * npix, C).half()}
    with pytest.raises(AssertionError):
        fr.compare(case, got, fr.run(case, ref, t, fr.REF), who="stale maximum")


def test_more_than_256_frames_are_refused_on_the_host_with_a_message_that_names_the_limit():
    """The call never launches: on a machine without a device the addresses are fabricated, with one they are sentinel-filled buffers that stay untouched."""
    from motioneditor_amd import capi
    L = capi.lib()
    r = lc.REFUSED_FRAMES
    C = r["heads"] * r["dh"]
    nbytes = r["batch"] * r["frames"] * r["npix"] * C * 2
    bufs = [torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(4)] if torch.cuda.is_available() else None
    a = capi.TAttnArgs()
    a.Q, a.K, a.V, a.O = [b.data_ptr() for b in bufs] if bufs else [0x100000 * (i + 1) for i in range(4)]
    a.ldq = a.ldk = a.ldv = a.ldo = C
    a.heads, a.dh, a.batch, a.frames, a.npix, a.scale = r["heads"], r["dh"], r["batch"], r["frames"], r["npix"], r["dh"] ** -0.5
    rc = L.me_tattn(ctypes.byref(a), None)
    msg = L.me_last_error().decode()
    assert rc == capi.ME_EINVAL and msg.startswith("me_tattn:") and "256" in msg, (rc, msg)
    if bufs:
        torch.cuda.synchronize()
        assert all(bool((b == 0xA5).all()) for b in bufs)
    # other head sizes above 48 frames: refused as before
    a.dh, a.heads, a.frames = 32, 10, 72
    assert L.me_tattn(ctypes.byref(a), None) == capi.ME_EINVAL and "frames must be one of" in L.me_last_error().decode()


def test_72_frame_denoise_step_on_the_emulated_abi_matches_the_oracle(monkeypatch, unet_sd_np, cn_sd_np, unet_sd_torch, cn_sd_torch):
    """The host path at 72 frames (nine adapter chunks, a temporal attention over 72 frames in every block): tests/test_step_cpu.py's step at step 4, both
    editors active.  It passes without the key-tiled kernel (the emulation has no frame limit): it guards the layers above me_tattn."""
    import emu_ops
    from conftest import max_rel
    from motioneditor_amd import schedulers
    from motioneditor_amd.attn_control import (FullySelfAttentionControlMask, TemporalSelfAttentionControl, regiter_fully_attention_editor_diffusers,
                                               regiter_temporal_attention_editor_diffusers)
    from motioneditor_amd.models import graph
    from motioneditor_amd.models.controlnet import ControlNetModel
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    import motioneditor_amd.models.unet_2d_condition as u
    import motioneditor_amd.pipelines.pipeline_motion_editor as pm
    from motioneditor_amd.pipelines import MotionEditorPipeline
    from oracle import ref_cpu
    from test_step_cpu import step_inputs
    for m in (graph, u, pm, schedulers):
        monkeypatch.setattr(m, "ops", emu_ops)
    f, step = 72, 4
    x = step_inputs(f=f)
    ddim = ref_cpu.DDIM()
    sp, tp = ref_cpu.SpatialEditor(x["masks"]), ref_cpu.TemporalEditor()
    sp.cur_step = tp.cur_step = step
    t = ddim.timesteps[step]
    images = torch.cat([x["skeleton"]] * 2).reshape(2 * f, 3, 64, 64)
    with torch.no_grad():
        want = ref_cpu.denoise_step(unet_sd_torch, cn_sd_torch, ddim, x["latents"], t, x["uncond"], x["cond"], images, sp, tp, 7.5)
    pipe = MotionEditorPipeline(unet=UNet2DConditionModel(unet_sd_np, device="cpu", dtype=torch.float32), controlnet=ControlNetModel(cn_sd_np, device="cpu", dtype=torch.float32))
    ted = TemporalSelfAttentionControl(start_step=4, start_layer=10)
    regiter_temporal_attention_editor_diffusers(pipe, ted)
    sed = FullySelfAttentionControlMask(start_step=4, start_layer=10, source_masks=x["masks"])
    regiter_fully_attention_editor_diffusers(pipe, sed)
    ted.cur_step = sed.cur_step = step
    pipe.scheduler.set_timesteps(50)
    emb = torch.cat([x["uncond"].expand(2, 77, 768), x["cond"]])
    got = pipe.denoise_step(x["latents"], t, emb, images, 7.5)
    assert got.shape == x["latents"].shape
    e = max_rel(got, want)
    print(f"72 frames x 8 x 8 latents, step 4: max-relative {e:.2e}")
    assert e < 2e-4
