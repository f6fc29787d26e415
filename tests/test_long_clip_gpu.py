"""Clips longer than 64 frames on a real MI355X.  Kernel level: every case of tests/long_clip_cases.py on me_tattn against the fp64 reference of
tests/ref64_fwd.py inside the entry point's own bound, the launch on tattn_long_kernel<dh> (me_last_kernel), the output in a guard-banded view, two launches
bitwise equal; one case per row order under the whole guard-band protocol of tests/guard.py (inputs and output as views inside poisoned allocations); the
refusal above 256 frames with its buffers untouched.  Model level: one two-branch denoising step at 72 and at 136 frames against the CPU oracle, the planned
executor at 72 frames against the eager step, and inversion + edit at 72 frames through util.ddim_inversion and MotionEditorPipeline.__call__.  Without the
key-tiled kernel every test here ends in me_tattn's refusal of more than 64 frames."""
import ctypes

import pytest
import torch

import fwd_run as fr
import guard
import long_clip_cases as lc
import ref64_fwd as ref
from conftest import rel_l2
from test_fwd_sweep_gpu import launch, ops                      # noqa: F401  (the fixture, and the guarded launch that checks me_last_kernel)
from test_model_gpu import STEP_TOL, controlnet, editors, record, unet    # noqa: F401

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("case", lc.CASES, ids=lambda c: c.id)
def test_long_kernel_matches_the_fp64_reference(ops, case):
    t = lc.build(case)
    want = fr.run(case, ref, t, fr.REF)
    got = launch(ops, case, t)
    figures = fr.compare(case, got, want, who="HIP")
    print(case.id, case.path, {k: (f"{r:.2e}", f"{m:.2e}") for k, (r, m) in figures.items()})
    again = launch(ops, case, t)
    assert fr.bitwise_equal(got["y"], again["y"]), f"{case.id}: two identical calls differ"


@pytest.mark.parametrize("cid", lc.GUARDED)
def test_long_kernel_stays_inside_its_views(ops, cid):
    """The protocol of tests/guard.py as test_guard_temporal_attention applies it: three launches on the same addresses with NaN, 0 and 6e4 around every
    input view, bitwise equal and finite; the sentinel around the output view intact; the inputs unmodified."""
    case = lc.BY_ID[cid]
    p, t = case.p, lc.build(case)
    C = p["heads"] * p["dh"]
    kw = dict(heads=p["heads"], dh=p["dh"], batch=p["batch"], frames=p["frames"], npix=p["npix"], kv_map=p.get("kv_map"), q_frames=p.get("q_frames", 0),
              q_frame0=p.get("q_frame0", 0), kv_parts=p.get("kv_parts", 1), q_parts=p.get("q_parts", 1))
    ins = {"q": guard.embed_in(t["q"], device="cuda"), "k": guard.embed_in(t["kv"][:, :C].contiguous(), device="cuda"), "v": guard.embed_in(t["kv"][:, C:].contiguous(), device="cuda")}
    out, _ = guard.sentinel_out((t["q"].shape[0], C))
    got = guard.run_guarded(lambda: ops.temporal_attention(ins["q"], ins["k"], ins["v"], out=out, **kw), ins, {"out": out})
    assert fr.kernel_matches(ops._last_kernel(), case.path), ops._last_kernel()
    fr.compare(case, {"y": got["out"].cpu()}, fr.run(case, ref, t, fr.REF), who="HIP under guard")


def test_more_than_256_frames_are_refused_and_the_buffers_stay_untouched(ops):
    from motioneditor_amd import capi
    L = capi.lib()
    r = lc.REFUSED_FRAMES
    C = r["heads"] * r["dh"]
    bufs = [torch.full((r["batch"] * r["frames"] * r["npix"] * C * 2 + 64,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(4)]
    a = capi.TAttnArgs()
    a.Q, a.K, a.V, a.O = [b.data_ptr() for b in bufs]
    a.ldq = a.ldk = a.ldv = a.ldo = C
    a.heads, a.dh, a.batch, a.frames, a.npix, a.scale = r["heads"], r["dh"], r["batch"], r["frames"], r["npix"], r["dh"] ** -0.5
    rc = L.me_tattn(ctypes.byref(a), None)
    msg = L.me_last_error().decode()
    torch.cuda.synchronize()
    assert rc == capi.ME_EINVAL and msg.startswith("me_tattn:") and "256" in msg, (rc, msg)
    assert all(bool((b == 0xA5).all()) for b in bufs)
    q = torch.zeros((r["batch"] * r["frames"] * r["npix"], C), dtype=torch.float16, device="cuda")
    with pytest.raises(ValueError, match="256"):
        ops.temporal_attention(q, q, q, **r)


# ------------------------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("f", [72, 136])
def test_denoise_step_at_72_and_136_frames_vs_cpu_oracle(unet, controlnet, unet_sd_torch, cn_sd_torch, f):
    """One full two-branch step at step 4 (ControlNet, adapter, both editors active) on 8 x 8 latents, as
    test_denoise_step_baseline_config0_and_48_frames_vs_cpu_oracle: 72 frames = two key stages and two query blocks, 136 = three and three."""
    from motioneditor_amd.pipelines import MotionEditorPipeline
    from oracle import ref_cpu
    from test_step_cpu import step_inputs
    x = step_inputs(f=f)
    step = 4
    ddim = ref_cpu.DDIM()
    sp, tp = ref_cpu.SpatialEditor(x["masks"]), ref_cpu.TemporalEditor()
    sp.cur_step = tp.cur_step = step
    t = ddim.timesteps[step]
    images = torch.cat([x["skeleton"]] * 2).reshape(2 * f, 3, 64, 64)
    with torch.no_grad():
        want = ref_cpu.denoise_step(unet_sd_torch, cn_sd_torch, ddim, x["latents"], t, x["uncond"], x["cond"], images, sp, tp, 7.5)
    pipe = MotionEditorPipeline(unet=unet, controlnet=controlnet)
    sed, ted = editors(unet, x["masks"])
    sed.cur_step = ted.cur_step = step
    pipe.scheduler.set_timesteps(50)
    emb = torch.cat([x["uncond"].expand(2, 77, 768), x["cond"]]).cuda()
    try:
        got = pipe.denoise_step(x["latents"].cuda(), t, emb, images.cuda(), 7.5)
    finally:
        unet.spatial_editor = unet.temporal_editor = None
    e = rel_l2(got, want)
    record(f"step4_f{f}_8x8_latents", e)
    print(f"{f} frames: rel-L2 {e:.3e} (<= {STEP_TOL})")
    assert e <= STEP_TOL, e


def test_planned_step_at_72_frames_equals_eager(unet, controlnet):
    """denoise_step_planned at 72 frames: three replays of the one plan of steps 4, 5, 6 (both editors active) with new latents, embeddings and
    timesteps each, bitwise the eager loop."""
    from motioneditor_amd.pipelines import MotionEditorPipeline
    from test_step_cpu import step_inputs
    x = step_inputs(f=72)
    f = 72
    images = torch.cat([x["skeleton"]] * 2).reshape(2 * f, 3, 64, 64).cuda()
    g = torch.Generator().manual_seed(5)
    uncs = [x["uncond"] + 0.05 * i * torch.randn(x["uncond"].shape, generator=g) for i in range(3)]
    pipe = MotionEditorPipeline(unet=unet, controlnet=controlnet)
    pipe.scheduler.set_timesteps(50)
    outs = {}
    try:
        for mode in ("eager", "plan"):
            sed, ted = editors(unet, x["masks"])
            sed.cur_step = ted.cur_step = 4
            lat = x["latents"].cuda()
            per_step = []
            for i in range(3):
                emb = torch.cat([uncs[i].expand(2, 77, 768), x["cond"]]).cuda()
                fn = pipe.denoise_step if mode == "eager" else pipe.denoise_step_planned
                lat = fn(lat, pipe.scheduler.timesteps[4 + i], emb, images, 7.5)
                per_step.append(lat.clone())
            outs[mode] = per_step
    finally:
        unet.spatial_editor = unet.temporal_editor = None
    (st,) = pipe._plans.values()
    assert st["plan"].stats()["replays"] >= 3
    for i, (a, b) in enumerate(zip(outs["eager"], outs["plan"])):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), (i, rel_l2(b, a))


def test_inversion_and_edit_at_72_frames(unet, controlnet):
    """util.ddim_inversion (two steps, normal_infer) and MotionEditorPipeline.__call__ on [source, target] (two steps, both editors registered, latents in and
    out) at 72 frames of 64 x 64 pixels: finite, and of the shapes the 8-frame call gives with the frame axis at 72."""
    from motioneditor_amd import util
    from motioneditor_amd.pipelines import MotionEditorPipeline
    from motioneditor_amd.schedulers import DDIMScheduler
    from test_step_cpu import step_inputs
    shapes = {}
    try:
        for f in (8, 72):
            x = step_inputs(f=f)
            pipe = MotionEditorPipeline(unet=unet, controlnet=controlnet)
            s = DDIMScheduler()
            s.set_timesteps(2)
            inv = util.ddim_inversion(pipe, s, x["latents"][:1].cuda(), 2, normal_infer=True, text_embeddings=x["uncond"].cuda())
            editors(unet, x["masks"])
            out = pipe(["a source prompt", "a target prompt"], video_length=f, height=64, width=64, num_inference_steps=2, guidance_scale=7.5,
                       latents=inv[-1].repeat(2, 1, 1, 1, 1), output_type="latent", text_embeddings=x["cond"].cuda(), negative_text_embeddings=x["uncond"].cuda(),
                       skeleton=x["skeleton"].cuda()).images
            unet.spatial_editor = unet.temporal_editor = None
            assert all(bool(torch.isfinite(v).all()) for v in inv) and bool(torch.isfinite(out).all()), f
            shapes[f] = ([tuple(v.shape) for v in inv], tuple(out.shape))
    finally:
        unet.spatial_editor = unet.temporal_editor = None
    at72 = lambda shp: shp[:2] + (72,) + shp[3:]    # noqa: E731
    assert shapes[72] == ([at72(v) for v in shapes[8][0]], at72(shapes[8][1])), shapes
    assert shapes[72][1] == (2, 4, 72, 8, 8)
