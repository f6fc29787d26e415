"""Training on clips longer than 64 frames on a real MI355X.  Kernel level: every case of tests/long_bwd_cases.py through ops.temporal_attention_bwd against
the fp64 reference of tests/ref64_bwd.py inside the case's bound (the entry point's own, or four times the emulation's floor where the case entry says so),
the launch on the key-tiled kernels (me_last_kernel), two launches bitwise equal, the dQ rows of queries whose dout rounds to zero exactly 0.0; the seam at
64 | 65 frames; refused calls with sentinel-filled buffers.  Model level at 72 frames on 8 x 8 latents (two key stages, two query blocks):
util.adapter_training_grads and the first gradient of util.null_optimization against the oracle under torch autograd, one UNetTuner step.  Without
me_tattn_bwd_long the kernel tests fail on the missing symbol and the model tests on me_tattn_bwd's "frames <= 64"."""
import ctypes

import pytest
import torch

import bwd_run as br
import long_bwd_cases as lb
import ref64_bwd as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the HIP library is the only compute path")
    from motioneditor_amd import capi, ops as _ops
    capi.lib()  # fails loudly when libmotioned.so is missing
    return _ops


def cu(t):
    return t.cuda()


# ------------------------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("case", lb.CASES, ids=lambda c: c.id)
def test_long_backward_matches_the_fp64_reference(ops, case):
    t = lb.build(case)
    want = br.run(case, ref, t, br.to_ref)
    seen = {}
    got = br.run(case, ops, t, cu, hook=lambda stage: seen.__setitem__(stage, ops._last_kernel()))
    assert br.kernel_matches(seen["bwd"], case.path), f"{case.id}: written for {case.path}, the launch took {seen['bwd']}"
    print(case.id, seen["bwd"], "bound", br.bound_of(case, "dq"), {n: tuple(f"{x:.2e}" for x in br.errors(got[n], want[n])) for n in sorted(want)})
    br.compare(case, got, want, who="HIP")
    again = br.run(case, ops, t, cu)
    for name in got:
        assert br.bitwise_equal(got[name], again[name]), f"{case.id}: {name} differs between two identical calls"
    if case.p.get("zero_block"):
        z = lb.zeroed_rows(case.p)
        assert float(got["dq"][z].abs().max()) == 0.0, f"{case.id}: dQ of queries whose dout rounds to zero reaches {float(got['dq'][z].abs().max()):.3e}"
        assert float(got["dq"].abs().max()) > 0.0


def test_the_seam_64_frames_stay_on_the_first_kernel_and_65_take_the_key_tiled_ones(ops):
    for frames, want in ((64, "tattn_bwd_kernel"), (65, lb.target(dict(frames=65, dh=40, heads=8)))):
        g = torch.Generator().manual_seed(frames)
        rows, C = frames * 2, 320
        qkv = (torch.randn(rows, 3 * C, generator=g) * 0.7).half().cuda()
        dout = torch.randn(rows, C, generator=g).cuda()
        got = ops.temporal_attention_bwd(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], None, dout, heads=8, dh=40, batch=1, frames=frames, npix=2)
        assert ops._last_kernel() == want == lb.target(dict(frames=frames, dh=40, heads=8)), (frames, ops._last_kernel())
        wq = ref.temporal_attention_bwd(qkv[:, :C].cpu(), qkv[:, C:2 * C].cpu(), qkv[:, 2 * C:].cpu(), None, dout.cpu().double(), heads=8, dh=40, batch=1, frames=frames, npix=2)
        for a, b in zip(got, wq):
            r, m = br.errors(a, b)
            assert r <= 2e-3 and m <= 2e-2, (frames, r, m)


def test_refused_calls_leave_sentinel_filled_buffers_untouched(ops):
    from motioneditor_amd import capi
    L = capi.lib()
    heads, dh, npix, batch = 8, 40, 2, 1
    C = heads * dh
    rows = batch * 257 * npix
    bufs = [torch.full((rows * C * 4 + 64,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(8)]     # dq dk dv q k v dout work
    ptr = [b.data_ptr() for b in bufs]

    def call(frames=72, dh_=dh, work=ptr[7], wb=None, lddq=C, q=ptr[3]):
        wb = lb.work_bytes(batch, frames, npix, heads) if wb is None else wb
        rc = L.me_tattn_bwd_long(ptr[0], lddq, ptr[1], C, ptr[2], C, q, C, ptr[4], C, ptr[5], C, ptr[6], C, batch, frames, npix, heads, dh_, dh ** -0.5, work, wb, None)
        return rc, L.me_last_error().decode()
    for kw, word in ((dict(frames=64), "> 64"), (dict(frames=257), "256"), (dict(dh_=48), "40, 80 or 160"), (dict(work=None), "work"), (dict(wb=8), "work"),
                     (dict(lddq=C - 4), "cover"), (dict(lddq=C + 2), "multiples"), (dict(q=ptr[3] + 8), "misaligned")):
        rc, msg = call(**kw)
        assert rc == capi.ME_EINVAL and msg.startswith("me_tattn_bwd_long:") and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert all(bool((b == 0xA5).all()) for b in bufs)
    q = torch.zeros((rows, C), dtype=torch.float16, device="cuda")
    with pytest.raises(ValueError, match="256"):
        ops.temporal_attention_bwd(q, q, q, None, q.float(), heads=heads, dh=dh, batch=batch, frames=257, npix=npix)
    assert ctypes.sizeof(ctypes.c_void_p) == 8


# ------------------------------------------------------------------------------------------------------------------ the model: 72 frames on 8 x 8 latents
@pytest.fixture(scope="module")
def golden():
    """oracle.ref_cpu under torch autograd on the inputs these tests rebuild (tools/make_golden_long_bwd.py: tens of CPU seconds at 72 frames, hence a fixture)."""
    import numpy as np
    from conftest import GOLD
    g = np.load(GOLD / lb.GOLDEN)
    assert int(g["frames"]) == lb.MODEL_FRAMES == 72
    return g


def test_adapter_training_gradients_at_72_frames_vs_oracle_autograd(unet_sd_np, golden):
    """util.adapter_training_grads at 72 frames (nine adapter chunks; every temporal attention of the tape differentiated by the key-tiled kernels) against
    ref_cpu.unet_forward under torch autograd on the same clip; the criteria and figures of test_adapter_training_gradients_on_the_gpu_vs_reference_golden."""
    import numpy as np
    from motioneditor_amd import util
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    c = br.training_clip(0, f=lb.MODEL_FRAMES, h=8)
    unet = UNet2DConditionModel(unet_sd_np, device="cuda")
    loss, grads = util.adapter_training_grads(unet, c["noisy"], c["t"], c["ehs"], c["down"], c["mid"], c["noise"])
    g = golden
    names = [str(n) for n in g["adapter_names"]]
    assert set(names) == set(grads)
    norms = np.array([float(grads[k].norm()) for k in names])
    live = g["adapter_grad_norms"] > 0           # 1x1-pixel attn_pose q / k projections get exactly zero gradient (one key: softmax = 1)
    assert float(norms[~live].max(initial=0.0)) < 1e-6
    rel = np.abs(norms[live] / g["adapter_grad_norms"][live] - 1)
    tot = float(np.sqrt((norms ** 2).sum()) / np.sqrt((g["adapter_grad_norms"] ** 2).sum()))
    fulls = []
    for i, k in enumerate(str(n) for n in g["adapter_full_names"]):
        want = torch.from_numpy(g[f"adapter_full_{i}"])
        fulls.append(float((grads[k].float().cpu() - want).norm() / want.norm().clamp_min(1e-30)))
    l0 = float(g["adapter_loss"])
    print("adapter training at 72 frames: loss", loss, "vs", l0, " total grad norm ratio", tot, " median / max per-parameter norm error", float(np.median(rel)), float(rel.max()),
          " full tensors rel-L2", fulls)
    assert abs(loss - l0) < 5e-3 * l0 and abs(tot - 1) < 2e-2 and float(np.median(rel)) < 2e-2 and max(fulls) < 5e-2, (loss, l0, tot, fulls)


def test_null_text_first_gradient_at_72_frames_vs_oracle_autograd(unet_sd_np, golden):
    """util.null_optimization, one DDIM step and one inner step at 72 frames: its first gradient (the grads= hook) against the oracle's autograd; the bound of
    the 8-frame test, rel-L2 < 3e-2."""
    from motioneditor_amd import util
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    from motioneditor_amd.schedulers import DDIMScheduler
    latents, context = lb.null_text_inputs()
    sched = DDIMScheduler()
    sched.set_timesteps(50)

    class Pipe:
        pass
    pipe = Pipe()
    pipe.unet = UNet2DConditionModel(unet_sd_np, device="cuda")
    grads = []
    out = util.null_optimization(pipe, sched, latents, context, 1, 1e-5, num_ddim_steps=1, grads=grads)
    want = torch.from_numpy(golden["null_grad0"])
    rel = float((grads[0].float().cpu() - want).norm() / want.norm())
    print("null-text at 72 frames: first gradient rel-L2", rel)
    assert len(out) == 1 and bool(torch.isfinite(out[0]).all()) and rel < 3e-2, rel


def test_one_unet_tuner_step_at_72_frames_is_finite_and_not_skipped(unet_sd_np):
    from motioneditor_amd import util
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    c = br.training_clip(1, f=lb.MODEL_FRAMES, h=8)
    tr = util.UNetTuner(UNet2DConditionModel(unet_sd_np, device="cuda"), lr=1e-3)
    before = tr.master.clone()
    loss = tr.step(c["noisy"], c["t"], c["ehs"], c["noise"])
    assert loss == loss and abs(loss) < 1e4 and tr.steps == 1 and tr.skipped_steps == 0
    assert bool(torch.isfinite(tr.master).all()) and not torch.equal(before, tr.master)
