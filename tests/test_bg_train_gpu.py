"""Stage-1 background tuning (train_bg.py) on the MI355X: the derived-weight refresh kernel (me_refresh_weights) against weights.Packed.ln_fold,
util.UNetTuner's gradients against the reference (tests/golden/bg_train.npz), its step against the oracle under autograd + AdamW, train -> infer,
a recorded denoising-step plan replayed after tuning, and examples/train_bg.py end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLD, ROOT

pytestmark = pytest.mark.gpu
T = torch.from_numpy
LR = 1e-3   # a visible step (the reference's 3e-5 moves fp32 weights by 1e-5)


def _golden():
    g = np.load(GOLD / "bg_train.npz")
    F32 = lambda k: T(g[k].astype(np.float32))   # noqa: E731
    return g, dict(noisy=F32("noisy"), noise=F32("noise"), ehs=F32("ehs"), t=int(g["t"]))


def test_refresh_kernel_matches_ln_fold():
    """me_refresh_weights on a plain entry (q rows of a fused q|k|v), a LayerNorm-fold entry (the same rows of the lnw fold) and a bias vector:
    W' rows bitwise what Packed.ln_fold builds from the same fp32 values, colsum / cvec to fp32 round-off, every row outside the table untouched."""
    from motioneditor_amd import ops
    from motioneditor_amd.weights import Packed
    g = torch.Generator().manual_seed(5)
    C, K = 320, 320
    st = {n: torch.randn(C, K, generator=g) * 0.05 for n in ("q", "k", "v")}
    st.update({"n.weight": 1 + 0.1 * torch.randn(K, generator=g), "n.bias": 0.1 * torch.randn(K, generator=g), "o.bias": torch.randn(C, generator=g)})
    P = Packed(st, "cuda")
    fused = P.fused(["q", "k", "v"])
    wq, cs, cv = P.ln_fold("n", ["q", "k", "v"])
    vec = P.vec("o.bias")
    fused0, wq0, cs0, cv0 = fused.clone(), wq.clone(), cs.clone(), cv.clone()
    new_q = torch.randn(C, K, generator=g) * 0.05
    new_b = torch.randn(C, generator=g)
    master = new_q.cuda()
    mb = new_b.cuda()
    gamma, beta = st["n.weight"].cuda(), st["n.bias"].cuda()
    tab = ops.refresh_table([(master, fused[:C, 0, :], None, None, None, None, None),
                             (master, wq[:C, 0, :], gamma, beta, None, cs[:C], cv[:C]),
                             (mb.reshape(1, -1), vec.reshape(1, -1), None, None, None, None, None)])
    ops.refresh_weights(tab)
    torch.cuda.synchronize()
    want = Packed(dict(st, q=new_q), "cuda").ln_fold("n", ["q", "k", "v"])
    assert torch.equal(fused[:C, 0, :], master.half()) and torch.equal(vec, mb.half())
    assert torch.equal(wq[:C], want[0][:C])
    # fp32 round-off of a K-term sum: bounded per row by its sum of magnitudes (the kernel sums in another order than torch)
    mag_cs = want[0][:C, 0, :].float().abs().sum(1)
    mag_cv = (new_q.cuda() * beta).abs().sum(1)
    assert bool(((cs[:C] - want[1][:C]).abs() <= 1e-5 * mag_cs).all()), float((cs[:C] - want[1][:C]).abs().max())
    assert bool(((cv[:C] - want[2][:C]).abs() <= 1e-5 * mag_cv).all()), float((cv[:C] - want[2][:C]).abs().max())
    assert torch.equal(fused[C:], fused0[C:]) and torch.equal(wq[C:], wq0[C:]) and torch.equal(cs[C:], cs0[C:]) and torch.equal(cv[C:], cv0[C:])
    assert not torch.equal(wq[:C], wq0[:C])


def test_tuner_gradients_on_the_gpu_vs_reference_golden(unet_sd_np):
    """UNetTuner.grads on the GPU (tape forward through the whole UNet, backward through the up path, the mid block AND the down path, row-range
    dW of the fused q|k|v) against the reference UNet's autograd (bg_train.npz); the adapter-training test's bounds."""
    from motioneditor_amd import util
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    g, c = _golden()
    tr = util.UNetTuner(UNet2DConditionModel(unet_sd_np, device="cuda"))
    loss, grads = tr.grads(c["noisy"], c["t"], c["ehs"], c["noise"])
    names = [str(n) for n in g["names"]]
    assert sorted(grads) == sorted(names)
    norms = np.array([float(grads[k].norm()) for k in names])
    rel = np.abs(norms / g["grad_norms"] - 1)
    tot = float(np.sqrt((norms ** 2).sum()) / np.sqrt((g["grad_norms"] ** 2).sum()))
    fulls = [float((grads[str(k)] - T(g[f"full_{i}"])).norm() / T(g[f"full_{i}"]).norm()) for i, k in enumerate(g["full_names"])]
    print("stage-1 gradients on GPU: loss", loss, "vs", float(g["loss"]), " total norm ratio", tot, " median / max per-parameter norm error",
          float(np.median(rel)), float(rel.max()), " full tensors rel-L2", fulls)
    assert abs(loss - float(g["loss"])) < 5e-3 * float(g["loss"]) and abs(tot - 1) < 2e-2 and float(np.median(rel)) < 2e-2 and max(fulls) < 5e-2, (loss, tot, fulls)


def test_tuner_step_on_the_gpu_vs_oracle_autograd_adamw(unet_sd_np):
    """UNetTuner.step entirely on the device against ref_cpu + autograd + clip_grad_norm_ + torch.optim.AdamW; the second step's loss equals the
    oracle's loss at the updated parameters; the transposed-weight cache of the backward does not grow over steps; everything outside the bucket
    (frozen k|v rows, the adapter's attn_temp, all other parameters) is bitwise unchanged on the device."""
    from motioneditor_amd import ops, util
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    from oracle import ref_cpu
    _, c = _golden()
    sd = {k: T(v).clone() for k, v in unet_sd_np.items()}
    unet = UNet2DConditionModel(unet_sd_np, device="cuda")
    tr = util.UNetTuner(unet, lr=LR)
    loss = tr.step(c["noisy"], c["t"], c["ehs"], c["noise"])
    cache1 = len(ops._wT_cache)
    names = tr.names
    params = {k: torch.nn.Parameter(sd[k].clone()) for k in names}
    opt = torch.optim.AdamW(list(params.values()), lr=LR, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)
    sd2 = dict(sd)
    sd2.update(params)
    l0 = torch.nn.functional.mse_loss(ref_cpu.unet_forward(sd2, c["noisy"], c["t"], c["ehs"]), c["noise"])
    for k, gr in zip(names, torch.autograd.grad(l0, [params[k] for k in names])):
        params[k].grad = gr
    torch.nn.utils.clip_grad_norm_(list(params.values()), 1.0)
    opt.step()
    got = tr.export_state_dict()
    num = sum(float((got[k] - params[k].detach()).pow(2).sum()) for k in names)
    den = sum(float((params[k].detach() - sd[k]).pow(2).sum()) for k in names)
    upd = (num / den) ** 0.5
    num_s = den_s = 0.0
    for k in names:      # tightly where the oracle's gradient is significant (> 1 % of its tensor's rms): AdamW's first step is ~ lr sign(g)
        gk, dref, dgot = params[k].grad, params[k].detach() - sd[k], got[k] - sd[k]
        sig = gk.abs() > 1e-2 * float(gk.pow(2).mean().sqrt())
        num_s += float(((dgot - dref) * sig).pow(2).sum())
        den_s += float((dref * sig).pow(2).sum())
    upd_s = (num_s / den_s) ** 0.5
    l0 = l0.detach()
    print("stage-1 tuner on GPU: loss", loss, "vs", float(l0), " update rel-L2", upd, " on significant gradients", upd_s)
    # measured on MI355X: loss 1.363333 vs 1.363318, whole update 5.1e-2 (the adapter step's bound is 5e-2: with the whole UNet's backward in front
    # of them, more elements sit at gradient-rounding level, where AdamW's first step ~ lr sign(g) may land 2 lr away), on significant gradients 1.1e-2
    # (the adapter step's bound of 2e-2 kept)
    assert abs(loss - float(l0)) < 5e-3 * float(l0) and upd < 8e-2 and upd_s < 2e-2, (loss, float(l0), upd, upd_s)
    with torch.no_grad():
        sd3 = dict(sd)
        sd3.update({k: v.detach() for k, v in params.items()})
        l1 = float(torch.nn.functional.mse_loss(ref_cpu.unet_forward(sd3, c["noisy"], c["t"], c["ehs"]), c["noise"]))
    loss2 = tr.step(c["noisy"], c["t"], c["ehs"], c["noise"])
    assert abs(loss2 - l1) < 5e-3 * l1 and abs(l1 - float(l0)) > 1e-5, (loss2, l1, float(l0))
    tr.step(c["noisy"], c["t"], c["ehs"], c["noise"])
    assert len(ops._wT_cache) <= cache1, "transposed-weight cache grows with the training steps"
    # frozen: the k|v rows of every fused attn1 projection and every packed tensor of an untrained parameter equal a fresh packing of the state
    from motioneditor_amd.weights import Packed
    ref = Packed(unet_sd_np, "cuda")
    trained = set(names)
    checked = 0
    for key, t in unet.P.cache.items():
        kind, _, joined = key.partition(":")
        if kind not in ("mat", "vec", "fused", "geglu", "gegluv") or not isinstance(t, torch.Tensor):
            continue
        fresh = ref._get(key)
        for r0, r1, n in unet.P.row_ranges(key):
            if n not in trained:
                assert torch.equal(t[r0:r1], fresh[r0:r1]), n
                checked += 1
    assert checked > 100
    for n in tr.unreached:
        assert torch.equal(unet.P.raw(n), T(unet_sd_np[n])), n


def test_train_then_infer_on_the_gpu(unet_sd_np):
    """Two tape-only steps, then the first ordinary forward (LayerNorm folds built now, from the live masters) equals a fresh UNet built from the
    exported state to the round-off of colsum / cvec and differs from the untrained UNet by far more; after a third step (folds refreshed in
    place) the same holds."""
    from motioneditor_amd import util
    from motioneditor_amd.models import graph
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    _, c = _golden()
    unet = UNet2DConditionModel(unet_sd_np, device="cuda")
    tr = util.UNetTuner(unet, lr=LR)
    tr.step(c["noisy"], c["t"], c["ehs"], c["noise"])
    tr.step(c["noisy"], c["t"], c["ehs"], c["noise"])
    assert not any(k.startswith("lnw") for k in unet.P.cache)
    text = graph.text_rows(c["ehs"].cuda())
    fwd = lambda m: graph.unet_forward(m.P, c["noisy"].cuda(), float(c["t"]), text).t.float()   # noqa: E731
    got = fwd(unet)
    assert any(k.startswith("lnw") for k in unet.P.cache)

    def fresh():
        sd = dict(unet_sd_np)
        sd.update({k: v.numpy() for k, v in tr.export_state_dict().items()})
        m = UNet2DConditionModel(sd, device="cuda")
        return fwd(m), m.P
    want, _ = fresh()
    base = fwd(UNet2DConditionModel(unet_sd_np, device="cuda"))
    e = float((got - want).norm() / want.norm())
    d = float((base - want).norm() / want.norm())
    print("train -> infer on GPU: vs fresh UNet", e, " vs untrained", d)
    assert e < 1e-3 and d > 10 * e, (e, d)     # measured: 0 (the folds were just built from the live masters, as the fresh UNet builds them), 1.08
    # a third step refreshes those folds IN PLACE (me_refresh_weights): W' bitwise, colsum / cvec to fp32 round-off of the fresh packing
    tr.step(c["noisy"], c["t"], c["ehs"], c["noise"])
    got3 = fwd(unet)
    want3, P3 = fresh()
    n = 0
    for key, ent in unet.P.cache.items():
        if key.startswith("lnw") and any(x in key for x in tr.names):
            w, cs, cv = ent
            w3, cs3, cv3 = P3.cache[key]
            assert torch.equal(w, w3), key
            assert float((cs - cs3).abs().max()) <= 1e-5 * float(w3.float().abs().sum(dim=(1, 2)).max()), key
            assert float((cv - cv3).abs().max()) <= 1e-5 * max(float(cv3.abs().max()), 1.0), key
            n += 1
    assert n == 16 * 3
    e3 = float((got3 - want3).norm() / want3.norm())
    print("after an in-place refresh: vs fresh UNet", e3)
    # measured 1.4e-3: the colsum / cvec round-off flips fp16 roundings of activations that the tuned (lr 1e-3) network amplifies; the untrained
    # network differs by ~1
    assert e3 < 1e-2, e3


def test_plan_recorded_before_tuning_replays_the_tuned_weights(unet_sd_np, cn_sd_np):
    """A denoise_step_planned plan recorded BEFORE tuning, replayed after two tuner steps, equals the eager step of the tuned pipeline bit for bit
    (the refresh writes into the tensors the plan captured) and differs from the untuned step."""
    from motioneditor_amd import util
    from motioneditor_amd.models.controlnet import ControlNetModel
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    from motioneditor_amd.pipelines import MotionEditorPipeline
    from test_step_cpu import step_inputs
    _, c = _golden()
    x = step_inputs()
    f = x["latents"].shape[2]
    pipe = MotionEditorPipeline(unet=UNet2DConditionModel(unet_sd_np, "cuda"), controlnet=ControlNetModel(cn_sd_np, "cuda"))
    pipe.scheduler.set_timesteps(50)
    t = pipe.scheduler.timesteps[4]
    images = torch.cat([x["skeleton"]] * 2).reshape(2 * f, 3, 64, 64).cuda()
    emb = torch.cat([x["uncond"].expand(2, 77, 768), x["cond"]]).cuda()
    lat = x["latents"].cuda()
    before = pipe.denoise_step_planned(lat, t, emb, images, 7.5).clone()
    assert torch.equal(before, pipe.denoise_step(lat, t, emb, images, 7.5))
    tr = util.UNetTuner(pipe.unet, lr=LR)
    tr.step(c["noisy"], c["t"], c["ehs"], c["noise"])
    tr.step(c["noisy"], c["t"], c["ehs"], c["noise"])
    n_plans = len(pipe._plans)
    replay = pipe.denoise_step_planned(lat, t, emb, images, 7.5).clone()
    assert len(pipe._plans) == n_plans, "the plan was recorded again instead of replayed"
    eager = pipe.denoise_step(lat, t, emb, images, 7.5)
    torch.cuda.synchronize()
    assert torch.equal(replay, eager)
    assert not torch.equal(replay, before)


def test_train_bg_example_runs_and_writes_a_checkpoint(tmp_path):
    """examples/train_bg.py at the size of train-bg.yaml (8 frames x 512^2): finite losses, ms/step printed, checkpoint-3/ readable by the loader."""
    out = tmp_path / "bg"
    r = subprocess.run([sys.executable, str(ROOT / "examples" / "train_bg.py"), "--frames", "8", "--size", "512", "--steps", "3", "--out", str(out)],
                       cwd=str(ROOT), capture_output=True, text=True, timeout=900, env=dict(os.environ))
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0
    losses = [float(ln.split("loss = ")[1].split()[0]) for ln in r.stdout.splitlines() if "loss = " in ln]
    assert len(losses) == 3 and all(np.isfinite(losses)), losses
    from motioneditor_amd import checkpoint
    sd = checkpoint.load_file(out / "checkpoint-3" / "model.safetensors")
    assert "down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_q.weight" in sd and len(sd) > 1000
