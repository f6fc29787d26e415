"""Stage-1 background tuning (train_bg.py) on the emulated ABI: util.UNetTuner -- parameter selection, row-range gradients of fused projections,
clip + AdamW on packed fp32 masters, the in-place refresh of every derived weight -- against the reference (tests/golden/bg_train.npz) and
against the oracle under torch autograd + clip_grad_norm_ + torch.optim.AdamW."""
import numpy as np
import pytest
import torch

import emu_train_ops
from conftest import GOLD

T = torch.from_numpy
LR = 1e-3   # a visible step (the reference's 3e-5 moves fp32 weights by 1e-5)


@pytest.fixture
def emu(monkeypatch):
    import motioneditor_amd.models.unet_2d_condition as u
    from motioneditor_amd import util
    from motioneditor_amd.models import graph
    for m in (graph, u, util):
        monkeypatch.setattr(m, "ops", emu_train_ops)


def _golden():
    g = np.load(GOLD / "bg_train.npz")
    F32 = lambda k: T(g[k].astype(np.float32))   # noqa: E731
    return g, dict(noisy=F32("noisy"), noise=F32("noise"), ehs=F32("ehs"), t=int(g["t"]))


def _unet(sd_np):
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    return UNet2DConditionModel(sd_np, device="cpu", dtype=torch.float32)


def _oracle_step(sd, names, clip, steps=1):
    """ref_cpu under autograd + clip_grad_norm_(1.0) + torch.optim.AdamW: the parameters after `steps` steps and the losses."""
    from oracle import ref_cpu
    params = {k: torch.nn.Parameter(sd[k].clone()) for k in names}
    opt = torch.optim.AdamW(list(params.values()), lr=LR, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)
    losses = []
    for _ in range(steps):
        sd2 = dict(sd)
        sd2.update(params)
        loss = torch.nn.functional.mse_loss(ref_cpu.unet_forward(sd2, clip["noisy"], clip["t"], clip["ehs"]), clip["noise"])
        for k, gr in zip(names, torch.autograd.grad(loss, [params[k] for k in names])):
            params[k].grad = gr
        torch.nn.utils.clip_grad_norm_(list(params.values()), 1.0)
        opt.step()
        losses.append(float(loss))
    return {k: v.detach() for k, v in params.items()}, losses


def test_selection_rule_and_the_tuner_bucket_match_the_reference(emu, unet_sd_np):
    """train_bg.py's module filter over the reference key schema selects exactly the parameters the reference trains -- with a gradient (the
    UNet's) and without one (the adapter's attn_temp, which the plain forward never reaches); the tuner's bucket holds exactly the first list."""
    from motioneditor_amd import util, weights
    g, _ = _golden()
    keys = [ln.split()[0] for ln in (GOLD / "unet_keys.txt").read_text().splitlines() if ln.strip()]
    sel = weights.select_trainable(keys, ("attn1.to_q", "attn2.to_q", "attn_temp"))
    reached, unreached = [str(n) for n in g["names"]], [str(n) for n in g["unreached"]]
    assert sorted(sel) == sorted(reached + unreached) and not set(reached) & set(unreached)
    tr = util.UNetTuner(_unet(unet_sd_np))
    assert tr.names == sorted(reached) and tr.unreached == sorted(unreached)
    assert sorted(tr.param_buffers) == sorted(reached)
    # q of every fused q|k|v is trained on its rows only: k|v own no bucket slot
    assert sum(b.numel() for b in tr.param_buffers.values()) == sum(unet_sd_np[n].size for n in reached)
    assert weights.select_trainable(["a.attn1.to_q.weight", "a.attn1.to_qx.weight", "b.norm1.weight"], (), ("norm1.weight",)) == ["b.norm1.weight"]


def test_unsupported_parameters_are_refused_by_name(emu, unet_sd_np):
    from motioneditor_amd import util
    with pytest.raises(NotImplementedError, match="temp_conv1"):
        util.UNetTuner(_unet(unet_sd_np), trainable_modules=("resnets.0.temp_conv1",))
    with pytest.raises(NotImplementedError, match="time_emb_proj"):
        util.UNetTuner(_unet(unet_sd_np), trainable_modules=("attn1.to_q",), trainable_params=("down_blocks.0.resnets.0.time_emb_proj.weight",))


def test_oracle_stage1_gradients_match_the_reference_unet(unet_sd_np):
    """Pins the oracle for this path: ref_cpu.unet_forward under autograd reproduces the reference UNet's loss and gradients (bg_train.npz)."""
    from oracle import ref_cpu
    g, c = _golden()
    sd = {k: T(v) for k, v in unet_sd_np.items()}
    names = [str(n) for n in g["names"]]
    for k in names:
        sd[k] = sd[k].clone().requires_grad_(True)
    loss = torch.nn.functional.mse_loss(ref_cpu.unet_forward(sd, c["noisy"], c["t"], c["ehs"]), c["noise"])
    assert abs(float(loss) - float(g["loss"])) < 1e-4 * float(g["loss"])
    grads = torch.autograd.grad(loss, [sd[k] for k in names])
    assert np.allclose(np.array([float(x.norm()) for x in grads]), g["grad_norms"], rtol=1e-3, atol=1e-9)
    for i, k in enumerate(str(n) for n in g["full_names"]):
        want = T(g[f"full_{i}"])
        assert float((grads[names.index(k)] - want).norm() / want.norm()) < 1e-3


def test_tuner_gradients_match_the_reference(emu, unet_sd_np):
    from motioneditor_amd import util
    g, c = _golden()
    tr = util.UNetTuner(_unet(unet_sd_np))
    loss, grads = tr.grads(c["noisy"], c["t"], c["ehs"], c["noise"])
    assert abs(loss - float(g["loss"])) < 1e-4 * float(g["loss"])
    names = [str(n) for n in g["names"]]
    norms = np.array([float(grads[k].norm()) for k in names])
    assert np.allclose(norms, g["grad_norms"], rtol=2e-3, atol=1e-9), float(np.abs(norms / g["grad_norms"] - 1).max())
    for i, k in enumerate(str(n) for n in g["full_names"]):
        want = T(g[f"full_{i}"])
        assert float((grads[k] - want).norm() / want.norm()) < 2e-3


def test_tuner_steps_match_autograd_adamw_and_leave_everything_else_bitwise(emu, unet_sd_np):
    """Two tuner steps against two oracle steps (autograd + clip_grad_norm_ + torch.optim.AdamW); every parameter outside the bucket -- the
    frozen k|v rows of the fused attn1 projections, the adapter's attn_temp, everything else -- bitwise unchanged."""
    from motioneditor_amd import util
    g, c = _golden()
    sd = {k: T(v).clone() for k, v in unet_sd_np.items()}    # a copy: the frozen values are compared bitwise after training
    unet = _unet(unet_sd_np)
    tr = util.UNetTuner(unet, lr=LR)
    l1 = tr.step(c["noisy"], c["t"], c["ehs"], c["noise"])
    l2 = tr.step(c["noisy"], c["t"], c["ehs"], c["noise"])
    want, losses = _oracle_step(sd, tr.names, c, steps=2)
    got = tr.export_state_dict()
    assert abs(l1 - losses[0]) < 1e-4 * losses[0] and abs(l2 - losses[1]) < 1e-4 * losses[1], (l1, l2, losses)
    num = sum(float((got[k] - want[k]).pow(2).sum()) for k in tr.names)
    den = sum(float((want[k] - sd[k]).pow(2).sum()) for k in tr.names)
    assert (num / den) ** 0.5 < 1e-2, (num / den) ** 0.5
    # nothing else moved: the live packed tensors of the frozen parameters are their state values
    P = unet.P
    trained = set(tr.names)
    for key, t in P.cache.items():
        kind, _, joined = key.partition(":")
        if kind != "fused" or "attn1.to_k.weight" not in joined:
            continue
        for r0, r1, n in P.row_ranges(key):
            if n not in trained:
                assert torch.equal(t[r0:r1, 0, :], sd[n]), n
    for n in tr.unreached + ["down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_k.weight", "conv_in.weight", "up_blocks.3.attentions.2.proj_out.weight"]:
        assert torch.equal(P.raw(n), sd[n]), n


def test_zero_output_projection_gives_weight_decay_only(emu, unet_sd_np):
    """attn_temp.to_out.0.weight = 0 (what checkpoint.inflate gives a real SD-1.5 UNet): attn_temp.to_q / k / v have an exactly zero gradient and
    still take AdamW's decoupled weight decay, p -> p (1 - lr wd); to_out itself moves."""
    from motioneditor_amd import util
    _, c = _golden()
    sd_np = dict(unet_sd_np)
    blk = "down_blocks.1.attentions.0.transformer_blocks.0.attn_temp"
    sd_np[blk + ".to_out.0.weight"] = np.zeros_like(unet_sd_np[blk + ".to_out.0.weight"])
    tr = util.UNetTuner(_unet(sd_np), lr=LR)
    tr.step(c["noisy"], c["t"], c["ehs"], c["noise"])
    got = tr.export_state_dict()
    for x in ("to_q", "to_k", "to_v"):
        p0 = torch.from_numpy(sd_np[f"{blk}.{x}.weight"])
        decayed = p0 * (1.0 - LR * 1e-2)
        assert float(((got[f"{blk}.{x}.weight"] - decayed).abs() - 3e-7 * p0.abs()).max()) <= 0.0, x   # -lr wd p, to fp32 rounding
        assert not torch.equal(got[f"{blk}.{x}.weight"], p0)
    assert float(got[blk + ".to_out.0.weight"].abs().max()) > 0.5 * LR


def test_train_then_infer_uses_the_tuned_weights(emu, unet_sd_np):
    """Two tape-only steps (no LayerNorm fold entry exists yet), then the first ordinary forward with the fold ON: it must equal a fresh UNet built
    from the exported state (to the round-off of colsum / cvec) and differ from the untrained UNet by far more than that."""
    from motioneditor_amd import util
    from motioneditor_amd.models import graph
    _, c = _golden()
    unet = _unet(unet_sd_np)
    tr = util.UNetTuner(unet, lr=LR)
    tr.step(c["noisy"], c["t"], c["ehs"], c["noise"])
    tr.step(c["noisy"], c["t"], c["ehs"], c["noise"])
    assert not any(k.startswith("lnw") for k in unet.P.cache)
    assert graph._fold()
    text = graph.text_rows(c["ehs"], torch.float32)
    got = graph.unet_forward(unet.P, c["noisy"], float(c["t"]), text).t
    sd = dict(unet_sd_np)
    sd.update({k: v.numpy() for k, v in tr.export_state_dict().items()})
    fresh = graph.unet_forward(_unet(sd).P, c["noisy"], float(c["t"]), text).t
    base = graph.unet_forward(_unet(unet_sd_np).P, c["noisy"], float(c["t"]), text).t
    e = float((got - fresh).norm() / fresh.norm())
    d = float((base - fresh).norm() / fresh.norm())
    assert e < 1e-5 and d > 100 * e, (e, d)
    # a third step refreshes the fold entries built in between, in place
    lnw = {k: v[0] for k, v in unet.P.cache.items() if k.startswith("lnw:") and "attn1.to_q" in k}
    tr.step(c["noisy"], c["t"], c["ehs"], c["noise"])
    got3 = graph.unet_forward(unet.P, c["noisy"], float(c["t"]), text).t
    assert all(unet.P.cache[k][0] is t for k, t in lnw.items())
    sd.update({k: v.numpy() for k, v in tr.export_state_dict().items()})
    fresh3 = graph.unet_forward(_unet(sd).P, c["noisy"], float(c["t"]), text).t
    assert float((got3 - fresh3).norm() / fresh3.norm()) < 1e-5


def test_checkpoint_round_trip(emu, unet_sd_np, tmp_path):
    """save_checkpoint(dir) -> from_pretrained(..., resume_from_checkpoint=dir): the trained tensors come back bitwise in fp32."""
    from safetensors.torch import save_file
    from motioneditor_amd import util
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    _, c = _golden()
    tr = util.UNetTuner(_unet(unet_sd_np), lr=LR)
    tr.step(c["noisy"], c["t"], c["ehs"], c["noise"])
    ck = tmp_path / "checkpoint-1"
    tr.save_checkpoint(ck)
    (tmp_path / "sd" / "unet").mkdir(parents=True)
    save_file({k: torch.from_numpy(v) for k, v in unet_sd_np.items() if not k.startswith("controlnet_adapter.")},
              str(tmp_path / "sd" / "unet" / "diffusion_pytorch_model.safetensors"))
    m = UNet2DConditionModel.from_pretrained(str(tmp_path / "sd"), subfolder="unet", resume_from_checkpoint=str(ck), device="cpu")
    got = tr.export_state_dict()
    for k, v in got.items():
        assert torch.equal(m.P.raw(k), v), k
    assert torch.equal(m.P.raw("conv_in.weight"), torch.from_numpy(unet_sd_np["conv_in.weight"]))
