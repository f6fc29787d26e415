"""Stage-1 tuning widened to the 3x3 convolutions and the GroupNorm affine parameters on the MI355X: me_conv_dw against the fp64 reference of
tests/ref64_bwd.py, me_groupnorm_bwd_params against fp64 autograd, me_refresh_ups4 bitwise against weights.Packed.fold_ups, util.UNetTuner at the widened
selection against the oracle under autograd + AdamW (the bounds of tests/test_bg_train_gpu.py), train -> infer, and a denoising-step plan recorded before a
tuner that trains the upsampler convolutions."""
import pytest
import torch

import tune_fixture as tf
from bwd_cases import BOUNDS
from guard import errs

pytestmark = pytest.mark.gpu
ALPHA = 0.5


def _conv_dw(n_img, Hin, Win, N, K, stride, ups, f16, seed=0, pad=8):
    """me_conv_dw through ops.gemm_dw on views with lddy > N and ldx > K, dst pre-filled.  -> (dst after, dst before, fp64 dW, M, (launch again) -> dst)."""
    from motioneditor_amd import ops
    x, dy, dst0, conv, M = tf.conv_dw_inputs(n_img, Hin, Win, N, K, stride, ups, seed)
    xw = torch.full((x.shape[0], K + pad), float("nan"), dtype=torch.float16, device="cuda")
    dw = torch.full((M, N + pad), float("nan"), dtype=torch.float16 if f16 else torch.float32, device="cuda")
    xw[:, :K], dw[:, :N] = x.cuda(), dy.cuda().to(dw.dtype)

    def launch():
        dst = dst0.cuda().clone()
        ops.gemm_dw(dw[:, :N], xw[:, :K], dst=dst, taps=9, K=K, M=M, alpha=ALPHA, conv=conv)
        torch.cuda.synchronize()
        return dst.cpu()
    return launch(), dst0, tf.conv_dw_ref64(x, dy, conv, M, ALPHA), M, launch


def _held(got, dst0, want, name):
    r, m = errs(got.double() - dst0.double(), want)
    print(f"me_conv_dw {name}: rel-L2 {r:.3e}, max/mean {m:.3e}")
    assert r <= BOUNDS["gemm_dw"][0] and m <= BOUNDS["gemm_dw"][1], (name, r, m)


@pytest.mark.parametrize("f16", [False, True], ids=["dy-f32", "dy-f16"])
@pytest.mark.parametrize("name,n_img,Hin,Win,N,K,stride,ups", [
    ("2x5x7-no-whole-tile", 2, 5, 7, 40, 72, 1, 0),
    ("stride2-7x9-to-4x5", 2, 7, 9, 40, 72, 2, 0),
    ("ups-3x5-to-6x10", 2, 3, 5, 40, 72, 1, 1),
])
def test_conv_dw_matches_the_fp64_reference(name, n_img, Hin, Win, N, K, stride, ups, f16):
    from motioneditor_amd import ops
    got, dst0, want, _, _ = _conv_dw(n_img, Hin, Win, N, K, stride, ups, f16)
    assert ops._last_kernel() == ("conv_dw_kernel<f16>" if f16 else "conv_dw_kernel<f32>")
    _held(got, dst0, want, name)


def test_conv_dw_at_one_pixel_changes_the_centre_tap_only():
    got, dst0, want, _, _ = _conv_dw(3, 1, 1, 40, 72, 1, 0, False, seed=1)
    _held(got, dst0, want, "3x1x1")
    others = [t for t in range(9) if t != 4]
    assert torch.equal(got[:, others], dst0[:, others]), "a padding tap changed dst"
    assert not torch.equal(got[:, 4], dst0[:, 4])


def test_conv_dw_320_with_row_splits_is_bitwise_reproducible():
    """N = K = 320 on 2 x 16 x 16: 5 x 5 block tiles, and (as the library's own geometry reports) more than one row split, folded in index order."""
    from motioneditor_amd import capi
    got, dst0, want, M, again = _conv_dw(2, 16, 16, 320, 320, 1, 0, False, seed=2)
    splits = capi.lib().me_conv_dw_splits(M, 320, 320)
    print("row splits:", splits)
    assert splits >= 2
    _held(got, dst0, want, "2x16x16-320")
    assert torch.equal(got, again()), "two identical calls differ"


@pytest.mark.parametrize("silu", [False, True], ids=["plain", "silu"])
@pytest.mark.parametrize("C,groups,rpg,nsg", tf.GN_CASES)
def test_groupnorm_bwd_params_matches_fp64_autograd(C, groups, rpg, nsg, silu):
    """Through ops.groupnorm_bwd(dgamma=, dbeta=), accumulating into non-zero buffers; tests/test_tune_conv_cpu.py shows the fp32 emulation inside the same
    bounds on the same inputs."""
    from motioneditor_amd import ops
    x, gamma, beta, dy, g0, b0 = tf.gn_inputs(C, rpg, nsg)
    dg, db = g0.cuda().clone(), b0.cuda().clone()
    dx = ops.groupnorm_bwd(x.cuda(), gamma.cuda(), beta.cuda(), dy.cuda(), rows_per_group=rpg, eps=1e-5, silu=silu, groups=groups, dgamma=dg, dbeta=db)
    dx0 = ops.groupnorm_bwd(x.cuda(), gamma.cuda(), beta.cuda(), dy.cuda(), rows_per_group=rpg, eps=1e-5, silu=silu, groups=groups)
    only = torch.zeros(C, device="cuda")
    ops.groupnorm_bwd(x.cuda(), gamma.cuda(), beta.cuda(), dy.cuda(), rows_per_group=rpg, eps=1e-5, silu=silu, groups=groups, dgamma=only)     # dbeta = NULL
    torch.cuda.synchronize()
    assert torch.equal(dx, dx0)
    wg, wb = tf.gn_params_ref64(x, gamma, beta, dy, rpg, groups, silu)
    for nm, got, start, want in (("dgamma", dg, g0, wg), ("dbeta", db, b0, wb), ("dgamma", only, torch.zeros(C), wg)):
        r, m = errs(got.cpu().double() - start.double(), want)
        print(f"me_groupnorm_bwd_params {nm} C={C} rpg={rpg} silu={silu}: rel-L2 {r:.3e}, max/mean {m:.3e}")
        b = BOUNDS["layernorm_bwd_params." + nm]
        # (the accumulation into a start value of magnitude 1 costs one fp32 rounding of it: 6e-8, far below either bound times the gradient's magnitude)
        assert r <= b[0] and m <= b[1], (nm, r, m)


def test_refresh_ups4_is_bitwise_fold_ups():
    from motioneditor_amd import ops
    from motioneditor_amd.weights import Packed
    w = torch.randn(136, 72, 3, 3, generator=torch.Generator().manual_seed(11)) * 0.1
    master = Packed._as_taps(w).contiguous().cuda()
    dst = torch.zeros(136, 16, 72, dtype=torch.float16, device="cuda")
    plain = torch.zeros(136, 9 * 72, dtype=torch.float16, device="cuda")
    ops.refresh_weights(ops.refresh_table([(master, dst, None, None, None, None, None), (master.reshape(136, -1), plain, None, None, None, None, None)]))
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), Packed.fold_ups(w).half()) and torch.equal(plain.cpu(), master.reshape(136, -1).half().cpu())
    assert ops._last_kernel() == "refresh_ups4_kernel"


# ------------------------------------------------------------------ the tuner
def _kinds(names):
    kinds = {"conv3x3": (".conv1.weight", ".conv2.weight", "samplers.0.conv.weight"), "conv1x1": ("conv_shortcut.weight", "proj_in.weight", "proj_out.weight"),
             "groupnorm": ("norm1.weight", "norm2.weight", "norm1.bias", "norm2.bias", ".norm.weight", ".norm.bias"), "dense": ("to_q.weight", "to_k.weight", "to_v.weight", "to_out.0.weight")}
    return {k: [n for n in names if n.endswith(suf)] for k, suf in kinds.items()}


def test_widened_tuner_gradients_and_step_on_the_gpu_vs_oracle(unet_sd_np):
    """UNetTuner.grads and one step at the CPU test's selection and size; bounds of tests/test_bg_train_gpu.py: loss 5e-3, total norm 2e-2, median
    per-parameter norm error 2e-2, update on significant gradients 2e-2, whole update 8e-2.  The figures are printed per parameter kind."""
    import numpy as np
    from motioneditor_amd import util
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    o, c = tf.oracle(), tf.golden()
    names, sd = o["names"], o["sd"]
    tr = util.UNetTuner(UNet2DConditionModel(unet_sd_np, device="cuda"), trainable_modules=tf.MODULES, lr=tf.LR)
    assert tr.names == names
    loss, grads = tr.grads(c["noisy"], c["t"], c["ehs"], c["noise"])
    ref = np.array([float(o["grads"][k].norm()) for k in names])
    norms = np.array([float(grads[k].norm()) for k in names])
    rel = np.abs(norms / ref - 1)
    tot = float(np.sqrt((norms ** 2).sum()) / np.sqrt((ref ** 2).sum()))
    l2 = {k: float((grads[k] - o["grads"][k]).norm() / o["grads"][k].norm()) for k in names}
    print("widened stage-1 gradients on GPU: loss", loss, "vs", o["losses"][0], " total norm ratio", tot, " median / max per-parameter norm error", float(np.median(rel)),
          float(rel.max()), " median / max per-parameter rel-L2", float(np.median(list(l2.values()))), max(l2.values()))
    for kind, ks in _kinds(names).items():
        idx = [names.index(k) for k in ks]
        print(f"  {kind}: {len(ks)} tensors, median norm error {float(np.median(rel[idx])):.3e}, median rel-L2 {float(np.median([l2[k] for k in ks])):.3e}, max rel-L2 {max(l2[k] for k in ks):.3e}")
    assert abs(loss - o["losses"][0]) < 5e-3 * o["losses"][0] and abs(tot - 1) < 2e-2 and float(np.median(rel)) < 2e-2, (loss, tot, float(np.median(rel)))
    for kind, ks in _kinds(names).items():           # no parameter kind hides behind the others' median
        assert float(np.median(rel[[names.index(k) for k in ks]])) < 2e-2, kind
    l1 = tr.step(c["noisy"], c["t"], c["ehs"], c["noise"])
    got, want = tr.export_state_dict(), o["after"][0]
    num = sum(float((got[k] - want[k]).pow(2).sum()) for k in names)
    den = sum(float((want[k] - sd[k]).pow(2).sum()) for k in names)
    num_s = den_s = 0.0
    for k in names:      # tightly where the oracle's gradient is significant (> 1 % of its tensor's rms): AdamW's first step is ~ lr sign(g)
        gk, dref, dgot = o["grads"][k], want[k] - sd[k], got[k] - sd[k]
        sig = gk.abs() > 1e-2 * float(gk.pow(2).mean().sqrt())
        num_s += float(((dgot - dref) * sig).pow(2).sum())
        den_s += float((dref * sig).pow(2).sum())
    upd, upd_s = (num / den) ** 0.5, (num_s / den_s) ** 0.5
    print("widened stage-1 step on GPU: loss", l1, " update rel-L2", upd, " on significant gradients", upd_s)
    assert abs(l1 - o["losses"][0]) < 5e-3 * o["losses"][0] and upd < 8e-2 and upd_s < 2e-2, (l1, upd, upd_s)
    l2_ = tr.step(c["noisy"], c["t"], c["ehs"], c["noise"])
    print("second step's loss", l2_, "vs the oracle's", o["losses"][1])
    assert abs(l2_ - o["losses"][1]) < 5e-3 * o["losses"][1], (l2_, o["losses"][1])


def test_widened_train_then_infer_on_the_gpu(unet_sd_np, monkeypatch):
    """(1) Two tape-only steps, then the first ordinary forward: every derived tensor is built now, from the live masters -- the trained upsampler convolutions
    keep the 9-tap form (Packed.mat_ups builds no fold behind a trainer), so the fresh UNet it is compared with runs with ME_UPS_FOLD=0; bound 1e-3.
    (2) A forward BEFORE the tuner exists leaves folded upsampler weights and LayerNorm folds in the cache; two steps rewrite them in place (me_refresh_ups4,
    me_refresh_weights) and the forward then equals a fresh UNet (folds on) within the in-place bound of test_train_then_infer_on_the_gpu, 1e-2; the folded
    tensors are the same objects, bitwise the fresh packing."""
    from motioneditor_amd import util
    from motioneditor_amd.models import graph
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    c = tf.golden()
    text = graph.text_rows(c["ehs"].cuda())
    fwd = lambda m: graph.unet_forward(m.P, c["noisy"].cuda(), float(c["t"]), text).t.float()   # noqa: E731

    def fresh(tr):
        sd = dict(unet_sd_np)
        sd.update({k: v.numpy() for k, v in tr.export_state_dict().items()})
        m = UNet2DConditionModel(sd, device="cuda")
        return fwd(m), m.P

    base = fwd(UNet2DConditionModel(unet_sd_np, device="cuda"))
    unet = UNet2DConditionModel(unet_sd_np, device="cuda")
    tr = util.UNetTuner(unet, trainable_modules=tf.MODULES, lr=tf.LR)
    for _ in range(2):
        tr.step(c["noisy"], c["t"], c["ehs"], c["noise"])
    monkeypatch.setenv("ME_UPS_FOLD", "0")
    got = fwd(unet)
    assert not any(k.startswith("ups4:") for k in unet.P.cache)
    want, _ = fresh(tr)
    monkeypatch.delenv("ME_UPS_FOLD")
    e, d = float((got - want).norm() / want.norm()), float((base - want).norm() / want.norm())
    print("widened train -> infer on GPU: vs fresh UNet", e, " vs untrained", d)
    assert e < 1e-3 and d > 10 * e, (e, d)

    unet = UNet2DConditionModel(unet_sd_np, device="cuda")
    assert torch.equal(fwd(unet), base)
    ups = {k: t for k, t in unet.P.cache.items() if k.startswith("ups4:")}
    assert len(ups) == 3
    tr = util.UNetTuner(unet, trainable_modules=tf.MODULES, lr=tf.LR)
    for _ in range(2):
        tr.step(c["noisy"], c["t"], c["ehs"], c["noise"])
    got = fwd(unet)
    want, P2 = fresh(tr)
    for k, t in ups.items():
        assert unet.P.cache[k] is t and torch.equal(t, P2.cache[k]), k
    e2, d2 = float((got - want).norm() / want.norm()), float((base - want).norm() / want.norm())
    print("after the in-place refresh of existing folds: vs fresh UNet", e2, " vs untrained", d2)
    assert e2 < 1e-2 and d2 > 10 * e2, (e2, d2)


def test_plan_recorded_before_tuning_the_upsamplers_replays_the_tuned_weights(unet_sd_np, cn_sd_np):
    """A denoise_step_planned plan recorded BEFORE a tuner that trains upsamplers.0.conv (and a GroupNorm, a resnet convolution): the plan captured the folded
    [N, 16, K] tensors; replayed after two steps it equals the eager step of the tuned pipeline bit for bit and differs from the untuned step."""
    from motioneditor_amd import util
    from motioneditor_amd.models.controlnet import ControlNetModel
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    from motioneditor_amd.pipelines import MotionEditorPipeline
    from test_step_cpu import step_inputs
    c = tf.golden()
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
    ups = {k: (v, v.clone()) for k, v in pipe.unet.P.cache.items() if k.startswith("ups4:")}
    assert len(ups) == 3
    tr = util.UNetTuner(pipe.unet, trainable_modules=("upsamplers.0.conv", "resnets.0.norm1", "resnets.1.conv2"), lr=tf.LR)
    tr.step(c["noisy"], c["t"], c["ehs"], c["noise"])
    tr.step(c["noisy"], c["t"], c["ehs"], c["noise"])
    for k, (v, v0) in ups.items():
        assert pipe.unet.P.cache[k] is v and not torch.equal(v, v0), k
    n_plans = len(pipe._plans)
    replay = pipe.denoise_step_planned(lat, t, emb, images, 7.5).clone()
    assert len(pipe._plans) == n_plans, "the plan was recorded again instead of replayed"
    eager = pipe.denoise_step(lat, t, emb, images, 7.5)
    torch.cuda.synchronize()
    assert torch.equal(replay, eager)
    assert not torch.equal(replay, before)
