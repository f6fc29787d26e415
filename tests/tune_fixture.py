"""TEST INFRASTRUCTURE shared by tests/test_tune_conv_cpu.py and tests/test_tune_conv_gpu.py: the widened stage-1 selection, the clip of
tests/golden/bg_train.npz (8 frames x 8^2 latents: the UNet's levels reach 1 x 1 pixel, where eight of the nine taps of a 3x3 convolution are padding) and
the oracle (oracle.ref_cpu.unet_forward under torch autograd + clip_grad_norm_ + torch.optim.AdamW), computed once per process."""
from __future__ import annotations

import functools

import numpy as np
import torch

from conftest import GOLD

T = torch.from_numpy
LR = 1e-3   # a visible step (the reference's 3e-5 moves fp32 weights by 1e-5)

# train_bg.py's filter matches module-path SUFFIXES, so a bare "conv1" would also select resnets.*.temp_conv1 and a bare "norm1" the LayerNorm
# transformer_blocks.0.norm1 -- both still refused by name.  The suffixes below select exactly the modules the widened tuner accepts: the default three, every
# resnet's conv1 / conv2 / conv_shortcut / norm1 / norm2 (a block has up to three resnets), the down- and upsampler convolutions, every proj_in / proj_out
# and the GroupNorm of the first transformer of every attention block.
MODULES = ("attn1.to_q", "attn2.to_q", "attn_temp", ".conv1", ".conv2", "conv_shortcut", "downsamplers.0.conv", "upsamplers.0.conv", "proj_in", "proj_out",
           "resnets.0.norm1", "resnets.1.norm1", "resnets.2.norm1", "resnets.0.norm2", "resnets.1.norm2", "resnets.2.norm2", "attentions.0.norm")


def golden():
    g = np.load(GOLD / "bg_train.npz")
    F32 = lambda k: T(g[k].astype(np.float32))   # noqa: E731
    return dict(noisy=F32("noisy"), noise=F32("noise"), ehs=F32("ehs"), t=int(g["t"]))


def selected(unet_sd_np):
    from motioneditor_amd import weights
    return sorted(n for n in weights.select_trainable(list(unet_sd_np), MODULES) if not n.startswith("controlnet_adapter."))


@functools.lru_cache(maxsize=1)
def _oracle(key):
    from motioneditor_amd import synth
    from oracle import ref_cpu
    sd_np = synth.synth_state_dict(synth.unet_schema())
    sd = {k: T(v).clone() for k, v in sd_np.items()}
    names, c = selected(sd_np), golden()
    params = {k: torch.nn.Parameter(sd[k].clone()) for k in names}
    opt = torch.optim.AdamW(list(params.values()), lr=LR, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)
    losses, grads, after = [], None, []
    for _ in range(2):
        sd2 = dict(sd)
        sd2.update(params)
        loss = torch.nn.functional.mse_loss(ref_cpu.unet_forward(sd2, c["noisy"], c["t"], c["ehs"]), c["noise"])
        gs = torch.autograd.grad(loss, [params[k] for k in names])
        for k, gr in zip(names, gs):
            params[k].grad = gr
        if grads is None:
            grads = {k: gr.detach().clone() for k, gr in zip(names, gs)}
        torch.nn.utils.clip_grad_norm_(list(params.values()), 1.0)
        opt.step()
        losses.append(float(loss.detach()))
        after.append({k: v.detach().clone() for k, v in params.items()})
    with torch.no_grad():
        sd3 = dict(sd)
        sd3.update(after[1])
        losses.append(float(torch.nn.functional.mse_loss(ref_cpu.unet_forward(sd3, c["noisy"], c["t"], c["ehs"]), c["noise"])))
    return dict(names=names, grads=grads, after=after, losses=losses, sd=sd)


def oracle():
    """names, the first step's gradients, the parameters after one and two oracle steps, the losses at steps 1, 2 and at the parameters after step 2, and the
    untrained state (torch tensors).  The synthetic UNet is deterministic, so one computation serves every test of the process; nothing mutates it."""
    return _oracle("unet")


# ---------------------------------------------------------------------------------------------------------------- kernel-level inputs (seeded, CPU tensors)
def conv_dw_inputs(n_img, Hin, Win, N, K, stride, ups, seed=0):
    """(x fp16 [n_img Hin Win, K], dy fp32 [M, N], dst0 fp32 [N, 9, K] non-zero, conv tuple, M) of one me_conv_dw call."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * N + K + Hin)
    Hout, Wout = ((Hin << ups) - 1) // stride + 1, ((Win << ups) - 1) // stride + 1
    M = n_img * Hout * Wout
    x = torch.randn(n_img * Hin * Win, K, generator=g).half()
    dy = torch.randn(M, N, generator=g)
    dst0 = torch.randn(N, 9, K, generator=g) * 0.5
    return x, dy, dst0, (Hin, Win, Hout, Wout, stride, ups), M


def conv_dw_ref64(x, dy, conv, M, alpha):
    """fp64 dW [N, 9, K] of the fp16-rounded operands (tests/ref64_bwd.py differentiates its own forward gather)."""
    import ref64_bwd
    return ref64_bwd.gemm_dw(dy, x, dst=torch.zeros((dy.shape[1], 9, x.shape[1]), dtype=torch.float64), taps=9, K=x.shape[1], M=M, alpha=alpha, conv=conv)


# (C, groups, rows_per_group, sample groups): rows_per_group 200 = 8 frames x 5 x 5 pixels, the 5-D all-frames statistics of the UNet's resnets over two batch
# rows; rows_per_group 6 = one 2 x 3 frame, the per-frame statistics of the transformer blocks' GroupNorm over three images
GN_CASES = [(320, 32, 200, 2), (320, 32, 6, 3), (64, 32, 200, 2), (64, 32, 6, 3)]


def gn_inputs(C, rpg, nsg, seed=0):
    g = torch.Generator().manual_seed(100 * seed + C + rpg)
    rows = nsg * rpg
    x = (torch.randn(rows, C, generator=g) * 1.5 + 0.5).half()
    gamma, beta = (1 + 0.2 * torch.randn(C, generator=g)).half(), (0.2 * torch.randn(C, generator=g)).half()
    dy = torch.randn(rows, C, generator=g)
    return x, gamma, beta, dy, torch.randn(C, generator=g), torch.randn(C, generator=g)


def gn_params_ref64(x, gamma, beta, dy, rpg, groups, silu):
    """fp64 autograd of tests/ref64_bwd.py's GroupNorm forward w.r.t. gamma and beta."""
    import ref64_bwd
    g0, b0 = gamma.double().clone().requires_grad_(True), beta.double().clone().requires_grad_(True)
    y = ref64_bwd._groupnorm(x.double(), g0, b0, rows_per_group=rpg, eps=1e-5, silu=silu, groups=groups)
    return torch.autograd.grad(y, [g0, b0], dy.double())
