"""Generate tests/golden/bg_train.npz: the arithmetic of one stage-1 training step of the REFERENCE (train_bg.py:162-174 parameter selection,
:340-346 forward / mse / backward) with the reference's own UNet.

Test infrastructure, not product code: it needs the reference tree, which it imports through oracle/shim exactly as oracle/make_golden.py does
(whose helpers it reuses).  Before anything is written, oracle/ref_cpu.unet_forward under autograd must reproduce the reference's loss (1e-4
relative) and the gradients of every selected parameter (1e-3 relative L2).

Usage:  python tools/make_golden_bg_train.py
"""
from __future__ import annotations

import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from oracle import make_golden as mg  # noqa: E402  (puts oracle/shim and the reference on sys.path)
from oracle import ref_cpu  # noqa: E402
from motioneditor_amd import synth  # noqa: E402

TRAINABLE_MODULES = ("attn1.to_q", "attn2.to_q", "attn_temp")   # train_bg.py:99-103
FULL = ["down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_q.weight",
        "mid_block.attentions.0.transformer_blocks.0.attn_temp.to_out.0.bias",
        "up_blocks.3.attentions.2.transformer_blocks.0.attn_temp.to_out.0.bias"]


def main() -> None:
    sd_np = synth.synth_state_dict(synth.unet_schema())
    unet = mg.build_reference_unet(sd_np)
    sd = {k: torch.from_numpy(v) for k, v in sd_np.items()}
    # train_bg.py:162-174, on the reference model itself
    unet.requires_grad_(False)
    for name, module in unet.named_modules():
        if name.endswith(TRAINABLE_MODULES):
            for p in module.parameters():
                p.requires_grad = True
    params = dict(unet.named_parameters())
    selected = [k for k, p in params.items() if p.requires_grad]

    B, f, h, w = 1, 8, 8, 8
    g = torch.Generator().manual_seed(4242)
    r16 = lambda x: x.half().float()   # noqa: E731  (fp16-representable inputs: stored as fp16 without loss)
    noisy = r16(torch.randn(B, 4, f, h, w, generator=g))
    noise = r16(torch.randn(B, 4, f, h, w, generator=g))
    ehs = r16(torch.randn(B, 77, 768, generator=g) * 0.3)
    t = int(torch.randint(0, 1000, (1,), generator=g))

    t0 = time.time()
    pred = mg.quiet(unet, noisy, torch.tensor([t]), encoder_hidden_states=ehs).sample
    loss = torch.nn.functional.mse_loss(pred.float(), noise.float(), reduction="mean")
    loss.backward()
    print(f"reference stage-1 forward + backward {time.time() - t0:.1f}s, t {t}, loss {float(loss):.6f}")
    with_grad = [k for k in selected if params[k].grad is not None]
    without = [k for k in selected if params[k].grad is None]
    ref_g = {k: params[k].grad.detach().clone() for k in with_grad}

    sd2 = dict(sd)
    for k in with_grad:
        sd2[k] = sd[k].clone().requires_grad_(True)
    loss2 = torch.nn.functional.mse_loss(ref_cpu.unet_forward(sd2, noisy, t, ehs), noise)
    gr = torch.autograd.grad(loss2, [sd2[k] for k in with_grad])
    num = sum(float((a - ref_g[k]).pow(2).sum()) for a, k in zip(gr, with_grad))
    tot = (num / sum(float(ref_g[k].pow(2).sum()) for k in with_grad)) ** 0.5
    print("oracle vs reference: loss", float(loss2), "vs", float(loss), " gradient rel-L2", tot, f" {len(with_grad)} with / {len(without)} without a gradient")
    assert abs(float(loss2) - float(loss)) < 1e-4 * float(loss) and tot < 1e-3, (float(loss2), float(loss), tot)

    h16 = lambda x: x.numpy().astype(np.float16)   # noqa: E731
    out = ROOT / "tests" / "golden" / "bg_train.npz"
    np.savez_compressed(out, noisy=h16(noisy), noise=h16(noise), ehs=h16(ehs), t=t, loss=float(loss), names=np.array(with_grad),
                        grad_norms=np.array([float(ref_g[k].norm()) for k in with_grad], dtype=np.float64), unreached=np.array(without),
                        full_names=np.array(FULL), **{f"full_{i}": ref_g[k].numpy() for i, k in enumerate(FULL)}, oracle_grad_relerr=tot)
    print(out, "written:", out.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
