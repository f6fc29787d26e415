"""TEST INFRASTRUCTURE shared by tests/test_multi_edit_cpu.py and tests/test_multi_edit_gpu.py: seeded inputs for one source and up to three targets,
and the oracle's answer for target k -- oracle/ref_cpu.denoise_step on the two rows (source, target k), which by definition is what the batched step must
give for (rec, e_k).  That answer does not depend on how many targets share the batch, so it is computed once per (geometry, target, step, masks) and
shared by every test of a session; nothing writes to it."""
import numpy as np
import torch

from motioneditor_amd import synth
from oracle import ref_cpu

MAX_N = 3


def multi_inputs(f=8, h=8, w=8, seed=33):
    """One source and MAX_N targets: every target has its own latent, prompt embedding and skeleton (a test of N targets takes the first N)."""
    T = torch.from_numpy
    return dict(latents=T(synth.synth_normal("multi.latents", (1 + MAX_N, 4, f, h, w), seed)),
                uncond=T(synth.synth_normal("multi.uncond", (1, 77, 768), seed, 0.3)),
                cond=T(synth.synth_normal("multi.cond", (1 + MAX_N, 77, 768), seed, 0.3)),
                skeletons=T(np.clip(synth.synth_normal("multi.skel", (MAX_N, f, 3, 8 * h, 8 * w), seed, 0.5) + 0.5, 0, 1)),
                masks=T(synth.synth_masks(f, 8 * h, 8 * w)))


def soft_masks(masks):
    g = torch.Generator().manual_seed(17)
    soft = (0.15 + 0.7 * masks.float() + 0.1 * torch.rand(masks.shape, generator=g)).clamp(0, 1)
    assert not bool(((soft == 0) | (soft == 1)).all())
    return soft


def batch_of(x, targets):
    """(latents [1+N], text rows [2(1+N)], images [(2 N f),3,H,W]) of the batched step for the targets `targets` (1-based, in this order)."""
    rows = [0] + list(targets)
    lat, cond = x["latents"][rows], x["cond"][rows]
    emb = torch.cat([x["uncond"].expand(len(rows), 77, 768), cond])
    sk = x["skeletons"][[k - 1 for k in targets]]
    images = torch.cat([sk] * 2).reshape(-1, *sk.shape[2:])
    return lat.contiguous(), emb.contiguous(), images.contiguous()


_want = {}


def oracle_pair(x, key, k, step, unet_sd_torch, cn_sd_torch, masks=None, start_step=4):
    """(latents [2,4,f,h,w] after the step, guided noise prediction [2,4,f,h,w]) of the oracle's two-row step of (source, target k) at `step`."""
    ck = (key, k, step, masks is not None, start_step)
    if ck not in _want:
        m = x["masks"] if masks is None else masks
        ddim = ref_cpu.DDIM()
        sp, tp = ref_cpu.SpatialEditor(m, start_step=start_step), ref_cpu.TemporalEditor(start_step=start_step)      # (start_layer 10; active from start_step on)
        sp.cur_step = tp.cur_step = step
        f = x["latents"].shape[2]
        sk = x["skeletons"][k - 1:k]
        images = torch.cat([sk] * 2).reshape(2 * f, *sk.shape[2:])
        taps = {}
        with torch.no_grad():
            lat = ref_cpu.denoise_step(unet_sd_torch, cn_sd_torch, ddim, x["latents"][[0, k]], ddim.timesteps[step], x["uncond"], x["cond"][[0, k]], images, sp, tp, 7.5,
                                       taps=taps)
        _want[ck] = (lat, taps["noise_pred"])
    return _want[ck]
