"""TEST INFRASTRUCTURE shared by test_tape_memory_cpu.py and test_tape_memory_gpu.py: the three forms of the autodiff tape --
`parent` (keeps everything: autodiff.PARENT_FORM), `lean` (recorded towards wrt / trainable, released during the walk) and `ckpt` (lean + segment
recomputation, with the recomputation check on) -- of the three consumers in util.py, on one backend.  Every comparison the tests make on what these
return is torch.equal: the forms run the same rules in the same order on the same values."""
import contextlib

import torch

import bwd_run as br
import long_bwd_cases as lb

FORMS = ("parent", "lean", "ckpt")


@contextlib.contextmanager
def form(name: str):
    from motioneditor_amd import autodiff
    saved = autodiff.PARENT_FORM, autodiff.CHECK_RECOMPUTE
    autodiff.PARENT_FORM, autodiff.CHECK_RECOMPUTE = name == "parent", True
    try:
        yield name == "ckpt"
    finally:
        autodiff.PARENT_FORM, autodiff.CHECK_RECOMPUTE = saved


def make_unet(sd_np, device):
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    return UNet2DConditionModel(sd_np, device=device) if device != "cpu" else UNet2DConditionModel(sd_np, device="cpu", dtype=torch.float32)


def adapter_grads(unet, name: str, f: int = 8, h: int = 8):
    """-> (loss, {parameter: gradient}, stats) of util.adapter_training_grads on br.training_clip(0, f, h)."""
    from motioneditor_amd import util
    c = br.training_clip(0, f=f, h=h)
    stats = {}
    with form(name) as ckpt:
        loss, grads = util.adapter_training_grads(unet, c["noisy"], c["t"], c["ehs"], c["down"], c["mid"], c["noise"], gradient_checkpointing=ckpt, stats=stats)
    return loss, grads, stats


def null_text(unet, name: str, f: int = 8, inner: int = 2):
    """-> (first gradient, optimised embedding) of one DDIM step with `inner` inner steps of util.null_optimization on lb.null_text_inputs(f)."""
    from motioneditor_amd import util
    from motioneditor_amd.schedulers import DDIMScheduler
    latents, context = lb.null_text_inputs(f)
    sched = DDIMScheduler()
    sched.set_timesteps(50)

    class Pipe:
        pass
    pipe = Pipe()
    pipe.unet = unet
    grads = []
    with form(name) as ckpt:
        out = util.null_optimization(pipe, sched, latents, context, inner, -1.0, num_ddim_steps=1, grads=grads, gradient_checkpointing=ckpt)   # epsilon < 0: no early stop
    assert len(grads) == inner and len(out) == 1
    return grads[0], out[0]


TUNER_SETS = {"default": {},
              "conv_gn": dict(trainable_modules=("attn1.to_q",), trainable_params=("up_blocks.1.resnets.0.conv1.weight", "up_blocks.1.resnets.0.norm2.weight",
                                                                                      "up_blocks.1.resnets.0.norm2.bias", "down_blocks.1.resnets.0.conv2.weight"))}


def tuner_masters(sd_np, device, name: str, which: str, f: int = 8):
    """-> (loss, the fp32 masters after one util.UNetTuner.step) on br.training_clip(1, f, 8).  A fresh model per call: the step rewrites weights in place."""
    from motioneditor_amd import util
    c = br.training_clip(1, f=f, h=8)
    with form(name) as ckpt:
        tr = util.UNetTuner(make_unet(sd_np, device), lr=1e-3, gradient_checkpointing=ckpt, **TUNER_SETS[which])
        loss = tr.step(c["noisy"], c["t"], c["ehs"], c["noise"])
    assert tr.steps == 1
    return loss, tr.master.clone()


def same(a, b) -> bool:
    return a.shape == b.shape and torch.equal(a, b)
