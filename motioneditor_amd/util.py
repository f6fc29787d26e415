"""DDIM inversion, the step in front of the denoising loop (reference `motion_editor/util.py:77-130`, called from
`inference.py:289-293` with `normal_infer=True`).  Same signatures; the prompt may be given as ready text embeddings
(`text_embeddings=[1,77,768]`) when the pipeline carries no text encoder.  Also here: the null-text optimisation that follows it
(`p2p/null_text_optimization.py:133-166`) and the adapter training step (`train_adaptor.py:364-385`), both on the reverse-mode tape of
`motioneditor_amd/autodiff.py` with loss, gradient norm and the Adam / AdamW update as device kernels (csrc/train.hip)."""
from __future__ import annotations

import math
from typing import List, Optional

import torch

from . import ops


def next_coeffs(ddim_scheduler, timestep: int):
    """next_sample = ca * sample + cb * model_output  (util.py:77-87 collapsed to one linear update)."""
    n_train = ddim_scheduler.config.num_train_timesteps
    cur_t = min(int(timestep) - n_train // ddim_scheduler.num_inference_steps, 999)
    a_c = float(ddim_scheduler.alphas_cumprod[cur_t]) if cur_t >= 0 else float(ddim_scheduler.final_alpha_cumprod)
    a_n = float(ddim_scheduler.alphas_cumprod[int(timestep)])
    return (a_n / a_c) ** 0.5, (1 - a_n) ** 0.5 - (a_n * (1 - a_c) / a_c) ** 0.5


def next_step(model_output: torch.Tensor, timestep: int, sample: torch.Tensor, ddim_scheduler) -> torch.Tensor:
    """util.py:77-87 on reference-layout tensors [B,4,f,h,w] (fp32 latents, any float model output)."""
    ca, cb = next_coeffs(ddim_scheduler, timestep)
    return ca * sample + cb * model_output.to(sample.dtype)


def _context(pipeline, prompt, text_embeddings: Optional[torch.Tensor]) -> torch.Tensor:
    if text_embeddings is not None:
        return text_embeddings
    if getattr(pipeline, "text_encoder", None) is None:
        raise ValueError("ddim_loop needs text_embeddings= when the pipeline has no text encoder")
    tok = pipeline.tokenizer([prompt], padding="max_length", max_length=pipeline.tokenizer.model_max_length, truncation=True, return_tensors="pt")
    return pipeline.text_encoder(tok.input_ids.to(pipeline.device))[0]      # util.py:64-71 (conditional half of init_prompt)


@torch.no_grad()
def ddim_loop(pipeline, ddim_scheduler, latent: torch.Tensor, num_inv_steps: int, prompt: str = "", normal_infer: bool = False,
              text_embeddings: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
    """util.py:111-124: one single-branch UNet forward on the conditional embedding per step, walking the timesteps
    upwards.  The linear update runs in the fused `me_cfg_ddim` kernel (guidance 1 on a duplicated noise prediction
    selects it unchanged)."""
    cond = _context(pipeline, prompt, text_embeddings)
    unet = pipeline.unet
    latent = latent.to(unet.device, torch.float32).contiguous()
    all_latent = [latent]
    for i in range(num_inv_steps):
        t = ddim_scheduler.timesteps[len(ddim_scheduler.timesteps) - i - 1]
        ehs = cond if cond.shape[0] == latent.shape[0] else cond.repeat(latent.shape[0], 1, 1)   # util.py:91-93
        eps = unet.forward_rows(latent, t, ehs, normal_infer=normal_infer).t
        ca, cb = next_coeffs(ddim_scheduler, int(t))
        latent = ops.cfg_ddim(latent, torch.cat([eps, eps]), guidance=1.0, ca=ca, cb=cb)
        all_latent.append(latent)
    return all_latent


@torch.no_grad()
def ddim_inversion(pipeline, ddim_scheduler, video_latent: torch.Tensor, num_inv_steps: int, prompt: str = "", normal_infer: bool = False,
                   text_embeddings: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
    """util.py:127-130."""
    return ddim_loop(pipeline, ddim_scheduler, video_latent, num_inv_steps, prompt, normal_infer=normal_infer, text_embeddings=text_embeddings)


# ---------------------------------------------------------------------------------------------------------------------
# Null-text optimisation (p2p/null_text_optimization.py:133-166; inference.py:277-287 runs it before the editing loop)
# ---------------------------------------------------------------------------------------------------------------------
def _loss_scale(amax: float) -> float:
    """The backward kernels carry gradients between layers in fp16 (like every activation): a power of two brings the seed's largest
    element to ~64; it is divided out again by the optimiser kernel (grad_scale)."""
    return 2.0 ** math.floor(math.log2(64.0 / amax)) if amax > 0.0 and math.isfinite(amax) else 1.0


def _checkpointing(unet, gradient_checkpointing: Optional[bool]) -> bool:
    """An entry point's `gradient_checkpointing=`: None reads the model's flag (unet.enable_gradient_checkpointing())."""
    return bool(getattr(unet, "gradient_checkpointing", False)) if gradient_checkpointing is None else bool(gradient_checkpointing)


def _tape_stats(stats: Optional[dict], tape=None, G=None) -> None:
    """What the tape held (autodiff.Tape.stashed_bytes, read at the end of the forward) and the gradient store's high-water mark, for callers that ask."""
    if stats is None:
        return
    if tape is not None:
        stats["stashed_bytes"] = tape.stashed_bytes()
    if G is not None:
        stats["grad_peak_bytes"], stats["grad_total_bytes"] = G.peak_bytes, G.total_bytes


def null_optimization(pipeline, ddim_scheduler, latents, context: torch.Tensor, null_inner_steps: int = 10, epsilon: float = 1e-5,
                      num_ddim_steps: Optional[int] = None, guidance_scale: float = 7.5, grads: Optional[list] = None,
                      gradient_checkpointing: Optional[bool] = None, stats: Optional[dict] = None) -> List[torch.Tensor]:
    """MyNullInversion.null_optimization: for each DDIM step a fresh Adam (lr 1e-2 (1 - i / 100)) moves the unconditional text
    embedding so that the guided prev_step of the current latent reproduces the inversion latent one step earlier; early stop at
    loss < epsilon + 2e-5 i; the latent then advances with the optimised embedding.  latents = the DDIM inversion trajectory
    (util.ddim_inversion), context = [uncond, cond] (2, 77, 768).  Returns the list of optimised [1, 77, 768] embeddings
    (what the pipeline takes as `uncond_embeddings`).

    The reference differentiates with torch autograd; here the forward is the same launch graph as everywhere else, the gradient
    comes from motioneditor_amd.autodiff (a tape over the C-ABI operators and their backward kernels) and the loss (me_mse_seed +
    me_sumsq_absmax), the loss-scale selection and Adam (me_adamw on the fp32 embedding) are device kernels too: the host reads two
    floats per inner step (the loss for the early stop, the seed's largest element for the loss scale).  As in the reference
    (`:49-51` hard-codes it) the UNet runs with normal_infer=False -- sparse-causal attn1 -- and without editors.

    The tape is recorded towards the text rows (autodiff.record(wrt=)): what is not downstream of them is neither logged nor kept.
    gradient_checkpointing (default: the flag unet.enable_gradient_checkpointing() sets): the UNet's blocks keep their boundary tensors only
    and are recomputed in the backward walk -- same gradient bit for bit, one more forward of the differentiated blocks.
    stats: a dict that receives the last inner step's stashed_bytes / grad_peak_bytes / grad_total_bytes."""
    from . import autodiff
    from .models import graph
    B_ = graph.ops
    unet = pipeline.unet
    P = unet.P
    dev = unet.device
    n = len(ddim_scheduler.timesteps) if num_ddim_steps is None else num_ddim_steps
    ckpt = _checkpointing(unet, gradient_checkpointing)
    uncond0, cond = context.to(dev).float().chunk(2)
    cond_rows = graph.text_rows(cond, P.dtype)
    out: List[torch.Tensor] = []
    latent_cur = latents[-1].to(dev).float().contiguous()
    nel = latent_cur.numel()
    uncond = uncond0.reshape(-1, uncond0.shape[-1]).contiguous().clone()          # fp32 master [77, 768]; Adam updates it in place

    def text_of(u32):   # the rows the UNet projects to K / V: OUR allocation, so that the gradient store can be asked for it
        rows = torch.empty(u32.shape, dtype=P.dtype, device=dev)
        return B_.cast_f16(rows, u32)

    for i in range(n):
        m_, v_ = torch.zeros_like(uncond), torch.zeros_like(uncond)              # a fresh Adam per DDIM step (:141)
        lr = 1e-2 * (1.0 - i / 100.0)
        latent_prev = latents[len(latents) - i - 2].to(dev).float().contiguous()
        t = ddim_scheduler.timesteps[i]
        ca, cb = ddim_scheduler.coeffs(int(t))
        eps_c = graph.unet_forward(P, latent_cur, float(t), cond_rows).t          # rows [(f h w), 4]
        for k in range(null_inner_steps):
            text = text_of(uncond)
            with (autodiff.record(graph) if autodiff.PARENT_FORM else autodiff.record(graph, wrt=[text], checkpoint=ckpt)) as tape:
                act = graph.unet_forward(P, latent_cur, float(t), text)
            _tape_stats(stats, tape=tape)
            # rec = prev_step(eps_u + g (eps_c - eps_u)) (:26-36), loss = mse(rec, latent_prev), d loss / d eps_u in the UNet's row layout
            diff, d_rows = B_.mse_seed(act.t, latent_prev, eps_c=eps_c, x=latent_cur, guidance=guidance_scale, ca=ca, cb=cb,
                                       coef=(2.0 / nel) * cb * (1.0 - guidance_scale))
            st = torch.cat([B_.sumsq_absmax(diff), B_.sumsq_absmax(d_rows)]).tolist()     # one host read: loss, seed magnitude
            loss = st[0] / nel
            ls = _loss_scale(st[3])
            G = autodiff.backward(tape, [(act.t, d_rows)], seed_scale=ls, wrt=[text])   # only what lies downstream of the text rows is walked
            g = G.view(text)
            _tape_stats(stats, G=G)
            if grads is not None:      # test hook (not part of the reference): the un-scaled gradient of this inner step
                grads.append((g / ls).reshape(uncond0.shape).clone())
            B_.adamw(uncond, m_, v_, g.contiguous(), lr=lr, step=k + 1, grad_scale=1.0 / ls)
            del tape, G
            if loss < epsilon + i * 2e-5:
                break
        out.append(uncond.reshape(uncond0.shape).clone())
        both = graph.unet_forward(P, torch.cat([latent_cur] * 2), float(t), torch.cat([text_of(uncond), cond_rows]), cfg_dup=True)   # the two rows are copies up to the text
        latent_cur = B_.cfg_ddim(latent_cur, both.t, guidance=guidance_scale, ca=ca, cb=cb)       # get_noise_pred + prev_step (:53-65)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Adapter training step, the arithmetic of train_adaptor.py:364-368
# ---------------------------------------------------------------------------------------------------------------------
def _unet_backward(unet, noisy_latents, timestep, encoder_hidden_states, down_block_res_samples, mid_block_res_sample, target, trainable, param_buffers=None,
                   sync_amax=None, gradient_checkpointing: Optional[bool] = None, stats: Optional[dict] = None):
    """Forward on the tape, loss, backward.  -> (loss, loss scale, gradient store); the gradients of the packed tensors `trainable()` names after the
    forward (autodiff.backward's `trainable`; packed layouts, times the loss scale) are accumulated into `param_buffers[key]` when given.  No residuals (None, None): the plain UNet forward.
    sync_amax: callable(tensor [2]) that makes the seed magnitude -- and with it the loss scale -- the same on every data-parallel rank (a MAX
    all-reduce), so that the gradient buckets can be summed.
    The tape is recorded towards the trained tensors (autodiff.record(trainable=)): `trainable` is asked again whenever the weight store has packed
    something new, so that a call's weight is known as the call is recorded.  gradient_checkpointing / stats: as in null_optimization."""
    from . import autodiff
    from .models import graph
    B_ = graph.ops
    P = unet.P
    dev = unet.device
    rows = lambda r: r if r.dim() == 2 else B_.nchw5_to_rows(r.to(dev))   # noqa: E731
    down = None if down_block_res_samples is None else [rows(r) for r in down_block_res_samples]
    mid = None if mid_block_res_sample is None else rows(mid_block_res_sample)
    ehs = graph.text_rows(encoder_hidden_states.to(dev), P.dtype).clone()
    t = float(timestep.item() if torch.is_tensor(timestep) else timestep)
    known = [-1, None]

    def current():   # packed tensors come into being at their first use: re-read when the store has grown
        if known[0] != len(P.cache):
            known[0], known[1] = len(P.cache), trainable()
        return known[1]
    with (autodiff.record(graph) if autodiff.PARENT_FORM else
          autodiff.record(graph, trainable=current, checkpoint=_checkpointing(unet, gradient_checkpointing))) as tape:
        act = graph.unet_forward(P, noisy_latents.to(dev), t, ehs, down_res=down, mid_res=mid, two_branch=False)
    _tape_stats(stats, tape=tape)
    tgt = target.to(dev).float().contiguous()
    diff, d_rows = B_.mse_seed(act.t, tgt, coef=2.0 / tgt.numel())          # loss = mse(model_pred, target) (:368)
    amax = B_.sumsq_absmax(d_rows)
    if sync_amax is not None:
        sync_amax(amax)
    st = torch.cat([B_.sumsq_absmax(diff), amax]).tolist()
    loss, ls = st[0] / tgt.numel(), _loss_scale(st[3])
    G = autodiff.backward(tape, [(act.t, d_rows)], trainable=trainable(), seed_scale=ls, param_buffers=param_buffers)
    _tape_stats(stats, G=G)
    return loss, ls, G


def adapter_training_grads(unet, noisy_latents: torch.Tensor, timestep, encoder_hidden_states: torch.Tensor, down_block_res_samples, mid_block_res_sample,
                           target: torch.Tensor, prefix: str = "controlnet_adapter.", gradient_checkpointing: Optional[bool] = None,
                           stats: Optional[dict] = None):
    """loss = mse(unet(noisy, t, ehs, down_block_additional_residuals, mid_block_additional_residual), target) on ONE clip and its gradient
    w.r.t. every parameter under `prefix`, keyed by the reference's parameter names and in the reference's layouts (host tensors) -- what
    `accelerator.backward(loss)` leaves in `.grad` of the adapter (the reference trains nothing else: train_adaptor.py freezes the
    rest).  Residuals in the reference layout [b, C, f, h', w'] (ControlNet outputs, no gradient).  The forward is the ordinary
    launch graph on an autodiff tape.  This is the inspection / export form; the training step itself (AdapterTrainer) keeps the gradients
    on the device in the packed layouts.  gradient_checkpointing / stats: as in null_optimization."""
    loss, ls, G = _unet_backward(unet, noisy_latents, timestep, encoder_hidden_states, down_block_res_samples, mid_block_res_sample, target, lambda: unet.P.trainable_ids(prefix),
                                 gradient_checkpointing=gradient_checkpointing, stats=stats)
    grads = {}
    for key, g in G.params.items():
        for name, gn in unet.P.unpack_grad(key, g).items():    # host copy in the reference layout
            gn = gn / ls
            grads[name] = grads[name] + gn if name in grads else gn
    return loss, grads


class AdapterTrainer:
    """One optimisation step of the content-aware motion adapter as train_adaptor.py:364-385 takes it, on the device: loss and gradients
    from the tape (every adapter parameter gradient accumulates straight into ONE flat fp32 bucket, in the packed layouts the kernels
    read), the data-parallel gradient average as one all-reduce of that bucket (RCCL on the GPU; what accelerate's DDP does for the
    reference), `clip_grad_norm_(max_grad_norm)` from a device reduction of the bucket, AdamW (the reference's defaults: lr 3e-5, betas
    (0.9, 0.999), weight decay 1e-2, eps 1e-8) on fp32 masters kept in the same packed layout, and the fp16 weights the forward reads
    refreshed IN PLACE from the masters by one cast kernel -- no gradient, master or optimiser state ever visits the host.  The loss is
    averaged over the ranks for logging as `:377` does.  `export_state_dict()` returns the trained parameters under the reference's names
    and layouts (what train_adaptor.py saves as the adapter checkpoint).  gradient_checkpointing: None follows unet.enable_gradient_checkpointing();
    `tape_stats`, when set to a dict, receives each step's stashed_bytes / grad_peak_bytes / grad_total_bytes."""

    def __init__(self, unet, lr: float = 3e-5, betas=(0.9, 0.999), weight_decay: float = 1e-2, eps: float = 1e-8, max_grad_norm: float = 1.0,
                 prefix: str = "controlnet_adapter.", group=None, gradient_checkpointing: Optional[bool] = None):
        from .models import graph
        self.unet, self.prefix, self.group, self.max_grad_norm = unet, prefix, group, max_grad_norm
        self.gradient_checkpointing, self.tape_stats = gradient_checkpointing, None
        self.lr, self.betas, self.weight_decay, self.eps = lr, betas, weight_decay, eps
        self.steps = 0
        self.skipped_steps = 0           # optimisation steps dropped because the gradient norm was not finite (fp16 overflow)
        P = unet.P
        P.make_private()                 # a private, mutable weight store
        self.names = sorted(k[len(P.prefix):] for k in P.state if k.startswith(P.prefix + prefix))
        self.keys = graph.adapter_pack(P, prefix)
        covered = sorted(n for k in self.keys for n in k.partition(":")[2].split("|"))
        if covered != self.names:
            raise RuntimeError("adapter_pack does not cover the adapter's parameters exactly once")
        dev = unet.device
        sizes = [P.cache[k].numel() for k in self.keys]
        total = (sum(sizes) + 3) // 4 * 4
        self.off = {}
        o = 0
        for k, n in zip(self.keys, sizes):
            self.off[k] = (o, n)
            o += n
        self.master = torch.zeros(total, dtype=torch.float32, device=dev)           # fp32 masters, packed layouts
        self.m, self.v, self.grad = torch.zeros_like(self.master), torch.zeros_like(self.master), torch.zeros_like(self.master)
        self.weights = torch.zeros(total, dtype=P.dtype, device=dev)                # what the forward reads (fp16 on the GPU)
        self.views = {}
        for k in self.keys:
            o, n = self.off[k]
            self.master[o:o + n].copy_(P.packed_f32(k).reshape(-1))                # exact fp32 values, not the fp16-rounded packing
            self.views[k] = P.rehome(k, self.weights[o:o + n])
        self.param_buffers = {k: self.grad[self.off[k][0]:self.off[k][0] + self.off[k][1]].view(self.views[k].shape) for k in self.keys}

    def _world(self) -> int:
        import torch.distributed as dist
        return dist.get_world_size(self.group) if (dist.is_available() and dist.is_initialized()) else 1

    def step(self, noisy_latents, timestep, encoder_hidden_states, down_block_res_samples, mid_block_res_sample, target) -> float:
        import torch.distributed as dist
        from .models import graph
        B_ = graph.ops
        world = self._world()
        dist_on = dist.is_available() and dist.is_initialized()
        self.grad.zero_()
        sync = None
        if dist_on:
            sync = lambda a: dist.all_reduce(a, op=dist.ReduceOp.MAX, group=self.group)   # noqa: E731  (one loss scale for every rank's bucket)
        loss, ls, G = _unet_backward(self.unet, noisy_latents, timestep, encoder_hidden_states, down_block_res_samples, mid_block_res_sample, target,
                                     lambda: self.unet.P.trainable_ids(self.prefix), param_buffers=self.param_buffers, sync_amax=sync,
                                     gradient_checkpointing=self.gradient_checkpointing, stats=self.tape_stats)
        stray = [k for k in G.params if k not in self.param_buffers]
        if stray:
            raise RuntimeError(f"a gradient reached packed tensors the trainer does not own: {stray[:3]}")
        if dist_on:
            dist.all_reduce(self.grad, group=self.group)                 # DP gradient sum: ONE bucket of every adapter gradient (averaged by grad_scale below)
            lt = torch.tensor([loss], dtype=torch.float32, device=self.grad.device)
            dist.all_reduce(lt, group=self.group)                        # train_adaptor.py:377 (accelerator.gather(loss).mean())
            loss = float(lt[0]) / world
        gn = B_.sumsq_absmax(self.grad)                                   # device scalar: sum of squares of the (scaled, summed) bucket
        if not bool(torch.isfinite(gn.reshape(-1)[0])):
            # an fp16 overflow somewhere downstream of the seed (the loss scale is chosen from the seed's magnitude): an inf / NaN gradient would
            # poison the masters and Adam's moments for good.  Skip the update, as accelerate's GradScaler does for the reference's fp16 runs.
            self.skipped_steps += 1
            return loss
        self.steps += 1
        B_.adamw(self.master, self.m, self.v, self.grad, lr=self.lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, weight_decay=self.weight_decay,
                 step=self.steps, gnorm_sq=gn, max_grad_norm=self.max_grad_norm, grad_scale=1.0 / (ls * world))
        B_.cast_f16(self.weights, self.master)                            # the packed weights of the next forward, in place
        B_.invalidate_transposed([v for v in self.views.values() if v.dim() == 3])
        return loss

    def export_state_dict(self):
        """{reference parameter name: fp32 host tensor in the reference layout} of the trained adapter parameters."""
        P = self.unet.P
        out = {}
        for k in self.keys:
            o, n = self.off[k]
            out.update(P.unpack_grad(k, self.master[o:o + n].view(self.views[k].shape)))
        for name, val in out.items():    # the model's own state follows the training: state_dict() / named_parameters() / .to(device) see the trained values
            P.state[P.prefix + name] = val.detach().cpu().clone()
        return out


# ---------------------------------------------------------------------------------------------------------------------
# Stage-1 background tuning of the UNet, the arithmetic of train_bg.py:162-174,202-208,326-350
# ---------------------------------------------------------------------------------------------------------------------
class UNetTuner:
    """One optimisation step of train_bg.py (stage 1) on the device: the parameters that train_bg.py's module / parameter filter selects
    (default: attn1.to_q, attn2.to_q and attn_temp of every transformer block; also accepted: the 3x3 convolutions of the residual blocks and of
    the down- / upsamplers, conv_shortcut, proj_in / proj_out and the GroupNorm affine parameters -- graph.unet_tune_pack names what is not) are
    trained on the plain UNet forward (no ControlNet residuals, sparse-causal attn1) against mse(model_pred, target), with clip_grad_norm_(max_grad_norm) and AdamW (the reference's defaults: lr 3e-5,
    betas (0.9, 0.999), weight decay 1e-2, eps 1e-8).

    The gradient bucket holds exactly the selected parameters the forward REACHES: the filter also matches the motion adapter's attn_temp,
    which this forward never runs -- torch.optim.AdamW skips those (their .grad stays None), so they are left out here and stay bitwise
    unchanged.  A reached parameter with an exactly zero gradient still takes AdamW's weight-decay step.  Parameters are trained on row
    ranges of the packed tensors that hold them (q of a fused q|k|v; k|v stay frozen and get no weight-gradient launch).

    Every weight derived from a trained parameter -- the fp16 packed tensors and the LayerNorm folds (W diag(gamma), colsum, W beta + b) of
    the inference forward, the folded upsampler weights (me_refresh_ups4) -- is rewritten IN PLACE after each update by one me_refresh_weights
    launch, so that recorded plans and captured graphs replay with the tuned weights; a derived tensor first built after tuning started is built from the live fp32 masters
    (weights.Packed.live).  No gradient, master or optimiser moment visits the host.  `save_checkpoint(dir)` writes what stage 2 and
    inference read back (checkpoint.load_unet_state_dict(resume_from_checkpoint=dir)).  gradient_checkpointing / `tape_stats`: as AdapterTrainer."""

    def __init__(self, unet, trainable_modules=("attn1.to_q", "attn2.to_q", "attn_temp"), trainable_params=(), lr: float = 3e-5, betas=(0.9, 0.999),
                 weight_decay: float = 1e-2, eps: float = 1e-8, max_grad_norm: float = 1.0, group=None, gradient_checkpointing: Optional[bool] = None):
        from .models import graph
        from .weights import select_trainable
        self.unet, self.group, self.max_grad_norm = unet, group, max_grad_norm
        self.gradient_checkpointing, self.tape_stats = gradient_checkpointing, None
        self.lr, self.betas, self.weight_decay, self.eps = lr, betas, weight_decay, eps
        self.steps = 0
        self.skipped_steps = 0
        P = unet.P
        P.make_private()
        selected = select_trainable([k[len(P.prefix):] for k in P.state if k.startswith(P.prefix)], trainable_modules, trainable_params)
        self.unreached = sorted(n for n in selected if n.startswith("controlnet_adapter."))   # the adapter runs with ControlNet residuals only
        self.names = sorted(n for n in selected if not n.startswith("controlnet_adapter."))
        if not self.names:
            raise ValueError("UNetTuner: the filter selects no parameter of the UNet forward")
        keys = graph.unet_tune_pack(P, self.names)
        want = set(self.names)
        slots, seen = [], set()
        for key in keys:
            for r0, r1, n in P.row_ranges(key):
                if n in want:
                    if n in seen:
                        raise RuntimeError(f"UNetTuner: {n} lies in two packed tensors of the forward")
                    seen.add(n)
                    slots.append((key, r0, r1, n))
        if seen != want:
            raise RuntimeError(f"UNetTuner: no packed tensor holds {sorted(want - seen)[:3]}")
        dev = unet.device
        off, o = {}, 0
        for key, r0, r1, n in slots:
            numel = (r1 - r0) * (P.cache[key][0].numel() if P.cache[key].dim() > 1 else 1)
            off[n] = (o, numel)
            o += (numel + 3) // 4 * 4                 # every slot 16-byte aligned (the refresh kernel's vector loads)
        self.master = torch.zeros(max(o, 4), dtype=torch.float32, device=dev)
        self.m, self.v, self.grad = torch.zeros_like(self.master), torch.zeros_like(self.master), torch.zeros_like(self.master)
        self.slots = slots
        self.kind = {n: key.partition(":")[0] for key, _, _, n in slots}
        self.masters, self.param_buffers = {}, {}
        packed = {}
        for key, r0, r1, n in slots:
            if key not in packed:
                packed[key] = P.packed_f32(key)            # exact fp32 values, not the fp16-rounded packing
            shape = (r1 - r0, *P.cache[key].shape[1:])
            o, numel = off[n]
            self.masters[n] = self.master[o:o + numel].view(shape)
            self.masters[n].copy_(packed[key][r0:r1].reshape(shape))
            self.param_buffers[n] = self.grad[o:o + numel].view(shape)
        del packed
        if P.device.type == "cpu":
            # a CPU store's fp32 packing of a Linear can be a VIEW of the caller's state array; the refresh rewrites packed tensors in place
            for key, t in list(P.cache.items()):
                kind, _, joined = key.partition(":")
                if kind in ("mat", "vec", "fused", "fvec", "geglu", "gegluv") and not want.isdisjoint(joined.split("|")):
                    P.cache[key] = t.clone()
        self.trainable = P.trainable_rows(keys, self.names)
        for n in self.names:                               # derived tensors built from now on read the live masters (a copy: never a view of one)
            P.live[n] = (lambda n=n: self._reference_layout(n).detach().to("cpu", copy=True))
        self._consts = {}
        self._table, self._table_sig = None, None

    # -- layouts ---------------------------------------------------------------------------------------------------------------------
    def _reference_layout(self, n: str, t: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The master of `n` (or `t`, a tensor in the same packed layout) in the reference's own layout, the shape P.raw(n) has: Linear [N, K],
        Conv2d [N, K, 3, 3] / [N, K, 1, 1] (packed tap-major as [N, 9, K] / [N, 1, K]) or a vector."""
        t, kind = (self.masters[n] if t is None else t), self.kind[n]
        if kind in ("geglu", "gegluv"):
            from .weights import Packed
            inv = torch.empty(t.shape[0], dtype=torch.long)
            inv[Packed._geglu_perm(t.shape[0] // 2)] = torch.arange(t.shape[0])
            t = t[inv.to(t.device)]
        if t.dim() != 3:
            return t.reshape(-1)
        shp = tuple(self.unet.P.state[self.unet.P.prefix + n].shape)      # from the state: never a live master's host copy
        if len(shp) == 4:                                                # [N, kh kw, K] -> [N, K, kh, kw]
            return t.reshape(shp[0], shp[2], shp[3], shp[1]).permute(0, 3, 1, 2)
        return t[:, 0, :]

    def _const(self, key: str, make) -> torch.Tensor:
        c = self._consts.get(key)
        if c is None:
            c = self._consts[key] = make().float().contiguous().to(self.unet.device)
        return c

    # -- the derived-weight refresh ----------------------------------------------------------------------------------------------------
    def _refresh_entries(self):
        """(entries for ops.refresh_table, 3-D tensors whose cached transposes go stale, signature of the cache entries they name)."""
        P = self.unet.P
        trained = set(self.names)
        ents, stale, sig = [], [], []
        for key, t in list(P.cache.items()):
            kind, _, joined = key.partition(":")
            ns = joined.split("|")
            if kind not in ("mat", "vec", "fused", "fvec", "geglu", "gegluv", "lnw", "lnwg", "ups4") or trained.isdisjoint(ns):
                continue
            if kind == "ups4":     # the folded form of a trained upsampler convolution: rewritten from the [N, 9, K] master by me_refresh_ups4
                sig.append((key, t.data_ptr()))
                ents.append((self.masters[ns[0]], t, None, None, None, None, None))
                continue
            if kind in ("lnw", "lnwg"):
                wq, colsum, cvec = t
                sig.append((key, wq.data_ptr(), colsum.data_ptr(), cvec.data_ptr()))
                stale.append(wq)
                norm_w, norm_b = ns[0], ns[1]
                gamma = self._const("g:" + norm_w, lambda: P.raw(norm_w).reshape(-1))
                beta = self._const("b:" + norm_b, lambda: P.raw(norm_b).reshape(-1))
                bias = next((n for n in ns[2:] if n.endswith(".bias")), None)
                bvec = None
                if bias is not None:
                    bvec = self.masters[bias].reshape(-1) if bias in trained else self._const(
                        "lnbias:" + key, lambda: P.packed_f32(("gegluv:" if kind == "lnwg" else "vec:") + bias).reshape(-1))
                K = wq.shape[2]
                for r0, r1, n in P.row_ranges(key):
                    if n not in trained and (bias is None or bias not in trained):
                        continue
                    src = self.masters[n].reshape(r1 - r0, K) if n in trained else self._const(
                        "w:" + n, lambda: P.packed_f32(("geglu:" if kind == "lnwg" else "mat:") + n).reshape(r1 - r0, K))
                    ents.append((src, wq[r0:r1].reshape(r1 - r0, K), gamma, beta, None if bvec is None else bvec[r0:r1], colsum[r0:r1], cvec[r0:r1]))
                continue
            sig.append((key, t.data_ptr()))
            if t.dim() == 3:
                stale.append(t)
            for r0, r1, n in P.row_ranges(key):
                if n in trained:
                    if t.dim() == 1:
                        ents.append((self.masters[n].reshape(1, -1), t[r0:r1].reshape(1, -1), None, None, None, None, None))
                    else:
                        ents.append((self.masters[n].reshape(r1 - r0, -1), t[r0:r1].reshape(r1 - r0, -1), None, None, None, None, None))
        return ents, stale, tuple(sig)

    def refresh(self) -> None:
        """Rewrite every derived weight of the trained parameters from the fp32 masters, in place, in one launch."""
        from .models import graph
        B_ = graph.ops
        ents, stale, sig = self._refresh_entries()
        if sig != self._table_sig:
            self._table = B_.refresh_table(ents)
            self._table_sig = sig
            self._stale = stale
        B_.refresh_weights(self._table)
        B_.invalidate_transposed(self._stale)

    # -- the step ------------------------------------------------------------------------------------------------------------------------
    def _world(self) -> int:
        import torch.distributed as dist
        return dist.get_world_size(self.group) if (dist.is_available() and dist.is_initialized()) else 1

    def step(self, noisy_latents, timestep, encoder_hidden_states, target) -> float:
        """train_bg.py:340-350 on one clip: model_pred = unet(noisy, t, ehs), loss = mse(model_pred, target), backward, clip, AdamW.  Returns the
        loss (averaged over the ranks of a process group, as accelerator.gather(loss).mean())."""
        import torch.distributed as dist
        from .models import graph
        B_ = graph.ops
        world = self._world()
        dist_on = dist.is_available() and dist.is_initialized()
        self.grad.zero_()
        sync = (lambda a: dist.all_reduce(a, op=dist.ReduceOp.MAX, group=self.group)) if dist_on else None
        loss, ls, G = _unet_backward(self.unet, noisy_latents, timestep, encoder_hidden_states, None, None, target, lambda: self.trainable,
                                     param_buffers=self.param_buffers, sync_amax=sync, gradient_checkpointing=self.gradient_checkpointing, stats=self.tape_stats)
        stray = [k for k in G.params if k not in self.param_buffers]
        if stray:
            raise RuntimeError(f"a gradient reached packed tensors the tuner does not own: {stray[:3]}")
        del G
        if dist_on:
            dist.all_reduce(self.grad, group=self.group)
            lt = torch.tensor([loss], dtype=torch.float32, device=self.grad.device)
            dist.all_reduce(lt, group=self.group)
            loss = float(lt[0]) / world
        gn = B_.sumsq_absmax(self.grad)
        if not bool(torch.isfinite(gn.reshape(-1)[0])):
            self.skipped_steps += 1          # fp16 overflow downstream of the seed: skip the update (accelerate's GradScaler does the same)
            return loss
        self.steps += 1
        B_.adamw(self.master, self.m, self.v, self.grad, lr=self.lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, weight_decay=self.weight_decay,
                 step=self.steps, gnorm_sq=gn, max_grad_norm=self.max_grad_norm, grad_scale=1.0 / (ls * world))
        self.refresh()
        return loss

    def grads(self, noisy_latents, timestep, encoder_hidden_states, target):
        """The inspection form of the step's backward (no update): (loss, {reference name: gradient, fp32 host tensor in the reference layout})
        of every parameter in the bucket -- what loss.backward() leaves in .grad on the reference."""
        self.grad.zero_()
        loss, ls, G = _unet_backward(self.unet, noisy_latents, timestep, encoder_hidden_states, None, None, target, lambda: self.trainable,
                                     param_buffers=self.param_buffers, gradient_checkpointing=self.gradient_checkpointing)
        del G
        out = {n: self._reference_layout(n, self.param_buffers[n] / ls).cpu().contiguous() for n in self.names}
        self.grad.zero_()
        return loss, out

    # -- export --------------------------------------------------------------------------------------------------------------------------
    def export_state_dict(self):
        """{reference parameter name: fp32 host tensor in the reference layout} of the trained parameters."""
        return {n: self._reference_layout(n).detach().cpu().contiguous().clone() for n in self.names}

    def save_checkpoint(self, directory) -> str:
        """`directory`/model.safetensors: the full UNet state in the reference key schema, trained parameters at their current values (the model
        weights of train_bg.py's checkpoint-N/; optimiser and RNG state are not written).  Returns the file's path."""
        import os
        from safetensors.torch import save_file
        P = self.unet.P
        out = {k[len(P.prefix):]: P.raw(k[len(P.prefix):]).contiguous().clone() for k in P.state if k.startswith(P.prefix)}
        out.update(self.export_state_dict())
        os.makedirs(directory, exist_ok=True)
        path = os.path.join(str(directory), "model.safetensors")
        save_file(out, path)
        return path


# ---------------------------------------------------------------------------------------------------------------------
# Video writers (reference `motion_editor/util.py:15-54`): same names and signatures.  The float -> uint8 grid is one device kernel
# (ops.video_grid_u8, csrc/image.hip) and one device -> host copy of uint8 frames; PIL writes the files.
# ---------------------------------------------------------------------------------------------------------------------
UPLOAD_DEVICE = "cuda"   # where a CPU tensor handed to the writers is uploaded to (the no-GPU tests point it at "cpu", beside the emulated ops)
GIF_FPS = 8   # util.py:46 `imageio.mimsave(path, outputs, fps=8)`: the GIF runs at 8 frames per second whatever `fps` says


def videos_to_grid_frames(videos: torch.Tensor, rescale: bool = False, n_rows: int = 4) -> torch.Tensor:
    """videos [b, c, t, h, w] (c = 1 or 3; a CPU tensor is uploaded first) -> uint8 host frames [t, Hg, Wg, 3]: per frame
    torchvision.utils.make_grid(x, nrow=n_rows), `(x + 1.0) / 2.0` when `rescale`, `(x * 255)` as uint8 (util.py:35-43).  One launch, one copy."""
    if not torch.is_tensor(videos) or videos.dim() != 5:
        raise ValueError("videos_to_grid_frames: expected a tensor [b, c, t, h, w]")
    v = videos.detach()
    if not v.is_cuda:
        v = v.to(UPLOAD_DEVICE)
    if v.dtype != torch.float32:
        v = v.float()
    return ops.video_grid_u8(v, n_rows=n_rows, rescale=bool(rescale)).cpu()


def save_videos_grid(videos: torch.Tensor, path: str, rescale=False, n_rows=4, fps=1):
    """util.py:34-54.  Writes the GIF (PIL: save_all, loop=0, 1000 / 8 = 125 ms per frame -- the reference hard-codes fps=8 for the GIF and uses `fps`
    only for the .mp4 twin it writes through imageio + ffmpeg).  The .mp4 is not written here (neither library exists on this platform), and a
    path that ends in .mp4 is refused."""
    import os
    from PIL import Image
    if str(path).lower().endswith(".mp4"):
        raise ValueError(f"save_videos_grid: {path}: .mp4 needs imageio + ffmpeg, which this package does not use; give a .gif path "
                         "(the reference's .mp4 twin of the GIF is not written)")
    frames = videos_to_grid_frames(videos, rescale=rescale, n_rows=n_rows).numpy()
    if os.path.dirname(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    ims = [Image.fromarray(f) for f in frames]
    ims[0].save(path, format="GIF", save_all=True, append_images=ims[1:], loop=0, duration=1000 // GIF_FPS)


def save_videos_as_images(videos: torch.Tensor, path: str, rescale=False, n_rows=4, fps=1):
    """util.py:15-31: `path`/vis_images/batch_{b}/frame_{t}.png, one lossless PNG per batch entry and frame (n_rows and fps are unused, as there)."""
    import os
    from PIL import Image
    if not torch.is_tensor(videos) or videos.dim() != 5:
        raise ValueError("save_videos_as_images: expected a tensor [b, c, t, h, w]")
    os.makedirs(os.path.join(path, "vis_images"), exist_ok=True)
    for batch_idx in range(videos.shape[0]):
        frames = videos_to_grid_frames(videos[batch_idx:batch_idx + 1], rescale=rescale).numpy()     # b = 1: the frame is the image itself
        save_dir = os.path.join(path, "vis_images", f"batch_{batch_idx}")
        os.makedirs(save_dir, exist_ok=True)
        for frame_idx, image in enumerate(frames):
            Image.fromarray(image).save(os.path.join(save_dir, f"frame_{frame_idx}.png"))


def save_attention_maps(maps: torch.Tensor, path: str, size: int = 256, fps: int = GIF_FPS):
    """Cross-attention heat maps as a GIF: maps [b, f, h, w] in [0, 1] (MutualAttentionBase.aggregate_cross_attn_map reshaped to its batch rows; NaN -- a
    constant map -- shows as black) -> grey frames, every map pixel a (size / h) x (size / w) block (nearest upsampling), the b maps of a frame side by
    side through the grid writer of the videos (ops.video_grid_u8), `fps` frames per second."""
    import os
    from PIL import Image
    if not torch.is_tensor(maps) or maps.dim() != 4:
        raise ValueError("save_attention_maps: expected a tensor [b, f, h, w]")
    if str(path).lower().endswith(".mp4"):
        raise ValueError(f"save_attention_maps: {path}: give a .gif path")
    b, f, h, w = maps.shape
    size, fps = int(size), int(fps)
    if size < max(h, w) or fps <= 0:
        raise ValueError(f"save_attention_maps: size must be at least the map's {max(h, w)} pixels and fps positive, got size {size}, fps {fps}")
    m = maps.detach().float().nan_to_num(0.0).clamp(0.0, 1.0)
    iy = (torch.arange(size, device=m.device) * h) // size          # nearest: output pixel y shows map row floor(y h / size)
    ix = (torch.arange(size, device=m.device) * w) // size
    video = m[:, :, iy][:, :, :, ix][:, None].contiguous()          # [b, 1, f, size, size]
    frames = videos_to_grid_frames(video).numpy()
    if os.path.dirname(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    ims = [Image.fromarray(fr) for fr in frames]
    ims[0].save(path, format="GIF", save_all=True, append_images=ims[1:], loop=0, duration=max(1000 // fps, 1))
    return path
