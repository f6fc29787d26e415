"""Spatial attention-editor base + registration, mirroring the reference's
``motion_editor/attn_control/fully_control_utils.py`` (MutualAttentionBase :29-70,
regiter_fully_attention_editor_diffusers :109-229).

Difference by design (MI355X-first): the reference monkey-patches ``forward`` of every
MotionFrameAttention / CrossAttention and hands the editor pre-gathered ``(B*H, n, dh)`` q/k/v
(keys already duplicated to [prev | cur]).  Here the UNet graph calls the registered editor with an
``AttnCall`` (un-gathered row views + geometry) and the editor picks a key-segment table for the
fused HIP kernel -- the gather and the masked-key duplication never exist in memory.  Counters,
gating and attributes are the reference's.
"""
from __future__ import annotations

import os

import torch

from .. import plan, segments

XATTN_KEYS = 77     # text keys of a cross-attention
XATTN_LD = 80       # row pitch of the accumulator: 320-byte rows, every row 16-byte aligned


class MutualAttentionBase:
    def __init__(self):
        self.cur_step = 0
        self.num_att_layers = -1
        self.cur_att_layer = 0
        # cross-attention maps (collect_cross_attention): off until asked for -- a step that collects nothing launches nothing more
        self._xa_on = False
        self._xa_tokens = 256
        self._xa_steps = None
        self._xa_keep = False
        self._xa_acc = None      # fp32 [B f tokens, XATTN_LD]: the SUM of the head-mean maps of every collected entry
        self._xa_items = 0       # B f of the accumulator
        self._xa_frames = 1      # f
        self._xa_count = 0       # entries summed so far (host side)

    def after_step(self):
        d = getattr(self, "mask_save_dir", None)
        if d is not None and self._xa_on and self._xa_count:
            self._save_cross_maps(d)

    # ---- cross-attention maps per prompt token (reference fully_control.py:257-277, 430-432) ---------------------------------------------
    def collect_cross_attention(self, tokens=256, step_idx=None, keep_entries=False):
        """From now on every text cross-attention with `tokens` queries per frame (256 = the reference's hard-coded 16 * 16, fully_control.py:431), in
        the steps of `step_idx` (None: every step), adds its head-mean probability map into ONE device accumulator fp32 [B f, tokens, 80] (columns
        0 .. 76 are the text tokens): one more kernel launch per such layer (ops.attention_probs, beta = 1), nothing else changes.  Rows are the
        reference's "(b f)" order over the full batch.  keep_entries additionally appends every entry [B f, tokens, 77] to `self.cross_attns`, the
        reference's list -- eager steps only (a replayed step runs no Python per layer)."""
        if self._xa_acc is not None and tokens != self._xa_tokens:
            raise ValueError(f"collect_cross_attention: the accumulator holds maps of {self._xa_tokens} tokens; a new size needs a new editor")
        self._xa_on, self._xa_tokens, self._xa_keep = True, int(tokens), bool(keep_entries)
        if keep_entries and not hasattr(self, "cross_attns"):
            self.cross_attns = []
        self._xa_steps = None if step_idx is None else frozenset(int(s) for s in step_idx)

    def stop_collecting(self):
        """Collection off; what was collected stays readable."""
        self._xa_on = False

    def reset_cross_attention(self):
        """Zero the accumulator in place (it keeps its address: recorded steps point at it) and the entry count."""
        if self._xa_acc is not None:
            self._xa_acc.zero_()
        self._xa_count = 0
        if self._xa_keep:
            self.cross_attns = []

    def collects_in_step(self, step=None) -> bool:
        """Will the step `step` (default: the coming one) collect?  Part of the executors' plan key: a step recorded without the probe launches is
        never replayed for a collecting step, nor the reverse."""
        step = self.cur_step if step is None else step
        return self._xa_on and (self._xa_steps is None or step in self._xa_steps)

    def cross_attention_state(self):
        """(a copy of the accumulator or None, the count): what a step computed more than once must put back (denoise_step_planned)."""
        return (None if self._xa_acc is None else self._xa_acc.clone(), self._xa_count, len(getattr(self, "cross_attns", ())))

    def restore_cross_attention(self, state):
        acc, count, n_kept = state
        if self._xa_acc is not None:
            if acc is None:
                self._xa_acc.zero_()
            else:
                self._xa_acc.copy_(acc)
        self._xa_count = count
        if self._xa_keep:
            del self.cross_attns[n_kept:]

    def _probe(self, call, seg_item):
        if call.N != self._xa_tokens or not self.collects_in_step():
            return
        if call.nk != XATTN_KEYS:
            raise ValueError(f"cross-attention maps: {XATTN_KEYS} text keys expected, the call has {call.nk}")
        items = call.B * call.f
        if self._xa_acc is None:
            plan.torch_fallback("allocating the cross-attention accumulator")      # (never reached: a recording pass follows a warm-up of the same step)
            self._xa_acc = torch.zeros((items * call.N, XATTN_LD), dtype=torch.float32, device=call.q.device)
            self._xa_items, self._xa_frames = items, call.f
        elif self._xa_items != items or self._xa_acc.device != call.q.device:
            raise ValueError(f"cross-attention maps: the accumulator holds {self._xa_items} (batch, frame) items, this call has {items}: "
                             "reset needs a new editor when the batch or the clip changes")
        call.probs(seg_item, self._xa_acc, 1.0)
        self._xa_count += 1
        if self._xa_keep:
            if plan.ACTIVE is not None:
                raise ValueError("collect_cross_attention(keep_entries=True) is for the eager executor only: a planned step replays launches, not the "
                                 "Python that appends to cross_attns")
            entry = torch.empty((items * call.N, XATTN_LD), dtype=torch.float32, device=call.q.device)
            call.probs(seg_item, entry, 0.0)
            self.cross_attns.append(entry[:, :XATTN_KEYS].reshape(items, call.N, XATTN_KEYS))

    def cross_attention_mean(self):
        """[B f, tokens, 77] fp32: the mean over the collected entries = torch.stack(self.cross_attns, 1).mean(1) of the reference."""
        if self._xa_acc is None or self._xa_count == 0:
            raise ValueError("no cross-attention map collected: collect_cross_attention() first, then run steps that reach layers of that token count")
        return self._xa_acc[:, :XATTN_KEYS].reshape(self._xa_items, self._xa_tokens, XATTN_KEYS) * (1.0 / self._xa_count)

    def aggregate_cross_attn_map(self, idx):
        """Reference fully_control.py:257-268: [B f, res, res] maps of token `idx` (a list: the sum over its tokens), each min-max normalised over its
        own pixels.  As there, a constant map (max == min) divides by zero and comes back NaN."""
        attn_map = self.cross_attention_mean()
        res = int(round(attn_map.shape[-2] ** 0.5))
        attn_map = attn_map.reshape(-1, res, res, attn_map.shape[-1])
        image = attn_map[..., idx]
        if isinstance(idx, list):
            image = image.sum(-1)
        image_min = image.min(dim=1, keepdim=True)[0].min(dim=2, keepdim=True)[0]
        image_max = image.max(dim=1, keepdim=True)[0].max(dim=2, keepdim=True)[0]
        return (image - image_min) / (image_max - image_min)

    def edit_rows(self):
        """The "(b f)" rows of the accumulator that belong to edit branches: each classifier-free-guidance half of the batch is [rec, e_1 .. e_N]."""
        f = self._xa_frames
        B = self._xa_items // f
        half = B // 2 if B >= 4 else B
        return [b * f + i for b in range(B) if b % half for i in range(f)]

    def _save_cross_maps(self, d):
        """mask_save_dir: the maps of cur_token_idx on the edit rows, one PNG per row, after every step (the mean so far)."""
        import numpy as np
        import PIL.Image
        maps = self.aggregate_cross_attn_map(list(getattr(self, "cur_token_idx", [1])))[self.edit_rows()]
        arr = (maps.nan_to_num(0.0).clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy()
        for r, im in zip(self.edit_rows(), arr):
            PIL.Image.fromarray(np.ascontiguousarray(im), mode="L").save(os.path.join(d, f"cross_attn_step{self.cur_step:03d}_row{r:03d}.png"))

    def __call__(self, q=None, k=None, v=None, sim=None, attn=None, is_cross=None, place_in_unet=None, num_heads=None,
                 attention_mask=None, **kwargs):
        out = self.forward(q=q, k=k, v=v, is_cross=is_cross, place_in_unet=place_in_unet, num_heads=num_heads,
                           attention_mask=attention_mask, sim=sim, attn=attn, **kwargs)
        self.cur_att_layer += 1
        if self.cur_att_layer == self.num_att_layers:
            self.cur_att_layer = 0
            self.cur_step += 1
            self.after_step()
        return out

    def forward(self, q=None, k=None, v=None, sim=None, attn=None, is_cross=None, place_in_unet=None, num_heads=None,
                attention_mask=None, call=None, text_seg=None, **kwargs):
        """Un-edited attention (reference :48-66): self = [prev | cur] frame keys, cross = text keys."""
        if call is None:
            raise ValueError("motioneditor_amd editors are driven by the UNet graph with call=AttnCall(...)")
        if is_cross:
            out = call.run(*text_seg)
            if self._xa_on:
                self._probe(call, text_seg[0])
            return out
        return call.run(*segments.prev_cur(call.B, call.f, call.q.device, getattr(call, "shard", None)))

    def edits_next_self_attention(self) -> bool:
        """Will the NEXT self-attention call be edited (K/V injection)?  The UNet graph asks before it shares the classifier-free-guidance
        prefix between batch entries (an edited layer needs the full (recon, edit) x (uncond, cond) batch).  The base class never edits."""
        return False

    def reset(self):
        self.cur_step = 0
        self.cur_att_layer = 0


def regiter_fully_attention_editor_diffusers(model, editor: MutualAttentionBase):
    """Register `editor` on ``model.unet`` (reference :109-229).  The reference counts the patched
    MotionFrameAttention + CrossAttention modules under down/mid/up: 16 transformer blocks x {attn1, attn2}."""
    unet = model.unet
    unet.spatial_editor = editor
    editor.num_att_layers = unet.num_spatial_attention_layers
    return editor
