"""TEST INFRASTRUCTURE: the cases of the long-clip backward tests (tests/test_long_bwd_cpu.py, tests/test_long_bwd_gpu.py, tests/test_guard_long_bwd_gpu.py):
ops.temporal_attention_bwd above 64 frames, where me_tattn_bwd_long (include/motioned_long.h, csrc/tattn_bwd_long.hip) rebuilds the softmax statistics in a
query-centric kernel (sweep 1: online lse / delta over key stages; sweep 2: dQ) and reads them in a key-centric kernel (dK, dV).

A case is a tests/bwd_cases.py Case of entry "temporal_attention_bwd", run by tests/bwd_run.py and held to that entry point's own bound against
tests/ref64_bwd.py.  Its q / k come from tests/long_clip_cases.py (`kind`: soft, rising, falling -- the running maximum changes in every stage, or never),
v ~ N(0, 0.7), dout ~ N(0, 1).  `zero_block`: the dout rows of frames 0 .. 63 are zero ONCE ROUNDED TO FP16, the value the matrix units multiply -- odd frames
hold 0.0, even frames N(0, 1) clamped to +-3.9, times 2^-27 (below half of fp16's smallest subnormal, 2^-25) -- so dP, delta and dS of those queries are exactly zero and so must their dQ
rows be; a delta summed from the unrounded dout is not zero there (query 0 has P = 1, dS = -delta = -2^-27 v.n rounds to a non-zero fp16 subnormal).

`emulate` is the fp32 emulation of the kernels AS BUILT: dout rounded to fp16, fp32 scores, the stage-wise online maximum / sum / delta of sweep 1 (stages
of 64 keys, 32 at dh 160), P = 2^(s c - lse) and dS = P (dP - delta) rounded to fp16, fp32 accumulation; its keyword flags are the deliberately wrong
variants of tests/test_long_bwd_cpu.py.

Bounds.  The entry point's bound, bwd_cases.BOUNDS["temporal_attention_bwd"] = (2e-3 rel-L2, 2e-2 max / mean), holds for every case whose emulation fits it.
The fp16 P / dS / dout operands do not fit it everywhere: on the falling inputs key 0 collects the mass of every query, so dK / dV of frame 0 are sums of up to
256 fp16-rounded terms measured against a mean dominated by small rows (max / mean up to 1.5e-1 at 256 frames); on the rising inputs K carries a component of
up to 100 along one direction that cancels in dQ = scale dS K only as exactly as dS is rounded (rel-L2 up to 2.6e-3, max / mean up to 1.3e-1).  Those cases
follow the `bound=` protocol of tests/bwd_cases.py: FLOORS holds the error of `emulate` against the fp64 reference measured on a CPU (the larger of dq, dk,
dv per figure), FACTOR = 4, and the case's bound is per figure the larger of the entry point's and FACTOR x floor; floor, factor and bound stand in the
case entry (p["floor"], p["factor"], Case.bound).  No figure comes from what the kernels returned; tests/test_long_bwd_cpu.py re-measures every floor."""
from __future__ import annotations

import math

import torch

import long_clip_cases as lc
from bwd_cases import BOUNDS, Case, seed_of

MIN_FRAMES, MAX_FRAMES = 65, 256                 # csrc/tattn_bwd_long.hip
BLK = 64                                         # query frames per block of the dq kernel, key frames per block of the dkv kernel
QSTAGE = 32                                      # queries per stage of the dkv kernel
LONG_DH = lc.LONG_DH
FRAME_EDGES = lc.FRAME_EDGES                     # 65: one query in the second block, one key in the second stage; 128 | 129; 256: the limit
KINDS = lc.KINDS
LOG2E = 1.4426950408889634


def key_stage(dh: int) -> int:
    """Keys per stage of tattn_bwd_long_dq_kernel<dh, KT>."""
    return 32 if dh > 80 else 64


def target(p) -> str:
    """me_last_kernel after ops.temporal_attention_bwd: csrc/bwd.hip's kernels up to 64 frames (bwd_cases.tattn_bwd_path), the pair of key-tiled kernels above."""
    from bwd_cases import tattn_bwd_path
    if p["frames"] <= 64:
        return tattn_bwd_path(p["frames"], p["dh"], p["heads"])
    return f"tattn_bwd_long_dq_kernel<{p['dh']}>+tattn_bwd_long_dkv_kernel<{p['dh']}>"


def work_bytes(batch: int, frames: int, npix: int, heads: int) -> int:
    """me_tattn_bwd_long_work_bytes, restated: lse and delta, one fp32 each per (row, head)."""
    return 0 if min(batch, frames, npix, heads) <= 0 else 8 * batch * frames * npix * heads


FACTOR = 4
# case id -> (rel-L2, max / mean) of `emulate` against tests/ref64_bwd.py, for the cases whose emulation leaves the entry point's bound in either figure
FLOORS = {
    "lbwd-F65-dh40-falling": (3.00e-04, 2.82e-02),
    "lbwd-F72-dh40-rising": (7.68e-04, 2.88e-02),
    "lbwd-F72-dh40-falling": (2.95e-04, 3.61e-02),
    "lbwd-F128-dh40-rising": (1.33e-03, 3.06e-02),
    "lbwd-F128-dh40-falling": (2.95e-04, 4.73e-02),
    "lbwd-F129-dh40-rising": (1.31e-03, 3.71e-02),
    "lbwd-F129-dh40-falling": (3.01e-04, 6.35e-02),
    "lbwd-F136-dh40-rising": (1.36e-03, 3.39e-02),
    "lbwd-F136-dh40-falling": (2.98e-04, 6.52e-02),
    "lbwd-F200-dh40-rising": (2.02e-03, 5.50e-02),
    "lbwd-F200-dh40-falling": (2.95e-04, 7.75e-02),
    "lbwd-F256-dh40-soft": (2.91e-04, 2.10e-02),
    "lbwd-F256-dh40-rising": (2.60e-03, 8.16e-02),
    "lbwd-F256-dh40-falling": (3.12e-04, 1.47e-01),
    "lbwd-F65-dh80-falling": (2.97e-04, 2.71e-02),
    "lbwd-F72-dh80-rising": (7.62e-04, 2.07e-02),
    "lbwd-F72-dh80-falling": (2.98e-04, 3.02e-02),
    "lbwd-F128-dh80-rising": (1.26e-03, 3.78e-02),
    "lbwd-F128-dh80-falling": (3.01e-04, 5.25e-02),
    "lbwd-F129-dh80-rising": (1.32e-03, 3.61e-02),
    "lbwd-F129-dh80-falling": (2.95e-04, 5.18e-02),
    "lbwd-F136-dh80-rising": (1.37e-03, 6.04e-02),
    "lbwd-F136-dh80-falling": (2.99e-04, 4.25e-02),
    "lbwd-F200-dh80-rising": (2.03e-03, 5.79e-02),
    "lbwd-F200-dh80-falling": (2.95e-04, 7.85e-02),
    "lbwd-F256-dh80-soft": (2.98e-04, 2.02e-02),
    "lbwd-F256-dh80-rising": (2.60e-03, 1.30e-01),
    "lbwd-F256-dh80-falling": (3.15e-04, 9.03e-02),
    "lbwd-F65-dh160-falling": (2.93e-04, 2.15e-02),
    "lbwd-F72-dh160-falling": (2.96e-04, 2.47e-02),
    "lbwd-F128-dh160-rising": (1.27e-03, 2.87e-02),
    "lbwd-F128-dh160-falling": (2.90e-04, 4.24e-02),
    "lbwd-F129-dh160-rising": (1.33e-03, 3.39e-02),
    "lbwd-F129-dh160-falling": (2.90e-04, 4.11e-02),
    "lbwd-F136-dh160-rising": (1.38e-03, 3.87e-02),
    "lbwd-F136-dh160-falling": (3.01e-04, 4.14e-02),
    "lbwd-F200-dh160-rising": (2.04e-03, 5.30e-02),
    "lbwd-F200-dh160-falling": (3.03e-04, 6.16e-02),
    "lbwd-F256-dh160-rising": (2.58e-03, 7.52e-02),
    "lbwd-F256-dh160-falling": (3.06e-04, 8.20e-02),
}

CASES = []


def _t(id_, **p):
    p.setdefault("npix", 3)
    p.setdefault("batch", 2)
    p.setdefault("heads", 320 // p["dh"])
    p.setdefault("kind", "soft")
    bound = None
    if f"lbwd-{id_}" in FLOORS:
        p["floor"], p["factor"] = FLOORS[f"lbwd-{id_}"], FACTOR
        bound = (max(BOUNDS["temporal_attention_bwd"][0], FACTOR * p["floor"][0]), max(BOUNDS["temporal_attention_bwd"][1], FACTOR * p["floor"][1]))
    CASES.append(Case(id=f"lbwd-{id_}", entry="temporal_attention_bwd", p=p, path=target(p), twice=True, bound=bound))


for _dh in LONG_DH:
    for _F in FRAME_EDGES:
        for _kind in KINDS:
            _t(f"F{_F}-dh{_dh}-{_kind}", frames=_F, dh=_dh, kind=_kind)
_t("fused-qkv-dout-padded", frames=104, dh=80, fused=True, do_pad=12)                     # q | k | v column views of one [rows, 3C] tensor, dout stride C + 12
_t("scale", frames=72, dh=160, scale=0.2, kind="rising")
_t("npix1", frames=136, dh=40, npix=1)
_t("heads-twice-the-slice", frames=72, dh=80, heads=8, batch=1)                           # 640 columns: two 320-column groups of the forward
_t("zero-block", frames=136, dh=40, zero_block=True)
for _dh in LONG_DH:
    _t(f"zero-block-dh{_dh}-F72", frames=72, dh=_dh, zero_block=True, batch=1, npix=2)
GUARDED = ("lbwd-F72-dh40-soft", "lbwd-F136-dh80-rising", "lbwd-F129-dh160-soft")        # one per head size for tests/test_guard_long_bwd_gpu.py

BY_ID = {c.id: c for c in CASES}


def build(case) -> dict:
    """dict(qkv fp16 [rows, 3C], dout fp32 [rows, C]): what bwd_run.run takes for this entry."""
    p = case.p
    C, rows = p["heads"] * p["dh"], p["batch"] * p["frames"] * p["npix"]
    fwd = Case(id=case.id, entry="temporal_attention", p={k: p[k] for k in ("frames", "dh", "heads", "npix", "batch", "kind", "scale") if k in p})
    t = lc.build(fwd)
    g = torch.Generator().manual_seed(seed_of(case.id + "/dout"))
    dout = torch.randn(rows, C, generator=g)
    if p.get("zero_block"):
        d = dout.reshape(p["batch"], p["frames"], p["npix"], C)
        d[:, 0:BLK:2] = d[:, 0:BLK:2].clamp(-3.9, 3.9) * 2.0 ** -27                          # |x| < 2^-25: rounds to 0.0 in fp16
        d[:, 1:BLK:2] = 0.0
        assert float(d[:, :BLK].half().abs().max()) == 0.0 and float(d[:, 0].abs().max()) > 0.0
    return dict(qkv=torch.cat([t["q"], t["kv"]], dim=1).contiguous(), dout=dout)


def zeroed_rows(p) -> torch.Tensor:
    """The rows of the frames whose dout is zero once rounded to fp16 (zero_block)."""
    r = torch.arange(p["batch"] * p["frames"] * p["npix"]).reshape(p["batch"], p["frames"], p["npix"])
    return r[:, :BLK].reshape(-1)


def emulate(q, k, v, dout, *, heads, dh, batch, frames, npix, scale=None, delta_no_rescale=False, stale_max=False, mask_shift=0, skip_first_query_stage=False,
            delta_unrounded=False):
    """(dq, dk, dv) fp32 as the two kernels compute them (see the module docstring); the flags are the mutants."""
    F, KT = frames, key_stage(dh)
    scale = dh ** -0.5 if scale is None else scale
    c = float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))
    sc32 = float(torch.tensor(scale, dtype=torch.float32))
    shp = lambda x: x.float().reshape(batch, F, npix, heads, dh).permute(0, 2, 3, 1, 4)    # noqa: E731  [b, p, h, frame, d]
    qf, kf, vf = shp(q), shp(k), shp(v)
    do16, do32 = shp(dout.half()), shp(dout)
    i = torch.arange(F)
    allowed = i[None, :] <= i[:, None] + mask_shift                                         # [query, key]
    s = torch.where(allowed, (qf @ kf.transpose(-1, -2)) * c, torch.tensor(-1.0e30))
    dp = do16 @ vf.transpose(-1, -2)
    dp_delta = do32 @ vf.transpose(-1, -2) if delta_unrounded else dp
    # sweep 1: stages beyond a query's diagonal are all-masked (maximum unchanged, alpha = 1, every term 0): walking them changes nothing
    m = torch.full(s.shape[:-1] + (1,), -1.0e30)
    l, dl, m_first = torch.zeros_like(m), torch.zeros_like(m), None
    for k0 in range(0, F, KT):
        blk = s[..., k0:k0 + KT]
        mx = torch.maximum(m, blk.max(dim=-1, keepdim=True).values)
        alpha = torch.exp2(m - mx)
        pv = torch.exp2(blk - mx)
        l = l * alpha + pv.sum(-1, keepdim=True)
        dl = (dl if delta_no_rescale else dl * alpha) + (pv * dp_delta[..., k0:k0 + KT]).sum(-1, keepdim=True)
        m = mx
        m_first = mx if m_first is None else m_first
    lse = (m_first if stale_max else m) + torch.log2(l)
    delta = dl / l
    # sweep 2 and the key-centric kernel: P and dS reach the matrix units as fp16
    P = torch.where(allowed, torch.exp2(s - lse), torch.tensor(0.0))
    dS16 = (P * (dp - delta)).half().float()
    P16 = P.half().float()
    dq = (dS16 @ kf) * sc32
    if skip_first_query_stage:                                                               # a key block that starts at its second 32-query stage
        first = (i[None, :] // BLK) * BLK + QSTAGE                                           # [1, key] -> first query the block of this key reads
        keep = (i[:, None] >= first).float()
        dS16, P16 = dS16 * keep, P16 * keep
    dk = (dS16.transpose(-1, -2) @ qf) * sc32
    dv = P16.transpose(-1, -2) @ do16
    back = lambda x: x.permute(0, 3, 1, 2, 4).reshape(batch * F * npix, heads * dh).contiguous()   # noqa: E731
    return back(dq), back(dk), back(dv)


class Emu:
    """A backend for bwd_run.run: the emulation above, or one of its mutants."""
    name = "long-bwd emulation"

    def __init__(self, **flags):
        self.flags = flags

    def temporal_attention_bwd(self, q, k, v, out, dout, **kw):
        assert math.isfinite(float(dout.abs().max()))
        return emulate(q, k, v, dout, **kw, **self.flags)


# ---------------------------------------------------------------------------------------------------------------- the model tests at 72 frames
MODEL_FRAMES = 72                                # two key stages, two query blocks; nine adapter chunks
GOLDEN = "long_bwd_f72.npz"                      # tests/golden/, written by tools/make_golden_long_bwd.py from oracle.ref_cpu under torch autograd
ADAPTER_FULL = ("controlnet_adapter.body.0.block2.weight", "controlnet_adapter.body.11.attn_self_temp.to_out.0.bias")    # the two full tensors of adapter_train.npz


def null_text_inputs(f: int = MODEL_FRAMES):
    """(latents [x_0, x_1], context [uncond, cond]) of the null-text test: seeded, on 8 x 8 latents."""
    g = torch.Generator().manual_seed(123)
    latents = [torch.randn(1, 4, f, 8, 8, generator=g) for _ in range(2)]
    return latents, torch.randn(2, 77, 768, generator=g) * 0.3
