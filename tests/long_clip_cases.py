"""TEST INFRASTRUCTURE: the cases of the long-clip tests (tests/test_long_clip_cpu.py, tests/test_long_clip_gpu.py): me_tattn above 64 frames, where the
key-tiled kernel tattn_long_kernel<dh> (csrc/tattn.hip) walks the keys in stages of 64 under an online softmax, one block per 64 query frames.

Built on tests/fwd_cases.py (Case, the temporal_attention builder, BOUNDS) and run by tests/fwd_run.py: a case here is a fwd_cases case of entry
"temporal_attention" with one more parameter, `kind`:
  soft     the inputs of fwd_cases.build: N(0, 0.7) everywhere, a flat softmax;
  rising   a unit direction u per head, 4 u added to every query and + 0.25 j / (4 scale) u to the key of frame j: the score of key j moves by + 0.25 j,
           so the running maximum of a query changes in EVERY stage it sees (a missing or doubled rescale, or a stage weighted by a stale maximum, is a
           gross error here and a small one on the soft inputs);
  falling  the same with - 0.25 j: the first stage holds the maximum and every later stage arrives far below it.
tattn_target restates the extended dispatch of me_tattn (fwd_cases.tattn_target stops at 64 frames and stays as it is)."""
from __future__ import annotations

from typing import Optional

import torch

import fwd_cases as fc
from bwd_cases import Case, seed_of

STAGE = 64                                       # keys per stage and queries per block of tattn_long_kernel
MAX_FRAMES = 256                                 # csrc/tattn.hip LONG_MAX_FRAMES
LONG_DH = (40, 80, 160)
# 65: one key in the second stage, one query in the second block; 128 | 129: the third stage appears with one key; 256: the limit
FRAME_EDGES = (65, 72, 128, 129, 136, 200, 256)
KINDS = ("soft", "rising", "falling")
STEP = 0.25                                      # score per frame of the rising / falling inputs
LONG_TARGETS = [f"tattn_long_kernel<{dh}>" for dh in LONG_DH]
REFUSED_FRAMES = dict(frames=MAX_FRAMES + 1, dh=40, heads=8, npix=1, batch=1)


def tattn_target(a) -> Optional[str]:
    """csrc/tattn.hip me_tattn with the key-tiled kernel (whatever ME_TATTN_MFMA says above 64 frames); None: refused."""
    dh, F = a["dh"], a["frames"]
    if F > STAGE and dh in LONG_DH:
        return f"tattn_long_kernel<{dh}>" if F <= MAX_FRAMES else None
    return fc.tattn_target(a)


def geometry(p):
    """(query blocks, [stages block qb walks]) of a launch: a block ends with the stage that holds its last real query's diagonal."""
    qf, q0 = (p["q_frames"], p.get("q_frame0", 0)) if p.get("q_frames") else (p["frames"], 0)
    nqb = (qf + STAGE - 1) // STAGE
    return nqb, [(q0 + min(qb * STAGE + STAGE - 1, qf - 1)) // STAGE + 1 for qb in range(nqb)]


CASES = []


def _t(id_, **p):
    p.setdefault("npix", 3)
    p.setdefault("batch", 2)
    p.setdefault("heads", 320 // p["dh"])
    CASES.append(Case(id=f"long-{id_}", entry="temporal_attention", p=p, path=tattn_target(p), twice=True))


for _dh in LONG_DH:
    for _F in FRAME_EDGES:
        for _kind in KINDS:
            _t(f"F{_F}-dh{_dh}-{_kind}", frames=_F, dh=_dh, kind=_kind)
# the three row orders, the editor's kv_map, strided operands
_t("q-frames-inside-a-stage", frames=136, dh=40, q_frames=40, q_frame0=72)               # a query window that starts inside a stage
_t("q-frames-last-shard", frames=128, dh=80, q_frames=32, q_frame0=96, kv_parts=4)
_t("pixel-sharded", frames=96, dh=160, kv_parts=4, q_parts=4, npix=5)
_t("npix1-batch8-kv-map", frames=72, dh=40, npix=1, batch=8, kv_map=[1, 0, 3, 2, 7, 7, 0, 5])
_t("strided", frames=104, dh=80, fused=True, scale=0.2)                                  # Q, K, V column views of wider tensors, a scale of its own
# one case per row order for the guard-band protocol (tests/guard.py)
GUARDED = ("long-F136-dh80-soft", "long-q-frames-inside-a-stage", "long-pixel-sharded")

BY_ID = {c.id: c for c in CASES}


def build(case) -> dict:
    """fwd_cases.build, with the rising / falling direction added (plain row order: row = (b * frames + frame) * npix + pixel)."""
    t = fc.build(case)
    p = case.p
    kind = p.get("kind", "soft")
    if kind == "soft":
        return t
    assert not p.get("q_frames") and p.get("kv_parts", 1) <= 1
    heads, dh, F, npix, batch = p["heads"], p["dh"], p["frames"], p["npix"], p["batch"]
    C, scale = heads * dh, p.get("scale") or dh ** -0.5
    u = torch.randn(heads, dh, generator=torch.Generator().manual_seed(seed_of(case.id + "/direction")))
    u = u / u.norm(dim=1, keepdim=True)
    q = t["q"].float().reshape(-1, heads, dh) + 4.0 * u
    kv = t["kv"].float().clone()
    k = kv[:, :C].reshape(batch, F, npix, heads, dh)
    shift = (1.0 if kind == "rising" else -1.0) * STEP * torch.arange(F, dtype=torch.float32) / (4.0 * scale)
    kv[:, :C] = (k + shift[None, :, None, None, None] * u).reshape(-1, C)
    return dict(q=q.reshape(-1, C).half(), kv=kv.half())


def stage_maxima(case, t):
    """[batch, npix, heads, frames, stages] in fp64: the largest scaled score of query i among the keys <= i of each stage (-inf: none)."""
    p = case.p
    heads, dh, F, npix, batch = p["heads"], p["dh"], p["frames"], p["npix"], p["batch"]
    C, scale = heads * dh, p.get("scale") or dh ** -0.5
    shp = lambda x: x.double().reshape(batch, F, npix, heads, dh).permute(0, 2, 3, 1, 4)    # noqa: E731
    s = shp(t["q"]) @ shp(t["kv"][:, :C]).transpose(-1, -2) * scale
    s = s.masked_fill(torch.arange(F)[None, :] > torch.arange(F)[:, None], float("-inf"))
    n = (F + STAGE - 1) // STAGE
    s = torch.nn.functional.pad(s, (0, n * STAGE - F), value=float("-inf"))
    return s.reshape(batch, npix, heads, F, n, STAGE).max(dim=-1).values
