"""TEST INFRASTRUCTURE: the cases of ops.attention_probs / me_attn_probs (include/motioned_probe.h) that tests/test_probe_cpu.py runs on the fp32
emulation and tests/test_probe_gpu.py on the kernel, both against the fp64 restatement of tests/ref64_probe.py on the same fp16 inputs.

Shapes: the smallest at which the kernel takes another path -- a block owns 64 queries and a wave 16 (nq 1, 15, 16, 17, 64, 65, 257: a lone query, a wave
short of one, full, one over, a full block, one over, five blocks); the keys are MFMA tiles of 16 staged up to 128 (nk 1, 16, 17, 64, 65, 77, 80, 128) and a
wave stores a row 64 keys at a time; dh 40 pads its second 32-column step in LDS; heads 1 has no next head to prefetch.

The bound of a case is a maximum absolute error (a probability is <= 1): 4 x the error of the fp32 emulation against fp64 on that case + 2e-6 (about 16
fp32 ulp at 1, for the hardware exp2 and the different summation order).  emu_error() measures the emulation once per case and process."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, Optional

import torch

SLACK = 2e-6
FACTOR = 4.0


@dataclass(frozen=True)
class Case:
    id: str
    nq: int = 65
    nk: int = 77
    dh: int = 40
    heads: int = 8
    n_items: int = 3
    n_kv: int = 2
    q_items: int = 0
    q_hm: bool = False          # head-major panels [heads, rows, dh] instead of a row tensor
    k_hm: bool = False
    ldp: Optional[int] = None   # None: nk
    beta: float = 0.0           # 0: into NaN-filled P; 1: three calls in a row into zeros
    q_std: float = 1.0
    k_std: float = 1.0
    scale: Optional[float] = None
    tags: tuple = field(default_factory=tuple)


def _sweep():
    out = []
    dhs = (40, 80, 160)
    for i, nq in enumerate((1, 15, 16, 17, 64, 65, 257)):
        out.append(Case(f"nq{nq}", nq=nq, dh=dhs[i % 3]))
    for i, nk in enumerate((1, 16, 17, 64, 65, 77, 80, 128)):
        out.append(Case(f"nk{nk}", nk=nk, nq=33, dh=dhs[(i + 1) % 3]))
    for dh in dhs:
        for heads in (8, 1):
            out.append(Case(f"dh{dh}-h{heads}", dh=dh, heads=heads, nq=48))
    out.append(Case("shared-queries", n_items=4, q_items=2, nq=40, dh=80))
    out.append(Case("shared-queries-hm", n_items=4, q_items=2, nq=40, dh=40, q_hm=True, k_hm=True))
    out.append(Case("hm-q-hm-k", q_hm=True, k_hm=True, dh=80))
    out.append(Case("row-q-hm-k", k_hm=True, dh=160, nq=20))
    out.append(Case("hm-q-row-k", q_hm=True, dh=40, nq=70))
    for ldp in (77, 80, 96):
        out.append(Case(f"ldp{ldp}", ldp=ldp, nq=17, dh=80))
    out.append(Case("ldp-odd-nk17", nk=17, ldp=17, nq=19))
    out.append(Case("beta1-three-times", beta=1.0, nq=65, ldp=80))
    out.append(Case("beta1-three-times-dh160", beta=1.0, nq=18, dh=160))
    out.append(Case("high-gain", q_std=3.0, k_std=3.0, nq=64, n_items=4, tags=("gain",)))               # logits of std ~ 9
    out.append(Case("huge-logits", dh=80, scale=2000.0, nq=64, n_items=4, tags=("huge",)))             # max |logit| > 1e4: the max subtraction decides
    return out


CASES = _sweep()
BY_ID: Dict[str, Case] = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def kv_items(c: Case) -> torch.Tensor:
    """A permuted table with repeats: item i reads text row (n_kv - 1 - i) % n_kv, so row order and kv order differ and rows are read more than once."""
    return torch.tensor([(c.n_kv - 1 - i) % c.n_kv for i in range(c.n_items)], dtype=torch.int32)


def build(c: Case):
    """The operator's arguments on the CPU: fp16 q / k in the case's layout (a row tensor is a column slice of wider rows, as the model's are)."""
    g = torch.Generator().manual_seed(sum(map(ord, c.id)))
    rows_q = (c.q_items or c.n_items) * c.nq
    q = (torch.randn(rows_q, c.heads, c.dh, generator=g) * c.q_std).to(torch.float16)
    k = (torch.randn(c.n_kv * c.nk, c.heads, c.dh, generator=g) * c.k_std).to(torch.float16)
    C = c.heads * c.dh

    def lay(t, hm):
        if hm:
            return t.permute(1, 0, 2).contiguous()
        wide = torch.full((t.shape[0], C + 16), float("nan"), dtype=torch.float16)   # ld > heads * dh: what lies behind a row is not the next row
        wide[:, 8:8 + C] = t.reshape(t.shape[0], C)
        return wide[:, 8:8 + C]
    return dict(q=lay(q, c.q_hm), k=lay(k, c.k_hm), kv_item=kv_items(c),
                kw=dict(heads=c.heads, dh=c.dh, n_items=c.n_items, nq=c.nq, nk=c.nk, q_items=c.q_items, scale=c.scale))


def to_device(t, device):
    """The layout survives the move: a row view stays a view of wider rows, panels stay panels."""
    if t.dim() == 2 and t.stride(0) != t.shape[1]:
        base = torch.empty((t.shape[0], t.stride(0)), dtype=t.dtype, device=device).fill_(float("nan"))
        off = t.storage_offset() % t.stride(0)
        v = base[:, off:off + t.shape[1]]
        v.copy_(t)
        return v
    return t.to(device)


def run(c: Case, op, t, device="cpu", out_dtype=torch.float32):
    """Runs `op` (ops.attention_probs, its emulation or the fp64 restatement) the way the case says.  Returns (the [rows, nk] result, the whole P buffer,
    the pad value): beta 0 goes into a NaN-filled P, beta 1 three times in a row into zeros; the pad columns >= nk hold 12345."""
    rows, ldp = c.n_items * c.nq, c.ldp or c.nk
    P = torch.full((rows, ldp), float("nan") if c.beta == 0 else 0.0, dtype=out_dtype, device=device)
    P[:, c.nk:] = 12345.0
    q, k, kv = to_device(t["q"], device), to_device(t["k"], device), t["kv_item"].to(device)
    for _ in range(1 if c.beta == 0 else 3):
        op(q, k, kv_item=kv, out=P, beta=c.beta, **t["kw"])
    return P[:, :c.nk].clone(), P, 12345.0


_emu_err: Dict[str, float] = {}
_ref: Dict[str, torch.Tensor] = {}


def reference(c: Case) -> torch.Tensor:
    """fp64 result of the case, computed once and shared (never modified)."""
    if c.id not in _ref:
        import ref64_probe
        _ref[c.id] = run(c, ref64_probe.attention_probs, build(c), out_dtype=torch.float64)[0]
    return _ref[c.id]


def emu_error(c: Case) -> float:
    """max |fp32 emulation - fp64| of the case, measured here on the CPU, once."""
    if c.id not in _emu_err:
        import emu_probe_ops
        got = run(c, emu_probe_ops.attention_probs, build(c))[0]
        _emu_err[c.id] = float((got.double() - reference(c)).abs().max())
    return _emu_err[c.id]


def bound(c: Case) -> float:
    return FACTOR * emu_error(c) + SLACK
