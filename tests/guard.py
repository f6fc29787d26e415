"""Guard-band harness: does a launch stay inside the views it was given?

Every operand of a guarded launch is a view into a larger allocation that the test owns.  Inputs lie in a surround of poison, outputs in a surround of a
recognisable bit pattern, and the launch runs three times on the SAME addresses with the input surroundings refilled with NaN, with 0 and with a large
finite value (run_guarded).  A kernel that reads past a view and lets that value reach a result -- the "masked by a zero weight" tail, 0 x NaN = NaN --
gives three different results; a kernel that writes past a view breaks the pattern behind it.  Nothing here ever hands a kernel a pointer whose legal
range ends at an allocation boundary: whatever a wrong kernel touches within one tile of a view belongs to the test.

What the harness sees: reads that CHANGE A RESULT and writes that LAND IN A GUARD.  A stray read whose value is discarded is invisible.  Guards are sized
by the caller to the largest tile of the kernel form under test (the defaults are 256 rows and 64 columns; weights get at least one BN x taps x K panel):
a stray of more than one tile beyond a view is out of reach of these tests.

Plain helpers: no fixtures, works on CPU tensors too (tests/test_guard_cpu.py runs the protocol on pure-torch stand-ins).
"""
from __future__ import annotations

import math
from typing import Callable, Dict, Iterable, Optional, Sequence

import torch

# The defaults of check() in tests/test_kernels_gpu.py (fp16 storage, fp32 accumulation).  Restated, not chosen here.
REL_L2 = 2e-3
MAX_REL = 2e-2

NAN, ZERO, BIG = float("nan"), 0.0, 6.0e4      # the three surroundings of the protocol (6.0e4: finite in fp16, survives a max, overflows a sum)
PHASES = (("nan", NAN), ("zero", ZERO), ("big", BIG))
INT_POISON = (0, 1, 2)                          # integer tables hold INDICES: their surroundings change with the phase but stay indices a kernel may follow inside the test's memory
SENTINEL = {torch.float16: 0x7E5A, torch.float32: 0x7FC5A5A5, torch.float64: 0x7FF85A5A5A5A5A5A, torch.int32: 0x5A5A5A5A, torch.uint8: 0x5A}   # NaNs with a payload / a fixed integer
_BITS = {torch.float16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64, torch.int32: torch.int32, torch.uint8: torch.uint8, torch.int64: torch.int64}
ROW_GUARD, COL_GUARD = 256, 64


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.float16)


def errs(got, want):
    got, want = got.detach().float().cpu().double(), want.detach().float().cpu().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert torch.isfinite(got).all()
    return float((got - want).norm() / want.norm().clamp_min(1e-30)), float((got - want).abs().max() / want.abs().mean().clamp_min(1e-30))


def check(got, want, name=""):
    """check() of tests/test_kernels_gpu.py at its default bounds; prints the figures before it asserts."""
    r, m = errs(got, want)
    print(f"{name}: rel-L2 {r:.3e}, max/mean {m:.3e}")
    assert r <= REL_L2 and m <= MAX_REL, f"{name}: rel-L2 {r:.3e} (<= {REL_L2}), max/mean {m:.3e} (<= {MAX_REL})"


def bits(t: torch.Tensor) -> torch.Tensor:
    """The raw bits of t as integers of the same width (bitwise comparisons: NaN == NaN, +0 != -0)."""
    return t.view(_BITS[t.dtype])


def _signed(pattern: int, dtype) -> int:
    n = torch.empty(0, dtype=_BITS[dtype]).element_size() * 8
    return pattern - (1 << n) if dtype != torch.uint8 and pattern >= 1 << (n - 1) else pattern


class Guard:
    """One operand: `view` (what the launch is given) inside the flat allocation `buf`."""

    def __init__(self, buf: torch.Tensor, view: torch.Tensor, name: str = ""):
        self.buf, self.view, self.name = buf, view, name
        self.offset = view.storage_offset() - buf.storage_offset()
        self.inside = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
        self.inside.as_strided(view.shape, view.stride(), self.offset).fill_(True)
        self.int_poison = INT_POISON
        self.sentinel = None

    def refill(self, poison) -> None:
        """The surroundings become `poison`; the values of the view stay."""
        keep = self.view.clone()
        self.buf.fill_(poison)
        self.view.copy_(keep)

    def where(self, flat: int) -> str:
        """A flat element of the allocation as (row, column) relative to the view (2-D views; the rows of the guard above the view are negative)."""
        rel = flat - self.offset
        if self.view.dim() == 2:
            ld = self.view.stride(0)
            r, c = rel // ld, rel % ld
            if c >= ld - self.offset % ld:        # a guard column left of the next row
                r, c = r + 1, c - ld
            return f"(row {r}, column {c}) relative to the view"
        return f"element {rel} relative to the view's first"

    def outside_intact(self, expect: torch.Tensor, what: str) -> None:
        """expect: the bits every element outside the view must hold (a 0-d tensor, or a snapshot of the whole allocation)."""
        bad = (bits(self.buf) != expect) & ~self.inside
        if bool(bad.any()):
            raise AssertionError(f"guard: {what} '{self.name}': {int(bad.sum())} elements outside the view were written, the first at {self.where(int(torch.nonzero(bad)[0]))}")


def _layout(shape, dtype, row_guard, col_guard, contiguous):
    """(allocation elements, offset, strides) of a view of `shape` with its guards."""
    es = torch.empty(0, dtype=dtype).element_size()
    v32 = 32 // es
    up = lambda n: (n + v32 - 1) // v32 * v32      # noqa: E731
    odd = lambda n: up(n) + v32 // 2               # noqa: E731  -- a multiple of 16 bytes that is not one of 32
    if len(shape) == 2 and not contiguous:
        rows, cols = shape
        left = odd(col_guard)
        ld = up(left + cols + col_guard)           # row pitch a multiple of 32 bytes: EVERY row of the view starts 16-, not 32-byte aligned
        return (rows + 2 * row_guard) * ld, row_guard * ld + left, (ld, 1)
    if len(shape) == 3 and not contiguous:         # head-major panels [heads, rows, dh]: strides (head, row, 1), guard rows between the heads
        heads, rows, dh = shape
        g = odd(row_guard * dh)
        hs = up(rows * dh + g)
        return g + heads * hs + g, g, (hs, dh, 1)
    g = odd(max(row_guard, 1) * max(col_guard, 1))
    return g + int(math.prod(shape)) + g, g, tuple(torch.empty(shape, device="meta").stride())


def _alloc(shape, dtype, device, row_guard, col_guard, contiguous, name) -> Guard:
    shape = tuple(shape)
    n, off, strides = _layout(shape, dtype, row_guard, col_guard, contiguous)
    buf = torch.empty(n, dtype=dtype, device=device)
    g = Guard(buf, buf.as_strided(shape, strides, off), name)
    if buf.is_cuda:      # the least alignment the ABI promises to accept, and not the start of an allocation
        assert g.view.data_ptr() % 16 == 0 and g.view.data_ptr() % 32 != 0 and g.view.data_ptr() != buf.data_ptr()
    g.view.guard = g
    return g


def embed_in(t: torch.Tensor, poison=NAN, *, row_guard: int = ROW_GUARD, col_guard: int = COL_GUARD, device=None, name: str = "", contiguous: bool = False,
             int_poison: Sequence[int] = INT_POISON) -> torch.Tensor:
    """A view with the values of `t` inside a larger allocation filled with `poison`, on `device` (default: t's).  2-D tensors get guard rows above and below
    and guard columns left and right (leading dimension > width); contiguous=True (weights [N, taps, K], vectors, tables, flat buckets: what the ABI wants
    contiguous) and every other rank get row_guard x col_guard guard elements before and after; 3-D tensors are head-major panels with strides (head, row, 1)
    and guard rows between the heads.  The view's address is 16-byte but not 32-byte aligned.  It carries its Guard as `.guard`."""
    g = _alloc(t.shape, t.dtype, t.device if device is None else device, row_guard, col_guard, contiguous or t.dim() not in (2, 3), name)
    g.int_poison = tuple(int_poison)
    g.buf.fill_(poison if t.dtype.is_floating_point else g.int_poison[0])
    g.view.copy_(t)
    return g.view


def sentinel_out(shape, dtype=torch.float16, *, device="cuda", row_guard: int = ROW_GUARD, col_guard: int = COL_GUARD, name: str = "", contiguous: bool = False):
    """(view, intact): an output view inside a larger allocation in which every element -- the view included -- holds SENTINEL[dtype]; intact() asserts by raw
    bits that everything outside the view still does and names the first offending (row, column) relative to the view."""
    g = _alloc(shape, dtype, device, row_guard, col_guard, contiguous or len(tuple(shape)) not in (2, 3), name)
    g.sentinel = torch.tensor(_signed(SENTINEL[dtype], dtype), dtype=_BITS[dtype], device=g.buf.device)
    bits(g.buf).fill_(int(g.sentinel))
    return g.view, lambda: g.outside_intact(g.sentinel, "output")


def _guards(ts) -> Dict[str, Guard]:
    if ts is None:
        return {}
    if not isinstance(ts, dict):
        ts = {f"#{i}": t for i, t in enumerate(ts)}
    out = {}
    for k, t in ts.items():
        if t is None:
            continue
        g = getattr(t, "guard", None)
        assert isinstance(g, Guard), f"guard: operand '{k}' was not made by embed_in / sentinel_out"
        g.name = g.name or k
        out[k] = g
    return out


def _sync(guards: Iterable[Guard]) -> None:
    if any(g.buf.is_cuda for g in guards):
        torch.cuda.synchronize()


def run_guarded(launch: Callable[[], None], inputs, outputs, inout=(), *, before: Optional[Callable[[], None]] = None):
    """The protocol.  `inputs`: views from embed_in (dict name -> view, or a sequence); `outputs`: views from sentinel_out; `inout`: names of INPUTS that the
    launch accumulates into or updates in place -- they are restored to the same bits before every launch, their view counts as a result and only their
    surroundings must stay unchanged.  `before()` runs ahead of every launch (the stale-scratch cases poison the scratch there).

    Three launches, identical in every argument, with the input surroundings NaN / 0 / 6e4.  Asserted: (1) the three results are finite and bitwise equal;
    (2) after each launch every element outside every output view still holds the sentinel; (3) every input allocation, surroundings included, is bitwise
    unchanged (in-out operands: their surroundings).  Returns the results of the NaN launch, name -> tensor (clones of the views)."""
    ins, outs = _guards(inputs), _guards(outputs)
    inout = set(inout)
    assert inout <= set(ins), f"guard: in-out operands {sorted(inout - set(ins))} are not among the inputs"
    assert not (set(ins) & set(outs)), "guard: an operand is either an input or an output"
    assert all(g.sentinel is not None for g in outs.values()), "guard: outputs come from sentinel_out"
    every = list(ins.values()) + list(outs.values())
    start = {k: ins[k].view.clone() for k in inout}
    results = []
    for pi, (phase, poison) in enumerate(PHASES):
        for k, g in ins.items():
            if k in inout:
                g.view.copy_(start[k])
            g.refill(poison if g.buf.dtype.is_floating_point else g.int_poison[pi])
        for g in outs.values():
            bits(g.buf).fill_(int(g.sentinel))
        snap = {k: bits(g.buf).clone() for k, g in ins.items()}
        if before is not None:
            before()
        _sync(every)
        launch()
        _sync(every)
        for g in outs.values():
            g.outside_intact(g.sentinel, f"[{phase} surroundings] output")
        for k, g in ins.items():
            if k in inout:
                g.outside_intact(snap[k], f"[{phase} surroundings] in-out operand")
            elif not torch.equal(bits(g.buf), snap[k]):
                bad = torch.nonzero(bits(g.buf) != snap[k])
                raise AssertionError(f"guard: [{phase} surroundings] input '{g.name}' was modified by the launch: {bad.numel()} elements, the first at {g.where(int(bad[0]))}")
        res = {k: g.view.clone() for k, g in outs.items()}
        res.update({k: ins[k].view.clone() for k in inout})
        results.append(res)
    r_nan = results[0]
    for (phase, _), res in zip(PHASES, results):
        for k, t in res.items():
            if t.dtype.is_floating_point and not bool(torch.isfinite(t).all()):
                bad = torch.nonzero(~torch.isfinite(t))
                raise AssertionError(f"guard: result '{k}' is not finite with {phase} surroundings: {bad.shape[0]} elements, the first at {tuple(bad[0].tolist())}: "
                                     "bytes outside a view reached the result, or a part of the output was never written")
            if not torch.equal(bits(t), bits(r_nan[k])):
                diff = torch.nonzero(bits(t) != bits(r_nan[k]))
                raise AssertionError(f"guard: result '{k}' with {phase} surroundings differs bitwise from the result with nan surroundings in {diff.shape[0]} elements, "
                                     f"the first at {tuple(diff[0].tolist())}: bytes outside a view reached the result")
    return r_nan


def _same(a, b, what: str) -> None:
    a, b = (a if isinstance(a, dict) else {"result": a}), (b if isinstance(b, dict) else {"result": b})
    for k in a:
        if a[k].dtype.is_floating_point:
            assert bool(torch.isfinite(a[k]).all()) and bool(torch.isfinite(b[k]).all()), f"guard: '{k}' is not finite {what}: stale scratch reached the result"
        if not torch.equal(bits(a[k]), bits(b[k])):
            diff = torch.nonzero(bits(a[k]) != bits(b[k]))
            raise AssertionError(f"guard: '{k}' differs bitwise {what} in {diff.shape[0]} elements, the first at {tuple(diff[0].tolist())}: stale scratch reached the result")


def scratch_independent(run: Callable[[], object], poison: Callable[[], object], run_larger: Optional[Callable[[], object]] = None) -> None:
    """The stale-scratch protocol.  `run()` launches and returns a tensor (or a dict of tensors) that it owns.  run, poison, run: bitwise equal and finite.  With
    `run_larger` (a larger launch of the same entry point, which grows and fills the same scratch): larger, run against poison, run -- the grow-only reuse a
    step performs."""
    first = run()
    poison()
    _same(first, run(), "between a launch on the scratch it left behind and one on NaN-filled scratch")
    if run_larger is not None:
        run_larger()
        after_larger = run()
        poison()
        _same(after_larger, run(), "between a launch after a larger one and one on NaN-filled scratch")


def poison_scratch(ops=None, value: float = NAN) -> int:
    """Fill every live block of the wrappers' grow-only scratch (ops._scratch, its retired blocks, ops._gn_scratch) with NaN; returns the number of blocks."""
    if ops is None:
        from motioneditor_amd import ops
    blocks = list(ops._scratch.values()) + list(ops._scratch_retired) + list(ops._gn_scratch.values())
    for t in blocks:
        t.fill_(value)
    if any(t.is_cuda for t in blocks):
        torch.cuda.synchronize()
    return len(blocks)
