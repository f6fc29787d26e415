"""Stream-order harness: is every cross-stream access of a recorded denoising step ordered by an event?

A denoising step is ~1100 launches on two HIP streams; `plan.StepPlan` records them once, with the event records / waits stated through `plan.record_event`,
`plan.wait_event`, `plan.wait_stream`, and re-issues the list at fixed addresses.  Whether a consumer on one stream sees the finished data of a producer on the
other rests on a handful of hand-placed calls, and no comparison of OUTPUTS can see a missing one: the usual timing wins the race on every run.  This module
decides it from the launch list, without timing and without a tolerance:

  * Trace -- while a step runs (recording into a plan, or eagerly, or on tests/emu_ops.py on the CPU) every launching function of the ops module and the four
    helpers of `plan` are wrapped; each op is logged with its stream, its call site, the views it reads and writes (TABLE: one entry per ops function; operands
    that never appear as arguments -- ops.STEP_PARAMS, the cached GroupNorm statistics, `_work` scratch, the per-call `vsum` of attention, the item order of a
    segment table -- enter through the accessor they come from) and the range of plan nodes it produced (me_plan_info before and after the call).
  * analyse -- vector-clock happens-before over the plan's own node list: stream order, and a WAIT orders everything before the latest preceding RECORD of its
    event (issue order: what hipStreamWaitEvent does on replay) before everything after the wait on its own stream.  Every two accesses to a common byte of which
    one is a write must be ordered; overlap is exact at element granularity (the column halves of a concat buffer are neighbours, not a conflict) and keyed on
    the ADDRESS (a pool block freed and handed out again within the pass is covered).  The prologue and epilogue of me_denoise_step (copies into the bound
    latents / text, plan_params_kernel, copy out) are nodes of the main stream.  replays=2 repeats the node list -- same addresses, events re-recorded -- so
    that step N on the side stream meets step N + 1 on the main stream.

Nothing here launches anything of its own and no racy sequence is ever executed: the mutations of tests/test_streamcheck_gpu.py edit the LOG.
No report is ever suppressed by a list of exceptions: a report is a hazard (fixed in the product) or an error of TABLE / the model (corrected, with a comment).

Plain helpers: no fixtures; works without a GPU (tests/test_streamcheck_cpu.py).
"""
from __future__ import annotations

import ctypes as C
import inspect
import linecache
import os
import sys
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

LAUNCH, RECORD, WAIT, NOP = 0, 1, 2, 3      # node kinds (0..2 = capi.PLAN_LAUNCH / PLAN_RECORD / PLAN_WAIT; NOP: a node deleted by a log mutation)
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


# ---------------------------------------------------------------------------------------------------------------------
# views
# ---------------------------------------------------------------------------------------------------------------------
class View:
    """One operand as the kernel sees it: storage address, byte offset, shape, byte strides, element size (`alloc`: the storage's (address, bytes))."""
    __slots__ = ("base", "offset", "shape", "strides", "esize", "name", "alloc", "_runs")

    def __init__(self, base: int, offset: int, shape: Sequence[int], strides: Sequence[int], esize: int, name: str = "", alloc: Optional[Tuple[int, int]] = None):
        self.base, self.offset, self.shape, self.strides, self.esize, self.name = int(base), int(offset), tuple(shape), tuple(strides), int(esize), name
        self.alloc = alloc
        self._runs = None
        assert all(s >= 0 for s in self.strides), f"streamcheck: view '{name}' has a negative stride"

    @classmethod
    def of(cls, t: torch.Tensor, name: str = "") -> "View":
        es, st = t.element_size(), t.untyped_storage()
        return cls(st.data_ptr(), t.storage_offset() * es, t.shape, [s * es for s in t.stride()], es, name, (st.data_ptr(), st.nbytes()))

    @classmethod
    def raw(cls, addr: int, nbytes: int, name: str = "") -> "View":
        return cls(addr, 0, (int(nbytes),), (1,), 1, name, (int(addr), int(nbytes)))

    @property
    def ptr(self) -> int:
        return self.base + self.offset

    def runs(self) -> Tuple[np.ndarray, int]:
        """(sorted start addresses, bytes per run): the view as maximal contiguous byte runs."""
        if self._runs is None:
            dims = sorted((st, n) for n, st in zip(self.shape, self.strides) if n > 1 and st > 0)
            if any(n == 0 for n in self.shape):
                self._runs = (np.zeros(0, dtype=np.int64), 0)
                return self._runs
            run, outer = self.esize, []
            for st, n in dims:
                if st == run and not outer:
                    run *= n
                else:
                    outer.append((st, n))
            starts = np.array([self.ptr], dtype=np.int64)
            for st, n in outer:
                starts = (starts[:, None] + np.arange(n, dtype=np.int64)[None, :] * st).reshape(-1)
            starts.sort()
            self._runs = (starts, run)
        return self._runs

    @property
    def lo(self) -> int:
        s, _ = self.runs()
        return int(s[0]) if len(s) else self.ptr

    @property
    def hi(self) -> int:
        s, n = self.runs()
        return int(s[-1]) + n if len(s) else self.ptr

    def describe(self) -> str:
        return f"'{self.name}' storage 0x{self.base:x} + {self.offset} shape {self.shape} byte strides {self.strides}"


def overlap(a: View, b: View) -> Optional[Tuple[int, int]]:
    """The first common byte range [lo, hi) of two views, or None: exact (run against run), not a bounding-box test."""
    sa, la = a.runs()
    sb, lb = b.runs()
    if not len(sa) or not len(sb) or a.hi <= b.lo or b.hi <= a.lo:
        return None
    if len(sa) > len(sb):
        sa, la, sb, lb = sb, lb, sa, la
    idx = np.searchsorted(sb, sa + la, side="left") - 1          # the last run of b that starts before the run of a ends (runs of one view are disjoint)
    hit = (idx >= 0) & (sb[np.clip(idx, 0, None)] + lb > sa)
    if not hit.any():
        return None
    i = int(np.argmax(hit))
    j = int(idx[i])
    return max(int(sa[i]), int(sb[j])), min(int(sa[i]) + la, int(sb[j]) + lb)


# ---------------------------------------------------------------------------------------------------------------------
# the log
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Op:
    name: str                      # the ops function
    site: str                      # "file.py:line (function)" of the call
    stream: int                    # plan stream index (0 = main)
    first: int                     # its plan nodes: [first, last)
    last: int
    reads: List[View] = field(default_factory=list)
    writes: List[View] = field(default_factory=list)
    code: str = ""                 # the source line of the call

    def where(self) -> str:
        nodes = f"node {self.first}" if self.last - self.first == 1 else (f"nodes {self.first}..{self.last - 1}" if self.last > self.first else "step entry")
        return f"{nodes} [{self.name} at {self.site}, stream {self.stream}]"


@dataclass
class Sync:
    kind: str                      # "record" | "wait" | "share"
    stream: int                    # raw stream key of the trace
    event: int                     # index of the event in the order of its record (-1: share)
    site: str
    code: str
    node: int = -1                 # plan node index (recording passes)
    view: Optional[View] = None    # share: the tensor kept alive


class Log:
    """A step as the analyser sees it: nodes [(kind, stream, event)] in issue order, ops attached by node range, the entry / exit work of me_denoise_step."""

    def __init__(self):
        self.nodes: List[Tuple[int, int, int]] = []
        self.ops: List[Op] = []
        self.prologue: List[Op] = []
        self.epilogue: List[Op] = []
        self._events = 0

    # -- hand-written logs --
    def launch(self, stream: int, name: str, reads: Sequence[View] = (), writes: Sequence[View] = (), site: str = "", n: int = 1) -> Op:
        op = Op(name, site or f"hand:{len(self.ops)} ({name})", stream, len(self.nodes), len(self.nodes) + n, list(reads), list(writes))
        self.nodes += [(LAUNCH, stream, -1)] * n
        self.ops.append(op)
        return op

    def record(self, stream: int, event: Optional[int] = None) -> int:
        if event is None:
            event, self._events = self._events, self._events + 1
        self.nodes.append((RECORD, stream, event))
        return event

    def wait(self, stream: int, event: int) -> int:
        self.nodes.append((WAIT, stream, event))
        return len(self.nodes) - 1

    def entry(self, name: str, reads: Sequence[View] = (), writes: Sequence[View] = ()) -> None:
        self.prologue.append(Op(name, "me_denoise_step (entry)", 0, 0, 0, list(reads), list(writes)))

    def exit(self, name: str, reads: Sequence[View] = (), writes: Sequence[View] = ()) -> None:
        self.epilogue.append(Op(name, "me_denoise_step (exit)", 0, 0, 0, list(reads), list(writes)))

    def without(self, node: int) -> "Log":
        """A copy with one node deleted (it becomes a NOP: every other index stays)."""
        out = Log()
        out.nodes = list(self.nodes)
        out.nodes[node] = (NOP, self.nodes[node][1], self.nodes[node][2])
        out.ops, out.prologue, out.epilogue, out._events = self.ops, self.prologue, self.epilogue, self._events
        return out


_KIND = {"RAW": "read-after-write", "WAR": "write-after-read", "WAW": "write-after-write"}


@dataclass
class Report:
    kind: str                      # "RAW" | "WAR" | "WAW" | "WAIT_BEFORE_RECORD"
    text: str
    first: Optional[Op] = None     # the earlier access (issue order)
    second: Optional[Op] = None
    replays: Tuple[int, int] = (0, 0)
    lo: int = 0
    hi: int = 0

    def __str__(self) -> str:
        return self.text


def analyse(log: Log, replays: int = 1, limit: int = 64) -> List[Report]:
    """Every unordered conflicting pair of accesses (at most `limit`, one per pair of ops and kind) and every WAIT without a preceding RECORD."""
    n_streams = 1 + max([0] + [s for _, s, _ in log.nodes] + [o.stream for o in log.ops])
    op_at: Dict[int, Op] = {}
    for o in log.ops:
        for i in range(o.first, o.last):
            assert i not in op_at, f"streamcheck: node {i} belongs to two ops"
            op_at[i] = o
    reports: List[Report] = []
    clock = np.zeros((n_streams, n_streams), dtype=np.int64)      # clock[s]: per stream, how many of its nodes happen before (or are) the latest node of s
    ev_clock: Dict[int, np.ndarray] = {}
    inst: List[Tuple[Op, int]] = []                                # op instances in issue order
    i_stream, i_seq_last, i_vc = [], [], []

    def begin(o: Op, r: int, s: int) -> int:
        inst.append((o, r))
        i_stream.append(s)
        i_vc.append(clock[s].copy())
        i_seq_last.append(int(clock[s, s]))
        return len(inst) - 1

    for r in range(replays):
        for o in log.prologue:
            clock[0, 0] += 1
            begin(o, r, 0)
        open_inst: Dict[int, int] = {}
        for i, (kind, s, e) in enumerate(log.nodes):
            if kind == NOP:
                continue
            clock[s, s] += 1
            if kind == RECORD:
                ev_clock[e] = clock[s].copy()
            elif kind == WAIT:
                if e not in ev_clock:
                    reports.append(Report("WAIT_BEFORE_RECORD", f"WAIT before its RECORD: node {i} waits on stream {s} for event {e}, which no earlier node has recorded "
                                                                  "(hipStreamWaitEvent on an event never recorded does not wait)"))
                else:
                    clock[s] = np.maximum(clock[s], ev_clock[e])
            else:
                o = op_at.get(i)
                if o is None:
                    continue
                assert o.stream == s, f"streamcheck: node {i} is on stream {s}, its op {o.where()} on another"
                if i == o.first:
                    open_inst[id(o)] = begin(o, r, s)
                i_seq_last[open_inst[id(o)]] = int(clock[s, s])
        for o in log.epilogue:
            clock[0, 0] += 1
            begin(o, r, 0)

    # one entry per (op instance, view)
    e_inst, e_lo, e_hi, e_w, e_view = [], [], [], [], []
    for k, (o, _) in enumerate(inst):
        for views, w in ((o.reads, False), (o.writes, True)):
            for v in views:
                if v.hi > v.lo:
                    e_inst.append(k), e_lo.append(v.lo), e_hi.append(v.hi), e_w.append(w), e_view.append(v)
    if not e_inst:
        return reports
    e_inst, e_lo, e_hi, e_w = np.array(e_inst), np.array(e_lo, dtype=np.int64), np.array(e_hi, dtype=np.int64), np.array(e_w)
    S, SEQL, VC = np.array(i_stream), np.array(i_seq_last, dtype=np.int64), np.stack(i_vc)
    seen = set()
    for wi in np.nonzero(e_w)[0]:
        kw = e_inst[wi]
        cand = (e_lo < e_hi[wi]) & (e_hi > e_lo[wi]) & (e_inst != kw) & (~e_w | (e_inst > kw))
        if not cand.any():
            continue
        ci = np.nonzero(cand)[0]
        ke = e_inst[ci]
        early, late = np.minimum(ke, kw), np.maximum(ke, kw)
        unordered = VC[late, S[early]] < SEQL[early]              # `early` happens before `late` iff late's clock has reached early's last node
        for c in ci[unordered]:
            k2 = int(e_inst[c])
            kind = "WAW" if e_w[c] else ("RAW" if k2 > kw else "WAR")
            a, b = (int(kw), k2) if kw < k2 else (k2, int(kw))
            if (a, b, kind) in seen:
                continue
            va, vb = (e_view[wi], e_view[c]) if kw < k2 else (e_view[c], e_view[wi])
            rng = overlap(va, vb)
            if rng is None:
                continue
            seen.add((a, b, kind))
            (oa, ra), (ob, rb) = inst[a], inst[b]
            verb_a = "writes" if kind in ("RAW", "WAW") else "reads"
            verb_b = "writes" if kind in ("WAR", "WAW") else "reads"
            reuse = "" if (va.base, va.offset, va.shape, va.strides) == (vb.base, vb.offset, vb.shape, vb.strides) or va.alloc is None or vb.alloc is None or va.alloc == vb.alloc \
                else " -- two different allocations at one address: a block handed out again"
            across = f" -- across replays {ra} and {rb}" if ra != rb else ""
            reports.append(Report(kind, f"{_KIND[kind]} hazard, no event orders the two: {oa.where()} (replay {ra}) {verb_a} {va.describe()}; {ob.where()} (replay {rb}) {verb_b} "
                                        f"{vb.describe()}; common bytes [0x{rng[0]:x}, 0x{rng[1]:x}){reuse}{across}", oa, ob, (ra, rb), rng[0], rng[1]))
            if len(reports) >= limit:
                return reports
    return reports


# ---------------------------------------------------------------------------------------------------------------------
# TABLE: what every launching function of ops reads and writes
# ---------------------------------------------------------------------------------------------------------------------
def _tensors(name, x):
    if isinstance(x, torch.Tensor):
        return [(name, x)]
    if isinstance(x, (tuple, list)):
        return [p for i, y in enumerate(x) for p in _tensors(f"{name}[{i}]", y)]
    return []


def _entry(reads: Sequence[str] = (), writes: Sequence[str] = (), ret: bool = True, hidden: Optional[Callable] = None):
    """reads / writes: argument names (tensors, or tuples holding tensors); ret: every tensor of the return value is written; hidden(ops, args) ->
    (reads, writes) lists of (name, tensor) for operands that are no arguments."""
    def f(o, a, r):
        rd = [p for n in reads for p in _tensors(n, a.get(n))]
        wr = [p for n in writes for p in _tensors(n, a.get(n))] + (_tensors("return", r) if ret else [])
        if hidden is not None:
            hr, hw = hidden(o, a)
            rd, wr = rd + hr, wr + hw
        return rd, wr
    return f


def _step_params(o, a):
    p = getattr(o, "STEP_PARAMS", None)       # the device-resident {t, guidance, ca, cb}: read by me_timestep_embed_dev / me_cfg_ddim_dev, written at every step's entry
    return ([("ops.STEP_PARAMS", p)] if p is not None else []), []


def _gemm(o, a, r):
    x, w = a["x"], a["w"]
    N, _, K = w.shape
    M = a.get("M") or x.shape[0]
    dense = a.get("conv") is None and a.get("tconv") is None
    rd = [("x", x[:M, :K] if dense else x[:, :K]), ("w", w)]           # a gather reads other rows than it writes: all of them
    for n in ("bias", "rowvec", "res", "res2"):
        t = a.get(n)
        if t is None:
            continue
        if n in ("res", "res2"):
            rows = a.get(n + "_rows") or M
            t = t[:rows, :min(N, t.shape[1])]
        elif n == "rowvec":
            t = t[:, :min(N, t.shape[1])]
        rd.append((n, t))
    rd += _tensors("ln", a.get("ln"))
    wr = _tensors("return", r)
    if a.get("row_range") is not None:                                 # only the rows [lo, hi) of the returned view are computed
        lo, hi = a["row_range"]
        wr = [("return", r[lo:hi])]
    return rd, wr


def _attention(o, a, r):
    c = a["heads"] * a["dh"]
    rd = [(n, a[n][:, :c] if a[n].dim() == 2 else a[n]) for n in ("q", "k", "v")] + [("seg_item", a["seg_item"]), ("seg_mode", a["seg_mode"])]
    if a.get("mask") is not None:
        rd.append(("mask", a["mask"]))
    if getattr(o, "ATTN_ITEM_ORDER", False):                            # me_attn_args.item_order: the permutation segments.py keeps beside the table
        from motioneditor_amd import segments
        order = segments.ITEM_ORDER.get(a["seg_item"].data_ptr())
        if order is not None and order.device == a["q"].device and order.numel() == a["n_items"]:
            rd.append(("segments.ITEM_ORDER", order))
    wr = _tensors("return", r if r.shape[1] == c else r[:, :c])
    if a.get("lse") is not None:
        wr.append(("lse", a["lse"]))
    return rd, wr                                                       # (+ vsum: through the library call, Trace._lib_proxy)


def _gn_stats(o, a):
    cache = getattr(o, "_gn_scratch", None)
    if cache is None:                                                   # (the emulation keeps no statistics buffer)
        return [], []
    x = a["x"]
    nbytes = o.capi.lib().me_groupnorm_scratch_bytes(x.shape[0], a["rows_per_group"], a["groups"])
    t = cache[(x.device, nbytes, o._stream(), torch.cuda.is_current_stream_capturing())]      # the key of ops.groupnorm: a KeyError here = the cache changed its rule
    return [("ops._gn_scratch", t)], [("ops._gn_scratch", t)]


def _copy_rows(o, a, r):
    y, x = a["y"], a["x"]
    return [("x", x)], [("y", y[:x.shape[0], :x.shape[1]])]


def _copy_blocks(o, a, r):
    y, x = a["y"], a["x"]
    return [("x", x)], [("y", y[:, :x.shape[1]])]


def _cfg_ddim(o, a, r):
    hr, _ = _step_params(o, a)
    return [("latents", a["latents"]), ("eps_rows", a["eps_rows"][:, :a["latents"].shape[1]])] + hr, _tensors("return", r)


TABLE: Dict[str, Callable] = {
    "gemm": _gemm,
    "ln_stats": _entry(["x"]),
    "conv_small": _entry(["inp", "w", "bias"]),
    "attention": _attention,
    "temporal_attention": _entry(["q", "k", "v"]),
    "groupnorm": _entry(["x", "gamma", "beta"], hidden=_gn_stats),     # returns `out` when one is given
    "layernorm": _entry(["x", "gamma", "beta"]),
    "softmax_rows": _entry(["x"]),
    "axpy_rows": _entry(["x", "a_"], ["y"], ret=False),
    "copy_rows": _copy_rows,
    "copy_blocks": _copy_blocks,
    "clone_rows": _entry(["x"]),
    "repeat_batch": _entry(["x"]),
    "to_f16_rows": _entry(["ehs"]),                                     # (an fp16 contiguous input comes back as a view of itself: no launch, no node, no access)
    "silu": _entry(["x"]),
    "relu": _entry(["x"]),
    "timestep_embed": _entry(hidden=_step_params),
    "cfg_ddim": _cfg_ddim,
    "gaussian_sample": _entry(["moments", "noise"]),
    "nchw_to_rows": _entry(["x"]),
    "rows_to_nchw": _entry(["x"]),
    "nchw5_to_rows": _entry(["x"]),
    "rows_to_nchw5": _entry(["rows"]),
    "cast_f16": _entry(["src"], ["dst"], ret=False),
}

# Public functions of ops.py that reach the library and have no TABLE entry, and why.  (launches, reason): a function that launches raises when a traced step calls it.
NOT_TRACED: Dict[str, Tuple[bool, str]] = {
    "gemm_splits_k": (False, "size query (me_gemm_work_bytes), no launch"),
    "attention_fallback_blocks": (False, "reads the library's diagnostic counter, no launch on tensors"),
    "quick_gelu": (True, "CLIP text encoder: runs before the denoising loop, on one stream"),
    "embed_rows": (True, "CLIP text encoder: runs before the denoising loop, on one stream"),
    "attention_causal": (True, "CLIP text encoder: runs before the denoising loop, on one stream"),
    "image_resize": (True, "clip I/O: refuses to run while a plan records (ops._not_in_a_plan)"),
    "video_grid_u8": (True, "clip I/O: refuses to run while a plan records (ops._not_in_a_plan)"),
    "grad_acc": (True, "training path: single stream, never part of a recorded step"),
    "gemm_dx": (True, "training path: single stream, never part of a recorded step"),
    "geglu_bwd": (True, "training path: single stream, never part of a recorded step"),
    "attention_bwd": (True, "training path: single stream, never part of a recorded step"),
    "temporal_attention_bwd": (True, "training path: single stream, never part of a recorded step"),
    "groupnorm_bwd": (True, "training path: single stream, never part of a recorded step"),
    "layernorm_bwd": (True, "training path: single stream, never part of a recorded step"),
    "gemm_dw": (True, "training path: single stream, never part of a recorded step"),
    "colsum_grad": (True, "training path: single stream, never part of a recorded step"),
    "relu_bwd": (True, "training path: single stream, never part of a recorded step"),
    "layernorm_bwd_params": (True, "training path: single stream, never part of a recorded step"),
    "sumsq_absmax": (True, "training path: single stream, never part of a recorded step"),
    "adamw": (True, "training path: single stream, never part of a recorded step"),
    "mse_seed": (True, "training path: single stream, never part of a recorded step"),
    "refresh_weights": (True, "training path: single stream, never part of a recorded step"),
}


def launching_functions(ops_mod) -> List[str]:
    """The public functions of an ops module whose body reaches `capi.lib()`, directly or through another function of the module."""
    src = {n: inspect.getsource(f) for n, f in vars(ops_mod).items() if inspect.isfunction(f) and f.__module__ == ops_mod.__name__}
    import re
    reach = {n for n, s in src.items() if "capi.lib()" in s}
    grew = True
    while grew:
        grew = False
        for n, s in src.items():
            if n not in reach and any(re.search(rf"\b{re.escape(m)}\(", s) for m in reach):
                reach.add(n)
                grew = True
    return sorted(n for n in reach if not n.startswith("_"))


# ---------------------------------------------------------------------------------------------------------------------
# the trace
# ---------------------------------------------------------------------------------------------------------------------
_SKIP_FILES = ("ops.py", "emu_ops.py", "plan.py", "streamcheck.py", "contextlib.py")


def _site() -> Tuple[str, str]:
    f = sys._getframe(2)
    while f is not None and os.path.basename(f.f_code.co_filename) in _SKIP_FILES:
        f = f.f_back
    if f is None:
        return "?", ""
    return f"{os.path.basename(f.f_code.co_filename)}:{f.f_lineno} ({f.f_code.co_name})", linecache.getline(f.f_code.co_filename, f.f_lineno).strip()


class _LibProxy:
    """capi.lib() while a trace runs: me_attn's argument block names the per-call `vsum` scratch, which ops.attention allocates and drops itself."""

    def __init__(self, real, trace):
        self._real, self._trace = real, trace

    def __getattr__(self, name):
        f = getattr(self._real, name)
        if name != "me_attn":
            return f

        def me_attn(args_ref, stream):
            a = args_ref._obj
            if a.vsum:
                self._trace._hidden_rw.append(View.raw(int(a.vsum), self._real.me_attn_vsum_bytes(a.n_kv_items, a.heads * a.dh), "attention.vsum"))
            return f(args_ref, stream)
        return me_attn


class Trace:
    """with Trace(ops_mod, plan_mod, pl): ...the step... -- patches the attributes of the modules themselves (graph, the pipeline, the model classes, schedulers and
    weights all bind `ops` on their own: they see the same module object); a call nested inside another ops function is logged once, at the outermost.

    pl: the StepPlan that is recording (node ranges from me_plan_info), or None (an eager step: ranges are op counts).
    check_values: synchronise around every op and apply the table-correctness rule -- every operand that existed before the call and shares no element with a
    view classed written must be bitwise unchanged (so: every read-only view is unchanged, and every view that changed is classed written)."""

    def __init__(self, ops_mod, plan_mod=None, pl=None, check_values: bool = False):
        self.ops_mod, self.plan_mod, self.pl, self.check_values = ops_mod, plan_mod, pl, check_values
        self.ops: List[Op] = []
        self.syncs: List[Sync] = []
        self.allocs: Dict[int, int] = {}            # every storage the trace has seen: address -> bytes (the largest seen there)
        self.calls = {"wait_stream": 0, "nested": 0, "checked_views": 0}
        self._depth = 0
        self._saved: List[Tuple[object, str, object]] = []
        self._hidden_rw: List[View] = []
        self._events: Dict[int, int] = {}
        self._keep: List[object] = []
        self._count = 0

    # -- plumbing --
    def _n_nodes(self) -> int:
        if self.pl is None:
            return self._count
        st = self.pl.stats()
        return st["launches"] + st["event_records"] + st["event_waits"]

    def _stream(self) -> int:
        f = getattr(self.ops_mod, "_stream", None)
        return int(f()) if f is not None else 0     # (the emulation has no streams)

    def _patch(self, mod, name, new) -> None:
        self._saved.append((mod, name, getattr(mod, name)))
        setattr(mod, name, new)

    def _view(self, name: str, t) -> View:
        v = t if isinstance(t, View) else View.of(t, name)
        if v.alloc is not None:
            self.allocs[v.alloc[0]] = max(self.allocs.get(v.alloc[0], 0), v.alloc[1])
        return v

    def __enter__(self) -> "Trace":
        o = self.ops_mod
        for name, f in list(vars(o).items()):
            if not inspect.isfunction(f) or f.__module__ != o.__name__ or name.startswith("_"):
                continue
            if name in TABLE:
                self._patch(o, name, self._wrap_op(name, f))
            elif name in NOT_TRACED:
                self._patch(o, name, self._wrap_untraced(name, f))
        if hasattr(o, "_work"):
            real_work = o._work

            def _work(*a, **k):
                t = real_work(*a, **k)
                if self._depth:
                    self._hidden_rw.append(t)
                return t
            self._patch(o, "_work", _work)
        if hasattr(o, "capi"):
            real_lib = o.capi.lib
            self._patch(o.capi, "lib", lambda: _LibProxy(real_lib(), self))
        p = self.plan_mod
        if p is not None:
            real_rec, real_wait, real_ws, real_share = p.record_event, p.wait_event, p.wait_stream, p.share

            def record_event(stream):
                n0 = self._n_nodes()
                ev = real_rec(stream)
                self._events[id(ev)] = len(self._events)
                self._keep.append(ev)
                site, code = _site()
                self.syncs.append(Sync("record", int(stream.cuda_stream), self._events[id(ev)], site, code, n0 if self.pl is not None else -1))
                return ev

            def wait_event(stream, ev):
                n0 = self._n_nodes()
                real_wait(stream, ev)
                site, code = _site()
                self.syncs.append(Sync("wait", int(stream.cuda_stream), self._events.get(id(ev), -1), site, code, n0 if self.pl is not None else -1))

            def wait_stream(waiter, signaller):       # (plan.wait_stream resolves record_event / wait_event at call time: the two above log it)
                self.calls["wait_stream"] += 1
                return real_ws(waiter, signaller)

            def share(t, stream):
                real_share(t, stream)
                site, code = _site()
                self.syncs.append(Sync("share", int(stream.cuda_stream), -1, site, code, -1, self._view("shared", t)))
            for n, f in (("record_event", record_event), ("wait_event", wait_event), ("wait_stream", wait_stream), ("share", share)):
                self._patch(p, n, f)
        return self

    def __exit__(self, *exc) -> None:
        for mod, name, old in reversed(self._saved):
            setattr(mod, name, old)
        self._saved.clear()

    def _wrap_untraced(self, name, fn):
        launches, why = NOT_TRACED[name]

        def wrapper(*a, **k):
            if launches and not self._depth:
                raise AssertionError(f"streamcheck: ops.{name} was called inside a traced step but has no TABLE entry (NOT_TRACED: {why})")
            return fn(*a, **k)
        return wrapper

    def _wrap_op(self, name, fn):
        sig = inspect.signature(fn)
        entry = TABLE[name]

        def wrapper(*a, **k):
            if self._depth:                         # nested inside another ops function: that one's entry covers it
                self.calls["nested"] += 1
                return fn(*a, **k)
            bound = sig.bind(*a, **k)
            bound.apply_defaults()
            args = dict(bound.arguments)
            site, code = _site()
            self._hidden_rw = []
            operands = [p for n, v in args.items() for p in _tensors(n, v)]
            cuda = any(t.is_cuda for _, t in operands)
            before = []
            if self.check_values:
                if cuda:
                    torch.cuda.synchronize()
                before = [(View.of(t, f"{name}.{n}"), t, t.clone()) for n, t in operands + _step_params(self.ops_mod, args)[0]]
            n0, stream = self._n_nodes(), self._stream()
            self._depth += 1
            try:
                ret = fn(*a, **k)
            finally:
                self._depth -= 1
            if self.pl is None:
                self._count += 1
            n1 = self._n_nodes()
            rd, wr = entry(self.ops_mod, args, ret)
            reads = [self._view(f"{name}.{n}", t) for n, t in rd]
            writes = [self._view(f"{name}.{n}", t) for n, t in wr]
            for h in self._hidden_rw:               # scratch handed out during the call: written, then read, by the launches of this op
                v = self._view(f"{name}.scratch", h)
                reads.append(v), writes.append(v)
            self.ops.append(Op(name, site, stream, n0, n1, reads, writes, code))
            if self.check_values:
                if cuda:
                    torch.cuda.synchronize()
                for v, t, snap in before:
                    if any(overlap(v, w) is not None for w in writes):
                        continue
                    self.calls["checked_views"] += 1
                    bt = _BITS[t.element_size()]
                    if not torch.equal(t.view(bt), snap.view(bt)):
                        bad = int((t.view(bt) != snap.view(bt)).sum())
                        raise AssertionError(f"streamcheck: TABLE['{name}'] is wrong: operand {v.describe()} of the call at {site} is not classed written, "
                                             f"but {bad} of its elements changed")
            return ret
        return wrapper


# ---------------------------------------------------------------------------------------------------------------------
# a recorded plan against its trace
# ---------------------------------------------------------------------------------------------------------------------
def build_log(tr: Trace, pl, lat_in=None, text=None, params=None, lat_out=None) -> Log:
    """Check 1 (trace against plan) and the Log for analyse(): the RECORD / WAIT nodes of the plan, with their streams and events, are the sequence the trace saw;
    the node ranges of the ops tile the plan's launches with none left over.  lat_in .. lat_out: the tensors given to plan.bind."""
    log = Log()
    log.nodes = [(k, s, e) for k, s, e, _, _ in pl.nodes()]
    stream_of: Dict[int, int] = {}                   # raw stream key of the trace -> the plan's stream index
    covered = np.zeros(len(log.nodes), dtype=np.int64)
    for o in tr.ops:
        assert 0 <= o.first <= o.last <= len(log.nodes), f"streamcheck: {o.where()} lies outside the plan's {len(log.nodes)} nodes"
        if o.last == o.first:
            continue
        ks = {log.nodes[i][0] for i in range(o.first, o.last)}
        ss = {log.nodes[i][1] for i in range(o.first, o.last)}
        assert ks == {LAUNCH}, f"streamcheck: {o.where()} covers nodes that are not launches"
        assert len(ss) == 1, f"streamcheck: {o.where()} launched on more than one stream: {sorted(ss)}"
        s = ss.pop()
        assert stream_of.setdefault(o.stream, s) == s, f"streamcheck: stream 0x{o.stream:x} of the trace maps to plan streams {stream_of[o.stream]} and {s}"
        covered[o.first:o.last] += 1
        log.ops.append(Op(o.name, o.site, s, o.first, o.last, o.reads, o.writes, o.code))
    assert len(set(stream_of.values())) == len(stream_of), f"streamcheck: two streams of the trace map to one plan stream: {stream_of}"
    launches = np.array([k == LAUNCH for k, _, _ in log.nodes])
    assert not (covered[launches] != 1).any(), (f"streamcheck: {int((covered[launches] == 0).sum())} launches of the plan belong to no traced op (the first: node "
                                                f"{int(np.nonzero(launches & (covered == 0))[0][0]) if (launches & (covered == 0)).any() else -1}), "
                                                f"{int((covered[launches] > 1).sum())} to more than one")
    assert not covered[~launches].any(), "streamcheck: an op's node range covers a RECORD / WAIT node"
    seen = [(RECORD if y.kind == "record" else WAIT, y.stream, y.event, y.node) for y in tr.syncs if y.kind != "share"]
    have = [(k, s, e, i) for i, (k, s, e) in enumerate(log.nodes) if k != LAUNCH]
    assert len(seen) == len(have), f"streamcheck: the trace saw {len(seen)} event records / waits, the plan holds {len(have)}"
    for (k1, s1, e1, n1), (k2, s2, e2, n2) in zip(seen, have):
        s1p = stream_of.setdefault(s1, s2)           # a stream that only ever records / waits is named by its first such node
        assert (k1, s1p, e1, n1) == (k2, s2, e2, n2), f"streamcheck: the trace saw (kind {k1}, stream {s1p}, event {e1}) at node {n1}, the plan holds (kind {k2}, stream {s2}, event {e2}) at node {n2}"
    if lat_in is not None:
        log.entry("hipMemcpyAsync(latents in)", writes=[tr._view("plan.lat_in", lat_in)])
    if text is not None:
        log.entry("hipMemcpyAsync(text in)", writes=[tr._view("plan.text", text)])
    if params is not None:
        log.entry("plan_params_kernel", writes=[tr._view("plan.params", params)])
    if lat_out is not None:
        log.exit("hipMemcpyAsync(latents out)", reads=[tr._view("plan.lat_out", lat_out)])
    return log


def check_completeness(tr: Trace, pl, log: Log) -> int:
    """Check 2: every 8-byte word of a launch's argument bytes (me_plan_node) that is an address inside an allocation the trace knows must lie inside a view that
    TABLE attributes to the op of that launch -- what catches a scratch buffer or a global that the table forgot.  The argument bytes arrive densely packed, each
    argument at its own size, so a pointer behind a 4-byte scalar sits at a multiple of 4: every 4-byte offset is tried.  Returns the number of addresses checked."""
    from motioneditor_amd import capi
    L = capi.lib()
    starts = np.array(sorted(tr.allocs), dtype=np.uint64)
    ends = np.array([a + tr.allocs[a] for a in sorted(tr.allocs)], dtype=np.uint64)
    ends = np.maximum.accumulate(ends)               # (allocations of different sizes at reused addresses may nest)
    info = capi.PlanNodeInfo()
    checked = 0
    for o in log.ops:
        views = o.reads + o.writes
        lo = np.array([v.lo for v in views], dtype=np.uint64)
        hi = np.array([v.hi for v in views], dtype=np.uint64)
        for i in range(o.first, o.last):
            capi.check(L.me_plan_node(pl._handle, i, C.byref(info), None, 0), "me_plan_node")
            n = int(info.arg_bytes)
            buf = C.create_string_buffer(max(n, 8))
            capi.check(L.me_plan_node(pl._handle, i, C.byref(info), buf, n), "me_plan_node")
            w4 = np.frombuffer(buf.raw[:n // 4 * 4], dtype="<u4").astype(np.uint64)
            if len(w4) < 2:
                continue
            words = np.unique(w4[:-1] | (w4[1:] << np.uint64(32)))
            idx = np.searchsorted(starts, words, side="right").astype(np.int64) - 1
            inside = (idx >= 0) & (words < ends[np.clip(idx, 0, None)])
            for addr in words[inside]:
                checked += 1
                if not ((lo <= addr) & (addr < hi)).any():
                    raise AssertionError(f"streamcheck: TABLE['{o.name}'] is incomplete: launch node {i} of {o.where()} is given the address 0x{int(addr):x}, which lies inside an "
                                         f"allocation the trace knows but in none of the views attributed to the op: {[v.describe() for v in views]}")
    return checked


def format_reports(reports: Sequence[Report]) -> str:
    return f"{len(reports)} report(s):\n" + "\n".join(f"  {r}" for r in reports)
