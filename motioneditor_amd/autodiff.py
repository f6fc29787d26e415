"""Reverse-mode tape over the C-ABI operators: the host side of the input-gradient (activation) backward that the
null-text optimisation needs (reference: p2p/null_text_optimization.py:133-166 differentiates the guided prev_step loss
w.r.t. the unconditional text embedding through the whole UNet with torch autograd).

The forward launch graph (models/graph.py) stays as it is.  While a tape is recording, every operator call that has a
backward rule is logged with the tensors it read and wrote; `backward()` then walks the log in reverse and calls the
operator's `*_bwd` / `*_dx` primitive of the same backend.  Gradients live in one fp32 buffer per ALLOCATION (a fused
q|k|v tensor, a skip-concat buffer, ...): a view's gradient is the same view of its allocation's buffer, so column slices
and `out=` targets accumulate where they belong without any graph surgery.

The primitives (`ops.gemm_dx`, `ops.geglu_bwd`, `ops.attention_bwd`, `ops.temporal_attention_bwd`, `ops.groupnorm_bwd`,
`ops.layernorm_bwd`, and for trained parameters `ops.gemm_dw`, `ops.colsum_grad`, `ops.layernorm_bwd_params`, `ops.relu_bwd`) are the
kernel-level contract of the backward pass; every accumulation into a gradient buffer goes through `ops.grad_acc`.  On the GPU each is a
HIP kernel of libmotioned (csrc/bwd.hip, attn_bwd.hip, train.hip, tune.hip) or me_gemm itself on transposed weights; tests/emu_ops.py states them on
the CPU (each as the vector-Jacobian product of its forward emulation) and pins this module, through `util.null_optimization` and
`util.adapter_training_grads`, against the reference's own optimisation (tests/golden/null_text.npz, adapter_train.npz).  Still raising
(not differentiated): edited / masked attention segments, shared query items, sharded row orders, the temporal editor's kv_map and the
pad-(0,1,0,1) convolution.

Memory.  A tape recorded with `trainable=` and / or `wrt=` is LEAN: a call that is not downstream of either is not logged, a
logged call keeps only the tensors whose VALUES its rule will read (a frozen GEMM keeps none: its rule needs the geometry of x and out, not
their contents), and the walk drops every gradient buffer and every stash as soon as nothing will touch it again.  With `checkpoint=True`
the blocks that models/graph.py marks as segments keep their boundary tensors only and are run a second time, under a recorder of their
own, when the walk reaches them.  None of this reorders a floating-point operation: the same rules run in the same order on the same
values.  A tape recorded without these arguments keeps everything and can be walked any number of times, as before.

Restrictions (asserted): single assignment -- no allocation region is written twice while recording (true for the
single-branch UNet forward; the in-place motion / ControlNet residual adds of the two-branch step are not differentiated).
"""
from __future__ import annotations

import dataclasses
import os
import weakref
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

_POISON = bool(os.environ.get("ME_GRAD_POISON"))   # tests: never-zeroed gradient buffers start as NaN, so a read before the first store shows
CHECK_RECOMPUTE = bool(os.environ.get("ME_CHECKPOINT_CHECK"))   # every boundary output a segment's second run produces is compared with the kept one; the first difference raises
PARENT_FORM = bool(os.environ.get("ME_TAPE_PARENT"))   # tests / tools/train_memory_bench.py: util's consumers record the keep-everything tape (the A/B baseline of DESIGN.md 7.7)


def _base(t: torch.Tensor) -> torch.Tensor:
    """The allocation `t` lives in.  Operator outputs are fresh contiguous 2-D allocations (or `out=` views of one) on the GPU;
    the CPU emulation sometimes returns a view of a permuted temporary -- such a tensor counts as its own allocation."""
    b = t._base
    return b if (b is not None and b.is_contiguous()) else t


class _Ref:
    """What a rule needs of a tensor whose VALUES it does not read: which allocation it lies in (a serial number, see _Alloc) and which part of it."""
    __slots__ = ("key", "shape", "strides", "off", "bshape", "device", "whole")

    def __init__(self, key: int, t: torch.Tensor, b: torch.Tensor):
        self.key, self.shape, self.strides, self.off = key, tuple(t.shape), tuple(t.stride()), t.storage_offset() - b.storage_offset()
        self.bshape, self.device = tuple(b.shape), b.device
        self.whole = b is t or (t.shape == b.shape and t.stride() == b.stride() and self.off == 0)

    def dim(self) -> int:
        return len(self.shape)

    def same_part(self, o: "_Ref") -> bool:
        return (self.shape, self.strides, self.off, self.bshape) == (o.shape, o.strides, o.off, o.bshape)


class _Alloc:
    """Allocation -> serial number.  The tape and the gradient store name allocations by these, not by id(): a lean tape lets activations die while it
    records, and an id may be handed out again once its tensor is gone.  The id() map holds a weak reference beside each number, so a stale entry is
    recognised on lookup and replaced."""

    def __init__(self):
        self.n = 0
        self.ids: Dict[int, Tuple[weakref.ref, int]] = {}

    def key(self, t: torch.Tensor) -> int:
        b = _base(t)
        e = self.ids.get(id(b))
        if e is not None and e[0]() is b:
            return e[1]
        self.n += 1
        self.ids[id(b)] = (weakref.ref(b), self.n)
        return self.n

    def ref(self, t: torch.Tensor) -> _Ref:
        return _Ref(self.key(t), t, _base(t))


class _Entry:
    __slots__ = ("outs", "rule", "saved", "in_keys", "params")

    def __init__(self, outs, rule, saved, in_keys, params):
        self.outs: Tuple[_Ref, ...] = tuple(outs)             # what the call wrote
        self.rule: Callable = rule
        self.saved: Tuple[torch.Tensor, ...] = tuple(saved)   # the activations whose values the rule reads (a segment: its boundary tensors)
        self.in_keys: Tuple[int, ...] = tuple(in_keys)        # the allocations of the activations the call read
        self.params: Tuple[torch.Tensor, ...] = tuple(params)  # the parameters it read (owned by the weight store; not counted as stash)


class Tape:
    def __init__(self, backend=None, lean: bool = False, alloc: Optional[_Alloc] = None):
        self.backend = backend
        self.lean = lean                      # recorded with trainable= / wrt=: pruned and trimmed at record time, walked once, released during the walk
        self.alloc = alloc if alloc is not None else _Alloc()
        self.entries: List[Optional[_Entry]] = []
        self.keep: List[torch.Tensor] = []    # keep-everything tape only: every tensor a call touched stays alive (and un-recycled) until the tape dies
        self.reach: set = set()               # lean: the allocations downstream of `wrt` or of a trained tensor, so far
        self.wrt_keys: set = set()
        self.walked = False

    def stashed_bytes(self) -> int:
        """Bytes of the unique storages the tape pins (activations; parameters belong to the weight store).  Read at the end of the forward."""
        seen, total = set(), 0
        for t in [t for e in self.entries if e is not None for t in e.saved] + self.keep:
            s = t.untyped_storage()
            if s.data_ptr() not in seen:
                seen.add(s.data_ptr())
                total += s.nbytes()
        return total


class Grads:
    """fp32 gradient buffers, one per allocation; `view(t)` is the part of it that `t` (a tensor, or the tape's _Ref of one) covers.  Every
    accumulation is the backend's `grad_acc` (a HIP kernel on the GPU).  `peak_bytes` is the high-water mark of live buffer bytes, `total_bytes`
    the sum over every buffer ever allocated (the two agree when nothing is released)."""

    def __init__(self, backend, trainable: Optional[Dict[int, str]] = None, param_buffers: Optional[Dict[str, torch.Tensor]] = None,
                 alloc: Optional[_Alloc] = None):
        self.B = backend
        self.A = alloc if alloc is not None else _Alloc()
        self.buf: Dict[int, torch.Tensor] = {}        # allocation key -> its buffer
        self.fresh: set = set()                       # keys of allocations whose buffer exists but holds nothing yet (first-touch store pending)
        self.keep: Dict[int, torch.Tensor] = {}       # allocation key -> the allocation, for buffers asked for by tensor: pinned as long as the buffer lives
        self.alias: Dict[int, int] = {}               # key of a segment's recomputed output -> key of the forward's own output (one buffer for both)
        self.trainable = trainable or {}              # id(packed parameter tensor) -> its key in weights.Packed.cache, or [(row0, row1, key)] of its trained rows
        self.params: Dict[str, torch.Tensor] = param_buffers if param_buffers is not None else {}   # key -> fp32 gradient in the packed layout
        self.live_bytes = self.peak_bytes = self.total_bytes = 0
        self.protected: set = set()                   # lean walk: the allocations whose buffers outlive it (wrt, seeds)

    def wants(self, t: Optional[torch.Tensor]) -> bool:
        return t is not None and id(t) in self.trainable

    def param(self, t: torch.Tensor) -> torch.Tensor:
        """The fp32 gradient buffer (packed layout) of trainable tensor `t`: a zeroed tensor at first use, or the caller's (a view of the
        trainer's flat gradient bucket)."""
        k = self.trainable[id(t)]
        g = self.params.get(k)
        if g is None:
            g = self.params[k] = torch.zeros(t.shape, dtype=torch.float32, device=t.device)
        return g

    def param_rows(self, t: torch.Tensor) -> Optional[List[Tuple[int, int, torch.Tensor]]]:
        """A tensor trained on ROW RANGES (trainable[id(t)] = [(row0, row1, key)], weights.Packed.trainable_rows): [(row0, row1, fp32 gradient
        buffer of rows row0:row1, packed layout)]; None for a tensor trained whole (trainable[id(t)] = key)."""
        spec = self.trainable[id(t)]
        if isinstance(spec, str):
            return None
        out = []
        for r0, r1, k in spec:
            g = self.params.get(k)
            if g is None:
                g = self.params[k] = torch.zeros((r1 - r0, *t.shape[1:]), dtype=torch.float32, device=t.device)
            out.append((r0, r1, g))
        return out

    def param_whole(self, t: torch.Tensor) -> torch.Tensor:
        """The gradient buffer of a tensor that is trained WHOLE, whichever way `trainable` names it (a key, or one row range that covers it)."""
        rows = self.param_rows(t)
        if rows is None:
            return self.param(t)
        if len(rows) != 1 or rows[0][0] != 0 or rows[0][1] != t.shape[0]:
            raise NotImplementedError("autodiff: a norm's affine vector is trained whole, not on row ranges")
        return rows[0][2]

    def _ref(self, t) -> _Ref:
        if isinstance(t, _Ref):
            return t
        r = self.A.ref(t)
        self.keep.setdefault(self.alias.get(r.key, r.key), _base(t))
        return r

    def key(self, t) -> int:
        k = t.key if isinstance(t, _Ref) else self.A.key(t)
        return self.alias.get(k, k)

    def has(self, t) -> bool:
        return self.key(t) in self.buf

    def drop(self, key: int) -> None:
        """Release the buffer of allocation `key` and, with it, the pin on the allocation (the one place where either goes)."""
        key = self.alias.get(key, key)
        g = self.buf.pop(key, None)
        if g is not None:
            self.live_bytes -= g.numel() * 4
        self.fresh.discard(key)
        self.keep.pop(key, None)

    def view(self, t, first_store: bool = False) -> torch.Tensor:
        """The part of its allocation's gradient buffer that `t` covers.  Buffers are zeroed at their first touch -- unless the caller says the
        touch STORES the whole buffer (`first_store`, and `t` is the whole allocation): then the buffer is allocated uninitialised and marked
        fresh until `take_fresh` hands the store permission out; any other touch of a fresh buffer zeroes it first."""
        r = self._ref(t)
        k = self.alias.get(r.key, r.key)
        g = self.buf.get(k)
        if g is None:
            if first_store and r.whole:
                g = torch.full(r.bshape, float("nan"), dtype=torch.float32, device=r.device) if _POISON else torch.empty(r.bshape, dtype=torch.float32, device=r.device)
                self.fresh.add(k)
            else:
                g = torch.zeros(r.bshape, dtype=torch.float32, device=r.device)
            self.buf[k] = g
            self.live_bytes += g.numel() * 4
            self.total_bytes += g.numel() * 4
            self.peak_bytes = max(self.peak_bytes, self.live_bytes)
        elif k in self.fresh and not (first_store and r.whole):
            g.zero_()
            self.fresh.discard(k)
        if r.whole:
            return g
        return g.as_strided(r.shape, r.strides, r.off)

    def take_fresh(self, t) -> bool:
        """True exactly once for a buffer `view(t, first_store=True)` left uninitialised: the caller now stores ALL of it."""
        k = self.key(t)
        if k in self.fresh:
            self.fresh.discard(k)
            return True
        return False

    def add(self, t, g: torch.Tensor, alpha: float = 1.0) -> None:
        """t: a tensor, a _Ref, or None (a lean tape's word for an input nobody reads the gradient of)."""
        if t is None:
            return
        covers = (g.dim() == 2 and t.dim() == 2 and g.shape[0] >= t.shape[0] and g.shape[1] >= t.shape[1]) or (g.dim() != 2 and g.numel() == _numel(t.shape))
        v = self.view(t, first_store=covers)
        store = covers and self.take_fresh(t)
        if g.dim() == 2 and v.dim() == 2:
            self.B.grad_acc(v[:g.shape[0], :g.shape[1]], g, alpha, None, store)
        else:
            self.B.grad_acc(v, g.reshape(v.shape), alpha, None, store)


def _numel(shape) -> int:
    n = 1
    for s in shape:
        n *= s
    return n


# ---------------------------------------------------------------------------------------------------------------------
# operator rules: (grads) -> None, closed over what the backward reads of the forward call.  Upper-case names are tensors (values are
# read), `*r` names are _Refs (geometry only; None on a lean tape = nobody reads that input's gradient)
# ---------------------------------------------------------------------------------------------------------------------
def _rule_gemm(B, x, xr, w, bias, out, outr, resr, res2r, had_res, kw):
    if kw.get("res_rows") or kw.get("res2_rows"):
        # a residual shared by several batch entries (read modulo its row count) would need its gradient SUMMED over the repeats: no rule does that yet
        raise NotImplementedError("autodiff: gemm with a shared residual (res_rows / res2_rows) has no backward rule; record with share=False")
    act, alpha, geglu, Mkw, conv, tconv = kw.get("act", 0), kw.get("alpha", 1.0), kw.get("geglu"), kw.get("M"), kw.get("conv"), kw.get("tconv")
    M = outr.shape[0]

    def rule(G: Grads):
        N, taps, K = w.shape
        dy = G.view(outr)
        for r in (resr, res2r):                              # epilogue residual adds come AFTER the activation: straight through
            if r is not None:
                G.add(r, dy)
        if act == 1:                                         # ReLU epilogue (adapter block1): needs the output WITHOUT the residuals
            if had_res:
                raise NotImplementedError("autodiff: ReLU epilogue together with residual terms")
            dy = B.relu_bwd(dy, out)
        elif act:
            raise NotImplementedError("autodiff: gemm with a SiLU epilogue lies on no differentiated path")
        if (geglu or G.wants(w)) and x is None:
            raise RuntimeError("autodiff: a weight became trainable after its call was recorded (the tape did not keep the call's input)")
        if geglu:
            # y = value * gelu(gate) of the biased pre-activation: recompute it (one GEMM) instead of stashing [M, N] per layer
            pre = B.gemm(x, w, M=Mkw, bias=bias)
            dpre = B.geglu_bwd(pre, dy)
        else:
            dpre = dy
        if G.wants(w):                                       # trainable weight: dW[n, tap, k] = sum_m dpre[m, n] * gather(x)[m, tap, k]
            rows = G.param_rows(w)
            if rows is None:
                B.gemm_dw(dpre, x, dst=G.param(w), taps=taps, K=K, M=M, alpha=alpha, conv=conv, tconv=tconv)
            else:                                            # trained row ranges only (q of a fused q|k|v): frozen rows get no launch
                for r0, r1, dst in rows:
                    B.gemm_dw(dpre[:, r0:r1], x, dst=dst, taps=taps, K=K, M=M, alpha=alpha, conv=conv, tconv=tconv)
        if G.wants(bias):
            rows = G.param_rows(bias)
            if rows is None:
                B.colsum_grad(dpre[:M], dst=G.param(bias))
            else:
                for r0, r1, dst in rows:
                    B.colsum_grad(dpre[:M, r0:r1], dst=dst)
        if xr is not None:
            dst = G.view(xr, first_store=True)
            B.gemm_dx(dpre, w, dst=dst, M=M, alpha=alpha, conv=conv, tconv=tconv, store=G.take_fresh(xr))
    return rule


def _rule_attention(B, q, k, v, out, lse, kw):
    def rule(G: Grads):
        B.attention_bwd(q, k, v, out, G.view(out), dq=G.view(q), dk=G.view(k), dv=G.view(v), lse=lse, **kw)
    return rule


def _rule_tattn(B, q, k, v, out, qr, kr, vr, kw):
    def rule(G: Grads):
        dq, dk, dv = B.temporal_attention_bwd(q, k, v, out, G.view(out), **kw)
        G.add(qr, dq)
        G.add(kr, dk)
        G.add(vr, dv)
    return rule


def _rule_groupnorm(B, x, xr, gamma, beta, outr, kw):
    def rule(G: Grads):
        if kw.get("reduce") is not None:
            raise NotImplementedError("autodiff: frame-sharded GroupNorm is not differentiated")
        aff = {}
        if G.wants(gamma):                                   # trained affine parameters (a vector is trained whole: one row range or the tensor itself)
            aff["dgamma"] = G.param_whole(gamma)
        if G.wants(beta):
            aff["dbeta"] = G.param_whole(beta)
        G.add(xr, B.groupnorm_bwd(x, gamma, beta, G.view(outr), rows_per_group=kw["rows_per_group"], eps=kw["eps"], silu=kw["silu"], groups=kw.get("groups", 32), **aff))
    return rule


def _rule_layernorm(B, x, xr, gamma, beta, outr, eps):
    def rule(G: Grads):
        dy = G.view(outr)
        if G.wants(gamma) or G.wants(beta):
            B.layernorm_bwd_params(x, dy, dgamma=G.param(gamma) if G.wants(gamma) else None, dbeta=G.param(beta) if G.wants(beta) else None, eps=eps)
        G.add(xr, B.layernorm_bwd(x, gamma, dy, eps=eps))
    return rule


def _tensors(obj, out=None) -> List[torch.Tensor]:
    """Every tensor inside a segment's arguments or result (graph.Act and friends are dataclasses; text_kv is a dict of column slices), each once."""
    out = [] if out is None else out
    if isinstance(obj, torch.Tensor):
        if not any(o is obj for o in out):
            out.append(obj)
    elif dataclasses.is_dataclass(obj) and not isinstance(obj, type):
        for f in dataclasses.fields(obj):
            _tensors(getattr(obj, f.name), out)
    elif isinstance(obj, (list, tuple)):
        for o in obj:
            _tensors(o, out)
    elif isinstance(obj, dict):
        for o in obj.values():
            _tensors(o, out)
    return out


def _rule_segment(mod, B, A: "_Alloc", trainable, reach: set, name: str, fn: Callable, args, kw, outs: List[torch.Tensor], rows_scale):
    """The second run of a checkpointed segment and the walk of what it recorded.  Everything that selects a kernel is as it was in the forward:
    the arguments are the very tensors the first run read, `out=` targets are replaced by a same-shaped view of a fresh allocation of the target's
    whole buffer (same leading dimension, same alignment; the forward's own output stays untouched and comparable), ops.SELECT_ROWS_SCALE is
    put back to what the segment started from, and scratch blocks (ops._work) are requested by size, which no kernel choice depends on."""
    def rule(G: Grads):
        kw2 = dict(kw)
        if kw2.get("out") is not None:
            o = kw2["out"]
            b = _base(o)
            kw2["out"] = torch.empty_like(b).as_strided(o.shape, o.stride(), o.storage_offset() - b.storage_offset())
        sub = Tape(B, lean=True, alloc=A)
        sub.reach = reach
        n0 = A.n
        saved_ops, saved_scale = mod.ops, getattr(B, "SELECT_ROWS_SCALE", None)
        mod.ops = Recorder(B, sub, module=mod, trainable=trainable)
        if rows_scale is not None:
            B.SELECT_ROWS_SCALE = rows_scale
        try:
            outs2 = _tensors(fn(*args, **kw2))
        finally:
            mod.ops = saved_ops
            if saved_scale is not None:
                B.SELECT_ROWS_SCALE = saved_scale
        if len(outs2) != len(outs):
            raise RuntimeError(f"autodiff: segment `{name}` returned {len(outs2)} tensors in its second run, {len(outs)} in the forward")
        protected = set()
        for j, (o, o2) in enumerate(zip(outs, outs2)):
            if CHECK_RECOMPUTE and not torch.equal(o, o2):
                bad = (o != o2).reshape(-1).nonzero()
                raise RuntimeError(f"autodiff: recomputed output {j} of segment `{name}` differs from the forward's in {bad.numel()} of {o.numel()} "
                                   f"elements (first at flat index {int(bad[0])}): something that selects a kernel changed between the two runs")
            r, r2 = A.ref(o), A.ref(o2)
            if not r.same_part(r2):
                raise RuntimeError(f"autodiff: segment `{name}` laid its output out differently in its second run")
            k = G.alias.get(r.key, r.key)
            if r2.key != k:
                G.alias[r2.key] = k
            protected.add(k)
        del outs2, kw2                                        # (the replaced `out=` buffer lives on only where a rule of the sub-tape reads it)
        _walk(sub, G, None, protected | G.protected)
        for k in [k for k in G.buf if k > n0]:               # whatever the segment's interior left behind (serial numbers grow: > n0 is the second run's)
            G.drop(k)
        for k in [k for k in G.alias if k > n0]:
            del G.alias[k]
    return rule


# operators without a backward rule that may run while a tape records: they read nothing the loss is differentiated through (the timestep
# embedding, conv_in on the input latents, layout conversions, allocation) or produce gradient-free side data
_GRADIENT_FREE = {"empty", "timestep_embed", "conv_small", "nchw5_to_rows", "rows_to_nchw5", "rows_to_nchw", "nchw_to_rows", "cfg_ddim", "gaussian_sample",
                  "grad_acc", "gemm_dx", "gemm_dw", "geglu_bwd", "attention_bwd", "temporal_attention_bwd", "groupnorm_bwd", "layernorm_bwd", "layernorm_bwd_params",
                  "colsum_grad", "relu_bwd", "sumsq_absmax", "adamw", "cast_f16", "mse_seed", "invalidate_transposed", "PROFILE", "STEP_PARAMS", "F16"}


class Recorder:
    """Stands in for the `ops` module of models/graph.py while a tape records: same functions, same results, plus the log."""

    recording = True   # models/graph.py keeps single assignment while this is its `ops` (out-of-place residual adds)
    NATIVE = False     # ... and keeps its torch-side data movement (text-embedding cast, clone): the library copies / casts that a recorded plan needs have no backward rule

    def __init__(self, backend, tape: Tape, module=None, trainable: Optional[Callable[[], Dict[int, str]]] = None, checkpoint: bool = False):
        self._b, self._t, self._m, self._A = backend, tape, module, tape.alloc
        self._tr = trainable                # () -> {id(packed tensor): ...}, asked per call: packed tensors come into being at their first use
        self._lean = tape.lean
        self._ckpt = checkpoint
        self._in_segment = None             # [a trained tensor was read] while a checkpointed segment runs its forward on the plain backend
        self._written: Dict[int, List[Tuple[int, int, int, int]]] = {}

    def __getattr__(self, name):
        # a compute operator without a rule on a differentiated path would cut the gradient silently: only the gradient-free ones pass
        if name.startswith("_") or name in _GRADIENT_FREE:
            return getattr(self._b, name)
        raise NotImplementedError(f"autodiff: operator `{name}` has no backward rule and is not known to be gradient-free; it may not run while a tape records")

    # -- single-assignment check: (row0, row1, col0, col1) boxes written per allocation must not overlap
    def _mark(self, t: torch.Tensor) -> None:
        b = _base(t)
        off = t.storage_offset() - b.storage_offset()
        ld = t.stride(0) if t.dim() == 2 else t.shape[-1]
        r0, c0 = (off // ld, off % ld) if ld else (0, 0)
        box = (r0, r0 + t.shape[0], c0, c0 + (t.shape[1] if t.dim() == 2 else ld))
        k = self._A.key(b)
        for o in self._written.setdefault(k, []):
            if box[0] < o[1] and o[0] < box[1] and box[2] < o[3] and o[2] < box[3]:
                raise RuntimeError("autodiff: a tensor region is written twice while recording (the tape assumes single assignment)")
        self._written[k].append(box)
        if not self._lean:
            self._t.keep.append(b)

    @staticmethod
    def _own(out, kw):
        """An output that is not an `out=` target must be an allocation of its own (the CPU emulation may hand back a view)."""
        return out if (kw.get("out") is not None or out._base is None) else out.contiguous().clone()

    # -- what a lean tape decides as the call is recorded
    def _wants(self, p: Optional[torch.Tensor]) -> bool:
        return p is not None and self._tr is not None and id(p) in self._tr()

    def _skip(self, acts: Sequence[Optional[torch.Tensor]], params: Sequence[Optional[torch.Tensor]]) -> bool:
        """True: the call is not logged -- it runs inside a checkpointed segment's forward, or (lean tape) it is downstream neither of `wrt` nor of
        a trained tensor.  The reachability backward() computes for a keep-everything tape, online."""
        trained = any(self._wants(p) for p in params)
        if self._in_segment is not None:
            self._in_segment[0] |= trained
            return True
        if not self._lean:
            return False
        R = self._t.reach
        return not (trained or any(t is not None and self._A.key(t) in R for t in acts))

    def _in(self, t: Optional[torch.Tensor]) -> Optional[_Ref]:
        """The _Ref through which a rule adds to input `t`'s gradient; None (lean) when nothing upstream of `t` will read it."""
        if t is None:
            return None
        r = self._A.ref(t)
        return r if (not self._lean or r.key in self._t.reach) else None

    def _log(self, outs: Sequence[torch.Tensor], rule: Callable, acts: Sequence[Optional[torch.Tensor]], saved: Sequence[Optional[torch.Tensor]],
             params: Sequence[Optional[torch.Tensor]] = ()) -> None:
        """acts: the activations the call read; saved: those of them (and of its outputs) whose values the rule reads."""
        for o in outs:
            self._mark(o)
        refs = [self._A.ref(o) for o in outs]
        acts = [t for t in acts if t is not None]
        if not self._lean:                   # the keep-everything tape: whatever the call touched
            self._t.keep.extend(acts)
            self._t.keep.extend(outs)
        self._t.entries.append(_Entry(refs, rule, [t for t in saved if t is not None], [self._A.key(t) for t in acts], [p for p in params if p is not None]))
        if self._lean:
            self._t.reach.update(r.key for r in refs)

    def gemm(self, x, w, **kw):
        out = self._own(self._b.gemm(x, w, **kw), kw)
        res, res2, bias = kw.get("res"), kw.get("res2"), kw.get("bias")
        if self._skip((x, res, res2), (w, bias)):
            return out
        M, N = out.shape
        geglu = bool(kw.get("geglu"))
        need_x = geglu or not self._lean or self._wants(w)               # a frozen GEMM's rule reads no activation: dx = dy W
        need_out = kw.get("act", 0) == 1
        kws = {a: b for a, b in kw.items() if not isinstance(b, torch.Tensor)}   # the scalars the rule reads; no tensor is pinned through them
        rule = _rule_gemm(self._b, x if need_x else None, self._in(x[:, :w.shape[2]]), w, bias if (geglu or self._wants(bias) or not self._lean) else None,
                          out if need_out else None, self._A.ref(out), None if res is None else self._in(res[:M, :N]), None if res2 is None else self._in(res2[:M, :N]), res is not None or res2 is not None, kws)
        self._log([out], rule, (x, res, res2), (x if need_x else None, out if need_out else None), (w, bias))
        return out

    def attention(self, q, k, v, **kw):
        lse = torch.empty((kw["n_items"] * kw["nq"], kw["heads"]), dtype=torch.float32, device=q.device)   # stashed for the fused backward
        out = self._own(self._b.attention(q, k, v, lse=lse, **kw), kw)
        if self._skip((q, k, v), ()):
            return out
        kw = {a: b for a, b in kw.items() if a != "out"}
        self._log([out], _rule_attention(self._b, q, k, v, out, lse, kw), (q, k, v), (q, k, v, out, lse, kw.get("mask")))
        return out

    def temporal_attention(self, q, k, v, **kw):
        out = self._own(self._b.temporal_attention(q, k, v, **kw), kw)
        if self._skip((q, k, v), ()):
            return out
        kws = {a: b for a, b in kw.items() if a != "out"}
        self._log([out], _rule_tattn(self._b, q, k, v, out, self._in(q), self._in(k), self._in(v), kws), (q, k, v), (q, k, v, out))
        return out

    def groupnorm(self, x, gamma, beta, **kw):
        out = self._own(self._b.groupnorm(x, gamma, beta, **kw), kw)
        if self._skip((x,), (gamma, beta)):
            return out
        self._log([out], _rule_groupnorm(self._b, x, self._in(x), gamma, beta, self._A.ref(out), {a: b for a, b in kw.items() if a != "out"}), (x,), (x,), (gamma, beta))
        return out

    def layernorm(self, x, gamma, beta, eps=1e-5):
        out = self._own(self._b.layernorm(x, gamma, beta, eps), {})
        if self._skip((x,), (gamma, beta)):
            return out
        self._log([out], _rule_layernorm(self._b, x, self._in(x), gamma, beta, self._A.ref(out), eps), (x,), (x,), (gamma, beta))
        return out

    def copy_rows(self, y, x):
        out = self._b.copy_rows(y, x)
        if self._skip((x,), ()):
            return out
        xr, yr = self._in(x), self._A.ref(y)
        self._log([y], lambda G: G.add(xr, G.view(yr)), (x,), ())
        return out

    def axpy_rows(self, y, x, a_, alpha=1.0):
        if _base(y) is _base(x):
            raise RuntimeError("autodiff: in-place axpy_rows is not differentiated")
        out = self._b.axpy_rows(y, x, a_, alpha)
        if self._skip((x, a_), ()):
            return out
        xr, ar, yr = self._in(x), self._in(a_), self._A.ref(y)
        self._log([y], lambda G: (G.add(xr, G.view(yr)), G.add(ar, G.view(yr), alpha)), (x, a_), ())
        return out

    # -- activation checkpointing: models/graph.py hands every resnet_block / transformer2d / adapter_block through here
    def segment(self, name: str, fn: Callable, args, kw):
        """Without checkpointing (or inside a segment already): a plain call, the block's operators are logged one by one.  With it: the block
        runs on the plain backend, its boundary tensors -- the tensors among its arguments, and its result -- are all the tape keeps of it, and
        the walk runs it again (_rule_segment).  A segment that is downstream neither of `wrt` nor of a trained tensor, and reads no trained
        tensor itself, keeps nothing."""
        if not self._ckpt or self._in_segment is not None:
            return fn(*args, **kw)
        ins = _tensors((args, kw))
        flag = self._in_segment = [False]
        try:
            res = fn(*args, **kw)
        finally:
            self._in_segment = None
        R = self._t.reach
        if not (flag[0] or any(self._A.key(t) in R for t in ins)):
            return res
        outs = _tensors(res)
        rule = _rule_segment(self._m, self._b, self._A, self._tr, R, name, fn, args, kw, outs, getattr(self._b, "SELECT_ROWS_SCALE", None))
        self._log(outs, rule, ins, ins + outs)
        return res


class record:
    """`with autodiff.record(graph) as tape:` -- the module's `ops` is a Recorder for the duration.

    trainable (a dict id(packed tensor) -> key / row ranges as backward() takes it, or a callable that returns the current one: packed tensors
    come into being at their first use, and a call's weight exists when the call is recorded) and wrt (the input tensors whose gradients the
    caller will read) make the tape LEAN -- see the module docstring; backward() must then be given the same `trainable`.  checkpoint: the
    segments of models/graph.py keep their boundary tensors only and are recomputed in the walk (needs a lean tape)."""

    def __init__(self, module, trainable=None, wrt: Optional[Sequence[torch.Tensor]] = None, checkpoint: bool = False):
        self.m = module
        self.lean = trainable is not None or wrt is not None
        if checkpoint and not self.lean:
            raise ValueError("autodiff.record: checkpoint=True needs trainable= and / or wrt= (what to recompute towards is decided as the tape records)")
        self.trainable = trainable if (trainable is None or callable(trainable)) else (lambda: trainable)
        self.wrt, self.checkpoint = list(wrt or ()), checkpoint

    def __enter__(self) -> Tape:
        self.saved = self.m.ops
        self.tape = Tape(self.saved, lean=self.lean)
        self.tape.wrt_keys = {self.tape.alloc.key(t) for t in self.wrt}
        self.tape.reach = set(self.tape.wrt_keys)
        self.m.ops = Recorder(self.saved, self.tape, module=self.m, trainable=self.trainable, checkpoint=self.checkpoint)
        return self.tape

    def __exit__(self, *exc):
        self.m.ops = self.saved
        return False


def _walk(tape: Tape, G: Grads, relevant: Optional[List[bool]], protected: set) -> None:
    """Run the rules of `tape` in reverse.  A lean tape is consumed: an entry's stash goes when its rule has run, and a gradient buffer goes when
    the earliest entry that writes into its allocation has run its rule (nothing upstream of that entry can touch it) -- unless it is
    protected: asked for through `wrt`, a seed, or the output of the segment this walk recomputes.  A buffer that an entry created for an
    input outside the tape's reach (attention hands dq / dk / dv to its kernel whether anybody reads them or not) goes at once."""
    n = len(tape.entries)
    first: Dict[int, int] = {}
    if tape.lean:
        if tape.walked:
            raise RuntimeError("autodiff: a tape recorded with trainable= / wrt= releases what it holds as it is walked: it can be walked once")
        tape.walked = True
        for i, e in enumerate(tape.entries):
            for r in e.outs:
                first.setdefault(r.key, i)
    for i in range(n - 1, -1, -1):
        e = tape.entries[i]
        if (relevant is None or relevant[i]) and any(G.has(o) for o in e.outs):
            e.rule(G)
        if tape.lean:
            for r in e.outs:
                if first[r.key] == i and G.key(r) not in protected:
                    G.drop(r.key)
            for k in e.in_keys:
                if k not in first and k not in tape.reach and k not in protected:
                    G.drop(k)
            tape.entries[i] = None


def backward(tape: Tape, seeds: Sequence[Tuple[torch.Tensor, torch.Tensor]], trainable: Optional[Dict[int, str]] = None, backend=None,
             param_buffers: Optional[Dict[str, torch.Tensor]] = None, seed_scale: float = 1.0, wrt: Optional[Sequence[torch.Tensor]] = None) -> Grads:
    """seeds: (tensor the forward produced, gradient of the loss w.r.t. it), entered as seed_scale * gradient (the loss scale).  Returns
    the gradient store; `G.view(t)` of any tensor the forward read is its gradient (zeros if nothing depended on it).  trainable:
    id(packed parameter tensor) -> key (weights.Packed.trainable_ids); their gradients, in the packed layout, end up in `G.params[key]`
    (accumulated into `param_buffers[key]` when the caller provides the buffers).  backend: the ops module the tape recorded on.

    wrt: the input tensors whose gradients the caller will read.  With `wrt` and / or `trainable` given, the walk is PRUNED to the calls that
    lie downstream of one of them: the null-text optimisation differentiates w.r.t. the text rows only, which first enter at the first
    cross-attention -- conv_in's successor resnet and the first block's self-attention need no backward at all; the adapter's parameters
    feed the up path only -- the UNet's down path and mid block need none.  (Without both, every call with a gradient is walked.)

    A tape that was RECORDED with them (autodiff.record(..., trainable=, wrt=)) is pruned already; only the gradients of its `wrt` tensors, of
    the seeds and of the parameters are there to be read afterwards -- every other buffer is released during the walk."""
    G = Grads(backend if backend is not None else tape.backend, trainable, param_buffers, alloc=tape.alloc)
    relevant = None
    protected: set = set()
    if tape.lean:
        protected = G.protected = set(tape.wrt_keys) | {G.key(t) for t, _ in seeds} | {G.key(t) for t in (wrt or ())}
    elif wrt is not None or trainable:
        reach = {tape.alloc.key(t) for t in (wrt or ())}
        tr = trainable or {}
        relevant = []
        for e in tape.entries:
            r = any(k in reach for k in e.in_keys) or any(id(p) in tr for p in e.params)
            relevant.append(r)
            if r:
                reach.update(o.key for o in e.outs)
    for t, g in seeds:
        G.add(t, g, seed_scale)
    _walk(tape, G, relevant, protected)
    return G
