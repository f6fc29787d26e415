"""TEST INFRASTRUCTURE: runs a case of tests/fwd_cases.py on a backend and compares two runs, on the helpers of tests/bwd_run.py (errors, bitwise_equal,
kernel_matches).

A backend is anything with the forward API of ``motioneditor_amd.ops``: the HIP library (ops itself), the fp64 reference (tests/ref64_fwd.py), the fp32
emulation (``Emu``: tests/emu_ops.py plus the forms it lacks -- ups = 3, head-major panels -- stated in fp32 here) or a deliberately wrong variant of the
latter (tests/test_fwd_sweep_cpu.py).  ``run`` returns {output name: CPU tensor}.  `X` says how the backend gets its tensors: X.dev moves an input, X.out
makes an output view -- on the GPU a guard-banded one (tests/guard.py) whose bands the caller checks afterwards."""
from __future__ import annotations

import contextlib
import os

import torch

import emu_ops
import fwd_cases as fc
import ref64_fwd
from bwd_run import _cpu, bitwise_equal, errors, kernel_matches   # noqa: F401  (re-exported: the sweeps' shared comparison helpers)

F16 = torch.float16


class Exchange:
    def __init__(self, dev, out_dtype, out=None):
        self.dev = dev
        self._out = out
        self.out_dtype = out_dtype

    def out(self, rows, cols, ld_pad=0, off=0, dtype=None):
        """An output view [rows, cols] with `ld_pad` more elements per row and `off` elements in front of every row (off = 4: 8-byte, not 16-byte aligned)."""
        if self._out is not None:
            return self._out(rows, cols, ld_pad, off, dtype or F16)
        dt = self.out_dtype if dtype in (None, F16) else (torch.float64 if self.out_dtype == torch.float64 else dtype)
        return torch.zeros((rows, cols + ld_pad + (8 if off else 0)), dtype=dt)[:, off:off + cols]


REF = Exchange(lambda t: t.clone(), torch.float64)
EMU = Exchange(lambda t: t.clone(), F16)


@contextlib.contextmanager
def switches(env):
    """The per-call switches of a case, set around its launch and put back (the library reads them with getenv at every call)."""
    env = {k: str(v) for k, v in (env or {}).items()}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Emu:
    """tests/emu_ops.py with the forms it lacks in front of it, in fp32."""
    name = "emu"

    def __getattr__(self, n):
        return getattr(emu_ops, n)

    def _ups3(self, x, w16, conv):
        Hin, Win, Hout, Wout = conv[:4]
        N, _, K = w16.shape
        n_img = x.shape[0] // (Hin * Win)
        pad = torch.zeros((n_img, Hin + 2, Win + 2, K))
        pad[:, 1:-1, 1:-1] = x.float()[:, :K].reshape(n_img, Hin, Win, K)
        y = torch.zeros((n_img, Hout, Wout, N))
        wf = w16.float()
        for py in range(2):
            for px in range(2):
                for ty in range(2):
                    for tx in range(2):
                        y[:, py::2, px::2] += pad[:, py + ty:py + ty + Hin, px + tx:px + tx + Win] @ self.ups3_tap(wf, py, px, ty, tx).t()
        return y.reshape(-1, N)

    def ups3_tap(self, wf, py, px, ty, tx):
        return wf[:, 4 * (2 * py + px) + 2 * ty + tx]

    def gemm(self, x, w, *, head_major=None, conv=None, M=None, **kw):
        if conv is not None and conv[5] == 3:             # the gather in fp32, then emu_ops' epilogue on it through an identity weight (exact in fp32)
            acc = self._ups3(x, w, conv)
            y = emu_ops.gemm(acc, torch.eye(w.shape[0])[:, None, :], M=M, **kw)
        else:
            y = emu_ops.gemm(x, w, M=M, conv=conv, **kw)
        if head_major is not None:
            col0, dh = head_major
            panels = y[:, col0:].reshape(y.shape[0], -1, dh).permute(1, 0, 2).contiguous()
            return (y[:, :col0] if col0 else None), panels
        return y

    def attention(self, q, k, v, *, heads, dh, **kw):
        rows = lambda t: t.permute(1, 0, 2).reshape(t.shape[1], heads * dh) if t.dim() == 3 else t    # noqa: E731
        return emu_ops.attention(rows(q), rows(k), rows(v), heads=heads, dh=dh, **kw)


# ---------------------------------------------------------------------------------------------------------------- gemm
def gemm_struct(capi, a):
    """me_gemm_args as far as me_gemm_work_bytes reads them (a host function: the addresses are never dereferenced)."""
    s = capi.GemmArgs()
    s.M, s.N, s.K = a["M"], a["N"], a["K"]
    s.gather = capi.GATHER_CONV3 if a.get("conv") else (capi.GATHER_TCONV if a.get("tconv") else capi.GATHER_DENSE)
    s.ups = a["conv"][5] if a.get("conv") else 0
    s.geglu, s.m_off = int(bool(a.get("geglu"))), a.get("m_off", 0)
    s.C2 = 16 if a.get("C2") else None
    s.ln_stats = 16 if a.get("ln") else None
    return s


def gemm_kwargs(case, t, X, M=None):
    """ops.gemm's arguments for the case's full launch (or its first M rows)."""
    p = case.p
    K = p["K"]
    Mf = p["M"]
    M = Mf if M is None else M
    kw = dict(M=M, geglu=bool(p.get("geglu")), act=p.get("act", 0), alpha=p.get("alpha", 1.0))
    if p.get("conv"):
        kw["conv"] = tuple(p["conv"])
    if p.get("tconv"):
        tc = tuple(p["tconv"])
        if len(tc) > 3:
            halo = Mf // tc[0]
            tc = tc[:5] + (Mf if tc[5] == "prev" else -1, Mf + halo if tc[6] == "next" else -1)
        kw["tconv"] = tc
    x = X.dev(t["x"])[:, :K]
    w = X.dev(t["w"])
    if "bias" in t:
        kw["bias"] = X.dev(t["bias"])
    if "rowvec" in t:
        kw["rowvec"], kw["rows_per_vec"] = X.dev(t["rowvec"]), p["rowvec"]
    n_out = p["N"] // 2 if p.get("geglu") else p["N"]
    for n in ("res", "res2"):
        if n in t and p.get(n) != "alias":
            off = p.get("res_off", 0) if n == "res" else 0
            if off:                                          # 8-byte, not 16-byte aligned: the tensor at column `off` of a wider one
                rows = t[n].shape[0]
                wide = X.dev(torch.cat([torch.full((rows, off), 7.0, dtype=F16), t[n], torch.full((rows, 8 - off), 7.0, dtype=F16)], dim=1))
                kw[n] = wide[:, off:off + n_out]
            else:
                kw[n] = X.dev(t[n])
            kw[n + "_rows"] = p.get(n + "_rows", 0)
    if p.get("ln"):
        kw["ln"] = (X.dev(t["ln_stats"]), X.dev(t["ln_colsum"]), X.dev(t["ln_cvec"]), 1e-5)
    return x, w, kw, n_out


@contextlib.contextmanager
def _work_fault(B, kind):
    """HIP only: hand me_gemm split-K scratch that is one byte short, or 8 bytes off its 16-byte alignment (me_gemm must fall back to the unsplit launch)."""
    if kind is None or not hasattr(B, "capi"):
        yield
        return
    L = B.capi.lib()
    real_bytes, real_work = L.me_gemm_work_bytes, B._work
    try:
        if kind == "short":
            L.me_gemm_work_bytes = lambda a: real_bytes(a) - 1
        else:
            B._work = lambda nbytes, device, tag: real_work(nbytes + 16, device, tag)[2:]
        yield
    finally:
        L.me_gemm_work_bytes, B._work = real_bytes, real_work


def run_gemm(case, B, t, X, hook, sub=0, pieces=None):
    """sub = k: the first M / k rows as a sub-batch that selects its kernel as the full launch does (HIP: ops.SELECT_ROWS_SCALE); pieces = cuts: the launch
    as row-range launches [0, c0), [c0, c1), ..., [c_last, M) into one output."""
    p = case.p
    Mf = p["M"]
    M = Mf // sub if sub else Mf
    x, w, kw, n_out = gemm_kwargs(case, t, X, M)
    res = {}
    if p.get("head_major") is not None:                     # ops.gemm allocates these outputs itself: no guard bands
        with _work_fault(B, p.get("work")):
            y, panels = B.gemm(x, w, head_major=tuple(p["head_major"]), **kw)
        hook("launch")
        if y is not None:
            res["y"] = _cpu(y)
        res["panels"] = _cpu(panels)
        return res
    out = X.out(Mf if pieces else M, n_out, p.get("c_pad", 0), p.get("c_off", 0))
    for n in ("res", "res2"):
        if p.get(n) == "alias":
            out.copy_(X.dev(t[n])[:M].to(out.dtype))
            kw[n], kw[n + "_rows"] = out, 0
    if p.get("ln_out"):
        kw["ln_out"] = True
    old_scale = getattr(B, "SELECT_ROWS_SCALE", 1)
    try:
        if sub and hasattr(B, "capi"):
            B.SELECT_ROWS_SCALE = sub
        with _work_fault(B, p.get("work")):
            if pieces:
                cuts = [0] + list(pieces) + [Mf]
                for lo, hi in zip(cuts[:-1], cuts[1:]):
                    if hi > lo:
                        B.gemm(x, w, out=out, row_range=(lo, hi), **kw)
                        hook("launch")
                y = out
            else:
                y = B.gemm(x, w, out=out, **kw)
                hook("launch")
    finally:
        if hasattr(B, "capi"):
            B.SELECT_ROWS_SCALE = old_scale
    if p.get("ln_out"):
        y, st = y
        res["ln_sum"], res["ln_sumsq"] = _cpu(st)[:, :, 0], _cpu(st)[:, :, 1]
    res["y"] = _cpu(y)[:M, :n_out]
    return res


# ---------------------------------------------------------------------------------------------------------------- attention
def _wide(X, t, pad):
    return X.dev(torch.cat([t, torch.full((t.shape[0], pad), 7.0, dtype=t.dtype)], dim=1))[:, :t.shape[1]] if pad else X.dev(t)


def run_attention(case, B, t, X, hook, order=True):
    p = case.p
    heads, dh, nq, nk = p["heads"], p["dh"], p["nq"], p["nk"]
    C, n_items = heads * dh, len(p["table"])
    kw = dict(heads=heads, dh=dh, n_items=n_items, nq=nq, nk=nk, q_items=p.get("q_items", 0))
    if p.get("scale"):
        kw["scale"] = p["scale"]
    if p.get("fused"):
        assert nq == nk and p["n_kv"] == n_items and not p.get("q_items")
        qkv = X.dev(torch.cat([t["q"], t["k"], t["v"]], dim=1))
        q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    else:
        q, k, v = _wide(X, t["q"], p.get("q_pad", 0)), X.dev(t["k"]), X.dev(t["v"])
    hm = p.get("head_major")
    panels = lambda a: a.reshape(a.shape[0], heads, dh).permute(1, 0, 2).contiguous()    # noqa: E731
    if hm:
        k, v = panels(k), panels(v)
        if hm == "qkv":
            q = panels(q)
    si, sm = X.dev(t["seg_item"]), X.dev(t["seg_mode"])
    mask = X.dev(t["mask"]) if "mask" in t else None
    out = X.out(n_items * nq, C, p.get("o_pad", 0), p.get("o_off", 0))
    lse = X.out(n_items * nq, heads, dtype=torch.float32) if p.get("lse") else None
    registered = None
    if p.get("item_order") and order and hasattr(B, "capi"):
        from motioneditor_amd import segments
        registered = si.data_ptr()
        segments.ITEM_ORDER[registered] = torch.tensor(p["item_order"], dtype=torch.int32, device=si.device)
    try:
        B.attention(q, k, v, seg_item=si, seg_mode=sm, mask=mask, out=out, lse=lse, **kw)
        hook("launch")
    finally:
        if registered is not None:
            from motioneditor_amd import segments
            segments.ITEM_ORDER.pop(registered, None)
    res = {"o": _cpu(out)[:, :C]}
    if lse is not None:      # the reference's comes from its attention_lse, the statement of what the forward stashes
        res["lse"] = B.attention_lse(q, k, seg_item=si, seg_mode=sm, **kw) if hasattr(B, "attention_lse") else _cpu(lse)
    return res


# ---------------------------------------------------------------------------------------------------------------- the smaller families
def run_tattn(case, B, t, X, hook):
    p = case.p
    heads, dh = p["heads"], p["dh"]
    C = heads * dh
    kw = dict(heads=heads, dh=dh, batch=p["batch"], frames=p["frames"], npix=p["npix"], kv_map=p.get("kv_map"), q_frames=p.get("q_frames", 0), q_frame0=p.get("q_frame0", 0),
              kv_parts=p.get("kv_parts", 1), q_parts=p.get("q_parts", 1))
    if p.get("scale"):
        kw["scale"] = p["scale"]
    kv = X.dev(t["kv"])
    q, k, v = _wide(X, t["q"], 8 if p.get("fused") else 0), kv[:, :C], kv[:, C:]
    if not hasattr(B, "capi"):
        return {"y": _cpu(B.temporal_attention(q, k, v, **kw))}
    out = X.out(q.shape[0], C)
    B.temporal_attention(q, k, v, out=out, **kw)
    hook("launch")
    return {"y": _cpu(out)}


def run_small(case, B, t, X, hook):
    p, e = case.p, case.entry
    hip = hasattr(B, "capi")
    if e == "groupnorm":
        x = _wide(X, t["x"], p.get("x_pad", 0))
        kw = dict(rows_per_group=p["rpg"], eps=1e-5, silu=p["silu"])
        if p.get("split"):                                   # stats -> hook -> apply: k times the statistics over k times the count is the identity
            k = p["split"]
            kw.update(reduce=lambda st: st.mul_(k), rows_per_group_total=k * p["rpg"])
        out = X.out(x.shape[0], p["C"]) if hip else None
        y = B.groupnorm(x, X.dev(t["gamma"]), X.dev(t["beta"]), out=out, **kw)
        return {"y": _cpu(y)}
    if e == "layernorm":
        x = _wide(X, t["x"], p.get("x_pad", 0))
        gm, bt = X.dev(t["gamma"]), X.dev(t["beta"])
        if not hip:
            return {"y": _cpu(B.layernorm(x, gm, bt, 1e-5))}
        out = X.out(p["rows"], p["C"])
        B.layernorm(x, gm, bt, 1e-5, out=out)
        return {"y": _cpu(out)}
    if e == "softmax_rows":
        x = _wide(X, t["x"], p["pad"])
        if p.get("inplace") and hip:
            return {"y": _cpu(B.softmax_rows(x, out=x))}
        out = X.out(p["rows"], p["cols"]) if hip else None
        return {"y": _cpu(B.softmax_rows(x, out=out) if hip else B.softmax_rows(x))}
    raise KeyError(e)


def run(case, B, t, X, hook=None, **kw):
    """Run `case` with inputs `t` (fwd_cases.build) on backend B.  hook("launch") is called after every launch -- the GPU test reads me_last_kernel there."""
    hook = hook or (lambda stage: None)
    if case.entry == "gemm":
        return run_gemm(case, B, t, X, hook, **kw)
    if case.entry == "attention":
        return run_attention(case, B, t, X, hook, **kw)
    if case.entry == "temporal_attention":
        return run_tattn(case, B, t, X, hook)
    return run_small(case, B, t, X, hook)


# ---------------------------------------------------------------------------------------------------------------- comparison
def bound_of(case, name):
    if case.bound is not None:
        return case.bound
    if name in ("ln_sum", "ln_sumsq"):
        return fc.BOUNDS["gemm.ln_out"]
    if case.entry == "softmax_rows":
        return fc.BOUNDS["softmax_rows"][0], fc.MAX_REL * case.p["cols"]
    return fc.BOUNDS[case.entry]


def compare(case, got, want, who=""):
    """Assert `got` (a run of the case) against `want` (the fp64 reference's run) inside the entry point's bound; returns {name: (rel-L2, max / mean)}.  The
    row sums of ln_out are held against the sums of the output rows `got` itself stored (the contract: include/motioned.h), the log-sum-exp to an absolute
    bound in its log2 units."""
    figures = {}
    assert set(got) == set(want), (case.id, sorted(got), sorted(want))
    for name in sorted(want):
        g, w = got[name].double(), want[name].double()
        assert tuple(g.shape) == tuple(w.shape), (case.id, name, tuple(g.shape), tuple(w.shape))
        assert bool(torch.isfinite(g).all()), f"{case.id} {who}: {name} is not finite"
        if name == "lse":
            worst = float((g - w).abs().max())
            assert worst <= fc.BOUNDS["attention.lse"][0], f"{case.id} {who}: log-sum-exp off by {worst:.3e} (<= {fc.BOUNDS['attention.lse'][0]})"
            figures[name] = (worst, 0.0)
            continue
        if name in ("ln_sum", "ln_sumsq"):
            parts = ref64_fwd._row_parts(got["y"].to(F16) if got["y"].dtype != torch.float64 else got["y"])
            w = parts[:, :, 0 if name == "ln_sum" else 1]
        rel_b, mx_b = bound_of(case, name)
        r, m = errors(g, w)
        assert r <= rel_b and m <= mx_b, f"{case.id} {who}: {name} rel-L2 {r:.3e} (<= {rel_b}), max/mean {m:.3e} (<= {mx_b})"
        figures[name] = (r, m)
    return figures
