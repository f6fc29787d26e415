"""TEST INFRASTRUCTURE: runs a case of tests/bwd_cases.py on a backend and compares two runs.

A backend is anything with the ``motioneditor_amd.ops`` backward API: the HIP library (ops itself), the fp64 reference (tests/ref64_bwd.py), the fp32
emulation (``Emu``, tests/emu_ops.py behind the two conventions the device path has and the emulation leaves to its caller) or a deliberately wrong variant of
the latter (tests/test_bwd_sweep_cpu.py).  ``run`` returns {output name: CPU tensor}; accumulating entries return the INCREMENT (result - what the buffer
held), so that the content accumulated onto does not dilute the comparison, plus the untouched surroundings of strided views under ``outside.*``."""
from __future__ import annotations

import fnmatch
import math

import torch

import bwd_cases
import emu_ops
from bwd_cases import BOUNDS


ADAMW_DEFAULTS = dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0)      # ops.adamw's


class Emu:
    """tests/emu_ops.py with the device path's conventions applied in front of it: dy reaches the MFMA as fp16 (gemm_dx, gemm_dw: the existing GPU tests
    round it by hand), and a TemporalConv whose chunk does not divide the frames is stated through the emulation's general (frame-sharded) form with
    one shard.  Entries the emulation lacks (no model code calls them through ops) are stated here in fp32."""
    name = "emu"

    def __getattr__(self, n):
        return getattr(emu_ops, n)

    @staticmethod
    def _tc(tconv):
        if tconv is not None and tconv[0] % tconv[2]:
            frames, npix, chunk = tconv
            return (frames, npix, chunk, 0, frames, -1, -1)
        return tconv

    def gemm_dx(self, dy, w, **kw):
        return emu_ops.gemm_dx(dy.half().float(), w, **kw)

    def gemm_dw(self, dy, x, *, tconv=None, **kw):
        return emu_ops.gemm_dw(dy.half().float(), x, tconv=self._tc(tconv), **kw)

    def softmax_bwd_rows(self, P, dP, scale=1.0):
        p, dp = P.float(), dP.float()
        return p * (dp - (p * dp).sum(dim=1, keepdim=True)) * scale

    def cast_rows_f16(self, src, pad_cols):
        out = torch.zeros((src.shape[0], pad_cols), dtype=torch.float16)
        out[:, :src.shape[1]] = src.half()
        return out

    def adamw(self, p, m, v, g, *, gnorm_sq=None, **kw):
        if gnorm_sq is not None and not math.isfinite(float(gnorm_sq.reshape(-1)[0])):
            return                                  # me_adamw's documented no-op; emu_ops.adamw states the finite update only
        for n in ("lr", "beta1", "beta2", "eps", "weight_decay"):     # the hyper-parameters as me_adamw's signature carries them: fp32
            kw[n] = float(torch.tensor(kw.get(n, ADAMW_DEFAULTS.get(n)), dtype=torch.float32))
        return emu_ops.adamw(p, m, v, g, gnorm_sq=gnorm_sq, **kw)


def to_emu(t):
    return t.clone()


def to_ref(t):
    return t.double() if t.dtype == torch.float32 else t.clone()


def _cpu(t):
    return t.detach().cpu()


def _bits(t):
    t = _cpu(t).contiguous()
    return t.view(torch.int32) if t.dtype in (torch.float32,) else (t.view(torch.int16) if t.dtype == torch.float16 else t)


def bitwise_equal(a, b) -> bool:
    """NaN-safe equality of two tensors of the same dtype (NaN-prefilled buffers must stay exactly what they were)."""
    a, b = _cpu(a), _cpu(b)
    if a.dtype != b.dtype:
        b = b.to(a.dtype)
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def run(case, B, t, dev, hook=None):
    """Run `case` with inputs `t` (bwd_cases.build) on backend B; `dev` moves a CPU tensor to the backend (device / dtype).  hook(stage): called after the
    forward ("fwd") and after the launch under test ("bwd") -- the GPU test reads me_last_kernel there."""
    p, e = case.p, case.entry
    hook = hook or (lambda stage: None)
    if e == "gemm_dw":
        N, K, M = p["N"], p["K"], p["M"]
        taps = 3 if p.get("tconv") else 1
        dy, x, dst = dev(t["dy"])[:, :N], dev(t["x"])[:, :K], dev(t["base"])
        B.gemm_dw(dy, x, dst=dst, taps=taps, K=K, M=M, alpha=p.get("alpha", 1.0), tconv=p.get("tconv"))
        hook("bwd")
        return {"dw": _cpu(dst) - to_like(t["base"], dst)}
    if e == "colsum_grad":
        dst = dev(t["base"])
        B.colsum_grad(dev(t["dy"])[:, :p["N"]], dst=dst, alpha=p.get("alpha", 1.0))
        return {"colsum": _cpu(dst) - to_like(t["base"], dst)}
    if e == "gemm_dx":
        K = p["K"]
        base = dev(t["base"])
        B.gemm_dx(dev(t["dy"]), dev(t["w"]), dst=base[:, 4:4 + K], M=p["M"], alpha=p.get("alpha", 1.0), conv=p.get("conv"), tconv=p.get("tconv"), store=bool(p.get("store")))
        hook("bwd")
        got = _cpu(base)
        inc = got[:, 4:4 + K] if p.get("store") else got[:, 4:4 + K] - to_like(t["base"], base)[:, 4:4 + K]
        return {"dx": inc, "outside.left": got[:, :4], "outside.right": got[:, 4 + K:]}
    if e == "attention_bwd":
        heads, dh, nq, nk = p["heads"], p["dh"], p["nq"], p["nk"]
        C, n_items = heads * dh, len(p["table"])
        args = dict(heads=heads, dh=dh, n_items=n_items, nq=nq, nk=nk)
        if p.get("scale"):
            args["scale"] = p["scale"]
        si, sm = dev(t["seg_item"]), dev(t["seg_mode"])
        if p.get("fused"):                       # q | k | v and their gradients as column slices of [rows, 3C] allocations
            assert nq == nk and p["n_kv"] == n_items
            qkv = dev(torch.cat([t["q"], t["k"], t["v"]], dim=1))
            q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
            gg = dev(torch.cat([t["dq"][:, :C], t["dk"][:, C:2 * C], t["dv"][:, 2 * C:]], dim=1))
            dq, dk, dv = gg[:, :C], gg[:, C:2 * C], gg[:, 2 * C:]
            base = [t["dq"][:, :C], t["dk"][:, C:2 * C], t["dv"][:, 2 * C:]]
        else:
            q, k, v = dev(t["q"]), dev(t["k"]), dev(t["v"])
            dq, dk, dv = dev(t["dq"]), dev(t["dk"]), dev(t["dv"])
            base = [t["dq"], t["dk"], t["dv"]]
        out = lse = None
        res = {}
        if hasattr(B, "attention"):              # the forward whose output and log-sum-exp the backward reads (the fp64 reference needs neither)
            lse = dev(torch.zeros((n_items * nq, heads), dtype=torch.float32))
            out = B.attention(q, k, v, seg_item=si, seg_mode=sm, lse=lse, **args)
            hook("fwd")
            res["lse"] = _cpu(lse)
        else:
            res["lse"] = B.attention_lse(t["q"], t["k"], seg_item=t["seg_item"], **args)
        B.attention_bwd(q, k, v, out, dev(t["dout"]), dq=dq, dk=dk, dv=dv, lse=lse, seg_item=si, seg_mode=sm, **args)
        hook("bwd")
        for n, a, b in zip(("dq", "dk", "dv"), (dq, dk, dv), base):
            res[n] = _cpu(a) - to_like(b, a)
        for kit in p.get("unnamed", ()):         # a kv item no query item lists: its rows are not written at all
            res[f"outside.dk{kit}"] = _cpu(dk)[kit * nk:(kit + 1) * nk]
            res[f"outside.dv{kit}"] = _cpu(dv)[kit * nk:(kit + 1) * nk]
        return res
    if e == "temporal_attention_bwd":
        heads, dh = p["heads"], p["dh"]
        C = heads * dh
        o = p.get("q_off", 0)
        if p.get("fused") or o:
            qkv = dev(torch.cat([torch.zeros((t["qkv"].shape[0], o), dtype=t["qkv"].dtype), t["qkv"], torch.zeros((t["qkv"].shape[0], 8 - o if o else 0), dtype=t["qkv"].dtype)], dim=1))
            q, k, v = qkv[:, o:o + C], qkv[:, o + C:o + 2 * C], qkv[:, o + 2 * C:o + 3 * C]
        else:
            q, k, v = (dev(t["qkv"][:, i * C:(i + 1) * C].contiguous()) for i in range(3))
        dout = dev(torch.cat([t["dout"], torch.full((t["dout"].shape[0], p.get("do_pad", 0)), 7.0)], dim=1))[:, :C]
        kw = dict(heads=heads, dh=dh, batch=p["batch"], frames=p["frames"], npix=p["npix"])
        if p.get("scale"):
            kw["scale"] = p["scale"]
        got = B.temporal_attention_bwd(q, k, v, None, dout, **kw)
        hook("bwd")
        return {n: _cpu(a) for n, a in zip(("dq", "dk", "dv"), got)}
    if e == "groupnorm_bwd":
        got = B.groupnorm_bwd(dev(t["x"]), dev(t["gamma"]), dev(t["beta"]), dev(t["dy"]), rows_per_group=p["rpg"], eps=1e-5, silu=p["silu"])
        return {"dx": _cpu(got)}
    if e == "layernorm_bwd":
        C = p["C"]
        x, dy = dev(t["x"])[:, :C], dev(t["dy"])[:, :C]
        if p.get("dx_pad") and hasattr(B, "capi"):          # a strided dx: ops.layernorm_bwd allocates its own, so the C ABI is called directly
            big = dev(torch.full((p["rows"], C + p["dx_pad"]), 5.0))
            dxv, gm = big[:, 8:8 + C], dev(t["gamma"])
            B.capi.check(B.capi.lib().me_layernorm_bwd(dxv.data_ptr(), dxv.stride(0), x.data_ptr(), x.stride(0), gm.data_ptr(), dy.data_ptr(), dy.stride(0), p["rows"], C, 1e-5,
                                                       B._stream()), "me_layernorm_bwd")
            got = _cpu(big)
            return {"dx": got[:, 8:8 + C], "outside.left": got[:, :8], "outside.right": got[:, 8 + C:]}
        got = _cpu(B.layernorm_bwd(x, dev(t["gamma"]), dy, eps=1e-5))
        if p.get("dx_pad"):
            five = torch.full((p["rows"], p["dx_pad"]), 5.0)
            return {"dx": got, "outside.left": five[:, :8], "outside.right": five[:, 8:]}
        return {"dx": got}
    if e == "layernorm_bwd_params":
        C = p["C"]
        dg = dev(t["dgamma"]) if p.get("only") != "dbeta" else None
        db = dev(t["dbeta"]) if p.get("only") != "dgamma" else None
        B.layernorm_bwd_params(dev(t["x"])[:, :C], dev(t["dy"])[:, :C], dgamma=dg, dbeta=db, eps=1e-5)
        res = {}
        if dg is not None:
            res["dgamma"] = _cpu(dg) - to_like(t["dgamma"], dg)
        if db is not None:
            res["dbeta"] = _cpu(db) - to_like(t["dbeta"], db)
        return res
    if e == "geglu_bwd":
        return {"dpre": _cpu(B.geglu_bwd(dev(t["pre"]), dev(t["dy"])[:, :p["N"] // 2]))}
    if e == "softmax_bwd_rows":
        cols = p["cols"]
        P, dP = dev(t["P"])[:, :cols], dev(t["dP"])[:, :cols]
        if hasattr(B, "capi"):                              # no ops wrapper (the fused me_attn_bwd replaced its caller): the C ABI directly, into a strided view
            big = dev(torch.full((p["rows"], cols + 16), 5.0).half())
            dS = big[:, 8:8 + cols]
            B.capi.check(B.capi.lib().me_softmax_bwd_rows(dS.data_ptr(), dS.stride(0), P.data_ptr(), P.stride(0), dP.data_ptr(), dP.stride(0), p["rows"], cols, p["scale"],
                                                          B._stream()), "me_softmax_bwd_rows")
            got = _cpu(big)
            return {"dS": got[:, 8:8 + cols], "outside.left": got[:, :8], "outside.right": got[:, 8 + cols:]}
        five = torch.full((p["rows"], 8), 5.0).half()
        return {"dS": _cpu(B.softmax_bwd_rows(P, dP, p["scale"])), "outside.left": five, "outside.right": five}
    if e == "relu_bwd":
        return {"dx": _cpu(B.relu_bwd(dev(t["dy"])[:, :p["cols"]], dev(t["out"])[:, :p["cols"]]))}
    if e == "grad_acc":
        rows, cols, pad = p["rows"], p["cols"], p["pad"]
        base, src = dev(t["base"]), dev(t["src"])
        if p.get("flat"):
            B.grad_acc(base.reshape(-1), src.reshape(-1), p["alpha"])
            return {"acc": _cpu(base) - to_like(t["base"], base)}
        B.grad_acc(base[:, pad:pad + cols], src[:, :cols], p["alpha"], pool=p.get("pool"), store=bool(p.get("store")))
        got = _cpu(base)
        inc = got[:, pad:pad + cols] if p.get("store") else got[:, pad:pad + cols] - to_like(t["base"], base)[:, pad:pad + cols]
        return {"acc": inc, "outside.left": got[:, :pad], "outside.right": got[:, pad + cols:]}
    if e == "cast_rows_f16":
        view = dev(t["src"])[:, p["off"]:p["off"] + p["cols"]]
        got = B._f16(view, p["pad_cols"]) if hasattr(B, "_f16") else B.cast_rows_f16(view, p["pad_cols"])
        return {"f16": _cpu(got)}
    if e == "cast_f16":
        dst = dev(torch.full((p["n"],), 5.0).half())
        return {"f16": _cpu(B.cast_f16(dst, dev(t["src"])))}
    if e == "mse_seed":
        full = p["full"]
        kw = dict(guidance=7.5, ca=1.01, cb=-0.2, coef=0.3) if full else dict(coef=2.0 / t["target"].numel())
        d, r = B.mse_seed(dev(t["eu"]), dev(t["target"]), eps_c=dev(t["ec"]) if full else None, x=dev(t["x"]) if full else None, **kw)
        return {"diff": _cpu(d), "seed": _cpu(r)}
    if e == "adamw":
        P_, M_, V_, G_ = dev(t["p"]), dev(t["m"]), dev(t["v"]), dev(t["g"])
        ls = 256.0
        G_ = G_ * ls                                          # the bucket arrives loss-scaled; grad_scale divides it out
        gn = None
        if p["clip"] in ("active", "idle"):
            gn = B.sumsq_absmax(G_)
        elif p["clip"] in ("inf", "nan"):
            gn = dev(torch.tensor([float(p["clip"]), 1.0], dtype=torch.float32))
        B.adamw(P_, M_, V_, G_, lr=1e-3, weight_decay=p["wd"], step=p["step"], gnorm_sq=gn, max_grad_norm=1.0, grad_scale=1.0 / ls)
        return {"p": _cpu(P_), "m": _cpu(M_), "v": _cpu(V_), "update": _cpu(P_) - to_like(t["p"], P_)}
    if e == "sumsq_absmax":
        r = _cpu(B.sumsq_absmax(dev(t["x"])))
        return {"sumsq": r[0:1], "absmax": r[1:2]}
    raise KeyError(e)


def to_like(cpu_t, like):
    """The CPU original in the precision the backend computed in (fp64 for the reference): what an accumulating entry started from."""
    return cpu_t.to(torch.float64) if like.dtype == torch.float64 else cpu_t.clone()


def errors(got, want):
    got, want = _cpu(got).double(), _cpu(want).double()
    diff = (got - want)
    return float(diff.norm() / want.norm().clamp_min(1e-30)), float(diff.abs().max() / want.abs().mean().clamp_min(1e-30))


def bound_of(case, name):
    if case.bound is not None:
        return case.bound
    e = case.entry
    if e == "layernorm_bwd_params":
        return BOUNDS[f"{e}.{name}"]
    if e == "grad_acc":
        return BOUNDS["grad_acc.f16" if case.p.get("f16") else "grad_acc.f32"]
    return BOUNDS[e]


def single_key_zero_bound(case):
    """Element-wise absolute bounds {"dq", "dk"} for an attention_bwd case whose every query item lists ONE kv item of ONE key (bwd_cases.py, `zero`): the true
    gradients are zero; what a kernel may leave is the difference of dP = sum_d dO16_d V_d and delta = sum_d dO16_d O_d (O = V) summed in two orders,
    |dS| <= E_q = 2 (dh - 1) 2^-24 sum_d |dO16_d V_d|, carried into dQ = scale dS k and dK = scale sum_q dS_q q_q; 1 + 2^-9 covers the fp16 rounding of dS
    and the fp32 accumulation of the products."""
    p = case.p
    assert p["nk"] == 1 and all(len(r) == 1 for r in p["table"])
    t = bwd_cases.build(case)
    heads, dh, nq = p["heads"], p["dh"], p["nq"]
    scale = p.get("scale") or dh ** -0.5
    do16 = t["dout"].half().double().reshape(-1, nq, heads, dh)
    q, k, v = t["q"].double().reshape(-1, nq, heads, dh), t["k"].double().reshape(-1, heads, dh), t["v"].double().reshape(-1, heads, dh)
    dq_b, dk_b = torch.zeros_like(q), torch.zeros_like(k)
    for it, (kit,) in enumerate(p["table"]):
        E = 2 * (dh - 1) * 2.0 ** -24 * (do16[it].abs() * v[kit].abs()).sum(-1, keepdim=True) * (1 + 2.0 ** -9)     # [nq, heads, 1]
        dq_b[it] = scale * E * k[kit].abs()
        dk_b[kit] += scale * (E * q[it].abs()).sum(0)
    C = heads * dh
    return {"dq": dq_b.reshape(-1, C), "dk": dk_b.reshape(-1, C)}


def _finite(case, who, name, g):
    assert bool(torch.isfinite(g.double()).all()), f"{case.id} {who}: {name} is not finite"


def _cmp_sumsq_absmax(case, who, name, g, w, want, device_types):
    """me_sumsq_absmax (include/motioned.h): a NaN anywhere -> both NaN, an inf -> both +inf, else the maximum exact and the sum inside its bound."""
    p = case.p
    if p.get("special") == "nan":
        assert bool(torch.isnan(g.double()).all()), f"{case.id} {who}: {name} = {g.tolist()} for an input that holds a NaN, want NaN"
    elif p.get("special"):
        assert float(g) == math.inf, f"{case.id} {who}: {name} = {g.tolist()} for an input that holds an inf, want +inf"
    elif name == "absmax":
        assert float(g) == float(w), f"{case.id} {who}: max |x| {float(g)} != {float(w)}"
    else:
        off = abs(float(g) / float(w) - 1.0)
        assert off <= BOUNDS["sumsq_absmax"][0], f"{case.id} {who}: sum of squares off by {off:.3e}"
        return off, 0.0


def _cmp_adamw(case, who, name, g, w, want, device_types):
    """p, m and v inside the entry point's bound; a non-finite gradient norm: bitwise what they were."""
    if case.p["clip"] in ("inf", "nan"):
        if name == "update":
            assert float(g.abs().max()) == 0.0
        else:
            assert bitwise_equal(g, w.to(g.dtype)), f"{case.id} {who}: {name} changed although the gradient norm was {case.p['clip']}"
        return None
    if name == "update":
        return None                                           # reported through p, m, v (the project's bound is stated on p)
    return _cmp_bounded(case, who, name, g, w, want, device_types)


def _cmp_zero(case, who, name, g, w):
    """An identically zero gradient: an absolute bound (single_key_zero_bound), nothing to divide by."""
    assert float(w.abs().max()) < 1e-12, f"{case.id}: the reference's {name} was meant to be zero"
    lim = single_key_zero_bound(case)[name]
    worst = float((g.double().abs() - lim).max())
    fig = (float(g.double().abs().max()), float(lim.max()))
    assert bool(torch.isfinite(g.double()).all()) and worst <= 0.0, f"{case.id} {who}: {name} should be zero, |{name}| reaches {fig[0]:.3e}, bound {fig[1]:.3e}"
    return fig


def _cmp_elementwise(case, who, name, g, w, rel_b, device_types):
    """rel-L2 inside the entry point's bound, every element inside the case's element-wise limit (bwd_cases.py, `elementwise=`); the elements the
    reference puts beyond fp16's range (`overflow`) must be +-inf of the right sign on the device and are left out of both figures."""
    keep = torch.ones_like(w, dtype=torch.bool)
    if case.p.get("overflow"):
        over, keep = w.abs() >= 65520.0, w.abs() < 65000.0
        assert int(over.sum()) >= 2
        if device_types:
            assert bool((g.double()[over] == torch.sign(w[over]) * math.inf).all()), f"{case.id} {who}: fp16 overflow must give +-inf of the right sign"
    _finite(case, who, name, g[keep])
    lim = bwd_cases.elementwise_limit(case, w)
    r = errors(g.double()[keep], w[keep])[0]
    excess = float(((g.double() - w.double()).abs() - lim)[keep].max())
    assert r <= rel_b and excess <= 0.0, f"{case.id} {who}: {name} rel-L2 {r:.3e} (<= {rel_b}), worst excess over the element-wise limit {excess:.3e} (<= 0)"
    return r, excess


def _cmp_bounded(case, who, name, g, w, want, device_types):
    """The default: rel-L2 and max / mean inside the bound of the entry point (or of the case, where it states one)."""
    if name in case.p.get("zero", ()):
        return _cmp_zero(case, who, name, g, w)
    if name == "lse":
        assert float((g.double() - w.double()).abs().max()) < 2e-2, f"{case.id} {who}: log-sum-exp stashed by the forward"
        return None
    rel_b, mx_b = bound_of(case, name)
    if rel_b == 0.0 and mx_b == 0.0:                          # exact: every value equal (torch.equal, as the existing tests: a selected-away -0.0 equals 0.0)
        assert torch.equal(g.float(), w.float()), f"{case.id} {who}: {name} is not exactly the reference"
        return None
    if case.elementwise:
        return _cmp_elementwise(case, who, name, g, w, rel_b, device_types)
    _finite(case, who, name, g)
    r, m = errors(g, w)
    assert r <= rel_b and m <= mx_b, f"{case.id} {who}: {name} rel-L2 {r:.3e} (<= {rel_b}), max/mean {m:.3e} (<= {mx_b})"
    return r, m


COMPARATORS = {"sumsq_absmax": _cmp_sumsq_absmax, "adamw": _cmp_adamw}      # entry -> its rule; every other entry: _cmp_bounded


def compare(case, got, want, who="", device_types=True):
    """Assert `got` (a run of the case) against `want` (the fp64 reference's run) inside the entry point's bound; returns {name: (rel-L2, max / mean)}.
    device_types: `got` comes from the HIP library (fp16 outputs, +-inf on fp16 overflow); False for the fp32 emulation, which keeps fp32."""
    figures = {}
    assert set(got) == set(want), (case.id, sorted(got), sorted(want))
    rule = COMPARATORS.get(case.entry, _cmp_bounded)
    for name in sorted(want):
        g, w = got[name], want[name]
        assert tuple(g.shape) == tuple(w.shape), (case.id, name, tuple(g.shape), tuple(w.shape))
        if name.startswith("outside."):
            assert bitwise_equal(g, w.to(g.dtype)), f"{case.id} {who}: {name} -- memory outside the view was written"
            continue
        fig = rule(case, who, name, g, w, want, device_types)
        if fig is not None:
            figures[name] = fig
    return figures


# ---------------------------------------------------------------------------------------------------------------- the trainers' skipped-step rule
def training_clip(rank, f=8, h=8):
    """One small training clip (latents, noise, text rows, adapter residuals, timestep), fp16-representable, seeded by rank."""
    from motioneditor_amd import synth
    g = torch.Generator().manual_seed(1000 + rank)
    r16 = lambda x: x.half().float()   # noqa: E731
    sizes = [h // (1 << (i // 3)) for i in range(12)]
    return dict(noisy=r16(torch.randn(1, 4, f, h, h, generator=g)), noise=r16(torch.randn(1, 4, f, h, h, generator=g)),
                ehs=r16(torch.randn(1, 77, 768, generator=g) * 0.3),
                down=[r16(torch.randn(1, c, f, sizes[i], sizes[i], generator=g) * 0.3) for i, c in enumerate(synth.ADAPTER_CH)],
                mid=r16(torch.randn(1, 1280, f, h // 8, h // 8, generator=g) * 0.3), t=501 - 100 * rank)


def poison_next_bucket(monkeypatch, backend, tr):
    """The trainer's next gradient bucket holds an inf when its norm is taken: written into the buffer from here, not by overflowing anything."""
    real = backend.sumsq_absmax
    state = {"armed": True, "calls": 0}

    def sumsq_absmax(x, out=None):
        if x.data_ptr() == tr.grad.data_ptr():
            state["calls"] += 1
            if state["armed"]:
                state["armed"] = False
                x[x.numel() // 3] = float("inf")
        return real(x, out) if out is not None else real(x)
    monkeypatch.setattr(backend, "sumsq_absmax", sumsq_absmax)
    return state


def packed_weights(tr):
    """The packed weights the forward reads and the trainer rewrites: the adapter trainer's one flat tensor, the tuner's packed tensors that hold a trained row."""
    if hasattr(tr, "weights"):
        return [tr.weights]
    return [tr.unet.P.cache[key] for key in sorted({s[0] for s in tr.slots})]


def assert_skipped_then_updates(tr, step, state):
    live = lambda: [tr.master, tr.m, tr.v] + packed_weights(tr)    # noqa: E731
    before = [t.clone() for t in live()]
    loss = step()
    assert math.isfinite(loss) and tr.skipped_steps == 1 and tr.steps == 0 and state["calls"] == 1
    for i, (a, b) in enumerate(zip(before, live())):
        assert bitwise_equal(a, b), f"{('master', 'm', 'v')[i] if i < 3 else 'packed weights'} changed in a step whose gradient bucket held an inf"
    step()                                                   # the next, clean step updates as usual
    assert tr.skipped_steps == 1 and tr.steps == 1 and state["calls"] == 2
    assert bool(torch.isfinite(tr.master).all()) and bool(torch.isfinite(tr.m).all()) and bool(torch.isfinite(tr.v).all())
    assert not torch.equal(before[0], tr.master) and float(tr.v.abs().max()) > 0
    assert any(not bitwise_equal(a, b) for a, b in zip(before[3:], live()[3:])), "the clean step left the packed weights alone"


def kernel_matches(got: str, want: str) -> bool:
    return fnmatch.fnmatchcase(got, want)
