"""TEST INFRASTRUCTURE: runs a case of tests/aux_cases.py on a backend and compares two runs, on tests/bwd_run.py's errors / bitwise_equal / kernel_matches / compare rules.

A backend is the HIP library (``motioneditor_amd.ops``: recognised by its ``capi``), the fp64 reference (tests/ref64_aux.py), the fp32 emulation (``Emu``: tests/emu_tune_ops.py
and tests/emu_clip_ops.py, extended below where a form is missing) or a deliberately wrong variant of the latter (tests/test_aux_sweep_cpu.py).  An ``Exchange`` says how
tensors reach the backend: ``dev`` moves an input, ``out`` hands an output view [rows, cols] of row pitch cols + pad, ``inout`` an operand that is accumulated into or
rewritten in place.  On the device (tests/test_aux_sweep_gpu.py) the last two are guard-banded views of tests/guard.py; entry points whose ops wrapper allocates its own
output are then called through the C ABI, so that the output is such a view too.  ``run`` returns {output name: CPU tensor}; accumulating entries return the INCREMENT,
strided outputs their untouched surroundings under ``outside.*``."""
from __future__ import annotations

import ctypes
import dataclasses

import torch

import aux_cases as ac
import bwd_run as br
import emu_clip_ops
import emu_tune_ops
import guard
from bwd_run import bitwise_equal, errors, kernel_matches, to_like  # noqa: F401

F16, F32, F64 = torch.float16, torch.float32, torch.float64


class Exchange:
    def __init__(self, dev, out, inout):
        self.dev, self.out, self.inout = dev, out, inout


def _plain_out(computed):
    """An output on the CPU: a COMPUTED one in the backend's precision (fp32 emulation, fp64 reference), a copied one in its own dtype."""
    def out(rows, cols, dtype, pad=0, computed_=True):
        dt = (computed or dtype) if computed_ else dtype
        return torch.full((rows, cols + pad), 5.0, dtype=dt)[:, :cols]
    return out


EMU = Exchange(lambda t: t.clone(), _plain_out(F32), lambda t: t.clone())
REF = Exchange(br.to_ref, _plain_out(F64), lambda t: t.double() if t.dtype == F32 else t.clone())


class Emu(br.Emu):
    """The fp32 emulation of the swept entry points: tests/emu_tune_ops.py (gemm_dw(conv=...), groupnorm_bwd(dgamma=, dbeta=), the refresh) and tests/emu_clip_ops.py
    (quick_gelu, embed_rows, attention_causal); embed_rows gets the zero row of an out-of-range id, which the device contract adds to the wrapper's."""
    name = "emu"

    def __getattr__(self, n):
        return getattr(emu_clip_ops, n) if hasattr(emu_clip_ops, n) and n in ("quick_gelu", "attention_causal") else getattr(emu_tune_ops, n)

    def embed_rows(self, tok, pos, ids, seq):
        ok = (ids >= 0) & (ids < tok.shape[0])
        y = emu_clip_ops.embed_rows(tok, pos, ids.clamp(0, tok.shape[0] - 1), seq)
        return torch.where(ok.reshape(-1, 1), y, torch.zeros((), dtype=y.dtype))

    def refresh(self, entries):
        """entries: the dicts of aux_cases.build with `dst` / `colsum` / `cvec` to rewrite in place."""
        tab = []
        for d in entries:
            if d["kind"] == "ups4":
                tab.append((d["master"], d["dst"], None, None, None, None, None))
            else:
                K = d["K"]
                tab.append((d["master"][:, :K], d["dst"][:, :K], d.get("gamma"), d.get("beta"), d.get("bias"), d.get("colsum"), d.get("cvec")))
        emu_tune_ops.refresh_weights(emu_tune_ops.refresh_table(tab))


def _cpu(t):
    return t.detach().cpu()


def _conv(p):
    return (p["Hin"], p["Win"], *ac.conv_out(p["Hin"], p["Win"], p["stride"], p["ups"]), p["stride"], p["ups"])


def copy_blocks_strides(p):
    """(ys0, ys1, xs0, xs1) of a copy_blocks case: the frame <-> pixel reorder of test_copy_blocks_is_the_frame_pixel_reorder (n0 = R, n1 = BF, rows = Ns)."""
    n0, n1, rows = p["n0"], p["n1"], p["rows"]
    if p.get("order") == "to-frame":
        return rows, n0 * rows, n1 * rows, rows
    return n1 * rows, rows, rows, n0 * rows


def run(case, B, t, X, hook=None, dev_params=False):
    """Run `case` with inputs `t` (aux_cases.build) on backend B through the exchange X.  hook(): called after the launch under test (the GPU test reads me_last_kernel
    there).  dev_params: the _dev variant of a step-scalar entry (HIP only): the scalars come from a device-resident [t, guidance, ca, cb]."""
    p, e = case.p, case.entry
    hook = hook or (lambda: None)
    hip = hasattr(B, "capi")
    L, st = (B.capi.lib(), B._stream()) if hip else (None, None)

    def chk(rc, name):
        B.capi.check(rc, name)
        hook()

    if e == "conv_dw":
        N, K, M = p["N"], p["K"], p["M"]
        dy, x, dst = X.dev(t["dy"])[:, :N], X.dev(t["x"])[:, :K], X.inout(t["base"])
        B.gemm_dw(dy, x, dst=dst, taps=9, K=K, M=M, alpha=p.get("alpha", 1.0), conv=_conv(p))
        hook()
        return {"dw": _cpu(dst) - to_like(t["base"], dst)}
    if e == "gn_params":
        C, rpg, groups, alpha = p["C"], p["rpg"], p["groups"], p.get("alpha", 1.0)
        x, dy, gamma, beta = X.dev(t["x"])[:, :C], X.dev(t["dy"])[:, :C], X.dev(t["gamma"]), X.dev(t["beta"])
        dg = X.inout(t["dgamma"]) if p.get("only") != "dbeta" else None
        db = X.inout(t["dbeta"]) if p.get("only") != "dgamma" else None
        kw = dict(rows_per_group=rpg, eps=1e-5, silu=p["silu"], groups=groups)
        if hip and alpha != 1.0:                                 # ops.groupnorm_bwd passes alpha = 1: the C ABI directly
            rows = x.shape[0]
            work = B._work(L.me_groupnorm_bwd_params_work_bytes(rows, rpg, C, groups), x.device, "gnp")
            chk(L.me_groupnorm_bwd_params(B._p(dg), B._p(db), x.data_ptr(), x.stride(0), gamma.data_ptr(), beta.data_ptr(), dy.data_ptr(), dy.stride(0), rows, rpg, C, groups, 1e-5,
                                          1 if p["silu"] else 0, alpha, work.data_ptr(), st), "me_groupnorm_bwd_params")
        elif hip:
            B.groupnorm_bwd(x, gamma, beta, dy, dgamma=dg, dbeta=db, **kw)
            hook()
        else:                                                    # the emulation / reference accumulate the plain gradient: alpha applied here
            zg, zb = (None if d is None else torch.zeros_like(d) for d in (dg, db))
            B.groupnorm_bwd(x, gamma, beta, dy, dgamma=zg, dbeta=zb, **kw)
            for d, z in ((dg, zg), (db, zb)):
                if d is not None:
                    d += alpha * z
        res = {}
        if dg is not None:
            res["dgamma"] = _cpu(dg) - to_like(t["dgamma"], dg)
        if db is not None:
            res["dbeta"] = _cpu(db) - to_like(t["dbeta"], db)
        return res
    if e == "refresh":
        return _run_refresh(case, B, t, X, hook)
    if e == "conv_small":
        Cin, Cout, n_img, H, W = p["Cin"], p["Cout"], p["n_img"], p["H"], p["W"]
        inp, w, bias = X.dev(t["inp"]), X.dev(t["w"]), None if t["bias"] is None else X.dev(t["bias"])
        if not hip:
            return {"y": _cpu(B.conv_small(inp, w, bias, n_img=n_img, Cin=Cin, H=H, Wd=W, silu=bool(p.get("silu")), **t["geo"]))}
        out = X.out(n_img * H * W, Cout, F16)
        a = B.capi.ConvSmallArgs()
        a.inp, a.W, a.bias, a.out = inp.data_ptr(), w.data_ptr(), B._p(bias), out.data_ptr()
        a.n_img, a.Cin, a.Cout, a.H, a.Wd = n_img, Cin, Cout, H, W
        a.img_stride, a.ch_stride, a.frames, a.frame_stride = t["geo"]["img_stride"], t["geo"]["ch_stride"], t["geo"].get("frames", 0), t["geo"].get("frame_stride", 0)
        a.in_is_f16, a.silu = 1 if inp.dtype == F16 else 0, 1 if p.get("silu") else 0
        chk(L.me_conv_small(ctypes.byref(a), st), "me_conv_small")
        return {"y": _cpu(out)}
    if e == "axpy_rows":
        rows, cols = p["rows"], p["cols"]
        x, a_ = X.dev(t["x"])[:, :cols], X.dev(t["a"])[:, :cols]
        if p.get("inplace"):                                     # Y is X: computed in the input's own precision
            base = X.inout(t["x"])
            y = base[:, :cols]
            B.axpy_rows(y, y, a_, p["alpha"])
            hook()
            got = _cpu(base)
            return {"y": got[:, :cols], "outside.right": got[:, cols:]}
        y = X.out(rows, cols, F16, p.get("y_pad", 0))
        B.axpy_rows(y, x, a_, p["alpha"])
        hook()
        return {"y": _cpu(y)}
    if e == "copy_rows":
        cols = p["cols"]
        y = X.out(p["rows"], cols, F16, p.get("y_pad", 0), False)
        B.copy_rows(y, X.dev(t["x"])[:, :cols])
        hook()
        return {"y": _cpu(y)}
    if e == "copy_blocks":
        n0, n1, rows, cols = p["n0"], p["n1"], p["rows"], p["cols"]
        ys0, ys1, xs0, xs1 = copy_blocks_strides(p)
        y = X.out(n0 * n1 * rows, cols, F16, p.get("y_pad", 0), False)
        B.copy_blocks(y, X.dev(t["x"])[:, :cols], n0, n1, rows, ys0=ys0, ys1=ys1, xs0=xs0, xs1=xs1)
        hook()
        return {"y": _cpu(y)}
    if e in ("silu", "relu", "quick_gelu"):
        n = p["n"]
        if not hip:
            return {"y": _cpu(getattr(B, e)(X.dev(t["x"])))}
        x = X.inout(t["x"]) if p.get("inplace") else X.dev(t["x"])
        y = x if p.get("inplace") else X.out(1, n, F16).reshape(-1)
        chk(getattr(L, "me_" + e)(y.data_ptr(), x.data_ptr(), n, st), "me_" + e)
        return {"y": _cpu(y).reshape(-1)}
    if e == "embed_rows":
        tok, pos, ids = X.dev(t["tok"]), X.dev(t["pos"]), X.dev(t["ids"])
        if not hip:
            return {"y": _cpu(B.embed_rows(tok, pos, ids, p["seq"]))}
        out = X.out(p["rows"], p["C"], F16, 0, False)
        chk(L.me_embed_rows(out.data_ptr(), tok.data_ptr(), pos.data_ptr(), ids.data_ptr(), p["rows"], p["seq"], p["C"], p["vocab"], st), "me_embed_rows")
        return {"y": _cpu(out)}
    if e == "timestep_embed":
        rows, dim = p["rows"], p["dim"]
        if not hip:
            return {"y": _cpu(B.timestep_embed(rows, dim, p["t"], "cpu"))}
        out = X.out(rows, dim, F16)
        if dev_params:
            sp = torch.tensor([p["t"], 0.0, 0.0, 0.0], dtype=F32, device=out.device)
            chk(L.me_timestep_embed_dev(out.data_ptr(), rows, dim, sp.data_ptr(), st), "me_timestep_embed_dev")
        else:
            chk(L.me_timestep_embed(out.data_ptr(), rows, dim, p["t"], st), "me_timestep_embed")
        return {"y": _cpu(out)}
    if e == "cfg_ddim":
        nb, C, f, h, w = p["nb"], p["C"], p["f"], p["h"], p["w"]
        lat, eps = X.dev(t["lat"]), X.dev(t["eps"])[:, :C]
        if not hip:
            return {"y": _cpu(B.cfg_ddim(lat, eps, guidance=p["guidance"], ca=t["ca"], cb=t["cb"])).reshape(nb * C, -1)}
        out = X.out(nb * C, f * h * w, F32)
        if dev_params:
            sp = torch.tensor([0.0, p["guidance"], t["ca"], t["cb"]], dtype=F32, device=out.device)
            chk(L.me_cfg_ddim_dev(out.data_ptr(), lat.data_ptr(), eps.data_ptr(), eps.stride(0), nb, C, f, h * w, sp.data_ptr(), st), "me_cfg_ddim_dev")
        else:
            chk(L.me_cfg_ddim(out.data_ptr(), lat.data_ptr(), eps.data_ptr(), eps.stride(0), nb, C, f, h * w, p["guidance"], t["ca"], t["cb"], st), "me_cfg_ddim")
        return {"y": _cpu(out)}
    if e == "gaussian_sample":
        n_img, npix, scale = p["n_img"], p["npix"], p.get("scale", 1.0)
        mom, noise = X.dev(t["mom"])[:, :8], X.dev(t["noise"])
        if not hip:
            return {"y": _cpu(B.gaussian_sample(mom, noise, n_img, npix, scale)).reshape(n_img * 4, npix)}
        out = X.out(n_img * 4, npix, F32)
        chk(L.me_gaussian_sample(out.data_ptr(), mom.data_ptr(), mom.stride(0), noise.data_ptr(), n_img, npix, scale, st), "me_gaussian_sample")
        return {"y": _cpu(out)}
    if e == "nchw_to_rows":
        n_img, C, npix = p["n_img"], p["C"], p["npix"]
        x = X.dev(t["x"])
        if not hip:
            return {"y": _cpu(B.nchw_to_rows(x, n_img, C, npix, t["img_stride"], t["ch_stride"]))}
        out = X.out(n_img * npix, C, F16, p.get("y_pad", 0))
        chk(L.me_nchw_to_rows(out.data_ptr(), out.stride(0), x.data_ptr(), t["img_stride"], t["ch_stride"], n_img, C, npix, st), "me_nchw_to_rows")
        return {"y": _cpu(out)}
    if e == "rows_to_nchw":
        n_img, C, npix = p["n_img"], p["C"], p["npix"]
        x = X.dev(t["x"])[:, :C]
        if not hip:
            return {"y": _cpu(B.rows_to_nchw(x, n_img, C, npix)).reshape(n_img * C, npix)}
        chs = npix + p.get("ch_pad", 0)                          # strided planes: image i, channel c at i * img_stride + c * ch_stride of the output
        ims = C * chs + p.get("img_pad", 0)
        base = X.out(n_img, ims, F32)
        chk(L.me_rows_to_nchw(base.data_ptr(), base.stride(0), chs, x.data_ptr(), x.stride(0), n_img, C, npix, st), "me_rows_to_nchw")
        got = _cpu(base)
        planes = torch.stack([got[:, c * chs:c * chs + npix] for c in range(C)], dim=1)
        gaps = torch.cat([got[:, c * chs + npix:(c + 1) * chs] for c in range(C)] + [got[:, C * chs:]], dim=1)
        assert bool((guard.bits(gaps) == guard._signed(guard.SENTINEL[F32], F32)).all()), f"{case.id}: the gaps between the planes were written"
        return {"y": planes.reshape(n_img * C, npix)}
    if e == "attention_causal":
        nq, heads, n_seq = p["nq"], p["heads"], p["n_seq"]
        C = heads * 64
        qkv = t["qkv"]
        if p.get("separate"):                                    # three tensors with pitches of their own
            q, k, v = (X.dev(bc_wide(qkv[:, i * C:(i + 1) * C], 8 * (i + 1)))[:, :C] for i in range(3))
        else:                                                    # column views of one fused [rows, 3 C] tensor, as the encoder passes them
            d = X.dev(qkv)
            q, k, v = d[:, :C], d[:, C:2 * C], d[:, 2 * C:]
        kw = dict(heads=heads, dh=64, n_seq=n_seq, nq=nq)
        if p.get("scale"):
            kw["scale"] = p["scale"]
        if not hip:
            return {"o": _cpu(B.attention_causal(q, k, v, **kw))}
        out = X.out(n_seq * nq, C, F16, p.get("o_pad", 0))
        chk(L.me_attn_causal(out.data_ptr(), out.stride(0), q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), n_seq, heads, 64, nq,
                             p.get("scale") or 0.125, st), "me_attn_causal")
        return {"o": _cpu(out)}
    raise KeyError(e)


def bc_wide(tt, pad):
    return ac._wide(tt.contiguous(), pad, fill=float("nan"))


def _run_refresh(case, B, t, X, hook):
    hip = hasattr(B, "capi")
    live, res = [], {}
    for d in t["entries"]:
        e = dict(d)
        for n in ("master", "gamma", "beta", "bias"):
            if e.get(n) is not None:
                e[n] = X.dev(d[n]) if hip else d[n].clone()
        for n in ("dst", "colsum", "cvec"):
            if e.get(n) is not None:
                e[n] = X.inout(d[n]) if hip else d[n].clone()
        live.append(e)
    if hip:
        tab = []
        for e in live:
            if e["kind"] == "ups4":
                tab.append((e["master"], e["dst"], None, None, None, None, None))
            else:
                K = e["K"]
                tab.append((e["master"][:, :K], e["dst"][:, :K], e.get("gamma"), e.get("beta"), e.get("bias"), e.get("colsum"), e.get("cvec")))
        B.refresh_weights(B.refresh_table(tab))
        hook()
    elif hasattr(B, "refresh"):
        B.refresh(live)
    else:                                                        # the reference: every entry from its own fp32 values
        for e in live:
            r = B.refresh_entry(e)
            if e["kind"] == "ups4":
                e["dst"] = r["w"]
            else:
                e["dst"][:, :e["K"]] = r["w"]
                if "colsum" in r:
                    e["colsum"], e["cvec"] = r["colsum"], r["cvec"]
    for i, e in enumerate(live):
        got = _cpu(e["dst"])
        if e["kind"] == "ups4":
            res[f"w{i}"] = got
            continue
        res[f"w{i}"], res[f"outside.w{i}"] = got[:, :e["K"]], got[:, e["K"]:]
        if e["kind"] != "plain":
            res[f"colsum{i}"], res[f"cvec{i}"] = _cpu(e["colsum"]), _cpu(e["cvec"])
    return res


def refresh_vector_bound(case, t):
    """Per-row absolute bounds of the colsum / cvec of a refresh case, as tests/test_bg_train_gpu.py test_refresh_kernel_matches_ln_fold states them: the fp32
    round-off of a K-term sum taken in another order, 1e-5 times the row's sum of magnitudes (of the rounded W' for colsum, of master * beta for cvec; + |bias|)."""
    out = {}
    for i, d in enumerate(t["entries"]):
        if d["kind"] in ("fold", "fold+bias"):
            m = d["master"][:, :d["K"]].double()
            out[f"colsum{i}"] = 1e-5 * (m.float() * d["gamma"][None, :]).half().double().abs().sum(dim=1)
            out[f"cvec{i}"] = 1e-5 * ((m * d["beta"].double()).abs().sum(dim=1) + (d["bias"].double().abs() if d.get("bias") is not None else 0.0))
    return out


def compare(case, got, want, who="", device_types=True, t=None):
    """bwd_run.compare with the bounds of tests/aux_cases.py: rel-L2 and max / mean inside the entry point's bound (exact where it says (0, 0); per element where the
    case names an elementwise= limit); `outside.*` bitwise; the refresh vectors inside refresh_vector_bound.  Returns {name: (rel-L2, max / mean)}."""
    figures = {}
    assert set(got) == set(want), (case.id, sorted(got), sorted(want))
    vec = refresh_vector_bound(case, t if t is not None else ac.build(case)) if case.entry == "refresh" else {}
    for name in sorted(want):
        g, w = got[name], want[name]
        assert tuple(g.shape) == tuple(w.shape), (case.id, name, tuple(g.shape), tuple(w.shape))
        if name.startswith("outside."):
            assert bitwise_equal(g, w.to(g.dtype)), f"{case.id} {who}: {name} -- memory outside the view was written"
            continue
        if name in vec:
            worst = float(((g.double() - w.double()).abs() - vec[name]).max())
            assert bool(torch.isfinite(g.double()).all()) and worst <= 0.0, f"{case.id} {who}: {name} beyond 1e-5 of its row's sum of magnitudes by {worst:.3e}"
            continue
        if case.p.get("saturating"):                             # finite everywhere, and exact where the formula says x or 0
            assert bool(torch.isfinite(g.double()).all()), f"{case.id} {who}: a saturating input gave a non-finite result"
            big = w.double().abs() >= 60000.0
            assert torch.equal(g.double()[big], w.double()[big]) and bool((g.double()[w.double() == 0.0] == 0.0).all()), f"{case.id} {who}: x -> x / x -> 0 not exact at +-65504 / +-0"
        fig = br._cmp_bounded(dataclasses.replace(case, bound=ac.bound_of(case, name)), who, name, g, w, want, device_types)
        if fig is not None:
            figures[name] = fig
    return figures


# ---------------------------------------------------------------------------------------------------------------- refused calls (tests/fwd_refused.py's shape)
def refused(capi):
    """(entry point, make, bad) as tests/fwd_refused.py's tables: make(ptr) builds the arguments of a VALID call from ptr(name, bytes) -> address; bad lists
    (label, change(arguments, ptr), needle of the refusal message), from aux_cases.CONV_DW_REFUSED / CAUSAL_REFUSED.  No violating call is ever launched."""
    from types import SimpleNamespace

    def change_of(over):
        def change(a, ptr):
            for k, v in over.items():
                if k.endswith("_off"):
                    setattr(a, k[:-4], getattr(a, k[:-4]) + v)
                else:
                    setattr(a, k, v)
        return change

    def conv_dw(ptr):
        a = capi.ConvDwArgs()
        a.M, a.N, a.K, a.lddy, a.ldx, a.dy_is_f16 = 70, 40, 72, 40, 72, 0
        a.Hin, a.Win, a.Hout, a.Wout, a.stride, a.ups, a.pad0, a.alpha = 5, 7, 5, 7, 1, 0, 0, 1.0
        a.dY, a.X, a.dW, a.work = ptr("dy", 280 * 40 * 4), ptr("x", 280 * 72 * 2), ptr("dw", 40 * 9 * 72 * 4), ptr("work", 2 * 40 * 9 * 72 * 4)
        return a

    def causal(ptr):
        n = 16 * 192 * 2
        return SimpleNamespace(O=ptr("o", n), ldo=64, Q=ptr("qkv", n), ldq=192, K=ptr("qkv", n) + 128, ldk=192, V=ptr("qkv", n) + 256, ldv=192, n_seq=1, heads=1, dh=64, nq=16, scale=0.125)

    yield "me_conv_dw", conv_dw, [(label, change_of(over), needle) for label, over, needle in ac.CONV_DW_REFUSED]
    yield "me_attn_causal", causal, [(label, change_of(over), needle) for label, over, needle in ac.CAUSAL_REFUSED]


def call_refused(L, entry, a):
    if entry == "me_attn_causal":
        return L.me_attn_causal(a.O, a.ldo, a.Q, a.ldq, a.K, a.ldk, a.V, a.ldv, a.n_seq, a.heads, a.dh, a.nq, a.scale, None)
    return getattr(L, entry)(ctypes.byref(a), None)
