"""The backward / training sweep without a GPU: the case table of tests/bwd_cases.py against itself, the fp32 emulation against the fp64 reference,
a set of deliberately wrong emulations against the table, the Python restatement of the launch geometry against the library's host functions, and the
non-finite contract of the trainers on the emulated backend.

Production-only cases (fp64 reference too slow here, left to tests/test_bwd_sweep_gpu.py): none -- the production-size cases take seconds and run here too."""
import math

import pytest
import torch

import bwd_cases as bc
import bwd_run as br
import emu_ops
import ref64_bwd as ref

PROD_ONLY = ()
_REF = {}


def ref_run(case, t):
    hit = _REF.get(case.id)
    if hit is None:
        hit = br.run(case, ref, t, br.to_ref)
        if sum(v.numel() for v in hit.values()) < 4_000_000:
            _REF[case.id] = hit
    return hit


# ------------------------------------------------------------------------------------------------------------------ the table itself
def test_case_ids_are_unique_and_production_only_cases_are_declared():
    ids = [c.id for c in bc.CASES]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)
    assert all(i in bc.BY_ID and i in __doc__ for i in PROD_ONLY) and len({bc.BY_ID[i].entry for i in PROD_ONLY}) == len(PROD_ONLY)   # at most one per entry point
    print("cases per entry point:", bc.case_counts(), "total", len(bc.CASES))


def _entry_checks(case, t):
    """The argument checks of the case's me_* entry point (include/motioned.h, the launchers in csrc/), restated on the case's tensors."""
    p, e = case.p, case.entry
    m8 = lambda *v: all(x % 8 == 0 for x in v)    # noqa: E731
    m4 = lambda *v: all(x % 4 == 0 for x in v)    # noqa: E731
    if e == "gemm_dw":
        assert p["M"] > 0 and m8(p["N"], p["K"], t["x"].shape[1]) and t["dy"].shape[1] % (8 if p.get("dy16") else 4) == 0
        if p.get("tconv"):
            frames, npix, chunk = p["tconv"]
            assert min(frames, npix, chunk) > 0 and p["M"] % (frames * npix) == 0
        assert bc.dw_work_bytes(p["M"], p["N"], p["K"]) > 0
    elif e == "gemm_dx":
        assert m8(p["K"]) and (p["N"] % 8 == 0 or p["N"] == 4)            # ops._w_transposed pads N to 8
        if p.get("conv"):
            Hin, Win, Hout, Wout, stride, ups = p["conv"]
            assert (Hout, Wout) == ((Hin * (2 if ups else 1) - 1) // stride + 1, (Win * (2 if ups else 1) - 1) // stride + 1) and p["M"] % (Hout * Wout) == 0
        if p.get("tconv"):
            assert p["M"] % (p["tconv"][0] * p["tconv"][1]) == 0 and p["tconv"][0] % p["tconv"][2] == 0
    elif e == "attention_bwd":
        assert p["dh"] in (40, 80, 160) and 1 <= max(len(r) for r in p["table"]) <= 3 and m8(p["heads"] * p["dh"])
        assert all(-1 <= k < p["n_kv"] for r in p["table"] for k in r) and all(r[0] >= 0 for r in p["table"])
        named = {k for r in p["table"] for k in r[:([*r, -1].index(-1))]}
        assert set(p.get("unnamed", ())) == set(range(p["n_kv"])) - named
    elif e == "temporal_attention_bwd":
        assert 0 < p["frames"] <= 64 and p["dh"] in (40, 80, 160) and m8(p["heads"] * p["dh"])
        assert case.path == bc.tattn_bwd_path(p["frames"], p["dh"], p["heads"], aligned=not p.get("q_off")) is not None
        if case.path.startswith("tattn_bwd2"):
            assert bc.tattn_bwd2_lds(p["frames"], p["dh"]) <= 150 * 1024
    elif e == "groupnorm_bwd":
        assert p["C"] % 32 == 0 and m8(p["C"]) and p["C"] <= 2560 and p["rpg"] > 0 and p["nsg"] > 0
    elif e == "layernorm_bwd":
        assert p["rows"] > 0 and min(t["x"].shape[1], t["dy"].shape[1]) >= p["C"]
    elif e == "layernorm_bwd_params":
        assert p["rows"] > 0 and p["C"] <= 1536
    elif e == "geglu_bwd":
        assert p["N"] % 32 == 0 and p["M"] > 0
    elif e == "softmax_bwd_rows":
        assert m8(p["cols"], t["P"].shape[1], t["dP"].shape[1])
    elif e == "grad_acc":
        assert p.get("flat") or (m4(p["cols"], p["pad"], t["base"].shape[1], t["src"].shape[1]))
        assert (p["rows"] * p["cols"]) % 4 == 0 and (not p.get("pool") or p["rows"] % (p["pool"][0] * p["pool"][1]) == 0)
    elif e == "cast_rows_f16":
        assert m4(p["cols"], p["pad_cols"], p["off"], t["src"].shape[1]) and p["pad_cols"] >= p["cols"]
    elif e in ("adamw", "sumsq_absmax", "cast_f16"):
        assert p["n"] >= 1
    elif e == "colsum_grad":
        assert p["M"] > 0 and p["N"] > 0
    elif e in ("relu_bwd", "mse_seed"):
        pass
    else:
        raise AssertionError(f"no entry checks stated for {e}")


@pytest.mark.parametrize("case", bc.CASES, ids=lambda c: c.id)
def test_fp32_emulation_agrees_with_the_fp64_reference_inside_the_gpu_bound(case):
    """Every case satisfies its entry point's argument checks, and tests/emu_ops.py in fp32 lands inside the bound tests/test_bwd_sweep_gpu.py applies to the
    HIP kernel on the same inputs: the bound is reachable by fp32 accumulation there, and the new reference is pinned against the old one."""
    t = bc.build(case)
    _entry_checks(case, t)
    want = ref_run(case, t)
    got = br.run(case, br.Emu(), t, br.to_emu)
    figures = br.compare(case, got, want, who="fp32 emulation", device_types=False)
    print(case.id, {k: (f"{r:.2e}", f"{m:.2e}") for k, (r, m) in figures.items()})


def test_the_derived_edges_are_where_the_launch_code_changes():
    """The table sits on both sides of what it claims: the deciding clamp of dw_geometry, splits == 1, a one-row last split, a swallowed split, the 256 cap;
    the chunk floor / cap / single-chunk branches of gn_bwd_chunks and every ny of the apply pass; both temporal kernels at every head dim."""
    dw = [c for c in bc.CASES if c.entry == "gemm_dw"]
    geo = {c.id: bc.dw_geometry(c.p["M"], c.p["N"], c.p["K"]) for c in dw}
    assert {g[2] for g in geo.values()} == {"tiles", "stages", "cap256"}
    assert any(g[0] == 1 for g in geo.values()) and any(g[0] == 256 for g in geo.values()) and any(g[0] == 41 for g in geo.values())
    assert geo["dw-short-last-split"][:2] == (5, 128) and 513 - 4 * 128 == 1
    assert geo["dw-swallowed-split"][:2] == (40, 128)                          # the 41-split clamp, then 128-row splits cover 5000 rows in 40
    assert any(c.p["M"] % geo[c.id][1] for c in dw) and any(c.p["M"] % geo[c.id][1] == 0 for c in dw)
    for N, K, lim in bc.DW_EDGE_SHAPES:
        edges = bc.dw_edges(N, K, lim)
        assert len(edges) >= 8 and all(f"dw-edge-N{N}-K{K}-M{M}" in bc.BY_ID for M in edges)
    assert bc.dw_geometry(32768, 64, 64)[0] == 256 and bc.dw_geometry(32769, 64, 64)[:2] == (205, 160)   # the cap, then 160-row splits: 51 splits swallowed
    gn = [c.p for c in bc.CASES if c.entry == "groupnorm_bwd"]
    ch = [bc.gn_bwd_chunks(p["rpg"] * p["nsg"], p["rpg"]) + (p["rpg"],) for p in gn]
    assert any(c == 512 for c, _, _ in ch) and any(c == 1 and r > 1 for c, _, r in ch) and any(cr == 8 and r < 8 for _, cr, r in ch)
    assert any(r % cr for _, cr, r in ch) and any(r % cr == 0 and c > 1 for c, cr, r in ch) and any(cr > 8 for _, cr, _ in ch)
    assert bc.gn_bwd_chunks(2 * 4097, 4097) == (456, 9) and 4097 - 455 * 9 == 2
    assert {bc.gn_apply_grid(p["rpg"] * p["nsg"], p["C"])[0] for p in gn} == {1, 2}
    paths = {c.path for c in bc.CASES if c.entry == "temporal_attention_bwd"}
    assert paths == {"tattn_bwd_kernel", "tattn_bwd2_kernel<40,8>", "tattn_bwd2_kernel<80,4>", "tattn_bwd2_kernel<160,2>"}
    assert bc.tattn_bwd2_lds(32, 40) == 149_504 and bc.tattn_bwd_path(**{k: bc.TATTN_REFUSED[k] for k in ("frames", "dh", "heads")}) is None
    for dh in (40, 80, 160):
        assert {c.p["frames"] for c in bc.CASES if c.entry == "temporal_attention_bwd" and c.p["dh"] == dh and c.p["heads"] == 8} >= set(bc.TATTN_FRAMES) - ({64} if dh == 160 else set())


def test_geometry_restatement_matches_the_library_host_functions():
    """me_gemm_dw_work_bytes / me_groupnorm_bwd_scratch_bytes are host functions (no launch): the Python restatement that placed the edges is the library's."""
    from motioneditor_amd import capi
    L = capi.lib()
    shapes = [(c.p["M"], c.p["N"], c.p["K"]) for c in bc.CASES if c.entry == "gemm_dw"]
    shapes += [(M, N, K) for N, K in ((64, 64), (320, 320), (2560, 320), (8, 8)) for M in list(range(1, 700, 7)) + [32767, 32768, 32769, 40000, 393216]]
    for M, N, K in shapes:
        assert L.me_gemm_dw_work_bytes(M, N, K) == bc.dw_work_bytes(M, N, K), (M, N, K)
    assert L.me_gemm_dw_work_bytes(0, 64, 64) == 0
    gn = [(c.p["rpg"] * c.p["nsg"], c.p["rpg"]) for c in bc.CASES if c.entry == "groupnorm_bwd"]
    gn += [(nsg * rpg, rpg) for nsg in (1, 2, 3, 4, 1024, 1025) for rpg in (1, 7, 8, 9, 24, 25, 383, 384, 385, 4095, 4096, 4097, 9216)]
    for rows, rpg in gn:
        assert L.me_groupnorm_scratch_bytes(rows, rpg, 32) == bc.gn_fwd_scratch_bytes(rows, rpg, 32), (rows, rpg)
        assert L.me_groupnorm_bwd_scratch_bytes(rows, rpg, 32) == bc.gn_bwd_scratch_bytes(rows, rpg, 32), (rows, rpg)


# ------------------------------------------------------------------------------------------------------------------ deliberately wrong emulations
class DroppedLastSplit(br.Emu):
    """gemm_dw that never folds the last split of dw_geometry."""
    def gemm_dw(self, dy, x, *, M, **kw):
        s, rps, _ = bc.dw_geometry(M, dy.shape[1], kw["K"])
        dy = dy.clone()
        if s > 1:
            dy[(s - 1) * rps:M] = 0
        return super().gemm_dw(dy, x, M=M, **kw)


class AlphaIgnored(br.Emu):
    def gemm_dw(self, dy, x, *, alpha=1.0, **kw):
        return super().gemm_dw(dy, x, alpha=1.0, **kw)

    def gemm_dx(self, dy, w, *, alpha=1.0, **kw):
        return super().gemm_dx(dy, w, alpha=1.0, **kw)

    def grad_acc(self, dst, src, alpha=1.0, pool=None, store=False):
        return emu_ops.grad_acc(dst, src, 1.0, pool, store)

    def colsum_grad(self, dy, *, dst, alpha=1.0):
        return emu_ops.colsum_grad(dy, dst=dst, alpha=1.0)


class StoreInsteadOfAccumulate(br.Emu):
    def gemm_dw(self, dy, x, *, dst, **kw):
        dst.zero_()
        return super().gemm_dw(dy, x, dst=dst, **kw)

    def grad_acc(self, dst, src, alpha=1.0, pool=None, store=False):
        return emu_ops.grad_acc(dst, src, alpha, pool, True)

    def layernorm_bwd_params(self, x, dy, *, dgamma=None, dbeta=None, eps=1e-5):
        for d in (dgamma, dbeta):
            if d is not None:
                d.zero_()
        return emu_ops.layernorm_bwd_params(x, dy, dgamma=dgamma, dbeta=dbeta, eps=eps)


class CausalMaskOffByOneFrame(br.Emu):
    """temporal attention whose query frame i also sees key frame i + 1."""
    def temporal_attention_bwd(self, q, k, v, out, dout, *, heads, dh, batch, frames, npix, scale=None, **kw):
        scale = dh ** -0.5 if scale is None else scale
        C = heads * dh
        leaves = [t.detach().float().clone().requires_grad_(True) for t in (q, k, v)]
        qq, kk, vv = (t[:, :C].reshape(batch, frames, npix, heads, dh).permute(0, 2, 3, 1, 4) for t in leaves)
        s = (qq @ kk.transpose(-1, -2)) * scale
        s = s.masked_fill(torch.arange(frames)[None, :] > torch.arange(frames)[:, None] + 1, -math.inf)
        y = (s.softmax(-1) @ vv).permute(0, 3, 1, 2, 4).reshape(batch * frames * npix, C)
        return torch.autograd.grad(y, leaves, dout.float()[:, :C])


class DkFromTheLastNamerOnly(br.Emu):
    """attention_bwd whose dK of a kv item several query items list is the LAST lister's contribution instead of the sum."""
    def attention_bwd(self, q, k, v, out, dout, *, dq, dk, dv, lse=None, heads, dh, n_items, nq, nk, seg_item, seg_mode, scale=None, **kw):
        table = seg_item.tolist()
        dk0 = dk.clone()
        for it in range(n_items):
            one = torch.tensor([table[it]], dtype=torch.int32)
            gk = torch.zeros_like(dk)
            emu_ops.attention_bwd(q[it * nq:(it + 1) * nq], k, v, None, dout[it * nq:(it + 1) * nq], dq=dq[it * nq:(it + 1) * nq], dk=gk, dv=dv, heads=heads, dh=dh, n_items=1,
                                  nq=nq, nk=nk, seg_item=one, seg_mode=torch.zeros_like(one), **({} if scale is None else {"scale": scale}))
            for kit in {x for x in table[it] if x >= 0}:
                dk[kit * nk:(kit + 1) * nk] = dk0[kit * nk:(kit + 1) * nk] + gk[kit * nk:(kit + 1) * nk]


class StatisticsOverTheChunk(br.Emu):
    """groupnorm_bwd whose statistics span one row chunk of gn_bwd_chunks instead of the whole group."""
    def groupnorm_bwd(self, x, gamma, beta, dy, *, rows_per_group, **kw):
        chunks, cr = bc.gn_bwd_chunks(x.shape[0], rows_per_group)
        if chunks > 1 and rows_per_group % cr == 0:
            rows_per_group = cr
        return emu_ops.groupnorm_bwd(x, gamma, beta, dy, rows_per_group=rows_per_group, **kw)


class DgammaAsAMean(br.Emu):
    def layernorm_bwd_params(self, x, dy, *, dgamma=None, dbeta=None, eps=1e-5):
        g0 = None if dgamma is None else dgamma.clone()
        emu_ops.layernorm_bwd_params(x, dy, dgamma=dgamma, dbeta=dbeta, eps=eps)
        if dgamma is not None:
            dgamma.copy_(g0 + (dgamma - g0) / x.shape[0])


class AdamWithoutBiasCorrection(br.Emu):
    def adamw(self, p, m, v, g, *, step, **kw):
        return super().adamw(p, m, v, g, step=10 ** 9, **kw)       # beta ** step == 0: both corrections are 1


class AbsmaxDropsNaN(br.Emu):
    """max |x| reduced with fmaxf, as the kernel did before the contract was written down."""
    def sumsq_absmax(self, x, out=None):
        r = emu_ops.sumsq_absmax(x)
        r[1] = torch.where(torch.isnan(x), torch.zeros_like(x), x.abs()).max()
        return r


MUTANTS = {
    "a dropped last split in gemm_dw": (DroppedLastSplit, ("gemm_dw",)),
    "alpha ignored": (AlphaIgnored, ("gemm_dw", "gemm_dx", "grad_acc", "colsum_grad")),
    "store instead of accumulate": (StoreInsteadOfAccumulate, ("gemm_dw", "grad_acc", "layernorm_bwd_params")),
    "a causal mask off by one frame in tattn_bwd": (CausalMaskOffByOneFrame, ("temporal_attention_bwd",)),
    "dk of a kv item named twice taken from the last namer only": (DkFromTheLastNamerOnly, ("attention_bwd",)),
    "group statistics over chunk_rows instead of rows_per_group": (StatisticsOverTheChunk, ("groupnorm_bwd",)),
    "dgamma as a mean": (DgammaAsAMean, ("layernorm_bwd_params",)),
    "AdamW without bias correction": (AdamWithoutBiasCorrection, ("adamw",)),
    "absmax that drops NaN": (AbsmaxDropsNaN, ("sumsq_absmax",)),
}


def _cost(case):
    """A size figure from the parameters alone: the mutant search tries the small cases first."""
    p = case.p
    return p.get("M", 1) * p.get("N", 1) * p.get("K", 1) + p.get("n", 0) + p.get("rows", 0) * p.get("C", p.get("cols", 1)) + p.get("rpg", 0) * p.get("nsg", 0) * p.get("C", 0) \
        + p.get("nq", 0) * p.get("nk", 0) * 100 + p.get("frames", 0) * p.get("npix", 0) * 1000


@pytest.mark.parametrize("name", list(MUTANTS))
def test_a_deliberately_wrong_emulation_fails_at_least_one_case(name):
    """A mutant that passes every case of its entry points means the table is too weak there: extend the table, do not delete the mutant."""
    cls, entries = MUTANTS[name]
    caught = []
    for entry in entries:
        hit = None
        for case in sorted((c for c in bc.CASES if c.entry == entry and not c.prod), key=_cost):
            t = bc.build(case)
            try:
                br.compare(case, br.run(case, cls(), t, br.to_emu), ref_run(case, t), who=name, device_types=False)
            except AssertionError as exc:
                hit = (case.id, str(exc).splitlines()[0][:160])
                break
        assert hit is not None, f"mutant '{name}' passes every {entry} case"
        caught.append(hit)
    for cid, msg in caught:
        print(f"mutant '{name}' caught by case {cid}: {msg}")


# ------------------------------------------------------------------------------------------------------------------ the non-finite contract on the emulated backend
def test_loss_scale_trusts_a_finite_absmax_only():
    from motioneditor_amd import util
    assert util._loss_scale(float("nan")) == 1.0 and util._loss_scale(float("inf")) == 1.0 and util._loss_scale(0.0) == 1.0
    assert util._loss_scale(0.5) == 2.0 ** math.floor(math.log2(64.0 / 0.5))
    for special in (float("nan"), float("inf"), float("-inf")):
        x = torch.randn(1000)
        x[17] = special
        for backend in (emu_ops, ref):
            r = backend.sumsq_absmax(x)
            assert not math.isfinite(float(r[0])) and not math.isfinite(float(r[1])), (special, backend.__name__, r)
            assert math.isnan(float(r[1])) == math.isnan(special)


def test_adapter_trainer_skips_a_step_whose_bucket_holds_an_inf(monkeypatch, unet_sd_np):
    import emu_train_ops
    import motioneditor_amd.models.unet_2d_condition as u
    from motioneditor_amd import util
    from motioneditor_amd.models import graph
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    for m in (graph, u, util):
        monkeypatch.setattr(m, "ops", emu_train_ops)
    tr = util.AdapterTrainer(UNet2DConditionModel(unet_sd_np, device="cpu", dtype=torch.float32), lr=1e-3)
    c = br.training_clip(0)
    state = br.poison_next_bucket(monkeypatch, emu_train_ops, tr)
    br.assert_skipped_then_updates(tr, lambda: tr.step(c["noisy"], c["t"], c["ehs"], c["down"], c["mid"], c["noise"]), state)


def test_background_tuner_skips_a_step_whose_bucket_holds_an_inf(monkeypatch, unet_sd_np):
    import emu_train_ops
    import motioneditor_amd.models.unet_2d_condition as u
    from motioneditor_amd import util
    from motioneditor_amd.models import graph
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    for m in (graph, u, util):
        monkeypatch.setattr(m, "ops", emu_train_ops)
    tr = util.UNetTuner(UNet2DConditionModel(unet_sd_np, device="cpu", dtype=torch.float32), lr=1e-3)
    c = br.training_clip(1)
    state = br.poison_next_bucket(monkeypatch, emu_train_ops, tr)
    br.assert_skipped_then_updates(tr, lambda: tr.step(c["noisy"], c["t"], c["ehs"], c["noise"]), state)
