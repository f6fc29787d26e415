"""The third sweep without a GPU: the case table of tests/aux_cases.py against itself, the fp32 emulation against the fp64 reference of tests/ref64_aux.py inside the
bound the GPU file applies, the Python restatement of the launch geometry against the library's host functions and a brute-force scan, the refused calls on
fabricated addresses, and eighteen deliberately wrong emulations against the table.

Production-only cases (fp64 reference too slow here, left to tests/test_aux_sweep_gpu.py): none -- the production-size cases take seconds and run here too."""
import math

import pytest
import torch
import torch.nn.functional as F

import aux_cases as ac
import aux_run as ar
import emu_ops
import ref64_aux as ref

PROD_ONLY = ()
_REF = {}


def ref_run(case, t):
    hit = _REF.get(case.id)
    if hit is None:
        hit = ar.run(case, ref, t, ar.REF)
        if sum(v.numel() for v in hit.values()) < 4_000_000:
            _REF[case.id] = hit
    return hit


# ------------------------------------------------------------------------------------------------------------------ the table itself
def test_case_ids_are_unique_and_the_bound_protocol_stays_rare():
    ids = [c.id for c in ac.CASES]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)
    assert all(i in ac.BY_ID and i in __doc__ for i in PROD_ONLY)
    counts = ac.case_counts()
    for e, n in counts.items():
        assert sum(1 for c in ac.CASES if c.entry == e and c.prod) <= 1, f"{e}: at most one production-size case per entry point"
        assert 10 * sum(1 for c in ac.CASES if c.entry == e and c.bound is not None) <= n, f"{e}: more than one case in ten states a bound of its own"
    assert set(counts) == set(ac.ENTRIES) and all(ac.bound_of(c, "dgamma") for c in ac.CASES)
    print("cases per entry point:", counts, "total", len(ac.CASES))


def _entry_checks(case, t):
    """The argument checks of the case's me_* entry point (include/motioned.h, include/motioned_tune.h, the launchers in csrc/), restated on the case's tensors."""
    p, e = case.p, case.entry
    m8 = lambda *v: all(x % 8 == 0 for x in v)    # noqa: E731
    m4 = lambda *v: all(x % 4 == 0 for x in v)    # noqa: E731
    if e == "conv_dw":
        Hout, Wout = ac.conv_out(p["Hin"], p["Win"], p["stride"], p["ups"])
        assert p["M"] > 0 and m8(p["N"], p["K"], t["x"].shape[1]) and t["dy"].shape[1] % (8 if p.get("dy16") else 4) == 0 and t["x"].shape[1] >= p["K"] and t["dy"].shape[1] >= p["N"]
        assert p["ups"] in (0, 1) and p["stride"] in (1, 2) and not (p["stride"] == 2 and p["ups"]) and p["M"] % (Hout * Wout) == 0 and p["M"] // (Hout * Wout) == p["n_img"]
        assert p["N"] * 9 * p["K"] * 4 <= ac.CW_CAP and ac.cw_work_bytes(p["M"], p["N"], p["K"]) > 0
        assert case.twice == (ac.cw_geometry(p["M"], p["N"], p["K"])[0] > 1), "twice=True on every multi-split case"
    elif e == "gn_params":
        assert 1 <= p["groups"] <= 64 and p["C"] % p["groups"] == 0 and m8(p["C"], t["x"].shape[1]) and p["C"] <= 2560 and m4(t["dy"].shape[1]) and p["rpg"] > 0 and p["nsg"] > 0
    elif e == "refresh":
        assert (case.path is None) == all(d["kind"] != "ups4" for d in t["entries"])
        for d in t["entries"]:
            if d["kind"] == "ups4":
                assert d["master"].shape[1] == 9 and d["dst"].shape[1] == 16 and m4(d["master"].shape[2])
            else:
                assert m4(d["K"], d["master"].shape[1], d["dst"].shape[1]) and (d["kind"] == "plain") == ("gamma" not in d)
    elif e == "conv_small":
        assert p["Cin"] in (3, 4) and m8(p["Cout"]) and min(p["n_img"], p["H"], p["W"]) > 0 and case.path == ac.conv_small_target(p["Cin"], p["Cout"])
        assert not p.get("frames") or p["n_img"] % p["frames"] == 0
    elif e == "axpy_rows":
        assert m4(p["cols"], t["x"].shape[1], t["a"].shape[1], p.get("y_pad", 0)) and p["rows"] > 0
    elif e in ("copy_rows", "copy_blocks"):
        assert m8(p["cols"], t["x"].shape[1], p.get("y_pad", 0)) and p["rows"] > 0
    elif e in ("silu", "relu", "quick_gelu"):
        assert p["n"] > 0 and t["x"].numel() == p["n"]
    elif e == "embed_rows":
        assert m8(p["C"]) and p["rows"] % p["seq"] == 0 and t["pos"].shape[0] >= p["seq"]
        assert p.get("bad_ids") or (int(t["ids"].min()) == 0 and int(t["ids"].max()) == p["vocab"] - 1)
    elif e == "timestep_embed":
        assert p["dim"] % 2 == 0 and p["rows"] > 0
    elif e == "cfg_ddim":
        assert t["eps"].shape[1] >= p["C"] and t["eps"].shape[0] == 2 * p["nb"] * p["f"] * p["h"] * p["w"]
    elif e == "gaussian_sample":
        assert t["mom"].shape[1] >= 8
    elif e in ("nchw_to_rows", "rows_to_nchw"):
        assert min(p["n_img"], p["C"], p["npix"]) > 0
    elif e == "attention_causal":
        assert 0 < p["nq"] <= 128 and p["heads"] > 0 and p["n_seq"] > 0 and p.get("o_pad", 0) % 8 == 0
    else:
        raise AssertionError(f"no entry checks stated for {e}")


@pytest.mark.parametrize("case", ac.CASES, ids=lambda c: c.id)
def test_fp32_emulation_agrees_with_the_fp64_reference_inside_the_gpu_bound(case):
    """Every case satisfies its entry point's argument checks, and the fp32 emulation lands inside the bound tests/test_aux_sweep_gpu.py applies to the HIP kernel on
    the same inputs: the bound is reachable by fp32 arithmetic there."""
    t = ac.build(case)
    _entry_checks(case, t)
    want = ref_run(case, t)
    got = ar.run(case, ar.Emu(), t, ar.EMU)
    figures = ar.compare(case, got, want, who="fp32 emulation", device_types=False, t=t)
    print(case.id, {k: (f"{r:.2e}", f"{m:.2e}") for k, (r, m) in figures.items()})


def test_the_derived_edges_are_where_the_launch_code_changes():
    """The table sits on both sides of what it claims."""
    cdw = [c for c in ac.CASES if c.entry == "conv_dw"]
    geo = {c.id: ac.cw_geometry(c.p["M"], c.p["N"], c.p["K"]) for c in cdw}
    assert {g[2] for g in geo.values()} == {"tiles", "stages", "scratch", "cap256"}
    assert geo["cdw-scratch-clamp"] == (1, 160, "scratch") and ac.cw_geometry(140, 1920, 1920)[:2] == (2, 96)          # 900 tiles, 126.6 MiB per split: two splits
    assert any(g[0] == 1 for g in geo.values()) and any(g[0] == 256 for g in geo.values()) and any(g[0] == 41 for g in geo.values())
    assert geo["cdw-short-last-split"][:2] == (5, 128) and 513 - 4 * 128 == 1
    assert geo["cdw-swallowed-split"][:2] == (40, 128) and ac.cw_geometry(5000, 320, 320)[2] == "stages"
    assert ac.cw_geometry(32768, 64, 64)[0] == 256 and ac.cw_geometry(32769, 64, 64)[:2] == (205, 160)                 # the cap, then 160-row splits: 51 splits swallowed
    for N, K, lim in ac.CW_EDGE_SHAPES:
        edges = ac.cw_edges(N, K, lim)
        assert len(edges) >= 8 and all(f"cdw-edge-N{N}-K{K}-M{M}" in ac.BY_ID for M in edges)
        whys = [ac.cw_geometry(M, N, K)[2] for M in edges]
        assert len(set(whys)) == 2 and any(ac.cw_geometry(M, N, K)[0] == 1 for M in edges) and any(ac.cw_geometry(M, N, K)[0] == 2 for M in edges)
    ms = {c.p["M"] for c in cdw}
    assert {1, 2, 31, 32, 33, 63, 64, 65} <= ms and any(c.p["M"] % geo[c.id][1] for c in cdw) and any(c.p["M"] % geo[c.id][1] == 0 and geo[c.id][0] > 1 for c in cdw)
    for cid in ("cdw-split-inside-an-image-row", "cdw-split-inside-a-row-s2", "cdw-split-inside-a-row-ups"):       # the first split ends inside an image row
        p = ac.BY_ID[cid].p
        Hout, Wout = ac.conv_out(p["Hin"], p["Win"], p["stride"], p["ups"])
        assert geo[cid][0] > 1 and (geo[cid][1] % (Hout * Wout)) % Wout != 0, cid
    fold = ac.BY_ID["cdw-fold-wraps"].p
    assert ac.grid_for(fold["N"] * 9 * fold["K"] // 4, 4096) == 4096 < (fold["N"] * 9 * fold["K"] // 4 + 255) // 256
    assert all(ac.grid_for(c.p["N"] * 9 * c.p["K"] // 4, 4096) < 4096 for c in cdw if c.id not in ("cdw-fold-wraps", "cdw-scratch-clamp"))
    assert {(c.p["stride"], c.p["ups"], c.p["Hin"] % 2, c.p["Win"] % 2) for c in cdw} >= {(1, 0, 1, 1), (1, 0, 0, 0), (2, 0, 1, 1), (2, 0, 0, 0), (2, 0, 1, 0), (1, 1, 1, 1), (1, 1, 0, 0)}
    assert any(c.p["Hin"] == 1 and c.p["Win"] > 1 for c in cdw) and any(c.p["Win"] == 1 and c.p["Hin"] > 1 for c in cdw) and any(c.p.get("dy16") for c in cdw)
    # groupnorm_bwd_params
    gnp = [c.p for c in ac.CASES if c.entry == "gn_params"]
    bl = [ac.gn_params_blocks(p["rpg"] * p["nsg"]) + (p["rpg"], p["rpg"] * p["nsg"]) for p in gnp]
    assert {b for b, _, _, _ in bl} >= {1, 2, 511, 512} and ac.gn_params_blocks(32832) == (512, 65) and -(-32832 // 65) == 506          # six blocks hold no row
    assert ac.gn_params_blocks(32704) == (511, 64) and ac.gn_params_blocks(32768) == (512, 64) and ac.gn_params_blocks(65) == (2, 33) and ac.gn_params_blocks(64) == (1, 64)
    assert any(rpg == 1 and b > 1 for b, _, rpg, _ in bl) and any(1 < rpg < rpb and rpb % rpg for _, rpb, rpg, _ in bl) and any(rpg == rpb and b > 1 for b, rpb, rpg, _ in bl)
    assert any(rpg > rpb and rpg % rpb for _, rpb, rpg, _ in bl) and any(rows % rpb for _, rpb, _, rows in bl)
    assert {p["C"] for p in gnp} >= {8, 64, 264, 2560} and {p["groups"] for p in gnp} >= {1, 32, 64} and any(p["C"] == p["groups"] for p in gnp)
    assert {p.get("only") for p in gnp} == {None, "dgamma", "dbeta"} and {p["silu"] for p in gnp} == {True, False}
    # conv_small
    cs = [c for c in ac.CASES if c.entry == "conv_small"]
    assert {c.path for c in cs} == {f"conv_small{k}_kernel<{ci}>" for k in ("", "_tile") for ci in (3, 4)}
    assert {(c.p["Cin"], c.p["Cout"]) for c in cs} >= {(ci, co) for ci in (3, 4) for co in (8, 56, 64, 80, 88, 96, 480, 488, 512)}
    assert [ac.conv_small_target(4, co).startswith("conv_small_tile") for co in (56, 64, 80, 96, 480, 488, 512)] == [False, True, False, True, True, False, False]
    assert ac.conv_small_geometry(3, 88, 65) == (256, 1, 2) and ac.conv_small_geometry(3, 512, 65) == (256, 1, 7) and ac.conv_small_geometry(4, 80, 65) == (256, 1, 1)
    for kind in ("tile", "direct"):
        assert {c.p["n_img"] * c.p["H"] * c.p["W"] for c in cs if c.id.startswith(f"cs-{kind}-pix")} == {1, 63, 64, 65, 255, 256, 257}
    assert any(c.p["H"] == 1 and c.p["W"] > 1 for c in cs) and any(c.p["W"] == 1 and c.p["H"] > 1 for c in cs) and any(c.p["H"] == c.p["W"] == 1 for c in cs)
    # the flat kernels: exactly one pass of the capped grid, and one vector more
    for entry, per in (("axpy_rows", 4), ("copy_rows", 8), ("copy_blocks", 8), ("embed_rows", 8)):
        vec = sorted(c.p["rows"] * c.p.get("n0", 1) * c.p.get("n1", 1) * (c.p.get("cols") or c.p["C"]) // per for c in ac.CASES if c.entry == entry)
        assert vec[-2:] == [ac.FLAT_EDGE, ac.FLAT_EDGE + 1] and (vec[0] == 1 or entry in ("copy_blocks", "embed_rows")), entry
        assert ac.grid_for(vec[-2], ac.FLAT_CAP) == ac.grid_for(vec[-1], ac.FLAT_CAP) == ac.FLAT_CAP and ac.grid_for(vec[-2] - 256, ac.FLAT_CAP) == ac.FLAT_CAP - 1
    for entry in ("silu", "relu", "quick_gelu"):
        ns = {c.p["n"] for c in ac.CASES if c.entry == entry}
        assert ns >= {1, 7, 8, 9, 2049, 2055, ac.FLAT_EDGE * 8, (ac.FLAT_EDGE + 1) * 8 + 1}
    up = ac.BY_ID["rf-ups4-beyond-the-grid"].p["entries"][0]
    assert up[1] * 16 * (up[2] // 4) > 8192 * 256 and ac.grid_for(up[1] * 16 * (up[2] // 4), 8192) == 8192
    # attention_causal: one and two query blocks, waves that return after the barrier, an odd tile count against the paired contraction, padded keys
    g = {nq: ac.attn_causal_geometry(nq) for nq in ac.CAUSAL_NQ}
    assert g[1] == [(1, 32, [1, 0, 0, 0])] and g[17] == [(17, 32, [1, 2, 0, 0])] and g[64] == [(64, 64, [1, 2, 3, 4])] and g[65] == [(64, 64, [1, 2, 3, 4]), (65, 96, [5, 0, 0, 0])]
    assert g[33][0] == (33, 64, [1, 2, 3, 0]) and g[77][1] == (77, 96, [5, 0, 0, 0]) and g[97][1] == (97, 128, [5, 6, 7, 0]) and g[128][1] == (128, 128, [5, 6, 7, 8])
    assert {c.p["nq"] for c in ac.CASES if c.entry == "attention_causal"} >= set(ac.CAUSAL_NQ)
    assert {c.p["kind"] for c in ac.CASES if c.entry == "attention_causal"} == {"soft", "rising", "falling", "high-gain"}


def test_geometry_restatement_matches_the_library_host_functions_and_a_brute_force_scan():
    """me_conv_dw_splits / me_conv_dw_work_bytes / me_groupnorm_bwd_params_work_bytes are host functions (no launch): the Python restatement that placed the edges is
    the library's.  The scan confirms what the table's docstring says about the 256 MiB clamp: it decides for 911 .. 1023 block tiles only."""
    from motioneditor_amd import capi
    L = capi.lib()
    shapes = [(c.p["M"], c.p["N"], c.p["K"]) for c in ac.CASES if c.entry == "conv_dw"]
    shapes += [(M, N, K) for N, K in ((64, 64), (320, 320), (2560, 320), (8, 8), (1920, 2048), (1280, 2560)) for M in list(range(1, 700, 7)) + [32767, 32768, 32769, 40000, 393216]]
    for M, N, K in shapes:
        s, rps, _ = ac.cw_geometry(M, N, K)
        assert L.me_conv_dw_splits(M, N, K) == s and L.me_conv_dw_work_bytes(M, N, K) == ac.cw_work_bytes(M, N, K), (M, N, K)
        assert (s - 1) * rps < M <= s * rps and rps % 32 == 0                     # every split holds a row, the splits cover M
    assert L.me_conv_dw_work_bytes(0, 64, 64) == 0 and L.me_conv_dw_splits(64, 0, 64) == 0
    deciding = set()
    for n in range(1, 41):                                                       # N, K multiples of 64 up to 2560: every tile count the UNet's channels reach
        for k in range(n, 41):
            N, K = 64 * n, 64 * k
            if N * 9 * K * 4 > ac.CW_CAP:
                continue
            for M in (1, 128, 129, 257, 4096, 40000, 400000):
                if ac.cw_geometry(M, N, K)[2] == "scratch":
                    deciding.add(n * k)
    assert deciding and min(deciding) >= 911 and max(deciding) <= 1023, sorted(deciding)
    for M in (1, 128):                                                           # below 129 rows the stage clamp already allows one split only
        assert ac.cw_geometry(M, 1920, 2048)[2] == "stages"
    rows = [1, 63, 64, 65, 127, 128, 129, 4095, 32704, 32767, 32768, 32769, 32832, 98304, 393216]
    for r in rows:
        for rpg in (1, r):
            for C, groups in ((64, 32), (264, 33), (2560, 64)):
                assert L.me_groupnorm_bwd_params_work_bytes(r, rpg, C, groups) == ac.gn_params_work_bytes(r, rpg, C, groups), (r, rpg, C, groups)
    for r in range(1, 40000):                                                    # the scan over rows: 33 .. 64 rows per block beyond one block, <= 512 blocks, every row covered
        b, rpb = ac.gn_params_blocks(r)
        assert b <= 512 and b * rpb >= r and (b == 1 or 33 <= rpb) and (b == 512 or rpb <= 64) and (r <= 32768 or b == 512)
    assert L.me_groupnorm_bwd_params_work_bytes(10, 3, 64, 32) == 0


def test_the_swept_entry_points_refuse_what_their_kernels_rely_on():
    """aux_run.refused on addresses that are never dereferenced: every violating call returns ME_EINVAL with a message naming the entry point BEFORE anything is
    launched (tests/test_aux_sweep_gpu.py repeats them on device buffers filled with a sentinel)."""
    if torch.cuda.is_available():      # (as tests/test_abi_cpu.py: with a device present a call that slipped through would launch on these numbers)
        pytest.skip("a device is present: the same violations run on real buffers in tests/test_aux_sweep_gpu.py")
    from motioneditor_amd import capi
    L = capi.lib()
    n = 0
    for entry, make, bad in ar.refused(capi):
        for label, change, needle in bad:
            fake = {}
            ptr = lambda name, nbytes: fake.setdefault(name, 0x100000 * (len(fake) + 1))    # noqa: E731
            a = make(ptr)
            change(a, ptr)
            rc = ar.call_refused(L, entry, a)
            msg = L.me_last_error().decode()
            assert rc == capi.ME_EINVAL and msg.startswith(entry + ":") and needle in msg, f"{entry} ({label}): status {rc}, message {msg!r}"
            n += 1
    assert n == len(ac.CONV_DW_REFUSED) + len(ac.CAUSAL_REFUSED) >= 19


# ------------------------------------------------------------------------------------------------------------------ deliberately wrong emulations
class _ConvDwRows(ar.Emu):
    """conv_dw mutants that lose rows of the contraction: `lost(M, splits, rows_per_split)` names them."""
    def lost(self, M, s, rps):
        return []

    def gemm_dw(self, dy, x, *, M, K, **kw):
        s, rps, _ = ac.cw_geometry(M, dy.shape[1], K)
        dy = dy.clone()
        for r in self.lost(M, s, rps):
            dy[r] = 0
        return super().gemm_dw(dy, x, M=M, K=K, **kw)


class PartialLastStageDropped(_ConvDwRows):
    def lost(self, M, s, rps):
        m0 = (s - 1) * rps
        return range(m0 + (M - m0) // 32 * 32, M)


class SplitStartsOneRowLate(_ConvDwRows):
    def lost(self, M, s, rps):
        return [sp * rps for sp in range(1, s)]


class FoldWithoutAlpha(ar.Emu):
    def gemm_dw(self, dy, x, *, alpha=1.0, **kw):
        return super().gemm_dw(dy, x, alpha=1.0, **kw)


class PaddingTapInImageAtHin1(ar.Emu):
    """At Hin = 1 the taps above and below the image read what the centre row reads (`iy` never checked against the one-row image)."""
    def gemm_dw(self, dy, x, *, dst, conv, **kw):
        inc = torch.zeros_like(dst)
        super().gemm_dw(dy, x, dst=inc, conv=conv, **kw)
        if conv[0] == 1 and conv[5] == 0:
            inc[:, 0:3] = inc[:, 3:6]
            inc[:, 6:9] = inc[:, 3:6]
        dst.add_(inc)
        return dst


def _gn_params_explicit(x, gamma, beta, dy, rpg, groups, silu, eps, stat_group=None, keep=None):
    """dgamma, dbeta in fp32 with the statistic group of every row nameable (stat_group[row]) and rows droppable (keep[row])."""
    rows, C = x.shape
    xf = x.float()
    t = xf.reshape(rows // rpg, rpg, groups, C // groups)
    mean, var = t.mean(dim=(1, 3)), t.var(dim=(1, 3), unbiased=False)                      # [nsg, groups]
    sg = torch.arange(rows) // rpg if stat_group is None else stat_group
    mean_r, var_r = mean[sg].repeat_interleave(C // groups, dim=1), var[sg].repeat_interleave(C // groups, dim=1)
    xh = (xf - mean_r) / torch.sqrt(var_r + eps)
    d = dy.float().clone()
    if silu:
        y = xh * gamma.float() + beta.float()
        sig = torch.sigmoid(y)
        d = d * sig * (1 + y * (1 - sig))
    if keep is not None:
        d = d * keep[:, None]
    return (d * xh).sum(0), d.sum(0)


class _GnParams(ar.Emu):
    def rows_of(self, rows, rpg):
        return None, None

    def groupnorm_bwd(self, x, gamma, beta, dy, *, rows_per_group, eps, silu, groups=32, dgamma=None, dbeta=None):
        sgrp, keep = self.rows_of(x.shape[0], rows_per_group)
        dg, db = _gn_params_explicit(x, gamma, beta, dy, rows_per_group, groups, silu, eps, sgrp, keep)
        if dgamma is not None:
            dgamma.add_(dg)
        if dbeta is not None:
            dbeta.add_(db)


class BlockKeepsItsFirstGroupsStatistics(_GnParams):
    """The rows after a sample-group boundary inside a block are normalised with another group's statistics: those of the group the block started in."""
    def rows_of(self, rows, rpg):
        _, rpb = ac.gn_params_blocks(rows)
        r = torch.arange(rows)
        return (r // rpb * rpb) // rpg, None


class LastBlocksShortRangeDropped(_GnParams):
    def rows_of(self, rows, rpg):
        _, rpb = ac.gn_params_blocks(rows)
        keep = torch.ones(rows)
        if rows % rpb:
            keep[rows // rpb * rpb:] = 0
        return None, keep


class UnaryTailSkipped(ar.Emu):
    def _cut(self, y):
        y = y.clone()
        y[y.numel() // 8 * 8:] = 0
        return y

    def silu(self, x):
        return self._cut(emu_ops.silu(x))

    def relu(self, x):
        return self._cut(emu_ops.relu(x))

    def quick_gelu(self, x):
        return self._cut(ar.emu_clip_ops.quick_gelu(x))


class FlatKernelsStopAtTheGridCap(ar.Emu):
    """No grid-stride loop: the work items beyond 16384 * 256 are never reached (what they would have written stays what it was)."""
    def axpy_rows(self, y, x, a_, alpha=1.0):
        n = ac.FLAT_EDGE * 4 // y.shape[1]
        return emu_ops.axpy_rows(y[:n], x[:n], a_[:n], alpha)

    def copy_rows(self, y, x):
        n = ac.FLAT_EDGE * 8 // x.shape[1]
        return emu_ops.copy_rows(y[:n], x[:n])

    def copy_blocks(self, y, x, n0, n1, rows, **kw):
        if n0 * n1 * rows * (x.shape[1] // 8) <= ac.FLAT_EDGE:
            return emu_ops.copy_blocks(y, x, n0, n1, rows, **kw)
        assert n0 == n1 == 1
        return emu_ops.copy_blocks(y, x, 1, 1, ac.FLAT_EDGE * 8 // x.shape[1], **kw)

    def _cut(self, y):
        y = y.clone()
        y[ac.FLAT_EDGE * 8:] = 0
        return y

    def silu(self, x):
        return self._cut(emu_ops.silu(x))

    def relu(self, x):
        return self._cut(emu_ops.relu(x))

    def quick_gelu(self, x):
        return self._cut(ar.emu_clip_ops.quick_gelu(x))

    def embed_rows(self, tok, pos, ids, seq):
        y = super().embed_rows(tok, pos, ids, seq).clone()
        y[ac.FLAT_EDGE * 8 // tok.shape[1]:] = 0
        return y


class ConvSmallLastPixelBlockUnwritten(ar.Emu):
    def conv_small(self, inp, w, bias, *, n_img, Cin, H, Wd, **kw):
        y = emu_ops.conv_small(inp, w, bias, n_img=n_img, Cin=Cin, H=H, Wd=Wd, **kw).clone()
        per = ac.conv_small_geometry(Cin, w.shape[0], y.shape[0])[0]
        if y.shape[0] % per:
            y[y.shape[0] // per * per:] = 0
        return y


class ConvSmallBorderTapNotZero(ar.Emu):
    """The taps outside the image read the nearest pixel instead of zero."""
    def conv_small(self, inp, w, bias, *, n_img, Cin, H, Wd, img_stride, ch_stride, frames=0, frame_stride=0, silu=False):
        flat = inp.reshape(-1).float()
        imgs = []
        for i in range(n_img):
            base = (i // frames) * img_stride + (i % frames) * frame_stride if frames > 0 else i * img_stride
            imgs.append(torch.stack([flat[base + c * ch_stride:base + c * ch_stride + H * Wd].reshape(H, Wd) for c in range(Cin)]))
        Cout = w.shape[0]
        y = F.conv2d(F.pad(torch.stack(imgs), (1, 1, 1, 1), mode="replicate"), w.float().reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2), None if bias is None else bias.float())
        return (F.silu(y) if silu else y).permute(0, 2, 3, 1).reshape(-1, Cout)


class ConvSmallSliceStartsAtTheWrongChannel(ar.Emu):
    """The direct kernel's second and later 80-channel slices start 8 channels early: their results land one vector to the left, the last vector is never written."""
    def conv_small(self, inp, w, bias, *, Cin, **kw):
        y = emu_ops.conv_small(inp, w, bias, Cin=Cin, **kw).clone()
        Cout = w.shape[0]
        if ac.conv_small_geometry(Cin, Cout, 1)[2] > 1:
            y[:, 72:Cout - 8] = y[:, 80:].clone()
            y[:, Cout - 8:] = 0
        return y


class _Causal(ar.Emu):
    """me_attn_causal written on the logits so that a mutant can change the mask and the denominator."""
    def mask(self, nq):
        return torch.arange(nq)[None, :] <= torch.arange(nq)[:, None]

    def extra_denominator(self, nq, m, scale):
        return 0.0

    def attention_causal(self, q, k, v, *, heads, dh, n_seq, nq, scale=None):
        scale = dh ** -0.5 if scale is None else scale
        sp = lambda t: t.float()[:n_seq * nq, :heads * dh].reshape(n_seq, nq, heads, dh).permute(0, 2, 1, 3)   # noqa: E731
        s = (sp(q) @ sp(k).transpose(-1, -2)) * scale
        s = s.masked_fill(~self.mask(nq), -math.inf)
        m = s.max(dim=-1, keepdim=True).values
        e = (s - m).exp()
        p = e / (e.sum(dim=-1, keepdim=True) + self.extra_denominator(nq, m, scale))
        return (p @ sp(v)).permute(0, 2, 1, 3).reshape(n_seq * nq, heads * dh)


class CausalMaskAdmitsTheNextKey(_Causal):
    def mask(self, nq):
        return torch.arange(nq)[None, :] <= torch.arange(nq)[:, None] + 1


class CausalMaskExcludesTheDiagonal(_Causal):
    def mask(self, nq):
        keep = torch.arange(nq)[None, :] < torch.arange(nq)[:, None]
        keep[0, 0] = True
        return keep


class CausalDenominatorCountsPaddedKeys(_Causal):
    """The zero-filled keys between nq and the end of the last 16-key tile (score 0) are counted in the denominator of the queries whose wave walks that tile."""
    def extra_denominator(self, nq, m, scale):
        pad = (nq + 15) // 16 * 16 - nq
        last_tile = (torch.arange(nq) >= (nq - 1) // 16 * 16).float()[None, None, :, None]
        return pad * last_tile * (0.0 - m).exp()


class EmbedPositionsByRowOverSeq(ar.Emu):
    def embed_rows(self, tok, pos, ids, seq):
        r = torch.arange(ids.numel())
        ok = (ids >= 0) & (ids < tok.shape[0])
        y = (tok.float()[ids.clamp(0, tok.shape[0] - 1).long()] + pos.float()[(r // seq) % pos.shape[0]]).to(tok.dtype)
        return torch.where(ok.reshape(-1, 1), y, torch.zeros((), dtype=y.dtype))


class GaussianSampleUnclamped(ar.Emu):
    def gaussian_sample(self, moments, noise, n_img, npix, scale=1.0):
        m = moments.float()[:, :8].reshape(n_img, npix, 8).permute(0, 2, 1)
        return (m[:, :4] + torch.exp(0.5 * m[:, 4:]) * noise.float().reshape(n_img, 4, npix)) * scale


class CfgDdimCondFromTheNextBatchEntry(ar.Emu):
    def cfg_ddim(self, latents, eps_rows, *, guidance, ca, cb):
        nb, C, f, h, w = latents.shape
        e = eps_rows.float()[:, :C].reshape(2 * nb, f, h * w, C).permute(0, 3, 1, 2).reshape(2 * nb, C, f, h, w)
        eu, ec = e[:nb], e[1:nb + 1]
        return ca * latents + cb * (eu + guidance * (ec - eu))


class RefreshSearchPicksThePreviousEntry(ar.Emu):
    """At a row0 boundary the search lands on the entry before: the row index is past that entry's rows and the wave returns -- the first row of every entry but
    the first stays what it was."""
    def refresh(self, entries):
        plain = [d for d in entries if d["kind"] != "ups4"]
        before = [{n: d[n][:1].clone() for n in ("dst", "colsum", "cvec") if d.get(n) is not None} for d in plain]
        super().refresh(entries)
        for d, b in list(zip(plain, before))[1:]:
            for n, v in b.items():
                d[n][:1] = v


MUTANTS = {
    "conv_dw drops a partial last stage": (PartialLastStageDropped, ("conv_dw",)),
    "conv_dw starts a split one row late": (SplitStartsOneRowLate, ("conv_dw",)),
    "conv_dw folds without alpha": (FoldWithoutAlpha, ("conv_dw",)),
    "conv_dw treats a padding tap as in-image at Hin = 1": (PaddingTapInImageAtHin1, ("conv_dw",)),
    "gn-params uses another group's statistics for the rows after a boundary inside a block": (BlockKeepsItsFirstGroupsStatistics, ("gn_params",)),
    "gn-params drops the last block's short range": (LastBlocksShortRangeDropped, ("gn_params",)),
    "the unary tail is skipped": (UnaryTailSkipped, ("silu", "relu", "quick_gelu")),
    "the flat kernels stop at the grid cap": (FlatKernelsStopAtTheGridCap, ("axpy_rows", "copy_rows", "copy_blocks", "silu", "relu", "quick_gelu", "embed_rows")),
    "conv_small leaves the last partial pixel block unwritten": (ConvSmallLastPixelBlockUnwritten, ("conv_small",)),
    "conv_small's border tap is not zero": (ConvSmallBorderTapNotZero, ("conv_small",)),
    "conv_small's 80-channel slice starts at the wrong channel": (ConvSmallSliceStartsAtTheWrongChannel, ("conv_small",)),
    "the causal mask admits key q + 1": (CausalMaskAdmitsTheNextKey, ("attention_causal",)),
    "the causal mask excludes the diagonal": (CausalMaskExcludesTheDiagonal, ("attention_causal",)),
    "the causal mask counts padded keys in the denominator": (CausalDenominatorCountsPaddedKeys, ("attention_causal",)),
    "embed_rows indexes positions by r // seq": (EmbedPositionsByRowOverSeq, ("embed_rows",)),
    "gaussian_sample goes unclamped": (GaussianSampleUnclamped, ("gaussian_sample",)),
    "cfg_ddim takes the conditional rows from b + 1 instead of b + nb": (CfgDdimCondFromTheNextBatchEntry, ("cfg_ddim",)),
    "the refresh search picks the previous entry at a row0 boundary": (RefreshSearchPicksThePreviousEntry, ("refresh",)),
}
# mutants that restate their operation (not a change of ar.Emu's result): un-mutated they must pass every case too
UNMUTATED = {"gn_params": _GnParams, "attention_causal": _Causal}


def _cost(case):
    """A size figure from the parameters alone: the mutant search tries the small cases first."""
    p = case.p
    return p.get("M", 1) * p.get("N", 1) * p.get("K", 1) + p.get("n", 0) + p.get("rows", 0) * p.get("cols", p.get("C", 1)) * p.get("n0", 1) * p.get("n1", 1) \
        + p.get("rpg", 0) * p.get("nsg", 0) * p.get("C", 0) + p.get("nq", 0) * p.get("heads", 0) * 100 + p.get("n_img", 0) * p.get("H", 0) * p.get("W", 0) * p.get("Cout", 0)


def _passes(case, backend, who):
    t = ac.build(case)
    try:
        ar.compare(case, ar.run(case, backend, t, ar.EMU), ref_run(case, t), who=who, device_types=False, t=t)
    except AssertionError as exc:
        return str(exc).splitlines()[0][:160]
    return None


@pytest.mark.parametrize("entry", list(UNMUTATED))
def test_the_restated_emulations_pass_every_case_when_un_mutated(entry):
    for case in (c for c in ac.CASES if c.entry == entry and not c.prod):
        assert _passes(case, UNMUTATED[entry](), "un-mutated") is None, case.id


@pytest.mark.parametrize("name", list(MUTANTS))
def test_a_deliberately_wrong_emulation_fails_at_least_one_case(name):
    """A mutant that passes every case of its entry points means the table is too weak there: extend the table, do not delete the mutant."""
    cls, entries = MUTANTS[name]
    for entry in entries:
        hit = None
        for case in sorted((c for c in ac.CASES if c.entry == entry and not c.prod), key=_cost):
            msg = _passes(case, cls(), name)
            if msg is not None:
                hit = (case.id, msg)
                break
        assert hit is not None, f"mutant '{name}' passes every {entry} case"
        print(f"mutant '{name}' caught by case {hit[0]}: {hit[1]}")
