"""The forward sweep without a GPU: the case table of tests/fwd_cases.py against itself (every launch target named in GEMM_TARGETS / ATTN_TARGETS /
TATTN_TARGETS is predicted for at least one case; every threshold of the restated dispatch has a pair of cases that differ only in crossing it), the fp32
emulation against the fp64 reference of tests/ref64_fwd.py inside the bound the GPU file applies to the HIP kernel, choose_split against the library's host
function me_gemm_work_bytes, the host-side argument checks restated on every case, the refused calls on fabricated addresses, and eleven deliberately wrong
emulations against the cases named for them."""
import ctypes
import math

import pytest
import torch

import emu_ops
import fwd_cases as fc
import fwd_run as fr
import ref64_fwd as ref
import ups_fold_ref

_REF = {}


def ref_run(case, t):
    hit = _REF.get(case.id)
    if hit is None:
        hit = fr.run(case, ref, t, fr.REF)
        if sum(v.numel() for v in hit.values()) < 2_000_000:
            _REF[case.id] = hit
    return hit


# ------------------------------------------------------------------------------------------------------------------ the table itself
def test_case_ids_are_unique():
    ids = [c.id for c in fc.CASES]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)
    assert sum(c.prod for c in fc.CASES) == 1 and fc.BY_ID["gemm-conv-halo-512-images"].prod
    assert all(c.bound is None and c.elementwise is None for c in fc.CASES)          # every case on its entry point's own bound
    print("cases per entry point:", fc.case_counts(), "total", len(fc.CASES))


def test_every_launch_target_is_predicted_for_a_case():
    by_entry = {e: {c.path for c in fc.CASES if c.entry == e} for e in ("gemm", "attention", "temporal_attention")}
    assert by_entry["gemm"] == set(fc.GEMM_TARGETS), by_entry["gemm"] ^ set(fc.GEMM_TARGETS)
    assert by_entry["attention"] == set(fc.ATTN_TARGETS), by_entry["attention"] ^ set(fc.ATTN_TARGETS)
    assert by_entry["temporal_attention"] == set(fc.TATTN_TARGETS), by_entry["temporal_attention"] ^ set(fc.TATTN_TARGETS)
    gemm = [c for c in fc.CASES if c.entry == "gemm"]
    # what the kernel name does not carry: both stagings and the packed-tap mode, every epilogue of launch_gemm8p, ln_out fused and appended, ups = 3 on each family
    assert {fc.gemm_staging(c.p) for c in gemm} == {"buf", "glds", "glds+packed"}
    epi = {fc.gemm_epilogue(fc._gemm_args(c.p), c.p.get("env")) for c in gemm if c.path.startswith("gemm8p")}
    assert epi == {"row0", "row2", "row4", "row6", "row12", "direct"}, epi
    ways_out = {c.id: fc.gemm_epilogue(fc._gemm_args(c.p), c.p.get("env")) for c in gemm if c.id.startswith("gemm-epi-8p256")}
    for cid in ("f8", "f10", "f14", "act1", "act2", "ldc-odd", "c-8-byte", "res-8-byte", "rowepi-off"):
        assert ways_out[f"gemm-epi-8p256-{cid}"] == "direct", cid
    assert ways_out["gemm-epi-8p256-out-aliases-res"] == "row4" and ways_out["gemm-epi-8p256-rpv-255"] == "row2"
    fused = {fc.gemm_ln_out_fused(fc._gemm_args(c.p), c.p.get("env")) for c in gemm if c.p.get("ln_out")}
    assert fused == {True, False}
    assert {c.path for c in gemm if c.p.get("conv") and c.p["conv"][5] == 3} >= {"gemm_kernel<128,64>", "gemm_kernel<128,128>", "gemm_kernel<128,160>", "gemm_kernel<256,320>", "gemm8p_kernel<256,320,true>",
                                                                                    "gemm8p_kernel<192,320,true>"}
    assert {c.path for c in gemm if c.p.get("ln")} >= {"gemm8p_kernel<256,320,false>", "gemm8p_kernel<256,256,false>", "gemm8p_kernel<192,320,false>", "gemm_kernel<128,64>"}
    for fam in ("gemm8p_kernel<256,320,false>", "gemm8p_kernel<192,320,false>", "gemm8p_kernel<128,320,false>", "gemm_kernel<256,320>", "gemm_kernel<128,160>", "gemm_kernel<128,128>",
                "gemm_kernel<128,64>"):
        mine = [c for c in gemm if c.path == fam]
        assert any(c.p.get("sel") for c in mine) and any(c.p.get("pieces") for c in mine) and any(c.twice for c in gemm if c.path.split("+")[0] == fam), fam
    for fam in ("gemm_kernel<256,320>+splitk", "gemm_kernel<128,160>+splitk", "gemm_kernel<128,128>+splitk", "gemm_kernel<128,64>+splitk"):
        assert any(c.p.get("sel") and c.twice for c in gemm if c.path == fam), fam
    splits = {fc.choose_split(c.p, fc._cdiv(c.p["M"], 128) * fc._cdiv(c.p["N"], 64), c.p["K"] // 64 * fc._taps(c.p), c.p.get("env")) for c in gemm if c.path == "gemm_kernel<128,64>+splitk"}
    assert splits == {2, 3, 4}, splits


def test_every_attention_kernel_sits_at_its_query_block_and_key_stage_edges():
    for target in fc.ATTN_TARGETS:
        mine = [c.p for c in fc.CASES if c.path == target]
        bq, stage = fc.attn_geometry(target)
        nqs, nks = {p["nq"] for p in mine}, {p["nk"] for p in mine}
        assert any(n % bq == 1 for n in nqs) and any(n % bq == bq - 1 or n < bq for n in nqs), (target, sorted(nqs))
        # nq = BQ exactly: everywhere but attn2_kernel<80,2,4,*>, which me_attn selects for nq < 128 = its BQ only
        assert any(n % bq == 0 for n in nqs) or target.startswith("attn2_kernel<80,2,4,"), (target, sorted(nqs))
        assert any(n % 64 for n in nks), (target, sorted(nks))
        if "fold" in target:
            assert {256, 257, 256 + stage + 1, 256 + 2 * stage - 1} <= nks, (target, stage, sorted(nks))
        elif "classic" in target:
            assert {1, 15, 16, 17, 63, 64, 65, 80, 81, 255} <= nks, (target, sorted(nks))
        elif "kvres" in target:
            assert {65, 77, 80} <= nks
        assert len({p["heads"] for p in mine}) >= 2, target
    frames = {(c.p["dh"], c.p["frames"]) for c in fc.CASES if c.entry == "temporal_attention"}
    assert frames >= {(dh, F) for dh in (40, 80, 160) for F in fc.TATTN_MFMA_FRAMES} | {(dh, F) for dh in (32, 320) for F in fc.TATTN_THREAD_FRAMES} | {(8, 8)}
    assert fc.tattn_target(fc.TATTN_REFUSED_THREADS) is None and fc.tattn_target(dict(frames=65, dh=40)) is None and fc.tattn_target(dict(frames=12, dh=32)) is None


_BOOKKEEPING = ("sel", "pieces", "lse", "n_kv")      # what a case asserts in addition, not what it launches


@pytest.mark.parametrize("name,below,at", fc.PAIRS, ids=[f"{n}: {a} | {b}" for n, a, b in fc.PAIRS])
def test_threshold_pairs_differ_only_in_crossing_the_threshold(name, below, at):
    a, b = fc.BY_ID[below], fc.BY_ID[at]
    what = lambda c: (c.path, fc.gemm_epilogue(fc._gemm_args(c.p), c.p.get("env")) if c.entry == "gemm" else None)    # noqa: E731
    assert what(a) != what(b) and (a.path != b.path or name == "ME_GEMM_ROWEPI"), (a.path, b.path)
    pa, pb = ({k: v for k, v in c.p.items() if k not in _BOOKKEEPING and v not in (None, 0, False)} for c in (a, b))
    diff = {k for k in set(pa) | set(pb) if pa.get(k) != pb.get(k)}
    assert len(diff) == 1, (name, diff)
    if diff == {"env"}:
        ea, eb = fc._envd(pa.get("env")), fc._envd(pb.get("env"))
        assert {k for k in ea if ea[k] != eb[k]} == {name}, (name, pa.get("env"), pb.get("env"))
    else:
        assert next(iter(diff)).split("_")[0] in name.replace("ldo", "o").replace("O alignment", "o").replace("nseg", "table"), (name, diff)


def test_every_threshold_of_the_restated_dispatch_has_a_pair():
    named = {n for n, _, _ in fc.PAIRS}
    assert named >= set(fc.THRESHOLDS), set(fc.THRESHOLDS) - named
    p192, p128, plain = fc.BY_ID["gemm-8p192-mink-K256"], fc.BY_ID["gemm-8p128-mink-K256"], fc.BY_ID["gemm-N320-default"]
    assert p192.path == "gemm8p_kernel<192,320,false>" and p128.path == "gemm8p_kernel<128,320,false>" and plain.path == "gemm_kernel<128,64>"
    for forced in (p192, p128):        # the same arguments under the default threshold stay on the 128-row kernel
        assert fc.gemm_target(fc._gemm_args(forced.p), None) == "gemm_kernel<128,64>"
    on, off = fc.BY_ID["gemm-epi-8p256-f6"], fc.BY_ID["gemm-epi-8p256-rowepi-off"]
    assert {k: v for k, v in on.p.items() if k != "env"} == {k: v for k, v in off.p.items() if k != "env"}
    assert fc.gemm_epilogue(fc._gemm_args(on.p), on.p["env"]) == "row6" and fc.gemm_epilogue(fc._gemm_args(off.p), off.p["env"]) == "direct"


# ------------------------------------------------------------------------------------------------------------------ restatement against the library
def test_choose_split_restatement_matches_me_gemm_work_bytes(monkeypatch):
    """me_gemm_work_bytes is a host function (no launch) that shares choose_split with me_gemm: a grid of shapes, every refusing argument, the threshold switch."""
    from motioneditor_amd import capi
    L = capi.lib()
    grid = [dict(M=M, N=N, K=K, **g) for M in (1, 127, 128, 129, 640, 1536, 2048, 2433, 8192, 40000) for N in (4, 320, 1216, 1276, 1280, 1440, 2560, 10240)
            for K in (8, 64, 72, 1984, 2048, 2112, 4096) for g in ({}, {"conv": (8, 8, 8, 8, 1, 0)}, {"tconv": (4, 16, 4)})]
    grid += [dict(M=128, N=1280, K=2048, **g) for g in ({"geglu": True}, {"C2": True}, {"m_off": 1}, {"ln": True}, {"conv": (4, 4, 8, 8, 1, 3)}, {"conv": (8, 8, 8, 8, 1, 1)})]
    grid += [c.p for c in fc.CASES if c.entry == "gemm" and not c.p.get("head_major") and not c.p.get("ln")]
    for env in (None, {"ME_GEMM_SPLITK": 0}, {"ME_GEMM_SPLITK": 8}, {"ME_GEMM_SPLITK": 9}, {"ME_GEMM_SPLITK": 100000}):
        with fr.switches(env):
            for a in grid:
                a = {k: v for k, v in a.items() if k != "env"}
                assert L.me_gemm_work_bytes(ctypes.byref(fr.gemm_struct(capi, a))) == fc.gemm_work_bytes(a, env), (a, env)
    # S itself: 1 ... 4 by the grid, never clamped by nit / 4 behind nit >= 32
    assert [fc.choose_split(dict(N=1280, K=2048), b, 32) for b in (1, 160, 213, 214, 319, 320, 399, 400, 639, 640)] == [4, 4, 4, 3, 3, 2, 2, 1, 1, 1]
    assert all(fc.choose_split(dict(N=1280, K=64 * n), 1, n) == (4 if n >= 32 else 1) for n in range(1, 70))


def _host_checks(case, t):
    """The argument checks of the case's me_* entry point (include/motioned.h; me_gemm / gemm_dispatch, me_attn, me_tattn, gn_validate, me_layernorm,
    me_softmax_rows in csrc/), restated on the case's parameters and tensors."""
    p, e = case.p, case.entry
    if e == "gemm":
        M, N, K = p["M"], p["N"], p["K"]
        assert min(M, N, K) > 0 and K % 8 == 0 and N % 4 == 0 and t["x"].shape[1] % 8 == 0
        terms = any(p.get(n) for n in ("rowvec", "res", "res2"))
        if p.get("conv"):
            Hin, Win, Hout, Wout, stride, ups, pad0 = p["conv"]
            assert min(Hin, Win, Hout, Wout) > 0 and stride in (1, 2) and 0 <= ups <= 3 and pad0 in (0, 1) and M % (Hout * Wout) == 0
            assert ups != 3 or (stride == 1 and not pad0 and (Hout, Wout) == (2 * Hin, 2 * Win) and not p.get("geglu") and t["w"].shape[1] == 16)
            assert not p.get("pieces")
        if p.get("tconv"):
            tc = p["tconv"]
            ftot, f0 = (tc[4], tc[3]) if len(tc) > 3 else (tc[0], 0)
            assert min(tc[:3]) > 0 and ftot % tc[2] == 0 and M % (tc[0] * tc[1]) == 0 and 0 <= f0 and f0 + tc[0] <= ftot
        assert not p.get("rowvec") or p["rowvec"] > 0
        assert p.get("act", 0) in (0, 1, 2) and p.get("res_rows", 0) >= 0 and p.get("res2_rows", 0) >= 0
        if p.get("geglu"):
            assert N % 32 == 0 and not terms and not p.get("act") and p.get("alpha", 1.0) == 1.0
        if p.get("head_major"):
            col0, dh = p["head_major"]
            assert not p.get("geglu") and not p.get("act") and not terms and dh % 8 == 0 and col0 % 16 == 0 and 0 <= col0 < N and (N - col0) % dh == 0 and not p.get("conv")
        if p.get("ln"):
            assert not p.get("conv") and not p.get("tconv") and not p.get("bias") and p.get("alpha", 1.0) == 1.0 and not terms and not p.get("act")
            assert 1 <= t["ln_stats"].shape[0] <= 4 and t["ln_stats"].shape[1] >= M
        if p.get("ln_out"):
            assert not p.get("geglu") and not p.get("head_major") and N % 8 == 0 and N <= 1536 and not p.get("c_pad")
        for cut in p.get("pieces") or ():
            assert 0 < cut < M
        if p.get("sel"):
            assert M % p["sel"] == 0 and (not p.get("conv") or (M // (p["conv"][2] * p["conv"][3])) % p["sel"] == 0) and not p.get("tconv")
        assert p.get("c_off", 0) in (0, 4) and p.get("c_pad", 0) % 4 == 0
    elif e == "attention":
        nseg = max(len(r) for r in p["table"])
        modes = {m for r in p.get("modes", ()) for m in r}
        assert p["dh"] in (40, 80, 160) and 1 <= nseg <= 3 and min(p["nq"], p["nk"], p["heads"]) > 0 and p.get("o_pad", 0) % 4 == 0 and p.get("o_off", 0) in (0, 4)
        assert all(r[0] >= 0 and -1 <= min(r) and max(r) < p["n_kv"] for r in p["table"])
        assert all(all(k < 0 for k in r[r.index(-1):]) for r in p["table"] if -1 in r)                      # skipped segments come last
        if modes & {1, 2}:
            assert not p.get("q_items") and not p.get("lse") and p["heads"] <= 8 and "mask" in t
        if 3 in modes:
            assert not p.get("lse") and p["heads"] * p["dh"] <= 2048
        assert not p.get("item_order") or sorted(p["item_order"]) == list(range(len(p["table"])))
        assert not p.get("q_items") or len(p["table"]) % p["q_items"] == 0
    elif e == "temporal_attention":
        assert 0 < p["batch"] <= 8 and p["dh"] % 8 == 0 and 320 % p["dh"] == 0 and (p["heads"] * p["dh"]) % 320 == 0 and case.path == fc.tattn_target(p) is not None
        qf, q0, kp, qp = p.get("q_frames", 0), p.get("q_frame0", 0), p.get("kv_parts", 1), p.get("q_parts", 1)
        assert q0 + qf <= p["frames"] and (kp <= 1 or p["frames"] % kp == 0) and (qp <= 1 or (qp == kp and not qf))
        assert all(0 <= m < p["batch"] for m in p.get("kv_map") or ())
    elif e == "groupnorm":
        assert p["C"] % 32 == 0 and p["C"] % 8 == 0 and p["C"] <= 2560 and p["rpg"] > 0 and p["nsg"] > 0
    elif e == "layernorm":
        assert p["rows"] > 0 and p["C"] % 8 == 0 and p["C"] <= 1536
    elif e == "softmax_rows":
        assert p["cols"] % 8 == 0 and p["cols"] <= 8192 and p["pad"] % 8 == 0
    else:
        raise AssertionError(f"no host checks stated for {e}")


@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: c.id)
def test_fp32_emulation_agrees_with_the_fp64_reference_inside_the_gpu_bound(case):
    """Every case satisfies its entry point's argument checks, and tests/emu_ops.py in fp32 lands inside the bound tests/test_fwd_sweep_gpu.py applies to the
    HIP kernel on the same inputs: the bound is reachable by fp32 accumulation there."""
    t = fc.build(case)
    _host_checks(case, t)
    want = ref_run(case, t)
    got = fr.run(case, fr.Emu(), t, fr.EMU)
    figures = fr.compare(case, got, want, who="fp32 emulation")
    print(case.id, case.path, {k: (f"{r:.2e}", f"{m:.2e}") for k, (r, m) in figures.items()})
    if case.p.get("pieces") and not case.p.get("pieces_only"):      # the row-range form of the reference is the one-launch form
        pieces = fr.run(case, ref, t, fr.REF, pieces=case.p["pieces"])
        assert torch.equal(pieces["y"], want["y"])


def test_ups_1_and_ups_3_cases_run_on_the_same_data():
    """Every ups = 3 case has an ups = 1 twin on the same input, terms and UNFOLDED weights; the references of the two differ by the fold's fp16 rounding of
    the weights alone (2^-11 relative per folded weight, so below 2^-11 in rel-L2)."""
    twins = [(c, fc.ups_twin(c)) for c in fc.CASES if c.entry == "gemm" and c.p.get("conv") and c.p["conv"][5] == 3]
    assert sum(t is not None for _, t in twins) >= 7
    for c3, c1 in twins:
        if c1 is None:
            continue
        t3, t1 = fc.build(c3), fc.build(c1)
        assert torch.equal(t3["x"], t1["x"]) and torch.equal(t3["w"], fc.fold_ups(t1["w"])) and all(torch.equal(t3[k], t1[k]) for k in t1 if k != "w")
        assert ups_fold_ref.rel_l2(ref_run(c3, t3)["y"], ref_run(c1, t1)["y"]) < 2.0 ** -11, c3.id


def test_the_folded_upsample_reference_is_the_definition():
    """ref64_bwd._gather_gemm at ups = 3 against tests/ups_fold_ref.py, and fwd_cases.fold_ups against the unfolded convolution (to the fold's fp16 rounding)."""
    g = torch.Generator().manual_seed(5)
    n_img, H, W, K, N = 3, 5, 7, 16, 24
    x, w9 = torch.randn(n_img * H * W, K, generator=g).half(), (torch.randn(N, 9, K, generator=g) * 0.1).half()
    w16 = fc.fold_ups(w9)
    mine = ref.gemm(x, w16, M=n_img * 4 * H * W, conv=(H, W, 2 * H, 2 * W, 1, 3, 0))
    assert float((mine - ups_fold_ref.conv_fold_ref(x, w16, n_img, H, W)).abs().max()) < 1e-12
    assert ups_fold_ref.rel_l2(mine, ups_fold_ref.conv_ups_ref(x, w9, n_img, H, W)) < 1e-3
    assert ups_fold_ref.rel_l2(ref.gemm(x, w9, M=n_img * 4 * H * W, conv=(H, W, 2 * H, 2 * W, 1, 1, 0)), ups_fold_ref.conv_ups_ref(x, w9, n_img, H, W)) < 1e-12


# ------------------------------------------------------------------------------------------------------------------ refused calls (no launch: fabricated addresses)
def test_the_forward_entry_points_refuse_what_their_kernels_rely_on():
    """tests/fwd_refused.py on addresses that are never dereferenced: every violating call returns ME_EINVAL with a message naming the entry point BEFORE
    anything is launched (tests/test_fwd_sweep_gpu.py repeats them on device buffers filled with a sentinel)."""
    if torch.cuda.is_available():      # (as tests/test_abi_cpu.py: with a device present a call that slipped through would launch on these numbers)
        pytest.skip("a device is present: the same violations run on real buffers in tests/test_fwd_sweep_gpu.py")
    import fwd_refused
    from motioneditor_amd import capi
    L = capi.lib()
    n = 0
    assert {e for e, _, _ in fwd_refused.tables(capi)} == {"me_gemm", "me_attn", "me_tattn", "me_groupnorm", "me_groupnorm_apply", "me_layernorm", "me_softmax_rows", "me_ln_stats"}
    for entry, make, bad in fwd_refused.tables(capi):
        for label, change, needle in bad:
            fake = {}
            ptr = lambda name, nbytes: fake.setdefault(name, 0x100000 * (len(fake) + 1))    # noqa: E731
            a = make(ptr)
            change(a, ptr)
            rc = fwd_refused.call(L, entry, a)
            msg = L.me_last_error().decode()
            assert rc == capi.ME_EINVAL and msg.startswith(("me_groupnorm" if entry.startswith("me_groupnorm") else entry) + ":") and needle in msg, f"{entry} ({label}): status {rc}, message {msg!r}"
            n += 1
    assert n >= 30


# ------------------------------------------------------------------------------------------------------------------ deliberately wrong emulations
class _RefAttention(fr.Emu):
    """me_attn written on the reference's per-item logits so that a mutant can change them (the arithmetic is not what the mutants are about)."""
    def mutate(self, lg, vals, p):
        return lg, vals

    def attention(self, q, k, v, *, heads, dh, n_items, nq, nk, seg_item, seg_mode, mask=None, scale=None, out=None, q_items=0, lse=None):
        scale = dh ** -0.5 if scale is None else scale
        for it, lg, vals in self.logits(q, k, v, heads=heads, dh=dh, n_items=n_items, nq=nq, nk=nk, seg_item=seg_item, seg_mode=seg_mode, mask=mask, scale=scale, q_items=q_items):
            lg, vals = self.mutate(lg, vals, dict(nk=nk))
            out[it * nq:(it + 1) * nq, :heads * dh] = (lg.softmax(-1) @ vals).permute(1, 0, 2).reshape(nq, heads * dh).to(out.dtype)
            if lse is not None:
                lse[it * nq:(it + 1) * nq] = (torch.logsumexp(lg, dim=-1) * ref.LOG2E).t()
        return out

    logits = staticmethod(ref._logits_values)


class LastKeyOfARaggedStageDropped(_RefAttention):
    def mutate(self, lg, vals, p):
        if p["nk"] % 64:
            lg = lg.clone()
            lg[..., -1] = -math.inf
        return lg, vals


class DualBinWithoutItsPlusOne(_RefAttention):
    @staticmethod
    def logits(q, k, v, *, seg_mode, **kw):
        return ref._logits_values(q, k, v, seg_mode=torch.where(seg_mode == 3, torch.zeros_like(seg_mode), seg_mode), **kw)


class DualPrevWithoutTheClampAtHeadZero(_RefAttention):
    @staticmethod
    def logits(q, k, v, *, mask, heads, **kw):
        rolled = torch.roll(mask, 1, dims=0)              # plane h - 1 for every head: head 0 reads the LAST plane instead of plane 0
        for it, lg, vals in ref._logits_values(q, k, v, mask=mask, heads=heads, **kw):
            for _, lg2, _ in ref._logits_values(q, k, v, mask=torch.cat([rolled[:1], mask[1:]]), heads=heads, **dict(kw, n_items=it + 1)):
                pass
            lg = lg.clone()
            lg[0] = lg2[0]
            yield it, lg, vals


class LastRowOfARaggedTileDropped(fr.Emu):
    def gemm(self, x, w, *, M=None, **kw):
        y = super().gemm(x, w, M=M, **kw)
        if y.shape[0] % 128:
            y[-1] = 0
        return y


class RowvecIndexOffByOne(fr.Emu):
    def gemm(self, x, w, *, rowvec=None, rows_per_vec=0, M=None, **kw):
        y = super().gemm(x, w, M=M, **kw)
        rows = y.shape[0]
        idx = ((torch.arange(rows) + 1) // rows_per_vec).clamp_max(rowvec.shape[0] - 1)
        y += rowvec.float()[idx][:, :y.shape[1]].to(y.dtype)
        return y


class ResRowsWrapIgnored(fr.Emu):
    def gemm(self, x, w, *, res=None, res_rows=0, M=None, **kw):
        y = super().gemm(x, w, M=M, **kw)
        y += res.float()[torch.arange(y.shape[0]).clamp_max(res.shape[0] - 1), :y.shape[1]].to(y.dtype)
        return y


class AlphaAppliedAfterTheBias(fr.Emu):
    def gemm(self, x, w, *, bias=None, alpha=1.0, res=None, M=None, **kw):
        y = super().gemm(x, w, M=M, alpha=1.0, bias=bias, **kw).float() * alpha
        return (y + res.float()[:y.shape[0], :y.shape[1]]).to(x.dtype)


class ConvPad0Ignored(fr.Emu):
    def gemm(self, x, w, *, conv=None, **kw):
        return super().gemm(x, w, conv=tuple(conv[:6]) + (0,), **kw)


class Ups3ParitySwapped(fr.Emu):
    def ups3_tap(self, wf, py, px, ty, tx):
        return wf[:, 4 * (2 * px + py) + 2 * ty + tx]


class CausalDiagonalExcluded(fr.Emu):
    def temporal_attention(self, q, k, v, *, heads, dh, batch, frames, npix, scale=None, **kw):
        C = heads * dh
        shp = lambda t: t.float()[:, :C].reshape(batch, frames, npix, heads, dh).permute(0, 2, 3, 1, 4)   # noqa: E731
        s = (shp(q) @ shp(k).transpose(-1, -2)) * (dh ** -0.5 if scale is None else scale)
        s = s.masked_fill(torch.arange(frames)[None, :] >= torch.arange(frames)[:, None].clamp_min(1), -math.inf)      # frame 0 keeps its own key: no empty row
        return (s.softmax(-1) @ shp(v)).permute(0, 3, 1, 2, 4).reshape(batch * frames * npix, C)


class KvMapIgnored(fr.Emu):
    def temporal_attention(self, q, k, v, *, kv_map=None, **kw):
        return emu_ops.temporal_attention(q, k, v, kv_map=None, **kw)


MUTANTS = {
    "the last key of a ragged stage dropped": (LastKeyOfARaggedStageDropped, "attn-40-4w-nk17-nq127"),
    "the last row of a ragged tile dropped": (LastRowOfARaggedTileDropped, "gemm-g128x64-dense-M129"),
    "rowvec row index off by one at a rows_per_vec boundary": (RowvecIndexOffByOne, "gemm-epi-8p256-rpv-255"),
    "res_rows wrap ignored": (ResRowsWrapIgnored, "gemm-epi-8p256-res-rows-96"),
    "alpha applied after the bias": (AlphaAppliedAfterTheBias, "gemm-epi-8p256-alpha"),
    "DUAL_PREV head not clamped at head 0": (DualPrevWithoutTheClampAtHeadZero, "attn-general-dual-dh40-prev-clamp"),
    "the + 1 of DUAL_BIN left out of the denominator": (DualBinWithoutItsPlusOne, "attn-dual-bin-dh40-h8-nq130-nk9"),
    "the causal diagonal excluded": (CausalDiagonalExcluded, "tattn-mfma-F7-dh40"),
    "kv_map ignored": (KvMapIgnored, "tattn-mfma-npix1-batch8-dh40"),
    "conv pad0 ignored": (ConvPad0Ignored, "gemm-conv-s2-pad0"),
    "ups = 3 parity swapped": (Ups3ParitySwapped, "gemm-conv-ups3-128x64"),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_a_deliberately_wrong_emulation_fails_its_named_case(name):
    """The case named for a mutant passes on the emulation proper (the test above) and fails on the mutant: the table can tell the two apart."""
    cls, cid = MUTANTS[name]
    case = fc.BY_ID[cid]
    t = fc.build(case)
    want = ref_run(case, t)
    with pytest.raises(AssertionError) as exc:
        fr.compare(case, fr.run(case, cls(), t, fr.EMU), want, who=name)
    print(f"mutant '{name}' caught by case {cid}: {str(exc.value).splitlines()[0][:160]}")
    if not issubclass(cls, _RefAttention):
        return
    fr.compare(case, fr.run(case, _RefAttention(), t, fr.EMU), want, who="unmutated")      # the vehicle itself is right
