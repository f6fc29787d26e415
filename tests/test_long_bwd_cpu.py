"""The temporal-attention backward above 64 frames, without a GPU: the case table of tests/long_bwd_cases.py against itself; the emulation of the kernels as
built (stage-wise online lse / delta, fp16 P / dS / dout, fp32 accumulation) against the fp64 reference on every case inside the case's bound, with every
recorded floor re-measured; five deliberately wrong emulations, each failing a named case; the ABI table of include/motioned_long.h (capi.LONG_SYMBOLS)
with the rules tests/test_tune_conv_cpu.py applies to its table; and the argument contract of me_tattn_bwd_long on the host."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

import bwd_cases as bc
import bwd_run as br
import long_bwd_cases as lb
import ref64_bwd as ref

ROOT = Path(__file__).resolve().parents[1]
ENTRY_BOUND = bc.BOUNDS["temporal_attention_bwd"]


# ------------------------------------------------------------------ the table
def test_the_table_holds_every_edge_and_states_its_bounds():
    ids = [c.id for c in lb.CASES]
    assert len(ids) == len(set(ids)) and set(lb.GUARDED) <= set(lb.BY_ID)
    assert {lb.BY_ID[i].p["dh"] for i in lb.GUARDED} == set(lb.LONG_DH)
    assert all(c.entry == "temporal_attention_bwd" and c.twice and c.path == lb.target(c.p) and lb.MIN_FRAMES <= c.p["frames"] <= lb.MAX_FRAMES for c in lb.CASES)
    edges = {(c.p["dh"], c.p["frames"], c.p["kind"]) for c in lb.CASES if c.id.startswith("lbwd-F")}
    assert edges == {(dh, F, k) for dh in lb.LONG_DH for F in lb.FRAME_EDGES for k in lb.KINDS} and lb.FRAME_EDGES == (65, 72, 128, 129, 136, 200, 256)
    assert all(c.p["npix"] == 3 and c.p["batch"] == 2 and c.p["heads"] == 320 // c.p["dh"] for c in lb.CASES if c.id.startswith("lbwd-F"))
    p = lambda i: lb.BY_ID[i].p    # noqa: E731
    assert p("lbwd-fused-qkv-dout-padded")["fused"] and p("lbwd-fused-qkv-dout-padded")["do_pad"] % 4 == 0 and p("lbwd-scale")["scale"] and p("lbwd-npix1")["npix"] == 1
    assert p("lbwd-heads-twice-the-slice")["heads"] == 2 * (320 // p("lbwd-heads-twice-the-slice")["dh"]) and p("lbwd-zero-block")["zero_block"]
    # the dispatch at the seam: bwd_cases' kernels up to 64 frames, the key-tiled pair above
    assert lb.target(dict(frames=64, dh=40, heads=8)) == bc.tattn_bwd_path(64, 40, 8) == "tattn_bwd_kernel"
    assert lb.target(dict(frames=65, dh=40, heads=8)) == "tattn_bwd_long_dq_kernel<40>+tattn_bwd_long_dkv_kernel<40>"
    # bounds: the entry point's own, or (bwd_cases.py, `bound=`) per figure the larger of it and FACTOR x the recorded floor, all three written into the entry
    assert lb.FACTOR == 4 and set(lb.FLOORS) <= set(lb.BY_ID)
    for c in lb.CASES:
        if c.id in lb.FLOORS:
            fl = lb.FLOORS[c.id]
            assert c.p["floor"] == fl and c.p["factor"] == 4 and (fl[0] > ENTRY_BOUND[0] or fl[1] > ENTRY_BOUND[1])
            assert c.bound == (max(ENTRY_BOUND[0], 4 * fl[0]), max(ENTRY_BOUND[1], 4 * fl[1]))
        else:
            assert c.bound is None and br.bound_of(c, "dq") == ENTRY_BOUND == (2e-3, 2e-2)


# ------------------------------------------------------------------ the emulation of the kernels as built
_shared = {}


def _inputs_and_reference(case):
    """Built once per case and shared by the tests below; never modified."""
    if case.id not in _shared:
        t = lb.build(case)
        _shared[case.id] = (t, br.run(case, ref, t, br.to_ref))
    return _shared[case.id]


@pytest.mark.parametrize("case", lb.CASES, ids=lambda c: c.id)
def test_emulation_of_the_kernels_agrees_with_the_fp64_reference(case):
    t, want = _inputs_and_reference(case)
    assert all(bool(torch.isfinite(v).all()) for v in t.values())
    got = br.run(case, lb.Emu(), t, br.to_emu)
    figs = {n: br.errors(got[n], want[n]) for n in sorted(want)}
    print(case.id, "bound", br.bound_of(case, "dq"), {n: (f"{r:.2e}", f"{m:.2e}") for n, (r, m) in figs.items()})
    br.compare(case, got, want, who="emulation", device_types=False)
    worst = (max(f[0] for f in figs.values()), max(f[1] for f in figs.values()))
    if case.id in lb.FLOORS:     # the recorded floor is this measurement (fp16 roundings dominate it: it does not depend on the machine's fp32 summation order)
        for rec, now, lim in zip(lb.FLOORS[case.id], worst, ENTRY_BOUND):
            if rec > lim:
                assert 0.8 * rec <= now <= 1.25 * rec, f"{case.id}: the recorded floor {rec:.2e} is not what the emulation measures, {now:.2e}"
    else:
        assert worst[0] <= ENTRY_BOUND[0] and worst[1] <= ENTRY_BOUND[1]
    if case.p.get("zero_block"):
        z = lb.zeroed_rows(case.p)
        assert float(got["dq"][z].abs().max()) == 0.0 and float(got["dq"].abs().max()) > 0.0
        assert float(t["dout"][z].abs().max()) > 0.0 and float(t["dout"][z].half().abs().max()) == 0.0


# ------------------------------------------------------------------ mutants
MUTANTS = [
    ("the online delta is not rescaled when the maximum moves", dict(delta_no_rescale=True), "lbwd-F136-dh40-rising"),
    ("sweep 2 weighs P by the maximum of the first stage", dict(stale_max=True), "lbwd-F136-dh80-rising"),
    ("the causal mask admits the frame after the query", dict(mask_shift=1), "lbwd-F72-dh40-soft"),
    ("a key block starts at its second query stage", dict(skip_first_query_stage=True), "lbwd-F129-dh160-soft"),
]


@pytest.mark.parametrize("what,flags,cid", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_a_deliberately_wrong_emulation_fails_its_case(what, flags, cid):
    case = lb.BY_ID[cid]
    t, want = _inputs_and_reference(case)
    with pytest.raises(AssertionError):
        br.compare(case, br.run(case, lb.Emu(**flags), t, br.to_emu), want, who=what, device_types=False)


@pytest.mark.parametrize("cid", [c.id for c in lb.CASES if c.p.get("zero_block")])
def test_delta_from_the_unrounded_dout_fails_the_exact_zero_case(cid):
    """The reference's dq of those queries is ~ 1e-8 (their dout is 2^-27 N(0, 1)): inside every bound.  What tells the mutant apart is the exact zero."""
    case = lb.BY_ID[cid]
    t, want = _inputs_and_reference(case)
    got = br.run(case, lb.Emu(delta_unrounded=True), t, br.to_emu)
    br.compare(case, got, want, who="delta from the unrounded dout", device_types=False)
    assert float(got["dq"][lb.zeroed_rows(case.p)].abs().max()) > 0.0


# ------------------------------------------------------------------ the ABI table of include/motioned_long.h
LAUNCHING = {"me_tattn_bwd_long"}


def test_long_symbols_are_declared_exported_and_apart_from_the_other_tables():
    from motioneditor_amd import build, capi
    build.build_lib(verbose=False)
    assert "tattn_bwd_long.hip" in build.SOURCES
    assert not set(capi.LONG_SYMBOLS) & (set(capi.SYMBOLS) | set(capi.IO_SYMBOLS) | set(capi.TUNE_SYMBOLS))
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "motioned_long.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(me_[a-z0-9_]+)\s*\(", header))
    assert declared == set(capi.LONG_SYMBOLS) == LAUNCHING | {"me_tattn_bwd_long_work_bytes"}
    L = ctypes.CDLL(str(capi.LIB_PATH))
    for name in declared:
        getattr(L, name)
    bound = capi.lib()
    for name, (res, args) in capi.LONG_SYMBOLS.items():
        assert getattr(bound, name).argtypes == args and getattr(bound, name).restype is res
    assert bound.me_abi_version() == capi.ABI_VERSION == 9
    for other in ("motioned.h", "motioned_io.h", "motioned_tune.h"):
        assert not any(name in (ROOT / "include" / other).read_text() for name in declared)
    # me_tattn_bwd_long = the arguments of me_tattn_bwd, then work, work_bytes, stream
    assert capi.LONG_SYMBOLS["me_tattn_bwd_long"][1][:-3] == capi.SYMBOLS["me_tattn_bwd"][1][:-1]


def test_every_launching_long_symbol_is_named_by_a_guard_case():
    from motioneditor_amd import capi
    import test_guard_long_bwd_gpu
    guarded = set()
    for syms in test_guard_long_bwd_gpu.GUARDED.values():
        guarded |= set(syms)
    assert guarded <= set(capi.LONG_SYMBOLS), sorted(guarded - set(capi.LONG_SYMBOLS))
    assert not LAUNCHING - guarded, f"entries without a guard case: {sorted(LAUNCHING - guarded)}"
    assert set(capi.LONG_SYMBOLS) - guarded <= {"me_tattn_bwd_long_work_bytes"}


# ------------------------------------------------------------------ the argument contract, on the host
def _call(L, **over):
    heads, dh, npix, batch, frames = 8, 40, 2, 1, 72
    a = dict(dq=0x100000, lddq=320, dk=0x200000, lddk=320, dv=0x300000, lddv=320, q=0x400000, ldq=320, k=0x500000, ldk=320, v=0x600000, ldv=320, dout=0x700000, lddo=320,
             batch=batch, frames=frames, npix=npix, heads=heads, dh=dh, scale=dh ** -0.5, work=0x800000, work_bytes=None)
    a.update(over)
    if a["work_bytes"] is None:
        a["work_bytes"] = lb.work_bytes(a["batch"], a["frames"], a["npix"], a["heads"])
    rc = L.me_tattn_bwd_long(*a.values(), None)
    return rc, L.me_last_error().decode()


REFUSED = [("64 frames", dict(frames=64), "> 64"), ("257 frames", dict(frames=257), "<= 256"), ("head dim 48", dict(dh=48), "40, 80 or 160"),
           ("null work", dict(work=None), "work"), ("misaligned work", dict(work=0x800008), "work"), ("undersized work", dict(work_bytes=8 * 72 * 2 * 8 - 1), "work_bytes"),
           ("null dq", dict(dq=None), "null"), ("no heads", dict(heads=0), "sizes"), ("no pixels", dict(npix=0), "sizes"),
           ("ldq not a multiple of 8", dict(ldq=324), "multiples"), ("lddo not a multiple of 4", dict(lddo=322), "multiples"),
           ("ldk narrower than heads * dh", dict(ldk=312), "cover"), ("lddv narrower than heads * dh", dict(lddv=316), "cover"),
           ("q misaligned", dict(q=0x400008), "misaligned"), ("dout misaligned", dict(dout=0x700004), "misaligned")]


@pytest.mark.parametrize("label,over,word", REFUSED, ids=[r[0] for r in REFUSED])
def test_me_tattn_bwd_long_refuses_on_the_host(label, over, word):
    """Fabricated addresses: a call that were not refused before its launch would come back ME_EHIP (or fault), not ME_EINVAL."""
    from motioneditor_amd import capi
    rc, msg = _call(capi.lib(), **over)
    assert rc == capi.ME_EINVAL and msg.startswith("me_tattn_bwd_long:") and word in msg, (label, rc, msg)


def test_work_bytes_match_their_restatement():
    from motioneditor_amd import capi
    L = capi.lib()
    for c in lb.CASES:
        a = (c.p["batch"], c.p["frames"], c.p["npix"], c.p["heads"])
        assert L.me_tattn_bwd_long_work_bytes(*a) == lb.work_bytes(*a) == 8 * a[0] * a[1] * a[2] * a[3], c.id
    assert L.me_tattn_bwd_long_work_bytes(1, 96, 4096, 8) == 8 * 96 * 4096 * 8
    assert L.me_tattn_bwd_long_work_bytes(8, 256, 65536, 32) == 8 * 8 * 256 * 65536 * 32      # beyond 2^31: 64-bit
    assert L.me_tattn_bwd_long_work_bytes(0, 72, 1, 1) == lb.work_bytes(0, 72, 1, 1) == 0
