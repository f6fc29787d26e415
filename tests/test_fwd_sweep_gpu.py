"""The forward sweep on a real MI355X: every case of tests/fwd_cases.py on the HIP library (csrc/gemm.hip, csrc/attn.hip, csrc/tattn.hip, csrc/norm.hip)
against the fp64 reference of tests/ref64_fwd.py, inside the bound its entry point already states; the kernel EVERY launch of the case took against the one
the restated dispatch predicts (me_last_kernel); every output in a guard-banded view (tests/guard.py) whose bands are intact afterwards -- the head-major
panels excepted, which ops.gemm allocates itself; and the bitwise properties the code promises: the same call twice, a sub-batch that selects its kernel
as the full launch (sel_rows), row-range pieces (m_off) against the one-launch form, a permuted item_order against the ascending one.  The per-call switches
of a case are set around its launches and put back.  Every launch is a legal one: the refused calls never reach the device (tests/test_fwd_sweep_cpu.py has
already shown, without one, that each is refused on the host)."""
import pytest
import torch

import fwd_cases as fc
import fwd_refused
import fwd_run as fr
import guard
import ref64_fwd as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the HIP library is the only compute path")
    from motioneditor_amd import capi, ops as _ops
    capi.lib()  # fails loudly when libmotioned.so is missing
    return _ops


def guarded(intacts):
    """fwd_run.Exchange for the device: inputs move as they are, every output is a view inside a sentinel-filled allocation; intacts collects the checks."""
    def out(rows, cols, ld_pad, off, dtype):
        if dtype == torch.float32:                                 # (the log-sum-exp: contiguous by its contract)
            view, intact = guard.sentinel_out((rows, cols), dtype, contiguous=True)
            intacts.append(intact)
            return view
        wide = cols + ld_pad + (8 if off else 0)
        base, intact = guard.sentinel_out((rows, wide), dtype, contiguous=bool(ld_pad % 8))      # ld % 8 != 0 needs a pitch of its own
        sentinel = guard._signed(guard.SENTINEL[dtype], dtype)

        def columns_beside_the_view():
            b = guard.bits(base)
            assert bool((b[:, :off] == sentinel).all()) and bool((b[:, off + cols:] == sentinel).all()), "columns beside the output view were written"
        intacts.extend((intact, columns_beside_the_view))
        return base[:, off:off + cols]
    return fr.Exchange(lambda t: t.cuda(), torch.float16, out)


def launch(ops, case, t, want_kernel=True, **kw):
    seen, intacts = [], []
    got = fr.run(case, ops, t, guarded(intacts), hook=lambda stage: seen.append(ops._last_kernel()), **kw)
    torch.cuda.synchronize()
    for intact in intacts:
        intact()
    if want_kernel and case.path:
        want = case.p.get("paths") or [case.path] * len(seen)
        assert seen and len(seen) == len(want) and all(fr.kernel_matches(k, w) for k, w in zip(seen, want)), f"{case.id}: the restated dispatch predicts {want}, the launches took {seen}"
    return got


@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: c.id)
def test_hip_kernel_matches_the_fp64_reference(ops, case):
    p = case.p
    t = fc.build(case)
    want = fr.run(case, ref, t, fr.REF)
    main = dict(pieces=p["pieces"]) if p.get("pieces_only") else {}
    with fr.switches(p.get("env")):
        if "fallback" in p:
            ops.attention_fallback_blocks(reset=True)
        got = launch(ops, case, t, **main)
        if "fallback" in p:       # padded zero queries of the ragged last block must not trip the fixed-offset softmax's fallback, saturating real ones must
            blocks = ops.attention_fallback_blocks()
            assert (blocks > 0) == p["fallback"], f"{case.id}: {blocks} blocks fell back to the running-maximum sweep"
        figures = fr.compare(case, got, want, who="HIP")
        print(case.id, case.path, {k: (f"{r:.2e}", f"{m:.2e}") for k, (r, m) in figures.items()})
        if case.twice:            # fixed-order reductions: the same call twice is bitwise the same
            again = launch(ops, case, t, **main)
            for name in got:
                assert fr.bitwise_equal(got[name], again[name]), f"{case.id}: {name} differs between two identical calls"
        if p.get("sel"):          # a sub-batch that selects its kernel as the full launch would is bitwise the same rows (split-K included)
            sub = launch(ops, case, t, sub=p["sel"])
            rows = sub["y"].shape[0]
            assert rows == p["M"] // p["sel"] and fr.bitwise_equal(sub["y"], got["y"][:rows]), f"{case.id}: the first {rows} rows as a sub-batch differ from the full launch"
        if p.get("pieces") and not p.get("pieces_only"):      # row-range pieces land on the kernel of the unsplit launch and give its rows
            pieces = launch(ops, case, t, pieces=p["pieces"])
            assert fr.bitwise_equal(pieces["y"], got["y"]), f"{case.id}: row-range pieces {p['pieces']} differ from the one-launch form"
        if p.get("item_order"):   # scheduling only
            ascending = launch(ops, case, t, order=False)
            assert fr.bitwise_equal(ascending["o"], got["o"]), f"{case.id}: item_order changed the output"


def test_ups_3_against_ups_1_on_the_same_data(ops):
    """The folded launch against the unfolded one on one input, both on the device: they differ by the fold's fp16 rounding of the weights (2^-11 relative per
    weight) and two fp16 roundings of the outputs (2^-11 each), so the entry point's rel-L2 of 2e-3 = 4.1 x 2^-11 holds between them."""
    n = 0
    for c3 in fc.CASES:
        c1 = fc.ups_twin(c3) if c3.entry == "gemm" else None
        if c1 is None:
            continue
        with fr.switches(c3.p.get("env")):
            y3 = launch(ops, c3, fc.build(c3))["y"]
        with fr.switches(c1.p.get("env")):
            y1 = launch(ops, c1, fc.build(c1))["y"]
        r, m = fr.errors(y3, y1)
        print(c3.id, "against", c1.id, f"rel-L2 {r:.2e} max/mean {m:.2e}")
        assert r <= fc.REL_L2, (c3.id, r)
        n += 1
    assert n >= 7


def test_split_k_falls_back_to_the_same_result_when_its_scratch_is_short_or_misaligned(ops):
    """csrc/gemm.hip:1750: one byte short, or 8 bytes off 16: the unsplit launch -- bitwise the launch with ME_GEMM_SPLITK=0."""
    off = fc.BY_ID["gemm-splitk-off"]
    t = fc.build(off)
    with fr.switches(off.p["env"]):
        whole = launch(ops, off, t)
    for cid in ("gemm-splitk-work-short", "gemm-splitk-work-misaligned"):
        case = fc.BY_ID[cid]
        assert {k: v for k, v in case.p.items() if k != "work"} == {k: v for k, v in off.p.items() if k != "env"}
        got = launch(ops, case, fc.build(off))
        assert fr.bitwise_equal(got["y"], whole["y"]), cid


def test_choose_split_restatement_matches_the_library_on_this_machine(ops):
    import ctypes
    from motioneditor_amd import capi
    for c in fc.CASES:
        if c.entry == "gemm" and not c.p.get("head_major") and not c.p.get("ln"):
            with fr.switches(c.p.get("env")):
                a = {k: v for k, v in c.p.items() if k != "env"}
                assert capi.lib().me_gemm_work_bytes(ctypes.byref(fr.gemm_struct(capi, a))) == fc.gemm_work_bytes(a, c.p.get("env")), c.id


def test_refused_forward_calls_leave_sentinel_filled_buffers_untouched(ops):
    """tests/fwd_refused.py on device buffers: every violating call returns ME_EINVAL with a message naming the entry point, and every buffer of the call holds
    its sentinel bytes afterwards."""
    from motioneditor_amd import capi
    L = capi.lib()
    for entry, make, bad in fwd_refused.tables(capi):
        bufs = {}

        def ptr(name, nbytes):
            if name not in bufs:
                bufs[name] = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            return bufs[name].data_ptr()
        for label, change, needle in bad:
            a = make(ptr)
            change(a, ptr)
            rc = fwd_refused.call(L, entry, a)
            msg = L.me_last_error().decode()
            assert rc == capi.ME_EINVAL and needle in msg, f"{entry} ({label}): status {rc}, message {msg!r}"
        torch.cuda.synchronize()
        assert bufs and all(bool((b == 0xA5).all()) for b in bufs.values()), f"{entry}: a refused call wrote to one of its buffers"
    r = fc.TATTN_REFUSED_THREADS
    C = r["heads"] * r["dh"]
    q = torch.zeros((r["batch"] * r["frames"] * r["npix"], C), dtype=torch.float16, device="cuda")
    with pytest.raises(ValueError, match="512 threads"):
        ops.temporal_attention(q, q, q, **r)
