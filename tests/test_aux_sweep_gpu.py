"""The third sweep on a real MI355X: every case of tests/aux_cases.py on the HIP library (csrc/tune.hip, csrc/eltwise.hip, csrc/clip.hip, csrc/train.hip's refresh)
against the fp64 reference of tests/ref64_aux.py, inside the bound its entry point already states; the kernel each launch took against the one the restated
dispatch predicts (me_last_kernel); every output a guard-banded view (tests/guard.py) whose bands are intact afterwards, every accumulated-into operand likewise; and
the bitwise promises: the same call twice, each _dev variant against its host-scalar twin, the refreshed weights against weights.Packed, the causal attention's
row 0 and its blindness to later keys.  Every launch is a legal one: the refused calls never reach the device (tests/test_aux_sweep_cpu.py has already shown, without
one, that each is refused on the host).  No child processes, no switches read once per process."""
import pytest
import torch

import aux_cases as ac
import aux_run as ar
import guard
import ref64_aux as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the HIP library is the only compute path")
    from motioneditor_amd import capi, ops as _ops
    capi.lib()  # fails loudly when libmotioned.so is missing
    return _ops


def guarded(intacts):
    """aux_run.Exchange for the device: inputs move as they are; an output is columns [0, cols) of a sentinel-filled [rows, cols + pad] allocation with guard
    elements before and after; an in-out operand keeps its values inside a NaN-filled allocation whose surroundings must stay bitwise what they were."""
    def out(rows, cols, dtype, pad=0, computed_=True):
        base, intact = guard.sentinel_out((rows, cols + pad), dtype, contiguous=True)
        sentinel = guard._signed(guard.SENTINEL[dtype], dtype)

        def columns_beside_the_view():
            assert bool((guard.bits(base)[:, cols:] == sentinel).all()), "columns beside the output view were written"
        intacts.extend((intact, columns_beside_the_view))
        return base[:, :cols]

    def inout(t):
        view = guard.embed_in(t, device="cuda", contiguous=True)
        snap = guard.bits(view.guard.buf).clone()
        intacts.append(lambda: view.guard.outside_intact(snap, "in-out operand"))
        return view
    return ar.Exchange(lambda t: t.cuda(), out, inout)


def launch(ops, case, t, **kw):
    seen, intacts = [], []
    got = ar.run(case, ops, t, guarded(intacts), hook=lambda: seen.append(ops._last_kernel()), **kw)
    torch.cuda.synchronize()
    for intact in intacts:
        intact()
    return got, seen


@pytest.mark.parametrize("case", ac.CASES, ids=lambda c: c.id)
def test_hip_kernel_matches_the_fp64_reference(ops, case):
    p = case.p
    t = ac.build(case)
    want = ar.run(case, ref, t, ar.REF)
    got, seen = launch(ops, case, t)
    assert seen and (case.path is None or ar.kernel_matches(seen[-1], case.path)), f"{case.id}: the restated dispatch predicts {case.path}, the launch took {seen}"
    figures = ar.compare(case, got, want, who="HIP", t=t)
    print(case.id, seen[-1], {k: (f"{r:.2e}", f"{m:.2e}") for k, (r, m) in figures.items()})
    if case.twice:                # fixed-order reductions, no atomics: the same call twice is bitwise the same
        again, _ = launch(ops, case, t)
        for name in got:
            assert ar.bitwise_equal(got[name], again[name]), f"{case.id}: {name} differs between two identical calls"
    if case.entry in ac.STEP_TWINS:       # the device-resident step parameters: bitwise the host-scalar launch
        twin, seen = launch(ops, case, t, dev_params=True)
        assert ar.kernel_matches(seen[-1], case.path + "<dev>") and ar.bitwise_equal(twin["y"], got["y"]), f"{case.id}: the _dev variant differs from its twin ({seen})"
    if case.entry == "attention_causal":  # what tests/test_clip_gpu.py test_attn_causal states, per case
        nq, n_seq, C = p["nq"], p["n_seq"], p["heads"] * 64
        o = got["o"].reshape(n_seq, nq, C)
        assert torch.equal(o[:, 0], t["qkv"][:, 2 * C:].reshape(n_seq, nq, C)[:, 0]), f"{case.id}: position 0 sees only itself, O[s, 0] = V[s, 0] exactly"
        t2 = dict(qkv=t["qkv"].clone())
        t2["qkv"].reshape(n_seq, nq, 3 * C)[:, nq - 1, C:] = 7.0
        o2 = launch(ops, case, t2)[0]["o"].reshape(n_seq, nq, C)
        assert ar.bitwise_equal(o2[:, :nq - 1], o[:, :nq - 1]), f"{case.id}: the last key / value row reached an earlier query"


def test_round_trip_through_the_layout_converters_is_exact(ops):
    """fp16-representable NCHW data -> rows -> NCHW, at every (C, npix) of the table, through strided planes and a wide row pitch."""
    for C in (3, 4, 8):
        for npix in (1, 85, 256):
            x = (torch.randn(3, C, npix + 3, generator=torch.Generator().manual_seed(C * 1000 + npix)) * 2).half().float()
            rows = torch.full((3 * npix, C + 8), float("nan"), dtype=torch.float16, device="cuda")
            back = torch.full((3, C, npix + 5), float("nan"), device="cuda")
            from motioneditor_amd import capi
            d = x.cuda()
            capi.check(capi.lib().me_nchw_to_rows(rows.data_ptr(), C + 8, d.data_ptr(), C * (npix + 3), npix + 3, 3, C, npix, ops._stream()), "me_nchw_to_rows")
            capi.check(capi.lib().me_rows_to_nchw(back.data_ptr(), C * (npix + 5), npix + 5, rows.data_ptr(), C + 8, 3, C, npix, ops._stream()), "me_rows_to_nchw")
            torch.cuda.synchronize()
            assert torch.equal(back[:, :, :npix].cpu(), x[:, :, :npix]) and bool(torch.isnan(back[:, :, npix:]).all()) and bool(torch.isnan(rows[:, C:]).all()), (C, npix)


def test_geometry_restatement_matches_the_library_host_functions(ops):
    """The Python restatement that placed the edges of the table, against the library this machine runs (host functions: no launch)."""
    from motioneditor_amd import capi
    L = capi.lib()
    for c in ac.CASES:
        p = c.p
        if c.entry == "conv_dw":
            assert L.me_conv_dw_splits(p["M"], p["N"], p["K"]) == ac.cw_geometry(p["M"], p["N"], p["K"])[0], c.id
            assert L.me_conv_dw_work_bytes(p["M"], p["N"], p["K"]) == ac.cw_work_bytes(p["M"], p["N"], p["K"]), c.id
        if c.entry == "gn_params":
            args = (p["rpg"] * p["nsg"], p["rpg"], p["C"], p["groups"])
            assert L.me_groupnorm_bwd_params_work_bytes(*args) == ac.gn_params_work_bytes(*args), c.id
    for N, K, lim in ac.CW_EDGE_SHAPES:
        for M in range(1, lim, 61):
            assert L.me_conv_dw_work_bytes(M, N, K) == ac.cw_work_bytes(M, N, K), (M, N, K)


def test_refused_calls_leave_sentinel_filled_buffers_untouched(ops):
    """aux_run.refused on device buffers: every violating call returns ME_EINVAL with a message naming the entry point, and every buffer of the call holds its
    sentinel bytes afterwards; through the wrappers the same violations raise."""
    from motioneditor_amd import capi
    L = capi.lib()
    for entry, make, bad in ar.refused(capi):
        bufs = {}

        def ptr(name, nbytes):
            if name not in bufs:
                bufs[name] = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            return bufs[name].data_ptr()
        for label, change, needle in bad:
            a = make(ptr)
            change(a, ptr)
            rc = ar.call_refused(L, entry, a)
            msg = L.me_last_error().decode()
            assert rc == capi.ME_EINVAL and msg.startswith(entry + ":") and needle in msg, f"{entry} ({label}): status {rc}, message {msg!r}"
        torch.cuda.synchronize()
        assert bufs and all(bool((b == 0xA5).all()) for b in bufs.values()), f"{entry}: a refused call wrote to one of its buffers"
    x = torch.zeros((2 * 129, 3 * 320), dtype=torch.float16, device="cuda")
    with pytest.raises(ValueError, match="128"):
        ops.attention_causal(x[:, :320], x[:, 320:640], x[:, 640:], heads=5, dh=64, n_seq=2, nq=129)
    dst = torch.full((40, 9, 72), 5.0, device="cuda")
    with pytest.raises(ValueError, match="pad0"):
        ops.gemm_dw(torch.zeros((70, 40), device="cuda"), torch.zeros((70, 72), dtype=torch.float16, device="cuda"), dst=dst, taps=9, K=72, M=70, conv=(5, 7, 5, 7, 1, 0, 1))
    assert bool((dst == 5.0).all())
