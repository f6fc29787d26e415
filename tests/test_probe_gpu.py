"""ops.attention_probs / me_attn_probs (csrc/attn_probs.hip) on a real MI355X against the fp64 restatement (tests/ref64_probe.py) on the same fp16 inputs,
over the cases of tests/probe_cases.py.  The bound of a case is a maximum absolute error: 4 x the error of the fp32 emulation on that case (measured on the
CPU of the same run, probe_cases.emu_error) + 2e-6.  Each case also asserts: finite results from a NaN-filled P (beta == 0 reads nothing), the pad columns
>= nk untouched, every row summing to 1 (3 after three beta = 1 calls) within the bound, two runs bitwise equal, me_last_kernel() naming the kernel."""
import pytest
import torch

import probe_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the HIP library is the only compute path")
    from motioneditor_amd import capi, ops as _ops
    capi.lib()
    return _ops


@pytest.mark.parametrize("cid", [c.id for c in pc.CASES])
def test_kernel_against_fp64(ops, cid):
    from motioneditor_amd import capi
    c = pc.BY_ID[cid]
    t = pc.build(c)
    want, bound = pc.reference(c), pc.bound(c)
    capi.lib().me_set_kernel(b"")
    got, P, pad = pc.run(c, ops.attention_probs, t, device="cuda")
    again = pc.run(c, ops.attention_probs, t, device="cuda")[0]
    torch.cuda.synchronize()
    kernel = capi.lib().me_last_kernel().decode()
    got, again, P = got.cpu(), again.cpu(), P.cpu()
    assert torch.isfinite(got).all(), "a NaN of P or of a pad row reached the result"
    err = float((got.double() - want).abs().max())
    calls = 1 if c.beta == 0 else 3
    sums = float((got.double().sum(1) - calls).abs().max())
    print(f"{cid}: {kernel}: max |err| {err:.3e} (bound {bound:.3e} = 4 x {pc.emu_error(c):.3e} + 2e-6), row sums off by {sums:.3e}")
    assert kernel == f"attn_probs_kernel<{c.dh}>"
    assert bool((P[:, c.nk:] == pad).all()), "columns >= nk were written"
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "two calls differ bitwise"
    assert err <= bound, f"{cid}: max |err| {err:.3e} > {bound:.3e}"
    assert sums <= bound, f"{cid}: row sums off by {sums:.3e} > {bound:.3e}"


def test_alpha_scales_and_a_recording_plan_captures_the_launch(ops):
    """alpha multiplies the mean; the launch goes through the library's launch hook (a recording plan holds exactly this one launch)."""
    import ctypes
    from motioneditor_amd import capi
    c = pc.BY_ID["ldp80"]
    t = pc.build(c)
    q, k, kv = pc.to_device(t["q"], "cuda"), pc.to_device(t["k"], "cuda"), t["kv_item"].cuda()
    one = torch.zeros((c.n_items * c.nq, 80), dtype=torch.float32, device="cuda")
    half = torch.zeros_like(one)
    ops.attention_probs(q, k, kv_item=kv, out=one, **t["kw"])
    L = capi.lib()
    plan = ctypes.c_void_p()
    capi.check(L.me_plan_begin(ctypes.byref(plan), ops._stream()), "me_plan_begin")
    try:
        ops.attention_probs(q, k, kv_item=kv, out=half, alpha=0.5, **t["kw"])
    finally:
        capi.check(L.me_plan_end(plan), "me_plan_end")
    st = capi.PlanStats()
    capi.check(L.me_plan_info(plan, ctypes.byref(st)), "me_plan_info")
    L.me_plan_destroy(plan)
    torch.cuda.synchronize()
    assert st.launches == 1
    assert torch.equal(half[:, :c.nk], one[:, :c.nk] * 0.5)     # a power of two: exact
