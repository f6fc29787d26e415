"""The backward / training sweep on a real MI355X: every case of tests/bwd_cases.py on the HIP library (csrc/bwd.hip, csrc/attn_bwd.hip, csrc/train.hip) against
the fp64 reference of tests/ref64_bwd.py, inside the bound its entry point already states; the kernel each launch took where the launcher names it; memory
outside strided views bitwise untouched; the non-finite contract of me_sumsq_absmax / me_adamw and of the trainers that rest on it; and the argument
contract of the backward ABI with sentinel-filled outputs.  Every launch is a legal one; tests/test_bwd_sweep_cpu.py shows that the fp32 emulation meets
the same bounds on the same inputs and that the table catches nine deliberately wrong emulations."""
import math

import pytest
import torch

import bwd_abi
import bwd_cases as bc
import bwd_run as br
import ref64_bwd as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the HIP library is the only compute path")
    from motioneditor_amd import capi, ops as _ops
    capi.lib()  # fails loudly when libmotioned.so is missing
    return _ops


def cu(t):
    return t.cuda()


@pytest.mark.parametrize("case", bc.CASES, ids=lambda c: c.id)
def test_hip_kernel_matches_the_fp64_reference(ops, case):
    p = case.p
    t = bc.build(case)
    want = br.run(case, ref, t, br.to_ref)
    seen = {}
    if p.get("peaked"):
        ops.attention_fallback_blocks(reset=True)
    got = br.run(case, ops, t, cu, hook=lambda stage: seen.__setitem__(stage, ops._last_kernel()))
    if p.get("fwd"):        # the forward form whose log-sum-exp this backward read
        assert br.kernel_matches(seen["fwd"], p["fwd"]), f"{case.id}: written for the forward {p['fwd']}, the launch took {seen['fwd']}"
    if case.path:
        assert br.kernel_matches(seen["bwd"], case.path), f"{case.id}: written for {case.path}, the launch took {seen['bwd']}"
    if p.get("peaked"):
        assert ops.attention_fallback_blocks() > 0, "the peaked logits were meant to send the forward's blocks to the running-maximum sweep"
    figures = br.compare(case, got, want, who="HIP")
    print(case.id, seen.get("bwd", ""), {k: (f"{r:.2e}", f"{m:.2e}") for k, (r, m) in figures.items()})
    if case.twice:          # fixed-order reductions: the same call twice is bitwise the same
        again = br.run(case, ops, t, cu)
        for name in got:
            assert br.bitwise_equal(got[name], again[name]), f"{case.id}: {name} differs between two identical calls"


def test_geometry_restatement_matches_the_library_host_functions(ops):
    """The Python restatement of dw_geometry / gn_bwd_chunks that placed the edges of the table, against the library this machine runs (host functions: no launch)."""
    from motioneditor_amd import capi
    L = capi.lib()
    for c in bc.CASES:
        if c.entry == "gemm_dw":
            assert L.me_gemm_dw_work_bytes(c.p["M"], c.p["N"], c.p["K"]) == bc.dw_work_bytes(c.p["M"], c.p["N"], c.p["K"]), c.id
        if c.entry == "groupnorm_bwd":
            rows = c.p["rpg"] * c.p["nsg"]
            assert L.me_groupnorm_bwd_scratch_bytes(rows, c.p["rpg"], 32) == bc.gn_bwd_scratch_bytes(rows, c.p["rpg"], 32), c.id
    for N, K, lim in bc.DW_EDGE_SHAPES:
        for M in range(1, lim, 61):
            assert L.me_gemm_dw_work_bytes(M, N, K) == bc.dw_work_bytes(M, N, K), (M, N, K)


def test_temporal_attention_bwd_refuses_64_frames_of_head_dim_160(ops):
    """frames = 64 is legal for dh = 40 and 80 (cases tattn-F64-dh40 / -dh80); with dh = 160 the first version's LDS tile does not fit: ME_EINVAL with the
    LDS message, and nothing is written."""
    r = bc.TATTN_REFUSED
    C, rows = r["heads"] * r["dh"], r["batch"] * r["frames"] * r["npix"]
    q = torch.randn(rows, 3 * C, device="cuda").half()
    dout = torch.randn(rows, C, device="cuda")
    outs = [torch.full((rows, C), 5.0, device="cuda") for _ in range(3)]
    from motioneditor_amd import capi
    rc = capi.lib().me_tattn_bwd(outs[0].data_ptr(), C, outs[1].data_ptr(), C, outs[2].data_ptr(), C, q[:, :C].data_ptr(), 3 * C, q[:, C:].data_ptr(), 3 * C,
                                 q[:, 2 * C:].data_ptr(), 3 * C, dout.data_ptr(), C, r["batch"], r["frames"], r["npix"], r["heads"], r["dh"], r["dh"] ** -0.5, ops._stream())
    msg = capi.lib().me_last_error().decode()
    assert rc == capi.ME_EINVAL and msg.startswith("me_tattn_bwd:") and "LDS" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert all(bool((o == 5.0).all()) for o in outs)
    with pytest.raises(ValueError, match="LDS"):
        ops.temporal_attention_bwd(q[:, :C], q[:, C:2 * C], q[:, 2 * C:], None, dout, **r)


@pytest.mark.parametrize("entry", ["me_gemm_dw", "me_attn_bwd", "me_tattn_bwd", "me_groupnorm_bwd", "me_layernorm_bwd", "me_geglu_bwd", "me_softmax_bwd_rows", "me_colsum",
                                   "me_sumsq_absmax", "me_adamw"])
def test_backward_abi_violations_leave_sentinel_filled_outputs_untouched(ops, entry):
    """tests/bwd_abi.py on device buffers: every violating call returns ME_EINVAL with a message naming the entry point, and every buffer of the call -- outputs
    and scratch included -- holds its sentinel bytes afterwards.  (tests/test_abi_cpu.py has already shown, without a device, that each of these calls is refused
    on the host.)"""
    from motioneditor_amd import capi
    L = capi.lib()
    spec = bwd_abi.entries(L)[entry]
    bufs = {}

    def ptr(name, nbytes):
        if name not in bufs:
            bufs[name] = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        return bufs[name].data_ptr()
    for label, overrides, needle in spec[2]:
        rc = bwd_abi.call(L, capi, entry, spec, overrides, ptr)
        msg = L.me_last_error().decode()
        assert rc == capi.ME_EINVAL and msg.startswith(entry + ":") and needle in msg, f"{entry} ({label}): status {rc}, message {msg!r}"
    torch.cuda.synchronize()
    assert bufs and all(bool((b == 0xA5).all()) for b in bufs.values()), f"{entry}: a refused call wrote to one of its buffers"


# ------------------------------------------------------------------------------------------------------------------ the non-finite contract
@pytest.mark.parametrize("special", ["inf", "nan"])
def test_adamw_with_a_non_finite_gradient_norm_is_a_no_op(ops, special):
    """me_adamw given an inf / NaN gnorm_sq leaves p, m and v bitwise unchanged -- also when the moments are non-zero and the gradient itself is finite."""
    g = torch.Generator().manual_seed(3)
    n = 70_001
    p0, m0, v0, gr = (torch.randn(n, generator=g) for _ in range(4))
    v0 = v0.abs()
    p, m, v = cu(p0), cu(m0), cu(v0)
    gn = cu(torch.tensor([float(special), 1.0]))
    ops.adamw(p, m, v, cu(gr), lr=1e-3, weight_decay=1e-2, step=7, gnorm_sq=gn, max_grad_norm=1.0, grad_scale=1.0)
    assert br.bitwise_equal(p, p0) and br.bitwise_equal(m, m0) and br.bitwise_equal(v, v0)
    ops.adamw(p, m, v, cu(gr), lr=1e-3, weight_decay=1e-2, step=7, gnorm_sq=ops.sumsq_absmax(cu(gr)), max_grad_norm=1.0, grad_scale=1.0)   # a finite norm: the step is taken
    assert not torch.equal(p.cpu(), p0) and bool(torch.isfinite(p).all())


def test_loss_scale_sees_a_nan_through_the_device_absmax(ops):
    """util._loss_scale trusts isfinite(max |x|): the device reduction must not drop a NaN (fmaxf would)."""
    from motioneditor_amd import util
    x = torch.randn(100_000)
    x[77_777] = float("nan")
    r = ops.sumsq_absmax(cu(x)).cpu()
    assert math.isnan(float(r[0])) and math.isnan(float(r[1]))
    assert util._loss_scale(float(r[1])) == 1.0


def _gpu_trainer_case(ops, monkeypatch, make, step_args):
    tr = make()
    state = br.poison_next_bucket(monkeypatch, ops, tr)
    br.assert_skipped_then_updates(tr, lambda: tr.step(*step_args), state)


def test_adapter_trainer_on_the_gpu_skips_a_step_whose_bucket_holds_an_inf(ops, monkeypatch, unet_sd_np):
    """The inf is written into the gradient bucket from the test (never by overflowing anything on the device): masters, moments and the packed fp16 weights
    stay bitwise what they were, skipped_steps == 1, and the next clean step updates normally."""
    from motioneditor_amd import util
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    c = br.training_clip(0)
    _gpu_trainer_case(ops, monkeypatch, lambda: util.AdapterTrainer(UNet2DConditionModel(unet_sd_np, device="cuda"), lr=1e-3),
                      (c["noisy"], c["t"], c["ehs"], c["down"], c["mid"], c["noise"]))


def test_background_tuner_on_the_gpu_skips_a_step_whose_bucket_holds_an_inf(ops, monkeypatch, unet_sd_np):
    from motioneditor_amd import util
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    c = br.training_clip(1)
    _gpu_trainer_case(ops, monkeypatch, lambda: util.UNetTuner(UNet2DConditionModel(unet_sd_np, device="cuda"), lr=1e-3), (c["noisy"], c["t"], c["ehs"], c["noise"]))
