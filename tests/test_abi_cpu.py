"""No-GPU checks: the C-ABI library builds for gfx950, loads, and exports every symbol include/motioned.h
declares; argument validation that needs no device; oracle vs the reference golden vectors."""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import GOLD, ROOT, max_rel


def test_library_loads_and_exports_every_declared_symbol():
    from motioneditor_amd import build, capi
    build.build_lib(verbose=False)
    header = (ROOT / "include" / "motioned.h").read_text()
    declared = set(re.findall(r"\b(me_[a-z0-9_]+)\s*\(", header))
    declared = {d for d in declared if not d.endswith("_args")}
    assert declared == set(capi.SYMBOLS), declared ^ set(capi.SYMBOLS)
    L = ctypes.CDLL(str(capi.LIB_PATH))
    for name in declared:
        getattr(L, name)
    assert capi.lib().me_abi_version() == capi.ABI_VERSION == 9


def test_argument_validation_returns_einval_without_a_device():
    from motioneditor_amd import capi
    L = capi.lib()
    a = capi.GemmArgs()
    assert L.me_gemm(ctypes.byref(a), None) == capi.ME_EINVAL and b"null" in L.me_last_error()
    a.X = a.W = a.C = 4096
    a.M, a.N, a.K, a.ldx, a.ldc = 8, 8, 12, 16, 8
    assert L.me_gemm(ctypes.byref(a), None) == capi.ME_EINVAL and b"multiples" in L.me_last_error()
    # ABI 6: the head-major second output needs a term-free epilogue, whole heads and aligned panels; the head strides of me_attn multiples of 8
    a.K, a.N, a.M, a.ldc = 16, 48, 8, 48
    a.C2, a.c2_col0, a.c2_dh, a.c2_hs = 4096, 16, 16, 8 * 16
    a.res, a.ldr = 4096, 48
    assert L.me_gemm(ctypes.byref(a), None) == capi.ME_EINVAL and b"head-major" in L.me_last_error()
    a.res, a.c2_dh = None, 12
    assert L.me_gemm(ctypes.byref(a), None) == capi.ME_EINVAL and b"head-major" in L.me_last_error()
    t = capi.AttnArgs()
    t.Q = t.K = t.V = t.O = t.seg_item = t.seg_mode = 4096
    t.n_items, t.nq, t.nk, t.heads, t.nseg, t.dh = 1, 1, 1, 8, 1, 40
    t.ldq = t.ldk = t.ldv = t.ldo = 320
    t.hsk = 12
    assert L.me_attn(ctypes.byref(t), None) == capi.ME_EINVAL and b"head strides" in L.me_last_error()
    t.hsk = 0
    t.n_items, t.nq, t.nk, t.heads, t.nseg, t.dh = 1, 1, 1, 8, 1, 64
    t.ldq = t.ldk = t.ldv = t.ldo = 512
    assert L.me_attn(ctypes.byref(t), None) == capi.ME_EINVAL and b"head dim" in L.me_last_error()
    with pytest.raises(ValueError):
        capi.check(capi.ME_EINVAL, "x")


def test_plan_records_the_launches_of_this_thread_without_a_device():
    """csrc/plan.hip: while a plan records, every kernel an entry point launches is appended with its grid, stream and argument bytes (the launch itself
    fails here -- no device -- which the entry point reports as before); events are numbered in recording order; misuse is refused."""
    import struct
    from motioneditor_amd import capi
    L = capi.lib()
    assert L.me_plan_recording() == 0
    ev = ctypes.c_int32(-1)
    assert L.me_plan_event_record(None, ctypes.byref(ev)) == capi.ME_EINVAL and b"no plan" in L.me_last_error()
    plan = ctypes.c_void_p()
    main, side = 0x1000, 0x2000                 # stream handles are opaque to the recorder
    assert L.me_plan_begin(ctypes.byref(plan), main) == capi.ME_OK and L.me_plan_recording() == 1
    other = ctypes.c_void_p()
    assert L.me_plan_begin(ctypes.byref(other), main) == capi.ME_EINVAL
    n = 4096
    rc = L.me_silu(0x10000, 0x20000, n, main)                                         # unary_kernel<0>(f16* Y, const f16* X, long n)
    assert rc in (capi.ME_OK, capi.ME_EHIP)
    assert L.me_plan_event_record(main, ctypes.byref(ev)) == capi.ME_OK and ev.value == 0
    assert L.me_plan_event_wait(side, 0) == capi.ME_OK
    assert L.me_plan_event_wait(side, 1) == capi.ME_EINVAL
    rc = L.me_axpy_rows(0x30000, 64, 0x40000, 64, 0x50000, 64, 8, 64, 0.5, side)       # axpy_rows_kernel(Y, ldy, X, ldx, A, lda, long rows, cols, alpha)
    assert rc in (capi.ME_OK, capi.ME_EHIP)
    assert L.me_silu(None, None, 0, main) == capi.ME_EINVAL                            # refused before any launch: nothing recorded
    st = capi.PlanStats()
    assert L.me_plan_info(plan, ctypes.byref(st)) == capi.ME_OK
    assert (st.launches, st.event_records, st.event_waits, st.streams) == (2, 1, 1, 2)
    info, buf = capi.PlanNodeInfo(), ctypes.create_string_buffer(256)
    assert L.me_plan_node(plan, 0, ctypes.byref(info), buf, 256) == capi.ME_OK
    assert (info.kind, info.stream, info.n_args, info.arg_bytes) == (capi.PLAN_LAUNCH, 0, 3, 24) and tuple(info.block) == (256, 1, 1) and info.grid[0] >= 1
    assert struct.unpack("<QQq", buf.raw[:24]) == (0x10000, 0x20000, n)
    assert L.me_plan_node(plan, 1, ctypes.byref(info), None, 0) == capi.ME_OK and (info.kind, info.stream, info.event) == (capi.PLAN_RECORD, 0, 0)
    assert L.me_plan_node(plan, 2, ctypes.byref(info), None, 0) == capi.ME_OK and (info.kind, info.stream, info.event) == (capi.PLAN_WAIT, 1, 0)
    assert L.me_plan_node(plan, 3, ctypes.byref(info), buf, 256) == capi.ME_OK and (info.kind, info.stream, info.n_args, info.arg_bytes) == (capi.PLAN_LAUNCH, 1, 9, 52)
    assert struct.unpack("<QiQiQiqif", buf.raw[:52]) == (0x30000, 64, 0x40000, 64, 0x50000, 64, 8, 64, 0.5)   # densely packed, declaration order
    assert L.me_plan_node(plan, 4, ctypes.byref(info), None, 0) == capi.ME_EINVAL
    assert L.me_denoise_step(plan, None, None, None, 1.0, 7.5, 1.0, 0.0, main) == capi.ME_EINVAL    # still recording
    rc = L.me_plan_end(plan)                      # creates the replay events: needs a device
    assert rc in (capi.ME_OK, capi.ME_EHIP) and L.me_plan_recording() == 0
    assert L.me_denoise_step(plan, None, None, None, 1.0, 7.5, 1.0, 0.0, main) == capi.ME_EINVAL    # not bound (or, without a device, not completed)
    assert L.me_plan_bind(plan, None, 0, None, 0, None, None) == capi.ME_EINVAL
    L.me_plan_destroy(plan)
    L.me_plan_destroy(None)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from motioneditor_amd import capi
    monkeypatch.setattr(capi, "_lib", None)
    monkeypatch.setattr(capi, "LIB_PATH", tmp_path / "nope.so")
    with pytest.raises(capi.MotionedError):
        capi.lib()


def test_schema_matches_reference_key_dump():
    from motioneditor_amd import synth
    ref = {}
    for line in (GOLD / "unet_keys.txt").read_text().splitlines():
        k, *shape = line.split()
        ref[k] = tuple(int(s) for s in shape)
    assert ref == dict(synth.unet_schema())
    assert sum(int(np.prod(s)) for s in synth.controlnet_schema().values()) == 361279120


def test_oracle_ddim_matches_reference_prev_step_vectors():
    from oracle import ref_cpu
    g = np.load(GOLD / "ddim.npz")
    d = ref_cpu.DDIM()
    assert d.timesteps == g["timesteps"].tolist()
    x, e = torch.from_numpy(g["x"]), torch.from_numpy(g["eps"])
    for t in (981, 501, 21, 1):
        assert max_rel(d.step(e, t, x), torch.from_numpy(g[f"prev_{t}"])) < 1e-5
        ca, cb = d.coeffs(t)
        assert max_rel(ca * x + cb * e, torch.from_numpy(g[f"prev_{t}"])) < 1e-4


def test_oracle_unet_matches_reference_golden(unet_sd_torch):
    """The CPU restatement against the output of the reference's own UNet2DConditionModel (single-branch case;
    the two-branch + editor cases are pinned at fixture-generation time and re-checked through the
    launch-graph tests)."""
    from motioneditor_amd import synth
    from oracle import ref_cpu
    g = np.load(GOLD / "unet_single.npz")
    c = synth.make_case_inputs("single", B=2, f=8, h=16, w=16)
    with torch.no_grad():
        out = ref_cpu.unet_forward(unet_sd_torch, c["sample"], c["t"], c["ehs"])
    assert max_rel(out, torch.from_numpy(g["out"])) < 2e-4


def test_plan_helpers_refuse_torch_kernels_inside_a_recorded_step(monkeypatch):
    """motioneditor_amd/plan.py: a torch kernel inside a step that is being recorded would be missing from every replay -- the launch graph's torch-side
    data-movement branches call `torch_fallback`, which must raise while a plan records and be silent otherwise; the autodiff recorder (which has no
    backward rule for the library's copies / casts) keeps the torch branches by presenting NATIVE = False."""
    from motioneditor_amd import autodiff, plan
    from motioneditor_amd.models import graph
    plan.torch_fallback("x")                                   # no plan recording: fine
    monkeypatch.setattr(plan, "ACTIVE", object())
    with pytest.raises(RuntimeError, match="missing from every replay"):
        plan.torch_fallback("text_rows")
    with pytest.raises(RuntimeError, match="missing from every replay"):
        graph.text_rows(torch.zeros(2, 77, 768))               # CPU tensor -> the torch branch -> refused while recording
    monkeypatch.setattr(plan, "ACTIVE", None)
    assert graph.text_rows(torch.zeros(2, 77, 768)).shape == (154, 768)
    assert autodiff.Recorder.NATIVE is False and autodiff.Recorder.recording is True


def test_edited_launch_item_order_is_a_pairwise_interleaving_permutation():
    """segments.edited_spatial hands me_attn a processing order (me_attn_args.item_order, ABI 8): (recon frame g, edit frame g, recon g + 1, ...) per
    (recon, edit) pair, a permutation of the items; other tables have none."""
    from motioneditor_amd import segments
    for B, f in ((4, 24), (2, 6), (4, 3)):
        si, _ = segments.edited_spatial(f, "cpu", True, B)
        order = segments.ITEM_ORDER[si.data_ptr()].tolist()
        assert sorted(order) == list(range(B * f))
        for k in range(0, B * f, 2):
            assert order[k] % (2 * f) < f and order[k + 1] == order[k] + f      # a reconstruction item, then the edit item of the same frame
        assert [o for o in order if o % (2 * f) < f] == sorted(o for o in order if o % (2 * f) < f)   # frames ascend inside a pair
    si, _ = segments.prev_cur(4, 24, "cpu")
    assert si.data_ptr() not in segments.ITEM_ORDER


# ------------------------------------------------------------------ the argument contract of the backward ABI (tests/bwd_abi.py)
import bwd_abi  # noqa: E402


@pytest.mark.parametrize("entry,label", bwd_abi.violation_ids(), ids=lambda v: str(v).replace(" ", "-"))
def test_backward_abi_refuses_a_violating_call_on_the_host(entry, label):
    """One call per documented constraint of me_gemm_dw, me_attn_bwd, me_tattn_bwd, me_groupnorm_bwd, me_layernorm_bwd, me_geglu_bwd, me_softmax_bwd_rows,
    me_colsum, me_sumsq_absmax and me_adamw that violates it: ME_EINVAL with a message that names the entry point and the constraint.  The pointers are fake
    (aligned numbers no kernel could run on): a call that slipped through the host checks would reach the launch and come back ME_EHIP here, never ME_EINVAL.
    With a device present a slipped call would launch on those numbers, so the test stands aside there: tests/test_bwd_sweep_gpu.py sends the same table with
    sentinel-filled device buffers."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present: the same violations run on real buffers in tests/test_bwd_sweep_gpu.py")
    from motioneditor_amd import capi
    L = capi.lib()
    spec = bwd_abi.entries(L)[entry]
    overrides, needle = next((o, n) for lab, o, n in spec[2] if lab == label)
    fake = {}

    def ptr(name, nbytes):
        return fake.setdefault(name, 0x100000 * (len(fake) + 1))
    rc = bwd_abi.call(L, capi, entry, spec, overrides, ptr)
    msg = L.me_last_error().decode()
    assert rc == capi.ME_EINVAL, f"{entry} ({label}): status {rc}, message {msg!r}"
    assert msg.startswith(entry + ":") and needle in msg, f"{entry} ({label}): message {msg!r} should name the entry point and hold {needle!r}"


def test_backward_abi_table_names_every_entry_point_of_the_contract():
    from motioneditor_amd import capi
    want = {"me_gemm_dw", "me_attn_bwd", "me_tattn_bwd", "me_groupnorm_bwd", "me_layernorm_bwd", "me_geglu_bwd", "me_softmax_bwd_rows", "me_colsum", "me_sumsq_absmax", "me_adamw"}
    table = bwd_abi.entries(capi.lib())
    assert set(table) == want and want <= set(capi.SYMBOLS)
    for entry, (kind, args, violations) in table.items():
        labels = [v[0] for v in violations]
        assert len(labels) == len(set(labels)) and len(labels) >= 4, entry
        names = {a[0] for a in args}
        assert all(set(o) <= names for _, o, _ in violations), entry
        nulled = {n for _, o, _ in violations for n, v in o.items() if v == bwd_abi.NULL}
        assert nulled, entry
        if kind == "args":
            assert len(args) + 1 == len(capi.SYMBOLS[entry][1]), entry           # the legal call matches the C signature (+ the stream)
