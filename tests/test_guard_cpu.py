"""The guard harness (tests/guard.py) without a GPU: every symbol of the C ABI is either named by a guard case of tests/test_guard_gpu.py or listed, with a
reason, as not launching on caller-provided tensors; and the harness itself catches what it is for -- a correct pure-torch stand-in passes run_guarded, six
deliberately wrong ones fail with the harness's own messages.  The stand-ins are CPU functions on CPU tensors that reach past their views through the
allocation behind them, the way a kernel does through a pointer; nothing wrong is ever launched on a GPU."""
import pytest
import torch

import guard
from guard import embed_in, rnd, run_guarded, scratch_independent, sentinel_out

# Symbols no guard case names, and why.  None of them launches a kernel on caller-provided tensors.
NOT_GUARDED = {
    "me_abi_version": "version query, no launch",
    "me_last_error": "error-string query, no launch",
    "me_last_kernel": "kernel-name query (the witness of every guard case), no launch",
    "me_device_info": "device query, no launch",
    "me_gemm_work_bytes": "size query, no launch",
    "me_groupnorm_scratch_bytes": "size query, no launch",
    "me_groupnorm_bwd_scratch_bytes": "size query, no launch",
    "me_attn_vsum_bytes": "size query, no launch",
    "me_gemm_dw_work_bytes": "size query, no launch",
    "me_colsum_work_bytes": "size query, no launch",
    "me_layernorm_bwd_params_work_bytes": "size query, no launch",
    "me_sumsq_work_bytes": "size query, no launch",
    "me_attn_fallback_blocks": "reads (and resets) the library's own diagnostic counter",
    "me_plan_begin": "plan API: records launches that are guarded one by one",
    "me_plan_event_record": "plan API: records launches that are guarded one by one",
    "me_plan_event_wait": "plan API: records launches that are guarded one by one",
    "me_plan_end": "plan API: records launches that are guarded one by one",
    "me_plan_recording": "plan API: state query",
    "me_plan_bind": "plan API: binds the buffers of a recorded step",
    "me_denoise_step": "plan API: replays recorded launches that are guarded one by one",
    "me_plan_info": "plan API: statistics query",
    "me_plan_node": "plan API: node query",
    "me_plan_destroy": "plan API: frees a plan",
}
_NO_LAUNCH = ("_bytes", "me_plan_", "me_abi_version", "me_last_", "me_device_info", "me_attn_fallback_blocks", "me_denoise_step")


def test_every_abi_symbol_is_guarded_or_listed_with_a_reason():
    from motioneditor_amd import capi
    import test_guard_gpu
    guarded = set()
    for syms in test_guard_gpu.GUARDED.values():
        guarded |= set(syms)
    assert len(test_guard_gpu.GUARDED) > 0
    symbols = set(capi.SYMBOLS)
    assert guarded <= symbols, f"guard cases name symbols the ABI does not have: {sorted(guarded - symbols)}"
    assert set(NOT_GUARDED) <= symbols, f"NOT_GUARDED lists symbols the ABI does not have: {sorted(set(NOT_GUARDED) - symbols)}"
    undecided = symbols - guarded - set(NOT_GUARDED)
    assert not undecided, f"ABI symbols without a guard case and without an entry in NOT_GUARDED: {sorted(undecided)}"
    both = guarded & set(NOT_GUARDED)
    assert not both, f"listed as not guarded although a guard case names them: {sorted(both)}"
    for s, why in NOT_GUARDED.items():
        assert why and any(s.endswith(p) or s.startswith(p) for p in _NO_LAUNCH), f"{s} may launch a kernel on caller-provided tensors: it needs a guard case"


# ------------------------------------------------------------------ the stand-ins: out[m, n] = sum_k x[m, k] w[n, k] on 4 x 4 tiles, M = 6, N = 6
M, N, K, T = 6, 6, 8, 4


def _raw(view):
    """(allocation, offset, pitch): what a kernel has -- a pointer and a leading dimension."""
    g = view.guard
    return g.buf, g.offset, view.stride(0)


def _rows(view, r0, n, cols):
    """n rows x cols columns from row r0 of the view ON, whether or not they exist in the view."""
    buf, off, ld = _raw(view)
    return buf.as_strided((n, cols), (ld, 1), off + r0 * ld)


def k_correct(x, w, out):
    out.copy_((x.float() @ w.float().t()).half())


def k_writes_a_row_past_the_output(x, w, out):
    k_correct(x, w, out)
    _rows(out, M, 1, N).copy_(out[M - 1:M])                     # the row tile stores all of its 4 + 4 rows' first extra row


def k_writes_a_guard_column(x, w, out):
    k_correct(x, w, out)
    _rows(out, 0, M, N + 1)[:, N] = 0                            # a 16-byte store that straddles the view's right edge


def k_masks_the_tail_rows_by_a_zero_weight(x, w, out):
    mp = (M + T - 1) // T * T
    xt = _rows(x, 0, mp, K).float()                               # loads rows M .. mp - 1 as well ...
    keep = (torch.arange(mp) < M).float()[:, None]
    colsum = (xt * keep).sum(0)                                   # ... and "masks" them: 0 x NaN = NaN
    out.copy_((x.float() @ w.float().t() + 0.0 * colsum.sum()).half())


def k_reads_a_weight_row_past_n(x, w, out):
    npad = (N + T - 1) // T * T
    wt = _rows(w, 0, npad, K).float()               # the column tile loads rows N .. npad - 1 of the weights
    acc = x.float() @ wt.t()
    out.copy_((acc[:, :N] - acc.max(dim=1, keepdim=True).values + acc[:, :N].max(dim=1, keepdim=True).values).half())   # a row maximum over the WHOLE tile


def k_leaves_an_input_modified(x, w, out):
    x.mul_(0.5)                                                   # pre-scales its operand in place and forgets to undo it
    out.copy_((2.0 * x.float() @ w.float().t()).half())


_partials = torch.zeros(M, N)


def k_accumulates_into_scratch_it_did_not_clear(x, w, out):
    _partials.add_(x.float() @ w.float().t())                     # split-K partial sums: += into scratch that is assumed to be zero
    out.copy_(_partials.half())


def _case(kernel):
    x = embed_in(rnd(M, K, seed=1), row_guard=T, col_guard=8, name="x")
    w = embed_in(rnd(N, K, seed=2, scale=K ** -0.5), row_guard=T, col_guard=8, name="w")
    out, _ = sentinel_out((M, N), device="cpu", row_guard=T, col_guard=8, name="out")
    return (lambda: kernel(x, w, out)), {"x": x, "w": w}, {"out": out}


def test_a_correct_stand_in_passes_and_matches_the_reference():
    launch, ins, outs = _case(k_correct)
    res = run_guarded(launch, ins, outs)
    guard.check(res["out"], rnd(M, K, seed=1).float() @ rnd(N, K, seed=2, scale=K ** -0.5).float().t(), "stand-in gemm")
    assert ins["x"].stride(0) > K and ins["x"].storage_offset() > 0      # the views really are strided and off the start of their allocations


@pytest.mark.parametrize("kernel,message", [
    (k_writes_a_row_past_the_output, r"guard: \[nan surroundings\] output 'out': 6 elements outside the view were written, the first at \(row 6, column 0\)"),
    (k_writes_a_guard_column, r"guard: \[nan surroundings\] output 'out': 6 elements outside the view were written, the first at \(row 0, column 6\)"),
    (k_masks_the_tail_rows_by_a_zero_weight, r"guard: result 'out' is not finite with nan surroundings: 36 elements, the first at \(0, 0\)"),
    (k_reads_a_weight_row_past_n, r"guard: result 'out' is not finite with nan surroundings"),
    (k_leaves_an_input_modified, r"guard: \[nan surroundings\] input 'x' was modified by the launch: 48 elements, the first at \(row 0, column 0\)"),
])
def test_a_wrong_stand_in_fails_with_the_harness_message(kernel, message):
    launch, ins, outs = _case(kernel)
    with pytest.raises(AssertionError, match=message):
        run_guarded(launch, ins, outs)


def test_a_finite_stray_read_is_caught_by_the_bitwise_comparison():
    """The NaN launch alone does not see a stray read that goes through a maximum with something larger; 0 against 6e4 does."""
    def kernel(x, w, out):
        extra = torch.nan_to_num(_rows(x, M, 1, K).float(), nan=0.0)     # a max() that swallows NaN, as v_max_f32 does
        out.copy_((x.float() @ w.float().t() + extra.max()).half())
    launch, ins, outs = _case(kernel)
    with pytest.raises(AssertionError, match=r"guard: result 'out' with big surroundings differs bitwise from the result with nan surroundings in 36 elements"):
        run_guarded(launch, ins, outs)


def test_stale_scratch_is_caught():
    launch, ins, outs = _case(k_accumulates_into_scratch_it_did_not_clear)
    _partials.zero_()
    with pytest.raises(AssertionError, match=r"guard: result 'out' with zero surroundings differs bitwise from the result with nan surroundings"):
        run_guarded(launch, ins, outs)                                    # three identical launches, three results

    def run():
        launch()
        return outs["out"].clone()
    _partials.zero_()
    with pytest.raises(AssertionError, match=r"guard: 'result' is not finite between a launch on the scratch it left behind and one on NaN-filled scratch"):
        scratch_independent(run, lambda: _partials.fill_(float("nan")))
    ok, ins, outs = _case(k_correct)

    def run_ok():
        ok()
        return outs["out"].clone()
    scratch_independent(run_ok, lambda: _partials.fill_(float("nan")), run_larger=run_ok)


def test_in_out_operands_are_restored_and_only_their_surroundings_are_pinned():
    x = embed_in(rnd(M, K, seed=1), row_guard=T, col_guard=8)
    acc = embed_in(rnd(M, K, seed=3).float(), row_guard=T, col_guard=8)
    want = rnd(M, K, seed=3).float() + rnd(M, K, seed=1).float()
    res = run_guarded(lambda: acc.add_(x.float()), {"x": x, "acc": acc}, {}, inout=["acc"])
    assert torch.equal(res["acc"], want)                                  # += ran three times on the same starting bits

    def past(n):
        acc.add_(x.float())
        _rows(acc, M, 1, n).zero_()
    with pytest.raises(AssertionError, match=r"in-out operand 'acc': 2 elements outside the view were written, the first at \(row 6, column 0\)"):
        run_guarded(lambda: past(2), {"x": x, "acc": acc}, {}, inout=["acc"])


def test_layouts_have_the_least_alignment_and_guards_on_every_side():
    for dtype, es in ((torch.float16, 2), (torch.float32, 4), (torch.int32, 4)):
        for shape, contiguous in (((5, 24), False), ((3, 7, 40), False), ((6, 3, 16), True), ((11,), False)):
            n, off, strides = guard._layout(shape, dtype, 4, 8, contiguous)
            assert (off * es) % 16 == 0 and (off * es) % 32 != 0 and off > 0
            last = off + sum((d - 1) * s for d, s in zip(shape, strides))
            assert n - 1 - last >= 8
            if len(shape) == 2 and not contiguous:
                assert strides[0] > shape[1] and (strides[0] * es) % 32 == 0
            if len(shape) == 3 and not contiguous:
                assert strides[0] >= shape[1] * shape[2] + 4 * shape[2] and strides[1] == shape[2]
    view, intact = sentinel_out((5, 24), torch.float32, device="cpu", row_guard=2, col_guard=4)
    intact()
    assert int(guard.bits(view)[0, 0]) == 0x7FC5A5A5 and bool(torch.isnan(view).all())
    view.guard.buf[0] = 1.0
    with pytest.raises(AssertionError, match=r"the first at \(row -2, column -12\)"):
        intact()
