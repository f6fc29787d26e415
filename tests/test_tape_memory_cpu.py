"""The memory-lean, checkpointing autodiff tape on the emulated ABI, 8 frames on 8 x 8 latents: the three forms of the tape
(tests/tape_memory_common.py) give bitwise the same losses, gradients and trained weights in all three consumers of util.py, with the
recomputation check on; what the tape pins shrinks from form to form and, checkpointed, is exactly the boundary tensors; the gradient store
releases during the walk; a perturbed second run is caught by name.  Every result comparison is torch.equal -- no tolerance."""
import types

import pytest
import torch

import bwd_run as br
import emu_tune_ops
import tape_memory_common as tm


def _patch(monkeypatch, backend):
    import motioneditor_amd.models.unet_2d_condition as u
    from motioneditor_amd import util
    from motioneditor_amd.models import graph
    for m in (graph, u, util):
        monkeypatch.setattr(m, "ops", backend)


@pytest.fixture
def emu(monkeypatch):
    _patch(monkeypatch, emu_tune_ops)


_cache = {}


def _adapter(unet_sd_np, name):
    """adapter_training_grads in one form, computed once per session (the caller has patched the backend in)."""
    if name not in _cache:
        _cache[name] = tm.adapter_grads(tm.make_unet(unet_sd_np, "cpu"), name)
    return _cache[name]


@pytest.mark.parametrize("name", ["lean", "ckpt"])
def test_adapter_gradients_are_bitwise_those_of_the_parent_form(emu, unet_sd_np, name):
    l0, g0, _ = _adapter(unet_sd_np, "parent")
    l1, g1, _ = _adapter(unet_sd_np, name)
    assert l1 == l0 and sorted(g1) == sorted(g0) and len(g0) > 300
    bad = [k for k in g0 if not tm.same(g0[k], g1[k])]
    assert not bad, (name, len(bad), bad[:3])
    assert any(float(g.abs().max()) > 0 for g in g0.values())


def test_null_text_gradient_and_embedding_are_bitwise_the_same_in_all_three_forms(emu, unet_sd_np):
    unet = tm.make_unet(unet_sd_np, "cpu")
    g0, e0 = tm.null_text(unet, "parent")
    assert float(g0.abs().max()) > 0
    for name in ("lean", "ckpt"):
        g, e = tm.null_text(unet, name)
        assert tm.same(g, g0) and tm.same(e, e0), name


@pytest.mark.parametrize("which", sorted(tm.TUNER_SETS))
def test_unet_tuner_step_ends_with_bitwise_the_parent_forms_masters(emu, unet_sd_np, which):
    l0, m0 = tm.tuner_masters(unet_sd_np, "cpu", "parent", which)
    for name in ("lean", "ckpt"):
        l, m = tm.tuner_masters(unet_sd_np, "cpu", name, which)
        assert l == l0 and tm.same(m, m0), (which, name)


def test_stash_and_gradient_store_shrink_from_form_to_form(emu, unet_sd_np):
    """stashed_bytes: checkpointed < lean < parent.  The lean walk's high-water mark of live gradient buffers lies below the sum of the buffers the parent
    form allocates (which releases none: its high-water mark IS that sum)."""
    s = {name: _adapter(unet_sd_np, name)[2] for name in tm.FORMS}
    print({k: v for k, v in s.items()})
    assert s["ckpt"]["stashed_bytes"] < s["lean"]["stashed_bytes"] < s["parent"]["stashed_bytes"]
    assert s["parent"]["grad_peak_bytes"] == s["parent"]["grad_total_bytes"]
    assert s["lean"]["grad_peak_bytes"] < s["parent"]["grad_total_bytes"]
    assert s["ckpt"]["grad_peak_bytes"] < s["parent"]["grad_total_bytes"]


class _Capture:
    """A backend wrapper that remembers which tensors the operators produced while `self.where` names a part of the UNet."""

    def __init__(self, backend):
        self._b, self.made, self.on = backend, [], False

    def __getattr__(self, n):
        f = getattr(self._b, n)
        if n not in ("gemm", "attention", "temporal_attention", "groupnorm", "layernorm", "conv_small"):
            return f

        def wrapped(*a, **k):
            out = f(*a, **k)
            if self.on:
                self.made.append(out)
            return out
        return wrapped


def _record_adapter_forward(unet, checkpoint, on_block=None):
    """The forward of util._unet_backward on a tape of its own: -> (tape, output Act, the segment calls [(name, args, kw, result)])."""
    from motioneditor_amd import autodiff
    from motioneditor_amd.models import graph
    c = br.training_clip(0, f=8, h=8)
    B_ = graph.ops
    P = unet.P
    down = [B_.nchw5_to_rows(r) for r in c["down"]]
    mid = B_.nchw5_to_rows(c["mid"])
    ehs = graph.text_rows(c["ehs"], P.dtype).clone()
    calls = []
    real = autodiff.Recorder.segment

    def spy(self, name, fn, args, kw):
        if on_block is not None:
            on_block(name, True)
        res = real(self, name, fn, args, kw)
        if on_block is not None:
            on_block(name, False)
        calls.append((name, args, kw, res))
        return res
    autodiff.Recorder.segment = spy
    try:
        with autodiff.record(graph, trainable=lambda: P.trainable_ids("controlnet_adapter."), checkpoint=checkpoint) as tape:
            act = graph.unet_forward(P, c["noisy"], float(c["t"]), ehs, down_res=down, mid_res=mid, two_branch=False)
    finally:
        autodiff.Recorder.segment = real
    return tape, act, calls


def test_adapter_training_tape_pins_nothing_a_down_or_mid_block_produced(monkeypatch, unet_sd_np):
    """The adapter's parameters feed the up path only.  Of everything an operator produced inside a down block or the mid block, the tape -- lean or
    checkpointed -- pins only the skips the adapter blocks read (the input of their trained attn_pose k|v projection), by identity of the allocations."""
    from motioneditor_amd import autodiff
    cap = _Capture(emu_tune_ops)
    _patch(monkeypatch, cap)

    def on_block(name, entering):
        if name.startswith(("down_blocks.", "mid_block.")):
            cap.on = entering
    for checkpoint in (False, True):
        del cap.made[:]
        tape, _, calls = _record_adapter_forward(tm.make_unet(unet_sd_np, "cpu"), checkpoint, on_block)
        assert len(cap.made) > 100
        made = {id(autodiff._base(t)) for t in cap.made}      # (cap.made keeps them alive: the ids are theirs alone)
        skips = {id(autodiff._base(args[3])) for name, args, _, _ in calls if name.startswith("controlnet_adapter.")}
        pinned = {id(autodiff._base(t)) for e in tape.entries for t in e.saved} | {id(autodiff._base(t)) for t in tape.keep}
        assert len(skips) == 12 and pinned and not ((pinned & made) - skips), (checkpoint, len((pinned & made) - skips))


def _unique_bytes(tensors):
    """Bytes of the distinct allocations under `tensors`, from their shapes."""
    from motioneditor_amd import autodiff
    seen = {}
    for t in tensors:
        b = autodiff._base(t)
        seen[id(b)] = b.numel() * b.element_size()
    return sum(seen.values())


def test_checkpointed_tape_pins_exactly_the_boundary_tensors(emu, unet_sd_np):
    """In adapter training the differentiated segments are the adapter blocks and every block of the up path.  The bytes the checkpointed tape pins at the
    end of the forward are those of their boundary tensors (the tensors among a segment's arguments, and its result) plus the one activation a call
    recorded outside a segment reads the values of (conv_norm_out's input: the last segment's output -- the skip adds, the concat copies and the frozen
    conv_out keep none)."""
    from motioneditor_amd import autodiff
    tape, act, calls = _record_adapter_forward(tm.make_unet(unet_sd_np, "cpu"), True)
    names = [n for n, *_ in calls]
    assert len(names) == 12 + (8 + 6) + 3 + (12 + 9)   # every adapter block, down resnet / attention, mid block and up resnet / attention passes the hook
    boundary = []
    for name, args, kw, res in calls:
        if name.startswith(("up_blocks.", "controlnet_adapter.")):
            boundary += autodiff._tensors((args, kw)) + autodiff._tensors(res)
    want = _unique_bytes(boundary)
    assert want > 0 and tape.stashed_bytes() == want, (tape.stashed_bytes(), want)
    # ... and it is what the segments' interiors would add to that which the lean form keeps on top
    lean, _, _ = _record_adapter_forward(tm.make_unet(unet_sd_np, "cpu"), False)
    assert lean.stashed_bytes() > want


def test_a_perturbed_second_run_is_caught_and_named(monkeypatch, unet_sd_np):
    """The recomputation check (ME_CHECKPOINT_CHECK): one element of one output of one segment's SECOND run is changed by the backend; the walk raises and
    names the segment."""
    target = "up_blocks.2.attentions.1"
    state = types.SimpleNamespace(inside=0, runs=0, hit=False)

    class Flip:
        def __getattr__(self, n):
            f = getattr(emu_tune_ops, n)
            if n != "gemm":
                return f

            def gemm(x, w, **kw):
                out = f(x, w, **kw)
                if state.inside and state.runs == 2 and not state.hit:
                    state.hit = True
                    out.view(-1)[3] += 1.0
                return out
            return gemm
    _patch(monkeypatch, Flip())
    from motioneditor_amd.models import graph
    real = graph.transformer2d.__wrapped__

    def counted(P, p, *a, **kw):
        if p != target:
            return real(P, p, *a, **kw)
        state.runs += 1
        state.inside += 1
        try:
            return real(P, p, *a, **kw)
        finally:
            state.inside -= 1
    monkeypatch.setattr(graph, "transformer2d", graph._segment(counted))
    with pytest.raises(RuntimeError, match=r"segment `up_blocks\.2\.attentions\.1` differs"):
        tm.adapter_grads(tm.make_unet(unet_sd_np, "cpu"), "ckpt")
    assert state.hit and state.runs == 2


def test_model_flag_is_the_default_and_the_argument_overrides_it(emu, unet_sd_np):
    from motioneditor_amd import util
    unet = tm.make_unet(unet_sd_np, "cpu")
    assert unet.gradient_checkpointing is False and util._checkpointing(unet, None) is False
    assert unet.enable_gradient_checkpointing() is unet and unet.gradient_checkpointing is True
    assert util._checkpointing(unet, None) is True and util._checkpointing(unet, False) is False
    unet.disable_gradient_checkpointing()
    assert util._checkpointing(unet, None) is False and util._checkpointing(unet, True) is True
    assert util.AdapterTrainer(tm.make_unet(unet_sd_np, "cpu"), gradient_checkpointing=True).gradient_checkpointing is True
