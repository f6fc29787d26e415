"""The stream-order checker (tests/streamcheck.py) without a GPU: the analyser on hand-written logs -- a correctly ordered miniature of the step's skeleton
passes, every planted defect fails with a message that names it --, the completeness of its read / write table against ops.py, and the table's correctness
against the emulation: the launch graphs of tests/test_graph_cpu.py and the two-branch step of tests/test_step_cpu.py run under the trace with tests/emu_ops.py
patched in, and after every op each view classed read-only is bitwise unchanged and each view that changed is classed written."""
import numpy as np
import pytest
import torch

import emu_ops
import streamcheck as sc
from motioneditor_amd import plan, schedulers, synth
from motioneditor_amd.models import graph


def V(name, addr, rows, cols, ld=None, es=2, alloc=None):
    """[rows, cols] of `es`-byte elements at byte address `addr`, row pitch `ld` elements."""
    ld = cols if ld is None else ld
    return sc.View(addr, 0, (rows, cols), (ld * es, es), es, name, alloc)


# ------------------------------------------------------------------ overlap: exact at element granularity
def _bytes_of(v):
    idx = np.zeros(1, dtype=np.int64)
    for n, st in zip(v.shape, v.strides):
        idx = (idx[:, None] + np.arange(n)[None, :] * st).reshape(-1)
    return set((v.ptr + idx[:, None] + np.arange(v.esize)[None, :]).reshape(-1).tolist())


def test_overlap_equals_brute_force_on_random_strided_views():
    g = np.random.default_rng(3)
    hits = 0
    for _ in range(300):
        vs = []
        for _ in range(2):
            es = int(g.choice([2, 4]))
            rows, cols, heads = int(g.integers(1, 6)), int(g.integers(1, 6)), int(g.integers(1, 3))
            ld = cols + int(g.integers(0, 5))
            hs = rows * ld + int(g.integers(0, 7))
            vs.append(sc.View(1000, int(g.integers(0, 40)) * es, (heads, rows, cols), (hs * es, ld * es, es), es))
        a, b = vs
        common = _bytes_of(a) & _bytes_of(b)
        got = sc.overlap(a, b)
        assert (got is None) == (not common), (a.describe(), b.describe(), got)
        if got is not None:
            hits += 1
            assert got[0] < got[1] and set(range(got[0], got[1])) <= common
    assert 30 < hits < 270          # both outcomes were exercised


def test_column_slice_neighbours_do_not_overlap():
    """The two column halves of a concat buffer (graph.unet_forward, skip_slot): bounding boxes intersect, no element is shared."""
    left, right = V("cat.left", 0x4000, 64, 32, ld=64), V("cat.right", 0x4000 + 64, 64, 32, ld=64)
    assert left.lo < right.hi and right.lo < left.hi
    assert sc.overlap(left, right) is None
    assert sc.overlap(left, V("cat", 0x4000, 64, 64)) is not None
    log = sc.Log()
    log.launch(0, "copy_rows", [], [left])
    log.launch(1, "axpy_rows", [right], [right])          # no event between the streams at all
    assert sc.analyse(log) == []
    log.launch(1, "gemm", [V("cat", 0x4000, 64, 64)], [])
    (r,) = sc.analyse(log)
    assert r.kind == "RAW" and "read-after-write hazard" in str(r) and r.first.name == "copy_rows" and r.second.name == "gemm"


# ------------------------------------------------------------------ the miniature of the step's skeleton
def mini(drop_ready_wait=False, drop_skip_wait=False, extra_write=False, early_wait=False, reuse=False, trailing=False):
    """pipelines.denoise_step + graph.unet_forward in ten launches: ControlNet and the adapter on stream 1, the UNet on stream 0."""
    L = sc.Log()
    lat_in, text, params, lat_out = V("lat_in", 0x1000, 1, 256, es=4), V("text", 0x2000, 77, 8), V("params", 0x3000, 1, 4, es=4), V("lat_out", 0x3800, 1, 256, es=4)
    L.entry("hipMemcpyAsync(latents in)", writes=[lat_in])
    L.entry("hipMemcpyAsync(text in)", writes=[text])
    L.entry("plan_params_kernel", writes=[params])
    x4 = V("x4", 0x10000, 2, 256, es=4)
    L.launch(0, "repeat_batch", [lat_in], [x4])
    L.wait(1, L.record(0))                                        # plan.wait_stream(side, main)
    down, mid = V("cn.down", 0x20000, 64, 32), V("cn.mid", 0x30000, 16, 32)
    if extra_write:
        L.launch(0, "fill", [], [down])
    L.launch(1, "controlnet_forward", [x4, text, params], [down, mid])
    ready = L.record(1)
    cat, left, skip = V("cat", 0x40000, 64, 64), V("cat.left", 0x40000, 64, 32, ld=64), V("cat.right = skip", 0x40000 + 64, 64, 32, ld=64)
    L.launch(0, "down_block_0", [x4, text, params], [skip])
    L.wait(1, L.record(0))                                        # push_skip
    motion = V("motion", 0x50000, 64, 32)
    tmp = [V("adapter.tmp", 0x80000, 64, 32, alloc=(0x80000, 4096))] if reuse else []
    L.launch(1, "adapter_block", [skip, down] + tmp, [motion] + tmp)
    h = V("h", 0x60000, 16, 32)
    L.launch(0, "down_block_1", [skip], [h])                      # main's last read of the skip
    e = L.record(0)
    if not drop_skip_wait:
        L.wait(1, e)                                              # "main is past its last read of every skip"
    L.launch(1, "axpy_rows", [skip, motion], [skip])              # the motion update, in place
    ad = L._events
    L._events += 1
    if early_wait:
        L.wait(0, ad)
    L.record(1, ad)                                               # adapter_done
    if trailing:
        L.launch(1, "late_side_work", [params], [V("side.scratch", 0x90000, 1, 64)])
    other = [V("main.other", 0x80000, 32, 128, alloc=(0x80000, 8192))] if reuse else []
    L.launch(0, "mid_block", [h, text], [h] + other)
    if not drop_ready_wait:
        L.wait(0, ready)
    L.launch(0, "axpy_rows", [h, mid], [h], site="graph.py:0 (mid-block add)")
    L.launch(0, "copy_rows", [h], [left])                         # beside the skip the side stream is updating: column neighbours
    if not early_wait:
        L.wait(0, ad)
    eps = V("eps", 0x70000, 64, 4)
    L.launch(0, "up_block", [cat], [eps])
    L.launch(0, "cfg_ddim", [lat_in, eps, params], [lat_out])
    L.exit("hipMemcpyAsync(latents out)", reads=[lat_out])
    return L


def test_correctly_ordered_miniature_passes_within_one_replay_and_across_two():
    assert sc.analyse(mini()) == []
    assert sc.analyse(mini(), replays=2) == []


def test_missing_wait_is_a_read_after_write():
    rs = sc.analyse(mini(drop_ready_wait=True))
    assert [r.kind for r in rs] == ["RAW"], sc.format_reports(rs)
    r = rs[0]
    assert "read-after-write hazard" in str(r) and "'cn.mid'" in str(r)
    assert (r.first.name, r.first.stream, r.second.name, r.second.stream) == ("controlnet_forward", 1, "axpy_rows", 0) and "mid-block add" in r.second.site
    assert (r.lo, r.hi) == (0x30000, 0x30000 + 16 * 32 * 2)


def test_missing_wait_before_an_in_place_update_is_a_write_after_read():
    rs = sc.analyse(mini(drop_skip_wait=True))
    assert [r.kind for r in rs] == ["WAR"], sc.format_reports(rs)
    assert "write-after-read hazard" in str(rs[0]) and (rs[0].first.name, rs[0].second.name) == ("down_block_1", "axpy_rows") and "skip" in str(rs[0])


def test_two_unordered_writers_are_a_write_after_write():
    rs = sc.analyse(mini(extra_write=True))
    assert [r.kind for r in rs] == ["WAW"], sc.format_reports(rs)
    assert "write-after-write hazard" in str(rs[0]) and (rs[0].first.name, rs[0].second.name) == ("fill", "controlnet_forward")


def test_wait_issued_before_its_record_is_reported():
    rs = sc.analyse(mini(early_wait=True))
    assert rs[0].kind == "WAIT_BEFORE_RECORD" and "WAIT before its RECORD" in str(rs[0]) and "event 4" in str(rs[0]), sc.format_reports(rs)
    assert any(r.kind == "RAW" and r.second.name == "up_block" for r in rs), sc.format_reports(rs)      # ... and it orders nothing


def test_edge_through_a_third_event_orders():
    def chain(relay):
        L = sc.Log()
        x = V("x", 0x1000, 8, 8)
        L.launch(1, "producer", [], [x])
        ea = L.record(1)
        if relay:
            L.wait(0, ea)
        L.wait(2, L.record(0))               # stream 2 waits for stream 0 only
        L.launch(2, "consumer", [x], [])
        return L
    assert sc.analyse(chain(True)) == []
    rs = sc.analyse(chain(False))
    assert [r.kind for r in rs] == ["RAW"] and "read-after-write" in str(rs[0])


def test_address_reused_on_the_other_stream_without_an_edge_is_reported():
    rs = sc.analyse(mini(reuse=True))
    assert rs and all(r.first.name == "adapter_block" and r.second.name == "mid_block" for r in rs), sc.format_reports(rs)
    assert {r.kind for r in rs} == {"WAW", "WAR"}
    assert all("two different allocations at one address: a block handed out again" in str(r) and "'adapter.tmp'" in str(r) and "'main.other'" in str(r) for r in rs)


def test_hazard_between_two_consecutive_replays_only():
    assert sc.analyse(mini(trailing=True)) == []
    rs = sc.analyse(mini(trailing=True), replays=2)
    assert [r.kind for r in rs] == ["WAR"], sc.format_reports(rs)
    r = rs[0]
    assert r.replays == (0, 1) and "across replays 0 and 1" in str(r) and "write-after-read hazard" in str(r)
    assert (r.first.name, r.first.stream, r.second.name, r.second.stream) == ("late_side_work", 1, "plan_params_kernel", 0)


def test_deleting_a_node_keeps_every_other_index():
    L = mini()
    waits = [i for i, (k, s, e) in enumerate(L.nodes) if k == sc.WAIT and s == 0]
    assert len(waits) == 2
    rs = sc.analyse(L.without(waits[1]))                # adapter_done
    assert rs and all(r.second.name == "up_block" for r in rs) and len(L.without(waits[1]).nodes) == len(L.nodes) and sc.analyse(L) == []


# ------------------------------------------------------------------ trace against plan, on stand-ins
def _stand_ins():
    """A two-function `ops`, the four helpers of `plan` and a plan that counts nodes, on CPU tensors: what Trace and build_log see of the real ones."""
    import types
    state = types.SimpleNamespace(nodes=[], events=0, cur=0)

    class Plan:
        def stats(self):
            return {k: sum(n[0] == i for n in state.nodes) for i, k in enumerate(("launches", "event_records", "event_waits"))}

        def nodes(self):
            return [(k, s, e, (1, 1, 1), (64, 1, 1)) for k, s, e in state.nodes]

    class Stream:
        def __init__(self, i):
            self.i, self.cuda_stream = i, 0x1000 * i

    class Event:
        pass

    pm, om = types.ModuleType("stand_in_plan"), types.ModuleType("stand_in_ops")

    def record_event(stream):
        ev = Event()
        ev.i, state.events = state.events, state.events + 1
        state.nodes.append((sc.RECORD, stream.i, ev.i))
        return ev

    def wait_event(stream, ev):
        state.nodes.append((sc.WAIT, stream.i, ev.i))

    def wait_stream(waiter, signaller):
        pm.wait_event(waiter, pm.record_event(signaller))

    def share(t, stream):
        pass

    def _stream():
        return 0x1000 * state.cur

    def copy_rows(y, x):
        state.nodes.append((sc.LAUNCH, state.cur, -1))
        y.copy_(x)
        return y

    def axpy_rows(y, x, a_, alpha=1.0):
        state.nodes += [(sc.LAUNCH, state.cur, -1)] * 2          # one op, two launches
        y.copy_(x + alpha * a_)
        return y

    def clone_rows(x):
        return om.copy_rows(torch.empty_like(x), x)             # nested: logged once, as clone_rows

    for mod, fns in ((pm, (record_event, wait_event, wait_stream, share)), (om, (_stream, copy_rows, axpy_rows, clone_rows))):
        for f in fns:
            f.__module__ = mod.__name__
            setattr(mod, f.__name__, f)
    return om, pm, Plan(), state, Stream(0), Stream(1)


def test_trace_matches_the_plan_and_feeds_the_analyser_on_stand_ins():
    om, pm, pl, state, main, side = _stand_ins()
    a, b, c = torch.zeros(4, 8), torch.ones(4, 8), torch.zeros(4, 8)
    with sc.Trace(om, pm, pl) as tr:
        om.copy_rows(a, b)
        pm.wait_stream(side, main)
        state.cur = 1
        m = om.clone_rows(a)
        ready = pm.record_event(side)
        state.cur = 0
        pm.wait_event(main, ready)
        om.axpy_rows(c, c, m)
    assert [(o.name, o.first, o.last) for o in tr.ops] == [("copy_rows", 0, 1), ("clone_rows", 3, 4), ("axpy_rows", 6, 8)] and tr.calls["nested"] == 1
    assert [(y.kind, y.event, y.node) for y in tr.syncs] == [("record", 0, 1), ("wait", 0, 2), ("record", 1, 4), ("wait", 1, 5)] and tr.calls["wait_stream"] == 1
    assert all("test_streamcheck_cpu.py" in y.site for y in tr.syncs) and "(test_trace_matches" in tr.syncs[3].site and "pm.wait_event(main, ready)" == tr.syncs[3].code
    log = sc.build_log(tr, pl, b, None, None, c)
    assert [o.stream for o in log.ops] == [0, 1, 0]
    assert sc.analyse(log) == [] and sc.analyse(log, replays=2) == []
    (r,) = sc.analyse(log.without(tr.syncs[3].node))
    assert r.kind == "RAW" and (r.first.name, r.first.stream, r.second.name, r.second.stream) == ("clone_rows", 1, "axpy_rows", 0) and "nodes 6..7" in str(r)
    rs = sc.analyse(log.without(tr.syncs[1].node))
    assert [(x.kind, x.first.name, x.second.name) for x in rs] == [("RAW", "copy_rows", "clone_rows")]
    # a launch that no traced op accounts for, and a record the trace did not see
    state.nodes.insert(6, (sc.LAUNCH, 0, -1))
    with pytest.raises(AssertionError, match="belong to no traced op"):
        sc.build_log(tr, pl)
    del state.nodes[6]
    state.nodes.append((sc.RECORD, 0, 2))
    with pytest.raises(AssertionError, match="the trace saw 4 event records / waits, the plan holds 5"):
        sc.build_log(tr, pl)


def test_completeness_check_reads_the_argument_bytes_of_a_real_plan():
    """check_completeness against the library's own plan (host code: no GPU): two launches appended by hand, their argument bytes read back through
    me_plan_node.  A pointer into a known allocation that no view of the op covers is reported -- also behind a 4-byte scalar, where it is not 8-byte aligned."""
    import ctypes as C
    from motioneditor_amd import capi
    L = capi.lib()
    append = L.me_plan_append_launch          # what me_launch calls for every kernel of the library while a plan records (me_common.h)
    append.restype, append.argtypes = None, [C.c_void_p] + [C.c_uint] * 7 + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    x, y, z = torch.zeros(64, 32, dtype=torch.float16), torch.zeros(64, 32, dtype=torch.float16), torch.zeros(16)

    def launch(*vals):
        argv = (C.c_void_p * len(vals))(*[C.cast(C.pointer(v), C.c_void_p) for v in vals])
        sizes = (C.c_uint * len(vals))(*[C.sizeof(v) for v in vals])
        append(None, 1, 1, 1, 64, 1, 1, 0, None, argv, sizes, len(vals))

    class Plan:
        _handle = C.c_void_p()

    capi.check(L.me_plan_begin(C.byref(Plan._handle), None), "me_plan_begin")
    try:
        launch(C.c_void_p(y.data_ptr()), C.c_void_p(x.data_ptr()), C.c_int32(64), C.c_int32(32))
        launch(C.c_int32(7), C.c_void_p(y.data_ptr() + 64), C.c_float(0.5), C.c_void_p(z.data_ptr()))      # the pointers sit at offsets 4 and 16
        capi.check(L.me_plan_end(Plan._handle), "me_plan_end")
        tr = sc.Trace(None)
        vx, vy, vz = tr._view("x", x), tr._view("y", y), tr._view("z", z)
        log = sc.Log()
        log.nodes = [(sc.LAUNCH, 0, -1)] * 2
        log.ops = [sc.Op("copy_rows", "here", 0, 0, 1, [vx], [vy]), sc.Op("axpy_rows", "here", 0, 1, 2, [vy], [vy])]
        with pytest.raises(AssertionError, match=rf"TABLE\['axpy_rows'\] is incomplete: launch node 1 .* is given the address 0x{z.data_ptr():x}, which lies inside an allocation"):
            sc.check_completeness(tr, Plan, log)
        log.ops[1].reads.append(vz)
        assert sc.check_completeness(tr, Plan, log) == 4
        log.ops[1].writes[0] = tr._view("y[:1]", y[:1])                                                     # ... and inside the allocation is not inside the view
        log.ops[1].reads[0] = log.ops[1].writes[0]
        with pytest.raises(AssertionError, match=rf"is given the address 0x{y.data_ptr() + 64:x}"):
            sc.check_completeness(tr, Plan, log)
    finally:
        L.me_plan_destroy(Plan._handle)


# ------------------------------------------------------------------ table completeness
def test_every_launching_function_of_ops_has_a_table_entry_or_a_reason():
    from motioneditor_amd import ops
    import inspect
    fns = set(sc.launching_functions(ops))
    assert {"gemm", "attention", "groupnorm", "clone_rows", "repeat_batch", "to_f16_rows", "gemm_dx", "cfg_ddim"} <= fns     # direct and through another function
    undecided = fns - set(sc.TABLE) - set(sc.NOT_TRACED)
    assert not undecided, f"ops functions that reach the library without a TABLE entry and without a reason in NOT_TRACED: {sorted(undecided)}"
    assert not set(sc.TABLE) & set(sc.NOT_TRACED)
    public = {n for n, f in vars(ops).items() if inspect.isfunction(f) and f.__module__ == ops.__name__ and not n.startswith("_")}
    stale = (set(sc.TABLE) | set(sc.NOT_TRACED)) - public
    assert not stale, f"entries for functions ops.py does not have: {sorted(stale)}"
    assert not set(sc.TABLE) - fns, f"TABLE entries for functions that launch nothing: {sorted(set(sc.TABLE) - fns)}"
    for n, (launches, why) in sc.NOT_TRACED.items():
        assert why and (launches or "no launch" in why), n


# ------------------------------------------------------------------ table correctness against the emulation
@pytest.fixture()
def emu(monkeypatch):
    import motioneditor_amd.models.controlnet as cm
    import motioneditor_amd.models.unet_2d_condition as u
    import motioneditor_amd.pipelines.pipeline_motion_editor as pm
    for m in (graph, u, cm, pm, schedulers):
        monkeypatch.setattr(m, "ops", emu_ops)
    return emu_ops


def test_table_holds_on_the_emulated_single_branch_unet(emu, unet_sd_np):
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    c = synth.make_case_inputs("single", B=2, f=8, h=8, w=8)
    unet = UNet2DConditionModel(unet_sd_np, device="cpu", dtype=torch.float32)
    real_gemm = emu_ops.gemm
    with sc.Trace(emu_ops, plan, None, check_values=True) as tr:
        assert emu_ops.gemm is not real_gemm
        out = unet(c["sample"], c["t"], c["ehs"]).sample
        with pytest.raises(AssertionError, match="ops.grad_acc was called inside a traced step but has no TABLE entry"):
            emu_ops.grad_acc(torch.zeros(4, 4), torch.ones(4, 4))
    assert emu_ops.gemm is real_gemm                                      # the module is as it was
    assert torch.equal(out, unet(c["sample"], c["t"], c["ehs"]).sample)   # tracing changes no result
    names = {o.name for o in tr.ops}
    assert {"gemm", "attention", "temporal_attention", "groupnorm", "conv_small", "copy_rows", "timestep_embed"} <= names, names
    assert len(tr.ops) > 300 and tr.calls["checked_views"] > 1000 and tr.calls["nested"] > 0, (len(tr.ops), tr.calls)
    assert all(o.last == o.first + 1 for o in tr.ops) and [o.first for o in tr.ops] == list(range(len(tr.ops)))
    assert all("graph.py" in o.site or "unet_2d_condition.py" in o.site for o in tr.ops), {o.site for o in tr.ops if "graph.py" not in o.site}


def test_table_holds_on_the_emulated_two_branch_step(emu, unet_sd_np, cn_sd_np):
    from motioneditor_amd.attn_control import (FullySelfAttentionControlMask, TemporalSelfAttentionControl,
                                               regiter_fully_attention_editor_diffusers, regiter_temporal_attention_editor_diffusers)
    from motioneditor_amd.models.controlnet import ControlNetModel
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    from motioneditor_amd.pipelines import MotionEditorPipeline
    from test_step_cpu import step_inputs
    x = step_inputs()
    f, step = x["latents"].shape[2], 4
    pipe = MotionEditorPipeline(unet=UNet2DConditionModel(unet_sd_np, device="cpu", dtype=torch.float32), controlnet=ControlNetModel(cn_sd_np, device="cpu", dtype=torch.float32))
    ted = TemporalSelfAttentionControl(start_step=4, start_layer=10)
    regiter_temporal_attention_editor_diffusers(pipe, ted)
    sed = FullySelfAttentionControlMask(start_step=4, start_layer=10, source_masks=x["masks"])
    regiter_fully_attention_editor_diffusers(pipe, sed)
    pipe.scheduler.set_timesteps(50)
    images = torch.cat([x["skeleton"]] * 2).reshape(2 * f, 3, 64, 64)
    emb = torch.cat([x["uncond"].expand(2, 77, 768), x["cond"]])
    outs = []
    for traced in (True, False):
        ted.cur_step = sed.cur_step = step
        if traced:
            with sc.Trace(emu_ops, plan, None, check_values=True) as tr:
                outs.append(pipe.denoise_step(x["latents"], pipe.scheduler.timesteps[step], emb, images, 7.5))
        else:
            outs.append(pipe.denoise_step(x["latents"], pipe.scheduler.timesteps[step], emb, images, 7.5))
    assert torch.equal(outs[0], outs[1])
    names = {o.name for o in tr.ops}
    assert {"gemm", "attention", "temporal_attention", "groupnorm", "conv_small", "copy_rows", "axpy_rows", "cfg_ddim"} <= names, names
    assert len(tr.ops) > 700 and tr.calls["checked_views"] > 2500, (len(tr.ops), tr.calls)
    # the in-place motion update and the mid-block add were seen as in-place: a written view that is also read
    inplace = [o for o in tr.ops if o.name == "axpy_rows" and any(sc.overlap(r, w) is not None for r in o.reads for w in o.writes)]
    assert len(inplace) >= 13 * 2, len(inplace)


def test_a_wrong_table_entry_is_caught_on_the_emulation(monkeypatch):
    """The correctness rule has teeth: an entry that classes the destination of a copy as read-only fails with the rule's own message."""
    monkeypatch.setitem(sc.TABLE, "copy_rows", sc._entry(["x", "y"], ret=False))
    y, x = torch.zeros(4, 8), torch.ones(4, 8)
    with sc.Trace(emu_ops, None, None, check_values=True):
        with pytest.raises(AssertionError, match=r"TABLE\['copy_rows'\] is wrong: operand 'copy_rows.y' .* is not classed written, but 32 of its elements changed"):
            emu_ops.copy_rows(y, x)
