"""Race check of the recorded two-stream denoising step on a real MI355X (tests/streamcheck.py).

The planned executor (pipelines.denoise_step_planned, csrc/plan.hip) records the ~1100 launches of a step on two HIP streams -- ControlNet and the motion adapter
on the side stream, beside the UNet's down path and mid block -- and re-issues them at fixed addresses.  Every step test compares outputs; a missing cross-stream
edge that the usual timing wins passes all of them.  Here the recording pass runs under streamcheck.Trace and the plan's own node list is analysed, for every
variant of the step the pipeline's switches select, at the sizes of the existing step tests (8 frames x 8 x 8 and 24 frames x 16 x 16 latents):

  1. trace against plan: the plan's RECORD / WAIT nodes are the sequence the trace saw, the ops' node ranges tile its launches;
  2. completeness: every address among a launch's argument bytes that lies in an allocation the trace knows lies in a view attributed to that op;
  3. table correctness on the real kernels: an eager pass, synchronised per op -- what is not classed written is bitwise unchanged;
  4. no hazard within one replay, none across two replays back to back.

Then the check is shown to have teeth ON THE LOG: deleting the adapter_done wait, the initial side-waits-main edge, or the mid-residual edge each produces
reports, the last one at graph.unet_forward's mid-block add against its ControlNet producer.  No racy launch sequence is executed."""
import itertools
import linecache
import time

import pytest
import torch

import streamcheck as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def unet(unet_sd_np):
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    return UNet2DConditionModel(unet_sd_np, device="cuda")


@pytest.fixture(scope="module")
def controlnet(cn_sd_np):
    from motioneditor_amd.models.controlnet import ControlNetModel
    return ControlNetModel(cn_sd_np, device="cuda")


def record_and_check(pipe, unet, lat, emb, images, masks, step):
    """One planned step with its recording pass traced, and checks 1 - 4.  Returns (trace, log)."""
    from motioneditor_amd import ops, plan
    from test_model_gpu import editors
    sed = ted = None
    unet.spatial_editor = unet.temporal_editor = None
    if masks is not None:
        sed, ted = editors(unet, masks)
        sed.cur_step = ted.cur_step = step
    t = pipe.scheduler.timesteps[step]
    traces = []
    real = pipe.denoise_step

    def traced(*a, **k):
        if plan.ACTIVE is None:                      # the warm-up pass
            return real(*a, **k)
        with sc.Trace(ops, plan, plan.ACTIVE) as tr:
            traces.append(tr)
            return real(*a, **k)

    pipe.denoise_step = traced
    try:
        t0 = time.time()
        out = pipe.denoise_step_planned(lat, t, emb, images, 7.5)
        torch.cuda.synchronize()
    finally:
        pipe.denoise_step = real
    (tr,) = traces
    (st,) = pipe._plans.values()
    pl = st["plan"]
    info = pl.stats()
    # 1. trace against plan
    log = sc.build_log(tr, pl, st["lat"], st["emb"], st["params"], st["out"])
    assert sum(o.last - o.first for o in log.ops) == info["launches"] > 300
    assert sum(1 for y in tr.syncs if y.kind == "record") == info["event_records"] and sum(1 for y in tr.syncs if y.kind == "wait") == info["event_waits"]
    # 2. completeness
    t1 = time.time()
    n_addr = sc.check_completeness(tr, pl, log)
    assert n_addr >= 2 * info["launches"], (n_addr, info)           # (every launch has at least an input and an output)
    # 4. no hazard, within one replay and across two
    t2 = time.time()
    one, two = sc.analyse(log), sc.analyse(log, replays=2)
    t3 = time.time()
    assert not one, "within one replay: " + sc.format_reports(one)
    assert not two, "across two replays: " + sc.format_reports(two)
    # 3. table correctness on the real kernels: the same step eagerly, on the device-resident step scalars the recorded launches read, synchronised per op
    if sed is not None:
        sed.cur_step = ted.cur_step = step
    ops.STEP_PARAMS = st["params"]
    try:
        with sc.Trace(ops, plan, None, check_values=True) as tv:
            eager = pipe.denoise_step(lat, t, emb, images, 7.5)
        torch.cuda.synchronize()
    finally:
        ops.STEP_PARAMS = None
    assert [(o.name, o.site) for o in tv.ops] == [(o.name, o.site) for o in tr.ops]
    assert tv.calls["checked_views"] > 2 * len(tv.ops)
    assert torch.equal(eager, out)
    print(f"streamcheck: {info['launches']} launches in {len(log.ops)} ops, {info['event_records']} records, {info['event_waits']} waits, {info['streams']} streams; "
          f"{n_addr} addresses attributed, {tv.calls['checked_views']} operands unchanged; record {t1 - t0:.1f} s, completeness {t2 - t1:.1f} s, "
          f"analysis {t3 - t2:.1f} s, value pass {time.time() - t3:.1f} s")
    unet.spatial_editor = unet.temporal_editor = None
    return tr, log


def step_case(f, hw):
    from test_step_cpu import step_inputs
    x = step_inputs(f=f, h=hw, w=hw)
    images = torch.cat([x["skeleton"]] * 2).reshape(2 * f, 3, 8 * hw, 8 * hw).cuda()
    emb = torch.cat([x["uncond"].expand(2, 77, 768), x["cond"]]).cuda()
    return x, images, emb


# (frames, latent size, step: 0 = editors inactive / 4 = active, dedup_cfg_prefix, dedup_controlnet, overlap_adapter): every combination at 8 frames, every
# switch flipped alone at 24 frames.  overlap_adapter off = ControlNet alone on the side stream.
CASES = [(8, 8, s, p, d, a) for s, p, d, a in itertools.product((0, 4), (True, False), (True, False), (True, False))] + \
        [(24, 16, s, p, d, a) for s in (0, 4) for p, d, a in ((True, True, True), (False, True, True), (True, False, True), (True, True, False))]


@pytest.mark.parametrize("f,hw,step,prefix,dedup_cn,overlap_adapter", CASES,
                         ids=[f"f{f}x{hw}-{'active' if s else 'inactive'}-prefix{int(p)}-cn{int(d)}-adapter{int(a)}" for f, hw, s, p, d, a in CASES])
def test_recorded_two_stream_step_has_no_unordered_access(unet, controlnet, f, hw, step, prefix, dedup_cn, overlap_adapter):
    from motioneditor_amd.pipelines import MotionEditorPipeline
    x, images, emb = step_case(f, hw)
    pipe = MotionEditorPipeline(unet=unet, controlnet=controlnet)
    pipe.scheduler.set_timesteps(50)
    pipe.dedup_cfg_prefix, pipe.dedup_controlnet, pipe.overlap_adapter = prefix, dedup_cn, overlap_adapter
    try:
        tr, log = record_and_check(pipe, unet, x["latents"].cuda(), emb, images, x["masks"], step)
        streams = {s for _, s, _ in log.nodes}
        assert streams == {0, 1}
        side_ops = [o for o in log.ops if o.stream == 1]
        assert any("(controlnet_forward)" in o.site for o in side_ops)
        assert any("(adapter_block)" in o.site for o in side_ops) == overlap_adapter
        waits_on_main = [y for y in tr.syncs if y.kind == "wait" and log.nodes[y.node][1] == 0]
        assert any("res_ready" in y.code for y in waits_on_main)                       # main waits for the ControlNet residuals in either form
        assert any("adapter_done" in y.code for y in waits_on_main) == overlap_adapter
    finally:
        unet.spatial_editor = unet.temporal_editor = None
        pipe.release_plans()


@pytest.mark.parametrize("f,hw", [(8, 8), (24, 16)])
def test_recorded_single_branch_step_is_trivially_clean(unet, f, hw):
    """No ControlNet, no editors: one stream, no events."""
    from motioneditor_amd.pipelines import MotionEditorPipeline
    x, _, _ = step_case(f, hw)
    pipe = MotionEditorPipeline(unet=unet)
    pipe.scheduler.set_timesteps(50)
    emb = torch.cat([x["uncond"][:1], x["cond"][:1]]).cuda()
    try:
        tr, log = record_and_check(pipe, unet, x["latents"][:1].cuda(), emb, None, None, 7)
        assert {s for _, s, _ in log.nodes} == {0} and all(k == sc.LAUNCH for k, _, _ in log.nodes) and not [y for y in tr.syncs if y.kind != "share"]
    finally:
        pipe.release_plans()


def test_log_mutations_produce_reports(unet, controlnet):
    """The check has teeth on the real log: each edge deleted ALONE (from the log, never from the execution) produces reports."""
    from motioneditor_amd.models import graph
    from motioneditor_amd.pipelines import MotionEditorPipeline
    x, images, emb = step_case(8, 8)
    pipe = MotionEditorPipeline(unet=unet, controlnet=controlnet)
    pipe.scheduler.set_timesteps(50)
    try:
        tr, log = record_and_check(pipe, unet, x["latents"].cuda(), emb, images, x["masks"], 4)
    finally:
        unet.spatial_editor = unet.temporal_editor = None
        pipe.release_plans()
    waits = [y for y in tr.syncs if y.kind == "wait"]

    def the(what, pred):
        hit = [y for y in waits if pred(y)]
        assert len(hit) == 1, (what, [(y.site, y.code) for y in waits])
        assert log.nodes[hit[0].node][0] == sc.WAIT
        return hit[0]

    # the up path's wait for the adapter: without it main reads the skips while the side stream may still be updating them
    y = the("adapter_done", lambda y: "adapter_done" in y.code and "(unet_forward)" in y.site)
    assert log.nodes[y.node][1] == 0
    rs = sc.analyse(log.without(y.node))
    print("adapter_done wait deleted: " + sc.format_reports(rs[:4]))
    assert rs and all(r.first.stream != r.second.stream for r in rs)
    assert any(r.kind == "RAW" and r.first.stream == 1 and r.first.name == "axpy_rows" and "(unet_forward)" in r.first.site and r.second.stream == 0 for r in rs)
    # the side stream's first wait for main: without it ControlNet reads the duplicated latents while main may still be writing them
    y = the("side waits main", lambda y: "(denoise_step)" in y.site and "wait_stream" in y.code)
    assert log.nodes[y.node][1] == 1
    rs = sc.analyse(log.without(y.node))
    print("initial side-waits-main edge deleted: " + sc.format_reports(rs[:4]))
    assert rs and any(r.kind == "RAW" and r.first.name == "repeat_batch" and r.first.stream == 0 and r.second.stream == 1 and "(controlnet_forward)" in r.second.site for r in rs)
    rs2 = sc.analyse(log.without(y.node), replays=2)
    assert len(rs2) >= len(rs)
    # the edge in front of the mid-block add: the hazard this check was written for
    y = the("res_ready", lambda y: "res_ready" in y.code and "(unet_forward)" in y.site)
    assert log.nodes[y.node][1] == 0
    rs = sc.analyse(log.without(y.node))
    print("mid-residual edge deleted: " + sc.format_reports(rs))
    assert rs
    # Nothing else hangs on this edge: every report has the mid-block add on main as its reader.  Its partner is the side stream's producer of the mid
    # residual -- or an EARLIER writer of the same pool block on that stream (the block was freed and handed out again for the residual): a read that
    # nothing orders behind the producer is not ordered behind those either, and the analysis, keyed on addresses, says so.
    for r in rs:
        assert r.kind == "RAW" and r.second.name == "axpy_rows" and r.second.stream == 0 and "graph.py" in r.second.site and "(unet_forward)" in r.second.site, str(r)
        line = int(r.second.site.split(":")[1].split()[0])
        assert any("mid_res" in linecache.getline(graph.__file__, line - d) for d in range(3)), str(r)        # ... the add of mid_res (its rows are sliced one line up)
        assert r.first.stream == 1 and "graph.py" in r.first.site, str(r)
    producer = [r for r in rs if "(controlnet_forward)" in r.first.site and "controlnet_mid_block" in r.first.code and r.first.name == "gemm"]
    assert producer, sc.format_reports(rs)
