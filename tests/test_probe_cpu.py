"""ops.attention_probs without a GPU: the fp32 emulation (tests/emu_probe_ops.py) against the fp64 restatement (tests/ref64_probe.py) on every case of
tests/probe_cases.py -- its error is what the kernel's bound is built from, so it is measured and printed here --, the properties the cases are there for,
the ABI table of include/motioned_probe.h (capi.PROBE_SYMBOLS) and every refusal of me_attn_probs, which happens on the host before any launch."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

import emu_probe_ops as emu
import probe_cases as pc
import ref64_probe as ref

ROOT = Path(__file__).resolve().parent.parent


def test_case_list_covers_what_the_kernel_branches_on():
    cs = pc.CASES
    assert {1, 15, 16, 17, 64, 65, 257} <= {c.nq for c in cs}
    assert {1, 16, 17, 64, 65, 77, 80, 128} <= {c.nk for c in cs}
    assert {(c.dh, c.heads) for c in cs} >= {(d, h) for d in (40, 80, 160) for h in (8, 1)}
    assert any(c.q_items and c.q_items == c.n_items // 2 for c in cs) and any(c.q_items == 0 for c in cs)
    assert {(c.q_hm, c.k_hm) for c in cs} == {(False, False), (True, True), (False, True), (True, False)}
    assert {77, 80, 96} <= {c.ldp for c in cs if c.nk == 77 and c.ldp}
    assert any(c.beta == 1.0 for c in cs) and any(c.beta == 0.0 for c in cs)
    for c in cs:   # a permuted table with repeats
        kv = pc.kv_items(c).tolist()
        assert len(set(kv)) < len(kv) and kv != sorted(kv)


@pytest.mark.parametrize("cid", [c.id for c in pc.CASES])
def test_emulation_against_fp64(cid):
    c = pc.BY_ID[cid]
    t = pc.build(c)
    want = pc.reference(c)
    got, P, pad = pc.run(c, emu.attention_probs, t)
    err = float((got.double() - want).abs().max())
    calls = 1 if c.beta == 0 else 3
    sums = float((got.double().sum(1) - calls).abs().max())
    big, std = ref.max_logit(t["q"], t["k"], kv_item=t["kv_item"], **t["kw"])
    print(f"{cid}: emulation max |err| {err:.3e} (kernel bound {pc.bound(c):.3e}), row sums off by {sums:.3e}, logits std {std:.3g} max {big:.4g}")
    assert torch.isfinite(got).all()                      # beta == 0 into NaN-filled P: nothing of it is read
    assert bool((P[:, c.nk:] == pad).all())               # columns >= nk are never touched
    assert err == pc.emu_error(c)                         # measured once, shared with the GPU test
    # fp32 softmax: a logit carries ~ sqrt(dh) half-ulp roundings of its own size, and d p = p (1 - p) d logit <= d logit / 4
    assert err <= calls * (max(big, 1.0) * 2.0 ** -24 * (c.dh ** 0.5 + 2) / 4 + 4 * 2.0 ** -24), err
    assert sums <= pc.bound(c)
    if "gain" in c.tags:
        assert 8.0 < std < 10.0
    if "huge" in c.tags:
        assert big > 1e4


def test_wrong_emulations_fail_a_named_case():
    """Each mistake the cases are there for breaks its case by far more than the case's bound."""
    def err(cid, op):
        c = pc.BY_ID[cid]
        return float((pc.run(c, op, pc.build(c))[0].double() - pc.reference(c)).abs().max()), pc.bound(c)

    def wrong(**change):
        def op(q, k, **kw):
            kw.update({n: f(kw) for n, f in change.items()})
            return emu.attention_probs(q, k, **kw)
        return op
    e, b = err("shared-queries", wrong(q_items=lambda kw: 1))                     # reads query item 0, not i % q_items
    assert e > 100 * b
    e, b = err("nq65", wrong(kv_item=lambda kw: torch.arange(kw["n_items"], dtype=torch.int32) % 2))   # ignores the permutation
    assert e > 100 * b
    e, b = err("beta1-three-times", wrong(beta=lambda kw: 0.0))                   # overwrites instead of accumulating
    assert e > 100 * b

    def no_max(q, k, *, heads, dh, n_items, nq, nk, kv_item, out, alpha=1.0, beta=0.0, q_items=0, scale=None):   # exp without the row maximum
        qh, kh = ref.heads_of(q, heads, dh).float(), ref.heads_of(k, heads, dh).float()
        for it, kit in enumerate(kv_item.tolist()):
            s = torch.einsum("qhd,khd->hqk", qh[it * nq:(it + 1) * nq], kh[kit * nk:(kit + 1) * nk]) * scale
            e_ = torch.exp(s)
            out[it * nq:(it + 1) * nq, :nk] = (e_ / e_.sum(-1, keepdim=True)).mean(0)
        return out
    c = pc.BY_ID["huge-logits"]
    assert not torch.isfinite(pc.run(c, no_max, pc.build(c))[0]).all()


# ------------------------------------------------------------------ the ABI table of include/motioned_probe.h
def test_probe_symbols_are_declared_exported_and_apart_from_the_other_tables():
    from motioneditor_amd import build, capi
    build.build_lib(verbose=False)
    assert "attn_probs.hip" in build.SOURCES
    assert not set(capi.PROBE_SYMBOLS) & (set(capi.SYMBOLS) | set(capi.IO_SYMBOLS) | set(capi.TUNE_SYMBOLS) | set(capi.LONG_SYMBOLS))
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "motioned_probe.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(me_[a-z0-9_]+)\s*\(", header))
    assert declared == set(capi.PROBE_SYMBOLS) == {"me_attn_probs"}
    L = ctypes.CDLL(str(capi.LIB_PATH))
    for name in declared:
        getattr(L, name)
    bound = capi.lib()
    for name, (res, args) in capi.PROBE_SYMBOLS.items():
        assert getattr(bound, name).argtypes == args and getattr(bound, name).restype is res
    assert bound.me_abi_version() == capi.ABI_VERSION == 9       # ABI 9 stays: no existing struct or symbol changed
    for other in ("motioned.h", "motioned_io.h", "motioned_tune.h", "motioned_long.h"):
        assert "me_attn_probs" not in (ROOT / "include" / other).read_text()
    # the struct as the header lays it out (LP64): three pointers, eight int32, a pointer, an int32 + pad, two int64, three floats + pad
    assert ctypes.sizeof(capi.AttnProbsArgs) == 104
    assert [f[0] for f in capi.AttnProbsArgs._fields_] == re.findall(r"\b(\w+)(?=[,;])", re.search(r"struct me_attn_probs_args \{(.*?)\}", header, re.S).group(1))


def test_every_launching_probe_symbol_is_named_by_a_guard_case():
    from motioneditor_amd import capi
    import test_guard_probe_gpu
    guarded = set()
    for syms in test_guard_probe_gpu.GUARDED.values():
        guarded |= set(syms)
    assert guarded == set(capi.PROBE_SYMBOLS)


def _args(**over):
    from motioneditor_amd import capi
    a = capi.AttnProbsArgs()
    P = 4096   # never dereferenced: every call below is refused before a launch
    a.Q, a.K, a.P, a.kv_item = P, P, P, P
    a.ldq, a.ldk, a.ldp = 320, 640, 80
    a.heads, a.dh, a.n_items, a.nq, a.nk = 8, 40, 4, 256, 77
    a.scale, a.alpha, a.beta = 40 ** -0.5, 1.0, 0.0
    for n, v in over.items():
        setattr(a, n, v)
    return a


REFUSALS = [
    (dict(Q=None), "null pointer"), (dict(K=None), "null pointer"), (dict(P=None), "null pointer"), (dict(kv_item=None), "null pointer"),
    (dict(dh=64), "head dim must be 40, 80 or 160"), (dict(dh=0), "head dim"),
    (dict(nk=0), "nk must be 1 .. 128"), (dict(nk=129, ldp=136), "nk must be 1 .. 128"),
    (dict(ldp=76), "ldp must be >= nk"),
    (dict(ldq=324), "row strides"), (dict(ldk=321), "row strides"), (dict(hsq=44), "head strides"), (dict(hsk=10244), "head strides"), (dict(hsk=-8), "head strides"),
    (dict(Q=4096 + 8), "misaligned pointer"), (dict(K=4096 + 2), "misaligned pointer"), (dict(P=4096 + 2), "misaligned pointer"), (dict(kv_item=4096 + 1), "misaligned pointer"),
    (dict(q_items=-1), "q_items must be >= 0"),
    (dict(n_items=1 << 20, nq=256, heads=8), "below 2^31"),
    (dict(heads=0), "bad sizes"), (dict(n_items=0), "bad sizes"), (dict(nq=0), "bad sizes"),
]


@pytest.mark.parametrize("over,word", REFUSALS, ids=[f"{'-'.join(o)}-{i}" for i, (o, _) in enumerate(REFUSALS)])
def test_refusals_return_einval_with_their_message_before_any_launch(over, word):
    from motioneditor_amd import capi
    L = capi.lib()
    L.me_set_kernel(b"untouched")
    assert L.me_attn_probs(ctypes.byref(_args(**over)), None) == capi.ME_EINVAL
    msg = L.me_last_error().decode()
    assert msg.startswith("me_attn_probs:") and word in msg, msg
    assert L.me_last_kernel() == b"untouched"                     # nothing was launched
    with pytest.raises(ValueError, match="me_attn_probs"):
        capi.check(capi.ME_EINVAL, "me_attn_probs")


def test_a_recording_plan_captures_the_launch_without_a_device():
    """The launch goes through the library's launch hook: a recording plan holds it with its grid (one block per item and 64 queries) and me_last_kernel()
    names it (the launch itself fails here -- no device -- which the entry point reports as any other does)."""
    from motioneditor_amd import capi
    L = capi.lib()
    plan = ctypes.c_void_p()
    assert L.me_plan_begin(ctypes.byref(plan), 0x1000) == capi.ME_OK
    try:
        assert L.me_attn_probs(ctypes.byref(_args(nk=0)), 0x1000) == capi.ME_EINVAL           # refused: nothing recorded
        assert L.me_attn_probs(ctypes.byref(_args(n_items=3, nq=65, dh=80, ldq=640)), 0x1000) in (capi.ME_OK, capi.ME_EHIP)
        assert L.me_last_kernel() == b"attn_probs_kernel<80>"
        st, info = capi.PlanStats(), capi.PlanNodeInfo()
        assert L.me_plan_info(plan, ctypes.byref(st)) == capi.ME_OK and st.launches == 1
        assert L.me_plan_node(plan, 0, ctypes.byref(info), None, 0) == capi.ME_OK
        assert (info.kind, info.n_args) == (capi.PLAN_LAUNCH, 1) and tuple(info.grid) == (3 * 2, 1, 1) and tuple(info.block) == (256, 1, 1)
    finally:
        assert L.me_plan_end(plan) in (capi.ME_OK, capi.ME_EHIP)
        L.me_plan_destroy(plan)
