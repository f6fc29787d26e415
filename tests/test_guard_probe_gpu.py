"""Guard-band cases for the entry of include/motioned_probe.h (capi.PROBE_SYMBOLS) on a real MI355X, through the protocol of tests/guard.py: three launches
of me_attn_probs on the same addresses with the input surroundings NaN / 0 / 6e4.  Q, K, the kv_item table and P are views inside allocations the test owns
(16- but not 32-byte aligned, row pitch larger than the width, guard rows above and below): the rows before and after every view and the columns >= nk of P
stay bitwise intact, the results are finite, bitwise equal across the launches and inside the case's bound.  The P of a beta = 0 call starts as a NaN
sentinel, view included: a kernel that read it would return it.  The query counts leave the last wave and the last block short (17, 65, 70 queries), the key
counts the last MFMA tile and the second 64-key store (17, 77, 128 keys): a kernel that read or wrote the pad would touch a guard."""
import pytest
import torch

import functools

import guard
import probe_cases as pc

pytestmark = pytest.mark.gpu

GUARDED = {}


def guards(*symbols):
    """Names the symbols a case drives (tests/test_probe_cpu.py checks the map against capi.PROBE_SYMBOLS) and counts the calls: a case that stops
    reaching a symbol it names fails."""
    def deco(fn):
        GUARDED[fn.__name__] = symbols

        @functools.wraps(fn)
        def run(*a, **kw):
            from motioneditor_amd import capi
            L, calls, saved = capi.lib(), dict.fromkeys(symbols, 0), {}
            for s in symbols:
                saved[s] = getattr(L, s)

                def spy(*args, _s=s):
                    calls[_s] += 1
                    return saved[_s](*args)
                setattr(L, s, spy)
            try:
                fn(*a, **kw)
            finally:
                for s in symbols:
                    setattr(L, s, saved[s])
            assert all(calls.values()), f"the case never reached {[s for s, n in calls.items() if not n]}"
        return run
    return deco


CASES = ("nq17", "nq65", "nk17", "nk128", "ldp80", "hm-q-hm-k", "hm-q-row-k", "shared-queries", "dh160-h1", "beta1-three-times")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the HIP library is the only compute path")
    from motioneditor_amd import capi, ops as _ops
    capi.lib()
    return _ops


@pytest.mark.parametrize("cid", CASES)
@guards("me_attn_probs")
def test_guard_attention_probs(ops, cid):
    c = pc.BY_ID[cid]
    t = pc.build(c)
    rows = c.n_items * c.nq
    ins = {"q": guard.embed_in(t["q"].contiguous(), device="cuda"), "k": guard.embed_in(t["k"].contiguous(), device="cuda"),
           "kv_item": guard.embed_in(t["kv_item"], device="cuda", contiguous=True, int_poison=(0, 1, 0))}
    if c.beta == 0:
        outs, inout = {"P": guard.sentinel_out((rows, c.nk), torch.float32)[0]}, ()
        P = outs["P"]
    else:      # accumulated into: restored to zeros before every launch, its surroundings poisoned
        ins["P"] = guard.embed_in(torch.zeros((rows, c.nk), dtype=torch.float32), device="cuda")
        outs, inout, P = {}, ("P",), ins["P"]

    def launch():
        for _ in range(1 if c.beta == 0 else 3):
            ops.attention_probs(ins["q"], ins["k"], kv_item=ins["kv_item"], out=P, beta=c.beta, **t["kw"])
    got = guard.run_guarded(launch, ins, outs, inout)["P"].cpu()
    err = float((got.double() - pc.reference(c)).abs().max())
    print(f"{cid} under guard: max |err| {err:.3e} (bound {pc.bound(c):.3e})")
    assert err <= pc.bound(c)
