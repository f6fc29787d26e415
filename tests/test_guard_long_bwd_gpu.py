"""Guard-band cases for the entry of include/motioned_long.h (capi.LONG_SYMBOLS) on a real MI355X, through the protocol of tests/guard.py: three launches of
me_tattn_bwd_long on the same addresses with the input surroundings NaN / 0 / 6e4; q, k, v, dout, the three gradients AND the scratch are views inside
allocations the test owns (16- but not 32-byte aligned, row pitch larger than the width, guard rows above and below), every surrounding bitwise intact, the
results finite, bitwise equal across the launches and inside the case's bound.  The last 64-frame block of every case holds pad frames (72, 136, 129 frames):
a kernel that read or wrote them would touch the guard rows, or the next batch entry.

GUARDED maps every case to the symbols it drives; tests/test_long_bwd_cpu.py checks it against capi.LONG_SYMBOLS without a GPU, and on the GPU the decorator
counts the calls, so a case that stops reaching a symbol it names fails."""
import functools

import pytest
import torch

import bwd_run as br
import guard
import long_bwd_cases as lb
import ref64_bwd as ref

pytestmark = pytest.mark.gpu

GUARDED = {}


def guards(*symbols):
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


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the HIP library is the only compute path")
    from motioneditor_amd import capi, ops as _ops
    capi.lib()
    return _ops


@pytest.mark.parametrize("cid", lb.GUARDED)
@guards("me_tattn_bwd_long")
def test_guard_temporal_attention_bwd_long(ops, cid):
    from motioneditor_amd import capi
    L = capi.lib()
    case = lb.BY_ID[cid]
    p, t = case.p, lb.build(case)
    heads, dh, batch, frames, npix = p["heads"], p["dh"], p["batch"], p["frames"], p["npix"]
    C, rows = heads * dh, batch * frames * npix
    ins = {n: guard.embed_in(t["qkv"][:, i * C:(i + 1) * C].contiguous(), device="cuda") for i, n in enumerate(("q", "k", "v"))}
    ins["dout"] = guard.embed_in(t["dout"], device="cuda")
    outs = {n: guard.sentinel_out((rows, C), torch.float32)[0] for n in ("dq", "dk", "dv")}
    nbytes = lb.work_bytes(batch, frames, npix, heads)
    outs["work"] = guard.sentinel_out((nbytes // 4,), torch.float32, contiguous=True)[0]        # every element of it is written: lse and delta of every (row, head)

    def launch():
        a = [x for n in ("dq", "dk", "dv") for x in (outs[n].data_ptr(), outs[n].stride(0))] + [x for n in ("q", "k", "v", "dout") for x in (ins[n].data_ptr(), ins[n].stride(0))]
        capi.check(L.me_tattn_bwd_long(*a, batch, frames, npix, heads, dh, p.get("scale") or dh ** -0.5, outs["work"].data_ptr(), nbytes, ops._stream()), "me_tattn_bwd_long")
    got = guard.run_guarded(launch, ins, outs)
    assert br.kernel_matches(L.me_last_kernel().decode(), case.path), L.me_last_kernel().decode()
    want = br.run(case, ref, t, br.to_ref)
    br.compare(case, {n: got[n].cpu() for n in ("dq", "dk", "dv")}, want, who="HIP under guard")
    # the scratch holds what the header says: the log2-domain log-sum-exp and delta = sum_j P dP per (row, head)
    lse = got["work"][:rows * heads].cpu().double().reshape(rows, heads)
    qd, kd = (t["qkv"][:, i * C:(i + 1) * C].double().reshape(batch, frames, npix, heads, dh).permute(0, 2, 3, 1, 4) for i in range(2))
    s = (qd @ kd.transpose(-1, -2)) * (p.get("scale") or dh ** -0.5)
    s = s.masked_fill(torch.arange(frames)[None, :] > torch.arange(frames)[:, None], float("-inf"))
    want_lse = (torch.logsumexp(s, dim=-1) * lb.LOG2E).permute(0, 3, 1, 2).reshape(rows, heads)
    assert float((lse - want_lse).abs().max()) < 2e-2      # the bound bwd_run applies to the log-sum-exp the spatial forward stashes
