"""Guard-band cases for the entries of include/motioned_vision.h (capi.VISION_SYMBOLS) on a real MI355X, through the protocol of tests/guard.py: three launches
on the same addresses with the input surroundings NaN / 0 / 6e4 (integer inputs: 0 / 1 / 2).  Every operand is a view inside an allocation the test owns
(16- but not 32-byte aligned, 2-D views with a row pitch larger than the width and guard rows above and below): everything around the views stays bitwise
intact, the results are finite, bitwise equal across the launches and equal to the emulation (tests/emu_clip_vision_ops.py) within the kernel's bound.
The shapes leave the last tile short: 257 keys (one key alone in its tile, a pair tile of padding), 50 and 17 keys, 65 queries' worth of blocks; K = 588
patch columns padded to 592; image widths that are no multiple of anything."""
import functools

import numpy as np
import pytest
import torch

import clip_vision_fixture as fx
import emu_clip_vision_ops as emu
import guard

pytestmark = pytest.mark.gpu

GUARDED = {}


def guards(*symbols):
    """Names the symbols a case drives (tests/test_clip_vision_cpu.py checks the map against capi.VISION_SYMBOLS) and counts the calls: a case that stops
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


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the HIP library is the only compute path")
    from motioneditor_amd import capi, ops as _ops
    capi.lib()
    return _ops


@pytest.mark.parametrize("n_seq,heads,n", [(2, 2, 257), (1, 3, 50), (2, 1, 17), (1, 1, 65)])
@guards("me_attn_full")
def test_guard_attention_full(ops, n_seq, heads, n):
    C = heads * 64
    qkv = guard.rnd(n_seq * n, 3 * C, seed=n)
    qkv[:, :2 * C] *= 3
    ins = {"qkv": guard.embed_in(qkv, device="cuda")}
    out, _ = guard.sentinel_out((n_seq * n, C))
    v = ins["qkv"]
    got = guard.run_guarded(lambda: ops.attention_full(v[:, :C], v[:, C:2 * C], v[:, 2 * C:], heads=heads, dh=64, n_seq=n_seq, n=n, out=out), ins, {"o": out})["o"]
    guard.check(got, emu.attention_full(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], heads=heads, dh=64, n_seq=n_seq, n=n), f"attention_full {n_seq}x{heads}x{n} under guard")


@pytest.mark.parametrize("n,S,patch", [(2, 28, 14), (1, 64, 32), (3, 15, 5)])
@guards("me_patch_rows")
def test_guard_patch_rows(ops, n, S, patch):
    pv = torch.from_numpy(fx.pixel_values(n, S))
    ins = {"pv": guard.embed_in(pv, device="cuda")}
    g, kpad = S // patch, (3 * patch * patch + 7) // 8 * 8
    out, _ = guard.sentinel_out((n * g * g, kpad))
    got = guard.run_guarded(lambda: ops.patch_rows(ins["pv"], patch, out=out), ins, {"rows": out})["rows"].cpu()
    assert torch.equal(got, emu.patch_rows(pv, patch, dtype=torch.float16))


@pytest.mark.parametrize("n,g2,C", [(2, 4, 64), (3, 49, 72), (1, 256, 256)])
@guards("me_vit_tokens")
def test_guard_vit_tokens(ops, n, g2, C):
    po, cls, pos = guard.rnd(n * g2, C, seed=1), guard.rnd(C, seed=2), guard.rnd(g2 + 1, C, seed=3)
    ins = {"po": guard.embed_in(po, device="cuda"), "cls": guard.embed_in(cls, device="cuda", contiguous=True), "pos": guard.embed_in(pos, device="cuda", contiguous=True)}
    out, _ = guard.sentinel_out((n * (g2 + 1), C))
    got = guard.run_guarded(lambda: ops.vit_tokens(ins["po"], ins["cls"], ins["pos"], n, out=out), ins, {"x": out})["x"].cpu()
    assert torch.equal(got, emu.vit_tokens(po, cls, pos, n))


@pytest.mark.parametrize("i,axis", [(0, 0), (0, 1), (2, 0), (1, 1)])
@guards("me_resample_u8")
def test_guard_resample_u8(ops, i, axis):
    from motioneditor_amd import vision
    im = torch.from_numpy(np.stack([fx.images()[i], fx.images()[i][::-1].copy()]))
    n, H, W, _ = im.shape
    osz = 37 if i == 1 else 224         # image 1 (150 x 113): a 4x shrink, 17 taps
    b, c, _ = vision.resample_tables(H if axis else W, osz)
    ins = {"src": guard.embed_in(im, device="cuda"), "bounds": guard.embed_in(torch.from_numpy(b), device="cuda", contiguous=True, int_poison=(0, 1, 2)),
           "coef": guard.embed_in(torch.from_numpy(c), device="cuda", contiguous=True, int_poison=(0, 1 << 22, -(1 << 20)))}
    shape = (n, osz, W, 3) if axis else (n, H, osz, 3)
    out, _ = guard.sentinel_out(shape, torch.uint8, contiguous=True)
    got = guard.run_guarded(lambda: ops.resample_u8(ins["src"], osz, axis, ins["bounds"], ins["coef"], out=out), ins, {"y": out})["y"].cpu()
    assert torch.equal(got, emu.resample_u8(im, osz, axis))


@guards("me_crop_normalize")
def test_guard_crop_normalize(ops):
    from motioneditor_amd.models.clip import OPENAI_CLIP_MEAN, OPENAI_CLIP_STD
    im = torch.from_numpy(np.stack([fx.images()[0], fx.images()[0][:, ::-1].copy()]))     # 96 x 128
    ins = {"src": guard.embed_in(im, device="cuda")}
    out, _ = guard.sentinel_out((2, 3, 50, 61), torch.float32, contiguous=True)
    got = guard.run_guarded(lambda: ops.crop_normalize(ins["src"], 23, 33, (50, 61), OPENAI_CLIP_MEAN, OPENAI_CLIP_STD, out=out), ins, {"pv": out})["pv"].cpu()
    assert torch.equal(got, emu.crop_normalize(im, 23, 33, (50, 61), OPENAI_CLIP_MEAN, OPENAI_CLIP_STD))


@pytest.mark.parametrize("rows,C,shared", [(7, 768, False), (5, 64, True), (1, 33, False), (23, 100, True)])
@guards("me_cosine_rows")
def test_guard_cosine_rows(ops, rows, C, shared):
    a, b = guard.rnd(rows, C, seed=5).float() + 0.3, guard.rnd(1 if shared else rows, C, seed=6).float()
    ins = {"a": guard.embed_in(a, device="cuda"), "b": guard.embed_in(b, device="cuda")}
    out, _ = guard.sentinel_out((rows,), torch.float32)
    got = guard.run_guarded(lambda: ops.cosine_rows(ins["a"], ins["b"], out=out), ins, {"cos": out})["cos"].cpu()
    want = (a.double() * b.double()).sum(1) / (a.double().norm(dim=1) * b.double().norm(dim=1))
    assert float((got.double() - want).abs().max()) <= 1e-6       # (the value bound is tests/test_clip_vision_gpu.py's business: this is the guard case)
