"""Guard-band cases for the clip I/O entries of include/motioned_io.h (capi.IO_SYMBOLS) on a real MI355X: me_image_resize and me_video_grid_u8 on views
with non-trivial strides inside allocations the test owns, through the protocol of tests/guard.py -- three launches on the same addresses with the input
surroundings changed, sentinels around every output, inputs unchanged -- plus the value check against tests/emu_image_ops.py.

Every operand is a 2-D guarded view (leading dimension larger than its width, 16- but not 32-byte aligned, guard rows above and below, guard columns left
and right) re-viewed in the layout the entry takes: images / channels / frames are runs of rows, so image, channel and row strides are all larger than the
packed ones.  Output widths are not multiples of the four pixels a thread stores, so the tail behind the last whole 16-byte (resize) / 12-byte (grid) store
runs in every case.  The fp32 video passes through the NaN / 0 / 6e4 surroundings unchanged; the uint8 source has no NaN and takes integer surroundings
(255, 0, 128), as the index tables of tests/test_guard_gpu.py do.

GUARDED maps every case to the symbols it drives; tests/test_clip_io_cpu.py checks it against capi.IO_SYMBOLS without a GPU, and on the GPU the decorator
counts the calls, so a case that stops reaching a symbol it names fails.  (A table of its own: tests/test_guard_gpu.py's GUARDED is checked against
capi.SYMBOLS.)"""
import fnmatch
import functools

import pytest
import torch

import emu_image_ops as emu_img
from clip_io_fixture import BILINEAR_ATOL, images_u8
from guard import embed_in, run_guarded, sentinel_out

pytestmark = pytest.mark.gpu

GUARDED = {}
U8_SURROUNDINGS = (255, 0, 128)


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


def kernel_is(ops, want):
    got = ops._last_kernel()
    print("kernel:", got)
    assert fnmatch.fnmatchcase(got, want), f"the case was written for {want}, the launch took {got}"


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
@pytest.mark.parametrize("n,H,W,C,oh,ow", [(3, 37, 53, 3, 24, 46), (2, 20, 31, 3, 33, 61), (3, 37, 53, 1, 24, 45), (2, 16, 18, 1, 16, 18), (1, 9, 7, 3, 5, 3)])
@guards("me_image_resize")
def test_guard_image_resize(ops, n, H, W, C, oh, ow, mode):
    """ow % 4 != 0 everywhere (ow = 3: no whole vector at all); up- and down-scaling, so the taps reach the last row and the last column of every image."""
    src = images_u8(n, H, W, C, seed=H * 100 + ow)
    s2 = embed_in(src.reshape(n * H, W * C), device="cuda", row_guard=8, col_guard=64, int_poison=U8_SURROUNDINGS, name="src")
    o2, _ = sentinel_out((n * C * oh, ow), torch.float32, device="cuda", row_guard=8, col_guard=64, name="out")
    s4, o4 = s2.view(n, H, W, C), o2.view(n, C, oh, ow)
    assert s4.stride(1) > W * C and o4.stride(2) > ow and s4.data_ptr() == s2.data_ptr() and o4.data_ptr() == o2.data_ptr()
    div, add = (127.5, -1.0) if C == 3 else (255.0, 0.0)
    got = run_guarded(lambda: ops.image_resize(s4, (oh, ow), mode, div=div, add=add, out=o4), {"src": s2}, {"out": o2})["out"].cpu().view(n, C, oh, ow)
    kernel_is(ops, f"image_resize_kernel<{C},{mode}>")
    want = emu_img.image_resize(src, (oh, ow), mode, div=div, add=add)
    err = float((got - want).abs().max()) * div
    print(f"guard image_resize {mode} {(n, H, W, C)} -> {(oh, ow)}: max |kernel - emulation| = {err:.3e} pixel units")
    if mode == "nearest" or (H, W) == (oh, ow):
        assert torch.equal(got, want)
    else:
        assert err <= BILINEAR_ATOL


@pytest.mark.parametrize("rescale", [False, True])
@pytest.mark.parametrize("b,c,f,h,w", [(5, 3, 3, 6, 9), (1, 3, 2, 7, 9), (2, 1, 2, 5, 10), (4, 3, 1, 3, 1)])
@guards("me_video_grid_u8")
def test_guard_video_grid_u8(ops, b, c, f, h, w, rescale):
    """b = 5 at n_rows = 4: three empty cells in the second row, which must be written (as the grid's padding) and nothing beyond Hg x Wg; Wg = 46, 9, 26, 14:
    never a multiple of 4."""
    g = torch.Generator().manual_seed(b * 10 + c)
    v = torch.rand(b, c, f, h, w, generator=g)
    if rescale:
        v = v * 2 - 1
    Hg, Wg = emu_img.grid_size(b, h, w, 4)
    assert Wg % 4
    v2 = embed_in(v.reshape(b * c * f * h, w), device="cuda", row_guard=8, col_guard=64, name="videos")
    o2, _ = sentinel_out((f * Hg, Wg * 3), torch.uint8, device="cuda", row_guard=8, col_guard=64, name="out")
    v5, o4 = v2.view(b, c, f, h, w), o2.view(f, Hg, Wg, 3)
    assert v5.stride(3) > w and o4.stride(1) > 3 * Wg
    got = run_guarded(lambda: ops.video_grid_u8(v5, n_rows=4, rescale=rescale, out=o4), {"videos": v2}, {"out": o2})["out"].cpu().view(f, Hg, Wg, 3)
    kernel_is(ops, "video_grid_u8_kernel")
    assert torch.equal(got, emu_img.video_grid_u8(v, n_rows=4, rescale=rescale))
    if b == 5:
        pad = 127 if rescale else 0
        assert bool((got[:, h + 4:, w + 4:] == pad).all()) and bool((got[:, :2] == pad).all()) and bool((got[:, :, -2:] == pad).all())
