"""Clip I/O on a real MI355X: the two kernels of csrc/image.hip against their CPU emulation (tests/emu_image_ops.py, itself held to F.interpolate and the
make_grid rules by tests/test_clip_io_cpu.py), at that suite's cases and at the shipping geometry; reproducibility bit for bit; VideoDataset on the device
against the emulated one; and the harness sequence of examples/run_edit.py fed from a clip folder and written back as GIF / PNG.

Bounds: nearest, the identity resize (affine included) and the uint8 grid bitwise; bilinear within 16 ulp(256) = 4.9e-4 in pixel units before the affine."""
import io
import sys

import numpy as np
import pytest
import torch

import emu_image_ops as emu_img
from clip_io_fixture import BILINEAR_ATOL, RESIZE_CASES, images_u8, write_clip
from conftest import ROOT

pytestmark = pytest.mark.gpu

SHIPPING = [((512, 512), (512, 512)), ((480, 854), (512, 512))]      # 8 frames x 3 channels: case-1 as shipped (identity), a 480p source


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the HIP library is the only compute path")
    from motioneditor_amd import capi, ops as _ops
    capi.lib()
    return _ops


def _resize_case(ops, src, ohw, mode, div, add, what):
    got = ops.image_resize(src.cuda(), ohw, mode, div=div, add=add)
    again = ops.image_resize(src.cuda(), ohw, mode, div=div, add=add)
    torch.cuda.synchronize()
    assert ops._last_kernel() == f"image_resize_kernel<{src.shape[3] if src.dim() == 4 else 1},{mode}>"
    want = emu_img.image_resize(src, ohw, mode, div=div, add=add)
    assert got.dtype == torch.float32 and got.shape == want.shape and got.is_contiguous()
    assert torch.equal(got, again), f"{what}: two runs differ"
    err = float((got.cpu() - want).abs().max()) * div
    print(f"{what} {mode} {tuple(src.shape)} -> {ohw}: max |kernel - emulation| = {err:.3e} pixel units (bilinear bound {BILINEAR_ATOL:.3e})")
    if mode == "nearest" or tuple(src.shape[1:3]) == tuple(ohw):
        assert torch.equal(got.cpu(), want), what
    else:
        assert err <= BILINEAR_ATOL, what
    return got


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
@pytest.mark.parametrize("C", [3, 1, 0])
@pytest.mark.parametrize("hw,ohw", RESIZE_CASES)
def test_image_resize_matches_the_emulation(ops, hw, ohw, C, mode):
    src = images_u8(3, hw[0], hw[1], C, seed=hw[0] * 1000 + ohw[0] + C)
    _resize_case(ops, src, ohw, mode, 1.0, 0.0, "plain")
    _resize_case(ops, src, ohw, mode, 127.5, -1.0, "frames")
    _resize_case(ops, src, ohw, mode, 255.0, 0.0, "conditions")


@pytest.mark.parametrize("hw,ohw", SHIPPING)
def test_image_resize_at_the_shipping_geometry(ops, hw, ohw):
    src = images_u8(8, hw[0], hw[1], 3, seed=hw[1])
    pv = _resize_case(ops, src, ohw, "bilinear", 127.5, -1.0, "pixel_values")
    assert -1.0 <= float(pv.min()) and float(pv.max()) <= 1.0
    _resize_case(ops, src, ohw, "bilinear", 255.0, 0.0, "conditions")


@pytest.mark.parametrize("ohw", [(512, 512), (128, 128)])
def test_mask_resize_at_the_shipping_geometry(ops, ohw):
    masks = (images_u8(8, 512, 512, 0, seed=9) > 127).to(torch.uint8) * 255
    m = _resize_case(ops, masks, ohw, "nearest", 255.0, 0.0, "masks")
    assert tuple(m.shape) == (8, 1, *ohw) and set(m.unique().tolist()) == {0.0, 1.0}


def test_image_resize_on_views_the_vector_store_cannot_take(ops):
    """An output view whose rows start 4 bytes off a 16-byte boundary and a source cropped out of a wider frame: the scalar store path, explicit strides."""
    wide = images_u8(2, 40, 70, 3, seed=4)
    src = wide[:, 3:37, 5:58]                                   # [2, 34, 53, 3] inside [2, 40, 70, 3]
    buf = torch.full((2, 3, 24, 50), -7.0, device="cuda")
    out = buf[..., 1:48]                                        # ow = 47
    got = ops.image_resize(wide.cuda()[:, 3:37, 5:58], (24, 47), "bilinear", div=255.0, out=out)
    torch.cuda.synchronize()
    assert got is out and out.data_ptr() % 16 == 4
    assert float((out.cpu() - emu_img.image_resize(src.contiguous(), (24, 47), "bilinear", div=255.0)).abs().max()) * 255 <= BILINEAR_ATOL
    assert bool((buf[..., :1] == -7.0).all()) and bool((buf[..., 48:] == -7.0).all())
    with pytest.raises(ValueError):
        ops.image_resize(wide.cuda().permute(0, 2, 1, 3), (24, 47))          # pixels not interleaved along x
    with pytest.raises(ValueError):
        ops.image_resize(wide.cuda(), (24, 47), out=buf)                      # wrong shape


@pytest.mark.parametrize("rescale", [False, True])
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("b", [1, 2, 4, 5])
def test_video_grid_matches_the_emulation(ops, b, c, rescale):
    f, h, w = 3, 6, 9
    g = torch.Generator().manual_seed(b * 10 + c)
    v = torch.rand(b, c, f, h, w, generator=g)
    v[0, 0, 0, 0, :3] = torch.tensor([0.0, 1.0, 0.5])
    if rescale:
        v = v * 2 - 1
    got, again = ops.video_grid_u8(v.cuda(), n_rows=4, rescale=rescale), ops.video_grid_u8(v.cuda(), n_rows=4, rescale=rescale)
    torch.cuda.synchronize()
    assert ops._last_kernel() == "video_grid_u8_kernel" and got.dtype == torch.uint8 and tuple(got.shape) == (f, *ops.grid_size(b, h, w, 4), 3)
    assert torch.equal(got, again) and torch.equal(got.cpu(), emu_img.video_grid_u8(v, n_rows=4, rescale=rescale))


def test_video_grid_at_the_shipping_geometry_and_outside_the_range(ops):
    g = torch.Generator().manual_seed(2)
    v = torch.rand(2, 3, 8, 512, 512, generator=g)
    got, again = ops.video_grid_u8(v.cuda()), ops.video_grid_u8(v.cuda())
    assert tuple(got.shape) == (8, 516, 1030, 3) and torch.equal(got, again) and torch.equal(got.cpu(), emu_img.video_grid_u8(v))
    edge = torch.tensor([-0.5, -1e-3, 0.0, 0.999, 1.0, 1.004, 1.5, 300.0, float("inf"), float("-inf"), float("nan"), 0.5]).reshape(1, 1, 1, 2, 6)
    assert ops.video_grid_u8(edge.cuda()).reshape(12, 3)[:, 0].tolist() == [0, 0, 0, 254, 255, 255, 255, 255, 255, 0, 0, 127]     # clamped where numpy wraps
    wide = (torch.randn(3, 3, 2, 5, 7, generator=g) * 2)
    assert torch.equal(ops.video_grid_u8(wide.cuda(), n_rows=2, rescale=True).cpu(), emu_img.video_grid_u8(wide, n_rows=2, rescale=True))


# ------------------------------------------------------------------ VideoDataset on the device
def _datasets(root, monkeypatch, **kw):
    from motioneditor_amd import ops as _ops
    from motioneditor_amd.data.dataset import VideoDataset
    args = dict(width=32, height=24, n_sample_frames=4, condition=["openposefull"], video_suffix=".png", source_mask_dir="man.mask")
    args.update(kw)
    dev = VideoDataset(str(root), "a girl is dancing", device="cuda", **args)[0]
    with monkeypatch.context() as m:
        m.setattr(_ops, "image_resize", emu_img.image_resize)
        cpu = VideoDataset(str(root), "a girl is dancing", device="cpu", **args)[0]
    return dev, cpu


def test_dataset_on_the_device_equals_the_emulated_dataset(ops, tmp_path, monkeypatch):
    write_clip(tmp_path)
    dev, cpu = _datasets(tmp_path, monkeypatch, sample_start_idx=1, sample_frame_rate=2)
    assert dev["pixel_values"].is_cuda and dev["source_masks"].is_cuda and dev["source_conditions"]["openposefull"].is_cuda
    assert dev["sample_indices"].tolist() == cpu["sample_indices"].tolist() == [1, 3, 5, 7]
    for what, a, b, div in (("pixel_values", dev["pixel_values"], cpu["pixel_values"], 127.5),
                            ("source_conditions", dev["source_conditions"]["openposefull"], cpu["source_conditions"]["openposefull"], 255.0),
                            ("target_conditions", dev["target_conditions"]["openposefull"], cpu["target_conditions"]["openposefull"], 255.0)):
        err = float((a.cpu() - b).abs().max()) * div
        print(f"dataset {what}: max |device - emulation| = {err:.3e} pixel units")
        assert a.dtype == torch.float32 and a.shape == b.shape and err <= BILINEAR_ATOL
    assert torch.equal(dev["source_masks"].cpu(), cpu["source_masks"])
    same, cpu_same = _datasets(tmp_path, monkeypatch, width=56, height=40, source_mask_dir=None)          # the clip's own size: the identity, bitwise
    assert torch.equal(same["pixel_values"].cpu(), cpu_same["pixel_values"]) and bool((same["source_masks"] == 1).all()) and same["source_masks"].is_cuda


# ------------------------------------------------------------------ end to end
def test_run_edit_from_a_clip_folder_to_gif_and_png(ops, tmp_path, unet_sd_np, cn_sd_np):
    """examples/run_edit.py --video-dir ... --out ...: the harness sequence on a batch from VideoDataset (8 frames at 128 x 128 from a 40 x 56 clip, synthetic
    weights), the files written from the returned tensors, and the same sequence fed the same pixel tensor by hand."""
    from PIL import Image
    sys.path.insert(0, str(ROOT / "examples"))
    import run_edit
    from motioneditor_amd import util
    from motioneditor_amd.models.controlnet import ControlNetModel
    from motioneditor_amd.models.unet_2d_condition import UNet2DConditionModel
    from motioneditor_amd.models.vae import AutoencoderKL
    from motioneditor_amd.pipelines import MotionEditorPipeline
    write_clip(tmp_path / "case")
    f, H = 8, 128
    a = run_edit.parser().parse_args(["--video-dir", str(tmp_path / "case"), "--mask-dir", "man.mask", "--frames", str(f), "--size", str(H), "--out", str(tmp_path / "out")])
    pipe = MotionEditorPipeline(vae=AutoencoderKL.from_synthetic("cuda"), unet=UNet2DConditionModel(unet_sd_np, "cuda:0"), controlnet=ControlNetModel(cn_sd_np, "cuda:0"))
    x = run_edit.clip_inputs(a)
    assert tuple(x["pixel_values"].shape) == (1, f, 3, H, H) and x["pixel_values"].is_cuda and tuple(x["source_masks"].shape) == (1, f, 1, H, H)
    s_inv, s_gen, inv_lat = run_edit.run(pipe, x, steps=2, inv_steps=2)
    assert tuple(s_gen.shape) == tuple(s_inv.shape) == (1, 3, f, H, H) and bool(torch.isfinite(s_gen).all()) and bool(torch.isfinite(s_inv).all())
    # the writers: GIF and PNG frames are videos_to_grid_frames of the returned tensors
    paths = run_edit.save_samples(a.out, "a boy is dancing", s_inv, s_gen)
    for path, sample in zip(paths, (s_gen, s_inv)):
        frames = util.videos_to_grid_frames(sample)
        assert tuple(frames.shape) == (f, H, H, 3) and torch.equal(frames, emu_img.video_grid_u8(sample.float().cpu()))
        with Image.open(path) as im:
            assert im.n_frames == f and im.size == (H, H) and im.info.get("loop") == 0
            for t in range(f):
                im.seek(t)
                rgb = np.asarray(im.convert("RGB"))
                # a GIF frame holds at most 256 colours: the file's frame is the grid frame through the format's own palette (PIL's quantiser on that frame
                # alone), and the grid frame itself where it has no more colours than that
                alone = io.BytesIO()
                Image.fromarray(frames[t].numpy()).save(alone, format="GIF")
                alone.seek(0)
                with Image.open(alone) as one:
                    assert np.array_equal(rgb, np.asarray(one.convert("RGB"))), (path, t)
                if len(np.unique(frames[t].numpy().reshape(-1, 3), axis=0)) <= 256:
                    assert np.array_equal(rgb, frames[t].numpy())
    util.save_videos_as_images(s_gen, str(tmp_path / "out"))
    frames = util.videos_to_grid_frames(s_gen)
    for t in range(f):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / "vis_images" / "batch_0" / f"frame_{t}.png")), frames[t].numpy())
    # the same pixel tensor fed by hand: bit for bit the same latents and samples
    pipe.unet.spatial_editor = pipe.unet.temporal_editor = None
    hand = {k: v.cuda() for k, v in run_edit.harness_inputs(f, H, H).items()}
    hand.update(pixel_values=x["pixel_values"].clone(), target_skeleton=x["target_skeleton"].clone(), source_masks=x["source_masks"].clone())
    h_inv, h_gen, h_lat = run_edit.run(pipe, hand, steps=2, inv_steps=2)
    assert torch.equal(inv_lat, h_lat) and torch.equal(s_inv, h_inv) and torch.equal(s_gen, h_gen)
