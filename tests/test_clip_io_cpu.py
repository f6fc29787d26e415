"""Clip I/O without a GPU: the emulation of the two image kernels (tests/emu_image_ops.py) against torch's own F.interpolate and a numpy restatement of
torchvision's make_grid; data.dataset.VideoDataset and the video writers of util on the emulated ops; the ABI table of include/motioned_io.h
(capi.IO_SYMBOLS), its argument validation without a device, and the guard rule of tests/test_guard_cpu.py applied to that table.

Bounds (stated before any of this ran): nearest and the identity resize bitwise, affine included; bilinear otherwise within 16 ulp(256) = 4.9e-4 in pixel
units before the affine -- the error of a four-term convex combination of integers below 256 in fp32, so a failure is a coordinate mismatch, not noise;
the uint8 grid bitwise on inputs in range."""
import ctypes
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import emu_image_ops as emu_img
from clip_io_fixture import BILINEAR_ATOL, RESIZE_CASES, images_u8, make_grid_numpy, tree_digest, write_clip
from conftest import ROOT

sys.path.insert(0, str(ROOT / "examples"))


@pytest.fixture
def emulated(monkeypatch):
    """ops.image_resize / ops.video_grid_u8 -> the CPU emulation; CPU tensors handed to the writers stay on the CPU."""
    from motioneditor_amd import ops, util
    monkeypatch.setattr(ops, "image_resize", emu_img.image_resize)
    monkeypatch.setattr(ops, "video_grid_u8", emu_img.video_grid_u8)
    monkeypatch.setattr(util, "UPLOAD_DEVICE", "cpu")
    return ops


def _ref(src, size, mode):
    x = src if src.dim() == 4 else src[..., None]
    return F.interpolate(x.permute(0, 3, 1, 2).float(), size=size, mode=mode)


# ------------------------------------------------------------------ the emulation against torch
@pytest.mark.parametrize("C", [3, 1, 0])
@pytest.mark.parametrize("hw,ohw", RESIZE_CASES)
def test_emulated_resize_matches_f_interpolate(hw, ohw, C):
    src = images_u8(3, hw[0], hw[1], C, seed=hw[0] * 1000 + ohw[0] + C)
    near = emu_img.image_resize(src, ohw, "nearest")
    assert near.dtype == torch.float32 and tuple(near.shape) == (3, max(C, 1), *ohw)
    assert torch.equal(near, _ref(src, ohw, "nearest"))
    assert torch.equal(emu_img.image_resize(src, ohw, "nearest", div=255.0), _ref(src, ohw, "nearest") / 255)
    got, want = emu_img.image_resize(src, ohw, "bilinear"), _ref(src, ohw, "bilinear")
    err = float((got - want).abs().max())
    print(f"bilinear {hw} -> {ohw}, C = {C}: max |emulation - F.interpolate| = {err:.3e} pixel units (bound {BILINEAR_ATOL:.3e})")
    if hw == ohw:
        assert torch.equal(got, want)
        assert torch.equal(emu_img.image_resize(src, ohw, "bilinear", div=127.5, add=-1.0), want / 127.5 - 1.0)
        assert torch.equal(emu_img.image_resize(src, ohw, "bilinear", div=255.0), want / 255)
    else:
        assert err <= BILINEAR_ATOL
    out = torch.full((3, max(C, 1), ohw[0], ohw[1] + 3), -7.0)[..., 1:-2]                # out= takes a strided view
    assert emu_img.image_resize(src, ohw, "bilinear", div=127.5, add=-1.0, out=out) is out
    assert torch.equal(out, got / 127.5 - 1.0)


def test_emulated_resize_refuses_what_the_wrapper_refuses():
    src = images_u8(1, 8, 8, 3, seed=1)
    for bad in (lambda: emu_img.image_resize(src, (4, 4), "bicubic"), lambda: emu_img.image_resize(src.float(), (4, 4)), lambda: emu_img.image_resize(src, (0, 4)),
                lambda: emu_img.image_resize(images_u8(1, 8, 8, 2, seed=1), (4, 4))):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("rescale", [False, True])
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("b", [1, 2, 4, 5])
def test_emulated_grid_matches_the_make_grid_rules(b, c, rescale):
    f, h, w = 3, 6, 9
    g = torch.Generator().manual_seed(b * 10 + c)
    v = torch.rand(b, c, f, h, w, generator=g)
    v[0, 0, 0, 0, :3] = torch.tensor([0.0, 1.0, 0.5])
    if rescale:
        v = v * 2 - 1
    got = emu_img.video_grid_u8(v, n_rows=4, rescale=rescale)
    Hg, Wg = emu_img.grid_size(b, h, w, 4)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (f, Hg, Wg, 3)
    assert (Hg, Wg) == ((h, w) if b == 1 else ((h + 2) * (2 if b == 5 else 1) + 2, (w + 2) * min(4, b) + 2))
    assert np.array_equal(got.numpy(), make_grid_numpy(v.numpy(), 4, rescale))
    if b == 5:   # the three empty cells of the second row hold the grid's padding: 0, or (0 + 1) / 2 * 255 truncated
        assert bool((got[:, h + 4:, w + 4:] == (127 if rescale else 0)).all())
    if b > 1:
        assert bool((got[:, :2] == (127 if rescale else 0)).all()) and bool((got[:, :, :2] == (127 if rescale else 0)).all())


def test_emulated_grid_clamps_where_numpy_wraps():
    v = torch.tensor([-0.5, -1e-3, 0.0, 0.999, 1.0, 1.004, 1.5, 300.0, float("inf"), float("-inf"), float("nan"), 0.5]).reshape(1, 1, 1, 2, 6)
    got = emu_img.video_grid_u8(v).reshape(12, 3)
    assert got[:, 0].tolist() == [0, 0, 0, 254, 255, 255, 255, 255, 255, 0, 0, 127] and torch.equal(got[:, 0], got[:, 2])
    got = emu_img.video_grid_u8(torch.tensor([-3.0, -1.0, 0.0, 1.0, 3.0, 0.5]).reshape(1, 1, 1, 1, 6), rescale=True).reshape(6, 3)
    assert got[:, 1].tolist() == [0, 0, 127, 255, 255, 191]


# ------------------------------------------------------------------ VideoDataset
def _dataset(root, **kw):
    from motioneditor_amd.data.dataset import VideoDataset
    args = dict(width=32, height=24, n_sample_frames=4, condition=["openposefull"], video_suffix=".png", source_mask_dir="man.mask", device="cpu")
    args.update(kw)
    return VideoDataset(str(root), "a girl is dancing", **args)


def _interp(a, size, mode):
    x = torch.from_numpy(a).float()
    x = x.permute(0, 3, 1, 2) if x.dim() == 4 else x[:, None]
    return F.interpolate(x, size=size, mode=mode)


def test_dataset_returns_the_reference_keys_shapes_and_values(tmp_path, emulated):
    clip = write_clip(tmp_path)
    before = tree_digest(tmp_path)
    ds = _dataset(tmp_path, sample_start_idx=1, sample_frame_rate=2)
    assert len(ds) == 1 and ds.video_length == 10 and ds.frame_list == clip["names"]
    ex = ds[0]
    assert set(ex) == {"pixel_values", "source_conditions", "target_conditions", "prompt_ids", "source_masks", "sample_indices", "prompt", "train_prompt"}
    idx = [1, 3, 5, 7]
    assert ex["sample_indices"].dtype == torch.int64 and ex["sample_indices"].tolist() == idx
    assert ex["prompt"] == "a girl is dancing" and ex["prompt_ids"] is None and ex["train_prompt"] == "openpose"
    pv, sm = ex["pixel_values"], ex["source_masks"]
    assert pv.dtype == torch.float32 and tuple(pv.shape) == (4, 3, 24, 32) and -1.0 <= float(pv.min()) and float(pv.max()) <= 1.0
    assert sm.dtype == torch.float32 and tuple(sm.shape) == (4, 1, 24, 32) and set(sm.unique().tolist()) == {0.0, 1.0}
    assert list(ex["source_conditions"]) == ["openposefull"] and list(ex["target_conditions"]) == ["openposefull"]
    # the reference arithmetic on the decoded arrays (PNG is lossless: the decoded arrays are the written ones)
    want = _interp(clip["images"][idx], (24, 32), "bilinear")
    err = float((pv - (want / 127.5 - 1.0)).abs().max())
    print(f"pixel_values: max |dataset - reference arithmetic| = {err:.3e} (bound {BILINEAR_ATOL / 127.5 + 2 ** -22:.3e})")
    assert err <= BILINEAR_ATOL / 127.5 + 2 ** -22             # the 16-ulp(256) bound through / 127.5, plus two roundings of a quotient below 2 (2 x 2^-24) and of the difference on either side
    for key, arr in (("source_conditions", clip["source"]), ("target_conditions", clip["target"])):
        c = ex[key]["openposefull"]
        assert c.dtype == torch.float32 and tuple(c.shape) == (4, 3, 24, 32) and 0.0 <= float(c.min()) and float(c.max()) <= 1.0
        assert float((c - _interp(arr[idx], (24, 32), "bilinear") / 255).abs().max()) <= BILINEAR_ATOL / 255 + 2 ** -24
    assert torch.equal(sm, _interp(clip["masks"][idx].astype(np.float32) / 255, (24, 32), "nearest"))
    assert tree_digest(tmp_path) == before                    # nothing written into the data folder


def test_dataset_sampling_arguments_and_defaults(tmp_path, emulated):
    import inspect
    from motioneditor_amd.data.dataset import VideoDataset
    clip = write_clip(tmp_path, frame_list=False)
    p = inspect.signature(VideoDataset.__init__).parameters
    assert [(k, p[k].default) for k in ("width", "height", "n_sample_frames", "sample_start_idx", "sample_frame_rate", "condition", "video_suffix",
                                        "condition_suffix", "random_sample", "source_mask_dir", "train_prompt", "device")] == [
        ("width", 512), ("height", 512), ("n_sample_frames", 8), ("sample_start_idx", 0), ("sample_frame_rate", 1), ("condition", "openpose"),
        ("video_suffix", ".jpg"), ("condition_suffix", ".png"), ("random_sample", False), ("source_mask_dir", None), ("train_prompt", "openpose"), ("device", "cuda")]
    assert p["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    before = tree_digest(tmp_path)
    ds = _dataset(tmp_path, source_mask_dir=None, n_sample_frames=3, sample_start_idx=4, condition="openposefull", some_key_of_the_yaml=1)
    assert ds.frame_list == clip["names"]                    # no frame_list.txt: the sorted stems of images/*
    ex = ds[0]
    assert ex["sample_indices"].tolist() == [4, 5, 6] and list(ex["source_conditions"]) == ["openposefull"]
    assert tuple(ex["source_masks"].shape) == (3, 1, 24, 32) and bool((ex["source_masks"] == 1).all())
    assert tree_digest(tmp_path) == before and not (tmp_path / "frame_list.txt").exists()
    full = _dataset(tmp_path, n_sample_frames=10)[0]
    assert full["sample_indices"].tolist() == list(range(10))
    assert torch.equal(full["pixel_values"][4:7], ex["pixel_values"])
    rs = _dataset(tmp_path, n_sample_frames=4, random_sample=True)
    for _ in range(5):
        i = rs[0]["sample_indices"].tolist()
        assert i == list(range(i[0], i[0] + 4)) and 0 <= i[0] <= 6
    with pytest.raises(NotImplementedError):
        ds.preprocess_img_embedding(None, None)


def test_dataset_errors_name_the_file_and_the_value(tmp_path, emulated):
    from PIL import Image
    write_clip(tmp_path)
    with pytest.raises(ValueError, match=r"lists 10 frames.*leaves 5 from sample_start_idx=0 at sample_frame_rate=2: fewer than n_sample_frames=6"):
        _dataset(tmp_path, n_sample_frames=6, sample_frame_rate=2)[0]
    with pytest.raises(FileNotFoundError, match=r"frame '0001' has no file .*images.0001\.jpg"):
        _dataset(tmp_path, video_suffix=".jpg")[0]
    (tmp_path / "target_condition" / "openposefull" / "0003.png").unlink()
    with pytest.raises(FileNotFoundError, match=r"target_condition.openposefull.0003\.png"):
        _dataset(tmp_path)[0]
    Image.fromarray(np.zeros((40, 60, 3), dtype=np.uint8)).save(tmp_path / "images" / "0002.png")
    with pytest.raises(ValueError, match=r"0002\.png is 60x40 \(width x height\), .*0001\.png is 56x40"):
        _dataset(tmp_path)[0]


def test_dataloader_batch_carries_the_shapes_inference_indexes(tmp_path, emulated):
    from torch.utils.data import DataLoader
    write_clip(tmp_path)
    ds = _dataset(tmp_path)
    ds.prompt_ids = torch.arange(77)                           # inference.py:143-146 sets the ids before the loader runs
    batch = next(iter(DataLoader(ds, batch_size=1)))
    assert tuple(batch["pixel_values"].shape) == (1, 4, 3, 24, 32)                     # :254, :260 video_length = pixel_values.shape[1]
    assert tuple(batch["source_conditions"]["openposefull"].shape) == (1, 4, 3, 24, 32)  # :267
    assert tuple(batch["target_conditions"]["openposefull"].shape) == (1, 4, 3, 24, 32)  # :268
    assert tuple(batch["source_masks"].shape) == (1, 4, 1, 24, 32)                     # :270
    assert tuple(batch["sample_indices"].shape) == (1, 4) and tuple(batch["prompt_ids"].shape) == (1, 77) and batch["prompt"] == ["a girl is dancing"]


# ------------------------------------------------------------------ the writers
def _video(b=2, c=3, f=5, h=10, w=14, seed=3):
    return torch.rand(b, c, f, h, w, generator=torch.Generator().manual_seed(seed))


def test_png_frames_round_trip_bitwise(tmp_path, emulated):
    from PIL import Image
    from motioneditor_amd import util
    v = _video()
    util.save_videos_as_images(v * 2 - 1, str(tmp_path), rescale=True)
    for b in range(2):
        want = util.videos_to_grid_frames(v[b:b + 1] * 2 - 1, rescale=True)
        assert want.dtype == torch.uint8 and tuple(want.shape) == (5, 10, 14, 3)
        for t in range(5):
            got = np.asarray(Image.open(tmp_path / "vis_images" / f"batch_{b}" / f"frame_{t}.png"))
            assert np.array_equal(got, want[t].numpy())
    assert sorted(p.name for p in (tmp_path / "vis_images").iterdir()) == ["batch_0", "batch_1"]


def test_gif_has_the_frames_the_size_and_the_timing(tmp_path, emulated, monkeypatch):
    """f frames of Wg x Hg, looping, 125 ms each.  125 ms is what the writer asks PIL for (checked on the call); a GIF stores delays in 1/100 s, so the file
    itself carries 12 units and reads back as 120 ms -- the same truncation the reference's `fps=8` meets in the format."""
    from PIL import Image
    from motioneditor_amd import util
    v = _video(b=5)
    frames = util.videos_to_grid_frames(v)
    assert tuple(frames.shape) == (5, 2 * 12 + 2, 4 * 16 + 2, 3) and np.array_equal(frames.numpy(), make_grid_numpy(v.numpy()))
    path = tmp_path / "sample" / "a boy is dancing.gif"
    asked, save = [], Image.Image.save

    def spy(self, fp, format=None, **params):
        asked.append(dict(params, format=format))
        return save(self, fp, format, **params)
    monkeypatch.setattr(Image.Image, "save", spy)
    util.save_videos_grid(v, str(path), fps=3)                 # fps does not reach the GIF (util.py:46 hard-codes 8)
    monkeypatch.setattr(Image.Image, "save", save)
    assert len(asked) == 1 and asked[0]["format"] == "GIF" and asked[0]["save_all"] is True and asked[0]["loop"] == 0 and asked[0]["duration"] == 125
    assert len(asked[0]["append_images"]) == 4
    with Image.open(path) as im:
        assert im.format == "GIF" and im.n_frames == 5 and im.size == (4 * 16 + 2, 2 * 12 + 2) and im.info.get("loop") == 0
        for t in range(5):
            im.seek(t)
            assert im.info["duration"] == 125 // 10 * 10
    assert not path.with_suffix(".mp4").exists()
    with pytest.raises(ValueError, match=r"\.mp4 needs imageio \+ ffmpeg"):
        util.save_videos_grid(v, str(tmp_path / "sample" / "x.mp4"))


def test_clip_io_refuses_to_run_inside_a_recorded_step(monkeypatch):
    from motioneditor_amd import ops, plan
    monkeypatch.setattr(plan, "ACTIVE", object())
    with pytest.raises(RuntimeError, match="do not belong in the step's plan"):
        ops.image_resize(images_u8(1, 4, 4, 3, seed=0), (4, 4))
    with pytest.raises(RuntimeError, match="do not belong in the step's plan"):
        ops.video_grid_u8(torch.zeros(1, 3, 1, 4, 4))


def test_wrappers_check_their_arguments_before_any_launch():
    from motioneditor_amd import ops
    with pytest.raises(ValueError, match="CUDA uint8"):
        ops.image_resize(images_u8(1, 4, 4, 3, seed=0), (4, 4))          # a CPU tensor: no fallback
    with pytest.raises(ValueError, match="mode must be"):
        ops.image_resize(images_u8(1, 4, 4, 3, seed=0), (4, 4), "area")
    with pytest.raises(ValueError, match="CUDA fp32"):
        ops.video_grid_u8(torch.zeros(1, 3, 1, 4, 4))
    assert ops.grid_size(1, 8, 9) == (8, 9) and ops.grid_size(5, 8, 9, 4) == (22, 46) and ops.grid_size(3, 8, 9, 2) == (22, 24)


# ------------------------------------------------------------------ the ABI table of include/motioned_io.h
def test_io_symbols_are_declared_exported_and_apart_from_the_step_abi():
    from motioneditor_amd import build, capi
    build.build_lib(verbose=False)
    assert "image.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA_FLAGS["image.hip"]
    assert not any("fast-math" in f for f in build.FLAGS + build.EXTRA_FLAGS["image.hip"])
    assert not set(capi.IO_SYMBOLS) & set(capi.SYMBOLS)
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "motioned_io.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(me_[a-z0-9_]+)\s*\(", header))
    assert declared == set(capi.IO_SYMBOLS) == {"me_image_resize", "me_video_grid_u8"}
    L = ctypes.CDLL(str(capi.LIB_PATH))
    for name in declared:
        getattr(L, name)
    bound = capi.lib()
    for name, (res, args) in capi.IO_SYMBOLS.items():
        assert getattr(bound, name).argtypes == args and getattr(bound, name).restype is res
    assert bound.me_abi_version() == capi.ABI_VERSION == 9
    step_header = (ROOT / "include" / "motioned.h").read_text()
    assert "me_image_resize" not in step_header and "me_video_grid_u8" not in step_header


def test_io_argument_validation_returns_einval_without_a_device():
    from motioneditor_amd import capi
    L = capi.lib()
    P = 4096            # never dereferenced: every call below is refused before a launch

    def resize(out=P, src=P, n=1, H=8, W=8, C=3, oh=4, ow=4, mode=capi.RESIZE_BILINEAR, div=1.0, s_row=None, o_row=None):
        s_row, o_row = W * C if s_row is None else s_row, ow if o_row is None else o_row
        return L.me_image_resize(out, C * oh * o_row, oh * o_row, o_row, src, H * s_row, s_row, n, H, W, C, oh, ow, mode, div, 0.0, None)

    def grid(out=P, vid=P, b=2, c=3, f=2, h=4, w=4, n_rows=4, o_row=None):
        Wg = w if b == 1 else (w + 2) * min(n_rows, b) + 2
        Hg = h if b == 1 else (h + 2) * -(-b // max(min(n_rows, b), 1)) + 2
        o_row = 3 * Wg if o_row is None else o_row
        return L.me_video_grid_u8(out, Hg * o_row, o_row, vid, c * f * h * w, f * h * w, h * w, w, b, c, f, h, w, n_rows, 0, None)

    for call, word in ((lambda: resize(out=None), b"null"), (lambda: resize(src=None), b"null"), (lambda: resize(C=2), b"C must be 1 or 3"),
                       (lambda: resize(oh=0), b"positive"), (lambda: resize(ow=0), b"positive"), (lambda: resize(mode=2), b"unknown mode"),
                       (lambda: resize(mode=-1), b"unknown mode"), (lambda: resize(s_row=23), b"strides"), (lambda: resize(o_row=3), b"strides"),
                       (lambda: resize(div=0.0), b"div"),
                       (lambda: grid(out=None), b"null"), (lambda: grid(vid=None), b"null"), (lambda: grid(c=2), b"c must be 1 or 3"),
                       (lambda: grid(h=0), b"positive"), (lambda: grid(f=0), b"positive"), (lambda: grid(n_rows=0), b"positive"),
                       (lambda: grid(o_row=3 * 14 - 1), b"strides")):
        assert call() == capi.ME_EINVAL and word in L.me_last_error(), L.me_last_error()
    with pytest.raises(ValueError, match="me_image_resize"):
        capi.check(resize(C=2), "me_image_resize")


def test_every_io_symbol_is_named_by_a_guard_case():
    """The rule of test_guard_cpu.py::test_every_abi_symbol_is_guarded_or_listed_with_a_reason for capi.IO_SYMBOLS; no exemptions -- both entries launch."""
    from motioneditor_amd import capi
    import test_guard_io_gpu
    guarded = set()
    for syms in test_guard_io_gpu.GUARDED.values():
        guarded |= set(syms)
    assert len(test_guard_io_gpu.GUARDED) > 0
    assert guarded <= set(capi.IO_SYMBOLS), f"guard cases name symbols the I/O table does not have: {sorted(guarded - set(capi.IO_SYMBOLS))}"
    assert not set(capi.IO_SYMBOLS) - guarded, f"I/O symbols without a guard case: {sorted(set(capi.IO_SYMBOLS) - guarded)}"


# ------------------------------------------------------------------ the example's flags
def test_run_edit_builds_its_batch_from_a_clip_folder(tmp_path, emulated):
    import run_edit
    write_clip(tmp_path / "case")
    a = run_edit.parser().parse_args(["--video-dir", str(tmp_path / "case"), "--mask-dir", "man.mask", "--frames", "4", "--size", "32", "--out", str(tmp_path / "out")])
    assert (a.condition, a.suffix, a.out) == ("openposefull", ".png", str(tmp_path / "out"))
    x = run_edit.clip_inputs(a, device="cpu")
    want = run_edit.harness_inputs(4, 32, 32)
    assert set(x) == set(want) and all(tuple(x[k].shape) == tuple(want[k].shape) and x[k].dtype == want[k].dtype for k in want)
    from motioneditor_amd.data.dataset import VideoDataset
    ex = VideoDataset(str(tmp_path / "case"), "", width=32, height=32, n_sample_frames=4, condition=["openposefull"], video_suffix=".png",
                      source_mask_dir="man.mask", device="cpu")[0]
    assert torch.equal(x["pixel_values"][0], ex["pixel_values"]) and torch.equal(x["target_skeleton"][0], ex["target_conditions"]["openposefull"])
    assert torch.equal(x["source_masks"][0], ex["source_masks"]) and set(x["source_masks"].unique().tolist()) == {0.0, 1.0}
    for k in ("text_embeddings", "negative_text_embeddings", "encode_noise"):
        assert torch.equal(x[k], want[k])
    d = run_edit.parser().parse_args([])                        # without the flags: the synthetic clip, as before
    assert d.video_dir is None and d.out is None and d.mask_dir is None and (d.frames, d.size) == (8, 128)
    v = torch.rand(1, 3, 4, 32, 32, generator=torch.Generator().manual_seed(1))
    paths = run_edit.save_samples(a.out, "a boy is dancing", v, 1 - v)
    assert paths == [f"{a.out}/sample/a boy is dancing.gif", f"{a.out}/sample/a boy is dancing-inv.gif"] and all(__import__("os").path.isfile(p) for p in paths)
