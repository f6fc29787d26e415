"""`VideoDataset` of the reference (`motion_editor/data/dataset.py`): one clip as a folder of frames, masks and condition images.

    data/case-1/images/0001.jpg ...                              the frames                         (video_suffix)
    data/case-1/source_condition/openposefull/0001.png ...       skeletons of the source motion     (condition_suffix)
    data/case-1/target_condition/openposefull/0001.png ...       skeletons of the target motion
    data/case-1/man.mask/0001.png ...                            foreground masks, 0 / 255          (source_mask_dir, always .png)
    data/case-1/frame_list.txt                                   frame names, one per line          (optional)

Same constructor arguments, defaults, keys, shapes, dtypes and value ranges as the reference class, so `VideoDataset(**input_data)` of
inference.py:141 and `torch.utils.data.DataLoader(ds, batch_size=1)` work unchanged.  What differs:

  * Files are decoded with PIL (frames and conditions `.convert("RGB")`, masks `.convert("L")`); the reference's decord / imageio / cv2 are not needed.
  * The decoded frames of a tensor are stacked into ONE uint8 array, uploaded once, and resized, converted to fp32 NCHW and scaled by one
    `me_image_resize` launch per tensor (ops.image_resize, csrc/image.hip) -- the reference's F.interpolate and `/ 127.5 - 1.0`, `/ 255`.  The
    returned tensors live on `device` (the one extra keyword, default "cuda"); the inputs never exist as fp32 on the host.
  * The reference writes `frame_list.txt` into the data folder when it is missing.  This class never writes into its input directory: without
    the file, the frame list is the sorted stems of `images/*`, every time.
  * A missing file, frames of unequal size and a clip with fewer frames than `n_sample_frames` raise errors that name the file and the value
    (the reference fails inside numpy / returns a short clip).
  * `preprocess_img_embedding` takes this package's `models.clip.CLIPImageProcessor` and `CLIPVisionModelWithProjection`; called without them it raises
    NotImplementedError, as it did before the package had an image encoder.
"""
from __future__ import annotations

import os.path as osp
import random
from glob import glob
from typing import Dict, List, Optional, Union

import numpy as np
import torch
from torch.utils.data import Dataset

from .. import ops


class VideoDataset(Dataset):
    def __init__(
            self,
            video_dir: str,
            prompt: str,
            width: int = 512,
            height: int = 512,
            n_sample_frames: int = 8,
            sample_start_idx: int = 0,
            sample_frame_rate: int = 1,
            condition: Union[str, List[str]] = 'openpose',
            video_suffix: str = '.jpg',
            condition_suffix: str = '.png',
            random_sample: bool = False,
            source_mask_dir: Optional[str] = None,
            train_prompt: Union[str, List[str]] = 'openpose',
            device: str = "cuda",
            **kwargs,
    ):
        self.video_dir = video_dir
        self.video_path = osp.join(self.video_dir, 'images')
        if isinstance(condition, str):
            condition = [condition]
        self.condition = list(condition)
        self.source_condition_path = {c: osp.join(self.video_dir, "source_condition", c) for c in self.condition}
        self.target_condition_path = {c: osp.join(self.video_dir, "target_condition", c) for c in self.condition}
        self.video_suffix = video_suffix
        self.condition_suffix = condition_suffix
        self.random_sample = random_sample
        self.source_mask_dir = osp.join(self.video_dir, source_mask_dir) if source_mask_dir else None

        frame_list_path = osp.join(self.video_dir, 'frame_list.txt')
        if osp.isfile(frame_list_path):
            with open(frame_list_path, 'r') as f:
                self.frame_list = f.read().splitlines()
        else:   # (dataset.py:51-58 also writes the file; the input directory stays as it is here)
            self.frame_list = [osp.basename(p).split('.')[0] for p in sorted(glob(osp.join(self.video_path, '*')))]
        self.video_length = len(self.frame_list)
        self.prompt = prompt
        self.prompt_ids = None
        self.width = width
        self.height = height
        self.n_sample_frames = n_sample_frames
        self.sample_start_idx = sample_start_idx
        self.sample_frame_rate = sample_frame_rate
        self.source_img_embeddings = []
        self.train_prompt = train_prompt
        self.device = device

    @torch.no_grad()
    def preprocess_img_embedding(self, feature_extractor, image_encoder):
        """dataset.py:76-82: one CLIP image embedding [projection_dim] per frame of the folder, appended to `source_img_embeddings`.  The frames are decoded
        with PIL (the reference's imageio gives the same RGB bytes) and go through processor and encoder -- this package's (models.clip) -- as one batch;
        the encoder is batch-invariant bit for bit, so each row is what a call per frame gives.  Like __getitem__ it wants the frames of one size."""
        if feature_extractor is None or image_encoder is None:
            raise NotImplementedError("VideoDataset.preprocess_img_embedding: motioneditor_amd has no CLIP image encoder (dataset.py:76-82 is not built)")
        frames = self._decode(self.video_path, self.frame_list, self.video_suffix, "RGB")         # uint8 [f, H, W, 3]: the whole folder in one batch
        embeds = image_encoder(feature_extractor(frames).pixel_values).image_embeds              # fp32 [f, projection_dim]
        self.source_img_embeddings.extend(embeds.unbind(0))

    def __len__(self):
        return 1

    def _decode(self, folder: str, names: List[str], suffix: str, pil_mode: str) -> torch.Tensor:
        """The named files of one folder as ONE uint8 tensor [f, H, W, 3] ("RGB") or [f, H, W] ("L") on the host."""
        from PIL import Image
        frames, first = [], None
        for name in names:
            path = osp.join(folder, name + suffix)
            if not osp.isfile(path):
                raise FileNotFoundError(f"VideoDataset: frame '{name}' has no file {path}")
            with Image.open(path) as im:
                a = np.asarray(im.convert(pil_mode))
            if first is None:
                first = (path, a.shape[:2])
            elif a.shape[:2] != first[1]:
                raise ValueError(f"VideoDataset: {path} is {a.shape[1]}x{a.shape[0]} (width x height), {first[0]} is {first[1][1]}x{first[1][0]}: "
                                 "the images of one folder must have one size")
            frames.append(a)
        return torch.from_numpy(np.stack(frames, axis=0))

    def _load(self, folder: str, names: List[str], suffix: str, pil_mode: str, mode: str, div: float, add: float) -> torch.Tensor:
        """decode -> one upload of uint8 -> one me_image_resize launch: fp32 [f, C, height, width] on the device."""
        return ops.image_resize(self._decode(folder, names, suffix, pil_mode).to(self.device), (self.height, self.width), mode, div=div, add=add)

    def __getitem__(self, index) -> Dict[str, object]:
        video_indices = list(range(self.sample_start_idx, self.video_length, self.sample_frame_rate))
        if len(video_indices) < self.n_sample_frames:
            raise ValueError(f"VideoDataset: {self.video_dir} lists {self.video_length} frames, which leaves {len(video_indices)} from sample_start_idx="
                             f"{self.sample_start_idx} at sample_frame_rate={self.sample_frame_rate}: fewer than n_sample_frames={self.n_sample_frames}")
        start_index = random.randint(0, len(video_indices) - self.n_sample_frames) if self.random_sample else 0   # [a, b] includes both
        sample_index = video_indices[start_index:start_index + self.n_sample_frames]
        names = [self.frame_list[i] for i in sample_index]

        video = self._load(self.video_path, names, self.video_suffix, "RGB", "bilinear", 127.5, -1.0)                 # video / 127.5 - 1.0  (:121-123, :144)
        source_conditions = {c: self._load(p, names, self.condition_suffix, "RGB", "bilinear", 255.0, 0.0)            # condition / 255      (:126-130)
                             for c, p in self.source_condition_path.items()}
        target_conditions = {c: self._load(p, names, self.condition_suffix, "RGB", "bilinear", 255.0, 0.0)            # (:133-137)
                             for c, p in self.target_condition_path.items()}
        if self.source_mask_dir:   # mask / 255, nearest (:104-105, :139-141; dividing the picked value is dividing first and picking then)
            source_mask = self._load(self.source_mask_dir, names, '.png', "L", "nearest", 255.0, 0.0)
        else:                      # np.ones(frame.shape[:2]) resized by nearest: ones (:107)
            source_mask = torch.ones((len(names), 1, self.height, self.width), dtype=torch.float32, device=self.device)

        return {
            "pixel_values": video,
            "source_conditions": source_conditions,
            "target_conditions": target_conditions,
            "prompt_ids": self.prompt_ids,
            "source_masks": source_mask,
            "sample_indices": torch.LongTensor(sample_index),
            "prompt": self.prompt,
            "train_prompt": self.train_prompt,
        }
