"""Image output (reference src/misc/image_io.py: prep_image :38-54, save_image :57-68).

prep_image runs on the image's device: the clip, the fp32 multiply by 255, the truncation to uint8
and the CHW -> HWC layout are one launch of tsplat_video_frames_fwd (the video path's kernel without
a depth input). It returns a uint8 tensor on that device; the reference returns a numpy array."""
from __future__ import annotations

from pathlib import Path
from typing import Union

import torch
from torch import Tensor

from .. import kernels


def prep_image(image: Tensor) -> Tensor:
    """[H, W], [C, H, W] (C = 1 or 3) or [B, 3, H, W] float image in 0..1 -> uint8 [H, W', 3] on the
    image's device (a batch is laid side by side, a single channel repeated), uint8(clip * 255)."""
    if image.ndim == 4:
        image = image.permute(1, 2, 0, 3).reshape(image.shape[1], image.shape[2], -1)
    if image.ndim == 2:
        image = image[None]
    if image.shape[0] == 1:
        image = image.expand(3, -1, -1)
    if image.ndim != 3 or image.shape[0] != 3:
        raise ValueError(f"prep_image: expected 1 or 3 channels, got {tuple(image.shape)}")
    return kernels.video_frames(image.detach()[None])[0]


def save_image(image: Tensor, path: Union[Path, str]) -> None:
    """Save a 0..1 float image (or an already prepared uint8 HWC one) as a PNG; the parent directory
    is made if it is missing."""
    from PIL import Image

    path = Path(path)
    path.parent.mkdir(exist_ok=True, parents=True)
    frame = image if image.dtype == torch.uint8 else prep_image(image)
    Image.fromarray(frame.cpu().numpy()).save(path)
