"""Shared type aliases and small records."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Literal

import torch

InitMethod = Literal["content", "random", "white"]
VideoMode = Literal["realtime", "postprocess"]
Precision = Literal["fp32", "bf16", "bf16x3"]
PreserveColor = Literal["off", "match", "luma"]
ResizeFilter = Literal["bilinear", "bicubic", "lanczos"]
Pooling = Literal["max", "avg"]
AutoMaskSpace = Literal["color", "features"]
GifDither = Literal["none", "ordered"]
VideoFormat = Literal["mp4", "mjpeg"]
LossHistory = dict[str, list[float]]
TensorList = list[torch.Tensor]


@dataclass(slots=True)
class InputPaths:
    """Content and style image paths; ``extra_style_paths``: further style images, blended with the first (``style_mix.py``);
    ``content_mask_path`` / ``style_mask_path``: the two masks of a guided run (``guidance.py``), both or neither."""

    content_path: str
    style_path: str
    extra_style_paths: tuple[str, ...] = ()
    content_mask_path: str | None = None
    style_mask_path: str | None = None

    @property
    def style_paths(self) -> tuple[str, ...]:
        """Every style image, ``style_path`` first."""
        return (self.style_path, *self.extra_style_paths)


@dataclass(slots=True)
class SaveOptions:
    """What the final save step should write and how to name it."""

    content_name: str
    style_name: str
    video_name: str | None = None
    gif_name: str | None = None
    normalize: bool = True
    video_created: bool = True
    gif_created: bool = False
    plot_losses: bool = True
