"""Inputs of the feature-space automatic-mask tests: the stripes pair - two images of one colour distribution that differ only
in the direction of their texture, so that the colour k-means cannot split them and the feature k-means can - and VGG features
of a host image from CPU torch convolutions of the synthetic weights."""
from __future__ import annotations

import numpy as np
import torch
from PIL import Image

from style_transfer_visualizer_amd import core_model, image_io, synthetic

LAYER = 10                    # conv3_1: 256 channels, a quarter-size grid
DIFFER_CAP = 16               # cells of 256 per image that may differ from the exact halves (the float64 run differs in 9)


def stripes_pair(size: int = 64) -> tuple[np.ndarray, np.ndarray]:
    """``(content, style)`` uint8 ``[size, size, 3]``.  Base pattern ``a``: stripes of period 4, two pixels at 64 and two at
    192; vertical stripes vary with x, horizontal ones with y; ``R = a, G = 0.9a + 10, B = 0.8a + 30`` truncated.  Content:
    vertical stripes for ``x < size/2``, horizontal elsewhere.  Style: vertical stripes for ``y < size/2``, horizontal
    elsewhere."""
    yy, xx = np.mgrid[0:size, 0:size]
    vertical = np.where(xx % 4 < 2, 64.0, 192.0)
    horizontal = np.where(yy % 4 < 2, 64.0, 192.0)

    def rgb(a):
        return np.stack([a, 0.9 * a + 10.0, 0.8 * a + 30.0], axis=-1).astype(np.uint8)
    content = rgb(np.where(xx < size // 2, vertical, horizontal))
    style = rgb(np.where(yy < size // 2, vertical, horizontal))
    return content, style


def write_stripes(tmp_path, size: int = 64) -> tuple[str, str]:
    """The pair as ``content.png`` / ``style.png`` under ``tmp_path``; their paths."""
    paths = []
    for name, arr in zip(("content", "style"), stripes_pair(size), strict=True):
        paths.append(str(tmp_path / f"{name}.png"))
        Image.fromarray(arr).save(paths[-1])
    return paths[0], paths[1]


def stripes_tensors(size: int = 64, device="cpu") -> tuple[torch.Tensor, torch.Tensor]:
    """The pair as the run sees it: ``[1, 3, size, size]`` fp32, ImageNet-normalised."""
    content, style = (image_io.apply_transforms(Image.fromarray(arr), torch.device(device), normalize=True)
                      for arr in stripes_pair(size))
    return content, style


def half_grids(side: int) -> tuple[torch.Tensor, torch.Tensor]:
    """The exact halves on a ``side x side`` grid, region 0 the vertical stripes: content ``x < side/2``, style ``y < side/2``."""
    yy, xx = np.mgrid[0:side, 0:side]
    return (torch.from_numpy((xx >= side // 2).astype(np.uint8)), torch.from_numpy((yy >= side // 2).astype(np.uint8)))


def cpu_features(img: torch.Tensor, layer: int = LAYER, seed: int = 0) -> torch.Tensor:
    """The output of VGG index ``layer`` for a host image ``[1, 3, H, W]`` under ``synthetic_conv_weights(seed)``, NHWC
    ``[H_l, W_l, C]`` fp32, by torch's CPU convolutions."""
    state = torch.get_rng_state()
    vgg = core_model.build_vgg_features(synthetic.synthetic_conv_weights(seed)).eval()
    torch.set_rng_state(state)
    x = img.detach().float().cpu()
    with torch.no_grad():
        for module in list(vgg.children())[:layer + 1]:
            x = module(x)
    return x[0].permute(1, 2, 0).contiguous()


def cpu_extract(content, style, layer, oc, precision):      # noqa: ARG001
    """``segment.run_features`` on the host (``extract=``)."""
    return [cpu_features(content, layer), cpu_features(style, layer)]
