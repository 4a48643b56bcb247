"""Spatial guidance: the label maps behind ``--content-mask`` / ``--style-mask`` (Gatys et al. 2017, "Controlling perceptual
factors in neural style transfer", section 4.2, the guided Gram matrices; no counterpart in the reference).

A label map is a uint8 ``[H, W]`` tensor: every pixel carries one region index ``0..R-1`` or ``NO_REGION`` (255).  Guidance is
hard - a pixel belongs to at most one region.  Everything here is host work on small integer tensors, done once per run (or
per level of a coarse-to-fine run), never inside the step:

* :func:`quantize` turns the 8-bit grey levels of a mask file into ``R`` uniform bands;
* :func:`resample_labels` follows an image through a resize (nearest sampling in integer arithmetic), a plain slice through
  a crop;
* :func:`renumber` drops the regions whose weight is 0 (their pixels become ``NO_REGION``) and numbers the rest ``0..Ra-1``;
* :func:`tap_maps` / :func:`region_counts` give every style tap its map and the pixel counts ``n_{l,r}`` that norm its Grams.

The device work is ``stv_mask_split`` (``ops.mask_split``) and the guided step of ``core_model`` / ``plan``.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

NO_REGION = 255
MAX_REGIONS = 4           # stv.h STV_MASK_MAX_REGIONS
MAX_COMBINE_ROWS = 64     # stv_loss_combine: n_terms <= 64


@dataclass(frozen=True, eq=False)
class Guide:
    """What a guided engine is built from: the weights of the ACTIVE regions, their numbers in the masks, and the two
    renumbered label maps (host uint8, at the run size of the content image and at the style image's own size)."""

    weights: tuple[float, ...]
    active: tuple[int, ...]
    content_labels: torch.Tensor
    style_labels: torch.Tensor

    @property
    def n(self) -> int:
        return len(self.weights)

    def key(self) -> tuple:
        return ("guide", self.n, self.weights, self.content_labels.data_ptr(), self.style_labels.data_ptr())


def make_guide(regions: int, weights, content_labels, style_labels) -> Guide:
    """Checked labels, zero-weight regions dropped and the rest renumbered (refusals before anything is built)."""
    w = check_region_weights(weights, regions)
    active = active_regions(w)
    c = renumber(check_labels(content_labels, regions, "content_labels"), w)
    s = renumber(check_labels(style_labels, regions, "style_labels"), w)
    return Guide(tuple(w[r] for r in active), active, c, s)


def check_regions(regions, *, minimum: int = 1, what: str = "guide_regions") -> int:
    """The number of regions as an int in ``minimum..MAX_REGIONS`` (the model API takes 1, the CLI and TOML 2 and up)."""
    if isinstance(regions, bool) or not isinstance(regions, int) or not minimum <= regions <= MAX_REGIONS:
        msg = f"{what} must be an integer from {minimum} to {MAX_REGIONS}, got {regions!r}"
        raise ValueError(msg)
    return regions


def check_region_weights(weights, regions: int) -> tuple[float, ...]:
    """One weight ``lambda_r`` per region as floats (``None``: every region 1.0).  Refused: another length, a negative or
    non-finite weight, all weights zero."""
    if weights is None:
        return (1.0,) * regions
    try:
        out = tuple(float(w) for w in weights)
    except (TypeError, ValueError):
        msg = f"region_weights must be {regions} numbers, got {weights!r}"
        raise ValueError(msg) from None
    if len(out) != regions:
        msg = f"region_weights has {len(out)} entries for {regions} regions: {list(out)}"
        raise ValueError(msg)
    if any(not math.isfinite(w) or w < 0.0 for w in out):
        msg = f"region_weights must be finite and >= 0, got {list(out)}"
        raise ValueError(msg)
    if not any(w > 0.0 for w in out):
        msg = f"region_weights are all zero ({list(out)}): no region would be styled"
        raise ValueError(msg)
    return out


def active_regions(weights: tuple[float, ...]) -> tuple[int, ...]:
    """The indices of the regions with a weight > 0, ascending: region ``active[k]`` runs as region ``k``."""
    return tuple(r for r, w in enumerate(weights) if w > 0.0)


def quantize(grey, regions: int) -> torch.Tensor:
    """8-bit grey levels -> labels: level ``v`` becomes region ``min(R-1, v*R // 256)`` - ``R`` uniform bands, so black and
    white give two regions and a few levels of JPEG noise stay inside their band."""
    g = torch.from_numpy(np.array(grey)) if not isinstance(grey, torch.Tensor) else grey
    if g.dtype != torch.uint8 or g.dim() != 2:
        msg = f"a mask is an 8-bit grey image [H, W], got {tuple(g.shape)} {g.dtype}"
        raise ValueError(msg)
    return torch.clamp(g.to(torch.int32) * regions // 256, max=regions - 1).to(torch.uint8)


def check_labels(labels, regions: int, what: str = "labels") -> torch.Tensor:
    """``labels`` as a contiguous uint8 ``[H, W]`` host tensor whose values are ``< regions`` or ``NO_REGION``."""
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.uint8 or labels.dim() != 2:
        got = f"{tuple(labels.shape)} {labels.dtype}" if isinstance(labels, torch.Tensor) else type(labels).__name__
        msg = f"{what} must be a uint8 tensor [H, W], got {got}"
        raise ValueError(msg)
    out = labels.detach().cpu().contiguous()
    bad = out[(out >= regions) & (out != NO_REGION)]
    if bad.numel():
        msg = f"{what} hold region {int(bad[0])}, but there are {regions} regions (0..{regions - 1}, or {NO_REGION} for none)"
        raise ValueError(msg)
    return out


def resample_labels(labels: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """``labels`` ``[H0, W0]`` at ``[H, W]`` by nearest sampling in integer arithmetic: output row ``y`` reads source row
    ``((2*y + 1) * H0) // (2*H)``, and the same along x (the source pixel under the output pixel's centre)."""
    H0, W0 = (int(v) for v in labels.shape)
    if H < 1 or W < 1:
        msg = f"cannot resample a label map to {H}x{W}"
        raise ValueError(msg)
    if (H0, W0) == (H, W):
        return labels
    ys = ((2 * torch.arange(H, dtype=torch.int64) + 1) * H0) // (2 * H)
    xs = ((2 * torch.arange(W, dtype=torch.int64) + 1) * W0) // (2 * W)
    return labels[ys][:, xs].contiguous()


def renumber(labels: torch.Tensor, weights: tuple[float, ...]) -> torch.Tensor:
    """``labels`` with the regions of weight 0 dropped: their pixels get ``NO_REGION``, the active regions are renumbered
    ``0..Ra-1`` in ascending order.  All weights > 0: the map itself."""
    active = active_regions(weights)
    if len(active) == len(weights):
        return labels
    lut = torch.full((256,), NO_REGION, dtype=torch.uint8)
    for k, r in enumerate(active):
        lut[r] = k
    return lut[labels.to(torch.int64)]


def tap_shapes(H: int, W: int, layers, style_at) -> list[tuple[int, int]]:
    """``(H_l, W_l)`` of every style tap of a feature stack in ascending layer order (a pooling layer halves, rounding down).
    ``layers``: the modules of the stack, or a VGG cfg tuple (``synthetic.VGG19_CFG``: a number is a conv and its ReLU, "M" a
    pool)."""
    from torch import nn  # noqa: PLC0415
    if isinstance(layers, tuple):
        pools = [p for v in layers for p in ((True,) if v == "M" else (False, False))]
    else:
        pools = [isinstance(layer, (nn.MaxPool2d, nn.AvgPool2d)) for layer in layers]
    out, want = [], sorted(set(style_at))
    for i, is_pool in enumerate(pools):
        if is_pool:
            H, W = H // 2, W // 2
        if i in want:
            out.append((H, W))
    return out


def check_maps(guide: Guide, layers, style_at) -> None:
    """Both maps of ``guide`` against every style tap of the stack: an active region without a pixel at a tap is refused
    (:func:`check_counts`) - host arithmetic on the label maps alone, before anything is built or launched."""
    names = sorted(set(style_at))
    for which, labels in (("content", guide.content_labels), ("style", guide.style_labels)):
        shapes = tap_shapes(int(labels.shape[0]), int(labels.shape[1]), layers, style_at)
        check_counts(tap_maps(labels, shapes), guide.n, which, guide.active, names)


def tap_maps(labels: torch.Tensor, shapes: list[tuple[int, int]]) -> list[torch.Tensor]:
    """The map of every style tap: the run-size map resampled to the tap's ``(H_l, W_l)``."""
    return [resample_labels(labels, h, w) for h, w in shapes]


def region_counts(labels: torch.Tensor, regions: int) -> list[int]:
    """``n_r = #{p : labels[p] == r}`` for ``r < regions``."""
    return [int(v) for v in torch.bincount(labels.reshape(-1).to(torch.int64), minlength=256)[:regions]]


def check_counts(maps: list[torch.Tensor], n_active: int, which: str, active: tuple[int, ...] | None = None,
                 layer_names: list | None = None) -> list[list[int]]:
    """The pixel counts ``n_{l,r}`` of every style tap; an active region without a pixel at a tap is refused, with the
    region (its number in the mask), the layer and the map (``which``: "content" or "style") named."""
    counts = []
    for l, m in enumerate(maps):
        row = region_counts(m, n_active)
        for k, n in enumerate(row):
            if n == 0:
                region = active[k] if active is not None else k
                layer = layer_names[l] if layer_names is not None else l
                msg = (f"region {region} of the {which} mask has no pixel at style layer {layer} "
                       f"({m.shape[0]}x{m.shape[1]} feature map): its guided Gram matrix is undefined "
                       "(enlarge the region, drop the deep style layers, or give the region weight 0)")
                raise ValueError(msg)
        counts.append(row)
    return counts


def check_rows(n_style_layers: int, n_active: int, n_other: int) -> None:
    """The combine kernel takes ``MAX_COMBINE_ROWS`` rows: one per (style layer, active region) plus the other terms."""
    rows = n_style_layers * n_active + n_other
    if rows > MAX_COMBINE_ROWS:
        msg = (f"{n_style_layers} style layers x {n_active} regions + {n_other} other terms = {rows} combine rows, "
               f"more than the {MAX_COMBINE_ROWS} the combine kernel takes")
        raise ValueError(msg)


def load_mask(path: str, image_hw: tuple[int, int], regions: int, which: str) -> torch.Tensor:
    """The label map of a mask file, read as 8-bit grey.  The mask must have the pixel size of its image file."""
    from PIL import Image  # noqa: PLC0415
    with Image.open(path) as img:
        grey = np.asarray(img.convert("L"))
    H, W = (int(v) for v in image_hw)
    if grey.shape != (H, W):
        msg = (f"the {which} mask {path} is {grey.shape[1]}x{grey.shape[0]} pixels, its image is {W}x{H}: "
               "a mask must have the size of its image file")
        raise ValueError(msg)
    return quantize(grey, regions)
