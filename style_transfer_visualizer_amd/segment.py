"""Automatic masks (``optimization.auto_mask``): the two label maps of a guided run from the two pictures themselves, by a
joint colour k-means (no counterpart in the reference; the front end of ``guidance.py``).

Content and style image are segmented TOGETHER into ``R`` colour regions, so region ``r`` of one picture corresponds to region
``r`` of the other by construction.  The images are the tensors the run sees - fp32 ``[3][H][W]`` behind the resize stage and
behind ``preserve_color = match`` (which moves the style's colours onto the content's and so helps the correspondence), in
whatever space they are in.  With ``s`` the cell size (``auto_mask_cell``)::

    P_i      = the s x s box means of image i (i = content, style), [3][H_i//s][W_i//s]              (ops.lap_pool)
    n_i      = number of cells of P_i; every sum over an image is divided by n_i: each image weighs 1/2 whatever its size
    mu       = (mean(P_c) + mean(P_s)) / 2
    Sigma    = (E_c[x x^T] + E_s[x x^T]) / 2 - mu mu^T        (raw moments: ops.color_stats on P_i; float64 on the host)
    v, lam   = principal eigenvector / eigenvalue of Sigma (numpy eigh)
               sign of v: v.(1,1,1) >= 0; if that is 0, the first non-zero component is positive
    c_k(0)   = fp32(mu + sqrt(max(lam, 0)) * z_k * v),  z_k = -1 + (2k+1)/R,  k = 0..R-1    (region 0: the dark end, as a rule)

    iteration t (at most MAX_ITER):
      label(p)  = argmin_k d_k(p),  d_k = ((e0*e0 + e1*e1) + e2*e2),  e_j = x_j(p) - c_k[j]
                  every product, sum and difference rounded to fp32 on its own; a strict `<` in ascending k: the lowest
                  index wins a tie                                                              (ops.kmeans_assign)
      S_k^i, N_k^i = sum of x and number of cells of image i with label k   (double)
      changed^i = cells of image i whose label differs from the previous iteration's   (first iteration: all)
      c_k(t)    = fp32((S_k^c/n_c + S_k^s/n_s) / (N_k^c/n_c + N_k^s/n_s))
                  float64 on the host; a cluster without cells in both images keeps its centroid
      stop when changed^c + changed^s == 0

The cell labels become the image's label map through ``guidance.resample_labels``; from there they are ordinary
``content_labels`` / ``style_labels``.  Inputs are taken as finite.

A segmentation is accepted (:func:`auto_guidance`) if every region holds at least ``1 / MIN_SHARE_DIV`` of the cells of each
pooled map and at least one pixel in every style tap's label map of both images, at every level of a coarse-to-fine run - the
condition the guided model enforces.  Otherwise everything is run again with ``R - 1``; at ``R == 1`` the run is unguided.

The pooling, the moments and the assignment are HIP kernels; the 3x3 algebra and the centroid update are NumPy float64 on the
host, with one readback of the two images' partial sums per iteration.

Not built: clustering in VGG feature space, spatial coordinates in the feature vector, per-region weights (the numbers of the
regions are not known in advance), several style images, row strips (``spatial.py``).
"""
from __future__ import annotations

import math
from pathlib import Path

import numpy as np
import torch

from . import _lib, color, guidance, ops
from .logging_utils import logger

CELLS = (1, 2, 4, 8, 16, 32)      # the pool sizes stv_lap takes (_lib.LAP_POOLS)
DEFAULT_CELL = 8
MAX_ITER = 20
MIN_SHARE_DIV = 64                # a region holds at least 1/64 of the cells of each pooled map: a design constant
MIN_CELLS_SIDE = 8                # the shorter side of either pooled map
_IMAGES = ("content", "style")


def check_cell(cell) -> int:
    """The cell size as an int out of :data:`CELLS`."""
    if isinstance(cell, bool) or not isinstance(cell, int) or cell not in CELLS:
        msg = f"auto_mask_cell must be one of {list(CELLS)}, got {cell!r}"
        raise ValueError(msg)
    return cell


def check_options(paths, oc) -> bool:
    """Whether the run asks for automatic masks; every refusal that needs no image comes from here (before the first launch):
    the option together with mask files, with several style images or with region weights, a cell size outside the set."""
    if not getattr(oc, "auto_mask", False):
        return False
    content_mask, style_mask = getattr(paths, "content_mask_path", None), getattr(paths, "style_mask_path", None)
    if content_mask or style_mask:
        msg = (f"--auto-mask cannot be combined with --content-mask / --style-mask (got content mask {content_mask!r} and "
               f"style mask {style_mask!r}): the masks come either from files or from the images")
        raise ValueError(msg)
    extra = tuple(getattr(paths, "extra_style_paths", ()))
    if extra:
        msg = (f"--auto-mask cannot be combined with --style-also ({len(extra)} further style images): masks with several "
               "style images are not built")
        raise ValueError(msg)
    weights = getattr(oc, "region_weights", None)
    if weights is not None:
        msg = (f"--auto-mask cannot be combined with --region-weights ({list(weights)}): which region gets which number is "
               "not known in advance (save the masks with --save-masks and give them back as files)")
        raise ValueError(msg)
    guidance.check_regions(getattr(oc, "mask_regions", 2), minimum=2, what="mask_regions")
    check_cell(getattr(oc, "auto_mask_cell", DEFAULT_CELL))
    return True


def check_sizes(content_hw, style_hw, cell: int) -> None:
    """Either image at run size gives a pooled map whose shorter side has at least ``MIN_CELLS_SIDE`` cells."""
    (Hc, Wc), (Hs, Ws) = ((int(v) for v in hw) for hw in (content_hw, style_hw))
    if min(Hc, Wc) // cell < MIN_CELLS_SIDE or min(Hs, Ws) // cell < MIN_CELLS_SIDE:
        msg = (f"--auto-mask: cells of {cell} pixels leave {Wc // cell}x{Hc // cell} cells of the {Wc}x{Hc} content image and "
               f"{Ws // cell}x{Hs // cell} of the {Ws}x{Hs} style image; the shorter side needs at least {MIN_CELLS_SIDE} "
               "(use a smaller --auto-mask-cell or larger images)")
        raise ValueError(msg)


def pool_cells(img: torch.Tensor, cell: int) -> torch.Tensor:
    """``P``: the ``cell x cell`` box means of a device image ``[3, H, W]`` or ``[1, 3, H, W]``, fp32 ``[3, H//cell, W//cell]``."""
    x = img.detach().contiguous()
    out = torch.empty(3, int(x.shape[-2]) // cell, int(x.shape[-1]) // cell, dtype=torch.float32, device=x.device)
    ops.lap_pool(x, out, cell)
    return out


def principal_axis(cov: np.ndarray) -> tuple[np.ndarray, float]:
    """``(v, lam)``: the principal eigenvector and eigenvalue of a symmetric 3x3 matrix, ``v`` signed so that ``v.(1,1,1)``
    is >= 0 and, where that is 0, its first non-zero component is positive."""
    lam, vec = np.linalg.eigh(np.asarray(cov, dtype=np.float64))
    v = vec[:, -1].copy()
    along = float(v.sum())
    if along == 0.0:
        nonzero = v[v != 0.0]
        along = float(nonzero[0]) if nonzero.size else 1.0
    return (-v if along < 0.0 else v), float(lam[-1])


def initial_centroids(stats, regions: int) -> np.ndarray:
    """``c_k(0)`` as fp32 ``[R, 3]`` from the two pooled maps' ``color.statistics`` (each image weighs 1/2)."""
    means = [np.asarray(sums, dtype=np.float64) / n for n, sums, _ in stats]
    seconds = [np.asarray(moments, dtype=np.float64) / n for n, _, moments in stats]
    mu = (means[0] + means[1]) / 2.0
    v, lam = principal_axis((seconds[0] + seconds[1]) / 2.0 - np.outer(mu, mu))
    z = -1.0 + (2.0 * np.arange(regions, dtype=np.float64) + 1.0) / regions
    return (mu[None, :] + math.sqrt(max(lam, 0.0)) * z[:, None] * v[None, :]).astype(np.float32)


def update_centroids(centroids: np.ndarray, sums: np.ndarray, counts: np.ndarray, cells) -> np.ndarray:
    """``c_k(t)`` from the two images' ``sums[i][k][3]`` and ``counts[i][k]`` (float64) and cell numbers ``cells[i]``."""
    out = centroids.copy()
    for k in range(centroids.shape[0]):
        weight = counts[0][k] / cells[0] + counts[1][k] / cells[1]
        if weight > 0.0:
            out[k] = ((sums[0][k] / cells[0] + sums[1][k] / cells[1]) / weight).astype(np.float32)
    return out


def auto_labels(content: torch.Tensor, style: torch.Tensor, regions: int, *, cell: int = DEFAULT_CELL, max_iter: int = MAX_ITER,  # noqa: PLR0913
                assign=ops.kmeans_assign, pool=pool_cells, moments=color.statistics) -> tuple[torch.Tensor, torch.Tensor, dict]:
    """One joint segmentation of the two images into ``regions`` regions (module docstring): the label maps of the content
    and of the style image (host uint8, at the images' sizes) and ``info`` - ``regions``, ``iterations``, ``converged``,
    ``cells`` (per image: the cells of each region), ``shares`` (the same as fractions) and ``centroids`` (fp32 ``[R, 3]``).

    ``assign`` / ``pool`` / ``moments`` are the three device operations (``ops.kmeans_assign``, :func:`pool_cells`,
    ``color.statistics``); the host tests hand in NumPy twins with the same signatures and run the whole algorithm without a
    device."""
    regions = guidance.check_regions(regions)
    cell = check_cell(cell)
    images = (content, style)
    pooled = [pool(img, cell) for img in images]
    cells = [int(p.shape[-2]) * int(p.shape[-1]) for p in pooled]
    centroids = initial_centroids([moments(p) for p in pooled], regions)
    device = pooled[0].device
    labels = [torch.full(tuple(p.shape[-2:]), guidance.NO_REGION, dtype=torch.uint8, device=device) for p in pooled]
    parts = torch.empty(2, _lib.KMEANS_PARTS, _lib.KMEANS_PART_DOUBLES, dtype=torch.float64, device=device)
    counts = np.zeros((2, regions))
    iterations, converged = 0, False
    while iterations < max_iter and not converged:
        c_dev = torch.from_numpy(centroids).to(device)
        for i in range(2):                      # back to back; one readback of both buffers
            assign(pooled[i], c_dev, labels[i], parts[i])
        totals = parts.cpu().numpy().sum(axis=1, dtype=np.float64)          # the 256 rows in index order
        per_cluster = totals[:, :4 * _lib.KMEANS_MAX_K].reshape(2, _lib.KMEANS_MAX_K, 4)[:, :regions]
        sums, counts = per_cluster[..., :3], per_cluster[..., 3]
        centroids = update_centroids(centroids, sums, counts, cells)
        iterations += 1
        converged = float(totals[:, -1].sum()) == 0.0
    maps = [guidance.resample_labels(lab.cpu(), int(img.shape[-2]), int(img.shape[-1])) for lab, img in zip(labels, images, strict=True)]
    info = {"regions": regions, "cell": cell, "iterations": iterations, "converged": converged,
            "cells": {name: [int(v) for v in counts[i]] for i, name in enumerate(_IMAGES)},
            "shares": {name: [float(v) / cells[i] for v in counts[i]] for i, name in enumerate(_IMAGES)},
            "centroids": centroids}
    return maps[0], maps[1], info


def _refusal(content_labels: torch.Tensor, style_labels: torch.Tensor, info: dict, style_layers, levels: int) -> str | None:
    """Why a segmentation is not accepted (the region, the image and the count named), or ``None``."""
    from . import pyramid, synthetic  # noqa: PLC0415
    regions = info["regions"]
    for name in _IMAGES:
        total = sum(info["cells"][name])
        for r, n in enumerate(info["cells"][name]):
            if n * MIN_SHARE_DIV < total:
                return f"region {r} holds {n} of the {total} cells of the {name} image, fewer than 1/{MIN_SHARE_DIV}"
    factor = 1 << (levels - 1)
    style_hw = tuple(int(v) & ~(factor - 1) for v in style_labels.shape)
    for level, maps in enumerate(pyramid.label_halvings(content_labels, style_labels, style_hw, levels)):
        for name, labels in zip(_IMAGES, maps, strict=True):
            H, W = (int(v) for v in labels.shape)
            shapes = guidance.tap_shapes(H, W, synthetic.VGG19_CFG, style_layers)
            for layer, tap in zip(sorted(set(style_layers)), guidance.tap_maps(labels, shapes), strict=True):
                for r, n in enumerate(guidance.region_counts(tap, regions)):
                    if n == 0:
                        where = f" at {W}x{H} (pyramid level {levels - level} of {levels})" if levels > 1 else ""
                        return (f"region {r} holds 0 pixels of the {name} image's {tap.shape[1]}x{tap.shape[0]} label map at "
                                f"style layer {layer}{where}")
    return None


def auto_guidance(content: torch.Tensor, style: torch.Tensor, oc, levels: int = 1, **kernels) -> tuple[torch.Tensor, torch.Tensor] | None:
    """The label maps of a run with ``oc.auto_mask``: :func:`auto_labels` with ``oc.mask_regions`` regions, and with one region
    fewer for as long as the segmentation is not accepted (module docstring), each time with one info line; ``None`` - the run
    is unguided, with one warning - when not even two regions are.  ``oc.mask_regions`` is set to the number of regions the
    maps hold: from here on they are handled exactly as maps read from files.  ``levels``: the run's ``pyramid_levels``.
    ``kernels``: handed to :func:`auto_labels` (``assign=``, ``pool=``, ``moments=``)."""
    asked = guidance.check_regions(getattr(oc, "mask_regions", 2), minimum=2, what="mask_regions")
    cell = check_cell(getattr(oc, "auto_mask_cell", DEFAULT_CELL))
    check_sizes(content.shape[-2:], style.shape[-2:], cell)        # (before the first launch)
    for regions in range(asked, 1, -1):
        content_labels, style_labels, info = auto_labels(content, style, regions, cell=cell, **kernels)
        why = _refusal(content_labels, style_labels, info, list(oc.style_layers), levels)
        if why is None:
            info["regions_asked"] = asked
            logger.info("Automatic masks: %d regions (asked for %d), cells of %d pixels, %d iterations%s; shares content %s, "
                        "style %s; centroids %s", regions, asked, cell, info["iterations"],
                        "" if info["converged"] else " (not converged)",
                        [round(v, 4) for v in info["shares"]["content"]], [round(v, 4) for v in info["shares"]["style"]],
                        [[round(float(v), 4) for v in row] for row in info["centroids"]])
            oc.mask_regions = regions
            return content_labels, style_labels
        logger.info("Automatic masks: %d regions not accepted: %s%s", regions, why,
                    f"; trying {regions - 1}" if regions > 2 else "")      # noqa: PLR2004
    logger.warning("Automatic masks: the two images do not split into two colour regions that both hold; "
                   "the run proceeds unguided (no masks)")
    return None


def save_label_png(labels: torch.Tensor, regions: int, path: str | Path) -> None:
    """``labels`` as an 8-bit grey PNG: region ``k`` at grey level ``((2k+1)*256) // (2R)``, the centre of its band under
    ``guidance.quantize`` - ``guidance.load_mask(path, ..., R, ...)`` reads back the same map."""
    from PIL import Image  # noqa: PLC0415
    lab = guidance.check_labels(labels, regions)
    if bool((lab >= regions).any()):
        msg = f"save_label_png: the map holds pixels of no region ({guidance.NO_REGION}); a grey level cannot say that"
        raise ValueError(msg)
    grey = ((2 * lab.to(torch.int32) + 1) * 256) // (2 * regions)
    Image.fromarray(grey.to(torch.uint8).numpy(), mode="L").save(str(path))
