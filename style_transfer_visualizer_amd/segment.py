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
               lam <= (s^2 * 2^-24)^2 * (tr E_c[x x^T] + tr E_s[x x^T]) / 2 over the raw pixels counts as 0: a spread that the
               rounding of the fp32 box means alone can produce (pooling_noise) is no spread
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

**Feature space** (``optimization.auto_mask_space = "features"``, ``auto_mask_layer``, default 10 = conv3_1).  Colour is a weak
correspondence: a day photograph and a night painting share no palette, and two textures of one mean colour are one region to
it.  The same joint k-means then runs on the activations of one VGG layer instead of box means of colours; a point is a pixel
of ``C`` = 64 to 512 channels, ``auto_mask_cell`` is unused and the layer's grid is the grid::

    F_i      = output of VGG index `layer` for image i, as the run sees the image (behind resize and preserve_color = match),
               in the run's precision and pooling; NHWC [n_i][C], bf16 or fp32 storage         (extract_features: plan.Schedule)
    mu       = (mean(F_c) + mean(F_s)) / 2                  (ops.kmeans_feat_assign keeping all-zero labels, K = 1)
    Sigma    = (F_c^T F_c / n_c + F_s^T F_s / n_s) / 2 - mu mu^T    (ops.gram_partial slabs summed in float64 on the host)
    v, lam   = principal eigenvector / eigenvalue (numpy eigh, C x C float64); the sign rule of principal_axis
    c_k(0)   = fp32(mu + sqrt(max(lam, 0)) * z_k * v),  z_k = -1 + (2k+1)/R

    iteration t (at most MAX_ITER):
      label(p)  = argmin_k d_k(p), a strict `<` in ascending k; d_k: per octet of 8 channels p = p + e*e in ascending order,
                  the C/8 octet sums combined pairwise (s = C/16 ... 1: p[o] = p[o] + p[o+s]), every operation rounded to
                  fp32 on its own                                                           (ops.kmeans_feat_assign)
      S_k^i[c], N_k^i, changed^i in double, in the launch's fixed order (stv.h)
      c_k(t)    = fp32((S_k^c/n_c + S_k^s/n_s) / (N_k^c/n_c + N_k^s/n_s)) in double ON THE DEVICE; a cluster empty in both
                  images keeps its centroid                                                 (ops.kmeans_feat_update)
      stop when changed^c + changed^s == 0       (the one readback per iteration: nine doubles; nothing is uploaded)

The grid labels ``[H_l][W_l]`` become image-size maps through ``guidance.resample_labels``; acceptance, the fall-back to ``R - 1``
and the unguided run with its warning are those of colour mode.  The two schedules of the extraction are dropped before the
run's model is built, and the generator state is put back behind the construction of the stack.

Not built: L2-normalised (cosine) distances, spatial coordinates in the feature vector, more than one layer at a time,
per-region weights (the numbers of the regions are not known in advance), several style images, row strips (``spatial.py``).
"""
from __future__ import annotations

import functools
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
MIN_CELLS_SIDE = 8                # the shorter side of either pooled map (colour) or feature grid (features)
SPACES = ("color", "features")    # where the clustering runs: box means of the colours, or one VGG layer's activations
MAX_FEATURE_ELEMENTS = 1 << 31    # n * C of one image's features: the bound of stv_kmeans_feat_assign
DEFAULT_LAYER = 10                # conv3_1: 256 channels on a quarter-size grid
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
        space = check_space(getattr(oc, "auto_mask_space", "color"))
        if space != "color":
            msg = f"--auto-mask-space {space} without --auto-mask: the option says where --auto-mask clusters and does nothing alone"
            raise ValueError(msg)
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
    if check_space(getattr(oc, "auto_mask_space", "color")) == "features":      # (the cell size is unused there)
        check_layer(getattr(oc, "auto_mask_layer", DEFAULT_LAYER))
    else:
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


def pooling_noise(raw_stats, cell: int) -> float:
    """An upper bound of the principal eigenvalue that the ROUNDING of the fp32 box means alone can put into ``Sigma``.
    An fp32 sum of ``m = cell*cell`` values in any order, times ``1/m``, is off by at most ``m * u * mean|x|`` of its box
    (``u = 2^-24``, first order); squared and averaged over the boxes that is at most ``(m u)^2 E[x^2]`` per channel (Jensen),
    and an eigenvalue of the rounding's covariance is at most its trace.  ``raw_stats``: ``color.statistics`` of the two images
    (the pixels the boxes cover); each image weighs 1/2.  ``cell == 1``: the pooled map is a copy, 0."""
    if cell == 1:
        return 0.0
    u = 2.0 ** -24
    trace = sum(float(np.trace(np.asarray(moments, dtype=np.float64))) / n for n, _, moments in raw_stats) / 2.0
    return (cell * cell * u) ** 2 * trace


def image_noise(images, cell: int, moments=None) -> float:
    """:func:`pooling_noise` of the two images: ``moments`` (``color.statistics``) of the pixels the ``cell x cell`` boxes cover.
    It does not depend on the number of regions: :func:`auto_guidance` forms it once."""
    if cell == 1:
        return 0.0
    moments = color.statistics if moments is None else moments
    covered = [img[..., :int(img.shape[-2]) // cell * cell, :int(img.shape[-1]) // cell * cell] for img in images]
    return pooling_noise([moments(img) for img in covered], cell)


def initial_centroids(stats, regions: int, noise: float = 0.0) -> np.ndarray:
    """``c_k(0)`` as fp32 ``[R, 3]`` from the two pooled maps' ``color.statistics`` (each image weighs 1/2).  ``noise``
    (:func:`pooling_noise`): a principal eigenvalue not above it counts as 0 - the centroids coincide, every cell gets label 0
    and the segmentation is not accepted - since a spread that small cannot be told from the rounding of the box means."""
    means = [np.asarray(sums, dtype=np.float64) / n for n, sums, _ in stats]
    seconds = [np.asarray(moments, dtype=np.float64) / n for n, _, moments in stats]
    mu = (means[0] + means[1]) / 2.0
    v, lam = principal_axis((seconds[0] + seconds[1]) / 2.0 - np.outer(mu, mu))
    if lam <= noise:
        lam = 0.0
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
                assign=ops.kmeans_assign, pool=pool_cells, moments=color.statistics, noise: float | None = None) -> tuple[torch.Tensor, torch.Tensor, dict]:
    """One joint segmentation of the two images into ``regions`` regions (module docstring): the label maps of the content
    and of the style image (host uint8, at the images' sizes) and ``info`` - ``regions``, ``iterations``, ``converged``,
    ``cells`` (per image: the cells of each region), ``shares`` (the same as fractions) and ``centroids`` (fp32 ``[R, 3]``).

    ``assign`` / ``pool`` / ``moments`` are the three device operations (``ops.kmeans_assign``, :func:`pool_cells`,
    ``color.statistics``); the host tests hand in NumPy twins with the same signatures and run the whole algorithm without a
    device.  ``noise``: :func:`image_noise` of the two images where the caller has it already."""
    regions = guidance.check_regions(regions)
    cell = check_cell(cell)
    images = (content, style)
    pooled = [pool(img, cell) for img in images]
    cells = [int(p.shape[-2]) * int(p.shape[-1]) for p in pooled]
    if noise is None:
        noise = image_noise(images, cell, moments)
    centroids = initial_centroids([moments(p) for p in pooled], regions, noise)
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


# ---- clustering in VGG feature space (auto_mask_space = "features") -------------------------------------------------------

def check_space(space) -> str:
    """Where ``--auto-mask`` clusters, out of :data:`SPACES`."""
    if not isinstance(space, str) or space not in SPACES:
        msg = f"auto_mask_space must be one of {list(SPACES)}, got {space!r}"
        raise ValueError(msg)
    return space


def layer_table() -> list[tuple[str, int, int]]:
    """Per index of the VGG19 feature stack: ``(kind, channels, pools in front)``, kind ``conv`` | ``relu`` | ``pool``."""
    from . import synthetic  # noqa: PLC0415
    table, channels, pools = [], 3, 0
    for v in synthetic.VGG19_CFG:
        if v == "M":
            pools += 1
            table.append(("pool", channels, pools))
        else:
            channels = int(v)
            table += [("conv", channels, pools), ("relu", channels, pools)]
    return table


def check_layer(layer) -> int:
    """The clustered layer as an int: a conv or ReLU index of the VGG19 stack (the indexing of ``style_layers``)."""
    table = layer_table()
    ok = not isinstance(layer, bool) and isinstance(layer, int) and 0 <= layer < len(table) and table[layer][0] != "pool"
    if not ok:
        pools = [i for i, row in enumerate(table) if row[0] == "pool"]
        msg = (f"auto_mask_layer must be a conv or ReLU index of the VGG19 stack (0 to {len(table) - 1} without the pooling "
               f"layers {pools}), got {layer!r}")
        raise ValueError(msg)
    return layer


def feature_grid(hw, layer: int) -> tuple[int, int]:
    """``(H_l, W_l)`` of layer ``layer``'s output for an image of ``hw``: halved (floor) once per pooling layer in front."""
    pools = layer_table()[layer][2]
    H, W = (int(v) for v in hw)
    for _ in range(pools):
        H, W = H // 2, W // 2
    return H, W


def check_feature_sizes(content_hw, style_hw, layer: int) -> None:
    """Either image at run size gives a feature grid whose shorter side has at least ``MIN_CELLS_SIDE`` cells."""
    (Hc, Wc), (Hs, Ws) = feature_grid(content_hw, layer), feature_grid(style_hw, layer)
    if min(Hc, Wc) < MIN_CELLS_SIDE or min(Hs, Ws) < MIN_CELLS_SIDE:
        msg = (f"--auto-mask-space features: layer {layer} leaves a {Wc}x{Hc} grid of the {int(content_hw[1])}x{int(content_hw[0])} "
               f"content image and a {Ws}x{Hs} grid of the {int(style_hw[1])}x{int(style_hw[0])} style image; the shorter side "
               f"needs at least {MIN_CELLS_SIDE} (use an earlier --auto-mask-layer or larger images)")
        raise ValueError(msg)
    channels = layer_table()[layer][1]
    for name, (H, W) in zip(_IMAGES, ((Hc, Wc), (Hs, Ws)), strict=True):
        if H * W * channels >= MAX_FEATURE_ELEMENTS:
            msg = (f"--auto-mask-space features: layer {layer} gives {W}x{H} pixels of {channels} channels of the {name} image, "
                   f"{H * W * channels} elements; the feature k-means takes fewer than {MAX_FEATURE_ELEMENTS} (use a later "
                   "--auto-mask-layer or smaller images)")
            raise ValueError(msg)


def extract_features(img: torch.Tensor, layers, layer: int, dtype: torch.dtype, *, split: bool = False) -> torch.Tensor:
    """``F``: the output of VGG index ``layer`` for a device image ``[1, 3, H, W]``, NHWC ``[H_l, W_l, C]`` in ``dtype`` - one
    forward program of a schedule at the image's own size with that layer as its only tap, as ``capture_style`` builds one for
    a style image.  The schedule is dropped with the call; the activation lives on."""
    from . import plan  # noqa: PLC0415
    x = img.detach().contiguous().float()
    H, W = (int(v) for v in x.shape[-2:])
    sched = plan.Schedule(list(layers), [], [layer], H, W, dtype, x.device, with_grad=False, split=split,
                          switches=plan.Switches.from_env())
    plan.Program(sched.forward_ops(x), extra=(sched,)).run()
    return sched.content_taps[0].buf.act


def run_features(content: torch.Tensor, style: torch.Tensor, layer: int, oc, precision) -> list[torch.Tensor]:
    """The two images' features as the run will see them: the run's stack (its weights and ``oc.pooling``), its precision
    (``None``: ``STV_PRECISION`` or fp32, as for the model).
    The generator state is put back: building the stack here leaves the run's own random draws where they were."""
    from . import core_model  # noqa: PLC0415
    state = torch.get_rng_state()
    try:
        # core_model's stack cache is keyed by the generator state a construction starts from; the run has not seeded yet, so
        # that state is whatever the process left.  From one constant state every call after the process's first is a cache hit.
        torch.set_rng_state(torch.Generator().manual_seed(0).get_state())
        vgg = core_model.replace_pooling(core_model.initialize_vgg(), core_model.check_pooling(getattr(oc, "pooling", "max")))
    finally:
        torch.set_rng_state(state)
    dtype, split = core_model.resolve_precision(precision), core_model.resolve_split(precision)
    return [extract_features(img, list(vgg.children()), layer, dtype, split=split) for img in (content, style)]


def feature_moments(F: torch.Tensor, *, split: bool = False):
    """``(n, sums[C], second[C, C])`` of device features ``[..., C]`` in float64: the channel sums from one
    ``ops.kmeans_feat_assign`` launch that keeps its labels (all 0, ``K = 1``), the raw second moments ``F^T F`` from the
    ``ops.gram_partial`` slabs (an MFMA product in the storage precision), both added up in float64 on the host.  The slabs
    hold the upper tile triangle; the lower one is its mirror."""
    C = int(F.shape[-1])
    n = F.numel() // C
    flat = F.reshape(n, C)
    labels = torch.zeros(n, dtype=torch.uint8, device=F.device)
    parts = ops.kmeans_feat_assign(flat, torch.zeros(1, C, dtype=torch.float32, device=F.device), labels, keep_labels=True)
    sums = parts[:, :C].cpu().numpy().sum(axis=0, dtype=np.float64)
    slabs = ops.gram_partial(flat, split=split).cpu().numpy().astype(np.float64).sum(axis=0)
    upper = np.triu(slabs)
    return n, sums, upper + np.triu(slabs, 1).T


def feature_start(stats, regions: int) -> dict:
    """``c_k(0)`` as fp32 ``[R, C]`` (``centroids``) with ``mu``, ``lam`` and ``v`` from the two images' :func:`feature_moments`
    (each image weighs 1/2): :func:`initial_centroids` in ``C`` dimensions."""
    means = [np.asarray(sums, dtype=np.float64) / n for n, sums, _ in stats]
    seconds = [np.asarray(second, dtype=np.float64) / n for n, _, second in stats]
    mu = (means[0] + means[1]) / 2.0
    v, lam = principal_axis((seconds[0] + seconds[1]) / 2.0 - np.outer(mu, mu))
    z = -1.0 + (2.0 * np.arange(regions, dtype=np.float64) + 1.0) / regions
    centroids = (mu[None, :] + math.sqrt(max(lam, 0.0)) * z[:, None] * v[None, :]).astype(np.float32)
    return {"centroids": centroids, "mu": mu, "lam": lam, "v": v}


def feature_labels(F_c: torch.Tensor, F_s: torch.Tensor, regions: int, *, max_iter: int = MAX_ITER, centroids=None, stats=None,  # noqa: PLR0913
                   assign=ops.kmeans_feat_assign, update=ops.kmeans_feat_update, moments=feature_moments) -> tuple[torch.Tensor, torch.Tensor, dict]:
    """One joint segmentation of the two images' features (NHWC ``[H_l, W_l, C]``, fp32 or bf16) into ``regions`` regions
    (module docstring): the label grids of the content and of the style image (host uint8 ``[H_l, W_l]``) and ``info`` -
    ``regions``, ``iterations``, ``converged``, ``cells``, ``shares``, ``centroids`` (fp32 ``[R, C]``), ``grids``, ``start``.

    ``centroids``: the start (fp32 ``[R, C]``) instead of the principal-axis one; ``stats``: the two images' moments where
    the caller has them already.  Per iteration two assignments, one update and one readback of nine doubles; nothing is
    uploaded.  ``assign`` / ``update`` / ``moments`` are the device operations; the host tests hand in NumPy twins."""
    regions = guidance.check_regions(regions)
    feats = (F_c, F_s)
    C = int(F_c.shape[-1])
    if any(F.dim() != 3 or int(F.shape[-1]) != C for F in feats):      # noqa: PLR2004
        msg = f"feature_labels: features of {tuple(F_c.shape)} and {tuple(F_s.shape)}, expected two [H, W, C] of one C"
        raise ValueError(msg)
    device = F_c.device
    cells = [int(F.shape[0]) * int(F.shape[1]) for F in feats]
    start = None
    if centroids is None:
        start = feature_start(stats if stats is not None else [moments(F) for F in feats], regions)
        centroids = start["centroids"]
    c_dev = torch.from_numpy(np.ascontiguousarray(centroids, dtype=np.float32)).to(device)
    if tuple(c_dev.shape) != (regions, C):
        msg = f"feature_labels: starting centroids of {tuple(c_dev.shape)}, expected {(regions, C)}"
        raise ValueError(msg)
    labels = [torch.full((n,), guidance.NO_REGION, dtype=torch.uint8, device=device) for n in cells]
    parts = [torch.empty(_lib.KMF_PARTS, _lib.kmf_row_doubles(C), dtype=torch.float64, device=device) for _ in feats]
    result = torch.empty(9, dtype=torch.float64, device=device)
    counts = np.zeros((2, regions))
    iterations, converged = 0, False
    while iterations < max_iter and not converged:
        for i in range(2):
            assign(feats[i], c_dev, labels[i], parts[i])
        update(parts[0], parts[1], c_dev, cells[0], cells[1], result)
        host = result.cpu().numpy()                                   # the one readback: 72 bytes
        counts = host[:2 * _lib.KMF_MAX_K].reshape(2, _lib.KMF_MAX_K)[:, :regions]
        iterations += 1
        converged = float(host[-1]) == 0.0
    grids = [lab.cpu().reshape(int(F.shape[0]), int(F.shape[1])) for lab, F in zip(labels, feats, strict=True)]
    info = {"regions": regions, "iterations": iterations, "converged": converged,
            "cells": {name: [int(v) for v in counts[i]] for i, name in enumerate(_IMAGES)},
            "shares": {name: [float(v) / cells[i] for v in counts[i]] for i, name in enumerate(_IMAGES)},
            "centroids": c_dev.cpu().numpy(), "grids": [tuple(g.shape) for g in grids], "start": start}
    return grids[0], grids[1], info


def _feature_guidance(content: torch.Tensor, style: torch.Tensor, oc, levels: int, asked: int, precision, *, extract=run_features,
                      **kernels) -> tuple[torch.Tensor, torch.Tensor] | None:
    """:func:`auto_guidance` with ``oc.auto_mask_space = "features"``: the features once, then :func:`feature_labels` with
    ``asked`` regions and with one fewer for as long as the segmentation is not accepted."""
    layer = check_layer(getattr(oc, "auto_mask_layer", DEFAULT_LAYER))
    check_feature_sizes(content.shape[-2:], style.shape[-2:], layer)        # (before the first launch)
    feats = extract(content, style, layer, oc, precision)
    if "moments" not in kernels and getattr(feats[0], "is_cuda", False):
        from . import core_model  # noqa: PLC0415
        kernels["moments"] = functools.partial(feature_moments, split=core_model.resolve_split(precision))
    stats = [kernels.get("moments", feature_moments)(F) for F in feats]
    sizes = [tuple(int(v) for v in img.shape[-2:]) for img in (content, style)]
    for regions in range(asked, 1, -1):
        grid_c, grid_s, info = feature_labels(feats[0], feats[1], regions, stats=stats, **kernels)
        content_labels, style_labels = (guidance.resample_labels(g, *hw) for g, hw in zip((grid_c, grid_s), sizes, strict=True))
        why = _refusal(content_labels, style_labels, info, list(oc.style_layers), levels)
        if why is None:
            info["regions_asked"] = asked
            (Hc, Wc), (Hs, Ws) = info["grids"]
            logger.info("Automatic masks: feature space, layer %d (grids %dx%d and %dx%d, %d channels), %d regions (asked for "
                        "%d), %d iterations%s; shares content %s, style %s", layer, Wc, Hc, Ws, Hs, int(feats[0].shape[-1]),
                        regions, asked, info["iterations"], "" if info["converged"] else " (not converged)",
                        [round(v, 4) for v in info["shares"]["content"]], [round(v, 4) for v in info["shares"]["style"]])
            oc.mask_regions = regions
            return content_labels, style_labels
        logger.info("Automatic masks: %d regions not accepted: %s%s", regions, why,
                    f"; trying {regions - 1}" if regions > 2 else "")      # noqa: PLR2004
    logger.warning("Automatic masks: the two images do not split into two feature regions that both hold; "
                   "the run proceeds unguided (no masks)")
    return None


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


def auto_guidance(content: torch.Tensor, style: torch.Tensor, oc, levels: int = 1, *, precision: str | None = None,
                  **kernels) -> tuple[torch.Tensor, torch.Tensor] | None:
    """The label maps of a run with ``oc.auto_mask``: :func:`auto_labels` with ``oc.mask_regions`` regions, and with one region
    fewer for as long as the segmentation is not accepted (module docstring), each time with one info line; ``None`` - the run
    is unguided, with one warning - when not even two regions are.  ``oc.mask_regions`` is set to the number of regions the
    maps hold: from here on they are handled exactly as maps read from files.  ``levels``: the run's ``pyramid_levels``.
    ``kernels``: handed to :func:`auto_labels` (``assign=``, ``pool=``, ``moments=``).
    With ``oc.auto_mask_space = "features"`` the same with :func:`feature_labels` on the activations of VGG index
    ``oc.auto_mask_layer`` in the run's ``precision`` (``kernels``: ``assign=``, ``update=``, ``moments=``, ``extract=``)."""
    asked = guidance.check_regions(getattr(oc, "mask_regions", 2), minimum=2, what="mask_regions")
    if check_space(getattr(oc, "auto_mask_space", "color")) == "features":
        return _feature_guidance(content, style, oc, levels, asked, precision, **kernels)
    cell = check_cell(getattr(oc, "auto_mask_cell", DEFAULT_CELL))
    check_sizes(content.shape[-2:], style.shape[-2:], cell)        # (before the first launch)
    noise = image_noise((content, style), cell, kernels.get("moments"))      # (once: it is the same for every R)
    for regions in range(asked, 1, -1):
        content_labels, style_labels, info = auto_labels(content, style, regions, cell=cell, noise=noise, **kernels)
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
