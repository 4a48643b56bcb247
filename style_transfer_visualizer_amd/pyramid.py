"""Coarse-to-fine runs (``optimization.pyramid_levels`` > 1): the schedule over image sizes.

Level ``k`` of ``levels`` works at ``(H >> (levels-1-k), W >> (levels-1-k))``, coarsest first.  Content and style of a
level are the loaded tensors halved on the device by ``ops.resize2x`` (2x2 box mean, in the normalised space); the
coarsest level starts from ``initialize_input`` and every later one from the previous result doubled by the same kernel
(bilinear), as a fresh leaf.  Every level is a fresh ``StyleContentModel``, a fresh optimiser and an unchanged
``OptimizationRunner`` on a copy of the config whose ``steps`` is that level's count: each step is the fused step the
single-level run takes, and the image never visits the host between levels.

Several style images (``style_mix.py``): ``style_img`` may be a list; each image is cropped and halved on its own, and each
level's targets are blended from that level's images.

Not built: frames (video / GIF) during such a run - their size would change between levels, so the built-in GIF collector
(``gif.py``) is not created for one either -, ratios other than two between levels, and row strips (``spatial.py``).
"""
from __future__ import annotations

import contextlib
import copy
import csv
import gc
from collections.abc import Callable
from pathlib import Path

import torch
from torch.optim import Optimizer

from . import _lib, core_model, ops, optimization, runtime, style_mix
from .constants import MIN_DIMENSION
from .logging_utils import logger
from .loss_logger import HEADER
from .optimizers import make_lbfgs
from .type_defs import LossHistory


def level_shapes(H: int, W: int, levels: int) -> list[tuple[int, int]]:
    """``(H >> k, W >> k)`` for the ``levels`` levels, coarsest first."""
    return [(H >> k, W >> k) for k in range(levels - 1, -1, -1)]


def level_steps(steps: int, levels: int, explicit: list[int] | None = None) -> list[int]:
    """Optimiser steps per level, coarsest first.  ``explicit`` (``optimization.pyramid_steps``) is used as given - it
    needs ``levels`` entries of at least 1, and the run then takes their sum; otherwise ``steps`` is split evenly and the
    remainder goes to the coarsest levels, one each."""
    if explicit is not None:
        counts = [int(v) for v in explicit]
        if len(counts) != levels:
            msg = f"pyramid_steps has {len(counts)} entries for {levels} pyramid levels"
            raise ValueError(msg)
        for v in counts:
            if v < 1:
                msg = f"pyramid_steps entries must be at least 1, got {v}"
                raise ValueError(msg)
        return counts
    if steps < levels:
        msg = f"{steps} steps cannot be split over {levels} pyramid levels (at least one step per level)"
        raise ValueError(msg)
    base, extra = divmod(steps, levels)
    return [base + (1 if k < extra else 0) for k in range(levels)]


def level_log_path(path: str | Path, level: int) -> Path:
    """``<stem>.level<k><suffix>`` next to ``path``: the loss CSV of one level while the run is under way."""
    p = Path(path)
    return p.with_name(f"{p.stem}.level{level}{p.suffix}")


def _validate(content_img: torch.Tensor, style_img: torch.Tensor, config, video_writer, gif_collector) -> tuple[int, int, int]:
    """The checks that need no model; returns (levels, style height, style width) after the crop."""
    levels = int(config.optimization.pyramid_levels)
    factor = 1 << (levels - 1)
    if levels > 1 and (video_writer is not None or gif_collector is not None
                       or config.video.create_video or config.video.create_gif):
        msg = (f"pyramid_levels = {levels} cannot be combined with a video or GIF: frames would change size between "
               "levels (not built; use --no-video / --final-only, or pyramid_levels = 1)")
        raise ValueError(msg)
    H, W = (int(v) for v in content_img.shape[-2:])
    for name, size in (("height", H), ("width", W)):
        if size % factor:
            msg = f"content {name} {size} is not divisible by {factor} (2**(pyramid_levels-1), pyramid_levels = {levels})"
            raise ValueError(msg)
    Hs, Ws = (int(v) & ~(factor - 1) for v in style_img.shape[-2:])
    for name, size in (("content height", H), ("content width", W), ("style height", Hs), ("style width", Ws)):
        if size // factor < MIN_DIMENSION:
            msg = (f"{name} {size} is {size // factor} at the coarsest of {levels} pyramid levels; "
                   f"the minimum dimension is {MIN_DIMENSION}")
            raise ValueError(msg)
    oc = config.optimization
    if float(getattr(oc, "lap_w", 0.0) or 0.0) > 0:        # every level pools its own content: the coarsest decides
        from .core_model import check_lap_fits, check_lap_pools  # noqa: PLC0415
        check_lap_fits(check_lap_pools(oc.lap_pools), H // factor, W // factor,
                       f" (the coarsest of {levels} pyramid levels)" if levels > 1 else "")
    return levels, Hs, Ws


def _halvings(img: torch.Tensor, levels: int) -> list[torch.Tensor]:
    """``img`` at every level, coarsest first: DOWN2 applied ``levels-1-k`` times."""
    chain = [img.contiguous()]
    for _ in range(levels - 1):
        chain.append(ops.resize2x(chain[-1], _lib.RESIZE_DOWN2))
    return chain[::-1]


def label_halvings(content_labels: torch.Tensor, style_labels: torch.Tensor, style_hw: tuple[int, int], levels: int) -> list:
    """The two label maps at every level, FINEST first: the style's map cropped to ``style_hw`` (the slice the style image is
    cropped by), then each level resampled (``guidance.resample_labels``) from the next finer one."""
    from . import guidance  # noqa: PLC0415
    Hs, Ws = style_hw
    chain = [(content_labels, style_labels[:Hs, :Ws].contiguous())]
    for _ in range(levels - 1):
        c, s = chain[-1]
        chain.append((guidance.resample_labels(c, c.shape[0] // 2, c.shape[1] // 2),
                      guidance.resample_labels(s, s.shape[0] // 2, s.shape[1] // 2)))
    return chain


def level_labels(content_labels, style_labels, style_hw: tuple[int, int], levels: int, n_styles: int, oc) -> list | None:
    """Per level, coarsest first, the keyword arguments of a guided level: (those of the model, those of ``set_targets``);
    ``None`` without label maps.  The style's map is cropped by the slice the style image was cropped by; a level's maps
    are resampled (``guidance.resample_labels``) from the maps of the next finer level - the stage in front of it."""
    if content_labels is None and style_labels is None:
        return None
    if content_labels is None or style_labels is None:
        msg = "content_labels and style_labels go together: one label map without the other"
        raise ValueError(msg)
    if n_styles != 1:
        msg = f"spatial guidance takes one style image, got {n_styles} (masks with several style images are not built)"
        raise ValueError(msg)
    from . import guidance  # noqa: PLC0415
    model_kw = {"guide_regions": guidance.check_regions(getattr(oc, "mask_regions", 2), minimum=2, what="mask_regions"),
                "region_weights": getattr(oc, "region_weights", None)}
    chain = label_halvings(content_labels, style_labels, style_hw, levels)
    from . import synthetic  # noqa: PLC0415
    for c, s in chain[::-1]:            # an active region that vanishes at a tap of some level: refused before the first launch
        guidance.check_maps(guidance.make_guide(model_kw["guide_regions"], model_kw["region_weights"], c, s),
                            synthetic.VGG19_CFG, oc.style_layers)
    return [(model_kw, {"content_labels": c, "style_labels": s}) for c, s in chain[::-1]]


def _merge_csv(target: Path, parts: list[tuple[Path, int]]) -> None:
    """One header and the levels' rows in order, ``step`` shifted by the steps before each level; removes the parts."""
    with target.open("w", newline="", encoding="utf-8") as out:
        writer = csv.writer(out)
        writer.writerow(HEADER)
        for path, offset in parts:
            with path.open(newline="", encoding="utf-8") as fh:
                rows = csv.reader(fh)
                next(rows, None)
                for row in rows:
                    writer.writerow([int(row[0]) + offset, *row[1:]])
    for path, _ in parts:
        path.unlink()


def run_pyramid(  # noqa: PLR0913
    content_img: torch.Tensor,
    style_img: torch.Tensor,
    device: torch.device,
    config,
    *,
    optimizer_factory: Callable[[torch.Tensor], Optimizer] | None = None,
    progress_bar: optimization.ProgressReporter | None = None,
    video_writer: optimization.FrameSink | None = None,
    gif_collector: optimization.FrameSink | None = None,
    seed: int | None = None,
    setup_lock=None,
    content_labels: torch.Tensor | None = None,
    style_labels: torch.Tensor | None = None,
) -> tuple[torch.Tensor, LossHistory, float]:
    """Run ``config.optimization.pyramid_levels`` levels, coarsest first; returns (image, history, elapsed) like
    ``OptimizationRunner.run``: the final level's image, the levels' histories concatenated per key, the seconds the
    levels' runners took together.

    ``video_writer`` / ``gif_collector`` exist to be refused.  ``seed``: seed the generators right before the coarsest
    level is built; ``setup_lock``: held while that happens and while any level's model is constructed (constructing one
    draws from the process-wide CPU generator) - ``main.style_transfer`` passes both, as it seeds under its lock in a
    single-level run.  ``content_labels`` / ``style_labels`` (both or neither; ``guidance.py``): the label maps of a guided
    run at the full size - the style's is cropped by the style's slice, each level's map is resampled from the next finer
    level's, and every level is a fresh guided model."""
    style_list = list(style_img) if isinstance(style_img, (list, tuple)) else [style_img]
    crops = [_validate(content_img, img, config, video_writer, gif_collector) for img in style_list]
    levels = crops[0][0]
    oc = config.optimization
    counts = level_steps(oc.steps, levels, oc.pyramid_steps)
    H, W = (int(v) for v in content_img.shape[-2:])
    shapes = level_shapes(H, W, levels)
    for i, (img, (_, Hs, Ws)) in enumerate(zip(style_list, crops, strict=True)):
        if (Hs, Ws) != tuple(img.shape[-2:]):
            logger.info("Style image cropped from %dx%d to %dx%d (a multiple of %d on both sides)",
                        img.shape[-1], img.shape[-2], Ws, Hs, 1 << (levels - 1))
            style_list[i] = img[..., :Hs, :Ws]
    contents, per_style = _halvings(content_img, levels), [_halvings(img, levels) for img in style_list]
    label_chain = level_labels(content_labels, style_labels, crops[0][1:], levels, len(style_list), oc)
    # level k's style: the tensor itself for one image (as always), the list of that level's images for a blend
    styles = per_style[0] if len(per_style) == 1 else [[chain[k] for chain in per_style] for k in range(levels)]

    log_path = Path(config.output.log_loss) if config.output.log_loss else None
    lock = setup_lock if setup_lock is not None else contextlib.nullcontext()
    owns_bar = progress_bar is None
    if owns_bar:
        from tqdm import tqdm  # noqa: PLC0415
        progress_bar = tqdm(total=sum(counts), desc="Style Transfer")

    history: LossHistory = {}
    csv_parts: list[tuple[Path, int]] = []
    elapsed, done = 0.0, 0
    image: torch.Tensor | None = None
    try:
        for k, (steps, (h, w)) in enumerate(zip(counts, shapes, strict=True)):
            logger.info("Pyramid level %d/%d: %dx%d, %d steps", k + 1, levels, w, h, steps)
            cfg = copy.deepcopy(config)
            cfg.optimization.steps = steps
            if log_path is not None:
                cfg.output.log_loss = str(level_log_path(log_path, k))
            with lock:
                if k == 0 and seed is not None:
                    runtime.setup_random_seed(seed)
                model = core_model.StyleContentModel(style_layers=oc.style_layers, content_layers=oc.content_layers,
                                                     precision=config.hardware.precision,
                                                     **style_mix.option_kwargs(oc, "style_layer_weights"),
                                                     **core_model.lap_option_kwargs(oc),
                                                     **core_model.pooling_option_kwargs(oc),
                                                     **(label_chain[k][0] if label_chain else {})).to(device)
                model.set_targets(styles[k], contents[k], **style_mix.option_kwargs(oc, "style_blend"),
                                  **(label_chain[k][1] if label_chain else {}))
                if k == 0:
                    input_img = core_model.initialize_input(contents[0], oc.init_method)
                else:
                    input_img = ops.resize2x(image.detach().contiguous(), _lib.RESIZE_UP2).requires_grad_(True)  # noqa: FBT003
            optimizer = (optimizer_factory(input_img) if optimizer_factory is not None else
                         make_lbfgs(input_img, lr=oc.lr, max_iter=oc.lbfgs_max_iter, max_eval=oc.lbfgs_max_eval))
            runner = optimization.OptimizationRunner(model, input_img, cfg, optimizer=optimizer, progress_bar=progress_bar)
            if runner.loss_logger is not None:
                csv_parts.append((Path(cfg.output.log_loss), done))
            image, level_history, seconds = runner.run()
            for key, vals in level_history.items():       # (loss lists only: the history carries no step numbers)
                history.setdefault(key, []).extend(vals)
            elapsed += seconds
            done += steps
            # A cached program pins its L-BFGS history (2.6 GB at 1024^2): nothing of this level may outlive it but the
            # image.  Dropping the names is not enough.  The cycle is torch's: frames of torch.optim.Optimizer.__init__
            # stay in a cycle with the instance they built (torch 2.10: a bare torch.optim.SGD is not freed by `del`
            # either), HipLBFGS / HipAdam derive from that class, and the optimiser owns the image, its gradient and
            # the history.  Runner and model alone are freed by reference counting.  Once optimisers are, this
            # collection can go.
            del runner, optimizer, model, input_img
            gc.collect()
    finally:
        if owns_bar:
            progress_bar.close()
    if log_path is not None and csv_parts:        # only after a complete run: a level that raised leaves its level files
        _merge_csv(log_path, csv_parts)
    return image, history, elapsed
