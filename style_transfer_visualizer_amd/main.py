"""Top-level orchestration: the production caller of the hot path (reference main.py:20-167).

validate -> seed -> device -> load images -> model/targets/optimizer -> run -> save PNG ->
``input_img.detach().clamp(0, 1)``.  Timelapse video (MP4) encoding is presentation and is not
part of this build: any ``FrameSink`` may be injected, otherwise video requests are downgraded
with a warning and the run proceeds like ``--no-video``.

``video.create_gif`` (``gif.py``): a GIF timelapse is built in.  On a GPU, without an injected ``gif_collector`` and outside a
coarse-to-fine run, a ``gif.DeviceGifCollector`` captures the frames on the device and writes ``timelapse_{content}_x_{style}.gif``
(the reference's name) with one global palette when the run is over; its budget refusal comes before the run's first kernel.
The intro and outro segments of the reference's GIF need its gallery renderer, which is not built: the two flags are ignored
with a warning.  An injected collector wins; on a CPU device and in a coarse-to-fine run the request is downgraded as a video
request is.  With ``create_gif`` off nothing here changes.

``video.format = "mjpeg"`` (``mjpeg.py``): a Motion-JPEG timelapse video is built in under the same conditions - ``create_video``
on, a GPU, no injected ``video_writer``, one level -: a ``mjpeg.DeviceMjpegWriter`` keeps the frames' DCT coefficients on the
device and writes ``timelapse_{content}_x_{style}.avi`` when the run is over; its refusals (frame size, budget) come before the
run's first kernel.  The intro and outro segments need the gallery renderer: ``intro_enabled`` and ``final_frame_compare`` are
ignored with a warning.  With ``format = "mp4"`` (the default) nothing here changes: the request is downgraded as before.

``optimization.preserve_color`` (``color.py``, no counterpart in the reference) adds one stage at either end: "match"
re-colours the style image right behind the loads, "luma" restores the content image's chrominance in the result right
in front of the save; "off" adds nothing.

``optimization.content_size`` / ``style_size`` / ``style_scale`` (``resize.py``, no counterpart in the reference) add one stage
right behind the two loads and in front of the colour match: the loaded tensors are resized on the device by ``ops.resize``,
in the space they are in (normalised when normalisation is on), so colour statistics, the ``luma`` swap and a coarse-to-fine
run all see the images the run sees.  With all three at 0 the stage is not entered.

``InputPaths.extra_style_paths`` / ``optimization.style_blend`` / ``optimization.style_layer_weights`` (``style_mix.py``, no
counterpart in the reference): every style image is loaded, resized and colour-matched on its own by the rules above, and the
list is handed to the model, which blends the Gram targets.  With no extra style and both options unset nothing here changes.

``InputPaths.content_mask_path`` / ``style_mask_path`` with ``optimization.mask_regions`` / ``region_weights`` (``guidance.py``, no
counterpart in the reference): the two masks are read and checked before the first launch, their label maps follow the images
through the resize stage and through every level of a coarse-to-fine run, and the model is a guided one.  Without masks nothing
here changes.

``optimization.auto_mask`` / ``auto_mask_cell`` (``segment.py``, no counterpart in the reference): the two label maps come from a
joint colour segmentation of the two images as the run sees them - behind the resize stage and the colour match, in front of
the model - and are then handled as maps read from files are; a pair of images that does not split runs unguided.
``output.save_masks`` writes the label maps of a guided run next to the result.  With the options off nothing here changes.
"""
from __future__ import annotations

import threading
from pathlib import Path

import torch

from . import color, core_model, guidance, image_io, ops, optimization, pyramid, runtime, segment, style_mix
from . import gif as gif_output
from . import mjpeg as mjpeg_output
from . import resize as resize_rules
from .logging_utils import logger
from .type_defs import InputPaths, SaveOptions

# Several images may be in flight in one process (style_transfer_batch): seeding the global generators and drawing
# the start image from them is one step per image, as in a sequential run.
_SETUP_LOCK = threading.Lock()


def _resize_inputs(content_img: torch.Tensor, style_img: torch.Tensor, oc) -> tuple[torch.Tensor, torch.Tensor]:
    """The two images at the sizes ``resize.plan_sizes`` gives (refusals first: nothing is launched for a run that cannot
    start); an image that keeps its size is handed on as it is."""
    content_hw, style_hw = resize_rules.plan_sizes(oc, content_img.shape[-2:], style_img.shape[-2:])
    for name, hw, img in (("Content", content_hw, content_img), ("Style", style_hw, style_img)):
        if hw is not None:
            logger.info("%s image resized from %dx%d to %dx%d (%s)", name, img.shape[-1], img.shape[-2], hw[1], hw[0],
                        oc.resize_filter)
    if content_hw is not None:
        content_img = ops.resize(content_img.contiguous(), content_hw, oc.resize_filter)
    if style_hw is not None:
        style_img = ops.resize(style_img.contiguous(), style_hw, oc.resize_filter)
    return content_img, style_img


def _resize_extra_style(style_img: torch.Tensor, content_hw: tuple[int, int], oc) -> torch.Tensor:
    """A further style image of a blend at the size ``resize.plan_sizes`` gives it: ``style_size`` / ``style_scale`` apply to
    its own longer side, against the content as it was loaded (as for the first style)."""
    _, style_hw = resize_rules.plan_sizes(oc, content_hw, style_img.shape[-2:])
    if style_hw is None:
        return style_img
    logger.info("Style image resized from %dx%d to %dx%d (%s)", style_img.shape[-1], style_img.shape[-2], style_hw[1],
                style_hw[0], oc.resize_filter)
    return ops.resize(style_img.contiguous(), style_hw, oc.resize_filter)


def _load_masks(paths: InputPaths, oc) -> tuple[torch.Tensor, torch.Tensor] | None:
    """The label maps of the two masks (host uint8, at the pixel size of the image files), or ``None`` without masks.  Every
    refusal that needs no device comes from here: one mask without the other, masks with several style images, the number
    of regions, the region weights, a mask of another size than its image."""
    content_mask, style_mask = getattr(paths, "content_mask_path", None), getattr(paths, "style_mask_path", None)
    if not content_mask and not style_mask:
        return None
    if not content_mask or not style_mask:
        msg = (f"--content-mask and --style-mask go together: got content mask {content_mask!r} and style mask {style_mask!r} "
               "(region r of the content takes the statistics of region r of the style)")
        raise ValueError(msg)
    extra = tuple(getattr(paths, "extra_style_paths", ()))
    if extra:
        msg = f"masks cannot be combined with --style-also ({len(extra)} further style images): masks with several style images are not built"
        raise ValueError(msg)
    regions = guidance.check_regions(getattr(oc, "mask_regions", 2), minimum=2, what="mask_regions")
    guidance.check_region_weights(getattr(oc, "region_weights", None), regions)
    from PIL import Image  # noqa: PLC0415
    maps = []
    for which, image_path, mask_path in (("content", paths.content_path, content_mask), ("style", paths.style_path, style_mask)):
        runtime.validate_input_paths(image_path, mask_path)
        with Image.open(image_path) as img:
            W, H = img.size
        maps.append(guidance.load_mask(mask_path, (H, W), regions, which))
    return maps[0], maps[1]


def _check_save_masks(paths: InputPaths, guided: bool) -> None:
    """``output.save_masks`` needs a guided run and two different file names."""
    if not guided:
        msg = "--save-masks without masks: give --content-mask and --style-mask, or --auto-mask"
        raise ValueError(msg)
    content_stem, style_stem = Path(paths.content_path).stem, Path(paths.style_path).stem
    if content_stem == style_stem:
        msg = (f"--save-masks: content image {paths.content_path!r} and style image {paths.style_path!r} share the stem "
               f"{content_stem!r}, so both label maps would be written to {content_stem}_mask.png")
        raise ValueError(msg)


def _style_stem(paths: InputPaths) -> str:
    """The style part of the output names: the stems of the style images joined by ``+``."""
    return "+".join(Path(p).stem for p in (paths.style_path, *getattr(paths, "extra_style_paths", ())))


def style_transfer(paths: InputPaths, config, *, video_writer=None, gif_collector=None, output_tag: str = "",
                   tag_png: bool = True) -> torch.Tensor:
    """Run one style transfer; returns the optimised image clamped to [0, 1].

    ``output_tag`` (``style_transfer_batch``): appended to the names of this run's loss CSV and loss plot - and, with
    ``tag_png``, of its PNG - so that several runs writing into one directory do not overwrite each other."""
    runtime.validate_input_paths(paths.content_path, paths.style_path)
    extra_paths = tuple(getattr(paths, "extra_style_paths", ()))
    for path in extra_paths:
        runtime.validate_input_paths(paths.content_path, path)
    runtime.validate_parameters(config.video.quality)
    style_blend = getattr(config.optimization, "style_blend", None)
    layer_weights = getattr(config.optimization, "style_layer_weights", None)
    if extra_paths or style_blend is not None:      # refusals before the first launch: the count, the length, the weights
        style_mix.blend_weights(style_blend, 1 + len(extra_paths))
    if layer_weights is not None:
        style_mix.check_layer_weights(layer_weights, config.optimization.style_layers)

    auto_mask = segment.check_options(paths, config.optimization)      # (refusals before the first launch)
    labels = _load_masks(paths, config.optimization)      # (refusals before the first launch)
    save_masks = bool(getattr(config.output, "save_masks", False))
    if save_masks:
        _check_save_masks(paths, auto_mask or labels is not None)

    if config.video.final_only:                 # reference main.py:30-33
        config.video.create_video = False
        config.video.create_gif = False
        config.video.save_every = config.optimization.steps + 1
    device = runtime.setup_device(config.hardware.device)
    # the built-in GIF collector keeps its frames on the device and needs one frame size: a GPU run at one level
    builtin_gif = (config.video.create_gif and gif_collector is None and device.type == "cuda"
                   and config.optimization.pyramid_levels == 1)
    # the built-in Motion-JPEG writer (video.format = "mjpeg") keeps coefficients on the device: the same conditions
    builtin_mjpeg = (config.video.create_video and video_writer is None and getattr(config.video, "format", "mp4") == "mjpeg"
                     and device.type == "cuda" and config.optimization.pyramid_levels == 1)
    if ((config.video.create_video and video_writer is None and not builtin_mjpeg)
            or (config.video.create_gif and gif_collector is None and not builtin_gif)):
        logger.warning("Timelapse encoding is not part of the MI355X build; continuing without video/GIF "
                       "(pass --no-video to silence this, or inject a frame sink).")
        config.video.create_video = video_writer is not None or builtin_mjpeg
        config.video.create_gif = gif_collector is not None or builtin_gif
    if builtin_gif:                             # refusals before the first launch: the palette size, the dither
        gif_colors = gif_output.check_colors(getattr(config.video, "gif_colors", gif_output.MAX_COLORS))
        gif_dither = getattr(config.video, "gif_dither", "ordered")
        gif_output.dither_spread(gif_dither)
        if config.video.gif_include_intro or config.video.gif_include_outro:
            logger.warning("gif_include_intro / gif_include_outro are ignored: the intro and outro segments of the GIF timelapse "
                           "are not built; the file holds the frames of the run.")

    if builtin_mjpeg:                           # (the quality was validated above)
        if config.video.intro_enabled or config.video.final_frame_compare:
            logger.warning("intro_enabled / final_frame_compare are ignored: the intro and outro segments of the MJPEG timelapse "
                           "are not built; the file holds the frames of the run (--no-intro --no-final-frame-compare silence this).")

    normalize = config.optimization.normalize
    content_img = image_io.load_image_to_tensor(paths.content_path, device, normalize=normalize)
    style_img = image_io.load_image_to_tensor(paths.style_path, device, normalize=normalize)
    extra_styles = [image_io.load_image_to_tensor(path, device, normalize=normalize) for path in extra_paths]
    oc = config.optimization
    gif_frames = oc.steps // config.video.save_every if builtin_gif else 0
    video_frames = oc.steps // config.video.save_every if builtin_mjpeg else 0
    if builtin_gif or builtin_mjpeg:            # the run has the content's size: refuse a store over the budget before any kernel
        run_hw = tuple(int(v) for v in content_img.shape[-2:])
        if oc.content_size > 0 or oc.style_size > 0 or oc.style_scale > 0:
            run_hw = resize_rules.plan_sizes(oc, run_hw, style_img.shape[-2:])[0] or run_hw
        if builtin_gif:
            gif_output.check_budget(gif_frames, *run_hw)
        if builtin_mjpeg:
            mjpeg_output.check_frame_size(*run_hw)
            mjpeg_output.check_budget(video_frames, *run_hw)
    if oc.content_size > 0 or oc.style_size > 0 or oc.style_scale > 0:
        loaded_hw = tuple(int(v) for v in content_img.shape[-2:])
        content_img, style_img = _resize_inputs(content_img, style_img, oc)
        extra_styles = [_resize_extra_style(img, loaded_hw, oc) for img in extra_styles]
        if labels is not None:                  # the maps follow their images: nearest sampling in integer arithmetic
            labels = (guidance.resample_labels(labels[0], *(int(v) for v in content_img.shape[-2:])),
                      guidance.resample_labels(labels[1], *(int(v) for v in style_img.shape[-2:])))
    preserve_color = config.optimization.preserve_color
    if preserve_color == "match":               # once per run, on the full-size images: a coarse-to-fine run halves the matched style
        style_img = color.match_style_to_content(style_img, content_img)
        extra_styles = [color.match_style_to_content(img, content_img) for img in extra_styles]
    if auto_mask:                               # the images the run sees; None: no split that holds, the run is unguided
        space_kw = ({"precision": config.hardware.precision} if getattr(oc, "auto_mask_space", "color") == "features" else {})
        labels = segment.auto_guidance(content_img, style_img, oc, oc.pyramid_levels, **space_kw)
    if extra_styles:                            # (one style: the tensor itself, as always)
        style_img = [style_img, *extra_styles]
    label_kw = {"content_labels": labels[0], "style_labels": labels[1]} if labels is not None else {}
    coarse_to_fine = config.optimization.pyramid_levels > 1
    if not coarse_to_fine:
        with _SETUP_LOCK:
            runtime.setup_random_seed(config.optimization.seed)
            model, input_img, optimizer = core_model.prepare_model_and_input(
                content_img, style_img, device, config.optimization, precision=config.hardware.precision, **label_kw)

    output_path = runtime.setup_output_directory(config.output.output)
    content_name, style_name = Path(paths.content_path).stem, _style_stem(paths) + (output_tag if tag_png else "")
    if output_tag and config.output.log_loss:
        log_path = Path(config.output.log_loss)
        config.output.log_loss = str(log_path.with_name(log_path.stem + output_tag + log_path.suffix))

    if save_masks and labels is not None:
        for stem, lab in ((content_name, labels[0]), (Path(paths.style_path).stem, labels[1])):
            segment.save_label_png(lab, oc.mask_regions, output_path / f"{stem}_mask.png")
            logger.info("Label map saved to: %s", output_path / f"{stem}_mask.png")

    gif_name = None
    if builtin_gif:
        gif_name = f"timelapse_{content_name}_x_{_style_stem(paths)}{output_tag}.gif"
        gif_collector = gif_output.DeviceGifCollector(
            output_path / gif_name, config.video.fps, int(input_img.shape[-2]), int(input_img.shape[-1]), gif_frames,
            colors=gif_colors, dither=gif_dither, device=device)

    video_name = None
    if builtin_mjpeg:
        video_name = f"timelapse_{content_name}_x_{_style_stem(paths)}{output_tag}.avi"
        video_writer = mjpeg_output.DeviceMjpegWriter(
            output_path / video_name, config.video.fps, int(input_img.shape[-2]), int(input_img.shape[-1]), video_frames,
            quality=config.video.quality, device=device,
            info=mjpeg_output.video_info(config.video.metadata_title, config.video.metadata_artist))

    if coarse_to_fine:                          # (refuses frame sinks: frames would change size between levels)
        input_img, loss_metrics, elapsed = pyramid.run_pyramid(
            content_img, style_img, device, config, video_writer=video_writer, gif_collector=gif_collector,
            seed=config.optimization.seed, setup_lock=_SETUP_LOCK, **label_kw)
    else:
        runner = optimization.OptimizationRunner(model, input_img, config, optimizer=optimizer,
                                                 video_writer=video_writer, gif_collector=gif_collector)
        input_img, loss_metrics, elapsed = runner.run()
    for sink in (video_writer, gif_collector):
        if sink is not None:
            sink.close()
    if preserve_color == "luma":                # the final full-size image only: frames showed the un-swapped one
        input_img = color.transfer_luma(input_img, content_img, normalize=normalize)

    runtime.save_outputs(input_img, loss_metrics, output_path, elapsed, SaveOptions(
        content_name=content_name, style_name=style_name, normalize=normalize,
        video_name=video_name, video_created=video_writer is not None, gif_name=gif_name, gif_created=gif_collector is not None,
        plot_losses=config.output.plot_losses),
        **({"plot_name": f"loss_plot{output_tag}.png"} if output_tag else {}))      # (untagged: the reference's call, runtime/output.py:55)
    return input_img.detach().clamp(0, 1)


def style_transfer_batch(pairs: list[InputPaths], config, *, images_per_gpu: int | None = None) -> list[torch.Tensor]:
    """Several INDEPENDENT content/style pairs, one process per GPU (launch with torchrun).

    Not a tensor batch - ``gram_matrix`` folds a batch dimension into channels (reference
    core_model.py:56-57) - but N replicas of the single-image path: rank r runs pairs r, r + world, ...
    each with its own model targets and L-BFGS state, writes their PNGs, and one all-gather at the end
    hands every rank the full ordered list of result images (they must share one size).
    ``images_per_gpu`` of a rank's pairs run at the same time, each on its own stream (opt-in: default 1, or
    ``STV_IMAGES_PER_GPU``; ``parallel.images_in_flight``) - same results, one image's optimizer update overlaps
    another's closure, at that many times the device memory.  Every pair works on its own copy of ``config``; with
    more than one pair the loss CSV (``output.log_loss``) and the loss plot carry the pair's index, and so does the PNG
    of a pair whose content/style names occur more than once in ``pairs`` - no two pairs write one file.
    """
    import copy  # noqa: PLC0415

    from . import parallel  # noqa: PLC0415

    _rank, local_rank, _world = parallel.init_distributed()
    if torch.cuda.is_available():              # "cuda" in the config then means this rank's GPU
        torch.cuda.set_device(local_rank % torch.cuda.device_count())

    stems = [(Path(p.content_path).stem, _style_stem(p)) for p in pairs]

    def one(index: int, paths: InputPaths) -> torch.Tensor:
        tag = f"_{index:03d}" if len(pairs) > 1 else ""
        # (a pair whose names are unique in the batch keeps the reference's PNG name, runtime/output.py:46-52)
        return style_transfer(paths, copy.deepcopy(config), output_tag=tag, tag_png=stems.count(stems[index]) > 1).contiguous()
    return parallel.run_sharded(list(pairs), one, concurrent=images_per_gpu)
