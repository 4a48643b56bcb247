"""``style-visualizer`` command line: same flags and override rules as reference cli.py:26-354.

Options that only have meaning for presentation features outside this build (comparison grids)
are accepted and reported as unavailable.  Additions: ``--precision {fp32,bf16,bf16x3}``, ``--tv-w``,
``--pyramid-levels`` / ``--pyramid-steps``, ``--preserve-color {off,match,luma}``, ``--content-size`` / ``--style-size`` /
``--style-scale`` / ``--resize-filter {bilinear,bicubic,lanczos}``, ``--style-also`` / ``--style-blend`` /
``--style-layer-weights``, ``--lap-w`` / ``--lap-pool``, ``--content-mask`` / ``--style-mask`` / ``--mask-regions`` /
``--region-weights``, ``--auto-mask`` / ``--auto-mask-cell`` / ``--auto-mask-space`` / ``--auto-mask-layer`` / ``--save-masks`` (``--content`` and ``--style`` stay exact options: argparse prefers an exact match to a prefix).
"""
from __future__ import annotations

import argparse
import sys

from . import config as stv_config
from . import main as stv_main
from . import guidance, style_mix
from .config_defaults import DEFAULT_LOG_EVERY
from .constants import VIDEO_QUALITY_MAX, VIDEO_QUALITY_MIN
from .logging_utils import logger
from .type_defs import InputPaths

S = argparse.SUPPRESS


def build_arg_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        description="Neural Style Transfer on AMD MI355X (hand-written HIP kernels)",
        formatter_class=argparse.RawDescriptionHelpFormatter,
        epilog="Normalization is enabled by default. Use --no-normalize to disable it")
    req = p.add_argument_group("required arguments")
    req.add_argument("--content", type=str, help="Path to content image")
    req.add_argument("--style", type=str, help="Path to style image")
    req.add_argument("--style-also", type=str, nargs="+", default=S, metavar="PATH",
                     help="Further style images, blended with --style (at most 8 style images in all)")

    out = p.add_argument_group("output")
    out.add_argument("--output", type=str, default=S, help="Output directory")
    out.add_argument("--no-plot", action="store_true", help="Disable loss plotting")
    out.add_argument("--log-loss", type=str, help="CSV file for loss metrics (disables the loss plot)")
    out.add_argument("--log-every", type=int, default=DEFAULT_LOG_EVERY, help="Log losses every N steps")
    out.add_argument("--save-masks", action="store_true",
                     help="Write the two label maps of a guided run (from mask files or --auto-mask) as grey PNGs, at run size")
    out.add_argument("--compare-inputs", action="store_true", help="(not available in this build)")
    out.add_argument("--compare-result", action="store_true", help="(not available in this build)")

    opt = p.add_argument_group("optimization")
    opt.add_argument("--steps", type=int, default=S, help="Number of optimization steps")
    opt.add_argument("--style-w", type=float, default=S, help="Style weight")
    opt.add_argument("--content-w", type=float, default=S, help="Content weight")
    opt.add_argument("--tv-w", type=float, default=S, help="Total-variation weight (0 = off, the default)")
    opt.add_argument("--lap-w", type=float, default=S,
                     help="Weight of the Laplacian loss against the content image (0 = off, the default)")
    opt.add_argument("--lap-pool", type=str,
                     help="Comma-separated pool sizes of the Laplacian loss, powers of two from 1 to 32 (default: 4)")
    opt.add_argument("--pyramid-levels", type=int, default=S,
                     help="Coarse-to-fine levels, each twice the size of the one before (1 = off, the default)")
    opt.add_argument("--pyramid-steps", type=str,
                     help="Comma-separated steps per pyramid level, coarsest first (default: --steps split evenly)")
    opt.add_argument("--preserve-color", choices=["off", "match", "luma"], default=S,
                     help="Keep the content image's colours: match = give the style image the content's colour mean and "
                          "covariance before the run, luma = keep only the result's luminance (off = the default)")
    opt.add_argument("--content-size", type=int, default=S,
                     help="Resize the content image so that its longer side has this many pixels (0 = keep, the default)")
    opt.add_argument("--style-size", type=int, default=S,
                     help="Resize the style image so that its longer side has this many pixels (0 = keep, the default)")
    opt.add_argument("--style-scale", type=float, default=S,
                     help="Resize the style image so that its longer side is this multiple of the content's "
                          "(0 = keep, the default; not together with --style-size)")
    opt.add_argument("--resize-filter", choices=["bilinear", "bicubic", "lanczos"], default=S,
                     help="Filter of the three resize options, antialiased on a downscale (default: lanczos)")
    opt.add_argument("--style-blend", type=str,
                     help="Comma-separated blend weights of the style images, --style's first (normalised to sum 1; "
                          "default: equal weights)")
    opt.add_argument("--style-layer-weights", type=str,
                     help="Comma-separated weights of the style layers, paired by position with --style-layers "
                          "(default: every layer counts 1)")
    opt.add_argument("--content-mask", type=str, default=S, metavar="PATH",
                     help="Grey mask of the content image (same pixel size): spatial guidance, together with --style-mask")
    opt.add_argument("--style-mask", type=str, default=S, metavar="PATH",
                     help="Grey mask of the style image (same pixel size): region r of the content takes region r of the style")
    opt.add_argument("--mask-regions", type=int, default=S,
                     help="Regions of the two masks, 2 to 4 uniform grey bands (default: 2, black and white)")
    opt.add_argument("--region-weights", type=str,
                     help="Comma-separated weights of the regions (default: every region counts 1; 0 leaves a region unstyled)")
    opt.add_argument("--auto-mask", action="store_true",
                     help="Spatial guidance without mask files: segment both images jointly into --mask-regions colour regions")
    opt.add_argument("--auto-mask-cell", type=int, choices=[1, 2, 4, 8, 16, 32], default=S,
                     help="Cell size of the --auto-mask segmentation in pixels (default: 8)")
    opt.add_argument("--auto-mask-space", choices=["color", "features"], default=S,
                     help="Where --auto-mask clusters: color (box means of the colours, the default) or features (one VGG layer)")
    opt.add_argument("--auto-mask-layer", type=int, default=S,
                     help="VGG layer index whose output --auto-mask-space features clusters (default: 10, conv3_1)")
    opt.add_argument("--pooling", choices=["max", "avg"], default=S,
                     help="Pooling layers of the feature stack: max (VGG as trained, the default) or avg (the mean of each 2x2 window)")
    opt.add_argument("--lr", type=float, default=S, help="Learning rate")
    opt.add_argument("--init-method", choices=["random", "white", "content"], default=S, help="Initialization method")
    opt.add_argument("--seed", type=int, default=S, help="Random seed")
    opt.add_argument("--no-normalize", action="store_true", help="Disable VGG19 normalization")
    opt.add_argument("--style-layers", type=str, help="Comma-separated VGG19 layer indices for style loss")
    opt.add_argument("--content-layers", type=str, help="Comma-separated VGG19 layer indices for content loss")

    vid = p.add_argument_group("video")
    vid.add_argument("--save-every", type=int, default=S, help="Save a frame every N steps")
    vid.add_argument("--fps", type=int, default=S, help="Frames per second for video")
    vid.add_argument("--quality", type=int, default=S, help="Video quality 1-10")
    vid.add_argument("--no-video", action="store_true", help="Disable video creation")
    vid.add_argument("--final-only", action="store_true", help="Only save the final image")
    vid.add_argument("--no-intro", action="store_true", help="Disable the intro segment")
    vid.add_argument("--intro-duration", type=float, default=S)
    vid.add_argument("--no-final-frame-compare", dest="final_frame_compare", action="store_false", default=S)
    vid.add_argument("--outro-duration", type=float, default=S)
    vid.add_argument("--metadata-title", type=str, default=S)
    vid.add_argument("--metadata-artist", type=str, default=S)
    vid.add_argument("--gif", dest="create_gif", action="store_true", default=S)
    vid.add_argument("--no-gif", dest="create_gif", action="store_false", default=S)
    vid.add_argument("--gif-include-intro", dest="gif_include_intro", action="store_true", default=S)
    vid.add_argument("--gif-include-outro", dest="gif_include_outro", action="store_true", default=S)
    vid.add_argument("--gif-colors", type=int, default=S,
                     help="Entries of the timelapse GIF's one palette, 2 to 256 (default: 256)")
    vid.add_argument("--gif-dither", choices=["none", "ordered"], default=S,
                     help="Dither of the timelapse GIF: ordered (8x8 Bayer, the default) or none")
    vid.add_argument("--video-mode", choices=["realtime", "postprocess"], default=S)
    vid.add_argument("--video-format", choices=["mp4", "mjpeg"], default=S,
                     help="Timelapse video: mp4 (the default; not encoded by this build) or mjpeg (Motion-JPEG in an AVI file, built in)")

    hw = p.add_argument_group("hardware")
    hw.add_argument("--device", type=str, default=S, help="Device to run on (cuda = MI355X under ROCm)")
    hw.add_argument("--precision", choices=["fp32", "bf16", "bf16x3"], default=S,
                    help="Activation storage: fp32 (parity mode), bf16 (fp32 accumulate) or bf16x3 "
                         "(fp32 storage, conv/Gram products from split bf16 operands)")

    cfg = p.add_argument_group("configuration")
    cfg.add_argument("--config", type=str, help="Path to config.toml")
    cfg.add_argument("--validate-config-only", action="store_true", help="Validate the config file and exit")
    return p


def log_parameters(paths: InputPaths, cfg: stv_config.StyleTransferConfig,
                   args: argparse.Namespace | None = None) -> None:
    """One INFO line per setting, "Label: value" (the labels of reference cli.py:247-300, which its tests grep for;
    plus the two hardware settings this build adds)."""
    def yes(flag: bool) -> str:
        return "Yes" if flag else "No"

    def on(flag: bool) -> str:
        return "Enabled" if flag else "Disabled"
    o, v = cfg.optimization, cfg.video
    rows: list[tuple[str, object]] = [("Content image loaded", paths.content_path), ("Style image loaded", paths.style_path)]
    if getattr(args, "config", None):
        rows.append(("Loaded config from", args.config))
    rows += [
        ("Output Directory", cfg.output.output), ("Steps", o.steps), ("Save Every", v.save_every),
        ("Style Weight", f"{o.style_w:g}"), ("Content Weight", f"{o.content_w:g}"), ("Learning Rate", f"{o.lr:g}"),
        ("Style Layers", o.style_layers), ("Content Layers", o.content_layers),
        ("FPS for Timelapse Video", v.fps), ("Video Quality", f"{v.quality} ({VIDEO_QUALITY_MIN}-{VIDEO_QUALITY_MAX} scale)"),
        ("Initialization Method", o.init_method), ("Normalization", on(o.normalize)),
        ("Video Creation", on(v.create_video)), ("Intro Duration (s)", f"{v.intro_duration_seconds:.2f}"),
        ("Outro Duration (s)", f"{v.outro_duration_seconds:.2f}"),
        ("GIF Export", on(v.create_gif)), ("GIF Intro Included", yes(v.gif_include_intro)),
        ("GIF Outro Included", yes(v.gif_include_outro)), ("Video Mode", v.mode),
        ("Loss Plotting", on(cfg.output.plot_losses)), ("Random Seed", o.seed),
        ("Device", cfg.hardware.device), ("Precision", cfg.hardware.precision),
    ]
    if o.tv_w > 0:
        rows.insert(next(i for i, (label, _) in enumerate(rows) if label == "Content Weight") + 1,
                    ("Total Variation Weight", f"{o.tv_w:g}"))
    if o.lap_w > 0:
        behind = "Total Variation Weight" if o.tv_w > 0 else "Content Weight"
        at = next(i for i, (label, _) in enumerate(rows) if label == behind) + 1
        rows[at:at] = [("Laplacian Weight", f"{o.lap_w:g}"), ("Laplacian Pool Sizes", ",".join(str(p) for p in o.lap_pools))]
    if o.pooling != "max":
        rows.insert(next(i for i, (label, _) in enumerate(rows) if label == "Content Layers") + 1, ("Pooling", o.pooling))
    if o.pyramid_levels > 1:
        at = next(i for i, (label, _) in enumerate(rows) if label == "Steps") + 1
        rows[at:at] = [("Pyramid Levels", o.pyramid_levels),
                       ("Pyramid Steps", o.pyramid_steps if o.pyramid_steps else "even split of Steps")]
    if o.preserve_color != "off":
        rows.insert(next(i for i, (label, _) in enumerate(rows) if label == "Initialization Method") + 1,
                    ("Preserve Color", o.preserve_color))
    resized = [("Content Size", o.content_size)] if o.content_size > 0 else []
    resized += [("Style Size", o.style_size)] if o.style_size > 0 else []
    resized += [("Style Scale", f"{o.style_scale:g}")] if o.style_scale > 0 else []
    if resized:
        at = next(i for i, (label, _) in enumerate(rows) if label == "Style image loaded") + 1
        rows[at:at] = [*resized, ("Resize Filter", o.resize_filter)]
    mixed = [("Style images", list(paths.style_paths))] if paths.extra_style_paths else []
    if paths.extra_style_paths or o.style_blend is not None:
        blend = style_mix.blend_weights(o.style_blend, len(paths.style_paths))
        mixed.append(("Style Blend Weights (normalised)", [float(b) for b in blend]))
    if mixed:
        at = next(i for i, (label, _) in enumerate(rows) if label == "Style image loaded") + 1
        rows[at:at] = mixed
    if o.style_layer_weights is not None:
        rows.insert(next(i for i, (label, _) in enumerate(rows) if label == "Style Layers") + 1,
                    ("Style Layer Weights", o.style_layer_weights))
    if paths.content_mask_path or paths.style_mask_path:
        weights = guidance.check_region_weights(o.region_weights, o.mask_regions)
        at = next(i for i, (label, _) in enumerate(rows) if label == "Style image loaded") + 1
        rows[at:at] = [("Content mask", paths.content_mask_path), ("Style mask", paths.style_mask_path),
                       ("Mask Regions", o.mask_regions), ("Region Weights", [float(w) for w in weights])]
    if o.auto_mask:
        at = next(i for i, (label, _) in enumerate(rows) if label == "Style image loaded") + 1
        rows[at:at] = [("Automatic Masks", "Enabled"), ("Mask Regions", o.mask_regions), ("Automatic Mask Cell", o.auto_mask_cell)]
        if getattr(o, "auto_mask_space", "color") == "features":      # (the cell size is unused there: the layer's grid is the grid)
            rows[at + 2:at + 3] = [("Automatic Mask Space", o.auto_mask_space), ("Automatic Mask Layer", o.auto_mask_layer)]
    if v.create_gif:
        at = next(i for i, (label, _) in enumerate(rows) if label == "GIF Outro Included") + 1
        rows[at:at] = [("GIF Colors", v.gif_colors), ("GIF Dither", v.gif_dither)]
    if v.format != "mp4":
        rows.insert(next(i for i, (label, _) in enumerate(rows) if label == "Video Creation") + 1, ("Video Format", v.format))
    if cfg.output.save_masks:
        rows.insert(next(i for i, (label, _) in enumerate(rows) if label == "Output Directory") + 1, ("Save Masks", "Yes"))
    for label, value in rows:
        logger.info("%s: %s", label, value)


def parse_int_list(s: str | list[int]) -> list[int]:
    """``"0,1,2"`` or a list of ints -> list of ints (reference cli.py:303-314 re-exports config's helper)."""
    return stv_config.parse_int_list(s)


def run_from_args(args: argparse.Namespace) -> None:
    base_cfg = None
    if args.config:
        base_cfg = stv_config.ConfigLoader.load(args.config)
        if args.validate_config_only:
            logger.info("Config %s validated successfully.", args.config)
            sys.exit(0)
    cfg = stv_config.build_config_from_cli(vars(args), base_config=base_cfg)
    paths = InputPaths(content_path=args.content, style_path=args.style,
                       extra_style_paths=tuple(getattr(args, "style_also", ())),
                       content_mask_path=getattr(args, "content_mask", None), style_mask_path=getattr(args, "style_mask", None))
    log_parameters(paths, cfg, args)
    stv_main.style_transfer(paths, cfg)
    if args.compare_inputs or args.compare_result:
        logger.warning("Comparison grids are a presentation feature outside this build; skipped.")


def main(argv: list[str] | None = None) -> None:
    parser = build_arg_parser()
    args = parser.parse_args(argv)
    if not args.validate_config_only and (not args.content or not args.style):
        parser.error("the following arguments are required: --content, --style")
    run_from_args(args)


if __name__ == "__main__":  # pragma: no cover
    main()
