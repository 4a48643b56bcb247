"""Configuration schema, TOML loader and CLI override rules.

Field names, bounds and override precedence follow reference config.py:53-309
so existing ``config.toml`` files and CLI invocations keep working.  The
additions are ``hardware.precision`` ("fp32" parity mode | "bf16" storage | "bf16x3" fp32 storage, split-bf16 products),
``optimization.tv_w`` (weight of the total-variation regulariser, 0 = off), ``optimization.pyramid_levels`` /
``optimization.pyramid_steps`` (coarse-to-fine runs: levels, and optionally the steps of each, coarsest first) and
``optimization.preserve_color`` ("off" | "match" | "luma": keep the content image's colours, ``color.py``) and
``optimization.content_size`` / ``style_size`` / ``style_scale`` / ``resize_filter`` (resize the inputs on the device before
the run, ``resize.py``; 0 = keep the file's size) and ``optimization.style_blend`` / ``style_layer_weights`` (blend weights of
several style images, a weight per style layer, ``style_mix.py``; ``None`` = not set) and ``optimization.lap_w`` /
``lap_pools`` (weight and pool sizes of the Laplacian loss against the content image, 0 = off) and ``optimization.mask_regions``
/ ``region_weights`` (regions of the two masks of a guided run and their weights, ``guidance.py``; read only with masks) and
``optimization.pooling`` ("max" | "avg": the pooling layers of the feature stack, "max" = VGG as trained) and
``optimization.auto_mask`` / ``auto_mask_cell`` (the two label maps from a joint colour segmentation of the two images instead
of mask files, and its cell size, ``segment.py``) / ``auto_mask_space`` / ``auto_mask_layer`` ("color" | "features": cluster box
means of the colours, or the activations of one VGG layer, index ``auto_mask_layer``) and ``output.save_masks`` (write the label maps of a guided run as PNGs) and ``video.gif_colors`` /
``gif_dither`` (entries of the timelapse GIF's one palette, 2..256, and its dither, "ordered" | "none", ``gif.py``) and
``video.format`` ("mp4" | "mjpeg": the timelapse video's container; only "mjpeg" has an encoder in this build, ``mjpeg.py``).
"""
from __future__ import annotations

from collections.abc import Callable, Mapping
from pathlib import Path
from typing import Any

from pydantic import BaseModel, Field, field_validator

from . import config_defaults as d
from .constants import VIDEO_QUALITY_MAX, VIDEO_QUALITY_MIN
from .logging_utils import logger
from .type_defs import AutoMaskSpace, GifDither, InitMethod, Pooling, Precision, PreserveColor, ResizeFilter, VideoFormat, VideoMode


class OptimizationConfig(BaseModel):
    """Optimisation settings."""

    steps: int = Field(d.DEFAULT_STEPS, ge=1)
    style_w: float = Field(d.DEFAULT_STYLE_WEIGHT, ge=0)
    content_w: float = Field(d.DEFAULT_CONTENT_WEIGHT, ge=0)
    tv_w: float = Field(d.DEFAULT_TV_WEIGHT, ge=0)
    lap_w: float = Field(d.DEFAULT_LAP_WEIGHT, ge=0, allow_inf_nan=False)
    lap_pools: list[int] = Field(default_factory=lambda: list(d.DEFAULT_LAP_POOLS))
    pyramid_levels: int = Field(d.DEFAULT_PYRAMID_LEVELS, ge=1, le=6)
    pyramid_steps: list[int] | None = d.DEFAULT_PYRAMID_STEPS
    preserve_color: PreserveColor = Field(d.DEFAULT_PRESERVE_COLOR)
    content_size: int = Field(d.DEFAULT_CONTENT_SIZE, ge=0)
    style_size: int = Field(d.DEFAULT_STYLE_SIZE, ge=0)
    style_scale: float = Field(d.DEFAULT_STYLE_SCALE, ge=0)
    resize_filter: ResizeFilter = Field(d.DEFAULT_RESIZE_FILTER)
    style_blend: list[float] | None = d.DEFAULT_STYLE_BLEND
    style_layer_weights: list[float] | None = d.DEFAULT_STYLE_LAYER_WEIGHTS
    mask_regions: int = Field(d.DEFAULT_MASK_REGIONS, ge=2, le=4)
    region_weights: list[float] | None = d.DEFAULT_REGION_WEIGHTS
    auto_mask: bool = d.DEFAULT_AUTO_MASK
    auto_mask_cell: int = Field(d.DEFAULT_AUTO_MASK_CELL)
    auto_mask_space: AutoMaskSpace = Field(d.DEFAULT_AUTO_MASK_SPACE)
    auto_mask_layer: int = Field(d.DEFAULT_AUTO_MASK_LAYER, ge=0)
    pooling: Pooling = Field(d.DEFAULT_POOLING)
    lr: float = Field(d.DEFAULT_LEARNING_RATE, gt=0)
    init_method: InitMethod = Field(d.DEFAULT_INIT_METHOD)
    seed: int = Field(d.DEFAULT_SEED, ge=0)
    normalize: bool = d.DEFAULT_NORMALIZE
    lbfgs_max_iter: int = Field(d.DEFAULT_LBFGS_MAX_ITER, ge=1)
    lbfgs_max_eval: int = Field(d.DEFAULT_LBFGS_MAX_EVAL, ge=1)
    style_layers: list[int] = Field(default_factory=lambda: list(d.DEFAULT_STYLE_LAYERS))
    content_layers: list[int] = Field(default_factory=lambda: list(d.DEFAULT_CONTENT_LAYERS))

    @field_validator("lap_pools")
    @classmethod
    def _lap_pools_allowed(cls, value: list[int]) -> list[int]:
        allowed = (1, 2, 4, 8, 16, 32)
        if not 1 <= len(value) <= 4 or len(set(value)) != len(value) or any(v not in allowed for v in value):
            msg = f"lap_pools takes one to four different pool sizes out of {list(allowed)}, got {value}"
            raise ValueError(msg)
        return value

    @field_validator("auto_mask_cell")
    @classmethod
    def _auto_mask_cell_allowed(cls, value: int) -> int:
        allowed = (1, 2, 4, 8, 16, 32)
        if value not in allowed:
            msg = f"auto_mask_cell must be one of {list(allowed)}, got {value}"
            raise ValueError(msg)
        return value


class VideoConfig(BaseModel):
    """Timelapse / GIF output settings."""

    save_every: int = Field(d.DEFAULT_SAVE_EVERY, ge=1)
    fps: int = Field(d.DEFAULT_FPS, ge=1, le=60)
    quality: int = Field(d.DEFAULT_VIDEO_QUALITY, ge=VIDEO_QUALITY_MIN, le=VIDEO_QUALITY_MAX)
    create_video: bool = d.DEFAULT_CREATE_VIDEO
    final_only: bool = d.DEFAULT_FINAL_ONLY
    intro_enabled: bool = d.DEFAULT_VIDEO_INTRO_ENABLED
    intro_duration_seconds: float = Field(d.DEFAULT_VIDEO_INTRO_DURATION, ge=0.0)
    metadata_title: str | None = None
    metadata_artist: str | None = None
    final_frame_compare: bool = d.DEFAULT_VIDEO_FINAL_FRAME_COMPARE
    outro_duration_seconds: float = Field(d.DEFAULT_VIDEO_OUTRO_DURATION, ge=0.0)
    mode: VideoMode = Field(d.DEFAULT_VIDEO_MODE)
    create_gif: bool = d.DEFAULT_CREATE_GIF
    gif_include_intro: bool = d.DEFAULT_GIF_INCLUDE_INTRO
    gif_include_outro: bool = d.DEFAULT_GIF_INCLUDE_OUTRO
    gif_colors: int = Field(d.DEFAULT_GIF_COLORS, ge=2, le=256)
    gif_dither: GifDither = Field(d.DEFAULT_GIF_DITHER)
    format: VideoFormat = Field(d.DEFAULT_VIDEO_FORMAT)
    mode_override: bool = Field(default=False, exclude=True, repr=False)


class HardwareConfig(BaseModel):
    """Device selection (+ activation storage precision on MI355X)."""

    device: str = Field(d.DEFAULT_DEVICE)
    precision: Precision = Field(d.DEFAULT_PRECISION)


class OutputConfig(BaseModel):
    """Output directory and loss logging."""

    output: str = Field(d.DEFAULT_OUTPUT_DIR)
    log_every: int = Field(d.DEFAULT_LOG_EVERY, ge=1)
    log_loss: str | None = None
    plot_losses: bool = True
    save_masks: bool = d.DEFAULT_SAVE_MASKS


class StyleTransferConfig(BaseModel):
    """Root object mirroring the sections of ``config.toml``."""

    output: OutputConfig = Field(default_factory=lambda: OutputConfig.model_validate({}))
    optimization: OptimizationConfig = Field(default_factory=lambda: OptimizationConfig.model_validate({}))
    video: VideoConfig = Field(default_factory=lambda: VideoConfig.model_validate({}))
    hardware: HardwareConfig = Field(default_factory=lambda: HardwareConfig.model_validate({}))


def _read_toml(path: Path) -> dict:
    try:
        import tomllib as toml_reader  # py >= 3.11
    except ModuleNotFoundError:
        try:
            import tomli as toml_reader
        except ModuleNotFoundError:
            import tomlkit
            with path.open("r", encoding="utf-8") as f:
                return dict(tomlkit.load(f))
    with path.open("rb") as f:
        return toml_reader.load(f)


class ConfigLoader:
    """TOML -> validated ``StyleTransferConfig``; missing sections fall back to defaults."""

    @staticmethod
    def load(path: str) -> StyleTransferConfig:
        config_path = Path(path)
        if not config_path.is_file():
            msg = f"Config file not found: {path}"
            raise FileNotFoundError(msg)
        return StyleTransferConfig.model_validate(_read_toml(config_path))


def parse_int_list(value: str | list[int]) -> list[int]:
    """``"0,5,10"`` -> ``[0, 5, 10]`` (lists pass through)."""
    if isinstance(value, list):
        return value
    return [int(v) for v in value.split(",")]


def parse_float_list(value: str | list[float]) -> list[float]:
    """``"0.7,0.3"`` -> ``[0.7, 0.3]`` (lists pass through)."""
    if isinstance(value, list):
        return value
    return [float(v) for v in value.split(",")]


# CLI key -> (section, attribute) for plain "present in args => overwrite" options
_DIRECT = {
    "output": ("output", "output"), "log_every": ("output", "log_every"), "log_loss": ("output", "log_loss"),
    "steps": ("optimization", "steps"), "style_w": ("optimization", "style_w"),
    "content_w": ("optimization", "content_w"), "tv_w": ("optimization", "tv_w"), "lap_w": ("optimization", "lap_w"),
    "mask_regions": ("optimization", "mask_regions"), "auto_mask_cell": ("optimization", "auto_mask_cell"),
    "auto_mask_space": ("optimization", "auto_mask_space"), "auto_mask_layer": ("optimization", "auto_mask_layer"),
    "pooling": ("optimization", "pooling"),
    "lr": ("optimization", "lr"),
    "pyramid_levels": ("optimization", "pyramid_levels"), "preserve_color": ("optimization", "preserve_color"),
    "content_size": ("optimization", "content_size"), "style_size": ("optimization", "style_size"),
    "style_scale": ("optimization", "style_scale"), "resize_filter": ("optimization", "resize_filter"),
    "init_method": ("optimization", "init_method"), "seed": ("optimization", "seed"),
    "save_every": ("video", "save_every"), "fps": ("video", "fps"), "quality": ("video", "quality"),
    "metadata_title": ("video", "metadata_title"), "metadata_artist": ("video", "metadata_artist"),
    "create_gif": ("video", "create_gif"), "gif_include_intro": ("video", "gif_include_intro"),
    "gif_include_outro": ("video", "gif_include_outro"),
    "gif_colors": ("video", "gif_colors"), "gif_dither": ("video", "gif_dither"), "video_format": ("video", "format"),
    "final_frame_compare": ("video", "final_frame_compare"),
    "device": ("hardware", "device"), "precision": ("hardware", "precision"),
}
# truthy flag -> (section, attribute, value)
_FLAGS = {
    "no_plot": ("output", "plot_losses", False), "no_normalize": ("optimization", "normalize", False),
    "no_video": ("video", "create_video", False), "no_intro": ("video", "intro_enabled", False),
    "final_only": ("video", "final_only", True),
    "auto_mask": ("optimization", "auto_mask", True), "save_masks": ("output", "save_masks", True),
}


def build_config_from_cli(
    cli_args: Mapping[str, Any],
    *,
    loader: Callable[[str], StyleTransferConfig] | None = None,
    base_config: StyleTransferConfig | None = None,
) -> StyleTransferConfig:
    """Apply CLI overrides on top of a TOML/base/default config (reference config.py:181-207)."""
    args = dict(cli_args)
    if base_config is not None:
        cfg = base_config.model_copy(deep=True)
    elif args.get("config"):
        cfg = (loader or ConfigLoader.load)(args["config"])
    else:
        cfg = StyleTransferConfig.model_validate({})

    _apply_output_overrides(cfg, args)
    _apply_optimization_overrides(cfg, args)
    _apply_video_overrides(cfg, args)
    _apply_hardware_overrides(cfg, args)
    _enforce_csv_plot_rule(cfg)
    return cfg


def _apply_section(cfg: StyleTransferConfig, args: Mapping[str, Any], section: str) -> None:
    """The table-driven part of one section: keys present in ``args`` overwrite, truthy flags set their value."""
    for key, (sec, attr) in _DIRECT.items():
        if sec == section and key in args:
            setattr(getattr(cfg, sec), attr, args[key])
    for key, (sec, attr, value) in _FLAGS.items():
        if sec == section and args.get(key):
            setattr(getattr(cfg, sec), attr, value)


# Per-section entry points under the names the reference's own tests reach for (config.py:210-299 there).
def _apply_output_overrides(cfg: StyleTransferConfig, args: Mapping[str, Any]) -> None:
    _apply_section(cfg, args, "output")


def _apply_optimization_overrides(cfg: StyleTransferConfig, args: Mapping[str, Any]) -> None:
    _apply_section(cfg, args, "optimization")
    if args.get("style_layers"):
        cfg.optimization.style_layers = parse_int_list(args["style_layers"])
    if args.get("content_layers"):
        cfg.optimization.content_layers = parse_int_list(args["content_layers"])
    if args.get("pyramid_steps"):
        cfg.optimization.pyramid_steps = parse_int_list(args["pyramid_steps"])
    if args.get("lap_pool"):
        cfg.optimization.lap_pools = OptimizationConfig(lap_pools=parse_int_list(args["lap_pool"])).lap_pools
    if args.get("region_weights"):
        cfg.optimization.region_weights = parse_float_list(args["region_weights"])
    if args.get("style_blend"):
        cfg.optimization.style_blend = parse_float_list(args["style_blend"])
    if args.get("style_layer_weights"):
        cfg.optimization.style_layer_weights = parse_float_list(args["style_layer_weights"])


def _apply_video_overrides(cfg: StyleTransferConfig, args: Mapping[str, Any]) -> None:
    _apply_section(cfg, args, "video")
    if "gif_colors" in args or "gif_dither" in args:            # (assignments are not validated: the field rules again)
        VideoConfig.model_validate({"gif_colors": cfg.video.gif_colors, "gif_dither": cfg.video.gif_dither})
    if "video_format" in args:
        VideoConfig.model_validate({"format": cfg.video.format})
    for key, attr in (("intro_duration", "intro_duration_seconds"), ("outro_duration", "outro_duration_seconds")):
        if key in args:
            setattr(cfg.video, attr, max(args[key], 0.0))       # negative durations mean "none"
    if "video_mode" in args:
        cfg.video.mode = args["video_mode"]
        cfg.video.mode_override = True
    # a non-default mode that came from a TOML file / base config counts as an explicit choice too
    if not cfg.video.mode_override and cfg.video.mode != d.DEFAULT_VIDEO_MODE:
        cfg.video.mode_override = True


def _apply_hardware_overrides(cfg: StyleTransferConfig, args: Mapping[str, Any]) -> None:
    _apply_section(cfg, args, "hardware")


def _enforce_csv_plot_rule(cfg: StyleTransferConfig) -> None:
    """CSV logging replaces the loss plot (reference config.py:302-309)."""
    if getattr(cfg.output, "log_loss", None) and cfg.output.plot_losses:
        logger.warning(
            "Loss plotting is disabled because CSV logging is enabled. "
            "Only loss CSV will be created.",
        )
        cfg.output.plot_losses = False
