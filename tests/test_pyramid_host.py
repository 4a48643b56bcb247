"""Coarse-to-fine runs (--pyramid-levels), everything that runs without a GPU: the split of sizes and steps, configuration,
the C ABI's argument checks, the up-front refusals of ``run_pyramid`` (none reaches a kernel), and the driver's
bookkeeping - history, CSV, progress bar, what it builds per level - with the resize replaced by its NumPy twin and the
model by a small autograd module."""
from __future__ import annotations

import csv
import os
import re

import pytest
import torch
from torch import nn

from style_transfer_visualizer_amd import _lib, cli, core_model, ops, pyramid
from style_transfer_visualizer_amd import config as stv_config
from style_transfer_visualizer_amd import config_defaults
from style_transfer_visualizer_amd.constants import MIN_DIMENSION
from tests import resize_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


# ------------------------------------------------------------------------------------------------ sizes and steps
def test_level_shapes():
    assert pyramid.level_shapes(1024, 512, 3) == [(256, 128), (512, 256), (1024, 512)]
    assert pyramid.level_shapes(128, 128, 1) == [(128, 128)]
    assert pyramid.level_shapes(256, 320, 2) == [(128, 160), (256, 320)]


def test_level_steps_even_split_and_remainder():
    assert pyramid.level_steps(9, 3) == [3, 3, 3]
    assert pyramid.level_steps(7, 3) == [3, 2, 2]                 # the remainder goes to the coarsest levels, one each
    assert pyramid.level_steps(500, 3) == [167, 167, 166]
    assert pyramid.level_steps(3, 3) == [1, 1, 1]
    assert pyramid.level_steps(5, 1) == [5]
    for steps, levels in ((7, 3), (500, 3), (11, 6)):
        assert sum(pyramid.level_steps(steps, levels)) == steps


def test_level_steps_refuses_fewer_steps_than_levels():
    with pytest.raises(ValueError, match="2 steps"):
        pyramid.level_steps(2, 3)


def test_level_steps_explicit_list():
    assert pyramid.level_steps(1500, 3, [5, 3, 2]) == [5, 3, 2]   # used as given: the total is their sum
    assert pyramid.level_steps(1, 3, [5, 3, 2]) == [5, 3, 2]
    with pytest.raises(ValueError, match="2 entries for 3"):
        pyramid.level_steps(10, 3, [5, 5])
    with pytest.raises(ValueError, match="at least 1, got 0"):
        pyramid.level_steps(10, 3, [5, 0, 5])


# ------------------------------------------------------------------------------------------------ configuration
def _cli_config(argv):
    args = cli.build_arg_parser().parse_args(argv)
    base = stv_config.ConfigLoader.load(args.config) if args.config else None
    return stv_config.build_config_from_cli(vars(args), base_config=base)


BASE = ["--content", "c.png", "--style", "s.png"]


def test_defaults():
    assert config_defaults.DEFAULT_PYRAMID_LEVELS == 1 and config_defaults.DEFAULT_PYRAMID_STEPS is None
    oc = stv_config.StyleTransferConfig.model_validate({}).optimization
    assert oc.pyramid_levels == 1 and oc.pyramid_steps is None
    oc = _cli_config(BASE).optimization
    assert oc.pyramid_levels == 1 and oc.pyramid_steps is None


def test_cli_and_toml_round_trip(tmp_path):
    oc = _cli_config([*BASE, "--pyramid-levels", "3", "--pyramid-steps", "5,3,2"]).optimization
    assert oc.pyramid_levels == 3 and oc.pyramid_steps == [5, 3, 2]
    toml = tmp_path / "config.toml"
    toml.write_text("[optimization]\npyramid_levels = 2\npyramid_steps = [40, 10]\nsteps = 7\n")
    cfg = stv_config.ConfigLoader.load(str(toml))
    assert (cfg.optimization.pyramid_levels, cfg.optimization.pyramid_steps, cfg.optimization.steps) == (2, [40, 10], 7)
    assert stv_config.StyleTransferConfig.model_validate(cfg.model_dump()).optimization.pyramid_steps == [40, 10]
    assert _cli_config(["--config", str(toml)]).optimization.pyramid_levels == 2                      # TOML alone
    oc = _cli_config(["--config", str(toml), "--pyramid-levels", "3", "--pyramid-steps", "1,2,3"]).optimization
    assert oc.pyramid_levels == 3 and oc.pyramid_steps == [1, 2, 3]                                   # the CLI overrides it
    assert stv_config._DIRECT["pyramid_levels"] == ("optimization", "pyramid_levels")


def test_levels_out_of_range_are_rejected(tmp_path):
    for bad in (0, 7):
        with pytest.raises(ValueError):
            stv_config.OptimizationConfig(pyramid_levels=bad)
    toml = tmp_path / "config.toml"
    toml.write_text("[optimization]\npyramid_levels = 9\n")
    with pytest.raises(ValueError):
        stv_config.ConfigLoader.load(str(toml))


def test_settings_summary_shows_the_rows_only_above_one_level(caplog):
    from style_transfer_visualizer_amd.type_defs import InputPaths
    paths = InputPaths(content_path="c.png", style_path="s.png")
    with caplog.at_level("INFO"):
        cli.log_parameters(paths, _cli_config(BASE))
    assert "Pyramid" not in caplog.text
    caplog.clear()
    with caplog.at_level("INFO"):
        cli.log_parameters(paths, _cli_config([*BASE, "--pyramid-steps", "4"]))      # levels = 1: still not shown
    assert "Pyramid" not in caplog.text
    caplog.clear()
    with caplog.at_level("INFO"):
        cli.log_parameters(paths, _cli_config([*BASE, "--pyramid-levels", "3", "--pyramid-steps", "5,3,2"]))
    assert "Pyramid Levels: 3" in caplog.text and "Pyramid Steps: [5, 3, 2]" in caplog.text
    caplog.clear()
    with caplog.at_level("INFO"):
        cli.log_parameters(paths, _cli_config([*BASE, "--pyramid-levels", "2"]))
    assert "Pyramid Levels: 2" in caplog.text and "Pyramid Steps: even split" in caplog.text


# ---------------------------------------------------------------------------------------------------------- ABI
def test_library_exports_stv_resize2x_and_the_constants_match_the_header():
    lib = _lib.load()
    assert hasattr(lib, "stv_resize2x") and "stv_resize2x" in _lib.SIGNATURES
    assert lib.stv_version() >= 106
    header = open(os.path.join(ROOT, "include", "stv.h")).read()
    modes = re.search(r"enum\s*\{\s*STV_RESIZE_DOWN2\s*=\s*(\d+)\s*,\s*STV_RESIZE_UP2\s*=\s*(\d+)\s*\}", header)
    assert (int(modes.group(1)), int(modes.group(2))) == (_lib.RESIZE_DOWN2, _lib.RESIZE_UP2) == (0, 1)
    assert int(re.search(r"#define\s+STV_RESIZE_THREADS\s+(\d+)", header).group(1)) == _lib.RESIZE_THREADS
    assert int(re.search(r"#define\s+STV_RESIZE_MAX_BLOCKS\s+(\d+)", header).group(1)) == _lib.RESIZE_MAX_BLOCKS
    source = open(os.path.join(ROOT, "style_transfer_visualizer_amd", "csrc", "pointwise.hip")).read()
    assert re.search(r"kResizeThreads\s*=\s*STV_RESIZE_THREADS", source)
    assert re.search(r"kResizeBlocks\s*=\s*STV_RESIZE_MAX_BLOCKS", source)
    # argument checks come before any device work: they can be asked for on a machine without a GPU
    D, U = _lib.RESIZE_DOWN2, _lib.RESIZE_UP2
    assert lib.stv_resize2x(None, 32, 3, 4, 4, D, None) == 1
    assert lib.stv_resize2x(16, None, 3, 4, 4, U, None) == 1
    assert lib.stv_resize2x(16, 16, 3, 4, 4, U, None) == 1                            # x == y
    assert lib.stv_resize2x(16, 32, 0, 4, 4, U, None) == 1
    assert lib.stv_resize2x(16, 32, 3, -1, 4, U, None) == 1
    assert lib.stv_resize2x(16, 32, 3, 4, 0, D, None) == 1
    assert lib.stv_resize2x(16, 32, 3, 5, 4, D, None) == 1                            # odd H with DOWN2
    assert lib.stv_resize2x(16, 32, 3, 4, 7, D, None) == 1                            # odd W with DOWN2
    assert lib.stv_resize2x(16, 32, 3, 4, 4, 2, None) == 1                            # unknown mode
    assert lib.stv_resize2x(16, 32, 2, 16384, 16384, D, None) == 1                    # input: 2 * 2^28 * 4 bytes = 2 GiB
    assert lib.stv_resize2x(16, 32, 2, 8192, 8192, U, None) == 1                      # output: 2 * 2^28 * 4 bytes = 2 GiB


# ------------------------------------------------------------------------------------------- up-front refusals
def _cfg(levels, *, steps=6, pyramid_steps=None, log_loss=None):
    cfg = stv_config.StyleTransferConfig.model_validate({})
    oc = cfg.optimization
    oc.steps, oc.pyramid_levels, oc.pyramid_steps = steps, levels, pyramid_steps
    oc.init_method, oc.normalize = "content", False
    cfg.video.create_video = False
    cfg.output.log_loss, cfg.output.log_every = log_loss, 1
    return cfg


class _Sink:
    def append_data(self, frame):
        pass

    def close(self):
        pass


@pytest.fixture
def no_kernels(monkeypatch):
    """Any resize or model construction is a failure of the test."""
    def forbidden(*a, **k):
        raise AssertionError("an up-front check let the run reach the device")
    monkeypatch.setattr(ops, "resize2x", forbidden)
    monkeypatch.setattr(core_model, "StyleContentModel", forbidden)


def _img(H, W):
    return torch.zeros(1, 3, H, W)


def test_indivisible_content_size_is_refused(no_kernels):
    with pytest.raises(ValueError, match=r"height 258 is not divisible by 4"):
        pyramid.run_pyramid(_img(258, 256), _img(256, 256), CPU, _cfg(3))
    with pytest.raises(ValueError, match=r"width 129 is not divisible by 2"):
        pyramid.run_pyramid(_img(128, 129), _img(256, 256), CPU, _cfg(2))


def test_coarsest_level_below_the_minimum_is_refused(no_kernels):
    assert MIN_DIMENSION == 64
    with pytest.raises(ValueError, match=r"content height 128 is 32 at the coarsest of 3"):
        pyramid.run_pyramid(_img(128, 256), _img(256, 256), CPU, _cfg(3))
    with pytest.raises(ValueError, match=r"content width 64 is 32 at the coarsest of 2"):
        pyramid.run_pyramid(_img(128, 64), _img(256, 256), CPU, _cfg(2))
    # the style image is cropped to a multiple of 4 first: 255 -> 252 -> 63 at the coarsest level
    with pytest.raises(ValueError, match=r"style width 252 is 63 at the coarsest of 3"):
        pyramid.run_pyramid(_img(256, 256), _img(300, 255), CPU, _cfg(3))


def test_frame_sinks_are_refused(no_kernels):
    for kw in ({"video_writer": _Sink()}, {"gif_collector": _Sink()}):
        with pytest.raises(ValueError, match=r"pyramid_levels = 2 cannot be combined with a video or GIF"):
            pyramid.run_pyramid(_img(128, 128), _img(128, 128), CPU, _cfg(2), **kw)
    for attr in ("create_video", "create_gif"):
        cfg = _cfg(2)
        setattr(cfg.video, attr, True)
        with pytest.raises(ValueError, match="cannot be combined with a video or GIF"):
            pyramid.run_pyramid(_img(128, 128), _img(128, 128), CPU, cfg)


def test_step_counts_are_checked_before_any_model(no_kernels):
    with pytest.raises(ValueError, match="1 steps cannot be split over 2"):
        pyramid.run_pyramid(_img(128, 128), _img(128, 128), CPU, _cfg(2, steps=1))
    with pytest.raises(ValueError, match="3 entries for 2"):
        pyramid.run_pyramid(_img(128, 128), _img(128, 128), CPU, _cfg(2, pyramid_steps=[1, 1, 1]))


# ------------------------------------------------------------------------------------------------- the driver
class _Bar:
    def __init__(self):
        self.updates, self.closed = 0, 0

    def update(self, n=1):
        self.updates += n

    def set_postfix(self, d=None, refresh=True, **kw):
        pass

    def close(self):
        self.closed += 1


class _Model(nn.Module):
    """Stands in for StyleContentModel on the CPU (the runner's autograd path): records what it is built and given."""

    built: list = []

    def __init__(self, style_layers, content_layers, precision=None):
        super().__init__()
        type(self).built.append(self)

    def set_targets(self, style, content):
        self.style, self.content = style.detach().clone(), content.detach().clone()

    def forward(self, x):
        return [(x.mean() - self.style.mean()) ** 2], [((x - self.content) ** 2).mean()]


def _twin_resize(x, mode, out=None):
    fn = rr.down2 if mode == _lib.RESIZE_DOWN2 else rr.up2
    return torch.from_numpy(fn(x.detach().numpy()))


@pytest.fixture
def host_driver(monkeypatch):
    _Model.built = []
    monkeypatch.setattr(core_model, "StyleContentModel", _Model)
    monkeypatch.setattr(ops, "resize2x", _twin_resize)


def _images():
    g = torch.Generator().manual_seed(4)
    return torch.rand(1, 3, 256, 256, generator=g), torch.rand(1, 3, 262, 259, generator=g)


def _sgd(x):
    return torch.optim.SGD([x], lr=0.5)


def test_levels_models_history_and_bar(host_driver, caplog):
    content, style = _images()
    bar = _Bar()
    cfg = _cfg(3, steps=7)
    seen = []

    def factory(x):
        seen.append(x)
        return _sgd(x)
    with caplog.at_level("INFO"):
        image, history, elapsed = pyramid.run_pyramid(content, style, CPU, cfg, optimizer_factory=factory, progress_bar=bar)
    assert cfg.optimization.steps == 7                                         # the caller's config is not edited
    assert [tuple(m.content.shape[-2:]) for m in _Model.built] == [(64, 64), (128, 128), (256, 256)]
    assert [tuple(m.style.shape[-2:]) for m in _Model.built] == [(65, 64), (130, 128), (260, 256)]      # 262x259 cropped to 260x256
    assert "Style image cropped from 259x262 to 256x260" in caplog.text
    for k, (size, steps) in enumerate(((64, 3), (128, 2), (256, 2))):
        assert f"Pyramid level {k + 1}/3: {size}x{size}, {steps} steps" in caplog.text
    # level images: DOWN2 of the loaded tensors, applied once more per coarser level
    half = rr.down2(content.numpy())
    assert torch.equal(_Model.built[2].content, content) and torch.equal(_Model.built[1].content, torch.from_numpy(half))
    assert torch.equal(_Model.built[0].content, torch.from_numpy(rr.down2(half)))
    # start images: the coarsest content (init_method = content), then leaves of twice the size
    assert [tuple(x.shape) for x in seen] == [(1, 3, 64, 64), (1, 3, 128, 128), (1, 3, 256, 256)]
    assert all(x.is_leaf and x.requires_grad for x in seen)
    assert image is seen[2] and tuple(image.shape) == (1, 3, 256, 256) and elapsed >= 0.0
    assert set(history) == {"style_loss", "content_loss", "total_loss"} and all(len(v) == 7 for v in history.values())
    assert bar.updates == 7 and bar.closed == 0                                # an injected bar stays the caller's to close


def test_start_of_a_level_is_up2_of_the_previous_result(host_driver):
    content, style = _images()
    results = {}

    def factory(x):
        results.setdefault("starts", []).append(x.detach().clone())
        results.setdefault("live", []).append(x)
        return _sgd(x)
    pyramid.run_pyramid(content, style, CPU, _cfg(2, pyramid_steps=[2, 1]), optimizer_factory=factory, progress_bar=_Bar())
    coarse_result = results["live"][0].detach()
    assert not torch.equal(coarse_result, results["starts"][0])               # the level moved its image
    assert torch.equal(results["starts"][1], torch.from_numpy(rr.up2(coarse_result.numpy())))


def test_csv_is_merged_and_level_files_are_removed(host_driver, tmp_path):
    content, style = _images()
    path = tmp_path / "logs" / "loss.csv"
    cfg = _cfg(3, steps=7, log_loss=str(path))
    _, history, _ = pyramid.run_pyramid(content, style, CPU, cfg, optimizer_factory=_sgd, progress_bar=_Bar())
    assert history == {}                                                      # CSV mode keeps no history, as in a single run
    rows = list(csv.reader(path.open()))
    assert rows[0] == ["step", "style_loss", "content_loss", "total_loss"]
    assert [r[0] for r in rows[1:]] == [str(k) for k in range(1, 8)]
    assert all(len(r) == 4 and float(r[3]) >= 0 for r in rows[1:])
    assert sorted(p.name for p in path.parent.iterdir()) == ["loss.csv"]
    assert pyramid.level_log_path(path, 1).name == "loss.level1.csv"
    assert cfg.output.log_loss == str(path)


def test_a_level_that_raises_keeps_its_exception_and_its_level_files(host_driver, tmp_path):
    """The merge happens after a complete run only: the error of the failing level is the one the caller sees, the
    finished level's rows stay in its own file, and the requested path is not written."""
    content, style = _images()
    path = tmp_path / "loss.csv"

    def factory(x):
        if x.shape[-1] == 256:
            raise RuntimeError("second level cannot start")
        return _sgd(x)
    with pytest.raises(RuntimeError, match="second level cannot start"):
        pyramid.run_pyramid(content, style, CPU, _cfg(2, steps=4, log_loss=str(path)), optimizer_factory=factory, progress_bar=_Bar())
    assert sorted(p.name for p in tmp_path.iterdir()) == ["loss.level0.csv"]
    assert len(list(csv.reader((tmp_path / "loss.level0.csv").open()))) == 3


def test_one_level_is_one_plain_run(host_driver):
    content, style = _images()
    image, history, _ = pyramid.run_pyramid(content, style, CPU, _cfg(1, steps=3), optimizer_factory=_sgd, progress_bar=_Bar())
    assert len(_Model.built) == 1 and tuple(_Model.built[0].style.shape[-2:]) == (262, 259)
    assert tuple(image.shape) == (1, 3, 256, 256) and all(len(v) == 3 for v in history.values())
