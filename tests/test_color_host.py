"""Colour preservation (--preserve-color), everything that runs without a GPU: configuration, the 3x3 algebra of
``color.matching_transform``, what the NumPy twins of the kernels (tests/color_ref.py) achieve on loader-like images, the C
ABI's argument checks, and the wiring of ``main.style_transfer`` with the three ops replaced by their twins."""
from __future__ import annotations

import os
import re
from pathlib import Path

import numpy as np
import pytest
import torch
from torch import nn

from style_transfer_visualizer_amd import _lib, cli, color, core_model, image_io, ops, optimization, pyramid, runtime
from style_transfer_visualizer_amd import config as stv_config
from style_transfer_visualizer_amd import config_defaults
from style_transfer_visualizer_amd import main as stv_main
from style_transfer_visualizer_amd.constants import MIN_DIMENSION
from style_transfer_visualizer_amd.type_defs import InputPaths
from tests import color_ref as cr
from tests import resize_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--content", "c.png", "--style", "s.png"]
SIZES = {"content": (64, 80), "style": (72, 64)}            # sides at MIN_DIMENSION or a little above
MEAN_BOUND = 1e-6            # absolute, on the float64 mean after the fp32 affine twin
COV_BOUND = 1e-6             # of the largest covariance entry
LUMA_BOUND = 1e-6


# ------------------------------------------------------------------------------------------------ configuration
def _cli_config(argv):
    args = cli.build_arg_parser().parse_args(argv)
    base = stv_config.ConfigLoader.load(args.config) if args.config else None
    return stv_config.build_config_from_cli(vars(args), base_config=base)


def test_default_is_off():
    assert config_defaults.DEFAULT_PRESERVE_COLOR == "off"
    assert stv_config.StyleTransferConfig.model_validate({}).optimization.preserve_color == "off"
    assert _cli_config(BASE).optimization.preserve_color == "off"


def test_cli_and_toml_round_trip(tmp_path):
    for mode in ("off", "match", "luma"):
        assert _cli_config([*BASE, "--preserve-color", mode]).optimization.preserve_color == mode
    toml = tmp_path / "config.toml"
    toml.write_text('[optimization]\npreserve_color = "luma"\nsteps = 7\n')
    cfg = stv_config.ConfigLoader.load(str(toml))
    assert cfg.optimization.preserve_color == "luma" and cfg.optimization.steps == 7
    assert stv_config.StyleTransferConfig.model_validate(cfg.model_dump()).optimization.preserve_color == "luma"
    assert _cli_config(["--config", str(toml)]).optimization.preserve_color == "luma"                         # TOML alone
    assert _cli_config(["--config", str(toml), "--preserve-color", "match"]).optimization.preserve_color == "match"
    assert stv_config._DIRECT["preserve_color"] == ("optimization", "preserve_color")


def test_an_unknown_value_is_refused(tmp_path, capsys):
    with pytest.raises(SystemExit):
        cli.build_arg_parser().parse_args([*BASE, "--preserve-color", "histogram"])
    assert "invalid choice" in capsys.readouterr().err
    with pytest.raises(ValueError):
        stv_config.OptimizationConfig(preserve_color="histogram")
    toml = tmp_path / "config.toml"
    toml.write_text('[optimization]\npreserve_color = "on"\n')
    with pytest.raises(ValueError):
        stv_config.ConfigLoader.load(str(toml))


def test_settings_summary_shows_the_row_only_when_on(caplog):
    paths = InputPaths(content_path="c.png", style_path="s.png")
    for argv in (BASE, [*BASE, "--preserve-color", "off"]):
        caplog.clear()
        with caplog.at_level("INFO"):
            cli.log_parameters(paths, _cli_config(argv))
        assert "Preserve Color" not in caplog.text
    for mode in ("match", "luma"):
        caplog.clear()
        with caplog.at_level("INFO"):
            cli.log_parameters(paths, _cli_config([*BASE, "--preserve-color", mode]))
        assert f"Preserve Color: {mode}" in caplog.text


# ------------------------------------------------------------------------------------------- matching_transform
def _cov(stats):
    n, sums, second = stats
    mu = sums / n
    return mu, second / n - np.outer(mu, mu)


def _random_image(seed: int, H: int, W: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    mix = rng.standard_normal((3, 3)) + 2.0 * np.eye(3)
    return np.einsum("ij,jhw->ihw", mix, rng.standard_normal((3, H, W))) + rng.standard_normal((3, 1, 1))


def test_full_rank_transform_matches_mean_and_covariance_in_float64(caplog):
    for seed in range(4):
        style, content = cr.stats(_random_image(seed, 33, 41)), cr.stats(_random_image(100 + seed, 29, 47))
        A, b, rank = color._matching_transform64(style, content)
        mu_s, cov_s = _cov(style)
        mu_c, cov_c = _cov(content)
        assert rank == 3 and A.dtype == np.float64 and b.dtype == np.float64
        assert np.abs(A @ cov_s @ A.T - cov_c).max() <= 1e-10
        assert np.abs(A @ mu_s + b - mu_c).max() <= 1e-10
        with caplog.at_level("WARNING"):
            A32, b32 = color.matching_transform(style, content)
        assert A32.dtype == np.float32 and b32.dtype == np.float32 and A32.shape == (3, 3) and b32.shape == (3,)
        assert np.array_equal(A32, A.astype(np.float32)) and np.array_equal(b32, b.astype(np.float32))
    assert "rank" not in caplog.text


def test_greyscale_style_gives_a_finite_rank_one_transform_and_one_warning(caplog):
    grey = np.random.default_rng(5).random((1, 40, 40))
    style, content = cr.stats(np.broadcast_to(grey, (3, 40, 40))), cr.stats(_random_image(7, 40, 40))
    with caplog.at_level("WARNING"):
        A, b = color.matching_transform(style, content)
    warnings = [r for r in caplog.records if r.levelname == "WARNING"]
    assert len(warnings) == 1 and "rank 1 of 3" in warnings[0].getMessage()
    assert np.isfinite(A).all() and np.isfinite(b).all()
    assert np.linalg.matrix_rank(A.astype(np.float64), tol=1e-5 * np.abs(A).max()) == 1
    # the one direction it has is matched: the mean exactly, and the variance the style had along (1,1,1)/sqrt(3)
    A64, b64, rank = color._matching_transform64(style, content)
    mu_s, cov_s = _cov(style)
    mu_c, cov_c = _cov(content)
    assert rank == 1 and np.abs(A64 @ mu_s + b64 - mu_c).max() <= 1e-10
    u = np.ones(3) / np.sqrt(3.0)
    root_c = np.linalg.eigh(cov_c)
    root_c = (root_c[1] * np.sqrt(root_c[0])) @ root_c[1].T
    assert np.abs(A64 @ cov_s @ A64.T - root_c @ np.outer(u, u) @ root_c).max() <= 1e-10


@pytest.mark.parametrize("value", [0.0, 0.5, (0.5 - 0.485) / 0.229])
def test_constant_style_gives_a_zero_matrix_and_the_content_mean(value, caplog):
    const = np.full((3, 64, 64), np.float32(value))
    style, content = cr.stats(const), cr.stats(_random_image(9, 64, 64))
    with caplog.at_level("WARNING"):
        A, b = color.matching_transform(style, content)
    assert np.array_equal(A, np.zeros((3, 3), dtype=np.float32))
    assert np.array_equal(b, (content[1] / content[0]).astype(np.float32))
    assert sum("rank 0 of 3" in r.getMessage() for r in caplog.records) == 1


# ---------------------------------------------------------------------------------------------- twin properties
def test_sizes_sit_at_the_minimum_dimension():
    assert min(min(hw) for hw in SIZES.values()) == MIN_DIMENSION == 64


@pytest.mark.parametrize("normalize", [True, False], ids=["normalised", "plain"])
def test_affine_twin_gives_the_style_the_content_statistics(normalize):
    content = cr.uint8_image(*SIZES["content"], 0, normalize=normalize)
    style = cr.uint8_image(*SIZES["style"], 1, normalize=normalize)
    A, b = color.matching_transform(cr.stats(style), cr.stats(content))
    matched = cr.affine(style, [*A.reshape(-1), *b])
    assert matched.dtype == np.float32 and matched.shape == style.shape
    mu, cov = cr.mean_cov(matched)
    mu_c, cov_c = cr.mean_cov(content)
    mu_s, cov_s = cr.mean_cov(style)
    mean_err, cov_err = np.abs(mu - mu_c).max(), np.abs(cov - cov_c).max() / np.abs(cov_c).max()
    print(f"affine twin, normalize={normalize}: mean error {mean_err:.2e}, covariance error {cov_err:.2e} of the largest entry")
    assert np.abs(mu_s - mu_c).max() > 1e-3 and np.abs(cov_s - cov_c).max() > 1e-3 * np.abs(cov_c).max()    # there was something to match
    assert mean_err <= MEAN_BOUND
    assert cov_err <= COV_BOUND


@pytest.mark.parametrize("normalize", [True, False], ids=["normalised", "plain"])
def test_luma_twin_keeps_the_luminance_of_the_result_and_the_chroma_of_the_content(normalize):
    H, W = SIZES["content"]
    content = cr.uint8_image(H, W, 0, normalize=normalize)
    noise = np.random.default_rng(3).standard_normal(content.shape).astype(np.float32)
    result = content + noise                                          # far outside [0, 1]: the clamp is at work
    out = cr.luma(result, content, normalize=normalize)
    assert out.dtype == np.float32 and out.shape == content.shape
    result_rgb, content_rgb = (cr.rgb01(v, normalize=normalize).astype(np.float64)[0] for v in (result, content))
    assert ((result_rgb == 0) | (result_rgb == 1)).mean() > 0.05
    out_rgb = out.astype(np.float64)[0]
    if normalize:
        out_rgb = out_rgb * np.reshape(cr.IMAGENET_STD, (3, 1, 1)) + np.reshape(cr.IMAGENET_MEAN, (3, 1, 1))
    w = np.reshape([0.299, 0.587, 0.114], (3, 1, 1))
    y_err = np.abs((w * out_rgb).sum(0) - (w * result_rgb).sum(0)).max()
    shift = out_rgb - content_rgb
    chroma_err = max(np.abs(shift[0] - shift[1]).max(), np.abs(shift[0] - shift[2]).max(), np.abs(shift[1] - shift[2]).max())
    print(f"luma twin, normalize={normalize}: luminance error {y_err:.2e}, chroma error {chroma_err:.2e}")
    assert np.abs(shift).max() > 0.1
    assert y_err <= LUMA_BOUND
    assert chroma_err <= LUMA_BOUND


def test_twins_treat_non_finite_values_like_prepare_image_for_output():
    x = torch.tensor([float("nan"), float("inf"), float("-inf"), -3.0, 0.25, 7.0]).repeat(3, 1).reshape(1, 3, 2, 3).contiguous()
    for normalize in (True, False):
        want = image_io.prepare_image_for_output(x, normalize=normalize).numpy()
        assert np.array_equal(cr.rgb01(x.numpy(), normalize=normalize), want)


# ---------------------------------------------------------------------------------------------------------- ABI
def test_library_exports_the_three_entry_points_and_the_constants_match_the_header():
    lib = _lib.load()
    for name in ("stv_color_stats", "stv_color_affine", "stv_luma_transfer"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.stv_version() >= 107
    header = open(os.path.join(ROOT, "include", "stv.h")).read()
    for name, value in (("STV_COLOR_VEC", _lib.COLOR_VEC), ("STV_COLOR_THREADS", _lib.COLOR_THREADS),
                        ("STV_COLOR_STATS_PARTS", _lib.COLOR_STATS_PARTS), ("STV_COLOR_MAX_BLOCKS", _lib.COLOR_MAX_BLOCKS)):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", header).group(1)) == value
    source = open(os.path.join(ROOT, "style_transfer_visualizer_amd", "csrc", "color.hip")).read()
    assert re.search(r"kColorThreads\s*=\s*STV_COLOR_THREADS", source)
    assert re.search(r"kColorStatsBlocks\s*=\s*STV_COLOR_STATS_PARTS", source)
    assert re.search(r"kColorBlocks\s*=\s*STV_COLOR_MAX_BLOCKS", source)


def test_bad_arguments_are_refused_before_any_device_work():
    """Each of these returns STV_ERR_ARG (1) on a machine without a GPU: the checks come before any HIP call."""
    import ctypes
    lib = _lib.load()
    m12 = (ctypes.c_float * 12)(*([1.0] * 12))
    m3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    X, Y, Z = 1 << 20, 2 << 20, 3 << 20                                # addresses that are never dereferenced
    # null pointers
    assert lib.stv_color_stats(None, Y, 4, 4, None) == 1
    assert lib.stv_color_stats(X, None, 4, 4, None) == 1
    assert lib.stv_color_affine(None, Y, m12, 4, 4, None) == 1
    assert lib.stv_color_affine(X, None, m12, 4, 4, None) == 1
    assert lib.stv_color_affine(X, Y, None, 4, 4, None) == 1
    assert lib.stv_luma_transfer(None, Y, Z, 4, 4, None, None, None) == 1
    assert lib.stv_luma_transfer(X, None, Z, 4, 4, None, None, None) == 1
    assert lib.stv_luma_transfer(X, Y, None, 4, 4, None, None, None) == 1
    assert lib.stv_luma_transfer(X, Y, Z, 4, 4, m3, None, None) == 1               # one of mean3 / std3 without the other
    assert lib.stv_luma_transfer(X, Y, Z, 4, 4, None, m3, None) == 1
    # non-positive dimensions; 3 * 16384 * 10923 * 4 bytes is just over 2 GiB, 3 * 8192 * 21846 * 4 as well
    for H, W in ((0, 4), (4, 0), (-1, 4), (4, -3), (16384, 10923), (8192, 21846), (1 << 15, 1 << 15)):
        assert 3 * H * W * 4 >= (1 << 31) or H <= 0 or W <= 0
        assert lib.stv_color_stats(X, Y, H, W, None) == 1
        assert lib.stv_color_affine(X, Y, m12, H, W, None) == 1
        assert lib.stv_color_affine(X, X, m12, H, W, None) == 1
        assert lib.stv_luma_transfer(X, Y, Z, H, W, None, None, None) == 1
    # overlap: 3 * 4 * 4 floats are 192 bytes
    assert lib.stv_luma_transfer(X, Y, Y, 4, 4, None, None, None) == 1             # out == content
    assert lib.stv_luma_transfer(X, Y, Y + 64, 4, 4, None, None, None) == 1
    assert lib.stv_luma_transfer(X, Y, X + 64, 4, 4, None, None, None) == 1        # out overlaps result without being it
    for delta in (4, 64, 188, -4, -188):
        assert lib.stv_color_affine(X, X + delta, m12, 4, 4, None) == 1            # partially overlapping ranges


# ------------------------------------------------------------------------------------------------------- wiring
class _Bar:
    def update(self, n=1):
        pass

    def set_postfix(self, d=None, refresh=True, **kw):
        pass

    def close(self):
        pass


class Recorder:
    def __init__(self):
        self.events: list = []
        self.prepared = None
        self.saved = None
        self.luma_args = None
        self.pyramid_args = None


def _twin_ops(monkeypatch, rec: Recorder) -> None:
    """The three ops replaced by their NumPy twins on host tensors; every call is an event."""
    def color_stats(img):
        rec.events.append("stats")
        parts = torch.zeros(_lib.COLOR_STATS_PARTS, 9, dtype=torch.float64)
        parts[0] = torch.from_numpy(cr.moments(img.numpy()))
        return parts

    def color_affine(x, m12, out=None):
        rec.events.append("affine")
        return torch.from_numpy(cr.affine(x.numpy(), m12))

    def luma_transfer(result, content, *, mean, std, out=None):
        rec.events.append("luma")
        rec.luma_args = (result, content, mean, std)
        return torch.from_numpy(cr.luma(result.numpy(), content.numpy(), normalize=mean is not None))
    monkeypatch.setattr(ops, "color_stats", color_stats)
    monkeypatch.setattr(ops, "color_affine", color_affine)
    monkeypatch.setattr(ops, "luma_transfer", luma_transfer)


@pytest.fixture
def loaded(monkeypatch):
    """``style_transfer`` on the CPU up to the model: the loaders and the save step are recording stand-ins, the three colour
    ops are their twins."""
    rec = Recorder()
    images = {"c.png": torch.from_numpy(cr.uint8_image(128, 128, 0, normalize=True)),
              "s.png": torch.from_numpy(cr.uint8_image(136, 128, 1, normalize=True))}
    _twin_ops(monkeypatch, rec)
    monkeypatch.setattr(runtime, "validate_input_paths", lambda *a, **k: None)
    monkeypatch.setattr(runtime, "setup_random_seed", lambda seed: rec.events.append("seed"))
    monkeypatch.setattr(runtime, "setup_device", lambda name: torch.device("cpu"))
    monkeypatch.setattr(runtime, "setup_output_directory", lambda p: Path("mock_output"))
    monkeypatch.setattr(runtime, "save_outputs", lambda *a, **k: setattr(rec, "saved", a))
    monkeypatch.setattr(image_io, "load_image_to_tensor", lambda path, device, normalize: images[path])
    return rec, images


@pytest.fixture
def wired(loaded, monkeypatch):
    """... and model construction and the runner as well.  The run's 'result' has values outside [0, 1]."""
    rec, images = loaded
    result = images["c.png"] + torch.randn(1, 3, 128, 128, generator=torch.Generator().manual_seed(2))

    def prepare(content, style, device, optimization_config, *, precision=None):
        rec.events.append("model")
        rec.prepared = (content, style)
        return "model", content.clone().requires_grad_(True), "optimizer"
    monkeypatch.setattr(core_model, "prepare_model_and_input", prepare)

    class FakeRunner:
        def __init__(self, *args, **kwargs):
            pass

        def run(self):
            rec.events.append("run")
            return result.clone().requires_grad_(True), {"total_loss": [1.0]}, 3.14
    monkeypatch.setattr(optimization, "OptimizationRunner", FakeRunner)
    return rec, images, result


def _cfg(mode: str | None, *, levels: int = 1):
    cfg = stv_config.StyleTransferConfig.model_validate({})
    cfg.optimization.steps = 4
    cfg.optimization.pyramid_levels = levels
    cfg.optimization.init_method = "content"
    cfg.video.create_video = False
    cfg.output.log_every = 1
    if mode is not None:
        cfg.optimization.preserve_color = mode
    return cfg


PATHS = InputPaths(content_path="c.png", style_path="s.png")


@pytest.mark.parametrize("mode", [None, "off"])
def test_off_calls_none_of_the_three_ops(wired, mode):
    rec, images, result = wired
    out = stv_main.style_transfer(PATHS, _cfg(mode))
    assert rec.events == ["seed", "model", "run"]
    assert rec.prepared[0] is images["c.png"] and rec.prepared[1] is images["s.png"]
    assert torch.equal(rec.saved[0], result) and torch.equal(out, result.clamp(0, 1))


def test_match_transforms_the_style_before_the_model_is_built(wired):
    rec, images, result = wired
    style_before = images["s.png"].clone()
    out = stv_main.style_transfer(PATHS, _cfg("match"))
    assert rec.events == ["stats", "stats", "affine", "seed", "model", "run"]
    A, b = color.matching_transform(cr.stats(images["s.png"].numpy()), cr.stats(images["c.png"].numpy()))
    want = torch.from_numpy(cr.affine(images["s.png"].numpy(), [*A.reshape(-1), *b]))
    content_seen, style_seen = rec.prepared
    assert content_seen is images["c.png"]
    assert torch.equal(style_seen, want) and not torch.equal(style_seen, images["s.png"])
    assert torch.equal(images["s.png"], style_before)                    # the loaded tensor is not modified
    assert torch.equal(rec.saved[0], result) and torch.equal(out, result.clamp(0, 1))      # the run's end is unchanged


def test_luma_runs_once_after_the_run_and_its_output_is_saved_and_returned(wired):
    rec, images, result = wired
    out = stv_main.style_transfer(PATHS, _cfg("luma"))
    assert rec.events == ["seed", "model", "run", "luma"]
    assert rec.prepared[1] is images["s.png"]
    got_result, got_content, mean, std = rec.luma_args
    assert torch.equal(got_result, result) and not got_result.requires_grad
    assert torch.equal(got_content, images["c.png"])
    assert list(mean) == [0.485, 0.456, 0.406] and list(std) == [0.229, 0.224, 0.225]
    want = torch.from_numpy(cr.luma(result.numpy(), images["c.png"].numpy(), normalize=True))
    assert torch.equal(rec.saved[0], want) and not torch.equal(want, result)
    assert torch.equal(out, want.clamp(0, 1)) and not out.requires_grad
    cfg = _cfg("luma")
    cfg.optimization.normalize = False
    stv_main.style_transfer(PATHS, cfg)
    assert rec.luma_args[2] is None and rec.luma_args[3] is None


class _Model(nn.Module):
    """Stands in for StyleContentModel on the CPU (the runner's autograd path): records what it is given."""

    built: list = []

    def __init__(self, style_layers, content_layers, precision=None):
        super().__init__()
        type(self).built.append(self)

    def set_targets(self, style, content):
        self.style, self.content = style.detach().clone(), content.detach().clone()

    def forward(self, x):
        return [(x.mean() - self.style.mean()) ** 2], [((x - self.content) ** 2).mean()]


def test_two_levels_receive_the_matched_style_and_run_no_colour_op(loaded, monkeypatch):
    """The real ``run_pyramid`` and runner under ``style_transfer``, with a small autograd module for the model, the resize
    twin and SGD (as tests/test_pyramid_host.py drives them)."""
    rec, images = loaded
    _Model.built = []
    monkeypatch.setattr(core_model, "StyleContentModel", _Model)
    monkeypatch.setattr(ops, "resize2x", lambda x, mode, out=None: torch.from_numpy(
        (rr.down2 if mode == _lib.RESIZE_DOWN2 else rr.up2)(x.detach().numpy())))
    real = pyramid.run_pyramid

    def spy(content, style, device, config, **kw):
        rec.pyramid_args = (content, style, list(rec.events))
        return real(content, style, device, config, optimizer_factory=lambda x: torch.optim.SGD([x], lr=0.5), progress_bar=_Bar(), **kw)
    monkeypatch.setattr(pyramid, "run_pyramid", spy)
    out = stv_main.style_transfer(PATHS, _cfg("match", levels=2))
    A, b = color.matching_transform(cr.stats(images["s.png"].numpy()), cr.stats(images["c.png"].numpy()))
    matched = torch.from_numpy(cr.affine(images["s.png"].numpy(), [*A.reshape(-1), *b]))
    content_seen, style_seen, events_at_entry = rec.pyramid_args
    assert content_seen is images["c.png"] and torch.equal(style_seen, matched)
    assert events_at_entry == ["stats", "stats", "affine"]
    assert rec.events == [*events_at_entry, "seed"]                       # inside the levels: the seeding, no colour op
    assert len(_Model.built) == 2
    assert torch.equal(_Model.built[1].style, matched)
    assert torch.equal(_Model.built[0].style, torch.from_numpy(rr.down2(matched.numpy())))
    assert torch.equal(_Model.built[1].content, images["c.png"])
    assert tuple(out.shape) == (1, 3, 128, 128)
