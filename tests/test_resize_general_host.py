"""Input resizing (--content-size, --style-size, --style-scale), everything that runs without a GPU: the coefficient tables
against the twin's (tests/resize_general_ref.py), the twin against PIL, the size rules and their refusals, configuration,
CLI, the C ABI's argument checks, and where the stage sits in ``main.style_transfer`` - with ``ops.resize`` replaced by the
twin and the model by a stand-in."""
from __future__ import annotations

import os
import re
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

from style_transfer_visualizer_amd import _lib, cli, color, core_model, image_io, ops, optimization, runtime
from style_transfer_visualizer_amd import config as stv_config
from style_transfer_visualizer_amd import config_defaults
from style_transfer_visualizer_amd import main as stv_main
from style_transfer_visualizer_amd import resize as rz
from style_transfer_visualizer_amd.constants import MIN_DIMENSION
from style_transfer_visualizer_amd.type_defs import InputPaths
from tests import resize_general_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERS = ("bilinear", "bicubic", "lanczos")
# (C, H, W) -> (Ho, Wo): the shapes of tests/test_gpu_resize_general_exact.py
SHAPES = [((3, 1, 1), (3, 5)), ((3, 5, 7), (3, 11)), ((3, 37, 53), (16, 20)), ((3, 16, 20), (37, 53)),
          ((3, 64, 48), (64, 31)), ((3, 64, 48), (23, 48)), ((1, 100, 75), (13, 9)), ((3, 9, 9), (9, 9)),
          ((3, 40, 36), (24, 32)), ((3, 40, 36), (24, 30)),
          # just past one pass of the capped grid (262144 items of four pixels), aligned and ragged, and one row short of it
          ((3, 300, 300), (296, 1184)), ((3, 300, 300), (296, 1181)), ((3, 300, 300), (295, 1184))]
AXES = sorted({(n_in, n_out) for (_, H, W), (Ho, Wo) in SHAPES for n_in, n_out in ((H, Ho), (W, Wo))})
ULP = float(np.spacing(np.float32(1.0)))


# ------------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("name", FILTERS)
def test_tables_equal_the_twins_bit_for_bit(name):
    per_pass = _lib.RESIZE_AXIS_MAX_BLOCKS * _lib.RESIZE_AXIS_THREADS
    assert 3 * 296 * (1184 // 4) > per_pass >= 3 * 295 * (1184 // 4)       # the last three shapes are what they claim
    for n_in, n_out in AXES:
        start, count, weights = rz.axis_table(n_in, n_out, name)
        s2, c2, w2 = gr.table(n_in, n_out, name)
        what = f"{name} {n_in} -> {n_out}"
        assert start.dtype == np.int32 and count.dtype == np.int32 and weights.dtype == np.float32, what
        assert start.shape == count.shape == (n_out,) and weights.shape == (n_out, int(count.max())), what
        assert np.array_equal(start, s2) and np.array_equal(count, c2), what
        assert np.array_equal(weights.view(np.uint32), w2.view(np.uint32)), what
        assert (start >= 0).all() and (count >= 1).all() and (start + count <= n_in).all(), what
        for i in range(n_out):
            assert not weights[i, count[i]:].any(), what                        # the padding is zero
            total = np.float32(0)
            for k in range(count[i]):
                total = total + weights[i, k]
            assert abs(float(total) - 1.0) <= 4 * ULP, f"{what}: row {i} sums to {float(total)!r}"


def test_supports_and_the_stretch_on_a_downscale():
    assert {k: v[1] for k, v in rz.FILTERS.items()} == {"bilinear": 1.0, "bicubic": 2.0, "lanczos": 3.0}
    for name, taps in (("bilinear", 2), ("bicubic", 4), ("lanczos", 6)):
        assert int(rz.axis_table(16, 37, name)[1].max()) == taps                 # an upscale: the filter's own support
        assert int(rz.axis_table(100, 25, name)[1].max()) == 4 * taps            # a downscale by 4: stretched by 4
    start, count, weights = rz.axis_table(8, 4, "bilinear")                      # by hand: c = 1, 3, 5, 7, support 2
    assert start.tolist() == [0, 1, 3, 5] and count.tolist() == [3, 4, 4, 3]
    assert weights[1].tolist() == [0.125, 0.375, 0.375, 0.125]
    assert weights[0].tolist() == [np.float32(3 / 7), np.float32(3 / 7), np.float32(1 / 7), 0.0]
    with pytest.raises(ValueError, match="unknown resize filter 'box'"):
        rz.axis_table(8, 4, "box")


# ------------------------------------------------------------------------------- the twin against PIL's resize
def _pil_resize(x: np.ndarray, size, name: str) -> np.ndarray:
    method = {"bilinear": Image.Resampling.BILINEAR, "bicubic": Image.Resampling.BICUBIC, "lanczos": Image.Resampling.LANCZOS}[name]
    planes = [np.asarray(Image.fromarray(p, mode="F").resize((size[1], size[0]), method), dtype=np.float32) for p in x]
    return np.stack(planes)


def _bound(shape, size, name: str, peak: float) -> float:
    """``((Th + 2) + (Tv + 2)) * 2^-24 * Ah * Av * max|x|`` from the tables: T the largest count per axis, A the largest
    row sum of |w|.  A pass of T taps in fp32 is T products and T sums of relative error 2^-24 each, plus the rounding of
    the weights and of PIL's own fp32 result per pass (the + 2); the second pass magnifies the first's error by at most
    Av, and either pass magnifies the data by at most A."""
    terms = []
    for n_in, n_out in ((shape[2], size[1]), (shape[1], size[0])):
        if n_in == n_out:
            terms.append((0, 1.0))
            continue
        _, count, weights = gr.table(n_in, n_out, name)
        terms.append((int(count.max()) + 2, float(np.abs(weights.astype(np.float64)).sum(axis=1).max())))
    (th, ah), (tv, av) = terms
    return (th + tv) * 2.0 ** -24 * ah * av * peak


@pytest.mark.parametrize("name", FILTERS)
@pytest.mark.parametrize("shape_size", [s for s in SHAPES if s[0][1] * s[0][2] < 10000], ids=lambda s: f"{s[0]}-{s[1]}")
def test_twin_agrees_with_pil_within_the_bound_of_its_tables(shape_size, name):
    shape, size = shape_size
    x = gr.randn3(*shape, seed=7 * shape[1] + shape[2])
    got = gr.resize(x, size, name)
    assert got.dtype == np.float32 and got.shape == (shape[0], *size)
    if size == shape[1:]:
        assert got is x or np.shares_memory(got, x)                            # same size: the input itself
        return
    want = _pil_resize(x, size, name)
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    bound = _bound(shape, size, name, float(np.abs(x).max()))
    print(f"{name} {shape} -> {size}: max |twin - PIL| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound, f"{name} {shape} -> {size}: {err:.3e} above {bound:.3e}"


# ------------------------------------------------------------------------------------------------- size rules
def test_target_size_on_hand_computed_cases():
    assert rz.target_size(100, 150, 96, 1) == (64, 96)                # 150x100 -> 96: 96x64
    assert rz.target_size(150, 100, 96, 1) == (96, 64)
    assert rz.target_size(200, 300, 260, 2) == (174, 260)             # 173.33 -> the nearest even number
    assert rz.target_size(3000, 4000, 1024, 4) == (768, 1024)
    assert rz.target_size(100, 200, 101, 1) == (51, 101)              # a tie: 50.5 rounds up
    assert rz.target_size(300, 200, 9, 4) == (8, 8)                   # ties in multiples of 4: 9 / 4 = 2.25 -> 8, 6 / 4 = 1.5 -> 8
    assert rz.target_size(10, 1000, 64, 8) == (8, 64)                 # 0.64 would round to 0: at least one multiple
    assert rz.target_size(64, 64, 64, 1) == (64, 64)
    with pytest.raises(ValueError, match="positive"):
        rz.target_size(0, 10, 5, 1)


def _oc(**kw):
    return stv_config.OptimizationConfig(**kw)


def test_plan_sizes():
    assert rz.plan_sizes(_oc(), (100, 150), (90, 120)) == (None, None)
    assert rz.plan_sizes(_oc(content_size=96), (100, 150), (90, 120)) == ((64, 96), None)
    assert rz.plan_sizes(_oc(content_size=150), (100, 150), (90, 120)) == (None, None)                 # already that size
    assert rz.plan_sizes(_oc(style_size=100), (100, 150), (90, 120)) == (None, (75, 100))
    # the scale refers to the content as the run will see it: 96 after --content-size, 150 without
    assert rz.plan_sizes(_oc(content_size=96, style_scale=1.0), (100, 150), (90, 120)) == ((64, 96), (72, 96))
    assert rz.plan_sizes(_oc(style_scale=1.0), (100, 150), (90, 120)) == (None, (113, 150))           # 112.5: the tie rounds up
    assert rz.plan_sizes(_oc(style_scale=2.0), (100, 150), (90, 120)) == (None, (225, 300))
    # a content that --pyramid-levels accepts: both sides multiples of 2**(levels-1)
    assert rz.plan_sizes(_oc(content_size=260, pyramid_levels=2), (200, 300), (300, 300)) == ((174, 260), None)
    assert rz.plan_sizes(_oc(content_size=1024, pyramid_levels=3), (3000, 4001), (300, 300)) == ((768, 1024), None)


@pytest.fixture
def no_kernels(monkeypatch):
    """Any resize or model construction is a failure of the test."""
    def forbidden(*a, **k):
        raise AssertionError("an up-front check let the run reach the device")
    monkeypatch.setattr(ops, "resize", forbidden)
    monkeypatch.setattr(ops, "resize2x", forbidden)
    monkeypatch.setattr(core_model, "StyleContentModel", forbidden)
    monkeypatch.setattr(core_model, "prepare_model_and_input", forbidden)


def test_plan_sizes_refusals():
    assert MIN_DIMENSION == 64
    with pytest.raises(ValueError, match=r"style_size = 128 and style_scale = 0\.5 both"):
        rz.plan_sizes(_oc(style_size=128, style_scale=0.5), (100, 150), (90, 120))
    with pytest.raises(ValueError, match=r"content_size = 90 resizes the content image from 150x100 to 90x60; the minimum dimension is 64"):
        rz.plan_sizes(_oc(content_size=90), (100, 150), (90, 120))
    with pytest.raises(ValueError, match=r"style_size = 80 resizes the style image from 120x90 to 80x60"):
        rz.plan_sizes(_oc(style_size=80), (100, 150), (90, 120))
    with pytest.raises(ValueError, match=r"style_scale = 0\.5 \(longer side 75\) resizes the style image from 120x90 to 75x56"):
        rz.plan_sizes(_oc(style_scale=0.5), (100, 150), (90, 120))


# -------------------------------------------------------------------------------------------------- surface
def _cli_config(argv):
    args = cli.build_arg_parser().parse_args(argv)
    base = stv_config.ConfigLoader.load(args.config) if args.config else None
    return stv_config.build_config_from_cli(vars(args), base_config=base)


BASE = ["--content", "c.png", "--style", "s.png"]


def test_defaults_and_bounds():
    assert (config_defaults.DEFAULT_CONTENT_SIZE, config_defaults.DEFAULT_STYLE_SIZE, config_defaults.DEFAULT_STYLE_SCALE,
            config_defaults.DEFAULT_RESIZE_FILTER) == (0, 0, 0.0, "lanczos")
    for oc in (stv_config.StyleTransferConfig.model_validate({}).optimization, _cli_config(BASE).optimization):
        assert (oc.content_size, oc.style_size, oc.style_scale, oc.resize_filter) == (0, 0, 0.0, "lanczos")
    for bad in ({"content_size": -1}, {"style_size": -1}, {"style_scale": -0.5}, {"resize_filter": "box"}):
        with pytest.raises(ValueError):
            stv_config.OptimizationConfig(**bad)


def test_cli_and_toml_round_trip(tmp_path, capsys):
    args = cli.build_arg_parser().parse_args(BASE)
    assert (args.content, args.style) == ("c.png", "s.png")                   # the exact options still parse as themselves
    oc = _cli_config([*BASE, "--content-size", "512", "--style-scale", "0.75", "--resize-filter", "bicubic"]).optimization
    assert (oc.content_size, oc.style_size, oc.style_scale, oc.resize_filter) == (512, 0, 0.75, "bicubic")
    oc = _cli_config([*BASE, "--style-size", "300"]).optimization
    assert (oc.content_size, oc.style_size, oc.style_scale, oc.resize_filter) == (0, 300, 0.0, "lanczos")
    toml = tmp_path / "config.toml"
    toml.write_text('[optimization]\ncontent_size = 640\nstyle_size = 320\nresize_filter = "bilinear"\n')
    cfg = stv_config.ConfigLoader.load(str(toml))
    assert (cfg.optimization.content_size, cfg.optimization.style_size, cfg.optimization.resize_filter) == (640, 320, "bilinear")
    assert stv_config.StyleTransferConfig.model_validate(cfg.model_dump()).optimization.content_size == 640
    assert _cli_config(["--config", str(toml)]).optimization.style_size == 320                        # TOML alone
    oc = _cli_config(["--config", str(toml), "--content-size", "96", "--resize-filter", "lanczos"]).optimization
    assert (oc.content_size, oc.style_size, oc.resize_filter) == (96, 320, "lanczos")                 # the CLI overrides it
    for key in ("content_size", "style_size", "style_scale", "resize_filter"):
        assert stv_config._DIRECT[key] == ("optimization", key)
    toml.write_text('[optimization]\nstyle_scale = -1.0\n')
    with pytest.raises(ValueError):
        stv_config.ConfigLoader.load(str(toml))
    with pytest.raises(SystemExit):
        cli.build_arg_parser().parse_args([*BASE, "--resize-filter", "box"])
    assert "invalid choice" in capsys.readouterr().err


def test_settings_summary_shows_only_the_settings_in_use(caplog):
    paths = InputPaths(content_path="c.png", style_path="s.png")
    labels = ("Content Size", "Style Size", "Style Scale", "Resize Filter")
    with caplog.at_level("INFO"):
        cli.log_parameters(paths, _cli_config([*BASE, "--resize-filter", "bicubic"]))     # a filter alone resizes nothing
    assert not any(label in caplog.text for label in labels)
    caplog.clear()
    with caplog.at_level("INFO"):
        cli.log_parameters(paths, _cli_config([*BASE, "--content-size", "512"]))
    assert "Content Size: 512" in caplog.text and "Resize Filter: lanczos" in caplog.text
    assert "Style Size" not in caplog.text and "Style Scale" not in caplog.text
    caplog.clear()
    with caplog.at_level("INFO"):
        cli.log_parameters(paths, _cli_config([*BASE, "--style-scale", "0.5", "--resize-filter", "bilinear"]))
    assert "Style Scale: 0.5" in caplog.text and "Resize Filter: bilinear" in caplog.text
    assert "Content Size" not in caplog.text and "Style Size" not in caplog.text
    caplog.clear()
    with caplog.at_level("INFO"):
        cli.log_parameters(paths, _cli_config([*BASE, "--style-size", "300"]))
    assert "Style Size: 300" in caplog.text


def test_library_exports_stv_resize_axis_and_the_constants_match_the_header():
    lib = _lib.load()
    assert hasattr(lib, "stv_resize_axis") and "stv_resize_axis" in _lib.SIGNATURES
    assert lib.stv_version() >= 109
    header = open(os.path.join(ROOT, "include", "stv.h")).read()
    for name, value in (("STV_RESIZE_AXIS_VEC", _lib.RESIZE_AXIS_VEC), ("STV_RESIZE_AXIS_THREADS", _lib.RESIZE_AXIS_THREADS),
                        ("STV_RESIZE_AXIS_MAX_BLOCKS", _lib.RESIZE_AXIS_MAX_BLOCKS)):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", header).group(1)) == value
    source = open(os.path.join(ROOT, "style_transfer_visualizer_amd", "csrc", "resize.hip")).read()
    assert re.search(r"kAxisThreads\s*=\s*STV_RESIZE_AXIS_THREADS", source)
    assert re.search(r"kAxisBlocks\s*=\s*STV_RESIZE_AXIS_MAX_BLOCKS", source)


def test_bad_arguments_are_refused_before_any_device_work():
    """Each of these returns STV_ERR_ARG (1) on a machine without a GPU: the checks come before any HIP call."""
    lib = _lib.load()
    X, Y, S, C, Wt = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20            # addresses that are never dereferenced

    def call(x=X, y=Y, planes=3, H=8, W=8, n_out=5, axis=0, start=S, count=C, weights=Wt, K=4):
        return lib.stv_resize_axis(x, y, planes, H, W, n_out, axis, start, count, weights, K, None)
    for null in ("x", "y", "start", "count", "weights"):
        assert call(**{null: None}) == 1, null
    assert call(y=X) == 1                                                    # x == y
    for name in ("planes", "H", "W", "n_out"):
        assert call(**{name: 0}) == 1 and call(**{name: -3}) == 1, name
    assert call(axis=2) == 1 and call(axis=-1) == 1
    assert call(K=0) == 1 and call(K=-1) == 1
    assert call(planes=2, H=16384, W=16384, n_out=8) == 1                    # input: 2 * 2^28 * 4 bytes = 2 GiB
    assert call(planes=2, H=16384, W=16384, n_out=8, axis=1) == 1
    assert call(planes=2, H=8, W=16384, n_out=16384, axis=0) == 1            # output of the row pass: 2 GiB
    assert call(planes=2, H=16384, W=8, n_out=16384, axis=1) == 1            # output of the column pass: 2 GiB


# ------------------------------------------------------------------------------------------- the stage in main
class Recorder:
    def __init__(self):
        self.events: list = []
        self.prepared = None
        self.resized: list = []
        self.match_args = None


def _image(H: int, W: int, seed: int) -> torch.Tensor:
    return torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(seed))


@pytest.fixture
def wired(monkeypatch):
    """``style_transfer`` on the CPU: loaders, colour match, model construction, runner and save step are recording
    stand-ins; ``ops.resize`` is the twin."""
    rec = Recorder()
    images = {"c.png": _image(100, 150, 0), "s.png": _image(90, 120, 1)}

    def resize(x, size, filter="lanczos", out=None, tmp=None):      # noqa: A002
        rec.events.append("resize")
        y = torch.from_numpy(gr.resize(x.numpy(), size, filter))
        rec.resized.append((x, tuple(size), filter, y))
        return y

    def match(style, content):
        rec.events.append("match")
        rec.match_args = (style, content)
        return style + 1.0

    def prepare(content, style, device, optimization_config, *, precision=None):
        rec.events.append("model")
        rec.prepared = (content, style)
        return "model", content.clone().requires_grad_(True), "optimizer"

    class FakeRunner:
        def __init__(self, model, input_img, *args, **kwargs):
            self.image = input_img

        def run(self):
            rec.events.append("run")
            return self.image, {"total_loss": [1.0]}, 3.14
    monkeypatch.setattr(ops, "resize", resize)
    monkeypatch.setattr(color, "match_style_to_content", match)
    monkeypatch.setattr(core_model, "prepare_model_and_input", prepare)
    monkeypatch.setattr(optimization, "OptimizationRunner", FakeRunner)
    monkeypatch.setattr(runtime, "validate_input_paths", lambda *a, **k: None)
    monkeypatch.setattr(runtime, "setup_random_seed", lambda seed: rec.events.append("seed"))
    monkeypatch.setattr(runtime, "setup_device", lambda name: torch.device("cpu"))
    monkeypatch.setattr(runtime, "setup_output_directory", lambda p: Path("mock_output"))
    monkeypatch.setattr(runtime, "save_outputs", lambda *a, **k: None)
    monkeypatch.setattr(image_io, "load_image_to_tensor", lambda path, device, normalize: images[path])
    return rec, images


def _cfg(**kw):
    cfg = stv_config.StyleTransferConfig.model_validate({})
    cfg.optimization.steps = 2
    cfg.optimization.init_method = "content"
    cfg.video.create_video = False
    for key, value in kw.items():
        setattr(cfg.optimization, key, value)
    return cfg


PATHS = InputPaths(content_path="c.png", style_path="s.png")


def test_main_resizes_before_the_colour_match_and_hands_the_resized_tensors_on(wired):
    rec, images = wired
    out = stv_main.style_transfer(PATHS, _cfg(content_size=96, style_scale=1.0, resize_filter="bicubic", preserve_color="match"))
    assert rec.events == ["resize", "resize", "match", "seed", "model", "run"]
    (cx, csize, cf, cy), (sx, ssize, sf, sy) = rec.resized
    assert cx is images["c.png"] and sx is images["s.png"]                    # the tensors as loaded
    assert (csize, ssize) == ((64, 96), (72, 96)) and cf == sf == "bicubic"
    assert rec.match_args[0] is sy and rec.match_args[1] is cy               # colour statistics see what the run sees
    content_seen, style_seen = rec.prepared
    assert content_seen is cy and torch.equal(style_seen, sy + 1.0)
    assert torch.equal(cy, torch.from_numpy(gr.resize(images["c.png"].numpy(), (64, 96), "bicubic")))
    assert tuple(out.shape) == (1, 3, 64, 96)


def test_only_the_image_that_changes_size_is_resized(wired):
    rec, images = wired
    stv_main.style_transfer(PATHS, _cfg(style_size=100))
    assert rec.events == ["resize", "seed", "model", "run"]
    assert rec.resized[0][0] is images["s.png"] and rec.resized[0][1:3] == ((75, 100), "lanczos")
    assert rec.prepared[0] is images["c.png"] and rec.prepared[1] is rec.resized[0][3]


def test_with_everything_at_zero_the_stage_is_not_entered(wired, monkeypatch):
    rec, images = wired

    def forbidden(*a, **k):
        raise AssertionError("the resize stage was entered with every setting at 0")
    monkeypatch.setattr(ops, "resize", forbidden)
    monkeypatch.setattr(rz, "plan_sizes", forbidden)
    monkeypatch.setattr(rz, "axis_table", forbidden)
    stv_main.style_transfer(PATHS, _cfg(resize_filter="bilinear"))
    assert rec.events == ["seed", "model", "run"]
    assert rec.prepared[0] is images["c.png"] and rec.prepared[1] is images["s.png"]      # the same tensors


def test_main_refuses_before_ops_resize_or_any_model(wired, no_kernels):
    rec, _ = wired
    with pytest.raises(ValueError, match="both set the style image's size"):
        stv_main.style_transfer(PATHS, _cfg(style_size=100, style_scale=1.0))
    with pytest.raises(ValueError, match=r"content_size = 90 resizes the content image from 150x100 to 90x60"):
        stv_main.style_transfer(PATHS, _cfg(content_size=90))
    with pytest.raises(ValueError, match=r"style_size = 80 resizes the style image from 120x90 to 80x60"):
        stv_main.style_transfer(PATHS, _cfg(content_size=120, style_size=80))
    assert rec.events == []
