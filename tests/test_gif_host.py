"""Timelapse GIF output, the parts that need no GPU: the palette cut, the Bayer matrix, the frame delay, the refusals, the
CLI / TOML surface, the wiring in ``main.style_transfer`` and in the runner, and the argument checks of the two entry points."""
from __future__ import annotations

import logging
from pathlib import Path

import numpy as np
import pytest
import torch

from style_transfer_visualizer_amd import _lib, cli, config_defaults, core_model, gif, image_io, optimization, runtime
from style_transfer_visualizer_amd import config as stv_config
from style_transfer_visualizer_amd import main as stv_main
from style_transfer_visualizer_amd.optimization import OptimizationCallbacks, OptimizationRunner
from style_transfer_visualizer_amd.type_defs import InputPaths
from tests import gif_ref

H, W = 96, 80


def _hist(frame: np.ndarray) -> np.ndarray:
    return gif_ref.frame_hist(frame)


def _random_fixture() -> np.ndarray:
    return np.random.default_rng(7).integers(64, 128, size=(H, W, 3)).astype(np.uint8)


def _gradient_fixture() -> np.ndarray:
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([x * 255 // (W - 1), y * 255 // (H - 1), (x + y) * 255 // (H + W - 2)], axis=2).astype(np.uint8)


def _palette_332() -> np.ndarray:
    """The uniform 3-3-2-bit palette: the cell centres of 8 x 8 x 4 equal cells."""
    r, g, b = np.meshgrid(np.arange(8) * 32 + 16, np.arange(8) * 32 + 16, np.arange(4) * 64 + 32, indexing="ij")
    return np.stack([r, g, b], axis=3).reshape(-1, 3).astype(np.uint8)


def _mse(frame: np.ndarray, palette: np.ndarray) -> float:
    idx = gif_ref.gif_map(frame, palette, 0)
    return float(((palette[idx].astype(np.int64) - frame.astype(np.int64)) ** 2).sum(axis=2).mean())


# ---- median_cut ------------------------------------------------------------------------------------------------------------

def test_median_cut_is_deterministic_and_bounded():
    hist = _hist(_random_fixture())
    for n in (2, 16, 255, 256):
        a, b = gif.median_cut(hist, n), gif.median_cut(hist.copy(), n)
        assert a.dtype == np.uint8 and a.ndim == 2 and a.shape[1] == 3 and 1 <= len(a) <= n
        assert np.array_equal(a, b)
    assert np.array_equal(gif.median_cut(hist.astype(np.uint32), 64), gif.median_cut(hist, 64))      # the device's counters


def test_few_occupied_cells_get_one_entry_each_at_the_cell_centre():
    rng = np.random.default_rng(3)
    cells = rng.choice(32768, size=200, replace=False)
    hist = np.zeros(32768, dtype=np.int64)
    hist[cells] = rng.integers(1, 1000, size=200)
    pal = gif.median_cut(hist, 256)
    want = {(8 * (c >> 10) + 4, 8 * ((c >> 5) & 31) + 4, 8 * (c & 31) + 4) for c in cells.tolist()}
    assert len(pal) == 200 and {tuple(int(v) for v in e) for e in pal} == want
    frame = np.zeros((4, 6, 3), dtype=np.uint8)
    frame[:, :3], frame[:, 3:] = (10, 200, 77), (250, 3, 129)
    two = gif.median_cut(_hist(frame), 256)
    assert len(two) == 2
    for colour in ((10, 200, 77), (250, 3, 129)):
        assert min(int(np.abs(e.astype(int) - np.array(colour)).max()) for e in two) <= 4


def test_a_grey_ramp_gives_32_entries():
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)
    pal = gif.median_cut(_hist(ramp), 256)
    assert len(pal) == 32 and sorted(int(e[0]) for e in pal) == [8 * c + 4 for c in range(32)]
    assert all(e[0] == e[1] == e[2] for e in pal)


def test_an_empty_histogram_and_bad_arguments_raise():
    with pytest.raises(ValueError, match="empty"):
        gif.median_cut(np.zeros(32768, dtype=np.int64), 256)
    with pytest.raises(ValueError, match="32768"):
        gif.median_cut(np.ones(100, dtype=np.int64), 256)
    with pytest.raises(ValueError, match="colours"):
        gif.median_cut(np.ones(32768, dtype=np.int64), 257)


@pytest.mark.parametrize("fixture", [_random_fixture, _gradient_fixture])
def test_the_cut_palette_beats_the_uniform_one_fourfold(fixture):
    """Measured with the rule as written: 29 against 659 (random), 61 against 848 (gradient)."""
    frame = fixture()
    pal = gif.median_cut(_hist(frame), 256)
    cut, uniform = _mse(frame, pal), _mse(frame, _palette_332())
    print(f"{fixture.__name__}: mse {cut:.1f} onto the cut palette ({len(pal)} entries), {uniform:.1f} onto 3-3-2")
    assert len(pal) == 256 and cut < uniform / 4


# ---- bayer8, the frame delay -----------------------------------------------------------------------------------------------

def test_bayer8_is_the_permutation_of_the_definition():
    b = gif.bayer8()
    assert b.shape == (8, 8) and sorted(b.reshape(-1).tolist()) == list(range(64))
    assert b[0, :4].tolist() == [0, 32, 8, 40] and b[1, :4].tolist() == [48, 16, 56, 24]
    assert np.array_equal(b, gif_ref.bayer8_recursive())
    offs = ((2 * b - 63) * gif.ORDERED_SPREAD) >> 7
    assert gif.ORDERED_SPREAD == 16 and offs.min() == -8 and offs.max() == 7


def test_frame_duration_table():
    assert [gif.frame_duration_cs(f) for f in (1, 10, 24, 30, 50, 100)] == [100, 10, 4, 3, 2, 2]
    with pytest.raises(ValueError):
        gif.frame_duration_cs(0)


# ---- refusals --------------------------------------------------------------------------------------------------------------

def test_the_budget_refusal_names_frames_size_bytes_and_budget():
    assert gif.GIF_MAX_DEVICE_BYTES == 4 << 30
    assert gif.check_budget(4096, 512, 512) == 4 << 30                     # exactly the budget passes
    with pytest.raises(ValueError) as err:
        gif.DeviceGifCollector("never.gif", 10, 1024, 768, 2000, device="cuda")       # refused before anything is allocated
    text = str(err.value)
    for part in ("2000 frames", "768x1024", str(2000 * 1024 * 768 * 4), str(4 << 30), "--save-every"):
        assert part in text, (part, text)


def test_config_refuses_bad_colours_and_dither(tmp_path):
    assert (config_defaults.DEFAULT_GIF_COLORS, config_defaults.DEFAULT_GIF_DITHER) == (256, "ordered")
    for bad in ({"gif_colors": 1}, {"gif_colors": 257}, {"gif_dither": "floyd"}):
        with pytest.raises(ValueError):
            stv_config.StyleTransferConfig.model_validate({"video": bad})
    for bad in (1, 257):
        with pytest.raises(ValueError):
            _cli_config([*BASE, "--gif-colors", str(bad)])
        with pytest.raises(ValueError, match="gif_colors"):
            gif.check_colors(bad)
    with pytest.raises(SystemExit):
        cli.build_arg_parser().parse_args([*BASE, "--gif-dither", "floyd"])
    with pytest.raises(ValueError, match="gif_dither"):
        gif.dither_spread("floyd")
    assert gif.dither_spread("none") == 0 and gif.dither_spread("ordered") == gif.ORDERED_SPREAD


# ---- CLI and TOML ----------------------------------------------------------------------------------------------------------

BASE = ["--content", "c.png", "--style", "s.png"]


def _cli_config(argv):
    args = cli.build_arg_parser().parse_args(argv)
    base = stv_config.ConfigLoader.load(args.config) if args.config else None
    return stv_config.build_config_from_cli(vars(args), base_config=base)


def test_cli_and_toml_round_trip(tmp_path, caplog):
    plain = _cli_config(BASE)
    assert (plain.video.gif_colors, plain.video.gif_dither, plain.video.create_gif) == (256, "ordered", False)
    cfg = _cli_config([*BASE, "--gif", "--gif-colors", "16", "--gif-dither", "none"])
    assert (cfg.video.create_gif, cfg.video.gif_colors, cfg.video.gif_dither) == (True, 16, "none")
    toml = tmp_path / "c.toml"
    toml.write_text('[video]\ncreate_gif = true\ngif_colors = 64\ngif_dither = "none"\n')
    from_toml = _cli_config([*BASE, "--config", str(toml)])
    assert (from_toml.video.create_gif, from_toml.video.gif_colors, from_toml.video.gif_dither) == (True, 64, "none")
    over = _cli_config([*BASE, "--config", str(toml), "--gif-colors", "8", "--gif-dither", "ordered"])          # the CLI wins
    assert (over.video.gif_colors, over.video.gif_dither) == (8, "ordered")
    paths = InputPaths("c.png", "s.png")
    with caplog.at_level(logging.INFO, logger="style_transfer"):
        cli.log_parameters(paths, cfg)
    assert "GIF Colors: 16" in caplog.text and "GIF Dither: none" in caplog.text
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="style_transfer"):
        cli.log_parameters(paths, plain)                                    # without --gif the rows stay away
    assert "GIF Colors" not in caplog.text and "GIF Dither" not in caplog.text


# ---- wiring in main.style_transfer (the fakes of tests/test_main.py) ----------------------------------------------------------

class _Recorder:
    def __init__(self):
        self.runner_args = None
        self.saved = None
        self.collectors = []


class _FakeCollector:
    def __init__(self, rec, path, fps, H, W, n_frames, **kw):
        self.args, self.kw, self.closed = (path, fps, H, W, n_frames), kw, 0
        rec.collectors.append(self)

    def close(self):
        self.closed += 1


@pytest.fixture
def wired(monkeypatch):
    rec = _Recorder()
    img = torch.linspace(-0.5, 1.5, 3 * 16 * 24).reshape(1, 3, 16, 24)
    rec.device = torch.device("cpu")
    monkeypatch.setattr(runtime, "validate_input_paths", lambda *a, **k: None)
    monkeypatch.setattr(runtime, "setup_random_seed", lambda seed: None)
    monkeypatch.setattr(runtime, "setup_device", lambda name: rec.device)
    monkeypatch.setattr(runtime, "setup_output_directory", lambda p: Path("mock_output"))
    monkeypatch.setattr(runtime, "save_outputs", lambda *a, **k: setattr(rec, "saved", a))
    monkeypatch.setattr(image_io, "load_image_to_tensor", lambda *a, **k: img.clone())
    monkeypatch.setattr(core_model, "prepare_model_and_input", lambda *a, **k: ("model", img.clone().requires_grad_(True), "optimizer"))
    monkeypatch.setattr(gif, "DeviceGifCollector", lambda *a, **k: _FakeCollector(rec, *a, **k))

    class FakeRunner:
        def __init__(self, *args, **kwargs):
            rec.runner_args = (args, kwargs)

        def run(self):
            return img.clone().requires_grad_(True), {"total_loss": [1.0]}, 3.14
    monkeypatch.setattr(optimization, "OptimizationRunner", FakeRunner)
    return rec


def _cfg(**video):
    cfg = stv_config.StyleTransferConfig.model_validate({})
    cfg.optimization.steps, cfg.optimization.seed = 10, 42
    cfg.video.create_video = False
    for k, v in video.items():
        setattr(cfg.video, k, v)
    return cfg


WARNING = "Timelapse encoding is not part of the MI355X build; continuing without video/GIF"


def test_gif_on_a_cpu_device_still_warns_and_downgrades(wired, caplog):
    cfg = _cfg(create_gif=True)
    with caplog.at_level(logging.WARNING, logger="style_transfer"):
        stv_main.style_transfer(InputPaths("a.png", "b.png"), cfg)
    assert sum(WARNING in m for m in caplog.messages) == 1
    assert cfg.video.create_gif is False and wired.runner_args[1]["gif_collector"] is None and not wired.collectors
    assert wired.saved[4].gif_created is False and wired.saved[4].gif_name is None


def test_a_video_request_still_warns_and_downgrades_next_to_the_built_in_gif(wired, caplog):
    wired.device = torch.device("cuda")
    cfg = _cfg(create_video=True, create_gif=True, save_every=3, fps=24, gif_colors=32, gif_dither="none")
    with caplog.at_level(logging.WARNING, logger="style_transfer"):
        stv_main.style_transfer(InputPaths("dir/a.png", "b.png"), cfg, output_tag="_007", tag_png=False)
    assert sum(WARNING in m for m in caplog.messages) == 1
    assert cfg.video.create_video is False and cfg.video.create_gif is True
    (col,) = wired.collectors
    assert col.args == (Path("mock_output") / "timelapse_a_x_b_007.gif", 24, 16, 24, 3)          # 10 // 3 frames of the run's size
    assert col.kw == {"colors": 32, "dither": "none", "device": torch.device("cuda")}
    assert wired.runner_args[1]["gif_collector"] is col and wired.runner_args[1]["video_writer"] is None and col.closed == 1
    opts = wired.saved[4]
    assert opts.gif_created is True and opts.gif_name == "timelapse_a_x_b_007.gif" and opts.video_created is False


def test_the_built_in_collector_needs_no_warning_and_an_injected_one_wins(wired, caplog):
    wired.device = torch.device("cuda")
    with caplog.at_level(logging.WARNING, logger="style_transfer"):
        stv_main.style_transfer(InputPaths("a.png", "b.png"), _cfg(create_gif=True))
    assert not caplog.messages and len(wired.collectors) == 1
    assert wired.saved[4].gif_name == "timelapse_a_x_b.gif"

    class Sink:
        closed = 0

        def append_data(self, frame):
            pass

        def close(self):
            self.closed += 1
    sink = Sink()
    stv_main.style_transfer(InputPaths("a.png", "b.png"), _cfg(create_gif=True), gif_collector=sink)
    assert len(wired.collectors) == 1 and wired.runner_args[1]["gif_collector"] is sink and sink.closed == 1
    assert wired.saved[4].gif_created is True and wired.saved[4].gif_name is None


def test_intro_and_outro_flags_give_one_warning_with_the_built_in_collector(wired, caplog):
    wired.device = torch.device("cuda")
    with caplog.at_level(logging.WARNING, logger="style_transfer"):
        stv_main.style_transfer(InputPaths("a.png", "b.png"), _cfg(create_gif=True, gif_include_intro=True, gif_include_outro=True))
    (message,) = caplog.messages
    assert "gif_include_intro" in message and "gif_include_outro" in message and len(wired.collectors) == 1


def test_final_only_and_a_pyramid_keep_the_built_in_collector_away(wired, caplog, monkeypatch):
    wired.device = torch.device("cuda")
    stv_main.style_transfer(InputPaths("a.png", "b.png"), _cfg(create_gif=True, final_only=True))
    assert not wired.collectors and wired.saved[4].gif_created is False
    from style_transfer_visualizer_amd import pyramid
    seen = {}

    def fake_pyramid(*a, **k):
        seen.update(k)
        return torch.zeros(1, 3, 16, 24), {}, 0.0
    monkeypatch.setattr(pyramid, "run_pyramid", fake_pyramid)
    cfg = _cfg(create_gif=True)
    cfg.optimization.pyramid_levels = 2
    with caplog.at_level(logging.WARNING, logger="style_transfer"):
        stv_main.style_transfer(InputPaths("a.png", "b.png"), cfg)
    assert sum(WARNING in m for m in caplog.messages) == 1 and cfg.video.create_gif is False
    assert not wired.collectors and seen["gif_collector"] is None


def test_the_budget_refusal_comes_before_the_model(wired, monkeypatch):
    wired.device = torch.device("cuda")
    big = torch.empty(1, 3, 4096, 4096)                    # (never read: only its shape counts)
    monkeypatch.setattr(image_io, "load_image_to_tensor", lambda *a, **k: big)
    cfg = _cfg(create_gif=True, save_every=1)
    cfg.optimization.steps = 100
    with pytest.raises(ValueError, match="100 frames of 4096x4096"):
        stv_main.style_transfer(InputPaths("a.png", "b.png"), cfg)
    assert wired.runner_args is None and not wired.collectors


def test_save_outputs_logs_the_gif_only_when_the_file_exists(tmp_path, caplog, monkeypatch):
    from style_transfer_visualizer_amd.type_defs import SaveOptions
    monkeypatch.setattr(image_io, "save_image", lambda *a, **k: None)
    opts = SaveOptions(content_name="a", style_name="b", video_created=False, gif_name="t.gif", gif_created=True, plot_losses=False)
    with caplog.at_level(logging.INFO, logger="style_transfer"):
        runtime.save_outputs(torch.zeros(1, 3, 4, 4), {}, tmp_path, 1.0, opts)
    assert "GIF saved to" not in caplog.text
    (tmp_path / "t.gif").write_bytes(b"GIF89a")
    with caplog.at_level(logging.INFO, logger="style_transfer"):
        runtime.save_outputs(torch.zeros(1, 3, 4, 4), {}, tmp_path, 1.0, opts)
    assert f"GIF saved to: {tmp_path / 't.gif'}" in caplog.text


# ---- the runner: a sink with append_device gets the image, no host frame is formed ----------------------------------------------

class _TinyModel(torch.nn.Module):
    def forward(self, x):
        return [(x ** 2).mean()], [((x + 0.5) ** 2).mean()]


class _Bar:
    def update(self, n=1):
        return None

    def set_postfix(self, *a, **k):
        return None

    def close(self):
        return None


class _DeviceSink:
    def __init__(self):
        self.device_calls, self.host_frames = [], []

    def append_device(self, image, *, normalize):
        self.device_calls.append((tuple(image.shape), normalize))

    def append_data(self, frame):
        self.host_frames.append(frame)

    def close(self):
        return None


def _runner(sink, *, steps=7, save_every=2, **kw):
    cfg = stv_config.StyleTransferConfig.model_validate({})
    cfg.optimization.steps, cfg.optimization.normalize = steps, False
    cfg.video.save_every, cfg.output.log_every = save_every, 2
    x = torch.full((1, 3, 8, 8), 0.25, requires_grad=True)
    return OptimizationRunner(_TinyModel(), x, cfg, optimizer=torch.optim.Adam([x]), progress_bar=_Bar(), gif_collector=sink, **kw)


def test_a_device_sink_alone_needs_no_host_frame(monkeypatch):
    def forbidden(*a, **k):
        raise AssertionError("a host frame was formed")
    monkeypatch.setattr(image_io, "frame_uint8", forbidden)
    sink = _DeviceSink()
    _runner(sink).run()
    assert sink.device_calls == [((1, 3, 8, 8), False)] * (7 // 2) and not sink.host_frames


def test_a_callback_or_a_writer_brings_the_host_frame_back(monkeypatch):
    calls = []
    real = image_io.frame_uint8
    monkeypatch.setattr(image_io, "frame_uint8", lambda *a, **k: calls.append(1) or real(*a, **k))
    sink, seen = _DeviceSink(), []
    _runner(sink, callbacks=OptimizationCallbacks(on_video_frame=lambda frame, step: seen.append((frame.shape, step)))).run()
    assert len(calls) == 3 and seen == [((8, 8, 3), 2), ((8, 8, 3), 4), ((8, 8, 3), 6)]
    assert len(sink.device_calls) == 3 and not sink.host_frames          # the device sink is not handed the host frame too

    class Writer:
        def __init__(self):
            self.frames = []

        def append_data(self, frame):
            self.frames.append(frame)

        def close(self):
            return None
    writer, sink = Writer(), _DeviceSink()
    _runner(sink, video_writer=writer).run()
    assert len(writer.frames) == 3 and len(sink.device_calls) == 3 and not sink.host_frames


# ---- ABI -------------------------------------------------------------------------------------------------------------------

def test_both_entry_points_refuse_bad_arguments_before_any_device_work():
    lib = _lib.load()
    assert lib.stv_version() >= 115
    ERR, P = 1, 0x1000          # (a non-null address: never dereferenced, the checks come first)
    assert lib.stv_frame_hist(None, 16, P, None) == ERR and lib.stv_frame_hist(P, 16, None, None) == ERR
    assert lib.stv_frame_hist(P, 0, P, None) == ERR
    assert lib.stv_frame_hist(P, (1 << 31) // 3 + 1, P, None) == ERR          # 3 * n >= 2 GiB
    good = dict(H=8, W=8, n=256, spread=16)

    def gif_map(frame=P, index=P, palette=P, **kw):
        a = {**good, **kw}
        return lib.stv_gif_map(frame, index, a["H"], a["W"], palette, a["n"], a["spread"], None)
    assert gif_map(frame=None) == ERR and gif_map(index=None) == ERR and gif_map(palette=None) == ERR
    assert gif_map(H=0) == ERR and gif_map(W=0) == ERR and gif_map(H=-3) == ERR
    assert gif_map(n=0) == ERR and gif_map(n=257) == ERR
    assert gif_map(spread=-1) == ERR and gif_map(spread=65) == ERR
    assert gif_map(H=32768, W=21846) == ERR                                     # H*W*3 >= 2 GiB
    assert (_lib.GIF_THREADS, _lib.GIF_MAX_BLOCKS, _lib.GIF_VEC, _lib.GIF_HIST_BINS) == (256, 2048, 4, 32768)
