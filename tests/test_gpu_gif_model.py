"""``--gif`` through ``main.style_transfer`` on a real MI355X: 64x64 PNG inputs, synthetic VGG19 weights, fp32, 6 steps, a
frame every 2.  There is no golden file (the reference's GIF path needs imageio); the independent checks are PIL's decoder
and the host pipeline - ``np.bincount``, ``gif.median_cut`` and the map twin of tests/gif_ref.py - applied to the host
frames of a second, identical run with an injected memory sink (runs are deterministic: README, pyramid section).  The
palette lookup of that pipeline must equal every decoded frame of the file exactly."""
from __future__ import annotations

import copy

import numpy as np
import pytest
import torch
from PIL import Image

from style_transfer_visualizer_amd import core_model, gif, image_io, main, optimization, runtime
from style_transfer_visualizer_amd import config as stv_config
from style_transfer_visualizer_amd.optimizers import HipAdam, HipLBFGS
from style_transfer_visualizer_amd.type_defs import InputPaths
from tests import color_ref as cr
from tests import gif_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SIDE, STEPS, EVERY, FPS = 64, 6, 2, 10
FRAMES = STEPS // EVERY


class _Bar:
    def update(self, n=1):
        return None

    def set_postfix(self, *a, **k):
        return None

    def close(self):
        return None


class MemorySink:
    def __init__(self):
        self.frames, self.closed = [], 0

    def append_data(self, frame):
        self.frames.append(np.array(frame, dtype=np.uint8))

    def close(self):
        self.closed += 1


def _png(folder, name: str, seed: int) -> str:
    rgb = cr.uint8_image(SIDE, SIDE, seed, normalize=False)[0].transpose(1, 2, 0)
    Image.fromarray(np.round(rgb * 255.0).astype(np.uint8)).save(folder / f"{name}.png")
    return str(folder / f"{name}.png")


def _config(out_dir, *, create_gif: bool, colors: int = 256, dither: str = "ordered"):
    cfg = stv_config.StyleTransferConfig.model_validate({})
    oc = cfg.optimization
    oc.steps, oc.init_method, oc.seed = STEPS, "random", 0
    cfg.hardware.device, cfg.hardware.precision = "cuda", "fp32"
    v = cfg.video
    v.create_video, v.create_gif, v.save_every, v.fps, v.gif_colors, v.gif_dither = False, create_gif, EVERY, FPS, colors, dither
    cfg.output.output, cfg.output.plot_losses, cfg.output.log_every = str(out_dir), False, 1
    return cfg


def _main_run(paths, cfg, monkeypatch, **kw):
    """``main.style_transfer`` with the loss history it hands to the save step; returns (image, history)."""
    seen = {}
    real = runtime.save_outputs

    def spy(input_img, loss_metrics, *a, **k):
        seen["losses"] = copy.deepcopy(loss_metrics)
        return real(input_img, loss_metrics, *a, **k)
    monkeypatch.setattr(runtime, "save_outputs", spy)
    image = main.style_transfer(paths, cfg, **kw).clone()
    monkeypatch.setattr(runtime, "save_outputs", real)
    return image, seen["losses"]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The inputs, and the two reference runs every test shares: frames off, and an injected host memory sink."""
    folder = tmp_path_factory.mktemp("gif")
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("STV_SYNTHETIC_WEIGHTS", "0")
        paths = InputPaths(content_path=_png(folder, "content", 0), style_path=_png(folder, "style", 1))
        off_image, off_losses = _main_run(paths, _config(folder / "off", create_gif=False), mp)
        sink = MemorySink()
        host_image, host_losses = _main_run(paths, _config(folder / "host", create_gif=True), mp, gif_collector=sink)
        assert sink.closed == 1 and len(sink.frames) == FRAMES and sink.frames[0].shape == (SIDE, SIDE, 3)
        assert not np.array_equal(sink.frames[0], sink.frames[-1])               # the run moves the image
        assert torch.equal(host_image, off_image) and host_losses == off_losses
        yield {"folder": folder, "paths": paths, "frames": sink.frames, "image": off_image, "losses": off_losses}


@pytest.fixture(autouse=True)
def _synthetic(monkeypatch):
    monkeypatch.setenv("STV_SYNTHETIC_WEIGHTS", "0")


def _decode(path) -> tuple[list[np.ndarray], list[int], int]:
    """Frames of the file as RGB arrays, expanded by their durations (PIL merges identical consecutive frames by adding
    their delays), the delays of the stored frames in ms, and the loop count."""
    cs = gif.frame_duration_cs(FPS)
    frames, delays = [], []
    with Image.open(path) as im:
        loop = im.info.get("loop")
        for i in range(im.n_frames):
            im.seek(i)
            delay = int(im.info["duration"])
            delays.append(delay)
            assert delay % (10 * cs) == 0
            frames += [np.array(im.convert("RGB"))] * (delay // (10 * cs))
    return frames, delays, loop


def _host_pipeline(frames: list[np.ndarray], colors: int, spread: int) -> list[np.ndarray]:
    hist = sum(gif_ref.frame_hist(f) for f in frames)
    palette = gif.median_cut(hist, colors)
    return [palette[gif_ref.gif_map(f, palette, spread)] for f in frames]


@pytest.mark.parametrize(("colors", "dither"), [(256, "ordered"), (256, "none"), (16, "ordered")])
def test_the_file_equals_the_host_pipeline_on_the_host_frames(world, monkeypatch, colors, dither):
    out = world["folder"] / f"gif_{colors}_{dither}"
    image, losses = _main_run(world["paths"], _config(out, create_gif=True, colors=colors, dither=dither), monkeypatch)
    (path,) = list(out.glob("timelapse_*.gif"))
    assert path.name == "timelapse_content_x_style.gif"
    frames, delays, loop = _decode(path)
    assert len(frames) == FRAMES and sum(delays) == FRAMES * 100 and loop == 0          # 10 fps: 10 cs per frame
    want = _host_pipeline(world["frames"], colors, gif.dither_spread(dither))
    for k in range(FRAMES):
        assert frames[k].shape == (SIDE, SIDE, 3)
        assert np.array_equal(frames[k], want[k]), f"frame {k}: {int((frames[k] != want[k]).any(axis=2).sum())} pixels differ"
    assert len({tuple(c) for f in frames for c in f.reshape(-1, 3)}) <= colors
    # frames on change nothing in the run: the same image and the same loss history, bit for bit
    assert torch.equal(image, world["image"]) and losses == world["losses"]


def _by_hand(world, which: str, sink) -> torch.Tensor:
    """The run as ``main`` composes it, with the optimizer chosen here and ``sink`` as the GIF collector."""
    cfg = _config(world["folder"] / "unused", create_gif=True)
    content = image_io.load_image_to_tensor(world["paths"].content_path, DEV, normalize=True)
    style = image_io.load_image_to_tensor(world["paths"].style_path, DEV, normalize=True)
    runtime.setup_random_seed(0)
    model, x, opt = core_model.prepare_model_and_input(content, style, DEV, cfg.optimization, precision="fp32")
    if which == "adam":
        opt = HipAdam([x], lr=2e-2)
    else:
        assert isinstance(opt, HipLBFGS) and opt.evals_per_step == 1
    x, _, _ = optimization.OptimizationRunner(model, x, cfg, optimizer=opt, progress_bar=_Bar(), gif_collector=sink).run()
    sink.close()
    return x.detach().clone()


@pytest.mark.parametrize("which", ["lbfgs", "adam"])
def test_the_collector_under_both_optimizers(world, which):
    path = world["folder"] / f"hand_{which}.gif"
    collector = gif.DeviceGifCollector(path, FPS, SIDE, SIDE, FRAMES, colors=256, dither="ordered", device=DEV)
    x_dev = _by_hand(world, which, collector)
    sink = MemorySink()
    x_host = _by_hand(world, which, sink)
    assert torch.equal(x_dev, x_host) and len(sink.frames) == FRAMES
    if which == "lbfgs":                                                        # the run main makes
        assert all(np.array_equal(a, b) for a, b in zip(sink.frames, world["frames"], strict=True))
    frames, _, loop = _decode(path)
    want = _host_pipeline(sink.frames, 256, gif.ORDERED_SPREAD)
    assert len(frames) == FRAMES and loop == 0
    assert all(np.array_equal(a, b) for a, b in zip(frames, want, strict=True))
    assert collector.palette is not None and len(collector.palette) <= 256 and set(collector.timings) == {
        "readback_s", "median_cut_s", "map_s", "copy_s", "encode_s"}


def test_collector_limits_and_close(world):
    folder = world["folder"]
    image = image_io.load_image_to_tensor(world["paths"].content_path, DEV, normalize=True)
    col = gif.DeviceGifCollector(folder / "limits.gif", FPS, SIDE, SIDE, 3, device=DEV)
    for _ in range(2):
        col.append_device(image, normalize=True)
    col.append_data(world["frames"][0])                                          # the FrameSink route fills a slot too
    with pytest.raises(RuntimeError, match="frame 4 appended to a store of 3"):
        col.append_device(image, normalize=True)
    with pytest.raises(RuntimeError, match="store of 3"):
        col.append_data(world["frames"][0])
    with pytest.raises(RuntimeError, match="a frame of"):
        gif.DeviceGifCollector(folder / "never.gif", FPS, SIDE, SIDE + 1, 1, device=DEV).append_device(image, normalize=True)
    col.close()
    stamp = (folder / "limits.gif").stat().st_mtime_ns
    col.close()                                                                 # harmless: nothing is written again
    assert (folder / "limits.gif").stat().st_mtime_ns == stamp
    with pytest.raises(RuntimeError, match="after close"):
        col.append_device(image, normalize=True)
    frames, delays, _ = _decode(folder / "limits.gif")
    assert len(frames) == 3 and np.array_equal(frames[0], frames[1])           # two captures of one image: merged, delays added
    want = _host_pipeline([image_io.frame_uint8(image, normalize=True)] * 2 + [world["frames"][0]], 256, gif.ORDERED_SPREAD)
    assert all(np.array_equal(a, b) for a, b in zip(frames, want, strict=True))
    empty = gif.DeviceGifCollector(folder / "empty.gif", FPS, SIDE, SIDE, 3, device=DEV)
    empty.close()
    none = gif.DeviceGifCollector(folder / "none.gif", FPS, SIDE, SIDE, 0, device=DEV)           # steps < save_every
    none.close()
    assert not (folder / "empty.gif").exists() and not (folder / "none.gif").exists()
