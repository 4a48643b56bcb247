"""``--video-format mjpeg`` through ``main.style_transfer`` on a real MI355X: 64x64 PNG inputs, synthetic VGG19 weights, fp32,
6 steps, a frame every 2.  There is no golden file (the reference's video path needs ffmpeg); the independent checks are PIL's
decoder and the host pipeline - the twins of tests/jpeg_ref.py, ``mjpeg.jpeg_headers`` and ``mjpeg.stuff`` - applied to the host
frames of a second, identical run with an injected memory sink (runs are deterministic: README, pyramid section).  Every
``00dc`` chunk of the file must equal that pipeline's JPEG byte for byte."""
from __future__ import annotations

import copy
import io

import numpy as np
import pytest
import torch
from PIL import Image

from style_transfer_visualizer_amd import core_model, image_io, main, mjpeg, optimization, runtime
from style_transfer_visualizer_amd import config as stv_config
from style_transfer_visualizer_amd.optimizers import HipAdam, HipLBFGS
from style_transfer_visualizer_amd.type_defs import InputPaths
from tests import color_ref as cr
from tests import jpeg_ref as jr

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


def _config(out_dir, *, video: bool, fmt: str = "mjpeg", quality: int = 10, create_gif: bool = False):
    cfg = stv_config.StyleTransferConfig.model_validate({})
    oc = cfg.optimization
    oc.steps, oc.init_method, oc.seed = STEPS, "random", 0
    cfg.hardware.device, cfg.hardware.precision = "cuda", "fp32"
    v = cfg.video
    v.create_video, v.format, v.quality, v.create_gif, v.save_every, v.fps = video, fmt, quality, create_gif, EVERY, FPS
    v.intro_enabled, v.final_frame_compare = False, False
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
    folder = tmp_path_factory.mktemp("mjpeg")
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("STV_SYNTHETIC_WEIGHTS", "0")
        paths = InputPaths(content_path=_png(folder, "content", 0), style_path=_png(folder, "style", 1))
        off_image, off_losses = _main_run(paths, _config(folder / "off", video=False), mp)
        sink = MemorySink()
        host_image, host_losses = _main_run(paths, _config(folder / "host", video=True), mp, video_writer=sink)
        assert sink.closed == 1 and len(sink.frames) == FRAMES and sink.frames[0].shape == (SIDE, SIDE, 3)
        assert not np.array_equal(sink.frames[0], sink.frames[-1])               # the run moves the image
        assert torch.equal(host_image, off_image) and host_losses == off_losses
        yield {"folder": folder, "paths": paths, "frames": sink.frames, "image": off_image, "losses": off_losses}


@pytest.fixture(autouse=True)
def _synthetic(monkeypatch):
    monkeypatch.setenv("STV_SYNTHETIC_WEIGHTS", "0")


def _check_file(path, frames: list[np.ndarray], quality: int) -> None:
    qtabs = mjpeg.quant_tables(mjpeg.jpeg_quality(quality))
    avi = jr.read_avi(path.read_bytes())
    assert avi["avih"][4] == len(frames) and avi["strh"][1][5] == FPS and avi["strh"][1][4] == 1
    assert len(avi["frames"]) == len(frames) == len(avi["index"])
    for k, (chunk, frame) in enumerate(zip(avi["frames"], frames, strict=True)):
        want = jr.encode_frame(frame, qtabs)
        assert chunk["data"] == want, f"frame {k}: {len(chunk['data'])} bytes against {len(want)}"
        with Image.open(io.BytesIO(chunk["data"])) as im:
            im.load()
            assert im.size == (SIDE, SIDE)


@pytest.mark.parametrize(("quality", "with_gif"), [(10, False), (3, False), (10, True)])
def test_the_file_equals_the_host_pipeline_on_the_host_frames(world, monkeypatch, quality, with_gif):
    out = world["folder"] / f"avi_{quality}_{with_gif}"
    image, losses = _main_run(world["paths"], _config(out, video=True, quality=quality, create_gif=with_gif), monkeypatch)
    (path,) = list(out.glob("timelapse_*.avi"))
    assert path.name == "timelapse_content_x_style.avi"
    _check_file(path, world["frames"], quality)
    avi = jr.read_avi(path.read_bytes())
    assert avi["info"][b"INAM"] == mjpeg.DEFAULT_TITLE and avi["info"][b"IART"] == mjpeg.DEFAULT_ARTIST
    # frames on change nothing in the run: the same image and the same loss history, bit for bit
    assert torch.equal(image, world["image"]) and losses == world["losses"]
    gifs = list(out.glob("timelapse_*.gif"))
    assert len(gifs) == (1 if with_gif else 0)
    if with_gif:                                                # both files; the GIF is the one a run without the video writes
        alone = world["folder"] / "gif_alone"
        _main_run(world["paths"], _config(alone, video=False, create_gif=True), monkeypatch)
        assert gifs[0].read_bytes() == (alone / "timelapse_content_x_style.gif").read_bytes()


def test_mp4_enters_nothing_new(world, monkeypatch, caplog):
    """``format = mp4``: the request is downgraded as before - no writer, no file, the program key and the bits of a run with
    the video off."""
    keys = []
    real = optimization.OptimizationRunner.run

    def spy(self):
        out = real(self)
        (engine,) = self.model._engines.values()
        # (without the addresses: the image, its gradient, the score log and the optimizer's state are new tensors per run)
        keys.append(sorted((k[0], k[3], k[4], k[5] is None, k[6] is None, k[7:]) for k in engine._programs if k[0] == "fused"))
        return out
    monkeypatch.setattr(optimization.OptimizationRunner, "run", spy)
    monkeypatch.setattr(mjpeg, "DeviceMjpegWriter", lambda *a, **k: pytest.fail("the MJPEG writer was created"))
    out = world["folder"] / "mp4"
    with caplog.at_level("WARNING", logger="style_transfer"):
        image, losses = _main_run(world["paths"], _config(out, video=True, fmt="mp4"), monkeypatch)
    assert sum("Timelapse encoding is not part of the MI355X build" in m for m in caplog.messages) == 1
    assert not list(out.glob("*.avi")) and torch.equal(image, world["image"]) and losses == world["losses"]
    _main_run(world["paths"], _config(world["folder"] / "off_again", video=False), monkeypatch)
    assert len(keys) == 2 and keys[0] == keys[1] and keys[0]          # the same programs under the same keys


def _by_hand(world, which: str, sink) -> torch.Tensor:
    """The run as ``main`` composes it, with the optimizer chosen here and ``sink`` as the video writer."""
    cfg = _config(world["folder"] / "unused", video=True)
    content = image_io.load_image_to_tensor(world["paths"].content_path, DEV, normalize=True)
    style = image_io.load_image_to_tensor(world["paths"].style_path, DEV, normalize=True)
    runtime.setup_random_seed(0)
    model, x, opt = core_model.prepare_model_and_input(content, style, DEV, cfg.optimization, precision="fp32")
    if which == "adam":
        opt = HipAdam([x], lr=2e-2)
    else:
        assert isinstance(opt, HipLBFGS) and opt.evals_per_step == 1
    x, _, _ = optimization.OptimizationRunner(model, x, cfg, optimizer=opt, progress_bar=_Bar(), video_writer=sink).run()
    sink.close()
    return x.detach().clone()


@pytest.mark.parametrize("which", ["lbfgs", "adam"])
def test_the_writer_under_both_optimizers(world, which):
    path = world["folder"] / f"hand_{which}.avi"
    writer = mjpeg.DeviceMjpegWriter(path, FPS, SIDE, SIDE, FRAMES, quality=3, device=DEV)
    x_dev = _by_hand(world, which, writer)
    sink = MemorySink()
    x_host = _by_hand(world, which, sink)
    assert torch.equal(x_dev, x_host) and len(sink.frames) == FRAMES
    if which == "lbfgs":                                                        # the run main makes
        assert all(np.array_equal(a, b) for a, b in zip(sink.frames, world["frames"], strict=True))
    _check_file(path, sink.frames, 3)
    assert writer.frames_written == FRAMES and writer.file_bytes == path.stat().st_size
    assert set(writer.timings) == {"bits_scan_s", "emit_s", "copy_s", "stuff_s", "avi_s"}


def test_writer_limits_batches_and_close(world, monkeypatch):
    folder = world["folder"]
    image = image_io.load_image_to_tensor(world["paths"].content_path, DEV, normalize=True)
    monkeypatch.setattr(mjpeg, "EMIT_BATCH_BYTES", 4096)                         # several emit batches for three small frames
    writer = mjpeg.DeviceMjpegWriter(folder / "limits.avi", FPS, SIDE, SIDE, 3, device=DEV)
    for _ in range(2):
        writer.append_device(image, normalize=True)
    writer.append_data(world["frames"][0])                                       # the FrameSink route fills a slot too
    with pytest.raises(RuntimeError, match="frame 4 appended to a store of 3"):
        writer.append_device(image, normalize=True)
    with pytest.raises(RuntimeError, match="store of 3"):
        writer.append_data(world["frames"][0])
    with pytest.raises(RuntimeError, match="a frame of"):
        mjpeg.DeviceMjpegWriter(folder / "never.avi", FPS, SIDE, SIDE + 1, 1, device=DEV).append_device(image, normalize=True)
    writer.close()
    stamp = (folder / "limits.avi").stat().st_mtime_ns
    writer.close()                                                               # harmless: nothing is written again
    assert (folder / "limits.avi").stat().st_mtime_ns == stamp
    with pytest.raises(RuntimeError, match="after close"):
        writer.append_device(image, normalize=True)
    first = image_io.frame_uint8(image, normalize=True)
    _check_file(folder / "limits.avi", [first, first, world["frames"][0]], 10)
    sizes = [c["size"] for c in jr.read_avi((folder / "limits.avi").read_bytes())["frames"]]
    assert sum(sizes) > 2 * 4096                                                 # the batches were split indeed
    empty = mjpeg.DeviceMjpegWriter(folder / "empty.avi", FPS, SIDE, SIDE, 3, device=DEV)
    empty.close()
    none = mjpeg.DeviceMjpegWriter(folder / "none.avi", FPS, SIDE, SIDE, 0, device=DEV)           # steps < save_every
    none.close()
    assert not (folder / "empty.avi").exists() and not (folder / "none.avi").exists()
