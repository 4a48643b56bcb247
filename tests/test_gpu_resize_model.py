"""--content-size / --style-size / --style-scale through ``main.style_transfer`` on a real MI355X: synthetic VGG19 weights,
PNG inputs, 3 steps, fp32 and bf16.  Runs are deterministic (README, pyramid section), so a run composed in the test from
``ops.resize``, ``prepare_model_and_input`` and ``OptimizationRunner`` (or ``run_pyramid``) on the loaded tensors is the
reference for the run ``main`` makes from the PNGs: bit for bit.
"""
from __future__ import annotations

import copy

import numpy as np
import pytest
import torch
from PIL import Image

from style_transfer_visualizer_amd import core_model, image_io, main, ops, optimization, pyramid, runtime
from style_transfer_visualizer_amd import config as stv_config
from style_transfer_visualizer_amd.type_defs import InputPaths
from tests import color_ref as cr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
PRECISIONS = ["fp32", "bf16"]
MEAN_BOUND, COV_BOUND = 1e-6, 1e-6        # the bounds tests/test_gpu_color_model.py holds the match to: the same op, other tensors


class _Bar:
    def update(self, n=1):
        return None

    def set_postfix(self, *a, **k):
        return None

    def close(self):
        return None


def _png(folder, name: str, seed: int, H: int, W: int) -> str:
    rgb = cr.uint8_image(H, W, seed, normalize=False)[0].transpose(1, 2, 0)         # correlated channels, full colour rank
    Image.fromarray(np.round(rgb * 255.0).astype(np.uint8)).save(folder / f"{name}.png")
    return str(folder / f"{name}.png")


@pytest.fixture
def inputs(tmp_path, monkeypatch):
    """PNGs by (H, W): content 100x150 (150 wide), style 90x120, and the pair of the coarse-to-fine test."""
    monkeypatch.setenv("STV_SYNTHETIC_WEIGHTS", "0")
    return {"content": _png(tmp_path, "content", 0, 100, 150), "style": _png(tmp_path, "style", 1, 90, 120),
            "content300": _png(tmp_path, "content300", 2, 200, 300), "content301": _png(tmp_path, "content301", 2, 201, 300),
            "style160": _png(tmp_path, "style160", 3, 140, 160), "out": tmp_path}


def _config(out_dir, precision: str, *, levels: int = 1, **resize):
    cfg = stv_config.StyleTransferConfig.model_validate({})
    oc = cfg.optimization
    oc.steps, oc.pyramid_levels, oc.init_method, oc.seed = 3, levels, "random", 0
    for key, value in resize.items():
        setattr(oc, key, value)
    cfg.hardware.device, cfg.hardware.precision = "cuda", precision
    cfg.video.create_video, cfg.video.final_only = False, True
    cfg.output.output, cfg.output.plot_losses, cfg.output.log_every = str(out_dir / "out"), False, 1
    return cfg


def _load(path: str) -> torch.Tensor:
    return image_io.load_image_to_tensor(path, DEV, normalize=True)


def _by_hand(content: torch.Tensor, style: torch.Tensor, cfg) -> torch.Tensor:
    """The single-level run as ``main`` composes it, on tensors."""
    runtime.setup_random_seed(cfg.optimization.seed)
    model, x, opt = core_model.prepare_model_and_input(content, style, DEV, cfg.optimization, precision=cfg.hardware.precision)
    ref = copy.deepcopy(cfg)
    ref.video.save_every = ref.optimization.steps + 1                    # what final_only makes of it in main
    x, _, _ = optimization.OptimizationRunner(model, x, ref, optimizer=opt, progress_bar=_Bar()).run()
    torch.cuda.synchronize()
    return x.detach().clamp(0, 1)


def _forbid(monkeypatch, *names) -> None:
    def forbidden(*a, **k):
        raise AssertionError("the run reached the device")
    for owner, name in names:
        monkeypatch.setattr(owner, name, forbidden)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_png_run_equals_the_run_on_resized_tensors(inputs, precision):
    cfg = _config(inputs["out"], precision, content_size=96, style_scale=1.0)
    got = main.style_transfer(InputPaths(content_path=inputs["content"], style_path=inputs["style"]), copy.deepcopy(cfg))
    assert tuple(got.shape) == (1, 3, 64, 96)
    content, style = ops.resize(_load(inputs["content"]), (64, 96)), ops.resize(_load(inputs["style"]), (72, 96))
    assert tuple(content.shape) == (1, 3, 64, 96) and tuple(style.shape) == (1, 3, 72, 96)
    want = _by_hand(content, style, cfg)
    assert torch.equal(got, want), f"max |diff| {float((got - want).abs().max()):.3e}"
    (png,) = list((inputs["out"] / "out").glob("stylized_*.png"))
    assert np.array(Image.open(png)).shape == (64, 96, 3)
    other = main.style_transfer(InputPaths(content_path=inputs["content"], style_path=inputs["style"]),
                                _config(inputs["out"], precision, content_size=96, style_scale=1.0, resize_filter="bilinear"))
    assert tuple(other.shape) == (1, 3, 64, 96) and not torch.equal(other, got)         # the filter reaches the kernel


@pytest.mark.parametrize("precision", PRECISIONS)
def test_content_size_makes_any_content_fit_a_coarse_to_fine_run(inputs, precision):
    cfg = _config(inputs["out"], precision, levels=2, content_size=260)
    paths = InputPaths(content_path=inputs["content300"], style_path=inputs["style160"])
    got = main.style_transfer(paths, copy.deepcopy(cfg))
    assert tuple(got.shape) == (1, 3, 174, 260)
    content = ops.resize(_load(inputs["content300"]), (174, 260))
    ref = copy.deepcopy(cfg)
    ref.video.save_every = ref.optimization.steps + 1                    # what final_only makes of it in main
    image, _, _ = pyramid.run_pyramid(content, _load(inputs["style160"]), DEV, ref, progress_bar=_Bar(), seed=cfg.optimization.seed)
    torch.cuda.synchronize()
    want = image.detach().clamp(0, 1)
    assert torch.equal(got, want), f"max |diff| {float((got - want).abs().max()):.3e}"
    # without --content-size the pyramid's own refusal stands, and with it 300x201 runs
    odd = InputPaths(content_path=inputs["content301"], style_path=inputs["style160"])
    with pytest.raises(ValueError, match=r"content height 201 is not divisible by 2"):
        main.style_transfer(odd, _config(inputs["out"], precision, levels=2))
    assert tuple(main.style_transfer(odd, copy.deepcopy(cfg)).shape) == (1, 3, 174, 260)


def test_a_style_size_below_the_minimum_is_refused_before_any_launch(inputs, monkeypatch):
    _forbid(monkeypatch, (ops, "resize"), (core_model, "prepare_model_and_input"), (core_model, "StyleContentModel"))
    paths = InputPaths(content_path=inputs["content"], style_path=inputs["style"])
    with pytest.raises(ValueError, match=r"style_size = 80 resizes the style image from 120x90 to 80x60; the minimum dimension is 64"):
        main.style_transfer(paths, _config(inputs["out"], "fp32", content_size=96, style_size=80))
    with pytest.raises(ValueError, match=r"style_size = 80 and style_scale = 1 both"):
        main.style_transfer(paths, _config(inputs["out"], "fp32", style_size=80, style_scale=1.0))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_match_gives_the_style_the_colour_moments_of_the_resized_content(inputs, precision, monkeypatch):
    seen = []
    real = core_model.StyleContentModel.set_targets

    def set_targets(self, style_img, content_img):
        seen.append((style_img.detach().clone(), content_img.detach().clone()))
        return real(self, style_img, content_img)
    monkeypatch.setattr(core_model.StyleContentModel, "set_targets", set_targets)
    cfg = _config(inputs["out"], precision, content_size=96, style_scale=1.0, preserve_color="match")
    main.style_transfer(InputPaths(content_path=inputs["content"], style_path=inputs["style"]), cfg)
    ((style, content),) = seen
    resized = ops.resize(_load(inputs["content"]), (64, 96))
    assert torch.equal(content, resized) and tuple(style.shape) == (1, 3, 72, 96)
    assert not torch.equal(style, ops.resize(_load(inputs["style"]), (72, 96)))            # the match did run
    mu, cov = cr.mean_cov(style.cpu().numpy())
    mu_c, cov_c = cr.mean_cov(resized.cpu().numpy())
    mean_err, cov_err = float(np.abs(mu - mu_c).max()), float(np.abs(cov - cov_c).max() / np.abs(cov_c).max())
    print(f"match after resize, {precision}: mean error {mean_err:.2e}, covariance error {cov_err:.2e} of the largest entry")
    assert mean_err <= MEAN_BOUND and cov_err <= COV_BOUND


@pytest.mark.parametrize("precision", PRECISIONS)
def test_options_at_zero_are_the_plain_run_and_launch_no_resize(inputs, precision, monkeypatch):
    _forbid(monkeypatch, (ops, "resize"))
    paths = InputPaths(content_path=inputs["content"], style_path=inputs["style"])
    cfg = _config(inputs["out"], precision, content_size=0, style_size=0, style_scale=0.0, resize_filter="bicubic")
    got = main.style_transfer(paths, copy.deepcopy(cfg))
    plain = main.style_transfer(paths, _config(inputs["out"], precision))              # a config that never mentions them
    want = _by_hand(_load(inputs["content"]), _load(inputs["style"]), cfg)
    assert tuple(got.shape) == (1, 3, 100, 150)
    assert torch.equal(got, plain) and torch.equal(got, want), f"max |diff| {float((got - want).abs().max()):.3e}"
