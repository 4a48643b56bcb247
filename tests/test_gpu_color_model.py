"""--preserve-color through ``main.style_transfer`` on a real MI355X: synthetic VGG19 weights, PNG inputs (content 64x80,
style 72x64), 3 steps, fp32 and bf16.  Every run is made once per (mode, precision) and shared by the tests that read it;
the spies record what the three colour ops were given and returned, which style image each model captured its targets
from, and the un-clamped image and loss history handed to ``runtime.save_outputs``.

Runs are deterministic (README, pyramid section), so an ``off`` run is a reference for the other two modes: ``match``
changes only the style tensor, ``luma`` only what happens behind the runner.
"""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch
from PIL import Image

from style_transfer_visualizer_amd import color, core_model, image_io, main, ops, runtime
from style_transfer_visualizer_amd import config as stv_config
from style_transfer_visualizer_amd.type_defs import InputPaths
from tests import color_ref as cr
from tests import resize_ref as rr
from tests.conftest import record_parity

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
CPU = torch.device("cpu")
PRECISIONS = ["fp32", "bf16"]
SIZES = {1: ((64, 80), (72, 64)), 2: ((128, 128), (136, 128))}        # levels -> (content, style) (H, W)
MEAN_BOUND, COV_BOUND = 1e-6, 1e-6                                    # the host test's bounds (tests/test_color_host.py)
_RUNS: dict = {}


def _paths(root, levels: int) -> InputPaths:
    folder = root / f"inputs{levels}"
    if not folder.exists():
        folder.mkdir()
        for name, seed, (H, W) in zip(("content", "style"), (0, 1), SIZES[levels], strict=True):
            rgb = cr.uint8_image(H, W, seed, normalize=False)[0].transpose(1, 2, 0)
            Image.fromarray(np.round(rgb * 255.0).astype(np.uint8)).save(folder / f"{name}.png")
    return InputPaths(content_path=str(folder / "content.png"), style_path=str(folder / "style.png"))


def _config(out_dir, mode: str | None, precision: str, levels: int):
    cfg = stv_config.StyleTransferConfig.model_validate({})
    oc = cfg.optimization
    oc.steps, oc.pyramid_levels, oc.init_method, oc.seed = 3, levels, "random", 0
    if mode is not None:                      # None: a config that never mentions the option
        oc.preserve_color = mode
    cfg.hardware.device, cfg.hardware.precision = "cuda", precision
    cfg.video.create_video, cfg.video.final_only = False, True
    cfg.output.output, cfg.output.plot_losses, cfg.output.log_every = str(out_dir), False, 1
    return cfg


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """``run(mode, precision, levels=1)`` -> the record of that run of ``main.style_transfer`` (made once)."""
    root = tmp_path_factory.mktemp("color_model")

    def make(mode: str | None, precision: str, levels: int = 1) -> dict:
        key = (mode, precision, levels)
        if key in _RUNS:
            return _RUNS[key]
        rec = {"stats": [], "affine": [], "luma": [], "styles": [], "paths": _paths(root, levels)}
        out_dir = root / f"out_{mode}_{precision}_{levels}"
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("STV_SYNTHETIC_WEIGHTS", "0")
            real_stats, real_affine, real_luma = ops.color_stats, ops.color_affine, ops.luma_transfer
            real_targets, real_save = core_model.StyleContentModel.set_targets, runtime.save_outputs

            def color_stats(img, out=None):
                parts = real_stats(img, out=out)
                rec["stats"].append(parts.clone())
                return parts

            def color_affine(x, m12, out=None):
                rec["affine"].append([float(v) for v in m12])
                return real_affine(x, m12, out=out)

            def luma_transfer(result, content, **kw):
                rec["luma"].append((result.detach().clone(), content.detach().clone(), kw))
                return real_luma(result, content, **kw)

            def set_targets(self, style_img, content_img):
                rec["styles"].append(style_img.detach().clone())
                return real_targets(self, style_img, content_img)

            def save_outputs(input_img, loss_metrics, *a, **k):
                rec["final"], rec["history"] = input_img.detach().clone(), {n: list(v) for n, v in loss_metrics.items()}
                return real_save(input_img, loss_metrics, *a, **k)
            mp.setattr(ops, "color_stats", color_stats)
            mp.setattr(ops, "color_affine", color_affine)
            mp.setattr(ops, "luma_transfer", luma_transfer)
            mp.setattr(core_model.StyleContentModel, "set_targets", set_targets)
            mp.setattr(runtime, "save_outputs", save_outputs)
            rec["returned"] = main.style_transfer(rec["paths"], _config(out_dir, mode, precision, levels)).clone()
            torch.cuda.synchronize()
        (rec["png"],) = list(out_dir.glob("stylized_*.png"))
        _RUNS[key] = rec
        return rec
    yield make
    _RUNS.clear()


def _loaded(paths: InputPaths) -> tuple[np.ndarray, np.ndarray]:
    """The two images as the loader hands them to the run (normalised fp32 ``[1, 3, H, W]``), on the host."""
    return (image_io.load_image_to_tensor(paths.content_path, CPU, normalize=True).numpy(),
            image_io.load_image_to_tensor(paths.style_path, CPU, normalize=True).numpy())


def _device_stats(parts: torch.Tensor, image: np.ndarray, what: str) -> tuple:
    """``(n, sums, moments)`` from the rows one launch left, after checking them against float64 NumPy (the 1e-12 rule)."""
    total = parts.cpu().numpy().sum(axis=0, dtype=np.float64)
    want, scale = cr.moments(image), cr.abs_moments(image)
    worst = float((np.abs(total - want) / scale).max())
    record_parity(what, "moments: worst |error| / sum|terms|", worst, 1e-12, "float64 NumPy")
    assert bool((np.abs(total - want) <= 1e-12 * scale).all()), f"{what}: {worst:.3e} of sum|terms|"
    second = np.empty((3, 3))
    for v, (i, j) in zip(total[3:], cr.PAIRS, strict=True):
        second[i, j] = second[j, i] = v
    return image.shape[-2] * image.shape[-1], total[:3].copy(), second


def _matched_twin(rec: dict, what: str) -> tuple[np.ndarray, np.ndarray]:
    """(content, matched style) on the host: the affine twin applied with the (A, b) that ``matching_transform`` returns for
    the statistics the device produced - style first, then content, as ``match_style_to_content`` asks for them."""
    content, style = _loaded(rec["paths"])
    assert len(rec["stats"]) == 2 and len(rec["affine"]) == 1 and rec["luma"] == []
    A, b = color.matching_transform(_device_stats(rec["stats"][0], style, f"{what} style"),
                                    _device_stats(rec["stats"][1], content, f"{what} content"))
    m12 = [*A.reshape(-1).tolist(), *b.tolist()]
    assert rec["affine"][0] == m12
    return content, cr.affine(style, m12)


def _finite(history: dict, steps: int = 3) -> bool:
    return (set(history) == {"style_loss", "content_loss", "total_loss"} and all(len(v) == steps for v in history.values())
            and all(math.isfinite(x) for v in history.values() for x in v))


# ---- match ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_match_hands_the_model_the_transformed_style(run, precision):
    rec = run("match", precision)
    content, matched = _matched_twin(rec, f"match {precision}")
    assert len(rec["styles"]) == 1
    got = rec["styles"][0].cpu()
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, 3, *SIZES[1][1])
    assert torch.equal(got, torch.from_numpy(matched)), f"{int((got != torch.from_numpy(matched)).sum())} elements differ from the twin"
    mu, cov = cr.mean_cov(got.numpy())
    mu_c, cov_c = cr.mean_cov(content)
    mean_err, cov_err = float(np.abs(mu - mu_c).max()), float(np.abs(cov - cov_c).max() / np.abs(cov_c).max())
    print(f"match {precision}: mean error {mean_err:.2e}, covariance error {cov_err:.2e} of the largest entry")
    record_parity(f"match {precision} 72x64 -> 64x80", "mean of the matched style: |error|", mean_err, MEAN_BOUND, "float64")
    record_parity(f"match {precision} 72x64 -> 64x80", "covariance: |error| / largest entry", cov_err, COV_BOUND, "float64")
    assert mean_err <= MEAN_BOUND and cov_err <= COV_BOUND
    assert _finite(rec["history"])
    off = run("off", precision)
    assert not torch.equal(rec["returned"], off["returned"]) and rec["history"] != off["history"]     # the targets did change
    assert tuple(rec["returned"].shape) == (1, 3, *SIZES[1][0])


# ---- luma -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_luma_is_the_twin_of_the_off_run(run, precision, tmp_path):
    off, rec = run("off", precision), run("luma", precision)
    content, _ = _loaded(rec["paths"])
    assert rec["stats"] == [] and rec["affine"] == [] and len(rec["luma"]) == 1
    result_seen, content_seen, kw = rec["luma"][0]
    assert torch.equal(result_seen, off["final"]) and torch.equal(content_seen.cpu(), torch.from_numpy(content))
    assert list(kw["mean"]) == list(cr.IMAGENET_MEAN) and list(kw["std"]) == list(cr.IMAGENET_STD)
    assert rec["history"] == off["history"] and _finite(rec["history"])
    twin = torch.from_numpy(cr.luma(off["final"].cpu().numpy(), content, normalize=True))
    assert torch.equal(rec["final"].cpu(), twin)                               # what save_outputs received
    assert torch.equal(rec["returned"].cpu(), twin.clamp(0, 1)), "the returned image is not the clamped twin"
    assert not torch.equal(rec["returned"], off["returned"])
    want_png = tmp_path / "twin.png"
    image_io.save_image(twin.to(DEV), want_png, normalize=True)
    got, want = np.array(Image.open(rec["png"])), np.array(Image.open(want_png))
    assert got.shape == (*SIZES[1][0], 3) and np.array_equal(got, want)
    assert not np.array_equal(got, np.array(Image.open(off["png"])))
    # the point of the mode: in [0, 1] RGB the saved picture differs from the content picture by (nearly) a grey value
    shift = got.astype(np.float64) - np.array(Image.open(rec["paths"].content_path)).astype(np.float64)
    inside = (got > 0).all(axis=2) & (got < 255).all(axis=2)                   # (where the export clamp did not cut a channel)
    print(f"luma {precision}: {inside.mean():.2f} of the pixels have no channel at 0 or 255")
    # each channel's shift is 255 d plus two roundings to a byte of at most 0.5 each: within 1.0 of the three channels' mean
    assert inside.any() and float(np.abs(shift - shift.mean(axis=2, keepdims=True))[inside].max()) <= 1.0


# ---- off ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_off_is_the_run_without_the_option(run, precision):
    off, plain = run("off", precision), run(None, precision)
    for rec in (off, plain):
        assert rec["stats"] == [] and rec["affine"] == [] and rec["luma"] == []          # none of the three ops is launched
        assert _finite(rec["history"]) and len(rec["styles"]) == 1
    assert torch.equal(off["returned"], plain["returned"]) and torch.equal(off["final"], plain["final"])
    assert off["history"] == plain["history"]
    assert np.array_equal(np.array(Image.open(off["png"])), np.array(Image.open(plain["png"])))
    _, style = _loaded(off["paths"])
    assert torch.equal(off["styles"][0].cpu(), torch.from_numpy(style))


# ---- match under a coarse-to-fine run ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_match_with_two_pyramid_levels_halves_the_matched_style(run, precision):
    rec = run("match", precision, 2)
    _, matched = _matched_twin(rec, f"match {precision}, 2 levels")                 # asserts: color_stats launched exactly twice
    assert len(rec["styles"]) == 2                                                  # coarsest first
    coarse, fine = (s.cpu() for s in rec["styles"])
    assert tuple(fine.shape) == (1, 3, *SIZES[2][1]) and tuple(coarse.shape) == (1, 3, SIZES[2][1][0] // 2, SIZES[2][1][1] // 2)
    assert torch.equal(fine, torch.from_numpy(matched))
    assert torch.equal(coarse, torch.from_numpy(rr.down2(matched)))
    assert _finite(rec["history"]) and tuple(rec["returned"].shape) == (1, 3, *SIZES[2][0])
