"""Automatic masks in VGG feature space (``--auto-mask-space features``) through whole runs on a real MI355X: 64x64 to 128x128
images, synthetic VGG19 weights, four L-BFGS steps.

* ``segment.feature_labels`` on the device against the same call through the NumPy twins of the two kernels, on the device's
  own features and from the same starting centroids: labels bit for bit, centroids equal as float64, iterations and counts.
* The device start (``mu``, ``lam``, ``v`` from the kept-labels launch and the MFMA Gram slabs) against float64 NumPy on the
  same features.  Measured on the MI355X (tools/feature_mask_bench.py, profiles/feature_mask_bench.json), the bounds below are
  four times the measured values, by storage type:

      =========  ===================  ==================  ================================
      storage    rel. error of lam    1 - |v . v_ref|     max |mu - mu_ref| / max |mu_ref|
      =========  ===================  ==================  ================================
      fp32       5.169e-09, 1.649e-08  9.659e-15, 7.327e-15  0, 0       (stripes 64^2, synthetic 96x80)
      bf16       4.484e-10, 8.802e-10  6.661e-16, 8.882e-16  0, 0
      =========  ===================  ==================  ================================

  (bf16 storage is the smaller error: a product of two bf16 values is exact in fp32, so only the fp32 accumulation rounds; the
  axis errors are a few units in the last place of the float64 dot product itself.)

* A run with ``--auto-mask --auto-mask-space features --save-masks`` against a run that gets those masks back as
  ``--content-mask`` / ``--style-mask``: the same image and loss history bit for bit, in fp32, bf16, coarse-to-fine at 128^2 and
  from a random start image (the variant that draws from the generator behind the stack's construction: it is what catches a
  generator state or VGG cache that the extraction disturbed).
* The stripes pair (tests/feature_mask_inputs.py): feature mode finds two regions whose saved masks are the halves (this test
  cannot pass without the feature); colour mode runs unguided with the warning and returns the plain run's image.  On the
  device the fp32 box means of the pair differ in their last bits by stripe direction (the sum of the same 32 + 32 values rounds
  differently for vertical and for horizontal stripes); ``segment.pooling_noise`` is what keeps the colour k-means from
  splitting the pair on that rounding - without it the MI355X accepted 2 regions after 2 iterations, shares [0.5, 0.5].
* With the option off, a run equals the run of a config object that does not have the new fields: image and program keys.
"""
from __future__ import annotations

import types

import numpy as np
import pytest
import torch

from style_transfer_visualizer_amd import config as stv_config
from style_transfer_visualizer_amd import core_model, guidance, segment, synthetic
from style_transfer_visualizer_amd import main as stv_main
from style_transfer_visualizer_amd.type_defs import InputPaths
from tests import feature_mask_inputs as fi
from tests import kmeans_feat_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
# four times the errors measured on the MI355X for the stripes pair and the synthetic pair: (relative error of lam, 1 - |v.v_ref|)
START_BOUNDS = {"fp32": (4 * 1.649e-08, 4 * 9.659e-15), "bf16": (4 * 8.802e-10, 4 * 8.882e-16)}


def _config(out_dir, precision="fp32", steps=4, **optimization):
    return stv_config.StyleTransferConfig.model_validate({
        "output": {"output": str(out_dir), "plot_losses": False, "log_loss": str(out_dir) + ".csv", "log_every": 1},
        "optimization": {"steps": steps, "init_method": "content", "seed": 0, **optimization},
        "video": {"create_video": False, "final_only": True}, "hardware": {"device": "cuda", "precision": precision}})


def _run(paths, cfg) -> tuple[torch.Tensor, str]:
    image = stv_main.style_transfer(paths, cfg).detach().cpu()
    with open(cfg.output.log_loss) as fh:
        return image, fh.read()


@pytest.fixture(autouse=True)
def _synthetic_weights(monkeypatch):
    monkeypatch.setenv("STV_SYNTHETIC_WEIGHTS", "0")


def _pair(case: str):
    if case == "stripes-64":
        return (*fi.stripes_tensors(64, DEV), 2)
    return synthetic.synthetic_image(0, 96, 80).to(DEV), synthetic.synthetic_image(1, 80, 96).to(DEV), 3


_FEATURES: dict = {}


def _features(case: str, precision: str):
    """The device's features of a pair, extracted once per (pair, precision) and left unchanged."""
    key = (case, precision)
    if key not in _FEATURES:
        content, style, regions = _pair(case)
        _FEATURES[key] = (segment.run_features(content, style, fi.LAYER, types.SimpleNamespace(), precision), regions)
    return _FEATURES[key]


# ---- device against twins ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("case", ["stripes-64", "synthetic-96x80-R3"])
def test_device_segmentation_equals_the_twins(case, precision):
    (F_c, F_s), regions = _features(case, precision)
    assert F_c.is_cuda and F_c.dtype == (torch.bfloat16 if precision == "bf16" else torch.float32) and int(F_c.shape[-1]) == 256      # noqa: PLR2004
    start = segment.feature_start([segment.feature_moments(F) for F in (F_c, F_s)], regions)["centroids"]
    c_dev, s_dev, i_dev = segment.feature_labels(F_c, F_s, regions, centroids=start)
    c_ref, s_ref, i_ref = segment.feature_labels(F_c, F_s, regions, centroids=start, assign=ref.assign_op, update=ref.update_op)
    print(f"{case} {precision}: {i_dev['iterations']} iterations, shares {i_dev['shares']}")
    assert torch.equal(c_dev, c_ref) and torch.equal(s_dev, s_ref)
    assert np.array_equal(i_dev["centroids"].astype(np.float64), i_ref["centroids"].astype(np.float64))
    assert i_dev["iterations"] == i_ref["iterations"] and i_dev["cells"] == i_ref["cells"] and i_dev["converged"] == i_ref["converged"]
    assert c_dev.dtype == torch.uint8 and not c_dev.is_cuda and tuple(c_dev.shape) == tuple(F_c.shape[:2])
    if case == "stripes-64":
        want = fi.half_grids(16)
        assert int((c_dev != want[0]).sum()) <= fi.DIFFER_CAP and int((s_dev != want[1]).sum()) <= fi.DIFFER_CAP


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("case", ["stripes-64", "synthetic-96x80-R3"])
def test_device_start_against_float64(case, precision):
    (F_c, F_s), regions = _features(case, precision)
    dev = segment.feature_start([segment.feature_moments(F) for F in (F_c, F_s)], regions)
    host = segment.feature_start([ref.moments_op(F) for F in (F_c, F_s)], regions)
    lam_err = abs(dev["lam"] - host["lam"]) / host["lam"]
    axis_err = 1.0 - abs(float(dev["v"] @ host["v"]))
    mu_err = float(np.abs(dev["mu"] - host["mu"]).max() / np.abs(host["mu"]).max())
    print(f"start {case} {precision}: lam rel err {lam_err:.3e}, 1-|v.v_ref| {axis_err:.3e}, mu err {mu_err:.3e}")
    lam_bound, axis_bound = START_BOUNDS[precision]
    assert lam_err <= lam_bound and axis_err <= axis_bound
    # mu: at most 1024 fp32 values per channel added in double in two different orders - n * 2^-53 * max|x| / max|mu|, with
    # max|x| / max|mu| far below 1e4
    assert mu_err <= 1e-9                                     # noqa: PLR2004
    assert float(dev["v"] @ host["v"]) > 0                    # the sign rule holds on both sides


# ---- an automatic run against the run with its saved masks --------------------------------------------------------------------

def _grid_of(mask: torch.Tensor, side: int) -> torch.Tensor:
    step = int(mask.shape[0]) // side
    return mask[step // 2::step, step // 2::step]


@pytest.mark.parametrize("variant", ["fp32", "bf16", "pyramid", "random-init"])
def test_automatic_run_equals_the_run_with_its_saved_masks(variant, tmp_path, caplog):
    size = 128 if variant == "pyramid" else 64
    precision = "bf16" if variant == "bf16" else "fp32"
    extra = {"pyramid_levels": 2} if variant == "pyramid" else {}
    if variant == "random-init":          # the start image is drawn behind the stack's construction: a generator state that
        extra = {"init_method": "random"}      # run_features left disturbed would change it, and with it every bit behind
    content, style = fi.write_stripes(tmp_path, size)
    auto_cfg = _config(tmp_path / "auto", precision, auto_mask=True, auto_mask_space="features", **extra)
    auto_cfg.output.save_masks = True
    with caplog.at_level("INFO"):
        auto_image, auto_log = _run(InputPaths(content, style), auto_cfg)
    assert "Automatic masks: feature space, layer 10" in caplog.text and "2 regions (asked for 2)" in caplog.text
    masks = [str(tmp_path / "auto" / f"{name}_mask.png") for name in ("content", "style")]
    for path, want in zip(masks, fi.half_grids(size // 4), strict=True):
        got = _grid_of(guidance.load_mask(path, (size, size), 2, "saved"), size // 4)
        assert int((got != want).sum()) <= fi.DIFFER_CAP
    file_cfg = _config(tmp_path / "files", precision, **extra)
    file_image, file_log = _run(InputPaths(content, style, content_mask_path=masks[0], style_mask_path=masks[1]), file_cfg)
    assert torch.equal(auto_image, file_image) and tuple(auto_image.shape[-2:]) == (size, size)
    assert auto_log == file_log and len(auto_log.splitlines()) == 1 + 4
    _, plain_log = _run(InputPaths(content, style), _config(tmp_path / "plain", precision, **extra))
    print(f"{variant}: guided  {auto_log.splitlines()[-1]}\n{variant}: plain   {plain_log.splitlines()[-1]}")
    assert plain_log != auto_log                                          # (the guidance does something)


# ---- the stripes pair: colour cannot, features can ------------------------------------------------------------------------------

def test_the_stripes_pair_is_guided_in_feature_space(tmp_path, caplog):
    content, style = fi.write_stripes(tmp_path)
    paths = InputPaths(content, style)
    plain_image, plain_log = _run(paths, _config(tmp_path / "plain"))
    cfg = _config(tmp_path / "features", auto_mask=True, auto_mask_space="features")
    cfg.output.save_masks = True
    with caplog.at_level("INFO"):
        feature_image, feature_log = _run(paths, cfg)
    assert "2 regions (asked for 2)" in caplog.text and "proceeds unguided" not in caplog.text
    for name, want in zip(("content", "style"), fi.half_grids(16), strict=True):
        got = _grid_of(guidance.load_mask(str(tmp_path / "features" / f"{name}_mask.png"), (64, 64), 2, "saved"), 16)
        differ = int((got != want).sum())
        print(f"{name}: {differ} of 256 cells differ from the halves")
        assert differ <= fi.DIFFER_CAP                        # region 0 is the vertical stripes in both images
    assert feature_log != plain_log and not torch.equal(feature_image, plain_image)


def test_the_stripes_pair_runs_unguided_in_colour_mode(tmp_path, caplog):
    """Every 8x8 box mean of the pair is one colour up to fp32 rounding: no spread, no split (``segment.pooling_noise``)."""
    content, style = fi.write_stripes(tmp_path)
    paths = InputPaths(content, style)
    with caplog.at_level("INFO"):
        colour_image, colour_log = _run(paths, _config(tmp_path / "colour", auto_mask=True))
    assert "2 regions not accepted" in caplog.text and "proceeds unguided" in caplog.text
    plain_image, plain_log = _run(paths, _config(tmp_path / "plain"))
    assert torch.equal(colour_image, plain_image) and colour_log == plain_log


# ---- the option off -------------------------------------------------------------------------------------------------------------

def test_with_the_option_off_the_run_is_the_run_of_a_config_without_the_fields(tmp_path, monkeypatch):
    content, style = fi.write_stripes(tmp_path)
    models = []
    prepare = core_model.prepare_model_and_input

    def recording(*args, **kw):
        out = prepare(*args, **kw)
        models.append((out[0], sorted(kw)))
        return out
    monkeypatch.setattr(core_model, "prepare_model_and_input", recording)
    for name in ("auto_guidance", "feature_labels", "run_features", "extract_features", "feature_moments", "save_label_png"):
        monkeypatch.setattr(segment, name, lambda *a, **k: pytest.fail("the option is off"))

    class Old:          # a section from before the options existed
        def __init__(self, section, drop):
            self.__dict__.update({k: v for k, v in section.model_dump().items() if k not in drop})
    cfg = _config(tmp_path / "new")
    new_image, new_log = _run(InputPaths(content, style), cfg)
    ref_cfg = _config(tmp_path / "old")
    old = type("Config", (), {"optimization": Old(ref_cfg.optimization, ("auto_mask_space", "auto_mask_layer")), "video": ref_cfg.video,
                              "hardware": ref_cfg.hardware, "output": ref_cfg.output})()
    assert not hasattr(old.optimization, "auto_mask_space") and not hasattr(old.optimization, "auto_mask_layer")
    old_image, old_log = _run(InputPaths(content, style), old)
    assert torch.equal(new_image, old_image) and new_log == old_log

    def keys(model):          # (without the addresses: the kind, the two weights and the optional parts of the key)
        (eng,) = model._engines.values()
        return [(k[0], k[3], k[4], k[7:]) for k in eng._programs if k[0] == "fused"]
    (new_model, new_kw), (old_model, old_kw) = models
    assert new_kw == old_kw == ["precision"]
    assert keys(new_model) == keys(old_model) and keys(new_model) and all(k[3] == () for k in keys(new_model))
    assert list(new_model._engines) == list(old_model._engines) == [(64, 64, 0)]
