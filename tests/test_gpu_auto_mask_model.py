"""Automatic masks (``--auto-mask``) through whole runs on a real MI355X: 64x64 and 128x128 images, synthetic VGG19 weights, four
L-BFGS steps.

* ``segment.auto_labels`` on the device against the same call through the NumPy twin of the assignment kernel: labels bit for
  bit, centroids equal as float64.
* A run with ``auto_mask`` against a run that is given the two label maps the first one saved (``--save-masks``) as
  ``--content-mask`` / ``--style-mask``: the same image and the same loss history, bit for bit, in fp32 and bf16, single-level
  and coarse-to-fine.  The pair is the textured halves of tests/test_segment_host.py, which establishes on the host that its
  segmentation is the halves.
* A pair that does not split runs unguided: the plain run's image, bit for bit.
* With the option off, a run equals the run of a config object that does not have the new fields: image and program keys.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch
from PIL import Image

from style_transfer_visualizer_amd import config as stv_config
from style_transfer_visualizer_amd import core_model, guidance, image_io, segment, synthetic
from style_transfer_visualizer_amd import main as stv_main
from style_transfer_visualizer_amd.type_defs import InputPaths
from tests import kmeans_ref as ref
from tests.test_segment_host import half_maps, write_halves

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


def _config(out_dir, precision="fp32", steps=4, **optimization):
    cfg = stv_config.StyleTransferConfig.model_validate({
        "output": {"output": str(out_dir), "plot_losses": False, "log_loss": str(out_dir) + ".csv", "log_every": 1},
        "optimization": {"steps": steps, "init_method": "content", "seed": 0, **optimization},
        "video": {"create_video": False, "final_only": True}, "hardware": {"device": "cuda", "precision": precision}})
    return cfg


def _run(paths, cfg) -> tuple[torch.Tensor, str]:
    image = stv_main.style_transfer(paths, cfg).detach().cpu()
    with open(cfg.output.log_loss) as fh:
        return image, fh.read()


@pytest.fixture(autouse=True)
def _synthetic_weights(monkeypatch):
    monkeypatch.setenv("STV_SYNTHETIC_WEIGHTS", "0")


# ---- device against twin ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["halves-64", "synthetic-96x80-R3-cell4", "synthetic-70x52-R4-cell2"])
def test_device_segmentation_equals_the_twin(case, tmp_path):
    if case == "halves-64":
        content, style = (image_io.load_image_to_tensor(p, DEV, normalize=True) for p in write_halves(tmp_path))
        regions, cell = 2, 8
    else:
        hw = (96, 80) if "96x80" in case else (70, 52)
        content, style = synthetic.synthetic_image(0, *hw).to(DEV), synthetic.synthetic_image(1, hw[1], hw[0]).to(DEV)
        regions, cell = (3, 4) if "R3" in case else (4, 2)
    c_dev, s_dev, i_dev = segment.auto_labels(content, style, regions, cell=cell)
    c_ref, s_ref, i_ref = segment.auto_labels(content, style, regions, cell=cell, assign=ref.assign_op)
    print(f"{case}: {i_dev['iterations']} iterations, shares {i_dev['shares']}")
    assert torch.equal(c_dev, c_ref) and torch.equal(s_dev, s_ref)
    assert np.array_equal(i_dev["centroids"].astype(np.float64), i_ref["centroids"].astype(np.float64))
    assert i_dev["iterations"] == i_ref["iterations"] and i_dev["cells"] == i_ref["cells"] and i_dev["converged"] == i_ref["converged"]
    assert c_dev.dtype == torch.uint8 and not c_dev.is_cuda and tuple(c_dev.shape) == tuple(content.shape[-2:])
    if case == "halves-64":
        want = half_maps(64)
        assert torch.equal(c_dev, want[0]) and torch.equal(s_dev, want[1])


# ---- an automatic run against the run with its saved masks --------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["fp32", "bf16", "pyramid"])
def test_automatic_run_equals_the_run_with_its_saved_masks(variant, tmp_path, caplog):
    size = 128 if variant == "pyramid" else 64
    precision = "bf16" if variant == "bf16" else "fp32"
    extra = {"pyramid_levels": 2} if variant == "pyramid" else {}
    content, style = write_halves(tmp_path, size)
    auto_cfg = _config(tmp_path / "auto", precision, auto_mask=True, **extra)
    auto_cfg.output.save_masks = True
    with caplog.at_level("INFO"):
        auto_image, auto_log = _run(InputPaths(content, style), auto_cfg)
    assert "Automatic masks: 2 regions (asked for 2)" in caplog.text
    masks = [str(tmp_path / "auto" / f"{name}_mask.png") for name in ("content", "style")]
    want = half_maps(size)
    for path, labels in zip(masks, want, strict=True):
        assert torch.equal(guidance.load_mask(path, (size, size), 2, "saved"), labels)
    file_cfg = _config(tmp_path / "files", precision, **extra)
    file_image, file_log = _run(InputPaths(content, style, content_mask_path=masks[0], style_mask_path=masks[1]), file_cfg)
    assert torch.equal(auto_image, file_image) and tuple(auto_image.shape[-2:]) == (size, size)
    assert auto_log == file_log and len(auto_log.splitlines()) == 1 + 4
    _, plain_log = _run(InputPaths(content, style), _config(tmp_path / "plain", precision, **extra))
    print(f"{variant}: guided  {auto_log.splitlines()[-1]}\n{variant}: plain   {plain_log.splitlines()[-1]}")
    assert plain_log != auto_log                                          # (the guidance does something)


# ---- the unguided fall-back ---------------------------------------------------------------------------------------------------

def test_a_pair_that_does_not_split_runs_as_the_plain_run(tmp_path, caplog):
    yy, xx = np.mgrid[0:64, 0:64]
    stripes = np.where(xx % 2 == 0, 100, 156)                 # every 8x8 cell of either image has the mean 128
    checker = np.where((xx + yy) % 2 == 0, 80, 176)
    for name, plane in (("content", stripes), ("style", checker)):
        Image.fromarray(np.repeat(plane[..., None], 3, axis=-1).astype(np.uint8)).save(tmp_path / f"{name}.png")
    paths = InputPaths(str(tmp_path / "content.png"), str(tmp_path / "style.png"))
    with caplog.at_level("INFO"):
        auto_image, auto_log = _run(paths, _config(tmp_path / "auto", auto_mask=True, mask_regions=3))
    assert "proceeds unguided" in caplog.text and "3 regions not accepted" in caplog.text and "2 regions not accepted" in caplog.text
    plain_image, plain_log = _run(paths, _config(tmp_path / "plain"))
    assert torch.equal(auto_image, plain_image) and auto_log == plain_log


# ---- the option off -------------------------------------------------------------------------------------------------------------

def test_with_the_option_off_the_run_is_the_run_of_a_config_without_the_fields(tmp_path, monkeypatch):
    content, style = write_halves(tmp_path)
    models = []
    prepare = core_model.prepare_model_and_input

    def recording(*args, **kw):
        out = prepare(*args, **kw)
        models.append((out[0], sorted(kw)))
        return out
    monkeypatch.setattr(core_model, "prepare_model_and_input", recording)
    for name in ("auto_guidance", "auto_labels", "pool_cells", "save_label_png"):
        monkeypatch.setattr(segment, name, lambda *a, **k: pytest.fail("the option is off"))

    class Old:          # a section from before the options existed
        def __init__(self, section, drop):
            self.__dict__.update({k: v for k, v in section.model_dump().items() if k not in drop})
    cfg = _config(tmp_path / "new")
    new_image, new_log = _run(InputPaths(content, style), cfg)
    ref_cfg = _config(tmp_path / "old")
    old = type("Config", (), {"optimization": Old(ref_cfg.optimization, ("auto_mask", "auto_mask_cell")), "video": ref_cfg.video,
                              "hardware": ref_cfg.hardware, "output": Old(ref_cfg.output, ("save_masks",))})()
    assert not hasattr(old.optimization, "auto_mask") and not hasattr(old.output, "save_masks")
    old_image, old_log = _run(InputPaths(content, style), old)
    assert torch.equal(new_image, old_image) and new_log == old_log

    def keys(model):          # (without the addresses: the kind, the two weights and the optional parts of the key)
        (eng,) = model._engines.values()
        return [(k[0], k[3], k[4], k[7:]) for k in eng._programs if k[0] == "fused"]
    (new_model, new_kw), (old_model, old_kw) = models
    assert new_kw == old_kw == ["precision"]
    assert keys(new_model) == keys(old_model) and keys(new_model) and all(k[3] == () for k in keys(new_model))
    assert list(new_model._engines) == list(old_model._engines) == [(64, 64, 0)]
