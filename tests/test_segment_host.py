"""Automatic masks (``--auto-mask``; ``segment.py``, ``stv_kmeans_assign``) without a GPU: the NumPy twin's own rules, the whole
algorithm through the twins, the fall-back, the eigenvector's sign, the mask round trip, the public surface and the ABI."""
from __future__ import annotations

import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch
from PIL import Image

from style_transfer_visualizer_amd import _lib, cli, config_defaults, core_model, guidance, segment
from style_transfer_visualizer_amd import config as stv_config
from style_transfer_visualizer_amd import main as stv_main
from style_transfer_visualizer_amd.type_defs import InputPaths
from tests import kmeans_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grey(plane: np.ndarray) -> torch.Tensor:
    """``[1, 3, H, W]`` fp32 with the three channels equal to ``plane``."""
    return torch.from_numpy(np.repeat(np.asarray(plane, dtype=np.float32)[None], 3, axis=0).copy())[None]


def halves(texture: float = 0.0) -> tuple[torch.Tensor, torch.Tensor]:
    """Content 64x64: left half 0.1, right half 0.9; style 64x64: top half 0.2, bottom half 0.8; ``texture``: the amplitude of
    a deterministic pattern added to both (shared with the GPU model test)."""
    yy, xx = np.mgrid[0:64, 0:64]
    wobble = texture * (((3 * yy + 5 * xx) % 7) - 3.0) / 3.0
    content = np.where(xx < 32, 0.1, 0.9) + wobble
    style = np.where(yy < 32, 0.2, 0.8) + wobble
    return _grey(content), _grey(style)


def halves_labels() -> tuple[torch.Tensor, torch.Tensor]:
    yy, xx = np.mgrid[0:64, 0:64]
    return torch.from_numpy((xx >= 32).astype(np.uint8)), torch.from_numpy((yy >= 32).astype(np.uint8))


def write_halves(folder, size: int = 64, texture: int = 6) -> tuple[str, str]:
    """The halves pair as 8-bit PNG files ``content.png`` / ``style.png`` in ``folder`` with a little deterministic texture (an
    integer pattern of amplitude ``texture`` grey levels, different in the three channels); shared with the GPU model test,
    whose runs read these files."""
    yy, xx = np.mgrid[0:size, 0:size]
    paths = []
    for name, dark, low, high in (("content", xx < size // 2, 26, 230), ("style", yy < size // 2, 51, 204)):
        planes = [np.where(dark, low, high) + ((((3 + c) * yy + (5 - c) * xx) % 7) - 3) * texture // 3 for c in range(3)]
        Image.fromarray(np.stack(planes, axis=-1).astype(np.uint8)).save(folder / f"{name}.png")
        paths.append(str(folder / f"{name}.png"))
    return paths[0], paths[1]


def half_maps(size: int) -> tuple[torch.Tensor, torch.Tensor]:
    yy, xx = np.mgrid[0:size, 0:size]
    return torch.from_numpy((xx >= size // 2).astype(np.uint8)), torch.from_numpy((yy >= size // 2).astype(np.uint8))


def _options(**kw):
    oc = stv_config.StyleTransferConfig.model_validate({}).optimization
    for key, value in kw.items():
        setattr(oc, key, value)
    return oc


# ---- 1. the twin's own rules ------------------------------------------------------------------------------------------------

def test_twin_gives_a_tie_to_the_lowest_index_and_one_cluster_everything():
    x = np.zeros((3, 2, 3), dtype=np.float32)
    x[:, 0, :] = (0.0, 1.0, 2.0)                        # pixel values 0, 1, 2 in every channel
    x[:, 1, :] = (1.0, 3.0, -1.0)
    c = np.array([[0, 0, 0], [2, 2, 2], [2, 2, 2]], dtype=np.float32)      # 1 is as far from 0 as from 2; clusters 1 and 2 coincide
    labels, sums, counts, changed = ref.assign(x, c, np.full((2, 3), 255, dtype=np.uint8))
    assert labels.tolist() == [[0, 0, 1], [0, 1, 0]]
    assert counts.tolist() == [4.0, 2.0, 0.0] and changed == 6
    assert sums.tolist() == [[1.0] * 3, [5.0] * 3, [0.0] * 3]
    again = ref.assign(x, c, labels)
    assert again[3] == 0 and np.array_equal(again[0], labels)
    one = ref.assign(x, c[:1] + 7.0, labels)
    assert not one[0].any() and one[2].tolist() == [6.0] and one[3] == 2
    # a NaN distance never wins; all NaN: label 0
    nan = ref.assign(x, np.array([[np.nan] * 3, [9, 9, 9]], dtype=np.float32), labels)
    assert (nan[0] == 1).all()
    assert not ref.assign(x, np.full((2, 3), np.nan, dtype=np.float32), labels)[0].any()


# ---- 2. the whole algorithm through the twins -------------------------------------------------------------------------------

@pytest.mark.parametrize("texture", [0.0, 0.02], ids=["flat", "textured"])
def test_halves_are_found_exactly_with_region_0_dark(texture):
    content, style = halves(texture)
    c, s, info = segment.auto_labels(content, style, 2, cell=8, **ref.HOST)
    want_c, want_s = halves_labels()
    assert torch.equal(c, want_c) and torch.equal(s, want_s)
    assert c.dtype == torch.uint8 and info["converged"] and info["iterations"] <= 3
    assert info["regions"] == 2 and info["cells"] == {"content": [32, 32], "style": [32, 32]}
    assert info["shares"] == {"content": [0.5, 0.5], "style": [0.5, 0.5]}
    cen = info["centroids"]
    assert cen.dtype == np.float32 and cen.shape == (2, 3) and (cen[0] < cen[1]).all()
    np.testing.assert_allclose(cen[:, 0], [0.15, 0.85], atol=0.02)          # the means of (0.1, 0.2) and of (0.9, 0.8)


@pytest.mark.parametrize("size", [64, 128])
@pytest.mark.parametrize("normalize", [True, False], ids=["normalised", "rgb"])
def test_the_textured_halves_files_still_segment_into_the_halves(tmp_path, size, normalize):
    from style_transfer_visualizer_amd import image_io
    content, style = (image_io.load_image_to_tensor(p, torch.device("cpu"), normalize=normalize) for p in write_halves(tmp_path, size))
    assert len(torch.unique(content)) > 12                  # (there is a texture)
    c, s, info = segment.auto_labels(content, style, 2, cell=8, **ref.HOST)
    want_c, want_s = half_maps(size)
    assert torch.equal(c, want_c) and torch.equal(s, want_s) and info["converged"] and info["iterations"] <= 3
    oc = _options(auto_mask=True)
    got = segment.auto_guidance(content, style, oc, 2 if size == 128 else 1, **ref.HOST)        # noqa: PLR2004
    assert got is not None and torch.equal(got[0], want_c) and torch.equal(got[1], want_s) and oc.mask_regions == 2


def _bands(sizes, values, axis, other) -> torch.Tensor:
    line = np.concatenate([np.full(n, v) for n, v in zip(sizes, values, strict=True)])
    plane = np.repeat(line[:, None], other, axis=1) if axis == 0 else np.repeat(line[None, :], other, axis=0)
    img = np.stack([plane, plane * 0.5, 1.0 - plane]).astype(np.float32)      # a colour, not a grey: all three channels count
    return torch.from_numpy(img)[None]


def test_each_image_weighs_one_half_whatever_its_size():
    # dyadic values on cell boundaries: every sum is exact, so "the same" means the same bits
    content = _bands((16, 32, 48), (0.125, 0.5, 0.875), 1, 64)                  # 64 x 96, three bands
    style = _bands((8, 8, 16, 32), (0.0625, 0.25, 0.625, 0.9375), 0, 64)        # 64 x 64, four bands
    doubled = style.repeat_interleave(2, dim=-2).repeat_interleave(2, dim=-1)
    for regions in (2, 3, 4):
        c1, s1, i1 = segment.auto_labels(content, style, regions, cell=8, **ref.HOST)
        c2, s2, i2 = segment.auto_labels(content, doubled, regions, cell=8, **ref.HOST)
        assert np.array_equal(i1["centroids"], i2["centroids"]) and i1["iterations"] == i2["iterations"]
        assert torch.equal(c1, c2)
        assert torch.equal(s2, s1.repeat_interleave(2, dim=0).repeat_interleave(2, dim=1))
        assert i1["shares"] == i2["shares"] and i1["converged"]
        assert [4 * n for n in i1["cells"]["style"]] == i2["cells"]["style"]


# ---- 3. validity and the fall-back ------------------------------------------------------------------------------------------

def test_a_colour_in_one_image_only_falls_back_by_one_region(caplog):
    content = _grey(np.repeat(np.repeat([[0.0, 0.25, 0.5, 1.0]], 16, axis=1), 64, axis=0))              # four stripes of 16 columns
    line = np.concatenate([np.full(16, 0.0), np.full(32, 0.25), np.full(16, 0.5)])                      # ... without the last colour
    style = _grey(np.repeat(line[None], 64, axis=0))
    oc = _options(mask_regions=4, auto_mask=True)
    with caplog.at_level("INFO"):
        labels = segment.auto_guidance(content, style, oc, 1, **ref.HOST)
    assert "4 regions not accepted: region 3 holds 0 of the 64 cells of the style image" in caplog.text
    assert "Automatic masks: 3 regions (asked for 4)" in caplog.text and "unguided" not in caplog.text
    assert oc.mask_regions == 3 and labels is not None
    for lab in labels:
        assert sorted(set(lab.reshape(-1).tolist())) == [0, 1, 2] and tuple(lab.shape) == (64, 64)
    assert guidance.region_counts(labels[0], 3)[0] == 64 * 16            # region 0: the dark stripe


def test_two_constant_equal_images_run_unguided_with_a_warning(caplog):
    img = _grey(np.full((64, 64), 0.5))
    oc = _options(mask_regions=3, auto_mask=True)
    with caplog.at_level("INFO"):
        assert segment.auto_guidance(img, img.clone(), oc, 1, **ref.HOST) is None
    warnings = [r for r in caplog.records if r.levelname == "WARNING"]
    assert len(warnings) == 1 and "proceeds unguided" in warnings[0].getMessage()
    assert "3 regions not accepted: region 1 holds 0 of the 64 cells of the content image" in caplog.text
    assert "2 regions not accepted" in caplog.text
    assert oc.mask_regions == 3              # (nothing to hand on: the option is as it was)


def test_a_region_that_vanishes_at_a_coarse_level_is_not_accepted():
    content, style = halves()
    c, s, info = segment.auto_labels(content, style, 2, cell=8, **ref.HOST)
    assert segment._refusal(c, s, info, [0, 5, 10, 19, 28], 1) is None
    assert segment._refusal(c, s, info, [0, 5, 10, 19, 28], 2) is None
    thin = c.clone()
    thin[:, 8:] = 1
    thin[:, :8] = 0                            # a strip of 8 of 64 columns: the 4x4 map of the deepest tap samples columns 8, 24, ...
    info["cells"]["content"] = [8, 56]
    why = segment._refusal(thin, s, info, [0, 5, 10, 19, 28], 1)
    assert why is not None and why.startswith("region 0 holds 0 pixels of the content image's 4x4 label map at style layer 28")
    assert "pyramid level" in segment._refusal(thin, s, info, [0, 5], 4)


def test_small_shares_are_not_accepted():
    content, style = halves()
    c, s, info = segment.auto_labels(content, style, 2, cell=1, **ref.HOST)
    info["cells"]["style"] = [63, 4033]         # 63 * 64 < 4096
    assert segment._refusal(c, s, info, [0], 1) == "region 0 holds 63 of the 4096 cells of the style image, fewer than 1/64"
    info["cells"]["style"] = [64, 4032]
    assert segment._refusal(c, s, info, [0], 1) is None
    assert segment.MIN_SHARE_DIV == 64


# ---- 4. the eigenvector's sign ----------------------------------------------------------------------------------------------

def test_the_principal_axis_points_to_the_bright_end_or_has_a_positive_first_component():
    for axis, want in (((1.0, -1.0, 0.0), (1, -1, 0)), ((-1.0, 1.0, 0.0), (1, -1, 0)), ((0.0, -1.0, 1.0), (0, 1, -1)),
                       ((-1.0, 0.0, 1.0), (1, 0, -1))):
        a = np.asarray(axis) / np.sqrt(2.0)
        v, lam = segment.principal_axis(2.0 * np.outer(a, a))
        assert v.sum() == 0.0, "the case is meant to sit on the rule's second branch"
        np.testing.assert_allclose(v, np.asarray(want) / np.sqrt(2.0), atol=1e-12)
        assert lam == pytest.approx(2.0)
    for axis in ((1.0, 1.0, 1.0), (-1.0, -1.0, -1.0), (-3.0, 1.0, 1.0), (3.0, -1.0, -1.0)):
        v, _ = segment.principal_axis(np.outer(axis, axis))
        assert v.sum() > 0.0
    v, lam = segment.principal_axis(np.zeros((3, 3)))
    assert lam == 0.0 and np.isfinite(v).all()


# ---- 5. the mask round trip -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("regions", [2, 3, 4])
def test_saved_label_maps_read_back_as_themselves(tmp_path, regions):
    gen = torch.Generator().manual_seed(regions)
    labels = torch.randint(0, regions, (37, 53), generator=gen, dtype=torch.uint8)
    path = tmp_path / "map.png"
    segment.save_label_png(labels, regions, path)
    with Image.open(path) as img:
        assert img.mode == "L" and img.size == (53, 37)
        levels = sorted(set(np.asarray(img).reshape(-1).tolist()))
    assert levels == [((2 * k + 1) * 256) // (2 * regions) for k in range(regions)]
    assert torch.equal(guidance.load_mask(str(path), (37, 53), regions, "content"), labels)
    with pytest.raises(ValueError, match="no region"):
        segment.save_label_png(torch.full((4, 4), guidance.NO_REGION, dtype=torch.uint8), regions, path)


# ---- 6. the public surface --------------------------------------------------------------------------------------------------

def _write_inputs(tmp_path, hw=(64, 64)):
    out = {}
    for name in ("content", "style", "more"):
        Image.fromarray(np.full((*hw, 3), 128, dtype=np.uint8)).save(tmp_path / f"{name}.png")
        Image.fromarray(np.zeros(hw, dtype=np.uint8)).save(tmp_path / f"{name}_mask.png")
        out[name], out[name + "_mask"] = str(tmp_path / f"{name}.png"), str(tmp_path / f"{name}_mask.png")
    return out


def test_every_refusal_names_its_values_and_comes_before_a_device_is_touched(tmp_path):
    p = _write_inputs(tmp_path)

    def run(paths, **kw):
        cfg = stv_config.StyleTransferConfig.model_validate({})
        cfg.hardware.device = "no-such-device"
        cfg.optimization.auto_mask = True
        for key, value in kw.items():
            object.__setattr__(cfg.optimization, key, value)
        stv_main.style_transfer(paths, cfg)
    plain = InputPaths(p["content"], p["style"])
    with pytest.raises(ValueError, match=re.escape(f"--auto-mask cannot be combined with --content-mask / --style-mask (got content mask "
                                                   f"{p['content_mask']!r} and style mask {p['style_mask']!r})")):
        run(InputPaths(p["content"], p["style"], content_mask_path=p["content_mask"], style_mask_path=p["style_mask"]))
    with pytest.raises(ValueError, match=re.escape("--auto-mask cannot be combined with --content-mask")):
        run(InputPaths(p["content"], p["style"], style_mask_path=p["style_mask"]))
    with pytest.raises(ValueError, match=re.escape("--auto-mask cannot be combined with --style-also (1 further style images)")):
        run(InputPaths(p["content"], p["style"], extra_style_paths=(p["more"],)))
    with pytest.raises(ValueError, match=re.escape("--auto-mask cannot be combined with --region-weights ([1.0, 0.5]): which region gets "
                                                   "which number is not known in advance")):
        run(plain, region_weights=[1.0, 0.5])
    for bad in (0, 3, 64, "8", True):
        with pytest.raises(ValueError, match=re.escape(f"auto_mask_cell must be one of [1, 2, 4, 8, 16, 32], got {bad!r}")):
            run(plain, auto_mask_cell=bad)
    with pytest.raises(ValueError, match="mask_regions must be an integer from 2 to 4, got 5"):
        run(plain, mask_regions=5)
    # --save-masks: needs a guided run, and two file names
    cfg = stv_config.StyleTransferConfig.model_validate({"output": {"save_masks": True}})
    cfg.hardware.device = "no-such-device"
    with pytest.raises(ValueError, match="--save-masks without masks"):
        stv_main.style_transfer(plain, cfg)
    (tmp_path / "other").mkdir()
    Image.fromarray(np.full((64, 64, 3), 128, dtype=np.uint8)).save(tmp_path / "other" / "content.png")
    cfg.optimization.auto_mask = True
    with pytest.raises(ValueError, match="share the stem 'content'"):
        stv_main.style_transfer(InputPaths(p["content"], str(tmp_path / "other" / "content.png")), cfg)
    # the refusals of the mask files stay as they are
    with pytest.raises(ValueError, match="--content-mask and --style-mask go together"):
        stv_main.style_transfer(InputPaths(p["content"], p["style"], content_mask_path=p["content_mask"]),
                                stv_config.StyleTransferConfig.model_validate({"hardware": {"device": "no-such-device"}}))


def test_images_too_small_for_the_cells_are_refused_before_the_first_launch():
    def never(*a, **k):
        raise AssertionError("a kernel was launched")
    big, small = torch.zeros(1, 3, 64, 96), torch.zeros(1, 3, 63, 200)
    msg = "--auto-mask: cells of 8 pixels leave 12x8 cells of the 96x64 content image and 25x7 of the 200x63 style image"
    with pytest.raises(ValueError, match=re.escape(msg)):
        segment.auto_guidance(big, small, _options(auto_mask=True), 1, assign=never, pool=never, moments=never)
    with pytest.raises(ValueError, match="leave 25x7 cells of the 200x63 content image and 12x8 of the 96x64 style image"):
        segment.auto_guidance(small, big, _options(auto_mask=True), 1, assign=never, pool=never, moments=never)
    with pytest.raises(ValueError, match="cells of 16 pixels"):
        segment.auto_guidance(big, big, _options(auto_mask=True, auto_mask_cell=16), 1, assign=never, pool=never, moments=never)
    segment.check_sizes((64, 96), (64, 64), 8)


def _cli_config(argv):
    args = cli.build_arg_parser().parse_args(argv)
    base = stv_config.ConfigLoader.load(args.config) if args.config else None
    return stv_config.build_config_from_cli(vars(args), base_config=base)


def test_config_and_cli_round_trip(tmp_path, caplog, capsys):
    base = ["--content", "c.png", "--style", "s.png"]
    assert (config_defaults.DEFAULT_AUTO_MASK, config_defaults.DEFAULT_AUTO_MASK_CELL, config_defaults.DEFAULT_SAVE_MASKS) == (False, 8, False)
    for cfg in (stv_config.StyleTransferConfig.model_validate({}), _cli_config(base)):
        assert (cfg.optimization.auto_mask, cfg.optimization.auto_mask_cell, cfg.output.save_masks) == (False, 8, False)
    cfg = _cli_config([*base, "--auto-mask", "--auto-mask-cell", "4", "--save-masks", "--mask-regions", "3"])
    assert (cfg.optimization.auto_mask, cfg.optimization.auto_mask_cell, cfg.output.save_masks, cfg.optimization.mask_regions) == (True, 4, True, 3)
    toml = tmp_path / "config.toml"
    toml.write_text("[optimization]\nauto_mask = true\nauto_mask_cell = 16\n[output]\nsave_masks = true\n")
    for cfg in (stv_config.ConfigLoader.load(str(toml)), _cli_config(["--config", str(toml)])):
        assert (cfg.optimization.auto_mask, cfg.optimization.auto_mask_cell, cfg.output.save_masks) == (True, 16, True)
    assert _cli_config(["--config", str(toml), "--auto-mask-cell", "2"]).optimization.auto_mask_cell == 2
    toml.write_text("[optimization]\nauto_mask_cell = 3\n")
    with pytest.raises(ValueError, match=re.escape("auto_mask_cell must be one of [1, 2, 4, 8, 16, 32], got 3")):
        stv_config.ConfigLoader.load(str(toml))
    with pytest.raises(SystemExit):
        cli.build_arg_parser().parse_args([*base, "--auto-mask-cell", "3"])
    assert "invalid choice: 3" in capsys.readouterr().err
    assert not hasattr(cli.build_arg_parser().parse_args(base), "auto_mask_cell")
    paths = InputPaths(content_path="c.png", style_path="s.png")
    with caplog.at_level("INFO"):
        cli.log_parameters(paths, _cli_config(base))
    assert "Automatic" not in caplog.text and "Save Masks" not in caplog.text and "Mask Regions" not in caplog.text
    caplog.clear()
    with caplog.at_level("INFO"):
        cli.log_parameters(paths, _cli_config([*base, "--auto-mask", "--save-masks"]))
    for line in ("Automatic Masks: Enabled", "Mask Regions: 2", "Automatic Mask Cell: 8", "Save Masks: Yes"):
        assert line in caplog.text


def test_with_the_option_off_the_run_reaches_the_model_with_the_keywords_it_gets_today(monkeypatch, tmp_path):
    p = _write_inputs(tmp_path)
    seen = []

    def probe(*args, **kw):
        seen.append((args, kw))
        raise KeyboardInterrupt          # (the call is what is looked at: nothing is built)
    monkeypatch.setattr(core_model, "prepare_model_and_input", probe)
    for name in ("auto_guidance", "auto_labels", "save_label_png"):
        monkeypatch.setattr(segment, name, lambda *a, **k: pytest.fail("the option is off"))
    cfg = stv_config.StyleTransferConfig.model_validate({})
    cfg.video.create_video = False
    with pytest.raises(KeyboardInterrupt):
        stv_main.style_transfer(InputPaths(p["content"], p["style"]), cfg)
    args, kw = seen[-1]
    assert sorted(kw) == ["precision"] and len(args) == 4 and args[3] is cfg.optimization
    assert tuple(args[0].shape) == tuple(args[1].shape) == (1, 3, 64, 64)

    class Old:          # a config whose sections predate the options
        def __init__(self, section, drop):
            self.__dict__.update({k: v for k, v in section.model_dump().items() if k not in drop})
    old = types.SimpleNamespace(optimization=Old(cfg.optimization, ("auto_mask", "auto_mask_cell")), video=cfg.video,
                                hardware=cfg.hardware, output=Old(cfg.output, ("save_masks",)))
    with pytest.raises(KeyboardInterrupt):
        stv_main.style_transfer(InputPaths(p["content"], p["style"]), old)
    assert sorted(seen[-1][1]) == ["precision"]

    # with the option on, the maps arrive as maps from files do; a pair that does not split arrives without
    calls = []
    c_lab, s_lab = torch.zeros(64, 64, dtype=torch.uint8), torch.ones(64, 64, dtype=torch.uint8)

    def guidance_probe(content, style, oc, levels):
        calls.append((tuple(content.shape), tuple(style.shape), levels))
        return (c_lab, s_lab) if len(calls) == 1 else None
    monkeypatch.setattr(segment, "auto_guidance", guidance_probe)
    cfg.optimization.auto_mask = True
    for want in (["content_labels", "precision", "style_labels"], ["precision"]):
        with pytest.raises(KeyboardInterrupt):
            stv_main.style_transfer(InputPaths(p["content"], p["style"]), cfg)
        assert sorted(seen[-1][1]) == want
    assert seen[-2][1]["content_labels"] is c_lab and seen[-2][1]["style_labels"] is s_lab
    assert calls == [((1, 3, 64, 64), (1, 3, 64, 64), 1)] * 2


# ---- 7. ABI -----------------------------------------------------------------------------------------------------------------

def test_library_exports_the_entry_point_and_the_constants_match_the_header():
    lib = _lib.load()
    assert hasattr(lib, "stv_kmeans_assign") and "stv_kmeans_assign" in _lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "stv.h")).read()
    for name, value in (("STV_KMEANS_THREADS", _lib.KMEANS_THREADS), ("STV_KMEANS_PARTS", _lib.KMEANS_PARTS),
                        ("STV_KMEANS_PART_DOUBLES", _lib.KMEANS_PART_DOUBLES)):
        assert re.search(rf"#define {name} {value}\b", header), name
    assert (_lib.KMEANS_THREADS, _lib.KMEANS_PARTS, _lib.KMEANS_PART_DOUBLES) == (256, 256, 17)
    assert _lib.KMEANS_PART_DOUBLES == 4 * _lib.KMEANS_MAX_K + 1 and _lib.KMEANS_MAX_K == guidance.MAX_REGIONS
    assert lib.stv_version() >= 114
    assert "kmeans.hip" in open(os.path.join(ROOT, "style_transfer_visualizer_amd", "csrc", "Makefile")).read()
    assert "STV_OP_KMEANS" not in header                 # set-up work: not an op of the step program
    assert segment.CELLS == _lib.LAP_POOLS


def test_argument_refusals_run_without_a_gpu():
    lib = _lib.load()
    buf = (ctypes.c_char * 8192)()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    x, c, lab, parts = base, base + 1024, base + 2048, base + 3072
    ERR = 1

    def call(x=x, c=c, lab=lab, parts=parts, H=4, W=4, K=2):
        return lib.stv_kmeans_assign(x, c, lab, parts, H, W, K, None)
    assert call(x=None) == call(c=None) == call(lab=None) == call(parts=None) == ERR
    for bad in (dict(H=0), dict(W=0), dict(H=-1), dict(W=-4), dict(K=0), dict(K=5), dict(K=-1), dict(K=1 << 30)):
        assert call(**bad) == ERR, bad
    # 3*H*W*4 bytes of 2 GiB or more, and sizes whose product overflows an int
    assert call(H=1 << 14, W=(1 << 14) // 3 * 2 + 2) == call(H=1 << 16, W=1 << 16) == call(H=1 << 30, W=1 << 30) == ERR
