"""Automatic masks in VGG feature space (``--auto-mask-space features``; ``segment.feature_labels``, ``stv_kmeans_feat_*``)
without a GPU: the NumPy twins' own rules on hand-sized cases, the whole algorithm through the twins on the stripes pair (two
images of one colour distribution that differ in the direction of their texture), the start, config and CLI, every refusal,
the option off, and the ABI of the two entry points."""
from __future__ import annotations

import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from style_transfer_visualizer_amd import _lib, cli, config_defaults, core_model, guidance, segment
from style_transfer_visualizer_amd import config as stv_config
from style_transfer_visualizer_amd import main as stv_main
from style_transfer_visualizer_amd.type_defs import InputPaths
from tests import feature_mask_inputs as fi
from tests import kmeans_feat_ref as ref
from tests import kmeans_ref as colour_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _options(**kw):
    base = {"auto_mask": True, "auto_mask_space": "features", "auto_mask_layer": fi.LAYER, "mask_regions": 2,
            "style_layers": [0, 5, 10, 19, 28]}
    return types.SimpleNamespace(**{**base, **kw})


# ---- 1. the twins' own rules -------------------------------------------------------------------------------------------------

def test_the_distance_is_summed_octet_by_octet_and_then_pairwise():
    rng = np.random.default_rng(0)
    x, c = rng.standard_normal((5, 64)).astype(F32), rng.standard_normal((3, 64)).astype(F32)
    d = ref.distances(x, c)
    assert d.dtype == F32 and d.shape == (5, 3)
    for p in range(5):
        for k in range(3):
            octets = []
            for o in range(8):
                s = F32(0.0)
                for j in range(8):
                    e = F32(x[p, 8 * o + j] - c[k, 8 * o + j])
                    s = F32(s + F32(e * e))
                octets.append(s)
            q = [F32(octets[i] + octets[i + 4]) for i in range(4)]
            q = [F32(q[i] + q[i + 2]) for i in range(2)]
            assert d[p, k] == F32(q[0] + q[1])
    assert np.allclose(d, ((x[:, None].astype(np.float64) - c[None]) ** 2).sum(-1), rtol=1e-5)


def test_ties_go_to_the_lowest_index_and_a_nan_never_wins():
    d = np.array([[1.0, 1.0, 2.0], [3.0, 2.0, 2.0], [np.nan, 5.0, 4.0], [np.nan, np.nan, np.nan], [np.inf, np.inf, np.inf],
                  [np.nan, 7.0, 7.0]], dtype=F32)
    assert ref.nearest(d).tolist() == [0, 1, 2, 0, 0, 1]
    x = np.zeros((1, 64), dtype=F32)
    c = np.stack([np.full(64, 2.0, F32), np.full(64, -2.0, F32)])
    labels, parts = ref.assign(x, c, np.array([255], dtype=np.uint8))
    assert labels.tolist() == [0] and parts[:, -1].sum() == 1 and parts[0, 64] == 1


def test_labels_in_place_counts_and_the_kept_mode():
    rng = np.random.default_rng(1)
    C, n = 128, 50
    x = rng.standard_normal((n, C)).astype(F32)
    c = rng.standard_normal((3, C)).astype(F32)
    labels, parts = ref.assign(x, c, np.full(n, 255, np.uint8))
    assert parts.shape == (_lib.KMF_PARTS, _lib.kmf_row_doubles(C)) == (256, 4 * 129 + 1)
    assert parts[:, -1].sum() == n and not parts[:, 3 * (C + 1):-1].any()
    for k in range(3):
        assert parts[:, k * (C + 1) + C].sum() == (labels == k).sum()
        assert np.allclose(parts[:, k * (C + 1):k * (C + 1) + C].sum(axis=0), x[labels == k].astype(np.float64).sum(axis=0), rtol=1e-12, atol=1e-12)
    again, parts = ref.assign(x, c, labels)
    assert np.array_equal(again, labels) and parts[:, -1].sum() == 0
    kept = labels.copy()
    kept[::5] = 255                                            # a label >= K is in no sum
    same, parts = ref.assign(x, c, kept, keep_labels=True)
    assert np.array_equal(same, kept) and not parts[:, -1].any()
    assert sum(parts[:, k * (C + 1) + C].sum() for k in range(3)) == (kept != 255).sum()      # noqa: PLR2004
    # adapters: labels of a tensor in place, untouched in the kept mode
    t = torch.full((n,), 255, dtype=torch.uint8)
    ref.assign_op(torch.from_numpy(x), torch.from_numpy(c), t)
    assert np.array_equal(t.numpy(), labels)
    ref.assign_op(torch.from_numpy(x), torch.from_numpy(c[:1]), t, keep_labels=True)
    assert np.array_equal(t.numpy(), labels)


def test_the_sums_follow_the_launch_geometry():
    """Pixel p of a [n, C] image sits in workgroup (p % per_pass) // (4 G): one pixel per workgroup row shows the mapping; values
    chosen so that double addition is inexact show the order pass -> group pairs -> waves."""
    for C in (64, 128, 256, 512):
        Q, G, per_pass = _lib.kmf_geometry(C)
        assert Q * G == 64 and per_pass == 256 * 4 * G                # noqa: PLR2004
        n = per_pass + 3
        x = np.zeros((n, C), dtype=F32)
        x[:, 0] = np.arange(1, n + 1)
        _, parts = ref.assign(x, np.zeros((1, C), F32), np.zeros(n, np.uint8), keep_labels=True)
        p = np.arange(n)
        want = np.zeros(256)
        np.add.at(want, (p % per_pass) // (4 * G), x[:, 0].astype(np.float64))
        assert np.array_equal(parts[:, 0], want) and np.array_equal(parts[:, C], np.bincount((p % per_pass) // (4 * G), minlength=256))
    # order: workgroup 0 of C = 64 holds pixels 0..31 (4 waves of 8) in pass 0 and per_pass.. in pass 1
    C, (_, G, per_pass) = 64, _lib.kmf_geometry(64)
    vals = np.array([1.0, 2.0 ** -30, -1.0, 2.0 ** 30, 3.0, 2.0 ** -40, 7.0, -2.0 ** 30] * 4, dtype=F32)
    x = np.zeros((per_pass + 32, C), dtype=F32)
    x[:32, 5], x[per_pass:, 5] = vals, vals[::-1] * F32(3.0)
    _, parts = ref.assign(x, np.zeros((1, C), F32), np.zeros(len(x), np.uint8), keep_labels=True)
    lane = x[:32, 5].astype(np.float64) + x[per_pass:, 5].astype(np.float64)        # pass order, per (wave, group)
    lane = lane.reshape(4, 8)
    wave = (lane[:, 0] + lane[:, 4]) + (lane[:, 2] + lane[:, 6]), (lane[:, 1] + lane[:, 5]) + (lane[:, 3] + lane[:, 7])
    wave = wave[0] + wave[1]
    assert parts[0, 5] == ((0.0 + wave[0]) + wave[1]) + wave[2] + wave[3]


def test_update_weighs_each_image_one_half_and_keeps_an_empty_cluster():
    C = 64
    parts_c, parts_s = (np.zeros((256, _lib.kmf_row_doubles(C))) for _ in range(2))
    parts_c[0, :C], parts_c[0, C] = 10.0, 10            # cluster 0: 10 of 100 content pixels of value 1 ...
    parts_s[3, :C], parts_s[3, C] = 90.0, 30            # ... and 30 of 60 style pixels of value 3
    parts_c[5, C + 1:2 * C + 1], parts_c[5, 2 * C + 1] = 8.0, 4      # cluster 1: content only
    parts_c[9, -1], parts_s[200, -1] = 5, 7
    start = np.arange(3 * C, dtype=F32).reshape(3, C)
    cen, result = ref.update(parts_c, parts_s, start, 100, 60)
    want0 = (10.0 / 100 + 90.0 / 60) / (10 / 100 + 30 / 60)
    assert np.array_equal(cen[0], np.full(C, F32(want0))) and np.array_equal(cen[1], np.full(C, F32(2.0)))
    assert np.array_equal(cen[2], start[2])                              # empty in both: kept
    assert result.tolist() == [10, 4, 0, 0, 30, 0, 0, 0, 12]


# ---- 2. the whole algorithm on the stripes pair ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def stripes_features():
    content, style = fi.stripes_tensors(64)
    return content, style, fi.cpu_features(content), fi.cpu_features(style)


def test_the_stripes_pair_splits_into_the_halves_in_feature_space(stripes_features):
    _, _, F_c, F_s = stripes_features
    assert tuple(F_c.shape) == tuple(F_s.shape) == (16, 16, 256)
    grid_c, grid_s, info = segment.feature_labels(F_c, F_s, 2, **ref.HOST)
    want_c, want_s = fi.half_grids(16)
    differ = int((grid_c != want_c).sum()), int((grid_s != want_s).sum())
    print(f"stripes 64: {info['iterations']} iterations, cells {info['cells']}, differing cells {differ}")
    assert info["converged"] and info["iterations"] <= segment.MAX_ITER
    assert max(differ) <= fi.DIFFER_CAP                       # region 0 is the vertical stripes in both images
    assert grid_c.dtype == torch.uint8 and tuple(grid_c.shape) == (16, 16) and info["grids"] == [(16, 16), (16, 16)]
    assert info["cells"]["content"] == [int((grid_c == k).sum()) for k in range(2)]
    # given the centroids it ended with, one more call changes nothing and needs one iteration
    again_c, again_s, again = segment.feature_labels(F_c, F_s, 2, centroids=info["centroids"], **ref.HOST)
    assert torch.equal(again_c, grid_c) and torch.equal(again_s, grid_s) and again["start"] is None


def test_auto_guidance_in_feature_space_gives_image_size_maps(stripes_features, caplog):
    content, style, _, _ = stripes_features
    oc = _options(mask_regions=3)
    with caplog.at_level("INFO"):
        maps = segment.auto_guidance(content, style, oc, 1, extract=fi.cpu_extract, **ref.HOST)
    assert maps is not None and oc.mask_regions in (2, 3)
    assert "Automatic masks: feature space, layer 10 (grids 16x16 and 16x16, 256 channels)" in caplog.text
    assert all(m.dtype == torch.uint8 and tuple(m.shape) == (64, 64) for m in maps)
    oc = _options()
    caplog.clear()
    with caplog.at_level("INFO"):
        content_labels, style_labels = segment.auto_guidance(content, style, oc, 1, extract=fi.cpu_extract, **ref.HOST)
    assert "2 regions (asked for 2)" in caplog.text and oc.mask_regions == 2      # noqa: PLR2004
    grids = fi.half_grids(16)
    for got, want in zip((content_labels, style_labels), grids, strict=True):
        assert torch.equal(got, guidance.resample_labels(got[2::4, 2::4].contiguous(), 64, 64))      # constant per 4x4 cell
        assert int((got[2::4, 2::4] != want).sum()) <= fi.DIFFER_CAP


def test_the_same_pair_in_colour_mode_is_not_accepted_and_runs_unguided(stripes_features, caplog):
    content, style, _, _ = stripes_features
    oc = _options(auto_mask_space="color")
    with caplog.at_level("INFO"):
        assert segment.auto_guidance(content, style, oc, 1, **colour_ref.HOST) is None
    assert "2 regions not accepted" in caplog.text and "proceeds unguided" in caplog.text
    no_fields = types.SimpleNamespace(auto_mask=True, mask_regions=2, style_layers=[0, 5, 10, 19, 28])
    assert segment.auto_guidance(content, style, no_fields, 1, **colour_ref.HOST) is None      # without the fields: colour


def _pool_fp32_in_row_order(img: torch.Tensor, cell: int) -> torch.Tensor:
    """Box means as an fp32 kernel forms them: the box's values added one after the other in fp32, row by row, times 1/m.  The sum
    of the same 32 + 32 values then depends on where they sit, which a float64 mean rounded once does not show."""
    x = img.detach().cpu().numpy().reshape(3, img.shape[-2], img.shape[-1]).astype(F32)
    h, w = x.shape[1] // cell, x.shape[2] // cell
    boxes = x[:, :h * cell, :w * cell].reshape(3, h, cell, w, cell).transpose(0, 1, 3, 2, 4).reshape(3, h, w, cell * cell)
    acc = np.zeros((3, h, w), dtype=F32)
    for j in range(cell * cell):
        acc = acc + boxes[..., j]
    return torch.from_numpy(acc * F32(1.0 / (cell * cell)))


def test_box_means_that_differ_only_by_fp32_rounding_are_no_spread(stripes_features, caplog):
    """The stripes pair again, pooled in fp32: the box means now differ in their last bits by stripe direction.  Without the floor
    of ``segment.pooling_noise`` the colour k-means splits the pair on that rounding; with it the run is unguided, as with exact
    box means."""
    content, style, _, _ = stripes_features
    pooled = [_pool_fp32_in_row_order(img, 8) for img in (content, style)]
    assert len(np.unique(pooled[0][0].numpy())) > 1                         # the rounding is there
    stats = [colour_ref.moments_op(p) for p in pooled]
    noise = segment.pooling_noise([colour_ref.moments_op(img) for img in (content, style)], 8)
    spread = segment.initial_centroids(stats, 2)
    assert not np.array_equal(spread[0], spread[1])                         # without the floor: two centroids a rounding apart
    floored = segment.initial_centroids(stats, 2, noise)
    assert np.array_equal(floored[0], floored[1])
    assert 0.0 < noise < 1e-9 and segment.pooling_noise(stats, 1) == 0.0    # far below any spread an 8-bit image can hold
    calls = []

    def counting_moments(img):
        calls.append(tuple(img.shape[-2:]))
        return colour_ref.moments_op(img)
    kernels = {**colour_ref.HOST, "pool": _pool_fp32_in_row_order, "moments": counting_moments}
    with caplog.at_level("INFO"):
        assert segment.auto_guidance(content, style, _options(auto_mask_space="color", mask_regions=3), 1, **kernels) is None
    assert calls == [(64, 64)] * 2 + [(8, 8)] * 4             # the raw images once for both R tried, the pooled maps per R
    ragged = torch.zeros(1, 3, 70, 83)
    calls.clear()
    segment.image_noise((ragged, ragged), 8, counting_moments)
    assert calls == [(64, 80)] * 2                            # the pixels the boxes cover
    kernels["moments"] = colour_ref.moments_op
    assert "2 regions not accepted" in caplog.text and "proceeds unguided" in caplog.text
    # a pair that does split is untouched by the floor: its spread is many orders above it
    yy, xx = np.mgrid[0:64, 0:64]
    dark_left = torch.from_numpy(np.where(xx < 32, 0.2, 0.8).astype(F32)).expand(1, 3, 64, 64).contiguous()
    maps = segment.auto_guidance(dark_left, dark_left, _options(auto_mask_space="color"), 1, **kernels)
    assert maps is not None and int(maps[0][0, 0]) == 0 and int(maps[0][0, 63]) == 1


# ---- 3. the start ------------------------------------------------------------------------------------------------------------

def test_the_start_lies_on_the_principal_axis_with_the_sign_rule_in_c_dimensions():
    rng = np.random.default_rng(3)
    C = 64
    axis = np.zeros(C)
    axis[3], axis[10] = 0.6, -0.8                                     # sums to a negative number: the rule flips it
    pts = rng.standard_normal((400, 1)) * 5.0 * axis[None] + rng.standard_normal((400, C)) * 0.01 + 2.0
    F = torch.from_numpy(pts.astype(F32)).reshape(20, 20, C)
    stats = [ref.moments_op(F), ref.moments_op(F)]
    start = segment.feature_start(stats, 4)
    assert start["centroids"].dtype == F32 and start["centroids"].shape == (4, C)
    v = start["v"]
    assert v.sum() >= 0 and abs(abs(v @ axis) - 1.0) < 1e-4 and v[10] > 0 > v[3]          # noqa: PLR2004
    assert np.allclose(start["mu"], pts.astype(F32).astype(np.float64).mean(axis=0))
    z = np.array([-0.75, -0.25, 0.25, 0.75])
    want = start["mu"][None] + np.sqrt(start["lam"]) * z[:, None] * v[None]
    assert np.array_equal(start["centroids"], want.astype(F32))
    # v.(1,...,1) == 0: the first non-zero component decides
    v2, _ = segment.principal_axis(np.outer([0, -1.0, 1.0, 0], [0, -1.0, 1.0, 0]))
    assert v2[1] > 0 > v2[2]
    # each image weighs 1/2 whatever its size
    small, large = ref.moments_op(F[:5]), ref.moments_op(F)
    mu = segment.feature_start([small, large], 2)["mu"]
    assert np.allclose(mu, (small[1] / small[0] + large[1] / large[0]) / 2)


def test_zero_variance_gives_coincident_centroids_and_a_refusal_not_an_error(caplog):
    F = torch.full((8, 8, 64), 0.5)
    start = segment.feature_start([ref.moments_op(F)] * 2, 3)
    assert np.array_equal(start["centroids"], np.full((3, 64), 0.5, F32))
    grid_c, _, info = segment.feature_labels(F, F, 3, **ref.HOST)
    assert not bool(grid_c.any()) and info["cells"]["content"] == [64, 0, 0] and info["iterations"] == 2      # noqa: PLR2004
    img = torch.zeros(1, 3, 32, 32)
    with caplog.at_level("INFO"):
        out = segment.auto_guidance(img, img, _options(mask_regions=3), 1, extract=lambda *a: [F, F], **ref.HOST)
    assert out is None and "3 regions not accepted: region 1 holds 0 of the 64 cells" in caplog.text
    assert "proceeds unguided" in caplog.text


# ---- 4. config, CLI, refusals ----------------------------------------------------------------------------------------------------

def _cli_config(argv):
    args = cli.build_arg_parser().parse_args(argv)
    base = stv_config.ConfigLoader.load(args.config) if args.config else None
    return stv_config.build_config_from_cli(vars(args), base_config=base)


def test_config_and_cli_round_trip(tmp_path, caplog, capsys):
    base = ["--content", "c.png", "--style", "s.png"]
    assert (config_defaults.DEFAULT_AUTO_MASK_SPACE, config_defaults.DEFAULT_AUTO_MASK_LAYER) == ("color", 10) == (segment.SPACES[0], segment.DEFAULT_LAYER)
    for cfg in (stv_config.StyleTransferConfig.model_validate({}), _cli_config(base)):
        assert (cfg.optimization.auto_mask_space, cfg.optimization.auto_mask_layer) == ("color", 10)
    cfg = _cli_config([*base, "--auto-mask", "--auto-mask-space", "features", "--auto-mask-layer", "12"])
    assert (cfg.optimization.auto_mask, cfg.optimization.auto_mask_space, cfg.optimization.auto_mask_layer) == (True, "features", 12)
    toml = tmp_path / "config.toml"
    toml.write_text("[optimization]\nauto_mask = true\nauto_mask_space = \"features\"\nauto_mask_layer = 5\n")
    for cfg in (stv_config.ConfigLoader.load(str(toml)), _cli_config(["--config", str(toml)])):
        assert (cfg.optimization.auto_mask_space, cfg.optimization.auto_mask_layer) == ("features", 5)
    assert _cli_config(["--config", str(toml), "--auto-mask-layer", "7"]).optimization.auto_mask_layer == 7      # noqa: PLR2004
    toml.write_text("[optimization]\nauto_mask_space = \"hsv\"\n")
    with pytest.raises(ValueError, match="auto_mask_space"):
        stv_config.ConfigLoader.load(str(toml))
    with pytest.raises(SystemExit):
        cli.build_arg_parser().parse_args([*base, "--auto-mask-space", "hsv"])
    assert "invalid choice: 'hsv'" in capsys.readouterr().err
    assert not hasattr(cli.build_arg_parser().parse_args(base), "auto_mask_space")
    paths = InputPaths(content_path="c.png", style_path="s.png")
    with caplog.at_level("INFO"):
        cli.log_parameters(paths, _cli_config([*base, "--auto-mask"]))
    assert "Automatic Mask Cell: 8" in caplog.text and "Automatic Mask Space" not in caplog.text and "Automatic Mask Layer" not in caplog.text
    caplog.clear()
    with caplog.at_level("INFO"):
        cli.log_parameters(paths, _cli_config([*base, "--auto-mask", "--auto-mask-space", "features"]))
    for line in ("Automatic Masks: Enabled", "Mask Regions: 2", "Automatic Mask Space: features", "Automatic Mask Layer: 10"):
        assert line in caplog.text
    assert "Automatic Mask Cell" not in caplog.text


def test_every_refusal_names_its_values_and_comes_before_a_device_is_touched(tmp_path):
    content, style = fi.write_stripes(tmp_path)

    def run(paths=None, auto_mask=True, **kw):
        cfg = stv_config.StyleTransferConfig.model_validate({})
        cfg.hardware.device = "no-such-device"
        cfg.optimization.auto_mask = auto_mask
        object.__setattr__(cfg.optimization, "auto_mask_space", "features")
        for key, value in kw.items():
            object.__setattr__(cfg.optimization, key, value)
        stv_main.style_transfer(paths or InputPaths(content, style), cfg)
    with pytest.raises(ValueError, match=re.escape("--auto-mask-space features without --auto-mask")):
        run(auto_mask=False)
    for bad in ("hsv", "", None, 3):
        with pytest.raises(ValueError, match=re.escape(f"auto_mask_space must be one of ['color', 'features'], got {bad!r}")):
            run(auto_mask_space=bad)
        with pytest.raises(ValueError, match=re.escape(f"got {bad!r}")):
            run(auto_mask=False, auto_mask_space=bad)
    for bad in (4, 9, 18, 27, 36, 37, -1, "10", True, 2.0):
        with pytest.raises(ValueError, match=re.escape(f"auto_mask_layer must be a conv or ReLU index of the VGG19 stack (0 to 36 without "
                                                       f"the pooling layers [4, 9, 18, 27, 36]), got {bad!r}")):
            run(auto_mask_layer=bad)
    # everything --auto-mask refuses today
    with pytest.raises(ValueError, match=re.escape("--auto-mask cannot be combined with --content-mask / --style-mask")):
        run(InputPaths(content, style, content_mask_path=content, style_mask_path=style))
    with pytest.raises(ValueError, match=re.escape("--auto-mask cannot be combined with --style-also (1 further style images)")):
        run(InputPaths(content, style, extra_style_paths=(style,)))
    with pytest.raises(ValueError, match=re.escape("--auto-mask cannot be combined with --region-weights ([1.0, 0.5])")):
        run(region_weights=[1.0, 0.5])
    with pytest.raises(ValueError, match="mask_regions must be an integer from 2 to 4, got 5"):
        run(mask_regions=5)
    # in feature space the cell size is unused and not looked at
    with pytest.raises(Exception, match="no-such-device|device") as info:
        run(auto_mask_cell=3)
    assert "auto_mask_cell" not in str(info.value)
    # in colour mode the layer is not looked at
    with pytest.raises(Exception, match="no-such-device|device") as info:
        cfg = stv_config.StyleTransferConfig.model_validate({})
        cfg.hardware.device, cfg.optimization.auto_mask = "no-such-device", True
        object.__setattr__(cfg.optimization, "auto_mask_layer", 4)
        stv_main.style_transfer(InputPaths(content, style), cfg)
    assert "auto_mask_layer" not in str(info.value)


def test_grids_too_small_are_refused_before_the_first_launch():
    def never(*a, **k):
        raise AssertionError("a kernel was launched")
    kernels = {"extract": never, "assign": never, "update": never, "moments": never}
    big, small = torch.zeros(1, 3, 64, 96), torch.zeros(1, 3, 31, 200)
    msg = ("--auto-mask-space features: layer 10 leaves a 24x16 grid of the 96x64 content image and a 50x7 grid of the 200x31 style "
           "image; the shorter side needs at least 8")
    with pytest.raises(ValueError, match=re.escape(msg)):
        segment.auto_guidance(big, small, _options(), 1, **kernels)
    with pytest.raises(ValueError, match=re.escape("leaves a 50x7 grid of the 200x31 content image and a 24x16 grid of the 96x64 style")):
        segment.auto_guidance(small, big, _options(), 1, **kernels)
    with pytest.raises(ValueError, match=re.escape("layer 28 leaves a 6x4 grid of the 96x64 content image and a 6x4 grid")):
        segment.auto_guidance(big, big, _options(auto_mask_layer=28), 1, **kernels)
    with pytest.raises(AssertionError, match="a kernel was launched"):          # 12x8 at layer 19: it fits
        segment.auto_guidance(big, big, _options(auto_mask_layer=19), 1, **kernels)
    # a feature map of 2^31 elements or more is refused by name, before the extraction
    huge = torch.zeros(1, 3, 1, 1).expand(1, 3, 8192, 4096)
    with pytest.raises(ValueError, match=re.escape("layer 0 gives 4096x8192 pixels of 64 channels of the content image, 2147483648 "
                                                   "elements; the feature k-means takes fewer than 2147483648")):
        segment.auto_guidance(huge, big, _options(auto_mask_layer=0), 1, **kernels)
    with pytest.raises(ValueError, match="of the style image, 2147483648 elements"):
        segment.auto_guidance(big, huge, _options(auto_mask_layer=1), 1, **kernels)
    segment.check_feature_sizes((8192, 4095), (64, 64), 0)
    assert segment.feature_grid((64, 96), 0) == (64, 96) and segment.feature_grid((65, 97), 10) == (16, 24)
    assert [segment.layer_table()[i] for i in (0, 1, 4, 10, 35, 36)] == [("conv", 64, 0), ("relu", 64, 0), ("pool", 64, 1), ("conv", 256, 2),
                                                                         ("relu", 512, 4), ("pool", 512, 5)]


def test_with_the_option_off_the_calls_are_todays(monkeypatch, tmp_path):
    content, style = fi.write_stripes(tmp_path)
    seen, calls = [], []

    def probe(*args, **kw):
        seen.append((args, kw))
        raise KeyboardInterrupt          # (the call is what is looked at: nothing is built)
    monkeypatch.setattr(core_model, "prepare_model_and_input", probe)
    for name in ("auto_guidance", "auto_labels", "feature_labels", "run_features", "extract_features", "feature_moments", "save_label_png"):
        monkeypatch.setattr(segment, name, lambda *a, **k: pytest.fail("the option is off"))
    cfg = stv_config.StyleTransferConfig.model_validate({})
    cfg.video.create_video = False

    class Old:          # a config whose sections predate the options
        def __init__(self, section, drop):
            self.__dict__.update({k: v for k, v in section.model_dump().items() if k not in drop})
    old = types.SimpleNamespace(optimization=Old(cfg.optimization, ("auto_mask_space", "auto_mask_layer")), video=cfg.video,
                                hardware=cfg.hardware, output=cfg.output)
    assert not hasattr(old.optimization, "auto_mask_space")
    for config in (cfg, old):
        with pytest.raises(KeyboardInterrupt):
            stv_main.style_transfer(InputPaths(content, style), config)
        args, kw = seen[-1]
        assert sorted(kw) == ["precision"] and len(args) == 4 and args[3] is config.optimization

    # --auto-mask without the new fields, and with the space at its default: segment is called as it is today
    def guidance_probe(*args, **kw):
        calls.append((len(args), sorted(kw)))
    monkeypatch.setattr(segment, "auto_guidance", guidance_probe)
    old.optimization.auto_mask = cfg.optimization.auto_mask = True
    for config in (cfg, old):
        with pytest.raises(KeyboardInterrupt):
            stv_main.style_transfer(InputPaths(content, style), config)
    assert calls == [(4, []), (4, [])]
    cfg.optimization.auto_mask_space = "features"
    cfg.hardware.precision = "bf16"
    with pytest.raises(KeyboardInterrupt):
        stv_main.style_transfer(InputPaths(content, style), cfg)
    assert calls[-1] == (4, ["precision"])


def test_the_extraction_leaves_the_generator_alone_and_builds_the_stack_once_per_process(monkeypatch):
    monkeypatch.setenv("STV_SYNTHETIC_WEIGHTS", "0")
    monkeypatch.delenv("STV_PRECISION", raising=False)        # (a precision of None is the model's default: fp32)
    core_model.clear_vgg_cache()
    built, seen = [], []
    build = core_model.build_vgg_features

    def counting(*a, **k):
        built.append(1)
        return build(*a, **k)
    monkeypatch.setattr(core_model, "build_vgg_features", counting)
    monkeypatch.setattr(segment, "extract_features", lambda img, layers, layer, dtype, split=False: seen.append((len(layers), layer, dtype, split)))
    img = torch.zeros(1, 3, 64, 64)
    for seed, precision in ((1, "fp32"), (2, "bf16"), (3, None)):
        torch.manual_seed(seed)
        torch.rand(seed)                                      # a generator state the cache has never seen
        before = torch.get_rng_state()
        segment.run_features(img, img, 10, types.SimpleNamespace(pooling="avg"), precision)
        assert torch.equal(torch.get_rng_state(), before)
    assert len(built) == 1 and len(seen) == 6                 # noqa: PLR2004
    assert seen[0] == (37, 10, torch.float32, False) and seen[2][2] == torch.bfloat16 and seen[4][2] == torch.float32
    core_model.clear_vgg_cache()


# ---- 5. ABI ------------------------------------------------------------------------------------------------------------------

def test_library_exports_the_entry_points_and_the_constants_match_the_header():
    lib = _lib.load()
    for name in ("stv_kmeans_feat_assign", "stv_kmeans_feat_update"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "stv.h")).read()
    for name, value in (("STV_KMF_THREADS", _lib.KMF_THREADS), ("STV_KMF_WAVES", _lib.KMF_WAVES), ("STV_KMF_PARTS", _lib.KMF_PARTS),
                        ("STV_KMF_MAX_K", _lib.KMF_MAX_K), ("STV_KMF_MAX_C", _lib.KMF_MAX_C)):
        assert re.search(rf"#define {name} {value}\b", header), name
    assert "#define STV_KMF_ROW_DOUBLES(C) (4 * ((C) + 1) + 1)" in header and _lib.kmf_row_doubles(512) == 2053      # noqa: PLR2004
    assert _lib.KMF_CHANNELS == (64, 128, 256, 512) and all(c in header for c in ("C = 64, 128, 256 or 512", "192, 320, 384 and 448"))
    assert _lib.KMF_THREADS == 64 * _lib.KMF_WAVES and _lib.KMF_MAX_K == guidance.MAX_REGIONS
    assert [_lib.kmf_geometry(C) for C in (64, 128, 256, 512)] == [(8, 8, 8192), (16, 4, 4096), (32, 2, 2048), (64, 1, 1024)]
    assert lib.stv_version() >= 117
    assert "kmeans_feat.hip" in open(os.path.join(ROOT, "style_transfer_visualizer_amd", "csrc", "Makefile")).read()
    assert "STV_OP_KMEANS" not in header and "STV_OP_KMF" not in header           # set-up work: not ops of the step program


def test_argument_refusals_run_without_a_gpu():
    lib = _lib.load()
    buf = (ctypes.c_char * 8192)()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    F, c, lab, parts, res = base, base + 1024, base + 2048, base + 3072, base + 4096
    ERR = 1

    def assign(F=F, dtype=_lib.STV_F32, c=c, lab=lab, parts=parts, n=4, C=64, K=2, keep=0):
        return lib.stv_kmeans_feat_assign(F, dtype, c, lab, parts, n, C, K, keep, None)

    def update(pc=parts, ps=parts, c=c, res=res, n_c=4, n_s=4, C=64, K=2):
        return lib.stv_kmeans_feat_update(pc, ps, c, res, n_c, n_s, C, K, None)
    assert assign(F=None) == assign(c=None) == assign(lab=None) == assign(parts=None) == ERR
    assert update(pc=None) == update(ps=None) == update(c=None) == update(res=None) == ERR
    shapes = (dict(C=0), dict(C=32), dict(C=96), dict(C=192), dict(C=320), dict(C=384), dict(C=448), dict(C=576), dict(C=1024), dict(C=-64), dict(K=0), dict(K=5), dict(K=-1))
    for bad in shapes:
        assert assign(**bad) == ERR and update(**bad) == ERR, bad
    for bad in (dict(n=0), dict(n=-3), dict(dtype=_lib.STV_BF16X3), dict(dtype=99), dict(F=F + 4), dict(n=1 << 22, C=512)):
        assert assign(**bad) == ERR, bad
    for bad in (dict(n_c=0), dict(n_s=0), dict(n_c=-1)):
        assert update(**bad) == ERR, bad
