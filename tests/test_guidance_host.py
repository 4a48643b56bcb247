"""Spatial guidance without a GPU: the label-map rules of guidance.py, every refusal, the configuration and command-line round
trip, the ABI of stv_mask_split, and the guided step as a host engine in device form builds it."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

from style_transfer_visualizer_amd import _lib, cli, core_model, guidance, plan, pyramid, spatial
from style_transfer_visualizer_amd import config as stv_config
from style_transfer_visualizer_amd import main as stv_main
from style_transfer_visualizer_amd.type_defs import InputPaths
from tests.test_core_model_host import CPU, RecordedProgram, _image, _layers, fused_step, host_engine, step_signature

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_TAPS = ([0, 5, 10, 19, 28], [21])


def halves(H, W):
    lab = torch.zeros(H, W, dtype=torch.uint8)
    lab[:, W // 2:] = 1
    return lab


# ---- label maps ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [2, 3, 4])
def test_band_quantisation_on_all_levels(R):
    grey = np.arange(256, dtype=np.uint8).reshape(16, 16)
    got = guidance.quantize(grey, R)
    assert got.dtype == torch.uint8 and got.shape == (16, 16)
    for v in range(256):
        assert int(got.reshape(-1)[v]) == min(R - 1, v * R // 256)
    assert int(got.reshape(-1)[0]) == 0 and int(got.reshape(-1)[255]) == R - 1
    # R uniform bands: black and white are the first and the last region, and a few levels of noise stay inside
    assert len({int(v) for v in got.reshape(-1)[:20]}) == 1 and len({int(v) for v in got.reshape(-1)[-20:]}) == 1
    counts = torch.bincount(got.reshape(-1).long())
    assert counts.numel() == R and int(counts.max() - counts.min()) <= 1


@pytest.mark.parametrize("size", [(37, 50), (3, 5), (75, 101), (150, 202)])
def test_resample_labels_is_the_nearest_rule_in_integers(size):
    g = torch.Generator().manual_seed(1)
    H0, W0 = 75, 101
    labels = torch.randint(0, 4, (H0, W0), generator=g).to(torch.uint8)
    H, W = size
    got = guidance.resample_labels(labels, H, W)
    assert got.shape == (H, W) and got.dtype == torch.uint8 and got.is_contiguous()
    # brute force in float64: the source pixel under the output pixel's centre
    for y in range(H):
        sy = int(np.floor((y + 0.5) * np.float64(H0) / np.float64(H)))
        assert sy == ((2 * y + 1) * H0) // (2 * H)
        for x in range(W):
            sx = int(np.floor((x + 0.5) * np.float64(W0) / np.float64(W)))
            assert int(got[y, x]) == int(labels[sy, sx])
    if size == (H0, W0):
        assert got is labels


def test_crop_and_resample_bookkeeping_of_a_two_level_pyramid():
    g = torch.Generator().manual_seed(2)
    content = torch.randint(0, 2, (128, 192), generator=g).to(torch.uint8)
    style = torch.randint(0, 2, (131, 150), generator=g).to(torch.uint8)
    oc = stv_config.StyleTransferConfig.model_validate({}).optimization
    oc.region_weights = [1.0, 0.5]
    chain = pyramid.level_labels(content, style, (130, 150), 2, 1, oc)
    assert len(chain) == 2
    (kw0, lab0), (kw1, lab1) = chain                     # coarsest first
    assert kw0 == kw1 == {"guide_regions": 2, "region_weights": [1.0, 0.5]}
    assert lab1["content_labels"] is content
    assert torch.equal(lab1["style_labels"], style[:130, :150])            # the style's crop: the same slice
    assert torch.equal(lab0["content_labels"], guidance.resample_labels(content, 64, 96))
    assert torch.equal(lab0["style_labels"], guidance.resample_labels(style[:130, :150].contiguous(), 65, 75))
    # a halving reads the odd rows and columns
    assert torch.equal(lab0["content_labels"], content[1::2, 1::2])
    assert pyramid.level_labels(None, None, (130, 150), 2, 1, oc) is None
    small = torch.zeros(128, 192, dtype=torch.uint8)
    small[:12, :12] = 1                                  # present at every tap of the full size, gone at 4x6 of the coarse level
    pyramid.level_labels(small, small, (128, 192), 1, 1, oc)
    with pytest.raises(ValueError, match=r"region 1 of the content mask has no pixel at style layer 28 \(4x6 feature map\)"):
        pyramid.level_labels(small, small, (128, 192), 2, 1, oc)
    with pytest.raises(ValueError, match="one label map without the other"):
        pyramid.level_labels(content, None, (130, 150), 2, 1, oc)
    with pytest.raises(ValueError, match="one style image, got 2"):
        pyramid.level_labels(content, style, (130, 150), 2, 2, oc)


def test_renumbering_under_a_zero_weight():
    labels = torch.tensor([[0, 1, 2, 3], [3, 2, 1, 0], [255, 0, 2, 2]], dtype=torch.uint8)
    w = guidance.check_region_weights([1.0, 0.0, 0.5, 0.0], 4)
    assert guidance.active_regions(w) == (0, 2)
    got = guidance.renumber(labels, w)
    assert got.tolist() == [[0, 255, 1, 255], [255, 1, 255, 0], [255, 0, 1, 1]]
    assert guidance.renumber(labels, (1.0, 1.0, 1.0, 2.0)) is labels
    g = guidance.make_guide(4, [1.0, 0.0, 0.5, 0.0], labels, labels)
    assert g.n == 2 and g.weights == (1.0, 0.5) and g.active == (0, 2) and g.content_labels.tolist() == got.tolist()
    assert guidance.region_counts(got, 2) == [3, 4]
    assert guidance.make_guide(2, None, labels.clamp(max=1), labels.clamp(max=1)).weights == (1.0, 1.0)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------

def test_region_count_and_weight_refusals():
    for bad in (0, 5, -1, 2.0, True, None):
        with pytest.raises(ValueError, match=re.escape(repr(bad))):
            guidance.check_regions(bad)
    assert [guidance.check_regions(r) for r in (1, 2, 3, 4)] == [1, 2, 3, 4]
    with pytest.raises(ValueError, match="from 2 to 4, got 1"):
        guidance.check_regions(1, minimum=2, what="mask_regions")
    with pytest.raises(ValueError, match=r"3 entries for 2 regions: \[1.0, 2.0, 3.0\]"):
        guidance.check_region_weights([1, 2, 3], 2)
    with pytest.raises(ValueError, match=r">= 0, got \[1.0, -0.5\]"):
        guidance.check_region_weights([1, -0.5], 2)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            guidance.check_region_weights([1, bad], 2)
    with pytest.raises(ValueError, match=r"all zero \(\[0.0, 0.0\]\)"):
        guidance.check_region_weights([0, 0], 2)
    with pytest.raises(ValueError, match="hold region 2, but there are 2 regions"):
        guidance.check_labels(torch.tensor([[0, 2]], dtype=torch.uint8), 2)
    with pytest.raises(ValueError, match="uint8 tensor"):
        guidance.check_labels(torch.zeros(4, 4), 2)
    with pytest.raises(ValueError, match="5 style layers x 4 regions \\+ 50 other terms = 70 combine rows"):
        guidance.check_rows(5, 4, 50)
    guidance.check_rows(15, 4, 4)


def test_an_empty_region_at_a_tap_is_refused_with_region_layer_and_map_named(monkeypatch):
    labels = torch.zeros(64, 64, dtype=torch.uint8)
    labels[:3, :3] = 1                                   # gone at the 8x8 map of layer 19 (its pixel centres read row and column 4)
    maps = guidance.tap_maps(labels, [(64, 64), (32, 32), (16, 16), (8, 8), (4, 4)])
    with pytest.raises(ValueError, match=r"region 1 of the style mask has no pixel at style layer 19 \(8x8 feature map\)"):
        guidance.check_counts(maps, 2, "style", (0, 1), [0, 5, 10, 19, 28])
    monkeypatch.setattr(plan, "Program", RecordedProgram)
    ok = halves(64, 64)
    with pytest.raises(ValueError, match="region 1 of the content mask has no pixel at style layer 19"):
        core_model._Engine(_layers(), *DEFAULT_TAPS, 64, 64, torch.bfloat16, CPU, assume_device=True,
                           guide=guidance.make_guide(2, None, labels, ok))
    # a dropped region may be empty: weight 0, the small region (number 0 in that mask) is not looked at
    inv = 1 - labels
    eng = core_model._Engine(_layers(), *DEFAULT_TAPS, 64, 64, torch.bfloat16, CPU, assume_device=True,
                             guide=guidance.make_guide(2, [0.0, 1.0], inv, ok))
    assert eng.n_style_rows == 5
    # and the number named is the one in the mask, not the renumbered one
    with pytest.raises(ValueError, match="region 1 of the content mask"):
        core_model._Engine(_layers(), *DEFAULT_TAPS, 64, 64, torch.bfloat16, CPU, assume_device=True,
                           guide=guidance.make_guide(2, [0.0, 1.0], labels, ok))
    with pytest.raises(ValueError, match=r"content_labels are \(64, 64\), the image is \(32, 32\)"):
        core_model._Engine(_layers(), *DEFAULT_TAPS, 32, 32, torch.bfloat16, CPU, assume_device=True,
                           guide=guidance.make_guide(2, None, ok, ok))


@pytest.fixture
def tiny_vgg(monkeypatch):
    monkeypatch.setattr(core_model, "initialize_vgg", lambda: torch.nn.Sequential(*_layers()))


def test_model_refusals(tiny_vgg):
    lab = halves(64, 64)
    img = torch.zeros(1, 3, 64, 64)
    with pytest.raises(ValueError, match="from 1 to 4, got 5"):
        core_model.StyleContentModel(*DEFAULT_TAPS, guide_regions=5)
    with pytest.raises(ValueError, match="without guide_regions"):
        core_model.StyleContentModel(*DEFAULT_TAPS, region_weights=[1.0, 1.0])
    with pytest.raises(ValueError, match="3 entries for 2 regions"):
        core_model.StyleContentModel(*DEFAULT_TAPS, guide_regions=2, region_weights=[1, 1, 1])
    plain = core_model.StyleContentModel(*DEFAULT_TAPS)
    assert plain.guide_regions == 0 and plain.region_weights is None
    with pytest.raises(ValueError, match="content_labels given, but the model was built without guide_regions"):
        plain.set_targets(img, img, content_labels=lab)
    guided = core_model.StyleContentModel(*DEFAULT_TAPS, guide_regions=2)
    assert guided.region_weights == (1.0, 1.0)
    with pytest.raises(ValueError, match="needs content_labels and style_labels, got content_labels"):
        guided.set_targets(img, img, content_labels=lab)
    with pytest.raises(ValueError, match="got neither"):
        guided.set_targets(img, img)
    with pytest.raises(ValueError, match="one style image, got 2"):
        guided.set_targets([img, img], img, content_labels=lab, style_labels=lab)
    with pytest.raises(ValueError, match=r"style_labels are \(64, 64\), their image is \(32, 64\)"):
        guided.set_targets(torch.zeros(1, 3, 32, 64), img, content_labels=lab, style_labels=lab)
    with pytest.raises(ValueError, match="hold region 3"):
        guided.set_targets(img, img, content_labels=lab * 3, style_labels=lab)
    tiny = torch.zeros(64, 64, dtype=torch.uint8)
    tiny[:3, :3] = 1
    with pytest.raises(ValueError, match=r"region 1 of the style mask has no pixel at style layer 19 \(8x8 feature map\)"):
        guided.set_targets(img, img, content_labels=lab, style_labels=tiny)          # (before any engine exists)
    assert not guided._engines
    with pytest.raises(RuntimeError, match="guide_regions = 2"):          # the autograd path raises, whatever the image
        guided(img)
    with pytest.raises(RuntimeError, match="needs a guided model"):
        plain.last_region_losses()


def test_row_strips_refuse_guidance():
    for shard in (spatial.SpatialShard, spatial.HaloShard):
        with pytest.raises(ValueError, match="guide_regions = 2, masks.*row-strip"):
            shard(_layers(), *DEFAULT_TAPS, torch.zeros(1, 3, 64, 64), [], dtype=torch.float32, style_w=1.0, content_w=1.0,
                  guide_regions=2)
    with pytest.raises(ValueError, match="no row strips"):
        plan.Schedule(_layers(), *DEFAULT_TAPS, 32, 64, torch.float32, CPU, with_grad=True, halo=1, guide=2)


def _write_inputs(tmp_path, hw=(64, 64), mask_hw=None):
    H, W = hw
    paths = {}
    for name in ("content", "style"):
        Image.fromarray(np.full((H, W, 3), 128, dtype=np.uint8)).save(tmp_path / f"{name}.png")
        mh, mw = mask_hw or hw
        mask = np.zeros((mh, mw), dtype=np.uint8)
        mask[:, mw // 2:] = 255
        Image.fromarray(mask).save(tmp_path / f"{name}_mask.png")
        paths[name] = str(tmp_path / f"{name}.png")
        paths[name + "_mask"] = str(tmp_path / f"{name}_mask.png")
    return paths


def test_mask_loading_and_its_refusals(tmp_path):
    p = _write_inputs(tmp_path)
    oc = stv_config.StyleTransferConfig.model_validate({}).optimization
    both = InputPaths(p["content"], p["style"], content_mask_path=p["content_mask"], style_mask_path=p["style_mask"])
    c, s = stv_main._load_masks(both, oc)
    assert torch.equal(c, halves(64, 64)) and torch.equal(s, halves(64, 64))
    assert stv_main._load_masks(InputPaths(p["content"], p["style"]), oc) is None
    with pytest.raises(ValueError, match="go together: got content mask .*content_mask.png' and style mask None"):
        stv_main._load_masks(InputPaths(p["content"], p["style"], content_mask_path=p["content_mask"]), oc)
    with pytest.raises(ValueError, match="go together"):
        stv_main._load_masks(InputPaths(p["content"], p["style"], style_mask_path=p["style_mask"]), oc)
    with pytest.raises(ValueError, match="--style-also \\(1 further style images\\)"):
        stv_main._load_masks(InputPaths(p["content"], p["style"], (p["style"],), p["content_mask"], p["style_mask"]), oc)
    oc.region_weights = [0.0, 0.0]
    with pytest.raises(ValueError, match="all zero"):
        stv_main._load_masks(both, oc)
    oc.region_weights = None
    small = tmp_path / "small"
    small.mkdir()
    q = _write_inputs(small, mask_hw=(32, 48))
    with pytest.raises(ValueError, match="content mask .* is 48x32 pixels, its image is 64x64"):
        stv_main._load_masks(InputPaths(q["content"], q["style"], content_mask_path=q["content_mask"],
                                        style_mask_path=q["style_mask"]), oc)
    # the whole run refuses before it touches a device
    cfg = stv_config.StyleTransferConfig.model_validate({})
    cfg.hardware.device = "no-such-device"
    with pytest.raises(ValueError, match="go together"):
        stv_main.style_transfer(InputPaths(p["content"], p["style"], content_mask_path=p["content_mask"]), cfg)


def test_prepare_model_and_input_refuses_one_label_map(tiny_vgg):
    oc = stv_config.StyleTransferConfig.model_validate({}).optimization
    img = torch.zeros(1, 3, 64, 64)
    with pytest.raises(ValueError, match="one label map without the other"):
        core_model.prepare_model_and_input(img, img, CPU, oc, content_labels=halves(64, 64))
    with pytest.raises(ValueError, match="one style image, got 2"):
        core_model.prepare_model_and_input(img, [img, img], CPU, oc, content_labels=halves(64, 64), style_labels=halves(64, 64))


# ---- configuration and command line ------------------------------------------------------------------------------------------------

def test_config_and_cli_round_trip(tmp_path, caplog):
    from style_transfer_visualizer_amd import config_defaults
    assert (config_defaults.DEFAULT_MASK_REGIONS, config_defaults.DEFAULT_REGION_WEIGHTS) == (2, None)
    oc = stv_config.StyleTransferConfig.model_validate({}).optimization
    assert (oc.mask_regions, oc.region_weights) == (2, None)
    for bad in (1, 5):
        with pytest.raises(ValueError, match="mask_regions"):
            stv_config.StyleTransferConfig.model_validate({"optimization": {"mask_regions": bad}})
    toml = tmp_path / "config.toml"
    toml.write_text("[optimization]\nmask_regions = 3\nregion_weights = [1.0, 0.0, 2.5]\n")
    loaded = stv_config.ConfigLoader.load(str(toml))
    assert (loaded.optimization.mask_regions, loaded.optimization.region_weights) == (3, [1.0, 0.0, 2.5])
    parser = cli.build_arg_parser()
    args = parser.parse_args(["--content", "c.png", "--style", "s.png", "--content-mask", "cm.png", "--style-mask", "sm.png",
                              "--mask-regions", "4", "--region-weights", "1,0.5,0,2"])
    cfg = stv_config.build_config_from_cli(vars(args))
    assert (cfg.optimization.mask_regions, cfg.optimization.region_weights) == (4, [1.0, 0.5, 0.0, 2.0])
    over = stv_config.build_config_from_cli(vars(parser.parse_args(["--content", "c", "--style", "s", "--mask-regions", "2"])),
                                            base_config=loaded)
    assert (over.optimization.mask_regions, over.optimization.region_weights) == (2, [1.0, 0.0, 2.5])
    # (a command-line override is assigned, not validated: the run refuses it with the masks, before the first launch)
    one = stv_config.build_config_from_cli(vars(parser.parse_args(["--content", "c", "--style", "s", "--mask-regions", "1"])))
    with pytest.raises(ValueError, match="mask_regions must be an integer from 2 to 4, got 1"):
        stv_main._load_masks(InputPaths("c", "s", content_mask_path="cm", style_mask_path="sm"), one.optimization)
    plain = parser.parse_args(["--content", "c.png", "--style", "s.png"])
    assert not hasattr(plain, "content_mask") and not hasattr(plain, "mask_regions")
    paths = InputPaths("c.png", "s.png")
    assert (paths.content_mask_path, paths.style_mask_path) == (None, None)
    assert [f for f in InputPaths.__dataclass_fields__][-2:] == ["content_mask_path", "style_mask_path"]
    with caplog.at_level("INFO"):
        cli.log_parameters(InputPaths("c.png", "s.png", content_mask_path="cm.png", style_mask_path="sm.png"), cfg, args)
    text = caplog.text
    assert "Content mask: cm.png" in text and "Style mask: sm.png" in text and "Mask Regions: 4" in text
    assert "Region Weights: [1.0, 0.5, 0.0, 2.0]" in text
    caplog.clear()
    with caplog.at_level("INFO"):
        cli.log_parameters(paths, stv_config.StyleTransferConfig.model_validate({}), plain)
    assert "mask" not in caplog.text.lower() and "Region" not in caplog.text


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------

def test_library_exports_stv_mask_split_and_the_constants_match_the_header():
    lib = _lib.load()
    assert hasattr(lib, "stv_mask_split") and "stv_mask_split" in _lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "stv.h")).read()
    for name, value in (("STV_MASK_MAX_REGIONS", _lib.MASK_MAX_REGIONS), ("STV_MASK_SPLIT_THREADS", _lib.MASK_SPLIT_THREADS),
                        ("STV_MASK_SPLIT_MAX_BLOCKS", _lib.MASK_SPLIT_MAX_BLOCKS)):
        assert re.search(rf"#define {name} {value}\b", header), name
    assert guidance.MAX_REGIONS == _lib.MASK_MAX_REGIONS == 4
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    names = re.findall(r"STV_OP_[A-Z_0-9]+", body[body.index("STV_OP_CONV_FIRST_FWD = 1"):])
    assert names.index("STV_OP_MASK_SPLIT") + 1 == _lib.OP_MASK_SPLIT == _lib.OP_LAP + 1 == 19     # appended
    assert lib.stv_version() >= 112
    assert "guide.hip" in open(os.path.join(ROOT, "style_transfer_visualizer_amd", "csrc", "Makefile")).read()


def test_argument_refusals_run_without_a_gpu():
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    F, labels, out = base, base + 1024, base + 2048

    def call(F=F, labels=labels, out=out, n=4, C=8, R=2, dtype=_lib.STV_F32):
        return lib.stv_mask_split(F, labels, out, n, C, R, dtype, None)
    assert call(F=None) == call(labels=None) == call(out=None) == 1
    assert call(R=0) == call(R=5) == call(n=0) == call(C=0) == call(C=-3) == 1
    assert call(dtype=_lib.STV_BF16X3) == call(dtype=7) == 1
    assert call(n=1 << 28, C=2) == 1 and call(n=1 << 29, C=1, dtype=_lib.STV_BF16) == 1       # a slab of 2 GiB
    assert call(n=1 << 31, C=1) == 1
    assert call(out=F) == call(out=F + 64) == 1                    # out overlapping F (4 * 8 * 4 = 128 bytes)
    assert call(out=F - 128) == 1                                  # the second slab is F
    assert call(out=labels - 255) == 1 and call(out=labels + 3) == 1    # out overlapping labels


# ---- the guided step --------------------------------------------------------------------------------------------------------------

def guided_engine(monkeypatch, dtype, weights=None, R=2, labels=None, **env):
    for name in ("STV_LOSS_BATCH", "STV_GRAM_FIN_LATE", "STV_LOSS_INTERLEAVE", "STV_FUSE_CONTENT"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    monkeypatch.setattr(plan, "Program", RecordedProgram)
    labels = halves(64, 64) if labels is None else labels
    eng = core_model._Engine(_layers(), *DEFAULT_TAPS, 64, 64, dtype, CPU, assume_device=True,
                             guide=guidance.make_guide(R, weights, labels, labels))
    for tap in eng.sched.all_chains():
        tap.target = torch.zeros(tap.buf.C, tap.buf.C)
    for tap in eng.sched.content_taps:
        tap.target = torch.empty_like(tap.buf.act)
    return eng


def guided_step(eng, x, grad, **kw):
    eng.loss_and_grad(x, grad, 1e5, 1.0, **kw)
    (prog,) = [p for key, p in eng._programs.items() if key[0] == "fused"]
    return prog.op_list


def test_guidance_off_is_the_step_and_the_key_of_a_model_without_the_option(monkeypatch, tiny_vgg):
    x, grad = _image(64, 64, "x"), _image(64, 64, "x.grad")
    a = host_engine(monkeypatch, torch.bfloat16, 64, 64, *DEFAULT_TAPS)
    want = step_signature(fused_step(a, x, grad))
    (key,) = [k for k in a._programs if k[0] == "fused"]
    assert key[-1] is None and not any(isinstance(e, tuple) and e and e[0] == "guide" for e in key)
    kinds = [sig[0] for sig in want]
    assert _lib.OP_MASK_SPLIT not in kinds
    assert a.guide is None and a.n_style_rows == a.n_style == 5 and a.sched.guide == 0
    monkeypatch.setattr(plan, "Program", RecordedProgram)
    off = core_model._Engine(_layers(), *DEFAULT_TAPS, 64, 64, torch.bfloat16, CPU, assume_device=True, guide=None)
    for tap in off.sched.style_taps:
        tap.target = torch.zeros(tap.buf.C, tap.buf.C)
    for tap in off.sched.content_taps:
        tap.target = torch.empty_like(tap.buf.act)
    assert step_signature(fused_step(off, x, grad)) == want and list(off._programs) == list(a._programs)
    assert all(t.regions is None and t.slabs is None and t.labels is None and t.norm is None for t in a.sched.style_taps)
    # ... and the model hands its engine no guidance keyword at all
    seen = {}
    real = core_model._Engine

    def spy(*args, **kw):
        seen.update(kw)
        return real(*args, assume_device=True, **kw)
    monkeypatch.setattr(core_model, "_Engine", spy)
    monkeypatch.setattr(plan, "Program", RecordedProgram)
    model = core_model.StyleContentModel(*DEFAULT_TAPS, precision="bf16")
    monkeypatch.setattr(model, "_engine_for", lambda img: spy(_layers(), *DEFAULT_TAPS, 64, 64, torch.bfloat16, CPU,
                                                           **({"guide": model._guide} if model._guide is not None else {})))
    model._check_guidance([x], x, None, None)
    assert model._guide is None and "guide" not in seen


def test_the_guided_step_of_two_regions(monkeypatch):
    x, grad = _image(64, 64, "x"), _image(64, 64, "x.grad")
    eng = guided_engine(monkeypatch, torch.bfloat16)
    s = eng.sched
    op_list = guided_step(eng, x, grad)
    kinds = [o.op for o in op_list]
    # 5 MASK_SPLIT ops, each directly behind its tap's producer
    splits = [i for i, k in enumerate(kinds) if k == _lib.OP_MASK_SPLIT]
    assert len(splits) == 5
    for i, tap in zip(splits, s.style_taps, strict=True):
        o, producer = op_list[i], op_list[i - 1]
        assert producer.op in (_lib.OP_CONV_FIRST_FWD, _lib.OP_CONV) and producer.q0 == tap.buf.act.data_ptr()
        assert (o.p0, o.p1, o.q0) == (tap.buf.act.data_ptr(), tap.labels.data_ptr(), tap.slabs.data_ptr())
        assert (o.n, o.cin, o.cout, o.dtype) == (tap.buf.H * tap.buf.W, tap.buf.C, 2, _lib.STV_BF16)
        assert tap.slabs.shape == (2, tap.buf.H, tap.buf.W, tap.buf.C) and tap.labels.dtype == torch.uint8
    # the two fusions that assume one Gram per tap are off; the others stand
    assert not any(o.op == _lib.OP_CONV and o.q2 and o.q3 for o in op_list)
    first = op_list[0]
    assert first.op == _lib.OP_CONV_FIRST_FWD and not first.q1
    assert not any(t.partials_fused for t in s.style_taps) and all(nd.gram is None for nd in s.nodes)
    plain = host_engine(monkeypatch, torch.bfloat16, 64, 64, *DEFAULT_TAPS)
    assert [(nd.fused, nd.route is not None, nd.dst.stored) for nd in s.nodes] == [
        (nd.fused, nd.route is not None, nd.dst.stored) for nd in plain.sched.nodes]
    assert s.grad_arena == plain.sched.grad_arena and [t.grad_fused for t in s.content_taps] == [True]
    # 10 products with taps == 1: slab r times seed r, ACCUM on every one but the first writer of a buffer
    products = [o for o in op_list if o.op == _lib.OP_CONV and o.taps == 1]
    assert len(products) == 10
    chains = list(reversed(s.style_taps))
    seen_out: set[int] = set()
    for k, o in enumerate(products):
        tap = chains[k // 2]
        c = tap.regions[k % 2]
        assert (o.p0, o.p1, o.q0) == (c.buf.act.data_ptr(), c.sgrad.data_ptr(), tap.buf.grad.data_ptr())
        assert c.buf.act.data_ptr() == tap.slabs[k % 2].data_ptr()
        first_writer = k % 2 == 0 and tap is chains[0]          # only the deepest tap's buffer has no writer in front
        assert bool(o.flags & _lib.ACCUM) == (not first_writer), k
        seen_out.add(o.q0)
    # the batched launches take at most 8 entries: 10 chains, two launches, norm = C * n_{l,r}
    multis = [o for o in op_list if o.op == _lib.OP_GRAM_MULTI]
    assert [o.n for o in multis] == [8, 2]
    entries = [e for o in multis for e in o.refs["p0"]]
    for e, c in zip(entries, s.all_chains(), strict=True):
        n = c.buf.H * c.buf.W
        assert (e.F, e.n_pixels, e.channels) == (c.buf.act.data_ptr(), n, c.buf.C)
        assert e.norm == float(c.buf.C * n // 2) == c.norm and e.sgrad == c.sgrad.data_ptr()
        assert e.coef == np.float32(1e5)
    # the combine table: 10 style rows in layer then region order, then the content row
    assert eng.table.shape == (11, 3) and eng.table[:10, 2].tolist() == [0] * 10 and int(eng.table[10, 2]) == 1
    assert [c.order for c in s.all_chains()] == list(range(10))
    for row, sc, c in zip(eng.table[:10], eng.scale[:10], s.all_chains(), strict=True):
        assert row.tolist() == [c.parts_off, c.parts_cnt, 0]
        assert float(sc) == float(np.float32(1.0 / (c.buf.C * c.buf.C)))
    combine = next(o for o in op_list if o.op == _lib.OP_LOSS_COMBINE)
    assert combine.cin == 11
    with pytest.raises(RuntimeError, match="no guided form"):
        eng.forward_losses(x)
    # the key carries the guidance
    (key,) = [k for k in eng._programs if k[0] == "fused"]
    assert key[-1][:3] == ("guide", 2, (1.0, 1.0)) and len(key[-1]) == 5


def test_scales_and_seed_coefficients_with_region_and_layer_weights(monkeypatch):
    x, grad = _image(64, 64, "x"), _image(64, 64, "x.grad")
    eng = guided_engine(monkeypatch, torch.float32, weights=[1.0, 0.25])
    layer_w = (1.0, 0.5, 2.0, 1.0, 0.2)
    op_list = guided_step(eng, x, grad, layer_w=layer_w, tv_w=3.0)
    combine = next(o for o in op_list if o.op == _lib.OP_LOSS_COMBINE)
    assert combine.cin == 12
    table, scale = combine.refs["p1"], combine.refs["p2"]
    assert table[:, 2].tolist() == [0] * 10 + [1, 2]
    finishes = [e for o in op_list if o.op == _lib.OP_GRAM_MULTI for e in o.refs["p0"]]
    for c, e in zip(eng.sched.all_chains(), finishes, strict=True):
        l, r = divmod(c.order, 2)
        lam = (1.0, 0.25)[r]
        assert float(scale[c.order]) == float(np.float32(layer_w[l] * lam / (c.buf.C * c.buf.C)))
        assert e.coef == np.float32(1e5 * layer_w[l] * lam)


def test_a_zero_weight_leaves_no_copy_no_chain_and_no_row(monkeypatch):
    x, grad = _image(64, 64, "x"), _image(64, 64, "x.grad")
    eng = guided_engine(monkeypatch, torch.bfloat16, weights=[1.0, 0.0])
    op_list = guided_step(eng, x, grad)
    assert eng.guide.n == 1 and eng.guide.active == (0,) and eng.n_style_rows == 5 and eng.table.shape == (6, 3)
    assert sum(1 for o in op_list if o.op == _lib.OP_CONV and o.taps == 1) == 5
    assert all(o.cout == 1 for o in op_list if o.op == _lib.OP_MASK_SPLIT)
    assert all(t.slabs.shape[0] == 1 and len(t.regions) == 1 for t in eng.sched.style_taps)
    assert [o.n for o in op_list if o.op == _lib.OP_GRAM_MULTI] == [5]
    assert int((eng.guide.content_labels == guidance.NO_REGION).sum()) == 64 * 32


@pytest.mark.parametrize("env", [{}, {"STV_LOSS_BATCH": "0"}, {"STV_LOSS_INTERLEAVE": "0"}], ids=["batched", "unbatched", "tail"])
def test_region_chains_take_the_placement_of_their_tap(monkeypatch, env):
    x, grad = _image(64, 64, "x"), _image(64, 64, "x.grad")
    eng = guided_engine(monkeypatch, torch.bfloat16, R=4, labels=halves(64, 64) + 2 * halves(64, 64).t(), **env)
    op_list = guided_step(eng, x, grad)
    kinds = [o.op for o in op_list]
    assert kinds.count(_lib.OP_MASK_SPLIT) == 5 and sum(1 for o in op_list if o.op == _lib.OP_CONV and o.taps == 1) == 20
    assert eng.table.shape == (21, 3)
    if env.get("STV_LOSS_BATCH") == "0":
        assert kinds.count(_lib.OP_GRAM_MULTI) == 0 and kinds.count(_lib.OP_GRAM_PARTIAL) == kinds.count(_lib.OP_GRAM_FINISH) == 20
        i = kinds.index(_lib.OP_MASK_SPLIT)
        assert kinds[i + 1:i + 9] == [_lib.OP_GRAM_PARTIAL, _lib.OP_GRAM_FINISH] * 4
        assert op_list[i + 2].f1 == float(64 * 64 * 64 // 4)
    else:
        assert [o.n for o in op_list if o.op == _lib.OP_GRAM_MULTI] == [8, 8, 4]
        if env.get("STV_LOSS_INTERLEAVE") == "0":
            last_fwd = max(i for i, o in enumerate(op_list) if o.op == _lib.OP_CONV and o.taps == 9 and i < kinds.index(_lib.OP_LOSS_COMBINE))
            assert min(i for i, k in enumerate(kinds) if k == _lib.OP_MASK_SPLIT) > last_fwd
    # built twice: the same op list, pointers included
    del eng._programs[next(iter(eng._programs))]
    assert step_signature(guided_step(eng, x, grad), canonical=False) == step_signature(op_list, canonical=False)
