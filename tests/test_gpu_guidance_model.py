"""Spatial guidance through the whole step on a real MI355X (64x64 and 48x80, the synthetic VGG19 of the fixture-size tests).

* ``guide_regions=1`` with all-zero labels IS the unguided step with its two one-Gram-per-tap fusions off, bit for bit: the whole
  guided plumbing (split, per-region chains, batched launches, 1x1 products, combine rows) held to arithmetic that is already
  verified, with no tolerance.
* ``R = 2`` and ``R = 4``: every slab equals the ``torch.where`` twin of the stored activation; every (layer, region)'s loss
  partials and seed equal what the direct entry points give on that slab with ``norm = C * n_{l,r}``; the region losses and the
  style score follow from the partials in the combine's order.  No tolerance either.
* Weights ``(1, 0)`` equal a run whose content labels carry 255 in place of region 1, bit for bit.
* Graph replay equals eager launches; guidance on, then off on the same model restores the unguided bits.
* A sign check that the guidance guides: under a swapped style label map the per-region losses of an image rise.
"""
from __future__ import annotations

import math

import pytest
import torch

from style_transfer_visualizer_amd import core_model, guidance, ops, synthetic
from tests.conftest import GoldenCase

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SIZES = [(64, 64), (48, 80)]
PRECISIONS = ["fp32", "bf16", "bf16x3"]
UNFUSED = {"STV_FUSE_GRAM": "0", "STV_FUSE_GRAM_FIRST": "0"}
STORE_ALL = {"STV_GRAD_ARENA": "0", "STV_SKIP_PREPOOL": "0"}


def halves(H, W):
    lab = torch.zeros(H, W, dtype=torch.uint8)
    lab[:, W // 2:] = 1
    return lab


def quadrants(H, W):
    lab = halves(H, W)
    lab[H // 2:] += 2
    return lab


def diagonal(H, W):
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return (x * H > y * W).to(torch.uint8)


def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _model(monkeypatch, precision, hw, *, regions=0, weights=None, labels=None, style_labels=None, style_hw=None, env=None,
           layer_weights=None):
    """Model with targets set, an image with ``requires_grad``, and the fixture's two loss weights.  ``env`` holds only while
    the engine is built (the switches are read then)."""
    case = GoldenCase("vgg19_white_lbfgs")
    m = case.meta
    w = case.weights()
    monkeypatch.setattr(core_model, "initialize_vgg", lambda: core_model.build_vgg_features(w, case.cfg).eval())
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    H, W = hw
    kw = {"guide_regions": regions, "region_weights": weights} if regions else {}
    if layer_weights is not None:
        kw["style_layer_weights"] = layer_weights
    model = core_model.StyleContentModel(list(m["style_layers"]), list(m["content_layers"]), precision=precision, **kw).to(DEV)
    style = synthetic.synthetic_image(1, *(style_hw or hw)).to(DEV)
    lab = {"content_labels": labels, "style_labels": labels if style_labels is None else style_labels} if regions else {}
    model.set_targets(style, synthetic.synthetic_image(0, H, W).to(DEV), **lab)
    x = synthetic.synthetic_image(2, H, W) + 0.25 * torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(5))
    x = x.to(DEV).requires_grad_(True)
    out = model.loss_and_grad(x, float(m["style_w"]), float(m["content_w"]))      # (builds the step under `env`)
    torch.cuda.synchronize()
    for k in (env or {}):
        monkeypatch.delenv(k)
    return model, x, float(m["style_w"]), float(m["content_w"]), out


def _engine(model, hw):
    (eng,) = [e for key, e in model._engines.items() if key[:2] == tuple(hw)]
    return eng


# ---- R = 1 is the unguided step ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_region_is_the_unguided_step_bit_for_bit(precision, hw, monkeypatch):
    plain, xp, sw, cw, (s0, c0, t0) = _model(monkeypatch, precision, hw, env=UNFUSED)
    g0 = xp.grad.clone()
    guided, xg, _, _, (s1, c1, t1) = _model(monkeypatch, precision, hw, regions=1, labels=torch.zeros(hw, dtype=torch.uint8))
    assert torch.equal(xp, xg)
    assert float(s0) > 0 and math.isfinite(float(t0)) and float(g0.abs().max()) > 0
    for tp, tg in zip(plain.style_targets, guided.style_targets, strict=True):
        assert tg.shape == (1, *tp.shape) and torch.equal(tg[0], tp), "captured style target"
    assert torch.equal(s1, s0), f"style score {float(s1)!r} against {float(s0)!r}"
    assert torch.equal(c1, c0) and torch.equal(t1, t0)
    assert torch.equal(xg.grad, g0), f"max |diff| {float((xg.grad - g0).abs().max()):.3e}"
    losses = guided.last_region_losses()
    assert losses.shape == (5, 1)
    with pytest.raises(RuntimeError, match="guide_regions"):
        guided(xg)


# ---- R = 2, R = 4: per-op composition -----------------------------------------------------------------------------------------

CASES = [((64, 64), 2, halves), ((64, 64), 4, quadrants), ((48, 80), 2, diagonal)]


@pytest.mark.parametrize("hw,R,make", CASES, ids=["64x64-halves", "64x64-quadrants", "48x80-diagonal"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_region_chain_equals_the_direct_entry_points(precision, hw, R, make, monkeypatch):
    labels = make(*hw)
    weights = [1.0, 0.5, 2.0, 0.25][:R]
    model, x, sw, cw, (style, content, total) = _model(monkeypatch, precision, hw, regions=R, weights=weights, labels=labels,
                                                       env=STORE_ALL)
    eng = _engine(model, hw)
    split = precision == "bf16x3"
    region_losses = model.last_region_losses().clone()
    assert region_losses.shape == (5, R)
    want_style = torch.zeros((), dtype=torch.float32)
    for l, tap in enumerate(eng.sched.style_taps):
        b = tap.buf
        n, C = b.H * b.W, b.C
        lab = guidance.resample_labels(labels, b.H, b.W)
        assert torch.equal(tap.labels.cpu(), lab)
        counts = guidance.region_counts(lab, R)
        if l == 4:      # conv5_1: 4x4, respectively 3x5 pixels
            assert sorted(counts) == {halves: [8, 8], quadrants: [4, 4, 4, 4], diagonal: [7, 8]}[make]
        fbits = _bits(b.act).reshape(n, C)
        lab_dev = lab.reshape(-1).to(DEV)
        for r, c in enumerate(tap.regions):
            twin = torch.where((lab_dev == r).unsqueeze(1), fbits, torch.zeros_like(fbits))
            assert torch.equal(_bits(tap.slabs[r]).reshape(n, C), twin), f"slab of layer {l}, region {r}"
            assert c.norm == float(C * counts[r])
            parts = ops.gram_partial(tap.slabs[r], split=split)
            cnt = ops.gram_loss_parts(C)
            loss_part = torch.full((cnt,), float("nan"), device=DEV)
            seed = torch.full((1, C, C), float("nan"), device=DEV, dtype=eng.dtype)
            ops.gram_finish(parts, n, C, target=model.style_targets[l][r], loss_part=loss_part, sgrad=seed,
                            coef=sw * 1.0 * weights[r], dtype=eng.dtype, norm=float(C * counts[r]))
            got = eng.parts[c.parts_off:c.parts_off + c.parts_cnt]
            assert c.parts_cnt == cnt and torch.equal(got, loss_part), f"loss partials of layer {l}, region {r}"
            assert torch.equal(_bits(c.sgrad), _bits(seed)), f"seed of layer {l}, region {r}"
            assert float(seed.float().abs().max()) > 0
            # the combine's order: the partials added in double, one rounding to fp32 with the row's scale, then the rows
            # added one by one in fp32
            tot = got.double().sum()
            unweighted = (tot * torch.tensor(1.0 / float(C * C), dtype=torch.float32).double()).float()
            assert torch.equal(region_losses[l, r].cpu(), unweighted.cpu()), f"region loss of layer {l}, region {r}"
            scale = torch.tensor(1.0 * weights[r] / float(C * C), dtype=torch.float64).float()
            assert torch.equal(eng.scale[c.order].cpu(), scale)
            want_style = want_style + (tot * scale.double()).float().cpu()
    assert torch.equal(style.cpu(), want_style), f"style score {float(style)!r} against {float(want_style)!r}"
    assert math.isfinite(float(total)) and float(total) > float(content)


# ---- a region of weight 0 is a region nobody is in -------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_a_zero_weight_equals_labels_without_the_region(precision, monkeypatch):
    hw = (48, 80)
    labels = diagonal(*hw)
    # (the style map keeps both regions: a dropped region needs no counterpart there)
    a, xa, _, _, out_a = _model(monkeypatch, precision, hw, regions=2, weights=[1.0, 0.0], labels=labels)
    erased = labels.clone()
    erased[labels == 1] = guidance.NO_REGION
    b, xb, _, _, out_b = _model(monkeypatch, precision, hw, regions=2, weights=[1.0, 0.0], labels=erased, style_labels=labels)
    c, xc, _, _, out_c = _model(monkeypatch, precision, hw, regions=1, labels=erased,
                                style_labels=guidance.renumber(labels, (1.0, 0.0)))
    assert a.last_region_losses().shape == (5, 1)
    for other, x_other, out in ((b, xb, out_b), (c, xc, out_c)):
        assert all(torch.equal(p, q) for p, q in zip(out_a, out, strict=True))
        assert torch.equal(xa.grad, x_other.grad)
        assert torch.equal(a.last_region_losses(), other.last_region_losses())
    both, xboth, _, _, out_both = _model(monkeypatch, precision, hw, regions=2, labels=labels)
    assert not torch.equal(out_both[0], out_a[0]) and not torch.equal(xboth.grad, xa.grad)


# ---- one program, one graph; on and off --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_graph_replay_equals_eager_and_off_restores_the_unguided_bits(precision, monkeypatch):
    hw = (48, 80)
    labels = diagonal(*hw)
    model, x, sw, cw, first = _model(monkeypatch, precision, hw, regions=2, weights=[1.0, 0.25], labels=labels)
    g_first = x.grad.clone()
    for _ in range(2):                                  # the captured graph, replayed
        again = model.loss_and_grad(x, sw, cw)
        assert all(torch.equal(p, q) for p, q in zip(first, again, strict=True)) and torch.equal(x.grad, g_first)
    eager, xe, _, _, out_e = _model(monkeypatch, precision, hw, regions=2, weights=[1.0, 0.25], labels=labels,
                                    env={"STV_HIP_GRAPH": "0"})
    assert not _engine(eager, hw).use_graph and _engine(model, hw).use_graph
    assert all(torch.equal(p, q) for p, q in zip(first, out_e, strict=True)) and torch.equal(xe.grad, g_first)
    # with tv_w the guided step is still one program: the TV term joins the total only
    s_tv, c_tv, t_tv = model.loss_and_grad(x, sw, cw, tv_w=50.0)
    assert torch.equal(s_tv, first[0]) and torch.equal(c_tv, first[1]) and float(t_tv) > float(first[2])
    # off on the same model: the unguided bits of a model that never was guided
    plain, xp, _, _, out_p = _model(monkeypatch, precision, hw)
    model.set_guidance(0)
    assert model.style_targets is None
    model.set_targets(synthetic.synthetic_image(1, *hw).to(DEV), synthetic.synthetic_image(0, *hw).to(DEV))
    out_off = model.loss_and_grad(x, sw, cw)
    assert all(torch.equal(p, q) for p, q in zip(out_p, out_off, strict=True)) and torch.equal(x.grad, xp.grad)
    assert not torch.equal(out_off[0], first[0])
    # ... and on again
    model.set_guidance(2, [1.0, 0.25])
    model.set_targets(synthetic.synthetic_image(1, *hw).to(DEV), synthetic.synthetic_image(0, *hw).to(DEV), content_labels=labels,
                      style_labels=labels)
    out_on = model.loss_and_grad(x, sw, cw)
    assert all(torch.equal(p, q) for p, q in zip(first, out_on, strict=True)) and torch.equal(x.grad, g_first)


# ---- the guidance guides -------------------------------------------------------------------------------------------------------------

def test_swapping_the_style_label_map_raises_the_region_losses(monkeypatch):
    """A style picture of two different textures, left and right.  An image that IS that picture has (near) zero region losses
    under the style's own label map; under the swapped map every region is asked for the other texture, and its losses rise."""
    hw = (64, 64)
    case = GoldenCase("vgg19_white_lbfgs")
    m = case.meta
    w = case.weights()
    monkeypatch.setattr(core_model, "initialize_vgg", lambda: core_model.build_vgg_features(w, case.cfg).eval())
    g = torch.Generator().manual_seed(3)
    fine = 0.5 + 0.3 * torch.randn(1, 3, 64, 32, generator=g)                                      # pixel noise
    coarse = (0.5 + 0.3 * torch.randn(1, 3, 8, 4, generator=g)).repeat_interleave(8, 2).repeat_interleave(8, 3)   # 8x8 blocks
    style = torch.cat([fine, coarse], dim=3).to(DEV)
    labels = halves(*hw)
    swapped = 1 - labels
    model = core_model.StyleContentModel(list(m["style_layers"]), list(m["content_layers"]), precision="fp32", guide_regions=2).to(DEV)
    x = style.clone().requires_grad_(True)
    losses = {}
    for name, style_labels in (("own", labels), ("swapped", swapped)):
        model.set_targets(style, style, content_labels=labels, style_labels=style_labels)
        model.loss_and_grad(x, 1.0, 1.0)
        losses[name] = model.last_region_losses().clone().cpu()
    print("region losses under the style's own map:", losses["own"].tolist(), "under the swapped map:", losses["swapped"].tolist())
    assert bool((losses["swapped"] > losses["own"]).all())


# ---- against the float64 definition ------------------------------------------------------------------------------------------------

def _reference(case, precision_model, x, labels, style_labels, style_img, content_img, regions, **weights):
    """The float64 definition (tests/guidance_ref.py) at ``x`` on the branch the HIP path took: its ReLU and pool decisions are
    imposed on the oracle (tests/parity_util.py), as tests/test_gpu_model.py does where decisions differ."""
    from oracle import core_model_ref as ocm
    from tests import guidance_ref as gref
    from tests import parity_util as pu
    m = case.meta
    prog64 = ocm.vgg_program([(w.double(), b.double()) for w, b in case.weights()], case.cfg)
    oracle = ocm.OracleModel(prog64, m["style_layers"], m["content_layers"])
    oracle.set_targets(style_img.double(), content_img.double())
    targets = gref.guided_targets(oracle, style_img.double(), style_labels, regions)
    locked = pu.lock(oracle, pu.hip_decisions(precision_model))
    return gref.loss_and_grad(locked, x.detach().cpu().double(), labels, targets, float(m["style_w"]), float(m["content_w"]), **weights)


FLOAT64_CASES = [((64, 64), (80, 64), halves, diagonal), ((48, 80), (64, 96), diagonal, halves)]


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("hw,style_hw,make,make_style", FLOAT64_CASES, ids=["64x64", "48x80"])
def test_fp32_step_against_the_float64_definition(hw, style_hw, make, make_style, weighted, monkeypatch):
    """Bounds: the ones tests/test_gpu_model.py holds the unguided fp32 step to - scores relative 2e-4, gradient 2e-4 of its
    maximum.  The style image has another size and another label map than the content."""
    from tests.conftest import record_parity
    case = GoldenCase("vgg19_white_lbfgs")
    labels, style_labels = make(*hw), make_style(*style_hw)
    region_w = [1.0, 0.25] if weighted else None
    layer_w = [1.0, 0.5, 2.0, 1.0, 0.25] if weighted else None
    model, x, sw, cw, (style, content, total) = _model(monkeypatch, "fp32", hw, regions=2, weights=region_w, labels=labels,
                                                       style_labels=style_labels, style_hw=style_hw, layer_weights=layer_w,
                                                       env={"STV_SKIP_PREPOOL": "0"})
    kw = {"region_w": region_w, "layer_w": layer_w} if weighted else {}
    losses_ref, s_ref, c_ref, t_ref, g_ref = _reference(case, model, x, labels, style_labels, synthetic.synthetic_image(1, *style_hw),
                                                        synthetic.synthetic_image(0, *hw), 2, **kw)
    name = f"guided fp32 {hw[0]}x{hw[1]} R=2" + (" weighted" if weighted else "")
    for what, got, ref in (("style score", style, s_ref), ("content score", content, c_ref), ("total", total, t_ref)):
        dev = abs(float(got) - float(ref)) / abs(float(ref))
        print(f"{name}: {what} {float(got)!r} against {float(ref)!r}: relative {dev:.3e}")
        record_parity(name, f"{what} vs float64 definition (rel)", dev, 2e-4)
        assert dev <= 2e-4, what
    region = model.last_region_losses().cpu().double()
    dev = float(((region - losses_ref).abs() / losses_ref.abs()).max())
    print(f"{name}: region losses, largest relative deviation {dev:.3e}")
    record_parity(name, "region losses vs float64 definition (rel, max)", dev, 2e-4)
    assert dev <= 2e-4
    gdev = float((x.grad.cpu().double() - g_ref).abs().max() / g_ref.abs().max())
    print(f"{name}: gradient, largest deviation {gdev:.3e} of its maximum")
    record_parity(name, "gradient vs float64 definition on the HIP path's branch (of scale)", gdev, 2e-4)
    assert gdev <= 2e-4


# ---- end to end ----------------------------------------------------------------------------------------------------------------------

CLI_VARIANTS = {
    "pyramid": ["--pyramid-levels", "2", "--steps", "8"],
    "content_size": ["--content-size", "96", "--steps", "6", "--region-weights", "1,0.5"],
    "lap_tv_multi_iter": ["--lap-w", "100", "--tv-w", "10", "--steps", "4"],
}


@pytest.mark.parametrize("variant", list(CLI_VARIANTS))
def test_cli_with_two_masks(variant, tmp_path, monkeypatch):
    import csv

    import numpy as np
    from PIL import Image

    from style_transfer_visualizer_amd import cli
    monkeypatch.setenv("STV_SYNTHETIC_WEIGHTS", "0")
    for name, seed in (("content", 0), ("style", 1)):
        img = synthetic.synthetic_image(seed, 128, 128, normalize=False)[0].permute(1, 2, 0).mul(255).byte().numpy()
        Image.fromarray(img).save(tmp_path / f"{name}.png")
    Image.fromarray((halves(128, 128) * 255).numpy()).save(tmp_path / "content_mask.png")
    Image.fromarray((halves(128, 128).t().contiguous() * 255).numpy()).save(tmp_path / "style_mask.png")      # top / bottom
    out_dir, log = tmp_path / "out", tmp_path / "loss.csv"
    argv = ["--content", str(tmp_path / "content.png"), "--style", str(tmp_path / "style.png"),
            "--content-mask", str(tmp_path / "content_mask.png"), "--style-mask", str(tmp_path / "style_mask.png"),
            "--init-method", "content", "--device", "cuda", "--no-video", "--final-only", "--seed", "0", "--no-plot",
            "--log-loss", str(log), "--log-every", "1", "--output", str(out_dir), *CLI_VARIANTS[variant]]
    if variant == "lap_tv_multi_iter":
        cfg = tmp_path / "config.toml"
        cfg.write_text("[optimization]\nlbfgs_max_iter = 3\nlbfgs_max_eval = 4\nmask_regions = 2\n")
        argv += ["--config", str(cfg)]
    cli.main(argv)
    (png,) = list(out_dir.glob("stylized_*.png"))
    assert Image.open(png).size == ((96, 96) if variant == "content_size" else (128, 128))
    with log.open() as fh:
        rows = list(csv.reader(fh))
    from style_transfer_visualizer_amd.pyramid import HEADER
    assert rows[0] == list(HEADER)
    total = [float(r[rows[0].index("total_loss")]) for r in rows[1:]]
    steps = int(CLI_VARIANTS[variant][CLI_VARIANTS[variant].index("--steps") + 1])
    assert len(total) == steps and all(math.isfinite(v) for v in total)
    if variant == "pyramid":                      # every level is a run of its own: decreasing inside a level
        assert total[3] < total[0] and total[7] < total[4]
    else:
        assert total[-1] < total[0]
    print(f"cli {variant}: total loss {total[0]:.6g} -> {total[-1]:.6g}")


class _Bar:
    def update(self, n=1):
        return None

    def set_postfix(self, *a, **k):
        return None

    def close(self):
        return None


def test_adam_steps_on_a_guided_model_lower_the_objective(monkeypatch):
    """``prepare_model_and_input`` with the two label maps, then five Adam steps through the runner."""
    from style_transfer_visualizer_amd import config as stv_config
    from style_transfer_visualizer_amd import optimization
    from style_transfer_visualizer_amd.optimizers import HipAdam
    case = GoldenCase("vgg19_white_lbfgs")
    m = case.meta
    w = case.weights()
    monkeypatch.setattr(core_model, "initialize_vgg", lambda: core_model.build_vgg_features(w, case.cfg).eval())
    cfg = stv_config.StyleTransferConfig.model_validate({})
    oc = cfg.optimization
    oc.steps, oc.style_w, oc.content_w, oc.init_method = 5, m["style_w"], m["content_w"], "content"
    oc.style_layers, oc.content_layers, oc.normalize = list(m["style_layers"]), list(m["content_layers"]), m["normalize"]
    oc.mask_regions, oc.region_weights = 2, [1.0, 0.5]
    cfg.hardware.precision, cfg.video.create_video = "fp32", False
    hw = (48, 80)
    content, style = synthetic.synthetic_image(0, *hw).to(DEV), synthetic.synthetic_image(1, *hw).to(DEV)
    model, x, _ = core_model.prepare_model_and_input(content, style, DEV, oc, precision="fp32", content_labels=diagonal(*hw),
                                                     style_labels=halves(*hw))
    assert model.guide_regions == 2 and model.region_weights == (1.0, 0.5) and model.style_targets[0].shape[0] == 2
    runner = optimization.OptimizationRunner(model, x, cfg, optimizer=HipAdam([x], lr=1e-2), progress_bar=_Bar())
    _, hist, _ = runner.run()
    torch.cuda.synchronize()
    assert all(len(v) == 5 for v in hist.values()) and all(math.isfinite(v) for vs in hist.values() for v in vs)
    assert hist["total_loss"][-1] < hist["total_loss"][0]
    assert model.last_region_losses().shape == (5, 2)
