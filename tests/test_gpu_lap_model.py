"""The Laplacian loss on real operands and through the whole step (64x64 and 48x80, the synthetic VGG19 of the fixture-size
tests): stv_lap against the NumPy fp32 twin on random normal images bit for bit, ``loss_and_grad(..., lap_w=)`` against
``lap_w=0`` on the same image bit for bit (alone and together with ``tv_w``), graph replay against eager launches,
multi-iteration L-BFGS, Adam, and the CLI with a pyramid.

Bounds (derived, u = 2^-24, nothing measured went into them):

* target, residual, gradient: none - they equal the fp32 twin (tests/lap_ref.py), whose distance from float64 the host tests
  bound;
* raw loss sum against the float64 sum of the twin's r^2, relative (all terms are non-negative, so the relative error of a sum
  is at most the longest chain of roundings any term goes through): the square, one add per tile of the workgroup's stride
  loop, 6 levels of the wave butterfly, 2 levels over the four waves; the partials are added in float64.
  ``gamma(lap_ref.partial_sum_depth(...))``;
* the weighted term of the step: two more roundings (the fp32 scale lap_w / (C*Hp*Wp), the fp32 result of the combine kernel,
  which adds the partials in double).
"""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

from style_transfer_visualizer_amd import _lib, core_model, ops, optimization, synthetic
from style_transfer_visualizer_amd import config as stv_config
from style_transfer_visualizer_amd.optimizers import HipAdam, HipLBFGS
from tests import lap_ref
from tests.conftest import GoldenCase, record_parity

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
LAP_W = 100.0
TV_W = 50.0
POOLS = (4, 16)
SIZES = [(64, 64), (48, 80)]
TH, TW, PARTS = _lib.LAP_TILE_H, _lib.LAP_TILE_W, _lib.LAP_LOSS_PARTS


def chain(C: int, Hp: int, Wp: int) -> int:
    return lap_ref.partial_sum_depth(C, Hp, Wp, TH, TW, PARTS)


class _Bar:
    def update(self, n=1):
        return None

    def set_postfix(self, *a, **k):
        return None

    def close(self):
        return None


def nan(shape) -> torch.Tensor:
    return torch.full(tuple(shape), float("nan"), device=DEV)


# ---- the kernel on real operands ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("hw", SIZES + [(33, 50)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_kernel_equals_the_fp32_twin(hw, p):
    H, W = hw
    g = torch.Generator().manual_seed(17 + W + p)
    x, content, dx0 = (torch.randn(1, 3, H, W, generator=g) for _ in range(3))
    Hp, Wp = H // p, W // p
    coef = core_model.lap_coef(LAP_W, 3, Hp, Wp, p)
    target, resid, parts = nan((3, Hp, Wp)), nan((3, Hp, Wp)), nan((PARTS,))
    ops.lap_pool(content.to(DEV), target, p)
    t_ref = lap_ref.pool(content, p)
    assert torch.equal(target.cpu(), torch.from_numpy(t_ref)), "pooled target"
    ops.lap_loss(x.to(DEV), target, resid, parts, p)
    r_ref = lap_ref.resid(x, t_ref, p)
    assert torch.equal(resid.cpu(), torch.from_numpy(r_ref)), "residual"
    dx = dx0.to(DEV)
    ops.lap_grad(resid, dx, p, coef=coef, flags=_lib.ACCUM)
    assert torch.equal(dx.cpu()[0], torch.from_numpy(lap_ref.grad_accum(r_ref, dx0, p, coef))), "accumulated gradient"
    want = lap_ref.raw_sum(r_ref)
    rel = abs(float(parts.double().sum()) - want) / want
    rel_bound = lap_ref.gamma(chain(3, Hp, Wp)) + 1e-12
    print(f"stv_lap {H}x{W} pool {p}: loss relative error {rel:.3e} (bound {rel_bound:.3e})")
    record_parity(f"stv_lap {H}x{W} pool {p} randn", "raw loss sum: relative error", rel, rel_bound,
                  f"chain of {chain(3, Hp, Wp)} roundings; target, residual, gradient equal the fp32 twin")
    assert not bool(torch.isnan(parts).any()) and rel <= rel_bound


# ---- the step ---------------------------------------------------------------------------------------------------------------------

def _model(monkeypatch, precision: str, H: int, W: int):
    case = GoldenCase("vgg19_white_lbfgs")
    weights = case.weights()
    monkeypatch.setattr(core_model, "initialize_vgg", lambda: core_model.build_vgg_features(weights, case.cfg).eval())
    m = case.meta
    model = core_model.StyleContentModel(list(m["style_layers"]), list(m["content_layers"]), precision=precision,
                                         lap_pools=POOLS).to(DEV)
    content = synthetic.synthetic_image(0, H, W)
    model.set_targets(synthetic.synthetic_image(1, H, W).to(DEV), content.to(DEV))
    x = synthetic.synthetic_image(2, H, W) + 0.25 * torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(5))
    return model, x.to(DEV).requires_grad_(True), float(m["style_w"]), float(m["content_w"]), content


@pytest.mark.parametrize("tv_w", [0.0, TV_W], ids=["alone", "with_tv"])
@pytest.mark.parametrize("hw", SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3"])
def test_step_with_the_term_against_the_step_without(precision, hw, tv_w, monkeypatch):
    H, W = hw
    model, x, sw, cw, content = _model(monkeypatch, precision, H, W)
    # the targets set_targets captured are the twin's cell means of the content image
    for p, t in zip(POOLS, model.lap_targets, strict=True):
        assert torch.equal(t.cpu(), torch.from_numpy(lap_ref.pool(content, p))), f"captured target, pool {p}"
    s0, c0, t0 = model.loss_and_grad(x, sw, cw, tv_w=tv_w)
    g0 = x.grad.clone()
    assert model.last_lap_terms() is None
    s1, c1, t1 = model.loss_and_grad(x, sw, cw, tv_w=tv_w, lap_w=LAP_W)
    g1, terms = x.grad.clone(), model.last_lap_terms().clone()
    assert terms.shape == (len(POOLS),) and terms.is_cuda
    assert (model.last_tv_term() is not None) == bool(tv_w)
    assert torch.equal(s1, s0) and torch.equal(c1, c0), "the style / content scores changed with lap_w"
    want_g, want_t = g0, t0
    for k, p in enumerate(POOLS):
        Hp, Wp = H // p, W // p
        resid, parts, written = nan((3, Hp, Wp)), nan((PARTS,)), nan(g0.shape)
        ops.lap_loss(x.detach(), model.lap_targets[k], resid, parts, p)
        ops.lap_grad(resid, written, p, coef=core_model.lap_coef(LAP_W, 3, Hp, Wp, p))
        assert float(written.abs().max()) > 0
        want_g = want_g + written              # the order of the accumulate ops
        want_t = want_t + terms[k]             # the combine's order: one fp32 add per term, in index order
        r_ref = lap_ref.resid(x.detach().cpu(), lap_ref.pool(content, p), p)
        assert torch.equal(resid.cpu(), torch.from_numpy(r_ref)), f"residual of the step's operands, pool {p}"
        want = LAP_W * lap_ref.raw_sum(r_ref) / (3 * Hp * Wp)
        rel = abs(float(terms[k]) - want) / want
        rel_bound = lap_ref.gamma(chain(3, Hp, Wp) + 2) + 1e-12
        record_parity(f"step {precision} {H}x{W} lap_w={LAP_W:g} tv_w={tv_w:g}", f"weighted term, pool {p}: relative error", rel,
                      rel_bound, f"chain of {chain(3, Hp, Wp) + 2} roundings")
        assert float(terms[k]) > 0 and rel <= rel_bound
    assert not torch.equal(g1, g0)
    assert torch.equal(g1, want_g), f"max |diff| {float((g1 - want_g).abs().max()):.3e}"
    assert torch.equal(t1, want_t)
    # back to lap_w = 0: the bits of the step without the term again - the two programs share nothing they should not
    s2, c2, t2 = model.loss_and_grad(x, sw, cw, tv_w=tv_w)
    assert model.last_lap_terms() is None
    assert torch.equal(s2, s0) and torch.equal(c2, c0) and torch.equal(t2, t0) and torch.equal(x.grad, g0)
    # ... and the other way round
    _, _, t3 = model.loss_and_grad(x, sw, cw, tv_w=tv_w, lap_w=LAP_W)
    assert torch.equal(t3, t1) and torch.equal(x.grad, g1) and torch.equal(model.last_lap_terms(), terms)
    with pytest.raises(ValueError, match="lap_w"):
        model.loss_and_grad(x, sw, cw, lap_w=-1.0)


def _run(monkeypatch, precision: str, steps: int, *, lap_w: float, tv_w: float = 0.0, max_iter: int = 1, max_eval: int = 1,
         env: dict | None = None, adam_lr: float | None = None, hw=(64, 64)):
    """Model + runner on the fixture weights at ``hw``; returns (image, history, runner, first-step snapshot)."""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    case = GoldenCase("vgg19_white_lbfgs")
    m = case.meta
    weights = case.weights()
    monkeypatch.setattr(core_model, "initialize_vgg", lambda: core_model.build_vgg_features(weights, case.cfg).eval())
    cfg = stv_config.StyleTransferConfig.model_validate({})
    oc = cfg.optimization
    oc.steps, oc.style_w, oc.content_w, oc.tv_w = steps, m["style_w"], m["content_w"], tv_w
    oc.lap_w, oc.lap_pools = lap_w, list(POOLS)
    oc.init_method = "random"
    oc.style_layers, oc.content_layers = list(m["style_layers"]), list(m["content_layers"])
    oc.normalize = m["normalize"]
    oc.lbfgs_max_iter, oc.lbfgs_max_eval = max_iter, max_eval
    cfg.hardware.precision = precision
    cfg.output.log_every = 5
    cfg.video.create_video = False
    content, style = synthetic.synthetic_image(0, *hw), synthetic.synthetic_image(1, *hw)
    torch.manual_seed(0)
    model, input_img, opt = core_model.prepare_model_and_input(content.to(DEV), style.to(DEV), DEV, oc, precision=precision)
    if adam_lr is not None:
        opt = HipAdam([input_img], lr=adam_lr)
    first = {"x0": input_img.detach().clone()}
    runner = optimization.OptimizationRunner(model, input_img, cfg, optimizer=opt, progress_bar=_Bar())
    img, hist, _ = runner.run()
    torch.cuda.synchronize()
    for k in (env or {}):
        monkeypatch.delenv(k)
    first["model"] = model
    return img.detach().clone(), hist, runner, first


def _terms_at(model, image: torch.Tensor, oc) -> float:
    """The sum of the weighted Laplacian terms at ``image`` (a probe evaluation outside any optimiser step)."""
    probe = image.detach().clone().requires_grad_(True)
    model.loss_and_grad(probe, oc.style_w, oc.content_w, tv_w=oc.tv_w, lap_w=oc.lap_w)
    return float(model.last_lap_terms().sum())


def _bytes(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous().view(torch.uint8).cpu()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_graph_replay_equals_eager_launches(precision, monkeypatch):
    """An OP_LAP on the wrong side of the dgrad or of the update would differ between the captured graph and the eager program
    only by luck; the two must agree bit for bit, and the term must have moved the image."""
    xg, hg, rg, _ = _run(monkeypatch, precision, 5, lap_w=LAP_W, tv_w=TV_W, hw=(48, 80))
    xe, he, re_, _ = _run(monkeypatch, precision, 5, lap_w=LAP_W, tv_w=TV_W, hw=(48, 80), env={"STV_HIP_GRAPH": "0"})
    x0, h0, _, _ = _run(monkeypatch, precision, 5, lap_w=0.0, tv_w=TV_W, hw=(48, 80))
    assert isinstance(rg.optimizer, HipLBFGS) and isinstance(re_.optimizer, HipLBFGS)
    assert torch.equal(xg, xe), f"max |diff| {float((xg - xe).abs().max()):.3e}"
    assert hg == he and all(len(v) == 5 for v in hg.values()) and all(math.isfinite(v) for v in hg["total_loss"])
    assert torch.equal(_bytes(rg.optimizer._dev_state), _bytes(re_.optimizer._dev_state))
    assert torch.equal(_bytes(rg.optimizer._work), _bytes(re_.optimizer._work))
    assert not torch.equal(xg, x0) and hg["total_loss"][0] > h0["total_loss"][0]
    assert hg["style_loss"][0] == h0["style_loss"][0] and hg["content_loss"][0] == h0["content_loss"][0]


def test_multi_iteration_lbfgs_lowers_the_term(monkeypatch):
    """Five steps of four iterations each from a random start: finite losses, and the Laplacian term has fallen."""
    x5, hist, runner, first = _run(monkeypatch, "bf16", 5, lap_w=LAP_W, max_iter=4, max_eval=5)
    opt = runner.optimizer
    assert isinstance(opt, HipLBFGS) and opt.iters_per_step == 4
    assert all(len(v) == 5 for v in hist.values()) and all(math.isfinite(v) for vs in hist.values() for v in vs)
    oc = runner.config.optimization
    before, after = _terms_at(first["model"], first["x0"], oc), _terms_at(first["model"], x5, oc)
    print(f"L-BFGS 5 x 4 iterations: weighted Laplacian terms {before:.5g} -> {after:.5g}")
    record_parity("L-BFGS 5x4 iterations 64x64 random init", "Laplacian terms after / before", after / before, 1.0,
                  f"{before:.5g} -> {after:.5g}")
    assert math.isfinite(after) and after < before
    assert hist["total_loss"][-1] < hist["total_loss"][0]


def test_adam_steps_lower_the_term(monkeypatch):
    x5, hist, runner, first = _run(monkeypatch, "fp32", 5, lap_w=LAP_W, adam_lr=1e-2)
    assert isinstance(runner.optimizer, HipAdam) and all(len(v) == 5 for v in hist.values())
    assert all(math.isfinite(v) for vs in hist.values() for v in vs)
    oc = runner.config.optimization
    before, after = _terms_at(first["model"], first["x0"], oc), _terms_at(first["model"], x5, oc)
    print(f"Adam 5 steps: weighted Laplacian terms {before:.5g} -> {after:.5g}")
    record_parity("Adam 5 steps 64x64 random init", "Laplacian terms after / before", after / before, 1.0, f"{before:.5g} -> {after:.5g}")
    assert math.isfinite(after) and after < before and not torch.equal(x5, first["x0"])


# ---- command line -------------------------------------------------------------------------------------------------------------------

CLI_LAP_W = 1000.0


def test_cli_with_a_pyramid_keeps_the_result_closer_to_the_content_laplacian(tmp_path, monkeypatch):
    """--lap-w --lap-pool 4,16 --pyramid-levels 2 through the command line (every level pools its own content): the run
    finishes, writes its PNG, and the final image's Laplacian loss against the content picture is below the same run's
    without the term."""
    from PIL import Image

    from style_transfer_visualizer_amd import cli
    monkeypatch.setenv("STV_SYNTHETIC_WEIGHTS", "0")
    pictures = {}
    for name, seed in (("content", 0), ("style", 1)):
        img = synthetic.synthetic_image(seed, 128, 128, normalize=False)[0].permute(1, 2, 0).mul(255).byte().numpy()
        Image.fromarray(img).save(tmp_path / f"{name}.png")
        pictures[name] = torch.from_numpy(img).permute(2, 0, 1).double() / 255.0
    lap = {}
    for w in (CLI_LAP_W, 0.0):
        out_dir = tmp_path / f"out_{w:g}"
        cli.main(["--content", str(tmp_path / "content.png"), "--style", str(tmp_path / "style.png"), "--steps", "16",
                  "--init-method", "random", "--device", "cuda", "--no-video", "--final-only", "--seed", "0", "--no-plot",
                  "--lap-w", str(w), "--lap-pool", "4,16", "--pyramid-levels", "2", "--output", str(out_dir)])
        (png,) = list(out_dir.glob("stylized_*.png"))
        pixels = torch.from_numpy(np.array(Image.open(png).convert("RGB"))).permute(2, 0, 1).double() / 255.0
        assert pixels.shape == (3, 128, 128)
        lap[w] = sum(lap_ref.loss(pixels, pictures["content"], p) for p in (4, 16))
    print(f"Laplacian loss of the final image after 16 steps: --lap-w {CLI_LAP_W:g}: {lap[CLI_LAP_W]:.6f}, --lap-w 0: {lap[0.0]:.6f}")
    record_parity("cli 128x128 2 levels x16 random init", f"lap(--lap-w {CLI_LAP_W:g}) / lap(--lap-w 0)", lap[CLI_LAP_W] / lap[0.0], 1.0,
                  f"{lap[CLI_LAP_W]:.6f} against {lap[0.0]:.6f}")
    assert lap[CLI_LAP_W] < lap[0.0]
