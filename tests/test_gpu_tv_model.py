"""The total-variation term on real operands and through the whole step (64x64 and 48x80, the synthetic VGG19 of the
fixture-size tests): stv_tv against float64 on random normal images, ``loss_and_grad(..., tv_w=)`` against ``tv_w=0`` on
the same image bit for bit, graph replay against eager launches, multi-iteration L-BFGS, Adam, and the CLI.

Bounds (derived, u = 2^-24, nothing measured went into them):

* gradient, per element: ``8 u coef sum|differences|`` - four subtractions, three additions and one multiply round;
* raw loss sum, relative (all terms are non-negative, so the relative error of a sum is at most the longest chain of
  roundings any term goes through): a thread adds 2 * TV_VEC squared differences per pass of the capped grid by FMA
  (one rounding each), a difference carries one rounding and is squared (2), the wave butterfly adds 6 levels, the
  workgroup 16 wave sums; the partials are added in float64.  ``(2 * TV_VEC * passes + 2 + 6 + 16) u``;
* the weighted term of the step: two more roundings (the fp32 scale tv_w / (C*H*W), the fp32 result of the combine
  kernel, which adds the partials in double).
"""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

from style_transfer_visualizer_amd import _lib, core_model, ops, optimization, synthetic
from style_transfer_visualizer_amd import config as stv_config
from style_transfer_visualizer_amd.optimizers import HipAdam, HipLBFGS
from tests import tv_ref
from tests.conftest import GoldenCase, record_parity

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
U = 2.0 ** -24
TV_W = 50.0
SIZES = [(64, 64), (48, 80)]


def loss_chain(C: int, H: int, W: int) -> int:
    items = C * H * -(-W // _lib.TV_VEC)
    passes = -(-items // (_lib.TV_LOSS_PARTS * _lib.TV_THREADS))
    return 2 * _lib.TV_VEC * passes + 2 + 6 + 16


class _Bar:
    def update(self, n=1):
        return None

    def set_postfix(self, *a, **k):
        return None

    def close(self):
        return None


# ---- the kernel on real operands ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", SIZES + [(33, 50)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_kernel_against_float64(hw):
    H, W = hw
    x = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(11 + W))
    coef = core_model.tv_coef(TV_W, 3, H, W)
    xd = x.to(DEV)
    parts = torch.full((_lib.TV_LOSS_PARTS,), float("nan"), device=DEV)
    dx = torch.full((1, 3, H, W), float("nan"), device=DEV)
    ops.tv(xd, loss_part=parts, dx=dx, coef=coef)
    want = coef * tv_ref.neighbour_sum(x)
    bound = 8 * U * coef * tv_ref.abs_difference_sum(x)
    err = (dx.cpu().double().reshape(3, H, W) - want).abs()
    worst = float((err / bound).max())
    raw = float(tv_ref.raw_sum(x))
    rel = abs(float(parts.double().sum()) - raw) / raw
    rel_bound = loss_chain(3, H, W) * U
    print(f"stv_tv {H}x{W}: gradient error / bound {worst:.3f}, loss relative error {rel:.3e} (bound {rel_bound:.3e})")
    record_parity(f"stv_tv {H}x{W} randn", "gradient: worst error / derived bound", worst, 1.0, "8 u coef sum|d|")
    record_parity(f"stv_tv {H}x{W} randn", "raw loss sum: relative error", rel, rel_bound, f"chain of {loss_chain(3, H, W)} roundings")
    assert bool((err <= bound).all()), f"gradient: worst error is {worst:.3f} of the bound"
    assert rel <= rel_bound


# ---- the step ---------------------------------------------------------------------------------------------------------------------

def _model(monkeypatch, precision: str, H: int, W: int):
    case = GoldenCase("vgg19_white_lbfgs")
    weights = case.weights()
    monkeypatch.setattr(core_model, "initialize_vgg", lambda: core_model.build_vgg_features(weights, case.cfg).eval())
    m = case.meta
    model = core_model.StyleContentModel(list(m["style_layers"]), list(m["content_layers"]), precision=precision).to(DEV)
    model.set_targets(synthetic.synthetic_image(1, H, W).to(DEV), synthetic.synthetic_image(0, H, W).to(DEV))
    x = synthetic.synthetic_image(2, H, W) + 0.25 * torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(5))
    return model, x.to(DEV).requires_grad_(True), float(m["style_w"]), float(m["content_w"])


@pytest.mark.parametrize("hw", SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3"])
def test_step_with_the_term_against_the_step_without(precision, hw, monkeypatch):
    H, W = hw
    model, x, sw, cw = _model(monkeypatch, precision, H, W)
    s0, c0, t0 = model.loss_and_grad(x, sw, cw)
    g0 = x.grad.clone()
    assert model.last_tv_term() is None
    s1, c1, t1 = model.loss_and_grad(x, sw, cw, tv_w=TV_W)
    g1, term = x.grad.clone(), model.last_tv_term().clone()
    assert term.dim() == 0 and term.is_cuda
    assert torch.equal(s1, s0) and torch.equal(c1, c0), "the style / content scores changed with tv_w"
    written = torch.full_like(g0, float("nan"))
    ops.tv(x.detach(), dx=written, coef=core_model.tv_coef(TV_W, 3, H, W))
    assert float(written.abs().max()) > 0 and not torch.equal(g1, g0)
    assert torch.equal(g1, g0 + written), f"max |diff| {float((g1 - (g0 + written)).abs().max()):.3e}"
    assert torch.equal(t1, t0 + term) and float(term) > 0
    want = TV_W * float(tv_ref.tv(x))
    rel = abs(float(term) - want) / want
    rel_bound = (loss_chain(3, H, W) + 2) * U
    record_parity(f"step {precision} {H}x{W} tv_w={TV_W:g}", "weighted TV term: relative error", rel, rel_bound,
                  f"chain of {loss_chain(3, H, W) + 2} roundings")
    assert rel <= rel_bound
    # back to tv_w = 0: the parent's bits again - the two programs share nothing they should not
    s2, c2, t2 = model.loss_and_grad(x, sw, cw)
    assert model.last_tv_term() is None
    assert torch.equal(s2, s0) and torch.equal(c2, c0) and torch.equal(t2, t0) and torch.equal(x.grad, g0)
    # ... and the other way round
    _, _, t3 = model.loss_and_grad(x, sw, cw, tv_w=TV_W)
    assert torch.equal(t3, t1) and torch.equal(x.grad, g1)
    with pytest.raises(ValueError, match="tv_w"):
        model.loss_and_grad(x, sw, cw, tv_w=-1.0)


def _run(monkeypatch, precision: str, steps: int, *, tv_w: float, max_iter: int = 1, max_eval: int = 1, env: dict | None = None,
         adam_lr: float | None = None, hw=(64, 64)):
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

    def on_step_end(metrics):
        if metrics.step == 1:
            first["x1"] = input_img.detach().clone()
    runner = optimization.OptimizationRunner(model, input_img, cfg, optimizer=opt, progress_bar=_Bar(),
                                             callbacks=optimization.OptimizationCallbacks(on_step_end=on_step_end))
    img, hist, _ = runner.run()
    torch.cuda.synchronize()
    for k in (env or {}):
        monkeypatch.delenv(k)
    first["model"] = model
    return img.detach().clone(), hist, runner, first


def _bytes(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous().view(torch.uint8).cpu()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_graph_replay_equals_eager_launches(precision, monkeypatch):
    """An OP_TV on the wrong side of the dgrad or of the update would differ between the captured graph and the eager
    program only by luck; the two must agree bit for bit, and the term must have moved the image."""
    xg, hg, rg, _ = _run(monkeypatch, precision, 5, tv_w=TV_W, hw=(48, 80))
    xe, he, re_, _ = _run(monkeypatch, precision, 5, tv_w=TV_W, hw=(48, 80), env={"STV_HIP_GRAPH": "0"})
    x0, h0, _, _ = _run(monkeypatch, precision, 5, tv_w=0.0, hw=(48, 80))
    assert isinstance(rg.optimizer, HipLBFGS) and isinstance(re_.optimizer, HipLBFGS)
    assert torch.equal(xg, xe), f"max |diff| {float((xg - xe).abs().max()):.3e}"
    assert hg == he and all(len(v) == 5 for v in hg.values()) and all(math.isfinite(v) for v in hg["total_loss"])
    assert torch.equal(_bytes(rg.optimizer._dev_state), _bytes(re_.optimizer._dev_state))
    assert torch.equal(_bytes(rg.optimizer._work), _bytes(re_.optimizer._work))
    assert rg.optimizer.device_state() == re_.optimizer.device_state()
    assert not torch.equal(xg, x0) and hg["total_loss"][0] > h0["total_loss"][0]
    assert hg["style_loss"][0] == h0["style_loss"][0] and hg["content_loss"][0] == h0["content_loss"][0]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_ten_steps_of_four_iterations_equal_forty_default_steps(precision, monkeypatch):
    """The multi-iteration L-BFGS op reads the total - term included - from scores[2]: 10 steps at max_iter=4, max_eval=5
    are 40 default steps, bit for bit, with the term as without."""
    x40, h40, r40, _ = _run(monkeypatch, precision, 40, tv_w=TV_W)
    x10, h10, r10, _ = _run(monkeypatch, precision, 10, tv_w=TV_W, max_iter=4, max_eval=5)
    opt = r10.optimizer
    assert isinstance(opt, HipLBFGS) and (opt.iters_per_step, opt.evals_per_step) == (4, 4)
    assert r40._closure_calls == 40 and r10._closure_calls == 40
    assert torch.equal(x10, x40), f"max |diff| {float((x10 - x40).abs().max()):.3e}"
    assert {k: v[3::4] for k, v in h40.items()} == h10 and all(len(v) == 10 for v in h10.values())
    st = opt.device_state()
    assert st["n_iter"] == 40 and st["step_pos"] == 0


def test_adam_steps(monkeypatch):
    """Five injected-Adam steps: finite losses; the first step's image is the one an Adam twin leaves when it is fed
    grad_0 + stv_tv(write) - bit for bit against a second HipAdam, and against torch.optim.Adam within the tolerance
    HipAdam itself is held to (tests/test_gpu_ops.py::test_adam_step_matches_oracle: a square root and a division)."""
    lr = 1e-2
    x5, hist, runner, first = _run(monkeypatch, "fp32", 5, tv_w=TV_W, adam_lr=lr)
    assert isinstance(runner.optimizer, HipAdam) and all(len(v) == 5 for v in hist.values())
    assert all(math.isfinite(v) for vs in hist.values() for v in vs)
    model, x0, x1 = first["model"], first["x0"], first["x1"]
    H, W = x0.shape[-2:]
    probe = x0.clone().requires_grad_(True)
    model.loss_and_grad(probe, runner.config.optimization.style_w, runner.config.optimization.content_w)
    written = torch.full_like(x0, float("nan"))
    ops.tv(x0, dx=written, coef=core_model.tv_coef(TV_W, 3, H, W))
    grad = probe.grad + written
    twin = x0.clone().requires_grad_(True)
    twin.grad = grad.clone()
    HipAdam([twin], lr=lr).step()
    assert torch.equal(twin.detach(), x1), f"max |diff| {float((twin.detach() - x1).abs().max()):.3e}"
    ref = x0.cpu().clone().requires_grad_(True)
    ref.grad = grad.cpu().clone()
    torch.optim.Adam([ref], lr=lr).step()
    np.testing.assert_allclose(x1.cpu().numpy(), ref.detach().numpy(), rtol=1e-5, atol=1e-6)
    assert not torch.equal(x1, x0)


# ---- command line -------------------------------------------------------------------------------------------------------------------

CLI_TV_W = 1000.0


def test_cli_lowers_the_total_variation_of_the_result(tmp_path, monkeypatch):
    """--tv-w through the command line: the run finishes, writes its PNG, and the final image's total variation is well
    below the same run's without the term."""
    from PIL import Image

    from style_transfer_visualizer_amd import cli
    monkeypatch.setenv("STV_SYNTHETIC_WEIGHTS", "0")
    for name, seed in (("content", 0), ("style", 1)):
        img = synthetic.synthetic_image(seed, 64, 64, normalize=False)[0].permute(1, 2, 0).mul(255).byte().numpy()
        Image.fromarray(img).save(tmp_path / f"{name}.png")
    tv = {}
    for w in (CLI_TV_W, 0.0):
        out_dir = tmp_path / f"out_{w:g}"
        cli.main(["--content", str(tmp_path / "content.png"), "--style", str(tmp_path / "style.png"), "--steps", "20",
                  "--init-method", "random", "--device", "cuda", "--no-video", "--final-only", "--seed", "0", "--no-plot",
                  "--tv-w", str(w), "--output", str(out_dir)])
        (png,) = list(out_dir.glob("stylized_*.png"))
        pixels = torch.from_numpy(np.array(Image.open(png).convert("RGB"))).permute(2, 0, 1).double() / 255.0
        assert pixels.shape == (3, 64, 64)
        tv[w] = float(tv_ref.tv(pixels))
    print(f"TV of the final image after 20 steps: --tv-w {CLI_TV_W:g}: {tv[CLI_TV_W]:.5f}, --tv-w 0: {tv[0.0]:.5f}")
    record_parity("cli 64x64 x20 random init", f"TV(--tv-w {CLI_TV_W:g}) / TV(--tv-w 0)", tv[CLI_TV_W] / tv[0.0], 0.5,
                  f"{tv[CLI_TV_W]:.5f} against {tv[0.0]:.5f}")
    assert tv[CLI_TV_W] < 0.5 * tv[0.0]
