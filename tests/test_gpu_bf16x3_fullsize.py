"""bf16x3 (fp32 storage, split-bf16 products) end to end on the full VGG19 widths.

* 512^2 (the fp32 parity set-up of tests/test_gpu_fullsize.py): targets and losses against the fp32 oracle, the
  gradient against float64 ON THE SAME ReLU / max-pool BRANCH (``pu.lock`` with the HIP decisions; near-ties decided
  differently would otherwise move whole gradient entries), and per pixel against the fp32 oracle given the HIP
  decisions.
* The reference's own in-trajectory images (cfg0_256_content_lbfgs50, vgg19_128_random_lbfgs12): losses against the
  reference's recorded values, gradient per pixel against the reference arithmetic on the HIP path's branch.
* configs[0] literally through ``cli.main --precision bf16x3`` (tests/test_gpu_configs.py's run, held to the fp32 bars).
* Two 20-step L-BFGS runs at 512^2: bit-identical images and losses.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import core_model_ref as ocm
from style_transfer_visualizer_amd import core_model, synthetic
from style_transfer_visualizer_amd.optimizers import HipLBFGS
from tests import parity_util as pu
from tests.conftest import LARGE_CASES, GoldenCase, record_parity

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
S_LAYERS, C_LAYERS = [0, 5, 10, 19, 28], [21]
STYLE_W, CONTENT_W = 1e5, 1.0


def _model(precision: str, style, content):
    model = core_model.StyleContentModel(S_LAYERS, C_LAYERS, precision=precision).to(DEV)
    model.set_targets(style.to(DEV), content.to(DEV))
    return model


def test_512_against_float64_on_the_same_branch(monkeypatch):
    monkeypatch.setenv("STV_SYNTHETIC_WEIGHTS", "0")
    size, case = 512, "vgg19_512x512_bf16x3"
    weights = synthetic.synthetic_conv_weights(0)
    content = synthetic.synthetic_image(0, size, size)
    style = synthetic.synthetic_image(1, size, size)
    x0 = torch.randn(content.shape, generator=torch.Generator().manual_seed(0))     # tests/golden/fullsize_fp64_512.npz
    model = _model("bf16x3", style, content)
    x = x0.to(DEV).clone().requires_grad_(True)
    s, c, t = model.loss_and_grad(x, STYLE_W, CONTENT_W)
    g = x.grad.detach().cpu().double()
    dec = pu.hip_decisions(model)

    oracle = ocm.OracleModel(ocm.vgg_program(weights, synthetic.VGG19_CFG), S_LAYERS, C_LAYERS)
    oracle.set_targets(style, content)
    for i, (tg, to) in enumerate(zip(model.style_targets, oracle.style_targets, strict=True)):
        dev = float((tg.cpu() - to).abs().max() / to.abs().max())
        record_parity(case, f"Gram target {i} (of max)", dev, 1e-4)
        assert dev <= 1e-4
    ct, co = model.content_targets[0].float().cpu(), oracle.content_targets[0]
    dev = float((ct - co).abs().max() / co.abs().max())
    record_parity(case, "content target (of max)", dev, 1e-4)
    assert dev <= 1e-4

    from tests.test_gpu_fullsize import _fp64_cache
    cache = _fp64_cache(size, x0)
    for nm, got, want in zip(("style", "content", "total"), (float(s), float(c), float(t)), cache["losses_fp32"], strict=True):
        rel = abs(got - float(want)) / abs(float(want))
        record_parity(case, f"{nm} loss vs fp32 oracle (rel)", rel, 1e-4)
        assert rel <= 1e-4
    k = int(cache["sub"])
    g64s = torch.from_numpy(cache["g64_sub"]).double()
    plain = float((g[..., ::k, ::k] - g64s).norm() / g64s.norm())
    record_parity(case, f"grad vs fp64, own decisions (rel rms, every {k}th row/col)", plain, float("nan"),
                  f"reported only: ReLU/pool near-ties included; the reference's CPU-fp32 path: {float(cache['err_cpu_sub']):.2e}")

    # float64 with the HIP path's decisions imposed: the split arithmetic alone
    w64 = [(w.double(), b.double()) for w, b in weights]
    oracle64 = ocm.OracleModel(ocm.vgg_program(w64, synthetic.VGG19_CFG), S_LAYERS, C_LAYERS)
    oracle64.set_targets(style.double(), content.double())
    g64 = ocm.loss_and_grad(pu.lock(oracle64, dec), x0.double(), STYLE_W, CONTENT_W)[3]
    err = float((g - g64).norm() / g64.norm())
    record_parity(case, "grad vs fp64 on the same branch (rel rms)", err, 1e-5, "issue bar; the fp32 mode measures ~4e-7")
    g32 = ocm.loss_and_grad(pu.lock(oracle, dec), x0, STYLE_W, CONTENT_W)[3].double()
    mx = float((g - g32).abs().max() / g32.abs().max())
    record_parity(case, "grad vs CPU-fp32 given the HIP decisions, per pixel max (of scale)", mx, 1e-4)
    print(f"{case}: grad vs fp64 same branch rel rms {err:.2e}, unlocked {plain:.2e}, per pixel vs fp32 locked {mx:.2e}")
    assert err <= 1e-5, f"{case}: {err:.2e} from float64 on the HIP path's branch"
    assert mx <= 1e-4


@pytest.mark.parametrize("name", LARGE_CASES)
def test_reference_in_trajectory_images(name, monkeypatch):
    monkeypatch.setenv("STV_SYNTHETIC_WEIGHTS", "0")
    case = GoldenCase(name)
    m, k = case.meta, case.meta["compact"]
    monkeypatch.setattr(core_model, "initialize_vgg", lambda: core_model.build_vgg_features(case.weights(), case.cfg).eval())
    content, style = case.images()
    model = core_model.StyleContentModel(list(m["style_layers"]), list(m["content_layers"]), precision="bf16x3").to(DEV)
    model.set_targets(style.to(DEV), content.to(DEV))
    oracle = ocm.OracleModel(ocm.vgg_program(case.weights(), case.cfg), m["style_layers"], m["content_layers"])
    oracle.set_targets(style, content)
    prog64 = ocm.vgg_program([(w.double(), b.double()) for w, b in case.weights()], case.cfg)
    oracle64 = ocm.OracleModel(prog64, m["style_layers"], m["content_layers"])
    oracle64.set_targets(style.double(), content.double())
    for k_full in m["full_steps"]:
        x_ref = torch.from_numpy(case.arrays[f"x_after_step_{k_full}"])
        x = x_ref.to(DEV).clone().requires_grad_(True)
        s, c, t = model.loss_and_grad(x, m["style_w"], m["content_w"])
        got = (float(s), float(c), float(t))
        want = tuple(float(case.arrays[f"{key}_loss"][k_full]) for key in ("style", "content", "total"))
        for key, a, b, wgt in zip(("style", "content", "total"), got, want, (m["style_w"], m["content_w"], 1.0), strict=True):
            rel = abs(a - b) / max(abs(b), 1e-30)
            if wgt * abs(a - b) <= 1e-6 * abs(want[2]):     # a term negligible in the total (as the fp32 test)
                rel = min(rel, 1e-6)
            record_parity(f"{name} bf16x3", f"{key} loss AT the reference's image after step {k_full} (rel)", rel, 1e-4)
            assert rel <= 1e-4, f"{name}: {key} loss {a!r} vs the reference's {b!r}"
        g = x.grad.detach().cpu()
        gscale = float(case.arrays[f"grad_at_step_{k_full + 1}_absmax"])
        g_ref_sub = case.arrays[f"grad_at_step_{k_full + 1}_sub"]
        plain = float(np.abs(g.numpy()[..., ::k, ::k] - g_ref_sub).max() / gscale)
        # on the HIP path's ReLU / pool branch, against float64: 1e-4 of scale (north_star), except at an image where
        # the problem itself is ill-conditioned - late in a run the style gradient is G - T, a small difference of
        # large Gram sums, and the reference's own fp32 arithmetic is then already far from float64 (3.4e-4 of scale at
        # cfg0's step 50).  There bf16x3's 2^-17 products (2^7 coarser than fp32's 2^-24) sit at a multiple of the
        # reference's error: measured 20x and 22x; bound 32x.  This is the mode's accuracy, stated in DESIGN.md 8b.
        dec = pu.hip_decisions(model)
        g_locked = ocm.loss_and_grad(pu.lock(oracle, dec), x_ref, m["style_w"], m["content_w"])[3]
        g64 = ocm.loss_and_grad(pu.lock(oracle64, dec), x_ref.double(), m["style_w"], m["content_w"])[3]
        err_hip = float((g.double() - g64).abs().max() / gscale)
        err_cpu = float((g_locked.double() - g64).abs().max() / gscale)
        bound = max(1e-4, 32.0 * err_cpu)
        record_parity(f"{name} bf16x3", f"gradient at step {k_full + 1} vs FLOAT64 on the HIP branch, per pixel (of scale)",
                      err_hip, bound, f"the reference arithmetic on that branch: {err_cpu:.1e} from float64; plain comparison "
                      f"with the reference's gradient (subsampled): {plain:.1e}")
        assert err_hip <= bound, f"{name} step {k_full + 1}: {err_hip:.2e} of scale from float64 (reference arithmetic {err_cpu:.2e})"


def test_configs0_literal_run_through_the_cli(tmp_path, monkeypatch):
    from tests import test_gpu_configs
    test_gpu_configs.test_configs0_literal_run_through_the_cli("bf16x3", tmp_path, monkeypatch)


def test_two_20_step_runs_are_bit_identical(monkeypatch):
    monkeypatch.setenv("STV_SYNTHETIC_WEIGHTS", "0")
    content = synthetic.synthetic_image(0, 512, 512)
    style = synthetic.synthetic_image(1, 512, 512)

    def run():
        model = _model("bf16x3", style, content)
        x = torch.randn(content.shape, generator=torch.Generator().manual_seed(0)).to(DEV).requires_grad_(True)
        opt = HipLBFGS([x], lr=1.0)
        losses = []
        for _ in range(20):
            losses.append(float(opt.step(lambda: model.loss_and_grad(x, STYLE_W, CONTENT_W)[2])))
        torch.cuda.synchronize()
        out = x.detach().cpu().clone(), losses
        del model, opt, x
        torch.cuda.empty_cache()
        return out
    a, b = run(), run()
    assert torch.equal(a[0], b[0]) and a[1] == b[1]
    assert all(np.isfinite(a[1])) and a[1][-1] < a[1][0]
