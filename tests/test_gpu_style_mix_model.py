"""Several style images and per-layer style weights through the model, the runner and ``main.style_transfer`` (64x64 and
48x80, the weights of the ``vgg19_white_lbfgs`` fixture, as tests/test_gpu_tv_model.py).

Targets: the blended ``style_targets`` against the NumPy twin of ``stv_gram_blend`` (tests/blend_ref.py) applied to the
targets captured one image at a time, bit for bit.  Step: blended targets against assigned targets, layer weights against
their power-of-two and all-ones identities bit for bit, and against the CPU oracle with the comparison and the bound
tests/test_gpu_model.py applies to the unweighted step of the same fixture:

* fp32: max |gradient error| <= 2e-4 of the gradient's scale, and where a ReLU / max-pool near-tie makes the plain comparison
  miss, the same bound on the branch the HIP path took (``test_targets_and_first_step_match_reference``);
* bf16: max |gradient error| < 0.1 of scale against the fp32 oracle (``test_bf16_storage_tracks_fp32``);
* bf16x3: tests/test_gpu_model.py holds no bf16x3 row for this fixture; the mode's contract is fp32-grade products on fp32
  storage, so it is held to the fp32 comparison and bound.

The weighted style score against ``forward()``'s per-layer losses: both come from the same loss partials, ``forward()`` rounds
each ``loss_l`` to fp32 (half an ulp each, relative to a term no larger than the sum when every weight is >= 0), the step
rounds each ``w_l/(C*C)`` scale and the sum: 2 ulp of the result bounds them.
"""
from __future__ import annotations

import csv
import math

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import core_model_ref as ocm
from style_transfer_visualizer_amd import _lib, color, core_model, image_io, main, ops, optimization, pyramid, runtime, synthetic
from style_transfer_visualizer_amd import config as stv_config
from style_transfer_visualizer_amd import resize as resize_rules
from style_transfer_visualizer_amd import style_mix
from style_transfer_visualizer_amd.optimizers import HipLBFGS
from style_transfer_visualizer_amd.type_defs import InputPaths
from tests import blend_ref
from tests import parity_util as pu
from tests.conftest import GoldenCase, record_parity

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
PRECISIONS = ["fp32", "bf16", "bf16x3"]
BLEND = (0.7, 0.3)
LAYER_W = (1.0, 0.5, 0.25, 2.0, 0.0)


class _Bar:
    def update(self, n=1):
        return None

    def set_postfix(self, *a, **k):
        return None

    def close(self):
        return None


@pytest.fixture
def blend_calls(monkeypatch):
    """Counts the launches of ``ops.gram_blend``."""
    calls = []
    real = ops.gram_blend

    def counted(stack, weights, out=None):
        calls.append((tuple(stack.shape), [float(w) for w in weights]))
        return real(stack, weights, out=out)
    monkeypatch.setattr(ops, "gram_blend", counted)
    return calls


def _case(monkeypatch) -> GoldenCase:
    case = GoldenCase("vgg19_white_lbfgs")
    weights = case.weights()
    monkeypatch.setattr(core_model, "initialize_vgg", lambda: core_model.build_vgg_features(weights, case.cfg).eval())
    return case


def _new_model(case: GoldenCase, precision: str, layer_w=None):
    m = case.meta
    return core_model.StyleContentModel(list(m["style_layers"]), list(m["content_layers"]), precision=precision,
                                        style_layer_weights=layer_w).to(DEV)


def _images():
    """Style A 64x64, style B 48x80, content 64x64, and the image to evaluate at: one leaf tensor per test, so that every
    evaluation of a model keys its program by the same addresses."""
    a, b = synthetic.synthetic_image(1, 64, 64).to(DEV), synthetic.synthetic_image(3, 48, 80).to(DEV)
    content = synthetic.synthetic_image(0, 64, 64).to(DEV)
    x = synthetic.synthetic_image(2, 64, 64) + 0.25 * torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(5))
    return a, b, content, x.to(DEV).requires_grad_(True)


def _captured(model, style, content) -> list[torch.Tensor]:
    model.set_targets(style, content)
    return [t.clone() for t in model.style_targets]


def _twin(tables_a, tables_b, raw) -> list[torch.Tensor]:
    w = style_mix.blend_weights(raw, 2)
    return [torch.from_numpy(blend_ref.blend(np.stack([ta.cpu().numpy(), tb.cpu().numpy()]), w)).to(DEV)
            for ta, tb in zip(tables_a, tables_b, strict=True)]


def _eval(model, x, sw, cw):
    s, c, t = model.loss_and_grad(x, sw, cw)
    return s.clone(), c.clone(), t.clone(), x.grad.clone()


# ---- targets ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_blended_targets_equal_the_twin_of_the_single_captures(precision, monkeypatch, blend_calls):
    case = _case(monkeypatch)
    a, b, content, _ = _images()
    model = _new_model(case, precision)
    ta, tb = _captured(model, a, content), _captured(model, b, content)
    assert blend_calls == [] and not any(torch.equal(p, q) for p, q in zip(ta, tb, strict=True))
    assert all(torch.equal(p, q) for p, q in zip(_captured(model, a, content), ta, strict=True))      # captures reproduce
    model.set_targets([a, b], content, style_blend=list(BLEND))
    want = _twin(ta, tb, BLEND)
    assert len(blend_calls) == len(ta) == 5                                   # one launch per style layer
    assert all(shape == (2, t.shape[0], t.shape[0]) for (shape, _), t in zip(blend_calls, ta, strict=True))
    assert all(w == [float(np.float32(0.7)), float(np.float32(0.3))] for _, w in blend_calls)
    for got, ref, t in zip(model.style_targets, want, ta, strict=True):
        assert got.dtype == torch.float32 and got.shape == t.shape and got.is_contiguous()
        assert torch.equal(got, ref), f"{int((got != ref).sum())} elements differ from the twin"
        assert not torch.equal(got, t)
    # equal weights by default, and the unnormalised form of the same weights
    model.set_targets([a, b], content)
    assert all(torch.equal(g, r) for g, r in zip(model.style_targets, _twin(ta, tb, (0.5, 0.5)), strict=True))
    model.set_targets((a, b), content, style_blend=[7, 3])
    assert all(torch.equal(g, r) for g, r in zip(model.style_targets, want, strict=True))
    # [A, A] with (0.5, 0.5) and [A, B] with (1, 0) are A alone
    for styles, raw in (([a, a], (0.5, 0.5)), ([a, b], (1, 0))):
        model.set_targets(styles, content, style_blend=list(raw))
        assert all(torch.equal(g, t) for g, t in zip(model.style_targets, ta, strict=True)), (raw,)


def test_one_style_launches_no_blend(monkeypatch, blend_calls):
    case = _case(monkeypatch)
    a, _, content, x = _images()
    model = _new_model(case, "fp32")
    plain = _captured(model, a, content)
    base = _eval(model, x, 1e5, 1.0)
    for form, kw in ((a, {}), ([a], {}), ((a,), {}), ([a], {"style_blend": [3.0]}), (a, {"style_blend": [1]})):
        model.set_targets(form, content, **kw)
        assert all(torch.equal(g, t) for g, t in zip(model.style_targets, plain, strict=True))
        got = _eval(model, x, 1e5, 1.0)
        assert all(torch.equal(p, q) for p, q in zip(got, base, strict=True))
    assert blend_calls == []
    with pytest.raises(ValueError, match=r"2 weights \[1\.0, 1\.0\] for 1 style image"):
        model.set_targets(a, content, style_blend=[1, 1])
    with pytest.raises(ValueError, match="got 9"):
        model.set_targets([a] * 9, content)
    with pytest.raises(ValueError, match="got 0"):
        model.set_targets([], content)
    assert blend_calls == []


# ---- the step with blended targets ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_step_with_blended_targets_equals_the_step_with_assigned_targets(precision, monkeypatch):
    case = _case(monkeypatch)
    sw, cw = float(case.meta["style_w"]), float(case.meta["content_w"])
    a, b, content, x = _images()
    model = _new_model(case, precision)
    ta, tb = _captured(model, a, content), _captured(model, b, content)
    model.set_targets([a, b], content, style_blend=list(BLEND))
    got = _eval(model, x, sw, cw)
    other = _new_model(case, precision)
    other.set_targets(a, content)
    only_a = _eval(other, x, sw, cw)
    other.style_targets = _twin(ta, tb, BLEND)
    want = _eval(other, x, sw, cw)
    for name, p, q in zip(("style", "content", "total", "gradient"), got, want, strict=True):
        assert torch.equal(p, q), f"{precision} {name}: max |diff| {float((p - q).abs().max()):.3e}"
    assert torch.isfinite(got[3]).all() and not torch.equal(got[0], only_a[0]) and not torch.equal(got[3], only_a[3])


# ---- layer weights, exact ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_layer_weight_identities(precision, monkeypatch):
    case = _case(monkeypatch)
    sw, cw = float(case.meta["style_w"]), float(case.meta["content_w"])
    a, _, content, x = _images()
    model = _new_model(case, precision)
    model.set_targets(a, content)
    base = _eval(model, x, sw, cw)
    (eng,) = model._engines.values()
    n_programs = len(eng._programs)
    # all ones: the step without weights, from the same program
    model.style_layer_weights = [1.0] * 5
    ones = _eval(model, x, sw, cw)
    assert all(torch.equal(p, q) for p, q in zip(ones, base, strict=True))
    assert len(eng._programs) == n_programs and not eng._heads
    # all 2.0 with style_w / 2: power-of-two scalings are exact
    model.style_layer_weights = [2.0] * 5
    s2, c2, t2, g2 = _eval(model, x, sw / 2, cw)
    assert len(eng._programs) == n_programs + 1
    assert torch.equal(t2, base[2]) and torch.equal(g2, base[3]) and torch.equal(c2, base[1])
    assert torch.equal(s2, base[0] * 2) and float(s2) > 0
    # (1, 0, 0, 0, 0): the first per-layer loss, as forward() returns it
    model.style_layer_weights = None
    per_layer, _ = model(x)
    first = per_layer[0].detach().clone()
    assert first.dtype == torch.float32
    model.style_layer_weights = [1, 0, 0, 0, 0]
    s1, _, _, g1 = _eval(model, x, sw, cw)
    assert torch.equal(s1, first), f"{float(s1)!r} against {float(first)!r}"
    assert torch.isfinite(g1).all() and not torch.equal(g1, base[3])
    # forward() keeps returning the unweighted losses while weights are set
    again, _ = model(x)
    assert all(torch.equal(p.detach(), q.detach()) for p, q in zip(again, per_layer, strict=True))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_weight_tuple_then_none_then_the_tuple_again(precision, monkeypatch):
    """Each program's own bits come back: the weighted and the unweighted step share nothing they should not."""
    case = _case(monkeypatch)
    sw, cw = float(case.meta["style_w"]), float(case.meta["content_w"])
    a, b, content, x = _images()
    model = _new_model(case, precision)
    model.set_targets([a, b], content, style_blend=list(BLEND))
    base = _eval(model, x, sw, cw)
    model.style_layer_weights = list(LAYER_W)
    weighted = _eval(model, x, sw, cw)
    assert not torch.equal(weighted[0], base[0]) and not torch.equal(weighted[3], base[3]) and torch.equal(weighted[1], base[1])
    model.style_layer_weights = None
    assert all(torch.equal(p, q) for p, q in zip(_eval(model, x, sw, cw), base, strict=True))
    model.style_layer_weights = list(LAYER_W)
    assert all(torch.equal(p, q) for p, q in zip(_eval(model, x, sw, cw), weighted, strict=True))
    tv = _eval_tv(model, x, sw, cw)
    model.style_layer_weights = None
    assert torch.equal(_eval_tv(model, x, sw, cw)[1], base[1]) and not torch.equal(_eval_tv(model, x, sw, cw)[0], tv[0])
    assert torch.equal(tv[0], weighted[0]) and torch.equal(tv[1], weighted[1])       # the TV row leaves the weighted scores alone


def _eval_tv(model, x, sw, cw):
    s, c, t = model.loss_and_grad(x, sw, cw, tv_w=50.0)
    return s.clone(), c.clone(), t.clone()


# ---- layer weights, against the oracle ------------------------------------------------------------------------------------------------

def _weighted_oracle(oracle, x0, sw, cw, tap_w):
    with torch.enable_grad():
        xr = x0.detach().clone().requires_grad_(True)
        s_losses, c_losses = oracle(xr)
        style = sum(w * term for w, term in zip(tap_w, s_losses, strict=True))
        total = sw * style + cw * torch.stack(c_losses).sum()
        total.backward()
    return style.detach(), total.detach(), xr.grad.detach()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_weighted_step_against_the_oracle(precision, monkeypatch):
    case = _case(monkeypatch)
    m = case.meta
    sw, cw = float(m["style_w"]), float(m["content_w"])
    content, style = case.images()
    x0 = case.tensor("x0")
    name = f"vgg19_white_lbfgs {precision} layer weights {LAYER_W}"
    model = _new_model(case, precision, list(LAYER_W))
    model.set_targets(style.to(DEV), content.to(DEV))
    xd = x0.to(DEV).requires_grad_(True)
    s, _, t, g = _eval(model, xd, sw, cw)
    d_hip = pu.hip_decisions(model)
    # the style score against forward()'s unweighted per-layer losses
    per_layer, _ = model(xd)
    want = math.fsum(w * float(term.detach().double()) for w, term in zip(LAYER_W, per_layer, strict=True))
    ulp = float(np.spacing(np.float32(want)))
    print(f"{name}: style score {float(s)!r}, float64 sum of w_l * loss_l {want!r}, ulp {ulp:.3e}")
    record_parity(name, "style score vs sum w_l loss_l (ulp)", abs(float(s) - want) / ulp, 2.0, "forward()'s fp32 losses, float64 sum")
    assert abs(float(s) - want) <= 2 * ulp
    # the gradient against the CPU oracle, its per-layer losses weighted here
    oracle = ocm.OracleModel(ocm.vgg_program(case.weights(), case.cfg), m["style_layers"], m["content_layers"])
    oracle.set_targets(style, content)
    s_ref, t_ref, g_ref = _weighted_oracle(oracle, x0, sw, cw, LAYER_W)
    gscale = float(g_ref.abs().max())
    dev = float((g.cpu() - g_ref).abs().max()) / gscale
    print(f"{name}: gradient error {dev:.3e} of scale, total {float(t)!r} against {float(t_ref)!r}")
    if precision == "bf16":
        record_parity(name, "gradient vs fp32 oracle (of scale)", dev, 0.1)
        assert float(t) == pytest.approx(float(t_ref), rel=5e-2)
        assert dev < 0.1, f"bf16 gradient drifted {dev:.3f} of scale"
        return
    assert float(s) == pytest.approx(float(s_ref), rel=2e-4) and float(t) == pytest.approx(float(t_ref), rel=2e-4)
    if dev <= 2e-4:
        record_parity(name, "gradient vs oracle (of scale)", dev, 2e-4)
        return
    nl = pu.n_program_layers(m["style_layers"], m["content_layers"])
    d_cpu = pu.oracle_decisions(oracle.program, x0, nl)
    flips = pu.count_flips(d_hip, d_cpu)
    prog64 = ocm.vgg_program([(w.double(), b.double()) for w, b in case.weights()], case.cfg)
    gap = pu.flip_gaps(d_hip, d_cpu, prog64, x0.double(), nl)
    _, _, g_locked = _weighted_oracle(pu.lock(oracle, d_hip), x0, sw, cw, LAYER_W)
    dev_locked = float((g.cpu() - g_locked).abs().max()) / gscale
    record_parity(name, "gradient vs oracle on the HIP path's branch (of scale)", dev_locked, 2e-4,
                  f"plain comparison {dev:.1e}: {flips} ReLU/pool decision(s) differ, float64 gap <= {gap:.1e} of the layer rms")
    assert 0 < flips <= 16 and gap < 1e-5, f"{name}: {flips} decisions differ, largest float64 gap {gap:.2e}"
    assert dev_locked <= 2e-4, f"{name}: gradient differs by {dev_locked:.2e} of scale on the same branch"


# ---- runs -----------------------------------------------------------------------------------------------------------------------

def _run(monkeypatch, precision: str, steps: int, *, layer_w, env: dict | None = None, log_loss=None):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    case = _case(monkeypatch)
    m = case.meta
    cfg = stv_config.StyleTransferConfig.model_validate({})
    oc = cfg.optimization
    oc.steps, oc.style_w, oc.content_w = steps, m["style_w"], m["content_w"]
    oc.init_method = "content"
    oc.style_layers, oc.content_layers = list(m["style_layers"]), list(m["content_layers"])
    oc.normalize = m["normalize"]
    oc.style_blend, oc.style_layer_weights = list(BLEND), layer_w
    cfg.hardware.precision = precision
    cfg.output.log_every = 1
    cfg.output.log_loss = str(log_loss) if log_loss is not None else None
    cfg.video.create_video = False
    a, b, content, _ = _images()
    torch.manual_seed(0)
    model, input_img, opt = core_model.prepare_model_and_input(content, [a, b], DEV, oc, precision=precision)
    runner = optimization.OptimizationRunner(model, input_img, cfg, optimizer=opt, progress_bar=_Bar())
    img, hist, _ = runner.run()
    torch.cuda.synchronize()
    for k in (env or {}):
        monkeypatch.delenv(k)
    return img.detach().clone(), hist, runner, model


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_graph_replay_equals_eager_launches_of_the_weighted_step(precision, monkeypatch):
    xg, hg, rg, _ = _run(monkeypatch, precision, 5, layer_w=list(LAYER_W))
    xe, he, re_, _ = _run(monkeypatch, precision, 5, layer_w=list(LAYER_W), env={"STV_HIP_GRAPH": "0"})
    x0, h0, _, _ = _run(monkeypatch, precision, 5, layer_w=None)
    assert isinstance(rg.optimizer, HipLBFGS) and isinstance(re_.optimizer, HipLBFGS)
    assert torch.equal(xg, xe), f"max |diff| {float((xg - xe).abs().max()):.3e}"
    assert hg == he and all(len(v) == 5 for v in hg.values())
    assert not torch.equal(xg, x0) and hg["style_loss"][0] != h0["style_loss"][0] and hg["content_loss"][0] == h0["content_loss"][0]


def test_five_steps_with_two_styles_and_layer_weights(monkeypatch, tmp_path, blend_calls):
    log = tmp_path / "loss.csv"
    img, hist, runner, model = _run(monkeypatch, "fp32", 5, layer_w=list(LAYER_W), log_loss=log)
    assert len(blend_calls) == 5 and hist == {}                               # (CSV mode keeps no history)
    with log.open(newline="") as fh:
        rows = list(csv.DictReader(fh))
    assert [int(r["step"]) for r in rows] == [1, 2, 3, 4, 5]
    totals = [float(r["total_loss"]) for r in rows]
    assert all(math.isfinite(v) for r in rows for v in map(float, r.values()))
    assert all(later < earlier for earlier, later in zip(totals, totals[1:])), totals
    # step 1 is evaluated at the content image: the CSV's style column is the weighted score of that evaluation
    a, b, content, _ = _images()
    at = content.clone().requires_grad_(True)
    s, c, t, _ = _eval(model, at, runner.config.optimization.style_w, runner.config.optimization.content_w)
    assert float(rows[0]["style_loss"]) == float(s) and float(rows[0]["content_loss"]) == float(c) and totals[0] == float(t)
    per_layer, _ = model(at)
    want = math.fsum(w * float(term.detach().double()) for w, term in zip(LAYER_W, per_layer, strict=True))
    plain = math.fsum(float(term.detach().double()) for term in per_layer)
    assert abs(float(s) - want) <= 2 * float(np.spacing(np.float32(want))) and abs(plain - want) > 1e-3 * want
    assert torch.isfinite(img).all() and not torch.equal(img, content)


# ---- main.style_transfer ----------------------------------------------------------------------------------------------------------

SIZES = {"content": (128, 128), "style": (136, 128), "other": (150, 200)}


def _pngs(root) -> dict:
    paths = {}
    for seed, (name, (H, W)) in enumerate(SIZES.items()):
        img = synthetic.synthetic_image(seed, H, W, normalize=False)[0].permute(1, 2, 0).mul(255).byte().numpy()
        paths[name] = str(root / f"{name}.png")
        Image.fromarray(img).save(paths[name])
    return paths


def _main_cfg(out_dir, **oc_fields):
    cfg = stv_config.StyleTransferConfig.model_validate({})
    oc = cfg.optimization
    oc.steps, oc.init_method, oc.seed = 4, "random", 0
    for k, v in oc_fields.items():
        setattr(oc, k, v)
    cfg.hardware.device, cfg.hardware.precision = "cuda", "fp32"
    cfg.video.create_video, cfg.video.final_only = False, True
    cfg.output.output, cfg.output.plot_losses, cfg.output.log_every = str(out_dir), False, 1
    return cfg


def test_main_with_two_styles_equals_the_stages_composed_by_hand(tmp_path, monkeypatch, blend_calls):
    monkeypatch.setenv("STV_SYNTHETIC_WEIGHTS", "0")
    p = _pngs(tmp_path)
    fields = dict(style_scale=1.5, preserve_color="match", pyramid_levels=2, style_blend=[0.7, 0.3],
                  style_layer_weights=[1, 0.8, 0.5, 0.3, 0.1])
    seen = []
    real_targets = core_model.StyleContentModel.set_targets

    def set_targets(self, style_img, content_img, **kw):
        seen.append(([s.detach().clone() for s in style_img], kw, self.style_layer_weights))
        return real_targets(self, style_img, content_img, **kw)
    monkeypatch.setattr(core_model.StyleContentModel, "set_targets", set_targets)
    out = main.style_transfer(InputPaths(p["content"], p["style"], (p["other"],)), _main_cfg(tmp_path / "out", **fields)).clone()
    torch.cuda.synchronize()
    (png,) = list((tmp_path / "out").glob("stylized_*.png"))
    assert png.name == "stylized_content_x_style+other.png" and len(blend_calls) == 10      # five layers, two levels
    # by hand: load, resize each style to its own longer side of round(1.5 * 128) = 192, match each, run the levels
    cfg = _main_cfg(tmp_path / "hand", **fields)
    oc = cfg.optimization
    content = image_io.load_image_to_tensor(p["content"], DEV, normalize=True)
    styles = []
    for key, want_hw in (("style", (192, 181)), ("other", (144, 192))):
        img = image_io.load_image_to_tensor(p[key], DEV, normalize=True)
        _, hw = resize_rules.plan_sizes(oc, content.shape[-2:], img.shape[-2:])
        assert hw == want_hw
        styles.append(color.match_style_to_content(ops.resize(img.contiguous(), hw, oc.resize_filter), content))
    fine = [styles[0][..., :192, :180], styles[1]]
    coarse = [ops.resize2x(s.contiguous(), _lib.RESIZE_DOWN2) for s in fine]
    assert len(seen) == 2
    for (got_styles, kw, lw), want_styles in zip(seen, (coarse, fine), strict=True):
        assert kw == {"style_blend": [0.7, 0.3]} and lw == (1.0, 0.8, 0.5, 0.3, 0.1)
        assert all(torch.equal(g, w) for g, w in zip(got_styles, want_styles, strict=True))
    monkeypatch.setattr(core_model.StyleContentModel, "set_targets", real_targets)
    by_hand, _, _ = pyramid.run_pyramid(content, styles, DEV, cfg, seed=oc.seed, progress_bar=_Bar())
    torch.cuda.synchronize()
    assert torch.equal(out, by_hand.detach().clamp(0, 1)), f"max |diff| {float((out - by_hand.detach().clamp(0, 1)).abs().max()):.3e}"
    assert tuple(out.shape) == (1, 3, 128, 128) and torch.isfinite(out).all()
    runtime.save_outputs(by_hand, {}, tmp_path / "hand", 0.0, main.SaveOptions(
        content_name="content", style_name="twin", normalize=True, video_created=False, plot_losses=False))
    assert np.array_equal(np.array(Image.open(png)), np.array(Image.open(tmp_path / "hand" / "stylized_content_x_twin.png")))
    # ... and the mix did change the picture
    single = main.style_transfer(InputPaths(p["content"], p["style"]), _main_cfg(
        tmp_path / "single", style_scale=1.5, preserve_color="match", pyramid_levels=2))
    assert not torch.equal(single, out)


def test_a_run_with_only_defaults_is_the_run_without_the_options(tmp_path, monkeypatch, blend_calls):
    monkeypatch.setenv("STV_SYNTHETIC_WEIGHTS", "0")
    p = _pngs(tmp_path)
    seen = []
    real_targets = core_model.StyleContentModel.set_targets

    def set_targets(self, style_img, content_img):          # the two-argument form: a run with defaults passes nothing more
        seen.append(style_img)
        return real_targets(self, style_img, content_img)
    monkeypatch.setattr(core_model.StyleContentModel, "set_targets", set_targets)
    old = main.style_transfer(InputPaths(p["content"], p["style"]), _main_cfg(tmp_path / "old")).clone()
    new = main.style_transfer(InputPaths(content_path=p["content"], style_path=p["style"], extra_style_paths=()),
                              _main_cfg(tmp_path / "new", style_blend=None, style_layer_weights=None)).clone()
    ones = main.style_transfer(InputPaths(p["content"], p["style"]),
                               _main_cfg(tmp_path / "ones", style_layer_weights=[1, 1, 1, 1, 1])).clone()
    torch.cuda.synchronize()
    assert blend_calls == [] and len(seen) == 3 and all(isinstance(s, torch.Tensor) for s in seen)
    assert torch.equal(old, new) and torch.equal(old, ones)
    names = [sorted(q.name for q in (tmp_path / d).iterdir()) for d in ("old", "new", "ones")]
    assert names[0] == names[1] == names[2] == ["stylized_content_x_style.png"]
    data = [(tmp_path / d / "stylized_content_x_style.png").read_bytes() for d in ("old", "new", "ones")]
    assert data[0] == data[1] == data[2]
