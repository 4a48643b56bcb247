"""Average pooling (``pooling="avg"``) through the whole step on a real MI355X: 64x64 and 70x52 (35 -> 17, 13 -> 6: odd maps whose
last row / column the pools drop), the synthetic VGG19 of the fixture-size tests.

* Wiring, bit for bit, in fp32, bf16 and bf16x3: after one step every average pool's output equals the twin of its stored input,
  and what it leaves in its input's gradient equals the twin of its output's gradient under the node's flags.
* The fp32 step against the float64 definition (tests/avgpool_ref.py), for the default layers and for ``[0, 2, 5]`` - the layout
  in which a pool meets a pending ReLU and has to take it itself.
* The bf16 step against the fp32 step, held to twice what max pooling's own bf16 step deviates from its fp32 step.
* The existing guidance identity with average pools; the optimisers; a 2-level pyramid run and the other style controls from the
  command line; and ``pooling="max"`` against a model built without the keyword.
"""
from __future__ import annotations

import math

import pytest
import torch

from style_transfer_visualizer_amd import core_model, synthetic
from tests import avgpool_ref as ref
from tests.conftest import GoldenCase, record_parity

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SIZES = [(64, 64), (70, 52)]
PRECISIONS = ["fp32", "bf16", "bf16x3"]
LAYOUTS = {"default": ([0, 5, 10, 19, 28], [21]), "0-2-5": ([0, 2, 5], [7])}
UNFUSED = {"STV_FUSE_GRAM": "0", "STV_FUSE_GRAM_FIRST": "0"}
OWN_GRADS = {"STV_GRAD_ARENA": "0"}


def _model(monkeypatch, precision, hw, *, layout="default", env=None, **kw):
    """Model with targets set, an image with ``requires_grad`` and one evaluated step.  ``env`` holds only while the engine is
    built (the switches are read then).  ``kw``: the model's keywords (``pooling``, ``guide_regions``, ...)."""
    case = GoldenCase("vgg19_white_lbfgs")
    m = case.meta
    w = case.weights()
    monkeypatch.setattr(core_model, "initialize_vgg", lambda: core_model.build_vgg_features(w, case.cfg).eval())
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    H, W = hw
    style_at, content_at = LAYOUTS[layout]
    labels = kw.pop("labels", None)
    model = core_model.StyleContentModel(list(style_at), list(content_at), precision=precision, **kw).to(DEV)
    lab = {"content_labels": labels, "style_labels": labels} if labels is not None else {}
    model.set_targets(synthetic.synthetic_image(1, H, W).to(DEV), synthetic.synthetic_image(0, H, W).to(DEV), **lab)
    x = synthetic.synthetic_image(2, H, W) + 0.25 * torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(5))
    x = x.to(DEV).requires_grad_(True)
    out = model.loss_and_grad(x, float(m["style_w"]), float(m["content_w"]))
    torch.cuda.synchronize()
    for k in (env or {}):
        monkeypatch.delenv(k)
    return model, x, float(m["style_w"]), float(m["content_w"]), out


def _engine(model):
    (eng,) = model._engines.values()
    return eng


def _pools(eng):
    return [nd for nd in eng.sched.nodes if nd.kind == "avgpool"]


# ---- wiring, bit for bit ---------------------------------------------------------------------------------------------------------

def _check_forward(eng):
    pools = _pools(eng)
    assert pools and not any(nd.kind == "pool" for nd in eng.sched.nodes)
    for nd in pools:
        assert nd.src.stored and not nd.fused and nd.idx is None
        want = ref.fwd(nd.src.act.cpu(), relu_in=nd.relu_in)
        assert torch.equal(nd.dst.act.cpu(), want), f"output of the pool at layer {nd.layer}"
        assert float(want.float().abs().max()) > 0
    return pools


def _check_backward(nd):
    s, d = nd.src, nd.dst
    mask = nd.relu_in or (s.relu_fused and not s.taps)
    want = ref.bwd(d.grad.cpu(), s.H, s.W, ref=s.act.cpu() if mask else None)
    assert torch.equal(s.grad.cpu(), want), f"gradient in front of the pool at layer {nd.layer}"
    assert float(want.float().abs().max()) > 0
    if s.H % 2:
        assert float(s.grad[-1].float().abs().max()) == 0
    if s.W % 2:
        assert float(s.grad[:, -1].float().abs().max()) == 0


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("hw", SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_average_pool_equals_the_twin_in_both_directions(precision, hw, layout, monkeypatch):
    model, x, sw, cw, (style, content, total) = _model(monkeypatch, precision, hw, layout=layout, pooling="avg", env=OWN_GRADS)
    eng = _engine(model)
    assert eng.pooling == "avg" and math.isfinite(float(total)) and float(x.grad.abs().max()) > 0
    pools = _check_forward(eng)
    assert len(pools) == (4 if layout == "default" else 1)
    shared = [nd for nd in pools if nd.src.taps]          # a tap's term accumulates onto the pool's: compared in a second run
    for nd in pools:
        if nd not in shared:
            _check_backward(nd)
    if layout == "0-2-5":
        (nd,) = shared
        assert nd.relu_in and nd.layer == 4 and [t.kind for t in nd.src.taps] == ["style"]
        # the same step with that tap's weight at 0: its seed is zero, F . 0 adds nothing, and the pool's term stands alone
        quiet, xq, _, _, _ = _model(monkeypatch, precision, hw, layout=layout, pooling="avg", env=OWN_GRADS,
                                    style_layer_weights=[1.0, 0.0, 1.0])
        (nq,) = [n for n in _pools(_engine(quiet)) if n.layer == 4]
        assert torch.equal(nq.dst.act.cpu(), nd.dst.act.cpu())
        _check_backward(nq)
        assert not torch.equal(nq.src.grad, nd.src.grad)          # (the tap's term is there in the first run)
    else:
        assert not shared


# ---- fp32 against the float64 definition ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("hw", SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_fp32_step_against_the_float64_definition(hw, layout, monkeypatch):
    """Bounds: the ones the unguided max-pooling step is held to - scores relative 2e-4, gradient 2e-4 of its maximum -, the
    reference evaluated on the ReLU branch the HIP path took (tests/parity_util.py), as the guided step's test does."""
    from tests import parity_util as pu
    case = GoldenCase("vgg19_white_lbfgs")
    model, x, sw, cw, (style, content, total) = _model(monkeypatch, "fp32", hw, layout=layout, pooling="avg")
    w64 = [(w.double(), b.double()) for w, b in case.weights()]
    r = ref.Reference(ref.program(w64, case.cfg), *LAYOUTS[layout])
    r.set_targets(synthetic.synthetic_image(1, *hw).double(), synthetic.synthetic_image(0, *hw).double())
    s_ref, c_ref, t_ref, g_ref = r.locked(pu.hip_decisions(model)).loss_and_grad(x.detach().cpu().double(), sw, cw)
    name = f"avg pooling fp32 {hw[0]}x{hw[1]} {layout}"
    for what, got, want in (("style score", style, s_ref), ("content score", content, c_ref), ("total", total, t_ref)):
        dev = abs(float(got) - float(want)) / abs(float(want))
        print(f"{name}: {what} {float(got)!r} against {float(want)!r}: relative {dev:.3e}")
        record_parity(name, f"{what} vs float64 definition (rel)", dev, 2e-4)
        assert dev <= 2e-4, what
    gdev = float((x.grad.cpu().double() - g_ref).abs().max() / g_ref.abs().max())
    print(f"{name}: gradient, largest deviation {gdev:.3e} of its maximum")
    record_parity(name, "gradient vs float64 definition on the HIP path's branch (of scale)", gdev, 2e-4)
    assert gdev <= 2e-4


# ---- forward(), the autograd path ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_forward_and_autograd_backward_against_the_float64_definition(layout, monkeypatch):
    """``model(x)`` with ``pooling="avg"`` at 64x64, the weighted sum formed by torch, ``.backward()``: the engine's forward
    program and its reverse program with upstream coefficients run the two average-pool ops (for ``[0, 2, 5]`` with the ReLU the
    pool takes).  Per-layer losses, scores and gradient against the float64 definition on the HIP path's ReLU branch at the bounds
    the autograd path is held to (tests/test_gpu_surface.py: 2e-4, gradient of its maximum), and against ``loss_and_grad`` of the
    same model at the same bound."""
    from style_transfer_visualizer_amd import _lib
    from tests import parity_util as pu
    hw = (64, 64)
    case = GoldenCase("vgg19_white_lbfgs")
    model, x, sw, cw, (s_fused, c_fused, t_fused) = _model(monkeypatch, "fp32", hw, layout=layout, pooling="avg")
    g_fused = x.grad.detach().clone()
    x.grad = None
    style, content = model(x)
    assert len(style) == len(LAYOUTS[layout][0]) and len(content) == len(LAYOUTS[layout][1])
    total = sw * torch.stack(style).sum() + cw * torch.stack(content).sum()
    total.backward()
    torch.cuda.synchronize()
    eng = _engine(model)
    progs = {k[0]: p for k, p in eng._programs.items() if k[0] in ("fwd", "bwd")}
    kinds = {name: [m[0] for m in p.op_meta] for name, p in progs.items()}
    n_pools = len(_pools(eng))
    assert kinds["fwd"].count(_lib.OP_AVGPOOL_FWD) == n_pools and kinds["bwd"].count(_lib.OP_AVGPOOL_BWD) == n_pools
    assert _lib.OP_POOL_FWD not in kinds["fwd"] and _lib.OP_POOL_BWD not in kinds["bwd"]
    if layout == "0-2-5":          # the pool behind conv1_2 takes the pending ReLU in both directions
        (f,) = [fl for m, fl in zip(progs["fwd"].op_meta, progs["fwd"].op_flags, strict=True) if m[0] == _lib.OP_AVGPOOL_FWD]
        (b,) = [fl for m, fl in zip(progs["bwd"].op_meta, progs["bwd"].op_flags, strict=True) if m[0] == _lib.OP_AVGPOOL_BWD]
        assert f == _lib.RELU_IN and b & _lib.MASK
    w64 = [(w.double(), b.double()) for w, b in case.weights()]
    r = ref.Reference(ref.program(w64, case.cfg), *LAYOUTS[layout])
    r.set_targets(synthetic.synthetic_image(1, *hw).double(), synthetic.synthetic_image(0, *hw).double())
    locked = r.locked(pu.hip_decisions(model))
    xc = x.detach().cpu().double()
    s_each, c_each = locked.losses(xc)
    s_ref, c_ref, t_ref, g_ref = locked.loss_and_grad(xc, sw, cw)
    name = f"avg pooling forward() fp32 64x64 {layout}"
    worst = max(abs(float(got) - float(want)) / abs(float(want)) for got, want in zip(list(style) + list(content), s_each + c_each, strict=True))
    print(f"{name}: per-layer losses, largest relative deviation {worst:.3e}")
    record_parity(name, "per-layer losses vs float64 definition (rel, max)", worst, 2e-4)
    assert worst <= 2e-4
    tdev = abs(float(total) - float(t_ref)) / abs(float(t_ref))
    record_parity(name, "total vs float64 definition (rel)", tdev, 2e-4)
    assert tdev <= 2e-4
    gdev = float((x.grad.cpu().double() - g_ref).abs().max() / g_ref.abs().max())
    print(f"{name}: gradient, largest deviation {gdev:.3e} of its maximum")
    record_parity(name, "autograd gradient vs float64 definition on the HIP path's branch (of scale)", gdev, 2e-4)
    assert gdev <= 2e-4
    # the fused step of the same model: the same kernels in another schedule
    assert float(torch.stack(style).sum()) == pytest.approx(float(s_fused), rel=2e-4)
    assert float(torch.stack(content).sum()) == pytest.approx(float(c_fused), rel=2e-4)
    fdev = float((x.grad - g_fused).abs().max() / g_fused.abs().max())
    record_parity(name, "autograd gradient vs loss_and_grad (of scale)", fdev, 2e-4)
    assert fdev <= 2e-4


# ---- bf16 against fp32 ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_bf16_step_tracks_fp32_at_least_as_well_as_max_pooling_does(hw, monkeypatch):
    """No number of the project's applies to this step, so the yardstick is measured here: the max-pooling step's own
    bf16-against-fp32 gradient deviation (relative rms) at the same size, weights and image.  The average has no arg-max to flip,
    so its deviation should be the lower one; the factor of two only guards against a wiring error, which shows at order one."""
    dev = {}
    for pooling in ("max", "avg"):
        grads = {}
        for precision in ("fp32", "bf16"):
            _, x, _, _, (_, _, total) = _model(monkeypatch, precision, hw, pooling=pooling)
            assert math.isfinite(float(total))
            grads[precision] = x.grad.detach().double().cpu()
        dev[pooling] = float((grads["bf16"] - grads["fp32"]).norm() / grads["fp32"].norm())
    name = f"pooling bf16 vs fp32 {hw[0]}x{hw[1]}"
    print(f"{name}: gradient rel rms, max pooling {dev['max']:.3e}, avg pooling {dev['avg']:.3e} (bound {2 * dev['max']:.3e})")
    record_parity(name, "max pooling: gradient bf16 vs fp32 (rel rms)", dev["max"], float("nan"), "the yardstick, measured")
    record_parity(name, "avg pooling: gradient bf16 vs fp32 (rel rms)", dev["avg"], 2 * dev["max"], "2 x max pooling's")
    assert 0 < dev["avg"] <= 2 * dev["max"]


# ---- guidance ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_one_region_is_the_unguided_average_pooling_step_bit_for_bit(precision, hw, monkeypatch):
    """The guidance identity (tests/test_gpu_guidance_model.py) on a stack of average pools: the tap label maps are sized by
    counting the pools of the stack, of either type."""
    plain, xp, _, _, (s0, c0, t0) = _model(monkeypatch, precision, hw, pooling="avg", env=UNFUSED)
    g0 = xp.grad.clone()
    guided, xg, _, _, (s1, c1, t1) = _model(monkeypatch, precision, hw, pooling="avg", guide_regions=1,
                                            labels=torch.zeros(hw, dtype=torch.uint8))
    assert torch.equal(xp, xg) and float(s0) > 0 and float(g0.abs().max()) > 0
    for tp, tg in zip(plain.style_targets, guided.style_targets, strict=True):
        assert torch.equal(tg[0], tp)
    assert torch.equal(s1, s0) and torch.equal(c1, c0) and torch.equal(t1, t0)
    assert torch.equal(xg.grad, g0), f"max |diff| {float((xg.grad - g0).abs().max()):.3e}"
    assert _engine(guided).pooling == "avg" and len(_pools(_engine(guided))) == 4


# ---- the default path ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_pooling_max_is_the_model_without_the_keyword(precision, monkeypatch):
    hw = (70, 52)
    plain, xp, _, _, out_p = _model(monkeypatch, precision, hw)
    given, xg, _, _, out_g = _model(monkeypatch, precision, hw, pooling="max")
    assert all(torch.equal(p, q) for p, q in zip(out_p, out_g, strict=True)) and torch.equal(xp.grad, xg.grad)
    assert list(plain._engines) == list(given._engines) == [(70, 52, xp.device.index)]
    def keys(model):          # (without the addresses of the image and its gradient)
        return [(k[0], *k[3:]) for k in _engine(model)._programs]
    assert keys(plain) == keys(given) and not any("pooling" in str(k) for k in keys(given))
    avg, xa, sw, cw, out_a = _model(monkeypatch, precision, hw, pooling="avg")
    assert not torch.equal(out_a[0], out_p[0]) and not torch.equal(xa.grad, xp.grad)
    assert list(avg._engines) == [(70, 52, xa.device.index, ("pooling", "avg"))]
    assert all(("pooling", "avg") in key for key in _engine(avg)._programs if key[0] == "fused")
    # graph replay equals the first (eager, capturing) evaluations
    first = xa.grad.clone()
    for _ in range(2):
        again = avg.loss_and_grad(xa, sw, cw)
        assert all(torch.equal(p, q) for p, q in zip(out_a, again, strict=True)) and torch.equal(xa.grad, first)
    eager, xe, _, _, out_e = _model(monkeypatch, precision, hw, pooling="avg", env={"STV_HIP_GRAPH": "0"})
    assert torch.equal(xe.grad, first) and all(torch.equal(p, q) for p, q in zip(out_a, out_e, strict=True))


# ---- the optimisers --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["lbfgs", "adam"])
def test_ten_optimiser_steps_lower_the_total(which, monkeypatch):
    from style_transfer_visualizer_amd.optimizers import HipAdam, HipLBFGS
    model, x, sw, cw, (_, _, start) = _model(monkeypatch, "bf16", (64, 64), pooling="avg")
    opt = HipLBFGS([x], lr=1.0) if which == "lbfgs" else HipAdam([x], lr=2e-2)
    totals = [float(start)]

    def closure():
        _, _, total = model.loss_and_grad(x, sw, cw)
        return total
    for _ in range(10):
        loss = opt.step(closure)
        totals.append(float(loss))
    _, _, end = model.loss_and_grad(x, sw, cw)
    torch.cuda.synchronize()
    totals.append(float(end))
    print(f"avg pooling, ten {which} steps: total {totals[0]:.6g} -> {totals[-1]:.6g}")
    assert all(math.isfinite(v) for v in totals) and totals[-1] < totals[0]


# ---- end to end ------------------------------------------------------------------------------------------------------------------------

CLI_VARIANTS = {
    "pyramid": ["--pyramid-levels", "2", "--steps", "8"],
    "tv_lap_color_two_styles_pyramid": ["--tv-w", "10", "--lap-w", "100", "--preserve-color", "luma", "--style-also", "STYLE2",
                                        "--pyramid-levels", "2", "--steps", "8"],
    "masks": ["--content-mask", "MASK", "--style-mask", "MASK", "--steps", "4"],
}


@pytest.mark.parametrize("variant", list(CLI_VARIANTS))
def test_cli_with_pooling_avg(variant, tmp_path, monkeypatch):
    """``--pooling avg`` from the command line, through ``main.style_transfer``: a 2-level pyramid run, the same together with
    ``--tv-w``, ``--lap-w``, ``--preserve-color`` and ``--style-also``, and a guided run with two masks."""
    import csv

    from PIL import Image

    from style_transfer_visualizer_amd import cli
    from style_transfer_visualizer_amd.pyramid import HEADER
    monkeypatch.setenv("STV_SYNTHETIC_WEIGHTS", "0")
    for name, seed in (("content", 0), ("style", 1), ("style2", 3)):
        img = synthetic.synthetic_image(seed, 128, 128, normalize=False)[0].permute(1, 2, 0).mul(255).byte().numpy()
        Image.fromarray(img).save(tmp_path / f"{name}.png")
    mask = torch.zeros(128, 128, dtype=torch.uint8)
    mask[:, 64:] = 255
    Image.fromarray(mask.numpy()).save(tmp_path / "mask.png")
    subst = {"STYLE2": str(tmp_path / "style2.png"), "MASK": str(tmp_path / "mask.png")}
    out_dir, log = tmp_path / "out", tmp_path / "loss.csv"
    argv = ["--content", str(tmp_path / "content.png"), "--style", str(tmp_path / "style.png"), "--pooling", "avg",
            "--init-method", "content", "--device", "cuda", "--precision", "bf16", "--no-video", "--final-only", "--seed", "0",
            "--no-plot", "--log-loss", str(log), "--log-every", "1", "--output", str(out_dir),
            *[subst.get(a, a) for a in CLI_VARIANTS[variant]]]
    seen = []
    built = core_model.StyleContentModel.__init__

    def spy(self, *a, **kw):
        seen.append(kw.get("pooling"))
        built(self, *a, **kw)
    monkeypatch.setattr(core_model.StyleContentModel, "__init__", spy)
    cli.main(argv)
    assert seen and all(p == "avg" for p in seen), seen            # every level's model
    assert len(seen) == (1 if variant == "masks" else 2)
    (png,) = list(out_dir.glob("stylized_*.png"))
    assert Image.open(png).size == (128, 128)
    with log.open() as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == list(HEADER)
    total = [float(r[rows[0].index("total_loss")]) for r in rows[1:]]
    steps = int(CLI_VARIANTS[variant][-1])
    assert len(total) == steps and all(math.isfinite(v) for v in total)
    if variant == "masks":
        assert total[-1] < total[0]
    else:                                         # every level is a run of its own: decreasing inside a level
        assert total[3] < total[0] and total[7] < total[4]
    print(f"cli --pooling avg, {variant}: total loss {total[0]:.6g} -> {total[-1]:.6g}")
