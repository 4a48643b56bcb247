"""Several style images and per-layer style weights, everything that needs no GPU: the blend weights, the twin of the blend
kernel against float64, the argument checks of ``stv_gram_blend``, config / TOML / command line, the wiring of
``main.style_transfer`` and ``pyramid.run_pyramid`` with the stages replaced by recorders, and the op lists a GPU engine
builds with layer weights (``assume_device=True``: the step a GPU engine builds, on host tensors, never run)."""
from __future__ import annotations

import ctypes
import functools
import logging
import os
import re
from pathlib import Path

import numpy as np
import pytest
import torch
from torch import nn

from style_transfer_visualizer_amd import (_lib, cli, color, core_model, image_io, ops, optimization, plan, pyramid, runtime,
                                           spatial, style_mix)
from style_transfer_visualizer_amd import config as stv_config
from style_transfer_visualizer_amd import main as stv_main
from style_transfer_visualizer_amd.type_defs import InputPaths
from tests import blend_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
U = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ blend weights
def test_blend_weights_normalise_in_double_and_round_once():
    w = style_mix.blend_weights([7, 3], 2)
    assert w.dtype == np.float32 and w.tolist() == [float(np.float32(0.7)), float(np.float32(0.3))]
    assert style_mix.blend_weights((2, 2), 2).tolist() == [0.5, 0.5]
    assert style_mix.blend_weights(None, 4).tolist() == [0.25] * 4
    assert style_mix.blend_weights(None, 3).tolist() == [float(np.float32(1.0 / 3.0))] * 3
    assert style_mix.blend_weights([5.0], 1).tolist() == [1.0] and style_mix.blend_weights(None, 1).tolist() == [1.0]
    assert style_mix.blend_weights([1, 0], 2).tolist() == [1.0, 0.0]
    raw = [0.1, 0.2, 0.3, 0.05, 0.6, 1e-3, 4.0, 2.5]
    want = (np.asarray(raw, dtype=np.float64) / np.float64(sum(raw))).astype(np.float32)
    assert np.array_equal(style_mix.blend_weights(raw, 8), want)


@pytest.mark.parametrize("raw,k,text", [
    ([1.0, 2.0], 3, r"2 weights \[1\.0, 2\.0\] for 3 style images"),
    ([1.0, -2.0], 2, r"-2\.0"),
    ([1.0, float("nan")], 2, "nan"),
    ([float("inf"), 1.0], 2, "inf"),
    ([0.0, 0.0], 2, r"\[0\.0, 0\.0\]"),
    ([0.0], 1, r"\[0\.0\]"),
    (None, 9, "got 9"),
    (None, 0, "got 0"),
    ([1.0] * 9, 9, "got 9"),
    (["a", 1.0], 2, "'a'"),
])
def test_blend_weights_refusals_name_the_values(raw, k, text):
    with pytest.raises(ValueError, match=text):
        style_mix.blend_weights(raw, k)


@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_twin_stays_within_its_roundings_of_float64(K):
    rng = np.random.default_rng(K)
    stack = (rng.standard_normal((K, 4099)) * 3e-3).astype(np.float32)
    stack[:, ::5] = 0.0
    w = style_mix.blend_weights(rng.uniform(0.0, 1.0, K), K)
    twin, exact = blend_ref.blend(stack, w), blend_ref.blend_f64(stack, w)
    assert twin.dtype == np.float32 and twin.shape == (4099,)
    bound = (2 * K - 1) * U * blend_ref.magnitude(stack, w) + 2.0 ** -149       # (one subnormal step: underflow of a product)
    assert bool((np.abs(twin.astype(np.float64) - exact) <= bound).all())
    if K == 1:
        assert np.array_equal(twin, stack[0])


# ------------------------------------------------------------------------------------------------------- ABI
def test_library_exports_the_symbol_and_the_constants_match_the_header():
    lib = _lib.load()
    assert hasattr(lib, "stv_gram_blend") and "stv_gram_blend" in _lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "stv.h")).read()
    for name, value in (("MAX_TABLES", _lib.BLEND_MAX_TABLES), ("VEC", _lib.BLEND_VEC), ("THREADS", _lib.BLEND_THREADS),
                        ("MAX_BLOCKS", _lib.BLEND_MAX_BLOCKS)):
        assert int(re.search(rf"#define\s+STV_BLEND_{name}\s+(\d+)", header).group(1)) == value
    assert lib.stv_version() >= 110 and style_mix.MAX_STYLES == 8
    assert "STV_OP_GRAM_BLEND" not in header            # not an op of the step program


def test_bad_arguments_are_rejected_before_any_device_work():
    lib = _lib.load()
    S, O = 1 << 20, 1 << 22                             # never dereferenced: every call below is refused first
    w2 = (ctypes.c_float * 2)(0.5, 0.5)

    def w(*values):
        return (ctypes.c_float * len(values))(*values)
    assert lib.stv_gram_blend(None, O, w2, 2, 16, None) == 1
    assert lib.stv_gram_blend(S, None, w2, 2, 16, None) == 1
    assert lib.stv_gram_blend(S, O, None, 2, 16, None) == 1
    assert lib.stv_gram_blend(S, O, w2, 0, 16, None) == 1
    assert lib.stv_gram_blend(S, O, w2, -1, 16, None) == 1
    assert lib.stv_gram_blend(S, O, w(*[0.1] * 9), 9, 16, None) == 1
    assert lib.stv_gram_blend(S, O, w2, 2, 0, None) == 1
    assert lib.stv_gram_blend(S, O, w2, 2, -4, None) == 1
    assert lib.stv_gram_blend(S, O, w(0.5, -0.5), 2, 16, None) == 1
    assert lib.stv_gram_blend(S, O, w(0.5, float("nan")), 2, 16, None) == 1
    assert lib.stv_gram_blend(S, O, w(float("inf"), 0.5), 2, 16, None) == 1
    assert lib.stv_gram_blend(S, O, w(-0.0, float("-inf")), 2, 16, None) == 1
    assert lib.stv_gram_blend(S, O, w2, 2, 1 << 28, None) == 1                        # a stack of 2 GiB
    for delta in (0, 64, 2 * 16 * 4 - 4, -4, -(16 * 4 - 4)):
        assert lib.stv_gram_blend(S, S + delta, w2, 2, 16, None) == 1                 # out overlaps the stack


# ------------------------------------------------------------------------------------- config and command line
BASE = ["--content", "c.png", "--style", "s.png"]


def _cli_config(argv):
    return stv_config.build_config_from_cli(vars(cli.build_arg_parser().parse_args(argv)))


def test_config_defaults_round_trip_and_toml(tmp_path):
    cfg = stv_config.StyleTransferConfig.model_validate({})
    assert cfg.optimization.style_blend is None and cfg.optimization.style_layer_weights is None
    cfg.optimization.style_blend = [0.7, 0.3]
    cfg.optimization.style_layer_weights = [1, 0.8, 0.5, 0.3, 0.1]
    again = stv_config.StyleTransferConfig.model_validate(cfg.model_dump()).optimization
    assert again.style_blend == [0.7, 0.3] and again.style_layer_weights == [1.0, 0.8, 0.5, 0.3, 0.1]
    toml = tmp_path / "config.toml"
    toml.write_text("[optimization]\nstyle_blend = [7, 3]\nstyle_layer_weights = [1.0, 0.5, 0.25, 2.0, 0.0]\n")
    loaded = stv_config.ConfigLoader.load(str(toml)).optimization
    assert loaded.style_blend == [7.0, 3.0] and loaded.style_layer_weights == [1.0, 0.5, 0.25, 2.0, 0.0]
    over = stv_config.build_config_from_cli({"config": str(toml), "style_blend": "1,1"}).optimization
    assert over.style_blend == [1.0, 1.0] and over.style_layer_weights == [1.0, 0.5, 0.25, 2.0, 0.0]


def test_command_line_options():
    assert stv_config.parse_float_list("0.7,0.3") == [0.7, 0.3] and stv_config.parse_float_list([1.0]) == [1.0]
    with pytest.raises(ValueError):
        stv_config.parse_float_list("0.7,x")
    args = cli.build_arg_parser().parse_args([*BASE, "--style-also", "t.png", "u.png", "--style-blend", "0.7,0.2,0.1",
                                              "--style-layer-weights", "1,0.8,0.5,0.3,0.1"])
    assert args.style == "s.png" and args.style_also == ["t.png", "u.png"]
    oc = stv_config.build_config_from_cli(vars(args)).optimization
    assert oc.style_blend == [0.7, 0.2, 0.1] and oc.style_layer_weights == [1.0, 0.8, 0.5, 0.3, 0.1]
    plain = cli.build_arg_parser().parse_args(BASE)
    assert not hasattr(plain, "style_also")
    oc = _cli_config(BASE).optimization
    assert oc.style_blend is None and oc.style_layer_weights is None


def test_run_from_args_fills_the_extra_paths(monkeypatch):
    seen = {}
    monkeypatch.setattr(cli, "log_parameters", lambda *a: None)
    monkeypatch.setattr(stv_main, "style_transfer", lambda paths, cfg: seen.update(paths=paths, cfg=cfg))
    cli.main([*BASE, "--style-also", "t.png", "--style-blend", "3,1"])
    assert seen["paths"] == InputPaths("c.png", "s.png", ("t.png",)) and seen["paths"].style_paths == ("s.png", "t.png")
    assert seen["cfg"].optimization.style_blend == [3.0, 1.0]
    cli.main(BASE)
    assert seen["paths"] == InputPaths("c.png", "s.png") and seen["paths"].extra_style_paths == ()


def test_log_parameters_prints_the_mix_only_when_it_is_set(caplog):
    with caplog.at_level(logging.INFO):
        cli.log_parameters(InputPaths("c.png", "s.png"), _cli_config(BASE))
    assert "Style images" not in caplog.text and "Blend" not in caplog.text and "Layer Weights" not in caplog.text
    caplog.clear()
    with caplog.at_level(logging.INFO):
        cli.log_parameters(InputPaths("c.png", "s.png", ("t.png",)),
                           _cli_config([*BASE, "--style-blend", "3,1", "--style-layer-weights", "1,0.8,0.5,0.3,0.1"]))
    assert "Style images: ['s.png', 't.png']" in caplog.text
    assert "Style Blend Weights (normalised): [0.75, 0.25]" in caplog.text
    assert "Style Layer Weights: [1.0, 0.8, 0.5, 0.3, 0.1]" in caplog.text


# ------------------------------------------------------------------------------------------------ layer weights
def test_layer_weights_are_paired_by_position_and_sorted_with_the_layers():
    assert style_mix.tap_weights(None, [0, 5]) is None and style_mix.tap_weights([1, 1.0], [5, 0]) is None
    assert style_mix.tap_weights([0.5, 2.0, 1.0], [10, 0, 5]) == (2.0, 1.0, 0.5)
    assert style_mix.check_layer_weights([1, 1], [5, 0]) == (1.0, 1.0)
    assert style_mix.is_trivial(None) and style_mix.is_trivial([1, 1.0]) and not style_mix.is_trivial([1, 0.5])
    with pytest.raises(ValueError, match=r"3 weights \[1\.0, 2\.0, 3\.0\] for 5 style layers \[0, 5, 10, 19, 28\]"):
        style_mix.check_layer_weights([1, 2, 3], [0, 5, 10, 19, 28])
    with pytest.raises(ValueError, match=r"-1\.0"):
        style_mix.check_layer_weights([1, -1], [0, 5])
    with pytest.raises(ValueError, match="inf"):
        style_mix.check_layer_weights([1, float("inf")], [0, 5])
    with pytest.raises(ValueError, match=r"duplicates: \[0, 5, 0\]"):
        style_mix.check_layer_weights([1, 2, 3], [0, 5, 0])
    assert style_mix.check_layer_weights(None, [0, 5, 0]) is None           # duplicates alone stay accepted


@functools.cache
def _layers():
    return list(core_model.build_vgg_features().eval().children())


def test_model_takes_the_weights_at_construction_and_afterwards(monkeypatch):
    monkeypatch.setattr(core_model, "initialize_vgg", lambda: core_model.build_vgg_features().eval())
    with pytest.raises(ValueError, match=r"2 weights .* for 5 style layers"):
        core_model.StyleContentModel([0, 5, 10, 19, 28], [21], style_layer_weights=[1, 2])
    model = core_model.StyleContentModel([28, 0, 5, 10, 19], [21], style_layer_weights=[5, 1, 2, 3, 4])
    assert model.style_layer_weights == (5.0, 1.0, 2.0, 3.0, 4.0) and model.style_tap_weights() == (1.0, 2.0, 3.0, 4.0, 5.0)
    model.style_layer_weights = None
    assert model.style_layer_weights is None and model.style_tap_weights() is None
    model.style_layer_weights = [1, 1, 1, 1, 1]
    assert model.style_layer_weights == (1.0,) * 5 and model.style_tap_weights() is None
    with pytest.raises(ValueError, match="nan"):
        model.style_layer_weights = [1, 1, 1, 1, float("nan")]
    assert model.style_layer_weights == (1.0,) * 5                           # a refused assignment changes nothing
    assert core_model.StyleContentModel([0, 5], [21]).style_layer_weights is None
    with pytest.raises(ValueError, match="got 0"):
        model.set_targets([], torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError, match="got 9"):
        model.set_targets([torch.zeros(1, 3, 8, 8)] * 9, torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError, match=r"2 weights \[1\.0, 1\.0\] for 1 style image"):
        model.set_targets(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8), style_blend=[1, 1])
    with pytest.raises(ValueError, match=r"\[0\.0\]"):
        model.set_targets([torch.zeros(1, 3, 8, 8)], torch.zeros(1, 3, 8, 8), style_blend=[0])


class RecordedProgram:
    """Stands in for ``plan.Program`` under a host engine: keeps the op list it is given and runs nothing."""

    def __init__(self, op_list, extra=()):
        self.op_list = list(op_list)

    def run(self, use_graph=False):
        pass


def _host_engine(monkeypatch, dtype, H, W):
    monkeypatch.setattr(plan, "Program", RecordedProgram)
    eng = core_model._Engine(_layers(), [0, 5, 10, 19, 28], [21], H, W, dtype, CPU, assume_device=True)
    for tap in eng.sched.style_taps:
        tap.target = torch.zeros(tap.buf.C, tap.buf.C)
    for tap in eng.sched.content_taps:
        tap.target = torch.empty_like(tap.buf.act)
    return eng


def _step(eng, x, grad, **kw):
    before = set(eng._programs)
    eng.loss_and_grad(x, grad, STYLE_W, 1.0, **kw)
    (key,) = set(eng._programs) - before
    return key, eng._programs[key].op_list


STYLE_W = 1e5 / 3.0            # (not a power of two: style_w * w_l rounds)
_FIELDS = ("op", "dtype", "flags", "taps", "H", "W", "cin", "cout", "n", "f0", "f1", "f2", "f3",
           "p0", "p1", "p2", "p3", "q0", "q1", "q2", "q3")


def _fp32(v: float) -> float:
    return float(np.float32(v))


def _seed_coefs(op_list, eng) -> dict[int, float]:
    """channels-of-the-tap -> seed coefficient, from the finish ops and the batched Gram op's tap array."""
    found = {}
    for o in op_list:
        if o.op == _lib.OP_GRAM_FINISH and o.q2:
            found[int(o.cin), int(o.n)] = o.f2
        elif o.op == _lib.OP_GRAM_MULTI:
            taps = ctypes.cast(o.p0, ctypes.POINTER(_lib.StvGramTap))
            for i in range(int(o.n)):
                if taps[i].sgrad:
                    found[int(taps[i].channels), int(taps[i].n_pixels)] = taps[i].coef
    by_tap = {}
    for tap in eng.sched.style_taps:
        by_tap[tap.order] = found[int(tap.buf.C), int(tap.buf.H * tap.buf.W)]
    return by_tap


@pytest.mark.parametrize("dtype,H,W", [(torch.bfloat16, 64, 64), (torch.float32, 48, 80)])
def test_op_lists_with_and_without_layer_weights(monkeypatch, dtype, H, W):
    x, grad = torch.zeros(1, 3, H, W), torch.zeros(1, 3, H, W)
    eng = _host_engine(monkeypatch, dtype, H, W)
    key_none, plain = _step(eng, x, grad)
    assert not any("layer_w" in str(part) for part in key_none) and not eng._heads
    # all ones reach the engine as None (style_mix.tap_weights): the same key, hence the same program
    assert style_mix.tap_weights([1.0] * 5, [0, 5, 10, 19, 28]) is None
    eng.loss_and_grad(x, grad, STYLE_W, 1.0, layer_w=style_mix.tap_weights([1, 1, 1, 1, 1], [0, 5, 10, 19, 28]))
    assert set(eng._programs) == {key_none} and not eng._heads

    lw = (1.0, 0.5, 0.3, 2.0, 0.0)
    key_w, weighted = _step(eng, x, grad, layer_w=lw)
    assert key_w != key_none and key_w[:len(key_none)] == key_none and key_w[-1] == ("layer_w", lw)
    assert [o.op for o in weighted] == [o.op for o in plain]
    c_plain = next(o for o in plain if o.op == _lib.OP_LOSS_COMBINE)
    c_w = next(o for o in weighted if o.op == _lib.OP_LOSS_COMBINE)
    assert c_plain.refs["p1"] is eng.table and c_plain.refs["p2"] is eng.scale and c_plain.refs["q0"] is eng.losses
    table, scale, losses = c_w.refs["p1"], c_w.refs["p2"], c_w.refs["q0"]
    assert table is eng.table and scale is not eng.scale and losses is not eng.losses and losses.shape == eng.losses.shape
    taps = eng.sched.style_taps
    assert scale.dtype == torch.float32 and scale.tolist() == [
        *[_fp32(w / float(t.buf.C * t.buf.C)) for w, t in zip(lw, taps, strict=True)], float(eng.scale[5])]
    assert float(eng.scale[1]) == _fp32(1.0 / float(taps[1].buf.C ** 2))           # the engine's own rows are untouched
    # every op but the combine op and the style taps' seed coefficients is the same, field by field
    coefs_plain, coefs_w = _seed_coefs(plain, eng), _seed_coefs(weighted, eng)
    assert coefs_plain == {k: _fp32(STYLE_W) for k in range(5)}
    assert coefs_w == {k: _fp32(STYLE_W * lw[k]) for k in range(5)}      # (the product formed in double)
    for a, b in zip(plain, weighted, strict=True):
        if a.op == _lib.OP_LOSS_COMBINE:
            skip = {"p2", "q0"}
        elif a.op == _lib.OP_GRAM_MULTI:
            skip = {"p0"}
            assert a.n == b.n
        elif a.op == _lib.OP_GRAM_FINISH:
            skip = {"f2"}
        else:
            skip = set()
        assert all(getattr(a, f) == getattr(b, f) for f in _FIELDS if f not in skip), (a.op, skip)
    # one (table, scale, losses) per weight tuple; together with tv_w one more, with the TV row behind the weighted rows
    _, again = _step(eng, x, torch.zeros(1, 3, H, W), layer_w=lw)
    assert next(o for o in again if o.op == _lib.OP_LOSS_COMBINE).refs["p2"] is scale
    key_tv, with_tv = _step(eng, x, grad, layer_w=lw, tv_w=0.5)
    assert ("tv", 0.5) in key_tv and ("layer_w", lw) in key_tv
    c_tv = next(o for o in with_tv if o.op == _lib.OP_LOSS_COMBINE)
    assert c_tv.cin == 7 and torch.equal(c_tv.refs["p2"][:6], scale) and torch.equal(c_tv.refs["p2"][6:], eng.head(0.5)[1][6:])
    with pytest.raises(ValueError, match="2 style layer weights for 5 style taps"):
        eng.loss_and_grad(x, grad, STYLE_W, 1.0, layer_w=(1.0, 2.0))
    # the forward-only program (forward()) never carries weights
    eng.forward_losses(x)
    fwd = eng._programs[("fwd", x.data_ptr())].op_list
    assert next(o for o in fwd if o.op == _lib.OP_LOSS_COMBINE).refs["p2"] is eng.scale


def test_the_cache_of_weighted_heads_is_bounded(monkeypatch):
    eng = _host_engine(monkeypatch, torch.float32, 32, 32)
    for i in range(40):
        eng.head(layer_w=(1.0, 1.0, 1.0, 1.0, float(i + 2)))
    assert len(eng._heads) <= 16


@pytest.mark.parametrize("cls", [spatial.HaloShard, spatial.SpatialShard])
def test_row_strips_refuse_layer_weights(cls):
    with pytest.raises(ValueError, match=r"style layer weights \[1\.0, 0\.5\]"):
        cls([], [], [], torch.zeros(1, 3, 16, 16), [], dtype=torch.float32, style_w=1.0, content_w=1.0,
            style_layer_weights=[1.0, 0.5])


# ------------------------------------------------------------------------------------------------------- runner
class _Bar:
    def update(self, n=1):
        pass

    def set_postfix(self, d=None, refresh=True, **kw):
        pass

    def close(self):
        pass


class _Plain(nn.Module):
    """Two style terms and a content term, autograd path; ``weights``: what ``style_tap_weights`` reports."""

    def __init__(self, weights=None):
        super().__init__()
        self.weights = weights

    def style_tap_weights(self):
        return self.weights

    def forward(self, x):
        return [(x ** 2).mean(), ((x - 2) ** 2).mean()], [((x - 1) ** 2).mean()]


def test_non_fused_runner_weights_the_style_terms_when_it_sums_them():
    cfg = stv_config.StyleTransferConfig.model_validate({})
    cfg.optimization.steps, cfg.optimization.style_w, cfg.optimization.content_w = 1, 2.0, 1.0
    x0 = torch.rand(1, 3, 6, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    got = {}
    for weights in (None, (0.25, 3.0)):
        x = x0.clone().requires_grad_(True)
        runner = optimization.OptimizationRunner(_Plain(weights), x, cfg, optimizer=torch.optim.SGD([x], lr=0.0), progress_bar=_Bar())
        _, history, _ = runner.run()
        got[weights] = (history["style_loss"][0], history["total_loss"][0], x.grad.clone())
    a, b = float((x0 ** 2).mean()), float(((x0 - 2) ** 2).mean())
    c = float(((x0 - 1) ** 2).mean())
    assert got[None][0] == pytest.approx(a + b, rel=1e-6)
    assert got[(0.25, 3.0)][0] == pytest.approx(0.25 * a + 3.0 * b, rel=1e-6)
    assert got[(0.25, 3.0)][1] == pytest.approx(2.0 * (0.25 * a + 3.0 * b) + c, rel=1e-6)
    n = x0.numel()
    want = 2.0 * (0.25 * 2 * x0 + 3.0 * 2 * (x0 - 2)) / n + 2 * (x0 - 1) / n
    assert torch.allclose(got[(0.25, 3.0)][2], want, rtol=1e-12, atol=1e-15)


# ------------------------------------------------------------------------------------------- main.style_transfer
class Recorder:
    def __init__(self):
        self.events: list = []
        self.prepared = None
        self.pyramid_args = None
        self.saved = None
        self.save_opts = None


IMAGES = {"c.png": (256, 256), "s.png": (136, 120), "t.png": (150, 200), "u.png": (128, 128)}


@pytest.fixture
def wired(monkeypatch):
    """``style_transfer`` on the CPU with every stage a recorder: loads, ``ops.resize``, the colour match, model
    construction, the runner, the pyramid driver and the save step."""
    rec = Recorder()
    images = {name: torch.rand(1, 3, *hw, generator=torch.Generator().manual_seed(i)) for i, (name, hw) in enumerate(IMAGES.items())}
    result = torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(9))

    def load(path, device, normalize):
        rec.events.append(("load", path))
        return images[path]

    def resize(x, size, filter="lanczos", **kw):
        rec.events.append(("resize", tuple(x.shape[-2:]), tuple(size)))
        return torch.zeros(*x.shape[:-2], *size) + x.mean()

    def match(style, content):
        rec.events.append(("match", tuple(style.shape[-2:])))
        return style + 1.0

    def prepare(content, style, device, optimization_config, *, precision=None):
        rec.events.append("model")
        rec.prepared = (content, style)
        return "model", content.clone().requires_grad_(True), "optimizer"

    def run_pyramid(content, style, device, config, **kw):
        rec.events.append("pyramid")
        rec.pyramid_args = (content, style)
        return result.clone(), {"total_loss": [1.0]}, 1.0

    class FakeRunner:
        def __init__(self, *args, **kwargs):
            pass

        def run(self):
            rec.events.append("run")
            return result.clone().requires_grad_(True), {"total_loss": [1.0]}, 3.14

    def save(img, metrics, out_dir, elapsed, opts, **kw):
        rec.saved, rec.save_opts = img, opts
    monkeypatch.setattr(runtime, "validate_input_paths", lambda c, s: rec.events.append(("validate", c, s)))
    monkeypatch.setattr(runtime, "setup_random_seed", lambda seed: None)
    monkeypatch.setattr(runtime, "setup_device", lambda name: torch.device("cpu"))
    monkeypatch.setattr(runtime, "setup_output_directory", lambda p: Path("mock_output"))
    monkeypatch.setattr(runtime, "save_outputs", save)
    monkeypatch.setattr(image_io, "load_image_to_tensor", load)
    monkeypatch.setattr(ops, "resize", resize)
    monkeypatch.setattr(color, "match_style_to_content", match)
    monkeypatch.setattr(core_model, "prepare_model_and_input", prepare)
    monkeypatch.setattr(pyramid, "run_pyramid", run_pyramid)
    monkeypatch.setattr(optimization, "OptimizationRunner", FakeRunner)
    for name in ("blend_weights", "check_layer_weights"):
        real = getattr(style_mix, name)
        monkeypatch.setattr(style_mix, name, lambda *a, _real=real, _name=name: (rec.events.append(("mix", _name)), _real(*a))[1])
    return rec, images, result


def _cfg(**oc):
    cfg = stv_config.StyleTransferConfig.model_validate({})
    cfg.optimization.steps = 4
    cfg.video.create_video = False
    for k, v in oc.items():
        setattr(cfg.optimization, k, v)
    return cfg


def test_defaults_call_nothing_new(wired):
    rec, images, result = wired
    out = stv_main.style_transfer(InputPaths("c.png", "s.png"), _cfg())
    assert rec.events == [("validate", "c.png", "s.png"), ("load", "c.png"), ("load", "s.png"), "model", "run"]
    assert rec.prepared[0] is images["c.png"] and rec.prepared[1] is images["s.png"]     # the tensor itself, no list
    assert rec.save_opts.style_name == "s" and torch.equal(out, result.clamp(0, 1))


def test_every_style_is_loaded_resized_and_matched_once_and_the_list_reaches_the_model(wired):
    rec, images, _ = wired
    paths = InputPaths("c.png", "s.png", ("t.png", "u.png"))
    cfg = _cfg(style_scale=0.5, preserve_color="match", style_blend=[2, 1, 1], style_layer_weights=[1, 0.8, 0.5, 0.3, 0.1])
    stv_main.style_transfer(paths, cfg)
    assert rec.events == [
        ("validate", "c.png", "s.png"), ("validate", "c.png", "t.png"), ("validate", "c.png", "u.png"),
        ("mix", "blend_weights"), ("mix", "check_layer_weights"),
        ("load", "c.png"), ("load", "s.png"), ("load", "t.png"), ("load", "u.png"),
        # each style's own longer side becomes round(0.5 * 256) = 128; u.png is 128x128 already and keeps its tensor
        ("resize", (136, 120), (128, 113)), ("resize", (150, 200), (96, 128)),
        ("match", (128, 113)), ("match", (96, 128)), ("match", (128, 128)),
        "model", "run"]
    content, styles = rec.prepared
    assert content is images["c.png"] and isinstance(styles, list) and [tuple(s.shape[-2:]) for s in styles] == [(128, 113), (96, 128), (128, 128)]
    assert torch.equal(styles[2], images["u.png"] + 1.0)
    assert rec.save_opts.style_name == "s+t+u" and rec.save_opts.content_name == "c"


def test_the_list_reaches_the_pyramid_driver(wired):
    rec, images, _ = wired
    stv_main.style_transfer(InputPaths("c.png", "s.png", ("t.png",)), _cfg(pyramid_levels=2))
    assert "pyramid" in rec.events and "model" not in rec.events and not any(e[0] in ("resize", "match") for e in rec.events if isinstance(e, tuple))
    content, styles = rec.pyramid_args
    assert content is images["c.png"] and isinstance(styles, list) and styles[0] is images["s.png"] and styles[1] is images["t.png"]


@pytest.mark.parametrize("paths,oc,text", [
    (InputPaths("c.png", "s.png", ("t.png",)), {"style_blend": [1, 2, 3]}, "3 weights"),
    (InputPaths("c.png", "s.png"), {"style_blend": [1, 2]}, "2 weights"),
    (InputPaths("c.png", "s.png", ("t.png",)), {"style_blend": [1, -2]}, r"-2\.0"),
    (InputPaths("c.png", "s.png", tuple(["t.png"] * 8)), {}, "got 9"),
    (InputPaths("c.png", "s.png"), {"style_layer_weights": [1, 2]}, "2 weights .* for 5 style layers"),
])
def test_refusals_come_before_the_first_load(wired, paths, oc, text):
    rec, _, _ = wired
    with pytest.raises(ValueError, match=text):
        stv_main.style_transfer(paths, _cfg(**oc))
    assert not any(isinstance(e, tuple) and e[0] == "load" for e in rec.events) and "model" not in rec.events


def test_a_missing_extra_style_is_reported_as_a_style_image(tmp_path):
    for name in ("c.png", "s.png"):
        (tmp_path / name).write_bytes(b"x")
    with pytest.raises(FileNotFoundError, match="Style image not found: .*t.png"):
        stv_main.style_transfer(InputPaths(str(tmp_path / "c.png"), str(tmp_path / "s.png"), (str(tmp_path / "t.png"),)), _cfg())


# --------------------------------------------------------------------------------- prepare_model_and_input, pyramid
class _Model(nn.Module):
    """Stands in for StyleContentModel on the CPU: records what it is given."""

    built: list = []

    def __init__(self, style_layers, content_layers, precision=None, **kw):
        super().__init__()
        self.kw, self.target_kw = kw, None
        type(self).built.append(self)

    def set_targets(self, style, content, **kw):
        self.style, self.content, self.target_kw = style, content, kw

    def forward(self, x):
        return [(x.mean()) ** 2], [((x - self.content) ** 2).mean()]


def test_prepare_hands_the_options_on_only_when_they_are_set(monkeypatch):
    _Model.built = []
    monkeypatch.setattr(core_model, "StyleContentModel", _Model)
    content, a, b = torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16), torch.rand(1, 3, 12, 20)
    oc = _cfg().optimization
    core_model.prepare_model_and_input(content, a, CPU, oc)
    assert _Model.built[-1].kw == {} and _Model.built[-1].target_kw == {} and _Model.built[-1].style is a
    oc = _cfg(style_blend=[3, 1], style_layer_weights=[1, 0.8, 0.5, 0.3, 0.1]).optimization
    core_model.prepare_model_and_input(content, [a, b], CPU, oc)
    built = _Model.built[-1]
    assert built.kw == {"style_layer_weights": [1.0, 0.8, 0.5, 0.3, 0.1]} and built.target_kw == {"style_blend": [3.0, 1.0]}
    assert built.style[0] is a and built.style[1] is b


def test_pyramid_crops_and_halves_each_style_on_its_own(monkeypatch):
    _Model.built = []
    monkeypatch.setattr(core_model, "StyleContentModel", _Model)

    def resize2x(x, mode, out=None):
        x = x.detach()
        if mode == _lib.RESIZE_DOWN2:
            return torch.nn.functional.avg_pool2d(x, 2)
        return torch.nn.functional.interpolate(x, scale_factor=2, mode="nearest")
    monkeypatch.setattr(ops, "resize2x", resize2x)
    content, a, b = torch.rand(1, 3, 128, 128), torch.rand(1, 3, 137, 128), torch.rand(1, 3, 130, 161)
    cfg = _cfg(pyramid_levels=2, style_blend=[3, 1], init_method="content")
    cfg.output.log_every = 1
    pyramid.run_pyramid(content, [a, b], CPU, cfg, optimizer_factory=lambda x: torch.optim.SGD([x], lr=0.1), progress_bar=_Bar())
    coarse, fine = _Model.built
    assert [tuple(s.shape[-2:]) for s in fine.style] == [(136, 128), (130, 160)]
    assert torch.equal(fine.style[0], a[..., :136, :]) and torch.equal(fine.style[1], b[..., :, :160])
    assert [tuple(s.shape[-2:]) for s in coarse.style] == [(68, 64), (65, 80)]
    assert torch.equal(coarse.style[1], resize2x(b[..., :, :160].contiguous(), _lib.RESIZE_DOWN2))
    assert coarse.target_kw == fine.target_kw == {"style_blend": [3.0, 1.0]} and coarse.kw == {}
    # one style: the tensor itself, and no keyword, as always
    _Model.built = []
    pyramid.run_pyramid(content, a, CPU, _cfg(pyramid_levels=2, init_method="content"),
                        optimizer_factory=lambda x: torch.optim.SGD([x], lr=0.1), progress_bar=_Bar())
    assert isinstance(_Model.built[1].style, torch.Tensor) and _Model.built[1].target_kw == {}
