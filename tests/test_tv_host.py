"""Total-variation term (--tv-w), everything that runs without a GPU: configuration, the torch definition against the
float64 oracle, the C ABI, the op lists of the fused step (built on host tensors, never run), the runner's two paths and
the row-strip refusal."""
from __future__ import annotations

import functools
import inspect
import os
import re

import pytest
import torch
from torch import nn

from style_transfer_visualizer_amd import _lib, cli, core_model, plan, spatial
from style_transfer_visualizer_amd import config as stv_config
from style_transfer_visualizer_amd import config_defaults
from style_transfer_visualizer_amd.optimization import OptimizationRunner
from tests import tv_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


# ------------------------------------------------------------------------------------------------ configuration
def _cli_config(argv):
    args = cli.build_arg_parser().parse_args(argv)
    base = stv_config.ConfigLoader.load(args.config) if args.config else None
    return stv_config.build_config_from_cli(vars(args), base_config=base)


def test_default_is_zero():
    assert config_defaults.DEFAULT_TV_WEIGHT == 0.0
    assert stv_config.StyleTransferConfig.model_validate({}).optimization.tv_w == 0.0
    assert _cli_config(["--content", "c.png", "--style", "s.png"]).optimization.tv_w == 0.0


def test_cli_and_toml_round_trip(tmp_path):
    assert _cli_config(["--content", "c.png", "--style", "s.png", "--tv-w", "0.5"]).optimization.tv_w == 0.5
    toml = tmp_path / "config.toml"
    toml.write_text("[optimization]\ntv_w = 0.25\nsteps = 7\n")
    cfg = stv_config.ConfigLoader.load(str(toml))
    assert cfg.optimization.tv_w == 0.25 and cfg.optimization.steps == 7
    assert stv_config.StyleTransferConfig.model_validate(cfg.model_dump()).optimization.tv_w == 0.25
    assert _cli_config(["--config", str(toml)]).optimization.tv_w == 0.25                       # TOML alone
    assert _cli_config(["--config", str(toml), "--tv-w", "2"]).optimization.tv_w == 2.0         # the CLI overrides it
    assert stv_config._DIRECT["tv_w"] == ("optimization", "tv_w")


def test_negative_weight_is_rejected(tmp_path):
    with pytest.raises(ValueError):
        stv_config.OptimizationConfig(tv_w=-0.1)
    toml = tmp_path / "config.toml"
    toml.write_text("[optimization]\ntv_w = -1.0\n")
    with pytest.raises(ValueError):
        stv_config.ConfigLoader.load(str(toml))


def test_settings_summary_shows_the_weight_only_when_set(caplog):
    from style_transfer_visualizer_amd.type_defs import InputPaths
    paths = InputPaths(content_path="c.png", style_path="s.png")
    with caplog.at_level("INFO"):
        cli.log_parameters(paths, _cli_config(["--content", "c.png", "--style", "s.png"]))
    assert "Total Variation Weight" not in caplog.text
    caplog.clear()
    with caplog.at_level("INFO"):
        cli.log_parameters(paths, _cli_config(["--content", "c.png", "--style", "s.png", "--tv-w", "0.5"]))
    assert "Total Variation Weight: 0.5" in caplog.text


# ------------------------------------------------------------------------------------------------------- oracle
def test_total_variation_matches_the_oracle_in_float64():
    g = torch.Generator().manual_seed(3)
    for shape in ((1, 3, 1, 1), (1, 3, 1, 7), (1, 3, 5, 1), (1, 1, 2, 2), (1, 3, 17, 33), (3, 6, 5)):
        x = torch.randn(shape, dtype=torch.float64, generator=g, requires_grad=True)
        want, want_grad = tv_ref.tv_and_grad(x)
        got = core_model.total_variation(x)
        assert got.dtype == torch.float64 and got.dim() == 0
        assert float(got.detach()) == pytest.approx(float(want), rel=1e-14, abs=0.0)
        (grad,) = torch.autograd.grad(got, x)
        assert torch.allclose(grad, want_grad, rtol=1e-13, atol=1e-15)
    with pytest.raises(ValueError):
        core_model.total_variation(torch.zeros(2, 3, 4, 4))


def test_hand_computed_values_on_a_1x2x2_image():
    x = torch.tensor([[[[1.0, 4.0], [-2.0, 8.0]]]], dtype=torch.float64, requires_grad=True)
    # vertical: (-2-1)^2 + (8-4)^2 = 25, horizontal: (4-1)^2 + (8+2)^2 = 109; C*H*W = 4
    want = (25.0 + 109.0) / 4.0
    assert float(core_model.total_variation(x).detach()) == want == float(tv_ref.tv(x))
    # 2/4 * sum over the two neighbours of (x - n)
    want_grad = 0.5 * torch.tensor([[[[(1 + 2) + (1 - 4), (4 - 8) + (4 - 1)], [(-2 - 1) + (-2 - 8), (8 - 4) + (8 + 2)]]]],
                                   dtype=torch.float64)
    (grad,) = torch.autograd.grad(core_model.total_variation(x), x)
    assert torch.equal(grad, want_grad) and torch.equal(tv_ref.tv_and_grad(x)[1], want_grad)
    assert float(core_model.total_variation(torch.zeros(1, 3, 1, 1, dtype=torch.float64))) == 0.0


# ---------------------------------------------------------------------------------------------------------- ABI
def test_library_exports_stv_tv_and_the_constants_match_the_header():
    lib = _lib.load()
    assert hasattr(lib, "stv_tv") and "stv_tv" in _lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "stv.h")).read()
    assert int(re.search(r"#define\s+STV_TV_LOSS_PARTS\s+(\d+)", header).group(1)) == _lib.TV_LOSS_PARTS
    ops_enum = re.search(r"enum\s*\{\s*(STV_OP_CONV_FIRST_FWD[^}]*)\}", header).group(1)
    names = [n.split("=")[0].strip() for n in ops_enum.split(",")]
    assert names.index("STV_OP_TV") + 1 == _lib.OP_TV == _lib.OP_LBFGS_ITER + 1       # appended: the others keep their numbers
    assert lib.stv_version() >= 105
    source = open(os.path.join(ROOT, "style_transfer_visualizer_amd", "csrc", "pointwise.hip")).read()
    assert int(re.search(r"kTvThreads\s*=\s*(\d+)", source).group(1)) == _lib.TV_THREADS
    assert re.search(r"kTvBlocks\s*=\s*STV_TV_LOSS_PARTS", source)
    # argument checks come before any device work: they can be asked for on a machine without a GPU
    assert lib.stv_tv(None, None, None, 3, 4, 4, 1.0, 0, None) == 1
    assert lib.stv_tv(16, None, None, 3, 4, 4, 1.0, 0, None) == 1                     # both outputs null
    assert lib.stv_tv(16, 32, None, 0, 4, 4, 1.0, 0, None) == 1
    assert lib.stv_tv(16, 32, None, 3, -1, 4, 1.0, 0, None) == 1
    assert lib.stv_tv(16, 32, None, 3, 4, 0, 1.0, 0, None) == 1
    assert lib.stv_tv(16, 32, None, 2, 16384, 16384, 1.0, 0, None) == 1               # 2 * 2^28 * 4 bytes = 2 GiB
    assert lib.stv_tv(16, None, 16, 3, 4, 4, 1.0, 0, None) == 1                       # x == dx


# ----------------------------------------------------------------------------------------------------- op lists
@functools.cache
def _layers():
    return list(core_model.build_vgg_features().eval().children())


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
    eng.loss_and_grad(x, grad, 1e5, 1.0, **kw)
    (key,) = set(eng._programs) - before
    return key, eng._programs[key].op_list


@pytest.mark.parametrize("dtype,H,W", [(torch.bfloat16, 64, 64), (torch.float32, 48, 80)])
def test_op_lists_with_and_without_the_term(monkeypatch, dtype, H, W):
    x, grad = torch.zeros(1, 3, H, W), torch.zeros(1, 3, H, W)
    key_plain, plain = _step(_host_engine(monkeypatch, dtype, H, W), x, grad)
    eng = _host_engine(monkeypatch, dtype, H, W)
    key_zero, zero = _step(eng, x, grad, tv_w=0.0)
    assert key_zero == key_plain and [o.op for o in zero] == [o.op for o in plain]
    combine = next(o for o in zero if o.op == _lib.OP_LOSS_COMBINE)
    assert combine.cin == 6 and combine.refs["p1"] is eng.table and combine.refs["p2"] is eng.scale

    key_tv, with_tv = _step(eng, x, grad, tv_w=0.5)
    assert key_tv != key_zero and ("tv", 0.5) in key_tv
    kinds = [o.op for o in with_tv]
    assert len(kinds) == len(plain) + 2 and kinds.count(_lib.OP_TV) == 2
    assert [k for k in kinds if k != _lib.OP_TV] == [o.op for o in plain]
    i_loss, i_grad = (i for i, k in enumerate(kinds) if k == _lib.OP_TV)
    loss_op, grad_op = with_tv[i_loss], with_tv[i_grad]
    # loss form: the head of the forward half, reads the image only, in front of the combine op
    assert i_loss == 0 and i_loss < kinds.index(_lib.OP_LOSS_COMBINE)
    assert loss_op.p0 == x.data_ptr() and loss_op.q0 and not loss_op.q1 and loss_op.flags == 0
    assert loss_op.q0 == eng.parts[eng.tv_parts_off:].data_ptr()
    assert eng.parts.numel() == eng.tv_parts_off + _lib.TV_LOSS_PARTS
    # accumulate form: right behind the first-layer dgrad that WRITES grad, in front of any L-BFGS op
    assert kinds[i_grad - 1] == _lib.OP_CONV_FIRST_DGRAD and with_tv[i_grad - 1].q0 == grad.data_ptr()
    assert not any(k in (_lib.OP_LBFGS_STEP, _lib.OP_LBFGS_ITER) for k in kinds[:i_grad])
    assert grad_op.p0 == x.data_ptr() and grad_op.q1 == grad.data_ptr() and not grad_op.q0 and grad_op.flags == _lib.ACCUM
    for o in (loss_op, grad_op):
        assert (o.cin, o.H, o.W) == (3, H, W)
    want_coef = torch.tensor(0.5 * 2.0 / (3 * H * W), dtype=torch.float64).to(torch.float32)
    assert grad_op.f0 == float(want_coef) == core_model.tv_coef(0.5, 3, H, W)
    # the combine table: the engine's rows and one more, of kind 2, whose scale carries the weight
    combine = next(o for o in with_tv if o.op == _lib.OP_LOSS_COMBINE)
    table, scale = combine.refs["p1"], combine.refs["p2"]
    assert combine.cin == 7 and table.shape == (7, 3) and torch.equal(table[:6], eng.table)
    assert table[6].tolist() == [eng.tv_parts_off, _lib.TV_LOSS_PARTS, 2] and not (eng.table[:, 2] == 2).any()
    assert torch.equal(scale[:6], eng.scale)
    assert float(scale[6]) == float(torch.tensor(0.5 / (3 * H * W), dtype=torch.float64).to(torch.float32))
    # the pair is cached per weight; another weight gets its own
    _, again = _step(eng, x, torch.zeros(1, 3, H, W), tv_w=0.5)
    assert next(o for o in again if o.op == _lib.OP_LOSS_COMBINE).refs["p1"] is table
    _, other = _step(eng, x, grad, tv_w=0.25)
    assert next(o for o in other if o.op == _lib.OP_LOSS_COMBINE).refs["p1"] is not table


def test_the_update_op_follows_the_accumulate_op(monkeypatch):
    """With the L-BFGS update at the end of the program (single- and multi-iteration form), the TV gradient is in
    ``grad`` before the update reads it."""
    from style_transfer_visualizer_amd import optimizers
    H = W = 64
    x, grad = torch.zeros(1, 3, H, W), torch.zeros(1, 3, H, W)
    for iters, op in ((0, _lib.OP_LBFGS_STEP), (4, _lib.OP_LBFGS_ITER)):
        eng = _host_engine(monkeypatch, torch.bfloat16, H, W)
        fields = {f: None for f in inspect.signature(optimizers.StepRequest).parameters}
        fields.update(state=torch.zeros(8), work=torch.zeros(8), history=100, lr=1.0, tol_grad=1e-7, tol_change=1e-9,
                      iters_per_step=iters)
        req = optimizers.StepRequest(**fields)
        _, ops_ = _step(eng, x, grad, tv_w=0.5, then_step=req)
        kinds = [o.op for o in ops_]
        assert kinds[-1] == op and kinds[-2] == _lib.OP_TV and kinds[-3] == _lib.OP_CONV_FIRST_DGRAD


# ------------------------------------------------------------------------------------------------------- runner
class _Bar:
    def update(self, n=1):
        pass

    def set_postfix(self, d=None, refresh=True, **kw):
        pass

    def close(self):
        pass


def _cfg(tv_w, steps=1):
    cfg = stv_config.StyleTransferConfig.model_validate({})
    cfg.optimization.steps, cfg.optimization.style_w, cfg.optimization.content_w = steps, 2.0, 1.0
    cfg.optimization.tv_w = tv_w
    cfg.optimization.normalize = False
    return cfg


class _FusedWithoutKeyword(nn.Module):
    def loss_and_grad(self, x, style_w, content_w):
        x.grad = torch.zeros_like(x)
        z = torch.zeros(())
        return z, z, z


class _FusedWithKeyword(nn.Module):
    seen = None

    def loss_and_grad(self, x, style_w, content_w, *, tv_w=0.0):
        type(self).seen = tv_w
        x.grad = torch.zeros_like(x)
        z = torch.zeros(())
        return z, z, z


class _Plain(nn.Module):
    def forward(self, x):
        return [(x ** 2).mean()], [((x - 1) ** 2).mean()]


def test_fused_runner_refuses_a_model_without_the_keyword():
    x = torch.rand(1, 3, 6, 5, requires_grad=True)
    runner = OptimizationRunner(_FusedWithoutKeyword(), x, _cfg(0.5), optimizer=torch.optim.SGD([x], lr=0.0), progress_bar=_Bar())
    with pytest.raises(ValueError, match="tv_w"):
        runner.run()
    x = torch.rand(1, 3, 6, 5, requires_grad=True)      # weight 0: the same model runs as it always did
    OptimizationRunner(_FusedWithoutKeyword(), x, _cfg(0.0), optimizer=torch.optim.SGD([x], lr=0.0), progress_bar=_Bar()).run()
    x = torch.rand(1, 3, 6, 5, requires_grad=True)
    OptimizationRunner(_FusedWithKeyword(), x, _cfg(0.5), optimizer=torch.optim.SGD([x], lr=0.0), progress_bar=_Bar()).run()
    assert _FusedWithKeyword.seen == 0.5


def test_non_fused_runner_adds_the_term_and_its_gradient():
    torch.manual_seed(5)
    x0 = torch.rand(1, 3, 6, 5, dtype=torch.float64)
    results = {}
    for tv_w in (0.0, 0.75):
        x = x0.clone().requires_grad_(True)
        runner = OptimizationRunner(_Plain(), x, _cfg(tv_w), optimizer=torch.optim.SGD([x], lr=0.0), progress_bar=_Bar())
        _, history, _ = runner.run()
        results[tv_w] = (history["total_loss"][0], x.grad.clone(), history["style_loss"][0], history["content_loss"][0])
    value, grad = tv_ref.tv_and_grad(x0)
    assert results[0.75][0] == pytest.approx(results[0.0][0] + 0.75 * float(value), rel=1e-6)     # (history is fp32)
    assert results[0.75][2:] == results[0.0][2:]                                                  # the scores do not carry it
    assert torch.allclose(results[0.75][1] - results[0.0][1], 0.75 * grad, rtol=1e-12, atol=1e-15)


# --------------------------------------------------------------------------------------------------- row strips
@pytest.mark.parametrize("cls", [spatial.HaloShard, spatial.SpatialShard])
def test_row_strips_refuse_the_term(cls):
    with pytest.raises(ValueError, match="total-variation"):
        cls([], [], [], torch.zeros(1, 3, 16, 16), [], dtype=torch.float32, style_w=1.0, content_w=1.0, tv_w=0.5)
