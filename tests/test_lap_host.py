"""Laplacian loss (--lap-w, --lap-pool), everything that runs without a GPU: the NumPy twin against the torch definition and
against itself in float64, the C ABI and its argument refusals, the op lists of the fused step (built on host tensors, never
run), configuration, the runner's two paths and the refusals."""
from __future__ import annotations

import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

from style_transfer_visualizer_amd import _lib, cli, core_model, plan, pyramid, spatial
from style_transfer_visualizer_amd import config as stv_config
from style_transfer_visualizer_amd import config_defaults
from style_transfer_visualizer_amd.optimization import OptimizationRunner
from tests import lap_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


# --------------------------------------------------------------------------------------------------------- twin
TWIN_SHAPES = [((3, 2, 2), 1), ((3, 4, 4), 2), ((1, 5, 7), 2), ((3, 9, 13), 4), ((3, 17, 33), 1), ((3, 32, 32), 16),
               ((3, 64, 64), 32), ((2, 40, 24), 8)]


@pytest.mark.parametrize("shape,p", TWIN_SHAPES)
def test_twin_equals_the_torch_definition_in_float64(shape, p):
    g = torch.Generator().manual_seed(11 + p)
    x = torch.randn(1, *shape, dtype=torch.float64, generator=g, requires_grad=True)
    content = torch.randn(1, *shape, dtype=torch.float64, generator=g)
    got = core_model.laplacian_loss(x, content, p)
    assert got.dtype == torch.float64 and got.dim() == 0
    assert float(got.detach()) == pytest.approx(lap_ref.loss(x, content, p), rel=1e-12, abs=0.0)
    (grad,) = torch.autograd.grad(got, x)
    want = torch.from_numpy(lap_ref.loss_grad(x, content, p)).reshape(x.shape)
    assert torch.allclose(grad, want, rtol=1e-11, atol=1e-14)
    assert float(core_model.laplacian_loss(x[0], content[0], p).detach()) == float(got.detach())      # [C, H, W] as well


def test_definition_refusals_and_a_hand_computed_value():
    with pytest.raises(ValueError):
        core_model.laplacian_loss(torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 4, 4), 2)
    with pytest.raises(ValueError):
        core_model.laplacian_loss(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 6), 2)
    with pytest.raises(ValueError):
        core_model.laplacian_loss(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4), 3)
    # one plane, 2 x 4 pixels, pool 2 over a zero content image: cells (3, -1); the remainder column takes no part for 2 x 5
    x = torch.tensor([[[[1.0, 5.0, 0.0, -2.0, 99.0], [3.0, 3.0, -1.0, -1.0, 99.0]]]], dtype=torch.float64, requires_grad=True)
    value = core_model.laplacian_loss(x, torch.zeros_like(x), 2)
    # e = [3, -1]; r = [3 - (-1), -1 - 3] = [4, -4]; lap = 32 / 2
    assert float(value.detach()) == 16.0 == lap_ref.loss(x, torch.zeros_like(x), 2)
    (grad,) = torch.autograd.grad(value, x)
    # L r = [8, -8]; 2 / (1*1*2*4) = 0.25
    want = torch.tensor([[[[2.0, 2.0, -2.0, -2.0, 0.0], [2.0, 2.0, -2.0, -2.0, 0.0]]]], dtype=torch.float64)
    assert torch.equal(grad, want)
    assert np.array_equal(lap_ref.loss_grad(x, torch.zeros_like(x), 2), want[0].numpy())


@pytest.mark.parametrize("shape,p", TWIN_SHAPES)
def test_fp32_twin_stays_within_its_rounding_chain_of_float64(shape, p):
    """The bounds are those of tests/lap_ref.py (``bounds``), derived there from the chain of rounded operations: 2p - 2 adds
    for a cell mean, one subtraction, at most four differences and three rounded adds per stencil, one product, one add."""
    g = torch.Generator().manual_seed(23 + p)
    x, content, dx0 = (torch.randn(shape, generator=g) for _ in range(3))
    coef = core_model.lap_coef(0.7, shape[0], shape[1] // p, shape[2] // p, p)
    b = lap_ref.bounds(x, content, p, coef, dx0)
    t32, t64 = lap_ref.pool(content, p), lap_ref.pool(content, p, np.float64)
    m32, m64 = lap_ref.pool(x, p), lap_ref.pool(x, p, np.float64)
    assert m32.dtype == np.float32 and (np.abs(m32 - m64) <= b["pool"]).all()
    r32, r64 = lap_ref.resid(x, t32, p), lap_ref.resid(x, t64, p, np.float64)
    assert r32.dtype == np.float32 and (np.abs(r32 - r64) <= b["r"]).all()
    d32 = lap_ref.grad_accum(r32, dx0, p, coef)
    d64 = lap_ref.grad_accum(r64, dx0, p, coef, dtype=np.float64)
    assert d32.dtype == np.float32 and (np.abs(d32 - d64) <= b["dx"]).all()
    assert float(b["dx"].max()) < 1e-4 * max(1.0, float(np.abs(d64).max()))       # (the bound is a tight one, not a licence)
    if p == 1:                                                                   # one pixel per cell: no add, no error
        assert np.array_equal(m32.astype(np.float64), m64)
    Hp, Wp = shape[1] // p, shape[2] // p
    cover = np.zeros(shape, dtype=bool)
    cover[:, :Hp * p, :Wp * p] = True
    assert np.array_equal(d32[~cover], lap_ref._chw(dx0, np.float32)[~cover])     # the remainder pixels: untouched
    assert not lap_ref.grad_accum(r32, dx0, p, coef, accum=False)[~cover].any()   # or zero


def test_scale_and_coefficient():
    want = float(torch.tensor(0.3 * 2.0 / (3 * 16 * 12 * 16), dtype=torch.float64).to(torch.float32))
    assert core_model.lap_coef(0.3, 3, 16, 12, 4) == want
    assert core_model.lap_scale(0.3, 3, 16, 12) == float(torch.tensor(0.3 / (3 * 16 * 12), dtype=torch.float64).to(torch.float32))


# ---------------------------------------------------------------------------------------------------------- ABI
def test_library_exports_stv_lap_and_the_constants_match_the_header():
    lib = _lib.load()
    assert hasattr(lib, "stv_lap") and "stv_lap" in _lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "stv.h")).read()

    def define(name):
        return int(re.search(rf"#define\s+{name}\s+(\d+)", header).group(1))
    assert define("STV_LAP_LOSS_PARTS") == _lib.LAP_LOSS_PARTS and define("STV_LAP_THREADS") == _lib.LAP_THREADS
    assert define("STV_LAP_TILE_H") == _lib.LAP_TILE_H and define("STV_LAP_TILE_W") == _lib.LAP_TILE_W
    assert define("STV_LAP_GRAD_MAX_BLOCKS") == _lib.LAP_GRAD_MAX_BLOCKS
    assert _lib.LAP_TILE_H * _lib.LAP_TILE_W == _lib.LAP_THREADS
    modes = re.search(r"enum\s*\{\s*STV_LAP_POOL\s*=\s*(\d+),\s*STV_LAP_LOSS\s*=\s*(\d+),\s*STV_LAP_GRAD\s*=\s*(\d+)", header)
    assert tuple(int(v) for v in modes.groups()) == (_lib.LAP_POOL, _lib.LAP_LOSS, _lib.LAP_GRAD)
    ops_enum = re.search(r"enum\s*\{\s*(STV_OP_CONV_FIRST_FWD[^}]*)\}", header).group(1)
    names = [n.split("=")[0].strip() for n in ops_enum.split(",")]
    assert names.index("STV_OP_LAP") + 1 == _lib.OP_LAP == _lib.OP_TV + 1 == 18        # appended: the others keep their numbers
    assert names.index("STV_OP_TV") + 1 == _lib.OP_TV == 17
    assert lib.stv_version() >= 111
    assert "lap.hip" in open(os.path.join(ROOT, "style_transfer_visualizer_amd", "csrc", "Makefile")).read()


def test_argument_checks_come_before_any_device_work():
    """Every refusal returns STV_ERR_ARG (1) on a machine without a GPU: nothing is launched.  Pointers are made-up numbers."""
    lib = _lib.load()
    X, T, R, P, D = 0x1000, 0x2000, 0x3000, 0x4000, 0x100000
    POOL, LOSS, GRAD = _lib.LAP_POOL, _lib.LAP_LOSS, _lib.LAP_GRAD

    def call(x=X, t=T, cells=R, part=P, dx=D, C=3, H=8, W=8, pool=2, mode=LOSS, flags=0):
        return lib.stv_lap(x, t, cells, part, dx, C, H, W, pool, 1.0, mode, flags, None)
    # the pointers each mode needs
    assert call(x=None, mode=POOL) == 1 and call(cells=None, mode=POOL) == 1
    assert call(x=None) == 1 and call(t=None) == 1 and call(cells=None) == 1 and call(part=None) == 1
    assert call(cells=None, mode=GRAD) == 1 and call(dx=None, mode=GRAD) == 1
    for mode in (POOL, LOSS, GRAD):
        for bad in (dict(C=0), dict(H=0), dict(W=-1), dict(C=-3)):
            assert call(mode=mode, **bad) == 1
        for pool in (0, -1, 3, 5, 6, 12, 64, 128):
            assert call(mode=mode, pool=pool, H=256, W=256) == 1
        assert call(mode=mode, pool=16, H=15, W=64) == 1 and call(mode=mode, pool=16, H=64, W=15) == 1       # no cell at all
        assert call(mode=mode, C=2, H=16384, W=16384) == 1                                                   # 2 GiB
        assert call(mode=mode, flags=_lib.MASK) == 1 and call(mode=mode, flags=_lib.ACCUM | _lib.RELU_IN) == 1
    assert call(mode=3) == 1 and call(mode=-1) == 1
    assert call(mode=POOL, flags=_lib.ACCUM) == 1 and call(mode=LOSS, flags=_lib.ACCUM) == 1                 # GRAD's flag
    # dx sharing a byte with the residual: 3*4*4*4 = 192 bytes of cells, 768 of image
    assert call(mode=GRAD, cells=R, dx=R) == 1 and call(mode=GRAD, cells=R, dx=R + 188) == 1
    assert call(mode=GRAD, cells=R + 764, dx=R) == 1


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


def _host_engine(monkeypatch, dtype, H, W, **kw):
    monkeypatch.setattr(plan, "Program", RecordedProgram)
    eng = core_model._Engine(_layers(), [0, 5, 10, 19, 28], [21], H, W, dtype, CPU, assume_device=True, **kw)
    for tap in eng.sched.style_taps:
        tap.target = torch.zeros(tap.buf.C, tap.buf.C)
    for tap in eng.sched.content_taps:
        tap.target = torch.empty_like(tap.buf.act)
    if eng.lap_pools:
        eng.bind_lap_targets([torch.zeros_like(r) for r in eng.lap_resid])
    return eng


def _step(eng, x, grad, **kw):
    before = set(eng._programs)
    eng.loss_and_grad(x, grad, 1e5, 1.0, **kw)
    (key,) = set(eng._programs) - before
    return key, eng._programs[key].op_list


def _fp32(v):
    return float(torch.tensor(v, dtype=torch.float64).to(torch.float32))


@pytest.mark.parametrize("dtype,H,W", [(torch.bfloat16, 64, 64), (torch.float32, 48, 80)])
def test_op_lists_with_and_without_the_term(monkeypatch, dtype, H, W):
    x, grad = torch.zeros(1, 3, H, W), torch.zeros(1, 3, H, W)
    plain_eng = _host_engine(monkeypatch, dtype, H, W)
    key_plain, plain = _step(plain_eng, x, grad)
    # an engine without pools allocates exactly what it did, and refuses the weight
    assert plain_eng.parts.numel() == plain_eng.tv_parts_off + _lib.TV_LOSS_PARTS and plain_eng.lap_pools == ()
    with pytest.raises(ValueError, match="lap_w = 0.5"):
        plain_eng.loss_and_grad(x, grad, 1e5, 1.0, lap_w=0.5)

    pools = (4, 16)
    eng = _host_engine(monkeypatch, dtype, H, W, lap_pools=pools)
    assert eng.lap_parts_off == eng.tv_parts_off + _lib.TV_LOSS_PARTS
    assert eng.parts.numel() == eng.lap_parts_off + 2 * _lib.LAP_LOSS_PARTS
    assert [tuple(r.shape) for r in eng.lap_resid] == [(3, H // 4, W // 4), (3, H // 16, W // 16)]
    key_zero, zero = _step(eng, x, grad, lap_w=0.0)
    assert key_zero == key_plain and [o.op for o in zero] == [o.op for o in plain]
    combine = next(o for o in zero if o.op == _lib.OP_LOSS_COMBINE)
    assert combine.cin == 6 and combine.refs["p1"] is eng.table and combine.refs["p2"] is eng.scale and combine.refs["q0"] is eng.losses
    key_tv0, tv_only = _step(eng, x, grad, tv_w=0.5)
    assert next(o for o in tv_only if o.op == _lib.OP_LOSS_COMBINE).refs["p1"] is eng.head(0.5)[0]
    assert not any("lap" in str(k) for k in key_tv0)

    for tv_w in (0.0, 0.5):
        base = tv_only if tv_w else plain
        key, with_lap = _step(eng, x, grad, lap_w=0.25, tv_w=tv_w)
        assert ("lap", 0.25, pools) in key and (("tv", 0.5) in key) == bool(tv_w)
        kinds = [o.op for o in with_lap]
        assert len(kinds) == len(base) + 2 * 2 and kinds.count(_lib.OP_LAP) == 4
        assert [k for k in kinds if k != _lib.OP_LAP] == [o.op for o in base]
        at = [i for i, k in enumerate(kinds) if k == _lib.OP_LAP]
        n_tv = 1 if tv_w else 0
        i_combine = kinds.index(_lib.OP_LOSS_COMBINE)
        # LOSS forms: the head of the forward half, behind TV's loss op (which stays at index 0), in front of the combine op
        assert at[:2] == [n_tv, n_tv + 1] and at[1] < i_combine
        assert (kinds[0] == _lib.OP_TV) == bool(tv_w)
        # GRAD forms: behind the first-layer dgrad (which WRITES grad) and TV's accumulate op, in front of any L-BFGS op
        i_dgrad = max(i for i, k in enumerate(kinds) if k == _lib.OP_CONV_FIRST_DGRAD)
        assert with_lap[i_dgrad].q0 == grad.data_ptr()
        assert at[2:] == [i_dgrad + 1 + n_tv, i_dgrad + 2 + n_tv]
        if tv_w:
            assert kinds[i_dgrad + 1] == _lib.OP_TV and with_lap[i_dgrad + 1].q1 == grad.data_ptr()
        assert not any(k in (_lib.OP_LBFGS_STEP, _lib.OP_LBFGS_ITER) for k in kinds)
        for k, p in enumerate(pools):
            loss_op, grad_op = with_lap[at[k]], with_lap[at[2 + k]]
            Hp, Wp = H // p, W // p
            for o in (loss_op, grad_op):
                assert (o.cin, o.H, o.W, o.cout) == (3, H, W, p) and o.q0 == eng.lap_resid[k].data_ptr()
            assert loss_op.taps == _lib.LAP_LOSS and loss_op.flags == 0 and loss_op.p0 == x.data_ptr()
            assert loss_op.p1 == eng.lap_targets[k].data_ptr() and not loss_op.q2
            assert loss_op.q1 == eng.parts[eng.lap_parts_off + k * _lib.LAP_LOSS_PARTS:].data_ptr()
            assert grad_op.taps == _lib.LAP_GRAD and grad_op.flags == _lib.ACCUM and grad_op.q2 == grad.data_ptr()
            assert not grad_op.p0 and not grad_op.p1 and not grad_op.q1
            assert grad_op.f0 == _fp32(0.25 * 2.0 / (3 * Hp * Wp * p * p)) == core_model.lap_coef(0.25, 3, Hp, Wp, p)
        # the combine table: the rows of the step without the term, then one kind-2 row per pool whose scale carries the weight
        combine = with_lap[i_combine]
        table, scale, losses = combine.refs["p1"], combine.refs["p2"], combine.refs["q0"]
        n0 = 6 + n_tv
        assert combine.cin == n0 + 2 and table.shape == (n0 + 2, 3) and losses.shape == (n0 + 2,)
        assert torch.equal(table[:6], eng.table) and torch.equal(scale[:6], eng.scale)
        if tv_w:
            assert table[6].tolist() == [eng.tv_parts_off, _lib.TV_LOSS_PARTS, 2]
            assert float(scale[6]) == core_model.tv_scale(0.5, 3, H, W)
        for k, p in enumerate(pools):
            assert table[n0 + k].tolist() == [eng.lap_parts_off + k * _lib.LAP_LOSS_PARTS, _lib.LAP_LOSS_PARTS, 2]
            assert float(scale[n0 + k]) == _fp32(0.25 / (3 * (H // p) * (W // p))) == core_model.lap_scale(0.25, 3, H // p, W // p)
        assert not (eng.table[:, 2] == 2).any()
        # the head is cached per (tv_w, lap_w, layer_w); another weight gets its own; the head of tv_w alone is what it was
        _, again = _step(eng, x, torch.zeros(1, 3, H, W), lap_w=0.25, tv_w=tv_w)
        assert next(o for o in again if o.op == _lib.OP_LOSS_COMBINE).refs["p1"] is table
        _, other = _step(eng, x, grad, lap_w=0.125, tv_w=tv_w)
        assert next(o for o in other if o.op == _lib.OP_LOSS_COMBINE).refs["p1"] is not table
        assert eng.head(tv_w, 0.25)[0] is table
    assert eng.head(0.5)[0].shape == (7, 3)


def test_head_with_layer_weights(monkeypatch):
    H = W = 64
    x, grad = torch.zeros(1, 3, H, W), torch.zeros(1, 3, H, W)
    eng = _host_engine(monkeypatch, torch.bfloat16, H, W, lap_pools=(8,))
    lw = (1.0, 0.8, 0.5, 0.3, 0.1)
    key, ops_ = _step(eng, x, grad, lap_w=2.0, tv_w=0.5, layer_w=lw)
    assert key[-3:] == (("tv", 0.5), ("layer_w", lw), ("lap", 2.0, (8,)))
    combine = next(o for o in ops_ if o.op == _lib.OP_LOSS_COMBINE)
    table, scale = combine.refs["p1"], combine.refs["p2"]
    assert table.shape == (8, 3) and torch.equal(scale[:7], eng.head(0.5, layer_w=lw)[1])
    assert table[7].tolist() == [eng.lap_parts_off, _lib.LAP_LOSS_PARTS, 2]
    assert eng.head(0.5, 2.0, lw)[0] is table and eng.head(0.5, 2.0)[0] is not table


@pytest.mark.parametrize("layer_w", [None, (1.0, 0.8, 0.5, 0.0, 0.1)], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("lap_w", [0.0, 0.25])
@pytest.mark.parametrize("tv_w", [0.0, 0.5])
def test_the_one_head_of_every_combination(monkeypatch, tv_w, lap_w, layer_w):
    """The table is the base rows, then the TV row, then the pool rows; the slots the head names are exactly those rows; the
    all-off combination is the engine's own three objects."""
    H = W = 64
    pools = (4, 16)
    eng = _host_engine(monkeypatch, torch.bfloat16, H, W, lap_pools=pools)
    head = eng.head(tv_w, lap_w, layer_w)
    if not tv_w and not lap_w and layer_w is None:
        assert head.table is eng.table and head.scale is eng.scale and head.losses is eng.losses
        assert head.tv is None and head.lap is None and not eng._heads
        return
    assert eng.head(tv_w, lap_w, layer_w) is head and list(eng._heads) == [(tv_w, lap_w, layer_w)]
    assert head.losses is not eng.losses and not head.losses.any()
    # base rows: the engine's, with the layer weights in the Gram chains' scales and 1 / numel for the content tap
    want_rows = eng.table.tolist()
    want_scale = [_fp32((1.0 if layer_w is None else layer_w[t.order]) / float(t.buf.C * t.buf.C)) for t in eng.sched.style_taps]
    want_scale += [_fp32(1.0 / float(t.buf.act.numel())) for t in eng.sched.content_taps]
    assert len(want_rows) == 6
    if layer_w is None:
        assert want_scale == eng.scale.tolist()
    # then the TV row, then one row per pool, each of kind 2 with the weight in its scale
    want_tv, want_lap = None, None
    if tv_w:
        want_tv = len(want_rows)
        want_rows.append([eng.tv_parts_off, _lib.TV_LOSS_PARTS, _lib.KIND_EXTRA])
        want_scale.append(core_model.tv_scale(tv_w, 3, H, W))
    if lap_w:
        want_lap = slice(len(want_rows), len(want_rows) + len(pools))
        for k, p in enumerate(pools):
            want_rows.append([eng.lap_parts_off + k * _lib.LAP_LOSS_PARTS, _lib.LAP_LOSS_PARTS, _lib.KIND_EXTRA])
            want_scale.append(core_model.lap_scale(lap_w, 3, H // p, W // p))
    assert head.table.dtype == torch.int32 and head.table.tolist() == want_rows
    assert head.scale.dtype == torch.float32 and head.scale.tolist() == want_scale
    assert (head.table is eng.table) == (not tv_w and not lap_w)
    assert head.losses.shape == (len(want_rows),) and head.losses.dtype == torch.float32
    assert head.tv == want_tv and head.lap == want_lap
    # the named slots, read as the model reads them, are views of exactly those rows' losses
    head.losses.copy_(torch.arange(len(want_rows), dtype=torch.float32))
    if tv_w:
        assert head.table[head.tv].tolist() == [eng.tv_parts_off, _lib.TV_LOSS_PARTS, 2] and float(head.losses[head.tv]) == 6.0
    if lap_w:
        assert head.table[head.lap, 0].tolist() == [eng.lap_parts_off + k * _lib.LAP_LOSS_PARTS for k in range(len(pools))]
        assert head.losses[head.lap].tolist() == [float(want_lap.start + k) for k in range(len(pools))]
        assert head.losses[head.lap].data_ptr() == head.losses[want_lap.start:].data_ptr()
    # the entries of the term list are those rows, in that order
    terms = eng.extra_terms(tv_w, lap_w)
    assert [t.kind for t in terms] == (["tv"] if tv_w else []) + (["lap"] * len(pools) if lap_w else [])
    assert [[t.off, t.cnt, _lib.KIND_EXTRA] for t in terms] == want_rows[6:]
    assert [_fp32(t.scale) for t in terms] == want_scale[6:]


def test_the_update_op_follows_the_accumulate_ops(monkeypatch):
    from style_transfer_visualizer_amd import optimizers
    H = W = 64
    x, grad = torch.zeros(1, 3, H, W), torch.zeros(1, 3, H, W)
    for iters, op in ((0, _lib.OP_LBFGS_STEP), (4, _lib.OP_LBFGS_ITER)):
        for tv_w in (0.0, 0.5):
            eng = _host_engine(monkeypatch, torch.bfloat16, H, W, lap_pools=(4, 16))
            fields = {f: None for f in inspect.signature(optimizers.StepRequest).parameters}
            fields.update(state=torch.zeros(8), work=torch.zeros(8), history=100, lr=1.0, tol_grad=1e-7, tol_change=1e-9,
                          iters_per_step=iters)
            _, ops_ = _step(eng, x, grad, lap_w=0.5, tv_w=tv_w, then_step=optimizers.StepRequest(**fields))
            kinds = [o.op for o in ops_]
            tail = [_lib.OP_CONV_FIRST_DGRAD] + ([_lib.OP_TV] if tv_w else []) + [_lib.OP_LAP, _lib.OP_LAP, op]
            assert kinds[-len(tail):] == tail


def test_engine_refusals(monkeypatch):
    monkeypatch.setattr(plan, "Program", RecordedProgram)
    for bad in ((3,), (0,), (64,), (4, 4), (1, 2, 4, 8, 16), (4.0,), (True,)):
        with pytest.raises(ValueError, match="lap_pools"):
            core_model.check_lap_pools(bad)
    assert core_model.check_lap_pools([4, 16]) == (4, 16) and core_model.check_lap_pools(None) == ()
    with pytest.raises(ValueError, match=r"pool size 32 leaves 1 x 2 cells of a 48 x 80 image"):
        core_model._Engine(_layers(), [0, 5], [21], 48, 80, torch.float32, CPU, assume_device=True, lap_pools=(4, 32))
    eng = core_model._Engine(_layers(), [0, 5, 10, 19, 28], [21], 64, 64, torch.float32, CPU, assume_device=True, lap_pools=(4,))
    with pytest.raises(RuntimeError, match="targets"):
        eng.loss_and_grad(torch.zeros(1, 3, 64, 64), torch.zeros(1, 3, 64, 64), 1.0, 1.0, lap_w=1.0)


# ------------------------------------------------------------------------------------------------ configuration
def _cli_config(argv):
    args = cli.build_arg_parser().parse_args(argv)
    base = stv_config.ConfigLoader.load(args.config) if args.config else None
    return stv_config.build_config_from_cli(vars(args), base_config=base)


def test_defaults():
    assert config_defaults.DEFAULT_LAP_WEIGHT == 0.0 and config_defaults.DEFAULT_LAP_POOLS == [4]
    oc = stv_config.StyleTransferConfig.model_validate({}).optimization
    assert oc.lap_w == 0.0 and oc.lap_pools == [4]
    oc = _cli_config(["--content", "c.png", "--style", "s.png"]).optimization
    assert oc.lap_w == 0.0 and oc.lap_pools == [4]


def test_cli_and_toml_round_trip(tmp_path):
    oc = _cli_config(["--content", "c.png", "--style", "s.png", "--lap-w", "100", "--lap-pool", "4,16"]).optimization
    assert oc.lap_w == 100.0 and oc.lap_pools == [4, 16]
    toml = tmp_path / "config.toml"
    toml.write_text("[optimization]\nlap_w = 0.25\nlap_pools = [2, 8]\nsteps = 7\n")
    cfg = stv_config.ConfigLoader.load(str(toml))
    assert cfg.optimization.lap_w == 0.25 and cfg.optimization.lap_pools == [2, 8] and cfg.optimization.steps == 7
    again = stv_config.StyleTransferConfig.model_validate(cfg.model_dump()).optimization
    assert again.lap_w == 0.25 and again.lap_pools == [2, 8]
    oc = _cli_config(["--config", str(toml)]).optimization                                  # TOML alone
    assert oc.lap_w == 0.25 and oc.lap_pools == [2, 8]
    oc = _cli_config(["--config", str(toml), "--lap-w", "2", "--lap-pool", "32"]).optimization      # the CLI overrides it
    assert oc.lap_w == 2.0 and oc.lap_pools == [32]
    assert stv_config._DIRECT["lap_w"] == ("optimization", "lap_w")


def test_values_outside_the_allowed_set_are_rejected(tmp_path):
    for bad in (dict(lap_w=-0.1), dict(lap_w=float("inf")), dict(lap_w=float("nan")), dict(lap_pools=[3]), dict(lap_pools=[]),
                dict(lap_pools=[64]), dict(lap_pools=[4, 4]), dict(lap_pools=[1, 2, 4, 8, 16])):
        with pytest.raises(ValueError):
            stv_config.OptimizationConfig(**bad)
    toml = tmp_path / "config.toml"
    toml.write_text("[optimization]\nlap_pools = [4, 6]\n")
    with pytest.raises(ValueError):
        stv_config.ConfigLoader.load(str(toml))
    with pytest.raises(ValueError):
        _cli_config(["--content", "c.png", "--style", "s.png", "--lap-pool", "4,5"])


def test_settings_summary_shows_the_rows_only_when_set(caplog):
    from style_transfer_visualizer_amd.type_defs import InputPaths
    paths = InputPaths(content_path="c.png", style_path="s.png")
    with caplog.at_level("INFO"):
        cli.log_parameters(paths, _cli_config(["--content", "c.png", "--style", "s.png", "--lap-pool", "4,16"]))
    assert "Laplacian" not in caplog.text
    caplog.clear()
    with caplog.at_level("INFO"):
        cli.log_parameters(paths, _cli_config(["--content", "c.png", "--style", "s.png", "--lap-w", "50", "--lap-pool", "4,16",
                                               "--tv-w", "0.5"]))
    assert "Laplacian Weight: 50" in caplog.text and "Laplacian Pool Sizes: 4,16" in caplog.text
    lines = [r.getMessage().split(":")[0] for r in caplog.records]
    assert lines.index("Laplacian Weight") == lines.index("Total Variation Weight") + 1


# ------------------------------------------------------------------------------------------------------- runner
class _Bar:
    def update(self, n=1):
        pass

    def set_postfix(self, d=None, refresh=True, **kw):
        pass

    def close(self):
        pass


def _cfg(lap_w, steps=1, **oc):
    cfg = stv_config.StyleTransferConfig.model_validate({})
    cfg.optimization.steps, cfg.optimization.style_w, cfg.optimization.content_w = steps, 2.0, 1.0
    cfg.optimization.lap_w = lap_w
    cfg.optimization.normalize = False
    cfg.video.create_video = False
    for k, v in oc.items():
        setattr(cfg.optimization, k, v)
    return cfg


class _FusedWithoutKeyword(nn.Module):
    calls = 0

    def loss_and_grad(self, x, style_w, content_w, *, tv_w=0.0):
        type(self).calls += 1
        x.grad = torch.zeros_like(x)
        z = torch.zeros(())
        return z, z, z


class _FusedWithKeyword(nn.Module):
    seen = None

    def loss_and_grad(self, x, style_w, content_w, *, tv_w=0.0, lap_w=0.0):
        type(self).seen = (tv_w, lap_w)
        x.grad = torch.zeros_like(x)
        z = torch.zeros(())
        return z, z, z


class _Plain(nn.Module):
    calls = 0

    def forward(self, x):
        type(self).calls += 1
        return [(x ** 2).mean()], [((x - 1) ** 2).mean()]


def _runner(model, cfg):
    x = torch.rand(1, 3, 6, 5, requires_grad=True)
    return OptimizationRunner(model, x, cfg, optimizer=torch.optim.SGD([x], lr=0.0), progress_bar=_Bar())


def test_fused_runner_hands_the_weight_on_or_refuses():
    _FusedWithoutKeyword.calls = 0
    with pytest.raises(ValueError, match=r"optimization\.lap_w = 0\.5.*takes no lap_w keyword"):
        _runner(_FusedWithoutKeyword(), _cfg(0.5)).run()
    assert _FusedWithoutKeyword.calls == 0                      # refused before the model is called
    _runner(_FusedWithoutKeyword(), _cfg(0.0)).run()            # weight 0: the same model runs as it always did
    assert _FusedWithoutKeyword.calls > 0
    _runner(_FusedWithKeyword(), _cfg(0.5)).run()
    assert _FusedWithKeyword.seen == (0.0, 0.5)
    _runner(_FusedWithKeyword(), _cfg(0.0)).run()
    assert _FusedWithKeyword.seen == (0.0, 0.0)


def test_non_fused_runner_refuses_instead_of_dropping_the_term():
    _Plain.calls = 0
    with pytest.raises(ValueError, match=r"lap_w = 0\.75"):
        _runner(_Plain(), _cfg(0.75)).run()
    _runner(_Plain(), _cfg(0.0)).run()
    assert _Plain.calls > 0


class _Model(nn.Module):
    """Stands in for StyleContentModel on the CPU: records what it is given."""

    built: list = []

    def __init__(self, style_layers, content_layers, precision=None, **kw):
        super().__init__()
        self.kw = kw
        type(self).built.append(self)

    def set_targets(self, style, content, **kw):
        self.content = content

    def forward(self, x):
        return [(x.mean()) ** 2], [((x - self.content) ** 2).mean()]


def test_prepare_passes_the_pools_only_when_the_weight_is_set(monkeypatch):
    _Model.built = []
    monkeypatch.setattr(core_model, "StyleContentModel", _Model)
    content, style = torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16)
    core_model.prepare_model_and_input(content, style, CPU, _cfg(0.0).optimization)
    assert _Model.built[-1].kw == {}
    core_model.prepare_model_and_input(content, style, CPU, _cfg(0.0, lap_pools=[4, 16]).optimization)
    assert _Model.built[-1].kw == {}                            # pools without a weight: no keyword either
    core_model.prepare_model_and_input(content, style, CPU, _cfg(3.0, lap_pools=[4, 16]).optimization)
    assert _Model.built[-1].kw == {"lap_pools": [4, 16]}
    assert core_model.lap_option_kwargs(object()) == {}         # settings objects from before the option


def test_model_refusals_come_before_any_launch(monkeypatch):
    monkeypatch.setattr(core_model, "initialize_vgg", lambda: core_model.build_vgg_features().eval())
    with pytest.raises(ValueError, match="lap_pools"):
        core_model.StyleContentModel([0, 5], [21], lap_pools=[3])
    plain = core_model.StyleContentModel([0, 5], [21])
    assert plain.lap_pools == () and plain.last_lap_terms() is None
    x = torch.zeros(1, 3, 16, 16)
    for bad, text in ((-1.0, "lap_w must be a finite weight >= 0, got -1.0"), (float("inf"), "got inf"), (float("nan"), "got nan")):
        with pytest.raises(ValueError, match=text):
            plain.loss_and_grad(x, 1.0, 1.0, lap_w=bad)
    with pytest.raises(ValueError, match=r"lap_w = 0\.5, but the model was built without lap_pools"):
        plain.loss_and_grad(x, 1.0, 1.0, lap_w=0.5)
    model = core_model.StyleContentModel([0, 5], [21], lap_pools=[4, 16])
    assert model.lap_pools == (4, 16)
    with pytest.raises(ValueError, match=r"pool size 16 leaves 1 x 3 cells of a 24 x 48 image"):
        model.set_targets(torch.zeros(1, 3, 24, 48), torch.zeros(1, 3, 24, 48))      # (before the engine asks for a GPU tensor)
    assert "lap_w" in inspect.signature(model.loss_and_grad).parameters


def test_pyramid_refuses_a_pool_too_large_for_the_coarsest_level(monkeypatch):
    # (with the run's own minimum dimension of 64 every allowed pool fits; the check is exercised below that)
    monkeypatch.setattr(pyramid, "MIN_DIMENSION", 8)
    cfg = _cfg(1.0, steps=4, lap_pools=[4, 16], pyramid_levels=3)
    content, style = torch.zeros(1, 3, 64, 96), torch.zeros(1, 3, 64, 64)
    with pytest.raises(ValueError, match=r"pool size 16 leaves 1 x 1 cells of a 16 x 24 image \(the coarsest of 3 pyramid levels\)"):
        pyramid.run_pyramid(content, style, CPU, cfg)
    cfg.optimization.lap_w = 0.0                                # off: the pools are not looked at
    assert pyramid._validate(content, style, cfg, None, None)[0] == 3


def test_every_pyramid_level_builds_its_model_with_the_pools(monkeypatch):
    from style_transfer_visualizer_amd import ops

    class _FusedModel(_Model):
        def loss_and_grad(self, x, style_w, content_w, *, lap_w=0.0):
            self.lap_w = lap_w
            x.grad = torch.zeros_like(x)
            z = torch.zeros(())
            return z, z, z

    def resize2x(x, mode, out=None):
        x = x.detach()
        if mode == _lib.RESIZE_DOWN2:
            return torch.nn.functional.avg_pool2d(x, 2)
        return torch.nn.functional.interpolate(x, scale_factor=2, mode="nearest")
    _Model.built = []
    monkeypatch.setattr(core_model, "StyleContentModel", _FusedModel)
    monkeypatch.setattr(ops, "resize2x", resize2x)
    content, style = torch.rand(1, 3, 128, 128), torch.rand(1, 3, 128, 128)
    cfg = _cfg(7.0, steps=2, lap_pools=[4, 16], pyramid_levels=2, init_method="content")
    pyramid.run_pyramid(content, style, CPU, cfg, optimizer_factory=lambda x: torch.optim.SGD([x], lr=0.1), progress_bar=_Bar())
    coarse, fine = _Model.built
    assert coarse.kw == fine.kw == {"lap_pools": [4, 16]} and coarse.lap_w == fine.lap_w == 7.0
    assert tuple(coarse.content.shape[-2:]) == (64, 64) and tuple(fine.content.shape[-2:]) == (128, 128)      # its own content
    _Model.built = []
    cfg = _cfg(0.0, steps=2, lap_pools=[4, 16], pyramid_levels=2, init_method="content")
    pyramid.run_pyramid(content, style, CPU, cfg, optimizer_factory=lambda x: torch.optim.SGD([x], lr=0.1), progress_bar=_Bar())
    assert [m.kw for m in _Model.built] == [{}, {}]


# --------------------------------------------------------------------------------------------------- row strips
@pytest.mark.parametrize("cls", [spatial.HaloShard, spatial.SpatialShard])
def test_row_strips_refuse_the_term(cls):
    with pytest.raises(ValueError, match="Laplacian"):
        cls([], [], [], torch.zeros(1, 3, 16, 16), [], dtype=torch.float32, style_w=1.0, content_w=1.0, lap_w=0.5)
