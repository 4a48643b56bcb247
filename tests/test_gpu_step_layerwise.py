"""Layer-wise parity of the composed step on the GPU: every tap layout, switch arm and precision that
``Schedule._decide`` distinguishes, at the smallest sizes that still have every structure.

Every case evaluates one step with one tensor per gradient and every activation stored (STV_GRAD_ARENA=0,
STV_SKIP_PREPOOL=0, no graph replay) and hands the engine to ``tests.layerwise.check_step``: each stored activation,
arg-max byte map, Gram seed, score, activation gradient and the image gradient must lie in the interval derived for it
from the float64 oracle op on the kernel's own stored inputs (tests/layerwise.py; proved on a CPU stand-in, with
mutations, in tests/test_layerwise_host.py).  The matrix cases then run the product's defaults (gradient slabs, dead
pre-pool maps not stored, graph replay) and require bit-identical scores, image gradient and stored tensors.  Every
case asserts the schedule decisions it exists for.  Weights carry a non-zero bias per layer.

The structures that joined the step later - average pooling, spatial guidance (one Gram chain and one gradient term per
region), style layer weights, the Laplacian terms - run as the rows of ``lw.STEP_CASES`` through the same three steps:
checked run, decisions, product defaults.  Their sizes: 40x24 (odd pooled maps: rows and columns an average pool drops),
64x48 (three regions all present at the 4x3 tap), 42x26 (image rows and columns outside the Laplacian's cells).

Sizes: 64x48 (non-square, four pools down to 4x3), 32x32 (the deepest map is 2x2), 40x24 (pooled maps become odd: 5x3
in front of the fourth pool, whose backward can then not ride in a dgrad - routed and unrouted pools in one schedule).
"""
from __future__ import annotations

import functools

import pytest
import torch

from style_transfer_visualizer_amd import _lib, core_model, guidance, synthetic
from tests import layerwise as lw
from tests.conftest import record_parity

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
STYLE_W, CONTENT_W = 1e5, 1.0
SIZE_OF = {"default": (40, 24), "content7": (32, 32), "prepool": (40, 24), "content_first": (32, 32),
           "two_content": (64, 48), "shared_buffer": (32, 32), "relu_taps": (64, 48), "pool_taps": (40, 24)}
# What _decide makes of each layout at its size (layer numbers): the convs whose dgrad routes a pooling backward (bf16
# only), the convs whose dgrad carries a Gram product, the pools that run as a pass of their own.
DECISIONS = {
    "default": dict(routes=[5, 10, 19], gram=[2, 7, 12, 21], own_pools=[]),         # the fourth pool (5x3 -> 2x1) is not routed
    "content7": dict(routes=[5, 19, 28], gram=[2, 7, 12, 21], own_pools=[9]),       # a content tap in front of the second pool
    "prepool": dict(routes=[], gram=[], own_pools=[4, 9, 18]),                      # every conv in front of a pool is tapped
    "content_first": dict(routes=[5, 10, 19, 28], gram=[], own_pools=[]),
    "two_content": dict(routes=[5, 10, 19, 28], gram=[], own_pools=[]),
    "shared_buffer": dict(routes=[5, 10, 19], gram=[2, 7], own_pools=[]),
    "relu_taps": dict(routes=[5, 10, 19], gram=[2], own_pools=[]),
    "pool_taps": dict(routes=[], gram=[5, 10], own_pools=[]),                       # a tapped pooled map is never routed over
}
CHECK_ENV = {"STV_GRAD_ARENA": "0", "STV_SKIP_PREPOOL": "0", "STV_HIP_GRAPH": "0"}


@functools.cache
def _weights(cfg: tuple) -> list:
    return lw.biased_weights(cfg)


@functools.cache
def _images(H: int, W: int) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    x0 = synthetic.synthetic_image(2, H, W) + 0.25 * torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(5))
    return synthetic.synthetic_image(1, H, W), synthetic.synthetic_image(0, H, W), x0.contiguous()


def _model(monkeypatch, layout, precision: str, H: int, W: int, cfg: tuple = synthetic.VGG19_CFG, **env):
    """A model with targets set, and a fresh leaf image on the device."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    weights = _weights(cfg)
    monkeypatch.setattr(core_model, "initialize_vgg", lambda: core_model.build_vgg_features(weights, cfg).eval())
    model = core_model.StyleContentModel(list(layout[0]), list(layout[1]), precision=precision).to(DEV)
    style, content, x0 = _images(H, W)
    model.set_targets(style.to(DEV), content.to(DEV))
    return model, x0.to(DEV).requires_grad_(True), x0


def _engine(model):
    return next(iter(model._engines.values()))


def _fused_program(eng):
    return next(p for k, p in eng._programs.items() if k[0] == "fused")


def _checked_step(monkeypatch, case: str, layout, precision: str, H: int, W: int, *, tv_w: float = 0.0,
                  cfg: tuple = synthetic.VGG19_CFG, **env):
    model, x, x0 = _model(monkeypatch, layout, precision, H, W, cfg, **{**CHECK_ENV, **env})
    scores = tuple(float(v) for v in model.loss_and_grad(x, STYLE_W, CONTENT_W, tv_w=tv_w))
    torch.cuda.synchronize()
    eng = _engine(model)
    lw.check_step(eng, x0, style_w=STYLE_W, content_w=CONTENT_W, x_grad=x.grad, tv_w=tv_w, record=record_parity, case=case)
    return model, eng, x, scores


def _ops(prog, op: int) -> list[int]:
    return [i for i, m in enumerate(prog.op_meta) if m[0] == op]


def _flagged(prog, flag: int) -> list[int]:
    return [i for i, f in enumerate(prog.op_flags) if f & flag and prog.op_meta[i][0] in (_lib.OP_CONV, _lib.OP_POOL_BWD)]


# ------------------------------------------------------------------------------------------- layouts x precisions
@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("layout", list(lw.LAYOUTS))
def test_every_stored_tensor_of_the_step(layout, precision, monkeypatch):
    H, W = SIZE_OF[layout]
    taps = lw.LAYOUTS[layout]
    case = f"step {layout} {H}x{W} {precision}"
    model, eng, x, scores = _checked_step(monkeypatch, case, taps, precision, H, W)
    nodes = eng.sched.nodes
    # the decisions this layout exists for
    want = DECISIONS[layout]
    assert [nd.layer for nd in nodes if nd.route is not None] == (want["routes"] if precision == "bf16" else [])
    assert [nd.layer for nd in nodes if nd.gram is not None] == want["gram"]
    assert [nd.layer for nd in nodes if nd.kind == "pool" and not nd.fused] == want["own_pools"]
    assert all((nd.idx is not None) == nd.fused for nd in nodes if nd.kind == "pool")
    if layout == "default" and precision == "bf16":      # routed pools and one that runs from its byte map, in one schedule
        prog = _fused_program(eng)
        assert len(_flagged(prog, _lib.POOL_ROUTE)) == 3 and len(_ops(prog, _lib.OP_POOL_BWD)) == 1
    if layout == "relu_taps":
        assert [nd.layer for nd in nodes if nd.kind == "relu"] == [1]
        assert [nd.layer for nd in nodes if nd.dst.relu_fused and nd.dst.taps] == [5, 10, 21]
    if layout == "pool_taps":
        tapped = [nd for nd in nodes if nd.dst.taps]
        assert [(nd.layer, nd.kind) for nd in tapped] == [(4, "pool"), (9, "pool"), (18, "pool")]
    if layout == "shared_buffer":
        assert sorted(t.kind for t in next(nd for nd in nodes if nd.layer == 5).dst.taps) == ["content", "style"]
    if layout in ("content_first", "two_content"):
        assert [t.kind for t in nodes[0].dst.taps] == ["content"]
    if layout == "prepool":
        assert not nodes[0].dst.relu_fused and not nodes[0].dst.taps and nodes[1].relu_in     # ReLU by the consumer
    assert all(t.grad_fused for t in eng.sched.content_taps)
    # ---- the product's defaults: gradient slabs, dead pre-pool maps not stored, graph replay
    model2, x2, _ = _model(monkeypatch, taps, precision, H, W, STV_GRAD_ARENA="1", STV_SKIP_PREPOOL="1", STV_HIP_GRAPH="1")
    scores2 = tuple(float(v) for v in model2.loss_and_grad(x2, STYLE_W, CONTENT_W))
    torch.cuda.synchronize()
    eng2 = _engine(model2)
    assert eng2.use_graph and eng2.sched.grad_arena
    assert scores2 == scores
    assert torch.equal(x2.grad, x.grad)
    skipped = 0
    for nd, nd2 in zip(nodes, eng2.sched.nodes, strict=True):
        if nd2.dst.stored:
            assert torch.equal(nd.dst.act, nd2.dst.act), f"L{nd.layer:02d} {nd.kind}: stored activation differs"
        skipped += not nd2.dst.stored
        assert (nd.idx is None) == (nd2.idx is None)
        if nd.idx is not None:
            assert torch.equal(nd.idx, nd2.idx), f"L{nd.layer:02d}: arg-max map differs"
    for t, t2 in zip(eng.sched.style_taps, eng2.sched.style_taps, strict=True):
        assert torch.equal(t.sgrad, t2.sgrad), f"style tap {t.order}: seed differs"
    assert skipped == (sum(1 for nd in nodes if nd.kind == "pool" and nd.fused) if precision == "bf16" else 0)
    record_parity(case, "product defaults vs the checked run", 0.0, 0.0,
                  f"bit-identical scores, image gradient, seeds, {len(nodes) - skipped} activations, byte maps; "
                  f"{skipped} pre-pool maps not stored, {eng2.sched._grad_slabs.shape[0]} gradient slabs")


# ------------------------------------------------------------------------------------------------ the narrow nets
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_narrow_net_takes_the_direct_conv_path(precision, monkeypatch):
    """(bf16x3 has no direct kernel: a shape off the matrix-core tiling is an error there.)"""
    case = f"step narrow 40x24 {precision}"
    model, eng, x, _ = _checked_step(monkeypatch, case, lw.NARROW_LAYOUT, precision, 40, 24, cfg=lw.NARROW_CFG[precision])
    lw.assert_narrow_branches(eng)
    prog = _fused_program(eng)
    assert _ops(prog, _lib.OP_POOL_FWD) and _ops(prog, _lib.OP_POOL_BWD)
    convs = [i for i in _ops(prog, _lib.OP_CONV) if prog.op_meta[i][5] == 9]
    assert any(prog.op_flags[i] & _lib.W_BLOCKED for i in convs) and any(not prog.op_flags[i] & _lib.W_BLOCKED for i in convs)


# -------------------------------------------------------------------------------------------------- switch arms
def _arm_fuse_pool(prog, eng, precision):
    assert len(_ops(prog, _lib.OP_POOL_FWD)) == 4 and not any(nd.fused for nd in eng.sched.nodes)


def _arm_pool_idx(prog, eng, precision):
    assert not _flagged(prog, _lib.POOL_IDX) and not _flagged(prog, _lib.POOL_ROUTE)
    assert len(_ops(prog, _lib.OP_POOL_BWD)) == 4 and any(nd.fused for nd in eng.sched.nodes)


def _arm_fuse_pool_bwd(prog, eng, precision):
    assert not _flagged(prog, _lib.POOL_ROUTE) and len(_flagged(prog, _lib.POOL_IDX)) == 4


def _arm_fuse_gram(prog, eng, precision):
    assert sum(1 for i in _ops(prog, _lib.OP_CONV) if prog.op_meta[i][5] == 1) == 5 and all(nd.gram is None for nd in eng.sched.nodes)


def _arm_w_blocked(prog, eng, precision):
    assert not _flagged(prog, _lib.W_BLOCKED) and all(nd.wf.dim() == 3 for nd in eng.sched.nodes if nd.kind == "conv")


def _arm_fuse_content(prog, eng, precision):
    assert len(_ops(prog, _lib.OP_CONTENT_GRAD)) == len(eng.sched.content_taps) and not any(t.grad_fused for t in eng.sched.content_taps)


def _arm_loss_batch_0(prog, eng, precision):
    assert not _ops(prog, _lib.OP_GRAM_MULTI) and len(_ops(prog, _lib.OP_GRAM_FINISH)) == len(eng.sched.style_taps)
    last_conv = max(i for i in _ops(prog, _lib.OP_CONV) if i < _ops(prog, _lib.OP_LOSS_COMBINE)[0])
    assert min(_ops(prog, _lib.OP_GRAM_FINISH)) < last_conv          # behind their producers


def _arm_loss_batch_1(prog, eng, precision):
    (multi,) = _ops(prog, _lib.OP_GRAM_MULTI)
    assert prog.op_meta[multi][6] == len(eng.sched.style_taps) and not _ops(prog, _lib.OP_GRAM_FINISH)


def _arm_gram_fin_late(prog, eng, precision):
    # no tap of these sizes is too large for the batched tail (48 MiB), so no finish pass is left to move: the arm runs
    # the default's ops - asserted, so that the row cannot be read as coverage of a late finish
    assert all(t.in_tail and not t.finish_late for t in eng.sched.style_taps) and len(_ops(prog, _lib.OP_GRAM_MULTI)) == 1


def _arm_loss_interleave(prog, eng, precision):
    combine = _ops(prog, _lib.OP_LOSS_COMBINE)[0]
    last_conv = max(i for i in _ops(prog, _lib.OP_CONV) if i < combine)
    head = [i for i in range(combine) if prog.op_meta[i][0] in (_lib.OP_CONTENT_LOSS, _lib.OP_GRAM_PARTIAL, _lib.OP_GRAM_FINISH, _lib.OP_GRAM_MULTI)]
    assert head and min(head) > last_conv and not eng.sched.interleave


def _arm_gram_first_0(prog, eng, precision):
    assert not eng.sched.style_taps[0].partials_fused


def _arm_gram_first_2(prog, eng, precision):
    assert eng.sched.style_taps[0].partials_fused == (precision == "bf16")


ARMS = {
    "STV_FUSE_POOL=0": (_arm_fuse_pool, ["default"], ["fp32", "bf16"]),
    "STV_POOL_IDX=0": (_arm_pool_idx, ["default"], ["fp32", "bf16"]),
    "STV_FUSE_POOL_BWD=0": (_arm_fuse_pool_bwd, ["default"], ["fp32", "bf16"]),
    "STV_FUSE_GRAM=0": (_arm_fuse_gram, ["default"], ["fp32", "bf16"]),
    "STV_W_BLOCKED=0": (_arm_w_blocked, ["default"], ["fp32", "bf16"]),
    "STV_FUSE_CONTENT=0": (_arm_fuse_content, ["default", "two_content"], ["fp32", "bf16"]),
    "STV_LOSS_BATCH=0": (_arm_loss_batch_0, ["default"], ["fp32", "bf16"]),
    "STV_LOSS_BATCH=1": (_arm_loss_batch_1, ["default"], ["fp32", "bf16"]),
    "STV_GRAM_FIN_LATE=0": (_arm_gram_fin_late, ["default"], ["fp32", "bf16"]),
    # (with every style tap batched the loss head sits in the tail either way: the arm moves ops where taps keep their place
    # behind their producers - one style tap, nothing to batch)
    "STV_LOSS_INTERLEAVE=0": (_arm_loss_interleave, ["default", "content_first"], ["fp32", "bf16"]),
    "STV_FUSE_GRAM_FIRST=0": (_arm_gram_first_0, ["default"], ["fp32", "bf16"]),
    "STV_FUSE_GRAM_FIRST=2": (_arm_gram_first_2, ["default"], ["fp32", "bf16"]),
}
ARM_CASES = [(arm, layout, precision) for arm, (_, layouts, precisions) in ARMS.items() for layout in layouts for precision in precisions]


@pytest.mark.parametrize(("arm", "layout", "precision"), ARM_CASES, ids=lambda v: v)
def test_switch_arm_against_the_oracle(arm, layout, precision, monkeypatch):
    name, value = arm.split("=")
    H, W = (32, 32) if layout == "default" else SIZE_OF[layout]
    _, eng, _, _ = _checked_step(monkeypatch, f"arm {arm} {layout} {H}x{W} {precision}", lw.LAYOUTS[layout], precision, H, W, **{name: value})
    ARMS[arm][0](_fused_program(eng), eng, precision)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_gradient_slabs_with_pooling_backward_in_the_chain(precision, monkeypatch):
    """STV_GRAD_ARENA=1 against 0 under STV_FUSE_POOL_BWD=0: the pooling backward passes are ops of the reverse chain, so
    pooled-resolution gradients take slabs too (every op of the chain reads one gradient and writes one: the walk of
    ``alloc_grads`` needs two slabs, with or without them).  The one-tensor-per-gradient run is checked against the oracle;
    the rotating run must reproduce it bit for bit (scores, image gradient, stored activations, the gradients of the
    slabs' last writers)."""
    H, W = 32, 32
    taps = lw.LAYOUTS["default"]
    case = f"arm STV_GRAD_ARENA=1 (pool bwd in chain) {H}x{W} {precision}"
    model, eng, x, scores = _checked_step(monkeypatch, case, taps, precision, H, W, STV_FUSE_POOL_BWD="0")
    assert len(_ops(_fused_program(eng), _lib.OP_POOL_BWD)) == 4
    model2, x2, _ = _model(monkeypatch, taps, precision, H, W, STV_GRAD_ARENA="1", STV_SKIP_PREPOOL="0", STV_HIP_GRAPH="0", STV_FUSE_POOL_BWD="0")
    scores2 = tuple(float(v) for v in model2.loss_and_grad(x2, STYLE_W, CONTENT_W))
    torch.cuda.synchronize()
    eng2 = _engine(model2)
    assert eng2.sched.grad_arena and eng2.sched._grad_slabs.shape[0] == 2
    in_slabs = [nd.layer for nd in eng2.sched.nodes if id(nd.dst) in eng2.sched._grad_slab_of]
    assert [nd.layer for nd in eng2.sched.nodes if nd.kind == "pool"] == [4, 9, 18, 27] and {4, 9, 18, 27} <= set(in_slabs)
    assert len(_ops(_fused_program(eng2), _lib.OP_POOL_BWD)) == 4
    assert scores2 == scores and torch.equal(x2.grad, x.grad)
    for nd, nd2 in zip(eng.sched.nodes, eng2.sched.nodes, strict=True):
        assert torch.equal(nd.dst.act, nd2.dst.act)
    # the first two buffers of the chain are the last writers of the two slabs
    for nd, nd2 in zip(eng.sched.nodes[:2], eng2.sched.nodes[:2], strict=True):
        assert torch.equal(nd.dst.grad, nd2.dst.grad), f"L{nd.layer:02d}: gradient differs"
    record_parity(case, "rotating gradients vs the checked run", 0.0, 0.0, "bit-identical scores, image gradient, activations, last writers")


# ------------------------------------------------------------------------------------------------ autograd path
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("layout", ["default", "shared_buffer"])
def test_autograd_path_with_a_coefficient_per_loss(layout, precision, monkeypatch):
    H, W = 32, 32
    taps = lw.LAYOUTS[layout]
    model, x, x0 = _model(monkeypatch, taps, precision, H, W, **CHECK_ENV)
    n = len(taps[0]) + len(taps[1])
    for rnd, base in enumerate((3e4, 7e3)):              # the second evaluation reuses the cached forward program
        gout = [base * (1.0 + 0.37 * ((i + rnd) % n)) for i in range(n)]
        x.grad = None
        style, content = model(x)
        total = sum(w * v for w, v in zip(gout, list(style) + list(content)))
        total.backward()
        torch.cuda.synchronize()
        eng = _engine(model)
        # (the backward program is keyed by the address of the gradient autograd allocates: one per address)
        assert [k[0] for k in eng._programs].count("fwd") == 1 and {k[0] for k in eng._programs} == {"fwd", "bwd"}
        lw.check_step(eng, x0, style_w=1.0, content_w=1.0, x_grad=x.grad, gout=gout, record=record_parity,
                      case=f"autograd {layout} {H}x{W} {precision} #{rnd}")
    prog = next(p for k, p in eng._programs.items() if k[0] == "bwd")
    assert len(_ops(prog, _lib.OP_GRAM_FINISH)) == len(taps[0]) and len(_ops(prog, _lib.OP_CONTENT_GRAD)) == len(taps[1])


# --------------------------------------------------------------------------------------------- total variation
def test_total_variation_term_joins_the_checked_image_gradient(monkeypatch):
    """The image gradient is the checked first-layer dgrad plus the float64 TV gradient (tests/tv_ref.py), within the
    bound of test_gpu_tv_model.py::test_kernel_against_float64 and one fp32 add; the total carries the term."""
    _, eng, _, _ = _checked_step(monkeypatch, "step default 32x32 bf16 tv_w=50", lw.LAYOUTS["default"], "bf16", 32, 32, tv_w=50.0)
    prog = _fused_program(eng)
    assert len(_ops(prog, _lib.OP_TV)) == 2 and _ops(prog, _lib.OP_TV)[1] == _ops(prog, _lib.OP_CONV_FIRST_DGRAD)[0] + 1


# ------------------------------------- average pooling, spatial guidance, layer weights, Laplacian terms (lw.STEP_CASES)
def _case_model(monkeypatch, name: str, precision: str, **env):
    """The model of one ``lw.STEP_CASES`` row with targets set, a fresh leaf image on the device, the host image."""
    spec = lw.STEP_CASES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    weights = _weights(synthetic.VGG19_CFG)
    monkeypatch.setattr(core_model, "initialize_vgg", lambda: core_model.build_vgg_features(weights, synthetic.VGG19_CFG).eval())
    style_at, content_at = lw.case_layout(spec)
    H, W = spec["size"]
    R = spec.get("regions", 0)
    kw = {}
    if R:
        kw.update(guide_regions=R, region_weights=list(lw.REGION_WEIGHTS[R]))
    if "layer_w" in spec:
        kw["style_layer_weights"] = list(spec["layer_w"])
    if "lap_pools" in spec:
        kw["lap_pools"] = spec["lap_pools"]
    model = core_model.StyleContentModel(list(style_at), list(content_at), precision=precision, pooling=spec.get("pooling", "max"), **kw).to(DEV)
    style, content, x0 = _images(H, W)
    labels = {}
    if R:
        content_labels, style_labels = lw.guide_labels(R, H, W)
        labels = dict(content_labels=content_labels, style_labels=style_labels)
        # the label maps by the model's own down-sampling: every region present at every tap, the deepest (4x3) included
        for which in (content_labels, style_labels):
            shapes = guidance.tap_shapes(H, W, synthetic.VGG19_CFG, style_at)
            counts = guidance.check_counts(guidance.tap_maps(which, shapes), R, "content")
            assert all(min(row) >= 1 for row in counts) and bool((which == guidance.NO_REGION).any())
    model.set_targets(style.to(DEV), content.to(DEV), **labels)
    return model, x0.to(DEV).requires_grad_(True), x0


def _step(model, x, spec) -> tuple:
    scores = tuple(float(v) for v in model.loss_and_grad(x, STYLE_W, CONTENT_W, tv_w=spec.get("tv_w", 0.0), lap_w=spec.get("lap_w", 0.0)))
    torch.cuda.synchronize()
    return scores


def _op_at(prog, i: int) -> int:
    return prog.op_meta[i][0]


def _assert_avg(prog, eng, name):
    nodes = eng.sched.nodes
    pools = [nd for nd in nodes if nd.kind in ("pool", "avgpool")]
    assert pools and all(nd.kind == "avgpool" and not nd.fused and nd.idx is None for nd in pools)
    assert all(nd.route is None for nd in nodes) and all(nd.dst.stored for nd in nodes)
    assert len(_ops(prog, _lib.OP_AVGPOOL_FWD)) == len(_ops(prog, _lib.OP_AVGPOOL_BWD)) == len(pools)
    assert not _ops(prog, _lib.OP_POOL_FWD) and not _ops(prog, _lib.OP_POOL_BWD)
    for nd in pools:                     # rows and columns the floor drops, as the only writer: +0
        s = nd.src
        if not s.taps and (s.H % 2 or s.W % 2):
            assert not bool(s.grad[2 * (s.H // 2):].any()) and not bool(s.grad[:, 2 * (s.W // 2):].any())
    accum = [i for i in _ops(prog, _lib.OP_AVGPOOL_BWD) if prog.op_flags[i] & _lib.ACCUM]
    if name == "avg default":
        assert any(nd.src.H % 2 and nd.src.W % 2 and not nd.src.taps for nd in pools) and not accum
    if name == "avg pending relu":      # (the layout ends at layer 7: one pool, behind the tapped conv 2)
        assert [nd.relu_in for nd in pools] == [True]
    if name == "avg content7":
        assert [nd.layer for nd in pools if nd.relu_in] == [9] and len(pools) == 4
    if name == "avg pool taps":
        assert [(nd.layer, nd.kind) for nd in nodes if nd.dst.taps] == [(4, "avgpool"), (9, "avgpool"), (18, "avgpool")]
    if name == "avg shared buffer":     # the dgrad of conv 7 accumulates onto the content gradient the forward half wrote
        assert any(prog.op_flags[i] & _lib.ACCUM for i in _ops(prog, _lib.OP_CONV) if prog.op_meta[i][5] == 9)
    if name == "avg prepool":           # and here the pool's own backward does
        assert len(accum) >= 1 and all(t.grad_fused for t in eng.sched.content_taps)


def _assert_guided(prog, eng, rep, name):
    s, R = eng.sched, eng.guide.n
    products = [i for i in _ops(prog, _lib.OP_CONV) if prog.op_meta[i][5] == 1]
    assert len(_ops(prog, _lib.OP_MASK_SPLIT)) == len(s.style_taps) and len(products) == R * len(s.style_taps)
    assert all(nd.gram is None for nd in s.nodes) and not any(t.partials_fused for t in s.style_taps)
    multi = [prog.op_meta[i][6] for i in _ops(prog, _lib.OP_GRAM_MULTI)]
    chains = R * len(s.style_taps)
    assert multi == [min(8, chains - k) for k in range(0, chains, 8)] and len(s.all_chains()) == chains
    if name == "guided R=3":
        assert multi == [8, 7]
    tapped = {f"grad L{nd.layer:02d} {nd.kind}" for nd in s.nodes if any(t.kind == "style" for t in nd.dst.taps)
              and (R > 1 or nd is not s.nodes[-1])}
    assert tapped <= set(rep.multi_stage)
    # only the very first product of the chain (the deepest tap's first region) stores
    assert [bool(prog.op_flags[i] & _lib.ACCUM) for i in products] == [bool(s.nodes[-1].dst.taps[0].kind != "style")] + [True] * (len(products) - 1)
    if name == "guided relu taps":      # one in-place mask per tapped ReLU output, behind the last of its R products
        masked = [nd.layer for nd in s.nodes if nd.dst.relu_fused and any(t.kind == "style" for t in nd.dst.taps)]
        behind = [i for i in _ops(prog, _lib.OP_RELU_BWD) if all(j in products for j in range(i - R, i))]
        relus = [nd.layer for nd in s.nodes if nd.kind == "relu"]     # (the backward of the materialised ReLU follows its output's products too)
        assert masked == [5, 10] and relus == [1] and len(behind) == 3 and all(i + 1 not in products for i in behind)
        assert len(_ops(prog, _lib.OP_RELU_BWD)) == 4                  # and the mask behind the content term of conv 21
    if name == "guided shared buffer":  # content gradient written in the forward half, then the dgrad and R products accumulate
        shared = next(nd for nd in s.nodes if nd.layer == 5).dst
        assert sorted(t.kind for t in shared.taps) == ["content", "style"] and all(t.grad_fused for t in s.content_taps)
        assert any(prog.op_flags[i] & _lib.ACCUM for i in _ops(prog, _lib.OP_CONV) if prog.op_meta[i][5] == 9)


def _assert_lap(prog, eng, spec):
    tv = 1 if spec.get("tv_w") else 0
    n = len(spec["lap_pools"])
    lap, dgrad = _ops(prog, _lib.OP_LAP), _ops(prog, _lib.OP_CONV_FIRST_DGRAD)[0]
    assert len(lap) == 2 * n and lap[:n] == list(range(tv, tv + n))                      # LOSS forms at the head, behind TV's
    assert lap[n:] == list(range(dgrad + 1 + tv, dgrad + 1 + tv + n))                    # GRAD forms behind the dgrad and TV
    assert all(prog.op_meta[i][5] == _lib.LAP_LOSS for i in lap[:n]) and all(prog.op_meta[i][5] == _lib.LAP_GRAD for i in lap[n:])
    assert all(prog.op_flags[i] & _lib.ACCUM for i in lap[n:]) and [prog.op_meta[i][4] for i in lap[n:]] == list(spec["lap_pools"])
    if tv:
        assert _ops(prog, _lib.OP_TV) == [0, dgrad + 1]


@pytest.mark.parametrize(("name", "precision"), lw.STEP_PARAMS, ids=lambda v: v.replace(" ", "-"))
def test_every_stored_tensor_of_the_new_structures(name, precision, monkeypatch):
    spec = lw.STEP_CASES[name]
    H, W = spec["size"]
    case = f"step {name} {H}x{W} {precision}"
    model, x, x0 = _case_model(monkeypatch, name, precision, **CHECK_ENV)
    scores = _step(model, x, spec)
    eng = _engine(model)
    rep = lw.check_step(eng, x0, style_w=STYLE_W, content_w=CONTENT_W, x_grad=x.grad, tv_w=spec.get("tv_w", 0.0),
                        lap_w=spec.get("lap_w", 0.0), layer_w=spec.get("layer_w"), record=record_parity, case=case)
    grad = x.grad.clone()
    regions = model.last_region_losses().clone() if eng.guide is not None else None
    prog = _fused_program(eng)
    # ---- the decisions this case exists for
    if spec.get("pooling") == "avg":
        _assert_avg(prog, eng, name)
    if eng.guide is not None:
        _assert_guided(prog, eng, rep, name)
    if "layer_w" in spec:                # the zero-weight tap: every seed of it is a zero
        for c in eng.sched.all_chains():
            parent = c.parent if c.parent is not None else c
            assert bool((c.sgrad == 0).all()) == (spec["layer_w"][parent.order] == 0.0)
    if "lap_pools" in spec:
        _assert_lap(prog, eng, spec)
        # pixels outside every pool's cells carry the dgrad (+ TV) value bit for bit: the same step without the term
        model.loss_and_grad(x, STYLE_W, CONTENT_W, tv_w=spec.get("tv_w", 0.0))
        torch.cuda.synchronize()
        outside = torch.ones(H, W, dtype=torch.bool, device=DEV)
        for p in spec["lap_pools"]:
            outside[:H // p * p, :W // p * p] = False
        assert torch.equal(x.grad[..., outside], grad[..., outside])
        assert bool(outside.any()) == all(H % p or W % p for p in spec["lap_pools"])
        assert not torch.equal(x.grad, grad)
    # ---- the product's defaults: gradient slabs, dead pre-pool maps not stored, graph replay
    model2, x2, _ = _case_model(monkeypatch, name, precision, STV_GRAD_ARENA="1", STV_SKIP_PREPOOL="1", STV_HIP_GRAPH="1")
    scores2 = _step(model2, x2, spec)
    eng2 = _engine(model2)
    assert eng2.use_graph and eng2.sched.grad_arena
    assert scores2 == scores
    assert torch.equal(x2.grad, grad)
    skipped = 0
    for nd, nd2 in zip(eng.sched.nodes, eng2.sched.nodes, strict=True):
        if nd2.dst.stored:
            assert torch.equal(nd.dst.act, nd2.dst.act), f"L{nd.layer:02d} {nd.kind}: stored activation differs"
        skipped += not nd2.dst.stored
    for t, t2 in zip(eng.sched.all_chains(), eng2.sched.all_chains(), strict=True):
        assert torch.equal(t.sgrad, t2.sgrad), f"Gram chain {t.order}: seed differs"
    if eng.guide is not None:
        for t, t2 in zip(eng.sched.style_taps, eng2.sched.style_taps, strict=True):
            assert torch.equal(t.slabs, t2.slabs), f"style tap {t.order}: region slabs differ"
        assert torch.equal(model2.last_region_losses(), regions)
    for r, r2 in zip(eng.lap_resid, eng2.lap_resid, strict=True):
        assert torch.equal(r, r2)
    record_parity(case, "product defaults vs the checked run", 0.0, 0.0,
                  f"bit-identical scores, image gradient, seeds, slabs, residuals, {len(eng.sched.nodes) - skipped} activations; "
                  f"{skipped} pre-pool maps not stored, {eng2.sched._grad_slabs.shape[0]} gradient slabs")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_autograd_path_with_average_pooling(precision, monkeypatch):
    H, W = 40, 24
    taps = lw.LAYOUTS["default"]
    monkeypatch.setattr(core_model, "initialize_vgg",
                        lambda: core_model.build_vgg_features(_weights(synthetic.VGG19_CFG), synthetic.VGG19_CFG).eval())
    for k, v in CHECK_ENV.items():
        monkeypatch.setenv(k, v)
    model = core_model.StyleContentModel(list(taps[0]), list(taps[1]), precision=precision, pooling="avg").to(DEV)
    style, content, x0 = _images(H, W)
    model.set_targets(style.to(DEV), content.to(DEV))
    x = x0.to(DEV).requires_grad_(True)
    n = len(taps[0]) + len(taps[1])
    gout = [3e4 * (1.0 + 0.37 * i) for i in range(n)]
    style_l, content_l = model(x)
    sum(w * v for w, v in zip(gout, list(style_l) + list(content_l))).backward()
    torch.cuda.synchronize()
    eng = _engine(model)
    assert eng.pooling == "avg" and sum(nd.kind == "avgpool" for nd in eng.sched.nodes) == 4
    lw.check_step(eng, x0, style_w=1.0, content_w=1.0, x_grad=x.grad, gout=gout, record=record_parity,
                  case=f"autograd avg default {H}x{W} {precision}")
