"""Host-side logic of the row-strip exchange that cannot run on the one-GPU box: the RCCL branch of
HaloShard._p2p (batch_isend_irecv over uint8 views) with the collective replaced by a loop-back fake; and the parts that
need no GPU at all: ``strip_rows`` over every (H, world), and the content-gradient coefficients and combine rows of the
strip loss head, read from the op lists a strip schedule builds in device form on host tensors."""
from __future__ import annotations

import ctypes
import types

import pytest
import torch
import torch.distributed as dist

from style_transfer_visualizer_amd import _lib, core_model, ops, plan, spatial
from tests import spatial_cases


def test_p2p_rccl_branch_stages_non_contiguous_rows(monkeypatch):
    sent = {}

    class FakeOp:
        def __init__(self, fn, tensor, peer, group):
            self.fn, self.tensor, self.peer = fn, tensor, peer

    class Done:
        def wait(self):
            return None

    def fake_batch(ops):
        # loop-back world: what goes to peer p is what comes back from peer p
        for op in ops:
            assert op.tensor.is_contiguous() and op.tensor.dtype == torch.uint8      # what send/recv accept
            if op.fn is dist.isend:
                sent[op.peer] = op.tensor.clone()
        for op in ops:
            if op.fn is dist.irecv:
                op.tensor.copy_(sent[op.peer])
        return [Done() for _ in ops]
    monkeypatch.setattr(dist, "P2POp", FakeOp)
    monkeypatch.setattr(dist, "batch_isend_irecv", fake_batch)
    def make(rank, group=None):
        ns = types.SimpleNamespace(rank=rank, world=3, group=group, _host_p2p=False)
        ns._peer = types.MethodType(spatial.HaloShard._peer, ns)
        return ns
    shard = make(1)       # a middle rank: two neighbours
    # NCHW image rows (non-contiguous [1, 3, W] slices) and NHWC activation rows (contiguous [W, C], bf16)
    x = torch.arange(1 * 3 * 6 * 5, dtype=torch.float32).reshape(1, 3, 6, 5)
    want_top, want_bot = x[:, :, 1].clone(), x[:, :, 4].clone()
    spatial.HaloShard._p2p(shard, x[:, :, 1], x[:, :, 4], x[:, :, 0], x[:, :, 5])
    assert torch.equal(x[:, :, 0], want_top) and torch.equal(x[:, :, 5], want_bot)
    a = torch.arange(6 * 5 * 8, dtype=torch.float32).reshape(6, 5, 8).bfloat16()
    want_top, want_bot = a[1].clone(), a[4].clone()
    spatial.HaloShard._p2p(shard, a[1], a[4], a[0], a[5])
    assert torch.equal(a[0], want_top) and torch.equal(a[5], want_bot)
    # an edge rank only talks to its one neighbour
    edge = make(0)
    sent.clear()
    top_before = a[0].clone()
    spatial.HaloShard._p2p(edge, a[1], a[4], a[0], a[5])
    assert set(sent) == {1} and torch.equal(a[0], top_before)
    # inside a sub-group the peers are named by GLOBAL rank (group ranks 0, 1, 2 = world ranks 4, 5, 7)
    monkeypatch.setattr(dist, "get_global_rank", lambda group, r: group[r])
    sent.clear()
    sub = make(1, group=[4, 5, 7])
    spatial.HaloShard._p2p(sub, a[1], a[4], a[0], a[5])
    assert set(sent) == {4, 7}


# ------------------------------------------------------------------------------------------------ strip_rows
def _verdicts(H: int, world: int) -> list:
    out = []
    for r in range(world):
        try:
            out.append(spatial.strip_rows(H, r, world))
        except ValueError as exc:
            out.append(str(exc))
    return out


def test_strip_rows_one_verdict_for_all_ranks_and_a_tiling_of_the_image():
    """``strip_rows`` is pure in (H, rank, world): every rank must reach the SAME verdict (a rank that raises while its
    peers construct their shards leaves them waiting in their first exchange), and the strips it hands out tile the
    image.  Every (H, world) with 16 <= H <= 640 and 1 <= world <= 8."""
    raising = 0
    for world in range(1, 9):
        for H in range(16, 641):
            got = _verdicts(H, world)
            if any(isinstance(g, str) for g in got):
                assert all(isinstance(g, str) for g in got), f"H={H} world={world}: ranks disagree: {got}"
                assert len(set(got)) == 1 and "too small for" in got[0], f"H={H} world={world}: {got}"
                raising += 1
                continue
            edge = 0
            for c0, c1, e0, e1 in got:            # the core strips tile [0, H) in rank order
                assert c0 == edge and c1 > c0 and c0 % 16 == 0, f"H={H} world={world}: {got}"
                assert 0 <= e0 <= c0 and c1 <= e1 <= H and e0 % 16 == 0, f"H={H} world={world}: {got}"
                edge = c1
            assert edge == H, f"H={H} world={world}: {got}"
    assert raising > 0


def test_strip_rows_pinned_layouts():
    got = _verdicts(96, 4)                        # base height 32: three strips cover the image, rank 3 has none
    assert got == ["image of 96 rows is too small for 4 strips of at least 16 rows"] * 4
    assert [spatial.strip_rows(2160, r, 4)[:2] for r in range(4)] == [(0, 544), (544, 1088), (1088, 1632), (1632, 2160)]
    for case in spatial_cases.CASES:              # the layouts tests/test_gpu_spatial_cases.py runs
        rows = [spatial.strip_rows(case.H, r, case.world) for r in range(case.world)]
        assert tuple(r[:2] for r in rows) == case.strips
        if case.extended:
            assert tuple(r[2:] for r in rows) == case.extended


# ------------------------------------------------------------------------------------------------ own-share coefficients
class _Recorded:
    """Stands in for ``plan.Program``: keeps the op list it is given and runs nothing."""

    def __init__(self, op_list, extra=()):
        self.op_list = list(op_list)

    def run(self, use_graph=False):
        pass


def _mini_layers():
    return list(core_model.build_vgg_features(None, spatial_cases.MINI).eval().children())


def _strip_head(monkeypatch, content_at, layout, content_w):
    """The strip schedule and its loss head in device form on host tensors (never run).  ``layout``: ("halo", H, rows) -
    the HaloShard way, one halo row on either side, own = the interior; ("recompute", H, rank, world) - the
    SpatialShard way, no halo, own = the core rows of the extended strip."""
    monkeypatch.setattr(plan, "Program", _Recorded)
    W, dtype, cpu = 40, torch.float32, torch.device("cpu")
    if layout[0] == "halo":
        _, H, rows = layout
        s = plan.Schedule(_mini_layers(), spatial_cases.S_AT, list(content_at), rows, W, dtype, cpu, with_grad=True, halo=1,
                          assume_device=True)
        x_grad = torch.zeros(1, 3, rows + 2, W)

        def own(buf, k, t):
            return s.interior(t)
    else:
        _, H, rank, world = layout
        c0, c1, e0, e1 = spatial.strip_rows(H, rank, world)
        s = plan.Schedule(_mini_layers(), spatial_cases.S_AT, list(content_at), e1 - e0, W, dtype, cpu, with_grad=True,
                          fuse_first_gram=False, assume_device=True)
        x_grad = torch.zeros(1, 3, e1 - e0, W)

        def own(buf, k, t):       # (spatial.SpatialShard.__init__: core_rows)
            return t[(c0 - e0) // k:buf.H if c1 >= H else (c1 - e0) // k]
    for tap in s.content_taps:
        tap.target = torch.zeros_like(tap.buf.act)
    targets = [torch.zeros(t.buf.C, t.buf.C) for t in s.style_taps]
    head = spatial._StripLossHead(s, own, H, targets, 1e2, content_w)
    return s, head, s.backward_ops(x_grad, content_coef=head.content_coef, coef_dev=None), H


LAYOUTS = [("halo", 128, 64),                  # two 64-row strips of H = 128: a tap's share is (64 / k + 2) / (128 / k)
           ("recompute", 200, 1, 2),           # the second strip of H = 200: clipped halos, the strip IS the image
           ("recompute", 404, 0, 2)]           # rows [0, 368) of 404: floor(404 / 8) = 50 makes the shares .9109 and .92


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda v: "-".join(str(p) for p in v))
@pytest.mark.parametrize("content_at", spatial_cases.CONTENT_SETS, ids=str)
def test_every_content_tap_takes_its_own_share(monkeypatch, content_at, layout):
    """The content-gradient op of a strip divides by the element count of the strip's buffer, the loss by the whole
    image's: the coefficient of tap i is ``content_w * (elements of ITS buffer) / (elements of ITS whole-image map)``.
    The shares differ between resolutions (two halo rows weigh more on a small map; pooled heights are floored), so a
    share handed to another tap scales that tap's gradient wrongly while every loss value stays right."""
    content_w = 0.75
    s, head, bwd, H = _strip_head(monkeypatch, content_at, layout, content_w)
    layers = _mini_layers()
    assert [t.order for t in s.content_taps] == list(range(len(content_at)))
    grad_ops = [o for o in bwd if o.op == _lib.OP_CONTENT_GRAD]
    assert len(grad_ops) == len(content_at)
    n_global, coefs = [], []
    for tap, layer in zip(s.content_taps, sorted(content_at), strict=True):
        k = spatial_cases.pool_factor(layers, layer)
        assert tap.buf.W == 40 // k
        (op,) = [o for o in grad_ops if o.refs["p1"] is tap.target]
        assert op.refs["p0"] is tap.buf.act and op.n == tap.buf.act.numel()
        n_global.append((H // k) * tap.buf.W * tap.buf.C)
        want = content_w * tap.buf.act.numel() / n_global[-1]
        # (the op holds its coefficient as a C float)
        assert op.f0 == ctypes.c_float(want).value, f"layer {layer} (k = {k}): coefficient {op.f0}, own share {want}"
        coefs.append(op.f0)
    if layout == LAYOUTS[0]:      # the shares written out: (64 / k + 2) / (128 / k)
        assert coefs == [content_w * {3: 0.515625, 8: 0.53125, 21: 0.625, 26: 0.625}[layer] for layer in sorted(content_at)]
    # the combine: content terms behind the style terms, in tap order, each normalised by its whole-image element count
    (combine,) = [o for o in head.phase2 if o.op == _lib.OP_LOSS_COMBINE]
    n_s, n_c = len(s.style_taps), len(content_at)
    assert combine.cin == n_s + n_c and (combine.f0, combine.f1) == (1e2, content_w)
    assert combine.refs["p1"] is head.table and combine.refs["p2"] is head.scale
    slot = sum(ops.gram_loss_parts(t.buf.C) for t in s.style_taps)
    assert head.table[n_s:].tolist() == [[slot + i, 1, 1] for i in range(n_c)]
    assert head.scale[n_s:].tolist() == [ctypes.c_float(1.0 / n).value for n in n_global]
    # ... and phase one writes tap i's squared error to the slot the reduce moves to row i
    loss_ops = [o for o in head.phase1 if o.op == _lib.OP_CONTENT_LOSS]
    for i, (tap, op) in enumerate(zip(s.content_taps, loss_ops, strict=True)):
        assert op.q0 == head.parts_c[i * _lib.CONTENT_LOSS_PARTS:].data_ptr()
        assert op.refs["p0"].data_ptr() >= tap.buf.act.data_ptr() and op.n == op.refs["p0"].numel() == op.refs["p1"].numel()
