"""Exact-operand parity of stv_tv and of the combine kernel's kind-2 rows on a real MI355X (the method of
tests/exact_head.py): images are integer-valued fp32 in [-8, 8] and the gradient coefficient is a power of two, so every
partial sum and every gradient element is exact in ANY summation order as long as the raw sum stays below 2^24 - which
each case asserts on the CPU.  Comparisons are torch.equal against the float64 value (tests/tv_ref.py), on outputs that
start from NaN.

The value pattern differs per channel and jumps by 12 or more between the last pixel of a row and the first of the next,
and by 11 or more between the last row of a plane and the first of the next: a difference taken across a row end or a channel plane
shows up as a wrong integer.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch

from style_transfer_visualizer_amd import _lib, ops
from tests import tv_ref
from tests.conftest import record_parity

from . import exact_head as eh

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = torch.float32
COEF = 0.25                       # a power of two: coef * (integer sum) is exact
LIMIT = float(2 ** 24)


def _second_trip_shape(ragged: bool) -> tuple[int, int, int]:
    """The smallest near-square C = 3 image whose work items (TV_VEC pixels of one row each) exceed one pass of the capped
    grid (TV_LOSS_PARTS workgroups x TV_THREADS items): the grid-stride loop runs twice.  One row less fits in one pass."""
    per_pass = _lib.TV_LOSS_PARTS * _lib.TV_THREADS
    w4 = math.isqrt(per_pass // 3) + 1
    H = per_pass // (3 * w4) + 1
    assert 3 * H * w4 > per_pass >= 3 * (H - 1) * w4
    return 3, H, _lib.TV_VEC * w4 - (3 if ragged else 0)


SHAPES = [(3, 1, 1), (3, 1, 7), (3, 5, 1), (1, 2, 2), (3, 4, 4), (3, 3, 5), (3, 17, 33), (3, 64, 48),
          _second_trip_shape(ragged=True), _second_trip_shape(ragged=False)]
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)      # noqa: E731


@functools.lru_cache(maxsize=None)
def case(shape: tuple[int, int, int]) -> dict:
    """Image, exact raw sum and exact neighbour sums of one shape; computed once, shared, never modified."""
    C, H, W = shape
    c = torch.arange(C).view(C, 1, 1)
    y = torch.arange(H).view(1, H, 1)
    x = torch.arange(W).view(1, 1, W)
    if C * H * W <= 3 * 64 * 48:      # a busy pattern, another one per channel
        v = (x * (3 + 2 * c) + y * (5 + c) + x * y * (c + 1) + 7 * c) % 17 - 8
    else:                             # large images: smooth blocks, so that the raw sum stays below 2^24
        v = (x // 16 + y // 16 + c) % 3 - 1
    v = v.clone()
    if H > 1:                         # first / last row of a plane, then (overriding them) first / last pixel of a row
        v[:, 0, :] = (-8 + c).expand(C, 1, W)[:, 0, :]
        v[:, -1, :] = (8 - c).expand(C, 1, W)[:, 0, :]
    if W > 1:
        v[:, :, 0] = (-8 + c).expand(C, H, 1)[:, :, 0]
        v[:, :, -1] = (8 - c).expand(C, H, 1)[:, :, 0]
    img = v.to(F32).contiguous()
    assert float(img.abs().max()) <= 8
    if W > 1 and H > 1:               # what a kernel that ignores row ends / plane ends would take a difference over
        assert float((img[:, 1:, 0] - img[:, :-1, -1]).abs().min()) >= 12
    if C > 1 and H > 1 and W > 2:
        assert float((img[1:, 0, 1:-1] - img[:-1, -1, 1:-1]).abs().min()) >= 11
    if C > 1 and H > 1 and W == 1:
        assert float((img[1:, 0] - img[:-1, -1]).abs().min()) >= 11
    raw = tv_ref.raw_sum(img)
    assert float(raw) < LIMIT and float(raw) == int(raw), f"raw sum {float(raw)} of {shape} is not exact in fp32"
    nsum = tv_ref.neighbour_sum(img)
    assert torch.equal(nsum, nsum.round()) and float(nsum.abs().max()) <= 64
    return {"x": img, "raw": raw, "nsum": nsum}


def nan(shape) -> torch.Tensor:
    return torch.full(shape, float("nan"), dtype=F32, device=DEV)


def same(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {tuple(got.shape)}/{got.dtype} for {tuple(want.shape)}/{want.dtype}"
    if torch.equal(got, want):
        return
    diff = ~(got == want)
    first = tuple(int(v) for v in diff.nonzero()[0])
    pytest.fail(f"{what}: {int(diff.sum())} of {got.numel()} elements differ; first at {first}: "
                f"got {float(got[first])!r}, expected {float(want[first])!r}")


def exact32(t64: torch.Tensor) -> torch.Tensor:
    assert torch.equal(t64.float().double(), t64), "expected value is not an fp32 number"
    return t64.float()


@pytest.fixture(scope="module", autouse=True)
def _parity_row():
    yield
    record_parity("exact total variation", "differing elements", 0.0, 0.0, f"{len(SHAPES)} shapes, compared bit for bit")


# ---- stv_tv --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_loss_partials(shape):
    """Every one of the partials is written (they start as NaN) and their float64 sum is the exact integer; a second
    launch leaves the same partials."""
    c = case(shape)
    x = c["x"].to(DEV)
    parts = nan((_lib.TV_LOSS_PARTS,))
    ops.tv(x, loss_part=parts)
    first = parts.clone()
    assert not bool(torch.isnan(first).any()), "a loss partial was not written"
    same(first.double().sum().reshape(1), c["raw"].reshape(1), f"tv {shape}: sum of the partials")
    if shape[1] * shape[2] == 1:
        same(first, torch.zeros_like(first), f"tv {shape}: no differences, every partial 0")
    parts.fill_(float("nan"))
    ops.tv(x, loss_part=parts)
    same(parts, first, f"tv {shape}: partials of a second launch")


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_gradient_write_and_accumulate(shape):
    c = case(shape)
    x = c["x"].to(DEV)
    want = exact32(COEF * c["nsum"])
    dx = nan(shape)
    ops.tv(x, dx=dx, coef=COEF)
    same(dx, want, f"tv {shape}: gradient, write mode")
    dx0 = eh.ints(shape, 4100 + shape[1] + shape[2], -8, 8)
    dx = dx0.to(DEV)
    ops.tv(x, dx=dx, coef=COEF, flags=_lib.ACCUM)
    same(dx, exact32(dx0.double() + COEF * c["nsum"]), f"tv {shape}: gradient, accumulate mode")


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_both_outputs_in_one_call_equal_the_two_calls(shape):
    c = case(shape)
    x = c["x"].to(DEV)
    parts, dx = nan((_lib.TV_LOSS_PARTS,)), nan(shape)
    ops.tv(x, loss_part=parts, dx=dx, coef=COEF)
    parts1, dx1 = nan((_lib.TV_LOSS_PARTS,)), nan(shape)
    ops.tv(x, loss_part=parts1)
    ops.tv(x, dx=dx1, coef=COEF)
    same(parts, parts1, f"tv {shape}: partials of the combined call")
    same(dx, dx1, f"tv {shape}: gradient of the combined call")
    same(dx, exact32(COEF * c["nsum"]), f"tv {shape}: gradient of the combined call, against float64")


@pytest.mark.parametrize("shape", [(3, 3, 5), (3, 4, 4), (3, 17, 33), (3, 64, 48), _second_trip_shape(True), _second_trip_shape(False)],
                         ids=_ids)
def test_accumulate_is_write_then_an_fp32_add(shape):
    """Real-valued image, gradient and coefficient: accumulate(dx0) == dx0 + write(), bit for bit - the product is
    rounded before the add (no FMA contraction), which is what lets the step's gradient be checked against
    grad_0 + stv_tv(write)."""
    g = torch.Generator().manual_seed(77 + shape[2])
    x = torch.randn(shape, generator=g).to(DEV)
    dx0 = torch.randn(shape, generator=g).to(DEV)
    coef = 0.37 / 3.0
    written = nan(shape)
    ops.tv(x, dx=written, coef=coef)
    assert not bool(torch.isnan(written).any())
    acc = dx0.clone()
    ops.tv(x, dx=acc, coef=coef, flags=_lib.ACCUM)
    same(acc, dx0 + written, f"tv {shape}: accumulate against write + add")
    parts, parts2 = nan((_lib.TV_LOSS_PARTS,)), nan((_lib.TV_LOSS_PARTS,))
    ops.tv(x, loss_part=parts)
    ops.tv(x, loss_part=parts2)
    same(parts, parts2, f"tv {shape}: partials of two launches on real values")


def test_rows_that_do_not_start_on_a_vector():
    """W % 4 == 0 but the base address is 4 bytes past a 16-byte boundary: the scalar path, same exact results."""
    shape = (3, 4, 8)
    c = case(shape)
    n = c["x"].numel()
    x = torch.zeros(n + 1, dtype=F32, device=DEV)[1:].view(shape)
    x.copy_(c["x"])
    assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    dx = nan((n + 1,))[1:].view(shape)
    parts = nan((_lib.TV_LOSS_PARTS,))
    ops.tv(x, loss_part=parts, dx=dx, coef=COEF)
    same(parts.double().sum().reshape(1), c["raw"].reshape(1), "tv unaligned: sum of the partials")
    same(dx, exact32(COEF * c["nsum"]), "tv unaligned: gradient")


def test_bad_arguments_are_refused():
    """STV_ERR_ARG from the entry point, RuntimeError from the binding; nothing is launched."""
    x = case((3, 4, 4))["x"].to(DEV)
    dx, parts = nan((3, 4, 4)), nan((_lib.TV_LOSS_PARTS,))
    with pytest.raises(RuntimeError, match="STV_ERR_ARG"):
        ops.tv(None, loss_part=parts, shape=(3, 4, 4))
    with pytest.raises(RuntimeError, match="STV_ERR_ARG"):
        ops.tv(x)                                                   # both outputs null
    for bad in ((0, 4, 4), (3, 0, 4), (3, 4, -1), (2, 16384, 16384)):      # the last: 2 * 2^28 * 4 bytes = 2 GiB
        with pytest.raises(RuntimeError, match="STV_ERR_ARG"):
            ops.tv(x, loss_part=parts, dx=dx, coef=COEF, shape=bad)
    with pytest.raises(RuntimeError, match="STV_ERR_ARG"):
        ops.tv(x, dx=x, coef=COEF)                                  # x == dx
    with pytest.raises(RuntimeError, match="STV_ERR_ARG"):
        ops.tv(x, dx=dx, coef=COEF, flags=_lib.MASK)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx).all()) and bool(torch.isnan(parts).all())


# ---- score combine with kind-2 rows ----------------------------------------------------------------------------------------------

COUNTS = {"last": ([32, 128, 512, 256, 256], [0, 0, 0, 1, 2]),
          "middle": ([32, 128, 256, 512, 256], [0, 0, 2, 0, 1]),
          "two": ([32, 256, 128, 256, 256, 512], [0, 2, 0, 1, 2, 0])}


@pytest.mark.parametrize("name", list(COUNTS))
def test_combine_with_extra_rows(name):
    """A kind-2 row joins neither score; the total is the fp32 total of the table without it, plus the terms in index
    order, one fp32 add each; the log ring's third row holds that total."""
    counts, kinds = COUNTS[name]
    table = eh._layout(counts, kinds)
    n = len(counts)
    parts = eh.ints((sum(counts),), 2600 + n, 0, 7)
    scale = [float(2.0 ** int(v)) for v in eh.ints((n,), 2610 + n, -2, 1)]
    style_w, content_w = 4.0, 0.5
    keep = [k for k in range(n) if kinds[k] != 2]
    base = eh.combine_expected(parts, [table[k] for k in keep], [scale[k] for k in keep], style_w, content_w)
    terms = [float(parts[table[k][0]:table[k][0] + table[k][1]].double().sum()) * scale[k] for k in range(n) if kinds[k] == 2]
    assert terms and all(t > 0 and float(np.float32(t)) == t for t in terms)
    total = np.float32(base["scores"][2])
    for t in terms:
        total = np.float32(total + np.float32(t))

    def run(rows, scales, log=None):
        losses, scores = nan((len(rows),)), nan((4,))
        args = (parts.to(DEV), torch.tensor(rows, dtype=torch.int32, device=DEV), torch.tensor(scales, dtype=F32, device=DEV),
                style_w, content_w, losses, scores)
        ops.loss_combine(*args) if log is None else ops.loss_combine_log(*args, *log)
        return losses.cpu(), scores.cpu()
    losses0, scores0 = run([table[k] for k in keep], [scale[k] for k in keep])
    same(scores0, torch.tensor(base["scores"], dtype=F32), f"combine {name}: the table without the extra rows")
    ring, count = nan((3, 4)), torch.zeros(1, dtype=torch.int32, device=DEV)
    losses, scores = run(table, scale, (ring, count))
    same(scores[:2], scores0[:2], f"combine {name}: style and content scores")
    same(losses[keep], losses0, f"combine {name}: the other terms")
    same(losses[[k for k in range(n) if kinds[k] == 2]], torch.tensor(terms, dtype=F32), f"combine {name}: the extra terms")
    same(scores[2:], torch.tensor([float(total), 1.0], dtype=F32), f"combine {name}: total and finite flag")
    assert float(scores[2]) != float(scores0[2])
    same(ring.cpu()[:, 0], scores[:3], f"combine {name}: ring record")
    assert int(count.cpu()) == 1
