"""Exact-operand parity of stv_lap and of the combine kernel's Laplacian rows on a real MI355X (the method of
tests/test_gpu_tv_exact.py): images are integer-valued fp32, built cell by cell as an integer cell mean plus a zero-sum,
non-constant pattern that differs per cell and per channel (one pixel of the cell +k, another -k), and the gradient coefficient
is a power of two.  Every cell mean is then the integer it was built from - a cell boundary off by one pixel or a wrong divisor
gives another number -, and every residual, partial sum and gradient element is exact in ANY summation order as long as the raw
sum stays below 2^24, which each case asserts on the CPU together with the integrality of every intermediate.  Comparisons are
torch.equal against the NumPy twin (tests/lap_ref.py; on these operands its fp32 and float64 forms agree, asserted too), on
outputs that start from NaN.

The cell means jump between the last cell of a row and the first of the next and between the last row of a plane and the first of
the next (borders of -A and A - c), so a stencil that crosses a row end or a plane end shows up as a wrong integer; the pixels
outside the covered Hp*p x Wp*p area hold 100, so a cell that reaches into them does too.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from style_transfer_visualizer_amd import _lib, ops
from tests import lap_ref
from tests.conftest import record_parity

from . import exact_head as eh

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = torch.float32
COEF = 0.25                       # a power of two: coef * (integer) is exact
LIMIT = float(2 ** 24)
TH, TW, PARTS = _lib.LAP_TILE_H, _lib.LAP_TILE_W, _lib.LAP_LOSS_PARTS


def _second_trip_loss() -> tuple[int, int, int, int]:
    """The smallest C = 3 shape whose tiles exceed one pass of the capped grid (LAP_LOSS_PARTS workgroups, one tile each):
    pool 1, one tile wide, one more row of tiles per plane than fits."""
    rows = PARTS // 3 + 1
    assert 3 * rows > PARTS >= 3 * (rows - 1)
    return 3, TH * rows, TW, 1


def _second_trip_grad() -> tuple[int, int, int, int]:
    """The GRAD mode's work items (LAP_VEC pixels of a row each) exceed one pass of its capped grid; pool 2 and an odd height:
    the last image row is a remainder row."""
    per_pass = _lib.LAP_GRAD_MAX_BLOCKS * _lib.LAP_THREADS
    W = 256
    H = per_pass // (3 * (W // _lib.LAP_VEC)) + 1
    H += 1 - H % 2
    assert 3 * H * (W // _lib.LAP_VEC) > per_pass
    return 3, H, W, 2


SHAPES = [(3, 1, 1, 1), (3, 2, 2, 2), (1, 4, 4, 2), (3, 5, 7, 2), (3, 9, 13, 4), (3, 17, 33, 1), (3, 32, 32, 32),
          *[(3, 64, 48, p) for p in (1, 2, 4, 8, 16)],
          # more than one tile along both axes and a ragged last tile: once on the scalar path with remainder pixels, once on vectors
          (3, (2 * TH + 3) * 2 + 1, (2 * TW + 5) * 2 + 1, 2), (3, (2 * TH + 3) * 4, (2 * TW + 5) * 4, 4),
          _second_trip_loss(), _second_trip_grad()]
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)      # noqa: E731


def _means(C: int, Hp: int, Wp: int, busy: bool) -> tuple[np.ndarray, np.ndarray]:
    """Integer cell means of the image and of the content image, [C, Hp, Wp]."""
    c = np.arange(C).reshape(C, 1, 1)
    i = np.arange(Hp).reshape(1, Hp, 1)
    j = np.arange(Wp).reshape(1, 1, Wp)
    if busy:
        mx = (j * (3 + 2 * c) + i * (5 + c) + i * j * (c + 1) + 7 * c) % 17 - 8
        mc = (j * (2 + c) + 3 * i + c) % 5 - 2
        amp = 8
    else:                             # large grids: smooth blocks, so that the raw sum stays below 2^24
        mx = (j // 16 + i // 16 + c) % 3 - 1
        mc = (i // 8 + 2 * (j // 8) + c) % 3 - 1
        amp = 3
    mx = np.broadcast_to(mx, (C, Hp, Wp)).copy()
    mc = np.broadcast_to(mc, (C, Hp, Wp)).copy()
    if Hp > 1:                        # first / last row of a plane, then (overriding them) first / last cell of a row
        mx[:, 0, :] = -amp
        mx[:, -1, :] = amp - c[:, 0]
    if Wp > 1:
        mx[:, :, 0] = -amp
        mx[:, :, -1] = amp - c[:, 0]
    return mx, mc


def _image(means: np.ndarray, H: int, W: int, p: int, salt: int) -> torch.Tensor:
    """The image whose cell (i, j) of plane c is its mean plus the zero-sum pattern: +k at one pixel, -k at another."""
    C, Hp, Wp = means.shape
    cells = np.repeat(means.reshape(C, Hp, Wp, 1), p * p, axis=3).astype(np.int64)
    if p > 1:
        c = np.arange(C).reshape(C, 1, 1, 1)
        i = np.arange(Hp).reshape(1, Hp, 1, 1)
        j = np.arange(Wp).reshape(1, 1, Wp, 1)
        k = 1 + (c + i + 2 * j + salt) % 3
        a = (3 * i + 5 * j + c + salt) % (p * p)
        b = (a + 1 + (i + j + c) % (p * p - 1)) % (p * p)
        assert (a != b).all()
        zero = np.zeros_like(cells)
        np.put_along_axis(zero, np.broadcast_to(a, k.shape).copy(), k, axis=3)
        np.put_along_axis(zero, np.broadcast_to(b, k.shape).copy(), -k, axis=3)
        assert (zero.sum(axis=3) == 0).all() and (zero != 0).any(axis=3).all()
        cells = cells + zero
    img = np.full((C, H, W), 100, dtype=np.int64)
    img[:, :Hp * p, :Wp * p] = cells.reshape(C, Hp, Wp, p, p).transpose(0, 1, 3, 2, 4).reshape(C, Hp * p, Wp * p)
    return torch.from_numpy(img.astype(np.float32)).contiguous()


@functools.lru_cache(maxsize=None)
def case(shape: tuple[int, int, int, int]) -> dict:
    """Images and every exact expected value of one (C, H, W, p); computed once, shared, never modified."""
    C, H, W, p = shape
    Hp, Wp = H // p, W // p
    for busy in (True, False):
        mx, mc = _means(C, Hp, Wp, busy)
        x, content = _image(mx, H, W, p, 0), _image(mc, H, W, p, 1)
        target = lap_ref.pool(content, p)
        r = lap_ref.resid(x, target, p)
        if lap_ref.raw_sum(r) < LIMIT:
            break
    assert float(x[:, :Hp * p, :Wp * p].abs().max()) <= 11
    # every intermediate is an integer, the same in fp32 and in float64: the cell means are the integers they were built from
    assert np.array_equal(target, mc) and np.array_equal(lap_ref.pool(x, p), mx)
    t64, r64 = lap_ref.pool(content, p, np.float64), lap_ref.resid(x, mc.astype(np.float64), p, np.float64)
    assert np.array_equal(t64, mc) and np.array_equal(r, r64) and np.array_equal(r, np.round(r))
    raw = lap_ref.raw_sum(r)
    assert raw < LIMIT and raw == int(raw) == float((r64 * r64).sum()), f"raw sum {raw} of {shape} is not exact in fp32"
    g = lap_ref.stencil(r)
    assert np.array_equal(g, lap_ref.stencil(r64)) and np.array_equal(g, np.round(g)) and float(np.abs(g).max()) < 2 ** 20
    if Hp > 1 and Wp > 1:             # what a stencil that ignores row ends / plane ends would take a difference over
        e = mx - mc
        assert np.abs(e[:, 1:, 0] - e[:, :-1, -1]).min() >= 2
        if C > 1 and Wp > 2:
            assert np.abs(e[1:, 0, 1:-1] - e[:-1, -1, 1:-1]).min() >= 2
    dx0 = eh.ints((C, H, W), 5100 + H + W + p, -8, 8)
    written = lap_ref.grad_accum(r, torch.zeros(C, H, W), p, COEF, accum=False)
    accumulated = lap_ref.grad_accum(r, dx0, p, COEF)
    assert np.array_equal(accumulated, lap_ref.grad_accum(r64, dx0, p, COEF, dtype=np.float64))
    assert np.array_equal(accumulated[:, :Hp * p, :Wp * p], dx0.numpy()[:, :Hp * p, :Wp * p] + written[:, :Hp * p, :Wp * p])
    return {"x": x, "content": content, "target": torch.from_numpy(target), "r": torch.from_numpy(r), "raw": raw, "dx0": dx0,
            "written": torch.from_numpy(written), "accumulated": torch.from_numpy(accumulated), "cells": (C, Hp, Wp)}


def nan(shape) -> torch.Tensor:
    return torch.full(tuple(shape), float("nan"), dtype=F32, device=DEV)


def same(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {tuple(got.shape)}/{got.dtype} for {tuple(want.shape)}/{want.dtype}"
    if torch.equal(got, want):
        return
    diff = ~(got == want)
    first = tuple(int(v) for v in diff.nonzero()[0])
    pytest.fail(f"{what}: {int(diff.sum())} of {got.numel()} elements differ; first at {first}: "
                f"got {float(got[first])!r}, expected {float(want[first])!r}")


@pytest.fixture(scope="module", autouse=True)
def _parity_row():
    yield
    record_parity("exact Laplacian loss", "differing elements", 0.0, 0.0, f"{len(SHAPES)} shapes, compared bit for bit")


# ---- stv_lap -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_pooled_target(shape):
    c = case(shape)
    out = nan(c["cells"])
    ops.lap_pool(c["content"].to(DEV), out, shape[3])
    same(out, c["target"], f"lap {shape}: pooled target")


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_residual_and_loss_partials(shape):
    """Every one of the partials is written (they start as NaN), their float64 sum is the exact integer, the residual is the
    twin's; a second launch leaves the same bits."""
    c = case(shape)
    x, target = c["x"].to(DEV), c["target"].to(DEV)
    resid, parts = nan(c["cells"]), nan((PARTS,))
    ops.lap_loss(x, target, resid, parts, shape[3])
    first, first_r = parts.clone(), resid.clone()
    assert not bool(torch.isnan(first).any()), "a loss partial was not written"
    same(first_r, c["r"], f"lap {shape}: residual")
    same(first.double().sum().reshape(1), torch.tensor([c["raw"]], dtype=torch.float64), f"lap {shape}: sum of the partials")
    if c["cells"][1] * c["cells"][2] == 1:
        same(first, torch.zeros_like(first), f"lap {shape}: a single cell has no neighbour, every partial 0")
    tiles = c["cells"][0] * -(-c["cells"][1] // TH) * -(-c["cells"][2] // TW)
    if tiles < PARTS:
        same(first[tiles:], torch.zeros(PARTS - tiles), f"lap {shape}: workgroups without a tile write 0")
    resid.fill_(float("nan"))
    parts.fill_(float("nan"))
    ops.lap_loss(x, target, resid, parts, shape[3])
    same(parts, first, f"lap {shape}: partials of a second launch")
    same(resid, first_r, f"lap {shape}: residual of a second launch")


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_gradient_write_and_accumulate(shape):
    """Write mode: the covered pixels hold coef * (L r) of their cell, the remainder pixels +0.  Accumulate mode: the covered
    pixels gain it, the remainder pixels are untouched."""
    c = case(shape)
    p = shape[3]
    r = c["r"].to(DEV)
    dx = nan(shape[:3])
    ops.lap_grad(r, dx, p, coef=COEF)
    same(dx, c["written"], f"lap {shape}: gradient, write mode")
    Hc, Wc = c["cells"][1] * p, c["cells"][2] * p
    rest = torch.ones(shape[:3], dtype=torch.bool)
    rest[:, :Hc, :Wc] = False
    assert not bool(torch.signbit(dx.cpu()[rest]).any()), "remainder pixels are written +0"
    dx = c["dx0"].to(DEV)
    ops.lap_grad(r, dx, p, coef=COEF, flags=_lib.ACCUM)
    same(dx, c["accumulated"], f"lap {shape}: gradient, accumulate mode")
    same(dx.cpu()[rest], c["dx0"][rest], f"lap {shape}: remainder pixels, accumulate mode")
    if bool(rest.any()):              # a NaN in a remainder pixel stays there and reaches no covered pixel
        dx = c["dx0"].clone()
        dx[rest] = float("nan")
        dx = dx.to(DEV)
        ops.lap_grad(r, dx, p, coef=COEF, flags=_lib.ACCUM)
        assert bool(torch.isnan(dx.cpu()[rest]).all()) and not bool(torch.isnan(dx.cpu()[~rest]).any())


REAL = [(3, 5, 7, 2), (3, 9, 13, 4), (3, 17, 33, 1), (3, 64, 48, 2), (3, 64, 48, 4), (3, 64, 48, 8), (3, 64, 48, 16), (3, 64, 64, 32),
        (3, (2 * TH + 3) * 4, (2 * TW + 5) * 4, 4), _second_trip_loss()]


@pytest.mark.parametrize("shape", REAL, ids=_ids)
def test_real_values_follow_the_stated_order_of_operations(shape):
    """Random normal images: target, residual and gradient equal the fp32 twin bit for bit (the summation order inside a cell,
    the stencil's order, the rounded product); accumulate(dx0) == dx0 + write(); two launches give the same partials, whose
    float64 sum is within the chain bound of the twin's."""
    C, H, W, p = shape
    g = torch.Generator().manual_seed(91 + H + p)
    x, content, dx0 = (torch.randn(C, H, W, generator=g) for _ in range(3))
    coef = 0.37 / 3.0
    cells = (C, H // p, W // p)
    target, resid, parts, parts2 = nan(cells), nan(cells), nan((PARTS,)), nan((PARTS,))
    ops.lap_pool(content.to(DEV), target, p)
    t_ref = lap_ref.pool(content, p)
    same(target, torch.from_numpy(t_ref), f"lap {shape}: target on real values")
    ops.lap_loss(x.to(DEV), target, resid, parts, p)
    r_ref = lap_ref.resid(x, t_ref, p)
    same(resid, torch.from_numpy(r_ref), f"lap {shape}: residual on real values")
    ops.lap_loss(x.to(DEV), target, resid, parts2, p)
    same(parts, parts2, f"lap {shape}: partials of two launches on real values")
    want = lap_ref.raw_sum(r_ref)
    depth = lap_ref.partial_sum_depth(*cells, TH, TW, PARTS)
    assert abs(float(parts.double().sum()) - want) <= lap_ref.gamma(depth) * want + 1e-12 * want
    written = nan((C, H, W))
    ops.lap_grad(resid, written, p, coef=coef)
    same(written, torch.from_numpy(lap_ref.grad_accum(r_ref, dx0, p, coef, accum=False)), f"lap {shape}: gradient on real values")
    acc = dx0.to(DEV)
    ops.lap_grad(resid, acc, p, coef=coef, flags=_lib.ACCUM)
    same(acc, torch.from_numpy(lap_ref.grad_accum(r_ref, dx0, p, coef)), f"lap {shape}: accumulated gradient on real values")
    same(acc, dx0.to(DEV) + written, f"lap {shape}: accumulate against write + add")


@pytest.mark.parametrize("p", [1, 2, 4])
def test_rows_that_do_not_start_on_a_vector(p):
    """W % 4 == 0 but the base addresses are 4 bytes past a 16-byte boundary: the scalar paths, same exact results."""
    shape = (3, 64, 48, p)
    c = case(shape)
    n = c["x"].numel()

    def shifted(src: torch.Tensor | None) -> torch.Tensor:
        t = nan((n + 1,))[1:].view(shape[:3])
        if src is not None:
            t.copy_(src)
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        return t
    target, resid, parts = nan(c["cells"]), nan(c["cells"]), nan((PARTS,))
    ops.lap_pool(shifted(c["content"]), target, p)
    same(target, c["target"], "lap unaligned: pooled target")
    ops.lap_loss(shifted(c["x"]), target, resid, parts, p)
    same(resid, c["r"], "lap unaligned: residual")
    same(parts.double().sum().reshape(1), torch.tensor([c["raw"]], dtype=torch.float64), "lap unaligned: sum of the partials")
    dx = shifted(None)
    ops.lap_grad(resid, dx, p, coef=COEF)
    same(dx, c["written"], "lap unaligned: gradient, write mode")
    dx = shifted(c["dx0"])
    ops.lap_grad(resid, dx, p, coef=COEF, flags=_lib.ACCUM)
    same(dx, c["accumulated"], "lap unaligned: gradient, accumulate mode")


def test_bad_arguments_are_refused():
    """STV_ERR_ARG from the entry point, RuntimeError from the binding; nothing is launched."""
    shape = (3, 9, 13, 4)
    c = case(shape)
    x, target = c["x"].to(DEV), c["target"].to(DEV)
    resid, parts, dx = nan(c["cells"]), nan((PARTS,)), nan(shape[:3])
    refused = pytest.raises(RuntimeError, match="STV_ERR_ARG")
    with refused:
        ops.lap_pool(None, resid, 4, shape=shape[:3])
    with refused:
        ops.lap_loss(x, None, resid, parts, 4)
    with refused:
        ops.lap_loss(x, target, resid, None, 4)
    with refused:
        ops.lap_grad(None, dx, 4, coef=COEF)
    with refused:
        ops.lap_grad(resid, None, 4, coef=COEF, shape=shape[:3])
    for bad in ((0, 9, 13), (3, 0, 13), (3, 9, -1), (2, 16384, 16384), (3, 3, 13), (3, 9, 3)):       # the last two: no cell
        with refused:
            ops.lap_loss(x, target, resid, parts, 4, shape=bad)
    for pool in (0, 3, 6, 64):
        with refused:
            ops.lap_loss(x, target, resid, parts, pool)
    with refused:
        ops.lap_grad(resid, dx, 4, coef=COEF, flags=_lib.MASK)
    with refused:
        ops.lap_loss(x, target, resid, parts, 4, flags=_lib.ACCUM)
    with refused:
        ops.lap_grad(dx, dx, 4, coef=COEF)                           # dx shares bytes with the residual
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx).all()) and bool(torch.isnan(parts).all()) and bool(torch.isnan(resid).all())


# ---- score combine with TV's row and two Laplacian rows ----------------------------------------------------------------------

def test_combine_with_the_tv_row_and_two_laplacian_rows():
    """Kind-2 rows join neither score; the total is the fp32 total of the table without them, plus TV's term, then the two
    Laplacian terms, in index order, one fp32 add each."""
    counts = [32, 128, 512, 256, 256, _lib.TV_LOSS_PARTS, PARTS, PARTS]
    kinds = [0, 0, 0, 0, 1, 2, 2, 2]
    table = eh._layout(counts, kinds)
    n = len(counts)
    parts = eh.ints((sum(counts),), 2700 + n, 0, 7)
    scale = [float(2.0 ** int(v)) for v in eh.ints((n,), 2710 + n, -2, 1)]
    style_w, content_w = 4.0, 0.5
    keep = [k for k in range(n) if kinds[k] != 2]
    base = eh.combine_expected(parts, [table[k] for k in keep], [scale[k] for k in keep], style_w, content_w)
    terms = [float(parts[table[k][0]:table[k][0] + table[k][1]].double().sum()) * scale[k] for k in range(n) if kinds[k] == 2]
    assert len(terms) == 3 and all(t > 0 and float(np.float32(t)) == t for t in terms)
    total = np.float32(base["scores"][2])
    for t in terms:
        total = np.float32(total + np.float32(t))
    losses, scores = nan((n,)), nan((4,))
    ops.loss_combine(parts.to(DEV), torch.tensor(table, dtype=torch.int32, device=DEV), torch.tensor(scale, dtype=F32, device=DEV),
                     style_w, content_w, losses, scores)
    same(scores[:2], torch.tensor(base["scores"][:2], dtype=F32), "combine: style and content scores")
    same(losses[[k for k in range(n) if kinds[k] == 2]], torch.tensor(terms, dtype=F32), "combine: the three extra terms")
    same(scores[2:], torch.tensor([float(total), 1.0], dtype=F32), "combine: total and finite flag")
    assert float(total) != float(base["scores"][2])
