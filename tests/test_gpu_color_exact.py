"""Exact parity of the three colour kernels (stv_color_stats, stv_color_affine, stv_luma_transfer) on a real MI355X.

Statistics: images are integer-valued fp32 in [-8, 8], so every moment is an integer that float64 holds exactly in ANY
summation order; the float64 sum over the rows of ``parts`` must equal the int64 moment.  The pattern differs per channel
so that the three cross moments and the three squares are six different integers - asserted on the CPU: a swapped channel
pair shows as a wrong integer.  One random-normal image checks real values against float64 NumPy within
``1e-12 * sum|terms|`` (double sums over chains of a few dozen terms are three orders of magnitude inside that).

Affine and luma: ``torch.equal`` against the fp32 NumPy twins of tests/color_ref.py, on outputs that start from NaN, out of
place and in place.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch

from style_transfer_visualizer_amd import _lib, ops
from tests import color_ref as cr
from tests.conftest import record_parity

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = torch.float32
MEAN, STD = cr.IMAGENET_MEAN, cr.IMAGENET_STD


def _second_trip_shape(blocks: int, *, ragged: bool) -> tuple[int, int]:
    """The smallest near-square image whose work items (COLOR_VEC pixels of one row each) exceed one pass of a grid capped at
    ``blocks`` workgroups of COLOR_THREADS items: the grid-stride loop runs twice.  One row less fits in one pass."""
    per_pass = blocks * _lib.COLOR_THREADS
    w4 = math.isqrt(per_pass) + 1
    H = per_pass // w4 + 1
    assert H * w4 > per_pass >= (H - 1) * w4
    return H, _lib.COLOR_VEC * w4 - (3 if ragged else 0)


SMALL = [(1, 1), (1, 7), (5, 1), (2, 2), (4, 4), (3, 5), (17, 33), (64, 48)]
STATS_SHAPES = SMALL + [_second_trip_shape(_lib.COLOR_STATS_PARTS, ragged=True), _second_trip_shape(_lib.COLOR_STATS_PARTS, ragged=False)]
MAP_SHAPES = SMALL + [_second_trip_shape(_lib.COLOR_MAX_BLOCKS, ragged=True), _second_trip_shape(_lib.COLOR_MAX_BLOCKS, ragged=False)]
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)      # noqa: E731
M12 = [1.25, -0.375, 0.0, 0.0, 0.8125, -1.5, -0.3, 0.0, 2.7, 0.1, -0.25, 0.0]   # positive, negative and zero entries


def nan(shape) -> torch.Tensor:
    return torch.full(tuple(shape), float("nan"), dtype=F32, device=DEV)


def offset_by_one(t: torch.Tensor) -> torch.Tensor:
    """A device copy of ``t`` whose base address is 4 bytes past a 16-byte boundary: the scalar path."""
    buf = torch.zeros(t.numel() + 1, dtype=F32, device=DEV)[1:].view(t.shape)
    buf.copy_(t)
    assert buf.data_ptr() % 16 == 4 and buf.is_contiguous()
    return buf


def same(got: torch.Tensor, want, what: str) -> None:
    got = got.detach().cpu()
    want = torch.from_numpy(np.ascontiguousarray(want)) if isinstance(want, np.ndarray) else want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {tuple(got.shape)}/{got.dtype} for {tuple(want.shape)}/{want.dtype}"
    if torch.equal(got, want):
        return
    diff = ~(got == want)
    first = tuple(int(v) for v in diff.nonzero()[0])
    pytest.fail(f"{what}: {int(diff.sum())} of {got.numel()} elements differ; first at {first}: "
                f"got {float(got[first])!r}, expected {float(want[first])!r}")


@pytest.fixture(scope="module", autouse=True)
def _parity_rows():
    yield
    record_parity("exact colour statistics", "differing moments", 0.0, 0.0, f"{len(STATS_SHAPES) + 1} cases, float64 sum of the rows == int64")
    record_parity("exact colour affine map", "differing elements", 0.0, 0.0, f"{len(MAP_SHAPES) + 1} cases, compared bit for bit")
    record_parity("exact luma transfer", "differing elements", 0.0, 0.0, f"{2 * (len(MAP_SHAPES) + 1)} cases, compared bit for bit")


# ---- stv_color_stats -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def int_case(shape: tuple[int, int]) -> dict:
    """Integer image and its exact moments; computed once, shared, never modified."""
    img = cr.pattern(*shape)
    v = img.astype(np.int64)
    assert np.abs(v).max() <= 8 and np.array_equal(v.astype(np.float32), img)
    exact = np.array([v[c].sum() for c in range(3)] + [(v[i] * v[j]).sum() for i, j in cr.PAIRS], dtype=np.int64)
    # six different integers: no two products can be exchanged unnoticed (and, from 16 pixels up, no two sums)
    assert len(set(exact[3:].tolist())) == 6, f"{shape}: second moments {exact[3:].tolist()} are not pairwise different"
    if shape[0] * shape[1] >= 16:
        assert len(set(exact[:3].tolist())) == 3, f"{shape}: sums {exact[:3].tolist()} are not pairwise different"
    return {"x": torch.from_numpy(img), "exact": exact}


def nan_parts() -> torch.Tensor:
    return torch.full((_lib.COLOR_STATS_PARTS, 9), float("nan"), dtype=torch.float64, device=DEV)


def _check_stats(x: torch.Tensor, exact: np.ndarray, what: str) -> torch.Tensor:
    """``parts`` starts as NaN; afterwards every entry is finite, the float64 sum over the rows is the exact integer, and a
    second launch leaves the same bits."""
    parts = nan_parts()
    assert ops.color_stats(x, out=parts) is parts
    first = parts.clone()
    assert bool(torch.isfinite(first).all()), f"{what}: a partial was not written"
    total = first.cpu().numpy().sum(axis=0, dtype=np.float64)
    assert np.array_equal(total, exact.astype(np.float64)), f"{what}: {total.tolist()} for {exact.tolist()}"
    parts.fill_(float("nan"))
    ops.color_stats(x, out=parts)
    assert torch.equal(parts, first), f"{what}: a second launch left other partials"
    return first


@pytest.mark.parametrize("shape", STATS_SHAPES, ids=_ids)
def test_statistics_are_the_exact_integers(shape):
    c = int_case(shape)
    rows = _check_stats(c["x"].to(DEV), c["exact"], f"stats {shape}")
    if shape[0] * shape[1] == 1:
        assert bool((rows[1:] == 0).all()), "a workgroup without items writes zeros"
    fresh = ops.color_stats(c["x"].to(DEV).unsqueeze(0))                        # [1, 3, H, W], default output
    assert torch.equal(fresh, rows)


def test_statistics_from_a_base_that_is_not_on_a_vector():
    shape = _second_trip_shape(_lib.COLOR_STATS_PARTS, ragged=False)
    c = int_case(shape)
    rows = _check_stats(offset_by_one(c["x"]), c["exact"], f"stats {shape} unaligned")
    # the same partials, row by row, as the vector path leaves: same items in the same order
    assert torch.equal(rows, ops.color_stats(c["x"].to(DEV)))


def test_statistics_of_real_values_against_float64():
    H, W = 64, 48
    x = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(21))
    got = ops.color_stats(x.to(DEV)).cpu().numpy().sum(axis=0, dtype=np.float64)
    want, scale = cr.moments(x.numpy()), cr.abs_moments(x.numpy())
    worst = float((np.abs(got - want) / scale).max())
    print(f"stv_color_stats {H}x{W} randn: worst |error| / sum|terms| = {worst:.3e}")
    record_parity(f"stv_color_stats {H}x{W} randn", "worst |error| / sum|terms|", worst, 1e-12, "float64 NumPy")
    assert bool((np.abs(got - want) <= 1e-12 * scale).all())


# ---- stv_color_affine ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def real_case(shape: tuple[int, int]) -> dict:
    H, W = shape
    g = torch.Generator().manual_seed(300 + H + W)
    x = torch.randn(1, 3, H, W, generator=g)
    return {"x": x, "affine": cr.affine(x.numpy(), M12)}


def _check_affine(x_dev: torch.Tensor, want: np.ndarray, what: str, make_out) -> None:
    out = make_out()
    got = ops.color_affine(x_dev, M12, out=out)
    assert got is out
    same(out, want, f"{what}: out of place")
    same(x_dev, real_case(tuple(want.shape[-2:]))["x"], f"{what}: the input of an out-of-place call")
    got = ops.color_affine(x_dev, M12, out=x_dev)
    assert got is x_dev
    same(x_dev, want, f"{what}: in place")


@pytest.mark.parametrize("shape", MAP_SHAPES, ids=_ids)
def test_affine_equals_the_twin(shape):
    c = real_case(shape)
    assert set(np.sign(M12)) == {-1.0, 0.0, 1.0}
    _check_affine(c["x"].to(DEV), c["affine"], f"affine {shape}", lambda: nan(c["x"].shape))
    y = ops.color_affine(c["x"].to(DEV)[0], M12)                              # [3, H, W], default output
    assert tuple(y.shape) == (3, *shape)
    same(y, c["affine"][0], f"affine {shape}: rank 3")


def test_affine_from_a_base_that_is_not_on_a_vector():
    shape = _second_trip_shape(_lib.COLOR_MAX_BLOCKS, ragged=False)
    c = real_case(shape)
    _check_affine(offset_by_one(c["x"]), c["affine"], f"affine {shape} unaligned", lambda: offset_by_one(nan(c["x"].shape)))


def test_affine_refusals():
    x = real_case((4, 4))["x"].to(DEV)
    flat = torch.zeros(2 * x.numel(), dtype=F32, device=DEV)
    a, b = flat[: x.numel()].view(x.shape), flat[4: 4 + x.numel()].view(x.shape)
    with pytest.raises(RuntimeError, match="STV_ERR_ARG"):
        ops.color_affine(a, M12, out=b)                                       # partially overlapping ranges
    with pytest.raises(RuntimeError, match="12"):
        ops.color_affine(x, M12[:9])
    with pytest.raises(RuntimeError, match="expects an fp32 image"):
        ops.color_affine(torch.zeros(1, 4, 4, 4, device=DEV), M12)
    with pytest.raises(RuntimeError, match="out is"):
        ops.color_affine(x, M12, out=torch.zeros(1, 3, 4, 8, device=DEV))
    torch.cuda.synchronize()
    assert not bool(flat.any())


# ---- stv_luma_transfer ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def luma_case(shape: tuple[int, int], normalize: bool) -> dict:
    """``content`` like a loaded image, ``result`` far outside [0, 1] after de-normalisation, with NaN and both infinities."""
    H, W = shape
    g = torch.Generator().manual_seed(500 + H + W)
    content = torch.rand(1, 3, H, W, generator=g)
    result = content + 1.5 * torch.randn(1, 3, H, W, generator=g)
    if normalize:
        mean, std = torch.tensor(MEAN).view(1, 3, 1, 1), torch.tensor(STD).view(1, 3, 1, 1)
        content, result = (content - mean) / std, (result - mean) / std
    flat = result.view(-1)
    for k, v in enumerate((float("nan"), float("inf"), float("-inf"))):
        flat[(k * 5) % flat.numel()::max(11, flat.numel() // 7)] = v        # (1x1: the last assignment wins, -inf in channel 0)
    rgb = cr.rgb01(result.numpy(), normalize=normalize)
    if H * W >= 16:
        assert (rgb == 0).any() and (rgb == 1).any() and ((rgb > 0) & (rgb < 1)).any()
        assert np.isnan(result.numpy()).any() and np.isposinf(result.numpy()).any() and np.isneginf(result.numpy()).any()
    want = cr.luma(result.numpy(), content.numpy(), normalize=normalize)
    assert np.isfinite(want).all()
    return {"result": result, "content": content, "want": want}


def _check_luma(result: torch.Tensor, content: torch.Tensor, want: np.ndarray, normalize: bool, what: str, make_out) -> None:
    kw = {"mean": MEAN if normalize else None, "std": STD if normalize else None}
    content_before = content.clone()
    out = make_out()
    got = ops.luma_transfer(result, content, out=out, **kw)
    assert got is out
    same(out, want, f"{what}: out of place")
    got = ops.luma_transfer(result, content, out=result, **kw)
    assert got is result
    same(result, want, f"{what}: in place over the result")
    same(content, content_before, f"{what}: the content image")


@pytest.mark.parametrize("normalize", [True, False], ids=["normalised", "plain"])
@pytest.mark.parametrize("shape", MAP_SHAPES, ids=_ids)
def test_luma_equals_the_twin(shape, normalize):
    c = luma_case(shape, normalize)
    _check_luma(c["result"].to(DEV), c["content"].to(DEV), c["want"], normalize, f"luma {shape} normalize={normalize}",
                lambda: nan(c["result"].shape))
    fresh = ops.luma_transfer(c["result"].to(DEV)[0], c["content"].to(DEV)[0], mean=MEAN if normalize else None,
                              std=STD if normalize else None)                 # [3, H, W], default output
    same(fresh, c["want"][0], f"luma {shape}: rank 3")


@pytest.mark.parametrize("normalize", [True, False], ids=["normalised", "plain"])
def test_luma_from_bases_that_are_not_on_a_vector(normalize):
    shape = _second_trip_shape(_lib.COLOR_MAX_BLOCKS, ragged=False)
    c = luma_case(shape, normalize)
    _check_luma(offset_by_one(c["result"]), offset_by_one(c["content"]), c["want"], normalize, f"luma {shape} unaligned",
                lambda: offset_by_one(nan(c["result"].shape)))


def test_luma_refusals():
    c = luma_case((4, 4), False)
    result, content = c["result"].to(DEV), c["content"].to(DEV)
    before = content.clone()
    with pytest.raises(RuntimeError, match="STV_ERR_ARG"):
        ops.luma_transfer(result, content, out=content, mean=None, std=None)      # out == content
    with pytest.raises(RuntimeError, match="STV_ERR_ARG"):
        ops.luma_transfer(result, content, mean=MEAN, std=None)
    with pytest.raises(RuntimeError, match="luma_transfer: result is"):
        ops.luma_transfer(result, torch.zeros(1, 3, 4, 8, device=DEV), mean=None, std=None)
    torch.cuda.synchronize()
    assert torch.equal(content, before)
