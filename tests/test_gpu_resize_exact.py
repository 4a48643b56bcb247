"""stv_resize2x on a real MI355X against its NumPy fp32 twin (tests/resize_ref.py), bit for bit: the arithmetic of both
modes is fixed to the rounding (every product and sum rounded on its own, in a stated order), so ``torch.equal`` is the
comparison for integer-valued and for random images alike - no tolerance.  Outputs start as NaN.

The integer pattern differs per channel and jumps by 12 or more between the last pixel of a row and the first of the next
and by 11 or more between the last row of a plane and the first of the next: a read across a row end or a channel plane
shows as a wrong value.
"""
from __future__ import annotations

import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from style_transfer_visualizer_amd import _lib, ops
from tests import resize_ref as rr
from tests.conftest import record_parity

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = torch.float32
UP, DOWN = _lib.RESIZE_UP2, _lib.RESIZE_DOWN2
TWIN = {UP: rr.up2, DOWN: rr.down2}
NAME = {UP: "up2", DOWN: "down2"}


def _second_trip_shape(mode: int, ragged: bool) -> tuple[int, int, int]:
    """The smallest near-square C = 3 INPUT whose output's work items (RESIZE_VEC output pixels of one row each) exceed
    one pass of the capped grid (RESIZE_MAX_BLOCKS workgroups x RESIZE_THREADS items): the grid-stride loop runs twice.
    One output row (DOWN2) or one input row (UP2: two output rows) less fits in one pass."""
    per_pass = _lib.RESIZE_MAX_BLOCKS * _lib.RESIZE_THREADS
    w4 = math.isqrt(per_pass // 3) + 1
    Ho = per_pass // (3 * w4) + 1
    if mode == UP:
        Ho += Ho & 1                                         # an UP2 output has an even number of rows
        assert 3 * Ho * w4 > per_pass >= 3 * (Ho - 2) * w4
        Wo = _lib.RESIZE_VEC * w4 - (2 if ragged else 0)     # ragged: an odd input width
        return 3, Ho // 2, Wo // 2
    assert 3 * Ho * w4 > per_pass >= 3 * (Ho - 1) * w4
    Wo = _lib.RESIZE_VEC * w4 - (3 if ragged else 0)
    return 3, 2 * Ho, 2 * Wo


SHAPES = {UP: [(3, 1, 1), (3, 1, 7), (3, 5, 1), (3, 3, 5), (3, 17, 33), (3, 64, 48), (1, 2, 2),
               _second_trip_shape(UP, ragged=False), _second_trip_shape(UP, ragged=True)],
          DOWN: [(3, 2, 2), (3, 2, 14), (3, 10, 2), (3, 6, 10), (3, 34, 66), (3, 128, 96),
                 _second_trip_shape(DOWN, ragged=False), _second_trip_shape(DOWN, ragged=True)]}
CASES = [(m, s) for m in (UP, DOWN) for s in SHAPES[m]]
_ids = lambda v: NAME[v[0]] + "-" + "x".join(map(str, v[1]))      # noqa: E731


@functools.lru_cache(maxsize=None)
def case(mode: int, shape: tuple[int, int, int], kind: str) -> dict:
    """Input and the twin's output for one mode, shape and kind of values; computed once, shared, never modified."""
    x = rr.pattern(*shape) if kind == "int" else rr.randn3(*shape, seed=31 * shape[1] + shape[2] + mode)
    want = TWIN[mode](x)
    assert want.dtype == np.float32
    return {"x": torch.from_numpy(x), "want": torch.from_numpy(want)}


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
    record_parity("exact 2x resize", "differing elements", 0.0, 0.0, f"{len(CASES)} mode/shape cases x integer and random values, bit for bit")


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("mode_shape", CASES, ids=_ids)
def test_against_the_twin(mode_shape, kind):
    mode, shape = mode_shape
    c = case(mode, shape, kind)
    x = c["x"].to(DEV)
    out = nan(c["want"].shape)
    back = ops.resize2x(x, mode, out=out)
    assert back is out
    same(out, c["want"], f"{NAME[mode]} {shape} {kind}")
    same(x, c["x"], f"{NAME[mode]} {shape} {kind}: the input afterwards")


@pytest.mark.parametrize("mode_shape", [(UP, (3, 17, 33)), (UP, (3, 64, 48)), (DOWN, (3, 34, 66)), (DOWN, (3, 128, 96))], ids=_ids)
def test_rank_four_and_fresh_output(mode_shape):
    """[1, 3, H, W] in, [1, 3, H', W'] out; without ``out`` a new tensor of the output's shape comes back."""
    mode, shape = mode_shape
    c = case(mode, shape, "randn")
    got = ops.resize2x(c["x"].to(DEV)[None], mode)
    assert got.dim() == 4 and got.shape[0] == 1
    same(got[0], c["want"], f"{NAME[mode]} {shape}: rank 4")
    got3 = ops.resize2x(c["x"].to(DEV), mode)
    same(got3, c["want"], f"{NAME[mode]} {shape}: rank 3, fresh output")


@pytest.mark.parametrize("offset_out", [True, False], ids=["both-offset", "input-offset"])
@pytest.mark.parametrize("mode_shape", [(UP, (3, 4, 8)), (DOWN, (3, 8, 16))], ids=_ids)
def test_rows_that_do_not_start_on_a_vector(mode_shape, offset_out):
    """Row lengths that would take the vector path, but the view starts 4 bytes past a 16-byte boundary: the scalar
    path, the same bits; the float in front of the output view and the one behind it stay NaN."""
    mode, shape = mode_shape
    c = case(mode, shape, "int")
    n = c["x"].numel()
    x = torch.zeros(n + 1, dtype=F32, device=DEV)[1:].view(shape)
    x.copy_(c["x"])
    assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    m = c["want"].numel()
    buf = nan((m + 2,))
    out = (buf[1:m + 1] if offset_out else nan((m,))).view(c["want"].shape)
    assert out.data_ptr() % 16 == (4 if offset_out else 0)
    ops.resize2x(x, mode, out=out)
    same(out, c["want"], f"{NAME[mode]} {shape}: unaligned rows")
    assert bool(torch.isnan(buf[0])) and bool(torch.isnan(buf[m + 1]))
    if offset_out:                       # an aligned input, an offset output
        out.fill_(float("nan"))
        ops.resize2x(c["x"].to(DEV), mode, out=out)
        same(out, c["want"], f"{NAME[mode]} {shape}: aligned input, offset output")


def test_bad_arguments_are_refused():
    """STV_ERR_ARG from the entry point (RuntimeError from the binding); nothing is launched: the output stays NaN."""
    x = case(DOWN, (3, 6, 10), "int")["x"].to(DEV)
    out = nan((3, 12, 20))
    lib = _lib.load()
    px, po = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.data_ptr())
    bad = [
        (None, po, 3, 6, 10, UP), (px, None, 3, 6, 10, UP), (px, px, 3, 6, 10, UP),                 # null, null, x == y
        (px, po, 0, 6, 10, UP), (px, po, 3, 0, 10, DOWN), (px, po, 3, 6, -2, UP),                     # non-positive sizes
        (px, po, 3, 5, 10, DOWN), (px, po, 3, 6, 9, DOWN),                                           # odd H / W with DOWN2
        (px, po, 3, 6, 10, 2), (px, po, 3, 6, 10, -1),                                               # unknown modes
        (px, po, 2, 16384, 16384, DOWN),                                                             # input of 2 GiB
        (px, po, 2, 8192, 8192, UP),                                                                 # output of 2 GiB
    ]
    for args in bad:
        assert lib.stv_resize2x(*args, None) == 1, f"stv_resize2x{args[2:]} was not refused"
    with pytest.raises(RuntimeError, match="STV_ERR_ARG"):
        ops.resize2x(torch.zeros(3, 5, 4, device=DEV), DOWN)
    with pytest.raises(RuntimeError, match="STV_ERR_ARG"):
        ops.resize2x(x, 7, out=out)
    with pytest.raises(RuntimeError, match="expected"):
        ops.resize2x(x, UP, out=nan((3, 6, 10)))
    with pytest.raises(RuntimeError, match="fp32 image"):
        ops.resize2x(x.to(torch.bfloat16), UP)
    with pytest.raises(RuntimeError, match="fp32 image"):
        ops.resize2x(torch.zeros(2, 3, 4, 4, device=DEV), UP)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
