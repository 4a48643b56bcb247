"""ops.resize (stv_resize_axis) on a real MI355X against its NumPy fp32 twin (tests/resize_general_ref.py), bit for bit: the
tables are float64 host arithmetic rounded to fp32 once, and the accumulation is fixed to the rounding (every product and sum
rounded on its own, taps in ascending order), so ``torch.equal`` is the comparison for integer-valued and for random images
alike - no tolerance.  Output and intermediate start as NaN.

The integer pattern (tests/resize_ref.py) differs per channel and jumps by 12 or more between the last pixel of a row and the
first of the next and by 11 or more between the last row of a plane and the first of the next: a read across a row end or a
channel plane shows as a wrong value.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch

from style_transfer_visualizer_amd import _lib, ops
from tests import resize_general_ref as gr
from tests.conftest import record_parity

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = torch.float32
FILTERS = ("bilinear", "bicubic", "lanczos")
PER_PASS = _lib.RESIZE_AXIS_MAX_BLOCKS * _lib.RESIZE_AXIS_THREADS


def _second_trip_size(ragged: bool, rows_short: int = 0) -> tuple[int, int]:
    """The smallest near-square C = 3 OUTPUT whose work items (RESIZE_AXIS_VEC output pixels of one row each) exceed one
    pass of the capped grid (RESIZE_AXIS_MAX_BLOCKS workgroups x RESIZE_AXIS_THREADS items): the grid-stride loop of the row
    pass runs twice.  From the 300-row input the column pass (3 * 300 rows of the same width) runs it twice as well.
    ``rows_short = 1``: one output row less fits in one pass of the row pass."""
    w4 = math.isqrt(PER_PASS // 3) + 1
    Ho = PER_PASS // (3 * w4) + 1
    assert 3 * Ho * w4 > PER_PASS >= 3 * (Ho - 1) * w4 and 3 * 300 * w4 > PER_PASS
    return Ho - rows_short, _lib.RESIZE_AXIS_VEC * w4 - (3 if ragged else 0)


BIG = (3, 300, 300)
CASES = [((3, 1, 1), (3, 5)), ((3, 5, 7), (3, 11)), ((3, 37, 53), (16, 20)), ((3, 16, 20), (37, 53)),
         ((3, 64, 48), (64, 31)),                # rows skipped
         ((3, 64, 48), (23, 48)),                # columns skipped
         ((1, 100, 75), (13, 9)),                # long rows of taps
         ((3, 40, 36), (24, 32)),                # vector variant in both passes
         ((3, 40, 36), (24, 30)),                # ragged rows: the guarded variant
         (BIG, _second_trip_size(ragged=False)), (BIG, _second_trip_size(ragged=True)),
         (BIG, _second_trip_size(ragged=False, rows_short=1))]
_ids = lambda v: "x".join(map(str, v[0])) + "-" + "x".join(map(str, v[1]))      # noqa: E731


@functools.lru_cache(maxsize=None)
def case(shape: tuple[int, int, int], size: tuple[int, int], name: str, kind: str) -> dict:
    """Input and the twin's output for one shape, size, filter and kind of values; computed once, shared, never modified."""
    x = gr.pattern(*shape) if kind == "int" else gr.randn3(*shape, seed=31 * shape[1] + shape[2] + size[0])
    want = gr.resize(x, size, name)
    assert want.dtype == np.float32 and want.shape == (shape[0], *size)
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
    record_parity("exact general resize", "differing elements", 0.0, 0.0,
                  f"{len(CASES)} shape/size cases x {len(FILTERS)} filters x integer and random values, bit for bit")


@pytest.mark.parametrize("kind", ["int", "randn"])
@pytest.mark.parametrize("name", FILTERS)
@pytest.mark.parametrize("shape_size", CASES, ids=_ids)
def test_against_the_twin(shape_size, name, kind):
    shape, size = shape_size
    c = case(shape, size, name, kind)
    x = c["x"].to(DEV)
    out, tmp = nan(c["want"].shape), nan((shape[0], shape[1], size[1]))
    back = ops.resize(x, size, name, out=out, tmp=tmp)
    assert back is out
    what = f"{name} {shape} -> {size} {kind}"
    same(out, c["want"], what)
    same(x, c["x"], f"{what}: the input afterwards")
    if size[0] != shape[1] and size[1] != shape[2]:            # both passes ran: the intermediate is the column pass alone
        same(tmp, torch.from_numpy(gr.resize(c["x"].numpy(), (shape[1], size[1]), name)), f"{what}: the intermediate")
    else:                                                      # one pass: straight from x into out
        assert bool(torch.isnan(tmp).all()), f"{what}: the intermediate was written although one pass is skipped"


@pytest.mark.parametrize("name", FILTERS)
def test_same_size_returns_the_input_without_a_launch(name):
    x = torch.from_numpy(gr.pattern(3, 9, 9)).to(DEV)
    out = nan((3, 9, 9))
    back = ops.resize(x, (9, 9), name, out=out)
    assert back is x
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert ops.resize(x[None], (9, 9), name).shape == (1, 3, 9, 9)


@pytest.mark.parametrize("shape_size", [((3, 37, 53), (16, 20)), ((3, 16, 20), (37, 53)), ((3, 40, 36), (24, 32))], ids=_ids)
def test_rank_four_and_fresh_output(shape_size):
    """[1, 3, H, W] in, [1, 3, Ho, Wo] out; without ``out`` and ``tmp`` new tensors are made."""
    shape, size = shape_size
    c = case(shape, size, "lanczos", "randn")
    got = ops.resize(c["x"].to(DEV)[None], size)
    assert got.dim() == 4 and got.shape[0] == 1
    same(got[0], c["want"], f"{shape} -> {size}: rank 4, default filter")
    same(ops.resize(c["x"].to(DEV), size, "lanczos"), c["want"], f"{shape} -> {size}: rank 3, fresh output")


@pytest.mark.parametrize("name", FILTERS)
@pytest.mark.parametrize("offset_out", [True, False], ids=["both-offset", "input-offset"])
def test_rows_that_do_not_start_on_a_vector(offset_out, name):
    """Row lengths that take the vector variant, but the view starts 4 bytes past a 16-byte boundary: the guarded variant,
    the same bits; the float in front of the output view and the one behind it stay NaN."""
    shape, size = (3, 40, 36), (24, 32)
    c = case(shape, size, name, "int")
    n = c["x"].numel()
    x = torch.zeros(n + 1, dtype=F32, device=DEV)[1:].view(shape)
    x.copy_(c["x"])
    assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    m = c["want"].numel()
    buf = nan((m + 2,))
    out = (buf[1:m + 1] if offset_out else nan((m,))).view(c["want"].shape)
    assert out.data_ptr() % 16 == (4 if offset_out else 0)
    ops.resize(x, size, name, out=out)
    same(out, c["want"], f"{name} {shape} -> {size}: unaligned rows")
    assert bool(torch.isnan(buf[0])) and bool(torch.isnan(buf[m + 1]))
    # a single pass from an offset input: rows only (16-byte loads need an aligned x), columns only
    for one in ((24, 36), (40, 32)):
        same(ops.resize(x, one, name), torch.from_numpy(gr.resize(c["x"].numpy(), one, name)), f"{name} {shape} -> {one}: offset input")


@pytest.mark.parametrize("shape_size", [((3, 37, 53), (16, 20)), ((3, 40, 36), (24, 32)), ((3, 64, 48), (23, 48))], ids=_ids)
def test_a_callers_buffer_is_written_and_nothing_beyond_it(shape_size):
    """``out`` and ``tmp`` are views into NaN canvases with a guard row of the output's width on either side."""
    shape, size = shape_size
    c = case(shape, size, "bicubic", "randn")
    C, (Ho, Wo), H = shape[0], size, shape[1]
    canvas, mid = nan((C * Ho + 2, Wo)), nan((C * H + 2, Wo))
    out, tmp = canvas[1:-1].view(C, Ho, Wo), mid[1:-1].view(C, H, Wo)
    back = ops.resize(c["x"].to(DEV), size, "bicubic", out=out, tmp=tmp)
    assert back is out
    same(out, c["want"], f"{shape} -> {size}: out=")
    for name, guard in (("out", canvas), ("tmp", mid)):
        assert bool(torch.isnan(guard[0]).all()) and bool(torch.isnan(guard[-1]).all()), f"a guard row of {name} was written"


def test_bad_arguments_are_refused():
    """RuntimeError from the binding or STV_ERR_ARG from the entry point; nothing is launched: the output stays NaN."""
    x = case((3, 5, 7), (3, 11), "lanczos", "int")["x"].to(DEV)
    out = nan((3, 3, 11))
    with pytest.raises(RuntimeError, match="expected"):
        ops.resize(x, (3, 11), out=nan((3, 3, 12)))
    with pytest.raises(RuntimeError, match="tmp is"):
        ops.resize(x, (3, 11), out=out, tmp=nan((3, 5, 12)))
    with pytest.raises(RuntimeError, match="fp32 image"):
        ops.resize(x.to(torch.bfloat16), (3, 11))
    with pytest.raises(RuntimeError, match="fp32 image"):
        ops.resize(torch.zeros(2, 3, 4, 4, device=DEV), (3, 11))
    with pytest.raises(RuntimeError, match="unknown filter"):
        ops.resize(x, (3, 11), "box", out=out)
    with pytest.raises(RuntimeError, match="positive"):
        ops.resize(x, (0, 11))
    lib = _lib.load()
    tab = torch.zeros(64, dtype=torch.int32, device=DEV)
    px, po, pt = x.data_ptr(), out.data_ptr(), tab.data_ptr()
    for args in ((px, px, 3, 5, 7, 3, 0, pt, pt, pt, 1), (px, po, 3, 5, 7, 3, 2, pt, pt, pt, 1), (px, po, 3, 5, 7, 3, 0, pt, pt, pt, 0),
                 (px, po, 3, 5, 7, 0, 0, pt, pt, pt, 1), (px, po, 3, 5, 7, 3, 0, None, pt, pt, 1)):
        assert lib.stv_resize_axis(*args, None) == 1, f"stv_resize_axis{args[2:]} was not refused"
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
