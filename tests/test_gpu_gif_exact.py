"""The two GIF kernels on a real MI355X against their NumPy twins (tests/gif_ref.py): integer arithmetic, so every
comparison is ``torch.equal``.  Shapes are the smallest that reach every path: one pixel, fewer pixels than a work item's
four, ``H*W % 4 != 0`` (the byte tail), fewer items than one workgroup, several workgroups (an item is four pixels, a
workgroup 256 items: 64x64 is four workgroups), sides that are no multiple of the 8x8 Bayer tile, and frames at byte
offsets of a packed store that are not 4-byte aligned (the scalar path) and that are (the vector path)."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from style_transfer_visualizer_amd import _lib, ops
from tests import gif_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
HIST_SHAPES = [(1, 1), (3, 5), (8, 8), (17, 23), (64, 64), (96, 80)]
MAP_SHAPES = [(1, 1), (3, 5), (9, 13), (17, 23), (64, 64), (40, 96)]
COLORS = [1, 2, 17, 255, 256]
SPREADS = [0, 16, 64]


@functools.lru_cache(maxsize=None)
def _frame(H: int, W: int, kind: str = "random") -> np.ndarray:
    rng = np.random.default_rng(1000 * H + W)
    if kind == "random":
        out = rng.integers(0, 256, size=(H, W, 3))
    elif kind == "constant":
        out = np.broadcast_to(np.array([37, 201, 118]), (H, W, 3))
    else:                                                       # only 0 and 255
        out = rng.integers(0, 2, size=(H, W, 3)) * 255
    out = np.ascontiguousarray(out.astype(np.uint8))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _palette(n: int) -> np.ndarray:
    out = np.random.default_rng(n).integers(0, 256, size=(n, 3)).astype(np.uint8)
    out.setflags(write=False)
    return out


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.array(a)).to(DEV)


def _zero_hist() -> torch.Tensor:
    return torch.zeros(_lib.GIF_HIST_BINS, dtype=torch.int32, device=DEV)


def _want_hist(*frames: np.ndarray) -> torch.Tensor:
    total = sum(gif_ref.frame_hist(f) for f in frames)
    return torch.from_numpy(total.astype(np.int32))


@pytest.mark.parametrize("kind", ["random", "constant", "binary"])
@pytest.mark.parametrize("shape", HIST_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_histogram_equals_bincount(shape, kind):
    frame = _frame(*shape, kind)
    got = ops.frame_hist(_dev(frame), _zero_hist()).cpu()
    assert int(got.sum()) == shape[0] * shape[1]
    assert torch.equal(got, _want_hist(frame))
    if kind == "constant":
        assert int(got.max()) == shape[0] * shape[1]            # every pixel in one bin: the contended case


@pytest.mark.parametrize("shape", [(96, 80), (17, 23), (3, 1000)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_merges_in_front_of_the_atomics_lose_no_pixel(shape):
    """The kernel adds a run of equal bins inside a work item, and a wave whose 256 pixels share one bin, with one atomic.
    Rows of one colour with a stripe through them: uniform waves next to mixed ones, runs of every length, a wave that
    is uniform but for its last, short item (17x23)."""
    H, W = shape
    frame = np.repeat((np.arange(H, dtype=np.uint8) * 37)[:, None, None], W, axis=1).repeat(3, axis=2)
    frame[:, W // 2:W // 2 + 3] = (255, 0, 9)
    frame = np.ascontiguousarray(frame)
    got = ops.frame_hist(_dev(frame), _zero_hist()).cpu()
    assert int(got.sum()) == H * W and torch.equal(got, _want_hist(frame))
    flat = np.full((H, W, 3), 200, dtype=np.uint8)
    assert torch.equal(ops.frame_hist(_dev(flat), _zero_hist()).cpu(), _want_hist(flat))


def test_histogram_accumulates_over_frames():
    a, b = _frame(17, 23), _frame(64, 64, "binary")
    hist = _zero_hist()
    ops.frame_hist(_dev(a), hist)
    ops.frame_hist(_dev(b), hist)
    assert torch.equal(hist.cpu(), _want_hist(a, b))
    assert torch.equal(hist.cpu(), ops.frame_hist(_dev(a), _zero_hist()).cpu() + ops.frame_hist(_dev(b), _zero_hist()).cpu())


@pytest.mark.parametrize("shape", [(5, 5), (17, 23), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_histogram_of_a_frame_at_byte_offset_75(shape):
    frame = _frame(*shape)
    n = frame.size
    buf = torch.full((75 + n + 64,), 255, dtype=torch.uint8, device=DEV)          # (255s around: a read outside would count)
    buf[75:75 + n] = _dev(frame).reshape(-1)
    view = buf[75:75 + n].view(*shape, 3)
    assert view.data_ptr() % 4 == 3
    assert torch.equal(ops.frame_hist(view, _zero_hist()).cpu(), _want_hist(frame))


@pytest.mark.parametrize("spread", SPREADS)
@pytest.mark.parametrize("n_colors", COLORS)
@pytest.mark.parametrize("shape", MAP_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_map_equals_the_brute_force_twin(shape, n_colors, spread):
    frame, palette = _frame(*shape), _palette(n_colors)
    got = ops.gif_map(_dev(frame), _dev(palette), spread).cpu()
    assert int(got.max()) < n_colors
    assert torch.equal(got, torch.from_numpy(gif_ref.gif_map(frame, palette, spread)))


def test_the_lowest_index_wins_a_tie():
    frame = _frame(17, 23)
    palette = np.concatenate([_palette(17), _palette(17), _palette(17)[:5]])        # every entry two or three times
    got = ops.gif_map(_dev(frame), _dev(palette), 16).cpu()
    assert int(got.max()) < 17
    assert torch.equal(got, torch.from_numpy(gif_ref.gif_map(frame, palette, 16)))
    tie = np.array([[[1, 0, 0]]], dtype=np.uint8)
    pal = np.array([[0, 0, 0], [2, 0, 0]], dtype=np.uint8)
    assert ops.gif_map(_dev(tie), _dev(pal), 0).cpu().tolist() == [[0]]
    assert ops.gif_map(_dev(tie), _dev(pal[::-1].copy()), 0).cpu().tolist() == [[0]]


@pytest.mark.parametrize("value", [0, 255])
def test_the_offset_is_clamped_at_both_ends(value):
    frame = np.full((17, 23, 3), value, dtype=np.uint8)
    palette = np.stack([np.arange(0, 256, 4)] * 3, axis=1).astype(np.uint8)         # a grey ramp: the offset shows in the index
    got = ops.gif_map(_dev(frame), _dev(palette), 64).cpu()
    want = gif_ref.gif_map(frame, palette, 64)
    assert len(np.unique(want)) > 4                                                  # the dither reaches the indices
    assert torch.equal(got, torch.from_numpy(want))


@pytest.mark.parametrize("shape", [(5, 5), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_frame_one_of_a_packed_store(shape):
    """Frame 1 starts at byte H*W*3 and its index plane at byte H*W: 75 and 25 for 5x5 (scalar path), aligned for 64x64."""
    H, W = shape
    frames = np.stack([_frame(H, W, "binary"), _frame(H, W), _frame(H, W, "constant")])
    palette = _palette(255)
    store = _dev(frames)
    index = torch.full((3, H, W), 255, dtype=torch.uint8, device=DEV)
    assert (store[1].data_ptr() - store.data_ptr(), index[1].data_ptr() - index.data_ptr()) == (H * W * 3, H * W)
    ops.gif_map(store[1], _dev(palette), 16, out=index[1])
    got = index.cpu()
    assert torch.equal(got[1], torch.from_numpy(gif_ref.gif_map(frames[1], palette, 16)))
    assert bool((got[0] == 255).all()) and bool((got[2] == 255).all())               # the neighbours' planes are untouched
    hist = ops.frame_hist(store[1], _zero_hist()).cpu()
    assert torch.equal(hist, _want_hist(frames[1]))


def test_wrappers_refuse_what_the_kernels_cannot_take():
    frame, palette = _dev(_frame(8, 8)), _dev(_palette(4))
    with pytest.raises(RuntimeError, match="uint8 frame"):
        ops.frame_hist(frame.float(), _zero_hist())
    with pytest.raises(RuntimeError, match="hist is"):
        ops.frame_hist(frame, torch.zeros(100, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="out is"):
        ops.gif_map(frame, palette, 0, out=torch.empty(8, 9, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="STV_ERR_ARG"):
        ops.gif_map(frame, palette, 65)
    with pytest.raises(RuntimeError, match="out is"):                               # a slot of another size is never written
        ops.image_to_u8(torch.zeros(1, 3, 8, 8, device=DEV), mean=None, std=None, rounding=False,
                        out=torch.empty(8, 7, 3, dtype=torch.uint8, device=DEV))
