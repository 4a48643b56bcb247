"""The four JPEG kernels on a real MI355X against their NumPy twins (tests/jpeg_ref.py): integer arithmetic, so every
comparison is ``torch.equal``.

``stv_jpeg_dct``: frame sizes from one pixel (one MCU, everything replicated) over sides that are no multiple of 8 or 16
(17x15, 15x17, 33x47: the clamped loads at both edges) to a frame of 300 MCUs (16x4800: 57 workgroups of 32 blocks, the last
one part empty); the frame at a 4-byte aligned base and at an odd byte offset (the 32-bit loads and the byte loads); constant,
primary, noise, checkerboard and gradient content; tables at three qualities and all-ones tables, which leave the
coefficients unscaled and so reach the clamps and the categories 10 and 11.

``stv_jpeg_block_bits`` / ``stv_jpeg_scan`` / ``stv_jpeg_emit``: planted coefficient arrays - see ``_planted``."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from style_transfer_visualizer_amd import mjpeg, ops
from tests import jpeg_ref as jr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SHAPES = [(1, 1), (8, 8), (16, 16), (17, 15), (15, 17), (33, 47), (96, 80), (16, 4800)]
TABLES = ["q15", "q50", "q95", "ones"]
PRIMARIES = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255)]


@functools.lru_cache(maxsize=None)
def _qtabs(name: str) -> np.ndarray:
    out = np.ones((2, 64), dtype=np.int32) if name == "ones" else mjpeg.quant_tables(int(name[1:]))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _frame(H: int, W: int, kind: str) -> np.ndarray:
    rng = np.random.default_rng(1000 * H + W)
    y, x = np.mgrid[0:H, 0:W]
    if kind == "noise":
        out = rng.integers(0, 256, size=(H, W, 3))
    elif kind == "checker":                                     # one-pixel checkerboard of 0 / 255
        out = np.repeat((((x + y) & 1) * 255)[:, :, None], 3, axis=2)
    elif kind == "gradient":
        out = np.stack([(x * 7) % 256, (y * 5) % 256, ((x + y) * 3) % 256], axis=-1)
    elif kind == "two":                                         # only 0 and 255, per channel
        out = rng.integers(0, 2, size=(H, W, 3)) * 255
    else:                                                       # "c<r>,<g>,<b>": one colour
        out = np.broadcast_to(np.array([int(v) for v in kind[1:].split(",")]), (H, W, 3))
    out = np.ascontiguousarray(out.astype(np.uint8))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _want(H: int, W: int, kind: str, table: str) -> torch.Tensor:
    return torch.from_numpy(jr.dct_quant(_frame(H, W, kind), _qtabs(table)))


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.array(a)).to(DEV)


def _at_offset(frame: np.ndarray, offset: int) -> torch.Tensor:
    """The frame on the device at ``offset`` bytes behind a 256-byte aligned base, 255s around it."""
    n = frame.size
    buf = torch.full((offset + n + 64,), 255, dtype=torch.uint8, device=DEV)
    buf[offset:offset + n] = _dev(frame).reshape(-1)
    view = buf[offset:offset + n].view(*frame.shape)
    assert view.data_ptr() % 4 == offset % 4
    return view


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_dct_equals_the_twin(shape, table):
    H, W = shape
    for kind in ("noise", "checker", "gradient", "two"):
        frame, want = _frame(H, W, kind), _want(H, W, kind, table)
        for offset in (0, 1):
            got = ops.jpeg_dct(_at_offset(frame, offset), _qtabs(table)).cpu()
            assert got.shape == (ops.jpeg_blocks(H, W), 64)
            assert torch.equal(got, want), f"{kind} at byte offset {offset}: {int((got != want).sum())} coefficients differ"


@pytest.mark.parametrize("table", TABLES)
def test_dct_of_constant_frames(table):
    """0, 255 and the six primaries and secondaries: only DC terms, at the ends of the colour conversion's range."""
    for colour in [(0, 0, 0), (255, 255, 255), *PRIMARIES]:
        kind = "c" + ",".join(str(v) for v in colour)
        for H, W in ((16, 16), (17, 15)):
            want = _want(H, W, kind, table)
            got = ops.jpeg_dct(_dev(_frame(H, W, kind)), _qtabs(table)).cpu()
            assert torch.equal(got, want)
            assert not bool(want[:, 1:].any())


def test_all_ones_tables_reach_the_clamps_and_the_top_categories():
    black, checker = _want(16, 16, "c0,0,0", "ones"), _want(96, 80, "checker", "ones")
    assert int(black[0, 0]) == -1024                            # DC of a block of -128: -1024 is kept, not clamped to -1023: category 11
    assert 512 < int(checker[:, 1:].abs().max()) <= 1023        # category 10, the largest of an AC coefficient


def test_dct_writes_one_slot_of_a_store():
    frame = _frame(33, 47, "noise")
    n = ops.jpeg_blocks(33, 47)
    store = torch.full((3, n, 64), 77, dtype=torch.int16, device=DEV)
    ops.jpeg_dct(_dev(frame), _qtabs("q50"), out=store[1])
    got = store.cpu()
    assert torch.equal(got[1], _want(33, 47, "noise", "q50")) and bool((got[0] == 77).all()) and bool((got[2] == 77).all())
    with pytest.raises(RuntimeError, match="out is"):
        ops.jpeg_dct(_dev(frame), _qtabs("q50"), out=store[:, :-1][1])
    with pytest.raises(RuntimeError, match="STV_ERR_ARG"):
        ops.jpeg_dct(_dev(frame), np.zeros(128, dtype=np.int32))


# ---- the entropy kernels ---------------------------------------------------------------------------------------------------

EDGES = [1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 127, 128, 255, 256, 511, 512, 1023]


@functools.lru_cache(maxsize=None)
def _planted() -> np.ndarray:
    """Three frames of three MCUs (18 blocks), int16 ``[3, 18, 64]`` in zigzag order.

    Frame 0: block 0 all zero (the first block of a frame: predictor 0, DC difference 0, an EOB alone); blocks 1..4 a value
    behind zero runs of 15, 16, 17 and 47 (none, one and two ZRL); block 5 a non-zero coefficient 63 (no EOB); blocks 6..11
    (MCU 1) +-1 ... +-1023 at every category edge, in luminance and in chrominance blocks; MCU 2 DCs of 1023 / -1024 / 1023
    / -1024 in the four Y blocks (differences of -2047 and +2047) and of -1024 against MCU 1's 1023 in Cb (-2047) and Cr.
    Frame 1: dense random coefficients of large magnitude (blocks of hundreds of bits: words in the middle of a block).
    Frame 2: all zero but separate DC chains - Y, Cb and Cr each take their own predictor over the three MCUs."""
    rng = np.random.default_rng(7)
    c = np.zeros((3, 18, 64), dtype=np.int16)
    for block, run in zip((1, 2, 3, 4), (15, 16, 17, 47), strict=True):
        c[0, block, 1 + run] = -5
        c[0, block, 0] = block
    c[0, 5, 63], c[0, 5, 1] = 3, -1
    for block in range(6, 12):
        vals = np.array([s * v for v in EDGES for s in (1, -1)])
        c[0, block, 1:1 + len(vals)] = vals if block % 2 == 0 else vals[::-1]
        c[0, block, 0] = 1023 if block >= 10 else 100 * (block - 8)
    c[0, 12:16, 0] = (1023, -1024, 1023, -1024)
    c[0, 16, 0], c[0, 17, 0] = -1024, -1024
    c[1] = np.clip(np.round(rng.laplace(0, 200, size=(18, 64))), -1023, 1023).astype(np.int16)
    c[1, :, 40:] = 0
    c[2, :, 0] = np.array([5, 5, 6, 4, -9, 30] * 3) + np.repeat(np.arange(3), 6) * np.array([1, 1, 1, 1, -7, 11] * 3)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _large() -> np.ndarray:
    """Two frames of 50 MCUs (300 blocks: several workgroups, scan runs of two blocks per thread), sparse like real frames."""
    rng = np.random.default_rng(11)
    c = np.round(rng.laplace(0, 6, size=(2, 300, 64)) * np.linspace(4, 0.05, 64)).astype(np.int16)
    c[1, :, 10:] = 0
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _twin(which: str):
    coefs = _planted() if which == "planted" else _large()
    bits = np.stack([jr.block_bits(f) for f in coefs]).astype(np.int64)
    offsets = np.cumsum(bits, axis=1) - bits
    scans = [jr.encode_scan(f) for f in coefs]
    return bits, offsets, bits.sum(axis=1), scans


@pytest.mark.parametrize("which", ["planted", "large"])
def test_lengths_offsets_and_totals(which):
    coefs = _planted() if which == "planted" else _large()
    bits, offsets, totals, scans = _twin(which)
    assert all(len(s) == (t + 7) // 8 for s, t in zip(scans, totals, strict=True)) and len(set(totals.tolist())) == len(totals)
    got_bits = ops.jpeg_block_bits(_dev(coefs))
    got_offsets, got_totals = ops.jpeg_scan(got_bits)
    assert torch.equal(got_bits.cpu(), torch.from_numpy(bits.astype(np.int32)))
    assert torch.equal(got_offsets.cpu(), torch.from_numpy(offsets.astype(np.int32)))
    assert torch.equal(got_totals.cpu(), torch.from_numpy(totals.astype(np.int32)))
    if which == "planted":
        assert bits[0, 0] == 2 + 4                              # DC category 0 (00) and EOB (1010)
        assert int(bits.max()) > 64                             # a block with whole words of its own


@pytest.mark.parametrize("which", ["planted", "large"])
def test_every_stream_byte(which):
    """All frames in one launch, streams of unequal length behind a base table with gaps: every byte of the buffer is compared,
    so a write outside a frame's stream shows too."""
    coefs = _planted() if which == "planted" else _large()
    bits, offsets, totals, scans = _twin(which)
    base, at = [], 8
    for s in scans:
        base.append(at)
        at += (len(s) + 3) // 4 * 4 + 12                        # (gaps between the streams, and in front of the first)
    want = np.zeros(at + 4, dtype=np.uint8)
    for b, s in zip(base, scans, strict=True):
        want[b:b + len(s)] = np.frombuffer(s, dtype=np.uint8)
    stream = torch.zeros(at + 4, dtype=torch.uint8, device=DEV)
    dev = _dev(coefs)
    got_offsets, _ = ops.jpeg_scan(ops.jpeg_block_bits(dev))
    ops.jpeg_emit(dev, got_offsets, _dev(np.array(base, dtype=np.int32)), stream)
    got = stream.cpu()
    assert torch.equal(got, torch.from_numpy(want)), f"{int((got != torch.from_numpy(want)).sum())} bytes differ"
    assert all(s[-1] & ((1 << (-int(t) % 8)) - 1) == (1 << (-int(t) % 8)) - 1 for s, t in zip(scans, totals, strict=True))      # 1-padding


def test_a_frame_range_of_a_store_and_the_capacity_guard():
    """Frames 1..2 of the planted store as a batch of their own (what ``close()`` does), and a buffer that ends inside the last
    stream: nothing is written past it."""
    coefs = _planted()
    _, offsets, _, scans = _twin("planted")
    dev = _dev(coefs)
    got_offsets, _ = ops.jpeg_scan(ops.jpeg_block_bits(dev))
    first = (len(scans[1]) + 3) // 4 * 4
    size = first + (len(scans[2]) + 3) // 4 * 4
    stream = torch.zeros(size, dtype=torch.uint8, device=DEV)
    ops.jpeg_emit(dev[1:3], got_offsets[1:3], _dev(np.array([0, first], dtype=np.int32)), stream)
    got = stream.cpu().numpy()
    assert got[:len(scans[1])].tobytes() == scans[1] and got[first:first + len(scans[2])].tobytes() == scans[2]
    short = 64                                                  # bytes: inside frame 1's stream
    guard = torch.zeros(short + 64, dtype=torch.uint8, device=DEV)
    ops.jpeg_emit(dev[1:2], got_offsets[1:2], _dev(np.array([0], dtype=np.int32)), guard[:short])
    got = guard.cpu().numpy()
    assert got[:short].tobytes() == scans[1][:short] and not got[short:].any()


def test_wrappers_refuse_what_the_kernels_cannot_take():
    coefs = _dev(_planted())
    with pytest.raises(RuntimeError, match="int16 coefficients"):
        ops.jpeg_block_bits(coefs.int())
    with pytest.raises(RuntimeError, match="STV_ERR_ARG"):
        ops.jpeg_block_bits(coefs[:, :17].contiguous())         # 17 blocks: no whole MCUs
    bits = ops.jpeg_block_bits(coefs)
    with pytest.raises(RuntimeError, match="offsets"):
        ops.jpeg_scan(bits, offsets=torch.empty(3, 17, dtype=torch.int32, device=DEV))
    offsets, _ = ops.jpeg_scan(bits)
    with pytest.raises(RuntimeError, match="STV_ERR_ARG"):
        ops.jpeg_emit(coefs, offsets, torch.zeros(3, dtype=torch.int32, device=DEV), torch.zeros(1022, dtype=torch.uint8, device=DEV))
