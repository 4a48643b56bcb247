"""Timelapse GIF output (``--gif``; no counterpart in the reference, whose GIF path encodes host frames with imageio).

Frames are captured on the device into a store allocated before the run - ``ops.image_to_u8`` writes the frame conversion of
the reference straight into the next slot, ``ops.frame_hist`` adds the slot to one colour histogram - so a saved frame costs
two launches and no host synchronisation.  When the run is over, ONE palette for all frames is cut from that histogram on the
host (``median_cut``: one colour table, no palette flicker), ``ops.gif_map`` maps every frame to palette indices with an
ordered dither, the index planes cross to the host in one copy, and only the LZW container is left to PIL.

Definitions, to the bit, are in ``include/stv.h``; ``tests/gif_ref.py`` holds NumPy twins of the two kernels.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from . import _lib
from .constants import IMAGENET_MEAN, IMAGENET_STD
from .logging_utils import logger

GIF_MAX_DEVICE_BYTES = 4 << 30      # frame store + index planes: 4 bytes per pixel and frame
# `--gif-dither ordered`: the Bayer offsets span -8..7, one histogram cell (8 levels) - the width of the quantisation step
# the palette is cut on.  A design choice, not derived: wider spreads trade banding for visible texture.
ORDERED_SPREAD = 16
DITHER_SPREAD = {"none": 0, "ordered": ORDERED_SPREAD}
MIN_COLORS, MAX_COLORS = 2, 256
_SIDE = 32                          # histogram cells per channel: bin = (r>>3)<<10 | (g>>3)<<5 | (b>>3)


def bayer8() -> np.ndarray:
    """The 8x8 Bayer matrix ``B8[y][x]`` of ``stv_gif_map``, a permutation of 0..63: the bits of ``x ^ y`` and of ``y``
    interleaved, the lowest bit of each pair on top."""
    y, x = np.mgrid[0:8, 0:8]
    t = np.zeros((8, 8), dtype=np.int64)
    for b in range(3):
        t |= (((x >> b) & 1) ^ ((y >> b) & 1)) << (2 * (2 - b) + 1)
        t |= ((y >> b) & 1) << (2 * (2 - b))
    return t


def frame_duration_cs(fps: int) -> int:
    """The GIF frame delay in centiseconds: the nearest to ``100 / fps``, never under 2 (viewers treat 0 and 1 as 10)."""
    fps = int(fps)
    if fps < 1:
        msg = f"fps must be at least 1, got {fps}"
        raise ValueError(msg)
    return max(2, (200 + fps) // (2 * fps))


class _Box:
    """An axis-aligned box of histogram cells with tight inclusive bounds."""

    __slots__ = ("hi", "lo", "pop")

    def __init__(self, h3: np.ndarray, lo: list[int], hi: list[int]) -> None:
        sub = h3[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1]
        self.lo, self.hi = [0, 0, 0], [0, 0, 0]
        for axis in range(3):
            occupied = np.nonzero(sub.sum(axis=tuple(a for a in range(3) if a != axis)))[0]
            self.lo[axis], self.hi[axis] = lo[axis] + int(occupied[0]), lo[axis] + int(occupied[-1])
        self.pop = int(sub.sum())

    def cells(self, h3: np.ndarray) -> np.ndarray:
        return h3[self.lo[0]:self.hi[0] + 1, self.lo[1]:self.hi[1] + 1, self.lo[2]:self.hi[2] + 1]

    def extents(self) -> list[int]:
        return [h - l for l, h in zip(self.lo, self.hi, strict=True)]


def median_cut(hist: np.ndarray, n_colors: int) -> np.ndarray:
    """A palette of at most ``n_colors`` entries, uint8 ``[n, 3]``, from the ``32*32*32`` colour histogram (any integer
    dtype, read as counts).  Deterministic, integers only:

    * boxes of cells carry tight bounds; the box with the largest ``population * longest extent`` is split (the lowest
      index wins a tie), along its longest axis (ties: r, then g, then b), at the population median, clamped so that both
      halves hold pixels; the lower half keeps the box's place, the upper half goes to the end of the list;
    * it stops at ``n_colors`` boxes or when no box has an extent left - an image with at most ``n_colors`` occupied cells
      gets one entry per cell;
    * an entry is the population-weighted mean of the cell centres ``8*c + 4`` per channel, rounded to nearest:
      ``(2*S + n) // (2*n)``; entries stay in the order the boxes were made.
    """
    n_colors = int(n_colors)
    if not 1 <= n_colors <= MAX_COLORS:
        msg = f"median_cut takes 1 to {MAX_COLORS} colours, got {n_colors}"
        raise ValueError(msg)
    h3 = np.asarray(hist)
    if h3.size != _SIDE ** 3:
        msg = f"median_cut expects a histogram of {_SIDE ** 3} bins, got {h3.size}"
        raise ValueError(msg)
    h3 = h3.astype(np.int64).reshape(_SIDE, _SIDE, _SIDE)
    if int(h3.sum()) <= 0 or int(h3.min()) < 0:
        msg = "median_cut: the histogram is empty (no frame was counted)"
        raise ValueError(msg)
    boxes = [_Box(h3, [0, 0, 0], [_SIDE - 1] * 3)]
    while len(boxes) < n_colors:
        scores = [box.pop * max(box.extents()) for box in boxes]
        best = max(scores)
        if best == 0:
            break
        at = scores.index(best)                     # the lowest index wins a tie
        box = boxes[at]
        ext = box.extents()
        axis = ext.index(max(ext))                  # ties: r, g, b
        along = box.cells(h3).sum(axis=tuple(a for a in range(3) if a != axis))
        cum = np.cumsum(along)
        cut = int(np.searchsorted(2 * cum, box.pop, side="left"))      # the first cell at which half the pixels are reached
        cut = min(cut, ext[axis] - 1)               # both halves non-empty: the bounds are tight, so the end cells hold pixels
        lo_hi, hi_lo = list(box.hi), list(box.lo)
        lo_hi[axis] = box.lo[axis] + cut
        hi_lo[axis] = box.lo[axis] + cut + 1
        boxes[at] = _Box(h3, box.lo, lo_hi)
        boxes.append(_Box(h3, hi_lo, box.hi))
    palette = np.zeros((len(boxes), 3), dtype=np.uint8)
    for k, box in enumerate(boxes):
        cells = box.cells(h3)
        for axis in range(3):
            along = cells.sum(axis=tuple(a for a in range(3) if a != axis))
            centres = 8 * np.arange(box.lo[axis], box.hi[axis] + 1, dtype=np.int64) + 4
            total = int((along * centres).sum())
            palette[k, axis] = (2 * total + box.pop) // (2 * box.pop)
    return palette


def check_colors(colors: int) -> int:
    colors = int(colors)
    if not MIN_COLORS <= colors <= MAX_COLORS:
        msg = f"gif_colors must be between {MIN_COLORS} and {MAX_COLORS}, got {colors}"
        raise ValueError(msg)
    return colors


def dither_spread(dither: str) -> int:
    if dither not in DITHER_SPREAD:
        msg = f"gif_dither must be one of {sorted(DITHER_SPREAD)}, got {dither!r}"
        raise ValueError(msg)
    return DITHER_SPREAD[dither]


def store_bytes(n_frames: int, H: int, W: int) -> int:
    """Device bytes of the frame store and the index planes of ``n_frames`` frames of ``H x W`` pixels."""
    return int(n_frames) * int(H) * int(W) * 4


def check_budget(n_frames: int, H: int, W: int) -> int:
    """Refuse a timelapse whose frames do not fit ``GIF_MAX_DEVICE_BYTES`` (spilling to the host is not built)."""
    need = store_bytes(n_frames, H, W)
    if need > GIF_MAX_DEVICE_BYTES:
        msg = (f"the GIF timelapse keeps its frames on the device: {n_frames} frames of {W}x{H} pixels need {need} bytes, over the "
               f"budget of {GIF_MAX_DEVICE_BYTES} bytes; save fewer frames with a larger --save-every")
        raise ValueError(msg)
    return need


class DeviceGifCollector:
    """A ``FrameSink`` that keeps its frames on the device and writes one GIF with one global palette on ``close()``.

    Everything is allocated here: ``[n_frames, H, W, 3]`` uint8 frames, ``[n_frames, H, W]`` uint8 indices, the histogram.
    ``append_device`` enqueues two launches on the current stream and returns: no synchronisation, no device allocation, no
    host read.  ``close()`` reads the histogram back, cuts the palette, maps the frames and hands the indices to PIL."""

    def __init__(self, path: str | Path, fps: int, H: int, W: int, n_frames: int, *, colors: int = MAX_COLORS,  # noqa: PLR0913
                 dither: str = "ordered", device: torch.device | str = "cuda") -> None:
        self.path = Path(path)
        self.H, self.W, self.n_frames = int(H), int(W), int(n_frames)
        if self.H < 1 or self.W < 1 or self.n_frames < 0:
            msg = f"DeviceGifCollector: {self.n_frames} frames of {self.W}x{self.H} pixels"
            raise ValueError(msg)
        self.colors = check_colors(colors)
        self.spread = dither_spread(dither)
        self.duration_cs = frame_duration_cs(fps)
        check_budget(self.n_frames, self.H, self.W)             # before anything is allocated or launched
        self.device = torch.device(device)
        if self.device.type != "cuda":
            msg = f"DeviceGifCollector keeps its frames on a GPU, got device {self.device}"
            raise RuntimeError(msg)
        self.count = 0
        self.closed = False
        self.timings: dict[str, float] = {}
        self.palette: np.ndarray | None = None      # the palette of the written file, after close()
        self._frames = self._index = self._hist = None
        if self.n_frames:
            self._frames = torch.empty(self.n_frames, self.H, self.W, 3, dtype=torch.uint8, device=self.device)
            self._index = torch.empty(self.n_frames, self.H, self.W, dtype=torch.uint8, device=self.device)
            self._hist = torch.zeros(_lib.GIF_HIST_BINS, dtype=torch.int32, device=self.device)

    def _next_slot(self) -> torch.Tensor:
        if self.closed:
            msg = "DeviceGifCollector: a frame appended after close()"
            raise RuntimeError(msg)
        if self.count >= self.n_frames:
            msg = f"DeviceGifCollector: frame {self.count + 1} appended to a store of {self.n_frames} frames"
            raise RuntimeError(msg)
        return self._frames[self.count]

    def append_device(self, image: torch.Tensor, *, normalize: bool) -> None:
        """Capture the image being optimised (fp32 ``[1, 3, H, W]`` or ``[3, H, W]`` on the device) as the next frame."""
        from . import ops  # noqa: PLC0415
        if tuple(image.shape[-2:]) != (self.H, self.W):
            msg = f"DeviceGifCollector: a frame of {tuple(image.shape[-2:])} for a store of {(self.H, self.W)}"
            raise RuntimeError(msg)
        slot = self._next_slot()
        ops.image_to_u8(image, mean=IMAGENET_MEAN if normalize else None, std=IMAGENET_STD if normalize else None,
                        rounding=False, out=slot)
        ops.frame_hist(slot, self._hist)
        self.count += 1

    def append_data(self, frame: np.ndarray) -> None:
        """The ``FrameSink`` protocol: a host frame, uint8 ``[H, W, 3]``, is uploaded into the next slot."""
        from . import ops  # noqa: PLC0415
        arr = np.ascontiguousarray(frame)
        if arr.dtype != np.uint8 or arr.shape != (self.H, self.W, 3):
            msg = f"DeviceGifCollector: a host frame of {arr.shape} {arr.dtype} for a store of {(self.H, self.W, 3)} uint8"
            raise RuntimeError(msg)
        slot = self._next_slot()
        slot.copy_(torch.from_numpy(arr))
        ops.frame_hist(slot, self._hist)
        self.count += 1

    def close(self) -> None:
        """Write the file (once; further calls do nothing) and free the store."""
        if self.closed:
            return
        self.closed = True
        try:
            if self.count == 0:
                logger.info("GIF timelapse: no frame was saved, %s is not written", self.path)
                return
            self._encode()
        finally:
            self._frames = self._index = self._hist = None

    def _encode(self) -> None:
        import time  # noqa: PLC0415

        from PIL import Image  # noqa: PLC0415

        from . import ops  # noqa: PLC0415
        clock = time.perf_counter
        t0 = clock()
        hist = self._hist.cpu().numpy().view(np.uint32)
        t1 = clock()
        palette = median_cut(hist, self.colors)
        t2 = clock()
        palette_dev = torch.from_numpy(palette).to(self.device)
        for i in range(self.count):
            ops.gif_map(self._frames[i], palette_dev, self.spread, out=self._index[i])
        torch.cuda.synchronize(self.device)
        t3 = clock()
        planes = self._index[:self.count].cpu().numpy()
        t4 = clock()
        flat = palette.reshape(-1).tolist()
        images = []
        for i in range(self.count):
            img = Image.fromarray(planes[i], "P")
            img.putpalette(flat)
            images.append(img)
        self.path.parent.mkdir(parents=True, exist_ok=True)
        images[0].save(str(self.path), format="GIF", save_all=True, append_images=images[1:],
                       duration=10 * self.duration_cs, loop=0, optimize=False)
        t5 = clock()
        self.palette = palette
        self.timings = {"readback_s": t1 - t0, "median_cut_s": t2 - t1, "map_s": t3 - t2, "copy_s": t4 - t3, "encode_s": t5 - t4}
        logger.info("GIF timelapse: %d frames, %d colours, %d ms per frame", self.count, len(palette), 10 * self.duration_cs)
