"""NumPy twins of the two GIF kernels (include/stv.h, "Timelapse GIF output"): integer arithmetic, the same to the bit.

Written from the definitions, not from the kernels: the Bayer matrix is built by sorting out the recursive construction
(``B_2n = [[4B, 4B+2], [4B+3, 4B+1]]``), not by the bit formula the kernel and ``gif.bayer8`` use."""
from __future__ import annotations

import numpy as np

HIST_BINS = 32768


def bayer8_recursive() -> np.ndarray:
    """The classic 8x8 ordered-dither matrix by recursion from ``[[0, 2], [3, 1]]``."""
    b = np.array([[0, 2], [3, 1]], dtype=np.int64)
    while b.shape[0] < 8:
        b = np.block([[4 * b, 4 * b + 2], [4 * b + 3, 4 * b + 1]])
    return b


def frame_hist(frame: np.ndarray, hist: np.ndarray | None = None) -> np.ndarray:
    """``hist[(r>>3)<<10 | (g>>3)<<5 | (b>>3)] += 1`` for every pixel of a uint8 ``[H, W, 3]`` frame; int64 counts."""
    px = frame.reshape(-1, 3).astype(np.int64)
    bins = ((px[:, 0] >> 3) << 10) | ((px[:, 1] >> 3) << 5) | (px[:, 2] >> 3)
    counts = np.bincount(bins, minlength=HIST_BINS).astype(np.int64)
    return counts if hist is None else hist.astype(np.int64) + counts


def dithered(frame: np.ndarray, spread: int) -> np.ndarray:
    """``clamp(frame + ((2*B8[y&7][x&7] - 63) * spread >> 7), 0, 255)``, the same offset for the three channels; int64."""
    H, W = frame.shape[:2]
    y, x = np.mgrid[0:H, 0:W]
    t = bayer8_recursive()[y & 7, x & 7]
    off = ((2 * t - 63) * int(spread)) >> 7                     # numpy's >> on negative ints is arithmetic: floor
    return np.clip(frame.astype(np.int64) + off[:, :, None], 0, 255)


def gif_map(frame: np.ndarray, palette: np.ndarray, spread: int) -> np.ndarray:
    """The index of the nearest palette entry per pixel (squared distance in integers, the lowest index wins a tie: what
    ``np.argmin`` returns) after the ordered dither; uint8 ``[H, W]``."""
    v = dithered(frame, spread).reshape(-1, 1, 3)
    pal = palette.astype(np.int64).reshape(1, -1, 3)
    out = np.empty(v.shape[0], dtype=np.uint8)
    for at in range(0, v.shape[0], 4096):                       # [4096, n, 3] blocks: bounded memory
        d = ((v[at:at + 4096] - pal) ** 2).sum(axis=2)
        out[at:at + 4096] = np.argmin(d, axis=1)
    return out.reshape(frame.shape[:2])
