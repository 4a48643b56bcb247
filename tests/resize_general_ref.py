"""NumPy fp32 twin of ``ops.resize`` (``stv_resize_axis``), written from the definition, not from the package or the kernel.

Tables, float64, for ``n_in -> n_out`` with a filter ``f`` of support ``S``:

    scale = n_in / n_out;  fs = max(scale, 1);  support = S * fs
    output i:  c = (i + 0.5) * scale;  start = max(int(c - support + 0.5), 0);  end = min(int(c + support + 0.5), n_in)
               w_k = f((start + k - c + 0.5) / fs) for k < end - start;  w_k /= (w_0 + w_1 + ...) summed left to right;
               each w_k rounded to fp32

Resampling, fp32, every product and every sum one NumPy float32 operation (no fused multiply-add), taps in ascending order:

    acc = 0;  for k = 0 .. count-1:  acc = acc + (w[k] * x[start + k])

columns first (``[C, H, W] -> [C, H, Wo]``), rows second; an axis that keeps its size is not filtered at all.
"""
from __future__ import annotations

import math

import numpy as np

from tests.resize_ref import pattern, randn3  # noqa: F401  (re-exported for the tests of the general resize)

F32 = np.float32
SUPPORT = {"bilinear": 1.0, "bicubic": 2.0, "lanczos": 3.0}
FILTER_NAMES = tuple(SUPPORT)


def weight(name: str, t: float) -> float:
    """The filter ``name`` at ``t``, float64."""
    t = math.fabs(t)
    if name == "bilinear":
        return max(1.0 - t, 0.0)
    if name == "bicubic":                       # Keys, a = -0.5
        if t < 1.0:
            return (1.5 * t - 2.5) * t * t + 1.0
        if t < 2.0:
            return -0.5 * (((t - 5.0) * t + 8.0) * t - 4.0)
        return 0.0
    if name == "lanczos":                       # sinc(t) * sinc(t / 3) inside (-3, 3)
        if t >= 3.0:
            return 0.0
        if t == 0.0:
            return 1.0
        a, b = math.pi * t, math.pi * (t / 3.0)
        return (math.sin(a) / a) * (math.sin(b) / b)
    raise KeyError(name)


def table(n_in: int, n_out: int, name: str) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(start int32 [n_out], count int32 [n_out], weights fp32 [n_out, K])``, rows zero-padded to the longest."""
    scale = n_in / n_out
    fs = scale if scale > 1.0 else 1.0
    support = SUPPORT[name] * fs
    start = np.zeros(n_out, dtype=np.int32)
    count = np.zeros(n_out, dtype=np.int32)
    rows = []
    for i in range(n_out):
        c = (i + 0.5) * scale
        lo = max(int(c - support + 0.5), 0)
        hi = min(int(c + support + 0.5), n_in)
        raw = [weight(name, (lo + k - c + 0.5) / fs) for k in range(hi - lo)]
        s = 0.0
        for v in raw:
            s = s + v
        rows.append([F32(v / s) for v in raw])
        start[i], count[i] = lo, hi - lo
    weights = np.zeros((n_out, int(count.max())), dtype=F32)
    for i, r in enumerate(rows):
        weights[i, :len(r)] = r
    return start, count, weights


def filter_last_axis(a: np.ndarray, n_out: int, name: str) -> np.ndarray:
    """``a [..., n_in] -> [..., n_out]``: the sequential fp32 accumulation along the last axis."""
    start, count, weights = table(a.shape[-1], n_out, name)
    out = np.empty((*a.shape[:-1], n_out), dtype=F32)
    for i in range(n_out):
        acc = np.zeros(a.shape[:-1], dtype=F32)
        for k in range(int(count[i])):
            acc = acc + weights[i, k] * a[..., int(start[i]) + k]
        assert acc.dtype == F32
        out[..., i] = acc
    return out


def resize(x, size: tuple[int, int], name: str = "lanczos") -> np.ndarray:
    """An image ``[..., C, H, W]`` at ``size = (Ho, Wo)``; fp32, same rank.  Same size: the input itself."""
    a = np.asarray(x, dtype=F32)
    H, W = a.shape[-2:]
    Ho, Wo = (int(v) for v in size)
    if (Ho, Wo) == (H, W):
        return a
    if Wo != W:
        a = filter_last_axis(a, Wo, name)
    if Ho != H:
        a = np.swapaxes(filter_last_axis(np.swapaxes(a, -1, -2), Ho, name), -1, -2)
    return np.ascontiguousarray(a)
