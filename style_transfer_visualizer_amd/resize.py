"""Input resizing (``optimization.content_size`` / ``style_size`` / ``style_scale``): the host side of ``ops.resize``.

Two things live here, both pure host arithmetic that needs no device:

*Coefficient tables.*  ``ops.resize`` is a separable, antialiased resampler (``stv_resize_axis``, one launch per axis):
output index ``i`` along an axis is ``sum_k weights[i][k] * x[start[i] + k]`` over ``count[i]`` taps.
:func:`axis_table` builds ``start``, ``count`` and ``weights`` for ``n_in -> n_out`` and one of three filters - ``bilinear``
(triangle, support 1), ``bicubic`` (Keys cubic with a = -0.5, support 2), ``lanczos`` (sinc windowed by sinc, a = 3) -
stretched by the scale factor on a downscale, which is what PIL's ``Image.resize`` and torch's ``antialias=True`` do.  All
table arithmetic is float64 in plain Python (``math.sin``; sums taken left to right); each weight is rounded to fp32 once,
at the end.

*Size rules.*  :func:`target_size` scales an image so that its longer side becomes a given length, in exact integer
arithmetic; :func:`plan_sizes` turns the three settings into the sizes ``main.style_transfer`` resizes to, and refuses what
cannot run before anything touches the device.

Not built: row strips (``spatial.py``), arbitrary ratios between the levels of a coarse-to-fine run (``pyramid.py`` keeps
its factor of two), and per-axis target sizes (the aspect ratio is kept up to the rounding of a side).
"""
from __future__ import annotations

import functools
import math

import numpy as np

from .constants import MIN_DIMENSION


def _triangle(x: float) -> float:
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _keys_cubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:                     # noqa: PLR2004
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x *= math.pi
    return math.sin(x) / x


def _lanczos3(x: float) -> float:
    x = abs(x)
    if x < 3.0:                     # noqa: PLR2004
        return _sinc(x) * _sinc(x / 3.0)
    return 0.0


# name -> (kernel, support)
FILTERS = {"bilinear": (_triangle, 1.0), "bicubic": (_keys_cubic, 2.0), "lanczos": (_lanczos3, 3.0)}


@functools.lru_cache(maxsize=64)
def axis_table(n_in: int, n_out: int, filter: str = "lanczos") -> tuple[np.ndarray, np.ndarray, np.ndarray]:  # noqa: A002
    """``(start int32 [n_out], count int32 [n_out], weights fp32 [n_out, K])`` of ``n_in -> n_out`` samples; ``K`` is the
    largest ``count``, rows are padded with zeros (never read), ``start + count <= n_in``, and every row of weights sums to
    one before the rounding to fp32.  The arrays are cached and read-only."""
    if filter not in FILTERS:
        msg = f"unknown resize filter {filter!r}: expected one of {sorted(FILTERS)}"
        raise ValueError(msg)
    if n_in < 1 or n_out < 1:
        msg = f"resize needs positive sizes, got {n_in} -> {n_out}"
        raise ValueError(msg)
    kernel, radius = FILTERS[filter]
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = radius * fs
    starts, rows = [], []
    for i in range(n_out):
        c = (i + 0.5) * scale
        first = max(int(c - support + 0.5), 0)
        last = min(int(c + support + 0.5), n_in)
        w = [kernel((first + k - c + 0.5) / fs) for k in range(last - first)]
        total = 0.0
        for v in w:
            total += v
        starts.append(first)
        rows.append([v / total for v in w])
    start = np.asarray(starts, dtype=np.int32)
    count = np.asarray([len(w) for w in rows], dtype=np.int32)
    weights = np.zeros((n_out, int(count.max())), dtype=np.float32)
    for i, w in enumerate(rows):
        weights[i, :len(w)] = np.asarray(w, dtype=np.float64).astype(np.float32)
    for a in (start, count, weights):
        a.setflags(write=False)
    return start, count, weights


def target_size(h: int, w: int, longer: int, multiple: int = 1) -> tuple[int, int]:
    """``(h, w)`` scaled so that the longer side becomes ``longer``: each side is rounded to the nearest multiple of
    ``multiple`` (ties up) and is at least ``multiple``.  Exact integer arithmetic."""
    h, w, longer, multiple = int(h), int(w), int(longer), int(multiple)
    if min(h, w, longer, multiple) < 1:
        msg = f"target_size needs positive numbers, got {h}x{w} -> {longer} in multiples of {multiple}"
        raise ValueError(msg)
    big = max(h, w)

    def side(s: int) -> int:
        return multiple * max(1, (2 * s * longer + big * multiple) // (2 * big * multiple))
    return side(h), side(w)


def _refuse_small(what: str, setting: str, src: tuple[int, int], dst: tuple[int, int]) -> None:
    if min(dst) < MIN_DIMENSION:
        msg = (f"{setting} resizes the {what} image from {src[1]}x{src[0]} to {dst[1]}x{dst[0]}; "
               f"the minimum dimension is {MIN_DIMENSION}")
        raise ValueError(msg)


def plan_sizes(optimization_config, content_hw, style_hw) -> tuple[tuple[int, int] | None, tuple[int, int] | None]:
    """``(content target, style target)`` as ``(H, W)``, ``None`` for an image that keeps its size.

    ``content_size = N``: the content's longer side becomes N, both sides multiples of ``2**(pyramid_levels-1)`` so that a
    coarse-to-fine run accepts them.  ``style_size = N``: the style's longer side becomes N.  ``style_scale = f``: it becomes
    ``round(f * longer side of the content as the run will see it)``.  ``ValueError``, naming the values, for ``style_size``
    together with ``style_scale`` and for a target with a side below ``MIN_DIMENSION``."""
    oc = optimization_config
    content_hw = (int(content_hw[0]), int(content_hw[1]))
    style_hw = (int(style_hw[0]), int(style_hw[1]))
    if oc.style_size > 0 and oc.style_scale > 0:
        msg = (f"style_size = {oc.style_size} and style_scale = {oc.style_scale:g} both set the style image's size: "
               "give one of them")
        raise ValueError(msg)
    content_to = content_hw
    if oc.content_size > 0:
        content_to = target_size(*content_hw, oc.content_size, 1 << (int(oc.pyramid_levels) - 1))
        _refuse_small("content", f"content_size = {oc.content_size}", content_hw, content_to)
    style_to = style_hw
    if oc.style_size > 0:
        style_to = target_size(*style_hw, oc.style_size, 1)
        _refuse_small("style", f"style_size = {oc.style_size}", style_hw, style_to)
    elif oc.style_scale > 0:
        longer = max(1, round(oc.style_scale * max(content_to)))
        style_to = target_size(*style_hw, longer, 1)
        _refuse_small("style", f"style_scale = {oc.style_scale:g} (longer side {longer})", style_hw, style_to)
    return (content_to if content_to != content_hw else None, style_to if style_to != style_hw else None)
