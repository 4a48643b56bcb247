"""What the style is made of: several style images mixed with blend weights, and a weight per style layer.

Both act on the style *targets* and on per-tap coefficients; the step keeps its op list and its kernels.

* Blend (jcjohnson/neural-style's ``-style_image a,b -style_blend_weights 7,3``): each of the ``K`` <= ``MAX_STYLES`` images is
  captured as a single one is, and per style layer the target is ``(...((b_0*G_0) + b_1*G_1) + ...) + b_{K-1}*G_{K-1}``, formed
  by one ``ops.gram_blend`` launch with every product and sum rounded to fp32 on its own.  The weights are normalised to sum 1
  in float64 and rounded to fp32 once (:func:`blend_weights`).
* Layer weights (Gatys' ``w_l``): the style score is ``sum_l w_l * loss_l``; for tap ``l`` the combine table's scale is
  ``w_l / (C*C)`` and the seed coefficient ``style_w * w_l`` (:func:`tap_weights` pairs the weights with the sorted taps).

Everything here is host arithmetic and refusals; nothing launches.
"""
from __future__ import annotations

import math
from collections.abc import Sequence

import numpy as np

from ._lib import BLEND_MAX_TABLES as MAX_STYLES


def _finite_nonneg(values: Sequence[float], what: str) -> list[float]:
    try:
        out = [float(v) for v in values]
    except (TypeError, ValueError):
        msg = f"{what} must be a list of numbers, got {values!r}"
        raise ValueError(msg) from None
    for v in out:
        if not math.isfinite(v) or v < 0:
            msg = f"{what} must be finite and >= 0, got {out}"
            raise ValueError(msg)
    return out


def blend_weights(raw: Sequence[float] | None, k: int) -> np.ndarray:
    """The ``k`` blend weights as fp32: ``raw`` normalised to sum 1 in float64, each rounded to fp32 once; ``None`` gives
    ``k`` equal weights.  ``ValueError``, naming the values: ``k`` outside 1..``MAX_STYLES``, a length other than ``k``, a
    weight that is negative or not finite, no weight above 0."""
    k = int(k)
    if not 1 <= k <= MAX_STYLES:
        msg = f"between 1 and {MAX_STYLES} style images can be blended, got {k}"
        raise ValueError(msg)
    if raw is None:
        return np.full(k, np.float64(1.0) / np.float64(k), dtype=np.float64).astype(np.float32)
    values = _finite_nonneg(raw, "style_blend weights")
    if len(values) != k:
        msg = f"style_blend has {len(values)} weights {values} for {k} style image{'s' if k != 1 else ''}"
        raise ValueError(msg)
    total = math.fsum(values)
    if not total > 0 or not math.isfinite(total):
        msg = f"style_blend needs at least one weight above 0 (and a finite sum), got {values}"
        raise ValueError(msg)
    return (np.asarray(values, dtype=np.float64) / np.float64(total)).astype(np.float32)


def check_layer_weights(weights: Sequence[float] | None, style_layers: Sequence[int]) -> tuple[float, ...] | None:
    """``weights`` as a tuple of floats paired by position with ``style_layers`` as given, or ``None``.  ``ValueError``,
    naming the values: a length other than ``len(style_layers)`` (both lengths named), a weight that is negative or not
    finite, duplicate entries in ``style_layers``."""
    if weights is None:
        return None
    values = _finite_nonneg(weights, "style_layer_weights")
    layers = [int(v) for v in style_layers]
    if len(values) != len(layers):
        msg = f"style_layer_weights has {len(values)} weights {values} for {len(layers)} style layers {layers}"
        raise ValueError(msg)
    if len(set(layers)) != len(layers):
        msg = f"style_layer_weights cannot be paired with style_layers that hold duplicates: {layers}"
        raise ValueError(msg)
    return tuple(values)


def tap_weights(weights: Sequence[float] | None, style_layers: Sequence[int]) -> tuple[float, ...] | None:
    """The layer weights in the order of the model's style taps (``style_layers`` sorted), or ``None`` when there are none
    or every one is exactly 1.0: the step is then the one without weights, under the same program key."""
    values = check_layer_weights(weights, style_layers)
    if values is None or all(v == 1.0 for v in values):
        return None
    by_layer = dict(zip((int(v) for v in style_layers), values, strict=True))
    return tuple(by_layer[layer] for layer in sorted(by_layer))


def is_trivial(weights: Sequence[float] | None) -> bool:
    """No layer weights, or all exactly 1.0."""
    return weights is None or all(float(v) == 1.0 for v in weights)


def option_kwargs(optimization, name: str) -> dict:
    """``{name: value}`` for a style-mix option (``style_blend``, ``style_layer_weights``) that is set on the optimisation
    settings, ``{}`` otherwise: the calls of a run without them stay as they were (stand-ins for the model take no such
    keyword)."""
    value = getattr(optimization, name, None)
    return {} if value is None else {name: list(value)}
