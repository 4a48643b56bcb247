"""NumPy twins of ``stv_gram_blend`` (style_transfer_visualizer_amd/csrc/blend.hip).

``blend``: the kernel's arithmetic in fp32 - every product and every sum rounded by ``np.float32`` on its own, tables in
ascending order, the first product starts the sum - so a device result can be compared with ``torch.equal``.
``blend_f64``: the same sum in float64 from the fp32 operands, for the host tests; the twin is within ``K`` roundings of it:
``K`` products and ``K - 1`` sums round once each, and every rounding is relative to a partial sum of magnitude at most
``sum_k |w_k G_k|``, so ``|twin - exact| <= (2K - 1) u sum_k |w_k G_k|`` to first order, u = 2^-24.
"""
from __future__ import annotations

import numpy as np


def blend(stack: np.ndarray, weights) -> np.ndarray:
    """fp32 ``(...((w0*G0) + w1*G1) + ...)`` of ``stack`` ``[K, ...]``, one rounding per operation."""
    stack = np.asarray(stack, dtype=np.float32)
    w = np.asarray(weights, dtype=np.float32)
    assert stack.shape[0] == w.shape[0] >= 1
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        acc = np.multiply(w[0], stack[0], dtype=np.float32)
        for k in range(1, stack.shape[0]):
            p = np.multiply(w[k], stack[k], dtype=np.float32)
            acc = np.add(acc, p, dtype=np.float32)
    return acc


def blend_f64(stack: np.ndarray, weights) -> np.ndarray:
    """The same sum in float64 from the fp32 operands."""
    stack = np.asarray(stack, dtype=np.float32).astype(np.float64)
    w = np.asarray(weights, dtype=np.float32).astype(np.float64)
    return np.tensordot(w, stack, axes=(0, 0))


def magnitude(stack: np.ndarray, weights) -> np.ndarray:
    """``sum_k |w_k G_k|`` in float64: what the roundings of the twin are relative to."""
    stack = np.abs(np.asarray(stack, dtype=np.float32).astype(np.float64))
    w = np.abs(np.asarray(weights, dtype=np.float32).astype(np.float64))
    return np.tensordot(w, stack, axes=(0, 0))
