"""NumPy twins of the automatic-mask kernels (``segment.py``): ``stv_kmeans_assign`` with the fp32 arithmetic of stv.h written
product by product, the box pooling and the raw colour moments - and adapters with the signatures ``segment.auto_labels``
takes as ``assign=`` / ``pool=`` / ``moments=``, so that the whole algorithm runs on the host."""
from __future__ import annotations

import numpy as np
import torch

from style_transfer_visualizer_amd import _lib

F32 = np.float32


def assign(x, centroids, prev):
    """``labels [H, W] uint8, sums [K, 3] float64, counts [K] float64, changed`` for ``x`` fp32 ``[3, H, W]``, ``centroids`` fp32
    ``[K, 3]`` and the previous labels ``prev`` uint8 ``[H, W]``.  ``d_k = ((e0*e0 + e1*e1) + e2*e2)`` with every difference,
    product and sum an fp32 operation of its own; the label is the first ``k`` in ascending order with ``d_k <`` the best so
    far, which starts at +inf - an explicit strict ``<`` (not ``np.argmin``, whose NaN and tie rules are its own)."""
    x = np.asarray(x, dtype=F32)
    c = np.asarray(centroids, dtype=F32)
    prev = np.asarray(prev, dtype=np.uint8)
    K = c.shape[0]
    best = np.full(x.shape[1:], np.inf, dtype=F32)
    labels = np.zeros(x.shape[1:], dtype=np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            e0, e1, e2 = (x[j] - c[k, j] for j in range(3))              # fp32 - fp32 -> fp32
            q0, q1, q2 = e0 * e0, e1 * e1, e2 * e2
            s01 = q0 + q1
            d = s01 + q2
            assert d.dtype == F32
            wins = d < best
            best = np.where(wins, d, best)
            labels = np.where(wins, np.uint8(k), labels)
    sums = np.zeros((K, 3), dtype=np.float64)
    counts = np.zeros(K, dtype=np.float64)
    for k in range(K):
        mine = labels == k
        counts[k] = float(mine.sum())
        for j in range(3):
            sums[k, j] = x[j][mine].astype(np.float64).sum()
    return labels, sums, counts, int((labels != prev).sum())


def parts_row(sums, counts, changed) -> np.ndarray:
    """One row of ``parts`` holding the totals (what the 256 rows of the kernel add up to)."""
    row = np.zeros(_lib.KMEANS_PART_DOUBLES, dtype=np.float64)
    for k in range(len(counts)):
        row[4 * k:4 * k + 3] = sums[k]
        row[4 * k + 3] = counts[k]
    row[-1] = changed
    return row


def assign_op(x: torch.Tensor, centroids: torch.Tensor, labels: torch.Tensor, parts: torch.Tensor | None = None) -> torch.Tensor:
    """:func:`assign` behind the signature of ``ops.kmeans_assign``, for tensors on any device: ``labels`` in place, the totals
    in row 0 of ``parts`` and zeros in the others."""
    img = x.detach().cpu().numpy().reshape(3, x.shape[-2], x.shape[-1])
    new, sums, counts, changed = assign(img, centroids.detach().cpu().numpy(), labels.cpu().numpy())
    labels.copy_(torch.from_numpy(new))
    if parts is None:
        parts = torch.empty(_lib.KMEANS_PARTS, _lib.KMEANS_PART_DOUBLES, dtype=torch.float64, device=x.device)
    host = np.zeros(tuple(parts.shape), dtype=np.float64)
    host[0] = parts_row(sums, counts, changed)
    parts.copy_(torch.from_numpy(host))
    return parts


def pool_op(img: torch.Tensor, cell: int) -> torch.Tensor:
    """The ``cell x cell`` box means of a host image as fp32 ``[3, H//cell, W//cell]`` (float64 means, rounded once)."""
    x = img.detach().cpu().numpy().reshape(3, img.shape[-2], img.shape[-1]).astype(np.float64)
    h, w = x.shape[1] // cell, x.shape[2] // cell
    cells = x[:, :h * cell, :w * cell].reshape(3, h, cell, w, cell).mean(axis=(2, 4))
    return torch.from_numpy(cells.astype(F32))


def moments_op(img: torch.Tensor):
    """``color.statistics`` of a host image: ``(n, sums[3], moments[3, 3])`` in float64."""
    x = img.detach().cpu().numpy().reshape(3, -1).astype(np.float64)
    return x.shape[1], x.sum(axis=1), x @ x.T


HOST = {"assign": assign_op, "pool": pool_op, "moments": moments_op}
