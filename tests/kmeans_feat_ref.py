"""NumPy twins of the feature-space k-means kernels (``csrc/kmeans_feat.hip``, ``segment.feature_labels``):
``stv_kmeans_feat_assign`` with the fp32 distance and the double sums in the order stv.h fixes, ``stv_kmeans_feat_update`` in
float64 - and adapters with the signatures of ``ops.kmeans_feat_assign`` / ``ops.kmeans_feat_update`` and of
``segment.feature_moments``, so that the whole algorithm runs on the host."""
from __future__ import annotations

import numpy as np
import torch

from style_transfer_visualizer_amd import _lib

F32 = np.float32
F64 = np.float64


def distances(x, centroids) -> np.ndarray:
    """``d[p][k]`` fp32 for ``x`` fp32 ``[n, C]`` and ``centroids`` fp32 ``[K, C]``: per octet of 8 channels
    ``p = p + e*e`` in ascending channel order from 0, then the octet sums combined by ``p = p[..., :s] + p[..., s:2s]`` for
    ``s = Q/2 ... 1``; every difference, product and sum an fp32 operation of its own."""
    x = np.asarray(x, dtype=F32)
    c = np.asarray(centroids, dtype=F32)
    n, C = x.shape
    K, Q = c.shape[0], C // 8
    assert C in _lib.KMF_CHANNELS, f"{C} channels: C/8 must be a power of two for the pairwise sums"
    with np.errstate(invalid="ignore", over="ignore"):
        e = x[:, None, :] - c[None, :, :]
        q = (e * e).reshape(n, K, Q, 8)
        p = np.zeros((n, K, Q), dtype=F32)
        for j in range(8):
            p = p + q[..., j]
        s = Q // 2
        while s >= 1:
            p = p[..., :s] + p[..., s:2 * s]
            s //= 2
    assert p.dtype == F32 and p.shape == (n, K, 1)
    return p[..., 0]


def nearest(d) -> np.ndarray:
    """The first ``k`` in ascending order with ``d_k <`` the best so far, which starts at +inf: an explicit strict ``<`` (the
    lowest index wins a tie, a NaN distance never wins, a pixel without a finite distance gets 0)."""
    best = np.full(d.shape[0], np.inf, dtype=F32)
    labels = np.zeros(d.shape[0], dtype=np.uint8)
    with np.errstate(invalid="ignore"):
        for k in range(d.shape[1]):
            wins = d[:, k] < best
            best = np.where(wins, d[:, k], best)
            labels = np.where(wins, np.uint8(k), labels)
    return labels


def _launch_sum(values: np.ndarray, G: int) -> np.ndarray:
    """``values`` ``[n, ...]`` float64 (zero where a pixel does not count) added in the launch's order: reshaped with zero
    padding to ``[pass][workgroup][wave][group][...]``; the passes one after the other from 0.0, the groups pairwise
    (``v = v[:h] + v[h:2h]``, ``h = G/2 ... 1``), the waves one after the other from 0.0.  ``[workgroup][...]``."""
    n = values.shape[0]
    tail = values.shape[1:]
    per_pass = _lib.KMF_PARTS * _lib.KMF_WAVES * G
    passes = max(1, -(-n // per_pass))
    padded = np.zeros((passes * per_pass, *tail), dtype=F64)
    padded[:n] = values
    padded = padded.reshape(passes, _lib.KMF_PARTS, _lib.KMF_WAVES, G, *tail)
    acc = np.zeros(padded.shape[1:], dtype=F64)
    for t in range(passes):
        acc = acc + padded[t]
    h = G // 2
    while h >= 1:
        acc = acc[:, :, :h] + acc[:, :, h:2 * h]
        h //= 2
    acc = acc[:, :, 0]
    out = np.zeros((_lib.KMF_PARTS, *tail), dtype=F64)
    for w in range(_lib.KMF_WAVES):
        out = out + acc[:, w]
    return out


def assign(x, centroids, prev, *, keep_labels: bool = False):
    """``labels [n] uint8, parts [KMF_PARTS, kmf_row_doubles(C)] float64`` for ``x`` fp32 ``[n, C]`` (bf16 features widened
    exactly beforehand), ``centroids`` fp32 ``[K, C]`` and the previous labels ``prev`` uint8 ``[n]``.  ``keep_labels``: the
    labels stay, the changed count is 0, a label >= K is in no sum."""
    x = np.asarray(x, dtype=F32)
    c = np.asarray(centroids, dtype=F32)
    prev = np.asarray(prev, dtype=np.uint8).reshape(-1)
    n, C = x.shape
    K = c.shape[0]
    _, G, _ = _lib.kmf_geometry(C)
    labels = prev.copy() if keep_labels else nearest(distances(x, c))
    parts = np.zeros((_lib.KMF_PARTS, _lib.kmf_row_doubles(C)), dtype=F64)
    wide = x.astype(F64)
    for k in range(K):
        mine = labels == k
        parts[:, k * (C + 1):k * (C + 1) + C] = _launch_sum(np.where(mine[:, None], wide, 0.0), G)
        parts[:, k * (C + 1) + C] = _launch_sum(mine.astype(F64), G)
    if not keep_labels:
        parts[:, -1] = _launch_sum((labels != prev).astype(F64), G)
    return labels, parts


def update(parts_c, parts_s, centroids, n_c: int, n_s: int):
    """``centroids [K, C] fp32, result [9] float64``: the rows of each image added in index order, then per cluster
    ``fp32((S_c/n_c + S_s/n_s) / (N_c/n_c + N_s/n_s))`` with every operation a float64 operation of its own; a cluster of
    weight 0 keeps its centroid."""
    c = np.asarray(centroids, dtype=F32).copy()
    K, C = c.shape
    totals = []
    for parts in (parts_c, parts_s):
        parts = np.asarray(parts, dtype=F64)
        total = parts[0].copy()
        for r in range(1, parts.shape[0]):
            total = total + parts[r]
        totals.append(total)
    result = np.zeros(9, dtype=F64)
    dc, ds = F64(n_c), F64(n_s)
    for k in range(K):
        at = k * (C + 1)
        nc, ns = totals[0][at + C], totals[1][at + C]
        weight = nc / dc + ns / ds
        if weight > 0.0:
            mean = totals[0][at:at + C] / dc + totals[1][at:at + C] / ds
            c[k] = (mean / weight).astype(F32)
        result[k], result[4 + k] = nc, ns
    result[8] = totals[0][-1] + totals[1][-1]
    return c, result


def _host(F: torch.Tensor) -> np.ndarray:
    C = int(F.shape[-1])
    return F.detach().float().cpu().numpy().reshape(-1, C)            # bf16 -> fp32 is exact


def assign_op(F: torch.Tensor, centroids: torch.Tensor, labels: torch.Tensor, parts: torch.Tensor | None = None, *,
              keep_labels: bool = False) -> torch.Tensor:
    """:func:`assign` behind the signature of ``ops.kmeans_feat_assign``, for tensors on any device: ``labels`` in place."""
    new, rows = assign(_host(F), centroids.detach().cpu().numpy(), labels.cpu().numpy(), keep_labels=keep_labels)
    if not keep_labels:
        labels.copy_(torch.from_numpy(new).reshape(labels.shape))
    if parts is None:
        parts = torch.empty(rows.shape, dtype=torch.float64, device=F.device)
    parts.copy_(torch.from_numpy(rows))
    return parts


def update_op(parts_c: torch.Tensor, parts_s: torch.Tensor, centroids: torch.Tensor, n_c: int, n_s: int,
              result: torch.Tensor | None = None) -> torch.Tensor:
    """:func:`update` behind the signature of ``ops.kmeans_feat_update``: ``centroids`` in place."""
    new, res = update(parts_c.cpu().numpy(), parts_s.cpu().numpy(), centroids.detach().cpu().numpy(), n_c, n_s)
    centroids.copy_(torch.from_numpy(new))
    if result is None:
        result = torch.empty(9, dtype=torch.float64, device=centroids.device)
    result.copy_(torch.from_numpy(res))
    return result


def moments_op(F: torch.Tensor):
    """``segment.feature_moments`` of features on any device in float64: ``(n, sums[C], second[C, C])``."""
    x = _host(F).astype(F64)
    return x.shape[0], x.sum(axis=0), x.T @ x


HOST = {"assign": assign_op, "update": update_op, "moments": moments_op}
