"""Exact parity of ``stv_kmeans_feat_assign`` / ``stv_kmeans_feat_update`` with their NumPy twins (tests/kmeans_feat_ref.py)
on a real MI355X: labels by ``torch.equal``, every double of every ``parts`` row, the updated centroids and the nine result
doubles bit for bit.

The feature values span forty binary orders of magnitude, so the sums of a ``parts`` entry are inexact in double and only the
launch's own order of additions reproduces them; the first test checks that its data has that property (a plain sum over
the pixels differs from the ordered one).  Sizes: one pixel, one short of a wave's pixels, a wave's pixels, one short of a
pass of the grid, a pass, a pass and one - for every channel count, both storage types and every ``K``.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from style_transfer_visualizer_amd import _lib, ops
from tests import kmeans_feat_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
CHANNELS = (64, 128, 256, 512)
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}


def bits(t) -> torch.Tensor:
    """The bit patterns of a float64 / float32 tensor or array, on the host."""
    t = torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t.detach().cpu().contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def features(seed: int, n: int, C: int, dtype: torch.dtype) -> torch.Tensor:
    """``[n, C]`` of ``dtype`` on the device: normal draws scaled by powers of two from 2^-20 to 2^20."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, C, generator=g) * torch.pow(2.0, torch.randint(-20, 21, (n, C), generator=g).float())
    return x.to(dtype).to(DEV)


def centroids(seed: int, K: int, C: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(1000 + seed)
    return (torch.randn(K, C, generator=g) * 64.0).to(DEV)


def nan_parts(C: int) -> torch.Tensor:
    return torch.full((_lib.KMF_PARTS, _lib.kmf_row_doubles(C)), float("nan"), dtype=torch.float64, device=DEV)


def check_assign(F, cen, labels, *, keep_labels=False) -> np.ndarray:
    """One launch against the twin: labels and every double; the parts as an array."""
    C = int(F.shape[-1])
    want_labels, want_parts = ref.assign(F.float().cpu().numpy(), cen.cpu().numpy(), labels.cpu().numpy(), keep_labels=keep_labels)
    parts = nan_parts(C)
    assert ops.kmeans_feat_assign(F, cen, labels, parts, keep_labels=keep_labels) is parts
    torch.cuda.synchronize()
    assert torch.equal(labels.cpu(), torch.from_numpy(want_labels))
    got = parts.cpu()
    assert not bool(torch.isnan(got).any())                   # every entry is written on every launch
    assert torch.equal(bits(got), bits(want_parts))
    return want_parts


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("C", CHANNELS)
def test_assign_equals_the_twin_at_every_size(C, name):
    Q, G, per_pass = _lib.kmf_geometry(C)
    assert (Q, G * Q, per_pass) == (C // 8, 64, _lib.KMF_PARTS * _lib.KMF_WAVES * G)
    sizes = sorted({1, max(1, G - 1), G, per_pass - 1, per_pass, per_pass + 1})
    order_matters = False
    for i, n in enumerate(sizes):
        for K in range(1, _lib.KMF_MAX_K + 1):
            F = features(17 * i + K, n, C, DTYPES[name])
            cen = centroids(i + K, K, C)
            labels = torch.full((n,), 255, dtype=torch.uint8, device=DEV)
            parts = check_assign(F, cen, labels)
            assert parts[:, -1].sum() == n                    # every label changed from 255
            assert sum(parts[:, k * (C + 1) + C].sum() for k in range(K)) == n
            assert not parts[:, K * (C + 1):-1].any()         # zeros for k >= K
            plain = F.float().cpu().numpy().astype(np.float64)[labels.cpu().numpy() == 0].sum(axis=0)
            total = parts[0, :C].copy()                       # cluster 0's sums: the rows in index order
            for r in range(1, parts.shape[0]):
                total = total + parts[r, :C]
            order_matters |= bool((plain != total).any())
            check_assign(F, cen, labels)                      # in place: the second pass changes nothing
    assert order_matters                                      # the data can tell one order of additions from another


def test_planted_ties_and_coincident_centroids():
    C, n = 128, 300
    F = features(3, n, C, torch.float32)
    F[7] = 0.0                                                # equidistant from +c and -c, exactly
    cen = centroids(3, 4, C)
    cen[1] = -cen[0]
    cen[2] = 3.0 * cen[0]                                     # (farther from the origin than the pair)
    cen[3] = cen[2]                                           # coincident: 3 never wins
    labels = torch.full((n,), 255, dtype=torch.uint8, device=DEV)
    check_assign(F, cen, labels)
    host = labels.cpu()
    assert int(host[7]) == 0 and not bool((host == 3).any())  # noqa: PLR2004
    d = ref.distances(F.cpu().numpy(), cen.cpu().numpy())
    assert d[7, 0] == d[7, 1]


def test_a_nan_distance_never_wins():
    C, n = 64, 40
    F = features(5, n, C, torch.float32)
    cen = centroids(5, 3, C)
    cen[0, 9] = float("nan")
    labels = torch.zeros(n, dtype=torch.uint8, device=DEV)
    ops.kmeans_feat_assign(F, cen, labels)
    want = ref.nearest(ref.distances(F.cpu().numpy(), cen.cpu().numpy()))
    assert torch.equal(labels.cpu(), torch.from_numpy(want)) and not bool((labels == 0).any())


@pytest.mark.parametrize("name", list(DTYPES))
def test_keep_labels_and_an_offset_base(name):
    C, n = 256, 2 * _lib.kmf_geometry(256)[2] + 37
    big = features(11, n + 1, C, DTYPES[name])
    F = big[1:]                                               # the base moved by one pixel
    assert F.is_contiguous() and F.data_ptr() != big.data_ptr()
    g = torch.Generator().manual_seed(4)
    start = torch.randint(0, 3, (n,), generator=g).to(torch.uint8)
    start[::17] = 255                                         # in no sum
    labels = start.to(DEV)
    parts = check_assign(F, centroids(1, 3, C), labels, keep_labels=True)
    assert torch.equal(labels.cpu(), start) and not parts[:, -1].any()
    assert sum(parts[:, k * (C + 1) + C].sum() for k in range(3)) == int((start != 255).sum())      # noqa: PLR2004
    check_assign(F, centroids(2, 4, C), labels)               # and the assignment on the same moved base
    mean = torch.zeros(n, dtype=torch.uint8, device=DEV)      # the pass that gives mu: all labels 0, K = 1
    parts = check_assign(F, torch.zeros(1, C, device=DEV), mean, keep_labels=True)
    assert parts[:, C].sum() == n


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("C", CHANNELS)
def test_update_equals_the_twin(C, name):
    K = 4
    n_c, n_s = 1500, 777
    F_c, F_s = features(21, n_c, C, DTYPES[name]), features(22, n_s, C, DTYPES[name])
    cen = centroids(9, K, C)
    cen[3] = 3.0e30                                           # empty in both images: keeps its centroid
    lab_c = torch.full((n_c,), 255, dtype=torch.uint8, device=DEV)
    lab_s = torch.full((n_s,), 255, dtype=torch.uint8, device=DEV)
    parts_c, parts_s = ops.kmeans_feat_assign(F_c, cen, lab_c), ops.kmeans_feat_assign(F_s, cen, lab_s)
    lab_s[lab_s == 2] = 0                                     # cluster 2: empty in the style image only
    parts_s = ops.kmeans_feat_assign(F_s, cen, lab_s, keep_labels=True)
    want_cen, want_res = ref.update(parts_c.cpu().numpy(), parts_s.cpu().numpy(), cen.cpu().numpy(), n_c, n_s)
    before = cen.clone()
    result = ops.kmeans_feat_update(parts_c, parts_s, cen, n_c, n_s)
    torch.cuda.synchronize()
    assert torch.equal(bits(cen), bits(want_cen)) and torch.equal(bits(result), bits(want_res))
    res = result.cpu().numpy()
    assert res[3] == 0 and res[7] == 0 and res[6] == 0 and res[2] > 0          # noqa: PLR2004
    assert torch.equal(cen[3], before[3]) and not torch.equal(cen[:3], before[:3])
    assert res[:4].sum() == n_c and res[4:8].sum() == n_s and res[8] == n_c     # (the kept style pass reports no change)


def test_ops_refusals():
    F = torch.zeros(10, 64, device=DEV)
    labels = torch.zeros(10, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="96 channels"):
        ops.kmeans_feat_assign(torch.zeros(10, 96, device=DEV), torch.zeros(2, 96, device=DEV), labels)
    for C in (192, 320, 384, 448):                            # multiples of 64 whose C/8 is no power of two
        with pytest.raises(RuntimeError, match=f"{C} channels"):
            ops.kmeans_feat_assign(torch.zeros(10, C, device=DEV), torch.zeros(2, C, device=DEV), labels)
        with pytest.raises(RuntimeError, match=f"{C} channels"):
            ops.kmeans_feat_update(torch.zeros(256, 4 * (C + 1) + 1, dtype=torch.float64, device=DEV),
                                   torch.zeros(256, 4 * (C + 1) + 1, dtype=torch.float64, device=DEV), torch.zeros(2, C, device=DEV), 10, 10)
    with pytest.raises(RuntimeError, match="576 channels"):
        ops.kmeans_feat_assign(torch.zeros(10, 576, device=DEV), torch.zeros(2, 576, device=DEV), labels)
    with pytest.raises(RuntimeError, match="5 centroids"):
        ops.kmeans_feat_assign(F, torch.zeros(5, 64, device=DEV), labels)
    with pytest.raises(RuntimeError, match="torch.float16"):
        ops.kmeans_feat_assign(F.half(), torch.zeros(2, 64, device=DEV), labels)
    with pytest.raises(RuntimeError, match="labels"):
        ops.kmeans_feat_assign(F, torch.zeros(2, 64, device=DEV), labels[:9])
