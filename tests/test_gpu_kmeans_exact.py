"""Exact parity of ``stv_kmeans_assign`` with its NumPy twin (tests/kmeans_ref.py) on a real MI355X.

Operands are exact: pixel values are small integers, centroids integers and half-integers, so every difference, square and sum
of the distance is exact in fp32, ties occur (two centroids coincide, and integer pixels sit half-way between others), and the
double sums are integers in any order.  Labels are compared with ``torch.equal``; the float64 sum over the 256 rows of ``parts``
is compared exactly, entry by entry, on a buffer that starts as NaN: every entry of every row is written.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from style_transfer_visualizer_amd import _lib, ops
from tests import kmeans_ref as ref
from tests.conftest import record_parity

pytestmark = pytest.mark.gpu

DEV = "cuda"
PER_PASS = _lib.KMEANS_PARTS * _lib.KMEANS_THREADS          # items (four pixels of a row) in one pass of the grid
SHAPES = [(1, 1), (1, 5), (3, 4), (4, 3), (5, 7), (8, 8), (64, 4096), (65, 4096)]
assert 64 * 4096 // 4 == PER_PASS
# clusters 1 and 3 coincide (3 never wins); cluster 2 is the mirror image of cluster 0 about the pixels (1, b, 1): every such
# pixel is an exact tie between the two, which cluster 0 wins
CENTROIDS = np.array([[0.0, 0.0, 0.0], [1.5, -0.5, 2.0], [2.0, 0.0, 2.0], [1.5, -0.5, 2.0]], dtype=np.float32)
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)      # noqa: E731


@functools.lru_cache(maxsize=None)
def image(shape: tuple[int, int]) -> np.ndarray:
    """Integer-valued fp32 ``[3, H, W]`` in [-3, 4], a different pattern per channel; shared, never modified."""
    H, W = shape
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([(3 * yy + xx) % 8 - 3, (yy + 5 * xx) % 7 - 3, (2 * yy + 3 * xx + yy * xx) % 6 - 2]).astype(np.float32)
    img[:, 0, 0] = img[:, -1, -1] = (1.0, 2.0, 1.0)        # distance 6 from clusters 0 and 2, 7.5 from cluster 1: a tie that decides
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def case(shape: tuple[int, int], K: int) -> dict:
    """The twin's answer for (shape, K), and previous labels that are random: computed once, shared."""
    x = image(shape)
    rng = np.random.RandomState(shape[0] * 131 + shape[1] + K)
    random_prev = rng.randint(0, 4, size=shape).astype(np.uint8)
    labels, sums, counts, _ = ref.assign(x, CENTROIDS[:K], random_prev)
    assert int(labels[0, 0]) == int(labels[-1, -1]) == 0            # the tie of clusters 0 and 2 goes to the lower index
    if K >= 3:      # noqa: PLR2004
        assert not (labels == 3).any()                  # cluster 3 coincides with cluster 1: the tie goes to the lower index
    assert np.array_equal(sums, np.round(sums)) and np.abs(sums).max() < 2.0 ** 40
    return {"x": x, "labels": labels, "sums": sums, "counts": counts, "random_prev": random_prev,
            "random_changed": int((random_prev != labels).sum())}


def on_device(array: np.ndarray, offset: int = 0) -> torch.Tensor:
    """A device copy of ``array`` whose base address is ``offset`` elements past an allocation's (aligned) start."""
    t = torch.from_numpy(np.array(array))                  # (a copy: the shared arrays are read-only)
    buf = torch.zeros(t.numel() + offset, dtype=t.dtype, device=DEV)[offset:].view(t.shape)
    buf.copy_(t)
    assert buf.is_contiguous() and buf.data_ptr() % 16 == (offset * t.element_size()) % 16
    return buf


def nan_parts() -> torch.Tensor:
    return torch.full((_lib.KMEANS_PARTS, _lib.KMEANS_PART_DOUBLES), float("nan"), dtype=torch.float64, device=DEV)


def check(x, cen, labels, parts, want: dict, changed: int, what: str) -> None:
    parts.fill_(float("nan"))
    assert ops.kmeans_assign(x, cen, labels, parts) is parts
    rows = parts.cpu().numpy()
    assert np.isfinite(rows).all(), f"{what}: {int((~np.isfinite(rows)).sum())} entries of parts were not written"
    K = len(want["counts"])
    total = rows.sum(axis=0, dtype=np.float64)
    print(f"{what}: counts {total[3:16:4].tolist()} changed {total[16]}")
    assert np.array_equal(total, ref.parts_row(want["sums"], want["counts"], changed)), f"{what}: {total.tolist()}"
    assert not rows[:, 4 * K:16].any(), f"{what}: entries of clusters >= K are not zero"
    got = labels.cpu()
    if not torch.equal(got, torch.from_numpy(want["labels"])):
        diff = (got != torch.from_numpy(want["labels"])).nonzero()
        first = tuple(int(v) for v in diff[0])
        pytest.fail(f"{what}: {len(diff)} labels differ; first at {first}: got {int(got[first])}, expected {int(want['labels'][first])}")


@pytest.fixture(scope="module", autouse=True)
def _parity_rows():
    yield
    record_parity("exact k-means assignment", "differing labels / sums", 0.0, 0.0,
                  f"{(len(SHAPES) + 2) * 4} cases x 4 launches, compared bit for bit")


@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("shape,offset", [*((s, "aligned") for s in SHAPES), ((8, 8), "x+4B"), ((8, 8), "labels+1B")],
                         ids=lambda v: _ids(v))
def test_labels_and_sums_equal_the_twin(shape, offset, K):
    want = case(shape, K)
    n = shape[0] * shape[1]
    x = on_device(want["x"], 1 if offset == "x+4B" else 0)
    cen = torch.from_numpy(CENTROIDS[:K].copy()).to(DEV)
    parts = nan_parts()
    what = f"{_ids(shape)} {offset} K={K}"

    def previous(values: np.ndarray) -> torch.Tensor:
        return on_device(values, 1 if offset == "labels+1B" else 0)
    # previous labels all 255: every label changes
    labels = previous(np.full(shape, 255, dtype=np.uint8))
    check(x, cen, labels, parts, want, n, what + " from 255")
    # a second launch on the same buffers: the labels are the answer, nothing changes, the same sums
    check(x, cen, labels, parts, want, 0, what + " again")
    # random previous labels: some change
    check(x, cen, previous(want["random_prev"]), parts, want, want["random_changed"], what + " from random")
    # previous labels equal to the answer, on a fresh buffer
    check(x, cen, previous(want["labels"]), parts, want, 0, what + " from the answer")
    assert want["x"].flags.writeable is False and torch.equal(x.cpu(), torch.from_numpy(want["x"]))      # the image is only read


def test_wrapper_refuses_what_the_kernel_does_not_take():
    x = torch.zeros(3, 4, 4, device=DEV)
    cen = torch.zeros(2, 3, device=DEV)
    labels = torch.zeros(4, 4, dtype=torch.uint8, device=DEV)
    for bad in (dict(x=x.double()), dict(x=torch.zeros(4, 4, 4, device=DEV)), dict(cen=torch.zeros(2, 4, device=DEV)),
                dict(cen=torch.zeros(5, 3, device=DEV)), dict(cen=cen.double()), dict(labels=labels.int()),
                dict(labels=torch.zeros(4, 5, dtype=torch.uint8, device=DEV)), dict(parts=torch.zeros(256, 16, dtype=torch.float64, device=DEV)),
                dict(parts=torch.zeros(256, 17, device=DEV))):
        args = {"x": x, "cen": cen, "labels": labels, "parts": None, **bad}
        with pytest.raises(RuntimeError):
            ops.kmeans_assign(args["x"], args["cen"], args["labels"], args["parts"])
    out = ops.kmeans_assign(x, cen, labels)
    assert tuple(out.shape) == (256, 17) and out.dtype == torch.float64 and float(out.sum(dim=0)[3]) == 16.0      # noqa: PLR2004
