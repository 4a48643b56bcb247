"""The NumPy fp32 twin of stv_resize2x (tests/resize_ref.py) against torch on the CPU: ``F.avg_pool2d(x, 2)`` and
``F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)``.  No GPU.

* Integer-valued images in [-8, 8]: every product with 0.75 / 0.25 and every sum is exact in fp32 (multiples of 1/16 far
  below 2^24), so the twin equals torch exactly whatever order torch evaluates in.
* ``3 * randn`` images: within ``8 * 2^-24 * max|x|``.  Each of the two passes of the twin makes at most three roundings
  (two products, one sum) of values bounded by max|x| - 4u with the one the second pass inherits - and torch's path makes
  as many: 4u + 4u.  (DOWN2: three sums and an exact product on each side, inside the same bound.)
"""
from __future__ import annotations

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import resize_ref as rr

U = 2.0 ** -24
UP_SHAPES = [(3, 1, 1), (3, 1, 7), (3, 5, 1), (3, 3, 5), (3, 17, 33), (3, 64, 48), (1, 2, 2)]
DOWN_SHAPES = [(3, 2, 2), (3, 2, 14), (3, 10, 2), (3, 6, 10), (3, 34, 66), (3, 128, 96)]
_ids = lambda v: "x".join(map(str, v))      # noqa: E731


def torch_up2(a: np.ndarray) -> np.ndarray:
    return F.interpolate(torch.from_numpy(a)[None], scale_factor=2, mode="bilinear", align_corners=False)[0].numpy()


def torch_down2(a: np.ndarray) -> np.ndarray:
    return F.avg_pool2d(torch.from_numpy(a)[None], 2)[0].numpy()


@pytest.mark.parametrize("shape", UP_SHAPES, ids=_ids)
def test_up2_equals_torch_on_integers(shape):
    a = rr.pattern(*shape)
    got = rr.up2(a)
    assert got.dtype == np.float32 and got.shape == (shape[0], 2 * shape[1], 2 * shape[2])
    assert np.array_equal(got, torch_up2(a))


@pytest.mark.parametrize("shape", DOWN_SHAPES, ids=_ids)
def test_down2_equals_torch_on_integers(shape):
    a = rr.pattern(*shape)
    got = rr.down2(a)
    assert got.dtype == np.float32 and got.shape == (shape[0], shape[1] // 2, shape[2] // 2)
    assert np.array_equal(got, torch_down2(a))


@pytest.mark.parametrize("shape", UP_SHAPES, ids=_ids)
def test_up2_stays_within_the_derived_bound_on_random_data(shape):
    a = rr.randn3(*shape, seed=100 + shape[2])
    err = float(np.abs(rr.up2(a).astype(np.float64) - torch_up2(a).astype(np.float64)).max())
    bound = 8 * U * float(np.abs(a).max())
    print(f"up2 {shape}: max |twin - torch| = {err / (U * float(np.abs(a).max())):.2f} u max|x| (bound 8)")
    assert err <= bound


@pytest.mark.parametrize("shape", DOWN_SHAPES, ids=_ids)
def test_down2_stays_within_the_derived_bound_on_random_data(shape):
    a = rr.randn3(*shape, seed=200 + shape[2])
    err = float(np.abs(rr.down2(a).astype(np.float64) - torch_down2(a).astype(np.float64)).max())
    bound = 8 * U * float(np.abs(a).max())
    print(f"down2 {shape}: max |twin - torch| = {err / (U * float(np.abs(a).max())):.2f} u max|x| (bound 8)")
    assert err <= bound


def test_twin_against_float64_definition():
    """The twin's index rule, checked against a float64 evaluation of half-pixel bilinear sampling written the long
    way (source coordinate (X + 0.5) / 2 - 0.5, clamped), on an exact integer image."""
    a = rr.pattern(3, 5, 7).astype(np.float64)
    C, H, W = a.shape
    want = np.empty((C, 2 * H, 2 * W))
    for Y in range(2 * H):
        sy = min(max((Y + 0.5) / 2 - 0.5, 0.0), H - 1.0)
        y0 = int(np.floor(sy)); y1 = min(y0 + 1, H - 1); wy = sy - y0
        for X in range(2 * W):
            sx = min(max((X + 0.5) / 2 - 0.5, 0.0), W - 1.0)
            x0 = int(np.floor(sx)); x1 = min(x0 + 1, W - 1); wx = sx - x0
            top = (1 - wx) * a[:, y0, x0] + wx * a[:, y0, x1]
            bot = (1 - wx) * a[:, y1, x0] + wx * a[:, y1, x1]
            want[:, Y, X] = (1 - wy) * top + wy * bot
    assert np.array_equal(rr.up2(a.astype(np.float32)).astype(np.float64), want)


def test_leading_dimension_is_kept_and_odd_sizes_are_refused():
    a = rr.pattern(3, 4, 6)
    assert rr.up2(a[None]).shape == (1, 3, 8, 12) and rr.down2(a[None]).shape == (1, 3, 2, 3)
    assert np.array_equal(rr.up2(a[None])[0], rr.up2(a))
    with pytest.raises(ValueError, match="even"):
        rr.down2(rr.pattern(3, 3, 4))
