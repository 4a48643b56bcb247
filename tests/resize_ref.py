"""NumPy fp32 twin of the two modes of ``stv_resize2x``, written from the definition in include/stv.h (not from the kernel).

Every product and every sum is one NumPy float32 operation - rounded to fp32 on its own, no fused multiply-add - in the
order the definition writes them, so that the kernel can be compared with ``torch.equal``.

    DOWN2   y[c,Y,X] = ((x[c,2Y,2X] + x[c,2Y,2X+1]) + (x[c,2Y+1,2X] + x[c,2Y+1,2X+1])) * 0.25
    UP2     output index X: near n = X >> 1, far f = clamp(n + (+1 if X is odd else -1), 0, size - 1);
            h[r,X] = 0.75*x[r,n] + 0.25*x[r,f] along the columns, then the same rule along the rows of h.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
NEAR_W, FAR_W, QUARTER = F32(0.75), F32(0.25), F32(0.25)


def _chw(x) -> tuple[np.ndarray, tuple]:
    a = np.asarray(x, dtype=F32)
    return a.reshape(a.shape[-3], a.shape[-2], a.shape[-1]), a.shape[:-2]


def near_far(size: int) -> tuple[np.ndarray, np.ndarray]:
    """Near and far source index of each of the ``2 * size`` output indices along one axis."""
    out = np.arange(2 * size)
    near = out >> 1
    far = np.clip(near + np.where(out & 1, 1, -1), 0, size - 1)
    return near, far


def down2(x) -> np.ndarray:
    """2x2 box mean of an image ``[..., C, H, W]`` with even H and W; fp32, same rank."""
    a, lead = _chw(x)
    C, H, W = a.shape
    if H % 2 or W % 2:
        msg = f"down2 needs even sizes, got {H}x{W}"
        raise ValueError(msg)
    top = a[:, 0::2, 0::2] + a[:, 0::2, 1::2]
    bottom = a[:, 1::2, 0::2] + a[:, 1::2, 1::2]
    y = (top + bottom) * QUARTER
    assert y.dtype == F32
    return y.reshape(*lead, H // 2, W // 2)


def up2(x) -> np.ndarray:
    """Bilinear 2x (half-pixel centres, clamped edges) of an image ``[..., C, H, W]``; fp32, same rank."""
    a, lead = _chw(x)
    C, H, W = a.shape
    n, f = near_far(W)
    h = NEAR_W * a[:, :, n] + FAR_W * a[:, :, f]                # columns first: [C, H, 2W]
    n, f = near_far(H)
    y = NEAR_W * h[:, n, :] + FAR_W * h[:, f, :]                # then rows: [C, 2H, 2W]
    assert h.dtype == F32 and y.dtype == F32
    return y.reshape(*lead, 2 * H, 2 * W)


def pattern(C: int, H: int, W: int) -> np.ndarray:
    """Integer-valued fp32 image in [-8, 8]: another busy pattern per channel; the first and last row of a plane and
    (overriding them) the first and last pixel of a row are pinned to -8 + c and 8 - c, so the value jumps by 12 or more
    across a row end and by 11 or more across a plane end - a read across either gives a wrong value."""
    c = np.arange(C).reshape(C, 1, 1)
    y = np.arange(H).reshape(1, H, 1)
    x = np.arange(W).reshape(1, 1, W)
    v = (x * (3 + 2 * c) + y * (5 + c) + x * y * (c + 1) + 7 * c) % 17 - 8
    v = np.broadcast_to(v, (C, H, W)).copy()
    if H > 1:
        v[:, 0, :] = -8 + c[:, 0]
        v[:, -1, :] = 8 - c[:, 0]
    if W > 1:
        v[:, :, 0] = -8 + c[:, 0]
        v[:, :, -1] = 8 - c[:, 0]
    img = v.astype(F32)
    assert np.abs(img).max() <= 8
    if C <= 3 and W > 1 and H > 1:
        assert np.abs(img[:, 1:, 0] - img[:, :-1, -1]).min() >= 12
    if 1 < C <= 3 and H > 1 and W > 2:
        assert np.abs(img[1:, 0, 1:-1] - img[:-1, -1, 1:-1]).min() >= 11
    return img


def randn3(C: int, H: int, W: int, seed: int) -> np.ndarray:
    """``3 * randn`` fp32 image from a seeded NumPy generator."""
    return (3.0 * np.random.default_rng(seed).standard_normal((C, H, W))).astype(F32)
