"""NumPy twins of the three colour kernels, written from the definitions in include/stv.h (not from the kernels).

    moments   float64 sums of x_c and of x_i * x_j over the pixels (the kernel forms both in double from the fp32 values)
    affine    y[c] = ((m[c][0]*x[0] + m[c][1]*x[1]) + m[c][2]*x[2]) + b[c]
    luma      out = content_rgb + (Y(result_rgb) - Y(content_rgb)), Rec.601 Y, in [0, 1] RGB, mapped back

In ``affine`` and ``luma`` every product and every sum is one NumPy float32 operation - rounded to fp32 on its own, no
fused multiply-add - in the order the definition writes them, so that the kernels can be compared with ``torch.equal``.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
REC601 = (F32(0.299), F32(0.587), F32(0.114))
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))          # order of the six products in a row of `parts`


def _chw(x, dtype=F32) -> tuple[np.ndarray, tuple]:
    a = np.asarray(x, dtype=dtype)
    assert a.shape[-3] == 3
    return a.reshape(3, a.shape[-2], a.shape[-1]), a.shape


def moments(x) -> np.ndarray:
    """The nine raw moments of an image ``[..., 3, H, W]`` in the kernel's order, float64: sum x0, x1, x2, then the products
    of ``PAIRS``."""
    a, _ = _chw(x, np.float64)
    return np.array([a[c].sum() for c in range(3)] + [(a[i] * a[j]).sum() for i, j in PAIRS], dtype=np.float64)


def abs_moments(x) -> np.ndarray:
    """sum |term| of each of the nine moments: the scale of a summation's rounding error."""
    a, _ = _chw(x, np.float64)
    return np.array([np.abs(a[c]).sum() for c in range(3)] + [np.abs(a[i] * a[j]).sum() for i, j in PAIRS], dtype=np.float64)


def stats(x) -> tuple[int, np.ndarray, np.ndarray]:
    """``(n, sums[3], moments[3, 3])`` as ``color.statistics`` returns them, from :func:`moments`."""
    a, _ = _chw(x, np.float64)
    m = moments(a)
    second = np.empty((3, 3))
    for v, (i, j) in zip(m[3:], PAIRS, strict=True):
        second[i, j] = second[j, i] = v
    return a.shape[1] * a.shape[2], m[:3].copy(), second


def mean_cov(x) -> tuple[np.ndarray, np.ndarray]:
    """Per-channel mean and 3x3 covariance (divisor n) of an image, float64, two-pass."""
    a, _ = _chw(x, np.float64)
    flat = a.reshape(3, -1)
    mu = flat.mean(axis=1)
    d = flat - mu[:, None]
    return mu, d @ d.T / flat.shape[1]


def affine(x, m12) -> np.ndarray:
    """The fp32 affine map of an image ``[..., 3, H, W]``; ``m12``: 12 numbers, row-major matrix then offset."""
    a, shape = _chw(x)
    t = np.asarray(m12, dtype=F32).reshape(-1)
    assert t.shape == (12,)
    m, b = t[:9].reshape(3, 3), t[9:]
    y = np.empty_like(a)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(3):
            s01 = m[c, 0] * a[0] + m[c, 1] * a[1]
            y[c] = (s01 + m[c, 2] * a[2]) + b[c]
    assert y.dtype == F32
    return y.reshape(shape)


def rgb01(x, *, normalize: bool) -> np.ndarray:
    """``prepare_image_for_output`` in fp32: denormalise (two roundings), nan -> 0, +inf -> 1, -inf -> 0, clamp to [0, 1]."""
    a, shape = _chw(x)
    with np.errstate(invalid="ignore", over="ignore"):
        if normalize:
            mean = np.asarray(IMAGENET_MEAN, dtype=F32).reshape(3, 1, 1)
            std = np.asarray(IMAGENET_STD, dtype=F32).reshape(3, 1, 1)
            a = a * std + mean
        a = np.where(np.isnan(a), F32(0), a)
        a = np.minimum(np.maximum(a, F32(0)), F32(1))
    assert a.dtype == F32
    return a.reshape(shape)


def luma_y(rgb) -> np.ndarray:
    """Rec.601 luminance ``(0.299 R + 0.587 G) + 0.114 B`` of ``[..., 3, H, W]`` in fp32 -> ``[H, W]``."""
    a, _ = _chw(rgb)
    y = (REC601[0] * a[0] + REC601[1] * a[1]) + REC601[2] * a[2]
    assert y.dtype == F32
    return y


def luma(result, content, *, normalize: bool) -> np.ndarray:
    """The fp32 luminance swap: the luminance of ``result`` on the chrominance of ``content``, in the tensors' space."""
    _, shape = _chw(result)
    r, k = rgb01(result, normalize=normalize).reshape(3, *shape[-2:]), rgb01(content, normalize=normalize).reshape(3, *shape[-2:])
    d = luma_y(r) - luma_y(k)
    o = k + d[None]
    if normalize:
        mean = np.asarray(IMAGENET_MEAN, dtype=F32).reshape(3, 1, 1)
        inv_std = (F32(1.0) / np.asarray(IMAGENET_STD, dtype=F32)).reshape(3, 1, 1)
        o = (o - mean) * inv_std
    assert o.dtype == F32
    return o.reshape(shape)


def pattern(H: int, W: int) -> np.ndarray:
    """Integer-valued fp32 image ``[3, H, W]`` in [-8, 8], another pattern per channel."""
    c = np.arange(3).reshape(3, 1, 1)
    y = np.arange(H).reshape(1, H, 1)
    x = np.arange(W).reshape(1, 1, W)
    v = (x * (3 + 2 * c) + y * (5 + c) + x * y * (c + 1) + 7 * c + (x // 3) * (c == 1) + (y // 2) * (c == 2)) % 17 - 8
    return np.broadcast_to(v, (3, H, W)).astype(F32)


def uint8_image(H: int, W: int, seed: int, *, normalize: bool) -> np.ndarray:
    """What the image loader returns for a random 8-bit picture with correlated channels: ``[1, 3, H, W]`` fp32."""
    rng = np.random.default_rng(seed)
    base = rng.random((1, H, W))
    mix = np.array([0.55, 0.35, 0.6]).reshape(3, 1, 1) + 0.05 * (seed % 4)
    raw = np.clip(mix * base + (1 - mix) * rng.random((3, H, W)) + 0.05 * (seed % 3 - 1), 0, 1)
    a = (np.floor(raw * 255.0).astype(np.uint8)).astype(F32) / F32(255)
    if normalize:
        a = (a - np.asarray(IMAGENET_MEAN, dtype=F32).reshape(3, 1, 1)) / np.asarray(IMAGENET_STD, dtype=F32).reshape(3, 1, 1)
    assert a.dtype == F32
    return a.reshape(1, 3, H, W)
