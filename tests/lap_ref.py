"""NumPy twin of the Laplacian loss (``stv_lap``, csrc/lap.hip), in the kernel's own order of operations, and rounding-chain
bounds of the fp32 twin against the float64 one.

    Hp = H // p, Wp = W // p;   P(x)[c,i,j] = mean of cell (i, j);   e = P(x) - t;   r = L e;   g = L r
    (L v)[i,j] = sum over the existing 4-neighbours n of (v[i,j] - n)          lap = sum r^2 / (C*Hp*Wp)

Every function takes ``dtype``: ``np.float32`` reproduces the kernel bit for bit (NumPy rounds every array operation to the
array's type, and nothing here is fused), ``np.float64`` is the same arithmetic in double.

    cell mean: each of the p rows of the cell summed left to right, the p row sums summed top to bottom, then * 1/p^2
    residual:  e = mean - t, one subtraction
    stencil:   s = +0, then s = s + (v - n) in the order up, down, left, right, where the neighbour exists
    gradient:  out = coef * (L r), then dx = dx + out (or dx = out, +0 outside the covered Hp*p x Wp*p pixels)
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32


def _chw(x, dtype) -> np.ndarray:
    a = np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x)
    return np.ascontiguousarray(a.reshape(a.shape[-3:]), dtype=dtype)


def pool(x, p: int, dtype=np.float32) -> np.ndarray:
    """Cell means ``[C, H//p, W//p]``."""
    a = _chw(x, dtype)
    C, H, W = a.shape
    Hp, Wp = H // p, W // p
    v = a[:, :Hp * p, :Wp * p].reshape(C, Hp, p, Wp, p)
    row = v[..., 0].copy()
    for k in range(1, p):                       # left to right
        row = row + v[..., k]
    total = row[:, :, 0, :].copy()
    for j in range(1, p):                       # top to bottom
        total = total + row[:, :, j, :]
    return total * dtype(1.0 / (p * p))


def stencil(v: np.ndarray) -> np.ndarray:
    """``L v`` on ``[C, Hp, Wp]``, in ``v``'s type."""
    s = np.zeros_like(v)
    s[:, 1:, :] = s[:, 1:, :] + (v[:, 1:, :] - v[:, :-1, :])        # up
    s[:, :-1, :] = s[:, :-1, :] + (v[:, :-1, :] - v[:, 1:, :])      # down
    s[:, :, 1:] = s[:, :, 1:] + (v[:, :, 1:] - v[:, :, :-1])        # left
    s[:, :, :-1] = s[:, :, :-1] + (v[:, :, :-1] - v[:, :, 1:])      # right
    return s


def resid(x, t, p: int, dtype=np.float32) -> np.ndarray:
    """``r = L (P(x) - t)`` with ``t`` the pooled target ``[C, Hp, Wp]``."""
    return stencil(pool(x, p, dtype) - np.asarray(t, dtype=dtype))


def raw_sum(r: np.ndarray) -> float:
    """Sum of ``r**2`` in float64 (the unscaled quantity the kernel's partial sums add up to; each square rounded to ``r``'s
    type first, as the kernel does)."""
    return float((r * r).astype(np.float64).sum())


def upsample(cells: np.ndarray, p: int) -> np.ndarray:
    return np.repeat(np.repeat(cells, p, axis=1), p, axis=2)


def grad_accum(r: np.ndarray, dx0, p: int, coef: float, accum: bool = True, dtype=np.float32) -> np.ndarray:
    """``dx0`` (``[C, H, W]``) after the GRAD mode: the covered pixels ``dx0 + coef * (L r)`` of their cell (``accum``) or
    ``coef * (L r)``, the others untouched (``accum``) or +0.  ``coef`` is the fp32 number the kernel receives."""
    d = _chw(dx0, dtype)
    C, H, W = d.shape
    Hp, Wp = H // p, W // p
    out = upsample(dtype(np.float32(coef)) * stencil(np.asarray(r, dtype=dtype)), p)
    res = d.copy() if accum else np.zeros_like(d)
    res[:, :Hp * p, :Wp * p] = (d[:, :Hp * p, :Wp * p] + out) if accum else out
    return res


def loss(x, content, p: int, dtype=np.float64) -> float:
    """``lap_p(x)`` against the content IMAGE."""
    r = resid(x, pool(content, p, dtype), p, dtype)
    return float((r.astype(np.float64) ** 2).sum() / r.size)


def loss_grad(x, content, p: int, dtype=np.float64) -> np.ndarray:
    """``d lap_p / dx`` as the kernel forms it: ``2 / (C*Hp*Wp*p*p) * (L r)`` of the pixel's cell, 0 outside the cover."""
    r = resid(x, pool(content, p, dtype), p, dtype)
    a = _chw(x, dtype)
    return grad_accum(r, np.zeros_like(a), p, 1.0, accum=False, dtype=dtype) * dtype(2.0 / (r.size * p * p))


# ---- rounding-chain bounds: |fp32 twin - float64 twin|, elementwise, for the SAME fp32 inputs ------------------------------------
# gamma(k) = k*U / (1 - k*U) bounds the relative error of a sum whose every element passes through at most k rounded adds.
def gamma(k: int) -> float:
    return k * U / (1.0 - k * U)


def _plus(d: np.ndarray) -> np.ndarray:
    """sum over the existing neighbours n of (d + d_n)."""
    s = np.zeros_like(d)
    s[:, 1:, :] += d[:, 1:, :] + d[:, :-1, :]
    s[:, :-1, :] += d[:, :-1, :] + d[:, 1:, :]
    s[:, :, 1:] += d[:, :, 1:] + d[:, :, :-1]
    s[:, :, :-1] += d[:, :, :-1] + d[:, :, 1:]
    return s


def _abs(v: np.ndarray) -> np.ndarray:
    """sum over the existing neighbours n of |v - v_n|."""
    s = np.zeros_like(v)
    s[:, 1:, :] += np.abs(v[:, 1:, :] - v[:, :-1, :])
    s[:, :-1, :] += np.abs(v[:, :-1, :] - v[:, 1:, :])
    s[:, :, 1:] += np.abs(v[:, :, 1:] - v[:, :, :-1])
    s[:, :, :-1] += np.abs(v[:, :, :-1] - v[:, :, 1:])
    return s


def _stencil_bound(v64: np.ndarray, dv: np.ndarray) -> np.ndarray:
    """Bound on |L32(v32) - L64(v64)| given |v32 - v64| <= dv.  Each difference fl(v - n) is off by at most
    dv + dv_n (its inputs) + U * |v32 - n32| (its rounding), |v32 - n32| <= |v64 - n64| + dv + dv_n; the up-to-four
    differences are then added in sequence from 0 (the first add is exact): at most 3 rounded adds, gamma(3) of the sum of
    their magnitudes."""
    dd = _plus(dv) + U * (_abs(v64) + _plus(dv))
    return dd * (1.0 + gamma(3)) + gamma(3) * _abs(v64)


def bounds(x, content, p: int, coef: float, dx0=None) -> dict:
    """Elementwise bounds for the fp32 twin against the float64 twin on the same fp32 images: ``pool`` (of x), ``e``, ``r``,
    ``out`` (= coef * L r on the cell grid) and, with ``dx0``, ``dx`` (on the pixel grid).

    cell mean: an element passes through at most (p-1) + (p-1) rounded adds, so |m32 - m64| <= gamma(2p-2) * mean|x| of the
    cell (the product with 1/p^2 is exact); the same for the target.  e = fl(m - t): the two input errors plus U * |m32 - t32|.
    r and g: :func:`_stencil_bound` twice.  out = fl(coef * g): coef * dg, plus U * |coef * g32|.  dx = fl(dx0 + out): dout plus
    U * |dx0 + out32|."""
    xa, ca = _chw(x, np.float64), _chw(content, np.float64)
    g2 = gamma(max(2 * p - 2, 0))
    dm, dt = g2 * pool(np.abs(xa), p, np.float64), g2 * pool(np.abs(ca), p, np.float64)
    e64 = pool(xa, p, np.float64) - pool(ca, p, np.float64)
    de = dm + dt
    de = de + U * (np.abs(e64) + de)
    r64 = stencil(e64)
    dr = _stencil_bound(e64, de)
    g64 = stencil(r64)
    dg = _stencil_bound(r64, dr)
    c = abs(float(np.float32(coef)))
    dout = c * dg + U * c * (np.abs(g64) + dg)
    out = {"pool": dm, "e": de, "r": dr, "out": dout}
    if dx0 is not None:
        d = _chw(dx0, np.float64)
        C, H, W = d.shape
        Hp, Wp = H // p, W // p
        full = np.zeros_like(d)
        cover = (slice(None), slice(0, Hp * p), slice(0, Wp * p))
        up_out, up_d = upsample(float(np.float32(coef)) * g64, p), upsample(dout, p)
        full[cover] = up_d + U * (np.abs(d[cover] + up_out) + up_d)
        out["dx"] = full
    return out


def partial_sum_depth(C: int, Hp: int, Wp: int, tile_h: int, tile_w: int, parts: int) -> int:
    """The most rounded operations an r^2 passes through on its way into a loss partial: the square, one add per tile of the
    workgroup's stride loop, six butterfly levels of the wave sum and two levels over the four waves."""
    tiles = C * (-(-Hp // tile_h)) * (-(-Wp // tile_w))
    return 1 + (-(-tiles // parts)) + 6 + 2
