"""Float64 CPU oracle of the total-variation term (the reference has none): the definition, autograd for the gradient.

    TV(x) = ( sum_{c,y<H-1,x} (x[c,y+1,x] - x[c,y,x])^2 + sum_{c,y,x<W-1} (x[c,y,x+1] - x[c,y,x])^2 ) / (C*H*W)
    dTV/dx[c,y,x] = (2/(C*H*W)) * sum over the existing 4-neighbours n of (x[c,y,x] - n)

Written with explicit loops over the two directions on a [C, H, W] view, independently of
``core_model.total_variation`` (which the host tests compare against this).
"""
from __future__ import annotations

import torch


def _chw64(x: torch.Tensor) -> torch.Tensor:
    t = x.detach().to("cpu", torch.float64)
    return t.reshape(t.shape[-3], t.shape[-2], t.shape[-1])


def raw_sum(x: torch.Tensor) -> torch.Tensor:
    """Sum of the squared forward differences (the unscaled quantity the kernel's partial sums add up to), float64."""
    t = _chw64(x) if not (x.dtype == torch.float64 and x.dim() == 3) else x
    C, H, W = t.shape
    total = t.sum() * 0.0        # (0, and a function of t even where an image has no differences at all)
    for c in range(C):
        plane = t[c]
        if H > 1:
            total = total + ((plane[1:, :] - plane[:-1, :]) ** 2).sum()
        if W > 1:
            total = total + ((plane[:, 1:] - plane[:, :-1]) ** 2).sum()
    return total


def tv(x: torch.Tensor) -> torch.Tensor:
    """TV(x) in float64 (0-d CPU tensor)."""
    t = _chw64(x)
    return raw_sum(t) / t.numel()


def tv_and_grad(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """(TV(x), dTV/dx) in float64 on the CPU; the gradient by autograd, shaped like ``x``."""
    t = _chw64(x).clone().requires_grad_(True)
    value = raw_sum(t) / t.numel()
    (g,) = torch.autograd.grad(value, t)
    return value.detach(), g.reshape(x.shape)


def neighbour_sum(x: torch.Tensor) -> torch.Tensor:
    """sum over the existing 4-neighbours n of (x - n), float64, shaped [C, H, W]: the gradient without its factor."""
    t = _chw64(x).clone().requires_grad_(True)
    (g,) = torch.autograd.grad(raw_sum(t), t)        # 2 * sum(x - n): halving is exact
    return g / 2.0


def abs_difference_sum(x: torch.Tensor) -> torch.Tensor:
    """sum over the existing 4-neighbours n of |x - n|, float64, [C, H, W]: the scale of the gradient's rounding error."""
    t = _chw64(x)
    out = torch.zeros_like(t)
    out[:, 1:, :] += (t[:, 1:, :] - t[:, :-1, :]).abs()
    out[:, :-1, :] += (t[:, :-1, :] - t[:, 1:, :]).abs()
    out[:, :, 1:] += (t[:, :, 1:] - t[:, :, :-1]).abs()
    out[:, :, :-1] += (t[:, :, :-1] - t[:, :, 1:]).abs()
    return out
