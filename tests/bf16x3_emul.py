"""CPU emulation of the bf16x3 split (STV_BF16X3) for the tests: float64 evaluation of ah*bh + ah*bl + al*bh.

hi = bf16_rne(x), lo = bf16_rne(x - hi) (x - hi exact in fp32), lo = 0 where hi is not finite - the kernels' rule
(csrc/conv_igemm_kernel.h split4, csrc/gram.hip split_word).
"""
from __future__ import annotations

import numpy as np
import torch


def split(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """fp32 tensor -> (hi, lo) as float64 tensors holding the bf16 values."""
    x = x.detach().float().cpu()
    hi = x.to(torch.bfloat16).float()
    with np.errstate(invalid="ignore", over="ignore"):
        r = torch.where(torch.isfinite(hi), x - hi, torch.zeros_like(x))
    lo = r.to(torch.bfloat16).float()
    return hi.double(), lo.double()


def product3(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Elementwise ah*bh + ah*bl + al*bh in float64."""
    ah, al = split(a)
    bh, bl = split(b)
    return ah * bh + ah * bl + al * bh


def conv3x3(x_hwc: torch.Tensor, w: torch.Tensor, *, relu_in: bool = False, exact: bool = False) -> torch.Tensor:
    """NHWC x [H,W,Cin] fp32, w [Cout,Cin,3,3] fp32 -> float64 [H,W,Cout]: the split conv (or exact float64)."""
    x = x_hwc.detach().float().cpu()
    if relu_in:
        x = x.clamp_min(0.0)
    xw = x.permute(2, 0, 1)[None]
    if exact:
        return torch.nn.functional.conv2d(xw.double(), w.detach().double().cpu(), padding=1)[0].permute(1, 2, 0)
    xh, xl = split(xw)
    wh, wl = split(w)
    f = torch.nn.functional.conv2d
    y = f(xh, wh, padding=1) + f(xh, wl, padding=1) + f(xl, wh, padding=1)
    return y[0].permute(1, 2, 0)


def gram(F_nc: torch.Tensor, *, exact: bool = False) -> torch.Tensor:
    """F [N,C] fp32 -> F^T F in float64 (split products, or exact)."""
    if exact:
        f = F_nc.detach().double().cpu()
        return f.T @ f
    h, lo = split(F_nc)
    return h.T @ h + h.T @ lo + lo.T @ h
