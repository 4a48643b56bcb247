"""Average pooling (``--pooling avg``), test infrastructure only.

* An fp32 NumPy twin of ``stv_avgpool_fwd`` / ``stv_avgpool_bwd`` (csrc/avgpool.hip), operation for operation: every sum is one
  fp32 addition in the kernel's order, the result is rounded once to the storage type (bf16 through ``tests.layerwise.round_to``).
  Tensors are NHWC ``[H, W, C]`` torch tensors of fp32 or bf16, as the kernels see them.
* The definition of the average-pooling step in plain differentiable torch (float64 when its inputs are): the conv stack with
  ``F.avg_pool2d`` in place of every pool, the project's Gram (clamp, then ``/ (C*H*W)``), MSE, autograd for the gradient.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import core_model_ref as ocm
from tests.layerwise import round_to

CLAMP = ocm.GRAM_CLAMP_MAX


# ------------------------------------------------------------------------------------------------ the kernels' twin
def _f32(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().float().numpy().astype(np.float32)


def _store(v: np.ndarray, dtype: torch.dtype) -> torch.Tensor:
    """fp32 values -> the storage type, rounded to nearest even."""
    assert v.dtype == np.float32
    return round_to(torch.from_numpy(np.ascontiguousarray(v)).double(), dtype).to(dtype)


def fwd(x: torch.Tensor, relu_in: bool = False) -> torch.Tensor:
    """``y[i,j] = (((x[2i,2j] + x[2i,2j+1]) + x[2i+1,2j]) + x[2i+1,2j+1]) * 0.25f``, each operand ``max(0, .)`` first with
    ``relu_in``."""
    H, W, _ = x.shape
    Hp, Wp = H // 2, W // 2
    v = _f32(x)
    if relu_in:
        v = np.maximum(v, np.float32(0))
    a, b = v[0:2 * Hp:2, 0:2 * Wp:2], v[0:2 * Hp:2, 1:2 * Wp:2]
    c, d = v[1:2 * Hp:2, 0:2 * Wp:2], v[1:2 * Hp:2, 1:2 * Wp:2]
    s = (a + b).astype(np.float32)
    s = (s + c).astype(np.float32)
    s = (s + d).astype(np.float32)
    return _store((s * np.float32(0.25)).astype(np.float32), x.dtype)


def bwd(dy: torch.Tensor, H: int, W: int, ref: torch.Tensor | None = None, dx: torch.Tensor | None = None) -> torch.Tensor:
    """``v = 0.25f * dy[y/2, x/2]`` inside ``2*Hp x 2*Wp``, else 0; ``ref``: ``v = 0`` where ``!(ref > 0)``; ``dx`` given (the
    accumulating form): ``dx + v`` in fp32 inside the pooled range, ``dx`` itself in the rows and columns the floor drops."""
    Hp, Wp, C = dy.shape
    assert (Hp, Wp) == (H // 2, W // 2)
    v = np.zeros((H, W, C), np.float32)
    g = (np.float32(0.25) * _f32(dy)).astype(np.float32)
    v[:2 * Hp, :2 * Wp] = np.repeat(np.repeat(g, 2, axis=0), 2, axis=1)
    if ref is not None:
        v = np.where(_f32(ref) > 0, v, np.float32(0)).astype(np.float32)
    if dx is None:
        return _store(v, dy.dtype)
    out = dx.detach().cpu().clone()
    old = _f32(dx)[:2 * Hp, :2 * Wp]
    out[:2 * Hp, :2 * Wp] = _store((old + v[:2 * Hp, :2 * Wp]).astype(np.float32), dy.dtype)
    return out


# ------------------------------------------------------------------------------------------------ the step's definition
def program(weights, cfg) -> list:
    """``oracle.core_model_ref.vgg_program`` with every pool an average pool."""
    return [("avgpool",) if layer[0] == "pool" else layer for layer in ocm.vgg_program(weights, cfg)]


def to_dtype(prog: list, dtype: torch.dtype) -> list:
    return [("conv", layer[1].to(dtype), layer[2].to(dtype)) if layer[0] == "conv" else layer for layer in prog]


def features(prog: list, x: torch.Tensor, taps) -> dict:
    """The output of every layer index in ``taps``."""
    out, last = {}, max(taps)
    for i, layer in enumerate(prog[:last + 1]):
        x = F.avg_pool2d(x, kernel_size=2, stride=2) if layer[0] == "avgpool" else ocm.run_layer(layer, x)
        if i in taps:
            out[i] = x
    return out


def gram(f: torch.Tensor) -> torch.Tensor:
    return ocm.gram_matrix(f, CLAMP)


class Reference:
    """Targets and losses of the average-pooling step for one (program, style layers, content layers)."""

    def __init__(self, prog: list, style_at, content_at) -> None:
        self.prog, self.style_at, self.content_at = prog, sorted(set(style_at)), sorted(set(content_at))
        self.taps = set(self.style_at) | set(self.content_at)

    def locked(self, decisions: dict) -> "Reference":
        """A copy that evaluates on the piecewise-linear branch another path took: its ReLUs are the given masks
        (``tests.parity_util.hip_decisions``; an average pool takes no decision).  Targets stay as captured."""
        other = Reference(list(self.prog), self.style_at, self.content_at)
        for li, d in decisions.items():
            if li < len(other.prog) and other.prog[li][0] == "relu" and d[0] == "relu_mask":
                other.prog[li] = d
        other.style_targets, other.content_targets = self.style_targets, self.content_targets
        return other

    def set_targets(self, style_img: torch.Tensor, content_img: torch.Tensor) -> None:
        with torch.no_grad():
            sf = features(self.prog, style_img, self.taps)
            cf = features(self.prog, content_img, self.taps)
        self.style_targets = [gram(sf[i]) for i in self.style_at]
        self.content_targets = [cf[i] for i in self.content_at]

    def losses(self, x: torch.Tensor) -> tuple[list, list]:
        f = features(self.prog, x, self.taps)
        return ([F.mse_loss(gram(f[i]), t) for i, t in zip(self.style_at, self.style_targets, strict=True)],
                [F.mse_loss(f[i], t) for i, t in zip(self.content_at, self.content_targets, strict=True)])

    def loss_and_grad(self, x: torch.Tensor, style_w: float, content_w: float):
        """(style score, content score, total, gradient) at ``x``."""
        xg = x.detach().clone().requires_grad_(True)
        s, c = self.losses(xg)
        style, content = torch.stack(s).sum(), torch.stack(c).sum()
        total = style_w * style + content_w * content
        (grad,) = torch.autograd.grad(total, xg)
        return style.detach(), content.detach(), total.detach(), grad
