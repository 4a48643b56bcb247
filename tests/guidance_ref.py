"""The definition of the guided style term in plain differentiable torch (float64 when its inputs are), on the feature maps of
the CPU oracle (``oracle.core_model_ref``: ``vgg_program``, ``OracleModel``), for the GPU tests of the guided step:

    F_{l,r}[p,:] = F_l[p,:] if m_l[p] == r, else 0
    n_{l,r}      = #{p : m_l[p] == r}
    G_{l,r}      = min(F_{l,r}^T F_{l,r}, clamp) / (C_l * n_{l,r})
    loss_{l,r}   = mse(G_{l,r}(x), G_{l,r}(style))          the style's Grams from the style image's own label map and counts
    style score  = sum_l w_l * sum_r lambda_r * loss_{l,r}

``m_l`` is the image-size label map resampled to the tap's size by ``guidance.resample_labels``.  Test infrastructure only.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import core_model_ref as ocm
from style_transfer_visualizer_amd import guidance

CLAMP = ocm.GRAM_CLAMP_MAX


def region_gram(f: torch.Tensor, labels: torch.Tensor, r: int) -> torch.Tensor:
    """``G_{l,r}`` of the features ``f`` ``[1, C, H, W]`` under the image-size label map ``labels``."""
    _, C, H, W = f.shape
    m = guidance.resample_labels(labels, H, W) == r
    n = int(m.sum())
    assert n > 0
    fr = (f * m.to(f.dtype)).reshape(C, H * W)
    return torch.mm(fr, fr.t()).clamp(max=CLAMP) / float(C * n)


def style_features(oracle: ocm.OracleModel, img: torch.Tensor) -> list[torch.Tensor]:
    feats = oracle._features(img)
    return [feats[j] for j in oracle.style_ids]


def guided_targets(oracle: ocm.OracleModel, style_img: torch.Tensor, style_labels: torch.Tensor, regions: int) -> list[list[torch.Tensor]]:
    with torch.no_grad():
        return [[region_gram(f, style_labels, r) for r in range(regions)] for f in style_features(oracle, style_img)]


def loss_and_grad(oracle: ocm.OracleModel, x: torch.Tensor, content_labels: torch.Tensor, targets: list[list[torch.Tensor]],
                  style_w: float, content_w: float, *, region_w=None, layer_w=None):
    """(region losses ``[L, R]``, style score, content score, total, gradient) at ``x``; ``oracle`` holds the content targets
    (``set_targets``) and, where it was locked (``tests/parity_util.lock``), another path's ReLU and pool decisions."""
    regions = len(targets[0])
    region_w = [1.0] * regions if region_w is None else list(region_w)
    layer_w = [1.0] * len(targets) if layer_w is None else list(layer_w)
    xg = x.detach().clone().requires_grad_(True)
    feats = oracle._features(xg)
    rows = []
    for l, j in enumerate(oracle.style_ids):
        rows.append(torch.stack([F.mse_loss(region_gram(feats[j], content_labels, r), targets[l][r]) for r in range(regions)]))
    losses = torch.stack(rows)
    style = sum(layer_w[l] * sum(region_w[r] * losses[l, r] for r in range(regions)) for l in range(len(targets)))
    content = sum(F.mse_loss(feats[j], oracle.content_targets[k]) for k, j in enumerate(oracle.content_ids))
    total = style_w * style + content_w * content
    (grad,) = torch.autograd.grad(total, xg)
    return losses.detach(), style.detach(), content.detach(), total.detach(), grad
