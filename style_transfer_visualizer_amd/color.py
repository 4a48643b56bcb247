"""Colour preservation (``optimization.preserve_color``): the two controls of Gatys et al. 2017, "Controlling perceptual
factors in neural style transfer", section 5, on the device tensors ``main.style_transfer`` loads and returns.

``match`` - colour statistics matching, before the run.  The style image becomes ``s' = A (s - mu_s) + mu_c`` so that its
per-channel mean and its 3x3 colour covariance are the content image's: ``A = Sigma_c^(1/2) Sigma_s^(-1/2)`` with symmetric
square roots through an eigendecomposition.  Eigenvalues of ``Sigma_s`` at or below ``RANK_CUTOFF * lambda_max`` count as
zero (a pseudo-inverse): a greyscale or constant style image gives a finite, rank-deficient ``A`` and one warning.  The map
is affine per pixel and ImageNet normalisation is a diagonal affine map, so the construction is the same in either space
and is applied in whatever space the tensors are in.

``luma`` - the content image's chrominance restored after the run: ``content_rgb + (Y(result_rgb) - Y(content_rgb))`` with
Rec.601 luminance, in [0, 1] RGB.

The moments (``ops.color_stats``: double partial sums, one launch and one device-to-host copy of 18 KB per image), the
affine map (``ops.color_affine``) and the luminance swap (``ops.luma_transfer``) are HIP kernels; the 3x3 algebra in
between is NumPy float64 on the host.

Not built: row strips (``spatial.py``), a per-frame swap for injected frame sinks (frames show the un-swapped image),
Cholesky or histogram-equalising variants of the match.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .constants import IMAGENET_MEAN, IMAGENET_STD
from .logging_utils import logger

RANK_CUTOFF = 1e-6
# Below this multiple of the mean raw second moment an eigenvalue of ``sum xx / n - mu mu^T`` is the cancellation's own
# rounding (float64 sums over up to 2^28 pixels), not a variance: a constant image has rank 0 whatever its value.
_NOISE_FLOOR = 1e-12

Stats = tuple[int, np.ndarray, np.ndarray]


def statistics(img: torch.Tensor) -> Stats:
    """``(n, sums[3], moments[3, 3])`` of an fp32 image ``[3, H, W]`` or ``[1, 3, H, W]`` on the device: pixel count, per-channel
    sums and the symmetric matrix of raw second moments ``sum x_i x_j``, float64 on the host."""
    rows = ops.color_stats(img.detach().contiguous()).cpu().numpy()
    total = rows.sum(axis=0, dtype=np.float64)
    moments = np.empty((3, 3), dtype=np.float64)
    moments[np.triu_indices(3)] = total[3:]
    moments = np.triu(moments) + np.triu(moments, 1).T
    return int(img.shape[-2]) * int(img.shape[-1]), total[:3].copy(), moments


def _mean_cov(stats: Stats) -> tuple[np.ndarray, np.ndarray, float]:
    n, sums, moments = stats
    mu = np.asarray(sums, dtype=np.float64) / n
    second = np.asarray(moments, dtype=np.float64) / n
    return mu, second - np.outer(mu, mu), _NOISE_FLOOR * float(np.trace(second))


def _matching_transform64(style_stats: Stats, content_stats: Stats) -> tuple[np.ndarray, np.ndarray, int]:
    """``(A, b, rank of Sigma_s)`` in float64."""
    mu_s, cov_s, floor_s = _mean_cov(style_stats)
    mu_c, cov_c, floor_c = _mean_cov(content_stats)
    lam_s, vec_s = np.linalg.eigh(cov_s)
    lam_c, vec_c = np.linalg.eigh(cov_c)
    keep = lam_s > max(RANK_CUTOFF * float(lam_s.max()), floor_s)
    inv_root = np.zeros(3)
    inv_root[keep] = 1.0 / np.sqrt(lam_s[keep])
    root_c = np.sqrt(np.where(lam_c > floor_c, lam_c, 0.0))
    A = ((vec_c * root_c) @ vec_c.T) @ ((vec_s * inv_root) @ vec_s.T)
    return A, mu_c - A @ mu_s, int(keep.sum())


def matching_transform(style_stats: Stats, content_stats: Stats) -> tuple[np.ndarray, np.ndarray]:
    """``(A fp32 [3, 3], b fp32 [3])`` with ``A Sigma_s A^T = Sigma_c`` and ``A mu_s + b = mu_c``, from two results of
    :func:`statistics`.  Pure host arithmetic in float64, rounded at the end; ``b = mu_c - A mu_s`` is formed before the
    rounding.  A rank-deficient ``Sigma_s`` (module docstring) is a warning naming the rank, not an error."""
    A, b, rank = _matching_transform64(style_stats, content_stats)
    if rank < 3:        # noqa: PLR2004
        logger.warning("preserve_color = match: the style image's colour covariance has rank %d of 3 (greyscale or constant "
                       "image?); matching the content's colours along %d direction(s) only", rank, rank)
    return A.astype(np.float32), b.astype(np.float32)


def match_style_to_content(style_img: torch.Tensor, content_img: torch.Tensor) -> torch.Tensor:
    """The style image with the content image's colour mean and covariance: a new tensor, ``style_img`` is not modified."""
    A, b = matching_transform(statistics(style_img), statistics(content_img))
    return ops.color_affine(style_img.detach().contiguous(), [*A.reshape(-1).tolist(), *b.tolist()])


def transfer_luma(result: torch.Tensor, content_img: torch.Tensor, *, normalize: bool) -> torch.Tensor:
    """Luminance of ``result``, chrominance of ``content_img`` (same size; ``normalize``: both are ImageNet-normalised):
    a new tensor in the same space, not clamped."""
    if tuple(result.shape[-2:]) != tuple(content_img.shape[-2:]):
        msg = f"preserve_color = luma: the result is {tuple(result.shape[-2:])}, the content image {tuple(content_img.shape[-2:])}"
        raise ValueError(msg)
    return ops.luma_transfer(result.detach().contiguous(), content_img.detach().contiguous(),
                             mean=IMAGENET_MEAN if normalize else None, std=IMAGENET_STD if normalize else None)
