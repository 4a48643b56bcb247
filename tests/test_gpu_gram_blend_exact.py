"""``stv_gram_blend`` against its NumPy fp32 twin (tests/blend_ref.py), bit for bit.

Sizes: 1 and 3 are the scalar tail alone, 4 is one vector item, 65*65 has a tail behind 1056 items and tables that do not
start on a 16-byte boundary, 64*64 is the aligned vector path, 512*512 (the largest Gram matrix of VGG19) sends the capped
grid through its loop twice - asserted from the launch constants the library documents.  Tables are random normals scaled
to Gram magnitudes with zeros, negatives and a subnormal planted; the weights hold an exact 0 and an exact 1 where K allows;
``out`` is pre-filled with NaN, so an element that is not written shows.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from style_transfer_visualizer_amd import _lib, ops
from tests import blend_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SIZES = [1, 3, 4, 65 * 65, 64 * 64, 512 * 512]
WEIGHTS = {1: [1.0], 2: [0.7, 0.3], 3: [1.0, 0.0, 0.25], 8: [0.0, 1.0, 0.125, 0.3, 0.05, 0.2, 0.075, 0.25]}


def _stack(K: int, n: int) -> np.ndarray:
    rng = np.random.default_rng(1000 * K + n % 997)
    stack = (rng.standard_normal((K, n)) * 3e-3).astype(np.float32)
    flat = stack.reshape(-1)
    flat[:: 7] = 0.0
    flat[K * n // 2] = np.float32(1e-41)                  # a subnormal
    flat[-1] = np.float32(-2.5e-3)
    return stack


def test_the_largest_size_takes_the_grid_through_its_loop_more_than_once():
    per_pass = _lib.BLEND_MAX_BLOCKS * _lib.BLEND_THREADS
    assert max(SIZES) // _lib.BLEND_VEC > per_pass, "pick a larger n: one pass of the capped grid covers it"
    assert all(n // _lib.BLEND_VEC <= per_pass for n in SIZES[:-1])


@pytest.mark.parametrize("K", sorted(WEIGHTS))
@pytest.mark.parametrize("n", SIZES)
def test_kernel_equals_the_twin(n, K):
    stack = _stack(K, n)
    w = np.asarray(WEIGHTS[K], dtype=np.float32)
    want = torch.from_numpy(blend_ref.blend(stack, w))
    out = torch.full((n,), float("nan"), device=DEV)
    got = ops.gram_blend(torch.from_numpy(stack).to(DEV), w.tolist(), out=out)
    assert got is out
    got = got.cpu()
    assert not torch.isnan(got).any(), "an element was not written"
    assert torch.equal(got, want), f"n={n} K={K}: {int((got != want).sum())} elements differ"
    if K == 1:
        assert torch.equal(got, torch.from_numpy(stack[0]))            # weight 1: the table itself


def test_a_stack_that_does_not_start_on_a_16_byte_boundary():
    """A view one float into an allocation: the walk with 4-byte aligned accesses, same bits."""
    K, n = 3, 64 * 64
    stack = _stack(K, n)
    w = WEIGHTS[K]
    base = torch.zeros(K * n + 1, device=DEV)
    base[1:].copy_(torch.from_numpy(stack).reshape(-1))
    view = base[1:].view(K, n)
    assert view.data_ptr() % 16 == 4
    got = ops.gram_blend(view, w, out=torch.full((n,), float("nan"), device=DEV)).cpu()
    assert torch.equal(got, torch.from_numpy(blend_ref.blend(stack, w)))


def test_shapes_and_refusals():
    stack = torch.from_numpy(_stack(2, 64)).to(DEV).view(2, 8, 8)
    assert tuple(ops.gram_blend(stack, [0.5, 0.5]).shape) == (8, 8)
    with pytest.raises(RuntimeError, match="weights"):
        ops.gram_blend(stack, [1.0])
    with pytest.raises(RuntimeError, match="STV_ERR_ARG"):
        ops.gram_blend(stack, [0.5, -0.5])
    with pytest.raises(RuntimeError, match="STV_ERR_ARG"):
        ops.gram_blend(stack, [0.5, float("nan")])
    with pytest.raises(RuntimeError, match="STV_ERR_ARG"):
        ops.gram_blend(stack, [0.5, 0.5], out=stack[1])               # out inside the stack
    nine = torch.zeros(9, 16, device=DEV)
    with pytest.raises(RuntimeError, match="STV_ERR_ARG"):
        ops.gram_blend(nine, [1.0] * 9)
