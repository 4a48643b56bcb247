"""Exactness of stv_mask_split on a real MI355X: every slab element holds the bits of its source or the bits of +0, compared on
integer views against a ``torch.where`` twin.  Inputs contain NaN (with payloads) and -0; output buffers are pre-filled with NaN
so that an element the kernel does not write shows.  The shapes cover both element sizes, the vector path with 1, 3, 8 and 64
vectors per pixel, pixels that straddle waves, the scalar path (a row that is no multiple of 16 bytes; an ``out`` base offset
by 4 bytes), and one shape just past one pass of the capped grid."""
from __future__ import annotations

import pytest
import torch

from style_transfer_visualizer_amd import _lib, ops

pytestmark = pytest.mark.gpu

NO_REGION = 255
# (n_pixels, C, dtype)
SHAPES = [
    (5 * 7, 64, torch.bfloat16),
    (33 * 50, 24, torch.bfloat16),          # 3 vectors per pixel: pixels straddle waves
    (6, 512, torch.bfloat16),
    (35, 3, torch.float32),                 # a 12-byte row: the scalar path
    (48 * 80, 36, torch.float32),
    (96 * 96, 256, torch.bfloat16),         # 294,912 items: just past one pass of 1,024 x 256
]


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _features(n: int, C: int, dtype: torch.dtype, seed: int) -> torch.Tensor:
    """Random features with NaNs of several payloads, -0, +0 and infinities sprinkled in (built on integer bits)."""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(n, C, generator=g).to(dtype)
    bits = _bits(f).clone()
    kind = torch.randint(0, 16, (n, C), generator=g)
    if dtype == torch.bfloat16:
        special = {0: 0x7FC1, 1: -32768, 2: 0, 3: 0x7F80, 4: -63}     # NaN with a payload, -0, +0, +inf, a negative NaN (0xFFC1)
        for k, v in special.items():
            bits[kind == k] = v
    else:
        special = {0: 0x7FC00001, 1: -2147483648, 2: 0, 3: 0x7F800000, 4: -4194303}      # the same; 0xFFC00001
        for k, v in special.items():
            bits[kind == k] = v
    return bits.view(dtype).cuda()


def _twin(F: torch.Tensor, labels: torch.Tensor, R: int) -> torch.Tensor:
    """[R, n, C] integer bits: the source's bits where the pixel carries the slab's label, 0 (the bits of +0) elsewhere."""
    b = _bits(F)
    return torch.stack([torch.where((labels == r).unsqueeze(1), b, torch.zeros_like(b)) for r in range(R)])


def _labels(n: int, R: int, how: str, seed: int) -> torch.Tensor:
    if how == "random":
        g = torch.Generator().manual_seed(seed)
        lab = torch.randint(0, R, (n,), generator=g).to(torch.uint8)
        lab[torch.rand(n, generator=g) < 0.2] = NO_REGION
        return lab.cuda()
    return torch.full((n,), R - 1, dtype=torch.uint8).cuda()      # all one value: the last slab is F, the others zero


def test_launch_constants_match_the_header():
    assert (_lib.MASK_MAX_REGIONS, _lib.MASK_SPLIT_THREADS, _lib.MASK_SPLIT_MAX_BLOCKS) == (4, 256, 1024)
    n, C, _ = SHAPES[-1]
    items = n * C * 2 // 16
    one_pass = _lib.MASK_SPLIT_MAX_BLOCKS * _lib.MASK_SPLIT_THREADS
    assert one_pass < items < 2 * one_pass


@pytest.mark.parametrize("how", ["random", "one_value"])
@pytest.mark.parametrize("R", [1, 2, 3, 4])
@pytest.mark.parametrize("n,C,dtype", SHAPES)
def test_slabs_hold_the_bits_of_the_source_or_zero(n, C, dtype, R, how):
    F = _features(n, C, dtype, seed=n + C)
    labels = _labels(n, R, how, seed=R)
    out = torch.full((R, n, C), float("nan"), dtype=dtype, device="cuda")
    got = ops.mask_split(F, labels, R, out=out)
    assert got is out
    assert torch.equal(_bits(out), _twin(F, labels, R))
    assert torch.equal(_bits(F), _bits(_features(n, C, dtype, seed=n + C)))      # the input is untouched


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("n,C,dtype", [(5 * 7, 64, torch.bfloat16), (48 * 80, 36, torch.float32)])
def test_an_out_base_offset_by_four_bytes_takes_the_unaligned_path(n, C, dtype, R):
    """Rows of a multiple of 16 bytes behind an ``out`` that starts 4 bytes past a 16-byte boundary; the bytes in front of
    and behind the slabs keep their fill."""
    es = 2 if dtype == torch.bfloat16 else 4
    pad = 4 // es
    F = _features(n, C, dtype, seed=7)
    labels = _labels(n, R, "random", seed=5)
    store = torch.full((R * n * C + 2 * pad + 16,), float("nan"), dtype=dtype, device="cuda")
    assert store.data_ptr() % 16 == 0
    out = store[pad:pad + R * n * C].view(R, n, C)
    assert out.data_ptr() % 16 == 4
    ops.mask_split(F, labels, R, out=out)
    assert torch.equal(_bits(out), _twin(F, labels, R))
    fill = _bits(torch.full((1,), float("nan"), dtype=dtype))[0].item()
    assert (_bits(store[:pad]) == fill).all() and (_bits(store[pad + R * n * C:]) == fill).all()


def test_the_executor_op_runs_the_same_kernel():
    """OP_MASK_SPLIT through a program (p0 = F, p1 = labels, q0 = out, n = n_pixels, cin = C, cout = R), eager and replayed."""
    from style_transfer_visualizer_amd import plan
    n, C, R = 33 * 50, 24, 3
    F = _features(n, C, torch.bfloat16, seed=1)
    labels = _labels(n, R, "random", seed=2)
    out = torch.full((R, n, C), float("nan"), dtype=torch.bfloat16, device="cuda")
    op = _lib.StvOp()
    op.op, op.dtype, op.n, op.cin, op.cout = _lib.OP_MASK_SPLIT, _lib.STV_BF16, n, C, R
    op.p0, op.p1, op.q0 = F.data_ptr(), labels.data_ptr(), out.data_ptr()
    prog = plan.Program([op], extra=(F, labels, out))
    want = _twin(F, labels, R)
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        for _ in range(3):              # eager warm-up + capture, then two replays
            out.fill_(float("nan"))
            prog.run(use_graph=True)
            torch.cuda.current_stream().synchronize()
            assert torch.equal(_bits(out), want)


def test_refusals_on_the_device():
    F = torch.zeros(8, 16, device="cuda")
    labels = torch.zeros(8, dtype=torch.uint8, device="cuda")
    lib = _lib.load()
    out = torch.zeros(2, 8, 16, device="cuda")
    assert lib.stv_mask_split(F.data_ptr(), labels.data_ptr(), out.data_ptr(), 8, 16, 2, _lib.STV_BF16X3, None) == 1
    assert lib.stv_mask_split(F.data_ptr(), labels.data_ptr(), F.data_ptr(), 8, 16, 1, _lib.STV_F32, None) == 1       # out == F
    both = torch.zeros(3, 8, 16, device="cuda")
    assert lib.stv_mask_split(both[2].data_ptr(), labels.data_ptr(), both.data_ptr(), 8, 16, 3, _lib.STV_F32, None) == 1
    with pytest.raises(RuntimeError, match="labels"):
        ops.mask_split(F, labels[:7], 2)
