"""Exactness of stv_avgpool_fwd / stv_avgpool_bwd on a real MI355X: every output equals the fp32 twin (tests/avgpool_ref.py, itself
held to torch's CPU avg_pool2d bit for bit by tests/test_avgpool_host.py) by ``torch.equal``, in fp32 and bf16, through the
direct entry points and through a one-op program, eager and replayed.  Output buffers are pre-filled so that an element the
kernel does not write - or writes where it must not - shows.  Shapes: the smallest maps (one window; odd rows and columns; more
than one vector per pixel; more than one wave), channel counts off the vector width (the scalar kernels), one shape whose work
items are exactly one pass of the capped grid and one just past it.  Non-finite inputs are out of scope."""
from __future__ import annotations

import pytest
import torch

from style_transfer_visualizer_amd import _lib, ops
from tests import avgpool_ref as ref

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
SMALL = [(2, 2, 8), (3, 5, 8), (5, 2, 16), (6, 10, 64),
         (7, 9, 3), (6, 5, 12)]                 # C = 3, 12: the scalar path for both vector widths (bf16 8, fp32 4)
ONE_PASS = _lib.AVGPOOL_MAX_BLOCKS * _lib.AVGPOOL_THREADS


def _big(extra_rows: int, extra_cols: int) -> tuple[int, int, int]:
    """bf16, C = 64 (8 work items per pixel or window): a map whose forward and backward items are exactly one pass of the capped
    grid, enlarged by the given rows and columns."""
    C, Wp = 64, 256
    Hp = ONE_PASS // (C // 8 * Wp)
    assert Hp * Wp * (C // 8) == ONE_PASS
    return 2 * Hp + extra_rows, 2 * Wp + extra_cols, C


EXACT, PAST = _big(0, 0), _big(2, 1)


def _items(H, W, C, vec):
    return (H // 2) * (W // 2) * (C // vec), ((H + 1) // 2) * ((W + 1) // 2) * (C // vec)


def test_launch_constants_match_the_header_and_the_big_shapes_sit_where_they_should():
    assert (_lib.AVGPOOL_THREADS, _lib.AVGPOOL_MAX_BLOCKS) == (256, 2048)
    assert _items(*EXACT, 8) == (ONE_PASS, ONE_PASS)
    f, b = _items(*PAST, 8)
    assert ONE_PASS < f < 2 * ONE_PASS and ONE_PASS < b < 2 * ONE_PASS and PAST[1] % 2 == 1


def _values(shape, dtype, seed, zeros=False):
    """Normal-range random values; ``zeros``: a fifth of them exactly zero (a ReLU mask must see zeros, negatives and positives)."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(*shape, generator=g) * 2
    if zeros:
        v[torch.rand(*shape, generator=g) < 0.2] = 0.0
    return v.to(dtype)


@pytest.mark.parametrize("relu_in", [False, True], ids=["plain", "relu_in"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "x".join(map(str, s)))
def test_forward_equals_the_twin(shape, dtype, relu_in):
    H, W, C = shape
    x = _values(shape, dtype, seed=H * 100 + W * 10 + C, zeros=relu_in)
    want = ref.fwd(x, relu_in=relu_in)
    xd = x.cuda()
    got = ops.avgpool_fwd(xd, relu_in=relu_in)
    assert got.shape == (H // 2, W // 2, C) and got.dtype == dtype
    assert torch.equal(got.cpu(), want)
    assert torch.equal(xd.cpu(), x)                                     # the input is untouched
    out = torch.full_like(got, 77.0)
    assert ops.avgpool_fwd(xd, out=out, relu_in=relu_in) is out and torch.equal(out.cpu(), want)
    if relu_in:
        assert bool((x.float() < 0).any()) and not torch.equal(want, ref.fwd(x))


@pytest.mark.parametrize("accum", [False, True], ids=["write", "accum"])
@pytest.mark.parametrize("mask", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "x".join(map(str, s)))
def test_backward_equals_the_twin(shape, dtype, mask, accum):
    H, W, C = shape
    Hp, Wp = H // 2, W // 2
    dy = _values((Hp, Wp, C), dtype, seed=H + W + C)
    r = _values(shape, dtype, seed=H * W + C, zeros=True) if mask else None
    if mask:
        assert bool((r.float() == 0).any()) and bool((r.float() < 0).any()) and bool((r.float() > 0).any())
    old = _values(shape, dtype, seed=3 * H + W)
    want = ref.bwd(dy, H, W, ref=r, dx=old if accum else None)
    dx = old.cuda() if accum else torch.full(shape, 77.0, dtype=dtype, device="cuda")
    got = ops.avgpool_bwd(dy.cuda(), H, W, ref=r.cuda() if mask else None, out=dx, accumulate=accum)
    assert got is dx and torch.equal(dx.cpu(), want)
    # the rows and columns the floor drops: zeros when written, their old values when accumulated onto
    tails = [dx[2 * Hp:].cpu(), dx[:, 2 * Wp:].cpu()]
    olds = [old[2 * Hp:], old[:, 2 * Wp:]]
    for t, o in zip(tails, olds, strict=True):
        assert torch.equal(t, o) if accum else float(t.float().abs().sum()) == 0.0
    if not accum and not mask:
        fresh = ops.avgpool_bwd(dy.cuda(), H, W)                        # a new tensor by default
        assert torch.equal(fresh.cpu(), want)


def test_bf16_means_on_an_exact_tie_round_to_even_both_ways():
    """Windows whose fp32 mean lies half-way between two bf16 values: three ones and 1 + 2^-6 give 1 + 2^-8, which goes DOWN to 1;
    three times u = 1 + 2^-7 and u + 2^-6 give u + 2^-8, which goes UP to 1 + 2^-6.  The same two ties in the accumulating
    backward: 1 + 0.25 * 2^-6 and u + 0.25 * 2^-6."""
    u = 1.0 + 2.0 ** -7
    x = torch.empty(2, 4, 8)
    x[:, 0:2] = 1.0
    x[1, 1] = 1.0 + 2.0 ** -6
    x[:, 2:4] = u
    x[1, 3] = u + 2.0 ** -6
    x = x.bfloat16()
    assert torch.equal(x.float()[1, 3], torch.full((8,), u + 2.0 ** -6))          # (the operands are bf16 numbers)
    got = ops.avgpool_fwd(x.cuda()).cpu()
    assert torch.equal(got, ref.fwd(x))
    assert torch.equal(got.float(), torch.tensor([1.0, 1.0 + 2.0 ** -6]).view(1, 2, 1).expand(1, 2, 8))
    dy = torch.full((1, 2, 8), 2.0 ** -6).bfloat16()
    dx = torch.empty(2, 4, 8)
    dx[:, 0:2], dx[:, 2:4] = 1.0, u
    dx = dx.bfloat16()
    want = ref.bwd(dy, 2, 4, dx=dx)
    out = ops.avgpool_bwd(dy.cuda(), 2, 4, out=dx.cuda(), accumulate=True).cpu()
    assert torch.equal(out, want)
    assert torch.equal(out.float()[:, 0:2], torch.full((2, 2, 8), 1.0)) and torch.equal(out.float()[:, 2:4], torch.full((2, 2, 8), 1.0 + 2.0 ** -6))


@pytest.mark.parametrize("shape", [EXACT, PAST], ids=["one_pass", "past_one_pass"])
def test_a_grid_at_and_past_its_cap(shape):
    """bf16, C = 64: the items of both kernels equal one pass of the capped grid (STV_AVGPOOL_MAX_BLOCKS x STV_AVGPOOL_THREADS,
    from the header), and exceed it - the stride loop's second trip, with an odd last column and two extra rows."""
    H, W, C = shape
    x = _values(shape, torch.bfloat16, seed=11, zeros=True)
    xd = x.cuda()
    assert torch.equal(ops.avgpool_fwd(xd, relu_in=True).cpu(), ref.fwd(x, relu_in=True))
    dy = _values((H // 2, W // 2, C), torch.bfloat16, seed=12)
    dyd = dy.cuda()
    plain = ops.avgpool_bwd(dyd, H, W, out=torch.full(shape, 77.0, dtype=torch.bfloat16, device="cuda"))
    assert torch.equal(plain.cpu(), ref.bwd(dy, H, W))
    old = _values(shape, torch.bfloat16, seed=13)
    both = ops.avgpool_bwd(dyd, H, W, ref=xd, out=old.cuda(), accumulate=True)
    assert torch.equal(both.cpu(), ref.bwd(dy, H, W, ref=x, dx=old))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_the_executor_ops_run_the_same_kernels(dtype):
    """OP_AVGPOOL_FWD (p0 = x, q0 = y) and OP_AVGPOOL_BWD (p0 = ref, p1 = dy, q0 = dx) through a one-op program each, eager and
    replayed."""
    from style_transfer_visualizer_amd import plan
    H, W, C = 9, 14, 24
    code = ops.dtype_code(dtype)
    x = _values((H, W, C), dtype, seed=1, zeros=True)
    dy = _values((H // 2, W // 2, C), dtype, seed=2)
    old = _values((H, W, C), dtype, seed=3)
    xd, dyd = x.cuda(), dy.cuda()
    y = torch.empty(H // 2, W // 2, C, dtype=dtype, device="cuda")
    dx = torch.empty(H, W, C, dtype=dtype, device="cuda")
    f = _lib.StvOp()
    f.op, f.dtype, f.flags, f.H, f.W, f.cin = _lib.OP_AVGPOOL_FWD, code, _lib.RELU_IN, H, W, C
    f.p0, f.q0 = xd.data_ptr(), y.data_ptr()
    b = _lib.StvOp()
    b.op, b.dtype, b.flags, b.H, b.W, b.cin = _lib.OP_AVGPOOL_BWD, code, _lib.MASK | _lib.ACCUM, H, W, C
    b.p0, b.p1, b.q0 = xd.data_ptr(), dyd.data_ptr(), dx.data_ptr()
    fwd, bwd = plan.Program([f], extra=(xd, y)), plan.Program([b], extra=(xd, dyd, dx))
    want_y, want_dx = ref.fwd(x, relu_in=True), ref.bwd(dy, H, W, ref=x, dx=old)
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        for _ in range(3):              # eager warm-up + capture, then two replays
            y.fill_(77.0)
            dx.copy_(old)
            fwd.run(use_graph=True)
            bwd.run(use_graph=True)
            torch.cuda.current_stream().synchronize()
            assert torch.equal(y.cpu(), want_y) and torch.equal(dx.cpu(), want_dx)
    # without STV_MASK the op's p0 may stay unset
    b2 = _lib.StvOp()
    b2.op, b2.dtype, b2.flags, b2.H, b2.W, b2.cin = _lib.OP_AVGPOOL_BWD, code, 0, H, W, C
    b2.p1, b2.q0 = dyd.data_ptr(), dx.data_ptr()
    plan.Program([b2], extra=(dyd, dx)).run()
    torch.cuda.synchronize()
    assert torch.equal(dx.cpu(), ref.bwd(dy, H, W))


def test_refusals_on_the_device():
    x = torch.zeros(4, 4, 8, device="cuda")
    y = torch.zeros(2, 2, 8, device="cuda")
    lib = _lib.load()
    assert lib.stv_avgpool_fwd(x.data_ptr(), y.data_ptr(), 4, 4, 8, 0, _lib.STV_BF16X3, None) == 1
    assert lib.stv_avgpool_bwd(None, y.data_ptr(), x.data_ptr(), 4, 4, 8, _lib.MASK, _lib.STV_F32, None) == 1
    assert lib.stv_avgpool_fwd(x.data_ptr(), y.data_ptr(), 4, 4, 8, _lib.RELU_OUT, _lib.STV_F32, None) == 1
    with pytest.raises(RuntimeError, match="accumulate=True needs"):
        ops.avgpool_bwd(y, 4, 4, accumulate=True)
    with pytest.raises(RuntimeError, match="dy is"):
        ops.avgpool_bwd(y, 6, 4)
    with pytest.raises(RuntimeError, match="STV_ERR_ARG"):
        ops.avgpool_fwd(torch.zeros(1, 4, 8, device="cuda"))
