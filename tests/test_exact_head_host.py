"""The exact-operand method for the loss head (tests/exact_head.py) checked without a GPU: every generator's own
preconditions hold for every case the GPU tests run, the references are what a direct float64 torch evaluation gives,
the case lists reach the code paths they are meant to reach under the launch constants copied from csrc, and a finish
kernel with one of three small faults would not produce the expected tensors."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import core_model_ref as ocm

from . import exact_head as eh
from . import exact_ints as ei

_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)      # noqa: E731


@pytest.mark.parametrize("kind", eh.CLAMP_KINDS)
@pytest.mark.parametrize("nc", eh.FINISH_CASES, ids=_ids)
def test_finish_generators_hold_and_match_autograd(nc, kind):
    """Budgets, power-of-two factors, the asymmetric delta and the tie are asserted by the generator itself; the
    reference is gram_matrix + mse_loss + autograd in float64 on the same operands (the seed is 2 dLoss/dR * coef:
    dF = (dR + dR^T) F = 2 dR F for the symmetric targets of a real run)."""
    n, C = nc
    c = eh.finish_case(n, C, kind)
    assert eh.is_pow2(c["norm"]) and c["ks"] == eh.gram_ksplit(n, C) and c["slabs"].shape == (c["ks"], C, C)
    held = ei.held_pairs(C)
    assert torch.equal(c["slabs"].double()[:, held].sum(0), c["R"][held]) and bool(c["slabs"][:, ~held].isnan().all())
    if kind == "tie":
        assert c["tie"] > 0 and c["cut"] > 0
    elif kind == "above":
        assert c["cut"] == 0
    else:
        assert c["cut"] > 0
    f4 = c["f"].double().t().reshape(1, C, 1, n)
    R = (f4.reshape(C, n) @ f4.reshape(C, n).t()).requires_grad_(True)
    if c["norm"] == float(C * n):
        assert torch.equal(ocm.gram_matrix(f4, c["clamp"]), c["gram"].double())
    G = R.clamp(max=c["clamp"]) / c["norm"]
    assert torch.equal(G.detach(), c["gram"].double())
    loss = F.mse_loss(G, c["target"].double(), reduction="sum")
    assert float(loss.detach()) == float(c["loss"])
    (c["coef"] * loss / (C * C)).backward()
    k = eh.k_grad(c["coef"], C, c["norm"])
    for dtype in eh.DTYPES:
        assert torch.equal(eh.seed_of(c, dtype).double(), 2.0 * R.grad)
        assert torch.equal(eh.seed_of(c, dtype, 0.5).double(), R.grad)
    m = eh.finish_model(c["slabs"], c["target"], C, c["clamp"], c["norm"], k)
    assert torch.equal(m["gram"], c["gram"].double()) and float(m["loss"]) == float(c["loss"])
    assert torch.equal(m["seed"], 2.0 * R.grad)


def test_other_finish_generators_hold():
    for n, C in eh.FINISH_CASES:
        assert torch.equal(eh.raw_case(n, C)["gram"].double(), eh.gram_operands(n, C)["R"])
    for C in eh.SPATIAL_C:
        for kind in eh.CLAMP_KINDS:
            c = eh.spatial_case(C, kind)
            assert c["slabs"].shape == (1, C, C) and eh.is_pow2(c["norm"]) and c["n"] == 1
            eh.seed_of(c, torch.bfloat16)
    for prec in ("fp32", "bf16"):
        for kind in eh.CLAMP_KINDS:
            m = eh.multi_case(prec, kind)
            assert len(m["taps"]) == 5 and {ei.gram_tile(t["C"]) for t in m["taps"]} == {64, 128}
            assert max(t["ks"] for t in m["taps"]) >= 33
            for t in m["taps"]:
                eh.seed_of(t, ei.storage_dtype(prec), 0.25)
    for kind in eh.CLAMP_KINDS:
        eh.finish_case(*eh.ABSENT_CASE, kind)
    H, W, C = eh.CHAIN_STYLE
    assert eh.is_pow2(C * H * W) and eh.is_pow2(eh.CHAIN_CONTENT_N)


def test_finish_cases_reach_every_ksplit_class_and_both_variants():
    ks = [eh.gram_ksplit(n, C) for n, C in eh.SINGLE_TAP]
    assert ks == [*eh.KSPLIT_LADDER, 128]
    assert {eh.finish_slices(k) for k in ks} == {eh.FIN_S_SHORT, eh.FIN_S_DEEP}
    assert eh.finish_slices(127) == eh.FIN_S_SHORT and eh.finish_slices(128) == eh.FIN_S_DEEP
    walks = {k: {eh.finish_walk(k, eh.finish_slices(k), s) for s in range(eh.finish_slices(k))} for k in (*ks, 24, 25)}
    # (trips through the unrolled loop, slabs added by its remainder code) over the slices of one element.  Fewer slabs
    # than slices, exactly as many, one more:
    assert walks[1] == {(0, 1), (0, 0)} and walks[7] == {(0, 1), (0, 0)} and walks[8] == {(0, 1)} and walks[9] == {(0, 2), (0, 1)}
    # the unrolled loop of the 8-slice variant starts at ksplit = 25 (slice 0); at 31 one slice is still without it, at
    # 32 every slice runs it once and the remainder code adds nothing, at 33 it adds one slab
    assert walks[24] == {(0, 3)} and walks[25] == {(1, 0), (0, 3)}
    assert walks[31] == {(1, 0), (0, 3)} and walks[32] == {(1, 0)} and walks[33] == {(1, 1), (1, 0)} and walks[64] == {(2, 0)}
    assert walks[127] == {(4, 0), (3, 3)}
    # the 32-slice variant: once without a remainder, once with one, several times
    assert walks[128] == {(1, 0)} and walks[160] == {(1, 1)} and walks[512] == {(4, 0)}
    for C in eh.MIRROR_C:
        small = [eh.gram_ksplit(n, c) for n, c in eh.MIRROR if c == C]
        assert any(1 < k < 25 for k in small), C
        assert C == 512 or any(k >= 33 for k in small), C
    assert any(C > 128 and eh.gram_ksplit(n, C) >= 33 for n, C in eh.MIRROR), "a mirrored matrix on the unrolled loop"
    assert {C * C % eh.FIN_E != 0 for _, C in eh.MIRROR} == {True, False}
    assert [eh.gram_ksplit(H * W, C) for H, W, C in eh.MULTI_TAPS] == [2, 1, 64, 1, 16]


def test_a_wrong_finish_does_not_give_the_expected_tensors():
    """Three faults the tests are written for, each on the CPU model of the kernel: the expected tensors move."""
    n, C = 777, 256
    c = eh.finish_case(n, C, "tie")
    k = eh.k_grad(c["coef"], C, c["norm"])
    args = (c["slabs"], c["target"], C, c["clamp"], c["norm"], k)
    good = eh.finish_model(*args)
    want_seed = eh.seed_of(c, torch.float32).double()
    assert torch.equal(good["seed"], want_seed)
    bad = eh.finish_model(*args, fault="mirror_row")
    assert torch.equal(bad["gram"], good["gram"]) and float(bad["loss"]) != float(c["loss"])
    assert int((bad["seed"] != want_seed).sum()) > 0 and int((bad["seed"].bfloat16() != eh.seed_of(c, torch.bfloat16)).sum()) > 0
    # ... and inside the existing tolerance of the loss (rel 1e-4) such a fault on ONE element would pass
    bad = eh.finish_model(*args, fault="strict_mask")
    assert float(bad["loss"]) == float(c["loss"]) and int((bad["seed"] != want_seed).sum()) == c["tie"]
    bad = eh.finish_model(*args, fault="drop_slab")
    assert not torch.equal(bad["gram"], good["gram"])
    # the ragged single-tile matrices see the two faults that need no mirror
    c = eh.finish_case(777, 100, "tie")
    args = (c["slabs"], c["target"], 100, c["clamp"], c["norm"], eh.k_grad(c["coef"], 100, c["norm"]))
    assert int((eh.finish_model(*args, fault="strict_mask")["seed"] != eh.seed_of(c, torch.float32).double()).sum()) == c["tie"]
    assert not torch.equal(eh.finish_model(*args, fault="drop_slab")["gram"], c["gram"].double())


@pytest.mark.parametrize("dtype", eh.DTYPES, ids=str)
def test_content_cases_hold_and_take_the_trips_they_are_listed_for(dtype):
    sizes = eh.content_sizes(dtype, grad=True)
    for n in sizes:
        c = eh.content_case(n)
        fr = c["f"].double().requires_grad_(True)
        loss = F.mse_loss(fr, c["t"].double(), reduction="sum")
        assert float(loss.detach()) == float(c["loss"])
        (loss / n).backward()
        if eh.is_pow2(n):
            k = eh.content_k(8.0, n)
            assert eh.is_pow2(k) and torch.equal(eh.stored(k * c["d"], dtype).double(), 8.0 * fr.grad)
            k = eh.content_k(n / 8.0, n, 0.5)
            assert k == 0.125 and torch.equal(eh.stored(k * c["d"] + c["prev"].double(), dtype).double(),
                                              n / 16.0 * fr.grad + c["prev"].double())
        assert bool((c["prev"].double() * c["d"] >= 0).all()), "accumulating must not cancel"
    loss_sizes = eh.content_sizes(dtype)
    assert max(eh.content_loss_trips(n, dtype) for n in loss_sizes[:-1]) == 1
    assert eh.content_loss_trips(loss_sizes[-1], dtype) == 2 and loss_sizes[-1] % eh.k_vec(dtype)
    assert eh.content_grad_trips(sizes[-1], dtype) == 2 and max(eh.content_grad_trips(n, dtype) for n in sizes[:-1]) == 1
    if dtype == torch.float32:      # the sizes the issue lists are the first second trips of the fp32 kernels
        assert eh.content_loss_trips((1 << 20) + 3, dtype) == 1 and eh.content_grad_trips((1 << 21) + 3, dtype) == 1
    assert 4 * max(loss_sizes) < eh.LIMIT


def test_content_bounds_see_an_indexing_error():
    """Ragged n: a value that belongs to the neighbouring element is off by a whole k or more, far outside the bound."""
    n = 4099
    c = eh.content_case(n)
    for dtype in eh.DTYPES:
        want = 8.0 * 2.0 / n * c["d"]
        centre, bound = eh.content_grad_bounds(want, dtype)
        shifted = torch.roll(want, 1)
        moved = (shifted - want).abs() > 0
        assert float(moved.double().mean()) > 0.5 and bool(((shifted - centre).abs() > bound)[moved].all())
        assert float(bound.max()) <= (2 ** -21 if dtype == torch.float32 else 2 ** -6) * float(want.abs().max())


@pytest.mark.parametrize("name", eh.COMBINE_NAMES)
def test_combine_cases_hold(name):
    c = eh.combine_case(name)
    assert c["finite"] and len(c["table"]) <= eh.COMBINE_MAXT
    offs = sorted((r[0], r[1]) for r in c["table"])
    assert all(a + n <= b for (a, n), (b, _) in zip(offs, offs[1:], strict=False)) and offs[-1][0] + offs[-1][1] <= len(c["parts"])
    # float64 numpy in table order
    p = c["parts"].double().numpy()
    l = [p[o:o + n].sum() * s for (o, n, _), s in zip(c["table"], c["scale"], strict=True)]
    style = sum(v for v, r in zip(l, c["table"], strict=True) if r[2] == 0)
    content = sum(v for v, r in zip(l, c["table"], strict=True) if r[2] != 0)
    assert c["losses"] == l and c["scores"] == [style, content, c["style_w"] * style + c["content_w"] * content, 1.0]
    assert np.float32(c["scores"][2]) == c["scores"][2]


def test_combine_cases_reach_the_unrolled_loop_and_the_limits():
    step = eh.combine_case("step")
    assert [r[1] for r in step["table"]] == eh.STEP_COUNTS
    shares = eh.wave_shares(step["table"])
    assert max(shares) > 192 + 63, "every lane of a wave takes the four-way unrolled loop"
    assert sum(1 for v in shares if v < 64) > 0, "a term boundary inside a wave's share"
    assert len(shares) > eh.COMBINE_NW
    assert max(eh.wave_shares(eh.combine_case("one_long")["table"])) == 512 == 2 * eh.COMBINE_UNROLL
    assert len(eh.combine_case("mixed64")["table"]) == eh.COMBINE_MAXT
    assert {r[2] for r in eh.combine_case("mixed64")["table"]} == {0, 1}
    assert 0 in [r[1] for r in eh.combine_case("empty_term")["table"]]
    assert eh.combine_case("empty_term")["losses"][1] == 0.0


@pytest.mark.parametrize("dtype", eh.DTYPES, ids=str)
def test_pool_cases_hold_and_match_autograd(dtype):
    scalar = set()
    for H, W, C in eh.pool_shapes(dtype):
        scalar.add(eh.pool_is_scalar(C, dtype))
        c = eh.pool_case(H, W, C)
        assert c["y"].shape == (H // 2, W // 2, C) and c["dx"][False].shape == (H, W, C)
        if H < 2 or W < 2:
            assert not bool(c["dx"][False].any()) and not bool(c["dx"][True].any())
            continue
        if H * W * C > 1 << 16:
            continue
        xr = eh._nchw(c["x"]).clone().requires_grad_(True)
        y = F.max_pool2d(xr, 2, 2)
        assert torch.equal(ei.nhwc(y.detach()), c["y"])
        y.backward(eh._nchw(c["dy"]))
        assert torch.equal(ei.nhwc(xr.grad), c["dx"][False])
        assert torch.equal(ei.nhwc(xr.grad * (xr.detach() > 0)), c["dx"][True])
        for t in (c["x"], c["dy"], c["prev"], c["dx"][True] + c["prev"]):
            assert torch.equal(t.to(dtype).float(), t)
    assert scalar == {True, False}, "the scalar and the vector kernels, in this type"
    trips_f = [eh.pool_fwd_trips(*s, dtype) for s in eh.pool_shapes(dtype)]
    trips_b = [eh.pool_bwd_trips(*s, dtype) for s in eh.pool_shapes(dtype)]
    assert max(trips_f) == 2 and max(trips_b) >= 2
    big = eh.POOL_SECOND_TRIP[torch.bfloat16][0]
    assert not eh.pool_is_scalar(big[2], torch.bfloat16) and eh.pool_fwd_trips(*big, torch.bfloat16) == 2
    assert eh.pool_bwd_trips(*big, torch.bfloat16) == 2
    small = eh.POOL_SECOND_TRIP[torch.float32][0]
    assert eh.pool_is_scalar(small[2], torch.float32) and eh.pool_fwd_trips(*small, torch.float32) == 2
    assert eh.pool_bwd_trips(*small, torch.float32) > 2
    assert eh.pool_fwd_trips(130, 130, 256, torch.bfloat16) == 1, "130 x 130 x 256 is one trip: the loops count windows"


def test_relu_and_adam_sizes_take_a_second_trip():
    for n in eh.RELU_SIZES + eh.RELU_SIZES_BF16:
        c = eh.relu_case(n)
        assert torch.equal(c["y"], F.relu(c["x"])) and (n < 64 or bool((c["x"] == 0).any()))
        if n >= 64:
            assert bool(torch.signbit(c["x"][c["x"] == 0]).any()) and not bool(torch.signbit(c["x"][c["x"] == 0]).all())
    assert eh.relu_fwd_trips(eh.RELU_SIZES[-1], torch.float32) == 2 and eh.relu_fwd_trips(eh.RELU_SIZES[-1], torch.bfloat16) == 1
    assert eh.relu_fwd_trips(eh.RELU_SIZES_BF16[-1], torch.bfloat16) == 2
    assert eh.relu_bwd_trips(eh.RELU_SIZES[-1]) > 2 and eh.relu_bwd_trips(4099) == 1
    assert eh.RELU_SIZES[-1] % 8 and eh.RELU_SIZES_BF16[-1] % 8
    assert eh.adam_trips(eh.ADAM_N) == 2 and eh.adam_trips(2048 * 256) == 1


def test_helpers():
    assert eh.gram_loss_parts(12) == 2 and eh.gram_loss_parts(512) == 2048
    assert math.isclose(eh.content_k(3.0, 4099), 3.0 * 2.0 / 4099, rel_tol=1e-6)
    u = eh.ulp(torch.tensor([1.0, 1.5, 2.0, 0.0, -3.0], dtype=torch.float64), torch.float32)
    assert u.tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 0.0, 2.0 ** -22]
    assert eh.ulp(torch.tensor([1.0], dtype=torch.float64), torch.bfloat16).tolist() == [2.0 ** -7]
