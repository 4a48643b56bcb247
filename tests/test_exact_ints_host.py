"""The exact-operand method (tests/exact_ints.py) checked without a GPU: every generator's own assertions hold for every
case the GPU tests run, the float64 oracle is reproduced bit for bit by fp32 arithmetic in other summation orders (which
is the property the GPU comparison rests on), and the case lists cover what they are meant to cover."""
from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

from . import bf16x3_emul as emu
from . import exact_ints as ei


def _shapes(table):
    return sorted({(prec, s) for prec in ei.PRECISIONS for s in table[prec]})


@pytest.mark.parametrize(("prec", "shape"), _shapes(ei.FORWARD_SHAPES) + _shapes(ei.POOL_SHAPES))
def test_forward_and_pool_generators_hold(prec, shape):
    info = ei.forward_case(prec, *shape)["info"]
    assert info["budget"] < ei.LIMIT
    if shape[2] >= 2 and shape[3] >= 2:
        for flags in (0, ei.RELU_OUT):
            p = ei.pool_case(prec, *shape, flags)
            assert p["pooled"].shape == (shape[2] // 2, shape[3] // 2, shape[1]) and int(p["idx"].max()) <= 7


@pytest.mark.parametrize(("prec", "shape"), _shapes(ei.ONE_SHAPES))
def test_one_by_one_generators_hold(prec, shape):
    assert ei.forward_case(prec, *shape, taps=1)["info"]["budget"] < ei.LIMIT


@pytest.mark.parametrize(("prec", "shape"), _shapes(ei.DGRAD_SHAPES))
def test_dgrad_generators_hold(prec, shape):
    assert ei.dgrad_case(prec, *shape)["info"]["budget"] < ei.LIMIT


@pytest.mark.parametrize(("prec", "shape"), _shapes(ei.DUAL_SHAPES))
def test_dual_generators_hold(prec, shape):
    assert ei.dual_case(prec, *shape)["info"]["budget"] < ei.LIMIT


def test_other_generators_hold():
    for cd, cs, H, W in ei.ROUTE_SHAPES:
        ei.route_case(cd, cs, H, W)
        ei.pool_case("bf16", 16, cs, 2 * H, 2 * W, ei.RELU_OUT)        # the forward launch that writes the arg-max map
    for cin, cout, H, W in ei.WS_SHAPES:
        ei.forward_case("bf16", cin, cout, H, W)
        if cin == cout:
            ei.dual_case("bf16", cin, cout, cout, H, W, True)
    for hw in ei.FIRST_HW + ei.FIRST_GRAM_HW:
        ei.first_case(*hw)
    for cin, cout in ei.FIRST_OTHER:
        for hw in ei.FIRST_OTHER_HW:
            ei.first_case(*hw, cin=cin, cout=cout)
    for prec, n, C in ei.GRAM_PARAMS:
        ei.gram_case(prec, n, C)
    for H, W, C in ei.FINISH_SHAPES:
        assert (C * H * W) & (C * H * W - 1) == 0, "the norm must be a power of two"
        ei.gram_case("fp32", H * W, C)


def test_every_bf16x3_form_has_a_case_where_the_dropped_term_counts():
    """A kernel that computed the full product (al.bl included) would differ from the expected value there."""
    assert any(ei.forward_case("bf16x3", *s)["info"]["dropped"] for s in ei.FORWARD_SHAPES["bf16x3"])
    assert any(ei.forward_case("bf16x3", *s)["info"]["dropped"] for s in ei.POOL_SHAPES["bf16x3"])
    assert any(ei.forward_case("bf16x3", *s, taps=1)["info"]["dropped"] for s in ei.ONE_SHAPES["bf16x3"])
    assert any(ei.dgrad_case("bf16x3", *s)["info"]["dropped"] for s in ei.DGRAD_SHAPES["bf16x3"])
    assert any(ei.dual_case("bf16x3", *s)["info"]["dropped"] for s in ei.DUAL_SHAPES["bf16x3"])
    assert any(ei.gram_case("bf16x3", n, C)["info"]["dropped"] for n, C in ei.GRAM_SHAPES)


def _chunked_fp32_conv(x, w, perm, chunk):
    """conv(x, w) accumulated in fp32, the K axis permuted and added chunk by chunk."""
    acc = None
    for k0 in range(0, len(perm), chunk):
        idx = perm[k0:k0 + chunk]
        part = F.conv2d(x[:, idx].float(), w[:, idx].float(), padding=w.shape[-1] // 2)
        acc = part if acc is None else acc + part
        assert acc.dtype == torch.float32
    return acc


@pytest.mark.parametrize(("prec", "shape"), _shapes(ei.FORWARD_SHAPES))
def test_oracle_is_what_fp32_gives_in_any_order(prec, shape):
    """The float64 reference's bits from fp32 convolutions of the same operands with the K axis permuted and accumulated
    in two different chunkings: under the budget no partial sum rounds, so every order gives the same number."""
    cin = shape[0]
    case = ei.forward_case(prec, *shape)
    x, w, b = case["x"], case["w"], case["b"]
    g = torch.Generator().manual_seed(cin)
    for chunk in (8, 24):
        perm = torch.randperm(cin, generator=g)
        if prec == "bf16x3":
            (xh, xl), (wh, wl) = emu.split(x), emu.split(w)
            got = (_chunked_fp32_conv(xl, wh, perm, chunk) + _chunked_fp32_conv(xh, wl, perm, chunk)
                   + _chunked_fp32_conv(xh, wh, perm, chunk))
        else:
            got = _chunked_fp32_conv(x, w, perm, chunk)
        got = got + b.view(1, -1, 1, 1)
        want = case["want"][0]
        assert torch.equal(ei.nhwc(got).to(want.dtype), want)


def test_bf16x3_expected_values_are_fp32_numbers():
    """store() asserts it for every expected tensor; here directly on the three-term value of the largest case."""
    cin, cout, H, W = max(ei.FORWARD_SHAPES["bf16x3"], key=lambda s: s[0])
    case = ei.forward_case("bf16x3", cin, cout, H, W)
    val, _ = ei.product("bf16x3", case["x"], case["w"])
    assert torch.equal(val.float().double(), val)
    hl, lh, ll = ei.cross_terms(case["x"], case["w"])
    assert bool((hl != 0).any()) and bool((lh != 0).any())


def test_route_and_argmax_helpers_agree_with_torch():
    """The CPU routing through arg-max bytes is max_pool2d's backward (first maximum wins), given the bytes of the map."""
    g = torch.Generator().manual_seed(3)
    y = torch.randint(-2, 3, (1, 5, 6, 8), generator=g).float()           # plenty of ties
    yr = y.clone().requires_grad_(True)
    dyp = torch.randint(1, 9, (1, 5, 3, 4), generator=g).float()
    F.max_pool2d(yr, 2, 2).backward(dyp)
    codes = ei.argmax_codes(y)
    got = ei.route(ei.nhwc(dyp), ei.nhwc(codes), mask=False)
    assert torch.equal(got, ei.nhwc(yr.grad))
    got_m = ei.route(ei.nhwc(dyp), ei.nhwc(codes), mask=True)
    assert torch.equal(got_m, ei.nhwc(yr.grad * (y > 0)))


def test_expected_row_rules():
    """The literal copy of the table's alt / kpairs / pooling columns, on the cases the issue names."""
    assert ei.forced_rows("fp32") == [1, 2, 3, 4, 5, 6, 7, 8] == ei.forced_rows("bf16x3")
    assert [c for c in range(ei.NUM_TILES) if not ei.tile_pools(c)] == [7, 8, 11, 12, 16, 17]
    assert ei.expected_row(13, "bf16", 32) == 13 and ei.expected_row(13, "bf16", 48) == 1
    assert ei.expected_row(13, "bf16", 32, 48) == 1 and ei.expected_row(18, "bf16", 64, 16) == 2
    assert ei.expected_row(16, "bf16", 32, pooled=True) == 4 and ei.expected_row(11, "fp32", 8, pooled=True) == 4
    assert ei.expected_row(9, "fp32", 8) == 1 and ei.expected_row(7, "bf16x3", 8) == 7


@pytest.mark.parametrize("prec", ei.PRECISIONS)
def test_forward_cases_cover_every_served_tile(prec):
    """K stages, image edges and channel edges, per tile that is launched in this precision (ei.covering)."""
    for tile in ei.forced_rows(prec):
        assert ei.covering(prec, tile) == [], f"{prec} tile {tile}"


def test_dual_cases_mix_whole_and_broken_stage_pairs():
    """cin % 32 == 0 with cin2 % 32 != 0 and the reverse (where only launch_mfma's rule sends a whole-pair tile to its
    stand-in), and a case that stays on the tile, for every whole-pair tile."""
    kinds = {(cd % 32 == 0, c2 % 32 == 0) for cd, _, c2, _, _ in ei.DUAL_SHAPES["bf16"]}
    assert kinds == {(True, False), (False, True), (True, True), (False, False)}
    for tile in (c for c in range(ei.NUM_TILES) if ei.tile_kpairs(c)):
        rows = {ei.expected_row(c, p, s[0], s[2]) for p, c, s in ei.DUAL_PARAMS if p == "bf16" and c == tile}
        assert rows == {tile, ei.tile_alt(tile)}


def test_pool_cases_have_odd_sizes_and_the_smallest_image():
    for prec in ei.PRECISIONS:
        hw = {(s[2], s[3]) for s in ei.POOL_SHAPES[prec]}
        assert (2, 2) in hw and any(h % 2 and w % 2 for h, w in hw)
        rows = {ei.expected_row(c, p, s[0], pooled=True) for p, c, s in ei.POOL_PARAMS if p == prec}
        assert ei.POOL_TILE in rows and rows <= {c for c in range(ei.NUM_TILES) if ei.tile_pools(c)}
