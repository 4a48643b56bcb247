"""Exact-integer parity of the conv and Gram kernels on a real MI355X (method and case lists: tests/exact_ints.py).

Every comparison is torch.equal against the float64 CPU value of integer operands for which fp32 arithmetic is exact in
any summation order: the same bits from every tile (STV_CONV_CFG forced, and the row that really ran read back with
stv_conv_last_launch), every K split, the blocked fp32 summation, the weight-stationary kernel and all three precisions.
Outputs start from a sentinel, so an element a kernel does not write differs too.  Accuracy - rounding, summation order,
the term bf16x3 drops - is not what these tests measure: test_gpu_ops.py and test_gpu_bf16x3.py keep that.
"""
from __future__ import annotations

import collections
import functools

import pytest
import torch

from style_transfer_visualizer_amd import _lib, ops
from tests.conftest import record_parity

from . import exact_ints as ei

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -77.0
RELU_BOTH = ops.RELU_IN | ops.RELU_OUT

# per test function: [comparisons, differing elements] -> one parity-table row each when the module is done
_TALLY: dict[str, list[int]] = collections.defaultdict(lambda: [0, 0])


@pytest.fixture(scope="module", autouse=True)
def _parity_rows():
    yield
    for name, (n, bad) in _TALLY.items():
        record_parity("exact integers", f"{name}: differing elements", bad, 0.0, f"{n} tensors compared bit for bit")


def same(got: torch.Tensor, want: torch.Tensor, fn: str, what: str) -> None:
    """torch.equal on the whole tensor; on failure the count of differing elements and the first one."""
    want = want.to(got.device)
    _TALLY[fn][0] += 1
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {tuple(got.shape)}/{got.dtype} for {tuple(want.shape)}/{want.dtype}"
    if torch.equal(got, want):
        return
    diff = ~(got == want)
    n = int(diff.sum())
    _TALLY[fn][1] += n
    first = tuple(int(v) for v in diff.nonzero()[0])
    pytest.fail(f"{what}: {n} of {got.numel()} elements differ; first at (y, x, channel) = {first}: "
                f"got {float(got[first])!r}, expected {float(want[first])!r}")


def ran(row: int, what: str) -> None:
    got = int(_lib.load().stv_conv_last_launch())
    assert got == row, f"{what}: launched row {got}, expected row {row}"


def sentinel(shape, dtype) -> torch.Tensor:
    return torch.full(tuple(shape), SENTINEL, device=DEV, dtype=dtype)


def act(t: torch.Tensor, prec: str) -> torch.Tensor:
    """[1,C,H,W] CPU fp32 -> NHWC in the storage type on the device."""
    return ops.to_nhwc(t, ei.storage_dtype(prec)).to(DEV)


def weight_forms(packed: torch.Tensor, prec: str) -> dict[str, torch.Tensor]:
    """[9,Cout,Cin] fp32 -> the weight layouts the precision takes: K-blocked and plain, or (bf16x3) K-blocked and split."""
    w = packed.to(ei.storage_dtype(prec)).to(DEV)
    if prec == "bf16x3":
        return {"split": ops.split_weights(ops.block_weights(w))}
    return {"blocked": ops.block_weights(w), "plain": w}


@functools.lru_cache(maxsize=None)
def forward_dev(prec, cin, cout, H, W, taps=9):
    c = ei.forward_case(prec, cin, cout, H, W, taps)
    if taps == 9:
        w = weight_forms(ops.pack_weights_fwd(c["w"]), prec)
    else:
        w = {"plain": c["w"].reshape(1, cout, cin).to(ei.storage_dtype(prec)).to(DEV)}      # bf16x3 splits them in the kernel
    return {"x": act(c["x"], prec), "w": w, "b": None if c["b"] is None else c["b"].to(DEV),
            "want": {f: v.to(DEV) for f, v in c["want"].items()}}


@pytest.mark.parametrize("param", ei.FORWARD_PARAMS, ids=ei.param_id)
def test_forward_every_tile(param, monkeypatch):
    """conv3x3 + bias under the four RELU_IN / RELU_OUT combinations, every weight layout."""
    prec, cfg, (cin, cout, H, W) = param
    monkeypatch.setenv("STV_CONV_CFG", str(cfg))
    d = forward_dev(prec, cin, cout, H, W)
    for form, w in d["w"].items():
        for flags in (0, ops.RELU_IN, ops.RELU_OUT, RELU_BOTH):
            what = f"forward {ei.param_id(param)} {form} flags={flags}"
            y = ops.conv_igemm(d["x"], w, d["b"], out=sentinel((H, W, cout), d["x"].dtype), flags=flags, split=prec == "bf16x3")
            ran(ei.expected_row(cfg, prec, cin), what)
            same(y, d["want"][flags], "forward", what)


@pytest.mark.parametrize("param", ei.ONE_PARAMS, ids=ei.param_id)
def test_one_by_one_every_tile(param, monkeypatch):
    """The pure 1x1 launch (TAPS = 1, the Gram-backward product): plain weights, which bf16x3 splits in the kernel."""
    prec, cfg, (cin, cout, H, W) = param
    monkeypatch.setenv("STV_CONV_CFG", str(cfg))
    d = forward_dev(prec, cin, cout, H, W, 1)
    for flags in (0, RELU_BOTH):
        what = f"1x1 {ei.param_id(param)} flags={flags}"
        y = ops.conv_igemm(d["x"], d["w"]["plain"], None, out=sentinel((H, W, cout), d["x"].dtype), flags=flags, split=prec == "bf16x3")
        ran(ei.expected_row(cfg, prec, cin), what)
        same(y, d["want"][flags], "one_by_one", what)


@functools.lru_cache(maxsize=None)
def dgrad_dev(prec, cd, cs, H, W):
    c = ei.dgrad_case(prec, cd, cs, H, W)
    return {"dy": act(c["dy"], prec), "w": weight_forms(ops.pack_weights_bwd(c["w"]), prec), "z": act(c["z"], prec),
            "prev": act(c["prev"], prec), "want": {f: v.to(DEV) for f, v in c["want"].items()}}


@pytest.mark.parametrize("param", ei.DGRAD_PARAMS, ids=ei.param_id)
def test_dgrad_mask_accum_every_tile(param, monkeypatch):
    prec, cfg, (cd, cs, H, W) = param
    monkeypatch.setenv("STV_CONV_CFG", str(cfg))
    d = dgrad_dev(prec, cd, cs, H, W)
    for form, w in d["w"].items():
        what = f"dgrad {ei.param_id(param)} {form}"
        out = d["prev"].clone()
        ops.conv_igemm(d["dy"], w, None, ref=d["z"], out=out, flags=ops.MASK | ops.ACCUM, split=prec == "bf16x3")
        ran(ei.expected_row(cfg, prec, cd), what)
        same(out, d["want"][ops.MASK | ops.ACCUM], "dgrad", what)


@functools.lru_cache(maxsize=None)
def pool_dev(prec, cin, cout, H, W, flags):
    c = ei.pool_case(prec, cin, cout, H, W, flags)
    return {k: c[k].to(DEV) for k in ("full", "pooled", "idx")}


def _pool_launches(prec, x, w, b, flags, want, fn, what, row):
    """stv_conv_igemm_pool with and without STV_POOL_ONLY: full map, pooled map, arg-max bytes."""
    H, W, _ = x.shape
    cout = want["full"].shape[2]
    for only in (0, ops.POOL_ONLY):
        y = sentinel((H, W, cout), x.dtype)
        yp = sentinel((H // 2, W // 2, cout), x.dtype)
        idx = torch.full((H // 2, W // 2, cout), 255, device=DEV, dtype=torch.uint8)
        ops.conv_igemm_pool(x, w, b, flags=flags | only, out=y, pool_out=yp, pool_idx=idx, split=prec == "bf16x3")
        ran(row, what)
        # with STV_POOL_ONLY the full-resolution map is not written at all
        same(y, sentinel(y.shape, y.dtype) if only else want["full"], fn, f"{what} only={only} full map")
        same(yp, want["pooled"], fn, f"{what} only={only} pooled map")
        same(idx, want["idx"], fn, f"{what} only={only} arg-max bytes")


@pytest.mark.parametrize("param", ei.POOL_PARAMS, ids=ei.param_id)
def test_pool_every_tile(param, monkeypatch):
    """A tile whose waves own no pooling window hands a pooled launch to kPoolTile."""
    prec, cfg, (cin, cout, H, W) = param
    monkeypatch.setenv("STV_CONV_CFG", str(cfg))
    d = forward_dev(prec, cin, cout, H, W)
    w = next(iter(d["w"].values()))
    for flags in (0, ops.RELU_OUT):
        _pool_launches(prec, d["x"], w, d["b"], flags, pool_dev(prec, cin, cout, H, W, flags), "pool",
                       f"pool {ei.param_id(param)} flags={flags}", ei.expected_row(cfg, prec, cin, pooled=True))


@functools.lru_cache(maxsize=None)
def dual_dev(prec, cd, cout, cin2, H, W, tied=False):
    c = ei.dual_case(prec, cd, cout, cin2, H, W, tied)
    x2 = act(c["x2"], prec)
    return {"dy": act(c["dy"], prec), "w": next(iter(weight_forms(ops.pack_weights_bwd(c["w"]), prec).values())), "x2": x2,
            "s": c["s"].to(ei.storage_dtype(prec)).to(DEV).contiguous(), "ref": x2 if tied else act(c["ref"], prec),
            "prev": act(c["prev"], prec), "want": {f: v.to(DEV) for f, v in c["want"].items()}}


@pytest.mark.parametrize("param", ei.DUAL_PARAMS, ids=ei.param_id)
def test_dual_every_tile(param, monkeypatch):
    """out = [prev +] mask(ref > 0) * dgrad(dy, w) + x2 . S^T.  A whole-pair tile (kpairs) runs only where cin AND cin2
    are multiples of 32: stv_conv_config, which never sees cin2, still names the forced tile where only cin2 breaks the
    pairs, and the launch then takes the tile's stand-in.  That difference is harmless - the product calls this form
    with cin2 = cout in {64, 128, 256, 512} only, and both tiles compute the same bits here - so it is pinned, not
    changed: the launched row is the stand-in, the advertised row the forced one."""
    prec, cfg, (cd, cout, cin2, H, W) = param
    monkeypatch.setenv("STV_CONV_CFG", str(cfg))
    d = dual_dev(prec, cd, cout, cin2, H, W)
    row = ei.expected_row(cfg, prec, cd, cin2)
    advertised = int(_lib.load().stv_conv_config(H, W, cd, cout, 9, ops.dtype_code(d["dy"].dtype, split=prec == "bf16x3")))
    assert advertised == ei.expected_row(cfg, prec, cd), "stv_conv_config decides on cin alone"
    if prec == "bf16" and ei.tile_kpairs(cfg) and cd % 32 == 0 and cin2 % 32:
        assert advertised == cfg and row == ei.tile_alt(cfg)
    for flags in (0, ops.MASK | ops.ACCUM):
        what = f"dual {ei.param_id(param)} flags={flags}"
        out = d["prev"].clone() if flags & ops.ACCUM else sentinel((H, W, cout), d["dy"].dtype)
        ops.conv_igemm_dual(d["dy"], d["w"], d["x2"], d["s"], ref=d["ref"] if flags & ops.MASK else None, out=out, flags=flags,
                            split=prec == "bf16x3")
        ran(row, what)
        same(out, d["want"][flags], "dual", what)


@functools.lru_cache(maxsize=None)
def route_dev(cd, cs, H, W):
    """Operands of the routed dgrad, and a genuine arg-max map: the bytes a conv + pool launch (the library's own tile
    choice) writes for a 2H x 2W map of cs channels - themselves compared with the CPU's."""
    c = ei.route_case(cd, cs, H, W)
    f = forward_dev("bf16", 16, cs, 2 * H, 2 * W)
    want = pool_dev("bf16", 16, cs, 2 * H, 2 * W, ops.RELU_OUT)
    idx = torch.full((H, W, cs), 255, device=DEV, dtype=torch.uint8)
    ops.conv_igemm_pool(f["x"], f["w"]["blocked"], f["b"], flags=ops.RELU_OUT, pool_idx=idx)
    same(idx, want["idx"], "route", f"arg-max bytes for the route {cs} {2 * H}x{2 * W}")
    return {"dy": act(c["dy"], "bf16"), "w": ops.block_weights(ops.pack_weights_bwd(c["w"]).bfloat16().to(DEV)), "idx": idx,
            "g": c["g"], "idx_cpu": idx.cpu()}


@pytest.mark.parametrize("param", ei.ROUTE_PARAMS, ids=ei.param_id)
def test_route_every_tile(param, monkeypatch):
    """stv_conv_igemm_route against the exact dgrad routed on the CPU through the kernel's own arg-max map."""
    cfg, (cd, cs, H, W) = param
    monkeypatch.setenv("STV_CONV_WS", "0")
    monkeypatch.delenv("STV_CONV_CFG", raising=False)
    d = route_dev(cd, cs, H, W)
    monkeypatch.setenv("STV_CONV_CFG", str(cfg))
    for flags in (0, ops.MASK):
        what = f"route {ei.param_id(param)} flags={flags}"
        got = sentinel((2 * H, 2 * W, cs), torch.bfloat16)
        ops.conv_igemm_route(d["dy"], d["w"], d["idx"], out=got, flags=flags)
        ran(ei.expected_row(cfg, "bf16", cd), what)
        same(got, ei.route(d["g"], d["idx_cpu"], bool(flags & ops.MASK)), "route", what)


@pytest.mark.parametrize("shape", ei.WS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_weight_stationary_kernel(shape, monkeypatch):
    """csrc/conv_ws.hip on the same forms, no tile forced: forward (four flag combinations, both weight layouts), the
    pooled forward with and without STV_POOL_ONLY, and the backward forms (masked dgrad; dgrad + Gram term with and
    without the mask)."""
    cin, cout, H, W = shape
    prec, bf16 = "bf16", torch.bfloat16
    monkeypatch.delenv("STV_CONV_CFG", raising=False)
    monkeypatch.setenv("STV_CONV_WS", "2")
    monkeypatch.setenv("STV_CONV_WS128", "2")
    d = forward_dev(prec, cin, cout, H, W)
    for form, w in d["w"].items():
        for flags in (0, ops.RELU_IN, ops.RELU_OUT, RELU_BOTH):
            what = f"ws forward {shape} {form} flags={flags}"
            assert ops.conv_uses_ws(H, W, cin, cout, bf16, flags=flags | (ops.W_BLOCKED if form == "blocked" else 0)), what
            y = ops.conv_igemm(d["x"], w, d["b"], out=sentinel((H, W, cout), bf16), flags=flags)
            ran(ei.LAUNCHED_WS, what)
            same(y, d["want"][flags], "weight_stationary", what)
    if H >= 2 and W >= 2:
        for flags in (ops.RELU_OUT, RELU_BOTH):
            assert ops.conv_uses_ws(H, W, cin, cout, bf16, flags=flags | ops.W_BLOCKED, has_pool=True)
            _pool_launches(prec, d["x"], d["w"]["blocked"], d["b"], flags, pool_dev(prec, cin, cout, H, W, flags),
                           "weight_stationary", f"ws pool {shape} flags={flags}", ei.LAUNCHED_WS)
    if cin == cout:
        b = dual_dev(prec, cin, cout, cout, H, W, True)
        for flags in (0, ops.MASK):
            what = f"ws dual {shape} flags={flags}"
            assert ops.conv_uses_ws(H, W, cin, cout, bf16, flags=flags | ops.W_BLOCKED, has_ref=True), what
            out = sentinel((H, W, cout), bf16)
            ops.conv_igemm_dual(b["dy"], b["w"], b["x2"], b["s"], ref=b["ref"] if flags else None, out=out, flags=flags)
            ran(ei.LAUNCHED_WS, what)
            same(out, b["want"][flags], "weight_stationary", what)
        g = dgrad_dev(prec, cin, cout, H, W)
        out = sentinel((H, W, cout), bf16)
        ops.conv_igemm(g["dy"], g["w"]["blocked"], None, ref=g["z"], out=out, flags=ops.MASK)
        ran(ei.LAUNCHED_WS, f"ws masked dgrad {shape}")
        same(out, g["want"][ops.MASK], "weight_stationary", f"ws masked dgrad {shape}")


def test_direct_kernel_is_reported(monkeypatch):
    """A shape outside the matrix-core tiling runs the direct kernel: row -1, the same exact value."""
    monkeypatch.delenv("STV_CONV_CFG", raising=False)
    x = ei.ints((1, 12, 5, 7), 1090, -3, 3)
    w = ei.ints((6, 12, 3, 3), 1091, -2, 2)
    want = ei.nhwc(ei.store("fp32", ei.product("fp32", x, w)[0]))
    y = ops.conv_igemm(act(x, "fp32"), ops.pack_weights_fwd(w).to(DEV), None, out=sentinel((5, 7, 6), torch.float32))
    ran(ei.LAUNCHED_DIRECT, "direct kernel")
    same(y, want, "direct", "direct kernel 12->6 5x7")


@pytest.mark.parametrize("hw", ei.FIRST_HW, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("variant", ["fp32", "bf16-matrix"])
@pytest.mark.parametrize("packed", [False, True])
def test_first_layer_forward_and_dgrad(hw, variant, packed):
    """conv_first_fwd / conv_first_dgrad: the fp32 kernels and the bf16 split-product kernels on the matrix cores, with
    caller-packed and call-packed weights, down to 1 x 1, 1 x 37 and 37 x 1."""
    H, W = hw
    dtype = torch.float32 if variant == "fp32" else torch.bfloat16
    c = ei.first_case(H, W)
    wf = ops.pack_weights_fwd(c["w"]).to(DEV)
    pk = ops.conv_first_pack(wf) if packed else None
    what = f"first layer {H}x{W} {variant} packed={packed}"
    y = ops.conv_first_fwd(c["x"].to(DEV), wf, c["b"].to(DEV), dtype, out=sentinel((H, W, 64), dtype), packed=pk)
    same(y, c["want"].to(dtype), "first_layer", what + " forward")
    dx = ops.conv_first_dgrad(ops.to_nhwc(c["dy"], dtype).to(DEV), wf, 3, out=sentinel((1, 3, H, W), torch.float32), packed=pk)
    same(dx, c["dx"], "first_layer", what + " dgrad")


@pytest.mark.parametrize("hw", ei.FIRST_OTHER_HW, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", ei.FIRST_OTHER, ids=lambda s: "to".join(map(str, s)))
def test_first_layer_other_shapes(shape, dtype, hw):
    """First layers that are not 3 -> 64: the lanes-per-pixel kernels (conv_first_*_kernel; one 16-byte channel vector
    per lane, 4 channels in fp32 and 8 in bf16) and the one-thread-per-output kernels (conv_first_*_generic).
    (cin, cout) -> kernel, fp32 / bf16:  (3, 8): 2 / 1 lanes per pixel;  (3, 16): 4 / 2;  (4, 32): 8 / 4, cin at kMaxCin;
    (3, 4): 1 lane / generic;  (3, 12): generic, 3 lanes is no power of two / generic;  (5, 8): forward lanes-per-pixel,
    dgrad generic (cin > kMaxCin);  (1, 8): lanes-per-pixel;  (4, 512): generic, more than 64 lanes / 72 KiB of weights.
    1 x 1 is a single pixel, 5 x 7 and 17 x 40 leave a ragged last workgroup; with the weights packed here and by the caller."""
    cin, cout = shape
    H, W = hw
    c = ei.first_case(H, W, cin=cin, cout=cout)
    wf = ops.pack_weights_fwd(c["w"]).to(DEV)
    for pk in (None, ops.conv_first_pack(wf)):
        what = f"first layer {cin}->{cout} {H}x{W} {dtype} packed={pk is not None}"
        y = ops.conv_first_fwd(c["x"].to(DEV), wf, c["b"].to(DEV), dtype, out=sentinel((H, W, cout), dtype), packed=pk)
        same(y, c["want"].to(dtype), "first_layer_other", what + " forward")
        dx = ops.conv_first_dgrad(ops.to_nhwc(c["dy"], dtype).to(DEV), wf, cin, out=sentinel((1, cin, H, W), torch.float32), packed=pk)
        same(dx, c["dx"], "first_layer_other", what + " dgrad")


@pytest.mark.parametrize("hw", ei.FIRST_GRAM_HW, ids=lambda s: "x".join(map(str, s)))
def test_first_layer_gram_slabs(hw):
    """conv_first_fwd(..., gram_partials=): the stored map, and slabs that add up to its Gram matrix exactly."""
    H, W = hw
    c = ei.first_case(H, W)
    wf = ops.pack_weights_fwd(c["w"]).to(DEV)
    slabs = torch.full((ops.gram_ksplit(H * W, 64), 64, 64), float("nan"), device=DEV)
    y = ops.conv_first_fwd(c["x"].to(DEV), wf, c["b"].to(DEV), torch.bfloat16, out=sentinel((H, W, 64), torch.bfloat16),
                           packed=ops.conv_first_pack(wf), gram_partials=slabs)
    same(y, c["want"].bfloat16(), "first_layer_gram", f"first layer {H}x{W} map beside the slabs")
    same(slabs.double().sum(0), c["gram"].double(), "first_layer_gram", f"first layer {H}x{W} Gram slabs")


@pytest.mark.parametrize(("prec", "n", "C"), ei.GRAM_PARAMS, ids=lambda v: str(v))
def test_gram_partial(prec, n, C):
    """stv_gram_partial: the slabs add up (in float64, exactly) to F^T F on the tile pairs they hold."""
    c = ei.gram_case(prec, n, C)
    slabs = ops.gram_partial(c["f"].to(ei.storage_dtype(prec)).to(DEV), split=prec == "bf16x3")
    held = ei.held_pairs(C).to(DEV)
    same(slabs.double().sum(0)[held], c["want"].double().to(DEV)[held], "gram_partial", f"gram {prec} n={n} C={C}")


def _clamps(R: torch.Tensor) -> list[float]:
    """A clamp above every entry (not engaged) and one that cuts the larger entries (engaged)."""
    top = float(R.max())
    assert top < 2.0 ** 23 and int((R > float(int(top) // 2)).sum()) > 0
    return [2.0 ** 23, float(int(top) // 2)]


@pytest.mark.parametrize("hwc", ei.FINISH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gram_finish_output(hwc):
    """stv_gram_finish's Gram output min(R, clamp) / norm with a power-of-two norm: exact, both blocks of the matrix."""
    H, W, C = hwc
    n = H * W
    c = ei.gram_case("fp32", n, C)
    R = c["want"]
    partials = ops.gram_partial(c["f"].to(DEV))
    for clamp in _clamps(R):
        g = sentinel((C, C), torch.float32)
        ops.gram_finish(partials, n, C, gram_out=g, clamp_max=clamp, norm=float(C * n))
        same(g, R.clamp_max(clamp) / float(C * n), "gram_finish", f"gram finish {hwc} clamp={clamp}")


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_gram_multi_output(prec):
    """stv_gram_multi: the batched chain's Gram outputs, norm = C * n a power of two for every tap."""
    dtype = ei.storage_dtype(prec)
    cases = [ei.gram_case(prec, H * W, C) for H, W, C in ei.FINISH_SHAPES]
    feats = [c["f"].reshape(H, W, C).to(dtype).to(DEV) for c, (H, W, C) in zip(cases, ei.FINISH_SHAPES, strict=True)]
    tgts = [torch.zeros(C, C, device=DEV) for _, _, C in ei.FINISH_SHAPES]
    top = max(float(c["want"].max()) for c in cases)
    low = min(float(c["want"].max()) for c in cases)
    for clamp in (2.0 * top, float(int(low) // 2)):
        grams, _, _ = ops.gram_multi(feats, tgts, clamp_max=clamp)
        for g, c, (H, W, C) in zip(grams, cases, ei.FINISH_SHAPES, strict=True):
            same(g, (c["want"].clamp_max(clamp) / float(C * H * W)), "gram_multi", f"gram multi {prec} {(H, W, C)} clamp={clamp}")
