"""The conv kernels at the largest maps their size guard accepts: tensors of exactly 2^31 bytes, and ragged ones a few
rows below (the guard itself, on both sides of the bound: test_conv_limits_host.py; nothing above the bound is launched
here - a refused call on real, smaller buffers would overrun them if the guard failed).

Why these sizes: the kernels address every tensor with 32-bit byte offsets and aim every padding tap, dead lane and
masked store at offset 2^31.  That offset must stay out of range, the record counts (2^31: no int) and the last live
offsets (2^31 - 16) must not wrap - none of which a smaller map can show.

Operands are small integers generated on the device (fp32 storage: with a share of odd +-(257 .. 511), whose bf16 low
part is +-1), every sum exact in fp32 in any order (the bound is asserted per case), outputs start from a sentinel.
Checked per case, on the launch with the library's own tile (stv_conv_last_launch says which row ran):
  * crops against the float64 CPU value (exact_ints.product / store), torch.equal: the first and last 4 rows, the 4
    rows around byte offset 2^30 and around 2^31 less one row, and the first and last 8 columns of 64 rows spread over
    the height;
  * the whole map, bit for bit, against the same op on row bands of at most 512 MiB - views into the big tensors with
    a two-row halo (two: a pooling window starts on an even row), only a band's own rows compared.  Those are the
    kernels under test at sizes test_gpu_conv_exact.py holds, and the crops overlap them;
  * the rows between a ragged map's end and 2^31 bytes still hold the sentinel.
Forced tiles (one per loader / epilogue path: three-deep ring, two-deep ring, K split = kPoolTile, and a 16x16x32 tile
at 32 channels) must reproduce the own-tile map bit for bit.

Device memory: the operand maps (2 x 2 GiB, kept per storage type), two outputs of 2 GiB, a band of 0.5 GiB and the pooled
maps: a case peaks at about 9.5 GiB.
"""
from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

from style_transfer_visualizer_amd import _lib, ops

from . import exact_ints as ei

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -77.0
LIMIT = 2 ** 31
BAND = 512 * 2 ** 20
HALO = 2
RELU_BOTH = ops.RELU_IN | ops.RELU_OUT
MAIN_TILES = (3, 6, 4)          # 4x64 on the three-deep ring, on the two-deep ring, with the K split (kPoolTile)
M16_TILE = 15                   # 4x64 on v_mfma_f32_16x16x32_bf16 (conv_igemm16.hip): bf16, cin % 32 == 0

# (precision, channels, rows of the 2^31-byte map, width, forced tiles)
GEOM = [
    ("bf16", 16, 8192, 8192, MAIN_TILES),
    ("bf16", 32, 4096, 8192, (M16_TILE,)),
    ("fp32", 8, 8192, 8192, MAIN_TILES),
    ("bf16x3", 8, 8192, 8192, MAIN_TILES),
]
RAGGED = 5                      # rows short of the bound: H is then no multiple of any tile height
FORMS = ("forward", "1x1", "dgrad", "pooled", "dual", "route")
CASES = [(prec, C, Hf - short, W, tiles, form) for prec, C, Hf, W, tiles in GEOM for short in (0, RAGGED) for form in FORMS
         if not (form == "route" and prec != "bf16")]


def case_id(c) -> str:
    prec, C, H, W, tiles, form = c
    return f"{prec}-{C}ch-{H}x{W}-{form}"


# ---- operands ------------------------------------------------------------------------------------------------------------
_MAPS: dict = {}               # one storage type at a time: {"key": dtype, "a": ..., "b": ...}


def fill_ints(t: torch.Tensor, seed: int, lo: int, hi: int, big_every: int = 0) -> None:
    """Uniform integers in [lo, hi] into a flat device tensor, in chunks; ``big_every`` = n: one element in n is an odd
    +-(257 .. 511) instead."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    n, step = t.numel(), 1 << 26
    for o in range(0, n, step):
        m = min(step, n - o)
        v = torch.randint(lo, hi + 1, (m,), device=DEV, dtype=torch.int16, generator=gen)
        if big_every:
            big = 257 + 2 * torch.randint(0, 128, (m,), device=DEV, dtype=torch.int16, generator=gen)
            big = big * (2 * torch.randint(0, 2, (m,), device=DEV, dtype=torch.int16, generator=gen) - 1)
            v = torch.where(torch.randint(0, big_every, (m,), device=DEV, dtype=torch.int16, generator=gen) == 0, big, v)
        t[o:o + m] = v


def maps(prec: str) -> dict:
    """Two flat operand maps of 2^31 bytes in the precision's storage type: `a` (the conv input; wide in fp32 storage)
    and `b` (small integers: ReLU-mask map, old output and second term's input)."""
    dtype = ei.storage_dtype(prec)
    if _MAPS.get("key") != dtype:
        _MAPS.clear()
        torch.cuda.empty_cache()
        n = LIMIT // dtype.itemsize
        _MAPS.update(key=dtype, a=torch.empty(n, device=DEV, dtype=dtype), b=torch.empty(n, device=DEV, dtype=dtype))
        fill_ints(_MAPS["a"], 4100, -3, 3, 0 if prec == "bf16" else 8)
        fill_ints(_MAPS["b"], 4101, -3, 3)
    return _MAPS


def weights(prec: str, cin: int, cout: int) -> dict:
    """CPU fp32 integer weights (NCHW conv form), integer bias, the 1x1 weight and the dual form's seed."""
    wide = prec != "bf16"
    return {"w": ei.ints((cout, cin, 3, 3), 4200 + cin, -2, 2, share=0.25 if wide else 0.0),
            "w1": ei.ints((cout, cin, 1, 1), 4201 + cin, -2, 2, share=0.25 if wide else 0.0),
            "s": ei.ints((cout, cout, 1, 1), 4202 + cin, -2, 2),
            "bias": ei.ints((cout,), 4203 + cin, -8, 8)}


def assert_budget(prec: str, wt: dict) -> None:
    """Every partial sum of every form stays an fp32 integer: max|a| * sum|w| + |bias| + |old| + max|b| * sum|s| < 2^24."""
    amax = 3 if prec == "bf16" else 511
    worst = amax * float(wt["w"].abs().sum((1, 2, 3)).max()) + 8 + 3 + 3 * float(wt["s"].abs().sum((1, 2, 3)).max())
    assert worst < 2 ** 24 / 2, f"budget {worst}"      # (bf16x3 sums hi and lo parts separately: a factor of two in hand)
    if prec == "bf16":
        assert worst < 2 ** 11                           # and a bf16 map's values stay where one unit shows after rounding


def dev_weights(prec: str, w: torch.Tensor) -> torch.Tensor:
    """NCHW conv weight -> what the kernels take: K-blocked (bf16x3: and pre-split) for a 3x3, plain rows for a 1x1."""
    dtype = ei.storage_dtype(prec)
    if w.shape[-1] == 1:
        return w.reshape(1, w.shape[0], w.shape[1]).to(dtype).to(DEV).contiguous()
    blocked = ops.block_weights(ops.pack_weights_fwd(w).to(dtype).to(DEV))
    return ops.split_weights(blocked) if prec == "bf16x3" else blocked


# ---- the float64 CPU value of one form on a patch ----------------------------------------------------------------------------
def expected(form: str, prec: str, flags: int, wt: dict, x: torch.Tensor, z: torch.Tensor | None) -> torch.Tensor:
    """NCHW fp32 patches (any batch; zero padding at their edges) -> the stored output, NCHW in the storage type.
    route: the dgrad values before routing."""
    if form in ("forward", "pooled", "1x1"):
        xin = x.clamp_min(0) if flags & ops.RELU_IN else x
        val = ei.product(prec, xin, wt["w1"] if form == "1x1" else wt["w"])[0]
        if form != "1x1":
            val = val + wt["bias"].double().view(1, -1, 1, 1)
        return ei.store(prec, val.clamp_min(0) if flags & ops.RELU_OUT else val)
    if form == "route":
        return ei.store(prec, ei.product(prec, x, wt["w"])[0])
    val = ei.product(prec, x, wt["w"])[0] * (z > 0).double()              # dgrad, dual: MASK | ACCUM onto old = z
    if form == "dual":
        val = val + ei.product(prec, z, wt["s"])[0]
    return ei.store(prec, val + z.double())


def nchw(t: torch.Tensor) -> torch.Tensor:
    """device NHWC rows -> CPU fp32 [1,C,H,W]"""
    return t.float().cpu().permute(2, 0, 1)[None].contiguous()


def same(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    want = want.to(got.device)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {tuple(got.shape)}/{got.dtype} for {tuple(want.shape)}/{want.dtype}"
    if not torch.equal(got, want):
        diff = ~(got == want)
        first = tuple(int(v) for v in diff.nonzero()[0])
        pytest.fail(f"{what}: {int(diff.sum())} of {got.numel()} elements differ; first at {first}: "
                    f"got {float(got[first])!r}, expected {float(want[first])!r}")


# ---- one launch of a form on (views of) the operand maps ---------------------------------------------------------------------
def launch(form: str, prec: str, flags: int, dw: dict, x: torch.Tensor, z: torch.Tensor | None, idx: torch.Tensor | None,
           out: torch.Tensor, pool: torch.Tensor | None = None, pidx: torch.Tensor | None = None) -> None:
    split = prec == "bf16x3"
    if form == "forward":
        ops.conv_igemm(x, dw["w"], dw["bias"], out=out, flags=flags, split=split)
    elif form == "1x1":
        ops.conv_igemm(x, dw["w1"], None, out=out, flags=flags, split=split)
    elif form == "dgrad":
        ops.conv_igemm(x, dw["w"], None, ref=z, out=out, flags=ops.MASK | ops.ACCUM, split=split)
    elif form == "pooled":
        ops.conv_igemm_pool(x, dw["w"], dw["bias"], flags=flags, out=out, pool_out=pool, pool_idx=pidx, split=split)
    elif form == "dual":
        ops.conv_igemm_dual(x, dw["w"], z, dw["s"], ref=z, out=out, flags=ops.MASK | ops.ACCUM, split=split)
    else:
        ops.conv_igemm_route(x, dw["w"], idx, out=out, flags=flags)


def fresh(form: str, z: torch.Tensor | None, shape, dtype) -> torch.Tensor:
    """The output before the launch: the old values (= z) where the form accumulates, else the sentinel."""
    if form in ("dgrad", "dual"):
        return z.clone()
    return torch.full(tuple(shape), SENTINEL, device=DEV, dtype=dtype)


def own_row(form: str, prec: str, H: int, W: int, cin: int, cout: int) -> int:
    taps = {"1x1": 1, "route": ops.TUNE_ROUTE}.get(form, 9)
    cfg = int(_lib.load().stv_conv_config(H, W, cin, cout, taps, ops.dtype_code(ei.storage_dtype(prec), split=prec == "bf16x3")))
    assert cfg >= 0, f"stv_conv_config {cfg}"
    return ei.expected_row(cfg, prec, cin, cout if form == "dual" else None, pooled=form == "pooled")


def ran(row: int, what: str) -> None:
    got = int(_lib.load().stv_conv_last_launch())
    assert got == row, f"{what}: launched row {got}, expected row {row}"


def crop_windows(H: int, row_bytes: int) -> list[tuple[int, int]]:
    """Own rows [a, b) of the row crops, even-aligned (pooling windows): the first and last 4 rows, the 4 around byte
    offset 2^30 and around 2^31 less one row (clipped to a ragged map)."""
    out = {(0, 4), (H - 4 - H % 2, H)}
    for off in (2 ** 30, LIMIT - row_bytes):
        r = (off // row_bytes) // 2 * 2
        a, b = max(r - 2, 0), min(r + 2, H)
        if b - a >= 2:
            out.add((a, b))
    return sorted(out)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_conv_at_the_bound(case, monkeypatch):
    prec, C, H, W, tiles, form = case
    dtype = ei.storage_dtype(prec)
    es = dtype.itemsize
    split = prec == "bf16x3"
    monkeypatch.delenv("STV_CONV_CFG", raising=False)
    monkeypatch.setenv("STV_CONV_WS", "0")
    m = maps(prec)
    wt = weights(prec, C, C)
    assert_budget(prec, wt)
    dw = {"w": dev_weights(prec, wt["w"]), "w1": dev_weights(prec, wt["w1"]), "s": dev_weights(prec, wt["s"])[0].contiguous(),
          "bias": wt["bias"].to(DEV)}
    route = form == "route"
    # the geometry of the launch: a routed dgrad runs at half the size and writes the 2^31-byte map
    Hi, Wi = (H // 2, W // 2) if route else (H, W)
    Ho, Wo = (2 * Hi, 2 * Wi) if route else (Hi, Wi)
    Hfull = LIMIT // (Wo * C * es)
    assert Hfull * Wo * C * es == LIMIT and Hfull - RAGGED - 1 <= Ho <= Hfull
    x = m["a"][:Hi * Wi * C].view(Hi, Wi, C)
    z = m["b"][:Hi * Wi * C].view(Hi, Wi, C) if form in ("dgrad", "dual") else None
    idx = None
    if route:
        idx = torch.empty(Hi, Wi, C, device=DEV, dtype=torch.uint8)
        fill_ints(idx.view(-1), 4300, 0, 7)
    flag_sets = {"forward": (0, RELU_BOTH), "1x1": (0, RELU_BOTH), "pooled": (ops.RELU_OUT, ops.RELU_OUT | ops.POOL_ONLY),
                 "route": (0, ops.MASK)}.get(form, (ops.MASK | ops.ACCUM,))
    row = own_row(form, prec, Hi, Wi, C, C)
    for flags in flag_sets:
        what = f"{case_id(case)} flags={flags}"
        only = bool(flags & ops.POOL_ONLY)
        # ---- the whole map, the library's own tile; the rows up to 2^31 bytes belong to the same allocation
        whole = fresh(form, m["b"][:Hfull * Wo * C].view(Hfull, Wo, C) if z is not None else None, (Hfull, Wo, C), dtype)
        got = whole[:Ho]
        pool = pidx = None
        if form == "pooled":
            pool = torch.full((Ho // 2, Wo // 2, C), SENTINEL, device=DEV, dtype=dtype)
            pidx = torch.full((Ho // 2, Wo // 2, C), 255, device=DEV, dtype=torch.uint8)
        launch(form, prec, flags, dw, x, z, idx, got, pool, pidx)
        ran(row, what)
        if z is not None:
            same(whole[Ho:], m["b"][Ho * Wo * C:Hfull * Wo * C].view(Hfull - Ho, Wo, C), f"{what}: rows past a ragged map")
        else:
            assert bool((whole[Ho:] == SENTINEL).all()), f"{what}: rows past a ragged map were written"
        if only:
            assert bool((got == SENTINEL).all()), f"{what}: STV_POOL_ONLY wrote the full map"

        # ---- row crops against the float64 CPU value
        for a, b in crop_windows(Ho, Wo * C * es):
            ai, bi = (a // 2, b // 2) if route else (a, b)
            a0, b0 = max(ai - 1, 0), min(bi + 1, Hi)
            val = expected(form, prec, flags, wt, nchw(x[a0:b0]), None if z is None else nchw(z[a0:b0]))[:, :, ai - a0:bi - a0]
            where = f"{what}: rows {a}..{b - 1}"
            if route:
                same(got[a:b], ei.route(ei.nhwc(val), idx[ai:bi].cpu(), bool(flags & ops.MASK)), where)
                continue
            if not only:
                same(got[a:b], ei.nhwc(val), where)
            if form == "pooled":
                f32 = val.float()
                same(pool[a // 2:b // 2], ei.nhwc(F.max_pool2d(f32, 2, 2)).to(dtype), where + " pooled")
                same(pidx[a // 2:b // 2], ei.nhwc(ei.argmax_codes(f32)), where + " arg-max bytes")

        # ---- the first and last 8 columns of 64 rows spread over the height
        if not only:
            rows = torch.linspace(0, Hi - 1, 64).long()
            r3 = rows[:, None] + torch.tensor([-1, 0, 1])
            live = ((r3 >= 0) & (r3 < Hi)).to(DEV)
            r3 = r3.clamp(0, Hi - 1).to(DEV)
            for c0, keep in ((0, slice(0, 8)), (Wi - 9, slice(1, 9))):
                def patch(t, c0=c0):
                    p = t[r3][:, :, c0:c0 + 9] * live[:, :, None, None]                   # [64, 3, 9, C]
                    return p.float().cpu().permute(0, 3, 1, 2).contiguous()
                # (a patch's inner edge is no image border: only the columns whose taps lie inside it are compared)
                val = expected(form, prec, flags, wt, patch(x), None if z is None else patch(z))[:, :, 1, keep]      # [64, C, 8]
                where = f"{what}: columns {c0 + keep.start}..{c0 + keep.stop - 1} of 64 rows"
                g = val.permute(0, 2, 1).contiguous()                                     # [64, 8, C]
                if route:
                    cols = slice(c0 + keep.start, c0 + keep.stop)
                    want = ei.route(g, idx[rows.to(DEV)][:, cols].cpu(), bool(flags & ops.MASK))                    # [128, 16, C]
                    r2 = torch.stack([2 * rows, 2 * rows + 1], 1).reshape(-1).to(DEV)
                    same(got[r2][:, 2 * cols.start:2 * cols.stop], want, where)
                else:
                    same(got[rows.to(DEV)][:, c0 + keep.start:c0 + keep.stop], g, where)

        # ---- the whole map against row bands of at most 512 MiB
        own = BAND // (Wo * C * es) - 2 * HALO * (2 if route else 1)
        assert own > 0 and own % 2 == 0
        for r0 in range(0, Ho, own):
            r1 = min(r0 + own, Ho)
            i0, i1 = (r0 // 2, r1 // 2) if route else (r0, r1)
            t0, t1 = max(i0 - HALO, 0), min(i1 + HALO, Hi)
            k = 2 if route else 1
            zb = None if z is None else z[t0:t1]
            ob = fresh(form, zb, (k * (t1 - t0), Wo, C), dtype)
            pb = ib = None
            if form == "pooled":
                pb = torch.full(((t1 - t0) // 2, Wo // 2, C), SENTINEL, device=DEV, dtype=dtype)
                ib = torch.full(((t1 - t0) // 2, Wo // 2, C), 255, device=DEV, dtype=torch.uint8)
            launch(form, prec, flags, dw, x[t0:t1], zb, None if idx is None else idx[t0:t1], ob, pb, ib)
            lo = k * (i0 - t0)
            where = f"{what}: band rows {r0}..{r1 - 1}"
            if not only:
                same(got[r0:r1], ob[lo:lo + (r1 - r0)], where)
            if form == "pooled":
                p0, p1 = r0 // 2, r1 // 2           # (an odd last row is in no window)
                same(pool[p0:p1], pb[lo // 2:lo // 2 + (p1 - p0)], where + " pooled")
                same(pidx[p0:p1], ib[lo // 2:lo // 2 + (p1 - p0)], where + " arg-max bytes")
            del ob, pb, ib

        # ---- forced tiles reproduce the map bit for bit
        for cfg in tiles:
            monkeypatch.setenv("STV_CONV_CFG", str(cfg))
            other = fresh(form, z, (Ho, Wo, C), dtype)
            po = io = None
            if form == "pooled":
                po, io = torch.full_like(pool, SENTINEL), torch.full_like(pidx, 255)
            launch(form, prec, flags, dw, x, z, idx, other, po, io)
            ran(ei.expected_row(cfg, prec, C, C if form == "dual" else None, pooled=form == "pooled"), f"{what} tile {cfg}")
            same(other, got, f"{what}: tile {cfg} against tile {row}")
            if form == "pooled":
                same(po, pool, f"{what}: tile {cfg} pooled")
                same(io, pidx, f"{what}: tile {cfg} arg-max bytes")
            del other, po, io
            monkeypatch.delenv("STV_CONV_CFG")
        del whole, got, pool, pidx


def test_release_operand_maps():
    """The 4 GiB of operands go back before the next module."""
    _MAPS.clear()
    torch.cuda.empty_cache()
