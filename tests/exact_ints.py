"""Exact-operand parity for the conv and Gram kernels: operands for which fp32 arithmetic is exact in EVERY summation
order, so that the float64 CPU result is the only correct answer, bit for bit - whatever the tile, the K split, the
blocked fp32 summation or the kernel (tests/test_gpu_conv_exact.py on the GPU, tests/test_exact_ints_host.py anywhere).

Operands are integers (bias: quarters) that the storage type holds exactly.  Every generator asserts its own
preconditions, so an unsuitable draw fails here and not in the kernel comparison:

* budget: for every output element  sum|x||w| + |bias| + |prev| (+ sum|z||S|) < 2^24 in units of the smallest quantum
  (1/4 where a bias is added): no partial sum in any order can round;
* bf16 storage ("narrow" operands, x in [-3, 3], w in [-2, 2]): the expected output is the exact value rounded once to
  bf16.  An off-by-one error shows only where |y| <= 256, so at least 95 % of the (linear, pre-ReLU / pre-mask) outputs
  of a case lie there and at least 90 % are non-zero;
* bf16x3 ("wide" operands: the small integers plus a share of odd +-(257 .. 511), whose bf16 low part is +-1): the
  expected value is ah.bh + ah.bl + al.bh from tests/bf16x3_emul.py::split; hi + lo == v exactly; each cross product is
  non-zero in at least half of the outputs (the share grows as K shrinks);
* fp32: the wide operands, expected value the exact product.

What this method does NOT cover is accuracy - rounding, summation order, bf16x3's dropped al.bl term: the tolerance
and emulation tests (test_gpu_ops.py, test_gpu_bf16x3.py) keep that.

The references are cached (functools.lru_cache): a case's reference is the same for every tile that is forced.
A plain helper module: no fixtures, no pytest hooks.
"""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

from style_transfer_visualizer_amd import synthetic

from . import bf16x3_emul as emu

RELU_IN, RELU_OUT, MASK, ACCUM = 1, 2, 4, 8          # include/stv.h
PRECISIONS = ("bf16", "fp32", "bf16x3")
LIMIT = float(2 ** 24)

# ---- the tile table: a literal copy of csrc/conv_tiles.h (rows are appended, never renumbered) -------------------------
#       TH   BN  WM KS NBUF M16    kpairs alt
TILES = {
    0: (8, 128, 4, 1, 3, False, False, 2),
    1: (8, 64, 4, 1, 3, False, False, 1),
    2: (4, 128, 1, 1, 3, False, False, 2),
    3: (4, 64, 2, 1, 3, False, False, 3),
    4: (4, 64, 2, 2, 3, False, False, 4),
    5: (8, 64, 4, 1, 2, False, False, 5),
    6: (4, 64, 2, 1, 2, False, False, 6),
    7: (2, 64, 2, 2, 3, False, False, 7),
    8: (1, 64, 1, 2, 3, False, False, 8),
    9: (16, 64, 4, 1, 3, False, False, 1),
    10: (16, 64, 4, 1, 2, False, False, 5),
    11: (2, 32, 2, 2, 3, False, False, 7),
    12: (4, 32, 4, 2, 3, False, False, 4),
    13: (8, 64, 4, 1, 4, True, True, 1),
    14: (16, 64, 4, 1, 4, True, True, 1),
    15: (4, 64, 2, 1, 4, True, True, 3),
    16: (2, 32, 2, 2, 4, True, True, 7),
    17: (4, 32, 4, 2, 4, True, True, 4),
    18: (16, 128, 4, 1, 2, False, True, 2),
}
NUM_TILES = len(TILES)
POOL_TILE = 4          # kPoolTile
LAUNCHED_DIRECT, LAUNCHED_WS = -1, -2      # stv_conv_last_launch() outside the table


def tile_th(c): return TILES[c][0]
def tile_bn(c): return TILES[c][1]
def tile_ks(c): return TILES[c][3]
def tile_nbuf(c): return TILES[c][4]
def tile_m16(c): return TILES[c][5]
def tile_kpairs(c): return TILES[c][6]
def tile_alt(c): return TILES[c][7]
def tile_pools(c): return (TILES[c][0] // TILES[c][2]) % 2 == 0
def tile_serves_f32(c): return tile_alt(c) == c and not tile_m16(c)


def forced_rows(prec: str) -> list[int]:
    """The rows a test forces: every row in bf16, the rows instantiated for 4-byte elements otherwise."""
    return list(range(NUM_TILES)) if prec == "bf16" else [c for c in range(NUM_TILES) if tile_serves_f32(c)]


def cfg_valid(cfg: int, cout: int) -> bool:
    """STV_CONV_CFG is honoured (a 128-wide tile needs more than 64 output channels)."""
    return not (cout <= 64 and tile_bn(cfg) == 128)


def expected_row(cfg: int, prec: str, cin: int, cin2: int | None = None, *, pooled: bool = False) -> int:
    """The row stv_conv_last_launch() must report after a launch with STV_CONV_CFG=cfg honoured: the row itself; its
    `alt` for 4-byte elements or where `kpairs` is not met in cin or cin2; kPoolTile where a pooled output meets a tile
    without a pooling window."""
    four = prec != "bf16"
    c = cfg
    if four or (tile_kpairs(c) and cin % 32):
        c = tile_alt(c)
    if pooled and not tile_pools(c):
        c = POOL_TILE
    pairs = (not four) and cin % 32 == 0 and (cin2 is None or cin2 % 32 == 0)
    if four or (tile_kpairs(c) and not pairs):
        c = tile_alt(c)
    return c


def stage_channels(prec: str) -> int:
    """Input channels of one K stage (32 bytes)."""
    return 16 if prec == "bf16" else 8


def store_group(prec: str) -> int:
    """Output channels of one 16-byte store."""
    return 8 if prec == "bf16" else 4


def storage_dtype(prec: str) -> torch.dtype:
    return torch.bfloat16 if prec == "bf16" else torch.float32


# ---- operands --------------------------------------------------------------------------------------------------------------

def _u(shape, seed: int, stream: int) -> torch.Tensor:
    n = int(np.prod(shape))
    return torch.from_numpy(synthetic.hash_uniform(seed, stream, n).astype(np.float64)).reshape(shape)


def ints(shape, seed: int, lo: int, hi: int, *, density: float = 1.0, share: float = 0.0) -> torch.Tensor:
    """Deterministic integer-valued fp32 tensor: uniform integers in [lo, hi], a fraction 1 - density zeroed, and a
    fraction `share` of the elements replaced by odd +-(257 .. 511) (bf16 high part != value, low part +-1)."""
    v = torch.floor(_u(shape, seed, 77) * (hi - lo + 1)) + lo
    if density < 1.0:
        v = torch.where(_u(shape, seed, 78) < density, v, torch.zeros_like(v))
    if share > 0.0:
        pick = _u(shape, seed, 79)
        big = 257.0 + 2.0 * torch.floor(_u(shape, seed, 80) * 128.0)
        big = torch.where(_u(shape, seed, 81) < 0.5, -big, big)
        v = torch.where(pick < share, big, v)
    return v.float()


def _share(prec: str, terms: float) -> float:
    """Share of 9-10-bit integers in a wide operand: about four of them among the non-zero terms of one output."""
    return 0.0 if prec == "bf16" else min(0.5, 4.0 / max(terms, 1.0))


def _density(k: int) -> float:
    return 1.0 if k <= 32 else 0.25


def _terms(k: int, H: int, W: int, taps: int) -> float:
    return k * _density(k) * (min(3, H) * min(3, W) if taps == 9 else 1)


# ---- arithmetic of one product -----------------------------------------------------------------------------------------

def _conv(x, w):
    return F.conv2d(x, w, padding=w.shape[-1] // 2)


def product(prec: str, x: torch.Tensor, w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """(value, budget) of conv(x, w) in float64 as `prec` specifies it: exact, or the three kept terms of bf16x3.
    x [1,K,H,W], w [N,K,k,k] fp32 integer-valued; budget = the same sum over absolute values."""
    if prec == "bf16x3":
        xh, xl = emu.split(x)
        wh, wl = emu.split(w)
        assert torch.equal(xh + xl, x.double()) and torch.equal(wh + wl, w.double()), "hi + lo != v"
        val = _conv(xh, wh) + _conv(xh, wl) + _conv(xl, wh)
        bud = _conv(xh.abs(), wh.abs()) + _conv(xh.abs(), wl.abs()) + _conv(xl.abs(), wh.abs())
        return val, bud
    if prec == "bf16":
        assert torch.equal(x.bfloat16().float(), x) and torch.equal(w.bfloat16().float(), w), "operand is not a bf16 value"
    return _conv(x.double(), w.double()), _conv(x.double().abs(), w.double().abs())


def cross_terms(x: torch.Tensor, w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """ah.bl, al.bh and the dropped al.bl of conv(x, w)."""
    xh, xl = emu.split(x)
    wh, wl = emu.split(w)
    return _conv(xh, wl), _conv(xl, wh), _conv(xl, wl)


class Unsuitable(AssertionError):
    """A draw that stays exact but would not show an error (too many zero / large outputs, idle cross terms)."""


def first_suitable(build):
    """build(salt) for salt = 0, 1, ...: the first draw whose visibility assertions hold (tiny cases - eight outputs -
    miss "90 % non-zero" by a single zero).  Deterministic; a case no salt suits fails with the last complaint."""
    for salt in range(16):
        try:
            return build(100 * salt)
        except Unsuitable as e:
            last = e
    raise last


def check_budget(bud: torch.Tensor, quantum: float, what: str) -> float:
    worst = float(bud.max()) / quantum
    assert worst < LIMIT, f"{what}: budget {worst:.0f} quanta >= 2^24"
    return worst


def check_visible(lin: torch.Tensor, what: str) -> None:
    """bf16 storage: the linear result must sit where an off-by-one error survives the output rounding."""
    small = float((lin.abs() <= 256).double().mean())
    nonzero = float((lin != 0).double().mean())
    if small < 0.95:
        raise Unsuitable(f"{what}: only {small:.3f} of the outputs within |y| <= 256")
    if nonzero < 0.90:
        raise Unsuitable(f"{what}: only {nonzero:.3f} of the outputs non-zero")


def check_cross(x, w, what: str, *extra) -> bool:
    """bf16x3: each cross product non-zero in at least half of the outputs.  `extra`: a second (x, w) pair whose terms
    add to the same outputs (the dual form).  Returns whether the dropped al.bl term is non-zero somewhere."""
    hl, lh, ll = cross_terms(x, w)
    if extra:
        a, b, c = cross_terms(*extra)
        hl, lh, ll = hl + a, lh + b, ll.abs() + c.abs()
    f_hl, f_lh = float((hl != 0).double().mean()), float((lh != 0).double().mean())
    if f_hl < 0.5 or f_lh < 0.5:
        raise Unsuitable(f"{what}: cross terms non-zero in {f_hl:.2f} / {f_lh:.2f} of the outputs")
    return bool((ll != 0).any())


def store(prec: str, t64: torch.Tensor) -> torch.Tensor:
    """The exact value as the storage type holds it: fp32 must hold it exactly, bf16 rounds it once (RNE)."""
    t32 = t64.float()
    assert torch.equal(t32.double(), t64), "expected value is not an fp32 number"
    return t32.bfloat16() if prec == "bf16" else t32


def nhwc(t: torch.Tensor) -> torch.Tensor:
    return t[0].permute(1, 2, 0).contiguous()


# ---- references, one per form --------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def forward_case(prec: str, cin: int, cout: int, H: int, W: int, taps: int = 9) -> dict:
    return first_suitable(lambda salt: _forward_case(prec, cin, cout, H, W, taps, salt))


def _forward_case(prec: str, cin: int, cout: int, H: int, W: int, taps: int, salt: int) -> dict:
    """conv (3x3 or 1x1) + bias under the four RELU_IN / RELU_OUT combinations.  x, w, b: CPU fp32; want[flags]: NHWC
    in the storage type."""
    k = 3 if taps == 9 else 1
    sh = _share(prec, _terms(cin, H, W, taps))
    x = ints((1, cin, H, W), 1000 + taps + salt, -3, 3, share=sh)
    w = ints((cout, cin, k, k), 1001 + taps + salt, -2, 2, density=_density(cin), share=sh)
    b = ints((cout,), 1002 + salt, -32, 32) / 4 if taps == 9 else None
    what = f"forward {prec} {cin}->{cout} {H}x{W} taps={taps}"
    want, info = {}, {}
    for relu_in in (0, RELU_IN):
        xin = x.clamp_min(0) if relu_in else x
        val, bud = product(prec, xin, w)
        if b is not None:
            val, bud = val + b.double().view(1, -1, 1, 1), bud + b.double().abs().view(1, -1, 1, 1)
        info["budget"] = max(info.get("budget", 0.0), check_budget(bud, 0.25, what))
        if prec == "bf16":
            check_visible(val, what)
        if prec == "bf16x3":
            info["dropped"] = check_cross(xin, w, what) or info.get("dropped", False)
        for relu_out in (0, RELU_OUT):
            want[relu_in | relu_out] = nhwc(store(prec, val.clamp_min(0) if relu_out else val))
    return {"x": x, "w": w, "b": b, "want": want, "info": info}


@functools.lru_cache(maxsize=None)
def dgrad_case(prec: str, cd: int, cs: int, H: int, W: int) -> dict:
    return first_suitable(lambda salt: _dgrad_case(prec, cd, cs, H, W, salt))


def _dgrad_case(prec: str, cd: int, cs: int, H: int, W: int, salt: int) -> dict:
    """Masked dgrad: out = [prev +] (z > 0) * conv_transpose(dy, w), w [cd, cs, 3, 3] the forward weight; want[flags] for
    MASK and MASK|ACCUM."""
    sh = _share(prec, _terms(cd, H, W, 9))
    dy = ints((1, cd, H, W), 1010 + salt, -3, 3, share=sh)
    w = ints((cd, cs, 3, 3), 1011 + salt, -2, 2, density=_density(cd), share=sh)
    z = ints((1, cs, H, W), 1012 + salt, -3, 3)
    prev = ints((1, cs, H, W), 1013 + salt, -8, 8)
    wt = w.flip(2, 3).transpose(0, 1).contiguous()
    what = f"dgrad {prec} {cd}->{cs} {H}x{W}"
    val, bud = product(prec, dy, wt)
    budget = check_budget(bud + prev.double().abs(), 1.0, what)
    if prec == "bf16":
        check_visible(val + prev.double(), what)
    dropped = check_cross(dy, wt, what) if prec == "bf16x3" else False
    m = (z > 0).double()
    want = {MASK: nhwc(store(prec, val * m)), MASK | ACCUM: nhwc(store(prec, val * m + prev.double()))}
    return {"dy": dy, "w": w, "z": z, "prev": prev, "want": want, "info": {"budget": budget, "dropped": dropped}}


def argmax_codes(full: torch.Tensor) -> torch.Tensor:
    """Arg-max bytes of MaxPool2d(2,2) over the STORED map [1,C,H,W] (float): bits 0-1 the window position of the first
    maximum in scan order, bit 2 set where that maximum is positive."""
    Hp, Wp = full.shape[2] // 2, full.shape[3] // 2
    f = full[:, :, :2 * Hp, :2 * Wp]
    best = f[:, :, 0::2, 0::2]
    code = torch.zeros_like(best, dtype=torch.int64)
    for pos, cand in ((1, f[:, :, 0::2, 1::2]), (2, f[:, :, 1::2, 0::2]), (3, f[:, :, 1::2, 1::2])):
        take = cand > best
        best = torch.where(take, cand, best)
        code = torch.where(take, torch.full_like(code, pos), code)
    code = code + 4 * (best > 0).long()
    return code.to(torch.uint8)


@functools.lru_cache(maxsize=None)
def pool_case(prec: str, cin: int, cout: int, H: int, W: int, flags: int) -> dict:
    """conv + bias [+ ReLU] and, from the stored map, its 2x2 max-pool (odd sizes drop the last row / column) and the
    arg-max bytes."""
    case = forward_case(prec, cin, cout, H, W)
    full = case["want"][flags]                                      # NHWC, storage type
    f = full.float().permute(2, 0, 1)[None]
    pooled = nhwc(F.max_pool2d(f, 2, 2)).to(full.dtype)
    return {"x": case["x"], "w": case["w"], "b": case["b"], "full": full, "pooled": pooled, "idx": nhwc(argmax_codes(f)),
            "info": case["info"]}


@functools.lru_cache(maxsize=None)
def dual_case(prec: str, cd: int, cout: int, cin2: int, H: int, W: int, tied: bool = False) -> dict:
    return first_suitable(lambda salt: _dual_case(prec, cd, cout, cin2, H, W, tied, salt))


def _dual_case(prec: str, cd: int, cout: int, cin2: int, H: int, W: int, tied: bool, salt: int) -> dict:
    """out = [prev +] mask(ref > 0) * conv_transpose(dy, w) + x2 . S^T, S [cout, cin2]; want[flags] for 0 and MASK|ACCUM
    (and MASK alone).  tied: the mask is x2's own sign (ref = x2, cin2 = cout) - the weight-stationary kernel's form."""
    sh = _share(prec, _terms(cd, H, W, 9))
    sh2 = _share(prec, _terms(cin2, H, W, 1))
    dy = ints((1, cd, H, W), 1020 + salt, -3, 3, share=sh)
    w = ints((cd, cout, 3, 3), 1021 + salt, -2, 2, density=_density(cd), share=sh)
    x2 = ints((1, cin2, H, W), 1022 + salt, -3, 3, share=sh2)
    s = ints((cout, cin2), 1023 + salt, -2, 2, density=_density(cin2), share=sh2)
    ref = x2 if tied else ints((1, cout, H, W), 1024 + salt, -3, 3)
    prev = ints((1, cout, H, W), 1025 + salt, -8, 8)
    wt = w.flip(2, 3).transpose(0, 1).contiguous()
    s4 = s.view(cout, cin2, 1, 1)
    what = f"dual {prec} {cd}->{cout} (+{cin2}) {H}x{W}"
    v1, b1 = product(prec, dy, wt)
    v2, b2 = product(prec, x2, s4)
    budget = check_budget(b1 + b2 + prev.double().abs(), 1.0, what)
    if prec == "bf16":
        check_visible(v1 + v2 + prev.double(), what)
    dropped = check_cross(dy, wt, what, x2, s4) if prec == "bf16x3" else False
    m = (ref > 0).double()
    want = {0: nhwc(store(prec, v1 + v2)), MASK: nhwc(store(prec, v1 * m + v2)),
            MASK | ACCUM: nhwc(store(prec, v1 * m + v2 + prev.double()))}
    return {"dy": dy, "w": w, "x2": x2, "s": s, "ref": ref, "prev": prev, "want": want,
            "info": {"budget": budget, "dropped": dropped}}


def route(g: torch.Tensor, idx: torch.Tensor, mask: bool) -> torch.Tensor:
    """MaxPool2d(2,2)'s backward through an arg-max byte map: g [H,W,C] -> [2H,2W,C], every element at the position its
    byte names (bits 0-1), with `mask` only where bit 2 is set; zeros elsewhere."""
    H, W, C = g.shape
    out = torch.zeros(2 * H, 2 * W, C, dtype=g.dtype)
    code = idx.long()
    keep = (code & 4) != 0 if mask else torch.ones_like(code, dtype=torch.bool)
    for pos in range(4):
        out[pos // 2::2, pos % 2::2] = torch.where(((code & 3) == pos) & keep, g, torch.zeros_like(g))
    return out


@functools.lru_cache(maxsize=None)
def route_case(cd: int, cs: int, H: int, W: int) -> dict:
    return first_suitable(lambda salt: _route_case(cd, cs, H, W, salt))


def _route_case(cd: int, cs: int, H: int, W: int, salt: int) -> dict:
    """bf16 dgrad (no mask of its own, no accumulate) at the pooled size: the values stv_conv_igemm_route routes."""
    dy = ints((1, cd, H, W), 1030 + salt, -3, 3)
    w = ints((cd, cs, 3, 3), 1031 + salt, -2, 2, density=_density(cd))
    wt = w.flip(2, 3).transpose(0, 1).contiguous()
    what = f"route {cd}->{cs} {H}x{W}"
    val, bud = product("bf16", dy, wt)
    budget = check_budget(bud, 1.0, what)
    check_visible(val, what)
    return {"dy": dy, "w": w, "g": nhwc(store("bf16", val)), "info": {"budget": budget}}


@functools.lru_cache(maxsize=None)
def first_case(H: int, W: int, *, cin: int = 3, cout: int = 64) -> dict:
    """First layer cin -> cout: small integers, which every kernel (VALU, the split product on the matrix cores)
    multiplies exactly.  want: conv + bias (integer bias: the Gram slabs of the stored map stay integers), a value
    bf16 holds too; dx: the dgrad of an integer dy, exact in fp32."""
    x = ints((1, cin, H, W), 1040, -3, 3)
    w = ints((cout, cin, 3, 3), 1041, -2, 2)
    b = ints((cout,), 1042, -8, 8)
    dy = ints((1, cout, H, W), 1043, -3, 3)
    what = f"first layer {cin}->{cout} {H}x{W}"
    val, bud = product("bf16", x, w)
    val, bud = val + b.double().view(1, -1, 1, 1), bud + b.double().abs().view(1, -1, 1, 1)
    check_budget(bud, 1.0, what)
    assert float((val.abs() <= 256).double().mean()) == 1.0, f"{what}: an output beyond 256 would round in bf16"
    wt = w.flip(2, 3).transpose(0, 1).contiguous()
    dx, dbud = product("bf16", dy, wt)
    check_budget(dbud, 1.0, what + " dgrad")
    y = val[0].permute(1, 2, 0).reshape(H * W, cout)
    gram = y.t() @ y
    check_budget(y.abs().t() @ y.abs(), 1.0, what + " gram")
    return {"x": x, "w": w, "b": b, "dy": dy, "want": nhwc(store("fp32", val)), "dx": store("fp32", dx), "gram": store("fp32", gram)}


def gram_tile(C: int) -> int:
    return 64 if C <= 64 else 128


def held_pairs(C: int) -> torch.Tensor:
    """[C, C] bool: the tile pairs ti <= tj that the slabs hold (the finish kernel mirrors the rest)."""
    t = torch.arange(C) // gram_tile(C)
    return t[:, None] <= t[None, :]


@functools.lru_cache(maxsize=None)
def gram_case(prec: str, n: int, C: int) -> dict:
    return first_suitable(lambda salt: _gram_case(prec, n, C, salt))


def _gram_case(prec: str, n: int, C: int, salt: int) -> dict:
    """F [n, C] integer features -> F^T F (bf16x3: the three kept terms), n * max^2 inside the budget."""
    f = ints((n, C), 1050 + C + salt, -3, 3, share=_share(prec, n / 2.0))
    what = f"gram {prec} n={n} C={C}"
    if prec == "bf16x3":
        h, lo = emu.split(f)
        assert torch.equal(h + lo, f.double())
        val = h.t() @ h + h.t() @ lo + lo.t() @ h
        cross_b = h.abs().t() @ lo.abs()
        bud = h.abs().t() @ h.abs() + cross_b + cross_b.t()
        cross = h.t() @ lo
        if float((cross != 0).double().mean()) < 0.5:
            raise Unsuitable(f"{what}: cross term mostly zero")
        dropped = bool(((lo.t() @ lo) != 0).any())
    else:
        if prec == "bf16":
            assert torch.equal(f.bfloat16().float(), f)
        val = f.double().t() @ f.double()
        bud = f.double().abs().t() @ f.double().abs()
        dropped = False
    budget = check_budget(bud, 1.0, what)
    return {"f": f, "want": store("fp32", val), "info": {"budget": budget, "dropped": dropped}}


# ---- the cases the GPU tests run (tests/test_exact_ints_host.py asserts that they cover what they are meant to) ----------
# (cin, cout, H, W) per precision.  No cross product: chosen so that every served tile of every precision sees each K
# stage count, image edge and channel edge at least once (covering(), below).
FORWARD_SHAPES = {
    "bf16": [(16, 8, 1, 1), (32, 136, 1, 33), (48, 72, 3, 64), (96, 136, 5, 33), (16, 136, 7, 32), (32, 72, 9, 1),
             (128, 128, 15, 33), (96, 72, 17, 32), (32, 136, 33, 33), (48, 136, 2, 1), (32, 64, 3, 32), (128, 136, 17, 64),
             (96, 136, 9, 32), (32, 136, 15, 1), (16, 72, 5, 33), (32, 8, 2, 33), (48, 136, 3, 33), (32, 72, 7, 33)],
    "fp32": [(8, 4, 1, 1), (16, 136, 1, 33), (24, 72, 3, 64), (48, 136, 5, 33), (8, 136, 7, 32), (16, 72, 9, 1),
             (64, 128, 9, 33), (48, 72, 17, 32), (24, 136, 2, 1), (16, 64, 3, 32), (24, 136, 3, 33), (8, 72, 5, 33),
             (16, 4, 2, 33)],
}
FORWARD_SHAPES["bf16x3"] = FORWARD_SHAPES["fp32"]

# the dgrad (cd, cs, H, W), the pooled forward (cin, cout, H, W; H, W >= 2), the 1x1 and the routed dgrad run a subset:
# their main loops are the forward's, what differs is the epilogue (and, for the 1x1, the TAPS = 1 instantiation)
DGRAD_SHAPES = {
    "bf16": [(16, 8, 1, 1), (32, 136, 1, 33), (48, 72, 3, 64), (96, 136, 5, 33), (32, 72, 9, 1), (128, 136, 17, 64)],
    "fp32": [(8, 4, 1, 1), (16, 136, 1, 33), (24, 72, 3, 64), (48, 136, 5, 33), (16, 72, 9, 1)],
}
DGRAD_SHAPES["bf16x3"] = DGRAD_SHAPES["fp32"]
POOL_SHAPES = {
    "bf16": [(16, 8, 2, 2), (32, 136, 3, 33), (48, 72, 5, 65), (96, 136, 9, 33), (32, 64, 17, 32), (128, 136, 33, 7)],
    "fp32": [(8, 4, 2, 2), (16, 136, 3, 33), (24, 72, 5, 65), (48, 136, 9, 33), (16, 64, 17, 32)],
}
POOL_SHAPES["bf16x3"] = POOL_SHAPES["fp32"]
ONE_SHAPES = {
    "bf16": [(16, 8, 1, 1), (32, 136, 3, 33), (48, 72, 5, 64), (96, 136, 9, 1), (128, 64, 17, 33)],
    "fp32": [(8, 4, 1, 1), (16, 136, 3, 33), (24, 72, 5, 64), (48, 136, 9, 1), (64, 64, 9, 33)],
}
ONE_SHAPES["bf16x3"] = ONE_SHAPES["fp32"]
# (cd, cout, cin2, H, W): whole stage pairs in cin but not in cin2, the reverse, both, neither
DUAL_SHAPES = {
    "bf16": [(32, 72, 48, 5, 33), (48, 64, 32, 9, 32), (32, 136, 96, 17, 33), (16, 8, 16, 1, 1), (96, 136, 32, 3, 1)],
    "fp32": [(16, 72, 24, 5, 33), (24, 64, 8, 9, 32), (48, 136, 16, 3, 33), (8, 4, 8, 1, 1)],
}
DUAL_SHAPES["bf16x3"] = DUAL_SHAPES["fp32"]
ROUTE_SHAPES = [(32, 72, 5, 33), (48, 136, 9, 32), (96, 64, 3, 1), (16, 8, 1, 1)]      # (cd, cs, pooled H, pooled W)

# the weight-stationary kernel (bf16; 64 -> 64, 64 -> 128, 128 -> 128): ragged, single-tile, several tiles per workgroup
# (one persistent workgroup per CU and block of output channels: 264 x 320 is 330 tiles of 8 x 32 pixels on 256 CUs,
# 136 x 320 -> 128 channels 170 tiles on 128 workgroups, 130 x 160 at Cin = 128 325 tiles of 2 x 32)
WS_SHAPES = [(64, 64, 13, 7), (64, 64, 8, 32), (64, 64, 75, 101), (64, 128, 40, 72), (64, 64, 1, 33), (64, 64, 264, 320),
             (64, 128, 136, 320), (128, 128, 13, 7), (128, 128, 2, 32), (128, 128, 3, 40), (128, 128, 75, 101),
             (128, 128, 130, 160)]

FIRST_HW = [(40, 72), (5, 7), (64, 64), (33, 100), (1, 1), (1, 37), (37, 1)]
FIRST_GRAM_HW = [(64, 64), (75, 101), (13, 7), (8, 32)]
# first layers that are not 3 -> 64 (tests/test_gpu_conv_exact.py::test_first_layer_other_shapes names the kernel each reaches)
FIRST_OTHER = [(3, 8), (3, 16), (4, 32), (3, 4), (3, 12), (5, 8), (1, 8), (4, 512)]
FIRST_OTHER_HW = [(1, 1), (5, 7), (17, 40)]
GRAM_SHAPES = [(n, C) for C in (8, 12, 64, 100, 128, 256, 512) for n in (777, 4099)] + [(64, 64), (1, 8), (63, 128)]
# (a channel count must fill whole 16-byte groups of the storage type: 12 and 100 in fp32 / bf16x3 only)
GRAM_PARAMS = [(p, n, C) for p in PRECISIONS for n, C in GRAM_SHAPES if C % store_group(p) == 0]
# Gram output through the finish pass: (H, W, C) with C * H * W a power of two (the norm), and the clamp
FINISH_SHAPES = [(8, 16, 64), (4, 8, 128), (16, 16, 8), (2, 4, 512), (32, 32, 256)]


def _params(shapes: dict, *, pooled: bool = False) -> list[tuple]:
    out = []
    for prec in PRECISIONS:
        for cfg in forced_rows(prec):
            for shape in shapes[prec]:
                if cfg_valid(cfg, shape[1]):
                    out.append((prec, cfg, shape))
    return out


FORWARD_PARAMS = _params(FORWARD_SHAPES)
DGRAD_PARAMS = _params(DGRAD_SHAPES)
POOL_PARAMS = _params(POOL_SHAPES)
ONE_PARAMS = _params(ONE_SHAPES)
DUAL_PARAMS = _params(DUAL_SHAPES)
ROUTE_PARAMS = [(cfg, s) for cfg in range(NUM_TILES) for s in ROUTE_SHAPES if cfg_valid(cfg, s[1])]


def param_id(p) -> str:
    *head, shape = p
    return "-".join([str(h) if not isinstance(h, int) else f"t{h}" for h in head] + ["x".join(map(str, shape))])


def covering(prec: str, tile: int) -> list[str]:
    """What the forward cases that LAUNCH `tile` in `prec` (forced row = launched row) leave uncovered; [] = all of:
    K stages {1, 2, 3, >= 2 NBUF} (whole-pair tiles: 1 and 3 stage pairs and >= 2 NBUF stages), an odd stage (pair)
    count on a KS = 2 tile, W in {1, 33, k * 32}, H in {1, TH - 1, TH + 1, >= 2 TH + 1}, cout one store group wide
    (64-wide and narrower tiles), 8 past BN (72 / 136) and a whole multiple of BN."""
    shapes = [s for (p, c, s) in FORWARD_PARAMS if p == prec and c == tile and expected_row(c, p, s[0]) == tile]
    ck, th, bn, nbuf = stage_channels(prec), tile_th(tile), tile_bn(tile), tile_nbuf(tile)
    stages = {s[0] // ck for s in shapes}
    missing = []
    if tile_kpairs(tile):
        need = {2, 6}
    else:
        need = {1, 2, 3}
    missing += [f"{k} K stages" for k in sorted(need - stages)]
    if not any(k >= 2 * nbuf for k in stages):
        missing.append(f">= {2 * nbuf} K stages")
    if tile_ks(tile) == 2:
        unit = 2 if tile_m16(tile) else 1
        if not any((k // unit) % 2 == 1 for k in stages):
            missing.append("odd stage count on a K-split tile")
    ws = {s[3] for s in shapes}
    missing += [f"W = {v}" for v in (1, 33) if v not in ws]
    if not any(v % 32 == 0 for v in ws):
        missing.append("W a multiple of 32")
    hs = {s[2] for s in shapes}
    missing += [f"H = {v}" for v in sorted({1, max(th - 1, 1), th + 1}) if v not in hs]
    if not any(v >= 2 * th + 1 for v in hs):
        missing.append(f"H >= {2 * th + 1}")
    couts = {s[1] for s in shapes}
    if bn <= 64 and store_group(prec) not in couts:
        missing.append(f"cout = {store_group(prec)}")
    if (136 if bn == 128 else 72) not in couts:
        missing.append("cout 8 past BN")
    if not any(v % bn == 0 for v in couts):
        missing.append("cout a multiple of BN")
    return missing
