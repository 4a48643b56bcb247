"""Exact-operand parity for the loss head and the pointwise kernels: everything between the Gram slabs and the optimizer
(tests/test_gpu_head_exact.py on the GPU, tests/test_exact_head_host.py anywhere).  The method is tests/exact_ints.py's:
operands for which fp32 arithmetic is exact in every summation order, so the float64 CPU value is the only right answer
and the comparison is torch.equal.

* Gram finish: integer features (n * max^2 < 2^23), an integer clamp, a power-of-two norm and the target
  T = (min(R, clamp) + delta) / norm with delta a non-zero integer, |delta| <= 100, and delta[i][j] != delta[j][i]:
  d = G - T = -delta / norm is exact, the 256 squares of one block add up below 2^22 / norm^2, and k * d is exact in
  fp32 and in bf16 because k is a power of two (coef = C^2 * 2^q where C is not one) and |delta| < 256.  An element
  finished as a mirror image that reads the wrong target entry, a mask with `<` for `<=` at a tie, a dropped slab:
  each changes the expected tensors (finish_model's faults, asserted in the host test).
* content loss: integer F, T = F + delta with |delta| <= 2: the sum of squares stays below 2^24 for every n here.
* score combine: integer partials, power-of-two scales and weights; every prefix of every sum is an fp32 number.
* pool / ReLU: selections and copies of small integers with many ties.

The slabs of a finish case are built here, not by stv_gram_partial (test_gram_partial holds that kernel): only the tile
pairs ti <= tj hold numbers, the rest is NaN, so a finish that reads what the partial kernel never writes differs too.

Launch constants are literal copies, named after their csrc counterparts; the host test asserts that the case lists
reach the paths they are meant to reach under these constants, and the GPU test that the ksplit twin is the library's.
A plain helper module: no fixtures, no pytest hooks.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from . import exact_ints as ei
from .exact_ints import Unsuitable, first_suitable, ints

MASK, ACCUM = ei.MASK, ei.ACCUM
LIMIT = ei.LIMIT

# ---- csrc/gram.hip ---------------------------------------------------------------------------------------------------------
PK = 32                                        # pixels per LDS stage (fp32 partial kernel): slabs hold whole stages
FIN_V, FIN_L, FIN_U = 4, 32, 4
FIN_E = FIN_L * FIN_V                          # Gram elements (and one loss partial) per finish block
FIN_S_SHORT, FIN_S_DEEP = 8, 32                # slices per element: gram_finish_multi_kernel<T, 8> / <T, 32>
FIN_DEEP_KSPLIT = 128                          # stv_gram_finish: `deep = ksplit >= 128`
GRAM_WGS, GRAM_WGS_MIN, GRAM_KDIV = 512, 128, 8
# ---- csrc/pointwise.hip, csrc/optim.hip --------------------------------------------------------------------------------
K_MAX_BLOCKS, POINTWISE_THREADS = 256 * 8, 256            # kMaxBlocks, the block size grid_for() assumes
CONTENT_LOSS_PARTS, K_CONTENT_THREADS = 256, 1024         # STV_CONTENT_LOSS_PARTS, kContentThreads
COMBINE_MAXT, COMBINE_NW, COMBINE_THREADS = 64, 16, 1024  # loss_combine_kernel: MAXT, NW
COMBINE_UNROLL = 4 * 64                                   # entries of one trip through its four-way unrolled loop
STV_ERR_ARG = 1

DTYPES = (torch.float32, torch.bfloat16)


def k_vec(dtype: torch.dtype) -> int:
    """elem_traits<T>::kVec: elements of one 16-byte vector."""
    return 8 if dtype == torch.bfloat16 else 4


def _ceil_div(a: int, b: int) -> int:
    return -(-a // b)


def is_pow2(v: float) -> bool:
    return v > 0 and math.frexp(v)[0] == 0.5


def f32_exact(t64: torch.Tensor) -> torch.Tensor:
    assert torch.equal(t64.float().double(), t64), "expected value is not an fp32 number"
    return t64.float()


def stored(t64: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """The exact value in the storage type, which must hold it exactly (no rounding at all is allowed here)."""
    out = f32_exact(t64).to(dtype)
    assert torch.equal(out.double(), t64), f"expected value is not a {dtype} number"
    return out


# ---- Gram finish ----------------------------------------------------------------------------------------------------------

def gram_ksplit(n_pixels: int, C: int) -> int:
    """Python twin of stv_gram_ksplit (no tuning variables set)."""
    nt = _ceil_div(C, ei.gram_tile(C))
    pairs = nt * (nt + 1) // 2
    lo, hi = _ceil_div(GRAM_WGS_MIN, pairs), max(GRAM_WGS // pairs, 1)
    ks = n_pixels // (GRAM_KDIV * C)
    ks = min(max(ks, lo), hi)
    ks = min(ks, _ceil_div(n_pixels, 64))
    return max(ks, 1)


def gram_loss_parts(C: int) -> int:
    return _ceil_div(C * C, FIN_E)


def finish_slices(ks: int) -> int:
    """FIN_S of the stand-alone finish launch (stv_gram_multi always launches FIN_S_SHORT)."""
    return FIN_S_DEEP if ks >= FIN_DEEP_KSPLIT else FIN_S_SHORT


def finish_walk(ks: int, fin_s: int, slice_: int = 0) -> tuple[int, int]:
    """(trips through the unrolled slab loop, slabs its remainder code adds) for one slice of gram_finish_body."""
    k, trips = slice_, 0
    while k + (FIN_U - 1) * fin_s < ks:
        k += FIN_U * fin_s
        trips += 1
    return trips, sum(1 for u in range(FIN_U) if k + u * fin_s < ks)


# single-tap finish: (n, C); C = 8 at n = 64 ks gives ksplit = ks for every ks <= 512
KSPLIT_LADDER = (1, 7, 8, 9, 31, 32, 33, 64, 127, 128, 160, 512)
SINGLE_TAP = [(64 * ks, 8) for ks in KSPLIT_LADDER] + [(8192, 64)]
# mirror and ragged tiles: every C at 1 < ks < 25 (n = 777: ks = 13) and at ks >= 33 (n = 4099: ks = 65, or 43 with three
# tile pairs).  C = 512 has ten tile pairs and ksplit <= 51: ks >= 33 would need n >= 135,168 and 34 MB of slabs, so its
# lower-triangle mirror meets the unrolled loop at C = 192 and 256 only.
MIRROR_C = (12, 72, 100, 128, 192, 256, 512)
MIRROR = [(777, C) for C in MIRROR_C] + [(4099, C) for C in MIRROR_C if C != 512]
FINISH_CASES = SINGLE_TAP + MIRROR
CLAMP_KINDS = ("above", "cut", "tie")
ABSENT_CASE = (777, 192)                     # target absent / sgrad absent / coef_dev absent and present
SPATIAL_C = (64, 256)                        # n_pixels = 1: one pre-reduced slab, the call spatial.py makes
# stv_gram_multi: five taps (H, W, C), both tile sizes, C * H * W a power of two (ops.gram_multi's norm), ksplit 2, 1, 64,
# 1, 16; every C also fills whole bf16 vectors
MULTI_TAPS = [(8, 16, 64), (4, 8, 128), (64, 64, 8), (2, 4, 512), (32, 32, 256)]
MULTI_TIE_TAP = 4                            # the tap whose Gram supplies the tie clamp of the batched launch
CHAIN_STYLE = (32, 32, 256)                  # the chained test's style tap (H, W, C) and content size
CHAIN_CONTENT_N = 1 << 17


def default_norm(n: int, C: int) -> float:
    """C * n where that is a power of two (the reference's own norm), else the nearest power of two."""
    return float(2 ** round(math.log2(C * n)))


def default_coef(C: int, q: int = 10) -> float:
    """2^q, times C^2 where C is no power of two: k_grad = coef * 4 / (C * C * norm) stays a power of two."""
    return float(2 ** q) * (1.0 if is_pow2(C) else float(C * C))


def k_grad(coef: float, C: int, norm: float, coef_dev: float = 1.0) -> float:
    """stv_gram_finish's k_grad (times *coef_dev) in fp32 arithmetic, asserted to be a power of two."""
    f = np.float32
    k = f(coef) * f(4.0) / (f(C) * f(C) * f(norm))
    k = float(f(k) * f(coef_dev))
    assert is_pow2(k) and float(f(coef)) == coef, f"k_grad {k!r} is not a power of two (coef {coef}, C {C}, norm {norm})"
    return k


def build_slabs(f: torch.Tensor, ks: int) -> torch.Tensor:
    """[ks, C, C] fp32: slab k is the Gram of pixel chunk k (chunks of whole PK-pixel stages, as stv_gram_partial cuts
    them) on the held tile pairs, NaN elsewhere."""
    n, C = f.shape
    chunk = _ceil_div(_ceil_div(n, ks), PK) * PK
    assert ks * chunk >= n
    pad = torch.zeros(ks * chunk, C, dtype=torch.float64)
    pad[:n] = f.double()
    blocks = pad.view(ks, chunk, C)
    slabs = torch.bmm(blocks.transpose(1, 2), blocks)
    held = ei.held_pairs(C)
    assert float(slabs[-1][held].abs().sum()) > 0, "the last slab must count"
    slabs[:, ~held] = float("nan")
    return f32_exact_nan(slabs)


def f32_exact_nan(t64: torch.Tensor) -> torch.Tensor:
    out = t64.float()
    assert torch.equal(out.double().nan_to_num(nan=-1.0), t64.nan_to_num(nan=-1.0))
    return out


@functools.lru_cache(maxsize=None)
def gram_operands(n: int, C: int, seed: int = 0) -> dict:
    """Integer features [n, C] in [-3, 3], R = F^T F (float64, exact) and the slabs stv_gram_finish(n, C) expects."""
    f = ints((n, C), 2000 + C + seed, -3, 3)
    R = f.double().t() @ f.double()
    assert n * 9 < 2 ** 23 and float((f.double().abs().t() @ f.double().abs()).max()) < 2 ** 23, "Gram budget"
    ks = gram_ksplit(n, C)
    return {"f": f, "R": R, "ks": ks, "slabs": build_slabs(f, ks)}


def delta_matrix(C: int, seed: int) -> torch.Tensor:
    """[C, C] float64 integers, 1 <= |delta| <= 100, delta[i][j] != delta[j][i] for every i != j."""
    d = ints((C, C), seed, 1, 100).double() * (ints((C, C), seed + 1, 0, 1).double() * 2 - 1)
    low = torch.tril(torch.ones(C, C, dtype=torch.bool), -1)
    d = torch.where(low & (d == d.t()), -d, d)
    off = ~torch.eye(C, dtype=torch.bool)
    assert bool((d != d.t())[off].all()) and bool((d != 0).all()) and float(d.abs().max()) <= 100
    return d


def pick_clamp(R: torch.Tensor, kind: str) -> float:
    """An integer clamp: above every entry; cutting the larger entries; equal to an entry that occurs, with entries on
    both sides of it (the tie must keep its seed, as torch's clamp backward does)."""
    top = float(R.max())
    if kind == "above":
        return float(2 ** 23)
    if kind == "cut":
        clamp = float(int(top) // 2)
        if not int((R > clamp).sum()) > 0:
            raise Unsuitable("nothing to cut")
        return clamp
    assert kind == "tie"
    vals = torch.unique(R)
    clamp = float(vals[(2 * len(vals)) // 3])
    if not (int((R == clamp).sum()) > 0 and int((R > clamp).sum()) > 0 and int((R < clamp).sum()) > 0):
        raise Unsuitable(f"no tie with entries on both sides at clamp {clamp}")
    return clamp


def finish_reference(R: torch.Tensor, clamp: float, norm: float, delta: torch.Tensor | None) -> dict:
    """float64: gram = min(R, clamp) / norm, target = gram + delta / norm, loss = sum (gram - target)^2 over the whole
    matrix, dmask = (gram - target) * [R <= clamp] (the seed is k_grad * dmask)."""
    assert is_pow2(norm) and (clamp == float("inf") or clamp == float(int(clamp)))
    Rc = R.clamp(max=clamp)
    gram = f32_exact(Rc / norm)
    out = {"gram": gram, "clamp": clamp, "norm": norm}
    if delta is not None:
        C = R.shape[0]
        assert float((Rc + delta).abs().max()) < LIMIT, "target budget"
        target = f32_exact((Rc + delta) / norm)
        d = gram.double() - target.double()
        assert torch.equal(d, -delta / norm)
        # one block adds 128 elements and at most 128 mirror images
        assert 2 * FIN_E * float((delta ** 2).max()) < 2 ** 22 and float((delta ** 2).sum()) < LIMIT * 2 ** 20
        loss = (d ** 2).sum()
        assert float(loss) * norm * norm == float((delta ** 2).sum())
        out.update(target=target, loss=loss, dmask=d * (R <= clamp).double(), tie=int((R == clamp).sum()),
                   cut=int((R > clamp).sum()), C=C)
    return out


@functools.lru_cache(maxsize=None)
def finish_case(n: int, C: int, kind: str, norm: float | None = None) -> dict:
    return first_suitable(lambda salt: _finish_case(n, C, kind, norm, salt))


def _finish_case(n: int, C: int, kind: str, norm: float | None, salt: int) -> dict:
    ops_ = gram_operands(n, C, salt)
    case = finish_reference(ops_["R"], pick_clamp(ops_["R"], kind), default_norm(n, C) if norm is None else norm,
                            delta_matrix(C, 2100 + C + salt))
    if kind == "tie":
        assert case["tie"] > 0 and case["cut"] > 0, "the clamp must equal an entry that occurs"
    case.update(f=ops_["f"], R=ops_["R"], ks=ops_["ks"], slabs=ops_["slabs"], n=n, coef=default_coef(C))
    k_grad(case["coef"], C, case["norm"])
    return case


def seed_of(case: dict, dtype: torch.dtype, coef_dev: float = 1.0) -> torch.Tensor:
    """The backward seed k_grad * (G - T) * [R <= clamp] in the storage type, exactly."""
    return stored(case["dmask"] * k_grad(case["coef"], case["C"], case["norm"], coef_dev), dtype)


@functools.lru_cache(maxsize=None)
def raw_case(n: int, C: int) -> dict:
    """clamp = inf, norm = 1: the raw-Gram call of core_model.gram_matrix and spatial.py; must return R itself."""
    ops_ = gram_operands(n, C)
    case = finish_reference(ops_["R"], float("inf"), 1.0, None)
    case.update(ks=ops_["ks"], slabs=ops_["slabs"], n=n)
    assert torch.equal(case["gram"].double(), ops_["R"])
    return case


@functools.lru_cache(maxsize=None)
def spatial_case(C: int, kind: str) -> dict:
    """n_pixels = 1 and ONE slab that already holds the complete (mirrored) raw Gram of 1024 pixels; the norm is passed."""
    n_global = 1024
    ops_ = gram_operands(n_global, C)
    assert gram_ksplit(1, C) == 1
    case = finish_reference(ops_["R"], pick_clamp(ops_["R"], kind), default_norm(n_global, C), delta_matrix(C, 2200 + C))
    case.update(slabs=f32_exact(ops_["R"])[None].contiguous(), ks=1, n=1, coef=default_coef(C), R=ops_["R"])
    return case


@functools.lru_cache(maxsize=None)
def multi_case(prec: str, kind: str) -> dict:
    """Five taps for one stv_gram_multi launch: one clamp for all (ops.gram_multi), the tie taken from MULTI_TIE_TAP."""
    taps = [gram_operands(H * W, C) for H, W, C in MULTI_TAPS]
    clamp = pick_clamp(taps[MULTI_TIE_TAP]["R"], kind)
    out = []
    for (H, W, C), t in zip(MULTI_TAPS, taps, strict=True):
        assert is_pow2(C * H * W) and C % k_vec(ei.storage_dtype(prec)) == 0
        case = finish_reference(t["R"], clamp, float(C * H * W), delta_matrix(C, 2300 + C))
        case.update(f=t["f"], ks=t["ks"], coef=2.0 ** 10, hwc=(H, W, C))
        out.append(case)
    if kind != "above":
        assert sum(c["cut"] > 0 for c in out) >= 2, "the clamp must cut entries of several taps"
    return {"taps": out, "clamp": clamp, "coef": 2.0 ** 10}


def finish_model(slabs: torch.Tensor, target: torch.Tensor, C: int, clamp: float, norm: float, k: float,
                 fault: str | None = None) -> dict:
    """gram_finish_body on the CPU (float64): the held tiles read row-wise, the lower tiles finished as mirror images.
    fault: "mirror_row" - a mirror image reads the target one row down; "strict_mask" - `<` for `<=`; "drop_slab" - the
    last slab is not added.  Without a fault this is finish_reference."""
    TS = ei.gram_tile(C)
    s = slabs.double()
    if fault == "drop_slab":
        s = s[:-1]
    R = s.sum(0)
    tile = torch.arange(C) // TS
    lower = tile[:, None] > tile[None, :]
    R = torch.where(lower, R.t(), R)                   # a lower-tile element takes its value from the mirror element
    assert not bool(R.isnan().any())
    G = R.clamp(max=clamp) / norm
    t = target.double()
    if fault == "mirror_row":
        t = torch.where(lower, torch.roll(t, -1, 0), t)
    d = G - t
    keep = (R < clamp) if fault == "strict_mask" else (R <= clamp)
    return {"gram": G, "loss": (d ** 2).sum(), "seed": k * d * keep.double()}


# ---- content loss and gradient ------------------------------------------------------------------------------------------------

CONTENT_SIZES = (1, 3, 8, 13, 4099, 1 << 17, (1 << 20) + 4 * 1024 + 3)
CONTENT_GRAD_ONLY = ((1 << 21) + 4 * 256 + 3,)
# bf16 vectors hold 8 elements: the same second trip through the loops comes at twice the size
CONTENT_SIZES_BF16 = ((1 << 21) + 8 * 1024 + 3,)
CONTENT_GRAD_ONLY_BF16 = ((1 << 22) + 8 * 256 + 3,)


def content_sizes(dtype: torch.dtype, *, grad: bool = False) -> list[int]:
    wide = dtype == torch.bfloat16
    out = list(CONTENT_SIZES) + (list(CONTENT_SIZES_BF16) if wide else [])
    if grad:
        out += list(CONTENT_GRAD_ONLY) + (list(CONTENT_GRAD_ONLY_BF16) if wide else [])
    return out


def strided_trips(items: int, blocks: int, threads: int) -> int:
    """Trips the busiest thread makes through `for (i = block * threads + thread; i < items; i += grid * threads)`."""
    return _ceil_div(items, blocks * threads)


def grid_for(work_items: int) -> int:
    """csrc/pointwise.hip grid_for()."""
    return min(max(_ceil_div(work_items, POINTWISE_THREADS), 1), K_MAX_BLOCKS)


def content_loss_trips(n: int, dtype: torch.dtype) -> int:
    return strided_trips(n // k_vec(dtype), CONTENT_LOSS_PARTS, K_CONTENT_THREADS)


def content_grad_trips(n: int, dtype: torch.dtype) -> int:
    items = n // k_vec(dtype)
    return strided_trips(items, grid_for(items + 1), POINTWISE_THREADS)


relu_fwd_trips = content_grad_trips            # stv_relu_fwd: the same grid_for(n / kVec + 1)


def relu_bwd_trips(n: int) -> int:
    return strided_trips(n, grid_for(n), POINTWISE_THREADS)


def adam_trips(n: int) -> int:
    return strided_trips(n, min(_ceil_div(n, 256), 2048), 256)


@functools.lru_cache(maxsize=None)
def content_case(n: int) -> dict:
    """F integers in [-3, 3], T = F + delta, |delta| <= 2 (all bf16 numbers); loss = sum delta^2 < 2^24; prev: integers in
    [0, 8] with the sign of d = F - T, so that accumulating never cancels (the 2-ulp bound of the ragged sizes is a
    bound on k * d, which must not be magnified by a small sum)."""
    f = ints((n,), 2400, -3, 3)
    delta = ints((n,), 2401, -2, 2)
    t = f + delta
    d = (f - t).double()
    loss = (d ** 2).sum()
    assert float(loss) <= 4 * n and float(loss) < LIMIT and (n < 8 or float(loss) > 0)
    prev = ints((n,), 2402, 0, 8) * torch.where(d < 0, -1.0, 1.0).float()
    for v in (f, t, prev):
        assert torch.equal(v.bfloat16().float(), v)
    return {"f": f, "t": t, "d": d, "loss": loss, "prev": prev}


def content_k(coef: float, n: int, coef_dev: float = 1.0) -> float:
    """content_grad_kernel's k in fp32 arithmetic: coef * coef_dev * (2 / n)."""
    f = np.float32
    return float(f(f(coef) * f(coef_dev)) * (f(2.0) / f(n)))


def ulp(t64: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Spacing of `dtype` numbers at |t| (float64 tensor; 0 at 0)."""
    bits = 23 if dtype == torch.float32 else 7
    _, e = torch.frexp(t64.abs())
    return torch.where(t64 == 0, torch.zeros_like(t64), torch.ldexp(torch.ones_like(t64), e - 1 - bits))


def content_grad_bounds(want64: torch.Tensor, dtype: torch.dtype) -> tuple[torch.Tensor, torch.Tensor]:
    """(centre, allowed distance) of the ragged-n gradient, both float64: fp32 - the float64 value and 2 ulp of it;
    bf16 - the float64 value rounded once and one bf16 ulp of that."""
    if dtype == torch.float32:
        return want64, 2.0 * ulp(want64, dtype)
    centre = want64.float().bfloat16().double()
    return centre, ulp(centre, dtype)


# ---- score combine ------------------------------------------------------------------------------------------------------------

def _prefix_exact(terms: list[float]) -> float:
    """Sequential fp32 sum of fp32 numbers, every prefix asserted exact."""
    acc = 0.0
    for v in terms:
        acc += v
        assert float(np.float32(acc)) == acc, "a prefix of the score sum is not an fp32 number"
    return acc


def combine_expected(parts: torch.Tensor, table: list[list[int]], scale: list[float], style_w: float, content_w: float) -> dict:
    """float64 evaluation of loss_combine_kernel with every intermediate asserted to be an fp32 number (non-finite
    partials excepted: they make their own term, their kind's score and the total non-finite)."""
    assert all(is_pow2(s) for s in scale) and is_pow2(style_w) and is_pow2(content_w)
    p = parts.double()
    losses = []
    for (off, cnt, _), s in zip(table, scale, strict=True):
        seg = p[off:off + cnt]
        v = float(seg.sum()) * s
        if math.isfinite(v):
            assert float(seg.abs().sum()) < LIMIT and float(np.float32(v)) == v
        losses.append(v)
    finite = all(math.isfinite(v) for v in losses)
    if finite:
        style = _prefix_exact([v for v, row in zip(losses, table, strict=True) if row[2] == 0])
        content = _prefix_exact([v for v, row in zip(losses, table, strict=True) if row[2] != 0])
        total = _prefix_exact([style_w * style, content_w * content])
        scores = [style, content, total, 1.0]
    else:
        scores = None
    return {"losses": losses, "scores": scores, "finite": finite}


def wave_shares(table: list[list[int]]) -> list[int]:
    """Entries of one term inside one wave's share of loss_combine_kernel's virtual array, for every (wave, term)."""
    starts = np.concatenate([[0], np.cumsum([row[1] for row in table])])
    total = int(starts[-1])
    chunk = _ceil_div(total, COMBINE_NW)
    out = []
    for w in range(COMBINE_NW):
        lo, hi = w * chunk, min(w * chunk + chunk, total)
        out += [min(int(starts[k + 1]), hi) - max(int(starts[k]), lo) for k in range(len(table))]
    return [v for v in out if v > 0]


def _layout(counts: list[int], kinds: list[int], order: list[int] | None = None) -> list[list[int]]:
    """[offset, count, kind] rows; `order`: the sequence in which the terms' partials lie in memory."""
    offs, acc = {}, 0
    for k in (order if order is not None else range(len(counts))):
        offs[k] = acc
        acc += counts[k]
    return [[offs[k], counts[k], kinds[k]] for k in range(len(counts))]


STEP_COUNTS = [32, 128, 512, 2048, 2048, 256]            # the step's own table: five style taps and the content term
COMBINE_NAMES = ("step", "mixed64", "empty_term", "one_long", "shuffled")


@functools.lru_cache(maxsize=None)
def combine_case(name: str) -> dict:
    if name == "step":
        counts, kinds, order = STEP_COUNTS, [0, 0, 0, 0, 0, 1], None
    elif name == "mixed64":
        counts = [int(v) for v in ints((64,), 2500, 1, 40)]
        kinds, order = [int(v) for v in ints((64,), 2501, 0, 1)], None
        assert 0 < sum(kinds) < 64
    elif name == "empty_term":
        counts, kinds, order = [40, 0, 300, 0, 17], [0, 0, 1, 1, 0], None
    elif name == "one_long":
        counts, kinds, order = [8192], [0], None
    else:
        counts, kinds, order = [300, 17, 640, 5, 1200], [0, 1, 0, 0, 1], [3, 0, 4, 2, 1]
    table = _layout(counts, kinds, order)
    if name == "shuffled":
        assert [r[0] for r in table] != sorted(r[0] for r in table)
    n = len(counts)
    parts = ints((sum(counts),), 2510 + n, 0, 7)
    scale = [float(2.0 ** int(v)) for v in ints((n,), 2520 + n, -2, 1)]
    style_w, content_w = 4.0, 0.5
    exp = combine_expected(parts, table, scale, style_w, content_w)
    return {"parts": parts, "table": table, "scale": scale, "style_w": style_w, "content_w": content_w, **exp}


# ---- pool / ReLU / Adam ---------------------------------------------------------------------------------------------------------

RELU_SIZES = (1, 7, 8, 9, 4099, (1 << 21) + 1024 + 3)
RELU_SIZES_BF16 = ((1 << 22) + 8 * 1024 + 3,)          # relu_fwd's vector loop takes its second trip here in bf16
ADAM_N = 2048 * 256 + 37

# (H, W, C).  C = 3, 6: the scalar kernels in both types; C = 12: vectors in fp32, scalar in bf16; H = 1 / W = 1: no window.
POOL_SHAPES = [(7, 9, 3), (6, 6, 6), (1, 8, 8), (8, 1, 8), (5, 5, 12), (2, 2, 8), (130, 130, 256)]
# the loops run over windows, not input vectors: (130, 130, 256) is 135,200 vector items in bf16.  A second trip needs
# more than 524,288 windows x vectors (vector kernels) or pooled elements (scalar forward):
POOL_SECOND_TRIP = {torch.bfloat16: [(258, 258, 256)], torch.float32: [(840, 840, 3)]}


def pool_shapes(dtype: torch.dtype) -> list[tuple[int, int, int]]:
    return [s for s in POOL_SHAPES if not (s == (130, 130, 256) and dtype != torch.bfloat16)] + POOL_SECOND_TRIP[dtype]


def pool_is_scalar(C: int, dtype: torch.dtype) -> bool:
    return C % k_vec(dtype) != 0


def pool_fwd_trips(H: int, W: int, C: int, dtype: torch.dtype) -> int:
    items = (H // 2) * (W // 2) * (C if pool_is_scalar(C, dtype) else C // k_vec(dtype))
    return strided_trips(items, grid_for(items), POINTWISE_THREADS)


def pool_bwd_trips(H: int, W: int, C: int, dtype: torch.dtype) -> int:
    items = H * W * C if pool_is_scalar(C, dtype) else ((H + 1) // 2) * ((W + 1) // 2) * (C // k_vec(dtype))
    return strided_trips(items, grid_for(items), POINTWISE_THREADS)


def _nchw(t: torch.Tensor) -> torch.Tensor:
    return t.permute(2, 0, 1)[None]


@functools.lru_cache(maxsize=None)
def pool_case(H: int, W: int, C: int) -> dict:
    """x [H, W, C]: integers in [-2, 2] (ties in nearly every window, positive ones included); dy, prev: integers.  y: the
    2x2 maximum; idx: the arg-max bytes (first maximum in scan order, bit 2 = maximum > 0); dx[mask]: dy routed
    through idx (rows and columns the floor drops get zero)."""
    Ho, Wo = H // 2, W // 2
    x = ints((H, W, C), 2600, -2, 2)
    dy = ints((Ho, Wo, C), 2601, 1, 9) * (ints((Ho, Wo, C), 2602, 0, 1) * 2 - 1)
    prev = ints((H, W, C), 2603, -8, 8)
    idx = ei.nhwc(ei.argmax_codes(_nchw(x))) if Ho and Wo else torch.zeros(Ho, Wo, C, dtype=torch.uint8)
    win = x[:2 * Ho, :2 * Wo].reshape(Ho, 2, Wo, 2, C)
    y = win.amax(dim=(1, 3)) if Ho and Wo else torch.zeros(Ho, Wo, C)
    dx = {}
    for mask in (False, True):
        full = torch.zeros(H, W, C)
        if Ho and Wo:
            full[:2 * Ho, :2 * Wo] = ei.route(dy, idx, mask)
        dx[mask] = full
    if Ho and Wo and H * W * C <= 4096:
        tied = win.permute(0, 2, 4, 1, 3).reshape(Ho, Wo, C, 4)
        dup = (tied == tied.amax(-1, keepdim=True)).sum(-1) > 1
        assert bool(dup.any()) and bool((dup & (y > 0)).any()), "ties, positive ones included"
    return {"x": x, "dy": dy, "prev": prev, "y": y, "idx": idx, "dx": dx}


@functools.lru_cache(maxsize=None)
def relu_case(n: int) -> dict:
    """x: integers in [-3, 3] with exact zeros, every fifth zero a -0.0; dy, prev: integers."""
    x = ints((n,), 2700, -3, 3)
    zero = (x == 0) & (torch.arange(n) % 5 == 0)
    x = torch.where(zero, torch.full_like(x, -0.0), x)
    dy = ints((n,), 2701, -9, 9)
    prev = ints((n,), 2702, -8, 8)
    return {"x": x, "dy": dy, "prev": prev, "y": x.clamp_min(0), "dx": dy * (x > 0).float()}
