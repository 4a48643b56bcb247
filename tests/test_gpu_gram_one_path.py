"""A single Gram tap and a batch of taps run the same bodies, so stv_gram_partial / stv_gram_finish and stv_gram_multi
leave the same bits on the same operands.  Real-valued features (a changed summation order would show), torch.equal on
whole tensors, every output started from a sentinel.

What each comparison holds: a batch of one partial-sum tap, from either entry point, launches the body behind direct
arguments (gram_partial_kernel / gram_partial_bf16_kernel); a batch of several goes through the batched wrappers.  So
stv_gram_multi with the tap alone repeats stv_gram_partial's launch and holds the host path that fills the batch.  The
mixed batch compares two different kernels: the tap under test at index 0 of its tile-size group, the companions at
a tap index and a block offset other than zero (bf16: both tile sizes in one grid).  The finish pass has one wrapper
kernel; there the test holds the two host paths that fill it.

The shapes are picked with the Python twin of stv_gram_ksplit (tests/exact_head.py): test_shapes_fall_in_their_classes
asserts that each one is the class it stands for, and that the twin is the library's for these shapes.
"""
from __future__ import annotations

import ctypes
import functools

import pytest
import torch

from style_transfer_visualizer_amd import _lib, ops

from . import exact_head as eh
from . import exact_ints as ei

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -77.0
PKB = 64                                    # csrc/gram.hip: pixels per LDS stage of the transposing-read bf16 body
PRECS = ("bf16", "fp32", "bf16x3")
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", "")      # noqa: E731


def _ceil_div(a: int, b: int) -> int:
    return -(-a // b)


def layout(n: int, C: int, pk: int) -> dict:
    """How stv_gram_partial cuts (n, C): slabs, pixels per slab (whole stages of pk pixels), pixels of the last slab."""
    ks = eh.gram_ksplit(n, C)
    chunk = _ceil_div(_ceil_div(n, ks), pk) * pk
    nt = _ceil_div(C, ei.gram_tile(C))
    return {"ks": ks, "chunk": chunk, "last": n - (ks - 1) * chunk, "tile": ei.gram_tile(C), "nt": nt, "pairs": nt * (nt + 1) // 2}


# (n, C) -> the class the shape stands for, as a predicate on its layout under either stage size
SHAPES = {
    (1, 8): lambda L, pk: L["ks"] == 1 and L["last"] == 1,
    (100, 8): lambda L, pk: L["ks"] == 2 and L["last"] % pk != 0,                              # a ragged last stage in slab 1
    (4099, 64): lambda L, pk: L["ks"] >= 33 and 0 < L["last"] < pk and L["tile"] == 64,
    (1000, 72): lambda L, pk: L["tile"] == 128 and L["nt"] == 1,                               # C % 64 != 0 (below)
    (520, 192): lambda L, pk: L["nt"] == 2 and L["pairs"] == 3 and 0 < L["last"] < pk,
    (300, 256): lambda L, pk: L["nt"] == 2 and L["tile"] == 128 and L["last"] > 0,             # C = 2 * 128 (below)
}
COMPANIONS = ((200, 136), (130, 24))        # a 128-wide and a 64-wide tap that share the mixed batch


def test_shapes_fall_in_their_classes():
    for (n, C), is_class in SHAPES.items():
        assert ops.gram_ksplit(n, C) == eh.gram_ksplit(n, C) and ops.gram_loss_parts(C) == eh.gram_loss_parts(C), (n, C)
        assert eh.gram_ksplit(n, C) < eh.FIN_DEEP_KSPLIT, "test_finish_* compares launches of 8 slices per element"
        for pk in (eh.PK, PKB):
            L = layout(n, C, pk)
            assert is_class(L, pk) and 0 < L["last"] <= L["chunk"], ((n, C), pk, L)
    assert 72 % 64 and 256 == 2 * 128
    assert [ei.gram_tile(C) for _, C in COMPANIONS] == [128, 64]
    for n, C in COMPANIONS:
        assert ops.gram_ksplit(n, C) == eh.gram_ksplit(n, C)


def sentinel(shape, dtype=torch.float32) -> torch.Tensor:
    return torch.full(tuple(shape), SENTINEL, device=DEV, dtype=dtype)


def slabs_for(n: int, C: int) -> torch.Tensor:
    return sentinel((eh.gram_ksplit(n, C), C, C))


@functools.lru_cache(maxsize=None)
def tap(prec: str, n: int, C: int) -> dict:
    """Real-valued features [n, C] in the storage type and the slabs stv_gram_partial leaves for them; both are shared by
    every test below and never written again."""
    g = torch.Generator().manual_seed(3100 + 7 * n + C)
    f = torch.randn(n, C, generator=g).to(ei.storage_dtype(prec)).to(DEV)
    slabs = ops.gram_partial(f, slabs_for(n, C), split=prec == "bf16x3")
    torch.cuda.synchronize()
    held = ei.held_pairs(C).to(DEV)
    assert bool((slabs[:, held] != SENTINEL).all()), "every held tile pair of every slab is written"
    assert bool((slabs[:, ~held] == SENTINEL).all()), "nothing else is"
    return {"f": f, "slabs": slabs}


def run_multi(entries: list[dict], code: int) -> None:
    """stv_gram_multi on entries of StvGramTap.fill keywords (tensors for addresses)."""
    table = (_lib.StvGramTap * len(entries))()
    for e, kw in zip(table, entries, strict=True):
        e.fill(**{k: v.data_ptr() if isinstance(v, torch.Tensor) else v for k, v in kw.items()})
    rc = _lib.load().stv_gram_multi(ctypes.addressof(table), len(entries), code, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "stv_gram_multi")
    torch.cuda.synchronize()


def code_of(prec: str) -> int:
    return ops.dtype_code(ei.storage_dtype(prec), split=prec == "bf16x3")


# ---- (a) partial sums --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nc", list(SHAPES), ids=_ids)
@pytest.mark.parametrize("prec", PRECS)
def test_partial_single_tap_equals_batched(prec, nc):
    """stv_gram_partial, stv_gram_multi with the tap alone, and stv_gram_multi with the tap ahead of a 128-wide and a
    64-wide one (bf16: both tile sizes in one grid): the same slabs, sentinel included where nothing is written."""
    n, C = nc
    single = tap(prec, n, C)
    alone = slabs_for(n, C)
    run_multi([dict(n_pixels=n, channels=C, clamp_max=5e5, coef=0.0, F=single["f"], partials=alone)], code_of(prec))
    assert torch.equal(alone, single["slabs"]), f"{prec} {nc}: batch of one"
    # the tap under test first: index 0 of its tile-size group in the batched wrapper, the companion of its size index 1
    batch = [(shape, slabs_for(*shape)) for shape in (nc, *COMPANIONS)]
    run_multi([dict(n_pixels=m, channels=D, clamp_max=5e5, coef=0.0, F=tap(prec, m, D)["f"], partials=s) for (m, D), s in batch],
              code_of(prec))
    for (m, D), s in batch:
        assert torch.equal(s, tap(prec, m, D)["slabs"]), f"{prec} {nc}: tap {(m, D)} of the mixed batch"


# ---- (b) finish --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nc", list(SHAPES), ids=_ids)
@pytest.mark.parametrize("seed_dtype", eh.DTYPES, ids=_ids)
def test_finish_single_tap_equals_batched(seed_dtype, nc):
    """stv_gram_finish and a one-tap stv_gram_multi (F absent: the finish pass alone) on the same slabs: the same Gram,
    loss partials and seed, with and without coef_dev.  ksplit < 128: both launch 8 slices per element."""
    n, C = nc
    prec = "bf16" if seed_dtype == torch.bfloat16 else "fp32"
    slabs = tap(prec, n, C)["slabs"]
    R = slabs.sum(0)[ei.held_pairs(C).to(DEV)]
    clamp = 0.5 * float(R.max())
    assert clamp > 0 and int((R > clamp).sum()) > 0 and int((R <= clamp).sum()) > 0, "the clamp cuts some entries"
    target = (torch.randn(C, C, generator=torch.Generator().manual_seed(3200 + C)) / C).to(DEV)
    for coef_dev in (None, torch.tensor([0.375], device=DEV)):
        outs = []
        for _ in range(2):
            outs.append({"gram_out": sentinel((C, C)), "loss_part": sentinel((eh.gram_loss_parts(C),)), "sgrad": sentinel((C, C), seed_dtype)})
        one, many = outs
        ops.gram_finish(slabs, n, C, target=target, clamp_max=clamp, coef=3.0, coef_dev=coef_dev, dtype=seed_dtype, **one)
        run_multi([dict(n_pixels=n, channels=C, clamp_max=clamp, coef=3.0, partials=slabs, target=target, coef_dev=coef_dev, **many)],
                  ops.dtype_code(seed_dtype))
        for k in one:
            assert bool((one[k] != SENTINEL).all()), f"{k} is written everywhere"
            assert torch.equal(one[k], many[k]), f"finish {_ids(seed_dtype)} {nc} coef_dev={coef_dev is not None}: {k}"


# ---- (c) bf16 features of 2 GiB ----------------------------------------------------------------------------------------------

def test_partial_bf16_features_of_2_gib():
    """C = 512, n = 2^21: exactly 2^31 bytes, the smallest map stv_gram_partial sends through the fp32-MFMA body instead
    of the transposing-read one.  Values in {-1, 0, 1}: every partial sum is an integer below 2^23, exact in any order,
    so the slabs must add up (float64) to what the slabs of the two halves - 2^30 bytes each, the transposing-read
    body - add up to.  About 2.2 GiB of device memory."""
    n, C = 1 << 21, 512
    assert n * C * 2 == 1 << 31 and n < 2 ** 23
    gen = torch.Generator(device=DEV).manual_seed(3300)
    f = torch.empty(n, C, device=DEV, dtype=torch.bfloat16)
    rows = n // 16
    for k in range(16):
        f[k * rows:(k + 1) * rows] = torch.randint(-1, 2, (rows, C), device=DEV, dtype=torch.int8, generator=gen)
    held = ei.held_pairs(C).to(DEV)
    whole = ops.gram_partial(f, slabs_for(n, C))
    torch.cuda.synchronize()
    assert bool((whole[:, ~held] == SENTINEL).all()), "only held tile pairs are written"
    got = whole.double().sum(0)[held]
    del whole
    want = sum(ops.gram_partial(f[a:a + n // 2], slabs_for(n // 2, C)).double().sum(0)[held] for a in (0, n // 2))
    assert float(want.abs().max()) < 2 ** 23 and float(want.max()) > n // 2, "integers in budget; the diagonal counts non-zeros"
    assert torch.equal(got, want)
