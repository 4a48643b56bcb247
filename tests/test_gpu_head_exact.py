"""Exact-operand parity of the loss head and the pointwise kernels on a real MI355X (method, case lists and launch
constants: tests/exact_head.py): stv_gram_finish and the finish stage of stv_gram_multi (Gram, loss partials, backward
seed), the content-loss kernels, stv_loss_combine / stv_loss_combine_log, the stand-alone pool and ReLU kernels, and
Adam's stride loop.

Every comparison is torch.equal against the float64 CPU value on outputs that start from a sentinel, with two
exceptions whose bounds are derived, not measured: the content gradient at sizes that are no power of two (k = coef*2/n
carries one rounding, the product one more: 2 ulp in fp32, one bf16 ulp of the value rounded once), and the Adam case
(a square root and a division: the tolerances of test_adam_step_matches_oracle), which is there for the loop, not for
exactness.  What ReLU and pooling do with NaN is not tested here.
"""
from __future__ import annotations

import collections
import fractions

import numpy as np
import pytest
import torch

from oracle import optim_ref
from style_transfer_visualizer_amd import _lib, ops
from tests.conftest import record_parity

from . import exact_head as eh
from . import exact_ints as ei

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -77.0
F32, BF16 = torch.float32, torch.bfloat16
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", "")      # noqa: E731

# per test function: [comparisons, differing elements] -> one parity-table row each when the module is done
_TALLY: dict[str, list[int]] = collections.defaultdict(lambda: [0, 0])
_ULPS: dict[str, list[float]] = collections.defaultdict(lambda: [0.0, 0.0])      # [worst distance in ulps, bound]


@pytest.fixture(scope="module", autouse=True)
def _parity_rows():
    yield
    for name, (n, bad) in _TALLY.items():
        record_parity("exact loss head", f"{name}: differing elements", bad, 0.0, f"{n} tensors compared bit for bit")
    for name, (worst, bound) in _ULPS.items():
        record_parity("exact loss head", f"{name}: distance in ulps", worst, bound, "derived bound (k: one rounding, product: one)")


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
    pytest.fail(f"{what}: {n} of {got.numel()} elements differ; first at {first}: got {float(got[first])!r}, expected {float(want[first])!r}")


def same_sum(parts: torch.Tensor, want: torch.Tensor, fn: str, what: str) -> None:
    """The partial sums, added in float64 (exact), are the float64 value."""
    same(parts.double().sum().reshape(1).cpu(), want.double().reshape(1), fn, what)


def within(got: torch.Tensor, want64: torch.Tensor, fn: str, what: str) -> None:
    """The derived bound of the ragged content gradient (eh.content_grad_bounds); exact zeros must be zeros."""
    centre, bound = eh.content_grad_bounds(want64, got.dtype)
    err = (got.double().cpu() - centre).abs()
    unit = bound / (2.0 if got.dtype == F32 else 1.0)
    ulps = torch.where(unit > 0, err / unit.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), err))
    worst = float(ulps.max())
    key = f"{fn} {_ids(got.dtype)}"
    _ULPS[key] = [max(_ULPS[key][0], worst), 2.0 if got.dtype == F32 else 1.0]
    print(f"{what}: worst distance {worst:.3f} ulp")
    assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} elements beyond the bound, worst {worst:.3f} ulp"


def sentinel(shape, dtype=F32) -> torch.Tensor:
    return torch.full(tuple(shape), SENTINEL, device=DEV, dtype=dtype)


def dev(t: torch.Tensor, dtype: torch.dtype | None = None) -> torch.Tensor:
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def scalar(v: float) -> torch.Tensor:
    return torch.tensor([v], device=DEV, dtype=F32)


# ---- Gram finish ----------------------------------------------------------------------------------------------------------------

def test_ksplit_twin_is_the_librarys():
    """The case lists are chosen through eh.gram_ksplit: they stay on their paths only while it is stv_gram_ksplit."""
    shapes = eh.FINISH_CASES + [(H * W, C) for H, W, C in eh.MULTI_TAPS] + [(1, C) for C in eh.SPATIAL_C] + [(24 * 64, 8), (25 * 64, 8)]
    for n, C in shapes:
        assert ops.gram_ksplit(n, C) == eh.gram_ksplit(n, C), (n, C)
        assert ops.gram_loss_parts(C) == eh.gram_loss_parts(C), C


def _finish(case: dict, n: int, C: int, dtype: torch.dtype, *, target=True, gram=True, loss=True, seed=True,
            coef_dev: float | None = None) -> dict:
    out = {"gram": sentinel((C, C)) if gram else None, "loss": sentinel((eh.gram_loss_parts(C),)) if loss else None,
           "seed": sentinel((C, C), dtype) if seed else None}
    assert ops.gram_ksplit(n, C) == case["slabs"].shape[0], "the kernel would read other slabs than the case holds"
    ops.gram_finish(dev(case["slabs"]), n, C, target=dev(case["target"]) if target else None, gram_out=out["gram"],
                    loss_part=out["loss"], sgrad=out["seed"], clamp_max=case["clamp"], coef=case.get("coef", 1.0),
                    coef_dev=None if coef_dev is None else scalar(coef_dev), dtype=dtype, norm=case["norm"])
    return out


@pytest.mark.parametrize("kind", eh.CLAMP_KINDS)
@pytest.mark.parametrize("nc", eh.FINISH_CASES, ids=_ids)
def test_gram_finish_gram_loss_and_seed(nc, kind):
    """Both finish variants, every ksplit class, ragged and mirrored tiles; three clamps, the tie among them."""
    n, C = nc
    c = eh.finish_case(n, C, kind)
    for dtype in eh.DTYPES:
        what = f"finish n={n} C={C} ks={c['ks']} clamp={kind} {_ids(dtype)}"
        out = _finish(c, n, C, dtype)
        same(out["gram"], c["gram"], "gram_finish", what + " gram")
        same_sum(out["loss"], c["loss"], "gram_finish", what + " loss")
        same(out["seed"], eh.seed_of(c, dtype), "gram_finish", what + " seed")


@pytest.mark.parametrize("nc", eh.FINISH_CASES, ids=_ids)
def test_gram_finish_raw(nc):
    """clamp = inf, norm = 1, no target: R itself, both triangles (core_model.gram_matrix, spatial.py phase 1)."""
    n, C = nc
    c = eh.raw_case(n, C)
    g = sentinel((C, C))
    assert ops.gram_ksplit(n, C) == c["slabs"].shape[0]
    ops.gram_finish(dev(c["slabs"]), n, C, gram_out=g, clamp_max=float("inf"), norm=1.0)
    same(g, c["gram"], "gram_finish_raw", f"raw finish n={n} C={C}")


@pytest.mark.parametrize("dtype", eh.DTYPES, ids=_ids)
def test_gram_finish_absent_outputs_and_coef_dev(dtype):
    n, C = eh.ABSENT_CASE
    c = eh.finish_case(n, C, "tie")
    fn = "gram_finish_absent"
    out = _finish(c, n, C, dtype, target=False)
    same(out["gram"], c["gram"], fn, "no target: gram")
    same(out["loss"], torch.zeros(eh.gram_loss_parts(C)), fn, "no target: loss partials are zero")
    same(out["seed"], sentinel((C, C), dtype), fn, "no target: the seed is not written")
    out = _finish(c, n, C, dtype, seed=False)
    same(out["gram"], c["gram"], fn, "no seed: gram")
    same_sum(out["loss"], c["loss"], fn, "no seed: loss")
    out = _finish(c, n, C, dtype, gram=False)
    same_sum(out["loss"], c["loss"], fn, "no gram: loss")
    same(out["seed"], eh.seed_of(c, dtype), fn, "no gram: seed")
    out = _finish(c, n, C, dtype, loss=False)
    same(out["seed"], eh.seed_of(c, dtype), fn, "no loss partials: seed")
    for cd in (0.5, 4.0):
        out = _finish(c, n, C, dtype, coef_dev=cd)
        same(out["seed"], eh.seed_of(c, dtype, cd), fn, f"coef_dev={cd}: seed")
        same_sum(out["loss"], c["loss"], fn, f"coef_dev={cd}: loss")


@pytest.mark.parametrize("kind", eh.CLAMP_KINDS)
@pytest.mark.parametrize("C", eh.SPATIAL_C)
def test_gram_finish_spatial_form(C, kind):
    """n_pixels = 1 with one pre-reduced slab and the norm passed: the second phase of spatial.py."""
    c = eh.spatial_case(C, kind)
    for dtype in eh.DTYPES:
        what = f"spatial finish C={C} clamp={kind} {_ids(dtype)}"
        out = _finish(c, 1, C, dtype, coef_dev=2.0)
        same(out["gram"], c["gram"], "gram_finish_spatial", what + " gram")
        same_sum(out["loss"], c["loss"], "gram_finish_spatial", what + " loss")
        same(out["seed"], eh.seed_of(c, dtype, 2.0), "gram_finish_spatial", what + " seed")


@pytest.mark.parametrize("kind", eh.CLAMP_KINDS)
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_gram_multi_gram_loss_and_seed(prec, kind):
    """stv_gram_multi, partial sums and finish: five taps of both tile sizes in one launch pair."""
    dtype = ei.storage_dtype(prec)
    m = eh.multi_case(prec, kind)
    feats = [dev(t["f"].reshape(*t["hwc"]), dtype) for t in m["taps"]]
    tgts = [dev(t["target"]) for t in m["taps"]]
    for cd in (None, 0.25):
        grams, parts, seeds = ops.gram_multi(feats, tgts, coef=m["coef"], clamp_max=m["clamp"],
                                             coef_dev=None if cd is None else scalar(cd))
        for t, g, lp, sg in zip(m["taps"], grams, parts, seeds, strict=True):
            what = f"gram multi {prec} {t['hwc']} clamp={kind} coef_dev={cd}"
            same(g, t["gram"], "gram_multi", what + " gram")
            same_sum(lp, t["loss"], "gram_multi", what + " loss")
            same(sg, eh.seed_of(t, dtype, 1.0 if cd is None else cd), "gram_multi", what + " seed")


# ---- content loss and gradient ------------------------------------------------------------------------------------------------

def _content_params(*, grad: bool) -> list:
    return [(d, n) for d in eh.DTYPES for n in eh.content_sizes(d, grad=grad)]


@pytest.mark.parametrize(("dtype", "n"), _content_params(grad=False), ids=_ids)
def test_content_loss_and_one_pass_gradient(dtype, n):
    """stv_content_loss and stv_content_loss_grad: the same exact partial sums; the one-pass gradient is the two-pass
    one bit for bit, and exact (n a power of two) or inside the derived bound."""
    c = eh.content_case(n)
    f, t = dev(c["f"], dtype), dev(c["t"], dtype)
    what = f"content n={n} {_ids(dtype)}"
    parts = sentinel((eh.CONTENT_LOSS_PARTS,))
    ops.content_loss(f, t, parts)
    same_sum(parts, c["loss"], "content_loss", what + " loss")
    coef = 8.0
    parts1, g_one, g_two = sentinel((eh.CONTENT_LOSS_PARTS,)), sentinel((n,), dtype), sentinel((n,), dtype)
    ops.content_loss_grad(f, t, parts1, g_one, coef)
    ops.content_grad(f, t, g_two, coef)
    same(parts1, parts, "content_loss", what + " one-pass partial sums")
    same(g_one, g_two, "content_loss", what + " one-pass gradient = two-pass gradient")
    if eh.is_pow2(n):
        same(g_one, eh.stored(eh.content_k(coef, n) * c["d"], dtype), "content_loss", what + " gradient")
    else:
        within(g_one, coef * 2.0 / n * c["d"], "content_loss_grad ragged n", what + " gradient")


@pytest.mark.parametrize(("dtype", "n"), _content_params(grad=True), ids=_ids)
def test_content_grad(dtype, n):
    """stv_content_grad: written, and accumulated onto an integer gradient with *coef_dev."""
    c = eh.content_case(n)
    f, t = dev(c["f"], dtype), dev(c["t"], dtype)
    what = f"content grad n={n} {_ids(dtype)}"
    if eh.is_pow2(n):
        g = sentinel((n,), dtype)
        ops.content_grad(f, t, g, 8.0)
        same(g, eh.stored(eh.content_k(8.0, n) * c["d"], dtype), "content_grad", what)
        g = dev(c["prev"], dtype)
        ops.content_grad(f, t, g, n / 8.0, coef_dev=scalar(0.5), flags=ops.ACCUM)
        assert eh.content_k(n / 8.0, n, 0.5) == 0.125
        same(g, eh.stored(0.125 * c["d"] + c["prev"].double(), dtype), "content_grad", what + " accumulated, coef_dev")
    else:
        g = sentinel((n,), dtype)
        ops.content_grad(f, t, g, 8.0)
        within(g, 8.0 * 2.0 / n * c["d"], "content_grad ragged n", what)
        coef = float(2 ** round(np.log2(n)))                   # k near 1: the product is not lost beside prev
        g = dev(c["prev"], dtype)
        ops.content_grad(f, t, g, coef, coef_dev=scalar(0.5), flags=ops.ACCUM)
        within(g, coef * 0.5 * 2.0 / n * c["d"] + c["prev"].double(), "content_grad ragged n", what + " accumulated, coef_dev")


# ---- score combine ------------------------------------------------------------------------------------------------------------

def _combine(c: dict, parts: torch.Tensor | None = None, log: tuple | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    n = len(c["table"])
    losses, scores = sentinel((n,)), sentinel((4,))
    args = (dev(c["parts"] if parts is None else parts), torch.tensor(c["table"], dtype=torch.int32, device=DEV),
            torch.tensor(c["scale"], dtype=F32, device=DEV), c["style_w"], c["content_w"], losses, scores)
    if log is None:
        ops.loss_combine(*args)
    else:
        ops.loss_combine_log(*args, *log)
    return losses, scores


@pytest.mark.parametrize("name", eh.COMBINE_NAMES)
def test_loss_combine(name):
    """The step's own table, 64 terms, empty terms, one long term, offsets out of table order: every output exact."""
    c = eh.combine_case(name)
    losses, scores = _combine(c)
    same(losses, torch.tensor(c["losses"], dtype=F32), "loss_combine", f"combine {name} losses")
    same(scores, torch.tensor(c["scores"], dtype=F32), "loss_combine", f"combine {name} scores")


def test_loss_combine_rejects_65_terms():
    c = eh.combine_case("mixed64")
    table = torch.tensor(c["table"] + [[0, 1, 0]], dtype=torch.int32, device=DEV)
    scale = torch.tensor(c["scale"] + [1.0], dtype=F32, device=DEV)
    losses, scores = sentinel((65,)), sentinel((4,))
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    args = (dev(c["parts"]).data_ptr(), table.data_ptr(), scale.data_ptr(), 65, c["style_w"], c["content_w"], losses.data_ptr(),
            scores.data_ptr())
    assert lib.stv_loss_combine(*args, stream) == eh.STV_ERR_ARG
    assert lib.stv_loss_combine_log(*args, None, 0, None, None, stream) == eh.STV_ERR_ARG
    torch.cuda.synchronize()
    same(losses, sentinel((65,)), "loss_combine", "65 terms: nothing written")
    same(scores, sentinel((4,)), "loss_combine", "65 terms: nothing written")


@pytest.mark.parametrize(("bad", "term"), [(float("nan"), 2), (float("inf"), 5)], ids=["nan-style", "inf-content"])
def test_loss_combine_flags_a_non_finite_score(bad, term):
    c = eh.combine_case("step")
    parts = c["parts"].clone()
    off, cnt, _ = c["table"][term]
    parts[off + cnt // 2] = bad
    losses, scores = _combine(c, parts)
    got, want = losses.cpu(), torch.tensor(c["losses"], dtype=F32)
    keep = torch.arange(len(want)) != term
    same(got[keep], want[keep], "loss_combine", f"{bad} in term {term}: the other terms")
    assert not bool(torch.isfinite(got[term])) and (bad == bad or bool(got[term] != got[term]))
    s = scores.cpu()
    assert float(s[3]) == 0.0 and not bool(torch.isfinite(s[2]))
    clean = 1 if term != 5 else 0                     # the score of the other kind stays exact
    same(s[clean:clean + 1], torch.tensor(c["scores"][clean:clean + 1], dtype=F32), "loss_combine", f"{bad}: the other kind's score")
    _, scores = _combine(c)
    assert float(scores.cpu()[3]) == 1.0


@pytest.mark.parametrize("host", [False, True], ids=["device-ring", "host-ring"])
def test_loss_combine_log_ring_wraps(host):
    """Capacity 4, seven records: the ring holds records 3..6 in the slots record % 4, the count is 7."""
    cap, calls = 4, 7
    c = eh.combine_case("step")
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    if host:
        box = ops.HostMailbox(64 + 3 * cap * 4)
        ring, seq = box.tensor(F32, (3, cap), offset=64), box.tensor(torch.int32, (1,), offset=0)
        ring.fill_(SENTINEL)
        log = (ring, count, seq)
    else:
        ring = sentinel((3, cap))
        log = (ring, count)
    want = []
    for k in range(calls):
        parts = c["parts"].clone()
        parts[0] += 8 * (k + 1)                       # a distinct integer in the first style term
        parts[c["table"][5][0]] += 8 * (calls - k)    # ... and in the content term
        exp = eh.combine_expected(parts, c["table"], c["scale"], c["style_w"], c["content_w"])
        _, scores = _combine(c, parts, log)
        same(scores, torch.tensor(exp["scores"], dtype=F32), "loss_combine_log", f"record {k} scores")
        want.append(exp["scores"][:3])
    assert len({tuple(w) for w in want}) == calls
    torch.cuda.current_stream().synchronize()
    expect = torch.full((3, cap), SENTINEL)
    for k in range(calls - cap, calls):
        expect[:, k % cap] = torch.tensor(want[k], dtype=F32)
    same(ring.cpu().clone(), expect, "loss_combine_log", "ring contents")
    assert int(count.cpu()) == calls
    if host:
        assert int(seq[0]) == calls


@pytest.mark.parametrize("dtype", eh.DTYPES, ids=_ids)
def test_loss_head_chained(dtype):
    """stv_gram_partial -> stv_gram_finish -> stv_content_loss -> stv_loss_combine on exact operands: the scores are the
    float64 evaluation, each rounded to fp32 once where the kernel rounds."""
    H, W, C = eh.CHAIN_STYLE
    n = H * W
    s = eh.finish_case(n, C, "tie")
    assert s["norm"] == float(C * n)
    cc = eh.content_case(eh.CHAIN_CONTENT_N)
    n_style, n_content = eh.gram_loss_parts(C), eh.CONTENT_LOSS_PARTS
    parts = sentinel((n_style + n_content,))
    seed = sentinel((C, C), dtype)
    slabs = ops.gram_partial(dev(s["f"].reshape(H, W, C), dtype))
    ops.gram_finish(slabs, n, C, target=dev(s["target"]), loss_part=parts[:n_style], sgrad=seed, clamp_max=s["clamp"],
                    coef=s["coef"], dtype=dtype, norm=s["norm"])
    ops.content_loss(dev(cc["f"], dtype), dev(cc["t"], dtype), parts[n_style:])
    table = torch.tensor([[0, n_style, 0], [n_style, n_content, 1]], dtype=torch.int32, device=DEV)
    scale = torch.tensor([1.0 / (C * C), 1.0 / eh.CHAIN_CONTENT_N], device=DEV)
    style_w, content_w = 2.0 ** 30, 2.0
    losses, scores = sentinel((2,)), sentinel((4,))
    ops.loss_combine(parts, table, scale, style_w, content_w, losses, scores)
    style = np.float32(float(s["loss"]) / (C * C))
    content = np.float32(float(cc["loss"]) / eh.CHAIN_CONTENT_N)
    assert float(content) * eh.CHAIN_CONTENT_N == float(cc["loss"]) and style > 0
    total = fractions.Fraction(style_w) * fractions.Fraction(float(style)) + fractions.Fraction(content_w) * fractions.Fraction(float(content))
    assert fractions.Fraction(float(total)) == total, "the total must be one rounding away from exact"
    assert 0.01 < style_w * float(style) / (content_w * float(content)) < 100.0, "both kinds must count in the total"
    want = torch.tensor([float(style), float(content), float(np.float32(float(total))), 1.0], dtype=F32)
    same(seed, eh.seed_of(s, dtype), "loss_head_chained", f"chained {_ids(dtype)} seed")
    same(losses, want[:2].clone(), "loss_head_chained", f"chained {_ids(dtype)} losses")
    same(scores, want, "loss_head_chained", f"chained {_ids(dtype)} scores")


# ---- ReLU, max pool, Adam -------------------------------------------------------------------------------------------------------

def _relu_params() -> list:
    return [(d, n) for d in eh.DTYPES for n in eh.RELU_SIZES + (eh.RELU_SIZES_BF16 if d == BF16 else ())]


@pytest.mark.parametrize(("dtype", "n"), _relu_params(), ids=_ids)
def test_relu_forward_backward(dtype, n):
    c = eh.relu_case(n)
    x, dy = dev(c["x"], dtype), dev(c["dy"], dtype)
    what = f"relu n={n} {_ids(dtype)}"
    same(ops.relu_fwd(x, out=sentinel((n,), dtype)), c["y"].to(dtype), "relu", what + " forward")
    same(ops.relu_bwd(x, dy, out=sentinel((n,), dtype)), c["dx"].to(dtype), "relu", what + " backward")
    same(ops.relu_bwd(x, dy, out=dev(c["prev"], dtype), flags=ops.ACCUM), (c["dx"] + c["prev"]).to(dtype), "relu",
         what + " backward accumulated")


def _pool_params() -> list:
    return [(d, s) for d in eh.DTYPES for s in eh.pool_shapes(d)]


def _pool_direct(fn: str, *args) -> None:
    """A shape without a single window has empty tensors, whose pointers torch reports as null: hand the library a
    live (one-vector) buffer in their place."""
    rc = getattr(_lib.load(), fn)(*args, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, f"{fn} returned {rc}"


@pytest.mark.parametrize(("dtype", "hwc"), _pool_params(), ids=_ids)
def test_maxpool_forward_backward(dtype, hwc):
    """Forward, backward, MASK | ACCUM and the byte-map backward; scalar kernels where C fills no whole vector."""
    H, W, C = hwc
    c = eh.pool_case(H, W, C)
    code = ops.dtype_code(dtype)
    x, prev = dev(c["x"], dtype), dev(c["prev"], dtype)
    what = f"maxpool {H}x{W}x{C} {_ids(dtype)}"
    want = {0: c["dx"][False], ops.MASK: c["dx"][True], ops.MASK | ops.ACCUM: c["dx"][True] + c["prev"]}
    vectors = C % eh.k_vec(dtype) == 0
    if H < 2 or W < 2:
        spare = sentinel((16,), dtype)
        _pool_direct("stv_maxpool_fwd", x.data_ptr(), spare.data_ptr(), H, W, C, code)
        for flags, w in want.items():
            dx = prev.clone() if flags & ops.ACCUM else sentinel((H, W, C), dtype)
            _pool_direct("stv_maxpool_bwd", x.data_ptr(), spare.data_ptr(), dx.data_ptr(), H, W, C, flags, code)
            same(dx, w.to(dtype), "maxpool", f"{what} backward flags={flags}: no window")
            if vectors:
                dx = prev.clone() if flags & ops.ACCUM else sentinel((H, W, C), dtype)
                _pool_direct("stv_maxpool_bwd", spare.data_ptr(), spare.data_ptr(), dx.data_ptr(), H, W, C, flags | _lib.POOL_IDX, code)
                same(dx, w.to(dtype), "maxpool", f"{what} byte-map backward flags={flags}: no window")
        same(spare, sentinel((16,), dtype), "maxpool", what + ": nothing written beside dx")
        return
    dy, idx = dev(c["dy"], dtype), dev(c["idx"])
    same(ops.maxpool_fwd(x, out=sentinel((H // 2, W // 2, C), dtype)), c["y"].to(dtype), "maxpool", what + " forward")
    for flags, w in want.items():
        dx = prev.clone() if flags & ops.ACCUM else sentinel((H, W, C), dtype)
        ops.maxpool_bwd(x, dy, out=dx, flags=flags)
        same(dx, w.to(dtype), "maxpool", f"{what} backward flags={flags}")
        if vectors:
            dx = prev.clone() if flags & ops.ACCUM else sentinel((H, W, C), dtype)
            ops.maxpool_bwd_idx(idx, dy, H, W, out=dx, flags=flags)
            same(dx, w.to(dtype), "maxpool", f"{what} byte-map backward flags={flags}")


def test_adam_stride_loop():
    """n = 2048 * 256 + 37: the capped grid takes a second trip.  Every element against optim_ref.AdamRef with the
    tolerances of test_adam_step_matches_oracle (a coverage case, not an exactness claim)."""
    n = eh.ADAM_N
    g = torch.Generator().manual_seed(97)
    x_ref = torch.rand(n, generator=g) * 2 - 1
    x = x_ref.clone().to(DEV)
    ref = optim_ref.AdamRef(x_ref, lr=1e-2)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for step in range(1, 4):
        grad = torch.rand(n, generator=g) * 2 - 1
        ref.step(lambda grad=grad: (None, grad))
        ops.adam_step(x, grad.to(DEV), m, v, step, lr=1e-2)
    got = x.cpu().numpy()
    err = np.abs(got - x_ref.numpy()) / (1e-6 + 1e-5 * np.abs(x_ref.numpy()))
    record_parity("adam stride loop", f"n={n}: |err| / (atol + rtol |x|)", float(err.max()), 1.0, "rtol 1e-5, atol 1e-6")
    np.testing.assert_allclose(got, x_ref.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(m.cpu().numpy(), ref.m.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(v.cpu().numpy(), ref.v.numpy(), rtol=1e-5, atol=1e-6)
