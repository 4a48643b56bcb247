"""Float64 references for the sweeps of the inner-product L-BFGS (csrc/lbfgs_compact.hip), and the sizes to run them at.

The launch shape of a step changes with the vector length ``n``: sweep A's tile (``pass_a_kernel<1|2|4>`` /
``pass_a_iter_kernel<1|2|4>``), the number of workgroups a tile's history pairs are dealt to (1 or 4) and sweep B's
tile (``pass_b_kernel<1|2|4>``) - six reachable classes.  ``CASES`` names the smallest and the raggedest ``n`` of each;
tests/test_gpu_lbfgs_geometry.py asserts, through ``ops.lbfgs_geometry``, that each still reaches the class in its
name, so retuning a threshold fails a test instead of silently losing coverage.

What the sweeps compute is observable directly, and is compared here rather than the final update:

* ``stv_lbfgsc_dots`` / ``stv_lbfgsc_iter`` leave every inner product of the step as a double in the workspace.  The
  history vectors, the gradient and the candidate pair ``y_c = g - prev_g``, ``s_c = d * t`` (one fp32 operation each:
  reproducible to the bit by ``Mirror``) are fp32, so every product is exact in double and the kernel's value and
  ``expected_dots`` are two float64 summations of the SAME numbers in different orders.  Each is within
  ``(n - 1) * 2**-53 * A`` of the exact sum, ``A = sum |a_i * b_i|`` (Higham, Accuracy and Stability, eq. 4.4: any
  order), hence ``|got - want| <= n * 2**-52 * A``: derived, not measured.  Maxima and the zero entry are exact.
* Sweep B's direction is ``fl32(cg*g + sum_j cs_j*s_j + cy_j*y_j)`` with the fp32 coefficients of the state block,
  accumulated in double: ``2m`` roundings of partial sums bounded by ``A_k`` (the sum of the absolute terms), then one
  rounding to fp32.  ``expected_direction`` sums the same exact products with a compensated (TwoSum) accumulation, so
  its own error is below ``2 * 2**-53 * A_k`` and the tolerance ``2**-24 * |want| + (2m + 2) * 2**-53 * A_k`` is a bound.

A tolerance that could swallow a dropped tail element would make the test pointless: ``floor_gradient`` keeps the
gradient away from zero at the last element and at the first element of the last tile, and ``sensitivity_margin``
(asserted for every case on the host, tests/test_lbfgs_geom_host.py) shows that leaving either element out of
``g.g`` or of any ``s_j.g`` moves the value by more than four times its tolerance.
"""
from __future__ import annotations

import torch

MAX_HIST = 128
NSCAL = 8
COUNT = 5 * MAX_HIST + NSCAL
SC = 5 * MAX_HIST                 # first scalar: max|g|, |g|_1, g.g, g.s_c, g.y_c, s_c.y_c, y_c.y_c, max|s_c| (iter only)
SC_DTMAX = 7
HISTORY = 6                       # ring of 7 slots: fills and evicts within a dozen calls
# state block of lbfgs_compact.hip: 8 ints, 8 floats, then ro / cs / cy by ring slot
F_T, F_CG, F_RO = 8, 14, 16
F_CS, F_CY = F_RO + MAX_HIST + 1, F_RO + 2 * (MAX_HIST + 1)
FLOOR = 1.0                       # (0.25 left margins of 2-4 at the 1M sizes; 1.0 leaves 50 and more)
CALLS, REPEAT_AT = 11, 8          # call 8 repeats the gradient of call 7: y = 0, nothing is pushed

# (name, n, (tile A, pair groups, tile B)) - the class the name promises
CASES = [
    ("n1_1024x4_1024", 1, (1024, 4, 1024)),                    # ld4_guard: one element of a partial vector
    ("n3_1024x4_1024", 3, (1024, 4, 1024)),                    # ld4_guard: three
    ("n4096_1024x4_1024", 4096, (1024, 4, 1024)),              # exactly one padded block, no pad
    ("n4099_1024x4_1024", 4099, (1024, 4, 1024)),              # one block plus 3
    ("n258048_1024x4_1024", 258048, (1024, 4, 1024)),          # 252 tiles: the last count with 4 pair groups
    ("n258049_1024x1_1024", 258049, (1024, 1, 1024)),          # nn = 262144, 256 tiles
    ("n524287_1024x1_1024", 524287, (1024, 1, 1024)),          # last n on the thin tile
    ("n524288_2048x1_2048", 524288, (2048, 1, 2048)),          # U = 2, exact
    ("n524293_2048x1_2048", 524293, (2048, 1, 2048)),          # U = 2, ragged
    ("n786431_2048x1_2048", 786431, (2048, 1, 2048)),          # last n before tile A grows
    ("n786435_4096x4_2048", 786435, (4096, 4, 2048)),          # U = 4 ragged, 193 tiles
    ("n1048575_4096x1_2048", 1048575, (4096, 1, 2048)),        # 256 tiles with sweep B still on 2048
    ("n1048576_4096x1_4096", 1048576, (4096, 1, 4096)),        # U = 4 in both sweeps, exact
    ("n1048581_4096x1_4096", 1048581, (4096, 1, 4096)),        # ... ragged
]
OVERRIDES = "STV_LBFGS_TILE, STV_LBFGS_TILE_B, STV_LBFGS_PGROUPS"


def threshold_mirror(n: int) -> dict:
    """tile_floats / step_geom / tile_floats_b of lbfgs_compact.hip restated (no overrides).  Only the source of the
    ``expected`` column of ``CASES``: the GPU test asserts against the library's own answer."""
    nn = (n + 4095) // 4096 * 4096
    tile_a = 4096 if n >= 4096 * 192 else 2048 if n >= 2048 * 256 else 1024
    ntiles = nn // tile_a
    pgroups = 1 if ntiles >= 256 else min(4, (768 + ntiles - 1) // ntiles)
    tile_b = 4096 if n >= 4096 * 256 else 2048 if n >= 2048 * 256 else 1024
    return {"nn": nn, "tile_a": tile_a, "ntiles": ntiles, "pgroups": pgroups, "tile_b": tile_b}


def geometry_class(geom: dict) -> tuple[int, int, int]:
    return geom["tile_a"], geom["pgroups"], geom["tile_b"]


def tail_positions(n: int, tile_a: int, tile_b: int) -> list[int]:
    """The elements a wrong tail would drop first: the last one, and the first of the last tile (of either sweep)."""
    return sorted({n - 1, (n - 1) // tile_a * tile_a, (n - 1) // tile_b * tile_b})


def floor_gradient(g: torch.Tensor, positions: list[int]) -> torch.Tensor:
    """``g`` with ``|g| >= FLOOR`` at ``positions``: ``FLOOR * sign(g)`` is added there.  Added always, not only below
    the floor: the result stays monotone in the gradient, so ``y.s > 0`` survives it even where the two positions are
    the whole vector (n = 1: adding it below the floor only left two of the eleven calls without a push)."""
    g = g.clone()
    idx = torch.tensor(positions, dtype=torch.long, device=g.device)
    v = g[idx]
    g[idx] = v + torch.where(v < 0, -FLOOR, FLOOR).to(v.dtype)
    return g


class Mirror:
    """An independent copy of the history.  Per call it is fed the gradient, the ``d`` and ``t`` the optimizer held
    BEFORE the call and the ``pushed`` / ``skip`` flags after it; it forms the candidate pair in fp32 (one operation per
    element each, so bit-reproducible), keeps the logical list of pairs (oldest first) and counts evictions."""

    def __init__(self, history: int) -> None:
        self.history = history
        self.pairs: list[tuple[torch.Tensor, torch.Tensor]] = []       # (s_j, y_j), oldest first
        self.prev_g: torch.Tensor | None = None
        self.evictions = 0
        self.n_iter = 0

    def candidate(self, g: torch.Tensor, d: torch.Tensor, t: float) -> tuple[torch.Tensor, torch.Tensor]:
        prev = self.prev_g if self.prev_g is not None else torch.zeros_like(g)
        y_c = g - prev
        s_c = d * torch.tensor(t, dtype=torch.float32, device=g.device)
        return y_c, s_c

    def commit(self, g: torch.Tensor, y_c: torch.Tensor, s_c: torch.Tensor, pushed: bool, skip: bool) -> None:
        if skip:
            assert not pushed
            return
        self.n_iter += 1
        if pushed:
            assert self.n_iter > 1
            self.pairs.append((s_c, y_c))
            if len(self.pairs) > self.history:
                self.pairs.pop(0)
                self.evictions += 1
        self.prev_g = g.clone()

    @property
    def head(self) -> int:
        return self.evictions % (self.history + 1)


def _dot(a: torch.Tensor, b: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    p = a * b                     # float64 product of two fp32 values: exact
    return p.sum(), p.abs().sum()


def expected_dots(pairs, g: torch.Tensor, y_c: torch.Tensor, s_c: torch.Tensor, *, with_dtmax: bool = False) -> dict:
    """The workspace block of inner products in float64, for the pairs held BEFORE the push.  Returns tensors of
    ``COUNT`` entries on ``g``'s device: ``want``, ``A`` (``sum |a_i b_i|`` beside every sum), ``exact`` (entries
    compared with ``==``: the maxima and the unused fourth product) and ``scope`` (entries the call defines)."""
    dev = g.device
    want = torch.zeros(COUNT, dtype=torch.float64, device=dev)
    A = torch.zeros(COUNT, dtype=torch.float64, device=dev)
    exact = torch.zeros(COUNT, dtype=torch.bool, device=dev)
    scope = torch.zeros(COUNT, dtype=torch.bool, device=dev)
    g64, y64, s64 = g.double(), y_c.double(), s_c.double()
    for jj, (s, y) in enumerate(pairs):
        sj, yj = s.double(), y.double()
        for k, (a, b) in ((0, (sj, g64)), (1, (yj, g64)), (2, (sj, y64)), (4, (yj, y64))):
            want[5 * jj + k], A[5 * jj + k] = _dot(a, b)
        exact[5 * jj + 3] = True                                   # y_j . s_c is never read: a zero
        scope[5 * jj: 5 * jj + 5] = True
    want[SC] = g64.abs().max()
    exact[SC] = True
    want[SC + 1] = A[SC + 1] = g64.abs().sum()
    for k, (a, b) in ((2, (g64, g64)), (3, (g64, s64)), (4, (g64, y64)), (5, (s64, y64)), (6, (y64, y64))):
        want[SC + k], A[SC + k] = _dot(a, b)
    scope[SC: SC + 7] = True
    if with_dtmax:
        want[SC + SC_DTMAX] = s64.abs().max()
        exact[SC + SC_DTMAX] = True
        scope[SC + SC_DTMAX] = True
    return {"want": want, "A": A, "exact": exact, "scope": scope}


def dots_tolerance(A: torch.Tensor, n: int) -> torch.Tensor:
    return float(n) * 2.0 ** -52 * A


def compare_dots(got: torch.Tensor, exp: dict, n: int) -> tuple[float, list[str]]:
    """(worst error / bound over the sums in scope, list of violations).  One transfer to the host."""
    want, A, exact, scope = (exp[k] for k in ("want", "A", "exact", "scope"))
    got = got.to(want.device)
    err = (got - want).abs()
    bound = dots_tolerance(A, n)
    table = torch.stack([got, want, err, bound, exact.double(), scope.double()]).cpu()
    worst, bad = 0.0, []
    for i in torch.nonzero(table[5]).flatten().tolist():
        gi, wi, ei, bi = (float(table[r, i]) for r in range(4))
        name = f"entry {i} ({'pair %d product %d' % divmod(i, 5) if i < SC else 'scalar %d' % (i - SC)})"
        if gi != gi:
            bad.append(f"{name}: NaN")
        elif table[4, i]:
            if gi != wi:
                bad.append(f"{name}: {gi!r} != {wi!r} (exact)")
        else:
            if ei > bi:
                bad.append(f"{name}: got {gi!r} want {wi!r}, error {ei:.3e} > bound {bi:.3e}")
            if bi > 0.0:
                worst = max(worst, ei / bi)
    return worst, bad


def coefficients(floats: torch.Tensor, head: int, m: int, history: int) -> tuple[float, list[float], list[float]]:
    """(cg, cs by logical index, cy by logical index) from the state block read as fp32 (``cs`` / ``cy`` are stored by
    ring slot: logical pair ``j`` sits in slot ``(head + j) % (history + 1)``)."""
    slots = [(head + j) % (history + 1) for j in range(m)]
    return (float(floats[F_CG]), [float(floats[F_CS + s]) for s in slots], [float(floats[F_CY + s]) for s in slots])


def expected_direction(g: torch.Tensor, pairs, cg: float, cs, cy) -> tuple[torch.Tensor, torch.Tensor]:
    """float64 ``cg*g + sum_j (cs_j*s_j + cy_j*y_j)`` over the logical pairs (``cs`` / ``cy`` by logical index, see
    ``coefficients``), and beside each element ``A_k``, the sum of the absolute terms.  Every term is an exact
    product; they are added with a compensated sum, so ``want`` is within ``~2**-53 |want|`` of the exact value."""
    terms = [g.double() * cg]
    for (s, y), a, b in zip(pairs, cs, cy, strict=True):
        terms += [s.double() * a, y.double() * b]
    total = terms[0].clone()
    comp = torch.zeros_like(total)
    A = terms[0].abs()
    for x in terms[1:]:
        t = total + x
        bp = t - total
        comp += (total - (t - bp)) + (x - bp)                       # TwoSum: the rounding error of total + x, exactly
        total = t
        A += x.abs()
    return total + comp, A


def direction_tolerance(want: torch.Tensor, A: torch.Tensor, m: int) -> torch.Tensor:
    return 2.0 ** -24 * want.abs() + (2 * m + 2) * 2.0 ** -53 * A


def ulp32(v: torch.Tensor) -> torch.Tensor:
    """Spacing of fp32 at ``|v|`` (float64 in, float64 out)."""
    f = v.abs().float()
    _, e = torch.frexp(f)
    e = torch.where(f == 0, torch.full_like(e, -200), e)
    return torch.ldexp(torch.ones_like(v), (e - 24).clamp_min(-149))


def sensitivity_margin(pairs, g: torch.Tensor, positions: list[int]) -> float:
    """Smallest ``(change of the value when one element is left out) / (4 x tolerance)`` over ``g.g`` and every
    ``s_j.g`` and the elements ``positions``.  Above 1: a sweep that dropped the element could not pass."""
    n = g.numel()
    g64 = g.double()
    margin = float("inf")
    for a in [g64] + [s.double() for s, _ in pairs]:
        p = a * g64
        full, tol = float(p.sum()), float(dots_tolerance(p.abs().sum(), n))
        for e in positions:
            without = float(p[:e].sum() + p[e + 1:].sum())
            margin = min(margin, abs(full - without) / (4.0 * tol))
    return margin


def read_state(state: torch.Tensor) -> tuple[dict, torch.Tensor]:
    """(integer fields, the whole block as fp32 on the host) of a compact state block."""
    raw = state.cpu()
    i = raw.view(torch.int32)
    ints = {"n_iter": int(i[0]), "hist_len": int(i[1]), "head": int(i[2]), "skip": int(i[3]), "no_update": int(i[4]),
            "pushed": int(i[5])}
    return ints, raw.view(torch.float32)
