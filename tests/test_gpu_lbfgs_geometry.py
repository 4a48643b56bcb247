"""Every launch geometry of the device L-BFGS sweeps against float64, plus the strided loops of optim.hip.

tests/lbfgs_geom.py explains the references, the bounds and the case list.  Per case (``CASES`` x entry: ``step`` =
``stv_lbfgsc_dots`` + ``stv_lbfgsc_apply``, ``iter`` = ``stv_lbfgsc_iter`` with one iteration per step) 11 calls with
history 6 - the ring fills, call 8 repeats a gradient (no push), three evictions, every history length 0..6 is dealt
over the pair groups - and after EVERY call:

* integers: history length, ring head (= evictions mod 7), iteration count, push and skip flags, and the ring's
  pairs bit for bit against ``lbfgs_geom.Mirror``;
* products: every inner product the call defines against ``expected_dots`` (float64, torch on the device) within
  ``n * 2**-52 * sum|a_i b_i|``; the maxima and the unused fourth product exactly;
* direction and update: ``d`` against ``expected_direction`` with the coefficients the state block holds, ``prev_g``
  equal to ``g``, ``x`` within one fp32 ulp of ``x + t*d``;
* padding: ``[n, nn)`` of ``d``, ``prev_g`` and every ``S`` / ``Y`` row exactly zero (the kernels read the pad
  unguarded and rely on that), the 8 sentinel floats behind ``x`` untouched (``g`` has NaN behind it), nothing NaN.

Each case first asserts, through ``ops.lbfgs_geometry``, that its ``n`` still reaches the class in its name.

Then: two shards of different classes with the host-side all-reduce; the operation-ordered form (optim.hip) over
three trips of its 131072-element stride, element-wise; one Adam step over more than two trips of its 524288-element
grid.  Worst ``error / bound`` per case goes to the parity table.
"""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

from oracle import optim_ref
from style_transfer_visualizer_amd import ops
from tests import lbfgs_geom as lg
from tests.conftest import record_parity
from tests.lbfgs_multi_util import objective

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
H = lg.HISTORY
SENTINEL = -77.0


def _tailed(n: int, fill: float, tail: float) -> tuple[torch.Tensor, torch.Tensor]:
    """(buffer of n + 8, its first n elements): the 8 floats behind the vector hold ``tail``."""
    buf = torch.full((n + 8,), tail, device=DEV)
    buf[:n] = fill
    return buf, buf[:n]


class _Device:
    """A compact L-BFGS over ``sum(sizes)`` elements as one shard or several (inner products summed on the host the
    way ``HipLBFGS(shard_group=)`` all-reduces them: SUM, max|g| with MAX).  Asserts each shard's geometry class."""

    def __init__(self, sizes: list[int], classes: list[tuple[int, int, int]], name: str) -> None:
        self.sizes, self.n = sizes, sum(sizes)
        self.bounds = [0, *np.cumsum(sizes).tolist()]
        self.geo, self.positions = [], []
        for b, k, want in zip(self.bounds[:-1], sizes, classes, strict=True):
            geo = ops.lbfgs_geometry(k, H)
            assert lg.geometry_class(geo) == want, \
                (f"{name}: n = {k} launches (tile A, pair groups, tile B) = {lg.geometry_class(geo)}, not the {want} this "
                 f"case is here for - a threshold was retuned (move the case) or one of {lg.OVERRIDES} is set")
            self.geo.append(geo)
            self.positions += [b + p for p in lg.tail_positions(k, geo["tile_a"], geo["tile_b"])]
        self.x_buf, self.x, self.g_buf, self.g = [], [], [], []
        for k in sizes:
            xb, x = _tailed(k, 0.0, SENTINEL)
            gb, g = _tailed(k, 0.0, float("nan"))
            self.x_buf.append(xb), self.x.append(x), self.g_buf.append(gb), self.g.append(g)
        self.st = [ops.lbfgs_alloc(k, H, DEV, compact=True) for k in sizes]
        self.views = [ops.lbfgs_views(work, k, H) for (_, work), k in zip(self.st, sizes, strict=True)]
        self.calls = 0

    def cat(self, what: str) -> torch.Tensor:
        """x, g, d or prev_g over ``[0, n)`` of every shard, concatenated (a copy)."""
        if what in ("x", "g"):
            return torch.cat(getattr(self, what))
        return torch.cat([v[what][:k] for v, k in zip(self.views, self.sizes, strict=True)])

    def row(self, ring: str, slot: int) -> torch.Tensor:
        return torch.cat([v[ring][slot, :k] for v, k in zip(self.views, self.sizes, strict=True)])

    def set_gradient(self, g: torch.Tensor) -> None:
        for gi, b, e in zip(self.g, self.bounds[:-1], self.bounds[1:], strict=True):
            gi.copy_(g[b:e])

    def call(self, entry: str, loss: torch.Tensor) -> torch.Tensor:
        """One optimizer call; returns the (combined) inner-product block it ran on, as a copy."""
        m_max = min(self.calls, H)
        self.calls += 1
        if entry == "iter":
            (state, work), = self.st
            ops.lbfgs_iter(self.x[0], self.g[0], loss.reshape(1).to(DEV), state, work, H, m_max, 1, 1.0)
            return ops.lbfgs_dots_view(work, self.n, H)[0].clone()
        blocks = [ops.lbfgs_dots(gi, state, work, H, m_max) for gi, (state, work) in zip(self.g, self.st, strict=True)]
        imax = ops.lbfgs_dots_view(self.st[0][1], self.sizes[0], H)[1]
        assert imax == lg.SC and blocks[0].numel() == lg.COUNT
        total = torch.stack(blocks).sum(0)
        total[imax] = torch.stack([v[imax] for v in blocks]).max()
        if len(blocks) > 1:
            for v in blocks:
                v.copy_(total)
        for xi, gi, (state, work) in zip(self.x, self.g, self.st, strict=True):
            ops.lbfgs_apply(xi, gi, state, work, H, 1.0)
        return total

    def state(self) -> tuple[dict, torch.Tensor]:
        """(integers, block as fp32) - the same on every shard, to the bit: each runs the same scalar recursion."""
        blocks = [s.cpu().view(torch.int32) for s, _ in self.st]
        for b in blocks[1:]:
            assert torch.equal(b, blocks[0]), "shards disagree on the state block"
        return lg.read_state(self.st[0][0])

    def check_padding(self, where: str) -> None:
        for k, geo, v, xb, x in zip(self.sizes, self.geo, self.views, self.x_buf, self.x, strict=True):
            assert v["d"].numel() == geo["nn"]
            bad = [name for name in ("d", "prev_g", "S", "Y") if int(torch.count_nonzero(v[name][..., k:]))]
            assert not bad, f"{where}: the pad [n, nn) of {bad} is not zero"
            bad = [name for name in ("d", "prev_g", "S", "Y") if not bool(torch.isfinite(v[name]).all())]
            assert not bad and bool(torch.isfinite(x).all()), f"{where}: non-finite values in {bad or 'x'}"
            assert bool((xb[k:] == SENTINEL).all()), f"{where}: the floats behind x were written"


def _run(name: str, sizes: list[int], classes: list[tuple[int, int, int]], entry: str, calls: int,
         repeat_at: int | None) -> None:
    dev = _Device(sizes, classes, name)
    n = dev.n
    f = objective(n)
    mirror = lg.Mirror(H)
    worst_dots = worst_dir = 0.0
    misrounded = 0            # elements of d that are not fl32 of the float64 combination (reported, not asserted)
    lens = set()
    for call in range(1, calls + 1):
        where = f"{name} {entry} call {call}"
        x_before = dev.cat("x")
        loss, g_raw = f(x_before)
        if call != repeat_at:
            dev.set_gradient(lg.floor_gradient(g_raw, dev.positions).to(DEV))
        g = dev.cat("g")
        ints0, fl0 = dev.state()
        d_before, t_before = dev.cat("d"), float(fl0[lg.F_T])
        y_c, s_c = mirror.candidate(g, d_before, t_before)
        exp = lg.expected_dots(mirror.pairs, g, y_c, s_c, with_dtmax=entry == "iter")
        got = dev.call(entry, loss)
        ints, fl = dev.state()
        # ---- products ------------------------------------------------------------------------------------
        ratio, bad = lg.compare_dots(got, exp, n)
        assert not bad, f"{where} ({len(mirror.pairs)} pairs): " + "; ".join(bad)
        worst_dots = max(worst_dots, ratio)
        # ---- integers: what torch's control flow does with the float64 products, and the mirror's lists --------
        want = exp["want"].cpu()
        skip = float(want[lg.SC].float()) <= 1e-7
        pushed = (not skip) and mirror.n_iter >= 1 and float(want[lg.SC + 5].float()) > 1e-10
        assert (ints["skip"], ints["pushed"]) == (int(skip), int(pushed)), f"{where}: {ints}, expected skip {skip} push {pushed}"
        if repeat_at is not None:
            assert not skip and pushed == (call not in (1, repeat_at)), f"{where}: the script expects another push pattern"
        mirror.commit(g, y_c, s_c, pushed, skip)
        assert (ints["n_iter"], ints["hist_len"], ints["head"]) == (mirror.n_iter, len(mirror.pairs), mirror.head), \
            f"{where}: {ints} vs iterations {mirror.n_iter}, {len(mirror.pairs)} pairs, {mirror.evictions} evictions"
        lens.add(ints["hist_len"])
        for j, (s, y) in enumerate(mirror.pairs):
            slot = (mirror.head + j) % (H + 1)
            assert torch.equal(dev.row("S", slot), s) and torch.equal(dev.row("Y", slot), y), \
                f"{where}: pair {j} (ring slot {slot}) differs from fl32(d*t) / fl32(g - prev_g)"
        # ---- direction and update ------------------------------------------------------------------------------
        x_after = dev.cat("x")
        if skip:
            assert torch.equal(x_after, x_before) and torch.equal(dev.cat("d"), d_before)
        else:
            m = len(mirror.pairs)
            cg, cs, cy = lg.coefficients(fl, mirror.head, m, H)
            d_want, A = lg.expected_direction(g, mirror.pairs, cg, cs, cy)
            d = dev.cat("d")
            err, tol = (d.double() - d_want).abs(), lg.direction_tolerance(d_want, A, m)
            over = int((err > tol).sum())
            k = int((err - tol).argmax())
            assert over == 0, (f"{where}: {over} elements of d off the float64 combination, worst at {k}: {float(d[k])!r} vs "
                               f"{float(d_want[k])!r}, error {float(err[k]):.3e} > {float(tol[k]):.3e}")
            worst_dir = max(worst_dir, float(torch.where(tol > 0, err / tol, torch.zeros_like(err)).max()))
            misrounded += int((d != d_want.float()).sum())
            assert torch.equal(dev.cat("prev_g"), g), f"{where}: prev_g is not g"
            if ints["no_update"]:
                assert torch.equal(x_after, x_before), f"{where}: no_update, but the image moved"
            else:
                x_want = x_before.double() + float(fl[lg.F_T]) * d.double()
                off = (x_after.double() - x_want).abs() > lg.ulp32(x_want)
                assert not bool(off.any()), f"{where}: {int(off.sum())} elements of x more than an ulp from x + t*d"
        dev.check_padding(where)
    if repeat_at is not None:
        assert mirror.evictions >= 3 and lens == set(range(H + 1)), f"{name}: {mirror.evictions} evictions, lengths {lens}"
    cls = " + ".join(f"({a},{p},{b})" for a, p, b in classes)
    record_parity(f"lbfgs geometry {name} {entry}", "products, error / bound", worst_dots, 1.0, f"class {cls}; {calls} calls")
    # (a correctly rounded d reaches 2**-24 |want| wherever |want| sits just above a power of two: a ratio near 1 is the
    #  fp32 rounding itself; the share of the double accumulation shows in the count of elements rounded the other way)
    record_parity(f"lbfgs geometry {name} {entry}", "direction, error / tolerance", worst_dir, 1.0,
                  f"class {cls}; {misrounded} of {calls * n} elements differ from fl32(float64)")


@pytest.mark.parametrize("entry", ["step", "iter"])
@pytest.mark.parametrize(("name", "n", "expected"), lg.CASES, ids=[c[0] for c in lg.CASES])
def test_sweeps_match_float64_in_every_launch_geometry(name, n, expected, entry):
    _run(name, [n], [expected], entry, lg.CALLS, lg.REPEAT_AT)


def test_shards_of_different_geometry_classes():
    """530000 + 4099 elements as two shards, (2048, 1, 2048) beside (1024, 4, 1024): the combined inner products
    against ``expected_dots`` of the whole vector (bound for the whole n), the concatenated image against the
    direction / update assertions; 9 calls."""
    _run("n530000+4099", [530000, 4099], [(2048, 1, 2048), (1024, 4, 1024)], "step", 9, None)


# ---------------------------------------------------------------------------------- optim.hip: the strided loops
def _twoloop_views(work: torch.Tensor, n: int, history: int) -> dict:
    """The operation-ordered form's workspace (optim.hip ``carve``): d, prev_g, S, Y at pitch align_up(n, 64)."""
    pitch = (n + 63) // 64 * 64
    rows = history + 1
    ring = work[2 * pitch: 2 * pitch + 2 * rows * pitch].view(2, rows, pitch)
    return {"d": work[:pitch], "prev_g": work[pitch: 2 * pitch], "S": ring[0], "Y": ring[1]}


def test_twoloop_form_element_wise_over_three_stride_trips():
    """``stv_lbfgs_step`` at n = 262144 + 77: every vector loop makes three trips of its 512 x 256 stride, the last one
    ragged.  After each of 9 steps: prev_g = g, the candidate pair is fl32(g - prev_g) / fl32(d * t) to the bit, x is
    within an ulp of x + t*d, and nothing was written behind n."""
    n, history = 262144 + 77, 6
    f = objective(n)
    x_buf, x = _tailed(n, 0.0, SENTINEL)
    g_buf, g = _tailed(n, 0.0, float("nan"))
    state, work = ops.lbfgs_alloc(n, history, DEV, compact=False)
    v = _twoloop_views(work, n, history)

    def read():
        raw = state.cpu()
        i, fl = raw.view(torch.int32), raw.view(torch.float32)
        return {"n_iter": int(i[0]), "hist_len": int(i[1]), "head": int(i[2]), "skip": int(i[3]), "no_update": int(i[4]),
                "t": float(fl[6])}
    for step in range(1, 10):
        where = f"twoloop step {step}"
        g.copy_(f(x)[1].to(DEV))
        s0 = read()
        slot = (s0["head"] + s0["hist_len"]) % (history + 1)
        x_before, d_before, pg_before = x.clone(), v["d"][:n].clone(), v["prev_g"][:n].clone()
        ops.lbfgs_step(x, g, state, work, history, min(step - 1, history), 1.0, compact=False)
        y_row, s_row = v["Y"][slot, :n].clone(), v["S"][slot, :n].clone()      # (the candidate's slot, pushed or not)
        s1 = read()
        assert (s1["skip"], s1["no_update"], s1["n_iter"]) == (0, 0, step), f"{where}: {s1}"
        assert s1["hist_len"] == min(step - 1, history) and s1["head"] == max(0, step - 1 - history), f"{where}: {s1}"
        assert torch.equal(v["prev_g"][:n], g), f"{where}: prev_g is not g"
        assert torch.equal(y_row, g - pg_before), f"{where}: candidate y is not fl32(g - prev_g)"
        assert torch.equal(s_row, d_before * torch.tensor(s0["t"], device=DEV)), f"{where}: candidate s is not fl32(d * t)"
        x_want = x_before.double() + s1["t"] * v["d"][:n].double()
        off = (x.double() - x_want).abs() > lg.ulp32(x_want)
        assert not bool(off.any()), f"{where}: {int(off.sum())} elements of x more than an ulp from x + t*d"
        assert float((x - x_before).abs().max()) > 0.0
        assert bool((x_buf[n:] == SENTINEL).all()), f"{where}: the floats behind x were written"
        for name in ("d", "prev_g", "S", "Y"):
            assert int(torch.count_nonzero(v[name][..., n:])) == 0, f"{where}: {name} written behind n"
            assert bool(torch.isfinite(v[name]).all()), f"{where}: non-finite {name}"


def test_adam_step_over_more_than_two_grid_trips():
    """``adam_kernel`` caps its grid at 2048 blocks (524288 elements a trip): n = 2 x 524288 + 3 makes two full trips and
    a third of 3 elements.  One step (number 7) from random x, g, m and v > 0 against ``AdamRef``'s arithmetic in
    float64 on the same inputs; the tolerances of test_gpu_ops.py::test_adam_step_matches_oracle on x, m and v."""
    n = 2 * 2048 * 256 + 3
    gen = torch.Generator().manual_seed(17)
    host = {"x": torch.randn(n, generator=gen), "g": torch.randn(n, generator=gen), "m": 0.1 * torch.randn(n, generator=gen),
            "v": 0.01 + torch.rand(n, generator=gen)}
    ref = optim_ref.AdamRef(host["x"].double(), lr=1e-2)
    ref.m, ref.v, ref.t = host["m"].double(), host["v"].double(), 6
    ref.step(lambda: (None, host["g"].double()))
    assert ref.t == 7
    bufs = {}
    for k, t in host.items():
        bufs[k] = _tailed(n, 0.0, SENTINEL)
        bufs[k][1].copy_(t)
    ops.adam_step(bufs["x"][1], bufs["g"][1], bufs["m"][1], bufs["v"][1], 7, lr=1e-2)
    for k, want in (("x", ref.x), ("m", ref.m), ("v", ref.v)):
        np.testing.assert_allclose(bufs[k][1].cpu().double().numpy(), want.numpy(), rtol=1e-5, atol=1e-6, err_msg=k)
    assert torch.equal(bufs["g"][1].cpu(), host["g"])
    assert float((bufs["x"][1].cpu() - host["x"]).abs().max()) > 1e-3          # (the step did move the image)
    for k, (buf, _) in bufs.items():
        assert bool((buf[n:] == SENTINEL).all()), f"the floats behind {k} were written"
    assert math.isfinite(float(bufs["x"][1].sum()))
