"""Host checks of tests/lbfgs_geom.py: the references and the case list that tests/test_gpu_lbfgs_geometry.py holds
the L-BFGS sweeps to must themselves be right, and sharp enough to notice one dropped element."""
from __future__ import annotations

import math

import pytest
import torch

from style_transfer_visualizer_amd import ops
from tests import lbfgs_geom as lg
from tests.lbfgs_multi_util import TracedLbfgs, objective


def drive(n: int, calls: int, repeat_at: int, history: int = lg.HISTORY, on_call=None) -> tuple[lg.Mirror, TracedLbfgs, list]:
    """The scripted run of the GPU test with the fp32 ``TracedLbfgs`` twin in the device's place: the quartic's gradient
    at the twin's iterate (floored at the tail positions), call ``repeat_at`` repeats the previous gradient.
    ``on_call(mirror_before_push, twin_before, g, y_c, s_c)`` runs in front of every step.  Returns the mirror, the twin
    and ``(hist_len, pushed)`` per call."""
    geo = lg.threshold_mirror(n)
    pos = lg.tail_positions(n, geo["tile_a"], geo["tile_b"])
    f = objective(n)
    twin = TracedLbfgs(torch.zeros(n), history_size=history)
    mirror = lg.Mirror(history)
    g_prev, trace = None, []
    for call in range(1, calls + 1):
        g = g_prev.clone() if call == repeat_at else lg.floor_gradient(f(twin.x)[1], pos)
        d = twin.d if twin.d is not None else torch.zeros(n)
        t = float(twin.t) if twin.t is not None else 0.0
        y_c, s_c = mirror.candidate(g, d, t)
        if on_call:
            on_call(mirror, twin, g, y_c, s_c)
        twin.step(lambda g=g: (torch.tensor(0.0), g.clone()))
        entry = twin.log[-1]
        mirror.commit(g, y_c, s_c, bool(entry.get("pushed")), entry["kind"] == "stop")
        trace.append((len(mirror.pairs), bool(entry.get("pushed"))))
        g_prev = g
    return mirror, twin, trace


def test_mirror_keeps_the_twins_history_bit_for_bit():
    """n = 4099, history 6, 14 steps, step 9 repeats a gradient: after every step the mirror's pairs are the twin's
    ``old_stps`` / ``old_dirs`` to the bit and it has counted the twin's evictions; in front of every step
    ``expected_dots`` agrees with a plain float64 ``torch.dot`` within the bound it is used with."""
    n, history = 4099, lg.HISTORY
    seen = {"evictions": 0, "len_before": 0, "calls": 0}

    def on_call(mirror, twin, g, y_c, s_c):
        # what the previous step did to the twin's lists
        if seen["calls"]:
            pushed = bool(twin.log[-1].get("pushed"))
            seen["evictions"] += int(pushed and seen["len_before"] == history)
        seen["len_before"] = len(twin.old_dirs)
        seen["calls"] += 1
        assert mirror.evictions == seen["evictions"] and len(mirror.pairs) == len(twin.old_dirs)
        for (s, y), ts, ty in zip(mirror.pairs, twin.old_stps, twin.old_dirs, strict=True):
            assert torch.equal(s, ts) and torch.equal(y, ty), f"call {seen['calls']}: pair differs from the twin's"
        exp = lg.expected_dots(mirror.pairs, g, y_c, s_c, with_dtmax=True)
        got = torch.zeros(lg.COUNT, dtype=torch.float64)
        g64, y64, s64 = g.double(), y_c.double(), s_c.double()
        for jj, (s, y) in enumerate(mirror.pairs):
            got[5 * jj + 0], got[5 * jj + 1] = torch.dot(s.double(), g64), torch.dot(y.double(), g64)
            got[5 * jj + 2], got[5 * jj + 4] = torch.dot(s.double(), y64), torch.dot(y.double(), y64)
        got[lg.SC + 0], got[lg.SC + 1], got[lg.SC + 2] = g.abs().max().double(), g64.abs().sum(), torch.dot(g64, g64)
        got[lg.SC + 3], got[lg.SC + 4] = torch.dot(g64, s64), torch.dot(g64, y64)
        got[lg.SC + 5], got[lg.SC + 6], got[lg.SC + 7] = torch.dot(s64, y64), torch.dot(y64, y64), s_c.abs().max().double()
        assert int(exp["scope"].sum()) == 5 * len(mirror.pairs) + 8
        _, bad = lg.compare_dots(got, exp, n)
        assert not bad, f"call {seen['calls']}: {bad}"
        # ... and the comparison does notice an error just over the bound, and a non-zero "zero"
        if mirror.pairs:
            off = got.clone()
            off[1] += 2.0 * float(lg.dots_tolerance(exp["A"][1], n))
            off[3] = 1e-300
            assert len(lg.compare_dots(off, exp, n)[1]) == 2

    mirror, twin, trace = drive(n, 14, 9, on_call=on_call)
    assert [p for _, p in trace] == [False] + [True] * 7 + [False] + [True] * 5
    assert mirror.evictions == 12 - history and mirror.head == mirror.evictions % (history + 1)
    assert len(twin.old_dirs) == history and mirror.n_iter == twin.n_iter == 14
    for (s, y), ts, ty in zip(mirror.pairs, twin.old_stps, twin.old_dirs, strict=True):
        assert torch.equal(s, ts) and torch.equal(y, ty)


@pytest.mark.parametrize(("name", "n", "expected"), lg.CASES, ids=[c[0] for c in lg.CASES])
def test_a_dropped_tail_element_cannot_hide_in_the_tolerance(name, n, expected):
    """For every case and every call of its script: leaving the last element, or the first element of the last tile,
    out of ``g.g`` or of any ``s_j.g`` moves the value by more than 4x the tolerance.  The script itself does what the
    GPU test relies on: every call but the first and the repeat pushes, the ring evicts three times and the history
    length passes through 0..6."""
    geo = lg.threshold_mirror(n)
    pos = lg.tail_positions(n, geo["tile_a"], geo["tile_b"])
    assert n - 1 in pos and (n - 1) // geo["tile_a"] * geo["tile_a"] in pos
    margins = []
    mirror, _, trace = drive(n, lg.CALLS, lg.REPEAT_AT,
                             on_call=lambda m, twin, g, y_c, s_c: margins.append(lg.sensitivity_margin(m.pairs, g, pos)))
    assert min(margins) > 1.0, f"{name}: a dropped element moves a product by only {4 * min(margins):.2f}x its tolerance"
    assert [p for _, p in trace] == [c not in (1, lg.REPEAT_AT) for c in range(1, lg.CALLS + 1)]
    assert mirror.evictions >= 3 and {h for h, _ in trace} == set(range(lg.HISTORY + 1))


def test_case_list_names_the_class_each_size_reaches():
    classes = set()
    for name, n, expected in lg.CASES:
        mirror = lg.threshold_mirror(n)
        assert lg.geometry_class(mirror) == expected, f"{name}: thresholds give {lg.geometry_class(mirror)}"
        assert name == f"n{n}_{expected[0]}x{expected[1]}_{expected[2]}"
        geo = ops.lbfgs_geometry(n, lg.HISTORY)               # host arithmetic: runs without a GPU
        assert geo == mirror, f"{name}: library {geo} vs thresholds {mirror} (overrides: {lg.OVERRIDES}?)"
        classes.add(expected)
    assert len(classes) == 6
    assert lg.threshold_mirror(258048)["ntiles"] == 252 and lg.threshold_mirror(786435)["ntiles"] == 193
    assert lg.threshold_mirror(1048575)["ntiles"] == 256 and lg.threshold_mirror(258049)["nn"] == 262144


def test_geometry_rejects_bad_arguments_and_views_follow_the_layout():
    from style_transfer_visualizer_amd import _lib
    lib = _lib.load()
    assert lib.stv_lbfgsc_geometry(0, 6, None, None, None, None, None) == 1
    assert lib.stv_lbfgsc_geometry(10, 0, None, None, None, None, None) == 1
    assert lib.stv_lbfgsc_geometry(10, 129, None, None, None, None, None) == 1
    assert lib.stv_lbfgsc_geometry(10, 6, None, None, None, None, None) == 0
    n, history = 4099, 6
    nn = 8192
    work = torch.arange(lib.stv_lbfgsc_workspace_bytes(n, history) // 4, dtype=torch.float32)
    v = ops.lbfgs_views(work, n, history)
    assert v["d"].shape == v["prev_g"].shape == (nn,) and v["S"].shape == v["Y"].shape == (history + 1, nn)
    assert float(v["d"][0]) == 0 and float(v["prev_g"][0]) == nn and float(v["S"][2, 1]) == 2 * nn + 2 * nn + 1
    assert float(v["Y"][0, 0]) == (2 + history + 1) * nn
    off = lib.stv_lbfgsc_dots_offset(n, history, None, None)
    assert off // 4 >= (2 + 2 * (history + 1)) * nn                # the rings end in front of the double tables


def test_expected_direction_is_the_exactly_rounded_combination():
    """Against ``math.fsum`` (exact) on a cancelling combination: the compensated sum is within 2**-53 of it, and
    ``A`` is the sum of the absolute terms."""
    gen = torch.Generator().manual_seed(3)
    n, m = 64, 6
    g = torch.randn(n, generator=gen)
    pairs = [(torch.randn(n, generator=gen) * 10.0 ** k, torch.randn(n, generator=gen) * 10.0 ** -k) for k in range(m)]
    cs = [float(torch.randn((), generator=gen)) for _ in range(m)]
    cy = [float(torch.randn((), generator=gen).float()) * 1e3 for _ in range(m)]
    cg = -0.37109375
    want, A = lg.expected_direction(g, pairs, cg, cs, cy)
    for k in range(n):
        terms = [cg * float(g[k])] + [c * float(s[k]) for (s, _), c in zip(pairs, cs, strict=True)] + \
                [c * float(y[k]) for (_, y), c in zip(pairs, cy, strict=True)]
        exact = math.fsum(terms)
        assert abs(float(want[k]) - exact) <= 2.0 ** -52 * abs(exact) + 1e-300
        assert abs(float(A[k]) - math.fsum(abs(t) for t in terms)) <= 1e-12 * float(A[k])
    tol = lg.direction_tolerance(want, A, m)
    assert bool((tol >= 2.0 ** -24 * want.abs()).all())


def test_ulp32_is_the_fp32_spacing():
    v = torch.tensor([1.0, 1.5, 2.0, 0.75, -3.0, 1e-45, 0.0, 16777216.0], dtype=torch.float64)
    f = v.float()
    up = torch.nextafter(f.abs(), torch.tensor(float("inf"))).double() - f.abs().double()
    got = lg.ulp32(v)
    assert torch.equal(got[:5], up[:5]) and float(got[7]) == 2.0
    assert float(got[5]) == 2.0 ** -149 and float(got[6]) == 2.0 ** -149
