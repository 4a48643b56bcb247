"""Device L-BFGS with several iterations per optimizer step (``stv_lbfgsc_iter``, ``HipLBFGS(max_iter > 1)``).

torch.optim.LBFGS with ``max_iter > 1`` (no line search; ``oracle/optim_ref.LbfgsRef`` is the statement) loops
"iteration, evaluation" inside one ``step`` and leaves the loop through one of seven exits.  The device runs the
same loop as one call per evaluation with the position inside the step and a live/dead flag in its state block
(csrc/lbfgs_compact.hip ``solve_body<true>``); the host never reads anything back.

Kernel versus twins (the pattern of tests/test_gpu_lbfgs_long.py): the device and an fp32 and a float64
``TracedLbfgs`` twin (tests/lbfgs_multi_util.py, bit-identical to ``LbfgsRef``: tests/test_lbfgs_multi_host.py) are
fed THE SAME loss and gradient sequence, evaluated at the DEVICE's iterate.  After every evaluation the device's
integer state, push flag and live/dead flag must equal what the fp32 twin did behind that evaluation; every update
must be as close to the float64 twin's as that file demands (at most 4x the fp32 twin's own deviation over this and
the few preceding updates, floor 2e-6 of the update).  Each case asserts that the exit it is about was taken in the
twin, with more than 64 pairs stored where the case can have them.

Bitwise: one iteration per step through the new entry equals ``stv_lbfgsc_step`` (image and every byte of the
history); ``max_iter=4, max_eval=5`` x N equals ``max_iter=1`` x 4N; ``max_iter=5, max_eval=4`` x N (3 iterations and
a 4th evaluation that no update follows) equals ``max_iter=1`` x 3N; a step abandoned by a raising closure leaves the
next step starting at position 1.
"""
from __future__ import annotations

import ctypes
import math

import pytest
import torch

from style_transfer_visualizer_amd import _lib, ops
from style_transfer_visualizer_amd.optimizers import HipLBFGS, lbfgs_schedule
from tests.lbfgs_multi_util import TracedLbfgs, objective

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
N = 20000


class _Device:
    """One ``stv_lbfgsc_iter`` state machine over ``n`` elements."""

    def __init__(self, n: int, history: int, iters: int, lr: float) -> None:
        self.history, self.iters, self.lr = history, iters, lr
        self.x = torch.zeros(n, device=DEV)
        self.state, self.work = ops.lbfgs_alloc(n, history, DEV, compact=True)
        self.calls = 0

    def call(self, loss: torch.Tensor, g: torch.Tensor) -> None:
        ops.lbfgs_iter(self.x, g.to(DEV), loss.reshape(1).to(DEV), self.state, self.work, self.history,
                       min(self.calls, self.history), self.iters, self.lr)
        self.calls += 1

    def image(self) -> torch.Tensor:
        return self.x.cpu()

    def ints(self) -> dict:
        raw = self.state.cpu().view(torch.int32)
        return {"n_iter": int(raw[0]), "hist_len": int(raw[1]), "skip": int(raw[3]), "no_update": int(raw[4]),
                "pushed": int(raw[5]), "step_pos": abs(int(raw[7])), "step_dead": int(raw[7]) < 0}


def run_case(case: str, *, max_iter: int, max_eval: int, steps: int, cond: float = 1e4, lr: float = 1.0,
             events: dict | None = None, history: int = 100, n: int = N, make_device=_Device) -> dict:
    """Drive device + twins through ``steps`` optimizer steps.  ``events``: ``(step, evaluation) -> name`` replaces
    that evaluation's gradient (``tiny`` 5e-8, ``flat`` 2e-7 sign(g), ``small`` 1e-3 sign(g), ``repeat`` the
    previous gradient).  Returns the fp32 twin's exits and, per exit, the largest history length it was taken at."""
    events = events or {}
    f = objective(n, cond)
    iters, evals = lbfgs_schedule(max_iter, max_eval)
    dev = make_device(n, history, iters, lr)
    x32, x64 = torch.zeros(n), torch.zeros(n, dtype=torch.float64)
    kw = dict(lr=lr, max_iter=max_iter, max_eval=max_eval, history_size=history)
    twin32, twin64 = TracedLbfgs(x32, **kw), TracedLbfgs(x64, **kw)
    prev_g = [None]
    e32_hist: list[float] = []
    worst_dev = worst_32 = 0.0
    hist_at_exit: dict[str, int] = {}
    pushes_skipped = 0

    def evaluate(x_dev: torch.Tensor, step: int, k: int):
        loss, g = f(x_dev)
        ev = events.get((step, k))
        if ev == "tiny":
            g = torch.full((n,), 5e-8)
        elif ev == "flat":
            g = 2e-7 * torch.sign(g)
        elif ev == "small":
            g = 1e-3 * torch.sign(g)
        elif ev == "repeat":
            g = prev_g[0].clone()
        prev_g[0] = g
        return loss, g

    for step in range(1, steps + 1):
        seq: list[tuple[torch.Tensor, torch.Tensor]] = []
        snaps: list[tuple[dict, torch.Tensor, torch.Tensor]] = []     # (ints, image before, image after) per device call

        def evaluate_and_call(step=step, seq=seq, snaps=snaps):
            k = len(seq) + 1
            before = dev.image()
            loss, g = evaluate(before, step, k)
            seq.append((loss, g))
            if k <= iters:
                dev.call(loss, g)
                snaps.append((dev.ints(), before, dev.image()))
            return loss, g

        def closure32():
            loss, g = evaluate_and_call()
            return loss, g.clone()
        log0 = len(twin32.log)
        twin32.step(closure32)
        made = len(seq)                                        # evaluations the reference made in this step
        replay = iter(seq[:made])

        def closure64():
            loss, g = next(replay)
            return loss, g.double()
        log0_64 = len(twin64.log)
        twin64.step(closure64)
        assert next(replay, None) is None and twin64.exits[-1] == twin32.exits[-1], \
            f"{case} step {step}: float64 twin left by {twin64.exits[-1]}, fp32 twin by {twin32.exits[-1]}"
        while len(seq) < evals:                                # the dead remainder: evaluations of an unchanged image
            evaluate_and_call()
        assert len(snaps) == iters
        exit_ = twin32.exits[-1]
        hist_at_exit[exit_] = max(hist_at_exit.get(exit_, -1), len(twin32.old_dirs))
        entries, entries64 = twin32.log[log0:], twin64.log[log0_64:]
        assert len(entries) == made == len(entries64)
        dead = False
        for k in range(1, iters + 1):
            st, before, after = snaps[k - 1]
            entry = entries[k - 1] if k <= made else None
            where = f"{case} step {step} evaluation {k}"
            if entry is None or entry["kind"] == "stop":       # a stop test fired here, or the step was over already
                dead = True
                assert st["skip"] == 1 and st["no_update"] == 0 and st["pushed"] == 0, f"{where}: {st}"
                assert torch.equal(before, after), f"{where}: a dead call moved the image"
            else:
                assert entry["kind"] == "iter"
                assert st["skip"] == 0 and st["no_update"] == int(entry["no_update"]), f"{where}: {st} vs {entry}"
                assert st["pushed"] == int(entry["pushed"]), f"{where}: push {st['pushed']} vs {entry['pushed']}"
                pushes_skipped += int(not entry["pushed"] and entry["n_iter"] > 1)
                dead = dead or entry["no_update"]
                u_dev = after.double() - before.double()
                if entry["no_update"]:
                    assert float(u_dev.abs().max()) == 0.0, f"{where}: the image must not move"
                else:
                    u_32, u_64 = entry["update"].double(), entries64[k - 1]["update"]
                    scale = float(u_64.abs().max())
                    assert scale > 0.0
                    e_dev = float((u_dev - u_64).abs().max()) / scale
                    e_32 = float((u_32 - u_64).abs().max()) / scale
                    e32_hist.append(e_32)
                    ref = max(e32_hist[-8:])
                    worst_dev, worst_32 = max(worst_dev, e_dev), max(worst_32, e_32)
                    assert e_dev <= max(4.0 * ref, 2e-6), \
                        (f"{where} (history {entry['hist_len']}): device update is {e_dev:.2e} from the float64 update, "
                         f"the fp32 reference {e_32:.2e} (window max {ref:.2e})")
            n_iter_ref = twin32.n_iter if entry is None else next(
                (e["n_iter"] for e in reversed(twin32.log[:log0 + k]) if e["kind"] == "iter"), 0)
            hist_ref = len(twin32.old_dirs) if entry is None else next(
                (e["hist_len"] for e in reversed(twin32.log[:log0 + k]) if e["kind"] == "iter"), 0)
            assert st["n_iter"] == n_iter_ref and st["hist_len"] == hist_ref, f"{where}: {st} vs {n_iter_ref}/{hist_ref}"
            assert st["step_pos"] == (k if k < iters else 0), f"{where}: position {st['step_pos']}"
            if k < iters:
                assert st["step_dead"] == bool(dead), f"{where}: dead flag {st['step_dead']} vs {dead}"
        assert torch.isfinite(dev.image()).all()
    assert dev.ints()["n_iter"] == twin32.n_iter == twin64.n_iter
    x_end = dev.image().double()
    dx = float((x_end - x64).abs().max() / x64.abs().max())
    dx32 = float((x32.double() - x64).abs().max() / x64.abs().max())
    print(f"{case}: worst update deviation {worst_dev:.2e} (fp32 reference {worst_32:.2e}); final x vs float64 {dx:.1e} "
          f"(reference {dx32:.1e}); exits {sorted(set(twin32.exits))}; history at exit {hist_at_exit}")
    assert dx <= max(4.0 * dx32, 2e-6)
    return {"exits": twin32.exits, "hist_at_exit": hist_at_exit, "pushes_skipped": pushes_skipped,
            "hist_len": len(twin32.old_dirs)}


def test_no_exit_every_step_leaves_by_max_iter():
    r = run_case("multi (4,5) no exit", max_iter=4, max_eval=5, steps=30)
    assert r["exits"] == ["max_iter"] * 30 and r["hist_len"] == 100          # 120 iterations: the ring is full


def test_max_eval_exit_every_step():
    """max_iter=8, max_eval=6: 5 iterations and 6 evaluations per step; no update follows the 6th."""
    r = run_case("multi (8,6) max_eval", max_iter=8, max_eval=6, steps=15)
    assert r["exits"] == ["max_eval"] * 15 and r["hist_at_exit"]["max_eval"] > 64


def test_loss_change_exit():
    """cond 1e2, max_iter=20, max_eval=25: once converged to fp32 resolution the loss stops changing (from step 3
    on; 28 steps so that the exit is also taken with more than 64 pairs stored)."""
    r = run_case("multi (20,25) loss change", max_iter=20, max_eval=25, steps=28, cond=1e2)
    assert r["exits"][:12].count("loss_change") >= 8 and r["hist_at_exit"]["loss_change"] > 64


def test_step_size_exit():
    """lr = 1e-5 and one 1e-3 sign(g) gradient mid-step: the update that follows has max|d*t| ~ 1e-11 <= 1e-9."""
    r = run_case("multi (4,5) step size", max_iter=4, max_eval=5, steps=21, lr=1e-5, events={(20, 2): "small"})
    assert r["exits"][19] == "step_size" and r["hist_at_exit"]["step_size"] > 64


def test_step_size_exit_in_the_first_step():
    """lr = 1e-6: the very first update (t = lr / |g|_1) is below the tolerance."""
    r = run_case("multi (4,5) lr 1e-6", max_iter=4, max_eval=5, steps=2, lr=1e-6)
    assert r["exits"] == ["step_size", "max_iter"]


def test_scripted_gradient_exits_with_a_long_history():
    """A 5e-8 gradient mid-step (gradient test inside the loop) and at a first evaluation (early return), a
    2e-7 sign(g) gradient mid-step (g.d > -1e-9: state saved, image not moved) and a repeated gradient (no push),
    all behind 76+ iterations."""
    events = {(20, 2): "tiny", (21, 1): "tiny", (22, 2): "flat", (23, 2): "repeat"}
    r = run_case("multi (4,5) scripted", max_iter=4, max_eval=5, steps=25, events=events)
    assert (r["exits"][19], r["exits"][20], r["exits"][21]) == ("grad", "early_return", "gtd")
    assert r["exits"][22] == "max_iter" and r["pushes_skipped"] >= 1
    assert all(r["hist_at_exit"][e] > 64 for e in ("grad", "early_return", "gtd"))


# ---------------------------------------------------------------------------------------------- bitwise
def test_one_iteration_per_step_is_bit_identical_to_lbfgsc_step():
    """``stv_lbfgsc_iter(iters_per_step=1)`` versus ``stv_lbfgsc_step``: 30 steps over a ring of 16 pairs (14
    evictions): same image, same history vectors and product tables, byte for byte."""
    n, history = N, 16
    f = objective(n)
    xa, xb = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    sa, wa = ops.lbfgs_alloc(n, history, DEV, compact=True)
    sb, wb = ops.lbfgs_alloc(n, history, DEV, compact=True)
    off = int(_lib.load().stv_lbfgsc_dots_offset(n, history, ctypes.byref(ctypes.c_int()), ctypes.byref(ctypes.c_int())))
    for step in range(30):
        loss, g = f(xa)
        g = g.to(DEV)
        m_max = min(step, history)
        ops.lbfgs_step(xa, g, sa, wa, history, m_max, 1.0, compact=True)
        ops.lbfgs_iter(xb, g, loss.reshape(1).to(DEV), sb, wb, history, m_max, 1, 1.0)
        assert torch.equal(xa, xb), f"step {step + 1}"
    # d, prev_g, S, Y, the S.Y and Y.Y tables - as raw words: half of a double, read as fp32, can be a NaN pattern
    assert torch.equal(wa[: off // 4].view(torch.int32), wb[: off // 4].view(torch.int32))
    ia, ib = sa.cpu().view(torch.int32), sb.cpu().view(torch.int32)
    assert torch.equal(ia[:7], ib[:7]) and int(ib[7]) == 0 and torch.equal(ia[8:15], ib[8:15])
    assert torch.equal(ia[16:], ib[16:])                                 # ro, direction coefficients


def _gpu_closure(p: torch.Tensor, n: int, fail_on: set | None = None):
    """Closure for ``HipLBFGS``: the quartic on the GPU (float64 elementwise, so deterministic), gradient into
    ``p.grad``; raises on the evaluation numbers in ``fail_on``."""
    gen = torch.Generator().manual_seed(5)
    a = torch.exp(torch.rand(n, generator=gen, dtype=torch.float64) * math.log(1e4)).to(DEV)
    b = torch.randn(n, generator=gen, dtype=torch.float64).to(DEV)
    count = [0]

    def closure():
        count[0] += 1
        if fail_on and count[0] in fail_on:
            msg = "scripted failure"
            raise RuntimeError(msg)
        x = p.detach().double()
        g = a * x - b + 0.2 * x ** 3
        g[1:] += 0.1 * x[:-1]
        g[:-1] += 0.1 * x[1:]
        p.grad = g.float()
        return ((0.5 * a * x * x - b * x + 0.05 * x ** 4).sum() + 0.1 * (x[1:] * x[:-1]).sum()).float()
    return closure, count


def _run_hip(max_iter: int, max_eval: int, steps: int, fail_on: set | None = None) -> tuple[torch.Tensor, HipLBFGS, int]:
    p = torch.zeros(N, device=DEV, requires_grad=True)
    opt = HipLBFGS([p], lr=1.0, max_iter=max_iter, max_eval=max_eval)
    closure, count = _gpu_closure(p, N, fail_on)
    for _ in range(steps):
        try:
            opt.step(closure)
        except RuntimeError as exc:
            if "scripted" not in str(exc):
                raise
    return p.detach().clone(), opt, count[0]


@pytest.fixture(scope="module")
def single_steps():
    """``HipLBFGS(max_iter=1)`` images after 13, 24 and 32 steps (one run, shared)."""
    p = torch.zeros(N, device=DEV, requires_grad=True)
    opt = HipLBFGS([p], lr=1.0)
    closure, _ = _gpu_closure(p, N)
    out = {}
    for step in range(1, 33):
        opt.step(closure)
        if step in (13, 24, 32):
            out[step] = p.detach().clone()
    return out


def test_four_iterations_per_step_equal_four_single_steps(single_steps):
    x, opt, calls = _run_hip(4, 5, 8)
    assert (opt.iters_per_step, opt.evals_per_step, calls) == (4, 4, 32)
    assert torch.equal(x, single_steps[32])
    st = opt.device_state()
    assert st["n_iter"] == 32 and st["step_pos"] == 0


def test_max_eval_below_max_iter_equals_three_single_steps(single_steps):
    """max_iter=5, max_eval=4: 3 iterations + 4 evaluations per step; the 4th evaluation is followed by no update."""
    x, opt, calls = _run_hip(5, 4, 8)
    assert (opt.iters_per_step, opt.evals_per_step, calls) == (3, 4, 32)
    assert torch.equal(x, single_steps[24])
    assert opt.device_state()["n_iter"] == 24


def test_abandoned_step_restarts_at_position_one(single_steps):
    """Steps 1-2 complete (8 evaluations), step 3's closure raises on its 2nd call (evaluation 10: one iteration of
    that step is applied and stays applied), step 4 is a normal step: 4 + 4 + 1 + 4 = 13 iterations, the image of 13
    single steps - without the reset step 4 would start at position 2, run 3 iterations and test a stale loss."""
    x, opt, _ = _run_hip(4, 5, 4, fail_on={10})
    st = opt.device_state()
    assert st["n_iter"] == 13 and st["step_pos"] == 0 and not st["step_dead"]
    assert torch.equal(x, single_steps[13])
    # the traced twin, fed one gradient per iteration the device ran, agrees on the integer state
    twin = TracedLbfgs(torch.zeros(N), max_iter=1, max_eval=1)
    f = objective(N)
    for _ in range(13):
        twin.step(lambda: f(twin.x))
    assert (twin.n_iter, len(twin.old_dirs)) == (st["n_iter"], st["hist_len"])


def test_limits_are_named():
    p = torch.zeros(64, device=DEV, requires_grad=True)
    with pytest.raises(ValueError, match="max_iter"):
        HipLBFGS([p], max_iter=4, shard_group=True)
