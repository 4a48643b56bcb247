"""``lbfgs_max_iter > 1`` on the host: the C ABI of the per-iteration entry, the host-known (iterations,
evaluations) schedule, and the restatements the GPU tests compare the device with.

No GPU: ``oracle.optim_ref.LbfgsRef`` (bit-identical to ``torch.optim.LBFGS`` on CPU, tests/test_oracle_golden.py)
is the statement of the algorithm; everything here is checked bit for bit against it.
"""
from __future__ import annotations

import pytest
import torch

from oracle import optim_ref
from style_transfer_visualizer_amd import _lib, optimizers
from tests.lbfgs_multi_util import EXITS, IterProtocol, TracedLbfgs, objective, run_protocol_step, schedule

GRID = [(20, 1), (5, 3), (5, 4), (4, 5), (1, 1), (1, 5), (2, 3), (8, 6), (20, 25), (3, 3), (2, 2), (7, 100)]
N = 2000


def test_library_exports_the_iteration_entry_and_rejects_null_pointers():
    lib = _lib.load()
    assert lib.stv_version() >= 103
    assert lib.stv_lbfgsc_iter(None, None, None, None, None, 10, 100, 0, 4, 1.0, 1e-7, 1e-9, None) == 1
    assert lib.stv_lbfgsc_iter_reset(None, None) == 1
    assert _lib.OP_LBFGS_ITER == _lib.OP_LBFGS_STEP + 1 == 16      # appended: the existing ops keep their numbers


def _scripted(n: int, cond: float = 1e4):
    """``(step, evaluation) -> gradient transform`` events on top of the quartic: each data-dependent exit once."""
    f = objective(n, cond)
    events = {(6, 2): "tiny", (8, 1): "tiny", (10, 2): "flat", (12, 2): "repeat"}

    def evaluate(x, step, k, prev_g):
        loss, g = f(x)
        ev = events.get((step, k))
        if ev == "tiny":
            g = torch.full((n,), 5e-8)
        elif ev == "flat":
            g = 2e-7 * torch.sign(g)
        elif ev == "repeat":
            g = prev_g.clone()
        return loss, g
    return evaluate


def _drive(opt_step, x, evaluate, steps):
    """Run ``steps`` optimizer steps; the closure evaluates at the optimizer's own iterate.  Returns evaluations/step."""
    counts, prev = [], [None]
    for step in range(1, steps + 1):
        k = [0]

        def closure():
            k[0] += 1
            loss, g = evaluate(x, step, k[0], prev[0])
            prev[0] = g
            return loss, g.clone()
        opt_step(closure)
        counts.append(k[0])
    return counts


@pytest.mark.parametrize(("max_iter", "max_eval"), GRID)
def test_schedule_equals_the_oracles_evaluation_counts(max_iter, max_eval):
    """(I, E) from the two settings alone = what ``LbfgsRef`` does on a sequence where no data-dependent exit fires."""
    iters, evals = optimizers.lbfgs_schedule(max_iter, max_eval)
    assert (iters, evals) == schedule(max_iter, max_eval)
    f = objective(N)
    x = torch.zeros(N)
    ref = optim_ref.LbfgsRef(x, max_iter=max_iter, max_eval=max_eval)
    counts = _drive(ref.step, x, lambda x_, *_: f(x_), 6)
    assert counts == [evals] * 6
    assert ref.n_iter == 6 * iters and ref.func_evals == 6 * evals


@pytest.mark.parametrize(("max_iter", "max_eval"), [(4, 5), (8, 6), (5, 4), (20, 25), (1, 1), (20, 1)])
def test_traced_restatement_is_bit_identical_to_the_oracle(max_iter, max_eval):
    """Same scripted sequence (every exit fires at least once for max_iter >= 4) -> same image, same state."""
    xa, xb = torch.zeros(N), torch.zeros(N)
    ref = optim_ref.LbfgsRef(xa, max_iter=max_iter, max_eval=max_eval)
    tr = TracedLbfgs(xb, max_iter=max_iter, max_eval=max_eval)
    ca = _drive(ref.step, xa, _scripted(N), 14)
    cb = _drive(tr.step, xb, _scripted(N), 14)
    assert ca == cb and torch.equal(xa, xb)
    assert (ref.n_iter, ref.func_evals, len(ref.old_dirs)) == (tr.n_iter, tr.func_evals, len(tr.old_dirs))
    assert torch.equal(ref.d, tr.d) and float(ref.t) == float(tr.t) and ref.prev_loss == tr.prev_loss
    assert all(torch.equal(a, b) for a, b in zip(ref.old_dirs, tr.old_dirs, strict=True))
    assert len(tr.exits) == 14 and set(tr.exits) <= set(EXITS) and len(tr.log) == sum(cb)
    if max_iter >= 4 and max_eval >= 4:
        assert {"early_return", "grad", "gtd"} <= set(tr.exits)
        assert any(e["kind"] == "iter" and not e["pushed"] and e["n_iter"] > 1 for e in tr.log)     # the repeated gradient


def test_loss_change_and_step_size_exits_are_traced():
    x = torch.zeros(N)
    tr = TracedLbfgs(x, max_iter=20, max_eval=25)
    f = objective(N, 1e2)
    _drive(tr.step, x, lambda x_, *_: f(x_), 12)
    assert "loss_change" in tr.exits
    x = torch.zeros(20000)                # (t = lr / |g|_1 in the very first iteration: max|d*t| ~ 1e-14 at this size)
    tr = TracedLbfgs(x, lr=1e-6, max_iter=4, max_eval=5)
    f = objective(20000)
    _drive(tr.step, x, lambda x_, *_: f(x_), 2)
    assert tr.exits == ["step_size", "max_iter"]


@pytest.mark.parametrize(("max_iter", "max_eval", "cond", "lr", "n"),
                         [(4, 5, 1e4, 1.0, N), (8, 6, 1e4, 1.0, N), (5, 4, 1e4, 1.0, N), (20, 25, 1e2, 1.0, N),
                          (4, 5, 1e4, 1e-6, 20000)])
def test_call_per_evaluation_protocol_leaves_the_oracles_image(max_iter, max_eval, cond, lr, n):
    """The form the device implements - E closure calls per step, one state-machine call behind the first I, the rest
    of a step dead after a data-dependent exit - leaves LbfgsRef's image and history bit for bit, with every exit in
    the sequence; it only evaluates more often (E per step where the oracle stops early)."""
    iters, evals = schedule(max_iter, max_eval)
    ev = _scripted(n, cond)
    xa, xb = torch.zeros(n), torch.zeros(n)
    ref = optim_ref.LbfgsRef(xa, lr=lr, max_iter=max_iter, max_eval=max_eval)
    pro = IterProtocol(xb, iters, lr=lr)
    steps = 14 if n == N else 4
    ca = _drive(ref.step, xa, ev, steps)
    cb = _drive(lambda closure: run_protocol_step(pro, evals, iters, closure), xb, ev, steps)     # (a dead call ignores its gradient)
    assert pro.pos == 0
    assert cb == [evals] * steps and all(a <= evals for a in ca)
    assert torch.equal(xa, xb)
    assert pro.n_iter == ref.n_iter and len(pro.S) == len(ref.old_dirs)
    assert all(torch.equal(a, b) for a, b in zip(ref.old_stps, pro.S, strict=True))


def test_multi_iteration_steps_equal_single_iteration_steps():
    """The two facts the GPU bitwise tests rest on: (4,5) x N = (1,1) x 4N, and (5,4) x N = (1,1) x 3N."""
    f = objective(N)
    for (mi, me), per in (((4, 5), 4), ((5, 4), 3)):
        xa, xb = torch.zeros(N), torch.zeros(N)
        a = optim_ref.LbfgsRef(xa, max_iter=mi, max_eval=me)
        b = optim_ref.LbfgsRef(xb, max_iter=1, max_eval=1)
        _drive(a.step, xa, lambda x_, *_: f(x_), 8)
        _drive(b.step, xb, lambda x_, *_: f(x_), 8 * per)
        assert torch.equal(xa, xb)
