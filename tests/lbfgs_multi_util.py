"""Helpers for the ``max_iter > 1`` L-BFGS tests (host and GPU).

``TracedLbfgs`` restates ``oracle.optim_ref.LbfgsRef.step`` (torch 2.10 ``LBFGS.step``, no line search) line by line
and additionally records, for every closure evaluation, what happened behind it and which exit ended the step - the
oracle itself only exposes the end state.  tests/test_lbfgs_multi_host.py checks it bit-identical to ``LbfgsRef``.
One deliberate difference, on a path the oracle does not define: when the closure RAISES mid-step, the iterations
completed so far stay committed (``d`` and ``t`` are saved), which is what a device-resident optimizer does - torch
and ``LbfgsRef`` keep the previous step's ``d`` beside an already moved image.

``IterProtocol`` is the call-per-evaluation form the device implements (``stv_lbfgsc_iter``): position inside the
step and a live/dead flag are state, the stop tests run before any state change, a dead call is a no-op.  It is
checked against ``LbfgsRef`` on the host and lets the GPU test's driver be exercised without a GPU.
"""
from __future__ import annotations

import math
from collections.abc import Callable

import torch

# how a step ended
EXITS = ("early_return", "gtd", "max_iter", "max_eval", "grad", "step_size", "loss_change")


def schedule(max_iter: int, max_eval: int) -> tuple[int, int]:
    """(iterations, evaluations) per step when no data-dependent exit fires, derived here from the loop itself:
    evaluation 1 opens the step, every iteration except the ``max_iter``-th is followed by one evaluation, and the
    loop leaves behind the evaluation that brings the count to ``max_eval``."""
    evals, iters = 1, 0
    while iters < max_iter:
        iters += 1
        if iters == max_iter:
            break
        evals += 1
        if evals >= max_eval:
            break
    return iters, evals


def objective(n: int, cond: float = 1e4, quart: float = 0.05, seed: int = 5):
    """``x -> (loss, grad)`` of  sum 0.5 a x^2 - b x + quart x^4 + 0.1 x_i x_{i+1}  with a spectrum 1..cond (the
    quartic of tests/test_gpu_lbfgs_long.py), evaluated in float64 and rounded to fp32."""
    gen = torch.Generator().manual_seed(seed)
    a = torch.exp(torch.rand(n, generator=gen, dtype=torch.float64) * math.log(cond))
    b = torch.randn(n, generator=gen, dtype=torch.float64)

    def loss_and_grad(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        x = x.double().cpu()
        g = a * x - b + 4.0 * quart * x ** 3
        g[1:] += 0.1 * x[:-1]
        g[:-1] += 0.1 * x[1:]
        loss = (0.5 * a * x * x - b * x + quart * x ** 4).sum() + 0.1 * (x[1:] * x[:-1]).sum()
        return loss.float(), g.float()
    return loss_and_grad


class TracedLbfgs:
    """``LbfgsRef.step`` with a trace.  ``self.log`` gets one dict per closure evaluation:
    ``kind`` = ``iter`` (an iteration ran behind it), ``stop`` (a stop test fired on it, or the early return),
    ``last_eval`` (the evaluation that reached ``max_eval``); for ``iter`` also ``pushed``, ``no_update``, ``n_iter``,
    ``hist_len`` and ``update`` (what was added to x).  ``self.exits`` gets one name of ``EXITS`` per step."""

    def __init__(self, x: torch.Tensor, lr: float = 1.0, max_iter: int = 1, max_eval: int | None = None,
                 tolerance_grad: float = 1e-7, tolerance_change: float = 1e-9, history_size: int = 100) -> None:
        self.x, self.lr, self.max_iter = x, lr, max_iter
        self.max_eval = max_eval if max_eval is not None else max_iter * 5 // 4
        self.tolerance_grad, self.tolerance_change, self.history_size = tolerance_grad, tolerance_change, history_size
        self.n_iter = self.func_evals = 0
        self.d = self.t = None
        self.old_dirs: list[torch.Tensor] = []
        self.old_stps: list[torch.Tensor] = []
        self.ro: list[torch.Tensor] = []
        self.H_diag = 1
        self.prev_flat_grad = None
        self.prev_loss = None
        self.al: list = [None] * history_size
        self.log: list[dict] = []
        self.exits: list[str] = []

    @torch.no_grad()
    def step(self, closure: Callable[[], tuple[torch.Tensor, torch.Tensor]]) -> torch.Tensor:
        orig_loss, grad = closure()
        loss = float(orig_loss)
        current_evals = 1
        self.func_evals += 1
        flat_grad = grad.reshape(-1)
        if flat_grad.abs().max() <= self.tolerance_grad:
            self.log.append({"kind": "stop"})
            self.exits.append("early_return")
            return orig_loss
        d, t = self.d, self.t
        n_iter = 0
        exit_ = "max_iter"
        try:
            while n_iter < self.max_iter:
                n_iter += 1
                self.n_iter += 1
                pushed = False
                if self.n_iter == 1:
                    d = flat_grad.neg()
                    self.old_dirs, self.old_stps, self.ro = [], [], []
                    self.H_diag = 1
                else:
                    y = flat_grad.sub(self.prev_flat_grad)
                    s = d.mul(t)
                    ys = y.dot(s)
                    if ys > 1e-10:
                        if len(self.old_dirs) == self.history_size:
                            self.old_dirs.pop(0)
                            self.old_stps.pop(0)
                            self.ro.pop(0)
                        self.old_dirs.append(y)
                        self.old_stps.append(s)
                        self.ro.append(1.0 / ys)
                        self.H_diag = ys / y.dot(y)
                        pushed = True
                    num_old = len(self.old_dirs)
                    al = self.al
                    q = flat_grad.neg()
                    for i in range(num_old - 1, -1, -1):
                        al[i] = self.old_stps[i].dot(q) * self.ro[i]
                        q.add_(self.old_dirs[i], alpha=-al[i])
                    d = r = torch.mul(q, self.H_diag)
                    for i in range(num_old):
                        be_i = self.old_dirs[i].dot(r) * self.ro[i]
                        r.add_(self.old_stps[i], alpha=al[i] - be_i)
                if self.prev_flat_grad is None:
                    self.prev_flat_grad = flat_grad.clone()
                else:
                    self.prev_flat_grad.copy_(flat_grad)
                self.prev_loss = loss
                if self.n_iter == 1:
                    t = min(1.0, 1.0 / flat_grad.abs().sum()) * self.lr
                else:
                    t = self.lr
                entry = {"kind": "iter", "pushed": pushed, "no_update": False, "n_iter": self.n_iter,
                         "hist_len": len(self.old_dirs), "update": None}
                self.log.append(entry)
                gtd = flat_grad.dot(d)
                if gtd > -self.tolerance_change:
                    entry["no_update"] = True
                    exit_ = "gtd"
                    break
                before = self.x.clone()
                self.x.view(-1).add_(d, alpha=t)
                entry["update"] = self.x - before
                ls_func_evals = 0
                if n_iter != self.max_iter:
                    new_loss, grad = closure()
                    loss = float(new_loss)
                    flat_grad = grad.reshape(-1)
                    ls_func_evals = 1
                current_evals += ls_func_evals
                self.func_evals += ls_func_evals
                if n_iter == self.max_iter:
                    break
                if current_evals >= self.max_eval:
                    self.log.append({"kind": "last_eval"})
                    exit_ = "max_eval"
                    break
                if flat_grad.abs().max() <= self.tolerance_grad:
                    exit_ = "grad"
                elif d.mul(t).abs().max() <= self.tolerance_change:
                    exit_ = "step_size"
                elif abs(loss - self.prev_loss) < self.tolerance_change:
                    exit_ = "loss_change"
                if exit_ != "max_iter":
                    self.log.append({"kind": "stop"})
                    break
        finally:
            self.d, self.t = d, t                # (also when the closure raised: see the module docstring)
        self.exits.append(exit_)
        return orig_loss


class IterProtocol:
    """The device's protocol on the host: ``call(loss, grad)`` once behind each of the first ``iters`` evaluations
    of a step; ``pos`` / ``dead`` are state.  Vector arithmetic as ``LbfgsRef`` (torch CPU ops in x's dtype)."""

    def __init__(self, x: torch.Tensor, iters: int, lr: float = 1.0, tolerance_grad: float = 1e-7,
                 tolerance_change: float = 1e-9, history_size: int = 100) -> None:
        self.x, self.iters, self.lr = x, iters, lr
        self.tolerance_grad, self.tolerance_change, self.history_size = tolerance_grad, tolerance_change, history_size
        self.n_iter = 0
        self.pos, self.dead = 0, False
        self.d = self.t = self.prev_g = self.prev_loss = None
        self.S: list[torch.Tensor] = []
        self.Y: list[torch.Tensor] = []
        self.ro: list = []
        self.H_diag = 1
        self.skip = self.no_update = self.pushed = 0

    def reset(self) -> None:
        self.pos, self.dead = 0, False

    @torch.no_grad()
    def call(self, loss: torch.Tensor, grad: torch.Tensor) -> None:
        g = grad.reshape(-1)
        pos = self.pos + 1
        stop = bool(g.abs().max() <= self.tolerance_grad)
        if pos > 1 and not stop:
            stop = bool(self.d.mul(self.t).abs().max() <= self.tolerance_change) or \
                abs(float(loss) - self.prev_loss) < self.tolerance_change
        if self.dead:
            stop = True
        self.skip, self.no_update, self.pushed = int(stop), 0, 0
        if not stop:
            self.n_iter += 1
            if self.n_iter == 1:
                d = g.neg()
                self.S, self.Y, self.ro, self.H_diag = [], [], [], 1
            else:
                y = g.sub(self.prev_g)
                s = self.d.mul(self.t)
                ys = y.dot(s)
                if ys > 1e-10:
                    if len(self.S) == self.history_size:
                        self.S.pop(0), self.Y.pop(0), self.ro.pop(0)
                    self.Y.append(y), self.S.append(s), self.ro.append(1.0 / ys)
                    self.H_diag = ys / y.dot(y)
                    self.pushed = 1
                m = len(self.S)
                al = [None] * m
                q = g.neg()
                for i in range(m - 1, -1, -1):
                    al[i] = self.S[i].dot(q) * self.ro[i]
                    q.add_(self.Y[i], alpha=-al[i])
                d = r = torch.mul(q, self.H_diag)
                for i in range(m):
                    be_i = self.Y[i].dot(r) * self.ro[i]
                    r.add_(self.S[i], alpha=al[i] - be_i)
            self.prev_g = g.clone()
            self.prev_loss = float(loss)
            self.t = (min(1.0, 1.0 / g.abs().sum()) * self.lr) if self.n_iter == 1 else self.lr
            self.d = d
            if g.dot(d) > -self.tolerance_change:
                self.no_update = 1
            else:
                self.x.view(-1).add_(d, alpha=self.t)
        self.dead = self.dead or stop or bool(self.no_update)
        self.pos = pos
        if pos >= self.iters:
            self.reset()

    def ints(self) -> dict:
        return {"n_iter": self.n_iter, "hist_len": len(self.S), "skip": self.skip, "no_update": self.no_update,
                "pushed": self.pushed, "step_pos": self.pos, "step_dead": self.dead}


def run_protocol_step(opt, evals: int, iters: int, closure) -> None:
    """One optimizer step in the call-per-evaluation form: ``evals`` closure calls, ``opt.call`` behind the first
    ``iters`` of them (what ``HipLBFGS.step`` does for ``max_iter > 1``)."""
    for k in range(evals):
        loss, g = closure()
        if k < iters:
            opt.call(loss, g)
