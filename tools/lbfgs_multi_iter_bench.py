"""What ``lbfgs_max_iter = 20`` costs per L-BFGS iteration, on the device path and on the torch fallback.

    python tools/lbfgs_multi_iter_bench.py [--sizes 512 1024] [--iters 60] [--rounds 3] [--out profiles/lbfgs_multi_iter_bench.json]

Synthetic VGG19 weights and images, bf16, history full (100 untimed iterations per leg first).  One process, three legs
alternating ``--rounds`` times (order rotated per round, so clock drift falls on all of them):

* ``max_iter1``  - ``HipLBFGS(max_iter=1)``: one iteration per step, the update inside the closure's hipGraph;
* ``device20``   - ``HipLBFGS(max_iter=20, max_eval=25)``: the same graph replayed 20 times per step
  (``stv_lbfgsc_iter``), exits decided on the device;
* ``torch20``    - ``torch.optim.LBFGS(max_iter=20, max_eval=25)`` on the same closure (what ``STV_LBFGS_MULTI=0``
  selects): its vector passes as torch kernels, its scalar tests as blocking reads.

Each leg has its own image and optimizer.  A timed run is wall time from a synchronised start to a synchronised end
(the torch leg synchronises by itself, so device events would not describe it) over ``--iters`` iterations' worth of
steps; iterations are counted from the optimizer's own ``n_iter``.  One JSON line; with ``--out`` also written there.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from style_transfer_visualizer_amd import core_model, synthetic  # noqa: E402
from style_transfer_visualizer_amd.optimizers import HipLBFGS, single_evaluation  # noqa: E402

S, C = [0, 5, 10, 19, 28], [21]
MAX_ITER, MAX_EVAL = 20, 25


def n_iter(opt) -> int:
    if isinstance(opt, HipLBFGS):
        return int(opt.device_state()["n_iter"])
    return int(opt.state[opt._params[0]].get("n_iter", 0))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--iters", type=int, default=60, help="iterations per timed run (a multiple of 20)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    weights = synthetic.synthetic_conv_weights(3)
    saved = core_model.initialize_vgg
    core_model.initialize_vgg = lambda: core_model.build_vgg_features(weights).eval()
    out = {"tool": "tools/lbfgs_multi_iter_bench.py", "device": torch.cuda.get_device_name(dev), "precision": "bf16",
           "history": 100, "max_iter": MAX_ITER, "max_eval": MAX_EVAL, "iters_per_run": args.iters, "results": {}}
    legs = ("max_iter1", "device20", "torch20")
    try:
        for size in args.sizes:
            content = synthetic.synthetic_image(0, size, size).to(dev)
            style = synthetic.synthetic_image(1, size, size).to(dev)
            model = core_model.StyleContentModel(S, C, precision="bf16").to(dev)
            model.set_targets(style, content)
            opts, closures, steps = {}, {}, {}
            side = torch.cuda.Stream(device=dev)          # a capturable stream, as the runner uses
            with torch.cuda.stream(side):
                for leg in legs:
                    xi = torch.randn(1, 3, size, size, generator=torch.Generator().manual_seed(0)).to(dev).requires_grad_(True)
                    if leg == "max_iter1":
                        opts[leg], steps[leg] = HipLBFGS([xi], lr=1.0), args.iters
                    elif leg == "device20":
                        opts[leg], steps[leg] = HipLBFGS([xi], lr=1.0, max_iter=MAX_ITER, max_eval=MAX_EVAL), args.iters // MAX_ITER
                    else:
                        opts[leg] = torch.optim.LBFGS([xi], lr=1.0, max_iter=MAX_ITER, max_eval=MAX_EVAL)
                        steps[leg] = args.iters // MAX_ITER
                    closures[leg] = single_evaluation(lambda xi=xi: model.loss_and_grad(xi, 1e5, 1.0, live_scores=True)[2])
                    for _ in range(100 if leg == "max_iter1" else 100 // MAX_ITER):      # fill the history, untimed
                        opts[leg].step(closures[leg])
                torch.cuda.synchronize()
                runs = {leg: [] for leg in legs}
                for r in range(args.rounds):
                    k = r % len(legs)
                    for leg in legs[k:] + legs[:k]:
                        opt = opts[leg]
                        before = n_iter(opt)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(steps[leg]):
                            opt.step(closures[leg])
                        torch.cuda.synchronize()
                        dt = time.perf_counter() - t0
                        done = n_iter(opt) - before
                        runs[leg].append({"iterations": done, "seconds": round(dt, 5),
                                          "ms_per_iteration": round(1e3 * dt / max(done, 1), 4)})
            res = {}
            for leg in legs:
                ms = [r["ms_per_iteration"] for r in runs[leg]]
                res[leg] = {"runs": runs[leg], "best_ms_per_iteration": min(ms), "worst_ms_per_iteration": max(ms),
                            "iterations_per_s": round(1e3 / min(ms), 1)}
            res["device20_over_max_iter1_time"] = round(res["device20"]["best_ms_per_iteration"] / res["max_iter1"]["best_ms_per_iteration"], 4)
            res["torch20_over_device20_time"] = round(res["torch20"]["best_ms_per_iteration"] / res["device20"]["best_ms_per_iteration"], 3)
            out["results"][str(size)] = res
            del model, opts, closures
            torch.cuda.empty_cache()
    finally:
        core_model.initialize_vgg = saved
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
