"""What the Laplacian loss (--lap-w, --lap-pool) costs per L-BFGS step: one MI355X, bf16, synthetic VGG19 up to conv5_1 (the
runner's default taps), a full history (100 pairs, filled by untimed steps first, as bench.py does).

    python tools/lap_bench.py [--sizes 512 1024] [--rounds 6] [--steps 200] [--lap-w 100] [--parent-root DIR]
                              [--out profiles/lap_loss_bench.json]

Three optimisers per size, each with its own model, image and history: ``lap_w=0`` (a model built without pools, as a run
without the option builds it: the step as it is without the feature, same op list, same program key), ``pools=4`` and
``pools=4,16`` with ``lap_w > 0`` (two more launches of stv_lap per pool: the LOSS form reads the image once, the GRAD form
reads and rewrites the gradient).  They alternate inside every round, the order reversed from round to round, so that clock
drift and other people's work on the host fall on all of them.  Every round's ms/step is kept: the spread of the ``lap_w=0``
rounds is the yardstick a difference has to be read against.

``--parent-root DIR``: a built checkout of the commit in front of the feature.  Its step joins every round as one more leg
(``parent``), run by a second process that stays alive for the whole measurement (``--serve``, driven over a pipe) and imports
the package from DIR - the same box, the same prefill, interleaved with the other legs.  This tree's ``lap_w=0`` step then
runs a second time in the same way, alone in a process of its own (``lap_w=0 alone``): the process of the three legs above holds
three models and three L-BFGS histories, the parent's process one, and a step's time depends a little on what else the process
has allocated.  With the option off the step must sit inside the spread of its own rounds and of the parent's:
``lap_w=0_alone_minus_parent_us`` against ``lap_w=0_alone_spread_us`` and ``parent_spread_us``.

One JSON document (printed, and written to ``--out``): per size and leg the rounds, their median, minimum and maximum, the
difference of the medians to ``lap_w=0`` in microseconds and percent, and the bytes the extra launches move at least (per pool
one image read, one gradient read and one gradient write of C*H*W*4 bytes each, plus the residual written and read).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, C = [0, 5, 10, 19, 28], [21]


class StepLeg:
    """One tree's fused L-BFGS step at one size: a model, an image and an optimiser of its own, prefilled."""

    def __init__(self, root: str, precision: str) -> None:
        sys.path.insert(0, root)
        import torch  # noqa: PLC0415
        from style_transfer_visualizer_amd import core_model, synthetic  # noqa: PLC0415
        from style_transfer_visualizer_amd.optimizers import HipLBFGS  # noqa: PLC0415
        self.torch, self.core_model, self.synthetic, self.lbfgs = torch, core_model, synthetic, HipLBFGS
        self.precision = precision
        self.dev = torch.device("cuda:0")
        self.side = torch.cuda.Stream(device=self.dev)        # (the legacy default stream cannot be captured)
        self.state: dict = {}

    def setup(self, key: str, size: int, pools: tuple, lap_w: float) -> None:
        torch, core_model, synthetic = self.torch, self.core_model, self.synthetic
        weights = synthetic.synthetic_conv_weights(3)
        saved = core_model.initialize_vgg
        core_model.initialize_vgg = lambda: core_model.build_vgg_features(weights).eval()
        try:
            model = core_model.StyleContentModel(S, C, precision=self.precision, **({"lap_pools": list(pools)} if pools else {})).to(self.dev)
        finally:
            core_model.initialize_vgg = saved
        model.set_targets(synthetic.synthetic_image(1, size, size).to(self.dev), synthetic.synthetic_image(0, size, size).to(self.dev))
        kw = {"lap_w": lap_w} if lap_w else {}                # (the tree in front of the feature has no such keyword)
        self.side.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(self.side):
            xi = torch.randn(1, 3, size, size, generator=torch.Generator().manual_seed(0)).to(self.dev).requires_grad_(True)
            opt = self.lbfgs([xi], lr=1.0, history_size=100)
            closure = lambda: model.loss_and_grad(xi, 1e5, 1.0, **kw)[2]      # noqa: E731
            for _ in range(100):                              # fill the history (and capture the step's graph): untimed
                opt.step(closure)
            self.side.synchronize()
        self.state[key] = (model, xi, opt, closure)

    def run(self, key: str, steps: int) -> float:
        """ms per step over ``steps`` steps, device events round them."""
        torch = self.torch
        _, _, opt, closure = self.state[key]
        with torch.cuda.stream(self.side):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                opt.step(closure)
            e1.record()
            self.side.synchronize()
        return e0.elapsed_time(e1) / steps

    def drop(self, key: str) -> None:
        self.state.pop(key, None)
        self.torch.cuda.empty_cache()


def serve(args) -> None:
    """``setup <size>`` / ``run <size> <steps>`` / ``drop <size>`` lines on stdin -> one answer line each on stdout."""
    leg = StepLeg(args.root, args.precision)
    real_stdout = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)                                             # keep the pipe for the answers
    real_stdout.write("ready\n")
    real_stdout.flush()
    for line in sys.stdin:
        words = line.split()
        if not words:
            continue
        if words[0] == "setup":
            leg.setup(words[1], int(words[1]), (), 0.0)
            answer = "ok"
        elif words[0] == "run":
            answer = f"{leg.run(words[1], int(words[2])):.6f}"
        else:
            leg.drop(words[1])
            answer = "ok"
        real_stdout.write(answer + "\n")
        real_stdout.flush()


class ParentLeg:
    """The step of another checkout, in a process of its own."""

    def __init__(self, root: str, precision: str) -> None:
        self.proc = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve", "--root", root, "--precision", precision],
                                     stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=root)
        if self.proc.stdout.readline().strip() != "ready":
            raise SystemExit(f"the process for {root} did not start")

    def ask(self, line: str) -> str:
        self.proc.stdin.write(line + "\n")
        self.proc.stdin.flush()
        answer = self.proc.stdout.readline().strip()
        if not answer:
            raise SystemExit("the parent's process ended early")
        return answer

    def close(self) -> None:
        self.proc.stdin.close()
        self.proc.wait(timeout=60)


def summary(step_ms: list[float]) -> dict:
    return {"rounds_ms_per_step": [round(v, 4) for v in step_ms], "median_ms_per_step": round(statistics.median(step_ms), 4),
            "min_ms_per_step": round(min(step_ms), 4), "max_ms_per_step": round(max(step_ms), 4),
            "median_steps_per_s": round(1000.0 / statistics.median(step_ms), 2)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=200, help="timed L-BFGS steps per leg and round (after a 100-step prefill)")
    ap.add_argument("--lap-w", type=float, default=100.0)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the commit in front of the feature")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lap_loss_bench.json"))
    ap.add_argument("--serve", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.serve:
        serve(args)
        return
    import torch  # noqa: PLC0415
    if not torch.cuda.is_available():
        raise SystemExit("tools/lap_bench.py measures on the GPU: no device found")
    here = StepLeg(ROOT, args.precision)
    parent = ParentLeg(os.path.abspath(args.parent_root), args.precision) if args.parent_root else None
    alone = ParentLeg(ROOT, args.precision) if args.parent_root else None
    served = {"parent": parent, "lap_w=0 alone": alone} if parent is not None else {}
    legs = {"lap_w=0": ((), 0.0), "pools=4": ((4,), float(args.lap_w)), "pools=4,16": ((4, 16), float(args.lap_w))}
    out = {"tool": "tools/lap_bench.py", "device": torch.cuda.get_device_name(0), "precision": args.precision, "history": 100,
           "steps_per_round": args.steps, "rounds": args.rounds, "lap_w": args.lap_w, "parent": bool(parent), "results": {}}
    try:
        for size in args.sizes:
            for leg, (pools, w) in legs.items():
                here.setup(leg, size, pools, w)
            for proc in served.values():
                proc.ask(f"setup {size}")
            names = list(legs) + list(served)
            times: dict[str, list[float]] = {leg: [] for leg in names}
            for r in range(args.rounds):
                for leg in (names if r % 2 == 0 else names[::-1]):
                    if leg in served:
                        times[leg].append(float(served[leg].ask(f"run {size} {args.steps}")))
                    else:
                        times[leg].append(here.run(leg, args.steps))
            res = {leg: summary(v) for leg, v in times.items()}
            base = res["lap_w=0"]["median_ms_per_step"]
            for leg, (pools, _) in legs.items():
                if pools:
                    res[leg]["extra_us_per_step"] = round((res[leg]["median_ms_per_step"] - base) * 1000.0, 2)
                    res[leg]["extra_percent"] = round(100.0 * (res[leg]["median_ms_per_step"] - base) / base, 3)
                    res[leg]["launches_added"] = 2 * len(pools)
                    res[leg]["extra_bytes_per_step_at_least"] = sum(3 * 3 * size * size * 4 + 2 * 3 * (size // p) * (size // p) * 4 for p in pools)
            res["lap_w=0_spread_us"] = round((res["lap_w=0"]["max_ms_per_step"] - res["lap_w=0"]["min_ms_per_step"]) * 1000.0, 2)
            if parent is not None:
                for leg, name in (("parent", "parent"), ("lap_w=0 alone", "lap_w=0_alone")):
                    res[name + "_spread_us"] = round((res[leg]["max_ms_per_step"] - res[leg]["min_ms_per_step"]) * 1000.0, 2)
                res["lap_w=0_minus_parent_us"] = round((base - res["parent"]["median_ms_per_step"]) * 1000.0, 2)
                res["lap_w=0_alone_minus_parent_us"] = round(
                    (res["lap_w=0 alone"]["median_ms_per_step"] - res["parent"]["median_ms_per_step"]) * 1000.0, 2)
                for proc in served.values():
                    proc.ask(f"drop {size}")
            out["results"][str(size)] = res
            for leg in legs:
                here.drop(leg)
    finally:
        for proc in served.values():
            proc.close()
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
