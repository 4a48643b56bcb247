"""What a coarse-to-fine run (--pyramid-levels) buys and costs: one MI355X, bf16, synthetic VGG19 up to conv5_1 (the runner's
default taps), 1024x1024 content, 512x512 style, random start, L-BFGS.

    python tools/pyramid_bench.py [--steps 500] [--levels 3] [--rounds 3] [--out profiles/pyramid_bench.json]

Two legs through ``pyramid.run_pyramid``, alternating inside every round with the order swapped from round to round (clock
drift and other people's work on the host fall on both), after one untimed round of each (code objects, tile choices):

* ``levels=1``: N steps at 1024^2 - the run as it is without the feature (one level is the plain set-up and runner);
* ``levels=L``: the same N steps split evenly over L levels, 1024 >> (L-1) first.

N defaults to the 500 steps of BASELINE configs[2].  Per leg and round: the seconds inside each level's
``OptimizationRunner.run`` (host clock between two device synchronisations), the seconds of set-up in front of each level
(model, targets, start image, optimiser: everything between the previous level's end and this level's first step), and the
FULL objective of the returned image - style, content and total score at 1024^2, evaluated by one fresh model that both
legs share.  Apart from the runs, every resize launch a 3-level run makes is timed on its own with device events
(``--resize-reps`` launches each after a warm-up, median).  One JSON document, printed and written to ``--out``.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from style_transfer_visualizer_amd import _lib, core_model, ops, optimization, pyramid, synthetic  # noqa: E402
from style_transfer_visualizer_amd import config as stv_config  # noqa: E402

S, C = [0, 5, 10, 19, 28], [21]
STYLE_W, CONTENT_W = 1e5, 1.0


class _Bar:
    def update(self, n=1):
        return None

    def set_postfix(self, *a, **k):
        return None

    def close(self):
        return None


class TimedRunner(optimization.OptimizationRunner):
    """The runner, unchanged, with a device synchronisation and a host clock reading on both sides of ``run``."""

    spans: list[tuple[float, float]] = []

    def run(self):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = super().run()
        torch.cuda.synchronize()
        type(self).spans.append((t0, time.perf_counter()))
        return out


def run_leg(content, style, dev, levels: int, steps: int, precision: str) -> tuple[torch.Tensor, dict]:
    cfg = stv_config.StyleTransferConfig.model_validate({})
    oc = cfg.optimization
    oc.steps, oc.pyramid_levels, oc.init_method = steps, levels, "random"
    oc.style_w, oc.content_w, oc.style_layers, oc.content_layers = STYLE_W, CONTENT_W, list(S), list(C)
    cfg.hardware.precision = precision
    cfg.video.create_video = False
    TimedRunner.spans = []
    torch.cuda.synchronize()
    start = time.perf_counter()
    image, _, _ = pyramid.run_pyramid(content, style, dev, cfg, progress_bar=_Bar(), seed=0)
    torch.cuda.synchronize()
    end = time.perf_counter()
    spans = TimedRunner.spans
    setup = [spans[k][0] - (spans[k - 1][1] if k else start) for k in range(len(spans))]
    optimise = [b - a for a, b in spans]
    return image.detach(), {
        "level_shapes": [list(s) for s in pyramid.level_shapes(content.shape[-2], content.shape[-1], levels)],
        "level_steps": pyramid.level_steps(steps, levels),
        "setup_s_per_level": [round(v, 4) for v in setup], "optimisation_s_per_level": [round(v, 4) for v in optimise],
        "setup_s": round(sum(setup), 4), "optimisation_s": round(sum(optimise), 4), "wall_s": round(end - start, 4)}


def resize_times(dev, reps: int) -> list[dict]:
    """Every launch of a 3-level run at 1024^2 content / 512^2 style, device events round the call, median of ``reps``."""
    D, U = _lib.RESIZE_DOWN2, _lib.RESIZE_UP2
    rows = []
    for what, mode, size in (("content DOWN2", D, 1024), ("content DOWN2", D, 512), ("style DOWN2", D, 512), ("style DOWN2", D, 256),
                             ("image UP2", U, 256), ("image UP2", U, 512)):
        x = torch.randn(1, 3, size, size, device=dev)
        out = ops.resize2x(x, mode)
        for _ in range(5):
            ops.resize2x(x, mode, out=out)
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.resize2x(x, mode, out=out)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1000.0)
        moved = (x.numel() + out.numel()) * 4
        med = statistics.median(times)
        rows.append({"launch": what, "in": [size, size], "out": list(out.shape[-2:]), "bytes_moved": moved,
                     "median_us": round(med, 2), "min_us": round(min(times), 2), "max_us": round(max(times), 2),
                     "GB_per_s_at_median": round(moved / med / 1e3, 1)})
    return rows


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500, help="optimiser steps per leg (BASELINE configs[2]: 500)")
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--size", type=int, default=1024, help="content side; the style image is half of it")
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--resize-reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pyramid_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/pyramid_bench.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    weights = synthetic.synthetic_conv_weights(3)
    saved_vgg, saved_runner = core_model.initialize_vgg, optimization.OptimizationRunner
    core_model.initialize_vgg = lambda: core_model.build_vgg_features(weights).eval()
    optimization.OptimizationRunner = TimedRunner
    legs = {"levels=1": 1, f"levels={args.levels}": args.levels}
    out = {"tool": "tools/pyramid_bench.py", "device": torch.cuda.get_device_name(dev), "precision": args.precision,
           "content": [args.size, args.size], "style": [args.size // 2, args.size // 2], "init_method": "random", "optimizer": "L-BFGS",
           "steps": args.steps, "rounds": args.rounds, "style_w": STYLE_W, "content_w": CONTENT_W, "legs": {}}
    try:
        content = synthetic.synthetic_image(0, args.size, args.size).to(dev)
        style = synthetic.synthetic_image(1, args.size // 2, args.size // 2).to(dev)
        judge = core_model.StyleContentModel(S, C, precision=args.precision).to(dev)       # the full-size objective, for both legs
        judge.set_targets(style, content)

        def objective(image: torch.Tensor) -> dict:
            x = image.clone().requires_grad_(True)
            side = torch.cuda.Stream(device=dev)            # (the legacy default stream cannot be captured: the runner's own set-up)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                s, c, t = judge.loss_and_grad(x, STYLE_W, CONTENT_W)
                vals = {"style_score": float(s), "content_score": float(c), "total": float(t)}
            torch.cuda.current_stream(dev).wait_stream(side)
            return vals

        start = torch.randn(1, 3, args.size, args.size, generator=torch.Generator().manual_seed(0)).to(dev)
        out["objective_of_a_random_image"] = objective(start)
        out["objective_of_the_content_image"] = objective(content)
        for leg, levels in legs.items():                    # untimed: code objects, tile choices, the VGG cache
            run_leg(content, style, dev, levels, min(args.steps, 30), args.precision)
        rounds: dict[str, list[dict]] = {leg: [] for leg in legs}
        for r in range(args.rounds):
            order = list(legs) if r % 2 == 0 else list(legs)[::-1]
            for leg in order:
                image, row = run_leg(content, style, dev, legs[leg], args.steps, args.precision)
                row["objective"] = objective(image)
                rounds[leg].append(row)
                del image
                torch.cuda.empty_cache()
        for leg, rows in rounds.items():
            out["legs"][leg] = {"rounds": rows}
            for key in ("optimisation_s", "setup_s", "wall_s"):
                vals = [row[key] for row in rows]
                out["legs"][leg][f"median_{key}"] = round(statistics.median(vals), 4)
                out["legs"][leg][f"range_{key}"] = [min(vals), max(vals)]
            out["legs"][leg]["median_total_objective"] = statistics.median(row["objective"]["total"] for row in rows)
        a, b = (out["legs"][leg] for leg in legs)
        out["optimisation_time_ratio"] = round(b["median_optimisation_s"] / a["median_optimisation_s"], 4)
        out["wall_time_ratio"] = round(b["median_wall_s"] / a["median_wall_s"], 4)
        out["total_objective_ratio"] = round(b["median_total_objective"] / a["median_total_objective"], 4)
        out["resize_launches"] = resize_times(dev, args.resize_reps)
    finally:
        core_model.initialize_vgg, optimization.OptimizationRunner = saved_vgg, saved_runner
    text = json.dumps(out, indent=1)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
