"""What the total-variation term (--tv-w) costs per L-BFGS step: one MI355X, bf16, synthetic VGG19 up to conv5_1 (the
runner's default taps), a full history (100 pairs, filled by untimed steps first, as bench.py does).

    python tools/tv_bench.py [--sizes 512 1024] [--rounds 6] [--steps 200] [--tv-w 1.0] [--out profiles/tv_loss_bench.json]

Two optimisers per size, each with its own image and history: one steps with ``tv_w = 0`` (the step as it is without the
feature: same op list, same program key), one with ``tv_w > 0`` (two more launches of stv_tv).  They alternate inside
every round, the order swapped from round to round, so that clock drift and other people's work on the host fall on
both.  Every round's steps/s and ms/step are kept: the spread of the ``tv_w = 0`` rounds is the yardstick a difference
has to be read against.  One JSON document (printed, and written to ``--out``): per size and leg the rounds, their
median, minimum and maximum, the difference of the medians in microseconds and percent, and the bytes the two extra
launches move (4 passes over the image: read + read, read + read-modify-write counted as 3 * H * W * 4 bytes each).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from style_transfer_visualizer_amd import core_model, synthetic  # noqa: E402
from style_transfer_visualizer_amd.optimizers import HipLBFGS  # noqa: E402

S, C = [0, 5, 10, 19, 28], [21]


def summary(step_ms: list[float]) -> dict:
    return {"rounds_ms_per_step": [round(v, 4) for v in step_ms], "rounds_steps_per_s": [round(1000.0 / v, 2) for v in step_ms],
            "median_ms_per_step": round(statistics.median(step_ms), 4), "min_ms_per_step": round(min(step_ms), 4),
            "max_ms_per_step": round(max(step_ms), 4), "median_steps_per_s": round(1000.0 / statistics.median(step_ms), 2)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=200, help="timed L-BFGS steps per leg and round (after a 100-step prefill)")
    ap.add_argument("--tv-w", type=float, default=1.0)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tv_loss_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/tv_bench.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    weights = synthetic.synthetic_conv_weights(3)
    saved = core_model.initialize_vgg
    core_model.initialize_vgg = lambda: core_model.build_vgg_features(weights).eval()
    legs = {"tv_w=0": 0.0, f"tv_w={args.tv_w:g}": float(args.tv_w)}
    out = {"tool": "tools/tv_bench.py", "device": torch.cuda.get_device_name(dev), "precision": args.precision, "history": 100,
           "steps_per_round": args.steps, "rounds": args.rounds, "tv_w": args.tv_w, "results": {}}
    try:
        for size in args.sizes:
            content = synthetic.synthetic_image(0, size, size).to(dev)
            style = synthetic.synthetic_image(1, size, size).to(dev)
            model = core_model.StyleContentModel(S, C, precision=args.precision).to(dev)
            model.set_targets(style, content)
            opts, images = {}, {}
            side = torch.cuda.Stream(device=dev)           # (the legacy default stream cannot be captured: the runner's own set-up)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for leg, w in legs.items():
                    xi = torch.randn(1, 3, size, size, generator=torch.Generator().manual_seed(0)).to(dev).requires_grad_(True)
                    opts[leg], images[leg] = HipLBFGS([xi], lr=1.0, history_size=100), xi
                    for _ in range(100):                   # fill the history (and capture the step's graph): untimed
                        opts[leg].step(lambda xi=xi, w=w: model.loss_and_grad(xi, 1e5, 1.0, tv_w=w)[2])
                side.synchronize()
                times: dict[str, list[float]] = {leg: [] for leg in legs}
                for r in range(args.rounds):
                    order = list(legs) if r % 2 == 0 else list(legs)[::-1]
                    for leg in order:
                        xi, opt, w = images[leg], opts[leg], legs[leg]
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(args.steps):
                            opt.step(lambda xi=xi, w=w: model.loss_and_grad(xi, 1e5, 1.0, tv_w=w)[2])
                        e1.record()
                        side.synchronize()
                        times[leg].append(e0.elapsed_time(e1) / args.steps)
            torch.cuda.current_stream(dev).wait_stream(side)
            res = {leg: summary(v) for leg, v in times.items()}
            base, with_tv = (res[leg]["median_ms_per_step"] for leg in legs)
            res["extra_us_per_step"] = round((with_tv - base) * 1000.0, 2)
            res["extra_percent"] = round(100.0 * (with_tv - base) / base, 3)
            res["tv_w=0_spread_percent"] = round(100.0 * (res["tv_w=0"]["max_ms_per_step"] - res["tv_w=0"]["min_ms_per_step"]) / base, 3)
            res["extra_bytes_per_step"] = 4 * 3 * size * size * 4
            out["results"][str(size)] = res
            del model, opts, images
            torch.cuda.empty_cache()
    finally:
        core_model.initialize_vgg = saved
    text = json.dumps(out, indent=1)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
