"""fp32 / bf16x3 / bf16 side by side on one GPU: L-BFGS steps at a full history (100 pairs, filled by untimed steps
first, as bench.py does), the fused closure alone (forward + Gram/content losses + backward) of the full VGG19 stack
up to conv5_1 (synthetic weights, the runner's default taps), and its forward + Gram half alone.

    python tools/precision_bench.py [--sizes 512 1024] [--reps 30] [--rounds 3]

The three precisions alternate inside every round (order rotated per round) so that clock drift falls on all of them;
the best round is reported.  One JSON line: per size and precision L-BFGS steps/s and ms per step, the closure ms and
closures/s, the forward + Gram ms, and the fraction of a 2.5 PFLOP/s matrix-core peak that the closure's conv + Gram
FLOPs reach.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from style_transfer_visualizer_amd import core_model, synthetic  # noqa: E402
from style_transfer_visualizer_amd.optimizers import HipLBFGS  # noqa: E402

S, C = [0, 5, 10, 19, 28], [21]
PEAK = 2.5e15


def closure_flops(size: int) -> float:
    """Conv (forward, dgrad) + Gram products of one closure, 2 FLOP per multiply-add (the first layer's dgrad excluded).
    The closure runs the stack up to its last tap, conv5_1 (layer 28): the first 17 entries of VGG19_CFG."""
    total, s, first = 0.0, size, True
    chans = []
    for e in synthetic.VGG19_CFG[:17]:
        if e == "M":
            s //= 2
            continue
        cin = chans[-1] if chans else 3
        total += 2.0 * s * s * 9 * cin * e * (1 if first else 2)
        first = False
        chans.append(e)
    for i, layer in enumerate([0, 5, 10, 19, 28]):
        c = [64, 128, 256, 512, 512][i]
        n = (size >> i) ** 2
        total += 2.0 * n * c * c * 2          # Gram forward + its backward (seed product)
    return total


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precisions", nargs="+", default=["fp32", "bf16x3", "bf16"])
    ap.add_argument("--steps", type=int, default=20, help="timed L-BFGS steps per round (after a 100-step prefill)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    weights = synthetic.synthetic_conv_weights(3)
    saved = core_model.initialize_vgg
    core_model.initialize_vgg = lambda: core_model.build_vgg_features(weights).eval()
    precisions = args.precisions
    out = {"tool": "tools/precision_bench.py", "device": torch.cuda.get_device_name(dev), "peak_flops": PEAK, "results": {}}
    try:
        for size in args.sizes:
            content = synthetic.synthetic_image(0, size, size).to(dev)
            style = synthetic.synthetic_image(1, size, size).to(dev)
            x = synthetic.synthetic_image(2, size, size).to(dev).requires_grad_(True)
            models, opts, images = {}, {}, {}
            for p in precisions:
                m = core_model.StyleContentModel(S, C, precision=p).to(dev)
                m.set_targets(style, content)
                for _ in range(3):
                    m.loss_and_grad(x, 1e5, 1.0)
                models[p] = m
                # the optimizer's own image and a full history: 100 untimed steps (each precision its own trajectory)
                xi = torch.randn(1, 3, size, size, generator=torch.Generator().manual_seed(0)).to(dev).requires_grad_(True)
                opts[p], images[p] = HipLBFGS([xi], lr=1.0, history_size=100), xi
                for _ in range(100):
                    opts[p].step(lambda m=m, xi=xi: m.loss_and_grad(xi, 1e5, 1.0)[2])
            torch.cuda.synchronize()
            best = {p: {"closure_ms": float("inf"), "fwd_gram_ms": float("inf"), "step_ms": float("inf")} for p in precisions}
            for r in range(args.rounds):
                k = r % len(precisions)
                order = precisions[k:] + precisions[:k]
                for p in order:
                    m = models[p]
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    xi, opt = images[p], opts[p]
                    e0.record()
                    for _ in range(args.steps):
                        opt.step(lambda m=m, xi=xi: m.loss_and_grad(xi, 1e5, 1.0)[2])
                    e1.record()
                    torch.cuda.synchronize()
                    best[p]["step_ms"] = min(best[p]["step_ms"], e0.elapsed_time(e1) / args.steps)
                    e0.record()
                    for _ in range(args.reps):
                        m.loss_and_grad(x, 1e5, 1.0)
                    e1.record()
                    torch.cuda.synchronize()
                    best[p]["closure_ms"] = min(best[p]["closure_ms"], e0.elapsed_time(e1) / args.reps)
                    with torch.no_grad():
                        e0.record()
                        for _ in range(args.reps):
                            m(x.detach())
                        e1.record()
                    torch.cuda.synchronize()
                    best[p]["fwd_gram_ms"] = min(best[p]["fwd_gram_ms"], e0.elapsed_time(e1) / args.reps)
            fl = closure_flops(size)
            res = {}
            for p in precisions:
                ms = best[p]["closure_ms"]
                res[p] = {"lbfgs_steps_per_s": round(1000.0 / best[p]["step_ms"], 2), "lbfgs_step_ms": round(best[p]["step_ms"], 4),
                          "closure_ms": round(ms, 4), "closures_per_s": round(1000.0 / ms, 2),
                          "fwd_gram_ms": round(best[p]["fwd_gram_ms"], 4),
                          "mfma_fraction_of_2p5_pflops": round(fl / (ms * 1e-3) / PEAK, 4)}
            if "fp32" in best and "bf16x3" in best:
                res["bf16x3_over_fp32_steps"] = round(best["fp32"]["step_ms"] / best["bf16x3"]["step_ms"], 3)
                res["bf16x3_over_fp32_closure"] = round(best["fp32"]["closure_ms"] / best["bf16x3"]["closure_ms"], 3)
            out["results"][str(size)] = res
            del models, opts, images
            torch.cuda.empty_cache()
    finally:
        core_model.initialize_vgg = saved
    print(json.dumps(out))


if __name__ == "__main__":
    main()
