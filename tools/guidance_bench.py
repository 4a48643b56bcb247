"""What spatial guidance (--content-mask, --style-mask) costs per L-BFGS step: one MI355X, bf16, synthetic VGG19 up to conv5_1
(the runner's default taps), a full history (100 pairs, filled by untimed steps first, as bench.py does).  The protocol of
tools/lap_bench.py.

    python tools/guidance_bench.py [--sizes 512 1024] [--rounds 6] [--steps 200] [--parent-root DIR]
                                   [--out profiles/guidance_bench.json]

Four optimisers per size, each with its own model, image and history: ``off`` (a model built without the option: the step as it
is without the feature, same op list, same program key), ``R=2 halves`` (left / right), ``R=4 quadrants`` and ``R=2 one weight 0``
(halves with region weights (1, 0): one slab, one chain per tap, half of every map unstyled).  They alternate inside every round,
the order reversed from round to round, after one untimed round.  Every round's ms/step is kept: the spread of the ``off`` rounds is
the yardstick a difference has to be read against.

``--parent-root DIR``: a built checkout of the commit in front of the feature.  Its step joins every round as one more leg
(``parent``), run by a second process that stays alive for the whole measurement (``--serve``, driven over a pipe) and imports the
package from DIR; this tree's ``off`` step then runs a second time in the same way, alone in a process of its own (``off alone``),
because a step's time depends a little on what else its process has allocated.  ``off_alone_minus_parent_us`` is to be read
against ``off_alone_spread_us`` and ``parent_spread_us``.

The tool also times ``stv_mask_split`` alone on every tap shape of every size with device events (``--split-reps`` launches per
measurement, R = 2 and R = 4): bytes moved ((1 + R) * n * C * element size + n label bytes) and GB/s.

One JSON document (printed, and written to ``--out``).
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
TAP_CHANNELS = (64, 128, 256, 512, 512)      # conv1_1 ... conv5_1, each at half the size of the one before
LEGS = {"off": None, "R=2 halves": (2, None), "R=4 quadrants": (4, None), "R=2 one weight 0": (2, (1.0, 0.0))}


def label_map(torch, regions: int, size: int):
    lab = torch.zeros(size, size, dtype=torch.uint8)
    lab[:, size // 2:] = 1
    if regions == 4:
        lab[size // 2:] += 2
    return lab


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

    def setup(self, key: str, size: int, guide: tuple | None) -> None:
        torch, core_model, synthetic = self.torch, self.core_model, self.synthetic
        weights = synthetic.synthetic_conv_weights(3)
        saved = core_model.initialize_vgg
        core_model.initialize_vgg = lambda: core_model.build_vgg_features(weights).eval()
        model_kw, label_kw = {}, {}                           # (the tree in front of the feature has no such keywords)
        if guide is not None:
            regions, region_w = guide
            model_kw = {"guide_regions": regions, "region_weights": region_w}
            lab = label_map(torch, regions, size)
            label_kw = {"content_labels": lab, "style_labels": lab}
        try:
            model = core_model.StyleContentModel(S, C, precision=self.precision, **model_kw).to(self.dev)
        finally:
            core_model.initialize_vgg = saved
        model.set_targets(synthetic.synthetic_image(1, size, size).to(self.dev), synthetic.synthetic_image(0, size, size).to(self.dev),
                          **label_kw)
        self.side.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(self.side):
            xi = torch.randn(1, 3, size, size, generator=torch.Generator().manual_seed(0)).to(self.dev).requires_grad_(True)
            opt = self.lbfgs([xi], lr=1.0, history_size=100)
            closure = lambda: model.loss_and_grad(xi, 1e5, 1.0)[2]      # noqa: E731
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

    def split_alone(self, size: int, reps: int) -> list[dict]:
        """stv_mask_split alone on every tap shape of ``size``: the median of 5 measurements of ``reps`` launches each."""
        torch = self.torch
        from style_transfer_visualizer_amd import ops  # noqa: PLC0415
        dtype = torch.bfloat16 if self.precision == "bf16" else torch.float32
        rows = []
        with torch.cuda.stream(self.side):
            for k, ch in enumerate(TAP_CHANNELS):
                side = size >> k
                feat = torch.randn(side, side, ch, device=self.dev).to(dtype)
                for regions in (2, 4):
                    lab = label_map(torch, regions, side).to(self.dev)
                    out = torch.empty(regions, side, side, ch, device=self.dev, dtype=dtype)
                    ops.mask_split(feat, lab, regions, out=out)
                    times = []
                    for _ in range(5):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(reps):
                            ops.mask_split(feat, lab, regions, out=out)
                        e1.record()
                        self.side.synchronize()
                        times.append(e0.elapsed_time(e1) * 1000.0 / reps)
                    us = statistics.median(times)
                    nbytes = (1 + regions) * feat.numel() * feat.element_size() + side * side
                    rows.append({"tap": f"conv{k + 1}_1", "H": side, "W": side, "C": ch, "R": regions, "bytes": nbytes,
                                 "us": round(us, 2), "GB_per_s": round(nbytes / us / 1000.0, 1)})
        return rows


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
            leg.setup(words[1], int(words[1]), None)
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
    ap.add_argument("--rounds", type=int, default=6, help="timed rounds, after one untimed round")
    ap.add_argument("--steps", type=int, default=200, help="timed L-BFGS steps per leg and round (after a 100-step prefill)")
    ap.add_argument("--split-reps", type=int, default=50, help="launches of stv_mask_split per measurement")
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the commit in front of the feature")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guidance_bench.json"))
    ap.add_argument("--serve", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.serve:
        serve(args)
        return
    import torch  # noqa: PLC0415
    if not torch.cuda.is_available():
        raise SystemExit("tools/guidance_bench.py measures on the GPU: no device found")
    here = StepLeg(ROOT, args.precision)
    parent = ParentLeg(os.path.abspath(args.parent_root), args.precision) if args.parent_root else None
    alone = ParentLeg(ROOT, args.precision) if args.parent_root else None
    served = {"parent": parent, "off alone": alone} if parent is not None else {}
    out = {"tool": "tools/guidance_bench.py", "device": torch.cuda.get_device_name(0), "precision": args.precision, "history": 100,
           "steps_per_round": args.steps, "rounds": args.rounds, "untimed_rounds": 1, "parent": bool(parent), "results": {},
           "mask_split_alone": {}}
    es = 2 if args.precision == "bf16" else 4
    try:
        for size in args.sizes:
            out["mask_split_alone"][str(size)] = here.split_alone(size, args.split_reps)
            for leg, guide in LEGS.items():
                here.setup(leg, size, guide)
            for proc in served.values():
                proc.ask(f"setup {size}")
            names = list(LEGS) + list(served)
            times: dict[str, list[float]] = {leg: [] for leg in names}
            for r in range(-1, args.rounds):                  # round -1: untimed
                for leg in (names if r % 2 == 0 else names[::-1]):
                    ms = float(served[leg].ask(f"run {size} {args.steps}")) if leg in served else here.run(leg, args.steps)
                    if r >= 0:
                        times[leg].append(ms)
            res = {leg: summary(v) for leg, v in times.items()}
            base = res["off"]["median_ms_per_step"]
            tap_bytes = sum((size >> k) ** 2 * ch * es for k, ch in enumerate(TAP_CHANNELS))
            for leg, guide in LEGS.items():
                if guide is None:
                    continue
                n_active = sum(1 for w in (guide[1] or (1.0,) * guide[0]) if w > 0)
                res[leg]["extra_us_per_step"] = round((res[leg]["median_ms_per_step"] - base) * 1000.0, 2)
                res[leg]["extra_percent"] = round(100.0 * (res[leg]["median_ms_per_step"] - base) / base, 3)
                res[leg]["active_regions"] = n_active
                # per region one write of every tap activation, one read by the Gram pass, one by the 1x1 product
                res[leg]["slab_bytes_per_step"] = 3 * n_active * tap_bytes
            res["tap_activation_bytes"] = tap_bytes
            res["off_spread_us"] = round((res["off"]["max_ms_per_step"] - res["off"]["min_ms_per_step"]) * 1000.0, 2)
            if parent is not None:
                for leg, name in (("parent", "parent"), ("off alone", "off_alone")):
                    res[name + "_spread_us"] = round((res[leg]["max_ms_per_step"] - res[leg]["min_ms_per_step"]) * 1000.0, 2)
                res["off_minus_parent_us"] = round((base - res["parent"]["median_ms_per_step"]) * 1000.0, 2)
                res["off_alone_minus_parent_us"] = round(
                    (res["off alone"]["median_ms_per_step"] - res["parent"]["median_ms_per_step"]) * 1000.0, 2)
                for proc in served.values():
                    proc.ask(f"drop {size}")
            out["results"][str(size)] = res
            for leg in LEGS:
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
