"""What several style images and per-layer style weights cost: one MI355X, synthetic VGG19, random start, L-BFGS.

    python tools/style_mix_bench.py [--steps 200] [--size 512] [--rounds 3] [--parent-root DIR] [--out profiles/style_mix_bench.json]

Two measurements, one JSON document (printed and written to ``--out``):

* the wall time of ``main.style_transfer`` (host clock between two device synchronisations: loads, set-up, the run, the PNG)
  for ``--steps`` bf16 steps at ``--size``^2 with one style image (``one``), with three (``three``, blend 0.5 / 0.3 / 0.2), and
  each of the two with the layer weights 1, 0.8, 0.5, 0.3, 0.1 (``one layer_w``, ``three layer_w``): ``--rounds`` rounds after
  one untimed round, the legs alternating inside every round with the order reversed from round to round;
* the ``stv_gram_blend`` launch with device events round the call, for the Gram sizes of VGG19's five style layers with 3 and
  with 8 tables: median and range of ``--reps`` launches after a warm-up, with the bytes each moves.

``--parent-root DIR``: a built checkout of the commit in front of the feature.  Its single-style leg joins every round as one
more leg (``parent one``), run by a second process that stays alive for the whole measurement (``--serve``, driven over a
pipe) and imports the package from DIR - the same box, the same warm-up, interleaved with the other legs.  ``one_spread_s``
and ``parent_spread_s`` record the range of each tree's own repeated single-style rounds: a difference inside them is nothing.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("one", "three", "one layer_w", "three layer_w")
BLEND = [0.5, 0.3, 0.2]
LAYER_W = [1.0, 0.8, 0.5, 0.3, 0.1]


def _import_package(root: str):
    sys.path.insert(0, root)
    import style_transfer_visualizer_amd  # noqa: F401, PLC0415
    from style_transfer_visualizer_amd import config as stv_config  # noqa: PLC0415
    from style_transfer_visualizer_amd import main as stv_main  # noqa: PLC0415
    from style_transfer_visualizer_amd.type_defs import InputPaths  # noqa: PLC0415
    return stv_config, stv_main, InputPaths


def write_inputs(folder: str, size: int) -> list[str]:
    """Four seeded 8-bit pictures: the content and three styles."""
    import numpy as np  # noqa: PLC0415
    from PIL import Image  # noqa: PLC0415
    paths = []
    for seed, name in enumerate(("content", "style", "style2", "style3")):
        rng = np.random.default_rng(seed)
        rgb = np.clip(0.6 * rng.random((size, size, 1)) + 0.4 * rng.random((size, size, 3)), 0, 1)
        path = os.path.join(folder, f"{name}.png")
        Image.fromarray((rgb * 255).astype(np.uint8)).save(path)
        paths.append(path)
    return paths


class Leg:
    """One tree's ``main.style_transfer``, timed."""

    def __init__(self, root: str, images: list[str], out_dir: str, steps: int, precision: str) -> None:
        import torch  # noqa: PLC0415
        self.torch = torch
        self.stv_config, self.stv_main, self.input_paths = _import_package(root)
        self.images, self.out_dir, self.steps, self.precision = images, out_dir, steps, precision

    def run(self, leg: str) -> float:
        cfg = self.stv_config.StyleTransferConfig.model_validate({})
        oc = cfg.optimization
        oc.steps, oc.init_method, oc.seed = self.steps, "random", 0
        paths = self.input_paths(content_path=self.images[0], style_path=self.images[1])
        if leg.startswith("three"):           # (the tree in front of the feature has none of these fields)
            paths = self.input_paths(self.images[0], self.images[1], tuple(self.images[2:4]))
            oc.style_blend = list(BLEND)
        if leg.endswith("layer_w"):
            oc.style_layer_weights = list(LAYER_W)
        cfg.hardware.device, cfg.hardware.precision = "cuda", self.precision
        cfg.video.create_video, cfg.video.final_only = False, True
        cfg.output.output, cfg.output.plot_losses = os.path.join(self.out_dir, leg.replace(" ", "_")), False
        self.torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.stv_main.style_transfer(paths, cfg)
        self.torch.cuda.synchronize()
        return time.perf_counter() - t0


def serve(args) -> None:
    """``run <leg>`` lines on stdin -> one line with the seconds each on stdout, until stdin closes."""
    leg = Leg(args.root, args.images.split(os.pathsep), args.out_dir, args.steps, args.precision)
    real_stdout = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)                             # the package logs and shows a progress bar: keep the pipe for the answers
    real_stdout.write("ready\n")
    real_stdout.flush()
    for line in sys.stdin:
        words = line.split(maxsplit=1)
        if len(words) == 2 and words[0] == "run":
            real_stdout.write(f"{leg.run(words[1].strip()):.6f}\n")
            real_stdout.flush()


class ParentLeg:
    """The single-style leg of another checkout, in a process of its own."""

    def __init__(self, root: str, images: list[str], out_dir: str, steps: int, precision: str) -> None:
        env = dict(os.environ, STV_SYNTHETIC_WEIGHTS="0")
        self.proc = subprocess.Popen(
            [sys.executable, os.path.abspath(__file__), "--serve", "--root", root, "--images", os.pathsep.join(images),
             "--out-dir", out_dir, "--steps", str(steps), "--precision", precision],
            stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env, cwd=root)
        if self.proc.stdout.readline().strip() != "ready":
            raise SystemExit(f"the process for {root} did not start")

    def run(self, leg: str) -> float:
        self.proc.stdin.write(f"run {leg}\n")
        self.proc.stdin.flush()
        answer = self.proc.stdout.readline().strip()
        if not answer:
            raise SystemExit("the parent's process ended early")
        return float(answer)

    def close(self) -> None:
        self.proc.stdin.close()
        self.proc.wait(timeout=60)


def kernel_times(reps: int) -> list[dict]:
    import torch  # noqa: PLC0415

    from style_transfer_visualizer_amd import ops  # noqa: PLC0415
    dev = torch.device("cuda:0")
    rows = []
    for K in (3, 8):
        weights = [1.0 / K] * K
        for C in (64, 128, 256, 512):
            stack = torch.randn(K, C, C, device=dev) * 3e-3
            out = torch.empty(C, C, device=dev)
            moved = (K + 1) * C * C * 4
            for _ in range(5):
                ops.gram_blend(stack, weights, out=out)
            torch.cuda.synchronize()
            times = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ops.gram_blend(stack, weights, out=out)
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1) * 1000.0)
            med = statistics.median(times)
            rows.append({"launch": "stv_gram_blend", "tables": K, "table": [C, C], "bytes_moved": moved, "median_us": round(med, 2),
                         "min_us": round(min(times), 2), "max_us": round(max(times), 2),
                         "GB_per_s_at_median": round(moved / med / 1e3, 1)})
    return rows


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the commit in front of the feature")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "style_mix_bench.json"))
    ap.add_argument("--serve", action="store_true", help=argparse.SUPPRESS)
    for name in ("--root", "--images", "--out-dir"):
        ap.add_argument(name, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.serve:
        serve(args)
        return
    os.environ.setdefault("STV_SYNTHETIC_WEIGHTS", "0")
    import torch  # noqa: PLC0415
    if not torch.cuda.is_available():
        raise SystemExit("tools/style_mix_bench.py measures on the GPU: no device found")
    out = {"tool": "tools/style_mix_bench.py", "device": torch.cuda.get_device_name(0), "precision": args.precision,
           "content": [args.size, args.size], "styles": [args.size, args.size], "init_method": "random", "optimizer": "L-BFGS",
           "steps": args.steps, "rounds": args.rounds, "style_blend": BLEND, "style_layer_weights": LAYER_W}
    with tempfile.TemporaryDirectory() as tmp:
        images = write_inputs(tmp, args.size)
        here = Leg(ROOT, images, os.path.join(tmp, "out"), args.steps, args.precision)
        legs: dict[str, tuple] = {leg: (here, leg) for leg in LEGS}
        parent = None
        if args.parent_root:
            parent = ParentLeg(os.path.abspath(args.parent_root), images, os.path.join(tmp, "out_parent"), args.steps, args.precision)
            legs["parent one"] = (parent, "one")
        try:
            for runner, leg in legs.values():               # untimed: code objects, tile choices, the VGG cache
                runner.run(leg)
            seconds: dict[str, list[float]] = {leg: [] for leg in legs}
            for r in range(args.rounds):
                for leg in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
                    runner, what = legs[leg]
                    seconds[leg].append(round(runner.run(what), 4))
        finally:
            if parent is not None:
                parent.close()
        out["style_transfer_wall_s"] = {leg: {"rounds": vals, "median": round(statistics.median(vals), 4), "range": [min(vals), max(vals)]}
                                        for leg, vals in seconds.items()}
        walls = out["style_transfer_wall_s"]
        out["one_spread_s"] = round(walls["one"]["range"][1] - walls["one"]["range"][0], 4)
        if parent is not None:
            out["parent_spread_s"] = round(walls["parent one"]["range"][1] - walls["parent one"]["range"][0], 4)
        base = walls["parent one" if parent is not None else "one"]
        out["median_minus_" + ("parent_one" if parent is not None else "one") + "_s"] = {
            leg: round(v["median"] - base["median"], 4) for leg, v in walls.items() if v is not base}
    out["launches"] = kernel_times(args.reps)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
