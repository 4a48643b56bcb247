"""What --preserve-color costs: one MI355X, synthetic VGG19, random start, L-BFGS.

    python tools/color_bench.py [--steps 200] [--size 512] [--rounds 3] [--parent-root DIR] [--out profiles/preserve_color_bench.json]

Three measurements, one JSON document (printed and written to ``--out``):

* each of the three launches (``stv_color_stats``, ``stv_color_affine``, ``stv_luma_transfer``) at 512^2 and 1024^2 with device
  events round the call: median and range of ``--reps`` launches after a warm-up, with the bytes each moves;
* the wall time of ``main.style_transfer`` (host clock between two device synchronisations: loads, set-up, the run, the PNG)
  for ``--steps`` bf16 steps at ``--size``^2 with ``off``, ``match`` and ``luma``: ``--rounds`` rounds after one untimed
  round, the legs alternating inside every round with the order reversed from round to round;
* the two stages on their own at ``--size``^2, host clock between two device synchronisations, median and range of ``--reps``
  calls: ``color.match_style_to_content`` (two statistics launches, two copies to the host, the 3x3 algebra, the affine
  launch) and ``color.transfer_luma`` (one launch).

``--parent-root DIR``: a built checkout of the commit in front of the feature.  Its ``off`` leg joins every round as one more
leg, run by a second process that stays alive for the whole measurement (``--serve``, driven over a pipe) and imports the
package from DIR - the same box, the same warm-up, interleaved with the other legs.
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
MODES = ("off", "match", "luma")


def _import_package(root: str):
    sys.path.insert(0, root)
    import style_transfer_visualizer_amd  # noqa: F401, PLC0415
    from style_transfer_visualizer_amd import config as stv_config  # noqa: PLC0415
    from style_transfer_visualizer_amd import main as stv_main  # noqa: PLC0415
    from style_transfer_visualizer_amd.type_defs import InputPaths  # noqa: PLC0415
    return stv_config, stv_main, InputPaths


def write_inputs(folder: str, size: int) -> tuple[str, str]:
    """Two seeded 8-bit pictures with correlated, differently tinted channels (full-rank colour covariances)."""
    import numpy as np  # noqa: PLC0415
    from PIL import Image  # noqa: PLC0415
    paths = []
    for name, seed, tint in (("content", 0, (0.9, 0.6, 0.4)), ("style", 1, (0.3, 0.5, 0.95))):
        rng = np.random.default_rng(seed)
        base = rng.random((size, size, 1))
        rgb = np.clip((0.6 * base + 0.4 * rng.random((size, size, 3))) * np.asarray(tint), 0, 1)
        path = os.path.join(folder, f"{name}.png")
        Image.fromarray((rgb * 255).astype(np.uint8)).save(path)
        paths.append(path)
    return paths[0], paths[1]


class Leg:
    """One tree's ``main.style_transfer``, timed."""

    def __init__(self, root: str, content: str, style: str, out_dir: str, steps: int, precision: str) -> None:
        import torch  # noqa: PLC0415
        self.torch = torch
        self.stv_config, self.stv_main, input_paths = _import_package(root)
        self.paths = input_paths(content_path=content, style_path=style)
        self.out_dir, self.steps, self.precision = out_dir, steps, precision

    def run(self, mode: str) -> float:
        cfg = self.stv_config.StyleTransferConfig.model_validate({})
        oc = cfg.optimization
        oc.steps, oc.init_method, oc.seed = self.steps, "random", 0
        if mode != "off":                     # (the tree in front of the feature has no such field)
            oc.preserve_color = mode
        cfg.hardware.device, cfg.hardware.precision = "cuda", self.precision
        cfg.video.create_video, cfg.video.final_only = False, True
        cfg.output.output, cfg.output.plot_losses = os.path.join(self.out_dir, mode), False
        self.torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.stv_main.style_transfer(self.paths, cfg)
        self.torch.cuda.synchronize()
        return time.perf_counter() - t0


def serve(args) -> None:
    """``run <mode>`` lines on stdin -> one line with the seconds each on stdout, until stdin closes."""
    leg = Leg(args.root, args.content, args.style, args.out_dir, args.steps, args.precision)
    real_stdout = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)                             # the package logs and shows a progress bar: keep the pipe for the answers
    real_stdout.write("ready\n")
    real_stdout.flush()
    for line in sys.stdin:
        words = line.split()
        if len(words) == 2 and words[0] == "run":
            real_stdout.write(f"{leg.run(words[1]):.6f}\n")
            real_stdout.flush()


class ParentLeg:
    """The ``off`` leg of another checkout, in a process of its own."""

    def __init__(self, root: str, content: str, style: str, out_dir: str, steps: int, precision: str) -> None:
        env = dict(os.environ, STV_SYNTHETIC_WEIGHTS="0")
        self.proc = subprocess.Popen(
            [sys.executable, os.path.abspath(__file__), "--serve", "--root", root, "--content", content, "--style", style,
             "--out-dir", out_dir, "--steps", str(steps), "--precision", precision],
            stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env, cwd=root)
        if self.proc.stdout.readline().strip() != "ready":
            raise SystemExit(f"the process for {root} did not start")

    def run(self, mode: str) -> float:
        self.proc.stdin.write(f"run {mode}\n")
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
    from style_transfer_visualizer_amd.constants import IMAGENET_MEAN, IMAGENET_STD  # noqa: PLC0415
    dev = torch.device("cuda:0")
    m12 = [0.9, 0.1, -0.05, 0.02, 1.1, 0.0, -0.1, 0.05, 0.8, 0.1, -0.2, 0.3]
    rows = []
    for size in (512, 1024):
        x, k = torch.randn(1, 3, size, size, device=dev), torch.randn(1, 3, size, size, device=dev)
        y = torch.empty_like(x)
        parts = ops.color_stats(x)
        image_bytes = x.numel() * 4
        launches = (("stv_color_stats", lambda: ops.color_stats(x, out=parts), image_bytes + parts.numel() * 8),
                    ("stv_color_affine", lambda: ops.color_affine(x, m12, out=y), 2 * image_bytes),
                    ("stv_luma_transfer", lambda: ops.luma_transfer(x, k, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=y), 3 * image_bytes))
        for name, launch, moved in launches:
            for _ in range(5):
                launch()
            torch.cuda.synchronize()
            times = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launch()
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1) * 1000.0)
            med = statistics.median(times)
            rows.append({"launch": name, "image": [size, size], "bytes_moved": moved, "median_us": round(med, 2),
                         "min_us": round(min(times), 2), "max_us": round(max(times), 2), "GB_per_s_at_median": round(moved / med / 1e3, 1)})
    return rows


def stage_times(size: int, reps: int) -> dict:
    import torch  # noqa: PLC0415

    from style_transfer_visualizer_amd import color  # noqa: PLC0415
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    content, style, result = (torch.randn(1, 3, size, size, generator=g).to(dev) for _ in range(3))
    rows = {}
    for name, call in (("match_style_to_content", lambda: color.match_style_to_content(style, content)),
                       ("transfer_luma", lambda: color.transfer_luma(result, content, normalize=True))):
        for _ in range(5):
            call()
        times = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e6)
        rows[name] = {"median_us": round(statistics.median(times), 1), "min_us": round(min(times), 1), "max_us": round(max(times), 1)}
    return rows


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the commit in front of the feature")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preserve_color_bench.json"))
    ap.add_argument("--serve", action="store_true", help=argparse.SUPPRESS)
    for name in ("--root", "--content", "--style", "--out-dir"):
        ap.add_argument(name, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.serve:
        serve(args)
        return
    os.environ.setdefault("STV_SYNTHETIC_WEIGHTS", "0")
    import torch  # noqa: PLC0415
    if not torch.cuda.is_available():
        raise SystemExit("tools/color_bench.py measures on the GPU: no device found")
    out = {"tool": "tools/color_bench.py", "device": torch.cuda.get_device_name(0), "precision": args.precision,
           "content": [args.size, args.size], "style": [args.size, args.size], "init_method": "random", "optimizer": "L-BFGS",
           "steps": args.steps, "rounds": args.rounds}
    with tempfile.TemporaryDirectory() as tmp:
        content, style = write_inputs(tmp, args.size)
        legs: dict[str, tuple] = {}
        here = Leg(ROOT, content, style, os.path.join(tmp, "out"), args.steps, args.precision)
        for mode in MODES:
            legs[mode] = (here, mode)
        parent = None
        if args.parent_root:
            parent = ParentLeg(os.path.abspath(args.parent_root), content, style, os.path.join(tmp, "out_parent"), args.steps, args.precision)
            legs["parent off"] = (parent, "off")
        try:
            for runner, mode in legs.values():              # untimed: code objects, tile choices, the VGG cache
                runner.run(mode)
            seconds: dict[str, list[float]] = {leg: [] for leg in legs}
            for r in range(args.rounds):
                for leg in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
                    runner, mode = legs[leg]
                    seconds[leg].append(round(runner.run(mode), 4))
        finally:
            if parent is not None:
                parent.close()
        out["style_transfer_wall_s"] = {leg: {"rounds": vals, "median": round(statistics.median(vals), 4), "range": [min(vals), max(vals)]}
                                        for leg, vals in seconds.items()}
        base = out["style_transfer_wall_s"]["off"]
        out["off_spread_s"] = round(base["range"][1] - base["range"][0], 4)
        out["median_minus_off_s"] = {leg: round(v["median"] - base["median"], 4) for leg, v in out["style_transfer_wall_s"].items() if leg != "off"}
    out["stages_host_clock"] = stage_times(args.size, args.reps)
    out["launches"] = kernel_times(args.reps)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
