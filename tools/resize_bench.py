"""What input resizing (--content-size, --style-size, --style-scale) costs: one MI355X.

    python tools/resize_bench.py [--steps 200] [--size 512] [--rounds 5] [--parent-root DIR] [--out profiles/resize_bench.json]

Three measurements, one JSON document (printed and written to ``--out``), after the method of tools/color_bench.py:

* each of the two launches of ``ops.resize`` (``stv_resize_axis``: columns into the intermediate, then rows) with device
  events round the call, for the three filters, at a camera-sized downscale (3000x2000 -> longer side 1024) and a 512^2 ->
  768^2 upscale: median and range of ``--reps`` launches after a warm-up, with the bytes each moves (input read once, output
  written once; the tables are a few KB).  The tables are on the device before the clock starts;
* the whole stage - ``ops.resize`` as ``main`` calls it: table look-up, one upload per pass, both launches, the two
  allocations - on the host clock between two device synchronisations, next to PIL's ``Image.resize`` of the same picture
  (8-bit RGB, the same filter) on the host, which is what a user does today in front of the run;
* the wall time of ``main.style_transfer`` (host clock between two device synchronisations: loads, set-up, the run, the PNG)
  for ``--steps`` bf16 steps at ``--size``^2 with the options at 0 (``off``) and with ``--content-size`` / ``--style-scale``
  that resize both images by a few pixels to ``--size``^2 (``on``): ``--rounds`` rounds after one untimed round, the legs
  alternating inside every round with the order reversed from round to round.

``--parent-root DIR``: a built checkout of the commit in front of the feature.  Its run joins every round as one more leg,
made by a second process that stays alive for the whole measurement (``--serve``, driven over a pipe) and imports the
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
FILTERS = ("bilinear", "bicubic", "lanczos")
SHAPES = (("camera downscale", (2000, 3000), (683, 1024)), ("upscale", (512, 512), (768, 768)))


def _import_package(root: str):
    sys.path.insert(0, root)
    import style_transfer_visualizer_amd  # noqa: F401, PLC0415
    from style_transfer_visualizer_amd import config as stv_config  # noqa: PLC0415
    from style_transfer_visualizer_amd import main as stv_main  # noqa: PLC0415
    from style_transfer_visualizer_amd.type_defs import InputPaths  # noqa: PLC0415
    return stv_config, stv_main, InputPaths


def _picture(seed: int, H: int, W: int):
    import numpy as np  # noqa: PLC0415
    rng = np.random.default_rng(seed)
    base = rng.random((H, W, 1))
    return (np.clip(0.6 * base + 0.4 * rng.random((H, W, 3)), 0, 1) * 255).astype(np.uint8)


def write_inputs(folder: str, size: int) -> dict[str, str]:
    """Seeded 8-bit pictures: a pair at ``size``^2 (the ``off`` legs) and a pair a few pixels larger (the ``on`` leg resizes
    it to ``size``^2, so every leg optimises the same number of pixels)."""
    from PIL import Image  # noqa: PLC0415
    paths = {}
    for name, seed, side in (("content", 0, size), ("style", 1, size), ("content_big", 0, size + 24), ("style_big", 1, size + 40)):
        paths[name] = os.path.join(folder, f"{name}.png")
        Image.fromarray(_picture(seed, side, side)).save(paths[name])
    return paths


class Leg:
    """One tree's ``main.style_transfer``, timed."""

    def __init__(self, root: str, inputs: dict[str, str], out_dir: str, steps: int, precision: str, size: int) -> None:
        import torch  # noqa: PLC0415
        self.torch = torch
        self.stv_config, self.stv_main, self.input_paths = _import_package(root)
        self.inputs, self.out_dir, self.steps, self.precision, self.size = inputs, out_dir, steps, precision, size

    def run(self, mode: str) -> float:
        cfg = self.stv_config.StyleTransferConfig.model_validate({})
        oc = cfg.optimization
        oc.steps, oc.init_method, oc.seed = self.steps, "random", 0
        suffix = ""
        if mode == "on":                      # (the tree in front of the feature has no such fields)
            oc.content_size, oc.style_scale, suffix = self.size, 1.0, "_big"
        cfg.hardware.device, cfg.hardware.precision = "cuda", self.precision
        cfg.video.create_video, cfg.video.final_only = False, True
        cfg.output.output, cfg.output.plot_losses = os.path.join(self.out_dir, mode), False
        paths = self.input_paths(content_path=self.inputs["content" + suffix], style_path=self.inputs["style" + suffix])
        self.torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.stv_main.style_transfer(paths, cfg)
        self.torch.cuda.synchronize()
        return time.perf_counter() - t0


def serve(args) -> None:
    """``run <mode>`` lines on stdin -> one line with the seconds each on stdout, until stdin closes."""
    leg = Leg(args.root, json.loads(args.inputs), args.out_dir, args.steps, args.precision, args.size)
    real_stdout = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)                             # the package logs and shows a progress bar: keep the pipe for the answers
    real_stdout.write("ready\n")
    real_stdout.flush()
    for line in sys.stdin:
        words = line.split()
        if len(words) == 2 and words[0] == "run":       # noqa: PLR2004
            real_stdout.write(f"{leg.run(words[1]):.6f}\n")
            real_stdout.flush()


class ParentLeg:
    """The run of another checkout, in a process of its own."""

    def __init__(self, root: str, inputs: dict[str, str], out_dir: str, steps: int, precision: str, size: int) -> None:
        env = dict(os.environ, STV_SYNTHETIC_WEIGHTS="0")
        self.proc = subprocess.Popen(
            [sys.executable, os.path.abspath(__file__), "--serve", "--root", root, "--inputs", json.dumps(inputs),
             "--out-dir", out_dir, "--steps", str(steps), "--precision", precision, "--size", str(size)],
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


def _summary(times: list[float], digits: int = 2) -> dict:
    return {"median_us": round(statistics.median(times), digits), "min_us": round(min(times), digits), "max_us": round(max(times), digits)}


def launch_times(reps: int) -> list[dict]:
    """Device events round each of the two passes, tables already on the device."""
    import torch  # noqa: PLC0415

    from style_transfer_visualizer_amd import _lib, ops  # noqa: PLC0415
    from style_transfer_visualizer_amd import resize as rz  # noqa: PLC0415
    dev = torch.device("cuda:0")
    lib = _lib.load()
    rows = []
    for label, (H, W), (Ho, Wo) in SHAPES:
        x = torch.randn(3, H, W, device=dev)
        mid, y = torch.empty(3, H, Wo, device=dev), torch.empty(3, Ho, Wo, device=dev)
        for name in FILTERS:
            for what, src, dst, h, w, n_out, axis in (("columns", x, mid, H, W, Wo, 1), ("rows", mid, y, H, Wo, Ho, 0)):
                start, count, weights = (torch.from_numpy(a.copy()).to(dev) for a in rz.axis_table(w if axis == 1 else h, n_out, name))
                K = int(weights.shape[1])

                def launch(src=src, dst=dst, h=h, w=w, n_out=n_out, axis=axis, start=start, count=count, weights=weights, K=K):
                    _lib.check(lib.stv_resize_axis(src.data_ptr(), dst.data_ptr(), 3, h, w, n_out, axis, start.data_ptr(),
                                                   count.data_ptr(), weights.data_ptr(), K, torch.cuda.current_stream().cuda_stream),
                               "stv_resize_axis")
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
                moved = (src.numel() + dst.numel()) * 4
                row = {"case": label, "filter": name, "pass": what, "input": list(src.shape[-2:]), "output": list(dst.shape[-2:]),
                       "taps_max": K, "bytes_moved": moved, **_summary(times)}
                row["GB_per_s_at_median"] = round(moved / row["median_us"] / 1e3, 1)
                rows.append(row)
    return rows


def stage_times(reps: int) -> list[dict]:
    """``ops.resize`` on the host clock between two synchronisations, and PIL's resize of the same 8-bit picture."""
    import torch  # noqa: PLC0415
    from PIL import Image  # noqa: PLC0415

    from style_transfer_visualizer_amd import ops  # noqa: PLC0415
    dev = torch.device("cuda:0")
    pil_filter = {"bilinear": Image.Resampling.BILINEAR, "bicubic": Image.Resampling.BICUBIC, "lanczos": Image.Resampling.LANCZOS}
    rows = []
    for label, (H, W), (Ho, Wo) in SHAPES:
        picture = Image.fromarray(_picture(5, H, W))
        x = torch.randn(1, 3, H, W, device=dev)
        for name in FILTERS:
            for _ in range(5):
                ops.resize(x, (Ho, Wo), name)
            device_us, host_us = [], []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ops.resize(x, (Ho, Wo), name)
                torch.cuda.synchronize()
                device_us.append((time.perf_counter() - t0) * 1e6)
            for _ in range(max(3, reps // 5)):
                t0 = time.perf_counter()
                picture.resize((Wo, Ho), pil_filter[name])
                host_us.append((time.perf_counter() - t0) * 1e6)
            rows.append({"case": label, "filter": name, "input": [H, W], "output": [Ho, Wo],
                         "ops_resize": _summary(device_us, 1), "pil_resize_on_the_host": _summary(host_us, 1)})
    return rows


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the commit in front of the feature")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize_bench.json"))
    ap.add_argument("--serve", action="store_true", help=argparse.SUPPRESS)
    for name in ("--root", "--inputs", "--out-dir"):
        ap.add_argument(name, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.serve:
        serve(args)
        return
    os.environ.setdefault("STV_SYNTHETIC_WEIGHTS", "0")
    import torch  # noqa: PLC0415
    if not torch.cuda.is_available():
        raise SystemExit("tools/resize_bench.py measures on the GPU: no device found")
    out = {"tool": "tools/resize_bench.py", "device": torch.cuda.get_device_name(0), "precision": args.precision,
           "content": [args.size, args.size], "style": [args.size, args.size], "init_method": "random", "optimizer": "L-BFGS",
           "steps": args.steps, "rounds": args.rounds,
           "on_leg": f"content {args.size + 24}^2 and style {args.size + 40}^2 resized to {args.size}^2 (lanczos)"}
    with tempfile.TemporaryDirectory() as tmp:
        inputs = write_inputs(tmp, args.size)
        here = Leg(ROOT, inputs, os.path.join(tmp, "out"), args.steps, args.precision, args.size)
        legs: dict[str, tuple] = {"off": (here, "off"), "on": (here, "on")}
        parent = None
        if args.parent_root:
            parent = ParentLeg(os.path.abspath(args.parent_root), inputs, os.path.join(tmp, "out_parent"), args.steps,
                               args.precision, args.size)
            legs["parent"] = (parent, "off")
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
    out["stage_host_clock"] = stage_times(args.reps)
    out["launches"] = launch_times(args.reps)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
