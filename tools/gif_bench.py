"""What a timelapse GIF costs a run, and that the step is the parent's: one MI355X.

    python tools/gif_bench.py [--size 512] [--steps 300] [--rounds 4] [--parent-root DIR] [--bench-py-pairs 3] [--out profiles/gif_bench.json]

Legs, each a whole ``OptimizationRunner`` run of ``--steps`` L-BFGS steps (bf16, synthetic VGG19, history 100, the loss log at its
default cadence), host clock between two device synchronisations, ms per step:

  1. ``off``            no frame sink: the run as it is without ``--gif``;
  2. ``host sink``      an injected memory sink, a frame every 10 steps: what a user could do before - ``image_io.frame_uint8``, one
                        launch and one blocking copy per frame;
  3. ``device 10``      ``gif.DeviceGifCollector``, a frame every 10 steps: two launches per frame, no synchronisation;
  4. ``device 1``       the same with a frame every step.

This tree's legs run in one process; with ``--parent-root DIR`` (a built checkout of the commit in front of the feature) a second
process runs legs 1 and 2 of that tree, interleaved with them.  One untimed round, then ``--rounds`` rounds whose order is
reversed from round to round; median and range over the rounds.  ``close()`` of the two collector legs is timed apart, split
into histogram readback, median cut, map launches, copy and PIL encode.  Then the two kernels alone, device events round one
launch, at 512^2 and 1024^2 for a constant-colour frame (every atomic on one counter) and a random frame (no two pixels in
a row alike); the size of the 30-frame file with and without dither; and, with ``--parent-root``, ``bench.py --gpus 1 --steps 200
--warmup 100`` of the two trees in alternating fresh processes.  No threshold anywhere: the figures, with their spreads.
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
S, C = [0, 5, 10, 19, 28], [21]
LEGS = {"off": None, "host sink": 10, "device 10": 10, "device 1": 1}          # name -> save_every
EXPECTATION = ("a saved frame costs two launch-bound launches of the order of 10 us each, as every pointwise launch measured in this "
               "project did: at a frame every 10 steps under 1 % of a 0.85 ms step, at a frame every step a few per cent; the host-sink "
               "leg pays one synchronisation per frame (the queue drains: tens of us and a lost overlap); PIL's LZW dominates close(), "
               "about 5 ms per random 512^2 frame on a CPU - random frames are its worst case; the constant-colour histogram launch "
               "is slower than the random one by the serialisation of 262144 atomics on one counter")


class _Bar:
    def update(self, n=1):
        return None

    def set_postfix(self, *a, **k):
        return None

    def close(self):
        return None


class _MemorySink:
    def __init__(self):
        self.frames = []

    def append_data(self, frame):
        self.frames.append(frame)

    def close(self):
        return None


class Legs:
    """One tree's run at one size: a model with targets and one image tensor, reset in place for every round."""

    def __init__(self, root: str, size: int, steps: int) -> None:
        sys.path.insert(0, root)
        import torch  # noqa: PLC0415
        from style_transfer_visualizer_amd import config as stv_config  # noqa: PLC0415
        from style_transfer_visualizer_amd import core_model, optimization, synthetic  # noqa: PLC0415
        from style_transfer_visualizer_amd.optimizers import HipLBFGS  # noqa: PLC0415
        self.torch, self.optimization, self.lbfgs, self.stv_config = torch, optimization, HipLBFGS, stv_config
        self.root, self.size, self.steps = root, size, steps
        self.dev = torch.device("cuda:0")
        weights = synthetic.synthetic_conv_weights(3)
        saved = core_model.initialize_vgg
        core_model.initialize_vgg = lambda: core_model.build_vgg_features(weights).eval()
        try:
            self.model = core_model.StyleContentModel(S, C, precision="bf16").to(self.dev)
        finally:
            core_model.initialize_vgg = saved
        self.model.set_targets(synthetic.synthetic_image(1, size, size).to(self.dev), synthetic.synthetic_image(0, size, size).to(self.dev))
        self.x0 = torch.randn(1, 3, size, size, generator=torch.Generator().manual_seed(0)).to(self.dev)
        self.x = self.x0.clone().requires_grad_(True)
        self.last_close: dict = {}
        self.last_bytes = 0

    def run(self, leg: str, dither: str = "ordered", out: str | None = None) -> float:
        """ms per step of one whole run of leg ``leg``; a collector's ``close()`` comes after the clock has stopped."""
        torch = self.torch
        cfg = self.stv_config.StyleTransferConfig.model_validate({})
        cfg.optimization.steps = self.steps
        every = LEGS[leg]
        cfg.video.save_every = every if every else self.steps + 1
        sink = None
        if leg == "host sink":
            sink = _MemorySink()
        elif every:
            from style_transfer_visualizer_amd import gif  # noqa: PLC0415
            path = out or os.path.join(tempfile.gettempdir(), f"gif_bench_{os.getpid()}.gif")
            sink = gif.DeviceGifCollector(path, 10, self.size, self.size, self.steps // every, dither=dither, device=self.dev)
        with torch.no_grad():
            self.x.copy_(self.x0)
        self.x.grad = None
        opt = self.lbfgs([self.x], lr=1.0, history_size=100, tolerance_grad=0.0, tolerance_change=0.0)
        runner = self.optimization.OptimizationRunner(self.model, self.x, cfg, optimizer=opt, progress_bar=_Bar(), gif_collector=sink)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        runner.run()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1000.0 / self.steps
        if sink is not None and every and leg != "host sink":
            t0 = time.perf_counter()
            sink.close()
            self.last_close = {"frames": sink.count, "total_s": round(time.perf_counter() - t0, 4),
                               **{k: round(v, 4) for k, v in sink.timings.items()}}
            self.last_bytes = os.path.getsize(sink.path)
            if out is None:
                os.remove(sink.path)
        return ms


def serve(args) -> None:
    """``run <leg>`` / ``close`` / ``size <dither>`` lines on stdin -> one answer line each."""
    real_stdout = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)                                             # keep the pipe for the answers
    legs = Legs(args.root, args.size, args.steps)
    real_stdout.write("ready\n")
    real_stdout.flush()
    for line in sys.stdin:
        words = line.strip().split(" ", 1)
        if not words[0]:
            continue
        if words[0] == "run":
            answer = f"{legs.run(words[1]):.6f}"
        elif words[0] == "close":
            answer = json.dumps(legs.last_close)
        else:
            legs.run("device 10", dither=words[1])
            answer = str(legs.last_bytes)
        real_stdout.write(answer + "\n")
        real_stdout.flush()


class LegProcess:
    """One tree's legs in a process of its own, under a time limit of its own."""

    def __init__(self, root: str, args) -> None:
        cmd = ["timeout", "-k", "10", str(args.leg_timeout), sys.executable, os.path.abspath(__file__), "--serve", "--root", root,
               "--size", str(args.size), "--steps", str(args.steps)]
        self.proc = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=root)
        if self.proc.stdout.readline().strip() != "ready":
            raise SystemExit(f"the process for {root} did not start")

    def ask(self, line: str) -> str:
        self.proc.stdin.write(line + "\n")
        self.proc.stdin.flush()
        answer = self.proc.stdout.readline().strip()
        if not answer:          # it ended (a fault, its time limit): nothing more is started
            raise SystemExit(f"a leg's process ended early (exit status {self.proc.wait(timeout=60)})")
        return answer

    def close(self) -> None:
        try:
            self.proc.stdin.close()
            self.proc.wait(timeout=60)
        except (OSError, subprocess.TimeoutExpired):
            self.proc.kill()


def summary(step_ms: list[float]) -> dict:
    return {"rounds_ms_per_step": [round(v, 4) for v in step_ms], "median_ms_per_step": round(statistics.median(step_ms), 4),
            "min_ms_per_step": round(min(step_ms), 4), "max_ms_per_step": round(max(step_ms), 4)}


def measure_runs(args) -> dict:
    procs = {"this": LegProcess(ROOT, args)}
    order = [("this", name) for name in LEGS]
    if args.parent_root:
        procs["parent"] = LegProcess(os.path.abspath(args.parent_root), args)
        order = [("parent", "off"), ("this", "off"), ("parent", "host sink"), ("this", "host sink"), ("this", "device 10"), ("this", "device 1")]
    out: dict = {}
    try:
        for who, name in order:                               # one untimed round
            procs[who].ask(f"run {name}")
        times: dict[str, list[float]] = {f"{who}: {name}": [] for who, name in order}
        closes: dict[str, list[dict]] = {"device 10": [], "device 1": []}
        for r in range(args.rounds):
            for who, name in (order if r % 2 == 0 else order[::-1]):
                times[f"{who}: {name}"].append(float(procs[who].ask(f"run {name}")))
                if name in closes:
                    closes[name].append(json.loads(procs[who].ask("close")))
        out["ms_per_step"] = {key: summary(v) for key, v in times.items()}
        base = out["ms_per_step"]["this: off"]["median_ms_per_step"]
        out["minus_off_us_per_step"] = {key: round((v["median_ms_per_step"] - base) * 1000.0, 2) for key, v in out["ms_per_step"].items()}
        out["close"] = {name: {"rounds": rows, "median_total_s": statistics.median(r["total_s"] for r in rows),
                               "median_encode_s": statistics.median(r["encode_s"] for r in rows)} for name, rows in closes.items()}
        out["file_bytes_30_frames"] = {d: int(procs["this"].ask(f"size {d}")) for d in ("ordered", "none")}
    finally:
        for proc in procs.values():
            proc.close()
    return out


def launch_times(reps: int) -> list[dict]:
    import torch  # noqa: PLC0415
    sys.path.insert(0, ROOT)
    from style_transfer_visualizer_amd import _lib, ops  # noqa: PLC0415
    dev = torch.device("cuda:0")
    rows = []

    def timed(call) -> dict:
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1000.0)
        return {"median_us": round(statistics.median(times), 2), "min_us": round(min(times), 2), "max_us": round(max(times), 2)}
    palette = torch.randint(0, 256, (256, 3), dtype=torch.uint8, device=dev)
    for size in (512, 1024):
        frames = {"constant": torch.full((size, size, 3), 77, dtype=torch.uint8, device=dev),
                  "random": torch.randint(0, 256, (size, size, 3), dtype=torch.uint8, device=dev)}
        hist = torch.zeros(_lib.GIF_HIST_BINS, dtype=torch.int32, device=dev)
        index = torch.empty(size, size, dtype=torch.uint8, device=dev)
        for kind, frame in frames.items():
            rows.append({"launch": "stv_frame_hist (runs and uniform waves merged)", "image": [size, size], "frame": kind,
                         **timed(lambda f=frame: ops.frame_hist(f, hist))})
            rows.append({"launch": "stv_gif_map (256 colours, spread 16)", "image": [size, size], "frame": kind,
                         **timed(lambda f=frame: ops.gif_map(f, palette, 16, out=index))})
    return rows


def bench_py_pairs(args) -> dict:
    cmd = ["timeout", "-k", "10", "300", sys.executable, "bench.py", "--gpus", "1", "--steps", "200", "--warmup", "100"]
    got: dict[str, list[float]] = {"parent_steps_per_s": [], "this_tree_steps_per_s": []}
    for _ in range(args.bench_py_pairs):
        for key, root in (("parent_steps_per_s", os.path.abspath(args.parent_root)), ("this_tree_steps_per_s", ROOT)):
            done = subprocess.run(cmd, cwd=root, capture_output=True, text=True, check=False)
            if done.returncode != 0:          # a fault or a time limit: nothing more is started
                raise SystemExit(f"bench.py in {root} ended with status {done.returncode}: {done.stderr[-400:]}")
            got[key].append(float(json.loads(done.stdout.strip().splitlines()[-1])["value"]))
    return {"command": "bench.py --gpus 1 --steps 200 --warmup 100", "order": "alternating fresh processes on one box, the parent first",
            **got, **{k.replace("steps_per_s", "median"): statistics.median(v) for k, v in got.items()}}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the commit in front of the feature")
    ap.add_argument("--bench-py-pairs", type=int, default=3, help="with --parent-root: pairs of bench.py runs (0: none)")
    ap.add_argument("--leg-timeout", type=int, default=500, help="seconds a leg's process may live")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gif_bench.json"))
    ap.add_argument("--serve", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.serve:
        serve(args)
        return
    out = {"tool": "tools/gif_bench.py", "device": None, "size": args.size, "steps_per_run": args.steps, "rounds": args.rounds,
           "untimed_rounds": 1, "parent": bool(args.parent_root), "expectation_written_before_measuring": EXPECTATION}

    def write() -> None:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    if args.parent_root and args.bench_py_pairs > 0:          # first: this process has not touched the device yet
        out["bench_py"] = bench_py_pairs(args)
        write()
    out["runs"] = measure_runs(args)
    write()
    import torch  # noqa: PLC0415
    if not torch.cuda.is_available():
        raise SystemExit("tools/gif_bench.py measures on the GPU: no device found")
    out["device"] = torch.cuda.get_device_name(0)
    out["launches"] = launch_times(args.reps)
    write()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
