"""What a Motion-JPEG timelapse costs a run, and that the step is the parent's: one MI355X.

    python tools/mjpeg_bench.py [--size 512] [--steps 300] [--rounds 4] [--parent-root DIR] [--bench-py-pairs 3] [--out profiles/mjpeg_bench.json]

Legs, each a whole ``OptimizationRunner`` run of ``--steps`` L-BFGS steps (bf16, synthetic VGG19, history 100, the loss log at its
default cadence), host clock between two device synchronisations, ms per step:

  1. ``off``            no frame sink: the run as it is with ``--no-video``;
  2. ``host sink``      an injected memory sink as ``video_writer``, a frame every 10 steps: what a user could do before -
                        ``image_io.frame_uint8``, one launch and one blocking copy per frame;
  3. ``device 10``      ``mjpeg.DeviceMjpegWriter``, a frame every 10 steps: two launches per frame, no synchronisation;
  4. ``device 1``       the same with a frame every step.

This tree's legs run in one process; with ``--parent-root DIR`` (a built checkout of the commit in front of the feature) a second
process runs leg 1 of that tree, interleaved with them.  One untimed round, then ``--rounds`` rounds whose order is reversed from
round to round; median and range over the rounds.  ``close()`` of the two writer legs is timed apart and split into its stages.
Then the four kernels alone, device events round one launch, and PIL's ``Image.save(..., "JPEG")`` of the same frames on the
host - what a user would otherwise do with the frames of a host sink; PSNR and size of the device encoder against PIL's on three
96x80 frames; and, with ``--parent-root``, ``bench.py --gpus 1 --steps 200 --warmup 100`` of the two trees in alternating fresh
processes.  No threshold anywhere: the figures, with their spreads.
"""
from __future__ import annotations

import argparse
import io
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

from gif_bench import _Bar, _MemorySink, bench_py_pairs, summary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, C = [0, 5, 10, 19, 28], [21]
LEGS = {"off": None, "host sink": 10, "device 10": 10, "device 1": 1}          # name -> save_every
EXPECTATION = ("a saved frame costs two launch-bound launches (the frame conversion and stv_jpeg_dct) of the order of 10 us each, as "
               "every pointwise launch measured in this project did: at a frame every 10 steps under 1 % of a 0.85 ms step, at a frame "
               "every step a few per cent; the host-sink leg pays one synchronisation per frame; close() is dominated by the copy of "
               "the streams and the host's byte stuffing and file write (tens of ms for 30 frames of 512^2), the three entropy "
               "launches are tens of us each; PIL needs a few ms per 512^2 frame on a CPU, so the device path should be several "
               "times cheaper per frame than encoding host frames with PIL")


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
        self.last_frames: list = []

    def run(self, leg: str) -> float:
        """ms per step of one whole run of leg ``leg``; a writer's ``close()`` comes after the clock has stopped."""
        torch = self.torch
        cfg = self.stv_config.StyleTransferConfig.model_validate({})
        cfg.optimization.steps = self.steps
        every = LEGS[leg]
        cfg.video.save_every = every if every else self.steps + 1
        sink = None
        if leg == "host sink":
            sink = _MemorySink()
        elif every:
            from style_transfer_visualizer_amd import mjpeg  # noqa: PLC0415
            path = os.path.join(tempfile.gettempdir(), f"mjpeg_bench_{os.getpid()}.avi")
            sink = mjpeg.DeviceMjpegWriter(path, 10, self.size, self.size, self.steps // every, quality=10, device=self.dev)
        with torch.no_grad():
            self.x.copy_(self.x0)
        self.x.grad = None
        opt = self.lbfgs([self.x], lr=1.0, history_size=100, tolerance_grad=0.0, tolerance_change=0.0)
        runner = self.optimization.OptimizationRunner(self.model, self.x, cfg, optimizer=opt, progress_bar=_Bar(), video_writer=sink)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        runner.run()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1000.0 / self.steps
        if leg == "host sink":
            self.last_frames = sink.frames
        elif sink is not None:
            t0 = time.perf_counter()
            sink.close()
            self.last_close = {"frames": sink.count, "file_bytes": sink.file_bytes, "total_s": round(time.perf_counter() - t0, 4),
                               **{k: round(v, 4) for k, v in sink.timings.items()}}
            os.remove(sink.path)
        return ms

    def pil_seconds(self) -> dict:
        """PIL's baseline JPEG encoder over the frames of the last host-sink leg, at the quality the writer legs use."""
        from PIL import Image  # noqa: PLC0415
        from style_transfer_visualizer_amd import mjpeg  # noqa: PLC0415
        Q = mjpeg.jpeg_quality(10)
        t0 = time.perf_counter()
        total = 0
        for frame in self.last_frames:
            buf = io.BytesIO()
            Image.fromarray(frame).save(buf, "JPEG", quality=Q, subsampling=2, optimize=False)
            total += buf.tell()
        seconds = time.perf_counter() - t0
        n = max(len(self.last_frames), 1)
        return {"frames": len(self.last_frames), "jpeg_quality": Q, "total_s": round(seconds, 4), "ms_per_frame": round(1000 * seconds / n, 3),
                "bytes": total}


def serve(args) -> None:
    """``run <leg>`` / ``close`` / ``pil`` lines on stdin -> one answer line each."""
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
            answer = json.dumps(legs.pil_seconds())
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


def measure_runs(args) -> dict:
    procs = {"this": LegProcess(ROOT, args)}
    order = [("this", name) for name in LEGS]
    if args.parent_root:
        procs["parent"] = LegProcess(os.path.abspath(args.parent_root), args)
        order = [("parent", "off"), *order]
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
                               "median_ms_per_frame": round(1000 * statistics.median(r["total_s"] / r["frames"] for r in rows), 3)}
                        for name, rows in closes.items()}
        out["pil_on_the_host_sinks_frames"] = json.loads(procs["this"].ask("pil"))
    finally:
        for proc in procs.values():
            proc.close()
    return out


def launch_times(reps: int) -> list[dict]:
    import numpy as np  # noqa: PLC0415
    import torch  # noqa: PLC0415
    sys.path.insert(0, ROOT)
    from style_transfer_visualizer_amd import mjpeg, ops  # noqa: PLC0415
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
    qtabs = mjpeg.quant_tables(mjpeg.jpeg_quality(10))
    n_frames = 30
    for size in (512, 1024):
        y, x = np.mgrid[0:size, 0:size]
        smooth = np.stack([128 + 100 * np.sin(x / 37.0), 128 + 100 * np.cos(y / 23.0), (x + y) * 255 // (2 * size - 2)], axis=2)
        frames = {"smooth": torch.from_numpy(np.clip(smooth, 0, 255).astype(np.uint8)).to(dev),
                  "random": torch.randint(0, 256, (size, size, 3), dtype=torch.uint8, device=dev)}
        blocks = ops.jpeg_blocks(size, size)
        coef = torch.empty(n_frames, blocks, 64, dtype=torch.int16, device=dev)
        for kind, frame in frames.items():
            rows.append({"launch": "stv_jpeg_dct (one frame)", "image": [size, size], "frame": kind,
                         **timed(lambda f=frame: ops.jpeg_dct(f, qtabs, out=coef[0]))})
            for i in range(n_frames):
                ops.jpeg_dct(frame, qtabs, out=coef[i])
            bits = ops.jpeg_block_bits(coef)
            offsets, totals = ops.jpeg_scan(bits)
            region = (((totals.cpu().numpy().view(np.uint32).astype(np.int64) + 7) // 8) + 3) // 4 * 4
            base = torch.from_numpy(np.concatenate([[0], np.cumsum(region)[:-1]]).astype(np.int32)).to(dev)
            stream = torch.zeros(int(region.sum()), dtype=torch.uint8, device=dev)
            rows.append({"launch": f"stv_jpeg_block_bits ({n_frames} frames)", "image": [size, size], "frame": kind,
                         **timed(lambda: ops.jpeg_block_bits(coef, out=bits))})
            rows.append({"launch": f"stv_jpeg_scan ({n_frames} frames)", "image": [size, size], "frame": kind,
                         **timed(lambda: ops.jpeg_scan(bits, offsets, totals))})
            # (the OR of a stream onto itself leaves it as it is: the buffer need not be zeroed between the repetitions)
            rows.append({"launch": f"stv_jpeg_emit ({n_frames} frames)", "image": [size, size], "frame": kind, "stream_bytes": int(region.sum()),
                         **timed(lambda: ops.jpeg_emit(coef, offsets, base, stream))})
    return rows


def quality_pairs() -> list[dict]:
    """PSNR against the source and file size of the device encoder and of PIL's (``subsampling=2, optimize=False``) on three 96x80
    frames - noise in [64, 128)^3, a gradient, a smooth image-like frame - at ``--quality`` 1, 5 and 9 (libjpeg 15, 55, 95)."""
    import numpy as np  # noqa: PLC0415
    import torch  # noqa: PLC0415
    from PIL import Image  # noqa: PLC0415
    sys.path.insert(0, ROOT)
    from style_transfer_visualizer_amd import mjpeg  # noqa: PLC0415
    H, W = 96, 80
    y, x = np.mgrid[0:H, 0:W]
    yf, xf = y.astype(np.float64), x.astype(np.float64)
    rng = np.random.default_rng(5)
    smooth = np.stack([128 + 80 * np.sin(xf / 11.0) * np.cos(yf / 17.0), 110 + 60 * np.cos((xf + yf) / 23.0) + 40 * (xf > 50),
                       90 + 70 * np.sin(yf / 9.0 + xf / 31.0)], axis=2) + rng.normal(0, 3, size=(H, W, 3))
    frames = {"noise": np.random.default_rng(7).integers(64, 128, size=(H, W, 3)).astype(np.uint8),
              "gradient": np.stack([x * 255 // (W - 1), y * 255 // (H - 1), (x + y) * 255 // (H + W - 2)], axis=2).astype(np.uint8),
              "smooth": np.clip(np.round(smooth), 0, 255).astype(np.uint8)}

    def psnr(a, b) -> float:
        return round(float(10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))), 3)
    rows = []
    path = os.path.join(tempfile.gettempdir(), f"mjpeg_bench_pairs_{os.getpid()}.avi")
    for name, frame in frames.items():
        for q in (1, 5, 9):
            writer = mjpeg.DeviceMjpegWriter(path, 10, H, W, 1, quality=q, device=torch.device("cuda:0"))
            writer.append_data(frame)
            writer.close()
            data = open(path, "rb").read()
            at = data.index(b"movi") + 4
            size = int.from_bytes(data[at + 4:at + 8], "little")
            mine = data[at + 8:at + 8 + size]
            buf = io.BytesIO()
            Image.fromarray(frame).save(buf, "JPEG", quality=mjpeg.jpeg_quality(q), subsampling=2, optimize=False)
            with Image.open(io.BytesIO(mine)) as a, Image.open(io.BytesIO(buf.getvalue())) as b:
                rows.append({"frame": name, "quality": q, "jpeg_quality": mjpeg.jpeg_quality(q),
                             "psnr_db": psnr(np.array(a.convert("RGB")), frame), "pil_psnr_db": psnr(np.array(b.convert("RGB")), frame),
                             "bytes": len(mine), "pil_bytes": buf.tell()})
    os.remove(path)
    return rows


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the commit in front of the feature")
    ap.add_argument("--bench-py-pairs", type=int, default=3, help="with --parent-root: pairs of bench.py runs (0: none)")
    ap.add_argument("--leg-timeout", type=int, default=500, help="seconds a leg's process may live")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mjpeg_bench.json"))
    ap.add_argument("--serve", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.serve:
        serve(args)
        return
    out = {"tool": "tools/mjpeg_bench.py", "device": None, "size": args.size, "steps_per_run": args.steps, "rounds": args.rounds,
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
        raise SystemExit("tools/mjpeg_bench.py measures on the GPU: no device found")
    out["device"] = torch.cuda.get_device_name(0)
    out["launches"] = launch_times(args.reps)
    write()
    out["quality_pairs"] = quality_pairs()
    write()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
