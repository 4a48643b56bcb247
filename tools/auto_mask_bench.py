"""What --auto-mask costs, and that the default step is the parent's: one MI355X.

    python tools/auto_mask_bench.py [--reps 50] [--parent-root DIR] [--bench-runs 3] [--out profiles/auto_mask_bench.json]

Four measurements, one JSON document (printed and written to ``--out``):

* the whole stage, ``segment.auto_labels`` (two pooling launches, two statistics launches and their copies, the 3x3 algebra,
  then per iteration one upload of the centroids, two assignment launches and one readback), host clock between two device
  synchronisations: median and range of ``--reps`` calls after a warm-up at 512^2 and 1024^2 for R = 2 and 4, cells of 8;
* one ``stv_kmeans_assign`` launch with device events round the call: median and range of ``--reps`` launches after a warm-up at
  64^2 and 128^2 (the pooled sizes of the two above) and at 1024^2 (cells of 1), for K = 2 and 4, with the bytes it moves;
* the NumPy twin of the same stage (tests/kmeans_ref.py) on the host, for scale: median of 3 calls;
* ``bench.py --gpus 1 --steps 200 --warmup 100`` of this tree and, with ``--parent-root DIR`` (a built checkout of the commit in
  front of the feature), of that one, in alternating fresh processes, ``--bench-runs`` each.  No threshold: the figures are
  this tree's median, the parent's, and the parent's own spread between its runs.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pictures(size: int):
    """Two seeded pictures ``[1, 3, size, size]`` with smooth regions and differently tinted channels, on the device."""
    import numpy as np  # noqa: PLC0415
    import torch  # noqa: PLC0415
    out = []
    for seed, tint in ((0, (0.9, 0.6, 0.4)), (1, (0.3, 0.5, 0.95))):
        rng = np.random.default_rng(seed)
        coarse = np.kron(rng.random((size // 64, size // 64, 1)), np.ones((64, 64, 1)))
        rgb = np.clip((0.7 * coarse + 0.3 * rng.random((size, size, 3))) * np.asarray(tint), 0, 1).astype(np.float32)
        out.append(torch.from_numpy(rgb).permute(2, 0, 1)[None].contiguous().to("cuda:0"))
    return out


def _summary(values: list[float], digits: int = 1) -> dict:
    return {"median_us": round(statistics.median(values), digits), "min_us": round(min(values), digits), "max_us": round(max(values), digits)}


def stage_times(reps: int) -> list[dict]:
    import torch  # noqa: PLC0415

    from style_transfer_visualizer_amd import segment  # noqa: PLC0415
    from tests import kmeans_ref as ref  # noqa: PLC0415
    rows = []
    for size in (512, 1024):
        content, style = pictures(size)
        for regions in (2, 4):
            for _ in range(5):
                info = segment.auto_labels(content, style, regions, cell=8)[2]
            times = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                segment.auto_labels(content, style, regions, cell=8)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e6)
            host, host_in = [], (content.cpu(), style.cpu())
            for _ in range(3):
                t0 = time.perf_counter()
                twin = segment.auto_labels(*host_in, regions, cell=8, **ref.HOST)[2]
                host.append((time.perf_counter() - t0) * 1e6)
            rows.append({"image": [size, size], "regions": regions, "cell": 8, "iterations": info["iterations"],
                         "converged": info["converged"], "device_stage": _summary(times),
                         "numpy_twin_stage": {**_summary(host), "iterations": twin["iterations"]}})
    return rows


def launch_times(reps: int) -> list[dict]:
    import torch  # noqa: PLC0415

    from style_transfer_visualizer_amd import ops  # noqa: PLC0415
    dev = torch.device("cuda:0")
    rows = []
    for size in (64, 128, 1024):
        x = torch.rand(3, size, size, device=dev)
        labels = torch.full((size, size), 255, dtype=torch.uint8, device=dev)
        parts = ops.kmeans_assign(x, torch.rand(2, 3, device=dev), labels)
        moved = x.numel() * 4 + 2 * labels.numel() + parts.numel() * 8
        for K in (2, 4):
            cen = torch.rand(K, 3, device=dev)
            for _ in range(5):
                ops.kmeans_assign(x, cen, labels, parts)
            torch.cuda.synchronize()
            times = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ops.kmeans_assign(x, cen, labels, parts)
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1) * 1000.0)
            med = statistics.median(times)
            rows.append({"launch": "stv_kmeans_assign", "image": [size, size], "K": K, "bytes_moved": moved, **_summary(times, 2),
                         "GB_per_s_at_median": round(moved / med / 1e3, 1)})
    return rows


def bench_runs(parent_root: str | None, runs: int) -> dict:
    """``bench.py`` of the two trees in alternating fresh processes; steps/s of every run."""
    trees = {"this tree": ROOT}
    if parent_root:
        trees["parent"] = os.path.abspath(parent_root)
    values: dict[str, list[float]] = {name: [] for name in trees}
    for _ in range(runs):
        for name, root in trees.items():
            done = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "200", "--warmup", "100"], cwd=root,
                                  capture_output=True, text=True, check=True, timeout=600)
            line = json.loads(done.stdout.strip().splitlines()[-1])
            values[name].append(float(line["value"]))
            print(f"bench.py of {name}: {line['value']} steps/s", file=sys.stderr, flush=True)
    out = {name: {"steps_per_s": vals, "median": statistics.median(vals), "range": [min(vals), max(vals)]} for name, vals in values.items()}
    if parent_root:
        out["this_tree_minus_parent_median"] = round(out["this tree"]["median"] - out["parent"]["median"], 3)
        out["parent_own_spread"] = round(out["parent"]["range"][1] - out["parent"]["range"][0], 3)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the commit in front of the feature")
    ap.add_argument("--bench-runs", type=int, default=3, help="bench.py runs per tree (0: skip)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "auto_mask_bench.json"))
    args = ap.parse_args()
    import torch  # noqa: PLC0415
    if not torch.cuda.is_available():
        raise SystemExit("tools/auto_mask_bench.py measures on the GPU: no device found")
    out = {"tool": "tools/auto_mask_bench.py", "device": None, "reps": args.reps,
           "expectation_written_before_measuring": "an iteration is two launches of about 10 us, one 70 KB readback and a few us of 3x3 "
                                                   "algebra; 2 to 20 iterations: of the order of a millisecond per run, next to 50 ms of set-up"}
    if args.bench_runs > 0:            # first: this process has not touched the device yet
        out["bench_py_steps_200_warmup_100"] = bench_runs(args.parent_root, args.bench_runs)
    out["device"] = torch.cuda.get_device_name(0)
    out["stage_host_clock"], out["launches"] = stage_times(args.reps), launch_times(args.reps)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
