"""What --auto-mask-space features costs, how exact its start is, and that the default step is the parent's: one MI355X.

    python tools/feature_mask_bench.py [--reps 30] [--parent-root DIR] [--bench-runs 3] [--out profiles/feature_mask_bench.json]

One JSON document (printed and written to ``--out``):

* the whole stage at 512^2 and 1024^2 for R = 2 and 4 (VGG index 10, synthetic weights, fp32), host clock between two device
  synchronisations, split into extraction (two forward programs to conv3_1, the stack and the schedules built each time; eight
  untimed calls first, so that the tuning of the layer shapes and the stack cache are out of the figure), start (the kept-labels
  launch, the Gram launch and the readback of its slabs per image, the 256x256 ``eigh``) and loop (per iteration two assignment
  launches, one update launch and a 72-byte readback): median and range of ``--reps`` calls after a warm-up;
* one launch of each kernel between device events, with the bytes it moves and GB/s at the median;
* the NumPy twin of the loop (tests/kmeans_feat_ref.py) on the host, for scale: one call;
* the start's error against float64 NumPy on the same features, fp32 and bf16 storage: relative error of ``lam``,
  ``1 - |v . v_ref|`` - the figures tests/test_gpu_feature_mask_model.py takes its bounds from (four times the measured value);
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
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LAYER = 10

EXPECTATION = ("two forward passes to conv3_1; one Gram launch per image with a readback of the CxC slabs; an eigh of 256x256 on the "
               "host; at most 20 iterations of three launch-bound launches and a 72-byte readback: single milliseconds, next to 50 ms "
               "of set-up")


def pictures(size: int):
    """Two seeded pictures ``[1, 3, size, size]`` of blocky regions under noise, on the device (as tools/auto_mask_bench.py)."""
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


def _timed(fn, reps: int, warm: int = 3):
    import torch  # noqa: PLC0415
    for _ in range(warm):
        out = fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e6)
    return out, _summary(times)


def stage_times(reps: int) -> list[dict]:
    from style_transfer_visualizer_amd import segment  # noqa: PLC0415
    from tests import kmeans_feat_ref as ref  # noqa: PLC0415
    rows = []
    oc = types.SimpleNamespace()
    for size in (512, 1024):
        content, style = pictures(size)
        feats, extraction = _timed(lambda: segment.run_features(content, style, LAYER, oc, "fp32"), max(10, reps // 3), warm=8)
        for regions in (2, 4):
            start, start_t = _timed(lambda: segment.feature_start([segment.feature_moments(F) for F in feats], regions), reps)
            (_, _, info), loop_t = _timed(lambda: segment.feature_labels(feats[0], feats[1], regions, centroids=start["centroids"]), reps)
            t0 = time.perf_counter()
            twin = segment.feature_labels(feats[0], feats[1], regions, centroids=start["centroids"], assign=ref.assign_op,
                                          update=ref.update_op)[2]
            twin_us = (time.perf_counter() - t0) * 1e6
            rows.append({"image": [size, size], "layer": LAYER, "grid": list(info["grids"][0]), "channels": int(feats[0].shape[-1]),
                         "regions": regions, "iterations": info["iterations"], "converged": info["converged"],
                         "extraction": extraction, "start": start_t, "loop": loop_t,
                         "numpy_twin_loop": {"us": round(twin_us, 1), "iterations": twin["iterations"]}})
    return rows


def launch_times(reps: int) -> list[dict]:
    import torch  # noqa: PLC0415

    from style_transfer_visualizer_amd import _lib, ops  # noqa: PLC0415
    dev = torch.device("cuda:0")
    rows = []
    for n, C, dtype in ((128 * 128, 256, torch.float32), (256 * 256, 256, torch.float32), (256 * 256, 256, torch.bfloat16),
                        (512 * 512, 64, torch.float32), (64 * 64, 512, torch.float32)):
        F = torch.randn(n, C, device=dev).to(dtype)
        labels = torch.full((n,), 255, dtype=torch.uint8, device=dev)
        for K in (2, 4):
            cen = torch.randn(K, C, device=dev)
            parts = ops.kmeans_feat_assign(F, cen, labels)
            result = torch.empty(9, dtype=torch.float64, device=dev)
            launches = {
                "stv_kmeans_feat_assign": (lambda: ops.kmeans_feat_assign(F, cen, labels, parts),
                                           F.numel() * F.element_size() + 2 * n + parts.numel() * 8 + cen.numel() * 4),
                "stv_kmeans_feat_update": (lambda: ops.kmeans_feat_update(parts, parts, cen, n, n, result),
                                           2 * _lib.KMF_PARTS * (K * (C + 1) + 1) * 8 + 2 * cen.numel() * 4 + 72),
            }
            for name, (fn, moved) in launches.items():
                for _ in range(5):
                    fn()
                torch.cuda.synchronize()
                times = []
                for _ in range(reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    times.append(e0.elapsed_time(e1) * 1000.0)
                med = statistics.median(times)
                rows.append({"launch": name, "pixels": n, "channels": C, "dtype": str(dtype).replace("torch.", ""), "K": K,
                             "bytes_moved": moved, **_summary(times, 2), "GB_per_s_at_median": round(moved / med / 1e3, 1)})
    return rows


def start_errors() -> list[dict]:
    """The device start against float64 NumPy on the same features: the pairs and precisions of the GPU test."""
    from style_transfer_visualizer_amd import segment, synthetic  # noqa: PLC0415
    from tests import feature_mask_inputs as fi  # noqa: PLC0415
    from tests import kmeans_feat_ref as ref  # noqa: PLC0415
    rows = []
    pairs = {"stripes-64": (*fi.stripes_tensors(64, "cuda:0"), 2),
             "synthetic-96x80": (synthetic.synthetic_image(0, 96, 80).to("cuda:0"), synthetic.synthetic_image(1, 80, 96).to("cuda:0"), 3)}
    for name, (content, style, regions) in pairs.items():
        for precision in ("fp32", "bf16"):
            feats = segment.run_features(content, style, LAYER, types.SimpleNamespace(), precision)
            dev = segment.feature_start([segment.feature_moments(F) for F in feats], regions)
            host = segment.feature_start([ref.moments_op(F) for F in feats], regions)
            rows.append({"pair": name, "storage": precision, "lam": host["lam"],
                         "lam_relative_error": abs(dev["lam"] - host["lam"]) / host["lam"],
                         "one_minus_abs_v_dot_v_ref": 1.0 - abs(float(dev["v"] @ host["v"])),
                         "mu_max_error_over_max_mu": float(abs(dev["mu"] - host["mu"]).max() / abs(host["mu"]).max())})
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
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the commit in front of the feature")
    ap.add_argument("--bench-runs", type=int, default=3, help="bench.py runs per tree (0: skip)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_mask_bench.json"))
    args = ap.parse_args()
    os.environ.setdefault("STV_SYNTHETIC_WEIGHTS", "0")
    import torch  # noqa: PLC0415
    if not torch.cuda.is_available():
        raise SystemExit("tools/feature_mask_bench.py measures on the GPU: no device found")
    out = {"tool": "tools/feature_mask_bench.py", "device": None, "reps": args.reps, "expectation_written_before_measuring": EXPECTATION}
    if args.bench_runs > 0:            # first: this process has not touched the device yet
        out["bench_py_steps_200_warmup_100"] = bench_runs(args.parent_root, args.bench_runs)
    out["device"] = torch.cuda.get_device_name(0)
    out["start_against_float64"] = start_errors()
    out["stage_host_clock"], out["launches"] = stage_times(args.reps), launch_times(args.reps)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
