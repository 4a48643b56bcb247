"""What average pooling (--pooling avg) costs per L-BFGS step: one MI355X, bf16, synthetic VGG19 up to conv5_1 (the runner's
default taps), a full history (100 pairs, filled by untimed steps first, as bench.py does).

    python tools/avgpool_bench.py [--sizes 512 1024] [--rounds 6] [--steps 200] [--passes N] [--parent-root DIR]
                                  [--bench-py-pairs 3] [--out profiles/avgpool_bench.json]

Four legs per size, each in a PROCESS OF ITS OWN that stays alive for the whole measurement (``--serve``, driven over a pipe, started
under ``timeout``): a step's time depends a little on what else its process has allocated, so no leg shares one.

  1. ``parent``        the step of the checkout given with ``--parent-root`` (the commit in front of the feature), package
                       imported from there;
  2. ``max``           this tree, ``pooling="max"``: must sit inside the parent's round-to-round spread;
  3. ``max unfused``   this tree, ``pooling="max"`` under ``STV_FUSE_POOL=0 STV_FUSE_POOL_BWD=0``: the max pools as stand-alone ops
                       - the schedule shape of ``avg``, with max kernels.  (3) - (2) is what fusing pools into the conv launches
                       is worth, i.e. what a fused average-pooling epilogue could at most win back;
  4. ``avg``           this tree, ``pooling="avg"``.

After one untimed round the legs alternate inside every round, the order reversed from round to round, so that clock drift and
other people's work on the host fall on all of them.  Every round's ms/step is kept, with median, minimum and maximum.
The whole measurement is a PASS, and there is one pass per leg, each with fresh processes started in the leg order rotated by
one: of the processes alive side by side the one started first runs faster than the others at 1024^2 (by 40-80 us per step,
whichever leg it is), so every leg takes that place once, and a leg is compared on the passes in which it did not have it
(``results``: the median over those passes, and every difference also pass by pass where neither side was first).
Every optimiser runs with ``tolerance_grad = tolerance_change = 0`` and every leg reports how far one more step moves the image:
an L-BFGS that has met a tolerance skips its update, and a round of such steps times the closure alone.

Then the pooling launches alone: the processes of legs 3 and 4 time every op of their step's program with device events
(``Program.profile``, each op 20 times back to back inside its event pair) and report the eight pooling ops with the bytes
each moves at least and the GB/s that makes.

With ``--parent-root`` the tool ends with ``bench.py --gpus 1 --steps 200 --warmup 100`` of the two trees in alternating fresh
processes (``bench_py_pairs``).

The expectation is written into the JSON document before anything is measured.  One document (printed, and written to ``--out``);
keys of an existing ``--out`` that this tool does not write are kept.
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
LEGS = {      # name -> (needs --parent-root, pooling keyword or None, environment of its process)
    "parent": (True, None, {}),
    "max": (False, "max", {}),
    "max unfused": (False, "max", {"STV_FUSE_POOL": "0", "STV_FUSE_POOL_BWD": "0"}),
    "avg": (False, "avg", {}),
}
POOL_OPS = {4: "POOL_FWD", 5: "POOL_BWD", 20: "AVGPOOL_FWD", 21: "AVGPOOL_BWD"}      # stv.h STV_OP_*
MASK, ACCUM = 4, 8

EXPECTATION = {
    "written": "before any measurement",
    "avg_minus_max": "about what (max unfused) - (max) costs: the same schedule shape, kernels that move the same bytes",
    "at_1024": "dominated by storing and re-reading the four pre-pool maps, which the fused max-pooling step never stores in bf16: "
               "conv1_2 134 MB, conv2_2 67 MB, conv3_4 34 MB, conv4_4 17 MB, 252 MB per closure",
    "max_vs_parent": "inside the parent's own round-to-round spread: with pooling='max' nothing changes - same op list, same "
                     "program key, same object code in every file but program.o",
    "fusion_case": "(max unfused) - (max) bounds what average pooling in the conv epilogues could win back",
}


class StepLeg:
    """One tree's fused L-BFGS step at one size: a model, an image and an optimiser, prefilled."""

    def __init__(self, root: str, precision: str, pooling: str | None) -> None:
        sys.path.insert(0, root)
        import torch  # noqa: PLC0415
        from style_transfer_visualizer_amd import core_model, synthetic  # noqa: PLC0415
        from style_transfer_visualizer_amd.optimizers import HipLBFGS  # noqa: PLC0415
        self.torch, self.core_model, self.synthetic, self.lbfgs = torch, core_model, synthetic, HipLBFGS
        self.precision, self.pooling = precision, pooling
        self.dev = torch.device("cuda:0")
        self.side = torch.cuda.Stream(device=self.dev)        # (the legacy default stream cannot be captured)
        self.state: dict = {}

    def setup(self, size: int) -> None:
        torch, core_model, synthetic = self.torch, self.core_model, self.synthetic
        weights = synthetic.synthetic_conv_weights(3)
        saved = core_model.initialize_vgg
        core_model.initialize_vgg = lambda: core_model.build_vgg_features(weights).eval()
        try:          # (the tree in front of the feature has no such keyword)
            kw = {"pooling": self.pooling} if self.pooling is not None else {}
            model = core_model.StyleContentModel(S, C, precision=self.precision, **kw).to(self.dev)
        finally:
            core_model.initialize_vgg = saved
        model.set_targets(synthetic.synthetic_image(1, size, size).to(self.dev), synthetic.synthetic_image(0, size, size).to(self.dev))
        self.side.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(self.side):
            xi = torch.randn(1, 3, size, size, generator=torch.Generator().manual_seed(0)).to(self.dev).requires_grad_(True)
            # tolerances 0 in every leg: with average pooling the gradient of this synthetic stack falls below torch's default
            # tolerance_grad (1e-7) after about 150 steps, the step's update then becomes a no-op (torch's early return) and a
            # "step" is the closure alone - 0.2 ms less at 512^2, 0.6 ms at 1024^2.  The cost of a step is wanted, not that exit.
            opt = self.lbfgs([xi], lr=1.0, history_size=100, tolerance_grad=0.0, tolerance_change=0.0)
            closure = lambda: model.loss_and_grad(xi, 1e5, 1.0)[2]      # noqa: E731
            for _ in range(100):                              # fill the history (and capture the step's graph): untimed
                opt.step(closure)
            self.side.synchronize()
        self.state[size] = (model, xi, opt, closure)

    def run(self, size: int, steps: int) -> float:
        """ms per step over ``steps`` steps, device events round them."""
        torch = self.torch
        _, _, opt, closure = self.state[size]
        with torch.cuda.stream(self.side):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                opt.step(closure)
            e1.record()
            self.side.synchronize()
        return e0.elapsed_time(e1) / steps

    def moved(self, size: int) -> float:
        """max |change of the image| over one more step: 0 means the optimiser has stopped and the rounds timed no update."""
        torch = self.torch
        _, xi, opt, closure = self.state[size]
        with torch.cuda.stream(self.side):
            before = xi.detach().clone()
            opt.step(closure)
            delta = float((xi.detach() - before).abs().max())
        return delta

    def launches(self, size: int, reps: int = 20) -> list[dict]:
        """The pooling ops of the step's program, timed alone (leaves the program's buffers meaningless: the last thing asked)."""
        torch = self.torch
        model = self.state[size][0]
        (eng,) = model._engines.values()
        prog = max((p for k, p in eng._programs.items() if k[0] == "fused"), key=lambda p: p.n_ops)
        with torch.cuda.stream(self.side):
            prog.profile(reps)                                # once untimed: caches and clocks as in a run
            ms = prog.profile(reps)
        es = 2 if self.precision == "bf16" else 4
        out = []
        for (op, H, W, cin, *_), flags, t in zip(prog.op_meta, prog.op_flags, ms, strict=True):
            if op not in POOL_OPS:
                continue
            full, pooled = H * W * cin * es, (H // 2) * (W // 2) * cin * es
            if op in (4, 20):
                moved = full + pooled                         # the map read, the pooled map written
            else:                                             # dy read, dx written; the mask's map (max: always its input) and an
                reads_ref = op == 5 or bool(flags & MASK)     # accumulated-onto dx read
                moved = pooled + full + (full if reads_ref else 0) + (full if flags & ACCUM else 0)
            out.append({"op": POOL_OPS[op], "H": H, "W": W, "C": cin, "flags": flags, "us": round(t * 1000.0, 2),
                        "bytes_at_least": moved, "GB_per_s": round(moved / (t * 1e-3) / 1e9, 1) if t > 0 else None})
        return out

    def drop(self, size: int) -> None:
        self.state.pop(size, None)
        self.torch.cuda.empty_cache()


def serve(args) -> None:
    """``setup <size>`` / ``run <size> <steps>`` / ``moved <size>`` / ``launches <size>`` / ``drop <size>`` lines on stdin -> one answer line each."""
    leg = StepLeg(args.root, args.precision, args.pooling)
    real_stdout = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)                                             # keep the pipe for the answers
    real_stdout.write("ready\n")
    real_stdout.flush()
    for line in sys.stdin:
        words = line.split()
        if not words:
            continue
        if words[0] == "setup":
            leg.setup(int(words[1]))
            answer = "ok"
        elif words[0] == "run":
            answer = f"{leg.run(int(words[1]), int(words[2])):.6f}"
        elif words[0] == "moved":
            answer = f"{leg.moved(int(words[1])):.6e}"
        elif words[0] == "launches":
            answer = json.dumps(leg.launches(int(words[1])))
        else:
            leg.drop(int(words[1]))
            answer = "ok"
        real_stdout.write(answer + "\n")
        real_stdout.flush()


class LegProcess:
    """One leg in a process of its own, under a time limit of its own."""

    def __init__(self, root: str, precision: str, pooling: str | None, env: dict, limit_s: int) -> None:
        cmd = ["timeout", "-k", "10", str(limit_s), sys.executable, os.path.abspath(__file__), "--serve", "--root", root,
               "--precision", precision] + (["--pooling", pooling] if pooling is not None else [])
        self.proc = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=root, env={**os.environ, **env})
        if self.proc.stdout.readline().strip() != "ready":
            raise SystemExit(f"the process for {root} ({pooling}, {env}) did not start")

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
            "min_ms_per_step": round(min(step_ms), 4), "max_ms_per_step": round(max(step_ms), 4),
            "spread_us": round((max(step_ms) - min(step_ms)) * 1000.0, 2),
            "median_steps_per_s": round(1000.0 / statistics.median(step_ms), 2)}


def measure_pass(args, order: list[str]) -> tuple[dict, dict]:
    """One pass: the legs' processes started in ``order``, all sizes measured, the processes closed.  Returns per size the
    legs' round summaries and the pooling launches alone."""
    procs: dict[str, LegProcess] = {}
    results, launches = {}, {}
    try:
        for name in order:
            needs_parent, pooling, env = LEGS[name]
            root = os.path.abspath(args.parent_root) if needs_parent else ROOT
            procs[name] = LegProcess(root, args.precision, pooling, env, args.leg_timeout)
        for size in args.sizes:
            for name in order:
                procs[name].ask(f"setup {size}")
            for name in order:                                # one untimed round
                procs[name].ask(f"run {size} {args.steps}")
            times: dict[str, list[float]] = {name: [] for name in order}
            for r in range(args.rounds):
                for name in (order if r % 2 == 0 else order[::-1]):
                    times[name].append(float(procs[name].ask(f"run {size} {args.steps}")))
            res = {name: summary(v) for name, v in times.items()}
            for name in order:          # a leg whose optimiser stopped timed closures without updates: it must show
                res[name]["image_moved_in_one_more_step"] = float(procs[name].ask(f"moved {size}"))
            results[str(size)] = res
            launches[str(size)] = {name: json.loads(procs[name].ask(f"launches {size}")) for name in ("max unfused", "avg")}
            for name in order:
                procs[name].ask(f"drop {size}")
    finally:
        for proc in procs.values():
            proc.close()
    return results, launches


def combine(passes: list[dict], legs: list[str], sizes: list[int]) -> dict:
    """Per size and leg the medians of all passes, and the comparison on the passes in which the leg's process was NOT the
    first one started: the first-started process of a pass runs faster than the others, whichever leg it is."""
    out = {}
    for size in map(str, sizes):
        res = {}
        for leg in legs:
            by_pass = [p["results"][size][leg]["median_ms_per_step"] for p in passes]
            later = [v for p, v in zip(passes, by_pass, strict=True) if p["leg_order"][0] != leg]
            first = [v for p, v in zip(passes, by_pass, strict=True) if p["leg_order"][0] == leg]
            use = later or by_pass
            res[leg] = {"median_ms_per_step_by_pass": by_pass, "when_started_first_ms_per_step": first,
                        "median_ms_per_step": round(statistics.median(use), 4), "min_ms_per_step": round(min(use), 4),
                        "max_ms_per_step": round(max(use), 4), "spread_over_passes_us": round((max(use) - min(use)) * 1000.0, 2),
                        "median_steps_per_s": round(1000.0 / statistics.median(use), 2),
                        "largest_spread_of_the_rounds_of_one_pass_us": max(p["results"][size][leg]["spread_us"] for p in passes)}
        med = {leg: res[leg]["median_ms_per_step"] for leg in legs}

        def diffs(a: str, b: str) -> dict:
            """a - b in microseconds: of the medians, and pass by pass where neither was started first."""
            each = [round((p["results"][size][a]["median_ms_per_step"] - p["results"][size][b]["median_ms_per_step"]) * 1000.0, 2)
                    for p in passes if p["leg_order"][0] not in (a, b)]
            return {"of_medians_us": round((med[a] - med[b]) * 1000.0, 2), "percent": round(100.0 * (med[a] - med[b]) / med[b], 3),
                    "per_pass_neither_first_us": each}
        res["avg_minus_max"] = diffs("avg", "max")
        res["max_unfused_minus_max"] = diffs("max unfused", "max")
        res["avg_minus_max_unfused"] = diffs("avg", "max unfused")
        if "parent" in med:
            res["max_minus_parent"] = diffs("max", "parent")
        out[size] = res
    return out


def bench_py_pairs(args, pairs: int) -> dict:
    """``bench.py --gpus 1 --steps 200 --warmup 100`` of the parent tree and of this tree in alternating fresh processes, the
    parent first, each under a time limit; steps/s of every run."""
    cmd = ["timeout", "-k", "10", "240", sys.executable, "bench.py", "--gpus", "1", "--steps", "200", "--warmup", "100"]
    got: dict[str, list[float]] = {"parent_steps_per_s": [], "this_tree_steps_per_s": []}
    for _ in range(pairs):
        for key, root in (("parent_steps_per_s", os.path.abspath(args.parent_root)), ("this_tree_steps_per_s", ROOT)):
            done = subprocess.run(cmd, cwd=root, capture_output=True, text=True, check=False)
            if done.returncode != 0:          # nothing more is started behind a failed run
                raise SystemExit(f"bench.py in {root} ended with status {done.returncode}: {done.stderr[-400:]}")
            got[key].append(float(json.loads(done.stdout.strip().splitlines()[-1])["value"]))
    return {"command": "bench.py --gpus 1 --steps 200 --warmup 100", "order": "alternating fresh processes on one box, the parent first", **got}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=200, help="timed L-BFGS steps per leg and round (after a 100-step prefill)")
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the commit in front of the feature")
    ap.add_argument("--passes", type=int, default=None,
                    help="passes, each with fresh processes started in the leg order rotated by one (default: one per leg, so "
                         "that every leg is the first-started process once)")
    ap.add_argument("--bench-py-pairs", type=int, default=3, help="with --parent-root: pairs of bench.py runs (0: none)")
    ap.add_argument("--leg-timeout", type=int, default=600, help="time limit of every leg's process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "avgpool_bench.json"))
    ap.add_argument("--serve", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--pooling", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.serve:
        serve(args)
        return
    import torch  # noqa: PLC0415
    if not torch.cuda.is_available():
        raise SystemExit("tools/avgpool_bench.py measures on the GPU: no device found")
    legs = [name for name, (needs_parent, _, _) in LEGS.items() if args.parent_root or not needs_parent]
    n_passes = len(legs) if args.passes is None else max(1, args.passes)
    out = {"tool": "tools/avgpool_bench.py", "device": torch.cuda.get_device_name(0), "precision": args.precision, "history": 100,
           "steps_per_round": args.steps, "rounds": args.rounds, "untimed_rounds": 1, "parent": bool(args.parent_root),
           "expectation": EXPECTATION, "results": {}, "passes": [], "pool_launches": {}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    kept = {}
    if os.path.exists(args.out):          # keys this tool does not write (figures merged in from elsewhere) survive a re-run
        try:
            with open(args.out) as fh:
                kept = {k: v for k, v in json.load(fh).items() if k not in out and k != "bench_py_pairs"}
        except (OSError, ValueError):
            kept = {}
    out.update(kept)

    def write() -> None:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    write()                                # the expectation stands before anything is measured
    for k in range(n_passes):
        order = legs[k % len(legs):] + legs[:k % len(legs)]
        results, launches = measure_pass(args, order)
        out["passes"].append({"leg_order": order, "results": results})
        if k == 0:
            out["pool_launches"] = launches
        out["results"] = combine(out["passes"], legs, args.sizes)
        write()
    if args.parent_root and args.bench_py_pairs > 0:
        out["bench_py_pairs"] = bench_py_pairs(args, args.bench_py_pairs)
    print(json.dumps(out))
    write()


if __name__ == "__main__":
    main()
