"""Row strips against the whole image at the layouts tests/test_gpu_spatial.py does not reach (tests/spatial_cases.py):
content taps at two resolutions, strips of unequal height down to ONE own row at the deepest level, an image height
that is no multiple of 16 with an odd width, bf16 storage, and recomputed halos clipped at the image border.

As in tests/test_gpu_spatial.py the ranks are gloo processes that share cuda:0, the network is MINI, images and
weights are synthetic.  The reference is the unsharded HIP model at the same image, evaluated in this process.  One
process group per WORLD SIZE walks all cases of that size (process start-up dominates the cost); never more than four
ranks beside this process.

The weights are ``style_w = 1e2, content_w = 1``: at the 1e5 of the older tests a content tap's gradient is 5e-5 to
5e-4 of the total's maximum, and a 20 % error of one tap hides below the 2e-5 gate.  Every case asserts that each
content tap ALONE carries at least 1 % of the whole gradient's maximum, so the gate sees every tap.
"""
from __future__ import annotations

import functools
import os
import queue
import socket
import time
import traceback

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.conftest import record_parity
from tests.spatial_cases import CASES, CONTENT_W, MINI, S_AT, STYLE_W, Case, cases_of

pytestmark = pytest.mark.gpu

OPTIMIZERS = (("adam", 1e-2), ("lbfgs", 1.0))
DEADLINE = 300.0      # seconds for one world's ranks to answer (they take a few); a rank that dies is noticed at once


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _setup(case: Case, precision: str, content_at=None):
    from style_transfer_visualizer_amd import core_model, synthetic
    dev = torch.device("cuda:0")
    weights = synthetic.synthetic_conv_weights(3, MINI)
    content = synthetic.synthetic_image(0, case.H, case.W).to(dev)
    style = synthetic.synthetic_image(1, 96, 128).to(dev)
    x0 = synthetic.synthetic_image(2, case.H, case.W).to(dev)
    saved = core_model.initialize_vgg                 # (also runs in spawned workers, where no monkeypatch fixture exists)
    core_model.initialize_vgg = lambda: core_model.build_vgg_features(weights, MINI).eval()
    try:
        model = core_model.StyleContentModel(S_AT, list(content_at or case.content_at), precision=precision).to(dev)
    finally:
        core_model.initialize_vgg = saved
    model.set_targets(style, content)
    return model, content, x0, dev


# ------------------------------------------------------------------------------------------------ the ranks
def _run_case(case: Case) -> dict:
    from style_transfer_visualizer_amd import spatial
    model, content, x0, dev = _setup(case, case.precision)
    dtype = torch.bfloat16 if case.precision == "bf16" else torch.float32
    args = (model._layers(), S_AT, list(case.content_at), content, model.style_targets)
    kw = dict(dtype=dtype, style_w=STYLE_W, content_w=CONTENT_W)
    out = {}
    if case.shard == "recompute":
        shard = spatial.SpatialShard(*args, **kw)
        out["rows"], out["ext"] = (shard.c0, shard.c1), (shard.e0, shard.e1)
        out["scores"] = shard.loss_and_grad(x0).cpu().numpy()
        out["grad"] = shard.g_core.cpu().numpy()
        if not case.steps:
            return out
        x = x0.clone()
        for _ in range(3):
            x = shard.adam_step(x, lr=1e-2)
        out["adam_image"] = x.cpu().numpy()
        return out
    shard = spatial.HaloShard(*args, **kw)
    shard.set_image(x0)
    out["rows"], out["exchanges"] = (shard.c0, shard.c1), shard.exchanges_per_closure
    out["scores"] = shard.loss_and_grad().cpu().numpy()
    out["grad"] = shard.g_core.cpu().numpy()
    for name, lr in OPTIMIZERS if case.precision == "fp32" and case.steps else ():
        shard = spatial.HaloShard(*args, **kw)
        shard.set_image(x0)
        out[f"{name}_totals"] = [float(shard.step(name, lr=lr)[2]) for _ in range(3)]
        out[f"{name}_image"] = shard.gather_image().cpu().numpy()
        if name == "lbfgs":
            out["lbfgs_state"] = shard._opt.device_state()
    return out


def _worker(rank: int, world: int, port: int, q) -> None:
    """Every case of this world size inside one process group.  Whatever goes wrong reaches the queue as text: the
    parent then stops the other ranks, which may be waiting for this one in a collective."""
    try:
        os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        out = {}
        for case in cases_of(world):
            out[case.name] = _run_case(case)
        torch.cuda.synchronize()
        # numpy (pickled by value): torch tensors in an mp.Queue need the sender alive on receipt
        q.put((rank, "ok", out))
        dist.barrier()
        dist.destroy_process_group()
    except BaseException:      # noqa: BLE001 - reported, not handled
        q.put((rank, "error", traceback.format_exc()))


def _stop(procs) -> None:
    for p in procs:
        if p.is_alive():
            p.terminate()
    for p in procs:
        p.join(timeout=10)
        if p.is_alive():
            p.kill()
            p.join()


def _run_world(world: int) -> dict:
    assert world <= 4
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    got, t0 = {}, time.time()
    try:
        for p in procs:
            p.start()
        while len(got) < world:
            try:
                rank, kind, payload = q.get(timeout=0.5)
            except queue.Empty:
                gone = [(r, p.exitcode) for r, p in enumerate(procs) if p.exitcode not in (None, 0) and r not in got]
                if gone and q.empty():
                    raise RuntimeError(f"world {world}: ranks ended without an answer (rank, exit code): {gone}") from None
                if time.time() - t0 > DEADLINE:
                    raise RuntimeError(f"world {world}: no answer from ranks {sorted(set(range(world)) - set(got))} "
                                       f"within {DEADLINE:.0f} s") from None
                continue
            if kind == "error":
                raise RuntimeError(f"world {world}, rank {rank}:\n{payload}")
            got[rank] = payload
        for p in procs:
            p.join(timeout=60)
        codes = [p.exitcode for p in procs]
        if codes != [0] * world:
            raise RuntimeError(f"world {world}: exit codes {codes}")
    finally:
        _stop(procs)          # no rank is left waiting in a collective with the GPU open
    return got


_WORLDS: dict = {}


def _world_results(world: int) -> dict:
    """The ranks of one world size run once; every case of that size reads their answer (or their failure)."""
    if world not in _WORLDS:
        try:
            _WORLDS[world] = _run_world(world)
        except RuntimeError as exc:
            _WORLDS[world] = exc
    if isinstance(_WORLDS[world], Exception):
        pytest.fail(str(_WORLDS[world]), pytrace=False)
    return _WORLDS[world]


# ------------------------------------------------------------------------------------------------ the whole image
@functools.cache
def _reference(H: int, W: int, content_at: tuple, shard: str, steps: bool) -> dict:
    """The unsharded fp32 HIP model at the case's image: scores, gradient, every content tap's own gradient maximum, and
    three steps of each optimizer the case runs.  Computed once per image; nothing in it is modified afterwards."""
    from style_transfer_visualizer_amd import optimizers
    case = Case("reference", shard, 1, H, W, (), content_at)
    model, content, x0, dev = _setup(case, "fp32")
    x = x0.clone().requires_grad_(True)
    scores = torch.stack(model.loss_and_grad(x, STYLE_W, CONTENT_W)).cpu()
    ref = {"scores": scores, "grad": x.grad.clone().cpu(), "tap_max": {}}
    for layer in content_at:          # d(content_w * this tap's loss)/dx alone: the style weight is zero
        tap_model = _setup(case, "fp32", content_at=[layer])[0]
        xt = x0.clone().requires_grad_(True)
        tap_model.loss_and_grad(xt, 0.0, CONTENT_W)
        ref["tap_max"][layer] = float(xt.grad.abs().max())
    makers = {"adam": lambda p: optimizers.HipAdam([p], lr=1e-2), "lbfgs": lambda p: optimizers.HipLBFGS([p], lr=1.0)}
    for name in () if not steps else ("adam",) if shard == "recompute" else ("adam", "lbfgs"):
        xa = x0.clone().requires_grad_(True)
        opt = makers[name](xa)
        totals = [float(opt.step(lambda: model.loss_and_grad(xa, STYLE_W, CONTENT_W)[2])) for _ in range(3)]
        ref[name] = (xa.detach().cpu(), totals)
        if name == "lbfgs":
            ref["lbfgs_state"] = opt.device_state()
    return ref


@functools.cache
def _bf16_gradient(case: Case) -> torch.Tensor:
    model, content, x0, dev = _setup(case, "bf16")
    x = x0.clone().requires_grad_(True)
    model.loss_and_grad(x, STYLE_W, CONTENT_W)
    return x.grad.clone().cpu()


# ------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_strips_equal_the_whole_image(case):
    """Per rank: scores against the whole image (rtol 2e-5), own-rows gradient within 2e-5 of the whole gradient's
    maximum, the strip bounds of the case table, 26 halo exchanges per closure; fp32 halo cases: three Adam and three
    L-BFGS steps against the unsharded optimizers (per-step totals 1e-5, the third L-BFGS total 2e-3 - its update is built
    from differences of fp32 inner products summed in another order; image 2e-4 / 2e-3 of range), gathered image and
    L-BFGS integer state bit-identical on all ranks; ``recompute``: three Adam steps, image within 1e-4.

    ``mixed-bf16``: losses against the fp32 whole image at 2e-3 (the bound of bf16 storage in tests/test_gpu_configs.py),
    own-rows gradient against the bf16 whole-image gradient at the 0.25 rms sanity bound of tests/test_gpu_fullsize.py -
    bf16 storage makes the network chaotic under rounding and no tighter bound is known for strips; the measured value is
    in the parity table (6.5e-3; with the taps' shares swapped it was 0.19: this bound does NOT see that defect, the
    fp32 ``mixed`` case at the same layout does - 0.17 of scale against 4.7e-7)."""
    got = {r: per_rank[case.name] for r, per_rank in _world_results(case.world).items()}
    ref = _reference(case.H, case.W, case.content_at, case.shard, case.steps)
    label = f"strips {case.name} {case.H}x{case.W} x{case.world}"
    g_ref, ref_scores = ref["grad"], ref["scores"]
    gscale = float(g_ref.abs().max())
    for layer, tap_max in ref["tap_max"].items():       # otherwise the gradient gate cannot see that tap at all
        print(f"{label}: content tap {layer} alone: max {tap_max:.3e} = {tap_max / gscale:.3f} of the whole gradient's {gscale:.3e}")
        assert tap_max >= 0.01 * gscale, f"content tap {layer}: {tap_max:.3e} of {gscale:.3e}"
    assert tuple(got[r]["rows"] for r in range(case.world)) == case.strips
    if case.shard == "recompute":
        assert tuple(got[r]["ext"] for r in range(case.world)) == case.extended
    else:
        assert all(got[r]["exchanges"] == 26 for r in range(case.world))      # 13 convs forward + 13 backward
    bf16 = case.precision == "bf16"
    worst_s = worst_g = 0.0
    failures = []
    for r in range(case.world):
        c0, c1 = got[r]["rows"]
        scores = torch.from_numpy(got[r]["scores"])
        dev_s = float(((scores - ref_scores).abs() / ref_scores.abs()).max())
        g = torch.from_numpy(got[r]["grad"])
        if bf16:
            g_b = _bf16_gradient(case)[:, :, c0:c1]
            dev_g = float((g - g_b).norm() / g_b.norm())
        else:
            dev_g = float((g - g_ref[:, :, c0:c1]).abs().max()) / gscale
        print(f"{label} rank {r}: scores {dev_s:.3e} (rel), own-rows gradient {dev_g:.3e}")
        worst_s, worst_g = max(worst_s, dev_s), max(worst_g, dev_g)
        s_tol, g_tol = (2e-3, 0.25) if bf16 else (2e-5, 2e-5)
        if not dev_s <= s_tol:
            failures.append(f"rank {r}: scores {scores} vs {ref_scores}: {dev_s:.3e} > {s_tol:g}")
        if not dev_g <= g_tol:
            failures.append(f"rank {r}: own-rows gradient differs from the whole image's by {dev_g:.3e} > {g_tol:g}")
    if bf16:
        record_parity(label, "bf16 strips vs the fp32 whole image, scores (rel)", worst_s, 2e-3, "bf16 storage against fp32")
        record_parity(label, "own-rows gradient, bf16 strips vs bf16 whole image (rms of rms)", worst_g, 0.25,
                      "sanity bound only: rounding chaos, see test_gpu_bf16_layerwise.py")
    else:
        record_parity(label, "strips vs the whole image, scores (rel)", worst_s, 2e-5)
        record_parity(label, "own-rows gradient of every strip vs the whole image (of scale)", worst_g, 2e-5,
                      "; ".join(f"tap {k} alone {v / gscale:.3f} of scale" for k, v in ref["tap_max"].items()))
    assert not failures, "\n".join(failures)
    if bf16 or not case.steps:
        return

    if case.shard == "recompute":
        x_ref, _ = ref["adam"]
        for r in range(case.world):
            x_fin = torch.from_numpy(got[r]["adam_image"])
            assert float((x_fin - x_ref).abs().max()) < 1e-4, f"rank {r}: image after 3 Adam steps differs"  # lr 1e-2 x normalised update
        return

    for name, _ in OPTIMIZERS:
        x_ref, totals = ref[name]
        for r in range(case.world):
            step_totals = got[r][f"{name}_totals"]
            np.testing.assert_allclose(step_totals[:2], totals[:2], rtol=1e-5)
            np.testing.assert_allclose(step_totals[2:], totals[2:], rtol=1e-5 if name == "adam" else 2e-3)
            x_fin = torch.from_numpy(got[r][f"{name}_image"])
            dev_img = float((x_fin - x_ref).abs().max() / x_ref.abs().max())
            bound = 2e-4 if name == "adam" else 2e-3
            print(f"{label} rank {r} {name}: image after 3 steps {dev_img:.3e} of range")
            assert dev_img < bound, f"rank {r} {name}: image after 3 steps differs by {dev_img:.2e} of its range"
            # every rank holds the same gathered image
            assert np.array_equal(got[0][f"{name}_image"], got[r][f"{name}_image"])
    # ... and ran the SAME scalar recursion: after the all-reduce the inner products are bit-identical on every rank
    for r in range(1, case.world):
        assert got[0]["lbfgs_state"] == got[r]["lbfgs_state"]
    st, want = got[0]["lbfgs_state"], ref["lbfgs_state"]
    assert (st["n_iter"], st["hist_len"], st["skip"]) == (want["n_iter"], want["hist_len"], want["skip"])
