"""The conv size guard on both sides of 2 GiB, without a GPU (the GPU side: test_gpu_conv_limits.py).

The library's answers (stv_conv_fits, stv_conv_config, stv_conv_tune: host arithmetic, nothing is launched) are held to
tests/conv_limits.py, which writes the byte count of every descriptor of every form out a second time.  The limit counts
BYTES per tensor: 2^30 fp32 elements pass an element count and are a 4 GiB map (test_bf16x3_host.py pins that for bf16x3).
"""
from __future__ import annotations

import ctypes

import pytest
import torch

from style_transfer_visualizer_amd import _lib, ops, plan

from . import conv_limits as cl
from .test_layerwise_host import vgg_layers

DTYPE = {"bf16": _lib.STV_BF16, "fp32": _lib.STV_F32, "bf16x3": _lib.STV_BF16X3}
REFUSED = -(100 + 1)                    # -(100 + STV_ERR_ARG): stv_conv_config and stv_conv_tune


def lib_fits(form, prec, H, W, cin, cout, cin2=0) -> bool:
    rc = int(_lib.load().stv_conv_fits(H, W, cin, cout, 1 if form == "1x1" else 9, cin2, cl.FORM_CODE[form], DTYPE[prec]))
    assert rc in (0, 1), rc
    return rc == 0


def lib_tile_queries(form, prec, H, W, cin, cout) -> list[int]:
    """stv_conv_config and stv_conv_tune for the forms they answer for (stv.h): taps 9 / 1, STV_TUNE_ROUTE."""
    taps = {"forward": 9, "1x1": 1, "pooled": 9, "route": ops.TUNE_ROUTE}[form]
    lib = _lib.load()
    return [int(lib.stv_conv_config(H, W, cin, cout, taps, DTYPE[prec])), int(lib.stv_conv_tune(H, W, cin, cout, taps, DTYPE[prec], None))]


def pin(monkeypatch) -> None:
    monkeypatch.setenv("STV_CONV_TUNE", "0")            # stv_conv_tune looks up, never measures
    monkeypatch.delenv("STV_CONV_CFG", raising=False)


def check(form, prec, H, W, cin, cout, cin2, want):
    what = f"{form} {prec} {H}x{W} {cin}->{cout} cin2={cin2}: {cl.tensor_bytes(form, prec, H, W, cin, cout, cin2)}"
    assert cl.conv_fits(form, prec, H, W, cin, cout, cin2) == want, what
    assert lib_fits(form, prec, H, W, cin, cout, cin2) == want, what
    if form != "dual":              # (the tile queries do not see cin2: stv.h)
        for r in lib_tile_queries(form, prec, H, W, cin, cout):
            assert (r >= 0) if want else (r == REFUSED), f"{what}: tile query {r}"


@pytest.mark.parametrize("case", cl.boundary_cases(), ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}x{c[3]}")
def test_largest_accepted_and_smallest_refused(case, monkeypatch):
    pin(monkeypatch)
    form, prec, H, W, cin, cout, cin2, want, _ = case
    check(form, prec, H, W, cin, cout, cin2, want)


@pytest.mark.parametrize(("prec", "H", "W", "want"), cl.TABLE, ids=lambda v: str(v))
def test_table_of_64_channel_maps(prec, H, W, want, monkeypatch):
    """3x3, 64 -> 64: every fp32 map over 2 GiB used to pass the element count, and stv_conv_config refused nothing."""
    pin(monkeypatch)
    lib = _lib.load()
    assert cl.conv_fits("forward", prec, H, W, 64, 64) == want
    tune = int(lib.stv_conv_tune(H, W, 64, 64, 9, DTYPE[prec], None))
    cfg = int(lib.stv_conv_config(H, W, 64, 64, 9, DTYPE[prec]))
    assert ((tune >= 0) if want else (tune == REFUSED)), f"stv_conv_tune {tune}"
    assert ((cfg >= 0) if want else (cfg == REFUSED)), f"stv_conv_config {cfg}"
    for form in ("forward", "pooled"):
        assert lib_fits(form, prec, H, W, 64, 64) == want
    assert lib_fits("dual", prec, H, W, 64, 64, 64) == want


@pytest.mark.parametrize(("prec", "H", "W", "C"), cl.EXACT, ids=lambda v: str(v))
def test_maps_of_exactly_2_gib_stay_accepted(prec, H, W, C, monkeypatch):
    pin(monkeypatch)
    assert H * W * C * cl.ES[prec] == cl.LIMIT
    for form in ("forward", "1x1", "pooled"):
        check(form, prec, H, W, C, C, 0, True)
    check("dual", prec, H, W, C, C, C, True)
    if prec == "bf16":              # as the routed output of a map a quarter its size
        check("route", prec, H // 2, W // 2, C, C, 0, True)
        check("route", prec, H // 2, W // 2 + 1, C, C, 0, False)


@pytest.mark.parametrize("case", cl.LONE, ids=lambda c: f"{c[0]}-{c[1]}-{c[7]}")
def test_each_tensor_decides_alone(case, monkeypatch):
    pin(monkeypatch)
    form, prec, H, W, cin, cout, cin2, tensor = case
    assert cl.deciders(form, prec, H, W, cin, cout, cin2) == [tensor]
    check(form, prec, H, W, cin, cout, cin2, False)
    if tensor in ("x2", "w2"):      # the tile queries see neither: they answer for the launch without the second term
        assert all(r >= -1 for r in lib_tile_queries("forward", prec, H, W, cin, cout))
    if tensor == "out":             # the same shape as a plain dgrad is fine
        check("forward", prec, H, W, cin, cout, 0, True)


@pytest.mark.parametrize("case", cl.POOLED_ODD, ids=lambda c: f"{c[1]}-{c[2]}x{c[3]}")
def test_pooled_launch_at_odd_sizes(case, monkeypatch):
    """The pooled map and its byte map are floor(H/2) x floor(W/2): always below the full map, which decides."""
    pin(monkeypatch)
    form, prec, H, W, cin, cout, want = case
    t = cl.tensor_bytes(form, prec, H, W, cin, cout)
    assert t["pool"] < t["y"] and t["idx"] < t["y"] and (H % 2 or W % 2)
    check(form, prec, H, W, cin, cout, 0, want)
    assert lib_fits("forward", prec, H, W, cin, cout) == want


def test_query_refuses_what_no_entry_point_takes():
    lib = _lib.load()
    ok = (64, 64, 16, 16)
    assert lib.stv_conv_fits(*ok, 9, 0, 0, _lib.STV_BF16) == 0
    assert lib.stv_conv_fits(*ok, 9, 0, 0, 7) == 1                       # dtype
    assert lib.stv_conv_fits(*ok, 5, 0, 0, _lib.STV_BF16) == 1           # taps
    assert lib.stv_conv_fits(*ok, 9, 0, 4, _lib.STV_BF16) == 1           # form
    assert lib.stv_conv_fits(*ok, 1, 0, 1, _lib.STV_BF16) == 1           # a 1x1 is a plain launch
    assert lib.stv_conv_fits(*ok, 9, 0, 2, _lib.STV_BF16) == 1           # a dual launch has a cin2
    assert lib.stv_conv_fits(*ok, 9, 16, 0, _lib.STV_BF16) == 1          # ... and nothing else has
    assert lib.stv_conv_fits(*ok, 9, 0, 3, _lib.STV_F32) == 1            # routing is bf16 only
    assert lib.stv_conv_fits(0, 64, 16, 16, 9, 0, 0, _lib.STV_BF16) == 1
    assert lib.stv_conv_fits(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 9, 0, 0, _lib.STV_F32) == 1     # no 64-bit wrap
    assert lib.stv_conv_fits(2 ** 31 - 1, 2 ** 31 - 1, 16, 2 ** 31 - 1, 9, 2 ** 31 - 1, 2, _lib.STV_F32) == 1
    assert lib.stv_version() >= 119


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: on a GPU machine a guard that regressed would launch on them")
def test_launch_entry_points_refuse_before_any_hip_call():
    """Refused shapes only, pointers that are never dereferenced: STV_ERR_ARG (1), not a launch error (2)."""
    lib = _lib.load()
    p = ctypes.c_void_p(16)
    for prec, H, W, want in cl.TABLE:
        if want:
            continue
        d = DTYPE[prec]
        fl = ops.W_BLOCKED if prec == "bf16x3" else 0
        assert lib.stv_conv_igemm(p, p, None, None, p, H, W, 64, 64, 9, fl, d, None) == 1
        assert lib.stv_conv_igemm(p, p, None, p, p, H, W, 64, 64, 9, fl | ops.MASK | ops.ACCUM, d, None) == 1
        assert lib.stv_conv_igemm(p, p, None, None, p, H, W, 64, 64, 1, 0, d, None) == 1
        assert lib.stv_conv_igemm_pool(p, p, None, p, p, p, H, W, 64, 64, fl, d, None) == 1
        assert lib.stv_conv_igemm_pool(p, p, None, None, p, p, H, W, 64, 64, fl | ops.POOL_ONLY, d, None) == 1
        assert lib.stv_conv_igemm_dual(p, p, p, p, None, p, H, W, 64, 64, 64, fl, d, None) == 1
    for form, prec, H, W, cin, cout, cin2, _ in cl.LONE:
        d = DTYPE[prec]
        fl = ops.W_BLOCKED if prec == "bf16x3" else 0
        if form == "route":
            assert lib.stv_conv_igemm_route(p, p, p, p, H, W, cin, cout, 0, d, None) == 1
        elif form == "dual":
            assert lib.stv_conv_igemm_dual(p, p, p, p, None, p, H, W, cin, cin2, cout, fl, d, None) == 1
        else:
            assert lib.stv_conv_igemm(p, p, None, None, p, H, W, cin, cout, 1 if form == "1x1" else 9,
                                      fl if form != "1x1" else 0, d, None) == 1


# ---- the plan refuses when it is built -------------------------------------------------------------------------------
META = torch.device("meta")             # nothing is allocated, whatever the size


def schedule(H, W, dtype, *, split=False, upto=2):
    return plan.Schedule(vgg_layers(), [upto], [], H, W, dtype, META, with_grad=False, split=split)


@pytest.mark.parametrize(("H", "W", "dtype", "split", "nbytes"), [
    (4096, 4096, torch.float32, False, 4096 * 4096 * 64 * 4),
    (cl.first_refused_square("fp32", 64),) * 2 + (torch.float32, False, cl.first_refused_square("fp32", 64) ** 2 * 64 * 4),
    (7680, 4320, torch.bfloat16, False, 7680 * 4320 * 64 * 2),
    (4096, 4096, torch.float32, True, 4096 * 4096 * 64 * 4),
], ids=["fp32-4096", "fp32-first-refused", "bf16-8k", "bf16x3-4096"])
def test_schedule_refuses_a_map_over_the_limit(H, W, dtype, split, nbytes):
    assert nbytes > cl.LIMIT
    name = "bf16" if dtype == torch.bfloat16 else "fp32"
    ways = ("" if name == "bf16" else "bf16 storage, ") + "a smaller image size, or row strips on several GPUs"
    with pytest.raises(ValueError, match=rf"layer 0: its {H}x{W}x64 {name} map holds {nbytes} bytes, over the conv kernels' limit of "
                                         rf"{cl.LIMIT} bytes per tensor \(32-bit offsets\): use {ways}$"):
        schedule(H, W, dtype, split=split)


def test_schedule_names_the_layer_that_is_too_large():
    """A first layer that fits in front of a wider one that does not: the refusal names the second conv."""
    layers = [torch.nn.Conv2d(3, 8, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(8, 64, 3, padding=1)]
    with pytest.raises(ValueError, match="layer 2: its 4096x4096x64 fp32 map"):
        plan.Schedule(layers, [2], [], 4096, 4096, torch.float32, META, with_grad=False)


@pytest.mark.parametrize(("H", "W", "dtype", "split"), [
    (3840, 2160, torch.float32, False), (4096, 4096, torch.bfloat16, False), (3840, 2160, torch.float32, True),
    (cl.first_refused_square("fp32", 64) - 1,) * 2 + (torch.float32, False),
], ids=["fp32-4k", "bf16-4096", "bf16x3-4k", "fp32-last-accepted"])
def test_schedule_accepts_up_to_the_limit(H, W, dtype, split):
    s = schedule(H, W, dtype, split=split)
    assert [nd.kind for nd in s.nodes] == ["conv_first", "conv"]
    assert max(nd.dst.act.numel() * nd.dst.act.element_size() for nd in s.nodes) <= cl.LIMIT


def test_device_form_plan_at_exactly_2_gib_routes_the_pooling_backward():
    """bf16 at 4096^2: conv1_2's map and the routed output of conv2_1's dgrad are exactly 2^31 bytes - the plan is built
    with every fusion a smaller image gets (the library's guard decides, at most 2^31 bytes), one column more is refused."""
    s = plan.Schedule(vgg_layers(), [0, 5], [7], 4096, 4096, torch.bfloat16, META, with_grad=True, assume_device=True)
    kinds = [(nd.kind, nd.layer) for nd in s.nodes]
    assert kinds == [("conv_first", 0), ("conv", 2), ("pool", 4), ("conv", 5), ("conv", 7)]
    assert s.nodes[2].fused and s.nodes[2].idx is not None and s.nodes[3].route is s.nodes[2]
    assert s.nodes[1].dst.act.numel() * 2 == cl.LIMIT
    assert cl.conv_fits("route", "bf16", 2048, 2048, 128, 64) and not cl.conv_fits("route", "bf16", 2048, 2049, 128, 64)
    with pytest.raises(ValueError, match="layer 0: its 4096x4098x64 bf16 map holds 2148532224 bytes"):
        plan.Schedule(vgg_layers(), [0, 5], [7], 4096, 4098, torch.bfloat16, META, with_grad=True, assume_device=True)


def test_row_strips_count_their_halo_rows():
    """A strip's buffers carry two halo rows: they count."""
    rows = cl.LIMIT // (8192 * 64 * 2)          # 2048 rows of 8192 x 64 bf16 = 2 GiB
    s = plan.Schedule(vgg_layers(), [0], [], rows - 2, 8192, torch.bfloat16, META, with_grad=False, halo=1)
    assert s.nodes[0].dst.act.shape[0] == rows
    with pytest.raises(ValueError, match=rf"layer 0: its {rows + 1}x8192x64 bf16 map"):
        plan.Schedule(vgg_layers(), [0], [], rows - 1, 8192, torch.bfloat16, META, with_grad=False, halo=1)
