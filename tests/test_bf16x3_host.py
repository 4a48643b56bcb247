"""bf16x3 precision (fp32 storage, split-bf16 products): configuration, ABI and the split's arithmetic, no GPU."""
from __future__ import annotations

import ctypes
import math
import os
import re

import pytest
import torch
from pydantic import ValidationError

from style_transfer_visualizer_amd import _lib, cli, core_model, ops
from style_transfer_visualizer_amd import config as stv_config

from . import bf16x3_emul as emu

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "stv.h")
VGG19 = [(3, 64), (64, 64), "M", (64, 128), (128, 128), "M", (128, 256), (256, 256), (256, 256), (256, 256), "M",
         (256, 512), (512, 512), (512, 512), (512, 512), "M", (512, 512), (512, 512), (512, 512), (512, 512)]


def _conv_shapes(size: int) -> list[tuple[int, int, int]]:
    out, s = [], size
    for e in VGG19:
        if e == "M":
            s //= 2
        elif e[0] != 3:                       # the first layer has a kernel of its own (fp32 in bf16x3 mode)
            out.append((s, e[0], e[1]))
    return out


def test_cli_and_toml_accept_bf16x3(tmp_path):
    args = cli.build_arg_parser().parse_args("--content a --style b --precision bf16x3".split())
    assert stv_config.build_config_from_cli(vars(args)).hardware.precision == "bf16x3"
    p = tmp_path / "c.toml"
    p.write_text('[hardware]\nprecision = "bf16x3"\n')
    assert stv_config.ConfigLoader.load(str(p)).hardware.precision == "bf16x3"
    with pytest.raises(ValidationError):
        stv_config.StyleTransferConfig.model_validate({"hardware": {"precision": "fp8"}})


def test_precision_resolution(monkeypatch):
    assert core_model.resolve_precision("bf16x3") == torch.float32 and core_model.resolve_split("bf16x3")
    assert not core_model.resolve_split("fp32") and not core_model.resolve_split("bf16")
    monkeypatch.setenv("STV_PRECISION", "bf16x3")
    assert core_model.resolve_precision() == torch.float32 and core_model.resolve_split()
    with pytest.raises(ValueError, match="fp8"):
        core_model.resolve_precision("fp8")


def test_enum_matches_header():
    text = open(HEADER).read()
    m = re.search(r"STV_BF16X3\s*=\s*(\d+)", text)
    assert m and int(m.group(1)) == _lib.STV_BF16X3 == 2
    assert ops.dtype_code(torch.float32, split=True) == _lib.STV_BF16X3
    with pytest.raises(RuntimeError):
        ops.dtype_code(torch.bfloat16, split=True)


@pytest.mark.parametrize("size", [64, 512, 1024])
def test_every_vgg19_shape_has_a_split_tile(monkeypatch, size):
    monkeypatch.setenv("STV_CONV_TUNE", "0")
    lib = _lib.load()
    for s, cin, cout in _conv_shapes(size):
        assert lib.stv_conv_config(s, s, cin, cout, 9, _lib.STV_BF16X3) >= 0, (s, cin, cout)      # forward
        assert lib.stv_conv_config(s, s, cout, cin, 9, _lib.STV_BF16X3) >= 0, (s, cout, cin)      # dgrad
        assert lib.stv_conv_config(s, s, cout, cout, 1, _lib.STV_BF16X3) >= 0                      # Gram backward
        assert lib.stv_conv_uses_ws(s, s, cin, cout, 9, _lib.STV_BF16X3, 0, 0, 0) == 0


def test_storage_only_entry_points_reject_bf16x3():
    lib = _lib.load()
    p = ctypes.c_void_p(16)          # never dereferenced: the dtype check comes first
    X3 = _lib.STV_BF16X3
    assert lib.stv_maxpool_fwd(p, p, 8, 8, 64, X3, None) == 1
    assert lib.stv_maxpool_bwd(p, p, p, 8, 8, 64, 0, X3, None) == 1
    assert lib.stv_relu_fwd(p, p, ctypes.c_size_t(64), X3, None) == 1
    assert lib.stv_relu_bwd(p, p, p, ctypes.c_size_t(64), 0, X3, None) == 1
    assert lib.stv_content_loss(p, p, p, ctypes.c_size_t(64), X3, None) == 1
    assert lib.stv_gram_finish(p, None, p, p, None, 64, 64, ctypes.c_float(5e5), ctypes.c_float(1.0),
                               ctypes.c_float(1.0), None, X3, None) == 1
    assert lib.stv_conv_first_fwd(p, p, None, p, None, 8, 8, 3, 64, X3, None) == 1
    assert lib.stv_conv_first_dgrad(p, p, p, 8, 8, 3, 64, X3, None) == 1
    assert lib.stv_conv_igemm_route(p, p, p, p, 8, 8, 64, 64, 0, X3, None) == 1


def test_byte_guard_counts_bytes():
    """4096 x 4096 x 64 fp32 = 4 GiB: 2^30 elements pass an element count, the 32-bit byte descriptors do not.
    (Every form, precision and tensor on both sides of the bound: tests/test_conv_limits_host.py, which holds the
    library's one predicate to a second writing of the byte counts; the maps of exactly 2^31 bytes on the GPU:
    tests/test_gpu_conv_limits.py.)"""
    lib = _lib.load()
    p = ctypes.c_void_p(16)
    assert lib.stv_conv_igemm(p, p, None, None, p, 4096, 4096, 64, 64, 9, 0, _lib.STV_BF16X3, None) == 1
    assert lib.stv_conv_igemm_pool(p, p, None, p, p, None, 4096, 4096, 64, 64, 0, _lib.STV_BF16X3, None) == 1
    assert lib.stv_conv_igemm_dual(p, p, p, p, None, p, 4096, 4096, 64, 64, 64, 0, _lib.STV_BF16X3, None) == 1
    assert lib.stv_gram_partial(p, p, 4096 * 4096, 64, _lib.STV_BF16X3, None) == 1
    assert lib.stv_conv_tune(4096, 4096, 64, 64, 9, _lib.STV_BF16X3, None) == -101


def test_weight_forms_are_fixed_per_geometry():
    """3x3: pre-split K-blocked weights only; 1x1 (the Gram-backward seed): plain fp32 weights only."""
    lib = _lib.load()
    p = ctypes.c_void_p(16)
    X3, WB = _lib.STV_BF16X3, _lib.W_BLOCKED
    assert lib.stv_conv_igemm(p, p, None, None, p, 64, 64, 64, 64, 9, 0, X3, None) == 1
    assert lib.stv_conv_igemm(p, p, None, None, p, 64, 64, 64, 64, 1, WB, X3, None) == 1
    assert lib.stv_conv_igemm_pool(p, p, None, p, p, None, 64, 64, 64, 64, 0, X3, None) == 1
    assert lib.stv_conv_igemm_dual(p, p, p, p, None, p, 64, 64, 64, 64, 64, 0, X3, None) == 1


def test_split_weights_layout():
    w = torch.randn(9, 2, 5, 8) * 3.0
    s = ops.split_weights(w)
    assert s.shape == w.shape and s.dtype == torch.float32
    q = s.view(torch.int16).view(torch.bfloat16).reshape(9, 2, 5, 2, 2, 4).float()   # [.., group, hi/lo, 4]
    hi, lo = emu.split(w)
    assert torch.equal(q[..., 0, :].reshape(w.shape).double(), hi)
    assert torch.equal(q[..., 1, :].reshape(w.shape).double(), lo)


def test_split_emulation_against_float64():
    g = torch.Generator().manual_seed(3)
    a = torch.randn(4096, generator=g) * torch.exp(torch.randn(4096, generator=g) * 4)
    b = torch.randn(4096, generator=g)
    special = torch.tensor([0.0, -0.0, 1e-40, -3e-39, 1.17e-38, float("inf"), -float("inf"), float("nan"), 3.3e38])
    a = torch.cat([a, special]); b = torch.cat([b, torch.full_like(special, 0.75)])
    got = emu.product3(a, b)
    exact = a.double() * b.double()
    fin = torch.isfinite(exact) & torch.isfinite(got)
    normal = a.abs() > 2.0 ** -100                  # lo of a (near-)subnormal x falls below bf16's smallest step
    rel = ((got - exact).abs() / exact.abs().clamp_min(1e-300))[fin & normal]
    assert float(rel.max()) < 2.0 ** -15            # worst case ~2^-16 relative, typical ~2^-18
    assert float(rel.median()) < 2.0 ** -17
    # (near-)subnormal values: absolute error at bf16's subnormal step
    tiny = fin & ~normal
    assert float((got - exact)[tiny].abs().max()) <= 2.0 ** -133 * 0.75 * 4
    # hi + lo reproduces x to ~2^-17, signed zeros and subnormals included
    hi, lo = emu.split(a)
    finite = torch.isfinite(a)
    assert torch.all(((hi + lo) - a.double())[finite].abs() <= a.double()[finite].abs() * 2.0 ** -16 + 2.0 ** -133)
    assert math.copysign(1.0, float(emu.split(torch.tensor([-0.0]))[0][0])) == -1.0
    # non-finite in -> non-finite out, and lo never carries the NaN alone
    assert not torch.isfinite(got[-4:-1]).any()
    assert torch.all(emu.split(special)[1][torch.isinf(special) | torch.isnan(special)] == 0)


def test_row_strips_refuse_bf16x3():
    from style_transfer_visualizer_amd import plan, spatial
    with pytest.raises(ValueError, match="bf16x3"):
        spatial.HaloShard([], [], [], torch.zeros(1, 3, 16, 16), [], dtype=torch.float32, style_w=1.0, content_w=1.0,
                          split=True)
    with pytest.raises(ValueError, match="bf16x3"):
        plan.Schedule([], [0], [], 16, 16, torch.bfloat16, torch.device("cpu"), with_grad=True, split=True)
