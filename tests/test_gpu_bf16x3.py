"""bf16x3 (fp32 storage, split-bf16 products) on the GPU: each product kernel against a float64 emulation of the split
(tight: fp32 accumulation error only) and against exact float64, then whole models against the fp32 mode and the CPU
oracle."""
from __future__ import annotations

import pytest
import torch

from style_transfer_visualizer_amd import core_model, ops, synthetic

from . import bf16x3_emul as emu

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _rel(got: torch.Tensor, want: torch.Tensor) -> float:
    got, want = got.double().cpu(), want.double().cpu()
    return float((got - want).abs().max() / want.abs().max())


def _split_w(w: torch.Tensor, *, bwd: bool = False) -> torch.Tensor:
    packed = ops.pack_weights_bwd(w) if bwd else ops.pack_weights_fwd(w)
    return ops.split_weights(ops.block_weights(packed.to(DEV)))


@pytest.mark.parametrize(("size", "cin", "cout", "relu_in"), [(64, 64, 128, False), (64, 128, 64, True),
                                                              (32, 256, 256, False), (16, 512, 512, True)])
def test_conv3x3_matches_split_emulation(size, cin, cout, relu_in):
    g = torch.Generator().manual_seed(size + cin)
    x = torch.randn(size, size, cin, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    y = ops.conv_igemm(x.to(DEV), _split_w(w), flags=ops.RELU_IN if relu_in else 0, split=True)
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    assert _rel(y, emu.conv3x3(x, w, relu_in=relu_in)) < 1e-6
    err = _rel(y, emu.conv3x3(x, w, relu_in=relu_in, exact=True))
    assert err < 2e-5, err
    # the fp32 mode on the same inputs is untouched and no closer to float64 than ~1e-6
    y32 = ops.conv_igemm(x.to(DEV), ops.block_weights(ops.pack_weights_fwd(w).to(DEV)),
                         flags=ops.RELU_IN if relu_in else 0)
    assert _rel(y32, emu.conv3x3(x, w, relu_in=relu_in, exact=True)) < 1e-5


@pytest.mark.parametrize(("size", "cin", "cout"), [(64, 64, 64), (32, 128, 256), (16, 256, 512)])
def test_conv_relu_pool_epilogue_matches_split_emulation(size, cin, cout):
    """The fused form the schedule emits in front of a max-pool: conv + bias + ReLU, its 2x2 max-pool and arg-max map."""
    g = torch.Generator().manual_seed(5 + cin)
    x = torch.randn(size, size, cin, generator=g).clamp_min(0)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    idx = torch.empty(size // 2, size // 2, cout, dtype=torch.uint8, device=DEV)
    y, yp = ops.conv_igemm_pool(x.to(DEV), _split_w(w), b.to(DEV), flags=ops.RELU_OUT, pool_idx=idx, split=True)
    torch.cuda.synchronize()
    for exact, bound in ((False, 1e-6), (True, 2e-5)):
        full = (emu.conv3x3(x, w, exact=exact) + b.double()).clamp_min(0)
        pooled = torch.nn.functional.max_pool2d(full.permute(2, 0, 1)[None], 2)[0].permute(1, 2, 0)
        assert _rel(y, full) < bound, exact
        assert _rel(yp, pooled) < bound, exact


def test_dgrad_with_mask_and_gram_term_matches_split_emulation():
    """The dual form the fp32 schedule emits for a tapped layer: mask(ref > 0) * conv3x3(dy, w^T) + x2 . seed."""
    g = torch.Generator().manual_seed(7)
    H, cin, cout = 32, 128, 64
    dy = torch.randn(H, H, cout, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * 0.05
    ref = torch.randn(H, H, cin, generator=g)
    x2 = torch.randn(H, H, cin, generator=g).clamp_min(0)
    seed = torch.randn(cin, cin, generator=g) * 0.01
    out = ops.conv_igemm_dual(dy.to(DEV), _split_w(w, bwd=True), x2.to(DEV), seed.to(DEV)[None].contiguous(),
                              ref=ref.to(DEV), flags=ops.MASK, split=True)
    torch.cuda.synchronize()
    wt = w.flip(2, 3).transpose(0, 1)                       # dgrad as a forward conv
    for exact, bound in ((False, 1e-6), (True, 2e-5)):
        conv = emu.conv3x3(dy, wt, exact=exact) * (ref.double() > 0)
        if exact:
            gt = x2.double() @ seed.double().T
        else:
            xh, xl = emu.split(x2)
            sh, sl = emu.split(seed)
            gt = xh @ sh.T + xh @ sl.T + xl @ sh.T
        err = _rel(out, conv + gt)
        assert err < bound, (exact, err)


def test_gram_backward_1x1_plain_seed_is_split_in_the_kernel():
    g = torch.Generator().manual_seed(11)
    F = torch.randn(32, 32, 64, generator=g).clamp_min(0)
    seed = torch.randn(64, 64, generator=g) * 1e-3
    y = ops.conv_igemm(F.to(DEV), seed.to(DEV)[None].contiguous(), split=True)
    torch.cuda.synchronize()
    fh, fl = emu.split(F)
    sh, sl = emu.split(seed)
    assert _rel(y, fh @ sh.T + fh @ sl.T + fl @ sh.T) < 1e-6
    assert _rel(y, F.double() @ seed.double().T) < 2e-5


@pytest.mark.parametrize(("n", "C"), [(64 * 64, 64), (32 * 32, 256), (4099, 100), (777, 12)])
def test_gram_partial_matches_split_emulation(n, C):
    g = torch.Generator().manual_seed(C)
    F = torch.randn(n, C, generator=g).clamp_min(0) * 3.0
    R = ops.gram_partial(F.to(DEV), split=True).sum(0).cpu()
    # the slabs hold the tile pairs ti <= tj only (the finish kernel mirrors them): compare those
    ts = 64 if C <= 64 else 128
    t = torch.arange(C) // ts
    upper = t[:, None] <= t[None, :]
    assert _rel(R[upper], emu.gram(F)[upper]) < 1e-6
    err = _rel(R[upper], emu.gram(F, exact=True)[upper])
    assert err < 2e-5, err


def test_non_finite_inputs_give_non_finite_outputs():
    x = torch.randn(16, 16, 64)
    x[5, 7, 3] = float("inf")
    x[9, 2, 60] = float("nan")
    w = torch.randn(64, 64, 3, 3) * 0.05
    y = ops.conv_igemm(x.to(DEV), _split_w(w), split=True).cpu()
    assert not torch.isfinite(y[4:7, 6:9]).all() and not torch.isfinite(y[8:11, 1:4]).all()
    assert torch.isfinite(y[12:, 12:]).all()
    R = ops.gram_partial(x.reshape(-1, 64).to(DEV), split=True).sum(0).cpu()
    assert not torch.isfinite(R[3, 3]) and not torch.isfinite(R[60, 60]) and torch.isfinite(R[10, 20])


# ---- whole models -------------------------------------------------------------------------------------------------
CFG = (16, 16, "M", 32, 32, "M", 64, 64, 64, 64, "M", 128, 128, 128, 128, "M", 128, 128, 128, 128, "M")
S, C = [0, 5, 10, 19, 28], [21]


def _model(weights, precision):
    saved = core_model.initialize_vgg
    core_model.initialize_vgg = lambda: core_model.build_vgg_features(weights, CFG).eval()
    try:
        return core_model.StyleContentModel(S, C, precision=precision).to(DEV)
    finally:
        core_model.initialize_vgg = saved


@pytest.fixture(scope="module")
def setup():
    weights = synthetic.synthetic_conv_weights(3, CFG)
    content = synthetic.synthetic_image(0, 128, 128)
    style = synthetic.synthetic_image(1, 160, 128)
    x0 = synthetic.synthetic_image(2, 128, 128)
    return weights, content, style, x0


def _run(model, style, content, x0):
    model.set_targets(style.to(DEV), content.to(DEV))
    x = x0.to(DEV).requires_grad_(True)
    s, c, t = model.loss_and_grad(x, 1e5, 1.0)
    torch.cuda.synchronize()
    return [float(s)], [float(c)], float(t), x.grad.detach().cpu().clone()


def test_model_matches_oracle_and_fp32_mode(setup):
    """Narrow stack at 128^2: losses against the fp32 mode and the oracle; the gradient per pixel against the fp32
    oracle given the HIP path's ReLU / max-pool decisions (tests/test_gpu_bf16x3_fullsize.py: 512^2, full widths)."""
    from oracle import core_model_ref as ocm
    from tests import parity_util as pu
    weights, content, style, x0 = setup
    oracle = ocm.OracleModel(ocm.vgg_program(weights, CFG), S, C)
    oracle.set_targets(style, content)
    _, _, t_ref, _ = ocm.loss_and_grad(oracle, x0, 1e5, 1.0)
    m3 = _model(weights, "bf16x3")
    s3, c3, t3, g3 = _run(m3, style, content, x0)
    dec = pu.hip_decisions(m3)
    s1, c1, t1, g1 = _run(_model(weights, "fp32"), style, content, x0)
    assert abs(t3 - float(t_ref)) / abs(float(t_ref)) < 1e-4
    for a, b in zip(s3 + c3, s1 + c1, strict=True):
        assert abs(a - b) <= 1e-4 * abs(b) + 1e-12
    g_locked = ocm.loss_and_grad(pu.lock(oracle, dec), x0, 1e5, 1.0)[3]
    mx = float((g3 - g_locked).abs().max() / g_locked.abs().max())
    print(f"bf16x3 128^2 grad vs CPU-fp32 given the HIP decisions: {mx:.2e} of scale")
    assert mx < 1e-4, mx


def test_bit_reproducible_and_no_cross_talk(setup):
    weights, content, style, x0 = setup
    a = _run(_model(weights, "bf16x3"), style, content, x0)
    b = _run(_model(weights, "bf16x3"), style, content, x0)
    assert a[:3] == b[:3] and torch.equal(a[3], b[3])
    only32 = _run(_model(weights, "fp32"), style, content, x0)
    m32, m3 = _model(weights, "fp32"), _model(weights, "bf16x3")
    mixed3 = _run(m3, style, content, x0)
    mixed32 = _run(m32, style, content, x0)
    assert mixed32[:3] == only32[:3] and torch.equal(mixed32[3], only32[3])
    assert mixed3[:3] == a[:3] and torch.equal(mixed3[3], a[3])
