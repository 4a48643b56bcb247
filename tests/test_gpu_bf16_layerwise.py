"""bf16 (the measured mode) held to a REAL bound at the benchmark's sizes: every tensor the bf16
path stores - each activation, each activation gradient, each Gram seed, the image gradient - is
compared with the oracle op applied to the KERNEL'S OWN stored inputs of that op ("teacher
forcing"), rounded to bf16 at the same point.

Why layer-wise and not end to end: with bf16 storage a network is chaotic with respect to
rounding.  A relative perturbation of 1e-7 of every conv sum (= a different fp32 summation order)
flips a few roundings by one bf16 ulp (2^-8); each flipped activation shifts 9*Cout sums of the
next layer by ~1e-4 and flips ~2 % of THOSE roundings, and after three layers the two runs differ
by independent +-1 ulp everywhere.  Measured on the reference arithmetic itself (CPU oracle with
bf16 rounding, VGG19, 128^2): 1e-7 noise on the conv sums moves the image gradient by 5.5 % rms,
the loss by 6e-5 (tests/test_oracle_golden.py::test_bf16_storage_is_chaotic_under_summation_order).
So two CORRECT bf16 evaluations agree on the loss to ~1e-4 and on the gradient only to ~10 %:
an end-to-end gradient tolerance cannot separate a wrong epilogue from rounding chaos, a per-op
comparison on identical inputs can.  Bound asserted here for every stored tensor: each element
within ONE bf16 ulp of the oracle's value (three where a loss tap accumulates onto an already rounded
gradient: two roundings), at most 2 % of the elements different at all (the
differences are roundings of fp32 sums that were accumulated in another order), pooling routes
bit-exact.  Measured fractions are printed in the parity table.
"""
from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

from style_transfer_visualizer_amd import _lib, core_model, ops, synthetic
from tests.conftest import record_parity

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
S_LAYERS, C_LAYERS = [0, 5, 10, 19, 28], [21]
STYLE_W, CONTENT_W = 1e5, 1.0


def _bf(t: torch.Tensor) -> torch.Tensor:
    return t.bfloat16().float()


def _nchw(act: torch.Tensor) -> torch.Tensor:
    """NHWC device buffer -> [1,C,H,W] fp32 on the CPU."""
    return act.detach().cpu().float().permute(2, 0, 1).unsqueeze(0).contiguous()


def _compare(case: str, what: str, got: torch.Tensor, want: torch.Tensor, *, exact: bool = False, ulps: float = 1.0) -> None:
    """`got`: what the kernel stored (bf16 values as fp32); `want`: bf16(oracle op on the same inputs)."""
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    diff = (got - want).abs()
    frac = float((diff > 0).float().mean())
    # one bf16 ulp is 2^-8..2^-7 of the value; the floor covers results that cancel to ~0 (there the
    # two fp32 sums differ by rounding of the terms, not of the result)
    scale = torch.maximum(got.abs(), want.abs())
    floor = 2.0 ** -7 * 1e-3 * float(want.abs().max())
    worst = float((diff / (2.0 ** -7 * scale + floor)).max())
    tol_frac = 0.0 if exact else 2e-2
    record_parity(case, f"{what}: fraction != oracle", frac, tol_frac,
                  "bit-exact expected" if exact else f"largest difference {worst:.2f} of one bf16 ulp (bound {ulps:g})")
    assert frac <= tol_frac, f"{case} {what}: {frac:.2e} of the elements differ"
    assert worst <= ulps, f"{case} {what}: an element is {worst:.2f} bf16 ulps from the oracle"


@pytest.mark.parametrize("size", [512, 1024])
def test_bf16_every_stored_tensor_within_one_ulp_of_the_oracle_op(size, monkeypatch):
    monkeypatch.setenv("STV_SYNTHETIC_WEIGHTS", "0")
    # every tensor the kernels CAN store: the product does not write the pre-pool maps nobody reads again
    # (STV_POOL_ONLY, plan.py); that form is compared with this one bit for bit at the end of the test
    monkeypatch.setenv("STV_SKIP_PREPOOL", "0")
    # ... and every gradient in a tensor of its own: the product rotates them through three slabs (plan.alloc_grads)
    monkeypatch.setenv("STV_GRAD_ARENA", "0")
    case = f"vgg19_{size}x{size}_bf16 layer-wise"
    content = synthetic.synthetic_image(0, size, size)
    style = synthetic.synthetic_image(1, size, size)
    x0 = torch.randn(content.shape, generator=torch.Generator().manual_seed(0))
    model = core_model.StyleContentModel(S_LAYERS, C_LAYERS, precision="bf16").to(DEV)
    model.set_targets(style.to(DEV), content.to(DEV))
    x = x0.to(DEV).requires_grad_(True)
    s_hip, c_hip, t_hip = (float(v) for v in model.loss_and_grad(x, STYLE_W, CONTENT_W))
    torch.cuda.synchronize()
    eng = next(iter(model._engines.values()))
    prog = next(p for k, p in eng._programs.items() if k[0] == "fused")
    dual = {(H, W, cout) for (op, H, W, cin, cout, taps, n) in prog.op_meta if op == _lib.OP_CONV and taps == 9 and n > 0}
    nodes = eng.sched.nodes
    # pooling backward folded into the dgrad behind the pool (stv_conv_igemm_route): no POOL_BWD ops left,
    # and the pooled-resolution gradient buffers are never written
    routed = not any(op == _lib.OP_POOL_BWD for (op, *_rest) in prog.op_meta)

    def weights_of(nd):
        conv = eng.layers[nd.layer]
        w = conv.weight.detach().cpu().float()
        b = conv.bias.detach().cpu().float() if conv.bias is not None else None
        return (w if nd.kind == "conv_first" else _bf(w)), b      # first layer keeps fp32 weights (two-term split)

    # ------------------------------------------------------------------ forward, op by op
    for nd in nodes:
        got = _nchw(nd.dst.act)
        if nd.kind in ("conv", "conv_first"):
            inp = x0 if nd.src is None else _nchw(nd.src.act)
            if nd.relu_in:
                inp = F.relu(inp)
            w, b = weights_of(nd)
            z = F.conv2d(inp, w, b, padding=1)
            if nd.dst.relu_fused:
                z = F.relu(z)
            _compare(case, f"fwd L{nd.layer:02d} conv {nd.cin}->{nd.dst.C} @{nd.dst.H}", got, _bf(z))
        elif nd.kind == "pool":
            _compare(case, f"fwd L{nd.layer:02d} pool @{nd.dst.H}", got, F.max_pool2d(_nchw(nd.src.act), 2, 2), exact=True)
        else:
            _compare(case, f"fwd L{nd.layer:02d} relu", got, F.relu(_nchw(nd.src.act)), exact=True)

    # ------------------------------------------------------------------ losses and seeds from the stored features
    style_sum = 0.0
    for tap in eng.sched.style_taps:
        f = _nchw(tap.buf.act).double().reshape(tap.buf.C, -1)
        raw = f @ f.t()
        norm = float(tap.buf.C * f.shape[1])
        g = raw.clamp(max=5e5) / norm
        tgt = tap.target.detach().cpu().double()
        style_sum += float(((g - tgt) ** 2).mean())
        k = torch.tensor(STYLE_W, dtype=torch.float32) * 4.0 / (float(tap.buf.C) * float(tap.buf.C) * norm)
        seed = _bf(torch.where(raw <= 5e5, float(k) * (g - tgt), torch.zeros_like(g)).float())
        got = tap.sgrad.detach().cpu().float().reshape(tap.buf.C, tap.buf.C)
        # G - T cancels: the fp32 Gram sum's own rounding (1e-6 of G) is visible in small entries
        floor = 1e-5 * float(k) * float(g.abs().max())
        near = (raw - 5e5).abs() <= 1e-5 * 5e5
        dev = ((got - seed).abs() / (2.0 ** -7 * seed.abs() + floor)).masked_fill(near, 0.0)
        record_parity(case, f"Gram seed S tap {tap.order} (C={tap.buf.C})", float(dev.max()), 1.0, "in bf16 ulps (+ fp32 floor)")
        assert float(dev.max()) <= 1.0
    content_sum = 0.0
    for tap in eng.sched.content_taps:
        content_sum += float(((_nchw(tap.buf.act).double() - _nchw(tap.target).double()) ** 2).mean())
    for nm, got, want in (("style", s_hip, style_sum), ("content", c_hip, content_sum),
                          ("total", t_hip, STYLE_W * style_sum + CONTENT_W * content_sum)):
        rel = abs(got - want) / abs(want)
        record_parity(case, f"{nm} loss from the stored features (rel)", rel, 1e-5)
        assert rel <= 1e-5

    # ------------------------------------------------------------------ backward, buffer by buffer
    def tap_term(tap):
        fb = _nchw(tap.buf.act)
        if tap.kind == "style":
            s_mat = tap.sgrad.detach().cpu().float().reshape(tap.buf.C, tap.buf.C)
            return torch.einsum("nk,bkhw->bnhw", s_mat, fb)
        n = tap.buf.act.numel()
        return (CONTENT_W * 2.0 / n) * (fb - _nchw(tap.target))

    for k_nd, nd in enumerate(nodes):
        b = nd.dst
        consumer = next((c for c in nodes if c.src is b), None)
        if routed and nd.kind == "pool":
            continue                          # its gradient only ever exists in the registers of the routing dgrad
        act = _nchw(b.act)
        relu_mask_by_consumer = consumer is not None and (consumer.relu_in or (b.relu_fused and not b.taps))
        fused_tap = None
        g = None
        # content taps whose gradient the forward half already wrote (stv_content_loss_grad): rounded first, and
        # whatever produces this buffer's gradient accumulates onto the rounded value
        pre = [t for t in b.taps if t.kind == "content" and t.grad_fused]
        pre_sum = sum((_bf(tap_term(t)) for t in pre), torch.zeros(())) if pre else None
        if consumer is not None:
            dy = _nchw(consumer.dst.grad)
            if consumer.kind == "conv":
                w, _ = weights_of(consumer)
                base = F.conv_transpose2d(dy, w, padding=1)
                if relu_mask_by_consumer:
                    base = base * (act > 0)
                fused_tap = next((t for t in b.taps if t.kind == "style" and (b.H, b.W, b.C) in dual), None)
                if fused_tap is not None:
                    base = base + tap_term(fused_tap)
                if pre:
                    base = base + pre_sum
                g = _bf(base)
            elif consumer.kind == "pool":
                if routed:                    # pooled gradient = bf16(dgrad of the conv behind the pool), then routed
                    conv_b = next(c for c in nodes if c.src is consumer.dst)
                    wb_, _ = weights_of(conv_b)
                    dy = _bf(F.conv_transpose2d(_nchw(conv_b.dst.grad), wb_, padding=1))
                _, idx = F.max_pool2d(act, 2, 2, return_indices=True)
                g = torch.zeros_like(act).flatten(2).scatter_(2, idx.flatten(2), dy.flatten(2)).reshape(act.shape)
                if relu_mask_by_consumer:
                    g = g * (act > 0)
            else:
                g = dy * (act > 0)
            if pre and consumer.kind != "conv":
                g = _bf(g + pre_sum)
        elif pre:
            g = pre_sum
        for tap in b.taps:
            if tap is fused_tap or any(tap is t for t in pre):
                continue
            term = tap_term(tap)
            g = _bf(term) if g is None else _bf(g + term)
        if b.relu_fused and b.taps:
            g = g * (act > 0)
        exact = consumer is not None and consumer.kind != "conv" and not b.taps and not (routed and consumer.kind == "pool")
        # a tap that ACCUMULATES onto the stored gradient rounds twice: a one-ulp difference of the first
        # rounding survives into a sum that may be smaller than its terms -> up to ~1 ulp of the larger
        # term plus one of the result
        n_accum = sum(1 for t in b.taps if t is not fused_tap) - (1 if consumer is None else 0)
        _compare(case, f"bwd grad of L{nd.layer:02d} {nd.kind} out ({b.C}ch @{b.H})", _nchw(b.grad), g, exact=exact,
                 ulps=1.0 if n_accum <= 0 else 3.0)

    first = nodes[0]
    w, _ = weights_of(first)
    gx = F.conv_transpose2d(_nchw(first.dst.grad), w, padding=1)
    rel = float((x.grad.detach().cpu() - gx).norm() / gx.norm())
    record_parity(case, "image gradient from the stored dL/d(conv1_1) (rel rms)", rel, 1e-4,
                  "fp32 output; first-layer weights enter as a two-term bf16 split (2^-16 per product)")
    assert rel <= 1e-4

    # ------------------------------------------------------------------ the product's default: dead pre-pool maps not stored
    # Same kernels, same arithmetic, the full-resolution stores of the four pooling convs dropped (conv1_2: 134 of its
    # 312 MB at 1024^2): every tensor that IS stored, the scores and the image gradient must be bit-identical.
    monkeypatch.setenv("STV_SKIP_PREPOOL", "1")
    monkeypatch.setenv("STV_GRAD_ARENA", "1")
    model2 = core_model.StyleContentModel(S_LAYERS, C_LAYERS, precision="bf16").to(DEV)
    model2.set_targets(style.to(DEV), content.to(DEV))
    x2 = x0.to(DEV).requires_grad_(True)
    scores2 = tuple(float(v) for v in model2.loss_and_grad(x2, STYLE_W, CONTENT_W))
    torch.cuda.synchronize()
    eng2 = next(iter(model2._engines.values()))
    skipped = [nd for nd in eng2.sched.nodes if not nd.dst.stored]
    assert len(skipped) == 4 and all(nd.kind == "conv" for nd in skipped), [nd.layer for nd in skipped]
    assert scores2 == (s_hip, c_hip, t_hip)
    assert torch.equal(x2.grad, x.grad)
    for nd, nd2 in zip(nodes, eng2.sched.nodes, strict=True):
        if nd2.dst.stored:
            assert torch.equal(nd.dst.act, nd2.dst.act), f"L{nd.layer:02d} {nd.kind}: stored activation differs"
        if nd.idx is not None:
            assert torch.equal(nd.idx, nd2.idx), f"L{nd.layer:02d}: arg-max map differs"
    # the gradients of the default run rotate through a few slabs (two here: every pooling backward rides in a dgrad, so
    # the reverse schedule reads one gradient and writes one): only the last writer of each slab is still there (and the
    # image gradient above is every one of them pushed through the rest of the chain)
    slabs = eng2.sched._grad_slabs
    own = [nd2 for nd2 in eng2.sched.nodes if nd2.dst.grad.untyped_storage().data_ptr() != slabs.untyped_storage().data_ptr()]
    assert len(own) == 1 and own[0].dst.taps and own[0].dst.taps[0].kind == "content"
    assert slabs.shape[0] == 2, slabs.shape
    for i in range(2):                           # conv1_1's and conv1_2's outputs: the last writers of the two slabs
        assert torch.equal(nodes[i].dst.grad, eng2.sched.nodes[i].dst.grad), f"L{nodes[i].layer:02d}: gradient differs"
    skipped_mb = sum(nd.dst.act.numel() * 2 for nd in skipped) / 1e6
    record_parity(case, "pre-pool maps not stored (STV_POOL_ONLY): everything else vs the all-stored run", 0.0, 0.0,
                  f"bit-identical scores, image gradient, {len(nodes) - 4} activations, arg-max maps; gradients rotating through {slabs.shape[0]} slabs of {slabs.shape[1] / 1e6:.0f} MB; {skipped_mb:.0f} MB of stores dropped per closure")
    del model, x, model2, x2
    torch.cuda.empty_cache()
