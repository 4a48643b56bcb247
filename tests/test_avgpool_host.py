"""Average pooling (--pooling avg) without a GPU: the twin of the two kernels against torch's CPU avg_pool2d, the ABI of
stv_avgpool_fwd / stv_avgpool_bwd and their argument refusals, the planner's average-pool step as a host engine in device form
builds it, the replaced module stack and its slicing (torch on the CPU against the float64 definition; ``forward()`` itself is held
to it on the GPU), every refusal, and the default call that does not pass the keyword."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from oracle import core_model_ref as ocm
from style_transfer_visualizer_amd import _lib, cli, config_defaults, core_model, plan, spatial, synthetic
from style_transfer_visualizer_amd import config as stv_config
from tests import avgpool_ref as ref
from tests.test_core_model_host import CPU, RecordedProgram, _image, _layers, fused_step, host_engine, step_signature

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_TAPS = ([0, 5, 10, 19, 28], [21])
TRAP_TAPS = ([0, 2, 5], [7])        # conv1_2 (layer 2) tapped: its ReLU is pending when the pool behind it (layer 4) is reached
SMALL_CFG = (8, 8, "M", 16, 16, "M", 32, 32, 32, 32, "M", 64, 64, 64, 64, "M", 64, 64, 64, 64, "M")


# ---- 1. the twin against torch's CPU avg_pool2d ------------------------------------------------------------------------------------

def _nchw(t):
    return t.permute(2, 0, 1).unsqueeze(0).contiguous()


def _nhwc(t):
    return t[0].permute(1, 2, 0).contiguous()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 2, 1), (5, 7, 3), (6, 10, 8), (9, 4, 8), (17, 13, 3), (31, 33, 1)])
def test_twin_is_torch_cpu_avg_pool2d_and_its_gradient(shape, dtype):
    H, W, C = shape
    g = torch.Generator().manual_seed(H * 1000 + W * 10 + C)
    x = (torch.randn(H, W, C, generator=g) * 3).to(dtype)
    xn = _nchw(x).requires_grad_(True)
    y = F.avg_pool2d(xn, 2, 2)
    assert np.array_equal(ref.fwd(x).float().numpy(), _nhwc(y.detach()).float().numpy())
    dy = (torch.randn(H // 2, W // 2, C, generator=g) * 3).to(dtype)
    (dx,) = torch.autograd.grad(y, xn, _nchw(dy))
    got = ref.bwd(dy, H, W)
    assert got.dtype == dtype and np.array_equal(got.float().numpy(), _nhwc(dx).float().numpy())
    # the ReLU forms: relu then pool, and the pool's gradient through that ReLU
    yr = F.avg_pool2d(F.relu(xn), 2, 2)
    assert np.array_equal(ref.fwd(x, relu_in=True).float().numpy(), _nhwc(yr.detach()).float().numpy())
    (dxr,) = torch.autograd.grad(yr, xn, _nchw(dy))
    assert np.array_equal(ref.bwd(dy, H, W, ref=x).float().numpy(), _nhwc(dxr).float().numpy())


def test_twin_sums_in_scan_order_and_accumulates_with_one_rounding():
    # ((1 + 0) + 2^-24) + 2^-24 = 1 (two ties to even), (1 + 0) + (2^-24 + 2^-24) = 1 + 2^-23: only the scan order gives torch's bits
    a, b, c, d = 1.0, 0.0, 2.0 ** -24, 2.0 ** -24
    x = torch.tensor([[[a], [b]], [[c], [d]]], dtype=torch.float32)
    want = np.float32(np.float32(np.float32(np.float32(a) + np.float32(b)) + np.float32(c)) + np.float32(d)) * np.float32(0.25)
    pairwise = np.float32(np.float32(np.float32(a) + np.float32(b)) + np.float32(np.float32(c) + np.float32(d))) * np.float32(0.25)
    assert float(ref.fwd(x)[0, 0, 0]) == float(want) == float(F.avg_pool2d(_nchw(x), 2, 2)) != float(pairwise)
    # bf16 ties: three ones and 1 + 2^-6 have the mean 1 + 2^-8, half-way between 1 and 1 + 2^-7: to even, 1;
    # three times 1 + 2^-7 and one 1 + 2^-6 + 2^-7 ... = 1 + 2^-7 + 2^-8: half-way between 1 + 2^-7 and 1 + 2^-6: to even, 1 + 2^-6
    lo = torch.tensor([[[1.0], [1.0]], [[1.0], [1.0 + 2.0 ** -6]]]).bfloat16()
    u = 1.0 + 2.0 ** -7
    hi = torch.tensor([[[u], [u]], [[u], [u + 2.0 ** -6]]]).bfloat16()
    assert float(ref.fwd(lo)[0, 0, 0]) == 1.0 == float(F.avg_pool2d(_nchw(lo), 2, 2))
    assert float(ref.fwd(hi)[0, 0, 0]) == 1.0 + 2.0 ** -6 == float(F.avg_pool2d(_nchw(hi), 2, 2))
    # accumulate: dx + 0.25 * dy in fp32, rounded once - 1 + 2^-8 is a tie that goes down to 1, (1 + 2^-7) + 2^-8 one that goes
    # up to 1 + 2^-6; the odd tail keeps its value (5), and without accumulation it is written zero
    dy = torch.tensor([[[2.0 ** -6]]]).bfloat16()
    for start, want in ((1.0, 1.0), (u, 1.0 + 2.0 ** -6)):
        dx = torch.full((3, 3, 1), 5.0).bfloat16()
        dx[:2, :2] = start
        got = ref.bwd(dy, 3, 3, dx=dx)
        assert got[:2, :2].float().unique().tolist() == [want]
        assert got[2].float().unique().tolist() == [5.0] and got[:, 2].float().unique().tolist() == [5.0]
    plain = ref.bwd(dy, 3, 3)
    assert plain[:2, :2].float().unique().tolist() == [2.0 ** -8]
    assert float(plain[2].float().abs().max()) == 0 and float(plain[:, 2].float().abs().max()) == 0


# ---- 2. ABI -----------------------------------------------------------------------------------------------------------------------

def test_library_exports_the_entry_points_and_the_constants_match_the_header():
    lib = _lib.load()
    for name in ("stv_avgpool_fwd", "stv_avgpool_bwd"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "stv.h")).read()
    for name, value in (("STV_AVGPOOL_THREADS", _lib.AVGPOOL_THREADS), ("STV_AVGPOOL_MAX_BLOCKS", _lib.AVGPOOL_MAX_BLOCKS)):
        assert re.search(rf"#define {name} {value}\b", header), name
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    names = re.findall(r"STV_OP_[A-Z_0-9]+", body[body.index("STV_OP_CONV_FIRST_FWD = 1"):])
    assert names.index("STV_OP_AVGPOOL_FWD") + 1 == _lib.OP_AVGPOOL_FWD == _lib.OP_MASK_SPLIT + 1 == 20      # appended
    assert names.index("STV_OP_AVGPOOL_BWD") + 1 == _lib.OP_AVGPOOL_BWD == 21 == len(names)
    assert lib.stv_version() >= 113
    assert "avgpool.hip" in open(os.path.join(ROOT, "style_transfer_visualizer_amd", "csrc", "Makefile")).read()
    assert ctypes.sizeof(_lib.StvOp) == 120           # stv_op_t keeps its layout


def test_argument_refusals_run_without_a_gpu():
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    a, b, c = base, base + 1024, base + 2048
    ERR = 1

    def fwd(x=a, y=b, H=4, W=4, C=8, flags=0, dtype=_lib.STV_F32):
        return lib.stv_avgpool_fwd(x, y, H, W, C, flags, dtype, None)

    def bwd(r=a, dy=b, dx=c, H=4, W=4, C=8, flags=0, dtype=_lib.STV_F32):
        return lib.stv_avgpool_bwd(r, dy, dx, H, W, C, flags, dtype, None)
    assert fwd(dtype=_lib.STV_BF16X3) == bwd(dtype=_lib.STV_BF16X3) == fwd(dtype=7) == bwd(dtype=-1) == ERR
    assert fwd(x=None) == fwd(y=None) == bwd(dy=None) == bwd(dx=None) == ERR
    assert bwd(r=None, flags=_lib.MASK) == bwd(r=None, flags=_lib.MASK | _lib.ACCUM) == ERR      # ref only with STV_MASK
    for bad in (dict(H=0), dict(W=0), dict(C=0), dict(H=-2), dict(W=-2), dict(C=-8), dict(H=1), dict(W=1)):
        assert fwd(**bad) == bwd(**bad) == ERR, bad
    # a tensor of 2 GiB or more: 2^29 fp32 elements, 2^30 bf16 elements; and sizes whose product overflows an int
    assert fwd(H=1 << 15, W=1 << 13, C=2) == bwd(H=1 << 15, W=1 << 13, C=2) == ERR
    assert fwd(H=1 << 15, W=1 << 14, C=2, dtype=_lib.STV_BF16) == bwd(H=1 << 15, W=1 << 14, C=2, dtype=_lib.STV_BF16) == ERR
    assert fwd(H=1 << 16, W=1 << 16, C=1) == bwd(H=1 << 20, W=1 << 20, C=1 << 20) == ERR
    for flag in (_lib.RELU_OUT, _lib.MASK, _lib.ACCUM, _lib.W_BLOCKED, _lib.POOL_IDX, _lib.POOL_ROUTE, _lib.POOL_ONLY, 256):
        assert fwd(flags=flag) == fwd(flags=flag | _lib.RELU_IN) == ERR, flag
    for flag in (_lib.RELU_IN, _lib.RELU_OUT, _lib.W_BLOCKED, _lib.POOL_IDX, _lib.POOL_ROUTE, _lib.POOL_ONLY, 256):
        assert bwd(flags=flag) == bwd(flags=flag | _lib.MASK | _lib.ACCUM) == ERR, flag


# ---- 3. the planner ----------------------------------------------------------------------------------------------------------------

def _avg_layers():
    return list(core_model.replace_pooling(nn.Sequential(*_layers()), "avg").children())


def avg_engine(monkeypatch, dtype, H, W, style_at, content_at, split=False, **env):
    """``tests.test_core_model_host.host_engine`` on the stack with average pools."""
    for name in ("STV_LOSS_BATCH", "STV_GRAM_FIN_LATE", "STV_LOSS_INTERLEAVE", "STV_FUSE_CONTENT"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    monkeypatch.setattr(plan, "Program", RecordedProgram)
    eng = core_model._Engine(_avg_layers(), style_at, content_at, H, W, dtype, CPU, assume_device=True, split=split)
    for tap in eng.sched.style_taps:
        tap.target = torch.zeros(tap.buf.C, tap.buf.C)
    for tap in eng.sched.content_taps:
        tap.target = torch.empty_like(tap.buf.act)
    return eng


def avg_step(eng, x, grad):
    eng.loss_and_grad(x, grad, 1e5, 1.0)
    (key,) = [k for k in eng._programs if k[0] == "fused"]
    return key, eng._programs[key].op_list


def test_replace_pooling_keeps_indices_parameters_and_the_generator():
    base = nn.Sequential(*_layers())
    state = torch.get_rng_state()
    avg = core_model.replace_pooling(base, "avg")
    assert torch.equal(torch.get_rng_state(), state)                      # no generator draw
    assert core_model.replace_pooling(base, "max") is base
    assert avg.training == base.training and core_model.replace_pooling(base.eval(), "avg").training is False
    assert core_model.replace_pooling(base.train(), "avg").training is True
    a, b = list(base.children()), list(avg.children())
    assert len(a) == len(b)
    for i, (la, lb) in enumerate(zip(a, b, strict=True)):
        if isinstance(la, nn.MaxPool2d):
            assert isinstance(lb, nn.AvgPool2d) and (lb.kernel_size, lb.stride, lb.padding, lb.ceil_mode) == (2, 2, 0, False), i
        else:
            assert lb is la
    assert sum(p.numel() for p in avg.parameters()) == sum(p.numel() for p in base.parameters())
    assert any(isinstance(l, nn.MaxPool2d) for l in base.children())      # the given (possibly cached) stack is untouched


@pytest.mark.parametrize("dtype,split", [(torch.float32, False), (torch.bfloat16, False), (torch.float32, True)],
                         ids=["fp32", "bf16", "bf16x3"])
def test_average_pools_are_ops_of_their_own_and_keep_off_every_pool_fusion(monkeypatch, dtype, split):
    eng = avg_engine(monkeypatch, dtype, 64, 64, *DEFAULT_TAPS, split=split)
    s = eng.sched
    pools = [nd for nd in s.nodes if nd.kind == "avgpool"]
    assert len(pools) == 4 and not any(nd.kind == "pool" for nd in s.nodes)
    assert all(not nd.fused and nd.idx is None and nd.src.stored and not nd.relu_in for nd in pools)
    assert all(nd.route is None for nd in s.nodes) and all(nd.dst.stored for nd in s.nodes)
    key, op_list = avg_step(eng, _image(64, 64, "x"), _image(64, 64, "x.grad"))
    assert ("pooling", "avg") in key and eng.pooling == "avg"
    kinds = [o.op for o in op_list]
    assert kinds.count(_lib.OP_AVGPOOL_FWD) == 4 and kinds.count(_lib.OP_AVGPOOL_BWD) == 4
    assert _lib.OP_POOL_FWD not in kinds and _lib.OP_POOL_BWD not in kinds
    convs = [o for o in op_list if o.op == _lib.OP_CONV]
    assert not any(o.q1 for o in convs) and not any(o.flags & (_lib.POOL_ROUTE | _lib.POOL_ONLY) for o in convs)
    storage = _lib.STV_BF16 if dtype == torch.bfloat16 else _lib.STV_F32         # bf16x3: the two ops run as STV_F32
    by_layer = {nd.layer: nd for nd in pools}
    fwd = [o for o in op_list if o.op == _lib.OP_AVGPOOL_FWD]
    bwd = [o for o in op_list if o.op == _lib.OP_AVGPOOL_BWD]
    for o, nd in zip(fwd, pools, strict=True):
        assert (o.dtype, o.flags, o.H, o.W, o.cin) == (storage, 0, nd.src.H, nd.src.W, nd.src.C)
        assert (o.p0, o.q0) == (nd.src.act.data_ptr(), nd.dst.act.data_ptr())
    for o, nd in zip(bwd, reversed(pools), strict=True):
        # the source of every default pool is a conv with the ReLU in its epilogue and no tap: the mask, ref = the stored map
        assert nd.src.relu_fused and not nd.src.taps
        assert (o.dtype, o.flags, o.H, o.W, o.cin) == (storage, _lib.MASK, nd.src.H, nd.src.W, nd.src.C)
        assert (o.p0, o.p1, o.q0) == (nd.src.act.data_ptr(), nd.dst.grad.data_ptr(), nd.src.grad.data_ptr())
    assert sorted(by_layer) == [4, 9, 18, 27]


def test_max_is_the_step_and_the_key_of_a_model_without_the_keyword(monkeypatch):
    x, grad = _image(64, 64, "x"), _image(64, 64, "x.grad")
    a = host_engine(monkeypatch, torch.bfloat16, 64, 64, *DEFAULT_TAPS)
    want = step_signature(fused_step(a, x, grad))
    monkeypatch.setattr(core_model, "initialize_vgg", lambda: nn.Sequential(*_layers()))
    plain, given = core_model.StyleContentModel(*DEFAULT_TAPS), core_model.StyleContentModel(*DEFAULT_TAPS, pooling="max")
    assert plain.pooling == given.pooling == "max"
    assert plain._engine_key(64, 64, 0) == given._engine_key(64, 64, 0) == (64, 64, 0)
    assert core_model.StyleContentModel(*DEFAULT_TAPS, pooling="avg")._engine_key(64, 64, 0) == (64, 64, 0, ("pooling", "avg"))
    monkeypatch.setattr(plan, "Program", RecordedProgram)
    b = core_model._Engine(given._layers(), *DEFAULT_TAPS, 64, 64, torch.bfloat16, CPU, assume_device=True)
    for tap in b.sched.style_taps:
        tap.target = torch.zeros(tap.buf.C, tap.buf.C)
    for tap in b.sched.content_taps:
        tap.target = torch.empty_like(tap.buf.act)
    assert b.pooling == "max"
    assert step_signature(fused_step(b, x, grad)) == want and list(b._programs) == list(a._programs)
    assert not any("pooling" in str(k) for k in b._programs)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_a_pending_relu_is_taken_by_the_average_pool(monkeypatch, dtype):
    """Style layers [0, 2, 5]: conv1_2 is tapped, its ReLU (layer 3) is pending at the pool (layer 4).  A max pool hands it to
    conv2_1; the average pool applies it itself: RELU_IN forward, MASK with ref = z backward, nothing pending behind it."""
    eng = avg_engine(monkeypatch, dtype, 64, 64, *TRAP_TAPS)
    s = eng.sched
    pool = next(nd for nd in s.nodes if nd.kind == "avgpool" and nd.layer == 4)
    after = s.nodes[s.nodes.index(pool) + 1]
    assert pool.relu_in and pool.src.taps and not pool.src.relu_fused
    assert after.kind == "conv" and after.layer == 5 and after.src is pool.dst and not after.relu_in
    _, op_list = avg_step(eng, _image(64, 64, "x"), _image(64, 64, "x.grad"))
    (f,) = [o for o in op_list if o.op == _lib.OP_AVGPOOL_FWD and o.q0 == pool.dst.act.data_ptr()]
    (b,) = [o for o in op_list if o.op == _lib.OP_AVGPOOL_BWD and o.q0 == pool.src.grad.data_ptr()]
    assert f.flags == _lib.RELU_IN and f.p0 == pool.src.act.data_ptr()
    # (the pool's op writes z's gradient; the tap's dF = F.S, which sees z itself, accumulates behind it, unmasked)
    assert b.flags == _lib.MASK and b.p0 == pool.src.act.data_ptr()
    later = op_list[op_list.index(b) + 1:]
    (tap_term,) = [o for o in later if o.op == _lib.OP_CONV and o.taps == 1 and o.q0 == pool.src.grad.data_ptr()]
    assert tap_term.flags & _lib.ACCUM and not tap_term.flags & _lib.MASK
    conv5 = [o for o in op_list if o.op == _lib.OP_CONV and o.taps == 9 and o.p0 == pool.dst.act.data_ptr()]
    assert len(conv5) == 1 and not conv5[0].flags & _lib.RELU_IN
    # the same taps under max pooling: the pool passes the ReLU on
    m = plan.Schedule(_layers(), *TRAP_TAPS, 64, 64, dtype, CPU, with_grad=True, assume_device=True)
    mp = next(nd for nd in m.nodes if nd.kind == "pool" and nd.layer == 4)
    assert not mp.relu_in and m.nodes[m.nodes.index(mp) + 1].relu_in


def test_guidance_counts_both_pool_types():
    from style_transfer_visualizer_amd import guidance
    want = guidance.tap_shapes(70, 52, _layers(), DEFAULT_TAPS[0])
    assert guidance.tap_shapes(70, 52, _avg_layers(), DEFAULT_TAPS[0]) == want == [(70, 52), (35, 26), (17, 13), (8, 6), (4, 3)]


# ---- 4. the definition against the model's module stack -------------------------------------------------------------------------------

@pytest.fixture
def small_vgg(monkeypatch):
    weights = synthetic.synthetic_conv_weights(3, SMALL_CFG)
    monkeypatch.setattr(core_model, "initialize_vgg", lambda: core_model.build_vgg_features(weights, SMALL_CFG).eval())
    return weights


@pytest.mark.parametrize("taps", [DEFAULT_TAPS, TRAP_TAPS], ids=["default", "0-2-5"])
def test_replaced_module_stack_and_its_slicing_against_the_float64_definition(small_vgg, taps):
    """A check of ``replace_pooling`` and of the block slicing, not of the HIP path: the model's ``vgg_blocks`` - torch modules,
    with ``nn.AvgPool2d`` where the pools were - evaluated by torch on the CPU in fp32 against the float64 statement of the
    definition in ``tests/avgpool_ref.py`` (same layers at the same indices, the same taps, the same Gram and MSE).
    ``forward()`` itself runs on the GPU only: tests/test_gpu_avgpool_model.py holds it, and its autograd backward, to that
    definition.  Bounds: fp32 torch against float64 torch, scores 1e-5 relative, gradient 2e-5 relative rms."""
    style_at, content_at = taps
    model = core_model.StyleContentModel(style_at, content_at, pooling="avg")
    layers = model._layers()
    assert sum(isinstance(l, nn.AvgPool2d) for l in layers) >= 1 and not any(isinstance(l, nn.MaxPool2d) for l in layers)
    content, style = synthetic.synthetic_image(0, 64, 64), synthetic.synthetic_image(1, 64, 64)
    x = synthetic.synthetic_image(2, 64, 64)

    def block_losses(img, targets=None):
        outs, cur = [], img
        for block in model.vgg_blocks:
            cur = block(cur)
            outs.append(cur)
        if targets is None:
            return [ocm.gram_matrix(outs[j]).detach() for j in model.style_ids], [outs[j].detach() for j in model.content_ids]
        st, ct = targets
        return (torch.stack([F.mse_loss(ocm.gram_matrix(outs[j]), t) for j, t in zip(model.style_ids, st, strict=True)]).sum(),
                torch.stack([F.mse_loss(outs[j], t) for j, t in zip(model.content_ids, ct, strict=True)]).sum())
    with torch.no_grad():
        st, _ = block_losses(style)
        _, ct = block_losses(content)
    xg = x.clone().requires_grad_(True)
    s32, c32 = block_losses(xg, (st, ct))
    t32 = 1e5 * s32 + 1.0 * c32
    (g32,) = torch.autograd.grad(t32, xg)

    w64 = [(w.double(), b.double()) for w, b in small_vgg]
    r = ref.Reference(ref.program(w64, SMALL_CFG), style_at, content_at)
    r.set_targets(style.double(), content.double())
    s64, c64, t64, g64 = r.loss_and_grad(x.double(), 1e5, 1.0)
    s32, c32, t32 = s32.detach(), c32.detach(), t32.detach()
    assert float(s32) == pytest.approx(float(s64), rel=1e-5) and float(c32) == pytest.approx(float(c64), rel=1e-5)
    assert float(t32) == pytest.approx(float(t64), rel=1e-5)
    err = float((g32.double() - g64).norm() / g64.norm())
    assert err <= 2e-5, f"gradient {err:.2e} (relative rms) from the float64 definition"
    # and the definition is not max pooling's: the two differ at order one
    rmax = ocm.OracleModel(ocm.vgg_program(w64, SMALL_CFG), style_at, content_at)
    rmax.set_targets(style.double(), content.double())
    assert abs(float(ocm.loss_and_grad(rmax, x.double(), 1e5, 1.0)[2]) - float(t64)) > 1e-2 * abs(float(t64))


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------

def _cli_config(argv):
    args = cli.build_arg_parser().parse_args(argv)
    base = stv_config.ConfigLoader.load(args.config) if args.config else None
    return stv_config.build_config_from_cli(vars(args), base_config=base)


def test_an_unknown_pooling_value_is_refused_with_the_value_named(small_vgg, tmp_path, capsys):
    class Options:
        pass
    for bad in ("mean", "AVG", "", None, 2, 0):
        with pytest.raises(ValueError, match=re.escape(f"got {bad!r}")):
            core_model.StyleContentModel(*DEFAULT_TAPS, pooling=bad)
        Options.pooling = bad                 # ... and where a run hands the option on: no value turns into "max" silently
        with pytest.raises(ValueError, match=re.escape(f"got {bad!r}")):
            core_model.pooling_option_kwargs(Options())
    with pytest.raises(ValueError, match="mean"):
        stv_config.StyleTransferConfig.model_validate({"optimization": {"pooling": "mean"}})
    toml = tmp_path / "config.toml"
    toml.write_text('[optimization]\npooling = "l2"\n')
    with pytest.raises(ValueError, match="l2"):
        stv_config.ConfigLoader.load(str(toml))
    with pytest.raises(SystemExit):
        cli.build_arg_parser().parse_args(["--content", "c.png", "--style", "s.png", "--pooling", "mean"])
    assert "invalid choice: 'mean'" in capsys.readouterr().err
    # (a value assigned past the validation - e.g. a library user's own options object - is refused where the model is built)
    oc = stv_config.StyleTransferConfig.model_validate({}).optimization
    object.__setattr__(oc, "pooling", "median")
    with pytest.raises(ValueError, match="got 'median'"):
        core_model.pooling_option_kwargs(oc)


def test_config_and_cli_round_trip(tmp_path, caplog):
    from style_transfer_visualizer_amd.type_defs import InputPaths
    assert config_defaults.DEFAULT_POOLING == "max"
    assert stv_config.StyleTransferConfig.model_validate({}).optimization.pooling == "max"
    assert _cli_config(["--content", "c.png", "--style", "s.png"]).optimization.pooling == "max"
    assert _cli_config(["--content", "c.png", "--style", "s.png", "--pooling", "avg"]).optimization.pooling == "avg"
    toml = tmp_path / "config.toml"
    toml.write_text('[optimization]\npooling = "avg"\n')
    assert stv_config.ConfigLoader.load(str(toml)).optimization.pooling == "avg"
    assert _cli_config(["--config", str(toml)]).optimization.pooling == "avg"
    assert _cli_config(["--config", str(toml), "--pooling", "max"]).optimization.pooling == "max"
    assert not hasattr(cli.build_arg_parser().parse_args(["--content", "c.png", "--style", "s.png"]), "pooling")
    paths = InputPaths(content_path="c.png", style_path="s.png")
    with caplog.at_level("INFO"):
        cli.log_parameters(paths, _cli_config(["--content", "c.png", "--style", "s.png"]))
    assert "Pooling" not in caplog.text
    caplog.clear()
    with caplog.at_level("INFO"):
        cli.log_parameters(paths, _cli_config(["--content", "c.png", "--style", "s.png", "--pooling", "avg"]))
    assert "Pooling: avg" in caplog.text


def test_row_strips_refuse_average_pooling():
    for shard in (spatial.SpatialShard, spatial.HaloShard):
        with pytest.raises(ValueError, match="pooling = 'avg'.*row-strip"):
            shard(_avg_layers(), *DEFAULT_TAPS, torch.zeros(1, 3, 64, 64), [], dtype=torch.float32, style_w=1.0, content_w=1.0)
    with pytest.raises(ValueError, match="no row strips"):
        plan.Schedule(_avg_layers(), *DEFAULT_TAPS, 32, 64, torch.float32, CPU, with_grad=True, halo=1)


@pytest.mark.parametrize("pool", [nn.AvgPool2d(3, 2), nn.AvgPool2d(2, 1), nn.AvgPool2d(2, 2, padding=1), nn.AvgPool2d(2, 2, ceil_mode=True),
                                  nn.AvgPool2d(2, 2, divisor_override=3), nn.AvgPool2d((2, 4), (2, 4))],
                         ids=["k3", "stride1", "pad1", "ceil", "divisor", "2x4"])
def test_an_average_pool_of_another_form_is_refused(pool):
    layers = [pool if i == 4 else l for i, l in enumerate(_layers())]
    with pytest.raises(RuntimeError, match=r"layer 4: only AvgPool2d\(2, 2\) has a HIP kernel"):
        plan.Schedule(layers, [0, 5], [7], 32, 32, torch.float32, CPU, with_grad=True)
    ok = [nn.AvgPool2d(2, 2, count_include_pad=False) if i == 4 else l for i, l in enumerate(_layers())]
    s = plan.Schedule(ok, [0, 5], [7], 32, 32, torch.float32, CPU, with_grad=True)     # irrelevant without padding
    assert [nd.kind for nd in s.nodes].count("avgpool") == 1


# ---- 6. the default call ---------------------------------------------------------------------------------------------------------------

def test_a_default_run_builds_the_model_with_the_call_it_always_made(monkeypatch):
    seen = []

    class Probe:
        def __init__(self, **kw):
            seen.append(kw)
            raise KeyboardInterrupt          # (the call is what is looked at: nothing is built)
    monkeypatch.setattr(core_model, "StyleContentModel", Probe)
    img = torch.zeros(1, 3, 16, 16)
    oc = stv_config.StyleTransferConfig.model_validate({}).optimization
    with pytest.raises(KeyboardInterrupt):
        core_model.prepare_model_and_input(img, img, CPU, oc)
    assert sorted(seen[-1]) == ["content_layers", "precision", "style_layers"]
    assert core_model.pooling_option_kwargs(oc) == {}
    oc.pooling = "avg"
    with pytest.raises(KeyboardInterrupt):
        core_model.prepare_model_and_input(img, img, CPU, oc)
    assert seen[-1]["pooling"] == "avg" and sorted(seen[-1]) == ["content_layers", "pooling", "precision", "style_layers"]

    # every pyramid level builds its model itself: the keyword with "avg", the call it always made without
    from style_transfer_visualizer_amd import pyramid
    cfg = stv_config.StyleTransferConfig.model_validate({})
    cfg.optimization.pyramid_levels, cfg.optimization.steps, cfg.video.create_video = 2, 2, False
    monkeypatch.setattr(pyramid.ops, "resize2x", lambda x, mode, out=None: F.avg_pool2d(x.detach(), 2))
    big = torch.zeros(1, 3, 128, 128)
    for pooling, want in (("max", ["content_layers", "precision", "style_layers"]),
                          ("avg", ["content_layers", "pooling", "precision", "style_layers"])):
        cfg.optimization.pooling = pooling
        with pytest.raises(KeyboardInterrupt):
            pyramid.run_pyramid(big, big, CPU, cfg, progress_bar=object())
        assert sorted(seen[-1]) == want and seen[-1].get("pooling", "max") == pooling

    class Bare:          # an options object from before the option existed
        style_layers, content_layers, init_method, lr, lbfgs_max_iter, lbfgs_max_eval = [0], [2], "content", 1.0, 1, 1
    with pytest.raises(KeyboardInterrupt):
        core_model.prepare_model_and_input(img, img, CPU, Bare())
    assert "pooling" not in seen[-1]
