"""Layer-wise ("teacher forcing") check of one evaluated step: every tensor the step stored is compared with the
float64 oracle op applied to the inputs the kernel itself stored, inside an interval DERIVED per element.

Plain helper module (no fixtures, no hooks), shared by tests/test_layerwise_host.py (a torch-CPU stand-in of the
kernels: proves the checker without a GPU) and tests/test_gpu_step_layerwise.py (the kernels).

The interval.  An output whose float64 value is ``r`` - a sum of ``K`` terms (products, bias, the previous gradient,
tap terms) with absolute sum ``A`` (the same op on absolute values) - lies, evaluated in fp32 in ANY order with one
rounding per term (fmaf chains and the f32 matrix instructions included), within ``e = gamma(K) * A`` of ``r``,
``gamma(K) = K u / (1 - K u)``, ``u = 2^-24``.  Storage rounds monotonically, so the stored value is accepted iff

    round_T(r - e) <= got <= round_T(r + e)          (T = fp32 or bf16, float64 -> fp32 -> T as the kernels round)

which for bf16 is ONE admissible value except where ``r`` sits within ``e`` of a rounding boundary, and for fp32 is
``|got - r| <= e + ulp32(r)/2``.  ReLU, masks, max-pool and its routes only move or zero values: they are applied to
both interval ends (all are monotone), so on them the interval is a point and the comparison is bit-exact.

A gradient that several launches form in place (a pre-written content term, then a dgrad with ACCUM, then tap
terms with ACCUM) is rounded to storage after every launch and only the last value survives: the intermediate is not
observable.  The oracle then carries the interval through every stage - both ends rounded to storage where the kernel
rounds - which is the "one storage ulp of the intermediate" widening, and counts those tensors (``multi-stage``).
The pooled gradient inside a routing dgrad (POOL_ROUTE) is such an intermediate too: bf16-rounded, then moved.

Operands are what the kernel sees: fp32 - fp32; bf16 - bf16 activations and bf16-rounded weights, the first layer's
fp32 image and weights as two-term bf16 splits (forward: hi.hi + hi.lo + lo.hi, dgrad: dy . (hi + lo)); bf16x3 - the
three-term split product of tests/bf16x3_emul.py for the ops of ``plan._PRODUCT_OPS``, plain fp32 elsewhere.

Average pooling (``avgpool`` nodes; never fused, routed or indexed).  Forward: a point - the twin of stv.h's fixed
arithmetic ``(((a+b)+c)+d)*0.25f`` (tests/avgpool_ref.fwd), operands clamped first under the node's ``relu_in``, one rounding
to storage; bit-exact.  Backward: ``v = 0.25f * dy`` (exact) at ``y < 2*Hp, x < 2*Wp``, ``+0`` in the rows and columns the
floor drops, zeroed where the un-pooled map is ``<= 0`` when the node's mask holds (``nd.relu_in or (s.relu_fused and not
s.taps)``).  As the only writer the interval is a point; onto a pre-written gradient it is ONE fp32 add inside the pooled
range, ``e = gamma(1) * (|v| + |prev|)`` on the storage-rounded ``prev``, and nothing (``prev`` itself, ``e = 0``) in the
dropped rows and columns.

Spatial guidance (``engine.guide``).  Slab ``r`` of a tapped buffer holds the source's value where ``label == r`` and ``+0``
elsewhere, label 255 included: a point, and no element may be ``-0`` where the rule says ``+0`` (kind ``region slab``).
Every child tap of ``s.chains(tap)`` follows the Gram rule with ``f`` its slab as stored and ``norm = fp32(C * n_r)``, ``n_r``
counted here from the tap's label map; its combine scale is the engine's own row and must EQUAL ``fp32(w_l * lambda_r /
C^2)`` formed in double; its seed coefficient is ``fp32(style_w * w_l * lambda_r)`` formed in double.  The style score sums
all rows; ``engine.region_losses()`` is checked against ``fp32(1 / C^2) * sum d^2`` per row with the row's own error terms
(kind ``region loss``).  Backward: a tapped buffer receives one term per chain, in the order of ``s.chains(tap)``, each a
launch of its own with a storage rounding behind it (``stage``); the first accumulates only onto what was already written
(a pre-written content gradient, the consumer's dgrad); no term rides in a dgrad (``nd.gram`` under guidance is refused);
``relu_fused and taps`` masks once, after the last term.

Layer weights (``layer_w``, one per style tap): seed coefficient ``fp32(style_w * w_l)``, scale ``fp32(w_l / C^2)`` (asserted
equal to the engine's row).  A weight of 0.0 gives a seed of zeros (point interval at 0), and a launch all of whose
products are exact zeros (``A == 0`` at an element) adds an exact zero: ``e = 0`` there, the previous value survives.

Laplacian (``lap_w``; pools from ``engine.lap_pools``).  ``engine.lap_resid[k]`` is a point: ``tests/lap_ref.resid`` in fp32 on
``x0`` and the engine's own ``lap_targets[k]`` (kind ``lap residual``).  The total gains, after the TV term and in index
order, ``scale_k * sum r^2`` of the stored residual (scale: the engine's row, asserted equal to ``core_model.lap_scale``),
error ``gamma(depth + 2) * term`` with ``depth = lap_ref.partial_sum_depth`` plus one fp32 add.  The image gradient gains one
stage per pool after the TV stage: ``t = coef * upsample(L r)`` from the STORED residual in float64, ``coef =
core_model.lap_coef``; its error is the last two steps of ``lap_ref.bounds`` with exact inputs - the stencil bound
(``lap_ref._stencil_bound(r, 0)``), then ``|coef| * dg + u * |coef| * (|L r| + dg)`` - and one fp32 add onto the rounded
previous stage; pixels outside ``Hp*p x Wp*p`` receive nothing (``e = 0``, the previous stage's interval itself).

Refused (RuntimeError naming the offender): a node or tap kind without a rule here, ``lap_w`` on an engine without
``lap_pools``, a guided schedule without attached regions, a Gram term in a dgrad under guidance, ``gout`` together with
guidance, ``layer_w`` or ``lap_w`` (the autograd path has none of them), row strips.

Precondition: one tensor per gradient and every activation stored (STV_GRAD_ARENA=0, STV_SKIP_PREPOOL=0).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch
import torch.nn.functional as F

from style_transfer_visualizer_amd import _lib, core_model, plan, synthetic
from tests import bf16x3_emul as emul
from tests import lap_ref, tv_ref

NODE_KINDS = ("conv_first", "conv", "pool", "avgpool", "relu")
TAP_KINDS = ("style", "content")

U = 2.0 ** -24
# Unit roundoff assumed for the accumulation INSIDE the bf16 matrix instructions (bf16 convs, bf16x3 products, the
# bf16 first layer, the bf16 / bf16x3 Gram sums).  Their internal accumulation is not documented; 2^-24 is the fp32
# rule.  The issue allows 2^-23 for these ops only, if correct kernels exceed 2^-24 - see the worst ratios recorded.
U_BF16_MFMA = 2.0 ** -24


# The tap layouts (style, content) of the matrix: the default; a content tap in front of a pool's conv; taps on the convs
# in front of pools; a content tap on the first conv (alone, and with a second content tap); style and content on one
# buffer; taps on ReLU outputs; taps on pool outputs.
LAYOUTS = {
    "default": ([0, 5, 10, 19, 28], [21]),
    "content7": ([0, 5, 10, 19, 28], [7]),
    "prepool": ([2, 7], [16, 25]),
    "content_first": ([28], [0]),
    "two_content": ([28], [0, 21]),
    "shared_buffer": ([0, 5], [5, 21]),
    "relu_taps": ([1, 6, 11], [22]),
    "pool_taps": ([4, 9], [18]),
}
# Narrow nets (channel counts that are no multiples of 32), one per storage width, such that in each: a convolution
# falls off the matrix-core tiling (direct kernel, plain weights: ``wf.dim() != 4``), the pool behind it cannot ride in
# its epilogue, and a style tap sits in front of a matrix-core dgrad whose buffer misses the granularity of the dual launch
# (``s.C % (32 // element_size)``: 24 channels of bf16, 36 of fp32), so its Gram product stays a launch of its own.
NARROW_CFG = {"bf16": (16, 24, 32, "M", 40, 40, "M", 72), "fp32": (16, 36, 40, "M", 40, 40, "M", 72)}
NARROW_LAYOUT = ([0, 2, 9], [5, 12])


# The new structures of the matrix (shared by the host proof and the GPU matrix).  "pending_relu": the conv in front of the
# only pool is tapped, so the pool takes the pending ReLU itself; "content7" has pools of both kinds in one schedule.
PENDING_RELU_LAYOUT = ([0, 2, 5], [7])
REGION_WEIGHTS = {1: (0.7,), 2: (0.7, 1.3), 3: (0.7, 1.3, 0.45)}       # not all 1, no power of two
LAYER_WEIGHTS = (0.5, 0.0, 1.7, 1.0, 3.0)
LAP_SIZE, GUIDE_SIZE = (42, 26), (64, 48)


TV_W, LAP_W = 50.0, 200.0
ALL3, TWO = ("fp32", "bf16", "bf16x3"), ("fp32", "bf16")
# name -> what the step is built with (keys absent: the step as it always was).  Sizes: 40x24 - pooled maps go odd (5x3 in
# front of the fourth pool: a row and a column dropped); 64x48 - the deepest map is 4x3, three regions all present there;
# 42x26 - p=4 gives 10x6 cells, p=8 5x3, two image rows and columns outside the cells in both.
STEP_CASES = {
    "avg default": dict(layout="default", size=(40, 24), pooling="avg", precisions=ALL3),
    "avg pending relu": dict(layout=PENDING_RELU_LAYOUT, size=(40, 24), pooling="avg", precisions=ALL3),
    "avg content7": dict(layout="content7", size=(40, 24), pooling="avg", precisions=ALL3),
    "avg pool taps": dict(layout="pool_taps", size=(40, 24), pooling="avg", precisions=ALL3),
    "avg shared buffer": dict(layout="shared_buffer", size=(32, 32), pooling="avg", precisions=ALL3),
    "avg prepool": dict(layout="prepool", size=(40, 24), pooling="avg", precisions=ALL3),
    "guided R=1": dict(layout="default", size=GUIDE_SIZE, regions=1, precisions=ALL3),
    "guided R=2": dict(layout="default", size=GUIDE_SIZE, regions=2, precisions=ALL3),
    "guided R=3": dict(layout="default", size=GUIDE_SIZE, regions=3, precisions=ALL3),
    "guided relu taps": dict(layout="relu_taps", size=GUIDE_SIZE, regions=2, precisions=TWO),
    "guided shared buffer": dict(layout="shared_buffer", size=GUIDE_SIZE, regions=2, precisions=TWO),
    "layer weights": dict(layout="default", size=(40, 24), layer_w=LAYER_WEIGHTS, precisions=ALL3),
    "lap (1,)": dict(layout="default", size=LAP_SIZE, lap_pools=(1,), lap_w=LAP_W, precisions=("fp32",)),
    "lap (1,) tv": dict(layout="default", size=LAP_SIZE, lap_pools=(1,), lap_w=LAP_W, tv_w=TV_W, precisions=("fp32",)),
    "lap (4,)": dict(layout="default", size=LAP_SIZE, lap_pools=(4,), lap_w=LAP_W, precisions=("fp32",)),
    "lap (4,) tv": dict(layout="default", size=LAP_SIZE, lap_pools=(4,), lap_w=LAP_W, tv_w=TV_W, precisions=("fp32",)),
    "lap (2, 8)": dict(layout="default", size=LAP_SIZE, lap_pools=(2, 8), lap_w=LAP_W, precisions=TWO),
    "lap (2, 8) tv": dict(layout="default", size=LAP_SIZE, lap_pools=(2, 8), lap_w=LAP_W, tv_w=TV_W, precisions=TWO),
    "all together": dict(layout="default", size=GUIDE_SIZE, pooling="avg", regions=2, layer_w=LAYER_WEIGHTS, tv_w=TV_W,
                         lap_pools=(4,), lap_w=LAP_W, precisions=TWO),
}
STEP_PARAMS = [(name, precision) for name, spec in STEP_CASES.items() for precision in spec["precisions"]]


def case_layout(spec: dict) -> tuple:
    return LAYOUTS[spec["layout"]] if isinstance(spec["layout"], str) else spec["layout"]


def guide_labels(regions: int, H: int = 64, W: int = 48) -> tuple[torch.Tensor, torch.Tensor]:
    """(content labels, style labels) of an ``H x W`` image pair, uint8: the content map has ``regions`` column bands and a
    band of 255 in its last quarter of rows, the style map ``regions`` row bands and a band of 255 in its last third of
    columns - so the two differ, every region is still present at a 4x3 tap (sampled rows 8, 24, 40, 56 and columns 8, 24,
    40 of a 64x48 map), and every tap has pixels that belong to no region."""
    content = (torch.arange(W) * regions // W).to(torch.uint8).repeat(H, 1)
    content[H - H // 4:, :] = 255
    style = (torch.arange(H) * regions // H).to(torch.uint8).reshape(H, 1).repeat(1, W)
    style[:, W - W // 3:] = 255
    return content.contiguous(), style.contiguous()


def assert_narrow_branches(eng) -> None:
    """The branches the narrow nets exist for were taken (shared with the GPU matrix)."""
    nodes = eng.sched.nodes
    convs = [nd for nd in nodes if nd.kind == "conv"]
    direct = [nd for nd in convs if nd.wf.dim() != 4]
    assert direct and any(nd.wf.dim() == 4 for nd in convs)
    assert any(nd.wb.dim() != 4 for nd in convs)
    excluded = [nd for nd in convs if nd.wb.dim() == 4 and any(t.kind == "style" for t in nd.src.taps)
                and nd.src.C % (32 // nd.src.act.element_size())]
    assert excluded and all(nd.gram is None for nd in excluded)
    pool = next(nd for k, nd in enumerate(nodes) if nd.kind == "pool" and nodes[k - 1] in direct)
    assert not pool.fused and pool.idx is None


def biased_weights(cfg: tuple) -> list:
    """Synthetic weights with a NON-zero bias per layer (the synthetic default is zero: a dropped bias would not show)."""
    return [(w, synthetic.synthetic_bias(7, li, w.shape[0])) for li, (w, _) in enumerate(synthetic.synthetic_conv_weights(0, cfg))]


def gamma(k: int, u: float = U) -> float:
    return k * u / (1.0 - k * u)


class LayerwiseMismatch(AssertionError):
    """``tensors``: the names of the stored tensors that left their interval, in the order they were checked."""

    def __init__(self, case: str, failures: list[tuple[str, str]]) -> None:
        self.tensors = [name for name, _ in failures]
        super().__init__(f"{case}: " + "; ".join(f"{name}: {why}" for name, why in failures))


@dataclass
class Report:
    """What one ``check_step`` saw: per tensor kind the worst ``(|got - r| - storage rounding) / e``, the number of
    elements that took the second admissible value, and the tensors whose interval went through several stages."""

    rows: dict = field(default_factory=dict)          # kind -> [worst ratio, second values, elements, tensors]
    multi_stage: list = field(default_factory=list)
    failures: list = field(default_factory=list)

    def add(self, kind: str, ratio: float, second: int, n: int) -> None:
        row = self.rows.setdefault(kind, [0.0, 0, 0, 0])
        row[0] = max(row[0], ratio)
        row[1] += second
        row[2] += n
        row[3] += 1


# ----------------------------------------------------------------------------------------------------- small helpers
def nchw(act: torch.Tensor) -> torch.Tensor:
    """NHWC buffer -> [1,C,H,W] float64 on the CPU (exact: every storage value is a double)."""
    return act.detach().cpu().double().permute(2, 0, 1).unsqueeze(0).contiguous()


def round_to(v: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """float64 -> fp32 (-> bf16), round to nearest even at each step as the kernels do; returned as float64."""
    v = v.float()
    if dtype == torch.bfloat16:
        v = v.bfloat16()
    return v.double()


def _ulp(v: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    bits = 8 if dtype == torch.bfloat16 else 24
    _, ex = torch.frexp(v.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(v), ex - bits)


def first_max(act: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """2x2/2 max pool (floor) of [1,C,H,W]: (maximum, window position q = 2*dy+dx of the FIRST maximum in scan order)."""
    H2, W2 = act.shape[2] // 2, act.shape[3] // 2
    win = torch.stack([act[:, :, dy:2 * H2:2, dx:2 * W2:2] for dy in (0, 1) for dx in (0, 1)])
    best, q = win[0], torch.zeros_like(win[0], dtype=torch.long)
    for k in range(1, 4):
        take = win[k] > best
        best, q = torch.where(take, win[k], best), torch.where(take, torch.full_like(q, k), q)
    return best, q


def scatter_pool(dy: torch.Tensor, q: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """Max-pool backward: ``dy`` [1,C,H/2,W/2] to window position ``q`` of a zero [1,C,H,W] map."""
    out = torch.zeros(dy.shape[0], dy.shape[1], H, W, dtype=dy.dtype)
    H2, W2 = dy.shape[2], dy.shape[3]
    for k in range(4):
        out[:, :, (k >> 1):2 * H2:2, (k & 1):2 * W2:2] = torch.where(q == k, dy, torch.zeros_like(dy))
    return out


def f32_scalar(*factors: float) -> torch.Tensor:
    out = torch.tensor(factors[0], dtype=torch.float32)
    for f in factors[1:]:
        out = out * torch.tensor(f, dtype=torch.float32)
    return out


def mode_of(engine) -> str:
    return "bf16" if engine.dtype == torch.bfloat16 else ("bf16x3" if engine.split else "fp32")


def _bilinear(fn, a: torch.Tensor, b: torch.Tensor, split: bool) -> tuple[torch.Tensor, torch.Tensor, int]:
    """``fn`` (bilinear, float64) on the operands as the kernel sees them: (value, the same on absolute values, products
    per term).  ``split``: the three-term product ah.bh + ah.bl + al.bh of two fp32 operands."""
    if not split:
        return fn(a, b), fn(a.abs(), b.abs()), 1
    (ah, al), (bh, bl) = emul.split(a), emul.split(b)
    r = fn(ah, bh) + fn(ah, bl) + fn(al, bh)
    A = fn(ah.abs(), bh.abs()) + fn(ah.abs(), bl.abs()) + fn(al.abs(), bh.abs())
    return r, A, 3


@dataclass
class Iv:
    """An interval [lo, hi] of float64 tensors around ``r``."""

    r: torch.Tensor
    lo: torch.Tensor
    hi: torch.Tensor

    @classmethod
    def of(cls, r: torch.Tensor, e: torch.Tensor | float = 0.0) -> Iv:
        return cls(r, r - e, r + e)

    def map(self, fn) -> Iv:          # a monotone (non-decreasing) elementwise function
        return Iv(fn(self.r), fn(self.lo), fn(self.hi))

    def rounded(self, dtype: torch.dtype) -> Iv:
        return self.map(lambda v: round_to(v, dtype))

    def absmax(self) -> torch.Tensor:
        return torch.maximum(self.lo.abs(), self.hi.abs())


# --------------------------------------------------------------------------------------------------------- the checker
class _Checker:
    def __init__(self, engine, x0, style_w, content_w, gout, x_grad, tv_w, case, report, lap_w=0.0, layer_w=None) -> None:
        self.eng, self.s = engine, engine.sched
        self.nodes = self.s.nodes
        self.x0 = x0.detach().cpu().double()
        self.mode = mode_of(engine)
        self.T = engine.dtype
        self.gout = None if gout is None else [float(v) for v in torch.as_tensor(gout).detach().float().cpu()]
        self.style_w, self.content_w = (1.0, 1.0) if gout is not None else (float(style_w), float(content_w))
        self.x_grad, self.tv_w, self.case, self.rep = x_grad, float(tv_w), case, report
        self.u_mm = U_BF16_MFMA if self.mode != "fp32" else U
        self.lap_w, self.layer_w, self.guide = float(lap_w), layer_w, engine.guide

    # -- the step's own combine head and coefficients
    def head(self) -> tuple:
        """(table, scale, losses) of the combine op this step ran (``_Engine._combine_op``'s choice)."""
        return self.eng.head(self.tv_w, self.lap_w, self.layer_w)

    def weights_of(self, chain) -> tuple[float, float]:
        """(w_l, lambda_r) of a Gram chain's tap."""
        parent = chain.parent if chain.parent is not None else chain
        w = 1.0 if self.layer_w is None else float(self.layer_w[parent.order])
        lam = 1.0 if self.guide is None else float(self.guide.weights[chain.order % self.guide.n])
        return w, lam

    def fail(self, name: str, why: str) -> None:
        self.rep.failures.append((name, why))

    # -- acceptance
    def accept(self, kind: str, name: str, got: torch.Tensor, iv: Iv, dtype: torch.dtype | None = None) -> None:
        dtype = dtype or self.T
        got = got.detach().cpu().double().reshape(iv.r.shape)
        lo, hi = round_to(iv.lo, dtype), round_to(iv.hi, dtype)
        bad = ~((got >= lo) & (got <= hi))           # (a NaN anywhere is outside)
        # how much of the derived error the kernel used: distance from the oracle value beyond the storage rounding,
        # relative to the element's own e (both taken after the monotone maps, so a clamped ReLU output reads 0 / 0)
        e = torch.maximum(iv.hi - iv.r, iv.r - iv.lo)
        excess = ((got - iv.r).abs() - _ulp(got, dtype) / 2).clamp_min(0.0)
        finite = (e > 0) & torch.isfinite(excess)
        ratio = float((excess[finite] / e[finite]).max()) if bool(finite.any()) else 0.0
        # bf16 storage: elements that took the second of two admissible values (fp32 storage: every value in e is one)
        second = int(((got != round_to(iv.r, dtype)) & ~bad).sum()) if dtype == torch.bfloat16 else 0
        self.rep.add(kind, ratio, second, got.numel())
        if bool(bad.any()):
            k = int(torch.nonzero(bad.flatten())[0])
            why = (f"{int(bad.sum())} of {got.numel()} elements outside their interval, first at {k}: got "
                   f"{float(got.flatten()[k])!r}, admissible [{float(lo.flatten()[k])!r}, {float(hi.flatten()[k])!r}]")
            self.rep.failures.append((name, why))

    # -- operands
    def weights(self, nd, *, dgrad: bool) -> tuple[torch.Tensor, torch.Tensor | None, bool]:
        """(weights as the kernel sees them [Cout,Cin,3,3] fp32-valued, bias, three-term split product?)"""
        conv = self.eng.layers[nd.layer]
        w = conv.weight.detach().cpu().float()
        b = conv.bias.detach().cpu().double() if conv.bias is not None else None
        first = nd.kind == "conv_first"
        if self.mode == "bf16":
            if not first:
                return w.bfloat16().float(), b, False
            if dgrad:                                        # dy . (hi + lo)
                hi, lo = emul.split(w)
                return (hi + lo), b, False
            return w, b, True                                 # forward: both operands split, three terms
        return w, b, self.mode == "bf16x3" and not first

    def conv_fwd(self, nd) -> Iv:
        inp = self.x0 if nd.src is None else nchw(nd.src.act)
        if nd.relu_in:
            inp = inp.clamp_min(0.0)
        w, b, split = self.weights(nd, dgrad=False)
        r, A, m = _bilinear(lambda a, c: F.conv2d(a.double(), c.double(), padding=1), inp, w, split)
        k = 9 * nd.cin * m
        if b is not None:
            r, A, k = r + b.view(1, -1, 1, 1), A + b.abs().view(1, -1, 1, 1), k + 1
        iv = Iv.of(r, gamma(k, self.u_mm if (self.mode != "fp32" and (split or nd.kind == "conv")) else U) * A)
        return iv.map(lambda v: v.clamp_min(0.0)) if nd.dst.relu_fused else iv

    def dgrad(self, nd) -> tuple[torch.Tensor, torch.Tensor, int, float]:
        """d(input) of conv `nd` from its stored output gradient: (r, A, K, u)."""
        dy = nchw(nd.dst.grad)
        w, _, split = self.weights(nd, dgrad=True)
        r, A, m = _bilinear(lambda a, c: F.conv_transpose2d(a.double(), c.double(), padding=1), dy, w, split)
        plain = self.mode == "fp32" or (self.mode == "bf16x3" and nd.kind == "conv_first")
        return r, A, 9 * nd.dst.C * m, (U if plain else self.u_mm)

    def seed_mat(self, tap) -> torch.Tensor:
        return tap.sgrad.detach().cpu().double().reshape(tap.buf.C, tap.buf.C)

    def tap_terms(self, tap) -> list[tuple[torch.Tensor, torch.Tensor, int, float]]:
        """The gradient terms of one tap on its buffer, one per launch: (r, A, K, u) - a style tap's one per Gram chain
        (per region under guidance, on the region's slab as stored), a content tap's one."""
        if tap.kind == "style":
            out = []
            for c in self.s.chains(tap):
                r, A, m = _bilinear(lambda a, w: torch.einsum("nk,bkhw->bnhw", w.double(), a.double()), nchw(c.buf.act),
                                    self.seed_mat(c), self.mode == "bf16x3")
                out.append((r, A, tap.buf.C * m, (self.u_mm if self.mode != "fp32" else U)))
            return out
        return [self.tap_term(tap)]

    def tap_term(self, tap) -> tuple[torch.Tensor, torch.Tensor, int, float]:
        """The gradient term of one tap with a single launch (a content tap, or a style tap without guidance)."""
        fb = nchw(tap.buf.act)
        if tap.kind == "style":
            (term,) = self.tap_terms(tap)
            return term
        k = self.content_k(tap)
        d = fb - nchw(tap.target)
        return k * d, (k * d).abs(), 2, U

    def content_k(self, tap) -> float:
        """coef * (2/n) as the kernels form it in fp32 (content_loss_kernel / content_grad_kernel)."""
        n = tap.buf.act.numel()
        two_n = torch.tensor(2.0, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)
        if self.gout is None:
            return float(f32_scalar(self.content_w) * two_n)
        return float(f32_scalar(1.0, self.gout[len(self.s.style_taps) + tap.order]) * two_n)

    # -- forward
    def forward(self) -> None:
        for k, nd in enumerate(self.nodes):
            name = f"act L{nd.layer:02d} {nd.kind}"
            if nd.kind in ("conv", "conv_first"):
                if nd.dst.stored:
                    self.accept("conv forward", name, nchw(nd.dst.act), self.conv_fwd(nd))
                else:
                    raise RuntimeError(f"{name}: not stored - the checker needs STV_SKIP_PREPOOL=0")
            elif nd.kind == "pool":
                best, q = first_max(nchw(nd.src.act))
                self.accept("pool forward", name, nchw(nd.dst.act), Iv.of(best))
                if nd.idx is not None:
                    code = (q + 4 * (best > 0)).double()
                    self.accept("arg-max map", f"idx L{nd.layer:02d}", nchw(nd.idx), Iv.of(code), torch.float32)
            elif nd.kind == "avgpool":
                from tests import avgpool_ref  # noqa: PLC0415  (it imports round_to from this module)
                want = avgpool_ref.fwd(nd.src.act.detach().cpu(), relu_in=nd.relu_in)
                self.accept("avgpool forward", name, nchw(nd.dst.act), Iv.of(nchw(want)))
            elif nd.kind == "relu":
                self.accept("relu forward", name, nchw(nd.dst.act), Iv.of(nchw(nd.src.act).clamp_min(0.0)))
            else:
                raise RuntimeError(f"{name}: no rule for a node of kind {nd.kind!r}")
            for tap in nd.dst.taps:
                if tap.kind == "style" and self.s.guide:
                    self.slabs(tap)

    def slabs(self, tap) -> None:
        """MASK_SPLIT: slab r = the source where label == r, +0 elsewhere (255 in no slab)."""
        src = nchw(tap.buf.act)
        labels = tap.labels.detach().cpu().long().reshape(1, 1, tap.buf.H, tap.buf.W)
        for r in range(self.s.guide):
            name = f"slab style{tap.order} r{r}"
            got = nchw(tap.slabs[r])
            inside = (labels == r).expand_as(src)
            self.accept("region slab", name, got, Iv.of(torch.where(inside, src, torch.zeros_like(src))))
            if bool((torch.signbit(got) & ~inside).any()):
                self.fail(name, "-0 outside the region (the rule writes +0)")

    # -- loss head
    def losses(self) -> None:
        s, eng = self.s, self.eng
        n_style = len(s.all_chains())
        x3 = self.mode == "bf16x3"
        terms, errs = [], []
        scale_row = self.eng.scale if self.gout is not None else self.head()[1]
        region_rows = []
        for row, tap in enumerate(s.all_chains()):
            C = tap.buf.C
            f = nchw(tap.buf.act).reshape(C, -1)
            n = f.shape[1]
            R, A, m = _bilinear(lambda a, c: a.double() @ c.double().t(), f, f, x3)
            e_R = gamma(n * m + 1, self.u_mm) * A
            w_l, lam = self.weights_of(tap)
            n_r = n if tap.parent is None else int((tap.parent.labels.detach().cpu() == tap.order % s.guide).sum())
            norm32 = torch.tensor(float(C * n_r), dtype=torch.float32)
            norm = float(norm32)
            G = R.clamp(max=plan.GRAM_CLAMP_MAX) / norm
            T = tap.target.detach().cpu().double()
            d = G - T
            e_G = e_R / norm + U * G.abs()
            e_d = e_G + U * (d.abs() + e_G)
            scale = float(scale_row[row])
            if self.gout is None and scale != core_model._fp32(w_l * lam / float(C * C)):
                self.fail(f"scale style{tap.order}", f"combine scale {scale!r} is not fp32(w_l * lambda_r / C^2) = "
                                                    f"{core_model._fp32(w_l * lam / float(C * C))!r}")
            sq = float((d * d).sum())
            e_sum = float((2 * d.abs() * e_d + e_d * e_d).sum()) + gamma(C * C + tap.parts_cnt + 1) * sq
            terms.append(scale * sq)
            errs.append(scale * e_sum + U * scale * sq)
            unit = core_model._fp32(1.0 / float(C * C))
            region_rows.append((tap.order, unit * sq, unit * e_sum + U * unit * sq))
            # the seed S = kk * [R <= clamp] * (G - T), kk = coef * 4 / (C * C * norm) (* upstream coefficient), in fp32
            c32 = torch.tensor(float(C), dtype=torch.float32)
            coef = self.style_w * w_l * lam if self.gout is None else 1.0       # formed in double, rounded to fp32 once
            kk = (f32_scalar(core_model._fp32(coef)) * 4.0) / (c32 * c32 * norm32)
            if self.gout is not None:
                kk = kk * torch.tensor(self.gout[tap.order], dtype=torch.float32)
            kk = float(kk)
            full, e_full = kk * d, abs(kk) * e_d + U * (kk * d).abs()
            zero = torch.zeros_like(d)
            live = R <= plan.GRAM_CLAMP_MAX
            near = (R - plan.GRAM_CLAMP_MAX).abs() <= e_R           # within e of the threshold either side is admissible
            r = torch.where(live, full, zero)
            lo = torch.where(live | near, torch.where(near, torch.minimum(full - e_full, zero), full - e_full), zero)
            hi = torch.where(live | near, torch.where(near, torch.maximum(full + e_full, zero), full + e_full), zero)
            self.accept("Gram seed", f"seed style{tap.order}", self.seed_mat(tap), Iv(r, lo, hi))
        if self.guide is not None:          # the unweighted per-row terms: one more combine launch over the same partials
            got_rows = eng.region_losses().detach().cpu().double().reshape(-1)
            for (order, r, e), got_r in zip(region_rows, got_rows, strict=True):
                self.accept("region loss", f"region loss style{order}", got_r.reshape(1),
                            Iv.of(torch.tensor([r], dtype=torch.float64), e), torch.float32)
        c_terms, c_errs = [], []
        for tap in s.content_taps:
            d = nchw(tap.buf.act) - nchw(tap.target)
            n = d.numel()
            scale = float(scale_row[n_style + tap.order])
            sq = float((d * d).sum())
            c_terms.append(scale * sq)
            c_errs.append(scale * gamma(n + tap.parts_cnt + 3) * sq + U * scale * sq)
        style, content = sum(terms), sum(c_terms)
        e_style = sum(errs) + gamma(max(len(terms), 1)) * style
        e_content = sum(c_errs) + gamma(max(len(c_terms), 1)) * content
        total = self.style_w * style + self.content_w * content
        e_total = (abs(self.style_w) * e_style + abs(self.content_w) * e_content
                   + gamma(3) * (abs(self.style_w) * style + abs(self.content_w) * content))
        if self.tv_w:
            C, H, W = self.x0.shape[1:]
            term = core_model.tv_scale(self.tv_w, C, H, W) * float(tv_ref.raw_sum(self.x0))
            items = C * H * -(-W // _lib.TV_VEC)
            chain = 2 * _lib.TV_VEC * -(-items // (_lib.TV_LOSS_PARTS * _lib.TV_THREADS)) + 2 + 6 + 16
            total, e_total = total + term, e_total + gamma(chain + 2) * term + U * (total + term)
        if self.lap_w:                       # one kind-2 row per pool behind TV's, added in index order, one fp32 add each
            at = n_style + len(s.content_taps) + (1 if self.tv_w else 0)
            for k, p in enumerate(eng.lap_pools):
                C, Hp, Wp = eng.lap_resid[k].shape
                name = f"lap resid p{p}"
                want = lap_ref.resid(self.x0.float(), eng.lap_targets[k].detach().cpu().numpy(), p, np.float32)
                self.accept("lap residual", name, eng.lap_resid[k].detach().cpu().double(),
                            Iv.of(torch.from_numpy(want).double()), torch.float32)
                scale = float(scale_row[at + k])
                if scale != core_model.lap_scale(self.lap_w, C, Hp, Wp):
                    self.fail(f"scale lap p{p}", f"combine scale {scale!r} is not {core_model.lap_scale(self.lap_w, C, Hp, Wp)!r}")
                term = scale * lap_ref.raw_sum(eng.lap_resid[k].detach().cpu().numpy())
                depth = lap_ref.partial_sum_depth(C, Hp, Wp, _lib.LAP_TILE_H, _lib.LAP_TILE_W, _lib.LAP_LOSS_PARTS)
                total, e_total = total + term, e_total + gamma(depth + 2) * term + U * (total + term)
        got = eng.scores.detach().cpu().double()
        for i, (nm, r, e) in enumerate((("style", style, e_style), ("content", content, e_content), ("total", total, e_total))):
            self.accept("score", f"score {nm}", got[i:i + 1], Iv.of(torch.tensor([r], dtype=torch.float64), e), torch.float32)

    # -- backward
    def stage(self, prev: Iv | None, r, A, k: int, u: float = U) -> Iv:
        """One launch onto a gradient: store ``r`` or, onto a stored (rounded) ``prev``, accumulate."""
        if prev is None:
            return Iv.of(r, gamma(k, u) * A)
        p = prev.rounded(self.T)
        e = gamma(k + 1, u) * (A + p.absmax())
        e = torch.where(A == 0, torch.zeros_like(e), e)       # a sum of exact zeros adds an exact zero
        return Iv(p.r + r, p.lo + r - e, p.hi + r + e)

    def backward(self) -> None:
        nodes = self.nodes
        routed = {id(nd.route) for nd in nodes if nd.route is not None}
        for nd in nodes:
            b = nd.dst
            if id(nd) in routed:
                continue                     # its gradient only ever exists in the registers of the routing dgrad
            name = f"grad L{nd.layer:02d} {nd.kind}"
            act = nchw(b.act)
            consumer = next((c for c in nodes if c.src is b), None)
            stages = 0
            iv: Iv | None = None
            for t in b.taps:
                if t.kind not in TAP_KINDS:
                    raise RuntimeError(f"{name}: no rule for a tap of kind {t.kind!r}")
            pre = [t for t in b.taps if t.kind == "content" and t.grad_fused and self.gout is None]
            for tap in pre:
                iv = self.stage(iv, *self.tap_term(tap))
                stages += 1
            in_dgrad = None
            if consumer is not None:
                stages += 1
                # the ReLU mask of this buffer rides in its consumer's launch (staged ReLU, or a fused ReLU nobody taps)
                if consumer.kind == "conv":
                    mask = consumer.relu_in or (b.relu_fused and not b.taps)
                    r, A, k, u = self.dgrad(consumer)
                    if mask:
                        r, A = r * (act > 0), A * (act > 0)
                    in_dgrad = consumer.gram
                    if in_dgrad is not None and self.s.guide:
                        raise RuntimeError(f"{name}: a Gram term in the dgrad of L{consumer.layer:02d} under guidance has no rule")
                    if in_dgrad is not None:
                        tr, tA, tk, _ = self.tap_term(in_dgrad)
                        r, A, k = r + tr, A + tA, k + tk
                    iv = self.stage(iv, r, A, k, u)
                elif consumer.kind == "pool":
                    mask = b.relu_fused and not b.taps
                    router = next((c for c in nodes if c.route is consumer), None)
                    if router is not None:        # pooled gradient = storage-rounded dgrad, in registers, then moved
                        r, A, k, u = self.dgrad(router)
                        dy = Iv.of(r, gamma(k, u) * A).rounded(self.T)
                    else:
                        dy = Iv.of(nchw(consumer.dst.grad))
                    if consumer.idx is not None:
                        code = nchw(consumer.idx).long()
                        q, live = code & 3, (code & 4) != 0
                    else:
                        best, q = first_max(act)
                        live = best > 0
                    if mask:
                        dy = dy.map(lambda v: torch.where(live, v, torch.zeros_like(v)))
                    g = dy.map(lambda v: scatter_pool(v, q, b.H, b.W))
                    if iv is not None:             # routed value + the stored gradient: one fp32 add
                        p = iv.rounded(self.T)
                        e = gamma(1) * (g.absmax() + p.absmax())
                        g = Iv(p.r + g.r, p.lo + g.lo - e, p.hi + g.hi + e)
                    iv = g
                elif consumer.kind == "avgpool":
                    dy = nchw(consumer.dst.grad)
                    Hp, Wp = dy.shape[2], dy.shape[3]
                    v = torch.zeros_like(act)
                    v[:, :, :2 * Hp, :2 * Wp] = (0.25 * dy).repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
                    if consumer.relu_in or (b.relu_fused and not b.taps):
                        v = torch.where(act > 0, v, torch.zeros_like(v))
                    g = Iv.of(v)
                    if iv is not None:             # one fp32 add inside the pooled range, nothing in the dropped rows / columns
                        p = iv.rounded(self.T)
                        e = gamma(1) * (v.abs() + p.absmax())
                        e[:, :, 2 * Hp:, :], e[:, :, :, 2 * Wp:] = 0.0, 0.0
                        g = Iv(p.r + v, p.lo + v - e, p.hi + v + e)
                    iv = g
                elif consumer.kind == "relu":      # a materialised ReLU
                    g = nchw(consumer.dst.grad) * (act > 0)
                    iv = self.stage(iv, g, g.abs(), 0)
                else:
                    raise RuntimeError(f"{name}: no rule for a consumer of kind {consumer.kind!r}")
            for tap in b.taps:
                if tap is in_dgrad or any(tap is t for t in pre):
                    continue
                for term in self.tap_terms(tap):
                    iv = self.stage(iv, *term)
                    stages += 1
            if iv is None:
                raise RuntimeError(f"{name}: activation without any gradient contribution")
            if b.relu_fused and b.taps:           # taps see relu(z): the summed gradient is masked once, in place
                iv = iv.rounded(self.T).map(lambda v: v * (act > 0))
            if stages > 1:
                self.rep.multi_stage.append(name)
            kind = ("gradient (moved)" if consumer is not None and consumer.kind != "conv" and stages == 1
                    and not any(c.route is consumer for c in nodes) else "gradient")
            if consumer is not None and consumer.kind == "avgpool":
                kind = "gradient (avgpool)"
            self.accept(kind, name, nchw(b.grad), iv)
        # the image gradient: the first layer's dgrad (fp32 output), then the total-variation term accumulated
        first = nodes[0]
        r, A, k, u = self.dgrad(first)
        iv = Iv.of(r, gamma(k, u) * A)
        if self.tv_w:
            C, H, W = self.x0.shape[1:]
            coef = core_model.tv_coef(self.tv_w, C, H, W)
            t = (coef * tv_ref.neighbour_sum(self.x0)).reshape(r.shape)
            e_t = (8 * U * coef * tv_ref.abs_difference_sum(self.x0)).reshape(r.shape)     # test_gpu_tv_model's bound
            p = iv.rounded(torch.float32)
            e = e_t + U * (t.abs() + e_t + p.absmax())
            iv = Iv(p.r + t, p.lo + t - e, p.hi + t + e)
        if self.lap_w:
            Ci, H, W = self.x0.shape[1:]
            for k, pool in enumerate(self.eng.lap_pools):
                r64 = self.eng.lap_resid[k].detach().cpu().double().numpy()
                _, Hp, Wp = r64.shape
                coef = core_model.lap_coef(self.lap_w, Ci, Hp, Wp, pool)
                g64 = lap_ref.stencil(r64)
                dg = lap_ref._stencil_bound(r64, np.zeros_like(r64))
                dout = abs(coef) * dg + U * abs(coef) * (np.abs(g64) + dg)
                t, e_t = torch.zeros(1, Ci, H, W, dtype=torch.float64), torch.zeros(1, Ci, H, W, dtype=torch.float64)
                t[0, :, :Hp * pool, :Wp * pool] = torch.from_numpy(lap_ref.upsample(coef * g64, pool))
                e_t[0, :, :Hp * pool, :Wp * pool] = torch.from_numpy(lap_ref.upsample(dout, pool))
                cover = torch.zeros(1, Ci, H, W, dtype=torch.bool)
                cover[0, :, :Hp * pool, :Wp * pool] = True
                p = iv.rounded(torch.float32)
                e = torch.where(cover, e_t + U * (t.abs() + e_t + p.absmax()), torch.zeros_like(e_t))
                iv = Iv(p.r + t, p.lo + t - e, p.hi + t + e)
        self.accept("image gradient", "image grad", self.x_grad.detach().cpu().double().reshape(r.shape), iv, torch.float32)


def check_step(engine, x0: torch.Tensor, *, style_w: float, content_w: float, x_grad: torch.Tensor, gout=None,
               tv_w: float = 0.0, lap_w: float = 0.0, layer_w=None, record=None, case: str = "step") -> Report:
    """Check every tensor one evaluated step left in ``engine``'s buffers (see the module docstring).

    ``x0``: the image of that step.  ``x_grad``: the image gradient it produced.  ``gout`` (autograd path,
    ``model(x)`` + ``.backward()``): the upstream coefficient of every loss term, style terms first - each tap's term
    is scaled by its own, the scores are the unweighted sums, and ``style_w`` / ``content_w`` are not used.
    ``lap_w``: the weight of the Laplacian terms (pools: ``engine.lap_pools``).  ``layer_w``: one weight per style tap, in tap
    order (``None``: all 1).  Guidance and the pooling kind are read from the engine (``engine.guide``, the node kinds).
    ``record``: ``tests.conftest.record_parity`` - one row per tensor kind.  Raises :class:`LayerwiseMismatch`."""
    s = engine.sched
    if s.halo:
        raise RuntimeError("check_step: row strips are out of scope")
    for nd in s.nodes:
        if nd.kind not in NODE_KINDS:
            raise RuntimeError(f"check_step: no rule for node kind {nd.kind!r} (layer {nd.layer})")
        for t in nd.dst.taps:
            if t.kind not in TAP_KINDS:
                raise RuntimeError(f"check_step: no rule for tap kind {t.kind!r} (layer {nd.layer})")
    if lap_w and not engine.lap_pools:
        raise RuntimeError(f"check_step: lap_w = {lap_w:g} on an engine without lap_pools")
    if bool(s.guide) != (engine.guide is not None) or (s.guide and engine.guide.n != s.guide):
        raise RuntimeError(f"check_step: schedule with guide = {s.guide} on an engine whose guide is {engine.guide!r}")
    if s.guide:
        for t in s.style_taps:
            if t.regions is None or t.labels is None or t.slabs is None or len(t.regions) != s.guide:
                raise RuntimeError(f"check_step: guided schedule without attached regions (style tap {t.order})")
    if gout is not None and (s.guide or lap_w or layer_w is not None):
        raise RuntimeError("check_step: gout (the autograd path) has no rule together with guidance, layer_w or lap_w")
    if layer_w is not None:
        layer_w = tuple(float(v) for v in layer_w)
        if len(layer_w) != len(s.style_taps):
            raise RuntimeError(f"check_step: {len(layer_w)} layer weights for {len(s.style_taps)} style taps")
    seen: dict = {}
    for nd in s.nodes:
        g = nd.dst.grad
        if g is None:
            raise RuntimeError("check_step: the engine holds no evaluated step (no gradients allocated)")
        if g.numel() == 0:
            continue
        if getattr(s, "_grad_slab_of", None) or g.data_ptr() in seen:
            raise RuntimeError("check_step: gradients share slabs - only the last writer of each survives "
                               "(build the engine with STV_GRAD_ARENA=0)")
        seen[g.data_ptr()] = nd
    if not all(nd.dst.stored for nd in s.nodes):
        raise RuntimeError("check_step: a pre-pool map is not stored (build the engine with STV_SKIP_PREPOOL=0)")
    rep = Report()
    chk = _Checker(engine, x0, style_w, content_w, gout, x_grad, tv_w, case, rep, lap_w, layer_w)
    chk.forward()
    chk.losses()
    chk.backward()
    if record is not None:
        for kind, (ratio, second, n, tensors) in rep.rows.items():
            record(case, f"{kind}: worst (|got - r| - ulp/2) / e", ratio, 1.0,
                   f"{tensors} tensors, {n} elements, {second} bf16 elements took the second admissible value")
        if rep.multi_stage:
            record(case, "gradients formed by several launches", float(len(rep.multi_stage)), float("nan"),
                   "interval carried through each storage rounding: " + ", ".join(rep.multi_stage))
    if rep.failures:
        raise LayerwiseMismatch(case, rep.failures)
    return rep
