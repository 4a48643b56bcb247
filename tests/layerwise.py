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

Precondition: one tensor per gradient and every activation stored (STV_GRAD_ARENA=0, STV_SKIP_PREPOOL=0).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import torch
import torch.nn.functional as F

from style_transfer_visualizer_amd import _lib, core_model, plan, synthetic
from tests import bf16x3_emul as emul
from tests import tv_ref

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
    def __init__(self, engine, x0, style_w, content_w, gout, x_grad, tv_w, case, report) -> None:
        self.eng, self.s = engine, engine.sched
        self.nodes = self.s.nodes
        self.x0 = x0.detach().cpu().double()
        self.mode = mode_of(engine)
        self.T = engine.dtype
        self.gout = None if gout is None else [float(v) for v in torch.as_tensor(gout).detach().float().cpu()]
        self.style_w, self.content_w = (1.0, 1.0) if gout is not None else (float(style_w), float(content_w))
        self.x_grad, self.tv_w, self.case, self.rep = x_grad, float(tv_w), case, report
        self.u_mm = U_BF16_MFMA if self.mode != "fp32" else U

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

    def tap_term(self, tap) -> tuple[torch.Tensor, torch.Tensor, int, float]:
        """The gradient term of one tap on its buffer: (r, A, K, u)."""
        fb = nchw(tap.buf.act)
        if tap.kind == "style":
            s_mat = self.seed_mat(tap)
            r, A, m = _bilinear(lambda a, c: torch.einsum("nk,bkhw->bnhw", c.double(), a.double()), fb, s_mat,
                                self.mode == "bf16x3")
            return r, A, tap.buf.C * m, (self.u_mm if self.mode != "fp32" else U)
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
            else:
                self.accept("relu forward", name, nchw(nd.dst.act), Iv.of(nchw(nd.src.act).clamp_min(0.0)))

    # -- loss head
    def losses(self) -> None:
        s, eng = self.s, self.eng
        n_style = len(s.style_taps)
        x3 = self.mode == "bf16x3"
        terms, errs = [], []
        for tap in s.style_taps:
            C = tap.buf.C
            f = nchw(tap.buf.act).reshape(C, -1)
            n = f.shape[1]
            R, A, m = _bilinear(lambda a, c: a.double() @ c.double().t(), f, f, x3)
            e_R = gamma(n * m + 1, self.u_mm) * A
            norm32 = torch.tensor(float(C * n), dtype=torch.float32)
            norm = float(norm32)
            G = R.clamp(max=plan.GRAM_CLAMP_MAX) / norm
            T = tap.target.detach().cpu().double()
            d = G - T
            e_G = e_R / norm + U * G.abs()
            e_d = e_G + U * (d.abs() + e_G)
            scale = float(eng.scale[tap.order])
            sq = float((d * d).sum())
            e_sum = float((2 * d.abs() * e_d + e_d * e_d).sum()) + gamma(C * C + tap.parts_cnt + 1) * sq
            terms.append(scale * sq)
            errs.append(scale * e_sum + U * scale * sq)
            # the seed S = kk * [R <= clamp] * (G - T), kk = coef * 4 / (C * C * norm) (* upstream coefficient), in fp32
            c32 = torch.tensor(float(C), dtype=torch.float32)
            coef = self.style_w if self.gout is None else 1.0
            kk = (f32_scalar(coef) * 4.0) / (c32 * c32 * norm32)
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
        c_terms, c_errs = [], []
        for tap in s.content_taps:
            d = nchw(tap.buf.act) - nchw(tap.target)
            n = d.numel()
            scale = float(eng.scale[n_style + tap.order])
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
                else:                              # a materialised ReLU
                    g = nchw(consumer.dst.grad) * (act > 0)
                    iv = self.stage(iv, g, g.abs(), 0)
            for tap in b.taps:
                if tap is in_dgrad or any(tap is t for t in pre):
                    continue
                iv = self.stage(iv, *self.tap_term(tap))
                stages += 1
            if iv is None:
                raise RuntimeError(f"{name}: activation without any gradient contribution")
            if b.relu_fused and b.taps:           # taps see relu(z): the summed gradient is masked once, in place
                iv = iv.rounded(self.T).map(lambda v: v * (act > 0))
            if stages > 1:
                self.rep.multi_stage.append(name)
            kind = ("gradient (moved)" if consumer is not None and consumer.kind != "conv" and stages == 1
                    and not any(c.route is consumer for c in nodes) else "gradient")
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
        self.accept("image gradient", "image grad", self.x_grad.detach().cpu().double().reshape(r.shape), iv, torch.float32)


def check_step(engine, x0: torch.Tensor, *, style_w: float, content_w: float, x_grad: torch.Tensor, gout=None,
               tv_w: float = 0.0, record=None, case: str = "step") -> Report:
    """Check every tensor one evaluated step left in ``engine``'s buffers (see the module docstring).

    ``x0``: the image of that step.  ``x_grad``: the image gradient it produced.  ``gout`` (autograd path,
    ``model(x)`` + ``.backward()``): the upstream coefficient of every loss term, style terms first - each tap's term
    is scaled by its own, the scores are the unweighted sums, and ``style_w`` / ``content_w`` are not used.
    ``record``: ``tests.conftest.record_parity`` - one row per tensor kind.  Raises :class:`LayerwiseMismatch`."""
    s = engine.sched
    if s.halo:
        raise RuntimeError("check_step: row strips are out of scope")
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
    chk = _Checker(engine, x0, style_w, content_w, gout, x_grad, tv_w, case, rep)
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
