"""The layer-wise checker (tests/layerwise.py) proved without a GPU.

A stand-in executor runs the op lists a GPU engine builds (device-form schedules on host tensors,
``assume_device=True``) with torch-CPU arithmetic in the storage precision: every op is interpreted from its own
fields, flags and operands (``op.refs``) - it does not read the schedule's decision fields, so it is independent of the
checker's per-node reading - and is applied to the stand-in's own previous tensors, rounding to bf16 where the
kernels round.  Asserted:

* ``check_step`` passes on the stand-in for every tap layout x precision of the GPU matrix, in two summation orders
  (channels as they are / reversed): the reference arithmetic alone stays inside the derived intervals;
* every mutation of the stand-in (two storage ulps on one element, a dropped bias, a mask from the wrong buffer, a
  lost ACCUM, a tap term applied twice, a route to the wrong window position, two upstream coefficients swapped, a
  pre-written content gradient overwritten by the pooling backward routed onto it) fails, naming the mutated tensor;
* the schedule's decision fields are consulted per node: where a field takes both values in one schedule, reading it
  as one global value fails.

The same three for the structures of ``lw.STEP_CASES`` - average pooling, spatial guidance, style layer weights, the
Laplacian terms.  The stand-in has ``avgpool_fwd`` / ``avgpool_bwd`` (the header's summation order; RELU_IN, MASK, ACCUM),
``mask_split`` and ``lap`` (LOSS and GRAD); its Gram finish resolves a chain over ``s.all_chains()`` and divides by the op's
own norm; ``set_targets`` forms the per-region targets by the float64 definition of tests/guidance_ref.py and the pooled
Laplacian targets; ``fused_step`` builds the op list as ``_Engine.loss_and_grad`` does.  Mutations: pairwise summation in
the pool, a lost or misplaced mask, a lost ACCUM and a written odd tail in its backward; label 255 copied into slab 0 and
two slabs swapped; a region norm from the parent's pixel count (in the op, and in the schedule), two region weights
swapped, the second region's product without ACCUM, a region's product applied twice, the ReLU mask behind the first term;
a layer weight in the seed or in the scale only; a Laplacian GRAD launch without ACCUM, in front of the storing dgrad, with
the other pool's coefficient, or writing a pixel outside the cells.  The refusals of ``check_step`` raise.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from style_transfer_visualizer_amd import _lib, core_model, guidance, ops, plan, synthetic
from tests import bf16x3_emul as emul
from tests import guidance_ref, lap_ref
from tests import layerwise as lw

CPU = torch.device("cpu")
STYLE_W, CONTENT_W = 1e5, 1.0
LAYOUTS, NARROW_CFG, NARROW_LAYOUT, assert_narrow_branches = lw.LAYOUTS, lw.NARROW_CFG, lw.NARROW_LAYOUT, lw.assert_narrow_branches
PRECISIONS = {"fp32": (torch.float32, False), "bf16": (torch.bfloat16, False), "bf16x3": (torch.float32, True)}
CHECK_ENV = {"STV_GRAD_ARENA": "0", "STV_SKIP_PREPOOL": "0"}


@functools.cache
def vgg_layers(cfg: tuple = synthetic.VGG19_CFG, pooling: str = "max") -> list:
    vgg = core_model.build_vgg_features(lw.biased_weights(cfg), cfg).eval()
    return list(core_model.replace_pooling(vgg, pooling).children())


def make_guide(regions: int, H: int, W: int):
    return guidance.make_guide(regions, list(lw.REGION_WEIGHTS[regions]), *lw.guide_labels(regions, H, W))


def make_engine(monkeypatch, layout, precision: str, H: int, W: int, cfg: tuple = synthetic.VGG19_CFG, *, pooling: str = "max",
                regions: int = 0, lap_pools: tuple = (), **env):
    for k, v in {**CHECK_ENV, **env}.items():
        monkeypatch.setenv(k, v)
    dtype, split = PRECISIONS[precision]
    style_at, content_at = layout
    layers = vgg_layers(cfg, pooling)[:max(style_at + content_at) + 1]
    extra = {"lap_pools": lap_pools} if lap_pools else {}
    if regions:      # (the guide reaches the engine as it does from the model)
        extra["guide"] = make_guide(regions, H, W)
    return core_model._Engine(layers, sorted(style_at), sorted(content_at), H, W, dtype, CPU, split=split, assume_device=True, **extra)


def cpu_loss_combine(parts, table, scale, style_w, content_w, losses, scores) -> None:
    """``ops.loss_combine`` for ``engine.region_losses()`` on host tensors: the partials added in double, one fp32 result."""
    for i, (o, c, _) in enumerate(table.tolist()):
        losses[i] = (parts[int(o):int(o) + int(c)].double().sum() * scale[i].double()).float()


# ------------------------------------------------------------------------------------------------ the stand-in executor
_OP_NAMES = {getattr(_lib, n): n[3:].lower() for n in dir(_lib) if n.startswith("OP_")}


def hwc(t: torch.Tensor) -> torch.Tensor:
    """NHWC buffer -> [1,C,H,W] fp32."""
    return t.detach().float().permute(2, 0, 1).unsqueeze(0)


def put(dst: torch.Tensor, nchw: torch.Tensor, accum: bool = False) -> None:
    v = nchw[0].permute(1, 2, 0)
    dst.copy_(v + dst.float() if accum else v)        # one fp32 add, one rounding to storage


def conv_f(a: torch.Tensor, w: torch.Tensor, rev: bool) -> torch.Tensor:
    return F.conv2d(a.flip(1), w.flip(1), padding=1) if rev else F.conv2d(a, w, padding=1)


def conv_b(a: torch.Tensor, w: torch.Tensor, rev: bool) -> torch.Tensor:
    return F.conv_transpose2d(a.flip(1), w.flip(0), padding=1) if rev else F.conv_transpose2d(a, w, padding=1)


def pool_pos(act: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """(maximum, position 2*dy+dx of the first maximum in scan order) of the 2x2 windows of [1,C,H,W] - by max_pool2d."""
    best, flat = F.max_pool2d(act, 2, 2, return_indices=True)
    W = act.shape[3]
    return best, ((flat // W) % 2) * 2 + (flat % W) % 2


def unpool(dy: torch.Tensor, q: torch.Tensor, H: int, W: int) -> torch.Tensor:
    out = torch.zeros(1, dy.shape[1], H, W)
    for k in range(4):
        out[:, :, (k >> 1):2 * dy.shape[2]:2, (k & 1):2 * dy.shape[3]:2] = dy * (q == k)
    return out


class StandIn:
    """Interprets ``StvOp`` lists on host tensors.  ``reverse``: sum every convolution over reversed channels.
    ``mutate`` = (kind, key): one deliberate error (``key``: the tensor the erring op writes, or a layer number)."""

    def __init__(self, eng, *, reverse: bool = False, mutate: tuple | None = None) -> None:
        self.eng, self.s, self.rev = eng, eng.sched, reverse
        self.bf16, self.x3 = eng.dtype == torch.bfloat16, eng.split
        self.mutate = mutate or (None, None)
        self.hits = 0
        self.products_on: dict = {}          # gradient buffer -> 1x1 products launched onto it so far (this step)
        self.lap_w, self.layer_w = 0.0, None

    def mut(self, kind: str, key) -> bool:
        if self.mutate[0] == kind and (self.mutate[1] is key or (not isinstance(key, torch.Tensor) and self.mutate[1] == key)):
            self.hits += 1
            return True
        return False

    def product(self, fn, a: torch.Tensor, w: torch.Tensor, split: bool) -> torch.Tensor:
        if not split:
            return fn(a, w, self.rev)
        (ah, al), (wh, wl) = emul.split(a), emul.split(w)
        ah, al, wh, wl = ah.float(), al.float(), wh.float(), wl.float()
        return fn(ah, wh, self.rev) + fn(ah, wl, self.rev) + fn(al, wh, self.rev)

    def conv_w(self, nd) -> torch.Tensor:
        w = self.eng.layers[nd.layer].weight.detach().float()
        return w.bfloat16().float() if (self.bf16 and nd.kind == "conv") else w

    def run(self, op_list: list) -> None:
        for op in op_list:
            getattr(self, "op_" + _OP_NAMES[int(op.op)])(op, op.refs)

    # -- forward
    def op_conv_first_fwd(self, op, r) -> None:
        nd = self.s.nodes[0]
        z = self.product(conv_f, r["p0"].float(), self.conv_w(nd), self.bf16)      # bf16: both operands split in two terms
        if "p2" in r and not self.mut("drop_bias", nd.layer):
            z = z + r["p2"].view(1, -1, 1, 1)
        put(r["q0"], z)

    def op_conv(self, op, r) -> None:
        w = r["p1"]
        nd = next((n for n in self.s.nodes if n.kind == "conv" and (n.wf is w or n.wb is w)), None)
        if nd is None:
            return self.tap_product(op, r)
        if nd.wb is w:
            return self.dgrad(op, r, nd)
        a = hwc(r["p0"])
        if op.flags & _lib.RELU_IN:
            a = a.clamp_min(0.0)
        z = self.product(conv_f, a, self.conv_w(nd), self.x3)
        if "p2" in r and not self.mut("drop_bias", nd.layer):
            z = z + r["p2"].view(1, -1, 1, 1)
        if op.flags & _lib.RELU_OUT:
            z = z.clamp_min(0.0)
        if not op.flags & _lib.POOL_ONLY:
            put(r["q0"], z)
        if "q1" in r:                        # the pool in the epilogue works on the values as stored
            best, q = pool_pos(z.to(r["q1"].dtype).float())
            put(r["q1"], best)
            if "q2" in r:
                put(r["q2"], (q + 4 * (best > 0)).float())

    def op_pool_fwd(self, op, r) -> None:
        put(r["q0"], F.max_pool2d(hwc(r["p0"]), 2, 2))

    def op_relu_fwd(self, op, r) -> None:
        put(r["q0"], hwc(r["p0"]).clamp_min(0.0))

    def op_avgpool_fwd(self, op, r) -> None:
        x = r["p0"].detach().float()
        if op.flags & _lib.RELU_IN:
            x = x.clamp_min(0.0)
        Hp, Wp = int(op.H) // 2, int(op.W) // 2
        a, b = x[0:2 * Hp:2, 0:2 * Wp:2], x[0:2 * Hp:2, 1:2 * Wp:2]
        c, d = x[1:2 * Hp:2, 0:2 * Wp:2], x[1:2 * Hp:2, 1:2 * Wp:2]
        # the header's order, every fp32 sum rounded on its own; one rounding to storage
        total = ((a + b) + (c + d)) if self.mut("avg_pairwise", r["q0"]) else (((a + b) + c) + d)
        r["q0"].copy_(total * 0.25)

    def op_mask_split(self, op, r) -> None:
        src, out = r["p0"], r["q0"]
        lab = r["p1"].reshape(src.shape[0], src.shape[1], 1).long()
        if self.mut("label255_into_slab0", out):
            lab = torch.where(lab == 255, torch.zeros_like(lab), lab)
        swap = self.mut("swap_slabs", out)
        for k in range(int(op.cout)):
            want = {0: 1, 1: 0}.get(k, k) if swap else k
            out[k].copy_(torch.where(lab == want, src, torch.zeros_like(src)))

    def op_lap(self, op, r) -> None:
        p, H, W = int(op.cout), int(op.H), int(op.W)
        Hp, Wp = H // p, W // p
        if int(op.taps) == _lib.LAP_LOSS:
            res = lap_ref.resid(r["p0"], r["p1"].numpy(), p, np.float32)
            r["q0"].copy_(torch.from_numpy(res))
            r["q1"][:_lib.LAP_LOSS_PARTS] = 0.0
            r["q1"][0] = float((res * res).sum(dtype=np.float32))
            return
        assert int(op.taps) == _lib.LAP_GRAD
        coef = float(op.f0)
        if self.mut("lap_swap_coef", p):
            q = next(v for v in self.eng.lap_pools if v != p)
            coef = core_model.lap_coef(self.lap_w, int(op.cin), H // q, W // q, q)
        accum = bool(op.flags & _lib.ACCUM) and not self.mut("lap_lost_accum", p)
        out = lap_ref.grad_accum(r["q0"].numpy(), r["q2"], p, coef, accum=accum)
        if self.mut("lap_margin", p):
            out[0, Hp * p, 0] += np.float32(1e-3)
        r["q2"].copy_(torch.from_numpy(out).reshape(r["q2"].shape))

    # -- loss head
    def op_gram_partial(self, op, r) -> None:
        pass                                 # (the raw Gram is summed where it is finished, from the same activation)

    def finish(self, tap, *, norm: float, target, loss_part, sgrad, coef: float, coef_dev) -> None:
        """``tap``: the chain the op's partials belong to (its ``buf`` is the region's slab under guidance); ``norm``: the op's."""
        C = tap.buf.C
        f = tap.buf.act.detach().float().reshape(-1, C)
        n = f.shape[0]
        if self.mut("norm_parent", sgrad):
            norm = float(C * n)
        if self.mut("swap_lambda", sgrad):
            lam = self.eng.guide.weights
            k = tap.order % len(lam)
            coef = coef * lam[(k + 1) % len(lam)] / lam[k]
        if self.mut("seed_without_w", sgrad):
            coef = coef / self.layer_w[tap.order]
        if self.x3:
            (h, lo) = emul.split(f)
            h, lo = h.float(), lo.float()
            R = h.t() @ h + h.t() @ lo + lo.t() @ h
        else:
            R = f.t() @ f
        norm = torch.tensor(norm, dtype=torch.float32)
        G = R.clamp(max=plan.GRAM_CLAMP_MAX) / norm
        if target is None:
            return
        d = G - target
        if loss_part is not None:
            loss_part[:tap.parts_cnt] = 0.0
            loss_part[0] = (d * d).sum()
        if sgrad is not None:
            c32 = torch.tensor(float(C), dtype=torch.float32)
            kk = (torch.tensor(coef, dtype=torch.float32) * 4.0) / (c32 * c32 * norm)
            if coef_dev is not None:
                kk = kk * coef_dev[0]
            sgrad.copy_(torch.where(R <= plan.GRAM_CLAMP_MAX, kk * d, torch.zeros_like(d)).reshape(sgrad.shape))

    def op_gram_finish(self, op, r) -> None:
        tap = next(t for t in self.s.all_chains() if t.partials is r["p0"])
        self.finish(tap, norm=float(op.f1), target=r.get("p1"), loss_part=r.get("q1"), sgrad=r.get("q2"), coef=float(op.f2), coef_dev=r.get("p2"))

    def op_gram_multi(self, op, r) -> None:
        by_ptr = {t.data_ptr(): t for t in r.values() if isinstance(t, torch.Tensor)}
        for e in list(r["p0"])[:int(op.n)]:
            tap = next(t for t in self.s.all_chains() if t.partials is not None and t.partials.data_ptr() == e.partials)
            self.finish(tap, norm=float(e.norm), target=by_ptr.get(e.target), loss_part=by_ptr.get(e.loss_part), sgrad=by_ptr.get(e.sgrad),
                        coef=float(e.coef), coef_dev=by_ptr.get(e.coef_dev))

    def op_content_loss(self, op, r) -> None:
        d = r["p0"].float() - r["p1"].float()
        r["q0"][:_lib.CONTENT_LOSS_PARTS] = 0.0
        r["q0"][0] = (d * d).sum()
        if "q1" in r:
            k = torch.tensor(float(op.f0), dtype=torch.float32) * (torch.tensor(2.0) / torch.tensor(float(op.n)))
            r["q1"].copy_(k * d)

    def op_loss_combine(self, op, r) -> None:
        parts, table, scale = r["p0"], r["p1"], r["p2"]
        scale = scale.clone()
        for i in range(len(scale)):
            if self.mut("scale_without_w", i):
                scale[i] = scale[i] / self.layer_w[i]
        terms = [(parts[int(o):int(o) + int(c)].double().sum() * scale[i].double()).float() for i, (o, c, _) in enumerate(table.tolist())]
        kinds = [int(k) for _, _, k in table.tolist()]
        r["q0"][:len(terms)] = torch.stack(terms)
        style = sum((t for t, k in zip(terms, kinds) if k == 0), torch.tensor(0.0))
        content = sum((t for t, k in zip(terms, kinds) if k == 1), torch.tensor(0.0))
        total = torch.tensor(float(op.f0)) * style + torch.tensor(float(op.f1)) * content
        for t, k in zip(terms, kinds):
            if k == 2:
                total = total + t
        r["q1"][:3] = torch.stack([style, content, total])

    # -- backward
    def tap_product(self, op, r) -> None:
        """dF = F . S as a 1x1 convolution."""
        C = int(op.cin)
        term = self.product(lambda a, w, rev: conv_f_1x1(a, w, rev), hwc(r["p0"]), r["p1"].detach().float().reshape(C, C), self.x3)
        accum = bool(op.flags & _lib.ACCUM) and not self.mut("lost_accum", r["q0"])
        put(r["q0"], term, accum)
        if self.mut("tap_twice", r["q0"]) or self.mut("region_twice", r["p0"]):
            put(r["q0"], term, True)
        done = self.products_on[id(r["q0"])] = self.products_on.get(id(r["q0"]), 0) + 1
        if done == 1 and self.mut("mask_early", r["q0"]):      # the in-place ReLU mask behind the FIRST term (op_relu_bwd skips it)
            act = next(n.dst.act for n in self.s.nodes if n.dst.grad is r["q0"])
            r["q0"].copy_(r["q0"].float() * (act.float() > 0))

    def dgrad(self, op, r, nd) -> None:
        g = self.product(conv_b, hwc(r["p0"]), self.conv_w(nd), self.x3)
        if op.flags & _lib.POOL_ROUTE:
            code = hwc(r["p2"]).long()
            q = code & 3
            if self.mut("wrong_route", r["q1"]):
                q = (q + 1) & 3
            g = g.to(r["q1"].dtype).float()                # the pooled gradient, rounded to storage, then moved
            if op.flags & _lib.MASK:
                g = g * ((code & 4) != 0)
            return put(r["q1"], unpool(g, q, r["q1"].shape[0], r["q1"].shape[1]))
        if op.flags & _lib.MASK:
            ref = r["p3"]
            if self.mut("wrong_mask", r["q0"]):
                ref = next(n.dst.act for n in self.s.nodes if n.dst.act.shape == ref.shape and n.dst.act is not ref)
            g = g * (hwc(ref) > 0)
        if "q3" in r:                                      # the Gram term of the tap on this buffer, same launch
            C = int(op.n)
            g = g + self.product(lambda a, w, rev: conv_f_1x1(a, w, rev), hwc(r["q2"]), r["q3"].detach().float().reshape(C, C), self.x3)
        put(r["q0"], g, bool(op.flags & _lib.ACCUM) and not self.mut("lost_accum", r["q0"]))

    def op_content_grad(self, op, r) -> None:
        k = torch.tensor(float(op.f0), dtype=torch.float32)
        if "p2" in r:
            k = k * r["p2"][0]
        k = k * (torch.tensor(2.0) / torch.tensor(float(op.n)))
        term = k * (r["p0"].float() - r["p1"].float())
        accum = bool(op.flags & _lib.ACCUM) and not self.mut("lost_accum", r["q0"])
        r["q0"].copy_(term + r["q0"].float() if accum else term)
        if self.mut("tap_twice", r["q0"]):
            r["q0"].copy_(term + r["q0"].float())

    def op_pool_bwd(self, op, r) -> None:
        dx = r["q0"]
        H, W = dx.shape[0], dx.shape[1]
        dy = hwc(r["p1"])
        if op.flags & _lib.POOL_IDX:
            code = hwc(r["p0"]).long()
            q, live = code & 3, (code & 4) != 0
        else:
            best, q = pool_pos(hwc(r["p0"]))
            live = best > 0
        if self.mut("wrong_route", dx):
            q = (q + 1) & 3
        if op.flags & _lib.MASK:
            dy = dy * live
        accum = bool(op.flags & _lib.ACCUM) and not (self.mut("lost_accum", dx) or self.mut("route_overwrites", dx))
        put(dx, unpool(dy, q, H, W), accum)

    def op_avgpool_bwd(self, op, r) -> None:
        dx = r["q0"]
        H, W = int(op.H), int(op.W)
        Hp, Wp = H // 2, W // 2
        v = torch.zeros(H, W, int(op.cin))
        v[:2 * Hp, :2 * Wp] = (0.25 * r["p1"].float()).repeat_interleave(2, dim=0).repeat_interleave(2, dim=1)
        if op.flags & _lib.MASK and not self.mut("lost_mask", dx):
            ref = r["p0"]
            if self.mut("wrong_mask", dx):
                ref = next(n.dst.act for n in self.s.nodes if n.dst.act.shape == ref.shape and n.dst.act is not ref)
            v = torch.where(ref.float() > 0, v, torch.zeros_like(v))
        if bool(op.flags & _lib.ACCUM) and not self.mut("lost_accum", dx):
            out = dx.float().clone()                       # the rows and columns the floor drops stay as they are
            out[:2 * Hp, :2 * Wp] += v[:2 * Hp, :2 * Wp]
        else:
            out = v
        if self.mut("odd_tail_written", dx):
            assert H % 2 or W % 2
            out[2 * Hp:, :] = 0.5
            out[:, 2 * Wp:] = 0.5
        dx.copy_(out)

    def op_relu_bwd(self, op, r) -> None:
        if r["p1"] is r["q0"] and self.mutate[0] == "mask_early" and self.mutate[1] is r["q0"]:
            return
        g = r["p1"].float() * (r["p0"].float() > 0)
        accum = bool(op.flags & _lib.ACCUM) and not self.mut("lost_accum", r["q0"])
        r["q0"].copy_(g + r["q0"].float() if accum else g)

    def op_conv_first_dgrad(self, op, r) -> None:
        nd = self.s.nodes[0]
        w = self.conv_w(nd)
        if self.bf16:                                      # dy . (hi + lo): the weights as a two-term bf16 split
            hi, lo = emul.split(w)
            w = (hi + lo).float()
        r["q0"].copy_(conv_b(hwc(r["p0"]), w, self.rev))

    def op_tv(self, op, r) -> None:
        x = r["p0"].float()
        if "q0" in r:
            dy, dx = x[..., 1:, :] - x[..., :-1, :], x[..., :, 1:] - x[..., :, :-1]
            r["q0"][:_lib.TV_LOSS_PARTS] = 0.0
            r["q0"][0] = (dy * dy).sum() + (dx * dx).sum()
        if "q1" in r:
            s = torch.zeros_like(x)
            s[..., 1:, :] += x[..., 1:, :] - x[..., :-1, :]
            s[..., :-1, :] += x[..., :-1, :] - x[..., 1:, :]
            s[..., :, 1:] += x[..., :, 1:] - x[..., :, :-1]
            s[..., :, :-1] += x[..., :, :-1] - x[..., :, 1:]
            r["q1"].add_(torch.tensor(float(op.f0)) * s)

    # -- whole evaluations
    def set_targets(self, style_img: torch.Tensor, content_img: torch.Tensor) -> None:
        s = self.s
        self.run(s.forward_ops(style_img))
        for tap in s.style_taps:
            if s.guide:      # per region, by the float64 definition, from the style image's own label map and counts
                f64 = tap.buf.act.detach().double().permute(2, 0, 1).unsqueeze(0)
                for r, c in enumerate(tap.regions):
                    c.target = guidance_ref.region_gram(f64, self.eng.guide.style_labels, r).float().contiguous()
                continue
            f = tap.buf.act.detach().float().reshape(-1, tap.buf.C)
            tap.target = ((f.t() @ f).clamp(max=plan.GRAM_CLAMP_MAX) / float(f.numel())).contiguous()
        self.run(s.forward_ops(content_img))
        for tap in s.content_taps:
            tap.target = tap.buf.act.clone()
        if self.eng.lap_pools:
            self.eng.bind_lap_targets([torch.from_numpy(lap_ref.pool(content_img, p)) for p in self.eng.lap_pools])

    def fused_step(self, x: torch.Tensor, style_w: float, content_w: float, tv_w: float = 0.0, lap_w: float = 0.0,
                   layer_w: tuple | None = None) -> torch.Tensor:
        """The op list of ``_Engine.loss_and_grad``, built as it builds it; returns the image gradient."""
        eng, s = self.eng, self.s
        self.lap_w, self.layer_w = lap_w, layer_w
        self.products_on.clear()
        grad = torch.zeros_like(x)
        fwd = eng._forward_with_losses(x, style_coef=style_w, with_seed=True, content_coef=content_w, layer_w=layer_w)
        bwd = s.backward_ops(grad, content_coef=content_w, coef_dev=None, prewritten=tuple(t for t in s.content_taps if t.grad_fused))
        if tv_w:
            fwd.insert(0, eng._tv_op(x, loss=True))
            k = max(i for i, o in enumerate(bwd) if o.op == _lib.OP_CONV_FIRST_DGRAD)
            bwd.insert(k + 1, eng._tv_op(x, grad=grad, tv_w=tv_w))
        if lap_w:
            at = 1 if tv_w else 0
            fwd[at:at] = eng._lap_ops(x)
            k = max(i for i, o in enumerate(bwd) if o.op == _lib.OP_CONV_FIRST_DGRAD) + (2 if tv_w else 1)
            if self.mut("lap_insertion", "in front of the dgrad"):      # (which stores: the accumulated terms are lost)
                k = max(i for i, o in enumerate(bwd) if o.op == _lib.OP_CONV_FIRST_DGRAD)
            bwd[k:k] = eng._lap_ops(x, grad=grad, lap_w=lap_w)
        self.run(fwd + [eng._combine_op(style_w, content_w, None, tv_w, layer_w, lap_w)] + bwd)
        return grad

    def autograd_step(self, x: torch.Tensor, gout: torch.Tensor) -> torch.Tensor:
        """The op lists of ``forward_losses`` + ``backward_from``."""
        eng, s = self.eng, self.s
        grad = torch.zeros_like(x)
        self.run(eng._forward_with_losses(x, style_coef=0.0, with_seed=False) + [eng._combine_op(1.0, 1.0)])
        g = gout.clone().float()
        if self.mutate[0] == "swap_coef":
            i = self.mutate[1]
            g[i], g[i + 1] = gout[i + 1], gout[i]
            self.hits += 1
        eng.coef_buf.copy_(g)
        seeds = []
        for tap in s.style_taps:
            seeds += s.gram_ops(tap, gram_out=None, target=tap.target, loss_part=None, sgrad=tap.sgrad, coef=1.0,
                                coef_dev=eng.coef_buf[tap.order:], partial=False)
        self.run(seeds + s.backward_ops(grad, content_coef=1.0, coef_dev=eng.coef_buf))
        return grad


def conv_f_1x1(a: torch.Tensor, s_mat: torch.Tensor, rev: bool) -> torch.Tensor:
    w = s_mat.reshape(*s_mat.shape, 1, 1)
    return F.conv2d(a.flip(1), w.flip(1)) if rev else F.conv2d(a, w)


def images(H: int, W: int) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    x0 = synthetic.synthetic_image(2, H, W) + 0.25 * torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(5))
    return synthetic.synthetic_image(1, H, W), synthetic.synthetic_image(0, H, W), x0.contiguous()


def evaluated(monkeypatch, layout, precision, H, W, *, reverse=False, mutate=None, gout=None, tv_w=0.0, cfg=synthetic.VGG19_CFG,
              pooling="max", regions=0, lap_pools=(), lap_w=0.0, layer_w=None, **env):
    eng = make_engine(monkeypatch, layout, precision, H, W, cfg, pooling=pooling, regions=regions, lap_pools=lap_pools, **env)
    monkeypatch.setattr(ops, "loss_combine", cpu_loss_combine)      # (engine.region_losses() launches it directly)
    style, content, x0 = images(H, W)
    eng.sched.alloc_grads()
    sim = StandIn(eng, reverse=reverse, mutate=mutate(eng) if callable(mutate) else mutate)
    sim.set_targets(style, content)
    grad = sim.autograd_step(x0, gout) if gout is not None else sim.fused_step(x0, STYLE_W, CONTENT_W, tv_w, lap_w, layer_w)
    return eng, x0, grad, sim


def check(eng, x0, grad, **kw):
    return lw.check_step(eng, x0, style_w=STYLE_W, content_w=CONTENT_W, x_grad=grad, **kw)


# ------------------------------------------------------------------------------------------------------------- the proof
@pytest.mark.parametrize("reverse", [False, True], ids=["order-as-is", "order-reversed"])
@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_reference_arithmetic_stays_inside_the_intervals(layout, precision, reverse, monkeypatch):
    H, W = (40, 24) if layout in ("default", "two_content", "relu_taps", "pool_taps") else (32, 32)
    eng, x0, grad, _ = evaluated(monkeypatch, LAYOUTS[layout], precision, H, W, reverse=reverse)
    rep = check(eng, x0, grad)
    assert {"conv forward", "Gram seed", "score", "gradient", "image gradient"} <= set(rep.rows)


@pytest.mark.parametrize("reverse", [False, True], ids=["order-as-is", "order-reversed"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_narrow_net_direct_convs(precision, reverse, monkeypatch):
    eng, x0, grad, _ = evaluated(monkeypatch, NARROW_LAYOUT, precision, 40, 24, cfg=NARROW_CFG[precision], reverse=reverse)
    assert_narrow_branches(eng)
    check(eng, x0, grad)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("layout", ["default", "shared_buffer"])
def test_autograd_path_with_a_coefficient_per_loss(layout, precision, monkeypatch):
    n = sum(len(v) for v in LAYOUTS[layout])
    gout = torch.tensor([3e4 * (1.0 + 0.37 * i) for i in range(n)])
    eng, x0, grad, _ = evaluated(monkeypatch, LAYOUTS[layout], precision, 32, 32, gout=gout)
    check(eng, x0, grad, gout=gout)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_total_variation_term(precision, monkeypatch):
    eng, x0, grad, _ = evaluated(monkeypatch, LAYOUTS["default"], precision, 32, 32, tv_w=50.0)
    check(eng, x0, grad, tv_w=50.0)
    with pytest.raises(lw.LayerwiseMismatch) as err:
        check(eng, x0, grad)                             # the term left out of the oracle: image gradient and total differ
    assert set(err.value.tensors) == {"score total", "image grad"}


@pytest.mark.parametrize("env", [{"STV_FUSE_POOL": "0"}, {"STV_POOL_IDX": "0"}, {"STV_FUSE_POOL_BWD": "0"}, {"STV_FUSE_GRAM": "0"},
                                 {"STV_FUSE_CONTENT": "0"}, {"STV_LOSS_BATCH": "0"}, {"STV_LOSS_INTERLEAVE": "0"}],
                         ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()))
def test_switch_arms(env, monkeypatch):
    eng, x0, grad, _ = evaluated(monkeypatch, LAYOUTS["default"], "bf16", 32, 32, **env)
    check(eng, x0, grad)


def test_refuses_rotating_gradients_and_unstored_maps(monkeypatch):
    eng, x0, grad, _ = evaluated(monkeypatch, LAYOUTS["default"], "bf16", 32, 32, STV_GRAD_ARENA="2")
    with pytest.raises(RuntimeError, match="share slabs"):
        check(eng, x0, grad)
    eng, x0, grad, _ = evaluated(monkeypatch, LAYOUTS["default"], "bf16", 32, 32, STV_SKIP_PREPOOL="1")
    with pytest.raises(RuntimeError, match="not stored"):
        check(eng, x0, grad)


# ------------------------------------------------------------ average pooling, guidance, layer weights, Laplacian terms
def evaluated_case(monkeypatch, name: str, precision: str, **kw):
    spec = {k: v for k, v in lw.STEP_CASES[name].items() if k != "precisions"}
    layout, (H, W) = lw.case_layout(spec), spec.pop("size")
    del spec["layout"]
    return evaluated(monkeypatch, layout, precision, H, W, **{**spec, **kw})


def check_case(name: str, eng, x0, grad, **kw):
    spec = lw.STEP_CASES[name]
    return check(eng, x0, grad, **{**{k: spec[k] for k in ("tv_w", "lap_w", "layer_w") if k in spec}, **kw})


NEW_KINDS = {"avg": {"avgpool forward", "gradient (avgpool)"}, "guided": {"region slab", "region loss"}, "lap": {"lap residual"},
             "all": {"avgpool forward", "gradient (avgpool)", "region slab", "region loss", "lap residual"}, "layer": set()}


@pytest.mark.parametrize("reverse", [False, True], ids=["order-as-is", "order-reversed"])
@pytest.mark.parametrize(("name", "precision"), lw.STEP_PARAMS, ids=lambda v: v.replace(" ", "-"))
def test_reference_arithmetic_stays_inside_the_intervals_of_the_new_structures(name, precision, reverse, monkeypatch):
    eng, x0, grad, _ = evaluated_case(monkeypatch, name, precision, reverse=reverse)
    rep = check_case(name, eng, x0, grad)
    assert NEW_KINDS[name.split()[0]] <= set(rep.rows)
    if eng.guide is not None:      # every tapped buffer takes one launch per region: all of them went through several stages
        assert {f"grad L{nd.layer:02d} {nd.kind}" for nd in eng.sched.nodes if any(t.kind == "style" for t in nd.dst.taps)
                and (eng.guide.n > 1 or nd is not eng.sched.nodes[-1])} <= set(rep.multi_stage)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_autograd_path_with_average_pooling(precision, monkeypatch):
    gout = torch.tensor([3e4 * (1.0 + 0.37 * i) for i in range(6)])
    eng, x0, grad, _ = evaluated(monkeypatch, LAYOUTS["default"], precision, 40, 24, gout=gout, pooling="avg")
    rep = check(eng, x0, grad, gout=gout)
    assert {"avgpool forward", "gradient (avgpool)"} <= set(rep.rows)


def test_the_new_refusals(monkeypatch):
    eng, x0, grad, _ = evaluated_case(monkeypatch, "avg default", "bf16")
    with pytest.raises(RuntimeError, match="lap_w = 3 on an engine without lap_pools"):
        check(eng, x0, grad, lap_w=3.0)
    pool = next(nd for nd in eng.sched.nodes if nd.kind == "avgpool")
    pool.kind = "lppool"
    with pytest.raises(RuntimeError, match="no rule for node kind 'lppool'"):
        check(eng, x0, grad)
    pool.kind = "avgpool"
    eng.sched.content_taps[0].kind = "histogram"
    with pytest.raises(RuntimeError, match="no rule for tap kind 'histogram'"):
        check(eng, x0, grad)
    eng, x0, grad, _ = evaluated_case(monkeypatch, "guided R=2", "bf16")
    eng.sched.style_taps[1].regions = None
    with pytest.raises(RuntimeError, match=r"guided schedule without attached regions \(style tap 1\)"):
        check(eng, x0, grad)
    eng, x0, grad, _ = evaluated_case(monkeypatch, "guided R=2", "bf16")
    with pytest.raises(RuntimeError, match="gout"):
        check(eng, x0, grad, gout=[1.0] * 6)
    eng.guide = None
    with pytest.raises(RuntimeError, match="guide = 2 on an engine whose guide is None"):
        check(eng, x0, grad)


# --------------------------------------------------------------------------------------------------------- the mutations
def node_of(eng, layer: int, kind: str | None = None):
    return next(nd for nd in eng.sched.nodes if nd.layer == layer and (kind is None or nd.kind == kind))


def expect_failure(eng, x0, grad, first: str, **kw) -> None:
    with pytest.raises(lw.LayerwiseMismatch) as err:
        check(eng, x0, grad, **kw)
    assert err.value.tensors[0] == first, err.value.tensors


TWO_ULP_CASES = [("bf16", "act L12 conv"), ("bf16", "grad L12 conv"), ("bf16", "seed style2"), ("bf16", "idx"),
                 ("fp32", "act L09 pool"), ("fp32", "grad L07 conv"), ("fp32", "idx"),
                 ("bf16x3", "act L09 pool"), ("bf16x3", "grad L07 conv")]


@pytest.mark.parametrize(("precision", "name"), TWO_ULP_CASES, ids=lambda v: v.replace(" ", "-"))
def test_one_element_two_storage_ulps_off(precision, name, monkeypatch):
    """bf16 storage: any stored tensor (at most two neighbouring values are admissible).  fp32 storage: the tensors that
    are bit-exact by construction (pool outputs, moved gradients, byte maps) - two fp32 ulps on a sum of K = 9 * Cin
    products are INSIDE the any-order bound K u A, there no per-element rule can tell them from another summation order."""
    eng, x0, grad, _ = evaluated(monkeypatch, LAYOUTS["default"], precision, 32, 32)
    if name == "idx":
        nd = next(n for n in eng.sched.nodes if n.idx is not None)
        flat = nd.idx.view(-1)
        flat[5] = ((int(flat[5]) + 1) & 3) | (int(flat[5]) & 4)
        return expect_failure(eng, x0, grad, f"idx L{nd.layer:02d}")
    if name.startswith("seed"):
        t = eng.sched.style_taps[2].sgrad
    else:
        _, layer, kind = name.split()
        nd = node_of(eng, int(layer[1:]), kind)
        t = nd.dst.act if name.startswith("act") else nd.dst.grad
    flat = t.view(-1)
    k = int(flat.float().abs().argmax())             # (an element that is not zero: a masked one has no value two ulps away)
    bits = 8 if t.dtype == torch.bfloat16 else 24
    ulp = 2.0 ** (torch.frexp(flat[k].float().abs())[1].item() - bits)
    flat[k] = flat[k].float() + 2 * ulp
    with pytest.raises(lw.LayerwiseMismatch) as err:
        check(eng, x0, grad)
    assert name in err.value.tensors, err.value.tensors


@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_a_dropped_bias(precision, monkeypatch):
    for layer in (0, 14):
        eng, x0, grad, sim = evaluated(monkeypatch, LAYOUTS["default"], precision, 32, 32, mutate=("drop_bias", layer))
        assert sim.hits >= 1
        expect_failure(eng, x0, grad, f"act L{layer:02d} {'conv_first' if layer == 0 else 'conv'}")


@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_a_relu_mask_from_the_wrong_buffer(precision, monkeypatch):
    # conv 12 -> relu -> conv 14: the dgrad of conv 14 masks with conv 12's stored output
    eng, x0, grad, sim = evaluated(monkeypatch, LAYOUTS["default"], precision, 32, 32, mutate=lambda e: ("wrong_mask", node_of(e, 12).dst.grad))
    assert sim.hits == 1
    expect_failure(eng, x0, grad, "grad L12 conv")


@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_a_lost_accum(precision, monkeypatch):
    # content tap on conv 21: the forward half wrote its gradient, the dgrad of conv 23 accumulates onto it
    eng, x0, grad, sim = evaluated(monkeypatch, LAYOUTS["default"], precision, 32, 32, mutate=lambda e: ("lost_accum", node_of(e, 21).dst.grad))
    assert sim.hits == 1
    expect_failure(eng, x0, grad, "grad L21 conv")
    # a Gram product launched on its own (no dual dgrad), accumulating onto the dgrad's result
    eng, x0, grad, sim = evaluated(monkeypatch, LAYOUTS["default"], precision, 32, 32, STV_FUSE_GRAM="0",
                                   mutate=lambda e: ("lost_accum", node_of(e, 10).dst.grad))
    assert sim.hits == 1
    expect_failure(eng, x0, grad, "grad L10 conv")


@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_a_tap_term_applied_twice(precision, monkeypatch):
    # the deepest tap (style, conv 28) stores the first gradient of the chain; a content tap behind a dgrad (two taps on 5)
    eng, x0, grad, sim = evaluated(monkeypatch, LAYOUTS["default"], precision, 32, 32, mutate=lambda e: ("tap_twice", node_of(e, 28).dst.grad))
    assert sim.hits == 1
    expect_failure(eng, x0, grad, "grad L28 conv")
    eng, x0, grad, sim = evaluated(monkeypatch, LAYOUTS["shared_buffer"], precision, 32, 32, STV_FUSE_CONTENT="0",
                                   mutate=lambda e: ("tap_twice", node_of(e, 5).dst.grad))
    assert sim.hits >= 1
    expect_failure(eng, x0, grad, "grad L05 conv")


@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_a_route_to_the_wrong_window_position(precision, monkeypatch):
    # the pool behind conv 7 (layer 9): routed by the dgrad of conv 10 in bf16, a pooling-backward pass otherwise
    eng, x0, grad, sim = evaluated(monkeypatch, LAYOUTS["default"], precision, 32, 32, mutate=lambda e: ("wrong_route", node_of(e, 7).dst.grad))
    assert sim.hits == 1
    assert (node_of(eng, 10).route is not None) == (precision == "bf16")
    expect_failure(eng, x0, grad, "grad L07 conv")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_an_upstream_coefficient_swapped_with_its_neighbour(precision, monkeypatch):
    gout = torch.tensor([3e4 * (1.0 + 0.37 * i) for i in range(6)])
    for i, first in ((1, "seed style1"), (4, "seed style4")):       # two style terms; the last style term and the content term
        eng, x0, grad, sim = evaluated(monkeypatch, LAYOUTS["default"], precision, 32, 32, gout=gout, mutate=("swap_coef", i))
        assert sim.hits == 1
        expect_failure(eng, x0, grad, first, gout=gout)
        if i == 4:
            with pytest.raises(lw.LayerwiseMismatch) as err:
                check(eng, x0, grad, gout=gout)
            assert "grad L21 conv" in err.value.tensors


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_a_prewritten_content_gradient_overwritten_by_the_routed_pooling_backward(precision, monkeypatch):
    # content tap on conv 16, in front of a pool: its gradient is written in the forward half, and the pooling backward
    # must ADD to it - which is why _decide never routes a dgrad (a launch that stores) into such a buffer
    eng, x0, grad, sim = evaluated(monkeypatch, LAYOUTS["prepool"], precision, 32, 32, mutate=lambda e: ("route_overwrites", node_of(e, 16).dst.grad))
    assert sim.hits == 1 and all(nd.route is None or nd.route.src is not node_of(eng, 16).dst for nd in eng.sched.nodes)
    expect_failure(eng, x0, grad, "grad L16 conv")


# ------------------------------------------------------------------------------------- decisions are read per node
def test_an_untapped_first_conv_leaves_its_relu_to_the_consumer():
    """The first-layer kernels have no ReLU epilogue (their op carries no flags): with layer 0 untapped the ReLU behind it
    must be applied by the next conv while staging - as a fused ReLU it was applied by nobody (found by the layouts
    without a tap on layer 0, the first rows of this file's matrix that ever ran such a schedule)."""
    s = plan.Schedule(vgg_layers(), [2, 7], [16, 25], 32, 32, torch.float32, CPU, with_grad=True, assume_device=True)
    first, second = s.nodes[0], s.nodes[1]
    assert first.kind == "conv_first" and not first.dst.relu_fused and second.relu_in
    fwd = s.forward_ops(torch.zeros(1, 3, 32, 32))
    assert fwd[0].op == _lib.OP_CONV_FIRST_FWD and fwd[0].flags == 0 and fwd[1].flags & _lib.RELU_IN


def _both(values) -> bool:
    return len({bool(v) if not isinstance(v, bool) else v for v in values}) == 2


def test_every_decision_field_is_read_per_node(monkeypatch):
    """40x24, bf16, default taps: the fourth pool's input is 5x3 - not twice its output - so the first three pools are
    routed and the fourth is not; tapped convs make relu_in, relu_fused and gram take both values as well.  Forcing any of
    them to one value for the whole schedule, as the walk this checker grew out of did, fails.  (``fused``, ``idx``,
    ``partials_fused`` and ``grad_fused`` choose between launches that store the same values - first maximum in scan
    order either way, the same sums in another order - so no stored tensor can tell their two readings apart.)"""
    def fresh():
        return evaluated(monkeypatch, LAYOUTS["default"], "bf16", 40, 24)
    eng, x0, grad, _ = fresh()
    convs = [nd for nd in eng.sched.nodes if nd.kind == "conv"]
    pools = [nd for nd in eng.sched.nodes if nd.kind == "pool"]
    assert _both(nd.route is not None for nd in convs) and _both(nd.gram is not None for nd in convs)
    assert _both(nd.relu_in for nd in convs) and _both(nd.dst.relu_fused for nd in convs)
    assert any(id(p) not in {id(nd.route) for nd in convs} for p in pools) and all(p.idx is not None and p.fused for p in pools)
    check(eng, x0, grad)
    for field, value in (("route", None), ("gram", None), ("relu_in", False), ("relu_in", True)):
        eng, x0, grad, _ = fresh()
        for nd in eng.sched.nodes:
            if nd.kind == "conv":
                setattr(nd, field, value)
        with pytest.raises(lw.LayerwiseMismatch):
            check(eng, x0, grad)
    for value in (False, True):
        eng, x0, grad, _ = fresh()
        for nd in eng.sched.nodes:
            if nd.kind == "conv":
                nd.dst.relu_fused = value
        with pytest.raises(lw.LayerwiseMismatch):
            check(eng, x0, grad)


# ------------------------------------------- mutations of the new structures: each fails, naming the mutated tensor
def mutated_case(monkeypatch, name: str, precision: str, mutate, first: str, *, hits: int | None = None):
    eng, x0, grad, sim = evaluated_case(monkeypatch, name, precision, mutate=mutate)
    assert sim.hits >= 1 if hits is None else sim.hits == hits, sim.hits
    with pytest.raises(lw.LayerwiseMismatch) as err:
        check_case(name, eng, x0, grad)
    assert err.value.tensors[0] == first, err.value.tensors
    return eng


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_avgpool_summed_pairwise(precision, monkeypatch):
    """(a+b)+(c+d) in place of ((a+b)+c)+d.  fp32 storage only: a window of four bf16 values sums exactly in fp32 in either
    order (8-bit significands, exponents a few apart), so bf16 storage cannot tell the two orders apart."""
    eng0, _, _, _ = evaluated_case(monkeypatch, "avg default", precision)      # (the pool runs three times: two captures, the step)
    eng = mutated_case(monkeypatch, "avg default", precision, lambda e: ("avg_pairwise", node_of(e, 4).dst.act), "act L04 avgpool")
    assert not torch.equal(node_of(eng0, 4).dst.act, node_of(eng, 4).dst.act)      # the two orders differ on this input


@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_avgpool_backward_mutations(precision, monkeypatch):
    # conv 2 -> ReLU (fused) -> avgpool 4: the pool's backward masks with conv 2's stored output
    eng = mutated_case(monkeypatch, "avg default", precision, lambda e: ("lost_mask", node_of(e, 2).dst.grad), "grad L02 conv", hits=1)
    assert node_of(eng, 2).dst.relu_fused and not node_of(eng, 4).relu_in
    mutated_case(monkeypatch, "avg default", precision, lambda e: ("wrong_mask", node_of(e, 2).dst.grad), "grad L02 conv", hits=1)
    # conv 2 tapped -> the pool takes the pending ReLU itself (relu_in): the mask is then the node's own
    eng = mutated_case(monkeypatch, "avg pending relu", precision, lambda e: ("lost_mask", node_of(e, 2).dst.grad), "grad L02 conv", hits=1)
    assert node_of(eng, 4).relu_in and not node_of(eng, 2).dst.relu_fused
    # content tap on conv 16 in front of avgpool 18: the forward half wrote the gradient, the pool's backward accumulates
    eng = mutated_case(monkeypatch, "avg prepool", precision, lambda e: ("lost_accum", node_of(e, 16).dst.grad), "grad L16 conv", hits=1)
    assert node_of(eng, 18).kind == "avgpool" and node_of(eng, 16).dst.taps[0].grad_fused
    # conv 25's map is 5x3: the fifth row and the third column take no part and must be written +0
    eng = mutated_case(monkeypatch, "avg default", precision, lambda e: ("odd_tail_written", node_of(e, 25).dst.grad), "grad L25 conv", hits=1)
    assert (node_of(eng, 25).dst.H, node_of(eng, 25).dst.W) == (5, 3)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_mask_split_mutations(precision, monkeypatch):
    mutated_case(monkeypatch, "guided R=2", precision, lambda e: ("label255_into_slab0", e.sched.style_taps[2].slabs), "slab style2 r0", hits=1)
    mutated_case(monkeypatch, "guided R=3", precision, lambda e: ("swap_slabs", e.sched.style_taps[2].slabs), "slab style2 r0", hits=1)


@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_region_chain_mutations(precision, monkeypatch):
    chain5 = lambda e: e.sched.all_chains()[5]      # noqa: E731  (style tap 2 = conv 10, region 1)
    mutated_case(monkeypatch, "guided R=2", precision, lambda e: ("norm_parent", chain5(e).sgrad), "seed style5", hits=1)
    mutated_case(monkeypatch, "guided R=2", precision, lambda e: ("swap_lambda", chain5(e).sgrad), "seed style5", hits=1)
    # the deepest tap opens the chain: region 0's product stores, region 1's accumulates
    mutated_case(monkeypatch, "guided R=2", precision, lambda e: ("lost_accum", node_of(e, 28).dst.grad), "grad L28 conv", hits=1)
    mutated_case(monkeypatch, "guided R=2", precision, lambda e: ("region_twice", chain5(e).buf.act), "grad L10 conv", hits=1)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_relu_mask_behind_the_first_region_term(precision, monkeypatch):
    eng = mutated_case(monkeypatch, "guided relu taps", precision, lambda e: ("mask_early", node_of(e, 5).dst.grad), "grad L05 conv", hits=1)
    assert node_of(eng, 5).dst.relu_fused and node_of(eng, 5).dst.taps


@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_layer_weight_in_seed_or_scale_only(precision, monkeypatch):
    mutated_case(monkeypatch, "layer weights", precision, lambda e: ("seed_without_w", e.sched.style_taps[2].sgrad), "seed style2", hits=1)
    mutated_case(monkeypatch, "layer weights", precision, ("scale_without_w", 2), "score style", hits=1)
    eng, x0, grad, _ = evaluated_case(monkeypatch, "layer weights", precision)
    assert float(eng.sched.style_taps[1].sgrad.float().abs().max()) == 0.0           # the zero-weight tap


def test_laplacian_mutations(monkeypatch):
    """(The term added to the total in front of TV's is not among them: the two orders differ by an fp32 ulp of the total,
    far inside the derived error of the scores, so no value of the weights makes it observable.)"""
    mutated_case(monkeypatch, "lap (4,)", "fp32", ("lap_lost_accum", 4), "image grad", hits=1)
    mutated_case(monkeypatch, "lap (2, 8) tv", "fp32", ("lap_lost_accum", 8), "image grad", hits=1)
    mutated_case(monkeypatch, "lap (2, 8)", "bf16", ("lap_swap_coef", 2), "image grad", hits=1)
    mutated_case(monkeypatch, "lap (4,) tv", "fp32", ("lap_margin", 4), "image grad", hits=1)
    mutated_case(monkeypatch, "lap (2, 8) tv", "bf16", ("lap_insertion", "in front of the dgrad"), "image grad", hits=1)
    eng, x0, grad, _ = evaluated_case(monkeypatch, "lap (4,)", "fp32")
    eng.lap_resid[0][1, 2, 3] += 1e-3
    with pytest.raises(lw.LayerwiseMismatch) as err:
        check_case("lap (4,)", eng, x0, grad)
    assert err.value.tensors[0] == "lap resid p4"


def test_avgpool_relu_in_is_read_per_node(monkeypatch):
    """content7: conv 7 is tapped, so the pool behind it takes the pending ReLU itself, the other three pools do not."""
    eng, x0, grad, _ = evaluated_case(monkeypatch, "avg content7", "bf16")
    pools = [nd for nd in eng.sched.nodes if nd.kind == "avgpool"]
    assert _both(nd.relu_in for nd in pools)
    check_case("avg content7", eng, x0, grad)
    # read as "no pool takes a ReLU": the pool behind conv 7 is then checked against the mean of unclamped values.  (The
    # other global reading, "every pool takes one", describes the same values: a pool without relu_in reads a map whose ReLU
    # ran in the conv's epilogue - clamping it again changes nothing, and its backward carries the mask either way.)
    eng, x0, grad, _ = evaluated_case(monkeypatch, "avg content7", "bf16")
    for nd in eng.sched.nodes:
        if nd.kind == "avgpool":
            nd.relu_in = False
    with pytest.raises(lw.LayerwiseMismatch) as err:
        check_case("avg content7", eng, x0, grad)
    assert err.value.tensors[0] == "act L09 avgpool"


def test_a_region_norm_of_the_parent_in_the_schedule(monkeypatch):
    """The same error one level up: the schedule itself hands a chain ``C * H * W`` as its norm (what ``attach_regions`` would do
    with the parent's pixel count), the stand-in runs the ops as built - the checker counts ``n_r`` from the label map itself."""
    eng = make_engine(monkeypatch, LAYOUTS["default"], "bf16", *lw.GUIDE_SIZE, regions=2)
    monkeypatch.setattr(ops, "loss_combine", cpu_loss_combine)
    chain = eng.sched.all_chains()[3]
    chain.norm = float(chain.buf.C * chain.buf.H * chain.buf.W)
    style, content, x0 = images(*lw.GUIDE_SIZE)
    eng.sched.alloc_grads()
    sim = StandIn(eng)
    sim.set_targets(style, content)
    grad = sim.fused_step(x0, STYLE_W, CONTENT_W)
    with pytest.raises(lw.LayerwiseMismatch) as err:
        check(eng, x0, grad)
    assert err.value.tensors[0] == "seed style3"
