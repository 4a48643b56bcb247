"""Lower a sliced VGG feature stack + loss taps to ``stv_op_t`` command buffers.

This is the host half of the hot path: it runs once per (model, image size),
allocates every activation / gradient / workspace buffer through PyTorch, and
emits flat op arrays that ``libstv_hip.so`` executes each optimisation step
(``stv_program_run``).  It restates, as a schedule, what autograd does for the
reference's ``StyleContentModel.forward`` + ``loss.backward()``
(/root/reference/src/style_transfer_visualizer/core_model.py:297-328,
optimization.py:292-313):

* conv -> ReLU pairs are fused (ReLU in the producer's epilogue) unless the
  conv output itself is tapped; then the consumer applies ReLU while staging;
* every gradient w.r.t. a stored activation is written exactly once by its
  consumer (with the ReLU mask fused in the epilogue) and tap gradients
  (Gram product, content difference) accumulate on top;
* Gram backward is ``dF = F . S`` with the symmetric seed ``S`` produced by
  ``stv_gram_finish``; it runs as a 1x1 conv on the matrix cores.

Which ops are fused, and where the loss-side ops of every tap go (behind its producer, or in the batched tail of
the forward pass), is decided once, in ``Schedule._decide``, from the ``Switches`` the schedule was constructed
with and from whether it runs on the GPU; the result lives in fields of ``Node``, ``Buf``, ``Tap`` and the
schedule.  ``forward_ops``, ``alloc_grads``, ``backward_ops``, the Gram emitters and the engine's loss head only
read those fields, so the op lists of one schedule do not depend on the order, or the number of times, they are built.

An op owns its operands: ``Schedule.emit`` records every tensor an op names by raw pointer on the op object
(``op.refs``), and a ``Program`` keeps alive what its ops reference (:func:`operands`) - nothing accumulates on the
schedule, and a program pins exactly what it runs on.
"""
from __future__ import annotations

import os

import ctypes
from dataclasses import dataclass, field

import torch
from torch import nn

from . import _lib, ops
from ._lib import (ACCUM, MASK, POOL_IDX, POOL_ONLY, POOL_ROUTE, W_BLOCKED, OP_GRAM_MULTI, OP_CONTENT_GRAD, OP_CONTENT_LOSS, OP_CONV, OP_CONV_FIRST_DGRAD,
                   OP_CONV_FIRST_FWD, OP_GRAM_FINISH, OP_GRAM_PARTIAL, OP_LOSS_COMBINE, OP_POOL_BWD,
                   OP_AVGPOOL_BWD, OP_AVGPOOL_FWD, OP_MASK_SPLIT, OP_POOL_FWD, OP_RELU_BWD, OP_RELU_FWD, OP_TV, RELU_IN, RELU_OUT, StvOp)

GRAM_CLAMP_MAX = 5e5  # reference constants.py:15


@dataclass(frozen=True)
class Switches:
    """The step-level A/B switches, read once: when a ``Schedule`` or an engine is constructed."""

    fuse_pool: bool = True            # STV_FUSE_POOL
    pool_idx: bool = True             # STV_POOL_IDX
    fuse_gram_first: int = 1          # STV_FUSE_GRAM_FIRST: 0 never, 1 where it pays, 2 always
    skip_prepool: bool = True         # STV_SKIP_PREPOOL
    fuse_pool_bwd: bool = True        # STV_FUSE_POOL_BWD
    fuse_gram: bool = True            # STV_FUSE_GRAM
    w_blocked: bool = True            # STV_W_BLOCKED
    grad_arena: int = 1               # STV_GRAD_ARENA: 0 one tensor per gradient, 1 slabs, 2 slabs also for host tensors
    fuse_content: bool = True         # STV_FUSE_CONTENT
    loss_batch: str = "auto"          # STV_LOSS_BATCH: "1" every style tap, "auto" the small ones, anything else none
    gram_fin_late: bool = True        # STV_GRAM_FIN_LATE
    loss_interleave: bool = True      # STV_LOSS_INTERLEAVE
    hip_graph: bool = True            # STV_HIP_GRAPH

    @classmethod
    def from_env(cls) -> Switches:
        def level(value: str) -> int:
            return {"0": 0, "2": 2}.get(value, 1)
        return cls(fuse_pool=os.environ.get("STV_FUSE_POOL", "1") != "0",
                   pool_idx=os.environ.get("STV_POOL_IDX", "1") != "0",
                   fuse_gram_first=level(os.environ.get("STV_FUSE_GRAM_FIRST", "1")),
                   skip_prepool=os.environ.get("STV_SKIP_PREPOOL", "1") != "0",
                   fuse_pool_bwd=os.environ.get("STV_FUSE_POOL_BWD", "1") != "0",
                   fuse_gram=os.environ.get("STV_FUSE_GRAM", "1") != "0",
                   w_blocked=os.environ.get("STV_W_BLOCKED", "1") != "0",
                   grad_arena=level(os.environ.get("STV_GRAD_ARENA", "1")),
                   fuse_content=os.environ.get("STV_FUSE_CONTENT", "1") != "0",
                   loss_batch=os.environ.get("STV_LOSS_BATCH", "auto"),
                   gram_fin_late=os.environ.get("STV_GRAM_FIN_LATE", "1") != "0",
                   loss_interleave=os.environ.get("STV_LOSS_INTERLEAVE", "1") == "1",
                   hip_graph=os.environ.get("STV_HIP_GRAPH", "1") != "0")


@dataclass
class Buf:
    """One materialised activation (NHWC) and, for the backward pass, its gradient."""

    H: int
    W: int
    C: int
    act: torch.Tensor
    relu_fused: bool = False       # stored value is relu(z)
    taps: list = field(default_factory=list)
    grad: torch.Tensor | None = None
    stored: bool = True            # False: the forward program does not write `act` (a pre-pool map nobody reads: STV_POOL_ONLY)


@dataclass
class Node:
    # conv_first | conv | pool | avgpool | relu.  An average pool is a kind of its own: every fusion below that tests for
    # "pool" (the conv epilogue's pooled output, the arg-max byte map, the routed dgrad) is a max-pool fusion and stays off;
    # an avgpool node is never `fused`, has no `idx`, is never a `route`, and its source map is always `stored`.
    # Its `relu_in`: the node takes a pending ReLU itself (mean(relu(z)) != relu(mean(z)): it cannot be left to the consumer)
    kind: str
    src: Buf | None
    dst: Buf
    relu_in: bool = False
    layer: int = -1
    wf: torch.Tensor | None = None
    wb: torch.Tensor | None = None
    packed: torch.Tensor | None = None  # conv_first: the kernel-side form of wf (ops.conv_first_pack), read by both directions
    bias: torch.Tensor | None = None
    cin: int = 0
    # fixed by Schedule._decide:
    fused: bool = False                 # pool nodes: the work rides in the preceding conv's epilogue
    idx: torch.Tensor | None = None     # pool nodes fused into a conv: arg-max byte map for the backward
    route: Node | None = None           # conv nodes: the pool node whose backward rides in this conv's dgrad
    gram: Tap | None = None             # conv nodes: the style tap whose dF = F.S rides in this conv's dgrad


@dataclass
class Tap:
    kind: str                      # style | content
    order: int                     # index inside its kind (block order)
    buf: Buf
    target: torch.Tensor | None = None
    # style
    partials: torch.Tensor | None = None
    partials_fused: bool = False      # the producing conv fills `partials` itself (stv_conv_first_fwd's gram_partials)
    sgrad: torch.Tensor | None = None
    parts_off: int = 0
    parts_cnt: int = 0
    # fixed by Schedule._decide - where the tap's loss-side ops go (row strips build a head of their own: unused there):
    in_tail: bool = False             # in the batched tail behind the last conv; False: right behind its producer
    finish_late: bool = False         # style: partial sums behind the producer, only the finish pass in the tail
    grad_fused: bool = False          # content: the fused step forms loss and gradient in one pass (stv_content_loss_grad)
    # spatial guidance (Schedule.attach_regions): a guided style tap owns a label map, the region slabs stv_mask_split fills
    # and one child tap per active region - its `buf` is the slab, its `norm` C times the region's pixel count; the child
    # carries the Gram chain (partials, target, seed, loss partials) and takes the placement of its parent
    labels: torch.Tensor | None = None
    slabs: torch.Tensor | None = None
    regions: list | None = None
    norm: float | None = None         # the Gram's divisor; None: C * H * W of the buffer (the reference's b*c*h*w)
    parent: Tap | None = None


def _check_layer(layer: nn.Module, idx: int) -> str:
    if isinstance(layer, nn.Conv2d):
        ok = (layer.kernel_size == (3, 3) and layer.stride == (1, 1) and layer.padding == (1, 1)
              and layer.dilation == (1, 1) and layer.groups == 1 and layer.padding_mode == "zeros")
        if not ok:
            msg = f"layer {idx}: only Conv2d(k=3, stride=1, padding=1) has a HIP kernel"
            raise RuntimeError(msg)
        return "conv"
    if isinstance(layer, nn.ReLU):
        return "relu"
    if isinstance(layer, nn.MaxPool2d):
        ks = layer.kernel_size if isinstance(layer.kernel_size, tuple) else (layer.kernel_size,) * 2
        stv = layer.stride if isinstance(layer.stride, tuple) else (layer.stride,) * 2
        pad = layer.padding if isinstance(layer.padding, tuple) else (layer.padding,) * 2
        if ks != (2, 2) or stv != (2, 2) or pad != (0, 0) or layer.ceil_mode:
            msg = f"layer {idx}: only MaxPool2d(2, 2) has a HIP kernel"
            raise RuntimeError(msg)
        return "pool"
    if isinstance(layer, nn.AvgPool2d):
        ks = layer.kernel_size if isinstance(layer.kernel_size, tuple) else (layer.kernel_size,) * 2
        stv = layer.stride if isinstance(layer.stride, tuple) else (layer.stride,) * 2
        pad = layer.padding if isinstance(layer.padding, tuple) else (layer.padding,) * 2
        # (count_include_pad only matters with padding; a divisor_override would change the 0.25)
        if ks != (2, 2) or stv != (2, 2) or pad != (0, 0) or layer.ceil_mode or layer.divisor_override is not None:
            msg = f"layer {idx}: only AvgPool2d(2, 2) has a HIP kernel"
            raise RuntimeError(msg)
        return "avgpool"
    msg = f"layer {idx}: {type(layer).__name__} has no HIP kernel on this path"
    raise RuntimeError(msg)


_PRODUCT_OPS = (OP_CONV, OP_GRAM_PARTIAL, OP_GRAM_MULTI)      # the ops that take STV_BF16X3 in bf16x3 mode


class Schedule:
    """Buffers + forward/backward op lists for one image size."""

    def __init__(self, layers: list[nn.Module], style_at: list[int], content_at: list[int],
                 H: int, W: int, dtype: torch.dtype, device: torch.device, *, with_grad: bool, halo: int = 0,
                 split: bool = False, switches: Switches | None = None, fuse_first_gram: bool = True,
                 assume_device: bool = False, guide: int = 0) -> None:
        """``halo`` = 1: the schedule of one ROW STRIP of a larger image (spatial.py).  ``H`` is the
        strip's own row count; every activation (and the image) carries ``halo`` extra rows above and
        below that the owner fills before each 3x3 convolution reads them (neighbour's rows, or zeros
        at the image border).  ``split=True`` (fp32 storage only): bf16x3 - the conv and Gram ops form their products
        from split bf16 operands (STV_BF16X3, weights pre-split at packing); every other op runs as in fp32.
        Convolutions run over the whole buffer - their output in the halo
        rows is meaningless and is replaced by the next exchange - while pooling works on the
        strip's own rows only (strip heights are multiples of 16, so no window straddles two strips).
        ``fuse_first_gram=False``: the Gram of a tapped first layer runs over a sub-range of its buffer
        (spatial.SpatialShard), so the first-layer kernel must not leave slabs of the whole map.
        ``assume_device``: take the decisions of a GPU schedule on host tensors - to be inspected, never run.
        ``guide`` > 0: spatial guidance with that many active regions - every style tap runs one Gram chain per region
        (``attach_regions`` hands it the label maps), so the two fusions that assume one Gram per tap are off."""
        self.H, self.W, self.dtype, self.device = H, W, dtype, device
        if guide and halo:
            msg = "spatial guidance (masks) runs on whole images only (no row strips)"
            raise ValueError(msg)
        self.guide = int(guide)
        if split and (dtype != torch.float32 or halo):
            msg = "bf16x3 (split-bf16 products) runs on fp32 storage and whole images only (no row strips)"
            raise ValueError(msg)
        self.split = split
        self.halo = halo
        self.switches = switches if switches is not None else Switches.from_env()
        self.device_form = assume_device or device.type == "cuda"      # the fusions below exist as GPU kernels only
        self.nodes: list[Node] = []
        self.style_taps: list[Tap] = []
        self.content_taps: list[Tap] = []
        self.with_grad = with_grad
        self._lower_forward(layers, style_at, content_at)
        self._decide(fuse_first_gram)

    # ------------------------------------------------------------------ forward walk
    def _new_buf(self, H: int, W: int, C: int) -> Buf:
        if self.halo:
            act = torch.zeros(H + 2 * self.halo, W, C, device=self.device, dtype=self.dtype)
            return Buf(H + 2 * self.halo, W, C, act)
        act = torch.empty(H, W, C, device=self.device, dtype=self.dtype)
        return Buf(H, W, C, act)

    def _check_map(self, layer: int, H: int, W: int, C: int) -> None:
        """Refuses a conv whose output map the conv kernels cannot address (32-bit byte offsets: ops.CONV_MAX_BYTES per
        tensor, include/stv.h stv_conv_fits).  Every activation of a schedule is such a map or a pooled, smaller one."""
        rows = H + 2 * self.halo
        nbytes = rows * W * C * torch.empty(0, dtype=self.dtype).element_size()
        if nbytes > ops.CONV_MAX_BYTES:
            name = {torch.bfloat16: "bf16", torch.float32: "fp32"}.get(self.dtype, str(self.dtype))
            ways = ("" if self.dtype == torch.bfloat16 else "bf16 storage, ") + "a smaller image size, or row strips on several GPUs"
            msg = (f"layer {layer}: its {rows}x{W}x{C} {name} map holds {nbytes} bytes, over the conv kernels' limit of "
                   f"{ops.CONV_MAX_BYTES} bytes per tensor (32-bit offsets): use {ways}")
            raise ValueError(msg)

    def interior(self, t: torch.Tensor) -> torch.Tensor:
        """The strip's own rows of an NHWC buffer (the whole buffer without halos)."""
        return t[self.halo:t.shape[0] - self.halo] if self.halo else t

    def _lower_forward(self, layers: list[nn.Module], style_at: list[int], content_at: list[int]) -> None:
        tapped = set(style_at) | set(content_at)
        last = max(tapped)
        kinds = [_check_layer(layer, i) for i, layer in enumerate(layers[:last + 1])]
        cur: Buf | None = None           # None = the NCHW fp32 image
        pending_relu = False
        H, W = self.H, self.W
        i = 0
        while i <= last:
            kind = kinds[i]
            out_idx = i
            if kind == "conv":
                conv: nn.Conv2d = layers[i]
                self._check_map(i, H, W, conv.out_channels)      # before anything of this layer is allocated
                w = conv.weight.detach().to(self.device, torch.float32)
                bias = (conv.bias.detach().to(self.device, torch.float32).contiguous()
                        if conv.bias is not None else None)
                cout, cin = w.shape[:2]
                dst = self._new_buf(H, W, cout)
                if cur is None:
                    if pending_relu:
                        msg = "a ReLU in front of the first convolution is not supported"
                        raise RuntimeError(msg)
                    node = Node("conv_first", None, dst, layer=i, wf=ops.pack_weights_fwd(w), bias=bias, cin=cin)
                    if self.device.type == "cuda":
                        node.packed = ops.conv_first_pack(node.wf)   # frozen weights: kernel-side packing, once
                else:
                    wf = ops.pack_weights_fwd(w).to(self.dtype)
                    wb = ops.pack_weights_bwd(w).to(self.dtype) if self.with_grad else None
                    # matrix-core shapes take K-blocked weights (W_BLOCKED is derived from w.dim() == 4)
                    # A/B knob (bf16x3: always blocked - its 3x3 kernels read pre-split K-blocked weights only)
                    blocked = self.split or self.switches.w_blocked
                    if blocked and ops.conv_uses_mfma(H, W, cin, cout, self.dtype, split=self.split):
                        wf = ops.block_weights(wf)
                        if self.split:     # frozen weights: split into bf16 hi / lo once, here
                            wf = ops.split_weights(wf)
                    if blocked and wb is not None and ops.conv_uses_mfma(H, W, cout, cin, self.dtype, split=self.split):
                        wb = ops.block_weights(wb)
                        if self.split:
                            wb = ops.split_weights(wb)
                    if self.device.type == "cuda":      # measure the tile configurations of this layer's shapes once
                        ops.conv_tune(H, W, cin, cout, 9, self.dtype, split=self.split)
                        if self.with_grad:
                            ops.conv_tune(H, W, cout, cin, 9, self.dtype, split=self.split)
                    node = Node("conv", cur, dst, relu_in=pending_relu, layer=i, wf=wf, wb=wb, bias=bias, cin=cin)
                pending_relu = False
                # (the first-layer kernels have no ReLU epilogue: an untapped first conv leaves z, and its consumer
                # applies the ReLU while staging, as behind a tapped conv)
                if i + 1 <= last and kinds[i + 1] == "relu" and i not in tapped and node.kind == "conv":
                    dst.relu_fused = True      # ReLU runs in this conv's epilogue
                    out_idx = i + 1
                self.nodes.append(node)
                cur = dst
            elif kind == "relu":
                if cur is None:
                    msg = "ReLU directly on the input image is not supported"
                    raise RuntimeError(msg)
                if i in tapped:
                    dst = self._new_buf(cur.H, cur.W, cur.C)
                    self.nodes.append(Node("relu", cur, dst, layer=i))
                    cur = dst
                    pending_relu = False
                else:
                    pending_relu = True        # applied by the consumer while staging
            else:  # pool | avgpool
                if cur is None:
                    msg = f"{'AvgPool' if kind == 'avgpool' else 'MaxPool'} directly on the input image is not supported"
                    raise RuntimeError(msg)
                if kind == "avgpool" and self.halo:
                    msg = "average pooling (AvgPool2d) runs on whole images only (no row strips)"
                    raise ValueError(msg)
                H, W = H // 2, W // 2
                if H < 1 or W < 1:
                    msg = "image too small for this many pooling layers"
                    raise RuntimeError(msg)
                dst = self._new_buf(H, W, cur.C)
                if kind == "avgpool":
                    # relu(maxpool(z)) == maxpool(relu(z)) lets a max pool pass a pending ReLU on to its consumer; for the
                    # mean that identity is false, so the node applies the ReLU itself (STV_RELU_IN) and nothing is pending
                    # behind it
                    self.nodes.append(Node("avgpool", cur, dst, relu_in=pending_relu, layer=i))
                    pending_relu = False
                else:
                    self.nodes.append(Node("pool", cur, dst, layer=i))
                cur = dst
                if pending_relu and i in tapped:   # relu(pool(z)) must exist as data
                    r = self._new_buf(H, W, cur.C)
                    self.nodes.append(Node("relu", cur, r, layer=i))
                    cur = r
                    pending_relu = False
            for idx in range(i, out_idx + 1):
                if idx in style_at:
                    assert cur is not None
                    tap = Tap("style", len(self.style_taps), cur)
                    cur.taps.append(tap)
                    self.style_taps.append(tap)
                if idx in content_at:
                    assert cur is not None
                    tap = Tap("content", len(self.content_taps), cur)
                    cur.taps.append(tap)
                    self.content_taps.append(tap)
            i = out_idx + 1

    # ------------------------------------------------------------------ fusion decisions
    def _decide(self, fuse_first_gram: bool) -> None:
        """Every fusion of the step, fixed before any op is emitted, with the buffers each one needs.  All of them exist
        as GPU kernels only (``device_form``); row strips pool their own rows and sum their own Gram ranges."""
        sw = self.switches
        whole = self.device_form and not self.halo
        for k, nd in enumerate(self.nodes):
            d = nd.dst
            nxt = self.nodes[k + 1] if k + 1 < len(self.nodes) else None
            tap = next((t for t in d.taps if t.kind == "style"), None)
            # a tapped first layer leaves the Gram slabs of its own output (no second pass over the map).
            # One slab per workgroup: pays once a workgroup walks >= 4 tiles of 8 x 32 pixels (1024^2: 8,
            # -11 us; at 512^2, 2 tiles each, the slab reduction costs what the separate pass did)
            if (nd.kind == "conv_first" and tap is not None and whole and fuse_first_gram and sw.fuse_gram_first and not self.guide
                    and ops.conv_first_gram_supported(d.H, d.W, nd.cin, d.C, self.dtype)
                    and (sw.fuse_gram_first == 2 or d.H * d.W >= 4 * 256 * ops.gram_ksplit(d.H * d.W, d.C))):
                tap.partials_fused = True
                self._partials(tap)
            # conv (ReLU in its epilogue) -> pool: one launch writes both maps.  Only where the conv
            # runs on the matrix cores, and not when the conv output itself is tapped pre-ReLU.
            if (nd.kind == "conv" and whole and sw.fuse_pool and nxt is not None and nxt.kind == "pool"
                    and d.relu_fused and nd.wf.dim() == 4):
                nxt.fused = True
                # the fused epilogue also leaves the arg-max map the pooling backward needs: one byte
                # per pooled element instead of re-reading the full-resolution activation
                if self.with_grad and sw.pool_idx:
                    nxt.idx = torch.empty(nxt.dst.H, nxt.dst.W, nxt.dst.C, device=self.device, dtype=torch.uint8)
                # The full-resolution map of a conv with the pool in its epilogue is dead in the bf16 step: the forward
                # pass continues from the pooled map, the backward pass routes through the arg-max byte map (its bit 2 is
                # the ReLU mask), and no tap sits on it - so it is not stored (conv1_2 at 1024^2: 134 MB of the
                # kernel's 312; STV_SKIP_PREPOOL=0 stores it, e.g. for the tests that look at every stored tensor).
                # fp32 (parity mode) keeps it: the parity tests read ReLU / arg-max decisions off the stored maps.
                d.stored = not (sw.skip_prepool and not d.taps and self.dtype == torch.bfloat16
                                and (not self.with_grad or nxt.idx is not None))
        self._place_losses()
        # the gradients of the reverse chain rotate through a few slabs (alloc_grads); 2: also on host tensors
        chain = all(nd.src is self.nodes[i - 1].dst for i, nd in enumerate(self.nodes) if i > 0)
        self.grad_arena = bool(sw.grad_arena and not self.halo and chain and (sw.grad_arena == 2 or self.device_form))
        if not self.with_grad:
            return
        for k, nd in enumerate(self.nodes):
            s = nd.src
            if nd.kind != "conv" or nd.wb.dim() != 4 or not self.device_form:
                continue
            # A Gram tap on the pre-ReLU output s: its gradient term F.S lands on the same buffer
            # as this dgrad.  One launch computes mask * dgrad + F.S (stv_conv_igemm_dual) instead
            # of a second launch that re-reads and re-writes s.grad.
            # (a guided tap has one term per region, each on a slab of its own: they stay 1x1 products)
            if sw.fuse_gram and not self.guide and not (s.relu_fused and s.taps) and s.C % (32 // s.act.element_size()) == 0:
                nd.gram = next((t for t in s.taps if t.kind == "style"), None)
            # s is a pooled map (arg-max byte map available, nothing else contributes to its gradient):
            # the dgrad's epilogue routes straight into the pre-pool gradient - no pooled-resolution
            # gradient, no pooling-backward pass.  Never into a buffer with a content tap: that gradient
            # may already hold the content term (stv_content_loss_grad), and a routed dgrad stores.
            pool_nd = self.nodes[k - 1]
            if self._routable(nd, pool_nd) and not any(t.kind == "content" for t in pool_nd.src.taps):
                nd.route = pool_nd

    def _place_losses(self) -> None:
        """Where the loss-side ops of every tap go (part of ``_decide``).  The Gram chain of a tap is a handful of
        latency-bound launches (partial sums, finish), and side by side in one grid (stv_gram_multi) several taps cost
        the slowest instead of the sum.  Deferring a tap to the end of the forward pass only pays while its activation
        is small enough to still sit in the Infinity Cache by then, so the decision is per tap: taps up to 48 MiB are
        batched behind the last conv, larger ones keep their place right behind their producer (512^2: all five taps
        batched; 1024^2: the three deep ones).  Same arithmetic and summation order either way (the batched kernels run
        the per-tap bodies).  A batch holds 2 to 8 taps and exists as a GPU kernel only."""
        sw = self.switches

        def small(tap: Tap) -> bool:
            return tap.buf.act.numel() * tap.buf.act.element_size() <= 48 * 2 ** 20
        tail = [tap for tap in self.style_taps if sw.loss_batch == "1" or (sw.loss_batch == "auto" and small(tap))]
        if not 2 <= len(tail) <= 8 or not self.device_form:
            tail = []
        for tap in tail:
            tap.in_tail = True
        # A LARGE tap keeps only its partial-sum pass behind its producer (that pass reads the activation: 67-134 MB at
        # 1024^2); its FINISH pass - a reduction of a few MB of fp32 slabs - joins the batched launch instead of being
        # a 6-7 us launch of its own (STV_GRAM_FIN_LATE=0: finish right behind the partial sums).  Same kernels' bodies,
        # same summation order per tap up to the grouping of a many-slab tap's slabs (8 instead of 32 per partial sum).
        if tail and sw.gram_fin_late and len(self.style_taps) <= 8:
            for tap in self.style_taps:
                tap.finish_late = not tap.in_tail
        for tap in self.content_taps:
            tap.in_tail = bool(tail) and len(tail) == len(self.style_taps)      # the content terms follow the batched launch
            # one content tap on the buffer: nothing else has written that buffer's gradient when the forward half gets there
            tap.grad_fused = (sw.fuse_content and self.with_grad
                              and sum(1 for t in tap.buf.taps if t.kind == "content") == 1)
        self.interleave = sw.loss_interleave      # loss ops right behind their producers; False: all behind the last conv

    def _routable(self, nd: Node, pool_nd: Node) -> bool:
        """The backward of `pool_nd`, the producer of conv `nd`'s input, can ride in `nd`'s dgrad: the input is a pooled
        map with an arg-max byte map, no tap on it, no mask, no Gram term on this launch."""
        s, d = nd.src, nd.dst
        return (self.switches.fuse_pool_bwd and pool_nd.kind == "pool" and pool_nd.idx is not None
                and self.dtype == torch.bfloat16 and not s.taps and not nd.relu_in and not s.relu_fused
                and pool_nd.src.H == 2 * s.H and pool_nd.src.W == 2 * s.W
                and ops.conv_fits(s.H, s.W, d.C, s.C, self.dtype, form=ops.CONV_ROUTE))

    def _partials(self, tap: Tap) -> torch.Tensor:
        """The split-K Gram slabs of a style tap (scratch, allocated at first use)."""
        if tap.partials is None:
            b = tap.buf
            tap.partials = torch.empty(ops.gram_ksplit(b.H * b.W, b.C), b.C, b.C, device=self.device, dtype=torch.float32)
        return tap.partials

    def attach_regions(self, maps: list[torch.Tensor], counts: list[list[int]]) -> None:
        """Spatial guidance: hand every style tap its label map (uint8 ``[H_l, W_l]``, values ``< guide`` or 255) and the
        pixel counts ``n_{l,r}`` of its regions (all > 0: guidance.check_counts).  The tap gets the slabs ``[Ra, H, W, C]``
        ``stv_mask_split`` fills and one child tap per region, ``order = l * Ra + r``, with the parent's placement."""
        if not self.guide or len(maps) != len(self.style_taps) or len(counts) != len(maps):
            msg = f"{len(maps)} label maps for {len(self.style_taps)} style taps of a schedule with {self.guide} regions"
            raise ValueError(msg)
        for tap, m, row in zip(self.style_taps, maps, counts, strict=True):
            b = tap.buf
            if tuple(m.shape) != (b.H, b.W) or m.dtype != torch.uint8 or len(row) != self.guide or min(row) < 1:
                msg = f"label map {tuple(m.shape)} {m.dtype} with counts {row} for a {b.H}x{b.W} style tap, {self.guide} regions"
                raise ValueError(msg)
            tap.labels = m.to(self.device).contiguous()
            tap.slabs = torch.empty(self.guide, b.H, b.W, b.C, device=self.device, dtype=self.dtype)
            tap.regions = [Tap("style", tap.order * self.guide + r, Buf(b.H, b.W, b.C, tap.slabs[r]), in_tail=tap.in_tail,
                               finish_late=tap.finish_late, norm=float(b.C * n), parent=tap) for r, n in enumerate(row)]

    def chains(self, tap: Tap) -> list[Tap]:
        """The taps that carry the Gram chains of style tap ``tap``: its regions under guidance, else the tap itself."""
        if self.guide:
            if tap.regions is None:
                msg = "internal: guided schedule without label maps (attach_regions)"
                raise RuntimeError(msg)
            return tap.regions
        return [tap]

    def all_chains(self) -> list[Tap]:
        return [c for tap in self.style_taps for c in self.chains(tap)]

    def mask_split_op(self, tap: Tap) -> StvOp:
        """The split of a guided style tap's activation into its region slabs (stv_mask_split)."""
        b = tap.buf
        return self.emit(op=OP_MASK_SPLIT, p0=b.act, p1=tap.labels, q0=tap.slabs, n=b.H * b.W, cin=b.C, cout=self.guide)

    # ------------------------------------------------------------------ op emission
    def emit(self, **kw) -> StvOp:
        """One op of this schedule's precision.  A tensor argument becomes its address in the op; the tensor itself
        is recorded under the field's name in ``op.refs``, so whoever holds the op holds its operands."""
        op = StvOp()
        # bf16x3: the ops that form products take STV_BF16X3, every other op runs on the fp32 storage as STV_F32
        op.dtype = ops.dtype_code(self.dtype, split=self.split and kw.get("op") in _PRODUCT_OPS)
        op.refs = {}
        for k, v in kw.items():
            if isinstance(v, torch.Tensor):
                op.refs[k] = v
                v = v.data_ptr()
            setattr(op, k, v)
        return op

    def forward_ops(self, x: torch.Tensor, after_node=None) -> list[StvOp]:
        """Forward schedule; ``after_node(node)`` may return extra ops to splice in right after a
        node's op (loss-side work that only needs that node's output)."""
        out = []
        for k, nd in enumerate(self.nodes):
            d = nd.dst
            if nd.fused:                 # its work rides in the preceding conv's epilogue
                if after_node is not None:
                    out += after_node(nd)
                continue
            if nd.kind == "conv_first":
                tap = next((t for t in d.taps if t.kind == "style"), None)
                slabs = tap.partials if tap is not None and tap.partials_fused else None
                out.append(self.emit(op=OP_CONV_FIRST_FWD, p0=x, p2=nd.bias, p3=nd.packed, q0=d.act, q1=slabs,
                                     H=d.H, W=d.W, cin=nd.cin, cout=d.C))
            elif nd.kind == "conv":
                pool = self.nodes[k + 1] if k + 1 < len(self.nodes) and self.nodes[k + 1].fused else None
                flags = ((RELU_IN if nd.relu_in else 0) | (RELU_OUT if d.relu_fused else 0)
                         | (W_BLOCKED if nd.wf.dim() == 4 else 0) | (0 if d.stored else POOL_ONLY))
                out.append(self.emit(op=OP_CONV, p0=nd.src.act, p1=nd.wf, p2=nd.bias, q0=d.act,
                                     q1=pool.dst.act if pool is not None else None,
                                     q2=pool.idx if pool is not None else None, H=d.H,
                                     W=d.W, cin=nd.cin, cout=d.C, taps=9, flags=flags))
            elif nd.kind == "pool":
                src_i = self.interior(nd.src.act)
                out.append(self.emit(op=OP_POOL_FWD, p0=src_i, q0=self.interior(d.act), H=src_i.shape[0], W=nd.src.W, cin=d.C))
            elif nd.kind == "avgpool":
                out.append(self.emit(op=OP_AVGPOOL_FWD, p0=nd.src.act, q0=d.act, H=nd.src.H, W=nd.src.W, cin=d.C,
                                     flags=RELU_IN if nd.relu_in else 0))
            else:
                out.append(self.emit(op=OP_RELU_FWD, p0=nd.src.act, q0=d.act, n=d.act.numel()))
            if after_node is not None:
                out += after_node(nd)
        return out

    def gram_ops(self, tap: Tap, *, gram_out: torch.Tensor | None, target: torch.Tensor | None,
                 loss_part: torch.Tensor | None, sgrad: torch.Tensor | None, coef: float,
                 coef_dev: torch.Tensor | None, partial: bool = True, finish: bool = True) -> list[StvOp]:
        b = tap.buf
        n = b.H * b.W
        out = []
        if partial and not tap.partials_fused:
            out.append(self.emit(op=OP_GRAM_PARTIAL, p0=b.act, q0=self._partials(tap), n=n, cin=b.C))
        if not finish:          # (the finish pass runs later, in a batched launch: gram_multi_op with partials_ready)
            return out
        out.append(self.emit(op=OP_GRAM_FINISH, p0=self._partials(tap), p1=target, p2=coef_dev, q0=gram_out, q1=loss_part,
                             q2=sgrad, n=n, cin=b.C, f0=GRAM_CLAMP_MAX, f1=float(b.C * n) if tap.norm is None else tap.norm, f2=coef))
        return out

    def gram_multi_op(self, specs: list[dict]) -> StvOp:
        """One batched Gram chain (stv_gram_multi) for several taps.  ``specs``: per tap the keyword
        arguments of :meth:`gram_ops` plus ``tap``.  The tap table is a host array the program copies."""
        table = (_lib.StvGramTap * len(specs))()
        refs: dict = {"p0": table}                  # the host array must outlive stv_program_create

        def ptr(t: torch.Tensor | None) -> int | None:
            if t is None:
                return None
            refs[len(refs)] = t
            return t.data_ptr()
        for e, sp in zip(table, specs, strict=True):
            tap = sp["tap"]
            b = tap.buf
            e.fill(n_pixels=b.H * b.W, channels=b.C, clamp_max=GRAM_CLAMP_MAX, coef=sp.get("coef", 0.0), norm=tap.norm,
                   F=None if (tap.partials_fused or sp.get("partials_ready")) else ptr(b.act), partials=ptr(self._partials(tap)),
                   **{k: ptr(sp.get(k)) for k in ("target", "gram_out", "loss_part", "sgrad", "coef_dev")})
        op = self.emit(op=OP_GRAM_MULTI, p0=ctypes.addressof(table), n=len(specs))
        op.refs = refs
        return op

    def alloc_grads(self) -> None:
        """Gradient storage of every activation.  The reverse schedule is a chain - the op of node i reads the gradient
        of node i's output and writes that of node i - 1's (i - 2's when the pooling backward rides in a dgrad's
        epilogue) - so on one GPU the gradients ROTATE through a few slabs instead of each owning memory that is touched
        once per step: the walk below follows the reverse schedule and hands every gradient the slab that was released
        LAST (the one the previous launch read), so a dgrad writes into lines that were in use one launch ago and are
        still on chip (Infinity Cache), not into lines last seen a step ago (`tools/cold_probe2.py`: a conv whose
        output range was just written runs 10-15 % faster than one storing to cold memory), and the working set of the
        backward pass shrinks from the sum of all gradients to two or three times the largest.  A buffer with a content
        tap keeps a tensor of its own (its gradient is written during the forward half).  Row strips keep one tensor
        per node (their halo rows are exchanged by address).  `STV_GRAD_ARENA=0`: one tensor per node everywhere;
        `backward_ops` checks, op by op, that no slab is read after somebody else wrote it."""
        todo = [nd for nd in self.nodes if nd.dst.grad is None]
        if not todo:
            return
        if not (self.grad_arena and len(todo) == len(self.nodes)):
            for nd in todo:              # strips: halo rows are read before anything wrote them -> start finite
                nd.dst.grad = torch.zeros_like(nd.dst.act) if self.halo else torch.empty_like(nd.dst.act)
            return
        own = {id(t.buf) for t in self.content_taps}
        slab_of: dict[int, int] = {}       # id(buf) -> slab number
        free: list[int] = []               # released slabs, the most recently released last
        n_slabs = 0

        def take(buf: Buf) -> None:
            nonlocal n_slabs
            if id(buf) in own or id(buf) in slab_of:
                return
            if free:
                slab_of[id(buf)] = free.pop()
            else:
                slab_of[id(buf)] = n_slabs
                n_slabs += 1

        def release(buf: Buf) -> None:
            if id(buf) in slab_of:
                free.append(slab_of[id(buf)])

        unused = {id(nd.route.dst) for nd in self.nodes if nd.route is not None}     # pooled maps whose gradient is never formed
        for nd in reversed(self.nodes):
            d = nd.dst
            if id(d) in unused:
                continue
            take(d)                        # (the deepest activation: first written by its own taps)
            if nd.kind != "conv_first":
                take(nd.route.src if nd.route is not None else nd.src)
            release(d)
        rot = [nd.dst for nd in self.nodes if id(nd.dst) in slab_of]
        nbytes = max((b.act.numel() * b.act.element_size() for b in rot), default=0)
        nbytes = (nbytes + 4095) // 4096 * 4096
        self._grad_slabs = torch.empty(max(n_slabs, 1), nbytes, device=self.device, dtype=torch.uint8)
        self._grad_slab_of = slab_of
        for nd in self.nodes:
            b = nd.dst
            if id(b) in slab_of:
                n = b.act.numel() * b.act.element_size()
                b.grad = self._grad_slabs[slab_of[id(b)], :n].view(b.act.dtype).view(b.act.shape)
            elif id(b) in unused:
                b.grad = self._grad_slabs[0, :0].view(b.act.dtype)       # never read or written
            else:
                b.grad = torch.empty_like(b.act)

    def backward_ops(self, x_grad: torch.Tensor, *, content_coef: float | list[float],
                     coef_dev: torch.Tensor | None, prewritten: tuple = ()) -> list[StvOp]:
        """Reverse schedule.  ``content_coef``: the coefficient of the content gradient, one for all content taps or one
        per tap (in tap order).  ``coef_dev`` (optional fp32 device vector, style terms
        first) holds upstream d(total)/d(loss_k) for the autograd path.  ``prewritten``: content taps whose
        gradient the forward half already WROTE into their buffer's ``grad`` (stv_content_loss_grad): no
        content-gradient pass for them, and whatever produces that gradient next accumulates onto it."""
        self.alloc_grads()
        out: list[StvOp] = []
        pre = {id(t) for t in prewritten}
        written: set[int] = {id(t.buf) for t in prewritten}

        def acc_flag(buf: Buf) -> int:
            return ACCUM if id(buf) in written else 0

        n_style = len(self.style_taps)
        tune = self.device.type == "cuda"      # (conv_tune measures on the device; its result is cached per shape)
        fused_taps = {id(nd.gram) for nd in self.nodes if nd.gram is not None}     # their dF = F.S rides in a dgrad
        routed = {id(nd.route) for nd in self.nodes if nd.route is not None}      # their backward rides in a dgrad
        # gradients that share a slab (alloc_grads): whoever reads one must find its own writer's data there
        slab_of = getattr(self, "_grad_slab_of", {})
        holder: dict[int, int] = {}      # slab -> id(buf) of its last writer

        def wr(buf: Buf) -> torch.Tensor:
            if id(buf) in slab_of:
                if id(buf) in written and holder.get(slab_of[id(buf)]) != id(buf):
                    raise RuntimeError("internal: gradient slab overwritten before its accumulation")
                holder[slab_of[id(buf)]] = id(buf)
            return buf.grad

        def rd(buf: Buf) -> torch.Tensor:
            if id(buf) in slab_of and holder.get(slab_of[id(buf)]) != id(buf):
                raise RuntimeError("internal: gradient slab overwritten before its reader ran")
            return buf.grad

        for nd in reversed(self.nodes):
            d = nd.dst
            if id(nd) in routed:         # its consumer's dgrad already wrote nd.src.grad
                continue
            for tap in d.taps:
                if id(tap) in fused_taps or id(tap) in pre:
                    continue
                if tap.kind == "style":
                    if tune:
                        ops.conv_tune(d.H, d.W, d.C, d.C, 1, self.dtype, split=self.split)
                    for c in self.chains(tap):      # (guided: dF += F_r . S_r per region, x = the region's slab)
                        out.append(self.emit(op=OP_CONV, p0=c.buf.act, p1=c.sgrad, q0=wr(d), H=d.H, W=d.W,
                                             cin=d.C, cout=d.C, taps=1, flags=acc_flag(d)))
                        written.add(id(d))
                else:
                    cd = coef_dev[n_style + tap.order:] if coef_dev is not None else None
                    coef = content_coef[tap.order] if isinstance(content_coef, (list, tuple)) else content_coef
                    out.append(self.emit(op=OP_CONTENT_GRAD, p0=d.act, p1=tap.target, p2=cd, q0=wr(d),
                                         n=d.act.numel(), f0=coef, flags=acc_flag(d)))
                written.add(id(d))
            if id(d) not in written:
                msg = "internal: activation without any gradient contribution"
                raise RuntimeError(msg)
            if d.relu_fused and d.taps:
                # taps see relu(z): mask the summed gradient once, in place
                out.append(self.emit(op=OP_RELU_BWD, p0=d.act, p1=rd(d), q0=d.grad, n=d.act.numel()))
            s = nd.src
            if nd.kind == "conv_first":
                out.append(self.emit(op=OP_CONV_FIRST_DGRAD, p0=rd(d), p2=nd.packed, q0=x_grad, H=d.H, W=d.W,
                                     cin=nd.cin, cout=d.C))
                continue
            mask_src = nd.relu_in or (s.relu_fused and not s.taps)
            if nd.kind == "conv":
                flags = (MASK if mask_src else 0) | acc_flag(s) | (W_BLOCKED if nd.wb.dim() == 4 else 0)
                if nd.route is not None:      # (s's own gradient is never formed)
                    ps = nd.route.src
                    if tune:
                        ops.conv_tune(s.H, s.W, d.C, s.C, ops.TUNE_ROUTE, self.dtype)
                    rflags = (MASK if (ps.relu_fused and not ps.taps) else 0) | W_BLOCKED | POOL_ROUTE
                    out.append(self.emit(op=OP_CONV, p0=rd(d), p1=nd.wb, p2=nd.route.idx, q1=wr(ps), H=s.H, W=s.W,
                                         cin=d.C, cout=s.C, taps=9, flags=rflags))
                    written.add(id(s))
                    written.add(id(ps))
                    continue
                if nd.gram is not None:
                    out.append(self.emit(op=OP_CONV, p0=rd(d), p1=nd.wb, p3=s.act if mask_src else None, q0=wr(s),
                                         q2=s.act, q3=nd.gram.sgrad, n=s.C, H=s.H, W=s.W, cin=d.C, cout=s.C, taps=9,
                                         flags=flags))
                else:
                    out.append(self.emit(op=OP_CONV, p0=rd(d), p1=nd.wb, p3=s.act if mask_src else None, q0=wr(s),
                                         H=s.H, W=s.W, cin=d.C, cout=s.C, taps=9, flags=flags))
            elif nd.kind == "pool":
                flags = (MASK if (s.relu_fused and not s.taps) else 0) | acc_flag(s)
                if nd.idx is not None:      # written by the forward conv that carried this pool
                    out.append(self.emit(op=OP_POOL_BWD, p0=nd.idx, p1=rd(d), q0=wr(s), H=s.H, W=s.W, cin=s.C,
                                         flags=flags | POOL_IDX))
                else:
                    s_i = self.interior(s.act)
                    out.append(self.emit(op=OP_POOL_BWD, p0=s_i, p1=self.interior(rd(d)), q0=self.interior(wr(s)),
                                         H=s_i.shape[0], W=s.W, cin=s.C, flags=flags))
            elif nd.kind == "avgpool":
                # the ReLU mask where the max pool op gets it, and where the node took a pending ReLU itself (ref = z)
                flags = (MASK if mask_src else 0) | acc_flag(s)
                out.append(self.emit(op=OP_AVGPOOL_BWD, p0=s.act if mask_src else None, p1=rd(d), q0=wr(s), H=s.H, W=s.W,
                                     cin=s.C, flags=flags))
            else:  # materialised relu
                out.append(self.emit(op=OP_RELU_BWD, p0=s.act, p1=rd(d), q0=wr(s), n=s.act.numel(),
                                     flags=acc_flag(s)))
            written.add(id(s))
        return out


def operands(op_list: list[StvOp]) -> list:
    """Everything the ops name by raw pointer: the tensors ``Schedule.emit`` recorded on them (and the host tap table
    of a batched Gram op)."""
    return [ref for o in op_list for ref in getattr(o, "refs", {}).values()]


class Program:
    """Owns a ``stv_program`` handle (host object inside libstv_hip.so) and keeps its ops' operands alive."""

    def __init__(self, op_list: list[StvOp], extra: tuple | list = ()) -> None:
        """``extra``: what must outlive the program without being an operand of one of its ops (or the operands of
        ops that were filled in by hand, without ``Schedule.emit``)."""
        self._keep = operands(op_list) + list(extra)
        arr = (StvOp * len(op_list))(*op_list)
        handle = ctypes.c_void_p()
        lib = _lib.load()
        _lib.check(lib.stv_program_create(arr, len(op_list), ctypes.byref(handle)), "stv_program_create")
        self._handle = handle
        self.n_ops = len(op_list)
        self.op_meta = [(int(o.op), int(o.H), int(o.W), int(o.cin), int(o.cout), int(o.taps), int(o.n))
                        for o in op_list]
        self.op_flags = [int(o.flags) for o in op_list]

    def run(self, use_graph: bool = False) -> None:
        lib = _lib.load()
        _lib.check(lib.stv_program_run(self._handle, 1 if use_graph else 0, torch.cuda.current_stream().cuda_stream),
                   "stv_program_run")

    def profile(self, reps: int = 1) -> list[float]:
        """Per-op device milliseconds (HIP events on the current stream); synchronises.  ``reps`` > 1
        launches every op that many times inside its event pair (timing only: buffers are then garbage)."""
        lib = _lib.load()
        out = (ctypes.c_float * self.n_ops)()
        _lib.check(lib.stv_program_profile_reps(self._handle, torch.cuda.current_stream().cuda_stream, int(reps), out, self.n_ops),
                   "stv_program_profile_reps")
        return list(out)

    def __del__(self) -> None:
        try:
            if self._handle:
                _lib.load().stv_program_destroy(self._handle)
                self._handle = None
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass
