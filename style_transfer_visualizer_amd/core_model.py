"""MI355X-native model + losses behind the reference's ``core_model`` API.

Public surface mirrors /root/reference/src/style_transfer_visualizer/core_model.py
(``gram_matrix`` :29, ``initialize_input`` :66, ``initialize_vgg`` :103,
``create_feature_blocks`` :120, ``StyleContentModel`` :149,
``prepare_model_and_input`` :331) with the same argument meaning and error
texts, but every forward/backward FLOP runs in hand-written HIP kernels from
``libstv_hip.so``; PyTorch only owns memory and streams.  There is no eager or
CPU fallback: tensors must live on the GPU and the library must be built.
"""
from __future__ import annotations

import copy
import hashlib
import os
import threading
from collections.abc import Callable
from pathlib import Path
from typing import NamedTuple
from urllib.parse import urlparse

import torch
from torch import nn
from torch.nn import functional as F

from . import _lib, guidance, ops, plan, style_mix, synthetic
from .constants import GRAM_MATRIX_CLAMP_MAX
from .logging_utils import logger

VGG19_WEIGHTS_URL = "https://download.pytorch.org/models/vgg19-dcbb9e9d.pth"
# storage dtype per precision; "bf16x3" stores fp32 and forms the conv / Gram products from split bf16 operands
_PRECISIONS = {"fp32": torch.float32, "bf16": torch.bfloat16, "bf16x3": torch.float32}
_SPLIT_PRECISIONS = frozenset({"bf16x3"})

# The two torchvision names the reference imports at module level (core_model.py:12) and its tests patch.  Without
# torchvision (this image) ``vgg19`` is None - ``initialize_vgg`` then builds the same stack itself and loads the
# cached checkpoint - and ``VGG19_Weights`` only carries the URL the cache file name is derived from.
try:
    from torchvision.models import VGG19_Weights, vgg19
except ImportError:
    vgg19 = None

    class _WeightsEntry:
        url = VGG19_WEIGHTS_URL

    class VGG19_Weights:  # noqa: N801
        IMAGENET1K_V1 = _WeightsEntry()
        DEFAULT = IMAGENET1K_V1


def _precision_name(precision: str | None) -> str:
    name = precision or os.environ.get("STV_PRECISION", "fp32")
    if name not in _PRECISIONS:
        msg = f"Unsupported precision: {name} (expected one of {sorted(_PRECISIONS)})"
        raise ValueError(msg)
    return name


def resolve_precision(precision: str | None = None) -> torch.dtype:
    """Activation storage dtype: fp32 = parity mode (default), bf16 = performance mode, bf16x3 = fp32 storage."""
    return _PRECISIONS[_precision_name(precision)]


def resolve_split(precision: str | None = None) -> bool:
    """True for bf16x3: conv and Gram products formed as ah*bh + ah*bl + al*bh on the bf16 matrix cores."""
    return _precision_name(precision) in _SPLIT_PRECISIONS


# --------------------------------------------------------------------------- gram
class _GramFn(torch.autograd.Function):
    """clamp(F F^T, max)/(b*c*h*w) for an NCHW tensor, via the split-K MFMA Gram kernels.

    Any ``b*c`` is accepted, like the reference: the channel axis is zero-padded to the kernels'
    granularity (8) - padded channels only add zero rows/columns, which are sliced away again.
    """

    _PAD = 8

    @staticmethod
    def forward(ctx, tensor: torch.Tensor, clamp_max: float) -> torch.Tensor:
        if tensor.dim() != 4:
            msg = f"gram_matrix expects a [batch, channels, h, w] tensor, got shape {tuple(tensor.shape)}"
            raise ValueError(msg)
        b, c, h, w = tensor.shape
        C, n = b * c, h * w
        Cp = -(-C // _GramFn._PAD) * _GramFn._PAD
        feat = tensor.detach().reshape(C, n).t().float()                 # [N, C] (NHWC view)
        if Cp != C:
            feat = torch.nn.functional.pad(feat, (0, Cp - C))
        feat = feat.contiguous()
        norm = float(C * n)
        partials = ops.gram_partial(feat)
        gram = torch.empty(Cp, Cp, device=tensor.device, dtype=torch.float32)
        raw = torch.empty(Cp, Cp, device=tensor.device, dtype=torch.float32)
        ops.gram_finish(partials, n, Cp, gram_out=gram, clamp_max=clamp_max, norm=norm)
        ops.gram_finish(partials, n, Cp, gram_out=raw, clamp_max=float("inf"), norm=1.0)    # R itself
        ctx.save_for_backward(feat, raw)
        ctx.meta = (b, c, h, w, clamp_max)
        return gram[:C, :C].to(tensor.dtype)

    @staticmethod
    def backward(ctx, gout: torch.Tensor):
        feat, raw = ctx.saved_tensors
        b, c, h, w, clamp_max = ctx.meta
        C, n = b * c, h * w
        Cp = raw.shape[0]
        g = torch.zeros(Cp, Cp, device=raw.device, dtype=torch.float32)
        g[:C, :C] = gout.float()
        seed = g * (raw <= clamp_max).float() / float(C * n)           # clamp passes gradient where R <= max
        seed = (seed + seed.t()).contiguous()                           # dF^T = F^T (dR + dR^T)
        d_feat = ops.conv_igemm(feat.reshape(1, n, Cp), seed.reshape(1, Cp, Cp))
        return d_feat.reshape(n, Cp)[:, :C].t().reshape(b, c, h, w).to(gout.dtype), None


def gram_matrix(tensor: torch.Tensor, clamp_max: float = GRAM_MATRIX_CLAMP_MAX) -> torch.Tensor:
    """Gram matrix of ``[batch, channels, h, w]`` features (batch folded into channels).

    Same arithmetic as reference core_model.py:56-63: ``mm(F, F.t()).clamp(max=clamp_max)``
    then ``div(b*c*h*w)``; returns ``[b*c, b*c]``.
    """
    return _GramFn.apply(tensor, float(clamp_max))


# ---------------------------------------------------------------- total variation
def total_variation(x: torch.Tensor) -> torch.Tensor:
    """Total variation of an image ``[1, C, H, W]`` (or ``[C, H, W]``), differentiable, on any device:

        TV(x) = ( sum (x[c,y+1,x] - x[c,y,x])^2 + sum (x[c,y,x+1] - x[c,y,x])^2 ) / (C*H*W)

    Differences never cross a row end or a channel plane; ``H = 1`` / ``W = 1`` have none in that direction.  The
    fused step forms ``tv_w * TV`` and its gradient in the ``stv_tv`` kernel (``StyleContentModel.loss_and_grad(...,
    tv_w=)``); this is the same definition as torch ops, for models without a fused step and as documentation."""
    if x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[0] != 1):
        msg = f"total_variation expects an image of shape [1, C, H, W] or [C, H, W], got {tuple(x.shape)}"
        raise ValueError(msg)
    dy = x[..., 1:, :] - x[..., :-1, :]
    dx = x[..., :, 1:] - x[..., :, :-1]
    return (dy.square().sum() + dx.square().sum()) / x.numel()


def _fp32(v: float) -> float:
    """``v`` (a double formed on the host) rounded to fp32 once, as the kernels receive it."""
    return float(torch.tensor(v, dtype=torch.float64).to(torch.float32))


def tv_scale(tv_w: float, C: int, H: int, W: int) -> float:
    """The combine-table scale of the TV term: ``fp32(tv_w / (C*H*W))`` - the weight rides in the scale."""
    return _fp32(float(tv_w) / float(C * H * W))


def tv_coef(tv_w: float, C: int, H: int, W: int) -> float:
    """The gradient coefficient of the TV term: ``fp32(tv_w * 2 / (C*H*W))``."""
    return _fp32(float(tv_w) * 2.0 / float(C * H * W))


# ---------------------------------------------------------------- Laplacian loss
LAP_MAX_POOLS = 4


def check_lap_pools(pools) -> tuple[int, ...]:
    """The pool sizes of the Laplacian loss as a tuple: one to ``LAP_MAX_POOLS`` of them, each a power of two from 1 to 32,
    no duplicates (an empty sequence or ``None``: no pools, the term is not available)."""
    if pools is None:
        return ()
    out = tuple(pools)
    if any(isinstance(v, bool) or not isinstance(v, int) or v not in _lib.LAP_POOLS for v in out):
        msg = f"lap_pools must be powers of two from 1 to 32 (one of {list(_lib.LAP_POOLS)}), got {list(out)}"
        raise ValueError(msg)
    if len(out) > LAP_MAX_POOLS or len(set(out)) != len(out):
        msg = f"lap_pools takes one to {LAP_MAX_POOLS} different pool sizes, got {list(out)}"
        raise ValueError(msg)
    return out


def check_lap_fits(pools, H: int, W: int, where: str = "") -> None:
    """Every pool needs a pooled grid of at least 2 x 2 cells at the image size, or the Laplacian has nothing to difference."""
    for p in pools:
        if min(H, W) // p < 2:
            msg = (f"lap_pools: pool size {p} leaves {H // p} x {W // p} cells of a {H} x {W} image{where}; "
                   "at least 2 x 2 are needed (use a smaller pool size or a larger image)")
            raise ValueError(msg)


def laplacian_loss(x: torch.Tensor, content: torch.Tensor, pool: int) -> torch.Tensor:
    """Laplacian loss of an image against the content image (``[1, C, H, W]`` or ``[C, H, W]``, same shape), differentiable, on
    any device (Li et al., "Laplacian-steered neural style transfer", 2017):

        e = avg_pool(x, pool) - avg_pool(content, pool);   r = L e;   lap = sum r^2 / (C * (H//pool) * (W//pool))

    with ``L`` the ``[[0,-1,0],[-1,4,-1],[0,-1,0]]`` filter per channel under replicate padding - the sum over the existing
    4-neighbours ``n`` of ``(e - n)``.  The fused step forms ``lap_w * sum_p lap_p`` and its gradient in the ``stv_lap`` kernel
    (``StyleContentModel(..., lap_pools=).loss_and_grad(..., lap_w=)``); this is the same definition as torch ops."""
    if x.shape != content.shape or x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[0] != 1):
        msg = (f"laplacian_loss expects two images of one shape [1, C, H, W] or [C, H, W], got {tuple(x.shape)} "
               f"and {tuple(content.shape)}")
        raise ValueError(msg)
    (pool,) = check_lap_pools((pool,))
    C = int(x.shape[-3])
    a, b = (t.reshape(1, C, t.shape[-2], t.shape[-1]) for t in (x, content))
    e = F.avg_pool2d(a, pool) - F.avg_pool2d(b, pool)
    kernel = torch.tensor([[0.0, -1.0, 0.0], [-1.0, 4.0, -1.0], [0.0, -1.0, 0.0]], dtype=e.dtype, device=e.device)
    r = F.conv2d(F.pad(e, (1, 1, 1, 1), mode="replicate"), kernel.expand(C, 1, 3, 3), groups=C)
    return r.square().sum() / r.numel()


def lap_scale(lap_w: float, C: int, Hp: int, Wp: int) -> float:
    """The combine-table scale of one pool's Laplacian term: ``fp32(lap_w / (C*Hp*Wp))`` - the weight rides in the scale."""
    return _fp32(float(lap_w) / float(C * Hp * Wp))


def lap_coef(lap_w: float, C: int, Hp: int, Wp: int, pool: int) -> float:
    """The gradient coefficient of one pool's Laplacian term: ``fp32(lap_w * 2 / (C*Hp*Wp*pool*pool))``."""
    return _fp32(float(lap_w) * 2.0 / float(C * Hp * Wp * pool * pool))


# ------------------------------------------------------------------- initialisation
def initialize_input(content_img: torch.Tensor, method: str) -> torch.Tensor:
    """Start image for the optimisation (reference core_model.py:66-100)."""
    if not isinstance(content_img, torch.Tensor):
        msg = f"Expected content_img to be a Tensor, got {type(content_img)}"
        raise TypeError(msg)
    if method == "content":
        start = content_img.clone()
    elif method == "random":
        if content_img.is_cuda:
            # The reference's --device cpu path (the one north_star compares with) draws randn_like on the
            # CPU generator; a draw on the GPU generator could never match it on the same --seed.  Same
            # generator, same shape/dtype -> the same values, then one copy to the device.
            start = torch.randn(content_img.shape, dtype=content_img.dtype).to(content_img.device)
        else:
            start = torch.randn_like(content_img)
    elif method == "white":
        start = torch.ones_like(content_img)
    else:
        msg = f"Unsupported initialization method: {method}"
        raise ValueError(msg)
    return start.requires_grad_(True)  # noqa: FBT003


def build_vgg_features(weights: list[tuple[torch.Tensor, torch.Tensor]] | None = None,
                       cfg: tuple = synthetic.VGG19_CFG) -> nn.Sequential:
    """torchvision-free ``vgg19().features`` topology (conv3x3 pad 1 / ReLU / MaxPool 2x2)."""
    layers: list[nn.Module] = []
    cin = 3
    it = iter(weights) if weights is not None else None
    for v in cfg:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            continue
        conv = nn.Conv2d(cin, int(v), kernel_size=3, padding=1)
        if it is not None:
            w, b = next(it)
            with torch.no_grad():
                conv.weight.copy_(w)
                conv.bias.copy_(b)
        layers += [conv, nn.ReLU(inplace=True)]
        cin = int(v)
    return nn.Sequential(*layers)


def consume_classifier_init() -> None:
    """Advance the CPU generator as constructing the rest of torchvision's VGG19 would.

    The reference builds ``vgg19(weights=IMAGENET1K_V1)`` (core_model.py:114) AFTER seeding
    (main.py:36) and BEFORE drawing the ``random`` start image (core_model.py:92): torchvision's
    ``_vgg`` runs ``VGG(make_layers(cfg), init_weights=False)``, i.e. the default ``reset_parameters`` of
    16 ``Conv2d`` (kaiming_uniform_ weight + uniform_ bias each, in layer order) and then of the classifier's
    ``Linear(25088, 4096)``, ``Linear(4096, 4096)``, ``Linear(4096, 1000)``; the checkpoint is loaded over them.
    ``build_vgg_features`` constructs the same 16 ``Conv2d`` in the same order; this function does the three
    ``Linear`` (by constructing and dropping them: identical consumption by construction, ~0.5 GB / 1 s once
    per run), so that ``randn`` afterwards continues where the reference's would.
    """
    for fan_in, fan_out in ((512 * 7 * 7, 4096), (4096, 4096), (4096, 1000)):
        nn.Linear(fan_in, fan_out)


# initialize_vgg() of the torchvision-free branches costs 0.75 s per call (tools/setup_profile.py: 143 M uniform draws that
# only exist to leave the CPU generator where torchvision's constructor would, 16 weight copies, the checkpoint load) - four
# times the 0.17 s a 200-step run at 512^2 takes, once per image of a batch.  Both results are functions of their inputs: the
# stack of (weight source), the generator state after of (generator state before).  So the process keeps the stack it built
# (a CPU master, handed out as a deep copy) and, per generator state it has seen, the state construction left behind; a
# second call from the same state (style_transfer reseeds per image) restores that state instead of drawing again.
# STV_VGG_CACHE=0: always construct.
_VGG_CACHE: dict = {}
_VGG_CACHE_LOCK = threading.Lock()


def clear_vgg_cache() -> None:
    with _VGG_CACHE_LOCK:
        _VGG_CACHE.clear()


def _vgg_cache_get(key: tuple) -> nn.Module | None:
    if os.environ.get("STV_VGG_CACHE", "1") == "0":
        return None
    digest = hashlib.sha1(torch.get_rng_state().numpy().tobytes()).digest()
    with _VGG_CACHE_LOCK:
        hit = _VGG_CACHE.get(key)
        after = hit["rng"].get(digest) if hit is not None else None
    if after is None:
        return None
    torch.set_rng_state(after.clone())
    return copy.deepcopy(hit["master"])


def _vgg_cache_put(key: tuple, before: torch.Tensor, vgg: nn.Module) -> None:
    if os.environ.get("STV_VGG_CACHE", "1") == "0":
        return
    digest = hashlib.sha1(before.numpy().tobytes()).digest()
    with _VGG_CACHE_LOCK:
        hit = _VGG_CACHE.get(key)
        if hit is None:
            if len(_VGG_CACHE) >= 2:                      # (a stack is 80 MB of host memory)
                _VGG_CACHE.pop(next(iter(_VGG_CACHE)))
            hit = _VGG_CACHE[key] = {"master": copy.deepcopy(vgg), "rng": {}}
        if len(hit["rng"]) >= 16:
            hit["rng"].pop(next(iter(hit["rng"])))
        hit["rng"][digest] = torch.get_rng_state()


def initialize_vgg() -> nn.Module:
    """Frozen VGG19 feature stack (reference core_model.py:103-117).

    Order of preference: torchvision with IMAGENET1K_V1 weights (as the
    reference); the cached ``vgg19-dcbb9e9d.pth`` loaded into the
    torchvision-free topology; deterministic synthetic weights when
    ``STV_SYNTHETIC_WEIGHTS=<seed>`` is set (benchmarks / offline boxes).
    The two torchvision-free branches are served from a per-process cache when weight source AND generator state
    have been seen before (same stack, same generator state afterwards as constructing again).
    """
    cache_dir = Path(torch.hub.get_dir()) / "checkpoints"
    cache_path = cache_dir / Path(urlparse(VGG19_Weights.IMAGENET1K_V1.url).path).name
    synth = os.environ.get("STV_SYNTHETIC_WEIGHTS")
    key = None
    if synth is not None:
        key = ("synthetic", synth)
    elif vgg19 is None and cache_path.exists():
        st = cache_path.stat()
        key = ("checkpoint", str(cache_path), st.st_mtime_ns, st.st_size)
    if key is not None:
        cached = _vgg_cache_get(key)
        if cached is not None:
            logger.info("Using synthetic VGG19 weights (seed %s)", synth) if synth is not None else logger.info(
                "Using cached VGG19 weights at %s", cache_path)
            return cached
    rng_before = torch.get_rng_state()
    if synth is not None:
        logger.info("Using synthetic VGG19 weights (seed %s)", synth)
        vgg = build_vgg_features(synthetic.synthetic_conv_weights(int(synth)))
        consume_classifier_init()
    else:
        if cache_path.exists():
            logger.info("Using cached VGG19 weights at %s", cache_path)
        else:
            logger.info("Downloading VGG19 weights to %s", cache_path)
        if vgg19 is not None:       # torchvision's constructor - or whatever a caller put under that name
            vgg = vgg19(weights=VGG19_Weights.IMAGENET1K_V1).features
        else:
            if not cache_path.exists():
                msg = (f"torchvision is not installed and {cache_path} is absent: place the IMAGENET1K_V1 "
                       "checkpoint there, or set STV_SYNTHETIC_WEIGHTS=<seed> for synthetic weights.")
                raise RuntimeError(msg) from None
            vgg = build_vgg_features()
            consume_classifier_init()
            state = torch.load(cache_path, map_location="cpu", weights_only=True)
            feats = {k[len("features."):]: v for k, v in state.items() if k.startswith("features.")}
            vgg.load_state_dict(feats)
    vgg = vgg.eval()
    for p in vgg.parameters():
        p.requires_grad_(False)  # noqa: FBT003
    if key is not None:
        _vgg_cache_put(key, rng_before, vgg)
    return vgg


POOLINGS = ("max", "avg")


def check_pooling(pooling) -> str:
    """The pooling kind of the feature stack, ``"max"`` (VGG as trained) or ``"avg"`` (Gatys et al.: the mean); any other
    value is refused, with the value named."""
    if not isinstance(pooling, str) or pooling not in POOLINGS:
        msg = f"pooling must be one of {list(POOLINGS)}, got {pooling!r}"
        raise ValueError(msg)
    return pooling


def replace_pooling(vgg: nn.Module, pooling: str) -> nn.Module:
    """``pooling = "avg"``: a stack with every ``MaxPool2d`` of ``vgg`` replaced by ``AvgPool2d(2, 2)`` - the other modules
    are shared, not copied (a cached stack stays as it is), indices keep their meaning, no parameter is added and no
    generator draw is made; the new stack is in the mode (train / eval) of ``vgg``.  ``"max"``: ``vgg`` itself."""
    if check_pooling(pooling) == "max":
        return vgg
    out = nn.Sequential(*[nn.AvgPool2d(kernel_size=2, stride=2) if isinstance(layer, nn.MaxPool2d) else layer
                          for layer in vgg.children()])
    return out.train(vgg.training)          # (the mode of the stack it stands in for: initialize_vgg() returns .eval())


def create_feature_blocks(
    vgg: nn.Module,
    style_layers: list[int],
    content_layers: list[int],
) -> tuple[nn.ModuleList, list[int], list[int]]:
    """Slice the stack after every tapped index (reference core_model.py:120-146).

    Returns ``(blocks, content_ids, style_ids)``; trailing untapped layers are
    dropped and every ReLU is made out-of-place.
    """
    blocks = nn.ModuleList()
    content_ids: list[int] = []
    style_ids: list[int] = []
    pending = nn.Sequential()
    for idx, layer in enumerate(vgg.children()):
        pending.add_module(str(idx), nn.ReLU(inplace=False) if isinstance(layer, nn.ReLU) else layer)
        hit_style, hit_content = idx in style_layers, idx in content_layers
        if hit_style or hit_content:
            blocks.append(pending)
            pending = nn.Sequential()
        if hit_style:
            style_ids.append(len(blocks) - 1)
        if hit_content:
            content_ids.append(len(blocks) - 1)
    return blocks, content_ids, style_ids


# --------------------------------------------------------------------------- engine
class _Term(NamedTuple):
    """One extra term of a step (``_Engine.extra_terms``): its loss partials in ``parts``, the scale of its combine row, and
    its two ops as ``loss_op(x)`` and ``grad_op(x, grad)``."""

    kind: str           # "tv" | "lap"
    off: int
    cnt: int
    scale: float
    loss_op: Callable
    grad_op: Callable


class _Head(NamedTuple):
    """The combine op's operands (``_Engine.head``) and where the extra terms' slots of ``losses`` are."""

    table: torch.Tensor
    scale: torch.Tensor
    losses: torch.Tensor
    tv: int | None          # the row of the total-variation term
    lap: slice | None       # the rows of the Laplacian terms, one per pool


class _Engine:
    """Buffers + command buffers for one (model, image size, device)."""

    def __init__(self, layers: list[nn.Module], style_at: list[int], content_at: list[int],
                 H: int, W: int, dtype: torch.dtype, device: torch.device, *, split: bool = False,
                 assume_device: bool = False, lap_pools: tuple = (), guide: guidance.Guide | None = None) -> None:
        """``assume_device``: as for ``plan.Schedule`` - the step a GPU engine builds, on host tensors, to be inspected.
        ``lap_pools``: the pool sizes of the Laplacian loss; the engine then owns, per pool, a target, a residual scratch and
        ``LAP_LOSS_PARTS`` loss partials.
        ``guide`` (spatial guidance): every style tap runs one Gram chain per active region on the slabs ``stv_mask_split``
        fills; the combine table has one kind-0 row per (layer, region), in layer then region order, and the style targets
        are ``[Ra, C, C]`` per layer.  ``None``: no allocation, no op, the engine as it always was."""
        self.layers, self.style_at, self.content_at = layers, style_at, content_at
        self.H, self.W, self.dtype, self.device = H, W, dtype, device
        self.split = split
        # (the A/B switches as they stand now, for every program of this engine)
        self.sched = plan.Schedule(layers, style_at, content_at, H, W, dtype, device, with_grad=True, split=split,
                                   switches=plan.Switches.from_env(), assume_device=assume_device,
                                   **({"guide": guide.n} if guide is not None else {}))
        s = self.sched
        self.guide = guide
        # the pooling kind of the stack, part of every step's program key ("max": the key as it always was)
        self.pooling = "avg" if any(nd.kind == "avgpool" for nd in s.nodes) else "max"
        self.n_style, self.n_content = len(s.style_taps), len(s.content_taps)
        if guide is not None:
            if tuple(guide.content_labels.shape) != (H, W):
                msg = f"content_labels are {tuple(guide.content_labels.shape)}, the image is {(H, W)}"
                raise ValueError(msg)
            guidance.check_rows(self.n_style, guide.n, self.n_content + 1 + len(lap_pools))
            maps = guidance.tap_maps(guide.content_labels, [(t.buf.H, t.buf.W) for t in s.style_taps])
            s.attach_regions(maps, guidance.check_counts(maps, guide.n, "content", guide.active, style_at))
        # one combine row per Gram chain: per style tap, or per (tap, region) under guidance
        self.n_style_rows = len(s.all_chains())
        n_terms = self.n_style_rows + self.n_content
        off = 0
        for tap in s.all_chains():
            tap.parts_off, tap.parts_cnt = off, ops.gram_loss_parts(tap.buf.C)
            off += tap.parts_cnt
            tap.sgrad = torch.zeros(1, tap.buf.C, tap.buf.C, device=device, dtype=dtype)
        for tap in s.content_taps:
            tap.parts_off, tap.parts_cnt = off, ops._lib.CONTENT_LOSS_PARTS
            off += tap.parts_cnt
        rows, scale = self._base_rows(None)
        # (the partial sums of the total-variation term sit behind every tap's; only a tv_w > 0 step reads or writes them)
        self.tv_parts_off = off
        # (and those of the Laplacian terms, one block per pool, behind them: an engine without pools allocates none)
        self.lap_pools = check_lap_pools(lap_pools)
        self.lap_parts_off = off + _lib.TV_LOSS_PARTS
        self.parts = torch.zeros(self.lap_parts_off + len(self.lap_pools) * _lib.LAP_LOSS_PARTS, device=device, dtype=torch.float32)
        self.table = torch.tensor(rows, dtype=torch.int32, device=device).reshape(-1, 3)
        self.scale = torch.tensor(scale, dtype=torch.float32, device=device)
        self.losses = torch.zeros(max(n_terms, 1), device=device, dtype=torch.float32)
        self.scores = torch.zeros(4, device=device, dtype=torch.float32)
        self.coef_buf = torch.ones(max(n_terms, 1), device=device, dtype=torch.float32)
        self._programs: dict = {}
        self._heads: dict = {}           # (tv_w, lap_w, layer weights) -> _Head of the combine op of any step but the plain one
        self._target_cache: dict = {}    # converted content targets (_nhwc_of)
        self._region_head: tuple | None = None      # (scale, losses, scores) of last_region_losses()' own combine launch
        self.image_channels = int(s.nodes[0].cin)
        check_lap_fits(self.lap_pools, H, W)
        cells = [(self.image_channels, H // p, W // p) for p in self.lap_pools]
        self.lap_targets: list[torch.Tensor | None] = [None] * len(cells)
        self.lap_resid = [torch.zeros(shape, device=device, dtype=torch.float32) for shape in cells]
        self.use_graph = s.switches.hip_graph
        # Every evaluation overwrites the shared activation buffers; an autograd backward is only
        # valid against the forward that filled them last.  `generation` counts evaluations.
        self.generation = 0
        self._stage: torch.Tensor | None = None      # fp32 contiguous copy of a non-conforming input

    def _chain_weights(self, tap, layer_w: tuple | None) -> tuple[float, float]:
        """``(w_l, lambda_r)`` of a Gram chain's tap: the weight of its style layer (1.0 without layer weights) and of its
        region (1.0 without guidance).  A factor of 1.0 is exact, so the products below are those of the plain step."""
        layer = tap if tap.parent is None else tap.parent      # (a region's chain hangs under its layer's tap)
        w = 1.0 if layer_w is None else float(layer_w[layer.order])
        return w, 1.0 if self.guide is None else self.guide.weights[tap.order % self.guide.n]

    def _style_scale(self, tap, layer_w: tuple | None) -> float:
        """The combine scale of a Gram chain's row, formed in double: ``w_l * lambda_r / C^2``."""
        w, lam = self._chain_weights(tap, layer_w)
        return w * lam / float(tap.buf.C * tap.buf.C)

    def _base_rows(self, layer_w: tuple | None) -> tuple[list, list]:
        """Rows ``[offset, count, kind]`` and scales of the combine table's taps: the Gram chains (kind 0), then the content
        taps (kind 1, ``1 / numel``)."""
        s = self.sched
        rows = [[t.parts_off, t.parts_cnt, 0] for t in s.all_chains()] + [[t.parts_off, t.parts_cnt, 1] for t in s.content_taps]
        scale = [self._style_scale(t, layer_w) for t in s.all_chains()]
        return rows, scale + [1.0 / float(t.buf.act.numel()) for t in s.content_taps]

    # -- op list pieces -------------------------------------------------------
    def _forward_with_losses(self, x: torch.Tensor, *, style_coef: float, with_seed: bool,
                             content_coef: float | None = None, layer_w: tuple | None = None) -> list:
        """Forward pass with the loss-side ops of every tap where ``Schedule._decide`` placed them: spliced in right
        behind the op that produces the tapped activation (while it is still L2 / Infinity-Cache resident), or in the
        tail - one batched Gram launch, then the content terms that follow it.  ``content_coef`` (the fused step: the
        coefficient is known) lets a content tap form loss and gradient in one pass.  ``layer_w`` (one weight per style tap, in
        tap order): tap ``l`` is seeded with ``style_coef * layer_w[l]``, the product formed here in double and rounded to
        fp32 where ``style_coef`` alone is; ``None``: every tap with ``style_coef``."""
        s = self.sched

        def coef_of(tap) -> float:      # style_w * w_l * lambda_r, left to right, in double
            w, lam = self._chain_weights(tap, layer_w)
            return style_coef * w * lam
        if content_coef is not None:
            s.alloc_grads()          # the content term's gradient is written during the forward half

        def chain(tap) -> list:
            if tap.kind == "style":
                return s.gram_ops(tap, gram_out=None, target=tap.target, loss_part=self.parts[tap.parts_off:],
                                  sgrad=tap.sgrad if with_seed else None, coef=coef_of(tap), coef_dev=None)
            fused = content_coef is not None and tap.grad_fused
            return [s.emit(op=plan.OP_CONTENT_LOSS, p0=tap.buf.act, p1=tap.target, q0=self.parts[tap.parts_off:],
                           q1=tap.buf.grad if fused else None, n=tap.buf.act.numel(), f0=content_coef if fused else 0.0)]
        batch = [dict(tap=tap, target=tap.target, loss_part=self.parts[tap.parts_off:],
                      sgrad=tap.sgrad if with_seed else None, coef=coef_of(tap), partials_ready=tap.finish_late)
                 for tap in s.all_chains() if tap.in_tail or tap.finish_late]
        # (a batched launch takes 8 entries; without guidance a batch never holds more)
        tail = [s.gram_multi_op(batch[i:i + 8]) for i in range(0, len(batch), 8)]
        for tap in s.content_taps:
            if tap.in_tail:
                tail += chain(tap)

        def after(node) -> list:
            out = []
            taps = []
            for tap in node.dst.taps:      # (guided: the split right behind the producer, then the regions' chains)
                if tap.kind == "style" and s.guide:
                    out.append(s.mask_split_op(tap))
                taps += s.chains(tap) if tap.kind == "style" else [tap]
            for tap in taps:
                if tap.finish_late:      # partial sums here (unless the first layer left them itself), finish in the tail
                    out += s.gram_ops(tap, gram_out=None, target=None, loss_part=None, sgrad=None, coef=0.0,
                                      coef_dev=None, finish=False)
                elif not tap.in_tail:
                    out += chain(tap)
            return out
        if s.interleave:
            return s.forward_ops(x, after_node=after) + tail
        return s.forward_ops(x) + [op for node in s.nodes for op in after(node)] + tail

    def _tv_op(self, x: torch.Tensor, *, loss: bool = False, grad: torch.Tensor | None = None, tv_w: float = 0.0):
        """The total-variation op on the image: its loss partials (``loss``), or ``grad += coef * sum(x - n)``."""
        return self.sched.emit(op=_lib.OP_TV, p0=x, q0=self.parts[self.tv_parts_off:] if loss else None, q1=grad,
                               cin=self.image_channels, H=self.H, W=self.W,
                               f0=tv_coef(tv_w, self.image_channels, self.H, self.W) if grad is not None else 0.0,
                               flags=_lib.ACCUM if grad is not None else 0)

    def _lap_op(self, k: int, x: torch.Tensor, *, grad: torch.Tensor | None = None, lap_w: float = 0.0):
        """The Laplacian op of pool ``k`` on the image: the LOSS form (residual and loss partials), or with ``grad`` the
        GRAD form, ``grad += coef * (L r)`` from the residual the LOSS form left."""
        p, resid = self.lap_pools[k], self.lap_resid[k]
        common = dict(op=_lib.OP_LAP, q0=resid, cin=self.image_channels, H=self.H, W=self.W, cout=p)
        if grad is None:
            return self.sched.emit(p0=x, p1=self.lap_targets[k], q1=self.parts[self.lap_parts_off + k * _lib.LAP_LOSS_PARTS:],
                                   taps=_lib.LAP_LOSS, **common)
        return self.sched.emit(q2=grad, taps=_lib.LAP_GRAD, flags=_lib.ACCUM, f0=lap_coef(lap_w, *resid.shape, p), **common)

    def _lap_ops(self, x: torch.Tensor, *, grad: torch.Tensor | None = None, lap_w: float = 0.0) -> list:
        """:meth:`_lap_op` of every pool, in the order of ``lap_pools``."""
        return [self._lap_op(k, x, grad=grad, lap_w=lap_w) for k in range(len(self.lap_pools))]

    def extra_terms(self, tv_w: float = 0.0, lap_w: float = 0.0) -> list[_Term]:
        """The terms of a step beyond the taps', in the order of their combine rows, of their loss ops at the head of the
        forward half and of their accumulate ops behind the first-layer dgrad: total variation with ``tv_w``, then one
        Laplacian term per pool with ``lap_w``.  The weight rides in the scale, so a term's slot of the losses holds the
        weighted term.  Head, op list and the model's views are all derived from this list."""
        terms = []
        if tv_w:
            terms.append(_Term("tv", self.tv_parts_off, _lib.TV_LOSS_PARTS, tv_scale(tv_w, self.image_channels, self.H, self.W),
                               lambda x: self._tv_op(x, loss=True), lambda x, grad: self._tv_op(x, grad=grad, tv_w=tv_w)))
        for k, resid in enumerate(self.lap_resid if lap_w else ()):
            terms.append(_Term("lap", self.lap_parts_off + k * _lib.LAP_LOSS_PARTS, _lib.LAP_LOSS_PARTS, lap_scale(lap_w, *resid.shape),
                               lambda x, k=k: self._lap_op(k, x), lambda x, grad, k=k: self._lap_op(k, x, grad=grad, lap_w=lap_w)))
        return terms

    def head(self, tv_w: float = 0.0, lap_w: float = 0.0, layer_w: tuple | None = None) -> _Head:
        """The combine op's operands for a step: the taps' rows (:meth:`_base_rows`; the style layer weights ride in their
        scales, so the style score is ``sum_l w_l * loss_l``), then one ``KIND_EXTRA`` row per entry of :meth:`extra_terms`.
        The plain step gets the engine's own table, scale and losses; every other combination a losses vector of its own
        (the engine's keeps the unweighted terms ``forward()`` returns), one head per ``(tv_w, lap_w, layer_w)`` in a cache
        of 16, oldest out."""
        terms = self.extra_terms(tv_w, lap_w)
        if not terms and layer_w is None:
            return _Head(self.table, self.scale, self.losses, None, None)
        key = (tv_w, lap_w, layer_w)
        head = self._heads.get(key)
        if head is None:
            if len(self._heads) >= 16:
                self._heads.pop(next(iter(self._heads)))
            rows, scale = self._base_rows(layer_w)
            tv = [len(rows) + i for i, t in enumerate(terms) if t.kind == "tv"]
            lap = [len(rows) + i for i, t in enumerate(terms) if t.kind == "lap"]
            table, losses = self.table, torch.zeros_like(self.losses)
            if terms:
                table = torch.tensor(rows + [[t.off, t.cnt, _lib.KIND_EXTRA] for t in terms], dtype=torch.int32, device=self.device)
                losses = torch.zeros(table.shape[0], device=self.device, dtype=torch.float32)
            scale = torch.tensor(scale + [t.scale for t in terms], dtype=torch.float32, device=self.device)
            head = self._heads[key] = _Head(table, scale, losses, tv[0] if tv else None, slice(lap[0], lap[-1] + 1) if lap else None)
        return head

    def _combine_op(self, style_w: float, content_w: float, score_log: tuple | None = None, tv_w: float = 0.0,
                    layer_w: tuple | None = None, lap_w: float = 0.0):
        """``score_log`` = (ring fp32 [3, capacity], device counter int32 [1][, host-visible record count int32 [1]]):
        the combine kernel also appends the three scores to the caller's history ring (stv_loss_combine_log).
        ``tv_w``, ``lap_w``, ``layer_w``: the step's :meth:`head`."""
        ring, count, seq = (tuple(score_log) + (None,))[:3] if score_log is not None else (None, None, None)
        head = self.head(tv_w, lap_w, layer_w)
        return self.sched.emit(op=plan.OP_LOSS_COMBINE, p0=self.parts, p1=head.table, p2=head.scale, p3=seq,
                               q0=head.losses, q1=self.scores, q2=ring, q3=count, n=ring.shape[1] if ring is not None else 0,
                               cin=head.table.shape[0], f0=style_w, f1=content_w)

    def _program(self, key: tuple, builder) -> plan.Program:
        prog = self._programs.get(key)
        if prog is None:
            if len(self._programs) >= 16:     # programs are keyed by buffer addresses: bound the cache (oldest out)
                self._programs.pop(next(iter(self._programs)))
            prog = self._programs[key] = plan.Program(builder())
        return prog

    # -- targets ---------------------------------------------------------------
    def stage_input(self, x: torch.Tensor) -> torch.Tensor:
        """A contiguous fp32 view of ``x``: ``x`` itself when it already is one, else a copy into one
        persistent staging buffer (a fresh temporary per call would key a new program + hipGraph by
        its address every time)."""
        xd = x.detach()
        if xd.is_contiguous() and xd.dtype == torch.float32:
            return xd
        if self._stage is None or self._stage.shape != xd.shape:
            self._stage = torch.empty(xd.shape, device=self.device, dtype=torch.float32)
        self._stage.copy_(xd)
        return self._stage

    def capture_content(self, content_img: torch.Tensor) -> list[torch.Tensor]:
        self.generation += 1
        x = content_img.detach().contiguous().float()
        plan.Program(self.sched.forward_ops(x)).run()
        targets = [tap.buf.act.clone() for tap in self.sched.content_taps]
        for tap, t in zip(self.sched.content_taps, targets, strict=True):
            tap.target = t
        return targets

    def capture_lap(self, content_img: torch.Tensor) -> list[torch.Tensor]:
        """The pooled content image per pool size (one POOL launch each): the Laplacian loss's targets."""
        x = content_img.detach().contiguous().float()
        targets = [torch.empty_like(r) for r in self.lap_resid]
        for p, t in zip(self.lap_pools, targets, strict=True):
            ops.lap_pool(x, t, p)
        self.bind_lap_targets(targets)
        return targets

    def bind_lap_targets(self, targets: list[torch.Tensor] | None) -> None:
        """Re-point the Laplacian ops at the model's pooled targets (they may have been replaced)."""
        if targets is None or len(targets) != len(self.lap_pools):
            msg = "Laplacian targets do not match the model's lap_pools: call set_targets() first"
            raise RuntimeError(msg)
        changed = False
        for k, (t, r) in enumerate(zip(targets, self.lap_resid, strict=True)):
            t = self._as_target(t, tuple(r.shape), torch.float32)
            changed |= self.lap_targets[k] is None or self.lap_targets[k].data_ptr() != t.data_ptr()
            self.lap_targets[k] = t
        if changed:
            self._programs.clear()

    def capture_style(self, style_img: torch.Tensor) -> list[torch.Tensor]:
        self.generation += 1
        x = style_img.detach().contiguous().float()
        Hs, Ws = x.shape[-2:]
        if self.guide is not None:
            return self._capture_style_guided(x)
        sched = (self.sched if (Hs, Ws) == (self.H, self.W) else
                 plan.Schedule(self.layers, self.style_at, self.content_at, Hs, Ws, self.dtype, self.device,
                               with_grad=False, split=self.split, switches=self.sched.switches))
        grams = [torch.empty(tap.buf.C, tap.buf.C, device=self.device, dtype=torch.float32) for tap in sched.style_taps]
        op_list = sched.forward_ops(x)
        for tap, g in zip(sched.style_taps, grams, strict=True):
            op_list += sched.gram_ops(tap, gram_out=g, target=None, loss_part=None, sgrad=None, coef=0.0, coef_dev=None)
        plan.Program(op_list, extra=(sched,)).run()      # (a schedule of the style image's own size lives as long as its program)
        for tap, g in zip(self.sched.style_taps, grams, strict=True):
            tap.target = g
        return grams

    def _capture_style_guided(self, x: torch.Tensor) -> list[torch.Tensor]:
        """Guided Gram targets ``[Ra, C, C]`` per style layer: the style image at its own size with its own label maps and
        pixel counts, through the same split and the same Gram ops as the step (a schedule of its own, also at the
        content's size: the engine's taps hold the content's maps)."""
        g = self.guide
        Hs, Ws = (int(v) for v in x.shape[-2:])
        if tuple(g.style_labels.shape) != (Hs, Ws):
            msg = f"style_labels are {tuple(g.style_labels.shape)}, the style image is {(Hs, Ws)}"
            raise ValueError(msg)
        sched = plan.Schedule(self.layers, self.style_at, self.content_at, Hs, Ws, self.dtype, self.device, with_grad=False,
                              split=self.split, switches=self.sched.switches, guide=g.n)
        maps = guidance.tap_maps(g.style_labels, [(t.buf.H, t.buf.W) for t in sched.style_taps])
        sched.attach_regions(maps, guidance.check_counts(maps, g.n, "style", g.active, self.style_at))
        grams = [torch.empty(g.n, tap.buf.C, tap.buf.C, device=self.device, dtype=torch.float32) for tap in sched.style_taps]
        op_list = sched.forward_ops(x)
        for tap, table in zip(sched.style_taps, grams, strict=True):
            op_list.append(sched.mask_split_op(tap))
            for r, c in enumerate(tap.regions):
                op_list += sched.gram_ops(c, gram_out=table[r], target=None, loss_part=None, sgrad=None, coef=0.0, coef_dev=None)
        plan.Program(op_list, extra=(sched,)).run()
        for tap, table in zip(self.sched.style_taps, grams, strict=True):
            for r, c in enumerate(tap.regions):
                c.target = table[r]
        return grams

    def bind_targets(self, style_targets: list[torch.Tensor], content_targets: list[torch.Tensor]) -> None:
        """Re-point taps at the model's public target lists (they may have been replaced)."""
        if len(style_targets) != self.n_style or len(content_targets) != self.n_content:
            msg = "target lists do not match the model's style/content layers"
            raise RuntimeError(msg)
        changed = False
        for tap, t in zip(self.sched.style_taps, style_targets, strict=True):
            if self.guide is not None:      # [Ra, C, C]: region r's chain reads table r
                t = self._as_target(t, (self.guide.n, tap.buf.C, tap.buf.C), torch.float32)
                for r, c in enumerate(tap.regions):
                    changed |= c.target is None or c.target.data_ptr() != t[r].data_ptr()
                    c.target = t[r]
                continue
            t = self._as_target(t, (tap.buf.C, tap.buf.C), torch.float32)
            changed |= tap.target is None or tap.target.data_ptr() != t.data_ptr()
            tap.target = t
        for tap, t in zip(self.sched.content_taps, content_targets, strict=True):
            if t.dim() == 4:    # [1,C,H,W] as the reference stores it -> NHWC storage
                t = self._nhwc_of(t)
            t = self._as_target(t, tuple(tap.buf.act.shape), self.dtype)
            changed |= tap.target is None or tap.target.data_ptr() != t.data_ptr()
            tap.target = t
        if changed:
            self._programs.clear()

    def _nhwc_of(self, t: torch.Tensor) -> torch.Tensor:
        """NHWC ``[H,W,C]`` storage of a ``[1,C,H,W]`` target.  The views ``set_targets`` publishes
        are recognised (channels-last strides, storage dtype): no copy.  Anything else is converted
        once and cached per (tensor, version) - this runs on every evaluation."""
        if t.shape[0] != 1:
            msg = f"content target must have batch size 1, got shape {tuple(t.shape)}"
            raise RuntimeError(msg)
        v = t[0].permute(1, 2, 0)
        if v.is_contiguous() and v.dtype == self.dtype and v.device == self.device:
            return v
        # The entry keeps the source tensor alive and is only reused for that very tensor object: a key of
        # (address, version) alone can be recycled by the caching allocator for a NEW target tensor once the
        # old one is freed, and the stale converted copy would be returned.
        cache = self._target_cache
        key = (t.data_ptr(), t._version, tuple(t.shape), t.dtype)
        hit = cache.get(key)
        if hit is None or hit[0] is not t:
            if len(cache) > 8:
                cache.clear()
            hit = (t, v.to(self.device, self.dtype).contiguous())
            cache[key] = hit
        return hit[1]

    def _as_target(self, t: torch.Tensor, shape: tuple, dtype: torch.dtype) -> torch.Tensor:
        if tuple(t.shape) != shape:
            msg = f"target shape {tuple(t.shape)} does not match features {shape}"
            raise RuntimeError(msg)
        if t.device != self.device or t.dtype != dtype or not t.is_contiguous():
            t = t.to(self.device, dtype).contiguous()
        return t

    # -- execution -------------------------------------------------------------
    def loss_and_grad(self, x: torch.Tensor, grad: torch.Tensor, style_w: float, content_w: float, *,
                      score_log: tuple | None = None, then_step=None, tv_w: float = 0.0,
                      layer_w: tuple | None = None, lap_w: float = 0.0) -> None:
        """``then_step`` (an ``optimizers.StepRequest`` for ``x``): the L-BFGS update of ``x`` from ``grad`` is the
        schedule's last op - closure and update are one launch (one hipGraph).
        ``tv_w`` > 0 adds ``tv_w * TV(x)``, ``lap_w`` > 0 (an engine with ``lap_pools``) ``lap_w * sum_p lap_p(x)`` to the total
        and their gradients to ``grad``, in two launches per entry of :meth:`extra_terms` (``stv_tv``, ``stv_lap``): the loss
        forms at the head of the forward half (the combine op, and through ``scores[2]`` the multi-iteration L-BFGS op and
        the logging ring, need the terms before the backward half), the accumulate forms right behind the first-layer
        dgrad, which WRITES ``grad``, in front of the L-BFGS op.  Weight 0: the step as it always was, under the same key.
        ``layer_w`` (one weight per style tap, in tap order, not all 1.0): the same op list with ``style_w * layer_w[l]`` as
        tap ``l``'s seed coefficient and ``layer_w[l] / (C*C)`` as its combine scale; the tuple is part of the key.
        ``None``: the step as it always was, under the same key."""
        if layer_w is not None and len(layer_w) != self.n_style:
            msg = f"{len(layer_w)} style layer weights for {self.n_style} style taps"
            raise ValueError(msg)
        if lap_w and not self.lap_pools:
            msg = f"lap_w = {lap_w:g} on an engine without lap_pools: the Laplacian term would be dropped"
            raise ValueError(msg)
        if lap_w and any(t is None for t in self.lap_targets):
            msg = "Laplacian targets must be set before computing losses."
            raise RuntimeError(msg)
        self.generation += 1
        key = ("fused", x.data_ptr(), grad.data_ptr(), style_w, content_w,
               None if score_log is None else (tuple(t.data_ptr() for t in score_log), tuple(score_log[0].shape)),
               None if then_step is None else then_step.key()) + self._options_key(tv_w, layer_w, lap_w)

        def build():
            s = self.sched
            fused_content = tuple(t for t in s.content_taps if t.grad_fused)
            tail = []
            if then_step is not None:
                # m_max = history: the reduction's grid covers a full history from the first step on (blocks past the
                # live pairs return at once), so ONE captured graph serves every step
                kw = dict(op=_lib.OP_LBFGS_STEP, p0=grad, q0=x, q1=then_step.state, q2=then_step.work, n=x.numel(),
                          cin=then_step.history, cout=then_step.history, f0=then_step.lr, f1=then_step.tol_grad,
                          f2=then_step.tol_change)
                if then_step.iters_per_step:
                    # several iterations per optimizer step: the same program replays for each of them (position and
                    # stop flag are device state); the step's loss test reads the total the combine op wrote
                    kw.update(op=_lib.OP_LBFGS_ITER, taps=then_step.iters_per_step, p1=self.scores[2:])
                tail.append(s.emit(**kw))
            fwd = self._forward_with_losses(x, style_coef=style_w, with_seed=True, content_coef=content_w, layer_w=layer_w)
            bwd = s.backward_ops(grad, content_coef=content_w, coef_dev=None, prewritten=fused_content)
            terms = self.extra_terms(tv_w, lap_w)
            if terms:      # loss forms at the head of the forward half; accumulate forms behind the dgrad that WRITES grad
                fwd[:0] = [t.loss_op(x) for t in terms]
                k = max(i for i, o in enumerate(bwd) if o.op == plan.OP_CONV_FIRST_DGRAD) + 1
                bwd[k:k] = [t.grad_op(x, grad) for t in terms]
            return fwd + [self._combine_op(style_w, content_w, score_log, tv_w, layer_w, lap_w)] + bwd + tail
        self._program(key, build).run(self.use_graph)

    def _options_key(self, tv_w: float, layer_w: tuple | None, lap_w: float) -> tuple:
        """The optional parts of a step's program key, each present only with its option on: none, the key as it always was."""
        parts = (("tv", tv_w) if tv_w else None, ("layer_w", layer_w) if layer_w is not None else None,
                 ("lap", lap_w, self.lap_pools) if lap_w else None, ("pooling", self.pooling) if self.pooling != "max" else None,
                 self.guide.key() if self.guide is not None else None)
        return tuple(p for p in parts if p is not None)

    def region_losses(self) -> torch.Tensor:
        """The unweighted terms ``loss_{l,r}`` of the last evaluation, ``[L, Ra]``: one more launch of the combine kernel
        over the style rows of the loss partials that evaluation left, with ``1 / C^2`` as every row's scale."""
        if self.guide is None:
            msg = "region losses exist on a guided model only (guide_regions > 0)"
            raise RuntimeError(msg)
        if self._region_head is None:
            sc = [1.0 / float(tap.buf.C * tap.buf.C) for tap in self.sched.all_chains()]
            self._region_head = (torch.tensor(sc, dtype=torch.float32, device=self.device),
                                 torch.zeros(self.n_style_rows, device=self.device, dtype=torch.float32),
                                 torch.zeros(4, device=self.device, dtype=torch.float32))
        scale, losses, scores = self._region_head
        ops.loss_combine(self.parts, self.table[:self.n_style_rows].contiguous(), scale, 1.0, 1.0, losses, scores)
        return losses.view(self.n_style, self.guide.n)

    def _refuse_autograd(self) -> None:
        if self.guide is not None:
            msg = "the autograd path (forward / backward) has no guided form: a guided engine runs loss_and_grad() only"
            raise RuntimeError(msg)

    def forward_losses(self, x: torch.Tensor) -> None:
        self._refuse_autograd()
        self.generation += 1
        key = ("fwd", x.data_ptr())

        def build():
            return (self._forward_with_losses(x, style_coef=0.0, with_seed=False)
                    + [self._combine_op(1.0, 1.0)])
        self._program(key, build).run(self.use_graph)

    def backward_from(self, gout: torch.Tensor, grad: torch.Tensor) -> None:
        self._refuse_autograd()
        self.coef_buf.copy_(gout)
        key = ("bwd", grad.data_ptr())

        def build():
            s = self.sched
            seeds = []
            for tap in s.style_taps:   # recompute the seeds with the upstream coefficients
                seeds += s.gram_ops(tap, gram_out=None, target=tap.target, loss_part=None, sgrad=tap.sgrad,
                                    coef=1.0, coef_dev=self.coef_buf[tap.order:], partial=False)
            return seeds + s.backward_ops(grad, content_coef=1.0, coef_dev=self.coef_buf)
        self._program(key, build).run(self.use_graph)


class _LossesFn(torch.autograd.Function):
    """``model(x)`` for autograd users: HIP forward now, HIP backward on ``.backward()``."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, engine: _Engine) -> torch.Tensor:
        engine.forward_losses(engine.stage_input(x))
        ctx.engine = engine
        ctx.generation = engine.generation
        ctx.x_meta = (x.shape, x.dtype)
        return engine.losses.clone()

    @staticmethod
    def backward(ctx, gout: torch.Tensor):
        engine: _Engine = ctx.engine
        if engine.generation != ctx.generation:
            # the engine keeps ONE set of activations per image size: a later model(x'),
            # loss_and_grad or set_targets has overwritten what this backward would differentiate
            msg = ("StyleContentModel: backward() of a forward pass whose activations were overwritten by a later "
                   "evaluation of the same model (call backward() before evaluating the model again).")
            raise RuntimeError(msg)
        shape, dtype = ctx.x_meta
        grad = torch.empty(shape, device=engine.device, dtype=torch.float32)
        engine.backward_from(gout.contiguous().float(), grad)
        return grad.to(dtype), None


# ---------------------------------------------------------------------------- model
class StyleContentModel(nn.Module):
    """VGG19 feature extractor with Gram style losses and content MSE losses.

    Same attributes as reference core_model.py:149-328 (``vgg_blocks``,
    ``style_ids``, ``content_ids``, ``style_targets``, ``content_targets``);
    ``forward`` returns two lists of 0-d loss tensors differentiable w.r.t. the
    input image.  ``loss_and_grad`` is the fused fast path used by the runner.
    """

    def __init__(self, style_layers: list[int], content_layers: list[int], *,
                 precision: str | None = None, style_layer_weights: list[float] | None = None,
                 lap_pools: tuple | list = (), guide_regions: int = 0, region_weights: list[float] | None = None,
                 pooling: str = "max") -> None:
        """``pooling``: ``"max"`` - the stack ``initialize_vgg()`` returns, the model as it always was - or ``"avg"``: its
        ``MaxPool2d`` modules replaced by ``AvgPool2d(2, 2)`` (``stv_avgpool_fwd`` / ``stv_avgpool_bwd`` as ops of their own in
        the step; ``forward()`` runs the replaced modules through autograd as it runs the others).
        ``guide_regions`` = R > 0 (1 to ``guidance.MAX_REGIONS``): spatial guidance - ``set_targets`` then takes one label map
        per image and the style term is ``sum_l w_l * sum_r lambda_r * loss_{l,r}`` with ``region_weights`` = lambda (default all
        1; a region of weight 0 is left unstyled).  0: no guidance, the model as it always was."""
        super().__init__()
        self.pooling = check_pooling(pooling)        # (refusals before the stack is built)
        self._guide: guidance.Guide | None = None
        self.set_guidance(guide_regions, region_weights, _init=True)
        self.lap_pools = check_lap_pools(lap_pools)     # pool sizes of the Laplacian loss; empty: the term is not available
        self.lap_targets: list[torch.Tensor] | None = None
        self._style_layers_given = [int(v) for v in style_layers]
        self.style_layer_weights = style_layer_weights      # (refusals before the stack is built)
        vgg = replace_pooling(initialize_vgg(), self.pooling)
        self.vgg_blocks, self.content_ids, self.style_ids = create_feature_blocks(
            vgg, style_layers, content_layers)
        self.style_targets: list[torch.Tensor] | None = None
        self.content_targets: list[torch.Tensor] | None = None
        self._style_at = sorted(set(style_layers))
        self._content_at = sorted(set(content_layers))
        self._dtype = resolve_precision(precision)
        self._split = resolve_split(precision)       # bf16x3: fp32 storage (self._dtype), split-bf16 products
        self._engines: dict = {}
        # what the last loss_and_grad() left: its engine, the gradient buffer and the views of its extra terms
        self._last_engine: _Engine | None = None
        self._grad_buf: torch.Tensor | None = None
        self._tv_term: torch.Tensor | None = None
        self._lap_terms: torch.Tensor | None = None

    # -- style layer weights -----------------------------------------------------
    @property
    def style_layer_weights(self) -> tuple[float, ...] | None:
        """One weight per entry of ``style_layers``, paired by position with the list as it was given (``None``: every
        layer counts 1).  The style score of :meth:`loss_and_grad` is ``sum_l w_l * loss_l``; :meth:`forward` keeps
        returning the unweighted per-layer losses.  Settable at any time; ``None`` and all-ones are the unweighted step."""
        return self._layer_weights

    @style_layer_weights.setter
    def style_layer_weights(self, weights: list[float] | None) -> None:
        self._layer_weights = style_mix.check_layer_weights(weights, self._style_layers_given)
        self._tap_weights = style_mix.tap_weights(self._layer_weights, self._style_layers_given)

    def style_tap_weights(self) -> tuple[float, ...] | None:
        """The layer weights in the order of ``forward()``'s style losses (the layers sorted), ``None`` when every one is 1."""
        return self._tap_weights

    # -- spatial guidance ----------------------------------------------------------
    def set_guidance(self, guide_regions: int, region_weights: list[float] | None = None, *, _init: bool = False) -> None:
        """Switch spatial guidance on (``guide_regions`` = R > 0) or off (0).  Targets and engines of the other mode are
        dropped: ``set_targets`` has to be called again."""
        if guide_regions == 0 and not isinstance(guide_regions, bool):
            if region_weights is not None:
                msg = f"region_weights {list(region_weights)} without guide_regions: the weights would be dropped"
                raise ValueError(msg)
            self.guide_regions, self.region_weights = 0, None
        else:
            regions = guidance.check_regions(guide_regions)
            self.guide_regions, self.region_weights = regions, guidance.check_region_weights(region_weights, regions)
        self._guide = None
        if not _init:
            self._engines.clear()
            self.style_targets = self.content_targets = self.lap_targets = None

    def last_region_losses(self) -> torch.Tensor:
        """The unweighted guided style terms ``loss_{l,r}`` of the last ``loss_and_grad``, ``[L, Ra]`` (layers sorted, active
        regions in ascending order)."""
        eng = self._last_engine
        if eng is None or eng.guide is None:
            msg = "last_region_losses() needs a guided model (guide_regions > 0) and an evaluation by loss_and_grad()"
            raise RuntimeError(msg)
        return eng.region_losses()

    # -- engine plumbing ---------------------------------------------------------
    def _layers(self) -> list[nn.Module]:
        return [layer for block in self.vgg_blocks for layer in block]

    def _check_image(self, x: torch.Tensor) -> None:
        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dim() != 4 or x.shape[0] != 1:
            msg = f"expected a GPU image of shape [1, C, H, W], got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}"
            raise RuntimeError(msg)
        # the condition torch's conv2d rejects in the reference; here the first-layer kernel takes
        # cin from the weights and would otherwise read out of bounds
        first = next((layer for layer in self._layers() if isinstance(layer, nn.Conv2d)), None)
        if first is not None and int(x.shape[1]) != first.in_channels:
            msg = (f"expected input with {first.in_channels} channels (the first convolution's in_channels), "
                   f"got {int(x.shape[1])} channels in shape {tuple(x.shape)}")
            raise RuntimeError(msg)

    def _engine_key(self, H: int, W: int, index: int | None) -> tuple:
        """What an engine of this model is kept under: size and device, and the pooling kind where it is not ``"max"``."""
        return (H, W, index) + ((("pooling", self.pooling),) if self.pooling != "max" else ())

    def _engine_for(self, x: torch.Tensor) -> _Engine:
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            msg = ("StyleContentModel runs on the MI355X HIP kernels only: the image must be a GPU tensor "
                   "(there is no CPU fallback on this path).")
            raise RuntimeError(msg)
        if x.dim() != 4 or x.shape[0] != 1:
            msg = f"expected an image of shape [1, C, H, W], got {tuple(x.shape)}"
            raise RuntimeError(msg)
        if not self._style_at and not self._content_at:
            msg = "no style or content layers configured"
            raise RuntimeError(msg)
        self._check_image(x)
        H, W = int(x.shape[-2]), int(x.shape[-1])
        key = self._engine_key(H, W, x.device.index)
        eng = self._engines.get(key)
        if eng is None:
            eng = _Engine(self._layers(), self._style_at, self._content_at, H, W, self._dtype, x.device, split=self._split,
                          **({"lap_pools": self.lap_pools} if self.lap_pools else {}),
                          **({"guide": self._guide} if self._guide is not None else {}))
            self._engines[key] = eng
        return eng

    def set_targets(self, style_img: torch.Tensor | list[torch.Tensor] | tuple[torch.Tensor, ...], content_img: torch.Tensor, *,
                    style_blend: list[float] | None = None, content_labels: torch.Tensor | None = None,
                    style_labels: torch.Tensor | None = None) -> None:
        """Capture Gram targets from the style image and activations from the content image.

        ``style_img`` may be a list or tuple of 1 to ``style_mix.MAX_STYLES`` images of any sizes: each is captured as a
        single one is, and per style layer the target is the blend ``(...((b_0*G_0) + b_1*G_1) + ...)`` of their Gram
        matrices, formed by one ``ops.gram_blend`` launch.  ``style_blend``: one weight per image, finite and >= 0,
        normalised to sum 1 (``style_mix.blend_weights``; ``None``: equal weights).  One image: no blend is launched."""
        styles = list(style_img) if isinstance(style_img, (list, tuple)) else [style_img]
        if not 1 <= len(styles) <= style_mix.MAX_STYLES:
            msg = f"between 1 and {style_mix.MAX_STYLES} style images can be blended, got {len(styles)}"
            raise ValueError(msg)
        blend = style_mix.blend_weights(style_blend, len(styles))       # (refusals before the first launch)
        self._guide = self._check_guidance(styles, content_img, content_labels, style_labels)
        if self._guide is not None and isinstance(content_img, torch.Tensor) and content_img.dim() == 4:
            # a guided engine is built from its label maps: new maps, a new engine
            self._engines.pop(self._engine_key(int(content_img.shape[-2]), int(content_img.shape[-1]), content_img.device.index), None)
        if self.lap_pools and isinstance(content_img, torch.Tensor) and content_img.dim() >= 2:
            check_lap_fits(self.lap_pools, int(content_img.shape[-2]), int(content_img.shape[-1]))
        eng = self._engine_for(content_img)
        for img in styles:
            if not isinstance(img, torch.Tensor) or not img.is_cuda:
                msg = "style image must be a GPU tensor (no CPU fallback on this path)"
                raise RuntimeError(msg)
            self._check_image(img)
        if len(styles) == 1:
            self.style_targets = eng.capture_style(styles[0])
        else:
            per_image = [eng.capture_style(img) for img in styles]
            self.style_targets = [ops.gram_blend(torch.stack(tables), blend) for tables in zip(*per_image, strict=True)]
            for tap, t in zip(eng.sched.style_taps, self.style_targets, strict=True):
                tap.target = t
        # public form as in the reference (core_model.py:230-232): [1, C, H, W].  They are zero-copy
        # NCHW views of the engine's NHWC buffers (channels-last strides, storage dtype).
        self.content_targets = [t.permute(2, 0, 1).unsqueeze(0) for t in eng.capture_content(content_img)]
        # the Laplacian loss's targets: the content image box-pooled, one [C, H//p, W//p] fp32 table per pool size
        self.lap_targets = eng.capture_lap(content_img) if self.lap_pools else None

    def _check_guidance(self, styles: list, content_img, content_labels, style_labels) -> guidance.Guide | None:
        """The label maps are required exactly when ``guide_regions`` > 0; every refusal comes before the first launch."""
        given = [name for name, t in (("content_labels", content_labels), ("style_labels", style_labels)) if t is not None]
        if not self.guide_regions:
            if given:
                msg = f"{' and '.join(given)} given, but the model was built without guide_regions: the labels would be dropped"
                raise ValueError(msg)
            return None
        if len(given) != 2:
            msg = (f"a model with guide_regions = {self.guide_regions} needs content_labels and style_labels, "
                   f"got {' and '.join(given) or 'neither'}")
            raise ValueError(msg)
        if len(styles) != 1:
            msg = f"spatial guidance takes one style image, got {len(styles)} (masks with several style images are not built)"
            raise ValueError(msg)
        guide = guidance.make_guide(self.guide_regions, self.region_weights, content_labels, style_labels)
        for name, labels, img in (("content_labels", guide.content_labels, content_img), ("style_labels", guide.style_labels, styles[0])):
            if isinstance(img, torch.Tensor) and img.dim() >= 2 and tuple(labels.shape) != tuple(int(v) for v in img.shape[-2:]):
                msg = f"{name} are {tuple(labels.shape)}, their image is {tuple(int(v) for v in img.shape[-2:])}"
                raise ValueError(msg)
        guidance.check_maps(guide, self._layers(), self._style_at)
        return guide

    def _require_targets(self) -> None:
        # same order and texts as reference core_model.py:255-258, 287-290
        if self.style_targets is None:
            msg = "style_targets must be set before computing losses."
            raise RuntimeError(msg)
        if self.content_targets is None:
            msg = "content_targets must be set before computing losses."
            raise RuntimeError(msg)

    def forward(self, x: torch.Tensor) -> tuple[list[torch.Tensor], list[torch.Tensor]]:
        """Per-layer style and content losses for ``x`` (``[1, C, H, W]``)."""
        if self.guide_regions:
            msg = (f"forward() is the unguided autograd path and this model has guide_regions = {self.guide_regions}: it would "
                   "return unguided losses (use loss_and_grad())")
            raise RuntimeError(msg)
        self._require_targets()
        eng = self._engine_for(x)
        eng.bind_targets(self.style_targets, self.content_targets)
        losses = _LossesFn.apply(x, eng)
        style = [losses[i] for i in range(eng.n_style)]
        content = [losses[eng.n_style + i] for i in range(eng.n_content)]
        return style, content

    def loss_and_grad(self, x: torch.Tensor, style_w: float, content_w: float, *, live_scores: bool = False,
                      score_log: tuple | None = None, tv_w: float = 0.0, lap_w: float = 0.0,
                      ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Fused step: writes d(style_w*S + content_w*C + tv_w*TV + lap_w*sum_p lap_p)/dx into ``x.grad``.

        Equivalent to reference optimization.py:292-313 (forward, weighted sum,
        ``loss.backward()``) in one command-buffer launch with no host sync.
        Returns 0-d device tensors (style_score, content_score, total).  With
        ``live_scores`` they are views of the engine's score buffer - valid until the
        next evaluation, one copy kernel less per step (the runner consumes them at once).
        ``score_log`` = (ring [3, capacity] fp32, counter [1] int32) on this device: the three scores are also
        appended to that history ring by the combine kernel itself (LossAccumulator.device_log()).
        ``tv_w`` > 0 adds the total-variation term (:func:`total_variation`) to the total (not to the two scores)
        and its gradient to ``x.grad``; :meth:`last_tv_term` returns the weighted term.
        With :attr:`style_layer_weights` the style score is ``sum_l w_l * loss_l`` and the gradient follows.
        ``lap_w`` > 0 (a model built with ``lap_pools``) adds the Laplacian terms (:func:`laplacian_loss` against the content
        image, one per pool size) to the total and their gradient to ``x.grad``; :meth:`last_lap_terms` returns them.
        """
        tv_w = float(tv_w)
        if not 0.0 <= tv_w < float("inf"):
            msg = f"tv_w must be a finite weight >= 0, got {tv_w}"
            raise ValueError(msg)
        lap_w = float(lap_w)
        if not 0.0 <= lap_w < float("inf"):
            msg = f"lap_w must be a finite weight >= 0, got {lap_w}"
            raise ValueError(msg)
        if lap_w and not self.lap_pools:
            msg = (f"lap_w = {lap_w:g}, but the model was built without lap_pools: the Laplacian term would be dropped "
                   "(StyleContentModel(..., lap_pools=[4]))")
            raise ValueError(msg)
        self._require_targets()
        eng = self._engine_for(x)
        eng.bind_targets(self.style_targets, self.content_targets)
        if lap_w:
            eng.bind_lap_targets(self.lap_targets)
        if x.dtype != torch.float32 or not x.is_contiguous():
            msg = "loss_and_grad needs a contiguous float32 image"
            raise RuntimeError(msg)
        grad = self._grad_buf
        if grad is None or grad.shape != x.shape or grad.device != x.device:
            grad = torch.zeros_like(x, requires_grad=False)
            self._grad_buf = grad
        from . import optimizers  # noqa: PLC0415
        # inside HipLBFGS.step(closure) for this very tensor: the update rides at the end of the same launch
        eng.loss_and_grad(x.detach(), grad, float(style_w), float(content_w), score_log=score_log,
                          then_step=optimizers.claim_step(x), tv_w=tv_w, layer_w=self._tap_weights,
                          **({"lap_w": lap_w} if lap_w else {}))
        self._last_engine = eng
        head = eng.head(tv_w, lap_w, self._tap_weights)       # (the one the step's combine op wrote)
        self._tv_term = None if head.tv is None else head.losses[head.tv]
        self._lap_terms = None if head.lap is None else head.losses[head.lap]
        x.grad = grad
        scores = eng.scores if live_scores else eng.scores.clone()
        return scores[0], scores[1], scores[2]

    def last_tv_term(self) -> torch.Tensor | None:
        """``tv_w * TV(x)`` of the last ``loss_and_grad`` as a 0-d device view (valid until the next evaluation with
        that weight), or ``None`` when that evaluation ran with ``tv_w == 0``."""
        return self._tv_term

    def last_lap_terms(self) -> torch.Tensor | None:
        """The weighted Laplacian terms ``lap_w * lap_p(x)`` of the last ``loss_and_grad``, one per pool size in the order of
        ``lap_pools``, as a 1-d device view (valid until the next evaluation with those weights), or ``None`` when that
        evaluation ran with ``lap_w == 0``."""
        return self._lap_terms


def lap_option_kwargs(optimization) -> dict:
    """``{"lap_pools": [...]}`` when ``optimization.lap_w`` > 0, else no keyword at all: a run without the term builds the
    model exactly as before."""
    if float(getattr(optimization, "lap_w", 0.0) or 0.0) > 0:
        return {"lap_pools": list(getattr(optimization, "lap_pools", None) or [])}
    return {}


def pooling_option_kwargs(optimization) -> dict:
    """``{"pooling": "avg"}`` when ``optimization.pooling`` is ``"avg"``, else no keyword at all: a default run builds the
    model exactly as before.  Any other value is refused, with the value named."""
    pooling = check_pooling(getattr(optimization, "pooling", "max"))
    return {"pooling": pooling} if pooling != "max" else {}


def prepare_model_and_input(
    content_img: torch.Tensor,
    style_img: torch.Tensor | list[torch.Tensor],
    device: torch.device,
    optimization,
    *,
    precision: str | None = None,
    content_labels: torch.Tensor | None = None,
    style_labels: torch.Tensor | None = None,
) -> tuple[nn.Module, torch.Tensor, torch.optim.Optimizer]:
    """Build model, start image and optimizer (reference core_model.py:331-350).

    ``precision`` (keyword-only extension): "fp32" | "bf16" activation storage, or "bf16x3"
    (fp32 storage, conv / Gram products from split bf16 operands);
    default from ``STV_PRECISION`` or fp32.  ``style_img`` may be a list of style images; ``optimization.style_blend``
    and ``optimization.style_layer_weights`` (``style_mix.py``) are read where the object has them; ``optimization.lap_pools``
    is handed to the model only when ``optimization.lap_w`` > 0.  ``content_labels`` / ``style_labels`` (uint8 ``[H, W]`` label
    maps of the two images, ``guidance.py``): the model is guided, with ``optimization.mask_regions`` and
    ``optimization.region_weights``; one without the other is refused.
    """
    from .optimizers import make_lbfgs  # noqa: PLC0415

    guide_kw, label_kw = {}, {}
    if content_labels is not None or style_labels is not None:
        if content_labels is None or style_labels is None:
            msg = "content_labels and style_labels go together: one label map without the other"
            raise ValueError(msg)
        if isinstance(style_img, (list, tuple)) and len(style_img) > 1:
            msg = f"spatial guidance takes one style image, got {len(style_img)} (masks with several style images are not built)"
            raise ValueError(msg)
        guide_kw = {"guide_regions": guidance.check_regions(getattr(optimization, "mask_regions", 2), minimum=2, what="mask_regions"),
                    "region_weights": getattr(optimization, "region_weights", None)}
        label_kw = {"content_labels": content_labels, "style_labels": style_labels}
    model = StyleContentModel(
        style_layers=optimization.style_layers,
        content_layers=optimization.content_layers,
        precision=precision,
        **style_mix.option_kwargs(optimization, "style_layer_weights"),
        **lap_option_kwargs(optimization),
        **pooling_option_kwargs(optimization),
        **guide_kw,
    ).to(device)
    model.set_targets(style_img, content_img, **style_mix.option_kwargs(optimization, "style_blend"), **label_kw)
    input_img = initialize_input(content_img, optimization.init_method)
    optimizer = make_lbfgs(
        input_img,
        lr=optimization.lr,
        max_iter=optimization.lbfgs_max_iter,
        max_eval=optimization.lbfgs_max_eval,
    )
    return model, input_img, optimizer
