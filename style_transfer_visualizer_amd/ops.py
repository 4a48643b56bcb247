"""Tensor-level wrappers over the C ABI (``include/stv.h``).

PyTorch is used only to own device memory and the current HIP stream; every
function here enqueues hand-written HIP kernels from ``libstv_hip.so`` and
raises ``RuntimeError`` if the library is missing or a call fails.

Layouts: activations are NHWC ``[H, W, C]`` tensors (batch 1) of dtype
float32 or bfloat16; the image / its gradient are ``[1, 3, H, W]`` float32.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import torch

from . import _lib
from . import resize as _resize
from ._lib import ACCUM, MASK, POOL_ONLY, RELU_IN, RELU_OUT, STV_BF16, STV_BF16X3, STV_F32, W_BLOCKED  # noqa: F401


def dtype_code(dtype: torch.dtype, *, split: bool = False) -> int:
    """The library's dtype code; ``split=True`` (fp32 storage only): STV_BF16X3, split-bf16 products."""
    if split:
        if dtype != torch.float32:
            msg = f"split-bf16 products (bf16x3) need fp32 storage, got {dtype}"
            raise RuntimeError(msg)
        return STV_BF16X3
    if dtype == torch.float32:
        return STV_F32
    if dtype == torch.bfloat16:
        return STV_BF16
    msg = f"unsupported activation dtype {dtype}; use torch.float32 or torch.bfloat16"
    raise RuntimeError(msg)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: torch.Tensor | None) -> int | None:
    if t is None:
        return None
    if not t.is_cuda:
        msg = "libstv_hip operates on device memory only (tensor is on CPU); there is no CPU fallback"
        raise RuntimeError(msg)
    if not t.is_contiguous():
        msg = "libstv_hip expects contiguous tensors"
        raise RuntimeError(msg)
    return t.data_ptr()


# ---- weight packing (once, at model build; not on the per-step path) ---------

def pack_weights_fwd(w: torch.Tensor) -> torch.Tensor:
    """[Cout,Cin,3,3] -> [9,Cout,Cin], tap = ky*3+kx (K-contiguous rows)."""
    cout, cin = w.shape[:2]
    return w.permute(2, 3, 0, 1).reshape(9, cout, cin).contiguous()


def pack_weights_bwd(w: torch.Tensor) -> torch.Tensor:
    """[Cout,Cin,3,3] -> [9,Cin,Cout] with flipped taps: dgrad as a forward conv."""
    cout, cin = w.shape[:2]
    return w.flip(2, 3).permute(2, 3, 1, 0).reshape(9, cin, cout).contiguous()


def block_weights(w: torch.Tensor) -> torch.Tensor:
    """[taps,Cout,Cin] (already in the compute dtype) -> K-blocked [taps,Cin/CK,Cout,CK], CK = 32 bytes.

    The layout ``STV_W_BLOCKED`` names (include/stv.h): the 32-byte K slices that one workgroup
    stages for its output channels become contiguous in memory.
    """
    taps, cout, cin = w.shape
    ck = 32 // w.element_size()
    if cin % ck:
        msg = f"cin={cin} is not a multiple of {ck}: this layer cannot use the K-blocked layout"
        raise RuntimeError(msg)
    return w.reshape(taps, cout, cin // ck, ck).permute(0, 2, 1, 3).contiguous()


def split_weights(w: torch.Tensor) -> torch.Tensor:
    """K-blocked fp32 weights -> the pre-split layout of STV_BF16X3 (include/stv.h), same shape, dtype and bytes.

    Each 16-byte group of four weights becomes their four bf16 hi parts (hi = bf16_rne(w)) followed by their four bf16
    lo parts (lo = bf16_rne(w - hi)): exactly the 8 bf16 k-values one lane hands to the MFMA.  Once, at model build.
    """
    if w.dtype != torch.float32 or w.shape[-1] % 4:
        msg = f"split_weights expects fp32 K-blocked weights, got {tuple(w.shape)}/{w.dtype}"
        raise RuntimeError(msg)
    hi = w.to(torch.bfloat16)
    lo = (w - hi.float()).to(torch.bfloat16)
    g = w.shape[-1] // 4
    both = torch.stack([hi.reshape(*w.shape[:-1], g, 4), lo.reshape(*w.shape[:-1], g, 4)], dim=-2)
    return both.contiguous().view(torch.int16).view(torch.float32).reshape(w.shape).contiguous()


def conv_uses_mfma(H: int, W: int, cin: int, cout: int, dtype: torch.dtype, *, split: bool = False) -> bool:
    """True when stv_conv_igemm runs this shape on the matrix cores (else: direct kernel, plain weights)."""
    return int(_lib.load().stv_conv_config(H, W, cin, cout, 9, dtype_code(dtype, split=split))) >= 0


def conv_uses_ws(H: int, W: int, cin: int, cout: int, dtype: torch.dtype, *, flags: int = 0, has_ref: bool = False,
                 has_pool: bool = False) -> bool:
    """True when this 3x3 launch runs on the weight-stationary persistent kernel (csrc/conv_ws.hip)."""
    return bool(_lib.load().stv_conv_uses_ws(H, W, cin, cout, 9, dtype_code(dtype), flags, int(has_ref), int(has_pool)))


CONV_MAX_BYTES = 2 ** 31      # what one tensor of a conv launch may hold (stv.h stv_conv_fits: 32-bit byte offsets)
CONV_PLAIN, CONV_POOL, CONV_DUAL, CONV_ROUTE = 0, 1, 2, 3      # stv.h STV_CONV_*: the forms stv_conv_fits answers for


def conv_fits(H: int, W: int, cin: int, cout: int, dtype: torch.dtype, *, form: int = CONV_PLAIN, taps: int = 9,
              cin2: int = 0, split: bool = False) -> bool:
    """True when the conv entry point of ``form`` passes its size guard for this shape (stv_conv_fits: host arithmetic)."""
    return int(_lib.load().stv_conv_fits(H, W, cin, cout, taps, cin2, form, dtype_code(dtype, split=split))) == 0


TUNE_ROUTE = 109      # stv.h STV_TUNE_ROUTE: `taps` value that tunes the shape as conv_igemm_route runs it


def conv_tune(H: int, W: int, cin: int, cout: int, taps: int, dtype: torch.dtype, *, split: bool = False) -> int:
    """Measure the tile configurations for one conv shape once (stv_conv_tune); returns the choice (-1: direct kernel).
    ``taps=TUNE_ROUTE``: the dgrad with the pooling backward in its epilogue (its own table entry)."""
    r = int(_lib.load().stv_conv_tune(H, W, cin, cout, taps, dtype_code(dtype, split=split), _stream()))
    if r < -1:
        _lib.check(-r - 100, "stv_conv_tune")
    return r


def to_nhwc(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """[1,C,H,W] -> [H,W,C] (test/fixture helper; the product never converts activations)."""
    return x[0].permute(1, 2, 0).contiguous().to(dtype)


def from_nhwc(x: torch.Tensor) -> torch.Tensor:
    return x.permute(2, 0, 1).unsqueeze(0).float().contiguous()


# ---- conv ---------------------------------------------------------------------

def conv_first_pack(wf: torch.Tensor) -> torch.Tensor:
    """Kernel-side form of a frozen first-layer weight [9,Cout,Cin] (fp32), any shape: what both directions read."""
    _, cout, cin = wf.shape
    lib = _lib.load()
    packed = torch.empty(int(lib.stv_conv_first_packed_bytes(cin, cout)) // 4, device=wf.device, dtype=torch.float32)
    _lib.check(lib.stv_conv_first_pack(_ptr(wf), _ptr(packed), cin, cout, _stream()), "stv_conv_first_pack")
    return packed


def conv_first_gram_supported(H: int, W: int, cin: int, cout: int, dtype: torch.dtype) -> bool:
    """True when the first layer can leave the Gram slabs of its own output (``gram_partials`` of conv_first_fwd)."""
    return bool(_lib.load().stv_conv_first_gram_supported(H, W, cin, cout, dtype_code(dtype)))


def conv_first_fwd(x_nchw: torch.Tensor, wf: torch.Tensor, bias: torch.Tensor | None,
                   dtype: torch.dtype, out: torch.Tensor | None = None, *,
                   packed: torch.Tensor | None = None, gram_partials: torch.Tensor | None = None) -> torch.Tensor:
    """``packed``: the weights from :func:`conv_first_pack`; None packs ``wf`` here (a torch-owned buffer, this stream).
    ``gram_partials`` ([gram_ksplit(H*W, cout), cout, cout] fp32; needs ``packed``): also filled, as :func:`gram_partial`
    of the result would."""
    _, cin, H, W = x_nchw.shape
    cout = wf.shape[1]
    if gram_partials is not None and (packed is None or tuple(gram_partials.shape) != (gram_ksplit(H * W, cout), cout, cout)):
        raise ValueError("gram_partials needs packed weights and [gram_ksplit(H*W, cout), cout, cout] slabs")
    if packed is None:
        packed = conv_first_pack(wf)
    if out is None:
        out = torch.empty(H, W, cout, device=x_nchw.device, dtype=dtype)
    _lib.check(_lib.load().stv_conv_first_fwd(_ptr(x_nchw), _ptr(packed), _ptr(bias), _ptr(out), _ptr(gram_partials),
                                              H, W, cin, cout, dtype_code(dtype), _stream()), "stv_conv_first_fwd")
    return out


def conv_first_dgrad(dy: torch.Tensor, wf: torch.Tensor, cin: int,
                     out: torch.Tensor | None = None, *, packed: torch.Tensor | None = None) -> torch.Tensor:
    H, W, cout = dy.shape
    if out is None:
        out = torch.empty(1, cin, H, W, device=dy.device, dtype=torch.float32)
    if packed is None:
        packed = conv_first_pack(wf)
    _lib.check(_lib.load().stv_conv_first_dgrad(_ptr(dy), _ptr(packed), _ptr(out), H, W, cin, cout,
                                                dtype_code(dy.dtype), _stream()), "stv_conv_first_dgrad")
    return out


# ---- conv ---------------------------------------------------------------------

def conv_igemm(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None = None,
               ref: torch.Tensor | None = None, out: torch.Tensor | None = None,
               flags: int = 0, *, split: bool = False) -> torch.Tensor:
    """x [H,W,Cin], w [taps,Cout,Cin] or K-blocked [taps,Cin/CK,Cout,CK] (same dtype) -> [H,W,Cout].
    ``split=True``: bf16x3 (fp32 storage; K-blocked weights must come from ``split_weights``)."""
    H, W, cin = x.shape
    if w.dim() == 4:
        taps, nck, cout, ck = w.shape
        cin_w = nck * ck
        flags |= W_BLOCKED
    else:
        taps, cout, cin_w = w.shape
    if cin_w != cin or w.dtype != x.dtype:
        msg = f"weight {tuple(w.shape)}/{w.dtype} does not match input {tuple(x.shape)}/{x.dtype}"
        raise RuntimeError(msg)
    if out is None:
        if flags & ACCUM:
            msg = "ACCUM needs an existing output tensor"
            raise RuntimeError(msg)
        out = torch.empty(H, W, cout, device=x.device, dtype=x.dtype)
    lib = _lib.load()
    _lib.check(lib.stv_conv_igemm(_ptr(x), _ptr(w), _ptr(bias), _ptr(ref), _ptr(out), H, W, cin, cout,
                                  taps, flags, dtype_code(x.dtype, split=split), _stream()), "stv_conv_igemm")
    return out


def conv_igemm_pool(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None, flags: int = 0,
                    out: torch.Tensor | None = None, pool_out: torch.Tensor | None = None,
                    pool_idx: torch.Tensor | None = None, *, split: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    """3x3 conv (+bias, +ReLU by flag) and MaxPool2d(2,2) of its output in one launch (stv_conv_igemm_pool).
    ``pool_idx`` (uint8 [H/2][W/2][cout], optional) receives the arg-max map ``maxpool_bwd_idx`` consumes.
    ``split=True``: bf16x3 (fp32 storage, weights from ``split_weights``)."""
    H, W, cin = x.shape
    if w.dim() == 4:
        taps, nck, cout, ck = w.shape
        flags |= W_BLOCKED
    else:
        taps, cout, _ = w.shape
    if taps != 9:
        msg = "the fused pool needs a 3x3 convolution"
        raise RuntimeError(msg)
    if out is None:
        out = torch.empty(H, W, cout, device=x.device, dtype=x.dtype)
    if pool_out is None:
        pool_out = torch.empty(H // 2, W // 2, cout, device=x.device, dtype=x.dtype)
    lib = _lib.load()
    _lib.check(lib.stv_conv_igemm_pool(_ptr(x), _ptr(w), _ptr(bias), _ptr(out), _ptr(pool_out), _ptr(pool_idx), H, W,
                                       cin, cout, flags, dtype_code(x.dtype, split=split), _stream()), "stv_conv_igemm_pool")
    return out, pool_out


def conv_igemm_dual(x: torch.Tensor, w: torch.Tensor, x2: torch.Tensor, w2: torch.Tensor,
                    ref: torch.Tensor | None = None, out: torch.Tensor | None = None, flags: int = 0, *,
                    split: bool = False) -> torch.Tensor:
    """out = [out +] mask(ref>0) * conv3x3(x, w) + x2 . w2^T in one launch (stv_conv_igemm_dual)."""
    H, W, cin = x.shape
    if w.dim() == 4:
        _, nck, cout, ck = w.shape
        flags |= W_BLOCKED
    else:
        _, cout, _ = w.shape
    cin2 = x2.shape[2]
    if out is None:
        if flags & ACCUM:
            msg = "ACCUM needs an existing output tensor"
            raise RuntimeError(msg)
        out = torch.empty(H, W, cout, device=x.device, dtype=x.dtype)
    lib = _lib.load()
    _lib.check(lib.stv_conv_igemm_dual(_ptr(x), _ptr(w), _ptr(x2), _ptr(w2), _ptr(ref), _ptr(out), H, W, cin, cin2,
                                       cout, flags, dtype_code(x.dtype, split=split), _stream()), "stv_conv_igemm_dual")
    return out


def conv_igemm_route(dy: torch.Tensor, w: torch.Tensor, pool_idx: torch.Tensor, out: torch.Tensor | None = None,
                     flags: int = 0) -> torch.Tensor:
    """dgrad of the conv behind a max-pool with the pooling backward in its epilogue (stv_conv_igemm_route):
    dy [H,W,Cin], w backward-packed, pool_idx [H,W,Cout] uint8 -> routed gradient [2H,2W,Cout]."""
    H, W, cin = dy.shape
    if w.dim() == 4:
        _, nck, cout, ck = w.shape
        flags |= W_BLOCKED
    else:
        _, cout, _ = w.shape
    if out is None:
        out = torch.empty(2 * H, 2 * W, cout, device=dy.device, dtype=dy.dtype)
    lib = _lib.load()
    _lib.check(lib.stv_conv_igemm_route(_ptr(dy), _ptr(w), _ptr(pool_idx), _ptr(out), H, W, cin, cout, flags,
                                        dtype_code(dy.dtype), _stream()), "stv_conv_igemm_route")
    return out


def gram_multi(feats: list[torch.Tensor], targets: list[torch.Tensor], *, coef: float = 1.0,
               clamp_max: float = 5e5, coef_dev: torch.Tensor | None = None,
               ) -> tuple[list[torch.Tensor], list[torch.Tensor], list[torch.Tensor]]:
    """Batched Gram chain (stv_gram_multi) over NHWC feature maps: returns (grams, loss partials, seeds) per tap.
    ``coef_dev``: a one-element fp32 device tensor every tap's seed is multiplied by."""
    lib = _lib.load()
    table = (_lib.StvGramTap * len(feats))()
    slabs, grams, parts, seeds = [], [], [], []
    for e, f, t in zip(table, feats, targets, strict=True):
        H, W, C = f.shape
        n = H * W
        slabs.append(torch.empty(gram_ksplit(n, C), C, C, device=f.device, dtype=torch.float32))
        grams.append(torch.empty(C, C, device=f.device, dtype=torch.float32))
        parts.append(torch.empty(gram_loss_parts(C), device=f.device, dtype=torch.float32))
        seeds.append(torch.empty(C, C, device=f.device, dtype=f.dtype))
        e.fill(n_pixels=n, channels=C, clamp_max=clamp_max, coef=coef, F=_ptr(f), partials=_ptr(slabs[-1]), target=_ptr(t),
               gram_out=_ptr(grams[-1]), loss_part=_ptr(parts[-1]), sgrad=_ptr(seeds[-1]), coef_dev=_ptr(coef_dev))
    _lib.check(lib.stv_gram_multi(ctypes.addressof(table), len(feats), dtype_code(feats[0].dtype), _stream()),
               "stv_gram_multi")
    torch.cuda.current_stream().synchronize()       # the slabs may go out of scope now
    return grams, parts, seeds


# ---- pool / relu --------------------------------------------------------------

def maxpool_fwd(x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    H, W, C = x.shape
    if out is None:
        out = torch.empty(H // 2, W // 2, C, device=x.device, dtype=x.dtype)
    lib = _lib.load()
    _lib.check(lib.stv_maxpool_fwd(_ptr(x), _ptr(out), H, W, C, dtype_code(x.dtype), _stream()),
               "stv_maxpool_fwd")
    return out


def maxpool_bwd_idx(idx: torch.Tensor, dy: torch.Tensor, H: int, W: int, out: torch.Tensor | None = None,
                    flags: int = 0) -> torch.Tensor:
    """Pooling backward from the arg-max byte map of ``conv_igemm_pool`` (H, W: the un-pooled size)."""
    C = dy.shape[-1]
    if out is None:
        out = torch.empty(H, W, C, device=dy.device, dtype=dy.dtype)
    lib = _lib.load()
    _lib.check(lib.stv_maxpool_bwd(_ptr(idx), _ptr(dy), _ptr(out), H, W, C, flags | _lib.POOL_IDX,
                                   dtype_code(dy.dtype), _stream()), "stv_maxpool_bwd")
    return out


def maxpool_bwd(x: torch.Tensor, dy: torch.Tensor, out: torch.Tensor | None = None,
                flags: int = 0) -> torch.Tensor:
    H, W, C = x.shape
    if out is None:
        out = torch.empty_like(x)
    lib = _lib.load()
    _lib.check(lib.stv_maxpool_bwd(_ptr(x), _ptr(dy), _ptr(out), H, W, C, flags, dtype_code(x.dtype),
                                   _stream()), "stv_maxpool_bwd")
    return out


def avgpool_fwd(x: torch.Tensor, out: torch.Tensor | None = None, relu_in: bool = False) -> torch.Tensor:
    """``AvgPool2d(2, 2)`` of an NHWC map (``stv_avgpool_fwd``): ``(((a + b) + c) + d) * 0.25`` in fp32 over each window
    in scan order, rounded once to storage; ``relu_in``: of ``max(0, x)``."""
    H, W, C = x.shape
    if out is None:
        out = torch.empty(H // 2, W // 2, C, device=x.device, dtype=x.dtype)
    elif tuple(out.shape) != (H // 2, W // 2, C) or out.dtype != x.dtype:
        msg = f"avgpool_fwd: out is {tuple(out.shape)} {out.dtype}, expected {(H // 2, W // 2, C)} {x.dtype}"
        raise RuntimeError(msg)
    lib = _lib.load()
    _lib.check(lib.stv_avgpool_fwd(_ptr(x), _ptr(out), H, W, C, RELU_IN if relu_in else 0, dtype_code(x.dtype), _stream()),
               "stv_avgpool_fwd")
    return out


def avgpool_bwd(dy: torch.Tensor, H: int, W: int, ref: torch.Tensor | None = None, out: torch.Tensor | None = None,
                accumulate: bool = False) -> torch.Tensor:
    """Backward of :func:`avgpool_fwd` (``stv_avgpool_bwd``; H, W: the un-pooled size): ``0.25 * dy`` to the four elements
    of each window; ``ref`` (the un-pooled activation): zero where ``!(ref > 0)``; ``accumulate``: added onto ``out``, whose
    rows and columns past the pooled range then keep their values (written as zeros otherwise)."""
    C = int(dy.shape[-1])
    shape = (int(H), int(W), C)
    if tuple(dy.shape) != (H // 2, W // 2, C):
        msg = f"avgpool_bwd: dy is {tuple(dy.shape)}, expected {(H // 2, W // 2, C)} for an un-pooled {H}x{W} map"
        raise RuntimeError(msg)
    if out is None:
        if accumulate:
            msg = "avgpool_bwd: accumulate=True needs the tensor to accumulate onto (out)"
            raise RuntimeError(msg)
        out = torch.empty(shape, device=dy.device, dtype=dy.dtype)
    for name, t in (("out", out), ("ref", ref)):
        if t is not None and (tuple(t.shape) != shape or t.dtype != dy.dtype):
            msg = f"avgpool_bwd: {name} is {tuple(t.shape)} {t.dtype}, expected {shape} {dy.dtype}"
            raise RuntimeError(msg)
    flags = (MASK if ref is not None else 0) | (ACCUM if accumulate else 0)
    lib = _lib.load()
    _lib.check(lib.stv_avgpool_bwd(_ptr(ref), _ptr(dy), _ptr(out), int(H), int(W), C, flags, dtype_code(dy.dtype), _stream()),
               "stv_avgpool_bwd")
    return out


def relu_fwd(x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    if out is None:
        out = torch.empty_like(x)
    lib = _lib.load()
    _lib.check(lib.stv_relu_fwd(_ptr(x), _ptr(out), x.numel(), dtype_code(x.dtype), _stream()), "stv_relu_fwd")
    return out


def relu_bwd(x: torch.Tensor, dy: torch.Tensor, out: torch.Tensor | None = None, flags: int = 0) -> torch.Tensor:
    if out is None:
        out = torch.empty_like(x)
    lib = _lib.load()
    _lib.check(lib.stv_relu_bwd(_ptr(x), _ptr(dy), _ptr(out), x.numel(), flags, dtype_code(x.dtype), _stream()),
               "stv_relu_bwd")
    return out


# ---- gram / content -------------------------------------------------------------

def gram_ksplit(n_pixels: int, C: int) -> int:
    return _lib.load().stv_gram_ksplit(n_pixels, C)


def gram_loss_parts(C: int) -> int:
    return _lib.load().stv_gram_loss_parts(C)


def gram_partial(F: torch.Tensor, partials: torch.Tensor | None = None, *, split: bool = False) -> torch.Tensor:
    """F [H,W,C] (or [N,C]) -> fp32 partial slabs [ksplit,C,C] (``split=True``: bf16x3 products of fp32 features)."""
    C = F.shape[-1]
    n = F.numel() // C
    if partials is None:
        partials = torch.empty(gram_ksplit(n, C), C, C, device=F.device, dtype=torch.float32)
    lib = _lib.load()
    _lib.check(lib.stv_gram_partial(_ptr(F), _ptr(partials), n, C, dtype_code(F.dtype, split=split), _stream()),
               "stv_gram_partial")
    return partials


def gram_finish(partials: torch.Tensor, n_pixels: int, C: int, *, target: torch.Tensor | None = None,
                gram_out: torch.Tensor | None = None, loss_part: torch.Tensor | None = None,
                sgrad: torch.Tensor | None = None, clamp_max: float = 5e5, coef: float = 1.0,
                coef_dev: torch.Tensor | None = None, dtype: torch.dtype = torch.float32,
                norm: float | None = None) -> None:
    """``norm`` defaults to ``C * n_pixels`` (the reference's ``b*c*h*w``); callers that padded the
    channel axis pass the un-padded product."""
    lib = _lib.load()
    _lib.check(lib.stv_gram_finish(_ptr(partials), _ptr(target), _ptr(gram_out), _ptr(loss_part), _ptr(sgrad),
                                   n_pixels, C, clamp_max, float(C * n_pixels) if norm is None else float(norm),
                                   coef, _ptr(coef_dev),
                                   dtype_code(dtype), _stream()), "stv_gram_finish")


def content_loss(F: torch.Tensor, target: torch.Tensor, loss_part: torch.Tensor) -> None:
    lib = _lib.load()
    _lib.check(lib.stv_content_loss(_ptr(F), _ptr(target), _ptr(loss_part), F.numel(), dtype_code(F.dtype),
                                    _stream()), "stv_content_loss")


def content_loss_grad(F: torch.Tensor, target: torch.Tensor, loss_part: torch.Tensor, dF: torch.Tensor, coef: float) -> None:
    """Loss partials (as :func:`content_loss`) and ``dF = coef * 2/n * (F - target)`` (written) in one pass."""
    lib = _lib.load()
    _lib.check(lib.stv_content_loss_grad(_ptr(F), _ptr(target), _ptr(loss_part), _ptr(dF), F.numel(), coef,
                                         dtype_code(F.dtype), _stream()), "stv_content_loss_grad")


def content_grad(F: torch.Tensor, target: torch.Tensor, dF: torch.Tensor, coef: float,
                 coef_dev: torch.Tensor | None = None, flags: int = 0) -> None:
    lib = _lib.load()
    _lib.check(lib.stv_content_grad(_ptr(F), _ptr(target), _ptr(dF), F.numel(), coef, _ptr(coef_dev), flags,
                                    dtype_code(F.dtype), _stream()), "stv_content_grad")


def tv(x: torch.Tensor | None, *, loss_part: torch.Tensor | None = None, dx: torch.Tensor | None = None,
       coef: float = 0.0, flags: int = 0, shape: tuple | None = None) -> None:
    """Total variation of the NCHW fp32 image ``x`` (``stv_tv``): ``loss_part`` receives ``TV_LOSS_PARTS`` raw partial
    sums of the squared forward differences, ``dx`` (written, or accumulated onto with ``ACCUM``) ``coef`` times the
    sum over the existing 4-neighbours of ``x - n``.  ``shape`` = (C, H, W), default ``x.shape[-3:]``."""
    lib = _lib.load()
    C, H, W = (int(v) for v in (shape if shape is not None else x.shape[-3:]))
    _lib.check(lib.stv_tv(_ptr(x), _ptr(loss_part), _ptr(dx), C, H, W, coef, flags, _stream()), "stv_tv")


def resize2x(x: torch.Tensor, mode: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """2x resize of a contiguous fp32 image ``[3, H, W]`` or ``[1, 3, H, W]`` on the device (``stv_resize2x``):
    ``RESIZE_DOWN2`` is the 2x2 box mean (H and W even), ``RESIZE_UP2`` bilinear with half-pixel centres and clamped
    edges.  Returns a tensor of the same rank (``out`` when given: same rank, the output's shape, not ``x``)."""
    lib = _lib.load()
    if x.dtype != torch.float32 or x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[0] != 1):
        msg = f"resize2x expects an fp32 image [C, H, W] or [1, C, H, W], got {tuple(x.shape)} {x.dtype}"
        raise RuntimeError(msg)
    C, H, W = (int(v) for v in x.shape[-3:])
    if mode == _lib.RESIZE_DOWN2:
        Ho, Wo = H // 2, W // 2
    else:                                   # (an unknown mode is the entry point's to refuse)
        Ho, Wo = 2 * H, 2 * W
    shape = (*x.shape[:-2], Ho, Wo)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32:
        msg = f"resize2x: out is {tuple(out.shape)} {out.dtype}, expected {shape} torch.float32"
        raise RuntimeError(msg)
    _lib.check(lib.stv_resize2x(_ptr(x), _ptr(out), C, H, W, int(mode), _stream()), "stv_resize2x")
    return out


@functools.lru_cache(maxsize=64)
def _packed_axis_table(n_in: int, n_out: int, filter: str) -> tuple[np.ndarray, int]:  # noqa: A002
    """One axis's table as a single int32 host array - ``start``, ``count``, then the bits of the fp32 weights row by row -
    and ``K``: one upload per pass."""
    start, count, weights = _resize.axis_table(n_in, n_out, filter)
    return np.concatenate([start, count, weights.reshape(-1).view(np.int32)]), int(weights.shape[1])


def _resize_pass(lib, x: torch.Tensor, y: torch.Tensor, planes: int, H: int, W: int, n_out: int, axis: int,  # noqa: PLR0913
                 filter: str) -> None:  # noqa: A002
    packed, K = _packed_axis_table(W if axis == 1 else H, n_out, filter)
    table = torch.from_numpy(packed).to(x.device)
    start, count, weights = table[:n_out], table[n_out:2 * n_out], table[2 * n_out:]
    _lib.check(lib.stv_resize_axis(_ptr(x), _ptr(y), planes, H, W, n_out, axis, _ptr(start), _ptr(count), _ptr(weights), K,
                                   _stream()), "stv_resize_axis")


def resize(x: torch.Tensor, size: tuple[int, int], filter: str = "lanczos", out: torch.Tensor | None = None,  # noqa: A002
           tmp: torch.Tensor | None = None) -> torch.Tensor:
    """Antialiased resize of a contiguous fp32 image ``[C, H, W]`` or ``[1, C, H, W]`` on the device to ``size = (Ho, Wo)``,
    up or down, with the ``bilinear``, ``bicubic`` or ``lanczos`` filter (``stv_resize_axis``; tables: ``resize.axis_table``).
    Columns are filtered first, into the intermediate ``[C, H, Wo]`` (``tmp`` when given), rows second.  A pass whose axis
    keeps its size is not launched; if both keep it, ``x`` itself is returned and ``out`` is not written.  Returns a tensor
    of the same rank (``out`` when given: same rank, the output's shape)."""
    lib = _lib.load()
    if x.dtype != torch.float32 or x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[0] != 1):
        msg = f"resize expects an fp32 image [C, H, W] or [1, C, H, W], got {tuple(x.shape)} {x.dtype}"
        raise RuntimeError(msg)
    if filter not in _resize.FILTERS:
        msg = f"resize: unknown filter {filter!r}, expected one of {sorted(_resize.FILTERS)}"
        raise RuntimeError(msg)
    C, H, W = (int(v) for v in x.shape[-3:])
    Ho, Wo = (int(v) for v in size)
    if Ho < 1 or Wo < 1:
        msg = f"resize: size is {(Ho, Wo)}, expected positive numbers"
        raise RuntimeError(msg)
    shape = (*x.shape[:-2], Ho, Wo)
    if out is not None and (tuple(out.shape) != shape or out.dtype != torch.float32):
        msg = f"resize: out is {tuple(out.shape)} {out.dtype}, expected {shape} torch.float32"
        raise RuntimeError(msg)
    if (Ho, Wo) == (H, W):
        return x
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    mid = x
    if Wo != W:
        mid = out
        if Ho != H:
            mid_shape = (*x.shape[:-2], H, Wo)
            if tmp is None:
                tmp = torch.empty(mid_shape, dtype=torch.float32, device=x.device)
            elif tuple(tmp.shape) != mid_shape or tmp.dtype != torch.float32:
                msg = f"resize: tmp is {tuple(tmp.shape)} {tmp.dtype}, expected {mid_shape} torch.float32"
                raise RuntimeError(msg)
            mid = tmp
        _resize_pass(lib, x, mid, C, H, W, Wo, 1, filter)
    if Ho != H:
        _resize_pass(lib, mid, out, C, H, Wo, Ho, 0, filter)
    return out


# ---- colour preservation (--preserve-color) ----------------------------------------

def _color_image(x: torch.Tensor, what: str) -> tuple[int, int]:
    """(H, W) of a contiguous fp32 image ``[3, H, W]`` or ``[1, 3, H, W]``; anything else is refused."""
    if x.dtype != torch.float32 or x.dim() not in (3, 4) or x.shape[-3] != 3 or (x.dim() == 4 and x.shape[0] != 1):
        msg = f"{what} expects an fp32 image [3, H, W] or [1, 3, H, W], got {tuple(x.shape)} {x.dtype}"
        raise RuntimeError(msg)
    return int(x.shape[-2]), int(x.shape[-1])


def _color_out(x: torch.Tensor, out: torch.Tensor | None, what: str) -> torch.Tensor:
    if out is None:
        return torch.empty_like(x, memory_format=torch.contiguous_format)
    if tuple(out.shape) != tuple(x.shape) or out.dtype != torch.float32:
        msg = f"{what}: out is {tuple(out.shape)} {out.dtype}, expected {tuple(x.shape)} torch.float32"
        raise RuntimeError(msg)
    return out


def color_stats(img: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """Raw colour moments of a contiguous fp32 image ``[3, H, W]`` or ``[1, 3, H, W]`` (``stv_color_stats``): a device
    tensor ``[COLOR_STATS_PARTS, 9]`` of float64, one row per workgroup - the sums of the three channels, then of the
    products x0x0, x0x1, x0x2, x1x1, x1x2, x2x2 - formed in double, in a fixed order; every entry is written (into ``out`` when given).  The caller adds the rows."""
    lib = _lib.load()
    H, W = _color_image(img, "color_stats")
    parts = out if out is not None else torch.empty(_lib.COLOR_STATS_PARTS, 9, dtype=torch.float64, device=img.device)
    if tuple(parts.shape) != (_lib.COLOR_STATS_PARTS, 9) or parts.dtype != torch.float64:
        msg = f"color_stats: out is {tuple(parts.shape)} {parts.dtype}, expected {(_lib.COLOR_STATS_PARTS, 9)} torch.float64"
        raise RuntimeError(msg)
    _lib.check(lib.stv_color_stats(_ptr(img), _ptr(parts), H, W, _stream()), "stv_color_stats")
    return parts


def color_affine(x: torch.Tensor, m12, out: torch.Tensor | None = None) -> torch.Tensor:
    """``y[c] = ((m[c][0]*x[0] + m[c][1]*x[1]) + m[c][2]*x[2]) + b[c]`` per pixel of a contiguous fp32 image ``[3, H, W]`` or
    ``[1, 3, H, W]`` (``stv_color_affine``), every operation rounded to fp32 on its own.  ``m12``: 12 host numbers, the
    row-major matrix followed by the offset.  ``out`` may be ``x`` (in place); returns ``out`` (a new tensor by default)."""
    lib = _lib.load()
    H, W = _color_image(x, "color_affine")
    values = [float(v) for v in m12]
    if len(values) != 12:       # noqa: PLR2004
        msg = f"color_affine: m12 holds {len(values)} numbers, expected 12 (3x3 matrix, then the offset)"
        raise RuntimeError(msg)
    out = _color_out(x, out, "color_affine")
    _lib.check(lib.stv_color_affine(_ptr(x), _ptr(out), (ctypes.c_float * 12)(*values), H, W, _stream()), "stv_color_affine")
    return out


def luma_transfer(result: torch.Tensor, content: torch.Tensor, *, mean: tuple | list | None, std: tuple | list | None,
                  out: torch.Tensor | None = None) -> torch.Tensor:
    """Luminance (Rec.601) of ``result`` with the chrominance of ``content`` (``stv_luma_transfer``), both contiguous fp32
    ``[3, H, W]`` or ``[1, 3, H, W]`` of one size: ``content_rgb + (Y(result_rgb) - Y(content_rgb))`` per channel, in
    [0, 1] RGB after ``prepare_image_for_output``'s rule, mapped back into the tensors' space.  ``mean``/``std`` given: the
    images are ImageNet-normalised.  ``out`` may be ``result``, not ``content``; returns ``out`` (a new tensor by default)."""
    lib = _lib.load()
    H, W = _color_image(result, "luma_transfer")
    if _color_image(content, "luma_transfer") != (H, W):
        msg = f"luma_transfer: result is {tuple(result.shape)}, content {tuple(content.shape)}"
        raise RuntimeError(msg)
    out = _color_out(result, out, "luma_transfer")
    m3 = (ctypes.c_float * 3)(*mean) if mean is not None else None
    s3 = (ctypes.c_float * 3)(*std) if std is not None else None
    _lib.check(lib.stv_luma_transfer(_ptr(result), _ptr(content), _ptr(out), H, W, m3, s3, _stream()), "stv_luma_transfer")
    return out


# ---- automatic masks (--auto-mask) -------------------------------------------------

def kmeans_assign(x: torch.Tensor, centroids: torch.Tensor, labels: torch.Tensor, parts: torch.Tensor | None = None) -> torch.Tensor:
    """One assignment pass of the colour k-means (``stv_kmeans_assign``) over a contiguous fp32 image ``[3, H, W]`` or
    ``[1, 3, H, W]``: ``labels`` (uint8 ``[H, W]``, in place: the previous labels in, the new ones out) receive the index of
    the nearest of the ``K`` <= ``KMEANS_MAX_K`` ``centroids`` (fp32 ``[K, 3]`` on the device; squared distance in fp32, the
    lowest index wins a tie).  Returns ``parts``, float64 ``[KMEANS_PARTS, KMEANS_PART_DOUBLES]`` on the device (a new tensor
    by default), one row per workgroup: per cluster the sums of the three channels and the count, then the number of labels
    that changed; every entry is written.  The caller adds the rows."""
    lib = _lib.load()
    H, W = _color_image(x, "kmeans_assign")
    if centroids.dtype != torch.float32 or centroids.dim() != 2 or centroids.shape[1] != 3 or not centroids.is_contiguous():   # noqa: PLR2004
        msg = f"kmeans_assign: centroids are {tuple(centroids.shape)} {centroids.dtype}, expected a contiguous fp32 [K, 3]"
        raise RuntimeError(msg)
    if labels.dtype != torch.uint8 or tuple(labels.shape) != (H, W) or not labels.is_contiguous():
        msg = f"kmeans_assign: labels are {tuple(labels.shape)} {labels.dtype}, expected a contiguous uint8 {(H, W)}"
        raise RuntimeError(msg)
    shape = (_lib.KMEANS_PARTS, _lib.KMEANS_PART_DOUBLES)
    if parts is None:
        parts = torch.empty(shape, dtype=torch.float64, device=x.device)
    elif tuple(parts.shape) != shape or parts.dtype != torch.float64 or not parts.is_contiguous():
        msg = f"kmeans_assign: parts is {tuple(parts.shape)} {parts.dtype}, expected a contiguous {shape} torch.float64"
        raise RuntimeError(msg)
    _lib.check(lib.stv_kmeans_assign(_ptr(x), _ptr(centroids), _ptr(labels), _ptr(parts), H, W, int(centroids.shape[0]), _stream()),
               "stv_kmeans_assign")
    return parts


# ---- automatic masks in VGG feature space (--auto-mask-space features) ----------------

def _kmf_shape(C: int, K: int, what: str) -> None:
    if C not in _lib.KMF_CHANNELS:
        msg = f"{what}: {C} channels; the feature k-means takes one of {list(_lib.KMF_CHANNELS)} (C/8 lanes per pixel, a power of two)"
        raise RuntimeError(msg)
    if not 1 <= K <= _lib.KMF_MAX_K:
        msg = f"{what}: {K} centroids; the feature k-means takes 1 to {_lib.KMF_MAX_K}"
        raise RuntimeError(msg)


def _kmf_centroids(centroids: torch.Tensor, what: str) -> tuple[int, int]:
    if centroids.dtype != torch.float32 or centroids.dim() != 2 or not centroids.is_contiguous():      # noqa: PLR2004
        msg = f"{what}: centroids are {tuple(centroids.shape)} {centroids.dtype}, expected a contiguous fp32 [K, C]"
        raise RuntimeError(msg)
    K, C = (int(v) for v in centroids.shape)
    _kmf_shape(C, K, what)
    return K, C


def _kmf_parts(parts: torch.Tensor | None, C: int, device, what: str) -> torch.Tensor:
    shape = (_lib.KMF_PARTS, _lib.kmf_row_doubles(C))
    if parts is None:
        return torch.empty(shape, dtype=torch.float64, device=device)
    if tuple(parts.shape) != shape or parts.dtype != torch.float64 or not parts.is_contiguous():
        msg = f"{what}: parts is {tuple(parts.shape)} {parts.dtype}, expected a contiguous {shape} torch.float64"
        raise RuntimeError(msg)
    return parts


def kmeans_feat_assign(F: torch.Tensor, centroids: torch.Tensor, labels: torch.Tensor, parts: torch.Tensor | None = None, *,
                       keep_labels: bool = False) -> torch.Tensor:
    """One assignment pass of the feature-space k-means (``stv_kmeans_feat_assign``) over contiguous NHWC features
    ``[..., C]`` of fp32 or bf16 storage: ``labels`` (uint8, one per pixel, in place) receive the index of the nearest of the
    ``K`` ``centroids`` (fp32 ``[K, C]`` on the device; the distance in the order stv.h fixes, the lowest index wins a tie).
    ``keep_labels``: the labels are read and not written (the sums and counts of the labels as they are).  Returns ``parts``,
    float64 ``[KMF_PARTS, kmf_row_doubles(C)]`` on the device (a new tensor by default), one row per workgroup."""
    lib = _lib.load()
    what = "kmeans_feat_assign"
    K, C = _kmf_centroids(centroids, what)
    if F.dtype not in (torch.float32, torch.bfloat16):
        msg = f"{what}: features are {F.dtype}; the two storage types are torch.float32 and torch.bfloat16"
        raise RuntimeError(msg)
    if F.dim() < 2 or int(F.shape[-1]) != C or not F.is_contiguous() or F.numel() == 0:      # noqa: PLR2004
        msg = f"{what}: features are {tuple(F.shape)}, expected a contiguous [..., {C}] (the centroids' channels last)"
        raise RuntimeError(msg)
    n = F.numel() // C
    if labels.dtype != torch.uint8 or labels.numel() != n or not labels.is_contiguous():
        msg = f"{what}: labels are {tuple(labels.shape)} {labels.dtype}, expected {n} contiguous uint8 (one per pixel)"
        raise RuntimeError(msg)
    parts = _kmf_parts(parts, C, F.device, what)
    _lib.check(lib.stv_kmeans_feat_assign(_ptr(F), dtype_code(F.dtype), _ptr(centroids), _ptr(labels), _ptr(parts), n, C, K,
                                          int(bool(keep_labels)), _stream()), "stv_kmeans_feat_assign")
    return parts


def kmeans_feat_update(parts_c: torch.Tensor, parts_s: torch.Tensor, centroids: torch.Tensor, n_c: int, n_s: int,
                       result: torch.Tensor | None = None) -> torch.Tensor:
    """The centroid update of the feature-space k-means on the device (``stv_kmeans_feat_update``): ``centroids`` (fp32
    ``[K, C]``) in place from the two images' ``parts`` and pixel numbers.  Returns ``result``, float64 ``[9]`` on the device:
    the four counts of the content image, the four of the style image, the changed total."""
    lib = _lib.load()
    what = "kmeans_feat_update"
    K, C = _kmf_centroids(centroids, what)
    parts_c, parts_s = _kmf_parts(parts_c, C, centroids.device, what), _kmf_parts(parts_s, C, centroids.device, what)
    if int(n_c) < 1 or int(n_s) < 1:
        msg = f"{what}: {n_c} and {n_s} pixels; both images hold at least one"
        raise RuntimeError(msg)
    if result is None:
        result = torch.empty(9, dtype=torch.float64, device=centroids.device)
    elif tuple(result.shape) != (9,) or result.dtype != torch.float64 or not result.is_contiguous():
        msg = f"{what}: result is {tuple(result.shape)} {result.dtype}, expected a contiguous (9,) torch.float64"
        raise RuntimeError(msg)
    _lib.check(lib.stv_kmeans_feat_update(_ptr(parts_c), _ptr(parts_s), _ptr(centroids), _ptr(result), int(n_c), int(n_s), C, K,
                                          _stream()), "stv_kmeans_feat_update")
    return result


# ---- blended Gram targets (several style images) ------------------------------------

def gram_blend(stack: torch.Tensor, weights, out: torch.Tensor | None = None) -> torch.Tensor:
    """``out = (...((w[0]*G_0) + w[1]*G_1) + ...) + w[K-1]*G_{K-1}`` element by element (``stv_gram_blend``) for a
    contiguous fp32 stack ``[K, ...]`` of ``K`` <= ``BLEND_MAX_TABLES`` tables, every product and every sum rounded to fp32
    on its own.  ``weights``: ``K`` host numbers, finite and >= 0, handed over as fp32.  ``out`` has the shape of one table
    and is not part of the stack; returns ``out`` (a new tensor by default)."""
    lib = _lib.load()
    if stack.dtype != torch.float32 or stack.dim() < 2:
        msg = f"gram_blend expects an fp32 stack [K, ...], got {tuple(stack.shape)} {stack.dtype}"
        raise RuntimeError(msg)
    K = int(stack.shape[0])
    values = [float(v) for v in weights]
    if len(values) != K:
        msg = f"gram_blend: {len(values)} weights for a stack of {K} tables"
        raise RuntimeError(msg)
    shape = tuple(stack.shape[1:])
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=stack.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32:
        msg = f"gram_blend: out is {tuple(out.shape)} {out.dtype}, expected {shape} torch.float32"
        raise RuntimeError(msg)
    _lib.check(lib.stv_gram_blend(_ptr(stack), _ptr(out), (ctypes.c_float * K)(*values), K, out.numel(), _stream()),
               "stv_gram_blend")
    return out


def mask_split(F: torch.Tensor, labels: torch.Tensor, regions: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """Region slabs of an NHWC activation (``stv_mask_split``): ``out[r, p, c]`` holds the bits of ``F[p, c]`` where
    ``labels[p] == r`` and ``+0`` elsewhere, for ``r < regions`` <= ``MASK_MAX_REGIONS``; a label >= ``regions`` (255) puts
    the pixel in no slab.  ``F``: ``[H, W, C]`` or ``[n, C]``, fp32 or bf16; ``labels``: uint8, one per pixel; ``out``:
    ``[regions, *F.shape]`` of ``F``'s dtype, sharing no byte with either; returns ``out`` (a new tensor by default)."""
    lib = _lib.load()
    C = int(F.shape[-1])
    n = F.numel() // max(C, 1)
    if labels.dtype != torch.uint8 or labels.numel() != n:
        msg = f"mask_split: labels are {tuple(labels.shape)} {labels.dtype}, expected {n} uint8 labels for features {tuple(F.shape)}"
        raise RuntimeError(msg)
    shape = (int(regions), *F.shape)
    if out is None:
        out = torch.empty(shape, dtype=F.dtype, device=F.device)
    elif tuple(out.shape) != shape or out.dtype != F.dtype:
        msg = f"mask_split: out is {tuple(out.shape)} {out.dtype}, expected {shape} {F.dtype}"
        raise RuntimeError(msg)
    _lib.check(lib.stv_mask_split(_ptr(F), _ptr(labels), _ptr(out), n, C, int(regions), dtype_code(F.dtype), _stream()),
               "stv_mask_split")
    return out


def _lap(x, target, cells, loss_part, dx, shape, pool: int, coef: float, mode: int, flags: int) -> None:
    lib = _lib.load()
    C, H, W = (int(v) for v in shape)
    _lib.check(lib.stv_lap(_ptr(x), _ptr(target), _ptr(cells), _ptr(loss_part), _ptr(dx), C, H, W, int(pool), coef, mode, flags,
                           _stream()), "stv_lap")


def lap_pool(x: torch.Tensor | None, out: torch.Tensor | None, pool: int, *, shape: tuple | None = None) -> None:
    """Cell means of the NCHW fp32 image ``x`` (``stv_lap``, mode POOL): ``out[C, H//pool, W//pool]`` receives the
    ``pool x pool`` box means (the Laplacian loss's target when ``x`` is the content image).  ``shape`` = the image's
    (C, H, W), default ``x.shape[-3:]``."""
    _lap(x, None, out, None, None, shape if shape is not None else x.shape[-3:], pool, 0.0, _lib.LAP_POOL, 0)


def lap_loss(x: torch.Tensor | None, target: torch.Tensor | None, resid: torch.Tensor | None, loss_part: torch.Tensor | None,
             pool: int, *, shape: tuple | None = None, flags: int = 0) -> None:
    """Laplacian loss of ``x`` against the pooled ``target`` (``stv_lap``, mode LOSS): ``resid[C, H//pool, W//pool]`` receives
    ``r = L (P(x) - target)``, ``loss_part`` ``LAP_LOSS_PARTS`` raw partial sums of ``r**2``."""
    _lap(x, target, resid, loss_part, None, shape if shape is not None else x.shape[-3:], pool, 0.0, _lib.LAP_LOSS, flags)


def lap_grad(resid: torch.Tensor | None, dx: torch.Tensor | None, pool: int, *, coef: float = 0.0, flags: int = 0,
             shape: tuple | None = None) -> None:
    """Gradient of the Laplacian loss from its residual (``stv_lap``, mode GRAD): ``dx`` (written, or accumulated onto with
    ``ACCUM``) ``coef * (L resid)`` of each pixel's cell.  ``shape`` = the image's (C, H, W), default ``dx.shape[-3:]``."""
    _lap(None, None, resid, None, dx, shape if shape is not None else dx.shape[-3:], pool, coef, _lib.LAP_GRAD, flags)


class HostMailbox:
    """Pinned host memory the GPU writes while the CPU reads (``stv_host_mailbox_alloc``: mapped under the same
    pointer on the device, fine-grained coherent, zeroed).  ``tensor`` / ``array`` are views; every view keeps this
    object - and with it the allocation - alive."""

    def __init__(self, nbytes: int) -> None:
        out = ctypes.c_void_p()
        _lib.check(_lib.load().stv_host_mailbox_alloc(int(nbytes), ctypes.byref(out)), "stv_host_mailbox_alloc")
        self.ptr, self.nbytes = int(out.value), int(nbytes)
        self._buf = (ctypes.c_char * self.nbytes).from_address(self.ptr)

    def tensor(self, dtype: torch.dtype, shape: tuple, offset: int = 0) -> torch.Tensor:
        count = 1
        for d in shape:
            count *= int(d)
        t = torch.frombuffer(self._buf, dtype=dtype, count=count, offset=offset).view(*shape)
        t._stv_owner = self          # (a program that baked this pointer into a graph keeps the tensor, hence the memory)
        return t

    def array(self, dtype, count: int, offset: int = 0):
        import numpy as np  # noqa: PLC0415
        a = np.frombuffer(self._buf, dtype=dtype, count=count, offset=offset)
        return a

    def __del__(self) -> None:
        try:
            if self.ptr:
                _lib.load().stv_host_mailbox_free(self.ptr)
                self.ptr = 0
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


def loss_combine(parts: torch.Tensor, table: torch.Tensor, scale: torch.Tensor, style_w: float,
                 content_w: float, losses: torch.Tensor, scores: torch.Tensor) -> None:
    lib = _lib.load()
    _lib.check(lib.stv_loss_combine(_ptr(parts), _ptr(table), _ptr(scale), table.shape[0], style_w, content_w,
                                    _ptr(losses), _ptr(scores), _stream()), "stv_loss_combine")


def loss_combine_log(parts: torch.Tensor, table: torch.Tensor, scale: torch.Tensor, style_w: float,
                     content_w: float, losses: torch.Tensor, scores: torch.Tensor, ring: torch.Tensor,
                     count: torch.Tensor, seq: torch.Tensor | None = None) -> None:
    """:func:`loss_combine` that also appends the three scores to ``ring`` [3, capacity] fp32 at slot
    ``count % capacity`` and adds one to ``count`` ([1] int32, device).  With ``seq`` ([1] int32) ring and seq are
    views of a :class:`HostMailbox`, whose host pointer is the device's; the record count is published there."""
    lib = _lib.load()
    host = seq is not None
    ring_p = ring.data_ptr() if host else _ptr(ring)
    _lib.check(lib.stv_loss_combine_log(_ptr(parts), _ptr(table), _ptr(scale), table.shape[0], style_w, content_w,
                                        _ptr(losses), _ptr(scores), ring_p, ring.shape[1], _ptr(count),
                                        seq.data_ptr() if host else None, _stream()), "stv_loss_combine_log")


# ---- frame / PNG export ---------------------------------------------------------

def image_to_u8(x: torch.Tensor, *, mean: tuple | list | None, std: tuple | list | None, rounding: bool,
                out: torch.Tensor | None = None) -> torch.Tensor:
    """[1,3,H,W] (or [3,H,W]) fp32 GPU image -> [H,W,3] uint8 GPU tensor (stv_image_to_u8).

    ``mean``/``std`` given: the image is ImageNet-normalised and is denormalised first; ``rounding``
    False = truncating ``*255`` (frames), True = ``+0.5`` rounding (final PNG)."""
    img = x.detach()
    if img.dim() == 4:
        if img.shape[0] != 1:
            msg = f"expected one image, got a batch of {img.shape[0]}"
            raise RuntimeError(msg)
        img = img[0]
    if img.dim() != 3 or img.shape[0] != 3 or img.dtype != torch.float32:
        msg = f"expected a float32 [3,H,W] image, got {tuple(img.shape)} {img.dtype}"
        raise RuntimeError(msg)
    img = img.contiguous()
    _, H, W = img.shape
    if out is None:
        out = torch.empty(H, W, 3, device=img.device, dtype=torch.uint8)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (H, W, 3) or not out.is_contiguous():      # (a slot of a frame store)
        msg = f"image_to_u8: out is {tuple(out.shape)} {out.dtype}, expected a contiguous uint8 {(H, W, 3)}"
        raise RuntimeError(msg)
    m3 = (ctypes.c_float * 3)(*mean) if mean is not None else None
    s3 = (ctypes.c_float * 3)(*std) if std is not None else None
    lib = _lib.load()
    _lib.check(lib.stv_image_to_u8(_ptr(img), _ptr(out), H, W, m3, s3, 1 if rounding else 0, _stream()),
               "stv_image_to_u8")
    return out


# ---- timelapse GIF (--gif) --------------------------------------------------------

def _gif_frame(frame: torch.Tensor, what: str) -> tuple[int, int]:
    if frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[2] != 3 or not frame.is_contiguous():   # noqa: PLR2004
        msg = f"{what} expects a contiguous uint8 frame [H, W, 3], got {tuple(frame.shape)} {frame.dtype}"
        raise RuntimeError(msg)
    return int(frame.shape[0]), int(frame.shape[1])


def frame_hist(frame: torch.Tensor, hist: torch.Tensor) -> torch.Tensor:
    """Add the pixels of a contiguous uint8 frame ``[H, W, 3]`` to the colour histogram ``hist`` (``stv_frame_hist``): bin
    ``(r>>3)<<10 | (g>>3)<<5 | (b>>3)`` counts one more per pixel.  ``hist``: ``GIF_HIST_BINS`` 32-bit counters on the
    device, ``torch.int32`` holding the bits of unsigned counts; it is accumulated into, so the caller zeroes it once.
    The frame may start at any byte (a slot of a packed store).  Returns ``hist``."""
    lib = _lib.load()
    H, W = _gif_frame(frame, "frame_hist")
    if hist.dtype != torch.int32 or tuple(hist.shape) != (_lib.GIF_HIST_BINS,) or not hist.is_contiguous():
        msg = f"frame_hist: hist is {tuple(hist.shape)} {hist.dtype}, expected a contiguous {(_lib.GIF_HIST_BINS,)} torch.int32"
        raise RuntimeError(msg)
    _lib.check(lib.stv_frame_hist(_ptr(frame), H * W, _ptr(hist), _stream()), "stv_frame_hist")
    return hist


def gif_map(frame: torch.Tensor, palette: torch.Tensor, spread: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """Palette indices of a contiguous uint8 frame ``[H, W, 3]`` (``stv_gif_map``): per pixel the 8x8 Bayer offset
    ``((2*B8[y&7][x&7] - 63) * spread) >> 7`` is added to the three channels, the sums are clamped to 0..255, and the index
    of the nearest entry of ``palette`` (uint8 ``[n, 3]`` on the device, ``n`` <= 256; squared distance in integers, the
    lowest index wins a tie) is written to ``out``, uint8 ``[H, W]`` (a new tensor by default).  ``spread`` 0..64, 0 = no
    dither.  Frame and ``out`` may start at any byte.  Returns ``out``."""
    lib = _lib.load()
    H, W = _gif_frame(frame, "gif_map")
    if palette.dtype != torch.uint8 or palette.dim() != 2 or palette.shape[1] != 3 or not palette.is_contiguous():   # noqa: PLR2004
        msg = f"gif_map: palette is {tuple(palette.shape)} {palette.dtype}, expected a contiguous uint8 [n, 3]"
        raise RuntimeError(msg)
    if out is None:
        out = torch.empty(H, W, dtype=torch.uint8, device=frame.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (H, W) or not out.is_contiguous():
        msg = f"gif_map: out is {tuple(out.shape)} {out.dtype}, expected a contiguous uint8 {(H, W)}"
        raise RuntimeError(msg)
    _lib.check(lib.stv_gif_map(_ptr(frame), _ptr(out), H, W, _ptr(palette), int(palette.shape[0]), int(spread), _stream()),
               "stv_gif_map")
    return out


# ---- Motion-JPEG timelapse (--video-format mjpeg) -----------------------------------

def jpeg_blocks(H: int, W: int) -> int:
    """8x8 blocks of a 4:2:0 frame of ``H x W`` pixels: six per 16x16 MCU, edges padded."""
    return ((int(H) + 15) // 16) * ((int(W) + 15) // 16) * 6


def _jpeg_coef(coef: torch.Tensor, what: str) -> tuple[int, int]:
    if coef.dtype != torch.int16 or coef.dim() != 3 or coef.shape[2] != 64 or not coef.is_contiguous():   # noqa: PLR2004
        msg = f"{what} expects contiguous int16 coefficients [frames, blocks, 64], got {tuple(coef.shape)} {coef.dtype}"
        raise RuntimeError(msg)
    return int(coef.shape[0]), int(coef.shape[1])


def _jpeg_u32(t: torch.Tensor, shape: tuple[int, ...], what: str) -> None:
    if t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous():
        msg = f"{what} is {tuple(t.shape)} {t.dtype}, expected a contiguous {shape} torch.int32"
        raise RuntimeError(msg)


def jpeg_dct(frame: torch.Tensor, qtabs, out: torch.Tensor | None = None) -> torch.Tensor:
    """Quantised DCT coefficients of a contiguous uint8 frame ``[H, W, 3]`` (``stv_jpeg_dct``): colour conversion, 4:2:0
    chroma, level shift, fixed-point 8x8 DCT, quantisation by ``qtabs`` (128 host integers in 1..255: the luminance table,
    then the chrominance table, row-major), int16 in zigzag order, ``[jpeg_blocks(H, W), 64]`` (a new tensor by default;
    ``out`` may be one frame of a store).  The frame may start at any byte.  Returns ``out``."""
    lib = _lib.load()
    H, W = _gif_frame(frame, "jpeg_dct")
    q = [int(v) for v in np.asarray(qtabs).reshape(-1)]
    if len(q) != 128:   # noqa: PLR2004
        msg = f"jpeg_dct: qtabs holds {len(q)} entries, expected 2 tables of 64"
        raise RuntimeError(msg)
    n = jpeg_blocks(H, W)
    if out is None:
        out = torch.empty(n, 64, dtype=torch.int16, device=frame.device)
    elif out.dtype != torch.int16 or tuple(out.shape) != (n, 64) or not out.is_contiguous():
        msg = f"jpeg_dct: out is {tuple(out.shape)} {out.dtype}, expected a contiguous int16 {(n, 64)}"
        raise RuntimeError(msg)
    _lib.check(lib.stv_jpeg_dct(_ptr(frame), (ctypes.c_int * 128)(*q), H, W, _ptr(out), _stream()), "stv_jpeg_dct")
    return out


def jpeg_block_bits(coef: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """The length in bits of every block's Huffman code (``stv_jpeg_block_bits``): ``coef`` int16 ``[frames, blocks, 64]`` in
    zigzag order, the result ``torch.int32 [frames, blocks]`` holding unsigned counts.  The DC of a block is coded against
    the previous block of its component inside its frame."""
    lib = _lib.load()
    F, B = _jpeg_coef(coef, "jpeg_block_bits")
    if out is None:
        out = torch.empty(F, B, dtype=torch.int32, device=coef.device)
    _jpeg_u32(out, (F, B), "jpeg_block_bits: out")
    _lib.check(lib.stv_jpeg_block_bits(_ptr(coef), F, B, _ptr(out), _stream()), "stv_jpeg_block_bits")
    return out


def jpeg_scan(bits: torch.Tensor, offsets: torch.Tensor | None = None,
              totals: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """Per frame the exclusive prefix sum of ``bits`` (``torch.int32 [frames, blocks]``) and its total (``stv_jpeg_scan``):
    returns ``(offsets [frames, blocks], totals [frames])``."""
    lib = _lib.load()
    if bits.dim() != 2:   # noqa: PLR2004
        msg = f"jpeg_scan expects bits [frames, blocks], got {tuple(bits.shape)}"
        raise RuntimeError(msg)
    F, B = int(bits.shape[0]), int(bits.shape[1])
    _jpeg_u32(bits, (F, B), "jpeg_scan: bits")
    if offsets is None:
        offsets = torch.empty(F, B, dtype=torch.int32, device=bits.device)
    if totals is None:
        totals = torch.empty(F, dtype=torch.int32, device=bits.device)
    _jpeg_u32(offsets, (F, B), "jpeg_scan: offsets")
    _jpeg_u32(totals, (F,), "jpeg_scan: totals")
    _lib.check(lib.stv_jpeg_scan(_ptr(bits), F, B, _ptr(offsets), _ptr(totals), _stream()), "stv_jpeg_scan")
    return offsets, totals


def jpeg_emit(coef: torch.Tensor, offsets: torch.Tensor, base: torch.Tensor, stream: torch.Tensor) -> torch.Tensor:
    """Write the Huffman code of every block into ``stream`` (``stv_jpeg_emit``): a ZEROED contiguous uint8 buffer whose size is
    a multiple of 4; frame ``f`` starts at byte ``base[f]`` (``torch.int32 [frames]``, multiples of 4) and block ``b`` at bit
    ``offsets[f, b]`` behind it, MSB first, the frame padded to a byte with 1-bits.  Returns ``stream``."""
    lib = _lib.load()
    F, B = _jpeg_coef(coef, "jpeg_emit")
    _jpeg_u32(offsets, (F, B), "jpeg_emit: offsets")
    _jpeg_u32(base, (F,), "jpeg_emit: base")
    if stream.dtype != torch.uint8 or stream.dim() != 1 or not stream.is_contiguous():
        msg = f"jpeg_emit: stream is {tuple(stream.shape)} {stream.dtype}, expected a contiguous uint8 vector"
        raise RuntimeError(msg)
    _lib.check(lib.stv_jpeg_emit(_ptr(coef), _ptr(offsets), _ptr(base), F, B, _ptr(stream), int(stream.numel()), _stream()),
               "stv_jpeg_emit")
    return stream


# ---- optimizers ---------------------------------------------------------------

def lbfgs_alloc(n: int, history: int, device: torch.device, *, compact: bool = False,
                ) -> tuple[torch.Tensor, torch.Tensor]:
    """Zeroed device state block + workspace for ``lbfgs_step`` (``compact`` selects the layout)."""
    lib = _lib.load()
    if compact:
        st_bytes, ws_bytes = lib.stv_lbfgsc_state_bytes(history), lib.stv_lbfgsc_workspace_bytes(n, history)
    else:
        st_bytes, ws_bytes = lib.stv_lbfgs_state_bytes(history), lib.stv_lbfgs_workspace_bytes(n, history)
    state = torch.zeros(st_bytes, dtype=torch.uint8, device=device)
    work = torch.zeros((ws_bytes + 3) // 4, dtype=torch.float32, device=device)
    return state, work


def lbfgs_step(x: torch.Tensor, grad: torch.Tensor, state: torch.Tensor, work: torch.Tensor, history: int,
               m_max: int, lr: float, tol_grad: float = 1e-7, tol_change: float = 1e-9, *,
               compact: bool = False) -> None:
    lib = _lib.load()
    fn = lib.stv_lbfgsc_step if compact else lib.stv_lbfgs_step
    _lib.check(fn(_ptr(x), _ptr(grad), _ptr(state), _ptr(work), x.numel(), history, m_max, lr,
                  tol_grad, tol_change, _stream()), "stv_lbfgsc_step" if compact else "stv_lbfgs_step")


def lbfgs_iter(x: torch.Tensor, grad: torch.Tensor, loss: torch.Tensor, state: torch.Tensor, work: torch.Tensor,
               history: int, m_max: int, iters_per_step: int, lr: float, tol_grad: float = 1e-7,
               tol_change: float = 1e-9) -> None:
    """One iteration of a compact L-BFGS step of ``iters_per_step`` iterations (stv_lbfgsc_iter); ``loss`` is a
    one-element float32 tensor on the device: the total of the evaluation that produced ``grad``."""
    if not loss.is_cuda or loss.dtype != torch.float32 or loss.numel() != 1:
        msg = "lbfgs_iter needs the loss as a one-element float32 GPU tensor"
        raise RuntimeError(msg)
    lib = _lib.load()
    _lib.check(lib.stv_lbfgsc_iter(_ptr(x), _ptr(grad), _ptr(loss), _ptr(state), _ptr(work), x.numel(), history, m_max,
                                   iters_per_step, lr, tol_grad, tol_change, _stream()), "stv_lbfgsc_iter")


def lbfgs_iter_reset(state: torch.Tensor) -> None:
    """The current step was abandoned midway: the next ``lbfgs_iter`` is call 1 of a new step (an enqueue)."""
    _lib.check(_lib.load().stv_lbfgsc_iter_reset(_ptr(state), _stream()), "stv_lbfgsc_iter_reset")


def lbfgs_dots(grad: torch.Tensor, state: torch.Tensor, work: torch.Tensor, history: int, m_max: int) -> torch.Tensor:
    """First half of a compact L-BFGS step (stv_lbfgsc_dots): this shard's partial inner products.
    Returns a float64 VIEW into ``work`` (5*128 + 8 entries) for the caller to all-reduce."""
    lib = _lib.load()
    n = grad.numel()
    _lib.check(lib.stv_lbfgsc_dots(_ptr(grad), _ptr(state), _ptr(work), n, history, m_max, _stream()), "stv_lbfgsc_dots")
    return lbfgs_dots_view(work, n, history)[0]


def lbfgs_dots_view(work: torch.Tensor, n: int, history: int) -> tuple[torch.Tensor, int]:
    """(float64 view of the step's inner products inside ``work``, index of the max|g| entry)."""
    count, imax = ctypes.c_int(), ctypes.c_int()
    off = int(_lib.load().stv_lbfgsc_dots_offset(n, history, ctypes.byref(count), ctypes.byref(imax)))
    if off % 8:
        msg = "internal: unaligned inner-product block"
        raise RuntimeError(msg)
    return work[off // 4: off // 4 + 2 * count.value].view(torch.float64), imax.value


def lbfgs_geometry(n: int, history: int) -> dict:
    """What a compact L-BFGS step over ``n`` elements launches (stv_lbfgsc_geometry; host only): ``nn`` (padded
    length), ``tile_a`` / ``ntiles`` / ``pgroups`` of sweep A, ``tile_b`` of sweep B."""
    nn = ctypes.c_size_t()
    tile_a, ntiles, pgroups, tile_b = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().stv_lbfgsc_geometry(n, history, ctypes.byref(nn), ctypes.byref(tile_a), ctypes.byref(ntiles),
                                               ctypes.byref(pgroups), ctypes.byref(tile_b)), "stv_lbfgsc_geometry")
    return {"nn": int(nn.value), "tile_a": tile_a.value, "ntiles": ntiles.value, "pgroups": pgroups.value,
            "tile_b": tile_b.value}


def lbfgs_views(work: torch.Tensor, n: int, history: int) -> dict:
    """fp32 views into a compact workspace: ``d`` and ``prev_g`` ``[nn]``, the rings ``S`` and ``Y``
    ``[history + 1, nn]`` (by ring slot), with ``nn`` from ``lbfgs_geometry``."""
    nn = lbfgs_geometry(n, history)["nn"]
    rows = history + 1
    ring = work[2 * nn: 2 * nn + 2 * rows * nn].view(2, rows, nn)
    return {"d": work[:nn], "prev_g": work[nn: 2 * nn], "S": ring[0], "Y": ring[1]}


def lbfgs_apply(x: torch.Tensor, grad: torch.Tensor, state: torch.Tensor, work: torch.Tensor, history: int, lr: float,
                tol_grad: float = 1e-7, tol_change: float = 1e-9) -> None:
    """Second half (stv_lbfgsc_apply): scalar recursion from the (all-reduced) inner products, then the update."""
    lib = _lib.load()
    _lib.check(lib.stv_lbfgsc_apply(_ptr(x), _ptr(grad), _ptr(state), _ptr(work), x.numel(), history, lr, tol_grad,
                                    tol_change, _stream()), "stv_lbfgsc_apply")


def adam_step(x: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, step: int,
              lr: float = 1e-3, betas: tuple[float, float] = (0.9, 0.999), eps: float = 1e-8) -> None:
    b1, b2 = betas
    bc1 = 1 - b1 ** step
    bc2_sqrt = (1 - b2 ** step) ** 0.5
    lib = _lib.load()
    _lib.check(lib.stv_adam_step(_ptr(x), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), x.numel(), lr, 1 - b1, b2,
                                 1 - b2, eps, bc1, bc2_sqrt, _stream()), "stv_adam_step")
