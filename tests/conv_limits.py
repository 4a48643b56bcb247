"""The conv entry points' size guard, written out a second time (the library's: csrc/conv_args.h conv_fits).

The matrix-core conv kernels address every tensor through a raw buffer descriptor: 32-bit byte offsets, a record count
in bytes, and the offset 2^31 (kOob) for every access that must be dropped or zero-filled.  The hardware drops an access
at or beyond the record count, so a launch is sound exactly when every record count is <= 2^31: a tensor of exactly
2 GiB is addressable, one more pixel is not.  ``tensor_bytes`` lists the descriptors of each form with their byte
formulas; nothing here is derived from what the library answers.
"""
from __future__ import annotations

LIMIT = 2 ** 31
ES = {"bf16": 2, "fp32": 4, "bf16x3": 4}                  # storage bytes (bf16x3 stores fp32)
CK = {"bf16": 16, "fp32": 8, "bf16x3": 8}                  # smallest cin the tiles take: one 32-byte K-stage
KVEC = {"bf16": 8, "fp32": 4, "bf16x3": 4}                 # smallest cout: one 16-byte store
FORMS = ("forward", "1x1", "pooled", "dual", "route")      # stv_conv_igemm (taps 9 / 1), _pool, _dual, _route
FORM_CODE = {"forward": 0, "1x1": 0, "pooled": 1, "dual": 2, "route": 3}      # include/stv.h STV_CONV_*


def tensor_bytes(form: str, prec: str, H: int, W: int, cin: int, cout: int, cin2: int = 0) -> dict[str, int]:
    """Bytes of every tensor the launch reads or writes through a descriptor."""
    es = ES[prec]
    taps = 1 if form == "1x1" else 9
    t = {"x": H * W * cin * es,                 # input map
         "w": taps * cout * cin * es,           # weights (plain, K-blocked and pre-split forms hold the same bytes)
         "y": H * W * cout * es,                # output map; the ReLU-mask map `ref` and the accumulate read-back have its size
         "bias": cout * 4}
    if form == "pooled":
        t["pool"] = (H // 2) * (W // 2) * cout * es         # floor: an odd last row / column is not pooled
        t["idx"] = (H // 2) * (W // 2) * cout               # arg-max byte map
    if form == "dual":
        t["x2"] = H * W * cin2 * es
        t["w2"] = cout * cin2 * es
    if form == "route":
        t["out"] = (2 * H) * (2 * W) * cout * es            # the routed output: four times y
        t["idx"] = H * W * cout
    return t


def conv_fits(form: str, prec: str, H: int, W: int, cin: int, cout: int, cin2: int = 0) -> bool:
    if form == "route" and prec != "bf16":
        return False                                        # packed-word routing: bf16 storage only
    return all(b <= LIMIT for b in tensor_bytes(form, prec, H, W, cin, cout, cin2).values())


def deciders(form: str, prec: str, H: int, W: int, cin: int, cout: int, cin2: int = 0) -> list[str]:
    """The tensors that are over the limit."""
    return sorted(k for k, b in tensor_bytes(form, prec, H, W, cin, cout, cin2).items() if b > LIMIT)


def first_refused_square(prec: str, channels: int) -> int:
    """Smallest s for which an s x s map of ``channels`` is refused."""
    s = 1
    while s * s * channels * ES[prec] <= LIMIT:
        s += 1
    return s


def _precs(form: str) -> tuple[str, ...]:
    return ("bf16",) if form == "route" else ("bf16", "fp32", "bf16x3")


def boundary_cases() -> list[tuple]:
    """(form, precision, H, W, cin, cout, cin2, accepted, note): per form and precision the largest accepted and the
    smallest refused shape at the smallest channel counts the tiles take, as a one-pixel-wide column (one pixel = one
    32-byte K-stage of input is the finest step there is) and as the 8192-wide map the GPU tests run."""
    out = []
    for form in FORMS:
        for prec in _precs(form):
            ck, kv, es = CK[prec], KVEC[prec], ES[prec]
            c2 = ck if form == "dual" else 0
            if form == "route":
                px = LIMIT // (4 * kv * es)                  # the routed output decides: 4 x H x W x cout
                out += [(form, prec, px, 1, ck, kv, 0, True, "column"), (form, prec, px + 1, 1, ck, kv, 0, False, "column + 1 px")]
                out += [(form, prec, 4096, 4096, ck, 2 * kv, 0, True, "4096^2 -> 8192^2 x 16"),
                        (form, prec, 4097, 4096, ck, 2 * kv, 0, False, "one row more")]
                continue
            px = LIMIT // (ck * es)                          # 2^26 pixels of one K-stage each
            w = 2 if form == "pooled" else 1                 # (a pooled launch needs two columns)
            out += [(form, prec, px // w, w, ck, kv, c2, True, "column"), (form, prec, px // w + 1, w, ck, kv, c2, False, "column + 1 row")]
            out += [(form, prec, 8192, 8192, ck, ck, c2, True, "8192^2"), (form, prec, 8193, 8192, ck, ck, c2, False, "one row more"),
                    (form, prec, 8192, 8193, ck, ck, c2, False, "one column more")]
    return out


# the issue's table: 3x3, Cin = Cout = 64.  (precision, H, W, accepted)
TABLE = [
    ("fp32", 3840, 2160, True),         # 1.98 GiB: the 4K map stays
    ("fp32", 2897, 2897, False),        # 2.001 GiB
    ("fp32", 4096, 4096, False),        # 4 GiB
    ("fp32", 5792, 5792, False),        # 7.998 GiB
    ("fp32", 5793, 5793, False),        # over 2^31 elements
    ("bf16", 4096, 4096, True),         # exactly 2 GiB
    ("bf16", 7680, 4320, False),        # 3.96 GiB
    ("bf16x3", 4096, 4096, False),      # 4 GiB
    ("bf16x3", 3840, 2160, True),
]

# maps of exactly 2^31 bytes: accepted by every form that can hold them
EXACT = [("bf16", 4096, 4096, 64), ("bf16", 8192, 8192, 16), ("fp32", 8192, 8192, 8), ("bf16x3", 8192, 8192, 8)]

# (form, precision, H, W, cin, cout, cin2, the ONE tensor over the limit): every other tensor of the launch fits
LONE = [
    ("route", "bf16", 4096, 4097, 16, 16, 0, "out"),          # input and y 512 MiB each: only the 4x output is over
    ("dual", "bf16", 4097, 4096, 16, 16, 64, "x2"),           # cin2 > max(cin, cout)
    ("dual", "fp32", 2049, 2048, 8, 8, 128, "x2"),
    ("dual", "bf16x3", 2049, 2048, 8, 8, 128, "x2"),
    ("forward", "fp32", 8, 8, 8192, 8192, 0, "w"),            # 9 x 8192 x 8192 x 4 = 2.25 GiB of weights, a 2 MiB map
    ("forward", "bf16", 8, 8, 16384, 8192, 0, "w"),
    ("dual", "fp32", 1, 1, 8, 32768, 32768, "w2"),            # the seed [cout][cin2]: 4 GiB (w: 9 MiB)
    ("forward", "bf16", 8193, 8192, 16, 8, 0, "x"),           # cin > cout: the input alone
    ("1x1", "fp32", 8193, 8192, 8, 4, 0, "x"),
    ("forward", "fp32", 4097, 4096, 8, 32, 0, "y"),           # cout > cin: the output alone (x 512 MiB)
]

# The pooled map and the arg-max byte map are floor(H/2) x floor(W/2) x cout: below y for every H and W, so they can
# never be the only tensor over the limit.  What odd sizes pin instead: the decision of a pooled launch is y's, and an
# odd H or W does not round the pooled map UP past it.  (form, precision, H, W, cin, cout, accepted)
POOLED_ODD = [
    ("pooled", "bf16", 8191, 8193, 16, 16, True),             # 8191 x 8193 < 8192^2: y below 2 GiB
    ("pooled", "bf16", 8193, 8193, 16, 16, False),
    ("pooled", "fp32", 4097, 4095, 8, 32, True),
    ("pooled", "fp32", 4097, 4097, 8, 32, False),
    ("pooled", "bf16x3", 3, 2 ** 26 // 3, 8, 4, True),
    ("pooled", "bf16x3", 3, 2 ** 26 // 3 + 1, 8, 4, False),
]
