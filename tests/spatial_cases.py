"""Case tables of the row-strip tests (tests/test_spatial_host.py, tests/test_gpu_spatial_cases.py): the MINI network of
tests/test_gpu_spatial.py, the strip layouts, and what both modules derive from them.  Plain module: no test, no fixture."""
from __future__ import annotations

from dataclasses import dataclass

from torch import nn

MINI = (8, 8, "M", 16, 16, "M", 32, 32, 32, 32, "M", 64, 64, 64, 64, "M", 64, 64, 64, 64, "M")
S_AT = [0, 5, 10, 19, 28]

# content-layer sets of the coefficient tests: one tap; taps at k = 1 / 8, 2 / 8, 2 / 8 / 8 (k: down-sampling factor)
CONTENT_SETS = ([21], [3, 21], [8, 21], [8, 21, 26])

STYLE_W, CONTENT_W = 1e2, 1.0      # a content tap's gradient is >= 2 % of the total at these weights (asserted per case at 1 %)


@dataclass(frozen=True)
class Case:
    name: str
    shard: str                 # "halo" | "recompute"
    world: int
    H: int
    W: int
    strips: tuple              # core rows (c0, c1) per rank
    content_at: tuple
    precision: str = "fp32"
    extended: tuple = ()       # recompute: extended rows (e0, e1) per rank
    steps: bool = True         # optimizer steps behind the closure (fp32 only)


CASES = (
    # taps at k = 1 and k = 8: their shares of a strip with two halo rows differ ((48 + 2) / 96 against (6 + 2) / 12)
    Case("mixed", "halo", 2, 96, 40, ((0, 48), (48, 96)), (3, 21)),
    # the middle rank exchanges both ways; the last strip has ONE own row between two halo rows at k = 16; unequal L-BFGS shards
    Case("ragged16", "halo", 3, 112, 40, ((0, 48), (48, 96), (96, 112)), (8, 21)),
    # H no multiple of 16 and an odd W: floored at every pool
    Case("oddsize", "halo", 2, 100, 37, ((0, 64), (64, 100)), (3, 21)),
    # bf16 storage: the halo rows move as bytes
    Case("mixed-bf16", "halo", 2, 96, 40, ((0, 48), (48, 96)), (3, 21), precision="bf16"),
    # recomputed 160-row halos, clipped at the image border; Gram and content sums over a core sub-range of the buffers
    Case("recompute", "recompute", 2, 400, 24, ((0, 208), (208, 400)), (3, 21), extended=((0, 368), (48, 400))),
    # (400 = 16 * 25: every pooled height divides, both taps of a strip have ONE share, 368 / 400 or 352 / 400.)  At 404
    # rows the deep map has floor(404 / 8) = 50 rows: rank 0's shares are 368 / 404 at k = 1 and 46 / 50 at k = 8.  The
    # closure only: the Adam steps of this class are `recompute`'s.  (Their bound, 1e-4 absolute on the image, is no
    # property of a correct closure: Adam's normalised update turns a gradient difference d into lr * d / |g|, so the few
    # pixels whose gradient is below 1e-5 of scale move by 1e-4 under fp32 rounding alone; measured here: 1.2e-4.)
    Case("recompute-odd", "recompute", 2, 404, 24, ((0, 208), (208, 404)), (3, 21), extended=((0, 368), (48, 404)),
         steps=False),
)


def cases_of(world: int) -> list[Case]:
    return [c for c in CASES if c.world == world]


def pool_factor(layers: list, layer: int) -> int:
    """Down-sampling factor of the output of ``layers[layer]``: doubles at every 2x2 pool up to and including it."""
    return 2 ** sum(isinstance(m, (nn.MaxPool2d, nn.AvgPool2d)) for m in layers[:layer + 1])
