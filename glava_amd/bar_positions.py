"""Which texels of the pre-smoothed texture GLava's bar modules sample (glv_batch_set_bar_texels).

With ``setsmoothpass true`` (the shipped default) a module's ``smooth_audio(tex, sz, p)`` is one fetch,
``texelFetch(tex, int(round(p * sz)), 0)`` (shaders/glava/util/smooth.glsl:61-63), from the texture the
pre-smoothing pass wrote.  These helpers restate the modules' float arithmetic for ``p`` in float32 and round
half to even, as Mesa's ``round()`` does, so ``Batch.set_bar_texels`` can reproduce the bars the modules draw.

Each returns ``(texels, ties)``: the uint32 texel table and, per entry, whether ``p * sz`` landed exactly on a
half -- where GLSL leaves the rounding direction to the implementation.
"""
from __future__ import annotations

import numpy as np

F = np.float32


def _snap(p: np.ndarray, n: int) -> tuple[np.ndarray, np.ndarray]:
    x = (p.astype(F) * F(n)).astype(F)                                   # idx * tex_sz in float
    ties = (x - np.floor(x)) == F(0.5)
    t = np.rint(x).astype(np.int64)                                       # half to even
    return np.clip(t, 0, n - 1).astype(np.uint32), ties


def radial_bar_texels(n: int, nbars: int = 160) -> tuple[np.ndarray, np.ndarray]:
    """radial/1.frag:69: bar k of a channel at pos = k / float(NBARS / 2), k = 0 .. NBARS/2 - 1 (NBARS: the module's
    define, 160 shipped: 80 bars per channel)."""
    half = nbars // 2
    k = np.arange(half, dtype=np.int64)
    pos = (k.astype(F) / F(half)).astype(F)
    return _snap(pos, n)


def bars_module_bar_texels(n: int, area_width: float, bar_width: float = 5, bar_gap: float = 1,
                           channels: int = 2) -> tuple[np.ndarray, np.ndarray]:
    """bars/1.frag:64-90 with DIRECTION 0: bar j = 1, 2, ... of one channel's side of the area at
    p = j / float(nbars / 2) (channels 2; / float(nbars) for one channel) + (0.5 + center) / AREA_WIDTH, where
    section = BAR_WIDTH + BAR_GAP, center = section / 2, nbars = floor(AREA_WIDTH * 0.5 / section) * 2.
    Bars with p > 1 are not drawn (bars/1.frag:77) and are dropped."""
    W = F(area_width)
    section = F(F(bar_width) + F(bar_gap))
    center = F(section / F(2.0))
    nbars = F(np.floor(F(W * F(0.5)) / section) * F(2))
    div = F(nbars / F(2)) if channels == 2 else nbars
    count = int(div)
    j = np.arange(1, count + 1, dtype=np.int64).astype(F)
    p = (j / div).astype(F)
    p = (p + F(F(F(0.5) + center) / W)).astype(F)                          # p += sign(p) * ((0.5 + center) / AREA_WIDTH), p > 0
    p = p[p <= F(1.0)]
    return _snap(p, n)
