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


def _snap_beyond(p: np.ndarray, n: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """_snap plus, per entry, whether the fetch lands on texel n or beyond (a position of 1.0 or more): GLSL leaves such a
    texelFetch undefined; the entry is clipped to n - 1 as _snap clips"""
    x = (p.astype(F) * F(n)).astype(F)
    t, ties = _snap(p, n)
    return t, ties, np.rint(x).astype(np.int64) >= n


def graph_column_texels(n: int, screen_w: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """graph/1.frag:87-88 (gl_FragCoord at integer pixel centres, graph/1.frag:2): a column's height starts from
    smooth_audio_adj(tex, sz, idx / half_w, pixel) -- util/smooth.glsl:67-73, three fetches at max(p - pixel, 0), p and
    min(p + pixel, 1), averaged as (al + am + ar) / 3.0F -- with half_w = screen.x / 2 (integer division) and
    pixel = 1.0F / float(screen.x).  Returns ``(texels[count, 3], ties[count, 3], beyond[count, 3])`` (left, middle, right)
    for idx = 0 .. screen_w - screen_w // 2 inclusive: the table ``Batch.set_column_texels`` takes.  Every index the module
    uses is a row of it: DIRECTION >= 0 draws x < half_w from the left channel at idx = half_w - x and the other pixels
    from the right channel at idx = x - half_w; DIRECTION < 0 at idx = x and idx = screen_w - x (which reaches half_w + 1
    for an odd width); `middle` reads positions 1 and 0, rows half_w and 0.  idx >= half_w is a position of 1.0 or more --
    texel n or beyond, which GLSL leaves undefined (the shipped shader multiplies the outermost column by 0): such entries
    are flagged in ``beyond`` and clipped to n - 1."""
    half_w = screen_w // 2
    if half_w < 1:
        raise ValueError("screen_w must be at least 2")
    pixel = F(F(1.0) / F(screen_w))
    idx = np.arange(screen_w - half_w + 1, dtype=np.int64).astype(F)
    p = (idx / F(half_w)).astype(F)
    pos = np.stack([np.maximum((p - pixel).astype(F), F(0.0)), p, np.minimum((p + pixel).astype(F), F(1.0))], axis=1)
    t, ties, beyond = _snap_beyond(pos.reshape(-1), n)
    return t.reshape(-1, 3), ties.reshape(-1, 3), beyond.reshape(-1, 3)


def wave_column_texels(n: int, screen_w: int) -> tuple[np.ndarray, np.ndarray]:
    """wave/1.frag:17-23 (gl_FragCoord at integer pixel centres, wave/1.frag:2): pixel x draws from
    texture(audio_l, (gl_FragCoord.x + o) / screen.x), o in {-1, 0, 1}, on a GL_NEAREST / GL_REPEAT texture
    (render.c:1714-1717; :514-517 for the upload texture when the pre-smoothing pass is off).  Returns ``(texels, edge)``
    for x + o = -1 .. screen_w -- ``screen_w + 2`` entries, pixel x uses entries x, x + 1, x + 2 -- the table
    ``Batch.set_bar_texels`` takes for GLV_OP_WAVE | GLV_OP_BARS.

    The mapping is the one OpenGL 4.5 section 8.14 prescribes for NEAREST with REPEAT, in float32 as the shader computes
    its coordinate: u = float(x + o) / float(screen_w), u' = u * n, texel = floor(u') mod n (Euclidean: -1 wraps to the top
    end, screen_w to texel 0).  It is taken from the specification and is NOT checked against llvmpipe: the reference
    harness under oracle/ only reads `optimize_fft` binds, so the wave module cannot be run through it.

    ``edge`` flags the entries where an implementation's coordinate precision may legitimately pick the neighbouring
    texel: u' within one float32 ulp of an integer.  One case is exempt: when (x + o) * n / screen_w IS that integer in
    exact arithmetic, then (n a power of two) the odd part of screen_w divides x + o, the quotient u is a dyadic rational
    that float32 -- and any binary fixed-point coordinate -- holds exactly, and scaling by n is exact too: every
    implementation lands on the same texel boundary and floor() picks the same texel.  So screen_w == n (u' = x + o)
    has no edges; a width with a large odd part (4097 against n = 4096) has."""
    if screen_w < 1:
        raise ValueError("screen_w must be at least 1")
    xi = np.arange(-1, screen_w + 1, dtype=np.int64)
    u = (xi.astype(F) / F(screen_w)).astype(F)
    up = (u * F(n)).astype(F)
    texels = np.mod(np.floor(up).astype(np.int64), n).astype(np.uint32)
    near = np.abs(up - np.rint(up)) <= np.spacing(np.abs(up))
    exact = (xi * n) % screen_w == 0
    return texels, near & ~exact


def circle_texels(n: int, theta, rotate: float = 3.14159265359 / 2, invert: int = 0) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """circle/1.frag:34-46 for the angles ``theta`` (radians: what atan(dy, dx) hands the shader's apply_smooth):
    idx = theta + ROTATE (circle.glsl: PI / 2), folded at PI through mod(abs(idx), TWOPI), negated when INVERT > 0,
    pos = abs(idx) / (PI + 0.001F).  Returns ``(texels, is_left, ties)``: the texel of each angle, whether the shader
    fetches it from the left channel (idx > 0; the right one otherwise) and the ties of _snap -- a table for
    ``Batch.set_bar_texels``."""
    TWOPI, PI = F(6.28318530718), F(3.14159265359)
    idx = (np.asarray(theta, dtype=np.float64).astype(F).reshape(-1) + F(rotate)).astype(F)
    a = np.abs(idx)
    d = (a - (TWOPI * np.floor((a / TWOPI).astype(F))).astype(F)).astype(F)            # mod(x, y) = x - y * floor(x / y)
    idx = np.where(d > PI, (-np.sign(idx) * (TWOPI - d).astype(F)).astype(F), idx).astype(F)
    if invert > 0:
        idx = (-idx).astype(F)
    pos = (np.abs(idx) / F(PI + F(0.001))).astype(F)
    t, ties = _snap(pos, n)
    return t, idx > 0, ties
