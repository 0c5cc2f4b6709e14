"""What the two files of track mode with a per-step update rate share (tests/test_track_rates.py on the GPU, tests/test_track_rates_host.py without one):
the rate tables and the classification of the texel table's steps.  A plain module, like track_lib.py (default collection does not pick it up)."""
import numpy as np

F32 = np.float32


def f32_list(values):
    """the values as Python floats that are exact float32"""
    return [float(F32(v)) for v in values]


STEPS = 11                                  # more than kTrackDepth = 8: the look-ahead ring wraps, with a ragged tail

# float state: the shipped step under rates a session can meet -- the ideal one, an interval without updates (the step is +inf, every value -inf; the
# next step recovers), a negative rate (values rise), a tiny and a huge one, and what live_session_rates gives at 60 and 30 fps
FLOAT_STEP = 4.2
FLOAT_UR = f32_list([86.1328125, 0.0, 61.0, -75.0, 1e-30, 1e30, 40.5, 59.0, 60.0, 1.0, 29.032258987426758])

# texel state: g * 65535 = 100.5 / ur.  Where that is a half-integer float rounding decides texel by texel and the host evaluates in float, as it does
# for a negative step; everywhere else it takes the packed integer step D -- the kernel's rates kind evaluates the float expression at every step
TEXEL_STEP = float(F32(100.5) / F32(65535))
TEXEL_UR = f32_list([1.0, 0.5, 3.0, 0.0, 0.25, -2.0, 1e6, F32(1) / F32(3), 2.0, 1e-3, 0.125])
TEXEL_FLOAT_STEPS = [0, 2, 5, 7]
TEXEL_INTEGER_D = [201, 65535, 402, 0, 50, 65535, 804]

assert len(FLOAT_UR) == len(TEXEL_UR) == STEPS


def step_of(gravity_step, ur):
    """render.c:728 in float32: a correctly rounded division, then a separate multiply"""
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        return F32(gravity_step) * (F32(1.0) / F32(ur))


def integer_step(g):
    """glv_tables.h gravity_r16_integer_step restated: is  m -> unorm16(unorm16_to_float(m) - g)  the integer step  m -> max(m - D, 0)  for every texel
    value m?  Returns (holds, D).  unorm16_to_float: m / 65535 correctly rounded; unorm16: clamp to [0, 1] (NaN to 0), times 65535 in double, to nearest even"""
    m = np.arange(65536, dtype=np.int64)
    f = (m.astype(np.float64) / 65535.0).astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        x = f - F32(g)
    c = np.where(np.isnan(x), F32(0), np.minimum(np.maximum(x, F32(0)), F32(1))).astype(np.float64)
    tex = np.rint(c * 65535.0).astype(np.int64)
    top = int(tex[65535])
    d = 65535 - top
    return bool((tex == np.maximum(m - d, 0)).all()), d


def classify(gravity_step, urs):
    """per step: (the host evaluates in float, D of the integer step or None)"""
    out = []
    for ur in urs:
        holds, d = integer_step(step_of(gravity_step, ur))
        out.append((not holds, d if holds else None))
    return out
