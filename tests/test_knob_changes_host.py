"""CPU: knob changes between updates on kept state -- the schedules, and the oracle held to the compiled reference under them.

GLava's `ur` is measured and differs on every frame (render.c:2387; 0 after an interval without updates), and fft_scale, gravity_step, avg_window can be
re-defined while the visualiser runs.  tests/test_knob_changes.py holds the device to the oracle under such changes; this file first pins the oracle's own
mid-sequence behaviour to the reference's compiled operators (their parameters are read on every call, their state is allocated by the first), and checks
that the GL schedule contains every kind of gravity step the GL_R16 state distinguishes (glv_tables.h gravity_r16_integer_step): the conditions are about
the inputs, so a schedule that lost one of them fails here, without a device.

Both schedules are defined in tests/gpu_lib.py, which the GPU file imports them from as well."""
import ctypes as C

import numpy as np
import pytest

from gpu_lib import float_schedule, gl_schedule, updates_of
from oracle_lib import Oracle, Ref, RefStream, StreamOracle, lcg_pcm_fast

F32 = np.float32


def step_of(k):
    """g of render.c:728 in float, as the library and the oracle evaluate it"""
    with np.errstate(divide="ignore"):
        return F32(k["gravity_step"]) * (F32(1.0) / F32(k["ur"]))


def r16_integer_step(g):
    """glv_tables.h:45-48 restated: is m -> unorm16(unorm16_to_float(m) - g) the integer step m -> max(m - D, 0) for EVERY texel value m (65 536
    evaluations of the float expression)?  -> (holds, D); D is the step taken from the largest texel.  unorm16(x) = rint(clamp(x, 0, 1) * 65535) in
    double, unorm16_to_float(c) = c / 65535 correctly rounded to float."""
    g = F32(g)
    m = np.arange(65536, dtype=np.int64)
    x = m.astype(F32) / F32(65535)
    got = np.rint(np.clip(x - g, F32(0), F32(1)).astype(np.float64) * 65535.0).astype(np.int64)
    d = 65535 - int(got[65535])
    return bool((got == np.where(m > d, m - d, 0)).all()), d


@pytest.mark.parametrize("F", [1, 5])
@pytest.mark.parametrize("n", [256, 4096, 16384])
def test_oracle_follows_the_reference_through_knob_changes(oracle, ref, n, F):
    """a StreamOracle whose attributes are reassigned between frame() calls against the reference's transform_fft / _gravity / _average with the fields
    of their parameter struct reassigned in step, fed from the oracle's unpack: bit for bit over 2 F + 4 updates, -inf included"""
    sched = float_schedule(updates_of(F))
    assert len({(k["ur"], k["gravity_step"]) for k in sched}) == len(sched)
    assert sched[1]["ur"] == 0.0 and np.isposinf(step_of(sched[1])) and sched[3]["gravity_step"] == 0.0 and sched[4]["gravity_step"] < 0 and step_of(sched[5]) > 50
    so = StreamOracle(n, avg_frames=F)
    rs = RefStream(Ref.params(avg_frames=F))
    saw_inf = False
    for u, k in enumerate(sched):
        pcm = (lcg_pcm_fast(7300 + 31 * u + n, 2 * n) // (1, 8, 64)[u % 3]).astype(np.int16)
        so.channels, so.fft_scale, so.fft_cutoff = k["channels"], k["fft_scale"], k["fft_cutoff"]
        so.gravity_step, so.ur, so.avg_window = k["gravity_step"], k["ur"], k["avg_window"]
        rs.p.fft_scale, rs.p.fft_cutoff, rs.p.gravity_step, rs.p.ur, rs.p.avg_window = k["fft_scale"], k["fft_cutoff"], k["gravity_step"], k["ur"], int(k["avg_window"])
        got = so.frame(pcm)
        want = rs.frame_from_float(*Oracle.unpack_s16(pcm, k["channels"]))
        assert not np.isnan(want).any(), u
        bad = got.view(np.uint32) != want.view(np.uint32)
        assert not bad.any(), (n, F, u, k, int(bad.sum()), np.argwhere(bad)[:3].tolist())
        if u == 1: assert np.isneginf(got).all()                   # ur = 0
        if u == 2: assert np.isfinite(got).any() or F > 1          # the gravity state recovers at once; the average once the frame has left the ring
        if u == 5: assert (got[np.isfinite(got)] < -10).all()      # the step larger than the signal
        saw_inf |= bool(np.isneginf(got).any())
    assert saw_inf and np.isfinite(got).all()                       # ... and by the end nothing of it is left
    rs.close()


def test_gl_schedule_contains_every_kind_of_gravity_step(emu):
    """the numpy restatement of gravity_r16_integer_step agrees with the header's function (through the host emulator) on every step of the GL
    schedule, and the schedule's first six updates -- what the shortest case runs -- contain: two integer steps with different D, a step that fails at a
    half-integer of g * 65535, g < 0, g >= 1, ur = 0, and integer -> float -> integer on consecutive updates"""
    emu.glvemu_gravity_step.argtypes = [C.c_float, C.c_float, C.POINTER(C.c_uint)]
    sched = gl_schedule(updates_of(5))
    kinds = []
    for k in sched:
        g = step_of(k)
        holds, d = r16_integer_step(g)
        d_lib = C.c_uint(0)
        assert bool(emu.glvemu_gravity_step(k["gravity_step"], k["ur"], C.byref(d_lib))) == holds and d_lib.value == d, (k, holds, d, d_lib.value)
        frac = float(g) * 65535.0 % 1.0 if np.isfinite(g) else 0.0
        kinds.append(dict(integer=holds, d=d, g=float(g), half=(not holds) and g > 0 and abs(frac - 0.5) < 1e-3))
    head = kinds[:6]
    assert len({x["d"] for x in head if x["integer"] and 0 < x["d"] < 65535}) >= 2, head
    assert any(x["half"] for x in head), head
    assert any(x["g"] < 0 and not x["integer"] for x in head), head
    assert any(1 <= x["g"] < np.inf for x in head), head
    assert any(k["ur"] == 0.0 for k in sched[:6]) and any(np.isposinf(x["g"]) and x["integer"] and x["d"] == 65535 for x in head), head
    assert any(head[i]["integer"] and not head[i + 1]["integer"] and head[i + 2]["integer"] for i in range(4)), head
    # the longer schedules keep alternating: float-evaluated steps between integer ones beyond the head too, no two consecutive updates with the same step
    assert sum(x["half"] for x in kinds[6:]) >= 2 and sum(x["integer"] for x in kinds[6:]) >= 3, kinds[6:]
    assert all(a["g"] != b["g"] for a, b in zip(kinds, kinds[1:]))
    assert len({(k["fft_scale"], k["fft_cutoff"]) for k in sched[:6]}) == 3 and {k["avg_window"] for k in sched[:6]} == {True, False}
