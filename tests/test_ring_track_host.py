"""CPU: several updates of a ring batch in one track call (glv_batch_ring_track_s16 / _f32) without a device -- the exported symbols against the header and
the ctypes mirror, the refusals that need no device, the shape of the host code (a plan, one executor, nothing but launches around the table call), and the
window rule in integers: update t of a call reads frames [(t + 1) * nf, (t + 1) * nf + n) of `ring oldest first ‖ new frames`, held to the windows a
simulated sequence of appends leaves in a rotating ring (glv_api.cpp ring_append / ring_push: write at the position, advance it, read from it)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from src_scan import ROOT, assert_launch_only, function_body, read_csrc, read_host_src, strip_comments

ENTRIES = ("glv_batch_ring_track_s16", "glv_batch_ring_track_f32")
QUERY = "glv_batch_ring_track_work_bytes"


def _decl(header, ret, name):
    m = re.search(r"\n" + ret + r" " + name + r"\s*\(([^;]*)\);", header)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_ring_track_symbols_are_exported_bound_and_declared(glvlib):
    L = C.CDLL(glvlib.LIB_PATH)
    lib = glvlib.lib()
    header = strip_comments(open(os.path.join(ROOT, "include", "glv_spectrum.h")).read())
    for name in ENTRIES + (QUERY,):
        assert hasattr(L, name), name
    assert _decl(header, "uint64_t", QUERY) == ["const glv_batch* b", "uint32_t new_frames", "uint32_t updates", "unsigned ops"]
    tail = ["uint32_t new_frames", "uint32_t updates", "void* d_out", "void* d_work", "unsigned ops", "void* hip_stream"]
    assert _decl(header, "int", ENTRIES[0]) == ["glv_batch* b", "const int16_t* d_new"] + tail
    assert _decl(header, "int", ENTRIES[1]) == ["glv_batch* b", "const float* d_new"] + tail
    u32, vp = C.c_uint32, C.c_void_p
    assert lib.glv_batch_ring_track_work_bytes.argtypes == [vp, u32, u32, C.c_uint] and lib.glv_batch_ring_track_work_bytes.restype is C.c_uint64
    for name in ENTRIES:
        assert getattr(lib, name).argtypes == [vp, vp, u32, u32, vp, vp, C.c_uint, vp], name
    for meth in ("ring_track_work_bytes", "ring_track_s16", "ring_track_f32"):
        assert callable(getattr(glvlib.Batch, meth)), meth
    assert lib.glv_abi_version() == 7                                            # added within the ABI: detected by the symbol


def test_ring_track_refuses_without_a_device(glvlib):
    lib = glvlib.lib()
    for name in ENTRIES:
        assert getattr(lib, name)(None, None, 256, 4, None, None, glvlib.OP_FFT, None) == glvlib.ERR_INVALID, name      # a NULL batch
        assert b"batch is NULL" in lib.glv_last_error()
    assert lib.glv_batch_ring_track_work_bytes(None, 256, 4, glvlib.OP_FFT) == 0
    assert b"batch is NULL" in lib.glv_last_error()
    # new_frames == 0 and updates == 0 are said by the plan before it looks at a ring or at the ops, in that order; every pointer of the call comes later
    src = strip_comments(read_host_src())
    plan = function_body(src, r"\nint plan_ring_track\(")
    assert plan.index("new_frames == 0 || new_frames > n") < plan.index("updates == 0") < plan.index("GLV_ERR_STATE") < plan.index("plan_track_at(")
    assert plan.index("GLV_ERR_STATE") < plan.index("plan_track_wave(")
    call = function_body(src, r"\nint ring_track\(glv_batch\* b,")
    assert call.index("!b") < call.index("plan_ring_track(") < call.index("!d_out || !d_work") < call.index("f32 && !d_new") < call.index("d_new) & (f32 ? 7u : 3u)")
    assert call.index("d_work) & 255u") < call.index("refuse_gravity_mix(") < call.index("refuse_stale_tilt(") < call.index("glv::launch_ring_track_stage(")


def test_the_call_is_launches_around_the_table_call():
    raw = read_host_src()
    assert_launch_only(raw, [r"\nint plan_ring_track\(", r"\nint ring_track\(glv_batch\* b,", r"\nuint64_t " + QUERY + r"\("] + [r"\nint " + name + r"\(" for name in ENTRIES])
    src = strip_comments(raw)
    for name in ENTRIES:
        body = function_body(src, r"\nint " + name + r"\(")
        assert "ring_track(b, " in body and "glv::launch_" not in body and "for (" not in body, name
    call = function_body(src, r"\nint ring_track\(glv_batch\* b,")
    for absent in ("for (", "while (", "hipMemcpy", "hipMemset", "Synchronize", "hipEvent"):
        assert absent not in call, absent
    # the stage launch, the table call on the staged recordings with the staged table, the write-back, and only then the ring's position
    order = [call.index(s) for s in ("glv::launch_ring_track_stage(", "track_at(b, r.stage, f32, rp.pitch, r.starts, updates,", "glv::launch_ring_track_keep(", "*pos = 0;",
                                     "b->last_launches += 2;")]
    assert order == sorted(order)
    assert call.count("glv::launch_") == 2 and src.count("int ring_track(") == 1 and src.count("int plan_ring_track(") == 1
    # one plan, one executor: nothing of the table call is restated
    assert src.count("int plan_track_at(") == 1 and src.count("int track_at(") == 1 and src.count("int track_wave(") == 1
    # the kernels: a unit of their own, plain C++ copies, 64-bit offsets, the launcher's cap
    unit = strip_comments(read_csrc("glv_ring_track.hip"))
    assert "asm" not in unit and "atomic" not in unit and "__shared__" not in unit
    assert unit.count("capped_grid((size_t) items, 1, kRingTrackGridCap)") == 2 and "(uint64_t) j * r.pitch" in unit and "(uint64_t) j * r.n" in unit
    assert "constexpr size_t kRingTrackGridCap = 256 * 8;" in read_csrc("glv_launch.h")
    from glava_amd import build as B
    assert "glv_ring_track" in B.SMALL and "-ffp-contract=off" in B.HIPFLAGS


# ---- the window rule, in integers ------------------------------------------------------------------------------------------------------------------------
def _rule_windows(ring_oldest_first, new, n, nf, updates):
    """the contract: frames [(t + 1) * nf, (t + 1) * nf + n) of ring ‖ new, and the ring afterwards (oldest first): the last n frames"""
    r = np.concatenate([ring_oldest_first, new])
    assert len(r) == n + updates * nf
    return [r[(t + 1) * nf:(t + 1) * nf + n] for t in range(updates)], r[len(r) - n:]


def _appended_windows(ring, pos, new, n, nf, updates):
    """the sequential calls: write nf frames at the position (wrapping), advance it, read n frames from it (wrapping)"""
    ring = ring.copy()
    wins = []
    for t in range(updates):
        for i in range(nf):
            ring[(pos + i) % n] = new[t * nf + i]
        pos = (pos + nf) % n
        wins.append(np.concatenate([ring[pos:], ring[:pos]]))
    return wins, np.concatenate([ring[pos:], ring[:pos]])


@pytest.mark.parametrize("n", [64, 256])
@pytest.mark.parametrize("nf", [1, 37, 64, "n"])
@pytest.mark.parametrize("updates", [1, 3, 10])
def test_the_window_rule_is_the_rotating_ring_s(n, nf, updates):
    nf = n if nf == "n" else nf
    rng = np.random.default_rng(n * 1000 + nf * 10 + updates)
    for pos in (0, 1, 37 % n, n - 1):
        ring = rng.integers(-30000, 30000, size=n)                             # the array as it lies: the oldest frame at `pos`
        new = rng.integers(-30000, 30000, size=updates * nf)
        oldest_first = np.concatenate([ring[pos:], ring[:pos]])
        want, ring_want = _appended_windows(ring, pos, new, n, nf, updates)
        got, ring_got = _rule_windows(oldest_first, new, n, nf, updates)
        for t in range(updates):
            assert (got[t] == want[t]).all(), (n, nf, updates, pos, t)
        assert (ring_got == ring_want).all(), (n, nf, updates, pos)


def test_the_cases_cover_both_sides_of_a_whole_ring():
    """updates * nf below n, equal to it and above it are all among the cases above"""
    totals = {(n, u * (n if nf == "n" else nf)) for n in (64, 256) for nf in (1, 37, 64, "n") for u in (1, 3, 10)}
    for n in (64, 256):
        assert any(t < n for m, t in totals if m == n) and any(t == n for m, t in totals if m == n) and any(t > 2 * n for m, t in totals if m == n)
