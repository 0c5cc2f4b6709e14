"""CPU: ring batches in track mode per stream (glv_batch_ring_track_each_s16 / _f32) without a device -- the exported symbols against the header and the
ctypes mirror, the refusals that need no device, the shape of the host code (a plan on the lockstep call's plan, one executor, nothing but launches around
the per-stream table call), the per-stream window rule in integers -- stream s's windows and final ring are those of `ring oldest first ‖ its first c * nf new
frames`, held to c simulated appends into a rotating ring -- and glava_amd.track_starts.ring_update_counts against a plain loop."""
import ctypes as C
import os

import numpy as np
import pytest

from glava_amd.track_starts import ring_update_counts
from src_scan import ROOT, assert_launch_only, function_body, read_csrc, read_host_src, strip_comments
from test_ring_track_host import _appended_windows, _decl

ENTRIES = ("glv_batch_ring_track_each_s16", "glv_batch_ring_track_each_f32")
QUERY = "glv_batch_ring_track_each_work_bytes"
EXECUTOR = r"\nint ring_track_each\(glv_batch\* b,"


def test_the_symbols_are_exported_bound_and_declared(glvlib):
    L = C.CDLL(glvlib.LIB_PATH)
    lib = glvlib.lib()
    header = strip_comments(open(os.path.join(ROOT, "include", "glv_spectrum.h")).read())
    for name in ENTRIES + (QUERY,):
        assert hasattr(L, name), name
    assert _decl(header, "uint64_t", QUERY) == ["const glv_batch* b", "uint32_t new_frames", "uint32_t updates", "unsigned ops"]
    tail = ["uint32_t new_frames", "uint32_t updates", "const float* d_ur", "const uint32_t* d_counts", "void* d_out", "void* d_work", "unsigned ops", "void* hip_stream"]
    assert _decl(header, "int", ENTRIES[0]) == ["glv_batch* b", "const int16_t* d_new"] + tail
    assert _decl(header, "int", ENTRIES[1]) == ["glv_batch* b", "const float* d_new"] + tail
    u32, vp = C.c_uint32, C.c_void_p
    assert getattr(lib, QUERY).argtypes == [vp, u32, u32, C.c_uint] and getattr(lib, QUERY).restype is C.c_uint64
    for name in ENTRIES:
        assert getattr(lib, name).argtypes == [vp, vp, u32, u32, vp, vp, vp, vp, C.c_uint, vp], name
    for meth in ("ring_track_each_work_bytes", "ring_track_each_s16", "ring_track_each_f32"):
        assert callable(getattr(glvlib.Batch, meth)), meth
    assert lib.glv_abi_version() == 7                                            # added within the ABI: detected by the symbol


def test_the_entries_refuse_without_a_device(glvlib):
    lib = glvlib.lib()
    for name in ENTRIES:
        assert getattr(lib, name)(None, None, 256, 4, None, None, None, None, glvlib.OP_FFT, None) == glvlib.ERR_INVALID, name      # a NULL batch
        assert b"batch is NULL" in lib.glv_last_error()
    assert getattr(lib, QUERY)(None, 256, 4, glvlib.OP_FFT) == 0
    assert b"batch is NULL" in lib.glv_last_error()


def test_the_refusals_come_before_the_first_launch_in_the_siblings_words():
    src = strip_comments(read_host_src())
    # the plan: the wave form first, in words that name the lockstep entries; then the lockstep call's plan -- new_frames, updates, the ring, the 2^32
    # bounds, plan_track_at's refusals and workspace -- with a row of starts per stream in the place of its one row
    plan = function_body(src, r"\nint plan_ring_track_each\(")
    assert plan.index("ops & GLV_OP_WAVE") < plan.index("plan_ring_track(b, f32, new_frames, updates, ops, rp)") < plan.index("b->streams * updates * 4u")
    assert "glv_batch_ring_track_s16 / _f32" in plan and "plan_track_at(" in function_body(src, r"\nint plan_ring_track\(")
    call = function_body(src, EXECUTOR)
    order = [call.index(s) for s in ("!b", "plan_ring_track_each(", "!d_out || !d_work", "f32 && !d_new", "d_new) & (f32 ? 7u : 3u)", "d_work) & 255u", "d_ur) & 3u", "d_counts) & 3u",
                                     "!(ops & GLV_OP_GRAVITY)", "!(ops & (GLV_OP_GRAVITY | GLV_OP_AVERAGE))", "refuse_gravity_mix(", "refuse_stale_tilt(", "glv::launch_ring_each_stage(")]
    assert order == sorted(order)
    each = function_body(src, r"\nint track_each\(glv_batch\* b,")
    for words in ('"d_ur must be 4-byte aligned"', '"d_counts must be 4-byte aligned"', '"a rates track call needs GLV_OP_GRAVITY, which reads the rate table (ops 0x%x)"',
                  '"the chain keeps no state for d_counts to protect: counts need GLV_OP_GRAVITY and / or GLV_OP_AVERAGE and no GLV_OP_WAVE (ops 0x%x)"'):
        assert words in call and words in each, words


def test_the_call_is_launches_around_the_per_stream_table_call():
    raw = read_host_src()
    assert_launch_only(raw, [r"\nint plan_ring_track_each\(", EXECUTOR, r"\nuint64_t " + QUERY + r"\("] + [r"\nint " + name + r"\(" for name in ENTRIES])
    src = strip_comments(raw)
    for name in ENTRIES:
        body = function_body(src, r"\nint " + name + r"\(")
        assert "ring_track_each(b, " in body and "glv::launch_" not in body and "for (" not in body and "while (" not in body, name
    call = function_body(src, EXECUTOR)
    for absent in ("for (", "while (", "hipMemcpy", "hipMemset", "Synchronize", "hipEvent"):
        assert absent not in call, absent
    # the stage launch, the per-stream table call on the staged recordings with the staged table, the write-back, and only then the ring's position
    order = [call.index(s) for s in ("glv::launch_ring_each_stage(", "track_each(b, e.r.stage, f32, rp.pitch, &tb, updates,", "glv::launch_ring_each_keep(", "*pos = 0;",
                                     "b->last_launches += 2;")]
    assert order == sorted(order)
    assert call.count("glv::launch_") == 2
    for restored in ("b->head = head;", "b->grav_cur = grav_cur;", "b->grav_mode = grav_mode;", "b->ran_live = ran_live;"):
        assert restored in call, restored
    # one plan and one executor of every name: nothing of the lockstep call or of the table calls is restated
    for once in ("int ring_track(", "int plan_ring_track(", "int ring_track_each(", "int plan_ring_track_each(", "int track_at(", "int track_each(", "int plan_track_at("):
        assert src.count(once) == 1, once


def test_the_kernels_are_a_unit_of_their_own():
    unit = strip_comments(read_csrc("glv_ring_each.hip"))
    assert "asm" not in unit and "atomic" not in unit and "__shared__" not in unit
    assert unit.count("capped_grid((size_t) items, 1, kRingTrackGridCap)") == 2 and "(uint64_t) j * r.pitch" in unit and "(uint64_t) j * r.n" in unit
    for kernel in ("glv_ring_stage_each_kernel", "glv_ring_keep_each_kernel"):
        assert unit.count("__global__ void __launch_bounds__(256) " + kernel + "(") == 1, kernel
    for launcher in (r"\nhipError_t launch_ring_each_stage\(", r"\nhipError_t launch_ring_each_keep\("):
        assert function_body(unit, launcher).lstrip("{ \n").startswith("if (!ring_each_ok(f32, e)) return hipErrorInvalidValue;"), launcher
    assert_launch_only(unit, [r"\nhipError_t launch_ring_each_stage\(", r"\nhipError_t launch_ring_each_keep\("])
    header = read_csrc("glv_launch.h")
    assert "hipError_t launch_ring_each_stage(bool f32, const RingTrackEach& e, hipStream_t st);" in header
    assert "hipError_t launch_ring_each_keep(bool f32, const RingTrackEach& e, hipStream_t st);" in header
    from glava_amd import build as B
    assert "glv_ring_each" in B.SMALL and "glv_ring_track" in B.SMALL


# ---- the per-stream window rule, in integers ---------------------------------------------------------------------------------------------------------------
def _rule(ring_oldest_first, new, n, nf, c):
    """the contract for a stream that takes c updates: windows [(t + 1) * nf, (t + 1) * nf + n) of R = ring ‖ the first c * nf new frames, and the ring
    afterwards (oldest first): the last n frames of R"""
    r = np.concatenate([ring_oldest_first, new[:c * nf]])
    return [r[(t + 1) * nf:(t + 1) * nf + n] for t in range(c)], r[len(r) - n:]


@pytest.mark.parametrize("n", [64, 256])
@pytest.mark.parametrize("nf", [1, 37, 64, "n"])
@pytest.mark.parametrize("c", [0, 1, 3, 10])
def test_a_stream_s_windows_and_ring_are_those_of_its_own_appends(n, nf, c):
    nf = n if nf == "n" else nf
    updates = 10                                                                 # the longest row: the new frames lie at its pitch whatever c is
    rng = np.random.default_rng(n * 1000 + nf * 10 + c)
    for pos in (0, 1, 37 % n, n - 1):
        ring = rng.integers(-30000, 30000, size=n)                             # the array as it lies: the oldest frame at `pos`
        new = rng.integers(-30000, 30000, size=updates * nf)
        oldest_first = np.concatenate([ring[pos:], ring[:pos]])
        want, ring_want = _appended_windows(ring, pos, new, n, nf, c)
        got, ring_got = _rule(oldest_first, new, n, nf, c)
        assert len(got) == len(want) == c
        for t in range(c):
            assert (got[t] == want[t]).all(), (n, nf, c, pos, t)
        assert (ring_got == ring_want).all(), (n, nf, c, pos)
        if c == 0:
            assert (ring_got == oldest_first).all()
        # the staged table's entries behind the count stay inside the staged region
        pitch = (n + updates * nf + 3) & ~3
        assert all((t + 1) * nf <= pitch - n for t in range(updates))


# ---- ring_update_counts -------------------------------------------------------------------------------------------------------------------------------------
def test_ring_update_counts_is_the_plain_loop():
    rng = np.random.default_rng(3)
    for nf in (1, 37, 256):
        for cap in (None, 1, 4, 1000):
            pending = [int(v) for v in rng.integers(0, 40 * nf, size=33)] + [0, nf - 1, nf, nf + 1, 5 * nf]
            counts, updates, leftover = ring_update_counts(pending, nf, cap)
            assert counts.dtype == np.uint32 and counts.shape == (len(pending),) and isinstance(updates, int) and all(isinstance(v, int) for v in leftover)
            longest = 0
            for i, frames in enumerate(pending):
                c, left = 0, frames
                while left >= nf and (cap is None or c < cap):
                    c, left = c + 1, left - nf
                assert (int(counts[i]), leftover[i]) == (c, left), (nf, cap, frames)
                longest = max(longest, c)
            assert updates == longest
    assert ring_update_counts([0, 3], 4)[1] == 0                                 # nothing to call
    assert ring_update_counts(np.asarray([512, 100]), 256)[2] == [0, 100]        # numpy integers in, Python ints out
    for bad in (dict(pending_frames=[], new_frames=1), dict(pending_frames=[1], new_frames=0), dict(pending_frames=[-1], new_frames=1), dict(pending_frames=[1.5], new_frames=1),
                dict(pending_frames=[True], new_frames=1), dict(pending_frames=[1], new_frames=1, cap=0), dict(pending_frames=[1 << 40], new_frames=1)):
        with pytest.raises(ValueError):
            ring_update_counts(**bad)
