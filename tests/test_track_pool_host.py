"""CPU: track mode over a pool of recordings (glv_batch_track_pool_s16 / _f32 / _f32_planar) without a device -- the exported symbols, the ctypes mirror of
glv_track_span against the header field by field, the refusals that need no device, the shape of the host code (one executor, no plan, nothing but launches),
and glava_amd.track_starts.pool_window_start / pool_spans against hand-computed cases of the rule the kernels evaluate (glv_frame.h pool_window_start, which
static_asserts pin in the library's own build)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from glava_amd.track_starts import SPAN_DTYPE, pool_spans, pool_window_start
from src_scan import ROOT, assert_launch_only, function_body, read_csrc, read_host_src, strip_comments

SYMBOLS = ("glv_batch_track_pool_s16", "glv_batch_track_pool_f32", "glv_batch_track_pool_f32_planar")


def test_track_pool_symbols_are_exported_bound_and_declared(glvlib):
    L = C.CDLL(glvlib.LIB_PATH)
    lib = glvlib.lib()
    header = strip_comments(open(os.path.join(ROOT, "include", "glv_spectrum.h")).read())
    for name in SYMBOLS:
        assert hasattr(L, name), name
        fn = getattr(lib, name)
        assert len(fn.argtypes) == 10 and fn.argtypes[2] is C.c_uint64 and fn.argtypes[4]._type_ is glvlib.TrackTables, name
        decl = re.search(r"\nint " + name + r"\s*\(([^;]*)\);", header)
        assert decl, name
        args = [" ".join(a.split()) for a in decl.group(1).split(",")]
        assert len(args) == 10 and args[2] == "uint64_t pool_frames" and args[3] == "const glv_track_span* d_spans" and args[4] == "const glv_track_tables* tb", (name, args)
    for meth in ("track_pool_s16", "track_pool_f32", "track_pool_f32_planar"):
        assert callable(getattr(glvlib.Batch, meth)), meth
    assert lib.glv_abi_version() == 7                                            # added within the ABI: detected by the symbol
    assert not hasattr(L, "glv_batch_track_pool_work_bytes")                     # sized by glv_batch_track_at_work_bytes: there is no other query


def test_the_span_structure_is_the_header_s_field_by_field(glvlib):
    header = strip_comments(open(os.path.join(ROOT, "include", "glv_spectrum.h")).read())
    body = re.search(r"typedef struct glv_track_span \{(.*?)\} glv_track_span;", header, re.S)
    assert body
    fields = [tuple(" ".join(line.split()).split(" ")) for line in body.group(1).split(";") if line.strip()]
    assert fields == [("uint64_t", "first"), ("uint32_t", "frames"), ("uint32_t", "reserved")]
    T = glvlib.TrackSpan
    assert [n for n, _ in T._fields_] == ["first", "frames", "reserved"]
    assert (T.first.offset, T.frames.offset, T.reserved.offset) == (0, 8, 12) and C.sizeof(T) == 16
    assert (T.first.size, T.frames.size, T.reserved.size) == (8, 4, 4)
    dt = np.dtype(SPAN_DTYPE)
    assert dt.itemsize == 16 and [dt.fields[n][1] for n in ("first", "frames", "reserved")] == [0, 8, 12]
    frame = strip_comments(read_csrc("glv_frame.h"))
    assert "struct alignas(16) TrackSpan { uint64_t first; uint32_t frames, reserved; };" in frame


def test_track_pool_refuses_without_a_device(glvlib):
    lib = glvlib.lib()
    tb = glvlib.TrackTables(None, None, None)
    for name in SYMBOLS:
        assert getattr(lib, name)(None, None, 0, None, C.byref(tb), 0, None, None, glvlib.OP_FFT, None) == glvlib.ERR_INVALID, name     # a NULL batch
        assert getattr(lib, name)(None, 16, 1 << 20, 16, C.byref(tb), 1, None, None, glvlib.OP_FFT, None) == glvlib.ERR_INVALID, name
    src = strip_comments(read_host_src())
    body = function_body(src, r"\nint track_pool\(glv_batch\* b,")
    assert body.index("!b") < body.index("!d_pool || !d_spans") < body.index("d_spans) & 15u") < body.index("pool_frames < window_frames(b)") < body.index("track_each(b, d_pool,")


def test_the_entries_add_one_executor_and_no_plan():
    raw = read_host_src()
    assert_launch_only(raw, [r"\nint track_pool\(glv_batch\* b,"] + [r"\nint " + name + r"\(" for name in SYMBOLS])
    src = strip_comments(raw)
    for name in SYMBOLS:
        body = function_body(src, r"\nint " + name + r"\(")
        assert "track_pool(b, " in body and "glv::launch_" not in body and "for (" not in body and "hipMalloc" not in body and "Synchronize" not in body, name
    body = function_body(src, r"\nint track_pool\(glv_batch\* b,")
    for absent in ("glv::launch_", "for (", "while (", "plan_track", "TrackPlan", "hipMalloc", "Synchronize"):
        assert absent not in body, absent
    # one plan, one scan stage, one transform launch: the pool travels in TrackInput through the per-stream call and the table call
    assert src.count("int plan_track_at(") == 1 and src.count("int track_scan(") == 1 and src.count("int track_windows(") == 1 and src.count("int track_wave(") == 1
    assert src.count("int track_pool(") == 1 and "glv::TrackPool pool" in src[src.index("struct TrackInput"):src.index("struct TrackPlan")]
    windows = function_body(src, r"\nint track_windows\(")
    assert windows.count("glv::launch_frame(") == 1 and "glv::IN_S16_TRACK_POOL" in windows and "glv::launch_decimate_pool(" in windows
    assert "launch_plan(b, a.units, hop_mode," in windows                         # planned as the sibling: the same plan row, the same wisdom
    assert "glv::launch_wave_track_pool(" in function_body(src, r"\nint track_wave\(glv_batch\* b,")
    # (a single-row batch is refused by the table call's own plan, which the pool call goes through; on the GPU: tests/test_track_pool.py)
    assert "b->single_row" in function_body(src, r"\nint track_chain\(") and "b->single_row" in function_body(src, r"\nint plan_track_wave\(")
    assert "glv::kPoolTrackKinds" in function_body(src, r"\nint batch_prepare\(")    # the new kinds' attributes are set at creation: a first call can be captured
    # the kernels: kinds of their own behind the old numbers, parts of their own, a unit of their own; one rule for the start
    frame, tmpl, inst, pool = (strip_comments(read_csrc(f)) for f in ("glv_frame.h", "glv_kernel_tmpl.h", "glv_inst.hip", "glv_pool.hip"))
    assert "IN_S16_TRACK_POOL = IN_S16_TRACK_EACH + kEachTrackKinds" in frame and "uint64_t pool_window_start(" in frame
    assert tmpl.count("pool_window_start(") == 1 and pool.count("pool_window_start(") == 1
    for kind, part in (("IN_S16_TRACK_POOL", "_part11"), ("IN_F32_TRACK_POOL", "_part12"), ("IN_F32_PLANAR_TRACK_POOL", "_part13")):
        assert inst.count(f"launch_log<{kind}, 0>") == 1 and inst.count(f"launch_log<{kind}, 1>") == 1, kind
        assert f"if (in_mode == {kind}) return GLV_CAT(GLV_CAT(launch_frame_, GLV_LOG_NN), {part})" in inst
    from glava_amd import build as B
    assert B.POOL_PARTS == (11, 12, 13) and B.EACH_PARTS == (8, 9, 10) and "glv_pool" in B.SMALL and "-ffp-contract=off" in B.HIPFLAGS
    assert "asm" not in pool
    for static in ("first = 2^33", "entry 0xFFFFFFFF", "frames < k n", "first + frames > pool_frames", "first >= pool_frames"):
        assert static in read_csrc("glv_frame.h"), static                         # the static_asserts that pin the 64-bit cases


# ---- the rule, in integers ---------------------------------------------------------------------------------------------------------------------------------
def test_pool_window_start_on_hand_computed_cases():
    n = 1024
    assert pool_window_start(0, 5000, 0, 5000, n) == 0
    assert pool_window_start(0, 5000, 3976, 5000, n) == 3976 and pool_window_start(0, 5000, 3977, 5000, n) == 3976
    assert pool_window_start(8, 5000, 100, 1 << 20, n) == 108
    assert pool_window_start(1 << 33, 5000, 100, (1 << 33) + 5000, n) == (1 << 33) + 100          # first > 2^32
    assert pool_window_start((1 << 32) + 3, 5000, 0xFFFFFFFF, 1 << 34, n) == (1 << 32) + 3 + 3976  # the largest entry: the span's last window
    assert pool_window_start((1 << 32) - 8, 0xFFFFFFFF, 0xFFFFF000, 1 << 34, n) == (1 << 33) - 4104  # nothing wraps at 32 bits
    assert pool_window_start(700, 1000, 77, 1 << 20, n) == 700                                    # frames < k n: every entry clamps to 0
    assert pool_window_start(700, n, 77, 1 << 20, n) == 700                                       # exactly one window
    assert pool_window_start(9000, 5000, 3000, 10000, n) == 8976                                  # first + frames > pool_frames: the pool's last window
    assert pool_window_start(10000, 5000, 0, 10000, n) == 8976 and pool_window_start((1 << 64) - 1, 5000, 3000, 10000, n) == 8976   # first >= pool_frames
    assert pool_window_start(0, n, 5, n, n) == 0                                                  # a pool of one window
    assert pool_window_start(0, 3 * n, 2 * n + 1, 3 * n, 3 * n) == 0                               # bufscale 3: the window is k n
    rng = np.random.default_rng(5)
    for _ in range(2000):                                                                          # never outside the pool, never outside a well-formed span
        pool = int(rng.integers(n, 1 << 40))
        first, frames, entry = int(rng.integers(0, 1 << 41)), int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32))
        w = pool_window_start(first, frames, entry, pool, n)
        assert 0 <= w <= pool - n
        if frames >= n and first + frames <= pool:
            assert first <= w and w + n <= first + frames and w == first + min(entry, frames - n)
    for bad in (dict(first=-1), dict(frames=1 << 32), dict(entry=1 << 32), dict(pool_frames=n - 1), dict(window=0), dict(first=1.5)):
        kw = dict(first=0, frames=n, entry=0, pool_frames=n, window=n); kw.update(bad)
        with pytest.raises(ValueError):
            pool_window_start(**kw)


def test_pool_spans_packs_recordings_on_groups_of_8_frames():
    lengths = [5000, 1, 1024, 77777, 8]
    first, frames = pool_spans(lengths)
    assert first == [0, 5000, 5008, 6032, 83816] and frames == 83824
    for a, l, nxt in zip(first, lengths, first[1:] + [frames]):
        assert a % 8 == 0 and a + l <= nxt                                                         # aligned, disjoint, in order
    for a, l in zip(first, lengths):                                                               # well-formed spans: the outer clamp never binds
        if l >= 1024:
            assert pool_window_start(a, l, 0xFFFFFFFF, frames, 1024) == a + l - 1024
    assert pool_spans([3, 3, 3], align=1) == ([0, 3, 6], 9) and pool_spans([3, 3], align=16) == ([0, 16], 19)
    assert pool_spans(np.asarray([9, 9], dtype=np.uint32)) == ([0, 16], 25)


def test_pool_spans_refuses_malformed_lengths():
    for bad in ([], [0], [-1], [1 << 32], [1.5], [True], [8, None]):
        with pytest.raises(ValueError):
            pool_spans(bad)
    for align in (0, -8, 1.0):
        with pytest.raises(ValueError):
            pool_spans([8], align=align)
