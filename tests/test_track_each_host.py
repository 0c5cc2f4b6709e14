"""CPU: track mode per stream (glv_batch_track_each_s16 / _f32 / _f32_planar) without a device -- the exported symbols, the ctypes mirror of
glv_track_tables against the header field by field, glava_amd.track_starts.stack_tables against the per-stream tables it stacks, and a numpy restatement of
the rule by which a stream's ring is presented at the batch's head, held to the portable order of glava_amd.stream_slots (glv_batch_stream_state_desc)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from glava_amd.stream_slots import unrotate
from glava_amd.track_starts import live_session_rates, renderer_starts, stack_tables
from src_scan import ROOT, function_body, read_csrc, read_host_src, strip_comments

SYMBOLS = ("glv_batch_track_each_s16", "glv_batch_track_each_f32", "glv_batch_track_each_f32_planar")
CTYPES_OF = {"const uint32_t*": C.c_void_p, "const float*": C.c_void_p}


def test_track_each_symbols_are_exported_bound_and_declared(glvlib):
    L = C.CDLL(glvlib.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(L, name), name
    lib = glvlib.lib()
    header = strip_comments(open(os.path.join(ROOT, "include", "glv_spectrum.h")).read())
    for name in SYMBOLS:
        fn = getattr(lib, name)
        assert len(fn.argtypes) == 9 and fn.argtypes[3] is not C.c_void_p, name          # the tables travel as a pointer to the structure
        assert fn.argtypes[3]._type_ is glvlib.TrackTables, name
        decl = re.search(r"\nint " + name + r"\s*\(([^;]*)\);", header)
        assert decl, name
        args = [a.strip() for a in decl.group(1).split(",")]
        assert len(args) == 9 and args[3] == "const glv_track_tables* tb" and args[4] == "uint32_t steps", (name, args)
    for meth in ("track_each_s16", "track_each_f32", "track_each_f32_planar"):
        assert callable(getattr(glvlib.Batch, meth)), meth
    assert lib.glv_abi_version() == 7                                            # added within the ABI: detected by the symbol
    assert not hasattr(L, "glv_batch_track_each_work_bytes")                     # sized by glv_batch_track_at_work_bytes: there is no other query


def test_the_ctypes_structure_is_the_header_s_field_by_field(glvlib):
    header = strip_comments(open(os.path.join(ROOT, "include", "glv_spectrum.h")).read())
    body = re.search(r"typedef struct glv_track_tables \{(.*?)\} glv_track_tables;", header, re.S)
    assert body
    fields = []
    for line in body.group(1).split(";"):
        line = " ".join(line.split())
        if not line: continue
        m = re.fullmatch(r"(const uint32_t\*|const float\*) (\w+)", line)
        assert m, line
        fields.append((m.group(2), m.group(1)))
    assert fields == [("d_starts", "const uint32_t*"), ("d_ur", "const float*"), ("d_counts", "const uint32_t*")]
    mirror = glvlib.TrackTables._fields_
    assert [n for n, _ in mirror] == [n for n, _ in fields]
    for (name, ctype), (_, ctext) in zip(mirror, fields):
        assert ctype is CTYPES_OF[ctext], name
        assert getattr(glvlib.TrackTables, name).offset == 8 * [n for n, _ in fields].index(name), name
    assert C.sizeof(glvlib.TrackTables) == 24


def test_track_each_refuses_without_a_device(glvlib):
    lib = glvlib.lib()
    tb = glvlib.TrackTables(None, None, None)
    for name in SYMBOLS:
        assert getattr(lib, name)(None, None, 0, C.byref(tb), 0, None, None, glvlib.OP_FFT, None) == glvlib.ERR_INVALID, name
        assert getattr(lib, name)(None, None, 0, None, 0, None, None, glvlib.OP_FFT, None) == glvlib.ERR_INVALID, name


def test_the_entries_add_one_executor_and_no_plan():
    src = strip_comments(read_host_src())
    for name in SYMBOLS:
        body = function_body(src, r"\nint " + name + r"\(")
        assert "track_each(b, " in body and "glv::launch_" not in body and "for (" not in body and "hipMalloc" not in body and "Synchronize" not in body, name
    body = function_body(src, r"\nint track_each\(glv_batch\* b,")
    assert "track_at(b, d_pcm," in body and "tb->d_ur)" in body
    for absent in ("glv::launch_", "for (", "while (", "plan_track", "TrackPlan", "hipMalloc", "Synchronize"):
        assert absent not in body, absent
    for refusal in ("!tb", "tb->d_ur) & 3u", "tb->d_counts) & 3u", "ops & GLV_OP_WAVE", "!(ops & GLV_OP_GRAVITY)", "!(ops & (GLV_OP_GRAVITY | GLV_OP_AVERAGE))"):
        assert refusal in body, refusal
    # the rates' refusals in the rates call's words
    rates = function_body(src, r"\nint track_rates\(glv_batch\* b,")
    for words in ('"GLV_OP_WAVE is stateless: no gravity reads the rate table (glv_batch_track_at_s16 / _f32; ops 0x%x)"',
                  '"a rates track call needs GLV_OP_GRAVITY, which reads the rate table (ops 0x%x)"'):
        assert words in rates and words in body, words
    # one plan, one scan stage: the per-stream call is carried by the table call's plan and executor
    assert src.count("int plan_track_at(") == 1 and src.count("int track_scan(") == 1 and src.count("int track_windows(") == 1 and src.count("int track_wave(") == 1
    assert "launch_track_each_scan(" in function_body(src, r"\nint track_scan\(") and src.count("launch_track_each_scan(") == 1
    # the kernels: the shared-table kinds keep their index, the per-stream kinds and the decimation read through the one rule
    frame, tmpl, dec, misc = (strip_comments(read_csrc(f)) for f in ("glv_frame.h", "glv_kernel_tmpl.h", "glv_decimate.hip", "glv_misc.hip"))
    assert "return w.starts[f % w.table_len];" in function_body(frame, r"uint32_t track_table_entry\(")
    assert "if constexpr (TRACK_EACH) return track_table_entry(a.trk, f);" in tmpl and "track_table_entry(d.w, f)" in dec
    assert misc.count("w.starts[(size_t) stream * w.hop + step]") == 3       # glv_wave_kernel's three window kinds
    kernel = function_body(misc, r"glv_track_each_scan_kernel\(const FrameArgs a, const TrackGeometry t, const TrackEach e\)")
    assert "const uint32_t turn = (t.steps - c) % F;" in kernel and "e.counts[stream]" in kernel and "t.ur" not in kernel
    assert "gravity_r16(tex, store, a.g, a.grav_sub, a.grav_int)" in kernel          # counts alone on texel state: the packed integer step, not the float form
    for line in kernel.split("\n"):
        if "ur[" in line or "gravity_r16_flt(" in line or "t.gravity_step" in line:
            assert "if constexpr (RATES)" in line, line


# ---- stack_tables ----------------------------------------------------------------------------------------------------------------------------------------
def test_stack_tables_pads_with_the_last_entry_and_reports_the_lengths():
    sessions = [live_session_rates(22050, 60, 40, 256), live_session_rates(22050, 30, 9, 256), live_session_rates(44100, 24, 31, 512)]
    rows = [(s, ur) for s, _, ur in sessions]
    starts, ur, counts = stack_tables(rows)
    steps = max(len(s) for s, _ in rows)
    assert starts.dtype == np.uint32 and ur.dtype == np.float32 and counts.dtype == np.uint32
    assert starts.shape == ur.shape == (3, steps) and counts.shape == (3,)
    assert len({len(s) for s, _ in rows}) == 3                                   # three different lengths
    for i, (s, u) in enumerate(rows):
        assert counts[i] == len(s) == len(u)
        assert starts[i, :len(s)].tolist() == s and ur[i, :len(u)].tolist() == u
        assert (starts[i, len(s):] == s[-1]).all() and (ur[i, len(u):] == np.float32(u[-1])).all()
    # a longer table on request; the counts stay the streams' own
    starts2, ur2, counts2 = stack_tables(rows, steps=steps + 5)
    assert starts2.shape == (3, steps + 5) and (counts2 == counts).all() and (starts2[:, :steps] == starts).all() and (ur2[:, steps:] == ur[:, -1:]).all()


def test_stack_tables_without_rates_and_with_a_stream_that_stands_still():
    a, b = renderer_starts(22050, 60, 1, 7), renderer_starts(44100, 24, 1, 3)
    starts, ur, counts = stack_tables([(a, None), (b, None), ([], None)])
    assert ur is None and counts.tolist() == [7, 3, 0]
    assert starts[0].tolist() == a and starts[1].tolist() == b + [b[-1]] * 4 and starts[2].tolist() == [0] * 7
    starts, ur, counts = stack_tables([(a, [2.0] * 7), (b, None), ([], [])])
    assert ur[0].tolist() == [2.0] * 7 and ur[1].tolist() == [1.0] * 7 and ur[2].tolist() == [1.0] * 7 and counts.tolist() == [7, 3, 0]


def test_stack_tables_refuses_malformed_rows():
    for bad in ([], [([1, 2], [1.0])], [([1, 2, 3], None)], [([-1], None)], [([1 << 32], None)], [([1.5], None)], [([], None)]):
        with pytest.raises(ValueError):
            stack_tables(bad, steps=2) if bad != [([], None)] else stack_tables(bad)
    with pytest.raises(ValueError):
        stack_tables([([1], None)], steps=0)


# ---- the ring, presented at the batch's head ---------------------------------------------------------------------------------------------------------------
def _walk(ring, head, frames):
    """`frames` sequential updates of one stream: each goes into slot `head`, which then advances (glv_frame.h apply_state; the host's head after a call)"""
    ring, F = ring.copy(), len(ring)
    for v in frames:
        ring[head] = v
        head = (head + 1) % F
    return ring, head


@pytest.mark.parametrize("F", [1, 2, 3, 5, 8])
def test_a_ring_turned_by_steps_minus_count_reads_at_the_batch_s_head_as_the_stream_s_own(F):
    """slot p of the stream's own walk stored to slot (p + steps - c) % F: in the portable order -- row q is ring slot (head + q) mod F, oldest first
    (stream_slots.unrotate) -- the batch's head after `steps` then shows what the stream's own head after c shows.  c = 0: the state as it was."""
    rng = np.random.default_rng(F)
    for head in range(F):
        for steps in (1, 2, 5, 6, 11):
            for c in sorted({0, 1, steps // 2, steps - 1, steps} - {-1}):
                before = rng.integers(1, 1 << 30, size=F)
                own, own_head = _walk(before, head, 1000 + np.arange(c))
                assert own_head == (head + c) % F
                stored = np.empty_like(own)
                for p in range(F):
                    stored[(p + steps - c) % F] = own[p]
                batch_head = (head + steps) % F
                assert (unrotate(stored, batch_head) == unrotate(own, own_head)).all(), (F, head, steps, c)
                if c == 0:
                    assert (unrotate(stored, batch_head) == unrotate(before, head)).all()
                # the gravity source of the next step under both heads: the newest row
                newest = lambda ring, h: ring[(h + F - 1) % F]                # noqa: E731
                assert newest(stored, batch_head) == newest(own, own_head)
