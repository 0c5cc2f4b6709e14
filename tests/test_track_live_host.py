"""CPU: track mode for GLV_OP_BARS_ONLY batches (glv_batch_track_live_s16 / _f32) without a device -- the exported symbols, their header declarations
and Python prototypes; the shape of the plan in the host sources; and the kept-bins rule against the work lists of the chunked float bars
(tests/emu/live_kept_emu.cpp, built here).  (The host walk of the stateless live epilogue left with the live transform classes, which were measured level
with the full-row ones at 64 streams: profiles/r15/track_live_rule.txt.)"""
import ctypes as C
import os
import re
import subprocess

import pytest

from src_scan import ROOT, TRACK_EXECUTOR, assert_launch_only, function_body, read_host_src, strip_comments

ENTRIES = ("glv_batch_track_live_s16", "glv_batch_track_live_f32")


def test_track_live_symbols_are_exported_declared_and_bound(glvlib):
    L = C.CDLL(glvlib.LIB_PATH)
    lib = glvlib.lib()
    header = open(os.path.join(ROOT, "include", "glv_spectrum.h")).read()
    assert hasattr(L, "glv_batch_track_live_work_bytes")
    assert "\nuint64_t glv_batch_track_live_work_bytes(const glv_batch* b, uint32_t pitch_frames, uint32_t hop, uint32_t steps, unsigned ops);" in header
    assert lib.glv_batch_track_live_work_bytes.restype is C.c_uint64 and len(lib.glv_batch_track_live_work_bytes.argtypes) == 5
    for name, ctype in zip(ENTRIES, (r"const int16_t\*", r"const float\*  ?")):
        assert hasattr(L, name), name
        assert len(getattr(lib, name).argtypes) == 9, name
        assert re.search(r"\nint " + name + r"\(glv_batch\* b, " + ctype + r" ?d_pcm, uint32_t pitch_frames, uint32_t hop, uint32_t steps, void\* d_out, void\* d_work,\s+unsigned ops, "
                         r"void\* hip_stream\);", header), name
    assert not hasattr(L, "glv_batch_track_live_f32_work_bytes")              # one query sizes both entries
    for meth in ("track_live_work_bytes", "track_live_s16", "track_live_f32"):
        assert callable(getattr(glvlib.Batch, meth)), meth
    assert lib.glv_abi_version() == 7                                        # added within the ABI: detected by the symbol


def test_the_live_plan_decides_nothing_itself():
    src = read_host_src()
    assert_launch_only(src, [r"\nint plan_track_live\(", r"\nuint32_t kept_bins\(", r"\nuint64_t glv_batch_track_live_work_bytes\("]
                       + [r"\nint " + e + r"\(" for e in ENTRIES] + TRACK_EXECUTOR)
    plain = strip_comments(src)
    body = function_body(plain, r"\nint plan_track_live\(")
    for call in ("track_args(", "windows_args(", "track_chain(", "windows_geometry("):
        assert call in body, call
    for decided_once in ("tp.state =", "tp.in16 =", "tp.out16 =", "tp.bars =", "tp.kept =", "check_ops(", "gl_storage == 2", "GLV_OP_BARS_ONLY", "single_row", "live_bins(", "columns()"):
        assert decided_once not in body, decided_once
    # the entries add no stage of their own: the plan, then the executor of the other FFT forms
    for name in ENTRIES:
        body = function_body(plain, r"\nint " + name + r"\(")
        assert "plan_track_live(" in body and "track(b, tp," in body and "glv::launch_" not in body and "for (" not in body, name
    # one scan launch in the host sources, one transform launch of the windows form, no loop in the executor
    assert plain.count("launch_track_scan(") == 1
    assert function_body(plain, r"\nint track_windows\(").count("glv::launch_frame(") == 1
    for sig in (r"\nint track\(glv_batch\* b,", r"\nint track_scan\("):
        body = function_body(plain, sig)
        assert "for (" not in body and "while (" not in body, sig
    # the four older refusals of a flagged batch stand, and the live form's refusal of an unflagged one names the entries that take it
    chain = function_body(src, r"\nint track_chain\(")
    assert "its state beyond the live bins does not exist, which the scan over time would read" in chain
    assert "glv_batch_track_windows_* / glv_batch_track_columns_*" in chain


@pytest.fixture(scope="module")
def liveemu(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "emu", "live_kept_emu.cpp")
    so = str(tmp_path_factory.mktemp("liveemu") / "libliveemu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src], check=True)
    L = C.CDLL(so)
    L.live_emu_kept.argtypes = [C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]; L.live_emu_kept.restype = C.c_uint32
    return L


@pytest.mark.parametrize("n,bars,phase", [(1024, 80, 0.0), (2048, 64, 0.0), (4096, 80, 0.0), (256, 80, 0.0), (16384, 80, 0.0), (1024, 255, 0.5)])
def test_kept_bins_cover_every_chunk_the_float_bars_read(liveemu, n, bars, phase):
    """the chains of tests/test_track_live.py whose third launch is the chunked float bars (80 bars of n = 1024, 64 bars of n = 2048) and their
    neighbours: K is a multiple of 64 that covers the live bins and first_bin + chunk of every work-list item"""
    live, reach = C.c_uint32(0), C.c_uint32(0)
    K = liveemu.live_emu_kept(n, bars, 0.025, phase, C.byref(live), C.byref(reach))
    assert reach.value > 0 and live.value > 0
    assert K % 64 == 0 and K >= live.value and K >= reach.value, (n, bars, K, live.value, reach.value)
    assert K - 64 < max(live.value, reach.value), "not the smallest"
