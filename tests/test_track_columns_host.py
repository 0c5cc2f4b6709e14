"""CPU: track mode for the graph module (glv_batch_track_columns_s16 / _f32) without a device -- the exported symbols, their header declarations and
Python prototypes; a host walk of the texel-row kind of glv_columns_kernel's row loop (tests/emu/cols_tex_emu.cpp, built here) against the oracle's
texels of the twin (bars = n, phase 0.5) pushed through the contract formula, and against the float-row walk on rows c / 65535.  (The scan's store
limit, which the issue's last test was about, was measured level with full stores and deleted: profiles/r14/track_columns.txt.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from glava_amd.bar_positions import graph_column_texels
from src_scan import ROOT, TRACK_EXECUTOR, assert_launch_only, function_body, read_csrc, read_host_src, strip_comments

F = np.float32
ENTRIES = ("glv_batch_track_columns_s16", "glv_batch_track_columns_f32")


def contract(T, table):
    """out[x] = fdiv(fadd(fadd(T(l), T(m)), T(r)), 3.0f) in numpy float32 (every operation rounded on its own)"""
    lm = (T[table[:, 0]] + T[table[:, 1]]).astype(F)
    return ((lm + T[table[:, 2]]).astype(F) / F(3.0)).astype(F)


def texel_floats(c):
    return (np.asarray(c).astype(F) / F(65535)).astype(F)


def test_track_columns_symbols_are_exported_declared_and_bound(glvlib):
    L = C.CDLL(glvlib.LIB_PATH)
    lib = glvlib.lib()
    header = open(os.path.join(ROOT, "include", "glv_spectrum.h")).read()
    assert hasattr(L, "glv_batch_track_columns_work_bytes")
    assert "\nuint64_t glv_batch_track_columns_work_bytes(const glv_batch* b, uint32_t pitch_frames, uint32_t hop, uint32_t steps, unsigned ops);" in header
    assert lib.glv_batch_track_columns_work_bytes.restype is C.c_uint64 and len(lib.glv_batch_track_columns_work_bytes.argtypes) == 5
    for name, ctype in zip(ENTRIES, (r"const int16_t\*", r"const float\*  ?")):
        assert hasattr(L, name), name
        assert len(getattr(lib, name).argtypes) == 9, name
        assert re.search(r"\nint " + name + r"\(glv_batch\* b, " + ctype + r" ?d_pcm, uint32_t pitch_frames, uint32_t hop, uint32_t steps, void\* d_out, void\* d_work,\s+unsigned ops, "
                         r"void\* hip_stream\);", header), name
    assert not hasattr(L, "glv_batch_track_columns_f32_work_bytes")           # one query sizes both entries
    for meth in ("track_columns_work_bytes", "track_columns_s16", "track_columns_f32"):
        assert callable(getattr(glvlib.Batch, meth)), meth
    assert lib.glv_abi_version() == 7                                        # added within the ABI: detected by the symbol


def test_track_columns_path_launches_and_nothing_else():
    src = read_host_src()
    assert_launch_only(src, [r"\nint plan_track_columns\(", r"\nint track_columns\(", r"\nint windows_args\(", r"\nvoid windows_geometry\(",
                             r"\nuint64_t glv_batch_track_columns_work_bytes\("] + [r"\nint " + e + r"\(" for e in ENTRIES] + TRACK_EXECUTOR)
    bars = read_csrc("glv_bars.hip")
    assert_launch_only(bars, [r"\nhipError_t launch_columns_texels\("])
    # the entries add no stage of their own: the plan, then the executor of the other FFT forms
    for name in ENTRIES:
        body = strip_comments(function_body(src, r"\nint " + name + r"\("))
        assert "plan_track_columns(" in body and "track(b, tp," in body and "glv::launch_" not in body, name
    # the refusals the other track plans make are made by the same functions here, not by copies
    body = strip_comments(function_body(src, r"\nint plan_track_columns\("))
    assert "track_args(" in body and "track_chain(" in body and "windows_args(" in body and "check_ops(" not in body
    # the other entries' refusal of column texels stands
    assert 'a track call has no columns form' in function_body(src, r"\nint track_chain\(")


@pytest.fixture(scope="module")
def colstex(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "emu", "cols_tex_emu.cpp")
    so = str(tmp_path_factory.mktemp("colstex") / "libcolstex.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src], check=True)
    L = C.CDLL(so)
    L.colstex_columns.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_float, C.c_int, C.c_void_p]
    L.colstex_columns.restype = C.c_int
    return L


def _rows(n, seed):
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 65536, size=(3, n), dtype=np.uint16)
    rows[1, : n // 4] = 65535                                               # the largest sums
    rows[2] = (rng.random(n) < 0.5) * rng.integers(0, 65536, size=n)
    return rows


def _walk(L, rows, n, table, mode, texel_rows, sf=0.025, hybrid=0.65):
    out = np.zeros((rows.shape[0], len(table)), F)
    rc = L.colstex_columns(rows.ctypes.data, rows.shape[0], n, table.ctypes.data, len(table), C.c_float(sf), mode, C.c_float(hybrid), int(texel_rows), out.ctypes.data)
    assert rc == 0, rc
    return out


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("n,W", [(1024, 100), (1024, 320), (4096, 320), (4096, 800)])
def test_texel_row_walk_equals_the_twin_through_the_contract_and_the_float_row_walk(colstex, oracle, n, W, mode):
    """the texel-row kind: bit for bit the twin's texels (average: the oracle's exact integer pass; maximum / hybrid: its float loop, then the GL_R16
    conversion) through the contract formula, and bit for bit the float-row kind on rows c / 65535"""
    rows = _rows(n, n + W + mode)
    table = np.ascontiguousarray(graph_column_texels(n, W)[0], np.uint32)
    texel = _walk(colstex, rows, n, table, mode, True)
    floats = _walk(colstex, rows, n, table, mode, False)
    assert (texel.view(np.uint32) == floats.view(np.uint32)).all()
    assert np.isfinite(texel).all() and texel.max() > 0
    for r in range(rows.shape[0]):
        if mode == 0:
            t, _ = oracle.bars_int(rows[r], n, smooth_factor=0.025, phase=0.5)
        else:
            t = oracle.texels_r16(oracle.bars_mode(texel_floats(rows[r]), n, mode, hybrid_weight=0.65, smooth_factor=0.025, phase=0.5))
        want = contract(texel_floats(t), table.astype(np.int64))
        assert (texel[r].view(np.uint32) == want.view(np.uint32)).all(), (r, int((texel[r].view(np.uint32) != want.view(np.uint32)).sum()))
