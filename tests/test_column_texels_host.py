"""CPU: the graph module's columns (glv_batch_set_column_texels) -- the exported symbol, the position helpers against literal float32
restatements of graph/1.frag and circle/1.frag, the contract formula against an evaluation of smooth_audio_adj's shader text
(tests/glsl_eval.py; tests/golden/column_vectors.npz, generator committed) and a host walk of the fused epilogue's step and of the
second launch's row loop (tests/emu/cols_emu.cpp, built here) against the oracle's exact integer texels of the twin (bars = n,
phase 0.5) pushed through the contract formula."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from glava_amd.bar_positions import circle_texels, graph_column_texels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_column_golden import CASES, texel_floats, texel_row  # noqa: E402

F = np.float32
SIZES = [1024, 4096, 16384]
WIDTHS = [320, 510, 800, 801, 1280, 1920]


def contract(T, table):
    """out[x] = fdiv(fadd(fadd(T(l), T(m)), T(r)), 3.0f) in numpy float32 (every operation rounded on its own)"""
    lm = (T[table[:, 0]] + T[table[:, 1]]).astype(F)
    return ((lm + T[table[:, 2]]).astype(F) / F(3.0)).astype(F)


def test_set_column_texels_is_exported():
    so = os.path.join(ROOT, "glava_amd", "csrc", "libglvspectrum.so")
    if not os.path.exists(so):
        from glava_amd import build as B
        B.build(tune=False, verbose=False)
    L = C.CDLL(so)
    assert hasattr(L, "glv_batch_set_column_texels")
    hdr = open(os.path.join(ROOT, "include", "glv_spectrum.h")).read()
    assert "int glv_batch_set_column_texels(glv_batch* b, const uint32_t* texels /* [count][3]: left, middle, right */, uint32_t count);" in hdr


def _glsl_round(x):
    """Mesa's round(): half to even; whether x sat exactly on a half; the unclipped texel"""
    x = F(x)
    return int(np.rint(x)), bool(x - np.floor(x) == F(0.5))


def _graph_pixel(n, W, x, direction):
    """graph/1.frag:87-88 + main() for pixel x (gl_FragCoord.x = x: pixel_center_integer, graph/1.frag:2): (channel, idx, the three
    positions smooth_audio_adj fetches at), float32 operation by operation"""
    half_w = F(W // 2)                                                           # half_w = (screen.x / 2): integer division, then float
    pixel = F(F(1.0) / F(W))
    fx = F(x)
    if fx < half_w:
        ch, idx = 0, (fx if direction < 0 else F(half_w - fx))                    # LEFT_IDX
    else:
        ch, idx = 1, (F(F(-fx) + F(W)) if direction < 0 else F(fx - half_w))      # RIGHT_IDX
    p = F(idx / half_w)
    return ch, idx, (max(F(p - pixel), F(0.0)), p, min(F(p + pixel), F(1.0)))


def _fetch(pos, n):
    t, tie = _glsl_round(F(F(pos) * F(n)))
    return min(max(t, 0), n - 1), tie, t >= n


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("direction", [1, -1])
def test_graph_columns_equal_the_shader_pixel_by_pixel(n, W, direction):
    tex, ties, beyond = graph_column_texels(n, W)
    half = W // 2
    assert tex.shape == ties.shape == beyond.shape == (W - half + 1, 3) and tex.dtype == np.uint32
    seen = set()
    for x in range(W):
        ch, idx, pos = _graph_pixel(n, W, x, direction)
        i = int(idx)
        assert F(i) == idx and 0 <= i < len(tex)
        seen.add(i)
        for j in range(3):
            t, tie, bey = _fetch(pos[j], n)
            assert (tex[i, j], bool(ties[i, j]), bool(beyond[i, j])) == (t, tie, bey), (x, j)
    # `middle` = smooth_audio_adj(audio_l, sz, 1, pixel) and (audio_r, sz, 0, pixel): rows half_w and 0
    pixel = F(F(1.0) / F(W))
    for p, i in ((F(1.0), half), (F(0.0), 0)):
        for j, pos in enumerate((max(F(p - pixel), F(0.0)), p, min(F(p + pixel), F(1.0)))):
            t, tie, bey = _fetch(pos, n)
            assert (tex[i, j], bool(ties[i, j]), bool(beyond[i, j])) == (t, tie, bey)
    # either direction uses every row but one end: DIRECTION >= 0 reaches idx 0 .. half_w, DIRECTION < 0 idx 0 .. W - half_w
    assert seen == set(range(0, half + 1)) if direction >= 0 else seen == set(range(0, W - half + 1))
    # the figures of the table: for idx = 0 .. half_w two entries lie beyond the texture (the middle and right fetch of idx = half_w), none ties,
    # and for an even width neighbouring columns share texels (idx / half_w + pixel is the next column's idx / half_w - pixel) -- 2 count - 1
    # distinct ones unless n is too small for that; an odd width's pixel is not half a column, its columns share fewer
    assert beyond[: half + 1].sum() == 2 and beyond[half, 1] and beyond[half, 2]
    assert not ties.any()
    assert (tex < n).all()
    if W % 2 == 0 and n >= 2 * W:
        assert len(np.unique(tex[: half + 1])) == 2 * (half + 1) - 1


def _circle_literal(n, theta, rotate, invert):
    """circle/1.frag:34-46 for one angle, float32 operation by operation (GLSL mod(x, y) = x - y * floor(x / y))"""
    TWOPI, PI = F(6.28318530718), F(3.14159265359)
    idx = F(F(theta) + F(rotate))
    a = F(abs(idx))
    d = F(a - F(TWOPI * F(np.floor(F(a / TWOPI)))))
    if d > PI:
        idx = F(-np.sign(idx) * F(TWOPI - d))
    if invert > 0:
        idx = F(-idx)
    pos = F(F(abs(idx)) / F(PI + F(0.001)))
    t, tie = _glsl_round(F(pos * F(n)))
    return min(t, n - 1), bool(idx > 0), tie


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("rotate,invert", [(3.14159265359 / 2, 0), (3.14159265359 / 2, 1), (0.0, 0), (2.5, 0)])
def test_circle_texels_equal_the_shader(n, rotate, invert):
    theta = np.concatenate([np.array([np.pi, -np.pi, 0.0, 2 * np.pi, 7.0, -7.5, 9.42, 13.0]), np.linspace(-np.pi, np.pi, 721), np.linspace(-3 * np.pi, 5 * np.pi, 97)])
    tex, left, ties = circle_texels(n, theta, rotate, invert)
    assert tex.dtype == np.uint32 and len(tex) == len(theta) and (tex < n).all()
    for i, th in enumerate(theta):
        assert (int(tex[i]), bool(left[i]), bool(ties[i])) == _circle_literal(n, th, rotate, invert), (i, th)


@pytest.mark.parametrize("n,W,seed", CASES)
def test_contract_formula_equals_the_shader_evaluation(n, W, seed):
    """smooth_audio_adj's shader text with _PRE_SMOOTHED_AUDIO 1 (the committed vectors; regenerated where the reference tree exists) against the
    contract formula on the helper's table, bit for bit.  Columns with a tie or a `beyond` entry are left out (NaN in the vectors): they may not
    exceed the columns at idx >= half_w -- one per table for an even width, two for an odd one (idx = half_w and half_w + 1)."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "column_vectors.npz"))[f"graph_n{n}_w{W}_s{seed}"]
    import glsl_eval
    if os.path.exists(os.path.join(glsl_eval.SHADER_ROOT, "util", "smooth.glsl")):
        from make_column_golden import evaluate
        assert (evaluate(n, W, seed).view(np.uint32) == gold.view(np.uint32)).all()
    tex, ties, beyond = graph_column_texels(n, W)
    left_out = ties.any(axis=1) | beyond.any(axis=1)
    print(f"n={n} W={W}: {int(left_out.sum())} of {len(tex)} columns left out")
    assert left_out.sum() <= len(tex) - W // 2
    assert (np.isnan(gold) == left_out).all()
    want = contract(texel_floats(texel_row(n, seed)), tex)
    assert (gold[~left_out].view(np.uint32) == want[~left_out].view(np.uint32)).all()


@pytest.fixture(scope="module")
def colsemu(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "emu", "cols_emu.cpp")
    so = str(tmp_path_factory.mktemp("colsemu") / "libcolsemu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src], check=True)
    L = C.CDLL(so)
    L.colsemu_columns.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p]
    L.colsemu_columns.restype = C.c_int
    L.colsemu_mean.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    return L


def test_column_mean_is_the_contract_formula(colsemu):
    rng = np.random.default_rng(5)
    c = rng.integers(0, 65536, size=(3, 200000), dtype=np.uint16)
    c[:, :6] = np.array([[0, 65535, 65535, 1, 0, 2], [0, 65535, 0, 1, 1, 2], [0, 65535, 65535, 1, 0, 3]], np.uint16)
    out = np.zeros(c.shape[1], F)
    colsemu.colsemu_mean(c[0].ctypes.data, c[1].ctypes.data, c[2].ctypes.data, c.shape[1], out.ctypes.data)
    T = texel_floats(np.arange(65536, dtype=np.uint32))
    want = contract(T, c.T.astype(np.int64))
    assert (out.view(np.uint32) == want.view(np.uint32)).all()


# (n, W, lanes per row, work-list batch): fused configurations -- N = 1024 E=8, 4096 E=16 and E=8, 16384 E=32 -- and lanes 0 = the second launch
@pytest.mark.parametrize("n,W,lanes,batch", [(1024, 200, 64, 2), (1024, 320, 0, 0), (4096, 320, 128, 2), (4096, 800, 256, 2), (4096, 800, 0, 0),
                                             (4096, 1920, 0, 0), (16384, 800, 256, 6), (16384, 1920, 0, 0)])
@pytest.mark.parametrize("sf", [0.025, 0.01])
def test_emulated_columns_equal_twin_texels_through_the_contract(colsemu, oracle, n, W, lanes, batch, sf):
    rng = np.random.default_rng(n + W + int(sf * 1000))
    rows = rng.integers(0, 65536, size=(3, n), dtype=np.uint16)
    rows[1, : n // 4] = 65535                                               # the largest sums
    rows[2] = (rng.random(n) < 0.5) * rng.integers(0, 65536, size=n)
    table = np.ascontiguousarray(graph_column_texels(n, W)[0], np.uint32)
    out = np.zeros((rows.shape[0], len(table)), F)
    rc = colsemu.colsemu_columns(rows.ctypes.data, rows.shape[0], n, table.ctypes.data, len(table), C.c_float(sf), lanes, batch, out.ctypes.data)
    assert rc == 0, rc
    for r in range(rows.shape[0]):
        t, _ = oracle.bars_int(rows[r], n, smooth_factor=sf, phase=0.5)
        want = contract(texel_floats(t), table.astype(np.int64))
        assert (out[r].view(np.uint32) == want.view(np.uint32)).all(), r


def test_distinct_texels_that_do_not_fit_are_refused_by_the_emulated_epilogue(colsemu):
    n, W = 4096, 800
    table = np.ascontiguousarray(graph_column_texels(n, W)[0], np.uint32)     # 801 distinct texels + the dump slot > 4 * 128
    rows = np.zeros((1, n), np.uint16); out = np.zeros((1, len(table)), F)
    assert colsemu.colsemu_columns(rows.ctypes.data, 1, n, table.ctypes.data, len(table), C.c_float(0.025), 128, 2, out.ctypes.data) == -2
