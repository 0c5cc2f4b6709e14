"""CPU: bars at texels of the pre-smoothing pass (glv_batch_set_bar_texels) -- the exported symbol, the modules' position
helpers against a literal float32 restatement of their shaders, and a host walk of the fused epilogue's integer sums
(tests/emu/snap_emu.cpp, built here) against the oracle's exact integer mean of the twin (bars = n, phase 0.5)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from glava_amd.bar_positions import bars_module_bar_texels, radial_bar_texels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_set_bar_texels_is_exported():
    so = os.path.join(ROOT, "glava_amd", "csrc", "libglvspectrum.so")
    if not os.path.exists(so):
        from glava_amd import build as B
        B.build(tune=False, verbose=False)
    L = C.CDLL(so)
    assert hasattr(L, "glv_batch_set_bar_texels")
    hdr = open(os.path.join(ROOT, "include", "glv_spectrum.h")).read()
    assert "int glv_batch_set_bar_texels(glv_batch* b, const uint32_t* texels, uint32_t count);" in hdr


def _glsl_round(x):
    """Mesa's round(): half to even; plus whether x sat exactly on a half"""
    x = F(x)
    return int(np.rint(x)), bool(x - np.floor(x) == F(0.5))


def _radial_literal(n, nbars):
    """radial/1.frag:57-70 at the centre angle of every bar of one channel (ROTATE 0, INVERT 0)"""
    TWOPI, PI = F(6.28318530718), F(3.14159265359)
    section = F(TWOPI / F(nbars))
    out, ties = [], []
    for k in range(nbars // 2):
        theta = F(F(F(k) + F(0.5)) * section)
        idx = F(theta + F(0.0))
        dir_ = F(np.fmod(abs(idx), TWOPI))
        if dir_ > PI:
            idx = F(-np.sign(idx) * F(TWOPI - dir_))
        idx = F(-idx)
        pos = F(F(int(F(abs(idx) / section))) / F(nbars // 2))
        t, tie = _glsl_round(F(pos * F(n)))
        out.append(t); ties.append(tie)
    return np.array(out, np.uint32), np.array(ties)


def _bars_literal(n, W, bar_width, bar_gap, channels):
    """bars/1.frag:51-90 pixel by pixel (DIRECTION 0, FLIP 0, INVERT 0): the texel of every drawn p > 0, in order of first appearance"""
    W = F(W)
    section = F(F(bar_width) + F(bar_gap))
    center = F(section / F(2.0))
    nbars = F(np.floor(F(W * F(0.5)) / section) * F(2))
    seen, out, ties = set(), [], []
    for x in range(int(W)):
        ax = F(F(x) + F(0.5))                                                     # gl_FragCoord.x
        dx = F(ax - F(W / F(2))) if channels == 2 else ax
        m = F(abs(F(np.fmod(dx, section)) if dx >= 0 else F(dx - section * np.floor(dx / section))))
        md = F(m - center)
        if not (md < np.ceil(F(bar_width) / F(2)) and md >= -np.floor(F(bar_width) / F(2))):
            continue
        s = F(dx / section)
        p = F(np.ceil(s)) if np.sign(s) == 1.0 else F(np.floor(s))
        p = F(p / F(nbars / F(2))) if channels == 2 else F(p / nbars)
        p = F(p + F(np.sign(p)) * F(F(F(0.5) + center) / W))
        if p > F(1.0) or p <= F(0.0):
            continue
        t, tie = _glsl_round(F(p * F(n)))
        if p not in seen:
            seen.add(p); out.append(t); ties.append(tie)
    return np.array(out, np.uint32), np.array(ties)


@pytest.mark.parametrize("n", [1024, 4096, 16384])
def test_radial_positions(n):
    t, ties = radial_bar_texels(n, 160)
    lt, lties = _radial_literal(n, 160)
    assert t.dtype == np.uint32 and len(t) == 80
    assert (t == lt).all() and (ties == lties).all()
    assert not ties.any()                     # k n / 80 never ends in .5 for a power-of-two n
    assert t[0] == 0 and (np.diff(t.astype(np.int64)) > 0).all() and t[-1] < n


@pytest.mark.parametrize("n", [1024, 4096, 16384])
@pytest.mark.parametrize("W,bw,gap,ch", [(1280, 5, 1, 2), (801, 4, 2, 2), (1000, 5, 1, 1)])
def test_bars_module_positions(n, W, bw, gap, ch):
    t, ties = bars_module_bar_texels(n, W, bw, gap, ch)
    lt, lties = _bars_literal(n, W, bw, gap, ch)
    assert len(t) > 10
    assert (t == lt).all() and (ties == lties).all()
    assert (t < n).all()


@pytest.fixture(scope="module")
def snapemu(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "emu", "snap_emu.cpp")
    so = str(tmp_path_factory.mktemp("snapemu") / "libsnapemu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src], check=True)
    L = C.CDLL(so)
    L.snapemu_bars.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
    L.snapemu_bars.restype = C.c_int
    L.snapemu_texel_roundtrip_failures.restype = C.c_int
    return L


def test_texels_survive_the_float_row(snapemu):
    assert snapemu.snapemu_texel_roundtrip_failures() == 0


def _emu(L, rows, n, tex, sf, lanes, batch, r16):
    rows = np.ascontiguousarray(rows, np.uint16)
    tex = np.ascontiguousarray(tex, np.uint32)
    out = np.zeros((rows.shape[0], len(tex)), np.uint16 if r16 else np.float32)
    rc = L.snapemu_bars(rows.ctypes.data, rows.shape[0], n, tex.ctypes.data, len(tex), C.c_float(sf), lanes, batch, int(r16), out.ctypes.data)
    assert rc == 0
    return out


# (n, lanes per row, work-list batch) of the fused configurations: N = 1024 E=8, 4096 E=16 and E=8, 16384 E=32
@pytest.mark.parametrize("n,lanes,batch", [(1024, 64, 2), (4096, 128, 2), (4096, 256, 2), (16384, 256, 6)])
@pytest.mark.parametrize("sf", [0.025, 0.01, 0.06])
def test_emulated_epilogue_equals_twin_integer_mean(snapemu, oracle, n, lanes, batch, sf):
    rng = np.random.default_rng(n + int(sf * 1000))
    rows = rng.integers(0, 65536, size=(3, n), dtype=np.uint16)
    rows[1, : n // 4] = 65535                                               # the largest sums
    rows[2] = (rng.random(n) < 0.5) * rng.integers(0, 65536, size=n)
    tex = np.concatenate([radial_bar_texels(n, 160)[0], np.array([n - 1, n // 2 + 1], np.uint32)])
    if len(tex) + 1 > 2 * lanes:
        tex = tex[: 2 * lanes - 1]
    got16 = _emu(snapemu, rows, n, tex, sf, lanes, batch, True)
    gotf = _emu(snapemu, rows, n, tex, sf, lanes, batch, False)
    for r in range(rows.shape[0]):
        t, f = oracle.bars_int(rows[r], n, smooth_factor=sf, phase=0.5)
        assert (got16[r] == t[tex]).all(), r
        assert (gotf[r].view(np.uint32) == f[tex].astype(np.float32).view(np.uint32)).all(), r
