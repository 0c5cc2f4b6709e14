"""CPU: glv_params.gl_storage = 3 -- the CPU operators on float state, then the GL_R16 upload of the finished buffer (`setaccelfft false`).

What a host without a device can pin: the value is accepted by validation (creation then fails for the missing device, not for the value), 4 is still
refused, and the reference composition the GPU tests hold the library to is well defined on the CPU: the oracle's float chain -> Oracle.texels_r16 ->
Oracle.bars_int(bars = n, phase 0.5), which must be the same thing as that composition fed with the compiled reference's committed chain outputs."""
import ctypes as C

import numpy as np
import pytest

from oracle_lib import Oracle, StreamOracle, lcg_pcm_fast

GL_STORAGE_UPLOAD = 3


def _create(G, **kw):
    h = C.c_void_p(None)
    cp = G.Params(**kw).c()
    mask = G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS
    rc = G.lib().glv_batch_create(C.byref(cp), 2, mask, 0, C.byref(h))
    if rc == G.OK:
        G.lib().glv_batch_destroy(h)
    return rc


def test_gl_storage_3_passes_validation_and_4_does_not(glvlib):
    G = glvlib
    assert G.GL_STORAGE_UPLOAD == GL_STORAGE_UPLOAD
    # validation runs before the device is looked for: without one an accepted value ends in GLV_ERR_NO_DEVICE, a refused one in GLV_ERR_INVALID
    want_ok = G.OK if G.device_count() > 0 else G.ERR_NO_DEVICE
    assert _create(G, n=1024, bars=1024, bar_phase=0.5, gl_storage=3) == want_ok
    assert _create(G, n=1024, bars=1024, bar_phase=0.5, gl_storage=0) == want_ok
    assert _create(G, n=1024, bars=1024, bar_phase=0.5, gl_storage=4) == G.ERR_INVALID
    assert "gl_storage=4" in G.lib().glv_last_error().decode()
    assert _create(G, n=1024, gl_storage=0xffffffff) == G.ERR_INVALID
    assert G.lib().glv_abi_version() == 7


@pytest.mark.parametrize("tag,F,win", [("F5w", 5, True), ("F6u", 6, False), ("F1w", 1, True)])
def test_reference_composition_is_defined_on_the_cpu(oracle, golden, tag, F, win):
    """float chain -> upload texels -> pre-smoothing pass, N = 1024, 9 updates: from the oracle's chain and from the committed reference outputs"""
    n = 1024
    so = StreamOracle(n, avg_frames=F, avg_window=win)
    want_rows = golden[f"chain_n1024_{tag}"]
    for fr in range(9):
        rows = so.frame(lcg_pcm_fast(500 + fr, 2 * n))
        U = Oracle.texels_r16(rows)
        U_ref = Oracle.texels_r16(want_rows[fr])
        assert U.dtype == np.uint16 and U.shape == (2, n)
        assert (U == U_ref).all(), fr
        for c in range(2):
            t, f = Oracle.bars_int(U[c], n, 0.025, 0.5)
            t_ref, f_ref = Oracle.bars_int(U_ref[c], n, 0.025, 0.5)
            assert (t == t_ref).all() and (f.view(np.uint32) == f_ref.view(np.uint32)).all(), (fr, c)
            # the pass is a weighted mean of texels: its texels stay inside the row's range; its floats are the unrounded means / 65535, so they lie
            # within half a texel of the texels (+ the float rounding of a value <= 1: 2^-24 * 65535 < 0.004 texels)
            assert t.min() >= U[c].min() and t.max() <= U[c].max()
            assert (np.abs(f.astype(np.float64) * 65535 - t) <= 0.5 + 0.004).all()
