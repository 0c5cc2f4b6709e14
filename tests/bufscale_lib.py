"""What the bufscale tests share (test_bufscale_host.py, test_bufscale.py, test_track_bufscale.py): a plain module, like oracle_lib.py and track_lib.py.

np_bufscale restates `setbufscale k` over the backend's unpack in numpy float32 -- one rounded operation per step, in the reference's order -- and
tests/test_bufscale_host.py holds it bit for bit to the oracle's glvo_bufscale, which tests/test_handle_audio.py pins to the reference's real rd_update."""
import numpy as np

F32 = np.float32
KS = (2, 3, 4, 8, 16)


def np_unpack(x, f32, channels):
    """the backend's unpack of interleaved frames x [..., frames, 2] -> (l, r) float32 [..., frames].  s16: v / 65535.0F, channels == 1: ((l + r) / 2) / 65535.0F
    with C's truncating integer division (fifo.c:94-110); f32: the samples, channels == 1: (l + r) / 2.0F (pulse_input.c:167)"""
    x = np.asarray(x)
    if f32:
        assert x.dtype == np.float32
        l, r = x[..., 0], x[..., 1]
        if channels == 1:
            with np.errstate(all="ignore"):
                m = ((l + r).astype(F32) / F32(2.0)).astype(F32)
            return m, m
        return l.copy(), r.copy()
    assert x.dtype == np.int16
    v = x.astype(np.int32)
    if channels == 1:
        s = v[..., 0] + v[..., 1]
        m = np.where(s < 0, -((-s) // 2), s // 2)                              # C: truncation toward zero
        f = (m.astype(F32) / F32(65535.0)).astype(F32)
        return f, f
    return (v[..., 0].astype(F32) / F32(65535.0)).astype(F32), (v[..., 1].astype(F32) / F32(65535.0)).astype(F32)


def np_decimate(rows, k):
    """rows float32 [..., k * n] -> [..., n]: acc = 0.0F; acc = acc + x[t k + a] for a = 0 .. k - 1 in order; acc / (float) k (render.c:1768-1781)"""
    rows = np.asarray(rows, dtype=F32)
    r = rows.reshape(*rows.shape[:-1], rows.shape[-1] // k, k)
    acc = np.zeros(r.shape[:-1], F32)
    with np.errstate(all="ignore"):
        for a in range(k):
            acc = (acc + r[..., a]).astype(F32)
        return (acc / F32(k)).astype(F32)


def np_bufscale(x, k, f32, channels):
    """interleaved windows x [streams][k * n][2] (int16, or float32 with f32) -> the planar rows the chain transforms, float32 [streams][2][n]"""
    l, r = np_unpack(x, f32, channels)
    return np.ascontiguousarray(np.stack([np_decimate(l, k), np_decimate(r, k)], axis=-2))


def np_bufscale_planar(x, k):
    """planar rows x float32 [streams][2][k * n] (lb / rb as rd_update finds them: no mix) -> float32 [streams][2][n]"""
    return np.ascontiguousarray(np_decimate(x, k))


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def oracle_bufscale(Oracle, x, k, f32, channels):
    """the same through the oracle: glvo_unpack_s16 / _f32 per stream, glvo_bufscale per row"""
    x = np.ascontiguousarray(x)
    streams, frames = x.shape[0], x.shape[1]
    n = frames // k
    out = np.empty((streams, 2, n), F32)
    L = Oracle.lib()
    for s in range(streams):
        l, r = np.empty(frames, F32), np.empty(frames, F32)
        (L.glvo_unpack_f32 if f32 else L.glvo_unpack_s16)(np.ascontiguousarray(x[s]).reshape(-1), frames, channels, l, r)
        for c, row in enumerate((l, r)):
            dec = np.empty(n, F32)
            L.glvo_bufscale(row, dec, n, k)
            out[s, c] = dec
    return out


# left to right ((0 + 1e8) + 1) + -1e8) + 1 = 1 -> 0.25; pairwise (1e8 + 1) + (-1e8 + 1) = 0; reversed ((1 + -1e8) + 1) + 1e8 = 0
ORDER_CASE = np.array([1.0e8, 1.0, -1.0e8, 1.0], F32)
