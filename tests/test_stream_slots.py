"""GPU: stream slots -- glv_batch_reset_streams / _save_streams / _load_streams, the lifecycle of chosen streams of a batch.

Contract (include/glv_spectrum.h): after a reset the listed streams are streams of a batch glv_batch_reset has just cleared; after save(A, i) and
load(B, j) stream j of B continues exactly as stream i of A would have, whatever head / ring positions the two batches are at; every other stream is
untouched.  Every assertion is bit equality (floats as uint32), in output and in state.  The reference is the library's own undisturbed path, which the
oracle suites hold to the reference: a fresh batch fed the same windows, or a twin batch that was never touched.

n = 256 and 7 streams unless a case needs more: an odd count; a stream's gravity rows are fewer 16-byte pieces than a workgroup takes per trip (128 on float
state, 64 on texels), its average ring more (640 / 320 at F = 5).  Blobs are indexed through glava_amd/stream_slots.py, the layout's numpy restatement."""
import ctypes as C

import numpy as np
import pytest

from glava_amd import stream_slots as SL
from track_lib import bars_batch, pcm, to_device, track

pytestmark = pytest.mark.gpu

N, S = 256, 7
FILL = 0xA5
GUARD = 4096


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------------------
def _chains(G):
    """name -> (parameters, creation mask, ops): the stateful chains the issue names"""
    g, a = G.OP_GRAVITY, G.OP_AVERAGE
    return {
        "gravity":  (dict(), g, G.OP_FFT | g),                                                           # form 1
        "chain_F1": (dict(avg_frames=1), g | a, G.OP_FFT | g | a),                                       # form 2
        "chain_F5": (dict(avg_frames=5), g | a, G.OP_FFT | g | a),
        "average":  (dict(avg_frames=5), a, G.OP_FFT | a),
        "gl_chain": (dict(avg_frames=5, gl_storage=1, avg_window_kind=1), g | a, G.OP_FFT | g | a | G.OP_R16),   # uint16 state
        "upload":   (dict(avg_frames=5, gl_storage=3), g | a, G.OP_FFT | g | a),
    }


CHAINS = ["gravity", "chain_F1", "chain_F5", "average", "gl_chain", "upload"]


def _make(G, chain, n=N, streams=S, extra_mask=0, **over):
    kw, mask, ops = _chains(G)[chain]
    p = G.Params(n=n, **{**kw, **over})
    return G.Batch(p, streams, mask | extra_mask), ops, p.avg_frames


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return _bits(a).shape == _bits(b).shape and bool((_bits(a) == _bits(b)).all())


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _idx(values):
    """uint32 [count] on the device (torch keeps them as int32 bits)"""
    return _dev(np.array(values, dtype=np.uint32).view(np.int32))


def _update(G, b, x, ops, w=None, method="process_s16", extra=()):
    """one update of every stream from x (host) -> the output on the host, [streams][2][w]"""
    import torch
    w = w or b.params.n
    o = torch.zeros((b.streams * 2, w), dtype=torch.int16 if ops & G.OP_R16 else torch.float32, device="cuda")
    getattr(b, method)(_dev(x), *extra, o, ops)
    torch.cuda.synchronize()
    return o.cpu().numpy().reshape(b.streams, 2, w)


def _windows(seed, count, streams=S, n=N):
    """`count` updates' inputs, int16 [streams][n][2] each, every stream at a level of its own"""
    return [pcm(seed + 31 * u, streams, n) for u in range(count)]


def _save(b, streams, guard=False, fill=FILL):
    """save_streams of the listed streams -> (desc, blobs uint8 [count][bytes] on the host); guard: bands before and behind the blob must come back intact"""
    import torch
    nbytes = int(b.stream_state_desc().bytes)
    count = len(streams)
    buf = torch.full((GUARD + count * nbytes + GUARD,), fill, dtype=torch.uint8, device="cuda")
    blob = buf[GUARD:GUARD + count * nbytes]
    assert blob.data_ptr() % 16 == 0
    d = b.save_streams(_idx(streams), count, blob)
    torch.cuda.synchronize()
    assert b.last_launches() == 1 and b.kernel_name() == "glv_slots_kernel"
    assert int(d.bytes) == nbytes == SL.stream_bytes(d)
    if guard:
        assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + count * nbytes:] == fill).all()), "a save wrote outside its blobs"
    return d, blob.cpu().numpy().reshape(count, nbytes)


def _save_all(b):
    return _save(b, list(range(b.streams)))


def _load(b, streams, blobs, desc):
    import torch
    d_blob = _dev(np.ascontiguousarray(blobs).reshape(-1))
    assert d_blob.data_ptr() % 16 == 0
    b.load_streams(_idx(streams), len(streams), d_blob, desc)
    torch.cuda.synchronize()
    assert b.last_launches() == 1 and b.kernel_name() == "glv_slots_kernel"


def _reset(b, streams, stream=None):
    import torch
    b.reset_streams(_idx(streams), len(streams), stream=stream)
    torch.cuda.synchronize()
    assert b.last_launches() == 1 and b.kernel_name() == "glv_slots_kernel"


def _download(G, address, count, dtype):
    out = np.empty(count, dtype)
    assert G.lib().glv_device_download(0, out.ctypes.data_as(C.c_void_p), C.c_void_p(address), C.c_size_t(out.nbytes), None) == 0
    assert G.lib().glv_device_sync(0, None) == 0
    return out


def _close(*batches):
    for b in batches: b.close()


def _mixed(own, src, pairs):
    """a batch's inputs with slot dst fed what stream s of another batch gets: pairs (s, dst)"""
    out = []
    for x, y in zip(own, src):
        z = np.array(x, copy=True)
        for s, dst in pairs: z[dst] = y[s]
        out.append(z)
    return out


# ---- reset --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", CHAINS)
def test_reset_streams_makes_fresh_streams_and_touches_no_other(glvlib, chain):
    """F + 2 updates (head != 0), reset {0, 3, 6}, F + 3 further updates: the three equal a fresh batch fed the same windows, the other four a twin that
    was never touched -- outputs and, at the end, state (a save of all streams; the gravity chain also through glv_batch_gravity_state)"""
    G = glvlib
    b, ops, F = _make(G, chain)
    twin, fresh = _make(G, chain)[0], _make(G, chain)[0]
    listed, others = [0, 3, 6], [1, 2, 4, 5]
    xs = _windows(100, 2 * F + 5)
    for x in xs[:F + 2]:
        assert _same(_update(G, b, x, ops), _update(G, twin, x, ops))
    before = b.stream_state_desc()
    _reset(b, listed)
    after = b.stream_state_desc()
    assert (after.gravity_form, after.kept_bins, after.regions, after.bytes) == (before.gravity_form, before.kept_bins, before.regions, before.bytes)
    for u, x in enumerate(xs[F + 2:]):
        got, kept, new = _update(G, b, x, ops), _update(G, twin, x, ops), _update(G, fresh, x, ops)
        assert _same(got[listed], new[listed]), (chain, u, "reset streams")
        assert _same(got[others], kept[others]), (chain, u, "other streams")
        assert bool((got != 0).any())
    (d, sb), (_, st), (_, sf) = _save_all(b), _save_all(twin), _save_all(fresh)
    assert _same(sb[listed], sf[listed]) and _same(sb[others], st[others]), chain
    assert (d.n, d.avg_frames, d.elem_bytes) == (N, F, 2 if chain == "gl_chain" else 4)
    if chain == "gravity":
        gb, gf, gt = (_download(G, x.gravity_state(), S * 2 * N, np.float32).reshape(S, 2 * N) for x in (b, fresh, twin))
        assert _same(gb[listed], gf[listed]) and _same(gb[others], gt[others])
    _close(b, twin, fresh)


@pytest.mark.parametrize("chain", ["chain_F5", "gl_chain"])
def test_reset_and_save_with_a_duplicate_and_an_entry_past_the_batch(glvlib, chain):
    """a table holding a duplicate and entries >= streams: the reset clears the listed streams and writes nothing else (a batch-wide save before and after
    differs only in them); the save leaves the blobs of the skipped entries and the guard bands as they were"""
    G = glvlib
    b, ops, F = _make(G, chain)
    for x in _windows(200, F + 2): _update(G, b, x, ops)
    table = [3, 3, S + 5, 0xFFFFFFFF, 6, S]
    d0, before = _save_all(b)
    d, blobs = _save(b, table, guard=True)
    for j, s in enumerate(table):
        if s < S: assert _same(blobs[j], before[s]), (j, s)
        else: assert bool((blobs[j] == FILL).all()), (j, s, "the blob of a skipped entry was written")
    _reset(b, table)
    _, after = _save_all(b)
    assert bool((after[[3, 6]] == 0).all()) and bool((before[[3, 6]] != 0).any())
    assert _same(after[[0, 1, 2, 4, 5]], before[[0, 1, 2, 4, 5]])
    # ... and a load from such a table: the listed streams come back, the skipped entries' blobs are not read into anything
    import torch
    b.load_streams(_idx([3, S + 5, 6]), 3, _dev(np.concatenate([before[3], np.full_like(before[3], 0x5A), before[6]])), d)
    torch.cuda.synchronize()
    assert _same(_save_all(b)[1], before)
    _close(b)


# ---- save and load ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", CHAINS)
def test_save_then_load_continues_the_stream_in_another_batch(glvlib, chain):
    """batch A after 7 updates, batch B after 2 (heads differ): A's {1, 4} into B's {5, 0}; B's two slots fed what A's two streams get for F + 3 updates give
    A's outputs and leave A's state; B's other streams equal B's twin"""
    G = glvlib
    a, ops, F = _make(G, chain)
    b, twin = _make(G, chain)[0], _make(G, chain)[0]
    pairs, others = [(1, 5), (4, 0)], [1, 2, 3, 4, 6]
    xa, xb = _windows(300, 7 + F + 3), _windows(5000, 2 + F + 3)
    for x in xa[:7]: _update(G, a, x, ops)
    for x in xb[:2]: assert _same(_update(G, b, x, ops), _update(G, twin, x, ops))
    d, blobs = _save(a, [s for s, _ in pairs], guard=True)
    assert d.gravity_form == {"gravity": 1, "average": 0}.get(chain, 2) and d.kept_bins == N
    _load(b, [dst for _, dst in pairs], blobs, d)
    for u, (x, y) in enumerate(zip(xa[7:], _mixed(xb[2:], xa[7:], pairs))):
        oa, ob, ot = _update(G, a, x, ops), _update(G, b, y, ops), _update(G, twin, y, ops)
        for s, dst in pairs: assert _same(ob[dst], oa[s]), (chain, u, s, dst)
        assert _same(ob[others], ot[others]), (chain, u, "other streams")
    (_, sa), (_, sb), (_, st) = _save_all(a), _save_all(b), _save_all(twin)
    for s, dst in pairs: assert _same(sb[dst], sa[s]), (chain, s, dst, "state")
    assert _same(sb[others], st[others])
    _close(a, b, twin)


@pytest.mark.parametrize("chain", CHAINS)
def test_checkpoint_and_resume_in_the_same_batch(glvlib, chain):
    """save {2} at step t, 3 updates, load {2} (the head has moved by 3), the same 3 updates again: the same 3 outputs -- the checkpoint a seek needs"""
    G = glvlib
    b, ops, F = _make(G, chain)
    xs = _windows(400, F + 2 + 3)
    for x in xs[:F + 2]: _update(G, b, x, ops)
    d, blob = _save(b, [2])
    first = [_update(G, b, x, ops)[2] for x in xs[F + 2:]]
    _, later = _save(b, [2])
    _load(b, [2], blob, d)
    assert _same(_save(b, [2])[1], blob)
    again = [_update(G, b, x, ops)[2] for x in xs[F + 2:]]
    for u in range(3): assert _same(first[u], again[u]), (chain, u)
    assert _same(_save(b, [2])[1], later)
    _close(b)


@pytest.mark.parametrize("chain", ["chain_F5", "gl_chain"])
def test_checkpoint_and_resume_under_track_at(glvlib, chain):
    """the same through glv_batch_track_at_s16, the steps cut at the checkpoint: [0, 7) in one call, save {2}, [7, 10), load {2}, [7, 10) again"""
    import torch
    G = glvlib
    b, ops, F = _make(G, chain)
    steps, cut = 10, 7
    starts = [(45 * t) % 301 for t in range(steps)]
    pitch = N + 301 + 39
    x = pcm(77, S, pitch)
    d_pcm, table = to_device(x, False, False), _idx(starts)
    dt = torch.int16 if ops & G.OP_R16 else torch.float32
    track(b, "at", d_pcm, pitch, table, cut, ops, N, dt)
    d, blob = _save(b, [2])
    first = track(b, "at", d_pcm, pitch, table, steps - cut, ops, N, dt, t0=cut).cpu().numpy().reshape(steps - cut, S, 2, N)
    _load(b, [2], blob, d)
    again = track(b, "at", d_pcm, pitch, table, steps - cut, ops, N, dt, t0=cut).cpu().numpy().reshape(steps - cut, S, 2, N)
    assert _same(first[:, 2], again[:, 2]) and bool((first[:, 2] != 0).any())
    # ... and they are what the sequential calls write
    seq, _, _ = _make(G, chain)
    for t in range(steps):
        o = _update(G, seq, x[:, starts[t]:starts[t] + N], ops)
        if t >= cut: assert _same(o, first[t - cut]), (chain, t)
    _close(b, seq)


# ---- blob layout --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", ["average", "chain_F5", "gl_chain"])
def test_blob_rows_are_the_ring_oldest_first(glvlib, chain):
    """after F + 3 updates blob row q of the average ring is what the update F - q calls ago stored: the transform's row (average alone), gravity's output
    (fused with average; uint16 texels on the GL chain) -- read from a twin batch that runs the chain up to the ring"""
    G = glvlib
    b, ops, F = _make(G, chain)
    if chain == "average": upto, uops = G.Batch(G.Params(n=N), S, G.OP_FFT), G.OP_FFT
    elif chain == "chain_F5": upto, uops = G.Batch(G.Params(n=N), S, G.OP_GRAVITY), G.OP_FFT | G.OP_GRAVITY
    else: upto, uops = G.Batch(G.Params(n=N, gl_storage=1), S, G.OP_GRAVITY), G.OP_FFT | G.OP_GRAVITY | G.OP_R16
    xs = _windows(600, F + 3)
    stored = []
    for x in xs:
        _update(G, b, x, ops)
        stored.append(_update(G, upto, x, uops))
    d, blobs = _save_all(b)
    for s in range(S):
        ring = SL.split_blob(d, blobs[s])["average"]
        for q in range(F):
            want = stored[len(xs) - F + q][s]
            assert _same(ring[:, q, :], want.view(ring.dtype)), (chain, s, q)
    _close(b, upto)


def test_blob_gravity_rows_are_the_gravity_state(glvlib):
    G = glvlib
    b, ops, _ = _make(G, "gravity")
    for x in _windows(650, 3): _update(G, b, x, ops)
    d, blobs = _save_all(b)
    state = _download(G, b.gravity_state(), S * 2 * N, np.float32).reshape(S, 2, N)
    for s in range(S): assert _same(SL.split_blob(d, blobs[s])["gravity"], state[s])
    assert d.regions == SL.REGION_GRAVITY and SL.region_offsets(d) == {"gravity": (0, 2 * N * 4)}
    _close(b)


# ---- rings --------------------------------------------------------------------------------------------------------------------------------------------
def _ring_frames(seed, frames, f32):
    x = pcm(seed, S, frames)
    return (x.astype(np.float32) / np.float32(32768)) if f32 else x


def _ring_batch(G, f32):
    if f32: return G.Batch(G.Params(n=N, avg_frames=3), S, G.OP_GRAVITY | G.OP_AVERAGE | G.OP_RING_F32), G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE
    return G.Batch(G.Params(n=N), S, G.OP_GRAVITY | G.OP_RING_S16), G.OP_FFT | G.OP_GRAVITY


def _ring_planar(b, f32):
    import torch
    o = torch.zeros((S, 2, N), dtype=torch.float32, device="cuda")
    b.ring_planar(o, f32)
    torch.cuda.synchronize()
    return o.cpu().numpy()


@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
@pytest.mark.parametrize("app_a,app_b", [((100, 37), (37,)), ((100,), (100, 100)), ((100, 37), (100, 100, 56)), ((255,), (37,))],
                         ids=["odd_odd", "aligned", "odd_to_zero", "last_frame"])
def test_rings_save_load_and_reset(glvlib, f32, app_a, app_b):
    """ring batches whose write positions differ (137 / 37: both odd, a 16-byte piece of the blob straddles the wrap of either ring; 100 / 200: whole pieces;
    137 / 0; 255 / 37): A's {1, 4} into B's {5, 0}, then reset {2, 6} of B -- checked by glv_batch_ring_planar and the next ring updates' outputs"""
    G = glvlib
    kind = "f32" if f32 else "s16"
    (a, ops), (b, _), (twin, _), (fresh, _) = (_ring_batch(G, f32) for _ in range(4))
    pairs, others = [(1, 5), (4, 0)], [1, 2, 3, 4, 6]
    for k, frames in enumerate(app_a): _update(G, a, _ring_frames(700 + k, frames, f32), ops, method=f"ring_update_{kind}", extra=(frames,))
    for k, frames in enumerate(app_b):
        x = _ring_frames(750 + k, frames, f32)
        _update(G, b, x, ops, method=f"ring_update_{kind}", extra=(frames,)); _update(G, twin, x, ops, method=f"ring_update_{kind}", extra=(frames,))
    d, blobs = _save(a, [1, 4], guard=True)
    assert d.regions == (SL.REGION_GRAVITY | SL.REGION_AVERAGE | SL.REGION_RING_F32 if f32 else SL.REGION_GRAVITY | SL.REGION_RING_S16)
    pa = _ring_planar(a, f32)
    name = "ring_f32" if f32 else "ring_s16"
    for j, s in enumerate([1, 4]):      # the blob's ring is the window oldest frame first: what the planar snapshot unpacks
        ring = SL.split_blob(d, blobs[j])[name]
        want = ring.astype(np.float32) if f32 else (ring.astype(np.float32) / np.float32(65535))      # fifo.c:94-110 / pulse_input.c:167, stereo
        assert _same(pa[s], np.ascontiguousarray(want.T)), (s, "blob ring")
    _load(b, [5, 0], blobs, d)
    pb, pt = _ring_planar(b, f32), _ring_planar(twin, f32)
    for s, dst in pairs: assert _same(pb[dst], pa[s]), (s, dst, "planar")
    assert _same(pb[others], pt[others])
    for u, frames in enumerate((64, 23, 256)):
        x, y = _ring_frames(800 + u, frames, f32), _ring_frames(850 + u, frames, f32)
        z = _mixed([y], [x], pairs)[0]
        oa = _update(G, a, x, ops, method=f"ring_update_{kind}", extra=(frames,))
        ob = _update(G, b, z, ops, method=f"ring_update_{kind}", extra=(frames,))
        ot = _update(G, twin, z, ops, method=f"ring_update_{kind}", extra=(frames,))
        for s, dst in pairs: assert _same(ob[dst], oa[s]), (u, s, dst)
        assert _same(ob[others], ot[others]), u
        if u == 0:      # reset two of B's streams between updates: from here they are a fresh batch's, which gets the same frames
            _reset(b, [2, 6])
            pr = _ring_planar(b, f32)
            assert bool((pr[[2, 6]] == 0).all()) and _same(pr[[1, 3, 4]], _ring_planar(twin, f32)[[1, 3, 4]]) and _same(pr[[5, 0]], _ring_planar(a, f32)[[1, 4]])
            others = [1, 3, 4]
        else:
            of = _update(G, fresh, z, ops, method=f"ring_update_{kind}", extra=(frames,))
            assert _same(ob[[2, 6]], of[[2, 6]]), (u, "reset streams")
            assert _same(_ring_planar(b, f32)[[2, 6]], _ring_planar(fresh, f32)[[2, 6]])
    _close(a, b, twin, fresh)


# ---- live classes -------------------------------------------------------------------------------------------------------------------------------------
FR = 5


def _live_case(G, case):
    """the float_80 and gl_smallest cases of tests/test_track_live.py: (n, parameters, ops), the first candidate size with live bins"""
    chain = G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS
    if case == "float_80": return 1024, dict(bars=80), chain
    for n in (256, 512, 1024, 2048, 4096):
        kw = dict(bars=n, bar_phase=0.5, smooth_factor=0.025, avg_window_kind=1, gl_storage=1)
        probe = bars_batch(G, n, kw, None, FR, 1)
        L = probe.live_bins(); probe.close()
        if L != 0: return n, kw, chain | G.OP_R16
    raise AssertionError("no candidate size of gl_smallest has live bins")


@pytest.mark.parametrize("source", ["live", "full"])
@pytest.mark.parametrize("case", ["float_80", "gl_smallest"])
def test_live_batches_take_live_blobs_and_full_chain_blobs(glvlib, case, source):
    """A (live, or the unflagged full chain) after 7 updates, live B after 2: A's {1, 4} into B's {5, 0}; the later bars of the two slots are A's.  A live
    blob says kept_bins == glv_batch_live_bins(), a full-chain blob kept_bins == n; a live blob into an unflagged batch is refused"""
    G = glvlib
    n, kw, ops = _live_case(G, case)
    w = kw["bars"]
    a = bars_batch(G, n, kw, None, FR, S, live=source == "live")
    b, twin = bars_batch(G, n, kw, None, FR, S), bars_batch(G, n, kw, None, FR, S)
    L = b.live_bins()
    assert 0 < L < n
    pairs, others = [(1, 5), (4, 0)], [1, 2, 3, 4, 6]
    xa, xb = _windows(900, 7 + FR + 3, n=n), _windows(950, 2 + FR + 3, n=n)
    assert b.stream_state_desc().kept_bins == n                 # the live class has not run yet
    for x in xa[:7]: _update(G, a, x, ops, w)
    for x in xb[:2]: assert _same(_update(G, b, x, ops, w), _update(G, twin, x, ops, w))
    d, blobs = _save(a, [1, 4])
    assert d.kept_bins == (L if source == "live" else n) and b.stream_state_desc().kept_bins == L
    _load(b, [5, 0], blobs, d)
    for u, (x, y) in enumerate(zip(xa[7:], _mixed(xb[2:], xa[7:], pairs))):
        oa, ob, ot = _update(G, a, x, ops, w), _update(G, b, y, ops, w), _update(G, twin, y, ops, w)
        for s, dst in pairs: assert _same(ob[dst], oa[s]), (case, source, u, s)
        assert _same(ob[others], ot[others]), (case, source, u)
        assert bool((oa != 0).any())
    if source == "live":
        full = bars_batch(G, n, kw, None, FR, S, live=False)
        with pytest.raises(G.GlvError) as ei:
            _load(full, [5, 0], blobs, d)
        assert ei.value.code == G.ERR_STATE and "live" in str(ei.value)
        full.close()
    _close(a, b, twin)


def test_a_live_blob_marks_a_fresh_live_batch_as_live(glvlib):
    """a live blob into a GLV_OP_BARS_ONLY batch that has not run yet: the batch then counts as having run its live class"""
    G = glvlib
    n, kw, ops = _live_case(G, "float_80")
    a, b = bars_batch(G, n, kw, None, FR, S), bars_batch(G, n, kw, None, FR, S)
    for x in _windows(970, 3, n=n): _update(G, a, x, ops, kw["bars"])
    d, blobs = _save(a, [1])
    assert b.stream_state_desc().kept_bins == n
    _load(b, [3], blobs, d)
    assert b.stream_state_desc().kept_bins == b.live_bins() == d.kept_bins
    x = _windows(980, 1, n=n)[0]
    y = _mixed([x], [x], [(1, 3)])[0]
    assert _same(_update(G, b, y, ops, kw["bars"])[3], _update(G, a, x, ops, kw["bars"])[1])
    _close(a, b)


# ---- form rules ---------------------------------------------------------------------------------------------------------------------------------------
def test_gravity_forms(glvlib):
    """a form-2 blob into a form-0 batch: the batch adopts the form and then refuses a form-1 call in refuse_gravity_mix's words; a form-1 blob into a
    form-2 batch is refused; an all-zero blob from a fresh batch loads into either and equals a reset"""
    G = glvlib
    g2 = G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE
    g1 = G.OP_FFT | G.OP_GRAVITY
    mk = lambda: _make(G, "chain_F5")[0]                        # noqa: E731
    two, one, zero, fresh = mk(), mk(), mk(), mk()
    xs = _windows(1000, 4)
    for x in xs[:3]: _update(G, two, x, g2); _update(G, one, x, g1)
    d2, blob2 = _save(two, [1])
    d1, blob1 = _save(one, [1])
    d0, blob0 = _save(fresh, [1])
    assert (d2.gravity_form, d1.gravity_form, d0.gravity_form) == (2, 1, 0) and bool((blob0 == 0).all())
    _load(zero, [4], blob2, d2)
    assert zero.stream_state_desc().gravity_form == 2
    with pytest.raises(G.GlvError) as ei:
        _update(G, zero, xs[3], g1)
    assert ei.value.code == G.ERR_STATE and "gravity was last applied fused with average" in str(ei.value)
    assert _same(_update(G, zero, _mixed([xs[3]], [xs[3]], [(1, 4)])[0], g2)[4], _update(G, two, xs[3], g2)[1])
    with pytest.raises(G.GlvError) as ei:
        _load(two, [0], blob1, d1)
    assert ei.value.code == G.ERR_STATE and "gravity was last applied fused with average" in str(ei.value)
    with pytest.raises(G.GlvError) as ei:
        _load(one, [0], blob2, d2)
    assert ei.value.code == G.ERR_STATE and "gravity was last applied without average" in str(ei.value)
    # the all-zero blob of a fresh batch: into a form-1 and a form-2 batch, against twins whose stream is reset
    for b, ops in ((one, g1), (two, g2)):
        twin = mk()
        for x in xs[:3]: _update(G, twin, x, ops)
        if b is two: _update(G, twin, xs[3], ops)
        _load(b, [0, 3], np.concatenate([blob0, blob0]), d0)
        _reset(twin, [0, 3])
        assert b.stream_state_desc().gravity_form == twin.stream_state_desc().gravity_form
        for x in _windows(1100, 3): assert _same(_update(G, b, x, ops), _update(G, twin, x, ops))
        assert _same(_save_all(b)[1], _save_all(twin)[1])
        twin.close()
    _close(two, one, zero, fresh)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------
def _refused(G, code, fn, *args, word=None):
    with pytest.raises(G.GlvError) as ei:
        fn(*args)
    assert ei.value.code == code, str(ei.value)
    if word: assert word in str(ei.value), str(ei.value)


def test_refusals_leave_the_batch_as_it_was(glvlib):
    """mismatched n, F and storage class, a misaligned blob, count == 0, NULL pointers: after each refusal the next process call gives what the twin gives"""
    import torch
    G = glvlib
    b, ops, F = _make(G, "chain_F5")
    twin = _make(G, "chain_F5")[0]
    xs = _windows(1200, 24)
    step = iter(xs)
    def still_the_twin():
        x = next(step)
        assert _same(_update(G, b, x, ops), _update(G, twin, x, ops))
    for _ in range(3): still_the_twin()
    d, blob = _save(b, [1]); _save(twin, [1])
    idx, d_blob = _idx([1]), torch.zeros((2 * int(d.bytes) + 64,), dtype=torch.uint8, device="cuda")
    for other in (G.Batch(G.Params(n=512, avg_frames=5), S, G.OP_GRAVITY | G.OP_AVERAGE), _make(G, "chain_F5", avg_frames=3)[0], _make(G, "gl_chain")[0],
                  _make(G, "gravity")[0], _make(G, "chain_F5", extra_mask=G.OP_RING_S16)[0]):
        _refused(G, G.ERR_STATE, b.load_streams, idx, 1, d_blob, other.stream_state_desc())
        still_the_twin()
        other.close()
    _refused(G, G.ERR_INVALID, b.load_streams, idx, 1, d_blob.data_ptr() + 4, d, word="16-byte")
    still_the_twin()
    _refused(G, G.ERR_INVALID, b.save_streams, idx, 1, d_blob.data_ptr() + 8, word="16-byte")
    _refused(G, G.ERR_INVALID, b.reset_streams, idx.data_ptr() + 2, 1)
    for call in ((b.reset_streams, idx, 0), (b.save_streams, idx, 0, d_blob), (b.load_streams, idx, 0, d_blob, d),
                 (b.reset_streams, None, 1), (b.save_streams, None, 1, d_blob), (b.save_streams, idx, 1, None), (b.load_streams, None, 1, d_blob, d),
                 (b.load_streams, idx, 1, None, d)):
        _refused(G, G.ERR_INVALID, *call)
        still_the_twin()
    L = G.lib()
    assert L.glv_batch_save_streams(b._h, C.c_void_p(idx.data_ptr()), 1, C.c_void_p(d_blob.data_ptr()), None, None) == G.ERR_INVALID
    assert L.glv_batch_load_streams(b._h, C.c_void_p(idx.data_ptr()), 1, C.c_void_p(d_blob.data_ptr()), None, None) == G.ERR_INVALID
    assert L.glv_batch_stream_state_desc(b._h, None) == G.ERR_INVALID
    still_the_twin()
    assert _same(_save_all(b)[1], _save_all(twin)[1])
    _close(b, twin)


def test_refused_while_the_output_is_the_state(glvlib):
    """GLV_OP_OUTPUT_IS_STATE in force: the latest gravity output lives in the caller's buffer -- all three refuse, naming the flag"""
    import torch
    G = glvlib
    b, ops, _ = _make(G, "gravity")
    twin = _make(G, "gravity")[0]
    xs = _windows(1300, 3)
    ob, ot = (torch.zeros((S * 2, N), dtype=torch.float32, device="cuda") for _ in range(2))
    for x in xs[:2]:
        b.process_s16(_dev(x), ob, ops | G.OP_OUTPUT_IS_STATE); twin.process_s16(_dev(x), ot, ops | G.OP_OUTPUT_IS_STATE)
    torch.cuda.synchronize()
    idx, d = _idx([1]), b.stream_state_desc()
    d_blob = torch.zeros((int(d.bytes),), dtype=torch.uint8, device="cuda")
    _refused(G, G.ERR_STATE, b.reset_streams, idx, 1, word="GLV_OP_OUTPUT_IS_STATE")
    _refused(G, G.ERR_STATE, b.save_streams, idx, 1, d_blob, word="GLV_OP_OUTPUT_IS_STATE")
    _refused(G, G.ERR_STATE, b.load_streams, idx, 1, d_blob, d, word="GLV_OP_OUTPUT_IS_STATE")
    b.process_s16(_dev(xs[2]), ob, ops | G.OP_OUTPUT_IS_STATE); twin.process_s16(_dev(xs[2]), ot, ops | G.OP_OUTPUT_IS_STATE)
    torch.cuda.synchronize()
    assert _same(ob.cpu().numpy(), ot.cpu().numpy())
    # ... and once a call has put the state back into the batch's own store they run
    _update(G, b, xs[0], ops)
    _reset(b, [1])
    _close(b, twin)


def test_refused_on_a_single_row_state_and_a_batch_without_state(glvlib):
    """the glv_state drop-ins' batch is one row: GLV_ERR_STATE (the handle's first member is that batch); a stateless batch resets with no launch and has
    nothing to save or load"""
    import torch
    G = glvlib
    s = G.State(G.Params(n=N))
    x0, x1 = np.linspace(-1, 1, N).astype(np.float32), np.linspace(0.5, -0.25, N).astype(np.float32)
    s.gravity(x0.copy())
    one_row = C.c_void_p.from_address(s._h.value).value                 # glv_state::b
    idx, d_blob, d = _idx([0]), torch.zeros((4096,), dtype=torch.uint8, device="cuda"), G.StreamStateDesc()
    L = G.lib()
    assert L.glv_batch_reset_streams(C.c_void_p(one_row), C.c_void_p(idx.data_ptr()), 1, None) == G.ERR_STATE
    assert L.glv_batch_save_streams(C.c_void_p(one_row), C.c_void_p(idx.data_ptr()), 1, C.c_void_p(d_blob.data_ptr()), C.byref(d), None) == G.ERR_STATE
    assert L.glv_batch_load_streams(C.c_void_p(one_row), C.c_void_p(idx.data_ptr()), 1, C.c_void_p(d_blob.data_ptr()), C.byref(d), None) == G.ERR_STATE
    assert L.glv_batch_stream_state_desc(C.c_void_p(one_row), C.byref(d)) == G.ERR_STATE
    twin = G.State(G.Params(n=N))
    twin.gravity(x0.copy())
    b1, b2 = x1.copy(), x1.copy()
    s.gravity(b1); twin.gravity(b2)
    assert _same(b1, b2) and not _same(b1, x1)
    s.close(); twin.close()
    b = G.Batch(G.Params(n=N), S, G.OP_FFT)
    x = _windows(1400, 1)[0]
    before = _update(G, b, x, G.OP_FFT)
    b.reset_streams(idx, 1)
    assert b.last_launches() == 0
    d = b.stream_state_desc()
    assert d.regions == 0 and d.bytes == 0
    _refused(G, G.ERR_STATE, b.save_streams, idx, 1, d_blob)
    _refused(G, G.ERR_STATE, b.load_streams, idx, 1, d_blob, d)
    assert _same(_update(G, b, x, G.OP_FFT), before)
    b.close()


# ---- hipGraph -----------------------------------------------------------------------------------------------------------------------------------------
def test_a_captured_reset_is_replayed_and_re_aimed(glvlib):
    """a reset of 2 streams captured into a hipGraph (one node, one stream; global capture mode: an allocation or a synchronous copy would invalidate it),
    replayed after two further updates with d_idx rewritten: the streams named then are fresh, the others untouched"""
    import torch
    G = glvlib
    hip = C.CDLL("libamdhip64.so")
    b, ops, F = _make(G, "chain_F5")
    twin, fresh = _make(G, "chain_F5")[0], _make(G, "chain_F5")[0]
    xs = _windows(1500, 2 + 2 + 3)
    for x in xs[:2]: _update(G, b, x, ops); _update(G, twin, x, ops)
    idx = _idx([1, 4])
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert hip.hipStreamBeginCapture(C.c_void_p(st.cuda_stream), 0) == 0
    try:
        b.reset_streams(idx, 2, stream=st.cuda_stream)
    finally:
        graph = C.c_void_p()
        rc = hip.hipStreamEndCapture(C.c_void_p(st.cuda_stream), C.byref(graph))
    assert rc == 0
    nodes = C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(nodes)) == 0 and nodes.value == 1
    exe = C.c_void_p()
    assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, C.c_size_t(0)) == 0
    # (the capture ran nothing: the batch still equals its twin)
    for x in xs[2:4]: assert _same(_update(G, b, x, ops), _update(G, twin, x, ops))
    idx.copy_(_idx([2, 5]))
    torch.cuda.synchronize()
    assert hip.hipGraphLaunch(exe, C.c_void_p(st.cuda_stream)) == 0
    st.synchronize()
    for x in xs[4:]:
        got, kept, new = _update(G, b, x, ops), _update(G, twin, x, ops), _update(G, fresh, x, ops)
        assert _same(got[[2, 5]], new[[2, 5]]) and _same(got[[0, 1, 3, 4, 6]], kept[[0, 1, 3, 4, 6]])
    hip.hipGraphExecDestroy(exe); hip.hipGraphDestroy(graph)
    _close(b, twin, fresh)


# ---- past the grid cap --------------------------------------------------------------------------------------------------------------------------------
def test_every_stream_of_a_large_batch_in_reversed_order(glvlib):
    """4096 streams of n = 256, F = 5 on float state: a stream is 768 pieces = 3 workgroup items, 12 288 in all against a grid cap of 2048 -- the kernel's
    loop makes 6 trips, and 2048 is no multiple of 3, so the (stream, chunk) pair carries on every trip.  All streams listed in reversed order; save / load
    round-trips every stream into a batch at another head"""
    G = glvlib
    streams = 4096
    a, ops, F = _make(G, "chain_F5", streams=streams)
    b = _make(G, "chain_F5", streams=streams)[0]
    xs = _windows(1600, 4, streams=streams)
    for x in xs[:3]: _update(G, a, x, ops)
    _update(G, b, xs[3], ops)
    order = list(range(streams - 1, -1, -1))
    d, rev = _save(a, order, guard=True)
    _, nat = _save_all(a)
    assert _same(rev[::-1], nat) and bool((nat != 0).any(axis=1).all())
    _load(b, order, rev, d)
    assert _same(_save_all(b)[1], nat)
    assert _same(_update(G, b, xs[3], ops), _update(G, a, xs[3], ops))
    _reset(b, order)
    assert bool((_save_all(b)[1] == 0).all())
    _close(a, b)
