"""GPU: elastic batches -- glv_batch_process_first_* / glv_batch_ring_update_first_* (the first `count` streams of a batch only) and glv_batch_copy_streams
(streams from slot to slot in one launch, no blob).

Contract (include/glv_spectrum.h): a prefix call is the un-suffixed call of a batch that has `count` streams -- the same output and state for streams
< count, nothing written at or behind row 2 * count; a copy is glv_batch_save_streams(src) + glv_batch_load_streams(dst), whatever positions the two batches
are at.  Every assertion is bit equality (floats as uint32).  The references are the library's own undisturbed paths, which the oracle suites hold to the
reference: a fresh batch of `count` streams, a twin that took the same streams through save and load, a one-stream batch per listener.

n = 256, capacity 7, prefixes 1, 4 and 7 (one stream; more than one workgroup's rows and no multiple of them; the whole batch) unless a case says more.
The helpers are those of tests/test_stream_slots.py."""
import ctypes as C

import numpy as np
import pytest

from glava_amd import stream_slots as SL
from test_stream_slots import (CHAINS, FILL, GUARD, N, S, _close, _dev, _idx, _live_case, _load, _make, _mixed, _refused, _ring_frames, _same, _save,
                               _save_all, _update, _windows)
from track_lib import bars_batch, pcm

pytestmark = pytest.mark.gpu

PREFIXES = (1, 4, 7)
METHODS = ("s16", "f32", "f32_stereo")
COPY_NAME = "glv_slot_copy_kernel"


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------------------
def _case(G, name, streams):
    """name -> (batch, ops, F, output width, window frames per n): the chains of test_stream_slots.py and the four the prefix test adds"""
    g, a = G.OP_GRAVITY, G.OP_AVERAGE
    if name in CHAINS or name == "bufscale2":
        b, ops, F = _make(G, "chain_F5" if name == "bufscale2" else name, streams=streams)
        if name == "bufscale2": b.set_bufscale(2)
        return b, ops, F, N, 2 if name == "bufscale2" else 1
    if name == "shipped":       # gl_storage 1, the pre-smoothing pass over every texel, texels out
        p = G.Params(n=N, avg_frames=5, avg_window_kind=1, gl_storage=1, bars=N, bar_phase=0.5)
        return G.Batch(p, streams, g | a | G.OP_BARS), G.OP_FFT | g | a | G.OP_BARS | G.OP_R16, 5, N, 1
    if name == "bars_only":
        n, kw, ops = _live_case(G, "float_80")
        b = bars_batch(G, n, kw, None, 5, streams)
        assert 0 < b.live_bins() < n
        return b, ops, 5, kw["bars"], 1
    assert name == "wave"
    return G.Batch(G.Params(n=N), streams, G.OP_WAVE), G.OP_WAVE | G.OP_R16, 1, N, 1


def _as(method, x):
    """int16 [streams][frames][2] as the input of process_<method>"""
    if method == "s16": return x
    f = x.astype(np.float32) / np.float32(32768)
    return f if method == "f32_stereo" else np.ascontiguousarray(f.transpose(0, 2, 1))


def _first(G, b, count, x, ops, w, method="process_first_s16", extra=()):
    """one prefix update from x (host, dense for `count` streams) -> [count][2][w]; the bytes in front of the output and behind row 2 * count, up to the
    rows a full call would write and a guard beyond, must come back as they were"""
    import torch
    elem = 2 if ops & G.OP_R16 else 4
    used, full = count * 2 * w * elem, b.streams * 2 * w * elem
    buf = torch.full((GUARD + full + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    out = buf[GUARD:GUARD + used]
    out.zero_()
    getattr(b, method)(count, _dev(x), *extra, out, ops)
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == FILL).all()), "a prefix call wrote in front of its output"
    assert bool((buf[GUARD + used:] == FILL).all()), "a prefix call wrote at or behind row 2 * count"
    return out.cpu().numpy().view(np.int16 if elem == 2 else np.float32).reshape(count, 2, w)


def _attempt(fn, *args):
    """(result, None), or (None, the refusal's code and words)"""
    from glava_amd import spectrum as G
    try:
        return fn(*args), None
    except G.GlvError as e:
        return None, (e.code, str(e))


def _states_equal(cap, ref, count):
    if cap.stream_state_desc().regions == 0:
        assert ref.stream_state_desc().regions == 0
        return True
    listed = list(range(count))
    (dc, sc), (dr, sr) = _save(cap, listed), _save(ref, listed)
    return _same(sc, sr) and (dc.gravity_form, dc.kept_bins, dc.bytes) == (dr.gravity_form, dr.kept_bins, dr.bytes)


# ---- the prefix -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", CHAINS + ["shipped", "bars_only", "wave", "bufscale2"])
def test_a_prefix_is_a_batch_of_that_size(glvlib, name, method):
    """process_first(count) on a capacity-7 batch against the plain call on a fresh `count`-stream batch, F + 3 updates: every output, the launches, the
    state at the end (save_streams of streams < count from both), and -- count == 7 -- the plain call on a capacity-7 twin.  What the plain call refuses the
    prefix call refuses in the same words."""
    G = glvlib
    for count in PREFIXES:
        cap, ops, F, w, k = _case(G, name, S)
        ref = _case(G, name, count)[0]
        n = cap.params.n
        for u, x in enumerate(_windows(2000 + count, F + 3, streams=S, n=k * n)):
            xin = np.ascontiguousarray(_as(method, x)[:count])
            want, no = _attempt(_update, G, ref, xin, ops, w, "process_" + method)
            got, refused = _attempt(_first, G, cap, count, xin, ops, w, "process_first_" + method)
            assert refused == no, (name, method, count, u)
            if no: break
            assert _same(got, want), (name, method, count, u)
            assert cap.last_launches() == ref.last_launches() and cap.kernel_name() == ref.kernel_name()
            assert bool((want != 0).any())
        else:
            assert _states_equal(cap, ref, count), (name, method, count, "state")
        assert no is None or method != "s16", (name, no)                  # every chain here runs from s16 frames
        _close(cap, ref)


def _ring_case(G, f32, streams):
    g, a = G.OP_GRAVITY, G.OP_AVERAGE
    if f32: return G.Batch(G.Params(n=N, avg_frames=3), streams, g | a | G.OP_RING_F32), G.OP_FFT | g | a
    return G.Batch(G.Params(n=N), streams, g | G.OP_RING_S16), G.OP_FFT | g


@pytest.mark.parametrize("frames", [37, 64])
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
def test_a_ring_prefix_is_a_ring_batch_of_that_size(glvlib, f32, frames):
    """both ring entries, 37 frames per update (the write position is never a multiple of a piece, the append wraps on the 7th) and 64: 8 updates against a
    `count`-stream ring batch; outputs, then the state with the rings"""
    G = glvlib
    kind = "f32" if f32 else "s16"
    for count in PREFIXES:
        (cap, ops), (ref, _) = _ring_case(G, f32, S), _ring_case(G, f32, count)
        for u in range(8):
            x = np.ascontiguousarray(_ring_frames(2100 + u, frames, f32)[:count])
            want = _update(G, ref, x, ops, method="ring_update_" + kind, extra=(frames,))
            got = _first(G, cap, count, x, ops, N, method="ring_update_first_" + kind, extra=(frames,))
            assert _same(got, want), (kind, frames, count, u)
            assert cap.last_launches() == ref.last_launches()
        assert _states_equal(cap, ref, count), (kind, frames, count)
        _close(cap, ref)


@pytest.mark.parametrize("grid", [1, 2])
def test_a_prefix_under_a_forced_grid(glvlib, grid):
    """glv_batch_set_grid 1 and 2 with a prefix of 5 of 7 (10 rows: a workgroup makes several trips): the automatic grid's bits"""
    G = glvlib
    forced, ops, F = _make(G, "chain_F5")
    auto = _make(G, "chain_F5")[0]
    forced.set_grid(grid)
    for u, x in enumerate(_windows(2200, F + 3)):
        got, want = _first(G, forced, 5, x[:5].copy(), ops, N), _first(G, auto, 5, x[:5].copy(), ops, N)
        assert _same(got, want), (grid, u)
        assert forced.last_grid() == grid
    assert _states_equal(forced, auto, 5)
    _close(forced, auto)


# ---- the life cycle ---------------------------------------------------------------------------------------------------------------------------------
def test_listeners_join_leave_and_the_pool_grows(glvlib):
    """12 updates of a capacity-6 GL chain (F = 5) driven by a DensePool: joins at updates 0, 0, 2 and 5 (a reset and a larger prefix), a leave from the
    middle at 4 (the last active slot copied into the hole), the pool grown to a capacity-9 batch at 6 (a cross-batch copy of all active streams; the new
    batch's head is 0, the old one's 1), a leave from the end at 7 (no copy), a join at 8 into a slot that held someone else.  Every listener's output on
    every update it lived through is that of a one-stream batch created when it joined and fed its own windows."""
    G = glvlib
    pool = SL.DensePool(6)
    batch, ops, F = _make(G, "gl_chain", streams=6)
    slot_of, ref_of = {}, {}
    copies = 0

    def join(who):
        slot_of[who] = pool.attach()
        ref_of[who] = _make(G, "gl_chain", streams=1)[0]
        batch.reset_streams(_idx([slot_of[who]]), 1)

    def leave(who):
        nonlocal copies
        move = pool.detach(slot_of.pop(who))
        ref_of.pop(who).close()
        if move is None: return
        src, dst = move
        batch.copy_streams(_idx([dst]), batch, _idx([src]), 1)
        assert batch.last_launches() == 1 and batch.kernel_name() == COPY_NAME
        copies += 1
        moved = [w for w, s in slot_of.items() if s == src]
        slot_of[moved[0]] = dst

    events = {0: [(join, "a"), (join, "b")], 2: [(join, "c")], 4: [(leave, "b")], 5: [(join, "d")], 7: [(leave, "d")], 8: [(join, "e")]}
    lived = {}
    for u in range(12):
        for fn, who in events.get(u, ()): fn(who)
        if u == 6:
            bigger = _make(G, "gl_chain", streams=9)[0]
            active = list(range(pool.active))
            bigger.copy_streams(_idx(active), batch, _idx(active), pool.active)
            pool.grow(9)
            batch.close()
            batch = bigger
        if u == 7: assert pool.active == 2 and copies == 1                   # the leave from the end moved nothing
        if u == 8: assert slot_of["e"] == 2                                  # ... and the slot d and c held before is e's
        windows = {who: pcm(3000 + 97 * ord(who) + 31 * u, 1, N) for who in slot_of}
        x = np.zeros((pool.active, N, 2), np.int16)
        for who, s in slot_of.items(): x[s] = windows[who][0]
        got = _first(G, batch, pool.active, x, ops, N)
        for who, s in slot_of.items():
            assert _same(got[s], _update(G, ref_of[who], windows[who], ops)[0]), (u, who, s)
            lived[who] = lived.get(who, 0) + 1
    assert sorted(slot_of.items()) == [("a", 0), ("c", 1), ("e", 2)] and pool.capacity == 9
    assert lived == {"a": 12, "b": 4, "c": 10, "d": 2, "e": 4}
    for b in ref_of.values(): b.close()
    batch.close()


# ---- the copy ---------------------------------------------------------------------------------------------------------------------------------------
PAIRS = [(0, 5), (6, 1), (3, 3)]                                            # (stream of src, stream of dst)


def _copy(dst, src, pairs, stream=None):
    import torch
    dst.copy_streams(_idx([d for _, d in pairs]), src, _idx([s for s, _ in pairs]), len(pairs), stream=stream)
    torch.cuda.synchronize()
    assert dst.last_launches() == 1 and dst.kernel_name() == COPY_NAME


def _by_blob(dst, src, pairs):
    d, blobs = _save(src, [s for s, _ in pairs])
    _load(dst, [t for _, t in pairs], blobs, d)


@pytest.mark.parametrize("chain", CHAINS)
def test_a_copy_is_save_plus_load(glvlib, chain):
    """src after 7 updates, dst and its twin after 4 (head 2 against 4 of F = 5; gl_chain: uint16 state; chain_F1: F = 1): the pairs by one copy into dst,
    by save and load into the twin -- the blobs of ALL streams of both are equal, src's are unchanged, and both continue bit for bit for F + 3 updates"""
    G = glvlib
    src, ops, F = _make(G, chain)
    dst, twin = _make(G, chain)[0], _make(G, chain)[0]
    xs = _windows(4000, 7) + _windows(4500, 4 + F + 3)
    for x in xs[:7]: _update(G, src, x, ops)
    for x in xs[7:11]: _update(G, dst, x, ops); _update(G, twin, x, ops)
    _, before = _save_all(src)
    _copy(dst, src, PAIRS)
    _by_blob(twin, src, PAIRS)
    (dd, sd), (dt, st) = _save_all(dst), _save_all(twin)
    assert _same(sd, st) and dd.gravity_form == dt.gravity_form, chain
    for s, t in PAIRS: assert _same(sd[t], before[s]) and bool((before[s] != 0).any())
    assert _same(_save_all(src)[1], before), (chain, "src was written")
    for u, x in enumerate(xs[11:]):
        assert _same(_update(G, dst, x, ops), _update(G, twin, x, ops)), (chain, u)
    assert _same(_save_all(dst)[1], _save_all(twin)[1])
    _close(src, dst, twin)


def _to_position(G, b, f32, appends, seed, also=()):
    kind = "f32" if f32 else "s16"
    for k, frames in enumerate(appends):
        x = _ring_frames(seed + k, frames, f32)
        for batch in (b, *also): _update(G, batch, x, batch_ops(G, f32), method="ring_update_" + kind, extra=(frames,))


def batch_ops(G, f32):
    return G.OP_FFT | G.OP_GRAVITY | (G.OP_AVERAGE if f32 else 0)


RING_POSITIONS = {0: (256,), 64: (64,), 37: (37,), 101: (64, 37)}


@pytest.mark.parametrize("pos_src,pos_dst", [(0, 64), (64, 37), (37, 64), (37, 101)], ids=["aligned_aligned", "aligned_off", "off_aligned", "off_off"])
@pytest.mark.parametrize("f32", [False, True], ids=["s16", "f32"])
def test_a_copy_between_rings_at_different_positions(glvlib, f32, pos_src, pos_dst):
    """ring batches whose write positions are 0 / 64 (a piece of the ring begins on 16 bytes: one access) or 37 / 101 (it does not, on s16 -- 37 mod 4 frames
    = 1 -- as on f32 -- 37 mod 2 = 1: single frames, each wrapped on its own), all four combinations of the two sides"""
    G = glvlib
    (src, ops), (dst, _), (twin, _) = (_ring_case(G, f32, S) for _ in range(3))
    _to_position(G, src, f32, RING_POSITIONS[pos_src], 5000)
    _to_position(G, dst, f32, RING_POSITIONS[pos_dst], 5100, also=(twin,))
    _, before = _save_all(src)
    _copy(dst, src, PAIRS)
    _by_blob(twin, src, PAIRS)
    sd, st = _save_all(dst)[1], _save_all(twin)[1]
    assert _same(sd, st), (f32, pos_src, pos_dst)
    for s, t in PAIRS: assert _same(sd[t], before[s]) and bool((before[s] != 0).any())
    assert _same(_save_all(src)[1], before)
    kind = "f32" if f32 else "s16"
    for u, frames in enumerate((64, 23, 256, 37)):
        x = _ring_frames(5200 + u, frames, f32)
        assert _same(_update(G, dst, x, ops, method="ring_update_" + kind, extra=(frames,)),
                     _update(G, twin, x, ops, method="ring_update_" + kind, extra=(frames,))), (f32, pos_src, pos_dst, u)
    assert _same(_save_all(dst)[1], _save_all(twin)[1])
    _close(src, dst, twin)


@pytest.mark.parametrize("chain", ["chain_F5", "gl_chain"])
def test_compaction_inside_one_batch(glvlib, chain):
    """dst == src: streams 5 and 6 into the holes 1 and 2, a pair (4, 4) that leaves its stream as it was; every other stream is untouched"""
    G = glvlib
    b, ops, F = _make(G, chain)
    for x in _windows(6000, F + 2): _update(G, b, x, ops)
    _, before = _save_all(b)
    _copy(b, b, [(5, 1), (6, 2), (4, 4)])
    _, after = _save_all(b)
    assert _same(after[1], before[5]) and _same(after[2], before[6]) and not _same(before[1], before[5])
    assert _same(after[[0, 3, 4, 5, 6]], before[[0, 3, 4, 5, 6]])
    _close(b)


def test_entries_past_either_batch_skip_their_pair(glvlib):
    G = glvlib
    src, ops, F = _make(G, "chain_F5")
    dst = _make(G, "chain_F5")[0]
    xs = _windows(6100, 5)
    for x in xs[:3]: _update(G, src, x, ops)
    for x in xs[3:]: _update(G, dst, x, ops)
    (_, bs), (_, bd) = _save_all(src), _save_all(dst)
    _copy(dst, src, [(S + 3, 2), (1, 0xFFFFFFFF), (2, 4), (S, S), (0x80000000, 0)])
    (_, as_), (_, ad) = _save_all(src), _save_all(dst)
    assert _same(as_, bs) and _same(ad[4], bs[2]) and not _same(bd[4], bs[2])
    assert _same(ad[[0, 1, 2, 3, 5, 6]], bd[[0, 1, 2, 3, 5, 6]])
    _close(src, dst)


def test_every_stream_of_701_in_reversed_order(glvlib):
    """701 streams of the float chain with F = 5: 3 chunks x 701 pairs = 2103 workgroup items against a grid cap of 2048 -- the kernel's loop makes a second
    trip, and 2048 is no multiple of 3, so the (pair, chunk) counter carries.  All streams in reversed order into a batch at another head"""
    G = glvlib
    streams = 701
    src, ops, F = _make(G, "chain_F5", streams=streams)
    dst, twin = _make(G, "chain_F5", streams=streams)[0], _make(G, "chain_F5", streams=streams)[0]
    xs = _windows(6200, 4, streams=streams)
    for x in xs[:3]: _update(G, src, x, ops)
    _update(G, dst, xs[3], ops); _update(G, twin, xs[3], ops)
    pairs = [(streams - 1 - j, j) for j in range(streams)]
    _copy(dst, src, pairs)
    _by_blob(twin, src, pairs)
    sd = _save_all(dst)[1]
    assert _same(sd, _save_all(twin)[1]) and _same(sd[::-1], _save_all(src)[1]) and bool((sd != 0).any(axis=1).all())
    assert _same(_update(G, dst, xs[3], ops), _update(G, twin, xs[3], ops))
    _close(src, dst, twin)


# ---- hipGraph ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_captured_copy_and_prefix_are_replayed_and_re_aimed(glvlib):
    """the FIRST calls of a fresh batch captured in torch.cuda.graph (global capture mode: an allocation or a synchronous copy would invalidate it): a copy
    of two streams from a batch at head 3 and F process_first calls (a full turn of the head, so that a replay starts where the capture did).  Replayed,
    then replayed with both tables and the inputs rewritten: each replay equals the eager calls on a twin, and the allocator saw nothing between"""
    import torch
    G = glvlib
    src, ops, F = _make(G, "chain_F5")
    dst, twin = _make(G, "chain_F5")[0], _make(G, "chain_F5")[0]
    for x in _windows(7000, 3): _update(G, src, x, ops)
    count = 4
    d_dst, d_src = _idx([0, 1]), _idx([2, 3])
    d_in = [torch.zeros((count, N, 2), dtype=torch.int16, device="cuda") for _ in range(F)]
    d_out = [torch.zeros((count * 2, N), dtype=torch.float32, device="cuda") for _ in range(F)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = torch.cuda.current_stream().cuda_stream
        dst.copy_streams(d_dst, src, d_src, 2, stream=st)
        for i in range(F): dst.process_first_s16(count, d_in[i], d_out[i], ops, stream=st)
    torch.cuda.synchronize()
    for r, (to, frm) in enumerate((([0, 1], [2, 3]), ([2, 3], [5, 6]))):
        xs = [np.ascontiguousarray(x[:count]) for x in _windows(7100 + 50 * r, F)]
        d_dst.copy_(_idx(to)); d_src.copy_(_idx(frm))
        for i in range(F): d_in[i].copy_(_dev(xs[i]))
        before = torch.cuda.memory_allocated()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
        _copy(twin, src, list(zip(frm, to)))
        for i in range(F):
            want = _first(G, twin, count, xs[i], ops, N)
            assert _same(d_out[i].cpu().numpy().reshape(count, 2, N), want), (r, i)
        assert _states_equal(dst, twin, count), r
    del graph
    _close(src, dst, twin)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_both_batches_as_they_were(glvlib):
    """a source of another n, F or storage, the form-1 / form-2 mix, count 0, NULL tables, prefixes of 0 and capacity + 1, a single-row batch: after each
    refusal both batches give the bits of twins that were never refused anything"""
    import torch
    G = glvlib
    g1, g2 = G.OP_FFT | G.OP_GRAVITY, G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE
    dst, ops, F = _make(G, "chain_F5")
    dst_twin, src, src_twin = (_make(G, "chain_F5")[0] for _ in range(3))
    steps = iter(_windows(8000, 40))

    def still_the_twins():
        x = next(steps)
        assert _same(_update(G, dst, x, ops), _update(G, dst_twin, x, ops)) and _same(_update(G, src, x, g1), _update(G, src_twin, x, g1))
    for _ in range(3): still_the_twins()
    one, idx = _idx([1]), _idx([2])
    _refused(G, G.ERR_STATE, dst.copy_streams, one, src, idx, 1, word="gravity was last applied fused with average")        # src runs gravity without average
    still_the_twins()
    _refused(G, G.ERR_STATE, src.copy_streams, one, dst, idx, 1, word="gravity was last applied without average")
    still_the_twins()
    for other in (G.Batch(G.Params(n=512, avg_frames=5), S, G.OP_GRAVITY | G.OP_AVERAGE), _make(G, "chain_F5", avg_frames=3)[0], _make(G, "gl_chain")[0],
                  _make(G, "gravity")[0], _make(G, "chain_F5", extra_mask=G.OP_RING_S16)[0]):
        _refused(G, G.ERR_STATE, dst.copy_streams, one, other, idx, 1, word="glv_batch_copy_streams: the source batch")
        _refused(G, G.ERR_STATE, other.copy_streams, one, dst, idx, 1, word="not of this batch's kind")
        still_the_twins()
        other.close()
    for call in ((dst.copy_streams, one, dst, idx, 0), (dst.copy_streams, None, dst, idx, 1), (dst.copy_streams, one, dst, None, 1),
                 (dst.copy_streams, one.data_ptr() + 2, dst, idx, 1)):
        _refused(G, G.ERR_INVALID, *call, word="glv_batch_copy_streams")
        still_the_twins()
    L = G.lib()
    assert L.glv_batch_copy_streams(dst._h, C.c_void_p(one.data_ptr()), None, C.c_void_p(idx.data_ptr()), 1, None) == G.ERR_INVALID
    d_in = torch.zeros((S + 1, N, 2), dtype=torch.int16, device="cuda")
    d_out = torch.zeros(((S + 1) * 2, N), dtype=torch.float32, device="cuda")
    for count in (0, S + 1):
        for method in METHODS:
            _refused(G, G.ERR_INVALID, getattr(dst, "process_first_" + method), count, d_in, d_out, ops, word=f"count={count}")
        for kind in ("s16", "f32"):
            _refused(G, G.ERR_INVALID, getattr(dst, "ring_update_first_" + kind), count, d_in, 8, d_out, ops, word=f"count={count}")
        still_the_twins()
    _refused(G, G.ERR_STATE, dst.ring_update_first_s16, 2, d_in, 8, d_out, ops, word="GLV_OP_RING_S16")           # the un-suffixed call's words
    _refused(G, G.ERR_INVALID, dst.process_first_s16, 2, d_in, d_out, G.OP_GRAVITY, word="s16 input requires")
    still_the_twins()
    # two batches that keep nothing, and the drop-ins' single row
    plain = G.Batch(G.Params(n=N), S, G.OP_FFT)
    _refused(G, G.ERR_STATE, plain.copy_streams, one, plain, idx, 1, word="neither state nor a ring")
    plain.close()
    s = G.State(G.Params(n=N))
    s.gravity(np.linspace(-1, 1, N).astype(np.float32))
    one_row = C.c_void_p(C.c_void_p.from_address(s._h.value).value)            # glv_state::b
    assert L.glv_batch_process_first_s16(one_row, 1, C.c_void_p(d_in.data_ptr()), C.c_void_p(d_out.data_ptr()), ops, None) == G.ERR_STATE
    assert L.glv_batch_copy_streams(one_row, C.c_void_p(one.data_ptr()), one_row, C.c_void_p(idx.data_ptr()), 1, None) == G.ERR_STATE
    s.close()
    still_the_twins()
    assert _same(_save_all(dst)[1], _save_all(dst_twin)[1]) and _same(_save_all(src)[1], _save_all(src_twin)[1])
    _close(dst, dst_twin, src, src_twin)


def test_a_live_source_is_refused_by_a_batch_that_keeps_whole_rows(glvlib):
    """a GLV_OP_BARS_ONLY batch that has run its live class keeps bins below glv_batch_live_bins() only: its streams go into a live batch of the same bins
    (which then counts as having run), not into the full chain"""
    G = glvlib
    n, kw, ops = _live_case(G, "float_80")
    w = kw["bars"]
    live, live_twin, fresh = (bars_batch(G, n, kw, None, 5, S) for _ in range(3))
    full, full_twin = (bars_batch(G, n, kw, None, 5, S, live=False) for _ in range(2))
    xs = _windows(9000, 6, n=n)
    for x in xs[:3]:
        for b in (live, live_twin, full, full_twin): _update(G, b, x, ops, w)
    one, idx = _idx([1]), _idx([2])
    _refused(G, G.ERR_STATE, full.copy_streams, one, live, idx, 1, word="GLV_OP_BARS_ONLY")
    for x in xs[3:5]:
        assert _same(_update(G, full, x, ops, w), _update(G, full_twin, x, ops, w)) and _same(_update(G, live, x, ops, w), _update(G, live_twin, x, ops, w))
    assert fresh.stream_state_desc().kept_bins == n
    _copy(fresh, live, [(1, 3)])
    assert fresh.stream_state_desc().kept_bins == fresh.live_bins() == live.stream_state_desc().kept_bins
    y = _mixed([xs[5]], [xs[5]], [(1, 3)])[0]
    assert _same(_update(G, fresh, y, ops, w)[3], _update(G, live, xs[5], ops, w)[1])
    _close(live, live_twin, fresh, full, full_twin)
