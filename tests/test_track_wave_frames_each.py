"""GPU: track mode at render frames per stream for the wave module (glv_batch_track_each_wave_frames_* / glv_batch_track_pool_wave_frames_*) -- every stream
with its own rows of the frame tables and of the window starts, its own number of steps and of frames and its own keep pair, its keyframes read from its own
windows of its recording or of its span of a pool.

Contract (include/glv_spectrum.h), everything compared with == on bits: a stream with c_s >= 1 steps and f_s >= 1 frames is glv_batch_track_wave_frames_* on a
ONE-stream batch over its own recording (pool entries: its materialised span, entries pre-clamped) with steps = c_s, frames = f_s, its rows, its rows of d_keys
and its keep pair; a stream with c_s = 0 lerps between its two carried keyframes (numpy float32 and the upload's quantiser, tests/track_wave_frames_each_lib.py);
blocks at j >= f_s are what the call's last stage makes of a zero texel row -- the block the lockstep call gives from zero keys with from == to == 0.

The shapes are tests/test_track_wave_frames.py's: n 256 (one group of lanes) and 1024 (four), 3 streams, 9 steps, 23 frames, batches created under
GLV_TRACK_FRAMES_SEGMENT=5 (five segments, the last one ragged); step counts (9, 4, 0) and frame counts (23, 11, 7), one of which ends inside a segment.  The
recordings begin one frame (planar: one float) behind a load boundary, so that both the wide and the narrow loads occur (asserted); workspace and output are
exactly the size asked for with guards behind both; 0xFFFFFFFF sits behind every count in d_from / d_to / d_starts and NaN behind the frame counts in d_mod: a
read past a count shows as wrong bits, never as a fault."""
import ctypes as C

import numpy as np
import pytest

from glava_amd.bar_positions import graph_column_texels
from glava_amd.track_starts import SPAN_DTYPE, keyframe_tables, renderer_starts, stack_frame_tables
from gpu_lib import eq
from oracle_lib import Oracle
from test_track_each import _dev_u32, _dev_ur
from test_track_frames import FROM, MOD, MODIFIED, TO, _keys, _same
from test_track_frames_each import COUNTS, FCOUNTS, FPS, KEEP, KNAME, _device, _layout, _rows
from test_track_wave_frames import FRAMES, STEPS, _batch, _forms, _launches, _want
from track_lib import GUARD, differing, out_dtype, rec, seq, windows
from track_wave_frames_each_lib import each_starts, keep_each, lerp_each, pool_starts, rows_each

pytestmark = pytest.mark.gpu
F32 = np.float32
STREAMS = 3
BIG = 0xFFFFFFFF
KERNEL = "glv_wave_frames_each_kernel"
ELEMENT = {"s16": 4, "f32": 8, "planar": 4}                                        # bytes between two frames of a channel


def _guarded(frm, to, mod, fcounts):
    """the three frame tables with 0xFFFFFFFF / NaN behind every stream's frame count"""
    frm, to, mod = np.array(frm, dtype=np.uint32), np.array(to, dtype=np.uint32), np.array(mod, dtype=np.float32)
    for s, f in enumerate(fcounts):
        frm[s, f:] = BIG; to[s, f:] = BIG; mod[s, f:] = np.nan
    return frm, to, mod


class _Wave:
    """recordings (or a pool and spans), a row of window starts per stream at its own display rate, and the calls on them"""

    def __init__(self, G, n, kind, pool, seed, channels=2, streams=STREAMS, steps=STEPS, stray=False):
        self.G, self.n, self.kind, self.pool, self.streams, self.steps = G, n, kind, pool, streams, steps
        self.f32 = kind != "s16"
        self.channels = 2 if kind == "planar" else channels                       # (the planar kinds do no mono mix)
        self.starts = np.asarray([renderer_starts(22050, FPS[s], 1, steps) for s in range(3)] + [[7 * t for t in range(steps)]] * (streams - 3), dtype=np.uint32)[:streams]
        longest = int(self.starts.max()) + n + 38
        if pool:
            # streams 0 and 1 on ONE span at different rates, stream 2 nested in it off a group of 8 frames and short enough that its late entries clamp;
            # stray: a fourth, live stream whose span lies outside the pool -- its windows are the pool's last window
            a = (16, longest)
            self.spans = [a, a, (a[0] + 257, int(self.starts[2, 5]) + n)] + ([((a[0] + a[1] + 45) | 1, 4 * n)] if stray else [])
            assert len(self.spans) == streams and (self.spans[2][0] - a[0]) % 8 != 0
            self.pool_frames = (a[0] + a[1] + 45) | 1
            if stray: assert self.spans[3][0] >= self.pool_frames
            self.x = rec(seed, 1, self.pool_frames, self.f32)[0]                   # [pool_frames][2]
            body = np.ascontiguousarray(self.x.T) if kind == "planar" else self.x
            self.d_pcm = _device(body, kind, 2 * n)
            self.d_spans = self._dev_spans()
            self.where = pool_starts(self.spans, self.starts, self.pool_frames, n)
            self.recordings = [self.x] * streams
            inside = np.asarray([[min(int(e), max(fr - n, 0)) for e in row] for row, (_, fr) in zip(self.starts, self.spans)])
            assert (inside[2] != self.starts[2]).any() and (inside[:2] == self.starts[:2]).all()      # the short span's late entries clamp, the shared span's do not
            if stray: assert (self.where[3] == self.pool_frames - n).all()
            base = [self.d_pcm.data_ptr() + int(a) * ELEMENT[kind] for a in self.where.reshape(-1)]
        else:
            self.pitch = longest | 1
            self.x = rec(seed, streams, self.pitch, self.f32)                      # [streams][pitch][2]
            self.d_pcm = _device(_layout(self.x, kind), kind, 2 * n)
            self.where = each_starts(self.starts, self.pitch, n)
            self.recordings = list(self.x)
            rows = 2 if kind == "planar" else 1
            base = [self.d_pcm.data_ptr() + (s * rows * self.pitch + int(a)) * ELEMENT[kind] for s in range(streams) for a in self.where[s]]
        at = {p % 16 for p in base}
        assert 0 in at and len(at) > 1, at                                       # groups that take the wide loads, and groups that do not

    def _dev_spans(self):
        import torch
        a = np.zeros((len(self.spans) + 1,), dtype=np.dtype(SPAN_DTYPE))
        for s, (first, frames) in enumerate(self.spans):
            a[s] = (first, frames, 0xDEADBEEF)
        a[-1] = (0xFFFFFFFFFFFFFFF0, 0xFFFFFFFF, 0)                                # one record behind the last stream: never read
        t = torch.from_numpy(a.view(np.int32).copy()).cuda()
        assert t.data_ptr() % 16 == 0
        return t

    def head(self, d_pcm=None):
        d_pcm = self.d_pcm if d_pcm is None else d_pcm
        if self.pool: return [d_pcm, self.pool_frames, self.d_spans]
        return [d_pcm] if self.kind == "planar" else [d_pcm, self.pitch]

    def tables(self, counts, starts=None, steps=None):
        """(d_starts, None, d_counts): the starts with 0xFFFFFFFF behind every stream's count"""
        steps = self.steps if steps is None else steps
        starts = np.array(self.starts if starts is None else starts, dtype=np.uint32)
        if counts is not None:
            for s, c in enumerate(counts): starts[s, c:] = BIG
        return (_dev_u32(starts, steps), None, _dev_u32(counts, 1) if counts is not None else None)

    def keyframes(self, counts, where=None):
        """float32 [steps][units][n] in numpy, NaN behind a stream's count"""
        return rows_each(self.recordings, self.where if where is None else where, counts, self.n, self.f32, self.channels)

    def call(self, b, tables, frame_rows, keys, ops, w, steps=None, stream=None):
        """one per-stream wave frames call: frame_rows = (from, to, mod, frame_counts or None, keep) in numpy; [frames][units][w], both guards checked"""
        import torch
        steps = self.steps if steps is None else steps
        frm, to, mod, fcounts, keep = frame_rows
        frames = frm.shape[1]
        dev = (_dev_u32(frm, frames), _dev_u32(to, frames), _dev_ur(mod), _dev_u32(fcounts, 1) if fcounts is not None else None, _dev_u32(keep, 2))
        dt = out_dtype(self.G, ops)
        nbytes = b.track_wave_frames_work_bytes(steps, frames, ops)
        up = lambda v: (v + 255) & ~255                                          # noqa: E731
        if not ops & self.G.OP_BARS: assert nbytes == 256
        else: assert nbytes in (up(frames * self.streams * 2 * self.n * 2), up(frames * self.streams * 2 * self.n * 4)), nbytes
        work = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        assert work.data_ptr() % 256 == 0
        count = frames * self.streams * 2 * w
        fill = 23130 if dt == torch.int16 else -7.0
        flat = torch.full((count + GUARD,), fill, dtype=dt, device="cuda")       # (the output too: a row the call leaves stale shows)
        name = ("track_pool_wave_frames_" if self.pool else "track_each_wave_frames_") + KNAME[self.kind]
        getattr(b, name)(*self.head(), tables, steps, dev, frames, keys, flat, work, ops, stream=stream)
        torch.cuda.synchronize()
        assert bool((work[nbytes:] == 0xA5).all()), "the call wrote behind the workspace it asked for"
        assert bool((flat[count:] == fill).all()), "the call wrote behind its output"
        if not ops & self.G.OP_BARS: assert bool((work[:nbytes] == 0xA5).all()), "a call without bars touched the workspace"
        return flat[:count].view(frames, self.streams * 2, w)


def _lockstep(G, b, kind, d_rec, pitch, starts, steps, frm, to, mod, keys, keep, ops, w):
    """glv_batch_track_wave_frames_* on `b` over recordings d_rec: [frames][units][w]"""
    import torch
    frames = len(frm)
    nbytes = b.track_wave_frames_work_bytes(steps, frames, ops)
    work = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    count = frames * b.streams * 2 * w
    flat = torch.zeros((count + GUARD,), dtype=out_dtype(G, ops), device="cuda")
    head = [d_rec] if kind == "planar" else [d_rec, pitch]
    getattr(b, "track_wave_frames_" + KNAME[kind])(*head, _dev_u32(starts, 0), steps, _dev_u32(frm, 0), _dev_u32(to, 0), _dev_ur(mod), frames, keys, keep, flat, work, ops)
    torch.cuda.synchronize()
    assert bool((work[nbytes:] == 0xA5).all()) and not bool(flat[count:].any())
    return flat[:count].view(frames, b.streams * 2, w)


def _twin(S, s, c, frm, to, mod, keys, keep, form, ops, w):
    """stream s alone: a one-stream batch over its own recording (pool: its materialised span, entries pre-clamped), its first c steps"""
    G, n = S.G, S.n
    if S.pool:
        first, frames = S.spans[s]
        host = S.x[None, first:first + frames]
        starts = [min(int(e), frames - n) for e in S.starts[s, :c]]
    else:
        host, starts = S.x[s:s + 1], S.starts[s, :c]
    t = _batch(G, n, 1, form, S.channels)
    got = _lockstep(G, t, S.kind, _device(_layout(host, S.kind), S.kind, 2 * n), host.shape[1], starts, c, frm, to, mod, keys, keep, ops, w)
    assert t.kernel_name() == "glv_wave_frames_kernel"
    t.close()
    return got


def _zero_block(G, n, form, channels, ops, w):
    """what the call's last stage makes of a zero texel row, [w]: the block the lockstep call gives from zero keys with from == to == 0"""
    x = rec(77, 1, (n + 38) | 1, False)
    t = _batch(G, n, 1, form, channels)
    got = _lockstep(G, t, "s16", _device(x, "s16", 2 * n), x.shape[1], [0], 1, [0], [0], [0.0], _keys(n, 1), (0, 1), ops, w)
    t.close()
    assert eq(got[0, 0], got[0, 1])
    return got[0, 0].clone()


# ---- 1. equal rows, NULL counts, equal keep pairs: the lockstep call ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [2, 1], ids=["stereo", "mono"])
@pytest.mark.parametrize("kind", ["s16", "f32", "planar"])
@pytest.mark.parametrize("n", [256, 1024])
def test_equal_rows_null_counts_and_equal_keep_pairs_are_the_lockstep_call(glvlib, n, kind, channels):
    G = glvlib
    S = _Wave(G, n, kind, False, 501, channels)
    row = S.starts[1]
    tile = lambda v, dt: np.tile(np.asarray(v, dtype=dt), (STREAMS, 1))           # noqa: E731
    for form, (_, _, w, ops) in _forms(G, n).items():
        be, bl = _batch(G, n, STREAMS, form, channels), _batch(G, n, STREAMS, form, channels)
        ke, kl = _keys(n, STREAMS, 31), _keys(n, STREAMS, 31)
        got = S.call(be, S.tables(None, tile(row, np.uint32)), (tile(FROM, np.uint32), tile(TO, np.uint32), tile(MOD, np.float32), None, tile((9, 10), np.uint32)), ke, ops, w)
        assert be.last_launches() == _launches(ops, G) and be.kernel_name() == KERNEL, (form, be.last_launches(), be.kernel_name())
        want = _lockstep(G, bl, kind, S.d_pcm, S.pitch, row, STEPS, FROM, TO, MOD, kl, (9, 10), ops, w)
        assert bl.last_launches() == be.last_launches() and bl.kernel_name() == "glv_wave_frames_kernel"
        assert eq(got, want), (form, differing(got, want))
        assert eq(ke, kl), form
        be.close(); bl.close()


# ---- 2. different rows per stream ----------------------------------------------------------------------------------------------------------------------------------
MIXED = [(kind, pool, n, 2) for kind in ("s16", "f32", "planar") for pool in (False, True) for n in (256, 1024)] + [("s16", False, 256, 1), ("f32", True, 1024, 1)]


@pytest.mark.parametrize("kind,pool,n,channels", MIXED, ids=["%s%s-n%d%s" % (k, "-pool" if p else "", n, "-mono" if c == 1 else "") for k, p, n, c in MIXED])
def test_every_stream_is_its_one_stream_twin(glvlib, oracle, kind, pool, n, channels):
    """another display rate, table permutation, count, frame count and keep pair per stream"""
    G = glvlib
    S = _Wave(G, n, kind, pool, 502, channels)
    frm, to, mod = _guarded(*_rows(), FCOUNTS)
    rows = S.keyframes(COUNTS)
    for form in ("texels", "floats", "pass", "bar_floats", "maximum"):
        _, _, w, ops = _forms(G, n)[form]
        b = _batch(G, n, STREAMS, form, channels)
        keys = _keys(n, STREAMS, 32)
        k_before = keys.clone()
        kh = k_before.cpu().numpy()
        got = S.call(b, S.tables(COUNTS), (frm, to, mod, np.asarray(FCOUNTS, dtype=np.uint32), np.asarray(KEEP, dtype=np.uint32)), keys, ops, w)
        assert b.last_launches() == _launches(ops, G) and b.kernel_name() == KERNEL, (form, b.last_launches(), b.kernel_name())
        zero = _zero_block(G, n, form, channels, ops, w)
        for s in range(STREAMS):
            c, f = COUNTS[s], FCOUNTS[s]
            mine, mine_keys = got[:, 2 * s:2 * s + 2], keys[:, 2 * s:2 * s + 2]
            if c >= 1:                                                            # no stream with steps is skipped
                tk = k_before[:, 2 * s:2 * s + 2].contiguous().clone()
                assert tk.data_ptr() % 16 == 0
                want = _twin(S, s, c, frm[s, :f], to[s, :f], mod[s, :f], tk, KEEP[s], form, ops, w)
                assert eq(mine[:f], want), (form, s, differing(mine[:f], want))
                assert eq(mine_keys, tk), (form, s, "keys")
            else:                                                                 # numpy float32 and unorm16: the two carried keyframes only
                wl, shown = lerp_each(kh, rows, frm, to, mod, COUNTS, FCOUNTS, STEPS)
                assert shown[:f, s].all() and not shown[f:, s].any() and np.isnan(rows[:, 2 * s:2 * s + 2]).all()
                U = Oracle.texels_r16(wl[:f, 2 * s:2 * s + 2].reshape(-1, n)).reshape(f, 2, n)
                g = mine[:f].cpu().numpy()
                if form in ("texels", "floats"): assert _same(g, _want(G, form, n, U)), (form, s)      # every frame, row and sample
                else:
                    for j in (0, f - 1): assert _same(g[j, 1], _want(G, form, n, U[j, 1])), (form, s, j)
                assert eq(mine_keys, k_before[:, 2 * s:2 * s + 2]), (form, s, "keep (0, 1)")
            for j in range(f, FRAMES):
                for ch in range(2): assert eq(mine[j, ch], zero), (form, s, j, "a frame behind the count")
        assert _same(keys.cpu().numpy(), keep_each(kh, rows, KEEP, COUNTS, STEPS)), form
        b.close()


# ---- 3. a pool: shared, nested and malformed spans against the materialised copy -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["s16", "f32", "planar"])
def test_a_pool_is_the_each_entry_on_the_materialised_copy(glvlib, oracle, kind):
    G = glvlib
    n, streams = 256, 4
    P = _Wave(G, n, kind, True, 503, streams=streams, stray=True)
    counts, fcounts = (9, 4, 9, 6), (23, 11, 7, 23)
    keep = np.asarray([(9, 10), (1, 5), (BIG, 3), (7, 2)], dtype=np.uint32)
    frm, to, mod = _guarded(*_rows(streams), fcounts)
    # the materialised copy: every stream's windows cut out of the pool where pool_window_start puts them, laid back to back in a recording of its own
    pitch = STEPS * n + 1
    x = np.zeros((streams, pitch, 2), dtype=P.x.dtype)
    entries = np.zeros((streams, STEPS), dtype=np.uint32)
    for s in range(streams):
        for t in range(STEPS):
            x[s, t * n:(t + 1) * n] = P.x[P.where[s, t]:P.where[s, t] + n]
            entries[s, t] = t * n
    E = _Wave(G, n, kind, False, 503, streams=streams)
    E.pitch, E.x, E.starts, E.d_pcm = pitch, x, entries, _device(_layout(x, kind), kind, 2 * n)
    for form in ("texels", "pass"):
        _, _, w, ops = _forms(G, n)[form]
        bp, be = _batch(G, n, streams, form), _batch(G, n, streams, form)
        kp, ke = _keys(n, streams, 33), _keys(n, streams, 33)
        kh = kp.cpu().numpy()
        rows = (frm, to, mod, np.asarray(fcounts, dtype=np.uint32), keep)
        got = P.call(bp, P.tables(counts), rows, kp, ops, w)
        want = E.call(be, E.tables(counts), rows, ke, ops, w)
        assert bp.kernel_name() == KERNEL and bp.last_launches() == _launches(ops, G)
        assert eq(got, want), (form, differing(got, want))
        assert eq(kp, ke), form
        if form == "texels":                                                      # ... and numpy, from the pool itself
            kf = P.keyframes(counts)
            wl, _ = lerp_each(kh, kf, frm, to, mod, counts, fcounts, STEPS)
            assert _same(got.cpu().numpy(), Oracle.texels_r16(wl.reshape(-1, n)).reshape(FRAMES, streams * 2, n))
            assert _same(kp.cpu().numpy(), keep_each(kh, kf, keep, counts, STEPS))
        bp.close(); be.close()


# ---- 4. a session cut in two at another step per stream ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,kind,pool", [("texels", "s16", False), ("pass", "f32", True), ("floats", "planar", False)])
def test_a_session_cut_in_two_at_another_step_per_stream_is_the_uncut_call(glvlib, form, kind, pool):
    """stream s takes 4, 2 and 0 of its 9 steps in the first call and the rest in the second; each piece starts from the d_keys its predecessor left"""
    G = glvlib
    n = 256
    _, _, w, ops = _forms(G, n)[form]
    S = _Wave(G, n, kind, pool, 504)
    on, uratio = [True] * FRAMES, [0.4] * FRAMES
    first_steps = [4, 2, 0]
    cuts = [[j for j, m in enumerate(MODIFIED) if m][c] for c in first_steps]
    assert len(set(cuts)) == 3 and cuts[2] == 0
    whole = stack_frame_tables([keyframe_tables(MODIFIED, on, uratio)] * STREAMS)
    a_rows, b_rows = [], []
    for cut in cuts:
        if cut == 0:
            a_rows.append(([], [], [], 0, 1)); b_rows.append(keyframe_tables(MODIFIED, on, uratio))
            continue
        idle = cut - 1 - max(j for j in range(cut) if MODIFIED[j])
        a_rows.append(keyframe_tables(MODIFIED[:cut], on[:cut], uratio[:cut]))
        b_rows.append(keyframe_tables(MODIFIED[cut:], on[cut:], uratio[cut:], kcounter=idle))
    part_a, part_b = stack_frame_tables(a_rows), stack_frame_tables(b_rows)
    assert part_a[3].tolist() == cuts and part_b[3].tolist() == [FRAMES - c for c in cuts]
    sa, sb = max(first_steps), STEPS - min(first_steps)
    pad = lambda rows, steps: np.asarray([list(r) + [0] * (steps - len(r)) for r in rows], dtype=np.uint32)      # noqa: E731
    tab_a = S.tables(first_steps, pad([S.starts[s, :c] for s, c in enumerate(first_steps)], sa), sa)
    tab_b = S.tables([STEPS - c for c in first_steps], pad([S.starts[s, c:] for s, c in enumerate(first_steps)], sb), sb)
    bw, bc = _batch(G, n, STREAMS, form), _batch(G, n, STREAMS, form)
    kw_, kc = _keys(n, STREAMS, 34), _keys(n, STREAMS, 34)
    want = S.call(bw, S.tables(None), whole, kw_, ops, w)
    a = S.call(bc, tab_a, part_a, kc, ops, w, steps=sa)
    b = S.call(bc, tab_b, part_b, kc, ops, w, steps=sb)
    for s, cut in enumerate(cuts):
        r = slice(2 * s, 2 * s + 2)
        assert eq(a[:cut, r], want[:cut, r]) and eq(b[:FRAMES - cut, r], want[cut:, r]), (form, s)
    assert eq(kc, kw_)
    bw.close(); bc.close()


# ---- 5. more work items than the grid ---------------------------------------------------------------------------------------------------------------------------------
def test_more_work_items_than_the_grid_has_workgroups(glvlib, oracle):
    """n = 256, three streams, segments of one frame: 3 * 2800 work items of the frames kernel against its 8192 workgroups (glv_track_frames.hip kFramesGridCap) --
    the grid loops, over streams with ragged frame counts and step counts; frames around the wrap (item 8192: frame 2730, stream 2) against numpy"""
    G = glvlib
    n, frames = 256, 2800
    assert STREAMS * frames > 256 * 32 and 8192 // STREAMS == 2730
    S = _Wave(G, n, "s16", False, 505)
    counts, fcounts = [9, 4, 0], [2800, 2731, 2790]
    rng = np.random.default_rng(23)
    frm = rng.integers(0, STEPS + 3, (STREAMS, frames)).astype(np.uint32)
    to = rng.integers(0, STEPS + 3, (STREAMS, frames)).astype(np.uint32)
    mod = rng.random((STREAMS, frames), dtype=np.float32)
    frm, to, mod = _guarded(frm, to, mod, fcounts)
    keep = np.asarray([(c + 1, c // 2) for c in counts], dtype=np.uint32)
    b = _batch(G, n, STREAMS, "texels", segment=1)
    ops = G.OP_WAVE | G.OP_R16
    keys = _keys(n, STREAMS, 35)
    kh = keys.cpu().numpy()
    got = S.call(b, S.tables(counts), (frm, to, mod, np.asarray(fcounts, dtype=np.uint32), keep), keys, ops, n).cpu().numpy()
    rows = S.keyframes(counts)
    sample = sorted({0, 1, 2, 2728, 2729, 2730, 2731, 2732, 2733, 2789, 2790, 2791, frames - 2, frames - 1} | {int(v) for v in rng.integers(0, frames, 30)})
    pick = lambda t: t[:, sample]                                                 # noqa: E731
    fc = [sum(1 for j in sample if j < f) for f in fcounts]
    wl, shown = lerp_each(kh, rows, pick(frm), pick(to), pick(mod), counts, fc, STEPS)
    U = Oracle.texels_r16(wl.reshape(-1, n)).reshape(len(sample), STREAMS * 2, n)
    for i, j in enumerate(sample):
        for s in range(STREAMS):
            assert bool(shown[i, s]) == (j < fcounts[s])
            assert _same(got[j, 2 * s:2 * s + 2], U[i, 2 * s:2 * s + 2]), (j, s)     # (a frame not shown: zero texels, which U holds for w = 0)
    assert _same(keys.cpu().numpy(), keep_each(kh, rows, keep, counts, STEPS))
    b.close()


# ---- 6. graph capture -------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_captured_first_call_replayed_after_rewriting_the_tables(glvlib, oracle):
    """kernels only: the first call of a batch can be captured (one stream, a linear graph); d_mod, a row of d_starts, d_counts and d_keep are read when the
    kernels run"""
    import torch
    G = glvlib
    n, form = 1024, "pass"
    _, _, w, ops = _forms(G, n)[form]
    S = _Wave(G, n, "s16", False, 506)
    frm, to, mod = _rows()
    b = _batch(G, n, STREAMS, form)
    keys = _keys(n, STREAMS, 36)
    kh = keys.cpu().numpy()
    work = torch.zeros((b.track_wave_frames_work_bytes(STEPS, FRAMES, ops),), dtype=torch.uint8, device="cuda")
    out = torch.zeros((FRAMES, STREAMS * 2, w), dtype=torch.int16, device="cuda")
    d_starts, d_counts = _dev_u32(S.starts, STEPS), _dev_u32([STEPS] * STREAMS, 1)
    d_from, d_to, d_mod = _dev_u32(frm, FRAMES), _dev_u32(to, FRAMES), _dev_ur(mod)
    d_fc, d_keep = _dev_u32(FCOUNTS, 1), _dev_u32([(0, 1)] * STREAMS, 2)
    other_mod = (F32(1.0) - mod).astype(np.float32)
    moved = np.array(S.starts)
    moved[1] = [int(S.starts[1, (t * 4 + 1) % STEPS]) + t for t in range(STEPS)]
    other_keep = np.asarray([(3, 9), (BIG, 2), (1, 0)], dtype=np.uint32)
    n_mod, n_starts, n_counts, n_keep = _dev_ur(other_mod), _dev_u32(moved, STEPS), _dev_u32(COUNTS, 1), _dev_u32(other_keep, 2)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        b.track_each_wave_frames_s16(S.d_pcm, S.pitch, (d_starts, None, d_counts), STEPS, (d_from, d_to, d_mod, d_fc, d_keep), FRAMES, keys, out, work, ops,
                                     stream=s.cuda_stream)
    assert b.last_launches() == 3 and b.kernel_name() == KERNEL
    torch.cuda.synchronize()
    assert not bool(out.any()) and _same(keys.cpu().numpy(), kh)                  # captured, not run
    with torch.cuda.stream(s):
        d_mod.copy_(n_mod); d_starts.copy_(n_starts); d_counts.copy_(n_counts); d_keep.copy_(n_keep)      # in stream order, in front of the replay
        g.replay()
    torch.cuda.synchronize()
    rows = S.keyframes(COUNTS, each_starts(moved, S.pitch, n))
    wl, _ = lerp_each(kh, rows, frm, to, other_mod, COUNTS, FCOUNTS, STEPS)
    U = Oracle.texels_r16(wl.reshape(-1, n)).reshape(FRAMES, STREAMS * 2, n)
    got = out.cpu().numpy()
    for j in range(FRAMES):
        for r in (0, 3, 5):                                                       # a row of every stream
            assert _same(got[j, r], _want(G, form, n, U[j, r])), (j, r)
    assert _same(keys.cpu().numpy(), keep_each(kh, rows, other_keep, COUNTS, STEPS))
    del g
    b.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_an_fft_batch_s_state_stays(glvlib):
    import torch
    G = glvlib
    n = 256
    S = _Wave(G, n, "s16", False, 507)
    P = _Wave(G, n, "s16", True, 507)
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    mask = G.OP_WAVE | G.OP_BARS | GA
    ops = G.OP_WAVE | G.OP_BARS | G.OP_R16
    chain = G.OP_FFT | GA | G.OP_R16
    kw = dict(n=n, gl_storage=1, avg_window_kind=1, bars=n, bar_phase=0.5)
    bt, twin = G.Batch(G.Params(**kw), STREAMS, mask), G.Batch(G.Params(**kw), STREAMS, mask)
    wins = windows(S.x, n, [int(a) for a in S.starts[0, :4]])
    assert eq(seq(bt, wins[:2], chain, n, torch.int16), seq(twin, wins[:2], chain, n, torch.int16))
    frm, to, mod = _rows()
    keys = _keys(n, STREAMS, 37)
    before = keys.clone()
    d_starts, _, d_counts = S.tables(COUNTS)
    d_ur = _dev_ur(np.ones((STREAMS, STEPS), dtype=np.float32))
    tabs = (_dev_u32(frm, 0), _dev_u32(to, 0), _dev_ur(mod), _dev_u32(FCOUNTS, 0), _dev_u32(KEEP, 0))
    work = torch.zeros((bt.track_wave_frames_work_bytes(STEPS, FRAMES, ops) + 64,), dtype=torch.uint8, device="cuda")
    out = torch.zeros((FRAMES * STREAMS * 2 * n + 64,), dtype=torch.int16, device="cuda")
    L = G.lib()
    launches = bt.last_launches()
    p = lambda t: None if t is None else t if isinstance(t, int) else t.data_ptr()      # noqa: E731

    def call(b=bt, pool=False, pcm=S.d_pcm, pitch=S.pitch, spans=P.d_spans, starts=d_starts, ur=None, counts=d_counts, tb=True, steps=STEPS, frm=tabs[0], to=tabs[1],
             mod=tabs[2], fc=tabs[3], keep=tabs[4], frames=FRAMES, d_keys=keys, fe=True, d_out=out, d_work=work, ops=ops):
        t = G.TrackTables(p(starts), p(ur), p(counts))
        s = G.TrackFramesEach(p(frm), p(to), p(mod), p(fc), p(keep), frames, p(d_keys))
        tail = (C.byref(t) if tb else None, steps, C.byref(s) if fe else None, p(d_out), p(d_work), ops, None)
        if pool: return L.glv_batch_track_pool_wave_frames_s16(b._h, p(P.d_pcm) if pcm is S.d_pcm else p(pcm), P.pool_frames if pitch == S.pitch else pitch, p(spans), *tail)
        return L.glv_batch_track_each_wave_frames_s16(b._h, p(pcm), pitch, *tail)

    INVALID, STATE = G.ERR_INVALID, G.ERR_STATE
    refused = [("fe NULL", INVALID, dict(fe=False)), ("d_from NULL", INVALID, dict(frm=None)), ("d_to NULL", INVALID, dict(to=None)), ("d_mod NULL", INVALID, dict(mod=None)),
               ("d_keep NULL", INVALID, dict(keep=None)), ("d_keys NULL", INVALID, dict(d_keys=None)), ("frames 0", INVALID, dict(frames=0)),
               ("d_keys alignment", INVALID, dict(d_keys=keys.data_ptr() + 4)), ("d_from alignment", INVALID, dict(frm=tabs[0].data_ptr() + 2)),
               ("d_to alignment", INVALID, dict(to=tabs[1].data_ptr() + 1)), ("d_mod alignment", INVALID, dict(mod=tabs[2].data_ptr() + 2)),
               ("d_frame_counts alignment", INVALID, dict(fc=tabs[3].data_ptr() + 2)), ("d_keep alignment", INVALID, dict(keep=tabs[4].data_ptr() + 1)),
               # the lockstep wave frames call's, about ops and frames
               ("no WAVE", INVALID, dict(ops=G.OP_BARS | G.OP_R16)), ("an FFT chain", INVALID, dict(ops=chain)), ("rows", INVALID, dict(frames=2 ** 31 // STREAMS + 1)),
               # the per-stream call's own
               ("tb NULL", INVALID, dict(tb=False)), ("steps 0", INVALID, dict(steps=0)), ("d_starts NULL", INVALID, dict(starts=None)), ("pitch", INVALID, dict(pitch=n - 1)),
               ("d_starts alignment", INVALID, dict(starts=d_starts.data_ptr() + 2)), ("a rate table", INVALID, dict(ur=d_ur)),
               ("d_ur alignment", INVALID, dict(ur=d_ur.data_ptr() + 2)), ("d_counts alignment", INVALID, dict(counts=d_counts.data_ptr() + 1)),
               ("d_pcm NULL", INVALID, dict(pcm=None)), ("d_out NULL", INVALID, dict(d_out=None)), ("d_work NULL", INVALID, dict(d_work=None)),
               ("d_work alignment", INVALID, dict(d_work=work.data_ptr() + 64)),
               # the pool call's own
               ("d_spans NULL", INVALID, dict(pool=True, spans=None)), ("d_spans alignment", INVALID, dict(pool=True, spans=P.d_spans.data_ptr() + 8)),
               ("pool_frames", INVALID, dict(pool=True, pitch=n - 1)), ("pool: fe NULL", INVALID, dict(pool=True, fe=False)), ("pool: frames 0", INVALID, dict(pool=True, frames=0)),
               ("pool: a rate table", INVALID, dict(pool=True, ur=d_ur))]
    for bad in (G.OP_FFT, G.OP_GRAVITY, G.OP_AVERAGE, G.OP_RAW, G.OP_SMOOTH, G.OP_WRANGE, G.OP_MAGNITUDE, G.OP_OUTPUT_IS_STATE, G.OP_PRIVATE_STATE):
        refused.append(("ops 0x%x" % bad, INVALID, dict(ops=ops | bad)))
    for name, code, kw_ in refused:
        assert call(**kw_) == code, (name, L.glv_last_error().decode())
        assert L.glv_last_error().decode(), name
        assert bt.last_launches() == launches, name
    # what glv_batch_track_wave_frames_* refuses of a batch, with its codes: gl_storage 0 with bars, a creation mask without both bits, column texels, bufscale 2
    others = [G.Batch(G.Params(n=n, bars=n, bar_phase=0.5, gl_storage=0), STREAMS, G.OP_WAVE | G.OP_BARS)]
    others += [G.Batch(G.Params(n=n, gl_storage=1, bars=n, bar_phase=0.5), STREAMS, m) for m in (G.OP_WAVE, G.OP_BARS, G.OP_BARS | GA)]
    table = graph_column_texels(n, 64)[0]
    cols = G.Batch(G.Params(n=n, gl_storage=1, bars=len(table)), STREAMS, mask)
    cols.set_column_texels(table)
    scaled = G.Batch(G.Params(**kw), STREAMS, mask)
    scaled.set_bufscale(2)
    for b, o in [(b, ops) for b in others] + [(cols, ops), (cols, G.OP_WAVE | G.OP_R16), (scaled, ops), (scaled, G.OP_WAVE | G.OP_R16)]:
        was = b.last_launches()
        for pool in (False, True):
            assert call(b=b, ops=o, pool=pool) == STATE, L.glv_last_error().decode()
            assert b.last_launches() == was
    assert "glv_batch_set_bufscale" in L.glv_last_error().decode()
    for b in others + [cols, scaled]: b.close()
    # the FFT entries per stream still refuse GLV_OP_WAVE, and say where it went
    t = G.TrackTables(p(d_starts), None, None)
    s = G.TrackFramesEach(*(p(x) for x in tabs), FRAMES, p(keys))
    assert L.glv_batch_track_each_frames_s16(bt._h, p(S.d_pcm), S.pitch, C.byref(t), STEPS, C.byref(s), p(out), p(work), ops, None) == INVALID
    assert "GLV_OP_WAVE" in L.glv_last_error().decode() and "glv_batch_track_each_wave_frames_*" in L.glv_last_error().decode()
    torch.cuda.synchronize()
    assert eq(keys, before) and not bool(out.any()) and not bool(work.any())      # nothing was launched
    # a call that runs: three launches, and the FFT chain on the same batch continues exactly like an untouched twin's
    rows = (frm, to, mod, np.asarray(FCOUNTS, dtype=np.uint32), np.asarray(KEEP, dtype=np.uint32))
    got = S.call(bt, S.tables(COUNTS), rows, keys, ops, n)
    assert bt.last_launches() == 3 and bool(got.any()) and not eq(keys, before)
    assert eq(seq(bt, wins[2:], chain, n, torch.int16), seq(twin, wins[2:], chain, n, torch.int16))
    bt.close(); twin.close()
