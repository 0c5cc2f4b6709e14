"""GPU: track mode at render frames per stream (glv_batch_track_each_frames_* / glv_batch_track_pool_frames_*) on gl_storage 3 batches -- every stream with its
own rows of the frame tables, its own number of steps and of frames and its own keep pair, on the updates of the per-stream or the pool call.

Contract (include/glv_spectrum.h), everything bit for bit: a stream with c_s >= 1 steps and f_s >= 1 frames is glv_batch_track_frames_* on a ONE-stream twin
batch brought to its state by glv_batch_copy_streams, on its own recording (pool entries: its materialised span, entries pre-clamped), with steps = c_s,
frames = f_s, its rows and its keep pair; a stream with c_s = 0 lerps between its two carried keyframes (numpy float32 and the upload's quantiser); blocks at
j >= f_s are what the call's last stage makes of a zero texel row -- the block a zero keyframe gives; every index in d_from, d_to and d_keep is clamped to
c_s + 1.  The numpy restatement of the rule is tests/track_frames_each_lib.py, which tests/test_track_frames_each_host.py holds to hand-computed cases.

The shapes are tests/test_track_frames.py's: n 256 and 4096, 3 streams, 9 steps, 23 frames, F = 5 with the head off 0, batches created under
GLV_TRACK_FRAMES_SEGMENT=5 (five segments, the last one ragged; a frame count of 11 and one of 7 end inside a segment), a workspace of exactly
glv_batch_track_frames_work_bytes and an output of exactly frames * streams * 2 * w elements with a guard behind each.  The tables carry 0xFFFFFFFF entries and
the rate table NaN entries behind them: a read past a table shows as wrong bits, never as a fault."""
import ctypes as C

import numpy as np
import pytest

from glava_amd.track_starts import SPAN_DTYPE, keyframe_tables, renderer_starts, stack_frame_tables
from gpu_lib import eq
from oracle_lib import Oracle
from test_track_each import _blobs, _dev_u32, _dev_ur, _process
from test_track_frames import F, FRAMES, FROM, MOD, MODIFIED, SEGMENT, STEPS, TO, URS, _batch, _forms, _keys, _ops, _same, _want
from track_frames_each_lib import clamp_each, keep_each, lerp_each
from track_lib import GUARD, differing, out_dtype, rec

pytestmark = pytest.mark.gpu
F32 = np.float32
STREAMS = 3
COUNTS = (9, 4, 0)
FCOUNTS = (23, 11, 7)
FPS = (60, 75, 50, 144, 30, 90, 120)
KNAME = {"s16": "s16", "f32": "f32", "planar": "f32_planar"}
BIG = 0xFFFFFFFF


def _rows(streams=STREAMS):
    """[streams][FRAMES] tables, another permutation of test_track_frames' per stream"""
    frm = [FROM, FROM[::-1], FROM[5:] + FROM[:5], TO, TO[::-1], FROM[11:] + FROM[:11], TO[3:] + TO[:3]][:streams]
    to = [TO, TO[::-1], TO[5:] + TO[:5], FROM, FROM[::-1], TO[7:] + TO[:7], FROM[3:] + FROM[:3]][:streams]
    mod = [MOD, MOD[::-1], MOD[9:] + MOD[:9], MOD[2:] + MOD[:2], MOD[::-1], MOD, MOD[4:] + MOD[:4]][:streams]
    return np.asarray(frm, dtype=np.uint32), np.asarray(to, dtype=np.uint32), np.asarray(mod, dtype=np.float32)


def _layout(x, kind):
    """host [streams][frames][2] in the layout of its kind: planar is [streams][2][frames]"""
    return np.ascontiguousarray(np.transpose(x, (0, 2, 1))) if kind == "planar" else np.ascontiguousarray(x)


def _device(a, kind, tail):
    """`a` on the device, one frame (planar: one float) behind a load boundary, `tail` elements of another pattern behind it"""
    import torch
    flat = torch.full((a.size + tail + 8,), 3, dtype=torch.int16 if kind == "s16" else torch.float32, device="cuda")
    off = 1 if kind == "planar" else 2
    view = flat[off:off + a.size]
    view.copy_(torch.from_numpy(np.array(a, copy=True).reshape(-1)))
    return view.view(a.shape)


class _Each:
    """recordings (or a pool and spans), per-stream window starts and rates, and the calls on them"""

    def __init__(self, G, n, kind, pool, seed, streams=STREAMS, steps=STEPS):
        self.G, self.n, self.kind, self.pool, self.streams, self.steps = G, n, kind, pool, streams, steps
        f32 = kind != "s16"
        self.starts = np.asarray([renderer_starts(22050, FPS[s], 1, steps) for s in range(streams)], dtype=np.uint32)       # another display rate per stream
        self.urs = np.asarray([np.roll(URS, s)[:steps] for s in range(streams)], dtype=np.float32)
        longest = int(self.starts.max()) + n + 38
        if pool:
            # streams 0 and 1 on ONE span at different frame rates, stream 2 nested in it off a group of 8 frames and short enough that its late entries clamp
            assert streams == 3
            a = (16, longest)
            self.spans = [a, a, (a[0] + 257, int(self.starts[2, 5]) + n)]
            self.pool_frames = (a[0] + a[1] + 45) | 1
            x = rec(seed, 1, self.pool_frames, f32)[0]                             # [pool_frames][2]
            body = np.ascontiguousarray(x.T) if kind == "planar" else x
            self.d_pcm = _device(body, kind, 2 * n)
            self.d_spans = self._dev_spans()
            self.one_host = [x[None, first:first + frames] for first, frames in self.spans]
            self.twin_starts = np.asarray([[min(int(e), fr - n) for e in row] for row, (_, fr) in zip(self.starts, self.spans)], dtype=np.uint32)
            assert (self.twin_starts[2] != self.starts[2]).any() and (self.twin_starts[:2] == self.starts[:2]).all()
        else:
            self.pitch = longest | 1
            x = rec(seed, streams, self.pitch, f32)
            self.d_pcm = _device(_layout(x, kind), kind, 2 * n)
            self.one_host = [x[s:s + 1] for s in range(streams)]
            self.twin_starts = self.starts
        self.warm = _layout(rec(seed + 1, streams, n + 64, f32), kind)

    def _dev_spans(self):
        import torch
        a = np.zeros((len(self.spans) + 1,), dtype=np.dtype(SPAN_DTYPE))
        for s, (first, frames) in enumerate(self.spans):
            a[s] = (first, frames, 0xDEADBEEF)
        a[-1] = (0xFFFFFFFFFFFFFFF0, 0xFFFFFFFF, 0)
        t = torch.from_numpy(a.view(np.int32).copy()).cuda()
        assert t.data_ptr() % 16 == 0
        return t

    def window(self, start, s=None):
        import torch
        sel = slice(None) if s is None else slice(s, s + 1)
        w = self.warm[sel, :, start:start + self.n] if self.kind == "planar" else self.warm[sel, start:start + self.n, :]
        return torch.from_numpy(np.ascontiguousarray(w)).cuda()

    def warm_up(self, batches, ops, w):
        """three updates of every stream: the head off 0, state in every stream, the same in every batch given"""
        for start in (3, 11, 29):
            for b in batches: _process(b, self.kind, self.window(start), ops, w, out_dtype(self.G, ops))

    def twins(self, b, form):
        """a one-stream twin per stream, at the stream's state"""
        import torch
        out = []
        for s in range(self.streams):
            t = _batch(self.G, self.n, 1, form)
            t.copy_streams(_dev_u32([0], 0), b, _dev_u32([s], 0), 1)
            out.append(t)
        torch.cuda.synchronize()
        return out

    def tables(self, counts, starts=None, urs=None, steps=None):
        steps = self.steps if steps is None else steps
        starts = self.starts if starts is None else starts
        urs = self.urs if urs is None else urs
        return (_dev_u32(starts, steps), _dev_ur(urs), _dev_u32(counts, 1) if counts is not None else None)

    def call(self, b, tables, frame_rows, keys, ops, w, steps=None, stream=None, sync=True):
        """one per-stream frames call: frame_rows = (from, to, mod, frame_counts or None, keep) in numpy; [frames][units][w]"""
        import torch
        steps = self.steps if steps is None else steps
        frm, to, mod, fcounts, keep = frame_rows
        frames = frm.shape[1]
        dev = (_dev_u32(frm, frames), _dev_u32(to, frames), _dev_ur(mod), _dev_u32(fcounts, 1) if fcounts is not None else None, _dev_u32(keep, 2))
        dt = out_dtype(self.G, ops)
        nbytes = b.track_frames_work_bytes(steps, frames, ops)
        work = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        assert work.data_ptr() % 256 == 0
        count = frames * self.streams * 2 * w
        fill = 23130 if dt == torch.int16 else -7.0
        flat = torch.full((count + GUARD,), fill, dtype=dt, device="cuda")       # (the output too: a row the call leaves stale shows)
        name = ("track_pool_frames_" if self.pool else "track_each_frames_") + KNAME[self.kind]
        if self.pool: head = [self.d_pcm, self.pool_frames, self.d_spans]
        else: head = [self.d_pcm] if self.kind == "planar" else [self.d_pcm, self.pitch]
        getattr(b, name)(*head, tables, steps, dev, frames, keys, flat, work, ops, stream=stream)
        self.held = (dev, tables, flat, work)
        if sync:
            torch.cuda.synchronize()
            assert bool((work[nbytes:] == 0xA5).all()), "the call wrote behind the workspace it asked for"
            assert bool((flat[count:] == fill).all()), "the call wrote behind its output"
        return flat[:count].view(frames, self.streams * 2, w)

    def lockstep(self, t, s, c, frm, to, mod, keys, keep, ops, w, rates=True):
        """glv_batch_track_frames_* on the one-stream batch `t` over stream s's recording and the first c entries of its rows: [frames][2][w]"""
        import torch
        frames = len(frm)
        host = _layout(self.one_host[s], self.kind)
        d_rec = _device(host, self.kind, 2 * self.n)
        pitch = self.one_host[s].shape[1]
        dt = out_dtype(self.G, ops)
        nbytes = t.track_frames_work_bytes(c, frames, ops)
        work = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        count = frames * 2 * w
        flat = torch.zeros((count + GUARD,), dtype=dt, device="cuda")
        d_starts, d_ur = _dev_u32(self.twin_starts[s, :c], 0), (_dev_ur(self.urs[s, :c]) if rates else None)
        tabs = (_dev_u32(frm, 0), _dev_u32(to, 0), _dev_ur(mod))
        head = [d_rec] if self.kind == "planar" else [d_rec, pitch]
        getattr(t, "track_frames_" + KNAME[self.kind])(*head, d_starts, d_ur, c, *tabs, frames, keys, keep, flat, work, ops)
        torch.cuda.synchronize()
        assert bool((work[nbytes:] == 0xA5).all()) and not bool(flat[count:].any())
        return flat[:count].view(frames, 2, w)

    def rates_call(self, t, s, c, ops, w):
        """glv_batch_track_rates_* on the one-stream batch `t`: stream s's first c updates and nothing else"""
        import torch
        d_rec = _device(_layout(self.one_host[s], self.kind), self.kind, 2 * self.n)
        out = torch.zeros((c, 2, w), dtype=out_dtype(self.G, ops), device="cuda")
        work = torch.zeros((t.track_at_work_bytes(c, ops),), dtype=torch.uint8, device="cuda")
        head = [d_rec] if self.kind == "planar" else [d_rec, self.one_host[s].shape[1]]
        getattr(t, "track_rates_" + KNAME[self.kind])(*head, _dev_u32(self.twin_starts[s, :c], 0), _dev_ur(self.urs[s, :c]), c, out, work, ops)
        torch.cuda.synchronize()

    def float_rows(self, counts):
        """float32 [steps][units][n]: every step's finished float rows from a gl_storage 0 twin of the whole batch (zeros behind a stream's count), head off 0 alike"""
        import torch
        G = self.G
        b = _batch(G, self.n, self.streams, "texels", storage=0)
        ops = G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE
        self.warm_up([b], ops, self.n)
        out = torch.zeros((self.steps, self.streams * 2, self.n), dtype=torch.float32, device="cuda")
        work = torch.zeros((b.track_at_work_bytes(self.steps, ops),), dtype=torch.uint8, device="cuda")
        name = ("track_pool_" if self.pool else "track_each_") + KNAME[self.kind]
        if self.pool: head = [self.d_pcm, self.pool_frames, self.d_spans]
        else: head = [self.d_pcm] if self.kind == "planar" else [self.d_pcm, self.pitch]
        getattr(b, name)(*head, *self.tables(counts), self.steps, out, work, ops)
        torch.cuda.synchronize()
        b.close()
        return out.cpu().numpy()


def _zero_block(G, n, form, ops, w):
    """what the call's last stage makes of a zero texel row, [w]: the block a zero keyframe gives (from == to == 0 over zeroed d_keys on a one-stream batch)"""
    S = _Each(G, n, "s16", False, 77, streams=1, steps=1)
    t = _batch(G, n, 1, form)
    got = S.lockstep(t, 0, 1, [0], [0], [0.0], _keys(n, 1), (0, 1), ops, w)
    t.close()
    assert eq(got[0, 0], got[0, 1])
    return got[0, 0].clone()


def _launches(form):
    return 2 + 2 + (0 if form == "texels" else 1)      # the per-stream call's transform and scan, the frames and the write-back, the bars


def _state_is_the_twins(S, b, twins, ops, w, what):
    """the portable blobs, then one more update of everything"""
    dt = out_dtype(S.G, ops)
    mine = _blobs(b)
    for s, t in enumerate(twins):
        assert bool((mine[s] == _blobs(t)[0]).all()), (*what, s, "blob")
    more = _process(b, S.kind, S.window(17), ops, w, dt)
    for s, t in enumerate(twins):
        assert eq(more[2 * s:2 * s + 2], _process(t, S.kind, S.window(17, s), ops, w, dt)), (*what, s, "next update")


# ---- 1. equal rows, NULL counts, equal keep pairs: the lockstep call ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,kind,n", [("texels", "s16", 256), ("pass", "s16", 4096), ("texels", "f32", 4096), ("bar", "f32", 256), ("pass", "planar", 256),
                                         ("texels", "planar", 4096)])
def test_equal_rows_null_counts_and_equal_keep_pairs_are_the_lockstep_call(glvlib, form, kind, n):
    import torch
    G = glvlib
    _, _, w, r16 = _forms(n)[form]
    ops = _ops(G, form, r16)
    S = _Each(G, n, kind, False, 401)
    row, ur = S.starts[1], S.urs[2]
    be, bl = _batch(G, n, STREAMS, form), _batch(G, n, STREAMS, form)
    S.warm_up([be, bl], ops, w)
    ke, kl = _keys(n, STREAMS, 21), _keys(n, STREAMS, 21)
    tile = lambda v, dt: np.tile(np.asarray(v, dtype=dt), (STREAMS, 1))           # noqa: E731
    got = S.call(be, S.tables(None, tile(row, np.uint32), tile(ur, np.float32)), (tile(FROM, np.uint32), tile(TO, np.uint32), tile(MOD, np.float32), None, tile((9, 10), np.uint32)),
                 ke, ops, w)
    assert be.last_launches() == _launches(form) and be.kernel_name() == "glv_track_frames_each_kernel", (be.last_launches(), be.kernel_name())
    # the existing entry on the same batch state, one row of every table for all
    dt = out_dtype(G, ops)
    work = torch.zeros((bl.track_frames_work_bytes(STEPS, FRAMES, ops),), dtype=torch.uint8, device="cuda")
    want = torch.zeros((FRAMES, STREAMS * 2, w), dtype=dt, device="cuda")
    head = [S.d_pcm] if kind == "planar" else [S.d_pcm, S.pitch]
    getattr(bl, "track_frames_" + KNAME[kind])(*head, _dev_u32(row, 0), _dev_ur(ur), STEPS, _dev_u32(FROM, 0), _dev_u32(TO, 0), _dev_ur(MOD), FRAMES, kl, (9, 10), want, work, ops)
    torch.cuda.synchronize()
    assert bl.last_launches() == be.last_launches() and bl.kernel_name() == "glv_track_frames_kernel"
    assert eq(got, want), differing(got, want)
    assert eq(ke, kl)
    assert bool((_blobs(be) == _blobs(bl)).all())
    win = S.window(17)
    assert eq(_process(be, kind, win, ops, w, dt), _process(bl, kind, win, ops, w, dt)), "next update"
    be.close(); bl.close()


# ---- 2. different rows per stream ----------------------------------------------------------------------------------------------------------------------------------
KEEP = ((9, 10), (1, 5), (0, 1))                                                  # pairs the host accepts for steps = c_s: (k, k'), (1, k), (0, 1)
CASES = [("texels", "s16", 256, False), ("texels", "f32", 4096, False), ("texels", "planar", 256, False), ("pass", "s16", 4096, False), ("bar", "f32", 256, False),
         ("col", "s16", 4096, False), ("maximum", "planar", 256, False), ("pass", "planar", 4096, False),
         ("texels", "s16", 4096, True), ("pass", "f32", 256, True), ("bar", "planar", 4096, True), ("texels", "planar", 256, True), ("maximum", "s16", 256, True),
         ("col", "f32", 256, True)]


@pytest.mark.parametrize("form,kind,n,pool", CASES, ids=["%s-%s-n%d%s" % (f, k, n, "-pool" if p else "") for f, k, n, p in CASES])
def test_every_stream_is_its_one_stream_twin(glvlib, oracle, form, kind, n, pool):
    G = glvlib
    _, _, w, r16 = _forms(n)[form]
    ops = _ops(G, form, r16)
    S = _Each(G, n, kind, pool, 402)
    frm, to, mod = _rows()
    b = _batch(G, n, STREAMS, form)
    S.warm_up([b], ops, w)
    twins = S.twins(b, form)
    keys = _keys(n, STREAMS, 22)
    k_before = keys.clone()
    got = S.call(b, S.tables(COUNTS), (frm, to, mod, np.asarray(FCOUNTS, dtype=np.uint32), np.asarray(KEEP, dtype=np.uint32)), keys, ops, w)
    assert b.last_launches() == _launches(form) and b.kernel_name() == "glv_track_frames_each_kernel", (b.last_launches(), b.kernel_name())
    zero = _zero_block(G, n, form, ops, w)
    for s in range(STREAMS):
        c, f = COUNTS[s], FCOUNTS[s]
        mine, mine_keys = got[:, 2 * s:2 * s + 2], keys[:, 2 * s:2 * s + 2]
        if c >= 1:                                                                # no stream with steps is skipped
            tk = k_before[:, 2 * s:2 * s + 2].contiguous().clone()
            assert tk.is_contiguous() and tk.data_ptr() % 16 == 0
            want = S.lockstep(twins[s], s, c, frm[s, :f], to[s, :f], mod[s, :f], tk, KEEP[s], ops, w)
            assert eq(mine[:f], want), (form, s, differing(mine[:f], want))
            assert eq(mine_keys, tk), (form, s, "keys")
        else:                                                                     # numpy float32 and unorm16: the two carried keyframes only
            kh = k_before.cpu().numpy()
            wl, shown = lerp_each(kh, np.zeros((STEPS,) + kh.shape[1:], F32), frm, to, mod, COUNTS, FCOUNTS, STEPS)
            assert shown[:f, s].all() and not shown[f:, s].any() and int(clamp_each(frm, COUNTS, STEPS)[s].max()) == 1
            U = Oracle.texels_r16(wl[:f, 2 * s:2 * s + 2].reshape(-1, n)).reshape(f, 2, n)
            g = mine[:f].cpu().numpy()
            if form == "texels": assert _same(g, U), (form, s)                    # GLV_OP_R16 alone: every frame, row and bin
            else:
                for j in (0, f - 1): assert _same(g[j, 1], _want(G, form, n, U[j, 1])), (form, s, j)
            assert eq(mine_keys, k_before[:, 2 * s:2 * s + 2]), (form, s, "keep (0, 1)")
        for j in range(f, FRAMES):
            for ch in range(2): assert eq(mine[j, ch], zero), (form, s, j, "a frame behind the count")
    _state_is_the_twins(S, b, twins, ops, w, (form, kind))
    for t in twins: t.close()
    b.close()


# ---- 3. indices beyond c_s + 1 ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,kind,n,pool", [("texels", "s16", 256, False), ("bar", "f32", 4096, False), ("texels", "planar", 4096, True)])
def test_indices_beyond_a_stream_s_last_keyframe_are_clamped_to_its_own_count(glvlib, form, kind, n, pool):
    """0xFFFFFFFF, and c_s + 2: on the stream with 4 of 9 steps that is keyframe 6, the row of step 4 -- valid for the batch, a zero row the scan wrote behind the
    stream's count.  Against the same call with tables clamped on the host (the kernel's own clamp then binds nowhere), and for the texels form against numpy."""
    G = glvlib
    _, _, w, r16 = _forms(n)[form]
    ops = _ops(G, form, r16)
    S = _Each(G, n, kind, pool, 403)
    frm, to, mod = _rows()
    counts = np.asarray(COUNTS)
    for s in range(STREAMS):
        frm[s, 0::3] = [BIG, counts[s] + 2] * 4; to[s, 1::4] = [counts[s] + 2, BIG, 1000, 2 ** 31, counts[s] + 2, BIG]
    keep = np.asarray([(BIG, 11), (6, BIG), (2, 3)], dtype=np.uint32)
    cf, ct, ck = (clamp_each(t, counts, STEPS).astype(np.uint32) for t in (frm, to, keep))
    assert (cf != frm).any() and (ct != to).any() and ck.tolist() == [[10, 10], [5, 5], [1, 1]]
    assert 6 in frm[1] and 6 in to[1]
    ba, bb = _batch(G, n, STREAMS, form), _batch(G, n, STREAMS, form)
    S.warm_up([ba, bb], ops, w)
    ka, kb = _keys(n, STREAMS, 23), _keys(n, STREAMS, 23)
    k_before = ka.cpu().numpy()
    got = S.call(ba, S.tables(COUNTS), (frm, to, mod, None, keep), ka, ops, w)
    want = S.call(bb, S.tables(COUNTS), (cf, ct, mod, None, ck), kb, ops, w)
    assert eq(got, want), differing(got, want)
    assert eq(ka, kb)
    rows = S.float_rows(COUNTS)
    assert not rows[4:, 2:4].any() and rows[3, 2:4].any()                         # the zero rows behind stream 1's count, which no frame and no keep pair may show
    assert _same(ka.cpu().numpy(), keep_each(k_before, rows, keep, counts, STEPS))
    if form == "texels":
        wl, _ = lerp_each(k_before, rows, frm, to, mod, counts, None, STEPS)
        assert _same(got.cpu().numpy(), Oracle.texels_r16(wl.reshape(-1, n)).reshape(FRAMES, STREAMS * 2, n))
    ba.close(); bb.close()


# ---- 4. keep pairs, and a session cut in two -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [((0, 1), (1, 4), (3, 7)), ((1, 0), (5, 2), (9, 9)), ((10, 2), (0, 0), (1, 1))], ids=["host-pairs", "swapped", "any"])
def test_keep_pairs_per_stream(glvlib, keep):
    """(0, 1) leaves a stream's keys, (1, k) and (k, k') as the lockstep call, and pairs the host's rule would refuse -- swapped, equal, backwards: a lane reads
    element i of both before it writes element i of either"""
    G = glvlib
    n, form = 256, "texels"
    ops = _ops(G, form, True)
    S = _Each(G, n, "s16", False, 404)
    counts = (9, 5, 9)
    frm, to, mod = _rows()
    b = _batch(G, n, STREAMS, form)
    S.warm_up([b], ops, n)
    keys = _keys(n, STREAMS, 24)
    k_before = keys.cpu().numpy()
    S.call(b, S.tables(counts), (frm, to, mod, None, np.asarray(keep, dtype=np.uint32)), keys, ops, n)
    rows = S.float_rows(counts)
    assert _same(keys.cpu().numpy(), keep_each(k_before, rows, keep, counts, STEPS))
    if keep[0] == (0, 1): assert _same(keys[:, 0:2].cpu().numpy(), k_before[:, 0:2])
    b.close()


@pytest.mark.parametrize("form,kind,pool", [("texels", "s16", False), ("pass", "f32", False), ("texels", "planar", True)])
def test_a_session_cut_in_two_at_another_frame_per_stream_is_the_uncut_call(glvlib, form, kind, pool):
    """stream s takes 3 + s of its 9 steps in the first call and the rest in the second; its frames are cut at the frame that runs its step 3 + s"""
    import torch
    G = glvlib
    n = 256
    _, _, w, r16 = _forms(n)[form]
    ops = _ops(G, form, r16)
    S = _Each(G, n, kind, pool, 405)
    on, uratio = [True] * FRAMES, [0.4] * FRAMES
    first_steps = [3, 4, 5]
    cuts = [[j for j, m in enumerate(MODIFIED) if m][c] for c in first_steps]
    assert len(set(cuts)) == 3
    whole = stack_frame_tables([keyframe_tables(MODIFIED, on, uratio)] * STREAMS)
    a_rows, b_rows = [], []
    for cut in cuts:
        idle = cut - 1 - max(j for j in range(cut) if MODIFIED[j])
        a_rows.append(keyframe_tables(MODIFIED[:cut], on[:cut], uratio[:cut]))
        b_rows.append(keyframe_tables(MODIFIED[cut:], on[cut:], uratio[cut:], kcounter=idle))
    part_a, part_b = stack_frame_tables(a_rows), stack_frame_tables(b_rows)
    assert part_a[3].tolist() == cuts and part_b[3].tolist() == [FRAMES - c for c in cuts] and part_a[4].tolist() != [list(part_a[4][0])] * 3
    sa, sb = max(first_steps), STEPS - min(first_steps)
    pad = lambda rows, steps: np.asarray([list(r) + [r[-1]] * (steps - len(r)) for r in rows])      # noqa: E731
    tab_a = S.tables(first_steps, pad([S.starts[s, :c] for s, c in enumerate(first_steps)], sa).astype(np.uint32),
                     pad([S.urs[s, :c] for s, c in enumerate(first_steps)], sa).astype(np.float32), sa)
    tab_b = S.tables([STEPS - c for c in first_steps], pad([S.starts[s, c:] for s, c in enumerate(first_steps)], sb).astype(np.uint32),
                     pad([S.urs[s, c:] for s, c in enumerate(first_steps)], sb).astype(np.float32), sb)
    bw, bc = _batch(G, n, STREAMS, form), _batch(G, n, STREAMS, form)
    S.warm_up([bw, bc], ops, w)
    kw_, kc = _keys(n, STREAMS, 25), _keys(n, STREAMS, 25)
    want = S.call(bw, S.tables(None), whole, kw_, ops, w)
    a = S.call(bc, tab_a, part_a, kc, ops, w, steps=sa)
    b = S.call(bc, tab_b, part_b, kc, ops, w, steps=sb)
    for s, cut in enumerate(cuts):
        r = slice(2 * s, 2 * s + 2)
        assert eq(a[:cut, r], want[:cut, r]) and eq(b[:FRAMES - cut, r], want[cut:, r]), (form, s)
    assert eq(kc, kw_)
    assert bool((_blobs(bc) == _blobs(bw)).all())
    win = S.window(17)
    dt = out_dtype(G, ops)
    assert eq(_process(bc, kind, win, ops, w, dt), _process(bw, kind, win, ops, w, dt)), "next update"
    torch.cuda.synchronize()
    bw.close(); bc.close()


# ---- 5. a frame count of 0 ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["texels", "pass"])
def test_a_stream_without_frames_keeps_its_keys_and_advances_by_its_steps(glvlib, form):
    G = glvlib
    n, kind = 256, "s16"
    _, _, w, r16 = _forms(n)[form]
    ops = _ops(G, form, r16)
    S = _Each(G, n, kind, False, 406)
    counts, fcounts = (9, 4, 2), (23, 0, 7)
    frm, to, mod = _rows()
    b = _batch(G, n, STREAMS, form)
    S.warm_up([b], ops, w)
    twins = S.twins(b, form)
    keys = _keys(n, STREAMS, 26)
    before = keys.clone()
    got = S.call(b, S.tables(counts), (frm, to, mod, np.asarray(fcounts, dtype=np.uint32), np.asarray([(9, 10), (0, 1), (1, 3)], dtype=np.uint32)), keys, ops, w)
    zero = _zero_block(G, n, form, ops, w)
    for j in range(FRAMES):
        for ch in (2, 3): assert eq(got[j, ch], zero), j                          # defined: the block a zero keyframe gives
    assert eq(keys[:, 2:4], before[:, 2:4])                                       # keep (0, 1)
    assert not eq(keys[:, 0:2], before[:, 0:2]) and not eq(keys[:, 4:6], before[:, 4:6])
    for s in range(STREAMS): S.rates_call(twins[s], s, counts[s], ops, w)         # the updates alone
    _state_is_the_twins(S, b, twins, ops, w, (form,))
    for t in twins: t.close()
    b.close()


# ---- 6. launch caps ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_more_work_items_than_the_grid_has_workgroups(glvlib, oracle):
    """n = 256, seven streams, segments of one frame: 14 * 601 work items of the frames kernel against its 8192 workgroups (glv_track_frames.hip kFramesGridCap) --
    the grid loops, over streams with ragged frame counts and step counts"""
    G = glvlib
    n, streams, frames = 256, 7, 601
    assert 2 * streams * frames > 256 * 32
    S = _Each(G, n, "s16", False, 407, streams=streams)
    counts = [9, 4, 0, 7, 1, 9, 3]
    fcounts = [601, 590, 1, 0, 333, 600, 64]
    rng = np.random.default_rng(19)
    frm = rng.integers(0, STEPS + 3, (streams, frames)).astype(np.uint32)
    to = rng.integers(0, STEPS + 3, (streams, frames)).astype(np.uint32)
    mod = rng.random((streams, frames), dtype=np.float32)
    keep = np.asarray([(c + 1, c // 2) for c in counts], dtype=np.uint32)
    b = _batch(G, n, streams, "texels", segment=1)
    ops = _ops(G, "texels", True)
    S.warm_up([b], ops, n)
    keys = _keys(n, streams, 27)
    k_before = keys.cpu().numpy()
    got = S.call(b, S.tables(counts), (frm, to, mod, np.asarray(fcounts, dtype=np.uint32), keep), keys, ops, n).cpu().numpy()
    rows = S.float_rows(counts)
    sample = sorted({0, 1, 2, 63, 64, 332, 333, 584, 585, 586, 589, 590, 599, 600} | {int(v) for v in rng.integers(0, frames, 30)})
    pick = lambda t: t[:, sample]                                                 # noqa: E731
    fc = [sum(1 for j in sample if j < f) for f in fcounts]
    wl, shown = lerp_each(k_before, rows, pick(frm), pick(to), pick(mod), counts, fc, STEPS)
    U = Oracle.texels_r16(wl.reshape(-1, n)).reshape(len(sample), streams * 2, n)
    for i, j in enumerate(sample):
        for s in range(streams):
            assert bool(shown[i, s]) == (j < fcounts[s])
            assert _same(got[j, 2 * s:2 * s + 2], U[i, 2 * s:2 * s + 2]), (j, s)     # (a frame not shown: zero texels, which U holds for w = 0)
    assert _same(keys.cpu().numpy(), keep_each(k_before, rows, keep, counts, STEPS))
    b.close()


# ---- 7. graph capture -------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_captured_call_replayed_after_rewriting_d_mod_d_frame_counts_and_d_keep(glvlib, oracle):
    """kernels only: the first per-stream frames call of a batch can be captured; tables, counts and keep pairs are read when the kernels run"""
    import torch
    G = glvlib
    n, form = 4096, "texels"
    ops = _ops(G, form, True)
    S = _Each(G, n, "s16", False, 408)
    frm, to, mod = _rows()
    b = _batch(G, n, STREAMS, form)
    keys = _keys(n, STREAMS, 28)
    k_before = keys.cpu().numpy()
    work = torch.zeros((b.track_frames_work_bytes(STEPS, FRAMES, ops),), dtype=torch.uint8, device="cuda")
    out = torch.zeros((FRAMES, STREAMS * 2, n), dtype=torch.int16, device="cuda")
    tables = S.tables(COUNTS)
    d_from, d_to, d_mod = _dev_u32(frm, FRAMES), _dev_u32(to, FRAMES), _dev_ur(mod)
    d_fc, d_keep = _dev_u32([FRAMES] * STREAMS, 1), _dev_u32([(0, 1)] * STREAMS, 2)
    other_mod = (F32(1.0) - mod).astype(np.float32)
    other_fc, other_keep = np.asarray(FCOUNTS, dtype=np.uint32), np.asarray([(3, 9), (BIG, 2), (1, 0)], dtype=np.uint32)
    n_mod, n_fc, n_keep = _dev_ur(other_mod), _dev_u32(other_fc, 1), _dev_u32(other_keep, 2)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        b.track_each_frames_s16(S.d_pcm, S.pitch, tables, STEPS, (d_from, d_to, d_mod, d_fc, d_keep), FRAMES, keys, out, work, ops, stream=s.cuda_stream)
    assert b.last_launches() == 4 and b.kernel_name() == "glv_track_frames_each_kernel"
    torch.cuda.synchronize()
    assert not bool(out.any()) and _same(keys.cpu().numpy(), k_before)             # captured, not run
    with torch.cuda.stream(s):
        d_mod.copy_(n_mod); d_fc.copy_(n_fc); d_keep.copy_(n_keep)                # in stream order, in front of the replay
        g.replay()
    torch.cuda.synchronize()
    b0 = _batch(G, n, STREAMS, "texels", storage=0)                               # the float rows of a batch that starts from zero state, as the captured one did
    o = torch.zeros((STEPS, STREAMS * 2, n), dtype=torch.float32, device="cuda")
    f_ops = G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE
    b0.track_each_s16(S.d_pcm, S.pitch, *S.tables(COUNTS), STEPS, o, torch.zeros((b0.track_at_work_bytes(STEPS, f_ops),), dtype=torch.uint8, device="cuda"), f_ops)
    torch.cuda.synchronize()
    rows = o.cpu().numpy()
    b0.close()
    wl, _ = lerp_each(k_before, rows, frm, to, other_mod, COUNTS, other_fc, STEPS)
    assert _same(out.cpu().numpy(), Oracle.texels_r16(wl.reshape(-1, n)).reshape(FRAMES, STREAMS * 2, n))
    assert _same(keys.cpu().numpy(), keep_each(k_before, rows, other_keep, COUNTS, STEPS))
    del g
    b.close()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_batch_as_it_was(glvlib):
    import torch
    G = glvlib
    n, form = 256, "pass"
    _, _, w, r16 = _forms(n)[form]
    ops = _ops(G, form, r16)
    S = _Each(G, n, "s16", False, 409)
    P = _Each(G, n, "s16", True, 409)
    frm, to, mod = _rows()
    bt, bs = _batch(G, n, STREAMS, form), _batch(G, n, STREAMS, form)
    S.warm_up([bt, bs], ops, w)
    blob = _blobs(bt).clone()
    keys = _keys(n, STREAMS, 29)
    before = keys.clone()
    d_starts, d_ur, d_counts = S.tables(COUNTS)
    tabs = (_dev_u32(frm, 0), _dev_u32(to, 0), _dev_ur(mod), _dev_u32(FCOUNTS, 0), _dev_u32(KEEP, 0))
    work = torch.zeros((bt.track_frames_work_bytes(STEPS, FRAMES, ops) + 64,), dtype=torch.uint8, device="cuda")
    out = torch.zeros((FRAMES * STREAMS * 2 * w + 64,), dtype=torch.int16, device="cuda")
    L = G.lib()
    p = lambda t: None if t is None else t if isinstance(t, int) else t.data_ptr()      # noqa: E731

    def call(b=bt, pool=False, pcm=S.d_pcm, pitch=S.pitch, spans=P.d_spans, starts=d_starts, ur=d_ur, counts=d_counts, tb=True, steps=STEPS, frm=tabs[0], to=tabs[1],
             mod=tabs[2], fc=tabs[3], keep=tabs[4], frames=FRAMES, d_keys=keys, fe=True, d_out=out, d_work=work, ops=ops):
        t = G.TrackTables(p(starts), p(ur), p(counts))
        s = G.TrackFramesEach(p(frm), p(to), p(mod), p(fc), p(keep), frames, p(d_keys))
        tail = (C.byref(t) if tb else None, steps, C.byref(s) if fe else None, p(d_out), p(d_work), ops, None)
        if pool: return L.glv_batch_track_pool_frames_s16(b._h, p(P.d_pcm) if pcm is S.d_pcm else p(pcm), P.pool_frames if pitch == S.pitch else pitch, p(spans), *tail)
        return L.glv_batch_track_each_frames_s16(b._h, p(pcm), pitch, *tail)

    INVALID, STATE = G.ERR_INVALID, G.ERR_STATE
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    refused = [("fe NULL", INVALID, dict(fe=False)), ("d_from NULL", INVALID, dict(frm=None)), ("d_to NULL", INVALID, dict(to=None)), ("d_mod NULL", INVALID, dict(mod=None)),
               ("d_keep NULL", INVALID, dict(keep=None)), ("d_keys NULL", INVALID, dict(d_keys=None)), ("frames 0", INVALID, dict(frames=0)),
               ("d_keys alignment", INVALID, dict(d_keys=keys.data_ptr() + 4)), ("d_from alignment", INVALID, dict(frm=tabs[0].data_ptr() + 2)),
               ("d_to alignment", INVALID, dict(to=tabs[1].data_ptr() + 1)), ("d_mod alignment", INVALID, dict(mod=tabs[2].data_ptr() + 2)),
               ("d_frame_counts alignment", INVALID, dict(fc=tabs[3].data_ptr() + 2)), ("d_keep alignment", INVALID, dict(keep=tabs[4].data_ptr() + 1)),
               # the lockstep frames call's, about ops and frames
               ("no R16 or BARS", INVALID, dict(ops=G.OP_FFT | GA)), ("WAVE", INVALID, dict(ops=G.OP_WAVE | G.OP_R16, ur=None, counts=None)),
               ("rows", INVALID, dict(frames=2 ** 31 // STREAMS + 1)),
               # the per-stream call's own
               ("tb NULL", INVALID, dict(tb=False)), ("steps 0", INVALID, dict(steps=0)), ("d_starts NULL", INVALID, dict(starts=None)), ("pitch", INVALID, dict(pitch=n - 1)),
               ("d_starts alignment", INVALID, dict(starts=d_starts.data_ptr() + 2)), ("d_ur alignment", INVALID, dict(ur=d_ur.data_ptr() + 2)),
               ("d_counts alignment", INVALID, dict(counts=d_counts.data_ptr() + 1)), ("rates without gravity", INVALID, dict(ops=G.OP_FFT | G.OP_AVERAGE | G.OP_BARS | G.OP_R16)),
               ("counts without state", INVALID, dict(ops=G.OP_FFT | G.OP_R16, ur=None)),
               ("d_pcm NULL", INVALID, dict(pcm=None)), ("d_out NULL", INVALID, dict(d_out=None)), ("d_work alignment", INVALID, dict(d_work=work.data_ptr() + 64)),
               ("RAW", INVALID, dict(ops=ops | G.OP_RAW)),
               # the pool call's own
               ("d_spans NULL", INVALID, dict(pool=True, spans=None)), ("d_spans alignment", INVALID, dict(pool=True, spans=P.d_spans.data_ptr() + 8)),
               ("pool_frames", INVALID, dict(pool=True, pitch=n - 1)), ("pool: fe NULL", INVALID, dict(pool=True, fe=False)), ("pool: frames 0", INVALID, dict(pool=True, frames=0))]
    for name, code, kw in refused:
        assert call(**kw) == code, (name, L.glv_last_error().decode())
        assert L.glv_last_error().decode(), name
    # any gl_storage but 3, and state the batch was not created with
    for storage in (0, 1):
        other = G.Batch(G.Params(n=n, avg_frames=F, gl_storage=storage, bars=n, bar_phase=0.5), STREAMS, GA | G.OP_BARS)
        assert call(b=other, ops=G.OP_FFT | GA | G.OP_R16) == STATE, storage
        other.close()
    gravity_only = G.Batch(G.Params(n=n, avg_frames=F, gl_storage=G.GL_STORAGE_UPLOAD, bars=n, bar_phase=0.5), STREAMS, G.OP_GRAVITY | G.OP_BARS)
    assert call(b=gravity_only) == STATE
    gravity_only.close()
    torch.cuda.synchronize()
    assert eq(keys, before) and not bool(out.any()) and not bool(work.any())      # nothing was launched
    assert bool((_blobs(bt) == blob).all())                                       # the state blob as it was
    # ... and the batch is where a batch that saw none of it is: output, keyframes and state agree, through the pool call too
    k2 = before.clone()
    rows = (frm, to, mod, np.asarray(FCOUNTS, dtype=np.uint32), np.asarray(KEEP, dtype=np.uint32))
    got = S.call(bt, S.tables(COUNTS), rows, keys, ops, w)
    want = S.call(bs, S.tables(COUNTS), rows, k2, ops, w)
    assert eq(got, want) and eq(keys, k2) and bool((_blobs(bt) == _blobs(bs)).all())
    bt.close(); bs.close()
