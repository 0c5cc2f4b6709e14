"""GPU: GLV_OP_BARS_ONLY batches through changes that move the live bins.

A flagged batch keeps state only where its bars sample (glv_batch_live_bins); a batch records the extent K its live calls have kept since creation, a reset
or the adoption of live streams -- the smallest any of them maintained -- and reports it as glv_batch_stream_state_desc().kept_bins (n while no live call
has run).  Once a live call has run, a change of the live bins -- glv_batch_set_params, either texel table, clearing one -- is accepted iff
0 < new live bins <= K, refused with GLV_ERR_STATE otherwise, and a refused change leaves the batch as it was.

Every case is written against the library's own report: the new live bins are read from a fresh batch of the new parameters, K just before the change,
and the change must be accepted exactly when the rule says so.  The reference of every output is an UNFLAGGED TWIN -- the same parameters, ops and input
without GLV_OP_BARS_ONLY, which runs the full chain -- compared bit for bit on every update (texels as int16, floats as int32); it receives the accepted
changes and not the refused ones.  For the GL_R16 chains the twin's side is anchored to the oracle: the `av` texels of a full-row batch of the same chain
against GLModel.  A library that refuses everything fails the changes that must be accepted (every shrink, every change to the same live bins, every
change on a batch that has not run live or was reset); one that reports too large a K accepts a change after which the flagged batch samples stale bins.

The ladder of live bins under sample_scale / sample_range is pinned on the CPU by tests/test_live_bins_changes_host.py.  The input is seeded full-band
noise whose level falls 16x on the update of every change, so that kept state dominates what follows; before each growing change a full-row batch of the
same chain must hold non-zero values in at least half of the bins that would become live (checked on the full rows, never on the flagged batch)."""
import numpy as np
import pytest

from gpu_lib import GLModel, eq, nan_rows as _nan, texel_rows as _texels
from oracle_lib import lcg_pcm_fast
from track_lib import differing, hop_windows, pitch_odd, seq, to_device, track, with_table

pytestmark = pytest.mark.gpu

F, STREAMS = 3, 3
RUN = F + 2                                                    # updates between two changes
LEVELS = (16, 8, 4, 2, 1)                                      # of the RUN updates behind a change: 16x down on the change, back up to full scale
# glv_batch_live_bins by (n, sample_scale) at the shipped range, and at scale 8 / range 0.8 (tests/test_live_bins_changes_host.py)
LADDER = {1024: {12: 256, 10: 256, 9: 320, 8: 320, 7: 384, 6: 448}, 4096: {12: 832, 10: 960, 9: 1088, 8: 1216, 7: 1408, 6: 1600}}
RANGE_08 = {1024: 256, 4096: 832}
# the rungs every kernel configuration has a live class for (three eighths of a row at the least); 1600 of 4096 has none: the full chain, live bins 0
LIVE_RUNGS = {1024: (12, 10, 9, 8, 7), 4096: (12, 10, 9, 8, 7)}
SCHEDULES = {4096: (9, 8, 10, 9, 12, 7, 6, "reset", 7, 8), 1024: (12, 9, 7, 9, "reset", 7, 9, 12)}
KNOBS = dict(fft_scale=10.2, fft_cutoff=0.3, gravity_step=4.2, ur=22050.0 / 256.0, avg_window=True)


def _noise(seed, u, streams, frames, level):
    """int16 [streams][frames][2] of update u at 1 / level of full scale, stream s another 2^s down"""
    x = lcg_pcm_fast(seed + 31 * u, streams * frames * 2).reshape(streams, frames, 2).copy()
    for s in range(streams):
        x[s] //= level * (1, 2, 4)[s % 3]
    return x


def _idx(values):
    import torch
    return torch.from_numpy(np.array(values, dtype=np.uint32).view(np.int32)).cuda()


def _chain(G, name, n, average):
    """-> (parameters, state mask, ops, output width, launches of a process call, ops of the full-row batch): the GL_R16 chain with bars = n in a second
    launch (kernel class 7), with 80 fused bars (9), the float chain with 80 fused bars (8)"""
    S = G.OP_GRAVITY | (G.OP_AVERAGE if average else 0)
    base = dict(n=n, avg_frames=F, log_mode=0)
    gl = dict(gl_storage=1, avg_window_kind=1)
    if name == "gl_rows": return dict(base, bars=n, bar_phase=0.5, **gl), S, G.OP_FFT | S | G.OP_BARS | G.OP_R16, n, 2, G.OP_FFT | S | G.OP_R16
    if name == "gl_80": return dict(base, bars=80, **gl), S, G.OP_FFT | S | G.OP_BARS, 80, 1, G.OP_FFT | S | G.OP_R16
    assert name == "float_80", name
    return dict(base, bars=80), S, G.OP_FFT | S | G.OP_BARS, 80, 1, G.OP_FFT | S


class Rig:
    """a flagged batch `b`, its unflagged twin `t` and a full-row batch `plain` of the same chain without bars, under the same parameters and input"""

    def __init__(self, G, chain, n, average=True, extra_mask=0, variant=None, model=False, table=None, plain=True):
        self.G, self.n, self.chain, self.variant = G, n, chain, variant
        self.kw, self.mask, self.ops, self.w, self.launches, self.plain_ops = _chain(G, chain, n, average)
        if table is not None: self.kw = dict(self.kw, bars=len(table[1]))
        self.extra, self.table, self.average = extra_mask, None, average
        mk = lambda m: G.Batch(G.Params(**self.kw), STREAMS, m | extra_mask)                                              # noqa: E731
        self.b, self.t = mk(self.mask | G.OP_BARS | G.OP_BARS_ONLY), mk(self.mask | G.OP_BARS)
        self.plain = mk(self.mask) if plain else None
        for x in self.all():
            if variant is not None: x.set_variant(variant)
        self.model = GLModel(STREAMS * 2, n, F, average) if model else None
        self.with_model = model
        self.last_plain, self.u, self.live_calls = None, 0, 0

    def all(self):
        return [x for x in (self.b, self.t, self.plain) if x is not None]

    def close(self):
        for x in self.all(): x.close()

    def kept(self):
        return int(self.b.stream_state_desc().kept_bins)

    def out(self, ops, w, rows=None):
        return (_texels if ops & self.G.OP_R16 else _nan)(rows or STREAMS * 2, w)

    def probe(self, kw, table):
        """glv_batch_live_bins of a fresh flagged batch under these parameters and this table"""
        p = with_table(self.G.Batch(self.G.Params(**kw), 1, self.mask | self.G.OP_BARS | self.G.OP_BARS_ONLY | self.extra), table)
        L = p.live_bins(); p.close()
        return L

    # ---- one update / one call on all three --------------------------------------------------------------------------------------------------------
    def step(self, fn_b, fn_t=None, fn_plain=None, live=True, what=()):
        """fn(batch, ops, w) -> the call's output, [rows][w] or [updates][rows][w]: the flagged batch against the twin bit for bit; the full-row batch's last
        update is kept for the precondition of the next growing change"""
        L = self.b.live_bins()
        got, want = fn_b(self.b, self.ops, self.w), (fn_t or fn_b)(self.t, self.ops, self.w)
        assert got.shape == want.shape and eq(got, want), (self.chain, self.n, self.variant, self.u, L, self.kept(), differing(got, want), *what)
        assert bool((got != 0).any())
        if live and L != 0:                                                   # (a track call whose kept bins leave the live share runs full rows: the extent stays)
            self.live_calls += self.kept() < self.n
            assert L <= self.kept(), (L, self.kept())                         # what the extent says covers what the call sampled
        if self.plain is not None:
            rows = (fn_plain or fn_b)(self.plain, self.plain_ops, self.n)
            self.last_plain = rows.reshape(-1, STREAMS * 2, self.n)[-1].cpu().numpy()
        self.u += 1
        return got

    def update(self, x, method="process_s16", extra=()):
        """one process / ring update of all three from the host frames x; the process call's kernel class through its launches and configuration"""
        import torch
        d = torch.from_numpy(np.ascontiguousarray(x)).cuda()

        def fn(batch, ops, w):
            o = self.out(ops, w)
            getattr(batch, method)(d, *extra, o, ops)
            return o
        L, K = self.b.live_bins(), self.kept()
        got = self.step(fn, live=False)
        launches, v = self.b.last_launches(), self.b.last_variant()
        if self.variant is not None: assert v == self.variant, (v, self.variant)
        assert launches == self.t.last_launches(), (launches, self.t.last_launches())
        if self.chain != "float_80" and not self.extra: assert launches == self.launches, (self.chain, launches)
        if L != 0 and (self.chain != "float_80" or launches == 1):            # the live class ran (a float chain in a configuration that cannot fuse: the full chain)
            self.live_calls += 1
            assert L <= self.kept() <= min(K, self.n - 1), (L, K, self.kept())
        if self.model is not None:
            k = {key: self.kw.get(key, v_) for key, v_ in KNOBS.items()}
            want = self.model.update(x, k)
            bad = self.last_plain.view(np.uint16) != want
            assert not bad.any(), ("the full rows against the model", self.u, int(bad.sum()), np.argwhere(bad)[:3].tolist())
        return got

    def run(self, seed, count=RUN, method="process_s16", frames=None, extra=()):
        for i in range(count):
            self.update(_noise(seed, self.u, STREAMS, frames or self.n, LEVELS[i % len(LEVELS)]), method, extra)

    def reset(self):
        for x in self.all(): x.reset()
        if self.with_model: self.model = GLModel(STREAMS * 2, self.n, F, self.average)
        self.live_calls, self.last_plain = 0, None
        assert self.kept() == self.n                                         # glv_batch_reset clears the extent

    # ---- one change ----------------------------------------------------------------------------------------------------------------------------------
    def change(self, table="same", fresh=False, **more):
        """glv_batch_set_params with `more` on top of the current parameters -- or, with `table`, glv_batch_set_bar_texels / _column_texels (None: clear) --
        held to the rule: accepted iff the batch has not run live or 0 < new live bins <= kept_bins; applied to the twin and the full-row batch only when
        accepted.  fresh: the caller knows that no live call has run since creation or the last reset.  -> (accepted, live bins before, new live bins)"""
        G, b, n = self.G, self.b, self.n
        new = dict(self.kw, **more)
        new_table = self.table if isinstance(table, str) else table
        L_old, K, arith = b.live_bins(), self.kept(), b.bars_arithmetic()
        L_new = self.probe(new, new_table)
        ran = K != n
        accept = (not ran) or 0 < L_new <= K
        print(f"{self.chain} n={n} v={self.variant} u={self.u}: {more or new_table and new_table[0] or 'clear'} live {L_old} -> {L_new}, kept {K}: {'accept' if accept else 'refuse'}")
        assert not (fresh and ran), "kept_bins must be n while no live call has run"
        if fresh or self.live_calls == 0 or 0 < L_new <= L_old: assert accept, (L_old, L_new, K)     # what must be accepted whatever K says
        if 0 < L_old < L_new and self.last_plain is not None:
            seg = self.last_plain[:2, L_old:L_new]                            # the loudest stream's rows
            frac = float((seg != 0).mean())
            print(f"    full rows, bins [{L_old}, {L_new}): {frac:.3f} non-zero")
            assert frac >= 0.5, (L_old, L_new, frac)
        if accept:
            for x in self.all():
                if more: x.set_params(G.Params(**new))
                if not isinstance(table, str) and x is not self.plain: with_table(x, table) if table else (x.set_bar_texels(None), x.set_column_texels(None))
            self.kw, self.table = new, new_table
            assert b.live_bins() == L_new and self.t.live_bins() == 0
            assert self.kept() == K                                           # a change keeps nothing and loses nothing
        else:
            with pytest.raises(G.GlvError) as ei:
                if more: b.set_params(G.Params(**new))
                else: with_table(b, table)
            assert ei.value.code == G.ERR_STATE, (ei.value.code, str(ei.value))
            assert (b.live_bins(), self.kept(), b.bars_arithmetic()) == (L_old, K, arith)
        return accept, L_old, L_new

    def rung(self, scale, rng=0.0, **kw):
        """sample_scale / sample_range through change(); the new live bins are the ladder's (0 where the size has no live class that far)"""
        accept, L_old, L_new = self.change(sample_scale=float(scale), sample_range=float(rng), **kw)
        want = RANGE_08[self.n] if rng else LADDER[self.n][scale]
        assert L_new == (want if rng or scale in LIVE_RUNGS[self.n] else 0), (self.n, scale, rng, L_new, want)
        return accept, L_old, L_new

    def climb(self, seed, run):
        """the size's schedule of scales, `run()` between the changes: the first change and the one behind a reset find a batch that has not run live"""
        fresh = True
        for s in SCHEDULES[self.n]:
            if s == "reset":
                self.reset(); fresh = True
                continue
            self.rung(s, fresh=fresh)
            fresh = False
            run()


# ---- 1. the process path -----------------------------------------------------------------------------------------------------------------------------
def _process_cases():
    out = []
    for chain, n in (("gl_rows", 4096), ("gl_80", 4096), ("float_80", 4096), ("float_80", 1024), ("gl_rows", 1024)):
        for average in (True, False):
            for v in (0, 1):
                out.append(pytest.param(chain, n, average, v, id=f"{chain}-{n}-{'average' if average else 'gravity'}-v{v}"))
    return out


@pytest.mark.parametrize("chain,n,average,variant", _process_cases())
def test_process_calls_through_the_ladder(glvlib, oracle, chain, n, average, variant):
    """glv_batch_process_s16 in both kernel configurations: the size's schedule of scales with F + 2 updates between the changes, then a change that leaves
    the live bins where they are (smooth_factor and the tilt), a shrink through sample_range, and glv_batch_reset_streams of every stream -- after which a
    growing change is still refused.  The GL_R16 chain in configuration 0: the full rows against the oracle's model on every update"""
    G = glvlib
    rig = Rig(G, chain, n, average, variant=variant, model=chain == "gl_rows" and variant == 0)
    assert rig.b.variants() == 2 and rig.kept() == n
    seed = 100 * n + 10 * variant + average
    rig.climb(seed, lambda: rig.run(seed))
    accept, L_old, L_new = rig.change(smooth_factor=0.05, fft_scale=7.0, fft_cutoff=0.5)
    assert accept and L_new == L_old
    rig.run(seed)
    accept, _, _ = rig.rung(8, 0.8)
    assert accept
    rig.run(seed)
    K = rig.kept()
    for x in rig.all(): x.reset_streams(_idx(range(STREAMS)), STREAMS)
    if rig.with_model: rig.model = GLModel(STREAMS * 2, n, F, average)        # (zeros in every slot read the same wherever the ring's head points)
    assert rig.kept() == K                                                    # the other streams of a batch are still partial: the extent stays
    accept, _, L_new = rig.rung(7)
    assert not accept and L_new > K
    rig.run(seed)
    rig.close()


# ---- 2. ring batches -----------------------------------------------------------------------------------------------------------------------------------
def test_ring_updates_through_the_ladder(glvlib):
    """the same schedule through glv_batch_ring_update_s16, 1500 new frames per update: the GL_R16 chain with bars = n"""
    G = glvlib
    n, nf = 4096, 1500
    rig = Rig(G, "gl_rows", n, extra_mask=G.OP_RING_S16)
    rig.climb(7000, lambda: rig.run(7000, method="ring_update_s16", frames=nf, extra=(nf,)))
    rig.close()


# ---- 3. track live -------------------------------------------------------------------------------------------------------------------------------------
def _recording(seed, n, hop, steps, f32):
    """(host recording, device recording, pitch): noise whose level walks LEVELS hop by hop, so that every call of RUN steps starts 16x below the end of the
    call before it"""
    import torch                                                              # noqa: F401
    pitch = pitch_odd(n, hop, steps + 1) + 2
    level = np.array(LEVELS)[(np.arange(pitch) // hop) % len(LEVELS)]
    if f32:
        x = (np.random.default_rng(seed).standard_normal((STREAMS, pitch, 2)) * 0.3).astype(np.float32)
        for s in range(STREAMS): x[s] = (x[s] / (level * (1, 2, 4)[s])[:, None].astype(np.float32)).astype(np.float32)
    else:
        x = lcg_pcm_fast(seed, STREAMS * pitch * 2).reshape(STREAMS, pitch, 2).copy()
        for s in range(STREAMS): x[s] //= (level * (1, 2, 4)[s])[:, None].astype(np.int16)
    return x, to_device(x, True, f32), pitch


class Tracked:
    """a Rig whose flagged batch runs RUN steps per glv_batch_track_live_* call; the twin and the full-row batch take the windows one by one"""

    def __init__(self, G, rig, seed, f32, pieces):
        import torch
        self.G, self.rig, self.f32, self.t0 = G, rig, f32, 0
        self.hop = 45 * rig.n // 256
        self.x, self.d_pcm, self.pitch = _recording(seed, rig.n, self.hop, pieces * RUN, f32)
        self.wins = hop_windows(self.x, rig.n, self.hop, 0, pieces * RUN)
        self.dt = lambda ops: torch.int16 if ops & G.OP_R16 else torch.float32                                            # noqa: E731

    def call(self):
        rig, t0 = self.rig, self.t0
        L = rig.b.live_bins()
        live = lambda b, ops, w: track(b, "live", self.d_pcm, self.pitch, self.hop, RUN, ops, w, self.dt(ops), t0=t0, f32=self.f32)      # noqa: E731
        one_by_one = lambda b, ops, w: seq(b, self.wins[t0:t0 + RUN], ops, w, self.dt(ops), self.f32)                                    # noqa: E731
        rig.step(live, one_by_one, one_by_one, what=("track", t0))
        assert rig.b.last_launches() == 3, rig.b.last_launches()
        if L != 0 and rig.ops & self.G.OP_R16: assert rig.kept() <= L       # texel rows: the scan keeps the live bins and no more
        self.t0 += RUN


@pytest.mark.parametrize("entry", ["s16", "f32"])
def test_track_live_calls_through_the_ladder(glvlib, entry):
    """glv_batch_track_live_s16 on the GL_R16 chain with bars = n (texel rows all the way) at n = 4096, glv_batch_track_live_f32 on the float chain with 80
    chunked bars at n = 1024: five steps per call at hop 45 n / 256, a change between calls, against the one-by-one process calls of the unflagged twin.
    A track call keeps exactly its kept bins: any growth behind one reads stale state"""
    G = glvlib
    f32 = entry == "f32"
    n = 1024 if f32 else 4096
    rig = Rig(G, "float_80" if f32 else "gl_rows", n)
    tr = Tracked(G, rig, 8100 + n, f32, sum(s != "reset" for s in SCHEDULES[n]))
    rig.climb(0, tr.call)
    rig.close()


# ---- 4. ring track -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("each", [False, True], ids=["lockstep", "each"])
def test_ring_track_calls_through_the_ladder(glvlib, each):
    """glv_batch_ring_track_s16 and glv_batch_ring_track_each_s16 (counts 2, 0, 1) on a flagged ring batch: two updates per call, two calls between changes"""
    import torch
    G = glvlib
    n, nf, updates = 1024, 300, 2
    rig = Rig(G, "gl_rows", n, extra_mask=G.OP_RING_S16)
    counts = _idx([2, 0, 1]) if each else None

    def call(b, ops, w):
        x = _noise(9100, rig.u, STREAMS, updates * nf, LEVELS[(2 * rig.u) % len(LEVELS)])
        d_new = torch.from_numpy(x).cuda()
        nbytes = (b.ring_track_each_work_bytes if each else b.ring_track_work_bytes)(nf, updates, ops)
        work = torch.zeros((nbytes,), dtype=torch.uint8, device="cuda")
        o = rig.out(ops, w, updates * STREAMS * 2).view(updates, STREAMS * 2, w)
        if each: b.ring_track_each_s16(d_new, nf, updates, None, counts, o, work, ops)
        else: b.ring_track_s16(d_new, nf, updates, o, work, ops)
        torch.cuda.synchronize()
        return o

    def run():
        for _ in range(2): rig.step(call, what=("ring track", each))
    rig.climb(0, run)
    rig.close()


# ---- 5. process and track calls on one batch -----------------------------------------------------------------------------------------------------------
def test_the_extent_follows_the_smallest_of_process_and_track_calls(glvlib):
    """process calls at scale 12, a change to 9, a live track call, a change to 8, process calls -- each change by the rule.  Then from a reset: process calls
    at 9, a shrink to 12 (the extent stays: no call has run there), a live track call at 12 -- which keeps its own bins and no more: the extent falls to them
    -- and the way back to 9 is refused"""
    G = glvlib
    n = 4096
    rig = Rig(G, "gl_rows", n)
    tr = Tracked(G, rig, 8700, False, 3)
    rig.rung(12, fresh=True); rig.run(8800)
    rig.rung(9); tr.call()
    rig.rung(8); rig.run(8800)
    rig.reset()
    rig.rung(9, fresh=True); rig.run(8800)
    K9 = rig.kept()
    assert K9 >= LADDER[n][9]
    accept, _, _ = rig.rung(12)
    assert accept and rig.kept() == K9
    tr.call()
    assert rig.kept() == LADDER[n][12] < K9                                   # a track call after process calls lowers the extent to its own
    accept, _, _ = rig.rung(9)
    assert not accept
    rig.run(8800); tr.call()
    rig.close()


# ---- 6. the texel tables -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bar", "col"])
def test_texel_tables_by_the_same_rule(glvlib, kind):
    """8 bars of the GL_R16 chain at n = 1024 sample 256 bins.  A table whose taps stay below them is accepted on a batch that ran live, one that reaches
    further (texels at the end of the row: 320 bins) is refused, the clear is accepted and the extent is what was kept.  From a reset: the far table first,
    then the near one -- a shrink, accepted -- and the far one is refused again"""
    G = glvlib
    n, B = 1024, 8
    near, far = np.arange(B) * 12 + 3, n - 1 - 3 * np.arange(B)[::-1]
    if kind == "col": near, far = np.stack([near, near + 1, near + 2], 1), np.stack([far - 2, far - 1, far], 1)
    rig = Rig(G, "gl_80", n, table=(kind, near), plain=False)                 # (the table sets the bar count; none is set yet)
    rig.w = B
    if kind == "bar": rig.ops |= G.OP_R16
    seed = 9500 + (kind == "col")
    L0 = rig.b.live_bins()
    assert L0 == 256 and rig.probe(rig.kw, (kind, far)) == 320 and rig.probe(rig.kw, (kind, near)) == L0
    rig.run(seed)
    assert rig.kept() == L0
    accept, _, _ = rig.change(table=(kind, near)); assert accept
    rig.run(seed)
    accept, _, _ = rig.change(table=(kind, far)); assert not accept
    rig.run(seed)
    accept, _, _ = rig.change(table=None); assert accept and rig.kept() == L0 and rig.b.live_bins() == L0
    rig.run(seed)
    rig.reset()
    accept, _, L = rig.change(table=(kind, far), fresh=True); assert accept and L == 320
    rig.run(seed)
    assert rig.kept() == 320
    accept, _, _ = rig.change(table=(kind, near)); assert accept               # a shrink
    assert rig.kept() == 320
    rig.run(seed)
    assert rig.kept() == L0
    accept, _, _ = rig.change(table=(kind, far)); assert not accept
    accept, _, _ = rig.change(table=None); assert accept and rig.kept() == L0
    accept, _, _ = rig.change(table=(kind, far)); assert not accept
    rig.run(seed)
    rig.close()


# ---- 7. stream slots and elastic copies ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("via", ["blob", "copy"])
def test_saved_and_copied_streams_carry_the_extent_they_were_kept_to(glvlib, via):
    """9 -> 10 -> (9 refused) -> 12 without a call: the descriptor says 960, what the calls kept, not the 832 the batch samples now.  The streams go into a fresh
    flagged batch at scale 10, which then keeps 960 itself, refuses the way to 9 and continues bit for bit as the source; a flagged batch at scale 9 refuses them"""
    import torch
    G = glvlib
    n = 4096
    rig = Rig(G, "gl_rows", n, plain=False)
    rig.rung(9, fresh=True); rig.run(9800)
    accept, _, _ = rig.rung(10); assert accept
    rig.run(9800)
    accept, _, _ = rig.rung(9); assert not accept
    accept, _, _ = rig.rung(12); assert accept
    assert rig.kept() == LADDER[n][10] and rig.b.live_bins() == LADDER[n][12]
    idx = _idx(range(STREAMS))
    blob = torch.zeros((STREAMS * int(rig.b.stream_state_desc().bytes),), dtype=torch.uint8, device="cuda")
    desc = rig.b.save_streams(idx, STREAMS, blob)
    assert desc.kept_bins == LADDER[n][10]
    accept, _, _ = rig.rung(10); assert accept
    flagged = rig.mask | G.OP_BARS | G.OP_BARS_ONLY
    at10 = G.Batch(G.Params(**rig.kw), STREAMS, flagged)
    at9 = G.Batch(G.Params(**dict(rig.kw, sample_scale=9.0)), STREAMS, flagged)
    assert at10.live_bins() == LADDER[n][10] and at9.live_bins() == LADDER[n][9]
    assert at10.stream_state_desc().kept_bins == at9.stream_state_desc().kept_bins == n
    with pytest.raises(G.GlvError) as ei:
        if via == "blob": at9.load_streams(idx, STREAMS, blob, desc)
        else: at9.copy_streams(idx, rig.b, idx, STREAMS)
    assert ei.value.code == G.ERR_STATE and at9.stream_state_desc().kept_bins == n
    if via == "blob": at10.load_streams(idx, STREAMS, blob, desc)
    else: at10.copy_streams(idx, rig.b, idx, STREAMS)
    torch.cuda.synchronize()
    assert at10.stream_state_desc().kept_bins == LADDER[n][10]              # a batch that had not run live adopts the streams' extent
    with pytest.raises(G.GlvError) as ei:
        at10.set_params(G.Params(**dict(rig.kw, sample_scale=9.0)))
    assert ei.value.code == G.ERR_STATE and at10.live_bins() == LADDER[n][10]
    for i in range(RUN):
        x = _noise(9800, rig.u, STREAMS, n, LEVELS[i])
        got = rig.update(x)
        o = rig.out(rig.ops, rig.w)
        at10.process_s16(torch.from_numpy(x).cuda(), o, rig.ops)
        assert eq(o, got), (via, i, differing(o, got))
    at10.close(); at9.close(); rig.close()


# ---- 8. what must be accepted -----------------------------------------------------------------------------------------------------------------------------
def test_a_batch_that_has_not_run_live_accepts_every_change(glvlib):
    """up and down the whole ladder, beyond the live share and back, and log_mode 2 and back, without a call in between; after calls and glv_batch_reset
    the same again; kept_bins is n all the while"""
    G = glvlib
    n = 4096
    rig = Rig(G, "gl_rows", n, plain=False)
    for again in range(2):
        for scale in (7, 12, 6, 9, 8, 10):
            accept, _, _ = rig.rung(scale, fresh=True)
            assert accept and rig.kept() == n
        accept, _, L = rig.change(log_mode=2, fresh=True); assert accept and L == 0
        accept, _, L = rig.change(log_mode=0, fresh=True); assert accept and L == LADDER[n][10]
        accept, _, _ = rig.rung(8, 0.8, fresh=True); assert accept
        rig.run(9900)
        assert rig.kept() == RANGE_08[n]
        rig.reset()
    rig.close()
