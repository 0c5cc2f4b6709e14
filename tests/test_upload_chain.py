"""GPU: glv_params.gl_storage = 3 -- the CPU operators on float state, then the GL_R16 upload of the finished buffer (GLava with `setaccelfft false`).

Yardstick: for every update the upload texels U come from a gl_storage 0 twin batch fed the same input (GLV_OP_FFT | GRAVITY | AVERAGE | R16: the parent's
code, pinned to the oracle elsewhere; with log_mode 0 U is checked against the oracle's texels here as well).  A gl_storage 3 batch must then give, bit for
bit, as texels and as floats:
    bars = n, bar_phase 0.5 (the pre-smoothing pass)          Oracle.bars_int(U)
    bar texels (radial / bars module)                          that pass at the table's texels
    column texels (graph module)                               column_mean of three texels of that pass (floats only)
    sample_mode maximum / hybrid, with and without a table     Oracle.bars_mode over U / 65535
Shapes: N = 1024 (64 lanes per row: 80 bars take the second trip) and 4096, 3 and 37 streams (ragged against every rows-per-workgroup), F = 5 and 1,
channels 1 and 2, both log modes, F + 3 updates; one case at N = 256 (two launches only) and one at N = 16384 (configuration 1 never fuses).  Rows: all of
them up to 8, else the first and last four, two in the middle and every ninth (`_rows`): where a ragged last workgroup or trip would show."""
import os

import numpy as np
import pytest

from glava_amd.bar_positions import bars_module_bar_texels, graph_column_texels, radial_bar_texels
from gpu_lib import eq as _eq
from oracle_lib import Oracle, StreamOracle, lcg_pcm_fast

pytestmark = pytest.mark.gpu
F32 = np.float32
# (n, streams, F, channels, log_mode)
CASES = [(1024, 3, 5, 2, 1), (1024, 37, 1, 1, 0), (4096, 37, 5, 2, 0), (4096, 3, 1, 1, 1), (256, 3, 5, 2, 1), (16384, 3, 5, 2, 1)]
IDS = ["n%d-s%d-F%d-c%d-log%d" % c for c in CASES]


def _kw(case, **more):
    n, _, F, ch, lm = case
    return dict(n=n, avg_frames=F, channels=ch, log_mode=lm, **more)


def _updates(case):
    return case[2] + 3


def _rows(case):
    rows = case[1] * 2
    if rows <= 8:
        return list(range(rows))
    return sorted(set([0, 1, 2, 3, rows // 2, rows // 2 + 1, rows - 4, rows - 3, rows - 2, rows - 1] + list(range(0, rows, 9))))


_PCM, _U, _PASS, _MODE = {}, {}, {}, {}


def _pcm(case, fr):
    """the int16 input of update fr, on the host and on the device: made once per case and shared, never written"""
    import torch
    key = (case, fr)
    if key not in _PCM:
        n, streams = case[0], case[1]
        x = (lcg_pcm_fast(4100 + 17 * fr + n, streams * 2 * n) // (1, 8, 64)[fr % 3]).astype(np.int16)
        x.setflags(write=False)
        _PCM[key] = (x, torch.from_numpy(np.array(x, copy=True)).cuda())
    return _PCM[key]


def _upload(G, case):
    """U[fr]: uint16 [rows][n], the upload texels of every update, from a gl_storage 0 batch (FFT | GRAVITY | AVERAGE | R16) -- computed once per case"""
    import torch
    if case not in _U:
        n, streams, F, ch, lm = case
        GA = G.OP_GRAVITY | G.OP_AVERAGE
        b = G.Batch(G.Params(**_kw(case)), streams, GA)
        out = torch.zeros((streams * 2, n), dtype=torch.int16, device="cuda")
        U = []
        for fr in range(_updates(case)):
            b.process_s16(_pcm(case, fr)[1], out, G.OP_FFT | GA | G.OP_R16)
            assert b.last_launches() == 1
            U.append(out.cpu().numpy().view(np.uint16).copy())
        b.close()
        if lm == 0:      # the bit-faithful log: U itself is the oracle's upload of the oracle's float chain
            for s in (0, streams - 1):
                so = StreamOracle(n, channels=ch, avg_frames=F)
                for fr in range(_updates(case)):
                    want = Oracle.texels_r16(so.frame(_pcm(case, fr)[0][s * 2 * n:(s + 1) * 2 * n]))
                    assert (U[fr][2 * s:2 * s + 2] == want).all(), (case, s, fr)
        for u in U:
            u.setflags(write=False)
        _U[case] = U
    return _U[case]


def _pass(G, case):
    """(texels, floats)[fr][row]: Oracle.bars_int(U, bars = n, phase 0.5) for the rows under test -- once per case"""
    if case not in _PASS:
        U, n = _upload(G, case), case[0]
        _PASS[case] = [{r: Oracle.bars_int(U[fr][r], n, 0.025, 0.5) for r in _rows(case)} for fr in range(_updates(case))]
    return _PASS[case]


def _mode(G, case, mode, bars, phase):
    """floats [fr][row]: Oracle.bars_mode over U / 65535 -- once per (case, mode, bars, phase)"""
    key = (case, mode, bars, phase)
    if key not in _MODE:
        U = _upload(G, case)
        x = lambda c: (c.astype(np.float64) / 65535).astype(F32)             # noqa: E731  (c / 65535 correctly rounded: what texelFetch returns)
        _MODE[key] = [{r: Oracle.bars_mode(x(U[fr][r]), bars, mode, 0.65, 0.025, phase) for r in _rows(case)} for fr in range(_updates(case))]
    return _MODE[key]


def _column_mean(tex, table):
    """tex uint16 [n], table [count][3] -> float32 [count]: fdiv(fadd(fadd(T(l), T(m)), T(r)), 3)"""
    T = (tex.astype(np.float64) / 65535).astype(F32)
    lm = (T[table[:, 0]] + T[table[:, 1]]).astype(F32)
    return ((lm + T[table[:, 2]]).astype(F32) / F32(3.0)).astype(F32)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint16)


class _Run:
    """one gl_storage 3 batch under test: created, table set, and per update one call whose rows under test are compared with want(fr, row)"""

    def __init__(self, G, case, name, bars, want, r16, bar_tex=None, col_tex=None, mask_more=0, ops=None, **kw):
        import torch
        self.G, self.case, self.name, self.want, self.r16 = G, case, name, want, r16
        GA = G.OP_GRAVITY | G.OP_AVERAGE
        self.b = G.Batch(G.Params(**_kw(case, bars=bars, gl_storage=G.GL_STORAGE_UPLOAD, **kw)), case[1], GA | G.OP_BARS | mask_more)
        if bar_tex is not None: self.b.set_bar_texels(bar_tex)
        if col_tex is not None: self.b.set_column_texels(col_tex)
        self.ops = (G.OP_FFT | GA if ops is None else ops) | G.OP_BARS | (G.OP_R16 if r16 else 0)
        self.out = torch.zeros((case[1] * 2, bars), dtype=torch.int16 if r16 else torch.float32, device="cuda")
        self.launches = set()

    def update(self, fr):
        self.b.process_s16(_pcm(self.case, fr)[1], self.out, self.ops)
        self.launches.add(self.b.last_launches())
        assert self.b.kernel_name() == "glv_frame_kernel"

    def check(self, fr):
        got = self.out.cpu().numpy()
        for r in _rows(self.case):
            w = self.want(fr, r)
            assert _bits(got[r]).dtype == _bits(w).dtype and (_bits(got[r]) == _bits(w)).all(), \
                (self.name, self.case, "texels" if self.r16 else "floats", fr, r, int((_bits(got[r]) != _bits(w)).sum()))

    def close(self):
        self.b.close()


def _drive(runs, case):
    import torch
    for fr in range(_updates(case)):
        for x in runs: x.update(fr)
        torch.cuda.synchronize()
        for x in runs: x.check(fr)
    for x in runs: x.close()


def _fuses(G, n, count, cols):
    """does the default kernel configuration of the size take `count` snapped results behind its row (as the GL_R16 chain's classes do)?"""
    lanes = {256: 16, 1024: 64, 4096: 128, 16384: 256}[n]
    return lanes % 64 == 0 and (count + 1 <= 4 * lanes and count <= 1023 if cols else count + 1 <= 2 * lanes)


def _col_widths(n):
    """one window width whose columns fuse at the size and one whose columns do not (at 256 neither does: 16 lanes per row)"""
    return {256: (64, 320), 1024: (120, 320), 4096: (320, 800), 16384: (320, 1920)}[n]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_pass_bar_texels_and_columns(glvlib, oracle, case):
    G, n = glvlib, case[0]
    P = _pass(G, case)
    radial = radial_bar_texels(n, 160)[0].astype(np.int64)
    module = bars_module_bar_texels(n, 1280, 5, 1, 2)[0].astype(np.int64)
    runs = []
    for r16 in (True, False):
        k = 0 if r16 else 1
        runs.append(_Run(G, case, "pass", n, lambda fr, r, k=k: P[fr][r][k], r16, bar_phase=0.5))
        assert runs[-1].b.bars_arithmetic() == G.BARS_I8_EXACT
        runs.append(_Run(G, case, "radial", len(radial), lambda fr, r, k=k: P[fr][r][k][radial], r16, bar_tex=radial))
        assert runs[-1].b.bars_arithmetic() == G.BARS_I8_EXACT
        runs.append(_Run(G, case, "module", len(module), lambda fr, r, k=k: P[fr][r][k][module], r16, bar_tex=module))
    tables = [graph_column_texels(n, W)[0].astype(np.int64) for W in _col_widths(n)]
    for t in tables:
        runs.append(_Run(G, case, "columns%d" % len(t), len(t), lambda fr, r, t=t: _column_mean(P[fr][r][0], t), False, col_tex=t))
    # a GLV_OP_BARS_ONLY batch has no live bins on this storage: the full chain, the same results
    runs.append(_Run(G, case, "radial_bars_only", len(radial), lambda fr, r: P[fr][r][0][radial], True, bar_tex=radial, mask_more=G.OP_BARS_ONLY))
    assert runs[-1].b.live_bins() == 0
    _drive(runs, case)
    by = {x.name + ("16" if x.r16 else ""): x.launches for x in runs}
    assert by["pass16"] == {2} and by["pass"] == {2}
    assert by["radial16"] == by["radial"] == by["radial_bars_only16"] == ({1} if _fuses(G, n, len(radial), False) else {2}), by
    assert by["module16"] == by["module"] == ({1} if _fuses(G, n, len(module), False) else {2}), by
    fused = [by["columns%d" % len(t)] == {1} for t in tables]
    assert fused == [_fuses(G, n, len(np.unique(t)), True) for t in tables], (by, fused)
    if n >= 1024: assert fused == [True, False]


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_maximum_hybrid(glvlib, oracle, case, mode):
    G, n = glvlib, case[0]
    M80, Mn = _mode(G, case, mode, 80, 0.0), _mode(G, case, mode, n, 0.5)
    radial = radial_bar_texels(n, 160)[0].astype(np.int64)
    table = graph_column_texels(n, _col_widths(n)[0])[0].astype(np.int64)
    tex = lambda f: Oracle.texels_r16(f)                                      # noqa: E731  (the r16 output: the bar's upload)
    runs = []
    for r16 in (True, False):
        q = tex if r16 else (lambda f: f)
        runs.append(_Run(G, case, "bars80", 80, lambda fr, r, q=q: q(M80[fr][r]), r16, sample_mode=mode))
        assert runs[-1].b.bars_arithmetic() == G.BARS_F32_SEQ
        runs.append(_Run(G, case, "bars_n", n, lambda fr, r, q=q: q(Mn[fr][r]), r16, sample_mode=mode, bar_phase=0.5))
        runs.append(_Run(G, case, "radial", len(radial), lambda fr, r, q=q: q(Mn[fr][r][radial]), r16, sample_mode=mode, bar_tex=radial))
    runs.append(_Run(G, case, "columns", len(table), lambda fr, r: _column_mean(tex(Mn[fr][r]), table), False, sample_mode=mode, col_tex=table))
    _drive(runs, case)
    for x in runs:
        assert x.launches == {2}, (x.name, x.launches)


def test_stateless_and_gravity_only_chains(glvlib, oracle):
    """an FFT chain with or without gravity / average: the bars sample the upload of whatever the finished row is"""
    import torch
    G = glvlib
    n, streams = 1024, 3
    case = (n, streams, 5, 2, 1)
    radial = radial_bar_texels(n, 160)[0].astype(np.int64)
    for chain in (0, G.OP_GRAVITY, G.OP_AVERAGE):
        twin = G.Batch(G.Params(**_kw(case)), streams, chain | G.OP_FFT)
        U = torch.zeros((streams * 2, n), dtype=torch.int16, device="cuda")
        runs = [_Run(G, case, "pass", n, None, True, bar_phase=0.5, ops=G.OP_FFT | chain), _Run(G, case, "radial", len(radial), None, False, bar_tex=radial, ops=G.OP_FFT | chain)]
        for fr in range(4):
            twin.process_s16(_pcm(case, fr)[1], U, G.OP_FFT | chain | G.OP_R16)
            for x in runs: x.update(fr)
            torch.cuda.synchronize()
            u = U.cpu().numpy().view(np.uint16)
            got16, gotf = runs[0].out.cpu().numpy().view(np.uint16), runs[1].out.cpu().numpy()
            for r in range(streams * 2):
                t, f = Oracle.bars_int(u[r], n, 0.025, 0.5)
                assert (got16[r] == t).all(), (chain, fr, r)
                assert (gotf[r].view(np.uint32) == f[radial].view(np.uint32)).all(), (chain, fr, r)
        assert runs[0].launches == {2} and runs[1].launches == ({1} if chain else {2}), (chain, runs[1].launches)
        for x in runs: x.close()
        twin.close()


def _unfused(make):
    """a batch created with GLV_UNFUSED_BARS in the environment: its bars always take a second launch"""
    os.environ["GLV_UNFUSED_BARS"] = "1"
    try:
        return make()
    finally:
        del os.environ["GLV_UNFUSED_BARS"]


@pytest.mark.parametrize("n", [1024, 4096, 16384])
def test_one_launch_equals_two_launches(glvlib, n):
    """bar texels and columns: the one-launch classes against the two-launch route, on both kernel configurations and with forced grids 1 and 3"""
    import torch
    G = glvlib
    streams = 3 if n == 16384 else 37
    case = (n, streams, 5, 2, 1)
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    radial = radial_bar_texels(n, 160)[0].astype(np.int64)
    table = graph_column_texels(n, _col_widths(n)[0])[0].astype(np.int64)
    seen = set()
    for what, tex, r16 in (("bar", radial, True), ("bar", radial, False), ("col", table, False)):
        def make():
            b = G.Batch(G.Params(**_kw(case, bars=len(tex), gl_storage=G.GL_STORAGE_UPLOAD)), streams, GA | G.OP_BARS)
            (b.set_bar_texels if what == "bar" else b.set_column_texels)(tex)
            return b
        two = _unfused(make)
        ones = []
        for v in range(two.variants()):
            for grid in (0, 1, 3):
                b = make(); b.set_variant(v); b.set_grid(grid)
                ones.append((v, grid, b))
        ops = G.OP_FFT | GA | G.OP_BARS | (G.OP_R16 if r16 else 0)
        dt = torch.int16 if r16 else torch.float32
        want = torch.zeros((streams * 2, len(tex)), dtype=dt, device="cuda")
        got = torch.zeros_like(want)
        for fr in range(_updates(case)):
            two.process_s16(_pcm(case, fr)[1], want, ops)
            assert two.last_launches() == 2
            for v, grid, b in ones:
                got.zero_()
                b.process_s16(_pcm(case, fr)[1], got, ops)
                seen.add((v, b.last_launches()))
                if grid: assert b.last_grid() == grid
                assert _eq(got, want), (n, what, r16, v, grid, fr)
        for _, _, b in ones: b.close()
        two.close()
    # configuration 0 fuses at every one of these sizes; configuration 1 of N = 16384 exchanges through split regions and never does
    assert (0, 1) in seen and (0, 2) not in seen
    assert ((1, 2) in seen) == (n == 16384) and ((1, 1) in seen) == (n != 16384), seen


def test_state_is_that_of_gl_storage_0_and_calls_interleave(glvlib):
    """calls without GLV_OP_BARS are gl_storage 0's in every bit -- float rows, texels, state -- with bars calls in between; then the batch moves to 0"""
    import torch
    G = glvlib
    for case in ((1024, 3, 5, 2, 1), (4096, 37, 1, 1, 0)):
        n, streams, F = case[0], case[1], case[2]
        GA = G.OP_GRAVITY | G.OP_AVERAGE
        a = G.Batch(G.Params(**_kw(case, bars=n, bar_phase=0.5, gl_storage=G.GL_STORAGE_UPLOAD)), streams, GA | G.OP_BARS)
        z = G.Batch(G.Params(**_kw(case, bars=n, bar_phase=0.5)), streams, GA | G.OP_BARS)
        of_a, of_z = (torch.zeros((streams * 2, n), device="cuda") for _ in range(2))
        ot_a, ot_z = (torch.zeros((streams * 2, n), dtype=torch.int16, device="cuda") for _ in range(2))
        chain = G.OP_FFT | GA
        for fr in range(_updates(case)):
            x = _pcm(case, fr)[1]
            kind = fr % 3
            if kind == 0:      # bars on 3; the twin advances its state with a plain call
                a.process_s16(x, ot_a, chain | G.OP_BARS | G.OP_R16); z.process_s16(x, of_z, chain)
            elif kind == 1:
                a.process_s16(x, of_a, chain); z.process_s16(x, of_z, chain)
                assert _eq(of_a, of_z), (case, fr)
            else:
                a.process_s16(x, ot_a, chain | G.OP_R16); z.process_s16(x, ot_z, chain | G.OP_R16)
                assert _eq(ot_a, ot_z), (case, fr)
        assert a.algorithmic_bytes(chain | G.OP_BARS | G.OP_R16) == z.algorithmic_bytes(chain | G.OP_BARS | G.OP_R16)
        a.set_params(G.Params(**_kw(case, bars=n, bar_phase=0.5, gl_storage=2)))
        a.set_params(G.Params(**_kw(case, bars=n, bar_phase=0.5, gl_storage=0)))
        for fr in range(2):
            x = _pcm(case, fr)[1]
            a.process_s16(x, of_a, chain); z.process_s16(x, of_z, chain)
            assert _eq(of_a, of_z), (case, "after the switch", fr)
        # ... and back: 0 -> 3 makes the integer tables and the rows between the launches
        a.set_params(G.Params(**_kw(case, bars=n, bar_phase=0.5, gl_storage=3)))
        assert a.bars_arithmetic() == G.BARS_I8_EXACT
        x = _pcm(case, 2)[1]
        a.process_s16(x, ot_a, chain | G.OP_BARS | G.OP_R16); z.process_s16(x, ot_z, chain | G.OP_R16)
        torch.cuda.synchronize()
        u, got = ot_z.cpu().numpy().view(np.uint16), ot_a.cpu().numpy().view(np.uint16)
        for r in (0, streams * 2 - 1):
            assert (got[r] == Oracle.bars_int(u[r], n, 0.025, 0.5)[0]).all(), (case, r)
        a.close(); z.close()


@pytest.mark.parametrize("kind", ["f32", "f32_stereo", "ring_s16", "ring_f32"])
def test_other_input_kinds(glvlib, kind):
    """every input kind of a process call: the snapped bars of the one-launch class against the two-launch route, and the pass against the oracle over the
    upload of a gl_storage 0 twin"""
    import torch
    from gpu_lib import bars_mask, update_inputs
    G = glvlib
    n, streams = 4096, 3
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    mask = bars_mask(G, kind, False)
    radial = radial_bar_texels(n, 160)[0].astype(np.int64)
    kw = dict(n=n, gl_storage=G.GL_STORAGE_UPLOAD)
    one = G.Batch(G.Params(bars=len(radial), **kw), streams, mask); one.set_bar_texels(radial)
    ps = G.Batch(G.Params(bars=n, bar_phase=0.5, **kw), streams, mask)
    twin = G.Batch(G.Params(n=n), streams, mask & ~G.OP_BARS)
    o1 = torch.zeros((streams * 2, len(radial)), dtype=torch.int16, device="cuda")
    op = torch.zeros((streams * 2, n), dtype=torch.int16, device="cuda"); U = torch.zeros_like(op)
    for fr in range(3):
        meth, x, extra = update_inputs(kind, streams, n, fr)
        getattr(one, meth)(x, *extra, o1, G.OP_FFT | GA | G.OP_BARS | G.OP_R16)
        assert one.last_launches() == 1
        getattr(ps, meth)(x, *extra, op, G.OP_FFT | GA | G.OP_BARS | G.OP_R16)
        assert ps.last_launches() == 2
        getattr(twin, meth)(x, *extra, U, G.OP_FFT | GA | G.OP_R16)
        torch.cuda.synchronize()
        u, gp, g1 = U.cpu().numpy().view(np.uint16), op.cpu().numpy().view(np.uint16), o1.cpu().numpy().view(np.uint16)
        for r in range(streams * 2):
            t = Oracle.bars_int(u[r], n, 0.025, 0.5)[0]
            assert (gp[r] == t).all() and (g1[r] == t[radial]).all(), (kind, fr, r)
    for b in (one, ps, twin): b.close()


def test_wave_with_bars_as_on_gl_storage_1(glvlib):
    import torch
    G = glvlib
    n, streams = 4096, 5
    mask = G.OP_WAVE | G.OP_BARS
    ops = G.OP_WAVE | G.OP_BARS | G.OP_R16
    a = G.Batch(G.Params(n=n, bars=n, bar_phase=0.5, gl_storage=G.GL_STORAGE_UPLOAD), streams, mask)
    z = G.Batch(G.Params(n=n, bars=n, bar_phase=0.5, gl_storage=1), streams, mask)
    oa = torch.zeros((streams * 2, n), dtype=torch.int16, device="cuda"); oz = torch.zeros_like(oa)
    for fr in range(2):
        x = torch.from_numpy(lcg_pcm_fast(610 + fr, streams * 2 * n)).cuda()
        a.process_s16(x, oa, ops); z.process_s16(x, oz, ops)
        assert (a.last_launches(), a.kernel_name()) == (z.last_launches(), z.kernel_name())
        assert _eq(oa, oz), fr
        xf = (x.to(torch.float32) / 32768).contiguous()
        a.process_f32_stereo(xf, oa, ops); z.process_f32_stereo(xf, oz, ops)
        assert a.last_launches() == z.last_launches() == 2
        assert _eq(oa, oz), fr
    assert bool((oa != 0).any())
    a.close(); z.close()
    # the single-stream drop-in's pass takes a state created with 3
    rows = (np.random.default_rng(3).standard_normal(n) * 0.2).astype(np.float32)
    ta, tz = np.zeros(n, np.uint16), np.zeros(n, np.uint16)
    sa = G.State(G.Params(n=n, bars=n, bar_phase=0.5, gl_storage=G.GL_STORAGE_UPLOAD)); sz = G.State(G.Params(n=n, bars=n, bar_phase=0.5, gl_storage=1))
    sa.wave_texture(rows, ta, True); sz.wave_texture(rows, tz, True)
    assert (ta == tz).all() and ta.any()
    sa.close(); sz.close()


def test_refusals_leave_the_batch_usable(glvlib):
    import torch
    G = glvlib
    n, streams = 1024, 3
    case = (n, streams, 5, 2, 1)
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    chain = G.OP_FFT | GA
    x = _pcm(case, 0)[1]

    def refused(code, fn):
        with pytest.raises(G.GlvError) as ei:
            fn()
        assert ei.value.code == code, (ei.value.code, str(ei.value))
        assert str(ei.value)

    with pytest.raises(G.GlvError) as ei:
        G.Batch(G.Params(n=n, gl_storage=4), streams, GA)
    assert ei.value.code == G.ERR_INVALID
    b = G.Batch(G.Params(**_kw(case, bars=80, gl_storage=G.GL_STORAGE_UPLOAD)), streams, GA | G.OP_BARS | G.OP_SMOOTH)
    twin = G.Batch(G.Params(**_kw(case, bars=80)), streams, GA | G.OP_SMOOTH)
    o80 = torch.zeros((streams * 2, 80), device="cuda"); o80t = torch.zeros((streams * 2, 80), dtype=torch.int16, device="cuda")
    of, ofz = torch.zeros((streams * 2, n), device="cuda"), torch.zeros((streams * 2, n), device="cuda")
    assert b.bars_arithmetic() == G.BARS_F32_CHAIN
    refused(G.ERR_STATE, lambda: b.process_s16(x, o80, chain | G.OP_BARS))                     # unsnapped 80 averaging bars
    refused(G.ERR_STATE, lambda: b.process_s16(x, o80t, chain | G.OP_BARS | G.OP_R16))
    refused(G.ERR_STATE, lambda: b.bars(of, o80))                                              # caller's float rows: a gl_storage 0 batch
    radial = radial_bar_texels(n, 160)[0]
    b.set_bar_texels(radial)
    refused(G.ERR_STATE, lambda: b.process_s16(x, o80, chain | G.OP_SMOOTH | G.OP_BARS))       # SMOOTH | BARS
    refused(G.ERR_STATE, lambda: b.process_s16(x, o80, G.OP_FFT | G.OP_RAW | G.OP_BARS))
    refused(G.ERR_STATE, lambda: b.set_params(G.Params(**_kw(case, bars=80, gl_storage=1))))    # 3 -> 1: another state class
    refused(G.ERR_STATE, lambda: b.set_params(G.Params(**_kw(case, bars=80, gl_storage=0))))    # a table is set: 0 has no texture for it
    b.set_bar_texels(None)
    table = graph_column_texels(n, 120)[0]
    cb = G.Batch(G.Params(**_kw(case, bars=len(table), gl_storage=G.GL_STORAGE_UPLOAD)), streams, GA | G.OP_BARS)
    cb.set_column_texels(table)
    oc16 = torch.zeros((streams * 2, len(table)), dtype=torch.int16, device="cuda")
    refused(G.ERR_STATE, lambda: cb.process_s16(x, oc16, chain | G.OP_BARS | G.OP_R16))         # R16 with columns
    refused(G.ERR_STATE, lambda: cb.process_s16(x, oc16, G.OP_WAVE | G.OP_R16))
    z = G.Batch(G.Params(**_kw(case, bars=80)), streams, GA | G.OP_BARS)
    refused(G.ERR_STATE, lambda: z.set_bar_texels(radial))                                      # still refused on 0
    refused(G.ERR_STATE, lambda: z.set_column_texels(graph_column_texels(n, 158)[0]))
    one = G.Batch(G.Params(**_kw(case, gl_storage=1, bars=80)), streams, GA | G.OP_BARS)
    refused(G.ERR_STATE, lambda: one.set_params(G.Params(**_kw(case, gl_storage=G.GL_STORAGE_UPLOAD, bars=80))))   # 1 -> 3
    # nothing above touched the state or the tables: the batch runs on, in step with a gl_storage 0 batch that saw none of it; without bars
    # GLV_OP_SMOOTH is what it is on 0
    for fr in range(3):
        xx = _pcm(case, fr)[1]
        ops = chain | (G.OP_SMOOTH if fr == 1 else 0)
        b.process_s16(xx, of, ops); twin.process_s16(xx, ofz, ops)
        assert _eq(of, ofz), fr
    b.set_bar_texels(radial)
    b.process_s16(x, o80, chain | G.OP_BARS)
    oc = torch.zeros((streams * 2, len(table)), device="cuda")
    cb.process_s16(x, oc, chain | G.OP_BARS)
    torch.cuda.synchronize()
    assert np.isfinite(o80.cpu().numpy()).all() and np.isfinite(oc.cpu().numpy()).all()
    for y in (b, twin, cb, z, one): y.close()


def test_graph_capture_of_first_call(glvlib):
    """process calls never allocate: the first call of each route can be captured"""
    import torch
    G = glvlib
    n, streams = 4096, 5
    case = (n, streams, 5, 2, 1)
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    radial = radial_bar_texels(n, 160)[0].astype(np.int64)
    ops = G.OP_FFT | GA | G.OP_BARS | G.OP_R16
    x = _pcm(case, 0)[1]
    ref = G.Batch(G.Params(**_kw(case, bars=n, bar_phase=0.5, gl_storage=G.GL_STORAGE_UPLOAD)), streams, GA | G.OP_BARS)
    want = torch.zeros((streams * 2, n), dtype=torch.int16, device="cuda")
    ref.process_s16(x, want, ops)
    for tex in (None, radial):
        bars = n if tex is None else len(tex)
        b = G.Batch(G.Params(**_kw(case, bars=bars, bar_phase=0.5, gl_storage=G.GL_STORAGE_UPLOAD)), streams, GA | G.OP_BARS)
        if tex is not None: b.set_bar_texels(tex)
        o = torch.zeros((streams * 2, bars), dtype=torch.int16, device="cuda")
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            b.process_s16(x, o, ops, stream=s.cuda_stream)
        g.replay()
        torch.cuda.synchronize()
        assert _eq(o, want if tex is None else want[:, torch.from_numpy(tex).cuda()].contiguous())
        del g
        b.close()
    ref.close()
