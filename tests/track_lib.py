"""The harness of the GPU track tests (test_track*.py, and the track sections of test_forced_grid.py, test_frame_count.py and test_knob_changes.py): a
plain module, like oracle_lib.py and src_scan.py (default collection does not pick it up; torch is imported inside the functions, as in the tests).

The shared contract: step t of a track call's output, and for stateful chains the batch's state afterwards, are bit for bit what `steps` consecutive
glv_batch_process_s16 / glv_batch_process_f32_stereo calls on the windows produce and leave behind.  The sequential side is a second batch driven window
by window (`seq`), the windows cut on the host from the same recording (`windows`); floats are compared as int32 (`eq`).  Every call made through `track`
gets a workspace of exactly the queried size and an output of exactly steps * streams * 2 * w elements, each followed by a guard region that must come
back intact, and a call that reports one launch must leave the workspace untouched -- for every entry, whichever file calls.  What differs per entry
(launch counts, kernel names, pitches, chains) stays stated in the entry's test file."""
import numpy as np

from gpu_lib import SIZES, eq  # noqa: F401  (eq: part of this module's interface)
from oracle_lib import lcg_pcm_fast

GUARD = 4096                                                 # bytes behind the workspace, elements behind the output
ENTRIES = ("residue", "windows", "wave", "columns", "live", "at")


def out_dtype(G, ops):
    import torch
    return torch.int16 if ops & G.OP_R16 else torch.float32


def differing(a, b):
    """how many elements differ, bit for bit (an assertion's message)"""
    import torch
    ia = a.view(torch.int32) if a.dtype == torch.float32 else a
    ib = b.view(torch.int32) if b.dtype == torch.float32 else b
    return int((ia != ib).sum())


# ---- pitches ------------------------------------------------------------------------------------------------------------------------------------------
def pitch_residue(n, hop, steps):
    """a multiple of the hop where n is one, as glv_batch_track_s16 asks: three hops of slack behind the last window"""
    return n + (steps - 1) * hop + 3 * hop


def pitch_odd(n, hop, steps):
    """odd, slack behind the last window: nothing but "long enough" is asked of it"""
    return (n + (steps - 1) * hop + 38) | 1


# ---- recordings ---------------------------------------------------------------------------------------------------------------------------------------
def pcm(seed, streams, pitch):
    """int16 [streams][pitch][2], every stream at a level of its own; a new array on every call, the caller's to write"""
    x = lcg_pcm_fast(seed, streams * pitch * 2).reshape(streams, pitch, 2).copy()
    for s in range(streams):
        x[s] //= (1, 8, 64)[s % 3]
    return x


_RECORDINGS = {}


def rec(seed, streams, pitch, f32=True):
    """float32 (f32) or int16 [streams][pitch][2], every stream at a level of its own: made once per shape and seed, shared, never written (a test that
    plants samples takes a copy)"""
    key = (seed, streams, pitch, f32)
    if key not in _RECORDINGS:
        if f32:
            x = (np.random.default_rng(seed).standard_normal((streams, pitch, 2)) * 0.3).astype(np.float32)
            for s in range(streams):
                x[s] *= np.float32((1.0, 0.125, 0.015625)[s % 3])
        else:
            x = pcm(seed, streams, pitch)
        x.setflags(write=False)
        if len(_RECORDINGS) > 64:
            _RECORDINGS.clear()
        _RECORDINGS[key] = x
    return _RECORDINGS[key]


def to_device(x, odd, f32, tail_frames=0):
    """the recording on the device: at a load boundary (8 bytes for s16, 16 for f32), or with `odd` one frame behind one.  tail_frames: that many frames of
    another pattern follow the last stream in the same allocation, so that a read past the recording shows as wrong bits and never leaves the allocation.
    Returns the view of the recording; it holds the whole allocation, the tail included"""
    import torch
    assert x.dtype == (np.float32 if f32 else np.int16)
    unit = 16 if f32 else 8
    flat = torch.zeros((x.size + 2 * tail_frames + 4,), dtype=torch.float32 if f32 else torch.int16, device="cuda")
    assert flat.data_ptr() % unit == 0
    off = 2 if odd else 0
    view = flat[off:off + x.size]
    view.copy_(torch.from_numpy(np.array(x, copy=True).reshape(-1)))                  # (a copy: the shared recordings are read-only)
    if tail_frames:
        tail = (np.arange(2 * tail_frames) % 251 + 3).astype(x.dtype)
        if f32:
            tail = tail / np.float32(300)
        flat[off + x.size:off + x.size + 2 * tail_frames].copy_(torch.from_numpy(tail))
    assert view.data_ptr() % unit == (unit // 2 if odd else 0)
    return view


# ---- the sequential side ------------------------------------------------------------------------------------------------------------------------------
def windows(x, n, starts):
    """the sequential side's inputs: the n frames of every stream from each of `starts` on, [streams][n][2] contiguous.  The hop entries' window t starts
    at t * hop; the table entry's at the clamped start (G.track_at_start)"""
    import torch
    return [torch.from_numpy(np.ascontiguousarray(x[:, a:a + n, :])).cuda() for a in starts]


def hop_windows(x, n, hop, t0, t1):
    """windows t0 .. t1 - 1 of a recording walked at `hop`"""
    return windows(x, n, [t * hop for t in range(t0, t1)])


def seq(b, wins, ops, w, dt, f32=False):
    """one process call per window, one synchronize; the results stacked [len(wins)][streams * 2][w]"""
    import torch
    outs = []
    for x in wins:
        o = torch.zeros((b.streams * 2, w), dtype=dt, device="cuda")
        (b.process_f32_stereo if f32 else b.process_s16)(x, o, ops)
        outs.append(o)
    torch.cuda.synchronize()
    return torch.stack(outs)


# ---- one track call -----------------------------------------------------------------------------------------------------------------------------------
def _sentinel(dt):
    import torch
    return 23130 if dt == torch.int16 else -7.0


def track(b, entry, d_pcm, pitch, hop, steps, ops, w, dt, t0=0, f32=False, stream=None, fill=0xA5, keep_work=False):
    """steps [t0, t0 + steps) in one call of glv_batch_track_<entry>_s16 / _f32 (`residue`: glv_batch_track_s16).  For `at`, `hop` is the device table of
    window starts and t0 moves the table pointer; for every other entry t0 moves d_pcm by t0 hops.  The workspace is exactly as large as the entry's query
    asks, filled with `fill`; the output exactly steps * streams * 2 * w elements of zeros; a guard behind each.  Checked on every call: both guards, and
    an untouched workspace where the call reports one launch.  Returns the output [steps][streams * 2][w] (keep_work: and the workspace, without its guard)"""
    import torch
    assert entry in ENTRIES and not (entry == "residue" and f32), entry
    kind = "f32" if f32 else "s16"
    if entry == "at":
        nbytes = b.track_at_work_bytes(steps, ops)
        call, where, how = getattr(b, f"track_at_{kind}"), d_pcm.data_ptr(), hop.data_ptr() + 4 * t0
    else:
        form = "track" if entry == "residue" else f"track_{entry}"
        nbytes = getattr(b, f"{form}_work_bytes")(pitch, hop, steps, ops)
        call, where, how = getattr(b, f"{form}_{kind}"), d_pcm.data_ptr() + t0 * hop * (8 if f32 else 4), hop
    work = torch.full((nbytes + GUARD,), fill, dtype=torch.uint8, device="cuda")
    assert work.data_ptr() % 256 == 0
    work[nbytes:] = 0xA5
    count = steps * b.streams * 2 * w
    flat = torch.zeros((count + GUARD,), dtype=dt, device="cuda")
    flat[count:] = _sentinel(dt)
    call(where, pitch, how, steps, flat, work, ops, stream=stream)
    torch.cuda.synchronize()
    assert bool((work[nbytes:] == 0xA5).all()), "the call wrote behind the workspace it asked for"
    assert bool((flat[count:] == _sentinel(dt)).all()), "the call wrote behind its output"
    if b.last_launches() == 1:
        assert bool((work[:nbytes] == fill).all()), "a call that runs in one launch touched the workspace"
    out = flat[:count].view(steps, b.streams * 2, w)
    return (out, work[:nbytes]) if keep_work else out


def compare(G, bt, bs, entry, x, d_pcm, pitch, hop, starts, n, steps, ops, w, launches, name, f32=False, state=True, what=()):
    """one call of `entry` on bt against the sequential calls on bs, every step; with `state`, the state both are left in, through one more update on
    each.  x: the host recording behind d_pcm; starts: where the windows lie in it, `steps` of them and with `state` one more; hop: as `track` takes it;
    launches, name: what glv_batch_last_launches and glv_batch_kernel_name report for the form, which the calling file states (None: not asserted).
    Returns the call's output"""
    assert len(starts) == steps + (1 if state else 0)
    dt = out_dtype(G, ops)
    got = track(bt, entry, d_pcm, pitch, hop, steps, ops, w, dt, f32=f32)
    if launches is not None:
        assert bt.last_launches() == launches, (bt.last_launches(), *what)
    if name is not None:
        assert bt.kernel_name() == name, (bt.kernel_name(), *what)
    wins = windows(x, n, starts)
    want = seq(bs, wins[:steps], ops, w, dt, f32)
    for t in range(steps):
        assert eq(got[t], want[t]), (*what, t, differing(got[t], want[t]))
    if state:
        assert eq(seq(bt, wins[steps:], ops, w, dt, f32), seq(bs, wins[steps:], ops, w, dt, f32)), (*what, "state")
    return got


def compare_hop(G, bt, bs, entry, x, odd, pitch, hop, n, steps, ops, w, launches, name, f32=False, state=True, what=()):
    """`compare` for the entries that walk the recording at a hop, the recording put at a load boundary or (odd) one frame behind one"""
    starts = [t * hop for t in range(steps + (1 if state else 0))]
    return compare(G, bt, bs, entry, x, to_device(x, odd, f32), pitch, hop, starts, n, steps, ops, w, launches, name, f32=f32, state=state, what=(hop, odd) + what)


# ---- what several entries' files state alike ------------------------------------------------------------------------------------------------------------
def launches_fft(G, ops):
    """launches of an FFT chain through the windows form: the transform, the scan where there is state, the bars"""
    state = bool(ops & (G.OP_GRAVITY | G.OP_AVERAGE))
    return 1 + (1 if state else 0) + (1 if ops & G.OP_BARS else 0)


def fft_kernel(G, ops):
    return "glv_track_scan_kernel" if ops & (G.OP_GRAVITY | G.OP_AVERAGE) else "glv_frame_kernel"


def with_table(b, table):
    """table: None, ("bar", bar texels) or ("col", column texels)"""
    if table: (b.set_bar_texels if table[0] == "bar" else b.set_column_texels)(table[1])
    return b


def bars_batch(G, n, kw, table, F, streams, live=True, variant=None):
    """a gravity | average | bars batch with its table set; live: created with GLV_OP_BARS_ONLY"""
    mask = G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS | (G.OP_BARS_ONLY if live else 0)
    b = with_table(G.Batch(G.Params(n=n, avg_frames=F, **kw), streams, mask), table)
    if variant is not None: b.set_variant(variant)
    return b


def work_regions(work, rows, n, e1, e2):
    """the two regions of a three-launch call's workspace, each with its element size: the transform's rows, then the scan's"""
    up = lambda v_: (v_ + 255) & ~255                                    # noqa: E731
    r1 = up(rows * n * e1)
    assert work.numel() == r1 + up(rows * n * e2), (work.numel(), r1, e2)
    return (work[:r1], e1), (work[r1:], e2)


def base_chains(G):
    """name -> (parameters, creation mask, ops): the chains every FFT entry's file runs alike.  `gl_chain_F1` is not among them: it carries GLV_OP_R16 in
    the s16 files and not in tests/test_track_f32.py, which has a `gl_chain_F1_r16` beside it"""
    S, GA = G.OP_GRAVITY, G.OP_GRAVITY | G.OP_AVERAGE
    return {
        "fft":             (dict(), G.OP_FFT, G.OP_FFT),
        "fft_r16":         (dict(), G.OP_FFT, G.OP_FFT | G.OP_R16),
        "gravity":         (dict(), S, G.OP_FFT | S),
        "chain":           (dict(), GA, G.OP_FFT | GA),
        "chain_plain_sum": (dict(avg_window=False, avg_frames=3), GA, G.OP_FFT | GA),
        "chain_r16":       (dict(), GA, G.OP_FFT | GA | G.OP_R16),
        "chain_mono":      (dict(channels=1), GA, G.OP_FFT | GA),
        "average":         (dict(), G.OP_AVERAGE, G.OP_FFT | G.OP_AVERAGE),
        "gl_gravity":      (dict(gl_storage=1), S, G.OP_FFT | S | G.OP_R16),
        "gl_chain":        (dict(gl_storage=1, avg_window_kind=1), GA, G.OP_FFT | GA),
        "gl_chain_r16":    (dict(gl_storage=1, avg_window_kind=1), GA, G.OP_FFT | GA | G.OP_R16),
        "gl_chain_mono":   (dict(gl_storage=1, channels=1), GA, G.OP_FFT | GA | G.OP_R16),
        "gl_fft":          (dict(gl_storage=1), G.OP_FFT, G.OP_FFT),
    }


def s16_chains(G):
    """the chains of the s16 files (test_track.py, test_track_windows.py and those that run its chains): gl_chain_F1 as texels"""
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    return {**base_chains(G), "gl_chain_F1": (dict(gl_storage=1, avg_frames=1), GA, G.OP_FFT | GA | G.OP_R16)}


S16_CHAIN_NAMES = ["fft", "fft_r16", "gravity", "chain", "chain_plain_sum", "chain_r16", "chain_mono", "average", "gl_gravity", "gl_chain", "gl_chain_r16",
                   "gl_chain_F1", "gl_chain_mono", "gl_fft"]
# (n, kernel configuration): every size and every configuration IN_S16_TRACK is built for (SIZES).  At 256 / 512 several slots share a wave (the load form's
# branch may diverge; 512 configuration 1 puts four windows in one wave), 1024 is the smallest size where none does.  The three entries that carry the
# full chain list came first; the others run the chains that differ in the transform launch: step-major rows straight into d_out (fft, fft_r16),
# stream-major rows for the scan (chain, gl_chain_r16) and the mono mix
S16_FULL_SIZES = [(256, 0), (1024, 0), (1024, 1)]
REDUCED_CHAINS = ["fft", "fft_r16", "chain", "gl_chain_r16", "chain_mono"]
S16_CHAIN_SIZES = [(c, n, v) for c in S16_CHAIN_NAMES for n, v in SIZES if (n, v) in S16_FULL_SIZES or c in REDUCED_CHAINS]
