"""CPU: track mode at render frames (glv_batch_track_frames_s16 / _f32) without a device -- the exported symbols and their Python prototypes,
glava_amd.track_starts.keyframe_tables against the reference's REAL rd_update with `setinterpolate true` (over the null GL of integration/nullgl_harness.c, the
method of tests/test_handle_audio.py), live_session_frames against a literal restatement of the counters of render.c:2379-2399 written here, and the path's
freedom from allocating / synchronising HIP calls (the method of tests/test_track_at_host.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from glava_amd.track_starts import keyframe_tables, live_session_frames, live_session_rates
from oracle_lib import Oracle, StreamOracle, lcg_pcm_fast
from src_scan import ROOT, TRACK_COMMON, TRACK_EXECUTOR, assert_launch_only, function_body, read_csrc, read_host_src, strip_comments

F32 = np.float32
SYMBOLS = ("glv_batch_track_frames_work_bytes", "glv_batch_track_frames_s16", "glv_batch_track_frames_f32")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_track_frames_symbols_are_exported_bound_and_declared(glvlib):
    L = C.CDLL(glvlib.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(L, name), name
    lib = glvlib.lib()
    assert lib.glv_batch_track_frames_work_bytes.restype is C.c_uint64
    assert len(lib.glv_batch_track_frames_work_bytes.argtypes) == 4
    assert len(lib.glv_batch_track_frames_s16.argtypes) == 11 and len(lib.glv_batch_track_frames_f32.argtypes) == 11
    for meth in ("track_frames_work_bytes", "track_frames_s16", "track_frames_f32"):
        assert callable(getattr(glvlib.Batch, meth)), meth
    header = open(os.path.join(ROOT, "include", "glv_spectrum.h")).read()
    for name in SYMBOLS:
        assert name + "(" in header, name
    assert "w = s + ((e - s) * d_mod[j])" in header                              # the expression is part of the contract
    assert lib.glv_abi_version() == 7                                            # added within the ABI: detected by the symbol


def test_the_python_mirror_of_glv_track_frames_has_the_headers_layout(glvlib, tmp_path):
    import subprocess
    fields = [f[0] for f in glvlib.TrackFrames._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "glv_spectrum.h"\nint main(void){ printf("%zu", sizeof(glv_track_frames));\n'
                   + "".join(f'printf(" %zu", offsetof(glv_track_frames, {f}));\n' for f in fields) + "return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == C.sizeof(glvlib.TrackFrames) and got[1:] == [getattr(glvlib.TrackFrames, f).offset for f in fields]


def test_track_frames_refuses_without_a_device(glvlib):
    lib = glvlib.lib()
    ops = glvlib.OP_FFT | glvlib.OP_R16
    fr = glvlib.TrackFrames()
    assert lib.glv_batch_track_frames_work_bytes(None, 1, 1, ops) == 0
    assert lib.glv_last_error().decode().startswith("batch is NULL")
    assert lib.glv_batch_track_frames_s16(None, None, 0, None, None, 0, C.byref(fr), None, None, ops, None) == glvlib.ERR_INVALID
    assert lib.glv_batch_track_frames_f32(None, None, 0, None, None, 0, None, None, None, ops, None) == glvlib.ERR_INVALID


# ---- keyframe_tables against the compiled reference ---------------------------------------------------------------------------------------------------
N = 512
#           a run of 0, of 1, of six (kcounter reaches 5), of two unmodified frames
MODIFIED = [True, True, False, True, False, False, False, False, False, False, True, True, False, False, True]


def _reference_uploads(ur, fr):
    """the reference's rd_update with interpolate = 1 and fixed ur / fr over MODIFIED: a frame with an update gets a new snapshot, a frame without one the
    buffers as the previous frame left them (glava.c:528-537 copies only when `modified`).  Returns the uploads and the int16 input of every update"""
    from test_handle_audio import REF_SO, cfg, load
    L = load(REF_SO)
    updates = sum(MODIFIED)
    pcm = lcg_pcm_fast(9100, updates * 2 * N).reshape(updates, N, 2)
    snaps = (pcm.astype(np.float32) / np.float32(65535)).transpose(0, 2, 1).copy()        # fifo.c:105-106
    c = cfg(N, interpolate=1, ur=ur, fr=fr)
    h = L.nullgl_create(C.byref(c))
    assert h
    lb, rb = np.zeros(N, np.float32), np.zeros(N, np.float32)
    ups, t = [], 0
    for m in MODIFIED:
        if m:
            lb, rb = snaps[t][0].copy(), snaps[t][1].copy()
            t += 1
        ul, ur_ = np.zeros(N, np.float32), np.zeros(N, np.float32)
        k = C.c_size_t(0)
        assert L.nullgl_update(h, lb, rb, N, int(m), ul, ur_, C.byref(k)) == 2 and k.value == N
        ups.append(np.stack([ul, ur_]))
    L.nullgl_destroy(h)
    return ups, pcm.reshape(updates, 2 * N)


@pytest.mark.parametrize("ur,fr", [(36.0, 120.0), (100.0, 110.0)], ids=["uratio0.3", "uratio0.909"])
def test_keyframe_tables_predict_what_the_reference_uploads(oracle, ur, fr):
    ups, pcm = _reference_uploads(ur, fr)
    uratio = float(F32(ur) / F32(fr))
    frames = len(MODIFIED)
    frm, to, mod, keep_from, keep_to = keyframe_tables(MODIFIED, [True] * frames, [uratio] * frames)
    assert len(frm) == len(to) == len(mod) == frames >= 12
    # the keyframes in the call's indexing: zeros (the harness zero-fills, as d_keys is before a session's first call), then the oracle chain's finished rows
    so = StreamOracle(N, avg_frames=5, ur=ur)
    keys = [np.zeros((2, N), np.float32), np.zeros((2, N), np.float32)] + [so.frame(p).copy() for p in pcm]
    lerped = 0
    kcounter = 0
    for j in range(frames):
        if frm[j] == to[j]:
            want = keys[frm[j]]
        else:
            s, e = keys[frm[j]], keys[to[j]]
            want = (s + ((e - s).astype(F32) * F32(mod[j])).astype(F32)).astype(F32)
            ref = np.empty((2, N), np.float32)
            for ch in range(2):
                Oracle.lib().glvo_lerp(np.ascontiguousarray(s[ch]), np.ascontiguousarray(e[ch]), ref[ch], N, F32(uratio), kcounter)
            assert (bits(want) == bits(ref)).all(), j                            # the numpy expression and the table's mod are the oracle's lerp
            lerped += 1
        assert (bits(ups[j]) == bits(want)).all(), (j, frm[j], to[j], mod[j])
        kcounter = 0 if MODIFIED[j] else kcounter + 1
    if uratio <= 0.9:
        assert lerped == frames and sum(1 for m in mod if m == 1.0) >= 2 and F32(uratio) * F32(5) > 1    # more than one clamped modifier
        assert 0.0 in mod and any(0.0 < m < 1.0 for m in mod)
        assert (frm[0], to[0]) == (0, 1) and (keep_from, keep_to) == (2 + sum(MODIFIED) - 2, 2 + sum(MODIFIED) - 1)
    else:
        # above 0.9 the reference forces interpolation off: every frame uploads its buffer, the keyframes are never pushed
        assert lerped == 0 and (keep_from, keep_to) == (0, 1)
        steps_seen = np.cumsum(MODIFIED) - 1
        assert frm == to == [2 + int(t) for t in steps_seen]


def test_keyframe_tables_counters_and_stale_keyframes():
    """the pushes happen under `on and modified` only: while interpolation is off the keyframes go stale, and it resumes from the stale pair"""
    modified = [True, False, True, True, False, True, False, False]
    on = [True, True, False, False, False, True, True, True]
    frm, to, mod, kf, kt = keyframe_tables(modified, on, [0.5] * 8)
    #            lerp(0,1)  lerp(1,2)  buffer   buffer   buffer  lerp(1,2) stale  lerp(2,5) ...
    assert frm == [0, 1, 3, 4, 4, 1, 2, 2] and to == [1, 2, 3, 4, 4, 2, 5, 5]
    assert mod == [0.0, 0.0, 0.0, 0.0, 0.0, 0.5, 0.0, 0.5] and (kf, kt) == (2, 5)
    # a frame without an update before the call's first one shows keyframe 1 when interpolation is off
    assert keyframe_tables([False, True], [False, False], [0.5, 0.5])[:2] == ([1, 2], [1, 2])
    # mod is a float32 product, clamped
    frm, to, mod, _, _ = keyframe_tables([True] + [False] * 6, [True] * 7, [0.3] * 7)
    assert mod == [0.0] + [float(min(F32(0.3) * F32(k), F32(1.0))) for k in range(6)] and mod[-1] == 1.0 and mod[-2] == 1.0 and mod[-3] < 1.0
    for bad in (([], [], []), ([True], [True, True], [0.5])):
        with pytest.raises(ValueError):
            keyframe_tables(*bad)
    with pytest.raises(ValueError):
        keyframe_tables([True], [True], [0.5], kcounter=-1)


@pytest.mark.parametrize("cut", [3, 4, 9, 10, 11])
def test_keyframe_tables_of_a_session_cut_into_calls(cut):
    """a call that starts with the kcounter its predecessor ended on gives the uncut session's tables, in its own indexing: 0 and 1 are what the predecessor
    kept, 2 + t its own step t"""
    modified = [True, False, True, True, False, False, True, False, False, False, True, True, False, True, False, False]
    on = [True] * len(modified)
    uratio = [0.4] * len(modified)
    whole = keyframe_tables(modified, on, uratio)
    first = keyframe_tables(modified[:cut], on[:cut], uratio[:cut])
    idle = 0
    while not modified[cut - 1 - idle]: idle += 1
    rest = keyframe_tables(modified[cut:], on[cut:], uratio[cut:], kcounter=idle)
    done = sum(modified[:cut])                                                   # steps of the first call
    names = {0: first[3], 1: first[4]}                                           # the second call's keyframes 0 and 1 in the first call's indexing, which is the session's
    session = lambda k: names[k] if k < 2 else k + done                          # noqa: E731
    assert first[0] == whole[0][:cut] and first[1] == whole[1][:cut] and first[2] == whole[2][:cut]
    assert [session(k) for k in rest[0]] == whole[0][cut:] and [session(k) for k in rest[1]] == whole[1][cut:] and rest[2] == whole[2][cut:]
    assert (session(rest[3]), session(rest[4])) == whole[3:]


# ---- live_session_frames ------------------------------------------------------------------------------------------------------------------------------------
def _walk(rate, fps, frames, update_frames):
    """render.c:1760-1763, :1804-1805, :2347-2353, :2379-2399 frame by frame, independent of the module: ur and fr start at 1.0F (:905-906); returns per frame
    (interpolates, start, end, shown, mod) in keyframe indices, and the keyframes after the last frame"""
    ur, fr = F32(1.0), F32(1.0)
    tcounter, ucounter, fcounter, kcounter, shown_updates = 0.0, 0, 0, 0, 0
    start, end, row, step = 0, 1, 1, 0
    out = []
    for j in range(frames):
        updates = (j * rate // fps) // update_frames
        modified = updates != shown_updates
        uratio = F32(ur / fr)                                  # :1761
        interpolate = bool(uratio <= F32(0.9))                 # :1763
        if modified:
            shown_updates = updates
            row = 2 + step
            step += 1
        m = F32(uratio * F32(kcounter))                        # :1804
        if m > F32(1.0): m = F32(1.0)                          # :1805
        out.append((interpolate, start, end, row, float(m)))
        if interpolate and modified: start, end = end, row     # :2347-2353
        fcounter += 1                                          # :2379
        if modified: ucounter += 1; kcounter = 0               # :2380-2382
        else: kcounter += 1                                    # :2383
        tcounter += 1.0 / float(fps)                           # :2384
        if tcounter >= 1.0:                                    # :2385
            fr = F32(fcounter / tcounter); ur = F32(ucounter / tcounter)        # :2386-2387
            tcounter, ucounter, fcounter = 0.0, 0, 0           # :2397-2399
    return out, (start, end)


@pytest.mark.parametrize("fps", [60, 144, 30, 100])
def test_live_session_frames_follow_the_reference_counters(fps):
    rate, update_frames = 22050, 256
    frames = 4 * fps + 7
    starts, ur, frm, to, mod, kf, kt = live_session_frames(rate, fps, frames, update_frames)
    s2, _, ur2 = live_session_rates(rate, fps, frames, update_frames)
    assert starts == s2 and ur == ur2                                            # the updates are live_session_rates' own
    walk, keep = _walk(rate, fps, frames, update_frames)
    assert len(frm) == len(to) == len(mod) == frames and (kf, kt) == keep
    for j, (interpolate, start, end, row, m) in enumerate(walk):
        if interpolate: assert (frm[j], to[j], mod[j]) == (start, end, m), j
        else: assert frm[j] == to[j] == row, j
    assert max(max(frm), max(to)) < len(starts) + 2 and kt < len(starts) + 2
    assert all(isinstance(v, int) for v in frm + to) and all(isinstance(v, float) and float(F32(v)) == v for v in mod)


def test_live_session_frames_literals():
    # 60 fps: uratio is 1.0, then 59 / 60 -- interpolation never turns on, every frame shows the latest finished row and d_keys is never written
    starts, ur, frm, to, mod, kf, kt = live_session_frames(22050, 60, 200, 256)
    assert frm == to and (kf, kt) == (0, 1) and set(mod) == {0.0}
    assert frm[:4] == [1, 2, 3, 4] and frm[-1] == 2 + len(starts) - 1
    # 144 fps: the first second closes after 145 frames (144 additions of 1 / 144 stay below 1.0) with 86 updates: ur = 85.4069, fr = 144.0, uratio 0.5931
    starts, ur, frm, to, mod, kf, kt = live_session_frames(22050, 144, 160, 256)
    assert all(a == b for a, b in zip(frm[:145], to[:145])) and all(a != b for a, b in zip(frm[145:], to[145:]))
    u = F32(F32(85.40689849853516) / F32(144.0))
    assert float(u) == 0.5931034684181213
    # frames 145 ..: the keyframes are still the zeros of d_keys until two updates have been pushed -- (0, 1), then (1, k), then (k, k')
    assert list(zip(frm[145:152], to[145:152])) == [(0, 1), (0, 1), (1, 88), (1, 88), (88, 89), (89, 90), (89, 90)]
    assert mod[145:152] == [float(F32(u * F32(k))) for k in (0, 1, 0, 1, 0, 0, 1)]
    assert len(starts) == 95 and (kf, kt) == (95, 96)                            # the last update's row is keyframe 2 + 94
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            live_session_frames(22050, bad, 4, 256)


# ---- the path ---------------------------------------------------------------------------------------------------------------------------------------------
def test_track_frames_path_has_no_allocating_or_synchronising_call():
    src = read_host_src()
    assert_launch_only(src, [r"\nint plan_track_frames\(", r"\nint track_frames\(glv_batch\* b,", r"\nint track_frames_call\(", r"\nint track_rates\(glv_batch\* b,",
                             r"\nint track_at\(glv_batch\* b,", r"\nint plan_track_at\(", r"\nint windows_args\(", r"\nvoid windows_geometry\(", r"\nint plan_track_windows\(",
                             r"\nint plan_track_columns\(", r"\nint plan_track_live\(", r"\nint track_columns\(", r"\nuint64_t glv_batch_track_frames_work_bytes\(",
                             r"\nint glv_batch_track_frames_s16\(", r"\nint glv_batch_track_frames_f32\("] + TRACK_EXECUTOR + TRACK_COMMON)
    plain = strip_comments(src)
    # the entries add no stage: the frames' own refusals, then the rates call or the table call with the frames handed on
    for name in ("glv_batch_track_frames_s16", "glv_batch_track_frames_f32"):
        body = function_body(plain, r"\nint " + name + r"\(")
        assert "track_frames_call(b, d_pcm," in body and "glv::launch_" not in body and "for (" not in body, name
    body = function_body(plain, r"\nint track_frames_call\(")
    assert "track_rates(b, d_pcm," in body and "track_at(b, d_pcm," in body
    for absent in ("glv::launch_", "for (", "while (", "TrackPlan", "hipSetDevice", "b->"):
        assert absent not in body, absent                                        # nothing of the batch is read, let alone written, before the plan accepts the call
    for refusal in ("!fr", "!fr->d_from || !fr->d_to || !fr->d_mod || !fr->d_keys", "& 3u", "& 15u", "(uint64_t) steps + 2u"):
        assert refusal in body, refusal
    body = function_body(plain, r"\nint plan_track_frames\(")
    for refusal in ("frames == 0", "ops & GLV_OP_WAVE", "GLV_OP_R16 | GLV_OP_BARS", "!upload_storage(b->p)", "b->single_row", "0xffffffffull"):
        assert refusal in body, refusal
    assert "plan_track_at(b, pitch_frames, 0u, steps, ops, tp)" in body and body.count("GLV_ERR_STATE") == 2
    # the steps run through the table call's executor, which has one frames stage: two launches, no loop, in front of the bars
    body = function_body(plain, r"\nint track\(glv_batch\* b,")
    assert body.count("track_frames(b, tp,") == 1 and body.index("track_scan(") < body.index("track_frames(b, tp,") < body.index("launch_bars_pass(")
    body = function_body(plain, r"\nint track_frames\(glv_batch\* b,")
    assert body.count("glv::launch_track_frames(") == 1 and body.count("glv::launch_track_keys(") == 1 and body.count("++b->last_launches") == 2
    assert "for (" not in body and "while (" not in body
    assert plain.count("launch_track_frames(") == 1 and plain.count("launch_track_keys(") == 1 and plain.count("launch_track_scan(") == 1
    assert plain.count("tp.fr = ") == 2                                           # the call's frames, and the sizing query's count of them
    # the launchers launch and nothing else; the kernel's grid loops instead of being capped
    unit = read_csrc("glv_track_frames.hip")
    assert_launch_only(unit, [r"\nhipError_t launch_track_frames\(", r"\nhipError_t launch_track_keys\("])
    kernel = strip_comments(function_body(unit, r"glv_track_frames_kernel\(const TrackFrames t,"))
    assert "item += gridDim.x" in kernel and "w = s + ((e - s) * m)" in kernel and "pack_unorm16(" in kernel
    assert "__builtin_fmaf" not in kernel and "fma(" not in kernel
    assert kernel.count("< last_key ? ") == 2 and kernel.count("key(k") == 2     # every index a table holds is clamped where it is taken, before any keyframe is loaded
    from glava_amd import build as B
    assert "glv_track_frames" in B.SMALL and "-ffp-contract=off" in B.HIPFLAGS
