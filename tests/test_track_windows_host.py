"""CPU: track mode at any hop (glv_batch_track_windows_s16) without a device -- the exported symbols and their Python prototypes, the map from
window (stream, step) to where it starts and to the row the transform launch writes, and the path's freedom from allocating / synchronising
HIP calls (the method of tests/test_track_host.py)."""
import ctypes as C
import os

from src_scan import ROOT, TRACK_EXECUTOR, assert_launch_only, function_body, read_csrc, read_host_src, strip_comments


def test_track_windows_symbols_are_exported_and_bound(glvlib):
    L = C.CDLL(glvlib.LIB_PATH)
    for name in ("glv_batch_track_windows_work_bytes", "glv_batch_track_windows_s16"):
        assert hasattr(L, name), name
    lib = glvlib.lib()
    assert lib.glv_batch_track_windows_work_bytes.restype is C.c_uint64
    assert len(lib.glv_batch_track_windows_work_bytes.argtypes) == 5 and len(lib.glv_batch_track_windows_s16.argtypes) == 9
    assert callable(glvlib.Batch.track_windows_work_bytes) and callable(glvlib.Batch.track_windows_s16)
    header = open(os.path.join(ROOT, "include", "glv_spectrum.h")).read()
    assert "glv_batch_track_windows_work_bytes(" in header and "glv_batch_track_windows_s16(" in header
    assert lib.glv_abi_version() == 7                                # added within the ABI: detected by the symbol


def test_every_window_is_one_row_in_both_orders(glvlib):
    """window (s, t) starts at s * pitch_frames + t * hop and is frame f = s * steps + t of the one transform launch; its channel rows are 2 f + ch
    (stream-major) or (t * streams + s) * 2 + ch (step-major): distinct rows that fill [0, 2 * streams * steps) in both orders, and the last frame any
    window reads is the last frame the call names."""
    G = glvlib
    for n in (256, 4096):
        for hop in (1, 45, 735, n // 4, n, n + 3):
            for steps in (1, 2, 11):
                need = n + (steps - 1) * hop
                for pitch in (need, need + 1, need + 3 * hop + 7):
                    for streams in (1, 3, 7):
                        starts = [G.track_window_start(pitch, hop, s, t) for s in range(streams) for t in range(steps)]
                        assert starts[0] == 0 and all(b > a for a, b in zip(starts, starts[1:]))          # stream-major enumeration walks the buffer forwards
                        assert max(starts) + n == (streams - 1) * pitch + (steps - 1) * hop + n
                        assert max(starts) + n <= streams * pitch
                        for s in range(streams):                                                           # no window crosses into the next stream
                            assert G.track_window_start(pitch, hop, s, steps - 1) + n <= (s + 1) * pitch
                        for step_major in (False, True):
                            rows = G.track_windows_rows(streams, steps, step_major)
                            assert len(rows) == streams * steps
                            both = sorted(r + ch for r in rows for ch in (0, 1))
                            assert both == list(range(2 * streams * steps)), (hop, steps, streams, step_major)
                            for s in range(streams):
                                for t in range(steps):
                                    f = s * steps + t
                                    assert rows[f] == ((t * streams + s) * 2 if step_major else 2 * f)


def test_track_windows_path_has_no_allocating_or_synchronising_call():
    src = read_host_src()
    assert_launch_only(src, [r"\nint plan_track_windows\(", r"\nint glv_batch_track_windows_s16\(", r"\nuint64_t glv_batch_track_windows_work_bytes\("] + TRACK_EXECUTOR)
    body = strip_comments(function_body(src, r"\nint track_windows\("))
    assert body.count("glv::launch_frame(") == 1 and "IN_S16_TRACK" in body                       # ONE transform launch, in the track input mode
    assert "for (" not in body and "while (" not in body                                          # ... and no loop of launches
    for sig in (r"\nint track\(glv_batch\* b,", r"\nint track_scan\(", r"\nint glv_batch_track_windows_s16\("):   # ... nor around it, nor after it
        body = strip_comments(function_body(src, sig))
        assert "for (" not in body and "while (" not in body and "glv::launch_frame(" not in body, sig
    # the launchers the path calls launch and nothing else
    assert_launch_only(read_csrc("glv_misc.hip"), [r"\nhipError_t launch_track_scan\(", r"\nhipError_t launch_frame\("])


def test_the_two_track_entries_share_their_decisions():
    """state / in16 / out16 / bars and every refusal that is not about hop or pitch are written once (track_chain, track_args) and both plans call them;
    what a call asks of the batch's earlier calls, and the scan, are written once for every entry"""
    src = strip_comments(read_host_src())
    for sig in (r"\nint plan_track\(", r"\nint plan_track_windows\("):
        body = function_body(src, sig)
        assert "track_args(" in body and "track_chain(" in body, sig
        for decided_once in ("tp.state =", "tp.in16 =", "tp.out16 =", "tp.bars =", "check_ops(", "gl_storage == 2", "GLV_OP_BARS_ONLY", "single_row"):
            assert decided_once not in body, (sig, decided_once)
    assert "log2_exact(hop)" not in function_body(src, r"\nint plan_track_windows\(")             # any hop
    # (check_ops has "... changed without glv_batch_set_params" messages of its own, about bars and smoothing: the tilt's is the one that ends in log_mode)
    for once in ('"gravity was last applied', 'log_mode changed without glv_batch_set_params")', "launch_track_scan("):
        assert src.count(once) == 1, once
