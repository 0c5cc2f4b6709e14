"""`setbufscale k` on the batched layer (glv_batch_set_bufscale): what the decimation stage moves per second, and what a whole call costs beside k = 1.

  (s) the stage alone -- glv::launch_decimate called directly (the library's own launcher, by its C++ symbol), HIP events around the one launch: bytes read plus
      written per second, 4 k n (s16) or 8 k n (f32) in and 8 n out per window, at k = 2, 4, 16 for `--streams` streams x one window (a process call's
      geometry) and for a `--table` streams x steps table call with the windows every 735 frames.  Beside profiles/stream_ceiling.json.  This is the number that
      says whether staging a workgroup's span through LDS is worth building
  (w) whole calls on the shipped pipeline (gl_storage 1, bars = n, bar_phase 0.5, texels out) at k = 2 beside the same configuration at k = 1 on n-frame
      windows: glv_batch_process_s16 on `--process-streams` streams, glv_batch_track_at_s16 on the `--table` point.  The difference is the stage plus the planar
      transform's extra 8 n bytes read per window; reported, not judged

    python tools/bufscale_bench.py [--n 4096] [--streams 65536] [--table 64x2048] [--process-streams 4096] [--rounds 7] [--parts s,w] [--out profiles/r21/bufscale.txt]

The project's protocol: every configuration of a part is warmed up once, then timed `rounds` times, the configurations alternating within a round; median ms
with the round-to-round spread (max - min), HIP-event times."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from glava_amd import spectrum as G  # noqa: E402


class TrackWindows(C.Structure):        # glava_amd/csrc/glv_frame.h
    _fields_ = [("pitch_frames", C.c_uint64), ("hop", C.c_uint64), ("steps", C.c_uint32), ("streams", C.c_uint32), ("step_major", C.c_uint32), ("pad", C.c_uint32),
                ("starts", C.c_void_p), ("start_max", C.c_uint32), ("pad2", C.c_uint32)]


class Decimate(C.Structure):            # glava_amd/csrc/glv_launch.h
    _fields_ = [("inp", C.c_void_p), ("out", C.c_void_p), ("n", C.c_uint32), ("k", C.c_uint32), ("mono", C.c_uint32), ("pad", C.c_uint32), ("w", TrackWindows)]


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(runs, rounds):
    """runs: name -> callable; one warm-up each, then `rounds` rounds in which they alternate.  name -> (median ms, spread)"""
    for fn in runs.values(): fn()
    torch.cuda.synchronize()
    t = {name: [] for name in runs}
    for _ in range(rounds):
        for name, fn in runs.items():
            t[name].append(events(fn))
    return {name: (float(np.median(v)), max(v) - min(v)) for name, v in t.items()}


def stage_part(args, lines):
    launch = getattr(C.CDLL(G.LIB_PATH), "_ZN3glv15launch_decimateEiRKNS_8DecimateEP12ihipStream_t")
    launch.argtypes = [C.c_int, C.POINTER(Decimate), C.c_void_p]
    n, ks = args.n, (2, 4, 16)
    S, steps = (int(v) for v in args.table.split("x"))
    lines.append(f"# {'part':>4} {'geometry':>16} {'kind':>4} {'k':>3} {'ms':>9} {'spread':>8} {'GiB moved':>10} {'GB/s':>8}")
    for geometry in ("process", "table"):
        streams = args.streams if geometry == "process" else S
        nsteps = 1 if geometry == "process" else steps
        kmax = max(ks)
        pitch = {k: k * n if geometry == "process" else (nsteps - 1) * 735 + k * n + 1 for k in ks}
        raw = torch.empty((streams * pitch[kmax] * 8 + 64,), dtype=torch.uint8, device="cuda")      # the largest recording (f32, k = 16); every other one is a view
        raw.view(torch.int16)[:].random_(-20000, 20000)                                               # s16 frames; read as floats: values of every size, some NaN (no cost on this path)
        out = torch.empty((nsteps * streams * 2 * n,), dtype=torch.float32, device="cuda")
        starts = torch.from_numpy((np.arange(nsteps, dtype=np.uint32) * 735).view(np.int32).copy()).cuda()
        runs, moved = {}, {}
        for f32 in (False, True):
            for k in ks:
                d = Decimate()
                d.inp, d.out, d.n, d.k, d.mono = raw.data_ptr(), out.data_ptr(), n, k, 0
                d.w.pitch_frames, d.w.hop, d.w.steps, d.w.streams, d.w.step_major = pitch[k], 0, nsteps, streams, 1
                if geometry == "table":
                    d.w.starts, d.w.start_max = starts.data_ptr(), pitch[k] - k * n
                name = ("f32" if f32 else "s16", k)

                def run(kind=1 if f32 else 0, d=d):
                    rc = launch(kind, C.byref(d), None)
                    if rc != 0: sys.exit(f"bufscale_bench: launch_decimate failed ({rc})")
                runs[name] = run
                moved[name] = nsteps * streams * ((8 if f32 else 4) * k * n + 8 * n)
        for (kind, k), (ms, spread) in alternate(runs, args.rounds).items():
            line = (f"  {'s':>4} {geometry + ' ' + str(streams) + 'x' + str(nsteps):>16} {kind:>4} {k:>3} {ms:>9.3f} {spread:>8.3f} {moved[(kind, k)] / 2 ** 30:>10.2f} "
                    f"{moved[(kind, k)] / (ms * 1e-3) / 1e9:>8.0f}")
            print(line, flush=True)
            lines.append(line)
        del raw, out
        torch.cuda.empty_cache()


def whole_part(args, lines):
    n, k = args.n, 2
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    ops = G.OP_FFT | GA | G.OP_BARS | G.OP_R16
    p = G.Params(n=n, gl_storage=1, avg_window_kind=1, bars=n, bar_phase=0.5)
    lines.append(f"# {'part':>4} {'call':>28} {'k=1 ms':>9} {'spread':>8} {'launches':>8} {'k=2 ms':>9} {'spread':>8} {'launches':>8} {'k=2 - k=1':>10}")
    # glv_batch_process_s16
    S = args.process_streams
    b1, b2 = G.Batch(p, S, GA | G.OP_BARS), G.Batch(p, S, GA | G.OP_BARS)
    b2.set_bufscale(k)
    x = torch.empty((S * k * n * 2,), dtype=torch.int16, device="cuda").random_(-20000, 20000)
    o1, o2 = (torch.zeros((S * 2, n), dtype=torch.int16, device="cuda") for _ in range(2))
    r = alternate({"k1": lambda: b1.process_s16(x, o1, ops), "k2": lambda: b2.process_s16(x, o2, ops)}, args.rounds)
    line = (f"  {'w':>4} {'process_s16 ' + str(S) + ' streams':>28} {r['k1'][0]:>9.3f} {r['k1'][1]:>8.3f} {b1.last_launches():>8} {r['k2'][0]:>9.3f} {r['k2'][1]:>8.3f} "
            f"{b2.last_launches():>8} {r['k2'][0] - r['k1'][0]:>10.3f}")
    print(line, flush=True); lines.append(line)
    b1.close(); b2.close()
    del x, o1, o2
    # glv_batch_track_at_s16
    S, steps = (int(v) for v in args.table.split("x"))
    b1, b2 = G.Batch(p, S, GA | G.OP_BARS), G.Batch(p, S, GA | G.OP_BARS)
    b2.set_bufscale(k)
    pitch = ((steps - 1) * 735 + k * n + 1) | 1
    x = torch.empty((S * pitch * 2,), dtype=torch.int16, device="cuda").random_(-20000, 20000)
    starts = torch.from_numpy((np.arange(steps, dtype=np.uint32) * 735).view(np.int32).copy()).cuda()
    o1, o2 = (torch.zeros((steps, S * 2, n), dtype=torch.int16, device="cuda") for _ in range(2))
    w1 = torch.empty((b1.track_at_work_bytes(steps, ops),), dtype=torch.uint8, device="cuda")
    w2 = torch.empty((b2.track_at_work_bytes(steps, ops),), dtype=torch.uint8, device="cuda")
    r = alternate({"k1": lambda: b1.track_at_s16(x, pitch, starts, steps, o1, w1, ops), "k2": lambda: b2.track_at_s16(x, pitch, starts, steps, o2, w2, ops)}, args.rounds)
    line = (f"  {'w':>4} {'track_at_s16 ' + args.table:>28} {r['k1'][0]:>9.3f} {r['k1'][1]:>8.3f} {b1.last_launches():>8} {r['k2'][0]:>9.3f} {r['k2'][1]:>8.3f} "
            f"{b2.last_launches():>8} {r['k2'][0] - r['k1'][0]:>10.3f}")
    print(line, flush=True); lines.append(line)
    lines.append(f"#      workspace MiB: k=1 {w1.numel() / 2 ** 20:.1f}, k=2 {w2.numel() / 2 ** 20:.1f}")
    b1.close(); b2.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--table", default="64x2048", help="streams x steps of the table call")
    ap.add_argument("--process-streams", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parts", default="s,w")
    ap.add_argument("--out", default=os.path.join("profiles", "r21", "bufscale.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bufscale_bench: no GPU -- nothing is measured without one")
    ceiling = json.load(open(os.path.join(ROOT, "profiles", "stream_ceiling.json")))
    lines = [f"# bufscale_bench: N={args.n}; {torch.cuda.get_device_name(0)}",
             f"# median of {args.rounds} rounds in which the configurations of a part alternate (spread = max - min); ms between HIP events",
             "# s: glv_decimate_kernel alone (glv::launch_decimate); moved = windows x (4 k n [s16] or 8 k n [f32] read + 8 n written): the algorithmic bytes -- a table",
             "#    call's windows overlap (every 735 frames), so most of what it reads comes from cache",
             "# w: the shipped pipeline (gl_storage 1, F = 5, bars = n, bar_phase 0.5, texels out); k=1 on n-frame windows, k=2 on 2 n-frame windows of the same batch shape",
             f"# profiles/stream_ceiling.json: {json.dumps(ceiling)[:200]}"]
    print("\n".join(lines), flush=True)
    for part in args.parts.split(","):
        (stage_part if part == "s" else whole_part)(args, lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
