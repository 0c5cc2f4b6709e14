"""Track mode at render frames (glv_batch_track_frames_s16) against what a caller had before it, alternating in one process.

  (a) the frames call with the tables of glava_amd.track_starts.live_session_frames(22050, 144, ..., 256) against glv_batch_track_rates_s16 on the same
      batch, steps and tables of the updates: what the frames cost on top of the steps
  (b) the frames stage alone, by difference of HIP-event times: the frames call with GLV_OP_R16 and no bars (transform, scan, frames kernel, write-back)
      against glv_batch_track_rates_s16 on a gl_storage 0 twin with float rows out (transform, scan) -- and the bytes it moves per second: the texels written
      plus one read of every keyframe row the tables name per segment, beside the write ceiling of profiles/stream_ceiling.json.  Reported, not judged
  (c) glv_batch_track_at_s16 on the shipped GL chain in this library against the library built from the parent commit (--parent-lib, loaded beside this
      one): whether the existing entry has moved

The configuration of (a) and (b): N = 4096, gl_storage 3, F = 5, the pre-smoothing pass (bars = n, bar_phase 0.5), texels out; of (c): the protocol of
tools/track_rates_bench.py part b.

    python tools/track_frames_bench.py [--points 1x2048,8x2048,64x2048,1024x256] [--rounds 7] [--parts a,b,c] [--parent-lib PATH] [--out profiles/r19/track_frames.txt]

The protocol of tools/track_rates_bench.py.  Per point: both forms are warmed up once, then timed `rounds` times alternating -- (a), (c): a host clock around
the call and the device synchronise that ends it; (b): a pair of HIP events around the call.  Prints and writes the table: median ms of each form with the
round-to-round spread (max - min).  A difference inside the spread is none.  Part c is left out where no parent library is given.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from glava_amd import spectrum as G  # noqa: E402
from glava_amd.track_starts import live_session_frames  # noqa: E402
from oracle_lib import lcg_pcm_fast  # noqa: E402
from track_at_bench import load_other, timed  # noqa: E402


def session(steps):
    """the tables of the longest 144 fps session that runs exactly `steps` updates"""
    lo, hi = 1, steps * 4 + 400
    while lo < hi:                                                              # the first frame count with more than `steps` updates
        mid = (lo + hi) // 2
        if len(live_session_frames(22050, 144, mid, 256)[0]) > steps: hi = mid
        else: lo = mid + 1
    t = live_session_frames(22050, 144, lo - 1, 256)
    assert len(t[0]) == steps
    return t


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def dev(a, dtype):
    a = np.asarray(a, dtype=dtype)
    return torch.from_numpy(a.view(np.int32).copy() if dtype == np.uint32 else a.copy()).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="1x2048,8x2048,64x2048,1024x256", help="streams x steps")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--parent-lib", default=None, help="libglvspectrum.so built from the parent commit (part c)")
    ap.add_argument("--out", default=os.path.join("profiles", "r19", "track_frames.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("track_frames_bench: no GPU -- nothing is measured without one")
    n = args.n
    parts = [q for q in args.parts.split(",") if q != "c" or args.parent_lib]
    GP = load_other(args.parent_lib) if "c" in parts else None
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    mask = GA | G.OP_BARS
    ceiling = json.load(open(os.path.join(ROOT, "profiles", "stream_ceiling.json")))
    lines = [f"# track_frames_bench: N={n} F=5 bars=n bar_phase=0.5 texels out; {torch.cuda.get_device_name(0)}",
             f"# median of {args.rounds} alternating rounds (spread = max - min); a, c: ms of a host clock around the call and the synchronise that ends it; b: ms between HIP events",
             "# a: gl_storage 3, `other` = glv_batch_track_rates_s16, `new` = glv_batch_track_frames_s16 on the same batch, steps and update tables, with the frames of",
             "#    live_session_frames(22050, 144, ..., 256); both with GLV_OP_BARS | GLV_OP_R16",
             "# b: `other` = glv_batch_track_rates_s16 on a gl_storage 0 twin, float rows out (transform + scan), `new` = glv_batch_track_frames_s16 with GLV_OP_R16 and no",
             "#    bars (transform + scan + frames kernel + write-back); stage = new - other, GB/s = (texels written + keyframe rows read once per segment they occur in) / stage",
             "# c: gl_storage 1, `other` = glv_batch_track_at_s16 with the table t * 735 in the parent commit's library, `new` = the same entry in this library",
             f"# profiles/stream_ceiling.json: {json.dumps(ceiling)[:300]}",
             f"# {'part':>4} {'streams':>7} {'steps':>6} {'frames':>6} {'other ms':>10} {'spread':>8} {'launches':>8} {'new ms':>10} {'spread':>8} {'launches':>8} {'work MiB':>9} {'new-other':>10} {'GB/s':>8}"]
    print("\n".join(lines), flush=True)
    points = [tuple(int(v) for v in pt.split("x")) for pt in args.points.split(",")]
    for part in parts:
        for S, steps in points:
            if part == "c":
                kw = dict(n=n, gl_storage=1, avg_window_kind=1, log_mode=1, bars=n, bar_phase=0.5)
                starts, frames = [t * 735 for t in range(steps)], 0
                ops = G.OP_FFT | GA | G.OP_BARS | G.OP_R16
            else:
                kw = dict(n=n, gl_storage=G.GL_STORAGE_UPLOAD, bars=n, bar_phase=0.5)
                starts, urs, frm, to, mod, kf, kt = session(steps)
                frames = len(frm)
                ops = G.OP_FFT | GA | G.OP_R16 | (G.OP_BARS if part == "a" else 0)
            p = G.Params(**kw)
            pitch = (max(starts) + n + 1) | 1                                   # odd
            bn = G.Batch(p, S, mask)
            if part == "c": bo = GP.Batch(GP.Params(**kw), S, mask)
            elif part == "b": bo = G.Batch(G.Params(n=n), S, GA)
            else: bo = bn                                                        # the same batch: both calls leave the state the updates leave
            x = lcg_pcm_fast(4242 + S, S * pitch * 2).reshape(S, pitch, 2).copy()
            if part != "c": x[:, :n, :] = 0                                      # GLava's zeroed buffers in front of the audio's first frame
            d_pcm = torch.from_numpy(x).cuda()
            d_starts = dev(starts, np.uint32)
            ops_o = G.OP_FFT | GA if part == "b" else ops
            wb_o = bo.track_at_work_bytes(steps, ops_o)
            out_o = torch.zeros((steps, S * 2, n), dtype=torch.float32 if part == "b" else torch.int16, device="cuda")
            work_o = torch.empty((wb_o,), dtype=torch.uint8, device="cuda")
            if part == "c":
                wb = bn.track_at_work_bytes(steps, ops)
                work, out_n = torch.empty((wb,), dtype=torch.uint8, device="cuda"), torch.zeros_like(out_o)

                def run_o(): bo.track_at_s16(d_pcm, pitch, d_starts, steps, out_o, work_o, ops)
                def run_n(): bn.track_at_s16(d_pcm, pitch, d_starts, steps, out_n, work, ops)
            else:
                d_ur, d_from, d_to, d_mod = dev(urs, np.float32), dev(frm, np.uint32), dev(to, np.uint32), dev(mod, np.float32)
                keys = torch.zeros((2, S * 2, n), dtype=torch.float32, device="cuda")
                wb = bn.track_frames_work_bytes(steps, frames, ops)
                work = torch.empty((wb,), dtype=torch.uint8, device="cuda")
                out_n = torch.zeros((frames, S * 2, n), dtype=torch.int16, device="cuda")

                def run_o(): bo.track_rates_s16(d_pcm, pitch, d_starts, d_ur, steps, out_o, work_o, ops_o)
                def run_n(): bn.track_frames_s16(d_pcm, pitch, d_starts, d_ur, steps, d_from, d_to, d_mod, frames, keys, (0, 1), out_n, work, ops)
            run_o(); l_o = bo.last_launches()
            run_n(); l_n = bn.last_launches()
            torch.cuda.synchronize()
            if part == "c":
                bo.reset(); bn.reset(); run_o(); run_n(); torch.cuda.synchronize()
                if not torch.equal(out_o, out_n):
                    sys.exit(f"track_frames_bench: part c streams={S}: the two libraries' outputs differ")
            clock = events if part == "b" else timed
            to_, tn = [], []
            for _ in range(args.rounds):
                to_.append(clock(run_o)); tn.append(clock(run_n))
            mo, mn = float(np.median(to_)), float(np.median(tn))
            rate = ""
            if part == "b":
                seg = max(8, -(-frames // max(1, -(-16384 // (S * 2 * (n // 256))))))      # glv::track_frames_segment
                reads = 0
                for j0 in range(0, frames, seg):
                    reads += len(set(frm[j0:j0 + seg]) | set(to[j0:j0 + seg]))
                moved = (frames * 2 + reads * 4 + 4 * 4) * S * 2 * n                        # texels out, keyframe rows in, the write-back's two rows in and out
                rate = f"{moved / ((mn - mo) * 1e-3) / 1e9:>8.0f}" if mn > mo else f"{'-':>8}"
            line = (f"  {part:>4} {S:>7} {steps:>6} {frames:>6} {mo:>10.3f} {max(to_) - min(to_):>8.3f} {l_o:>8} {mn:>10.3f} {max(tn) - min(tn):>8.3f} {l_n:>8} {wb / 2 ** 20:>9.1f} "
                    f"{mn - mo:>10.3f} {rate}")
            print(line, flush=True)
            lines.append(line)
            if bo is not bn: bo.close()
            bn.close()
            del d_pcm, work, work_o, out_o, out_n
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
