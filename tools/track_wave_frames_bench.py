"""Track mode at render frames for the wave module (glv_batch_track_wave_frames_s16) against what a caller had before it, alternating in one process.

  (a) the whole call with the tables of glava_amd.track_starts.live_session_frames(22050, 144, ..., 256) against glv_batch_track_at_s16 with the same wave ops on
      the same batch and steps: every render frame's texture against every update's
  (b) the frames stage alone, texels out: the call with GLV_OP_WAVE | GLV_OP_R16 (the frames kernel and the write-back, nothing else runs) between a pair of HIP
      events -- and the bytes it moves per second: the texels written plus the keyframe bytes read (4 n bytes of s16 a stream for a keyframe from the recording,
      8 n of floats for one of d_keys, once per segment it occurs in), beside profiles/stream_ceiling.json.  Reported, not judged
  (c) glv_batch_track_frames_s16 (the protocol of tools/track_frames_bench.py part a) and glv_batch_track_wave_s16 (hop 256, the same wave ops) in this library
      against the library built from the parent commit (--parent-lib, loaded beside this one): whether the existing entries have moved

The configuration of (a) and (b): N = 4096, gl_storage 1, the pre-smoothing pass (bars = n, bar_phase 0.5), GLV_OP_WAVE | GLV_OP_BARS | GLV_OP_R16.

    python tools/track_wave_frames_bench.py [--points 1x2048,8x2048,64x2048,1024x256] [--rounds 7] [--parts a,b,c] [--segment FRAMES] [--parent-lib PATH]
                                            [--out profiles/r20/track_wave_frames.txt]

The protocol of tools/track_frames_bench.py.  Per point: both forms are warmed up once, then timed `rounds` times alternating -- (a), (c): a host clock around the
call and the device synchronise that ends it; (b): a pair of HIP events around the call.  Prints and writes the table: median ms of each form with the
round-to-round spread (max - min).  A difference inside the spread is none.  --segment: GLV_TRACK_FRAMES_SEGMENT for the batches of (a) and (b) (0: the default).
Part c is left out where no parent library is given.
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
from oracle_lib import lcg_pcm_fast  # noqa: E402
from track_at_bench import load_other, timed  # noqa: E402
from track_frames_bench import dev, events, session  # noqa: E402


def default_segment(frames, streams, n):
    """glv::track_frames_segment(frames, streams, n)"""
    per_segment = streams * ((n // 4 + 63) // 64)
    wanted = 1 if per_segment >= 16384 else -(-16384 // per_segment)
    return max(8, -(-frames // wanted))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="1x2048,8x2048,64x2048,1024x256", help="streams x steps")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--segment", type=int, default=0)
    ap.add_argument("--parent-lib", default=None, help="libglvspectrum.so built from the parent commit (part c)")
    ap.add_argument("--out", default=os.path.join("profiles", "r20", "track_wave_frames.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("track_wave_frames_bench: no GPU -- nothing is measured without one")
    n = args.n
    parts = [q for q in args.parts.split(",") if q != "c" or args.parent_lib]
    GP = load_other(args.parent_lib) if "c" in parts else None
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    ceiling = json.load(open(os.path.join(ROOT, "profiles", "stream_ceiling.json")))
    lines = [f"# track_wave_frames_bench: N={n} bars=n bar_phase=0.5; segment {args.segment or 'default'}; {torch.cuda.get_device_name(0)}",
             f"# median of {args.rounds} alternating rounds (spread = max - min); a, c: ms of a host clock around the call and the synchronise that ends it; b: ms between HIP events",
             "# a: gl_storage 1, GLV_OP_WAVE | GLV_OP_BARS | GLV_OP_R16: `other` = glv_batch_track_at_s16 (every update's texture), `new` = glv_batch_track_wave_frames_s16 on the",
             "#    same batch and steps with the frames of live_session_frames(22050, 144, ..., 256) (every render frame's)",
             "# b: `new` = glv_batch_track_wave_frames_s16 with GLV_OP_WAVE | GLV_OP_R16: the frames kernel and the write-back; `other` = glv_batch_track_at_s16 with the same ops",
             "#    (the waveform kernel over the steps); GB/s = (texels written + keyframe bytes read once per segment they occur in) / new",
             "# c: `other` = the parent commit's library, `new` = this one: cf glv_batch_track_frames_s16 (gl_storage 3, F = 5, FFT | GRAVITY | AVERAGE | BARS | R16, the same",
             "#    frames), cw glv_batch_track_wave_s16 (gl_storage 1, hop 256, GLV_OP_WAVE | GLV_OP_BARS | GLV_OP_R16)",
             f"# profiles/stream_ceiling.json: {json.dumps(ceiling)[:300]}",
             f"# {'part':>4} {'streams':>7} {'steps':>6} {'frames':>6} {'other ms':>10} {'spread':>8} {'launches':>8} {'new ms':>10} {'spread':>8} {'launches':>8} {'work MiB':>9} {'GB/s':>8}"]
    print("\n".join(lines), flush=True)
    points = [tuple(int(v) for v in pt.split("x")) for pt in args.points.split(",")]
    runs = [(p, "") for p in parts if p != "c"] + ([("c", "f"), ("c", "w")] if "c" in parts else [])
    for part, sub in runs:
        for S, steps in points:
            starts, urs, frm, to, mod, kf, kt = session(steps)
            frames = len(frm)
            pitch = (max(max(starts), (steps - 1) * 256) + n + 1) | 1           # odd
            x = lcg_pcm_fast(4242 + S, S * pitch * 2).reshape(S, pitch, 2).copy()
            x[:, :n, :] = 0                                                      # GLava's zeroed buffers in front of the audio's first frame
            d_pcm = torch.from_numpy(x).cuda()
            d_starts, d_from, d_to, d_mod = dev(starts, np.uint32), dev(frm, np.uint32), dev(to, np.uint32), dev(mod, np.float32)
            keys = torch.zeros((2, S * 2, n), dtype=torch.float32, device="cuda")
            wave_kw = dict(n=n, gl_storage=1, bars=n, bar_phase=0.5)
            if args.segment and part != "c": os.environ["GLV_TRACK_FRAMES_SEGMENT"] = str(args.segment)
            try:
                if sub == "f":
                    kw, mask, ops = dict(n=n, gl_storage=G.GL_STORAGE_UPLOAD, bars=n, bar_phase=0.5), GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS | G.OP_R16
                    bo, bn = GP.Batch(GP.Params(**kw), S, mask), G.Batch(G.Params(**kw), S, mask)
                elif sub == "w":
                    mask, ops = G.OP_WAVE | G.OP_BARS, G.OP_WAVE | G.OP_BARS | G.OP_R16
                    bo, bn = GP.Batch(GP.Params(**wave_kw), S, mask), G.Batch(G.Params(**wave_kw), S, mask)
                else:
                    ops = G.OP_WAVE | G.OP_R16 | (G.OP_BARS if part == "a" else 0)
                    bn = G.Batch(G.Params(**wave_kw), S, G.OP_WAVE | G.OP_BARS)
                    bo = bn
            finally:
                os.environ.pop("GLV_TRACK_FRAMES_SEGMENT", None)
            if sub == "f":
                d_ur = dev(urs, np.float32)
                wb = bn.track_frames_work_bytes(steps, frames, ops)
                work_o, work = torch.empty((bo.track_frames_work_bytes(steps, frames, ops),), dtype=torch.uint8, device="cuda"), torch.empty((wb,), dtype=torch.uint8, device="cuda")
                out_o = torch.zeros((frames, S * 2, n), dtype=torch.int16, device="cuda")
                out_n, keys_o = torch.zeros_like(out_o), torch.zeros_like(keys)

                def run_o(): bo.track_frames_s16(d_pcm, pitch, d_starts, d_ur, steps, d_from, d_to, d_mod, frames, keys_o, (0, 1), out_o, work_o, ops)
                def run_n(): bn.track_frames_s16(d_pcm, pitch, d_starts, d_ur, steps, d_from, d_to, d_mod, frames, keys, (0, 1), out_n, work, ops)
            elif sub == "w":
                wb = bn.track_wave_work_bytes(pitch, 256, steps, ops)
                work_o, work = torch.empty((bo.track_wave_work_bytes(pitch, 256, steps, ops),), dtype=torch.uint8, device="cuda"), torch.empty((wb,), dtype=torch.uint8, device="cuda")
                out_o = torch.zeros((steps, S * 2, n), dtype=torch.int16, device="cuda")
                out_n = torch.zeros_like(out_o)

                def run_o(): bo.track_wave_s16(d_pcm, pitch, 256, steps, out_o, work_o, ops)
                def run_n(): bn.track_wave_s16(d_pcm, pitch, 256, steps, out_n, work, ops)
            else:
                wb = bn.track_wave_frames_work_bytes(steps, frames, ops)
                work_o, work = torch.empty((bo.track_at_work_bytes(steps, ops),), dtype=torch.uint8, device="cuda"), torch.empty((wb,), dtype=torch.uint8, device="cuda")
                out_o = torch.zeros((steps, S * 2, n), dtype=torch.int16, device="cuda")
                out_n = torch.zeros((frames, S * 2, n), dtype=torch.int16, device="cuda")

                def run_o(): bo.track_at_s16(d_pcm, pitch, d_starts, steps, out_o, work_o, ops)
                def run_n(): bn.track_wave_frames_s16(d_pcm, pitch, d_starts, steps, d_from, d_to, d_mod, frames, keys, (0, 1), out_n, work, ops)
            run_o(); l_o = bo.last_launches()
            run_n(); l_n = bn.last_launches()
            torch.cuda.synchronize()
            if part == "c" and not torch.equal(out_o, out_n):
                sys.exit(f"track_wave_frames_bench: part c{sub} streams={S}: the two libraries' outputs differ")
            clock = events if part == "b" else timed
            to_, tn = [], []
            for _ in range(args.rounds):
                to_.append(clock(run_o)); tn.append(clock(run_n))
            mo, mn = float(np.median(to_)), float(np.median(tn))
            rate = ""
            if part == "b":
                seg = args.segment or default_segment(frames, S, n)
                read = 0
                for j0 in range(0, frames, seg):
                    read += sum(8 if k < 2 else 4 for k in set(frm[j0:j0 + seg]) | set(to[j0:j0 + seg]))
                moved = (frames * 2 * 2 + read + 2 * 8 + 2 * 8) * S * n          # texels out (two rows a stream), keyframes in, the write-back's two keyframes in and out
                rate = f"{moved / (mn * 1e-3) / 1e9:>8.0f}"
            line = (f"  {part + sub:>4} {S:>7} {steps:>6} {frames:>6} {mo:>10.3f} {max(to_) - min(to_):>8.3f} {l_o:>8} {mn:>10.3f} {max(tn) - min(tn):>8.3f} {l_n:>8} {wb / 2 ** 20:>9.1f} "
                    f"{rate}")
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
