"""Track mode with a per-step update rate (glv_batch_track_rates_s16) against what a caller had before it, alternating in one process.

  (a) the rates entry with every d_ur[t] = the batch's own ur against glv_batch_track_at_s16 on the same table of starts (t * 735), in the same library:
      what the per-step float evaluation of the gravity step costs
  (b) glv_batch_track_at_s16 in this library against the library built from the parent commit (--parent-lib, loaded beside this one): whether the
      existing entry has moved
  (c) the tables of glava_amd.track_starts.live_session_rates(22050, 60, ..., 256) against the same windows through glv_batch_process_s16 one by one with
      glv_batch_set_params (ur of the step) between the calls, the windows cut beforehand

The shipped configuration: N = 4096, the GL chain (gl_storage 1, F = 5) with the pre-smoothing pass (bars = n, bar_phase 0.5), texels out.

    python tools/track_rates_bench.py [--points 1x2048,8x2048,64x2048,1024x256] [--rounds 7] [--parts a,b,c] [--parent-lib PATH] [--out profiles/r17/track_rates.txt]

The protocol of tools/track_at_bench.py.  Per point: both forms are warmed up once, their outputs compared bit for bit from a reset state, then timed
`rounds` times alternating (a host clock around the call and the device synchronise that ends it: what a caller waits for, launch overhead included).
Prints and writes the table: median ms of each form with the round-to-round spread (max - min) and the ratio.  A difference inside the spread is none.
Part b is left out where no parent library is given.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from glava_amd import spectrum as G  # noqa: E402
from glava_amd.track_starts import live_session_rates  # noqa: E402
from oracle_lib import lcg_pcm_fast  # noqa: E402
from track_at_bench import load_other, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="1x2048,8x2048,64x2048,1024x256", help="streams x steps")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--parent-lib", default=None, help="libglvspectrum.so built from the parent commit (part b)")
    ap.add_argument("--out", default=os.path.join("profiles", "r17", "track_rates.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("track_rates_bench: no GPU -- nothing is measured without one")
    n, hop = args.n, 735
    parts = [q for q in args.parts.split(",") if q != "b" or args.parent_lib]
    GP = load_other(args.parent_lib) if "b" in parts else None
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    mask, ops = GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS | G.OP_R16
    kw = dict(n=n, gl_storage=1, avg_window_kind=1, log_mode=1, bars=n, bar_phase=0.5)
    p = G.Params(**kw)
    lines = [f"# track_rates_bench: N={n} gl_storage=1 F={p.avg_frames} bars=n bar_phase=0.5 texels out; {torch.cuda.get_device_name(0)}",
             f"# ms = host clock around the call(s) and the synchronise that ends them, median of {args.rounds} alternating rounds (spread = max - min)",
             "# a: `other` = glv_batch_track_at_s16 with the table t * 735, `new` = glv_batch_track_rates_s16 on the same table with every d_ur[t] = the batch's ur",
             "# b: `other` = glv_batch_track_at_s16 with the table t * 735 in the parent commit's library, `new` = the same entry in this library",
             "# c: `other` = the same windows through glv_batch_process_s16 one by one, glv_batch_set_params (ur of the step) before each,",
             "#    `new` = glv_batch_track_rates_s16 with the tables of live_session_rates(22050, 60, ..., 256)",
             f"# {'part':>4} {'streams':>7} {'steps':>6} {'other ms':>10} {'spread':>8} {'launches':>8} {'new ms':>10} {'spread':>8} {'launches':>8} {'work MiB':>9} {'other/new':>11}"]
    print("\n".join(lines), flush=True)
    points = [tuple(int(v) for v in pt.split("x")) for pt in args.points.split(",")]
    for part in parts:
        for S, steps in points:
            if part == "c":
                starts, _, urs = live_session_rates(22050, 60, steps + 2, 256)
                starts, urs = starts[:steps], urs[:steps]
                assert len(starts) == steps
            else:
                starts, urs = [t * hop for t in range(steps)], [p.ur] * steps
            pitch = (max(starts) + n + 1) | 1                                   # odd
            bn = G.Batch(p, S, mask)
            bo = GP.Batch(GP.Params(**kw), S, mask) if part == "b" else G.Batch(p, S, mask)
            wb = bn.track_at_work_bytes(steps, ops)
            x = lcg_pcm_fast(4242 + S, S * pitch * 2).reshape(S, pitch, 2).copy()
            if part == "c":
                x[:, :n, :] = 0                                                  # GLava's zeroed buffers in front of the audio's first frame
            d_pcm = torch.from_numpy(x).cuda()
            d_starts = torch.from_numpy(np.asarray(starts, dtype=np.uint32).view(np.int32).copy()).cuda()
            d_ur = torch.from_numpy(np.asarray(urs, dtype=np.float32)).cuda()
            work = torch.empty((wb,), dtype=torch.uint8, device="cuda")
            out_o = torch.zeros((steps, S * 2, n), dtype=torch.int16, device="cuda")
            out_n = torch.zeros_like(out_o)
            wins = None
            if part == "c":
                wins = torch.stack([d_pcm[:, s:s + n, :] for s in starts]).contiguous()         # [steps][S][n][2]
                step_params = [G.Params(**kw, ur=u) for u in urs]

                def run_o():
                    for t in range(steps):
                        bo.set_params(step_params[t])
                        bo.process_s16(wins[t], out_o[t], ops)
            else:
                def run_o():
                    bo.track_at_s16(d_pcm, pitch, d_starts, steps, out_o, work, ops)
            if part == "b":
                def run_n():
                    bn.track_at_s16(d_pcm, pitch, d_starts, steps, out_n, work, ops)
            else:
                def run_n():
                    bn.track_rates_s16(d_pcm, pitch, d_starts, d_ur, steps, out_n, work, ops)

            run_o(); l_o = steps * bo.last_launches() if part == "c" else bo.last_launches()
            run_n(); l_n = bn.last_launches()
            bo.reset(); bn.reset()
            run_o(); run_n()
            torch.cuda.synchronize()
            if not torch.equal(out_o, out_n):
                sys.exit(f"track_rates_bench: part {part} streams={S}: the two forms' outputs differ")
            to, tn = [], []
            for _ in range(args.rounds):
                to.append(timed(run_o)); tn.append(timed(run_n))
            mo, mn = float(np.median(to)), float(np.median(tn))
            line = (f"  {part:>4} {S:>7} {steps:>6} {mo:>10.3f} {max(to) - min(to):>8.3f} {l_o:>8} {mn:>10.3f} {max(tn) - min(tn):>8.3f} {l_n:>8} {wb / 2 ** 20:>9.1f} {mo / mn:>11.3f}")
            print(line, flush=True)
            lines.append(line)
            bo.close(); bn.close()
            del d_pcm, work, out_o, out_n, wins
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
