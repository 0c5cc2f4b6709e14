"""Track mode from float recordings (glv_batch_track_windows_f32, glv_batch_track_wave_f32) against what a caller had before them, alternating in one
process.  Per point three forms over the same windows, hop 735:

  f32 track   the float track call on a float recording
  one by one  the same windows through glv_batch_process_f32_stereo, one call per update, the windows cut beforehand (cutting not counted)
  s16 track   glv_batch_track_windows_s16 / glv_batch_track_wave_s16 on an s16 recording of the same shape (half the input bytes)

Two chains at the shipped configuration, N = 4096: `fft` = the GL chain (gl_storage 1, F = 5) with the pre-smoothing pass (bars = n, bar_phase 0.5),
texels out; `wave` = GLV_OP_WAVE | GLV_OP_BARS | GLV_OP_R16 on the same parameters.

    python tools/track_f32_bench.py [--points 1x2048,8x2048,64x2048,1024x256] [--rounds 7] [--max-gib 24] [--out profiles/r13/track_f32.txt]

Per point: every form is warmed up once, the float track call's output compared bit for bit with the one-by-one form's from a reset state, then all
three timed `rounds` times alternating (a host clock around the calls and the device synchronise that ends them: what a caller waits for, launch
overhead included).  Where the buffers would exceed --max-gib the steps are halved until they fit.  Prints and writes the table: median ms of each form
with the round-to-round spread (max - min) and the ratios.  A difference inside the spread is none.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from glava_amd import spectrum as G  # noqa: E402
from oracle_lib import lcg_pcm_fast  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="1x2048,8x2048,64x2048,1024x256", help="streams x steps")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--hop", type=int, default=735)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--max-gib", type=float, default=24.0)
    ap.add_argument("--chains", default="fft,wave")
    ap.add_argument("--out", default=os.path.join("profiles", "r13", "track_f32.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("track_f32_bench: no GPU -- nothing is measured without one")
    n, hop = args.n, args.hop
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    p = G.Params(n=n, gl_storage=1, avg_window_kind=1, log_mode=1, bars=n, bar_phase=0.5)
    chains = {"fft": (GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS | G.OP_R16), "wave": (G.OP_WAVE | G.OP_BARS, G.OP_WAVE | G.OP_BARS | G.OP_R16)}
    head = [f"# track_f32_bench: N={n} hop={hop} gl_storage=1 F={p.avg_frames} bars=n bar_phase=0.5 texels out; {torch.cuda.get_device_name(0)}",
            "# fft = GLV_OP_FFT | GRAVITY | AVERAGE | BARS | R16 (glv_batch_track_windows_*); wave = GLV_OP_WAVE | BARS | R16 (glv_batch_track_wave_*)",
            f"# ms = host clock around the calls and the synchronise that ends them, median of {args.rounds} alternating rounds (spread = max - min)",
            "# one by one = the same windows through glv_batch_process_f32_stereo, window cutting not counted; s16 track = the s16 entry on an s16 recording of the same shape",
            f"# {'chain':>5} {'streams':>7} {'steps':>6} {'f32 track ms':>12} {'spread':>8} {'launches':>8} {'one by one ms':>13} {'spread':>8} {'launches':>8} "
            f"{'s16 track ms':>12} {'spread':>8} {'launches':>8} {'work MiB':>9} {'1by1/f32':>9} {'f32/s16':>8}"]
    lines = list(head)
    print("\n".join(lines), flush=True)
    points = [tuple(int(v) for v in pt.split("x")) for pt in args.points.split(",")]
    for chain in args.chains.split(","):
        mask, ops = chains[chain]
        wave = chain == "wave"
        for S, steps in points:
            while True:
                pitch = (n + (steps - 1) * hop) | 1                       # odd: every second stream starts 8-byte aligned and no more
                bf = G.Batch(p, S, mask)
                wb = (bf.track_wave_work_bytes if wave else bf.track_windows_work_bytes)(pitch, hop, steps, ops)
                out_bytes = steps * S * 2 * n * 2
                total = wb + S * pitch * 12 + 3 * out_bytes + steps * S * n * 8
                if total <= args.max_gib * 2 ** 30 or steps <= 8:
                    break
                bf.close()
                steps //= 2
            bo, bi = G.Batch(p, S, mask), G.Batch(p, S, mask)
            xi = lcg_pcm_fast(4242 + S, S * pitch * 2).reshape(S, pitch, 2)
            d_i = torch.from_numpy(xi).cuda()
            d_f = d_i.to(torch.float32) / 32768.0                          # the same signal as floats: float [S][pitch][2]
            assert d_f.data_ptr() % 16 == 0 and d_f.is_contiguous()
            work = torch.empty((wb,), dtype=torch.uint8, device="cuda")
            out_f = torch.zeros((steps, S * 2, n), dtype=torch.int16, device="cuda")
            out_o, out_i = torch.zeros_like(out_f), torch.zeros_like(out_f)
            wins = torch.stack([d_f[:, t * hop:t * hop + n, :] for t in range(steps)]).contiguous()         # [steps][S][n][2]

            def run_f():
                (bf.track_wave_f32 if wave else bf.track_windows_f32)(d_f, pitch, hop, steps, out_f, work, ops)

            def run_o():
                for t in range(steps):
                    bo.process_f32_stereo(wins[t], out_o[t], ops)

            def run_i():
                (bi.track_wave_s16 if wave else bi.track_windows_s16)(d_i, pitch, hop, steps, out_i, work, ops)

            run_f(); l_f = bf.last_launches()
            run_o(); l_o = steps * bo.last_launches()
            run_i(); l_i = bi.last_launches()
            bf.reset(); bo.reset(); bi.reset()
            run_f(); run_o(); run_i()
            torch.cuda.synchronize()
            if not torch.equal(out_f, out_o):
                sys.exit(f"track_f32_bench: {chain} streams={S}: the track call and the one-by-one calls differ")
            tf, to, ti = [], [], []
            for _ in range(args.rounds):
                tf.append(timed(run_f)); to.append(timed(run_o)); ti.append(timed(run_i))
            mf, mo, mi = float(np.median(tf)), float(np.median(to)), float(np.median(ti))
            line = (f"  {chain:>5} {S:>7} {steps:>6} {mf:>12.3f} {max(tf) - min(tf):>8.3f} {l_f:>8} {mo:>13.3f} {max(to) - min(to):>8.3f} {l_o:>8} "
                    f"{mi:>12.3f} {max(ti) - min(ti):>8.3f} {l_i:>8} {wb / 2 ** 20:>9.1f} {mo / mf:>9.2f} {mf / mi:>8.2f}")
            print(line, flush=True)
            lines.append(line)
            bf.close(); bo.close(); bi.close()
            del d_i, d_f, work, out_f, out_o, out_i, wins
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
