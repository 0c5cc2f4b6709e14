"""Track mode for the graph module (glv_batch_track_columns_s16) against the same updates issued one by one, alternating in one process.

  (one)   `steps` glv_batch_process_s16 calls with the same column table, the windows cut beforehand (the cutting is not counted)
  (track) one glv_batch_track_columns_s16 call

(profiles/r14/track_columns.txt was recorded while the scan still had a store limit -- only the bins the columns read -- and a creation-time switch for full
stores: its `track` column is the limit, `full` the scan as it is now.  The limit was not faster by more than the spread at 64 streams and was deleted with
the switch, so this tool now times the one form there is and its table has no `full` columns.)

The shipped configuration: N = 4096, hop 735 (44.1 kHz at 60 fps), the GL chain (gl_storage 1, F = 5), the graph module's tables for an 800-pixel and a
320-pixel window; an odd pitch.

    python tools/track_columns_bench.py [--points 1x2048,8x2048,64x2048,1024x256] [--widths 800,320] [--rounds 7] [--max-gib 24] [--out profiles/r14/track_columns.txt]

Per point: both forms are warmed up once, their outputs compared bit for bit from a reset state, then timed `rounds` times alternating (a host clock
around the calls and the device synchronise that ends them: what a caller waits for, launch overhead included).  Where the buffers would exceed --max-gib
the steps are halved until they fit.  Prints and writes the table: median ms of each form with the round-to-round spread (max - min) and the ratio.  A
difference inside the spread is none.
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
from glava_amd.bar_positions import graph_column_texels  # noqa: E402
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
    ap.add_argument("--widths", default="800,320", help="window widths in pixels: the graph module's column tables")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--hop", type=int, default=735)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--max-gib", type=float, default=24.0)
    ap.add_argument("--out", default=os.path.join("profiles", "r14", "track_columns.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("track_columns_bench: no GPU -- nothing is measured without one")
    n, hop = args.n, args.hop
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    mask, ops = GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS
    head = [f"# track_columns_bench: N={n} hop={hop} gl_storage=1 F=5, graph-module column tables; {torch.cuda.get_device_name(0)}",
            f"# ms = host clock around the calls and the synchronise that ends them, median of {args.rounds} alternating rounds (spread = max - min)",
            "# one = the same windows through glv_batch_process_s16 one by one with the same table; track = glv_batch_track_columns_s16",
            f"# {'width':>5} {'cols':>5} {'texels':>6} {'streams':>7} {'steps':>6} {'one ms':>10} {'spread':>8} {'launches':>8} {'track ms':>10} {'spread':>8} "
            f"{'work MiB':>9} {'one/track':>9}"]
    lines = list(head)
    print("\n".join(lines), flush=True)
    points = [tuple(int(v) for v in pt.split("x")) for pt in args.points.split(",")]
    for W in (int(w) for w in args.widths.split(",")):
        table = np.ascontiguousarray(graph_column_texels(n, W)[0], np.int64)
        cols = len(table)
        p = G.Params(n=n, gl_storage=1, avg_window_kind=1, avg_frames=5, log_mode=1, bars=cols)

        def batch(S):
            b = G.Batch(p, S, mask)
            b.set_column_texels(table)
            return b

        for S, steps in points:
            while True:
                pitch = (n + (steps - 1) * hop) | 1
                bt = batch(S)
                wb = bt.track_columns_work_bytes(pitch, hop, steps, ops)
                total = wb + S * pitch * 4 + 2 * steps * S * 2 * cols * 4 + steps * S * n * 4
                if total <= args.max_gib * 2 ** 30 or steps <= 8:
                    break
                bt.close()
                steps //= 2
            bo = batch(S)
            x = lcg_pcm_fast(4242 + S, S * pitch * 2).reshape(-1, 2)
            d_pcm = torch.from_numpy(x).cuda().view(S, pitch, 2)
            work = torch.empty((wb,), dtype=torch.uint8, device="cuda")
            out_o = torch.zeros((steps, S * 2, cols), dtype=torch.float32, device="cuda")
            out_t = torch.zeros_like(out_o)
            wins = torch.stack([d_pcm[:, t * hop:t * hop + n, :] for t in range(steps)]).contiguous()         # [steps][S][n][2]

            def run_o():
                for t in range(steps):
                    bo.process_s16(wins[t], out_o[t], ops)

            def run_t():
                bt.track_columns_s16(d_pcm, pitch, hop, steps, out_t, work, ops)

            run_o(); l_o = bo.last_launches()
            run_t()
            bo.reset(); bt.reset()
            run_o(); run_t()
            torch.cuda.synchronize()
            if not torch.equal(out_o.view(torch.int32), out_t.view(torch.int32)):
                sys.exit(f"track_columns_bench: width {W} streams={S}: the two forms' outputs differ")
            to, tt = [], []
            for _ in range(args.rounds):
                to.append(timed(run_o)); tt.append(timed(run_t))
            mo, mt = float(np.median(to)), float(np.median(tt))
            line = (f"  {W:>5} {cols:>5} {len(np.unique(table)):>6} {S:>7} {steps:>6} {mo:>10.3f} {max(to) - min(to):>8.3f} {steps * l_o:>8} {mt:>10.3f} {max(tt) - min(tt):>8.3f} "
                    f"{wb / 2 ** 20:>9.1f} {mo / mt:>9.2f}")
            print(line, flush=True)
            lines.append(line)
            for b in (bo, bt): b.close()
            del d_pcm, work, out_o, out_t, wins
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
