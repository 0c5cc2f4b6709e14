"""Track mode against the same updates issued one by one, alternating in one process.

  (a) one by one   `steps` glv_batch_process_s16 calls, one window per stream each (the windows cut beforehand: [steps][streams][n][2])
  (b) track        one glv_batch_track_s16 call over the same windows of the long buffer

The shipped configuration: N = 4096, hop 256, the GL chain (gl_storage 1, F = 5) with the pre-smoothing pass (bars = n, bar_phase 0.5), texels out.

    python tools/track_bench.py [--streams 1,8,64,1024] [--steps 2048] [--rounds 5] [--max-gib 24] [--out profiles/r10/track.txt]

Per stream count: both forms are warmed up once, their outputs compared bit for bit from a reset state, then timed `rounds` times alternating (a host clock
around the calls and the device synchronise that ends them: what a caller waits for, launch overhead included).  Where the buffers of `steps` updates would
exceed --max-gib the steps are halved until they fit.  Prints and writes the table: median ms of each form with the round-to-round spread (max - min), ms
per update, and the ratio.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,8,64,1024")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--hop", type=int, default=256)
    ap.add_argument("--steps", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-gib", type=float, default=24.0)
    ap.add_argument("--out", default=os.path.join("profiles", "r10", "track.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("track_bench: no GPU -- nothing is measured without one")
    n, hop = args.n, args.hop
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    mask, ops = GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS | G.OP_R16
    p = G.Params(n=n, gl_storage=1, avg_window_kind=1, log_mode=1, bars=n, bar_phase=0.5)
    lines = [f"# track_bench: N={n} hop={hop} gl_storage=1 F={p.avg_frames} bars=n bar_phase=0.5 texels out; {torch.cuda.get_device_name(0)}",
             f"# ms = host clock around the calls and the synchronise that ends them, median of {args.rounds} alternating rounds (spread = max - min)",
             f"# {'streams':>7} {'steps':>6} {'one-by-one ms':>14} {'spread':>8} {'per update':>11} {'track ms':>10} {'spread':>8} {'per update':>11} {'ratio':>7} {'launches':>9} {'work MiB':>9}"]
    print("\n".join(lines), flush=True)
    for S in [int(s) for s in args.streams.split(",")]:
        steps = args.steps
        while True:
            pitch = n + (steps - 1) * hop
            ba = G.Batch(p, S, mask)
            work_bytes = ba.track_work_bytes(pitch, hop, steps, ops)
            total = work_bytes + S * pitch * 4 + 2 * steps * S * 2 * n * 2 + steps * S * n * 4
            if total <= args.max_gib * 2 ** 30 or steps <= 8:
                break
            ba.close()
            steps //= 2
        bb = G.Batch(p, S, mask)
        x = lcg_pcm_fast(4242 + S, S * pitch * 2).reshape(S, pitch, 2)
        d_pcm = torch.from_numpy(x).cuda()
        wins = torch.stack([d_pcm[:, t * hop:t * hop + n, :] for t in range(steps)]).contiguous()         # [steps][S][n][2]
        work = torch.empty((work_bytes,), dtype=torch.uint8, device="cuda")
        out_a = torch.zeros((steps, S * 2, n), dtype=torch.int16, device="cuda")
        out_b = torch.zeros_like(out_a)

        def run_a():
            for t in range(steps):
                ba.process_s16(wins[t], out_a[t], ops)

        def run_b():
            bb.track_s16(d_pcm, pitch, hop, steps, out_b, work, ops)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        run_a(); run_b()                                   # warm-up: code objects, the allocator
        ba.reset(); bb.reset()
        run_a(); run_b()
        torch.cuda.synchronize()
        if not torch.equal(out_a, out_b):
            sys.exit(f"track_bench: streams={S}: the track call's output differs from the one-by-one calls'")
        launches = bb.last_launches()
        ta, tb = [], []
        for _ in range(args.rounds):
            ta.append(timed(run_a)); tb.append(timed(run_b))
        ma, mb = float(np.median(ta)), float(np.median(tb))
        line = (f"  {S:>7} {steps:>6} {ma:>14.3f} {max(ta) - min(ta):>8.3f} {ma / steps:>11.5f} {mb:>10.3f} {max(tb) - min(tb):>8.3f} {mb / steps:>11.5f} "
                f"{ma / mb:>7.2f} {launches:>9} {work_bytes / 2 ** 20:>9.1f}")
        print(line, flush=True)
        lines.append(line)
        ba.close(); bb.close()
        del d_pcm, wins, work, out_a, out_b
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
