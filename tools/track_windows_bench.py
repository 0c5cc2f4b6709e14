"""Track mode at any hop (glv_batch_track_windows_s16) against what a caller had before it, alternating in one process.

  (a) hop 256: the new entry against glv_batch_track_s16 (the residue form, untouched) on the same recording, with a tight pitch and with a pitch of
      twice what the call consumes -- the slack the residue form transforms and the new one does not
  (b) hop 735 and hop 736: the new entry against `steps` glv_batch_process_s16 calls with the windows cut beforehand.  Every window of the 736 run is
      8-byte aligned; every second one of the 735 run is not: the pair separates what the dword loads cost from everything else
  (c) hop 735 with d_pcm advanced by one frame

The shipped configuration: N = 4096, the GL chain (gl_storage 1, F = 5) with the pre-smoothing pass (bars = n, bar_phase 0.5), texels out.

    python tools/track_windows_bench.py [--points 1x2048,8x2048,64x2048,1024x256] [--rounds 7] [--max-gib 24] [--out profiles/r12/track_windows.txt]

Per point: both forms are warmed up once, their outputs compared bit for bit from a reset state, then timed `rounds` times alternating (a host clock around
the calls and the device synchronise that ends them: what a caller waits for, launch overhead included).  Where the buffers would exceed --max-gib the steps
are halved until they fit.  Prints and writes the table: median ms of each form with the round-to-round spread (max - min) and the ratio.  A difference
inside the spread is none.
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--max-gib", type=float, default=24.0)
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--out", default=os.path.join("profiles", "r12", "track_windows.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("track_windows_bench: no GPU -- nothing is measured without one")
    n = args.n
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    mask, ops = GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS | G.OP_R16
    p = G.Params(n=n, gl_storage=1, avg_window_kind=1, log_mode=1, bars=n, bar_phase=0.5)
    head = [f"# track_windows_bench: N={n} gl_storage=1 F={p.avg_frames} bars=n bar_phase=0.5 texels out; {torch.cuda.get_device_name(0)}",
            f"# ms = host clock around the calls and the synchronise that ends them, median of {args.rounds} alternating rounds (spread = max - min)",
            "# `other` = glv_batch_track_s16 (residue) in part a, the same windows through glv_batch_process_s16 one by one in parts b and c",
            f"# {'part':>4} {'hop':>5} {'pitch':>6} {'off':>3} {'streams':>7} {'steps':>6} {'other ms':>10} {'spread':>8} {'launches':>8} {'work MiB':>9} "
            f"{'windows ms':>10} {'spread':>8} {'launches':>8} {'work MiB':>9} {'other/windows':>13}"]
    lines = list(head)
    print("\n".join(lines), flush=True)
    points = [tuple(int(v) for v in pt.split("x")) for pt in args.points.split(",")]
    cases = []       # part, hop, pitch factor, offset frames
    if "a" in args.parts: cases += [("a", 256, 1, 0), ("a", 256, 2, 0)]
    if "b" in args.parts: cases += [("b", 735, 1, 0), ("b", 736, 1, 0)]
    if "c" in args.parts: cases += [("c", 735, 1, 1)]
    for part, hop, pf, off in cases:
        for S, steps in points:
            while True:
                need = n + (steps - 1) * hop
                pitch = need * pf if part == "a" else need + 1          # part a: a multiple of the hop, as the residue entry asks; else odd
                bn = G.Batch(p, S, mask)
                wb_new = bn.track_windows_work_bytes(pitch, hop, steps, ops)
                wb_old = bn.track_work_bytes(pitch, hop, steps, ops) if part == "a" else 0
                out_bytes = steps * S * 2 * n * 2
                total = max(wb_new, wb_old) + S * pitch * 4 + 2 * out_bytes + (0 if part == "a" else steps * S * n * 4)
                if total <= args.max_gib * 2 ** 30 or steps <= 8:
                    break
                bn.close()
                steps //= 2
            bo = G.Batch(p, S, mask)
            x = lcg_pcm_fast(4242 + S, (S * pitch + off + 2) * 2).reshape(-1, 2)
            buf = torch.from_numpy(x).cuda()
            assert buf.data_ptr() % 8 == 0
            d_pcm = buf[off:off + S * pitch].view(S, pitch, 2)
            work = torch.empty((max(wb_new, wb_old),), dtype=torch.uint8, device="cuda")
            out_o = torch.zeros((steps, S * 2, n), dtype=torch.int16, device="cuda")
            out_n = torch.zeros_like(out_o)
            if part == "a":
                def run_o():
                    bo.track_s16(d_pcm, pitch, hop, steps, out_o, work, ops)
            else:
                wins = torch.stack([d_pcm[:, t * hop:t * hop + n, :] for t in range(steps)]).contiguous()         # [steps][S][n][2]

                def run_o():
                    for t in range(steps):
                        bo.process_s16(wins[t], out_o[t], ops)

            def run_n():
                bn.track_windows_s16(d_pcm, pitch, hop, steps, out_n, work, ops)

            run_o(); l_o = bo.last_launches() if part == "a" else steps * bo.last_launches()
            run_n(); l_n = bn.last_launches()
            bo.reset(); bn.reset()
            run_o(); run_n()
            torch.cuda.synchronize()
            if not torch.equal(out_o, out_n):
                sys.exit(f"track_windows_bench: part {part} hop {hop} streams={S}: the two forms' outputs differ")
            to, tn = [], []
            for _ in range(args.rounds):
                to.append(timed(run_o)); tn.append(timed(run_n))
            mo, mn = float(np.median(to)), float(np.median(tn))
            line = (f"  {part:>4} {hop:>5} {('x%d' % pf) if part == 'a' else 'odd':>6} {off:>3} {S:>7} {steps:>6} {mo:>10.3f} {max(to) - min(to):>8.3f} {l_o:>8} {wb_old / 2 ** 20:>9.1f} "
                    f"{mn:>10.3f} {max(tn) - min(tn):>8.3f} {l_n:>8} {wb_new / 2 ** 20:>9.1f} {mo / mn:>13.2f}")
            print(line, flush=True)
            lines.append(line)
            bo.close(); bn.close()
            del buf, d_pcm, work, out_o, out_n
            if part != "a":
                del wins
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
