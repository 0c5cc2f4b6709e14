"""Track mode for the wave module against the same updates issued one by one, alternating in one process.

  (a) one by one     `steps` glv_batch_process_s16 calls, one window per stream each (the windows cut beforehand, [steps][streams][n][2]: the cutting and
                     the upload a caller of this form pays are NOT timed, which flatters it)
  (b) track, rows    one glv_batch_track_wave_s16 call over the same windows of the long buffer; a workgroup of the one-launch form takes 64 consecutive
                     output rows (GLV_TRACK_WAVE_ORDER=rows at creation)
  (c) track, steps   the same call, a workgroup takes 64 consecutive steps of one channel row (GLV_TRACK_WAVE_ORDER=steps)

The shipped configuration: N = 4096, gl_storage 1, the pre-smoothing pass (bars = n, bar_phase 0.5), texels out: GLV_OP_WAVE | GLV_OP_BARS | GLV_OP_R16.

    python tools/track_wave_bench.py [--points 1x2048x256,8x2048x256,64x2048x256,1024x256x256,1x2048x735] [--rounds 7] [--out profiles/r11/track_wave.txt]
    GLV_SPECTRUM_LIB=<a library built from the parent commit> python tools/track_wave_bench.py --one-by-one-only --append ...

A point is streams x steps x hop.  Per point every form is warmed up, the track outputs are compared bit for bit with the one-by-one calls', then all are
timed `rounds` times alternating (a host clock around the calls and around the device synchronise that ends them: what a caller waits for, launch overhead
included).  Prints and writes the table: median ms of each form with the round-to-round spread (max - min) and the ratios.  --one-by-one-only times form
(a) alone and needs no track entry point: the baseline of a library built before it existed.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glava_amd import spectrum as G  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="1x2048x256,8x2048x256,64x2048x256,1024x256x256,1x2048x735")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--one-by-one-only", action="store_true")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "r11", "track_wave.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("track_wave_bench: no GPU -- nothing is measured without one")
    n = args.n
    mask = G.OP_WAVE | G.OP_BARS
    ops = G.OP_WAVE | G.OP_BARS | G.OP_R16
    p = G.Params(n=n, gl_storage=1, bars=n, bar_phase=0.5)
    lines = [f"# track_wave_bench: N={n} gl_storage=1 bars=n bar_phase=0.5 WAVE|BARS|R16; {torch.cuda.get_device_name(0)}; library {os.path.relpath(G.LIB_PATH, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))}",
             f"# ms = host clock around the calls and the synchronise that ends them, median of {args.rounds} alternating rounds (spread = max - min)"]
    if args.one_by_one_only:
        lines.insert(0, "# the one-by-one form alone (--one-by-one-only), through the library GLV_SPECTRUM_LIB names -- a build of another commit, kept outside the tree")
        lines.append(f"# {'streams':>7} {'steps':>6} {'hop':>5} {'one-by-one ms':>14} {'spread':>8} {'per update':>11}")
    else:
        lines.append(f"# {'streams':>7} {'steps':>6} {'hop':>5} {'one-by-one ms':>14} {'spread':>8} {'rows ms':>9} {'spread':>8} {'steps ms':>9} {'spread':>8} "
                     f"{'1x1/rows':>9} {'1x1/steps':>10} {'launches':>9} {'work MiB':>9}")
    print("\n".join(lines), flush=True)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for point in args.points.split(","):
        S, steps, hop = (int(v) for v in point.split("x"))
        pitch = (n + (steps - 1) * hop + 7) // 8 * 8
        gen = torch.Generator(device="cuda").manual_seed(4242 + S)
        d_pcm = torch.randint(-32768, 32768, (S, pitch, 2), generator=gen, device="cuda", dtype=torch.int32).to(torch.int16)
        wins = torch.stack([d_pcm[:, t * hop:t * hop + n, :] for t in range(steps)]).contiguous()         # [steps][S][n][2]
        out_a = torch.zeros((steps, S * 2, n), dtype=torch.int16, device="cuda")
        ba = G.Batch(p, S, mask)

        def run_a():
            for t in range(steps):
                ba.process_s16(wins[t], out_a[t], ops)

        forms = [("a", run_a)]
        if not args.one_by_one_only:
            tracks = {}
            for order in ("rows", "steps"):
                os.environ["GLV_TRACK_WAVE_ORDER"] = order
                tracks[order] = G.Batch(p, S, mask)
                del os.environ["GLV_TRACK_WAVE_ORDER"]
            work_bytes = tracks["rows"].track_wave_work_bytes(pitch, hop, steps, ops)
            work = torch.empty((work_bytes,), dtype=torch.uint8, device="cuda")
            out_b = torch.zeros_like(out_a)
            for order, b in tracks.items():
                forms.append((order, lambda b=b: b.track_wave_s16(d_pcm, pitch, hop, steps, out_b, work, ops)))
        for _, fn in forms:                                  # warm-up: code objects, the allocator
            fn()
        torch.cuda.synchronize()
        for k, fn in forms[1:]:
            out_b.zero_()
            fn()
            torch.cuda.synchronize()
            if not torch.equal(out_a, out_b):
                sys.exit(f"track_wave_bench: {point}: the track call's output ({k}) differs from the one-by-one calls'")
        res = {k: [] for k, _ in forms}
        for r in range(args.rounds):
            for k, fn in forms if r % 2 == 0 else forms[::-1]:
                res[k].append(timed(fn))
        med = {k: float(np.median(v)) for k, v in res.items()}
        spread = {k: max(v) - min(v) for k, v in res.items()}
        if args.one_by_one_only:
            line = f"  {S:>7} {steps:>6} {hop:>5} {med['a']:>14.3f} {spread['a']:>8.3f} {med['a'] / steps:>11.5f}"
        else:
            line = (f"  {S:>7} {steps:>6} {hop:>5} {med['a']:>14.3f} {spread['a']:>8.3f} {med['rows']:>9.3f} {spread['rows']:>8.3f} {med['steps']:>9.3f} "
                    f"{spread['steps']:>8.3f} {med['a'] / med['rows']:>9.2f} {med['a'] / med['steps']:>10.2f} {tracks['rows'].last_launches():>9} {work_bytes / 2 ** 20:>9.1f}")
            for b in tracks.values():
                b.close()
            del work, out_b
        print(line, flush=True)
        lines.append(line)
        ba.close()
        del d_pcm, wins, out_a
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
