"""Track mode from planar float recordings (glv_batch_track_at_f32_planar) beside the interleaved entry on the interleaved copy of the same recording,
alternating in one process -- and, with --parent-lib, the existing table entries of this library beside the parent commit's.

  (p) glv_batch_track_at_f32 on float [streams][pitch][2] against glv_batch_track_at_f32_planar on float [streams][2][pitch]: the shipped FFT pipeline
  (w) the same pair for the wave module, GLV_OP_WAVE | GLV_OP_BARS | GLV_OP_R16
  (s) glv_batch_track_at_s16 in the parent commit's library against the same entry in this library
  (f) glv_batch_track_at_f32 likewise

The protocol of tools/track_at_bench.py (profiles/r16/track_at.txt): N = 4096, the GL chain (gl_storage 1, F = 5) with the pre-smoothing pass (bars = n,
bar_phase 0.5), texels out, the table t * 735; 1 / 8 / 64 streams x 2048 steps and 1024 x 256.

    python tools/track_planar_bench.py [--points 1x2048,8x2048,64x2048,1024x256] [--rounds 7] [--parts p,w] [--out profiles/r24/track_planar.txt]
    python tools/track_planar_bench.py --parts s,f --parent-lib PATH --out profiles/r24/bench_compare.txt

Per point: both forms are warmed up once, their outputs compared bit for bit from a reset state, then timed `rounds` times alternating (a host clock around
the call and the device synchronise that ends it: what a caller waits for, launch overhead included).  Prints and writes the table: median ms of each form
with the round-to-round spread (max - min), the difference of the medians and whether it lies inside the larger spread.  A difference inside the spread is none.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from glava_amd import spectrum as G  # noqa: E402
from glava_amd.track_starts import hop_starts  # noqa: E402
from track_at_bench import load_other, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="1x2048,8x2048,64x2048,1024x256", help="streams x steps")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parts", default="p,w")
    ap.add_argument("--parent-lib", default=None, help="libglvspectrum.so built from the parent commit (parts s and f)")
    ap.add_argument("--out", default=os.path.join("profiles", "r24", "track_planar.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("track_planar_bench: no GPU -- nothing is measured without one")
    n, hop = args.n, 735
    parts = [q for q in args.parts.split(",") if q in ("p", "w") or args.parent_lib]
    GP = load_other(args.parent_lib) if ("s" in parts or "f" in parts) else None
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    lines = [f"# track_planar_bench: N={n} gl_storage=1 F=5 bars=n bar_phase=0.5 texels out, table t * {hop}; {torch.cuda.get_device_name(0)}",
             f"# ms = host clock around the call and the synchronise that ends it, median of {args.rounds} alternating rounds (spread = max - min)",
             "# p: `other` = glv_batch_track_at_f32 on the interleaved copy, `this` = glv_batch_track_at_f32_planar on the planar recording: FFT | GRAVITY | AVERAGE | BARS | R16",
             "# w: the same pair, GLV_OP_WAVE | GLV_OP_BARS | GLV_OP_R16",
             "# s / f: `other` = glv_batch_track_at_s16 / _f32 in the parent commit's library, `this` = the same entry in this library",
             "# diff = this - other; `inside`: |diff| <= the larger of the two spreads",
             f"# {'part':>4} {'streams':>7} {'steps':>6} {'other ms':>10} {'spread':>8} {'this ms':>10} {'spread':>8} {'launches':>8} {'diff ms':>9} {'inside':>6} {'other/this':>10}"]
    print("\n".join(lines), flush=True)
    points = [tuple(int(v) for v in pt.split("x")) for pt in args.points.split(",")]
    for part in parts:
        wave = part == "w"
        mask = (G.OP_WAVE | G.OP_BARS) if wave else (GA | G.OP_BARS)
        ops = (G.OP_WAVE | G.OP_BARS | G.OP_R16) if wave else (G.OP_FFT | GA | G.OP_BARS | G.OP_R16)
        kw = dict(n=n, gl_storage=1, avg_window_kind=1, log_mode=1, bars=n, bar_phase=0.5)
        for S, steps in points:
            starts = hop_starts(steps, hop)
            pitch = (max(starts) + n + 1) | 1                                   # odd: the second row of every stream starts off the first one's boundaries
            bn = G.Batch(G.Params(**kw), S, mask)
            bo = (GP if part in ("s", "f") else G).Batch((GP if part in ("s", "f") else G).Params(**kw), S, mask)
            wb = bn.track_at_work_bytes(steps, ops)
            g = torch.Generator(device="cuda")
            g.manual_seed(4242 + S)
            if part == "s":
                inter = torch.randint(-32768, 32768, (S, pitch, 2), generator=g, device="cuda", dtype=torch.int32).to(torch.int16)
            else:
                inter = (torch.rand((S, pitch, 2), generator=g, device="cuda") * 2.0 - 1.0)
            planar = inter.transpose(1, 2).contiguous() if part in ("p", "w") else None      # [S][2][pitch]: the same samples
            d_starts = torch.from_numpy(np.asarray(starts, dtype=np.uint32).view(np.int32).copy()).cuda()
            work = torch.empty((wb,), dtype=torch.uint8, device="cuda")
            out_o = torch.zeros((steps, S * 2, n), dtype=torch.int16, device="cuda")
            out_n = torch.zeros_like(out_o)
            if part == "s":
                def run_o(): bo.track_at_s16(inter, pitch, d_starts, steps, out_o, work, ops)
                def run_n(): bn.track_at_s16(inter, pitch, d_starts, steps, out_n, work, ops)
            elif part == "f":
                def run_o(): bo.track_at_f32(inter, pitch, d_starts, steps, out_o, work, ops)
                def run_n(): bn.track_at_f32(inter, pitch, d_starts, steps, out_n, work, ops)
            else:
                def run_o(): bo.track_at_f32(inter, pitch, d_starts, steps, out_o, work, ops)
                def run_n(): bn.track_at_f32_planar(planar, d_starts, steps, out_n, work, ops)
            run_o(); run_n()
            launches = bn.last_launches()
            bo.reset(); bn.reset()
            run_o(); run_n()
            torch.cuda.synchronize()
            if not torch.equal(out_o, out_n):
                sys.exit(f"track_planar_bench: part {part} streams={S}: the two forms' outputs differ")
            to, tn = [], []
            for _ in range(args.rounds):
                to.append(timed(run_o)); tn.append(timed(run_n))
            mo, mn = float(np.median(to)), float(np.median(tn))
            so, sn = max(to) - min(to), max(tn) - min(tn)
            line = (f"  {part:>4} {S:>7} {steps:>6} {mo:>10.3f} {so:>8.3f} {mn:>10.3f} {sn:>8.3f} {launches:>8} {mn - mo:>+9.3f} "
                    f"{'yes' if abs(mn - mo) <= max(so, sn) else 'NO':>6} {mo / mn:>10.3f}")
            print(line, flush=True)
            lines.append(line)
            bo.close(); bn.close()
            del inter, planar, work, out_o, out_n
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
