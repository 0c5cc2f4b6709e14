"""Track mode per stream (glv_batch_track_each_s16) against what a caller had before it, alternating in one process.

  (1) equal rows and full counts against glv_batch_track_rates_s16 on the same tables (t * 735, every rate the batch's ur), in the same library: the price
      of the per-stream index and of the per-stream scan kernel.  Reported, not bounded.
  (2) per-stream tables of glava_amd.track_starts.live_session_rates (a different frame rate per stream) with mixed counts -- a quarter of the streams at 0, a
      quarter at half, the rest at all steps -- against the same work as one-stream batches one after another (glv_batch_track_rates_s16 over each stream's
      own count on its own recording): what the feature replaces.  Up to 64 streams every stream has a batch of its own and the outputs are compared bit for
      bit first; beyond, ONE one-stream batch runs every stream's call in turn (the same launches and bytes; its state is not any stream's, so nothing is compared).
  (3) glv_batch_track_at_s16 and glv_batch_track_rates_s16 in this library against the library built from the parent commit (--parent-lib, loaded beside this
      one): whether the existing entries have moved.  `inside`: |diff| <= the larger of the two round-to-round spreads.

The shipped configuration: N = 4096, the GL chain (gl_storage 1, F = 5) with the pre-smoothing pass (bars = n, bar_phase 0.5), texels out.

    python tools/track_each_bench.py [--points 1x2048,8x2048,64x2048,1024x256] [--rounds 7] [--parts 1,2,3] [--parent-lib PATH] [--out profiles/r25/track_each.txt]

The protocol of tools/track_rates_bench.py: per point both forms are warmed up once, compared from a reset state where stated, then timed `rounds` times
alternating (a host clock around the call(s) and the device synchronise that ends them).  Medians with the spread (max - min).  Part 3 is left out where no
parent library is given."""
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
from glava_amd.track_starts import live_session_rates, stack_tables  # noqa: E402
from oracle_lib import lcg_pcm_fast  # noqa: E402
from track_at_bench import load_other, timed  # noqa: E402

FPS = (60, 30, 144, 24, 50, 75, 120, 48)


def u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="1x2048,8x2048,64x2048,1024x256", help="streams x steps")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parts", default="1,2,3")
    ap.add_argument("--parent-lib", default=None, help="libglvspectrum.so built from the parent commit (part 3)")
    ap.add_argument("--out", default=os.path.join("profiles", "r25", "track_each.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("track_each_bench: no GPU -- nothing is measured without one")
    n, hop = args.n, 735
    parts = [q for q in args.parts.split(",") if q != "3" or args.parent_lib]
    GP = load_other(args.parent_lib) if "3" in parts else None
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    mask, ops = GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS | G.OP_R16
    kw = dict(n=n, gl_storage=1, avg_window_kind=1, log_mode=1, bars=n, bar_phase=0.5)
    p = G.Params(**kw)
    lines = [f"# track_each_bench: N={n} gl_storage=1 F={p.avg_frames} bars=n bar_phase=0.5 texels out; {torch.cuda.get_device_name(0)}",
             f"# ms = host clock around the call(s) and the synchronise that ends them, median of {args.rounds} alternating rounds (spread = max - min)",
             "# 1: `other` = glv_batch_track_rates_s16, table t * 735, every rate the batch's ur; `new` = glv_batch_track_each_s16 with that row for every stream, counts NULL",
             "# 2: `other` = one-stream batches one after another, glv_batch_track_rates_s16 over each stream's own count; `new` = glv_batch_track_each_s16, per-stream",
             "#    live_session_rates tables, a quarter of the streams at count 0, a quarter at half, the rest at all steps",
             "# 3a / 3r: `other` = glv_batch_track_at_s16 / _rates_s16 in the parent commit's library, `new` = the same entry in this library",
             "# diff = new - other; `inside`: |diff| <= the larger of the two spreads",
             f"# {'part':>4} {'streams':>7} {'steps':>6} {'other ms':>10} {'spread':>8} {'new ms':>10} {'spread':>8} {'launches':>8} {'diff ms':>9} {'inside':>6} {'other/new':>10} {'compared':>8}"]
    print("\n".join(lines), flush=True)
    points = [tuple(int(v) for v in pt.split("x")) for pt in args.points.split(",")]
    runs = [q for q in ("1", "2") if q in parts] + (["3a", "3r"] if "3" in parts else [])
    for part in runs:
        for S, steps in points:
            if part == "2":
                rows = []
                for s in range(S):
                    st, _, ur = live_session_rates(22050, FPS[s % len(FPS)], steps * 3 + 8, 256)
                    c = 0 if s % 4 == 0 else steps // 2 if s % 4 == 1 else steps
                    rows.append((st[:c], ur[:c]))
                starts, urs, counts = stack_tables(rows, steps=steps)
            else:
                starts = np.tile(np.asarray([t * hop for t in range(steps)], dtype=np.uint32), (S, 1))
                urs, counts = np.full((S, steps), p.ur, dtype=np.float32), None
            pitch = (int(starts.max()) + n + 1) | 1                               # odd
            x = lcg_pcm_fast(4242 + S, S * pitch * 2).reshape(S, pitch, 2).copy()
            d_pcm = torch.from_numpy(x).cuda()
            bn = G.Batch(p, S, mask)
            wb = bn.track_at_work_bytes(steps, ops)
            work = torch.empty((wb,), dtype=torch.uint8, device="cuda")
            out_o = torch.zeros((steps, S * 2, n), dtype=torch.int16, device="cuda")
            out_n = torch.zeros_like(out_o)
            d_starts, d_ur = u32(starts), torch.from_numpy(urs).cuda()
            d_counts = u32(counts) if counts is not None else None
            compared = True
            if part == "2":
                own = S <= 64
                compared = own
                ones = [G.Batch(p, 1, mask) for _ in range(S if own else 1)]
                row_s, row_u = [u32(starts[s]) for s in range(S)], [torch.from_numpy(urs[s].copy()).cuda() for s in range(S)]
                outs = [torch.zeros((max(int(counts[s]), 1), 2, n), dtype=torch.int16, device="cuda") for s in range(S)]

                def run_o():
                    for s in range(S):
                        c = int(counts[s])
                        if c: ones[s if own else 0].track_rates_s16(d_pcm[s], pitch, row_s[s], row_u[s], c, outs[s], work, ops)

                def run_n():
                    bn.track_each_s16(d_pcm, pitch, d_starts, d_ur, d_counts, steps, out_n, work, ops)
                others = ones
            else:
                lib_o = GP if part in ("3a", "3r") else G
                bo = lib_o.Batch(lib_o.Params(**kw), S, mask)
                others = [bo]
                row0, ur0 = u32(starts[0]), torch.from_numpy(urs[0].copy()).cuda()
                if part == "3a":
                    def run_o(): bo.track_at_s16(d_pcm, pitch, row0, steps, out_o, work, ops)
                    def run_n(): bn.track_at_s16(d_pcm, pitch, row0, steps, out_n, work, ops)
                elif part == "3r":
                    def run_o(): bo.track_rates_s16(d_pcm, pitch, row0, ur0, steps, out_o, work, ops)
                    def run_n(): bn.track_rates_s16(d_pcm, pitch, row0, ur0, steps, out_n, work, ops)
                else:
                    def run_o(): bo.track_rates_s16(d_pcm, pitch, row0, ur0, steps, out_o, work, ops)
                    def run_n(): bn.track_each_s16(d_pcm, pitch, d_starts, d_ur, None, steps, out_n, work, ops)
            run_o(); run_n(); l_n = bn.last_launches()
            for b in others + [bn]: b.reset()
            run_o(); run_n()
            torch.cuda.synchronize()
            if part == "2":
                if compared:
                    for s in range(S):
                        c = int(counts[s])
                        if c and not torch.equal(outs[s][:c], out_n[:c, 2 * s:2 * s + 2]):
                            sys.exit(f"track_each_bench: part 2 streams={S}: stream {s} differs from its one-stream batch")
                        if not bool((out_n[c:, 2 * s:2 * s + 2] == 0).all()):
                            sys.exit(f"track_each_bench: part 2 streams={S}: stream {s} has a row behind its count that is not a zero row's")
            elif not torch.equal(out_o, out_n):
                sys.exit(f"track_each_bench: part {part} streams={S}: the two forms' outputs differ")
            to, tn = [], []
            for _ in range(args.rounds):
                to.append(timed(run_o)); tn.append(timed(run_n))
            mo, mn = float(np.median(to)), float(np.median(tn))
            so, sn = max(to) - min(to), max(tn) - min(tn)
            line = (f"  {part:>4} {S:>7} {steps:>6} {mo:>10.3f} {so:>8.3f} {mn:>10.3f} {sn:>8.3f} {l_n:>8} {mn - mo:>+9.3f} {'yes' if abs(mn - mo) <= max(so, sn) else 'NO':>6} {mo / mn:>10.3f}"
                    f" {'yes' if compared else 'no':>8}")
            print(line, flush=True)
            lines.append(line)
            for b in others + [bn]: b.close()
            del d_pcm, work, out_o, out_n
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
