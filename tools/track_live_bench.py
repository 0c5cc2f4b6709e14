"""Track mode for GLV_OP_BARS_ONLY batches (glv_batch_track_live_s16) against what a caller had before it, alternating in one process.

  (a) live        glv_batch_track_live_s16 on a flagged batch: the windows form's transform, the scan over the kept bins
  (b) windows     glv_batch_track_windows_s16 on an unflagged batch, from a library built from the commit BEFORE the live entry (--parent-lib: a second
                  copy of the library loaded beside the product; without it the column is skipped)
  (c) one by one  the same windows through glv_batch_process_s16 on a flagged batch (windows cut beforehand, not counted)

(A fourth column, the live entry with live classes for the transform behind a creation-time switch, decided that those classes go: its one run is
profiles/r15/track_live_rule.txt, where column (d) is the form that ships and (a) the one that left.)

The shipped pipeline: N = 4096, hop 735, an odd pitch, the GL chain (gl_storage 1, F = 5) with the pre-smoothing pass (bars = n, bar_phase 0.5), texels out.

    python tools/track_live_bench.py [--points 1x2048,8x2048,64x2048,1024x256] [--rounds 7] [--parent-lib PATH] [--out profiles/r15/track_live.txt]

Per point: every form is warmed up once, the outputs compared bit for bit from a reset state, then timed `rounds` times alternating (a host clock around the
call and the synchronise that ends it).  Prints and writes the table: median ms of each form with the round-to-round spread (max - min).  A difference inside
the spread is none.
"""
import argparse
import importlib.util
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from glava_amd import spectrum as G  # noqa: E402
from oracle_lib import lcg_pcm_fast  # noqa: E402


def second_library(path):
    """the Python mirror bound to another copy of the library (its own module object, its own ctypes handle)"""
    spec = importlib.util.spec_from_file_location("glv_parent_spectrum", os.path.join(ROOT, "glava_amd", "spectrum.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["glv_parent_spectrum"] = mod
    os.environ["GLV_SPECTRUM_LIB"] = os.path.abspath(path)
    try:
        spec.loader.exec_module(mod)
        mod.lib()
    finally:
        del os.environ["GLV_SPECTRUM_LIB"]
    return mod


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
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join("profiles", "r15", "track_live.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("track_live_bench: no GPU -- nothing is measured without one")
    G.lib()
    P = second_library(args.parent_lib) if args.parent_lib else None
    n, hop = args.n, args.hop
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    mask, ops = GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS | G.OP_R16
    kw = dict(n=n, gl_storage=1, avg_window_kind=1, log_mode=1, bars=n, bar_phase=0.5)
    p = G.Params(**kw)
    lines = [f"# track_live_bench: N={n} hop={hop} gl_storage=1 F={p.avg_frames} bars=n bar_phase=0.5 texels out; {torch.cuda.get_device_name(0)}",
             f"# ms = host clock around the call(s) and the synchronise that ends them, median of {args.rounds} alternating rounds (spread = max - min)",
             "# (a) glv_batch_track_live_s16   (b) glv_batch_track_windows_s16, unflagged batch, the library before the live entry"
             + ("" if P else " -- NOT MEASURED: no --parent-lib"),
             "# (c) the same windows through glv_batch_process_s16 one by one on a flagged batch",
             f"# {'streams':>7} {'steps':>6} {'live bins':>9}   {'(a) ms':>9} {'spread':>7}   {'(b) ms':>9} {'spread':>7}   {'(c) ms':>9} {'spread':>7}   {'b/a':>5} {'c/a':>5}"]
    print("\n".join(lines), flush=True)
    for S, steps in [tuple(int(v) for v in pt.split("x")) for pt in args.points.split(",")]:
        pitch = n + (steps - 1) * hop + 1
        ba, bc = G.Batch(p, S, mask | G.OP_BARS_ONLY), G.Batch(p, S, mask | G.OP_BARS_ONLY)
        bb = P.Batch(P.Params(**kw), S, mask) if P else None
        wb = ba.track_live_work_bytes(pitch, hop, steps, ops)
        if bb: assert bb.track_windows_work_bytes(pitch, hop, steps, ops) == wb
        x = lcg_pcm_fast(4242 + S, (S * pitch + 2) * 2).reshape(-1, 2)
        buf = torch.from_numpy(x).cuda()
        d_pcm = buf[:S * pitch].view(S, pitch, 2)
        work = torch.empty((wb,), dtype=torch.uint8, device="cuda")
        outs = {k: torch.zeros((steps, S * 2, n), dtype=torch.int16, device="cuda") for k in "abc"}
        wins = torch.stack([d_pcm[:, t * hop:t * hop + n, :] for t in range(steps)]).contiguous()         # [steps][S][n][2]

        def run_a(): ba.track_live_s16(d_pcm, pitch, hop, steps, outs["a"], work, ops)
        def run_b(): bb.track_windows_s16(d_pcm, pitch, hop, steps, outs["b"], work, ops)

        def run_c():
            for t in range(steps):
                bc.process_s16(wins[t], outs["c"][t], ops)

        runs = [("a", run_a, ba)] + ([("b", run_b, bb)] if bb else []) + [("c", run_c, bc)]
        for _, fn, _b in runs: fn()
        for _, _fn, b in runs: b.reset()
        for _, fn, _b in runs: fn()
        torch.cuda.synchronize()
        for k, _fn, _b in runs:
            if not torch.equal(outs[k], outs["a"]):
                sys.exit(f"track_live_bench: streams={S}: form ({k}) differs from the live entry")
        ts = {k: [] for k, _, _ in runs}
        for _ in range(args.rounds):
            for k, fn, _b in runs: ts[k].append(timed(fn))
        med = {k: float(np.median(v)) for k, v in ts.items()}
        spr = {k: max(v) - min(v) for k, v in ts.items()}
        cell = lambda k: f"{med[k]:>9.3f} {spr[k]:>7.3f}" if k in med else f"{'n/a':>9} {'':>7}"      # noqa: E731
        ratio = lambda k: f"{med[k] / med['a']:>5.2f}" if k in med else f"{'n/a':>5}"                  # noqa: E731
        line = f"  {S:>7} {steps:>6} {ba.live_bins():>9}   {cell('a')}   {cell('b')}   {cell('c')}   {ratio('b')} {ratio('c')}"
        print(line, flush=True)
        lines.append(line)
        for _, _fn, b in runs: b.close()
        del buf, d_pcm, work, outs, wins
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
