"""gl_storage 3 (the CPU operators on float state, GLV_OP_BARS over the GL_R16 upload: GLava with `setaccelfft false`) beside what existed, alternating in
one process.

  (a) existing entries in this library against the library built from the parent commit (--parent-lib, loaded beside this one): the gl_storage 0 chain
      with GLV_OP_R16 out, the shipped gl_storage 1 pipeline (bars = n, bar_phase 0.5, texels out) -- both at --streams x N -- and glv_batch_track_at_s16
      on the shipped pipeline at the four track shapes (the table t * 735)
  (n) the new path, for orientation: PCM -> pre-smoothed texels on gl_storage 3 (bars = n, bar_phase 0.5, texels out) beside the gl_storage 0 chain with
      GLV_OP_R16 out (the part of the work that already existed), and beside the gl_storage 1 pipeline
  (f) the rule for the one-launch classes FC_STATE_SNAP / FC_STATE_COLS: the radial bar texels and a 320-pixel column table on gl_storage 3 in one launch
      against the two-launch route (a batch created under GLV_UNFUSED_BARS: kernels the parent already has)

    python tools/upload_chain_bench.py [--streams 65536] [--n 4096] [--points 1x2048,8x2048,64x2048,1024x256] [--rounds 7] [--parts a,n,f]
                                       [--parent-lib PATH] [--new-first] [--out profiles/r18/upload_chain.txt]

The protocol of tools/track_rates_bench.py.  Per line: both forms are warmed up, their outputs compared bit for bit from a reset state where they compute
the same thing, then timed `rounds` times alternating (a host clock around the call and the device synchronise that ends it).  Prints and writes the
table: median ms of each form with the round-to-round spread (max - min) and the ratio.  A difference inside the spread is none.  Part a is left out where
no parent library is given.
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
from glava_amd.bar_positions import graph_column_texels, radial_bar_texels  # noqa: E402
from oracle_lib import lcg_pcm_fast  # noqa: E402
from track_at_bench import load_other, timed  # noqa: E402


def unfused(make):
    os.environ["GLV_UNFUSED_BARS"] = "1"
    try:
        return make()
    finally:
        del os.environ["GLV_UNFUSED_BARS"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--points", default="1x2048,8x2048,64x2048,1024x256", help="streams x steps of the track shapes")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parts", default="a,n,f")
    ap.add_argument("--parent-lib", default=None, help="libglvspectrum.so built from the parent commit (part a)")
    ap.add_argument("--new-first", action="store_true", help="part a's process-call lines: create this library's batch before the parent's (the state arrays' "
                    "placement follows the order of creation, and a stateful chain's speed follows the placement)")
    ap.add_argument("--out", default=os.path.join("profiles", "r18", "upload_chain.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("upload_chain_bench: no GPU -- nothing is measured without one")
    n, S, hop = args.n, args.streams, 735
    parts = [q for q in args.parts.split(",") if q != "a" or args.parent_lib]
    GP = load_other(args.parent_lib) if "a" in parts else None
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    chain = G.OP_FFT | GA
    lines = [f"# upload_chain_bench: N={n} F=5 log_mode=1; {torch.cuda.get_device_name(0)}",
             f"# ms = host clock around the call and the synchronise that ends it, median of {args.rounds} alternating rounds (spread = max - min)",
             "# a: `other` = the entry in the parent commit's library, `new` = the same entry in this library",
             "# n: `new` = gl_storage 3, bars = n, bar_phase 0.5, texels out (PCM -> pre-smoothed texels); `other` = the entry named",
             "# f: `other` = the two-launch route (GLV_UNFUSED_BARS), `new` = the one-launch class, same table, floats out",
             f"# {'part':>4} {'entry':<34} {'streams':>7} {'steps':>6} {'other ms':>10} {'spread':>8} {'launches':>8} {'new ms':>10} {'spread':>8} {'launches':>8} {'other/new':>10}"]
    print("\n".join(lines), flush=True)

    def report(part, entry, streams, steps, run_o, run_n, bo, bn, out_o, out_n, same):
        run_o(); l_o = bo.last_launches()
        run_n(); l_n = bn.last_launches()
        bo.reset(); bn.reset()
        run_o(); run_n()
        torch.cuda.synchronize()
        if same and not torch.equal(out_o, out_n):
            sys.exit(f"upload_chain_bench: part {part} {entry}: the two forms' outputs differ")
        to, tn = [], []
        for _ in range(args.rounds):
            to.append(timed(run_o)); tn.append(timed(run_n))
        mo, mn = float(np.median(to)), float(np.median(tn))
        line = (f"  {part:>4} {entry:<34} {streams:>7} {steps:>6} {mo:>10.3f} {max(to) - min(to):>8.3f} {l_o:>8} {mn:>10.3f} {max(tn) - min(tn):>8.3f} {l_n:>8} {mo / mn:>10.3f}")
        print(line, flush=True)
        lines.append(line)

    kw0 = dict(n=n, log_mode=1)
    kw1 = dict(n=n, log_mode=1, gl_storage=1, avg_window_kind=1, bars=n, bar_phase=0.5)
    kw3 = dict(n=n, log_mode=1, gl_storage=3, bars=n, bar_phase=0.5)
    pcm = torch.from_numpy(lcg_pcm_fast(4242, S * 2 * n)).cuda()
    tex_o = torch.zeros((S * 2, n), dtype=torch.int16, device="cuda")
    tex_n = torch.zeros_like(tex_o)

    def pair(mod_o, kw_o, mask_o, ops_o, mod_n, kw_n, mask_n, ops_n, part, entry, same):
        if args.new_first and part == "a":
            bn = mod_n.Batch(mod_n.Params(**kw_n), S, mask_n); bo = mod_o.Batch(mod_o.Params(**kw_o), S, mask_o)
        else:
            bo, bn = mod_o.Batch(mod_o.Params(**kw_o), S, mask_o), mod_n.Batch(mod_n.Params(**kw_n), S, mask_n)
        report(part, entry, S, 1, lambda: bo.process_s16(pcm, tex_o, ops_o), lambda: bn.process_s16(pcm, tex_n, ops_n), bo, bn, tex_o, tex_n, same)
        bo.close(); bn.close()

    if "a" in parts:
        pair(GP, kw0, GA, chain | G.OP_R16, G, kw0, GA, chain | G.OP_R16, "a", "gl_storage 0 chain, R16 out", True)
        pair(GP, kw1, GA | G.OP_BARS, chain | G.OP_BARS | G.OP_R16, G, kw1, GA | G.OP_BARS, chain | G.OP_BARS | G.OP_R16, "a", "gl_storage 1 pipeline", True)
    if "n" in parts:
        pair(G, kw0, GA, chain | G.OP_R16, G, kw3, GA | G.OP_BARS, chain | G.OP_BARS | G.OP_R16, "n", "vs gl_storage 0 chain, R16 out", False)
        pair(G, kw1, GA | G.OP_BARS, chain | G.OP_BARS | G.OP_R16, G, kw3, GA | G.OP_BARS, chain | G.OP_BARS | G.OP_R16, "n", "vs gl_storage 1 pipeline", False)
    if "f" in parts:
        radial = radial_bar_texels(n, 160)[0]
        cols = graph_column_texels(n, 320)[0]
        for name, table, setter in (("radial bar texels", radial, "set_bar_texels"), ("320-pixel columns", cols, "set_column_texels")):
            def make():
                b = G.Batch(G.Params(n=n, log_mode=1, gl_storage=3, bars=len(table)), S, GA | G.OP_BARS)
                getattr(b, setter)(table)
                return b
            bo, bn = unfused(make), make()
            oo = torch.zeros((S * 2, len(table)), dtype=torch.float32, device="cuda"); on = torch.zeros_like(oo)
            report("f", name, S, 1, lambda: bo.process_s16(pcm, oo, chain | G.OP_BARS), lambda: bn.process_s16(pcm, on, chain | G.OP_BARS), bo, bn, oo.view(torch.int32),
                   on.view(torch.int32), True)
            bo.close(); bn.close()
            del oo, on
    del pcm, tex_o, tex_n
    torch.cuda.empty_cache()
    if "a" in parts:
        mask, ops = GA | G.OP_BARS, chain | G.OP_BARS | G.OP_R16
        for streams, steps in [tuple(int(v) for v in pt.split("x")) for pt in args.points.split(",")]:
            starts = [t * hop for t in range(steps)]
            pitch = (max(starts) + n + 1) | 1
            bo, bn = GP.Batch(GP.Params(**kw1), streams, mask), G.Batch(G.Params(**kw1), streams, mask)
            wb = bn.track_at_work_bytes(steps, ops)
            d_pcm = torch.from_numpy(lcg_pcm_fast(4242 + streams, streams * pitch * 2)).cuda()
            d_starts = torch.from_numpy(np.asarray(starts, dtype=np.uint32).view(np.int32).copy()).cuda()
            work = torch.empty((wb,), dtype=torch.uint8, device="cuda")
            out_o = torch.zeros((steps, streams * 2, n), dtype=torch.int16, device="cuda"); out_n = torch.zeros_like(out_o)
            report("a", "glv_batch_track_at_s16", streams, steps, lambda: bo.track_at_s16(d_pcm, pitch, d_starts, steps, out_o, work, ops),
                   lambda: bn.track_at_s16(d_pcm, pitch, d_starts, steps, out_n, work, ops), bo, bn, out_o, out_n, True)
            bo.close(); bn.close()
            del d_pcm, work, out_o, out_n
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
