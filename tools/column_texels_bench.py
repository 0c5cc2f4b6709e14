"""The graph module's columns (means of three texels of the pre-smoothing pass): the ways to get them, alternating in one process (HIP events).

  (a) twin     the GL_R16 chain with bars = n, bar_phase 0.5 (frame kernel + the i8 matrix-core pass over every texel), then a gather of the
               column texels and their float average in torch -- what a caller had to do before glv_batch_set_column_texels
  (b) columns  the same chain with bars = columns and the column table set, on the route the library plans (reported per width)
  (c) second   (b) forced onto the second launch (GLV_UNFUSED_BARS at creation), where (b) took the fused route: the other route, for the threshold

    python tools/column_texels_bench.py [--streams 65536] [--n 4096] [--widths 320,800,1920] [--iters 20] [--rounds 7]
Prints one line per round and width and the medians (ms per update of all streams; M frames/s, a frame = one stereo frame of one stream) with the
round-to-round spread (max - min) of each.  Counts the values of (b) that differ from the twin's texels averaged on the CPU in float32 first.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from glava_amd import spectrum as G  # noqa: E402
from glava_amd.bar_positions import graph_column_texels  # noqa: E402
from oracle_lib import lcg_pcm_fast  # noqa: E402

F = np.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--widths", default="320,800,1920")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    S, n = args.streams, args.n
    mask = G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS | G.OP_BARS_ONLY
    kw = dict(n=n, gl_storage=1, avg_window_kind=1, log_mode=1)
    ops = G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS
    pcm = torch.from_numpy(lcg_pcm_fast(1234, S * 2 * n)).cuda()
    twin = G.Batch(G.Params(bars=n, bar_phase=0.5, **kw), S, mask)
    out_t = torch.empty((S * 2, n), dtype=torch.int16, device="cuda")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.iters

    for W in [int(w) for w in args.widths.split(",")]:
        table = graph_column_texels(n, W)[0].astype(np.int64)
        cnt = len(table)
        cols = G.Batch(G.Params(bars=cnt, **kw), S, mask)
        cols.set_column_texels(table)
        twin.reset()                                       # the chains are stateful: (a) and (b) run the same number of updates from here on
        idx = torch.from_numpy(table.reshape(-1)).cuda()
        gathered = torch.empty((S * 2, 3 * cnt), dtype=torch.int16, device="cuda")
        out_a = torch.empty((S * 2, cnt), dtype=torch.float32, device="cuda")
        out_b = torch.empty((S * 2, cnt), dtype=torch.float32, device="cuda")
        out_c = torch.empty((S * 2, cnt), dtype=torch.float32, device="cuda")

        def run_a():
            twin.process_s16(pcm, out_t, ops | G.OP_R16)
            torch.index_select(out_t, 1, idx, out=gathered)
            t = (gathered.to(torch.int32) & 0xffff).to(torch.float32).div_(65535.0).view(S * 2, cnt, 3)
            torch.div((t[:, :, 0] + t[:, :, 1]) + t[:, :, 2], 3.0, out=out_a)

        def run_b():
            cols.process_s16(pcm, out_b, ops)

        for _ in range(3):
            run_a(); run_b()
        torch.cuda.synchronize()
        route = {1: "fused (one launch)", 2: "second launch (glv_columns_kernel)"}[cols.last_launches()]
        rows = out_t[:64].cpu().numpy().view(np.uint16)
        T = (rows.astype(F) / F(65535)).astype(F)
        want = (((T[:, table[:, 0]] + T[:, table[:, 1]]).astype(F) + T[:, table[:, 2]]).astype(F) / F(3)).astype(F)
        bad = int((out_b[:64].cpu().numpy().view(np.uint32) != want.view(np.uint32)).sum())
        bad_a = int((out_a[:64].cpu().numpy().view(np.uint32) != want.view(np.uint32)).sum())
        second = None
        if cols.last_launches() == 1:
            os.environ["GLV_UNFUSED_BARS"] = "1"
            second = G.Batch(G.Params(bars=cnt, **kw), S, mask)
            del os.environ["GLV_UNFUSED_BARS"]
            second.set_column_texels(table)
            for _ in range(3):
                second.process_s16(pcm, out_c, ops)
            torch.cuda.synchronize()
            assert second.last_launches() == 2
            assert torch.equal(out_c.view(torch.int32), out_b.view(torch.int32)), "the two routes differ"
        print(f"width {W}: streams={S} n={n} columns={cnt} over {len(np.unique(table))} distinct texels; (b) route: {route}; values of the first 64 rows that "
              f"differ from the twin's texels averaged in float32 on the CPU: (b) {bad}, (a) in torch {bad_a}", flush=True)
        assert bad == 0, "columns differ from the contract"
        fns = [("a", run_a), ("b", run_b)] + ([("c", lambda: second.process_s16(pcm, out_c, ops))] if second else [])
        res = {k: [] for k, _ in fns}
        for r in range(args.rounds):
            for k, fn in fns if r % 2 == 0 else fns[::-1]:
                res[k].append(timed(fn))
            print(f"  round {r}: " + "  ".join(f"({k}) {res[k][-1]:.3f} ms" for k, _ in fns), flush=True)
        med = {k: float(np.median(v)) for k, v in res.items()}
        spread = {k: max(v) - min(v) for k, v in res.items()}
        print(f"  median: " + "   ".join(f"({k}) {med[k]:.3f} ms (spread {spread[k]:.3f}) = {S / (med[k] * 1e-3) / 1e6:.1f} M frames/s" for k, _ in fns)
              + f"   (a)/(b) {med['a'] / med['b']:.2f}x" + (f"   (c)/(b) {med['c'] / med['b']:.2f}x" if second else ""), flush=True)
        cols.close()
        if second:
            second.close()
        del gathered, out_a, out_b, out_c
    twin.close()


if __name__ == "__main__":
    main()
