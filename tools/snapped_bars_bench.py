"""Bars at texels of the pre-smoothing pass: the two ways to get them, alternating A/B in one process (HIP events, warm-up).

  (a) twin    the GL_R16 chain with bars = n, bar_phase 0.5 (frame kernel + the i8 matrix-core pass over every texel), then a gather
              of the 80 texels the radial module samples -- what a caller had to do before glv_batch_set_bar_texels
  (b) snapped the same chain with bars = 80 and the texel table set: the integer sums in the frame kernel's epilogue, one launch
  (c) fused   for scale: the unsnapped fused bars (GLV_OP_BARS at k / 80, setsmoothpass false semantics), one launch

    python tools/snapped_bars_bench.py [--streams 65536] [--n 4096] [--iters 20] [--rounds 5]
Prints one line per round and the medians in M frames/s (a frame = one stereo frame of one stream).  Checks (b) == (a) bit for bit first.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from glava_amd import spectrum as G  # noqa: E402
from glava_amd.bar_positions import radial_bar_texels  # noqa: E402
from oracle_lib import lcg_pcm_fast  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    S, n = args.streams, args.n
    tex = radial_bar_texels(n, 160)[0]
    mask = G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS | G.OP_BARS_ONLY
    kw = dict(n=n, gl_storage=1, avg_window_kind=1, log_mode=1)
    twin = G.Batch(G.Params(bars=n, bar_phase=0.5, **kw), S, mask)
    snap = G.Batch(G.Params(bars=80, **kw), S, mask)
    snap.set_bar_texels(tex)
    plain = G.Batch(G.Params(bars=80, **kw), S, mask)
    ops = G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS | G.OP_R16
    pcm = torch.from_numpy(lcg_pcm_fast(1234, S * 2 * n)).cuda()
    out_t = torch.empty((S * 2, n), dtype=torch.int16, device="cuda")
    gathered = torch.empty((S * 2, 80), dtype=torch.int16, device="cuda")
    out_s = torch.empty((S * 2, 80), dtype=torch.int16, device="cuda")
    out_p = torch.empty((S * 2, 80), dtype=torch.int16, device="cuda")
    idx = torch.from_numpy(tex.astype(np.int64)).cuda()

    def run_a():
        twin.process_s16(pcm, out_t, ops)
        torch.index_select(out_t, 1, idx, out=gathered)

    def run_b():
        snap.process_s16(pcm, out_s, ops)

    def run_c():
        plain.process_s16(pcm, out_p, ops)

    for _ in range(3):
        run_a(); run_b(); run_c()
    torch.cuda.synchronize()
    assert torch.equal(gathered, out_s), "snapped bars differ from the twin's texels"
    print(f"streams={S} n={n} bars=80 (radial texels); launches: twin {twin.last_launches()} + gather, snapped {snap.last_launches()}, "
          f"unsnapped fused {plain.last_launches()}; (b) == (a) bit for bit", flush=True)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.iters

    res = {"a": [], "b": [], "c": []}
    for r in range(args.rounds):
        for k, fn in (("a", run_a), ("b", run_b), ("c", run_c)) if r % 2 == 0 else (("c", run_c), ("b", run_b), ("a", run_a)):
            res[k].append(timed(fn))
        print(f"round {r}: (a) twin+gather {res['a'][-1]:.3f} ms  (b) snapped {res['b'][-1]:.3f} ms  (c) unsnapped fused {res['c'][-1]:.3f} ms", flush=True)
    med = {k: float(np.median(v)) for k, v in res.items()}
    mfps = {k: S / (v * 1e-3) / 1e6 for k, v in med.items()}
    print(f"median: (a) {med['a']:.3f} ms = {mfps['a']:.1f} M frames/s   (b) {med['b']:.3f} ms = {mfps['b']:.1f} M frames/s   "
          f"(c) {med['c']:.3f} ms = {mfps['c']:.1f} M frames/s   (b)/(a) speed-up {med['a'] / med['b']:.2f}x   (b) vs (c) {med['b'] / med['c']:.2f}x time")
    for b in (twin, snap, plain):
        b.close()


if __name__ == "__main__":
    main()
