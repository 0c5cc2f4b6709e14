"""The texture the wave module samples (GLV_OP_WAVE | GLV_OP_BARS | GLV_OP_R16, bars = n, bar_phase 0.5): its two forms, alternating in one process.

  (one)  the integer pre-smoothing pass straight from the s16 frames: unpack, wrange and the upload's quantisation on the way into LDS, ONE launch
  (two)  GLV_UNFUSED_WAVE at creation: the waveform kernel writes the upload's texels the bars sample, then the pass over those rows -- the kernel the
         GL_R16 chain already launched second, plus the trivial waveform kernel
  (gl)   for orientation, the GL_R16 spectrum chain (FFT + gravity + average) of the same streams with and without its pre-smoothing launch: the
         difference is about that launch over the same rows (about: with the pass the chain's first launch stores only the bins the pass samples)

    python tools/wave_texture_bench.py [--streams 65536] [--n 4096] [--iters 20] [--rounds 7]
Times are HIP events around every launch of a call (glv_batch_timing_*), ms per call of all streams, warm; one line per round (the order of the forms
alternates) and the medians with their round-to-round spread.  The two forms' texels are compared first: they must be equal.
The (gl+pass) - (gl) difference is only about the pass's own time; for the launch itself run a short pass of this tool under
    rocprofv3 --kernel-trace --stats -- python tools/wave_texture_bench.py --rounds 2 --iters 10
and read glv_bars_rows_i8_kernel's rows: the texel-source instantiation is the GL chain's (and the two-launch form's) second launch, the PCM-source one the one-launch form.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from glava_amd import spectrum as G  # noqa: E402
from oracle_lib import lcg_pcm_fast  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    S, n = args.streams, args.n
    p = G.Params(n=n, bars=n, bar_phase=0.5, gl_storage=1, avg_window_kind=1)
    ops = G.OP_WAVE | G.OP_BARS | G.OP_R16
    pcm = torch.from_numpy(lcg_pcm_fast(1234, S * 2 * n)).cuda()
    one = G.Batch(p, S, G.OP_WAVE | G.OP_BARS)
    os.environ["GLV_UNFUSED_WAVE"] = "1"
    two = G.Batch(p, S, G.OP_WAVE | G.OP_BARS)
    del os.environ["GLV_UNFUSED_WAVE"]
    gl = G.Batch(p, S, G.OP_GRAVITY | G.OP_AVERAGE | G.OP_BARS)
    gl0 = G.Batch(p, S, G.OP_GRAVITY | G.OP_AVERAGE)
    gl_ops = G.OP_FFT | G.OP_GRAVITY | G.OP_AVERAGE | G.OP_R16
    out1 = torch.empty((S * 2, n), dtype=torch.int16, device="cuda")
    out2 = torch.empty((S * 2, n), dtype=torch.int16, device="cuda")

    def timed(b, fn):
        b.timing_begin()
        for _ in range(args.iters):
            fn()
        ms, _ = b.timing_end()
        return ms / args.iters

    forms = [("one", one, lambda: one.process_s16(pcm, out1, ops)),
             ("two", two, lambda: two.process_s16(pcm, out2, ops)),
             ("gl+pass", gl, lambda: gl.process_s16(pcm, out2, gl_ops | G.OP_BARS)),
             ("gl", gl0, lambda: gl0.process_s16(pcm, out2, gl_ops))]
    for _ in range(5):                                       # warm: clocks, caches, the first launch of every kernel
        for _, _, fn in forms:
            fn()
    torch.cuda.synchronize()
    one.process_s16(pcm, out1, ops); l1 = one.last_launches(); k1 = one.kernel_name()
    two.process_s16(pcm, out2, ops); l2 = two.last_launches(); k2 = two.kernel_name()
    torch.cuda.synchronize()
    assert torch.equal(out1, out2), "the two forms differ"
    gl.process_s16(pcm, out2, gl_ops | G.OP_BARS); lg = gl.last_launches()
    torch.cuda.synchronize()
    print(f"streams={S} n={n} bars={n}: (one) {l1} launch(es), {k1}; (two) {l2} launch(es), first {k2}; texels equal; the GL chain with its pass: {lg} launches; "
          f"algorithmic bytes per call {one.algorithmic_bytes(ops, True)} (input below bin {(one.algorithmic_bytes(ops, True) // S - 4 * n) // 4})", flush=True)
    res = {k: [] for k, _, _ in forms}
    for r in range(args.rounds):
        for k, b, fn in forms if r % 2 == 0 else forms[::-1]:
            res[k].append(timed(b, fn))
        print(f"  round {r}: " + "  ".join(f"({k}) {res[k][-1]:.3f} ms" for k, _, _ in forms), flush=True)
    med = {k: float(np.median(v)) for k, v in res.items()}
    spread = {k: max(v) - min(v) for k, v in res.items()}
    print("  median: " + "   ".join(f"({k}) {med[k]:.3f} ms (spread {spread[k]:.3f})" for k, _, _ in forms), flush=True)
    print(f"  (one) {S / (med['one'] * 1e-3) / 1e6:.1f} M frames/s, (two) {S / (med['two'] * 1e-3) / 1e6:.1f} M frames/s, (two)/(one) {med['two'] / med['one']:.2f}x; "
          f"the GL chain's pre-smoothing launch over the same {S * 2} rows: {med['gl+pass'] - med['gl']:.3f} ms (gl+pass - gl)", flush=True)
    for b in (one, two, gl, gl0):
        b.close()


if __name__ == "__main__":
    main()
