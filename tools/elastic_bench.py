"""Elastic batches (glv_batch_process_first_s16, glv_batch_copy_streams): what a half-empty batch costs, and what moving streams costs without the blob.

    python tools/elastic_bench.py [--n 4096] [--streams 65536] [--prefixes 8192,32768,0] [--counts 1,64,4096,0] [--rounds 7] [--out profiles/r23/elastic.txt]

The batches are the shipped GL chain (gl_storage 1, F = 5: uint16 state, 24 n bytes per stream), texels out.  A prefix or count of 0 is every stream.
  part a   glv_batch_process_first_s16(count) on the capacity batch beside glv_batch_process_s16 on a batch created with exactly `count` streams: the same
           kernel on the same rows, so a difference is the state arrays' placement (profiles/r06/modes.txt: 7 - 14 % between placements of one process),
           which this tool cannot read -- every batch here is a hipMalloc of its own, made once, and the figures say which batch they are of
  part b   glv_batch_copy_streams of `count` streams, evenly spread, between two batches at different heads (2 and 4) and inside one batch (the upper half's
           streams into the lower half's), beside glv_batch_save_streams + glv_batch_load_streams of the same streams; bytes = streams x bytes per stream x 2
The project's protocol: every configuration is warmed up once, then timed `rounds` times, the configurations alternating within a round; median ms between
HIP events with the round-to-round spread (max - min).  Figures are reported, none is judged."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from glava_amd import spectrum as G  # noqa: E402
from stream_slots_bench import alternate  # noqa: E402


def table(values):
    return torch.from_numpy(np.asarray(values, dtype=np.uint32).view(np.int32).copy()).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--prefixes", default="8192,32768,0", help="part a: streams updated; 0: all")
    ap.add_argument("--counts", default="1,64,4096,0", help="part b: streams copied per call; 0: all (inside one batch: half)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "r23", "elastic.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("elastic_bench: no GPU -- nothing is measured without one")
    n, S = args.n, args.streams
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    ops = G.OP_FFT | GA | G.OP_R16
    params = G.Params(n=n, gl_storage=1, avg_window_kind=1)
    pcm = torch.empty((S * n * 2,), dtype=torch.int16, device="cuda").random_(-20000, 20000)
    out = torch.zeros((S * 2, n), dtype=torch.int16, device="cuda")
    ceiling = json.load(open(os.path.join(ROOT, "profiles", "stream_ceiling.json")))
    lines = [f"# elastic_bench: N={n} F=5 gl_storage 1 (uint16 state), capacity {S} streams; {torch.cuda.get_device_name(0)}",
             f"# median of {args.rounds} rounds in which the configurations alternate (spread = max - min); ms between HIP events around the call(s)",
             "# part a: process_first_s16(count) on the capacity batch / process_s16 on a batch of exactly `count` streams (FFT | GRAVITY | AVERAGE, texels out); the same",
             "#         kernel on the same rows -- every batch's state is its own hipMalloc, whose placement relative to the output buffer this tool cannot read",
             f"# {'call':>28} {'streams':>8} {'ms':>9} {'spread':>8}"]
    print("\n".join(lines), flush=True)

    # ---- part a ----
    prefixes = [S if int(c) == 0 else int(c) for c in args.prefixes.split(",")]
    cap = G.Batch(params, S, GA)
    exact = {c: G.Batch(params, c, GA) for c in prefixes}
    runs = {}
    for c in prefixes:
        runs[("first on the capacity batch", c)] = lambda c=c: cap.process_first_s16(c, pcm, out, ops)
        runs[("batch of that size", c)] = lambda c=c: exact[c].process_s16(pcm, out, ops)
    res = alternate(runs, args.rounds)
    for (call, c), (ms, spread) in res.items():
        line = f"  {call:>28} {c:>8} {ms:>9.4f} {spread:>8.4f}"
        print(line, flush=True); lines.append(line)
    for c in prefixes:
        a, b = res[("first on the capacity batch", c)], res[("batch of that size", c)]
        lines.append(f"# {c} streams: prefix - exact = {a[0] - b[0]:+.4f} ms ({100 * (a[0] - b[0]) / b[0]:+.2f} %), spreads {a[1]:.4f} / {b[1]:.4f}")
        print(lines[-1], flush=True)
    for b in exact.values(): b.close()

    # ---- part b ----
    other = G.Batch(params, S, GA)
    cap.reset()
    for _ in range(7): cap.process_s16(pcm, out, ops)           # head 2, every ring slot written
    for _ in range(4): other.process_s16(pcm, out, ops)         # head 4
    torch.cuda.synchronize()
    per = int(cap.stream_state_desc().bytes)
    counts = [S if int(c) == 0 else int(c) for c in args.counts.split(",")]
    blob = torch.empty((max(counts) * per,), dtype=torch.uint8, device="cuda")
    spread_t = {c: table(np.arange(c, dtype=np.uint64) * (S // c)) for c in counts}
    half = {c: min(c, S // 2) for c in counts}
    lower = {c: table(np.arange(half[c], dtype=np.uint64) * ((S // 2) // half[c])) for c in counts}
    upper = {c: table(S // 2 + np.arange(half[c], dtype=np.uint64) * ((S // 2) // half[c])) for c in counts}
    lines += ["# part b: streams copied from the capacity batch (head 2) into a second one (head 4), by glv_batch_copy_streams and by save + load through a blob; and",
              f"#         inside the capacity batch, upper half into lower half.  {per} bytes per stream; moved = streams x bytes per stream x 2 (read + written)",
              f"# profiles/stream_ceiling.json: {json.dumps(ceiling)[:200]}",
              f"# {'call':>28} {'streams':>8} {'ms':>9} {'spread':>8} {'MiB moved':>10} {'GB/s':>8} {'% of ceiling':>12}"]
    print("\n".join(lines[-4:]), flush=True)

    def by_blob(dst, d_dst, src, d_src, c):
        d = src.save_streams(d_src, c, blob)
        dst.load_streams(d_dst, c, blob, d)
    runs = {}
    for c in counts:
        runs[("copy, two batches", c)] = lambda c=c: other.copy_streams(spread_t[c], cap, spread_t[c], c)
        runs[("save + load, two batches", c)] = lambda c=c: by_blob(other, spread_t[c], cap, spread_t[c], c)
        runs[("copy, one batch", half[c])] = lambda c=c: cap.copy_streams(lower[c], cap, upper[c], half[c])
        runs[("save + load, one batch", half[c])] = lambda c=c: by_blob(cap, lower[c], cap, upper[c], half[c])
    res = alternate(runs, args.rounds)
    for (call, c), (ms, spread) in res.items():
        moved = 2 * c * per
        rate = moved / (ms * 1e-3) / 1e9
        line = f"  {call:>28} {c:>8} {ms:>9.4f} {spread:>8.4f} {moved / 2 ** 20:>10.2f} {rate:>8.0f} {100 * rate / ceiling['gbs']:>12.1f}"
        print(line, flush=True); lines.append(line)
    cap.close(); other.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
