"""Stream slots (glv_batch_reset_streams / _save_streams / _load_streams): what the one launch costs for 1, 64, 4096 and all streams of the headline batch, the
bytes it moves per second beside profiles/stream_ceiling.json, and -- the figure a service cares about -- what resetting ONE stream costs beside one
glv_batch_process_s16 of the whole batch.  For orientation: glv_batch_reset (synchronous memsets of every array) on the same batch.

    python tools/stream_slots_bench.py [--n 4096] [--streams 65536] [--counts 1,64,4096,0] [--rounds 7] [--out profiles/r22/stream_slots.txt]

The batch is the shipped GL chain (gl_storage 1, F = 5: uint16 state, 24 n bytes per stream).  A count of 0 is every stream.  Listed streams are spread evenly
over the batch.  Bytes moved: count x bytes per stream written by a reset, read and written by a save or a load.  The project's protocol: every configuration
is warmed up once, then timed `rounds` times, the configurations alternating within a round; median ms between HIP events with the round-to-round spread
(max - min).  Figures are reported, none is judged."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from glava_amd import spectrum as G  # noqa: E402


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(runs, rounds):
    """runs: name -> callable; one warm-up each, then `rounds` rounds in which they alternate.  name -> (median ms, spread)"""
    for fn in runs.values(): fn()
    torch.cuda.synchronize()
    t = {name: [] for name in runs}
    for _ in range(rounds):
        for name, fn in runs.items():
            t[name].append(events(fn))
    return {name: (float(np.median(v)), max(v) - min(v)) for name, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--counts", default="1,64,4096,0", help="listed streams per call; 0: all")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "r22", "stream_slots.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("stream_slots_bench: no GPU -- nothing is measured without one")
    n, S = args.n, args.streams
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    ops = G.OP_FFT | GA | G.OP_R16
    b = G.Batch(G.Params(n=n, gl_storage=1, avg_window_kind=1), S, GA)
    pcm = torch.empty((S * n * 2,), dtype=torch.int16, device="cuda").random_(-20000, 20000)
    out = torch.zeros((S * 2, n), dtype=torch.int16, device="cuda")
    for _ in range(7): b.process_s16(pcm, out, ops)             # head != 0, every ring slot written
    torch.cuda.synchronize()
    desc = b.stream_state_desc()
    per = int(desc.bytes)
    counts = [S if int(c) == 0 else int(c) for c in args.counts.split(",")]
    blob = torch.empty((max(counts) * per,), dtype=torch.uint8, device="cuda")
    tables = {c: torch.from_numpy((np.arange(c, dtype=np.uint32) * (S // c)).view(np.int32).copy()).cuda() for c in counts}
    d = b.save_streams(tables[max(counts)], max(counts), blob)  # blobs a load may take, whatever runs first
    runs = {("process_s16", S): lambda: b.process_s16(pcm, out, ops), ("glv_batch_reset", S): b.reset}
    for c in counts:
        runs[("reset", c)] = lambda c=c: b.reset_streams(tables[c], c)
        runs[("save", c)] = lambda c=c: b.save_streams(tables[c], c, blob)
        runs[("load", c)] = lambda c=c: b.load_streams(tables[c], c, blob, d)
    ceiling = json.load(open(os.path.join(ROOT, "profiles", "stream_ceiling.json")))
    lines = [f"# stream_slots_bench: N={n} F=5 gl_storage 1 (uint16 state), {S} streams, {per} bytes per stream ({S * per / 2 ** 30:.2f} GiB of state); {torch.cuda.get_device_name(0)}",
             f"# median of {args.rounds} rounds in which the configurations alternate (spread = max - min); ms between HIP events around the one call",
             "# moved = listed streams x bytes per stream, once for a reset (written), twice for a save or a load (read + written); listed streams spread evenly over the batch",
             "# glv_batch_reset: the synchronous memsets of every array, for orientation; process_s16: one update of the whole batch (FFT | GRAVITY | AVERAGE, texels out)",
             f"# profiles/stream_ceiling.json: {json.dumps(ceiling)[:200]}",
             f"# {'call':>16} {'streams':>8} {'ms':>9} {'spread':>8} {'MiB moved':>10} {'GB/s':>8} {'% of ceiling':>12}"]
    print("\n".join(lines), flush=True)
    res = alternate(runs, args.rounds)
    for (call, c), (ms, spread) in res.items():
        moved = 0 if call == "process_s16" else c * per * (1 if "reset" in call else 2)
        rate = moved / (ms * 1e-3) / 1e9
        line = f"  {call:>16} {c:>8} {ms:>9.4f} {spread:>8.4f} {moved / 2 ** 20:>10.2f} " + (f"{rate:>8.0f} {100 * rate / ceiling['gbs']:>12.1f}" if moved else f"{'':>8} {'':>12}")
        print(line, flush=True)
        lines.append(line)
    proc = res[("process_s16", S)][0]
    for call in ("reset", "save", "load"):
        if (call, 1) in res:
            lines.append(f"# one stream, {call}: {res[(call, 1)][0] * 1e3:.1f} us = {100 * res[(call, 1)][0] / proc:.3f} % of one glv_batch_process_s16 of the batch ({proc:.3f} ms)")
    print("\n".join(lines[-3:]), flush=True)
    b.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
