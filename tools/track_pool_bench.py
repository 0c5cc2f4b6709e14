"""Track mode over a pool of recordings (glv_batch_track_pool_s16) against what a caller had before it, alternating in one process.

  (1) the pool call against glv_batch_track_each_s16 on the materialised copy, the same tables: every stream its own recording (packed by
      glava_amd.track_starts.pool_spans), window t at t * 735 of it, every rate the batch's ur, counts NULL.  The price of the span load and of the pool
      kinds' registers.  No threshold: the yardstick is the _each_ side's own spread in the same run (`inside`: the pool side is not behind by more).
  (2) `streams` listeners of ONE recording at staggered positions (listener s begins s * 1000 frames in): the pool call with the recording once in HBM
      against _each_ with one copy per listener.  Time and bytes of PCM held.
  (3) glv_batch_track_at_s16 (3a) and glv_batch_track_each_s16 (3e) in this library against the library built from the parent commit (--parent-lib, loaded
      beside this one): whether the existing entries have moved.  `inside`: |diff| <= the larger of the two round-to-round spreads.

The shipped configuration: N = 4096, the GL chain (gl_storage 1, F = 5) with the pre-smoothing pass (bars = n, bar_phase 0.5), texels out.

    python tools/track_pool_bench.py [--points 1x2048,8x2048,64x2048,1024x256] [--rounds 7] [--parts 1,2,3] [--parent-lib PATH] [--out profiles/r26/track_pool.txt]

Per point both forms are warmed up once, reset, run and compared bit for bit, then timed `rounds` times alternating with HIP events around the call (recorded
on the stream the call runs on).  Medians with the spread (max - min).  Part 3 is left out where no parent library is given; --out3 names its file."""
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
from glava_amd.track_starts import SPAN_DTYPE, pool_spans  # noqa: E402
from oracle_lib import lcg_pcm_fast  # noqa: E402
from track_at_bench import load_other  # noqa: E402

HOP, STAGGER = 735, 1000


def u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).cuda()


def dev_spans(first, frames):
    a = np.zeros((len(first),), dtype=np.dtype(SPAN_DTYPE))
    a["first"], a["frames"] = first, frames
    return torch.from_numpy(a.view(np.int32).copy()).cuda()


def timed(fn):
    """milliseconds between two HIP events around fn()"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="1x2048,8x2048,64x2048,1024x256", help="streams x steps")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parts", default="1,2,3")
    ap.add_argument("--parent-lib", default=None, help="libglvspectrum.so built from the parent commit (part 3)")
    ap.add_argument("--out", default=os.path.join("profiles", "r26", "track_pool.txt"))
    ap.add_argument("--out3", default=os.path.join("profiles", "r26", "track_pool_parent.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("track_pool_bench: no GPU -- nothing is measured without one")
    n = args.n
    parts = [q for q in args.parts.split(",") if q != "3" or args.parent_lib]
    GP = load_other(args.parent_lib) if "3" in parts else None
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    mask, ops = GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS | G.OP_R16
    kw = dict(n=n, gl_storage=1, avg_window_kind=1, log_mode=1, bars=n, bar_phase=0.5)
    p = G.Params(**kw)
    head = [f"# track_pool_bench: N={n} gl_storage=1 F={p.avg_frames} bars=n bar_phase=0.5 texels out; {torch.cuda.get_device_name(0)}",
            f"# ms = HIP events around the call, median of {args.rounds} alternating rounds (spread = max - min); outputs compared bit for bit first",
            "# 1: `other` = glv_batch_track_each_s16 on the materialised copy [streams][pitch], `new` = glv_batch_track_pool_s16 on the packed pool, the same tables",
            "#    (window t of stream s at t * 735 of its own recording); `inside`: new - other <= the _each_ side's own spread",
            "# 2: listeners of ONE recording, listener s beginning s * 1000 frames in: `other` = _each_ with a copy per listener, `new` = the pool call, the recording once",
            "# 3a / 3e: `other` = glv_batch_track_at_s16 / _each_s16 in the parent commit's library, `new` = the same entry in this library; `inside`: |diff| <= the larger spread",
            f"# {'part':>4} {'streams':>7} {'steps':>6} {'other ms':>10} {'spread':>8} {'new ms':>10} {'spread':>8} {'launches':>8} {'diff ms':>9} {'inside':>6} {'other/new':>10} {'other PCM MB':>13} {'new PCM MB':>11}"]
    print("\n".join(head), flush=True)
    lines, lines3 = list(head), list(head)
    points = [tuple(int(v) for v in pt.split("x")) for pt in args.points.split(",")]
    runs = [q for q in ("1", "2") if q in parts] + (["3a", "3e"] if "3" in parts else [])
    for part in runs:
        for S, steps in (points if part != "2" else [pt for pt in points if pt[0] >= 1024] or points[-1:]):
            reach = (steps - 1) * HOP + n                                          # frames a listener's table walks over
            if part == "2":
                lengths, listeners = [reach + (S - 1) * STAGGER], [0] * S
                starts = np.asarray([[s * STAGGER + t * HOP for t in range(steps)] for s in range(S)], dtype=np.uint32)
            else:
                lengths, listeners = [reach + 8 * s + 1 for s in range(S)], list(range(S))
                starts = np.tile(np.asarray([t * HOP for t in range(steps)], dtype=np.uint32), (S, 1))
            first, pool_frames = pool_spans(lengths)
            pool = torch.from_numpy(lcg_pcm_fast(4242 + S, pool_frames * 2).reshape(pool_frames, 2).copy()).cuda()
            pitch = max(lengths) | 1
            d_pcm = torch.zeros((S, pitch, 2), dtype=torch.int16, device="cuda")
            for s in range(S):
                r = listeners[s]
                d_pcm[s, :lengths[r]].copy_(pool[first[r]:first[r] + lengths[r]])
            d_spans = dev_spans([first[r] for r in listeners], [lengths[r] for r in listeners])
            d_starts, row0 = u32(starts), u32(starts[0])
            bn = G.Batch(p, S, mask)
            lib_o = GP if part in ("3a", "3e") else G
            bo = lib_o.Batch(lib_o.Params(**kw), S, mask)
            work = torch.empty((bn.track_at_work_bytes(steps, ops),), dtype=torch.uint8, device="cuda")
            out_o = torch.zeros((steps, S * 2, n), dtype=torch.int16, device="cuda")
            out_n = torch.zeros_like(out_o)
            if part == "3a":
                def run_o(): bo.track_at_s16(d_pcm, pitch, row0, steps, out_o, work, ops)
                def run_n(): bn.track_at_s16(d_pcm, pitch, row0, steps, out_n, work, ops)
            elif part == "3e":
                def run_o(): bo.track_each_s16(d_pcm, pitch, d_starts, None, None, steps, out_o, work, ops)
                def run_n(): bn.track_each_s16(d_pcm, pitch, d_starts, None, None, steps, out_n, work, ops)
            else:
                def run_o(): bo.track_each_s16(d_pcm, pitch, d_starts, None, None, steps, out_o, work, ops)
                def run_n(): bn.track_pool_s16(pool, pool_frames, d_spans, d_starts, None, None, steps, out_n, work, ops)
            run_o(); run_n(); l_n = bn.last_launches()
            for b in (bo, bn): b.reset()
            run_o(); run_n()
            torch.cuda.synchronize()
            if not torch.equal(out_o, out_n):
                sys.exit(f"track_pool_bench: part {part} streams={S}: the two forms' outputs differ")
            to, tn = [], []
            for _ in range(args.rounds):
                to.append(timed(run_o)); tn.append(timed(run_n))
            mo, mn = float(np.median(to)), float(np.median(tn))
            so, sn = max(to) - min(to), max(tn) - min(tn)
            inside = (mn - mo <= so) if part in ("1", "2") else (abs(mn - mo) <= max(so, sn))
            mb_o = d_pcm.numel() * 2 / 1e6
            mb_n = mb_o if part in ("3a", "3e") else pool.numel() * 2 / 1e6
            line = (f"  {part:>4} {S:>7} {steps:>6} {mo:>10.3f} {so:>8.3f} {mn:>10.3f} {sn:>8.3f} {l_n:>8} {mn - mo:>+9.3f} {'yes' if inside else 'NO':>6} {mo / mn:>10.3f}"
                    f" {mb_o:>13.1f} {mb_n:>11.1f}")
            print(line, flush=True)
            (lines3 if part in ("3a", "3e") else lines).append(line)
            bo.close(); bn.close()
            del d_pcm, pool, work, out_o, out_n
            torch.cuda.empty_cache()
    for path, text in ((args.out, lines), (args.out3, lines3)):
        if len(text) > len(head):
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
