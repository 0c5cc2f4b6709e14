"""Ring batches in track mode (glv_batch_ring_track_s16) against what a live caller had before it, alternating in one process.

  (1) `updates` updates of 256 new frames in ONE glv_batch_ring_track_s16 call against the same updates as `updates` sequential glv_batch_ring_update_s16 calls
      on a twin batch (each an append -- two strided copies where it wraps -- plus the chain's launches).  The ratio at every point, behind or ahead.
  (s) the two copies alone -- glv::launch_ring_track_stage / _keep called directly (the library's own launchers, by their C++ symbols), HIP events around the one
      launch: ms and bytes read plus written per second, beside profiles/stream_ceiling.json.
  (p) glv_batch_ring_update_s16 (pr) and glv_batch_track_at_s16 (pa) in this library against the library built from the parent commit (--parent-lib, loaded beside
      this one): whether the existing entries have moved.  `inside`: |diff| <= the parent's own round-to-round spread.

The shipped configuration: N = 4096, the GL chain (gl_storage 1, F = 5) with the pre-smoothing pass (bars = n, bar_phase 0.5), texels out, new_frames = 256.

    python tools/ring_track_bench.py [--streams 1,8,64,1024] [--updates 4,16,64] [--rounds 7] [--parts 1,s,p] [--parent-lib PATH] [--out profiles/r29/ring_track.txt]

Per point both forms are warmed up once, reset, run and compared bit for bit, then timed `rounds` times alternating with HIP events around the calls (recorded on
the stream they run on).  Medians with the spread (max - min).  Part p is left out where no parent library is given; --outp names its file."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from glava_amd import spectrum as G  # noqa: E402
from oracle_lib import lcg_pcm_fast  # noqa: E402
from track_at_bench import load_other  # noqa: E402
from track_pool_bench import timed  # noqa: E402

NF = 256


class RingTrack(C.Structure):
    """glv_launch.h RingTrack"""
    _fields_ = [("ring", C.c_void_p), ("fresh", C.c_void_p), ("stage", C.c_void_p), ("starts", C.c_void_p),
                ("n", C.c_uint32), ("pos", C.c_uint32), ("new_frames", C.c_uint32), ("updates", C.c_uint32), ("pitch", C.c_uint32), ("streams", C.c_uint32)]


def measure(runs, rounds):
    """name -> (median ms, spread) of `rounds` rounds in which the runs alternate"""
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            times[k].append(timed(fn))
    return {k: (float(np.median(v)), max(v) - min(v)) for k, v in times.items()}


def part_1(args, p, mask, ops, lines):
    n = p.n
    for S in args.streams:
        for U in args.updates:
            new = torch.from_numpy(lcg_pcm_fast(777 + S + U, S * U * NF * 2).reshape(S, U * NF, 2).copy()).cuda()
            chunks = [new[:, t * NF:(t + 1) * NF].contiguous() for t in range(U)]
            bt, bs = G.Batch(p, S, mask | G.OP_RING_S16), G.Batch(p, S, mask | G.OP_RING_S16)
            work = torch.empty((bt.ring_track_work_bytes(NF, U, ops),), dtype=torch.uint8, device="cuda")
            out_t = torch.zeros((U, S * 2, n), dtype=torch.int16, device="cuda")
            out_s = torch.zeros_like(out_t)

            def run_t(): bt.ring_track_s16(new, NF, U, out_t, work, ops)

            def run_s():
                for t in range(U):
                    bs.ring_update_s16(chunks[t], NF, out_s[t], ops)
            run_t(); run_s(); l_t = bt.last_launches()
            for b in (bt, bs): b.reset()
            run_t(); run_s()
            torch.cuda.synchronize()
            if not torch.equal(out_t, out_s):
                sys.exit(f"ring_track_bench: streams={S} updates={U}: the two forms' outputs differ")
            m = measure({"seq": run_s, "new": run_t}, args.rounds)
            (ms, ss), (mt, st) = m["seq"], m["new"]
            line = f"  {'1':>4} {S:>7} {U:>7} {ms:>10.3f} {ss:>8.3f} {mt:>10.3f} {st:>8.3f} {l_t:>8} {ms / mt:>10.2f} {work.numel() / 1e6:>10.1f}"
            print(line, flush=True); lines.append(line)
            bt.close(); bs.close()
            del new, chunks, work, out_t, out_s
            torch.cuda.empty_cache()


def part_s(args, p, lines):
    L = C.CDLL(G.LIB_PATH)
    stage = getattr(L, "_ZN3glv23launch_ring_track_stageEbRKNS_9RingTrackEP12ihipStream_t")
    keep = getattr(L, "_ZN3glv22launch_ring_track_keepEbRKNS_9RingTrackEP12ihipStream_t")
    for fn in (stage, keep): fn.argtypes = [C.c_bool, C.POINTER(RingTrack), C.c_void_p]
    n = p.n
    for S in args.streams:
        for U in args.updates:
            pitch = (n + U * NF + 3) & ~3
            ring = torch.from_numpy(lcg_pcm_fast(5 + S, S * n * 2).reshape(S, n, 2).copy()).cuda()
            new = torch.from_numpy(lcg_pcm_fast(6 + S + U, S * U * NF * 2).reshape(S, U * NF, 2).copy()).cuda()
            staged = torch.zeros((S, pitch, 2), dtype=torch.int16, device="cuda")
            starts = torch.zeros((U,), dtype=torch.int32, device="cuda")
            r = RingTrack(ring.data_ptr(), new.data_ptr(), staged.data_ptr(), starts.data_ptr(), n, 111, NF, U, pitch, S)

            def call(fn):
                def run():
                    if fn(False, C.byref(r), None) != 0: sys.exit("ring_track_bench: a copy launch failed")
                return run
            m = measure({"stage": call(stage), "keep": call(keep)}, args.rounds)
            moved = {"stage": S * ((n + U * NF) + pitch) * 4 + 4 * U, "keep": 2 * S * n * 4}
            for k in ("stage", "keep"):
                ms, sp = m[k]
                line = f"  {'s':>4} {S:>7} {U:>7} {k:>10} {ms:>10.4f} {sp:>8.4f} {moved[k] / 1e6:>10.2f} {moved[k] / (ms * 1e-3) / 1e12:>8.3f}"
                print(line, flush=True); lines.append(line)
            del ring, new, staged, starts
            torch.cuda.empty_cache()


def part_p(args, kw, mask, ops, GP, lines):
    n = kw["n"]
    for part in ("pr", "pa"):
        for S in args.streams:
            U = 16
            bo, bn = GP.Batch(GP.Params(**kw), S, mask | GP.OP_RING_S16), G.Batch(G.Params(**kw), S, mask | G.OP_RING_S16)
            out_o = torch.zeros((U, S * 2, n), dtype=torch.int16, device="cuda")
            out_n = torch.zeros_like(out_o)
            if part == "pr":
                new = torch.from_numpy(lcg_pcm_fast(31 + S, S * NF * 2).reshape(S, NF, 2).copy()).cuda()

                def run_o(): bo.ring_update_s16(new, NF, out_o[0], ops)
                def run_n(): bn.ring_update_s16(new, NF, out_n[0], ops)
            else:
                pitch = n + U * NF
                pcm = torch.from_numpy(lcg_pcm_fast(32 + S, S * pitch * 2).reshape(S, pitch, 2).copy()).cuda()
                d_starts = torch.from_numpy(np.asarray([(t + 1) * NF for t in range(U)], dtype=np.int32)).cuda()
                work = torch.empty((bn.track_at_work_bytes(U, ops),), dtype=torch.uint8, device="cuda")

                def run_o(): bo.track_at_s16(pcm, pitch, d_starts, U, out_o, work, ops)
                def run_n(): bn.track_at_s16(pcm, pitch, d_starts, U, out_n, work, ops)
            run_o(); run_n()
            for b in (bo, bn): b.reset()
            run_o(); run_n()
            torch.cuda.synchronize()
            if not torch.equal(out_o, out_n):
                sys.exit(f"ring_track_bench: part {part} streams={S}: the two libraries' outputs differ")
            m = measure({"other": run_o, "new": run_n}, args.rounds)
            (mo, so), (mn, sn) = m["other"], m["new"]
            line = f"  {part:>4} {S:>7} {(1 if part == 'pr' else U):>7} {mo:>10.4f} {so:>8.4f} {mn:>10.4f} {sn:>8.4f} {mn - mo:>+9.4f} {'yes' if abs(mn - mo) <= so else 'NO':>6} {mo / mn:>10.3f}"
            print(line, flush=True); lines.append(line)
            bo.close(); bn.close()
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,8,64,1024")
    ap.add_argument("--updates", default="4,16,64")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parts", default="1,s,p")
    ap.add_argument("--parent-lib", default=None, help="libglvspectrum.so built from the parent commit (part p)")
    ap.add_argument("--out", default=os.path.join("profiles", "r29", "ring_track.txt"))
    ap.add_argument("--outp", default=os.path.join("profiles", "r29", "ring_track_parent.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ring_track_bench: no GPU -- nothing is measured without one")
    args.streams = [int(v) for v in args.streams.split(",")]
    args.updates = [int(v) for v in args.updates.split(",")]
    parts = [q for q in args.parts.split(",") if q != "p" or args.parent_lib]
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    mask, ops = GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS | G.OP_R16
    kw = dict(n=args.n, gl_storage=1, avg_window_kind=1, log_mode=1, bars=args.n, bar_phase=0.5)
    p = G.Params(**kw)
    ceiling = json.load(open(os.path.join(ROOT, "profiles", "stream_ceiling.json")))
    head = [f"# ring_track_bench: N={args.n} gl_storage=1 F={p.avg_frames} bars=n bar_phase=0.5 texels out, new_frames={NF}; {torch.cuda.get_device_name(0)}",
            f"# ms = HIP events around the calls, median of {args.rounds} alternating rounds (spread = max - min); outputs compared bit for bit first",
            f"# profiles/stream_ceiling.json: {json.dumps(ceiling)[:200]}"]
    lines, linesp = list(head), list(head)
    print("\n".join(head), flush=True)
    if "1" in parts:
        lines += ["# 1: `seq` = `updates` glv_batch_ring_update_s16 calls on a twin batch, `new` = one glv_batch_ring_track_s16 call; work MB = the call's workspace",
                  f"# {'part':>4} {'streams':>7} {'updates':>7} {'seq ms':>10} {'spread':>8} {'new ms':>10} {'spread':>8} {'launches':>8} {'seq/new':>10} {'work MB':>10}"]
        print("\n".join(lines[-2:]), flush=True)
        part_1(args, p, mask, ops, lines)
    if "s" in parts:
        lines += ["# s: the copies alone, s16 frames, the ring at frame 111: stage = glv_ring_stage_kernel (reads n + updates * 256 frames a stream, writes the pitch and the table),",
                  "#    keep = glv_ring_keep_kernel (reads and writes n frames a stream); moved = bytes read + written",
                  f"# {'part':>4} {'streams':>7} {'updates':>7} {'copy':>10} {'ms':>10} {'spread':>8} {'moved MB':>10} {'TB/s':>8}"]
        print("\n".join(lines[-3:]), flush=True)
        part_s(args, p, lines)
    if "p" in parts:
        linesp += ["# pr: glv_batch_ring_update_s16 (one update of 256 frames); pa: glv_batch_track_at_s16 (16 steps, starts (t + 1) * 256): `other` = the parent commit's library,",
                   "#     `new` = this one, loaded side by side; `inside`: |new - other| <= the parent's spread",
                   f"# {'part':>4} {'streams':>7} {'steps':>7} {'other ms':>10} {'spread':>8} {'new ms':>10} {'spread':>8} {'diff ms':>9} {'inside':>6} {'other/new':>10}"]
        print("\n".join(linesp[-3:]), flush=True)
        part_p(args, kw, mask, ops, load_other(args.parent_lib), linesp)
    for path, text in ((args.out, lines), (args.outp, linesp)):
        if len(text) > len(head):
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
