"""Ring batches in track mode per stream (glv_batch_ring_track_each_s16) against the lockstep entry, against one-stream batches, and the existing entries
against the parent commit's library, alternating in one process.

  (1) equal counts, both tables NULL: glv_batch_ring_track_each_s16 against glv_batch_ring_track_s16 on a twin batch.  The expectation: inside that entry's spread.
  (2) mixed counts -- a quarter of the streams at 0, a quarter at half the updates, the rest full -- with a row of live_session_rates (22050 Hz, 60 fps) per
      stream, in ONE call against the same work as one-stream ring batches one after another (DESIGN 4.19's comparison): a call of the same entry per stream
      with a count above 0, `updates` = its count, its own rate row.  The ratio at every point.
  (s) the two copies alone -- glv::launch_ring_each_stage / _keep called directly (the library's own launchers, by their C++ symbols) with the mixed counts,
      HIP events around the one launch: ms and bytes read plus written per second.
  (p) glv_batch_ring_track_s16 (pt), glv_batch_ring_update_s16 (pr) and glv_batch_track_each_s16 (pe) in this library against the library built from the
      parent commit (--parent-lib, loaded beside this one): whether the existing entries have moved.  `inside`: |diff| <= the parent's own spread.

The shipped configuration: N = 4096, the GL chain (gl_storage 1, F = 5) with the pre-smoothing pass (bars = n, bar_phase 0.5), texels out, new_frames = 256.

    python tools/ring_track_each_bench.py [--streams 1,8,64,1024] [--updates 4,16,64] [--rounds 7] [--parts 1,2,s,p] [--parent-lib PATH]
                                          [--out profiles/r30/ring_track_each.txt] [--outp profiles/r30/ring_track_each_parent.txt]

Per point both forms are warmed up once, reset, run and compared bit for bit, then timed `rounds` times alternating with HIP events around the calls.
Medians with the spread (max - min).  Part p is left out where no parent library is given."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from glava_amd import spectrum as G  # noqa: E402
from glava_amd.track_starts import live_session_rates  # noqa: E402
from oracle_lib import lcg_pcm_fast  # noqa: E402
from ring_track_bench import NF, RingTrack, measure  # noqa: E402
from track_at_bench import load_other  # noqa: E402


class RingTrackEach(C.Structure):
    """glv_launch.h RingTrackEach"""
    _fields_ = [("r", RingTrack), ("counts", C.c_void_p)]


def pcm(seed, S, frames):
    return torch.from_numpy(lcg_pcm_fast(seed, S * frames * 2).reshape(S, frames, 2).copy()).cuda()


def mixed_counts(S, U):
    """a quarter of the streams at 0, a quarter at half, the rest full (one stream: full)"""
    return np.asarray([U if S == 1 else (0, U // 2, U, U)[s % 4] for s in range(S)], dtype=np.uint32)


def rate_rows(S, U):
    """a row of live_session_rates per stream: the session's rates from another render frame on for every stream (1.0, then 59.0, then 60.0)"""
    ur = live_session_rates(22050, 60, 400, NF)[2]
    return np.asarray([[ur[(37 * s + t) % len(ur)] for t in range(U)] for s in range(S)], dtype=np.float32)


def part_1(args, p, mask, ops, lines):
    n = p.n
    for S in args.streams:
        for U in args.updates:
            new = pcm(777 + S + U, S, U * NF)
            be, bl = G.Batch(p, S, mask | G.OP_RING_S16), G.Batch(p, S, mask | G.OP_RING_S16)
            work_e = torch.empty((be.ring_track_each_work_bytes(NF, U, ops),), dtype=torch.uint8, device="cuda")
            work_l = torch.empty((bl.ring_track_work_bytes(NF, U, ops),), dtype=torch.uint8, device="cuda")
            out_e = torch.zeros((U, S * 2, n), dtype=torch.int16, device="cuda")
            out_l = torch.zeros_like(out_e)

            def run_e(): be.ring_track_each_s16(new, NF, U, None, None, out_e, work_e, ops)
            def run_l(): bl.ring_track_s16(new, NF, U, out_l, work_l, ops)
            run_e(); run_l(); launches = be.last_launches()
            for b in (be, bl): b.reset()
            run_e(); run_l()
            torch.cuda.synchronize()
            if not torch.equal(out_e, out_l):
                sys.exit(f"ring_track_each_bench: part 1 streams={S} updates={U}: the two entries' outputs differ")
            m = measure({"lock": run_l, "each": run_e}, args.rounds)
            (ml, sl), (me, se) = m["lock"], m["each"]
            line = f"  {'1':>4} {S:>7} {U:>7} {ml:>10.4f} {sl:>8.4f} {me:>10.4f} {se:>8.4f} {launches:>8} {me - ml:>+9.4f} {'yes' if abs(me - ml) <= sl else 'NO':>6} {ml / me:>10.3f}"
            print(line, flush=True); lines.append(line)
            be.close(); bl.close()
            del new, work_e, work_l, out_e, out_l
            torch.cuda.empty_cache()


def part_2(args, p, mask, ops, lines):
    n = p.n
    for S in args.streams:
        for U in args.updates:
            counts, urs = mixed_counts(S, U), rate_rows(S, U)
            new = pcm(778 + S + U, S, U * NF)
            d_counts, d_ur = torch.from_numpy(counts.view(np.int32)).cuda(), torch.from_numpy(urs).cuda()
            bb = G.Batch(p, S, mask | G.OP_RING_S16)
            work = torch.empty((bb.ring_track_each_work_bytes(NF, U, ops),), dtype=torch.uint8, device="cuda")
            out_b = torch.zeros((U, S * 2, n), dtype=torch.int16, device="cuda")
            ones = []                                                              # (batch, its new frames, its rate row, its output, its count)
            one_work = torch.empty((bb.ring_track_each_work_bytes(NF, U, ops) // S + (1 << 20),), dtype=torch.uint8, device="cuda")
            for s in range(S):
                c = int(counts[s])
                if c == 0: continue
                b1 = G.Batch(p, 1, mask | G.OP_RING_S16)
                assert b1.ring_track_each_work_bytes(NF, c, ops) <= one_work.numel()
                ones.append((b1, new[s:s + 1, :c * NF].contiguous(), torch.from_numpy(urs[s:s + 1, :c].copy()).cuda(), torch.zeros((c, 2, n), dtype=torch.int16, device="cuda"), c, s))

            def run_b(): bb.ring_track_each_s16(new, NF, U, d_ur, d_counts, out_b, work, ops)

            def run_1():
                for b1, x, ur, o, c, _ in ones:
                    b1.ring_track_each_s16(x, NF, c, ur, None, o, one_work, ops)
            run_b(); run_1()
            for b in [bb] + [t[0] for t in ones]: b.reset()
            run_b(); run_1()
            torch.cuda.synchronize()
            for b1, x, ur, o, c, s in ones:
                if not torch.equal(out_b[:c, 2 * s:2 * s + 2], o):
                    sys.exit(f"ring_track_each_bench: part 2 streams={S} updates={U}: stream {s} differs from its one-stream batch")
            m = measure({"ones": run_1, "one": run_b}, args.rounds)
            (m1, s1), (mb, sb) = m["ones"], m["one"]
            line = f"  {'2':>4} {S:>7} {U:>7} {int(counts.sum()):>8} {len(ones):>6} {m1:>10.3f} {s1:>8.3f} {mb:>10.3f} {sb:>8.3f} {m1 / mb:>10.2f}"
            print(line, flush=True); lines.append(line)
            for t in ones: t[0].close()
            bb.close()
            del new, work, out_b, ones, one_work
            torch.cuda.empty_cache()


def part_s(args, p, lines):
    L = C.CDLL(G.LIB_PATH)
    stage = getattr(L, "_ZN3glv22launch_ring_each_stageEbRKNS_13RingTrackEachEP12ihipStream_t")
    keep = getattr(L, "_ZN3glv21launch_ring_each_keepEbRKNS_13RingTrackEachEP12ihipStream_t")
    for fn in (stage, keep): fn.argtypes = [C.c_bool, C.POINTER(RingTrackEach), C.c_void_p]
    n = p.n
    for S in args.streams:
        for U in args.updates:
            pitch = (n + U * NF + 3) & ~3
            counts = mixed_counts(S, U)
            ring, new = pcm(5 + S, S, n), pcm(6 + S + U, S, U * NF)
            staged = torch.zeros((S, pitch, 2), dtype=torch.int16, device="cuda")
            starts = torch.zeros((S, U), dtype=torch.int32, device="cuda")
            d_counts = torch.from_numpy(counts.view(np.int32)).cuda()
            e = RingTrackEach(RingTrack(ring.data_ptr(), new.data_ptr(), staged.data_ptr(), starts.data_ptr(), n, 111, NF, U, pitch, S), d_counts.data_ptr())

            def call(fn):
                def run():
                    if fn(False, C.byref(e), None) != 0: sys.exit("ring_track_each_bench: a copy launch failed")
                return run
            m = measure({"stage": call(stage), "keep": call(keep)}, args.rounds)
            own = int(counts.sum()) * NF
            moved = {"stage": (S * n + own + S * pitch) * 4 + 4 * S * U + 4 * S, "keep": 2 * S * n * 4 + 4 * S}
            for k in ("stage", "keep"):
                ms, sp = m[k]
                line = f"  {'s':>4} {S:>7} {U:>7} {k:>10} {ms:>10.4f} {sp:>8.4f} {moved[k] / 1e6:>10.2f} {moved[k] / (ms * 1e-3) / 1e12:>8.3f}"
                print(line, flush=True); lines.append(line)
            del ring, new, staged, starts, d_counts
            torch.cuda.empty_cache()


def part_p(args, kw, mask, ops, GP, lines):
    n, U = kw["n"], 16
    for part in ("pt", "pr", "pe"):
        for S in args.streams:
            bo, bn = GP.Batch(GP.Params(**kw), S, mask | GP.OP_RING_S16), G.Batch(G.Params(**kw), S, mask | G.OP_RING_S16)
            out_o = torch.zeros((U, S * 2, n), dtype=torch.int16, device="cuda")
            out_n = torch.zeros_like(out_o)
            if part == "pt":
                new = pcm(30 + S, S, U * NF)
                work = torch.empty((bn.ring_track_work_bytes(NF, U, ops),), dtype=torch.uint8, device="cuda")

                def run_o(): bo.ring_track_s16(new, NF, U, out_o, work, ops)
                def run_n(): bn.ring_track_s16(new, NF, U, out_n, work, ops)
            elif part == "pr":
                new = pcm(31 + S, S, NF)

                def run_o(): bo.ring_update_s16(new, NF, out_o[0], ops)
                def run_n(): bn.ring_update_s16(new, NF, out_n[0], ops)
            else:
                pitch = n + U * NF
                rec = pcm(32 + S, S, pitch)
                d_starts = torch.from_numpy(np.tile(np.arange(1, U + 1, dtype=np.int32) * NF, (S, 1))).cuda()
                d_ur = torch.from_numpy(rate_rows(S, U)).cuda()
                d_counts = torch.from_numpy(mixed_counts(S, U).view(np.int32)).cuda()
                work = torch.empty((bn.track_at_work_bytes(U, ops),), dtype=torch.uint8, device="cuda")

                def run_o(): bo.track_each_s16(rec, pitch, d_starts, d_ur, d_counts, U, out_o, work, ops)
                def run_n(): bn.track_each_s16(rec, pitch, d_starts, d_ur, d_counts, U, out_n, work, ops)
            run_o(); run_n()
            for b in (bo, bn): b.reset()
            run_o(); run_n()
            torch.cuda.synchronize()
            if not torch.equal(out_o, out_n):
                sys.exit(f"ring_track_each_bench: part {part} streams={S}: the two libraries' outputs differ")
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
    ap.add_argument("--parts", default="1,2,s,p")
    ap.add_argument("--parent-lib", default=None, help="libglvspectrum.so built from the parent commit (part p)")
    ap.add_argument("--out", default=os.path.join("profiles", "r30", "ring_track_each.txt"))
    ap.add_argument("--outp", default=os.path.join("profiles", "r30", "ring_track_each_parent.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ring_track_each_bench: no GPU -- nothing is measured without one")
    args.streams = [int(v) for v in args.streams.split(",")]
    args.updates = [int(v) for v in args.updates.split(",")]
    parts = [q for q in args.parts.split(",") if q != "p" or args.parent_lib]
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    mask, ops = GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS | G.OP_R16
    kw = dict(n=args.n, gl_storage=1, avg_window_kind=1, log_mode=1, bars=args.n, bar_phase=0.5)
    p = G.Params(**kw)
    head = [f"# ring_track_each_bench: N={args.n} gl_storage=1 F={p.avg_frames} bars=n bar_phase=0.5 texels out, new_frames={NF}; {torch.cuda.get_device_name(0)}",
            f"# ms = HIP events around the calls, median of {args.rounds} alternating rounds (spread = max - min); outputs compared bit for bit first"]
    lines, linesp = list(head), list(head)
    print("\n".join(head), flush=True)
    if "1" in parts:
        lines += ["# 1: every stream takes all updates, d_counts and d_ur NULL: `lock` = glv_batch_ring_track_s16 on a twin batch, `each` = glv_batch_ring_track_each_s16;",
                  "#    `inside`: |each - lock| <= the lockstep entry's spread",
                  f"# {'part':>4} {'streams':>7} {'updates':>7} {'lock ms':>10} {'spread':>8} {'each ms':>10} {'spread':>8} {'launches':>8} {'diff ms':>9} {'inside':>6} {'lock/each':>10}"]
        print("\n".join(lines[-3:]), flush=True)
        part_1(args, p, mask, ops, lines)
    if "2" in parts:
        lines += ["# 2: counts 0 / updates / 2 / updates / updates by stream mod 4 (one stream: all), a row of live_session_rates(22050, 60) per stream: `ones` = a call of the",
                  "#    same entry per stream with a count above 0 on a one-stream ring batch, one after another; `one` = ONE call on the batch; taken = the sum of the counts",
                  f"# {'part':>4} {'streams':>7} {'updates':>7} {'taken':>8} {'calls':>6} {'ones ms':>10} {'spread':>8} {'one ms':>10} {'spread':>8} {'ones/one':>10}"]
        print("\n".join(lines[-3:]), flush=True)
        part_2(args, p, mask, ops, lines)
    if "s" in parts:
        lines += ["# s: the copies alone with part 2's counts, s16 frames, the ring at frame 111: stage = glv_ring_stage_each_kernel (reads n + c_s * 256 frames a stream and its",
                  "#    count, writes the pitch and streams * updates starts), keep = glv_ring_keep_each_kernel (reads and writes n frames a stream); moved = bytes read + written",
                  f"# {'part':>4} {'streams':>7} {'updates':>7} {'copy':>10} {'ms':>10} {'spread':>8} {'moved MB':>10} {'TB/s':>8}"]
        print("\n".join(lines[-3:]), flush=True)
        part_s(args, p, lines)
    if "p" in parts:
        linesp += ["# pt: glv_batch_ring_track_s16 (16 updates of 256 frames); pr: glv_batch_ring_update_s16 (one update); pe: glv_batch_track_each_s16 (16 steps, part 2's counts and rates):",
                   "#     `other` = the parent commit's library, `new` = this one, loaded side by side; `inside`: |new - other| <= the parent's spread",
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
