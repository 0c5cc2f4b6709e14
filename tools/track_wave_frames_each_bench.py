"""Track mode at render frames per stream for the wave module (glv_batch_track_each_wave_frames_s16 / glv_batch_track_pool_wave_frames_s16) against what a
caller had before it, alternating in one process.

  (a) equal rows for all streams, NULL counts, equal keep pairs: glv_batch_track_each_wave_frames_s16 against glv_batch_track_wave_frames_s16 on the same tables --
      what the per-stream kernels cost where the lockstep call would have done.  "Level" means inside the lockstep call's own round-to-round spread
  (b) listeners at mixed display rates: stream s runs the session of glava_amd.track_starts.live_session_frames(22050, fps, ..., 256) at fps = 60 / 75 / 120 /
      144 in turn over the same stretch of time, and every fourth stream stands still (count 0, its last keyframe shown on every frame: from == to == 1).  One
      call, against the same work as one-stream glv_batch_track_wave_frames_s16 calls one after another on one one-stream batch (the streams that stand still are
      skipped on that side: the lockstep call refuses steps == 0)
  (c) `streams` listeners of ONE pooled recording (b's listeners, every span the whole pool): glv_batch_track_pool_wave_frames_s16 against
      glv_batch_track_each_wave_frames_s16 on the materialised copy, a recording per stream
  (d) glv_batch_track_wave_frames_s16 (d1: a's tables) and glv_batch_track_each_frames_s16 (d2: gl_storage 3, F = 5, FFT | GRAVITY | AVERAGE | BARS | R16, equal
      rows) in this library against the library built from the parent commit (--parent-lib, loaded beside this one): whether the existing entries have moved.
      "Level" means inside the parent's spread.  Written to --compare-out

The configuration of (a) - (c): N = 4096, gl_storage 1, the pre-smoothing pass (bars = n, bar_phase 0.5), GLV_OP_WAVE | GLV_OP_BARS | GLV_OP_R16: texels out --
the protocol of tools/track_wave_frames_bench.py and tools/track_frames_each_bench.py.

    python tools/track_wave_frames_each_bench.py [--points 1x2048,8x2048,64x2048,1024x256] [--rounds 7] [--parts a,b,c,d] [--parent-lib PATH]
                                                 [--out profiles/r28/track_wave_frames_each.txt] [--compare-out profiles/r28/bench_compare.txt]

Per point the outputs of both sides are compared bit for bit first (b: every stream up to 64 streams, eight streams spread over the batch beyond), then both
are warmed up once and timed `rounds` times alternating, a host clock around the calls and the device synchronise that ends them.  Prints and writes the tables:
median ms of each side with the round-to-round spread (max - min).  Part d is left out where no parent library is given.
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
from glava_amd.track_starts import SPAN_DTYPE, stack_frame_tables, stack_tables  # noqa: E402
from oracle_lib import lcg_pcm_fast  # noqa: E402
from track_at_bench import load_other, timed  # noqa: E402
from track_frames_bench import dev, session  # noqa: E402
from track_frames_each_bench import listeners  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="1x2048,8x2048,64x2048,1024x256", help="streams x steps")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parts", default="a,b,c,d")
    ap.add_argument("--parent-lib", default=None, help="libglvspectrum.so built from the parent commit (part d)")
    ap.add_argument("--out", default=os.path.join("profiles", "r28", "track_wave_frames_each.txt"))
    ap.add_argument("--compare-out", default=os.path.join("profiles", "r28", "bench_compare.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("track_wave_frames_each_bench: no GPU -- nothing is measured without one")
    n = args.n
    parts = [q for q in args.parts.split(",") if q != "d" or args.parent_lib]
    GP = load_other(args.parent_lib) if "d" in parts else None
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    wave_kw, wave_mask, wave_ops = dict(n=n, gl_storage=1, bars=n, bar_phase=0.5), G.OP_WAVE | G.OP_BARS, G.OP_WAVE | G.OP_BARS | G.OP_R16
    fft_kw, fft_mask, fft_ops = dict(n=n, gl_storage=G.GL_STORAGE_UPLOAD, bars=n, bar_phase=0.5), GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS | G.OP_R16
    column = (f"# {'part':>4} {'streams':>7} {'steps':>6} {'frames':>6} {'other ms':>10} {'spread':>8} {'launches':>8} {'new ms':>10} {'spread':>8} {'launches':>8} "
              f"{'other/new':>9} {'level':>6}")
    head = [f"# track_wave_frames_each_bench: N={n} bars=n bar_phase=0.5 (the pre-smoothing pass) texels out; {torch.cuda.get_device_name(0)}",
            f"# median of {args.rounds} alternating rounds (spread = max - min), ms of a host clock around the calls and the synchronise that ends them; outputs compared bit for bit first"]
    lines = head + [
        "# gl_storage 1, GLV_OP_WAVE | GLV_OP_BARS | GLV_OP_R16",
        "# a: `other` = glv_batch_track_wave_frames_s16, `new` = glv_batch_track_each_wave_frames_s16 with the same row of every table for all streams, NULL counts, equal",
        "#    keep pairs; the tables of live_session_frames(22050, 144, ..., 256).  level: |new - other| <= the lockstep call's spread",
        "# b: `other` = one glv_batch_track_wave_frames_s16 call per moving stream on ONE one-stream batch, one after another, `new` = one",
        "#    glv_batch_track_each_wave_frames_s16 call; stream s at 60 / 75 / 120 / 144 fps in turn over the same stretch of time, every fourth standing still (count 0;",
        "#    skipped on the other side)",
        "# c: `other` = glv_batch_track_each_wave_frames_s16 on the materialised copy (a recording per stream), `new` = glv_batch_track_pool_wave_frames_s16 with every",
        "#    stream's span the whole of ONE recording; b's listeners.  level: |new - other| <= the larger spread",
        column]
    compare = head + [
        "# `other` = the parent commit's library, `new` = this one, loaded side by side.  level (not moved): |new - other| <= the parent's spread",
        "# d1: glv_batch_track_wave_frames_s16, gl_storage 1, GLV_OP_WAVE | GLV_OP_BARS | GLV_OP_R16, the tables of live_session_frames(22050, 144, ..., 256)",
        "# d2: glv_batch_track_each_frames_s16, gl_storage 3, F = 5, FFT | GRAVITY | AVERAGE | BARS | R16, the same row of every table for all streams",
        column]
    print("\n".join(lines), flush=True)
    points = [tuple(int(v) for v in pt.split("x")) for pt in args.points.split(",")]
    expanded = [q for part in parts for q in (("d1", "d2") if part == "d" else (part,))]
    for part in expanded:
        for S, steps in points:
            starts, urs, frm, to, mod, kf, kt = session(steps)
            frames = len(frm)
            if part in ("b", "c"):
                each = listeners(S, steps)
                t_starts, _, t_counts = stack_tables([(t[0], None) for t in each], steps)
                f_from, f_to, f_mod, f_counts, f_keep = stack_frame_tables([t[2:] for t in each])
                frames = f_from.shape[1]
            else:
                t_starts, t_counts = np.tile(np.asarray(starts, dtype=np.uint32), (S, 1)), None
                f_from, f_to, f_mod = (np.tile(np.asarray(v, dtype=dt), (S, 1)) for v, dt in ((frm, np.uint32), (to, np.uint32), (mod, np.float32)))
                f_counts, f_keep = None, np.tile(np.asarray((kf, kt), dtype=np.uint32), (S, 1))
            pitch = (int(t_starts.max()) + n + 1) | 1                           # odd
            recordings = 1 if part == "c" else S
            x = lcg_pcm_fast(4242 + S, recordings * pitch * 2).reshape(recordings, pitch, 2).copy()
            x[:, :n, :] = 0                                                      # GLava's zeroed buffers in front of the audio's first frame
            d_pcm = torch.from_numpy(x).cuda()
            d_tab = (dev(t_starts, np.uint32), None, dev(t_counts, np.uint32) if t_counts is not None else None)
            d_fr = (dev(f_from, np.uint32), dev(f_to, np.uint32), dev(f_mod, np.float32), dev(f_counts, np.uint32) if f_counts is not None else None, dev(f_keep, np.uint32))
            d_starts, d_ur, d_from, d_to, d_mod = dev(starts, np.uint32), dev(urs, np.float32), dev(frm, np.uint32), dev(to, np.uint32), dev(mod, np.float32)
            keys_n = torch.zeros((2, S * 2, n), dtype=torch.float32, device="cuda")
            keys_o = torch.zeros_like(keys_n)
            if part == "d2":
                bo, bn = GP.Batch(GP.Params(**fft_kw), S, fft_mask), G.Batch(G.Params(**fft_kw), S, fft_mask)
                d_tab = (d_tab[0], dev(np.tile(np.asarray(urs, dtype=np.float32), (S, 1)), np.float32), None)
                wb = bn.track_frames_work_bytes(steps, frames, fft_ops)
                work_n, work_o = (torch.empty((wb,), dtype=torch.uint8, device="cuda") for _ in range(2))
                out_n, out_o = (torch.zeros((frames, S * 2, n), dtype=torch.int16, device="cuda") for _ in range(2))

                def run_o(): bo.track_each_frames_s16(d_pcm, pitch, d_tab, steps, d_fr, frames, keys_o, out_o, work_o, fft_ops)
                def run_n(): bn.track_each_frames_s16(d_pcm, pitch, d_tab, steps, d_fr, frames, keys_n, out_n, work_n, fft_ops)
                same = lambda: torch.equal(out_o, out_n) and torch.equal(keys_o, keys_n)      # noqa: E731
            elif part in ("a", "d1"):
                GO = GP if part == "d1" else G
                bo, bn = GO.Batch(GO.Params(**wave_kw), S, wave_mask), G.Batch(G.Params(**wave_kw), S, wave_mask)
                wb = bn.track_wave_frames_work_bytes(steps, frames, wave_ops)
                work_n, work_o = (torch.empty((wb,), dtype=torch.uint8, device="cuda") for _ in range(2))
                out_n, out_o = (torch.zeros((frames, S * 2, n), dtype=torch.int16, device="cuda") for _ in range(2))

                def run_o(): bo.track_wave_frames_s16(d_pcm, pitch, d_starts, steps, d_from, d_to, d_mod, frames, keys_o, (kf, kt), out_o, work_o, wave_ops)
                if part == "a":
                    def run_n(): bn.track_each_wave_frames_s16(d_pcm, pitch, d_tab, steps, d_fr, frames, keys_n, out_n, work_n, wave_ops)
                else:
                    def run_n(): bn.track_wave_frames_s16(d_pcm, pitch, d_starts, steps, d_from, d_to, d_mod, frames, keys_n, (kf, kt), out_n, work_n, wave_ops)
                same = lambda: torch.equal(out_o, out_n) and torch.equal(keys_o, keys_n)      # noqa: E731
            elif part == "c":
                bo, bn = G.Batch(G.Params(**wave_kw), S, wave_mask), G.Batch(G.Params(**wave_kw), S, wave_mask)
                spans = np.zeros((S,), dtype=np.dtype(SPAN_DTYPE))
                spans["first"], spans["frames"] = 0, pitch
                d_spans = torch.from_numpy(spans.view(np.int32).copy()).cuda()
                d_copy = d_pcm.expand(S, pitch, 2).contiguous()                  # the materialised copy: every listener its own recording
                wb = bn.track_wave_frames_work_bytes(steps, frames, wave_ops)
                work_n, work_o = (torch.empty((wb,), dtype=torch.uint8, device="cuda") for _ in range(2))
                out_n, out_o = (torch.zeros((frames, S * 2, n), dtype=torch.int16, device="cuda") for _ in range(2))

                def run_o(): bo.track_each_wave_frames_s16(d_copy, pitch, d_tab, steps, d_fr, frames, keys_o, out_o, work_o, wave_ops)
                def run_n(): bn.track_pool_wave_frames_s16(d_pcm, pitch, d_spans, d_tab, steps, d_fr, frames, keys_n, out_n, work_n, wave_ops)
                same = lambda: torch.equal(out_o, out_n) and torch.equal(keys_o, keys_n)      # noqa: E731
            else:
                bo, bn = G.Batch(G.Params(**wave_kw), 1, wave_mask), G.Batch(G.Params(**wave_kw), S, wave_mask)
                moving = [s for s in range(S) if len(each[s][0]) > 0]
                longest = max(len(each[s][2]) for s in moving)
                one = []                                                         # per moving stream: its own tables on the device, made once
                for s in moving:
                    t = each[s]
                    one.append((s, len(t[0]), len(t[2]), dev(t[0], np.uint32), dev(t[2], np.uint32), dev(t[3], np.uint32), dev(t[4], np.float32), (t[5], t[6])))
                keys_o = torch.zeros((2, 2, n), dtype=torch.float32, device="cuda")
                wb = bn.track_wave_frames_work_bytes(steps, frames, wave_ops)
                work_n = torch.empty((wb,), dtype=torch.uint8, device="cuda")
                work_o = torch.empty((bo.track_wave_frames_work_bytes(steps, longest, wave_ops),), dtype=torch.uint8, device="cuda")
                out_n = torch.zeros((frames, S * 2, n), dtype=torch.int16, device="cuda")
                out_o = torch.zeros((longest, 2, n), dtype=torch.int16, device="cuda")

                def run_o():
                    for s, c, f, a_starts, a_from, a_to, a_mod, keep in one:
                        bo.track_wave_frames_s16(d_pcm[s], pitch, a_starts, c, a_from, a_to, a_mod, f, keys_o, keep, out_o, work_o, wave_ops)

                def run_n(): bn.track_each_wave_frames_s16(d_pcm, pitch, d_tab, steps, d_fr, frames, keys_n, out_n, work_n, wave_ops)

                def same():
                    picked = moving if S <= 64 else moving[::max(1, len(moving) // 8)][:8]
                    keys_n.zero_(); run_n(); torch.cuda.synchronize()
                    for s, c, f, a_starts, a_from, a_to, a_mod, keep in one:
                        if s not in picked: continue
                        keys_o.zero_()
                        bo.track_wave_frames_s16(d_pcm[s], pitch, a_starts, c, a_from, a_to, a_mod, f, keys_o, keep, out_o, work_o, wave_ops)
                        torch.cuda.synchronize()
                        if not (torch.equal(out_o[:f], out_n[:f, 2 * s:2 * s + 2]) and torch.equal(keys_o, keys_n[:, 2 * s:2 * s + 2])): return False
                    return True
            if part != "b":
                run_o(); run_n(); torch.cuda.synchronize()                       # a warm-up; then both from the same state and keys
                if part == "d2": bo.reset(); bn.reset()
                keys_n.zero_(); keys_o.zero_()
                run_o(); run_n(); torch.cuda.synchronize()
            if not same():
                sys.exit(f"track_wave_frames_each_bench: part {part} streams={S}: the two sides' outputs differ")
            run_o(); l_o = bo.last_launches() * (len(one) if part == "b" else 1)
            run_n(); l_n = bn.last_launches()
            torch.cuda.synchronize()
            to_, tn = [], []
            for _ in range(args.rounds):
                to_.append(timed(run_o)); tn.append(timed(run_n))
            mo, mn = float(np.median(to_)), float(np.median(tn))
            so, sn = max(to_) - min(to_), max(tn) - min(tn)
            bound = max(so, sn) if part == "c" else so
            level = "-" if part == "b" else "yes" if abs(mn - mo) <= bound else "NO"
            line = f"  {part:>4} {S:>7} {steps:>6} {frames:>6} {mo:>10.3f} {so:>8.3f} {l_o:>8} {mn:>10.3f} {sn:>8.3f} {l_n:>8} {mo / mn:>9.2f} {level:>6}"
            print(line, flush=True)
            (compare if part in ("d1", "d2") else lines).append(line)
            bo.close(); bn.close()
            del d_pcm, work_n, work_o, out_o, out_n
            torch.cuda.empty_cache()
    for path, text in ((args.out, lines), (args.compare_out, compare)):
        if path == args.compare_out and "d" not in parts: continue
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
