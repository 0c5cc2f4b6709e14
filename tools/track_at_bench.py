"""Track mode at given window starts (glv_batch_track_at_s16 / _f32) against what a caller had before it, alternating in one process.

  (a) the table t * 735 against glv_batch_track_windows_s16 at hop 735 in the same library (`--f32`: the float entries): what the lookup costs
  (b) glv_batch_track_windows_s16 at hop 735 in this library against the library built from the parent commit (--parent-lib, loaded beside this one):
      whether the existing entry has moved
  (c) the 22050 Hz / 60 fps table (glava_amd.track_starts.renderer_starts: 367.5 frames a step) against the same windows through glv_batch_process_s16
      one by one, the windows cut beforehand

The shipped configuration: N = 4096, the GL chain (gl_storage 1, F = 5) with the pre-smoothing pass (bars = n, bar_phase 0.5), texels out.

    python tools/track_at_bench.py [--points 1x2048,8x2048,64x2048,1024x256] [--rounds 7] [--parts a,b,c,f] [--parent-lib PATH] [--out profiles/r16/track_at.txt]

The method of tools/track_windows_bench.py.  Per point: both forms are warmed up once, their outputs compared bit for bit from a reset state, then timed
`rounds` times alternating (a host clock around the call and the device synchronise that ends it: what a caller waits for, launch overhead included).
Prints and writes the table: median ms of each form with the round-to-round spread (max - min) and the ratio.  A difference inside the spread is none.
Part f is part a from a float recording.  Part b is left out where no parent library is given.
"""
import argparse
import importlib.util
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from glava_amd import spectrum as G  # noqa: E402
from glava_amd.track_starts import renderer_starts  # noqa: E402
from oracle_lib import lcg_pcm_fast  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def load_other(path):
    """a second copy of the Python layer bound to another build of the library (its own module state, its own CDLL handle)"""
    old = os.environ.get("GLV_SPECTRUM_LIB")
    os.environ["GLV_SPECTRUM_LIB"] = os.path.abspath(path)
    try:
        spec = importlib.util.spec_from_file_location("glava_amd_spectrum_parent", os.path.join(ROOT, "glava_amd", "spectrum.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        mod.lib()
    finally:
        if old is None: del os.environ["GLV_SPECTRUM_LIB"]
        else: os.environ["GLV_SPECTRUM_LIB"] = old
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="1x2048,8x2048,64x2048,1024x256", help="streams x steps")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parts", default="a,b,c,f")
    ap.add_argument("--parent-lib", default=None, help="libglvspectrum.so built from the parent commit (part b)")
    ap.add_argument("--out", default=os.path.join("profiles", "r16", "track_at.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("track_at_bench: no GPU -- nothing is measured without one")
    n, hop = args.n, 735
    parts = [q for q in args.parts.split(",") if q != "b" or args.parent_lib]
    GP = load_other(args.parent_lib) if "b" in parts else None
    GA = G.OP_GRAVITY | G.OP_AVERAGE
    mask, ops = GA | G.OP_BARS, G.OP_FFT | GA | G.OP_BARS | G.OP_R16
    kw = dict(n=n, gl_storage=1, avg_window_kind=1, log_mode=1, bars=n, bar_phase=0.5)
    p = G.Params(**kw)
    lines = [f"# track_at_bench: N={n} gl_storage=1 F={p.avg_frames} bars=n bar_phase=0.5 texels out; {torch.cuda.get_device_name(0)}",
             f"# ms = host clock around the call(s) and the synchronise that ends them, median of {args.rounds} alternating rounds (spread = max - min)",
             "# a: `other` = glv_batch_track_windows_s16 at hop 735, `table` = glv_batch_track_at_s16 with the table t * 735 (f: the same, _f32 entries, float recording)",
             "# b: `other` = glv_batch_track_windows_s16 at hop 735 in the parent commit's library, `table` column = the same entry in this library",
             "# c: `other` = the same windows through glv_batch_process_s16 one by one, `table` = glv_batch_track_at_s16 with the 22050 Hz / 60 fps table",
             f"# {'part':>4} {'streams':>7} {'steps':>6} {'other ms':>10} {'spread':>8} {'launches':>8} {'table ms':>10} {'spread':>8} {'launches':>8} {'work MiB':>9} {'other/table':>11}"]
    print("\n".join(lines), flush=True)
    points = [tuple(int(v) for v in pt.split("x")) for pt in args.points.split(",")]
    for part in parts:
        f32 = part == "f"
        for S, steps in points:
            starts = renderer_starts(22050, 60, 1, steps) if part == "c" else [t * hop for t in range(steps)]
            pitch = (max(starts) + n + 1) | 1                                   # odd
            bn = G.Batch(p, S, mask)
            if part == "b":
                bo = GP.Batch(GP.Params(**kw), S, mask)
            else:
                bo = G.Batch(p, S, mask)
            wb = bn.track_at_work_bytes(steps, ops)                               # (the windows query's value for the same steps)
            x = lcg_pcm_fast(4242 + S, S * pitch * 2).reshape(-1, 2)
            if f32:
                x = x.astype(np.float32) / np.float32(32768)
            buf = torch.from_numpy(x).cuda()
            d_pcm = buf.view(S, pitch, 2)
            d_starts = torch.from_numpy(np.asarray(starts, dtype=np.uint32).view(np.int32).copy()).cuda()
            work = torch.empty((wb,), dtype=torch.uint8, device="cuda")
            out_o = torch.zeros((steps, S * 2, n), dtype=torch.int16, device="cuda")
            out_n = torch.zeros_like(out_o)
            wins = None
            if part == "c":
                wins = torch.stack([d_pcm[:, s:s + n, :] for s in starts]).contiguous()         # [steps][S][n][2]

                def run_o():
                    for t in range(steps):
                        bo.process_s16(wins[t], out_o[t], ops)
            elif f32:
                def run_o():
                    bo.track_windows_f32(d_pcm, pitch, hop, steps, out_o, work, ops)
            else:
                def run_o():
                    bo.track_windows_s16(d_pcm, pitch, hop, steps, out_o, work, ops)
            if part == "b":
                def run_n():
                    bn.track_windows_s16(d_pcm, pitch, hop, steps, out_n, work, ops)
            elif f32:
                def run_n():
                    bn.track_at_f32(d_pcm, pitch, d_starts, steps, out_n, work, ops)
            else:
                def run_n():
                    bn.track_at_s16(d_pcm, pitch, d_starts, steps, out_n, work, ops)

            run_o(); l_o = steps * bo.last_launches() if part == "c" else bo.last_launches()
            run_n(); l_n = bn.last_launches()
            bo.reset(); bn.reset()
            run_o(); run_n()
            torch.cuda.synchronize()
            if not torch.equal(out_o, out_n):
                sys.exit(f"track_at_bench: part {part} streams={S}: the two forms' outputs differ")
            to, tn = [], []
            for _ in range(args.rounds):
                to.append(timed(run_o)); tn.append(timed(run_n))
            mo, mn = float(np.median(to)), float(np.median(tn))
            line = (f"  {part:>4} {S:>7} {steps:>6} {mo:>10.3f} {max(to) - min(to):>8.3f} {l_o:>8} {mn:>10.3f} {max(tn) - min(tn):>8.3f} {l_n:>8} {wb / 2 ** 20:>9.1f} {mo / mn:>11.3f}")
            print(line, flush=True)
            lines.append(line)
            bo.close(); bn.close()
            del buf, d_pcm, work, out_o, out_n, wins
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
