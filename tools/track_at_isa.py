"""VGPRs and scratch of the table kinds of the frame kernel (IN_S16_TRACK_AT, IN_F32_TRACK_AT) beside their hop kinds, from the product's own objects --
and, with --parent-build, the hop kinds beside those of another build (the parent commit's): have the existing kernels moved?

    python -m glava_amd.build && python tools/track_at_isa.py [--parent-build DIR] [--out profiles/r16/track_at_isa.txt]

Reads glava_amd/csrc/build/glv_inst_<k>_<part>.o (parts 3 / 4: the hop kinds, parts 5 / 6: the table kinds) the way tools/track_f32_isa.py does.  Needs no
GPU.  Exit status 1 if a hop kind differs from the parent build's in registers or scratch."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from track_f32_isa import OBJ, kernels  # noqa: E402

PAIRS = ((3, 5, "5", "7"), (4, 6, "6", "8"))      # hop part, table part, hop IN_MODE, table IN_MODE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-build", default=None, help="glava_amd/csrc/build of the library the hop kinds are compared with")
    ap.add_argument("--out", default=os.path.join("profiles", "r16", "track_at_isa.txt"))
    a = ap.parse_args()
    lines = ["# glv_frame_kernel, gfx950: the table kinds IN_S16_TRACK_AT (7) / IN_F32_TRACK_AT (8) beside the hop kinds IN_S16_TRACK (5) / IN_F32_TRACK (6)",
             "# of the same size, configuration, log mode and class (0 plain, 3 texel rows)",
             f"# {'N':>6} {'mode':>4} {'log':>3} {'slots':>5} {'E':>3} {'class':>5}   {'hop vgpr':>8} {'scratch':>7}   {'table vgpr':>10} {'scratch':>7}   {'d vgpr':>6} {'d scratch':>9}"]
    more = moved = total = 0
    for k in range(7, 15):
        for hop_part, table_part, hop_mode, table_mode in PAIRS:
            hop = kernels(os.path.join(OBJ, f"glv_inst_{k}_{hop_part}.o"))
            table = kernels(os.path.join(OBJ, f"glv_inst_{k}_{table_part}.o"))
            for args, (v, _, s) in sorted(table.items()):
                assert args[1] == table_mode, args
                tv, _, ts = hop[args[:1] + (hop_mode,) + args[2:]]
                more += s > ts
                lines.append(f"  {2 << int(args[0]):>6} {args[1]:>4} {args[2]:>3} {args[3]:>5} {1 << int(args[10]):>3} {args[11]:>5}   {tv:>8} {ts:>7}   {v:>10} {s:>7}   {v - tv:>+6} {s - ts:>+9}")
            if a.parent_build:
                old = kernels(os.path.join(a.parent_build, f"glv_inst_{k}_{hop_part}.o"))
                assert old.keys() == hop.keys()
                total += len(hop)
                moved += sum(old[key] != hop[key] for key in hop)
    lines.append(f"# table kinds with more scratch than their hop kind: {more}")
    if a.parent_build:
        lines.append(f"# hop kinds whose VGPRs, AGPRs or scratch differ from the parent build's: {moved} of {total}")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(1 if moved else 0)


if __name__ == "__main__":
    main()
