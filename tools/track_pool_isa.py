"""Have the existing kernels moved, and what do the pool kinds of a track call cost?  tools/track_each_isa.py's comparison -- the gfx950 device code of every
product object both trees have, .text and kernel descriptors byte for byte, against the parent commit's build, every object that differs compared kernel by
kernel -- then:

  * the frame kernel's pool kinds (IN_S16_TRACK_POOL 13, IN_F32_TRACK_POOL 14, IN_F32_PLANAR_TRACK_POOL 15: parts 11, 12, 13 of glv_inst.hip) beside their
    per-stream siblings (10, 11, 12: parts 8, 9, 10) of the same size, configuration, log mode and class.  A pool kind IS its sibling with the stream's 16-byte
    span loaded beside the table entry and pool_window_start in the place of the clamp: d vgpr / d scratch is what the span costs;
  * the kernels of glv_pool (new) beside the kinds of glv_decimate_kernel and glv_wave_kernel they restate, with registers, scratch, LDS and instruction
    counts (compiled to assembly), and those kinds in both trees.

    python -m glava_amd.build && python tools/track_pool_isa.py --parent-build DIR/glava_amd/csrc/build [--out profiles/r26/track_pool_isa.txt]

Both trees must be built; the parent's sources are taken from beside its build directory.  Needs no GPU.  Exit status 1 if an object or kernel of the parent's
has moved or is gone (what the pool kinds cost beside their siblings is reported, not judged)."""
import argparse
import glob
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from glava_amd.build import CSRC, OBJ, SMALL  # noqa: E402
from bufscale_isa import device_kernels  # noqa: E402
from track_each_isa import asm_kernels  # noqa: E402
from track_f32_isa import kernels  # noqa: E402
from track_frames_isa import device_sections  # noqa: E402

WATCHED = r"glv_wave_kernel|glv_decimate_kernel"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-build", required=True, help="glava_amd/csrc/build of the tree to compare with, built")
    ap.add_argument("--out", default=os.path.join("profiles", "r26", "track_pool_isa.txt"))
    a = ap.parse_args()
    parent_csrc = os.path.dirname(os.path.abspath(a.parent_build))
    lines = ["# device code of the product objects, gfx950: this tree against the parent commit's build.  Per object: .text and .rodata (kernel descriptors) bytes and",
             "# sha256[:16]; an object that differs as a whole is compared kernel by kernel, machine code and descriptor"]
    moved = seen = identical = 0
    with tempfile.TemporaryDirectory() as tmp:
        for obj in sorted(glob.glob(os.path.join(OBJ, "*.o"))):
            name = os.path.basename(obj)
            if not name.startswith(("glv_inst_", *SMALL)): continue              # (the host units hold no kernels)
            here = device_sections(obj, tmp)
            other = os.path.join(a.parent_build, name)
            head = f"{name:<22} .text {here['.text'][0]:>8} {here['.text'][1]}  .rodata {here['.rodata'][0]:>6} {here['.rodata'][1]}  "
            if not os.path.exists(other):
                lines.append(head + "new in this tree")
                continue
            seen += 1
            there = device_sections(other, tmp)
            if here == there:
                identical += 1
                lines.append(head + "identical to the parent's")
                continue
            mine, theirs = device_kernels(obj, tmp), device_kernels(other, tmp)
            lines.append(head + f"differs as a whole (parent .text {there['.text']} .rodata {there['.rodata']}): kernel by kernel --")
            bad = 0
            for k in sorted(set(mine) | set(theirs)):
                what = "new in this tree" if k not in theirs else "GONE" if k not in mine else "identical to the parent's" if mine[k] == theirs[k] else f"DIFFERS: parent {theirs[k]}"
                lines.append(f"    {k:<72} {(mine.get(k) or theirs[k])[0]:>6} bytes {(mine.get(k) or theirs[k])[1]}  {what}")
                bad += k not in mine or (k in theirs and mine[k] != theirs[k])
            lines.append(f"    ... {len(theirs)} kernels of the parent's object, {len(theirs) - bad} identical in code and descriptor")
            moved += bad != 0
        lines.append(f"# objects both trees have: {seen}; identical as a whole: {identical}; objects with a kernel of the parent's moved or gone: {moved}")
        lines += ["# glv_frame_kernel: the pool kinds (13, 14, 15) beside their per-stream siblings (10, 11, 12), the same size, configuration, log mode and class (0 plain,",
                  "# 3 texel rows).  The pool kind is the sibling with the span's 16-byte load and pool_window_start: d vgpr / d scratch is what the span costs",
                  f"# {'kind':>4} {'N':>6} {'log':>3} {'slots':>5} {'E':>3} {'class':>5}   {'each vgpr':>9} {'sgpr':>5} {'scratch':>7}   {'pool vgpr':>9} {'sgpr':>5} {'scratch':>7}   {'d vgpr':>6} {'d sgpr':>6} {'d scratch':>9}"]
        worse = grew = total = 0
        for each_part, pool_part, each_kind, pool_kind in ((8, 11, "10", "13"), (9, 12, "11", "14"), (10, 13, "12", "15")):
            for k in range(7, 15):
                each = kernels(os.path.join(OBJ, f"glv_inst_{k}_{each_part}.o"))
                pool = kernels(os.path.join(OBJ, f"glv_inst_{k}_{pool_part}.o"))
                for args, (v, sg, s) in sorted(pool.items()):
                    assert args[1] == pool_kind, args
                    tv, tsg, ts = each[args[:1] + (each_kind,) + args[2:]]
                    total += 1
                    worse += s > 0 and ts == 0
                    grew += v > tv or s > ts
                    lines.append(f"  {pool_kind:>4} {2 << int(args[0]):>6} {args[2]:>3} {args[3]:>5} {1 << int(args[10]):>3} {args[11]:>5}   {tv:>9} {tsg:>5} {ts:>7}   {v:>9} {sg:>5} {s:>7}"
                                 f"   {v - tv:>+6} {sg - tsg:>+6} {s - ts:>+9}")
        lines.append(f"# pool frame kernels: {total}; with more VGPRs or scratch than the sibling: {grew}; with scratch where the sibling has none: {worse}")
        lines += ["# glv_pool (new) beside the kinds it restates in glv_decimate and glv_misc (both trees), from the device assembly: VGPRs, SGPRs, scratch bytes, static LDS",
                  "# bytes, instructions (parent's in brackets where they moved)"]
        small_moved = 0
        for k, (v, sg, s, lds, ins) in sorted(asm_kernels(CSRC, "glv_pool", tmp, "new").items()):
            lines.append(f"    glv_pool: {k}: VGPRs {v}  SGPRs {sg}  scratch {s} B  LDS {lds} B  instructions {ins}  new in this tree")
        for unit in ("glv_decimate", "glv_misc"):
            mine, theirs = asm_kernels(CSRC, unit, tmp, "new"), asm_kernels(parent_csrc, unit, tmp, "parent")
            for k in sorted(mine):
                if not re.search(WATCHED, k): continue
                old = theirs.get(k)
                v, sg, s, lds, ins = mine[k]
                was = "new in this tree" if old is None else "as the parent's" if old == mine[k] else f"MOVED: parent [VGPRs {old[0]} SGPRs {old[1]} scratch {old[2]} LDS {old[3]} instructions {old[4]}]"
                small_moved += old is not None and old != mine[k]
                lines.append(f"    {unit}: {k}: VGPRs {v}  SGPRs {sg}  scratch {s} B  LDS {lds} B  instructions {ins}  {was}")
        lines.append(f"# decimate and wave kinds that existed and moved: {small_moved}")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(1 if moved or small_moved else 0)


if __name__ == "__main__":
    main()
