"""Have the existing kernels moved, and what do the two copies of a per-stream ring track call cost beside the lockstep pair?  tools/ring_track_isa.py's
comparison -- the gfx950 device code of every product object both trees have, .text and kernel descriptors byte for byte, against the parent commit's build,
every object that differs compared kernel by kernel -- then the kernels of glv_ring_each (new) and of glv_ring_track (the parent's, the yardstick) with
registers, scratch, LDS and instruction counts (compiled to assembly).

    python -m glava_amd.build && python tools/ring_track_each_isa.py --parent-build DIR/glava_amd/csrc/build [--out profiles/r30/ring_track_each_isa.txt]

Both trees must be built.  Needs no GPU.  Exit status 1 if an object or kernel of the parent's has moved or is gone."""
import argparse
import glob
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from glava_amd.build import CSRC, OBJ, SMALL  # noqa: E402
from bufscale_isa import device_kernels  # noqa: E402
from track_each_isa import asm_kernels  # noqa: E402
from track_frames_isa import device_sections  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-build", required=True, help="glava_amd/csrc/build of the tree to compare with, built")
    ap.add_argument("--out", default=os.path.join("profiles", "r30", "ring_track_each_isa.txt"))
    a = ap.parse_args()
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
        lines.append("# from the device assembly: VGPRs, SGPRs, scratch bytes, static LDS bytes, instructions -- glv_ring_each (new in this tree) beside glv_ring_track (the lockstep pair)")
        for unit in ("glv_ring_each", "glv_ring_track"):
            for k, (v, sg, s, lds, ins) in sorted(asm_kernels(CSRC, unit, tmp, "new").items()):
                lines.append(f"    {unit}: {k}: VGPRs {v}  SGPRs {sg}  scratch {s} B  LDS {lds} B  instructions {ins}")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(1 if moved else 0)


if __name__ == "__main__":
    main()
