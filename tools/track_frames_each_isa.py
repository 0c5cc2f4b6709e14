"""Have the existing kernels moved, and what do the per-stream frames kernels take?  tools/track_pool_isa.py's comparison -- the gfx950 device code of every
product object both trees have, .text and kernel descriptors byte for byte, against the parent commit's build, every object that differs compared kernel by
kernel (glv_track_frames differs as a whole: two kernels were added to it) -- then the kernels of glv_track_frames.hip from the device assembly: registers,
scratch, LDS and instruction counts of glv_track_frames_each_kernel and glv_track_keys_each_kernel beside glv_track_frames_kernel and glv_track_keys_kernel,
with their scalar and vector memory loads counted (the per-stream kernels read their tables and counts through uniform loads).

    python -m glava_amd.build && python tools/track_frames_each_isa.py --parent-build DIR/glava_amd/csrc/build [--out profiles/r27/track_frames_each_isa.txt]

Both trees must be built; the parent's sources are taken from beside its build directory.  Needs no GPU.  Exit status 1 if an object or kernel of the parent's
has moved or is gone."""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from glava_amd.build import CSRC, HIPFLAGS, OBJ, SMALL, _hipcc  # noqa: E402
from bufscale_isa import device_kernels  # noqa: E402
from track_each_isa import asm_kernels  # noqa: E402
from track_frames_isa import device_sections  # noqa: E402

WATCHED = r"glv_track_frames_kernel|glv_track_keys_kernel|glv_track_frames_each_kernel|glv_track_keys_each_kernel"


def loads(csrc, unit, tmp, tag):
    """name -> (scalar loads, vector loads, vector stores, waits on the vector memory counter) of every kernel of a unit, from its device assembly"""
    asm = os.path.join(tmp, f"{unit}_{tag}_loads.s")
    subprocess.run([_hipcc(), *HIPFLAGS, "--cuda-device-only", "-S", os.path.join(csrc, unit + ".hip"), "-o", asm], check=True, capture_output=True)
    text = open(asm).read()
    out = {}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end", text, re.S | re.M):
        body = m.group(2)
        out[m.group(1)] = (len(re.findall(r"^\s+s_load_", body, re.M)), len(re.findall(r"^\s+global_load_", body, re.M)), len(re.findall(r"^\s+global_store_", body, re.M)),
                           len(re.findall(r"vmcnt\(", body)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-build", required=True, help="glava_amd/csrc/build of the tree to compare with, built")
    ap.add_argument("--out", default=os.path.join("profiles", "r27", "track_frames_each_isa.txt"))
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
        lines += ["# glv_track_frames: the per-stream kernels beside the lockstep ones, from the device assembly: VGPRs, SGPRs, scratch bytes, static LDS bytes, instructions;",
                  "# scalar memory loads, vector memory loads, vector memory stores, waits that name the vector memory counter (parent's in brackets where they moved)"]
        mine, theirs = asm_kernels(CSRC, "glv_track_frames", tmp, "new"), asm_kernels(parent_csrc, "glv_track_frames", tmp, "parent")
        mem = loads(CSRC, "glv_track_frames", tmp, "new")
        small_moved = 0
        for k in sorted(mine):
            if not re.search(WATCHED, k): continue
            old = theirs.get(k)
            v, sg, s, lds, ins = mine[k]
            sl, vl, vs, waits = mem.get(k, (-1, -1, -1, -1))
            was = "new in this tree" if old is None else "as the parent's" if old == mine[k] else f"MOVED: parent [VGPRs {old[0]} SGPRs {old[1]} scratch {old[2]} LDS {old[3]} instructions {old[4]}]"
            small_moved += old is not None and old != mine[k]
            lines.append(f"    {k}: VGPRs {v}  SGPRs {sg}  scratch {s} B  LDS {lds} B  instructions {ins}  s_load {sl}  global_load {vl}  global_store {vs}  vmcnt waits {waits}  {was}")
        lines.append(f"# frames and write-back kernels that existed and moved: {small_moved}")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(1 if moved or small_moved else 0)


if __name__ == "__main__":
    main()
