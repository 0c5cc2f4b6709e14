"""Have the existing kernels moved, and what do the planar track kinds cost?  tools/bufscale_isa.py's comparison -- the gfx950 device code of every product
object both trees have, .text and kernel descriptors byte for byte, against the parent commit's build -- with EVERY unit that gained kernels compared kernel by
kernel (glv_misc, glv_decimate, glv_track_frames), then the registers and scratch of each new kind: the frame kernel's IN_F32_PLANAR_TRACK_AT (part 7 of
glv_inst.hip) beside its IN_F32_TRACK_AT twin (part 6) of the same size, configuration, log mode and class, and the new kernels of the three small units.

    python -m glava_amd.build && python tools/track_planar_isa.py --parent-build DIR/glava_amd/csrc/build [--out profiles/r24/track_planar_isa.txt]

Both trees must be built.  Needs no GPU.  Exit status 1 if a kernel the parent has moved or is gone, or if a planar frame kernel has scratch where its twin has none."""
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
from track_f32_isa import kernels  # noqa: E402
from track_frames_isa import device_sections  # noqa: E402

NEW = {"glv_misc": r"glv_wave_kernelILi5E", "glv_decimate": r"glv_decimate_kernelILi3E", "glv_track_frames": r"_planar_kernel"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-build", required=True, help="glava_amd/csrc/build of the tree to compare with, built")
    ap.add_argument("--out", default=os.path.join("profiles", "r24", "track_planar_isa.txt"))
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
                if k not in theirs or what != "identical to the parent's":
                    lines.append(f"    {k:<72} {(mine.get(k) or theirs[k])[0]:>6} bytes {(mine.get(k) or theirs[k])[1]}  {what}")
                bad += k not in mine or (k in theirs and mine[k] != theirs[k])
            lines.append(f"    ... {len(theirs)} kernels of the parent's object, {len(theirs) - bad} identical in code and descriptor")
            moved += bad != 0
        lines.append(f"# objects both trees have: {seen}; identical as a whole: {identical}; with a kernel of the parent's moved or gone: {moved}")
        # the frame kernel's planar table kind beside its interleaved twin
        lines += ["# glv_frame_kernel: IN_F32_PLANAR_TRACK_AT (9) beside IN_F32_TRACK_AT (8), the same size, configuration, log mode and class (0 plain, 3 texel rows)",
                  f"# {'N':>6} {'log':>3} {'slots':>5} {'E':>3} {'class':>5}   {'twin vgpr':>9} {'scratch':>7}   {'planar vgpr':>11} {'scratch':>7}   {'d vgpr':>6} {'d scratch':>9}"]
        worse = 0
        for k in range(7, 15):
            twin = kernels(os.path.join(OBJ, f"glv_inst_{k}_6.o"))
            planar = kernels(os.path.join(OBJ, f"glv_inst_{k}_7.o"))
            for args, (v, _, s) in sorted(planar.items()):
                assert args[1] == "9", args
                tv, _, ts = twin[args[:1] + ("8",) + args[2:]]
                worse += s > 0 and ts == 0
                lines.append(f"  {2 << int(args[0]):>6} {args[2]:>3} {args[3]:>5} {1 << int(args[10]):>3} {args[11]:>5}   {tv:>9} {ts:>7}   {v:>11} {s:>7}   {v - tv:>+6} {s - ts:>+9}")
        lines.append(f"# planar kinds with scratch where the twin has none: {worse}")
        lines.append("# the new kernels of the small units: registers and scratch from the kernel descriptors")
        for unit, pat in NEW.items():
            asm = os.path.join(tmp, unit + ".s")
            subprocess.run([_hipcc(), *HIPFLAGS, "--cuda-device-only", "-S", os.path.join(CSRC, unit + ".hip"), "-o", asm], check=True, capture_output=True)
            for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", open(asm).read(), re.S):
                if not re.search(pat, m.group(1)): continue
                g = lambda key: (re.search(r"\.amdhsa_" + key + r" (\d+)", m.group(2)) or [None, "?"])[1]    # noqa: E731
                lines.append(f"    {unit}: {m.group(1)}: VGPRs {g('next_free_vgpr')}  SGPRs {g('next_free_sgpr')}  scratch {g('private_segment_fixed_size')} B  LDS {g('group_segment_fixed_size')} B")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(1 if moved or worse else 0)


if __name__ == "__main__":
    main()
