"""Have the existing kernels moved?  The comparison of tools/track_frames_isa.py -- the gfx950 device code of every product object both trees have, .text and
kernel descriptors byte for byte -- between this tree's build and the parent commit's, and the registers and scratch of the new unit's kernels
(--unit, glv_decimate.hip unless given: VGPRs, SGPRs, scratch bytes, and tools/isa_stats.py's instruction mix).

    python tools/bufscale_isa.py --parent-build DIR/glava_amd/csrc/build [--unit glv_decimate] [--out profiles/r21/bufscale_isa.txt]
    python tools/bufscale_isa.py --parent-build DIR/glava_amd/csrc/build --unit glv_slots --out profiles/r22/stream_slots_isa.txt

Both trees must be built (python -m glava_amd.build).  Needs no GPU.  Exit status 1 if an object both trees have differs.  Where the unit named by --unit exists
in both trees and differs as a whole -- a kernel was added to it -- its kernels are compared one by one instead: exit status 1 if one the parent has moved."""
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
from track_frames_isa import ARCH, LLVM, device_sections  # noqa: E402


def device_kernels(obj, tmp):
    """{kernel: (bytes, sha256[:16] of its machine code, sha256[:16] of its descriptor)} of the gfx950 code object inside a host object: what is compared where
    an object differs as a whole because a kernel was added to its unit (a kernel's branches are relative, so its bytes do not depend on its neighbours)"""
    import hashlib
    fb, co = os.path.join(tmp, "k.hipfb"), os.path.join(tmp, "k.co")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fb, obj, os.path.join(tmp, "k.copy")], check=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fb, "--targets=hipv4-amdgcn-amd-amdhsa--" + ARCH, "--output=" + co], check=True)
    raw, base = {}, {}
    for line in subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-S", "-W", co], check=True, capture_output=True, text=True).stdout.split("\n"):
        m = re.match(r"\s*\[\s*\d+\]\s+(\.text|\.rodata)\s+\S+\s+([0-9a-f]+)\s", line)
        if m:
            path = os.path.join(tmp, "k" + m.group(1))
            subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=" + m.group(1), co, path], check=True)
            raw[m.group(1)], base[m.group(1)] = open(path, "rb").read(), int(m.group(2), 16)
    code, desc = {}, {}
    for line in subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-s", "-W", co], check=True, capture_output=True, text=True).stdout.split("\n"):
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC":
            at = int(f[1], 16) - base[".text"]
            code[f[7]] = raw[".text"][at:at + int(f[2])]
        elif len(f) == 8 and f[3] == "OBJECT" and f[7].endswith(".kd"):
            at = int(f[1], 16) - base[".rodata"]
            d = bytearray(raw[".rodata"][at:at + 64])
            d[16:24] = bytes(8)                                                 # the distance to the kernel's code: layout, not the kernel (device_sections)
            desc[f[7][:-3]] = bytes(d)
    return {k: (len(v), hashlib.sha256(v).hexdigest()[:16], hashlib.sha256(desc.get(k, b"")).hexdigest()[:16]) for k, v in code.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-build", required=True, help="glava_amd/csrc/build of the tree to compare with, built")
    ap.add_argument("--unit", default="glv_decimate", help="the unit new in this tree, whose kernels' registers and scratch are listed")
    ap.add_argument("--out", default=os.path.join("profiles", "r21", "bufscale_isa.txt"))
    a = ap.parse_args()
    lines = ["# device code of the product objects, gfx950: this tree against the parent commit's build.  Per object and section: bytes, sha256[:16] of this tree's, and",
             "# whether the parent's are the same bytes.  .text: the machine code of every kernel of the object; .rodata: the kernel descriptors (VGPRs, SGPRs, scratch, LDS)"]
    moved, seen, kernel_moved = 0, 0, 0
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
            there = device_sections(other, tmp)
            seen += 1
            if here != there and name == a.unit + ".o":
                # the unit that gained kernels: every kernel the parent's object has, one by one
                mine, theirs = device_kernels(obj, tmp), device_kernels(other, tmp)
                lines.append(head + f"differs as a whole (parent .text {there['.text']} .rodata {there['.rodata']}): kernel by kernel, code and descriptor --")
                for k in sorted(set(mine) | set(theirs)):
                    what = "new in this tree" if k not in theirs else "GONE" if k not in mine else "identical to the parent's" if mine[k] == theirs[k] else f"DIFFERS: parent {theirs[k]}"
                    lines.append(f"    {k:<56} {(mine.get(k) or theirs[k])[0]:>6} bytes {(mine.get(k) or theirs[k])[1]}  {what}")
                    kernel_moved += k not in mine or (k in theirs and mine[k] != theirs[k])
                moved += kernel_moved != 0
                continue
            moved += here != there
            lines.append(head + ("identical to the parent's" if here == there else f"DIFFERS: parent .text {there['.text']} .rodata {there['.rodata']}"))
        lines.append(f"# objects both trees have: {seen}; moved against the parent: {moved}")
        asm = os.path.join(tmp, a.unit + ".s")
        subprocess.run([_hipcc(), *HIPFLAGS, "--cuda-device-only", "-S", os.path.join(CSRC, a.unit + ".hip"), "-o", asm], check=True)
        text = open(asm).read()
        lines.append(f"# the new unit's kernels ({a.unit}.hip): registers and scratch from the kernel descriptors")
        for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
            g = lambda k: (re.search(r"\.amdhsa_" + k + r" (\d+)", m.group(2)) or [None, "?"])[1]    # noqa: E731
            lines.append(f"    {m.group(1)}: VGPRs {g('next_free_vgpr')}  SGPRs {g('next_free_sgpr')}  scratch {g('private_segment_fixed_size')} B  LDS {g('group_segment_fixed_size')} B")
        lines.append("# ... and their instruction mix (tools/isa_stats.py):")
        lines += ["    " + x for x in subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_stats.py"), asm], check=True, capture_output=True, text=True).stdout.split("\n") if x.strip()]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(1 if moved else 0)


if __name__ == "__main__":
    main()
