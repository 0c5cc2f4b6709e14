"""Have the existing kernels moved?  The device code of every product object both trees have -- the frame kernels (glv_inst_*), glv_misc (the scan, the small
kernels) and glv_bars (every bars kernel) -- compared between this tree's build and another tree's (the parent commit's), and the figures of
tools/isa_stats.py for the kernels of the new unit.

    python tools/track_frames_isa.py --parent-build DIR/glava_amd/csrc/build [--out profiles/r19/track_frames_isa.txt]

Per object: the gfx950 code object is taken out of the host object's .hip_fatbin section (llvm-objcopy, clang-offload-bundler) and its .text section -- the
machine code of every kernel in it -- is compared byte for byte; the kernel descriptors (.rodata: registers, scratch, LDS) likewise, but for each
descriptor's offset to its code.  Identical bytes are
identical registers, scratch and instruction counts, and more.  Both trees must be built (python -m glava_amd.build).  Needs no GPU.  Exit status 1 if an
object both trees have differs."""
import argparse
import glob
import hashlib
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from glava_amd.build import ARCH, CSRC, HIPFLAGS, OBJ, _hipcc  # noqa: E402

LLVM = "/opt/rocm/llvm/bin"


def device_sections(obj, tmp):
    """{section: sha256} of the .text and .rodata of the gfx950 code object inside a host object"""
    fb, co = os.path.join(tmp, "x.hipfb"), os.path.join(tmp, "x.co")
    if ".hip_fatbin" not in subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-S", obj], check=True, capture_output=True, text=True).stdout:
        return {".text": (0, "-"), ".rodata": (0, "-")}                          # (a part no kernel of this size is built for)
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fb, obj, os.path.join(tmp, "x.copy")], check=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fb, "--targets=hipv4-amdgcn-amd-amdhsa--" + ARCH, "--output=" + co], check=True)
    out = {}
    for sec in (".text", ".rodata"):
        raw = os.path.join(tmp, "x" + sec)
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=" + sec, co, raw], check=True)
        data = bytearray(open(raw, "rb").read())
        if sec == ".rodata" and len(data) % 64 == 0:
            # a kernel descriptor is 64 bytes, of which bytes 16-23 hold the distance from the descriptor to its kernel's code: that moves with the section
            # layout (the length of a source path in a note is enough) and says nothing about the kernel -- left out of the comparison
            for d in range(0, len(data), 64): data[d + 16:d + 24] = bytes(8)
        out[sec] = (len(data), hashlib.sha256(data).hexdigest()[:16])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-build", required=True, help="glava_amd/csrc/build of the tree to compare with, built")
    ap.add_argument("--out", default=os.path.join("profiles", "r19", "track_frames_isa.txt"))
    a = ap.parse_args()
    lines = ["# device code of the product objects, gfx950: this tree against the parent commit's build.  Per object and section: bytes, sha256[:16] of this tree's, and",
             "# whether the parent's are the same bytes.  .text: the machine code of every kernel of the object; .rodata: the kernel descriptors (VGPRs, SGPRs, scratch, LDS)"]
    moved, seen = 0, 0
    with tempfile.TemporaryDirectory() as tmp:
        for obj in sorted(glob.glob(os.path.join(OBJ, "*.o"))):
            name = os.path.basename(obj)
            if not name.startswith(("glv_inst_", "glv_misc", "glv_bars", "glv_track_frames")): continue      # (the host units hold no kernels)
            here = device_sections(obj, tmp)
            other = os.path.join(a.parent_build, name)
            if not os.path.exists(other):
                lines.append(f"{name:<22} .text {here['.text'][0]:>8} {here['.text'][1]}  .rodata {here['.rodata'][0]:>6} {here['.rodata'][1]}  new in this tree")
                continue
            there = device_sections(other, tmp)
            same = here == there
            seen += 1
            moved += not same
            lines.append(f"{name:<22} .text {here['.text'][0]:>8} {here['.text'][1]}  .rodata {here['.rodata'][0]:>6} {here['.rodata'][1]}  "
                         + ("identical to the parent's" if same else f"DIFFERS: parent .text {there['.text']} .rodata {there['.rodata']}"))
        lines.append(f"# objects both trees have: {seen}; moved against the parent: {moved}")
        asm = os.path.join(tmp, "frames.s")
        subprocess.run([_hipcc(), *HIPFLAGS, "--cuda-device-only", "-S", os.path.join(CSRC, "glv_track_frames.hip"), "-o", asm], check=True)
        lines.append("# the new unit's kernels (tools/isa_stats.py):")
        lines += ["    " + x for x in subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_stats.py"), asm], check=True, capture_output=True, text=True).stdout.split("\n") if x.strip()]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(1 if moved else 0)


if __name__ == "__main__":
    main()
