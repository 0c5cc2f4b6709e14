"""Have the existing kernels moved?  Registers and scratch of every kernel of chosen translation units, compiled from this tree and from another tree's
sources (the parent commit's), side by side: the frame kernel's classes (glv_inst.hip, per size and part), the track scan's kinds (glv_misc.hip) and the bars
kernels (glv_bars.hip).  gl_storage 3 added two frame classes (FC_STATE_SNAP 14, FC_STATE_COLS 15), a store limit in the texel-row epilogue of classes 3 and
4, and a texel-row kind of glv_bars_mode_kernel; everything else must keep its figures.

    python tools/upload_chain_isa.py --parent-csrc DIR/glava_amd/csrc [--sizes 9,11,13] [--parts 0] [--out profiles/r18/upload_chain_isa.txt]

Compiles the device side with the product's flags (glava_amd.build.HIPFLAGS) into a temporary directory; reads the .amdhsa_ metadata of every kernel
(next_free_vgpr, next_free_sgpr, private_segment_fixed_size = scratch bytes per lane) and the instruction count between the kernel's label and its
s_endpgm.  Needs no GPU.  Exit status 1 if a kernel both trees have differs in registers or scratch."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from glava_amd.build import CSRC, HIPFLAGS, _hipcc  # noqa: E402


def kernels(csrc, src, flags, tmp, tag):
    """{demangled kernel name: (vgpr, sgpr, scratch, instructions)}"""
    asm = os.path.join(tmp, tag + ".s")
    subprocess.run([_hipcc(), *HIPFLAGS, *flags, "--cuda-device-only", "-S", os.path.join(csrc, src), "-o", asm], check=True, capture_output=True)
    text = open(asm).read()
    meta = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        g = lambda k: int((re.search(r"\.amdhsa_" + k + r" (\d+)", m.group(2)) or [None, "-1"])[1])     # noqa: E731
        body = re.search(r"^" + re.escape(m.group(1)) + r":[^\n]*\n(.*?)\n\s*s_endpgm", text, re.S | re.M)
        count = sum(1 for ln in body.group(1).split("\n") if re.match(r"\s+[sv]_|\s+(global|ds|scratch|buffer|flat)_", ln)) if body else -1
        meta[m.group(1)] = (g("next_free_vgpr"), g("next_free_sgpr"), g("private_segment_fixed_size"), count)
    names = subprocess.run(["c++filt"], input="\n".join(meta), capture_output=True, text=True).stdout.split("\n")
    return {re.sub(r"^void ", "", d): meta[k] for k, d in zip(meta, names)}


def frame_class(name):
    """the kernel class of a glv_frame_kernel instantiation: its twelfth template argument"""
    m = re.search(r"glv_frame_kernel<([^>]*)>", name)
    return int(m.group(1).split(",")[11]) if m else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-csrc", required=True, help="glava_amd/csrc of the tree the kernels are compared with")
    ap.add_argument("--sizes", default="9,11,13", help="log2(nn) of the glv_inst.hip units (9: N = 1024, 11: 4096, 13: 16384)")
    ap.add_argument("--parts", default="0", help="GLV_INST_PART of the glv_inst.hip units")
    ap.add_argument("--out", default=os.path.join("profiles", "r18", "upload_chain_isa.txt"))
    a = ap.parse_args()
    units = [("glv_inst.hip", [f"-DGLV_LOG_NN={k}", f"-DGLV_INST_PART={p}"], f"inst_{k}_{p}") for k in a.sizes.split(",") for p in a.parts.split(",")]
    units += [("glv_misc.hip", [], "misc"), ("glv_bars.hip", [], "bars")]
    lines = ["# registers / scratch of every kernel, this tree against the parent's sources; gfx950, the product's flags",
             "# per unit: kernels both trees have (identical / moved), then the kernels only this tree has: vgpr sgpr scratch instructions"]
    moved_total = 0
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 2)) as ex:
        jobs = [(u, ex.submit(kernels, CSRC, u[0], u[1], tmp, "this_" + u[2]), ex.submit(kernels, a.parent_csrc, u[0], u[1], tmp, "parent_" + u[2])) for u in units]
        for (src, flags, tag), f_here, f_parent in jobs:
            here, parent = f_here.result(), f_parent.result()
            both = sorted(set(here) & set(parent))
            moved = [k for k in both if here[k][:3] != parent[k][:3]]
            resized = [k for k in both if here[k][:3] == parent[k][:3] and here[k][3] != parent[k][3]]
            moved_total += len(moved)
            lines.append(f"{src} {' '.join(flags)}: {len(both)} kernels in both trees, {len(both) - len(moved)} with the parent's vgpr / sgpr / scratch, {len(moved)} moved; "
                         f"{len(resized)} of the unmoved differ in instruction count")
            per_class = {}
            for k in both:
                c = frame_class(k)
                if c is not None:
                    per_class.setdefault(c, []).append(k)
            for c in sorted(per_class):
                ks = per_class[c]
                v = sorted({here[k][0] for k in ks}); s = sorted({here[k][2] for k in ks})
                lines.append(f"    class {c:>2}: {len(ks):>3} kernels, vgpr {v[0]}-{v[-1]}, scratch {s[0]}-{s[-1]} bytes: "
                             f"{sum(1 for k in ks if k in moved)} moved, {sum(1 for k in ks if k in resized)} other instruction count")
            for k in moved:
                lines.append(f"    MOVED {k}: parent {parent[k]} -> {here[k]}")
            for k in resized:
                lines.append(f"    instructions {parent[k][3]} -> {here[k][3]}: {k}")
            for k in sorted(set(here) - set(parent)):
                lines.append(f"    new   {k}: {here[k]}")
            for k in sorted(set(parent) - set(here)):
                lines.append(f"    gone  {k}: {parent[k]}")
    lines.append(f"# kernels that moved against the parent: {moved_total}")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(1 if moved_total else 0)


if __name__ == "__main__":
    main()
