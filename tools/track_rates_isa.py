"""Registers, scratch and instruction mix of glv_track_scan_kernel's kinds (glava_amd/csrc/glv_misc.hip): the rates kinds of glv_batch_track_rates_s16 / _f32
beside the two kinds every other track call runs -- and, with --parent-csrc, those two beside the same kernels compiled from another tree's sources (the
parent commit's): have the existing kinds moved?

    python tools/track_rates_isa.py [--parent-csrc DIR/glava_amd/csrc] [--out profiles/r17/track_rates_isa.txt]

Compiles the device side of glv_misc.hip to assembly with the product's flags (glava_amd.build.HIPFLAGS) into a temporary directory and summarises it with
tools/isa_stats.py.  Needs no GPU.  Exit status 1 if an existing kind differs from the parent's in any figure."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from glava_amd.build import CSRC, HIPFLAGS, _hipcc  # noqa: E402


def scan_kinds(csrc, tmp, tag):
    """{template arguments: [summary lines of tools/isa_stats.py]} of the scan kernel's instantiations in csrc/glv_misc.hip"""
    asm = os.path.join(tmp, tag + ".s")
    subprocess.run([_hipcc(), *HIPFLAGS, "--cuda-device-only", "-S", os.path.join(csrc, "glv_misc.hip"), "-o", asm], check=True)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_stats.py"), asm], check=True, capture_output=True, text=True).stdout.split("\n")
    sgpr = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", open(asm).read(), re.S):
        sgpr[m.group(1)] = (re.search(r"\.amdhsa_next_free_sgpr (\d+)", m.group(2)) or [None, "?"])[1]
    kinds = {}
    for i, line in enumerate(out):
        m = re.search(r"glv_track_scan_kernel<([^>]*)>", line)
        if m:
            mangled = [k for k in sgpr if "glv_track_scan_kernel" in k and subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip() == line.strip()]
            extra = f"    sgpr {sgpr[mangled[0]]}" if mangled else ""
            kinds[m.group(1)] = [out[i + 1].strip() + extra, out[i + 2].strip()]
    return kinds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-csrc", default=None, help="glava_amd/csrc of the tree the existing kinds are compared with")
    ap.add_argument("--out", default=os.path.join("profiles", "r17", "track_rates_isa.txt"))
    a = ap.parse_args()
    lines = ["# glv_track_scan_kernel, gfx950, the product's flags: <IN16, RATES> -- <false, false> float rows, <true, false> texel rows (every track call before the",
             "# rates entries), <false, true> / <true, true> the rates kinds of glv_batch_track_rates_s16 / _f32.  Figures: tools/isa_stats.py (static instruction counts)"]
    with tempfile.TemporaryDirectory() as tmp:
        here = scan_kinds(CSRC, tmp, "this")
        parent = scan_kinds(a.parent_csrc, tmp, "parent") if a.parent_csrc else None
    for kind in sorted(here):
        lines.append(f"this tree   <{kind}>")
        lines += ["    " + x for x in here[kind]]
    moved = 0
    if parent is not None:
        for kind in sorted(parent):
            lines.append(f"parent      <{kind}>")
            lines += ["    " + x for x in parent[kind]]
            now = here.get(kind + ", false")
            same = now == parent[kind]
            moved += not same
            lines.append(f"    -> this tree's <{kind}, false>: {'identical figures' if same else 'DIFFERS'}")
        lines.append(f"# existing kinds that moved against the parent: {moved} of {len(parent)}")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(1 if moved else 0)


if __name__ == "__main__":
    main()
