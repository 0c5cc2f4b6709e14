"""VGPRs and scratch of the IN_F32_TRACK frame kernels beside their IN_F32_STEREO counterparts, from the product's own objects.

    python -m glava_amd.build && python tools/track_f32_isa.py [--out profiles/r13/track_f32_isa.txt]

Reads the gfx950 code objects bundled in glava_amd/csrc/build/glv_inst_<k>_<part>.o (parts 1 and 2 hold IN_F32_STEREO, part 4 IN_F32_TRACK), takes every
glv_frame_kernel's .vgpr_count and .private_segment_fixed_size from the code object's metadata note, and pairs the kernels that differ in the input mode
alone.  Needs no GPU.  Exit status 1 if a track kernel has scratch where its counterpart has none."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "glava_amd", "csrc", "build")
LLVM = os.environ.get("GLV_LLVM_BIN", "/opt/rocm/llvm/bin")
IN_F32_STEREO, IN_F32_TRACK = "3", "6"


def kernels(obj):
    """{template argument tuple: (vgprs, agprs, scratch bytes per lane)} of the glv_frame_kernel instantiations in one object"""
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "k.fatbin"), os.path.join(d, "k.co")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj, os.path.join(d, "rest.o")], capture_output=True)
        if not os.path.exists(fat):
            return {}                                                   # no device code (N = 256 has one configuration: its part 2 is empty)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat, "--output=" + co,
                        "--unbundle"], check=True)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    out = {}
    for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        block = ".agpr_count:" + block
        get = lambda k: re.search(r"\." + k + r":\s*'?([^\s']+)", block).group(1)      # noqa: E731
        sym = get("name")
        dem = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout
        m = re.search(r"glv_frame_kernel<(.*)>", dem)
        if not m:
            continue
        args = tuple(re.sub(r"\(.*?\)", "", a).strip() for a in m.group(1).split(","))
        out[args] = (int(get("vgpr_count")), int(get("agpr_count")), int(get("private_segment_fixed_size")))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r13", "track_f32_isa.txt"))
    a = ap.parse_args()
    lines = ["# glv_frame_kernel, gfx950: IN_F32_TRACK (6) beside the IN_F32_STEREO (3) kernel of the same size, configuration, log mode and class",
             "# template arguments: LOG_NN, IN_MODE, LOG_MODE, SLOTS, NBUF, TWREG, WINLDS, OCC, PREFETCH, TILTREG, LOG_E, CLASS (0 plain, 3 texel rows), WPRE",
             f"# {'N':>6} {'log':>3} {'slots':>5} {'E':>3} {'class':>5}   {'stereo vgpr':>11} {'scratch':>7}   {'track vgpr':>10} {'scratch':>7}   {'d vgpr':>6}"]
    bad = 0
    for k in range(7, 15):
        stereo = {}
        for part in (1, 2):
            stereo.update(kernels(os.path.join(OBJ, f"glv_inst_{k}_{part}.o")))
        track = kernels(os.path.join(OBJ, f"glv_inst_{k}_4.o"))
        for args, (v, _, s) in sorted(track.items()):
            assert args[1] == IN_F32_TRACK, args
            twin = stereo[args[:1] + (IN_F32_STEREO,) + args[2:]]
            new_scratch = s > 0 and twin[2] == 0
            bad += new_scratch
            lines.append(f"  {2 << int(args[0]):>6} {args[2]:>3} {args[3]:>5} {1 << int(args[10]):>3} {args[11]:>5}   {twin[0]:>11} {twin[2]:>7}   {v:>10} {s:>7}   {v - twin[0]:>+6}"
                         + ("   NEW SCRATCH" if new_scratch else ""))
    lines.append(f"# kernels with scratch where the counterpart has none: {bad}")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
