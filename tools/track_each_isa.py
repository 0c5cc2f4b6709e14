"""Have the existing kernels moved, and what do the per-stream track kinds cost?  tools/track_planar_isa.py's comparison -- the gfx950 device code of every
product object both trees have, .text and kernel descriptors byte for byte, against the parent commit's build, every object that differs compared kernel by
kernel -- then:

  * the frame kernel's per-stream table kinds (IN_S16_TRACK_EACH 10, IN_F32_TRACK_EACH 11, IN_F32_PLANAR_TRACK_EACH 12: parts 8, 9, 10 of glv_inst.hip) beside
    their shared-table twins (7, 8, 9: parts 5, 6, 7) of the same size, configuration, log mode and class.  A per-stream kind IS its twin with the table index
    taken modulo TrackWindows::table_len instead of TrackWindows::steps, so this table is also what folding the index into the twins would have cost them;
  * every kernel of glv_misc and glv_decimate that is new or differs from the parent's, and the scan kinds that existed, with registers, scratch, LDS and
    instruction counts in both trees (compiled to assembly from both source trees).

    python -m glava_amd.build && python tools/track_each_isa.py --parent-build DIR/glava_amd/csrc/build [--out profiles/r25/track_each_isa.txt]

Both trees must be built; the parent's sources are taken from beside its build directory.  Needs no GPU.  Exit status 1 if a frame kernel of the parent's has
moved or is gone, if an existing scan kind's registers, scratch or instruction count moved, or if a per-stream frame kind has scratch where its twin has none."""
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

WATCHED = r"glv_track_scan_kernel|glv_track_each_scan_kernel|glv_wave_kernel|glv_decimate_kernel"


def asm_kernels(csrc, unit, tmp, tag):
    """name -> (vgpr, sgpr, scratch, lds, instructions) of every kernel of a unit, from its device assembly"""
    asm = os.path.join(tmp, f"{unit}_{tag}.s")
    subprocess.run([_hipcc(), *HIPFLAGS, "--cuda-device-only", "-S", os.path.join(csrc, unit + ".hip"), "-o", asm], check=True, capture_output=True)
    text = open(asm).read()
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        g = lambda key: int((re.search(r"\.amdhsa_" + key + r" (\d+)", m.group(2)) or [None, "-1"])[1])    # noqa: E731
        body = re.search(r"^" + re.escape(m.group(1)) + r":[^\n]*\n(.*?)^\.Lfunc_end", text, re.S | re.M)
        count = sum(1 for l in body.group(1).split("\n") if re.match(r"\s+[a-z]", l) and not l.strip().startswith((".", ";"))) if body else -1
        out[m.group(1)] = (g("next_free_vgpr"), g("next_free_sgpr"), g("private_segment_fixed_size"), g("group_segment_fixed_size"), count)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-build", required=True, help="glava_amd/csrc/build of the tree to compare with, built")
    ap.add_argument("--out", default=os.path.join("profiles", "r25", "track_each_isa.txt"))
    a = ap.parse_args()
    parent_csrc = os.path.dirname(os.path.abspath(a.parent_build))
    lines = ["# device code of the product objects, gfx950: this tree against the parent commit's build.  Per object: .text and .rodata (kernel descriptors) bytes and",
             "# sha256[:16]; an object that differs as a whole is compared kernel by kernel, machine code and descriptor"]
    frame_moved = seen = identical = 0
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
            frame_moved += bad != 0 and name.startswith("glv_inst_")
        lines.append(f"# objects both trees have: {seen}; identical as a whole: {identical}; frame-kernel objects with a kernel of the parent's moved or gone: {frame_moved}")
        # the per-stream table kinds beside their shared-table twins
        lines += ["# glv_frame_kernel: the per-stream kinds (10, 11, 12) beside their shared-table twins (7, 8, 9), the same size, configuration, log mode and class (0 plain,",
                  "# 3 texel rows).  The per-stream kind is the twin with `f % table_len` in the place of `f % steps`: d vgpr / d scratch is what that operand costs",
                  f"# {'kind':>4} {'N':>6} {'log':>3} {'slots':>5} {'E':>3} {'class':>5}   {'twin vgpr':>9} {'sgpr':>5} {'scratch':>7}   {'each vgpr':>9} {'sgpr':>5} {'scratch':>7}   {'d vgpr':>6} {'d sgpr':>6} {'d scratch':>9}"]
        worse = grew = total = 0
        for twin_part, each_part, twin_kind, each_kind in ((5, 8, "7", "10"), (6, 9, "8", "11"), (7, 10, "9", "12")):
            for k in range(7, 15):
                twin = kernels(os.path.join(OBJ, f"glv_inst_{k}_{twin_part}.o"))
                each = kernels(os.path.join(OBJ, f"glv_inst_{k}_{each_part}.o"))
                for args, (v, sg, s) in sorted(each.items()):
                    assert args[1] == each_kind, args
                    tv, tsg, ts = twin[args[:1] + (twin_kind,) + args[2:]]
                    total += 1
                    worse += s > 0 and ts == 0
                    grew += v > tv or s > ts
                    lines.append(f"  {each_kind:>4} {2 << int(args[0]):>6} {args[2]:>3} {args[3]:>5} {1 << int(args[10]):>3} {args[11]:>5}   {tv:>9} {tsg:>5} {ts:>7}   {v:>9} {sg:>5} {s:>7}"
                                 f"   {v - tv:>+6} {sg - tsg:>+6} {s - ts:>+9}")
        lines.append(f"# per-stream frame kernels: {total}; with more VGPRs or scratch than the twin: {grew}; with scratch where the twin has none: {worse}")
        # the small units: what is new, what changed, and the scan kinds that existed
        lines += ["# glv_misc, glv_decimate: kernels that are new or whose assembly figures differ from the parent's, and every scan kind; from the device assembly of both",
                  "# source trees: VGPRs, SGPRs, scratch bytes, static LDS bytes, instructions (parent's in brackets)"]
        scan_moved = 0
        for unit in ("glv_misc", "glv_decimate"):
            mine, theirs = asm_kernels(CSRC, unit, tmp, "new"), asm_kernels(parent_csrc, unit, tmp, "parent")
            for k in sorted(mine):
                if not re.search(WATCHED, k): continue
                old = theirs.get(k)
                scan = "glv_track_scan_kernel" in k
                if old == mine[k] and not scan: continue
                v, sg, s, lds, ins = mine[k]
                was = "new in this tree" if old is None else "as the parent's" if old == mine[k] else f"MOVED: parent [VGPRs {old[0]} SGPRs {old[1]} scratch {old[2]} LDS {old[3]} instructions {old[4]}]"
                scan_moved += scan and old != mine[k]
                lines.append(f"    {unit}: {k}: VGPRs {v}  SGPRs {sg}  scratch {s} B  LDS {lds} B  instructions {ins}  {was}")
        lines.append(f"# scan kinds that existed and moved: {scan_moved}")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(1 if frame_moved or worse or scan_moved else 0)


if __name__ == "__main__":
    main()
