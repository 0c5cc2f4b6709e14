"""Have the existing kernels moved, and what do the per-stream wave frames kernels take?  tools/track_frames_each_isa.py's comparison, as it is -- the gfx950
device code of every product object both trees have against the parent commit's build, an object that differs compared kernel by kernel (glv_track_frames differs
as a whole: the per-stream wave kernels were added to it) -- with the wave module's kernels of glv_track_frames.hip listed behind it: registers, scratch, LDS,
instruction counts and memory instructions of every kind of glv_wave_frames_each_kernel and glv_wave_keys_each_kernel (input kind, each-or-pool, texels-or-floats)
beside glv_wave_frames_kernel / glv_wave_keys_kernel and their planar copies.

    python -m glava_amd.build && python tools/track_wave_frames_each_isa.py --parent-build DIR/glava_amd/csrc/build [--out profiles/r28/track_wave_frames_each_isa.txt]

Both trees must be built; the parent's sources are taken from beside its build directory.  Needs no GPU.  Exit status 1 if an object or kernel of the parent's
has moved or is gone."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_frames_each_isa as base  # noqa: E402

base.WATCHED = r"glv_wave_frames_kernel|glv_wave_keys_kernel|glv_wave_frames_planar_kernel|glv_wave_keys_planar_kernel|glv_wave_frames_each_kernel|glv_wave_keys_each_kernel"

if __name__ == "__main__":
    if not any(arg.startswith("--out") for arg in sys.argv[1:]):
        sys.argv += ["--out", os.path.join("profiles", "r28", "track_wave_frames_each_isa.txt")]
    base.main()
