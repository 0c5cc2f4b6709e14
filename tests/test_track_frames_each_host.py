"""CPU: track mode at render frames per stream (glv_batch_track_each_frames_* / glv_batch_track_pool_frames_*) without a device -- the six exported symbols,
the ctypes mirror of glv_track_frames_each against the header field by field, glava_amd.track_starts.stack_frame_tables against the rows it stacks, the
refusals the vetting function makes before it reads anything of the batch, the shape of the host code (no second plan, no second executor), and the numpy
restatement of the per-stream clamp and zero-fill rule (tests/track_frames_each_lib.py) that tests/test_track_frames_each.py holds the kernels to."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from glava_amd.track_starts import keyframe_tables, live_session_frames, stack_frame_tables
from src_scan import ROOT, assert_launch_only, function_body, read_csrc, read_host_src, strip_comments
from track_frames_each_lib import clamp_each, keep_each, lerp_each

KINDS = ("s16", "f32", "f32_planar")
EACH = tuple("glv_batch_track_each_frames_" + k for k in KINDS)
POOL = tuple("glv_batch_track_pool_frames_" + k for k in KINDS)
F32 = np.float32


def _header():
    return strip_comments(open(os.path.join(ROOT, "include", "glv_spectrum.h")).read())


def test_the_six_symbols_are_exported_bound_and_declared(glvlib):
    L = C.CDLL(glvlib.LIB_PATH)
    lib = glvlib.lib()
    header = _header()
    for name in EACH + POOL:
        assert hasattr(L, name), name
        fn = getattr(lib, name)
        pool = name in POOL
        assert len(fn.argtypes) == (11 if pool else 10), name
        tb, fe = (4, 6) if pool else (3, 5)
        assert fn.argtypes[tb]._type_ is glvlib.TrackTables and fn.argtypes[fe]._type_ is glvlib.TrackFramesEach, name
        assert fn.argtypes[2] is (C.c_uint64 if pool else C.c_uint32), name
        decl = re.search(r"\nint " + name + r"\s*\(([^;]*)\);", header)
        assert decl, name
        args = [" ".join(a.split()) for a in decl.group(1).split(",")]
        assert len(args) == len(fn.argtypes), (name, args)
        assert args[tb] == "const glv_track_tables* tb" and args[tb + 1] == "uint32_t steps" and args[fe] == "const glv_track_frames_each* fe", (name, args)
        if pool: assert args[2] == "uint64_t pool_frames" and args[3] == "const glv_track_span* d_spans", (name, args)
    for kind in KINDS:
        assert callable(getattr(glvlib.Batch, "track_each_frames_" + kind)) and callable(getattr(glvlib.Batch, "track_pool_frames_" + kind)), kind
    assert lib.glv_abi_version() == 7                                            # added within the ABI: detected by the symbol
    for absent in ("glv_batch_track_each_frames_work_bytes", "glv_batch_track_pool_frames_work_bytes", "glv_batch_track_frames_each_work_bytes"):
        assert not hasattr(L, absent), absent                                    # sized by glv_batch_track_frames_work_bytes: there is no other query
    assert "work_bytes" not in "".join(re.findall(r"\n\w+ (glv_batch_track_(?:each|pool)_frames\w*)\(", header))


def test_the_mirror_is_the_header_s_structure_field_by_field(glvlib):
    body = re.search(r"typedef struct glv_track_frames_each \{(.*?)\} glv_track_frames_each;", _header(), re.S)
    assert body
    fields = [tuple(" ".join(line.split()).rsplit(" ", 1)) for line in body.group(1).split(";") if line.strip()]
    assert fields == [("const uint32_t*", "d_from"), ("const uint32_t*", "d_to"), ("const float*", "d_mod"), ("const uint32_t*", "d_frame_counts"),
                      ("const uint32_t*", "d_keep"), ("uint32_t", "frames"), ("float*", "d_keys")]
    T = glvlib.TrackFramesEach
    assert [n for n, _ in T._fields_] == [n for _, n in fields]
    for (ctext, name), (_, ctype) in zip(fields, T._fields_):
        assert ctype is (C.c_uint32 if ctext == "uint32_t" else C.c_void_p), name
    offsets = dict(d_from=0, d_to=8, d_mod=16, d_frame_counts=24, d_keep=32, frames=40, d_keys=48)
    assert {n: getattr(T, n).offset for n in offsets} == offsets
    assert C.sizeof(T) == 56 and C.alignment(T) == 8
    # the lockstep structure keeps its layout, and the device side's TrackFrames its members: the per-stream operands have a structure of their own
    assert C.sizeof(glvlib.TrackFrames) == 48
    launch = strip_comments(read_csrc("glv_launch.h"))
    assert "struct TrackFrames {\n    const uint32_t* from; const uint32_t* to; const float* mod;\n    const float* keys; const float* rows;\n    void* out;\n" \
           "    uint32_t frames, steps, units, n, limit, segment;\n};" in launch
    assert re.search(r"struct TrackFramesEach \{\s*TrackFrames t;\s*const uint32_t\* frame_counts;\s*const uint32_t\* counts;\s*\};", launch)


# ---- stack_frame_tables ---------------------------------------------------------------------------------------------------------------------------------------
def test_stack_frame_tables_pads_ragged_rows_and_counts_them():
    a = live_session_frames(22050, 60, 150, 256)[2:]                              # a 60 Hz display: never interpolates
    b = live_session_frames(22050, 144, 330, 256)[2:]                             # a 144 Hz display on the same recording: does, from its second second on
    c = keyframe_tables([True, False, True], [True] * 3, [0.4] * 3)
    empty = ([], [], [], 0, 1)
    rows = [a, b, c, empty]
    frm, to, mod, counts, keep = stack_frame_tables(rows)
    assert frm.dtype == to.dtype == counts.dtype == keep.dtype == np.uint32 and mod.dtype == np.float32
    assert frm.shape == to.shape == mod.shape == (4, 330) and counts.tolist() == [150, 330, 3, 0] and keep.shape == (4, 2)
    for i, (f, t, m, kf, kt) in enumerate(rows):
        k = len(f)
        assert frm[i, :k].tolist() == f and to[i, :k].tolist() == t and mod[i, :k].tolist() == [float(F32(v)) for v in m], i
        assert not frm[i, k:].any() and not to[i, k:].any() and not mod[i, k:].any(), i      # the padding: never read, defined all the same
        assert keep[i].tolist() == [kf, kt], i
    assert (a[0], a[1]) != (b[0][:150], b[1][:150]) and (a[3], a[4]) != (b[3], b[4])       # listeners at different display rates do differ: tables and keep pairs
    assert keep[3].tolist() == [0, 1]
    # a longer common length, and a batch of empty rows only
    frm2, _, _, counts2, _ = stack_frame_tables(rows, frames=400)
    assert frm2.shape == (4, 400) and counts2.tolist() == counts.tolist() and (frm2[:, :330] == frm).all() and not frm2[:, 330:].any()
    only = stack_frame_tables([empty, empty])
    assert only[0].shape == (2, 1) and only[3].tolist() == [0, 0]                # `frames` of a call is at least 1
    # generators and numpy integers are taken
    g = stack_frame_tables([(iter([1, 2]), np.asarray([2, 3], dtype=np.uint32), (v for v in (0.5, 1.0)), np.uint32(1), 3)])
    assert g[0].tolist() == [[1, 2]] and g[1].tolist() == [[2, 3]] and g[4].tolist() == [[1, 3]]


def test_stack_frame_tables_refuses_malformed_rows():
    ok = ([0, 1], [1, 2], [0.5, 1.0], 1, 2)
    for bad in ([], [([0], [1, 2], [0.5], 0, 1)], [([0], [1], [0.5, 0.1], 0, 1)], [([-1], [1], [0.5], 0, 1)], [([0], [1 << 32], [0.5], 0, 1)], [([0], [1], [0.5], 0, 1 << 32)],
                [([0], [1], [0.5], -1, 1)], [([0.5], [1], [0.5], 0, 1)], [([True], [1], [0.5], 0, 1)]):
        with pytest.raises(ValueError):
            stack_frame_tables(bad)
    with pytest.raises(ValueError):
        stack_frame_tables([ok], frames=1)
    for frames in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            stack_frame_tables([ok], frames=frames)


# ---- the refusals that need no device ---------------------------------------------------------------------------------------------------------------------------
def test_the_vetting_function_refuses_before_it_reads_the_batch(glvlib):
    """a handle that is no batch: every refusal below is made before anything of the batch is read, which the shape test pins in the source"""
    lib = glvlib.lib()
    handle = C.create_string_buffer(1 << 16)
    store = C.create_string_buffer(1024)                                          # addresses to aim pointers at: nothing is dereferenced
    base = (C.addressof(store) + 63) & ~63
    tb = glvlib.TrackTables(base, None, None)
    ops = glvlib.OP_FFT | glvlib.OP_R16

    def fe(**kw):
        f = dict(d_from=base, d_to=base + 64, d_mod=base + 128, d_frame_counts=base + 192, d_keep=base + 256, frames=5, d_keys=base + 320)
        f.update(kw)
        return glvlib.TrackFramesEach(*(f[n] for n, _ in glvlib.TrackFramesEach._fields_))

    cases = [("fe is NULL", None), ("NULL device pointer in glv_track_frames_each", fe(d_from=None)), ("NULL device pointer in glv_track_frames_each", fe(d_to=None)),
             ("NULL device pointer in glv_track_frames_each", fe(d_mod=None)), ("NULL device pointer in glv_track_frames_each", fe(d_keep=None)),
             ("NULL device pointer in glv_track_frames_each", fe(d_keys=None)), ("4-byte aligned", fe(d_from=base + 2)), ("4-byte aligned", fe(d_to=base + 65)),
             ("4-byte aligned", fe(d_mod=base + 130)), ("4-byte aligned", fe(d_frame_counts=base + 193)), ("4-byte aligned", fe(d_keep=base + 258)),
             ("d_keys must be 16-byte aligned", fe(d_keys=base + 324)), ("frames must be > 0", fe(frames=0))]
    for name in EACH + POOL:
        head = (handle, base, 1 << 20, base, C.byref(tb), 3) if name in POOL else (handle, base, 1 << 20, C.byref(tb), 3)
        for message, s in cases:
            assert getattr(lib, name)(*head, C.byref(s) if s is not None else None, base, base, ops, None) == glvlib.ERR_INVALID, (name, message)
            assert message in lib.glv_last_error().decode(), (name, message, lib.glv_last_error().decode())
        # a structure that is not aligned like a pointer
        raw = C.create_string_buffer(C.sizeof(glvlib.TrackFramesEach) + 16)
        at = ((C.addressof(raw) + 7) & ~7) + 4
        C.memmove(at, C.byref(fe()), C.sizeof(glvlib.TrackFramesEach))
        assert getattr(lib, name)(*head, C.cast(at, C.POINTER(glvlib.TrackFramesEach)), base, base, ops, None) == glvlib.ERR_INVALID, name
        assert "aligned like a pointer" in lib.glv_last_error().decode(), name
        # the wave form has no per-stream frames
        assert getattr(lib, name)(*head, C.byref(fe()), base, base, glvlib.OP_WAVE | glvlib.OP_R16, None) == glvlib.ERR_INVALID, name
        assert "GLV_OP_WAVE" in lib.glv_last_error().decode(), name
        # a NULL batch, and d_frame_counts NULL is no refusal of its own: the next one in line answers (the per-stream call's NULL tb)
        assert getattr(lib, name)(None, *head[1:], C.byref(fe()), base, base, ops, None) == glvlib.ERR_INVALID, name
        assert "batch is NULL" in lib.glv_last_error().decode(), name
        if name in EACH:                                                          # (the pool call looks at the batch's window first)
            assert getattr(lib, name)(*head[:-2], None, 3, C.byref(fe(d_frame_counts=None)), base, base, ops, None) == glvlib.ERR_INVALID, name
            assert "tb is NULL" in lib.glv_last_error().decode(), (name, lib.glv_last_error().decode())
    assert not any(handle.raw), "a refusal wrote to the handle"


def test_the_entries_add_one_vetting_function_and_no_plan_or_executor():
    raw = read_host_src()
    assert_launch_only(raw, [r"\nint track_each_frames_call\("] + [r"\nint " + name + r"\(" for name in EACH + POOL])
    src = strip_comments(raw)
    for name in EACH + POOL:
        body = function_body(src, r"\nint " + name + r"\(")
        assert "track_each_frames_call(b, " in body and "glv::launch_" not in body and "for (" not in body and "TrackPlan" not in body, name
    body = function_body(src, r"\nint track_each_frames_call\(")
    for absent in ("glv::launch_", "for (", "while (", "TrackPlan", "plan_track", "hipSetDevice", "b->"):
        assert absent not in body, absent                                        # nothing of the batch is read, let alone written, before the plan accepts the call
    order = ["!b", "!fe", "alignof(glv_track_frames_each)", "ops & GLV_OP_WAVE", "!fe->d_from || !fe->d_to || !fe->d_mod || !fe->d_keep || !fe->d_keys", "& 3u", "& 15u",
             "fe->frames == 0", "track_pool(b, d_pcm,", "track_each(b, d_pcm,"]
    at = [body.index(s) for s in order]
    assert at == sorted(at), order
    assert "d_frame_counts" not in body[:body.index("& 3u")].split("!fe->d_from")[1].split(")")[0]       # the one pointer that may be NULL
    # one plan, one executor, one frames stage: the frames travel in TrackInput through the pool call and the per-stream call into the table call
    for once in ("int plan_track_frames(", "int track_frames(glv_batch* b,", "int track(glv_batch* b,", "int track_at(glv_batch* b,", "int track_each(glv_batch* b,",
                 "int track_pool(glv_batch* b,", "struct TrackPlan {"):
        assert src.count(once) == 1, once
    assert "const glv_track_frames_each* frames" in src[src.index("struct TrackInput"):src.index("struct TrackPlan")]
    assert "const glv_track_frames_each* fe" in src[src.index("struct TrackPlan"):src.index("uint64_t window_frames(")]
    at_body = function_body(src, r"\nint track_at\(glv_batch\* b,")
    assert "f32.frames" in at_body and "tp.fe = fe" in at_body and "plan_track_frames(b, pitch_frames, steps, ops, tp)" in at_body
    stage = function_body(src, r"\nint track_frames\(glv_batch\* b,")
    assert stage.count("glv::launch_track_frames_each(") == 1 and stage.count("glv::launch_track_keys_each(") == 1 and stage.count("++b->last_launches") == 2
    assert "tp.counts" in stage and "tp.fe->d_frame_counts" in stage and "tp.fe->d_keep" in stage and "b->track_frames_segment" in stage
    assert '"glv_track_frames_each_kernel"' in function_body(src, r"\nint track\(glv_batch\* b,")
    assert "tp.fe" not in function_body(src, r"\nint plan_track_frames\(")          # the plan needs `frames` alone


def test_the_kernels_are_new_and_the_old_ones_keep_their_source():
    unit = read_csrc("glv_track_frames.hip")
    assert_launch_only(unit, [r"\nhipError_t launch_track_frames_each\(", r"\nhipError_t launch_track_keys_each\("])
    each = strip_comments(function_body(unit, r"glv_track_frames_each_kernel\(const TrackFrames t,"))
    base = strip_comments(function_body(unit, r"glv_track_frames_kernel\(const TrackFrames t,"))
    for shared in ("item += gridDim.x", "w = s + ((e - s) * m)", "pack_unorm16(", "if (kf != ks) ns = kf == ke ? e : key(kf);", "if (kt != ke) e = kt == ks ? s : key(kt);"):
        assert shared in each and shared in base, shared
    assert "__builtin_fmaf" not in each and "fma(" not in each and "asm" not in each
    assert each.count("< last_key ? ") == 2 and each.count("key(k") == 2         # every index a table holds is clamped where it is taken, before any keyframe is loaded
    assert "const uint32_t stream = row >> 1;" in each and "(size_t) stream * t.frames" in each
    assert "counts[stream]" in each and "frame_counts[stream]" in each and "const uint32_t last_key = c + 1u;" in each
    assert "for (uint32_t j = jw; j < j1; ++j)" in each and "glv_u2{ 0u, 0u }" in each                    # zeros behind the stream's frame count
    assert "if (jw - j > (uint32_t) kFramesDepth)" in each and "(uint32_t) d < jw - j0" in each           # no table entry at j >= f_s is requested
    assert "t.from[" not in each and "t.to[" not in each and "t.mod[" not in each                         # the tables come as __restrict__ arguments: uniform loads
    assert "last_key = t.steps + 1u" in base and "t.from[j + (uint32_t) kFramesDepth]" in base            # the lockstep kernel as it was
    keys = strip_comments(function_body(unit, r"glv_track_keys_each_kernel\(float\* keys,"))
    assert keys.count("< last_key ? ") == 2 and "const glv_f4 va = a[i], vb = b[i];" in keys and keys.index("vb = b[i]") < keys.index("k0[i] = va")
    from glava_amd import build as B
    assert "glv_track_frames" in B.SMALL and "-ffp-contract=off" in B.HIPFLAGS


# ---- the rule, in numpy -----------------------------------------------------------------------------------------------------------------------------------------
def test_the_numpy_rule_on_hand_computed_cases():
    steps, n = 4, 4
    rng = np.random.default_rng(3)
    keys = rng.random((2, 6, n), dtype=np.float32)
    rows = rng.random((steps, 6, n), dtype=np.float32) + F32(2.0)                # rows beyond a stream's count are told apart from its keys
    counts, fcounts = [4, 2, 0], [5, 3, 0]
    big = 0xFFFFFFFF
    frm = [[0, 1, 2, 5, big], [0, 3, 4, 9, 9], [0, 2, big, 1, 1]]
    to = [[1, 2, 3, 5, 5], [1, 4, big, 9, 9], [1, 1, 1, big, 0]]
    mod = np.asarray([[0.5, 0.25, 1.0, 0.7, 0.1]] * 3, dtype=np.float32)
    assert clamp_each(frm, counts, steps).tolist() == [[0, 1, 2, 5, 5], [0, 3, 3, 3, 3], [0, 1, 1, 1, 1]]
    assert clamp_each([[5, 9]], None or [7], 4).tolist() == [[5, 5]]             # a count above `steps` is `steps`
    w, shown = lerp_each(keys, rows, frm, to, mod, counts, fcounts, steps)
    assert shown.tolist() == [[True, True, False], [True, True, False], [True, True, False], [True, False, False], [True, False, False]]
    lerp = lambda s, e, m: (s + ((e - s).astype(F32) * F32(m)).astype(F32)).astype(F32)      # noqa: E731
    # stream 0, all four steps: plain lerps; (5, 5) is the last step's row itself
    assert (w[0, 0:2] == lerp(keys[0, 0:2], keys[1, 0:2], 0.5)).all() and (w[2, 0:2] == lerp(rows[0, 0:2], rows[1, 0:2], 1.0)).all()
    assert (w[3, 0:2] == rows[3, 0:2]).all() and (w[4, 0:2] == rows[3, 0:2]).all()                    # big clamps to 5 == to: the keyframe's own bits
    # stream 1, two steps: 4 and big clamp to c + 1 = 3, the row of step 1 -- never step 2's or step 3's, which the scan zero-fills
    assert (w[1, 2:4] == rows[1, 2:4]).all() and (w[2, 2:4] == rows[1, 2:4]).all()
    assert not w[3:, 2:4].any()                                                   # behind its three frames
    # stream 2, no step and no frame: nothing shown; with frames it would lerp between its two carried keyframes only
    assert not w[:, 4:6].any()
    w2, shown2 = lerp_each(keys, rows, frm, to, mod, counts, None, steps)
    assert shown2.all() and (w2[1, 4:6] == keys[1, 4:6]).all() and (w2[2, 4:6] == keys[1, 4:6]).all() and (w2[4, 4:6] == lerp(keys[1, 4:6], keys[0, 4:6], 0.1)).all()
    assert (w2[:3, 0:4] == w[:3, 0:4]).all()
    # NULL counts: every stream takes every step
    w3, _ = lerp_each(keys, rows, frm, to, mod, None, None, steps)
    assert (w3[1, 2:4] == lerp(rows[1, 2:4], rows[2, 2:4], 0.25)).all() and (w3[3, 2:4] == rows[3, 2:4]).all()
    # the write-back: both read before either is written, per stream, clamped
    after = keep_each(keys, rows, [[1, 0], [2, big], [big, 3]], counts, steps)
    assert (after[0, 0:2] == keys[1, 0:2]).all() and (after[1, 0:2] == keys[0, 0:2]).all()          # swapped
    assert (after[0, 2:4] == rows[0, 2:4]).all() and (after[1, 2:4] == rows[1, 2:4]).all()          # big -> c + 1 = 3
    assert (after[0, 4:6] == keys[1, 4:6]).all() and (after[1, 4:6] == keys[1, 4:6]).all()          # c = 0: both clamp to 1
    same = keep_each(keys, rows, [[0, 1]] * 3, counts, steps)
    assert (same == keys).all()
