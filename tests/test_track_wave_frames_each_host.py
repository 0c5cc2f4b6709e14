"""CPU: track mode at render frames per stream for the wave module (glv_batch_track_each_wave_frames_* / glv_batch_track_pool_wave_frames_*) without a device --
the six exported symbols against the header and the ctypes prototypes, the refusals the vetting function makes before it reads anything of the batch, the shape
of the host code (one vetting function, one stage, no second plan) and of the two new kernels, and the numpy restatement of the rule
(tests/track_wave_frames_each_lib.py) that tests/test_track_wave_frames_each.py holds the kernels to, on hand-computed cases."""
import ctypes as C
import os
import re

import numpy as np

from glava_amd.track_starts import pool_window_start
from src_scan import ROOT, assert_launch_only, function_body, read_csrc, read_host_src, strip_comments
from track_wave_frames_each_lib import clamp_each, each_starts, keep_each, lerp_each, pool_starts, rows_each

KINDS = ("s16", "f32", "f32_planar")
EACH = tuple("glv_batch_track_each_wave_frames_" + k for k in KINDS)
POOL = tuple("glv_batch_track_pool_wave_frames_" + k for k in KINDS)
F32 = np.float32
BIG = 0xFFFFFFFF


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
        sibling = getattr(lib, name.replace("_wave_frames_", "_frames_"))
        assert list(fn.argtypes) == list(sibling.argtypes) and len(fn.argtypes) == (11 if pool else 10), name      # the FFT sibling's argument list, exactly
        tb, fe = (4, 6) if pool else (3, 5)
        assert fn.argtypes[tb]._type_ is glvlib.TrackTables and fn.argtypes[fe]._type_ is glvlib.TrackFramesEach, name
        assert fn.argtypes[2] is (C.c_uint64 if pool else C.c_uint32), name
        decl = re.search(r"\nint " + name + r"\s*\(([^;]*)\);", header)
        twin = re.search(r"\nint " + name.replace("_wave_frames_", "_frames_") + r"\s*\(([^;]*)\);", header)
        assert decl and twin, name
        args = [" ".join(a.split()) for a in decl.group(1).split(",")]
        assert args == [" ".join(a.split()) for a in twin.group(1).split(",")] and len(args) == len(fn.argtypes), (name, args)
    for kind in KINDS:
        assert callable(getattr(glvlib.Batch, "track_each_wave_frames_" + kind)) and callable(getattr(glvlib.Batch, "track_pool_wave_frames_" + kind)), kind
    assert lib.glv_abi_version() == 7                                            # added within the ABI: detected by the symbol
    for absent in ("glv_batch_track_each_wave_frames_work_bytes", "glv_batch_track_pool_wave_frames_work_bytes", "glv_batch_track_wave_frames_each_work_bytes"):
        assert not hasattr(L, absent), absent                                    # sized by glv_batch_track_wave_frames_work_bytes: there is no other query
    assert "work_bytes" not in "".join(re.findall(r"\n\w+ (glv_batch_track_(?:each|pool)_wave_frames\w*)\(", header))


def test_the_vetting_function_refuses_before_it_reads_the_batch(glvlib):
    """a handle that is no batch: every refusal below is made before anything of the batch is read, which the shape test pins in the source"""
    lib = glvlib.lib()
    handle = C.create_string_buffer(1 << 16)
    store = C.create_string_buffer(1024)                                          # addresses to aim pointers at: nothing is dereferenced
    base = (C.addressof(store) + 63) & ~63
    tb = glvlib.TrackTables(base, None, None)
    rated = glvlib.TrackTables(base, base + 384, None)
    ops = glvlib.OP_WAVE | glvlib.OP_R16

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
        call = getattr(lib, name)
        for message, s in cases:
            assert call(*head, C.byref(s) if s is not None else None, base, base, ops, None) == glvlib.ERR_INVALID, (name, message)
            assert message in lib.glv_last_error().decode(), (name, message, lib.glv_last_error().decode())
        # a structure that is not aligned like a pointer
        raw = C.create_string_buffer(C.sizeof(glvlib.TrackFramesEach) + 16)
        at = ((C.addressof(raw) + 7) & ~7) + 4
        C.memmove(at, C.byref(fe()), C.sizeof(glvlib.TrackFramesEach))
        assert call(*head, C.cast(at, C.POINTER(glvlib.TrackFramesEach)), base, base, ops, None) == glvlib.ERR_INVALID, name
        assert "aligned like a pointer" in lib.glv_last_error().decode(), name
        # ops without GLV_OP_WAVE: the message names the FFT entries
        for chain in (glvlib.OP_FFT | glvlib.OP_R16, glvlib.OP_BARS | glvlib.OP_R16, 0):
            assert call(*head, C.byref(fe()), base, base, chain, None) == glvlib.ERR_INVALID, name
            assert "glv_batch_track_each_frames_*" in lib.glv_last_error().decode() and "GLV_OP_WAVE" in lib.glv_last_error().decode(), name
        # a NULL batch; a NULL tb (d_frame_counts NULL is no refusal of its own: the next one in line answers)
        assert call(None, *head[1:], C.byref(fe()), base, base, ops, None) == glvlib.ERR_INVALID, name
        assert "batch is NULL" in lib.glv_last_error().decode(), name
        if name in EACH:                                                          # (the pool call looks at the batch's window first)
            assert call(*head[:-2], None, 3, C.byref(fe(d_frame_counts=None)), base, base, ops, None) == glvlib.ERR_INVALID, name
            assert "tb is NULL" in lib.glv_last_error().decode(), (name, lib.glv_last_error().decode())
            # a rate table: refused in the per-stream call's words
            assert call(*head[:-2], C.byref(rated), 3, C.byref(fe()), base, base, ops, None) == glvlib.ERR_INVALID, name
            assert "GLV_OP_WAVE is stateless: no gravity reads the rate table" in lib.glv_last_error().decode(), (name, lib.glv_last_error().decode())
    assert not any(handle.raw), "a refusal wrote to the handle"


def test_the_entries_add_one_vetting_function_one_stage_and_no_plan():
    raw = read_host_src()
    assert_launch_only(raw, [r"\nint track_each_wave_frames_call\(", r"\nint track_wave_each_frames\(glv_batch\* b,", r"\nint track_wave\(glv_batch\* b,",
                             r"\nint track_each\(glv_batch\* b,", r"\nint track_pool\(glv_batch\* b,"] + [r"\nint " + name + r"\(" for name in EACH + POOL])
    src = strip_comments(raw)
    for name in EACH + POOL:
        body = function_body(src, r"\nint " + name + r"\(")
        assert "track_each_wave_frames_call(b, " in body and "glv::launch_" not in body and "for (" not in body and "TrackWavePlan" not in body, name
    body = function_body(src, r"\nint track_each_wave_frames_call\(")
    for absent in ("glv::launch_", "for (", "while (", "TrackPlan", "TrackWavePlan", "plan_track", "hipSetDevice", "b->"):
        assert absent not in body, absent                                        # nothing of the batch is read, let alone written, before the plan accepts the call
    order = ["!b", "!fe", "alignof(glv_track_frames_each)", "!(ops & GLV_OP_WAVE)", "!fe->d_from || !fe->d_to || !fe->d_mod || !fe->d_keep || !fe->d_keys", "& 3u", "& 15u",
             "fe->frames == 0", "track_pool(b, d_pcm,", "track_each(b, d_pcm,"]
    at = [body.index(s) for s in order]
    assert at == sorted(at), order
    # one plan, one executor: the frames travel in TrackInput through the pool call and the per-stream call into the table call's wave executor
    for once in ("int plan_track_wave(", "int track_wave(", "int track_wave_each_frames(glv_batch* b,", "int track_each_wave_frames_call(", "struct TrackWavePlan {"):
        assert src.count(once) == 1, once
    wave = function_body(src, r"\nint track_wave\(glv_batch\* b,")
    assert wave.count("track_wave_each_frames(b, tp,") == 1 and wave.count("plan_track_wave(") == 1 and "shape.frames = f32.frames->frames" in wave
    assert wave.index("track_wave_each_frames(b, tp,") < wave.index("launch_bars_pass(") and '"glv_wave_frames_each_kernel"' in wave
    stage = function_body(src, r"\nint track_wave_each_frames\(glv_batch\* b,")
    assert stage.count("glv::launch_wave_each_frames(") == 1 and stage.count("glv::launch_wave_each_keys(") == 1 and stage.count("++b->last_launches") == 2
    assert src.count("launch_wave_each_frames(") == 1 and src.count("launch_wave_each_keys(") == 1
    for used in ("in.counts", "fe.d_frame_counts", "fe.d_keep", "in.pool", "b->track_frames_segment", "glv::track_frames_segment(", "tp.pl.wave_limit", "tp.pl.wave_r16"):
        assert used in stage, used
    assert "for (" not in stage and "while (" not in stage
    # the counts reach the kernels; every other wave call keeps its refusal of them
    each = function_body(src, r"\nint track_each\(glv_batch\* b,")
    assert "f32.counts = tb->d_counts" in each and "f32.frames && (ops & GLV_OP_WAVE)" in each
    assert "the chain keeps no state for d_counts to protect" in each
    # the FFT entries keep refusing the wave module, and say where it went
    fft = function_body(src, r"\nint track_each_frames_call\(")
    assert "GLV_OP_WAVE" in fft and "glv_batch_track_each_wave_frames_*" in fft


def test_the_kernels_are_new_and_the_old_ones_keep_their_source():
    unit = read_csrc("glv_track_frames.hip")
    assert_launch_only(unit, [r"\nhipError_t launch_wave_each_frames\(", r"\nhipError_t launch_wave_each_keys\("])
    plain = strip_comments(unit)
    assert "asm" not in plain and "fma" not in plain
    each = strip_comments(function_body(unit, r"glv_wave_frames_each_kernel\(const void\* pcm,"))
    base = strip_comments(function_body(unit, r"glv_wave_frames_kernel\(const void\* pcm,"))
    for shared in ("item += gridDim.x", "wl = sl + ((el - sl) * m)", "wr = sr + ((er - sr) * m)", "pack_unorm16(", "unorm16_to_float(", "if (kf == ke) { nl = el; nr = er; }",
                   "if (kt == ks) { el = sl; er = sr; }"):
        assert shared in each and shared in base, shared
    assert each.count("< last_key ? ") == 2 and each.count("key(k") == 2          # every index a table holds is clamped where it is taken, before any keyframe is loaded
    assert "counts[stream]" in each and "frame_counts[stream]" in each and "const uint32_t last_key = c + 1u;" in each and "(size_t) stream * t.frames" in each
    assert "for (uint32_t j = jw; j < j1; ++j)" in each and "glv_u2{ 0u, 0u }" in each and "glv_f4{ 0.0f, 0.0f, 0.0f, 0.0f }" in each      # zeros behind the frame count
    assert "if (jw - j > (uint32_t) kFramesDepth)" in each and "(uint32_t) d < jw - j0" in each          # no table entry at j >= f_s is requested
    assert "t.from[" not in each and "t.to[" not in each and "t.mod[" not in each and "w.starts[" not in each      # the tables come as __restrict__ arguments
    head = unit[unit.index("glv_wave_frames_each_kernel(const void* pcm,"):]
    head = head[:head.index("{")]
    for table in ("tfrom", "tto", "tmod", "frame_counts", "counts", "starts", "spans"):
        assert re.search(r"const \w+\* __restrict__ " + table + r"\b", head), table
    keys = strip_comments(function_body(unit, r"glv_wave_keys_each_kernel\(const void\* pcm,"))
    assert keys.count("< last_key ? ") == 2 and keys.count("wave_each_key<KIND, POOL>(") == 2 and "counts[stream]" in keys and "keep[2u * stream]" in keys
    assert keys.index("kt, stream, i") < keys.index("= al;")                      # both kept keyframes are read before either is written
    key = strip_comments(function_body(unit, r"void wave_each_key\(const void\* pcm,"))
    for reused in ("pool_window_start(", "wave_window_start(w, stream, step, entry)", "starts[(size_t) stream * w.steps + step]", "unpack_s16_mono(", "unpack_s16(",
                   "+ 1.0f) / 2.0f", "& 15u"):
        assert reused in key, reused
    assert key.index("if (k < 2u)") < key.index("starts[") < key.index("spans + stream")      # a stream without steps reads neither its starts nor its span
    assert strip_comments(read_csrc("glv_frame.h")).count("uint64_t pool_window_start(") == 1 and "uint64_t pool_window_start(" not in plain      # the rule is not restated
    # the lockstep kernels and wave_key as they were
    assert "const uint32_t last_key = w.steps + 1u;" in base and "t.from[j + (uint32_t) kFramesDepth]" in base and base.count("wave_key<F32_IN>(") == 2
    old = strip_comments(function_body(unit, r"void wave_key\(const void\* pcm,"))
    assert "wave_window_start(w, stream, step, w.starts[step])" in old and "spans" not in old and "counts" not in old
    from glava_amd import build as B
    assert "glv_track_frames" in B.SMALL and "-ffp-contract=off" in B.HIPFLAGS


# ---- the rule, in numpy -----------------------------------------------------------------------------------------------------------------------------------------
def test_the_numpy_rule_on_hand_computed_cases():
    n, steps, pitch = 4, 4, 12
    x = (np.arange(3 * pitch * 2, dtype=np.int16).reshape(3, pitch, 2) * 517 - 9000).astype(np.int16)
    starts = [[0, 3, 8, BIG], [5, 5, 1, 0], [BIG, BIG, BIG, BIG]]
    counts, fcounts = [4, 2, 0], [5, 3, 2]
    where = each_starts(starts, pitch, n)
    assert where.tolist() == [[0, 3, 8, 8], [5, 5, 1, 0], [8, 8, 8, 8]]             # 0xFFFFFFFF clamps to the recording's last window
    rows = rows_each(list(x), where, counts, n, False, 2)
    assert rows.shape == (steps, 6, n)
    wr = lambda v: ((F32(v) / F32(65535) + F32(1)) / F32(2))                      # noqa: E731  (unpack, + 1.0F, / 2.0F: each rounded to float32)
    assert rows[1, 0, 2] == wr(x[0, 5, 0]) and rows[1, 1, 2] == wr(x[0, 5, 1]) and rows[3, 0, 0] == wr(x[0, 8, 0]) and rows[0, 2, 3] == wr(x[1, 8, 0])
    assert np.isnan(rows[2:, 2:4]).all() and np.isnan(rows[:, 4:6]).all() and not np.isnan(rows[:2, 2:4]).any()      # no keyframe behind a stream's count
    keys = np.random.default_rng(5).random((2, 6, n), dtype=np.float32) + F32(2.0)  # told apart from every wave keyframe, which lies in [0, 1]
    frm = [[0, 1, 2, 5, BIG], [0, 3, 4, 9, 9], [0, 2, BIG, 1, 1]]
    to = [[1, 2, 3, 5, 5], [1, 4, BIG, 9, 9], [1, 1, 1, BIG, 0]]
    mod = np.asarray([[0.5, 0.25, 1.0, 0.7, 0.1]] * 3, dtype=np.float32)
    assert clamp_each(frm, counts, steps).tolist() == [[0, 1, 2, 5, 5], [0, 3, 3, 3, 3], [0, 1, 1, 1, 1]]
    w, shown = lerp_each(keys, rows, frm, to, mod, counts, fcounts, steps)
    assert shown.tolist() == [[True, True, True], [True, True, True], [True, True, False], [True, False, False], [True, False, False]]
    assert not np.isnan(w).any()                                                   # no index reached a step behind a count
    lerp = lambda s, e, m: (s + ((e - s).astype(F32) * F32(m)).astype(F32)).astype(F32)      # noqa: E731
    assert (w[0, 0:2] == lerp(keys[0, 0:2], keys[1, 0:2], 0.5)).all() and (w[2, 0:2] == lerp(rows[0, 0:2], rows[1, 0:2], 1.0)).all()
    assert (w[3, 0:2] == rows[3, 0:2]).all() and (w[4, 0:2] == rows[3, 0:2]).all()  # 0xFFFFFFFF clamps to 5 == to: the keyframe's own bits
    assert (w[1, 2:4] == rows[1, 2:4]).all() and (w[2, 2:4] == rows[1, 2:4]).all() and not w[3:, 2:4].any()      # c = 2: 4 and 0xFFFFFFFF are keyframe 3
    # c_s = 0: the two carried keyframes only -- (0, 1) lerps, (2 -> 1, 1) is keyframe 1 itself; nothing of the recording
    assert (w[0, 4:6] == lerp(keys[0, 4:6], keys[1, 4:6], 0.5)).all() and (w[1, 4:6] == keys[1, 4:6]).all() and not w[2:, 4:6].any()
    after = keep_each(keys, rows, [[1, 0], [2, BIG], [BIG, 3]], counts, steps)
    assert (after[0, 0:2] == keys[1, 0:2]).all() and (after[1, 0:2] == keys[0, 0:2]).all()          # swapped: both read before either is written
    assert (after[0, 2:4] == rows[0, 2:4]).all() and (after[1, 2:4] == rows[1, 2:4]).all()          # 0xFFFFFFFF -> c + 1 = 3
    assert (after[0, 4:6] == keys[1, 4:6]).all() and (after[1, 4:6] == keys[1, 4:6]).all()          # c = 0: both clamp to 1
    # mono and float recordings go through the same unpack as the lockstep test's keyframes
    xf = (x.astype(F32) / F32(40000)).astype(F32)
    mono = rows_each(list(xf), where, None, n, True, 1)
    assert (mono[0, 0] == mono[0, 1]).all() and mono[2, 0, 1] == ((xf[0, 9, 0] + xf[0, 9, 1]) / F32(2) + F32(1)) / F32(2)


def test_the_pool_start_is_the_library_s_rule():
    n, pool_frames = 256, 5001
    spans = [(16, 3000), (16, 3000), (273, 700), (5001, 64), (4900, 90)]           # two on one span, one nested and short, first >= pool_frames, a span below a window
    starts = [[0, 100, 2744, 2745, BIG], [7, 7, 7, 7, 7], [0, 443, 444, 445, BIG], [0, 1, 2, 3, BIG], [0, 50, 51, 52, BIG]]
    got = pool_starts(spans, starts, pool_frames, n)
    assert got.tolist() == [[16, 116, 2760, 2760, 2760], [23] * 5, [273, 716, 717, 717, 717], [4745] * 5, [4745] * 5]
    for (first, frames), row, g in zip(spans, starts, got):
        for e, v in zip(row, g):
            assert v == pool_window_start(first, frames, e, pool_frames, n) and 0 <= v <= pool_frames - n
    rule = strip_comments(read_csrc("glv_frame.h"))
    assert "return first >= last || last - first <= into ? last : first + into;" in function_body(rule, r"uint64_t pool_window_start\(")
