"""CPU: stream slots (glv_batch_reset_streams / _save_streams / _load_streams) -- what can be held without a device: the Python mirror of
glv_stream_state_desc against the header as a C compiler lays it out, the numpy restatement of the blob layout (glava_amd/stream_slots.py, which
tests/test_stream_slots.py indexes blobs with), the exported symbols and their argument checks, and that the three calls are launches only."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from glava_amd import stream_slots as SL
from src_scan import assert_launch_only, function_body, read_csrc, read_host_src, strip_comments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "glv_spectrum.h")
ENTRIES = ["glv_batch_stream_state_desc", "glv_batch_reset_streams", "glv_batch_save_streams", "glv_batch_load_streams"]


def test_python_mirror_of_the_descriptor_has_the_headers_layout(glvlib, tmp_path):
    fields = [f[0] for f in glvlib.StreamStateDesc._fields_]
    assert fields == ["n", "avg_frames", "elem_bytes", "gravity_form", "regions", "kept_bins", "bytes"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "glv_spectrum.h"\nint main(void){ printf("%zu", sizeof(glv_stream_state_desc));\n'
                   + "".join(f'printf(" %zu", offsetof(glv_stream_state_desc, {f}));\n' for f in fields) + "return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == C.sizeof(glvlib.StreamStateDesc) == 32
    assert got[1:] == [getattr(glvlib.StreamStateDesc, f).offset for f in fields]
    body = re.search(r"typedef struct glv_stream_state_desc \{(.*?)\} glv_stream_state_desc;", open(HEADER).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [m for decl in re.findall(r"\b(?:uint32_t|uint64_t)\s+([\w\s,]+);", body) for m in re.split(r"\s*,\s*", decl.strip())]
    assert members == fields, (members, fields)


def test_library_exports_the_entries_and_refuses_null_arguments(glvlib):
    """within ABI 7, detected by the symbol; a NULL batch is an argument error before any device is touched"""
    L = glvlib.lib()
    for name in ENTRIES:
        assert hasattr(L, name), name
    assert L.glv_abi_version() == 7
    d = glvlib.StreamStateDesc()
    assert L.glv_batch_stream_state_desc(None, C.byref(d)) == glvlib.ERR_INVALID
    assert L.glv_batch_reset_streams(None, None, 1, None) == glvlib.ERR_INVALID
    assert L.glv_batch_save_streams(None, None, 1, None, C.byref(d), None) == glvlib.ERR_INVALID
    assert L.glv_batch_load_streams(None, None, 1, None, C.byref(d), None) == glvlib.ERR_INVALID
    assert b"NULL" in L.glv_last_error()
    for method in ("stream_state_desc", "reset_streams", "save_streams", "load_streams"):
        assert callable(getattr(glvlib.Batch, method))


def test_the_three_calls_launch_and_nothing_else():
    """nothing is allocated, nothing copied or awaited: the calls can be captured into a hipGraph"""
    sigs = [rf"\nint {name}\(" for name in ENTRIES] + [r"\nint slots_launch\(", r"\nint slots_check\(", r"\nvoid stream_regions\(", r"\nvoid stream_desc\("]
    src = read_host_src()
    assert_launch_only(src, sigs)
    assert strip_comments(function_body(src, r"\nint slots_launch\(")).count("launch_slots(") == 1
    # ... and the kernel unit is plain loads and stores: no atomics, no LDS, no inline assembly
    kernel = strip_comments(read_csrc("glv_slots.hip"))
    for word in ("atomic", "__shared__", "asm", "__builtin_amdgcn"):
        assert word not in kernel, word
    assert '"glv_slots"' in open(os.path.join(ROOT, "glava_amd", "build.py")).read()


def _desc(n=256, F=5, elem=4, regions=3, form=2):
    return dict(n=n, avg_frames=F, elem_bytes=elem, gravity_form=form, regions=regions, kept_bins=n)


def test_region_offsets_follow_the_order_of_the_header():
    d = _desc(regions=15)
    assert SL.region_offsets(d) == {"gravity": (0, 2048), "average": (2048, 10240), "ring_s16": (12288, 1024), "ring_f32": (13312, 2048)}
    assert SL.stream_bytes(d) == 15360
    assert SL.region_offsets(_desc(elem=2, regions=3)) == {"gravity": (0, 1024), "average": (1024, 5120)}
    assert SL.region_offsets(_desc(regions=SL.REGION_AVERAGE | SL.REGION_RING_F32, F=1)) == {"average": (0, 2048), "ring_f32": (2048, 2048)}
    assert SL.region_offsets(_desc(regions=0)) == {} and SL.stream_bytes(_desc(regions=0)) == 0
    # every region is whole 16-byte pieces at every size the library takes (n >= 256)
    for n in (256, 4096, 32768):
        for elem in (2, 4):
            for at, nbytes in SL.region_offsets(_desc(n=n, F=3, elem=elem, regions=15)).values():
                assert at % 16 == 0 and nbytes % 16 == 0
    with pytest.raises(ValueError):
        SL.region_offsets(_desc(elem=8))
    with pytest.raises(ValueError):
        SL.region_offsets(_desc(regions=16))


def test_the_descriptor_may_be_the_ctypes_mirror(glvlib):
    d = glvlib.StreamStateDesc(n=512, avg_frames=2, elem_bytes=2, gravity_form=1, regions=7, kept_bins=512, bytes=0)
    assert SL.region_offsets(d) == {"gravity": (0, 2048), "average": (2048, 4096), "ring_s16": (6144, 2048)}


def test_split_blob_views_every_region_in_its_type():
    d = _desc(n=256, F=2, elem=2, regions=15)
    blob = (np.arange(SL.stream_bytes(d)) % 251).astype(np.uint8)
    parts = SL.split_blob(d, blob)
    assert [(k, v.dtype, v.shape) for k, v in parts.items()] == [("gravity", np.uint16, (2, 256)), ("average", np.uint16, (2, 2, 256)),
                                                                  ("ring_s16", np.int16, (256, 2)), ("ring_f32", np.float32, (256, 2))]
    assert np.concatenate([v.reshape(-1).view(np.uint8) for v in parts.values()]).tobytes() == blob.tobytes()
    assert parts["average"][1, 0, 0] == blob[1024 + 2 * 512:][:2].view(np.uint16)[0]
    with pytest.raises(ValueError):
        SL.split_blob(d, blob[:-16])


def test_unrotate_puts_the_oldest_entry_first():
    """head is the slot that receives the next frame: the oldest.  A ring of F = 5 slots written round and round, 7 frames in: head = 2, the slots hold
    frames 5 6 2 3 4, and the blob holds 2 3 4 5 6"""
    F, frames = 5, 7
    ring = np.zeros((2, F, 4), np.int64)
    for t in range(frames):
        ring[:, t % F, :] = t
    head = frames % F
    blob = SL.unrotate(ring, head, axis=1)
    assert [int(blob[0, q, 0]) for q in range(F)] == [2, 3, 4, 5, 6]
    assert (np.roll(blob, head, axis=1) == ring).all()
    # a PCM ring of n frames at write position 137: blob frame q is ring frame (137 + q) mod n
    n = 256
    pcm = np.arange(2 * n).reshape(n, 2)
    out = SL.unrotate(pcm, 137)
    for q in (0, 1, 118, 119, 255):
        assert (out[q] == pcm[(137 + q) % n]).all()
    assert (SL.unrotate(pcm, 0) == pcm).all()
    # a blob moves between batches at different positions: the destination keeps it rotated by its own, and reads the same blob back
    assert (SL.unrotate(np.roll(out, 37, axis=0), 37) == out).all()
    with pytest.raises(ValueError):
        SL.unrotate(pcm, n)
